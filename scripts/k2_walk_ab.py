#!/usr/bin/env python3
"""A/B of the hypothesis walk of the exact K2 vector builds ("k2_hyp_walk" 1 / 2 / 4) in ONE process (the pattern of scripts/k2_path_ab.py): the walks alternate on
device buffers, the one that goes first rotating; kernel time from the dispatch's own events (dsac_profile_enable), as bench.py takes it.  Shapes: the
benchmark's 16 frames x 256 hypotheses x 640x480 (err + soft, error images only, sums only, the 16-bit images) and one frame of 256 x 640x480, where the
auto policy must report a walk of 1.  Every round also checks that all walks wrote the same bits.

    python scripts/k2_walk_ab.py [--rounds 9] [--reps 20] > profiles/k2_walk_path_ab.txt
    python scripts/k2_walk_ab.py --once --walk K       one bench-shape launch after a settling one (what a counter run profiles)
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WALKS = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--walk", type=int, default=0)
    ap.add_argument("--per-round", action="store_true", help="list every round's mean under each line (which rounds a wide range comes from)")
    a = ap.parse_args()
    import torch
    import dsac_amd
    from dsac_amd import synth
    dev = torch.device("cuda", 0)
    eng = dsac_amd.Engine(0)
    print("# device: %s" % eng.device_info())
    h, w = 480, 640
    P = h * w

    def setup(frames, N):
        fr = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=True) for f in range(min(frames, 4))]
        xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % len(fr)]["xyz"] for f in range(frames)]))).to(dev)
        if frames > 1:
            eng.set_frames(xyz, None, h, w, fr[0]["cam"], borrow=True)
        else:
            eng.set_frame(xyz[0], None, h, w, fr[0]["cam"], borrow=True)
        poses = torch.from_numpy(synth.random_poses(frames * N, seed=11)).to(dev)
        poses[:, 5] += 2500.0
        return xyz, poses

    if a.once:
        keep, poses = setup(16, 256)
        err = torch.empty(16 * 256, P, dtype=torch.float32, device=dev)
        soft = torch.zeros(16 * 256, dtype=torch.float64, device=dev)
        eng.set_option("k2_hyp_walk", a.walk)
        for _ in range(2):
            eng.reproject(poses, N=16 * 256, err=err, soft=soft)
        eng.synchronize()
        print("k2_form %s, k2_hyp_walk %d -> ran %d" % (eng.k2_form(), a.walk, eng.get_option("k2_hyp_walk_last")))
        return 0

    print("# K2 kernel time per launch (us): median (min .. max) over %d rounds of the mean of %d launches (after one settling round), the walks alternating"
          " inside every round, the one that goes first rotating" % (a.rounds, a.reps))
    for frames, N in ((16, 256), (1, 256)):
        keep, poses = setup(frames, N)
        eng.set_option("k2_hyp_walk", 0)
        probe = torch.zeros(frames * N, dtype=torch.float64, device=dev)
        eng.reproject(poses, N=frames * N, err=None, soft=probe)
        eng.synchronize()
        print("%2d x %d x %dx%d: the auto policy runs a walk of %d" % (frames, N, w, h, eng.get_option("k2_hyp_walk_last")), flush=True)
        for what, dt, want_err, want_soft in (("err + soft", torch.float32, True, True), ("error images only", torch.float32, True, False),
                                              ("sums only", torch.float32, False, True), ("binary16 images + soft", torch.float16, True, True),
                                              ("bfloat16 images + soft", torch.bfloat16, True, True)):
            errs = [torch.empty(frames * N, P, dtype=dt, device=dev) if want_err else None for _ in WALKS]
            softs = [torch.zeros(frames * N, dtype=torch.float64, device=dev) if want_soft else None for _ in WALKS]
            res = {k: [] for k in WALKS}
            for rnd in range(a.rounds + 1):  # round 0 settles
                for j in range(len(WALKS)):
                    k = (j + rnd) % len(WALKS)
                    eng.set_option("k2_hyp_walk", WALKS[k])
                    eng.reproject(poses, N=frames * N, err=errs[k], soft=softs[k])
                    eng.synchronize()
                    assert eng.k2_form() == ("exact (vector build)", 0) and eng.get_option("k2_hyp_walk_last") == WALKS[k]
                    eng.profile_enable(True, stride=1)
                    eng.profile_read(0, reset=True)
                    for _ in range(a.reps):
                        eng.reproject(poses, N=frames * N, err=errs[k], soft=softs[k])
                    eng.synchronize()
                    ms, n = eng.profile_read(0, reset=True)
                    eng.profile_enable(False)
                    assert n == a.reps, (n, a.reps)
                    if rnd:
                        res[WALKS[k]].append(ms * 1e3 / n)
                bits = torch.int32 if dt == torch.float32 else torch.int16
                for k in range(1, len(WALKS)):
                    assert not want_err or torch.equal(errs[0].view(bits), errs[k].view(bits)), "walk %d wrote different error images" % WALKS[k]
                    assert not want_soft or torch.equal(softs[0].view(torch.int64), softs[k].view(torch.int64)), "walk %d wrote different sums" % WALKS[k]
            eng.set_option("k2_hyp_walk", 0)
            m1 = statistics.median(res[1])
            print("%2d x %d x %dx%d, %-24s" % (frames, N, w, h, what) + "   ".join("walk %d: %.2f (%.2f .. %.2f)" % (k, statistics.median(v), min(v), max(v)) for k, v in res.items()) +
                  "   walk 2 / 1 %.4f, walk 4 / 1 %.4f, same bits" % (statistics.median(res[2]) / m1, statistics.median(res[4]) / m1), flush=True)
            if a.per_round:
                for k, v in res.items():
                    print("#     walk %d by round: %s" % (k, " ".join("%.1f" % x for x in v)), flush=True)
            del errs, softs
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
