#!/usr/bin/env python3
"""A/B of the two paths of the exact K2 vector builds in ONE process: the default choice per tile (full-tile path wherever a tile is whole) against the
general path for every tile ("k2_flags" bit 30), alternating on device buffers; kernel time from the dispatch's own events (dsac_profile_enable), as bench.py
takes it.  Shapes: the benchmark's 16 frames x 256 hypotheses x 640x480 and one frame of 256 x 640x480; err + soft, error images only, and the 16-bit images.
Every round also checks that the two paths wrote the same bits.

    python scripts/k2_path_ab.py [--rounds 9] [--reps 20] > profiles/k2_waits_path_ab.txt
    python scripts/k2_path_ab.py --once [--general]      one bench-shape launch after a settling one (what a counter run profiles)
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENERAL = 1 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--general", action="store_true")
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
        eng.set_option("k2_flags", GENERAL if a.general else 0)
        for _ in range(2):
            eng.reproject(poses, N=16 * 256, err=err, soft=soft)
        eng.synchronize()
        print("k2_form %s, k2_flags %#x" % (eng.k2_form(), eng.get_option("k2_flags")))
        return 0

    print("# K2 kernel time per launch (us): median (min .. max) over %d rounds of the mean of %d launches (after one settling round), the two paths alternating"
          " inside every round, the side that goes first alternating too" % (a.rounds, a.reps))
    paths = [("default (full-tile path per tile)", 0), ("general path for every tile (k2_flags bit 30)", GENERAL)]
    for frames, N in ((16, 256), (1, 256)):
        keep, poses = setup(frames, N)
        for what, dt, want_soft in (("err + soft", torch.float32, True), ("error images only", torch.float32, False), ("binary16 images + soft", torch.float16, True),
                                    ("bfloat16 images + soft", torch.bfloat16, True)):
            errs = [torch.empty(frames * N, P, dtype=dt, device=dev) for _ in paths]
            softs = [torch.zeros(frames * N, dtype=torch.float64, device=dev) if want_soft else None for _ in paths]
            res = {l: [] for l, _ in paths}
            for rnd in range(a.rounds + 1):  # round 0 settles
                order = list(enumerate(paths))
                for k, (label, flags) in (order if rnd % 2 else order[::-1]):
                    eng.set_option("k2_flags", flags)
                    eng.reproject(poses, N=frames * N, err=errs[k], soft=softs[k])
                    eng.synchronize()
                    assert eng.k2_form() == ("exact (vector build)", 0)
                    eng.profile_enable(True, stride=1)
                    eng.profile_read(0, reset=True)
                    for _ in range(a.reps):
                        eng.reproject(poses, N=frames * N, err=errs[k], soft=softs[k])
                    eng.synchronize()
                    ms, n = eng.profile_read(0, reset=True)
                    eng.profile_enable(False)
                    assert n == a.reps, (n, a.reps)
                    if rnd:
                        res[label].append(ms * 1e3 / n)
                bits = torch.int32 if dt == torch.float32 else torch.int16
                assert torch.equal(errs[0].view(bits), errs[1].view(bits)), "the two paths wrote different error images"
                assert not want_soft or torch.equal(softs[0].view(torch.int64), softs[1].view(torch.int64)), "the two paths wrote different sums"
            eng.set_option("k2_flags", 0)
            print("%2d x %d x %dx%d, %-24s" % (frames, N, w, h, what) + "   ".join("%s: %.2f (%.2f .. %.2f)" % (l, statistics.median(v), min(v), max(v)) for l, v in res.items()) +
                  "   default / general %.4f, same bits" % (statistics.median(res[paths[0][0]]) / statistics.median(res[paths[1][0]])), flush=True)
            del errs, softs
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
