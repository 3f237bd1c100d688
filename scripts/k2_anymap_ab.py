#!/usr/bin/env python3
"""A/B of K2's any-map build (k2_flags bit 29 on a map the vector kernels cannot read) against the fp32 VALU form such maps took before ("k2_exact_auto" 0) and
against the vector build on 640x480, alternating in ONE process; kernel time from the dispatch's own events (dsac_profile_enable), as bench.py takes it.
Also the any-map build on 640x480 through an err buffer 4 bytes off the 16-byte grid (the same cells, only the stores' alignment differs), and the whole call
of dsac_k2_range_census.

    python scripts/k2_anymap_ab.py [--rounds 5] [--reps 20] > profiles/k2_anymap_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANY = 1 << 29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import dsac_amd
    from dsac_amd import synth
    dev = torch.device("cuda", 0)
    eng = dsac_amd.Engine(0)
    print("# device: %s" % eng.device_info())
    print("# K2 kernel time per launch (us), median of %d rounds x %d launches, forms alternating inside every round; err + soft" % (a.rounds, a.reps))

    def timed(frames, N, h, w, forms):
        """forms: [(label, {option: value})]; returns {label: [us per launch of every round]}"""
        P = h * w
        fr = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=True) for f in range(min(frames, 4))]
        xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % len(fr)]["xyz"] for f in range(frames)]))).to(dev)
        if frames > 1:
            eng.set_frames(xyz, None, h, w, fr[0]["cam"], borrow=True)
        else:
            eng.set_frame(xyz[0], None, h, w, fr[0]["cam"], borrow=True)
        poses = torch.from_numpy(synth.random_poses(frames * N, seed=11)).to(dev)
        poses[:, 5] += 2500.0
        err_buf = torch.empty(frames * N * P + 4, dtype=torch.float32, device=dev)
        errs = {0: err_buf[:frames * N * P], 4: err_buf[1:1 + frames * N * P]}  # 16-byte aligned / 4 bytes off
        soft = torch.zeros(frames * N, dtype=torch.float64, device=dev)
        res, names = {l: [] for l, _ in forms}, {}
        for rnd in range(a.rounds + 1):  # round 0 settles
            for label, opts in forms:
                err = errs[opts.get("err_off", 0)]
                for k in ("k2_variant", "k2_flags", "k2_exact_auto"):
                    eng.set_option(k, opts.get(k, {"k2_variant": -1, "k2_flags": 0, "k2_exact_auto": 1}[k]))
                eng.reproject(poses, N=frames * N, err=err, soft=soft)
                eng.synchronize()
                names[label] = eng.k2_form()
                eng.profile_enable(True, stride=1)
                eng.profile_read(0, reset=True)
                for _ in range(a.reps):
                    eng.reproject(poses, N=frames * N, err=err, soft=soft)
                eng.synchronize()
                ms, n = eng.profile_read(0, reset=True)
                eng.profile_enable(False)
                if rnd:
                    res[label].append(ms * 1e3 / n)
        for k, v in (("k2_variant", -1), ("k2_flags", 0), ("k2_exact_auto", 1)):
            eng.set_option(k, v)
        for label, _ in forms:
            v = res[label]
            print("%-16s %3d x %4d x %dx%d  %-52s form %-22s median %8.1f us  (min %8.1f  max %8.1f)  %.3f ns per cell" %
                  ("", frames, N, w, h, label, names[label][0], statistics.median(v), min(v), max(v), statistics.median(v) * 1e3 / (frames * N * P)))
        del err, errs, err_buf, xyz
        torch.cuda.empty_cache()
        return {l: statistics.median(v) for l, v in res.items()}

    odd = [("fp32 VALU fallback (k2_exact_auto 0, the parent's default here)", {"k2_exact_auto": 0}),
           ("any-map exact (bit 29; the default takes the same)", {"k2_flags": ANY})]
    vec = [("vector exact (default)", {}),
           ("any-map exact, err 4 bytes off the 16-byte grid", {"k2_flags": ANY, "err_off": 4}),
           ("fp32 VALU fallback, err 4 bytes off (k2_exact_auto 0)", {"k2_exact_auto": 0, "err_off": 4})]
    for frames in (1, 16):
        print("\n== %d x 256 hypotheses" % frames)
        o = timed(frames, 256, 479, 641, odd)
        v = timed(frames, 256, 480, 640, vec)
        ratio = o[odd[1][0]] / o[odd[0][0]]
        per_cell = (o[odd[1][0]] / (479 * 641)) / (v[vec[0][0]] / (480 * 640))
        print("any-map / fp32 fallback on 641x479: %.3f  (gate: <= 1.73)   any-map per cell / vector exact per cell at 640x480: %.3f  (target: <= 1.2)" % (ratio, per_cell))
        assert ratio <= 1.73, "the any-map build costs more than the precise mode's price over the fast form"

    # the census: 16 x 256 x 640x480
    fr = [synth.chess_like_frame(480, 640, seed=2305 + f) for f in range(4)]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % 4]["xyz"] for f in range(16)]))).to(dev)
    eng.set_frames(xyz, None, 480, 640, fr[0]["cam"], borrow=True)
    poses = synth.random_poses(16 * 256, seed=11)
    eng.k2_census(poses)
    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        r = eng.k2_census(poses)
        t.append((time.perf_counter() - t0) * 1e6)
    print("\ndsac_k2_range_census, 16 x 256 x 640x480, whole call with its upload, two counters back and the synchronisation: median %.1f us (min %.1f), result %s" %
          (statistics.median(t), min(t), r))
    eng.close()


if __name__ == "__main__":
    main()
