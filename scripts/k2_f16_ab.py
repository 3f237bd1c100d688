#!/usr/bin/env python3
"""A/B of K2's half-precision error images (dsac_reproject_f16, both store layouts of "k2_f16_store") against the float call, alternating in ONE process on
device buffers; kernel time from the dispatch's own events (dsac_profile_enable), as bench.py takes it.  Shapes: the benchmark's 16 frames x 256 hypotheses
x 640x480, one frame of 256 x 640x480, and 256 x 40x40.  Err + soft, and error images only.  Every round also checks that the halves are the rounded floats.

    python scripts/k2_f16_ab.py [--rounds 5] [--reps 20] > profiles/k2_f16_ab.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    print("# K2 kernel time per launch (us): median over %d rounds of the mean of %d launches (after one settling round), the three calls alternating inside"
          " every round" % (a.rounds, a.reps))
    forms = [("float  (dsac_reproject)", torch.float32, 0), ("half, 8-byte stores  (k2_f16_store 0)", torch.float16, 0),
             ("half, 16-byte stores after a lane exchange  (k2_f16_store 1)", torch.float16, 1)]

    def timed(frames, N, h, w, want_soft):
        P = h * w
        fr = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=True) for f in range(min(frames, 4))]
        xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % len(fr)]["xyz"] for f in range(frames)]))).to(dev)
        if frames > 1:
            eng.set_frames(xyz, None, h, w, fr[0]["cam"], borrow=True)
        else:
            eng.set_frame(xyz[0], None, h, w, fr[0]["cam"], borrow=True)
        poses = torch.from_numpy(synth.random_poses(frames * N, seed=11)).to(dev)
        poses[:, 5] += 2500.0
        errs = {torch.float32: torch.empty(frames * N, P, dtype=torch.float32, device=dev), torch.float16: torch.empty(frames * N, P, dtype=torch.float16, device=dev)}
        soft = torch.zeros(frames * N, dtype=torch.float64, device=dev) if want_soft else None
        res = {l: [] for l, _, _ in forms}
        for rnd in range(a.rounds + 1):  # round 0 settles
            for label, dt, layout in forms:
                eng.set_option("k2_f16_store", layout)
                eng.reproject(poses, N=frames * N, err=errs[dt], soft=soft)
                eng.synchronize()
                assert eng.k2_form() == ("exact (vector build)", 0)
                eng.profile_enable(True, stride=1)
                eng.profile_read(0, reset=True)
                for _ in range(a.reps):
                    eng.reproject(poses, N=frames * N, err=errs[dt], soft=soft)
                eng.synchronize()
                ms, n = eng.profile_read(0, reset=True)
                eng.profile_enable(False)
                if rnd:
                    res[label].append(ms * 1e3 / n)
                if dt == torch.float16:  # the float call ran first in this round: its images are the reference
                    rows = slice(0, min(frames * N, 512))
                    assert torch.equal(errs[dt][rows].view(torch.int16), errs[torch.float32][rows].to(torch.float16).view(torch.int16)), label
        eng.set_option("k2_f16_store", 1)  # the default
        med = {}
        for label, dt, _ in forms:
            v = res[label]
            med[label] = statistics.median(v)
            gb = frames * N * P * (4 if dt == torch.float32 else 2) / 1e9
            print("%3d x %4d x %dx%d  %-9s %-62s median %8.1f us  (min %8.1f  max %8.1f)  %6.2f GB of images, %5.2f TB/s" %
                  (frames, N, w, h, "err+soft" if want_soft else "err only", label, med[label], min(v), max(v), gb, gb / med[label] * 1e3))
        base = med[forms[0][0]]
        print("%s half / float: 8-byte stores %.3f, 16-byte stores %.3f" % (" " * 28, med[forms[1][0]] / base, med[forms[2][0]] / base))
        del errs, xyz
        torch.cuda.empty_cache()
        return med

    for frames, N, h, w in ((16, 256, 480, 640), (1, 256, 480, 640), (1, 256, 40, 40)):
        for want_soft in (True, False):
            print("\n== %d x %d hypotheses on %dx%d, %s" % (frames, N, w, h, "err + soft" if want_soft else "error images only"))
            timed(frames, N, h, w, want_soft)
    eng.close()


if __name__ == "__main__":
    main()
