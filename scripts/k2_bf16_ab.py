#!/usr/bin/env python3
"""A/B of K2's bfloat16 error images (dsac_reproject_bf16) against the binary16 call (dsac_reproject_f16) and the float call, alternating in ONE process on
device buffers; kernel time from the dispatch's own events (dsac_profile_enable), as bench.py takes it.  Both store layouts of "k2_f16_store" for both 16-bit
types.  Shapes (those of scripts/k2_f16_ab.py): the benchmark's 16 frames x 256 hypotheses x 640x480, one frame of 256 x 640x480, and 256 x 40x40; err + soft,
and error images only.  Every round also checks that the 16-bit images are the rounded floats.

What must hold, and fails the run (exit status 1, after everything is printed) when it does not: at every shape and in either layout the bfloat16 call is not
above 1.05 x the binary16 call beside it (equal bytes, one conversion instruction per pair either way), and at the bench shape it is below the float call.

    python scripts/k2_bf16_ab.py [--rounds 5] [--reps 20] > profiles/k2_bf16_ab.txt
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
    print("# K2 kernel time per launch (us): median over %d rounds of the mean of %d launches (after one settling round), the five calls alternating inside"
          " every round" % (a.rounds, a.reps))
    forms = [("float     (dsac_reproject)", torch.float32, 0), ("binary16, 16-byte stores  (k2_f16_store 1)", torch.float16, 1),
             ("bfloat16, 16-byte stores  (k2_f16_store 1)", torch.bfloat16, 1), ("binary16,  8-byte stores  (k2_f16_store 0)", torch.float16, 0),
             ("bfloat16,  8-byte stores  (k2_f16_store 0)", torch.bfloat16, 0)]

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
        errs = {dt: torch.empty(frames * N, P, dtype=dt, device=dev) for dt in (torch.float32, torch.float16, torch.bfloat16)}
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
                if dt != torch.float32:  # the float call ran first in this round: its images are the reference
                    rows = slice(0, min(frames * N, 512))
                    assert torch.equal(errs[dt][rows].view(torch.int16), errs[torch.float32][rows].to(dt).view(torch.int16)), label
        eng.set_option("k2_f16_store", 1)  # the default
        med = {}
        for label, dt, _ in forms:
            v = res[label]
            med[label] = statistics.median(v)
            gb = frames * N * P * (4 if dt == torch.float32 else 2) / 1e9
            print("%3d x %4d x %dx%d  %-9s %-44s median %8.1f us  (min %8.1f  max %8.1f)  %6.2f GB of images, %5.2f TB/s" %
                  (frames, N, w, h, "err+soft" if want_soft else "err only", label, med[label], min(v), max(v), gb, gb / med[label] * 1e3))
        f32, h1, b1, h0, b0 = (med[l] for l, _, _ in forms)
        print("%s bfloat16 / binary16: 16-byte stores %.3f, 8-byte stores %.3f     bfloat16 / float: %.3f, %.3f" % (" " * 28, b1 / h1, b0 / h0, b1 / f32, b0 / f32))
        shape = "%d x %d x %dx%d %s" % (frames, N, w, h, "err+soft" if want_soft else "err only")
        broken = []
        for name, b, hh in (("16-byte stores", b1, h1), ("8-byte stores", b0, h0)):
            if b > 1.05 * hh:
                broken.append("%s, %s: bfloat16 %.1f us > 1.05 x binary16 %.1f us" % (shape, name, b, hh))
        if frames > 1 and not b1 < f32:
            broken.append("%s: bfloat16 %.1f us is not below the float call %.1f us" % (shape, b1, f32))
        del errs, xyz
        torch.cuda.empty_cache()
        return broken

    broken = []
    for frames, N, h, w in ((16, 256, 480, 640), (1, 256, 480, 640), (1, 256, 40, 40)):
        for want_soft in (True, False):
            print("\n== %d x %d hypotheses on %dx%d, %s" % (frames, N, w, h, "err + soft" if want_soft else "error images only"))
            broken += timed(frames, N, h, w, want_soft)
    eng.close()
    print("\nbounds: %s" % ("all hold" if not broken else "BROKEN"))
    for b in broken:
        print("  " + b)
    if broken:
        sys.exit(1)


if __name__ == "__main__":
    main()
