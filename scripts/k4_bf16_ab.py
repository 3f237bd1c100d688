#!/usr/bin/env python3
"""A/B of K4 on bfloat16 gradient images (dsac_score_backward_bf16) against the binary16 call and the float call, four cases alternating in ONE process on
device buffers:

    (a) the float call on float32 gradient images
    (b) the bfloat16 path without dsac_score_backward_bf16: torch's .float() of the bfloat16 images, then the float call
    (c) the binary16 call on binary16 images
    (d) the bfloat16 call on the bfloat16 images

Two times per case: the K4 main pass from the profile scope (dsac_profile_read which = 1: events around the main-pass launch) and the whole -- conversion where
there is one, main pass and finish kernel -- from a pair of stream events around the repetitions.  Shapes (those of scripts/k4_f16_ab.py): K4's own
256 x 640x480, and the score-model seam's batch of 16 frames x 128 x 40x40.  Every round also checks that (d) returns (a)'s gradient on the same values
(zeroed buffers, last bit of the fp64 atomics).

What must hold, and fails the run (exit status 1, after everything is printed) when it does not, at both shapes: (d)'s main pass <= 1.05 x (c)'s -- equal
bytes, one widening instruction per pair either way --, and (d)'s whole < (b)'s whole.

    python scripts/k4_bf16_ab.py [--rounds 5] [--reps 20] > profiles/k4_bf16_ab.txt
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
    torch.cuda.set_device(dev)
    eng = dsac_amd.Engine(0, stream=torch.cuda.current_stream(dev))  # torch's conversion and K4 on one stream, ordered by it alone
    print("# device: %s" % eng.device_info())
    print("# time per call (us): median over %d rounds of the mean of %d calls (after one settling round), the four cases alternating inside every round" % (a.rounds, a.reps))
    print("# main pass = dsac_profile_read(which = 1); whole = stream events around the calls (conversion where there is one + main pass + finish kernel)")
    cases = ["(a) float call on float images", "(b) torch .float() of the bfloat16 images + float call", "(c) binary16 call on binary16 images",
             "(d) bfloat16 call on the bfloat16 images"]

    def timed(frames, N, h, w, sampled):
        P = h * w
        fr = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=not sampled) for f in range(min(frames, 4))]
        xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % len(fr)]["xyz"] for f in range(frames)]))).to(dev)
        uv = torch.from_numpy(fr[0]["uv"]).to(dev) if sampled else None
        if frames > 1:
            eng.set_frames(xyz, uv, h, w, fr[0]["cam"], borrow=True)
        else:
            eng.set_frame(xyz[0], uv, h, w, fr[0]["cam"], borrow=True)
        T = frames * N
        poses = torch.from_numpy(synth.random_poses(T, seed=11)).to(dev)
        poses[:, 5] += 2500.0
        rng = np.random.default_rng(3)
        sets = torch.from_numpy(np.stack([rng.permutation(P)[:4 * N].reshape(N, 4) for _ in range(frames)]).reshape(T, 4).astype(np.int32)).to(dev)
        dpnp = torch.from_numpy(rng.standard_normal((T, 6, 12)) * 1e-3).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        dbf = (torch.randn(T, P, generator=gen, device=dev) * 1e-3).to(torch.bfloat16)
        d32 = dbf.float()
        d16 = d32.to(torch.float16)
        grad = torch.zeros(frames * P, 3, dtype=torch.float64, device=dev)

        def call(case):
            if case == 0:
                eng.dScore(poses, sets, d32, dpnp=dpnp, grad=grad)
            elif case == 1:
                eng.dScore(poses, sets, dbf.float(), dpnp=dpnp, grad=grad)
            elif case == 2:
                eng.dScore(poses, sets, d16, dpnp=dpnp, grad=grad)
            else:
                eng.dScore(poses, sets, dbf, dpnp=dpnp, grad=grad)

        main_us, whole_us = {c: [] for c in cases}, {c: [] for c in cases}
        first = {}
        for rnd in range(a.rounds + 1):  # round 0 settles
            for ci, label in enumerate(cases):
                grad.zero_()
                call(ci)
                eng.synchronize()
                if ci in (0, 3):
                    first[ci] = grad.clone()
                eng.profile_enable(True, stride=1)
                eng.profile_read(1, reset=True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call(ci)
                e1.record()
                e1.synchronize()
                ms, n = eng.profile_read(1, reset=True)
                eng.profile_enable(False)
                assert n == a.reps, (n, a.reps)
                if rnd:
                    main_us[label].append(ms * 1e3 / n)
                    whole_us[label].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            scale = float(first[0].abs().max())
            diff = float((first[3] - first[0]).abs().max())
            assert scale > 0 and diff <= 1e-12 * scale, (diff, scale)
        med = {}
        for label in cases:
            med[label] = (statistics.median(main_us[label]), statistics.median(whole_us[label]))
            print("%3d x %4d x %dx%d  %-56s main pass median %8.1f us (min %8.1f max %8.1f)   whole median %8.1f us (min %8.1f max %8.1f)" %
                  (frames, N, w, h, label, med[label][0], min(main_us[label]), max(main_us[label]), med[label][1], min(whole_us[label]), max(whole_us[label])))
        (am, aw), (bm, bw), (cm, cw), (dm, dw) = (med[c] for c in cases)
        print("%s (d) / (c): main pass %.3f, whole %.3f     (d) / (a): main pass %.3f, whole %.3f     (d) / (b): whole %.3f     the conversion pass of (b): %.1f us on top of (a)'s whole" %
              (" " * 22, dm / cm, dw / cw, dm / am, dw / aw, dw / bw, bw - aw))
        broken = []
        if dm > 1.05 * cm:
            broken.append("%d x %d x %dx%d: (d) main pass %.1f us > 1.05 x (c) %.1f us" % (frames, N, w, h, dm, cm))
        if not dw < bw:
            broken.append("%d x %d x %dx%d: (d) whole %.1f us is not below (b) whole %.1f us" % (frames, N, w, h, dw, bw))
        del d16, d32, dbf, grad, xyz
        torch.cuda.empty_cache()
        return broken

    broken = []
    for frames, N, h, w, sampled in ((1, 256, 480, 640, False), (16, 128, 40, 40, True)):
        print("\n== %d frame(s) x %d hypotheses on %dx%d, %s" % (frames, N, w, h, "sampled pixel positions" if sampled else "implicit pixel grid"))
        broken += timed(frames, N, h, w, sampled)
    eng.close()
    print("\nbounds: %s" % ("all hold" if not broken else "BROKEN"))
    for b in broken:
        print("  " + b)
    if broken:
        sys.exit(1)


if __name__ == "__main__":
    main()
