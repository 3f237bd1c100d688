#!/usr/bin/env python3
"""A/B of the two ways path I of the DSAC trainer differentiates the refinement, cases alternating in ONE process on device buffers, 640 x 480, max_inl = 100:

    (a) dsac_refine_fd_sets at M = 32: the finite differences (18 + 6 cap replicas per hypothesis, every replica a whole 8-step refinement), with the cap
        Engine.backwardDSAC chooses (the largest inlier count of the 32 maps over skip = 100)
    (b) dsac_refine_gn_backward at B = 32: the Gauss-Newton linearisation, gradient accumulated into grad_xyz
    (c) the same at B = 256
    (d) the same on a batch of 16 frames x 256

The hypotheses are K1's on a synthetic frame (256 of them, refined by dsac_refine_all); (a) and (b) take the 32 with the largest softmax weight -- the trainer
differentiates the hypotheses that carry weight --, (c) and (d) all 256, poses whose walk crosses the whole map included.  Times are stream events around the
repetitions.  The run fails (exit status 1, after everything is printed) only if (b) is not faster than (a).

    python scripts/refine_gn_ab.py [--rounds 5] [--reps 10] > profiles/refine_gn_ab.txt
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
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import dsac_amd
    from dsac_amd import synth
    from dsac_amd.capi import check, lib, ptr
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = dsac_amd.Engine(0, stream=torch.cuda.current_stream(dev))
    print("# device: %s" % eng.device_info())
    print("# time per call (us): median over %d rounds of the mean of %d calls (after one settling round), the cases alternating inside every round; stream events" %
          (a.rounds, a.reps))
    H, W, N, M, FR, MAX_INL, MIN_INL, THR, STEPS = 480, 640, 256, 32, 16, 100, 50, 10.0, 8
    P = H * W
    fr = synth.chess_like_frame(H, W, seed=1305)
    perm = synth.fast_permutations(P, STEPS)
    gt = synth.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0]))
    eng.set_frame(fr["xyz"], fr["uv"], H, W, fr["cam"])
    # the forward pass the trainer would have run: K1, soft-inlier scores, softmax, the refinement of every hypothesis, the loss gradients
    poses, sets, ok = eng.sample(N, seed=1305, thr=THR)
    soft = np.zeros(N)
    eng.reproject(poses, soft=soft)
    w, _, _ = eng.softMax(soft, 0.1)
    ref, steps_done = eng.refineAll(poses, perm, sets=sets, max_inl=MAX_INL, min_inl=MIN_INL, thr=THR)
    dL = eng.maxLossBatch(ref, gt, want_grad=True)["grad"]
    top = np.sort(np.argsort(-w)[:M])
    _, _, maps = eng.refineAll(poses[top], perm, sets=sets[top], max_inl=MAX_INL, min_inl=MIN_INL, thr=THR, want_inlier_maps=True)
    skip = max(1, int(1 / np.float32(0.01)))
    cap = max(1, int((maps != 0).sum(1).max()) // skip)
    rows = np.maximum(steps_done.astype(np.int64) - 1, 0).astype(np.int32)
    print("# %d hypotheses sampled; the %d of largest weight: weights %.2e .. %.2e, inlier cells per map %d .. %d, cap = %d (skip %d): %d replicas per call of (a)" %
          (N, M, w[top].min(), w[top].max(), (maps != 0).sum(1).min(), (maps != 0).sum(1).max(), cap, skip, M * (18 + 6 * cap)))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_perm = t(perm)
    fd = dict(sets=t(sets[top]), maps=t(maps), J_set=torch.zeros(M, 54, dtype=torch.float64, device=dev), px=torch.zeros(M, cap, dtype=torch.int32, device=dev),
              J_obj=torch.zeros(M, cap, 18, dtype=torch.float64, device=dev), n=torch.zeros(M, dtype=torch.int32, device=dev))
    del maps

    def gn_args(idx, frames):
        B = len(idx) * frames
        tile = lambda x: t(np.concatenate([x[idx]] * frames))
        return dict(B=B, ref=tile(ref), rows=tile(rows), dL=tile(dL), coef=tile(w), grad=torch.zeros(frames * P, 3, dtype=torch.float64, device=dev),
                    n=torch.zeros(B, dtype=torch.int32, device=dev))

    g32, g256, g16 = gn_args(top, 1), gn_args(np.arange(N), 1), gn_args(np.arange(N), FR)
    xyz16 = t(fr["xyz"]).unsqueeze(0).repeat(FR, 1, 1).contiguous()
    d_xyz, d_uv = t(fr["xyz"]), t(fr["uv"])

    def call_fd():
        check(eng._ctx, lib.dsac_refine_fd_sets(eng._ctx, M, ptr(fd["sets"]), ptr(d_perm), STEPS, MAX_INL, MIN_INL, THR, ptr(fd["maps"]), 0.01, 2.0, ptr(fd["J_set"]),
                                                ptr(fd["px"]), ptr(fd["J_obj"]), cap, ptr(fd["n"])))

    def call_gn(g):
        check(eng._ctx, lib.dsac_refine_gn_backward(eng._ctx, g["B"], ptr(g["ref"]), None, ptr(d_perm), STEPS, ptr(g["rows"]), MAX_INL, MIN_INL, THR, ptr(g["dL"]),
                                                    ptr(g["coef"]), ptr(g["grad"]), None, None, ptr(g["n"])))

    cases = [("(a) dsac_refine_fd_sets       M = %d, cap = %d" % (M, cap), 1, call_fd), ("(b) dsac_refine_gn_backward   B = %d" % M, 1, lambda: call_gn(g32)),
             ("(c) dsac_refine_gn_backward   B = %d" % N, 1, lambda: call_gn(g256)), ("(d) dsac_refine_gn_backward   %d frames x %d" % (FR, N), FR, lambda: call_gn(g16))]
    us = {c[0]: [] for c in cases}
    frames_set = 0
    for rnd in range(a.rounds + 1):  # round 0 settles
        for label, frames, call in cases:
            if frames != frames_set:  # outside the timed region
                if frames > 1:
                    eng.set_frames(xyz16, d_uv, H, W, fr["cam"], borrow=True)
                else:
                    eng.set_frame(d_xyz, d_uv, H, W, fr["cam"], borrow=True)
                frames_set = frames
            call()
            eng.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            e1.synchronize()
            if rnd:
                us[label].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    med = {}
    for label, _, _ in cases:
        med[label] = statistics.median(us[label])
        print("%-52s median %10.1f us (min %10.1f max %10.1f)" % (label, med[label], min(us[label]), max(us[label])))
    ta, tb, tc, td = (med[c[0]] for c in cases)
    print("problems with a result: (b) %d of %d, (c) %d of %d, (d) %d of %d; finite-difference cells per hypothesis in (a): %d .. %d" %
          (int((g32["n"] > 0).sum()), M, int((g256["n"] > 0).sum()), N, int((g16["n"] > 0).sum()), FR * N, int(fd["n"].min()), int(fd["n"].max())))
    print("(a) / (b) = %.1f     (c) / (b) = %.2f for 8 x the problems     (d) per frame = %.1f us" % (ta / tb, tc / tb, td / FR))
    eng.close()
    if not tb < ta:
        print("BROKEN: (b) %.1f us is not faster than (a) %.1f us" % (tb, ta))
        sys.exit(1)
    print("bound: holds ((b) is faster than (a))")


if __name__ == "__main__":
    main()
