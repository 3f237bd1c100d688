#!/usr/bin/env python3
"""A/B of the two forms of dsac_refine_soft (split: pass + step launches; fused: one launch), its backward, and two yardsticks, the cases alternating in ONE
process on device buffers:

    shapes   640 x 480 x B = 256;   16 frames x 256 x 40 x 40;   80 x 60 x B = 64 and B = 1
    per shape: the whole call (max_iters = 20, step_tol = 1e-6) in both forms; a call with max_iters = 1 (two passes, two steps) as the time per pass;
               dsac_refine_soft_backward;  dsac_refine_all on the same problems;  the same (problem, cell) pair count through K2's soft-only form
    crossover: both forms at B = 64 and B = 1 on maps of 1 600 .. 76 800 cells: the largest map on which the fused form is not slower is what the auto constant
               (SOFT_FUSED_MAX_CELLS, k_refine.hip) is set from

Start poses are the ground truth displaced by 0.03 rad / 40 mm.  Times are stream events around the repetitions.  Nothing is asserted: the issue fixes no time.

    python scripts/refine_soft_ab.py [--rounds 3] [--reps 5] > profiles/refine_soft_ab.txt
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
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
    TAU, BETA, CUT, MIN_SOFT, STEPS = 10.0, 0.5, 42.0, 50.0, 8
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rng = np.random.default_rng(3)

    def shape(H, W, B, frames=1):
        """Device buffers of one shape: `frames` copies of one synthetic frame, B problems per frame."""
        fr = synth.chess_like_frame(H, W, seed=1305)
        n = B * frames
        poses = fr["gt_pose"] + np.concatenate([rng.normal(scale=0.03, size=(n, 3)), rng.normal(scale=40.0, size=(n, 3))], 1)
        xyz = t(fr["xyz"]) if frames == 1 else t(fr["xyz"]).unsqueeze(0).repeat(frames, 1, 1).contiguous()
        f64 = dict(dtype=torch.float64, device=dev)
        return dict(H=H, W=W, P=H * W, B=n, frames=frames, cam=fr["cam"], xyz=xyz, uv=t(fr["uv"]), poses=t(poses), out=torch.zeros(n, 6, **f64), soft=torch.zeros(n, **f64),
                    it=torch.zeros(n, dtype=torch.int32, device=dev), st=torch.zeros(n, dtype=torch.int32, device=dev), dL=t(rng.normal(size=(n, 6))),
                    grad=torch.zeros(frames * H * W, 3, **f64), ok=torch.zeros(n, dtype=torch.int32, device=dev), perm=t(synth.fast_permutations(H * W, STEPS)),
                    sd=torch.zeros(n, dtype=torch.int32, device=dev))

    def set_shape(s):
        if s["frames"] > 1:
            eng.set_frames(s["xyz"], s["uv"], s["H"], s["W"], s["cam"], borrow=True)
        else:
            eng.set_frame(s["xyz"], s["uv"], s["H"], s["W"], s["cam"], borrow=True)

    def soft(s, form, max_iters):
        eng.set_option("refine_soft_form", form)
        check(eng._ctx, lib.dsac_refine_soft(eng._ctx, s["B"], ptr(s["poses"]), None, TAU, BETA, CUT, MIN_SOFT, max_iters, 1e-6, ptr(s["out"]), ptr(s["soft"]), ptr(s["it"]),
                                             ptr(s["st"])))

    def bwd(s):
        check(eng._ctx, lib.dsac_refine_soft_backward(eng._ctx, s["B"], ptr(s["out"]), None, TAU, BETA, CUT, MIN_SOFT, ptr(s["dL"]), None, 0, ptr(s["grad"]), ptr(s["ok"])))

    def walk(s):
        check(eng._ctx, lib.dsac_refine_all(eng._ctx, s["B"], ptr(s["poses"]), ptr(s["perm"]), STEPS, 100, 50, 10.0, None, ptr(s["out"]), None, ptr(s["sd"])))

    def k2(s):
        check(eng._ctx, lib.dsac_reproject(eng._ctx, s["B"], ptr(s["poses"]), 100.0, None, TAU, BETA, ptr(s["soft"])))

    def measure(cases):
        """cases: (label, shape, call).  Returns label -> median us."""
        us = {c[0]: [] for c in cases}
        current = None
        for rnd in range(a.rounds + 1):  # round 0 settles
            for label, s, call in cases:
                if s is not current:  # outside the timed region
                    set_shape(s)
                    current = s
                call(s)
                eng.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call(s)
                e1.record()
                e1.synchronize()
                if rnd:
                    us[label].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}

    shapes = [("640 x 480 x 256", shape(480, 640, 256)), ("16 frames x 256 x 40 x 40", shape(40, 40, 256, 16)), ("80 x 60 x 64", shape(60, 80, 64)),
              ("80 x 60 x 1", shape(60, 80, 1))]
    for name, s in shapes:
        cases = [("split, whole call", s, lambda s: soft(s, 0, 20)), ("fused, whole call", s, lambda s: soft(s, 1, 20)),
                 ("split, max_iters 1", s, lambda s: soft(s, 0, 1)), ("fused, max_iters 1", s, lambda s: soft(s, 1, 1))]
        if s["frames"] == 1:  # the yardsticks: K6's walk on the same start poses, K2's soft-only form on the same pair count
            cases += [("dsac_refine_all (8 steps, max_inl 100)", s, walk)]
            if s["B"] % 128 == 0:
                cases += [("dsac_reproject, soft only", s, k2)]
        if s["P"] > 100000:  # the fused form walks a big map with one workgroup per problem: once is enough to show it
            cases = [c for c in cases if c[0] != "fused, whole call"]
        res = measure(cases)
        set_shape(s)
        soft(s, 0, 20)  # the refined poses the backward is timed at
        eng.synchronize()
        res.update(measure([("backward", s, bwd)]))
        iters = s["it"].cpu().numpy()
        status = np.bincount(s["st"].cpu().numpy(), minlength=6)
        print("\n## %s   (accepted steps: mean %.1f, max %d; statuses CONVERGED %d MAXIT %d SCORE %d FEW %d SINGULAR %d NONFINITE %d; backward ok %d of %d)" %
              ((name, iters.mean(), iters.max()) + tuple(status[:6]) + (int(s["ok"].sum()), s["B"])))
        for label, (med, lo, hi) in res.items():
            extra = "   per pass %.1f us" % (med / 2) if "max_iters 1" in label else ""
            print("%-44s median %10.1f us (min %10.1f max %10.1f)%s" % (label, med, lo, hi, extra))
    print("\n## crossover of the forms (whole call, max_iters 20)")
    best = {}
    for B in (64, 1):
        for H, W in ((40, 40), (60, 80), (96, 128), (120, 160), (240, 320)):
            s = shape(H, W, B)
            r = measure([("split", s, lambda s: soft(s, 0, 20)), ("fused", s, lambda s: soft(s, 1, 20))])
            print("B %3d  %3d x %3d = %6d cells   split %9.1f us   fused %9.1f us   %s" % (B, H, W, H * W, r["split"][0], r["fused"][0],
                                                                                        "fused" if r["fused"][0] <= r["split"][0] else "split"))
            if r["fused"][0] <= r["split"][0]:
                best[B] = max(best.get(B, 0), H * W)
    print("largest map on which the fused form is not slower: %s" % ", ".join("B = %d: %d cells" % (B, c) for B, c in best.items()))
    eng.set_option("refine_soft_form", -1)
    eng.close()


if __name__ == "__main__":
    main()
