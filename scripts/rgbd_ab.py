#!/usr/bin/env python3
"""A/B of the RGB-D calls against their RGB twins, the cases alternating in ONE process on device buffers:

    (a) dsac_score_rgbd (err + soft, and err only) against dsac_reproject on its default form, on the same frames and poses:
        16 x 256 x 640x480 (the bench shape), 1 x 256 x 640x480, 256 x 40x40 -- times, achieved store bandwidth, ratio.
        EXIT STATUS 1 if the RGB-D kernel exceeds 1.05 x dsac_reproject's time at the bench shape (err + soft): the bytes stored are the same and the
        arithmetic is less, so slower means the store schedule was lost.  5 % is the margin this project's A/B scripts use against their own repeat spread.
    (b) dsac_sample_rgbd against dsac_sample at 1 x 256, 1 x 4096, 16 x 256 (640x480).  Report only.
    (c) dsac_refine_rgbd against dsac_refine_soft (split form) at 16 x 256 x 40x40 and 256 x 640x480, whole calls and max_iters = 1.  Report only.

Times are stream events around the repetitions.

    python scripts/rgbd_ab.py [--rounds 3] [--reps 5] > profiles/rgbd_ab.txt
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
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rng = np.random.default_rng(3)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)

    def shape(H, W, N, frames=1, with_err=True):
        """`frames` copies of one synthetic RGB-D frame, N hypotheses / problems per frame: start poses = the ground truth displaced by 0.03 rad / 40 mm"""
        fr = synth.chess_like_frame_rgbd(H, W, seed=1305)
        n = N * frames
        poses = fr["gt_pose"] + np.concatenate([rng.normal(scale=0.03, size=(n, 3)), rng.normal(scale=40.0, size=(n, 3))], 1)
        rep = lambda x: t(x) if frames == 1 else t(x).unsqueeze(0).repeat(frames, 1, 1).contiguous()
        return dict(H=H, W=W, P=H * W, N=n, frames=frames, cam=fr["cam"], xyz=rep(fr["xyz"]), uv=t(fr["uv"]), pts=rep(fr["cam_xyz"]), poses=t(poses),
                    err=torch.empty(n, H * W, dtype=torch.float32, device=dev) if with_err else None, soft=torch.zeros(n, **f64), out=torch.zeros(n, 6, **f64),
                    it=torch.zeros(n, **i32), st=torch.zeros(n, **i32), hyps=torch.zeros(n, 6, **f64), sets=torch.zeros(n, 4, **i32),
                    ok=torch.zeros(n, dtype=torch.uint8, device=dev))

    def set_shape(s):
        if s["frames"] > 1:
            eng.set_frames(s["xyz"], s["uv"], s["H"], s["W"], s["cam"], borrow=True)
        else:
            eng.set_frame(s["xyz"], s["uv"], s["H"], s["W"], s["cam"], borrow=True)
        eng.set_camera_points(s["pts"])

    ctx = eng._ctx
    score_rgbd = lambda s, err, soft: check(ctx, lib.dsac_score_rgbd(ctx, s["N"], ptr(s["poses"]), 1000.0, ptr(s["err"]) if err else None, 100.0, 0.05, ptr(s["soft"]) if soft else None))
    score_rgb = lambda s, err, soft: check(ctx, lib.dsac_reproject(ctx, s["N"], ptr(s["poses"]), 100.0, ptr(s["err"]) if err else None, 10.0, 0.5, ptr(s["soft"]) if soft else None))
    sample_rgbd = lambda s: check(ctx, lib.dsac_sample_rgbd(ctx, s["N"], 1305, None, 100.0, 1 << 20, ptr(s["hyps"]), ptr(s["sets"]), ptr(s["ok"])))
    sample_rgb = lambda s: check(ctx, lib.dsac_sample(ctx, s["N"], 1305, None, 10.0, 1 << 20, ptr(s["hyps"]), ptr(s["sets"]), ptr(s["ok"])))

    def refine_rgbd(s, iters):
        check(ctx, lib.dsac_refine_rgbd(ctx, s["N"], ptr(s["poses"]), None, 100.0, 0.05, 100.0, 50.0, iters, 1e-6, ptr(s["out"]), ptr(s["soft"]), ptr(s["it"]), ptr(s["st"])))

    def refine_rgb(s, iters):
        eng.set_option("refine_soft_form", 0)
        check(ctx, lib.dsac_refine_soft(ctx, s["N"], ptr(s["poses"]), None, 10.0, 0.5, 42.0, 50.0, iters, 1e-6, ptr(s["out"]), ptr(s["soft"]), ptr(s["it"]), ptr(s["st"])))

    def measure(s, cases):
        """cases: (label, call).  Returns label -> (median, min, max) us."""
        us = {c[0]: [] for c in cases}
        set_shape(s)
        for rnd in range(a.rounds + 1):  # round 0 settles
            for label, call in cases:
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

    def show(res, bytes_stored=None):
        for label, (med, lo, hi) in res.items():
            bw = "   %.2f TB/s stored" % (bytes_stored / med * 1e-6) if bytes_stored and "err" in label else ""
            print("%-44s median %10.1f us (min %10.1f max %10.1f)%s" % (label, med, lo, hi, bw))

    failed = False
    print("\n# (a) scoring: dsac_score_rgbd against dsac_reproject (default form: k2_form_last below)")
    for name, H, W, N, F, bench in (("16 x 256 x 640x480 (bench shape)", 480, 640, 256, 16, True), ("1 x 256 x 640x480", 480, 640, 256, 1, False), ("256 x 40x40", 40, 40, 256, 1, False)):
        s = shape(H, W, N, F)
        res = measure(s, [("rgbd  err + soft", lambda s: score_rgbd(s, True, True)), ("rgb   err + soft", lambda s: score_rgb(s, True, True)),
                          ("rgbd  err only", lambda s: score_rgbd(s, True, False)), ("rgb   err only", lambda s: score_rgb(s, True, False)),
                          ("rgbd  soft only", lambda s: score_rgbd(s, False, True)), ("rgb   soft only", lambda s: score_rgb(s, False, True))])
        print("\n## %s   (dsac_reproject ran form %s)" % (name, eng.k2_form()))
        show(res, bytes_stored=4.0 * s["N"] * s["P"])
        for k in ("err + soft", "err only", "soft only"):
            print("ratio rgbd / rgb, %-10s %.3f" % (k, res["rgbd  " + k][0] / res["rgb   " + k][0]))
        if bench and res["rgbd  err + soft"][0] > 1.05 * res["rgb   err + soft"][0]:
            failed = True
            print("MISSED: dsac_score_rgbd takes more than 1.05 x dsac_reproject's time at the bench shape")
        del s
        torch.cuda.empty_cache()
    print("\n# (b) sampling: dsac_sample_rgbd against dsac_sample, 640x480")
    for name, N, F in (("1 x 256", 256, 1), ("1 x 4096", 4096, 1), ("16 x 256", 256, 16)):
        s = shape(480, 640, N, F, with_err=False)
        res = measure(s, [("dsac_sample_rgbd", sample_rgbd), ("dsac_sample", sample_rgb)])
        print("\n## %s" % name)
        show(res)
        print("ratio rgbd / rgb %.3f" % (res["dsac_sample_rgbd"][0] / res["dsac_sample"][0]))
    print("\n# (c) refinement: dsac_refine_rgbd against dsac_refine_soft (split form)")
    for name, H, W, N, F in (("16 x 256 x 40x40", 40, 40, 256, 16), ("256 x 640x480", 480, 640, 256, 1)):
        s = shape(H, W, N, F, with_err=False)
        res = measure(s, [("rgbd, whole call (max_iters 20)", lambda s: refine_rgbd(s, 20)), ("rgb,  whole call (max_iters 20)", lambda s: refine_rgb(s, 20)),
                          ("rgbd, max_iters 1", lambda s: refine_rgbd(s, 1)), ("rgb,  max_iters 1", lambda s: refine_rgb(s, 1))])
        refine_rgbd(s, 20)
        eng.synchronize()
        iters = s["it"].cpu().numpy()
        status = np.bincount(s["st"].cpu().numpy(), minlength=6)
        print("\n## %s   (rgbd accepted steps: mean %.1f, max %d; statuses CONVERGED %d MAXIT %d SCORE %d FEW %d SINGULAR %d NONFINITE %d)" %
              ((name, iters.mean(), iters.max()) + tuple(status[:6])))
        show(res)
        print("ratio rgbd / rgb: whole call %.3f, max_iters 1 (two passes, two steps) %.3f" %
              (res["rgbd, whole call (max_iters 20)"][0] / res["rgb,  whole call (max_iters 20)"][0], res["rgbd, max_iters 1"][0] / res["rgb,  max_iters 1"][0]))
    eng.set_option("refine_soft_form", -1)
    eng.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
