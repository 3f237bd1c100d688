#!/usr/bin/env python3
"""Timing of the enqueue-only reference-stream chain (dsac_sample_refstream_frames, "pi_refstream") against the per-image call it stands beside.
Device events around synchronised work, after warm-up, old and new alternating in one process, medians and quartiles.
  (a) one 640 x 480 image, 256 hypotheses, 1 and 8 streams: dsac_sample_refstream against dsac_sample_refstream_frames with one frame
  (b) dsac_process_images on 16 such images with "pi_refstream" 0 and 1
  (c) the evaluation program: per-image -refstream 1 loop against -refstream 1 -batch 16 on 64 synthetic 640 x 480 images
usage: refstream_frames_bench.py [--reps 40] [--chain-only F]   (--chain-only: nothing but a few chains over F frames, for a kernel trace)"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quart(x):
    q1, med, q3 = np.percentile(np.asarray(x), [25, 50, 75])
    return med, q1, q3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--chain-only", type=int, default=0)
    ap.add_argument("--skip-driver", action="store_true")
    a = ap.parse_args()
    import torch
    import dsac_amd
    from dsac_amd import synth
    from dsac_amd.capi import lib, ptr, check
    H, W, N = 480, 640, 256
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eng = dsac_amd.Engine(0, stream=stream)
    F = max(16, a.chain_only)
    frames = [synth.chess_like_frame(H, W, seed=2305 + i) for i in range(F)]
    cam = frames[0]["cam"]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([f["xyz"] for f in frames]))).to(dev)
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    poses, sets, ok = z((F * N, 6)), z((F * N, 4), torch.int32), z(F * N, torch.uint8)
    torch.cuda.synchronize(dev)

    if a.chain_only:
        eng.set_frames(xyz[:a.chain_only], None, H, W, cam, borrow=True)
        for T in (1, 8):
            for _ in range(3):
                eng.refstreamInit(1305, T)
                eng.sampleRefstreamFrames(N, out=(poses, sets, ok), counters=False)
        eng.synchronize()
        print("chain-only: 3 chains over %d frames for 1 and 8 streams" % a.chain_only)
        return

    def timed(fn, prep):
        prep()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    # ---- (a) -------------------------------------------------------------------------------------------------------------------------------
    eng.set_frame(xyz[0], None, H, W, cam, borrow=True)
    for T in (1, 8):
        old = lambda: check(eng._ctx, lib.dsac_sample_refstream(eng._ctx, N, 10.0, 1 << 24, ptr(poses), ptr(sets), ptr(ok), None, None))
        new = lambda: eng.sampleRefstreamFrames(N, out=(poses, sets, ok), counters=False)
        prep = lambda: eng.refstreamInit(1305, T)
        for _ in range(5):
            timed(old, prep), timed(new, prep)
        to, tn = [], []
        for _ in range(a.reps):
            to.append(timed(old, prep))
            tn.append(timed(new, prep))
        mo, o1, o3 = quart(to)
        mn, n1, n3 = quart(tn)
        print("(a) 640x480, 256 hypotheses, %d stream(s), %d alternating repetitions: dsac_sample_refstream median %.1f us (quartiles %.1f .. %.1f, IQR %.1f); "
              "dsac_sample_refstream_frames (1 frame, default budget) median %.1f us (quartiles %.1f .. %.1f); condition new <= old + IQR(old) = %.1f: %s"
              % (T, a.reps, mo, o1, o3, o3 - o1, mn, n1, n3, mo + (o3 - o1), "met" if mn <= mo + (o3 - o1) else "NOT met"))

    # ---- (b) -------------------------------------------------------------------------------------------------------------------------------
    Fb = 16
    perm = torch.from_numpy(synth.fast_permutations(H * W, 8)).to(dev)
    gts = z((Fb, 6))
    out = dict(hyps=poses[:Fb * N], sampledPoints=sets[:Fb * N], ok=ok[:Fb * N], scores=z(Fb * N), sfScores=z(Fb * N), sfEntropy=z(Fb), avgHyp=z((Fb, 6)), refAvgHyp=z((Fb, 6)),
               refSteps=z(Fb, torch.int32), out4=z((Fb, 4)))
    torch.cuda.synchronize(dev)
    eng.set_frames(xyz[:Fb], None, H, W, cam, borrow=True)
    for T in (1, 8):
        prep = lambda: eng.refstreamInit(1305, T)
        ctr = lambda: eng.processImages(N, perm, gt_jp6=gts, seed=7, out=out, refstream=False)
        rs = lambda: eng.processImages(N, perm, gt_jp6=gts, seed=7, out=out, refstream=True)
        for _ in range(3):
            timed(ctr, prep), timed(rs, prep)
        tc, tr = [], []
        for _ in range(max(30, a.reps)):
            tc.append(timed(ctr, prep))
            tr.append(timed(rs, prep))
        mc, c1, c3 = quart(tc)
        mr, r1, r3 = quart(tr)
        print("(b) dsac_process_images, 16 x 640x480 x 256 hypotheses, %d stream(s): counter stream median %.1f us per call (quartiles %.1f .. %.1f) = %.1f us per image; "
              "pi_refstream median %.1f us per call (quartiles %.1f .. %.1f) = %.1f us per image" % (T, mc, c1, c3, mc / Fb, mr, r1, r3, mr / Fb))
    eng.set_option("pi_refstream", 0)
    eng.close()

    # ---- (c) -------------------------------------------------------------------------------------------------------------------------------
    if a.skip_driver:
        return
    import tempfile
    exe = os.path.join(ROOT, "dsac_amd", "host", "test_ransac_softam")
    for batch in (0, 16):
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run([exe, "-synth", "64", "-mw", "640", "-mh", "480", "-rI", "256", "-refstream", "1", "-batch", str(batch), "-passes", "4"], cwd=d,
                               capture_output=True, text=True, timeout=500)
            m = re.search(r"^Timing:.*$", r.stdout, re.M)
            print("(c) test_ransac_softam -synth 64 -mw 640 -mh 480 -rI 256 -refstream 1 -batch %d -passes 4 (rc %d): %s" % (batch, r.returncode, m.group(0) if m else r.stdout[-400:]))


if __name__ == "__main__":
    main()
