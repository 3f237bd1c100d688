#!/usr/bin/env python3
"""What guided sampling (dsac_set_sampling_weights) costs and buys, measured in ONE process on device buffers, the cases alternating inside every round.

    K1        dsac_sample on 640x480 synthetic frames (30 % outliers) at 1 x 256, 1 x 4 096 and 16 x 256 hypotheses: uniform draw (no weights), all-ones
              weights (the same distribution through the table: what the search costs) and inlier_mask weights (what guidance buys).  GPU time per
              launch from a pair of events around a run of back-to-back launches on the context's stream.
    table     dsac_set_sampling_weights from a device tensor at 1 and 16 frames: the same way
    call      the whole dsac_process_images call at the benchmark's shape (16 x 256 x 640x480), uniform against inlier_mask: host time per call

The cases swap order from round to round and every timed run follows an untimed run of the same length of the same case.  Reported per line: the median over
the rounds, min and max, and the ratio to the uniform draw with the spread of the uniform draw's own repeats beside it.

    python scripts/k1_guided_ab.py [--rounds 6] [--reps 50] [--out profiles/k1_guided_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_TRIES = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k1_guided_ab.txt"))
    a = ap.parse_args()
    import torch
    import dsac_amd
    from dsac_amd import synth
    dev = torch.device("cuda", 0)
    eng = dsac_amd.Engine(0)
    st = torch.cuda.ExternalStream(eng.stream, device=dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# device: %s" % eng.device_info())
    say("# cases alternate inside every round of one process; %d rounds of %d launches after one settling round, each after an untimed run of the same length;"
        " the order of the cases rotates every round; max_tries = %d" % (a.rounds, a.reps, MAX_TRIES))
    cases = ("uniform (no weights)", "all-ones weights", "inlier_mask weights")

    def report(what, res, names, unit="us"):
        med = {s: statistics.median(res[s]) for s in names}
        base = names[0]
        for s in names:
            say("%-30s %-22s median %9.2f %s  (min %9.2f  max %9.2f)" % (what, s, med[s], unit, min(res[s]), max(res[s])))
        spread = (min(res[base]) / med[base], max(res[base]) / med[base])
        for s in names[1:]:
            r = med[s] / med[base]
            say("%-30s %s / %s = %.4f; the uniform draw's own repeats span %.4f .. %.4f of their median: %s" %
                (what, s, base, r, spread[0], spread[1], "inside" if spread[0] <= r <= spread[1] else "OUTSIDE"))
        return med

    def gpu_us(fn, reps):
        """GPU time per call of `reps` back-to-back enqueues on the context's stream"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
        eng.synchronize()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / reps

    h, w = 480, 640
    P = h * w
    F16 = 16
    fr = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=True) for f in range(4)]
    cam = fr[0]["cam"]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % 4]["xyz"] for f in range(F16)]))).to(dev)
    mask = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % 4]["inlier_mask"].astype(np.float32) for f in range(F16)]))).to(dev)
    ones = torch.ones(F16, P, dtype=torch.float32, device=dev)
    table_us = {}

    def set_frames(F):
        if F == 1:
            eng.set_frame(xyz[0], None, h, w, cam, borrow=True)
        else:
            eng.set_frames(xyz[:F], None, h, w, cam, borrow=True)

    def set_case(s, F):
        set_frames(F)  # clears the weights
        if s == cases[1]:
            eng.set_sampling_weights(ones[:F])
        elif s == cases[2]:
            eng.set_sampling_weights(mask[:F])
        assert eng.get_option("sampling_weights") == (0 if s == cases[0] else 1)

    # ---- K1 alone
    for F, N in ((1, 256), (1, 4096), (16, 256)):
        n = F * N
        out = (torch.zeros(n, 6, dtype=torch.float64, device=dev), torch.zeros(n, 4, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
        res = {s: [] for s in cases}
        acc, sets_of = {}, {}
        for rnd in range(a.rounds + 1):
            order = cases[rnd % 3:] + cases[:rnd % 3]
            for s in order:
                set_case(s, F)
                fn = lambda: eng.sample(n, seed=9, thr=10.0, max_tries=MAX_TRIES, out=out)
                gpu_us(fn, a.reps)
                t = gpu_us(fn, a.reps)
                if rnd:
                    res[s].append(t)
                acc[s] = float(out[2].double().mean())
                sets_of[s] = out[1].clone()
        say("\n== K1 alone (dsac_sample), %d x %d hypotheses on %dx%d: GPU time per launch" % (F, N, w, h))
        report("K1 %2d x %4d" % (F, N), res, cases)
        in_mask = float(mask[:F].reshape(F, P).gather(1, sets_of[cases[2]].reshape(F, N * 4).long()).mean())
        say("%-30s accepted fraction: %s; cells of the guided sets inside the mask: %.4f" % ("", ", ".join("%s %.4f" % (s, acc[s]) for s in cases), in_mask))

    # ---- the table build
    for F in (1, 16):
        set_frames(F)
        res = []
        for rnd in range(a.rounds + 1):
            fn = lambda: eng.set_sampling_weights(mask[:F])
            gpu_us(fn, a.reps)
            t = gpu_us(fn, a.reps)
            if rnd:
                res.append(t)
        table_us[F] = statistics.median(res)
        say("\n== table build (dsac_set_sampling_weights, device tensor), %d frame(s) of %dx%d: GPU time per call" % (F, w, h))
        say("%-30s median %9.2f us  (min %9.2f  max %9.2f)" % ("table build, %2d frame(s)" % F, table_us[F], min(res), max(res)))

    # ---- the whole call at the benchmark's shape
    F, N = 16, 256
    n = F * N
    perm = torch.from_numpy(synth.fast_permutations(P, 8)).to(dev)
    gts = torch.zeros(F, 6, dtype=torch.float64, device=dev)
    run_err = torch.empty(n, P, dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(hyps=torch.zeros(n, 6, **f64), sampledPoints=torch.zeros(n, 4, dtype=torch.int32, device=dev), ok=torch.zeros(n, dtype=torch.uint8, device=dev),
               scores=torch.zeros(n, **f64), sfScores=torch.zeros(n, **f64), sfEntropy=torch.zeros(F, **f64), avgHyp=torch.zeros(F, 6, **f64),
               refAvgHyp=torch.zeros(F, 6, **f64), refSteps=torch.zeros(F, dtype=torch.int32, device=dev), out4=torch.zeros(F, 4, **f64))
    two = (cases[0], cases[2])
    res = {s: [] for s in two}
    reps = max(5, a.reps // 5)
    for rnd in range(a.rounds + 1):
        for s in (two if rnd % 2 == 0 else two[::-1]):
            set_case(s, F)
            for _ in range(reps):
                eng.processImages(N, perm, gt_jp6=gts, seed=9, max_tries=MAX_TRIES, err=run_err, out=out)
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.processImages(N, perm, gt_jp6=gts, seed=9, max_tries=MAX_TRIES, err=run_err, out=out)
            eng.synchronize()
            if rnd:
                res[s].append((time.perf_counter() - t0) * 1e6 / reps)
    say("\n== the whole dsac_process_images call (K1, K2, K3, K6, K7), %d x %d hypotheses on %dx%d: host time per call" % (F, N, w, h))
    report("dsac_process_images", res, two)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
