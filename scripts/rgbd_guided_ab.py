#!/usr/bin/env python3
"""What guided RGB-D sampling (dsac_set_sampling_weights_rgbd) costs, measured in ONE process on device buffers, the cases alternating inside every round.

    draw      dsac_sample_rgbd on 640x480 synthetic RGB-D frames (10 % depth holes) at 1 x 256, 1 x 4 096 and 16 x 256 hypotheses: uniform draw (no
              weights), all-ones weights (the uniform distribution over the VALID cells through the table: what the search costs) and a 50 % mask.
              Beside it, the yardstick: the 2D dsac_sample at the same shapes, uniform and with all-ones weights (dsac_set_sampling_weights).
              GPU time per launch from a pair of events around a run of back-to-back launches on the context's stream.
    table     dsac_set_sampling_weights_rgbd from a device tensor at 1 and 16 frames (the masking launch + the table build): the same way

The cases swap order from round to round and every timed run follows an untimed run of the same length of the same case.

GATE: at every shape (guided RGB-D - uniform RGB-D) must not exceed 1.25 x (guided 2D - uniform 2D), medians, all-ones weights on both sides: the added time
is the same table search for three side-by-side candidates instead of four.  The script exits non-zero otherwise.

    python scripts/rgbd_guided_ab.py [--rounds 6] [--reps 50] [--out profiles/rgbd_guided_ab.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_TRIES = 4096
GATE = 1.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd_guided_ab.txt"))
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
    cases = ("rgbd uniform (no weights)", "rgbd all-ones weights", "rgbd 50 % mask", "2d uniform (no weights)", "2d all-ones weights")

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
    fr = [synth.chess_like_frame_rgbd(h, w, seed=2305 + f, grid_uv=True, missing_frac=0.1) for f in range(4)]
    cam = fr[0]["cam"]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % 4]["xyz"] for f in range(F16)]))).to(dev)
    pts = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % 4]["cam_xyz"] for f in range(F16)]))).to(dev)
    holes = float(np.mean([np.isnan(f["cam_xyz"][:, 2]).mean() for f in fr]))
    say("# frames: %dx%d, %.1f %% of the cells without a measured point" % (w, h, 100.0 * holes))
    ones = torch.ones(F16, P, dtype=torch.float32, device=dev)
    half = torch.from_numpy((np.random.default_rng(7).random((F16, P)) < 0.5).astype(np.float32)).to(dev)

    def set_frames(F, points):
        if F == 1:
            eng.set_frame(xyz[0], None, h, w, cam, borrow=True)
        else:
            eng.set_frames(xyz[:F], None, h, w, cam, borrow=True)
        if points:
            eng.set_camera_points(pts[:F])

    def set_case(s, F):
        rgbd = s.startswith("rgbd")
        set_frames(F, rgbd)  # clears every kind of weights
        if s == cases[1]:
            eng.set_sampling_weights_rgbd(ones[:F])
        elif s == cases[2]:
            eng.set_sampling_weights_rgbd(half[:F])
        elif s == cases[4]:
            eng.set_sampling_weights(ones[:F])
        assert eng.get_option("sampling_weights") == (1 if s == cases[4] else 0)
        assert eng.get_option("sampling_weights_rgbd") == (1 if s in cases[1:3] else 0)

    failed = []
    for F, N in ((1, 256), (1, 4096), (16, 256)):
        n = F * N
        out3 = (torch.zeros(n, 6, dtype=torch.float64, device=dev), torch.zeros(n, 3, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
        out4 = (torch.zeros(n, 6, dtype=torch.float64, device=dev), torch.zeros(n, 4, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
        res = {s: [] for s in cases}
        acc = {}
        for rnd in range(a.rounds + 1):
            k = rnd % len(cases)
            for s in cases[k:] + cases[:k]:
                set_case(s, F)
                if s.startswith("rgbd"):
                    fn = lambda: eng.sampleRGBD(n, seed=9, thr=100.0, max_tries=MAX_TRIES, out=out3)
                else:
                    fn = lambda: eng.sample(n, seed=9, thr=10.0, max_tries=MAX_TRIES, out=out4)
                gpu_us(fn, a.reps)
                t = gpu_us(fn, a.reps)
                if rnd:
                    res[s].append(t)
                acc[s] = float((out3 if s.startswith("rgbd") else out4)[2].double().mean())
                if s == cases[2]:
                    in_mask = float(half[:F].reshape(F, P).gather(1, out3[1].reshape(F, N * 3).long()).mean())
        say("\n== the draw alone, %d x %d hypotheses on %dx%d: GPU time per launch" % (F, N, w, h))
        med = {s: statistics.median(res[s]) for s in cases}
        for s in cases:
            say("%-16s %-28s median %9.2f us  (min %9.2f  max %9.2f)  accepted %.4f" % ("%2d x %4d" % (F, N), s, med[s], min(res[s]), max(res[s]), acc[s]))
        say("%-16s cells of the masked sets inside the mask: %.4f" % ("", in_mask))
        base = cases[0]
        say("%-16s the uniform RGB-D draw's own repeats span %.4f .. %.4f of their median" % ("", min(res[base]) / med[base], max(res[base]) / med[base]))
        d3, d2 = med[cases[1]] - med[cases[0]], med[cases[4]] - med[cases[3]]
        ok = d3 <= GATE * d2
        say("%-16s added by the table: RGB-D %+.2f us (x %.3f of the uniform draw), 2D %+.2f us (x %.3f); RGB-D / 2D = %.3f, gate <= %.2f: %s" %
            ("", d3, med[cases[1]] / med[cases[0]], d2, med[cases[4]] / med[cases[3]], d3 / d2 if d2 > 0 else float("inf"), GATE, "ok" if ok else "FAILED"))
        say("%-16s 50 %% mask / all-ones = %.3f" % ("", med[cases[2]] / med[cases[1]]))
        if not ok:
            failed.append((F, N))

    # ---- the masked table build
    for F in (1, 16):
        set_frames(F, True)
        res = []
        for rnd in range(a.rounds + 1):
            fn = lambda: eng.set_sampling_weights_rgbd(half[:F])
            gpu_us(fn, a.reps)
            t = gpu_us(fn, a.reps)
            if rnd:
                res.append(t)
        say("\n== masked table build (dsac_set_sampling_weights_rgbd, device tensor), %d frame(s) of %dx%d: GPU time per call" % (F, w, h))
        say("%-30s median %9.2f us  (min %9.2f  max %9.2f)" % ("masked table build, %2d frame(s)" % F, statistics.median(res), min(res), max(res)))
    eng.close()
    say("\n# gate (guided RGB-D - uniform RGB-D) <= %.2f x (guided 2D - uniform 2D): %s" % (GATE, "held at every shape" if not failed else "FAILED at %s" % failed))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
