#!/usr/bin/env python3
"""A/B of frame batches with one camera per frame (dsac_set_frames_cams) against the shared-camera batch (dsac_set_frames), alternating in ONE process on
device buffers.  The table holds 16 EQUAL rows, so both sides compute the same thing and must agree in every bit: the script fails if they do not.  What is
timed is what the table costs: one scalar load per workgroup in K2 and K4, per wave in K1 / K6, the per-frame exponent in the record kernel.

    K2       dsac_reproject, err + soft, at the benchmark's shape (16 frames x 256 hypotheses x 640x480): kernel time from the dispatch's own events
    call     the whole dsac_process_images call at the same shape: host time per call over a run of calls, synchronised at the end
    K4       dsac_score_backward at 16 frames x 128 hypotheses x 40x40: the main pass's kernel time

The two sides swap places from round to round and every timed run follows an untimed run of the same length on the same side (what a block follows -- the
other side's launches, or the comparison of two 5 GB volumes -- otherwise shows as a few per cent between two identical kernels).
Reported per line: the median over the rounds, min and max, and the ratio per-frame / shared with the spread of the shared-camera repeats beside it (a
ratio inside that spread is no difference).

    python scripts/frame_cams_ab.py [--rounds 6] [--reps 20] [--out profiles/frame_cams_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_cams_ab.txt"))
    a = ap.parse_args()
    import torch
    import dsac_amd
    from dsac_amd import synth
    dev = torch.device("cuda", 0)
    eng = dsac_amd.Engine(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# device: %s" % eng.device_info())
    say("# per-frame cameras (a table of 16 equal rows) against the shared camera, alternating inside every round of one process; %d rounds of %d launches after one"
        " settling round, each after an untimed run of the same length; the sides swap places every round; results compared bit for bit in every round" % (a.rounds, a.reps))
    sides = ("shared camera  (dsac_set_frames)", "16 equal rows  (dsac_set_frames_cams)")

    def report(what, res, unit="us"):
        med = [statistics.median(res[s]) for s in sides]
        for s, m in zip(sides, med):
            say("%-34s %-40s median %9.1f %s  (min %9.1f  max %9.1f)" % (what, s, m, unit, min(res[s]), max(res[s])))
        spread = (min(res[sides[0]]) / med[0], max(res[sides[0]]) / med[0])
        ratio = med[1] / med[0]
        say("%-34s per-frame / shared = %.4f; the shared camera's own repeats span %.4f .. %.4f of their median: %s" %
            (what, ratio, spread[0], spread[1], "inside" if spread[0] <= ratio <= spread[1] else "OUTSIDE"))
        return ratio, spread

    def setter(xyz, h, w, cam, frames):
        table = np.tile(np.array(cam, np.float32), (frames, 1))
        return {sides[0]: lambda: eng.set_frames(xyz, None, h, w, cam, borrow=True), sides[1]: lambda: eng.set_frames(xyz, None, h, w, table, borrow=True)}

    # ---- K2 and the whole call at the benchmark's shape
    F, N, h, w = 16, 256, 480, 640
    P = h * w
    fr = [synth.chess_like_frame(h, w, seed=2305 + f, grid_uv=True) for f in range(4)]
    cam = fr[0]["cam"]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr[f % 4]["xyz"] for f in range(F)]))).to(dev)
    set_as = setter(xyz, h, w, cam, F)
    poses = torch.from_numpy(synth.random_poses(F * N, seed=11)).to(dev)
    poses[:, 5] += 2500.0
    # both sides write the SAME 5 GB of error images (two buffers are two placements in HBM, which alone is worth a few per cent); a side's images are
    # copied aside after its timed run for the comparison
    run_err = torch.empty(F * N, P, dtype=torch.float32, device=dev)
    err = {s: torch.empty(F * N, P, dtype=torch.float32, device=dev) for s in sides}
    soft = {s: torch.zeros(F * N, dtype=torch.float64, device=dev) for s in sides}
    res = {s: [] for s in sides}
    for rnd in range(a.rounds + 1):
        for s in (sides if rnd % 2 == 0 else sides[::-1]):
            set_as[s]()
            for _ in range(a.reps):
                eng.reproject(poses, N=F * N, err=run_err, soft=soft[s])
            eng.synchronize()
            assert eng.k2_form() == ("exact (vector build)", 0)
            assert eng.get_option("frame_cams") == (1 if s == sides[1] else 0)
            eng.profile_enable(True, stride=1)
            eng.profile_read(0, reset=True)
            for _ in range(a.reps):
                eng.reproject(poses, N=F * N, err=run_err, soft=soft[s])
            eng.synchronize()
            ms, n = eng.profile_read(0, reset=True)
            eng.profile_enable(False)
            if rnd:
                res[s].append(ms * 1e3 / n)
            err[s].copy_(run_err)
            torch.cuda.synchronize(dev)
        if not (torch.equal(err[sides[0]], err[sides[1]]) and torch.equal(soft[sides[0]], soft[sides[1]])):
            sys.exit("K2: the table of equal rows and the shared camera differ")
    say("\n== K2 (dsac_reproject, err + soft), %d x %d hypotheses on %dx%d: kernel time per launch" % (F, N, w, h))
    report("K2 kernel", res)

    perm = torch.from_numpy(synth.fast_permutations(P, 8)).to(dev)
    gts = torch.zeros(F, 6, dtype=torch.float64, device=dev)

    def bufs():
        n = F * N
        return dict(hyps=torch.zeros(n, 6, dtype=torch.float64, device=dev), sampledPoints=torch.zeros(n, 4, dtype=torch.int32, device=dev),
                    ok=torch.zeros(n, dtype=torch.uint8, device=dev), scores=torch.zeros(n, dtype=torch.float64, device=dev),
                    sfScores=torch.zeros(n, dtype=torch.float64, device=dev), sfEntropy=torch.zeros(F, dtype=torch.float64, device=dev),
                    avgHyp=torch.zeros(F, 6, dtype=torch.float64, device=dev), refAvgHyp=torch.zeros(F, 6, dtype=torch.float64, device=dev),
                    refSteps=torch.zeros(F, dtype=torch.int32, device=dev), out4=torch.zeros(F, 4, dtype=torch.float64, device=dev))
    out = {s: bufs() for s in sides}
    torch.cuda.synchronize(dev)
    res = {s: [] for s in sides}
    for rnd in range(a.rounds + 1):
        for s in (sides if rnd % 2 == 0 else sides[::-1]):
            set_as[s]()
            for _ in range(a.reps):
                eng.processImages(N, perm, gt_jp6=gts, seed=9, err=run_err, out=out[s])
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                eng.processImages(N, perm, gt_jp6=gts, seed=9, err=run_err, out=out[s])
            eng.synchronize()
            if rnd:
                res[s].append((time.perf_counter() - t0) * 1e6 / a.reps)
            err[s].copy_(run_err)
            torch.cuda.synchronize(dev)
        same = torch.equal(err[sides[0]], err[sides[1]]) and all(torch.equal(out[sides[0]][k], out[sides[1]][k]) for k in out[sides[0]])
        if not same:
            sys.exit("dsac_process_images: the table of equal rows and the shared camera differ")
    say("\n== the whole dsac_process_images call (K1, K2, K3, K6, K7), %d x %d hypotheses on %dx%d: host time per call" % (F, N, w, h))
    report("dsac_process_images", res)
    say("%-34s = %.1f us per image with the shared camera" % ("", statistics.median(res[sides[0]]) / F))
    del err, run_err, xyz
    torch.cuda.empty_cache()

    # ---- K4 at 16 frames x 128 hypotheses x 40x40
    F, N, h, w = 16, 128, 40, 40
    P = h * w
    fr = [synth.chess_like_frame(h, w, seed=610 + f, quantise_int16=True) for f in range(F)]
    cam = fr[0]["cam"]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([f_["xyz"] for f_ in fr]))).to(dev)
    uv = torch.from_numpy(fr[0]["uv"]).to(dev)
    table = np.tile(np.array(cam, np.float32), (F, 1))
    set_as = {sides[0]: lambda: eng.set_frames(xyz, uv, h, w, cam, borrow=True), sides[1]: lambda: eng.set_frames(xyz, uv, h, w, table, borrow=True)}
    set_as[sides[0]]()
    p_h, s_h, ok = eng.sample(F * N, seed=3)
    posesd, setsd = torch.from_numpy(p_h).to(dev), torch.from_numpy(s_h).to(dev)
    J = torch.from_numpy(np.asarray(eng.dPNP(s_h))).to(dev)
    d_err = torch.from_numpy((np.random.default_rng(11).standard_normal((F * N, P)) * 1e-3).astype(np.float32)).to(dev)
    grad = {s: torch.zeros(F * P, 3, dtype=torch.float64, device=dev) for s in sides}
    res = {s: [] for s in sides}
    for rnd in range(a.rounds + 1):
        for s in (sides if rnd % 2 == 0 else sides[::-1]):
            set_as[s]()
            for _ in range(a.reps):
                eng.dScore(posesd, setsd, d_err, dpnp=J, grad=grad[s])
            eng.synchronize()
            eng.profile_enable(True, stride=1)
            eng.profile_read(1, reset=True)
            for _ in range(a.reps):
                eng.dScore(posesd, setsd, d_err, dpnp=J, grad=grad[s])
            eng.synchronize()
            ms, n = eng.profile_read(1, reset=True)
            eng.profile_enable(False)
            if rnd:
                res[s].append(ms * 1e3 / n)
        # the pose sums of the last launch: bit for bit (the gradient itself meets in fp64 atomics whose order is the hardware's, on both sides)
        G6 = {}
        for s in sides:
            set_as[s]()
            eng.dScore(posesd, setsd, d_err, dpnp=J, grad=grad[s])
            G6[s] = eng.lastPoseGradients(F * N).copy()
        if not np.array_equal(G6[sides[0]], G6[sides[1]]):
            sys.exit("K4: the pose sums under the table of equal rows and under the shared camera differ")
    say("\n== K4 (dsac_score_backward, main pass), %d x %d hypotheses on %dx%d: kernel time per launch" % (F, N, w, h))
    report("K4 main pass", res)
    rel = float((grad[sides[0]] - grad[sides[1]]).abs().max() / grad[sides[0]].abs().max())
    say("%-34s pose sums bit for bit; accumulated gradients differ by %.1e of the largest entry (fp64 atomics on shared cells)" % ("", rel))
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
