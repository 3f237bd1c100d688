"""dsac_sample_refstream_frames and "pi_refstream": the sampling loop in the reference's own random stream (std::mt19937(seed + t) per OpenMP thread,
core/thread_rand.cpp:40-69; core/cnn_softam.h:1010-1060) as a chain that is enqueued without a host round trip, for frame batches, and inside
dsac_process_images / dsac_process_images_begin.  Sets bit-identical to the REAL reference's on both golden frames, to the oracle's loop (the standard
library's own generator and distribution) image by image on the running generators, and to dsac_sample_refstream called per image."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SUBSAMPLE_OUTPUTS = 6400  # stochasticSubSample (core/cnn_softam.h:283-309): four 32-bit outputs per cell of its 40 x 40 grid, on generator 0


def golden(v):
    g = np.load(os.path.join(HERE, "golden", "ref_frame_v%d.npz" % v))
    sets_ref = g["sampledPoints"][:, :, 1] * 40 + g["sampledPoints"][:, :, 0]
    return g, sets_ref, g["estObj"].astype(np.float32), g["sampling"].astype(np.float32)


@pytest.fixture(scope="module")
def frames480(synth):
    """16 synthetic 640 x 480 frames (seeds 2305 ... 2320)."""
    fr = [synth.chess_like_frame(480, 640, seed=2305 + i) for i in range(16)]
    return np.ascontiguousarray(np.stack([f["xyz"] for f in fr])), fr[0]["cam"]


@pytest.fixture(scope="module")
def oracle480(orc, synth, frames480):
    """The oracle's loop over the 16 frames on running generators, 256 hypotheses, for 1 and 4 threads: (poses, sets, ok, consumed, attempts) per image."""
    xyz, cam = frames480
    uv = synth.pixel_grid(480, 640)
    res = {}
    for T in (1, 4):
        skip = np.zeros(T, np.uint64)
        per = []
        for f in range(16):
            r = orc.sample_refstream(256, 1305, xyz[f], uv, 480, 640, cam, threads=T, skip32=skip)
            skip = skip + r[3]
            per.append(r)
        res[T] = per
    return res


# ---- 1. the real reference's sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,seed", [(1, 1305), (2, 4242)])
def test_golden_frames_one_thread_equal_the_real_reference(engine, v, seed):
    g, sets_ref, xyz, uv = golden(v)
    engine.set_frame(xyz, uv, 40, 40, g["cam"])
    engine.refstreamInit(seed, 1)
    poses, sets, ok, consumed, attempts = engine.sampleRefstreamFrames(64, thr=10.0, discard0=SUBSAMPLE_OUTPUTS)
    assert ok.all()
    assert np.array_equal(sets, sets_ref), "minimal sets differ from the real reference's (%d of 64 equal)" % (sets == sets_ref).all(axis=1).sum()
    assert np.abs(poses - g["hyps"]).max() <= 1e-5
    assert consumed.shape == (1, 1) and attempts[0, 0] >= 64 and consumed[0, 0] >= 8 * attempts[0, 0]


@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("threads", [3, 4])
def test_golden_frames_several_threads_equal_the_real_reference(engine, v, threads):
    g, _, xyz, uv = golden(v)
    t = np.load(os.path.join(HERE, "golden", "ref_threads_v%d.npz" % v))
    engine.set_frame(xyz, uv, 40, 40, g["cam"])
    engine.refstreamInit(int(t["seed"]), threads)
    poses, sets, ok, consumed, attempts = engine.sampleRefstreamFrames(64, thr=10.0, discard0=SUBSAMPLE_OUTPUTS)
    assert ok.all() and np.array_equal(sets, t["t%d_sets" % threads])
    assert np.abs(poses - t["t%d_hyps" % threads]).max() <= 1e-5


# ---- 2. running generators over a batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 3, 4, 7])
def test_batch_of_three_images_on_running_generators_against_the_oracle(engine, orc, threads):
    g, _, xyz, uv = golden(2)
    engine.set_frames(np.ascontiguousarray(np.stack([xyz] * 3)), uv, 40, 40, g["cam"])
    engine.refstreamInit(4242, threads)
    p, s, ok, c, a = engine.sampleRefstreamFrames(61, thr=10.0, discard0=SUBSAMPLE_OUTPUTS)
    assert c.shape == (3, threads) and a.shape == (3, threads)
    skip = np.zeros(threads, np.uint64)
    for f in range(3):
        skip[0] += SUBSAMPLE_OUTPUTS  # before EVERY image
        po, so, oko, co, ao = orc.sample_refstream(61, 4242, xyz, uv, 40, 40, g["cam"], threads=threads, skip32=skip)
        sl = slice(61 * f, 61 * (f + 1))
        assert oko.all() and np.array_equal(s[sl], so) and np.array_equal(ok[sl], oko), "image %d" % f
        assert np.array_equal(c[f], co) and np.array_equal(a[f], ao), "image %d" % f
        assert np.abs(p[sl] - po).max() <= 1e-6
        skip = skip + co


# ---- 3. 640 x 480, against the oracle and against dsac_sample_refstream per image --------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
def test_640x480_batch_against_the_oracle_and_the_per_image_call(engine, frames480, oracle480, threads):
    xyz, cam = frames480
    H, W, N, F = 480, 640, 256, 16
    engine.set_frames(xyz, None, H, W, cam)
    engine.refstreamInit(1305, threads)
    p, s, ok, c, a = engine.sampleRefstreamFrames(N, thr=10.0)
    assert ok.all()
    for f in range(F):
        po, so, oko, co, ao = oracle480[threads][f]
        sl = slice(N * f, N * (f + 1))
        assert oko.all() and np.array_equal(s[sl], so), "image %d" % f
        assert np.array_equal(c[f], co) and np.array_equal(a[f], ao), "image %d" % f
        assert np.abs(p[sl] - po).max() <= 1e-6 * max(1.0, np.abs(po).max())
    # the per-image entry point from the same generator state: identical sets, poses bit for bit, identical counters
    engine.refstreamInit(1305, threads)
    for f in range(F):
        engine.set_frame(xyz[f], None, H, W, cam)
        p1, s1, ok1, c1, a1 = engine.sampleRefstream(N, thr=10.0)
        sl = slice(N * f, N * (f + 1))
        assert np.array_equal(s1, s[sl]) and np.array_equal(p1, p[sl]) and np.array_equal(ok1, ok[sl]), "image %d" % f
        assert np.array_equal(c1, c[f]) and np.array_equal(a1, a[f]), "image %d" % f
    # ... and the two may be mixed: a chain continues where the per-image call stopped
    engine.refstreamInit(1305, threads)
    engine.set_frame(xyz[0], None, H, W, cam)
    engine.sampleRefstream(N, thr=10.0)
    engine.set_frame(xyz[1], None, H, W, cam)
    p2, s2, ok2, c2, a2 = engine.sampleRefstreamFrames(N, thr=10.0)
    assert np.array_equal(s2, s[N:2 * N]) and np.array_equal(p2, p[N:2 * N]) and np.array_equal(c2[0], c[1])


# ---- 4. a budget that ends inside image 0 ------------------------------------------------------------------------------------------------------
def test_budget_ends_inside_image_0_and_image_1_continues(engine, orc, synth, frames480, oracle480):
    xyz, cam = frames480
    H, W, N = 480, 640, 256
    uv = synth.pixel_grid(H, W)
    po, so, oko, co, ao = oracle480[1][0]
    budget = int(ao[0]) // 2
    engine.set_frames(xyz[:2], None, H, W, cam)
    engine.refstreamInit(1305, 1)
    p, s, ok, c, a = engine.sampleRefstreamFrames(N, thr=10.0, max_attempts=budget)
    n = int(ok[:N].sum())
    assert 0 < n < N and ok[:n].all() and not ok[n:N].any()
    assert np.array_equal(s[:n], so[:n]) and np.abs(p[:n] - po[:n]).max() <= 1e-6 * max(1.0, np.abs(po).max()) and not p[n:N].any()
    assert a[0, 0] == budget
    # the oracle under the same budget: the same prefix, the same generator position
    pb, sb, okb, cb, ab = orc.sample_refstream(N, 1305, xyz[0], uv, H, W, cam, threads=1, max_attempts=budget)
    assert int(okb.sum()) == n and ab[0] == budget and c[0, 0] == cb[0]
    # image 1 of the same batch continues from there (it may or may not fit the halved budget: compare under the same one)
    p1, s1, ok1, c1, a1 = orc.sample_refstream(N, 1305, xyz[1], uv, H, W, cam, threads=1, skip32=cb, max_attempts=budget)
    n1 = int(ok1.sum())
    assert n1 > 0 and np.array_equal(ok[N:], ok1) and np.array_equal(s[N:N + n1], s1[:n1])
    assert c[1, 0] == c1[0] and a[1, 0] == a1[0]


# ---- 5. inside dsac_process_images and the begin / finish pair ---------------------------------------------------------------------------------
def _bufs(torch, dev, F, N):
    n = F * N
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    return dict(hyps=z((n, 6)), sampledPoints=z((n, 4), torch.int32), ok=z(n, torch.uint8), scores=z(n), sfScores=z(n), sfEntropy=z(F), avgHyp=z((F, 6)),
                refAvgHyp=z((F, 6)), refSteps=z(F, torch.int32), out4=z((F, 4)))


@pytest.mark.parametrize("threads", [1, 4])
def test_pi_refstream_in_process_images_and_the_seam(synth, orc, frames480, oracle480, threads):
    import torch
    import dsac_amd
    from dsac_amd.capi import lib, ptr, check
    xyz, cam = frames480
    H, W, N, F = 480, 640, 256, 8  # two consecutive calls of 8 frames each: the 16 frames, the second call continues the stream
    P = H * W
    dev = torch.device("cuda", 0)
    perm_h = synth.fast_permutations(P, 8)
    gts_h = np.zeros((16, 6))
    gts_h[:, 3:] = [10.0, -20.0, 30.0]
    perm = torch.from_numpy(perm_h).to(dev)
    gts = torch.from_numpy(gts_h).to(dev)
    xyz_d = torch.from_numpy(xyz).to(dev)
    keys = ("hyps", "sampledPoints", "ok", "scores", "sfScores", "sfEntropy", "avgHyp", "refAvgHyp", "refSteps", "out4")
    results = {}
    eng = dsac_amd.Engine(0)
    try:
        for path in ("whole", "seam"):
            for defer in (0, 1, 2):
                eng.set_option("pi_defer_tail", defer)
                eng.refstreamInit(1305, threads)
                outs = [_bufs(torch, dev, F, N) for _ in range(2)]
                soft = [torch.zeros(F * N, dtype=torch.float64, device=dev) for _ in range(2)]
                torch.cuda.synchronize(dev)
                for k in range(2):
                    eng.set_frames(xyz_d[F * k:F * (k + 1)], None, H, W, cam, borrow=True)
                    if path == "whole":
                        eng.processImages(N, perm, gt_jp6=gts[F * k:F * (k + 1)], seed=99, out=outs[k], refstream=True)
                    else:
                        o = outs[k]
                        eng.processImagesBegin(N, None, seed=99, soft=soft[k], out=(o["hyps"], o["sampledPoints"], o["ok"]), refstream=True)
                        eng.processImagesFinish(N, soft[k], perm, o["hyps"], gt_jp6=gts[F * k:F * (k + 1)], scale=0.1, out=o)
                eng.joinTail()
                eng.synchronize()
                torch.cuda.synchronize(dev)
                if path == "seam":
                    for k in range(2):
                        outs[k]["scores"] = soft[k]
                results[(path, defer)] = {key: np.concatenate([outs[k][key].cpu().numpy() for k in range(2)]) for key in keys}
        eng.set_option("pi_defer_tail", 0)
        eng.set_option("pi_refstream", 0)
        base = results[("whole", 0)]
        assert base["ok"].all()
        # the sets are the oracle's, image by image
        for f in range(16):
            assert np.array_equal(base["sampledPoints"][N * f:N * (f + 1)], oracle480[threads][f][1]), "image %d" % f
        # the three deferral modes and the seam (scores = the soft-inlier sums, scale 0.1: what the whole call computes) equal each other bit for bit
        for key_r, r in results.items():
            for key in keys:
                assert np.array_equal(r[key], base[key]), (key_r, key)
        # every other output is what the single-frame entry points give when they are handed those sets (the replay path: dsac_score_hypotheses with
        # sets, dsac_refine, dsac_loss), compared as tests/test_gpu_process_images.py compares the batch with its host-orchestrated mirror
        for f in range(16):
            sl = slice(N * f, N * (f + 1))
            eng.set_frame(xyz[f], None, H, W, cam)
            poses, sets, ok, scores, w, ent, avg = eng.scoreHypotheses(N, sets=base["sampledPoints"][sl], thr=10.0, scale=0.1)
            assert np.array_equal(sets, base["sampledPoints"][sl]) and np.array_equal(poses, base["hyps"][sl]) and np.array_equal(ok, base["ok"][sl])
            assert np.abs(w - base["sfScores"][sl]).max() <= 1e-6
            assert np.abs(avg - base["avgHyp"][f]).max() <= 1e-6 * max(1.0, np.abs(avg).max())
            ref, sd = np.zeros((1, 6)), np.zeros(1, np.int32)
            check(eng._ctx, lib.dsac_refine(eng._ctx, 1, ptr(np.ascontiguousarray(base["avgHyp"][f:f + 1])), ptr(perm_h), 8, 100, 50, 10.0, None, None, ptr(ref), None, ptr(sd)))
            assert np.abs(ref[0] - base["refAvgHyp"][f]).max() <= 1e-5 * max(1.0, np.abs(ref).max()) and sd[0] == base["refSteps"][f]
            l = eng.maxLossFrames(base["refAvgHyp"][f:f + 1], gts_h[f:f + 1])["out4"][0]
            assert abs(l[0] - base["out4"][f][0]) <= 1e-5 * max(1.0, l[0]) and l[3] == base["out4"][f][3]
    finally:
        eng.close()


# ---- 6. enqueue-only -----------------------------------------------------------------------------------------------------------------------------
def test_the_call_returns_before_the_stream_has_run(synth, frames480, oracle480):
    """A device-side delay of some tens of milliseconds sits in front of the call on the context's stream: dsac_sample_refstream_frames with device
    arrays returns while it is still running (the stream's query says so), dsac_sample_refstream -- which reads need[] back -- only after it."""
    import time
    import torch
    import dsac_amd
    xyz, cam = frames480
    H, W, N, F = 480, 640, 256, 2
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eng = dsac_amd.Engine(0, stream=stream)
    try:
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        out = (z((F * N, 6), torch.float64), z((F * N, 4), torch.int32), z(F * N, torch.uint8), z((F, 1), torch.int64), z((F, 1), torch.int64))
        one = (z((N, 6), torch.float64), z((N, 4), torch.int32), z(N, torch.uint8))
        xyz_d = torch.from_numpy(xyz[:F]).to(dev)
        torch.cuda.synchronize(dev)
        # the delay: sized from the clock rate, then checked with events (the spin kernel's counter need not tick at the shader clock)
        khz = eng.device_info()["clock_khz"]
        cycles = int(khz * 50)  # 50 ms of shader clocks
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            torch.cuda._sleep(cycles)
            e1.record(stream)
        stream.synchronize()
        ms = e0.elapsed_time(e1)
        cycles = int(cycles * 50.0 / max(ms, 1e-3))
        print("delay: %d cycles took %.2f ms; using %d cycles for ~50 ms" % (int(khz * 50), ms, cycles))
        # warm-up: scratch and generators exist, kernels are loaded
        eng.set_frames(xyz_d, None, H, W, cam, borrow=True)
        eng.refstreamInit(1305, 1)
        eng.sampleRefstreamFrames(N, out=out)
        eng.set_frame(xyz_d[0], None, H, W, cam, borrow=True)
        eng.sampleRefstream(N, out=one)
        eng.synchronize()
        # the probe on the new call
        eng.set_frames(xyz_d, None, H, W, cam, borrow=True)
        eng.refstreamInit(1305, 1)
        stream.synchronize()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
        t0 = time.perf_counter()
        eng.sampleRefstreamFrames(N, out=out)
        t1 = time.perf_counter()
        pending = not stream.query()
        print("dsac_sample_refstream_frames returned after %.3f ms, stream still busy: %s" % ((t1 - t0) * 1e3, pending))
        assert pending, "the call returned only after the stream had drained: it synchronised"
        stream.synchronize()
        s = out[1].cpu().numpy()
        for f in range(F):
            assert np.array_equal(s[N * f:N * (f + 1)], oracle480[1][f][1])
        assert np.array_equal(out[4].cpu().numpy()[:, 0], [oracle480[1][f][4][0] for f in range(F)])
        # the same probe on the per-image call: it comes back only when the delay is over, so the probe discriminates
        eng.set_frame(xyz_d[0], None, H, W, cam, borrow=True)
        eng.refstreamInit(1305, 1)
        stream.synchronize()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
        t0 = time.perf_counter()
        eng.sampleRefstream(N, out=one)
        t1 = time.perf_counter()
        drained = stream.query()
        print("dsac_sample_refstream returned after %.3f ms, stream drained: %s" % ((t1 - t0) * 1e3, drained))
        assert drained and (t1 - t0) * 1e3 >= 10.0
        assert np.array_equal(one[1].cpu().numpy(), oracle480[1][0][1])
    finally:
        eng.close()


# ---- 8. misuse ---------------------------------------------------------------------------------------------------------------------------------
def test_misuse(synth):
    import dsac_amd
    g, _, xyz, uv = golden(1)
    perm = synth.fast_permutations(1600, 8)
    e2 = dsac_amd.Engine(0)
    try:
        e2.set_frame(xyz, uv, 40, 40, g["cam"])
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            e2.sampleRefstreamFrames(8)  # no dsac_refstream_init
        assert ei.value.code == dsac_amd.capi.DSAC_ERR_INVALID
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            e2.processImages(128, perm, refstream=True)
        assert ei.value.code == dsac_amd.capi.DSAC_ERR_INVALID
        with pytest.raises(dsac_amd.capi.DsacError):
            e2.processImagesBegin(128, None, soft=np.zeros(128), refstream=True)
        e2.refstreamInit(1305, 2)
        before = e2.sampleRefstreamFrames(8)[1].copy()
        e2.refstreamInit(1305, 2)
        # budgets beyond the window limit (64 windows: the ramp from 256 and then 16 384 each) are refused, not truncated
        inside = sum(256 << k for k in range(6)) + 58 * 16384
        for bad in (inside + 1, 1 << 24, -1):
            with pytest.raises(dsac_amd.capi.DsacError) as ei:
                e2.sampleRefstreamFrames(8, max_attempts=bad)
            assert ei.value.code == dsac_amd.capi.DSAC_ERR_INVALID
        with pytest.raises(dsac_amd.capi.DsacError):
            e2.sampleRefstreamFrames(8, discard0=(1 << 24) + 1)
        with pytest.raises(dsac_amd.capi.DsacError):
            e2.processImages(128, perm, refstream=dict(attempts=1 << 24))
        with pytest.raises(dsac_amd.capi.DsacError):
            e2.set_option("pi_refstream_discard0", -1)
        with pytest.raises(dsac_amd.capi.DsacError):
            e2.set_option("pi_refstream_attempts", -1)
        # none of the refused calls launched anything: the generators are where refstreamInit left them
        assert np.array_equal(e2.sampleRefstreamFrames(8)[1], before)
        # a frame of fewer than 4 cells
        e2.set_frame(xyz[:3], uv[:3], 1, 3, g["cam"])
        e2.set_option("pi_refstream_attempts", 0)
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            e2.processImages(128, synth.fast_permutations(3, 8), refstream=True)
        assert ei.value.code == dsac_amd.capi.DSAC_ERR_INVALID
        with pytest.raises(dsac_amd.capi.DsacError):
            e2.sampleRefstreamFrames(8)
    finally:
        e2.close()
