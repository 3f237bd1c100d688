"""Guided sampling on the GPU: dsac_set_sampling_weights, dsac_sampling_table, dsac_sampling_weights_backward (include/dsac_hip.h has the contract).

The expected side is tests/guided_ref.py -- the table with np.cumsum(dtype=uint64), the draw with searchsorted, the redraw loop in Python -- and, for poses,
the library's own evaluation of GIVEN sets (dsac_sample(sets=...): k_eval_sets, which guided sampling does not touch): the restatement's candidate sets of
attempts 0 .. A - 1 of every hypothesis go through one such call, and the first accepted attempt is chosen on the host.  max_tries is passed explicitly (<= 256)
everywhere: a concentrated table can reject every attempt and the default is 2^20.

    1. the table, bit for bit through dsac_sampling_table (sizes around the build's 1 024-cell tile, T past 2^32, a batch with an all-zero frame)
    2. sets, poses and ok of the weighted dsac_sample, bit for bit; rows with ok = 0 by the rule; the oracle as judge of the accepted sets
    3. the whole calls against the weighted dsac_sample with the same seed, scores against dsac_reproject
    4. lifecycle and refusals
    5. the gradient against a double-precision evaluation of its formula
"""
import ctypes as C

import numpy as np
import pytest

import guided_ref as gr
from conftest import margin

pytestmark = pytest.mark.gpu

INVALID, NO_FRAME = -1, -4
THR = 10.0
CAMS3 = np.array([(525.0, 525.0, 320.0, 240.0), (585.0, 585.0, 320.0, 240.0), (260.0, 260.0, 300.0, 250.0)], np.float32)  # the frames' uv are full-image pixels


def _defaults(e):
    for key, v in (("k2_variant", -1), ("k2_flags", 0), ("k2_exact_auto", 1), ("pi_defer_tail", 0), ("pi_refstream", 0), ("k1_horn", 0), ("seed_stride", 1)):
        e.set_option(key, v)


@pytest.fixture()
def eng(engine):
    _defaults(engine)
    yield engine
    _defaults(engine)
    if engine.P:
        engine.set_sampling_weights(None)


# ---- weight patterns -------------------------------------------------------------------------------------------------------------------------
def w_ones(P, mask=None, seed=0):
    return np.ones(P, np.float32)


def w_mask01(P, mask=None, seed=0):
    if mask is not None:
        return mask.astype(np.float32)
    return (np.random.default_rng(100 + seed).random(P) < 0.6).astype(np.float32)


def w_heavy(P, mask=None, seed=0):
    """10^U(-9, 0): hundreds of cells fall below wmax * 2^-24 and get mass 0"""
    return (10.0 ** np.random.default_rng(200 + seed).uniform(-9.0, 0.0, P)).astype(np.float32)


def w_mixed(P, mask=None, seed=0):
    """NaN, -1, +inf and 0 mixed into a positive pattern"""
    rng = np.random.default_rng(300 + seed)
    w = rng.uniform(0.1, 3.0, P).astype(np.float32)
    bad = np.array([np.nan, -1.0, np.inf, 0.0], np.float32)
    idx = rng.permutation(P)[:max(1, P // 3)]
    w[idx] = bad[np.arange(idx.size) % 4]
    return w


def w_zero(P, mask=None, seed=0):
    return np.zeros(P, np.float32)


def w_half(P, mask, seed=0):
    """ones with one inlier cell set to P: it carries half the mass"""
    w = np.ones(P, np.float32)
    w[np.flatnonzero(mask)[len(np.flatnonzero(mask)) // 2]] = np.float32(P)
    return w


def w_three(P, mask, seed=0):
    """three positive cells only: no attempt can succeed"""
    w = np.zeros(P, np.float32)
    w[np.flatnonzero(mask)[[3, 40, 90]]] = (1.0, 2.0, 0.5)
    return w


def w_four_lopsided(P, mask, seed=0):
    """four cells with mass, one of them 16 units against 3 x 2^24: every attempt runs out of candidates (n >= 4, so max_tries is walked)"""
    w = np.zeros(P, np.float32)
    w[np.flatnonzero(mask)[[3, 40, 90, 120]]] = (1.0, 1.0, 1.0, 2.0 ** -20)
    return w


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------------
def _shape_of(P):
    return {1961: (37, 53), 66049: (257, 257)}.get(P, (1, P))


def _set_blank_frames(e, F, P):
    H, W = _shape_of(P)
    xyz = np.zeros((F, P, 3), np.float32)
    if F == 1:
        e.set_frame(xyz[0], None, H, W)
    else:
        e.set_frames(xyz, None, H, W)


def _check_table(e, w, F, P):
    e.set_sampling_weights(w)
    got = e.sampling_table()
    assert got.shape == (F, P) and got.dtype == np.uint64
    for f in range(F):
        C_, T, n, S, m = gr.build_table(w.reshape(F, P)[f])
        assert np.array_equal(got[f], C_), (f, P, int(np.flatnonzero(got[f] != C_)[0]))
    return got


TABLE_SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 1961, 4096, 4097)


@pytest.mark.parametrize("P", TABLE_SIZES)
def test_table_bit_for_bit(eng, P):
    _set_blank_frames(eng, 1, P)
    for i, pat in enumerate((w_ones, w_mask01, w_heavy, w_mixed, w_zero)):
        w = pat(P, None, seed=i)
        got = _check_table(eng, w, 1, P)
        if pat is w_zero:
            assert not got.any()
        if pat is w_heavy and P >= 1961:
            v, m = gr.valid_cells(w), gr.build_table(w)[4]
            assert np.count_nonzero(v & (m == 0)) >= 100, "the heavy tail must send hundreds of valid cells to mass 0"


def test_table_total_passes_2_to_32(eng):
    P = 66049
    _set_blank_frames(eng, 1, P)
    got = _check_table(eng, w_ones(P), 1, P)
    assert int(got[0, -1]) == P << 24 > 1 << 32


def test_table_of_a_batch_with_an_all_zero_frame(eng):
    P, F = 1961, 3
    _set_blank_frames(eng, F, P)
    w = np.stack([w_heavy(P, seed=5), w_zero(P), w_mixed(P, seed=6)])
    got = _check_table(eng, w, F, P)
    assert got[0, -1] > 0 and not got[1].any() and got[2, -1] > 0
    # a device tensor only enqueues the build, and the caller may overwrite the buffer afterwards in stream order
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.ExternalStream(eng.stream, device=dev) if eng.stream else torch.cuda.default_stream(dev)
    wd = torch.from_numpy(w).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(st):
        eng.set_sampling_weights(wd)
        wd.fill_(7.0)
    assert np.array_equal(eng.sampling_table(), got)
    # any float dtype, converted to float32
    eng.set_sampling_weights(w.astype(np.float64))
    assert np.array_equal(eng.sampling_table(), got)


# ---- 2. sets, poses and ok --------------------------------------------------------------------------------------------------------------------
_FRAMES, _EXPECT = {}, {}
STATS = dict(redraws=0, late=0, fail_drawn=0, fail_zero=0)


def _frame(synth, H, W, seed=1305, cam=None):
    key = (H, W, seed, None if cam is None else tuple(cam))
    if key not in _FRAMES:
        _FRAMES[key] = synth.chess_like_frame(H, W, seed=seed) if cam is None else synth.chess_like_frame(H, W, seed=seed, cam=tuple(float(c) for c in cam))
    return _FRAMES[key]


def _expected(e, fr, w, N, seed, A, key):
    """The rule of include/dsac_hip.h on one frame: (poses, sets, ok) of N hypotheses with max_tries = A.  Sets the frame (which clears any weights)."""
    if key in _EXPECT:
        return _EXPECT[key]
    C_, T, n, S, m = gr.build_table(w)
    sets, drawn, redraws = gr.attempt_sets(C_, T, n, seed, N, A)
    e.set_frame(fr["xyz"], fr["uv"], fr["H"], fr["W"], fr["cam"])
    p_all, s_all, ok_all = e.sample(N * A, thr=THR, sets=sets.reshape(-1, 4))
    assert np.array_equal(s_all, sets.reshape(-1, 4))
    ok_all = ok_all.reshape(N, A) & drawn
    p_all = p_all.reshape(N, A, 6)
    poses, out_sets, ok = np.zeros((N, 6)), np.zeros((N, 4), np.int32), np.zeros(N, np.uint8)
    first = np.full(N, -1)
    for h in range(N):
        acc = np.flatnonzero(ok_all[h])
        if acc.size:
            first[h] = acc[0]
            poses[h], out_sets[h], ok[h] = p_all[h, acc[0]], sets[h, acc[0]], 1
        elif n >= 4 and drawn[h, A - 1]:
            out_sets[h] = sets[h, A - 1]
    # what the reference side exercises (never read from the kernel's output)
    STATS["redraws"] += int(np.count_nonzero(redraws))
    STATS["late"] += int(np.count_nonzero(first > 0))
    STATS["fail_drawn"] += int(np.count_nonzero((ok == 0) & out_sets.any(axis=1)))
    STATS["fail_zero"] += int(np.count_nonzero((ok == 0) & ~out_sets.any(axis=1)))
    _EXPECT[key] = (poses, out_sets, ok, first, sets, m)
    return _EXPECT[key]


# (H, W, pattern, N, max_tries): N = 1, 64, 130 and 640 all reach the one guided build (one wave per hypothesis; grid = N); 100 and 130 attempts: a second,
# partial round of 64 lanes; 8 attempts at ~1 accepted in 12: exhausted rows that report the last attempt's set
SINGLE = [(40, 40, w_ones, 64, 64), (40, 40, w_mask01, 130, 100), (40, 40, w_heavy, 64, 64), (40, 40, w_half, 64, 64), (40, 40, w_three, 64, 64),
          (40, 40, w_four_lopsided, 64, 130), (37, 53, w_mask01, 640, 32), (37, 53, w_heavy, 1, 64), (37, 53, w_ones, 130, 8), (37, 53, w_half, 64, 64)]


@pytest.mark.parametrize("H,W,pat,N,A", SINGLE, ids=lambda v: getattr(v, "__name__", str(v)))
def test_weighted_sample_bit_for_bit(eng, synth, orc, H, W, pat, N, A):
    fr = _frame(synth, H, W)
    P, seed = H * W, 1305 + N
    w = pat(P, fr["inlier_mask"], seed=1)
    poses, sets, ok, first, all_sets, m = _expected(eng, fr, w, N, seed, A, (H, W, pat.__name__, N, A))
    eng.set_frame(fr["xyz"], fr["uv"], H, W, fr["cam"])
    eng.set_sampling_weights(w)
    got_p, got_s, got_ok = eng.sample(N, seed=seed, thr=THR, max_tries=A)
    assert np.array_equal(got_ok, ok), np.flatnonzero(got_ok != ok)[:8]
    assert np.array_equal(got_s, sets), np.flatnonzero((got_s != sets).any(axis=1))[:8]
    assert np.array_equal(got_p, poses)
    assert not got_p[ok == 0].any()
    if pat in (w_three, w_four_lopsided):
        assert not ok.any() and not sets.any()
    else:
        assert ok.any()
        assert (m[sets[ok == 1]] > 0).all()
    if pat is w_mask01:  # every cell of every set lies in the mask
        assert fr["inlier_mask"][got_s[got_ok == 1]].all()
    if (H, W, pat, N) == (40, 40, w_mask01, 130):  # the oracle as judge of the accepted sets
        acc = np.flatnonzero(ok)
        pr, sr, okr, _ = orc.sample(acc.size, 0, fr["xyz"], fr["uv"], H, W, fr["cam"], thr=THR, sets=sets[acc])
        assert okr.all()
        rel = (np.abs(got_p[acc] - pr) / (np.abs(pr) + 1e-3)).max(axis=1)
        margin("a1", "guided K1: accepted sets re-solved by the oracle, median relative pose error", np.median(rel), 1e-8)


def _batch3(synth):
    frames = [_frame(synth, 24, 32, seed=300 + f, cam=CAMS3[f]) for f in range(3)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frames]))
    return frames, xyz, uv


@pytest.mark.parametrize("seed_stride", (1, 5))
def test_weighted_sample_on_a_batch_with_a_camera_table(eng, synth, seed_stride):
    """3 x 24 x 32, one camera and one weight pattern per frame, the middle frame without any mass: frame f is the single-frame rule with seed + f * stride"""
    frames, xyz, uv = _batch3(synth)
    P, Nf, A, seed = 24 * 32, 64, 96, 77
    w = np.stack([w_mask01(P, frames[0]["inlier_mask"]), w_zero(P), w_heavy(P, seed=9)])
    exp = [_expected(eng, frames[f], w[f], Nf, seed + f * seed_stride, A, ("batch3", f, seed_stride)) for f in range(3)]
    eng.set_option("seed_stride", seed_stride)
    eng.set_frames(xyz, uv, 24, 32, CAMS3, uv_per_frame=True)
    assert eng.get_option("frame_cams") == 1
    eng.set_sampling_weights(w)
    got_p, got_s, got_ok = eng.sample(3 * Nf, seed=seed, thr=THR, max_tries=A)
    for f in range(3):
        sl = slice(f * Nf, (f + 1) * Nf)
        assert np.array_equal(got_ok[sl], exp[f][2]) and np.array_equal(got_s[sl], exp[f][1]) and np.array_equal(got_p[sl], exp[f][0]), f
    assert got_ok[:Nf].any() and got_ok[2 * Nf:].any()
    assert not got_ok[Nf:2 * Nf].any() and not got_s[Nf:2 * Nf].any() and not got_p[Nf:2 * Nf].any()


def test_the_expected_side_exercised_every_branch(eng, synth, orc):
    """Reads the reference side only: the cases above met redraws, a first accepted attempt > 0, exhausted rows that report a drawn set and rows of zeros."""
    for H, W, pat, N, A in SINGLE:  # whatever the selection ran, the figures are taken over all cases
        fr = _frame(synth, H, W)
        _expected(eng, fr, pat(H * W, fr["inlier_mask"], seed=1), N, 1305 + N, A, (H, W, pat.__name__, N, A))
    print("guided K1 expected side:", STATS)
    assert STATS["redraws"] > 0 and STATS["late"] > 0 and STATS["fail_drawn"] > 0 and STATS["fail_zero"] > 0, STATS


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------------------
def _batch4(synth):
    frames = [_frame(synth, 24, 32, seed=300 + f) for f in range(4)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frames]))
    P = 24 * 32
    w = np.stack([w_mask01(P, frames[0]["inlier_mask"]), w_heavy(P, seed=3), w_half(P, frames[2]["inlier_mask"]), w_ones(P)])
    return frames, xyz, uv, w


def test_whole_calls_draw_by_the_same_rule(eng, synth):
    import torch
    dev = torch.device("cuda", 0)
    frames, xyz, uv, w = _batch4(synth)
    F, N, P, A, seed = 4, 128, 24 * 32, 256, 91
    cam = frames[0]["cam"]
    eng.set_frames(xyz, uv, 24, 32, cam, uv_per_frame=True)
    eng.set_sampling_weights(w)
    ref_p, ref_s, ref_ok = eng.sample(F * N, seed=seed, thr=THR, max_tries=A)
    assert ref_ok.all()
    _, ref_soft = eng.reproject(ref_p, soft=np.zeros(F * N))
    ref_err = np.zeros((F * N, P), np.float32)
    eng.reproject(ref_p, err=ref_err)

    def same(p, s, ok, what):
        assert np.array_equal(np.asarray(ok), ref_ok) and np.array_equal(np.asarray(s), ref_s) and np.array_equal(np.asarray(p), ref_p), what

    # dsac_score_hypotheses_frames
    out = eng.scoreHypothesesFrames(N, seed=seed, thr=THR, max_tries=A)
    same(out[0], out[1], out[2], "dsac_score_hypotheses_frames")
    assert np.array_equal(out[3], ref_soft)
    # dsac_process_images, every "pi_defer_tail" mode, device-resident so that modes 1 and 2 really defer
    perm = torch.from_numpy(synth.fast_permutations(P, 8)).to(dev)
    for mode in (0, 1, 2):
        eng.set_option("pi_defer_tail", mode)
        f64 = dict(dtype=torch.float64, device=dev)
        o = dict(hyps=torch.zeros(F * N, 6, **f64), sampledPoints=torch.zeros(F * N, 4, dtype=torch.int32, device=dev), ok=torch.zeros(F * N, dtype=torch.uint8, device=dev),
                 scores=torch.zeros(F * N, **f64), sfScores=torch.zeros(F * N, **f64), sfEntropy=torch.zeros(F, **f64), avgHyp=torch.zeros(F, 6, **f64),
                 refAvgHyp=torch.zeros(F, 6, **f64), refSteps=torch.zeros(F, dtype=torch.int32, device=dev))
        eng.processImages(N, perm, seed=seed, thr=THR, max_tries=A, out=o)
        eng.joinTail()
        eng.synchronize()
        same(o["hyps"].cpu().numpy(), o["sampledPoints"].cpu().numpy(), o["ok"].cpu().numpy(), "dsac_process_images, pi_defer_tail %d" % mode)
        assert np.array_equal(o["scores"].cpu().numpy(), ref_soft), mode
    eng.set_option("pi_defer_tail", 0)
    # dsac_process_images_begin and its bfloat16 twin
    err = np.zeros((F * N, P), np.float32)
    soft = np.zeros(F * N)
    p, s, ok = eng.processImagesBegin(N, err, seed=seed, thr=THR, max_tries=A, soft=soft)
    same(p, s, ok, "dsac_process_images_begin")
    assert np.array_equal(soft, ref_soft) and np.array_equal(err, ref_err)
    err16 = torch.zeros(F * N, P, dtype=torch.bfloat16, device=dev)
    soft = np.zeros(F * N)
    p, s, ok = eng.processImagesBegin(N, err16, seed=seed, thr=THR, max_tries=A, soft=soft)
    eng.synchronize()
    same(p, s, ok, "dsac_process_images_begin_bf16")
    assert np.array_equal(soft, ref_soft)
    assert eng.get_option("sampling_weights") == 1
    # dsac_score_hypotheses: one frame (frame 2 of the batch, the half-mass table) against the weighted dsac_sample on that frame
    fr = frames[2]
    eng.set_frame(fr["xyz"], fr["uv"], 24, 32, cam)
    eng.set_sampling_weights(w[2])
    p1, s1, ok1 = eng.sample(N, seed=seed + 2, thr=THR, max_tries=A)
    assert np.array_equal(p1, ref_p[2 * N:3 * N]) and np.array_equal(s1, ref_s[2 * N:3 * N])
    out = eng.scoreHypotheses(N, seed=seed + 2, thr=THR, max_tries=A)
    assert np.array_equal(out[0], p1) and np.array_equal(out[1], s1) and np.array_equal(out[2], ok1)
    _, soft1 = eng.reproject(p1, soft=np.zeros(N))
    assert np.array_equal(out[3], soft1)


# ---- 4. lifecycle and refusals --------------------------------------------------------------------------------------------------------------------
def test_lifecycle(eng, synth):
    import dsac_amd
    fr = _frame(synth, 40, 40)
    frames, xyz, uv = _batch3(synth)
    P, N, A = 1600, 64, 64
    w = w_mask01(P, fr["inlier_mask"])

    def set_one():
        eng.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])

    set_one()
    assert eng.get_option("sampling_weights") == 0
    plain = eng.sample(N, seed=5, thr=THR, max_tries=A)
    with dsac_amd.Engine(0) as fresh:  # a context that never had weights
        fresh.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
        never = fresh.sample(N, seed=5, thr=THR, max_tries=A)
    assert all(np.array_equal(a, b) for a, b in zip(plain, never))
    eng.set_sampling_weights(w)
    assert eng.get_option("sampling_weights") == 1
    guided = eng.sample(N, seed=5, thr=THR, max_tries=A)
    assert not np.array_equal(guided[1], plain[1])
    # given sets are unaffected while weights are active
    given = eng.sample(N, thr=THR, sets=plain[1])
    assert np.array_equal(given[0], plain[0]) and np.array_equal(given[1], plain[1]) and np.array_equal(given[2], plain[2])
    # NULL clears, and so does each of the three set-frame calls; afterwards the results are those of a context that never had weights
    def set_shared():
        eng.set_frames(xyz, uv, 24, 32, tuple(float(c) for c in CAMS3[0]), uv_per_frame=True)

    def set_cams():
        eng.set_frames(xyz, uv, 24, 32, CAMS3, uv_per_frame=True)

    with dsac_amd.Engine(0) as fresh:
        never_b = {}
        for name, cam in (("shared", tuple(float(c) for c in CAMS3[0])), ("cams", CAMS3)):
            fresh.set_frames(xyz, uv, 24, 32, cam, uv_per_frame=True)
            never_b[name] = fresh.sample(3 * N, seed=5, thr=THR, max_tries=A)
    for k, (clear, want, n) in enumerate(((lambda: eng.set_sampling_weights(None), never, N), (set_one, never, N), (set_shared, never_b["shared"], 3 * N),
                                          (set_cams, never_b["cams"], 3 * N))):
        set_one()
        eng.set_sampling_weights(w)
        assert eng.get_option("sampling_weights") == 1
        clear()
        assert eng.get_option("sampling_weights") == 0, k
        again = eng.sample(n, seed=5, thr=THR, max_tries=A)
        assert all(np.array_equal(a, b) for a, b in zip(again, want)), k
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            eng.sampling_table()
        assert ei.value.code == INVALID
    # weights set on a batch are cleared by the single-frame call as well
    set_cams()
    eng.set_sampling_weights(np.ones((3, 24 * 32), np.float32))
    assert eng.get_option("sampling_weights") == 1 and eng.get_option("frame_cams") == 1
    set_one()
    assert eng.get_option("sampling_weights") == 0
    assert all(np.array_equal(a, b) for a, b in zip(eng.sample(N, seed=5, thr=THR, max_tries=A), never))
    with pytest.raises(ValueError):
        eng.set_sampling_weights(np.ones(P + 1, np.float32))


def test_refusals_leave_the_outputs_alone(eng, synth):
    import torch
    import dsac_amd
    from dsac_amd.capi import lib, ptr
    dev = torch.device("cuda", 0)
    fr = _frame(synth, 40, 40)
    P, N, A = 1600, 128, 64
    eng.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    eng.set_sampling_weights(w_mask01(P, fr["inlier_mask"]))

    def filled():
        return np.full((N, 6), 7.5), np.full((N, 4), -3, np.int32), np.full(N, 9, np.uint8)

    def untouched(o):
        return (o[0] == 7.5).all() and (o[1] == -3).all() and (o[2] == 9).all()

    def refused(call, word):
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            call()
        assert ei.value.code == INVALID and word in str(ei.value) and "sampling weights" in str(ei.value), str(ei.value)

    # the reference-stream calls and "pi_refstream" = 1
    eng.refstreamInit(1305, 2)
    o = filled()
    refused(lambda: eng.sampleRefstream(N, thr=THR, max_attempts=4096, out=o), "dsac_sample_refstream")
    refused(lambda: eng.sampleRefstreamFrames(N, thr=THR, out=o), "dsac_sample_refstream_frames")
    err = np.full((N, P), 3.0, np.float32)
    eng.set_option("pi_refstream", 1)
    refused(lambda: eng.processImagesBegin(N, err, seed=1, thr=THR, max_tries=A, out=o), "pi_refstream")
    perm = synth.fast_permutations(P, 8)
    res = dict(hyps=o[0], sampledPoints=o[1], ok=o[2])
    refused(lambda: eng.processImages(N, perm, seed=1, thr=THR, max_tries=A, out=res), "pi_refstream")
    eng.set_option("pi_refstream", 0)
    assert untouched(o) and (err == 3.0).all()
    # dsac_sample_ahead
    dp, ds, dok = torch.full((N, 6), 7.5, dtype=torch.float64, device=dev), torch.full((N, 4), -3, dtype=torch.int32, device=dev), torch.full((N,), 9, dtype=torch.uint8, device=dev)
    refused(lambda: eng.sampleAhead(0, N, 1, dp, ds, dok, thr=THR, max_tries=A), "dsac_sample_ahead")
    torch.cuda.synchronize(dev)
    assert untouched((dp.cpu().numpy(), ds.cpu().numpy(), dok.cpu().numpy()))
    # "k1_horn" = 1 in every call that draws; given sets still pass
    eng.set_option("k1_horn", 1)
    refused(lambda: eng.sample(N, seed=1, thr=THR, max_tries=A, out=o), "k1_horn")
    refused(lambda: eng.scoreHypotheses(N, seed=1, thr=THR, max_tries=A, out=o + (np.zeros(N), np.zeros(N), np.zeros(1), np.zeros(6))), "k1_horn")
    refused(lambda: eng.processImagesBegin(N, err, seed=1, thr=THR, max_tries=A, out=o), "k1_horn")
    refused(lambda: eng.processImages(N, perm, seed=1, thr=THR, max_tries=A, out=res), "k1_horn")
    assert untouched(o) and (err == 3.0).all()
    eng.sample(4, thr=THR, sets=np.arange(16, dtype=np.int32).reshape(4, 4) * 7)
    eng.set_option("k1_horn", 0)
    eng.sample(N, seed=1, thr=THR, max_tries=A, out=o)
    assert not untouched(o)
    # the gradient and the table need active weights; a context without a frame has none to set
    eng.set_sampling_weights(None)
    with pytest.raises(dsac_amd.capi.DsacError) as ei:
        eng.sampling_weights_backward(o[1], o[2], np.ones(N))
    assert ei.value.code == INVALID
    with dsac_amd.Engine(0) as fresh:
        w = np.ones(P, np.float32)
        assert lib.dsac_set_sampling_weights(fresh._ctx, ptr(w)) == NO_FRAME
        assert lib.dsac_set_sampling_weights(fresh._ctx, None) == NO_FRAME
        v = C.c_int(-1)
        assert lib.dsac_get_option(fresh._ctx, b"sampling_weights", C.byref(v)) == 0 and v.value == 0


# ---- 5. the gradient ------------------------------------------------------------------------------------------------------------------------------
def _check_backward(e, w, F, P, Nf, sets, ok, g, what):
    """two calls: the second accumulates onto the first.  Per cell |got - ref| <= (n + 4) 2^-53 sum|addends| + P 2^-53 |uniform term| (the last term: the order
    of S_f's sum), with n, the addends and the uniform term those of both calls together"""
    e.set_sampling_weights(w)
    start = np.random.default_rng(1).normal(size=(F, P))
    grad = start.copy()
    out = e.sampling_weights_backward(sets, ok, g, grad)
    assert out is grad
    e.sampling_weights_backward(sets, ok, 0.5 * g, grad)
    worst = 0.0
    for f in range(F):
        sl = slice(f * Nf, (f + 1) * Nf)
        S = gr.build_table(w[f])[3]
        r1, m1, c1, u1 = gr.backward_ref(w[f], S, sets[sl], ok[sl], g[sl])
        r2, m2, c2, u2 = gr.backward_ref(w[f], S, sets[sl], ok[sl], 0.5 * g[sl])
        v = gr.valid_cells(w[f])
        assert np.array_equal(grad[f][~v], start[f][~v]), "invalid cells are exactly unchanged"
        ref = (start[f] + r1) + r2
        mag = np.abs(start[f]) + m1 + m2
        bound = (c1 + c2 + 2 + 4) * 2.0 ** -53 * mag + P * 2.0 ** -53 * (u1 + u2)
        diff = np.abs(grad[f] - ref)
        assert (diff[v] <= bound[v]).all(), (f, int(np.argmax(diff - bound)))
        if np.any(bound[v] > 0):
            worst = max(worst, float((diff[v] / np.where(bound[v] > 0, bound[v], 1.0)).max()))
        assert np.count_nonzero(grad[f][v] != start[f][v]) > 0 or not ok[sl].any()
    margin("g1", "guided sampling gradient (%s): worst |got - ref| in units of the per-cell bound" % what, worst, 1.0)


def test_backward_single_frame(eng, synth):
    fr = _frame(synth, 40, 40)
    P, N = 1600, 96
    rng = np.random.default_rng(21)
    w = w_mixed(P, seed=4)
    valid = np.flatnonzero(gr.valid_cells(w))
    sets = rng.choice(valid[:40], size=(N, 4)).astype(np.int32)   # 40 cells shared by many sets
    sets[::7, 1] = np.flatnonzero(~gr.valid_cells(w))[:len(sets[::7])]  # invalid cells inside sets: they receive nothing
    ok = (rng.random(N) < 0.8).astype(np.uint8)
    g = rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, N)
    eng.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    assert (ok == 0).any() and len(np.unique(sets)) < 80
    _check_backward(eng, w[None], 1, P, N, sets, ok, g, "one frame, 96 hypotheses")


def test_backward_batch_of_three(eng, synth):
    frames, xyz, uv = _batch3(synth)
    P, Nf, F = 24 * 32, 64, 3
    rng = np.random.default_rng(22)
    w = np.stack([w_heavy(P, seed=9), w_mixed(P, seed=8), w_mask01(P, frames[2]["inlier_mask"])])
    eng.set_frames(xyz, uv, 24, 32, CAMS3, uv_per_frame=True)
    sets = np.zeros((F * Nf, 4), np.int32)
    for f in range(F):
        valid = np.flatnonzero(gr.valid_cells(w[f]))
        sets[f * Nf:(f + 1) * Nf] = rng.choice(valid[:25], size=(Nf, 4))
    sets[5] = (0, 1, 2, 3)
    ok = (rng.random(F * Nf) < 0.7).astype(np.uint8)
    ok[Nf:Nf + 8] = 0
    g = rng.normal(size=F * Nf)
    _check_backward(eng, w, F, P, Nf, sets, ok, g, "3 frames x 64 hypotheses")
    # the gradient of the sets the guided K1 drew itself
    eng.set_sampling_weights(w)
    p, s, okk = eng.sample(F * Nf, seed=3, thr=THR, max_tries=128)
    _check_backward(eng, w, F, P, Nf, s, okk, g, "3 frames x 64 hypotheses, K1's own sets")
