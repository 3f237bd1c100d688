"""Guided RGB-D sampling on the GPU: dsac_set_sampling_weights_rgbd, dsac_sampling_table_rgbd, the guided draw of dsac_sample_rgbd and
dsac_sampling_weights_backward_rgbd (include/dsac_hip.h has the contract).

The expected side is tests/rgbd_guided_ref.py -- the masked table with np.cumsum(dtype=uint64), the draw with searchsorted, the three-cell walk in Python --
and, for acceptance and poses, the library's own evaluation of GIVEN sets (dsac_sample_rgbd(sets=...), which the weights do not touch): the pattern of
test_gpu_rgbd.py::_walk_frames.  Small maps only; max_tries is passed explicitly everywhere.

    1. the masked table, bit for bit through dsac_sampling_table_rgbd
    2. sets, ok and poses of the guided dsac_sample_rgbd, bit for bit; what the expected side met
    3. lifecycle and refusals
    4. the pipelines
    5. the gradient against a double-precision evaluation of its formula
"""
import numpy as np
import pytest

import guided_ref as gr
import rgbd_guided_ref as g3
import rgbd_ref as rr
from conftest import margin

pytestmark = pytest.mark.gpu

INVALID, NO_FRAME = -1, -4


@pytest.fixture()
def eng(engine):
    engine.set_option("seed_stride", 1)
    yield engine
    engine.set_option("seed_stride", 1)
    if engine.P:
        engine.set_sampling_weights(None)
        if engine.get_option("camera_points"):
            engine.set_sampling_weights_rgbd(None)


def _set(e, H, W, xyz, cam):
    if xyz.shape[0] == 1:
        e.set_frame(xyz[0], None, H, W)
    else:
        e.set_frames(xyz, None, H, W)
    e.set_camera_points(cam)


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------------
def _check_table(e, w, valid):
    F, P = valid.shape
    e.set_sampling_weights_rgbd(w)
    assert e.get_option("sampling_weights_rgbd") == 1
    got = e.sampling_table_rgbd()
    assert got.shape == (F, P) and got.dtype == np.uint64
    for f in range(F):
        want = g3.build_table(w.reshape(F, P)[f], valid[f])[0]
        assert np.array_equal(got[f], want), (f, int(np.flatnonzero(got[f] != want)[0]))
    return got


@pytest.mark.parametrize("H,W", [(3, 5), (40, 40), (37, 53)])
def test_table_bit_for_bit(eng, H, W):
    xyz, cam, v = g3.frame(H, W)
    _set(eng, H, W, xyz, cam)
    assert eng.get_option("sampling_weights_rgbd") == 0
    tables = {}
    for name in (g3.PATTERNS if H * W >= 1600 else g3.SMALL_PATTERNS):
        w = g3.PATTERNS[name](v[0])[None]
        tables[name] = _check_table(eng, w, v)
        masked = g3.masked_weights(w[0], v[0])
        assert not np.diff(np.concatenate([[np.uint64(0)], tables[name][0]]))[~gr.valid_cells(masked)].any()  # no mass on a hole or an invalid weight
    assert np.array_equal(tables["on_holes"], tables["ones"]) and int(tables["ones"][0, -1]) == int(v[0].sum()) << 24
    eng.set_sampling_weights_rgbd(None)
    assert eng.get_option("sampling_weights_rgbd") == 0


def test_table_of_a_batch_whose_middle_frame_has_two_cells(eng):
    H, W = 40, 40
    xyz, cam, v = g3.frame(H, W, frames=3)
    _set(eng, H, W, xyz, cam)
    w = np.stack([g3.w_heavy(v[0]), g3.w_two(v[1]), g3.w_mixed(v[2])])
    got = _check_table(eng, w, v)
    assert int(got[1, -1]) == (1 << 24) + (1 << 23) and got[0, -1] > 0 and got[2, -1] > 0
    # a device tensor only enqueues the build, and the caller may overwrite the buffer afterwards in stream order
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.ExternalStream(eng.stream, device=dev) if eng.stream else torch.cuda.default_stream(dev)
    wd = torch.from_numpy(w).to(dev)
    torch.cuda.synchronize(dev)
    eng.set_sampling_weights_rgbd(None)
    with torch.cuda.stream(st):
        eng.set_sampling_weights_rgbd(wd)
        wd.fill_(7.0)
    assert np.array_equal(eng.sampling_table_rgbd(), got)
    with pytest.raises(ValueError):
        eng.set_sampling_weights_rgbd(np.ones(H * W + 1, np.float32))


# ---- 2. sets, ok and poses ----------------------------------------------------------------------------------------------------------------------------
STATS = dict(redraw=0, undrawn=0, late=0, fail_drawn=0, fail_zero=0)
_EXPECT = {}


def _expected(e, case):
    """the restatement's walk on every frame of the case, acceptance and pose of every attempt from the library's given-sets path on that frame (no weights set)"""
    if case in _EXPECT:
        return _EXPECT[case]
    H, W, F, Nf, A, stride, thr, pats, clean = case
    xyz, cam, v, w = g3.case_inputs(case)
    poses, sets, oks = [], [], []
    for f in range(F):
        C_, T, n, S, m = g3.build_table(w[f], v[f])
        att, _ = g3.attempt_sets3(C_, T, n, g3.SEED + f * stride, Nf, A)
        look = None
        if att is not None:
            flat = np.array([s if s is not None else [0, 0, 0] for row in att for s in row], np.int32)
            e.set_frame(xyz[f], None, H, W)
            e.set_camera_points(cam[f])
            gp, gs, gok = e.sampleRGBD(len(flat), sets=flat, thr=thr)
            assert np.array_equal(gs, flat)
            gp, gok = gp.reshape(Nf, A, 6), gok.reshape(Nf, A)
            look = lambda h, a, s, gp=gp, gok=gok: (bool(gok[h, a]), gp[h, a])
        pf, sf, of, st = g3.sample_frame(w[f], v[f], g3.SEED + f * stride, Nf, A, look)
        for k in STATS:
            STATS[k] += st[k]
        poses.append(pf); sets.append(sf); oks.append(of)
    _EXPECT[case] = (np.concatenate(poses), np.concatenate(sets), np.concatenate(oks))
    return _EXPECT[case]


def _case_id(c):
    return "%dx%d-%dx%d-t%d-s%d-thr%g-%s%s" % (c[1], c[0], c[2], c[3], c[4], c[5], c[6], "+".join(c[7]), "-clean" if c[8] else "")


@pytest.mark.parametrize("case", g3.CASES, ids=_case_id)
def test_guided_sets_are_the_reference_walk_bit_for_bit(eng, case):
    H, W, F, Nf, A, stride, thr, pats, clean = case
    xyz, cam, v, w = g3.case_inputs(case)
    want_p, want_s, want_ok = _expected(eng, case)
    eng.set_option("seed_stride", stride)
    _set(eng, H, W, xyz, cam)
    eng.set_sampling_weights_rgbd(w)
    poses, sets, ok = eng.sampleRGBD(F * Nf, seed=g3.SEED, thr=thr, max_tries=A)
    assert np.array_equal(ok, want_ok), np.flatnonzero(ok != want_ok)[:8]
    assert np.array_equal(sets, want_s), np.flatnonzero((sets != want_s).any(axis=1))[:8]
    assert poses.tobytes() == want_p.tobytes()
    assert not poses[ok == 0].any()
    # every accepted or reported set: VALID cells with mass
    for f in range(F):
        sl = slice(f * Nf, (f + 1) * Nf)
        m = g3.build_table(w[f], v[f])[4]
        rows = sets[sl][sets[sl].any(axis=1) | (ok[sl] == 1)]
        assert v[f][rows].all() and (m[rows] > 0).all()
    if pats == ("lopsided",):
        assert not ok.any() and not sets.any()
    if thr < 1e-6:
        assert not ok.any() and sets.any(axis=1).all()  # nothing accepted: the sets of the last attempt
    if clean:  # exact data: every drawn attempt is accepted, a hypothesis fails only where no attempt drew
        assert np.array_equal(ok == 0, ~sets.any(axis=1))
    if len(pats) == 3:
        assert ok[:Nf].any() and ok[2 * Nf:].any() and not ok[Nf:2 * Nf].any() and not sets[Nf:2 * Nf].any()


def test_the_expected_side_met_every_branch(eng):
    """Reads the expected side only: over the whole parameter list it met a redraw, an attempt without a set, an acceptance in the second round or later, a
    failure with a drawn set and a failure with a zero set."""
    for case in g3.CASES:
        _expected(eng, case)
    print("guided RGB-D expected side:", STATS)
    assert all(STATS[k] > 0 for k in STATS), STATS


# ---- 3. lifecycle and refusals ------------------------------------------------------------------------------------------------------------------------
def _filled(N):
    return np.full((N, 6), 7.5), np.full((N, 3), -3, np.int32), np.full(N, 9, np.uint8)


def _untouched(o):
    return (o[0] == 7.5).all() and (o[1] == -3).all() and (o[2] == 9).all()


def test_lifecycle(eng):
    import dsac_amd
    H, W, N, A = 40, 40, 64, 70
    P = H * W
    xyz3, cam3, v3 = g3.frame(H, W, frames=3)
    xyz, cam, v = xyz3[:1], cam3[:1], v3[:1]
    w = g3.w_mask01(v[0])
    kw = dict(seed=5, thr=60.0, max_tries=A)
    with dsac_amd.Engine(0) as fresh:  # a context that never had weights
        _set(fresh, H, W, xyz, cam)
        never = fresh.sampleRGBD(N, **kw)
        _set(fresh, H, W, xyz3, cam3)
        never3 = fresh.sampleRGBD(3 * N, **kw)
        fresh.set_frame(xyz[0], None, H, W)
        never2d = fresh.sample(N, seed=5, thr=10.0, max_tries=A)
        fresh.set_sampling_weights(w)
        never2d_guided = fresh.sample(N, seed=5, thr=10.0, max_tries=A)
    _set(eng, H, W, xyz, cam)
    eng.set_sampling_weights_rgbd(w)
    guided = eng.sampleRGBD(N, **kw)
    assert guided[2].any() and not np.array_equal(guided[1], never[1]) and (w[guided[1][guided[2] == 1]] > 0).all()
    # given sets, dsac_sample and the 2D guided draw give the same bits with and without the RGB-D weights
    given = eng.sampleRGBD(N, sets=never[1], thr=60.0)
    assert all(np.array_equal(a, b) for a, b in zip(given, never))
    assert all(np.array_equal(a, b) for a, b in zip(eng.sample(N, seed=5, thr=10.0, max_tries=A), never2d))
    # with the 2D weights active as well the RGB-D sampler still refuses, and says why
    eng.set_sampling_weights(w)
    assert eng.get_option("sampling_weights") == 1 and eng.get_option("sampling_weights_rgbd") == 1
    assert all(np.array_equal(a, b) for a, b in zip(eng.sample(N, seed=5, thr=10.0, max_tries=A), never2d_guided))
    o = _filled(N)
    with pytest.raises(dsac_amd.capi.DsacError, match="sampling weights are active") as ei:
        eng.sampleRGBD(N, out=o, **kw)
    assert ei.value.code == INVALID and "dsac_set_sampling_weights_rgbd" in str(ei.value) and _untouched(o)
    eng.set_sampling_weights(None)
    assert all(np.array_equal(a, b) for a, b in zip(eng.sampleRGBD(N, **kw), guided))
    # NULL, new camera points, NULL camera points and every set-frame call clear the weights
    cams3 = np.tile(np.float32([525, 525, 320, 240]), (3, 1))
    clears = ((lambda: eng.set_sampling_weights_rgbd(None), False, never, N),
              (lambda: eng.set_camera_points(cam), False, never, N),
              (lambda: eng.set_camera_points(None), True, never, N),
              (lambda: eng.set_frame(xyz[0], None, H, W), True, never, N),
              (lambda: eng.set_frames(xyz3, None, H, W), True, never3, 3 * N),
              (lambda: eng.set_frames(xyz3, None, H, W, cam=cams3), True, never3, 3 * N))
    for k, (clear, lost_points, want, n) in enumerate(clears):
        _set(eng, H, W, xyz, cam)
        eng.set_sampling_weights_rgbd(w)
        assert eng.get_option("sampling_weights_rgbd") == 1
        clear()
        assert eng.get_option("sampling_weights_rgbd") == 0, k
        if lost_points:
            assert eng.get_option("camera_points") == 0, k
            eng.set_camera_points(cam if n == N else cam3)
            assert eng.get_option("sampling_weights_rgbd") == 0, k
        again = eng.sampleRGBD(n, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(again, want)), k
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            eng.sampling_table_rgbd()
        assert ei.value.code == INVALID
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            eng.sampling_weights_backward_rgbd(again[1], again[2], np.ones(n))
        assert ei.value.code == INVALID
    with pytest.raises(ValueError):
        eng.set_sampling_weights_rgbd(np.ones(P + 1, np.float32))


def test_refusals_leave_the_outputs_alone(eng):
    import ctypes as C
    import dsac_amd
    from dsac_amd.capi import lib, ptr
    H, W, N = 40, 40, 64
    xyz, cam, v = g3.frame(H, W)
    w = np.ones(H * W, np.float32)
    with dsac_amd.Engine(0) as fresh:  # no frame
        assert lib.dsac_set_sampling_weights_rgbd(fresh._ctx, ptr(w)) == NO_FRAME
        assert lib.dsac_set_sampling_weights_rgbd(fresh._ctx, None) == NO_FRAME
        val = C.c_int(-1)
        assert lib.dsac_get_option(fresh._ctx, b"sampling_weights_rgbd", C.byref(val)) == 0 and val.value == 0
        assert lib.dsac_set_option(fresh._ctx, b"sampling_weights_rgbd", 1) != 0  # read-only
    eng.set_frame(xyz[0], None, H, W)  # a frame, no camera points
    for arg in (w, None):
        with pytest.raises(dsac_amd.capi.DsacError, match="camera points") as ei:
            eng.set_sampling_weights_rgbd(arg)
        assert ei.value.code == INVALID
    assert eng.get_option("sampling_weights_rgbd") == 0
    table, grad = np.full((1, H * W), 5, np.uint64), np.full((1, H * W), 2.5)
    o = _filled(N)
    for call in (lambda: eng.sampling_table_rgbd(table), lambda: eng.sampling_weights_backward_rgbd(o[1], o[2], np.ones(N), grad)):
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            call()
        assert ei.value.code == INVALID
    eng.set_camera_points(cam)
    for call in (lambda: eng.sampling_table_rgbd(table), lambda: eng.sampling_weights_backward_rgbd(o[1], o[2], np.ones(N), grad)):
        with pytest.raises(dsac_amd.capi.DsacError) as ei:
            call()
        assert ei.value.code == INVALID
    # bad arguments of the gradient while weights are active
    eng.set_sampling_weights_rgbd(w)
    ctx = eng._ctx
    for n_arg, sets_arg in ((0, ptr(o[1])), (-3, ptr(o[1])), (N, None)):
        assert lib.dsac_sampling_weights_backward_rgbd(ctx, n_arg, sets_arg, ptr(o[2]), ptr(np.ones(N)), ptr(grad)) == INVALID
    assert lib.dsac_sampling_table_rgbd(ctx, None) == INVALID
    assert (table == 5).all() and (grad == 2.5).all() and _untouched(o)


# ---- 4. the pipelines ---------------------------------------------------------------------------------------------------------------------------------
def test_pipelines_keep_displaced_cells_out_of_the_sets(eng):
    from dsac_amd import synth
    H, W, F, N = 40, 40, 3, 64
    P = H * W
    frs = [synth.chess_like_frame_rgbd(H, W, seed=200 + f, noise_mm=5.0, grid_uv=True) for f in range(F)]
    xyz, cam, gt = np.stack([f["xyz"] for f in frs]), np.stack([f["cam_xyz"] for f in frs]).copy(), np.stack([f["gt_pose"] for f in frs])
    gt_jp = np.stack([synth.cv_to_jp6(g) for g in gt])
    w = np.ones((F, P), np.float32)
    moved = np.zeros((F, P), bool)
    for f in range(F):  # a moving object: 30 % of the cells measure a surface half a metre off, and the mask knows them
        idx = np.random.default_rng(40 + f).permutation(P)[:int(0.3 * P)]
        moved[f, idx] = True
        cam[f, idx] += np.float32([500.0, 0.0, 0.0])
        w[f, idx] = 0.0
    singles = []
    for f in range(F):
        eng.set_frame(xyz[f], None, H, W)
        eng.set_camera_points(cam[f])
        eng.set_sampling_weights_rgbd(w[f])
        one = eng.processImageRGBD(N, seed=1305 + f, gt_jp6=gt_jp[f])
        singles.append(one)
        assert one["ok"].any() and not moved[f][one["sampledPoints"][one["ok"] == 1]].any()
        ref = one["refAvgHyp"]
        Ra, Rb = rr.rodrigues(ref[:3]), rr.rodrigues(gt[f][:3])
        ang = np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))
        assert ang <= 5.0 and np.linalg.norm(ref[3:] - gt[f][3:]) <= 50.0
    eng.set_frames(xyz, None, H, W)
    eng.set_camera_points(cam)
    eng.set_sampling_weights_rgbd(w)
    r = eng.processImagesRGBD(N, gt_jp6=gt_jp, seed=1305)
    eng.synchronize()
    sets, ok = r["sampledPoints"].cpu().numpy(), r["ok"].cpu().numpy()
    for f in range(F):
        sl = slice(f * N, (f + 1) * N)
        assert np.array_equal(sets[sl], singles[f]["sampledPoints"]) and np.array_equal(ok[sl], singles[f]["ok"])
        assert not moved[f][sets[sl][ok[sl] == 1]].any()


# ---- 5. the gradient ------------------------------------------------------------------------------------------------------------------------------
def _check_backward(e, w, valid, Nf, sets, ok, g, what):
    """two calls: the second accumulates onto the first.  Per cell |got - ref| <= (n + 4) 2^-53 sum|addends| + P 2^-53 |uniform term| (the last term: the order
    of S'_f's sum), with n, the addends and the uniform term those of both calls together -- the bound of test_gpu_guided.py::_check_backward"""
    F, P = valid.shape
    e.set_sampling_weights_rgbd(w)
    start = np.random.default_rng(1).normal(size=(F, P))
    grad = start.copy()
    out = e.sampling_weights_backward_rgbd(sets, ok, g, grad)
    assert out is grad
    e.sampling_weights_backward_rgbd(sets, ok, 0.5 * g, grad)
    worst = 0.0
    for f in range(F):
        sl = slice(f * Nf, (f + 1) * Nf)
        S = g3.build_table(w[f], valid[f])[3]
        r1, m1, c1, u1 = g3.backward_ref3(w[f], valid[f], S, sets[sl], ok[sl], g[sl])
        r2, m2, c2, u2 = g3.backward_ref3(w[f], valid[f], S, sets[sl], ok[sl], 0.5 * g[sl])
        v = gr.valid_cells(g3.masked_weights(w[f], valid[f]))
        assert np.array_equal(grad[f][~v], start[f][~v]), "cells without mass are exactly unchanged"
        ref = (start[f] + r1) + r2
        mag = np.abs(start[f]) + m1 + m2
        bound = (c1 + c2 + 2 + 4) * 2.0 ** -53 * mag + P * 2.0 ** -53 * (u1 + u2)
        diff = np.abs(grad[f] - ref)
        assert (diff[v] <= bound[v]).all(), (f, int(np.argmax(diff - bound)))
        if np.any(bound[v] > 0):
            worst = max(worst, float((diff[v] / np.where(bound[v] > 0, bound[v], 1.0)).max()))
        assert np.count_nonzero(grad[f][v] != start[f][v]) > 0 or not ok[sl].any()
    margin("g3", "guided RGB-D sampling gradient (%s): worst |got - ref| in units of the per-cell bound" % what, worst, 1.0)


def test_backward_single_frame(eng):
    H, W, N = 40, 40, 96
    xyz, cam, v = g3.frame(H, W)
    _set(eng, H, W, xyz, cam)
    rng = np.random.default_rng(21)
    w = g3.w_mixed(v[0])
    mass = gr.valid_cells(g3.masked_weights(w, v[0]))
    cells = np.flatnonzero(mass)
    sets = rng.choice(cells[:40], size=(N, 3)).astype(np.int32)  # 40 cells shared by many sets
    holes, bad_w = np.flatnonzero(~v[0]), np.flatnonzero(v[0] & ~gr.valid_cells(w))
    sets[::7, 1] = holes[:len(sets[::7])]       # cells that are not VALID inside sets: they receive nothing
    sets[3::7, 2] = bad_w[:len(sets[3::7])]     # VALID cells whose weight has no mass (NaN, -1, inf, 0)
    w[holes[:5]] = 9.0                          # weight on holes counts for nothing
    ok = (rng.random(N) < 0.8).astype(np.uint8)
    g = rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, N)
    assert (ok == 0).any() and len(np.unique(sets)) < 80
    _check_backward(eng, w[None], v, N, sets, ok, g, "one frame, 96 hypotheses")


def test_backward_batch_of_three_and_the_kernels_own_sets(eng):
    H, W, F, Nf = 40, 40, 3, 64
    xyz, cam, v = g3.frame(H, W, frames=F)
    _set(eng, H, W, xyz, cam)
    rng = np.random.default_rng(22)
    w = np.stack([g3.w_heavy(v[0]), g3.w_mixed(v[1]), g3.w_mask01(v[2])])
    sets = np.zeros((F * Nf, 3), np.int32)
    for f in range(F):
        cells = np.flatnonzero(gr.valid_cells(g3.masked_weights(w[f], v[f])))
        sets[f * Nf:(f + 1) * Nf] = rng.choice(cells[:25], size=(Nf, 3))
    sets[5] = (0, 1, 2)
    ok = (rng.random(F * Nf) < 0.7).astype(np.uint8)
    ok[Nf:Nf + 8] = 0
    g = rng.normal(size=F * Nf)
    _check_backward(eng, w, v, Nf, sets, ok, g, "3 frames x 64 hypotheses")
    # the gradient of the sets the guided kernel drew itself
    eng.set_sampling_weights_rgbd(w)
    p, s, okk = eng.sampleRGBD(F * Nf, seed=3, thr=60.0, max_tries=128)
    assert okk.any()
    _check_backward(eng, w, v, Nf, s, okk, g, "3 frames x 64 hypotheses, the sampler's own sets")
