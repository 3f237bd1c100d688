"""K4 on half-precision gradient images: dsac_score_backward_f16 (k_score_backward_mfma<.., _Float16>) and dsac_soft_score_derr_f16.

The contract: the half call is the float call on the widened values -- the same launch plan, the same summation orders, an exact conversion (subnormal halves
included) --, so with grad_xyz zeroed beforehand gradient and pose sums are equal bit for bit; whatever the matrix-core form cannot do is refused by name
before anything is staged or enqueued.  The yardstick is the float call on the same values; one comparison goes to the oracle.

Bit-for-bit needs an order-independent float call.  The main pass adds at most two fp64 atomics per cell (they commute on a zero); the support scatter adds
one more per hypothesis that has the cell in its minimal set, so the identity tests draw minimal sets that share no cell (`_unique_sets`; clean frames, so
that any set gives a sane pose).  Where sampled sets share cells (the torch-free chain) the bound is the project's 1e-12 for fp64 atomics on shared support
cells (tests/test_gpu_backward_batch.py), and 1e-5 of the largest entry where two launches group their fp32 partial sums by different tiles (ibid.)."""
import numpy as np
import pytest

from conftest import margin

pytestmark = pytest.mark.gpu

# +-0, +-2^-24 (the smallest subnormal), +-the largest subnormal, 2^-14 (the smallest normal), +-65504
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF], np.uint16)
_CACHE = {}


def _halves(N, P, seed):
    """N x P halves from a normal sample with every special value at three cells of every row."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((N, P)).astype(np.float16)
    bits = d.view(np.uint16)
    cols = np.stack([rng.choice(P, 3 * len(SPECIALS), replace=False) for _ in range(N)])
    bits[np.arange(N)[:, None], cols] = np.tile(SPECIALS, 3)[None, :]
    return d


def _unique_sets(N, P, seed):
    return np.random.default_rng(seed).permutation(P)[:4 * N].reshape(N, 4).astype(np.int32)


def _case(engine, synth, H, W, sampled, N):
    """(frame, poses, sets, halves) for one shape, made once, shared and left unchanged; the frame is set in the engine."""
    key = (H, W, sampled, N)
    fr = _CACHE.setdefault((H, W, sampled), synth.chess_like_frame(H, W, seed=1305 + H + W, noise_mm=1.0, outlier_frac=0.0, grid_uv=not sampled))
    engine.set_frame(fr["xyz"], fr["uv"] if sampled else None, H, W, fr["cam"])
    if key not in _CACHE:
        sets = _unique_sets(N, H * W, N)
        poses, sets_out, _ = engine.sample(N, sets=sets, thr=10.0)
        assert np.array_equal(sets_out, sets) and np.isfinite(poses).all()
        _CACHE[key] = (poses, sets, _halves(N, H * W, 7 * N + H))
    return (fr,) + _CACHE[key]


def _both(engine, poses, sets, d16, **kw):
    N = sets.shape[0]
    g16 = engine.dScore(poses, sets, d16, **kw)
    p16 = engine.lastPoseGradients(N)
    g32 = engine.dScore(poses, sets, d16.astype(np.float32), **kw)
    p32 = engine.lastPoseGradients(N)
    assert np.isfinite(g32).all() and np.abs(g32).max() > 0
    return g16, p16, g32, p32


def _assert_identical(g16, p16, g32, p32):
    bad = np.argwhere(g16 != g32)
    assert bad.size == 0, "%d gradient entries differ, first %s: %r against %r" % (len(bad), tuple(bad[0]), g16[tuple(bad[0])], g32[tuple(bad[0])])
    assert np.array_equal(g16, g32) and np.array_equal(p16, p32)


# ---- identity with the float call on the widened values --------------------------------------------------------------------------------------
# 40 x 40 sampled: the small-map plan, 2 chunks (N = 40: ragged last group; N = 272: more than 256 hypotheses, grad_part + the reduction); 38 high x 42 wide
# sampled: 1 596 cells, the last chunk partly beyond the map; 36 x 44 implicit grid (UV = false); 416 high x 320 wide implicit: 133 120 cells = 520 tiles
# of 4 chunks on 512 persistent workgroups (the big-map plan, tiles split between two workgroups, gradient through fp64 atomics)
@pytest.mark.parametrize("H,W,sampled,N", [(40, 40, True, 64), (40, 40, True, 40), (40, 40, True, 272), (38, 42, True, 64), (36, 44, False, 64),
                                           (416, 320, False, 40)])
def test_identical_to_the_float_call(engine, synth, H, W, sampled, N):
    _, poses, sets, d16 = _case(engine, synth, H, W, sampled, N)
    _assert_identical(*_both(engine, poses, sets, d16))


def test_identical_with_the_transposed_index(engine, synth):
    _, poses, sets, d16 = _case(engine, synth, 40, 40, True, 64)
    _assert_identical(*_both(engine, poses, sets, d16, quirk_transpose=True))


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [False, True])
def test_parity_with_the_oracle(engine, orc, frame40, quirk):
    fr, N = frame40, 64
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    poses, sets, _, _ = orc.sample(N, 5, fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    d16 = _halves(N, 1600, 1)
    ref, _, _ = orc.dScore(sets, d16.astype(np.float64), fr["xyz"], fr["uv"], 40, 40, fr["cam"], quirk_transpose=quirk)
    J = np.stack([orc.dPNP(fr["uv"][s_], fr["xyz"][s_], fr["cam"]) for s_ in sets])  # the same dPNP on both sides, as tests/test_gpu_backward.py
    got = engine.dScore(poses, sets, d16, dpnp=J, quirk_transpose=quirk)
    margin("a12", "dScore on half gradient images 40x40 (index quirk on/off): gradient max-rel vs oracle", np.abs(got - ref).max() / np.abs(ref).max(), 1e-3)
    margin("a12", "dScore on half gradient images 40x40 (index quirk on/off): gradient relative l2 error", np.linalg.norm(got - ref) / np.linalg.norm(ref), 5e-4)


# ---- frame batches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nf", [32, 24])
def test_frame_batches(engine, synth, Nf):
    """Nf = 32: one launch for the batch; Nf = 24 (16 does not divide it): frame by frame inside the call."""
    H = W = 40
    F, P = 3, 1600
    frames = [synth.chess_like_frame(H, W, seed=420 + f, noise_mm=1.0, outlier_frac=0.0) for f in range(F)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frames]))
    cam = frames[0]["cam"]
    ps, ss = [], []
    for f in range(F):
        engine.set_frame(xyz[f], uv[f], H, W, cam)
        sets = _unique_sets(Nf, P, 50 + f)
        ps.append(engine.sample(Nf, sets=sets)[0]); ss.append(sets)
    poses, sets = np.concatenate(ps), np.concatenate(ss)
    d16 = _halves(F * Nf, P, Nf)
    engine.set_frames(xyz, uv, H, W, cam, uv_per_frame=True)
    engine.profile_enable(True, stride=1)
    engine.profile_read(1, reset=True)
    g16 = engine.dScore(poses, sets, d16)
    _, launches = engine.profile_read(1, reset=True)
    engine.profile_enable(False)
    assert launches == (1 if Nf % 16 == 0 else F)  # the K4 profile scope counts the half call's main passes
    p16 = engine.lastPoseGradients(F * Nf)
    g32 = engine.dScore(poses, sets, d16.astype(np.float32))
    _assert_identical(g16, p16, g32, engine.lastPoseGradients(F * Nf))
    assert g16.shape == (F * P, 3)
    for f in range(F):
        hs, cs = slice(f * Nf, (f + 1) * Nf), slice(f * P, (f + 1) * P)
        engine.set_frame(xyz[f], uv[f], H, W, cam)
        g1 = engine.dScore(poses[hs], sets[hs], d16[hs])
        p1 = engine.lastPoseGradients(Nf)
        if Nf % 16 == 0:  # the batch's tile is the frame's 32 hypotheses, the single frame's small-map plan has tiles of 16: fp32 partial sums grouped otherwise
            margin("a15", "half frame batch in one launch vs single-frame half calls, K4 gradient: max |d| / max |g|", np.abs(g16[cs] - g1).max() / np.abs(g1).max(), 1e-5)
            margin("a10", "half frame batch in one launch vs single-frame half calls, pose sums: max |d| / max |G6|", np.abs(p16[hs] - p1).max() / np.abs(p1).max(), 1e-5)
        else:  # the same launches as the single-frame calls
            assert np.array_equal(g16[cs], g1) and np.array_equal(p16[hs], p1)


# ---- argument kinds and modes --------------------------------------------------------------------------------------------------------------------
def test_host_and_device_halves_give_equal_results(engine, synth):
    import torch
    _, poses, sets, d16 = _case(engine, synth, 40, 40, True, 64)
    g_host = engine.dScore(poses, sets, d16)
    p_host = engine.lastPoseGradients(64)
    dev = torch.device("cuda", 0)
    d_dev = torch.from_numpy(d16).to(dev)
    grad = torch.zeros(1600, 3, dtype=torch.float64, device=dev)
    engine.dScore(torch.from_numpy(poses).to(dev), torch.from_numpy(sets).to(dev), d_dev, grad=grad)
    p_dev = engine.lastPoseGradients(64)
    engine.synchronize()
    assert np.array_equal(grad.cpu().numpy(), g_host) and np.array_equal(p_dev, p_host)


def test_the_staged_form(engine, synth):
    _, poses, sets, d16 = _case(engine, synth, 36, 44, False, 64)
    g_auto = engine.dScore(poses, sets, d16)
    engine.set_option("k4_variant", 1999)
    try:
        g16, p16, g32, p32 = _both(engine, poses, sets, d16)
    finally:
        engine.set_option("k4_variant", -1)
    _assert_identical(g16, p16, g32, p32)
    assert np.abs(g16 - g_auto).max() <= 1e-5 * np.abs(g_auto).max()  # the two stagings group the fp32 partial sums differently


def test_accumulates(engine, synth):
    _, poses, sets, d16 = _case(engine, synth, 40, 40, True, 64)
    g0 = engine.dScore(poses, sets, d16)
    g1 = engine.dScore(poses, sets, d16, grad=g0.copy())
    assert np.allclose(g1, 2 * g0, rtol=1e-6, atol=1e-9 * np.abs(g0).max())


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
PATTERN = 12345.0


def _off_by(n_bytes, count, dtype):
    """`count` elements of dtype whose first byte sits n_bytes past a 16-byte address; returns (array, keep-alive)."""
    item = np.dtype(dtype).itemsize
    buf = np.zeros(count + 32 // item, dtype)
    start = ((-buf.ctypes.data) % 16 + n_bytes) // item
    a = buf[start:start + count]
    assert a.ctypes.data % 16 == n_bytes
    return a, buf


@pytest.mark.parametrize("case", ["NULL", "parity", "writeback", "37x53", "xyz off the grid", "uv off the grid", "implicit grid 38x42", "d_err16 off by 2 bytes",
                                  "k4_variant 0", "k4_variant 1020", "fx != fy"])
def test_refusals(engine, synth, case):
    import torch
    from dsac_amd import capi
    lib, ptr = capi.lib, capi.ptr
    H, W, cam, sampled, flags = 40, 40, synth.CAM_7SCENES, True, 0
    if case == "37x53":
        H, W = 37, 53
    elif case == "implicit grid 38x42":
        H, W, sampled = 38, 42, False  # 1 596 cells: H*W % 4 == 0, W % 4 == 2
    elif case == "fx != fy":
        cam = (525.0, 520.0, 320.0, 240.0)
    elif case == "parity":
        flags = capi.DSAC_BWD_PARITY_FP64
    elif case == "writeback":
        flags = capi.DSAC_BWD_PARITY_FP64 | capi.DSAC_BWD_QUIRK_ROT_WRITEBACK
    N, P = 32, H * W
    fr = synth.chess_like_frame(H, W, seed=5, cam=cam, noise_mm=1.0, outlier_frac=0.0, grid_uv=not sampled)
    dev = torch.device("cuda", 0)
    keep = []
    # poses and dPNP from the frame on the engine's own (aligned) copy; the float call is handed this dPNP, so that only K4 reads a frame off the grid
    engine.set_frame(fr["xyz"], fr["uv"] if sampled else None, H, W, cam)
    sets = _unique_sets(N, P, 3)
    poses = np.ascontiguousarray(engine.sample(N, sets=sets)[0])
    J = np.ascontiguousarray(engine.dPNP(sets))
    if case in ("xyz off the grid", "uv off the grid"):  # a borrowed device frame, one float past a 16-byte address
        def place(a, off):
            t = torch.zeros(a.size + 4, dtype=torch.float32, device=dev)
            t[off:off + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
            keep.append(t)
            return t[off:off + a.size]
        xyz_t, uv_t = place(fr["xyz"], 1 if case.startswith("xyz") else 0), place(fr["uv"], 1 if case.startswith("uv") else 0)
        assert (xyz_t.data_ptr() % 16 != 0) == case.startswith("xyz") and (uv_t.data_ptr() % 16 != 0) == case.startswith("uv")
        engine.set_frame(xyz_t, uv_t, H, W, cam, borrow=True)
    try:
        d32 = _halves(N, P, 2).astype(np.float32)
        float_runs = case != "fx != fy"
        if float_runs:  # a float call first: the count and the sums a refused call must leave behind
            engine.dScore(poses, sets, d32, dpnp=J)
            G6_before = engine.lastPoseGradients(N)
        d16, hold = _off_by(2 if case == "d_err16 off by 2 bytes" else 0, N * P, np.float16)
        d16[:] = d32.reshape(-1).astype(np.float16)
        if case.startswith("k4_variant"):
            engine.set_option("k4_variant", int(case.split()[1]))
        grad = np.full((P, 3), PATTERN)
        rc = lib.dsac_score_backward_f16(engine._ctx, N, ptr(poses), ptr(sets), None if case == "NULL" else d16.ctypes.data, None, flags, ptr(grad))
        assert rc == capi.DSAC_ERR_INVALID, case
        msg = lib.dsac_last_error(engine._ctx).decode()
        assert msg.startswith("dsac_score_backward_f16:") and len(msg) > 35, msg
        engine.synchronize()
        assert bool((grad == PATTERN).all()), "a refused call wrote into grad_xyz"
        if float_runs:
            assert np.array_equal(engine.lastPoseGradients(N), G6_before)
            with pytest.raises(capi.DsacError):
                engine.lastPoseGradients(N + 1)
        # the float call on the same frame, options and flags runs (or is refused) as before
        g = np.zeros((P, 3))
        rc = lib.dsac_score_backward(engine._ctx, N, ptr(poses), ptr(sets), ptr(d32), ptr(J), flags, ptr(g))
        assert rc == (capi.DSAC_OK if float_runs else capi.DSAC_ERR_INVALID), (case, lib.dsac_last_error(engine._ctx).decode())
        if float_runs:
            assert np.isfinite(g).all() and np.abs(g).max() > 0
    finally:
        engine.set_option("k4_variant", -1)
        engine.set_frame(fr["xyz"], fr["uv"], H, W, cam)  # nothing borrowed is left behind
        engine.synchronize()


@pytest.mark.parametrize("case", ["batch of 37x53", "batch with xyz off the grid", "batch with d_err16 off by 4 bytes"])
def test_refusals_on_a_frame_batch(engine, synth, case):
    """The refusal looks at every frame of a batch.  (With H*W % 4 == 0 the frames of a batch lie 16 | H*W * 12 bytes apart, so they leave the 16-byte grid together.)"""
    import torch
    from dsac_amd import capi
    lib, ptr = capi.lib, capi.ptr
    H, W = (37, 53) if case == "batch of 37x53" else (40, 40)
    F, Nf, P, cam = 2, 32, H * W, synth.CAM_7SCENES
    frames = [synth.chess_like_frame(H, W, seed=60 + f, noise_mm=1.0, outlier_frac=0.0) for f in range(F)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    uv = frames[0]["uv"]
    ps, ss = [], []
    for f in range(F):
        engine.set_frame(xyz[f], uv, H, W, cam)
        sets = _unique_sets(Nf, P, 70 + f)
        ps.append(engine.sample(Nf, sets=sets)[0]); ss.append(sets)
    poses, sets = np.ascontiguousarray(np.concatenate(ps)), np.ascontiguousarray(np.concatenate(ss))
    dev = torch.device("cuda", 0)
    off = 1 if case == "batch with xyz off the grid" else 0
    buf = torch.zeros(xyz.size + 4, dtype=torch.float32, device=dev)
    xyz_t = buf[off:off + xyz.size]
    xyz_t.copy_(torch.from_numpy(xyz.reshape(-1)).to(dev))
    uv_t = torch.from_numpy(uv).to(dev)
    assert (xyz_t.data_ptr() % 16 != 0) == bool(off)
    try:
        engine.set_frames(xyz_t.view(F, P, 3), uv_t, H, W, cam, borrow=True)
        d16, hold = _off_by(4 if case.endswith("4 bytes") else 0, F * Nf * P, np.float16)
        d16[:] = _halves(F * Nf, P, 9).reshape(-1)
        grad = np.full((F * P, 3), PATTERN)
        rc = lib.dsac_score_backward_f16(engine._ctx, F * Nf, ptr(poses), ptr(sets), d16.ctypes.data, None, 0, ptr(grad))
        assert rc == capi.DSAC_ERR_INVALID, case
        assert lib.dsac_last_error(engine._ctx).decode().startswith("dsac_score_backward_f16:")
        engine.synchronize()
        assert bool((grad == PATTERN).all()), "a refused call wrote into grad_xyz"
        if not off and not case.endswith("4 bytes"):
            return
        # the same batch on the grid runs, and equals the float call
        engine.set_frames(xyz, uv, H, W, cam)
        d_ok = d16.reshape(F * Nf, P).copy()
        assert d_ok.ctypes.data % 8 == 0
        _assert_identical(*_both(engine, poses, sets, d_ok))
    finally:
        engine.set_frame(frames[0]["xyz"], uv, H, W, cam)  # nothing borrowed is left behind
        engine.synchronize()


def test_the_python_layer_refuses_the_parity_mode_in_half(engine, synth):
    _, poses, sets, d16 = _case(engine, synth, 40, 40, True, 64)
    from dsac_amd import capi
    with pytest.raises(ValueError):
        engine.dScore(poses, sets, d16, parity_fp64=True)
    assert capi.lib.dsac_score_backward_f16(None, 64, capi.ptr(poses), capi.ptr(sets), capi.ptr(d16), None, 0, None) == capi.DSAC_ERR_INVALID  # no context


# ---- the gradient images of the soft-inlier score in half --------------------------------------------------------------------------------------------
TAU, BETA, CLAMP = 10.0, 0.5, 100.0


def test_soft_score_derr_in_half(engine, frame40):
    from dsac_amd import capi
    lib, ptr = capi.lib, capi.ptr
    fr, N, P = frame40, 64, 1600
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    poses, _, _ = engine.sample(N, seed=77, thr=10.0, max_tries=1 << 16)
    err16 = np.zeros((N, P), np.float16)
    engine.reproject(poses, err=err16)
    rng = np.random.default_rng(4)
    g = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-6.0, 0.0, N)  # |d_err| <= |g| beta / 4: rows from 1e-1 down into the half subnormals and below
    want32 = np.zeros((N, P), np.float32)
    engine.softScoreDErr(g, err16.astype(np.float32), want32, tau=TAU, beta=BETA, clamp=CLAMP)
    want = want32.astype(np.float16).view(np.uint16)
    got16 = np.full((N, P), 0x5A5A, np.uint16).view(np.float16)
    assert engine.softScoreDErr(g, err16, got16, tau=TAU, beta=BETA, clamp=CLAMP) is got16
    got = got16.view(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d cells differ, first %s: %#x against %#x" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    subnormal = ((got & 0x7C00) == 0) & ((got & 0x03FF) != 0)
    normal = (got & 0x7C00) != 0
    assert subnormal.sum() > 100 and normal.sum() > 100, (int(subnormal.sum()), int(normal.sum()))
    on_clamp = err16 == np.float16(CLAMP)
    assert on_clamp.sum() > 0 and not got[on_clamp].any()
    # refusals: a NULL pointer, a pointer off the 8-byte grid, a map with H*W % 4 != 0
    ctx = engine._ctx
    off, hold = _off_by(2, N * P, np.float16)
    for args in ((None, ptr(got16)), (ptr(err16), None), (off.ctypes.data, ptr(got16)), (ptr(err16), off.ctypes.data)):
        assert lib.dsac_soft_score_derr_f16(ctx, N, ptr(g), args[0], CLAMP, TAU, BETA, args[1]) == capi.DSAC_ERR_INVALID
        assert lib.dsac_last_error(ctx).decode().startswith("dsac_soft_score_derr_f16:")
    engine.synchronize()
    assert np.array_equal(got16.view(np.uint16), want) and not hold.any()
    engine.set_frame(np.zeros((37 * 53, 3), np.float32) + 1000.0, None, 37, 53, fr["cam"])
    assert lib.dsac_soft_score_derr_f16(ctx, 1, ptr(g), ptr(err16), CLAMP, TAU, BETA, ptr(got16)) == capi.DSAC_ERR_INVALID


def test_the_torch_free_chain(synth):
    """dsac_process_images_begin_f16 -> dsac_soft_score_derr_f16 -> dsac_score_backward_f16 on host arrays: the whole seam in half without device code of the
    caller's.  Sampled minimal sets share cells, so the gradient is compared to the last bit of the fp64 atomics (1e-12, as the float batches are)."""
    import dsac_amd
    H = W = 40
    F, N, P = 2, 128, 1600
    frames = [synth.chess_like_frame(H, W, seed=700 + f, quantise_int16=True) for f in range(F)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    with dsac_amd.Engine(0) as e:
        e.set_frames(xyz, frames[0]["uv"], H, W, frames[0]["cam"])
        err16 = np.zeros((F * N, P), np.float16)
        soft = np.zeros(F * N)
        poses, sets, ok = e.processImagesBegin(N, err16, seed=91, soft=soft)
        assert ok.all() and e.k2_form() == ("exact (vector build)", 0)
        g = np.random.default_rng(8).standard_normal(F * N)
        d16 = e.softScoreDErr(g, err16, np.zeros((F * N, P), np.float16), tau=TAU, beta=BETA)
        assert np.abs(d16.astype(np.float32)).max() > 0
        g16 = e.dScore(poses, sets, d16)
        p16 = e.lastPoseGradients(F * N)
        g32 = e.dScore(poses, sets, d16.astype(np.float32))
        p32 = e.lastPoseGradients(F * N)
    assert g16.shape == (F * P, 3) and np.abs(g32).max() > 0
    margin("a15", "the seam in half on host arrays: K4 on half gradient images vs the float K4 on the widened values, max |d| / max |g|",
           np.abs(g16 - g32).max() / np.abs(g32).max(), 1e-12)
    assert np.array_equal(p16, p32)


# ---- ScoredFrameBatch ----------------------------------------------------------------------------------------------------------------------------
def test_scored_frame_batch_hands_k4_the_halves(synth, orc):
    import torch
    from dsac_amd import e2e
    from test_gpu_err_f16 import GRAD_REL_MEASURED
    S, F, N, sub = 40, 2, 128, 0.05
    P = S * S
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = e2e.ScoreNet().to(dev)
    frames = [synth.chess_like_frame(S, S, seed=900 + f, quantise_int16=True) for f in range(F)]
    perm_d = torch.as_tensor(synth.fast_permutations(P, 8), device=dev)
    gt_d = torch.as_tensor(np.stack([orc.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0])) for fr in frames]), device=dev)
    xyz_d = torch.stack([torch.as_tensor(fr["xyz"], dtype=torch.float32, device=dev) for fr in frames]).contiguous()
    uv_d = torch.stack([torch.as_tensor(fr["uv"], device=dev) for fr in frames]).contiguous()
    grads, seen = {}, {}
    for dt in (torch.float32, torch.float16):
        for quirk in (True,):  # the transposed seam: the transpose + contiguous() of the gradient images stays in half
            sb = e2e.ScoredFrameBatch(0, frames=F, hyps=N, sub_sample=sub, score_net=net, err_dtype=dt)
            inner = sb.engine.dScore

            def spy(poses, sets, d_err, _inner=inner, _key=(dt, quirk), **kw):
                seen[_key] = (d_err.dtype, d_err.is_contiguous(), tuple(d_err.shape))
                return _inner(poses, sets, d_err, **kw)
            sb.engine.dScore = spy
            sb.forward(xyz_d, uv_d, gt_d, perm_d, seed=1305)
            for p in net.parameters():
                p.grad = None
            grads[(dt, quirk)] = sb.backward(quirk_transpose=quirk).clone()
            torch.cuda.synchronize()
            sb.engine.close()
    for quirk in (True,):
        assert seen[(torch.float32, quirk)] == (torch.float32, True, (F * N, P))
        assert seen[(torch.float16, quirk)] == (torch.float16, True, (F * N, P))  # no .float() in between: K4 is handed the model's halves
        g32, g16 = grads[(torch.float32, quirk)], grads[(torch.float16, quirk)]
        assert bool(torch.isfinite(g16).all()) and float(g16.abs().max()) > 0.0
        rel = float((g16 - g32).abs().max() / g32.abs().max())
        print("ScoredFrameBatch half against float (transposed %s): max |grad_xyz difference| / max |grad_xyz| = %.3e" % (quirk, rel))
        assert rel <= max(4.0 * GRAD_REL_MEASURED, 1e-2), rel
