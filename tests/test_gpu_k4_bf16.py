"""K4 on bfloat16 gradient images: dsac_score_backward_bf16 (k_score_backward_mfma<.., __bf16>) and dsac_soft_score_derr_bf16.

The contract is the binary16 call's: the bfloat16 call is the float call on the widened values -- the same launch plan, the same summation orders, an exact
widening (a bfloat16 is the upper half of the float of the same value) --, so with grad_xyz zeroed beforehand gradient and pose sums are equal bit for bit;
whatever the matrix-core form cannot do is refused by name before anything is staged or enqueued.  The yardstick is the float call on the same values, torch's
CPU conversion for a rounding, and the oracle once.  numpy has no bfloat16: host images are uint16 arrays handed over with elem="bf16".

Bit-for-bit needs an order-independent float call: the identity tests draw minimal sets that share no cell (tests/test_gpu_k4_f16.py explains why).  Where
sampled sets share support cells the bound is the project's 1e-12 for fp64 atomics on shared cells, and 1e-5 of the largest entry where two launches group
their fp32 partial sums by different tiles (tests/test_gpu_backward_batch.py)."""
import numpy as np
import pytest

from conftest import margin

pytestmark = pytest.mark.gpu

# +-0, the smallest and the largest subnormal, the smallest normal, 2^-30 (below everything binary16 holds), +-6.5e4.  Nothing large enough to overflow the
# fp32 sums: the identity would then compare NaN with NaN
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x007F, 0x0080, 0x3080, 0x477F, 0xC77F], np.uint16)
_CACHE = {}


def _to_bf16(a32):
    """float32 -> bfloat16 bit patterns (uint16), rounded to nearest even by torch on the CPU."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def _widen(b16):
    """bfloat16 bit patterns -> the float32 of the same value (exact)."""
    return (b16.astype(np.uint32) << 16).view(np.float32)


def _images(N, P, seed):
    """N x P bfloat16 bit patterns from a normal sample with every special value at three cells of every row."""
    rng = np.random.default_rng(seed)
    bits = _to_bf16(rng.standard_normal((N, P)).astype(np.float32))
    cols = np.stack([rng.choice(P, 3 * len(SPECIALS), replace=False) for _ in range(N)])
    bits[np.arange(N)[:, None], cols] = np.tile(SPECIALS, 3)[None, :]
    return bits


def _unique_sets(N, P, seed):
    return np.random.default_rng(seed).permutation(P)[:4 * N].reshape(N, 4).astype(np.int32)


def _case(engine, synth, H, W, sampled, N):
    """(frame, poses, sets, images) for one shape, made once, shared and left unchanged; the frame is set in the engine."""
    key = (H, W, sampled, N)
    fr = _CACHE.setdefault((H, W, sampled), synth.chess_like_frame(H, W, seed=1305 + H + W, noise_mm=1.0, outlier_frac=0.0, grid_uv=not sampled))
    engine.set_frame(fr["xyz"], fr["uv"] if sampled else None, H, W, fr["cam"])
    if key not in _CACHE:
        sets = _unique_sets(N, H * W, N)
        poses, sets_out, _ = engine.sample(N, sets=sets, thr=10.0)
        assert np.array_equal(sets_out, sets) and np.isfinite(poses).all()
        _CACHE[key] = (poses, sets, _images(N, H * W, 7 * N + H))
    return (fr,) + _CACHE[key]


def _both(engine, poses, sets, b16, **kw):
    N = sets.shape[0]
    g16 = engine.dScore(poses, sets, b16, elem="bf16", **kw)
    p16 = engine.lastPoseGradients(N)
    g32 = engine.dScore(poses, sets, _widen(b16), **kw)
    p32 = engine.lastPoseGradients(N)
    assert np.isfinite(g32).all() and np.abs(g32).max() > 0
    return g16, p16, g32, p32


def _assert_identical(g16, p16, g32, p32):
    bad = np.argwhere(g16 != g32)
    assert bad.size == 0, "%d gradient entries differ, first %s: %r against %r" % (len(bad), tuple(bad[0]), g16[tuple(bad[0])], g32[tuple(bad[0])])
    assert np.array_equal(g16, g32) and np.array_equal(p16, p32)


# ---- identity with the float call on the widened values ------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_k4_f16.py: 40 x 40 sampled is the small-map plan, 2 chunks (N = 40: ragged last group; N = 272: more than 256 hypotheses,
# grad_part + the reduction); 38 high x 42 wide sampled: the last chunk partly beyond the map; 36 x 44 implicit grid; 416 high x 320 wide implicit: the
# big-map plan, 4 chunks, tiles split between two workgroups, gradient through fp64 atomics
@pytest.mark.parametrize("H,W,sampled,N", [(40, 40, True, 64), (40, 40, True, 40), (40, 40, True, 272), (38, 42, True, 64), (36, 44, False, 64),
                                           (416, 320, False, 40)])
def test_identical_to_the_float_call(engine, synth, H, W, sampled, N):
    _, poses, sets, b16 = _case(engine, synth, H, W, sampled, N)
    _assert_identical(*_both(engine, poses, sets, b16))


def test_identical_with_the_transposed_index(engine, synth):
    _, poses, sets, b16 = _case(engine, synth, 40, 40, True, 64)
    _assert_identical(*_both(engine, poses, sets, b16, quirk_transpose=True))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [False, True])
def test_parity_with_the_oracle(engine, orc, frame40, quirk):
    """The gradient images are exactly representable on both sides, so the float kernel's own error is all there is: the float test's tolerances."""
    fr, N = frame40, 64
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    poses, sets, _, _ = orc.sample(N, 5, fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    b16 = _images(N, 1600, 1)
    ref, _, _ = orc.dScore(sets, _widen(b16).astype(np.float64), fr["xyz"], fr["uv"], 40, 40, fr["cam"], quirk_transpose=quirk)
    J = np.stack([orc.dPNP(fr["uv"][s_], fr["xyz"][s_], fr["cam"]) for s_ in sets])  # the same dPNP on both sides
    got = engine.dScore(poses, sets, b16, dpnp=J, quirk_transpose=quirk, elem="bf16")
    margin("a12", "dScore on bfloat16 gradient images 40x40 (index quirk on/off): gradient max-rel vs oracle", np.abs(got - ref).max() / np.abs(ref).max(), 1e-3)
    margin("a12", "dScore on bfloat16 gradient images 40x40 (index quirk on/off): gradient relative l2 error", np.linalg.norm(got - ref) / np.linalg.norm(ref), 5e-4)


# ---- frame batches -----------------------------------------------------------------------------------------------------------------------------------
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
    b16 = _images(F * Nf, P, Nf)
    engine.set_frames(xyz, uv, H, W, cam, uv_per_frame=True)
    engine.profile_enable(True, stride=1)
    engine.profile_read(1, reset=True)
    g16 = engine.dScore(poses, sets, b16, elem="bf16")
    _, launches = engine.profile_read(1, reset=True)
    engine.profile_enable(False)
    assert launches == (1 if Nf % 16 == 0 else F)
    p16 = engine.lastPoseGradients(F * Nf)
    g32 = engine.dScore(poses, sets, _widen(b16))
    _assert_identical(g16, p16, g32, engine.lastPoseGradients(F * Nf))
    assert g16.shape == (F * P, 3)
    for f in range(F):
        hs, cs = slice(f * Nf, (f + 1) * Nf), slice(f * P, (f + 1) * P)
        engine.set_frame(xyz[f], uv[f], H, W, cam)
        g1 = engine.dScore(poses[hs], sets[hs], np.ascontiguousarray(b16[hs]), elem="bf16")
        p1 = engine.lastPoseGradients(Nf)
        if Nf % 16 == 0:  # the batch's tile is the frame's 32 hypotheses, the single frame's small-map plan has tiles of 16: fp32 partial sums grouped otherwise
            margin("a15", "bfloat16 frame batch in one launch vs single-frame bfloat16 calls, K4 gradient: max |d| / max |g|", np.abs(g16[cs] - g1).max() / np.abs(g1).max(), 1e-5)
            margin("a10", "bfloat16 frame batch in one launch vs single-frame bfloat16 calls, pose sums: max |d| / max |G6|", np.abs(p16[hs] - p1).max() / np.abs(p1).max(), 1e-5)
        else:  # the same launches as the single-frame calls
            assert np.array_equal(g16[cs], g1) and np.array_equal(p16[hs], p1)


# ---- argument kinds and modes ------------------------------------------------------------------------------------------------------------------------
def test_host_and_device_images_give_equal_results(engine, synth):
    import torch
    _, poses, sets, b16 = _case(engine, synth, 40, 40, True, 64)
    g_host = engine.dScore(poses, sets, b16, elem="bf16")
    p_host = engine.lastPoseGradients(64)
    dev = torch.device("cuda", 0)
    d_dev = torch.from_numpy(b16.view(np.int16)).to(dev).view(torch.bfloat16)
    grad = torch.zeros(1600, 3, dtype=torch.float64, device=dev)
    engine.dScore(torch.from_numpy(poses).to(dev), torch.from_numpy(sets).to(dev), d_dev, grad=grad)  # a bfloat16 tensor: by its dtype
    p_dev = engine.lastPoseGradients(64)
    engine.synchronize()
    assert np.array_equal(grad.cpu().numpy(), g_host) and np.array_equal(p_dev, p_host)


def test_the_staged_form(engine, synth):
    _, poses, sets, b16 = _case(engine, synth, 36, 44, False, 64)
    g_auto = engine.dScore(poses, sets, b16, elem="bf16")
    engine.set_option("k4_variant", 1999)
    try:
        g16, p16, g32, p32 = _both(engine, poses, sets, b16)
    finally:
        engine.set_option("k4_variant", -1)
    _assert_identical(g16, p16, g32, p32)
    assert np.abs(g16 - g_auto).max() <= 1e-5 * np.abs(g_auto).max()  # the two stagings group the fp32 partial sums differently


def test_accumulates(engine, synth):
    """Into a non-zero grad_xyz: within the last bit of a cell, as two runs of the float call.  A cell receives at most three fp64 additions per call (two from
    the main pass, one from the support scatter: the sets share no cell), each rounded at the size of a partial sum, which the largest entry of the doubled
    gradient bounds on these data: 3 x 2^-53 x that, asserted as 4 x 2^-53."""
    _, poses, sets, b16 = _case(engine, synth, 40, 40, True, 64)
    g0 = engine.dScore(poses, sets, b16, elem="bf16")
    g1 = engine.dScore(poses, sets, b16, elem="bf16", grad=g0.copy())
    g1f = engine.dScore(poses, sets, _widen(b16), grad=g0.copy())
    tol = 4 * 2.0 ** -53 * np.abs(g1f).max()
    print("accumulation: max |bf16 - float| = %.3e, max |bf16 - 2 g0| = %.3e, tolerance %.3e" % (np.abs(g1 - g1f).max(), np.abs(g1 - 2 * g0).max(), tol))
    assert np.abs(g1 - g1f).max() <= tol
    assert np.abs(g1 - 2 * g0).max() <= tol


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
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
        bits = _images(N, P, 2)
        d32 = _widen(bits)
        float_runs = case != "fx != fy"
        if float_runs:  # a float call first: the count and the sums a refused call must leave behind
            engine.dScore(poses, sets, d32, dpnp=J)
            G6_before = engine.lastPoseGradients(N)
        d16, hold = _off_by(2 if case == "d_err16 off by 2 bytes" else 0, N * P, np.uint16)
        d16[:] = bits.reshape(-1)
        if case.startswith("k4_variant"):
            engine.set_option("k4_variant", int(case.split()[1]))
        grad = np.full((P, 3), PATTERN)
        rc = lib.dsac_score_backward_bf16(engine._ctx, N, ptr(poses), ptr(sets), None if case == "NULL" else d16.ctypes.data, None, flags, ptr(grad))
        assert rc == capi.DSAC_ERR_INVALID, case
        msg = lib.dsac_last_error(engine._ctx).decode()
        assert msg.startswith("dsac_score_backward_bf16:") and len(msg) > 35, msg
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
    """The refusal looks at every frame of a batch."""
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
        d16, hold = _off_by(4 if case.endswith("4 bytes") else 0, F * Nf * P, np.uint16)
        d16[:] = _images(F * Nf, P, 9).reshape(-1)
        grad = np.full((F * P, 3), PATTERN)
        rc = lib.dsac_score_backward_bf16(engine._ctx, F * Nf, ptr(poses), ptr(sets), d16.ctypes.data, None, 0, ptr(grad))
        assert rc == capi.DSAC_ERR_INVALID, case
        assert lib.dsac_last_error(engine._ctx).decode().startswith("dsac_score_backward_bf16:")
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


@pytest.mark.parametrize("variant", [3, 4, 6, 7, 1003])
def test_forms_that_are_not_built_for_bfloat16_are_refused(engine, synth, variant):
    """The 5- and 6-chunk forms and the high-occupancy forms need scratch in every element type: bfloat16 is not built for them, the call says so by name and
    touches nothing; the float call on the same option runs."""
    from dsac_amd import capi
    lib, ptr = capi.lib, capi.ptr
    _, poses, sets, b16 = _case(engine, synth, 40, 40, True, 64)
    N, P = 64, 1600
    engine.dScore(poses, sets, _widen(b16))
    G6_before = engine.lastPoseGradients(N)
    engine.set_option("k4_variant", variant)
    try:
        grad = np.full((P, 3), PATTERN)
        rc = lib.dsac_score_backward_bf16(engine._ctx, N, ptr(poses), ptr(sets), ptr(b16), None, 0, ptr(grad))
        assert rc == capi.DSAC_ERR_INVALID
        msg = lib.dsac_last_error(engine._ctx).decode()
        assert msg.startswith("dsac_score_backward_bf16:") and "bfloat16" in msg, msg
        engine.synchronize()
        assert bool((grad == PATTERN).all()) and np.array_equal(engine.lastPoseGradients(N), G6_before)
        g = engine.dScore(poses, sets, _widen(b16))
        assert np.isfinite(g).all() and np.abs(g).max() > 0
    finally:
        engine.set_option("k4_variant", -1)


@pytest.mark.parametrize("variant", [1, 2, 5])
def test_every_form_built_for_bfloat16_equals_the_float_call(engine, synth, variant):
    _, poses, sets, b16 = _case(engine, synth, 40, 40, True, 64)
    engine.set_option("k4_variant", variant)
    try:
        _assert_identical(*_both(engine, poses, sets, b16))
    finally:
        engine.set_option("k4_variant", -1)


def test_the_python_layer_refuses_the_parity_mode_in_bfloat16(engine, synth):
    _, poses, sets, b16 = _case(engine, synth, 40, 40, True, 64)
    from dsac_amd import capi
    with pytest.raises(ValueError):
        engine.dScore(poses, sets, b16, elem="bf16", parity_fp64=True)
    assert capi.lib.dsac_score_backward_bf16(None, 64, capi.ptr(poses), capi.ptr(sets), capi.ptr(b16), None, 0, None) == capi.DSAC_ERR_INVALID  # no context


# ---- the gradient images of the soft-inlier score in bfloat16 ------------------------------------------------------------------------------------------
TAU, BETA, CLAMP = 10.0, 0.5, 100.0


def _err_images(engine, fr, N):
    """bfloat16 error images (uint16) of N sampled hypotheses on the 40 x 40 frame, which is set in the engine."""
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    poses, _, _ = engine.sample(N, seed=77, thr=10.0, max_tries=1 << 16)
    err16 = np.zeros((N, 1600), np.uint16)
    engine.reproject(poses, err=err16, elem="bf16")
    return err16


def test_soft_score_derr_in_bfloat16(engine, frame40):
    """Every cell's bits are torch's CPU rounding of dsac_soft_score_derr on the widened images: the fp32 result is formed as in the float kernel, then rounded
    once (a compiler that fuses the last multiply into the conversion fails this)."""
    from dsac_amd import capi
    lib, ptr = capi.lib, capi.ptr
    fr, N, P = frame40, 64, 1600
    err16 = _err_images(engine, fr, N)
    rng = np.random.default_rng(4)
    g = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-9.0, 0.0, N)
    want32 = np.zeros((N, P), np.float32)
    engine.softScoreDErr(g, _widen(err16), want32, tau=TAU, beta=BETA, clamp=CLAMP)
    want = _to_bf16(want32)
    got = np.full((N, P), 0x5A5A, np.uint16)
    assert engine.softScoreDErr(g, err16, got, tau=TAU, beta=BETA, clamp=CLAMP, elem="bf16") is got
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d cells differ, first %s: %#x against %#x" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    assert (want32 != 0).sum() > 1000
    on_clamp = _widen(err16) == np.float32(CLAMP)
    assert on_clamp.sum() > 0 and not got[on_clamp].any()
    # refusals: a NULL pointer, a pointer off the 8-byte grid, a map with H*W % 4 != 0
    ctx = engine._ctx
    off, hold = _off_by(2, N * P, np.uint16)
    for args in ((None, ptr(got)), (ptr(err16), None), (off.ctypes.data, ptr(got)), (ptr(err16), off.ctypes.data)):
        assert lib.dsac_soft_score_derr_bf16(ctx, N, ptr(g), args[0], CLAMP, TAU, BETA, args[1]) == capi.DSAC_ERR_INVALID
        assert lib.dsac_last_error(ctx).decode().startswith("dsac_soft_score_derr_bf16:")
    engine.synchronize()
    assert np.array_equal(got, want) and not hold.any()
    engine.set_frame(np.zeros((37 * 53, 3), np.float32) + 1000.0, None, 37, 53, fr["cam"])
    assert lib.dsac_soft_score_derr_bf16(ctx, 1, ptr(g), ptr(err16), CLAMP, TAU, BETA, ptr(got)) == capi.DSAC_ERR_INVALID


def test_small_gradients_survive(engine, synth):
    """The point of the feature.  With g[h] = 1e-9 every gradient value is <= 1e-9 beta / 4 = 1.25e-10, below half of binary16's smallest subnormal (3e-8):
    the half call returns zeros, the bfloat16 call the float call's values to one rounding (2^-8 relative), and K4 a gradient from them."""
    N, P = 64, 1600
    _, poses, sets, _ = _case(engine, synth, 40, 40, True, N)  # minimal sets that share no cell: K4 is compared bit for bit
    err16 = np.zeros((N, P), np.uint16)
    engine.reproject(poses, err=err16, elem="bf16")
    g = np.full(N, 1e-9)
    err32 = _widen(err16)
    d32 = engine.softScoreDErr(g, err32, np.zeros((N, P), np.float32), tau=TAU, beta=BETA, clamp=CLAMP)
    assert np.abs(d32).max() <= 1.25e-10 and (d32 != 0).sum() > 1000
    errh = err32.astype(np.float16)
    dh = engine.softScoreDErr(g, errh, np.full((N, P), 1.0, np.float16), tau=TAU, beta=BETA, clamp=CLAMP)
    assert bool((dh == 0).all())  # binary16: every value underflows to (a signed) zero
    db = engine.softScoreDErr(g, err16, np.zeros((N, P), np.uint16), tau=TAU, beta=BETA, clamp=CLAMP, elem="bf16")
    wb = _widen(db)
    nz = d32 != 0
    assert bool((wb[nz] != 0).all()) and not wb[~nz].any()
    assert float((np.abs(wb[nz].astype(np.float64) - d32[nz]) / np.abs(d32[nz])).max()) <= 2.0 ** -8
    g16, p16, g32, p32 = _both(engine, poses, sets, db)
    assert np.abs(g16).max() > 0
    _assert_identical(g16, p16, g32, p32)


# ---- ScoredFrameBatch ------------------------------------------------------------------------------------------------------------------------------
def test_scored_frame_batch_in_bfloat16(synth, orc):
    """The forward images are the float call's rounded, the model's gradient images are bfloat16 and go to K4 as they are, and K4's contribution equals
    Engine.dScore on d.float() to the last bit of the fp64 atomics (1e-12: sampled sets share support cells).  No tolerance is asserted between a bfloat16 and
    a float32 MODEL: that difference is the model's rounding, not the library's.  128 hypotheses per frame: the smallest count the seam takes for a batch of
    frames (no K2 hypothesis tile may straddle two frames).  The score model is two small matrix products instead of e2e.ScoreNet, whose bfloat16 convolutions
    cost half a minute of kernel selection on their first call; what is checked here is on the library's side of the seam."""
    import torch
    from dsac_amd import e2e
    S, F, N, sub = 40, 2, 128, 0.05
    P = S * S
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(P, 16), torch.nn.Linear(16, 1)

        def forward(self, err):
            return self.b(torch.relu(self.a(err.flatten(1) * 0.01))).squeeze(1)

    frames = [synth.chess_like_frame(S, S, seed=900 + f, quantise_int16=True) for f in range(F)]
    perm_d = torch.as_tensor(synth.fast_permutations(P, 8), device=dev)
    gt_d = torch.as_tensor(np.stack([orc.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0])) for fr in frames]), device=dev)
    xyz_d = torch.stack([torch.as_tensor(fr["xyz"], dtype=torch.float32, device=dev) for fr in frames]).contiguous()
    uv_d = torch.stack([torch.as_tensor(fr["uv"], device=dev) for fr in frames]).contiguous()
    sb = e2e.ScoredFrameBatch(0, frames=F, hyps=N, sub_sample=sub, score_net=Net(), err_dtype=torch.bfloat16)
    inner, seen = sb.engine.dScore, {}

    def spy(poses, sets, d_err, **kw):
        seen["before"] = kw["grad"].clone()  # path I's part, already in grad_xyz
        seen["args"] = (poses, sets, d_err, dict(kw))
        return inner(poses, sets, d_err, **kw)
    sb.engine.dScore = spy
    try:
        sb.forward(xyz_d, uv_d, gt_d, perm_d, seed=1305)
        assert sb.err.dtype == torch.bfloat16
        err32 = torch.empty(F * N, P, dtype=torch.float32, device=dev)
        sb.engine.reproject(sb.poses, N=F * N, err=err32)  # the float call on the same poses and frames
        got = sb.backward().clone()
        torch.cuda.synchronize()
        assert torch.equal(sb.err.view(F * N, P).view(torch.int16).cpu(), err32.cpu().to(torch.bfloat16).view(torch.int16))
        assert sb._err_in.grad.dtype == torch.bfloat16
        poses, sets, d_err, kw = seen["args"]
        assert d_err.dtype == torch.bfloat16 and d_err.is_contiguous() and tuple(d_err.shape) == (F * N, P)
        assert float(d_err.float().abs().max()) > 0.0
        kw["grad"] = seen["before"].clone()
        want = inner(poses, sets, d_err.float().contiguous(), **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()) and float((got - seen["before"]).abs().max()) > 0.0
        margin("a15", "ScoredFrameBatch in bfloat16: grad_xyz vs Engine.dScore on d.float(), max |d| / max |g|",
               float((got - want).abs().max() / want.abs().max()), 1e-12)
    finally:
        sb.engine.close()
