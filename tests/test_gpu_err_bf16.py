"""bfloat16 error images from K2 at the score-model seam: dsac_reproject_bf16 / dsac_process_images_begin_bf16 (k_reproject_st<.., EXF = 5 / 6>).

The contract is the binary16 call's with another rounding: every stored element is the float call's float rounded to bfloat16 to nearest even (a NaN stays a
NaN), the soft-inlier sums and everything downstream of them are the float call's bit for bit, the launch is the exact-transform vector build on the auto
policy's two tiles (<64 hypotheses, 64 cells> up to 16 384 cells, <64, 256> above), and whatever that build cannot do is refused by name before anything is
enqueued.  The yardstick for the rounding is torch's CPU conversion float32 -> bfloat16; numpy has no bfloat16, so host images are uint16 arrays handed over
with elem="bf16".  Both settings of "k2_f16_store" run every image comparison (on a small map
on the implicit grid with W % 64 != 0 the bfloat16 call takes the layout whose build needs no scratch under either setting; the values do not depend on it)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAU, BETA, CLAMP = 10.0, 0.5, 100.0
EXACT, PRECISE = 1 << 28, 1 << 25
VEC = "exact (vector build)"
PATTERN = 0x5A5A


def _defaults(e):
    e.set_option("k2_variant", -1)
    e.set_option("k2_flags", 0)
    e.set_option("k2_exact_auto", 1)
    e.set_option("k2_f16_store", 1)
    e.set_option("pi_defer_tail", 0)


@pytest.fixture()
def eng(engine):
    _defaults(engine)
    yield engine
    _defaults(engine)


_FRAMES = {}


def _frame(synth, H, W, sampled):
    """One synthetic frame per (shape, kind), shared by the tests and left unchanged.  sampled: stratified pixel positions handed over as uv; else u = x, v = y
    and no uv (the kernels' implicit grid)."""
    key = (H, W, sampled)
    if key not in _FRAMES:
        _FRAMES[key] = synth.chess_like_frame(H, W, seed=1305 + H + W, grid_uv=not sampled)
    return _FRAMES[key]


def _set(eng, fr, sampled):
    eng.set_frame(fr["xyz"], fr["uv"] if sampled else None, fr["H"], fr["W"], fr["cam"])


def _bf16_bits(a32):
    """The bit patterns of float32 values rounded to bfloat16 by torch on the CPU (round to nearest even)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _assert_rounded(got, err32, what=""):
    """Every element of got (uint16) is the rounded float; where the float call stored a NaN, a NaN (exponent all ones, a non-zero mantissa)."""
    want = _bf16_bits(err32)
    nan = np.isnan(err32)
    if nan.any():
        assert bool((((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x007F) != 0)).all()), "%s: a NaN of the float call is no NaN in bfloat16" % what
    bad = np.argwhere((got != want) & ~nan)
    assert bad.size == 0, "%s: %d cells differ, first (hypothesis, cell) %s: %#x against %#x" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _same_as_float_call(eng, poses, N, P, want_soft=True, layouts=(0, 1)):
    """dsac_reproject, then dsac_reproject_bf16 in every store layout: elements == the rounded floats on every cell, soft bit for bit, the exact vector build.
    Returns the images of the layouts."""
    err32 = np.zeros((N, P), np.float32)
    soft32 = np.zeros(N) if want_soft else None
    eng.reproject(poses, err=err32, soft=soft32, tau=TAU, beta=BETA)
    assert eng.k2_form() == (VEC, 0)
    out = []
    for layout in layouts:
        eng.set_option("k2_f16_store", layout)
        err16 = np.full((N, P), PATTERN, np.uint16)
        soft16 = np.full(N, -1.0) if want_soft else None
        eng.reproject(poses, err=err16, soft=soft16, tau=TAU, beta=BETA, elem="bf16")
        assert eng.k2_form() == (VEC, 0)
        _assert_rounded(err16, err32, "layout %d" % layout)
        if want_soft:
            assert np.array_equal(soft16.view(np.uint64), soft32.view(np.uint64)), "layout %d: soft differs" % layout
        out.append(err16)
    return out


# ---- rounded floats, both tiles, both layouts --------------------------------------------------------------------------------------------------
# small tile (<= 16 384 cells): 40 x 40 = 25 whole chunks; 44 wide x 36 high = 1 584 cells, last chunk partial.  Big tile: 128 wide x 132 high = 16 896
# cells (W % 64 == 0: the G64 build); 136 wide x 124 high = 16 864 cells (W % 64 != 0, last 256-cell tile partial).  N = 80: a ragged hypothesis tile
@pytest.mark.parametrize("N", [64, 80])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("H,W", [(40, 40), (36, 44), (132, 128), (124, 136)])
def test_elements_are_the_rounded_floats(eng, synth, H, W, sampled, N):
    fr = _frame(synth, H, W, sampled)
    _set(eng, fr, sampled)
    poses, _, _ = eng.sample(N, seed=77, thr=10.0, max_tries=1 << 16)
    a, b = _same_as_float_call(eng, poses, N, H * W)
    assert np.array_equal(a, b)  # the two store layouts agree


@pytest.mark.parametrize("H,W", [(40, 40), (132, 128)])
def test_error_images_only(eng, synth, H, W):
    fr = _frame(synth, H, W, False)
    _set(eng, fr, False)
    poses, _, _ = eng.sample(64, seed=78, thr=10.0, max_tries=1 << 16)
    _same_as_float_call(eng, poses, 64, H * W, want_soft=False)


def test_far_chunk(eng, synth):
    """A chunk with a coordinate beyond 65.5 m takes the in-kernel fp32 path, in bfloat16 as in float."""
    fr = dict(_frame(synth, 40, 40, False))
    fr["xyz"] = fr["xyz"].copy()
    fr["xyz"][70, 0] = 70000.0  # chunk 1
    _set(eng, fr, False)
    poses, _, _ = eng.sample(64, seed=79, thr=10.0, max_tries=1 << 16)
    far, _ = eng.k2_census(poses)
    assert far >= 1
    _same_as_float_call(eng, poses, 64, 1600)


def test_host_pointers_against_device_pointers(eng, synth):
    import torch
    from dsac_amd import capi
    fr = _frame(synth, 40, 40, False)
    _set(eng, fr, False)
    N, P = 64, 1600
    poses, _, _ = eng.sample(N, seed=77, thr=10.0, max_tries=1 << 16)
    assert isinstance(poses, np.ndarray)
    err32, soft32 = np.zeros((N, P), np.float32), np.zeros(N)
    err16, soft16 = np.full((N, P), PATTERN, np.uint16), np.zeros(N)
    capi.check(eng._ctx, capi.lib.dsac_reproject(eng._ctx, N, capi.ptr(poses), CLAMP, capi.ptr(err32), TAU, BETA, capi.ptr(soft32)))
    capi.check(eng._ctx, capi.lib.dsac_reproject_bf16(eng._ctx, N, capi.ptr(poses), CLAMP, capi.ptr(err16), TAU, BETA, capi.ptr(soft16)))
    _assert_rounded(err16, err32, "host pointers")
    assert np.array_equal(soft16.view(np.uint64), soft32.view(np.uint64))
    assert eng.get_option("k2_form_last") == 4  # DSAC_K2_FORM_EXACT_VEC
    dev = torch.device("cuda", 0)
    e_dev = torch.full((N, P), 7.0, dtype=torch.bfloat16, device=dev)
    s_dev = torch.zeros(N, dtype=torch.float64, device=dev)
    eng.reproject(torch.from_numpy(poses).to(dev), N=N, err=e_dev, soft=s_dev, tau=TAU, beta=BETA)  # the tensor's dtype picks the call
    eng.synchronize()
    assert np.array_equal(e_dev.view(torch.int16).cpu().numpy().view(np.uint16), err16)
    assert np.array_equal(s_dev.cpu().numpy().view(np.uint64), soft32.view(np.uint64))


# ---- a frame batch through the seam ------------------------------------------------------------------------------------------------------------
def test_frame_batch_through_the_seam(synth, orc):
    """begin_bf16 -> finish on scores equal to soft: everything but the images is dsac_process_images' bit for bit, the images are its images rounded."""
    import torch
    import dsac_amd
    dev = torch.device("cuda", 0)
    H = W = 40
    F, N, P = 2, 128, 1600
    frames = [synth.chess_like_frame(H, W, seed=700 + f, quantise_int16=True) for f in range(F)]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))).to(dev)
    uv = torch.from_numpy(frames[0]["uv"]).to(dev)
    perm = torch.from_numpy(synth.fast_permutations(P, 8)).to(dev)
    gts = torch.from_numpy(np.stack([orc.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0])) for fr in frames])).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)

    def bufs():
        return dict(hyps=torch.zeros(F * N, 6, **f64), sampledPoints=torch.zeros(F * N, 4, dtype=torch.int32, device=dev),
                    ok=torch.zeros(F * N, dtype=torch.uint8, device=dev), scores=torch.zeros(F * N, **f64), sfScores=torch.zeros(F * N, **f64),
                    sfEntropy=torch.zeros(F, **f64), avgHyp=torch.zeros(F, 6, **f64), refAvgHyp=torch.zeros(F, 6, **f64),
                    refSteps=torch.zeros(F, dtype=torch.int32, device=dev), out4=torch.zeros(F, 4, **f64))

    with dsac_amd.Engine(0) as e:
        e.set_frames(xyz, uv, H, W, frames[0]["cam"], borrow=True)
        o32, o16 = bufs(), bufs()
        e32 = torch.empty(F * N, P, dtype=torch.float32, device=dev)
        e16 = torch.full((F * N, P), 7.0, dtype=torch.bfloat16, device=dev)
        e.processImages(N, perm, gt_jp6=gts, seed=91, scale=0.1, err=e32, out=o32)
        e.processImagesBegin(N, e16, seed=91, soft=o16["scores"], out=(o16["hyps"], o16["sampledPoints"], o16["ok"]))
        assert e.k2_form() == (VEC, 0)
        e.processImagesFinish(N, o16["scores"], perm, o16["hyps"], gt_jp6=gts, scale=0.1, out=o16)
        e.synchronize()
        assert bool(o32["ok"].all())
        for key in o32:  # poses, sets, ok, soft (scores), w (sfScores), avg6, ref6, steps, out4
            assert torch.equal(o16[key], o32[key]), key
        assert torch.equal(e16.view(torch.int16).cpu(), e32.cpu().to(torch.bfloat16).view(torch.int16))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def _aligned_u16(n, off_bytes=0):
    """n uint16 words whose first byte sits off_bytes past a 16-byte address, filled with the pattern; returns (array, keep-alive)."""
    buf = np.full(n + 32, PATTERN, np.uint16)
    start = ((-buf.ctypes.data) % 16 + off_bytes) // 2
    a = buf[start:start + n]
    assert a.ctypes.data % 16 == off_bytes
    return a, buf


@pytest.mark.parametrize("case", ["53x37", "42x38", "err16 off by 2 bytes", "f = 1100", "k2_variant 24", "k2_flags bit 25", "k2_exact_auto 0", "NULL"])
def test_refusals(eng, synth, case):
    from dsac_amd import capi
    H, W, cam, off = 40, 40, synth.CAM_7SCENES, 0
    if case == "53x37":
        H, W = 37, 53
    elif case == "42x38":
        H, W = 38, 42  # 1 596 cells: a multiple of 4, not of 8
    elif case == "f = 1100":
        cam = (1100.0, 1100.0, 320.0, 240.0)
    elif case == "err16 off by 2 bytes":
        off = 2
    fr = synth.chess_like_frame(H, W, seed=5, cam=cam, grid_uv=True)
    eng.set_frame(fr["xyz"], None, H, W, cam)
    N, P = 64, H * W
    poses, _, _ = eng.sample(N, seed=1, thr=10.0, max_tries=1 << 16)
    # a float launch first, so that "k2_form_last" has a value a refused call could overwrite
    soft = np.zeros(N)
    eng.reproject(poses, soft=soft)
    if case == "k2_variant 24":
        eng.set_option("k2_variant", 24)
    elif case == "k2_flags bit 25":
        eng.set_option("k2_flags", PRECISE)
    elif case == "k2_exact_auto 0":
        eng.set_option("k2_exact_auto", 0)
    before = (eng.get_option("k2_form_last"), eng.get_option("k2_form_why_last"))
    err16, keep = _aligned_u16(N * P, off)
    where = None if case == "NULL" else err16.ctypes.data
    rc = capi.lib.dsac_reproject_bf16(eng._ctx, N, capi.ptr(poses), CLAMP, where, TAU, BETA, capi.ptr(soft))
    assert rc == capi.DSAC_ERR_INVALID, case
    msg = capi.lib.dsac_last_error(eng._ctx).decode()
    assert msg.startswith("dsac_reproject_bf16:") and len(msg) > 30, msg
    sets, ok = np.zeros((N, 4), np.int32), np.zeros(N, np.uint8)
    rc = capi.lib.dsac_process_images_begin_bf16(eng._ctx, N, 1, 10.0, 1 << 16, CLAMP, TAU, BETA, capi.ptr(np.zeros((N, 6))), capi.ptr(sets), capi.ptr(ok),
                                                 where, capi.ptr(soft))
    assert rc == capi.DSAC_ERR_INVALID, case
    assert capi.lib.dsac_last_error(eng._ctx).decode().startswith("dsac_process_images_begin_bf16:")
    eng.synchronize()
    assert bool((keep == PATTERN).all()), "a refused call wrote into err16"
    assert (eng.get_option("k2_form_last"), eng.get_option("k2_form_why_last")) == before
    if case == "k2_exact_auto 0":
        eng.set_option("k2_flags", EXACT)  # bit 28 asks for the exact form by name: bfloat16 images again
        e16 = np.zeros((N, P), np.uint16)
        eng.reproject(poses, err=e16, elem="bf16")
        assert eng.k2_form() == (VEC, 0) and e16.any()
    assert capi.lib.dsac_reproject_bf16(None, N, capi.ptr(poses), CLAMP, None, TAU, BETA, None) == capi.DSAC_ERR_INVALID  # no context
