"""Half-precision error images from K2 at the score-model seam: dsac_reproject_f16 / dsac_process_images_begin_f16 (k_reproject_st<.., EXF = 3 / 4>).

The contract: every stored half is the float call's float rounded to nearest even, the soft-inlier sums (and everything downstream of them) are the float
call's bit for bit, the launch is the exact-transform vector build on the auto policy's two tiles (<64 hypotheses, 64 cells> up to 16 384 cells, <64, 256>
above), and whatever that build cannot do is refused by name before anything is enqueued.  Shapes are the smallest that reach every path of both tiles:
whole and partial last chunks, whole and ragged hypothesis tiles, the implicit grid with and without W % 64 == 0, sampled positions.  Both store layouts
("k2_f16_store" 0 / 1) run every image comparison."""

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


def _same_as_float_call(eng, poses, N, P, want_soft=True, layouts=(0, 1)):
    """dsac_reproject, then dsac_reproject_f16 in every store layout: halves == the rounded floats on every cell, soft bit for bit, the exact vector build."""
    err32 = np.zeros((N, P), np.float32)
    soft32 = np.zeros(N) if want_soft else None
    eng.reproject(poses, err=err32, soft=soft32, tau=TAU, beta=BETA)
    assert eng.k2_form() == (VEC, 0)
    want = err32.astype(np.float16).view(np.uint16)
    for layout in layouts:
        eng.set_option("k2_f16_store", layout)
        err16 = np.full((N, P), PATTERN, np.uint16).view(np.float16)
        soft16 = np.full(N, -1.0) if want_soft else None
        eng.reproject(poses, err=err16, soft=soft16, tau=TAU, beta=BETA)
        assert eng.k2_form() == (VEC, 0)
        got = err16.view(np.uint16)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "layout %d: %d cells differ, first (hypothesis, cell) %s: %#x against %#x" % (
            layout, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        if want_soft:
            assert np.array_equal(soft16.view(np.uint64), soft32.view(np.uint64)), "layout %d: soft differs" % layout
    return err32


# ---- 1. / 2. bit-exact against the float call, both tiles ------------------------------------------------------------------------------
# small tile (<= 16 384 cells): 40 x 40 = 25 whole chunks; 44 wide x 36 high = 1 584 cells, last chunk partial.  Big tile: 128 wide x 132 high = 16 896
# cells (W % 64 == 0: the G64 build); 136 wide x 124 high = 16 864 cells (W % 64 != 0, last 256-cell tile partial)
@pytest.mark.parametrize("N", [64, 80])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("H,W", [(40, 40), (36, 44), (132, 128), (124, 136)])
def test_halves_are_the_rounded_floats(eng, synth, H, W, sampled, N):
    fr = _frame(synth, H, W, sampled)
    _set(eng, fr, sampled)
    poses, _, _ = eng.sample(N, seed=77, thr=10.0, max_tries=1 << 16)
    _same_as_float_call(eng, poses, N, H * W)


# ---- 3. error images only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 40), (132, 128)])
def test_error_images_only(eng, synth, H, W):
    fr = _frame(synth, H, W, False)
    _set(eng, fr, False)
    poses, _, _ = eng.sample(64, seed=78, thr=10.0, max_tries=1 << 16)
    _same_as_float_call(eng, poses, 64, H * W, want_soft=False)


# ---- 4. a chunk with a far coordinate takes the in-kernel fp32 path, in half as in float ----------------------------------------------------
def test_far_chunk(eng, synth):
    fr = dict(_frame(synth, 40, 40, False))
    fr["xyz"] = fr["xyz"].copy()
    fr["xyz"][70, 0] = 70000.0  # chunk 1
    _set(eng, fr, False)
    poses, _, _ = eng.sample(64, seed=79, thr=10.0, max_tries=1 << 16)
    far, _ = eng.k2_census(poses)
    assert far >= 1
    _same_as_float_call(eng, poses, 64, 1600)


# ---- 5. a frame batch through the seam ---------------------------------------------------------------------------------------------------
def test_frame_batch_through_the_seam(synth, orc):
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
        for mode in (0, 2):
            e.set_option("pi_defer_tail", mode)
            o32, o16 = bufs(), bufs()
            e32 = torch.empty(F * N, P, dtype=torch.float32, device=dev)
            e16 = torch.full((F * N, P), 7.0, dtype=torch.float16, device=dev)
            e.processImagesBegin(N, e32, seed=91, soft=o32["scores"], out=(o32["hyps"], o32["sampledPoints"], o32["ok"]))
            e.processImagesFinish(N, o32["scores"], perm, o32["hyps"], gt_jp6=gts, scale=0.1, out=o32)
            e.processImagesBegin(N, e16, seed=91, soft=o16["scores"], out=(o16["hyps"], o16["sampledPoints"], o16["ok"]))
            assert e.k2_form() == (VEC, 0)
            e.processImagesFinish(N, o16["scores"], perm, o16["hyps"], gt_jp6=gts, scale=0.1, out=o16)
            e.joinTail()
            e.synchronize()
            assert bool(o32["ok"].all())
            for key in o32:  # poses, sets, ok, soft (scores), w (sfScores), avg6, ref6, out4 and the rest
                assert torch.equal(o16[key], o32[key]), (key, mode)
            assert torch.equal(e16.view(torch.int16), e32.to(torch.float16).view(torch.int16)), mode
        e.set_option("pi_defer_tail", 0)


# ---- 6. host pointers for every argument -------------------------------------------------------------------------------------------------
def test_host_pointers(eng, synth):
    from dsac_amd import capi
    fr = _frame(synth, 40, 40, False)
    _set(eng, fr, False)
    N, P = 64, 1600
    poses, _, _ = eng.sample(N, seed=77, thr=10.0, max_tries=1 << 16)
    assert isinstance(poses, np.ndarray)
    err32, soft32 = np.zeros((N, P), np.float32), np.zeros(N)
    err16, soft16 = np.full((N, P), PATTERN, np.uint16), np.zeros(N)
    capi.check(eng._ctx, capi.lib.dsac_reproject(eng._ctx, N, capi.ptr(poses), CLAMP, capi.ptr(err32), TAU, BETA, capi.ptr(soft32)))
    capi.check(eng._ctx, capi.lib.dsac_reproject_f16(eng._ctx, N, capi.ptr(poses), CLAMP, capi.ptr(err16), TAU, BETA, capi.ptr(soft16)))
    assert np.array_equal(err16, err32.astype(np.float16).view(np.uint16))
    assert np.array_equal(soft16.view(np.uint64), soft32.view(np.uint64))
    assert eng.get_option("k2_form_last") == 4  # DSAC_K2_FORM_EXACT_VEC


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def _aligned_u16(n, off_bytes=0):
    """n uint16 words whose first byte sits off_bytes past a 16-byte address, filled with the pattern; returns (array, keep-alive)."""
    buf = np.full(n + 32, PATTERN, np.uint16)
    start = ((-buf.ctypes.data) % 16 + off_bytes) // 2
    a = buf[start:start + n]
    assert a.ctypes.data % 16 == off_bytes
    return a, buf


@pytest.mark.parametrize("case", ["53x37", "42x38", "err16 off by 2 bytes", "f = 1100", "k2_variant 24", "k2_flags bit 25", "k2_exact_auto 0"])
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
    rc = capi.lib.dsac_reproject_f16(eng._ctx, N, capi.ptr(poses), CLAMP, err16.ctypes.data, TAU, BETA, capi.ptr(soft))
    assert rc == capi.DSAC_ERR_INVALID, case
    msg = capi.lib.dsac_last_error(eng._ctx).decode()
    assert msg.startswith("dsac_reproject_f16:") and len(msg) > 30, msg
    sets, ok = np.zeros((N, 4), np.int32), np.zeros(N, np.uint8)
    rc = capi.lib.dsac_process_images_begin_f16(eng._ctx, N, 1, 10.0, 1 << 16, CLAMP, TAU, BETA, capi.ptr(np.zeros((N, 6))), capi.ptr(sets), capi.ptr(ok),
                                                err16.ctypes.data, capi.ptr(soft))
    assert rc == capi.DSAC_ERR_INVALID, case
    assert capi.lib.dsac_last_error(eng._ctx).decode().startswith("dsac_process_images_begin_f16:")
    eng.synchronize()
    assert bool((keep == PATTERN).all()), "a refused call wrote into err16"
    assert (eng.get_option("k2_form_last"), eng.get_option("k2_form_why_last")) == before
    # the float call on the same frame and options still runs (or is refused) as before: the half path changes nothing for it
    if case == "k2_exact_auto 0":
        eng.set_option("k2_flags", EXACT)  # bit 28 asks for the exact form by name: half images again
        e16 = np.zeros((N, P), np.float16)
        eng.reproject(poses, err=e16)
        assert eng.k2_form() == (VEC, 0)


def test_null_err16_is_refused(eng, synth):
    from dsac_amd import capi
    fr = _frame(synth, 40, 40, False)
    _set(eng, fr, False)
    poses, _, _ = eng.sample(64, seed=77, thr=10.0, max_tries=1 << 16)
    soft = np.zeros(64)
    assert capi.lib.dsac_reproject_f16(eng._ctx, 64, capi.ptr(poses), CLAMP, None, TAU, BETA, capi.ptr(soft)) == capi.DSAC_ERR_INVALID
    assert capi.lib.dsac_reproject_f16(None, 64, capi.ptr(poses), CLAMP, None, TAU, BETA, None) == capi.DSAC_ERR_INVALID


# ---- 8. the Python seam ------------------------------------------------------------------------------------------------------------------
def test_process_images_scored_in_half(synth, orc):
    import torch
    import dsac_amd
    dev = torch.device("cuda", 0)
    H = W = 40
    F, N, P = 2, 128, 1600
    frames = [synth.chess_like_frame(H, W, seed=700 + f, quantise_int16=True) for f in range(F)]
    xyz = torch.from_numpy(np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))).to(dev)
    uv = torch.from_numpy(frames[0]["uv"]).to(dev)
    perm = synth.fast_permutations(P, 8)
    gts = np.stack([orc.cv_to_jp6(fr["gt_pose"]) for fr in frames])
    seen = []

    def score_fn(e):
        seen.append(e)
        return torch.sigmoid(BETA * (TAU - e.float())).sum(dim=(1, 2))

    with dsac_amd.Engine(0) as e:
        e.set_frames(xyz, uv, H, W, frames[0]["cam"], borrow=True)
        r32 = e.processImagesScored(N, perm, score_fn, gt_jp6=gts, seed=91, scale=0.1)
        r16 = e.processImagesScored(N, perm, score_fn, gt_jp6=gts, seed=91, scale=0.1, err_dtype=torch.float16)
        e.synchronize()
    e32, e16 = seen
    assert e32.dtype == torch.float32
    assert e16.dtype == torch.float16 and e16.is_contiguous() and tuple(e16.shape) == (F * N, H, W)
    assert r16["diffMaps"].data_ptr() == e16.data_ptr() and r16["diffMaps"].dtype == torch.float16
    assert torch.equal(r16["hyps"], r32["hyps"])
    assert torch.equal(e16.view(torch.int16), e32.to(torch.float16).view(torch.int16))
    # not asserted beyond finiteness: the two score vectors differ by the rounding of the images, so the soft-argmax poses the refinement starts from do
    w32, w16 = r32["sfScores"].view(F, N), r16["sfScores"].view(F, N)
    for f in range(F):
        same = int(w32[f].argmax()) == int(w16[f].argmax())
        d = float((r16["refAvgHyp"][f] - r32["refAvgHyp"][f]).abs().max())
        print("frame %d: same argmax weight %s, max |refined pose (half) - refined pose (float)| = %.3e" % (f, same, d))
    assert bool(torch.isfinite(r16["refAvgHyp"]).all())


# ScoredFrameBatch in half against the float32 batch on the same inputs: K1, the K2 scores and K6 are bit-identical, only the score model's arithmetic
# (fp16 under autocast on fp16 images) differs.  Largest relative difference of grad_xyz measured on MI355X: see GRAD_REL_MEASURED; asserted: 4 x that or
# 1e-2, whichever is larger.
GRAD_REL_MEASURED = 1.493e-07  # measured on MI355X (2 frames x 128 x 40x40): path I dominates grad_xyz, the score model's gradient images are a small part of it


def test_scored_frame_batch_in_half(synth, orc):
    import torch
    from dsac_amd import e2e
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
    grads = {}
    for dt in (torch.float32, torch.float16):
        sb = e2e.ScoredFrameBatch(0, frames=F, hyps=N, sub_sample=sub, score_net=net, err_dtype=dt)
        sb.forward(xyz_d, uv_d, gt_d, perm_d, seed=1305)
        assert sb.err.dtype == dt
        for p in net.parameters():
            p.grad = None
        grads[dt] = sb.backward().clone()
        torch.cuda.synchronize()
        if dt == torch.float32:
            poses32, err32 = sb.poses.clone(), sb.err.clone()
        else:
            assert torch.equal(sb.poses, poses32)
            assert torch.equal(sb.err.view(torch.int16), err32.to(torch.float16).view(torch.int16))
    g32, g16 = grads[torch.float32], grads[torch.float16]
    assert bool(torch.isfinite(g16).all()) and float(g16.abs().max()) > 0.0
    rel = float((g16 - g32).abs().max() / g32.abs().max())
    print("ScoredFrameBatch half against float: max |grad_xyz difference| / max |grad_xyz| = %.3e" % rel)
    assert rel <= max(4.0 * GRAD_REL_MEASURED, 1e-2), rel
