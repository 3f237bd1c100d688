"""Frame batches with one camera per frame: dsac_set_frames_cams (Engine.set_frames(cam=<F x 4 array>)).

The contract: every call that accepts a batch gives the results of F single-frame calls, frame f under dsac_set_frame(..., cams[f]) with the seed
seed + f -- bit for bit wherever the shared-camera batch is bit for bit against single frames, and within the bounds tests/test_gpu_backward_batch.py
documents for K4 (fp32 partial sums grouped by the launch's workgroup count) elsewhere.  A table of equal rows gives dsac_set_frames bit for bit.

Cameras: CAMS covers three split exponents of K2's exact form (ceil(log2 f) = 10, 10, 9, 10, 10: 260 px next to 525 px is what a shared exponent would get
wrong) and one row with fx != fy (forward calls only).  Frame i is synth.chess_like_frame(H, W, seed=300 + i, cam=CAMS[i]).  Implicit-grid cases use cameras
scaled to the map (like _grid_frame of tests/test_gpu_backward_batch.py) with another scale and principal point per frame.  On the CPU oracle, with the seeds
41 + i, oracle.sample serves all 128 hypotheses of every frame of every case below and the largest translation is 10.2 m -- nothing is near the 131 m range of
the split records, so ok.all() is a fair precondition.

Shapes, the smallest that still reach every build of K2's exact form:
    40 x 40,   4 x 128, per-frame uv     the vector build, <64, 64> tile
    37 x 53,   3 x 128, per-frame uv     the any-map build and its tail launch (1 961 cells)
    48 x 64,   3 x 128, implicit grid    W % 64 == 0: the G64 build
    128 x 160, 2 x 128, implicit grid    P > 16 384: the <64, 256> tile
"""
import numpy as np
import pytest

from conftest import excl_clamp_edge, margin
from test_gpu_backward_batch import _grid_frame, dpnp_substitution_frame
from test_gpu_pipeline import oracle_backward

pytestmark = pytest.mark.gpu

CAMS = [(525.0, 525.0, 320.0, 240.0), (585.0, 585.0, 320.0, 240.0), (260.0, 260.0, 300.0, 250.0), (480.0, 520.0, 330.0, 235.0), (1000.0, 1000.0, 320.0, 240.0)]
VEC, ANY = "exact (vector build)", "exact (any-map build)"
SHAPES = [(40, 40, 4, 128, False, VEC), (37, 53, 3, 128, False, ANY), (48, 64, 3, 128, True, VEC), (128, 160, 2, 128, True, VEC)]
FWD_KEYS = ("hyps", "sampledPoints", "ok", "scores", "sfScores", "sfEntropy", "avgHyp", "refAvgHyp", "refSteps", "inlierMaps", "out4")
INVALID = -1


def _defaults(e):
    for key, v in (("k2_variant", -1), ("k2_flags", 0), ("k2_exact_auto", 1), ("k2_f16_store", 1), ("pi_defer_tail", 0), ("pi_refstream", 0), ("k6_waves", 0)):
        e.set_option(key, v)


@pytest.fixture()
def eng(engine):
    _defaults(engine)
    yield engine
    _defaults(engine)


def _grid_cam(H, W, f):
    """the camera of implicit-grid frame f: 525 px at 640 columns scaled to the map, then another scale and principal point per frame"""
    s = (1.0, 1.11, 0.52, 0.93)[f]
    return (525.0 * W / 640 * s, 525.0 * W / 640 * s, W / 2.0 + 3.0 * f, H / 2.0 - 2.0 * f)


_CASES = {}


def _case(synth, orc, H, W, F, implicit, first=0):
    """Frames, cameras, permutations and ground truths of one shape: made once, shared by the tests, left unchanged."""
    key = (H, W, F, implicit, first)
    if key not in _CASES:
        if implicit:
            cams = [_grid_cam(H, W, f) for f in range(F)]
            frames = [_grid_frame(synth, H, W, 300 + f, cams[f]) for f in range(F)]
        else:
            cams = [CAMS[first + f] for f in range(F)]
            frames = [synth.chess_like_frame(H, W, seed=300 + first + f, cam=cams[f]) for f in range(F)]
        _CASES[key] = dict(H=H, W=W, F=F, P=H * W, implicit=implicit, frames=frames, cams=np.array(cams, np.float32),
                           xyz=np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames])),
                           uv=None if implicit else np.ascontiguousarray(np.stack([fr["uv"] for fr in frames])),
                           perm=synth.fast_permutations(H * W, 8),
                           gts=np.stack([orc.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0])) for fr in frames]))
    return _CASES[key]


def _set_batch(e, c, cam=None):
    e.set_frames(c["xyz"], c["uv"], c["H"], c["W"], c["cams"] if cam is None else cam, uv_per_frame=c["uv"] is not None)


def _set_one(e, c, f, cam=None):
    e.set_frame(c["xyz"][f], None if c["uv"] is None else c["uv"][f], c["H"], c["W"], tuple(float(v) for v in c["cams"][f]) if cam is None else cam)


_FORWARD = {}


def _forward(e, c, N, seed=41):
    """dsac_process_images on the per-frame-camera batch (error images, inlier maps), once per shape"""
    key = (c["H"], c["W"], c["F"], c["implicit"], c["cams"].tobytes(), N, seed)
    if key not in _FORWARD:
        _set_batch(e, c)
        err = np.zeros((c["F"] * N, c["P"]), np.float32)
        b = e.processImages(N, c["perm"], gt_jp6=c["gts"], seed=seed, err=err, want_inlier_maps=True)
        _FORWARD[key] = (b, err, e.k2_form())
    return _FORWARD[key]


def _rows(b, key, f, N):
    return b[key][f * N:(f + 1) * N] if len(b[key]) != len(b["sfEntropy"]) else b[key][f:f + 1]


# ---- 1. forward == single frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,F,N,implicit,form", SHAPES)
def test_forward_equals_single_frame_calls(eng, orc, synth, H, W, F, N, implicit, form):
    c = _case(synth, orc, H, W, F, implicit)
    P = c["P"]
    b, err, k2 = _forward(eng, c, N)
    assert eng.get_option("frame_cams") == 1
    assert k2 == (form, 0)
    assert b["ok"].all()
    err_sh = np.zeros((F * N, P), np.float32)
    sh = eng.scoreHypothesesFrames(N, seed=41, err=err_sh)
    assert eng.k2_form() == (form, 0)
    for f in range(F):
        _set_one(eng, c, f)
        assert eng.get_option("frame_cams") == 0
        e1 = np.zeros((N, P), np.float32)
        s = eng.processImages(N, c["perm"], gt_jp6=c["gts"][f:f + 1], seed=41 + f, err=e1, want_inlier_maps=True)
        assert eng.k2_form() == (form, 0)
        for key in FWD_KEYS:
            assert np.array_equal(_rows(b, key, f, N), s[key]), (key, f)
        assert np.array_equal(err[f * N:(f + 1) * N], e1), f
        # dsac_score_hypotheses_frames against dsac_score_hypotheses under the frame's camera
        e2 = np.zeros((N, P), np.float32)
        s2 = eng.scoreHypotheses(N, seed=41 + f, err=e2)
        for got, want in zip(sh, s2):
            got = got[f * N:(f + 1) * N] if len(got) == F * N else got[f]
            assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)), f
        assert np.array_equal(err_sh[f * N:(f + 1) * N], e2), f
    # the companion: the same maps as a shared-camera batch under frame 0's camera give something else wherever the cameras differ
    _set_batch(eng, c, cam=tuple(float(v) for v in c["cams"][0]))
    assert eng.get_option("frame_cams") == 0
    err0 = np.zeros((F * N, P), np.float32)
    b0 = eng.processImages(N, c["perm"], gt_jp6=c["gts"], seed=41, err=err0, want_inlier_maps=True)
    assert np.array_equal(err0[:N], err[:N]) and np.array_equal(b0["refAvgHyp"][0], b["refAvgHyp"][0])
    for f in range(1, F):
        assert not np.array_equal(err0[f * N:(f + 1) * N], err[f * N:(f + 1) * N]), f
        assert not np.array_equal(b0["hyps"][f * N:(f + 1) * N], b["hyps"][f * N:(f + 1) * N]), f


def test_stage_calls_equal_single_frame_calls(eng, orc, synth):
    """dsac_sample (sets drawn) and dsac_reproject on a batch of all five cameras at 40 x 40, error images and soft-inlier sums"""
    H, W, F, N = 40, 40, 5, 128
    c = _case(synth, orc, H, W, F, False)
    _set_batch(eng, c)
    poses, sets, ok = eng.sample(F * N, seed=41)
    assert ok.all()
    err, soft = np.zeros((F * N, c["P"]), np.float32), np.zeros(F * N)
    eng.reproject(poses, err=err, soft=soft)
    assert eng.k2_form() == (VEC, 0)
    J = np.asarray(eng.dPNP(sets))
    for f in range(F):
        sl = slice(f * N, (f + 1) * N)
        _set_one(eng, c, f)
        p1, s1, ok1 = eng.sample(N, seed=41 + f)
        assert np.array_equal(poses[sl], p1) and np.array_equal(sets[sl], s1) and np.array_equal(ok[sl], ok1), f
        e1, so1 = np.zeros((N, c["P"]), np.float32), np.zeros(N)
        eng.reproject(p1, err=e1, soft=so1)
        assert np.array_equal(err[sl], e1) and np.array_equal(soft[sl], so1), f
        assert np.array_equal(J[sl], np.asarray(eng.dPNP(s1))), f
    _set_batch(eng, c, cam=CAMS[0])
    err0 = np.zeros((F * N, c["P"]), np.float32)
    eng.reproject(poses, err=err0)
    assert np.array_equal(err0[:N], err[:N]) and all(not np.array_equal(err0[f * N:(f + 1) * N], err[f * N:(f + 1) * N]) for f in range(1, F))


# ---- 2. equal rows == dsac_set_frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,F,N", [(40, 40, 4, 128), (37, 53, 3, 128)])
def test_equal_rows_equal_the_shared_camera_batch(eng, orc, synth, H, W, F, N):
    import dsac_amd
    c = _case(synth, orc, H, W, F, False)
    cam = CAMS[1]
    _set_batch(eng, c, cam=cam)
    assert eng.get_option("frame_cams") == 0
    ea = np.zeros((F * N, c["P"]), np.float32)
    a = eng.processImages(N, c["perm"], gt_jp6=c["gts"], seed=7, err=ea, want_inlier_maps=True)
    _set_batch(eng, c, cam=np.tile(np.array(cam, np.float32), (F, 1)))
    assert eng.get_option("frame_cams") == 1
    eb = np.zeros((F * N, c["P"]), np.float32)
    b = eng.processImages(N, c["perm"], gt_jp6=c["gts"], seed=7, err=eb, want_inlier_maps=True)
    assert np.array_equal(ea, eb)
    for key in FWD_KEYS:
        assert np.array_equal(a[key], b[key]), key
    # back to one frame: the table is gone, and the result is a fresh engine's
    _set_one(eng, c, 2)
    assert eng.get_option("frame_cams") == 0
    s = eng.processImages(N, c["perm"], gt_jp6=c["gts"][2:3], seed=9, want_inlier_maps=True)
    with dsac_amd.Engine(0) as fresh:
        _set_one(fresh, c, 2)
        t = fresh.processImages(N, c["perm"], gt_jp6=c["gts"][2:3], seed=9, want_inlier_maps=True)
    for key in FWD_KEYS:
        assert np.array_equal(s[key], t[key]), key


# ---- 3. against the oracle, every frame under its own camera --------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,F,N,implicit,form", SHAPES[:3])
def test_every_frame_against_the_oracle_under_its_own_camera(eng, orc, synth, H, W, F, N, implicit, form):
    """Tolerances: the error images as tests/test_gpu_k2_exact.py (1e-3 px off the clamp edge, softmax weights 1e-4), the soft-argmax pose as
    tests/test_gpu_forward.py (1e-10 given the weights), refined pose and loss as tests/test_gpu_process_images.py (1e-7, 1e-9; inlier maps identical)."""
    c = _case(synth, orc, H, W, F, implicit)
    b, err, _ = _forward(eng, c, N)
    uvg = np.stack(np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)), -1).reshape(-1, 2)
    for f in range(F):
        sl = slice(f * N, (f + 1) * N)
        cam = tuple(float(v) for v in c["cams"][f])
        uv = uvg if implicit else c["uv"][f]
        ref = orc.get_diff_maps(b["hyps"][sl], c["xyz"][f], uv, H, W, cam)
        m = excl_clamp_edge(err[sl], ref, 100.0)
        margin("a3", "per-frame cameras (%dx%d): error images of every frame vs the oracle under ITS camera, max |err - oracle| px" % (W, H),
               np.abs(err[sl] - ref)[m].max(), 1e-3)
        w_ref = orc.softMax(0.1 * orc.soft_inlier(ref, 10.0, 0.5))
        margin("a4", "per-frame cameras (%dx%d): softmax weights of every frame vs the oracle, max |w - oracle|" % (W, H), np.abs(b["sfScores"][sl] - w_ref).max(), 1e-4)
        margin("a5", "per-frame cameras (%dx%d): soft-argmax pose given equal weights and poses, max abs difference" % (W, H),
               np.abs(b["avgHyp"][f] - orc.avg_pose(b["sfScores"][sl], b["hyps"][sl])).max(), 1e-10)
        ref_o, imap_o, _ = orc.refine(b["avgHyp"][f], c["perm"], c["xyz"][f], uv, H, W, cam, want_inlier_map=True)
        margin("a6", "per-frame cameras (%dx%d): refined pose of every frame vs the oracle, max-rel (inlier maps identical)" % (W, H),
               np.abs(ref_o[0] - b["refAvgHyp"][f]).max() / max(1.0, np.abs(ref_o).max()), 1e-7)
        assert np.array_equal(imap_o, b["inlierMaps"][f]), f
        R1, t1 = orc.cv2our(b["refAvgHyp"][f])
        loss_o = orc.maxLoss(R1, t1, orc.rodrigues_vec2mat(c["gts"][f][:3]), c["gts"][f][3:])
        margin("a7", "per-frame cameras (%dx%d): loss of every frame vs the oracle, relative" % (W, H), abs(loss_o - b["out4"][f][0]) / max(1.0, loss_o), 1e-9)


# ---- 4. the 16-bit seam ---------------------------------------------------------------------------------------------------------------------
def _rounded_bits(a32, elem):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32))
    return t.to(torch.float16 if elem == "f16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _widen(bits, elem):
    import torch
    t = torch.from_numpy(bits.view(np.int16).copy())
    return t.view(torch.float16 if elem == "f16" else torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("elem", ["f16", "bf16"])
def test_sixteen_bit_seam(eng, orc, synth, elem):
    H, W, F, N = 40, 40, 3, 128
    c = _case(synth, orc, H, W, F, False)
    P = c["P"]
    _set_batch(eng, c)
    err32, soft32 = np.zeros((F * N, P), np.float32), np.zeros(F * N)
    p32 = eng.processImagesBegin(N, err32, seed=41, soft=soft32)
    assert eng.k2_form() == (VEC, 0) and p32[2].all()
    err16, soft16 = np.full((F * N, P), 0x5A5A, np.uint16), np.full(F * N, -1.0)
    p16 = eng.processImagesBegin(N, err16, seed=41, soft=soft16, elem=elem)
    assert eng.k2_form() == (VEC, 0)
    assert np.array_equal(err16, _rounded_bits(err32, elem))
    assert all(np.array_equal(a, b) for a, b in zip(p32, p16)) and np.array_equal(soft16.view(np.uint64), soft32.view(np.uint64))
    # K4 on 16-bit gradient images: the float call on the widened values, bit for bit, into a zeroed gradient.  Bit for bit needs an order-independent float
    # call (tests/test_gpu_k4_f16.py): the support scatter adds one fp64 atomic per hypothesis that has a cell in its set, so the scatter goes to sets that
    # share no cell within a frame (K5's Jacobians are those of the sampled sets: the identity does not ask the two to belong together)
    rng = np.random.default_rng(5)
    d16 = _rounded_bits((rng.standard_normal((F * N, P)) * 1e-3).astype(np.float32), elem)
    J = np.asarray(eng.dPNP(p32[1]))
    apart = np.concatenate([rng.permutation(P)[:4 * N].reshape(N, 4) for _ in range(F)]).astype(np.int32)
    g16 = eng.dScore(p32[0], apart, d16, dpnp=J, elem=elem, grad=np.zeros((F * P, 3)))
    G6_16 = eng.lastPoseGradients(F * N).copy()
    g32 = eng.dScore(p32[0], apart, _widen(d16, elem), dpnp=J, grad=np.zeros((F * P, 3)))
    assert np.abs(g32).max() > 0
    assert np.array_equal(g16, g32) and np.array_equal(G6_16, eng.lastPoseGradients(F * N))


# ---- 5. backward ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,F,N,implicit", [(40, 40, 3, 128, False), (37, 53, 2, 128, True)])
def test_backward_chain_with_per_frame_cameras(eng, orc, synth, H, W, F, N, implicit):
    """The chain of tests/test_gpu_backward_batch.py::test_backward_on_a_frame_batch -- path I, dSoftScore, dScore, dRefineFrames, dPNP -- on rows with fx == fy,
    against single frames under that file's documented bounds and against the oracle's chain of every frame under its own camera."""
    c = _case(synth, orc, H, W, F, implicit)
    P, perm, gts, xyz = c["P"], c["perm"], c["gts"], c["xyz"]
    assert (c["cams"][:, 0] == c["cams"][:, 1]).all()
    alpha, tau, beta, sub = 0.1, 10.0, 0.5, 0.2
    fwd, _, _ = _forward(eng, c, N)
    assert fwd["ok"].all()
    d_err = (np.random.default_rng(5).standard_normal((F * N, P)) * 1e-3).astype(np.float32)

    def backward(nf, sl, fsl):
        J = np.zeros((nf * N, 6, 12))
        r = eng.backwardPath1(fwd["hyps"][sl], fwd["sampledPoints"][sl], fwd["sfScores"][sl], fwd["avgHyp"][fsl], fwd["refAvgHyp"][fsl], gts[fsl], perm,
                              fwd["inlierMaps"][fsl], sub_sample=sub, out_dpnp=J)
        g_path1 = r["grad"].copy()
        g_soft = eng.dSoftScore(fwd["hyps"][sl], fwd["sampledPoints"][sl], r["g"] * alpha, tau=tau, beta=beta, dpnp=J)
        G6_soft = eng.lastPoseGradients(nf * N)
        g_derr = eng.dScore(fwd["hyps"][sl], fwd["sampledPoints"][sl], d_err[sl], dpnp=J)
        Jh, px, Jo, n = eng.dRefineFrames(fwd["avgHyp"][fsl], perm, fwd["inlierMaps"][fsl], sub_sample=sub, cap=64)
        return dict(path1=g_path1, g=r["g"].copy(), dL=np.asarray(r["dL"]).reshape(nf, 6), v6=np.asarray(r["v6"]).reshape(nf, 6), dpnp=J, soft=g_soft, G6=G6_soft,
                    derr=g_derr, Jh=Jh, px=px, Jo=Jo, n=n, dpnp_call=eng.dPNP(fwd["sampledPoints"][sl]))

    _set_batch(eng, c)
    b = backward(F, slice(0, F * N), slice(0, F))
    assert b["path1"].shape == (F * P, 3) and (b["n"] > 0).all()
    uvg = np.stack(np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)), -1).reshape(-1, 2)
    for f in range(F):
        cam = tuple(float(v) for v in c["cams"][f])
        _set_one(eng, c, f)
        hs, ps = slice(f * N, (f + 1) * N), slice(f * P, (f + 1) * P)
        s = backward(1, hs, slice(f, f + 1))
        for key, sl_ in (("g", hs), ("dL", slice(f, f + 1)), ("v6", slice(f, f + 1)), ("dpnp", hs), ("dpnp_call", hs), ("Jh", slice(f, f + 1)),
                         ("px", slice(f, f + 1)), ("Jo", slice(f, f + 1)), ("n", slice(f, f + 1))):
            assert np.array_equal(b[key][sl_], s[key]), (key, f)
        margin("a15", "per-frame cameras: frame batch vs single-frame call, path-I gradient (fp64 atomics on shared support cells): max |d| / max |g|",
               np.abs(b["path1"][ps] - s["path1"]).max() / max(np.abs(s["path1"]).max(), 1e-300), 1e-12)
        for key in ("soft", "derr"):
            margin("a15", "per-frame cameras: frame batch vs single-frame call, K4 gradient (%s): max |d| / max |g|" % key,
                   np.abs(b[key][ps] - s[key]).max() / max(np.abs(s[key]).max(), 1e-300), 1e-5)
        margin("a10", "per-frame cameras: frame batch vs single-frame call, K4 pose sums: max-rel",
               (np.abs(b["G6"][hs] - s["G6"]).max(1) / np.maximum(np.abs(s["G6"]).max(1), 1e-9 * np.abs(s["G6"]).max() + 1e-300)).max(), 1e-4)
        # the batch's frame f against the oracle's chain under the frame's own camera
        uvh = uvg if implicit else c["uv"][f]
        fr = dict(c["frames"][f], uv=uvh, cam=cam)
        fw = dict(hyps=fwd["hyps"][hs], sampledPoints=fwd["sampledPoints"][hs], sfScores=fwd["sfScores"][hs], avgHyp=fwd["avgHyp"][f], refAvgHyp=fwd["refAvgHyp"][f],
                  pixelIdxs=perm, inlierMap=fwd["inlierMaps"][f], score_scale=alpha)
        ref_grad, dL, v6, g, coef6 = oracle_backward(orc, fr, fw, gts[f], tau=tau, beta=beta, sub_sample=sub)
        ref_grad = ref_grad + dpnp_substitution_frame(eng, orc, fr, xyz[f], None if implicit else c["uv"][f], H, W, cam, fw["sampledPoints"], coef6)
        got = b["soft"][ps] + b["path1"][ps]
        scale = np.abs(ref_grad).max()
        assert scale >= 1e-6 * np.abs(dL).max()
        margin("a15", "per-frame cameras: end-to-end gradient of every frame vs the oracle's chain under its camera, max-rel", np.abs(got - ref_grad).max() / scale, 1e-5)
        margin("a8", "per-frame cameras: dLossMax of every frame vs oracle", np.abs(b["dL"][f] - dL).max() / max(1.0, np.abs(dL).max()), 1e-8)
        # the companion: under frame 0's camera the single-frame K4 gradient of a frame with another camera is something else
        if f > 0:
            _set_one(eng, c, f, cam=tuple(float(v) for v in c["cams"][0]))
            other = eng.dScore(fwd["hyps"][hs], fwd["sampledPoints"][hs], d_err[hs], dpnp=b["dpnp"][hs])
            assert np.abs(other - s["derr"]).max() > 1e-3 * np.abs(s["derr"]).max()


# ---- 6. K6: the scan path ------------------------------------------------------------------------------------------------------------------
def test_refinement_scan_path_equals_the_fused_kernel_and_single_frames(eng, orc, synth):
    """2 frames x 16 problems on 128 x 128: 16 384 cells and 32 problems, the scan's threshold.  CAMS[0] and CAMS[2]; starts near the truth and random ones (long
    walks).  The scan (k6_waves 0), the fused kernel (k6_waves 1) and the single-frame calls (16 problems: the fused kernel) agree bit for bit."""
    H, W, F, K = 128, 128, 2, 16
    cams = [CAMS[0], CAMS[2]]
    frames = [synth.chess_like_frame(H, W, seed=300 + i, cam=cams[i]) for i in range(F)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    uv = np.ascontiguousarray(np.stack([fr["uv"] for fr in frames]))
    perm = synth.fast_permutations(H * W, 8, seed=3)
    rng = np.random.default_rng(17)
    init = np.zeros((F * K, 6))
    for f in range(F):
        good = frames[f]["gt_pose"] + rng.normal(size=(K, 6)) * np.array([0.01, 0.01, 0.01, 10.0, 10.0, 10.0])
        rand = frames[f]["gt_pose"] + rng.normal(size=(K, 6)) * np.array([0.3, 0.3, 0.3, 400.0, 400.0, 400.0])
        init[f * K:(f + 1) * K] = np.where((np.arange(K) % 2 == 0)[:, None], good, rand)
    table = np.array(cams, np.float32)
    eng.set_frames(xyz, uv, H, W, table, uv_per_frame=True)
    scan = eng.refineAll(init, perm, want_inlier_maps=True)
    eng.set_option("k6_waves", 1)
    fused = eng.refineAll(init, perm, want_inlier_maps=True)
    eng.set_option("k6_waves", 0)
    print("steps done per problem:", scan[1])
    assert (scan[1] == 8).any()
    for a, b in zip(scan, fused):
        assert np.array_equal(a, b)
    for f in range(F):
        sl = slice(f * K, (f + 1) * K)
        eng.set_frame(xyz[f], uv[f], H, W, cams[f])
        one = eng.refineAll(init[sl], perm, want_inlier_maps=True)
        for a, b in zip(scan, one):
            assert np.array_equal(a[sl], b), f
    # the companion: the second frame under the first frame's camera refines to something else
    eng.set_frames(xyz, uv, H, W, cams[0], uv_per_frame=True)
    shared = eng.refineAll(init, perm, want_inlier_maps=True)
    assert np.array_equal(shared[0][:K], scan[0][:K]) and not np.array_equal(shared[0][K:], scan[0][K:])


# ---- 7. the DSAC variant -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,F,N,own_uv", [(40, 40, 3, 64, True), (48, 64, 4, 32, False), (480, 640, 2, 16, None), (37, 53, 2, 24, False), (23, 77, 3, 40, True)])
def test_dsac_variant_with_per_frame_cameras(eng, orc, synth, H, W, F, N, own_uv):
    """dsac_refine_all and dsac_refine_fd_sets_frames at the shapes of tests/test_gpu_dsac_variant_batch.py == the single-frame calls under each camera"""
    from dsac_amd.capi import lib, ptr, check
    P = H * W
    cams = CAMS[:F]
    frames = [synth.chess_like_frame(H, W, seed=1200 + f, cam=cams[f], quantise_int16=(H == 40)) for f in range(F)]
    xyz = np.ascontiguousarray(np.stack([fr["xyz"] for fr in frames]))
    uv = None if own_uv is None else (np.ascontiguousarray(np.stack([fr["uv"] for fr in frames])) if own_uv else frames[0]["uv"])
    uv_of = (lambda f: None) if own_uv is None else ((lambda f: uv[f]) if own_uv else (lambda f: uv))
    perm = synth.fast_permutations(P, 8)
    table = np.array(cams, np.float32)
    poses, sets = np.zeros((F * N, 6)), np.zeros((F * N, 4), np.int32)
    for f in range(F):
        eng.set_frame(xyz[f], uv_of(f), H, W, cams[f])
        poses[f * N:(f + 1) * N], sets[f * N:(f + 1) * N], _ = eng.sample(N, seed=60 + f)
    eng.set_frames(xyz, uv, H, W, table, uv_per_frame=bool(own_uv))
    ref_b, sd_b, maps_b = eng.refineAll(poses, perm, sets=sets, want_inlier_maps=True)
    assert (sd_b > 0).any()
    rng = np.random.default_rng(3)
    sel = np.concatenate([f * N + np.sort(rng.choice(N, size=2 + f, replace=False)) for f in range(F)]).astype(np.int32)
    frame_of = (sel // N).astype(np.int32)
    M, cap = len(sel), 8
    Js_b, px_b, Jo_b, n_b = np.zeros((M, 6, 9)), np.zeros((M, cap), np.int32), np.zeros((M, cap, 6, 3)), np.zeros(M, np.int32)
    ssel, msel = np.ascontiguousarray(sets[sel]), np.ascontiguousarray(maps_b[sel])  # held here: ptr() takes an address, not a reference
    check(eng._ctx, lib.dsac_refine_fd_sets_frames(eng._ctx, M, ptr(ssel), ptr(frame_of), ptr(perm), 8, 100, 50, 10.0, ptr(msel), 0.05, 2.0, ptr(Js_b), ptr(px_b),
                                                   ptr(Jo_b), cap, ptr(n_b)))
    for f in range(F):
        eng.set_frame(xyz[f], uv_of(f), H, W, cams[f])
        sl = slice(f * N, (f + 1) * N)
        r1, sd1, m1 = eng.refineAll(poses[sl], perm, sets=sets[sl], want_inlier_maps=True)
        assert np.array_equal(ref_b[sl], r1) and np.array_equal(sd_b[sl], sd1) and np.array_equal(maps_b[sl], m1), f
        k = np.flatnonzero(frame_of == f)
        Js, n1, px, Jo = eng.dRefineSets(sets[sel[k]], perm, maps_b[sel[k]], sub_sample=0.05, cap=cap)
        assert np.array_equal(Js, Js_b[k]) and np.array_equal(n1, n_b[k]), f
        for a, m in enumerate(k):
            assert np.array_equal(px[a][:n1[a]], px_b[m][:n_b[m]]) and np.array_equal(Jo[a][:n1[a]], Jo_b[m][:n_b[m]]), (f, a)


# ---- 8. the reference stream ---------------------------------------------------------------------------------------------------------------
def test_reference_stream_with_per_frame_cameras(eng, orc, synth):
    """"pi_refstream" on 40 x 40, 3 x 128, one generator: sets, counters and poses == the image-by-image calls on the running generator under each camera"""
    H, W, F, N = 40, 40, 3, 128
    c = _case(synth, orc, H, W, F, False)
    eng.refstreamInit(1305, 1)
    _set_batch(eng, c)
    b = eng.processImages(N, c["perm"], gt_jp6=c["gts"], seed=0, want_inlier_maps=True, refstream=True)
    eng.refstreamInit(1305, 1)
    cb = eng.sampleRefstreamFrames(N)
    assert np.array_equal(cb[0], b["hyps"]) and np.array_equal(cb[1], b["sampledPoints"])
    eng.refstreamInit(1305, 1)
    for f in range(F):
        _set_one(eng, c, f)
        s = eng.processImages(N, c["perm"], gt_jp6=c["gts"][f:f + 1], seed=0, want_inlier_maps=True, refstream=True)
        for key in FWD_KEYS:
            assert np.array_equal(_rows(b, key, f, N), s[key]), (key, f)
    eng.refstreamInit(1305, 1)
    for f in range(F):
        _set_one(eng, c, f)
        p1, s1, ok1, c1, a1 = eng.sampleRefstreamFrames(N)
        sl = slice(f * N, (f + 1) * N)
        assert np.array_equal(cb[0][sl], p1) and np.array_equal(cb[1][sl], s1) and np.array_equal(cb[2][sl], ok1), f
        assert np.array_equal(cb[3][f], c1[0]) and np.array_equal(cb[4][f], a1[0]), f
    eng.set_option("pi_refstream", 0)


# ---- 9. the range census -------------------------------------------------------------------------------------------------------------------
def test_range_census_is_the_sum_of_the_per_frame_calls(eng, orc, synth):
    H, W, F, N = 40, 40, 3, 128
    c = _case(synth, orc, H, W, F, False)
    b, _, _ = _forward(eng, c, N)
    poses = b["hyps"].copy()
    poses[N + 5, 5] = 200000.0  # t_z = 200 m in frame 1: beyond the split records' 131 m
    _set_batch(eng, c)
    far, oor = eng.k2_census(poses)
    singles = []
    for f in range(F):
        _set_one(eng, c, f)
        singles.append(eng.k2_census(poses[f * N:(f + 1) * N]))
    assert oor == sum(s[1] for s in singles) and oor >= 1 and singles[1][1] >= 1
    assert far == sum(s[0] for s in singles)
    _set_batch(eng, c)
    with pytest.raises(Exception, match="frames x"):
        eng.k2_census(poses[:F * N - 1])


# ---- 10. ordering --------------------------------------------------------------------------------------------------------------------------
def test_deferred_tail_and_table_lifetime(eng, orc, synth):
    """"pi_defer_tail" 1: two consecutive dsac_process_images calls on two batches with different tables and different output arrays -- the refinement tail of the
    first still reads its table while the second batch is set -- equal the in-order run bit for bit.  And the caller's array may be overwritten as soon as
    dsac_set_frames_cams has returned."""
    import torch
    from dsac_amd.capi import lib, ptr, check, DSAC_FRAME_BORROW
    H, W, F, N = 40, 40, 3, 128
    dev = torch.device("cuda", 0)
    cases = [_case(synth, orc, H, W, F, False), _case(synth, orc, H, W, F, False, first=2)]
    assert not np.array_equal(cases[0]["cams"], cases[1]["cams"])
    P = H * W
    perm = torch.from_numpy(cases[0]["perm"]).to(dev)
    dxyz = [torch.from_numpy(c["xyz"]).to(dev) for c in cases]
    duv = [torch.from_numpy(c["uv"]).to(dev) for c in cases]
    gts = [torch.from_numpy(c["gts"]).to(dev) for c in cases]

    def bufs():
        n = F * N
        return dict(hyps=torch.zeros(n, 6, dtype=torch.float64, device=dev), sampledPoints=torch.zeros(n, 4, dtype=torch.int32, device=dev),
                    ok=torch.zeros(n, dtype=torch.uint8, device=dev), scores=torch.zeros(n, dtype=torch.float64, device=dev),
                    sfScores=torch.zeros(n, dtype=torch.float64, device=dev), sfEntropy=torch.zeros(F, dtype=torch.float64, device=dev),
                    avgHyp=torch.zeros(F, 6, dtype=torch.float64, device=dev), refAvgHyp=torch.zeros(F, 6, dtype=torch.float64, device=dev),
                    refSteps=torch.zeros(F, dtype=torch.int32, device=dev), out4=torch.zeros(F, 4, dtype=torch.float64, device=dev),
                    inlierMaps=torch.zeros(F, P, dtype=torch.int32, device=dev))

    def run(defer, clobber):
        eng.set_option("pi_defer_tail", int(defer))
        outs = [bufs(), bufs()]
        torch.cuda.synchronize(dev)
        for k in range(2):
            if clobber:  # the C call itself, then the caller's array is overwritten before anything has been synchronised
                table = cases[k]["cams"].copy()
                check(eng._ctx, lib.dsac_set_frames_cams(eng._ctx, F, ptr(dxyz[k]), ptr(duv[k]), 1, H, W, ptr(table), DSAC_FRAME_BORROW))
                table[:] = 77.0
                eng.H, eng.W, eng.P, eng.frames = H, W, P, F
            else:
                eng.set_frames(dxyz[k], duv[k], H, W, cases[k]["cams"], uv_per_frame=True, borrow=True)
            eng.processImages(N, perm, gt_jp6=gts[k], seed=41, out=outs[k])
        eng.joinTail()
        eng.synchronize()
        return [{key: v.cpu().numpy().copy() for key, v in o.items()} for o in outs]

    try:
        plain = run(0, False)
        assert all(o["ok"].all() for o in plain)
        for other in (run(1, False), run(1, True), run(0, True)):
            for a, b in zip(plain, other):
                for key in a:
                    assert np.array_equal(a[key], b[key]), key
        # what the in-order run computed is the host-array call's result
        for k in range(2):
            b, _, _ = _forward(eng, cases[k], N)
            for key in FWD_KEYS:
                assert np.array_equal(np.asarray(b[key]).reshape(-1), plain[k][key].reshape(-1)), key
    finally:
        eng.set_option("pi_defer_tail", 0)


# ---- 11. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng, orc, synth):
    import torch
    from dsac_amd.capi import lib, ptr, DsacError
    H, W, F, N = 40, 40, 4, 128
    c = _case(synth, orc, H, W, F, False)
    P = c["P"]
    b, _, _ = _forward(eng, c, N)  # leaves k2_form_last at the exact vector build
    poses, sets = b["hyps"], b["sampledPoints"]
    _set_batch(eng, c)
    err = np.zeros((F * N, P), np.float32)
    eng.reproject(poses, err=err)
    form = eng.get_option("k2_form_last")
    assert (eng.k2_form()[0], form) == (VEC, 4)

    def refused(call, *words):
        before = err.copy()
        with pytest.raises(DsacError) as ei:
            call()
        assert ei.value.code == INVALID, ei.value
        for w in words:
            assert w in str(ei.value), (w, str(ei.value))
        assert eng.get_option("k2_form_last") == form
        assert np.array_equal(err, before)

    # K2: a focal length above 1 024 px in one row, and every option that would name another form
    wide = c["cams"].copy()
    wide[2, :2] = 1100.0
    _set_batch(eng, c, cam=wide)
    refused(lambda: eng.reproject(poses, err=err), "1024", "frame 2")
    refused(lambda: eng.processImages(N, c["perm"]), "1024")
    refused(lambda: eng.scoreHypothesesFrames(N), "1024")
    _set_batch(eng, c)
    for key, value, word in (("k2_variant", 84, "k2_variant"), ("k2_flags", 1 << 25, "k2_flags"), ("k2_exact_auto", 0, "k2_exact_auto")):
        eng.set_option(key, value)
        try:
            refused(lambda: eng.reproject(poses, err=err), word)
            refused(lambda: eng.processImagesBegin(N, err), word)
        finally:
            _defaults(eng)
    eng.set_option("k2_flags", 1 << 28)  # bits 28 / 29 ask for the form that runs anyway
    e2 = np.zeros_like(err)
    eng.reproject(poses, err=e2)
    _defaults(eng)
    assert np.array_equal(e2, err)
    # the backward calls: the row with fx != fy, by its frame index
    d_err = np.zeros((F * N, P), np.float32)
    refused(lambda: eng.dScore(poses, sets, d_err), "fx == fy", "frame 3")
    refused(lambda: eng.dSoftScore(poses, sets, np.zeros(F * N)), "fx == fy", "frame 3")
    refused(lambda: eng.backwardPath1(poses, sets, b["sfScores"], b["avgHyp"], b["refAvgHyp"], c["gts"], c["perm"], b["inlierMaps"], sub_sample=0.2), "fx == fy", "frame 3")
    # the pipelined pair
    dev = torch.device("cuda", 0)
    dp, ds, dk = torch.zeros(F * N, 6, dtype=torch.float64, device=dev), torch.zeros(F * N, 4, dtype=torch.int32, device=dev), torch.zeros(F * N, dtype=torch.uint8, device=dev)
    refused(lambda: eng.sampleAhead(0, F * N, 41, dp, ds, dk), "dsac_sample_ahead", "per-frame cameras")
    # the call itself: NULL, a device pointer, a zero and a NaN focal length -- nothing changes in the context
    ctx = eng._ctx
    args = (ctx, F, ptr(c["xyz"]), ptr(c["uv"]), 1, H, W)
    assert lib.dsac_set_frames_cams(*args, None, 0) == INVALID and b"cams is NULL" in lib.dsac_last_error(ctx)
    dcams = torch.from_numpy(c["cams"]).to(dev)
    assert lib.dsac_set_frames_cams(*args, ptr(dcams), 0) == INVALID and b"device pointer" in lib.dsac_last_error(ctx)
    for bad in (0.0, np.nan, np.inf):
        t = c["cams"].copy()
        t[1, 1] = bad
        assert lib.dsac_set_frames_cams(*args, ptr(t), 0) == INVALID
        msg = lib.dsac_last_error(ctx)
        assert b"focal length" in msg and b"row 1" in msg, msg
    assert eng.get_option("frame_cams") == 1 and eng.get_option("k2_form_last") == form
    e3 = np.zeros_like(err)
    eng.reproject(poses, err=e3)  # the batch and its table are what they were
    assert np.array_equal(e3, err)
    with pytest.raises(ValueError):
        eng.set_frames(c["xyz"], c["uv"], H, W, c["cams"][:, :3], uv_per_frame=True)


# ---- 12. e2e.ScoredFrameBatch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_scored_frame_batch_with_a_camera_table(eng, orc, synth, dtype):
    """e2e.ScoredFrameBatch(cam=<F x 4>) end to end -- begin, the score model on the error images, finish, path I, the model's backward, K4 -- in float, binary16
    and bfloat16.  What the library computes in front of the model is compared bit for bit with the single-frame begin call under each frame's camera (poses,
    sets, error images; the 16-bit images are torch's rounding of the float ones); behind the model the run has to be finite, non-zero and -- for the frame whose
    camera is not row 0 -- something else than the shared-camera batch under row 0.  Two frames x 128 hypotheses: the smallest count the seam takes for a batch."""
    import torch
    from dsac_amd import e2e
    S, F, N, sub = 40, 2, 128, 0.05
    c = _case(synth, orc, S, S, F, False)
    assert (c["cams"][:, 0] == c["cams"][:, 1]).all()
    dt = getattr(torch, dtype)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)

    class Net(torch.nn.Module):  # two small matrix products, as in tests/test_gpu_k4_bf16.py: e2e.ScoreNet's convolutions cost half a minute of kernel selection
        def __init__(self):      # on their first bfloat16 call, and what is checked here is on the library's side of the seam
            super().__init__()
            self.a, self.b = torch.nn.Linear(S * S, 16), torch.nn.Linear(16, 1)

        def forward(self, err):
            return self.b(torch.relu(self.a(err.flatten(1) * 0.01))).squeeze(1)

    net = Net().to(dev)
    perm_d, gt_d = torch.as_tensor(c["perm"], device=dev), torch.as_tensor(c["gts"], device=dev)
    xyz_d, uv_d = torch.as_tensor(c["xyz"], device=dev).contiguous(), torch.as_tensor(c["uv"], device=dev).contiguous()

    def run(frames, cam, xyz, uv, gt, seed, err_dtype=dt):
        sb = e2e.ScoredFrameBatch(0, frames=frames, hyps=N, sub_sample=sub, score_net=net, cam=cam, err_dtype=err_dtype)
        res = sb.forward(xyz, uv, gt, perm_d, seed=seed)
        for p in net.parameters():
            p.grad = None
        grad = sb.backward().clone()
        torch.cuda.synchronize()
        assert sb.err.dtype == err_dtype and sb.engine.get_option("frame_cams") == (1 if np.ndim(cam) == 2 else 0)
        return dict(poses=sb.poses.clone(), sets=sb.sets.clone(), err=sb.err.reshape(frames * N, -1).clone(), grad=grad, ref=res["refAvgHyp"].clone(), ok=sb.ok.clone())

    b = run(F, c["cams"], xyz_d, uv_d, gt_d, 41)
    assert bool(b["ok"].all()) and bool(torch.isfinite(b["grad"]).all()) and float(b["grad"].abs().max()) > 0.0
    if dt != torch.float32:
        b32 = run(F, c["cams"], xyz_d, uv_d, gt_d, 41, err_dtype=torch.float32)
        assert torch.equal(b["poses"], b32["poses"]) and torch.equal(b["err"].view(torch.int16), b32["err"].to(dt).view(torch.int16))
    bits = torch.int32 if dt == torch.float32 else torch.int16
    for f in range(F):
        _set_one(eng, c, f)
        e1 = torch.zeros(N, S * S, dtype=dt, device=dev)
        p1, s1, _ = eng.processImagesBegin(N, e1, seed=41 + f)
        eng.synchronize()
        sl = slice(f * N, (f + 1) * N)
        assert np.array_equal(b["poses"][sl].cpu().numpy(), p1) and np.array_equal(b["sets"][sl].cpu().numpy(), s1), f
        assert torch.equal(b["err"][sl].view(bits), e1.view(bits)), f
    shared = run(F, tuple(float(v) for v in c["cams"][0]), xyz_d, uv_d, gt_d, 41)
    assert torch.equal(shared["err"][:N], b["err"][:N])
    for f in range(1, F):
        assert not torch.equal(shared["err"][f * N:(f + 1) * N], b["err"][f * N:(f + 1) * N]), f
        assert not torch.equal(shared["grad"][f], b["grad"][f]), f
