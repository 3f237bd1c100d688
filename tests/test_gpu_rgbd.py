"""RGB-D localisation on the GPU through the C ABI (Engine): camera points, dsac_sample_rgbd, dsac_score_rgbd, dsac_refine_rgbd and the pipelines against
tests/rgbd_ref.py.  Shapes are the smallest at which the kernels can go wrong (ragged maps, ragged hypothesis tiles, round boundaries of the sampler)."""
import numpy as np
import pytest

import rgbd_ref as ref
from conftest import margin
from dsac_amd import capi

pytestmark = pytest.mark.gpu
TAU, BETA, CLAMP = 100.0, 0.05, 1000.0


def _set(engine, H, W, xyz, cam):
    """one frame or a batch, with its camera points"""
    if xyz.shape[0] == 1:
        engine.set_frame(xyz[0], None, H, W)
    else:
        engine.set_frames(xyz, None, H, W)
    engine.set_camera_points(cam)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. camera points -------------------------------------------------------------------------------------------------------------------------------
def test_camera_points_copy_counts_and_clearing(engine):
    H, W = 37, 53
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=31, frames=3, missing_frac=0.1)
    assert np.isinf(cam).any() and (cam[..., 2] == 0).any() and (cam[..., 2] < 0).any() and np.isnan(xyz).any()
    engine.set_frames(xyz, None, H, W)
    assert engine.get_option("camera_points") == 0
    with pytest.raises(capi.DsacError, match="no camera points"):
        engine.camera_points()
    engine.set_camera_points(cam)
    assert engine.get_option("camera_points") == 1
    want, n = ref.canonical(xyz, cam)
    got, n_got = engine.camera_points()
    assert _same(got, want) and np.array_equal(n_got, n)
    engine.set_camera_points(None)
    assert engine.get_option("camera_points") == 0
    for setter in (lambda: engine.set_frame(xyz[0], None, H, W), lambda: engine.set_frames(xyz, None, H, W),
                   lambda: engine.set_frames(xyz, None, H, W, cam=np.tile(np.float32([525, 525, 320, 240]), (3, 1)))):
        engine.set_frames(xyz, None, H, W)
        engine.set_camera_points(cam)
        assert engine.get_option("camera_points") == 1
        setter()
        assert engine.get_option("camera_points") == 0
    # the depth helper: back-projection through the implicit grid gives the points the frame was generated from
    from dsac_amd import synth
    fr = synth.chess_like_frame_rgbd(H, W, seed=5, grid_uv=True)
    engine.set_frame(fr["xyz"], None, H, W, cam=fr["cam"])
    pts = engine.set_depth(fr["depth"])
    got, n_got = engine.camera_points()
    assert int(n_got[0]) == int((~fr["missing_mask"]).sum()) and _same(got[0], pts[0])
    assert np.allclose(got[0][~fr["missing_mask"]], fr["cam_xyz"][~fr["missing_mask"]], rtol=1e-5, atol=1e-2)


# ---- 2. sampling, given sets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 40), (37, 53)])
def test_given_sets_match_the_svd_kabsch(engine, H, W):
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=60 + W, missing_frac=0.1)
    _set(engine, H, W, xyz, cam)
    canon = ref.canonical(xyz, cam)[0][0]
    valid = np.flatnonzero(ref.valid_cells(xyz[0], cam[0]))
    rng = np.random.default_rng(3)
    sets = np.array([rng.choice(valid, 3, replace=False) for _ in range(512)], np.int32)
    thr = 400.0  # between the inlier triples (tens of mm) and triples with an outlier cell (metres)
    poses, sets_out, ok = engine.sampleRGBD(512, sets=sets, thr=thr)
    assert np.array_equal(sets_out, sets)
    well, near, worst, wrong = 0, 0, 0.0, 0
    for i, s in enumerate(sets):
        p, R, t = ref.kabsch3(xyz[0], canon, s)
        res = ref.residuals3(xyz[0], canon, s, R, t)
        qa, qs = ref.triangle_quality(xyz[0][s].astype(np.float64))
        ca, cs = ref.triangle_quality(canon[s].astype(np.float64))
        if np.abs(res - thr).min() <= 1e-6:
            near += 1
        else:
            wrong += int(ok[i]) != int(ref.accept3(p, res, thr))
        if min(qa, ca) >= 5.0 and min(qs, cs) >= 50.0:
            well += 1
            if ok[i]:
                worst = max(worst, float((np.abs(poses[i] - p) / np.maximum(1.0, np.abs(p))).max()))
    assert wrong == 0
    assert 0 < ok.sum() < 512
    margin("rgbd2", "share of well-conditioned triples (angle >= 5 deg, sides >= 50 mm), %dx%d" % (W, H), well / 512.0, 0.9, at_least=True)
    margin("rgbd2", "share of triples with a residual within 1e-6 mm of thr, %dx%d" % (W, H), near / 512.0, 0.01)
    margin("rgbd2", "given sets: |pose - SVD Kabsch| / max(1, |.|) on well-conditioned triples, %dx%d" % (W, H), worst, 1e-9)
    assert np.array_equal(poses[ok == 0], np.zeros((int((ok == 0).sum()), 6)))


def test_given_sets_with_bad_cells(engine):
    H, W = 40, 40
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=61, missing_frac=0.1)
    _set(engine, H, W, xyz, cam)
    v = ref.valid_cells(xyz[0], cam[0])
    good, bad = np.flatnonzero(v), np.flatnonzero(~v)
    sets = np.array([[good[0], good[1], good[0]], [good[0], -1, good[2]], [good[0], good[1], H * W], [bad[0], good[1], good[2]], [good[3], good[4], good[5]]], np.int32)
    poses, sets_out, ok = engine.sampleRGBD(len(sets), sets=sets, thr=1e9)
    assert np.array_equal(ok, [0, 0, 0, 0, 1]) and np.array_equal(sets_out, sets)
    assert np.array_equal(poses[:4], np.zeros((4, 6))) and np.abs(poses[4]).max() > 0


# ---- 3. sampling, drawn sets: bit for bit the reference's walk with the library's own evaluation of every attempt -----------------------------------------
def _walk_frames(engine, H, W, xyz, cam, Nf, seed, stride, thr, max_tries):
    """the reference's result for every frame: attempts from rgbd_ref, acceptance and pose of each attempt from the library's given-sets path on that frame"""
    poses, sets, oks = [], [], []
    for f in range(xyz.shape[0]):
        valid = ref.valid_cells(xyz[f], cam[f])
        if valid.sum() < 3:
            poses.append(np.zeros((Nf, 6))); sets.append(np.zeros((Nf, 3), np.int32)); oks.append(np.zeros(Nf, np.uint8))
            continue
        att = ref.attempt_sets(Nf, seed + f * stride, W, H, valid, max_tries)
        flat = np.array([s if s is not None else [0, 0, 0] for a in att for s in a], np.int32)
        engine.set_frame(xyz[f], None, H, W)
        engine.set_camera_points(cam[f])
        gp, _, gok = engine.sampleRGBD(len(flat), sets=flat, thr=thr)
        gp, gok = gp.reshape(Nf, max_tries, 6), gok.reshape(Nf, max_tries)
        pf, sf, of = np.zeros((Nf, 6)), np.zeros((Nf, 3), np.int32), np.zeros(Nf, np.uint8)
        for h in range(Nf):
            look = {tuple(s): (bool(gok[h, a]), gp[h, a]) for a, s in enumerate(att[h]) if s is not None}
            pf[h], sf[h], of[h] = ref.walk(att[h], lambda s: look[tuple(s)])
        poses.append(pf); sets.append(sf); oks.append(of)
    return np.concatenate(poses), np.concatenate(sets), np.concatenate(oks)


@pytest.mark.parametrize("H,W,F,Nf,max_tries,stride,thr", [
    (40, 40, 1, 257, 3, 1, 60.0), (37, 53, 1, 65, 70, 1, 25.0), (3, 5, 1, 63, 3, 1, 200.0), (40, 40, 1, 64, 1, 1, 60.0), (40, 40, 1, 1, 70, 1, 25.0),
    (40, 40, 3, 128, 3, 1, 60.0), (40, 40, 3, 128, 3, 5, 60.0), (40, 40, 1, 65, 70, 1, 1e-9)])
def test_drawn_sets_are_the_reference_walk_bit_for_bit(engine, H, W, F, Nf, max_tries, stride, thr):
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=70 + H * W + F, frames=F, missing_frac=0.1 if H * W > 15 else 0.3)
    want = _walk_frames(engine, H, W, xyz, cam, Nf, 1305, stride, thr, max_tries)
    engine.set_option("seed_stride", stride)
    try:
        _set(engine, H, W, xyz, cam)
        poses, sets, ok = engine.sampleRGBD(F * Nf, seed=1305, thr=thr, max_tries=max_tries)
    finally:
        engine.set_option("seed_stride", 1)
    assert np.array_equal(ok, want[2]) and np.array_equal(sets, want[1])
    assert poses.tobytes() == want[0].tobytes()
    if thr < 1e-6:
        assert ok.sum() == 0 and np.abs(sets).max() > 0  # nothing accepted: the sets of the last attempt
    elif max_tries >= 3 and Nf > 8:
        assert 0 < ok.sum()


def test_frames_with_three_and_two_valid_cells(engine):
    H, W = 40, 40
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=75, frames=2, dirty=False, missing_frac=0.0, noise_mm=0.0, outlier_frac=0.0, depth_noise_mm=0.0)
    keep3, keep2 = [17, 803, 1422], [5, 900]
    for f, keep in ((0, keep3), (1, keep2)):
        m = np.ones(H * W, bool)
        m[keep] = False
        cam[f][m] = np.nan
    want = _walk_frames(engine, H, W, xyz[:1], cam[:1], 64, 9, 1, 100.0, 70)
    _set(engine, H, W, xyz, cam)
    assert np.array_equal(engine.camera_points()[1], [3, 2])
    poses, sets, ok = engine.sampleRGBD(128, seed=9, thr=100.0, max_tries=70)
    assert np.array_equal(ok[:64], want[2]) and np.array_equal(sets[:64], want[1]) and poses[:64].tobytes() == want[0].tobytes()
    assert not ok[64:].any() and not sets[64:].any() and not poses[64:].any()
    for h in np.flatnonzero(ok[:64]):
        assert sorted(sets[h]) == keep3
    # two VALID cells: every hypothesis fails at once, whatever max_tries is
    engine.set_frame(xyz[1], None, H, W)
    engine.set_camera_points(cam[1])
    poses, sets, ok = engine.sampleRGBD(256, seed=9, thr=100.0, max_tries=1 << 20)
    assert not ok.any() and not sets.any() and not poses.any()


def test_sampling_refusals(engine):
    H, W = 40, 40
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=76, frames=2, missing_frac=0.1)
    engine.set_frames(xyz, None, H, W)
    with pytest.raises(capi.DsacError, match="no camera points"):
        engine.sampleRGBD(8)
    engine.set_camera_points(cam)
    with pytest.raises(capi.DsacError, match="frame batch"):
        engine.sampleRGBD(8, sets=np.zeros((8, 3), np.int32))
    with pytest.raises(capi.DsacError, match="frame batch"):
        engine.sampleRGBD(7)
    engine.set_sampling_weights(np.ones((2, H * W), np.float32))
    with pytest.raises(capi.DsacError, match="sampling weights are active"):
        engine.sampleRGBD(8)
    engine.set_sampling_weights(None)
    assert engine.sampleRGBD(8)[2].shape == (8,)


# ---- 4. scoring -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def score_refs():
    """float64 distances of every case, computed once"""
    out = {}
    for name, *_ in ref.SCORE_CASES:
        H, W, xyz, cam, poses = ref.score_case(name)
        canon = ref.canonical(xyz, cam)[0]
        F, Nf = xyz.shape[0], len(poses) // xyz.shape[0]
        d = np.concatenate([ref.distances(poses[f * Nf:(f + 1) * Nf], xyz[f], canon[f]) for f in range(F)])
        bound = np.concatenate([ref.score_bound(poses[f * Nf:(f + 1) * Nf], xyz[f], canon[f], ref.err_images(d[f * Nf:(f + 1) * Nf], CLAMP)) for f in range(F)])
        out[name] = (H, W, xyz, cam, poses, d, bound)
    return out


@pytest.mark.parametrize("name", [c[0] for c in ref.SCORE_CASES])
def test_score_against_float64(engine, score_refs, name):
    H, W, xyz, cam, poses, d, bound = score_refs[name]
    N, P = len(poses), H * W
    _set(engine, H, W, xyz, cam)
    e64 = ref.err_images(d, CLAMP)
    s64 = ref.soft_sums(d, CLAMP, TAU, BETA)
    err, soft = np.full((N, P), -1.0, np.float32), np.zeros(N)
    engine.scoreRGBD(poses, err=err, soft=soft, tau=TAU, beta=BETA, clamp=CLAMP)
    fin = np.isfinite(bound)
    assert (err[~fin] == np.float32(CLAMP)).all()  # cells that are not VALID store the clamp
    assert (np.abs(err - e64) <= bound).all()
    margin("rgbd4", "score: worst |err - float64| / [2^-24 (12 (|X|_1 + |t|_1 + |C|_1) + 8 ref)]", float((np.abs(err - e64)[fin] / bound[fin]).max()), 1.0)
    # soft: every sigmoid moves by at most beta / 4 of its error's bound; 16 x 2^-24 of the sum covers the fp32 sigmoid (fma, exp2, add, rcp, mask: 6
    # roundings or 1-ulp approximations) and the fp32 additions below the per-tile partial sums (10 levels: 16 terms in a lane, 16 lanes of a row)
    tol = (BETA / 4 * np.where(fin, bound, 0.0)).sum(1) + 16 * 2.0 ** -24 * s64
    assert (np.abs(soft - s64) <= tol).all()
    margin("rgbd4", "score: worst |soft - float64| / (sum beta / 4 bound + 16 x 2^-24 soft)", float((np.abs(soft - s64) / np.maximum(tol, 1e-300)).max()), 1.0)
    # err only and soft only give the same bits, on a buffer 4 bytes off a 16-byte address too; two calls give the same soft
    big = np.full(N * P + 8, -1.0, np.float32)
    off = (4 - (big.ctypes.data % 16) // 4) % 4 + 1  # the first element 4 bytes past a 16-byte address
    sl = big[off:off + N * P].reshape(N, P)
    assert sl.ctypes.data % 16 == 4
    engine.scoreRGBD(poses, err=sl, tau=TAU, beta=BETA, clamp=CLAMP)
    assert np.array_equal(sl, err) and (big[:off] == -1).all() and (big[off + N * P:] == -1).all()
    soft2 = np.zeros(N)
    engine.scoreRGBD(poses, soft=soft2, tau=TAU, beta=BETA, clamp=CLAMP)
    assert soft2.tobytes() == soft.tobytes()


def test_score_refusals_and_empty_calls(engine):
    H, W = 3, 5
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=80, frames=2, missing_frac=0.3)
    engine.set_frames(xyz, None, H, W)
    poses = np.zeros((4, 6))
    with pytest.raises(capi.DsacError, match="no camera points"):
        engine.scoreRGBD(poses, soft=np.zeros(4))
    engine.set_camera_points(cam)
    with pytest.raises(capi.DsacError, match="frame batch"):
        engine.scoreRGBD(np.zeros((3, 6)), soft=np.zeros(3))
    engine.scoreRGBD(poses)  # neither output: nothing to do
    # the zero pose reads |X - C| back
    err = np.zeros((4, H * W), np.float32)
    engine.scoreRGBD(poses, err=err, clamp=1e9)
    canon = ref.canonical(xyz, cam)[0]
    for f in range(2):
        v = ~np.isnan(canon[f][:, 0])
        want = np.linalg.norm(xyz[f][v].astype(np.float64) - canon[f][v], axis=1)
        assert np.allclose(err[2 * f][v], want, rtol=1e-5) and (err[2 * f][~v] == np.float32(1e9)).all()


# ---- refinement -------------------------------------------------------------------------------------------------------------------------------------
def test_refine_against_the_longdouble_loop(engine):
    H, W, xyz, cam, gt, init = ref.refine_case()
    F, B = xyz.shape[0], len(init)
    per = B // F
    canon = ref.canonical(xyz, cam)[0]
    want = [ref.refine(init[b], xyz[b // per], canon[b // per], TAU, BETA, 100.0, 50.0, 20, 1e-6) for b in range(B)]
    _set(engine, H, W, xyz, cam)
    out, soft, iters, status = engine.refineRGBD(init, tau=TAU, beta=BETA, min_soft=50.0, max_iters=20, step_tol=1e-6)
    out2, soft2, iters2, status2 = engine.refineRGBD(init, tau=TAU, beta=BETA, min_soft=50.0, max_iters=20, step_tol=1e-6)
    assert out.tobytes() == out2.tobytes() and soft.tobytes() == soft2.tobytes() and np.array_equal(iters, iters2) and np.array_equal(status, status2)
    worst_p = worst_s = 0.0
    decided = 0
    for b, (h, S, it, st, mg) in enumerate(want):
        if mg < 1.0:
            continue
        decided += 1
        assert (int(status[b]), int(iters[b])) == (st, it), (b, ref.STATUS[st], capi.SOFT_STATUS[status[b]])
        if st == 5:
            assert _same(out[b], init[b]) and soft[b] == 0
            continue
        worst_p = max(worst_p, float((np.abs(out[b] - h) / np.maximum(1.0, np.abs(h))).max()))
        worst_s = max(worst_s, abs(soft[b] - S) / max(S, 1.0))
    assert decided >= 0.95 * B
    # every step is a fixed function of 16 ordered sums (relative error ~ P x 2^-53 = 2e-13) through an eigenvector whose conditioning is the relative
    # eigenvalue gap (O(1) on these frames) and a product with |X| ~ 3e3 mm; the loop is contractive, so the error does not compound: 1e-9 leaves three decades
    margin("rgbd5", "refine: |pose - longdouble loop| / max(1, |.|) where the loop's decisions are decided", worst_p, 1e-9)
    margin("rgbd5", "refine: |soft - longdouble loop| / max(1, S)", worst_s, 1e-9)
    # explicit frame_of in another order gives each problem the same bits
    order = np.random.default_rng(1).permutation(B)
    o3, s3, i3, st3 = engine.refineRGBD(init[order], frame_of=(order // per).astype(np.int32), tau=TAU, beta=BETA, min_soft=50.0, max_iters=20, step_tol=1e-6)
    assert _same(o3, out[order]) and np.array_equal(st3, status[order]) and np.array_equal(i3, iters[order])


def test_refine_refusals(engine):
    H, W = 40, 40
    xyz, cam, _ = ref.rgbd_frame(H, W, seed=90, frames=2, missing_frac=0.1)
    engine.set_frames(xyz, None, H, W)
    with pytest.raises(capi.DsacError, match="no camera points"):
        engine.refineRGBD(np.zeros((2, 6)))
    engine.set_camera_points(cam)
    for kw, msg in ((dict(cut=0.0), "cut"), (dict(cut=101.0), "cut"), (dict(beta=0.0, cut=50.0), "beta"), (dict(max_iters=0), "max_iters"), (dict(step_tol=-1.0), "step_tol")):
        with pytest.raises(capi.DsacError, match=msg):
            engine.refineRGBD(np.zeros((2, 6)), **kw)
    with pytest.raises(capi.DsacError, match="frame batch"):
        engine.refineRGBD(np.zeros((3, 6)))


# ---- pipelines --------------------------------------------------------------------------------------------------------------------------------------
def test_pipelines_localise_and_agree(engine):
    import torch
    from dsac_amd import synth
    H, W, F, N = 40, 40, 3, 64
    frs = [synth.chess_like_frame_rgbd(H, W, seed=200 + f, noise_mm=5.0, grid_uv=True) for f in range(F)]
    xyz, cam, gt = np.stack([f["xyz"] for f in frs]), np.stack([f["cam_xyz"] for f in frs]), np.stack([f["gt_pose"] for f in frs])
    gt_jp = np.stack([synth.cv_to_jp6(g) for g in gt])
    engine.set_frames(xyz, None, H, W)
    engine.set_camera_points(cam)
    r = engine.processImagesRGBD(N, gt_jp6=gt_jp, seed=1305)
    engine.synchronize()
    ref_b = r["refAvgHyp"].cpu().numpy()
    for f in range(F):
        engine.set_frame(xyz[f], None, H, W)
        engine.set_camera_points(cam[f])
        one = engine.processImageRGBD(N, seed=1305 + f, gt_jp6=gt_jp[f])
        assert abs(one["loss"] - float(r["out4"][f, 0])) <= 1e-12 * max(1.0, abs(one["loss"]))
        assert np.array_equal(one["hyps"], r["hyps"].cpu().numpy()[f * N:(f + 1) * N]) and one["hypIdx"] == int(r["hypIdx"][f])
        assert one["refAvgHyp"].tobytes() == ref_b[f].tobytes() and one["refStatus"] == int(r["refStatus"][f])
        Ra, Rb = ref.rodrigues(ref_b[f][:3]), ref.rodrigues(gt[f][:3])
        ang = np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))
        assert ang <= 5.0 and np.linalg.norm(ref_b[f][3:] - gt[f][3:]) <= 50.0
        soft = engine.processImageRGBD(N, seed=1305 + f, select="softargmax")
        assert np.isfinite(soft["refAvgHyp"]).all()
    assert isinstance(r["scores"], torch.Tensor) and r["scores"].is_cuda
