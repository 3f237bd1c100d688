"""RGB-D scoring and refinement off the launch plans of the small maps (tests/test_gpu_rgbd.py has those): scoring parameters that overflow the sigmoid's
exponent and an infinite or tiny clamp, device buffers on a map with a second tile group, refinement on chunks above 256 cells, ragged last trips and maps of one
partial trip with every status of the loop, the two kernels against each other, a first VALID cell beyond the first workgroup and a scene far from its origin.
The reference is tests/rgbd_ref.py throughout; every tolerance is the one test_gpu_rgbd.py states for the same quantity."""
import numpy as np
import pytest

import rgbd_ref as ref
from conftest import margin
from dsac_amd import capi

pytestmark = pytest.mark.gpu
TAU, BETA = 100.0, 0.05


def _set(engine, H, W, xyz, cam):
    if xyz.shape[0] == 1:
        engine.set_frame(xyz[0], None, H, W)
    else:
        engine.set_frames(xyz, None, H, W)
    engine.set_camera_points(cam)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _score_ref(name, clamp, tau, beta):
    """float64 distances, clamped errors, pair bounds (inf where the cell is not VALID), soft sums and their tolerance for a case of rgbd_ref.SCORE_CASES"""
    H, W, xyz, cam, poses = ref.score_case(name)
    canon = ref.canonical(xyz, cam)[0]
    F, Nf = xyz.shape[0], len(poses) // xyz.shape[0]
    rows = [slice(f * Nf, (f + 1) * Nf) for f in range(F)]
    d = np.concatenate([ref.distances(poses[r], xyz[f], canon[f]) for f, r in enumerate(rows)])
    e64 = ref.err_images(d, clamp)
    bound = np.concatenate([ref.score_bound(poses[r], xyz[f], canon[f], e64[r]) for f, r in enumerate(rows)])
    with np.errstate(over="ignore"):
        s64 = ref.soft_sums(d, clamp, tau, beta)
    tol = (beta / 4 * np.where(np.isfinite(bound), bound, 0.0)).sum(1) + 16 * 2.0 ** -24 * s64
    return H, W, xyz, cam, poses, d, e64, bound, s64, tol


# ---- scoring parameters ---------------------------------------------------------------------------------------------------------------------------------
def test_score_with_a_sharp_sigmoid_and_an_infinite_clamp(engine):
    tau, beta, clamp = 10.0, 2.0, np.inf
    H, W, xyz, cam, poses, d, e64, bound, s64, tol = _score_ref("53x37", clamp, tau, beta)
    N, P = len(poses), H * W
    _set(engine, H, W, xyz, cam)
    err, soft = np.full((N, P), -1.0, np.float32), np.full(N, -1.0)
    engine.scoreRGBD(poses, err=err, soft=soft, tau=tau, beta=beta, clamp=clamp)
    fin = np.isfinite(bound)
    assert (~fin).any() and np.isposinf(err[~fin]).all()  # cells that are not VALID store the clamp: +inf
    assert np.isfinite(err[fin]).all() and (np.abs(err[fin] - e64[fin]) <= bound[fin]).all()
    margin("rgbd4", "score, clamp +inf: worst |err - float64| / [2^-24 (12 (|X|_1 + |t|_1 + |C|_1) + 8 ref)]", float((np.abs(err[fin] - e64[fin]) / bound[fin]).max()), 1.0)
    assert np.isfinite(soft).all()
    assert (np.abs(soft - s64) <= tol).all()
    margin("rgbd4", "score, tau 10 beta 2: worst |soft - float64| / (sum beta / 4 bound + 16 x 2^-24 soft)", float((np.abs(soft - s64) / np.maximum(tol, 1e-300)).max()), 1.0)
    # beta (e - tau) log2(e) > 128 from e = 54.4 mm on: the exponential is +inf in fp32 and the sigmoid exactly 0.  A hypothesis whose every VALID cell lies beyond
    # 100 mm -- the 50 m pose and the zero pose among them -- scores exactly 0: neither those cells nor the cells that are not VALID (err = +inf, weight 0) add anything
    far = np.where(fin, d, np.inf).min(1) > 100.0
    assert far[-1] and far[-2] and not far.all()
    assert (soft[far] == 0.0).all() and (s64[~far] > 1.0).any() and (soft[s64 > 1.0] > 0.0).all()
    soft2 = np.full(N, -1.0)
    engine.scoreRGBD(poses, soft=soft2, tau=tau, beta=beta, clamp=clamp)
    assert soft2.tobytes() == soft.tobytes()


def test_score_with_a_clamp_below_the_distances(engine):
    clamp = 1.0
    H, W, xyz, cam, poses, d, e64, bound, s64, tol = _score_ref("53x37", clamp, TAU, BETA)
    N, P = len(poses), H * W
    _set(engine, H, W, xyz, cam)
    err, soft = np.full((N, P), -1.0, np.float32), np.full(N, -1.0)
    engine.scoreRGBD(poses, err=err, soft=soft, tau=TAU, beta=BETA, clamp=clamp)
    fin = np.isfinite(bound)
    assert (err[~fin] == np.float32(1.0)).all()
    assert (np.abs(err - e64)[fin] <= bound[fin]).all()
    margin("rgbd4", "score, clamp 1: worst |err - float64| / [2^-24 (12 (|X|_1 + |t|_1 + |C|_1) + 8 ref)]", float((np.abs(err - e64)[fin] / bound[fin]).max()), 1.0)
    # exactly the clamp wherever the float64 distance exceeds it by more than the bound AT THAT DISTANCE (the larger of the two bounds)
    assert xyz.shape[0] == 1
    wide = ref.score_bound(poses, xyz[0], ref.canonical(xyz, cam)[0][0], d)
    beyond = fin & (np.where(fin, d, 0.0) > 1.0 + np.where(fin, wide, 0.0))
    assert beyond[fin].mean() > 0.9 and (err[beyond] == np.float32(1.0)).all()
    assert (err <= np.float32(1.0)).all()
    assert (np.abs(soft - s64) <= tol).all()
    margin("rgbd4", "score, clamp 1: worst |soft - float64| / (sum beta / 4 bound + 16 x 2^-24 soft)", float((np.abs(soft - s64) / np.maximum(tol, 1e-300)).max()), 1.0)


def test_score_into_device_buffers_matches_the_host_call(engine):
    import torch
    H, W, xyz, cam, poses = ref.score_case("149x55")
    N, P = len(poses), H * W
    _set(engine, H, W, xyz, cam)
    err, soft = np.full((N, P), -1.0, np.float32), np.full(N, -1.0)
    engine.scoreRGBD(poses, err=err, soft=soft, tau=TAU, beta=BETA, clamp=1000.0)
    assert (err >= 0).all() and (soft >= 0).all()
    dev = torch.device("cuda", engine.device)
    d_poses = torch.as_tensor(poses, dtype=torch.float64, device=dev).contiguous()
    d_big = torch.full((N * P + 2,), -1.0, dtype=torch.float32, device=dev)
    d_soft = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
    d_err = d_big[1:1 + N * P]
    assert d_err.data_ptr() % 16 == 4 and d_err.is_contiguous()
    torch.cuda.synchronize(dev)  # the engine has a stream of its own: the fills above are done before it reads and writes
    engine.scoreRGBD(d_poses, err=d_err, soft=d_soft, tau=TAU, beta=BETA, clamp=1000.0)
    engine.synchronize()
    big = d_big.cpu().numpy()
    assert big[0] == -1.0 and big[-1] == -1.0
    assert big[1:-1].tobytes() == err.tobytes()
    assert d_soft.cpu().numpy().tobytes() == soft.tobytes()


# ---- refinement -----------------------------------------------------------------------------------------------------------------------------------------
def _check_refine(engine, label, H, W, xyz, cam, init, want, tau, beta, cut, min_soft, max_iters, step_tol):
    """what test_refine_against_the_longdouble_loop asserts: statuses and step counts equal wherever the reference's margin is >= 1, pose and soft within 1e-9
    relative there, two calls bit-identical, a shuffled frame_of gives each problem the same bits.  Returns (poses, soft, iters, status)."""
    F, B = xyz.shape[0], len(init)
    per = B // F
    kw = dict(tau=tau, beta=beta, cut=cut, min_soft=min_soft, max_iters=max_iters, step_tol=step_tol)
    _set(engine, H, W, xyz, cam)
    out, soft, iters, status = engine.refineRGBD(init, **kw)
    out2, soft2, iters2, status2 = engine.refineRGBD(init, **kw)
    assert out.tobytes() == out2.tobytes() and soft.tobytes() == soft2.tobytes() and np.array_equal(iters, iters2) and np.array_equal(status, status2)
    worst_p = worst_s = 0.0
    decided = 0
    for b, (h, S, it, st, mg) in enumerate(want):
        if mg < 1.0:
            continue
        decided += 1
        assert (int(status[b]), int(iters[b])) == (st, it), (label, b, ref.STATUS[st], it, capi.SOFT_STATUS[status[b]], int(iters[b]))
        if st == 5:
            assert _same(out[b], init[b]) and soft[b] == 0
            continue
        worst_p = max(worst_p, float((np.abs(out[b] - h) / np.maximum(1.0, np.abs(h))).max()))
        worst_s = max(worst_s, abs(soft[b] - S) / max(S, 1.0))
    assert decided >= 0.95 * B
    # the reasoning of test_refine_against_the_longdouble_loop; the ordered sums grow to 65 764 terms, P x 2^-53 = 7e-12: still two decades inside 1e-9
    margin("rgbd5", "refine, %s: |pose - longdouble loop| / max(1, |.|), decided problems" % label, worst_p, 1e-9)
    margin("rgbd5", "refine, %s: |soft - longdouble loop| / max(1, S)" % label, worst_s, 1e-9)
    order = np.random.default_rng(1).permutation(B)
    o3, s3, i3, st3 = engine.refineRGBD(init[order], frame_of=(order // per).astype(np.int32), **kw)
    assert _same(o3, out[order]) and s3.tobytes() == soft[order].tobytes() and np.array_equal(st3, status[order]) and np.array_equal(i3, iters[order])
    return out, soft, iters, status


@pytest.mark.parametrize("params", ref.REFINE_PARAMS, ids=lambda p: "soft%g-it%d-tol%g-cut%g" % p)
@pytest.mark.parametrize("HW", ref.REFINE_CORPORA, ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
def test_refine_off_the_256_cell_chunk(engine, HW, params):
    """chunks of 320 cells with a last one of 164 (two full trips and one of 36 lanes), 33 chunks of 256 with a last one of 64, one partial trip of 63 lanes;
    max_iters 20 / 2 / 1, step_tol 1e-6 / 0, cut 100 / 60: every status but SINGULAR, MAXIT on the last of the max_iters + 1 launch pairs"""
    min_soft, max_iters, step_tol, cut = params
    H, W, xyz, cam, gt, init = ref.refine_corpus(*HW)
    want = ref.refine_reference(xyz, cam, init, TAU, BETA, cut, min_soft, max_iters, step_tol, key=(HW, params))
    out, soft, iters, status = _check_refine(engine, "%dx%d" % (W, H), H, W, xyz, cam, init, want, TAU, BETA, cut, min_soft, max_iters, step_tol)
    maxit = np.array([w[3] == 1 and w[4] >= 1.0 for w in want])
    assert ((status == 1) == (iters == max_iters)).all()  # MAXIT, and only MAXIT, has taken max_iters steps
    assert ((status[maxit] == 1) & (iters[maxit] == max_iters)).all()
    if max_iters <= 2 and H > 1:  # the three near-truth starts of each frame run out of steps (tests/test_rgbd_ref_cpu.py holds the reference to that)
        assert maxit.sum() == 6
    if HW == (1, 63) and max_iters <= 2:
        assert maxit.sum() >= 3
    if max_iters == 20 and H > 1:
        assert {"CONVERGED", "SCORE", "FEW", "NONFINITE"} <= {capi.SOFT_STATUS[s] for s in status}


def test_refined_soft_is_the_score_kernels_soft(engine):
    """dsac_refine_rgbd's soft_out against dsac_score_rgbd's soft at the refined poses, sharper sigmoid (tau 40, beta 0.5): the scoring test's tolerance for soft
    plus the weight the refinement's cut removes, at most sigmoid(beta (tau - cut)) = 9e-14 per cell"""
    tau, beta, cut = 40.0, 0.5, 100.0
    H, W, xyz, cam, gt, init = ref.refine_corpus(64, 129)
    P = H * W
    want = ref.refine_reference(xyz, cam, init, tau, beta, cut, 50.0, 20, 1e-6, key=("cross", 64, 129))
    out, soft, iters, status = _check_refine(engine, "129x64, tau 40 beta 0.5", H, W, xyz, cam, init, want, tau, beta, cut, 50.0, 20, 1e-6)
    assert (status == 0).any() and iters.max() >= 6
    score = np.full(len(out), -1.0)
    engine.scoreRGBD(out, soft=score, tau=tau, beta=beta, clamp=1000.0)
    assert np.isfinite(score).all()
    canon = ref.canonical(xyz, cam)[0]
    per = len(out) // xyz.shape[0]
    worst = 0.0
    for b in range(len(out)):
        if status[b] == 5:  # a non-finite start pose comes back as it went in: every error is the clamp
            assert soft[b] == 0 and score[b] <= P / (1.0 + np.exp(-beta * (tau - 1000.0)))
            continue
        f = b // per
        d = ref.distances(out[b:b + 1], xyz[f], canon[f])
        bound = ref.score_bound(out[b:b + 1], xyz[f], canon[f], ref.err_images(d, 1000.0))
        with np.errstate(over="ignore"):
            s64 = ref.soft_sums(d, 1000.0, tau, beta)[0]
        tol = (beta / 4 * np.where(np.isfinite(bound), bound, 0.0)).sum() + 16 * 2.0 ** -24 * s64 + P / (1.0 + np.exp(-beta * (tau - cut)))
        assert abs(score[b] - soft[b]) <= tol, (b, score[b], soft[b], tol)
        worst = max(worst, abs(score[b] - soft[b]) / tol)
    margin("rgbd5", "|refine soft_out - score soft| at the refined poses / (score's soft tolerance + P sigmoid(beta (tau - cut)))", worst, 1.0)


# ---- the first VALID cell and a far scene origin ----------------------------------------------------------------------------------------------------------
def test_first_valid_cell_in_the_second_workgroup(engine):
    H, W, xyz, cam, gt, init = ref.late_first_case()
    want_canon, n = ref.canonical(xyz, cam)
    first = [int(np.argmax(~np.isnan(want_canon[f][:, 0]))) for f in range(2)]
    assert first[0] < 256 <= first[1] < 512
    _set(engine, H, W, xyz, cam)
    got, n_got = engine.camera_points()
    assert _same(got, want_canon) and np.array_equal(n_got, n) and n[0] - n[1] > 200
    want = ref.refine_reference(xyz, cam, init, TAU, BETA, 100.0, 50.0, 20, 1e-6, key="late")
    _check_refine(engine, "first VALID cell 300+", H, W, xyz, cam, init, want, TAU, BETA, 100.0, 50.0, 20, 1e-6)


@pytest.mark.parametrize("late", [False, True], ids=["first-cell-early", "first-cell-late"])
def test_refine_on_a_scene_far_from_its_origin(engine, late):
    """The scene 374 m from its origin, the camera points near the camera: the 16 sums are taken about the first VALID cell, so the tolerance is the 1e-9 of every
    refinement test -- in plain float64 the centred sums stay within 2.3e-13 of the long-double loop on this corpus and the uncentred ones within 2.6e-10
    (tests/test_rgbd_ref_cpu.py::test_far_origin_needs_the_centred_sums).  late: frame 1's first VALID cell comes from the second workgroup's minimum."""
    H, W, xyz, cam, gt, init = ref.far_origin_case(late)
    want = ref.refine_reference(xyz, cam, init, TAU, BETA, 100.0, 50.0, 20, 1e-6, key=("far", late))
    out, soft, iters, status = _check_refine(engine, "origin 374 m away", H, W, xyz, cam, init, want, TAU, BETA, 100.0, 50.0, 20, 1e-6)
    assert (status == 0).sum() >= 16
