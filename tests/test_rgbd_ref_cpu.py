"""CPU tests of the RGB-D reference (tests/rgbd_ref.py) and of the corpus the GPU tests use: the reference recovers the ground truth, an fp32 evaluation of
the scoring formulas stays inside the per-pair bound the GPU test asserts while wrong evaluations do not, and the new exports exist."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import rgbd_ref as ref
from dsac_amd import synth

TAU, BETA, CUT = 100.0, 0.05, 100.0


def _localise(xyz, cam, W, H, N, seed, thr=100.0, max_tries=64):
    """the reference alone: walk -> soft scores -> argmax -> refine"""
    v = ref.valid_cells(xyz, cam)
    canon = ref.canonical(xyz[None], cam[None])[0][0]

    def evaluate(cells):
        pose, R, t = ref.kabsch3(xyz, canon, cells)
        return ref.accept3(pose, ref.residuals3(xyz, canon, cells, R, t), thr), pose

    sets = ref.attempt_sets(N, seed, W, H, v, max_tries)
    poses = np.array([ref.walk(s, evaluate)[0] for s in sets])
    soft = ref.soft_sums(ref.distances(poses, xyz, canon), 1000.0, TAU, BETA)
    best = int(np.argmax(soft))
    return ref.refine(poses[best], xyz, canon, TAU, BETA, CUT, 50.0, 20, 1e-9), poses[best]


def _pose_err(a, b):
    Ra, Rb = ref.rodrigues(a[:3]), ref.rodrigues(b[:3])
    ang = np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))
    return ang, np.linalg.norm(a[3:] - b[3:])


def test_reference_recovers_ground_truth_without_noise():
    fr = synth.chess_like_frame_rgbd(40, 40, seed=11, noise_mm=0.0, outlier_frac=0.0, depth_noise_mm=0.0, missing_frac=0.0, grid_uv=True)
    (h, S, it, st, _), _ = _localise(fr["xyz"], fr["cam_xyz"], 40, 40, 16, 5)
    gt = fr["gt_pose"]
    # float32 inputs: a coordinate of a few metres carries 2^-24 x 4e3 mm = 2.4e-4 mm of rounding; over 1 600 cells the pose averages it down
    assert np.abs(h[:3] - gt[:3]).max() <= 1e-6 * max(1.0, np.abs(gt[:3]).max())
    assert np.abs(h[3:] - gt[3:]).max() <= 1e-6 * max(1.0, np.abs(gt[3:]).max())
    assert S > 0.99 * 1600 * 1 / (1 + np.exp(-BETA * TAU))


@pytest.mark.parametrize("seed", range(8))
def test_reference_localises_with_noise_and_outliers(seed):
    fr = synth.chess_like_frame_rgbd(40, 40, seed=100 + seed, noise_mm=5.0, outlier_frac=0.3, depth_noise_mm=5.0, missing_frac=0.1, grid_uv=True)
    (h, S, it, st, _), _ = _localise(fr["xyz"], fr["cam_xyz"], 40, 40, 32, 1305 + seed)
    ang, dt = _pose_err(h, fr["gt_pose"])
    assert ang <= 5.0 and dt <= 50.0, (ang, dt, ref.STATUS[st])


@pytest.mark.parametrize("name", [c[0] for c in ref.SCORE_CASES])
def test_fp32_evaluation_stays_inside_the_pair_bound(name):
    H, W, xyz, cam, poses = ref.score_case(name)
    F = xyz.shape[0]
    Nf = len(poses) // F
    canon = ref.canonical(xyz, cam)[0]
    worst = 0.0
    for f in range(F):
        p = poses[f * Nf:(f + 1) * Nf]
        d = ref.distances(p, xyz[f], canon[f])
        e64 = ref.err_images(d, 1000.0)
        bound = ref.score_bound(p, xyz[f], canon[f], e64)
        e32 = ref.score_fp32(p, xyz[f], canon[f], 1000.0)
        assert (np.abs(e32 - e64) <= bound).all()
        fin = np.isfinite(bound)
        worst = max(worst, float((np.abs(e32 - e64)[fin] / bound[fin]).max()))
    print("fp32 evaluation: worst |err - ref| / bound = %.3f on %s" % (worst, name))


@pytest.mark.parametrize("variant", ["Rt", "not", "swap", "noclamp"])
def test_wrong_evaluations_exceed_the_pair_bound(variant):
    H, W, xyz, cam, poses = ref.score_case("40x40")
    canon = ref.canonical(xyz, cam)[0][0]
    e64 = ref.err_images(ref.distances(poses, xyz[0], canon), 1000.0)
    bound = ref.score_bound(poses, xyz[0], canon, e64)
    e32 = ref.score_fp32(poses, xyz[0], canon, 1000.0, variant=variant)
    assert (np.abs(e32 - e64) > bound).any()


def _score_comparisons_pass(err, soft, e64, s64, bound, clamp=1000.0, beta=BETA):
    """the three comparisons test_score_against_float64 (tests/test_gpu_rgbd.py) makes on the library's err and soft, as one verdict"""
    fin = np.isfinite(bound)
    tol = (beta / 4 * np.where(fin, bound, 0.0)).sum(1) + 16 * 2.0 ** -24 * s64
    return bool((err[~fin] == np.float32(clamp)).all() and (np.abs(err - e64) <= bound).all() and (np.abs(soft - s64) <= tol).all())


@pytest.mark.parametrize("name", ["149x55", "129x64"])
def test_planted_decode_faults_fail_the_score_comparisons(name):
    """Maps with a second group of 32 cell tiles: an err / soft pair that went through a wrong block decode fails the comparisons of the GPU test.  The stand-in for
    the library is the fp32 restatement (which passes), pre-filled with -1 as the GPU test pre-fills err; each fault is planted in a copy of it."""
    H, W, xyz, cam, poses = ref.score_case(name)
    P, F = H * W, xyz.shape[0]
    Nf = len(poses) // F
    T = ref.SCORE_TILE
    canon = ref.canonical(xyz, cam)[0]
    d = np.concatenate([ref.distances(poses[f * Nf:(f + 1) * Nf], xyz[f], canon[f]) for f in range(F)])
    e64 = ref.err_images(d, 1000.0)
    s64 = ref.soft_sums(d, 1000.0, TAU, BETA)
    bound = np.concatenate([ref.score_bound(poses[f * Nf:(f + 1) * Nf], xyz[f], canon[f], e64[f * Nf:(f + 1) * Nf]) for f in range(F)])
    err = np.concatenate([ref.score_fp32(poses[f * Nf:(f + 1) * Nf], xyz[f], canon[f], 1000.0) for f in range(F)])
    valid = ~np.isnan(d)

    def soft_of(e, cells=slice(None)):  # sigmoids of the fp32 errors, summed in float64 over the VALID cells
        return np.where(valid[:, cells], 1.0 / (1.0 + np.exp(-BETA * (TAU - e[:, cells].astype(np.float64)))), 0.0).sum(1)

    soft = soft_of(err)
    assert _score_comparisons_pass(err, soft, e64, s64, bound)
    PT = (P + T - 1) // T
    assert PT > 32 and Nf == 65  # a second tile group, and a ragged hypothesis tile of one row per frame
    last = (PT - 1) * T
    # 1. the last cell tile never written
    bad = err.copy()
    bad[:, last:] = -1.0
    assert not _score_comparisons_pass(bad, soft, e64, s64, bound)
    # 2. the decode without q % PTG: cell tiles 32 and up carry what tiles 0 and up of the same row hold
    bad = err.copy()
    bad[:, 32 * T:] = err[:, :P - 32 * T]
    assert not _score_comparisons_pass(bad, soft, e64, s64, bound)
    # 3. the ragged hypothesis tile (row 64 of every frame) carries the rows of the tile before it (row 0 of the frame)
    bad, bad_soft = err.copy(), soft.copy()
    for f in range(F):
        bad[f * Nf + 64] = err[f * Nf]
        bad_soft[f * Nf + 64] = soft[f * Nf]
    assert not _score_comparisons_pass(bad, soft, e64, s64, bound)
    assert not _score_comparisons_pass(err, bad_soft, e64, s64, bound)
    # 4. soft without the partial sum of the last tile.  On 129x64 that tile holds 64 cells and the reference's sigmoids on it reach 57 x the tolerance of the
    # best hypothesis with this frame seed (at least 2 x is required here); on 149x55 it holds 3 cells, too few to tell
    if name == "129x64":
        fin = np.isfinite(bound)
        tol = (BETA / 4 * np.where(fin, bound, 0.0)).sum(1) + 16 * 2.0 ** -24 * s64
        part = ref.soft_sums(d[:, last:], 1000.0, TAU, BETA)
        print("last tile: worst sum of sigmoids / tolerance = %.1f" % (part / tol).max())
        assert (part / tol).max() >= 2.0
        assert not _score_comparisons_pass(err, soft - soft_of(err, slice(last, None)), e64, s64, bound)


def _undecided(res):
    return float(np.mean([r[4] < 1.0 for r in res]))


def test_refinement_corpus_is_decided():
    """The GPU refinement tests compare statuses and step counts wherever no decision of the reference's loop lies within reach of double-precision rounding
    (rgbd_ref.refine's margin >= 1); at most 5 % of a corpus may be undecided by that rule, on the 40 x 40 corpus and on every corpus and parameter set of
    rgbd_ref.REFINE_CORPORA x REFINE_PARAMS, and together the runs show every status but SINGULAR (tests/test_gpu_rgbd_wild.py has that one)."""
    seen = set()
    for (Hc, Wc) in ref.REFINE_CORPORA:
        _, _, xyz, cam, gt, init = ref.refine_corpus(Hc, Wc)
        for (min_soft, max_iters, step_tol, cut) in ref.REFINE_PARAMS:
            res = ref.refine_reference(xyz, cam, init, TAU, BETA, cut, min_soft, max_iters, step_tol)
            print("%dx%d" % (Wc, Hc), (min_soft, max_iters, step_tol, cut), "undecided", _undecided(res), [(ref.STATUS[r[3]], r[2], "%.1e" % r[4]) for r in res])
            assert _undecided(res) <= 0.05
            assert all(r[2] == max_iters for r in res if r[3] == 1) and all(r[2] < max_iters for r in res if r[3] != 1)
            seen |= {ref.STATUS[r[3]] for r in res}
            if max_iters <= 2 and Hc > 1:  # the near-truth starts of the large maps run out of steps
                assert sum(r[3] == 1 for r in res) == 6
    assert seen >= {"CONVERGED", "MAXIT", "SCORE", "FEW", "NONFINITE"}
    # the two kernels' cross-check (sharper sigmoid on the 129 x 64 map) is decided too
    _, _, xyz, cam, gt, init = ref.refine_corpus(64, 129)
    res = ref.refine_reference(xyz, cam, init, 40.0, 0.5, 100.0, 50.0, 20, 1e-6)
    assert _undecided(res) <= 0.05 and any(r[3] == 0 for r in res)
    H, W, xyz, cam, gt, init = ref.refine_case()
    F = xyz.shape[0]
    canon = ref.canonical(xyz, cam)[0]
    per = len(init) // F
    res = [ref.refine(init[b], xyz[b // per], canon[b // per], TAU, BETA, CUT, 50.0, 20, 1e-6) for b in range(len(init))]
    undecided = np.mean([r[4] < 1.0 for r in res])
    print("undecided", undecided, [(ref.STATUS[r[3]], r[2], "%.1e" % r[4]) for r in res])
    assert undecided <= 0.05
    st = [ref.STATUS[r[3]] for r in res]
    assert "NONFINITE" in st and "FEW" in st and ("CONVERGED" in st or "MAXIT" in st)
    for b, r in enumerate(res):  # a refined pose never scores below its start
        if r[3] in (0, 1, 2):
            ang, dt = _pose_err(r[0], gt[b // per])
            assert ang < 1.0 and dt < 20.0, (b, ang, dt)


def _worst_against(ld, other):
    """worst |pose - long-double pose| / max(1, |.|) and |S - S_ld| / max(1, S) over the decided problems; statuses and step counts must agree there"""
    wp = ws = 0.0
    for a, b in zip(ld, other):
        if a[4] < 1.0:
            continue
        assert (a[3], a[2]) == (b[3], b[2])
        if a[3] != 5:
            wp = max(wp, float((np.abs(b[0] - a[0]) / np.maximum(1.0, np.abs(a[0]))).max()))
            ws = max(ws, abs(b[1] - a[1]) / max(1.0, a[1]))
    return wp, ws


@pytest.mark.parametrize("late", [False, True])
def test_far_origin_needs_the_centred_sums(late):
    """A scene 374 m from its origin (rgbd_ref.far_origin_case): the kernels' 16 sums in plain float64 stay within 1e-10 of the long-double loop when they are
    taken about the first VALID cell, so the GPU test keeps its 1e-9 there; taken about the origin they lose three more digits.
    Measured: centred 1.6e-13 (2.3e-13 with frame 1's first 300 cells not VALID), uncentred 2.6e-10 (2.0e-10)."""
    H, W, xyz, cam, gt, init = ref.far_origin_case(late)
    assert np.abs(xyz[np.isfinite(xyz).all(-1)]).max() > 2.9e5 and np.nanmax(np.abs(cam[np.isfinite(cam).all(-1)])) < 1e4
    ld = ref.refine_reference(xyz, cam, init, TAU, BETA, CUT, 50.0, 20, 1e-6)
    assert _undecided(ld) <= 0.05
    st = [ref.STATUS[r[3]] for r in ld]
    assert st.count("CONVERGED") >= 16 and "FEW" in st and "NONFINITE" in st
    for b, r in enumerate(ld):  # noise-free camera points: every near start converges onto the ground truth of the shifted frame
        if r[3] == 0:
            g = gt[b // (len(init) // 2)]
            assert np.abs(r[0][:3] - g[:3]).max() <= 1e-6 and np.abs(r[0][3:] - g[3:]).max() <= 1.0
    centred = _worst_against(ld, ref.refine_reference(xyz, cam, init, TAU, BETA, CUT, 50.0, 20, 1e-6, loop=ref.refine_f64))
    uncentred = _worst_against(ld, ref.refine_reference(xyz, cam, init, TAU, BETA, CUT, 50.0, 20, 1e-6,
                                                        loop=lambda *a: ref.refine_f64(*a, centred=False)))
    print("far origin%s: float64 against long double, pose / soft: centred %.3e / %.3e, uncentred %.3e / %.3e" % (" (late)" if late else "", *centred, *uncentred))
    assert centred[0] <= 1e-10 and centred[1] <= 1e-10  # the condition under which the GPU tolerance stays 1e-9
    assert uncentred[0] >= 100 * centred[0]


def test_late_first_cell_corpus():
    """rgbd_ref.late_first_case: frame 1's first VALID cell lies beyond the first 256 cells, frame 0's does not, and the reference is decided on it"""
    H, W, xyz, cam, gt, init = ref.late_first_case()
    v = ref.valid_cells(xyz, cam)
    assert int(np.argmax(v[0])) < 256 <= 300 <= int(np.argmax(v[1])) < 512
    ld = ref.refine_reference(xyz, cam, init, TAU, BETA, CUT, 50.0, 20, 1e-6)
    assert _undecided(ld) <= 0.05
    wp, ws = _worst_against(ld, ref.refine_reference(xyz, cam, init, TAU, BETA, CUT, 50.0, 20, 1e-6, loop=ref.refine_f64))
    assert wp <= 1e-10 and ws <= 1e-10


def test_new_exports_are_bound_and_built():
    from dsac_amd import capi
    names = ["dsac_set_camera_points", "dsac_get_camera_points", "dsac_sample_rgbd", "dsac_score_rgbd", "dsac_refine_rgbd"]
    lib = ctypes.CDLL(capi.LIB_PATH)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (dsac_[a-z0-9_]+)", out))
    for n in names:
        assert n in capi.EXPORTS and hasattr(lib, n) and n in exported, n


def test_synthetic_rgbd_frame_is_consistent():
    a = synth.chess_like_frame_rgbd(40, 40, seed=7)
    b = synth.chess_like_frame(40, 40, seed=7)
    assert np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["uv"], b["uv"]) and np.array_equal(a["gt_pose"], b["gt_pose"])
    miss = np.isnan(a["cam_xyz"]).any(1)
    assert 0.05 < miss.mean() < 0.15 and np.array_equal(miss, a["depth"] == 0)
    # the inlier cells align with their measured points under the ground-truth pose: 20 mm of coordinate noise and 5 mm of depth noise
    d = ref.distances(a["gt_pose"][None], a["xyz"], a["cam_xyz"])[0]
    ok = a["inlier_mask"] & ~miss
    assert np.median(d[ok]) < 60 and np.median(d[~a["inlier_mask"] & ~miss]) > 500
    fx, fy, cx, cy = a["cam"]
    back = np.stack([(a["uv"][:, 0] - cx) / fx * a["depth"], (a["uv"][:, 1] - cy) / fy * a["depth"], a["depth"]], -1)
    assert np.allclose(back[~miss], a["cam_xyz"][~miss], rtol=1e-5, atol=1e-2)
