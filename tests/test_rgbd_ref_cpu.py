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


def test_refinement_corpus_is_decided():
    """The GPU refinement test compares statuses and step counts wherever no decision of the reference's loop lies within reach of double-precision rounding
    (rgbd_ref.refine's margin >= 1); at most 5 % of the corpus may be undecided by that rule."""
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
