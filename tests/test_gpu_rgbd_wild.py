"""RGB-D calls on the edge corpus: maps without a VALID cell, rank-deficient correspondences, non-finite poses, one-cell maps."""
import numpy as np
import pytest

import rgbd_ref as ref
from dsac_amd import capi

pytestmark = pytest.mark.gpu
S = capi.SOFT_STATUS


def _frame(H, W, seed=300):
    xyz, cam, gt = ref.rgbd_frame(H, W, seed=seed, dirty=False, missing_frac=0.0, noise_mm=0.0, outlier_frac=0.0, depth_noise_mm=0.0)
    return xyz[0], cam[0], gt[0]


def test_map_without_a_valid_cell(engine):
    H, W = 7, 9
    xyz, cam, gt = _frame(H, W)
    cam[:] = np.nan
    engine.set_frame(xyz, None, H, W)
    engine.set_camera_points(cam)
    assert engine.camera_points()[1][0] == 0
    poses, sets, ok = engine.sampleRGBD(65, max_tries=1 << 20)
    assert not ok.any() and not sets.any() and not poses.any()
    err, soft = np.zeros((3, H * W), np.float32), np.ones(3)
    engine.scoreRGBD(np.stack([gt, np.zeros(6), ref.FAR_POSE]), err=err, soft=soft, clamp=123.0)
    assert (err == 123.0).all() and (soft == 0).all()
    out, s, it, st = engine.refineRGBD(gt, min_soft=0.0)
    assert S[st[0]] == "SINGULAR" and np.array_equal(out[0], gt) and s[0] == 0 and it[0] == 0
    out, s, it, st = engine.refineRGBD(gt, min_soft=1.0)
    assert S[st[0]] == "FEW" and np.array_equal(out[0], gt)


def test_rank_deficient_correspondences_are_singular(engine):
    H, W = 40, 40
    xyz, cam, gt = _frame(H, W)
    R = ref.rodrigues(gt[:3])
    # VALID cells on one line of the scene: the rotation about the line is free
    line = np.float32([100.0, -50.0, 30.0])[None, :] + np.linspace(-800, 800, H * W, dtype=np.float32)[:, None] * np.float32([0.6, 0.0, 0.8])[None, :]
    engine.set_frame(line, None, H, W)
    engine.set_camera_points((line.astype(np.float64) @ R.T + gt[3:]).astype(np.float32))
    out, s, it, st = engine.refineRGBD(gt, min_soft=50.0)
    assert S[st[0]] == "SINGULAR" and np.array_equal(out[0], gt) and s[0] > 50
    # a single VALID cell
    one = np.full((H * W, 3), np.nan, np.float32)
    c = (xyz.astype(np.float64) @ R.T + gt[3:]).astype(np.float32)
    one[77] = c[77]
    engine.set_frame(xyz, None, H, W)
    engine.set_camera_points(one)
    out, s, it, st = engine.refineRGBD(gt, min_soft=0.1)
    assert S[st[0]] == "SINGULAR" and 0.1 <= s[0] <= 1.0
    # three collinear cells as a given set: a non-finite or far-off pose, never accepted at a tight threshold ... and never a crash
    engine.set_frame(line, None, H, W)
    engine.set_camera_points((line.astype(np.float64) @ R.T + gt[3:]).astype(np.float32))
    poses, sets, ok = engine.sampleRGBD(1, sets=np.int32([[0, 800, 1599]]), thr=100.0)
    assert np.isfinite(poses).all() and (ok[0] == 0) == (not poses.any())


def test_non_finite_and_far_poses(engine):
    H, W = 1, 1
    xyz, cam = np.float32([[10.0, 20.0, 30.0]]), np.float32([[11.0, 20.0, 30.0]])
    engine.set_frame(xyz, None, H, W)
    engine.set_camera_points(cam)
    poses = np.zeros((4, 6))
    poses[1, 3] = np.nan
    poses[2, 0] = np.inf
    poses[3, 5] = 1e30
    err, soft = np.zeros((4, 1), np.float32), np.zeros(4)
    engine.scoreRGBD(poses, err=err, soft=soft, clamp=500.0)
    assert err[0, 0] == 1.0 and (err[1:, 0] == 500.0).all() and np.isfinite(soft).all()
    out, s, it, st = engine.refineRGBD(poses[:2], min_soft=0.0)
    assert S[st[1]] == "NONFINITE" and S[st[0]] == "SINGULAR"
    assert engine.sampleRGBD(5, max_tries=4)[2].sum() == 0  # one cell: no attempt can draw three
