"""Pins tests/k4_ref.py -- the reference, the corpus and the metric of tests/test_gpu_k4_cells.py -- without a GPU:
  * k4_reference equals the oracle (orc.dScore, orc.dProjectdObj, orc.dProjectdHyp);
  * a correct fp32 kernel (k4_fp32_model) passes the per-cell bound and the pose-sum bounds on every corpus case;
  * mask_pairs removes at most 2 % of the pairs of every case;
  * six wrong kernels fail the per-cell bound, two of them where the older metric (largest error over largest entry <= 1e-3) sees nothing.

Cells that lose all their hypotheses.  Every pose of a case lies within 0.03 rad / 40 mm of the frame's ground truth, so a scene point within 200 mm of the
camera plane (one of the outliers that synth.chess_like_frame scatters through the volume) is that near under ALL poses: the depth rule masks the cell in
every hypothesis, whatever the seed -- about 0.1 % of the cells of a map, 42 of 33 600 on the largest.  Such a cell has scale == 0 and the GPU test holds it
to an exact 0.0, a stricter check than the bound.  The clamp-edge band must not take a cell out on its own, and such cells stay under the 2 % cap as well."""
import functools

import numpy as np
import pytest

import k4_ref as kr


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(orc):
    return orc


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------------------
def _p3p_case(orc, fr, N, seed):
    H, W = fr["H"], fr["W"]
    _, sets, ok, _ = orc.sample(N, seed, fr["xyz"], fr["uv"], H, W, fr["cam"])
    assert ok.all()
    poses = np.stack([orc.solve_p3p(fr["xyz"][s], fr["uv"][s], fr["cam"])[1] for s in sets])
    rng = np.random.default_rng(seed)
    dDiff = rng.normal(size=(N, H * W))
    # a hypothesis' own cells: the residual is round-off, its direction differs between any two implementations (the EPS guard of cnn_softam.h:430,490)
    dDiff[np.arange(N)[:, None], sets] = 0
    return poses, sets, dDiff


@pytest.mark.parametrize("H,W,N,seed", [(40, 40, 24, 5), (38, 42, 8, 6)])
def test_reference_equals_the_oracles_dscore(orc, synth, frame40, H, W, N, seed):
    fr = frame40 if (H, W) == (40, 40) else synth.chess_like_frame(H, W, seed=21)
    poses, sets, dDiff = _p3p_case(orc, fr, N, seed)
    outside = np.ones(H * W, bool)
    outside[sets.reshape(-1)] = False
    for tr in ((False, True) if H == W else (False,)):
        ref = kr.k4_reference(poses, fr["xyz"], fr["uv"], fr["cam"], d_err=dDiff, transpose=tr)
        grad_o, G6_o, _ = orc.dScore(sets, dDiff, fr["xyz"], fr["uv"], H, W, fr["cam"], quirk_transpose=tr)
        assert np.abs(ref["G6"] - G6_o).max() <= 1e-10 * np.abs(G6_o).max()
        cells = kr.transpose_cells(outside, W) if tr else outside  # the support term lands on the sets' cells (K5 and the scatter have their own tests)
        assert np.abs(ref["grad"] - grad_o)[cells].max() <= 1e-10 * np.abs(grad_o).max()
        assert (ref["scale"] + 1e-300 >= np.abs(ref["grad"]).max(1)).all()


def test_reference_equals_the_oracles_pair_functions(orc, frame40):
    fr = frame40
    poses, sets, _ = _p3p_case(orc, fr, 24, 5)
    geo = kr.k4_geometry(poses, fr["xyz"], fr["uv"], fr["cam"])
    rng = np.random.default_rng(9)
    n = 0
    while n < 50:
        h, p = int(rng.integers(24)), int(rng.integers(1600))
        if p in sets[h]:
            continue
        n += 1
        R, t = orc.cv2our(poses[h])
        J3 = orc.dProjectdObj(fr["uv"][p], fr["xyz"][p], R, t, fr["cam"])
        J6 = orc.dProjectdHyp(fr["uv"][p], fr["xyz"][p], R, t, fr["cam"])
        C = geo["C"][h, p]
        mine6 = np.concatenate([geo["dRdH"][h] @ np.outer(C, geo["X"][p]).reshape(9), C])
        assert np.abs(geo["J3"][h, p] - J3).max() <= 1e-12 * max(1.0, np.abs(J3).max())
        assert np.abs(mine6 - J6).max() <= 1e-12 * max(1.0, np.abs(J6).max())


def test_guards_of_the_reference(orc):
    """|Ez| < 1e-8 and err > 100 give zero rows, as in the oracle's functions"""
    cam = (525.0, 525.0, 320.0, 240.0)
    pose = np.zeros((1, 6))
    R, t = orc.cv2our(pose[0])
    X = np.array([[0.0, 0.0, 0.0], [5000.0, 0.0, -1000.0 * R[2, 2]], [10.0, 20.0, -1000.0 * R[2, 2]]], np.float32)
    uv = np.array([[300.0, 200.0]] * 3, np.float32)
    geo = kr.k4_geometry(pose, X, uv, cam)
    for p in range(3):
        assert np.allclose(geo["J3"][0, p], orc.dProjectdObj(uv[p], X[p], R, t, cam), rtol=1e-12, atol=0)
    assert not geo["J3"][0, 0].any() and not geo["J3"][0, 1].any() and geo["J3"][0, 2].any()
    assert np.isinf(geo["err"][0, 0]) and geo["err"][0, 1] > 100.0


# ---- a correct fp32 kernel passes; the cap ----------------------------------------------------------------------------------------------------
INPUTS = ("flat", "heavy", "soft")


@functools.lru_cache(maxsize=None)
def _model(idx, name):
    b = kr.build_case(idx)
    ms = [kr.k4_fp32_model(p["poses"], p["fr"]["xyz"], p["fr"]["uv"], p["fr"]["cam"], d_err=None if name == "soft" else p["d_err"][name],
                           g=p["g"] if name == "soft" else None, transpose=b["transpose"]) for p in b["parts"]]
    return np.concatenate([m["grad"] for m in ms]), np.concatenate([m["G6"] for m in ms])


def _case_index(family, **match):
    for i, c in enumerate(kr.CORPUS):
        if c["family"] == family and all(c.get(k, c["opt"].get(k)) == v for k, v in match.items()):
            return i
    raise KeyError((family, match))


@pytest.mark.parametrize("idx", range(len(kr.CORPUS)), ids=[kr.case_id(c) for c in kr.CORPUS])
def test_a_correct_fp32_kernel_passes(idx):
    b = kr.build_case(idx)
    for name in INPUTS:
        grad, G6 = _model(idx, name)
        ref = b["refs"][name]
        cell = kr.cell_ratio(grad, ref, b["clean_cells"] if name == "soft" else None)
        pr = kr.pose_ratios(G6, ref["G6"])
        print("%s %s: per-cell %.2e, pose sums median %.2e max %.2e" % (kr.case_id(b["case"]), name, cell, np.median(pr), pr.max()))
        assert np.isfinite(grad).all()
        assert cell <= kr.CELL_TOL, (name, cell)
        assert np.median(pr) <= kr.POSE_MEDIAN and pr.max() <= kr.POSE_MAX, (name, np.median(pr), pr.max())
        if name != "soft":
            assert not grad[ref["scale"] == 0].any()


@pytest.mark.parametrize("idx", range(len(kr.CORPUS)), ids=[kr.case_id(c) for c in kr.CORPUS])
def test_the_mask_stays_under_its_cap(idx):
    b = kr.build_case(idx)
    for p in b["parts"]:
        m = p["masked"]
        assert m.mean() <= kr.MASK_CAP, m.mean()
        lost = m.all(0)
        # see the module docstring: only the depth rule, which follows the frame and not the hypothesis, takes whole cells; never the clamp-edge band
        near_in_all = (np.abs(p["geo"]["Ez"]) < 200.0).all(0)
        assert not (lost & ~near_in_all).any()
        assert lost.mean() <= kr.MASK_CAP, lost.mean()
        for name in ("flat", "heavy"):
            assert not p["d_err"][name][m].any() and p["d_err"][name].dtype == np.float32


# ---- wrong kernels fail -----------------------------------------------------------------------------------------------------------------------
def _run(b, d_err=None, g=None, poses=None, **kw):
    p = b["parts"][0]
    return kr.k4_fp32_model(p["poses"] if poses is None else poses, p["fr"]["xyz"], p["fr"]["uv"], p["fr"]["cam"], d_err=d_err, g=g, **kw)["grad"]


def test_mutation_1_a_clamped_load_used_as_data():
    """the last 4 valid cells take d_err of the 4 cells before them; heavy-tailed input: the per-cell bound fires, the global metric does not"""
    b = kr.build_case(_case_index("chunk tail"))
    d = b["parts"][0]["d_err"]["heavy"].copy()
    P = b["P"]
    d[:, P - 4:] = d[:, P - 8:P - 4]
    grad = _run(b, d_err=d)
    ref = b["refs"]["heavy"]
    assert kr.cell_ratio(grad, ref) > kr.CELL_TOL
    assert kr.global_ratio(grad, ref) <= 1e-3


def test_mutation_2_last_hypothesis_of_a_ragged_tile_counted_twice():
    b = kr.build_case(_case_index("hypothesis edges", N=17))
    p = b["parts"][0]
    d = np.concatenate([p["d_err"]["flat"], p["d_err"]["flat"][-1:]])
    grad = _run(b, d_err=d, poses=np.concatenate([p["poses"], p["poses"][-1:]]))
    assert kr.cell_ratio(grad, b["refs"]["flat"]) > kr.CELL_TOL


def test_mutation_3_a_hypothesis_group_of_one_tile_dropped():
    """form 1 (CH = 2): hypotheses 16 .. 31 contribute nothing to the 128 cells of pixel tile 131"""
    b = kr.build_case(_case_index("split tiles, direct"))
    d = b["parts"][0]["d_err"]["flat"].copy()
    d[16:32, 131 * 128:132 * 128] = 0
    assert kr.cell_ratio(_run(b, d_err=d), b["refs"]["flat"]) > kr.CELL_TOL


def test_mutation_4_no_weight_between_50_and_100_px_in_the_soft_mode():
    """the fused sigmoid's weight at 50 px is exp(-20) of its largest: the global metric cannot see those cells at all"""
    b = kr.build_case(_case_index("chunk tail"))
    p = b["parts"][0]
    err = p["geo"]["err"]
    w = kr.soft_weights(p["g"], err)
    w[(err > 50.0) & (err < 100.0)] = 0
    grad = _run(b, d_err=w.astype(np.float32))
    ref = b["refs"]["soft"]
    assert kr.cell_ratio(grad, ref, b["clean_cells"]) > kr.CELL_TOL
    assert kr.global_ratio(grad, ref) <= 1e-3
    # the unmutated weights through the same path pass: the mutation is what fires
    assert kr.cell_ratio(_run(b, d_err=kr.soft_weights(p["g"], err).astype(np.float32)), ref, b["clean_cells"]) <= kr.CELL_TOL


def test_mutation_5_keep_taken_at_90_px():
    b = kr.build_case(_case_index("implicit tail"))
    grad = _run(b, d_err=b["parts"][0]["d_err"]["flat"], clamp=90.0)
    assert kr.cell_ratio(grad, b["refs"]["flat"]) > kr.CELL_TOL


def test_mutation_6_rows_x_and_y_of_one_chunk_swapped():
    b = kr.build_case(_case_index("one tile + 4", W=33))
    grad = _model(_case_index("one tile + 4", W=33), "flat")[0].copy()
    grad[16:32] = grad[16:32][:, [1, 0, 2]]
    assert kr.cell_ratio(grad, b["refs"]["flat"]) > kr.CELL_TOL


def test_bf16_rounding_helper():
    a = np.array([1.0, 1.00390625, 1.01171875, -3.1415927, 1e-3, 0.0], np.float32)
    w = kr.bf16_widen(kr.bf16_bits(a))
    assert np.array_equal(w, np.array([1.0, 1.0, 1.015625, -3.140625, w[4], 0.0], np.float32)) and abs(w[4] - 1e-3) <= 1e-3 * 2.0 ** -8
