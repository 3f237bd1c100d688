"""The numpy restatement behind the tests of dsac_refine_gn_backward (tests/refine_gn_ref.py), checked on the CPU against things that do not share its
formulas: central differences of synth.cv_to_jp6 for T, central differences of a converged Gauss-Newton solve for J_obj.  Then the corpus conditions, and that
the GPU test's bound sees five deliberate one-term mistakes."""
import numpy as np
import pytest

import refine_gn_ref as gr
from refine_gn_ref import synth


@pytest.fixture(scope="module")
def corpus():
    return gr.corpus()


@pytest.fixture(scope="module")
def expected(corpus):
    return {k: gr.expected(c) for k, c in corpus.items()}


def test_T_against_central_differences(corpus):
    poses = [c.poses[b] for c in corpus.values() for b in range(min(c.B, 3)) if np.all(np.isfinite(c.poses[b]))]
    poses += [np.array([0.02, -0.03, 0.01, 100.0, -50.0, 2000.0]), np.array([1.1, -0.7, 0.4, -300.0, 20.0, 1500.0])]  # the series branch of J_l(rho); a large angle
    worst = 0.0
    for h in poses:
        T = gr.cv_to_jp6_jacobian(h)
        fd = np.zeros((6, 6))
        for j in range(6):
            e = np.zeros(6)
            e[j] = 1e-6 if j < 3 else 1e-3
            fd[:, j] = (synth.cv_to_jp6(h + e) - synth.cv_to_jp6(h - e)) / (2 * e[j])
        worst = max(worst, np.abs(T - fd).max() / np.abs(fd).max())
    print("T against central differences: worst relative deviation %.2e" % worst)
    assert worst <= 1e-6


def test_J_obj_against_central_differences_of_a_converged_solve():
    """Noise-free 40 x 40 frame, the list of a pose near the ground truth, Gauss-Newton to convergence on that fixed list: the formula at the converged pose
    against central differences (0.5 mm) of the converged pose in every coordinate of twelve cells of the list.  The residuals left are the float32 rounding of
    the coordinates, so the dropped second-order terms are at the differences' own error."""
    fr = synth.chess_like_frame(40, 40, seed=11, noise_mm=0.0, outlier_frac=0.3)
    perm = synth.fast_permutations(1600, 1, seed=7)[0]
    h0 = fr["gt_pose"] + np.array([0.01, -0.01, 0.005, 5.0, -5.0, 8.0])
    L = gr.walk(h0, fr["xyz"], fr["uv"], fr["cam"], perm, 10.0, 100)
    assert len(L) == 100
    X, uv = fr["xyz"][L].astype(np.float64), fr["uv"][L]
    h = gr.gn_solve(h0, X, uv, fr["cam"])
    J, cond = gr.gn_jacobians(h, X, uv, fr["cam"])
    eps, worst = 0.5, 0.0
    for i in range(0, 96, 8):
        fd = np.zeros((6, 3))
        for c in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[i, c] += eps
            Xm[i, c] -= eps
            fd[:, c] = (synth.cv_to_jp6(gr.gn_solve(h, Xp, uv, fr["cam"])) - synth.cv_to_jp6(gr.gn_solve(h, Xm, uv, fr["cam"]))) / (2 * eps)
        worst = max(worst, np.abs(J[i] - fd).max() / np.abs(J).max())
    print("J_obj against central differences of the converged solve: worst relative deviation %.2e, cond(A) %.2e" % (worst, cond))
    assert worst <= 1e-5


def test_corpus_conditions(corpus, expected):
    total = sum(gr.check_corpus_conditions(c, expected[k]) for k, c in corpus.items())
    assert total >= 100
    assert expected["b70"]["n"][5] == 0 and expected["b70"]["n"][9] == 0
    assert (np.delete(expected["b70"]["n"], [5, 9]) == 100).all()
    for mi in gr.MAX_INLS:
        assert (expected["max_inl_%d" % mi]["n"] == mi).all()
    assert ((expected["short"]["n"] >= 50) & (expected["short"]["n"] < 256)).all()  # the walk reaches the end of the row
    sh = expected["shared"]
    assert len(np.intersect1d(sh["cells"][0, :100], sh["cells"][1, :100])) >= 50  # two lists that share cells
    assert len({tuple(c) for c in corpus["frames_b6"].cams[:, :2].tolist()}) == 3 and (corpus["frames_b6"].cams[:, 0] != corpus["frames_b6"].cams[:, 1]).all()


@pytest.mark.parametrize("variant", gr.WRONG_VARIANTS)
def test_wrong_variants_fail_the_bound(corpus, expected, variant):
    """Every one-term mistake exceeds the GPU test's bound on EVERY differentiated problem of the cases below (fx for fy needs fx != fy: the frame batch)."""
    names = ("frames_b6", "frames_of") if variant == "fx_for_fy" else ("b1", "max_inl_64", "max_inl_256", "short", "frames_b6")
    least = np.inf
    for name in names:
        case, exp = corpus[name], expected[name]
        wrong = gr.expected(case, variant)
        assert np.array_equal(wrong["n"], exp["n"])
        for b in range(case.B):
            k = int(exp["n"][b])
            if k:
                least = min(least, gr.jacobian_ratio(wrong["J"][b, :k], exp["J"][b, :k], exp["cond"][b]))
    print("%s: least ratio to cond 2^-52 max|J_ref| over the problems: %.2e (asserted bound: %.1e)" % (variant, least, gr.RHO_ASSERT))
    assert least > gr.RHO_ASSERT
