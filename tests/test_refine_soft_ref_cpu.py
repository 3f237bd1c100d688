"""The numpy restatement behind the tests of dsac_refine_soft and dsac_refine_soft_backward (tests/refine_soft_ref.py), checked on the CPU: (a) its analytic
d h / d X against central differences of a pure re-weighted Gauss-Newton solve, (b) the corpus conditions, (c) that the GPU test's bound sees five one-term
mistakes, (d) that no corpus problem ends below the score it started from."""
import numpy as np
import pytest

import refine_soft_ref as sr
from refine_gn_ref import synth


@pytest.fixture(scope="module")
def corpus():
    return sr.corpus()


@pytest.fixture(scope="module")
def expected(corpus):
    return {k: sr.expected(c) for k, c in corpus.items()}


# relative to the largest entry, measured with this restatement: weight derivatives / fixed weights at 0, 5, 20 mm of noise.  What remains is the dropped
# second-order term (the residual-weighted second derivatives of the projection), which grows with the residuals
MEASURED = {0.0: (2.6e-4, 4.0e-4), 5.0: (1.1e-2, 5.7e-2), 20.0: (1.3e-2, 0.65)}


@pytest.mark.parametrize("noise", [0.0, 5.0, 20.0])
def test_gradient_against_central_differences_of_a_pure_irls_solve(noise):
    """40 x 40 frame: the analytic T d h / d X at the fixed point of the re-weighted solve (no accept test, iterated to 1e-15) against central differences
    (+- 0.25 mm) of that fixed point in every coordinate of twelve cells that carry weight.  The weight-derivative form is closer than the fixed-weight form at
    every noise level, and each stays within 2 x of what was measured."""
    fr = synth.chess_like_frame(40, 40, seed=11, noise_mm=noise, outlier_frac=0.3)
    par = (10.0, 0.5, 42.0)
    args = (fr["xyz"].astype(np.float64), fr["uv"], fr["cam"])
    h = sr.irls_solve(fr["gt_pose"] + np.array([0.004, -0.004, 0.002, 3.0, -3.0, 4.0]), *args, *par)
    full = sr.backward(h, *args, *par, 50.0)
    fixed = sr.backward(h, *args, *par, 50.0, fixed=True)
    assert full is not None and fixed is not None and np.array_equal(full["cells"], fixed["cells"])
    w = sr.cell_terms(h, *args, *par)[4][full["cells"]]
    order = np.argsort(-w, kind="stable")[:: max(1, len(w) // 12)][:12]  # twelve cells spread over the weights, the heaviest first
    eps, dev = 0.25, {"full": 0.0, "fixed": 0.0}
    scale = np.abs(full["J"][order]).max()
    for i in order:
        p = int(full["cells"][i])
        fd = np.zeros((6, 3))
        for c in range(3):
            Xp, Xm = args[0].copy(), args[0].copy()
            Xp[p, c] += eps
            Xm[p, c] -= eps
            fd[:, c] = (synth.cv_to_jp6(sr.irls_solve(h, Xp, *args[1:], *par)) - synth.cv_to_jp6(sr.irls_solve(h, Xm, *args[1:], *par))) / (2 * eps)
        dev["full"] = max(dev["full"], np.abs(full["J"][i] - fd).max() / scale)
        dev["fixed"] = max(dev["fixed"], np.abs(fixed["J"][i] - fd).max() / scale)
    print("noise %4.1f mm: analytic against central differences, relative to the largest entry: weight derivatives %.3e, fixed weights %.3e" %
          (noise, dev["full"], dev["fixed"]))
    assert dev["full"] < dev["fixed"]
    assert dev["full"] <= 2 * MEASURED[noise][0] and dev["fixed"] <= 2 * MEASURED[noise][1]


def test_corpus_conditions(corpus, expected):
    """expected() runs the restatement in strict mode: it raises where a decision sits on an edge.  Here: the shapes, the statuses and the bound's ceiling."""
    seen = set()
    for name, case in corpus.items():
        exp = expected[name]
        seen |= set(int(s) for s in exp["status"])
        run = np.isin(exp["status"], (sr.CONVERGED, sr.MAXIT, sr.SCORE))
        assert (exp["cond"][run] <= sr.COND_MAX).all(), name
        assert (exp["iters"] <= case.max_iters).all() and (exp["iters"][exp["status"] == sr.MAXIT] == case.max_iters).all(), name
    assert seen == {sr.CONVERGED, sr.MAXIT, sr.SCORE, sr.FEW, sr.NONFINITE}, [sr.STATUS[s] for s in seen]  # every status except SINGULAR
    assert sr.RHO_ASSERT <= sr.RHO_CEILING and sr.RHO_BWD_ASSERT <= sr.RHO_CEILING and sr.RHO_CEILING * sr.COND_MAX * sr.EPS <= 1e-6
    assert expected["uv40"]["status"][6] == sr.NONFINITE and expected["uv40"]["status"][7] == sr.FEW
    assert corpus["grid37x53"].uv is None and corpus["grid37x53"].P % 2 == 1
    assert {c.max_iters for c in corpus.values()} == {1, 3, 20} and {c.cut for c in corpus.values()} == {25.0, 42.0, 100.0}
    cams = corpus["frames_b6"].cams
    assert len({tuple(c) for c in cams[:, :2].tolist()}) == 3 and (cams[:, 0] != cams[:, 1]).all()
    assert corpus["frames_of"].frame_of.tolist() == [2, 0, 0, 1, 2] and corpus["big"].P == 480 * 640 and corpus["big"].B == 4 and corpus["b1"].B == 1


def test_refined_pose_never_scores_below_its_start(corpus, expected):
    for name, case in corpus.items():
        exp = expected[name]
        for b in range(case.B):
            S0 = sr.score(case.poses[b], *case.frame(b), case.tau, case.beta, case.cut)
            assert exp["S"][b] >= S0, (name, b)
            assert exp["S0"][b] == S0


@pytest.mark.parametrize("variant", sr.WRONG_VARIANTS)
def test_wrong_variants_fail_the_bound(corpus, expected, variant):
    """Every one-term mistake exceeds the GPU test's backward bound on EVERY differentiated problem of the cases below (fx for fy needs fx != fy)."""
    names = ("frames_b6", "frames_of") if variant == "fx_for_fy" else ("b1", "grid37x53", "frames_b6")
    least = np.inf
    for name in names:
        case, exp = corpus[name], expected[name]
        right, wrong = sr.expected_backward(case, exp["h"]), sr.expected_backward(case, exp["h"], variant=variant)
        for b in range(case.B):
            assert right[b] is not None and wrong[b] is not None
            # a mistake in the residual moves a few cells across cut: the comparison is made on the cells both carry
            _, ir, iw = np.intersect1d(right[b]["cells"], wrong[b]["cells"], return_indices=True)
            assert len(ir) >= 0.9 * len(right[b]["cells"])
            least = min(least, sr.jacobian_ratio(wrong[b]["J"][iw], right[b]["J"][ir], right[b]["cond"]))
    print("%s: least ratio to cond 2^-52 max|J_ref| over the problems: %.2e (asserted bound: %.1e)" % (variant, least, sr.RHO_BWD_ASSERT))
    assert least > 100 * sr.RHO_CEILING
