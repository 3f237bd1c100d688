"""dsac_refine_gn_backward on the GPU (include/dsac_hip.h has the definition) against tests/refine_gn_ref.py, whose formulas tests/test_refine_gn_ref_cpu.py
checks against central differences.  Lists and counts are compared exactly (no corpus residual lies within 1e-3 px of its threshold); Jacobians per problem by
    max |J - J_ref| <= RHO_ASSERT * cond(A_b) * 2^-52 * max |J_ref|,   RHO_ASSERT = 8 x the worst ratio measured on the MI355X (profiles/refine_gn_margins.txt),
at most 1e-6 relative on every corpus problem; gradients per entry by the same bound on the sum of the absolute terms.  40 x 40 and 37 x 53 maps only."""
import os

import numpy as np
import pytest

import refine_gn_ref as gr
from conftest import margin
from dsac_amd import capi, synth
from dsac_amd.capi import lib, ptr

pytestmark = pytest.mark.gpu
INVALID, NO_FRAME = capi.DSAC_ERR_INVALID, capi.DSAC_ERR_NO_FRAME


@pytest.fixture(scope="module")
def corpus():
    return gr.corpus()


@pytest.fixture(scope="module")
def expected(corpus):
    return {k: gr.expected(c) for k, c in corpus.items()}


def _report(line):
    """Figures that are reported, not asserted: printed (run with -s to see them), and appended to $DSAC_GN_REPORT_FILE when that names a file."""
    print(line)
    path = os.environ.get("DSAC_GN_REPORT_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _set(e, case):
    if case.F == 1:
        e.set_frame(case.xyz[0], case.uv, case.H, case.W, tuple(float(c) for c in case.cams[0]))
    else:
        e.set_frames(case.xyz, case.uv, case.H, case.W, cam=case.cams)


def _outputs(case, fill_cells=-7, fill_J=-7.5, fill_n=-7):
    return (np.full((case.B, case.max_inl), fill_cells, np.int32), np.full((case.B, case.max_inl, 6, 3), fill_J), np.full(case.B, fill_n, np.int32))


def _call(e, case, cells=None, J=None, n=None, dL=None, coef=None, grad=None, conv=lambda a: a, sync=False, **over):
    """The raw call on `case` (the frame must be set).  conv: what every array argument goes through (identity: host arrays); sync: wait for the stream before
    the converted arguments go out of scope (with device pointers the call only enqueues).  Returns the status."""
    a = dict(B=case.B, poses=np.ascontiguousarray(case.poses), frame_of=np.ascontiguousarray(case.frame_of) if case.give_frame_of else None,
             perm=np.ascontiguousarray(case.perm), steps=case.perm.shape[0], rows=np.ascontiguousarray(case.rows), max_inl=case.max_inl, min_inl=case.min_inl,
             thr=case.thr)
    a.update(over)
    c = lambda x: None if x is None else conv(x)
    keep = [c(a["poses"]), c(a["frame_of"]), c(a["perm"]), c(a["rows"]), c(dL), c(coef)]
    rc = lib.dsac_refine_gn_backward(e._ctx, int(a["B"]), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), int(a["steps"]), ptr(keep[3]), int(a["max_inl"]),
                                     int(a["min_inl"]), float(a["thr"]), ptr(keep[4]), ptr(keep[5]), ptr(grad), ptr(cells), ptr(J), ptr(n))
    if sync:
        e.synchronize()
    return rc


def _check_jacobians(case, exp, cells, J, n, what):
    """Lists and counts exactly, untouched entries untouched (the -7 / -7.5 fill of _outputs), Jacobians within the bound.  Returns the worst ratio."""
    assert np.array_equal(n, exp["n"]), (case.name, n, exp["n"])
    worst = 0.0
    for b in range(case.B):
        k = int(exp["n"][b])
        assert np.array_equal(cells[b, :k], exp["cells"][b, :k]), (case.name, b)
        assert (cells[b, k:] == -7).all() and (J[b, k:] == -7.5).all(), (case.name, b)
        if k:
            worst = max(worst, gr.jacobian_ratio(J[b, :k], exp["J"][b, :k], exp["cond"][b]))
    margin("gn", "%s: max|J - J_ref| / (cond(A) 2^-52 max|J_ref|), worst problem" % what, worst, gr.RHO_ASSERT)
    return worst


ALL_CASES = ["b70", "b1", "short", "frames_b6", "frames_of"] + ["max_inl_%d" % m for m in gr.MAX_INLS]


@pytest.mark.parametrize("name", ALL_CASES)
def test_lists_and_jacobians(engine, corpus, expected, name):
    """B = 70 with per-problem rows, a NaN pose (5) and a pose with too few inliers (9); B = 1; the short list on the implicit 37 x 53 grid; the 3-frame batch
    with per-frame cameras by the call's own mapping and with frame_of = (2, 0, 0, 1, 2); every max_inl around the 64-lane trips."""
    case, exp = corpus[name], expected[name]
    gr.check_corpus_conditions(case, exp)
    _set(engine, case)
    cells, J, n = _outputs(case)
    assert _call(engine, case, cells, J, n) == 0, lib.dsac_last_error(engine._ctx)
    worst = _check_jacobians(case, exp, cells, J, n, name)
    _report("%-12s B %3d max_inl %3d  worst ratio %.3e  worst cond(A) %.2e  asserted relative bound at that cond %.2e" %
            (name, case.B, case.max_inl, worst, np.nanmax(exp["cond"]), gr.RHO_ASSERT * np.nanmax(exp["cond"]) * gr.EPS))


def _grad_inputs(case, seed):
    rng = np.random.default_rng(seed)
    dL = rng.normal(size=(case.B, 6)) * np.array([100.0, 100.0, 100.0, 1.0, 1.0, 1.0])  # a loss in degrees and centimetres weighs rotations far above millimetres
    coef = rng.uniform(0.1, 1.0, size=case.B)
    grad0 = rng.normal(size=(case.F, case.P, 3))
    return dL, coef, grad0


def _check_grad(case, exp, g, dL, coef, grad0, what):
    ref, tol = gr.expected_grad(case, exp, dL, coef, grad0)
    touched = np.zeros((case.F, case.P), bool)
    for b in range(case.B):
        touched[int(case.frame_of[b]), exp["cells"][b, :int(exp["n"][b])]] = True
    g = g.reshape(case.F, case.P, 3)
    assert np.array_equal(g[~touched], grad0[~touched]), what  # cells outside every list keep their value exactly
    assert touched.any()
    worst = float((np.abs(g - ref)[touched] / tol[touched]).max())
    margin("gn", "%s: |grad - ref| over its bound (RHO_ASSERT cond 2^-52 sum|terms| + 4 x 2^-52 |sum|), worst entry" % what, worst, 1.0)


@pytest.mark.parametrize("name", ["shared", "b70", "frames_of", "short"])
def test_gradient(engine, corpus, expected, name):
    """Accumulation onto non-zero contents, coef, two problems whose lists share cells ("shared"), problems without a result in the batch ("b70"), a frame batch
    with frame_of, the implicit grid; with and without the Jacobians in the same call."""
    case, exp = corpus[name], expected[name]
    _set(engine, case)
    dL, coef, grad0 = _grad_inputs(case, 5)
    if name == "shared":
        assert len(np.intersect1d(exp["cells"][0, :100], exp["cells"][1, :100])) >= 50
    g = grad0.copy()
    assert _call(engine, case, dL=dL, coef=coef, grad=g) == 0, lib.dsac_last_error(engine._ctx)
    _check_grad(case, exp, g, dL, coef, grad0, name + " (gradient alone)")
    g2 = grad0.copy()
    cells, J, n = _outputs(case)
    assert _call(engine, case, cells, J, n, dL=dL, coef=coef, grad=g2) == 0
    _check_grad(case, exp, g2, dL, coef, grad0, name + " (with Jacobians)")
    _check_jacobians(case, exp, cells, J, n, name + " (with gradient)")
    g3 = np.zeros_like(grad0)  # coef NULL = 1
    assert _call(engine, case, dL=dL, grad=g3) == 0
    _check_grad(case, exp, g3, dL, np.ones(case.B), np.zeros_like(grad0), name + " (coef NULL)")


@pytest.mark.parametrize("name", ["b70", "frames_of"])
def test_device_arguments_equal_host_arguments(engine, corpus, expected, name):
    import torch
    case, exp = corpus[name], expected[name]
    _set(engine, case)
    dL, coef, grad0 = _grad_inputs(case, 6)
    cells, J, n = _outputs(case)
    g = grad0.copy()
    assert _call(engine, case, cells, J, n, dL=dL, coef=coef, grad=g) == 0
    dev = lambda a: torch.as_tensor(a, device="cuda:0")
    dc, dJ, dn, dg = (dev(a) for a in _outputs(case) + (grad0.copy(),))
    torch.cuda.synchronize()
    assert _call(engine, case, dc, dJ, dn, dL=dL, coef=coef, grad=dg, conv=dev, sync=True) == 0
    assert np.array_equal(dc.cpu().numpy(), cells) and np.array_equal(dn.cpu().numpy(), n) and np.array_equal(dJ.cpu().numpy(), J)
    # the atomics of two calls arrive in their own order: the sums agree to the roundings of a sum of a few terms
    _, tol = gr.expected_grad(case, exp, dL, coef, grad0, rho=0.0)
    assert (np.abs(dg.cpu().numpy() - g) <= tol).all()


def test_refusals(engine, corpus, expected):
    """Every refusal of the header, DSAC_ERR_INVALID by name, with nothing written."""
    case = corpus["frames_b6"]
    _set(engine, case)
    dL, coef, grad0 = _grad_inputs(case, 7)

    def refused(want_grad=True, want_cells=True, want_J=True, **over):
        cells, J, n = _outputs(case)
        g = grad0.copy()
        kw = dict(dL=dL, coef=coef, grad=g) if want_grad else {}
        kw.update({k: over.pop(k) for k in ("dL", "grad") if k in over})
        rc = _call(engine, case, cells if want_cells else None, J if want_J else None, n, **kw, **over)
        assert (cells == -7).all() and (J == -7.5).all() and (n == -7).all() and np.array_equal(g, grad0), over
        return rc

    assert refused(B=0) == INVALID
    assert refused(max_inl=0) == INVALID and refused(max_inl=257) == INVALID
    assert refused(min_inl=2) == INVALID
    assert refused(steps=0) == INVALID
    assert refused(perm=None) == INVALID and refused(poses=None) == INVALID
    assert refused(dL=None) == INVALID  # grad_xyz without dL
    assert refused(grad=None) == INVALID  # dL without grad_xyz
    assert refused(want_grad=False, want_J=False) == INVALID and refused(want_grad=False, want_cells=False, want_J=False) == INVALID  # nothing requested
    assert refused(want_cells=False) == INVALID  # J_obj without cells
    assert refused(B=5) == INVALID  # 5 problems on 3 frames without frame_of
    assert refused(rows=np.array([0, 1, 2, 0, 1, 0], np.int32)) == INVALID and refused(rows=np.array([0, 1, -1, 0, 1, 0], np.int32)) == INVALID
    assert b"dsac_refine_gn_backward" in lib.dsac_last_error(engine._ctx)
    assert lib.dsac_refine_gn_backward(None, 1, None, None, None, 1, None, 100, 50, 10.0, None, None, None, None, None, None) == INVALID
    import dsac_amd
    with dsac_amd.Engine(0) as fresh:  # a context without a frame
        cells, J, n = _outputs(case)
        assert _call(fresh, case, cells, J, n) == NO_FRAME
        assert (cells == -7).all() and (n == -7).all()
    # the same arguments are accepted once nothing is wrong with them
    cells, J, n = _outputs(case)
    assert _call(engine, case, cells, J, n, dL=dL, coef=coef, grad=grad0.copy()) == 0


def test_engine_entry(engine, corpus, expected):
    """Engine.dRefineGN: defaults, the returned tuple, the gradient allocated when none is given."""
    case, exp = corpus["max_inl_129"], expected["max_inl_129"]
    _set(engine, case)
    dL, coef, _ = _grad_inputs(case, 8)
    g, n, cells, J = engine.dRefineGN(case.poses, case.perm, rows=case.rows, max_inl=129, dL=dL, coef=coef, want_jacobians=True)
    assert g.shape == (case.P, 3) and np.array_equal(n, exp["n"]) and np.array_equal(cells, exp["cells"])
    _check_grad(case, exp, g, dL, coef, np.zeros((1, case.P, 3)), "Engine.dRefineGN")
    g2, n2 = engine.dRefineGN(case.poses, case.perm, rows=case.rows, max_inl=129, dL=dL, coef=coef, grad=g.copy())
    assert np.array_equal(n2, n) and np.allclose(g2, 2 * g, rtol=1e-12, atol=0)
    none, n3, cells3, _ = engine.dRefineGN(case.poses[:1], case.perm, max_inl=129, want_jacobians=True)  # rows default to row 0, which is problem 0's
    assert none is None and n3[0] == 129 and np.array_equal(cells3[0], exp["cells"][0])


def _dsac_forward(engine, fr, N=32):
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    perm = synth.fast_permutations(1600, 8, seed=3)
    gt = synth.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0]))
    # alpha = 0.01: a flat softmax, so that more than a handful of the 32 hypotheses carry weight above min_prob
    return perm, gt, engine.processImageDSAC(N=N, seed=77, perm=perm, gt_jp6=gt, draw_u=0.37, alpha=0.01)


def test_backward_dsac(engine):
    """backwardDSAC(refine_grad="gn") = the numpy composition w x dLossMax x reference J_obj + the unchanged path II; "fd" = the call without the argument, bit
    for bit.  The hypotheses are what K1 sampled and K6 refined on the corpus' 40 x 40 frame: those whose refined pose does not meet the corpus conditions
    (a residual within 1e-3 px of the threshold, cond(A), the jp angle) are given no weight, so that the expected lists are the kernel's by construction."""
    fr = synth.chess_like_frame(40, 40, seed=44, outlier_frac=0.3)
    perm, gt, fwd = _dsac_forward(engine, fr)
    w, ref = fwd["sfScores"].copy(), fwd["refHyps"]
    rows = np.maximum(fwd["refSteps"].astype(np.int64) - 1, 0).astype(np.int32)
    case = gr.Case("dsac", fr["xyz"][None], fr["uv"], 40, 40, [fr["cam"]], perm, ref, rows, np.zeros(len(w), np.int32), False, 100, 50, 10.0)
    exp = gr.expected(case)
    for b in range(case.B):
        good = np.all(np.isfinite(ref[b])) and gr.pose_ok(ref[b], fr["xyz"], fr["uv"], fr["cam"], 10.0)
        if good and exp["n"][b]:
            good = exp["cond"][b] <= gr.COND_MAX and gr.ANGLE_MIN <= gr.jp_angle(ref[b]) <= gr.ANGLE_MAX
        if not good:
            w[b] = 0.0
    sel = np.flatnonzero(w > 1e-4)
    assert len(sel) >= 3 and (exp["n"][sel] > 0).sum() >= 3, "too few hypotheses carry weight for this test to mean anything"
    fwd = dict(fwd, sfScores=w)
    gn = engine.backwardDSAC(fwd, gt, refine_grad="gn")
    dL = gn["dLoss_dRef"]
    g_soft = engine.selectDSAC(w, fwd["losses"])[2]
    path2 = engine.dSoftScore(fwd["hyps"], fwd["sampledPoints"], g_soft * fwd["score_scale"])
    sub = case.with_params("dsac_sel", sel=sel)
    sub_exp = {k: v[sel] for k, v in exp.items()}
    ref_grad, tol = gr.expected_grad(sub, sub_exp, dL[sel], w[sel], path2.reshape(1, 1600, 3))
    # path II is summed again inside backwardDSAC: an entry is at most 4 N + 1 fp64 additions (the main pass, four support points per hypothesis) whose order is
    # the atomics' own, each rounding by at most 2^-52 of a partial sum -- bounded here by the largest entry of path II
    tol = tol + (4 * len(w) + 1) * gr.EPS * np.abs(path2).max()
    worst = float((np.abs(gn["grad"].reshape(1, 1600, 3) - ref_grad) / np.maximum(tol, 1e-300)).max())
    margin("gn", "backwardDSAC(refine_grad=gn): |grad - (path II + w dL J_ref)| over its bound, worst entry (%d hypotheses)" % len(sel), worst, 1.0)
    # "fd" is the call without the argument.  Two identical calls do not return the same bits: path II's fp64 atomics arrive in their own order (the bound
    # above).  With all losses zero the score gradients are exact zeros and path II adds nothing, so what is left -- path I, where the argument acts -- must be
    # equal bit for bit; the whole calls agree to path II's reordering.
    zero = dict(fwd, losses=np.zeros_like(fwd["losses"]))
    a, b = engine.backwardDSAC(zero, gt), engine.backwardDSAC(zero, gt, refine_grad="fd")
    assert np.abs(a["grad"]).max() > 0 and not a["scoreOutputGradients"].any()
    assert np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["dLoss_dRef"], b["dLoss_dRef"])
    a, b = engine.backwardDSAC(fwd, gt), engine.backwardDSAC(fwd, gt, refine_grad="fd")
    assert np.array_equal(a["dLoss_dRef"], b["dLoss_dRef"]) and np.array_equal(a["scoreOutputGradients"], b["scoreOutputGradients"])
    assert np.abs(a["grad"] - b["grad"]).max() <= 2 * (4 * len(w) + 1) * gr.EPS * np.abs(path2).max()
    with pytest.raises(ValueError):
        engine.backwardDSAC(fwd, gt, refine_grad="exact")


def test_report_gn_against_fd_on_a_noise_free_frame(engine):
    """Reported, not asserted: path I by "gn" over path I by "fd" on the entries both touch, noise-free 40 x 40 frame.  The finite differences visit every
    skip-th inlier cell and scale it by skip to stand for the cells they pass over, so the ratio of the two on a visited cell is about 1 / skip."""
    fr = synth.chess_like_frame(40, 40, seed=44, noise_mm=0.0, outlier_frac=0.3)
    perm, gt, fwd = _dsac_forward(engine, fr)
    g_soft = engine.selectDSAC(fwd["sfScores"], fwd["losses"])[2]
    path2 = engine.dSoftScore(fwd["hyps"], fwd["sampledPoints"], g_soft * fwd["score_scale"])
    sub_sample = 0.05
    skip = int(1 / np.float32(sub_sample))
    gn = engine.backwardDSAC(fwd, gt, refine_grad="gn", sub_sample=sub_sample)["grad"] - path2
    fd = engine.backwardDSAC(fwd, gt, refine_grad="fd", sub_sample=sub_sample)["grad"] - path2
    sets = np.unique(fwd["sampledPoints"][fwd["sfScores"] > 1e-4])
    both = (np.abs(gn) > 0).all(1) & (np.abs(fd) > 0).all(1)
    both[sets] = False  # the minimal sets' cells carry the J_set term under "fd" only
    if both.sum():
        ratio = (gn[both] / fd[both]).ravel()
        _report("gn / fd path-I gradient, noise-free 40 x 40, sub_sample %.2f (skip %d), %d cells both touch (minimal-set cells left out): median ratio %.4f "
                "(x skip: %.3f), quartiles %.4f .. %.4f; cells with a gradient: gn %d, fd %d" %
                (sub_sample, skip, int(both.sum()), np.median(ratio), np.median(ratio) * skip, np.percentile(ratio, 25), np.percentile(ratio, 75),
                 int((np.abs(gn) > 0).any(1).sum()), int((np.abs(fd) > 0).any(1).sum())))
    else:
        _report("gn / fd path-I gradient, noise-free 40 x 40: no cell touched by both")
