"""dsac_refine_soft and dsac_refine_soft_backward on the GPU (include/dsac_hip.h has the definitions) against tests/refine_soft_ref.py, whose formulas
tests/test_refine_soft_ref_cpu.py checks against central differences.  Statuses and step counts are compared exactly (the corpus keeps every decision off its
edge); poses, scores and Jacobians by rho x cond x 2^-52 bounds with rho = 8 x the worst ratio measured on the MI355X (profiles/refine_soft_margins.txt), at
most 1e-6 relative.  Both forms of the forward loop are forced in turn on every case except 480 x 640, which runs the split form only."""
import os

import numpy as np
import pytest

import refine_soft_ref as sr
from conftest import margin
from dsac_amd import capi, synth
from dsac_amd.capi import lib, ptr

pytestmark = pytest.mark.gpu
INVALID, NO_FRAME = capi.DSAC_ERR_INVALID, capi.DSAC_ERR_NO_FRAME
FORM_NAME = {0: "split", 1: "fused"}


@pytest.fixture(scope="module")
def corpus():
    return sr.corpus()


@pytest.fixture(scope="module")
def expected(corpus):
    return {k: sr.expected(c) for k, c in corpus.items()}


@pytest.fixture(scope="module")
def expected_bwd(corpus, expected):
    """The restated backward at the restated refined poses, with and without the weight derivatives, for the small cases."""
    return {k: {fixed: sr.expected_backward(corpus[k], expected[k]["h"], fixed=fixed) for fixed in (False, True)} for k in sr.SMALL_CASES}


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_option("refine_soft_form", -1)


def _report(line):
    """Figures that are reported next to what is asserted: printed, and appended to $DSAC_SOFT_REPORT_FILE when that names a file."""
    print(line)
    path = os.environ.get("DSAC_SOFT_REPORT_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _set(e, case, only=None):
    """The case's frames, or frame `only` alone through dsac_set_frame with that frame's camera."""
    if only is not None:
        e.set_frame(case.xyz[only], case.uv, case.H, case.W, tuple(float(c) for c in case.cams[only]))
    elif case.F == 1:
        e.set_frame(case.xyz[0], case.uv, case.H, case.W, tuple(float(c) for c in case.cams[0]))
    else:
        e.set_frames(case.xyz, case.uv, case.H, case.W, cam=case.cams)


def _fwd_outputs(B):
    return np.full((B, 6), -7.5), np.full(B, -7.5), np.full(B, -7, np.int32), np.full(B, -7, np.int32)


def _fwd(e, case, outs=None, conv=lambda a: a, sync=False, **over):
    """The raw forward call (the frame must be set).  Returns (rc, out_poses, soft, iters, status)."""
    a = dict(B=case.B, poses=np.ascontiguousarray(case.poses), frame_of=np.ascontiguousarray(case.frame_of) if case.give_frame_of else None, tau=case.tau,
             beta=case.beta, cut=case.cut, min_soft=case.min_soft, max_iters=case.max_iters, step_tol=case.step_tol)
    a.update(over)
    outs = _fwd_outputs(int(max(a["B"], 1))) if outs is None else outs
    keep = [None if x is None else conv(x) for x in (a["poses"], a["frame_of"])]
    rc = lib.dsac_refine_soft(e._ctx, int(a["B"]), ptr(keep[0]), ptr(keep[1]), float(a["tau"]), float(a["beta"]), float(a["cut"]), float(a["min_soft"]),
                              int(a["max_iters"]), float(a["step_tol"]), *[ptr(o) for o in outs])
    if sync:
        e.synchronize()
    return (rc,) + tuple(outs)


def _bwd(e, case, ref, dL, coef, grad, ok=None, flags=0, conv=lambda a: a, sync=False, **over):
    a = dict(B=case.B, poses=np.ascontiguousarray(ref), frame_of=np.ascontiguousarray(case.frame_of) if case.give_frame_of else None, tau=case.tau, beta=case.beta,
             cut=case.cut, min_soft=case.min_soft, dL=dL, coef=coef, grad=grad)
    a.update(over)
    keep = [None if x is None else conv(x) for x in (a["poses"], a["frame_of"], a["dL"], a["coef"])]
    rc = lib.dsac_refine_soft_backward(e._ctx, int(a["B"]), ptr(keep[0]), ptr(keep[1]), float(a["tau"]), float(a["beta"]), float(a["cut"]), float(a["min_soft"]),
                                       ptr(keep[2]), ptr(keep[3]), int(flags), ptr(a["grad"]), ptr(ok))
    if sync:
        e.synchronize()
    return rc


CASE_FORMS = [(n, f) for n in sr.SMALL_CASES for f in (0, 1)] + [("big", 0)]


@pytest.mark.parametrize("name,form", CASE_FORMS, ids=["%s-%s" % (n, FORM_NAME[f]) for n, f in CASE_FORMS])
def test_forward(eng, corpus, expected, name, form):
    """Decisions (status, accepted steps) equal to the restatement's; poses and scores within the bound; S(out) >= S(h0) with S(h0) by numpy."""
    case, exp = corpus[name], expected[name]
    _set(eng, case)
    eng.set_option("refine_soft_form", form)
    rc, h, S, it, status = _fwd(eng, case)
    assert rc == 0, lib.dsac_last_error(eng._ctx)
    assert np.array_equal(status, exp["status"]), (name, [sr.STATUS[s] for s in status], [sr.STATUS[s] for s in exp["status"]])
    assert np.array_equal(it, exp["iters"]), (name, it, exp["iters"])
    worst_h = worst_S = 0.0
    for b in range(case.B):
        if exp["status"][b] == sr.NONFINITE:
            assert np.array_equal(h[b], case.poses[b], equal_nan=True) and S[b] == 0 and it[b] == 0
            continue
        # never below the start pose's score, both by numpy: the pose is the start pose itself, or one whose score the corpus keeps 1e-10 S above it
        assert sr.score(h[b], *case.frame(b), case.tau, case.beta, case.cut) >= exp["S0"][b], (name, b)
        if exp["status"][b] == sr.FEW:
            assert np.array_equal(h[b], case.poses[b]) and abs(S[b] - exp["S"][b]) <= 64 * sr.EPS * max(exp["S"][b], 1.0)
            continue
        rh, rS = sr.forward_ratios(h[b], S[b], exp, b)
        worst_h, worst_S = max(worst_h, rh), max(worst_S, rS)
    _report("forward  %-16s %-5s B %d  worst |h - h_ref| ratio %.3e  worst |S - S_ref| ratio %.3e  worst cond(A) %.2e" %
            (name, FORM_NAME[form], case.B, worst_h, worst_S, np.nanmax(exp["cond"])))
    margin("soft", "%s %s: |h - h_ref|inf / (cond(A) 2^-52 max(1, |h_ref|inf)), worst problem" % (name, FORM_NAME[form]), worst_h, sr.RHO_ASSERT)
    margin("soft", "%s %s: |S - S_ref| / (cond(A) 2^-52 S_ref), worst problem" % (name, FORM_NAME[form]), worst_S, sr.RHO_ASSERT)


def _grad_inputs(case, seed):
    rng = np.random.default_rng(seed)
    dL = rng.normal(size=(case.B, 6)) * np.array([100.0, 100.0, 100.0, 1.0, 1.0, 1.0])
    return dL, rng.uniform(0.1, 1.0, size=case.B), rng.normal(size=(case.F, case.P, 3))


@pytest.mark.parametrize("fixed", [False, True], ids=["weight-derivatives", "fixed-weights"])
@pytest.mark.parametrize("name", sr.SMALL_CASES)
def test_backward_gradient(eng, corpus, expected, expected_bwd, name, fixed):
    """Random dL and coef, a non-zero grad_xyz to accumulate into: within the per-term bound; cells of weight zero keep their bits; problems without a result
    (the NaN pose and the far pose of uv40) leave everything untouched and report ok = 0."""
    case, bwd = corpus[name], expected_bwd[name][fixed]
    ref = expected[name]["h"]
    _set(eng, case)
    dL, coef, grad0 = _grad_inputs(case, 5)
    g, ok = grad0.copy(), np.full(case.B, -7, np.int32)
    assert _bwd(eng, case, ref, dL, coef, g, ok, flags=1 if fixed else 0) == 0, lib.dsac_last_error(eng._ctx)
    assert np.array_equal(ok, [0 if r is None else 1 for r in bwd]), (name, ok)
    want, tol, touched = sr.expected_grad(case, bwd, dL, coef, grad0)
    assert np.array_equal(g[~touched], grad0[~touched]) and touched.any() and not touched.all()
    worst = float((np.abs(g - want)[touched] / tol[touched]).max())
    margin("soft", "%s %s: |grad - ref| over its bound, worst entry" % (name, "fixed weights" if fixed else "weight derivatives"), worst, 1.0)
    g3 = np.zeros_like(grad0)  # coef NULL = 1, ok NULL
    assert _bwd(eng, case, ref, dL, None, g3, None, flags=1 if fixed else 0) == 0
    want, tol, touched = sr.expected_grad(case, bwd, dL, np.ones(case.B), np.zeros_like(grad0))
    assert float((np.abs(g3 - want)[touched] / tol[touched]).max()) <= 1.0 and not g3[~touched].any()


@pytest.mark.parametrize("fixed", [False, True], ids=["weight-derivatives", "fixed-weights"])
@pytest.mark.parametrize("name", ["b1", "grid37x53", "frames_of"])
def test_backward_unit_dL_recover_the_jacobians(eng, corpus, expected, expected_bwd, name, fixed):
    case, bwd = corpus[name], expected_bwd[name][fixed]
    _set(eng, case)
    J = [np.zeros((len(r["cells"]), 6, 3)) for r in bwd]
    for k in range(6):
        dL = np.zeros((case.B, 6))
        dL[:, k] = 1.0
        g = np.zeros((case.F, case.P, 3))
        assert _bwd(eng, case, expected[name]["h"], dL, None, g, flags=1 if fixed else 0) == 0
        if len(set(case.frame_of.tolist())) == case.B:  # one problem per frame: the cell sums are single terms
            for b in range(case.B):
                J[b][:, k] = g[int(case.frame_of[b])][bwd[b]["cells"]]
    if len(set(case.frame_of.tolist())) != case.B:  # problems share frames: one problem at a time through coef
        for b in range(case.B):
            for k in range(6):
                dL, coef = np.zeros((case.B, 6)), np.zeros(case.B)
                dL[b, k], coef[b] = 1.0, 1.0
                g = np.zeros((case.F, case.P, 3))
                assert _bwd(eng, case, expected[name]["h"], dL, coef, g, flags=1 if fixed else 0) == 0
                J[b][:, k] = g[int(case.frame_of[b])][bwd[b]["cells"]]
    worst = max(sr.jacobian_ratio(J[b], bwd[b]["J"], bwd[b]["cond"]) for b in range(case.B))
    _report("backward %-16s %-18s worst max|J - J_ref| / (cond(H) 2^-52 max|J_ref|) %.3e  worst cond(H) %.2e" %
            (name, "fixed weights" if fixed else "weight derivatives", worst, max(r["cond"] for r in bwd)))
    margin("soft", "%s %s: max|J - J_ref| / (cond(H) 2^-52 max|J_ref|), worst problem" % (name, "fixed weights" if fixed else "weight derivatives"), worst,
           sr.RHO_BWD_ASSERT)


@pytest.mark.parametrize("name,form", [("uv40", 0), ("uv40", 1), ("frames_of", 0), ("frames_of", 1), ("m96x128", 0)])
def test_bit_reproducible_and_device_arguments(eng, corpus, expected, name, form):
    """Two identical forward calls and two identical backward calls give the same bits; so do host and device pointers."""
    import torch
    case = corpus[name]
    _set(eng, case)
    eng.set_option("refine_soft_form", form)
    a, b = _fwd(eng, case), _fwd(eng, case)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
    dev = lambda v: torch.as_tensor(v, device="cuda:0")
    douts = tuple(dev(o) for o in _fwd_outputs(case.B))
    torch.cuda.synchronize()
    assert _fwd(eng, case, outs=douts, conv=dev, sync=True)[0] == 0
    for x, y in zip(a[1:], douts):
        assert np.array_equal(x, y.cpu().numpy(), equal_nan=x.dtype.kind == "f")
    ref = expected[name]["h"]
    dL, coef, grad0 = _grad_inputs(case, 6)
    g1, g2, ok1, ok2 = grad0.copy(), grad0.copy(), np.zeros(case.B, np.int32), np.zeros(case.B, np.int32)
    assert _bwd(eng, case, ref, dL, coef, g1, ok1) == 0 and _bwd(eng, case, ref, dL, coef, g2, ok2) == 0
    assert np.array_equal(g1, g2) and np.array_equal(ok1, ok2) and not np.array_equal(g1, grad0)
    dg, dok = dev(grad0.copy()), dev(np.zeros(case.B, np.int32))
    torch.cuda.synchronize()
    assert _bwd(eng, case, ref, dL, coef, dg, dok, conv=dev, sync=True) == 0
    assert np.array_equal(dg.cpu().numpy(), g1) and np.array_equal(dok.cpu().numpy(), ok1)


@pytest.mark.parametrize("form", [0, 1], ids=["split", "fused"])
def test_frame_batch_equals_single_frames(eng, corpus, expected, form):
    """frames_of on the batch against its problems run frame by frame through dsac_set_frame with that frame's camera: the same bits, forward and backward."""
    case = corpus["frames_of"]
    eng.set_option("refine_soft_form", form)
    _set(eng, case)
    rc, h, S, it, status = _fwd(eng, case)
    assert rc == 0
    ref = expected["frames_of"]["h"]
    dL, coef, grad0 = _grad_inputs(case, 9)
    g = grad0.copy()
    assert _bwd(eng, case, ref, dL, coef, g) == 0
    for f in range(case.F):
        sel = np.flatnonzero(case.frame_of == f)
        sub = sr.Case("f%d" % f, case.xyz[f:f + 1], case.uv, case.H, case.W, case.cams[f:f + 1], case.poses[sel], np.zeros(len(sel), np.int32), False, case.tau, case.beta,
                      case.cut, case.min_soft, case.max_iters, case.step_tol)
        _set(eng, case, only=f)
        rc, h1, S1, it1, st1 = _fwd(eng, sub)
        assert rc == 0
        assert np.array_equal(h1, h[sel]) and np.array_equal(S1, S[sel]) and np.array_equal(it1, it[sel]) and np.array_equal(st1, status[sel])
        g1 = grad0[f:f + 1].copy()
        assert _bwd(eng, sub, ref[sel], dL[sel], coef[sel], g1) == 0
        assert np.array_equal(g1[0], g[f])


def test_forms_and_option(eng, corpus):
    """The option is read back; the forms agree far inside the bound's ceiling on a case (they need not agree bit for bit)."""
    case = corpus["grid37x53"]
    _set(eng, case)
    assert eng.get_option("refine_soft_form") == -1
    res = {}
    for form in (0, 1, -1):
        eng.set_option("refine_soft_form", form)
        assert eng.get_option("refine_soft_form") == form
        res[form] = _fwd(eng, case)
        assert res[form][0] == 0
    for x, y in zip(res[1][1:], res[-1][1:]):  # 1 961 cells: auto is the fused form
        assert np.array_equal(x, y)
    assert np.array_equal(res[0][3], res[1][3]) and np.array_equal(res[0][4], res[1][4])
    assert np.abs(res[0][1] - res[1][1]).max() <= 1e-6 * max(1.0, np.abs(res[1][1]).max())
    for bad in (-2, 2):
        assert lib.dsac_set_option(eng._ctx, b"refine_soft_form", bad) == INVALID
    assert eng.get_option("refine_soft_form") == -1


def test_refusals(eng, corpus, expected):
    """Every refusal of the header, DSAC_ERR_INVALID by name, with nothing written."""
    case = corpus["frames_b6"]
    _set(eng, case)
    nan, inf = float("nan"), float("inf")

    def refused(**over):
        outs = _fwd_outputs(case.B)
        rc = _fwd(eng, case, outs=outs, **over)[0]
        assert (outs[0] == -7.5).all() and (outs[1] == -7.5).all() and (outs[2] == -7).all() and (outs[3] == -7).all(), over
        assert rc != 0 and b"dsac_refine_soft:" in lib.dsac_last_error(eng._ctx), over
        return rc

    assert refused(B=0) == INVALID and refused(B=5) == INVALID  # 5 problems on 3 frames without frame_of
    assert refused(max_iters=0) == INVALID and refused(max_iters=65) == INVALID
    assert refused(cut=0.0) == INVALID and refused(cut=100.5) == INVALID and refused(cut=nan) == INVALID
    assert refused(beta=0.0) == INVALID and refused(beta=-0.5) == INVALID
    for key in ("tau", "beta", "min_soft", "step_tol"):
        assert refused(**{key: nan}) == INVALID and refused(**{key: inf}) == INVALID
    assert refused(step_tol=-1e-9) == INVALID
    assert refused(poses=None) == INVALID
    assert lib.dsac_refine_soft(eng._ctx, case.B, ptr(np.ascontiguousarray(case.poses)), None, 10.0, 0.5, 42.0, 50.0, 20, 1e-6, None, None, None, None) == INVALID
    assert lib.dsac_refine_soft(None, 1, None, None, 10.0, 0.5, 42.0, 50.0, 20, 1e-6, None, None, None, None) == INVALID

    ref = expected["frames_b6"]["h"]
    dL, coef, grad0 = _grad_inputs(case, 7)

    def refused_bwd(**over):
        g, ok = grad0.copy(), np.full(case.B, -7, np.int32)
        kw = dict(grad=g)
        kw.update(over)
        flags = kw.pop("flags", 0)
        rc = _bwd(eng, case, kw.pop("ref", ref), kw.pop("dL", dL), coef, kw.pop("grad"), ok, flags=flags, **kw)
        assert np.array_equal(g, grad0) and (ok == -7).all(), over
        assert rc != 0 and b"dsac_refine_soft_backward:" in lib.dsac_last_error(eng._ctx), over
        return rc

    assert refused_bwd(B=0) == INVALID and refused_bwd(B=5) == INVALID
    assert refused_bwd(cut=0.0) == INVALID and refused_bwd(cut=101.0) == INVALID and refused_bwd(beta=0.0) == INVALID
    for key in ("tau", "beta", "min_soft"):
        assert refused_bwd(**{key: nan}) == INVALID
    assert refused_bwd(poses=None) == INVALID and refused_bwd(dL=None) == INVALID and refused_bwd(grad=None) == INVALID
    assert refused_bwd(flags=2) == INVALID
    import dsac_amd
    with dsac_amd.Engine(0) as fresh:  # a context without a frame
        outs = _fwd_outputs(case.B)
        assert _fwd(fresh, case, outs=outs)[0] == NO_FRAME and (outs[0] == -7.5).all()
        g = grad0.copy()
        assert _bwd(fresh, case, ref, dL, coef, g) == NO_FRAME and np.array_equal(g, grad0)
    # the same arguments are accepted once nothing is wrong with them
    assert _fwd(eng, case)[0] == 0 and _bwd(eng, case, ref, dL, coef, grad0.copy()) == 0


def test_engine_entries(eng, corpus, expected, expected_bwd):
    """Engine.refineSoft / Engine.dRefineSoft: defaults (cut = tau + 16 / beta = 42), the returned tuples, the gradient allocated when none is given."""
    case, exp = corpus["uv40"], expected["uv40"]
    _set(eng, case)
    h, S, it, status = eng.refineSoft(case.poses)
    assert np.array_equal(status, exp["status"]) and np.array_equal(it, exp["iters"])
    rc, h2, S2, it2, st2 = _fwd(eng, case)
    assert rc == 0 and np.array_equal(h, h2, equal_nan=True) and np.array_equal(S, S2)
    dL, coef, _ = _grad_inputs(case, 8)
    g, ok = eng.dRefineSoft(exp["h"], dL, coef=coef)
    assert g.shape == (case.P, 3) and np.array_equal(ok, [0 if r is None else 1 for r in expected_bwd["uv40"][False]])
    want, tol, touched = sr.expected_grad(case, expected_bwd["uv40"][False], dL, coef, np.zeros((1, case.P, 3)))
    assert float((np.abs(g[None] - want)[touched] / tol[touched]).max()) <= 1.0
    g2, _ = eng.dRefineSoft(exp["h"], dL, coef=coef, grad=g.copy())
    assert np.allclose(g2, 2 * g, rtol=1e-12, atol=0)
    gf, _ = eng.dRefineSoft(exp["h"], dL, coef=coef, fixed_weights=True)
    want, tol, touched = sr.expected_grad(case, expected_bwd["uv40"][True], dL, coef, np.zeros((1, case.P, 3)))
    assert float((np.abs(gf[None] - want)[touched] / tol[touched]).max()) <= 1.0 and not np.array_equal(gf, g)


def _dsac_forward(engine, fr, N=32, **kw):
    engine.set_frame(fr["xyz"], fr["uv"], 40, 40, fr["cam"])
    perm = synth.fast_permutations(1600, 8, seed=3)
    gt = synth.cv_to_jp6(fr["gt_pose"] + np.array([0.01, -0.02, 0.01, 5.0, -8.0, 12.0]))
    # alpha = 0.01: a flat softmax, so that more than a handful of the 32 hypotheses carry weight above min_prob
    return perm, gt, engine.processImageDSAC(N=N, seed=77, perm=perm, gt_jp6=gt, draw_u=0.37, alpha=0.01, **kw)


def test_process_and_backward_dsac(eng):
    """processImageDSAC(refine="soft") refines with refineSoft; backwardDSAC(refine_grad="soft") = the numpy composition w x dLossMax x reference Jacobians + the
    unchanged path II.  Hypotheses whose refined pose does not meet the corpus conditions for the backward (cond(H)) are given no weight.  The default paths
    stay bit-equal to the calls without the new arguments (zero losses: path II's fp64 atomics add nothing then)."""
    fr = synth.chess_like_frame(40, 40, seed=44, outlier_frac=0.3)
    perm, gt, fwd = _dsac_forward(eng, fr, refine="soft")
    ref2, S2, it2, st2 = eng.refineSoft(fwd["hyps"], min_soft=50.0)
    assert np.array_equal(fwd["refHyps"], ref2, equal_nan=True) and np.array_equal(fwd["refSteps"], it2) and np.array_equal(fwd["refStatus"], st2)
    assert fwd["inlierMaps"] is None
    w, ref = fwd["sfScores"].copy(), fwd["refHyps"]
    case = sr.Case("dsac", fr["xyz"][None], fr["uv"], 40, 40, [fr["cam"]], ref, np.zeros(len(w), np.int32), False)
    bwd = sr.expected_backward(case, ref)
    for b in range(case.B):
        if bwd[b] is None or bwd[b]["cond"] > sr.COND_MAX:
            w[b] = 0.0
    sel = np.flatnonzero(w > 1e-4)
    assert len(sel) >= 3, "too few hypotheses carry weight for this test to mean anything"
    fwd = dict(fwd, sfScores=w)
    out = eng.backwardDSAC(fwd, gt, refine_grad="soft")
    dL = out["dLoss_dRef"]
    g_soft = eng.selectDSAC(w, fwd["losses"])[2]
    path2 = eng.dSoftScore(fwd["hyps"], fwd["sampledPoints"], g_soft * fwd["score_scale"])
    sub = sr.Case("dsac_sel", fr["xyz"][None], fr["uv"], 40, 40, [fr["cam"]], ref[sel], np.zeros(len(sel), np.int32), False)
    want, tol, _ = sr.expected_grad(sub, [bwd[b] for b in sel], dL[sel], w[sel], path2.reshape(1, 1600, 3))
    # path II is summed again inside backwardDSAC: at most 4 N + 1 fp64 additions per entry in the atomics' own order (tests/test_gpu_refine_gn.py)
    tol = tol + (4 * len(w) + 1) * sr.EPS * np.abs(path2).max()
    worst = float((np.abs(out["grad"].reshape(1, 1600, 3) - want) / np.maximum(tol, 1e-300)).max())
    margin("soft", "backwardDSAC(refine_grad=soft): |grad - (path II + w dL J_ref)| over its bound, worst entry (%d hypotheses)" % len(sel), worst, 1.0)
    # the defaults: "walk" and "fd" are the calls without the arguments
    _, _, a = _dsac_forward(eng, fr)
    _, _, b = _dsac_forward(eng, fr, refine="walk")
    for k in ("hyps", "refHyps", "refSteps", "inlierMaps", "sfScores", "losses"):
        assert np.array_equal(a[k], b[k]), k
    assert "refStatus" not in a
    zero = dict(a, losses=np.zeros_like(a["losses"]))
    x, y = eng.backwardDSAC(zero, gt), eng.backwardDSAC(zero, gt, refine_grad="fd")
    assert np.abs(x["grad"]).max() > 0 and np.array_equal(x["grad"], y["grad"]) and np.array_equal(x["dLoss_dRef"], y["dLoss_dRef"])
    with pytest.raises(ValueError):
        eng.backwardDSAC(fwd, gt, refine_grad="exact")
    with pytest.raises(ValueError):
        _dsac_forward(eng, fr, refine="hard")
