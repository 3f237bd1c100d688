"""dsac_refine_soft and dsac_refine_soft_backward on the GPU off the easy corpus: the cases of tests/refine_soft_wild.py (P3P hypotheses of the CPU oracle's sampler
as start poses, batches of 256 and 210 problems, dead cells and cells on the camera plane, maps below one 64-lane trip).  Decided problems are compared with the
restatement as tests/test_gpu_refine_soft.py compares its corpus; every problem gets the postconditions of the header's definition.  The tolerances come from the
restatement and its plain-float64 form on the CPU (refine_soft_wild.float64_figures), never from the kernel's output; tests/test_refine_soft_wild_cpu.py shows what
they reject."""
import numpy as np
import pytest

import refine_soft_ref as sr
import refine_soft_wild as sw
from conftest import margin
from dsac_amd.capi import lib
from test_gpu_refine_soft import FORM_NAME, _bwd, _fwd, _report, _set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return sw.cases()


@pytest.fixture
def eng(engine):
    yield engine
    engine.set_option("refine_soft_form", -1)


def _hist(status):
    return " ".join("%s %d" % (sr.STATUS[s], int((status == s).sum())) for s in range(6) if (status == s).any())


_POST_CACHE = {}


def _check_forward(case, form, h, S, it, status):
    """Decided problems against the restatement; the postconditions on every problem.  Reports and asserts the worst ratios."""
    exp, f64 = sw.expected(case), sw.float64_figures(case)
    dec = exp["decided"]
    tag = "%s %s" % (case.name, FORM_NAME[form])
    _report("forward  %-18s %-5s B %d  kernel: %s | restatement: %s | undecided %d" %
            (case.name, FORM_NAME[form], case.B, _hist(status), _hist(exp["status"]), int((~dec).sum())))
    failures = []
    worst_h = worst_S = low_S = worst_pass = 0.0
    for b in range(case.B):
        pr = sw.problem(case, b)
        bad = sw.postconditions(pr, h[b], S[b], it[b], status[b], f64["pass_rel"], _POST_CACHE)
        if bad:
            failures.append((b, "postconditions", bad))
        if np.all(np.isfinite(h[b])) and status[b] != sr.NONFINITE:
            P = sw.cached_pass(pr, h[b], _POST_CACHE)
            worst_pass = max(worst_pass, (abs(S[b] - P["S"]) - P["near"]) / max(P["S"], 1.0))
        if not dec[b]:
            continue
        if status[b] != exp["status"][b] or it[b] != exp["iters"][b]:
            failures.append((b, "decided", "%s after %d steps, the restatement: %s after %d" % (sr.STATUS[status[b]], it[b], sr.STATUS[exp["status"][b]], exp["iters"][b])))
            continue
        if exp["status"][b] in (sr.CONVERGED, sr.MAXIT, sr.SCORE):
            rh, rS = sr.forward_ratios(h[b], S[b], exp, b)
            # rho cond(A) 2^-52 bounds what the solve's rounding moves.  Where cond(A) is small (7.96 on dead_zero) that is below one rounding of S itself: there
            # the floor of refine_soft_wild.float64_figures is the bound on S, everywhere else rho is (the larger of the two, never the sum)
            dS, S_ref = abs(S[b] - exp["S"][b]), exp["S"][b]
            if f64["rho"] * exp["cond"][b] * sr.EPS * S_ref < f64["S_floor"] * max(S_ref, 1.0):
                low_S, rS = max(low_S, dS / (f64["S_floor"] * max(S_ref, 1.0))), 0.0
            worst_h, worst_S = max(worst_h, rh), max(worst_S, rS)
    _report("forward  %-18s %-5s worst ratio over cond(A) 2^-52: kernel |h - h_ref| %.3e |S - S_ref| %.3e (%.3e of the floor where that is the larger bound) | "
            "CPU float64 |h - h_ref| %.3e |S - S_ref| %.3e (flips %d) | rho %.3e" %
            (case.name, FORM_NAME[form], worst_h, worst_S, low_S, f64["ratio_h"], f64["ratio_S"], f64["flips"], f64["rho"]))
    _report("forward  %-18s %-5s pass |S - S_ref(h_out)| / max(S_ref, 1): kernel %.3e | CPU float64 %.3e | tolerance %.3e" %
            (case.name, FORM_NAME[form], worst_pass, f64["pass_ratio"], f64["pass_rel"]))
    assert not failures, (tag, len(failures), failures[:8])
    margin("soft", "%s: |h - h_ref|inf / (cond(A) 2^-52 max(1, |h_ref|inf)), worst decided problem" % tag, worst_h, f64["rho"])
    margin("soft", "%s: |S - S_ref| / (cond(A) 2^-52 S_ref), worst decided problem" % tag, worst_S, f64["rho"])
    margin("soft", "%s: |S - S_ref| over the floor of the S bound where rho cond(A) 2^-52 S_ref is below it, worst decided problem" % tag, low_S, 1.0)
    margin("soft", "%s: pass |S - S_ref(h_out)| / max(S_ref, 1), worst problem" % tag, worst_pass, f64["pass_rel"])


WILD_FORMS = [(n, f) for n in sw.FORWARD_CASES for f in (0, 1)]


@pytest.mark.parametrize("name,form", WILD_FORMS, ids=["%s-%s" % (n, FORM_NAME[f]) for n, f in WILD_FORMS])
def test_forward_wild(eng, cases, name, form):
    case = cases[name]
    _set(eng, case)
    eng.set_option("refine_soft_form", form)
    rc, h, S, it, status = _fwd(eng, case)
    assert rc == 0, lib.dsac_last_error(eng._ctx)
    if name == "dead_cells":  # the dead cells leave every problem finite
        assert np.isfinite(h).all() and np.isfinite(S).all()
    if name == "one_live3x5":  # the zero pose meets a pivot of exactly zero in any fp64 evaluation (refine_soft_wild.cases, (5))
        assert status[0] == sr.SINGULAR and it[0] == 0 and not h[0].any()
    _check_forward(case, form, h, S, it, status)


@pytest.mark.parametrize("form", [0, 1], ids=["split", "fused"])
@pytest.mark.parametrize("name", ["sampled_frames", "sampled_frames_of"])
def test_frame_batches_equal_single_frames(eng, cases, name, form):
    """210 problems by the call's own mapping, and 100 shuffled ones of which frame 1 has none and frame 0 has 70: the same bits as frame by frame."""
    case = cases[name]
    eng.set_option("refine_soft_form", form)
    _set(eng, case)
    rc, h, S, it, status = _fwd(eng, case)
    assert rc == 0, lib.dsac_last_error(eng._ctx)
    for f in range(case.F):
        sel = np.flatnonzero(case.frame_of == f)
        if not len(sel):
            continue
        sub = sr.Case("f%d" % f, case.xyz[f:f + 1], case.uv, case.H, case.W, case.cams[f:f + 1], case.poses[sel], np.zeros(len(sel), np.int32), False, **sw.par_of(case))
        _set(eng, case, only=f)
        rc, h1, S1, it1, st1 = _fwd(eng, sub)
        assert rc == 0
        assert np.array_equal(h1, h[sel], equal_nan=True) and np.array_equal(S1, S[sel]) and np.array_equal(it1, it[sel]) and np.array_equal(st1, status[sel]), (name, f)


def _bwd_inputs(sub, bwd, seed):
    """Random dL and coef, a non-zero gradient to accumulate into with NaN entries at cells that no problem touches."""
    rng = np.random.default_rng(seed)
    dL = rng.normal(size=(sub.B, 6)) * np.array([100.0, 100.0, 100.0, 1.0, 1.0, 1.0])
    coef, grad0 = rng.uniform(0.1, 1.0, size=sub.B), rng.normal(size=(sub.F, sub.P, 3))
    touched = sr.expected_grad(sub, bwd, dL, coef, grad0)[2]
    free = np.argwhere(~touched)
    assert len(free) >= 4, "every cell carries weight: nowhere to put a NaN"
    for f, p in free[:: max(1, len(free) // 16)]:
        grad0[f, p, (f + p) % 3] = np.nan
    return dL, coef, grad0


@pytest.mark.parametrize("fixed", [False, True], ids=["weight-derivatives", "fixed-weights"])
@pytest.mark.parametrize("name", sw.BACKWARD_CASES)
def test_backward_wild(eng, cases, name, fixed):
    """The backward at the restatement's refined poses on full batches: ok_out exact, the gradient within expected_grad's per-term bound, untouched cells (NaN
    entries among them) bit-equal, two calls bit-identical -- sampled_frames by the call's own mapping, sampled_frames_of by frame_of; and the scatter's tile loop in isolation: the gradient of the batch minus that of problems 0 .. 31
    alone is the gradient of problems 32 .. alone, within the rounding of the cells' sums."""
    case = cases[name]
    sel, ref, bwd = sw.backward_selection(case, sw.expected(case), fixed)
    sub = sw.subcase(case, sel, frame_of=case.frame_of[sel], give=True if case.F > 1 else False)
    none = sum(r is None for r in bwd)
    _report("backward %-18s %-18s kept %d of %d problems, %d without a result, worst cond(H) %.2e" %
            (name, "fixed weights" if fixed else "weight derivatives", sub.B, case.B, none, max(r["cond"] for r in bwd if r is not None)))
    assert sub.B > 32 and (name not in sw.SAMPLED or sub.B >= 200)
    # the call itself keeps the case's way of naming frames.  sampled_frames: the call's own mapping b // 70, so that k_soft_scatter walks the window b0 .. b1 of
    # its frame (b0 = 70 f, tiles of 32 / 32 / 6, records without a result at 7 and 37 inside frame 0's window); that needs every problem kept
    if name == "sampled_frames":
        assert len(sel) == case.B and not case.give_frame_of
    call = sub if case.give_frame_of or len(sel) != case.B else sw.subcase(case, sel, give=False)
    _set(eng, sub)
    flags = 1 if fixed else 0
    dL, coef, grad0 = _bwd_inputs(sub, bwd, 11)
    g, ok = grad0.copy(), np.full(sub.B, -7, np.int32)
    assert _bwd(eng, call, ref, dL, coef, g, ok, flags=flags) == 0, lib.dsac_last_error(eng._ctx)
    assert np.array_equal(ok, [0 if r is None else 1 for r in bwd]), (name, np.flatnonzero(ok != np.array([0 if r is None else 1 for r in bwd])))
    want, tol, touched = sr.expected_grad(sub, bwd, dL, coef, grad0)
    assert np.isnan(grad0[~touched]).any() and touched.any()
    assert np.array_equal(g[~touched].view(np.int64), grad0[~touched].view(np.int64))
    worst = float((np.abs(g - want)[touched] / tol[touched]).max())
    g2, ok2 = grad0.copy(), np.full(sub.B, -7, np.int32)
    assert _bwd(eng, call, ref, dL, coef, g2, ok2, flags=flags) == 0
    assert np.array_equal(g2.view(np.int64), g.view(np.int64)) and np.array_equal(ok2, ok)
    # the tile loop: full = first + rest, each from a zero gradient
    zero = np.zeros_like(grad0)
    parts = {}
    for key, idx in (("full", np.arange(sub.B)), ("first", np.arange(32)), ("rest", np.arange(32, sub.B))):
        part = sw.subcase(sub, idx, frame_of=sub.frame_of[idx], give=sub.give_frame_of)
        parts[key] = zero.copy()
        assert _bwd(eng, part, ref[idx], dL[idx], coef[idx], parts[key], None, flags=flags) == 0
    if not call.give_frame_of and case.F > 1:  # the window b0 .. b1 and frame_of name the same problems of a frame in the same order: the same bits
        own = zero.copy()
        assert _bwd(eng, call, ref, dL, coef, own, None, flags=flags) == 0
        assert np.array_equal(own, parts["full"])
    _, tol0, touched0 = sr.expected_grad(sub, bwd, dL, coef, zero, rho=0.0)  # (2 count + 1) 2^-52 of the absolute sum per entry: the sums' own rounding
    assert np.abs(parts["first"]).max() > 0 and np.abs(parts["rest"]).max() > 0
    assert not parts["full"][~touched0].any() and not parts["rest"][~touched0].any()
    split = float((np.abs((parts["full"] - parts["first"]) - parts["rest"])[touched0] / (2 * tol0[touched0])).max())
    _report("backward %-18s %-18s kernel: |grad - ref| over its bound %.3e | |(full - problems 0..31) - problems 32..| over the sums' rounding %.3e" %
            (name, "fixed weights" if fixed else "weight derivatives", worst, split))
    margin("soft", "%s %s: |grad - ref| over its bound, worst entry (%d problems)" % (name, "fixed weights" if fixed else "weight derivatives", sub.B), worst, 1.0)
    margin("soft", "%s %s: |(grad - grad of problems 0..31) - grad of problems 32..| over the sums' rounding" % (name, "fixed weights" if fixed else "weight derivatives"),
           split, 1.0)
