"""tests/refine_soft_wild.py on the CPU: (a) the conditions of its cases, from the restatement alone, (b) that the postconditions accept the restatement's own
outputs on every problem of every case, (c) that they reject six wrong kernels, modelled as edits of the restatement, and that expected_grad rejects a gradient
without the second scatter tile, (d) that the restatement applies the z = 1 rule to a cell on the camera plane."""
import numpy as np
import pytest

import refine_soft_ref as sr
import refine_soft_wild as sw
from refine_gn_ref import jacobians


@pytest.fixture(scope="module")
def cases():
    return sw.cases()


def _hist(status):
    return {sr.STATUS[s]: int((status == s).sum()) for s in range(6) if (status == s).any()}


def test_case_conditions(cases):
    """At most 2 % of a sampled case is undecided; FEW, MAXIT, SCORE and CONVERGED all occur among the sampled problems; the shapes are what the kernels' paths need."""
    seen = set()
    for name in sw.FORWARD_CASES:
        case, exp = cases[name], sw.expected(cases[name])
        und = int((~exp["decided"]).sum())
        print("%-18s B %3d  undecided %d (%.2f %%)  %s  S0 %.3g .. %.3g  worst decided cond(A) %.3g" %
              (name, case.B, und, 100.0 * und / case.B, _hist(exp["status"]), exp["S0"].min(), exp["S0"].max(),
               np.nanmax(np.where(exp["decided"], exp["cond"], np.nan)) if np.isfinite(np.where(exp["decided"], exp["cond"], np.nan)).any() else 0.0))
        if name.startswith("sampled"):
            assert und <= 0.02 * case.B, (name, und)
            seen |= set(int(s) for s in exp["status"])
        assert not (exp["decided"] & (exp["status"] == sr.SINGULAR)).any(), name  # never on a problem the corpus conditions accept
    assert {sr.FEW, sr.MAXIT, sr.SCORE, sr.CONVERGED} <= seen, [sr.STATUS[s] for s in seen]
    assert cases["sampled44"].B == 256 and cases["sampled45"].B == 256
    sf, so = cases["sampled_frames"], cases["sampled_frames_of"]
    assert sf.B == 210 and not sf.give_frame_of and np.array_equal(sf.frame_of, np.arange(210) // 70)
    counts = np.bincount(so.frame_of, minlength=3)
    assert so.give_frame_of and counts[1] == 0 and counts.max() > 64 and (np.diff(so.frame_of) != 0).sum() > 10, counts
    assert [cases[n].P for n in sw.TINY_CASES] == [15, 255, 256, 257] and all(cases[n].uv is None and cases[n].B == 8 for n in sw.TINY_CASES)


def test_dead_cells_case(cases):
    """16 NaN cells, 8 infinite cells, 8 cells on the zero pose's camera plane that are live under the z = 1 rule -- which the restatement applies; 40 poses that
    were decided on the clean frame."""
    case = cases["dead_cells"]
    xyz, cells = case.xyz[0], case.cells
    assert np.isnan(xyz[cells["nan"]]).any(1).all() and np.isinf(xyz[cells["inf"]]).any(1).all() and (xyz[cells["plane"], 2] == 0).all()
    assert case.B == sw.N_DEAD_POSES + 1 and not case.poses[-1].any()
    assert np.isfinite(np.delete(xyz, np.concatenate([cells["nan"], cells["inf"]]), axis=0)).all()
    fx, fy, cx, cy = case.cams[0].astype(np.float64)
    r, J, G = jacobians(np.zeros(6), xyz[cells["plane"]], case.uv[cells["plane"]], case.cams[0])
    X, uv = xyz[cells["plane"]].astype(np.float64), case.uv[cells["plane"]].astype(np.float64)
    assert np.array_equal(r, np.stack([X[:, 0] * fx + cx - uv[:, 0], X[:, 1] * fy + cy - uv[:, 1]], -1))  # z = 1
    assert np.isfinite(J).all() and np.isfinite(G).all() and np.array_equal(J[:, 0, 3], np.full(8, fx))
    _, _, _, e, w = sr.cell_terms(np.zeros(6), xyz, case.uv, case.cams[0], case.tau, case.beta, case.cut)
    assert (e[cells["plane"]] < 2.5).all() and (w[cells["plane"]] > 0.9).all()
    assert not w[cells["nan"]].any() and not w[cells["inf"]].any()
    exp = sw.expected(case)
    assert np.isfinite(exp["h"]).all() and np.isfinite(exp["S"]).all()
    assert (exp["decided"][:-1].sum() >= 36), exp["decided"]  # the 32 cells change little for poses that were decided without them


def test_one_live_cell_is_singular(cases):
    """One finite cell on the optical axis at the zero pose: row and column 2 of A are exact zeros, so the plain-float64 L D L^T factorisation -- the kernel's
    solve -- meets a pivot of exactly zero and the status is SINGULAR; the postconditions accept that, and every problem of the case is undecided."""
    case, exp = cases["one_live3x5"], sw.expected(cases["one_live3x5"])
    assert not exp["decided"].any() and np.isfinite(case.xyz[0]).all(1).sum() == 1
    pr = sw.problem(case, 0)
    P = sw.pass_at(case.poses[0], pr, plain=True)
    assert 0.5 < P["S"] < 1.0 and not P["A"][2].any() and not P["A"][:, 2].any() and P["A"][0, 0] > 0 and P["A"][1, 1] > 0 and P["A"][0, 1] == 0
    r = sw.run_loop(pr, plain=True)
    assert r["status"] == sr.SINGULAR and r["iters"] == 0
    assert not sw.postconditions(pr, r["h"], r["S"], r["iters"], r["status"])
    print("one_live3x5: plain-float64 loop", [sr.STATUS[sw.run_loop(sw.problem(case, b), plain=True)["status"]] for b in range(case.B)])


@pytest.mark.parametrize("name", sw.FORWARD_CASES)
def test_postconditions_accept_the_restatement(cases, name):
    case, exp, f64 = cases[name], sw.expected(cases[name]), sw.float64_figures(cases[name])
    print("%-18s plain-float64 pass |S_64 - S_ref| / max(S_ref, 1) %.3e -> pass tolerance %.3e;  float64 loop ratios h %.3e S %.3e (flips %d) -> rho %.3e" %
          (name, f64["pass_ratio"], f64["pass_rel"], f64["ratio_h"], f64["ratio_S"], f64["flips"], f64["rho"]))
    assert sr.RHO_ASSERT <= f64["rho"] <= sr.RHO_CEILING
    for b in range(case.B):
        bad = sw.postconditions(sw.problem(case, b), exp["h"][b], exp["S"][b], exp["iters"][b], exp["status"][b], f64["pass_rel"])
        assert not bad, (name, b, bad)


@pytest.mark.parametrize("variant", sw.POST_VARIANTS)
def test_postconditions_reject_wrong_kernels(cases, variant):
    """Each wrong kernel run on the first eight problems of every status in sampled44 and sampled45 and on dead_zero: the postconditions alone reject it on at least one problem,
    and on every problem where the edit changes what is returned in a way the header rules out for that status (FEW for a moved pose, SCORE for S at the trial, MAXIT for the step count;
    a step taken although S fell where it falls below the start pose: after accepted steps the header's guarantees on the returned pose alone need not see it, which is
    why decided problems are also compared with the restatement).  A problem the edit does not change is accepted."""
    rejected, changed, must = 0, 0, {"s_at_trial": sr.SCORE, "accept_fall": sr.SCORE, "few_moved": sr.FEW, "iters_plus_one": sr.MAXIT}.get(variant)
    picks = [(n, int(b)) for n in sw.SAMPLED for s in range(4) for b in np.flatnonzero(sw.expected(cases[n])["status"] == s)[:8]]
    picks.append(("dead_zero", 0))  # SCORE at the first step: the sampled problems fall only after accepted steps
    for name, b in picks:
        case, exp = cases[name], sw.expected(cases[name])
        rel = sw.float64_figures(case)["pass_rel"]
        pr = sw.problem(case, b)
        r = sw.run_loop(pr, variant=variant)
        bad = sw.postconditions(pr, r["h"], r["S"], r["iters"], r["status"], rel)
        differs = not (np.array_equal(r["h"], exp["h"][b]) and r["S"] == exp["S"][b] and r["iters"] == exp["iters"][b] and r["status"] == exp["status"][b])
        assert differs or not bad, (b, bad)
        changed += differs
        rejected += bool(bad)
        if must is not None and exp["status"][b] == must and exp["decided"][b] and (variant != "accept_fall" or exp["iters"][b] == 0):
            assert bad, (variant, b, sr.STATUS[must])
    print("%-16s changes %d of %d problems, rejected on %d" % (variant, changed, len(picks), rejected))
    assert rejected >= 1


def test_postconditions_reject_a_dead_cell_counted(cases):
    """A cell whose residual is not a number counted with weight 1: S is off by the number of such cells on every problem."""
    case = cases["dead_cells"]
    rel = sw.float64_figures(case)["pass_rel"]
    for b in (0, 17, case.B - 1):
        pr = sw.problem(case, b)
        r = sw.run_loop(pr, variant="dead_as_one")
        assert sw.postconditions(pr, r["h"], r["S"], r["iters"], r["status"], rel), b


@pytest.mark.parametrize("fixed", [False, True], ids=["weight-derivatives", "fixed-weights"])
def test_backward_selection_and_the_missing_tile(cases, fixed):
    """At least 200 of 256 problems stay in the backward of the sampled cases, problems without a result among them; expected_grad rejects the gradient of the first
    32 problems alone (what a scatter that stops after its first tile gives)."""
    for name in sw.BACKWARD_CASES:
        case, exp = cases[name], sw.expected(cases[name])
        sel, _, bwd = sw.backward_selection(case, exp, fixed)
        none = sum(r is None for r in bwd)
        print("%-10s %-18s kept %d of %d, %d without a result, worst cond(H) %.3g" %
              (name, "fixed weights" if fixed else "weight derivatives", len(sel), case.B, none, max(r["cond"] for r in bwd if r is not None)))
        assert len(sel) >= (200 if name in sw.SAMPLED else 34) and any(r is None for r in bwd[:32]) and any(r is None for r in bwd[32:])
        sub = sw.subcase(case, sel)
        rng = np.random.default_rng(3)
        dL, coef, grad0 = rng.normal(size=(sub.B, 6)), rng.uniform(0.1, 1.0, size=sub.B), rng.normal(size=(sub.F, sub.P, 3))
        want, tol, touched = sr.expected_grad(sub, bwd, dL, coef, grad0)
        first = sr.expected_grad(sw.subcase(case, sel[:32]), bwd[:32], dL[:32], coef[:32], grad0)[0]
        assert (np.abs(first - want)[touched] > tol[touched]).mean() > 0.5
