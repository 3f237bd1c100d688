"""numpy restatement of dsac_refine_soft and dsac_refine_soft_backward (include/dsac_hip.h has the definitions) and the corpus their tests run on.

What is restated:
    cell terms     r_p, J_p, G_p from tests/refine_gn_ref.py (float64; dR / d rho written as [J_l e_j]x R, a second derivation of the kernel's), e_p = |r_p|, the
                   weight w_p = 1 / (1 + exp(-beta (tau - e_p))) in float64, zero where e_p is not finite or e_p >= cut
    pass           S = sum w, A = sum w J^T J, g = sum w J^T r, summed in np.longdouble
    loop           the header's steps 1 - 5; delta = A^-1 g with A inverted in long double (refine_gn_ref.inverse_ld); poses and the tests on |delta| and S in
                   float64, as the kernel holds them
    backward       M_p = w I + (w' / e) r r^T, H = sum J^T M J (long double), d h / d X_p = -H^-1 J^T M G, mapped through T = d cv_to_jp6 / d cv6

Corpus conditions, checked at every iterate of the restatement so that no decision of the loop sits on an edge the kernel's rounding could cross:
    |S' - S| >= 1e-10 S,   | |delta| / lim - 1 | >= 1e-6,   |S - min_soft| >= 1e-6,   no cell within 1e-9 px of cut,   cond(A) <= 1.4e8.

The bound.  Kernel and restatement evaluate the same formulas; what separates them is rounding amplified by the solve:
    |h - h_ref|_inf <= RHO_ASSERT cond(A) 2^-52 max(1, |h_ref|_inf),   |S - S_ref| <= RHO_ASSERT cond(A) 2^-52 S_ref
with cond(A) the largest over the problem's iterates, and for the backward per problem
    max |J - J_ref| <= RHO_BWD_ASSERT cond(H) 2^-52 max |J_ref|.
RHO_* = 8 x the worst ratio measured on the MI355X over the corpus (profiles/refine_soft_margins.txt), the factor for compiler changes; never above 32, which
with cond <= 1.4e8 keeps every bound at or below 1e-6 relative.
WRONG_VARIANTS are one-term mistakes that tests/test_refine_soft_ref_cpu.py shows to fail the backward bound by a large factor.
"""
import numpy as np

from refine_gn_ref import cv_to_jp6_jacobian, grid_uv, inverse_ld, jacobians, synth

EPS = 2.0 ** -52
COND_MAX = 1.4e8
RHO_CEILING = 32.0
RHO_MEASURED = 6.6e-7  # worst forward ratio over the corpus on the MI355X, both forms: |S - S_ref|, uv40_it1_cut100 split (profiles/refine_soft_margins.txt)
RHO_BWD_MEASURED = 4.1e-5  # worst backward ratio: frames_of with the weight derivatives
RHO_ASSERT = min(8 * RHO_MEASURED, RHO_CEILING)
RHO_BWD_ASSERT = min(8 * RHO_BWD_MEASURED, RHO_CEILING)
CONVERGED, MAXIT, SCORE, FEW, SINGULAR, NONFINITE = range(6)
STATUS = ("CONVERGED", "MAXIT", "SCORE", "FEW", "SINGULAR", "NONFINITE")
WRONG_VARIANTS = ("no_x_dz", "fx_for_fy", "g_without_r", "no_t", "m_without_rr")
EDGE_S, EDGE_STEP, EDGE_MIN_SOFT, EDGE_CUT = 1e-10, 1e-6, 1e-6, 1e-9
DBL_EPSILON = 2.220446049250313e-16


class EdgeError(AssertionError):
    """A decision of the restated loop sits closer to its edge than the corpus conditions allow."""


def cell_terms(h, xyz, uv, cam, tau, beta, cut, variant=None):
    """r (P, 2), J (P, 2, 6), G (P, 2, 3), e (P,), w (P,) of every cell at the cv pose h; w = 0 exactly where e is not finite or e >= cut."""
    with np.errstate(all="ignore"):
        r, J, G = jacobians(h, xyz, uv, cam, variant)
        e = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        near = np.isfinite(e) & (e < cut)
        w = np.where(near, 1.0 / (1.0 + np.exp(-beta * (tau - np.where(near, e, 0.0)))), 0.0)
    return r, J, G, e, w


def _ld_gram(a, b):
    """a^T b with rows summed in long double (a (n, i), b (n, j) float64: the products are formed in long double too)."""
    return a.astype(np.longdouble).T @ b.astype(np.longdouble)


def soft_pass(h, xyz, uv, cam, tau, beta, cut):
    """S, A (6 x 6), g (6,) in long double, and the smallest distance of a finite residual from cut."""
    r, J, _, e, w = cell_terms(h, xyz, uv, cam, tau, beta, cut)
    live = np.flatnonzero(w > 0)
    fin = np.isfinite(e)
    edge = float(np.abs(e[fin] - cut).min()) if fin.any() else np.inf
    if not len(live):
        z = np.longdouble(0)
        return z, np.zeros((6, 6), np.longdouble), np.zeros(6, np.longdouble), edge
    wl = w[live].astype(np.longdouble)
    Jl = J[live].astype(np.longdouble).reshape(-1, 6)  # rows (p, u), (p, v)
    w2 = np.repeat(wl, 2)
    A = (Jl * w2[:, None]).T @ Jl
    g = (Jl * w2[:, None]).T @ r[live].astype(np.longdouble).reshape(-1)
    return wl.sum(), A, g, edge


def score(h, xyz, uv, cam, tau, beta, cut):
    """S(h) as float64 (0 for a non-finite pose)."""
    if not np.all(np.isfinite(h)):
        return 0.0
    return float(soft_pass(h, xyz, uv, cam, tau, beta, cut)[0])


def refine_soft(h0, xyz, uv, cam, tau, beta, cut, min_soft, max_iters, step_tol, strict=True):
    """The header's loop.  Returns dict(h, S, iters, status, cond: the largest cond(A) over the iterates, S0: S at the start pose).
    strict: raise EdgeError where a decision is closer to its edge than the corpus conditions allow."""
    h = np.asarray(h0, dtype=np.float64).copy()
    # the corpus builder has run most strict calls before expected() asks for them again: remembered by the data the arguments point at
    key = (xyz.ctypes.data, xyz.shape, uv.ctypes.data, tuple(float(c) for c in cam), h.tobytes(), tau, beta, cut, min_soft, max_iters, step_tol)
    if strict and key in _MEMO:
        return dict(_MEMO[key])
    r = _refine_soft(h, xyz, uv, cam, tau, beta, cut, min_soft, max_iters, step_tol, strict)
    if strict:
        _MEMO[key] = dict(r)
    return r


_MEMO = {}


def _refine_soft(h, xyz, uv, cam, tau, beta, cut, min_soft, max_iters, step_tol, strict):
    def edge(ok, what):
        if strict and not ok:
            raise EdgeError(what)

    if not np.all(np.isfinite(h)):
        return dict(h=h, S=0.0, iters=0, status=NONFINITE, cond=np.nan, S0=0.0)
    S, A, g, d_cut = soft_pass(h, xyz, uv, cam, tau, beta, cut)
    edge(d_cut >= EDGE_CUT, "a cell within 1e-9 px of cut")
    S = float(S)
    S0 = S
    edge(abs(S - min_soft) >= EDGE_MIN_SOFT, "S within 1e-6 of min_soft")
    if not S >= min_soft:
        return dict(h=h, S=S, iters=0, status=FEW, cond=np.nan, S0=S0)
    it, worst = 0, 0.0
    while True:
        A64 = A.astype(np.float64)
        c = float(np.linalg.cond(A64))
        edge(c <= COND_MAX, "cond(A) = %.3g" % c)
        worst = max(worst, c)
        if np.linalg.eigvalsh(A64).min() <= 0:
            return dict(h=h, S=S, iters=it, status=SINGULAR, cond=worst, S0=S0)
        delta = (inverse_ld(A) @ g).astype(np.float64)
        lim = step_tol * (float(np.sqrt(h @ h)) + DBL_EPSILON)
        nd = float(np.sqrt(delta @ delta))
        edge(lim == 0 or abs(nd / lim - 1) >= EDGE_STEP, "|delta| within 1e-6 of its limit")
        if nd <= lim:
            return dict(h=h, S=S, iters=it, status=CONVERGED, cond=worst, S0=S0)
        h2 = h - delta
        S2, A2, g2, d_cut = soft_pass(h2, xyz, uv, cam, tau, beta, cut)
        edge(d_cut >= EDGE_CUT, "a cell within 1e-9 px of cut")
        S2 = float(S2)
        edge(abs(S2 - S) >= EDGE_S * S, "S' within 1e-10 S of S")
        if not S2 >= S:
            return dict(h=h, S=S, iters=it, status=SCORE, cond=worst, S0=S0)
        h, S, A, g, it = h2, S2, A2, g2, it + 1
        if it >= max_iters:
            return dict(h=h, S=S, iters=it, status=MAXIT, cond=worst, S0=S0)


def irls_solve(h0, xyz, uv, cam, tau, beta, cut, iters=200, tol=1e-15):
    """Pure re-weighted Gauss-Newton, no accept test, iterated until the step is below tol |h| (the fixed point the backward linearises)."""
    h = np.asarray(h0, dtype=np.float64).copy()
    for _ in range(iters):
        _, A, g, _ = soft_pass(h, xyz, uv, cam, tau, beta, cut)
        d = (inverse_ld(A) @ g).astype(np.float64)
        h = h - d
        if np.linalg.norm(d) <= tol * np.linalg.norm(h):
            break
    return h


def backward(h, xyz, uv, cam, tau, beta, cut, min_soft, fixed=False, variant=None):
    """None where the problem has no result, else dict(cells: the cells with w > 0, J (n, 6, 3): T d h / d X_p of those cells, cond: cond(H))."""
    h = np.asarray(h, dtype=np.float64)
    if not np.all(np.isfinite(h)):
        return None
    r, J, G, e, w = cell_terms(h, xyz, uv, cam, tau, beta, cut, variant)
    live = np.flatnonzero(w > 0)
    if not len(live) or not float(w[live].astype(np.longdouble).sum()) >= min_soft:
        return None
    r, J, G, e, w = r[live], J[live], G[live], e[live], w[live]
    with np.errstate(all="ignore"):
        k = np.where(e > 0, -beta * w * (1.0 - w) / np.where(e > 0, e, 1.0), 0.0)
    if fixed or variant == "m_without_rr":
        k = np.zeros_like(k)
    M = (w[:, None, None] * np.eye(2)[None] + k[:, None, None] * r[:, :, None] * r[:, None, :]).astype(np.longdouble)  # (n, 2, 2)
    Jl, Gl = J.astype(np.longdouble), G.astype(np.longdouble)
    MJ = np.einsum("pkl,pla->pka", M, Jl)
    H = Jl.reshape(-1, 6).T @ MJ.reshape(-1, 6)
    H64 = H.astype(np.float64)
    if np.linalg.eigvalsh(0.5 * (H64 + H64.T)).min() <= 0:
        return None
    T = np.eye(6) if variant == "no_t" else cv_to_jp6_jacobian(h)
    TH = T.astype(np.longdouble) @ inverse_ld(H)
    MG = np.einsum("pkl,plc->pkc", M, Gl)
    JtMG = np.einsum("pka,pkc->pac", Jl, MG)
    Jobj = -np.einsum("ka,pac->pkc", TH, JtMG)
    return dict(cells=live.astype(np.int64), J=Jobj.astype(np.float64), cond=float(np.linalg.cond(H64)))


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call: the frame(s), the start poses and the call's parameters.  xyz (F, P, 3) float32; uv (P, 2) float32 shared by the frames or None (the implicit
    grid); cams (F, 4); poses (B, 6); frame_of (B,); give_frame_of: pass frame_of to the call (else the call's own mapping must give the same);
    fused: the fused form is run on this case as well."""

    def __init__(self, name, xyz, uv, H, W, cams, poses, frame_of, give_frame_of, tau=10.0, beta=0.5, cut=42.0, min_soft=50.0, max_iters=20, step_tol=1e-6, fused=True):
        self.name, self.xyz, self.uv, self.H, self.W = name, xyz, uv, H, W
        self.cams = np.asarray(cams, np.float32).reshape(-1, 4)
        self.poses, self.frame_of, self.give_frame_of = np.asarray(poses, np.float64), np.asarray(frame_of, np.int32), give_frame_of
        self.tau, self.beta, self.cut, self.min_soft, self.max_iters, self.step_tol, self.fused = tau, beta, cut, min_soft, max_iters, step_tol, fused
        self.F, self.P, self.B = xyz.shape[0], H * W, len(self.poses)

    def uv_of(self):
        return self.uv if self.uv is not None else grid_uv(self.H, self.W)

    def frame(self, b):
        f = int(self.frame_of[b])
        return self.xyz[f], self.uv_of(), self.cams[f]

    def forms(self):
        return (0, 1) if self.fused else (0,)


def expected(case, strict=True):
    """The restated loop on every problem: dict(h (B, 6), S, iters, status, cond, S0)."""
    rs = [refine_soft(case.poses[b], *case.frame(b), case.tau, case.beta, case.cut, case.min_soft, case.max_iters, case.step_tol, strict) for b in range(case.B)]
    return {k: np.array([r[k] for r in rs]) for k in ("h", "S", "iters", "status", "cond", "S0")}


def expected_backward(case, ref_poses, fixed=False, variant=None):
    """backward() of every problem at ref_poses (B, 6): a list of B dicts or None."""
    return [backward(ref_poses[b], *case.frame(b), case.tau, case.beta, case.cut, case.min_soft, fixed, variant) for b in range(case.B)]


def expected_grad(case, bwd, dL, coef, grad0, rho=None):
    """grad0 + sum_b coef[b] dL[b]^T J_b per cell (F, P, 3) in long double, the tolerance per entry and which cells are touched.  The tolerance is the Jacobian
    bound of every contributing problem on the sum of its absolute terms |coef dL_k J_ref[k][c]|, plus the roundings of the cell's own sum: one per added problem
    and one for the start value, each at most 2^-52 of the absolute sum, and one more for each term's final product."""
    rho = RHO_BWD_ASSERT if rho is None else rho
    g = grad0.astype(np.longdouble).copy()
    tol = np.zeros(grad0.shape)
    mag = np.abs(grad0).astype(np.float64)
    count = np.zeros(grad0.shape[:2])
    for b in range(case.B):
        if bwd[b] is None:
            continue
        f, L = int(case.frame_of[b]), bwd[b]["cells"]
        g[f][L] += (coef[b] * np.einsum("k,ikc->ic", dL[b], bwd[b]["J"])).astype(np.longdouble)
        terms = np.abs(coef[b]) * np.einsum("k,ikc->ic", np.abs(dL[b]), np.abs(bwd[b]["J"]))
        mag[f][L] += terms
        tol[f][L] += rho * bwd[b]["cond"] * EPS * terms
        count[f][L] += 1
    return g.astype(np.float64), tol + (2 * count[:, :, None] + 1) * EPS * mag, count > 0


def jacobian_ratio(J, J_ref, cond):
    return float(np.abs(J - J_ref).max() / (cond * EPS * np.abs(J_ref).max()))


def forward_ratios(h, S, exp, b):
    """(|h - h_ref|_inf, |S - S_ref|) over cond(A) 2^-52 max(1, |h_ref|_inf) and cond(A) 2^-52 S_ref: the figures RHO_MEASURED is the worst of."""
    c = exp["cond"][b]
    href = exp["h"][b]
    return (float(np.abs(h - href).max() / (c * EPS * max(1.0, np.abs(href).max()))), float(abs(S - exp["S"][b]) / (c * EPS * exp["S"][b])))


def _draw(rng, count, gt, xyz, uv, cam, rot_sigma, t_sigma, par, want=None):
    """`count` start poses around gt whose restated loop meets the corpus conditions (rejection sampling, deterministic); want: statuses to accept."""
    out = []
    for _ in range(100 * count):
        if len(out) == count:
            break
        h = gt + np.concatenate([rng.normal(scale=rot_sigma, size=3), rng.normal(scale=t_sigma, size=3)])
        try:
            r = refine_soft(h, xyz, uv, cam, **par)
        except EdgeError:
            continue
        if r["status"] in (FEW, SINGULAR) or (want is not None and r["status"] not in want):
            continue
        out.append(h)
    assert len(out) == count, "the corpus builder found %d of %d poses" % (len(out), count)
    return out


def _far_pose(rng, gt, xyz, uv, cam, par):
    for _ in range(200):
        h = gt + np.concatenate([rng.normal(scale=0.3, size=3), rng.normal(scale=300.0, size=3)])
        try:
            if refine_soft(h, xyz, uv, cam, **par)["status"] == FEW:
                return h
        except EdgeError:
            pass
    raise AssertionError("no far pose found")


SPREADS = ((0.004, 4.0), (0.03, 40.0))
_CORPUS = None


def _par(tau=10.0, beta=0.5, cut=42.0, min_soft=50.0, max_iters=20, step_tol=1e-6):
    return dict(tau=tau, beta=beta, cut=cut, min_soft=min_soft, max_iters=max_iters, step_tol=step_tol)


def corpus():
    """The cases, built once: dict name -> Case."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    C = {}
    rng = np.random.default_rng(20240917)

    def both_spreads(n, gt, xyz, uv, cam, par, want=None):
        return [h for rs, ts in SPREADS for h in _draw(rng, n, gt, xyz, uv, cam, rs, ts, par, want)]

    # (1) 40 x 40 with sampled pixel positions: three poses of each spread, a NaN pose (6) and a far pose (7); then the same frame stopped after 1 and 3
    # steps with cut = 100 and 25, and with a loose step_tol, which ends in CONVERGED
    fr = synth.chess_like_frame(40, 40, seed=44, outlier_frac=0.3)
    one = (fr["xyz"][None], fr["uv"], 40, 40, [fr["cam"]])
    args = (fr["gt_pose"], fr["xyz"], fr["uv"], fr["cam"])
    poses = both_spreads(3, *args, _par())
    nan = fr["gt_pose"].copy()
    nan[1] = np.nan
    poses += [nan, _far_pose(rng, *args, _par())]
    C["uv40"] = Case("uv40", *one, poses, np.zeros(len(poses), np.int32), False, **_par())
    for name, par in (("uv40_it1_cut100", _par(max_iters=1, cut=100.0)), ("uv40_it3_cut25", _par(max_iters=3, cut=25.0)), ("uv40_loose", _par(step_tol=2e-3))):
        want = (MAXIT,) if par["max_iters"] < 20 else (CONVERGED,)
        ps = both_spreads(2, *args, par, want)
        C[name] = Case(name, *one, ps, np.zeros(len(ps), np.int32), False, **par)
    C["b1"] = Case("b1", *one, poses[4:5], np.zeros(1, np.int32), False, **_par())
    # (2) 37 x 53 on the implicit grid: an odd cell count
    cam2 = (60.0, 60.0, 26.0, 18.0)
    fr2 = synth.chess_like_frame(37, 53, seed=41, cam=cam2, outlier_frac=0.3, grid_uv=True)
    ps = both_spreads(2, fr2["gt_pose"], fr2["xyz"], fr2["uv"], cam2, _par())
    C["grid37x53"] = Case("grid37x53", fr2["xyz"][None], None, 37, 53, [cam2], ps, np.zeros(len(ps), np.int32), False, **_par())
    # (3) 96 x 128: several chunks per problem in the split form
    fr3 = synth.chess_like_frame(96, 128, seed=43, outlier_frac=0.3)
    ps = both_spreads(1, fr3["gt_pose"], fr3["xyz"], fr3["uv"], fr3["cam"], _par())
    C["m96x128"] = Case("m96x128", fr3["xyz"][None], fr3["uv"], 96, 128, [fr3["cam"]], ps, np.zeros(len(ps), np.int32), False, **_par())
    # (4) three 40 x 40 frames with one camera each, fx != fy: B = 6 by the call's own mapping, B = 5 with frame_of = (2, 0, 0, 1, 2)
    cams3 = np.array([(525.0, 500.0, 320.0, 240.0), (480.0, 525.0, 300.0, 250.0), (560.0, 540.0, 330.0, 230.0)], np.float32)
    frs = [synth.chess_like_frame(40, 40, seed=(8, 35, 30)[f], cam=tuple(float(c) for c in cams3[f]), outlier_frac=0.3, stratified=False) for f in range(3)]
    xyz3 = np.stack([f["xyz"] for f in frs])
    uv3 = frs[0]["uv"]
    for name, fof, give in (("frames_b6", (0, 0, 1, 1, 2, 2), False), ("frames_of", (2, 0, 0, 1, 2), True)):
        ps = [_draw(rng, 1, frs[f]["gt_pose"], xyz3[f], uv3, cams3[f], *SPREADS[b % 2], _par())[0] for b, f in enumerate(fof)]
        C[name] = Case(name, xyz3, uv3, 40, 40, cams3, ps, np.array(fof, np.int32), give, **_par())
    # (5) 480 x 640, B = 4, three steps: the split form only
    fr5 = synth.chess_like_frame(480, 640, seed=1305, outlier_frac=0.3)
    par5 = _par(max_iters=3)
    ps = both_spreads(2, fr5["gt_pose"], fr5["xyz"], fr5["uv"], fr5["cam"], par5)
    C["big"] = Case("big", fr5["xyz"][None], fr5["uv"], 480, 640, [fr5["cam"]], ps, np.zeros(4, np.int32), False, fused=False, **par5)
    _CORPUS = C
    return C


SMALL_CASES = ("uv40", "uv40_it1_cut100", "uv40_it3_cut25", "uv40_loose", "b1", "grid37x53", "m96x128", "frames_b6", "frames_of")
ALL_CASES = SMALL_CASES + ("big",)
