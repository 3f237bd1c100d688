"""dsac_refine_soft and dsac_refine_soft_backward off the easy corpus of tests/refine_soft_ref.py: the postconditions of the header's definition, checked with numpy
alone whatever path the loop took, and the cases they run on -- start poses that the CPU oracle's P3P sampler drew (what processImageDSAC(refine="soft") hands
the refinement), full batches of 256 and 210 problems, maps with dead cells and cells on the camera plane, maps smaller than one 64-lane trip.

Problem classes.  A problem is DECIDED when refine_soft_ref.refine_soft(strict=True) raises no EdgeError: no decision of its loop sits on an edge and cond(A) stays
at or below COND_MAX.  Decided problems are compared with the restatement as tests/test_gpu_refine_soft.py does (status and steps equal, pose and S within
rho cond(A) 2^-52) and get the postconditions on top; undecided problems get the postconditions alone.

The pass tolerance.  tol(h) = pass_rel max(S_ref(h), 1) + near(h):
    pass_rel   64 x 2^-52, the constant the existing suite asserts for FEW problems, raised to 8 x the worst |S_64 - S_ref| / max(S_ref, 1) of a plain-float64 pass
               (the kernel's formulas, float64 products, np.sum) over the case's start and refined poses, measured on the CPU against the long double pass
    near(h)    sigmoid(beta (tau - cut)) for every cell the restatement finds within EDGE_CUT = 1e-9 px of cut: such a cell may fall on either side in the kernel
Where two passes meet in one inequality (S_ref(h_out) against S_ref(h0), S_ref(h') against S_ref(h_out)) one tolerance is granted, the larger of the two passes'.

rho for the new cases = min(RHO_CEILING, max(RHO_ASSERT, 8 x the worst ratio of the plain-float64 restatement of the whole loop against the long double one over the
case's decided problems)): the float64 loop is what any fp64 kernel of these formulas can be expected to hold, it is computed on the CPU, and no figure of the kernel
enters.  8 is the project's factor for compiler changes.  rho cond(A) 2^-52 bounds what the solve's rounding moves; on a problem whose cond(A) is small (7.96 on
dead_zero, where the bound would be 1e-20 relative) it is below one unit in the last place of S, which no fp64 sum over the cells holds.  The S bound of a decided
problem therefore has a floor, S_floor max(S_ref, 1) with S_floor = 8 x the larger of the case's CPU float64 pass ratio and 2^-53, one rounding of S itself (1.8e-15
for the sampled cases, 8.9e-16 for dead_zero, against the pass tolerance's 1.4e-14): the larger of the two bounds holds, never their sum.  With rho = 5.28e-6 the
floor is the larger one only below cond(A) = 1.5e6.

What the postconditions cannot see.  In SCORE the restated trial h' = h_out - delta is the kernel's up to the solve's rounding (cond(A) 2^-52 |delta|); S_ref(h') is
compared with the pass tolerance alone, which holds wherever S(h') is further below S(h_out) than the score moves over that distance -- every decided problem,
whose margin is 1e-10 S, and in practice every sampled one."""
import numpy as np

import refine_soft_ref as sr
from refine_gn_ref import grid_uv, inverse_ld, synth

PASS_FLOOR = 64 * sr.EPS
LOOP = (sr.CONVERGED, sr.MAXIT, sr.SCORE, sr.SINGULAR)
POST_VARIANTS = ("s_at_trial", "accept_fall", "iters_plus_one", "loose_converged", "few_moved")  # + "dead_as_one", which needs dead cells


def par_of(case):
    return dict(tau=case.tau, beta=case.beta, cut=case.cut, min_soft=case.min_soft, max_iters=case.max_iters, step_tol=case.step_tol)


def problem(case, b):
    """One problem of a case: dict(h0, xyz, uv, cam, tau, beta, cut, min_soft, max_iters, step_tol)."""
    xyz, uv, cam = case.frame(b)
    return dict(h0=case.poses[b], xyz=xyz, uv=uv, cam=cam, **par_of(case))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def pass_at(h, pr, plain=False, dead_as_one=False):
    """The pass at h: dict(S float, A (6, 6), g (6,), near).  Long double sums (plain: float64 products and np.sum).  A non-finite pose gives every cell a
    non-finite residual, so all sums are zero.  dead_as_one: the wrong kernel that counts a cell whose residual is not a number with weight 1."""
    z = np.float64 if plain else np.longdouble
    if not np.all(np.isfinite(h)):
        return dict(S=0.0, A=np.zeros((6, 6), z), g=np.zeros(6, z), near=0.0)
    r, J, _, e, w = sr.cell_terms(h, pr["xyz"], pr["uv"], pr["cam"], pr["tau"], pr["beta"], pr["cut"])
    fin = np.isfinite(e)
    near = float(np.count_nonzero(np.abs(e[fin] - pr["cut"]) < sr.EDGE_CUT)) * float(_sigmoid(pr["beta"] * (pr["tau"] - pr["cut"])))
    live = np.flatnonzero(w > 0)
    extra = float(np.count_nonzero(np.isnan(e))) if dead_as_one else 0.0
    if not len(live):
        return dict(S=extra, A=np.zeros((6, 6), z), g=np.zeros(6, z), near=near)
    Jl, rl, w2 = J[live].reshape(-1, 6), r[live].reshape(-1), np.repeat(w[live], 2)
    if plain:
        S = float(np.sum(w[live]))
        A = np.sum((w2[:, None] * Jl)[:, :, None] * Jl[:, None, :], axis=0)
        g = np.sum((w2 * rl)[:, None] * Jl, axis=0)
    else:
        Jl, rl, w2 = Jl.astype(z), rl.astype(z), w2.astype(z)
        S = float(w[live].astype(z).sum())
        A = (Jl * w2[:, None]).T @ Jl
        g = (Jl * w2[:, None]).T @ rl
    return dict(S=S + extra, A=A, g=g, near=near)


def _ldlt_solve64(A, g):
    """A^-1 g by an L D L^T factorisation without pivoting in float64, or None at a non-positive pivot: the plain-float64 restatement's solve."""
    n = 6
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        D[j] = A[j, j] - float(np.sum(L[j, :j] * L[j, :j] * D[:j]))
        if not D[j] > 0:
            return None
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - float(np.sum(L[i, :j] * L[j, :j] * D[:j]))) / D[j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = g[i] - float(np.sum(L[i, :i] * y[:i]))
    y = y / D
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - float(np.sum(L[i + 1:, i] * x[i + 1:]))
    return x


def step_at(P, plain=False):
    """delta = A^-1 g of a pass (float64), cond(A), and whether A is positive definite in float64."""
    A64 = np.asarray(P["A"], np.float64)
    if not np.all(np.isfinite(A64)):
        return None, np.inf, False
    with np.errstate(all="ignore"):
        c = float(np.linalg.cond(A64))
        pd = bool(np.linalg.eigvalsh(A64).min() > 0)
    if plain:
        d = _ldlt_solve64(A64, np.asarray(P["g"], np.float64))
        return d, c, d is not None
    if not pd:
        return None, c, False
    with np.errstate(all="ignore"):
        return (inverse_ld(P["A"]) @ P["g"]).astype(np.float64), c, True


def run_loop(pr, plain=False, variant=None):
    """The header's loop without the corpus conditions: the long double restatement (the results of refine_soft_ref.refine_soft(strict=False)), the plain-float64
    restatement (plain), or a wrong kernel (variant, one of POST_VARIANTS or "dead_as_one").  dict(h, S, iters, status, cond, S0)."""
    h = np.asarray(pr["h0"], np.float64).copy()
    dead = variant == "dead_as_one"
    step_tol = pr["step_tol"] * (10.0 if variant == "loose_converged" else 1.0)
    plus = 1 if variant == "iters_plus_one" else 0
    if not np.all(np.isfinite(h)):
        return dict(h=h, S=0.0, iters=0, status=sr.NONFINITE, cond=np.nan, S0=0.0)
    P = pass_at(h, pr, plain, dead)
    S = S0 = P["S"]
    if not S >= pr["min_soft"]:
        if variant == "few_moved":
            h = h * (1.0 + 2.0 ** -40)
        return dict(h=h, S=S, iters=0, status=sr.FEW, cond=np.nan, S0=S0)
    it, worst = 0, 0.0
    while True:
        d, c, pd = step_at(P, plain)
        worst = max(worst, c)
        if not pd:
            return dict(h=h, S=S, iters=it + plus, status=sr.SINGULAR, cond=worst, S0=S0)
        if float(np.sqrt(d @ d)) <= step_tol * (float(np.sqrt(h @ h)) + sr.DBL_EPSILON):
            return dict(h=h, S=S, iters=it + plus, status=sr.CONVERGED, cond=worst, S0=S0)
        h2 = h - d
        P2 = pass_at(h2, pr, plain, dead)
        if not P2["S"] >= S:
            if variant == "s_at_trial":
                return dict(h=h, S=P2["S"], iters=it + plus, status=sr.SCORE, cond=worst, S0=S0)
            if variant == "accept_fall":  # the falling step is taken before the loop ends
                return dict(h=h2, S=P2["S"], iters=it + 1, status=sr.SCORE, cond=worst, S0=S0)
            return dict(h=h, S=S, iters=it + plus, status=sr.SCORE, cond=worst, S0=S0)
        h, S, P, it = h2, P2["S"], P2, it + 1
        if it >= pr["max_iters"]:
            return dict(h=h, S=S, iters=it + plus, status=sr.MAXIT, cond=worst, S0=S0)


def cached_pass(pr, h, cache):
    """pass_at(h, pr) in long double, remembered in `cache` by the frame's data, the camera, cut and the pose's bits."""
    h = np.asarray(h, np.float64)
    k = (pr["xyz"].ctypes.data, tuple(float(c) for c in pr["cam"]), pr["tau"], pr["beta"], pr["cut"], h.tobytes())
    if k not in cache:
        cache[k] = pass_at(h, pr)
    return cache[k]


def postconditions(pr, h_out, S_out, iters, status, pass_rel=PASS_FLOOR, cache=None):
    """What the header of dsac_refine_soft guarantees for one problem whatever path the loop took, checked on the restated long double pass at the poses the
    call returned.  Returns the list of violated conditions (empty: accepted).  cache: a dict that keeps the passes by pose between calls (the start pose is
    shared by the two forms of the loop)."""
    bad = []
    h0 = np.asarray(pr["h0"], np.float64)
    h_out = np.asarray(h_out, np.float64)
    status, iters, S_out = int(status), int(iters), float(S_out)
    cache = {} if cache is None else cache

    def ref(h):
        return cached_pass(pr, h, cache)

    def tol(P):
        return pass_rel * max(P["S"], 1.0) + P["near"]

    if not 0 <= status <= 5:
        return ["status %d outside 0 .. 5" % status]
    if not 0 <= iters <= pr["max_iters"]:
        bad.append("iters %d outside 0 .. max_iters" % iters)
    if (status == sr.MAXIT) != (iters == pr["max_iters"]):
        bad.append("%s with iters %d of %d" % (sr.STATUS[status], iters, pr["max_iters"]))
    nonfinite = not np.all(np.isfinite(h0))
    if (status == sr.NONFINITE) != nonfinite:
        bad.append("NONFINITE must hold exactly for a non-finite start pose")
    same = h_out.tobytes() == h0.tobytes()
    if status in (sr.NONFINITE, sr.FEW) and not (same and iters == 0):
        bad.append("%s: the start pose must come back bit for bit with iters 0" % sr.STATUS[status])
    if status == sr.NONFINITE:
        if S_out != 0:
            bad.append("NONFINITE with S %r" % S_out)
        return bad
    if nonfinite:
        return bad
    if pr["step_tol"] >= 2.0 ** -40 and (iters == 0) != same:  # an accepted step is longer than step_tol |h|: it moves the pose
        bad.append("iters %d but the pose %s" % (iters, "did not move" if same else "moved"))
    P0, Po = ref(h0), ref(h_out)
    if not abs(S_out - Po["S"]) <= tol(Po):
        bad.append("S_out %.17g is not S_ref(h_out) %.17g within %.3g" % (S_out, Po["S"], tol(Po)))
    if not Po["S"] >= P0["S"] - max(tol(P0), tol(Po)):
        bad.append("S_ref(h_out) %.17g below S_ref(h0) %.17g" % (Po["S"], P0["S"]))
    if status == sr.FEW:
        if not P0["S"] < pr["min_soft"] + tol(P0):
            bad.append("FEW with S_ref(h0) %.17g, min_soft %g" % (P0["S"], pr["min_soft"]))
        return bad
    if not P0["S"] >= pr["min_soft"] - tol(P0):
        bad.append("%s with S_ref(h0) %.17g below min_soft %g" % (sr.STATUS[status], P0["S"], pr["min_soft"]))
    if status == sr.MAXIT:
        return bad
    d, c, pd = step_at(Po)
    if status == sr.SINGULAR:
        if not c > sr.COND_MAX:
            bad.append("SINGULAR with cond(A_ref(h_out)) %.3g" % c)
        return bad
    if not pd:  # the restated step does not exist: cond(A) 2^-52 is of order one, nothing more can be said
        if not c > sr.COND_MAX:
            bad.append("A_ref(h_out) is not positive definite at cond %.3g" % c)
        return bad
    if status == sr.CONVERGED:
        lim = pr["step_tol"] * (float(np.sqrt(h_out @ h_out)) + sr.DBL_EPSILON) * (1.0 + sr.RHO_ASSERT * c * sr.EPS)
        nd = float(np.sqrt(d @ d))
        if not nd <= lim:
            bad.append("CONVERGED with |delta| %.6g above %.6g" % (nd, lim))
    else:  # SCORE
        P2 = ref(h_out - d)
        if not P2["S"] < Po["S"] + max(tol(Po), tol(P2)):
            bad.append("SCORE but S_ref(h') %.17g is not below S_ref(h_out) %.17g" % (P2["S"], Po["S"]))
    return bad


# ---- expected values ---------------------------------------------------------------------------------------------------------------------------
_EXP = {}


def expected(case):
    """The restated loop on every problem, strict where that raises no EdgeError: dict(h, S, iters, status, cond, S0, decided (B,) bool).  Built once per case."""
    if case.name in _EXP:
        return _EXP[case.name]
    rs, decided = [], []
    for b in range(case.B):
        args = (case.poses[b],) + case.frame(b) + (case.tau, case.beta, case.cut, case.min_soft, case.max_iters, case.step_tol)
        try:
            rs.append(sr.refine_soft(*args, strict=True))
            decided.append(True)
        except sr.EdgeError:
            rs.append(run_loop(problem(case, b)))
            decided.append(False)
    out = {k: np.array([r[k] for r in rs]) for k in ("h", "S", "iters", "status", "cond", "S0")}
    out["decided"] = np.array(decided)
    _EXP[case.name] = out
    return out


_F64 = {}


def float64_figures(case):
    """The plain-float64 restatement against the long double one, on the CPU: dict(pass_rel: the case's pass tolerance factor, S_floor: the floor of the S bound of
    decided problems (module text), pass_ratio: the worst
    |S_64 - S_ref| / max(S_ref, 1) behind it, rho: the case's rho, ratio_h, ratio_S: the worst forward ratios of the float64 loop over the decided problems,
    flips: decided problems on which the float64 loop decides differently)."""
    if case.name in _F64:
        return _F64[case.name]
    exp = expected(case)
    worst_pass = worst_h = worst_S = 0.0
    flips = 0
    for b in range(case.B):
        pr = problem(case, b)
        for h in (case.poses[b], exp["h"][b]):
            if np.all(np.isfinite(h)):
                ld = pass_at(h, pr)["S"]
                worst_pass = max(worst_pass, abs(pass_at(h, pr, plain=True)["S"] - ld) / max(ld, 1.0))
        if exp["decided"][b] and exp["status"][b] in (sr.CONVERGED, sr.MAXIT, sr.SCORE):
            r = run_loop(pr, plain=True)
            if r["status"] != exp["status"][b] or r["iters"] != exp["iters"][b]:
                flips += 1
                continue
            rh, rS = sr.forward_ratios(r["h"], r["S"], exp, b)
            worst_h, worst_S = max(worst_h, rh), max(worst_S, rS)
    out = dict(pass_ratio=worst_pass, pass_rel=max(PASS_FLOOR, 8 * worst_pass), S_floor=8 * max(worst_pass, 2.0 ** -53), ratio_h=worst_h, ratio_S=worst_S, flips=flips,
               rho=min(sr.RHO_CEILING, max(sr.RHO_ASSERT, 8 * max(worst_h, worst_S))))
    _F64[case.name] = out
    return out


_SEL = {}


def backward_selection(case, exp, fixed):
    """Built once per case and flag: see _backward_selection."""
    if (case.name, fixed) not in _SEL:
        _SEL[(case.name, fixed)] = _backward_selection(case, exp, fixed)
    return _SEL[(case.name, fixed)]


def _backward_selection(case, exp, fixed):
    """The problems of a case that its backward test keeps, with the restated backward of each (None: no result) at the restated refined poses.  Kept: problems
    without a result because the pose is not finite or S < min_soft (FEW), and problems whose restated H is positive definite with cond(H) <= COND_MAX.  Left out:
    every other problem, and one whose pass at the refined pose sits on an edge (S within 1e-6 of min_soft, a cell within 1e-9 px of cut: ok_out or a cell's
    weight could fall either way).  The refined poses of the kept problems 7 and 37 are then given a NaN entry, so that every case has records without a result
    in its first and in its second scatter tile, whatever its statuses.  Returns (sel, ref (len(sel), 6), bwd)."""
    sel, bwd = [], []
    for b in range(case.B):
        h = exp["h"][b]
        if not np.all(np.isfinite(h)):
            sel.append(b)
            bwd.append(None)
            continue
        P = pass_at(h, problem(case, b))
        if P["near"] > 0 or abs(P["S"] - case.min_soft) < sr.EDGE_MIN_SOFT:
            continue
        r = sr.backward(h, *case.frame(b), case.tau, case.beta, case.cut, case.min_soft, fixed)
        if not P["S"] >= case.min_soft:
            assert r is None
            sel.append(b)
            bwd.append(None)
        elif r is not None and r["cond"] <= sr.COND_MAX:
            sel.append(b)
            bwd.append(r)
    sel = np.array(sel)
    ref = exp["h"][sel].copy()
    for i in (7, 37):
        if i < len(sel):
            ref[i, i % 6] = np.nan
            bwd[i] = None
    return sel, ref, bwd


def subcase(case, sel, name=None, frame_of=None, give=None):
    sel = np.asarray(sel)
    return sr.Case(name or case.name + "_sel", case.xyz, case.uv, case.H, case.W, case.cams, case.poses[sel], case.frame_of[sel] if frame_of is None else frame_of,
                   case.give_frame_of if give is None else give, **par_of(case))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
CAMS3 = np.array([(525.0, 500.0, 320.0, 240.0), (480.0, 525.0, 300.0, 250.0), (560.0, 540.0, 330.0, 230.0)], np.float32)  # the cameras of frames_b6
TINY = ((3, 5), (15, 17), (16, 16), (1, 257))
SAMPLED = ("sampled44", "sampled45")
N_DEAD_POSES, N_NAN, N_INF, N_PLANE = 40, 16, 8, 8
_CASES = None


def grid_cam(H, W):
    """The camera scaled to the map, as tests/dpnp_corpus.py scales it."""
    return (525.0 * W / 640, 525.0 * W / 640, W / 2.0, H / 2.0)


def _sample(orc, n, seed, xyz, uv, H, W, cam):
    return orc.sample(n, seed, xyz, uv, H, W, cam, thr=10.0, max_tries=4096)[0]


def cases():
    """The cases, built once: dict name -> Case.  The start poses come from the CPU oracle's sampler."""
    global _CASES
    if _CASES is not None:
        return _CASES
    from oracle import oracle as orc
    orc.build()
    C = {}
    # (1) the pipeline's own size: 256 P3P hypotheses on one 40 x 40 frame, at 30 % and 60 % outliers
    frames = {}
    for name, seed, frac in (("sampled44", 44, 0.3), ("sampled45", 45, 0.6)):
        fr = frames[name] = synth.chess_like_frame(40, 40, seed=seed, outlier_frac=frac)
        poses = _sample(orc, 256, 1305, fr["xyz"], fr["uv"], 40, 40, fr["cam"])
        C[name] = sr.Case(name, fr["xyz"][None], fr["uv"], 40, 40, [fr["cam"]], poses, np.zeros(256, np.int32), False)
    # (2) three frames with one camera each, 70 sampled poses per frame = two scatter tiles + 6: the call's own mapping, and a shuffled frame_of with
    # 70 problems of frame 0, 30 of frame 2 and none of frame 1
    frs = [synth.chess_like_frame(40, 40, seed=(8, 35, 30)[f], cam=tuple(float(c) for c in CAMS3[f]), outlier_frac=0.3, stratified=False) for f in range(3)]
    xyz3, uv3 = np.stack([f["xyz"] for f in frs]), frs[0]["uv"]
    poses = np.concatenate([_sample(orc, 70, 1305 + f, xyz3[f], uv3, 40, 40, CAMS3[f]) for f in range(3)])
    fof = np.repeat(np.arange(3, dtype=np.int32), 70)
    C["sampled_frames"] = sr.Case("sampled_frames", xyz3, uv3, 40, 40, CAMS3, poses, fof, False)
    pick = np.random.default_rng(20241020).permutation(np.concatenate([np.arange(70), 140 + np.arange(30)]))
    C["sampled_frames_of"] = sr.Case("sampled_frames_of", xyz3, uv3, 40, 40, CAMS3, poses[pick], fof[pick], True)
    # (3) dead cells: sampled44's frame with 16 NaN cells, 8 infinite cells and 8 cells with X_z = 0; 40 of sampled44's decided poses and an exactly-zero
    # pose, for which the 8 cells lie on the camera plane and are live under the z = 1 rule (residual 0.25 .. 2 px).  dead_zero: that pose alone at min_soft = 1
    fr = frames["sampled44"]
    e44 = expected(C["sampled44"])
    good = np.flatnonzero(e44["decided"] & np.isin(e44["status"], (sr.CONVERGED, sr.MAXIT, sr.SCORE)))
    sel = good[np.linspace(0, len(good) - 1, N_DEAD_POSES).astype(int)]
    cells = np.random.default_rng(20241021).permutation(1600)[:N_NAN + N_INF + N_PLANE]
    xyz = fr["xyz"].copy()
    xyz[cells[:N_NAN], np.arange(N_NAN) % 3] = np.nan
    xyz[cells[:4]] = np.nan
    xyz[cells[N_NAN:N_NAN + N_INF], np.arange(N_INF) % 3] = np.where(np.arange(N_INF) % 2, np.inf, -np.inf)
    xyz[cells[N_NAN + 4:N_NAN + N_INF]] = np.inf
    plane = cells[N_NAN + N_INF:]
    fx, fy, cx, cy = fr["cam"]
    off = 0.25 * (1 + np.arange(N_PLANE))
    xyz[plane, 0] = (fr["uv"][plane, 0] - cx + off) / fx
    xyz[plane, 1] = (fr["uv"][plane, 1] - cy) / fy
    xyz[plane, 2] = 0.0
    xyz = xyz.astype(np.float32)
    poses = np.concatenate([C["sampled44"].poses[sel], np.zeros((1, 6))])
    C["dead_cells"] = sr.Case("dead_cells", xyz[None], fr["uv"], 40, 40, [fr["cam"]], poses, np.zeros(len(poses), np.int32), False)
    C["dead_cells"].cells = dict(nan=cells[:N_NAN], inf=cells[N_NAN:N_NAN + N_INF], plane=plane)
    C["dead_zero"] = sr.Case("dead_zero", xyz[None], fr["uv"], 40, 40, [fr["cam"]], np.zeros((1, 6)), np.zeros(1, np.int32), False, **sr._par(min_soft=1.0))
    # (4) maps below one 64-lane trip, one cell below and exactly at refine_soft_geom's first boundary of 256 cells, and one row of 257: the implicit grid, the
    # camera scaled to the map, min_soft = cells / 32 (50 on 1 600 cells); four noise poses (two of each spread) and four sampled ones
    rng = np.random.default_rng(20241022)
    for H, W in TINY:
        cam = grid_cam(H, W)
        fr = synth.chess_like_frame(H, W, seed=46, cam=cam, outlier_frac=0.3, grid_uv=True)
        assert np.array_equal(fr["uv"], grid_uv(H, W))
        noise = [fr["gt_pose"] + np.concatenate([rng.normal(scale=rs, size=3), rng.normal(scale=ts, size=3)]) for rs, ts in sr.SPREADS for _ in range(2)]
        poses = np.concatenate([np.array(noise), _sample(orc, 4, 1305, fr["xyz"], fr["uv"], H, W, cam)])
        name = "tiny%dx%d" % (H, W)
        C[name] = sr.Case(name, fr["xyz"][None], None, H, W, [cam], poses, np.zeros(8, np.int32), False, **sr._par(min_soft=H * W / 32.0))
    # (5) DSAC_SOFT_SINGULAR: a 3 x 5 map with one finite cell, X = (0, 0, 1000), min_soft = 0.5.  A is a sum over one cell and has rank 2.  At the zero pose R = I
    # and dR / d rho are exact, the cell sits on the optical axis (x = y = 0), and row and column 2 of A (the rotation about the axis) are exact zeros: the third
    # pivot of the L D L^T factorisation is 0 - 0 - 0 whatever the rounding, so the status is SINGULAR in any fp64 evaluation.  The seven other poses (translated,
    # then rotated) leave the deficient pivots to rounding: postconditions only
    cam = grid_cam(3, 5)
    xyz = np.full((15, 3), np.nan, np.float32)
    xyz[7] = (0.0, 0.0, 1000.0)
    poses = np.zeros((8, 6))
    poses[1:4, 3:] = ((50.0, 0.0, 0.0), (0.0, -30.0, 20.0), (10.0, 10.0, -100.0))
    poses[4:] = rng.normal(size=(4, 6)) * np.array([0.01, 0.01, 0.01, 20.0, 20.0, 20.0])
    C["one_live3x5"] = sr.Case("one_live3x5", xyz[None], None, 3, 5, [cam], poses, np.zeros(8, np.int32), False, **sr._par(min_soft=0.5))
    _CASES = C
    return C


TINY_CASES = tuple("tiny%dx%d" % hw for hw in TINY)
FORWARD_CASES = SAMPLED + ("sampled_frames", "sampled_frames_of", "dead_cells", "dead_zero") + TINY_CASES + ("one_live3x5",)
BACKWARD_CASES = SAMPLED + ("sampled_frames", "sampled_frames_of", "dead_cells")
