"""numpy restatement of dsac_refine_gn_backward (include/dsac_hip.h has the definition) and the corpus its tests run on.

What is restated, in float64 unless said otherwise:
    walk           the first max_inl cells of a permutation row whose residual at the pose is below thr: the projection rounded to float32, the difference in
                   float32, the norm in double, clamped at 100, compared as float32 -- a NaN is below no threshold
    jacobians      r_p, J_p = d r_p / d h (2 x 6), G_p = d r_p / d X_p (2 x 3) at a cv pose; dR / d rho_j is written as [J_l(rho) e_j]x R, not as the derivative of
                   Rodrigues' formula term by term, so that the kernel's dR / d rho is checked against a second derivation
    A              sum of J_p^T J_p, accumulated and inverted in np.longdouble (Gaussian elimination with partial pivoting): the expected side's own error is
                   cond(A) * 2^-64 where long double is the x87 type, far below what the fp64 kernel can hold, so the measured margin is the kernel's
    T              d cv_to_jp6 / d cv6 = blockdiag(J_l(rho')^-1 D J_l(rho), D), D = diag(1, -1, -1)
    J_obj, grad    T (-A^-1 J_p^T G_p), and sum coef dL^T J_obj per cell

WRONG_VARIANTS are deliberate mistakes (one term each) that tests/test_refine_gn_ref_cpu.py shows to fail the GPU test's bound: the bound can see them.

The bound.  Both sides are deterministic fp64 evaluations of the same formulas; what separates them is rounding amplified by the solve, so per problem
    max |J - J_ref| <= RHO_ASSERT * cond(A_b) * 2^-52 * max |J_ref|
with RHO_ASSERT = 8 x the worst ratio measured on the MI355X over the corpus (profiles/refine_gn_margins.txt); the factor is for compiler changes.  The corpus
keeps cond(A) <= COND_MAX = 1.4e8, which holds the bound at or below 1e-6 relative for any RHO_ASSERT up to 32.  The measured ratio is 7e-7: the L D L^T solve
of these matrices is far from its worst case, kernel and restatement agree to about ten units in the last place, and the asserted bound is 2e-14 relative.
"""
import numpy as np


def _load_synth():
    """dsac_amd.synth, the frame generator: plain numpy.  The package refuses to import without its built library, and the CPU tests of the restatements must run
    without one: then the module is loaded from its file."""
    try:
        from dsac_amd import synth
        return synth
    except ImportError:
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsac_amd", "synth.py")
        spec = importlib.util.spec_from_file_location("dsac_amd_synth", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod


synth = _load_synth()

EPS = 2.0 ** -52
COND_MAX = 1.4e8
ANGLE_MIN, ANGLE_MAX = 0.05, np.pi - 0.1  # of the jp rotation vector
THR_MARGIN = 1e-3  # px: no corpus residual this close to its threshold (the float projection's ulp is 6e-5 px at 640 px)
RHO_MEASURED = 7.0e-7  # worst max|J - J_ref| / (cond(A) 2^-52 max|J_ref|) over the corpus on the MI355X (profiles/refine_gn_margins.txt)
RHO_ASSERT = 8 * RHO_MEASURED
WRONG_VARIANTS = ("no_x_dz", "fx_for_fy", "g_without_r", "no_t", "no_sign")


# ---- rotations ---------------------------------------------------------------------------------------------------------------------------------
def skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=np.float64)


def so3_left_jacobian(r, inverse=False):
    """J_l(r) = I + a [r]x + b [r]x^2, a = (1 - cos t) / t^2, b = (t - sin t) / t^3; inverse: I - [r]x / 2 + c [r]x^2, c = 1 / t^2 - cot(t / 2) / (2 t).
    Half-angle forms; below t = 0.1 the series of the differences that cancel (next term below 3e-16)."""
    r = np.asarray(r, dtype=np.float64)
    t2 = float(r @ r)
    K = skew(r)
    if t2 < 1e-2:
        a = 0.5 - t2 / 24 + t2 ** 2 / 720 - t2 ** 3 / 40320
        b = 1 / 6 - t2 / 120 + t2 ** 2 / 5040 - t2 ** 3 / 362880
        c = 1 / 12 + t2 / 720 + t2 ** 2 / 30240 + t2 ** 3 / 1209600
    else:
        t = np.sqrt(t2)
        sh, ch = np.sin(t / 2), np.cos(t / 2)
        a = 2 * sh * sh / t2
        b = (t - 2 * sh * ch) / (t2 * t)
        c = 1 / t2 - ch / (2 * t * sh)
    if inverse:
        return np.eye(3) - 0.5 * K + c * (K @ K)
    return np.eye(3) + a * K + b * (K @ K)


D3 = np.diag([1.0, -1.0, -1.0])


def cv_to_jp6_jacobian(h):
    """T = d cv_to_jp6 / d cv6 at the cv pose h (6 x 6)."""
    h = np.asarray(h, dtype=np.float64)
    jp = synth.cv_to_jp6(h)
    T = np.zeros((6, 6))
    T[:3, :3] = so3_left_jacobian(jp[:3], inverse=True) @ D3 @ so3_left_jacobian(h[:3])
    T[3:, 3:] = D3
    return T


def jp_angle(h):
    return float(np.linalg.norm(synth.cv_to_jp6(h)[:3]))


# ---- residuals and the walk -------------------------------------------------------------------------------------------------------------------
def grid_uv(H, W):
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.stack([u, v], -1).reshape(-1, 2)


def residuals_exact(h, xyz, uv, cam):
    """Reprojection distance of every cell in px, all in double (for the corpus' distance from the threshold)."""
    fx, fy, cx, cy = [float(c) for c in cam]
    Xc = xyz.astype(np.float64) @ synth.rodrigues(h[:3]).T + np.asarray(h[3:], dtype=np.float64)
    with np.errstate(all="ignore"):
        z = np.where(Xc[:, 2] != 0, 1.0 / Xc[:, 2], 1.0)
        du = Xc[:, 0] * z * fx + cx - uv[:, 0].astype(np.float64)
        dv = Xc[:, 1] * z * fy + cy - uv[:, 1].astype(np.float64)
        return np.sqrt(du * du + dv * dv)


def residuals_f(h, xyz, uv, cam):
    """K6's residual: the projection rounded to float32, the difference in float32, the norm in double, clamped at 100, as float32."""
    fx, fy, cx, cy = [float(c) for c in cam]
    Xc = xyz.astype(np.float64) @ synth.rodrigues(h[:3]).T + np.asarray(h[3:], dtype=np.float64)
    with np.errstate(all="ignore"):
        z = np.where(Xc[:, 2] != 0, 1.0 / Xc[:, 2], 1.0)
        u = (Xc[:, 0] * z * fx + cx).astype(np.float32)
        v = (Xc[:, 1] * z * fy + cy).astype(np.float32)
        dx = (uv[:, 0].astype(np.float32) - u).astype(np.float64)
        dy = (uv[:, 1].astype(np.float32) - v).astype(np.float64)
        d = np.sqrt(dx * dx + dy * dy)
        return np.where(100.0 < d, 100.0, d).astype(np.float32)


def walk(h, xyz, uv, cam, perm_row, thr, max_inl):
    """The first max_inl cells along perm_row with a residual below thr (float32 comparison; NaN is below nothing)."""
    if not np.all(np.isfinite(h)):
        return np.zeros(0, np.int32)
    e = residuals_f(h, xyz, uv, cam)[perm_row]
    with np.errstate(invalid="ignore"):
        hit = e < np.float32(thr)
    return np.asarray(perm_row, dtype=np.int32)[hit][:max_inl]


# ---- Jacobians --------------------------------------------------------------------------------------------------------------------------------
def jacobians(h, X, uv, cam, variant=None):
    """r (n, 2), J (n, 2, 6), G (n, 2, 3) of the correspondences (X, uv) at the cv pose h."""
    fx, fy, cx, cy = [float(c) for c in cam]
    if variant == "fx_for_fy":
        fy = fx
    h = np.asarray(h, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    R = synth.rodrigues(h[:3])
    Jl = so3_left_jacobian(h[:3])
    Xc = X @ R.T + h[3:]
    with np.errstate(divide="ignore"):
        z = np.where(Xc[:, 2] != 0, 1.0 / Xc[:, 2], 1.0)  # no depth rule: a cell on the camera plane is projected with z = 1, as in K2 and K6
    x, y = Xc[:, 0] * z, Xc[:, 1] * z
    tu, tv = fx * z, fy * z
    r = np.stack([x * fx + cx - uv[:, 0].astype(np.float64), y * fy + cy - uv[:, 1].astype(np.float64)], -1)
    n = len(X)
    J = np.zeros((n, 2, 6))
    for j in range(3):
        dXc = X @ (skew(Jl[:, j]) @ R).T  # (dR / d rho_j) X
        if variant == "no_x_dz":
            J[:, 0, j] = tu * dXc[:, 0]
        else:
            J[:, 0, j] = tu * (dXc[:, 0] - x * dXc[:, 2])
        J[:, 1, j] = tv * (dXc[:, 1] - y * dXc[:, 2])
    J[:, 0, 3], J[:, 0, 5] = tu, -tu * x
    J[:, 1, 4], J[:, 1, 5] = tv, -tv * y
    Rg = np.eye(3) if variant == "g_without_r" else R
    G = np.stack([tu[:, None] * (Rg[0][None, :] - x[:, None] * Rg[2][None, :]), tv[:, None] * (Rg[1][None, :] - y[:, None] * Rg[2][None, :])], 1)
    return r, J, G


def inverse_ld(A):
    """A^-1 in np.longdouble by Gauss-Jordan elimination with partial pivoting (np.linalg has no long double)."""
    n = A.shape[0]
    M = np.concatenate([A.astype(np.longdouble), np.eye(n, dtype=np.longdouble)], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return M[:, n:]


def normal_matrix(J):
    """A = sum J_p^T J_p (6 x 6, long double)."""
    Jl = J.astype(np.longdouble)
    return np.einsum("pka,pkb->ab", Jl, Jl)


def gn_jacobians(h, X, uv, cam, variant=None):
    """J_obj (n, 6, 3) of the correspondences (X, uv) at the cv pose h, and cond(A)."""
    _, J, G = jacobians(h, X, uv, cam, variant)
    A = normal_matrix(J)
    Ai = inverse_ld(A)
    T = np.eye(6) if variant == "no_t" else cv_to_jp6_jacobian(h)
    M = T.astype(np.longdouble) @ Ai
    sign = 1.0 if variant == "no_sign" else -1.0
    JtG = np.einsum("pka,pkc->pac", J, G).astype(np.longdouble)  # J_p^T G_p (n, 6, 3)
    Jobj = sign * np.einsum("ka,pac->pkc", M, JtG)
    return Jobj.astype(np.float64), float(np.linalg.cond(A.astype(np.float64)))


def gn_solve(h0, X, uv, cam, iters=50):
    """Gauss-Newton to convergence on the fixed correspondences (X, uv), from h0."""
    h = np.asarray(h0, dtype=np.float64).copy()
    for _ in range(iters):
        r, J, _ = jacobians(h, X, uv, cam)
        A = np.einsum("pka,pkb->ab", J, J)
        g = np.einsum("pka,pk->a", J, r)
        d = np.linalg.solve(A, g)
        h = h - d
        if np.linalg.norm(d) <= 1e-14 * np.linalg.norm(h):
            break
    return h


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call of dsac_refine_gn_backward: the frame(s), the problems and the call's parameters.
    xyz (F, P, 3) float32; uv (P, 2) float32 shared by the frames or None (the implicit grid); cams (F, 4) float32; poses (B, 6); frame_of (B,) the frame of every
    problem; give_frame_of: pass frame_of to the call (else the call's own mapping b // (B // F) must give the same); skip: problems not meant to be
    differentiated (their expected n_out is 0)."""

    def __init__(self, name, xyz, uv, H, W, cams, perm, poses, rows, frame_of, give_frame_of, max_inl, min_inl, thr, skip=()):
        self.name, self.xyz, self.uv, self.H, self.W, self.cams = name, xyz, uv, H, W, np.asarray(cams, np.float32).reshape(-1, 4)
        self.perm, self.poses, self.rows, self.frame_of, self.give_frame_of = perm, poses, rows, frame_of, give_frame_of
        self.max_inl, self.min_inl, self.thr, self.skip = max_inl, min_inl, thr, tuple(skip)
        self.F, self.P, self.B = xyz.shape[0], H * W, len(poses)

    def uv_of(self):
        return self.uv if self.uv is not None else grid_uv(self.H, self.W)

    def with_params(self, name, max_inl=None, min_inl=None, sel=None):
        sel = np.arange(self.B) if sel is None else np.asarray(sel)
        skip = tuple(int(np.flatnonzero(sel == s)[0]) for s in self.skip if s in sel)
        return Case(name, self.xyz, self.uv, self.H, self.W, self.cams, self.perm, self.poses[sel], self.rows[sel], self.frame_of[sel], self.give_frame_of,
                    self.max_inl if max_inl is None else max_inl, self.min_inl if min_inl is None else min_inl, self.thr, skip)


def expected(case, variant=None):
    """What the call must give: n (B,), cells (B, max_inl; -1 where nothing is written), J_obj (B, max_inl, 6, 3; NaN where nothing is written), cond (B,)."""
    B, mi = case.B, case.max_inl
    n = np.zeros(B, np.int32)
    cells = np.full((B, mi), -1, np.int32)
    J = np.full((B, mi, 6, 3), np.nan)
    cond = np.full(B, np.nan)
    uv = case.uv_of()
    for b in range(B):
        f = int(case.frame_of[b])
        L = walk(case.poses[b], case.xyz[f], uv, case.cams[f], case.perm[case.rows[b]], case.thr, mi)
        if len(L) < case.min_inl:
            continue
        n[b] = len(L)
        cells[b, :len(L)] = L
        J[b, :len(L)], cond[b] = gn_jacobians(case.poses[b], case.xyz[f][L], uv[L], case.cams[f], variant)
    return dict(n=n, cells=cells, J=J, cond=cond)


def expected_grad(case, exp, dL, coef, grad0, rho=RHO_ASSERT):
    """grad0 + sum coef dL^T J_obj per cell (F, P, 3), and the tolerance per entry: the Jacobian bound of every contributing problem on the sum of its absolute
    terms |coef dL_k J_ref[k][c]|, plus the roundings of the sum itself (4 x 2^-52 of the absolute sum, grad0 included: one per addition of a few terms)."""
    g = grad0.astype(np.longdouble).copy()
    tol = np.zeros(grad0.shape)
    mag = np.abs(grad0).astype(np.float64)
    for b in range(case.B):
        k = int(exp["n"][b])
        if not k:
            continue
        f, L = int(case.frame_of[b]), exp["cells"][b, :k]
        t = coef[b] * np.einsum("k,ikc->ic", dL[b], exp["J"][b, :k])
        np.add.at(g[f], L, t.astype(np.longdouble))
        terms = np.abs(coef[b]) * np.einsum("k,ikc->ic", np.abs(dL[b]), np.abs(exp["J"][b, :k]))
        np.add.at(mag[f], L, terms)
        np.add.at(tol[f], L, rho * exp["cond"][b] * EPS * terms)
    return g.astype(np.float64), tol + 4 * EPS * mag


def jacobian_ratio(J, J_ref, cond):
    """max |J - J_ref| / (cond 2^-52 max |J_ref|): the figure RHO_MEASURED is the corpus' worst case of."""
    return float(np.abs(J - J_ref).max() / (cond * EPS * np.abs(J_ref).max()))


def pose_ok(h, xyz, uv, cam, thr):
    """The corpus conditions every pose meets: no residual within THR_MARGIN of thr."""
    d = residuals_exact(h, xyz, uv, cam)
    return bool(np.all(np.abs(d[np.isfinite(d)] - thr) > THR_MARGIN))


def _draw_poses(rng, count, gt, xyz, uv, cam, perm, rows, thr, max_inls, min_inl, rot_sigma=0.004, t_sigma=4.0):
    """`count` poses around gt that meet the corpus conditions for every max_inl of max_inls on their row (rejection sampling, deterministic)."""
    out = []
    for _ in range(200 * count):
        if len(out) == count:
            break
        h = gt + np.concatenate([rng.normal(scale=rot_sigma, size=3), rng.normal(scale=t_sigma, size=3)])
        if not pose_ok(h, xyz, uv, cam, thr) or not (ANGLE_MIN <= jp_angle(h) <= ANGLE_MAX):
            continue
        row = perm[rows[len(out)]]
        good = True
        for mi in max_inls:
            L = walk(h, xyz, uv, cam, row, thr, mi)
            if len(L) < min_inl or gn_jacobians(h, xyz[L], uv[L], cam)[1] > COND_MAX:
                good = False
                break
        if good:
            out.append(h)
    assert len(out) == count, "the corpus builder found %d of %d poses" % (len(out), count)
    return np.array(out)


def _far_pose(rng, gt, xyz, uv, cam, perm_row, thr, min_inl):
    """A pose with fewer than min_inl cells below thr (and none within THR_MARGIN of it)."""
    for _ in range(200):
        h = gt + np.concatenate([rng.normal(scale=0.3, size=3), rng.normal(scale=300.0, size=3)])
        if pose_ok(h, xyz, uv, cam, thr) and len(walk(h, xyz, uv, cam, perm_row, thr, 256)) < min_inl:
            return h
    raise AssertionError("no far pose found")


MAX_INLS = (64, 65, 100, 128, 129, 256)
_CORPUS = None


def corpus():
    """The cases, built once: dict name -> Case."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    C = {}
    rng = np.random.default_rng(20240611)
    # (1) 40 x 40, sampled pixel positions, 70 problems on three permutation rows; problem 5 is a NaN pose, problem 9 has too few inliers.
    # The first four poses also meet the conditions for every max_inl of MAX_INLS
    fr = synth.chess_like_frame(40, 40, seed=44, outlier_frac=0.3)
    perm = synth.fast_permutations(1600, 3, seed=7)
    rows = (np.arange(70) % 3).astype(np.int32)
    p4 = _draw_poses(rng, 4, fr["gt_pose"], fr["xyz"], fr["uv"], fr["cam"], perm, rows[:4], 10.0, MAX_INLS, 50)
    p66 = _draw_poses(rng, 66, fr["gt_pose"], fr["xyz"], fr["uv"], fr["cam"], perm, rows[4:], 10.0, (100,), 50)
    poses = np.concatenate([p4, p66])
    poses[5] = fr["gt_pose"]
    poses[5, 1] = np.nan
    poses[9] = _far_pose(rng, fr["gt_pose"], fr["xyz"], fr["uv"], fr["cam"], perm[rows[9]], 10.0, 50)
    main = Case("b70", fr["xyz"][None], fr["uv"], 40, 40, [fr["cam"]], perm, poses, rows, np.zeros(70, np.int32), False, 100, 50, 10.0, skip=(5, 9))
    C["b70"] = main
    C["b1"] = main.with_params("b1", sel=[2])
    for mi in MAX_INLS:
        C["max_inl_%d" % mi] = main.with_params("max_inl_%d" % mi, max_inl=mi, sel=[0, 1, 2, 3])
    # two problems whose lists share cells (the same row, poses a fraction of a pixel apart) next to one on another row: the gradient's accumulation
    C["shared"] = main.with_params("shared", sel=[0, 3, 6, 1])
    # (2) 37 x 53 on the implicit grid, thr = 2: nine cells in ten are outliers, so the walk reaches the end of the 1 961-cell row with fewer than max_inl = 256
    cam2 = (60.0, 60.0, 26.0, 18.0)
    fr2 = synth.chess_like_frame(37, 53, seed=41, cam=cam2, outlier_frac=0.9, grid_uv=True)
    perm2 = synth.fast_permutations(1961, 2, seed=8)
    rows2 = np.array([1, 0], np.int32)
    uv2 = grid_uv(37, 53)
    assert np.array_equal(uv2, fr2["uv"])
    poses2 = _draw_poses(rng, 2, fr2["gt_pose"], fr2["xyz"], uv2, cam2, perm2, rows2, 2.0, (256,), 50, rot_sigma=0.002, t_sigma=2.0)
    C["short"] = Case("short", fr2["xyz"][None], None, 37, 53, [cam2], perm2, poses2, rows2, np.zeros(2, np.int32), False, 256, 50, 2.0)
    # (3) three 40 x 40 frames with one camera each, fx != fy, shared pixel positions: B = 6 by the call's own mapping, B = 5 with frame_of = (2, 0, 0, 1, 2)
    cams3 = np.array([(525.0, 500.0, 320.0, 240.0), (480.0, 525.0, 300.0, 250.0), (560.0, 540.0, 330.0, 230.0)], np.float32)
    frs = [synth.chess_like_frame(40, 40, seed=(8, 35, 30)[f], cam=tuple(float(c) for c in cams3[f]), outlier_frac=0.3, stratified=False) for f in range(3)]
    xyz3 = np.stack([f["xyz"] for f in frs])
    uv3 = frs[0]["uv"]
    perm3 = synth.fast_permutations(1600, 2, seed=9)
    for name, fof, give in (("frames_b6", (0, 0, 1, 1, 2, 2), False), ("frames_of", (2, 0, 0, 1, 2), True)):
        fof = np.array(fof, np.int32)
        rows3 = (np.arange(len(fof)) % 2).astype(np.int32)
        poses3 = np.concatenate([_draw_poses(rng, 1, frs[f]["gt_pose"], xyz3[f], uv3, cams3[f], perm3, rows3[b:b + 1], 10.0, (100,), 50) for b, f in enumerate(fof)])
        C[name] = Case(name, xyz3, uv3, 40, 40, cams3, perm3, poses3, rows3, fof, give, 100, 50, 10.0)
    _CORPUS = C
    return C


def check_corpus_conditions(case, exp):
    """The conditions of the module text, for one case and its expected values: returns the number of differentiated problems."""
    uv = case.uv_of()
    count = 0
    for b in range(case.B):
        f = int(case.frame_of[b])
        if not np.all(np.isfinite(case.poses[b])):
            assert b in case.skip
            continue
        assert pose_ok(case.poses[b], case.xyz[f], uv, case.cams[f], case.thr), (case.name, b)
        if b in case.skip:
            assert exp["n"][b] == 0, (case.name, b)
            continue
        assert exp["n"][b] >= case.min_inl, (case.name, b)
        assert exp["cond"][b] <= COND_MAX, (case.name, b, exp["cond"][b])
        assert ANGLE_MIN <= jp_angle(case.poses[b]) <= ANGLE_MAX, (case.name, b)
        assert RHO_ASSERT * exp["cond"][b] * EPS <= 1e-6, (case.name, b)
        count += 1
    return count
