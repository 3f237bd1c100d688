"""numpy / Python-integer restatement of the RGB-D calls (include/dsac_hip.h, "RGB-D localisation"): the reference the RGB-D tests compare the library with.

    valid_cells / canonical   the VALID rule, the canonical copy (NaN in every cell that is not VALID) and the counts n_f
    attempt_set               the candidate walk of one attempt, with Python integers
    kabsch3                   the three-point pose by an SVD Kabsch in float64
    accept3                   the acceptance rule on a pose (finite, three residuals below thr)
    walk                      the sampling loop of one frame, with each attempt's acceptance and pose supplied by the caller (the library's own given-sets path
                              in the bit-for-bit tests, kabsch3 + accept3 in the CPU tests)
    distances / soft_sums     float64 distances and soft-inlier sums
    score_bound               the per-pair bound of dsac_score_rgbd
    refine                    the refinement loop with sums and the eigen-solve in np.longdouble
    refine_f64                the same loop in plain float64 from the kernels' 16 sums, about the first VALID cell or about the origin
    score_case / refine_case / refine_corpus / late_first_case / far_origin_case   the corpora the CPU and GPU tests share
No GPU, no library call."""
import numpy as np

M64 = (1 << 64) - 1
STATUS = ("CONVERGED", "MAXIT", "SCORE", "FEW", "SINGULAR", "NONFINITE")


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hyp_key(seed, h):
    return mix64((seed & M64) ^ mix64(h))


def draw_cell(key, a, k, W, H):
    v = mix64((key + ((a << 16) | k)) & M64)
    x = ((v >> 32) * W) >> 32
    y = ((v & 0xFFFFFFFF) * H) >> 32
    return y * W + x


def valid_cells(xyz, cam_xyz):
    """xyz, cam_xyz: (..., P, 3) float32 -> bool (..., P)"""
    xyz, cam_xyz = np.asarray(xyz, np.float32), np.asarray(cam_xyz, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(cam_xyz).all(-1) & (cam_xyz[..., 2] > 0) & np.isfinite(xyz).all(-1)


def canonical(xyz, cam_xyz):
    """the context's copy and the VALID counts per frame: (F, P, 3) float32 with NaN in every cell that is not VALID, (F,) int"""
    cam = np.array(cam_xyz, np.float32, copy=True)
    v = valid_cells(xyz, cam)
    cam[~v] = np.nan
    return cam, v.reshape(v.shape[0] if v.ndim > 1 else 1, -1).sum(-1)


def attempt_set(key, a, W, H, valid):
    """the three cells of attempt a, or None when 32 candidates do not give three"""
    got = []
    for k in range(32):
        c = draw_cell(key, a, k, W, H)
        if valid[c] and c not in got:
            got.append(c)
            if len(got) == 3:
                return got
    return None


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 2.220446049250313e-16:
        return np.eye(3)
    a = r / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(a, a) + np.sin(th) * K


def rodrigues_inv(R):
    """rotation matrix -> Rodrigues vector (angles away from pi)"""
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v) / 2
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arctan2(s, c)
    if s < 1e-12:
        return np.zeros(3)
    return v / (2 * s) * th


def kabsch(X, C, w=None, dtype=np.float64):
    """weighted rigid alignment C ~= R X + t by SVD; returns R, t"""
    X, C = np.asarray(X, dtype), np.asarray(C, dtype)
    w = np.ones(len(X), dtype) if w is None else np.asarray(w, dtype)
    S = w.sum()
    xm, cm = (w[:, None] * X).sum(0) / S, (w[:, None] * C).sum(0) / S
    K = ((w[:, None] * (X - xm)).T @ (C - cm)).astype(np.float64)
    U, _, Vt = np.linalg.svd(K)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, np.asarray(cm, np.float64) - R @ np.asarray(xm, np.float64)


def kabsch3(xyz, cam, cells):
    """the pose of a minimal set: cv 6-vector, R, t"""
    X, C = np.asarray(xyz, np.float64)[list(cells)], np.asarray(cam, np.float64)[list(cells)]
    R, t = kabsch(X, C)
    return np.concatenate([rodrigues_inv(R), t]), R, t


def residuals3(xyz, cam, cells, R, t):
    X, C = np.asarray(xyz, np.float64)[list(cells)], np.asarray(cam, np.float64)[list(cells)]
    return np.linalg.norm(X @ R.T + t - C, axis=1)


def accept3(pose, res, thr):
    return bool(np.isfinite(pose).all() and (res < thr).all())


def triangle_quality(P3):
    """smallest angle (degrees) and smallest side of a triangle of three points"""
    P3 = np.asarray(P3, np.float64)
    a, b, c = (np.linalg.norm(P3[1] - P3[2]), np.linalg.norm(P3[0] - P3[2]), np.linalg.norm(P3[0] - P3[1]))
    side = min(a, b, c)
    if side == 0:
        return 0.0, 0.0
    angs = []
    for (x, y, z) in ((a, b, c), (b, c, a), (c, a, b)):
        angs.append(np.degrees(np.arccos(np.clip((y * y + z * z - x * x) / (2 * y * z), -1, 1))))
    return min(angs), side


def attempt_sets(N, seed, W, H, valid, max_tries):
    """sets[h][a] (list of 3 cells or None) for every attempt of every hypothesis of one frame"""
    out = []
    for h in range(N):
        key = hyp_key(seed, h)
        out.append([attempt_set(key, a, W, H, valid) for a in range(max_tries)])
    return out


def walk(sets_h, evaluate):
    """one hypothesis: sets_h[a] for a < max_tries; evaluate(cells) -> (accepted, pose6).  Returns (pose, set, ok) by the rule of dsac_sample_rgbd."""
    for s in sets_h:
        if s is None:
            continue
        acc, pose = evaluate(s)
        if acc:
            return np.asarray(pose, np.float64), list(s), 1
    last = sets_h[-1]
    return np.zeros(6), (list(last) if last is not None else [0, 0, 0]), 0


def distances(poses, xyz, cam):
    """(N, P) float64 |R X + t - C|, NaN where the cell is not VALID (cam canonical)"""
    X, C = np.asarray(xyz, np.float64), np.asarray(cam, np.float64)
    out = np.empty((len(poses), len(X)))
    for i, h in enumerate(np.asarray(poses, np.float64)):
        out[i] = np.linalg.norm(X @ rodrigues(h[:3]).T + h[3:] - C, axis=1)
    return out


def err_images(d, clamp):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(d), clamp, np.minimum(d, clamp))


def soft_sums(d, clamp, tau, beta):
    e = err_images(d, clamp)
    s = 1.0 / (1.0 + np.exp(-beta * (tau - e)))
    return np.where(np.isnan(d), 0.0, s).sum(-1)


def score_bound(poses, xyz, cam, ref):
    """2^-24 [12 (|X|_1 + |t|_1 + |C|_1) + 8 ref] per pair, (N, P); inf where the cell is not VALID"""
    X1 = np.abs(np.asarray(xyz, np.float64)).sum(-1)
    C1 = np.abs(np.asarray(cam, np.float64)).sum(-1)
    t1 = np.abs(np.asarray(poses, np.float64)[:, 3:]).sum(-1)
    with np.errstate(invalid="ignore"):
        b = 2.0 ** -24 * (12 * (X1[None, :] + t1[:, None] + C1[None, :]) + 8 * ref)
    return np.where(np.isnan(b), np.inf, b)


# ---- refinement ---------------------------------------------------------------------------------------------------------------------------------
LD = np.longdouble


def _pass(h, X, C, v, tau, beta, cut):
    R = rodrigues(h[:3]).astype(LD)
    D = X @ R.T + h[3:].astype(LD) - C
    d = np.sqrt((D * D).sum(-1))
    with np.errstate(invalid="ignore", over="ignore"):
        w = 1 / (1 + np.exp(-LD(beta) * (LD(tau) - d)))
        w = np.where(v & np.isfinite(d) & (d < cut), w, LD(0))
    return w


def _horn(K):
    s = np.asarray(K, np.float64)
    N = np.array([[s[0, 0] + s[1, 1] + s[2, 2], s[1, 2] - s[2, 1], s[2, 0] - s[0, 2], s[0, 1] - s[1, 0]],
                  [s[1, 2] - s[2, 1], s[0, 0] - s[1, 1] - s[2, 2], s[0, 1] + s[1, 0], s[2, 0] + s[0, 2]],
                  [s[2, 0] - s[0, 2], s[0, 1] + s[1, 0], s[1, 1] - s[2, 2] - s[0, 0], s[1, 2] + s[2, 1]],
                  [s[0, 1] - s[1, 0], s[2, 0] + s[0, 2], s[1, 2] + s[2, 1], s[2, 2] - s[0, 0] - s[1, 1]]])
    ev, U = np.linalg.eigh(N)
    q = U[:, 3]
    q0, q1, q2, q3 = q
    R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                  [2 * (q1 * q2 + q0 * q3), q0 * q0 + q2 * q2 - q1 * q1 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                  [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 + q3 * q3 - q1 * q1 - q2 * q2]])
    return R, ev[3], ev[2]


def refine(h0, xyz, cam, tau, beta, cut, min_soft, max_iters, step_tol):
    """the loop of dsac_refine_rgbd for one problem.  Returns (pose, S, iters, status index, margin).  margin: how far the closest decision of the loop was
    from its threshold, as a multiple of what double-precision evaluation can move it by -- S against min_soft and S(h') against S(h) relative to
    P x 2^-53 x S (an ordered sum of P terms), the step against its tolerance and l1 - l2 against 1e-9 l1 relative to 1e-9.  A problem whose margin is below 1
    is undecided between two outcomes at double precision."""
    h = np.asarray(h0, np.float64).copy()
    if not np.isfinite(h).all():
        return h, 0.0, 0, 5, np.inf
    v = valid_cells(xyz, cam)
    X = np.where(v[:, None], np.asarray(xyz, np.float64), 0.0).astype(LD)
    C = np.where(v[:, None], np.asarray(cam, np.float64), 0.0).astype(LD)
    margin = np.inf
    w = _pass(h, X, C, v, tau, beta, cut)
    S = w.sum()
    noise = lambda s: len(X) * 2.0 ** -53 * max(float(s), 1.0)
    margin = min(margin, abs(float(S) - min_soft) / noise(S))
    if not S >= min_soft:
        return h, float(S), 0, 3, margin
    it = 0
    while True:
        xm, cm = (w[:, None] * X).sum(0) / S, (w[:, None] * C).sum(0) / S
        K = (w[:, None] * (X - xm)).T @ (C - cm) / S
        R, l1, l2 = _horn(K)
        hn = np.concatenate([rodrigues_inv(R), np.asarray(cm, np.float64) - R @ np.asarray(xm, np.float64)])
        margin = min(margin, abs((l1 - l2) - 1e-9 * l1) / (1e-9 * max(abs(l1), 1e-300)))
        if not np.isfinite(hn).all() or not (l1 - l2 > 1e-9 * l1):
            return h, float(S), it, 4, margin
        step, ref = np.linalg.norm(hn - h), step_tol * (np.linalg.norm(h) + 2.220446049250313e-16)
        with np.errstate(over="ignore"):  # step_tol = 0: the step is never within reach of its tolerance
            margin = min(margin, abs(step - ref) / (1e-9 * max(ref, 1e-300)))
        if step <= ref:
            return h, float(S), it, 0, margin
        wn = _pass(hn, X, C, v, tau, beta, cut)
        Sn = wn.sum()
        margin = min(margin, abs(float(Sn - S)) / noise(S))
        if not Sn >= S:
            return h, float(S), it, 2, margin
        h, w, S = hn, wn, Sn
        it += 1
        if it >= max_iters:
            return h, float(S), it, 1, margin


# ---- the corpus the scoring and refinement tests share (CPU and GPU) -------------------------------------------------------------------------------
def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two floats is exact in double"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def score_fp32(poses, xyz, cam, clamp, variant=""):
    """the scoring formulas in float32 as the kernel states them: float records, D = fma chain onto -C, sqrt of the fused squared norm, min with the clamp.
    variant: a deliberately wrong evaluation -- "Rt" (R transposed), "not" (t dropped), "swap" (C and X swapped), "noclamp"."""
    X, C = np.asarray(xyz, np.float32), np.asarray(cam, np.float32)
    if variant == "swap":
        X, C = C, X
    out = np.empty((len(poses), len(X)), np.float32)
    for i, h in enumerate(np.asarray(poses, np.float64)):
        R = rodrigues(h[:3])
        R = (R.T if variant == "Rt" else R).astype(np.float32)
        t = (np.zeros(3) if variant == "not" else h[3:]).astype(np.float32)
        q = np.zeros(len(X), np.float32)
        for j in range(3):
            d = fmaf(R[j, 0], X[:, 0], -C[:, j])
            d = fmaf(R[j, 1], X[:, 1], d)
            d = fmaf(R[j, 2], X[:, 2], d)
            d = fmaf(np.float32(1.0), t[j], d)
            q = fmaf(d, d, q) if j else (d * d).astype(np.float32)
        e = np.sqrt(q)
        with np.errstate(invalid="ignore"):
            out[i] = np.where(np.isnan(e), np.float32(clamp), e if variant == "noclamp" else np.minimum(e, np.float32(clamp)))
    return out


def rgbd_frame(H, W, seed, frames=1, dirty=True, **kw):
    """`frames` synthetic RGB-D frames of one geometry: xyz (F, P, 3), cam_xyz (F, P, 3) as handed to the library (NOT canonical), gt (F, 6).  dirty: a few
    cells of every frame carry each kind of invalid value: NaN / inf camera points, z = 0, z < 0, NaN scene coordinates."""
    from dsac_amd import synth
    xs, cs, gts = [], [], []
    for f in range(frames):
        fr = synth.chess_like_frame_rgbd(H, W, seed=seed + 17 * f, **kw)  # stratified pixel positions over 640 x 480: wide triangles
        xyz, cam = fr["xyz"].copy(), fr["cam_xyz"].copy()
        P = H * W
        if dirty and P >= 12:
            rng = np.random.default_rng(seed + 1000 + f)
            idx = rng.permutation(P)[:5]
            cam[idx[0], 0] = np.inf
            cam[idx[1], 2] = 0.0
            cam[idx[2], 2] = -cam[idx[2], 2] if np.isfinite(cam[idx[2], 2]) else -1.0
            xyz[idx[3], 1] = np.nan
            cam[idx[4], 1] = -np.inf
        xs.append(xyz)
        cs.append(cam)
        gts.append(fr["gt_pose"])
    return np.stack(xs), np.stack(cs), np.stack(gts)


def sampled_poses(xyz, cam, n, seed):
    """n poses of random VALID triples of one frame (kabsch3), the reference's own"""
    v = np.flatnonzero(valid_cells(xyz, cam))
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        cells = rng.choice(v, 3, replace=False)
        p = kabsch3(xyz, cam, cells)[0]
        if np.isfinite(p).all():
            out.append(p)
    return np.array(out)


FAR_POSE = np.array([0.3, -0.2, 0.1, 30000.0, -30000.0, 26457.513110645905])  # |t| = 50 m
SCORE_CASES = (  # name, H, W, frames, hypotheses per frame
    ("40x40", 40, 40, 1, 256), ("53x37", 37, 53, 1, 129), ("641x3", 3, 641, 1, 65), ("15", 3, 5, 1, 63), ("257", 1, 257, 1, 1),
    ("3x64", 40, 40, 3, 64), ("2x65", 37, 53, 2, 65),
    # more than 32 cell tiles of 256: the scoring kernel's block decode has a second tile group (PT = tiles, PTG = groups of 32)
    ("149x55", 55, 149, 2, 65),   # 8 195 cells: PT 33, PTG 2, the last tile holds 3 cells; two hypothesis tiles per frame, the second of one row; two frames
    ("129x64", 64, 129, 1, 65),   # 8 256 cells: PT 33, the last tile is one full chunk of 64
    ("129x129", 129, 129, 1, 3))  # 16 641 cells: PT 66, PTG 3, the last tile holds 1 cell
SCORE_TILE = 256  # cells of one scoring tile; 32 tiles make a group


def score_case(name):
    """xyz (F, P, 3), cam as given (F, P, 3), poses (F * Nf, 6): sampled poses plus the zero pose plus a pose with |t| = 50 m"""
    _, H, W, F, Nf = next(c for c in SCORE_CASES if c[0] == name)
    xyz, cam, _ = rgbd_frame(H, W, seed=4200 + H * W, frames=F, missing_frac=0.1)
    poses = []
    for f in range(F):
        p = sampled_poses(xyz[f], cam[f], Nf, seed=77 + f)
        if Nf >= 3:
            p[-1] = 0.0
            p[-2] = FAR_POSE
        poses.append(p)
    return H, W, xyz, cam, np.concatenate(poses)


def refine_case(H=40, W=40, frames=2, per_frame=12, seed=900):
    """start poses around the ground truth of every frame (perturbed by up to ~3 degrees / 60 mm), plus a far one, a non-finite one and the zero pose"""
    xyz, cam, gt = rgbd_frame(H, W, seed=seed, frames=frames, missing_frac=0.1, depth_noise_mm=5.0)
    rng = np.random.default_rng(seed)
    init = []
    for f in range(frames):
        p = gt[f][None, :] + np.concatenate([rng.normal(scale=0.02, size=(per_frame, 3)), rng.normal(scale=30.0, size=(per_frame, 3))], 1)
        p[-1] = FAR_POSE
        p[-2] = 0.0
        p[-3, 4] = np.nan
        init.append(p)
    return H, W, xyz, cam, gt, np.concatenate(init)


# ---- refinement off the 256-cell chunk: corpora and parameter sets (CPU and GPU) -----------------------------------------------------------------------
# the refinement's chunks are 256 cells up to 65 536 cells and whole 64-lane trips beyond:
#   164 x 401 = 65 764 cells: 206 chunks of 320, the last of 164 cells (two full trips and one of 36 lanes)
#   64 x 129  =  8 256 cells: 33 chunks of 256, the last of 64 cells
#   1 x 63: one partial trip
REFINE_CORPORA = ((164, 401), (64, 129), (1, 63))  # each 2 frames x 6 start poses, seed 901
REFINE_PARAMS = ((50.0, 20, 1e-6, 100.0), (5.0, 2, 0.0, 60.0), (5.0, 1, 0.0, 100.0))  # min_soft, max_iters, step_tol, cut
_REFINE_CACHE = {}


def refine_corpus(H, W):
    return refine_case(H, W, frames=2, per_frame=6, seed=901)


def refine_reference(xyz, cam, init, tau, beta, cut, min_soft, max_iters, step_tol, loop=None, key=None):
    """the loop (default: the long-double one) on every problem of a corpus, problem b on frame b // (B / F); cam as given.  key: cache the result under it"""
    if key is not None and key in _REFINE_CACHE:
        return _REFINE_CACHE[key]
    loop = refine if loop is None else loop
    canon = canonical(xyz, cam)[0]
    per = len(init) // xyz.shape[0]
    out = [loop(init[b], xyz[b // per], canon[b // per], tau, beta, cut, min_soft, max_iters, step_tol) for b in range(len(init))]
    if key is not None:
        _REFINE_CACHE[key] = out
    return out


def refine_f64(h0, xyz, cam, tau, beta, cut, min_soft, max_iters, step_tol, centred=True):
    """the loop of `refine` in plain float64 from the 16 sums the kernels take -- S, sum w x, sum w c, sum w x c^T about the first VALID cell (x = X - X0,
    c = C - C0; centred=False: about the origin) -- with K = sum w x c^T / S - xm cm^T and t = (C0 + cm) - R (X0 + xm).  Returns (pose, S, iters, status)."""
    h = np.asarray(h0, np.float64).copy()
    if not np.isfinite(h).all():
        return h, 0.0, 0, 5
    v = valid_cells(xyz, cam)
    X = np.where(v[:, None], np.asarray(xyz, np.float64), 0.0)
    C = np.where(v[:, None], np.asarray(cam, np.float64), 0.0)
    first = int(np.argmax(v)) if v.any() else -1
    X0 = X[first].copy() if centred and first >= 0 else np.zeros(3)
    C0 = C[first].copy() if centred and first >= 0 else np.zeros(3)
    x, c = X - X0, C - C0

    def sums(pose):
        D = X @ rodrigues(pose[:3]).T + pose[3:] - C
        d = np.sqrt((D * D).sum(-1))
        with np.errstate(invalid="ignore", over="ignore"):
            w = 1 / (1 + np.exp(-beta * (tau - d)))
            w = np.where(v & np.isfinite(d) & (d < cut), w, 0.0)
        wx = w[:, None] * x
        return w.sum(), wx.sum(0), (w[:, None] * c).sum(0), wx.T @ c

    S, sx, sc, sxc = sums(h)
    if not S >= min_soft:
        return h, float(S), 0, 3
    it = 0
    while True:
        with np.errstate(invalid="ignore", divide="ignore"):
            xm, cm = sx / S, sc / S
            K = sxc / S - np.outer(xm, cm)
        if not np.isfinite(K).all():
            return h, float(S), it, 4
        R, l1, l2 = _horn(K)
        hn = np.concatenate([rodrigues_inv(R), (C0 + cm) - R @ (X0 + xm)])
        if not np.isfinite(hn).all() or not (l1 - l2 > 1e-9 * l1):
            return h, float(S), it, 4
        if np.linalg.norm(hn - h) <= step_tol * (np.linalg.norm(h) + 2.220446049250313e-16):
            return h, float(S), it, 0
        Sn, sxn, scn, sxcn = sums(hn)
        if not Sn >= S:
            return h, float(S), it, 2
        h, S, sx, sc, sxc = hn, Sn, sxn, scn, sxcn
        it += 1
        if it >= max_iters:
            return h, float(S), it, 1


FAR_SHIFT = np.array([2e5, -3e5, 1e5])  # mm


def late_first_case():
    """the 2 x 40 x 40 refinement corpus with the first 300 cells of frame 1 not VALID (camera point NaN): that frame's first VALID cell lies in the second
    workgroup of the canonical copy's kernel; frame 0 is untouched"""
    H, W, xyz, cam, gt, init = refine_case()
    cam = cam.copy()
    cam[1, :300] = np.nan
    return H, W, xyz, cam, gt, init


def far_origin_case(late=False):
    """the 2 x 40 x 40 refinement corpus in a scene frame whose origin is FAR_SHIFT away: float32 coordinates X + shift, camera points regenerated as
    R X' + t' (the ground truth in the shifted frame, t' = t - R shift) in float64 from those float32 coordinates and rounded to float32 -- cells that were not
    VALID keep their values -- and every start pose moved to the shifted frame the same way, so it sees the distances it saw before.
    late: frame 1 loses its first 300 cells as in late_first_case."""
    H, W, xyz, cam, gt, init = late_first_case() if late else refine_case()
    per = len(init) // xyz.shape[0]
    xyz_f = (xyz.astype(np.float64) + FAR_SHIFT).astype(np.float32)
    cam_f, gt_f, init_f = cam.copy(), gt.copy(), init.copy()
    for f in range(xyz.shape[0]):
        R = rodrigues(gt[f][:3])
        gt_f[f][3:] = gt[f][3:] - R @ FAR_SHIFT
        v = valid_cells(xyz_f[f], cam[f])
        cam_f[f][v] = (xyz_f[f][v].astype(np.float64) @ R.T + gt_f[f][3:]).astype(np.float32)
    for b in range(len(init)):
        if np.isfinite(init[b]).all():
            init_f[b][3:] = init[b][3:] - rodrigues(init[b][:3]) @ FAR_SHIFT
    return H, W, xyz_f, cam_f, gt_f, init_f
