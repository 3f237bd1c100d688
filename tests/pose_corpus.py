"""Singular poses and non-finite scores for the fp64 tail kernels (K3, K4's finish, K6, K7), chosen on the CPU by the oracle alone (a plain helper
module like tests/lm_corpus.py: no fixtures, no GPU, nothing measured on a GPU enters it).

cv2our (core/types.h:186-214) negates rows 1 and 2 of the rotation matrix, so a camera aligned with the scene axes (cv rvec = 0: the first frame of a
sequence) is a jp rotation by exactly pi about x, and cv rvec = (pi, 0, 0) is the jp identity.  K7's rodrigues_m2v and the jp Jacobian behind
dsac_last_pose_gradients work in the jp convention, so those poses sit in the hand-written special cases of dmath.h: the s < 1e-5 branch of
rodrigues_m2v with its sign heuristics, its c > 0 exit, the theta < DBL_EPSILON select of rodrigues_R / rodrigues_J and the 1 - cos cancellation just
above it -- and in k_pose_loss the zero-error exit, the NaN-to-zero rule, the trace clamps, the 1e7 loss clamp and the glen > 1e-5 identity branch.

  identity_scene   a map whose ground-truth cv pose is (0, 0, 0, 120, -340, 2100)
  loss_cases       (est cv6, gt jp6, class) for K7, every case with the oracle's loss / J6, its sensitivity `sens` and the J6 bound that follows
  score_cases      score vectors for K3 with -inf, underflow, subnormal weights, NaN and +inf

Stability verdict of a loss case, oracle alone: the chain cv2our -> rodvec_and_trans -> dLossMax is re-run with each of the 9 entries of the jp rotation
matrix moved one ulp up and down, and with each of the 12 input components moved one ulp.  sens = the largest resulting change of J6 relative to
max(1, |J6|max); the case's J6 bound is max(1e-8, 4 sens) -- 1e-8 is K7's bound away from these poses (tests/test_gpu_refine.py, row a8), 4 x the
oracle's own sensitivity is the rule of test_dpnp_parity.  A case whose bound exceeds 1e-4 (or whose oracle J6 is not finite), or that sits on the
zero-error exit by rounding alone (_on_the_zero_exit), is unstable: its J6 is not compared on the GPU, its loss still is.  tests/test_pose_corpus_cpu.py holds the corpus to its conditions.

Deliberately left out of loss_cases: a NaN or infinite ROTATION in the estimate (the reference's answer runs through OpenCV's SVD of a NaN matrix, which
the oracle does not pin), and dRefineHyp / dPNP at jp angle pi (the reference's own central differences straddle the +pi / -pi representation there).
"""
import ctypes as C
import functools

import numpy as np

CAM = (525.0, 525.0, 320.0, 240.0)
GT_CV = np.array([0.2, -0.1, 0.05, 120.0, -340.0, 2100.0])      # the generic ground truth of test_loss_and_gradient
IDENT_CV = np.array([0.0, 0.0, 0.0, 120.0, -340.0, 2100.0])     # the identity scene's: jp rotation (pi, 0, 0)
T_JP = np.array([120.0, 340.0, -2100.0])                         # the same translation in the jp convention
PER = 16
JP_PI_M = (0.0, 1e-17, 1e-12, 1e-9, 1e-7, 1e-6, 9e-6, 1.1e-5, 1e-4)     # both sides of rodrigues_m2v's s < 1e-5
JP_ZERO_D = (0.0, 1e-17, 1e-12, 1e-9, 1e-7, 9e-6, 1.1e-5, 1e-4)
# (angle, axes).  Within 1e-6 of pi the reference's own 1 / sqrt(3 - tr^2 + 2 tr) is decided by the last bits of the trace (tr + 1 = (pi - a)^2 is below
# 1e-12, one ulp of tr is 2e-16; at the clamp the factor is 1 / 0): those angles are unstable by the verdict whatever the axis, so they get 4 axes each and
# the stable side four more angles up to pi - 1e-5 -- the class keeps its unstable share under the cap and every one of its angles.
ROT_ERR_A = ((1e-5, PER), (1e-3, PER), (1.0, PER), (np.pi - 1e-2, PER), (np.pi - 1e-3, PER), (np.pi - 1e-4, PER), (np.pi - 1e-5, PER),
             (np.pi - 1e-6, 4), (np.pi - 1e-9, 4), (np.pi, 4))
ROT_ERR_AT_CLAMP = np.pi - 2e-6   # from here on the reference's J6 may be infinite (the division by sqrt(0)): finiteness is not asserted
JP_PI_T_SIGMA = 50.0              # mm.  Against the identity scene's ground truth the loss is the translation error and J6 turns with its direction: one ulp of the jp
                                  # matrix's diagonal moves m2v's axis by 7e-9 at angle pi, |t| / 10 = 210 cm times that over tErr[cm] is the sensitivity
                                  # (3 mm of noise: 4 sens up to 7e-4 and 21 unstable cases; 50 mm: all stable)
T_ERR_A = (0.0, 1e-9, 1e-6)
GT_SINGULAR_LEN = (0.0, 5e-6, 1.5e-5, np.pi)                     # both sides of glen > 1e-5, and angle pi
CLASSES = ("jp_pi", "jp_zero", "rot_err", "t_err", "zero", "gt_singular", "clamp", "nan_t")
J6_FLOOR, SENS_FACTOR, UNSTABLE_ABOVE = 1e-8, 4.0, 1e-4
MAX_UNSTABLE_SHARE = 1.0 / 8
SCORE_N = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def identity_scene(seed, noise_mm, H=40, W=40):
    """An H x W map on the pixel grid (u = x, v = y), depths 800-3500 mm, no outliers, ground-truth cv pose IDENT_CV: xyz = Xc - t + noise as float32."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAM
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    u, v = u.reshape(-1), v.reshape(-1)
    depth = rng.uniform(800.0, 3500.0, size=H * W)
    Xc = np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], -1)
    noise = rng.normal(size=(H * W, 3)) * noise_mm
    return dict(xyz=(Xc - IDENT_CV[3:] + noise).astype(np.float32), uv=np.stack([u, v], -1).astype(np.float32), gt_pose=IDENT_CV.copy(), H=H, W=W, cam=CAM)


def singular_starts(seed, sigma_mm, per_m=2):
    """Start poses next to the identity scene's ground truth: rvec m u over JP_PI_M (m = 0 exactly among them), translation + N(0, sigma_mm)."""
    rng = np.random.default_rng(seed)
    m = np.repeat(np.asarray(JP_PI_M), per_m)
    out = np.tile(IDENT_CV, (len(m), 1))
    out[:, :3] = m[:, None] * _units(rng, len(m))
    out[:, 3:] += rng.normal(size=(len(m), 3)) * sigma_mm
    return out


def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def gt_matrix(orc, gt_jp6):
    """Hypothesis(std::vector<double>) (core/Hypothesis.cpp:81-99): the identity up to a rotation vector of length 1e-5, cv::Rodrigues beyond."""
    r = np.asarray(gt_jp6[:3], np.float64)
    return orc.rodrigues_vec2mat(r) if np.sqrt((r * r).sum()) > 1e-5 else np.eye(3)


def oracle_loss(orc, est_cv6, gt_jp6):
    """(loss, rotErr [deg], tErr [mm], correct) of maxLoss(Hypothesis(cv2our(est)), Hypothesis(gt))."""
    Re, te = orc.cv2our(est_cv6)
    Rg, tg = gt_matrix(orc, gt_jp6), np.asarray(gt_jp6[3:], np.float64)
    rot, tr = orc.pose_errors(Rg, tg, Re, te)
    return orc.maxLoss(Rg, tg, Re, te), rot, tr, bool(rot < 5 and tr < 50)


def oracle_J6(orc, est_cv6, gt_jp6, m2v=None):
    """dLossMax(getRodVecAndTrans(cv2our(est)), gt); m2v replaces the oracle's matrix -> vector step (the CPU test puts the kernel's there)."""
    R, t = orc.cv2our(est_cv6)
    est_jp = orc.rodvec_and_trans(R, t) if m2v is None else np.concatenate([m2v(R), t])
    return orc.dLossMax(est_jp, gt_jp6)


def sensitivity(orc, est_cv6, gt_jp6):
    """(J6, sens): the largest change of the oracle's J6 under one-ulp moves of the jp rotation matrix's entries and of the 12 inputs, relative to
    max(1, |J6|max).  A J6 that is not finite, or a run that is not, counts as infinite."""
    J = oracle_J6(orc, est_cv6, gt_jp6)
    if not np.isfinite(J).all():
        return J, np.inf
    runs = []
    R, t = orc.cv2our(est_cv6)
    for k in range(9):
        for away in (np.inf, -np.inf):
            R2 = R.copy()
            R2.flat[k] = np.nextafter(R.flat[k], away)
            runs.append(orc.dLossMax(orc.rodvec_and_trans(R2, t), gt_jp6))
    x = np.concatenate([est_cv6, gt_jp6])
    for k in range(12):
        for away in (np.inf, -np.inf):
            x2 = x.copy()
            x2[k] = np.nextafter(x[k], away)
            runs.append(oracle_J6(orc, x2[:6], x2[6:]))
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(runs) - J[None, :]).max()
    return J, (float(d) if np.isfinite(d) else np.inf) / max(1.0, float(np.abs(J).max()))


def _compose(orc, gt_cv, rot, shift=None):
    """gt with its rotation composed with Rod(rot) about the SAME camera centre (moved by `shift` mm): the rotation error is |rot|, the translation
    error |shift| -- both to rounding."""
    Rg = orc.rodrigues_vec2mat(gt_cv[:3])
    centre = -Rg.T @ gt_cv[3:]
    if shift is not None:
        centre = centre + shift
    if np.any(rot != 0):
        Re = orc.rodrigues_vec2mat(rot) @ Rg
        rvec = orc.rodrigues_mat2vec(Re)
        Re = orc.rodrigues_vec2mat(rvec)
    else:
        Re, rvec = Rg, gt_cv[:3]
    return np.concatenate([rvec, -Re @ centre])


def _raw_cases(orc):
    rng = np.random.default_rng(20260)
    gt_generic, gt_ident = orc.cv_to_jp6(GT_CV), orc.cv_to_jp6(IDENT_CV)
    gt_small = np.concatenate([[0.02, -0.01, 0.03], T_JP])
    out = []

    def add(cls, est, gt, tag):
        out.append(dict(cls=cls, est=np.asarray(est, np.float64).copy(), gt=np.asarray(gt, np.float64).copy(), tag=tag))

    # jp_pi: cv rotation m u -- the jp rotation is by pi - O(m) -- against a generic ground truth and against one that sits at jp angle pi itself
    for m in JP_PI_M:
        for u in _units(rng, PER):
            est = np.concatenate([m * u, IDENT_CV[3:] + rng.normal(size=3) * JP_PI_T_SIGMA])
            add("jp_pi", est, gt_generic, "m=%g vs generic" % m)
            add("jp_pi", est, gt_ident, "m=%g vs identity scene" % m)
    # jp_zero: jp rotation Rod(d u) -- rodrigues_m2v's c > 0 exit, the theta < eps select of the derivative inside dLossMax
    for d in JP_ZERO_D:
        for u in _units(rng, PER):
            est = orc.our2cv(orc.rodrigues_vec2mat(d * u), T_JP + rng.normal(size=3) * 3.0)
            add("jp_zero", est, gt_generic, "d=%g vs generic" % d)
            add("jp_zero", est, gt_small, "d=%g vs small" % d)
    flipped = np.concatenate([[np.pi, 0.0, 0.0], GT_CV[3:]])
    add("jp_zero", flipped, gt_generic, "cv rvec (pi, 0, 0) vs generic")
    add("jp_zero", flipped, gt_small, "cv rvec (pi, 0, 0) vs small")
    # rot_err: the rotation branch up to the trace clamp at -1, the translation error at rounding level
    for a, axes in ROT_ERR_A:
        for u in _units(rng, axes):
            add("rot_err", _compose(orc, GT_CV, a * u), gt_generic, "a=%.10g" % a)
    # t_err: the translation branch; the smallest shift keeps tErr[cm] above 20 x the rotation error [deg]
    for a in T_ERR_A:
        lo = max(1e-4, 200.0 * np.rad2deg(a))
        for u, v, mag in zip(_units(rng, PER), _units(rng, PER), np.geomspace(lo, 100.0, PER)):
            add("t_err", _compose(orc, GT_CV, a * u, mag * v), gt_generic, "a=%g shift=%.3g mm" % (a, mag))
    # zero: est equal to gt exactly, and within 1e-10 -- the zero-error exit.  Three of the exact ones have a generic rotation (see _on_the_zero_exit)
    for name, cv in (("generic", GT_CV), ("identity scene", IDENT_CV), ("cv rvec (pi, 0, 0)", flipped)):
        add("zero", cv, orc.cv_to_jp6(cv), "exact, " + name)
    for k in range(2):
        cv = np.concatenate([_units(rng, 1)[0] * rng.uniform(0.1, 2.5), rng.normal(size=3) * 500.0 + [0, 0, 2000.0]])
        add("zero", cv, orc.cv_to_jp6(cv), "exact, random pose %d" % k)
    for k in range(PER - 5):
        cv = np.concatenate([(IDENT_CV, flipped)[k % 2][:3], rng.normal(size=3) * 500.0 + [0, 0, 2000.0]])
        add("zero", cv, orc.cv_to_jp6(cv), "exact, %s rotation, random translation %d" % (("identity scene's", "flipped")[k % 2], k))
    for k in range(PER):
        cv = (IDENT_CV, flipped)[k % 2].copy()
        cv[3:] += rng.normal(size=3) * 1e-10
        add("zero", cv, orc.cv_to_jp6((IDENT_CV, flipped)[k % 2]), "within 1e-10, %d" % k)
    # gt_singular: ground-truth jp rotations on both sides of max_loss_forward's glen > 1e-5, and of angle pi
    for L in GT_SINGULAR_LEN:
        for u, n in zip(_units(rng, PER), _units(rng, PER)):
            gt = np.concatenate([L * u, T_JP])
            est = orc.our2cv(orc.rodrigues_vec2mat(L * u + 0.03 * n), T_JP + rng.normal(size=3) * 20.0)
            add("gt_singular", est, gt, "glen=%.10g" % L)
    # clamp: loss 1e7 with a zero gradient, and just below it
    for mag, tag in ((1e9, "beyond"), (9.9e7, "just below")):
        for v in _units(rng, PER):
            add("clamp", _compose(orc, GT_CV, np.zeros(3), mag * v), gt_generic, tag)
    # nan_t: a NaN in the estimate's translation -- cv2our zeroes the translation (core/types.h:186-214)
    for k in range(PER):
        est = GT_CV + np.concatenate([rng.normal(size=3) * 0.05, rng.normal(size=3) * 50.0])
        est[([3], [4], [5], [3, 4, 5])[k % 4]] = np.nan
        add("nan_t", est, gt_generic, "NaN in t, %d" % k)
    return out


def _on_the_zero_exit(orc, c):
    """est and gt agree to rounding (the zero class) but the trace of rot1 rot2^T is 3 only up to rounding.  J6 is 0 / 0 there: dLossMax returns exactly 0
    when its computed trace (nine rounded products, summed) comes out as 3 or more, and 1 / sqrt(3 - tr) x rounding residue -- up to 1e-5 -- when it comes
    out one ulp below, and which of the two happens is decided by the order and the fusing of those nine products, not by any input: in the oracle 10 of
    14 generic poses with est == gt return 0 and stay 0 under every one-ulp move, and a kernel that sums the same products with fused multiply-adds lands
    on the other side for some of them.  Such a case sits on the exit's discontinuity and tests nothing about J6: it counts as unstable.  The exit itself
    is tested where the trace is 3 in any arithmetic: both matrices made of 0, +-1 and entries whose squares vanish below an ulp (the jp rotations by pi
    about x and by 0 -- the poses this corpus is about)."""
    if not (c["tErr"] / 10 < 1e-8 and c["rotErr"] < 1e-5):  # the exit is tErr[cm] + rotErr[deg] < 1e-8, and a rotation error is 0 or at least 1.2e-6 deg
        return False
    R, t = orc.cv2our(c["est"])
    rot1, rot2 = orc.rodrigues_vec2mat(orc.rodvec_and_trans(R, t)[:3]), orc.rodrigues_vec2mat(c["gt"][:3])
    a = np.abs(np.concatenate([rot1.reshape(-1), rot2.reshape(-1)]))
    return not bool(np.all((a == 0) | (a == 1) | (a < 1e-8)))


@functools.lru_cache(maxsize=None)
def _loss_cases(orc):
    cases = _raw_cases(orc)
    for c in cases:
        c["loss"], c["rotErr"], c["tErr"], c["correct"] = oracle_loss(orc, c["est"], c["gt"])
        c["J6"], c["sens"] = sensitivity(orc, c["est"], c["gt"])
        c["bound"] = max(J6_FLOOR, SENS_FACTOR * c["sens"])
        c["on_exit"] = _on_the_zero_exit(orc, c)
        c["stable"] = bool(c["bound"] <= UNSTABLE_ABOVE) and not c["on_exit"]
        # the oracle's J6 is exactly zero and stays so under every one-ulp move: an exit (zero error, the loss clamp), not a rounding accident
        c["robust_zero"] = bool(not c["J6"].any() and c["sens"] == 0.0) and not c["on_exit"]
    return cases


def loss_cases(orc):
    """The K7 corpus: a list of dicts cls, tag, est (cv6), gt (jp6), and by the oracle loss, rotErr, tErr, correct, J6, sens, bound, stable, robust_zero."""
    return _loss_cases(orc)


def padded_loss_cases(orc):
    """loss_cases padded with a generic case until the count exceeds 128 and is no multiple of 64 (K7 runs 64 estimates per workgroup)."""
    cases = list(loss_cases(orc))
    generic = next(c for c in cases if c["cls"] == "rot_err" and c["tag"] == "a=1")
    while len(cases) <= 128 or len(cases) % 64 == 0:
        cases.append(generic)
    return cases


def summary(cases):
    """{class: (size, unstable, largest bound among the stable ones)}"""
    out = {}
    for cls in CLASSES:
        sel = [c for c in cases if c["cls"] == cls]
        out[cls] = (len(sel), sum(not c["stable"] for c in sel), max([c["bound"] for c in sel if c["stable"]], default=0.0))
    return out


def pose_gradients(orc, fr, poses, d_err):
    """G6[h] = sum_p d_err[h, p] * dProjectdHyp(uv_p, xyz_p, cv2our(pose_h)) (core/cnn_softam.h:631-632): orc.dScore's pose gradients restated for given
    poses (orc.dScore only takes minimal sets).  Calls the oracle's own dProjectdHyp cell by cell."""
    lib = orc.lib()
    xyz = np.ascontiguousarray(fr["xyz"], np.float32)
    uv = np.ascontiguousarray(fr["uv"], np.float32)
    cam = np.ascontiguousarray(fr["cam"], np.float64)
    d_err = np.asarray(d_err, np.float64)
    P = xyz.shape[0]
    J = np.zeros((P, 6))
    G6 = np.zeros((len(poses), 6))
    vp = C.c_void_p
    pu, px, pj, pc = uv.ctypes.data, xyz.ctypes.data, J.ctypes.data, vp(cam.ctypes.data)
    f = lib.orc_dProjectdHyp
    for h, pose in enumerate(np.asarray(poses, np.float64).reshape(-1, 6)):
        R, t = orc.cv2our(pose)
        R, t = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t)
        pR, pt = vp(R.ctypes.data), vp(t.ctypes.data)
        for p in range(P):
            f(vp(pu + 8 * p), vp(px + 12 * p), pR, pt, pc, vp(pj + 48 * p))
        G6[h] = d_err[h] @ J
    return G6


def score_cases(N):
    """[(name, scores N, poses N x 6)] for K3: scores a score model can produce (a masked hypothesis is -inf) and scores it must not (NaN, +inf)."""
    rng = np.random.default_rng(7000 + N)
    base = rng.normal(scale=5.0, size=N)
    poses = np.concatenate([rng.normal(scale=0.3, size=(N, 3)), rng.normal(scale=300.0, size=(N, 3)) + np.array([0.0, 0.0, 2000.0])], -1)
    out = []

    def add(name, s):
        out.append((name, np.asarray(s, np.float64), poses))

    s = base.copy(); s[N // 2] = -np.inf
    add("one -inf", s)
    s = base.copy(); s[1::2] = -np.inf
    add("half -inf", s)
    add("all equal", np.full(N, 3.7))
    add("beyond underflow", np.resize(np.array([0.0, -800.0, -30000.0, -1e6, -745.2, -1e300]), N))
    s = -740.0 + rng.uniform(-4.0, 4.0, size=N); s[0] = 0.0
    add("subnormal weights", s)
    s = base.copy(); s[0] = np.nan
    add("NaN at index 0", s)
    s = base.copy(); s[N - 1] = np.nan
    add("NaN elsewhere", s)
    s = base.copy(); s[N // 3] = np.inf
    add("+inf", s)
    add("all -inf", np.full(N, -np.inf))
    return out
