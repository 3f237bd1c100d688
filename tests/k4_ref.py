"""Reference, fp32 model and corpus for the per-cell tests of K4 (tests/test_k4_ref_cpu.py, tests/test_gpu_k4_cells.py).

k4_reference: dScore part (iii) without the support scatter, vectorised numpy in float64.  The arithmetic is d_project_d_obj / d_project_d_hyp of
oracle/dsac_oracle.cpp (core/cnn_softam.h:404-453, :464-528): jp pose from orc.cv2our, guards |Ez| < 1e-8 -> 0 and err > 100 -> 0, then err + 1e-8; the
rotation part through orc.rodrigues_mat2vec and orc.rodrigues_vec2mat(jac=True), once per hypothesis.  Beside the gradient it returns `scale`, the absolute
sum behind every cell: the per-cell metric compares a cell's error with the cell's own scale, not with the largest entry of the map.

k4_fp32_model: K4's pair arithmetic (the comment block of k_score_backward_mfma in dsac_amd/csrc/k_backward.hip) in plain np.float32 -- what a correct fp32
kernel computes.  Only the CPU checks use it: it shows that the asserted bounds pass a correct kernel and catch six wrong ones.

mask_pairs: the (hypothesis, cell) pairs that carry no weight in the corpus: the clamp edge |err - 100| <= 0.01 (the guard err > 100 -> 0 is a
discontinuity; tests/test_gpu_backward_big.py drops the same band) and |Ez| < 200 mm (fp32 cancellation of E = RX + t next to the camera centre, the
depth rule of tests/test_gpu_random_shapes.py).

The corpus is chosen from K4's launch plan (dk::backward_plan); tests/test_gpu_k4_cells.py says which plan values each case relies on."""
import functools

import numpy as np

from dsac_amd import synth
from oracle import oracle as orc

TAU, BETA, CLAMP = 10.0, 0.5, 100.0
CELL_TOL = 1e-3          # SURVEY.md 8(c), fp32 fast mode -- applied to each cell's own absolute sum
POSE_MEDIAN, POSE_MAX = 1e-4, 1e-3   # the pose-sum figures of tests/test_gpu_backward.py
MASK_CAP = 0.02          # mask_pairs may remove at most this share of a case's pairs


# ---- geometry shared by the reference's three inputs ------------------------------------------------------------------------------------------
def k4_geometry(poses_cv6, xyz, uv, cam):
    """Per (hypothesis, cell): J3 = dProjectdObj (N x P x 3), C = the three translation entries of dProjectdHyp (N x P x 3: its rotation entries are
    sum_k (C_j X_k) dRdH[i, 3 j + k]), err (unclamped, inf where |Ez| < 1e-8), Ez; per hypothesis dRdH (N x 3 x 9).  float64 throughout."""
    poses = np.asarray(poses_cv6, np.float64).reshape(-1, 6)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    pt = np.asarray(uv, np.float32).astype(np.float64)
    f, cx, cy = float(cam[0]), float(cam[2]), float(cam[3])
    N, P = poses.shape[0], X.shape[0]
    J3, Cc = np.zeros((N, P, 3)), np.zeros((N, P, 3))
    err, Ez, dRdH = np.zeros((N, P)), np.zeros((N, P)), np.zeros((N, 3, 9))
    with np.errstate(divide="ignore", invalid="ignore"):
        for h in range(N):
            R, t = orc.cv2our(poses[h])
            ex = R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]   # the oracle's order of operations
            ey = R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]
            ez = R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2]
            near = np.abs(ez) < 1e-8
            px, py = -f * ex / ez + cx, f * ey / ez + cy
            du, dv = pt[:, 0] - px, pt[:, 1] - py
            e = np.sqrt(du * du + dv * dv)
            keep = ~near & ~(e > CLAMP)
            ee = e + 1e-8
            for c in range(3):
                pxd = -f * R[0, c] / ez + f * ex / ez / ez * R[2, c]
                pyd = f * R[1, c] / ez - f * ey / ez / ez * R[2, c]
                J3[h, :, c] = np.where(keep, 0.5 / ee * (2 * du * -pxd + 2 * dv * -pyd), 0.0)
            n0, n1 = -1 / ee * du, -1 / ee * dv
            Cc[h, :, 0] = np.where(keep, n0 * (-f / ez), 0.0)
            Cc[h, :, 1] = np.where(keep, n1 * (f / ez), 0.0)
            Cc[h, :, 2] = np.where(keep, n0 * (f * ex / ez / ez) + n1 * (-f * ey / ez / ez), 0.0)
            err[h] = np.where(near, np.inf, e)
            Ez[h] = ez
            dRdH[h] = orc.rodrigues_vec2mat(orc.rodrigues_mat2vec(R), jac=True)[1]
    return dict(J3=J3, C=Cc, err=err, Ez=Ez, dRdH=dRdH, X=X)


def soft_weights(g, err, tau=TAU, beta=BETA, clamp=CLAMP):
    """g[h] * d sigmoid(beta (tau - min(err, clamp))) / d err, in float64"""
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-beta * (tau - np.minimum(err, clamp))))
    return np.asarray(g, np.float64)[:, None] * (-beta) * s * (1.0 - s)


def transpose_cells(a, W):
    """row p = y W + x of `a` moved to row x W + y (core/cnn_softam.h:628 on a square map)"""
    P = a.shape[0]
    assert W * W == P, "the transposed cell index needs a square map"
    p = np.arange(P)
    out = np.empty_like(a)
    out[(p % W) * W + p // W] = a
    return out


def k4_reference(poses_cv6, xyz, uv, cam, d_err=None, g=None, tau=TAU, beta=BETA, clamp=CLAMP, transpose=False, geom=None):
    """-> dict(grad P x 3, scale P, G6 N x 6, err N x P, Ez N x P).  With g: the fused soft-inlier weights.  geom: k4_geometry's result for the same
    poses and frame (computed when absent)."""
    geo = geom if geom is not None else k4_geometry(poses_cv6, xyz, uv, cam)
    w = soft_weights(g, geo["err"], tau, beta, clamp) if g is not None else np.asarray(d_err, np.float64)
    J3, Cc = geo["J3"], geo["C"]
    grad = np.einsum("hp,hpc->pc", w, J3)
    scale = np.einsum("hp,hp->p", np.abs(w), np.sqrt((J3 * J3).sum(2)))
    wC = w[:, :, None] * Cc
    M = np.einsum("hpj,pk->hjk", wC, geo["X"]).reshape(-1, 9)
    G6 = np.concatenate([np.einsum("hik,hk->hi", geo["dRdH"], M), wC.sum(1)], 1)
    if transpose:
        W = int(round(np.sqrt(grad.shape[0])))
        grad, scale = transpose_cells(grad, W), transpose_cells(scale, W)
    return dict(grad=grad, scale=scale, G6=G6, err=geo["err"], Ez=geo["Ez"])


def mask_pairs(err, Ez):
    return (np.abs(err - CLAMP) <= 0.01) | (np.abs(Ez) < 200.0)


# ---- a correct fp32 kernel ---------------------------------------------------------------------------------------------------------------------
def k4_fp32_model(poses_cv6, xyz, uv, cam, d_err=None, g=None, tau=TAU, beta=BETA, clamp=CLAMP, transpose=False):
    """K4's pair arithmetic in np.float32: A = (u - cx) Ez + f Ex, B = (v - cy) Ez - f Ey, S = A^2 + B^2, keep = clamp((clamp^2 Ez^2 - S) 1e30, 0, 1),
    m = 1 / sqrt(Ez^2 S + 1e-30), 1 / Ez = m^2 S Ez, C0 / f = A w m, -C1 / f = B w m, -C2 = (C0 Ex + C1 Ey) / Ez, the three coefficient rows; the pose
    sums against (f Ex, -f Ey, Ez, 1), off-diagonal pairs only, finished in float64 like k_support_scatter.  -> dict(grad, G6)."""
    f32 = np.float32
    poses = np.asarray(poses_cv6, np.float64).reshape(-1, 6)
    X = np.asarray(xyz, np.float32)
    pt = np.asarray(uv, np.float32)
    f, cx, cy = f32(cam[0]), f32(cam[2]), f32(cam[3])
    N, P = poses.shape[0], X.shape[0]
    pu, pv = pt[:, 0] - cx, pt[:, 1] - cy
    cl, cl2 = f32(clamp), f32(clamp) * f32(clamp)
    LOG2E = f32(1.4426950408889634)
    kA, kB = f32(beta) * LOG2E, f32(-beta) * f32(tau) * LOG2E
    gx, gy, gz = np.zeros(P, f32), np.zeros(P, f32), np.zeros(P, f32)
    G6 = np.zeros((N, 6))
    with np.errstate(over="ignore", invalid="ignore"):
        for h in range(N):
            R64, t64 = orc.cv2our(poses[h])
            R, t = R64.astype(f32), t64.astype(f32)
            bx = (f * R[0, 0], f * R[0, 1], f * R[0, 2], f * t[0])
            by = (f * -R[1, 0], f * -R[1, 1], f * -R[1, 2], f * -t[1])
            bz = (R[2, 0], R[2, 1], R[2, 2], t[2])
            ex = ((X[:, 0] * bx[0] + X[:, 1] * bx[1]) + X[:, 2] * bx[2]) + bx[3]   # f Ex
            ny = ((X[:, 0] * by[0] + X[:, 1] * by[1]) + X[:, 2] * by[2]) + by[3]   # -f Ey
            ez = ((X[:, 0] * bz[0] + X[:, 1] * bz[1]) + X[:, 2] * bz[2]) + bz[3]
            A, B = pu * ez + ex, pv * ez + ny
            Sq = B * B + A * A
            zz = ez * ez
            keep = np.clip((zz * cl2 - Sq) * f32(1e30), f32(0), f32(1))
            m = f32(1) / np.sqrt(zz * Sq + f32(1e-30))
            if g is not None:
                e = Sq * m
                sg = f32(1) / (np.exp2(kA * np.minimum(e, cl) + kB) + f32(1))
                w = (sg * (f32(g[h]) * f32(-beta))) * (f32(1) - sg)
            else:
                w = np.asarray(d_err[h], f32)
            w = w * keep
            q0 = w * m
            iz = (m * m) * (Sq * ez)
            C0, nC1 = A * q0, B * q0
            nC2 = (nC1 * ny + C0 * ex) * iz
            gx += (f * R[0, 0]) * C0 + ((f * -R[1, 0]) * nC1 + (-R[2, 0]) * nC2)
            gy += (f * R[0, 1]) * C0 + ((f * -R[1, 1]) * nC1 + (-R[2, 1]) * nC2)
            gz += (f * R[0, 2]) * C0 + ((f * -R[1, 2]) * nC1 + (-R[2, 2]) * nC2)
            # pose sums: a[3 j + m] = sum C~_j E~_m (j != m), a[9 + j] = sum C~_j, fp32 over the cells, then k_support_scatter's fp64 finish
            Ct, Et = (C0, nC1, nC2), (ex, ny, ez)
            a = np.zeros(12)
            for j in range(3):
                for k in range(3):
                    if j != k:
                        a[3 * j + k] = float((Ct[j] * Et[k]).sum(dtype=f32))
                a[9 + j] = float(Ct[j].sum(dtype=f32))
            fd = float(f)
            sj, sm = (fd, -fd, -1.0), (1.0 / fd, -1.0 / fd, 1.0)
            Bv = np.array([sj[j] * a[9 + j] for j in range(3)])
            S9 = np.zeros(9)
            for j in range(3):
                for k in range(3):
                    if j != k:
                        S9[3 * j + k] = sj[j] * sm[k] * a[3 * j + k] - float(t[k]) * Bv[j]
            Rre, J = orc.rodrigues_vec2mat(orc.rodrigues_mat2vec(R64), jac=True)
            for i in range(3):
                Om = J[i].reshape(3, 3) @ Rre.T   # Omega_i = (dR / d rod_i) R^T, skew-symmetric
                G6[h, i] = (S9 * Om.reshape(9)).sum()
            G6[h, 3:] = Bv
    grad = np.stack([gx, gy, gz], 1).astype(np.float64)
    if transpose:
        grad = transpose_cells(grad, int(round(np.sqrt(P))))
    return dict(grad=grad, G6=G6)


# ---- the metric --------------------------------------------------------------------------------------------------------------------------------
def cell_ratio(grad, ref, cells=None):
    """max over the cells of max_c |grad - ref| / (scale + 1e-30 / CELL_TOL): <= CELL_TOL is the asserted per-cell bound
    max_c |grad[p, c] - ref[p, c]| <= CELL_TOL * scale[p] + 1e-30."""
    r = np.abs(grad - ref["grad"]).max(1) / (ref["scale"] + 1e-30 / CELL_TOL)
    if cells is not None:
        r = r[cells]
    return float(r.max(initial=0.0))


def pose_ratios(G6, ref_G6):
    """per hypothesis: max-rel to its largest component (hypotheses whose reference sums are all zero: 0 when the sums are exactly zero, inf otherwise)"""
    big = np.abs(ref_G6).max(1)
    d = np.abs(G6 - ref_G6).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(big > 0, d / np.where(big > 0, big, 1.0), np.where(d == 0, 0.0, np.inf))


def global_ratio(grad, ref):
    """the metric of the older K4 tests: max |g - ref| / max |ref|"""
    return float(np.abs(grad - ref["grad"]).max() / max(np.abs(ref["grad"]).max(), 1e-300))


# ---- 16-bit gradient images --------------------------------------------------------------------------------------------------------------------
def bf16_bits(a32):
    """float32 -> bfloat16 bit patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------------
# (family, H, W, implicit uv, N, variants, options).  Every (map, N) is one set of inputs shared by its variants.
def _corpus():
    out = []

    def add(family, H, W, implicit, N, variants, seed=None, **opt):
        out.append(dict(family=family, H=H, W=W, implicit=implicit, N=N, variants=tuple(variants), seed=seed, opt=opt))
    for N in (1, 5):
        add("tiny", 2, 2, False, N, (-1, 1, 2))
        add("tiny", 3, 4, True, N, (-1, 1, 2))
    # seed 9944: the first seed of a scan whose heavy-tailed field has the map's last eight cells in its tail (exponent < -2.9) -- where a clamped load used
    # as data (mutation 1 of tests/test_k4_ref_cpu.py) is invisible to a metric relative to the map's largest entry
    add("chunk tail", 38, 42, False, 40, (-1, 1, 2, 3, 4, 5, 6, 7), seed=9944, accumulate=True)
    add("implicit tail", 36, 44, True, 17, (-1, 1, 2, 3, 4, 5, 6, 7))
    for form, ch in ((1, 2), (2, 4), (3, 5), (4, 6), (5, 3), (6, 2), (7, 3)):
        add("one tile + 4", 4, 16 * ch + 1, False, 16, (form,))
    add("VALU forms", 37, 41, False, 33, (-1, 0))
    add("VALU forms", 38, 42, True, 33, (-1, 0))
    for N in (1, 15, 16, 17, 257):
        add("hypothesis edges", 38, 42, False, N, (-1, 2))
    add("split tiles, direct", 168, 200, False, 48, (101,))
    add("split tiles, layered", 120, 160, False, 80, (111,))
    add("staged", 38, 42, False, 40, (1999, 1002))
    add("transposed index", 40, 40, False, 24, (-1, 0), transpose=True)
    add("16-bit images", 38, 42, False, 40, (-1, 1, 5), elem="f16")
    add("16-bit images", 38, 42, False, 40, (-1, 1, 5), elem="bf16")
    add("frame batch", 38, 42, False, 48, (-1,), frames=3)
    return out


CORPUS = _corpus()
# one camera per frame of the batch: fx = fy, three focal lengths, three principal points
BATCH_CAMS = ((525.0, 525.0, 320.0, 240.0), (260.0, 260.0, 300.0, 250.0), (610.0, 610.0, 335.0, 228.0))


def case_id(c):
    return "%s-%dx%d%s-N%d%s" % (c["family"].replace(" ", "_").replace(",", "").replace("+", "p"), c["H"], c["W"], "i" if c["implicit"] else "s", c["N"],
                                 "".join("-%s%s" % (k, "" if v is True else v) for k, v in sorted(c["opt"].items())))


def _seed(c):
    if c["seed"] is not None:
        return c["seed"]
    return 4000 + 7 * c["H"] + 13 * c["W"] + 3 * c["N"] + (1 if c["implicit"] else 0)


def _frame_inputs(H, W, implicit, N, seed, cam, elem):
    """One frame's inputs and reference: frame, poses (ground truth + N(0, 0.03 rad) / N(0, 40 mm)), sets (any 4 distinct cells), the two d_err fields
    (float32, zero on mask_pairs; 16-bit cases: rounded first, the reference gets the rounded values), g, and k4_reference of the three inputs."""
    P = H * W
    if cam is None:
        # implicit pixel positions are the cell indices: the full-size camera scaled down, principal point at the map's centre (tests/test_gpu_random_shapes.py)
        cam = (525.0 * W / 640, 525.0 * W / 640, W / 2.0, H / 2.0) if implicit else synth.CAM_7SCENES
    fr = synth.chess_like_frame(H, W, seed=seed, grid_uv=implicit, cam=cam)
    rng = np.random.default_rng(seed + 100000)
    poses = fr["gt_pose"] + rng.normal(size=(N, 6)) * np.array([0.03, 0.03, 0.03, 40.0, 40.0, 40.0])
    sets = np.stack([rng.choice(P, 4, replace=False) for _ in range(N)]).astype(np.int32)
    geo = k4_geometry(poses, fr["xyz"], fr["uv"], fr["cam"])
    masked = mask_pairs(geo["err"], geo["Ez"])
    flat = (rng.standard_normal((N, P)) * 1e-3).astype(np.float32)
    heavy = (rng.standard_normal((N, P)) * 10.0 ** rng.uniform(-4.0, 0.0, size=P)[None, :]).astype(np.float32)
    d_err, bits = {}, {}
    for name, d in (("flat", flat), ("heavy", heavy)):
        if elem == "f16":
            bits[name] = d.astype(np.float16)
            d = bits[name].astype(np.float32)
        elif elem == "bf16":
            bits[name] = bf16_bits(d)
            d = bf16_widen(bits[name])
        d = np.where(masked, np.float32(0), d)
        if elem == "f16":
            bits[name] = d.astype(np.float16)   # exact: d holds halves and zeros
        elif elem == "bf16":
            bits[name] = bf16_bits(d)
        d_err[name] = np.ascontiguousarray(d)
    g = rng.normal(size=N)
    return dict(fr=fr, poses=poses, sets=sets, geo=geo, masked=masked, d_err=d_err, bits=bits, g=g)


@functools.lru_cache(maxsize=None)
def _build(idx):
    c = CORPUS[idx]
    H, W, N, opt = c["H"], c["W"], c["N"], c["opt"]
    frames = opt.get("frames", 1)
    elem = opt.get("elem", "f32")
    tr = bool(opt.get("transpose"))
    parts = [_frame_inputs(H, W, c["implicit"], N, _seed(c) + 17 * f, BATCH_CAMS[f] if frames > 1 else None, elem) for f in range(frames)]
    refs = {}
    for name in ("flat", "heavy", "soft"):
        rs = [k4_reference(p["poses"], p["fr"]["xyz"], p["fr"]["uv"], p["fr"]["cam"], d_err=None if name == "soft" else p["d_err"][name],
                           g=p["g"] if name == "soft" else None, transpose=tr, geom=p["geo"]) for p in parts]
        refs[name] = dict(grad=np.concatenate([r["grad"] for r in rs]), scale=np.concatenate([r["scale"] for r in rs]), G6=np.concatenate([r["G6"] for r in rs]))
    clean = np.concatenate([~p["masked"].any(0) for p in parts])   # cells without a masked pair (the soft mode's per-cell check)
    if tr:
        clean = transpose_cells(clean, W)
    return dict(case=c, parts=parts, refs=refs, clean_cells=clean, frames=frames, elem=elem, transpose=tr, H=H, W=W, P=H * W, N=N)


def build_case(idx):
    """Inputs and references of CORPUS[idx], computed once per process and shared: treat the arrays as read-only."""
    return _build(idx)
