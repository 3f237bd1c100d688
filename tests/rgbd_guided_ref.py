"""Guided RGB-D sampling restated in numpy and Python integers (include/dsac_hip.h, dsac_set_sampling_weights_rgbd), built on guided_ref (the table, the
draw) and rgbd_ref (the VALID rule, the sampling loop): the expected side of tests/test_gpu_rgbd_guided.py, itself checked by tests/test_rgbd_guided_ref_cpu.py.

    masked_weights(w, valid)   w' = w where the cell is VALID, 0 elsewhere -- before anything else
    build_table(w, valid)      guided_ref.build_table of w': (C', T', n', S', masses)
    walk3(cells)               the three-cell walk over the 32 candidate cells of one attempt: a candidate already in the set is skipped
    attempt_sets3(...)         sets[h][a] (three cells or None) of every attempt, in the shape rgbd_ref.walk takes, and the candidates each attempt used
    backward_ref3(...)         one frame of dsac_sampling_weights_backward_rgbd in double precision
    PATTERNS / frame / CASES   the corpus the CPU and the GPU tests share
No GPU, no library call."""
import math

import numpy as np

import guided_ref as gr
import rgbd_ref as rr

_U = np.uint64


def masked_weights(w, valid):
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    return np.where(np.asarray(valid, bool).reshape(-1), w, np.float32(0.0)).astype(np.float32)


def build_table(w, valid):
    """One frame: (C' uint64[P], T', n', S', masses uint64[P]) -- the 2D rule applied to the masked weights."""
    return gr.build_table(masked_weights(w, valid))


def candidate_cells(C, T, seed, N, A):
    """cells int64 [N][A][32]: candidate k of attempt a of hypothesis h, v = mix64(key(h) + ((a << 16) | k))"""
    keys = gr.hyp_key(seed, np.arange(N))
    att = np.arange(A, dtype=np.uint64) << _U(16)
    with np.errstate(over="ignore"):
        base = keys[:, None] + att[None, :]
        v = gr.mix64(base[:, :, None] + np.arange(32, dtype=np.uint64)[None, None, :])
    return gr.cell_of(C, T, v.reshape(-1)).reshape(N, A, 32)


def walk3(cells, limit=32):
    """(the three cells or None, candidates used): candidates in order, one that is already in the set is skipped, more than `limit` fail the attempt"""
    got = []
    for k in range(limit):
        c = int(cells[k])
        if c not in got:
            got.append(c)
            if len(got) == 3:
                return got, k + 1
    return None, limit


def attempt_sets3(C, T, n, seed, N, A, walk=walk3):
    """sets[h][a] = [c0, c1, c2] or None for a < A (what rgbd_ref.walk takes), used int [N][A] (candidates the attempt took).  n < 3: None"""
    if n < 3:
        return None, np.zeros((N, A), np.int64)
    cells = candidate_cells(C, T, seed, N, A)
    sets, used = [], np.zeros((N, A), np.int64)
    for h in range(N):
        row = []
        for a in range(A):
            s, used[h, a] = walk(cells[h, a])
            row.append(s)
        sets.append(row)
    return sets, used


def sample_frame(w, valid, seed, N, A, evaluate, walk=walk3):
    """dsac_sample_rgbd's drawn path on one frame with active RGB-D weights: (poses [N][6], sets [N][3], ok [N], stats).  evaluate(h, a, cells) ->
    (accepted, pose6).  stats counts what the walk met: attempts with skipped candidates, attempts without a set, hypotheses accepted at an attempt >= 64,
    failures that report a drawn set, failures that report zeros."""
    C, T, n, S, m = build_table(w, valid)
    poses, out, ok = np.zeros((N, 6)), np.zeros((N, 3), np.int32), np.zeros(N, np.uint8)
    stats = dict(redraw=0, undrawn=0, late=0, fail_drawn=0, fail_zero=0)
    sets, used = attempt_sets3(C, T, n, seed, N, A, walk)
    if sets is None:
        stats["fail_zero"] = N
        return poses, out, ok, stats
    for h in range(N):
        first = -1
        for a, s in enumerate(sets[h]):
            if s is None:
                continue
            acc, pose = evaluate(h, a, s)
            if acc:
                first = a
                poses[h], out[h], ok[h] = pose, s, 1
                break
        if first < 0 and sets[h][-1] is not None:
            out[h] = sets[h][-1]
        walked = A if first < 0 else first + 1
        stats["redraw"] += int(sum(1 for a in range(walked) if sets[h][a] is not None and used[h, a] > 3))
        stats["undrawn"] += int(sum(1 for a in range(walked) if sets[h][a] is None))
        stats["late"] += int(first >= 64)
        stats["fail_drawn"] += int(first < 0 and sets[h][-1] is not None)
        stats["fail_zero"] += int(first < 0 and sets[h][-1] is None)
    return poses, out, ok, stats


def kabsch_evaluator(xyz, canon, thr):
    """the numpy evaluator of the CPU tests: rgbd_ref.kabsch3 + accept3"""
    def ev(h, a, cells):
        p, R, t = rr.kabsch3(xyz, canon, cells)
        return rr.accept3(p, rr.residuals3(xyz, canon, cells, R, t), thr), p
    return ev


def backward_ref3(w, valid, S, sets, ok, g, uniform=3.0):
    """One frame of dsac_sampling_weights_backward_rgbd: (gradient [P], sum of |addends| [P], addend count [P], |uniform term|).  A cell has mass
    iff its masked weight is finite and > 0; the uniform term -3 G / S' uses the exactly rounded sum G of the accepted g (math.fsum)."""
    wm = masked_weights(w, valid)
    v = gr.valid_cells(wm)
    P = wm.size
    grad, mag, cnt = np.zeros(P), np.zeros(P), np.zeros(P, np.int64)
    acc = [h for h in range(len(ok)) if ok[h]]
    uni = -uniform * math.fsum(float(g[h]) for h in acc) / S if acc and v.any() else 0.0
    for h in acc:
        for c in sets[h]:
            if 0 <= c < P and v[c]:
                a = float(g[h]) / float(np.float64(wm[c]))
                grad[c] += a
                mag[c] += abs(a)
                cnt[c] += 1
    grad[v] += uni
    mag[v] += abs(uni)
    return grad, mag, cnt, abs(uni)


# ---- the corpus (CPU and GPU) -----------------------------------------------------------------------------------------------------------------------
FRAME_SEEDS = {(40, 40): 1671, (37, 53): 2032, (3, 5): 1671}
_FRAMES = {}


def frame(H, W, frames=1, **kw):
    """xyz, cam (as handed to the library), VALID mask -- each (F, P, ...); 10 % depth holes (30 % on the 15-cell map)"""
    key = (H, W, frames, tuple(sorted(kw.items())))
    if key not in _FRAMES:
        kw2 = dict(missing_frac=0.3 if H * W <= 15 else 0.1)
        kw2.update(kw)
        xyz, cam, _ = rr.rgbd_frame(H, W, seed=FRAME_SEEDS[(H, W)], frames=frames, **kw2)
        _FRAMES[key] = (xyz, cam, rr.valid_cells(xyz, cam))
    return _FRAMES[key]


def clean_frame(H, W):
    return frame(H, W, dirty=False, noise_mm=0.0, outlier_frac=0.0, depth_noise_mm=0.0)


def _rng(s):
    return np.random.default_rng(s)


def w_ones(v):
    return np.ones(v.size, np.float32)


def w_mask01(v):
    return (_rng(1).random(v.size) < 0.5).astype(np.float32)


def w_heavy(v):
    w = (_rng(2).random(v.size) ** 8).astype(np.float32)
    w[_rng(3).permutation(v.size)[:3]] = 50.0
    return w


def w_mixed(v):
    P = v.size
    rng = _rng(4)
    w = rng.random(P).astype(np.float32)
    idx = rng.permutation(P)[:min(80, 4 * (P // 4))].reshape(4, -1)
    for bad, cells in zip((np.nan, -1.0, np.inf, 0.0), idx):
        w[cells] = bad
    return w


def w_on_holes(v):
    return np.where(v, np.float32(1e-3), np.float32(1.0)).astype(np.float32)


def w_three(v):
    w = np.zeros(v.size, np.float32)
    w[np.flatnonzero(v)[[3, 400, 900]]] = (1.0, 2.0, 3.0)
    return w


def w_lopsided(v):
    w = np.zeros(v.size, np.float32)
    w[np.flatnonzero(v)[[5, 300, 700, 1100]]] = (1.0, 2.0 ** -23, 2.0 ** -23, 2.0 ** -24)
    return w


def w_two(v):
    w = np.zeros(v.size, np.float32)
    w[np.flatnonzero(v)[[10, 1000]]] = (1.0, 0.5)
    w[np.flatnonzero(~v)[:5]] = 2.0
    return w


PATTERNS = dict(ones=w_ones, mask01=w_mask01, heavy=w_heavy, mixed=w_mixed, on_holes=w_on_holes, three=w_three, lopsided=w_lopsided, two=w_two)
SMALL_PATTERNS = ("ones", "mask01", "heavy", "mixed", "on_holes")  # the patterns that do not name cells by number: every map size

# (H, W, F, Nf, max_tries, seed_stride, thr, pattern(s), clean): the sampling cases of the GPU test; one pattern per frame
CASES = (
    (40, 40, 1, 64, 3, 1, 60.0, ("ones",), False),
    (40, 40, 1, 65, 70, 1, 25.0, ("mask01",), False),
    (37, 53, 1, 65, 130, 1, 8.0, ("heavy",), False),
    (40, 40, 1, 64, 70, 1, 100.0, ("three",), False),
    (40, 40, 1, 64, 70, 1, 100.0, ("three",), True),
    (40, 40, 1, 64, 70, 1, 100.0, ("lopsided",), False),
    (40, 40, 1, 65, 70, 1, 1e-9, ("mask01",), False),
    (3, 5, 1, 63, 3, 1, 200.0, ("ones",), False),
    (40, 40, 1, 1, 70, 1, 25.0, ("heavy",), False),
    (40, 40, 1, 257, 3, 1, 60.0, ("mixed",), False),
    (40, 40, 3, 128, 3, 1, 60.0, ("heavy", "two", "mask01"), False),
    (40, 40, 3, 128, 3, 5, 60.0, ("heavy", "two", "mask01"), False),
    # attempt 46 of hypothesis 16 gets its third cell from candidate 31, the last one allowed; nothing is accepted on this frame, so with max_tries 47 that
    # set is what the hypothesis reports (tests/test_rgbd_guided_ref_cpu.py holds this: a walk that stops one candidate early reports zeros there)
    (40, 40, 1, 64, 47, 1, 100.0, ("three",), False))
SEED = 1305


def case_inputs(case):
    """xyz (F, P, 3), cam (F, P, 3), valid (F, P), weights (F, P) of a sampling case"""
    H, W, F, Nf, A, stride, thr, pats, clean = case
    xyz, cam, v = clean_frame(H, W) if clean else frame(H, W, frames=F)
    w = np.stack([PATTERNS[pats[f]](v[f]) for f in range(F)])
    return xyz, cam, v, w
