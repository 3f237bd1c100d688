"""Guided sampling restated in numpy and Python integers (include/dsac_hip.h, dsac_set_sampling_weights): the table, the draw, the redraw loop.

No device, no library: this is the expected side of tests/test_gpu_guided.py and is itself checked by tests/test_guided_ref_cpu.py.
    mix64 / hyp_key        the counter stream of dmath.h (splitmix64's finaliser), on uint64 arrays
    build_table(w)         masses m_p = floor((double) w_p / (double) wmax * 2^24) for the valid cells (finite, > 0), C = cumsum in uint64, T, n, S
    cell_of(C, T, v)       t = floor(v * T / 2^64) in Python integers, the smallest p with C[p] > t (searchsorted, side='right')
    attempt_sets(...)      candidate sets of attempts 0 .. A - 1 of hypotheses 0 .. N - 1: duplicates redrawn with the next k, more than 32 candidates fail
"""
import numpy as np

M64 = (1 << 64) - 1
_U = np.uint64


def mix64(z):
    """dm::mix64 on a uint64 array (wrap-around arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def hyp_key(seed, hyp):
    """dm::hyp_key: mix64(seed ^ mix64(hyp)); hyp may be an array."""
    return mix64(_U(int(seed) & M64) ^ mix64(np.asarray(hyp, dtype=np.uint64)))


def valid_cells(w):
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    return np.isfinite(w) & (w > 0)


def build_table(w):
    """One frame: (C uint64[P], T, n, S, masses uint64[P])."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    v = valid_cells(w)
    m = np.zeros(w.shape, np.uint64)
    if v.any():
        wmax = np.float64(w[v].max())
        m[v] = np.floor(w[v].astype(np.float64) / wmax * 16777216.0).astype(np.uint64)
    C = np.cumsum(m, dtype=np.uint64)
    return C, int(C[-1]), int(np.count_nonzero(m)), float(np.sum(w[v].astype(np.float64))), m


def t_of_int(v, T):
    """floor(v * T / 2^64) for a uint64 array v, in Python integers (what __umul64hi computes): the definition."""
    return np.array([(int(x) * int(T)) >> 64 for x in np.asarray(v, dtype=np.uint64).reshape(-1)], dtype=np.uint64).reshape(np.shape(v))


def t_of(v, T):
    """The same from 32-bit halves in uint64 arrays (no sum below overflows); tests/test_guided_ref_cpu.py holds it against t_of_int."""
    v = np.asarray(v, dtype=np.uint64)
    m32 = _U(0xFFFFFFFF)
    vh, vl, th, tl = v >> _U(32), v & m32, _U(int(T) >> 32), _U(int(T) & 0xFFFFFFFF)
    hi_lo = vh * tl
    cross = ((vl * tl) >> _U(32)) + (hi_lo & m32) + vl * th
    return vh * th + (hi_lo >> _U(32)) + (cross >> _U(32))


def cell_of(C, T, v):
    """The cell of the 64-bit value(s) v: the smallest p with C[p] > t."""
    return np.searchsorted(C, t_of(v, T), side="right").astype(np.int64)


def attempt_sets(C, T, n, seed, N, A, first_attempt=0):
    """sets int32 [N][A][4], drawn uint8 [N][A] (0: the attempt ran out of candidates; its row is zeros), redraws int [N][A] (candidates beyond four).
    Attempt a of hypothesis h draws candidate k from v = mix64(key(h) + ((a << 16) | k)).  n < 4: nothing can be drawn (all zeros)."""
    sets = np.zeros((N, A, 4), np.int32)
    drawn = np.zeros((N, A), np.uint8)
    redraws = np.zeros((N, A), np.int64)
    if n < 4:
        return sets, drawn, redraws
    keys = hyp_key(seed, np.arange(N))
    att = (np.arange(first_attempt, first_attempt + A, dtype=np.uint64) << _U(16))
    with np.errstate(over="ignore"):
        base = keys[:, None] + att[None, :]                       # [N][A]
        v = mix64(base[:, :, None] + np.arange(32, dtype=np.uint64)[None, None, :])  # all 32 candidates of every attempt
    cells = cell_of(C, T, v.reshape(-1)).reshape(N, A, 32)
    for h in range(N):
        for a in range(A):
            got = []
            k = 0
            while len(got) < 4 and k < 32:
                c = int(cells[h, a, k])
                k += 1
                if c not in got:
                    got.append(c)
            if len(got) == 4:
                sets[h, a] = got
                drawn[h, a] = 1
                redraws[h, a] = k - 4
    return sets, drawn, redraws


def backward_ref(w, S, sets, ok, g):
    """One frame of dsac_sampling_weights_backward in double precision: (gradient [P], sum of |addends| [P], addend count [P], |uniform term|).
    The uniform term -4 G / S uses the exactly rounded sum G of the accepted g (math.fsum)."""
    import math
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    v = valid_cells(w)
    P = w.size
    grad, mag, cnt = np.zeros(P), np.zeros(P), np.zeros(P, np.int64)
    acc = [h for h in range(len(ok)) if ok[h]]
    uni = -4.0 * math.fsum(float(g[h]) for h in acc) / S if acc and v.any() else 0.0
    for h in acc:
        for c in sets[h]:
            if 0 <= c < P and v[c]:
                a = float(g[h]) / float(np.float64(w[c]))
                grad[c] += a
                mag[c] += abs(a)
                cnt[c] += 1
    grad[v] += uni
    mag[v] += abs(uni)
    return grad, mag, cnt, abs(uni)
