#!/usr/bin/env python3
"""Generates tests/golden/dpnp_exact.npz: dPNP's central differences from EXACT P3P poses, for the accepted sets of tests/dpnp_corpus.py (frames A, B, C
at eps = 0.1, frame A also at 0.5 and 2.0).  Needs mpmath; the fixture it writes is all the tests read.  Run:  python tests/golden/make_dpnp_exact.py

This is a reference of the operation itself, independent of the project's restatement of dPNP in oracle/dsac_oracle.cpp and of Gao's quartic:

  inputs, taken exactly   the float32 coordinates and positions, the camera as the floats the engine receives; the positions normalised and rounded to
                          float once ((u - cx) / fx, as OpenCV's solvePnP hands them to its P3P); the perturbation replayed in np.float32
                          (v += eps; v -= 2 eps; v += eps for every coordinate in front of a column's own); the divisor float(np.float32(2) * np.float32(eps))
  per perturbed point set the three depths d_i of the first three points are the root of d_i^2 + d_j^2 - 2 d_i d_j cos(theta_ij) = |X_i - X_j|^2 next to the
                          oracle's pose: Newton in 60-digit arithmetic from the oracle's depths, to a step below 1e-40.  The camera-frame triangle
                          d_i b_i and the scene triangle X_i are then congruent, and the pose is the rigid motion between their orthonormal triads
  the 6-vector            cv2our (rows 1 and 2 of the rotation and t_y, t_z negated), the rotation vector of that matrix, the translation; the
                          difference of the two sides over the divisor is rounded to double once, at the end

A solve that does not converge in 30 steps, or lands more than 1e-3 (rad, or mm / 1000) from the oracle's pose, has converged elsewhere (another root of
the P3P, or none): its set is left out of the fixture, and at most 5 % of a frame's sets may be.  The oracle only supplies the starting point and the choice
among the P3P's up to four roots; no figure of it enters J_exact.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import dpnp_corpus as dc  # noqa: E402

OUT = os.path.join(HERE, "dpnp_exact.npz")
GROUPS = (("A", 0.1), ("B", 0.1), ("C", 0.1), ("A", 0.5), ("A", 2.0))
DIGITS, MAX_STEPS, STEP_BELOW, ELSEWHERE = 60, 30, 1e-40, 1e-3
MAX_LEFT_OUT = 0.05
PAIRS = ((1, 2), (0, 2), (0, 1))


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def _vec(mp, a):
    return [mp.mpf(float(v)) for v in a]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unit(mp, a):
    n = mp.sqrt(_dot(a, a))
    return [x / n for x in a]


def _triad(mp, p):
    e1 = _unit(mp, _sub(p[1], p[0]))
    e3 = _unit(mp, _cross(_sub(p[1], p[0]), _sub(p[2], p[0])))
    return [e1, _cross(e3, e1), e3]


def _rotation(mp, r):
    """Rodrigues' formula"""
    th = mp.sqrt(_dot(r, r))
    if th == 0:
        return [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]
    k = [x / th for x in r]
    c, s = mp.cos(th), mp.sin(th)
    K = [[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]
    return [[c * int(i == j) + (1 - c) * k[i] * k[j] + s * K[i][j] for j in range(3)] for i in range(3)]


def _rotation_vector(mp, R):
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    a = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    s = mp.sqrt(_dot(a, a)) / 2
    th = mp.atan2(s, c)
    if s == 0:
        assert c > 0, "rotation by pi: outside this fixture"
        return [mp.mpf(0)] * 3
    return [x * th / (2 * s) for x in a]


def bearings(mp, uv4, cam):
    """unit rays of the first three positions from their float-normalised coordinates"""
    fx, fy, cx, cy = [float(np.float32(c)) for c in cam]
    out = []
    for i in range(3):
        xn = np.float32((float(uv4[i][0]) - cx) * (1.0 / fx))
        yn = np.float32((float(uv4[i][1]) - cy) * (1.0 / fy))
        out.append(_unit(mp, [mp.mpf(float(xn)), mp.mpf(float(yn)), mp.mpf(1)]))
    return out


def exact_jp6(mp, X4, uv4, cam, start_cv6):
    """The jp 6-vector of the exact P3P pose next to start_cv6 (mpf), or None when the solve converges elsewhere."""
    b = bearings(mp, uv4, cam)
    X = [_vec(mp, X4[i]) for i in range(3)]
    cos = {p: _dot(b[p[0]], b[p[1]]) for p in PAIRS}
    D2 = {p: _dot(_sub(X[p[0]], X[p[1]]), _sub(X[p[0]], X[p[1]])) for p in PAIRS}
    R0, t0 = _rotation(mp, _vec(mp, start_cv6[:3])), _vec(mp, start_cv6[3:])
    d = []
    for i in range(3):
        Pc = [_dot(R0[r], X[i]) + t0[r] for r in range(3)]
        d.append(mp.sqrt(_dot(Pc, Pc)))
    for _ in range(MAX_STEPS):
        F = mp.matrix([d[i] ** 2 + d[j] ** 2 - 2 * d[i] * d[j] * cos[(i, j)] - D2[(i, j)] for i, j in PAIRS])
        Jm = mp.zeros(3, 3)
        for r, (i, j) in enumerate(PAIRS):
            Jm[r, i] = 2 * d[i] - 2 * d[j] * cos[(i, j)]
            Jm[r, j] = 2 * d[j] - 2 * d[i] * cos[(i, j)]
        try:
            step = mp.lu_solve(Jm, F)
        except ZeroDivisionError:
            return None
        d = [d[i] - step[i] for i in range(3)]
        if max(abs(step[i]) for i in range(3)) < STEP_BELOW:
            break
    else:
        return None
    if min(d) <= 0:
        return None
    Ec, Ew = _triad(mp, [[d[i] * x for x in b[i]] for i in range(3)]), _triad(mp, X)
    R = [[sum(Ec[k][r] * Ew[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
    t = [d[0] * b[0][r] - _dot(R[r], X[0]) for r in range(3)]
    Rj = [R[0], [-x for x in R[1]], [-x for x in R[2]]]
    jp = _rotation_vector(mp, Rj) + [t[0], -t[1], -t[2]]
    # the same for the start, to tell a solve that went elsewhere
    R0j = [R0[0], [-x for x in R0[1]], [-x for x in R0[2]]]
    jp0 = _rotation_vector(mp, R0j) + [t0[0], -t0[1], -t0[2]]
    off = max(max(abs(jp[k] - jp0[k]) for k in range(3)), max(abs(jp[k] - jp0[k]) for k in range(3, 6)) / 1000)
    return jp if off <= ELSEWHERE else None


def exact_J(orc, fr, set4, eps):
    """6 x 12 doubles, or None when one of the 24 solves fails in the oracle or converges elsewhere"""
    mp = _mp()
    set4 = np.asarray(set4)
    uv4, X0 = fr["uv"][set4], fr["xyz"][set4]
    div = mp.mpf(dc.divisor(eps))
    J = np.zeros((6, 12))
    for c in range(12):
        side = []
        for sgn in (+1, -1):
            X = dc.perturbed_points(X0, c, sgn, eps)
            ok, pose = orc.solve_p3p(X, uv4, fr["cam"])
            jp = exact_jp6(mp, X, uv4, fr["cam"], pose) if ok else None
            if jp is None:
                return None
            side.append(jp)
        for k in range(6):
            J[k, c] = float((side[0][k] - side[1][k]) / div)
    return J


def main():
    from oracle import oracle as orc
    orc.build()
    tags, sets, epss, Js, errs = [], [], [], [], []
    for tag, eps in GROUPS:
        fr = dc.frame(tag)
        left_out = 0
        for s in dc.accepted_sets(orc, tag):
            J = exact_J(orc, fr, s, eps)
            if J is None:
                left_out += 1
                continue
            tags.append(tag); sets.append(s); epss.append(eps); Js.append(J)
            errs.append(dc.rel(dc.oracle_J(orc, fr, s, eps), J))
        e = np.array(errs[-(dc.N_ACCEPTED - left_out):])
        print("frame %s eps %-4g: %d sets, %d left out; oracle vs exact: median %.2e  max %.2e" % (tag, eps, len(e), left_out, np.median(e), e.max()), flush=True)
        assert left_out <= MAX_LEFT_OUT * dc.N_ACCEPTED, (tag, eps, left_out)
    np.savez_compressed(OUT, tag=np.array(tags), set=np.array(sets, np.int32), eps=np.array(epss, np.float64), J_exact=np.array(Js),
                        oracle_rel=np.array(errs), frame_tags=np.array(["A", "B", "C"]),
                        frame_crc=np.array([dc.checksum(t) for t in ("A", "B", "C")], np.uint32))
    print("wrote %s (%d sets, %d bytes)" % (OUT, len(tags), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
