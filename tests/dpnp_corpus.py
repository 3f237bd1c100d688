"""Minimal sets for K5 (k_dpnp) off the one shape of test_dpnp_parity, chosen on the CPU by the oracle alone (a plain helper module like
tests/pose_corpus.py and tests/lm_corpus.py: no fixtures, no GPU, nothing measured on a GPU enters it).

Frames (synth.chess_like_frame, the smallest shapes that still reach every branch of load_set and of the kernel):

  A   37 x 41, unquantised float coordinates, an explicit table of positions with a deterministic sub-pixel jitter, the default camera
  B   24 x 32, positions on the map's own grid, handed to the engine WITHOUT a table (load_set's y = p / W, u = p - y W with H != W)
  C   40 x 40, int16-quantised coordinates, camera (585, 610, 300.5, 250.25): fx != fy and an off-centre principal point
  D   3 x 5, grid positions without a table: 15 cells, most sets of four collinear or nearly so

B and D use a camera scaled to the map (525 px at 640 columns, the principal point in the middle): under the 640-column camera a 32-column grid is a bundle
of rays 3.5 degrees wide and no set of it is conditioned at all.

Sets per frame: `accepted` -- 64 sets the oracle's sampler accepts -- and `random` -- 192 sets of four distinct random cells, which is where P3P fails
outright (the zero pose of safeSolvePnP), fails on one side of a central difference only, or changes its winning root between the two sides.

Frozen lists (cell indices written below, each found by a search function that stays here and that tests/test_dpnp_corpus_cpu.py re-runs):

  ZERO    16 sets per frame on A - C whose oracle Jacobian is exactly zero and stays exactly zero under all 24 one-ulp moves of the 12 coordinates
  BIG     sets on A and C with |J|max > 1e3 and a one-ulp sensitivity <= 1e-4, each with its class: "one_sided" (P3P fails on one side of the steepest
          column's difference: the other side is differenced against the zero pose), "switch" (both sides solve, and between them the pose jumps between
          two ADJACENT float values of the coordinate: another root wins), "steep" (neither)
  REPLAY  accepted sets of frame A on which the sequential float perturbation of the reference (v += eps; v -= 2 eps; v += eps, core/cnn_softam.h:115-135)
          demonstrably matters, in two forms (replay_case()):
          J_noreplay  every column from the pristine points, each side perturbed once (v + eps, v - eps).  The reference's backward side is (v + eps) - 2 eps,
                      up to an ulp of v away, and an ulp over 2 eps = 0.2 mm is 1e-3 of the column: kept are sets with
                      rel(J, J_noreplay) >= 100 max(1e-9, 4 sens) -- 345 of 512 candidates, the median distance is 3e-4.
          J_lane      the column's own two sides as the reference runs them, the coordinates IN FRONT of it pristine: k_dpnp without its `cc < c` line.
                      The round trips move those coordinates by an ulp or so, which is what sens measures: over the 512 candidates rel(J, J_lane) is at
                      most 0.63 of the set's bound max(1e-6, 4 sens) and at most 2.5 sens.  NO comparison with the oracle under K5's bound can tell a
                      kernel without that line from one with it.  What can is a which-side check: kept are sets with rel(J, J_lane) >= max(1e-7, sens)
                      (37 of the 345), on which a kernel that replays is nearer to J than to J_lane unless its own error reaches half a one-ulp sensitivity.

Stability verdict of a set at a step eps (the rule of test_dpnp_parity and of pose_corpus): sens = the largest change of the oracle's J, relative to
max(1, |J|max), over one-ulp moves of the 12 float coordinates in both directions; bound = max(1e-6, 4 sens); a set whose bound exceeds 1e-2 (or whose J is
not finite) is unstable: its J is not compared on the GPU, its finiteness is.

What the searches found (tests/test_dpnp_corpus_cpu.py prints the numbers):
  * BIG: one_sided and switch on both frames; no stable member of "steep" within the budget (BIG_NOTE below the list).
  * POISONED: no kind dropped -- the oracle's answer is reproducible and finite for NaN, +inf and -inf.  In one of the first three points every solve
    fails and J is exactly zero; in the fourth point only the choice among the roots is spoilt (it falls on the first) and J is an ordinary Jacobian.
  * REPLAY: frame A at eps = 0.1, the coordinates as they are (up to 4 m, where a float round trip moves a coordinate by up to 2.4e-4 mm).
"""
import functools

import numpy as np

EPS = 0.1
EXTRA_EPS = (0.5, 2.0, 0.01)             # frame A's accepted sets only.  2 eps is a power of two for the first two: * (1 / (2 eps)) and / (2 eps) coincide
TAGS = ("A", "B", "C", "D")
CAM_C = (585.0, 610.0, 300.5, 250.25)
N_ACCEPTED, N_RANDOM, N_ZERO, N_BIG_MIN, N_REPLAY_MIN = 64, 192, 16, 6, 32
FLOOR, SENS_FACTOR, UNSTABLE_ABOVE = 1e-6, 4.0, 1e-2
BIG_ABOVE, BIG_SENS = 1e3, 1e-4
BIG_BLOCK, BIG_BUDGET_BLOCKS = 1000, 200  # 200 000 random sets per frame
MAX_UNSTABLE_ACCEPTED, MAX_UNSTABLE_RANDOM, MIN_STABLE_NONZERO_D = 0.10, 0.35, 8
_SEEDS = {"A": 5101, "B": 5102, "C": 5103, "D": 5104}
REPLAY_TAG, REPLAY_EPS = "A", 0.1
REPLAY_FACTOR, REPLAY_FLOOR = 100.0, 1e-9
LANE_FLOOR = 1e-7


def _grid_cam(H, W):
    return (525.0 * W / 640, 525.0 * W / 640, W / 2.0, H / 2.0)


@functools.lru_cache(maxsize=None)
def frame(tag):
    """dict xyz (P x 3 float32), uv (P x 2 float32: what the oracle is given), uv_arg (the engine's: the same table, or None for the implicit grid), H, W, cam"""
    from dsac_amd import synth
    if tag == "A":
        fr = synth.chess_like_frame(37, 41, seed=_SEEDS[tag])
        p = np.arange(37 * 41, dtype=np.float64)
        jitter = np.stack([np.sin(1.7 * p + 0.3), np.cos(2.3 * p + 1.1)], -1) * 0.37  # sub-pixel, deterministic, no two cells alike
        uv = (fr["uv"].astype(np.float64) + jitter).astype(np.float32)
        fr = dict(fr, uv=uv, uv_arg=uv)
    elif tag == "B":
        fr = synth.chess_like_frame(24, 32, seed=_SEEDS[tag], cam=_grid_cam(24, 32), grid_uv=True)
        fr = dict(fr, uv_arg=None)
    elif tag == "C":
        fr = synth.chess_like_frame(40, 40, seed=_SEEDS[tag], cam=CAM_C, quantise_int16=True)
        fr = dict(fr, uv_arg=fr["uv"])
    elif tag == "D":
        fr = synth.chess_like_frame(3, 5, seed=_SEEDS[tag], cam=_grid_cam(3, 5), grid_uv=True, outlier_frac=0.0)
        fr = dict(fr, uv_arg=None)
    else:
        raise KeyError(tag)
    fr["xyz"] = np.ascontiguousarray(fr["xyz"], np.float32)
    fr["uv"] = np.ascontiguousarray(fr["uv"], np.float32)
    fr["xyz"].setflags(write=False)
    fr["uv"].setflags(write=False)
    return fr


def set_frame(engine, tag, xyz=None):
    """The frame as the engine gets it (B and D without a table of positions)."""
    fr = frame(tag)
    engine.set_frame(fr["xyz"] if xyz is None else xyz, fr["uv_arg"], fr["H"], fr["W"], fr["cam"])
    return fr


def checksum(tag):
    """A checksum of the frame's bytes (coordinates, positions, camera), for the fixture of tests/golden/make_dpnp_exact.py."""
    import zlib
    fr = frame(tag)
    return zlib.crc32(fr["xyz"].tobytes() + fr["uv"].tobytes() + np.asarray(fr["cam"], np.float64).tobytes()) & 0xFFFFFFFF


# ---- the oracle on one set ---------------------------------------------------------------------------------------------------------------------
def oracle_J(orc, fr, set4, eps=EPS, xyz=None):
    set4 = np.asarray(set4)
    return orc.dPNP(fr["uv"][set4], (fr["xyz"] if xyz is None else xyz)[set4], fr["cam"], eps=eps)


def rel(J, Jref):
    """max |J - Jref| / max(1, |Jref|max)"""
    return float(np.abs(np.asarray(J) - Jref).max() / max(1.0, np.abs(Jref).max()))


def sensitivity(orc, fr, set4, eps=EPS, J=None, xyz=None):
    """(J, sens): sens = the largest change of the oracle's J, relative to max(1, |J|max), over the 24 one-ulp moves of the set's float coordinates (a
    coordinate that is not finite -- the poisoned maps -- stays as it is).  A J that is not finite, or a run that is not, counts as infinite."""
    set4 = np.asarray(set4)
    uv4, X0 = fr["uv"][set4], (fr["xyz"] if xyz is None else xyz)[set4]
    if J is None:
        J = orc.dPNP(uv4, X0, fr["cam"], eps=eps)
    if not np.isfinite(J).all():
        return J, np.inf
    sc = max(1.0, float(np.abs(J).max()))
    worst = 0.0
    for c in range(12):
        for away in (np.float32(np.inf), np.float32(-np.inf)):
            X1 = X0.copy().reshape(-1)
            if not np.isfinite(X1[c]):
                continue
            X1[c] = np.nextafter(X1[c], away)
            d = np.abs(orc.dPNP(uv4, X1.reshape(4, 3), fr["cam"], eps=eps) - J).max()
            if not np.isfinite(d):
                return J, np.inf
            worst = max(worst, float(d))
    return J, worst / sc


def verdict(orc, fr, set4, eps=EPS, xyz=None):
    """dict set, eps, J, sens, bound, stable, zero (the oracle's J is exactly zero), robust_zero (and stays so under every one-ulp move)"""
    J, sens = sensitivity(orc, fr, set4, eps, xyz=xyz)
    bound = max(FLOOR, SENS_FACTOR * sens)
    zero = not J.any()
    return dict(set=np.asarray(set4, np.int32).copy(), eps=eps, J=J, sens=sens, bound=bound, stable=bool(bound <= UNSTABLE_ABOVE), zero=bool(zero),
                robust_zero=bool(zero and sens == 0.0))


# ---- the sets ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _accepted_sets(orc, tag, n=N_ACCEPTED, seed_offset=0):
    fr = frame(tag)
    _, sets, ok, _ = orc.sample(n, _SEEDS[tag] + 40 + seed_offset, fr["xyz"], fr["uv"], fr["H"], fr["W"], fr["cam"])
    assert ok.all(), "the oracle's sampler did not serve every hypothesis on frame %s" % tag
    sets.setflags(write=False)
    return sets


def accepted_sets(orc, tag):
    return _accepted_sets(orc, tag)


def _distinct_cells(rng, P, n):
    out = np.empty((n, 4), np.int32)
    for i in range(n):
        out[i] = rng.choice(P, size=4, replace=False)
    return out


@functools.lru_cache(maxsize=None)
def random_sets(tag):
    fr = frame(tag)
    sets = _distinct_cells(np.random.default_rng(_SEEDS[tag] + 80), fr["H"] * fr["W"], N_RANDOM)
    sets.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def _cases(orc, tag, kind, eps):
    fr = frame(tag)
    sets = accepted_sets(orc, tag) if kind == "accepted" else random_sets(tag)
    return tuple(verdict(orc, fr, s, eps) for s in sets)


def cases(orc, tag, kind, eps=EPS):
    """The verdicts of the frame's `accepted` or `random` sets at this step, in the sets' order (computed once, shared, left unchanged)."""
    return _cases(orc, tag, kind, float(eps))


def groups():
    """[(tag, kind, eps)] of everything the GPU test compares set by set"""
    out = [(tag, kind, EPS) for tag in TAGS for kind in ("accepted", "random")]
    return out + [("A", "accepted", e) for e in EXTRA_EPS]


# ---- zero ------------------------------------------------------------------------------------------------------------------------------------------
def search_zero(orc, tag, n=N_ZERO):
    """The first n random sets of four distinct cells (the stream of seed + 120) whose oracle J is exactly zero under the set itself and all 24 one-ulp moves"""
    fr = frame(tag)
    rng = np.random.default_rng(_SEEDS[tag] + 120)
    found = []
    while len(found) < n:
        s = _distinct_cells(rng, fr["H"] * fr["W"], 1)[0]
        J = oracle_J(orc, fr, s)
        if J.any():
            continue
        if sensitivity(orc, fr, s, J=J)[1] == 0.0:
            found.append(tuple(int(v) for v in s))
    return found


# ---- big -------------------------------------------------------------------------------------------------------------------------------------------
def perturbed_points(X0, c, side, eps=EPS, replay=True, own_round_trip=True):
    """The float coordinates of the solve (column c, side +1 / -1).  replay: the round trips of the coordinates in front of c, as the reference runs them;
    own_round_trip: the backward side is (v + eps) - 2 eps as in the reference, otherwise v - eps."""
    e = np.float32(eps)
    X = np.array(X0, np.float32).reshape(-1).copy()
    if replay:
        for cc in range(c):
            X[cc] = np.float32(np.float32(np.float32(X[cc] + e) - np.float32(2) * e) + e)
    if side > 0:
        X[c] = np.float32(X[c] + e)
    elif own_round_trip:
        X[c] = np.float32(np.float32(X[c] + e) - np.float32(2) * e)
    else:
        X[c] = np.float32(X[c] - e)
    return X.reshape(4, 3)


def divisor(eps):
    """2 * eps as the reference forms it: a float product, promoted"""
    return float(np.float32(2) * np.float32(eps))


def restated_J(orc, fr, set4, eps=EPS, replay=True, own_round_trip=True):
    """dPNP from orc.solve_p3p and orc.cv_to_jp6 on the points of perturbed_points.  With both switches on this IS orc.dPNP (the CPU test holds it to
    that, bit for bit); replay=False, own_round_trip=False is J_noreplay: every column from the pristine points, each side perturbed once."""
    set4 = np.asarray(set4)
    uv4, X0 = fr["uv"][set4], fr["xyz"][set4]
    J = np.zeros((6, 12))
    for c in range(12):
        side = []
        for sgn in (+1, -1):
            ok, pose = orc.solve_p3p(perturbed_points(X0, c, sgn, eps, replay, own_round_trip), uv4, fr["cam"])
            side.append(orc.cv_to_jp6(pose if ok else np.zeros(6)))
        J[:, c] = (side[0] - side[1]) / divisor(eps)
    if np.isnan(J).any():
        J[:] = 0.0
    return J


def classify_big(orc, fr, set4, J, eps=EPS):
    """The class of a big set by its steepest column: "one_sided", "switch" or "steep" (see the module docstring)."""
    set4 = np.asarray(set4)
    uv4, X0 = fr["uv"][set4], fr["xyz"][set4]
    c = int(np.argmax(np.abs(J).max(axis=0)))
    hi, lo = perturbed_points(X0, c, +1, eps), perturbed_points(X0, c, -1, eps)
    (ok_hi, p_hi), (ok_lo, p_lo) = orc.solve_p3p(hi, uv4, fr["cam"]), orc.solve_p3p(lo, uv4, fr["cam"])
    if ok_hi != ok_lo:
        return "one_sided"
    if not ok_hi:
        return "steep"  # cannot be: both sides the zero pose gives a zero column

    def pose_at(v):
        X = hi.copy().reshape(-1)
        X[c] = v
        ok, p = orc.solve_p3p(X.reshape(4, 3), uv4, fr["cam"])
        return orc.cv_to_jp6(p if ok else np.zeros(6))

    a, b = lo.reshape(-1)[c], hi.reshape(-1)[c]
    fa, fb = orc.cv_to_jp6(p_lo), orc.cv_to_jp6(p_hi)
    total = np.abs(fb - fa).max()
    # bisect on the half with the larger jump until a and b are adjacent floats
    while np.nextafter(a, np.float32(np.inf)) < b:
        m = np.float32(0.5 * (np.float64(a) + np.float64(b)))
        if not (a < m < b):
            break
        fm = pose_at(m)
        if np.abs(fm - fa).max() >= np.abs(fb - fm).max():
            b, fb = m, fm
        else:
            a, fa = m, fm
    return "switch" if np.abs(fb - fa).max() >= 0.5 * total else "steep"


def search_big(orc, tag, blocks):
    """[(block, set, class)] of the stable big sets among blocks of BIG_BLOCK random sets each (block b is the stream of (seed + 160, b))"""
    fr = frame(tag)
    found = []
    for b in blocks:
        sets = _distinct_cells(np.random.default_rng([_SEEDS[tag] + 160, int(b)]), fr["H"] * fr["W"], BIG_BLOCK)
        for s in sets:
            J = oracle_J(orc, fr, s)
            if not (np.isfinite(J).all() and np.abs(J).max() > BIG_ABOVE):
                continue
            if sensitivity(orc, fr, s, J=J)[1] <= BIG_SENS:
                found.append((int(b), tuple(int(v) for v in s), classify_big(orc, fr, s, J)))
    return found


# ---- poisoned --------------------------------------------------------------------------------------------------------------------------------------
POISON_KINDS = (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf))


@functools.lru_cache(maxsize=None)
def poisoned(orc):
    """Frame A with a NaN, a +inf or a -inf in one coordinate of one cell of each of 12 accepted sets (3 kinds x 4 sets; the MAP is modified, the sets are as
    sampled).  Returns dict xyz (the modified map), sets (12 x 4), kinds (12 names), J (the oracle's, 12 x 6 x 12), clean (the accepted sets that touch no
    modified cell).  The oracle's answer is taken twice and must be the same both times and finite."""
    fr = frame("A")
    sets = accepted_sets(orc, "A")
    xyz = fr["xyz"].copy()
    chosen, kinds, cells = [], [], set()
    for h, s in enumerate(sets):
        if len(chosen) == 12:
            break
        if len(set(s.tolist())) < 4 or any(int(p) in cells for p in s):
            continue
        k = len(chosen)
        name, value = POISON_KINDS[k // 4]
        cell, axis = int(s[k % 4]), k % 3  # every position in the set and every axis takes its turn
        xyz[cell, axis] = value
        cells.add(cell)
        chosen.append(h)
        kinds.append(name)
    assert len(chosen) == 12
    J = np.stack([oracle_J(orc, fr, sets[h], xyz=xyz) for h in chosen])
    again = np.stack([oracle_J(orc, fr, sets[h], xyz=xyz) for h in chosen])
    clean = np.array([h for h in range(len(sets)) if not any(int(p) in cells for p in sets[h])], np.int64)
    xyz.setflags(write=False)
    return dict(xyz=xyz, sets=sets[chosen].copy(), kinds=tuple(kinds), J=J, reproducible=bool(np.array_equal(J, again, equal_nan=True)),
                clean=sets[clean].copy(), cells=tuple(sorted(cells)))


# ---- replay ----------------------------------------------------------------------------------------------------------------------------------------
def replay_candidates(orc, n=512):
    """Accepted sets of the replay frame beyond the 64 of `accepted` (the sampler's next seed)"""
    return _accepted_sets(orc, REPLAY_TAG, n, 1)


def replay_case(orc, set4):
    """The verdict of a set on the replay frame with J_noreplay (every column from the pristine points, each side perturbed once), J_lane (the coordinates in
    front of a column pristine, the column's own two sides as the reference runs them: what k_dpnp computes without its `cc < c` line) and their distances
    from the oracle's J."""
    fr = frame(REPLAY_TAG)
    v = verdict(orc, fr, set4, REPLAY_EPS)
    v["J_noreplay"] = restated_J(orc, fr, set4, REPLAY_EPS, replay=False, own_round_trip=False)
    v["J_lane"] = restated_J(orc, fr, set4, REPLAY_EPS, replay=False, own_round_trip=True)
    v["d_noreplay"], v["d_lane"] = rel(v["J_noreplay"], v["J"]), rel(v["J_lane"], v["J"])
    v["matters"] = bool(v["stable"] and v["d_noreplay"] >= REPLAY_FACTOR * max(REPLAY_FLOOR, SENS_FACTOR * v["sens"]))
    v["lane_matters"] = bool(v["d_lane"] >= max(LANE_FLOOR, v["sens"]))
    return v


def search_replay(orc, n=512, keep=37):
    """The first `keep` candidates on which both forms of the replay matter"""
    out = []
    for s in replay_candidates(orc, n):
        c = replay_case(orc, s)
        if c["matters"] and c["lane_matters"] and len(out) < keep:
            out.append(tuple(int(p) for p in s))
    return out


@functools.lru_cache(maxsize=None)
def replay_cases(orc):
    return tuple(replay_case(orc, s) for s in REPLAY)


@functools.lru_cache(maxsize=None)
def zero_cases(orc, tag):
    return tuple(verdict(orc, frame(tag), s) for s in ZERO[tag])


@functools.lru_cache(maxsize=None)
def big_cases(orc, tag):
    out = []
    for block, s, cls in BIG[tag]:
        v = verdict(orc, frame(tag), s)
        v["cls"], v["block"] = cls, block
        out.append(v)
    return tuple(out)


# ---- frozen lists (python tests/dpnp_corpus.py prints them) -------------------------------------------------------------------------------------------
ZERO = {
    "A": [(406, 1085, 256, 1330), (1340, 466, 1105, 750), (415, 1198, 811, 1295), (139, 491, 1437, 248), (319, 585, 992, 1516), (517, 1049, 1278, 1463),
          (1339, 308, 1424, 102), (1478, 713, 532, 1016), (282, 8, 973, 849), (1274, 404, 534, 563), (815, 1463, 195, 1018), (114, 788, 10, 1095),
          (1409, 31, 875, 519), (1384, 614, 132, 1006), (330, 942, 710, 955), (839, 408, 239, 939)],
    "B": [(366, 741, 100, 85), (660, 559, 517, 706), (738, 274, 689, 573), (291, 663, 25, 402), (30, 104, 593, 567), (256, 574, 354, 50),
          (140, 99, 705, 220), (499, 385, 747, 105), (6, 403, 117, 643), (215, 310, 628, 330), (307, 648, 629, 89), (446, 1, 197, 342),
          (760, 94, 114, 270), (381, 458, 425, 436), (762, 711, 33, 107), (581, 337, 424, 289)],
    "C": [(1105, 1479, 516, 974), (35, 1572, 387, 41), (182, 1190, 735, 797), (470, 1340, 50, 823), (1413, 1070, 39, 1085), (697, 1576, 328, 36),
          (1540, 20, 793, 136), (1035, 464, 1460, 1388), (845, 706, 1569, 496), (649, 221, 717, 613), (847, 992, 1058, 544), (634, 1125, 1459, 1194),
          (75, 486, 249, 988), (379, 1223, 1249, 832), (798, 665, 649, 186), (477, 129, 1137, 605)],
}
# (block, set, class).  Kept from the 200 blocks of the budget: every one_sided find, and the switch finds of blocks 0 - 49.
BIG = {
    "A": [(10, (319, 304, 972, 928), "one_sided"), (12, (586, 851, 229, 309), "switch"), (18, (621, 526, 1130, 915), "switch"),
          (20, (298, 433, 384, 1475), "switch"), (20, (340, 1277, 105, 698), "switch"), (21, (1079, 518, 413, 1420), "switch"),
          (22, (965, 1121, 1461, 542), "switch"), (25, (211, 217, 52, 409), "switch"), (37, (1302, 202, 170, 1202), "switch"),
          (44, (985, 453, 1100, 1175), "switch"), (44, (224, 588, 1367, 569), "switch"), (47, (994, 1321, 413, 1443), "switch"),
          (94, (1082, 986, 1347, 694), "one_sided"), (106, (1060, 1115, 1328, 1131), "one_sided"), (134, (271, 1204, 384, 330), "one_sided"),
          (146, (163, 644, 1380, 106), "one_sided"), (154, (636, 999, 1316, 479), "one_sided"), (166, (137, 295, 491, 777), "one_sided"),
          (171, (987, 491, 142, 72), "one_sided")],
    "C": [(0, (444, 1201, 1300, 449), "switch"), (2, (280, 540, 689, 542), "switch"), (6, (1505, 1475, 1398, 1348), "switch"),
          (10, (335, 196, 369, 1509), "switch"), (11, (29, 1567, 222, 1128), "one_sided"), (13, (1001, 1502, 1093, 835), "switch"),
          (17, (1382, 976, 150, 1532), "switch"), (26, (542, 1025, 241, 230), "switch"), (27, (1212, 303, 71, 820), "switch"),
          (29, (1507, 1162, 934, 1025), "switch"), (33, (339, 121, 437, 723), "one_sided"), (35, (884, 712, 990, 398), "switch"),
          (39, (709, 92, 699, 763), "one_sided"), (42, (510, 1555, 730, 886), "switch"), (49, (106, 717, 144, 454), "switch"),
          (83, (738, 702, 56, 838), "one_sided"), (130, (354, 412, 510, 636), "one_sided"), (137, (1582, 100, 873, 906), "one_sided"),
          (168, (927, 952, 277, 501), "one_sided"), (193, (94, 244, 878, 1115), "one_sided")],
}
BIG_NOTE = """The full budget (200 blocks of 1000 random sets per frame) finds 40 stable big sets on frame A (8 one_sided, 32 switch) and 51 on frame C
(8 one_sided, 43 switch).  The class "steep" -- |J|max > 1e3 with both sides solved and no jump between adjacent floats -- has NO stable member within the
budget on either frame: a Jacobian that steep without a discontinuity behind it moves by more than 1e-4 of its scale under a one-ulp move."""
# The first 37 of the 512 candidates that satisfy search_replay's two rules (the issue's, and d_lane >= max(1e-7, sens))
REPLAY = ((990, 595, 269, 1367), (892, 721, 457, 761), (1484, 980, 387, 897), (942, 567, 894, 858), (207, 563, 1441, 1412), (682, 802, 642, 65),
          (637, 331, 443, 651), (246, 216, 418, 1057), (1238, 175, 561, 263), (443, 160, 271, 396), (745, 1175, 1095, 1301), (25, 1516, 818, 1189),
          (914, 1471, 556, 550), (481, 255, 1351, 1236), (705, 1139, 270, 42), (29, 717, 1340, 485), (120, 1476, 305, 1233), (83, 761, 1300, 318),
          (62, 1158, 611, 442), (1358, 388, 234, 1203), (743, 313, 220, 302), (17, 207, 1132, 472), (1285, 420, 519, 277), (285, 347, 800, 1449),
          (1386, 264, 917, 25), (1114, 286, 1078, 312), (1139, 263, 1098, 500), (433, 648, 995, 144), (1175, 534, 67, 819), (1417, 387, 1000, 1080),
          (474, 892, 1217, 786), (900, 460, 324, 180), (1511, 79, 389, 636), (76, 1098, 1471, 783), (939, 1386, 238, 155), (732, 1396, 1125, 303),
          (99, 1510, 887, 1349))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as o
    o.build()
    what = sys.argv[1]
    if what == "zero":
        print("ZERO = {")
        for t in ("A", "B", "C"):
            print('    "%s": %r,' % (t, search_zero(o, t)))
        print("}")
    elif what == "big":  # python tests/dpnp_corpus.py big A 0 200
        t, b0, b1 = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        for b in range(b0, b1):
            for row in search_big(o, t, [b]):
                print("%s %r," % (t, row), flush=True)
    elif what == "replay":
        print("REPLAY = %r" % (tuple(search_replay(o)),))
