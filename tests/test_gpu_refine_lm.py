"""K6's Levenberg-Marquardt (lm_pnp in k_refine.hip) off its easy path, against the CPU oracle.

tests/test_gpu_refine.py refines from next to the right pose: about three accepted iterations per call and hardly a rejected trial.  This file owns the
branches those runs never take: a rejected trial (lambda x10, the state restored), runs of 15 and more rejections, lambda at 1e0 and above, the forced
accept when a rejection would take lambda past 1e16, the 20-iteration cap, the zero step that stands in for a damped matrix that is not positive
definite, and the two call sites of lm_pnp (the fused k_refine<S> and k_refine_lm behind k_refine_walk).

The problems come from tests/lm_corpus.py (128 x 128 maps, thr = 120 above the error clamp: a step's list is the first 100 finite cells of its
permutation row, far starts).  The oracle labels every problem by its own LM statistics and gives it a stability verdict from re-runs under perturbations
that are equivalent in exact arithmetic (tests/test_lm_corpus_cpu.py holds the corpus to its conditions); nothing measured on the GPU enters either.

Tolerance, as in tests/test_gpu_refine.py: both sides run the same fp64 arithmetic, so a stable problem's refined pose agrees to rtol 1e-7, atol 1e-9
and step counts and inlier maps are identical.  Across launch forms of the GPU the results are bit-identical, stable or not.
"""
import numpy as np
import pytest

import lm_corpus
from conftest import margin

pytestmark = pytest.mark.gpu

H, W, P = lm_corpus.H, lm_corpus.W, lm_corpus.P
KW = dict(max_inl=lm_corpus.MAX_INL, min_inl=lm_corpus.MIN_INL, thr=lm_corpus.THR)
FORMS = (1, 2, 4, 8, 0)  # "k6_waves": the fused kernel with 1 / 2 / 4 / 8 waves per problem; 0 = by the problem count (the two-launch step when it qualifies)


def _rel(got, ref):
    return np.abs(got - ref).max(-1) / np.maximum(1.0, np.abs(ref).max(-1))


def _fused(engine, fn):
    engine.set_option("k6_waves", 1)
    try:
        return fn()
    finally:
        engine.set_option("k6_waves", 0)


def _all_forms(engine, B, init, perm, what):
    """refineAll under every launch form: poses, step counts and inlier maps must be the same bits.  Returns the fused one-wave result."""
    # refine_split_applies (kernels.h): "k6_waves" 0, >= 32 problems, >= 16 384 cells, no perturbation, no fused loss -> form 0 is k_refine_walk + k_refine_lm
    assert B >= 32 and init.shape[0] == B and engine.P >= 16384 and engine.get_option("k6_waves") == 0
    res = {}
    try:
        for waves in FORMS:
            engine.set_option("k6_waves", waves)
            res[waves] = engine.refineAll(init, perm, want_inlier_maps=True, **KW)
    finally:
        engine.set_option("k6_waves", 0)
    for waves in FORMS[1:]:
        for a, b, name in zip(res[1], res[waves], ("poses", "steps_done", "inlier maps")):
            assert np.array_equal(a, b, equal_nan=True), "%s: %s of k6_waves %d differ from k6_waves 1" % (what, name, waves)
    return res[1]


def _expected_map(perm, steps_done):
    """thr above the clamp on a finite map: the map counts the first MAX_INL cells of every finished row."""
    m = np.zeros(P, np.int32)
    for s in range(steps_done):
        np.add.at(m, perm[s, :lm_corpus.MAX_INL], 1)
    return m


@pytest.mark.parametrize("name,steps", [(n, s) for n in lm_corpus.MAPS for s in lm_corpus.STEPS])
def test_fused_kernel_against_the_oracle(engine, orc, name, steps):
    """(a) k_refine<1> on every stable problem, a quarter of them with a replica perturbation on a cell of step 0's list."""
    g = lm_corpus.corpus(orc)[(name, steps)]
    fr, perm, init, stable = g["frame"], g["perm"], g["init"], g["stable"]
    engine.set_frame(fr["xyz"], None, H, W, fr["cam"])
    got, sd = _fused(engine, lambda: engine.refine(init, perm, pert_px_c=g["px"], pert_value=g["val"], **KW))
    rel = _rel(got, g["ref"])
    with np.errstate(invalid="ignore"):
        rel = np.where(np.isfinite(rel), rel, np.inf)
    idx = np.flatnonzero(stable)
    assert len(idx) >= 64 - lm_corpus.MAX_UNSTABLE
    print("%s x %d steps: %d stable problems (%d with a replica perturbation); unstable ones (not asserted) differ by up to %.3e" %
          (name, steps, len(idx), int((g["px"][idx, 0] >= 0).sum()), rel[~stable].max() if (~stable).any() else 0.0))
    worst = {}
    for l in lm_corpus.LABELS + ("any",):
        sel = [b for b in idx if l == "any" or l in g["labels"][b]]
        if sel:
            worst[l] = (len(sel), float(rel[sel].max()), int(sel[int(np.argmax(rel[sel]))]))
            print("    label %-15s %2d problems, worst max |d| / max(1, |pose|) %.3e (problem %d)" % ((l,) + worst[l]))
    assert np.array_equal(sd[idx], g["sd"][idx]) and np.all(sd[idx] == steps)
    for l, (n, w, _) in worst.items():
        margin("a6", "K6 LM off the easy path (%s map, %d steps, stable problems labelled '%s'): refined pose vs oracle, max |d| / max(1, |pose|)" % (name, steps, l), w, 1e-7)
    assert np.allclose(got[idx], g["ref"][idx], rtol=1e-7, atol=1e-9)
    # inlier maps of 8 stable problems without a perturbation: the oracle's, which is 1 (+ 1 per repeat) on exactly the first 100 cells of every row
    pick = [b for b in idx if g["px"][b, 0] < 0][:8]
    assert len(pick) == 8
    _, sd8, maps = _fused(engine, lambda: engine.refineAll(init[pick], perm, want_inlier_maps=True, **KW))
    for i, b in enumerate(pick):
        _, imap_r, sd_r = orc.refine(init[b], perm, fr["xyz"], fr["uv"], H, W, fr["cam"], inlier_count=lm_corpus.MAX_INL, min_inliers=lm_corpus.MIN_INL,
                                     thr=lm_corpus.THR, want_inlier_map=True)
        assert sd8[i] == sd_r[0] == steps
        assert np.array_equal(maps[i], imap_r) and np.array_equal(imap_r, _expected_map(perm, steps)), b


@pytest.mark.parametrize("name", list(lm_corpus.MAPS))
def test_every_launch_form_runs_the_same_machine(engine, orc, name):
    """(b) the whole corpus, chaotic problems included (bit equality needs no stability, and they probe it hardest): k_refine<1, 2, 4, 8> and
    k_refine_walk + k_refine_lm."""
    g = lm_corpus.corpus(orc)[(name, 8)]
    fr = g["frame"]
    engine.set_frame(fr["xyz"], None, H, W, fr["cam"])
    for steps in lm_corpus.STEPS:
        poses, sd, maps = _all_forms(engine, 64, g["init"], g["perm"][:steps], "%s x %d steps" % (name, steps))
        for b in range(64):  # whatever a chaotic problem ends as, its map is the lists of the steps it finished
            assert np.array_equal(maps[b], _expected_map(g["perm"], int(sd[b]))), b


@pytest.mark.parametrize("steps", [2, 3, 4])
def test_fixed_point_forced_accept(engine, orc, steps):
    """(c) the same permutation row in successive steps: the third call starts on the fixed point of the first two, rejects 19 trials in a row and is
    force-accepted at the lambda ceiling (tests/test_lm_corpus_cpu.py asserts that of the oracle's run).  Four copies of the eight starts make the
    32 problems from which "k6_waves" 0 takes the two-launch step."""
    fp = lm_corpus.fixed_point(orc)
    fr, perm, run = fp["frame"], fp["perm"][:steps], fp["runs"][steps]
    engine.set_frame(fr["xyz"], None, H, W, fr["cam"])
    init = np.tile(fp["init"], (4, 1))
    poses, sd, maps = _all_forms(engine, 32, init, perm, "fixed point, %d steps" % steps)
    assert np.array_equal(poses[:8], poses[8:16]) and np.array_equal(poses[:8], poses[24:])
    assert np.array_equal(sd[:8], run["sd"]) and np.all(sd == steps)
    margin("a6", "K6 LM on the fixed point (clean map, one permutation row for every step, %d steps): refined pose vs oracle, max |d| / max(1, |pose|)" % steps,
           _rel(poses[:8], run["ref"]).max(), 1e-7)
    assert np.allclose(poses[:8], run["ref"], rtol=1e-7, atol=1e-9)
    assert np.array_equal(maps[0], _expected_map(perm, steps))


def _near_starts(fr, B=32, seed=5):
    rng = np.random.default_rng(seed)
    return fr["gt_pose"][None, :] + rng.normal(size=(B, 6)) * 0.01 * np.array([1.0, 1.0, 1.0, 1000.0, 1000.0, 1000.0])


def _oracle(orc, fr, xyz, init, perm, maps_of=()):
    kw = dict(inlier_count=lm_corpus.MAX_INL, min_inliers=lm_corpus.MIN_INL, thr=lm_corpus.THR)
    ref, sd = orc.refine(init, perm, xyz, fr["uv"], H, W, fr["cam"], **kw)
    maps = {b: orc.refine(init[b], perm, xyz, fr["uv"], H, W, fr["cam"], want_inlier_map=True, **kw)[1] for b in maps_of}
    return ref, sd, maps


def test_degenerate_all_zero_map(engine, orc):
    """(d) every coordinate zero: the rotation columns of the normal equations vanish, the oracle's elimination meets a zero pivot and the kernel's
    L D L^T a pivot that is not positive -- both take a zero step, the trial equals the start and ends the call.  Three steps, the start's own bits."""
    fr = lm_corpus.frame("clean")
    xyz = np.zeros((P, 3), np.float32)
    perm = lm_corpus.permutations()[:3]
    init = lm_corpus.starts("clean")[:32]
    ref, sd_r, _ = _oracle(orc, fr, xyz, init, perm)
    assert np.array_equal(ref, init) and np.all(sd_r == 3)
    engine.set_frame(xyz, None, H, W, fr["cam"])
    poses, sd, maps = _all_forms(engine, 32, init, perm, "all-zero map")
    assert np.array_equal(poses, init) and np.all(sd == 3)
    assert np.array_equal(maps[0], _expected_map(perm, 3))


def test_degenerate_inf_coordinate_among_the_first_cells(engine, orc):
    """(d) one infinite coordinate inside step 1's first 100 cells.  In the reference's arithmetic all three camera coordinates of that cell are
    infinite, 1 / Z is zero and inf x 0 makes its residual NaN: the cell is no inlier at any threshold and step 1's list closes with the row's 101st
    cell (the oracle's inlier map says so; this is asserted of the oracle before the GPU is looked at).  Three steps, a finite pose, the same inlier
    maps, the pose within the file's tolerance."""
    fr = lm_corpus.frame("clean")
    perm = lm_corpus.permutations()[:3]
    cell = int([c for c in perm[1, :lm_corpus.MAX_INL] if c not in set(perm[0, :lm_corpus.MAX_INL].tolist())][10])
    xyz = fr["xyz"].copy()
    xyz[cell, 0] = np.inf
    init = _near_starts(fr)
    ref, sd_r, maps_r = _oracle(orc, fr, xyz, init, perm, maps_of=(0, 1, 2, 3))
    assert np.all(sd_r == 3) and np.isfinite(ref).all()
    assert maps_r[0][cell] == 0 and maps_r[0][perm[1, lm_corpus.MAX_INL]] >= 1 and maps_r[0].sum() == 300
    engine.set_frame(xyz, None, H, W, fr["cam"])
    poses, sd, maps = _all_forms(engine, 32, init, perm, "one inf coordinate")
    assert np.array_equal(sd, sd_r)
    for b, m in maps_r.items():
        assert np.array_equal(maps[b], m), b
    margin("a6", "K6 LM with an infinite coordinate among step 1's first 100 cells (3 steps): refined pose vs oracle, max |d| / max(1, |pose|)", _rel(poses, ref).max(), 1e-7)
    assert np.allclose(poses, ref, rtol=1e-7, atol=1e-9)


def test_degenerate_nan_cells_at_the_head_of_a_row(engine, orc):
    """(d) NaN in the first 50 cells of row 0: no inliers, so step 0's list is the next 100 cells."""
    fr = lm_corpus.frame("clean")
    perm = lm_corpus.permutations()[:3]
    xyz = fr["xyz"].copy()
    xyz[perm[0, :50]] = np.nan
    init = _near_starts(fr, seed=6)
    ref, sd_r, maps_r = _oracle(orc, fr, xyz, init, perm, maps_of=(0, 1, 2, 3))
    assert np.all(sd_r == 3) and np.isfinite(ref).all()
    step0 = np.zeros(P, np.int32)
    step0[perm[0, 50:150]] = 1
    bad = np.zeros(P, bool)
    bad[perm[0, :50]] = True
    assert np.all(maps_r[0][bad] == 0) and np.all(maps_r[0] >= step0) and maps_r[0].sum() == 300
    engine.set_frame(xyz, None, H, W, fr["cam"])
    poses, sd, maps = _all_forms(engine, 32, init, perm, "NaN cells")
    assert np.array_equal(sd, sd_r)
    for b, m in maps_r.items():
        assert np.array_equal(maps[b], m), b
    margin("a6", "K6 LM with NaN cells at the head of row 0 (3 steps): refined pose vs oracle, max |d| / max(1, |pose|)", _rel(poses, ref).max(), 1e-7)
    assert np.allclose(poses, ref, rtol=1e-7, atol=1e-9)


def test_degenerate_every_cell_the_same_point(engine):
    """(d) one 3-D point in every cell: rank-deficient normal equations, the oracle walks to an arbitrary pose and no parity is claimed.  Every launch
    form returns finite numbers, at most three steps, and the bits of every other form."""
    fr = lm_corpus.frame("clean")
    xyz = np.tile(np.array([[120.0, -340.0, 2100.0]], np.float32), (P, 1))
    perm = lm_corpus.permutations()[:3]
    init = _near_starts(fr, seed=7)
    engine.set_frame(xyz, None, H, W, fr["cam"])
    poses, sd, maps = _all_forms(engine, 32, init, perm, "every cell the same point")
    assert np.isfinite(poses).all() and np.all(sd <= 3) and np.all(sd >= 0)
