"""Guided RGB-D sampling without a device: header, binding and export map carry the three calls, and the restatement the GPU tests compare against
(tests/rgbd_guided_ref.py) does what include/dsac_hip.h states -- the mask is applied before the normalisation, a cell without mass is never returned, fewer than
three cells of mass yield no set -- and tells four planted mistakes apart on the corpus the GPU tests run, so that those comparisons can fail."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import guided_ref as gr
import rgbd_guided_ref as g3
import rgbd_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"dsac_set_sampling_weights_rgbd": ["dsac_ctx* ctx", "const float* weights_or_null"],
        "dsac_sampling_table_rgbd": ["dsac_ctx* ctx", "uint64_t* cdf_out"],
        "dsac_sampling_weights_backward_rgbd": ["dsac_ctx* ctx", "int N", "const int32_t* sets", "const uint8_t* ok", "const double* g", "double* grad_w"]}


def _header_decl(name):
    txt = open(os.path.join(ROOT, "include", "dsac_hip.h")).read()
    m = re.search(r"DSAC_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in include/dsac_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_binding_and_export_map_carry_the_calls():
    from dsac_amd import capi
    globs = re.findall(r"^\s*([A-Za-z_*][\w*]*);", open(os.path.join(ROOT, "dsac_amd", "csrc", "exports.map")).read().split("local:")[0], re.M)
    for name, want in WANT.items():
        args = _header_decl(name)
        assert args == want
        assert getattr(capi.lib, name).argtypes == [C.c_void_p if "*" in a else C.c_int for a in args]
        assert name in capi.EXPORTS
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "exports.map does not export %s" % name


def test_null_context_is_rejected_without_crashing():
    from dsac_amd import capi
    w = np.ones(4, np.float32)
    assert capi.lib.dsac_set_sampling_weights_rgbd(None, w.ctypes.data) == capi.DSAC_ERR_INVALID
    assert capi.lib.dsac_sampling_table_rgbd(None, None) == capi.DSAC_ERR_INVALID
    assert capi.lib.dsac_sampling_weights_backward_rgbd(None, 1, None, None, None, None) == capi.DSAC_ERR_INVALID


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------
def _normalise_then_mask(w, valid):
    """planted mistake: the masses of the 2D rule on w itself, the cells that are not VALID zeroed afterwards"""
    m = gr.build_table(w)[4].copy()
    m[~valid] = 0
    return np.cumsum(m, dtype=np.uint64)


@pytest.mark.parametrize("H,W", [(40, 40), (37, 53), (3, 5)])
def test_the_mask_is_applied_before_the_normalisation(H, W):
    xyz, cam, v = g3.frame(H, W)
    v = v[0]
    assert 0 < (~v).sum() < v.size
    ones, holes = g3.build_table(g3.w_ones(v), v), g3.build_table(g3.w_on_holes(v), v)
    assert np.array_equal(ones[0], holes[0]) and ones[1] == holes[1] == int(v.sum()) << 24 and ones[2] == holes[2] == int(v.sum())
    assert holes[3] == pytest.approx(1e-3 * v.sum(), rel=1e-6)  # S' sums the weights as given, not the masses
    # the planted mistake gives another table: the measured cells keep floor(1e-3 * 2^24) units each
    wrong = _normalise_then_mask(g3.w_on_holes(v), v)
    assert not np.array_equal(wrong, holes[0]) and int(wrong[-1]) == int(v.sum()) * int(np.floor(np.float64(np.float32(1e-3)) * 16777216.0))


def test_cells_without_mass_are_never_returned():
    xyz, cam, v = g3.frame(40, 40)
    v = v[0]
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 1 << 64, 20000, dtype=np.uint64)
    vals[:3] = (0, (1 << 64) - 1, 1 << 63)
    for name in ("ones", "mask01", "heavy", "mixed", "on_holes", "three", "lopsided"):
        w = g3.PATTERNS[name](v)
        C_, T, n, S, m = g3.build_table(w, v)
        assert n >= 3 and not m[~v].any(), name
        cells = gr.cell_of(C_, T, vals)
        assert (m[cells] > 0).all() and v[cells].all(), name
        if name == "three":  # a three-cell table only ever returns those three cells
            keep = np.flatnonzero(v)[[3, 400, 900]]
            assert set(cells.tolist()) == set(keep.tolist()) and n == 3
            assert np.flatnonzero(m).tolist() == keep.tolist() and m[keep].tolist() == [(1 << 24) // 3, (1 << 25) // 3, 1 << 24]
            sets, used = g3.attempt_sets3(C_, T, n, 7, 8, 8)
            for row in sets:
                for s in row:
                    assert s is None or sorted(s) == keep.tolist()


def test_fewer_than_three_cells_of_mass_yield_no_set():
    xyz, cam, v = g3.frame(40, 40)
    v = v[0]
    C_, T, n, S, m = g3.build_table(g3.w_two(v), v)
    assert n == 2 and T == (1 << 24) + (1 << 23) and S == 1.5  # the weight on the five holes counts for nothing
    assert g3.attempt_sets3(C_, T, n, 3, 4, 4)[0] is None
    p, s, ok, st = g3.sample_frame(g3.w_two(v), v, 3, 4, 4, None)
    assert not p.any() and not s.any() and not ok.any() and st["fail_zero"] == 4
    # the rule itself, with the n' < 3 shortcut taken away: two cells of mass exhaust the 32 candidates of every attempt
    sets, used = g3.attempt_sets3(C_, T, 3, 3, 4, 4)
    assert all(s is None for row in sets for s in row)


# ---- the corpus: what the walk meets, and the planted mistakes ---------------------------------------------------------------------------------------
_RESULTS = {}


def _run(case, walk=g3.walk3):
    """the case with numpy Kabsch as the evaluator: per frame (poses, sets, ok, stats)"""
    key = (case, walk.__name__)
    if key not in _RESULTS:
        H, W, F, Nf, A, stride, thr, pats, clean = case
        xyz, cam, v, w = g3.case_inputs(case)
        canon = rr.canonical(xyz, cam)[0]
        _RESULTS[key] = [g3.sample_frame(w[f], v[f], g3.SEED + f * stride, Nf, A, g3.kabsch_evaluator(xyz[f], canon[f], thr), walk) for f in range(F)]
    return _RESULTS[key]


def _case(pattern, where=None):
    """the first case of that pattern; where: {field index of the case tuple: value}"""
    return next(c for c in g3.CASES if c[7] == (pattern,) and all(c[i] == x for i, x in (where or {}).items()))


def test_the_corpus_meets_every_branch():
    total = dict(redraw=0, undrawn=0, late=0, fail_drawn=0, fail_zero=0)
    for case in g3.CASES:
        xyz, cam, v, w = g3.case_inputs(case)
        for f, (poses, sets, ok, st) in enumerate(_run(case)):
            for k in total:
                total[k] += st[k]
            m = g3.build_table(w[f], v[f])[4]
            rows = sets[sets.any(axis=1)]
            assert v[f][rows].all() and (m[rows] > 0).all(), "a reported set holds a cell that is not VALID or has no mass"
            assert not poses[ok == 0].any()
    print("guided RGB-D corpus, numpy Kabsch:", total)
    assert all(total[k] > 0 for k in total), total
    heavy = _run(_case("heavy", {0: 37}))[0][3]
    assert heavy["redraw"] > 0 and heavy["late"] > 0 and heavy["fail_drawn"] > 0, heavy
    three = _run(_case("three", {8: False}))[0][3]
    assert three["undrawn"] > 0 and three["fail_zero"] > 0, three
    lop = _run(_case("lopsided"))[0]
    assert lop[3]["fail_zero"] == 64 and lop[3]["undrawn"] == 64 * 70 and not lop[1].any()
    tight = _run(_case("mask01", {6: 1e-9}))[0]
    assert tight[3]["fail_drawn"] == 65 and not tight[2].any()
    clean = _run(_case("three", {8: True}))[0]
    assert clean[2].sum() + clean[3]["fail_zero"] == 64  # exact data: every drawn attempt is accepted
    batch = _run(next(c for c in g3.CASES if c[2] == 3))
    assert batch[1][3]["fail_zero"] == 128 and batch[0][2].any() and batch[2][2].any()


def _walk_restart(cells, limit=32):
    """planted mistake: a repeated candidate restarts the set at that candidate instead of being skipped"""
    got = []
    for k in range(limit):
        c = int(cells[k])
        got = [c] if c in got else got + [c]
        if len(got) == 3:
            return got, k + 1
    return None, limit


def _walk_31(cells, limit=32):
    """planted mistake: the attempt fails after 31 candidates"""
    return g3.walk3(cells, 31)


@pytest.mark.parametrize("walk", [_walk_restart, _walk_31])
def test_planted_walk_mistakes_change_a_result_of_the_corpus(walk):
    changed = []
    for case in g3.CASES:
        if case[7][0] not in ("heavy", "three"):
            continue
        for good, bad in zip(_run(case), _run(case, walk)):
            if not (np.array_equal(good[1], bad[1]) and np.array_equal(good[2], bad[2])):
                changed.append(case)
    assert changed, "the corpus cannot tell %s from the rule" % walk.__name__


def test_planted_uniform_term_changes_the_gradient():
    case = _case("heavy", {0: 37})
    xyz, cam, v, w = g3.case_inputs(case)
    poses, sets, ok, st = _run(case)[0]
    S = g3.build_table(w[0], v[0])[3]
    g = np.random.default_rng(5).normal(size=len(ok))
    right = g3.backward_ref3(w[0], v[0], S, sets, ok, g)
    wrong = g3.backward_ref3(w[0], v[0], S, sets, ok, g, uniform=4.0)
    mass = gr.valid_cells(g3.masked_weights(w[0], v[0]))
    bound = (right[2] + 4) * 2.0 ** -53 * right[1] + v[0].size * 2.0 ** -53 * right[3]  # the GPU test's per-cell bound
    assert (np.abs(right[0] - wrong[0])[mass] > bound[mass]).all()
    assert not right[0][~mass].any() and not wrong[0][~mass].any()
