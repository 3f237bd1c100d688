"""Guided sampling without a device: header, binding and export map carry the three calls, and the restatement the GPU tests compare against
(tests/guided_ref.py) does what include/dsac_hip.h states -- on a 5-cell table exactly m_p of the T values of t land in cell p, a cell without mass is
never returned, a table with fewer than four cells of mass yields no set, and the vectorised multiply-high equals the Python-integer one."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np

import guided_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsac_set_sampling_weights", "dsac_sampling_table", "dsac_sampling_weights_backward")


def _header_decl(name):
    txt = open(os.path.join(ROOT, "include", "dsac_hip.h")).read()
    m = re.search(r"DSAC_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in include/dsac_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_binding_and_export_map_carry_the_calls():
    from dsac_amd import capi
    want = {"dsac_set_sampling_weights": ["dsac_ctx* ctx", "const float* weights_or_null"],
            "dsac_sampling_table": ["dsac_ctx* ctx", "uint64_t* cdf_out"],
            "dsac_sampling_weights_backward": ["dsac_ctx* ctx", "int N", "const int32_t* sets", "const uint8_t* ok", "const double* g", "double* grad_w"]}
    globs = re.findall(r"^\s*([A-Za-z_*][\w*]*);", open(os.path.join(ROOT, "dsac_amd", "csrc", "exports.map")).read().split("local:")[0], re.M)
    for name in NAMES:
        args = _header_decl(name)
        assert args == want[name]
        assert getattr(capi.lib, name).argtypes == [C.c_void_p if "*" in a else C.c_int for a in args]
        assert name in capi.EXPORTS
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "exports.map does not export %s" % name


def test_null_context_is_rejected_without_crashing():
    from dsac_amd import capi
    w = np.ones(4, np.float32)
    assert capi.lib.dsac_set_sampling_weights(None, w.ctypes.data) == capi.DSAC_ERR_INVALID
    assert capi.lib.dsac_sampling_table(None, None) == capi.DSAC_ERR_INVALID
    assert capi.lib.dsac_sampling_weights_backward(None, 1, None, None, None, None) == capi.DSAC_ERR_INVALID


def test_multiply_high_halves_equal_python_integers():
    rng = np.random.default_rng(5)
    v = rng.integers(0, 1 << 64, 4096, dtype=np.uint64)
    v[:4] = (0, 1, (1 << 64) - 1, 1 << 63)
    for T in (1, 5, (1 << 24), (1 << 32) - 1, (1 << 32) + 7, 66049 << 24, (1 << 54) - 3):
        assert np.array_equal(gr.t_of(v, T), gr.t_of_int(v, T)), T


def test_five_cell_table_sends_m_p_values_of_t_to_cell_p():
    # the maximum 16.0 has 2^24 units, a weight k * 2^-20 has floor(k * 2^-20 / 16 * 2^24) = k
    w = np.array([3, 0, 5, 0, 1], np.float32) * np.float32(2.0 ** -20)
    w[3] = 16.0
    C_, T, n, S, m = gr.build_table(w)
    assert m.tolist() == [3, 0, 5, 1 << 24, 1] and T == 9 + (1 << 24) and n == 4
    assert C_.tolist() == [3, 3, 8, 8 + (1 << 24), 9 + (1 << 24)]
    # every t in [0, T): exactly m_p of them go to cell p (searchsorted on the table itself; t_of maps v onto these t)
    cells = np.searchsorted(C_, np.arange(T, dtype=np.uint64), side="right")
    assert np.bincount(cells, minlength=5).tolist() == m.tolist()
    # and through the 64-bit values: the smallest and largest v of every t-bucket's neighbourhood stay inside [0, T)
    v = np.array([0, 1, (1 << 64) - 1, (1 << 63), ((1 << 64) // T) * 3, ((1 << 64) // T) * 3 + (1 << 40)], dtype=np.uint64)
    got = gr.cell_of(C_, T, v)
    assert got.min() >= 0 and got.max() <= 4 and 1 not in got.tolist()
    assert got[0] == 0 and got[2] == 4


def test_cells_without_mass_are_never_returned():
    rng = np.random.default_rng(11)
    w = (10.0 ** rng.uniform(-9, 0, 500)).astype(np.float32)
    w[rng.integers(0, 500, 60)] = np.array([np.nan, -1.0, np.inf, 0.0] * 15, np.float32)
    w[0] = 0.0       # a table that begins ...
    w[-1] = np.nan   # ... and ends without mass
    C_, T, n, S, m = gr.build_table(w)
    assert 4 <= n < np.count_nonzero(gr.valid_cells(w)), "the heavy tail must send valid cells to mass 0"
    v = rng.integers(0, 1 << 64, 20000, dtype=np.uint64)
    v[:3] = (0, (1 << 64) - 1, 1 << 63)
    cells = gr.cell_of(C_, T, v)
    assert cells.min() >= 0 and cells.max() < 500 and (m[cells] > 0).all()
    sets, drawn, redraws = gr.attempt_sets(C_, T, n, seed=7, N=8, A=8)
    assert (m[sets[drawn == 1]] > 0).all()
    for s in sets[drawn == 1]:
        assert len(set(s.tolist())) == 4


def test_fewer_than_four_cells_of_mass_yield_no_set():
    for w in (np.zeros(50, np.float32), np.full(50, np.nan, np.float32), -np.ones(50, np.float32)):
        C_, T, n, S, m = gr.build_table(w)
        assert T == 0 and n == 0
        sets, drawn, _ = gr.attempt_sets(C_, T, n, seed=3, N=4, A=4)
        assert not drawn.any() and not sets.any()
    w = np.zeros(50, np.float32)
    w[[3, 17, 40]] = (1.0, 2.0, 0.5)
    C_, T, n, S, m = gr.build_table(w)
    assert n == 3 and T == (1 << 24) + (1 << 23) + (1 << 22) and S == 3.5
    sets, drawn, _ = gr.attempt_sets(C_, T, n, seed=3, N=4, A=4)
    assert not drawn.any() and not sets.any()
    # the rule itself, with the n < 4 shortcut taken away: three cells of mass exhaust the 32 candidates of every attempt
    sets, drawn, _ = gr.attempt_sets(C_, T, 4, seed=3, N=4, A=4)
    assert not drawn.any() and not sets.any()


def test_equal_weights_are_the_uniform_distribution_over_cells():
    C_, T, n, S, m = gr.build_table(np.ones(1600, np.float32))
    assert T == 1600 << 24 and n == 1600 and S == 1600.0
    sets, drawn, redraws = gr.attempt_sets(C_, T, n, seed=1305, N=64, A=64)
    assert drawn.all() and sets.min() >= 0 and sets.max() < 1600
    assert 0 < np.count_nonzero(redraws) < 64  # ~6 / P of the 4 096 attempts meet a duplicate: 15 expected
