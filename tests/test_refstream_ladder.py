"""The window ladder of the enqueue-only reference-stream chain (dsac_sample_refstream_frames; rs::window_ladder in dsac_amd/csrc/refstream.h) and its
accounting rule, compiled with g++: the chain is enqueued without reading anything back, so the host fixes the window sizes beforehand -- they must sum
to the attempt budget exactly, grow monotonically to the cap, and the documented window limit must be the one the API refuses beyond.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def rsl(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rsl") / "librsl.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "helpers", "refstream_ladder_host.cpp")])
    lib = C.CDLL(out)
    lib.rsl_default_budget.restype = C.c_longlong
    lib.rsl_check_range.restype = C.c_longlong
    lib.rsl_check_range.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
    lib.rsl_ladder.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_int]
    lib.rsl_charge.restype = C.c_longlong
    lib.rsl_charge.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def ladder(rsl, want, budget, cap=4096):
    s = np.zeros(cap, np.int32)
    n = rsl.rsl_ladder(want, budget, s.ctypes.data, cap)
    return n, s[:min(n, cap)]


def test_sizes_sum_to_the_budget_and_grow_to_the_cap(rsl):
    # every budget from 1 to 2^20 for a spread of wanted counts (the first window's rungs: 256 ... 16384) ...
    for want in (1, 2, 9, 16, 17, 61, 64, 100, 256, 257, 1000, 1024, 1025, 4096):
        assert rsl.rsl_check_range(want, 1, 1 << 20) == 0, "wanted %d" % want
    # ... and every wanted count from 1 to 4096 for a spread of budgets
    for budget in (1, 255, 256, 257, 4095, 4096, 4097, 16384, 65535, 65536, 99991, (1 << 20) - 1, 1 << 20):
        for want in range(1, 4097):
            assert rsl.rsl_check_range(want, budget, budget) == 0, (want, budget)
    n, s = ladder(rsl, 256, 65536)
    assert list(s) == [4096, 8192, 16384, 16384, 16384, 4096] and n == 6
    n, s = ladder(rsl, 16, 1000)
    assert list(s) == [256, 512, 232]
    n, s = ladder(rsl, 61, 100)
    assert list(s) == [100]


def test_first_window_and_default_budget(rsl):
    lo, hi, per = rsl.rsl_window_min(), rsl.rsl_window_max(), rsl.rsl_window_per_hyp()
    assert (lo, hi, per) == (256, 16384, 16)
    for want in range(1, 4097):
        a = rsl.rsl_window_first(want)
        assert lo <= a <= hi and a & (a - 1) == 0
        assert a >= min(hi, per * want) and (a == lo or a // 2 < per * want)
        assert rsl.rsl_default_budget(want) == max(4096, 256 * want)
        # the default budget stays inside the window limit up to 4096 hypotheses per stream (beyond, the caller names a budget)
        assert ladder(rsl, want, rsl.rsl_default_budget(want))[0] <= rsl.rsl_max_windows()


def test_window_limit_is_the_documented_one(rsl):
    """include/dsac_hip.h states the limit the API refuses beyond; the API uses rs::MAX_WINDOWS (tests/test_gpu_refstream_frames.py::test_misuse hits it)."""
    limit = rsl.rsl_max_windows()
    hdr = open(os.path.join(ROOT, "include", "dsac_hip.h")).read()
    m = re.search(r"needs more than (\d+) windows", hdr)
    assert m and int(m.group(1)) == limit == 64
    # the largest budget inside the limit for one hypothesis per stream: the ramp 256 ... 8192 and 58 windows of 16384
    inside = sum(256 << k for k in range(6)) + 58 * 16384
    assert ladder(rsl, 1, inside)[0] == limit and ladder(rsl, 1, inside + 1)[0] == limit + 1
    assert ladder(rsl, 4096, 64 * 16384)[0] == limit and ladder(rsl, 4096, 64 * 16384 + 1)[0] == limit + 1


def test_untemper_inverts_temper_and_recovers_a_block_state(rsl):
    """The step kernel puts a generator behind the last attempt used by untempering the 624 outputs of the block that holds that position instead of
    twisting up to it: mt_untemper must invert mt_temper on every word, and a block's outputs must give back the block's state."""
    rsl.rsl_untemper_mismatches.restype = C.c_longlong
    rsl.rsl_untemper_mismatches.argtypes = [C.c_uint32, C.c_uint32, C.c_longlong]
    assert rsl.rsl_untemper_mismatches(0, 1, 1 << 22) == 0
    assert rsl.rsl_untemper_mismatches(0xfff00000, 1, 1 << 20) == 0
    assert rsl.rsl_untemper_mismatches(12345, 2654435761, 1 << 22) == 0  # a stride that walks the whole word range
    rsl.rsl_state_from_outputs.argtypes = [C.c_uint32, C.c_uint64]
    for seed, skip in ((1305, 1), (1305, 624), (1305, 625), (4242, 6400), (0, 27808), (0xFFFFFFFF, 100000)):
        assert rsl.rsl_state_from_outputs(seed, skip) == 0, (seed, skip)


def test_attempts_charged_are_attempts_used(rsl):
    """A hand-made accept pattern: the stream's 5 hypotheses are served by its attempts 3, 300, 301, 700 and 5000.  Whatever ladder the budget gives,
    the stream is charged 5001 attempts (index of the last one used + 1), not the sum of the windows it touched; with a budget that ends before the
    fifth acceptance it is charged the whole budget and serves four."""
    accept = np.zeros(20000, np.uint8)
    accept[[3, 300, 301, 700, 5000, 5001, 5002, 9000]] = 1
    for want, budget in ((5, 20000), (5, 5001), (5, 6000), (40, 20000), (1, 20000)):
        n, s = ladder(rsl, want, budget)
        served = C.c_int(0)
        charged = rsl.rsl_charge(5, accept.ctypes.data, len(accept), s.ctypes.data, n, C.byref(served))
        assert served.value == 5 and charged == 5001, (want, budget, list(s))
        assert int(s.sum()) == budget
    for budget in (5000, 4000, 701):
        n, s = ladder(rsl, 5, budget)
        served = C.c_int(0)
        charged = rsl.rsl_charge(5, accept.ctypes.data, len(accept), s.ctypes.data, n, C.byref(served))
        assert served.value == 4 and charged == budget
    # one window that holds everything charges the same as many small ones
    one = np.array([20000], np.int32)
    served = C.c_int(0)
    assert rsl.rsl_charge(5, accept.ctypes.data, len(accept), one.ctypes.data, 1, C.byref(served)) == 5001
