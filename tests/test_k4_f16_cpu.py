"""K4 on half-precision gradient images, the parts that need no device: the two exports are declared with their float twins' argtypes, and Engine.dScore /
Engine.softScoreDErr pick the entry point by the dtype of the images (float16 -> the _f16 call on the array itself, anything else -> the float call)."""
import ctypes as C

import numpy as np
import pytest


def test_exports_are_declared():
    from dsac_amd import capi
    assert "dsac_score_backward_f16" in capi.EXPORTS and "dsac_soft_score_derr_f16" in capi.EXPORTS
    assert capi.lib.dsac_score_backward_f16.argtypes == capi.lib.dsac_score_backward.argtypes
    assert capi.lib.dsac_soft_score_derr_f16.argtypes == capi.lib.dsac_soft_score_derr.argtypes


class _Recorder:
    """Stands in for the loaded library: every C function is a stub that records its name and arguments and returns DSAC_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture()
def recorded(monkeypatch):
    from dsac_amd import capi, engine
    rec = _Recorder()
    monkeypatch.setattr(capi, "lib", rec)
    monkeypatch.setattr(engine, "lib", rec)  # the engine module binds the library by name at import
    e = engine.Engine.__new__(engine.Engine)  # no dsac_create: no device
    e._ctx, e.device, e.H, e.W, e.P, e.frames = C.c_void_p(), 0, 4, 8, 32, 1
    return e, rec


POSES, SETS = np.zeros((2, 6)), np.zeros((2, 4), np.int32)


@pytest.mark.parametrize("dtype,want", [(np.float32, "dsac_score_backward"), (np.float16, "dsac_score_backward_f16")])
def test_dscore_dispatches_on_the_dtype_of_d_err(recorded, dtype, want):
    e, rec = recorded
    d_err = np.zeros((2, 32), dtype)
    grad = e.dScore(POSES, SETS, d_err, quirk_transpose=True)
    assert [c[0] for c in rec.calls] == [want]
    args = rec.calls[0][1]
    assert args[1] == 2 and args[4] == d_err.ctypes.data  # the array itself is handed over, no converted copy
    assert args[6] == 1 and args[7] == grad.ctypes.data and grad.shape == (32, 3)


def test_dscore_on_torch_tensors_dispatches_too(recorded):
    import torch
    e, rec = recorded
    d16, d32 = torch.zeros(2, 32, dtype=torch.float16), torch.zeros(2, 32, dtype=torch.float32)
    e.dScore(POSES, SETS, d16)
    e.dScore(POSES, SETS, d32)
    assert [c[0] for c in rec.calls] == ["dsac_score_backward_f16", "dsac_score_backward"]
    assert rec.calls[0][1][4] == d16.data_ptr() and rec.calls[1][1][4] == d32.data_ptr()


def test_dscore_converts_other_numpy_dtypes_for_the_float_call(recorded):
    e, rec = recorded
    e.dScore(POSES, SETS, np.zeros((2, 32), np.float64))
    assert [c[0] for c in rec.calls] == ["dsac_score_backward"]


@pytest.mark.parametrize("kw", [dict(parity_fp64=True), dict(quirk_rot_writeback=True)])
def test_the_parity_mode_does_not_take_halves(recorded, kw):
    e, rec = recorded
    with pytest.raises(ValueError):
        e.dScore(POSES, SETS, np.zeros((2, 32), np.float16), **kw)
    assert rec.calls == []
    e.dScore(POSES, SETS, np.zeros((2, 32), np.float32), **kw)  # the float call takes them as before
    assert [c[0] for c in rec.calls] == ["dsac_score_backward"] and rec.calls[0][1][6] & 2


@pytest.mark.parametrize("dtype,want", [(np.float32, "dsac_soft_score_derr"), (np.float16, "dsac_soft_score_derr_f16")])
def test_soft_score_derr_dispatches_on_the_dtype(recorded, dtype, want):
    e, rec = recorded
    err, d_err = np.zeros((2, 32), dtype), np.zeros((2, 32), dtype)
    assert e.softScoreDErr(np.zeros(2), err, d_err, tau=9.0, beta=0.25) is d_err
    assert [c[0] for c in rec.calls] == [want]
    args = rec.calls[0][1]
    assert args[1] == 2 and args[3] == err.ctypes.data and args[7] == d_err.ctypes.data and args[4:7] == (100.0, 9.0, 0.25)
    with pytest.raises(ValueError):
        e.softScoreDErr(np.zeros(2), np.zeros((2, 32), np.float16), np.zeros((2, 32), np.float32))
