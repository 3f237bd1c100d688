"""Half-precision error images, the parts that need no device: the two exports are declared, and Engine.reproject / processImagesBegin pick the entry point by
the dtype of `err` (float16 -> the _f16 call, float32 -> the float call, as before)."""
import ctypes as C

import numpy as np
import pytest


def test_exports_are_declared():
    from dsac_amd import capi
    assert "dsac_reproject_f16" in capi.EXPORTS and "dsac_process_images_begin_f16" in capi.EXPORTS
    assert capi.lib.dsac_reproject_f16.argtypes == capi.lib.dsac_reproject.argtypes
    assert capi.lib.dsac_process_images_begin_f16.argtypes == capi.lib.dsac_process_images_begin.argtypes


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


@pytest.mark.parametrize("dtype,want", [(np.float32, "dsac_reproject"), (np.float16, "dsac_reproject_f16")])
def test_reproject_dispatches_on_the_dtype_of_err(recorded, dtype, want):
    e, rec = recorded
    err = np.zeros((2, 32), dtype)
    e.reproject(np.zeros((2, 6)), err=err, soft=np.zeros(2))
    assert [c[0] for c in rec.calls] == [want]
    assert rec.calls[0][1][4] == err.ctypes.data  # the array itself is handed over, no converted copy


def test_reproject_without_error_images_is_the_float_call(recorded):
    e, rec = recorded
    e.reproject(np.zeros((2, 6)), soft=np.zeros(2))
    assert [c[0] for c in rec.calls] == ["dsac_reproject"]


@pytest.mark.parametrize("dtype,want", [(np.float32, "dsac_process_images_begin"), (np.float16, "dsac_process_images_begin_f16")])
def test_process_images_begin_dispatches_on_the_dtype_of_err(recorded, dtype, want):
    e, rec = recorded
    err = np.zeros((3, 32), dtype)
    e.processImagesBegin(3, err, seed=7)
    assert [c[0] for c in rec.calls] == [want]
    assert rec.calls[0][1][11] == err.ctypes.data


def test_torch_half_tensor_dispatches_too(recorded):
    import torch
    e, rec = recorded
    e.reproject(np.zeros((2, 6)), err=torch.zeros(2, 32, dtype=torch.float16))
    e.reproject(np.zeros((2, 6)), err=torch.zeros(2, 32, dtype=torch.float32))
    assert [c[0] for c in rec.calls] == ["dsac_reproject_f16", "dsac_reproject"]
