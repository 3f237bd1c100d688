"""bfloat16 at the score-model seam, the parts that need no device: the four exports are declared with their _f16 twins' argtypes, and Engine.reproject /
processImagesBegin / dScore / softScoreDErr pick the _bf16 entry point for a torch.bfloat16 tensor by its dtype, for a numpy uint16 array (numpy has no
bfloat16) only with elem="bf16"; float32 and float16 arrays go where they went before."""
import ctypes as C

import numpy as np
import pytest

PAIRS = [("dsac_reproject_bf16", "dsac_reproject_f16"), ("dsac_process_images_begin_bf16", "dsac_process_images_begin_f16"),
         ("dsac_score_backward_bf16", "dsac_score_backward_f16"), ("dsac_soft_score_derr_bf16", "dsac_soft_score_derr_f16")]


@pytest.mark.parametrize("bf,half", PAIRS)
def test_exports_are_declared(bf, half):
    from dsac_amd import capi
    assert bf in capi.EXPORTS
    assert getattr(capi.lib, bf).argtypes == getattr(capi.lib, half).argtypes


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


def _bf(*shape):
    import torch
    return torch.zeros(*shape, dtype=torch.bfloat16)


def _names(rec):
    return [c[0] for c in rec.calls]


# ---- a torch.bfloat16 tensor decides by its dtype; its own address is handed over ---------------------------------------------------------------
def test_reproject_takes_a_bfloat16_tensor(recorded):
    e, rec = recorded
    err = _bf(2, 32)
    e.reproject(POSES, err=err, soft=np.zeros(2))
    assert _names(rec) == ["dsac_reproject_bf16"]
    assert rec.calls[0][1][4] == err.data_ptr()


def test_process_images_begin_takes_a_bfloat16_tensor(recorded):
    e, rec = recorded
    err = _bf(3, 32)
    e.processImagesBegin(3, err, seed=7)
    assert _names(rec) == ["dsac_process_images_begin_bf16"]
    assert rec.calls[0][1][11] == err.data_ptr()


def test_dscore_takes_a_bfloat16_tensor(recorded):
    e, rec = recorded
    d = _bf(2, 32)
    grad = e.dScore(POSES, SETS, d, quirk_transpose=True)
    assert _names(rec) == ["dsac_score_backward_bf16"]
    args = rec.calls[0][1]
    assert args[1] == 2 and args[4] == d.data_ptr() and args[6] == 1 and args[7] == grad.ctypes.data


def test_soft_score_derr_takes_bfloat16_tensors(recorded):
    e, rec = recorded
    err, d = _bf(2, 32), _bf(2, 32)
    assert e.softScoreDErr(np.zeros(2), err, d, tau=9.0, beta=0.25) is d
    assert _names(rec) == ["dsac_soft_score_derr_bf16"]
    args = rec.calls[0][1]
    assert args[3] == err.data_ptr() and args[7] == d.data_ptr() and args[4:7] == (100.0, 9.0, 0.25)


# ---- numpy has no bfloat16: uint16 arrays and raw addresses only with the keyword ----------------------------------------------------------------
def test_uint16_arrays_need_the_keyword(recorded):
    e, rec = recorded
    u = np.zeros((2, 32), np.uint16)
    u3 = np.zeros((3, 32), np.uint16)
    for call in (lambda **kw: e.reproject(POSES, err=u, **kw), lambda **kw: e.processImagesBegin(3, u3, **kw), lambda **kw: e.dScore(POSES, SETS, u, **kw),
                 lambda **kw: e.softScoreDErr(np.zeros(2), u, u.copy(), **kw)):
        with pytest.raises(ValueError):
            call()
    assert rec.calls == []  # refused, never guessed: nothing reached the library
    e.reproject(POSES, err=u, elem="bf16")
    e.processImagesBegin(3, u3, elem="bf16")
    e.dScore(POSES, SETS, u, elem="bf16")
    d = u.copy()
    e.softScoreDErr(np.zeros(2), u, d, elem="bf16")
    assert _names(rec) == ["dsac_reproject_bf16", "dsac_process_images_begin_bf16", "dsac_score_backward_bf16", "dsac_soft_score_derr_bf16"]
    assert rec.calls[0][1][4] == u.ctypes.data and rec.calls[1][1][11] == u3.ctypes.data and rec.calls[2][1][4] == u.ctypes.data  # no converted copy
    assert rec.calls[3][1][3] == u.ctypes.data and rec.calls[3][1][7] == d.ctypes.data


def test_a_raw_address_takes_the_keyword(recorded):
    e, rec = recorded
    e.reproject(POSES, err=4096, elem="bf16")
    e.reproject(POSES, err=4096)  # without it an address is floats, as before
    assert _names(rec) == ["dsac_reproject_bf16", "dsac_reproject"]
    assert rec.calls[0][1][4] == 4096


def test_the_keyword_does_not_override_a_dtype(recorded):
    e, rec = recorded
    for arr in (np.zeros((2, 32), np.float32), np.zeros((2, 32), np.float16)):
        with pytest.raises(ValueError):
            e.reproject(POSES, err=arr, elem="bf16")
        with pytest.raises(ValueError):
            e.dScore(POSES, SETS, arr, elem="bf16")
    with pytest.raises(ValueError):
        e.reproject(POSES, err=_bf(2, 32), elem="f16")  # the keyword may repeat a dtype, never contradict it
    assert rec.calls == []


def test_the_keyword_may_repeat_a_dtype_or_name_halves_in_a_uint16_array(recorded):
    e, rec = recorded
    e.reproject(POSES, err=np.zeros((2, 32), np.float32), elem="f32")
    e.reproject(POSES, err=np.zeros((2, 32), np.float16), elem="f16")
    e.reproject(POSES, err=_bf(2, 32), elem="bf16")
    e.reproject(POSES, err=np.zeros((2, 32), np.uint16), elem="f16")
    assert _names(rec) == ["dsac_reproject", "dsac_reproject_f16", "dsac_reproject_bf16", "dsac_reproject_f16"]
    with pytest.raises(ValueError):
        e.reproject(POSES, err=np.zeros((2, 32), np.uint16), elem="f32")
    with pytest.raises(ValueError):
        e.reproject(POSES, err=np.zeros((2, 32), np.float32), elem="half")


# ---- float32 and float16 go where they went -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,suffix", [(np.float32, ""), (np.float16, "_f16")])
def test_float_and_half_arrays_reach_their_calls(recorded, dtype, suffix):
    e, rec = recorded
    err, err3, d = np.zeros((2, 32), dtype), np.zeros((3, 32), dtype), np.zeros((2, 32), dtype)
    e.reproject(POSES, err=err)
    e.processImagesBegin(3, err3)
    e.dScore(POSES, SETS, d)
    e.softScoreDErr(np.zeros(2), err, d)
    assert _names(rec) == ["dsac_reproject" + suffix, "dsac_process_images_begin" + suffix, "dsac_score_backward" + suffix, "dsac_soft_score_derr" + suffix]
    assert rec.calls[0][1][4] == err.ctypes.data and rec.calls[2][1][4] == d.ctypes.data


# ---- what dScore and softScoreDErr refuse -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(parity_fp64=True), dict(quirk_rot_writeback=True)])
def test_the_parity_mode_does_not_take_bfloat16(recorded, kw):
    e, rec = recorded
    with pytest.raises(ValueError):
        e.dScore(POSES, SETS, _bf(2, 32), **kw)
    with pytest.raises(ValueError):
        e.dScore(POSES, SETS, np.zeros((2, 32), np.uint16), elem="bf16", **kw)
    assert rec.calls == []


def test_soft_score_derr_refuses_mixed_element_types(recorded):
    import torch
    e, rec = recorded
    g = np.zeros(2)
    for err, d in ((_bf(2, 32), torch.zeros(2, 32, dtype=torch.float16)), (_bf(2, 32), torch.zeros(2, 32)), (torch.zeros(2, 32), _bf(2, 32)),
                   (np.zeros((2, 32), np.float16), _bf(2, 32))):
        with pytest.raises(ValueError):
            e.softScoreDErr(g, err, d)
    with pytest.raises(ValueError):
        e.softScoreDErr(g, np.zeros((2, 32), np.uint16), np.zeros((2, 32), np.float32), elem="bf16")
    assert rec.calls == []
