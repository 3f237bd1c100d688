"""dsac_set_frames_cams without a device: the binding declares the call with the header's signature, a NULL context is rejected without a crash, and the
(F, 4) / (4,) shape logic of Engine.set_frames (engine.frame_cams_arg) accepts what the call takes and raises on everything else before the library is
reached."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_decl(name):
    txt = open(os.path.join(ROOT, "include", "dsac_hip.h")).read()
    m = re.search(r"DSAC_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, re.S)
    assert m, "%s is not declared in include/dsac_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_binding_declares_the_headers_signature():
    from dsac_amd import capi
    args = _header_decl("dsac_set_frames_cams")
    assert args == ["dsac_ctx* ctx", "int frames", "const float* xyz", "const float* uv_or_null", "int uv_per_frame", "int H", "int W", "const float* cams",
                    "unsigned flags"]
    ctype_of = lambda a: C.c_void_p if "*" in a else C.c_uint if a.startswith("unsigned") else C.c_int
    assert capi.lib.dsac_set_frames_cams.argtypes == [ctype_of(a) for a in args]
    assert "dsac_set_frames_cams" in capi.EXPORTS
    # the neighbour it mirrors: the same arguments but for the camera (four floats there, one host pointer here)
    ref = _header_decl("dsac_set_frames")
    assert ref[:7] == args[:7] and ref[-1] == args[-1] and ref[7:-1] == ["float fx", "float fy", "float cx", "float cy"]


def test_null_context_is_rejected_without_crashing():
    from dsac_amd import capi
    cams = np.array([[525.0, 525.0, 320.0, 240.0]], np.float32)
    xyz = np.zeros((4, 3), np.float32)
    assert capi.lib.dsac_set_frames_cams(None, 1, xyz.ctypes.data, None, 0, 2, 2, cams.ctypes.data, 0) == capi.DSAC_ERR_INVALID
    assert b"NULL" in capi.lib.dsac_last_error(None)
    assert capi.lib.dsac_set_frames_cams(None, 1, None, None, 0, 2, 2, None, 0) == capi.DSAC_ERR_INVALID


def test_camera_argument_shapes():
    from dsac_amd.engine import frame_cams_arg
    F = 3
    shared, table = frame_cams_arg((525.0, 525.0, 320.0, 240.0), F)
    assert table is None and shared == (525.0, 525.0, 320.0, 240.0) and all(type(c) is float for c in shared)
    shared, table = frame_cams_arg(np.array([585, 585, 320, 240]), F)  # any dtype np.asarray takes
    assert table is None and shared == (585.0, 585.0, 320.0, 240.0)
    rows = [[525.0, 525.0, 320.0, 240.0], [585.0, 585.0, 320.0, 240.0], [260.0, 260.0, 300.0, 250.0]]
    for given in (rows, np.array(rows, np.float64), np.asfortranarray(np.array(rows, np.float32)), tuple(tuple(r) for r in rows)):
        shared, table = frame_cams_arg(given, F)
        assert shared is None and table.dtype == np.float32 and table.shape == (F, 4) and table.flags["C_CONTIGUOUS"]
        assert np.array_equal(table, np.array(rows, np.float32))
    # four frames: a (4,) camera is the shared one, a (4, 4) table one camera per frame
    assert frame_cams_arg(rows[0], 4)[1] is None
    assert frame_cams_arg(rows + [rows[0]], 4)[0] is None
    for wrong in (np.zeros((F, 3)), np.zeros((F + 1, 4)), np.zeros((F, 4, 1)), np.zeros((1, F, 4)), np.zeros(3), 525.0):
        with pytest.raises(ValueError, match="cam must have shape"):
            frame_cams_arg(wrong, F)
