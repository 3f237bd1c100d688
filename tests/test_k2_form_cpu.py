"""CPU-side checks of the K2 form query and the range census (dsac_get_option, dsac_k2_range_census): the symbols are exported, bound and documented, and
a NULL context is rejected without touching a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_entry_points_are_exported_and_reject_a_null_context():
    from dsac_amd import capi
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (dsac_[a-z0-9_]+)", out))
    assert {"dsac_get_option", "dsac_k2_range_census"} <= exported
    assert {"dsac_get_option", "dsac_k2_range_census"} <= set(capi.EXPORTS)
    v = C.c_int(123)
    assert capi.lib.dsac_get_option(None, b"k2_flags", C.byref(v)) == capi.DSAC_ERR_INVALID
    assert v.value == 123
    assert b"NULL" in capi.lib.dsac_last_error(None)
    far, oor = C.c_longlong(-7), C.c_longlong(-7)
    assert capi.lib.dsac_k2_range_census(None, 1, None, C.byref(far), C.byref(oor)) == capi.DSAC_ERR_INVALID
    assert (far.value, oor.value) == (-7, -7)
    assert b"NULL" in capi.lib.dsac_last_error(None)


def test_the_binding_names_every_form_and_reason_of_the_header():
    """enum dsac_k2_form and the DSAC_K2_WHY_* bits of include/dsac_hip.h against dsac_amd.capi: same count, same values."""
    from dsac_amd import capi
    txt = open(os.path.join(ROOT, "include", "dsac_hip.h")).read()
    forms = dict((n, int(v)) for n, v in re.findall(r"\b(DSAC_K2_FORM_[A-Z0-9_]+)\s*=\s*(\d+)", txt))
    assert sorted(forms.values()) == list(range(len(capi.K2_FORMS)))
    assert capi.K2_FORMS[forms["DSAC_K2_FORM_NONE"]] == "none"
    assert capi.K2_FORMS[forms["DSAC_K2_FORM_EXACT_VEC"]] == "exact (vector build)"
    assert capi.K2_FORMS[forms["DSAC_K2_FORM_EXACT_ANY"]] == "exact (any-map build)"
    assert capi.K2_FORMS[forms["DSAC_K2_FORM_PRECISE"]] == "precise"
    why = dict((n, int(v)) for n, v in re.findall(r"#define\s+(DSAC_K2_WHY_[A-Z0-9_]+)\s+(\d+)", txt))
    assert why and all(getattr(capi, n) == v for n, v in why.items())
    assert sorted(why.values()) == [1 << i for i in range(len(why))]
