"""The lift's entry points without a device (include/dcora_hip.h: dcora_lift_params_default, dcora_rbcd_lift,
dcora_ra_rbcd_lift, dcora_rbcd_rank, dcora_ra_rbcd_rank): the defaults, the refusal of NULL handles before any device
use, and what tests/test_abi_guard_cpu.py asks of every entry point -- declared in the header, bound in
capi.SIGNATURES, exported by the library."""
import ctypes as C
import re

import numpy as np
import pytest

ENTRIES = ("dcora_lift_params_default", "dcora_rbcd_lift", "dcora_ra_rbcd_lift", "dcora_rbcd_rank",
           "dcora_ra_rbcd_rank")


@pytest.fixture(scope="module")
def capi(built):
    from dcora_amd import capi
    return capi


def test_defaults(capi):
    p = capi.LiftParams(7.0, 7.0, 7, 7.0)
    assert capi.lib().dcora_lift_params_default(C.byref(p)) == 0
    assert (p.gradient_tolerance, p.preconditioned_gradient_tolerance, p.is_second_order, p.central_reg) == \
        (1e-6, 1e-6, 0, -1.0)
    assert capi.lib().dcora_lift_params_default(None) == 1
    assert capi.lib().dcora_last_error().decode() == "null argument"


def test_null_handles_are_refused_without_a_device(capi):
    L = capi.lib()
    p = capi.LiftParams()
    L.dcora_lift_params_default(C.byref(p))
    v, esc, r = np.zeros(4), C.c_int(5), C.c_int(5)
    for fn in (L.dcora_rbcd_lift, L.dcora_ra_rbcd_lift):
        assert fn(None, -1.0, v, C.byref(p), C.byref(esc), None) == 1
        assert L.dcora_last_error().decode() == "null argument"
    for fn in (L.dcora_rbcd_rank, L.dcora_ra_rbcd_rank):
        assert fn(None, C.byref(r)) == 1
        assert L.dcora_last_error().decode() == "null argument"
    assert esc.value == 5 and r.value == 5  # nothing was written


def test_entries_are_declared_bound_and_exported(capi):
    with open(capi.HEADER_PATH) as f:
        header = f.read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SIGNATURES and capi.SIGNATURES[name][0] is C.c_int
        assert getattr(L, name)
    # the struct the binding passes is the header's: two doubles, an int, a double
    m = re.search(r"typedef struct \{([^}]*)\} dcora_lift_params;", header)
    assert m
    fields = re.findall(r"(\w+)\s*[,;]", re.sub(r"\b(double|int)\b", "", m.group(1)))
    assert fields == [n for n, _ in capi.LiftParams._fields_]
