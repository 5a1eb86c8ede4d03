"""The C ABI's promise (include/dcora_hip.h): every function returns a status and nothing throws across the boundary; a
NULL handle or a NULL required pointer is DCORA_ERR_BAD_ARG.  Every function of capi.SIGNATURES is called with every
pointer NULL and every number 0 -- in a child interpreter, so that a crash fails the test instead of ending the run.
Host only: skipped where a device is present, so that no NULL ever reaches a live device.  The guard and the library's
thread helper (dcora_amd/csrc/host_threads.h) are also unit-tested under ASan + UBSan."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import common

ROOT = os.path.dirname(common.HERE)

CHILD = r"""
import ctypes as C, json, sys
import numpy as np
from dcora_amd import capi

L = C.CDLL(capi.LIB_PATH)
L.dcora_device_count.restype = C.c_int
if L.dcora_device_count() > 0:
    print(json.dumps({"device": True}))
    sys.exit(0)
L.dcora_last_error.restype = C.c_char_p


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, np.ctypeslib._ndptr))


out = {}
for name, (res, args) in capi.SIGNATURES.items():
    fn = getattr(L, name)
    fn.restype = res
    fn.argtypes = [C.c_void_p if is_pointer(t) else t for t in args]
    status = fn(*[None if is_pointer(t) else 0 for t in args])
    msg = L.dcora_last_error().decode()
    out[name] = {"status": status if isinstance(status, int) else None, "pointers": any(map(is_pointer, args)),
                 "error": msg}

# dcora_cert_prepare reads the caller's pattern only after checking it (d = 2, n = 2: k = 6), before any device use
fn = L.dcora_cert_prepare
fn.restype = C.c_int
dims = capi.Dims(1, 2, 2, 0, 0, 0)
pat = {"rp0": ([1] * 7, [0]), "decreasing": ([0, 2, 1, 1, 1, 1, 1], [0, 1]), "ci_ge_k": ([0, 1, 1, 1, 1, 1, 1], [6]),
       "ci_negative": ([0, 1, 1, 1, 1, 1, 1], [-1])}
prep = {}
for key, (rp, ci) in pat.items():
    rp, ci = np.array(rp, np.int32), np.array(ci, np.int32)
    st = fn(C.byref(dims), rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), 1, 0)
    prep[key] = [st, L.dcora_last_error().decode()]
print(json.dumps({"device": False, "calls": out, "prepare": prep}))
"""


@pytest.fixture(scope="module")
def null_calls(built):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, "the child crashed (status %d): %s" % (r.returncode, r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    if res["device"]:
        pytest.skip("a device is present: NULL arguments are only handed to the library without one")
    return res


def test_every_entry_point_returns_and_refuses_null(null_calls):
    from dcora_amd import capi
    calls = null_calls["calls"]
    assert set(calls) == set(capi.SIGNATURES)
    for name, c in calls.items():
        if name.endswith("_destroy"):
            assert c["status"] == 0, (name, c)
        elif c["pointers"] and capi.SIGNATURES[name][0] is ctypes.c_int:
            assert c["status"] == 1 and c["error"] == "null argument", (name, c)


def test_cert_prepare_refuses_malformed_patterns_before_device_use(null_calls):
    prep = null_calls["prepare"]
    assert prep["rp0"] == [1, "cert_prepare: rowptr[0] must be 0"]
    assert prep["decreasing"] == [1, "cert_prepare: rowptr decreases"]
    assert prep["ci_ge_k"] == [1, "cert_prepare: column index out of range"]
    assert prep["ci_negative"] == [1, "cert_prepare: column index out of range"]


def test_python_cert_prepare_checks_the_order_of_Q(built):
    import numpy as np
    import scipy.sparse as sp
    import dcora_amd as da
    Q = da.Csr.from_scipy(sp.identity(7, format="csr"))
    with pytest.raises(ValueError):
        da.cert_prepare(Q, 2, 2)  # (d + 1) n = 6


def test_host_threads_and_guard_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_host_threads")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "dcora_amd", "csrc"),
           os.path.join(common.HERE, "cpp", "test_host_threads.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.strip() == "ok", r.stdout
