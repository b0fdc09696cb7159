"""CPU: the MESS rule (include/machisplin_hip.h, "MESS extrapolation map").  The numpy restatement the GPU tests compare
with is itself checked against a hand-computed table; mhs_mess_create refuses bad reference tables before it touches a
device; and the rule header the kernel is built from (csrc/mess_rule.h) gives the same table in a plain C++ program
compiled with gcc under AddressSanitizer + UBSan and run stand-alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mess_ref
from machisplin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ref = [1, 2, 3, 4]: p, s, i = #{r <= p}
HAND = [(2.5, 100.0, 2), (1.0, 50.0, 1), (3.0, 50.0, 3), (4.0, 0.0, 4), (0.0, -100.0 / 3.0, 0), (5.0, -100.0 / 3.0, 4)]


def test_restatement_gives_the_hand_computed_table():
    ref = np.array([3.0, 1.0, 4.0, 2.0])          # unsorted on purpose
    p = np.array([h[0] for h in HAND])
    s = mess_ref.similarity(ref, p)
    assert np.array_equal(s, np.array([h[1] for h in HAND]))
    assert np.isnan(mess_ref.similarity(ref, np.array([np.nan])))[0]


def test_restatement_min_mod_ties_and_na():
    ref = np.array([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [4.0, 40.0]])
    v0 = np.array([2.5, 1.0, 0.0, 2.5, np.nan, 1.0])
    v1 = np.array([25.0, 25.0, 25.0, 50.0, 25.0, 30.0])
    m, mod = mess_ref.mess(ref, [v0, v1])
    #            100|100   50|100   -33|100   100|-33   NA   50|50 (an exact tie: the lowest variable)
    assert np.array_equal(m, np.array([100.0, 50.0, -100.0 / 3.0, -100.0 / 3.0, np.nan, 50.0]), equal_nan=True)
    assert np.array_equal(mod, np.array([0, 0, 0, 1, -1, 0], dtype=np.int32))
    assert mod.dtype == np.int32


def _create(ref):
    ref = np.asfortranarray(np.asarray(ref, dtype=np.float64))
    h = C.c_void_p()
    lib = _lib.load()
    rc = lib.mhs_mess_create(ref.ctypes.data, ref.shape[0], ref.shape[1], C.byref(h))
    msg = lib.mhs_last_error().decode()
    if rc == _lib.OK:
        lib.mhs_mess_free(h)
    return rc, msg


def test_create_refuses_bad_tables_before_any_device_call():
    good = np.column_stack([np.arange(5.0), np.arange(5.0)[::-1] * 2.0])
    bad = good.copy(); bad[3, 1] = np.nan
    rc, msg = _create(bad)
    assert rc == _lib.ERR_INVALID and "row 3" in msg and "variable 1" in msg and "drop NA rows first" in msg and "V73:154" in msg
    bad = good.copy(); bad[0, 0] = np.inf
    rc, msg = _create(bad)
    assert rc == _lib.ERR_INVALID and "row 0" in msg and "variable 0" in msg
    rc, msg = _create(good[:1])
    assert rc == _lib.ERR_INVALID and "n_ref" in msg
    rc, msg = _create(np.zeros((5, 0)))
    assert rc == _lib.ERR_INVALID and "n_vars" in msg
    bad = good.copy(); bad[:, 1] = 7.0
    rc, msg = _create(bad)
    assert rc == _lib.ERR_INVALID and "variable 1" in msg and "constant" in msg
    # a good table passes every check: what is left is the device (present and initialised, or not)
    rc, msg = _create(good)
    assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mess_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "mess_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout + pr.stderr
    lines = pr.stdout.split("\n")
    assert lines[len(HAND)] == "OK"
    for line, (p, s, i) in zip(lines, HAND):
        got = line.split()
        assert float(got[0]) == p and float(got[1]) == s and int(got[2]) == i, line
