"""CPU: the two process-wide settings of the TPS standard errors (mhs_tps_se_max_n, mhs_tps_se_build_mode) through
ctypes -- ranges, the value handed back, and that neither needs an initialised device."""
import ctypes as C

import pytest

from machisplin_amd import _lib

SE_MAX_N, SE_HARD_MAX_N = 2048, 20000


@pytest.fixture(autouse=True)
def _restore_settings():
    yield
    lib = _lib.load()
    assert lib.mhs_tps_se_build_mode(0) == _lib.OK
    assert lib.mhs_tps_se_max_n(SE_MAX_N, None) == _lib.OK


def test_max_n_returns_the_previous_value_and_checks_its_range():
    lib = _lib.load()          # dlopen only: no mhs_init
    prev = C.c_int64(-1)
    assert lib.mhs_tps_se_max_n(4096, C.byref(prev)) == _lib.OK
    assert prev.value == SE_MAX_N
    assert lib.mhs_tps_se_max_n(SE_HARD_MAX_N, C.byref(prev)) == _lib.OK
    assert prev.value == 4096
    assert lib.mhs_tps_se_max_n(1, C.byref(prev)) == _lib.OK
    assert prev.value == SE_HARD_MAX_N
    for bad in (0, -1, SE_HARD_MAX_N + 1):
        prev.value = -7
        assert lib.mhs_tps_se_max_n(bad, C.byref(prev)) == _lib.ERR_INVALID
        assert prev.value == -7                      # nothing written, nothing changed
        assert b"mhs_tps_se_max_n" in lib.mhs_last_error()
    assert lib.mhs_tps_se_max_n(SE_MAX_N, C.byref(prev)) == _lib.OK
    assert prev.value == 1
    assert lib.mhs_tps_se_max_n(SE_MAX_N, None) == _lib.OK      # previous may be NULL


def test_build_mode_checks_its_range():
    lib = _lib.load()
    for mode in (0, 1, 2):
        assert lib.mhs_tps_se_build_mode(mode) == _lib.OK
    for bad in (3, -1):
        assert lib.mhs_tps_se_build_mode(bad) == _lib.ERR_INVALID


def test_python_wrappers_need_no_device():
    import machisplin_amd as mhs
    assert (mhs.SE_BUILD_AUTO, mhs.SE_BUILD_HOST, mhs.SE_BUILD_DEVICE) == (0, 1, 2)
    assert mhs.se_max_n(3000) == SE_MAX_N
    assert mhs.se_max_n(SE_MAX_N) == 3000
    mhs.se_build_mode(mhs.SE_BUILD_DEVICE)
    mhs.se_build_mode(mhs.SE_BUILD_AUTO)
    with pytest.raises(mhs.MhsError) as ei:
        mhs.se_build_mode(3)
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(mhs.MhsError) as ei:
        mhs.se_max_n(SE_HARD_MAX_N + 1)
    assert ei.value.code == _lib.ERR_INVALID
