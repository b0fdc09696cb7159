"""GPU: the device sort of 64-bit keys (include/machisplin_hip.h, section "sort"; csrc/sort_keys.hip).  The sorted bytes equal
numpy.sort's, for every number of keys around the wave and tile sizes (SORT_TILE_KEYS, read from the text of csrc/sort_keys.h)
crossed with key sets that pin each property: equal keys (every pass skipped), keys that differ in one, two or three bytes (the
passes that run, and in which buffer the result ends), sorted and reversed input, and two values alternating lane by lane and
tile by tile, where every wave holds both digits and an unstable or racy pass shows."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", "sort_keys.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


T = _constant("SORT_TILE_KEYS")
assert _constant("SORT_RADIX_BITS") == 8
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37)
BASE = np.uint64(0x5A3C_0000_1200_0034)


def key_sets(n):
    """name -> (uint64 keys, the number of passes that must run, or None where it depends on the draw)"""
    rng = np.random.default_rng(1000 + n)
    i = np.arange(n, dtype=np.uint64)
    rnd = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    byte = lambda k: rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * k)       # noqa: E731
    many = n >= 64                                                                       # enough keys that every drawn byte varies
    two = BASE | byte(1) | byte(6)
    three = BASE | byte(0) | byte(3) | byte(7)
    return {
        "random": (rnd, None),
        "equal": (np.full(n, BASE, dtype=np.uint64), 0),
        "low_byte": (BASE | byte(0), 1 if many else None),
        "bits_32_39": (BASE | byte(4), 1 if many else None),
        "two_bytes": (two, 2 if many else None),
        "three_bytes": (three, 3 if many else None),
        "sorted": (np.sort(rnd), None),
        "reversed": (np.sort(rnd)[::-1].copy(), None),
        # two values that differ in two digits, alternating by lane and by tile: equal digits of either pass sit in every wave
        "alternating": (np.where((i + i // np.uint64(T)) % np.uint64(2) == 0, BASE | np.uint64(0x0000_0000_0000_0100), BASE | np.uint64(0x0001_0000_0000_0000)),
                        2 if n >= 2 else 0),
    }


def _sort(hip, keys, **kw):
    import torch
    t = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    info = hip.zonal.sort_keys(t, **kw)
    return t.cpu().numpy().view(np.uint64), info


@pytest.mark.parametrize("n", SIZES)
def test_sorted_bytes_equal_numpy(hip, n):
    for name, (keys, passes) in key_sets(n).items():
        got, info = _sort(hip, keys)
        want = np.sort(keys)
        assert got.tobytes() == want.tobytes(), (n, name)
        if passes is not None:
            assert info["passes_run"] == passes, (n, name, info)
        assert info["passes_run"] <= 8
        if n:
            assert 8 * n <= info["scratch_bytes"] <= 8 * n + 256 + 1024 * (-(-n // T)) + 256 + 8192, (n, info)
        else:
            assert info == {"passes_run": 0, "scratch_bytes": 0}


def test_stability_shows_in_a_window_that_hides_the_low_bits(hip):
    """Sorting by the bits 16 .. 23 alone must keep the input order of keys with equal bits there: the low 16 bits carry the
    input index, so the result is numpy's STABLE sort by that byte -- over several tiles, every wave holding every digit."""
    n = 3 * T + 5
    rng = np.random.default_rng(7)
    keys = (rng.integers(0, 4, n, dtype=np.uint64) << np.uint64(16)) | np.arange(n, dtype=np.uint64)
    got, info = _sort(hip, keys, bit_lo=16, bit_hi=24)
    order = np.argsort((keys >> np.uint64(16)) & np.uint64(0xFF), kind="stable")
    assert got.tobytes() == keys[order].tobytes() and info["passes_run"] == 1
    # a window of 3 bits inside a byte, and one that spans two digits with a narrow last digit
    keys = rng.integers(0, 2 ** 20, n, dtype=np.uint64)
    for lo, hi in ((5, 8), (3, 14), (0, 20), (12, 12)):
        got, info = _sort(hip, keys, bit_lo=lo, bit_hi=hi)
        digit = (keys >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)
        assert got.tobytes() == keys[np.argsort(digit, kind="stable")].tobytes(), (lo, hi)
        assert info["passes_run"] == -(-(hi - lo) // 8), (lo, hi, info)


def test_windows_that_cut_off_equal_high_bits(hip):
    n = 2 * T + 37
    rng = np.random.default_rng(11)
    keys = (np.uint64(0xABCD) << np.uint64(48)) | rng.integers(0, 2 ** 41, n, dtype=np.uint64)
    want = np.sort(keys)
    for lo, hi in ((0, 41), (0, 48), (0, 64)):
        got, info = _sort(hip, keys, bit_lo=lo, bit_hi=hi)
        assert got.tobytes() == want.tobytes() and info["passes_run"] == 6, (lo, hi, info)


def test_the_same_call_twice_gives_the_same_bytes_and_a_storage_offset_is_respected(hip):
    import torch
    n = 2 * T + 37
    rng = np.random.default_rng(13)
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64) & np.uint64(0x0000_00FF_0000_FFFF)     # many ties
    a, _ = _sort(hip, keys)
    b, _ = _sort(hip, keys)
    assert a.tobytes() == b.tobytes() == np.sort(keys).tobytes()
    # a view into a larger tensor: the neighbours keep their values
    big = torch.full((n + 10,), 7, dtype=torch.int64, device="cuda")
    view = big[3:3 + n]
    view.copy_(torch.from_numpy(keys.view(np.int64).copy()))
    assert view.storage_offset() == 3
    hip.zonal.sort_keys(view)
    out = big.cpu().numpy()
    assert out[3:3 + n].view(np.uint64).tobytes() == np.sort(keys).tobytes() and (out[:3] == 7).all() and (out[3 + n:] == 7).all()
    # uint64 tensors are taken as they are
    u = torch.from_numpy(keys.view(np.int64).copy()).cuda().view(torch.uint64)
    hip.zonal.sort_keys(u)
    assert u.view(torch.int64).cpu().numpy().view(np.uint64).tobytes() == np.sort(keys).tobytes()
