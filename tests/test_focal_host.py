"""Host: the focal rule without a GPU.  The numpy restatement of the section "focal" (tests/focal_ref.py) against the rule header
csrc/focal_rule.h compiled into a plain C++ program under AddressSanitizer and UBSan (tests/focal_check.cpp), bit for bit; and
against a brute-force window loop in np.longdouble, within the bound the header derives."""
import os
import subprocess

import numpy as np
import pytest

import focal_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = ("count", "sum", "mean", "sd", "minus_mean", "dev")


def _check_plane():
    """the plane tests/focal_check.cpp makes"""
    nr, nc = 70, 150
    z = np.empty(nr * nc)
    x = 0x9E3779B97F4A7C15
    for i in range(nr * nc):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        z[i] = 1200.0 + float(x >> 11) * (600.0 / 9007199254740992.0)
        if i % 17 == 3 or i // nc == 5:
            z[i] = np.nan
    z[40 * nc + 7] = -9999.0
    return z.reshape(nr, nc)


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "focal_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "focal_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr
    lines = pr.stdout.split("\n")
    n_lines = 3 * 2 * len(fr.STATS) + 2 * 2 * len(SUMS)              # every statistic for the squares, the sum family for the circles
    assert lines[-2] == "OK" and len(lines) == n_lines + 2
    z = _check_plane()
    seen = set()
    for ln in lines[:-2]:
        shape, R, fill, name, *words = ln.split()
        got = np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64).reshape(z.shape)
        want = fr.focal(z, -9999.0, int(R), (name,), shape, bool(int(fill)), 1500.0)[0]
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got) & ~np.isnan(got), np.signbit(want) & ~np.isnan(want)), ln[:40]
        seen.add((shape, int(R), int(fill), name))
    assert len(seen) == n_lines


@pytest.mark.parametrize("shape", ("square", "circle"))
@pytest.mark.parametrize("offset", (0.0, 2000.0))
def test_restatement_within_the_derived_bound_of_an_extended_precision_loop(shape, offset):
    rng = np.random.default_rng(5)
    z = 2000.0 + 5.0 * rng.standard_normal((70, 150))               # the elevations the offset is for: mean 2 000, sd 5
    z[20] = np.nan
    z[30:34, 40:49] = -9999.0
    for R in (1, 7, 65):
        n, S1, S2 = fr.sums(z, -9999.0, R, shape, offset)
        bn, b1, b2, _, _ = fr.brute(z, -9999.0, R, shape, offset, np.longdouble)
        assert np.array_equal(n, bn)
        e1, e2 = float(np.abs(S1 - b1).max()), float(np.abs(S2 - b2).max())
        t1, t2 = fr.bound(z, -9999.0, R, shape, offset, 1), fr.bound(z, -9999.0, R, shape, offset, 2)
        print(f"{shape} R = {R} offset = {offset}: |S1 - exact| = {e1:.3e} (bound {t1:.3e}), |S2 - exact| = {e2:.3e} (bound {t2:.3e})")
        assert e1 <= t1 and e2 <= t2


def test_the_offset_keeps_sd_sound():
    """sd of elevations of mean 2 000 and sd 5: with the offset the formula loses nothing, as the bound says"""
    rng = np.random.default_rng(6)
    z = 2000.0 + 5.0 * rng.standard_normal((40, 90))
    ok = np.ones(z.shape, dtype=bool)
    n, S1, S2 = fr.sums(z, np.nan, 4, "square", 2000.0)
    sd = fr.statistics(n, S1, S2, z, ok, 2000.0, False)["sd"]
    bn, b1, b2, _, _ = fr.brute(z, np.nan, 4, "square", 2000.0, np.longdouble)
    exact = np.sqrt((b2 - b1 * b1 / bn) / (bn - 1)).astype(np.float64)
    # var = (S2 - S1^2 / n) / (n - 1): its error is at most (E2 + 2 |S1| E1 / n + 3 u (S2 + S1^2 / n)) / (n - 1), and sd's half of that over sd
    E1, E2 = fr.bound(z, np.nan, 4, "square", 2000.0, 1), fr.bound(z, np.nan, 4, "square", 2000.0, 2)
    tol = (E2 + 2.0 * np.abs(S1) * E1 / n + 3.0 * fr.U * (S2 + S1 * S1 / n)) / (n - 1) / (2.0 * exact) * 1.01 + 2.0 * fr.U * exact
    assert (np.abs(sd - exact) <= tol).all() and tol.max() < 1e-9


def test_restated_min_and_max_equal_the_window_loop():
    rng = np.random.default_rng(8)
    z = rng.standard_normal((40, 90))
    z[10] = np.nan
    z[rng.random(z.shape) < 0.1] = -9999.0
    for R in (1, 5, 64, 90):
        mn, mx = fr.minmax(z, -9999.0, R)
        _, _, _, bmn, bmx = fr.brute(z, -9999.0, R)
        assert np.array_equal(mn, bmn) and np.array_equal(mx, bmx)


def test_blocked_prefix_is_the_header_rule_written_as_one_loop():
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, 200):
        x = rng.standard_normal(n) * 1e3
        P = np.empty(n)
        run = 0.0
        for b0 in range(0, n, fr.B):
            s = 0.0
            for i in range(b0, min(n, b0 + fr.B)):
                s = x[i] if i == b0 else s + x[i]
                P[i] = run + s
            run = run + s
        assert np.array_equal(P, fr.blocked_prefix(x, 0))
    assert [fr.half_width(5, d) for d in range(6)] == [5, 4, 4, 4, 3, 0] and fr.half_width(45, 45) == 0 and fr.half_width(700, 0) == 700
