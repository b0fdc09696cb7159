"""CPU: the plan of the fits' staging block (machisplin_amd/csrc/fit_stage.h: typed pieces on 16-byte boundaries, marks,
the host mirror of one byte range) needs no HIP header, so a plain C++17 compiler builds tests/fit_stage_check.cpp
against it and the program's own asserts run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fit_stage_plan_with_a_plain_cxx_compiler(tmp_path):
    exe = str(tmp_path / "fit_stage_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "fit_stage_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    assert "warning" not in pr.stderr, pr.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("fit_stage OK"), run.stdout
