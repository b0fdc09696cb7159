#!/usr/bin/env python
"""Time of the proximity call (machisplin_amd.proximity -> mhs_proximity_dev, csrc/proximity.hip) on a RESIDENT
10 000 x 10 000 float32 plane, float32 products, `dist` alone and all six products, on three feature masks:

  (a) the `alt` stand-in of the bundled overviews (tools/hydro_speed.py), mirrored to that size, features where it is at most its
      median: a coastline-like mask;
  (b) random features at density 1e-5;
  (c) random features at density 0.5.

    python tools/proximity_speed.py [--repeats 5] [--n 10000] [--out profiles/proximity_speed.txt]

The call's figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the call (info is
read, so the call ends in its one synchronise).  The three phases' kernel times come from a run of their own under
``rocprofv3 --kernel-trace`` (the same passes; the median over the timed ones of each kernel's duration); without rocprofv3 they
are reported as not measured.  Bytes a phase MUST move, for n cells: A reads the plane and writes near (8 n); B1 reads near and
writes at most one stack entry per cell (4 n + 8 n); B2 reads near and the stack entries and writes the products (12 n + 4 n for
`dist`, + 24 n for all six).  The share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).  scipy's
``distance_transform_edt`` on the CPU at 2 000 x 2 000 is timed in the same run as a statement of scale only.  There is no earlier
route in this library, so there is no pass mark.  The GPU parts run in child processes of their own under a time limit."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.3e12
ALL = ("d2", "index", "dist", "dir_x", "dir_y", "value")
KERNELS = ("prox_rows_kernel", "prox_cols_kernel", "prox_cells_kernel")


def device_part(a):
    import numpy as np
    import torch
    import machisplin_amd as mhs
    from machisplin_amd.proximity import proximity
    from hydro_speed import alt_stand_in
    mhs.init()
    n = a.n
    dev = torch.device("cuda", torch.cuda.current_device())
    g = mhs.Geometry(1000.0, 5000.0 + 30.0 * n, 30.0, 30.0, n, n)
    gen = torch.Generator(device=dev).manual_seed(5)
    cases = []
    alt = alt_stand_in(n, n)
    if alt is not None:
        med = float(np.nanmedian(alt))
        cases.append(("(a) alt stand-in <= its median", mhs.RasterStack(g, torch.from_numpy(alt)[None], float("nan")), "le", med))
    u = torch.rand((1, n, n), device=dev, generator=gen, dtype=torch.float32)
    st = mhs.RasterStack(g, u, float("nan"))
    cases.append(("(b) random, density 1e-5", st, "lt", 1e-5))
    cases.append(("(c) random, density 0.5", st, "lt", 0.5))
    out = []
    for name, stack, where, thr in cases:
        for products in (("dist",), ALL):
            info = {}

            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                planes, i = proximity(stack, 0, where, thr, products, value_layer=0, out_dtype=torch.float32)
                e1.record()
                e1.synchronize()
                info.update(i)
                del planes
                return e0.elapsed_time(e1)
            run()                                                           # warm-up
            ms = [run() for _ in range(a.repeats)]
            out.append({"name": name, "products": len(products), "ms": statistics.median(ms), "lo": min(ms), "hi": max(ms), "cells": n * n,
                        "n_features": info["n_features"], "max_d2": info["max_d2"], "scratch_bytes": info["scratch_bytes"]})
    print("DEVICE " + json.dumps(out))


def child(a, extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--n", str(a.n)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        return None
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])


def phase_times(a, n_cases):
    """per case the median duration (ms) of each of the three kernels over the timed passes, from a rocprofv3 kernel trace of the
    same passes; None without rocprofv3 or if the trace does not hold what the passes must have launched"""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    d = tempfile.mkdtemp(prefix="prox_trace_")
    try:
        if child(a, prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "prox", "--"]) is None:
            return None
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    k = [k for k in KERNELS if k in r["Kernel_Name"]]
                    if k:
                        rows.append((float(r["Start_Timestamp"]), k[0], (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e6))
        rows.sort()
        per_pass = 1 + a.repeats
        if len(rows) != 3 * per_pass * n_cases:
            return None
        out = []
        for c in range(n_cases):
            rec = {}
            for j, k in enumerate(KERNELS):
                ms = [rows[3 * (c * per_pass + p) + j] for p in range(1, per_pass)]
                if any(m[1] != k for m in ms):
                    return None
                rec[k] = statistics.median(m[2] for m in ms)
            out.append(rec)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def scipy_scale():
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        return None
    mask = np.random.default_rng(5).random((2000, 2000)) < 1e-3
    t0 = time.perf_counter()
    ndimage.distance_transform_edt(~mask)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proximity_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    recs = child(a)
    if recs is None:
        return 1
    phases = phase_times(a, len(recs))
    lines = ["Proximity on a resident %d x %d float32 plane, float32 products; the call: median of %d passes after a warm-up [min .. max], "
             "device events around the call.  Phases A (rows), B1 (columns), B2 (cells): kernel durations from a rocprofv3 kernel trace of "
             "the same passes in a run of its own%s.  Bytes = what a phase must move (see the tool's text); share of 6.3 TB/s (achievable "
             "HBM rate, 8 TB/s peak).  Scratch: %.2f bytes per cell." % (a.n, a.n, a.repeats, "" if phases else " -- NOT MEASURED in this run",
                                                                     recs[0]["scratch_bytes"] / recs[0]["cells"])]
    for i, d in enumerate(recs):
        n = d["cells"]
        lines.append("%-34s %s: %9.3f ms [%0.3f .. %0.3f]   %d features, max d2 %d" % (d["name"], "dist alone " if d["products"] == 1 else "six products",
                                                                                   d["ms"], d["lo"], d["hi"], d["n_features"], d["max_d2"]))
        if phases:
            must = (8 * n, 12 * n, 12 * n + (4 if d["products"] == 1 else 24) * n)
            for k, b, label in zip(KERNELS, must, ("A  rows", "B1 columns", "B2 cells")):
                ms = phases[i][k]
                tbs = b / (ms * 1e-3) / 1e12
                lines.append("    %-11s %9.3f ms   %6.3f GB -> %6.3f TB/s = %4.1f %% of the achievable rate" % (label, ms, b / 1e9, tbs, 100.0 * tbs * 1e12 / HBM))
    cpu = scipy_scale()
    lines.append("scipy.ndimage.distance_transform_edt on the CPU, 2 000 x 2 000 (1/25 of the cells), density 1e-3: %s -- scale only, another "
                 "machine part and another size." % ("%.0f ms" % cpu if cpu is not None else "not measured (no scipy)"))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
