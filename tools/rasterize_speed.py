#!/usr/bin/env python
"""Time of the rasterize call (machisplin_amd.rasterize -> mhs_rasterize_dev, csrc/rasterize.hip) on a 10 000 x 10 000 grid, on
five sets of features made here with numpy:

  (a) one coastline-like polygon: a star of 10^6 vertices whose radius wanders, `index`;
  (b) a partition of the grid into 55 x 55 = 3 025 polygons, a jittered lattice whose cells share their edges, `index`;
  (c) 10^5 line segments of up to 300 cells, each a feature, `index`;
  (d) 10^6 points, each a feature, `index` and `count`;
  (e) one rectangle that contains the whole grid, `index`: every cell receives one atomicMax of the fill phase, and nothing else
      of the call is large -- the cost of the per-cell atomic.

    python tools/rasterize_speed.py [--repeats 5] [--n 10000] [--out profiles/rasterize_speed.txt]

A figure is the median of ``--repeats`` timed calls after one warm-up call, device events around the Python call (so the host's
passes over the geometry, its copy to the device and the one synchronisation inside the call are in it).  The phases are each
kernel's mean duration per call from a ``rocprofv3 --kernel-trace`` run of its own per case (a fresh process; warm-up included);
without rocprofv3 they are reported as not measured.  For scale only: ``matplotlib.path.Path.contains_points`` on the CPU with
polygon (a) scaled to a 2 000 x 2 000 grid, timed on ONE COLUMN of 2 000 cell centres -- its cost is points x vertices, so the
whole grid is 2 000 times that, which is stated as an extrapolation, not a measurement.  There is no earlier route in this
library, so there is no pass mark."""
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

CASES = ("a", "b", "c", "d", "e")
NAMES = {"a": "(a) one polygon of 10^6 vertices", "b": "(b) 3 025 polygons that share edges", "c": "(c) 10^5 line segments", "d": "(d) 10^6 points, with count",
         "e": "(e) one rectangle over the whole grid"}
KERNELS = ("rz_init_kernel", "rz_count_kernel", "rz_scan_kernel", "rz_prefix_kernel", "rz_gather_kernel", "rz_cross_kernel", "rz_span_kernel",
           "rz_fill_kernel", "rz_points_kernel", "rz_products_kernel")


def star(n_vertices, cx, cy, radius, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, n_vertices))
    wander = 1.0 + 0.25 * np.sin(7.0 * a) + 0.1 * np.sin(61.0 * a) + 0.03 * np.sin(977.0 * a) + 0.01 * rng.uniform(-1.0, 1.0, n_vertices)
    xy = np.column_stack([cx + radius * wander * np.cos(a), cy + radius * wander * np.sin(a)])
    return np.vstack([xy, xy[:1]])


def features(case, g):
    import numpy as np
    from machisplin_amd.vector import Features
    n = g.nrow
    rng = np.random.default_rng(7)
    if case == "a":
        return Features.from_parts("polygon", [[star(10 ** 6, g.xmin + 0.5 * n * g.xres, g.ymax - 0.5 * n * g.yres, 0.33 * n * g.xres)]]), ("index",)
    if case == "b":
        k = 55
        X = g.xmin + np.arange(k + 1) * (n * g.xres / k) + np.zeros((k + 1, 1))
        Y = g.ymax - np.arange(k + 1)[:, None] * (n * g.yres / k) + np.zeros((1, k + 1))
        X[1:-1, 1:-1] += rng.uniform(-0.3, 0.3, (k - 1, k - 1)) * n * g.xres / k
        Y[1:-1, 1:-1] += rng.uniform(-0.3, 0.3, (k - 1, k - 1)) * n * g.yres / k
        i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
        corners = [(i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j), (i, j)]
        coords = np.stack([np.stack([X[a, b].ravel(), Y[a, b].ravel()], axis=1) for a, b in corners], axis=1).reshape(-1, 2)
        return Features("polygon", coords, np.arange(0, 5 * k * k + 1, 5), np.arange(k * k + 1)), ("index",)
    if case == "c":
        m = 10 ** 5
        p = np.column_stack([g.xmin + rng.uniform(0, n, m) * g.xres, g.ymax - rng.uniform(0, n, m) * g.yres])
        q = p + rng.uniform(-300.0, 300.0, (m, 2)) * np.array([g.xres, g.yres])
        return Features("line", np.stack([p, q], axis=1).reshape(-1, 2), np.arange(0, 2 * m + 1, 2), np.arange(m + 1)), ("index",)
    if case == "d":
        m = 10 ** 6
        p = np.column_stack([g.xmin + rng.uniform(0, n, m) * g.xres, g.ymax - rng.uniform(0, n, m) * g.yres])
        return Features("point", p, np.arange(m + 1), np.arange(m + 1)), ("index", "count")
    x0, x1, y0, y1 = g.xmin - g.xres, g.xmin + (n + 1) * g.xres, g.ymax - (n + 1) * g.yres, g.ymax + g.yres
    return Features.from_parts("polygon", [[np.array([[x0, y1], [x1, y1], [x1, y0], [x0, y0], [x0, y1]])]]), ("index",)


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd.rasterize import rasterize
    mhs.init()
    n = a.n
    g = mhs.Geometry(1000.0, 5000.0 + 30.0 * n, 30.0, 30.0, n, n)
    out = []
    for case in (a.case,) if a.case else CASES:
        ft, products = features(case, g)
        info = {}

        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            planes, i = rasterize(ft, g, products)
            e1.record()
            e1.synchronize()
            info.update(i)
            del planes
            return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3
        run()                                                               # warm-up
        ms = [run() for _ in range(a.repeats)]
        out.append({"case": case, "ms": statistics.median(m[0] for m in ms), "lo": min(m[0] for m in ms), "hi": max(m[0] for m in ms),
                    "wall_ms": statistics.median(m[1] for m in ms), "info": info})
    print("DEVICE " + json.dumps(out))


def child(a, extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--n", str(a.n)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        return None
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])


def phase_times(a, case):
    """each kernel's mean duration per call (ms) over the 1 + repeats calls of one case, from a rocprofv3 kernel trace of a process
    of its own; None without rocprofv3"""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    d = tempfile.mkdtemp(prefix="rz_trace_")
    try:
        if child(a, extra=["--case", case], prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "rz", "--"]) is None:
            return None
        total = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    for k in KERNELS:
                        if k in r["Kernel_Name"]:
                            total[k] = total.get(k, 0.0) + (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e6
        return {k: v / (1 + a.repeats) for k, v in total.items()} or None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def matplotlib_scale():
    """seconds of Path.contains_points for 2 000 cell centres (one column of a 2 000 x 2 000 grid) against polygon (a); None without matplotlib"""
    try:
        from matplotlib.path import Path
    except ImportError:
        return None
    import numpy as np
    path = Path(star(10 ** 6, 1000.0, 1000.0, 660.0))
    pts = np.column_stack([np.full(2000, 1000.5), np.arange(2000) + 0.5])
    t0 = time.perf_counter()
    path.contains_points(pts)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rasterize_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--case", default=None, choices=CASES, help=argparse.SUPPRESS)
    ap.add_argument("--no-trace", action="store_true", help="leave the phase times out")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    recs = child(a)
    if recs is None:
        return 1
    lines = ["Rasterize onto a %d x %d grid; the call: median of %d calls after a warm-up [min .. max], device events around the Python call (the "
             "host's passes over the geometry, its copy to the device and the call's synchronisations are in it); ONE run.  Phases: each kernel's "
             "mean duration per call from a rocprofv3 kernel trace in a process of its own per case." % (a.n, a.n, a.repeats)]
    for d in recs:
        i = d["info"]
        lines.append("%-40s %9.3f ms [%0.3f .. %0.3f]   %d features, %d vertices, %d items, %d cells burned; %d batch(es), scratch %.1f MiB" % (
            NAMES[d["case"]], d["ms"], d["lo"], d["hi"], i["n_features"], i["n_vertices"], i["n_items"], i["n_burned"], i["n_batches"],
            i["scratch_bytes"] / 2 ** 20))
        phases = None if a.no_trace else phase_times(a, d["case"])
        if phases is None:
            lines.append("    phases: NOT MEASURED in this run")
        else:
            lines.append("    " + "   ".join("%s %.3f" % (k.replace("rz_", "").replace("_kernel", ""), phases[k]) for k in KERNELS if k in phases) +
                         "   (ms; sum %.3f)" % sum(phases.values()))
    s = matplotlib_scale()
    lines.append("For scale only: matplotlib.path.Path.contains_points on the CPU, polygon (a) against ONE COLUMN of 2 000 cell centres of a 2 000 x 2 000 "
                 "grid: %s" % ("not measured (no matplotlib)" if s is None else
                               "%.2f s; its cost is points x vertices, so the whole grid would be 2 000 times that, about %.0f s (extrapolated, not measured)." % (s, 2000 * s)))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
