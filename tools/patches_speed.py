#!/usr/bin/env python
"""Time of the patches call (machisplin_amd.patches -> mhs_patches_dev, csrc/patches.hip) on a RESIDENT 10 000 x 10 000 float32
plane, connectivity 8, `label` alone and all five products, on three feature masks:

  (a) the `alt` stand-in of the bundled overviews (tools/hydro_speed.py), mirrored to that size, features where it is at most its
      median: the coastline-like mask of tools/proximity_speed.py;
  (b) random features at density 0.41;
  (c) random features at density 0.59 -- the two percolation thresholds, where patches wind through many tiles.

    python tools/patches_speed.py [--repeats 5] [--n 10000] [--out profiles/patches_speed.txt]

The call's figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the call.  `label`
alone is the library entry without an info block (three launches: tiles, borders, flatten; nothing is read back); all five
products is the Python call, which reads the info and so ends in its one synchronise.  The phases' kernel times come from a run
of their own under ``rocprofv3 --kernel-trace`` (the all-products passes only; the median over the timed ones of each kernel's
duration); without rocprofv3 they are reported as not measured.  Bytes a phase MUST move by the layout, for n cells: the tiles
read the plane and write label and the count table (12 n); the flatten reads label (4 n; it writes only words that change); the
counts read the table and label (8 n); the roots pass and the ids pass read label (4 n each); the products pass reads label and
writes the four planes (4 n + 10 n; the table look-ups through label come on top).  The border merge and the one-workgroup scan
are not streams and get no share.  The share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).  For scale only, in the same
run: ``scipy.ndimage.label`` on the CPU on a 2 000 x 2 000 crop of mask (c), and the proximity call's `dist` on mask (c).  There
is no earlier route in this library, so there is no pass mark.  The GPU parts run in child processes of their own under a time
limit."""
import argparse
import csv
import ctypes as C
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
ALL = ("label", "id", "size", "edge", "keep")
KERNELS = ("patch_tile_kernel", "patch_border_kernel", "patch_flatten_kernel", "patch_counts_kernel", "patch_roots_kernel", "patch_scan_kernel",
           "patch_ids_kernel", "patch_products_kernel")
MUST = (12, None, 4, 8, 4, None, 4, 14)                                    # bytes per cell a phase must move; None: not a stream
CROP = 2000


def device_part(a):
    import numpy as np
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import _lib
    from machisplin_amd.patches import patches
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
    cases.append(("(b) random, density 0.41", st, "lt", 0.41))
    cases.append(("(c) random, density 0.59", st, "lt", 0.59))
    label = torch.empty((n, n), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = []
    for name, stack, where, thr in cases:
        src = stack.planes
        cg = g.c_struct()
        cs = _lib.Stack(src.data_ptr(), 1, _lib.F32, src.stride(0), src.stride(1), float("nan"))
        only_label = _lib.PatchesOut(label.data_ptr(), None, None, None, None)
        code = ("na", "valid", "lt", "le").index(where)
        for products in (() if a.trace else ("label",), ALL):
            if not products:
                continue
            info = {}

            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if len(products) == 1:
                    _lib.check(_lib.lib().mhs_patches_dev(C.byref(cg), C.byref(cs), 0, code, thr, 8, 1, 2 ** 63 - 1, 0, C.byref(only_label), n, stream,
                                                          None))
                else:
                    planes, i = patches(stack, 0, where, thr, 8, products, min_size=100)
                    info.update(i)
                    del planes
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            run()                                                           # warm-up
            ms = [run() for _ in range(a.repeats)]
            out.append({"name": name, "products": len(products), "ms": statistics.median(ms), "lo": min(ms), "hi": max(ms), "cells": n * n,
                        "info": info})
    if not a.trace:                                                        # scale: proximity's dist on mask (c), and the crop for scipy
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        proximity(st, 0, "lt", 0.59, "dist", out_dtype=torch.float32)
        e0.record()
        proximity(st, 0, "lt", 0.59, "dist", out_dtype=torch.float32)
        e1.record()
        e1.synchronize()
        crop = (u[0, :CROP, :CROP] < 0.59).cpu().numpy()
        cpu = None
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            ndimage.label(crop, structure=np.ones((3, 3)))
            cpu = (time.perf_counter() - t0) * 1e3
        except ImportError:
            pass
        out.append({"proximity_ms": e0.elapsed_time(e1), "scipy_ms": cpu, "crop": list(crop.shape)})
    print("DEVICE " + json.dumps(out))


def child(a, extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--n", str(a.n)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        return None
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])


def phase_times(a, n_cases):
    """per case the median duration (ms) of each kernel over the timed all-products passes, from a rocprofv3 kernel trace of those
    passes; None without rocprofv3 or if the trace does not hold what the passes must have launched"""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    d = tempfile.mkdtemp(prefix="patch_trace_")
    try:
        if child(a, extra=["--trace"], prefix=[prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "patch", "--"]) is None:
            return None
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    k = [k for k in KERNELS if k in r["Kernel_Name"]]
                    if k:
                        rows.append((float(r["Start_Timestamp"]), k[0], (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e6))
        rows.sort()
        per_pass, nk = 1 + a.repeats, len(KERNELS)
        if len(rows) != nk * per_pass * n_cases:
            return None
        out = []
        for c in range(n_cases):
            rec = {}
            for j, k in enumerate(KERNELS):
                ms = [rows[nk * (c * per_pass + p) + j] for p in range(1, per_pass)]
                if any(m[1] != k for m in ms):
                    return None
                rec[k] = statistics.median(m[2] for m in ms)
            out.append(rec)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    recs = child(a)
    if recs is None:
        return 1
    scale, recs = recs[-1], recs[:-1]
    full = [d for d in recs if d["products"] > 1]
    phases = phase_times(a, len(full))
    lines = ["Patches on a resident %d x %d float32 plane, connectivity 8; the call: median of %d passes after a warm-up [min .. max], device "
             "events around the call; ONE run.  label alone: the library entry without an info block (tiles, borders, flatten).  Five products: "
             "the Python call (keep: min_size 100), info read back.  Phases: kernel durations from a rocprofv3 kernel trace of the five-product "
             "passes in a run of its own%s.  Bytes = what a phase must move by the layout (see the tool's text); share of 6.3 TB/s (achievable "
             "HBM rate, 8 TB/s peak); the border merge and the one-workgroup scan are not streams." % (
                 a.n, a.n, a.repeats, "" if phases else " -- NOT MEASURED in this run")]
    k_full = 0
    for d in recs:
        n, i = d["cells"], d["info"]
        tail = "" if not i else "   %d features, %d patches (largest %d cells), %d kept; scratch %.2f bytes per cell" % (
            i["n_features"], i["n_patches"], i["max_size"], i["n_kept_patches"], i["scratch_bytes"] / n)
        lines.append("%-34s %s: %9.3f ms [%0.3f .. %0.3f]%s" % (d["name"], "label alone  " if d["products"] == 1 else "five products", d["ms"], d["lo"],
                                                               d["hi"], tail))
        if d["products"] > 1:
            if phases:
                for k, per_cell in zip(KERNELS, MUST):
                    ms = phases[k_full][k]
                    if per_cell is None:
                        lines.append("    %-22s %9.3f ms" % (k, ms))
                    else:
                        tbs = per_cell * n / (ms * 1e-3) / 1e12
                        lines.append("    %-22s %9.3f ms   %6.3f GB -> %6.3f TB/s = %4.1f %% of the achievable rate" % (k, ms, per_cell * n / 1e9, tbs,
                                                                                                                      100.0 * tbs * 1e12 / HBM))
            k_full += 1
    lines.append("For scale only: scipy.ndimage.label on the CPU on a %d x %d crop of mask (c) (1/%d of the cells): %s; proximity `dist` on mask (c), "
                 "the whole plane: %.3f ms." % (scale["crop"][0], scale["crop"][1], (a.n * a.n) // (scale["crop"][0] * scale["crop"][1]),
                                                "%.0f ms" % scale["scipy_ms"] if scale["scipy_ms"] is not None else "not measured (no scipy)",
                                                scale["proximity_ms"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
