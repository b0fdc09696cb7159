#!/usr/bin/env python
"""Time of the MESS grid call (Mess.grid -> mhs_mess_grid_dev, csrc/mess.hip) on RESIDENT planes at cfg3's shape: 5 covariate
layers, 10 000 x 10 000 cells, 5 000 reference rows (the stations' own cells), for float32 and int16 planes, with and without
the MoD plane, with and without LONG / LAT among the variables.

    python tools/mess_speed.py [--repeats 5] [--nrow 10000 --ncol 10000 --stations 5000] [--out profiles/mess_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the one kernel the call
enqueues.  Beside the time: the bytes the algorithm needs -- every plane element read once, every output element written once,
C sizeof(type) + 8 (+ 4) bytes per cell -- over that time, and its share of the HBM rate a streaming kernel can reach on the
MI355X (about 6.3 TB/s of the 8 TB/s peak).  The searches of the sorted tables are served by LDS and L2 and are not counted as
traffic: the share says how far the call is from the one-pass bound, not how busy the memory system is.  The GPU part runs in
a child process of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

C_LAYERS = 5
HBM_ACHIEVABLE = 6.3e12       # bytes / s


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import synth
    mhs.init()
    g = synth.grid(a.nrow, a.ncol)
    xy, _, _, _ = synth.stations(g, a.stations, 3)
    out = []
    for dtype, esz in (("f32", 4), ("i16", 2)):
        planes, nodata = synth.covariates(g, C_LAYERS, 3, dtype=dtype)
        stack = mhs.RasterStack(g, planes, nodata)
        X, _, _ = mhs.mltps.station_predictors(stack, xy)
        X = X[~np.isnan(X).any(axis=1)]
        mess = torch.empty((g.nrow, g.ncol), dtype=torch.float64, device=planes.device)
        mod = torch.empty((g.nrow, g.ncol), dtype=torch.int32, device=planes.device)
        for lonlat in (False, True):
            m = mhs.Mess(X if lonlat else X[:, :C_LAYERS])
            for with_mod in (False, True):
                def run():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    m.grid(stack, out=mess, mod=mod if with_mod else False)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                run()                                                   # warm-up
                ms = [run() for _ in range(a.repeats)]
                negative = int((mess < 0).sum().item())
                out.append({"dtype": dtype, "lonlat": lonlat, "mod": with_mod, "n_ref": int(X.shape[0]), "ms": statistics.median(ms),
                            "lo": min(ms), "hi": max(ms), "bytes": g.ncell * (C_LAYERS * esz + 8 + (4 if with_mod else 0)),
                            "negative": negative})
            del m
        del stack, planes
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--stations", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mess_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--nrow", str(a.nrow),
                        "--ncol", str(a.ncol), "--stations", str(a.stations)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    lines = ["MESS grid call on resident planes: %d layers, %d x %d cells, %d stations; median of %d passes after a warm-up [min .. max], "
             "device events around the call; bytes = every plane element once + every output element once; share of %.1f TB/s "
             "(achievable HBM rate, 8 TB/s peak)" % (C_LAYERS, a.nrow, a.ncol, a.stations, a.repeats, HBM_ACHIEVABLE / 1e12)]
    for d in json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:]):
        rate = d["bytes"] / (d["ms"] * 1e-3)
        lines.append("%-7s planes, %d variables%s, %s:  %8.3f ms [%0.3f .. %0.3f]   %6.3f GB -> %6.3f TB/s = %4.1f %% of the achievable rate   "
                     "(%d reference rows, %d cells with MESS < 0)"
                     % ({"f32": "float32", "i16": "int16"}[d["dtype"]], C_LAYERS + 2 * d["lonlat"], " (LONG, LAT)" if d["lonlat"] else "",
                        "MESS + MoD" if d["mod"] else "MESS only ", d["ms"], d["lo"], d["hi"], d["bytes"] / 1e9, rate / 1e12,
                        100.0 * rate / HBM_ACHIEVABLE, d["n_ref"], d["negative"]))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
