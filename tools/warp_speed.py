#!/usr/bin/env python
"""Time of the warp (machisplin_amd.project.warp -> mhs_warp_dev, csrc/warp.hip) on a RESIDENT float32 plane, float32 output:

  a 10 000 x 10 000 lon/lat plane of 1 arc second onto 10 000 x 10 000 UTM cells of 30 m, with NEAR, BILINEAR and CUBIC,
  at 1 and at 5 layers; and, in the same run, for scale, resample BILINEAR at the same size shifted by 0.37 of a cell.

    python tools/warp_speed.py [--repeats 5] [--n 10000] [--out profiles/warp_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the PYTHON call
(``project.warp`` / ``resample.resample``: the events also bracket the ctypes marshalling, tens of microseconds, of both); the
lattice is made (and measured) on the host once, outside the timed passes, and its arrays are resident.  Bytes = every source element
once + every output element once; the share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).  There is no earlier
route in this library, so there is no pass mark.  The GPU part runs in a child process of its own under a time limit."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import project as pj
    from machisplin_amd.resample import resample
    mhs.init()
    n = a.n
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(5)
    res = 1.0 / 3600.0
    src_g = mhs.Geometry(4.0, 46.0, res, res, n, n)                   # zone 31, one to four degrees off its central meridian
    crs = pj.utm(31)
    x, y = pj.transform(pj.LONLAT, crs, src_g.xmin + 0.5 * n * res, src_g.ymax - 0.5 * n * res)
    dst_g = mhs.Geometry(math.floor(float(x) / 30.0) * 30.0 - 15.0 * n, math.floor(float(y) / 30.0) * 30.0 + 15.0 * n, 30.0, 30.0, n, n)
    lat = pj.lattice(pj.LONLAT, crs, dst_g, src_g, tol=0.01)
    shift_g = mhs.Geometry(src_g.xmin + 0.37 * res, src_g.ymax - 0.37 * res, res, res, n, n)
    out = [{"note": "lattice: step %d, %d x %d nodes, measured error %.3g source cells at %d points" %
                    (lat.step, lat.sx.shape[0], lat.sx.shape[1], lat.max_error, lat.n_checked)}]

    def timed(call):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        run()                                                           # warm-up (the lattice goes up here)
        ms = [run() for _ in range(a.repeats)]
        return {"ms": statistics.median(ms), "lo": min(ms), "hi": max(ms)}

    for layers in (1, 5):
        stack = mhs.RasterStack(src_g, 100.0 * torch.randn((layers, n, n), device=dev, generator=gen, dtype=torch.float32), -32768.0)
        buf = torch.empty((layers, n, n), dtype=torch.float32, device=dev)
        for method in ("near", "bilinear", "cubic"):
            rec = timed(lambda: pj.warp(stack, dst_g, lat, method, out=buf))
            rec.update(name="warp %d^2 1'' -> UTM 30 m, %s, %d layer%s" % (n, method, layers, "" if layers == 1 else "s"), bytes=8 * n * n * layers,
                       valid=float((~torch.isnan(buf[0, ::97, ::89])).double().mean()))
            out.append(rec)
        if layers == 1:
            rec = timed(lambda: resample(stack, shift_g, "bilinear", out=buf))
            rec.update(name="    resample %d^2 shifted 0.37 cell, bilinear, 1 layer (for scale)" % n, bytes=8 * n * n, valid=float((~torch.isnan(buf[0, ::97, ::89])).double().mean()))
            out.append(rec)
        del stack, buf
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the planes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--n", str(a.n)],
                       capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    recs = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
    lines = ["Warp of a resident float32 plane, float32 output; median of %d passes after a warm-up [min .. max], device events around the "
             "Python call (its marshalling, tens of microseconds, included); the lattice is made on the host outside the timed passes.  Bytes = every source element once + every output element "
             "once; share of 6.3 TB/s (achievable HBM rate, 8 TB/s peak).  valid = share of a sample of the output that is not NA." % a.repeats]
    for d in recs:
        if "note" in d:
            lines.append(d["note"])
            continue
        tbs = d["bytes"] / (d["ms"] * 1e-3) / 1e12
        lines.append("%-72s %9.3f ms [%0.3f .. %0.3f]   %6.3f GB -> %6.3f TB/s = %4.1f %% of the achievable rate   valid %.3f" %
                     (d["name"] + ":", d["ms"], d["lo"], d["hi"], d["bytes"] / 1e9, tbs, 100.0 * tbs * 1e12 / HBM, d["valid"]))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
