#!/usr/bin/env python
"""Time of the three terrain calls (terrain.terrain / relief / geomorphon -> mhs_terrain_dev, mhs_relief_dev,
mhs_geomorphon_dev, csrc/terrain.hip) on a RESIDENT elevation plane of 10 000 x 10 000 cells, int16 and float32:

  * the 3 x 3 kernel with one plane (slope_deg), with four (slope_deg, aspect_deg, tpi, roughness) and with all ten, float64
    and float32 outputs;
  * relief (above_min) in a window of radius 17 cells -- the bundled relative_elevation500m;
  * geomorphons with search lengths 10 and 32.

    python tools/terrain_speed.py [--repeats 5] [--nrow 10000 --ncol 10000] [--out profiles/terrain_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the one kernel the call
enqueues.  Beside the 3 x 3 kernel's time: its one-pass bytes -- every plane element read once, every output element written
once, sizeof(type) + sizeof(out) n_out bytes per cell -- over that time, and their share of the HBM rate a streaming kernel
reaches on the MI355X (about 6.3 TB/s of the 8 TB/s peak).  The halo re-reads are served by L2 and are not counted: the share
says how far the call is from the one-pass bound.  Relief and geomorphons are bound by their LDS reads and arithmetic, not by
memory; they are given in cells per second.  There is no earlier route to compare with.  The GPU part runs in a child process
of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

HBM_ACHIEVABLE = 6.3e12       # bytes / s


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import synth, terrain
    mhs.init()
    g = synth.grid(a.nrow, a.ncol)
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(5)
    r = torch.arange(a.nrow, device=dev, dtype=torch.float32)[:, None]
    c = torch.arange(a.ncol, device=dev, dtype=torch.float32)[None, :]
    dem = 1500.0 + 400.0 * torch.sin(r / 310.0) * torch.cos(c / 270.0) + 0.05 * r + 15.0 * torch.randn((a.nrow, a.ncol), device=dev, generator=gen)
    del r, c
    out = []

    def timed(call):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        run()                                                           # warm-up
        ms = [run() for _ in range(a.repeats)]
        return {"ms": statistics.median(ms), "lo": min(ms), "hi": max(ms)}

    for dtype, esz in (("i16", 2), ("f32", 4)):
        planes = (dem.round().to(torch.int16) if dtype == "i16" else dem.clone())[None]
        stack = mhs.RasterStack(g, planes, -32768.0)
        for names in (("slope_deg",), ("slope_deg", "aspect_deg", "tpi", "roughness"), terrain.VARS):
            for odt, osz in ((torch.float64, 8), (torch.float32, 4)):
                buf = torch.empty((len(names), a.nrow, a.ncol), dtype=odt, device=dev)
                rec = timed(lambda: terrain.terrain(stack, v=names, dx=30.0, dy=30.0, out=buf, out_dtype=odt))
                rec.update(kind="terrain", dtype=dtype, n_out=len(names), out_bytes=osz, bytes=g.ncell * (esz + osz * len(names)),
                           check=float(torch.nan_to_num(buf[0]).double().mean().item()))
                out.append(rec)
                del buf
        buf = torch.empty((1, a.nrow, a.ncol), dtype=torch.float32, device=dev)
        rec = timed(lambda: terrain.relief(stack, 17, ("above_min",), out=buf, out_dtype=torch.float32))
        rec.update(kind="relief", dtype=dtype, param=17, check=float(torch.nan_to_num(buf[0]).double().mean().item()))
        out.append(rec)
        del buf
        forms = torch.empty((a.nrow, a.ncol), dtype=torch.int16, device=dev)
        for search in (10, 32):
            rec = timed(lambda: terrain.geomorphon(stack, search, 1.0, dx=30.0, dy=30.0, out=forms))
            rec.update(kind="geomorphon", dtype=dtype, param=search, check=float((forms == 6).double().mean().item()))
            out.append(rec)
        del forms, stack, planes
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--nrow", str(a.nrow),
                        "--ncol", str(a.ncol)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    ncell = a.nrow * a.ncol
    lines = ["Terrain calls on a resident elevation plane: %d x %d cells; median of %d passes after a warm-up [min .. max], device events "
             "around the call.  3 x 3 kernel: bytes = every plane element once + every output element once; share of %.1f TB/s "
             "(achievable HBM rate, 8 TB/s peak).  dx = dy = 30." % (a.nrow, a.ncol, a.repeats, HBM_ACHIEVABLE / 1e12)]
    label = {"f32": "float32", "i16": "int16"}
    for d in json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:]):
        head = "%-7s plane, " % label[d["dtype"]]
        span = "%9.3f ms [%0.3f .. %0.3f]" % (d["ms"], d["lo"], d["hi"])
        if d["kind"] == "terrain":
            rate = d["bytes"] / (d["ms"] * 1e-3)
            lines.append(head + "3 x 3, %2d float%d planes:  %s   %6.3f GB -> %6.3f TB/s = %4.1f %% of the achievable rate"
                         % (d["n_out"], 8 * d["out_bytes"], span, d["bytes"] / 1e9, rate / 1e12, 100.0 * rate / HBM_ACHIEVABLE))
        else:
            what = "relief above_min, radius %d" % d["param"] if d["kind"] == "relief" else "geomorphons, search %d" % d["param"]
            lines.append(head + "%-28s %s   %6.2f G cells / s" % (what + ":", span, ncell / (d["ms"] * 1e-3) / 1e9))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
