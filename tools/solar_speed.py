#!/usr/bin/env python
"""Time of the solar call (terrain.solar -> mhs_solar_dev, solar_kernel of csrc/terrain.hip) on a RESIDENT float32 elevation
plane of 10 000 x 10 000 cells, search lengths 10 and 32, float32 outputs:

  * svf alone (the sixteen rays and sixteen divisions, no table walk, no slope);
  * svf, direct and sun_hours together (the rays, the Horn slope and the walk over the default sun tables: four days, steps
    of 30 minutes, latitude 45);
  * horizon alone (the rays, sixteen planes written);
  * and, in the same run, geomorphons at the same search length -- the only related figure: 8 rays that stop at an NA against
    16 that do not.

    python tools/solar_speed.py [--repeats 5] [--nrow 10000 --ncol 10000] [--out profiles/solar_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the call (the upload of
the tables, a few kilobytes, is part of it).  The kernels are bound by their LDS reads and float64 arithmetic, not by memory;
they are given in cells per second.  There is no earlier route to compare with, so there is no pass mark.  The GPU part runs
in a child process of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCTS = (("svf",), ("svf", "direct", "sun_hours"), ("horizon",))


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
    stack = mhs.RasterStack(g, dem[None], -32768.0)
    tables = terrain.sun_tables(g, lat=45.0, dx=30.0, dy=30.0)
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

    for search in (10, 32):
        for names in PRODUCTS:
            n = 16 if names == ("horizon",) else len(names)
            buf = torch.empty((n, a.nrow, a.ncol), dtype=torch.float32, device=dev)
            rec = timed(lambda: terrain.solar(stack, search, names, tables, dx=30.0, dy=30.0, out=buf, out_dtype=torch.float32))
            rec.update(kind="solar", products=list(names), search=search, entries=int(tables.start[-1]),
                       check=float(torch.nan_to_num(buf[0]).double().mean().item()))
            out.append(rec)
            del buf
        forms = torch.empty((a.nrow, a.ncol), dtype=torch.int16, device=dev)
        rec = timed(lambda: terrain.geomorphon(stack, search, 1.0, dx=30.0, dy=30.0, out=forms))
        rec.update(kind="geomorphon", search=search, check=float((forms == 6).double().mean().item()))
        out.append(rec)
        del forms
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solar_speed.txt"))
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
    recs = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
    n_ent = max(d.get("entries", 0) for d in recs)
    lines = ["Solar call on a resident float32 elevation plane: %d x %d cells, float32 outputs; median of %d passes after a warm-up "
             "[min .. max], device events around the call.  Default sun tables (latitude 45, 4 days, 30-minute steps: %d entries).  "
             "dx = dy = 30.  Geomorphons (8 rays) at the same search length for comparison." % (a.nrow, a.ncol, a.repeats, n_ent)]
    for d in recs:
        span = "%9.3f ms [%0.3f .. %0.3f]" % (d["ms"], d["lo"], d["hi"])
        what = "solar %s, search %d" % (" + ".join(d["products"]), d["search"]) if d["kind"] == "solar" else "geomorphons, search %d" % d["search"]
        lines.append("%-46s %s   %6.2f G cells / s" % (what + ":", span, ncell / (d["ms"] * 1e-3) / 1e9))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
