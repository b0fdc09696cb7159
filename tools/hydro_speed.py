#!/usr/bin/env python
"""Time of the hydrology call (terrain.hydro -> mhs_hydro_dev, csrc/hydro.hip) on a RESIDENT elevation plane of 10 000 x 10 000
cells, float32 and int16, all four products (filled, flowdir, flowacc, twi; float32 outputs):

  * a synthetic relief with pits: layer 0 of synth.covariates (six sinusoids of 0.5 - 6 cycles across the side, 76 .. 4668 m,
    seed 5) plus uniform noise of +- 3 m from torch's generator (seed 5) -- the noise makes small pits everywhere, the
    sinusoids' closed basins make lakes of many tiles;
  * the `alt` stand-in bench.py makes of the reference's bundled overviews (tests/golden/cfg1_extdata.npz: the TWI overview
    rotated by 180 degrees and shifted by half a tile, minus a tenth of the slope, rescaled to 76 .. 4668 m), mirrored into a
    mosaic of the plane's size; NoData cells stay NA.

    python tools/hydro_speed.py [--repeats 5] [--nrow 10000 --ncol 10000] [--out profiles/hydro_speed.txt]

Every figure is the median of ``--repeats`` timed calls after one warm-up call, on one MI355X: the whole call by device
events around it, and per phase (fill, flat distance, accumulation) the host wall-clock time the library reports in
mhs_hydro_info (the host synchronises once per pass, so wall clock is what a caller sees), the passes, and the share of tiles
that were dirty per pass = tile solves / (passes x tiles).  There is no earlier route and the reference has none: no pass
mark.  The GPU part runs in a child process of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

PHASES = ("fill", "flat", "acc")


def alt_stand_in(nrow, ncol):
    """bench.py's stand-in for alt.tif, mirrored to nrow x ncol: float32 with NaN at NoData, or None without the fixture"""
    from machisplin_amd import synth
    fixture = os.path.join(ROOT, "tests", "golden", "cfg1_extdata.npz")
    if not os.path.exists(fixture):
        return None
    d = np.load(fixture)
    twi, slp = d["TWI"].astype(np.float32), d["slope"].astype(np.float32)
    twi[twi == -32768] = np.nan
    slp[slp == -32768] = np.nan
    sub = np.roll(twi[::-1, ::-1], (twi.shape[0] // 2, twi.shape[1] // 2), axis=(0, 1)) - 0.1 * np.roll(slp, twi.shape[1] // 3, axis=1)
    lo, hi = np.nanmin(sub), np.nanmax(sub)
    a_lo, a_hi = synth.COV_RANGES[0]
    sub = (sub - lo) / (hi - lo) * (a_hi - a_lo) + a_lo
    ny, nx = -(-nrow // sub.shape[0]), -(-ncol // sub.shape[1])
    rows = []
    for iy in range(ny):
        t = sub[::-1] if iy & 1 else sub
        rows.append(np.concatenate([t[:, ::-1] if ix & 1 else t for ix in range(nx)], axis=1))
    return np.ascontiguousarray(np.concatenate(rows, axis=0)[:nrow, :ncol])


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import synth, terrain
    mhs.init()
    g = synth.grid(a.nrow, a.ncol)
    dev = torch.device("cuda", torch.cuda.current_device())
    planes = []
    relief, _ = synth.covariates(g, 1, 5, dtype="f32")
    gen = torch.Generator(device=dev).manual_seed(5)
    relief[0] += 6.0 * torch.rand((a.nrow, a.ncol), device=dev, generator=gen) - 3.0
    planes.append(("synthetic relief with pits", relief[0]))
    alt = alt_stand_in(a.nrow, a.ncol)
    if alt is not None:
        planes.append(("alt stand-in of the bundled overviews", torch.from_numpy(alt).to(dev)))
    out = []
    for name, z in planes:
        for dtype in ("f32", "i16"):
            if dtype == "i16":
                p = torch.where(torch.isnan(z), torch.full_like(z, -32768.0), z.round()).to(torch.int16)[None]
            else:
                p = z[None]
            stack = mhs.RasterStack(g, p, -32768.0 if dtype == "i16" else float("nan"))
            recs = []
            for rep in range(a.repeats + 1):                                # the first is the warm-up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res, info = terrain.hydro(stack, products=terrain.HYDRO, dx=30.0, dy=30.0, out_dtype=torch.float32, max_passes=a.max_passes)
                e1.record()
                e1.synchronize()
                info["ms"] = e0.elapsed_time(e1)
                recs.append(info)
                check = float(torch.nan_to_num(res["twi"]).double().mean().item())
                del res
            recs = recs[1:]
            rec = {k: recs[0][k] for k in ("passes_fill", "passes_flat", "passes_acc", "n_valid", "n_raised", "n_sinks", "n_tiles",
                                           "solves_fill", "solves_flat", "solves_acc")}
            for k in ("ms", "ms_fill", "ms_flat", "ms_acc"):
                v = [r[k] for r in recs]
                rec[k] = {"med": statistics.median(v), "lo": min(v), "hi": max(v)}
            rec.update(plane=name, dtype=dtype, check=check)
            out.append(rec)
            print("DONE " + json.dumps(rec), flush=True)
            del stack, p
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--max-passes", type=int, default=0, help="the cap on the passes of a phase (0 = the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hydro_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--nrow", str(a.nrow),
                        "--ncol", str(a.ncol), "--max-passes", str(a.max_passes)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    lines = ["Hydrology call (filled, flowdir, flowacc, twi; float32 outputs) on a resident elevation plane: %d x %d cells, dx = dy = 30; "
             "median of %d calls after a warm-up [min .. max] on one MI355X.  Whole call: device events around it; phases: host wall "
             "clock (one stream synchronisation per pass).  dirty = tile solves / (passes x tiles)." % (a.nrow, a.ncol, a.repeats)]
    label = {"f32": "float32", "i16": "int16"}
    for d in json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:]):
        lines.append("%s, %s plane: %9.1f ms [%0.1f .. %0.1f] = %6.1f M cells / s; %d valid cells, %d raised, %d sinks, %d tiles"
                     % (d["plane"], label[d["dtype"]], d["ms"]["med"], d["ms"]["lo"], d["ms"]["hi"], d["n_valid"] / (d["ms"]["med"] * 1e-3) / 1e6,
                        d["n_valid"], d["n_raised"], d["n_sinks"], d["n_tiles"]))
        for ph, what in zip(PHASES, ("fill", "flat distance", "accumulation")):
            t, n = d["ms_" + ph], d["passes_" + ph]
            lines.append("    %-14s %9.1f ms [%0.1f .. %0.1f]  %5d passes, %5.1f %% of the tiles dirty per pass"
                         % (what + ":", t["med"], t["lo"], t["hi"], n, 100.0 * d["solves_" + ph] / (n * d["n_tiles"])))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
