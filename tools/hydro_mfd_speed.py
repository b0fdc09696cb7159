#!/usr/bin/env python
"""Time of the multiple-flow-direction hydrology call (terrain.hydro_mfd -> mhs_hydro_mfd_dev, csrc/hydro.hip) on a RESIDENT
elevation plane of 10 000 x 10 000 cells (float32), all three products (filled, flowacc, twi; float32 outputs), at the
exponents 1 and 1.1, beside the D8 call (terrain.hydro, all four products) on the same plane IN THE SAME RUN -- the only
meaningful comparison.  The planes are those of tools/hydro_speed.py: the synthetic relief with pits and the mirrored `alt`
stand-in of the bundled overviews.

    python tools/hydro_mfd_speed.py [--repeats 5] [--nrow 10000 --ncol 10000] [--out profiles/hydro_mfd_speed.txt]

Every figure is the median of ``--repeats`` timed calls after one warm-up call, on one MI355X: the whole call by device
events around it, and per phase (fill, flat distance, accumulation) the host wall-clock time the library reports in
mhs_hydro_info, the passes, and the share of tiles that were dirty per pass = tile solves / (passes x tiles).  The MFD
accumulation's time includes its shares kernel (the only place pow is called) and the zeroing of the share planes.  The GPU
part runs in a child process of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hydro_speed import PHASES, alt_stand_in          # noqa: E402  (the same planes)

ROUTES = (("D8", None), ("MFD, exponent 1", 1.0), ("MFD, exponent 1.1", 1.1))


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
        stack = mhs.RasterStack(g, z[None], float("nan"))
        for route, x in ROUTES:
            recs = []
            for rep in range(a.repeats + 1):                                # the first is the warm-up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if x is None:
                    res, info = terrain.hydro(stack, products=terrain.HYDRO, dx=30.0, dy=30.0, out_dtype=torch.float32, max_passes=a.max_passes)
                else:
                    res, info = terrain.hydro_mfd(stack, products=terrain.HYDRO_MFD, exponent=x, dx=30.0, dy=30.0, out_dtype=torch.float32,
                                                  max_passes=a.max_passes)
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
            rec.update(plane=name, route=route, check=check)
            out.append(rec)
            print("DONE " + json.dumps(rec), flush=True)
        del stack
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--max-passes", type=int, default=0, help="the cap on the passes of a phase (0 = the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hydro_mfd_speed.txt"))
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
    lines = ["Hydrology calls on a resident float32 elevation plane: %d x %d cells, dx = dy = 30; D8 (filled, flowdir, flowacc, twi) and "
             "multiple flow direction (filled, flowacc, twi) in the same run, float32 outputs; median of %d calls after a warm-up "
             "[min .. max] on one MI355X.  Whole call: device events around it; phases: host wall clock (one stream synchronisation per "
             "pass; the MFD accumulation includes its shares kernel).  dirty = tile solves / (passes x tiles)." % (a.nrow, a.ncol, a.repeats)]
    for d in json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:]):
        lines.append("%s, %s: %9.1f ms [%0.1f .. %0.1f] = %6.1f M cells / s; %d valid cells, %d raised, %d sinks, %d tiles"
                     % (d["plane"], d["route"], d["ms"]["med"], d["ms"]["lo"], d["ms"]["hi"], d["n_valid"] / (d["ms"]["med"] * 1e-3) / 1e6,
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
