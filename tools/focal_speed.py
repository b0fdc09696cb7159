#!/usr/bin/env python
"""Time of the window statistics at any radius (machisplin_amd.focal.focal -> mhs_focal_dev, csrc/focal.hip) on a RESIDENT
10 000 x 10 000 float32 plane, float32 outputs:

  square  mean, and mean + sd + min + max, at R = 17, 45, 170 and 700 -- the claim to check: the time does not grow with R;
          three radii (17, 170, 700) in one call against the three calls;
  circle  minus_mean at R = 17, 45 and 170 -- O(R) per cell;
  and, in the same run, the one earlier route, terrain.relief minus_mean at R = 17 and R = 45 (its limit), and for scale
  torch.nn.functional.avg_pool2d of the same plane with a 35 x 35 kernel, stride 1.

    python tools/focal_speed.py [--repeats 5] [--n 10000] [--out profiles/focal_speed.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/focal_speed.py --device-part --trace      (which kernel dominates)

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the PYTHON call (the
events also bracket the ctypes marshalling, tens of microseconds).  Bytes = what the kernels of csrc/focal.hip move per cell by
their layout, every element counted once per kernel that reads or writes it: the row prefixes 4 + 20, per radius of a square
window 40 + 24 (the column blocks) and 52 + 4 per output plane (the statistics), with min / max 4 + 32 once and 32 + 16, 32 + 32,
32 per radius; a circle reads 2 x 20 bytes per window row and cell, nearly all of it from cache, so its share means little.  The
share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).  Nothing is gated: beyond R = 45 there is no earlier route.  The GPU
part runs in a child process of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
MINMAX = ("min", "max", "range", "above_min", "below_max")


def bytes_per_cell(shape, names, radii):
    """by the layout of csrc/focal.hip; see the module's text"""
    mm = any(k in MINMAX for k in names)
    b = 24 + (36 if mm else 0)
    for R in radii:
        if shape == "square":
            b += 64 + 52 + 4 * len(names) + (176 if mm else 0)
        else:
            b += 40 * (2 * R + 1) + 4 + 4 * len(names)
    return b


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import focal, terrain
    mhs.init()
    n = a.n
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(5)
    g = mhs.Geometry(500000.0, 4100000.0, 30.0, 30.0, n, n)
    plane = 2000.0 + 300.0 * torch.randn((1, n, n), device=dev, generator=gen, dtype=torch.float32)
    plane[0, n // 3:n // 3 + 40, n // 2:n // 2 + 70] = float("nan")
    stack = mhs.RasterStack(g, plane, -32768.0)
    out = []

    def timed(call, repeats=a.repeats):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        run()
        ms = [run() for _ in range(repeats)]
        return {"ms": statistics.median(ms), "lo": min(ms), "hi": max(ms)}

    def case(name, shape, names, radii, repeats=a.repeats):
        buf = torch.empty((len(names) * len(radii), n, n), dtype=torch.float32, device=dev)
        rec = timed(lambda: focal.focal(stack, list(radii), names, shape=shape, offset=2000.0, out_dtype=torch.float32, out=buf), repeats)
        rec.update(name=name, bytes=bytes_per_cell(shape, names, radii) * n * n, valid=float((~torch.isnan(buf[0, ::97, ::89])).double().mean()))
        out.append(rec)
        del buf

    if a.trace:                                                        # one case, twice: for a kernel trace
        case("trace", "square", ("mean", "sd", "min", "max"), (170,), repeats=1)
        print("DEVICE " + json.dumps(out))
        return
    for R in (17, 45, 170, 700):
        case("square mean, R = %d" % R, "square", ("mean",), (R,))
    for R in (17, 45, 170, 700):
        case("square mean + sd + min + max, R = %d" % R, "square", ("mean", "sd", "min", "max"), (R,))
    case("square mean + sd, R = 17, 170, 700 in ONE call", "square", ("mean", "sd"), (17, 170, 700))
    for R in (17, 170, 700):
        case("    square mean + sd, R = %d alone" % R, "square", ("mean", "sd"), (R,))
    for R in (17, 45, 170):
        case("circle minus_mean, R = %d" % R, "circle", ("minus_mean",), (R,), repeats=min(a.repeats, 3 if R > 45 else a.repeats))
    buf = torch.empty((1, n, n), dtype=torch.float32, device=dev)
    for R in (17, 45):
        rec = timed(lambda: terrain.relief(stack, R, ("minus_mean",), out_dtype=torch.float32, out=buf))
        rec.update(name="    terrain.relief minus_mean, R = %d (the earlier route, circle in LDS)" % R, bytes=8 * n * n, valid=float((~torch.isnan(buf[0, ::97, ::89])).double().mean()))
        out.append(rec)
    rec = timed(lambda: torch.nn.functional.avg_pool2d(plane, 35, stride=1, padding=17))
    rec.update(name="    torch avg_pool2d 35 x 35, stride 1 (for scale)", bytes=8 * n * n, valid=1.0)
    out.append(rec)
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace", action="store_true", help="with --device-part: one case only, for a kernel trace")
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
    lines = ["Window statistics of a resident %d x %d float32 plane, float32 outputs; median of %d passes after a warm-up [min .. max], device events "
             "around the Python call (its marshalling, tens of microseconds, included).  Bytes = what the kernels move by their layout (tools/focal_speed.py); "
             "share of 6.3 TB/s (achievable HBM rate, 8 TB/s peak).  valid = share of a sample of the first output plane that is not NA." % (a.n, a.n, a.repeats)]
    for d in recs:
        tbs = d["bytes"] / (d["ms"] * 1e-3) / 1e12
        lines.append("%-76s %10.3f ms [%0.3f .. %0.3f]   %7.3f GB -> %6.3f TB/s = %5.1f %% of the achievable rate   valid %.3f" %
                     (d["name"] + ":", d["ms"], d["lo"], d["hi"], d["bytes"] / 1e9, tbs, 100.0 * tbs * 1e12 / HBM, d["valid"]))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
