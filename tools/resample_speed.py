#!/usr/bin/env python
"""Time of the resample calls (machisplin_amd.resample -> mhs_resample_dev / mhs_extract_points_dev, csrc/resample.hip) on
RESIDENT float32 planes, float32 outputs:

  (a) a 10 000 x 10 000 plane onto 300 x 300 cells with MEAN (a factor of 33.3: footprints of 33 and 34 that vary);
  (b) the reverse, a 300 x 300 plane onto 10 000 x 10 000 cells with BILINEAR and with CUBIC (the staged regime);
  (c) 10 000 x 10 000 onto the same size shifted by 0.37 of a cell, BILINEAR (the staged regime at a ratio of 1);
  (d) 5 000 points extracted from 5 layers of 10 000 x 10 000, bilinear.

    python tools/resample_speed.py [--repeats 5] [--n 10000] [--out profiles/resample_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the call.  Bytes = every
source element once + every output element once; the share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).  Beside
each grid case the same run times what a user has today in torch: ``torch.nn.functional.interpolate(align_corners=False)`` for
(b) and ``avg_pool2d`` on an aligned integer-factor variant of (a) (10 000 -> 400 by 25, no NA handling).  That comparison is
at the same sizes, not the same rule: it gives scale only.  There is no earlier route in this library, so there is no pass
mark.  The GPU part runs in a child process of its own under a time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12


def device_part(a):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import machisplin_amd as mhs
    from machisplin_amd.resample import extract, resample
    mhs.init()
    n, m = a.n, a.small
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(5)
    big_g = mhs.Geometry(1000.0, 5000.0 + 30.0 * n, 30.0, 30.0, n, n)
    small_g = mhs.Geometry(1000.0, 5000.0 + 30.0 * n, 30.0 * n / m, 30.0 * n / m, m, m)
    shift_g = mhs.Geometry(1000.0 + 0.37 * 30.0, 5000.0 + 30.0 * n - 0.37 * 30.0, 30.0, 30.0, n, n)
    big = mhs.RasterStack(big_g, 100.0 * torch.randn((1, n, n), device=dev, generator=gen, dtype=torch.float32), -32768.0)
    small = mhs.RasterStack(small_g, 100.0 * torch.randn((1, m, m), device=dev, generator=gen, dtype=torch.float32), -32768.0)
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

    def case(name, call, nbytes, check):
        rec = timed(call)
        rec.update(name=name, bytes=nbytes, check=float(check()))
        out.append(rec)

    buf_s = torch.empty((1, m, m), dtype=torch.float32, device=dev)
    buf_b = torch.empty((1, n, n), dtype=torch.float32, device=dev)
    case("(a) %d^2 -> %d^2 mean" % (n, m), lambda: resample(big, small_g, "mean", out=buf_s), 4 * (n * n + m * m), lambda: buf_s.double().mean())
    f = 25
    case("    torch avg_pool2d by %d, %d^2 -> %d^2" % (f, n, n // f), lambda: F.avg_pool2d(big.planes[None], f), 4 * (n * n + (n // f) ** 2), lambda: 0.0)
    for method in ("bilinear", "cubic"):
        case("(b) %d^2 -> %d^2 %s" % (m, n, method), lambda: resample(small, big_g, method, out=buf_b), 4 * (n * n + m * m), lambda: torch.nan_to_num(buf_b).double().mean())
    case("    torch interpolate bilinear, %d^2 -> %d^2" % (m, n), lambda: F.interpolate(small.planes[None], size=(n, n), mode="bilinear", align_corners=False),
         4 * (n * n + m * m), lambda: 0.0)
    case("    torch interpolate bicubic, %d^2 -> %d^2" % (m, n), lambda: F.interpolate(small.planes[None], size=(n, n), mode="bicubic", align_corners=False),
         4 * (n * n + m * m), lambda: 0.0)
    case("(c) %d^2 -> %d^2 shifted 0.37 cell, bilinear" % (n, n), lambda: resample(big, shift_g, "bilinear", out=buf_b), 8 * n * n,
         lambda: torch.nan_to_num(buf_b).double().mean())
    del buf_b
    layers = mhs.RasterStack(big_g, 100.0 * torch.randn((5, n, n), device=dev, generator=gen, dtype=torch.float32), -32768.0)
    rng = np.random.default_rng(9)
    xy = np.column_stack([rng.uniform(big_g.xmin, big_g.xmax, 5000), rng.uniform(big_g.ymin, big_g.ymax, 5000)])
    got = {}

    def points():
        got["v"] = extract(layers, xy, "bilinear")
    case("(d) 5000 points x 5 layers, bilinear (with the copies of xy and the values)", points, 0, lambda: np.nanmean(got["v"]))
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the large plane")
    ap.add_argument("--small", type=int, default=300, help="edge of the small plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--n", str(a.n), "--small", str(a.small)],
                       capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    recs = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
    lines = ["Resample calls on resident float32 planes, float32 outputs; median of %d passes after a warm-up [min .. max], device events "
             "around the call.  Bytes = every source element once + every output element once; share of 6.3 TB/s (achievable HBM rate, "
             "8 TB/s peak).  The torch lines are what a user has today at the same sizes, not the same rule: scale only." % a.repeats]
    for d in recs:
        span = "%9.3f ms [%0.3f .. %0.3f]" % (d["ms"], d["lo"], d["hi"])
        rate = ""
        if d["bytes"]:
            tbs = d["bytes"] / (d["ms"] * 1e-3) / 1e12
            rate = "   %6.3f GB -> %6.3f TB/s = %4.1f %% of the achievable rate" % (d["bytes"] / 1e9, tbs, 100.0 * tbs * 1e12 / HBM)
        lines.append("%-78s %s%s" % (d["name"] + ":", span, rate))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
