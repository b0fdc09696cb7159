"""Speed of the TPS standard-error path (csrc/tps_se.hip): host build of Q = -M^-1 per spline, and the quadratic-form
kernel on a window / on all tiles of a tiled surface.  FP64 rate counts 2 (n+3)^2 flop per cell (z'Qz), against the
78.6 TF/s FP64 peak of the MI355X.  One JSON line per case.

    python tools/se_speed.py [--reps 3]

Wall times are HIP-event times around the library calls; run it under `rocprofv3 --kernel-trace --stats` for the
kernel alone (tps_se_kernel).  The tiled cases include their fits, Q builds and the mosaic."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import machisplin_amd as m  # noqa: E402
from machisplin_amd import synth  # noqa: E402

PEAK_TF = 78.6


def events_ms(fn, reps):
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def tile_flop(g, xy, tile_edge):
    """sum over the tiles of keep cells x 2 (n_tile + 3)^2, n_tile the distinct stations of the tile's fit box"""
    nRx, nCx, fit_win, keep_win = m.tiles.step3_tile_windows(g, tile_edge)
    rows, cols = m.tiles.cells_from_xy(g, xy)
    total, ns = 0.0, []
    for f, k in zip(fit_win, keep_win):
        sel = (rows >= f[0]) & (rows < f[1]) & (cols >= f[2]) & (cols < f[3])
        n = int(np.unique(xy[sel], axis=0).shape[0])
        if n < 10:
            continue
        ns.append(n)
        total += float((k[1] - k[0]) * (k[3] - k[2])) * 2.0 * (n + 3) ** 2
    return total, ns, nRx * nCx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    m.init()
    # one spline, n = 224, on a 1 500 x 1 500 window
    g = synth.grid(1500, 1500)
    xy, _, _, uv = synth.stations(g, 224, 5)
    y = synth.tps_residual(uv, 5)
    fit = m.Tps(xy, y)
    t0 = time.perf_counter()
    s2 = fit.sigma2                                   # builds Q on the host and uploads it
    build_ms = (time.perf_counter() - t0) * 1e3
    out = torch.empty((g.nrow, g.ncol), dtype=torch.float64, device="cuda")
    m.interpolate_se(g, fit, out=out)
    ms = events_ms(lambda: m.interpolate_se(g, fit, out=out), args.reps)
    flop = g.nrow * g.ncol * 2.0 * (fit.n + 3) ** 2
    print(json.dumps({"case": "one spline n=224, 1500^2", "n": fit.n, "sigma2": s2, "q_build_ms": round(build_ms, 2),
                      "ms": round(ms, 3), "tflops": round(flop / ms / 1e9, 2), "pct_peak": round(100 * flop / ms / 1e9 / PEAK_TF, 1)}),
          flush=True)
    # Q-build time by spline size (host, one spline, all the process's threads)
    for n in (224, 750, 2000):
        gq = synth.grid(3000, 3000)
        xq, _, _, uq = synth.stations(gq, n, 7)
        f = m.Tps(xq, synth.tps_residual(uq, 7), lambda_=1e-3)
        t0 = time.perf_counter()
        f.sigma2
        print(json.dumps({"case": f"Q build n={n}", "q_build_ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
    # tiled surfaces: cfg3-sized (5 000 stations, 10 000^2, 49 tiles) and four tiles of 1 530 stations on 2 000^2
    for label, nrow, nst, edge in (("cfg3 tiled 10000^2, 5000 stations", 10000, 5000, 1500),
                                   ("4 tiles 2000^2, 1530 stations", 2000, 1530, 1000)):
        g = synth.grid(nrow, nrow)
        xy, _, _, uv = synth.stations(g, nst, 3)
        resid = synth.tps_residual(uv, 3)
        out = torch.empty((nrow, nrow), dtype=torch.float64, device="cuda")
        m.tps_residual_surface_se(g, xy, resid, tile_edge=edge, out=out)
        ms = events_ms(lambda: m.tps_residual_surface_se(g, xy, resid, tile_edge=edge, out=out), args.reps)
        flop, ns, nt = tile_flop(g, xy, edge)
        print(json.dumps({"case": label, "tiles": nt, "n_min": min(ns), "n_max": max(ns), "gflop": round(flop / 1e9, 1),
                          "call_ms": round(ms, 2), "tflops_call": round(flop / ms / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
