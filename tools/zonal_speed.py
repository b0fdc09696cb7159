#!/usr/bin/env python
"""Time of the zonal call (machisplin_amd.zonal -> mhs_zonal_dev, csrc/zonal.hip) on a RESIDENT 10 000 x 10 000 float32 plane
(the synthetic relief of tools/hydro_speed.py), in ONE process, on five zone planes:

  (a) the `id` plane (minus 1) of the coastline-like mask of tools/proximity_speed.py: the 8-connected patches of the cells of the
      `alt` stand-in that are at most its median (left out where the fixture is missing);
  (b) the `label` plane of the random mask at density 0.59: cell-number labels, one giant zone and many small ones;
  (c) the outlet labels of flowpath on the synthetic relief: drainage basins, cell-number labels;
  (d) a blocky "land cover" plane: 1 000 classes in blocks of 50 x 50 cells;
  (e) every cell its own zone.

    python tools/zonal_speed.py [--repeats 5] [--n 10000] [--out profiles/zonal_speed.txt]

Two calls per zone plane: `mean` as a table only, and all statistics as a table with three planes (mean, minus_mean, dev; float32).
The table is the present form for the cell-number labels (b, c, e) and dense otherwise; n_zones is given, the quantum is measured,
the info is read back.  A figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the call; a measurement whose
warm-up pass alone takes more than two seconds is not repeated, and that pass is its figure.
Bytes the call MUST move by the layout, for n cells: the range pass and the accumulate pass each read the layer and the zone plane
(8 n each); the planes pass reads them again and writes three float32 planes (8 n + 12 n); the tables come on top and are not
counted.  So 16 n for the table-only call, 36 n with the planes; the share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).

The accumulate path alone, with and without the multi-tile strip: the library entry with n_zones and quantum given, `mean` as a
dense table and no info, so that the range pass is skipped -- a memset, the accumulate kernel, the finalise kernel and the one
synchronise that reads the device flag; once as it is and once with MHS_ZONAL_NO_STRIP.  The difference of the two is the
accumulate kernel's.

For scale only, in the same run: the patches call with five products on mask (b).  (torch's ``index_add_`` of float64 over the same
zones was to be the other scale: it is left out, because on the one machine it was tried on the call had not returned after two
minutes at 2 000 x 2 000 cells.)  There is no earlier route in this library, so there is no pass mark."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.3e12
THREE = ("mean", "minus_mean", "dev")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zonal_speed.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import _lib, synth, terrain
    from machisplin_amd.flowpath import flowpath
    from machisplin_amd.patches import patches
    from machisplin_amd.zonal import zonal, TABLE_STATS
    from hydro_speed import alt_stand_in
    mhs.init()
    n = a.n
    cells = n * n
    dev = torch.device("cuda", torch.cuda.current_device())
    g = synth.grid(n, n)
    gen = torch.Generator(device=dev).manual_seed(5)
    relief, _ = synth.covariates(g, 1, 5, dtype="f32")
    relief[0] += 6.0 * torch.rand((n, n), device=dev, generator=gen) - 3.0
    st = mhs.RasterStack(g, relief[:1], float("nan"))

    def timed(fn, what=""):
        """median, min, max over the timed passes; a measurement whose warm-up pass alone takes more than two seconds is not
        repeated: that pass is its figure (min = max)"""
        print("timing " + what, file=sys.stderr, flush=True)
        ms, last = [], None
        for _ in range(a.repeats + 1):                                     # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            if len(ms) == 1 and ms[0] > 2000.0:
                return ms[0], ms[0], ms[0], last
        ms = ms[1:]
        return statistics.median(ms), min(ms), max(ms), last

    # the zone planes: (name, int32 plane, n_zones, table form)
    planes = []
    print("making the zone planes", file=sys.stderr, flush=True)
    alt = alt_stand_in(n, n)
    if alt is not None:
        ast = mhs.RasterStack(g, torch.from_numpy(alt)[None], float("nan"))
        ids, info = patches(ast, 0, "le", float(np.nanmedian(alt)), 8, "id")
        planes.append(("(a) patch ids of the coastline-like mask", ids - 1, info["n_patches"], "dense"))
        del ast, ids
    u = torch.rand((1, n, n), device=dev, generator=gen, dtype=torch.float32)
    ust = mhs.RasterStack(g, u, float("nan"))
    label, _ = patches(ust, 0, "lt", 0.59, 8, "label")
    planes.append(("(b) patch labels, random mask 0.59", label, cells, "present"))
    hp, _ = terrain.hydro(st, products=("flowdir",), dx=30.0, dy=30.0)
    basin, _ = flowpath(hp["flowdir"], st, 0, "outlet", None, "index")
    planes.append(("(c) flowpath outlet labels", basin, cells, "present"))
    del hp, label, basin
    r = torch.arange(n, device=dev)
    blocks = (r[:, None] // 50) * ((n + 49) // 50) + r[None, :] // 50
    planes.append(("(d) 1 000 classes in 50 x 50 blocks", ((blocks * 7919) % 1000).to(torch.int32), 1000, "dense"))
    planes.append(("(e) every cell its own zone", torch.arange(cells, device=dev, dtype=torch.int32).reshape(n, n), cells, "present"))
    del blocks
    print("the zone planes are made", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(text):
        """a result line: printed and written at once, so that a run that is cut short leaves what it had"""
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    lines = ["Zonal statistics on a resident %d x %d float32 plane (synthetic relief); median of %d passes after a warm-up [min .. max], device "
             "events around the call; ONE run in one process.  n_zones given, quantum measured, info read back.  Bytes = what the call must "
             "move by the layout (16 per cell for a table, 36 with three float32 planes; see the tool's text); share of 6.3 TB/s (achievable HBM "
             "rate, 8 TB/s peak).  Accumulate path: the library entry with n_zones and quantum given and no info (memset, accumulate, finalise, "
             "the flag read back), with the strip of 8 tiles and with MHS_ZONAL_NO_STRIP." % (n, n, a.repeats)]
    say(lines[0])
    cg = g.c_struct()
    src = st.planes
    cs = _lib.Stack(src.data_ptr(), 1, _lib.F32, src.stride(0), src.stride(1), float("nan"))
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, zones, nz, form in planes:
        zones = zones.contiguous()
        for what, per_cell, kw in (("mean, table only", 16, dict(stats=("mean",), planes=())),
                                   ("all statistics + three planes", 36, dict(stats=TABLE_STATS, planes=THREE, out_dtype=torch.float32))):
            med, lo, hi, (_, _, info) = timed(lambda: zonal(st, zones, 0, n_zones=nz, table=form, **kw), name + " " + what)
            tbs = per_cell * cells / (med * 1e-3) / 1e12
            say("%-42s %-30s %9.3f ms [%0.3f .. %0.3f]   %5.2f GB -> %5.3f TB/s = %4.1f %% of the achievable rate   %d zones present, "
                         "quantum 2^%d, %d inexact, scratch %.0f MB" % (name, what, med, lo, hi, per_cell * cells / 1e9, tbs, 100.0 * tbs * 1e12 / HBM,
                                                                       info["n_present"], int(np.log2(info["quantum"])), info["n_inexact"],
                                                                       info["scratch_bytes"] / 1e6))
        quantum = info["quantum"]
        mean = torch.empty(nz, dtype=torch.float64, device=dev)
        tab = _lib.ZonalTable(nz, None, None, None, mean.data_ptr())

        def entry(flags):
            _lib.check(_lib.lib().mhs_zonal_dev(C.byref(cg), C.byref(cs), 0, zones.data_ptr(), zones.stride(0), nz, quantum, flags, C.byref(tab), None,
                                                stream, None))
        with_strip, without = timed(lambda: entry(0), "accumulate path"), timed(lambda: entry(1), "accumulate path, no strip")
        say("    accumulate path (dense table): strip %9.3f ms [%0.3f .. %0.3f]   no strip %9.3f ms [%0.3f .. %0.3f]" % (with_strip[:3] + without[:3]))
        del mean
    med, lo, hi, _ = timed(lambda: patches(ust, 0, "lt", 0.59, 8, ("label", "id", "size", "edge", "keep"), min_size=100), "patches")
    say("For scale only: patches with five products on the random mask 0.59: %.3f ms [%0.3f .. %0.3f]." % (med, lo, hi))
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
