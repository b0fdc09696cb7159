#!/usr/bin/env python
"""Time of the three calls of machisplin_amd.classes (csrc/classes.hip) on a RESIDENT 10 000 x 10 000 int16 land-cover stand-in with
K = 16 classes, in ONE process, on two planes:

  blobs     the synthetic relief of tools/hydro_speed.py cut into 16 classes at equal steps of elevation (torch.bucketize on the
            device: np.digitize of 10^8 cells, without the trip to the host): coherent land cover, long runs;
  speckle   a random class in every cell: every run has length 1.

    python tools/classes_speed.py [--repeats 5] [--n 10000] [--only aggregate] [--out profiles/classes_speed.txt]

  aggregate  onto 400 x 400 (25 x 25 source cells to a target cell): `mode` alone, and `mode` with `frac` of all 16 classes.  Twice:
             the Python call (which asks for the info, so the census pass over the source runs too and the stream is
             synchronised), and the library entry with the classes given and no info -- class_aggregate_kernel alone, which only
             enqueues.  Bytes the kernel MUST move by the layout: the int16 source once (2 bytes a cell; the target planes are
             0.0003 of that and not counted); the share is of 6.3 TB/s, the achievable HBM rate (8 TB/s peak).
  crosstab   `counts` and `mode` as a table over the 1 000 blocks of 50 x 50 cells of tools/zonal_speed.py, and over the outlet
             labels of flowpath on the relief, renumbered 0 .. B - 1 (by torch.unique: the basins touch one another, so `patches`,
             which labels the connected pieces of a MASK, would merge them; its `id` renumbers labels of separate patches).  The
             Python call, and the entry with classes and n_zones given and no info (memset, class_zone_kernel, finish, the flag
             read back).
  focal      `frac` of 3 of the classes at R = 17 and R = 170, square, float32.

The one other route to FRACTIONS at the parent commit, timed in the same run: K calls of resample.resample(indicator, geom, "mean"),
and K calls of zonal.zonal(indicator, zones, stats=("mean",)), each with its indicator made by torch.  The ratio is reported
whichever way it falls.  A figure is the median of ``--repeats`` timed passes after one warm-up pass, device events around the
call.  Nothing is gated: mode, variety and simpson have no other route."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.3e12
K = 16
CODES = [11, 21, 22, 23, 24, 31, 41, 42, 43, 52, 71, 81, 82, 90, 95, 12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the plane")
    ap.add_argument("--only", default=None, choices=["aggregate", "crosstab", "focal"], help="one call only (a kernel trace of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_speed.txt"))
    a = ap.parse_args()
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import _lib, classes, synth, terrain
    from machisplin_amd.flowpath import flowpath
    from machisplin_amd.resample import resample
    from machisplin_amd.zonal import zonal
    mhs.init()
    n = a.n
    cells = n * n
    dev = torch.device("cuda", torch.cuda.current_device())
    g = synth.grid(n, n)
    gen = torch.Generator(device=dev).manual_seed(5)
    relief, _ = synth.covariates(g, 1, 5, dtype="f32")
    relief[0] += 6.0 * torch.rand((n, n), device=dev, generator=gen) - 3.0
    codes = torch.tensor(sorted(CODES), device=dev, dtype=torch.int16)
    lo, hi = float(relief[0].min()), float(relief[0].max())
    edges = torch.linspace(lo, hi, K + 1, device=dev)[1:-1].contiguous()
    blobs = codes[torch.bucketize(relief[0].contiguous(), edges)]
    speckle = codes[torch.randint(0, K, (n, n), device=dev, generator=gen)]
    covers = {"blobs": mhs.RasterStack(g, blobs[None], -32768.0), "speckle": mhs.RasterStack(g, speckle[None], -32768.0)}
    run_len = {name: cells / float((st.planes[0][:, 1:] != st.planes[0][:, :-1]).sum() + n) for name, st in covers.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    cl = (C.c_int32 * K)(*sorted(CODES))

    def timed(fn, what=""):
        print("timing " + what, file=sys.stderr, flush=True)
        ms, last = [], None
        for _ in range(a.repeats + 1):                                     # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = ms[1:]
        return statistics.median(ms), min(ms), max(ms), last

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(text):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say("Categorical layers on a resident %d x %d int16 plane with K = %d classes; median of %d passes after a warm-up [min .. max], device "
        "events around the call; ONE run in one process.  blobs: the synthetic relief in %d steps of elevation (mean run %.1f cells); speckle: a "
        "random class per cell (mean run %.2f cells).  'call' = the Python call (census pass and info included); 'entry' = the library entry "
        "with the classes given and no info." % (n, n, K, a.repeats, K, run_len["blobs"], run_len["speckle"]))

    def stack_struct(st):
        p = st.planes
        return _lib.Stack(p.data_ptr(), 1, _lib.I16, p.stride(0), p.stride(1), st.nodata)

    # ---- aggregate
    if a.only in (None, "aggregate"):
        T = mhs.Geometry(g.xmin, g.ymax, g.xres * 25, g.yres * 25, n // 25, n // 25)
        sg, tg = g.c_struct(), T.c_struct()
        for name, st in covers.items():
            cs = stack_struct(st)
            mode = torch.empty((T.nrow, T.ncol), dtype=torch.int32, device=dev)
            frac = torch.empty((K, T.nrow, T.ncol), dtype=torch.float32, device=dev)
            for what, products in (("mode", ("mode",)), ("mode + frac of 16", ("mode", "frac"))):
                med, lo_, hi_, _ = timed(lambda: classes.aggregate(st, T, 0, CODES, products, out_dtype=torch.float32), f"aggregate {name} {what}")
                pl = _lib.ClassPlanes(mode.data_ptr(), None, None, None, None, frac.data_ptr() if "frac" in products else None, T.ncol, T.nrow * T.ncol, _lib.F32)

                def entry():
                    _lib.check(_lib.lib().mhs_class_aggregate_dev(C.byref(sg), C.byref(cs), 0, C.byref(tg), cl, K, None, 0, C.byref(pl), stream, None))
                emed, elo, ehi, _ = timed(entry, f"aggregate entry {name} {what}")
                tbs = 2.0 * cells / (emed * 1e-3) / 1e12
                say("aggregate onto %d x %d  %-8s %-18s call %8.3f ms [%0.3f .. %0.3f]   entry %8.3f ms [%0.3f .. %0.3f]   %4.2f GB -> %5.3f TB/s = %4.1f %% "
                    "of the achievable rate" % (T.nrow, T.ncol, name, what, med, lo_, hi_, emed, elo, ehi, 2.0 * cells / 1e9, tbs, 100.0 * tbs * 1e12 / HBM))
            # the other route to fractions: K resample means of torch-made indicators

            def k_resamples():
                z = st.planes[0]
                for code in sorted(CODES):
                    ind = (z == code).to(torch.float32)
                    resample(mhs.RasterStack(g, ind[None]), T, "mean")
            rmed, rlo, rhi, _ = timed(k_resamples, f"16 resample means {name}")
            say("    the other route, %d x resample.resample(torch indicator, 'mean'):  %8.3f ms [%0.3f .. %0.3f]   = %.2f x the call with mode + frac of 16, "
                "%.2f x its entry" % (K, rmed, rlo, rhi, rmed / med, rmed / emed))
    # ---- crosstab
    if a.only in (None, "crosstab"):
        r = torch.arange(n, device=dev)
        blocks = (((r[:, None] // 50) * ((n + 49) // 50) + r[None, :] // 50) * 7919 % 1000).to(torch.int32).contiguous()
        st_rel = mhs.RasterStack(g, relief[:1], float("nan"))
        hp, _ = terrain.hydro(st_rel, products=("flowdir",), dx=30.0, dy=30.0)
        basin, _ = flowpath(hp["flowdir"], st_rel, 0, "outlet", None, "index")
        uniq, inverse = torch.unique(basin, return_inverse=True)
        shift = 1 if int(uniq[0]) < 0 else 0
        basins = (inverse - shift).to(torch.int32).contiguous()
        n_basins = int(uniq.numel()) - shift
        del hp, basin, uniq, inverse, st_rel
        cg = g.c_struct()
        for zname, zones, nz in (("1 000 blocks of 50 x 50", blocks, 1000), ("%d flowpath basins" % n_basins, basins, n_basins)):
            for name, st in covers.items():
                cs = stack_struct(st)
                med, lo_, hi_, (_, _, info) = timed(lambda: classes.crosstab(st, zones, 0, CODES, nz, ("counts", "mode")), f"crosstab {zname} {name}")
                counts = torch.empty((nz, K), dtype=torch.int32, device=dev)
                mode = torch.empty(nz, dtype=torch.int32, device=dev)
                tab = _lib.ClassTable(nz, counts.data_ptr(), None, None, None, mode.data_ptr())

                def entry():
                    _lib.check(_lib.lib().mhs_class_crosstab_dev(C.byref(cg), C.byref(cs), 0, zones.data_ptr(), zones.stride(0), nz, cl, K, None, 0, C.byref(tab),
                                                                 None, stream, None))
                emed, elo, ehi, _ = timed(entry, f"crosstab entry {zname} {name}")
                tbs = 6.0 * cells / (emed * 1e-3) / 1e12
                say("crosstab over %-26s %-8s counts + mode   call %8.3f ms [%0.3f .. %0.3f]   entry %8.3f ms [%0.3f .. %0.3f]   %4.2f GB (layer + zones) -> "
                    "%5.3f TB/s = %4.1f %% of the achievable rate   scratch %.1f MB" % (zname, name, med, lo_, hi_, emed, elo, ehi, 6.0 * cells / 1e9, tbs,
                                                                                       100.0 * tbs * 1e12 / HBM, info["scratch_bytes"] / 1e6))

                def k_zonals():
                    z = st.planes[0]
                    for code in sorted(CODES):
                        ind = (z == code).to(torch.float32)
                        zonal(mhs.RasterStack(g, ind[None]), zones, 0, ("mean",), n_zones=nz, quantum=1.0)
                zmed, zlo, zhi, _ = timed(k_zonals, f"16 zonal means {zname} {name}")
                say("    the other route, %d x zonal.zonal(torch indicator, 'mean'):  %8.3f ms [%0.3f .. %0.3f]   = %.2f x the call, %.2f x its entry"
                    % (K, zmed, zlo, zhi, zmed / med, zmed / emed))
    # ---- focal
    if a.only in (None, "focal"):
        three = sorted(CODES)[4:7]
        for R in (17, 170):
            for name, st in covers.items():
                med, lo_, hi_, _ = timed(lambda: classes.focal(st, R, 0, three, ("frac",), out_dtype=torch.float32), f"focal R {R} {name}")
                say("focal frac of 3 classes, R = %-3d  %-8s %8.3f ms [%0.3f .. %0.3f]   (%.3f ms per class)" % (R, name, med, lo_, hi_, med / 3))
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
