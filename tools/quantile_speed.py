#!/usr/bin/env python
"""Time of the quantile call (machisplin_amd.zonal.quantile -> mhs_zonal_quantile_dev, csrc/quantile.hip on csrc/sort_keys.hip) on a
RESIDENT 10 000 x 10 000 float32 plane (the synthetic relief of tools/hydro_speed.py), in ONE process, on the five zone planes of
tools/zonal_speed.py -- (a) patch ids of the coastline-like mask, (b) patch labels of a random mask, (c) flowpath outlet labels,
(d) 1 000 classes in blocks, (e) every cell its own zone -- and (f) the whole layer as one zone.

    python tools/quantile_speed.py [--repeats 5] [--n 10000] [--out profiles/quantile_speed.txt] [--no-trace]

Two calls per zone plane: the median alone as a table, and five probabilities (0.05, 0.25, 0.5, 0.75, 0.95) as a table with the
``frac_below`` plane (float32).  The table is the present form for the cell-number labels (b, c, e) and dense otherwise; n_zones is
given, the quantum measured, the info read back (so the call ends with a synchronise).  A figure is the median of ``--repeats``
timed passes after one warm-up pass, device events around the call; a measurement whose warm-up pass alone takes more than ten
seconds is not repeated, and that pass is its figure.  ``passes_run`` and the scratch are the info's.

The sort phase: unless ``--no-trace``, the tool starts ONE fresh child process of itself under ``rocprofv3 --kernel-trace --stats``
(``--child PLANE``: a warm-up and one median-only call on that zone plane, nothing else) per zone plane and sums the times of the
``sort_*`` kernels and of all kernels from the child's kernel statistics, halved for the two calls.  Counters are not collected.

For scale only, in the same run: ``torch.sort`` of the same int64 keys (made by torch from the zone plane and the quantised
values), and ``zonal`` with ``mean`` as a table on the same zones.  There is no earlier route in this library, so there is no
pass mark."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIVE = (0.05, 0.25, 0.5, 0.75, 0.95)
NAMES = ("a", "b", "c", "d", "e", "f")


def zone_planes(mhs, g, st, n, dev, gen, only=None):
    """(letter, name, int32 plane or None, n_zones, table form); `only`: just that letter"""
    import numpy as np
    import torch
    from machisplin_amd import terrain
    from machisplin_amd.flowpath import flowpath
    from machisplin_amd.patches import patches
    from hydro_speed import alt_stand_in
    cells = n * n
    want = lambda k: only is None or only == k                                 # noqa: E731
    if want("a"):
        alt = alt_stand_in(n, n)
        if alt is not None:
            ast = mhs.RasterStack(g, torch.from_numpy(alt)[None], float("nan"))
            ids, info = patches(ast, 0, "le", float(np.nanmedian(alt)), 8, "id")
            yield "a", "(a) patch ids of the coastline-like mask", (ids - 1).contiguous(), info["n_patches"], "dense"
            del ast, ids
    if want("b"):
        u = torch.rand((1, n, n), device=dev, generator=gen, dtype=torch.float32)
        label, _ = patches(mhs.RasterStack(g, u, float("nan")), 0, "lt", 0.59, 8, "label")
        del u
        yield "b", "(b) patch labels, random mask 0.59", label, cells, "present"
        del label
    if want("c"):
        hp, _ = terrain.hydro(st, products=("flowdir",), dx=30.0, dy=30.0)
        basin, _ = flowpath(hp["flowdir"], st, 0, "outlet", None, "index")
        del hp
        yield "c", "(c) flowpath outlet labels", basin, cells, "present"
        del basin
    if want("d"):
        r = torch.arange(n, device=dev)
        blocks = (r[:, None] // 50) * ((n + 49) // 50) + r[None, :] // 50
        yield "d", "(d) 1 000 classes in 50 x 50 blocks", ((blocks * 7919) % 1000).to(torch.int32), 1000, "dense"
        del blocks
    if want("e"):
        yield "e", "(e) every cell its own zone", torch.arange(cells, device=dev, dtype=torch.int32).reshape(n, n), cells, "present"
    if want("f"):
        yield "f", "(f) the whole layer", None, None, "dense"


def trace_child(letter, n):
    """(sort ms, all kernels ms) of one median-only call on zone plane `letter`, from a child of this tool under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", letter,
               "--n", str(n)]
        pr = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if pr.returncode != 0:
            return None
        sort_ns = all_ns = 0.0
        found = False
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name, total = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
                if name.startswith(("sort_", "quantile_", "zonal_range")) or "mhs::sort_" in name or "mhs::quantile_" in name or "mhs::zonal_range" in name:
                    found = True
                    all_ns += total
                    if "sort_" in name:
                        sort_ns += total
        return (sort_ns / 2e6, all_ns / 2e6) if found else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10000, help="edge of the plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_speed.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", choices=NAMES, default=None, help="internal: a warm-up and one median-only call on that zone plane")
    a = ap.parse_args()
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import synth
    from machisplin_amd.zonal import quantile, zonal
    mhs.init()
    n = a.n
    cells = n * n
    dev = torch.device("cuda", torch.cuda.current_device())
    g = synth.grid(n, n)
    gen = torch.Generator(device=dev).manual_seed(5)
    relief, _ = synth.covariates(g, 1, 5, dtype="f32")
    relief[0] += 6.0 * torch.rand((n, n), device=dev, generator=gen) - 3.0
    st = mhs.RasterStack(g, relief[:1], float("nan"))

    if a.child:
        for _, _, zones, nz, form in zone_planes(mhs, g, st, n, dev, gen, a.child):
            for _ in range(2):
                quantile(st, zones, (0.5,), n_zones=nz, table=form)
            torch.cuda.synchronize()
        return 0

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
            if len(ms) == 1 and ms[0] > 10000.0:
                return ms[0], ms[0], ms[0], last
        ms = ms[1:]
        return statistics.median(ms), min(ms), max(ms), last

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(text):
        """a result line: printed and written at once, so that a run that is cut short leaves what it had"""
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    say("Zonal quantiles on a resident %d x %d float32 plane (synthetic relief); median of %d passes after a warm-up [min .. max], device events "
        "around the call; ONE run in one process.  n_zones given, quantum measured, info read back.  Sort phase: the sort_* kernels of one call, "
        "from a kernel trace of a child process of its own.  For scale only: torch.sort of the same int64 keys, and zonal's mean on the same zones."
        % (n, n, a.repeats))
    for letter, name, zones, nz, form in zone_planes(mhs, g, st, n, dev, gen):
        for what, kw in (("median, table only", dict(probs=(0.5,))),
                         ("five probabilities + frac_below", dict(probs=FIVE, planes=("frac_below",), out_dtype=torch.float32))):
            med, lo, hi, (_, _, info) = timed(lambda: quantile(st, zones, n_zones=nz, table=form, **kw), name + " " + what)
            say("%-42s %-32s %9.3f ms [%0.3f .. %0.3f]   %d passes, %d zones present, %d contributing, scratch %.0f MB = %.2f bytes per cell"
                % (name, what, med, lo, hi, info["passes_run"], info["n_present"], info["n_contributing"], info["scratch_bytes"] / 1e6,
                   info["scratch_bytes"] / cells))
        if not a.no_trace:
            got = trace_child(letter, n)
            say("    sort phase of the median-only call: " + ("%.3f ms of %.3f ms in this feature's kernels" % got if got else "no trace (rocprofv3 failed)"))
        # for scale: torch.sort of the same keys, zonal's mean on the same zones
        q = torch.round(st.planes[0].to(torch.float64) / info["quantum"]).to(torch.int64) + 2 ** 30
        keys = q if zones is None else torch.where(zones >= 0, (zones.to(torch.int64) << 32) | q, torch.full_like(q, int(info["n_zones"]) << 32))
        del q
        keys = keys.reshape(-1)
        med, lo, hi, _ = timed(lambda: torch.sort(keys), name + " torch.sort")
        say("    for scale: torch.sort of the same int64 keys %9.3f ms [%0.3f .. %0.3f]" % (med, lo, hi))
        del keys
        zz = zones if zones is not None else torch.zeros((n, n), dtype=torch.int32, device=dev)
        med, lo, hi, _ = timed(lambda: zonal(st, zz, 0, stats=("mean",), n_zones=nz or 1, table=form), name + " zonal mean")
        say("    for scale: zonal mean, table only           %9.3f ms [%0.3f .. %0.3f]" % (med, lo, hi))
        del zz
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
