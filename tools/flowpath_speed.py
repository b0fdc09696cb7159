#!/usr/bin/env python
"""Time of the flow-path call (flowpath.flowpath -> mhs_flowpath_dev, csrc/flowpath.hip) on a RESIDENT elevation plane of
10 000 x 10 000 float32 cells, on the two planes of tools/hydro_speed.py: the synthetic relief with pits and the `alt` stand-in
of the bundled overviews.  terrain.hydro runs first, untimed, and makes the D8 directions and the accumulation.  Timed:

  * index alone, and index + dist + drop, to the first cell with flowacc >= 1 000 on the cell's own path, the root where the
    path meets none (what covariates() makes "hand" and "flowdist_stream" from);
  * the outlet labels (index, no targets);
  * each of them with and without the local phase (the in-tile doubling in LDS), with the global rounds of both routes;
  * for scale, the Euclidean ("above_stream", 1 000) of proximity -- dist and value to the nearest stream cell -- in the same run.

    python tools/flowpath_speed.py [--repeats 5] [--nrow 10000 --ncol 10000] [--out profiles/flowpath_speed.txt]

Every figure is the median of ``--repeats`` timed calls after one warm-up call, on one MI355X, by device events around the
whole call (which synchronises the stream once per doubling round, so the events see what a caller sees).  Outputs float32.
There is no earlier route and the reference has none: no pass mark.  The GPU part runs in a child process of its own under a
time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hydro_speed import alt_stand_in  # noqa: E402

STREAM_A = 1000.0
CALLS = (("index to the first stream cell", dict(where="ge", threshold=STREAM_A, products=("index",))),
         ("index + dist + drop to it", dict(where="ge", threshold=STREAM_A, products=("index", "dist", "drop"), value_layer=1)),
         ("outlet labels (index)", dict(where="outlet", products=("index",))))


def device_part(a):
    import torch
    import machisplin_amd as mhs
    from machisplin_amd import synth, terrain
    from machisplin_amd.flowpath import flowpath
    from machisplin_amd.proximity import proximity
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

    def timed(fn):
        ms, last = [], None
        for rep in range(a.repeats + 1):                                    # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = ms[1:]
        return {"med": statistics.median(ms), "lo": min(ms), "hi": max(ms)}, last

    out = []
    for name, z in planes:
        hp, _ = terrain.hydro(mhs.RasterStack(g, z[None], float("nan")), products=("flowdir", "flowacc"), dx=30.0, dy=30.0, out_dtype=torch.float32)
        pair = mhs.RasterStack(g, torch.stack([hp["flowacc"], z]), float("nan"))
        flowdir = hp["flowdir"]
        del hp
        rec = {"plane": name, "calls": []}
        for what, kw in CALLS:
            for local in (True, False):
                t, (res, info) = timed(lambda: flowpath(flowdir, pair, 0, root_is_target=True, local=local, out_dtype=torch.float32, dx=30.0, dy=30.0, **kw))
                first = res if isinstance(res, torch.Tensor) else res["index"]
                rec["calls"].append({"what": what, "local": local, "ms": t, "check": int(first.to(torch.int64).sum().item()),
                                     **{k: info[k] for k in ("n_valid", "n_targets", "n_roots", "max_steps", "rounds", "scratch_bytes")}})
                del res, first
        t, (res, info) = timed(lambda: proximity(pair, 0, "ge", STREAM_A, ("dist", "value"), value_layer=1, unit=30.0, out_dtype=torch.float32))
        rec["euclid"] = {"ms": t, "n_features": info["n_features"]}
        del res, pair, flowdir
        out.append(rec)
        print("DONE " + json.dumps(rec), flush=True)
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowpath_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats), "--nrow", str(a.nrow),
                        "--ncol", str(a.ncol)], capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    lines = ["Flow-path call on a resident plane of %d x %d cells (float32 DEM, D8 directions and accumulation of terrain.hydro, untimed; "
             "dx = dy = 30; float32 outputs); streams: flowacc >= %g, the root where a path meets none.  Median of %d calls after a warm-up "
             "[min .. max] on one MI355X, device events around the whole call (one stream synchronisation per doubling round).  "
             "rounds = global doubling rounds that moved a cell." % (a.nrow, a.ncol, STREAM_A, a.repeats)]
    for d in json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:]):
        c0 = d["calls"][0]
        lines.append("%s: %d valid cells, %d stream cells, %d roots" % (d["plane"], c0["n_valid"], c0["n_targets"], c0["n_roots"]))
        for c in d["calls"]:
            lines.append("    %-32s %-20s %8.1f ms [%0.1f .. %0.1f]  %2d rounds, longest path %s steps, scratch %.0f MB"
                         % (c["what"] + ":", "with the local phase" if c["local"] else "global rounds only", c["ms"]["med"], c["ms"]["lo"], c["ms"]["hi"],
                            c["rounds"], c["max_steps"] if c["max_steps"] >= 0 else "(not carried)", c["scratch_bytes"] / 1e6))
        e = d["euclid"]
        lines.append("    %-32s %-20s %8.1f ms [%0.1f .. %0.1f]  (%d stream cells)"
                     % ("Euclidean dist + value:", "proximity", e["ms"]["med"], e["ms"]["lo"], e["ms"]["hi"], e["n_features"]))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
