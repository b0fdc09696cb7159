#!/usr/bin/env python
"""Wall time of the device fit of earth models (mhs_earth_fit_many) at the size of the bundled example: n = 813, p = 7,
default arguments -- one model; a layer's 121 models (11 calls of earth(nfold = 10): each a fit on all its rows and ten
on nine tenths of them) in ONE call; and the same 121 models one call at a time.

    python tools/earth_fit_speed.py [--repeats 5] [--out profiles/earth_fit_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, host work included (sorting the rows
per variable, the copies both ways, reading the records back).  Each of the three measurements runs in a child process
of its own under its own time limit; a child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

N, P = 813, 7
PARTS = ("one", "batch", "singles")


def data(k, n=N):
    rng = np.random.default_rng([17, k])
    X = np.round(rng.uniform(0.0, 1.0, (n, P)), 3)
    y = (3.0 * np.maximum(X[:, 0] - 0.4, 0.0) - 2.0 * np.maximum(0.6 - X[:, 1], 0.0) + 1.5 * X[:, 2] + np.sin(5.0 * X[:, 3])
         + 0.1 * rng.standard_normal(n))
    return X, y


def layer():
    """the 121 training sets of a layer: 11 models, each with its ten nfold sub-models"""
    sets = []
    for k in range(11):
        X, y = data(k)
        fold = np.resize(np.arange(1, 11), N)[np.random.default_rng([18, k]).permutation(N)]
        sets.append((X, y))
        sets += [(X[fold != f], y[fold != f]) for f in range(1, 11)]
    return sets


def device_part(part, repeats):
    import machisplin_amd as mhs
    mhs.init()
    sets = [data(0)] if part == "one" else layer()
    Xs, ys = [s[0] for s in sets], [s[1] for s in sets]

    def run():
        if part == "singles":
            return [mhs.models.Earth.fit(X, y) for X, y in sets]
        return mhs.models.earth_fit_many(Xs, ys)

    models = run()                                             # warm-up
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
    print("DEVICE " + json.dumps({"part": part, "models": len(sets), "s": statistics.median(times), "min_s": min(times), "max_s": max(times),
                                  "terms": [len(m.selected) for m in models][:11]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-part", choices=PARTS, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=150, help="seconds each GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a.device_part, a.repeats)
        return 0
    lines = ["earth fit, n = %d, p = %d, default arguments (nk 21); median of %d passes after a warm-up, host work included" % (N, P, a.repeats)]
    res = {}
    for part in PARTS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", part, "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode or 1
        res[part] = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
    what = {"one": "one model, one call", "batch": "a layer's 121 models in ONE call", "singles": "the same 121 models, one call each"}
    for part in PARTS:
        d = res[part]
        lines.append("%-36s %9.3f ms [%0.3f .. %0.3f]  = %7.3f ms per model" % (what[part], 1e3 * d["s"], 1e3 * d["min_s"], 1e3 * d["max_s"],
                                                                              1e3 * d["s"] / d["models"]))
    lines.append("batched call against 121 single calls: %.1f x; forward terms of the first models: %s"
                 % (res["singles"]["s"] / res["batch"]["s"], res["batch"]["terms"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
