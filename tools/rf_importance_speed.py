#!/usr/bin/env python
"""Time of the device permutation importance of a randomForest regression forest (mhs_rf_importance_many), 500 trees,
n_perm = 1, default mtry and nodesize:

* the layer shape of tools/learn_fit_many_speed.py: n = 732, p = 5 (the generator of that tool);
* n = 5 000, p = 5: past the rows the kernel keeps on chip;

each beside the time of models.rf_fit_many for the same forest, for scale.

    python tools/rf_importance_speed.py [--repeats 5] [--out profiles/rf_importance_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, wall clock around the whole Python call
(the call returns after its results are on the host): the host's part -- the argument checks, staging, the copies both
ways, for the fit the sorting of the rows and mhs_rf_load -- is included, drawing the bags and seeds is not.  The GPU
part runs in a child process of its own under a time limit."""
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

P, TREES, N_PERM = 5, 500, 1
CASES = (("n = 732 (a fold of the 813 stations)", 732), ("n = 5000", 5000))


def data(n):
    rng = np.random.default_rng([23, n])
    X = rng.normal(size=(n, P)) * np.array([1, 2, 3, 1, 5.0]) + np.arange(P)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.05 * X[:, 2] * X[:, 3] + 0.1 * rng.normal(size=n)
    return X, y


def median_of(run, repeats):
    run()                                                   # warm-up
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def device_part(repeats):
    import machisplin_amd as mhs
    mhs.init()
    out = []
    for label, n in CASES:
        X, y = data(n)
        rng = np.random.default_rng([24, n])
        bags = np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(TREES)]).astype(np.int32)
        seeds = rng.integers(0, 2 ** 64, size=TREES, dtype=np.uint64)
        perm = rng.integers(0, 2 ** 64, size=TREES, dtype=np.uint64)
        fit = median_of(lambda: mhs.models.rf_fit_many([X], [y], TREES, None, 5, [bags], [seeds]), repeats)
        m = mhs.models.rf_fit_many([X], [y], TREES, None, 5, [bags], [seeds])[0]
        imp = median_of(lambda: mhs.models.rf_importance_many([m], [X], [y], [bags], [perm], N_PERM), repeats)
        out.append({"case": label, "n": n, "nodes": int(m.params["tree_offsets"][-1]), "oob": int((bags == 0).sum()), "fit": fit, "importance": imp,
                    "inc_mse": [float(v) for v in m.importance[:, 0]]})
    print("DEVICE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rf_importance_speed.txt"))
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a.repeats)
        return 0
    lines = ["randomForest permutation importance, p = %d, %d trees, n_perm = %d, default mtry and nodesize; median of %d passes after a "
             "warm-up [min .. max], wall clock around the Python call, host work included" % (P, TREES, N_PERM, a.repeats)]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats)],
                       capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    for d in json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:]):
        lines.append("%-38s rf_importance_many %7.4f s [%0.4f .. %0.4f]   rf_fit_many (for scale) %7.4f s [%0.4f .. %0.4f]   %d nodes, %d "
                     "out-of-bag rows over the trees" % ((d["case"] + ":",) + tuple(d["importance"]) + tuple(d["fit"]) + (d["nodes"], d["oob"])))
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
