#!/usr/bin/env python
"""Time of the device growth of randomForest regression forests (mhs_rf_fit_many), p = 7, mtry = 2, nodesize 5:

* 500 trees at n = 813 (the bundled example's stations);
* 500 trees at n = 5 000;
* ten fold forests of 4 500 rows, 500 trees each, in ONE call (5 000 trees in one launch);

with, as CONTEXT FROM A DIFFERENT IMPLEMENTATION (not a target), the wall time of scikit-learn's
RandomForestRegressor(n_estimators=500, max_features=mtry, min_samples_split=6, n_jobs=16) on the same rows.

    python tools/rf_grow_speed.py [--repeats 5] [--out profiles/rf_grow_speed.txt] [--no-sklearn]

Every device figure is the median of ``--repeats`` timed calls after one warm-up call, between two HIP events recorded
on the default stream around the whole call: the host's part (sorting the rows per variable, the copies both ways,
mhs_rf_load of the result) is included, drawing the bags is not.  The GPU part runs in a child process of its own under a
time limit."""
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

P, MTRY, TREES = 7, 2, 500
CASES = (("500 trees, n = 813", 1, 813), ("500 trees, n = 5000", 1, 5000), ("10 fold forests of 4500 rows, 500 trees each", 10, 4500))


def data(n, k):
    rng = np.random.default_rng([17, n, k])
    X = rng.normal(size=(n, P))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] * X[:, 2] + 0.2 * np.abs(X[:, 3]) + 0.1 * rng.normal(size=n)
    return X, y


def device_part(repeats):
    import torch
    import machisplin_amd as mhs
    mhs.init()
    out = []
    for label, count, n in CASES:
        sets = [data(n, k) for k in range(count)]
        Xs, ys = [s[0] for s in sets], [s[1] for s in sets]
        bags, seeds = [], []
        for k in range(count):
            rng = np.random.default_rng([18, n, k])
            bags.append(np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(TREES)]).astype(np.int32))
            seeds.append(rng.integers(0, 2 ** 64, size=TREES, dtype=np.uint64))
        run = lambda: mhs.models.rf_fit_many(Xs, ys, TREES, MTRY, 5, bags, seeds)
        models = run()                                     # warm-up
        nodes = int(sum(m.params["tree_offsets"][-1] for m in models))
        del models
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ms = run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
            del ms
        out.append({"case": label, "models": count, "n": n, "nodes": nodes, "call_s": statistics.median(times), "min_s": min(times),
                    "max_s": max(times)})
    print("DEVICE " + json.dumps(out))


def sklearn_part(count, n, jobs):
    from sklearn.ensemble import RandomForestRegressor
    t0 = time.perf_counter()
    for k in range(count):
        X, y = data(n, k)
        RandomForestRegressor(n_estimators=TREES, max_features=MTRY, min_samples_split=6, n_jobs=jobs, random_state=k).fit(X, y)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a.repeats)
        return 0
    lines = ["randomForest growth, p = %d, mtry = %d, nodesize 5, %d trees per forest; median of %d calls after a warm-up (HIP events around the call)"
             % (P, MTRY, TREES, a.repeats)]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--repeats", str(a.repeats)],
                       capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    dev = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
    for d in dev:
        lines.append("device  %-46s %8.3f s per call [%0.3f .. %0.3f], %d nodes" % (d["case"] + ":", d["call_s"], d["min_s"], d["max_s"], d["nodes"]))
    if not a.no_sklearn:
        jobs = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
        for label, count, n in CASES:
            lines.append("sklearn %-46s %8.3f s wall, n_jobs = %d (context: a different implementation, not a target)"
                         % (label + ":", sklearn_part(count, n, jobs), jobs))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
