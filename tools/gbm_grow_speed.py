#!/usr/bin/env python
"""Wall time per tree of the device growth of gbm's trees (mhs_gbm_grow_many) at the size of a CV fold's training set:
n = 3600, p = 7, interaction depth 25, bag fraction 0.5 -- one model, and 10 and 100 models in one call -- with
scikit-learn's GradientBoostingRegressor (same tree shape, subsample 0.5) on the host's threads as a CPU yardstick.

    python tools/gbm_grow_speed.py [--trees 100] [--repeats 5] [--out profiles/gbm_grow_speed.txt] [--no-sklearn]

Every device figure is the median of ``--repeats`` timed calls after one warm-up call, host work of the call included
(sorting the rows per variable, the copies both ways).  The GPU part runs in a child process of its own under a time limit."""
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

N, P, DEPTH = 3600, 7, 25


def data(k):
    rng = np.random.default_rng([7, k])
    X = rng.normal(size=(N, P))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] * X[:, 2] + 0.2 * np.abs(X[:, 3]) + 0.1 * rng.normal(size=N)
    return X, y


def device_part(trees, repeats):
    import machisplin_amd as mhs
    mhs.init()
    out = []
    sets = [data(k) for k in range(100)]
    for count in (1, 10, 100):
        Xs, ys = [s[0] for s in sets[:count]], [s[1] for s in sets[:count]]
        bags = [np.stack([np.random.default_rng([9, k, t]).permutation(N)[:N // 2] for t in range(trees)]) for k in range(count)]
        mhs.models.gbm_fit_many(Xs, ys, trees, bags=bags)          # warm-up
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            mhs.models.gbm_fit_many(Xs, ys, trees, bags=bags)
            times.append(time.perf_counter() - t0)
        med = statistics.median(times)
        out.append({"models": count, "trees": trees, "call_s": med, "min_s": min(times), "max_s": max(times),
                    "ms_per_tree_of_one_model": 1e3 * med / trees, "ms_per_tree_and_model": 1e3 * med / (trees * count)})
    print("DEVICE " + json.dumps(out))


def sklearn_part(trees, models, threads):
    from concurrent.futures import ProcessPoolExecutor
    t0 = time.perf_counter()
    with ProcessPoolExecutor(max_workers=threads) as ex:
        list(ex.map(_sk_one, [(k, trees) for k in range(models)]))
    return time.perf_counter() - t0


def _sk_one(arg):
    from sklearn.ensemble import GradientBoostingRegressor
    k, trees = arg
    X, y = data(k)
    GradientBoostingRegressor(n_estimators=trees, learning_rate=0.01, max_leaf_nodes=DEPTH + 1, max_depth=None, min_samples_leaf=10,
                              subsample=0.5, criterion="squared_error", random_state=k).fit(X, y)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--device-part", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        device_part(a.trees, a.repeats)
        return 0
    lines = ["gbm growth, n = %d, p = %d, interaction depth %d, bag fraction 0.5, %d trees per call; median of %d calls after a warm-up"
             % (N, P, DEPTH, a.trees, a.repeats)]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "--trees", str(a.trees), "--repeats", str(a.repeats)],
                       capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    dev = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
    for d in dev:
        lines.append("device  %3d model(s) in one call: %8.3f s per call [%0.3f .. %0.3f]  = %7.3f ms per tree of a model, %7.3f ms per tree and model"
                     % (d["models"], d["call_s"], d["min_s"], d["max_s"], d["ms_per_tree_of_one_model"], d["ms_per_tree_and_model"]))
    if not a.no_sklearn:
        threads = int(os.environ.get("OMP_NUM_THREADS", "16"))
        for models in (1, 10, 100):
            s = sklearn_part(a.trees, models, min(threads, models))
            lines.append("sklearn %3d model(s), %2d processes:  %8.3f s                              = %7.3f ms per tree of a model, %7.3f ms per tree and model"
                         % (models, min(threads, models), s, 1e3 * s / a.trees, 1e3 * s / (a.trees * models)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
