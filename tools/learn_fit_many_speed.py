#!/usr/bin/env python
"""Wall time of a layer's nnet and ksvm fits in ONE call (mhs_nnet_fit_many / mhs_svr_fit_many) against the loop of
single fits (Nnet.fit / Ksvm.fit), at the shape of the bundled example: 732 training rows (nine tenths of 813
stations), p = 5, nnet with maxit = 10000, ksvm with kernlab's defaults and sigma = 0.2 -- 11 models (a layer: ten fold
models and the final one) and 132 models (twelve layers).

    python tools/learn_fit_many_speed.py [--repeats 5] [--out profiles/learn_fit_many_speed.txt]

Every figure is the median of ``--repeats`` timed passes after one warm-up pass, host work included (scaling, the
copies both ways, building the model objects); the calls are synchronous.  Each measurement runs in a child process of
its own under its own time limit; a child that fails ends the run.  The data are synthetic."""
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

N, P, SIGMA = 732, 5, 0.2
MEMBERS = ("nnet", "ksvm")
COUNTS = (11, 132)
ROUTES = ("batch", "singles")


def data(k):
    rng = np.random.default_rng([23, k])
    X = rng.normal(size=(N, P)) * np.array([1, 2, 3, 1, 5.0]) + np.arange(P)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.05 * X[:, 2] * X[:, 3] + 0.1 * rng.normal(size=N)
    return X, y


def device_part(member, count, route, repeats):
    import machisplin_amd as mhs
    mhs.init()
    sets = [data(k) for k in range(count)]
    Xs, ys = [s[0] for s in sets], [s[1] for s in sets]
    w0 = [np.random.default_rng([29, k]).uniform(-0.7, 0.7, (P + 1) * 10 + 11) for k in range(count)]

    def run():
        if member == "nnet":
            if route == "batch":
                return mhs.models.nnet_fit_many(Xs, ys, w0)
            return [mhs.models.Nnet.fit(X, y, w) for (X, y), w in zip(sets, w0)]
        if route == "batch":
            return mhs.models.ksvm_fit_many(Xs, ys, SIGMA)
        return [mhs.models.Ksvm.fit(X, y, SIGMA) for X, y in sets]

    models = run()                                             # warm-up
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
    work = [m.counts[0] + m.counts[1] for m in models] if member == "nnet" else [m.n_iter for m in models]
    print("DEVICE " + json.dumps({"member": member, "models": count, "route": route, "s": statistics.median(times), "min_s": min(times),
                                  "max_s": max(times), "work_max": int(max(work)), "work_mean": float(np.mean(work))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-part", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=240, help="seconds each GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        member, count, route = a.device_part.split(":")
        device_part(member, int(count), route, a.repeats)
        return 0
    lines = ["nnet (maxit 10000) and ksvm (sigma %.1f) fits, n = %d, p = %d; median of %d passes after a warm-up, host work included; "
             "work = evaluations (nnet) / SMO iterations (ksvm) of a model" % (SIGMA, N, P, a.repeats)]
    for member in MEMBERS:
        for count in COUNTS:
            res = {}
            for route in ROUTES:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "%s:%d:%s" % (member, count, route),
                                    "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return r.returncode or 1
                res[route] = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
            for route, what in (("batch", "ONE call"), ("singles", "one call each")):
                d = res[route]
                lines.append("%-5s %3d models, %-13s %10.3f ms [%0.3f .. %0.3f]  = %8.3f ms per model" % (
                    member, count, what, 1e3 * d["s"], 1e3 * d["min_s"], 1e3 * d["max_s"], 1e3 * d["s"] / count))
            lines.append("%-5s %3d models: the batched call against the loop of single fits: %.1f x; work of the slowest model %d, mean %.0f"
                         % (member, count, res["singles"]["s"] / res["batch"]["s"], res["batch"]["work_max"], res["batch"]["work_mean"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
