#!/usr/bin/env python
"""Wall time of building Q = -M^-1 for the TPS prediction standard errors, on the host (the single-threaded block formula
of csrc/tps_se.hip, the yardstick) and on the device (csrc/tps_se_build.hip), by the number of distinct stations.

    python tools/se_build_speed.py [--repeats 5] [--out profiles/se_build_speed.txt]

The figure is ``build_ms`` of ``Tps.se_info()``: what the library itself measured around the build, the upload of Q
included for the host build.  Every pass fits a fresh handle (fixed lambda: the build does not depend on the fit's
route) and asks one standard error of it; the median of ``--repeats`` passes after one warm-up pass is reported, with
Q's bytes.  Each row runs in a child process of its own under its own time limit; a child that fails ends the run.
The stations are synthetic (uniform in a 2 x 2 degree box)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROWS = [(224, ("host", "device")), (750, ("host", "device")), (2000, ("host", "device")),
        (5000, ("device",)), (10000, ("device",)), (20000, ("device",))]
LAMBDA = 1e-3


def device_part(n, where, repeats):
    import machisplin_amd as mhs
    mhs.init()
    mhs.se_max_n(mhs.tps.SE_HARD_MAX_N)
    mhs.se_build_mode(mhs.SE_BUILD_HOST if where == "host" else mhs.SE_BUILD_DEVICE)
    rng = np.random.default_rng([31, n])
    xy = np.column_stack([rng.uniform(-78.0, -76.0, n), rng.uniform(-7.0, -5.0, n)])
    u = (xy - xy.min(0)) / (xy.max(0) - xy.min(0))
    y = np.sin(6 * u[:, 0]) * np.cos(5 * u[:, 1]) + 0.1 * rng.standard_normal(n)
    times, info, se = [], None, None
    for k in range(repeats + 1):
        fit = mhs.Tps(xy, y, lambda_=LAMBDA)
        se = fit.predict_se(xy[:1])
        info = fit.se_info()
        assert info["built_on"] == (mhs.SE_BUILD_HOST if where == "host" else mhs.SE_BUILD_DEVICE)
        if k:                                                   # pass 0 is the warm-up
            times.append(info["build_ms"])
        del fit
    print("DEVICE " + json.dumps({"n": n, "where": where, "ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
                                  "q_bytes": info["q_bytes"], "se0": float(se[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-part", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=300, help="seconds each GPU child process may take")
    a = ap.parse_args()
    if a.device_part:
        n, where = a.device_part.split(":")
        device_part(int(n), where, a.repeats)
        return 0
    lines = ["build of Q = -M^-1 (TPS standard errors), build_ms of se_info; fixed lambda %g, a fresh handle per pass, "
             "median of %d passes after a warm-up [min .. max]" % (LAMBDA, a.repeats)]
    for n, wheres in ROWS:
        res = {}
        for where in wheres:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-part", "%d:%s" % (n, where),
                                "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode or 1
            res[where] = json.loads([l for l in r.stdout.splitlines() if l.startswith("DEVICE ")][-1][7:])
            d = res[where]
            lines.append("n = %5d  %-6s build %11.3f ms [%0.3f .. %0.3f]   Q %13d bytes" % (
                n, where, d["ms"], d["min_ms"], d["max_ms"], d["q_bytes"]))
            print(lines[-1], flush=True)
        if len(res) == 2:
            lines.append("n = %5d  host build / device build: %.2f x; SE at the first station differs by %.1e relative" % (
                n, res["host"]["ms"] / res["device"]["ms"], abs(res["host"]["se0"] - res["device"]["se0"]) / res["host"]["se0"]))
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
