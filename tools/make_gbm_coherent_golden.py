#!/usr/bin/env python
"""Record the coherent gbm kernel's planes for tests/test_gbm_coherent_parent_gpu.py.

Run on an MI355X from a checkout whose library was built from the commit BEFORE the per-lane lists went
(gbm_coherent_kernel building (threshold, predictor, bit position) lists of the straddling levels in every lane): the
file is that build's word on what every cell of the cases is, and the test demands the same bits of every later build.

    python tools/make_gbm_coherent_golden.py [out.npz]        (default: tests/golden/gbm_coherent_parent.npz)

Inputs come from tests/gbm_coherent_cases.py (seeded, host-built); their SHA-256 is stored beside each plane so that the
test can tell changed inputs from a changed kernel.  The planes together are 10 MB of doubles that do not compress, so each
is stored as the SHA-256 of its bits plus a sample of its cells (gbm_coherent_cases.sample); the window of 2^20 cells, which
goes through the probe, also stores the probe's (cost, count).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import machisplin_amd as hip
    import gbm_coherent_cases as gc

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gbm_coherent_parent.npz")
    hip.init()
    for k in ("MHS_GBM_FORCE_COHERENT", "MHS_GBM_NO_COHERENT"):
        os.environ.pop(k, None)
    rec = {}
    for name in gc.case_names():
        geom, pl, nodata, prm, win, forced = gc.build(name)
        got, model = gc.predict(hip, name)
        if not forced:
            cost, count = gc.probe_last(model)
            assert count > 0 and cost < 83 * count, ("the probe did not pick the coherent kernel", cost, count)
            rec[name + "_probe"] = np.array([cost, count], dtype=np.int64)
        plain, _ = gc.predict(hip, name, env=("MHS_GBM_NO_COHERENT",))
        assert np.array_equal(np.isnan(got), np.isnan(plain))
        assert not np.array_equal(got, plain, equal_nan=True), "the coherent kernel did not run"
        assert np.nanmax(np.abs(got - plain)) <= 1e-13 * np.nanmax(np.abs(plain))
        rec[name + "_plane_sha256"] = np.array(gc.plane_digest(got))
        rec[name + "_sample"] = gc.sample(got)
        rec[name + "_shape"] = np.array(got.shape, dtype=np.int64)
        rec[name + "_sha256"] = np.array(gc.digest(pl, prm))
        print(name, got.shape, "NA cells", int(np.isnan(got).sum()), rec[name + "_plane_sha256"], rec.get(name + "_probe"))
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
