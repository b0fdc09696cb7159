#!/usr/bin/env python
"""Record the ksvm row-tile kernel's planes for tests/test_ksvm_resident_gpu.py.

Run on an MI355X from a checkout whose library was built from the commit BEFORE the resident-wave change
(svr_rt_kernel with one tile per wave at every P): the file is that build's word on what every cell
of the 5-row shapes is, and the test demands the same bits of every later build.

    python tools/make_ksvm_rowtile_golden.py [out.npz]        (default: tests/golden/ksvm_rowtile_parent.npz)

Inputs come from tests/ksvm_resident_cases.py (seeded, host-built); their SHA-256 is stored beside each plane so that the
test can tell changed inputs from a changed kernel.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import machisplin_amd as hip
    from machisplin_amd import synth
    import ksvm_resident_cases as kc

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ksvm_rowtile_parent.npz")
    hip.init()
    rec = {}
    for key, ncol, nsv, npos in kc.golden_cases():
        geom = synth.grid(kc.GOLDEN_NROW, ncol)
        pl, nodata = kc.planes(kc.GOLDEN_NROW, ncol, "f32")
        prm = kc.svr_params(geom, nsv=nsv, npos=npos)
        os.environ.pop("MHS_SVR_NO_ROWTILE", None)
        got = kc.row_tile_plane(hip, geom, pl, nodata, prm)
        os.environ["MHS_SVR_NO_ROWTILE"] = "1"
        plain = kc.row_tile_plane(hip, geom, pl, nodata, prm)
        del os.environ["MHS_SVR_NO_ROWTILE"]
        assert not np.array_equal(got, plain, equal_nan=True), "the row-tile kernel did not run"
        assert np.nanmax(np.abs(got - plain)) <= 1e-12 * np.nanmax(np.abs(plain))
        rec[key] = got
        rec[key + "_sha256"] = np.array(kc.digest(pl, prm))
        print(key, got.shape, "NA cells", int(np.isnan(got).sum()), rec[key + "_sha256"])
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
