"""gbm_coherent_kernel without its per-lane lists of the straddling levels (a straddling tree's class words are re-read
when the cell loop reaches the tree; the lut_cls format is unchanged): every plane is, bit for bit, the plane of the kernel
it replaces, the one that built those lists (tests/golden/gbm_coherent_parent.npz, recorded by
tools/make_gbm_coherent_golden.py from a build of the commit before).  The fixture keeps the SHA-256 of each plane's float64
bits and a sample of its cells (the planes themselves are 10 MB that do not compress); the window of 2^20 cells goes through
the probe and both launches, and its probe sums must be the recorded ones too, since which kernel a window gets decides its
bits.  A digest that fails while the sample agrees says that cells outside the sampled columns differ, not which: run the
tool on both builds and compare the planes to find them.

Not run by any test: a model with 2^20 or more distinct split values of one predictor, for which build_lut_meta_t publishes
no class words and the model keeps off this kernel (it would need some 210 000 trees).

Cases (tests/gbm_coherent_cases.py): smooth planes with 900 trees (15 chunks: both LDS buffers in both parities), fast
planes with 1 % NoData (3-5 straddling levels), float64 planes in a window clipped on all four sides, int16 with three
splits and one split (padding levels), 64 and 70 trees (one chunk; a second chunk of padding), eight predictors."""
import functools
import os

import numpy as np
import pytest

import gbm_coherent_cases as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbm_coherent_parent.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_every_straddle_class_occurs_in_the_cases():
    """(tile, tree) pairs with 0, 1, 2, 3, 4 and 5 straddling levels, counted on the host from the ranks: at least 50 of each
    over the forced cases (the singles, the pairs and every depth of the three-or-more loop run)."""
    total = np.zeros(6, dtype=np.int64)
    for name in gc.case_names():
        if name != "probe_2p20":
            total += gc.straddle_histogram(name)
    assert (total >= 50).all(), total


@pytest.mark.gpu
@pytest.mark.parametrize("name", gc.case_names())
def test_planes_are_the_parent_kernels_bits(hip, name):
    g = _golden()
    geom, pl, nodata, prm, win, forced = gc.build(name)
    assert str(g[name + "_sha256"]) == gc.digest(pl, prm), "the inputs are not the recorded ones: the fixture says nothing"
    got, model = gc.predict(hip, name)
    r0, r1, c0, c1 = win
    assert got.shape == tuple(g[name + "_shape"]) == (r1 - r0, c1 - c0)
    if not forced:
        assert gc.probe_last(model) == tuple(int(x) for x in g[name + "_probe"])
    smp, want = gc.sample(got), g[name + "_sample"]
    differ = smp.view(np.uint64) != want.view(np.uint64)
    print(name, "sampled cells that differ:", int(differ.sum()), "of", differ.size,
          "largest difference", float(np.nanmax(np.abs(smp - want))))
    assert not differ.any(), "sampled cells differ from the parent's: first at sample index %s" % (np.argwhere(differ)[:1].tolist(),)
    assert gc.plane_digest(got) == str(g[name + "_plane_sha256"]), \
        "the plane's bits are not the parent's although all %d sampled cells agree: the cells that differ lie outside the " \
        "sample (every 13th column); the fixture cannot say where" % differ.size
