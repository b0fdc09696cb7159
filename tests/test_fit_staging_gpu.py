"""GPU: the host staging of the five batched fits (mhs_gbm_grow_many, mhs_rf_fit_many, mhs_earth_fit_many,
mhs_nnet_fit_many, mhs_svr_fit_many).  Three models of 37, 63 and 101 rows (p = 3) share ONE call: odd lengths, so every
piece of a model and every model is followed by padding up to the next 16-byte boundary of the device block.  The same
three in reverse order, and each alone, lie at other offsets of the block; every output array and scalar of every model
must be the same to the last bit in all three ways.  A piece that is misplaced, too short or read back from the wrong
offset shows here."""
import numpy as np
import pytest

import gbm_inputs
import rf_inputs

pytestmark = pytest.mark.gpu

ROWS, P = (37, 63, 101), 3


def _sets():
    out = []
    for k, n in enumerate(ROWS):
        rng = np.random.default_rng([50, k])
        X = rng.normal(size=(n, P))
        out.append((X, np.sin(X[:, 0]) + 0.3 * X[:, 1] * X[:, 2] + 0.1 * rng.normal(size=n)))
    return out


def _flat(prefix, obj):
    """every array and scalar below obj (dicts walked), as name -> bytes"""
    if isinstance(obj, dict):
        out = {}
        for key, val in obj.items():
            out.update(_flat(prefix + "." + key, val))
        return out
    a = np.asarray(obj)
    return {prefix: (a.dtype.str, a.shape, a.tobytes())}


def _record(m, names):
    out = {}
    for name in names:
        out.update(_flat(name, getattr(m, name)))
    return out


def _three_ways(fit, names, extra):
    """fit(Xs, ys, extras) -> models.  The batch, the batch reversed, every model alone: equal records."""
    sets = _sets()
    Xs, ys = [s[0] for s in sets], [s[1] for s in sets]
    batch = fit(Xs, ys, extra)
    back = fit(Xs[::-1], ys[::-1], [e[::-1] for e in extra])[::-1]
    alone = [fit([Xs[k]], [ys[k]], [[e[k]] for e in extra])[0] for k in range(len(sets))]
    for k in range(len(sets)):
        want = _record(alone[k], names)
        assert len(want) >= len(names)
        for other in (batch[k], back[k]):
            got = _record(other, names)
            assert got.keys() == want.keys()
            for key in want:
                assert got[key] == want[key], (k, key)
    return batch


def test_gbm_three_ways(hip):
    bags = [gbm_inputs.bags_for(n, 5, [51, k]) for k, n in enumerate(ROWS)]
    fit = lambda Xs, ys, e: hip.models.gbm_fit_many(Xs, ys, 5, e[0], interaction_depth=3, n_minobsinnode=3)
    batch = _three_ways(fit, ("params", "fit", "init_f"), [bags])
    for m, n in zip(batch, ROWS):
        assert m.params["tree_offsets"].shape == (6,) and m.params["tree_offsets"][-1] >= 5 and m.fit.shape == (n,)


def test_rf_three_ways(hip):
    drawn = [rf_inputs.bags_for(n, 5, [52, k]) for k, n in enumerate(ROWS)]
    fit = lambda Xs, ys, e: hip.models.rf_fit_many(Xs, ys, 5, inbag=e[0], seeds=e[1])
    batch = _three_ways(fit, ("params", "oob_pred", "oob_count", "inc_node_purity"), [[d[0] for d in drawn], [d[1] for d in drawn]])
    for m, n in zip(batch, ROWS):
        assert m.params["tree_offsets"].shape == (6,) and m.oob_pred.shape == (n,) and m.inc_node_purity.shape == (P,)


def test_earth_three_ways(hip):
    fit = lambda Xs, ys, e: hip.models.earth_fit_many(Xs, ys)
    names = ("params", "forward", "selected", "rss_per_subset", "gcv_per_subset", "prune_terms", "rss", "gcv", "rsq", "grsq")
    batch = _three_ways(fit, names, [])
    assert all(m.params["coef"].size >= 2 for m in batch)


def test_nnet_three_ways(hip):
    w0 = [np.random.default_rng([53, k]).uniform(-0.7, 0.7, (P + 1) * 10 + 10 + 1) for k in range(len(ROWS))]
    fit = lambda Xs, ys, e: hip.models.nnet_fit_many(Xs, ys, e[0], maxit=25)
    batch = _three_ways(fit, ("wts", "value", "counts", "fail"), [w0])
    assert all(m.counts[0] > 1 and not np.array_equal(m.wts, w) for m, w in zip(batch, w0))


def test_ksvm_three_ways(hip):
    fit = lambda Xs, ys, e: hip.models.ksvm_fit_many(Xs, ys, 0.3)
    batch = _three_ways(fit, ("params", "beta", "n_iter"), [])
    assert all(m.n_iter > 0 and m.beta.shape == (n,) for m, n in zip(batch, ROWS))
