// The ensemble members' model handle (mhs_model, ensemble_int.h): the loaders of lm, nnet, earth, ksvm and gbm -- check the
// caller's arrays, convert them to what the kernels read, upload, adopt --, the handle's twin on another device slot, its
// release.  Host code only: the kernels and everything that launches one are in ensemble.hip; randomForest's loader builds
// the forest kernels' tables and stays beside them in forest.hip.
#include <algorithm>
#include <cmath>
#include <functional>
#include <mutex>
#include <vector>
#include "ensemble_int.h"

namespace mhs {

int finish_trees(mhs_model *m, const std::vector<Node> &nodes, const std::vector<int> &off) {
    const int nt = m->n_trees;
    const size_t xs_bytes = (size_t)m->p * TREE_R * 256 * sizeof(double);
    int biggest = 0;
    for (int t = 0; t < nt; ++t) biggest = std::max(biggest, off[t + 1] - off[t]);
    int cap = (m->kind == K_GBM) ? std::max(GBM_CHUNK_NODES, biggest) : biggest;
    m->lds_ok = xs_bytes + (size_t)cap * sizeof(Node) <= LDS_LIMIT;
    std::vector<TreeChunk> chunks;
    if (m->lds_ok) {
        int t = 0;
        while (t < nt) {
            TreeChunk c{t, 0, off[t], 0};
            while (t < nt && off[t + 1] - c.node_begin <= cap) { ++t; }
            c.n_trees = t - c.first_tree;
            c.node_count = off[t] - c.node_begin;
            chunks.push_back(c);
        }
        m->max_chunk_nodes = cap;
    } else {
        chunks.push_back(TreeChunk{0, nt, 0, off[nt]});
        m->max_chunk_nodes = 0;
    }
    m->n_chunks = (int)chunks.size();
    m->n_nodes = (int64_t)nodes.size();
    if (int rc = to_device(nodes.data(), nodes.size(), &m->nodes)) return rc;
    if (int rc = to_device(off.data(), off.size(), &m->tree_off)) return rc;
    return to_device(chunks.data(), chunks.size(), &m->chunks);
}

int check_common(int p, mhs_model **out) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(out != nullptr, "out is NULL");
    MHS_REQUIRE(p >= 2 && p <= 64, "p (covariates + LONG + LAT) out of range: the loaders take 2 .. 64 predictors");
    return MHS_OK;
}

// The handle's twin on another device slot, built on first use from the remembered loader call.
int model_on_slot(const mhs_model *m, int slot, const mhs_model **out) {
    MHS_REQUIRE(m && out && slot >= 0 && slot < MAX_SLOTS, "bad arguments");
    const int dev = ctx_slot(slot).device;
    if (m->slot == slot && m->device == dev) { *out = m; return MHS_OK; }
    mhs_model *w = const_cast<mhs_model *>(m);
    std::lock_guard<std::mutex> lk(w->mu);
    if (w->replica[slot] && w->replica[slot]->device != dev) {      // the slots were re-initialised on other devices
        mhs_model_free(w->replica[slot]);
        w->replica[slot] = nullptr;
    }
    if (!w->replica[slot]) {
        MHS_REQUIRE((bool)w->reload, "model handle cannot be replicated");
        SlotBind bind(slot);
        mhs_model *r = nullptr;
        if (int rc = w->reload(&r)) return rc;
        w->replica[slot] = r;
    }
    *out = w->replica[slot];
    return MHS_OK;
}

// A handle under construction: released on every exit of its loader except the last step, adopt(): the handle remembers
// where its buffers live and the loader call that built it (`reload`, with copies of the flat arrays: model_on_slot
// repeats it on another slot) and goes to the caller.
struct Loading {
    mhs_model *m = new mhs_model();
    Loading() = default;
    Loading(const Loading &) = delete;
    Loading &operator=(const Loading &) = delete;
    ~Loading() { if (m) mhs_model_free(m); }
    mhs_model *operator->() const { return m; }
    int adopt(std::function<int(mhs_model **)> reload, mhs_model **out) {
        m->slot = current_slot(); m->device = ctx().device;
        m->reload = std::move(reload);
        *out = m;
        m = nullptr;
        return MHS_OK;
    }
};

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_model_free(mhs_model *m) {
    if (!m) return MHS_OK;
    for (mhs_model *&r : m->replica) if (r) { mhs_model_free(r); r = nullptr; }
    void *const device_blocks[] = {m->dpar, m->ipar, m->nodes, m->tree_off, m->chunks, m->split_scratch, m->na_list[0], m->na_list[1],
                                   m->na_list[2], m->na_list[3], m->lut, m->lut_meta, m->lut_rt, m->lut_rt_meta, m->lut_cls, m->gbm_probe,
                                   m->lut_sorted, m->lut_sorted_off, m->axis_rank, m->rf_nodes, m->rf_lval, m->rf_depth, m->rf_dmin,
                                   m->rf_coff, m->rf_csub, m->rf_clval};
    for (void *q : device_blocks) (void)hipFree(q);      // hipFree(NULL) succeeds
    for (void *q : m->retired) (void)hipFree(q);
    for (hipEvent_t e : m->na_done) if (e) (void)hipEventDestroy(e);
    delete m;
    return MHS_OK;
}

int mhs_lm_load(const double *coef, int p, mhs_model **out) {
    if (int rc = check_common(p, out)) return rc;
    MHS_REQUIRE(coef != nullptr, "coef is NULL");
    Loading m;
    m->kind = K_LM; m->p = p;
    if (int rc = to_device(coef, (size_t)p + 1, &m->dpar)) return rc;
    return m.adopt([v = std::vector<double>(coef, coef + p + 1), p](mhs_model **o) { return mhs_lm_load(v.data(), p, o); }, out);
}

int mhs_nnet_load(const double *wts, int p, int size, double y_scale, double y_shift, mhs_model **out) {
    if (int rc = check_common(p, out)) return rc;
    MHS_REQUIRE(wts != nullptr && size >= 1 && size <= 4096, "bad nnet arguments");
    static_assert(PMAX == 12, "the message below names the limit");
    MHS_REQUIRE(p <= PMAX, "p exceeds the 12 predictors supported for nnet");
    Loading m;
    m->kind = K_NNET; m->p = p; m->n0 = size; m->s0 = y_scale; m->s1 = y_shift;
    if (int rc = to_device(wts, (size_t)(p + 1) * size + size + 1, &m->dpar)) return rc;
    return m.adopt([v = std::vector<double>(wts, wts + (size_t)(p + 1) * size + size + 1), p, size, y_scale, y_shift](mhs_model **o) {
        return mhs_nnet_load(v.data(), p, size, y_scale, y_shift, o);
    }, out);
}

int mhs_earth_load(const double *coef, const int32_t *dirs, const double *cuts, int nterms, int p,
                   mhs_model **out) {
    if (int rc = check_common(p, out)) return rc;
    MHS_REQUIRE(coef && dirs && cuts && nterms >= 1, "bad earth arguments");
    std::vector<int> tstart(1, 0), fvar, fdir;
    std::vector<double> fcut;
    for (int k = 0; k < nterms; ++k) {
        for (int v = 0; v < p; ++v) {
            const int d = dirs[(size_t)k * p + v];
            MHS_REQUIRE(d == 0 || d == 1 || d == -1 || d == 2, "earth dirs must be 0, 1, -1 or 2");
            if (d != 0) { fvar.push_back(v); fdir.push_back(d); fcut.push_back(cuts[(size_t)k * p + v]); }
        }
        tstart.push_back((int)fvar.size());
    }
    Loading m;
    m->kind = K_EARTH; m->p = p; m->n0 = nterms; m->n1 = (int)fvar.size();
    std::vector<double> dp(coef, coef + nterms);
    dp.insert(dp.end(), fcut.begin(), fcut.end());
    std::vector<int> ip(tstart);
    ip.insert(ip.end(), fvar.begin(), fvar.end());
    ip.insert(ip.end(), fdir.begin(), fdir.end());
    int rc = to_device(dp.data(), dp.size(), &m->dpar);
    if (!rc) rc = to_device(ip.data(), ip.size(), &m->ipar);
    if (rc) return rc;
    return m.adopt([c = std::vector<double>(coef, coef + nterms), d = std::vector<int32_t>(dirs, dirs + (size_t)nterms * p),
                    q = std::vector<double>(cuts, cuts + (size_t)nterms * p), nterms, p](mhs_model **o) {
        return mhs_earth_load(c.data(), d.data(), q.data(), nterms, p, o);
    }, out);
}

int mhs_svr_load(const double *alpha, const double *sv, int64_t nsv, int p, double b, double sigma,
                 const double *x_center, const double *x_scale, double y_center, double y_scale,
                 mhs_model **out) {
    if (int rc = check_common(p, out)) return rc;
    MHS_REQUIRE(alpha && sv && x_center && x_scale && nsv >= 1 && nsv < (1LL << 30), "bad ksvm arguments");
    MHS_REQUIRE(p <= PMAX, "p exceeds the 12 predictors supported for ksvm");
    MHS_REQUIRE(sigma > 0, "sigma must be positive");
    for (int j = 0; j < p; ++j) MHS_REQUIRE(x_scale[j] != 0.0, "x_scale has a zero entry");
    const int stride = ((p + 1) + 3) & ~3;  // doubles per support vector, 32-byte multiple
    // support vectors with alpha > 0 first, then alpha < 0 (alpha = 0 contributes nothing), |alpha| / amax folded
    // into the exponent
    double amax = 0.0;
    std::vector<int64_t> order;
    for (int64_t v = 0; v < nsv; ++v) {
        MHS_REQUIRE(std::isfinite(alpha[v]), "non-finite alpha");
        amax = std::max(amax, fabs(alpha[v]));
        if (alpha[v] > 0) order.push_back(v);
    }
    const int npos = (int)order.size();
    for (int64_t v = 0; v < nsv; ++v) if (alpha[v] < 0) order.push_back(v);
    const int64_t nkeep = (int64_t)order.size();
    std::vector<double> h((size_t)nkeep * stride + 2 * p, 0.0);
    for (int64_t e = 0; e < nkeep; ++e) {
        const int64_t v = order[(size_t)e];
        double ss = 0.0;
        for (int j = 0; j < p; ++j) {
            const double x = sv[(size_t)v * p + j];
            h[(size_t)e * stride + j] = -2.0 * sigma * x / EXP_RANGE;
            ss += x * x;
        }
        h[(size_t)e * stride + p] = (sigma * ss - log(fabs(alpha[v]) / amax)) / EXP_RANGE;
    }
    for (int j = 0; j < p; ++j) { h[(size_t)nkeep * stride + j] = x_center[j]; h[(size_t)nkeep * stride + p + j] = x_scale[j]; }
    Loading m;
    m->kind = K_SVR; m->p = p; m->n0 = (int)nkeep; m->n1 = stride; m->n2 = npos; m->s4 = amax;
    m->s0 = b; m->s1 = sigma; m->s2 = y_center; m->s3 = y_scale;
    if (int rc = to_device(h.data(), h.size(), &m->dpar)) return rc;
    return m.adopt([a = std::vector<double>(alpha, alpha + nsv), v = std::vector<double>(sv, sv + (size_t)nsv * p), nsv, p, b, sigma,
                    xc = std::vector<double>(x_center, x_center + p), xs = std::vector<double>(x_scale, x_scale + p), y_center,
                    y_scale](mhs_model **o) {
        return mhs_svr_load(a.data(), v.data(), nsv, p, b, sigma, xc.data(), xs.data(), y_center, y_scale, o);
    }, out);
}

int mhs_gbm_load(double init_f, int64_t n_trees, const int64_t *tree_offsets, const int32_t *split_var,
                 const double *split_val, const int32_t *left, const int32_t *right,
                 const int32_t *missing, int p, mhs_model **out) {
    if (int rc = check_common(p, out)) return rc;
    MHS_REQUIRE(tree_offsets && split_var && split_val && left && right && missing, "NULL gbm array");
    MHS_REQUIRE(n_trees >= 0 && n_trees < (1LL << 30) && tree_offsets[0] == 0, "bad tree offsets");
    const int64_t nn = tree_offsets[n_trees];
    MHS_REQUIRE(nn < (1LL << 31), "too many nodes");
    std::vector<Node> nodes((size_t)nn);
    std::vector<int> off((size_t)n_trees + 1);
    for (int64_t t = 0; t <= n_trees; ++t) off[t] = (int)tree_offsets[t];
    for (int64_t t = 0; t < n_trees; ++t) {
        const int64_t o = tree_offsets[t], cnt = tree_offsets[t + 1] - o;
        MHS_REQUIRE(cnt >= 1 && cnt <= 65535, "a gbm tree must have 1..65535 nodes");
        for (int64_t k = 0; k < cnt; ++k) {
            Node &nd = nodes[(size_t)(o + k)];
            nd.val = split_val[o + k];
            nd.var = (short)split_var[o + k];
            if (split_var[o + k] >= 0) {
                MHS_REQUIRE(split_var[o + k] < p, "gbm SplitVar out of range");
                MHS_REQUIRE(left[o + k] >= 0 && left[o + k] < cnt && right[o + k] >= 0 && right[o + k] < cnt &&
                            missing[o + k] >= 0 && missing[o + k] < cnt, "gbm child index out of range");
                nd.left = (unsigned short)left[o + k]; nd.right = (unsigned short)right[o + k];
                nd.missing = (unsigned short)missing[o + k];
            } else { nd.var = -1; nd.left = nd.right = nd.missing = 0; }
        }
    }
    Loading m;
    m->kind = K_GBM; m->p = p; m->n_trees = (int)n_trees; m->init_f = init_f;
    if (int rc = finish_trees(m.m, nodes, off)) return rc;
    // predicate-LUT form (gbm_lut_kernel) when every tree has at most 6 splits
    int max_splits = 0;
    for (int64_t t = 0; t < n_trees; ++t) {
        int ns = 0;
        for (int k = off[t]; k < off[t + 1]; ++k) ns += nodes[(size_t)k].var >= 0;
        max_splits = std::max(max_splits, ns);
    }
    if (n_trees > 0 && max_splits <= 6) {
        const int S = max_splits <= 5 ? 5 : 6;
        m->lut_S = S;
        m->n_trees_padded = (int)((n_trees + LUT_CHUNK - 1) / LUT_CHUNK * LUT_CHUNK);
        m->lut_var.assign((size_t)n_trees * S, -1);
        m->lut_thr.assign((size_t)n_trees * S, 0.0);
        std::vector<double> lut(((size_t)m->n_trees_padded) << S, 0.0);
        std::vector<int> qmap;
        for (int64_t t = 0; t < n_trees; ++t) {
            const int o = off[t], cnt = off[t + 1] - off[t];
            qmap.assign((size_t)cnt, -1);
            int q = 0;
            for (int k = 0; k < cnt; ++k)
                if (nodes[(size_t)(o + k)].var >= 0) {
                    qmap[k] = q;
                    m->lut_var[(size_t)t * S + q] = nodes[(size_t)(o + k)].var;
                    m->lut_thr[(size_t)t * S + q] = nodes[(size_t)(o + k)].val;
                    ++q;
                }
            for (int b = 0; b < (1 << S); ++b) {
                int k = 0, guard = 0;
                while (nodes[(size_t)(o + k)].var >= 0 && guard++ <= cnt) {
                    const int bit = (b >> (S - 1 - qmap[k])) & 1;  // predicate 0 is the most significant bit
                    k = bit ? nodes[(size_t)(o + k)].left : nodes[(size_t)(o + k)].right;
                }
                lut[((size_t)t << S) + b] = nodes[(size_t)(o + k)].val;
            }
        }
        if (int rc = to_device(lut.data(), lut.size(), &m->lut)) return rc;
        m->lut_host = std::move(lut);
    }
    return m.adopt([init_f, n_trees, to = std::vector<int64_t>(tree_offsets, tree_offsets + n_trees + 1),
                    sv = std::vector<int32_t>(split_var, split_var + nn), sl = std::vector<double>(split_val, split_val + nn),
                    l = std::vector<int32_t>(left, left + nn), r = std::vector<int32_t>(right, right + nn),
                    ms = std::vector<int32_t>(missing, missing + nn), p](mhs_model **o) {
        return mhs_gbm_load(init_f, n_trees, to.data(), sv.data(), sl.data(), l.data(), r.data(), ms.data(), p, o);
    }, out);
}

int mhs_model_info(const mhs_model *m, int *kind, int *p, int64_t *n_trees) {
    MHS_REQUIRE(m != nullptr, "NULL model");
    if (kind) *kind = m->kind;
    if (p) *p = m->p;
    if (n_trees) *n_trees = (m->kind == K_GBM || m->kind == K_RF) ? m->n_trees : 0;
    return MHS_OK;
}

}  // extern "C"
