// Permutation importance of randomForest regression forests on the device: randomForest(mod.form, data, importance =
// TRUE)'s $importance[, "%IncMSE"] and $importanceSD, what the reference stores as the forest's $var.imp (V73:517-519).
// It is regRF's rule with the randomness made an INPUT, as rf_fit.hip takes its bags and draw seeds: one uint64 per tree
// drives every permutation through the counter-based generator of the fit (fit_mix), so there is no sequential RNG state
// and R's Mersenne-Twister stream is NOT reproduced.  Any randomForest handle will do (mhs_rf_load's or
// mhs_rf_fit_many's): the kernel reads the handle's device-resident 16-byte Node records and tree_off (ensemble_int.h),
// x <= split goes left.
//
// THE RULE, for tree t with seed s_t: O = the rows with inbag[t][i] == 0 in ascending order, m = |O|;
// e0 = sum over O of (pred_t(x_i) - y_i)^2; a variable is USED if some split node of the tree tests it.  For a used
// variable v and k = 0 .. n_perm - 1: h = mix(s_t + k p + v), key_j = mix(h + j), sigma = the stable ascending argsort of
// the keys; row O_j is walked with its x_v replaced by x_v of row O_sigma(j); e_k is the same sum of squares.
// delta[t][v] = (sum_k e_k / n_perm - e0) / m, 0 for an unused variable and for every variable of a tree with m = 0
// (regRF would divide by zero there).  IncMSE_v = sum_t delta[t][v] / n_trees and SD_v = sqrt(max(0, (sum_t delta[t][v]^2
// / n_trees - IncMSE_v^2) / n_trees)).
//
// The work is (trees x used variables x permutations) walks of the out-of-bag rows: ONE WORKGROUP (4 waves) PER TREE,
// all count x n_trees trees in one launch, the dynamic LDS sized by the rows of the call's largest model (16 B per row
// and 16 B per node), so several small trees share a compute unit.  Inside a block:
//
//   1. the out-of-bag rows are compacted in ascending order (ballot / popcount, wave 0);
//   2. the tree's Node records are staged in LDS when they fit (RI_LDS_NODES), read from L2 otherwise;
//   3. the baseline walk gives e0;
//   4. the used-variable mask is the OR over the split nodes (a wave butterfly, the waves combined through LDS);
//   5. per used (v, k): the keys in parallel, the permutation ON CHIP by a bitonic sort of the (key, j) pairs over the
//      next power of two (padding pairs carry the largest key and j >= m, so they end behind every real pair; comparing
//      (key, j) lexicographically IS the stable argsort: the definition is order-free and the result exact), then the walk.
//
// For n <= RI_LDS_ROWS the row list, the keys and the permutation live in LDS; beyond, in a per-tree device scratch (the
// same code and the same arithmetic: only the address space differs).  A second small kernel reduces tree_delta to
// IncMSE and SD IN TREE ORDER.  No floating-point atomics anywhere.
//
// SUMMATION ORDER.  A sum of squares over the out-of-bag rows j = 0 .. m - 1 is taken in 64-row steps: step q holds rows
// 64 q .. 64 q + 63 (lane = j mod 64, absent rows add 0) and is reduced by fit_common.h's xor butterfly; wave w adds the
// steps q = w, w + 4, w + 8, ... to its running sum in that order, and the block's sum is ((wave 0 + wave 1) + wave 2) +
// wave 3.  The e_k of a variable are added in k order.  The order depends on m alone, so a tree's deltas are
// bit-reproducible from call to call and do not depend on which other trees or models share the launch; they equal
// row-by-row sums up to the last bits.
#include <vector>
#include "ensemble_int.h"
#include "fit_common.h"

namespace mhs {

constexpr int RI_T = 256;               // threads of a tree's workgroup
constexpr int RI_W = RI_T / 64;
constexpr int RI_MAXP = 64;             // mhs_rf_load's range: the used-variable mask is one 64-bit word
constexpr int RI_LDS_ROWS = 4096;       // rows whose list (4 B), key (8 B) and permutation (4 B) stay in LDS: a power of two
constexpr int RI_LDS_NODES = 2048;      // Node records (16 B) of a tree staged in LDS
constexpr int RI_MAX_PERM = 16;

struct RiModelDev {
    const double *X, *y;                // n x p column-major, n
    const int *inbag;                   // n_trees x n
    const unsigned long long *seeds;    // n_trees
    const Node *nodes;                  // the handle's
    const int *tree_off;                // n_trees + 1
    int n, pad;
};

struct RiTree {
    long long row_off, key_off;         // into the scratch row lists / the scratch keys and permutations (models beyond RI_LDS_ROWS)
    int model, tree;
};

struct RiWork {
    int *rows, *perm;                   // scratch, per tree n / pow2(n)
    unsigned long long *key;            // scratch, per tree pow2(n)
    double *delta;                      // count x n_trees x p
};

inline int ri_pow2(int64_t v) { int q = 1; while (q < v) q <<= 1; return q; }

// The block's sum of (pred(x_j) - y_j)^2 over the out-of-bag rows rows[0 .. m), row j walked with its x_v replaced by x_v
// of row rows[perm[j]] (v < 0: as it is), in the order the file header states.  Every thread returns the sum; `part`
// is RI_W doubles of LDS.  The whole block calls.
__device__ __forceinline__ double ri_walk_sum(const Node *nd, int nn, const double *__restrict__ X, const double *__restrict__ y, int n,
                                              const int *rows, const int *perm, int m, int v, double *part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int base = wave * 64; base < m; base += RI_T) {
        const int j = base + lane;
        double sq = 0.0;
        if (j < m) {
            const int row = rows[j];
            const int from = v >= 0 ? rows[perm[j]] : row;        // perm[0 .. m) < m: the padding pairs sort behind
            int e = 0;
            Node q = nd[0];
            for (int step = 0; step < nn && q.var >= 0; ++step) {
                const double x = X[(size_t)q.var * n + (q.var == v ? from : row)];
                e = x <= q.val ? q.left : q.right;
                q = nd[e];
            }
            const double d = q.val - y[row];
            sq = d * d;
        }
        s = s + fit_wave_sum(sq);
    }
    __syncthreads();                    // the previous call's readers of part[] are done
    if (lane == 0) part[wave] = s;
    __syncthreads();
    double tot = part[0];
#pragma unroll
    for (int w = 1; w < RI_W; ++w) tot = tot + part[w];
    return tot;
}

__global__ __launch_bounds__(RI_T) void rf_importance_kernel(const RiModelDev *__restrict__ models, const RiTree *__restrict__ trees, RiWork S,
                                                             int p, int n_perm, int lds_rows, int lds_cap, int lds_nodes) {
    extern __shared__ __attribute__((aligned(16))) char ri_dyn[];
    __shared__ double s_part[RI_W];
    __shared__ unsigned long long s_used[RI_W];
    __shared__ int s_m;
    const RiTree T = trees[blockIdx.x];
    const RiModelDev M = models[T.model];
    const int n = M.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- LDS: [node records | keys | row list | permutation], every piece 16-byte aligned
    char *q0 = ri_dyn;
    Node *l_nodes = (Node *)q0;                             q0 += sizeof(Node) * (size_t)lds_nodes;
    unsigned long long *l_key = (unsigned long long *)q0;   q0 += fit_align(sizeof(unsigned long long) * (size_t)lds_cap);
    int *l_rows = (int *)q0;                                q0 += fit_align(sizeof(int) * (size_t)lds_rows);
    int *l_perm = (int *)q0;
    const bool in_lds = n <= lds_rows;
    int *rows = in_lds ? l_rows : S.rows + T.row_off;
    int *perm = in_lds ? l_perm : S.perm + T.key_off;
    unsigned long long *key = in_lds ? l_key : S.key + T.key_off;
    const int *cin = M.inbag + (size_t)T.tree * n;
    const int o = M.tree_off[T.tree], nn = M.tree_off[T.tree + 1] - o;
    double *delta = S.delta + (size_t)blockIdx.x * p;

    // ---- (1) the out-of-bag rows, ascending
    if (wave == 0) {
        const unsigned long long lt = (1ull << lane) - 1ull;
        int at = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const bool f = i < n && cin[i] == 0;
            const unsigned long long bl = __ballot(f);
            if (f) rows[at + __popcll(bl & lt)] = i;
            at += __popcll(bl);
        }
        if (lane == 0) s_m = at;
    }
    // ---- (2) the tree's node records
    const bool staged = nn <= lds_nodes;
    if (staged)
        for (int e = tid; e < nn; e += RI_T) l_nodes[e] = M.nodes[o + e];
    const Node *nd = staged ? l_nodes : M.nodes + o;
    __syncthreads();
    const int m = s_m;
    if (m == 0) {                       // no out-of-bag row: a zero row (the block is uniform here)
        for (int v = tid; v < p; v += RI_T) delta[v] = 0.0;
        return;
    }
    // ---- (3) the baseline
    const double e0 = ri_walk_sum(nd, nn, M.X, M.y, n, rows, perm, m, -1, s_part);
    // ---- (4) the variables the tree tests
    unsigned long long mine = 0ull;
    for (int e = tid; e < nn; e += RI_T) {
        const int var = nd[e].var;
        if (var >= 0) mine |= 1ull << (var & 63);
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) mine |= __shfl_xor(mine, sh);
    if (lane == 0) s_used[wave] = mine;
    __syncthreads();
    unsigned long long used = 0ull;
#pragma unroll
    for (int w = 0; w < RI_W; ++w) used |= s_used[w];
    // ---- (5) every used variable, every permutation
    int P2 = 1;
    while (P2 < m) P2 <<= 1;
    const unsigned long long seed = M.seeds[T.tree];
    for (int v = 0; v < p; ++v) {
        if (!((used >> v) & 1ull)) {
            if (tid == 0) delta[v] = 0.0;
            continue;
        }
        double sum = 0.0;
        for (int k = 0; k < n_perm; ++k) {
            const unsigned long long h = fit_mix(seed + (unsigned long long)k * (unsigned long long)p + (unsigned long long)v);
            // (the previous walk's barriers lie behind its last read of perm[])
            for (int j = tid; j < P2; j += RI_T) {
                key[j] = j < m ? fit_mix(h + (unsigned long long)j) : ~0ull;
                perm[j] = j;
            }
            __syncthreads();
            for (int size = 2; size <= P2; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = tid; i < (P2 >> 1); i += RI_T) {
                        const int lo = i & (stride - 1);
                        const int a = ((i - lo) << 1) + lo, b = a + stride;
                        const unsigned long long ka = key[a], kb = key[b];
                        const int ja = perm[a], jb = perm[b];
                        const bool greater = ka > kb || (ka == kb && ja > jb);
                        if (greater == ((a & size) == 0)) { key[a] = kb; key[b] = ka; perm[a] = jb; perm[b] = ja; }
                    }
                    __syncthreads();
                }
            sum = sum + ri_walk_sum(nd, nn, M.X, M.y, n, rows, perm, m, v, s_part);
        }
        if (tid == 0) delta[v] = (sum / (double)n_perm - e0) / (double)m;
    }
}

// IncMSE and its SD of every variable of every model, trees in order (one thread per model and variable)
__global__ void rf_importance_reduce_kernel(const double *__restrict__ delta, double *__restrict__ inc, double *__restrict__ sd, int count,
                                            int n_trees, int p) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count * p) return;
    const int k = q / p, v = q - k * p;
    const double *d = delta + (size_t)k * n_trees * p + v;
    double s = 0.0, s2 = 0.0;
    for (int t = 0; t < n_trees; ++t) {
        const double x = d[(size_t)t * p];
        s = s + x;
        s2 = s2 + x * x;
    }
    const double mean = s / (double)n_trees;
    const double var = (s2 / (double)n_trees - mean * mean) / (double)n_trees;
    inc[q] = mean;
    sd[q] = sqrt(var > 0.0 ? var : 0.0);
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_rf_importance_many(int count, const mhs_model *const *models, const double *const *X, const double *const *y, const int64_t *n,
                           int p, const int32_t *const *inbag, const uint64_t *const *perm_seeds, int n_perm, double *const *inc_mse,
                           double *const *inc_mse_sd, double *const *tree_delta) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(models && X && y && n && inbag && perm_seeds, "NULL argument");
    if (int rc = fit_check_batch(__func__, count, p, RI_MAXP)) return rc;
    MHS_REQUIRE(n_perm >= 1 && n_perm <= RI_MAX_PERM, "n_perm must be 1..16");
    // ---- checks, and the layout of the uploaded block: every model's inputs, then the model and tree records
    struct Lay { FitPiece<double> X, y; FitPiece<int> inbag; FitPiece<unsigned long long> seeds; };
    std::vector<Lay> lay((size_t)count);
    FitBlock in, work, res;
    int n_trees = 0;
    int64_t n_max = 0;
    for (int k = 0; k < count; ++k) {
        const mhs_model *m = models[k];
        MHS_REQUIRE(m != nullptr && m->kind == K_RF, "not a randomForest handle");
        MHS_REQUIRE(m->p == p, "the forest was built for another number of predictors");
        MHS_REQUIRE(m->device == ctx().device, "the forest lives on another device");
        MHS_REQUIRE(k == 0 || m->n_trees == n_trees, "the forests must have the same number of trees");
        n_trees = m->n_trees;
        MHS_REQUIRE(inbag[k] && perm_seeds[k], "NULL array of a model");
        if (int rc = fit_check_model(__func__, X[k], y[k], n[k], p)) return rc;
        MHS_REQUIRE(n[k] * (int64_t)n_trees < (1LL << 40), "inbag too large");
        const int32_t *cb = inbag[k];
        for (int64_t e = 0; e < n[k] * n_trees; ++e) MHS_REQUIRE(cb[e] >= 0, "negative in-bag count");
        n_max = std::max(n_max, n[k]);
        lay[k].X = in.take<double>((size_t)n[k] * p); lay[k].y = in.take<double>((size_t)n[k]);
        lay[k].inbag = in.take<int>((size_t)n[k] * n_trees); lay[k].seeds = in.take<unsigned long long>((size_t)n_trees);
    }
    MHS_REQUIRE(n_trees >= 1 && (int64_t)count * n_trees < (1LL << 30), "too many trees in one call");
    const size_t NT = (size_t)count * (size_t)n_trees;
    const FitPiece<RiModelDev> mod = in.take<RiModelDev>((size_t)count);
    const FitPiece<RiTree> tree = in.take<RiTree>(NT);
    // the LDS of a block is sized by the rows of the call's largest model (up to RI_LDS_ROWS) and by its largest tree (up to
    // RI_LDS_NODES), so small trees share a compute unit; a model beyond RI_LDS_ROWS gets a scratch per tree
    const int lds_rows = (int)std::min<int64_t>(n_max, RI_LDS_ROWS), lds_cap = ri_pow2(lds_rows);
    hipStream_t s = ctx().stream;
    int max_nodes = 1;
    std::vector<int> toff((size_t)n_trees + 1);
    for (int k = 0; k < count; ++k) {
        MHS_HIP(hipMemcpyAsync(toff.data(), models[k]->tree_off, sizeof(int) * toff.size(), hipMemcpyDeviceToHost, s));
        MHS_HIP(hipStreamSynchronize(s));
        for (int t = 0; t < n_trees; ++t) max_nodes = std::max(max_nodes, toff[(size_t)t + 1] - toff[(size_t)t]);
    }
    const int lds_nodes = std::min(max_nodes, RI_LDS_NODES);
    std::vector<RiTree> ht(NT);
    long long row_total = 0, key_total = 0;
    for (int k = 0; k < count; ++k)
        for (int t = 0; t < n_trees; ++t) {
            RiTree &T = ht[(size_t)k * n_trees + t];
            T.model = k; T.tree = t; T.row_off = row_total; T.key_off = key_total;
            if (n[k] > lds_rows) { row_total += n[k]; key_total += ri_pow2(n[k]); }
        }
    const FitPiece<int> w_rows = work.take<int>((size_t)row_total), w_perm = work.take<int>((size_t)key_total);
    const FitPiece<unsigned long long> w_key = work.take<unsigned long long>((size_t)key_total);
    const FitPiece<double> r_delta = res.take<double>(NT * p), r_inc = res.take<double>((size_t)count * p), r_sd = res.take<double>((size_t)count * p);
    in.mirror(0, in.mark()); res.mirror(0, res.mark());
    MHS_HIP(in.alloc()); MHS_HIP(work.alloc()); MHS_HIP(res.alloc());
    std::copy(ht.begin(), ht.end(), in.host(tree));
    for (int k = 0; k < count; ++k) {
        const Lay &L = lay[k];
        std::copy_n(X[k], (size_t)n[k] * p, in.host(L.X));
        std::copy_n(y[k], (size_t)n[k], in.host(L.y));
        std::copy_n(inbag[k], (size_t)n[k] * n_trees, in.host(L.inbag));
        std::copy_n(perm_seeds[k], (size_t)n_trees, in.host(L.seeds));
        RiModelDev &m = in.host(mod)[k];
        m.X = in.dev(L.X); m.y = in.dev(L.y); m.inbag = in.dev(L.inbag); m.seeds = in.dev(L.seeds);
        m.nodes = models[k]->nodes; m.tree_off = models[k]->tree_off; m.n = (int)n[k]; m.pad = 0;
    }
    RiWork S;
    S.rows = work.dev(w_rows); S.perm = work.dev(w_perm); S.key = work.dev(w_key); S.delta = res.dev(r_delta);
    MHS_HIP(in.upload(0, in.mark(), s));
    const size_t lds_bytes = sizeof(Node) * (size_t)lds_nodes + fit_align(sizeof(unsigned long long) * (size_t)lds_cap) +
                             fit_align(sizeof(int) * (size_t)lds_rows) + fit_align(sizeof(int) * (size_t)lds_cap);
    MHS_HIP(hipFuncSetAttribute((const void *)rf_importance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(rf_importance_kernel, dim3((unsigned)NT), dim3(RI_T), lds_bytes, s, (const RiModelDev *)in.dev(mod),
                       (const RiTree *)in.dev(tree), S, p, n_perm, lds_rows, lds_cap, lds_nodes);
    MHS_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf_importance_reduce_kernel, dim3((unsigned)((count * p + 63) / 64)), dim3(64), 0, s, (const double *)S.delta,
                       res.dev(r_inc), res.dev(r_sd), count, n_trees, p);
    MHS_HIP(hipGetLastError());
    MHS_HIP(res.download(0, res.mark(), s));
    MHS_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < count; ++k) {
        if (inc_mse && inc_mse[k]) std::copy_n(res.host(r_inc) + (size_t)k * p, (size_t)p, inc_mse[k]);
        if (inc_mse_sd && inc_mse_sd[k]) std::copy_n(res.host(r_sd) + (size_t)k * p, (size_t)p, inc_mse_sd[k]);
        if (tree_delta && tree_delta[k]) std::copy_n(res.host(r_delta) + (size_t)k * n_trees * p, (size_t)n_trees * p, tree_delta[k]);
    }
    return MHS_OK;
}

}  // extern "C"
