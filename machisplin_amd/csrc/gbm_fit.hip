// Growing gbm's boosted regression trees on the device (the part cv.py left in the
// package): gbm::gbm / gbm.more as machisplin.gbm.step drives them (V73:1772 the first 50 trees of every fold model,
// V73:1908 gbm.more in the stage loop, V73:2101 the final model), distribution = "gaussian", no weights, no offset,
// train.fraction = 1.  The bag of every tree is an INPUT (the reference draws it from R's RNG); given the bags the
// CART below is deterministic.
//
// The parallelism is across models, not rows: dozens of independent boosting chains (10 CV folds x 10 inner folds,
// V73:247) of a few thousand rows, each a strict sequence of 26-leaf trees.  One launch grows n_new trees for `count`
// models, ONE RESIDENT WORKGROUP (16 waves) per model, no host round trip per tree:
//
//   * the rows are sorted per variable once, on the host (stable: ties in row order);
//   * per tree the sorted orders are compacted to the bag rows (a ballot / popcount pass per variable, a wave per
//     variable), so that every terminal node owns ONE CONTIGUOUS SEGMENT of every variable's order;
//   * a split stable-partitions the parent's segment in every variable's order (ballot / popcount again) -- the two
//     children's segments are again contiguous and sorted;
//   * the split search of a node and a variable is a wave's prefix sum of z over the segment (64 rows per step:
//     Hillis-Steele over the lanes with __shfl_up, plus a carried running sum), the candidate between
//     consecutive distinct values evaluated by the lane that holds the right-hand row; the wave's arg-max takes the
//     LOWEST position among equal improvements, the variables are combined in index order with a strict '>': gbm's
//     "first variable, lowest position" tie-break.  Only the two children just created are searched: every older
//     terminal keeps its cached best split (its rows and z have not changed, so gbm recomputing it gets the same);
//   * z, the bag flag and the left / right mark of every row live in LDS for n <= GF_LDS_ROWS (80 KiB of the 160),
//     in HBM / L2 beyond (same code, same arithmetic: only the address space differs); the orders stay in L2.
//
// SUMMATION ORDER.  gbm adds z row by row along the sorted order; here the left sum at position j is
// (sum of the earlier 64-row steps, added step by step) + (a log-depth lane prefix inside the step).  The chunking
// is fixed (64 rows from the segment's start, whatever else runs), so a model's trees are bit-reproducible from call
// to call and do not depend on which other models share the launch -- but the left sums differ from gbm's sequential
// ones in the last bits, and two candidate splits whose improvements agree to ~1e-13 relative may be ordered
// differently.  Split VALUES are 0.5 * (x_prev + x) of the data and are bit-equal whenever the same candidate wins.
//
// mhs_gbm_grow_many_reduction is the same kernel with one more output: the improvement every split node won with (gbm's
// ErrorReduction, what relative.influence sums per variable), kept in a sixth per-node LDS array and written in the
// stored preorder beside the five node arrays, 0 at terminals.
#include <vector>
#include "fit_common.h"

namespace mhs {

constexpr int GF_T = 1024;              // threads of a model's workgroup
constexpr int GF_W = GF_T / 64;
constexpr int GF_MAXDEPTH = 64;         // interaction.depth (the reference passes tree.complexity = 25, V73:247)
constexpr int GF_MAXP = 64;             // mhs_gbm_load's range
constexpr int GF_NODES = 3 * GF_MAXDEPTH + 1;
constexpr int GF_SLOTS = 2 * GF_MAXDEPTH + 1;
constexpr int GF_LDS_ROWS = 8192;       // rows whose z (8 B) and flags (2 B) stay in LDS

struct GfModel {
    const double *X, *y;                // n x p column-major, n
    double *F;                          // n, in / out
    const int *bags;                    // n_new x bag
    const int *ord;                     // p x n: rows in ascending order of every variable (stable)
    int *idx, *scr;                     // p x bag each: the bag rows in every variable's order, grouped by terminal node
    double *zg;                         // n (rows beyond GF_LDS_ROWS)
    unsigned char *fg;                  // 2 n
    long long *toff;                    // n_new + 1
    int *svar, *left, *right, *miss;    // n_new * (3 depth + 1)
    double *sval;
    double *red;                        // n_new * (3 depth + 1): the improvement of every split node (NULL: not asked for)
    int n, bag;
};

struct GfBest { double imp, ls, sv; int pos, var; };

// Best split of one terminal node along one variable: seg[0 .. m) are the node's bag rows in ascending order of xcol,
// tot the node's sum of z.  Every lane returns the wave's result (imp = 0: none).
__device__ __forceinline__ GfBest gf_search(const int *seg, int m, const double *__restrict__ xcol, const double *z,
                                            double tot, int minobs) {
    const int lane = threadIdx.x & 63;
    double carry = 0.0, xlast = 0.0;
    double bimp = 0.0, bls = 0.0, bsv = 0.0;
    int bpos = 0;
    for (int base = 0; base < m; base += 64) {
        const int j = base + lane;
        const bool ok = j < m;
        const int row = ok ? seg[j] : 0;
        const double zz = ok ? z[row] : 0.0, x = ok ? xcol[row] : 0.0;
        const double inc = fit_wave_scan(zz);
        double pinc = __shfl_up(inc, 1), px = __shfl_up(x, 1);
        if (lane == 0) { pinc = 0.0; px = xlast; }
        if (ok && j >= minobs && m - j >= minobs && j >= 1 && px < x) {
            const double ls = carry + pinc, nl = (double)j, nr = (double)(m - j);
            const double d = ls / nl - (tot - ls) / nr;
            const double imp = nl * nr / (nl + nr) * d * d;
            if (imp > bimp) { bimp = imp; bls = ls; bsv = 0.5 * (px + x); bpos = j; }      // a lane's positions ascend: the lowest stays
        }
        carry = carry + __shfl(inc, 63);
        xlast = __shfl(x, 63);
    }
    GfBest b;
    b.imp = bimp; b.pos = bpos; b.var = -1;
    const int src = fit_wave_argbest(b.imp, b.pos);         // the payload comes from the lane that holds the winner
    b.ls = __shfl(bls, src);
    b.sv = __shfl(bsv, src);
    return b;
}

__global__ __launch_bounds__(GF_T) void gbm_grow_kernel(const GfModel *__restrict__ models, int p, int n_new, int depth, int minobs,
                                                        double shrinkage, int lds_rows) {
    extern __shared__ double gf_dyn[];
    __shared__ int t_node[GF_SLOTS], t_start[GF_SLOTS], t_cnt[GF_SLOTS], b_var[GF_SLOTS], b_pos[GF_SLOTS];
    __shared__ double t_sum[GF_SLOTS], b_imp[GF_SLOTS], b_ls[GF_SLOTS], b_sv[GF_SLOTS];
    __shared__ int n_var[GF_NODES], n_left[GF_NODES], n_right[GF_NODES], n_miss[GF_NODES], n_pre[GF_NODES];
    __shared__ double n_val[GF_NODES];          // split value of an internal node, mean of z (then x shrinkage) of a terminal one
    __shared__ double n_imp[GF_NODES];          // the improvement an internal node was split for (gbm's ErrorReduction), 0 at a terminal one
    __shared__ double r_imp[2 * GF_MAXP], r_ls[2 * GF_MAXP], r_sv[2 * GF_MAXP];
    __shared__ int r_pos[2 * GF_MAXP], s_nterm, s_nnodes;

    const GfModel M = models[blockIdx.x];
    const int n = M.n, B = M.bag, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool in_lds = n <= lds_rows;
    double *z = in_lds ? gf_dyn : M.zg;
    unsigned char *inbag = in_lds ? (unsigned char *)(gf_dyn + lds_rows) : M.fg;
    unsigned char *mark = inbag + n;
    long long node_off = 0;
    if (tid == 0) M.toff[0] = 0;

    for (int t = 0; t < n_new; ++t) {
        // ---- z = y - F, the bag flags
        for (int i = tid; i < n; i += GF_T) { z[i] = M.y[i] - M.F[i]; inbag[i] = 0; }
        __syncthreads();
        for (int b = tid; b < B; b += GF_T) inbag[M.bags[(size_t)t * B + b]] = 1;
        __syncthreads();
        // ---- every variable's order, bag rows only
        for (int v = wave; v < p; v += GF_W) fit_compact_order(M.ord + (size_t)v * n, n, inbag, M.idx + (size_t)v * B, B);
        __syncthreads();
        // ---- root: sum of z over the bag in variable 0's order, 64 rows at a time
        if (wave == 0) {
            double carry = 0.0;
            for (int base = 0; base < B; base += 64) {
                const int j = base + lane;
                carry = carry + __shfl(fit_wave_scan(j < B ? z[M.idx[j]] : 0.0), 63);
            }
            if (lane == 0) {
                t_node[0] = 0; t_start[0] = 0; t_cnt[0] = B; t_sum[0] = carry;
                n_var[0] = -1; n_val[0] = carry / (double)B; n_left[0] = n_right[0] = n_miss[0] = 0; n_imp[0] = 0.0;
                s_nterm = 1; s_nnodes = 1;
            }
        }
        __syncthreads();
        int first = 0, n_search = 1;      // the slots to search: `first` and (n_search == 2) the last but one
        for (int d = 0; d < depth; ++d) {
            // ---- best split of the terminal nodes just created
            const int nterm = s_nterm;
            for (int q = wave; q < n_search * p; q += GF_W) {
                const int c = q / p, v = q - c * p, slot = c == 0 ? first : nterm - 2;
                const GfBest b = gf_search(M.idx + (size_t)v * B + t_start[slot], t_cnt[slot], M.X + (size_t)v * n, z, t_sum[slot], minobs);
                if (lane == 0) { r_imp[q] = b.imp; r_ls[q] = b.ls; r_sv[q] = b.sv; r_pos[q] = b.pos; }
            }
            __syncthreads();
            if (tid < n_search) {
                const int slot = tid == 0 ? first : nterm - 2;
                double bi = 0.0, bl = 0.0, bs = 0.0;
                int bv = -1, bp = 0;
                for (int v = 0; v < p; ++v) {
                    const int q = tid * p + v;
                    if (r_imp[q] > bi) { bi = r_imp[q]; bl = r_ls[q]; bs = r_sv[q]; bp = r_pos[q]; bv = v; }
                }
                b_imp[slot] = bi; b_ls[slot] = bl; b_sv[slot] = bs; b_pos[slot] = bp; b_var[slot] = bv;
            }
            __syncthreads();
            // ---- the terminal node to split: strictly greatest improvement in terminal-list order
            int k = -1;
            double best = 0.0;
            for (int s = 0; s < nterm; ++s)
                if (b_imp[s] > best) { best = b_imp[s]; k = s; }
            if (k < 0) break;
            const int v = b_var[k], nL = b_pos[k], s0 = t_start[k], m = t_cnt[k];
            const double ls = b_ls[k], tot = t_sum[k], sv = b_sv[k];
            {
                const int *seg = M.idx + (size_t)v * B + s0;
                for (int j = tid; j < m; j += GF_T) mark[seg[j]] = j < nL ? 1 : 0;
            }
            __syncthreads();
            // ---- stable partition of the parent's segment in every other variable's order
            for (int u = wave; u < p; u += GF_W)
                if (u != v) fit_partition(M.idx + (size_t)u * B + s0, M.scr + (size_t)u * B + s0, m, nL, mark);
            __syncthreads();
            for (int e = tid; e < p * m; e += GF_T) {
                const int u = e / m, j = e - u * m;
                if (u != v) M.idx[(size_t)u * B + s0 + j] = M.scr[(size_t)u * B + s0 + j];
            }
            if (tid == 0) {
                const int pn = t_node[k], nn = s_nnodes;
                const double pm = n_val[pn];
                n_var[pn] = v; n_val[pn] = sv; n_left[pn] = nn; n_right[pn] = nn + 1; n_miss[pn] = nn + 2; n_imp[pn] = best;
                n_var[nn] = -1; n_val[nn] = ls / (double)nL;
                n_var[nn + 1] = -1; n_val[nn + 1] = (tot - ls) / (double)(m - nL);
                n_imp[nn] = n_imp[nn + 1] = n_imp[nn + 2] = 0.0;
                n_var[nn + 2] = -1; n_val[nn + 2] = pm;                     // no NA in the training rows (V73:154): the parent's mean
                // the left child takes the parent's place in the terminal list, right and missing are appended
                t_node[k] = nn; t_cnt[k] = nL; t_sum[k] = ls;
                t_node[nterm] = nn + 1; t_start[nterm] = s0 + nL; t_cnt[nterm] = m - nL; t_sum[nterm] = tot - ls;
                t_node[nterm + 1] = nn + 2; t_start[nterm + 1] = 0; t_cnt[nterm + 1] = 0; t_sum[nterm + 1] = 0.0;
                b_imp[nterm + 1] = 0.0; b_var[nterm + 1] = -1; b_pos[nterm + 1] = 0; b_ls[nterm + 1] = 0.0; b_sv[nterm + 1] = 0.0;
                s_nnodes = nn + 3; s_nterm = nterm + 2;
            }
            __syncthreads();
            first = k;
            n_search = 2;               // slots k and nterm (= the new s_nterm - 2)
        }
        // ---- terminal values, F, and the tree in gbm's stored order (preorder: node, left, right, missing)
        const int nnodes = s_nnodes;
        __syncthreads();
        for (int e = tid; e < nnodes; e += GF_T)
            if (n_var[e] < 0) n_val[e] = shrinkage * n_val[e];
        __syncthreads();
        for (int i = tid; i < n; i += GF_T) {
            int e = 0;
            while (n_var[e] >= 0) e = M.X[(size_t)n_var[e] * n + i] < n_val[e] ? n_left[e] : n_right[e];
            M.F[i] = M.F[i] + n_val[e];
        }
        if (tid == 0) {
            int stack[GF_MAXDEPTH * 2 + 4], top = 0, cnt = 0;
            stack[top++] = 0;
            while (top > 0) {
                const int e = stack[--top];
                n_pre[e] = cnt++;
                if (n_var[e] >= 0) { stack[top++] = n_miss[e]; stack[top++] = n_right[e]; stack[top++] = n_left[e]; }
            }
        }
        __syncthreads();
        for (int e = tid; e < nnodes; e += GF_T) {
            const long long o = node_off + n_pre[e];
            const bool split = n_var[e] >= 0;
            M.svar[o] = n_var[e]; M.sval[o] = n_val[e];
            M.left[o] = split ? n_pre[n_left[e]] : -1;
            M.right[o] = split ? n_pre[n_right[e]] : -1;
            M.miss[o] = split ? n_pre[n_miss[e]] : -1;
            if (M.red) M.red[o] = split ? n_imp[e] : 0.0;
        }
        node_off += nnodes;
        if (tid == 0) M.toff[t + 1] = node_off;
        __syncthreads();
    }
}

}  // namespace mhs

using namespace mhs;

// Both entry points: `fn` is the name the argument errors carry; error_reduction NULL = mhs_gbm_grow_many.
static int gbm_grow_many(const char *fn, int count, const double *const *X, const double *const *y, const int64_t *n, int p,
                         const int32_t *const *bags, const int64_t *bag_size, int n_new, int interaction_depth, int n_minobsinnode,
                         double shrinkage, int first_call, double *const *F, double *init_f, int64_t *const *tree_offsets,
                         int32_t *const *split_var, double *const *split_val, int32_t *const *left, int32_t *const *right,
                         int32_t *const *missing, double *const *error_reduction) {
    if (int rc = require_ready()) return rc;
    FIT_REQUIRE(X && y && n && bags && bag_size && F && tree_offsets && split_var && split_val && left && right && missing,
                "NULL argument");
    if (int rc = fit_check_batch(fn, count, p, GF_MAXP)) return rc;
    FIT_REQUIRE(n_new >= 1 && n_new < (1 << 24), "n_new out of range");
    FIT_REQUIRE(interaction_depth >= 1 && interaction_depth <= GF_MAXDEPTH, "interaction_depth must be 1..64");
    FIT_REQUIRE(n_minobsinnode >= 1, "n_minobsinnode must be positive");
    FIT_REQUIRE(std::isfinite(shrinkage), "shrinkage is not finite");
    FIT_REQUIRE(!first_call || init_f, "init_f is NULL on the first call");
    const size_t cap = (size_t)n_new * (3 * (size_t)interaction_depth + 1);
    // ---- checks, and the layout of the one device block: [uploaded: inputs, records | F | outputs | work]
    struct Lay { FitPiece<double> X, y, F, sval, zg, red; FitPiece<int> bags, ord, svar, left, right, miss, idx, scr;
                 FitPiece<long long> toff; FitPiece<unsigned char> fg; };
    std::vector<Lay> lay((size_t)count);
    FitBlock blk;
    int64_t n_max = 0;
    for (int k = 0; k < count; ++k) {
        FIT_REQUIRE(bags[k] && F[k] && tree_offsets[k] && split_var[k] && split_val[k] && left[k] && right[k] && missing[k],
                    "NULL array of a model");
        if (int rc = fit_check_model(fn, X[k], y[k], n[k], p)) return rc;
        FIT_REQUIRE(bag_size[k] >= 1 && bag_size[k] <= n[k], "bag_size must be between 1 and n");
        n_max = std::max(n_max, n[k]);
        lay[k].X = blk.take<double>((size_t)n[k] * p); lay[k].y = blk.take<double>((size_t)n[k]);
        lay[k].bags = blk.take<int>((size_t)n_new * (size_t)bag_size[k]); lay[k].ord = blk.take<int>((size_t)n[k] * p);
    }
    const FitPiece<GfModel> mod = blk.take<GfModel>((size_t)count);
    const size_t in_end = blk.mark();
    for (int k = 0; k < count; ++k) lay[k].F = blk.take<double>((size_t)n[k]);
    const size_t up_end = blk.mark();
    for (int k = 0; k < count; ++k) {
        lay[k].toff = blk.take<long long>((size_t)n_new + 1);
        lay[k].sval = blk.take<double>(cap); lay[k].svar = blk.take<int>(cap);
        lay[k].left = blk.take<int>(cap); lay[k].right = blk.take<int>(cap); lay[k].miss = blk.take<int>(cap);
    }
    const auto wants_red = [&](int k) { return error_reduction && error_reduction[k]; };
    for (int k = 0; k < count; ++k)
        if (wants_red(k)) lay[k].red = blk.take<double>(cap);
    const size_t down_end = blk.mark();
    for (int k = 0; k < count; ++k) {
        lay[k].idx = blk.take<int>((size_t)bag_size[k] * p); lay[k].scr = blk.take<int>((size_t)bag_size[k] * p);
        lay[k].zg = blk.take<double>((size_t)n[k]); lay[k].fg = blk.take<unsigned char>(2 * (size_t)n[k]);
    }
    blk.mirror(0, up_end, down_end - in_end);       // the same bytes take [F | outputs] home
    MHS_HIP(blk.alloc());
    for (int k = 0; k < count; ++k) {
        const Lay &L = lay[k];
        const int64_t nk = n[k], bk = bag_size[k];
        double *hF = blk.host(L.F); int *hb = blk.host(L.bags);
        std::copy_n(X[k], (size_t)nk * p, blk.host(L.X));
        std::copy_n(y[k], (size_t)nk, blk.host(L.y));
        double sum = 0.0;
        for (int64_t i = 0; i < nk; ++i) sum += y[k][i];
        if (first_call) {
            init_f[k] = sum / (double)nk;
            for (int64_t i = 0; i < nk; ++i) hF[i] = init_f[k];
        } else {
            for (int64_t i = 0; i < nk; ++i) { FIT_REQUIRE(std::isfinite(F[k][i]), "non-finite F"); hF[i] = F[k][i]; }
        }
        std::vector<int> stamp((size_t)nk, -1);
        for (int t = 0; t < n_new; ++t)
            for (int64_t b = 0; b < bk; ++b) {
                const int32_t r = bags[k][(size_t)t * bk + b];
                FIT_REQUIRE(r >= 0 && r < nk, "bag index out of range");
                FIT_REQUIRE(stamp[(size_t)r] != t, "a row appears twice in one bag (gbm samples without replacement)");
                stamp[(size_t)r] = t;
                hb[(size_t)t * bk + b] = r;
            }
        fit_sorted_orders(X[k], nk, p, blk.host(L.ord));
        GfModel &m = blk.host(mod)[k];
        m.X = blk.dev(L.X); m.y = blk.dev(L.y); m.F = blk.dev(L.F); m.bags = blk.dev(L.bags); m.ord = blk.dev(L.ord);
        m.idx = blk.dev(L.idx); m.scr = blk.dev(L.scr); m.zg = blk.dev(L.zg); m.fg = blk.dev(L.fg);
        m.toff = blk.dev(L.toff); m.sval = blk.dev(L.sval); m.svar = blk.dev(L.svar);
        m.left = blk.dev(L.left); m.right = blk.dev(L.right); m.miss = blk.dev(L.miss);
        m.red = wants_red(k) ? blk.dev(L.red) : nullptr;
        m.n = (int)nk; m.bag = (int)bk;
    }
    hipStream_t s = ctx().stream;
    MHS_HIP(blk.upload(0, up_end, s));
    const int lds_rows = (int)std::min<int64_t>(n_max, GF_LDS_ROWS);
    const size_t lds_bytes = fit_align((size_t)lds_rows * 10);
    MHS_HIP(hipFuncSetAttribute((const void *)gbm_grow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(gbm_grow_kernel, dim3((unsigned)count), dim3(GF_T), lds_bytes, s, (const GfModel *)blk.dev(mod), p, n_new,
                       interaction_depth, n_minobsinnode, shrinkage, lds_rows);
    MHS_HIP(hipGetLastError());
    blk.mirror(in_end, down_end);
    MHS_HIP(blk.download(in_end, down_end, s));
    MHS_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < count; ++k) {
        const Lay &L = lay[k];
        std::copy_n(blk.host(L.F), (size_t)n[k], F[k]);
        const long long *to = blk.host(L.toff);
        for (int t = 0; t <= n_new; ++t) tree_offsets[k][t] = (int64_t)to[t];
        const size_t nn = (size_t)to[n_new];
        if (nn > cap) { set_error("%s: node count exceeds its bound", fn); return MHS_ERR_NUMERIC; }
        std::copy_n(blk.host(L.sval), nn, split_val[k]);
        std::copy_n(blk.host(L.svar), nn, split_var[k]);
        std::copy_n(blk.host(L.left), nn, left[k]);
        std::copy_n(blk.host(L.right), nn, right[k]);
        std::copy_n(blk.host(L.miss), nn, missing[k]);
        if (wants_red(k)) std::copy_n(blk.host(L.red), nn, error_reduction[k]);
    }
    return MHS_OK;
}

extern "C" {

int mhs_gbm_grow_many(int count, const double *const *X, const double *const *y, const int64_t *n, int p,
                      const int32_t *const *bags, const int64_t *bag_size, int n_new, int interaction_depth,
                      int n_minobsinnode, double shrinkage, int first_call, double *const *F, double *init_f,
                      int64_t *const *tree_offsets, int32_t *const *split_var, double *const *split_val,
                      int32_t *const *left, int32_t *const *right, int32_t *const *missing) {
    return gbm_grow_many(__func__, count, X, y, n, p, bags, bag_size, n_new, interaction_depth, n_minobsinnode, shrinkage, first_call, F,
                         init_f, tree_offsets, split_var, split_val, left, right, missing, nullptr);
}

int mhs_gbm_grow_many_reduction(int count, const double *const *X, const double *const *y, const int64_t *n, int p,
                                const int32_t *const *bags, const int64_t *bag_size, int n_new, int interaction_depth,
                                int n_minobsinnode, double shrinkage, int first_call, double *const *F, double *init_f,
                                int64_t *const *tree_offsets, int32_t *const *split_var, double *const *split_val,
                                int32_t *const *left, int32_t *const *right, int32_t *const *missing,
                                double *const *error_reduction) {
    return gbm_grow_many(__func__, count, X, y, n, p, bags, bag_size, n_new, interaction_depth, n_minobsinnode, shrinkage, first_call, F,
                         init_f, tree_offsets, split_var, split_val, left, right, missing, error_reduction);
}

}  // extern "C"
