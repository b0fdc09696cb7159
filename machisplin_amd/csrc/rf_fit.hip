// Growing randomForest's regression forests on the device: randomForest::randomForest(mod.form, data = train) as the
// reference calls it eleven times per layer (V73:248 once per CV fold, V73:517 the final model) with the package's
// defaults -- ntree = 500, mtry = max(floor(p / 3), 1), nodesize = 5, a bootstrap of n rows with replacement, numeric
// predictors, no NA in the training rows (V73:154).  The randomness is an INPUT, as gbm's bags are in gbm_fit.hip:
// inbag[t][i] says how many times row i is in tree t's bootstrap (a row with count c weighs c in every sum and every
// population count: the same tree as duplicating the row, because no candidate lies between equal values), and one
// uint64 seed per tree drives the per-node variable draw through a counter-based generator (fit_mix / rf_draw below), so
// the growth carries no sequential RNG state.  R's Mersenne-Twister stream is NOT reproduced: the forest is
// randomForest's for these bags and draws, not for R's set.seed (the caveat of Gbm.fit).  The modulo bias of the draw
// is accepted (p <= 64).  The RANDOM tie-break between equal criteria of recent randomForest releases is not
// reproduced either: ties go to the lowest position within a variable and to the first drawn variable.  Permutation
// importance (importance = TRUE's %IncMSE) takes its randomness from the caller in the same way: rf_importance.hip.
//
// The parallelism is across trees: a forest is n_trees INDEPENDENT CARTs, and the ten fold forests of a layer are
// 5 000 of them.  One launch grows all count x n_trees trees, ONE WORKGROUP (4 waves) PER TREE; the dynamic LDS is sized
// by the rows (13 B per row), so several small trees share a compute unit:
//
//   * the rows are sorted per variable once per model, on the host (stable: ties in row order);
//   * per tree the sorted orders are compacted to the in-bag rows (ballot / popcount, a wave per variable), so that every
//     node owns ONE CONTIGUOUS SEGMENT of every variable's order;
//   * the tree grows LEVEL BY LEVEL.  Nodes are numbered in creation order and a level is a contiguous index range; the
//     children of a level's splitting nodes get the next free indices in the order of their parents (a ballot / popcount
//     scan over the level), which is exactly the numbering of processing the nodes one by one in index order;
//   * per level: (1) every node's population, sum and prediction from its own segment, a wave per node; (2) the split
//     search, the level's (node, drawn variable) pairs spread over the waves in batches of RF_PAIRS -- a wave's weighted
//     prefix scan of c y and of c over the segment, the candidate between consecutive distinct values evaluated by the
//     lane that holds the right-hand row, criterion sl^2 / nl + sr^2 / nr - tot^2 / m, the wave's arg-max taking the
//     LOWEST position among equal criteria -- and the pairs of a node combined in draw order with a strict '>';
//     (3) the numbering; (4) the left / right marks of the splitting nodes' rows; (5) a stable partition of every
//     splitting node's segment in every variable's order (ballot / popcount) from one index buffer into the other, the
//     two buffers changing roles from level to level.  Depth is unbounded: growth ends with an empty level;
//   * y, the counts and the marks live in LDS for n <= RF_LDS_ROWS (104 KiB of the 160), in HBM / L2 beyond (the same
//     code and the same arithmetic: only the address space differs); the orders stay in L2;
//   * node arrays go straight to a worst-case slab per tree in device memory (2 distinct - 1 nodes); a second small
//     kernel compacts the slabs into mhs_rf_load's layout, and the host hands them to mhs_rf_load;
//   * the out-of-bag rows of a tree walk it at the end of the block; the per-tree predictions and the per-tree sums of
//     the winning criteria are reduced IN TREE ORDER by a small kernel (no floating-point atomics anywhere).
//
// SUMMATION ORDER.  A sequential implementation adds c y row by row along the sorted order; here the left sum at position
// j is (the sum of the earlier 64-row steps, added step by step) + (a log-depth lane prefix inside the step), a node's
// total is (64-row steps of its segment in variable 0's order, each reduced by an xor butterfly, added step by step), a
// tree's IncNodePurity term is the same over its nodes in index order, and the forest reductions run in tree order.
// The chunking is fixed by the segment alone, so a tree is bit-reproducible from call to call and does not depend on
// which other trees or models share the launch -- but the sums differ from sequential ones in the last bits, and two
// candidates whose criteria agree to ~1e-13 relative may be ordered differently (with nodesize 5 small nodes offer
// such pairs all the time: two variables that cut off the same rows).  Split VALUES are 0.5 (a + b) of the data (or a)
// and are bit-equal whenever the same candidate wins.
#include <vector>
#include "ensemble_int.h"
#include "fit_common.h"

namespace mhs {

constexpr int RF_T = 256;               // threads of a tree's workgroup
constexpr int RF_W = RF_T / 64;
constexpr int RF_MAXP = 64;             // mhs_rf_load's range
constexpr int RF_LDS_ROWS = 8192;       // rows whose y (8 B), count (4 B) and mark (1 B) stay in LDS
constexpr int RF_PAIRS = 256;           // (node, drawn variable) pairs searched between two barriers

struct RfModelDev {
    const double *X, *y;                // n x p column-major, n
    const int *ord;                     // p x n: rows in ascending order of every variable (stable)
    const int *inbag;                   // n_trees x n
    const unsigned long long *seeds;    // n_trees
    double *oob_pred;                   // n
    int *oob_count;                     // n
    double *purity;                     // p
    long long row_base;                 // first row of the model's first tree in the per-tree row buffers
    int n, first_tree;
};

struct RfTree {
    long long idx_off, node_off, row_off, out_off;      // into the index buffers, the node slabs, the row buffers, the compacted arrays
    int model, tree, distinct, pad;
};

struct RfWork {
    int *idx, *scr;                                     // per tree p x distinct: the in-bag rows in every variable's order, grouped by node
    int *left, *right, *var, *start, *cnt, *pop;        // node slabs (children 0-based, var -1 = terminal)
    double *split, *pred, *tot, *crit;
    double *oob;                                        // per tree n: its prediction for its out-of-bag rows
    unsigned char *mark;                                // per tree n (rows beyond RF_LDS_ROWS)
    double *purity;                                     // per tree p
    int *n_nodes, *flag;                                // per tree
};

// The j-th drawn variable of node k of a tree with seed `seed`: ind[] lives one entry per lane (p <= 64).  Every lane
// returns the same value.
__device__ __forceinline__ int rf_draw(unsigned long long seed, int k, int j, int p) {
    const int lane = threadIdx.x & 63;
    const unsigned long long h = fit_mix(seed + (unsigned long long)k);
    int ind = lane, last = p - 1, take = 0;
    for (int s = 0; s <= j; ++s) {
        const int i = (int)(fit_mix(h + (unsigned long long)s) % (unsigned long long)(last + 1));
        take = __shfl(ind, i);
        const int moved = __shfl(ind, last);
        if (lane == i) ind = moved;
        --last;
    }
    return take;
}

struct RfBest { double crit, sv; int pos; };

// Best split of one node along one variable: seg[0 .. m) are the node's in-bag rows in ascending order of xcol, tot its
// sum of c y, pop its population.  Every lane returns the wave's result (crit = 0: none).
__device__ __forceinline__ RfBest rf_search(const int *seg, int m, const double *__restrict__ xcol, const double *y, const int *c,
                                            double tot, int pop) {
    const int lane = threadIdx.x & 63;
    const double whole = tot * tot / (double)pop;
    double carry = 0.0, xlast = 0.0;
    int ccarry = 0;
    double bcrit = 0.0, bsv = 0.0;
    int bpos = 0;
    for (int base = 0; base < m; base += 64) {
        const int j = base + lane;
        const bool ok = j < m;
        const int row = ok ? seg[j] : 0;
        const int cc = ok ? c[row] : 0;
        const double x = ok ? xcol[row] : 0.0;
        const double inc = fit_wave_scan(ok ? (double)cc * y[row] : 0.0);
        const int ic = fit_wave_scan(cc);
        double pinc = __shfl_up(inc, 1), px = __shfl_up(x, 1);
        int pic = __shfl_up(ic, 1);
        if (lane == 0) { pinc = 0.0; pic = 0; px = xlast; }
        if (ok && j >= 1 && px < x) {
            const double sl = carry + pinc, sr = tot - sl;
            const int il = ccarry + pic;
            const double nl = (double)il, nr = (double)(pop - il);
            const double crit = sl * sl / nl + sr * sr / nr - whole;
            if (crit > bcrit) {                                     // a lane's positions ascend: the lowest stays
                const double mid = 0.5 * (px + x);
                bcrit = crit; bpos = j; bsv = mid < x ? mid : px;
            }
        }
        carry = carry + __shfl(inc, 63);
        ccarry += __shfl(ic, 63);
        xlast = __shfl(x, 63);
    }
    RfBest b;
    b.crit = bcrit; b.pos = bpos;
    b.sv = __shfl(bsv, fit_wave_argbest(b.crit, b.pos));           // the payload comes from the lane that holds the winner
    return b;
}

__global__ __launch_bounds__(RF_T) void rf_grow_kernel(const RfModelDev *__restrict__ models, const RfTree *__restrict__ trees, RfWork S,
                                                       int p, int mtry, int nodesize, int lds_rows) {
    extern __shared__ __attribute__((aligned(16))) char rf_dyn[];
    const RfTree T = trees[blockIdx.x];
    const RfModelDev M = models[T.model];
    const int n = M.n, B = T.distinct, cap = 2 * B - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    // ---- LDS: [y | counts | marks | the pair results | the level's state], every piece 16-byte aligned
    char *q0 = rf_dyn;
    double *ly = (double *)q0;                  q0 += fit_align(sizeof(double) * (size_t)lds_rows);
    int *lc = (int *)q0;                        q0 += fit_align(sizeof(int) * (size_t)lds_rows);
    unsigned char *lm = (unsigned char *)q0;    q0 += fit_align((size_t)lds_rows);
    double *r_crit = (double *)q0;              q0 += sizeof(double) * RF_PAIRS;
    double *r_sv = (double *)q0;                q0 += sizeof(double) * RF_PAIRS;
    int *r_pos = (int *)q0;                     q0 += sizeof(int) * RF_PAIRS;
    int *r_var = (int *)q0;                     q0 += sizeof(int) * RF_PAIRS;
    int *s_lev = (int *)q0;                     // level begin, level end (= nodes so far)
    const bool in_lds = n <= lds_rows;
    const int *cin = M.inbag + (size_t)T.tree * n;
    const double *y = in_lds ? ly : M.y;
    const int *c = in_lds ? lc : cin;
    unsigned char *mark = in_lds ? lm : S.mark + T.row_off;
    const unsigned long long seed = M.seeds[T.tree];
    int *left = S.left + T.node_off, *right = S.right + T.node_off, *var = S.var + T.node_off, *start = S.start + T.node_off;
    int *cnt = S.cnt + T.node_off, *pop = S.pop + T.node_off;
    double *split = S.split + T.node_off, *pred = S.pred + T.node_off, *tot = S.tot + T.node_off, *crit = S.crit + T.node_off;
    int *cur = S.idx + T.idx_off, *oth = S.scr + T.idx_off;

    if (in_lds)
        for (int i = tid; i < n; i += RF_T) { ly[i] = M.y[i]; lc[i] = cin[i]; }
    if (tid == 0) { start[0] = 0; cnt[0] = B; s_lev[0] = 0; s_lev[1] = 1; }
    __syncthreads();
    // ---- every variable's order, in-bag rows only
    for (int v = wave; v < p; v += RF_W) fit_compact_order(M.ord + (size_t)v * n, n, c, cur + (size_t)v * B, B);
    __syncthreads();
    const int per_batch = RF_PAIRS / mtry;          // nodes of a level searched between two barriers
    for (;;) {
        const int lb = s_lev[0], le = s_lev[1];
        if (lb >= le) break;
        // ---- (1) population, sum and prediction of every node of the level, from its segment in variable 0's order
        for (int k = lb + wave; k < le; k += RF_W) {
            const int *seg = cur + start[k];
            const int m = cnt[k];
            double s = 0.0;
            int w = 0;
            for (int base = 0; base < m; base += 64) {
                const int j = base + lane;
                const int row = j < m ? seg[j] : 0;
                const int cc = j < m ? c[row] : 0;
                s = s + fit_wave_sum(j < m ? (double)cc * y[row] : 0.0);
                w += fit_wave_sum(cc);
            }
            if (lane == 0) {
                pop[k] = w; tot[k] = s; pred[k] = s / (double)w;
                var[k] = -1; left[k] = 0; right[k] = 0; split[k] = 0.0; crit[k] = 0.0;
            }
        }
        __syncthreads();
        // ---- (2) the split search: the level's (node, drawn variable) pairs over the waves
        for (int b0 = lb; b0 < le; b0 += per_batch) {
            const int nb = min(per_batch, le - b0);
            for (int q = wave; q < nb * mtry; q += RF_W) {
                const int kk = q / mtry, j = q - kk * mtry, k = b0 + kk;
                const int m = cnt[k], w = pop[k];
                RfBest b;
                b.crit = 0.0; b.sv = 0.0; b.pos = 0;
                int v = -1;
                if ((k == 0 || w > nodesize) && m >= 2) {
                    v = rf_draw(seed, k, j, p);
                    b = rf_search(cur + (size_t)v * B + start[k], m, M.X + (size_t)v * n, y, c, tot[k], w);
                }
                if (lane == 0) { r_crit[q] = b.crit; r_sv[q] = b.sv; r_pos[q] = b.pos; r_var[q] = v; }
            }
            __syncthreads();
            if (tid < nb) {
                const int k = b0 + tid;
                double bc = 0.0, bs = 0.0;
                int bv = -1, bp = 0;
                for (int j = 0; j < mtry; ++j) {
                    const int q = tid * mtry + j;
                    if (r_crit[q] > bc) { bc = r_crit[q]; bs = r_sv[q]; bp = r_pos[q]; bv = r_var[q]; }
                }
                if (bv >= 0) { var[k] = bv; split[k] = bs; crit[k] = bc; left[k] = bp; }       // left: the rows that go left, until (3)
            }
            __syncthreads();
        }
        // ---- (3) the children's numbers: the next free indices, in the order of their parents
        if (wave == 0) {
            int made = 0;
            for (int base = lb; base < le; base += 64) {
                const int k = base + lane;
                bool sp = k < le && var[k] >= 0;
                const unsigned long long bl = __ballot(sp);
                const int c0 = le + 2 * (made + __popcll(bl & lt));
                if (sp && c0 + 1 >= cap) {        // cannot happen (every child holds a distinct row)
                    S.flag[blockIdx.x] = 1; var[k] = -1; sp = false;
                }
                if (sp) {
                    const int nl = left[k], s0 = start[k], m = cnt[k];
                    left[k] = c0; right[k] = c0 + 1;
                    start[c0] = s0; cnt[c0] = nl;
                    start[c0 + 1] = s0 + nl; cnt[c0 + 1] = m - nl;
                }
                made += __popcll(bl);
            }
            if (lane == 0) { s_lev[0] = le; s_lev[1] = min(le + 2 * made, cap); }
        }
        __syncthreads();
        // ---- (4) the marks of the splitting nodes' rows
        for (int k = lb + wave; k < le; k += RF_W) {
            if (var[k] < 0) continue;
            const int *seg = cur + (size_t)var[k] * B + start[k];
            const int m = cnt[k], nl = cnt[left[k]];
            for (int j = lane; j < m; j += 64) mark[seg[j]] = j < nl ? 1 : 0;
        }
        __syncthreads();
        // ---- (5) stable partition of every splitting node's segment in every variable's order
        for (int q = wave; q < (le - lb) * p; q += RF_W) {
            const int kk = q / p, u = q - kk * p, k = lb + kk;
            if (var[k] < 0) continue;
            const size_t at = (size_t)u * B + start[k];
            fit_partition(cur + at, oth + at, cnt[k], cnt[left[k]], mark);
        }
        __syncthreads();
        int *sw = cur; cur = oth; oth = sw;
    }
    const int nn = s_lev[1];
    if (tid == 0) S.n_nodes[blockIdx.x] = nn;
    // ---- the tree's prediction for its out-of-bag rows
    double *oob = S.oob + T.row_off;
    for (int i = tid; i < n; i += RF_T) {
        if (c[i] != 0) continue;
        int e = 0;
        for (int step = 0; step < nn && var[e] >= 0; ++step) e = M.X[(size_t)var[e] * n + i] <= split[e] ? left[e] : right[e];
        oob[i] = pred[e];
    }
    // ---- the winning criteria summed per variable, nodes in index order
    for (int v = wave; v < p; v += RF_W) {
        double s = 0.0;
        for (int base = 0; base < nn; base += 64) {
            const int k = base + lane;
            s = s + fit_wave_sum(k < nn && var[k] == v ? crit[k] : 0.0);
        }
        if (lane == 0) S.purity[(size_t)blockIdx.x * p + v] = s;
    }
}

// tree_offsets of every model: a running sum over its trees (one thread per model)
__global__ void rf_offsets_kernel(const int *__restrict__ n_nodes, long long *__restrict__ toff, int count, int n_trees) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    long long at = 0;
    toff[(size_t)k * (n_trees + 1)] = 0;
    for (int t = 0; t < n_trees; ++t) {
        at += n_nodes[(size_t)k * n_trees + t];
        toff[(size_t)k * (n_trees + 1) + t + 1] = at;
    }
}

// the slabs -> mhs_rf_load's layout (one block per tree)
__global__ void rf_compact_kernel(const RfTree *__restrict__ trees, RfWork S, const long long *__restrict__ toff, int n_trees,
                                  int *__restrict__ o_left, int *__restrict__ o_right, int *__restrict__ o_status, int *__restrict__ o_var,
                                  double *__restrict__ o_split, double *__restrict__ o_pred) {
    const RfTree T = trees[blockIdx.x];
    const int nn = S.n_nodes[blockIdx.x];
    const long long o = T.out_off + toff[(size_t)T.model * (n_trees + 1) + T.tree];
    for (int e = threadIdx.x; e < nn; e += blockDim.x) {
        const long long s = T.node_off + e;
        const bool sp = S.var[s] >= 0;
        o_left[o + e] = sp ? S.left[s] + 1 : 0;
        o_right[o + e] = sp ? S.right[s] + 1 : 0;
        o_status[o + e] = sp ? -3 : -1;
        o_var[o + e] = sp ? S.var[s] + 1 : 0;
        o_split[o + e] = sp ? S.split[s] : 0.0;
        o_pred[o + e] = S.pred[s];
    }
}

// out-of-bag mean of every row (trees in order) and IncNodePurity of every variable (trees in order)
__global__ void rf_reduce_kernel(const RfModelDev *__restrict__ models, RfWork S, int p, int n_trees) {
    const RfModelDev M = models[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M.n) {
        double s = 0.0;
        int w = 0;
        for (int t = 0; t < n_trees; ++t)
            if (M.inbag[(size_t)t * M.n + i] == 0) { s = s + S.oob[M.row_base + (long long)t * M.n + i]; ++w; }
        M.oob_pred[i] = w ? s / (double)w : NAN;
        M.oob_count[i] = w;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < p) {
        double s = 0.0;
        for (int t = 0; t < n_trees; ++t) s = s + S.purity[(size_t)(M.first_tree + t) * p + threadIdx.x];
        M.purity[threadIdx.x] = s / (double)n_trees;
    }
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_rf_fit_many(int count, const double *const *X, const double *const *y, const int64_t *n, int p, int n_trees, int mtry,
                    int nodesize, const int32_t *const *inbag, const uint64_t *const *seeds, mhs_model **models_out,
                    double *const *oob_pred, int32_t *const *oob_count, double *const *inc_node_purity) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(X && y && n && inbag && seeds && models_out, "NULL argument");
    if (int rc = fit_check_batch(__func__, count, p, RF_MAXP)) return rc;
    MHS_REQUIRE(n_trees >= 1 && n_trees < (1 << 20), "n_trees out of range");
    MHS_REQUIRE(mtry >= 1 && mtry <= p, "mtry must be 1..p");
    MHS_REQUIRE(nodesize >= 1, "nodesize must be positive");
    MHS_REQUIRE((int64_t)count * n_trees < (1LL << 30), "too many trees in one call");
    for (int k = 0; k < count; ++k) models_out[k] = nullptr;
    // ---- checks, and the layout of the uploaded block: every model's inputs, then the model and tree records
    struct Lay { FitPiece<double> X, y; FitPiece<int> ord, inbag; FitPiece<unsigned long long> seeds; };
    std::vector<Lay> lay((size_t)count);
    const size_t NT = (size_t)count * (size_t)n_trees;
    std::vector<RfTree> ht(NT);
    std::vector<long long> out_base((size_t)count + 1, 0), res_off((size_t)count + 1, 0);
    FitBlock in, work, res;
    long long idx_total = 0, node_total = 0, row_total = 0;
    int64_t n_max = 0;
    for (int k = 0; k < count; ++k) {
        MHS_REQUIRE(inbag[k] && seeds[k], "NULL array of a model");
        if (int rc = fit_check_model(__func__, X[k], y[k], n[k], p)) return rc;
        const int64_t nk = n[k];
        n_max = std::max(n_max, nk);
        lay[k].X = in.take<double>((size_t)nk * p); lay[k].y = in.take<double>((size_t)nk); lay[k].ord = in.take<int>((size_t)nk * p);
        lay[k].inbag = in.take<int>((size_t)nk * n_trees); lay[k].seeds = in.take<unsigned long long>((size_t)n_trees);
        long long out_nodes = 0;
        for (int t = 0; t < n_trees; ++t) {
            const int32_t *cb = inbag[k] + (size_t)t * nk;
            int64_t distinct = 0, popl = 0;
            for (int64_t i = 0; i < nk; ++i) {
                MHS_REQUIRE(cb[i] >= 0, "negative in-bag count");
                distinct += cb[i] > 0; popl += cb[i];
            }
            MHS_REQUIRE(distinct >= 1, "a tree whose in-bag counts are all zero");
            MHS_REQUIRE(popl < (1LL << 31), "a tree's in-bag counts sum to 2^31 or more");
            RfTree &T = ht[(size_t)k * n_trees + t];
            T.model = k; T.tree = t; T.distinct = (int)distinct; T.pad = 0;
            T.idx_off = idx_total; idx_total += distinct * p;
            T.node_off = node_total; node_total += 2 * distinct - 1;
            T.row_off = row_total; row_total += nk;
            T.out_off = out_base[k];
            out_nodes += 2 * distinct - 1;
        }
        out_base[k + 1] = out_base[k] + out_nodes;
        res_off[k + 1] = res_off[k] + nk;
    }
    const size_t NN = (size_t)node_total, NR = (size_t)row_total, NO = (size_t)out_base[count], NS = (size_t)res_off[count];
    const FitPiece<RfModelDev> mod = in.take<RfModelDev>((size_t)count);
    const FitPiece<RfTree> tree = in.take<RfTree>(NT);
    // ---- the other two blocks: [work: index buffers, node slabs, per-tree rows] and [results: what comes home at once | compacted arrays]
    const FitPiece<int> w_idx = work.take<int>((size_t)idx_total), w_scr = work.take<int>((size_t)idx_total);
    FitPiece<int> w_int[6], r_int[4];
    FitPiece<double> w_dbl[4], r_dbl[2];
    for (auto &a : w_int) a = work.take<int>(NN);
    for (auto &a : w_dbl) a = work.take<double>(NN);
    const FitPiece<double> w_oob = work.take<double>(NR);
    const FitPiece<unsigned char> w_mark = work.take<unsigned char>(NR);
    const FitPiece<double> w_pur = work.take<double>(NT * p);
    const FitPiece<int> w_nn = work.take<int>(NT), w_flag = work.take<int>(NT);
    const FitPiece<long long> r_toff = res.take<long long>((size_t)count * ((size_t)n_trees + 1));
    const FitPiece<int> r_flag = res.take<int>(NT);
    const FitPiece<double> r_oobp = res.take<double>(NS);
    const FitPiece<int> r_oobc = res.take<int>(NS);
    const FitPiece<double> r_pur = res.take<double>((size_t)count * p);
    const size_t small_end = res.mark();
    for (auto &a : r_int) a = res.take<int>(NO);
    for (auto &a : r_dbl) a = res.take<double>(NO);
    in.mirror(0, in.mark()); res.mirror(0, small_end);
    MHS_HIP(in.alloc()); MHS_HIP(work.alloc()); MHS_HIP(res.alloc());
    std::copy(ht.begin(), ht.end(), in.host(tree));
    for (int k = 0; k < count; ++k) {
        const Lay &L = lay[k];
        const int64_t nk = n[k];
        std::copy_n(X[k], (size_t)nk * p, in.host(L.X));
        std::copy_n(y[k], (size_t)nk, in.host(L.y));
        std::copy_n(inbag[k], (size_t)nk * n_trees, in.host(L.inbag));
        std::copy_n(seeds[k], (size_t)n_trees, in.host(L.seeds));
        fit_sorted_orders(X[k], nk, p, in.host(L.ord));
        RfModelDev &m = in.host(mod)[k];
        m.X = in.dev(L.X); m.y = in.dev(L.y); m.ord = in.dev(L.ord); m.inbag = in.dev(L.inbag); m.seeds = in.dev(L.seeds);
        m.oob_pred = res.dev(r_oobp) + res_off[k]; m.oob_count = res.dev(r_oobc) + res_off[k];
        m.purity = res.dev(r_pur) + (size_t)k * p;
        m.row_base = ht[(size_t)k * n_trees].row_off; m.n = (int)nk; m.first_tree = k * n_trees;
    }
    RfWork S;
    S.idx = work.dev(w_idx); S.scr = work.dev(w_scr);
    S.left = work.dev(w_int[0]); S.right = work.dev(w_int[1]); S.var = work.dev(w_int[2]);
    S.start = work.dev(w_int[3]); S.cnt = work.dev(w_int[4]); S.pop = work.dev(w_int[5]);
    S.split = work.dev(w_dbl[0]); S.pred = work.dev(w_dbl[1]); S.tot = work.dev(w_dbl[2]); S.crit = work.dev(w_dbl[3]);
    S.oob = work.dev(w_oob); S.mark = work.dev(w_mark); S.purity = work.dev(w_pur);
    S.n_nodes = work.dev(w_nn); S.flag = work.dev(w_flag);
    const RfModelDev *dmod = in.dev(mod); const RfTree *dtree = in.dev(tree);
    hipStream_t s = ctx().stream;
    MHS_HIP(in.upload(0, in.mark(), s));
    MHS_HIP(work.zero(w_flag, s));
    // the LDS of a block is sized by the rows of the call's largest model (up to RF_LDS_ROWS), so small trees share a compute unit
    const int lds_rows = (int)std::min<int64_t>(n_max, RF_LDS_ROWS);
    const size_t lds_bytes = fit_align(sizeof(double) * (size_t)lds_rows) + fit_align(sizeof(int) * (size_t)lds_rows) + fit_align((size_t)lds_rows) +
                             (2 * sizeof(double) + 2 * sizeof(int)) * RF_PAIRS + 16;
    MHS_HIP(hipFuncSetAttribute((const void *)rf_grow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(rf_grow_kernel, dim3((unsigned)NT), dim3(RF_T), lds_bytes, s, dmod, dtree, S, p, mtry, nodesize, lds_rows);
    MHS_HIP(hipGetLastError());
    long long *d_toff = res.dev(r_toff);
    hipLaunchKernelGGL(rf_offsets_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, S.n_nodes, d_toff, count, n_trees);
    MHS_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf_compact_kernel, dim3((unsigned)NT), dim3(256), 0, s, dtree, S, d_toff, n_trees, res.dev(r_int[0]), res.dev(r_int[1]),
                       res.dev(r_int[2]), res.dev(r_int[3]), res.dev(r_dbl[0]), res.dev(r_dbl[1]));
    MHS_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf_reduce_kernel, dim3((unsigned)((n_max + 255) / 256), (unsigned)count), dim3(256), 0, s, dmod, S, p, n_trees);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(res.dev(r_flag), S.flag, r_flag.bytes(), hipMemcpyDeviceToDevice, s));
    MHS_HIP(res.download(0, small_end, s));
    MHS_HIP(hipStreamSynchronize(s));
    const int *flags = res.host(r_flag);
    for (size_t t = 0; t < NT; ++t)
        if (flags[t]) { set_error("mhs_rf_fit_many: a tree's node count exceeds its bound"); return MHS_ERR_NUMERIC; }
    // ---- the compacted arrays of every model, then the ordinary loader
    std::vector<std::shared_ptr<RfFitted>> fitted((size_t)count);
    for (int k = 0; k < count; ++k) {
        const long long *to = res.host(r_toff) + (size_t)k * ((size_t)n_trees + 1);
        const size_t nn = (size_t)to[n_trees];
        if ((long long)nn > out_base[k + 1] - out_base[k]) { set_error("mhs_rf_fit_many: node count exceeds its bound"); return MHS_ERR_NUMERIC; }
        auto f = std::make_shared<RfFitted>();
        f->tree_offsets.assign(to, to + n_trees + 1);
        f->left.resize(nn); f->right.resize(nn); f->status.resize(nn); f->best_var.resize(nn); f->split.resize(nn); f->node_pred.resize(nn);
        int32_t *const ia[4] = {f->left.data(), f->right.data(), f->status.data(), f->best_var.data()};
        double *const da[2] = {f->split.data(), f->node_pred.data()};
        for (int a = 0; a < 4; ++a)
            MHS_HIP(hipMemcpyAsync(ia[a], res.dev(r_int[a]) + out_base[k], sizeof(int) * nn, hipMemcpyDeviceToHost, s));
        for (int a = 0; a < 2; ++a)
            MHS_HIP(hipMemcpyAsync(da[a], res.dev(r_dbl[a]) + out_base[k], sizeof(double) * nn, hipMemcpyDeviceToHost, s));
        fitted[k] = f;
    }
    MHS_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < count; ++k) {
        const RfFitted &f = *fitted[k];
        mhs_model *m = nullptr;
        int rc = mhs_rf_load(n_trees, f.tree_offsets.data(), f.left.data(), f.right.data(), f.status.data(), f.best_var.data(),
                             f.split.data(), f.node_pred.data(), p, &m);
        if (rc) {
            for (int q = 0; q < k; ++q) { mhs_model_free(models_out[q]); models_out[q] = nullptr; }
            return rc;
        }
        m->rf_fitted = fitted[k];
        models_out[k] = m;
        if (oob_pred && oob_pred[k]) std::copy_n(res.host(r_oobp) + res_off[k], (size_t)n[k], oob_pred[k]);
        if (oob_count && oob_count[k]) std::copy_n(res.host(r_oobc) + res_off[k], (size_t)n[k], oob_count[k]);
        if (inc_node_purity && inc_node_purity[k]) std::copy_n(res.host(r_pur) + (size_t)k * p, (size_t)p, inc_node_purity[k]);
    }
    return MHS_OK;
}

int mhs_rf_get(const mhs_model *m, int64_t *n_nodes, int32_t *left, int32_t *right, int32_t *status, int32_t *best_var,
               double *split, double *node_pred, int64_t *tree_offsets) {
    MHS_REQUIRE(m != nullptr && n_nodes != nullptr, "NULL argument");
    MHS_REQUIRE(m->kind == K_RF && m->rf_fitted, "not a forest fitted by mhs_rf_fit_many");
    const RfFitted &f = *m->rf_fitted;
    *n_nodes = (int64_t)f.left.size();
    if (left) std::copy(f.left.begin(), f.left.end(), left);
    if (right) std::copy(f.right.begin(), f.right.end(), right);
    if (status) std::copy(f.status.begin(), f.status.end(), status);
    if (best_var) std::copy(f.best_var.begin(), f.best_var.end(), best_var);
    if (split) std::copy(f.split.begin(), f.split.end(), split);
    if (node_pred) std::copy(f.node_pred.begin(), f.node_pred.end(), node_pred);
    if (tree_offsets) std::copy(f.tree_offsets.begin(), f.tree_offsets.end(), tree_offsets);
    return MHS_OK;
}

}  // extern "C"
