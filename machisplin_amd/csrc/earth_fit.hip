// Fitting earth (MARS) models on the device: earth::earth(mod.form, data, nfold = 10) as the reference calls it eleven
// times per layer (V73:250 once per CV fold, V73:539 the final model) -- degree = 1, pmethod = "backward", penalty = 2,
// thresh = 0.001, nk = min(200, max(20, 2 p)) + 1, automatic minspan / endspan, numeric predictors, no weights, no NA in the
// training rows (V73:154).  nfold = 10 makes earth fit ten more models per call for its CV R^2: 121 independent fits per
// layer.  Not a port: the earth package is only imported by the reference; the rule is the one include/machisplin_hip.h
// states above mhs_earth_fit_many (its departures from earth's own C code are listed there), restated in numpy by
// tests/earth_ref.py.
//
// The parallelism is across models: `count` models in ONE launch, ONE RESIDENT WORKGROUP (4 waves) PER MODEL; forward
// pass, pruning and coefficients all run inside that workgroup and the host does no fitting arithmetic (it sorts the rows
// per variable once per model, stable, as rf_fit.hip does, and derives minspan / endspan from n and p).
//
//   * the residual r and the column being added live in LDS for n <= EARTH_LDS_ROWS (16 B per row), in a per-model slab
//     in device memory beyond (the same code and the same arithmetic: only the address space differs);
//   * the orthonormal basis Q (n x nk doubles, row-major: a row's entries are contiguous) lives in a per-model slab in
//     device memory, which at these sizes sits in L2; so does XO (p x n): every variable's column orthogonalised
//     against the current basis, updated with each new basis column (modified Gram-Schmidt), so that the in-span test
//     and the linear candidate of a variable cost one pass over its column;
//   * THE KNOT SEARCH of a variable belongs to one wave; the waves of the block take the variables round-robin.  The
//     wave walks the variable's sorted order from the TOP in 64-row steps, a lane per position u (rows above: u).  With
//     d_u = x_(u-1) - x_u >= 0 the hinge at the knot x_u satisfies, for any column q,
//         S_u = sum_{u' < u} q_u'                 (a prefix sum),
//         h_u . q = G_u = G_(u-1) + d_u S_u        (a prefix sum of d S: Friedman's update, all knots of a variable
//                                                  in O(n M) instead of a solve per knot),
//     and |h_u|^2 = H2_u = H2_(u-1) + d_u (2 H1_(u-1) + d_u u), H1_u = H1_(u-1) + d_u u.  Only differences of neighbouring
//     x enter, so a large offset of x (a longitude) costs no digits.  Per basis column, for q_x (the variable's own
//     orthogonalised column) and for r: |h_o|^2 = H2 - sum_k G_k^2 - G_x^2, h_o . r = G_r - G_x (q_x . r).  The carries
//     of column k between steps sit in lane k's registers (M <= 63 while a search runs);
//   * the block's arg-max follows the rule's candidate order: variables ascending, linear before knots, knots by
//     position, only a strictly greater reduction replaces the best;
//   * the winning term's column(s) are formed explicitly and orthogonalised TWICE against Q (classical Gram-Schmidt,
//     a wave per basis column for the dot products); the triangular factor R (B = Q R) and Q'y grow with them, r is
//     updated with the new column and the recorded RSS is sum r^2;
//   * PRUNING works on R and Q'y, never on the normal equations: at every size thread j solves row j of R^-1 (w), the
//     coefficient is beta_j = w . Q'y and dropping term j raises the RSS by beta_j^2 / |w|^2; the chosen column is deleted
//     from R with Givens rotations (wave 0, a lane per column) that also rotate Q'y.  The coefficients of every size are
//     kept, so the selected size's least squares come from that same factor.  R and the rows w live in LDS (the space
//     r and the column occupied during the forward pass).
//
// SUMMATION ORDER.  A sum over the rows of a model (mean, RSS, a dot product with a basis column) is taken either by the
// block -- thread t adds rows t, t + 256, ... in order, a wave adds its lanes with an xor butterfly, the four waves are
// added in order -- or by one wave -- lane l adds rows l, l + 64, ..., then the butterfly.  A prefix sum along a sorted
// order is (the carry of the earlier 64-row steps, added step by step) + (a log-depth lane scan inside the step).  All of
// it is fixed by n, p and nk alone: a model is bit-identical from call to call and whatever else shares the launch; there
// are no floating-point atomics.  The sums differ from sequential ones in the last bits, which is why the tests follow
// the device's own choices with a certificate (earth_ref.check_model) instead of comparing structures.
#include <vector>
#include "ensemble_int.h"
#include "fit_common.h"

namespace mhs {

constexpr int EARTH_T = 256;                 // threads of a model's workgroup
constexpr int EARTH_W = EARTH_T / 64;
constexpr int EARTH_MAXP = 64;               // mhs_earth_load's range
constexpr int EARTH_LDS_ROWS = 4096;         // rows whose residual and working column (8 B each) stay in LDS
constexpr double EARTH_SPAN_TOL = 1e-10;
static_assert(MHS_EARTH_MAX_NK <= 65, "the search keeps the carries of basis column k in lane k");

enum { ES_CONSTANT = MHS_EARTH_STOP_CONSTANT, ES_NK = MHS_EARTH_STOP_NK, ES_NONE = MHS_EARTH_STOP_NONE, ES_THRESH = MHS_EARTH_STOP_THRESH,
       ES_RSQ = MHS_EARTH_STOP_RSQ, ES_GRSQ = MHS_EARTH_STOP_GRSQ };

struct EarthModelDev {
    const double *X, *y;            // n x p column-major, n
    const int *ord;                 // p x n: rows in ascending order of every variable (stable)
    double *Q;                      // n x nk row-major
    double *XO;                     // p x n
    double *rg, *bg;                // n each (used beyond EARTH_LDS_ROWS)
    double *R, *z;                  // nk x nk column-major, nk
    double *out_d;                  // [cut nk | forward rss nk | rss per subset nk | gcv per subset nk | beta nk x nk | rss gcv rsq grsq]
    int *out_i;                     // [var nk | dir nk | prune_terms nk x nk | M, stop, selected size, flag]
    int n, minspan, endspan, pad;
};

// the block's sum of one value per thread: waves in order.  Every thread calls it and gets the same value.
__device__ __forceinline__ double earth_block_sum(double v, double *part) {
    v = fit_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

__device__ __forceinline__ double earth_gcv(double rss, int k, int n, double penalty) {
    const double c = (double)k + penalty * (double)(k - 1) / 2.0;
    if (c >= (double)n) return INFINITY;
    const double d = 1.0 - c / (double)n;
    return (rss / (double)n) / (d * d);
}

struct EarthBest { double red; int kind, pos; };

// The best candidate of variable v for one wave: kind 0 none, 2 linear, 1 pair, 3 single hinge; pos the knot's position in
// the sorted order.  Every lane returns the same.
__device__ __forceinline__ EarthBest earth_search(const EarthModelDev &Md, int v, int M, int ldq, const double *r, double xn2) {
    const int lane = threadIdx.x & 63;
    const int n = Md.n, ms = Md.minspan, es = Md.endspan;
    const double *xo = Md.XO + (size_t)v * n;
    const double *xc = Md.X + (size_t)v * n;
    const int *od = Md.ord + (size_t)v * n;
    double s2 = 0.0, sr = 0.0;
    for (int i = lane; i < n; i += 64) { const double a = xo[i]; s2 = s2 + a * a; sr = sr + a * r[i]; }
    s2 = fit_wave_sum(s2); sr = fit_wave_sum(sr);
    const bool has_lin = s2 > EARTH_SPAN_TOL * xn2;
    const double inv = has_lin ? 1.0 / sqrt(s2) : 0.0;
    const double cx = sr * inv, lin = has_lin ? cx * cx : 0.0;
    EarthBest best;
    best.red = lin; best.kind = has_lin ? 2 : 0; best.pos = -1;
    double Sc = 0.0, Gc = 0.0;                      // lane k: the carries of basis column k
    double Sx = 0.0, Gx = 0.0, Sr = 0.0, Gr = 0.0, H1c = 0.0, H2c = 0.0, xlast = 0.0;
    double lred = -1.0;
    int lpos = -1;
    for (int base = 0; base < n; base += 64) {
        const int u = base + lane;
        const bool ok = u < n;
        const int j = n - 1 - u;
        const int row = ok ? od[j] : 0;
        const double x = ok ? xc[row] : 0.0;
        double xp = __shfl_up(x, 1);
        if (lane == 0) xp = xlast;
        const double d = (ok && u > 0) ? xp - x : 0.0;
        const double cnt = (double)u;
        const double H1 = H1c + fit_wave_scan(d * cnt);
        double H1p = __shfl_up(H1, 1);
        if (lane == 0) H1p = H1c;
        const double H2 = H2c + fit_wave_scan(d * (2.0 * H1p + d * cnt));
        H1c = __shfl(H1, 63); H2c = __shfl(H2, 63);
        double den = H2;
        const double *qrow = Md.Q + (size_t)row * ldq;
        for (int k = 0; k < M; ++k) {
            const double q = ok ? qrow[k] : 0.0;
            const double si = fit_wave_scan(q);
            double se = __shfl_up(si, 1);
            if (lane == 0) se = 0.0;
            const double sk = __shfl(Sc, k);
            const double G = __shfl(Gc, k) + fit_wave_scan(d * (sk + se));
            den = den - G * G;
            const double ns = sk + __shfl(si, 63), ng = __shfl(G, 63);
            if (lane == k) { Sc = ns; Gc = ng; }
        }
        double gx = 0.0;
        if (has_lin) {
            const double q = ok ? xo[row] * inv : 0.0;
            const double si = fit_wave_scan(q);
            double se = __shfl_up(si, 1);
            if (lane == 0) se = 0.0;
            gx = Gx + fit_wave_scan(d * (Sx + se));
            den = den - gx * gx;
            Sx = Sx + __shfl(si, 63); Gx = __shfl(gx, 63);
        }
        double gr;
        {
            const double q = ok ? r[row] : 0.0;
            const double si = fit_wave_scan(q);
            double se = __shfl_up(si, 1);
            if (lane == 0) se = 0.0;
            gr = Gr + fit_wave_scan(d * (Sr + se));
            Sr = Sr + __shfl(si, 63); Gr = __shfl(gr, 63);
        }
        bool elig = ok && j >= es && j < n - es && (j - es) % ms == 0;
        if (elig) elig = x > xc[od[j - 1]];              // j >= endspan >= 1
        if (elig && H2 > 0.0 && den > EARTH_SPAN_TOL * H2) {
            const double num = gr - gx * cx;
            const double red = lin + num * num / den;
            if (red >= lred) { lred = red; lpos = j; }     // a lane's positions descend: the lowest stays
        }
        xlast = __shfl(x, 63);
    }
    double wred = lred;
    int wpos = lpos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double r2 = __shfl_xor(wred, o);
        const int p2 = __shfl_xor(wpos, o);
        if (p2 >= 0 && (wpos < 0 || r2 > wred || (r2 == wred && p2 < wpos))) { wred = r2; wpos = p2; }
    }
    if (wpos >= 0 && wred > best.red) { best.red = wred; best.kind = has_lin ? 1 : 3; best.pos = wpos; }
    return best;
}

__global__ __launch_bounds__(EARTH_T) void earth_fit_kernel(const EarthModelDev *__restrict__ models, int p, int nk, double thresh,
                                                            double penalty, int lds_rows) {
    extern __shared__ __attribute__((aligned(16))) char earth_dyn[];
    const EarthModelDev Md = models[blockIdx.x];
    const int n = Md.n, ldq = nk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- LDS: [fixed part] [r | column]  or, after the forward pass,  [R | rows of R^-1]
    char *q0 = earth_dyn;
    double *part = (double *)q0;        q0 += sizeof(double) * 4;
    double *sh_d = (double *)q0;        q0 += sizeof(double) * 4;       // rss0, rss, best reduction, scratch
    double *v_red = (double *)q0;       q0 += sizeof(double) * EARTH_MAXP;
    double *xn2 = (double *)q0;         q0 += sizeof(double) * EARTH_MAXP;
    double *ck = (double *)q0;          q0 += sizeof(double) * (MHS_EARTH_MAX_NK + 1);
    double *dlt = (double *)q0;         q0 += sizeof(double) * (MHS_EARTH_MAX_NK + 1);
    double *zw = (double *)q0;          q0 += sizeof(double) * (MHS_EARTH_MAX_NK + 1);
    int *v_kind = (int *)q0;            q0 += sizeof(int) * EARTH_MAXP;
    int *v_pos = (int *)q0;             q0 += sizeof(int) * EARTH_MAXP;
    int *kept = (int *)q0;              q0 += sizeof(int) * (MHS_EARTH_MAX_NK + 3);
    int *sh_i = (int *)q0;              q0 += sizeof(int) * 8;          // M, best v, best kind, best pos, flag, j*
    double *big = (double *)q0;
    const bool in_lds = n <= lds_rows;
    double *r = in_lds ? big : Md.rg;
    double *b = in_lds ? big + lds_rows : Md.bg;
    double *Rw = big, *W = big + (size_t)nk * nk;

    double *o_cut = Md.out_d, *o_frss = o_cut + nk, *o_srss = o_frss + nk, *o_gcv = o_srss + nk, *o_beta = o_gcv + nk;
    double *o_stat = o_beta + (size_t)nk * nk;
    int *o_var = Md.out_i, *o_dir = o_var + nk, *o_pt = o_dir + nk, *o_head = o_pt + (size_t)nk * nk;

    // ---- the intercept: q0 = 1 / sqrt(n), r = y - mean y
    double acc = 0.0;
    for (int i = tid; i < n; i += EARTH_T) acc = acc + Md.y[i];
    const double sum_y = earth_block_sum(acc, part);
    const double mean = sum_y / (double)n, qs = 1.0 / sqrt((double)n);
    acc = 0.0;
    for (int i = tid; i < n; i += EARTH_T) {
        const double e = Md.y[i] - mean;
        r[i] = e; acc = acc + e * e;
        Md.Q[(size_t)i * ldq] = qs;
    }
    const double rss0 = earth_block_sum(acc, part);
    if (tid == 0) {
        Md.R[0] = sqrt((double)n); Md.z[0] = sum_y * qs;
        o_var[0] = -1; o_dir[0] = 0; o_cut[0] = 0.0; o_frss[0] = rss0;
        sh_i[0] = 1; sh_i[4] = 0;
        sh_d[1] = rss0;
    }
    // every variable's column orthogonalised against the intercept (twice), and its raw squared norm
    for (int v = wave; v < p; v += EARTH_W) {
        const double *xc = Md.X + (size_t)v * n;
        double *xo = Md.XO + (size_t)v * n;
        double s = 0.0, s2 = 0.0;
        for (int i = lane; i < n; i += 64) { const double a = xc[i]; s = s + a; s2 = s2 + a * a; }
        s = fit_wave_sum(s); s2 = fit_wave_sum(s2);
        const double m1 = s / (double)n;
        double t = 0.0;
        for (int i = lane; i < n; i += 64) { const double a = xc[i] - m1; xo[i] = a; t = t + a; }
        t = fit_wave_sum(t);
        const double m2 = t / (double)n;
        for (int i = lane; i < n; i += 64) xo[i] = xo[i] - m2;
        if (lane == 0) xn2[v] = s2;
    }
    __syncthreads();
    const double gcv1 = earth_gcv(rss0, 1, n, penalty);

    // ================================================================ the forward pass
    int stop = 0;
    if (rss0 == 0.0) stop = ES_CONSTANT;
    while (!stop) {
        const int M = sh_i[0];
        if (M + 2 > nk) { stop = ES_NK; break; }
        for (int v = wave; v < p; v += EARTH_W) {
            const EarthBest bv = earth_search(Md, v, M, ldq, r, xn2[v]);
            if (lane == 0) { v_red[v] = bv.red; v_kind[v] = bv.kind; v_pos[v] = bv.pos; }
        }
        __syncthreads();
        if (tid == 0) {
            double br = 0.0;
            int bvv = -1;
            for (int v = 0; v < p; ++v)
                if (v_kind[v] != 0 && v_red[v] > br) { br = v_red[v]; bvv = v; }
            sh_d[2] = br; sh_i[1] = bvv; sh_i[2] = bvv >= 0 ? v_kind[bvv] : 0; sh_i[3] = bvv >= 0 ? v_pos[bvv] : -1;
        }
        __syncthreads();
        const double best = sh_d[2];
        const int bv = sh_i[1], bkind = sh_i[2], bpos = sh_i[3];
        if (bv < 0 || !(best > 0.0)) { stop = ES_NONE; break; }
        if (best / rss0 < thresh) { stop = ES_THRESH; break; }
        const double *xc = Md.X + (size_t)bv * n;
        const double cut = bkind == 2 ? 0.0 : xc[Md.ord[(size_t)bv * n + bpos]];
        const int ncols = bkind == 1 ? 2 : 1;
        bool bad = false;
        for (int c = 0; c < ncols; ++c) {
            const int Mc = M + c;
            const int dir = bkind == 2 ? 2 : (c == 0 ? 1 : -1);
            for (int i = tid; i < n; i += EARTH_T) {
                const double x = xc[i];
                b[i] = dir == 2 ? x : (dir == 1 ? fmax(0.0, x - cut) : fmax(0.0, cut - x));
            }
            __syncthreads();
            for (int pass = 0; pass < 2; ++pass) {
                for (int k = wave; k < Mc; k += EARTH_W) {
                    double s = 0.0;
                    for (int i = lane; i < n; i += 64) s = s + Md.Q[(size_t)i * ldq + k] * b[i];
                    s = fit_wave_sum(s);
                    if (lane == 0) {
                        ck[k] = s;
                        double *rk = Md.R + (size_t)Mc * nk + k;
                        *rk = pass == 0 ? s : *rk + s;
                    }
                }
                __syncthreads();
                for (int i = tid; i < n; i += EARTH_T) {
                    const double *qrow = Md.Q + (size_t)i * ldq;
                    double e = b[i];
                    for (int k = 0; k < Mc; ++k) e = e - ck[k] * qrow[k];
                    b[i] = e;
                }
                __syncthreads();
            }
            acc = 0.0;
            for (int i = tid; i < n; i += EARTH_T) acc = acc + b[i] * b[i];
            const double nrm2 = earth_block_sum(acc, part);
            if (!(nrm2 > 0.0)) { bad = true; break; }
            const double dn = sqrt(nrm2);
            acc = 0.0;
            for (int i = tid; i < n; i += EARTH_T) {
                const double q = b[i] / dn;
                b[i] = q; Md.Q[(size_t)i * ldq + Mc] = q;
                acc = acc + q * r[i];
            }
            const double zq = earth_block_sum(acc, part);
            for (int i = tid; i < n; i += EARTH_T) r[i] = r[i] - b[i] * zq;
            if (tid == 0) {
                Md.R[(size_t)Mc * nk + Mc] = dn; Md.z[Mc] = zq;
                o_var[Mc] = bv; o_dir[Mc] = dir; o_cut[Mc] = cut;
            }
            for (int v = wave; v < p; v += EARTH_W) {
                double *xo = Md.XO + (size_t)v * n;
                double s = 0.0;
                for (int i = lane; i < n; i += 64) s = s + b[i] * xo[i];
                s = fit_wave_sum(s);
                for (int i = lane; i < n; i += 64) xo[i] = xo[i] - b[i] * s;
            }
            __syncthreads();
        }
        if (bad) {
            if (tid == 0) sh_i[4] = 1;
            stop = ES_NONE;
            break;
        }
        acc = 0.0;
        for (int i = tid; i < n; i += EARTH_T) acc = acc + r[i] * r[i];
        const double rss = earth_block_sum(acc, part);
        const int Mn = M + ncols;
        if (tid == 0) {
            for (int c = M; c < Mn; ++c) o_frss[c] = rss;
            sh_i[0] = Mn; sh_d[1] = rss;
        }
        __syncthreads();
        if (1.0 - rss / rss0 > 1.0 - thresh) stop = ES_RSQ;
        else if (1.0 - earth_gcv(rss, Mn, n, penalty) / gcv1 < -10.0) stop = ES_GRSQ;
    }
    __syncthreads();

    // ================================================================ pruning, on R and Q'y
    const int M = sh_i[0];
    for (int e = tid; e < M * M; e += EARTH_T) {
        const int c = e / M, k = e - c * M;
        Rw[(size_t)c * nk + k] = k <= c ? Md.R[(size_t)c * nk + k] : 0.0;
    }
    if (tid < M) { zw[tid] = Md.z[tid]; kept[tid] = tid; }
    if (tid == 0) sh_d[3] = sh_d[1];
    for (int m = M; m >= 1; --m) {
        __syncthreads();
        if (tid < m) {
            const int j = tid;
            double *w = W + (size_t)j * nk;
            w[j] = 1.0 / Rw[(size_t)j * nk + j];
            double nrm = w[j] * w[j], bj = w[j] * zw[j];
            for (int k = j + 1; k < m; ++k) {
                const double *col = Rw + (size_t)k * nk;
                double s = 0.0;
                for (int i = j; i < k; ++i) s = s + w[i] * col[i];
                const double wk = -s / col[k];
                w[k] = wk;
                nrm = nrm + wk * wk; bj = bj + wk * zw[k];
            }
            o_beta[(size_t)(m - 1) * nk + j] = bj;
            dlt[j] = bj * bj / nrm;
            o_pt[(size_t)(m - 1) * nk + j] = kept[j];
        } else if (tid < nk) {
            o_pt[(size_t)(m - 1) * nk + tid] = -1;
        }
        __syncthreads();
        if (m == 1) {
            if (tid == 0) { o_srss[0] = sh_d[3]; o_beta[0] = mean; }        // least squares on the intercept alone IS the mean
            break;
        }
        if (tid == 0) {
            int js = 1;
            for (int j = 2; j < m; ++j)
                if (dlt[j] < dlt[js]) js = j;
            if (!(dlt[js] >= 0.0)) sh_i[4] = 1;                 // a NaN: a zero pivot in R
            sh_i[5] = js;
            o_srss[m - 1] = sh_d[3];
            sh_d[3] = sh_d[3] + dlt[js];
        }
        __syncthreads();
        const int js = sh_i[5];
        // column js out: the columns to its right move one to the left (a thread per row), then Givens rotations
        if (tid < m) {
            for (int c = js; c < m - 1; ++c) Rw[(size_t)c * nk + tid] = Rw[(size_t)(c + 1) * nk + tid];
            if (tid == 0)
                for (int c = js; c < m - 1; ++c) kept[c] = kept[c + 1];
        }
        __syncthreads();
        if (wave == 0) {
            for (int i = js; i < m - 1; ++i) {
                double t1[2], t2[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int c = lane + 64 * s;
                    const bool on = c >= i && c < m - 1;
                    t1[s] = on ? Rw[(size_t)c * nk + i] : 0.0;
                    t2[s] = on ? Rw[(size_t)c * nk + i + 1] : 0.0;
                }
                const double a = __shfl(i < 64 ? t1[0] : t1[1], i & 63), bb = __shfl(i < 64 ? t2[0] : t2[1], i & 63);
                const double rho = sqrt(a * a + bb * bb);
                const double cs = rho > 0.0 ? a / rho : 1.0, sn = rho > 0.0 ? bb / rho : 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int c = lane + 64 * s;
                    if (c >= i && c < m - 1) {
                        Rw[(size_t)c * nk + i] = cs * t1[s] + sn * t2[s];
                        Rw[(size_t)c * nk + i + 1] = c == i ? 0.0 : cs * t2[s] - sn * t1[s];
                    }
                }
                if (lane == 0) {
                    const double z1 = zw[i], z2 = zw[i + 1];
                    zw[i] = cs * z1 + sn * z2; zw[i + 1] = cs * z2 - sn * z1;
                }
            }
        }
    }
    __syncthreads();
    // ---- the size with the smallest GCV (the smaller size on a tie)
    if (tid == 0) {
        int ksel = 1;
        double gbest = 0.0;
        for (int k = 1; k <= M; ++k) {
            const double g = earth_gcv(o_srss[k - 1], k, n, penalty);
            o_gcv[k - 1] = g;
            if (k == 1 || g < gbest) { gbest = g; ksel = k; }
        }
        const double rs = o_srss[ksel - 1];
        o_stat[0] = rs; o_stat[1] = gbest;
        o_stat[2] = rss0 > 0.0 ? 1.0 - rs / rss0 : 0.0;
        o_stat[3] = rss0 > 0.0 ? 1.0 - gbest / gcv1 : 0.0;
        o_head[0] = M; o_head[1] = stop; o_head[2] = ksel; o_head[3] = sh_i[4];
    }
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_earth_fit_many(int count, const double *const *X, const double *const *y, const int64_t *n, int p, int nk, double thresh,
                       double penalty, int minspan, int endspan, mhs_model **models_out) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(X && y && n && models_out, "NULL argument");
    if (int rc = fit_check_batch(__func__, count, p, EARTH_MAXP)) return rc;
    if (nk <= 0) nk = std::min(200, std::max(20, 2 * p)) + 1;
    MHS_REQUIRE(nk <= MHS_EARTH_MAX_NK, "nk exceeds MHS_EARTH_MAX_NK (p > 32 must pass an nk)");
    MHS_REQUIRE(thresh >= 0.0 && penalty >= 0.0, "thresh and penalty must not be negative");       // (false for NaN)
    for (int k = 0; k < count; ++k) models_out[k] = nullptr;
    // ---- checks, and the layout of the three blocks: [uploaded: inputs, records] [work] [out: every model's records, zeroed, all home]
    struct Lay { FitPiece<double> X, y, Q, XO, rg, bg, R, z; FitPiece<int> ord; };
    std::vector<Lay> lay((size_t)count);
    FitBlock in, work, out;
    int64_t n_max = 0;
    const size_t od_len = 4 * (size_t)nk + (size_t)nk * nk + 4, oi_len = 2 * (size_t)nk + (size_t)nk * nk + 4;
    for (int k = 0; k < count; ++k) {
        MHS_REQUIRE(n[k] >= 2 && n[k] * (int64_t)std::max(p, nk) < (1LL << 31), "n out of range");
        if (int rc = fit_check_model(__func__, X[k], y[k], n[k], p)) return rc;
        const size_t nn = (size_t)n[k]; n_max = std::max(n_max, n[k]);
        lay[k].X = in.take<double>(nn * p); lay[k].y = in.take<double>(nn); lay[k].ord = in.take<int>(nn * p);
        lay[k].Q = work.take<double>(nn * nk); lay[k].XO = work.take<double>(nn * p);
        lay[k].rg = work.take<double>(nn); lay[k].bg = work.take<double>(nn);
        lay[k].R = work.take<double>((size_t)nk * nk); lay[k].z = work.take<double>((size_t)nk);
    }
    const FitPiece<EarthModelDev> mod = in.take<EarthModelDev>((size_t)count);
    const FitPiece<double> od = out.take<double>(od_len * count);       // the models' records back to back, as the kernel's rows are
    const FitPiece<int> oi = out.take<int>(oi_len * count);
    in.mirror(0, in.mark()); out.mirror(0, out.mark());
    MHS_HIP(in.alloc()); MHS_HIP(work.alloc()); MHS_HIP(out.alloc());
    for (int k = 0; k < count; ++k) {
        const Lay &L = lay[k];
        const int64_t nn = n[k];
        std::copy_n(X[k], (size_t)nn * p, in.host(L.X));
        std::copy_n(y[k], (size_t)nn, in.host(L.y));
        fit_sorted_orders(X[k], nn, p, in.host(L.ord));
        EarthModelDev &m = in.host(mod)[k];
        m.X = in.dev(L.X); m.y = in.dev(L.y); m.ord = in.dev(L.ord);
        m.Q = work.dev(L.Q); m.XO = work.dev(L.XO); m.rg = work.dev(L.rg); m.bg = work.dev(L.bg); m.R = work.dev(L.R); m.z = work.dev(L.z);
        m.out_d = out.dev(od) + od_len * k; m.out_i = out.dev(oi) + oi_len * k;
        m.n = (int)nn; m.pad = 0;
        const int ms = (int)(-std::log2(-(1.0 / ((double)p * (double)nn)) * std::log(1.0 - 0.05)) / 2.5);
        const int es = (int)(3.0 - std::log2(0.05 / (double)p));
        m.minspan = minspan > 0 ? minspan : std::max(1, ms);
        m.endspan = endspan > 0 ? endspan : std::max(1, es);
    }
    hipStream_t s = ctx().stream;
    MHS_HIP(in.upload(0, in.mark(), s));
    MHS_HIP(out.zero(0, out.mark(), s));
    // the LDS of a block: the fixed part, then the larger of (r, the column) for the call's largest model and (R, rows of R^-1)
    const int lds_rows = (int)std::min<int64_t>(n_max, EARTH_LDS_ROWS);
    const size_t fixed = sizeof(double) * (8 + 2 * EARTH_MAXP + 3 * (MHS_EARTH_MAX_NK + 1)) + sizeof(int) * (2 * EARTH_MAXP + MHS_EARTH_MAX_NK + 3 + 8);
    const size_t lds_bytes = fit_align(fixed) + sizeof(double) * std::max<size_t>(2 * (size_t)lds_rows, 2 * (size_t)nk * nk) + 16;
    MHS_HIP(hipFuncSetAttribute((const void *)earth_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(earth_fit_kernel, dim3((unsigned)count), dim3(EARTH_T), lds_bytes, s, (const EarthModelDev *)in.dev(mod), p, nk, thresh,
                       penalty, lds_rows);
    MHS_HIP(hipGetLastError());
    MHS_HIP(out.download(0, out.mark(), s));
    MHS_HIP(hipStreamSynchronize(s));
    // ---- the records, then the ordinary loader
    for (int k = 0; k < count; ++k) {
        const double *d = out.host(od) + od_len * k;
        const int *iv = out.host(oi) + oi_len * k;
        const int *head = iv + 2 * (size_t)nk + (size_t)nk * nk;
        const int M = head[0], ksel = head[2];
        int rc = MHS_OK;
        if (head[3] || M < 1 || M > nk || ksel < 1 || ksel > M) {
            set_error("mhs_earth_fit_many: model %d: a basis column or a pivot of the triangular factor vanished", k);
            rc = MHS_ERR_NUMERIC;
        }
        auto f = std::make_shared<EarthFitted>();
        if (!rc) {
            f->p = p; f->n_forward = M; f->n_selected = ksel; f->stop = head[1];
            f->fwd_dirs.assign((size_t)M * p, 0); f->fwd_cuts.assign((size_t)M * p, 0.0);
            for (int t = 1; t < M; ++t) {
                const int v = iv[t];
                if (v < 0 || v >= p) { rc = MHS_ERR_NUMERIC; set_error("mhs_earth_fit_many: corrupt term record"); break; }
                f->fwd_dirs[(size_t)t * p + v] = iv[nk + t];
                f->fwd_cuts[(size_t)t * p + v] = d[t];
            }
        }
        if (!rc) {
            f->fwd_rss.assign(d + nk, d + nk + M);
            f->rss_sub.assign(d + 2 * (size_t)nk, d + 2 * (size_t)nk + M);
            f->gcv_sub.assign(d + 3 * (size_t)nk, d + 3 * (size_t)nk + M);
            f->prune_terms.assign((size_t)M * M, -1);
            const int *pt = iv + 2 * (size_t)nk;
            for (int a = 0; a < M; ++a)
                for (int c = 0; c <= a; ++c) f->prune_terms[(size_t)a * M + c] = pt[(size_t)a * nk + c];
            f->selected.assign((size_t)M, 0);
            const double *beta = d + 4 * (size_t)nk + (size_t)(ksel - 1) * nk;
            f->coef.assign(beta, beta + ksel);
            f->dirs.assign((size_t)ksel * p, 0); f->cuts.assign((size_t)ksel * p, 0.0);
            for (int c = 0; c < ksel && !rc; ++c) {
                const int t = pt[(size_t)(ksel - 1) * nk + c];
                if (t < 0 || t >= M) { rc = MHS_ERR_NUMERIC; set_error("mhs_earth_fit_many: corrupt pruning record"); break; }
                f->selected[(size_t)t] = 1;
                std::copy_n(f->fwd_dirs.begin() + (size_t)t * p, p, f->dirs.begin() + (size_t)c * p);
                std::copy_n(f->fwd_cuts.begin() + (size_t)t * p, p, f->cuts.begin() + (size_t)c * p);
            }
            const double *st = d + 4 * (size_t)nk + (size_t)nk * nk;
            std::copy_n(st, 4, f->stats);
        }
        mhs_model *m = nullptr;
        if (!rc) rc = mhs_earth_load(f->coef.data(), f->dirs.data(), f->cuts.data(), ksel, p, &m);
        if (rc) {
            for (int q = 0; q < k; ++q) { mhs_model_free(models_out[q]); models_out[q] = nullptr; }
            return rc;
        }
        m->earth_fitted = f;
        models_out[k] = m;
    }
    return MHS_OK;
}

int mhs_earth_get(const mhs_model *m, int *n_selected, int *n_forward, int *stop_reason, double *coef, int32_t *dirs, double *cuts,
                  int32_t *forward_dirs, double *forward_cuts, double *forward_rss, int32_t *selected, double *rss_per_subset,
                  double *gcv_per_subset, int32_t *prune_terms, double *stats) {
    MHS_REQUIRE(m != nullptr && n_selected != nullptr && n_forward != nullptr, "NULL argument");
    MHS_REQUIRE(m->kind == K_EARTH && m->earth_fitted, "not a model fitted by mhs_earth_fit_many");
    const EarthFitted &f = *m->earth_fitted;
    *n_selected = f.n_selected; *n_forward = f.n_forward;
    if (stop_reason) *stop_reason = f.stop;
    if (coef) std::copy(f.coef.begin(), f.coef.end(), coef);
    if (dirs) std::copy(f.dirs.begin(), f.dirs.end(), dirs);
    if (cuts) std::copy(f.cuts.begin(), f.cuts.end(), cuts);
    if (forward_dirs) std::copy(f.fwd_dirs.begin(), f.fwd_dirs.end(), forward_dirs);
    if (forward_cuts) std::copy(f.fwd_cuts.begin(), f.fwd_cuts.end(), forward_cuts);
    if (forward_rss) std::copy(f.fwd_rss.begin(), f.fwd_rss.end(), forward_rss);
    if (selected) std::copy(f.selected.begin(), f.selected.end(), selected);
    if (rss_per_subset) std::copy(f.rss_sub.begin(), f.rss_sub.end(), rss_per_subset);
    if (gcv_per_subset) std::copy(f.gcv_sub.begin(), f.gcv_sub.end(), gcv_per_subset);
    if (prune_terms) std::copy(f.prune_terms.begin(), f.prune_terms.end(), prune_terms);
    if (stats) std::copy_n(f.stats, 4, stats);
    return MHS_OK;
}

}  // extern "C"
