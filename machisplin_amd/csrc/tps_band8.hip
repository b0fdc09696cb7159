// The 8-column band route of the spline fit's GCV search (interface: tps_band8.h): every kernel of the blocked Householder
// reduction of B = Q2'KQ2 to bandwidth 8, the replay of a finished reduction on another right-hand side, the three
// back-transforms, and the host code that drives them.
#include <algorithm>
#include <vector>
#include "common.h"
#include "devmath.h"
#include "tps_band8.h"

namespace mhs {

// =============================================================================================
// Blocked reduction of B to a symmetric BAND of width BW (GCV path).  The classical Householder
// tridiagonalisation needs ~n dependent steps, each a full pass over the matrix plus a single-
// block latency kernel (n = 5000: 10^4 launches, 180 ms).  Reducing only to bandwidth BW = 8
// takes n/BW panel steps of four launches, each pass doing BW times the work, and the GCV
// criterion is then evaluated directly on the band (banded Cholesky + Takahashi trace on the host,
// tps_gcv_host.hip) -- no tridiagonal form, no eigenvalues.  Per panel at column c (t = m-c-BW):
//   band_panel_reg_kernel   Householder QR of P = B[c+BW:, c:c+BW] -> V (t x BW), T (compact WY),
//                           reflectors kept in place, R left in the band; g <- Q' g       (one block)
//   band_symm_kernel        Y = A22 V as split-K partial sums, and the partial sums of M = V'Y
//                           (A22 = B[c+BW:, c+BW:], read once, 8 B/element)
//   band_update_kernel<1>   S = sym(T' M T), W = Y T - 1/2 V S, first 64-column block of
//                           A22 <- A22 - V W' - W V' (= Q' A22 Q); the next panel starts behind it
//   band_update_kernel<0>   the other column blocks, on the second stream (read + write once)
// =============================================================================================

// -DMHS_PANEL_TRACE: s_memtime stamps per phase of band_panel_reg_kernel (first panel and the one at t ~ 2500),
// read back with mhs_debug_panel_trace(); how the reductions were found to be 80 % of the kernel.  Off by default.
#ifdef MHS_PANEL_TRACE
__device__ unsigned long long g_panel_trace[2][32];
__device__ int g_trace_slot = -1;
__device__ int g_trace_inner = 0;
#define PTRACE(k) do { if (threadIdx.x == 0 && g_trace_slot >= 0) g_panel_trace[g_trace_slot][k] = __builtin_readcyclecounter(); } while (0)
#define PTRACE_IN(k) do { if (threadIdx.x == 0 && g_trace_slot >= 0 && g_trace_inner) g_panel_trace[g_trace_slot][k] = __builtin_readcyclecounter(); } while (0)
#else
#define PTRACE(k) do {} while (0)
#define PTRACE_IN(k) do {} while (0)
#endif
// sum K per-thread values over the block; result in every thread.  lds: >= 17 * K doubles.
template <int K>
__device__ __forceinline__ void block_sum_vec(double (&v)[K], double *lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {  // thread k adds the per-wave partials of value k, in wave order
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += lds[w * K + threadIdx.x];
        lds[16 * K + threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = lds[16 * K + k];
}

__global__ __launch_bounds__(1024) void band_panel_kernel(double *__restrict__ A, int64_t ld, int c0, int r0,
                                                          int t, double *__restrict__ Vd, int64_t vs,
                                                          double *__restrict__ Tm, double *__restrict__ g) {
    __shared__ double lds[17 * 44];
    __shared__ double taus[BW];
    __shared__ double Ts[BW * BW];
    __shared__ double zs[BW];
    const int nref = min(BW, t - 1);
    double *P = A + (int64_t)c0 * ld + r0;  // P[i + j*ld]
    for (int j = 0; j < BW; ++j) {
        double *x = P + (int64_t)j * ld;
        if (j >= nref) {  // nothing left to annihilate in this column
            for (int i = threadIdx.x; i < t; i += blockDim.x) Vd[j * vs + i] = 0.0;
            if (threadIdx.x == 0) taus[j] = 0.0;
            __syncthreads();
            continue;
        }
        double part[1] = {0.0};
        for (int i = j + 1 + threadIdx.x; i < t; i += blockDim.x) part[0] = fma(x[i], x[i], part[0]);
        block_sum_vec<1>(part, lds);
        const double ss = part[0], alpha = x[j];
        __syncthreads();
        double beta = alpha, tau = 0.0, scal = 0.0;
        if (ss != 0.0) {
            beta = -copysign(sqrt(alpha * alpha + ss), alpha);
            tau = (beta - alpha) / beta;
            scal = 1.0 / (alpha - beta);
        }
        for (int i = threadIdx.x; i < t; i += blockDim.x) {
            const double vi = i < j ? 0.0 : (i == j ? 1.0 : x[i] * scal);
            Vd[j * vs + i] = vi;
            if (i == j) x[i] = beta; else if (i > j) x[i] = vi;
        }
        if (threadIdx.x == 0) taus[j] = tau;
        __syncthreads();
        // apply H_j to the remaining panel columns: s_k = v' P[:,k];  P[:,k] -= tau s_k v
        double sk[BW - 1];
#pragma unroll
        for (int k = 0; k < BW - 1; ++k) sk[k] = 0.0;
        for (int i = j + threadIdx.x; i < t; i += blockDim.x) {
            const double vi = Vd[j * vs + i];
#pragma unroll
            for (int k = 0; k < BW - 1; ++k)
                if (j + 1 + k < BW) sk[k] = fma(vi, P[(int64_t)(j + 1 + k) * ld + i], sk[k]);
        }
        block_sum_vec<BW - 1>(sk, lds);
        for (int i = j + threadIdx.x; i < t; i += blockDim.x) {
            const double vi = tau * Vd[j * vs + i];
#pragma unroll
            for (int k = 0; k < BW - 1; ++k)
                if (j + 1 + k < BW) P[(int64_t)(j + 1 + k) * ld + i] -= sk[k] * vi;
        }
        __syncthreads();
    }
    // G = V'V (upper triangle, 36 values) and sg = V'g (8 values) in one pass
    double acc[44];
#pragma unroll
    for (int k = 0; k < 44; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < t; i += blockDim.x) {
        double v[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) v[a] = Vd[a * vs + i];
        const double gi = g[i];
        int k = 0;
#pragma unroll
        for (int a = 0; a < BW; ++a)
#pragma unroll
            for (int b = a; b < BW; ++b) { acc[k] = fma(v[a], v[b], acc[k]); ++k; }
#pragma unroll
        for (int a = 0; a < BW; ++a) acc[36 + a] = fma(v[a], gi, acc[36 + a]);
    }
    block_sum_vec<44>(acc, lds);
    if (threadIdx.x == 0) {
        double G[BW][BW];
        int k = 0;
        for (int a = 0; a < BW; ++a)
            for (int b = a; b < BW; ++b) { G[a][b] = acc[k]; G[b][a] = acc[k]; ++k; }
        // larft: T upper triangular, T[r + BW*c]
        for (int e = 0; e < BW * BW; ++e) Ts[e] = 0.0;
        for (int j = 0; j < BW; ++j) {
            const double tj = taus[j];
            Ts[j + BW * j] = tj;
            for (int i = 0; i < j; ++i) {
                double sum = 0.0;
                for (int l = i; l < j; ++l) sum += Ts[i + BW * l] * G[l][j];
                Ts[i + BW * j] = -tj * sum;
            }
        }
        for (int e = 0; e < BW * BW; ++e) Tm[e] = Ts[e];
        // z = T' (V'g):  g <- g - V z   (Q' = I - V T' V')
        for (int a = 0; a < BW; ++a) {
            double sum = 0.0;
            for (int b = 0; b <= a; ++b) sum += Ts[b + BW * a] * acc[36 + b];
            zs[a] = sum;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < t; i += blockDim.x) {
        double gi = g[i];
#pragma unroll
        for (int a = 0; a < BW; ++a) gi -= Vd[a * vs + i] * zs[a];
        g[i] = gi;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// TALL panels (t > PANEL_THREADS * PANEL_RPT rows: the first panels of a fit with more than ~5 000 unknowns, e.g. the
// 20 000-station fit of BASELINE config 5).  The single-block streaming kernel above moves the panel at what ONE block
// can stream (~35 GB/s: 0.77 ms per panel at t = 15 000, and there are 1 900 of them at n = 20 000); here a panel is
// factorised by a short chain of MANY-block launches instead -- one per Householder step, each a single pass over the
// panel that applies reflector J and, in the same pass, forms the partial dot products reflector J + 1 needs:
//   tall_dots0_kernel            S_p = sum_{i > 0} x[i][0] x[i][p] per row block; row 0 published
//   tall_step_kernel (x BW)      totals of step J's partials -> beta, tau, v = scal x[:, J], w_p = x[J][p] + scal S_p;
//                                x[:, p] -= tau w_p v; dense V column J; partials and pivot row of step J + 1
//   tall_gram_kernel             partials of G = V'V (upper triangle) and V'g
//   tall_finish_kernel           every block: T = larft(tau, G), z = T'(V'g), its rows of g -= V z; block 0 stores T
// Every block re-derives the step's scalars from the same partials in the same order (no single-block launch in the
// chain).  11 launches per panel, ~6 us each.
// ---------------------------------------------------------------------------------------------------------------
constexpr int TALL_RPB = 256;                   // rows per block: one row per thread -- 60-80 blocks for a 15-20 000-row panel
constexpr int TALL_MAXBLK = 256;                // up to 65 536 rows
struct TallScratch {                            // device scratch of one fit lane
    double part[2][TALL_MAXBLK][BW];            // partial dot products, ping-pong between steps
    double rowj[BW + 1][BW];                    // pivot row J as it is when step J starts (entries p >= J)
    double taus[BW];
    double gpart[TALL_MAXBLK][44];              // partials of G (36) and V'g (8)
};

// sum BW per-thread values over a 256-thread block (fixed order), result in every thread
__device__ __forceinline__ void block_sum8(double (&v)[BW], double (*lds)[BW]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < BW; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < BW; ++k) lds[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BW; ++k) v[k] = (lds[0][k] + lds[1][k]) + (lds[2][k] + lds[3][k]);
}

__global__ __launch_bounds__(256) void tall_dots0_kernel(const double *__restrict__ A, int64_t ld, int c0, int r0, int t,
                                                         TallScratch *__restrict__ sc) {
    __shared__ double lds[4][BW];
    const double *P = A + (int64_t)c0 * ld + r0;
    double acc[BW];
#pragma unroll
    for (int p = 0; p < BW; ++p) acc[p] = 0.0;
#pragma unroll
    for (int r = 0; r < TALL_RPB / 256; ++r) {
        const int i = blockIdx.x * TALL_RPB + r * 256 + threadIdx.x;
        if (i < t && i > 0) {
            const double x0 = P[i];
#pragma unroll
            for (int p = 0; p < BW; ++p) acc[p] = fma(x0, P[(int64_t)p * ld + i], acc[p]);
        }
    }
    block_sum8(acc, lds);
    if (threadIdx.x < BW) sc->part[0][blockIdx.x][threadIdx.x] = acc[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x < BW) sc->rowj[0][threadIdx.x] = P[(int64_t)threadIdx.x * ld];
}

__global__ __launch_bounds__(256) void tall_step_kernel(double *__restrict__ A, int64_t ld, int c0, int r0, int t, int J,
                                                        double *__restrict__ Vd, int64_t vs, TallScratch *__restrict__ sc) {
    __shared__ double lds[4][BW];
    const int nblk = gridDim.x, ph = J & 1;
    // totals of this step's dot products: thread b takes row block b's partials, then a block sum (every block, same order)
    double S[BW];
#pragma unroll
    for (int p = 0; p < BW; ++p) S[p] = (int)threadIdx.x < nblk ? sc->part[ph][threadIdx.x][p] : 0.0;
    block_sum8(S, lds);
    __syncthreads();
    double xj[BW];
#pragma unroll
    for (int p = 0; p < BW; ++p) xj[p] = sc->rowj[J][p];
    double alpha = 0.0, ss = 0.0;
#pragma unroll
    for (int p = 0; p < BW; ++p) if (p == J) { alpha = xj[p]; ss = S[p]; }
    double beta = alpha, tau = 0.0, scal = 0.0;
    if (ss != 0.0) {
        beta = -copysign(sqrt(alpha * alpha + ss), alpha);
        tau = (beta - alpha) / beta;
        scal = 1.0 / (alpha - beta);
    }
    double tw[BW];      // tau w_p for the columns still to be updated (p > J), 0 otherwise
#pragma unroll
    for (int p = 0; p < BW; ++p) tw[p] = p > J ? tau * fma(scal, S[p], xj[p]) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->taus[J] = tau;
    double *P = A + (int64_t)c0 * ld + r0;
    double acc[BW];
#pragma unroll
    for (int p = 0; p < BW; ++p) acc[p] = 0.0;
#pragma unroll
    for (int r = 0; r < TALL_RPB / 256; ++r) {
        const int i = blockIdx.x * TALL_RPB + r * 256 + threadIdx.x;
        if (i >= t) continue;
        double x[BW];
#pragma unroll
        for (int p = 0; p < BW; ++p) x[p] = P[(int64_t)p * ld + i];
        double v = 0.0;
        if (i == J) {
            v = 1.0;
#pragma unroll
            for (int p = 0; p < BW; ++p) { if (p == J) x[p] = beta; else if (p > J) x[p] -= tw[p]; }
        } else if (i > J) {
#pragma unroll
            for (int p = 0; p < BW; ++p) if (p == J) v = x[p] * scal;
#pragma unroll
            for (int p = 0; p < BW; ++p) { if (p == J) x[p] = v; else if (p > J) x[p] -= tw[p] * v; }
        }
        if (i >= J) {
#pragma unroll
            for (int p = 0; p < BW; ++p) if (p >= J) P[(int64_t)p * ld + i] = x[p];
        }
        Vd[(int64_t)J * vs + i] = v;
        if (J + 1 < BW) {
            if (i == J + 1) {
#pragma unroll
                for (int p = 0; p < BW; ++p) sc->rowj[J + 1][p] = x[p];
            }
            if (i > J + 1) {
                double xn = 0.0;
#pragma unroll
                for (int p = 0; p < BW; ++p) if (p == J + 1) xn = x[p];
#pragma unroll
                for (int p = 0; p < BW; ++p) if (p > J) acc[p] = fma(xn, x[p], acc[p]);
            }
        }
    }
    if (J + 1 < BW) {
        block_sum8(acc, lds);
        if (threadIdx.x < BW) sc->part[ph ^ 1][blockIdx.x][threadIdx.x] = acc[threadIdx.x];
    }
}

__global__ __launch_bounds__(256) void tall_gram_kernel(const double *__restrict__ Vd, int64_t vs, int t,
                                                        const double *__restrict__ g, TallScratch *__restrict__ sc) {
    __shared__ double lds[4][44];
    double acc[44];
#pragma unroll
    for (int k = 0; k < 44; ++k) acc[k] = 0.0;
#pragma unroll
    for (int r = 0; r < TALL_RPB / 256; ++r) {
        const int i = blockIdx.x * TALL_RPB + r * 256 + threadIdx.x;
        if (i >= t) continue;
        double v[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) v[a] = Vd[(int64_t)a * vs + i];
        const double gi = g[i];
        int k = 0;
#pragma unroll
        for (int a = 0; a < BW; ++a)
#pragma unroll
            for (int b = a; b < BW; ++b) { acc[k] = fma(v[a], v[b], acc[k]); ++k; }
#pragma unroll
        for (int a = 0; a < BW; ++a) acc[36 + a] = fma(v[a], gi, acc[36 + a]);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 44; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 44; ++k) lds[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 44) sc->gpart[blockIdx.x][threadIdx.x] = (lds[0][threadIdx.x] + lds[1][threadIdx.x]) + (lds[2][threadIdx.x] + lds[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void tall_finish_kernel(const double *__restrict__ Vd, int64_t vs, int t, double *__restrict__ g,
                                                          double *__restrict__ Tm, const TallScratch *__restrict__ sc) {
    __shared__ double tot[44], Ts[BW * BW], zs[BW], grp[5][44];
    const int nblk = gridDim.x;
    if (threadIdx.x < 220) {      // five groups of 44 threads stride over the row blocks, then the groups are added in order
        const int k = threadIdx.x % 44, gq = threadIdx.x / 44;
        double s = 0.0;
        for (int b = gq; b < nblk; b += 5) s += sc->gpart[b][k];
        grp[gq][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 44) tot[threadIdx.x] = ((grp[0][threadIdx.x] + grp[1][threadIdx.x]) + (grp[2][threadIdx.x] + grp[3][threadIdx.x])) + grp[4][threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double G[BW][BW];
        int k = 0;
        for (int a = 0; a < BW; ++a)
            for (int b = a; b < BW; ++b) { G[a][b] = tot[k]; G[b][a] = tot[k]; ++k; }
        for (int e = 0; e < BW * BW; ++e) Ts[e] = 0.0;
        for (int j = 0; j < BW; ++j) {          // larft: T upper triangular, T[r + BW c]
            const double tj = sc->taus[j];
            Ts[j + BW * j] = tj;
            for (int i = 0; i < j; ++i) {
                double sum = 0.0;
                for (int l = i; l < j; ++l) sum += Ts[i + BW * l] * G[l][j];
                Ts[i + BW * j] = -tj * sum;
            }
        }
        for (int a = 0; a < BW; ++a) {          // z = T' (V'g)
            double sum = 0.0;
            for (int b = 0; b <= a; ++b) sum += Ts[b + BW * a] * tot[36 + b];
            zs[a] = sum;
        }
        if (blockIdx.x == 0) for (int e = 0; e < BW * BW; ++e) Tm[e] = Ts[e];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TALL_RPB / 256; ++r) {
        const int i = blockIdx.x * TALL_RPB + r * 256 + threadIdx.x;
        if (i >= t) continue;
        double gi = g[i];
#pragma unroll
        for (int a = 0; a < BW; ++a) gi -= Vd[(int64_t)a * vs + i] * zs[a];
        g[i] = gi;
    }
}

// Register-resident variant for t <= PANEL_THREADS * PANEL_RPT rows: the whole t x BW panel (320 KB at
// t = 5000) lives in the register file of ONE CU -- each thread owns PANEL_RPT rows of all BW
// columns -- so the BW Householder steps touch global memory only to load and store the panel.
// (The streaming version above is latency-bound: a single block keeps ~8 KB of loads in flight.)
// The kernel is a chain of BW + 2 block reductions and nothing else hides their latency, so each one
// is pared down to: DPP row/wave reduction (no LDS crossbar traffic), lane 63 of every wave stores its
// partials, ONE barrier, then every wave adds the partials itself in its first lanes (fixed order) and
// broadcasts the totals with v_readlane -- the partial buffers alternate, so no second barrier
// guards their reuse, and everything a step derives from the totals (next pivot, R entries, the
// downdated column norms) is recomputed by every wave instead of being published through LDS.
#ifndef PANEL_RPT_V
#define PANEL_RPT_V 10
#define PANEL_THREADS_V 512
#endif
constexpr int PANEL_RPT = PANEL_RPT_V;
constexpr int PANEL_THREADS = PANEL_THREADS_V;
// Shorter panels take fewer waves (1 .. 8 of them, 640 rows each): every reduction then adds fewer partials behind
// a cheaper barrier, and a panel of up to 640 rows is reduced inside one wave (t = 197: 24.7 -> 13.4 us).
template <int PANEL_WAVES>
struct PanelShared {
    double part[2][PANEL_WAVES][BW];   // per-wave partial sums of a reduction (alternating buffers)
    double rowj[2][BW];                // entries of the pivot row before the step's update (positions 1..BW-1)
    double nxt[2][2];                  // row J+1 before the update: its entries in the pivot column and the next one
    double cn0[PANEL_WAVES][BW];       // per wave: initial squared column norms ...
    double cn[PANEL_WAVES][BW];        // ... and the norms downdated by the R entries formed so far
    double Gs[BW][BW];                 // Gs[l][j] = v_l' v_j (l < j)
    double taus[BW];
};

// The BW Householder steps of the register-resident panel as ONE loop body: the columns are kept
// rotated so that the pivot column is always x[.][0], the columns still to be updated follow it and
// the reflectors already formed sit at the end (step J: positions 1..BW-1-J are columns J+1.., positions
// BW-J.. are v_0..v_{J-1}); after the step the columns rotate left by one, and BW rotations restore the
// original order.  Every index into x[][] stays a compile-time constant (the panel lives in VGPRs)
// while the code is BW times smaller than BW specialised steps -- the kernel is one block, launched
// ~n/BW times on whichever CU is free, so its instruction footprint is fetched cold every time.
// Row i = tid + PANEL_THREADS r: only r = 0 can hold rows on or above the diagonal; rows past the end
// of the panel hold zeros and stay zero.
//
// One reduction per step, over raw products: S_p = sum_{i > J} x[i][0] x[i][p].  With v = e_J + scal x[J+1:][0]
// the step needs w_p = v' x[:, p] = x[J][p] + scal S_p (for a reflector position: v_l' v_J, since v_l[J] is what
// the panel stores there), so beta / tau / scal (a square root and two divisions) are off the critical path of
// the reduction.  Column norms are computed once and DOWNDATED (LAPACK's dlaqps idea): below row J the
// squared norm of column J is its initial value minus the squares of its entries in rows 0..J-1, the R entries,
// which every wave recomputes from the step's totals; when the difference cancels (below 1 % of the initial
// norm) the norm is summed afresh.
template <int PANEL_WAVES>
__device__ __forceinline__ int panel_steps(double (&x)[PANEL_RPT][BW], int nref, PanelShared<PANEL_WAVES> &sh) {
    const int i0 = threadIdx.x;     // the row held in x[0][.]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int ph = 0;
    double alpha;
    {
        double part[BW];
#pragma unroll
        for (int p = 0; p < BW; ++p) {
            part[p] = 0.0;
#pragma unroll
            for (int r = 0; r < PANEL_RPT; ++r) part[p] = fma(x[r][p], x[r][p], part[p]);
        }
        if (i0 == 0) sh.nxt[ph][1] = x[0][0];
        wave_publish<BW>(part, sh.part[ph]);
        __syncthreads();
        const double tot = block_total<BW, PANEL_WAVES>(sh.part[ph]);
        if (lane < BW) { sh.cn0[wave][lane] = tot; sh.cn[wave][lane] = tot; }
        alpha = sh.nxt[ph][1];
        ph ^= 1;
    }
    PTRACE(2);
#pragma unroll 1
    for (int J = 0; J < BW; ++J) {
        PTRACE(3 + J);
#ifdef MHS_PANEL_TRACE
        if (threadIdx.x == 0) g_trace_inner = (J == 3);
#endif
        if (J < nref) {
            PTRACE_IN(15);
            // raw products with the pivot column, rows below J only
            double red[BW - 1];
#pragma unroll
            for (int p = 1; p < BW; ++p) red[p - 1] = i0 > J ? x[0][0] * x[0][p] : 0.0;
#pragma unroll
            for (int r = 1; r < PANEL_RPT; ++r) {
#pragma unroll
                for (int p = 1; p < BW; ++p) red[p - 1] = fma(x[r][0], x[r][p], red[p - 1]);
            }
            if (i0 == J) {
#pragma unroll
                for (int p = 1; p < BW; ++p) sh.rowj[ph][p] = x[0][p];
            }
            if (i0 == J + 1) { sh.nxt[ph][0] = x[0][0]; sh.nxt[ph][1] = x[0][1]; }
            PTRACE_IN(16);
            wave_publish<BW - 1>(red, sh.part[ph]);
            PTRACE_IN(17);
            const double c0 = sh.cn0[wave][J];
            double ss = sh.cn[wave][J] - alpha * alpha;
            if (!(ss > 0.01 * c0)) {   // uniform
                double fresh[1] = {i0 > J ? x[0][0] * x[0][0] : 0.0};
#pragma unroll
                for (int r = 1; r < PANEL_RPT; ++r) fresh[0] = fma(x[r][0], x[r][0], fresh[0]);
                __syncthreads();     // the step's own partials sit in part[ph]: use the other buffer, fenced
                wave_publish<1>(fresh, sh.part[ph ^ 1]);
                __syncthreads();
                ss = lane_value(block_total<1, PANEL_WAVES>(sh.part[ph ^ 1]), 0);
            }
            double beta = alpha, tau = 0.0, scal = 0.0;
            if (ss != 0.0) {
                beta = -copysign(sqrt(alpha * alpha + ss), alpha);
                tau = (beta - alpha) / beta;
                scal = 1.0 / (alpha - beta);
            }
            PTRACE_IN(18);
            __syncthreads();
            PTRACE_IN(19);
            // lane k < BW-1 of every wave: total k, i.e. position p = k + 1
            const int k = lane < BW - 1 ? lane : BW - 2;
            const double xj = sh.rowj[ph][k + 1];
            const double wk = fma(scal, block_total<BW - 1, PANEL_WAVES>(sh.part[ph]), xj);
            const bool live = k + 1 < BW - J;              // a column still to be updated (else: reflector k+1+J-BW)
            const double twk = live ? tau * wk : 0.0;
            if (live && lane < BW - 1) {                   // R entry of column J+1+k in row J: downdate its norm
                const double rk = xj - twk;
                sh.cn[wave][J + 1 + k] -= rk * rk;
            }
            if (wave == 0 && lane < BW - 1 && !live) sh.Gs[k + 1 + J - BW][J] = wk;
            if (threadIdx.x == 0) sh.taus[J] = tau;
            // next pivot: row J+1 of position 1 after the update (meaningless, and unused, after the last step)
            const double vn = sh.nxt[ph][0] * scal;
            const double an = sh.nxt[ph][1] - twk * vn;    // lane 0's twk
            alpha = lane_value(an, 0);
            double tw[BW - 1];
#pragma unroll
            for (int p = 1; p < BW; ++p) tw[p - 1] = lane_value(twk, p - 1);
            ph ^= 1;
            PTRACE_IN(20);
            // apply: rows above J untouched, row J has v = 1, rows below v = scal x
            if (i0 == J) {
                x[0][0] = beta;
#pragma unroll
                for (int p = 1; p < BW; ++p) x[0][p] -= tw[p - 1];
            } else if (i0 > J) {
                const double v0 = x[0][0] * scal;
                x[0][0] = v0;
#pragma unroll
                for (int p = 1; p < BW; ++p) x[0][p] -= tw[p - 1] * v0;
            }
#pragma unroll
            for (int r = 1; r < PANEL_RPT; ++r) {
                const double vr = x[r][0] * scal;
                x[r][0] = vr;
#pragma unroll
                for (int p = 1; p < BW; ++p) x[r][p] -= tw[p - 1] * vr;
            }
            PTRACE_IN(21);
        } else if (threadIdx.x == 0) {   // uniform: nothing left to annihilate; H_J = I
            sh.taus[J] = 0.0;
            for (int l = 0; l < BW; ++l) sh.Gs[l][J] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < PANEL_RPT; ++r) {
            const double first = x[r][0];
#pragma unroll
            for (int p = 0; p + 1 < BW; ++p) x[r][p] = x[r][p + 1];
            x[r][BW - 1] = first;
        }
    }
    return ph;
}

template <int PANEL_WAVES>
__global__ __launch_bounds__(64 * PANEL_WAVES) void band_panel_reg_kernel(double *__restrict__ A, int64_t ld, int c0,
                                                                          int r0, int t, double *__restrict__ Vd,
                                                                          int64_t vs, double *__restrict__ Tm,
                                                                          double *__restrict__ g, double *__restrict__ aux) {
    constexpr int PANEL_THREADS = 64 * PANEL_WAVES;   // shadows the largest form's constant
    __shared__ PanelShared<PANEL_WAVES> sh;
#ifdef MHS_PANEL_TRACE
    if (threadIdx.x == 0) g_trace_slot = (c0 == 3) ? 0 : ((t >= 2497 && t < 2505) ? 1 : -1);
    __syncthreads();
#endif
    PTRACE(0);
    const int nref = min(BW, t - 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *P = A + (int64_t)c0 * ld + r0;
    double x[PANEL_RPT][BW];   // x[r][j] = P[tid + PANEL_THREADS r][j]
    // unconditional loads at a clamped row (one batch in flight), zeroed past the end of the panel
#pragma unroll
    for (int r = 0; r < PANEL_RPT; ++r) {
        const int i = threadIdx.x + PANEL_THREADS * r;
        const unsigned ii = i < t ? (unsigned)i : 0u;
#pragma unroll
        for (int j = 0; j < BW; ++j) { const double *Pj = P + (int64_t)j * ld; x[r][j] = Pj[ii]; }
    }
#pragma unroll
    for (int r = 0; r < PANEL_RPT; ++r) {
        if ((int)threadIdx.x + PANEL_THREADS * r >= t) {
#pragma unroll
            for (int j = 0; j < BW; ++j) x[r][j] = 0.0;
        }
    }
    PTRACE(1);
    const int ph = panel_steps(x, nref, sh);   // the partial buffer the next reduction may use
    PTRACE(11);
    double z[BW];   // z = T' (V'g), uniform
    {   // sg = V' g (g as it was on entry)
        double sg[BW];
#pragma unroll
        for (int j = 0; j < BW; ++j) sg[j] = 0.0;
#pragma unroll
        for (int r = 0; r < PANEL_RPT; ++r) {
            const int i = threadIdx.x + PANEL_THREADS * r;
            const double gi = i < t ? g[(unsigned)i] : 0.0;
#pragma unroll
            for (int j = 0; j < BW; ++j) {
                // rows of r > 0 lie below every diagonal entry (and are zero when the panel is shorter)
                const double vj = r > 0 ? x[r][j] : ((j >= nref || i < j || i >= t) ? 0.0 : (i == j ? 1.0 : x[r][j]));
                sg[j] = fma(vj, gi, sg[j]);
            }
        }
        wave_publish<BW>(sg, sh.part[ph]);
        __syncthreads();
        PTRACE(12);
        // z = T' sg without T: inv(T) is upper triangular with 1/tau on the diagonal and G above it, so
        // z_a = tau_a (sg_a - sum_{b < a} G[b][a] z_b).  Every wave runs the recurrence in its lanes 0..BW-1
        // (lane b holds z_b and row b of G; the sum is a DPP reduction over the 8 lanes).
        const int b = lane < BW ? lane : BW - 1;
        const double sgb = block_total<BW, PANEL_WAVES>(sh.part[ph]), taub = sh.taus[b];
        double zb = 0.0;
#pragma unroll
        for (int a = 0; a < BW; ++a) {
            double c = b < a ? sh.Gs[b][a] * zb : 0.0;
            c += dpp_fetch<0xB1, 0xf>(c);
            c += dpp_fetch<0x4E, 0xf>(c);
            c += dpp_fetch<0x141, 0xf>(c);
            if (b == a) zb = taub * (sgb - c);
        }
#pragma unroll
        for (int a = 0; a < BW; ++a) z[a] = lane_value(zb, a);
    }
    PTRACE(13);
    // store the panel (R on/above its diagonal, reflectors below), the dense V, and g <- Q' g
#pragma unroll
    for (int r = 0; r < PANEL_RPT; ++r) {
        const int i = threadIdx.x + PANEL_THREADS * r;
        if (i < t) {
            double gi = g[(unsigned)i];
#pragma unroll
            for (int j = 0; j < BW; ++j) {
                double *Pj = P + (int64_t)j * ld, *Vj = Vd + (int64_t)j * vs;
                Pj[(unsigned)i] = x[r][j];
                const double vj = r > 0 ? x[r][j] : ((j >= nref || i < j) ? 0.0 : (i == j ? 1.0 : x[r][j]));
                Vj[(unsigned)i] = vj;
                gi -= vj * z[j];
            }
            g[(unsigned)i] = gi;
        }
    }
    // what "Q' onto another right-hand side" needs to repeat this panel's update of g bit for bit (band_qt_kernel; the
    // reduction cache of the band route): tau_0..7 and G = (v_l'v_j)
    if (aux) for (int e = threadIdx.x; e < BW + BW * BW; e += PANEL_THREADS) aux[e] = e < BW ? sh.taus[e] : sh.Gs[(e - BW) / BW][(e - BW) % BW];
    if (wave == 0) {
        // larft, after the stores so that the panel's registers are free: lane i < BW forms row i of T
        // (T[i][j] = -tau_j sum_{l=i}^{j-1} T[i][l] G[l][j], a recurrence along the row only)
        const int i = lane < BW ? lane : BW - 1;
        double Trow[BW];
#pragma unroll
        for (int j = 0; j < BW; ++j) {
            const double tj = sh.taus[j];
            double sum = 0.0;
#pragma unroll
            for (int l = 0; l < j; ++l) sum += (l >= i ? Trow[l] : 0.0) * sh.Gs[l][j];
            Trow[j] = j < i ? 0.0 : (j == i ? tj : -tj * sum);
        }
        if (lane < BW) {
#pragma unroll
            for (int j = 0; j < BW; ++j) Tm[i + BW * j] = Trow[j];
        }
    }
    PTRACE(14);
}
#ifdef MHS_PANEL_TRACE
extern "C" __attribute__((visibility("default"))) int mhs_debug_panel_trace(unsigned long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_panel_trace), sizeof(unsigned long long) * 64);
}
#endif

// g <- Q'g for ANOTHER right-hand side with the reflectors of a finished band reduction (mhs_tps_reduction_cache, band
// route: the other response layers of a station table, V73:203 -- B = Q2'KQ2 depends on the coordinates only).  One block
// walks the panels in order and repeats, per panel, exactly what band_panel_reg_kernel did to g: the same rows per
// thread (i = tid + 64 NW r with the panel's own wave count NW), the same fma chain for V'g, the same lane-swap / DPP
// reduction tree, the same recurrence for z = T'(V'g) from tau and G = (v_l'v_j) (stored by the panel kernel: aux), the
// same multiply-subtract order -- so the rotated g, hence lambda, c and d, equal the full fit's bit for bit.
template <int NW>
__device__ __forceinline__ void qt_panel(const double *__restrict__ P, int64_t ld, int t, const double *__restrict__ aux,
                                         double *__restrict__ g, double (*part)[BW]) {
    constexpr int PT = 64 * NW;
    const int nref = min(BW, t - 1);
    const int lane = threadIdx.x & 63;
    const bool on = (int)threadIdx.x < PT;
    double v[PANEL_RPT][BW], gi[PANEL_RPT];
    if (on) {
#pragma unroll
        for (int r = 0; r < PANEL_RPT; ++r) {
            const int i = threadIdx.x + PT * r;
            const unsigned ii = i < t ? (unsigned)i : 0u;
#pragma unroll
            for (int j = 0; j < BW; ++j) v[r][j] = P[(int64_t)j * ld + ii];
            gi[r] = i < t ? g[ii] : 0.0;
        }
        double sg[BW];
#pragma unroll
        for (int j = 0; j < BW; ++j) sg[j] = 0.0;
#pragma unroll
        for (int r = 0; r < PANEL_RPT; ++r) {
            const int i = threadIdx.x + PT * r;
#pragma unroll
            for (int j = 0; j < BW; ++j) {
                const double vj = i >= t ? 0.0 : (r > 0 ? v[r][j] : ((j >= nref || i < j) ? 0.0 : (i == j ? 1.0 : v[r][j])));
                v[r][j] = vj;
                sg[j] = fma(vj, gi[r], sg[j]);
            }
        }
        wave_publish<BW>(sg, part);
    }
    __syncthreads();
    if (on) {
        const int b = lane < BW ? lane : BW - 1;
        const double sgb = block_total<BW, NW>(part), taub = aux[b];
        double zb = 0.0;
#pragma unroll
        for (int a = 0; a < BW; ++a) {
            double c = b < a ? aux[BW + b * BW + a] * zb : 0.0;
            c += dpp_fetch<0xB1, 0xf>(c);
            c += dpp_fetch<0x4E, 0xf>(c);
            c += dpp_fetch<0x141, 0xf>(c);
            if (b == a) zb = taub * (sgb - c);
        }
        double z[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) z[a] = lane_value(zb, a);
#pragma unroll
        for (int r = 0; r < PANEL_RPT; ++r) {
            const int i = threadIdx.x + PT * r;
            if (i < t) {
                double x = gi[r];
#pragma unroll
                for (int j = 0; j < BW; ++j) x -= v[r][j] * z[j];
                g[(unsigned)i] = x;
            }
        }
    }
    __syncthreads();      // g of the next panel's rows is in place, the partial buffer may be reused
}

__global__ __launch_bounds__(PANEL_THREADS) void band_qt_kernel(const double *__restrict__ A, int64_t ld, int off0, int m, int npanels,
                                                                const double *__restrict__ aux, double *__restrict__ g) {
    __shared__ double part[PANEL_THREADS / 64][BW];
    for (int p = 0; p < npanels; ++p) {
        const int c = p * BW, t = m - c - BW;
        const double *P = A + (int64_t)(off0 + c) * ld + off0 + c + BW;
        const int nw = t <= 256 * PANEL_RPT ? (t + 64 * PANEL_RPT - 1) / (64 * PANEL_RPT) : PANEL_THREADS / 64;   // band8_reduce's choice
        const double *ax = aux + (int64_t)p * PANEL_AUX;
        double *gp = g + c + BW;
        switch (nw) {
            case 1: qt_panel<1>(P, ld, t, ax, gp, part); break;
            case 2: qt_panel<2>(P, ld, t, ax, gp, part); break;
            case 3: qt_panel<3>(P, ld, t, ax, gp, part); break;
            case 4: qt_panel<4>(P, ld, t, ax, gp, part); break;
            default: qt_panel<PANEL_THREADS / 64>(P, ld, t, ax, gp, part); break;
        }
    }
}

// Sum 64 per-lane values over the wave: two halving stages with the gfx950 lane-swap instructions
// (v_permlane32_swap / v_permlane16_swap exchange half-waves / odd and even rows between two registers, so
// each output costs two swaps and an add), then a DPP reduction within the rows of 16 lanes.  Afterwards
// every lane of row r = lane >> 4 holds, in w[i], the total of value 4 i + rho(r), rho = {0, 2, 1, 3}.
// ~340 VALU instructions and no LDS traffic, against 768 ds_bpermute for 64 butterfly sums.
__device__ __forceinline__ int wave_sum64_slot(int row, int i) { return 4 * i + ((row & 1) << 1 | (row >> 1)); }
__device__ __forceinline__ void wave_sum64(const double (&v)[64], double (&w)[16]) {
    double u[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) u[i] = swap_add32(v[2 * i], v[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = swap_add16(u[2 * i], u[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        w[i] += dpp_fetch<0xB1, 0xf>(w[i]);
        w[i] += dpp_fetch<0x4E, 0xf>(w[i]);
        w[i] += dpp_fetch<0x141, 0xf>(w[i]);
        w[i] += dpp_fetch<0x140, 0xf>(w[i]);
    }
}

// Y = A22 V as split-K partial sums: block (cg, sp) owns 32 columns (8 per wave) and one of nsplit = gridDim.y
// row ranges; lanes run over rows (barrier-free loop, 16 loads per lane and 64 rows in flight).
// Ypart[sp][j][i] partial sums are added up by the consumers; the block also emits its share of M = V'Y
// (64 values) so that S = T'(V'Y)T needs no second pass over Y.
constexpr int SYMM_MAX_SPLITS = 8;
constexpr int SYMM_CPW = 8;              // columns per wave
constexpr int SYMM_COLS = 4 * SYMM_CPW;  // per block
// Two row ranges measured best at n = 5000 (more blocks shorten this kernel but every consumer of Y and M then
// adds more partials: 1 -> 85.8, 2 -> 81.6, 3 -> 82.5, 4 -> 84.3, 8 -> 91.3 ms per fit) -- except where two ranges
// make slightly more than one block per CU: a block streams its columns at ~35 GB/s whatever else runs, so
// 264 blocks on 256 CUs take twice as long as 256 (t = 4197: 39 us, t = 3397: 20 us).  Then the split count with
// the fewest (rounds of 256 blocks) x (rows per block) is taken.
static inline int symm_splits(int t) {
    const int ncg = (t + SYMM_COLS - 1) / SYMM_COLS;
    int want = 2;
    if (ncg * 2 > 256) {
        double best = 1e30;
        for (int sp = 2; sp <= SYMM_MAX_SPLITS; ++sp) {
            const double cost = (double)((ncg * sp + 255) / 256) / sp;
            if (cost < best - 1e-12) { best = cost; want = sp; }
        }
    }
    return std::max(1, std::min(want, (t + 63) / 64));
}

__global__ __launch_bounds__(256) void band_symm_kernel(const double *__restrict__ A, int64_t ld, int r0, int t,
                                                        const double *__restrict__ Vd, int64_t vs,
                                                        double *__restrict__ Ypart, double *__restrict__ Mpart) {
    __shared__ double Ms[4][BW * BW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col0 = blockIdx.x * SYMM_COLS + wave * SYMM_CPW;
    const int rows_per = ((t + (int)gridDim.y - 1) / (int)gridDim.y + 63) & ~63;
    const int rbeg = blockIdx.y * rows_per, rend = min(t, rbeg + rows_per);
    const int ncol_ok = min(SYMM_CPW, t - col0);   // <= 0: this wave has no column
    double acc[SYMM_CPW * BW];   // acc[c * BW + j]
#pragma unroll
    for (int e = 0; e < SYMM_CPW * BW; ++e) acc[e] = 0.0;
    const double *a0 = A + (int64_t)r0 * ld + r0;
    // lane = row: the lane's V row comes straight from global memory (V is t x 8, L2-resident), so the loop has
    // no barrier and the loads of the next 64 rows are in flight while these are multiplied.  Rows and columns
    // past the end are read at a clamped index and multiplied by zero.
    const double *ac[SYMM_CPW];
#pragma unroll
    for (int c = 0; c < SYMM_CPW; ++c) ac[c] = a0 + (int64_t)(col0 + (c < ncol_ok ? c : 0)) * ld;
#pragma unroll 2
    for (int rb = ncol_ok > 0 ? rbeg : rend; rb < rend; rb += 64) {
        const int r = rb + lane;
        const unsigned rr = (unsigned)min(r, rend - 1);
        const double keep = r < rend ? 1.0 : 0.0;
        double a[SYMM_CPW], v[BW];
#pragma unroll
        for (int c = 0; c < SYMM_CPW; ++c) a[c] = ac[c][rr];
#pragma unroll
        for (int j = 0; j < BW; ++j) v[j] = Vd[(int64_t)j * vs + rr] * keep;
#pragma unroll
        for (int j = 0; j < BW; ++j)
#pragma unroll
            for (int c = 0; c < SYMM_CPW; ++c) acc[c * BW + j] = fma(a[c], v[j], acc[c * BW + j]);
    }
    double w[16];
    wave_sum64(acc, w);
    // row r of the wave now holds y_c[j] for every column c and j in {rho, rho + 4} (value 4 i + rho: c = i / 2,
    // j = rho + 4 (i & 1)).  Its first lane stores them; lanes a = 0..7 of the row form this wave's share of
    // M = V'Y for those two j: M[a][j] += V[a][col c] y_c[j].
    const int row = lane >> 4, rho = (row & 1) << 1 | (row >> 1), la = lane & 15;
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int c = 0; c < SYMM_CPW; ++c) {
        if (c < ncol_ok) {
            if (la == 0) {
                Ypart[(int64_t)blockIdx.y * BW * vs + (int64_t)rho * vs + col0 + c] = w[2 * c];
                Ypart[(int64_t)blockIdx.y * BW * vs + (int64_t)(rho + 4) * vs + col0 + c] = w[2 * c + 1];
            }
            const double va = Vd[(int64_t)(la & 7) * vs + col0 + c];
            m0 = fma(va, w[2 * c], m0);
            m1 = fma(va, w[2 * c + 1], m1);
        }
    }
    if (la < BW) { Ms[wave][la + BW * rho] = m0; Ms[wave][la + BW * (rho + 4)] = m1; }
    __syncthreads();
    if (threadIdx.x < BW * BW)
        Mpart[(int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * (BW * BW) + threadIdx.x] =
            (Ms[0][threadIdx.x] + Ms[1][threadIdx.x]) + (Ms[2][threadIdx.x] + Ms[3][threadIdx.x]);
}

// A22 <- A22 - V W' - W V' on 64 x 64 tiles, W = Y T - 1/2 V S.  Bitwise symmetric.  The launch for the first
// column block (FIRST; it is on the critical path, the next panel waits for it) forms W for its tile's row set
// from the split-K partial sums of Y and also stores it; the launch for the other column blocks, which runs
// behind it on the second stream, just reads W.  Every FIRST block also forms S = sym(T' M T), M = V'Y = the sum
// of the symmetric product's Mpart blocks, for itself (same order in every block, hence the same bits): a
// few hundred L2-resident loads per thread cost less than a single-block kernel in the dependency chain.
template <bool FIRST>
__global__ __launch_bounds__(256) void band_update_kernel(double *__restrict__ A, int64_t ld, int r0, int t,
                                                          const double *__restrict__ Vd,
                                                          const double *__restrict__ Ypart, int nsplit,
                                                          int64_t vs, const double *__restrict__ Tm,
                                                          const double *__restrict__ Mpart, int nparts,
                                                          double *__restrict__ Wd) {
    __shared__ double Vs[2][64][BW + 1], Ws[2][64][BW + 1];
    __shared__ double Ts[BW * BW], Ss[BW * BW];
    __shared__ double red[16][BW * BW], Mm[BW * BW], MT[BW * BW];
    const int i0 = blockIdx.x * 64, j0 = FIRST ? 0 : (blockIdx.y + 1) * 64;
    // What the previous kernels wrote comes from memory, not from this XCD's L2: a load costs ~2 us and the launch
    // is a chain of them unless they are all issued before anything waits -- first the partial sums of M (the
    // longest dependent path), then the rows of V and Y (or W), then the tile itself.
    double4 msum = {0.0, 0.0, 0.0, 0.0};
    if (FIRST) {   // 16 groups of 16 threads, 32-byte loads
        const int e4 = (threadIdx.x & 15) * 4, grp = threadIdx.x >> 4;
#pragma unroll 4
        for (int p = grp; p < nparts; p += 16) {
            const double4 m4 = *(const double4 *)(Mpart + (int64_t)p * (BW * BW) + e4);
            msum.x += m4.x; msum.y += m4.y; msum.z += m4.z; msum.w += m4.w;
        }
    }
    const int set = (threadIdx.x >> 6) & 1, rr = threadIdx.x & 63;   // threads 0..127: one per row of the I / J set
    const int row = (set ? j0 : i0) + rr;
    const bool ok = row < t;
    const unsigned rc = ok ? (unsigned)row : 0u;
    double v[BW], y[BW];
    if (threadIdx.x < 128) {
#pragma unroll
        for (int b = 0; b < BW; ++b) v[b] = ok ? Vd[b * vs + rc] : 0.0;
        if (FIRST) {
#pragma unroll
            for (int b = 0; b < BW; ++b) y[b] = ok ? Ypart[b * vs + rc] : 0.0;
            for (int sp = 1; sp < nsplit; ++sp) {
#pragma unroll
                for (int b = 0; b < BW; ++b) y[b] += ok ? Ypart[(int64_t)sp * BW * vs + b * vs + rc] : 0.0;
            }
        } else {
#pragma unroll
            for (int b = 0; b < BW; ++b) y[b] = ok ? Wd[b * vs + rc] : 0.0;     // W itself
        }
    }
    const int li = threadIdx.x & 63, i = i0 + li;
    double *a = A + (int64_t)r0 * ld + r0 + min(i, t - 1);
    const int jb = (threadIdx.x >> 6) * 16;
    double old[16];   // columns and rows past the end are read at a clamped index and not written
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) old[jj] = a[(int64_t)min(j0 + jb + jj, t - 1) * ld];
    if (FIRST) {
        const int e4 = (threadIdx.x & 15) * 4, grp = threadIdx.x >> 4, e = threadIdx.x & 63;
        red[grp][e4] = msum.x; red[grp][e4 + 1] = msum.y; red[grp][e4 + 2] = msum.z; red[grp][e4 + 3] = msum.w;
        if (threadIdx.x < BW * BW) Ts[threadIdx.x] = Tm[threadIdx.x];
        __syncthreads();
        if (threadIdx.x < BW * BW) {
            double m = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) m += red[q][e];
            Mm[e] = m;
        }
        __syncthreads();
        if (threadIdx.x < BW * BW) {  // MT = M T  (T upper: T[b + BW*c], b <= c)
            const int a2 = e % BW, c = e / BW;
            double m = 0.0;
            for (int b2 = 0; b2 <= c; ++b2) m += Mm[a2 + BW * b2] * Ts[b2 + BW * c];
            MT[a2 + BW * c] = m;
        }
        __syncthreads();
        if (threadIdx.x < BW * BW) {  // S = T' MT, symmetrised
            const int a2 = e % BW, c = e / BW;
            double s1 = 0.0, s2 = 0.0;
            for (int d = 0; d <= a2; ++d) s1 += Ts[d + BW * a2] * MT[d + BW * c];
            for (int d = 0; d <= c; ++d) s2 += Ts[d + BW * c] * MT[d + BW * a2];
            Ss[a2 + BW * c] = 0.5 * (s1 + s2);
        }
        __syncthreads();
    }
    if (threadIdx.x < 128) {
        if (FIRST) {
#pragma unroll
            for (int a2 = 0; a2 < BW; ++a2) {
                double x = 0.0, vsum = 0.0;
#pragma unroll
                for (int b = 0; b <= a2; ++b) x = fma(y[b], Ts[b + BW * a2], x);
#pragma unroll
                for (int c = 0; c < BW; ++c) vsum = fma(v[c], Ss[c + BW * a2], vsum);
                const double wv = x - 0.5 * vsum;
                Vs[set][rr][a2] = v[a2];
                Ws[set][rr][a2] = wv;
                if (set == 0 && ok) Wd[a2 * vs + rc] = wv;
            }
        } else {
#pragma unroll
            for (int a2 = 0; a2 < BW; ++a2) { Vs[set][rr][a2] = v[a2]; Ws[set][rr][a2] = y[a2]; }
        }
    }
    __syncthreads();
    if (i >= t) return;
    double vi[BW], wi[BW];
#pragma unroll
    for (int l = 0; l < BW; ++l) { vi[l] = Vs[0][li][l]; wi[l] = Ws[0][li][l]; }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        const int j = j0 + jb + jj;
        double sum = 0.0;
#pragma unroll
        for (int l = 0; l < BW; ++l) sum += vi[l] * Ws[1][jb + jj][l] + wi[l] * Vs[1][jb + jj][l];
        if (j < t) a[(int64_t)j * ld] = old[jj] - sum;
    }
}

// =============================================================================================
// DELAYED trailing update (large trailing matrices; LAPACK dsytrd's idea carried to the band reduction).  The eager
// scheme above rewrites the whole trailing matrix after every panel of 8 columns: 24 bytes of HBM traffic per matrix
// element and panel (symmetric product 8, rank-16 update 16), which is what a fit of 10 000+ unknowns waits for.
// Here the updates of DG = 8 consecutive panels are ACCUMULATED -- Z = [V_0 .. V_7 | W_0 .. W_7], 128 columns -- and
// applied once per group as one rank-128 product on v_mfma_f64_16x16x4f64 (band_rankk_kernel), while inside the group
// the matrix stays stale and what the next panel needs is corrected on the fly:
//   panel columns   A[:, next 8] -= sum_{q <= j} V_q W_q[next]' + W_q V_q[next]'          (band_wfix_kernel)
//   Y = A_true V    = A_stale V - sum_{q < j} V_q (W_q'V) + W_q (V_q'V)                    (band_gram_kernel + band_wfix_kernel)
//   M = V'Y         = M_stale - sum_{q < j} G1_q'G2_q + G2_q'G1_q,   G1_q = V_q'V, G2_q = W_q'V
// Traffic per element and panel: 8 (symmetric product) + 16/8 (group update) = 10 bytes, and the group update is a
// K = 128 contraction -- MFMA-shaped -- instead of eight memory-bound rank-16 passes.  Rows are indexed from the
// group's first trailing row; slot j of Z holds panel j's V (columns 8 j ..) and W (columns 64 + 8 j ..), valid from
// row 8 j on (nothing ever reads a slot above its first row).
// =============================================================================================
constexpr int DG = 8;                       // panels per group
constexpr int DG_K = 2 * DG * BW;           // columns of Z
constexpr int GRAM_RPB = 4096;              // rows per block of the Gram kernel (256 threads x 16)
constexpr int GRAM_MAXBLK = 16;             // up to 65 536 rows

// G[y][a][b] partial over a row range, y = 0 .. 2 j - 1: (y < j ? V_y : W_{y-j})' V_p.  Grid (row blocks, 2 j).
__global__ __launch_bounds__(256) void band_gram_kernel(const double *__restrict__ Z, int64_t vs, int goff, int t, int j,
                                                        double *__restrict__ Gpart /* [rowblk][2 j][64] */) {
    __shared__ double red[4][BW * BW];
    const int y = blockIdx.y, q = y < j ? y : y - j;
    const double *U = Z + (int64_t)((y < j ? 0 : DG * BW) + q * BW) * vs + goff;     // V_q or W_q, local row 0 of this panel
    const double *V = Z + (int64_t)(j * BW) * vs + goff;                              // V_p
    double acc[BW * BW];   // acc[a * BW + b]
#pragma unroll
    for (int e = 0; e < BW * BW; ++e) acc[e] = 0.0;
    for (int r = 0; r < GRAM_RPB / 256; ++r) {
        const int i = blockIdx.x * GRAM_RPB + r * 256 + threadIdx.x;
        const bool ok = i < t;
        const unsigned ii = ok ? (unsigned)i : 0u;
        double u[BW], v[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) { u[a] = ok ? U[(int64_t)a * vs + ii] : 0.0; v[a] = V[(int64_t)a * vs + ii]; }
#pragma unroll
        for (int a = 0; a < BW; ++a)
#pragma unroll
            for (int b = 0; b < BW; ++b) acc[a * BW + b] = fma(u[a], v[b], acc[a * BW + b]);
    }
    double w[16];
    wave_sum64(acc, w);      // row r of the wave holds value 4 i + rho(r) in w[i]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = lane >> 4;
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) red[wave][wave_sum64_slot(row, i)] = w[i];
    }
    __syncthreads();
    if (threadIdx.x < BW * BW)
        Gpart[((int64_t)blockIdx.x * gridDim.y + y) * (BW * BW) + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// W_p for 64 rows per block (stored into slot j of Z) and the fix-up of the next panel's 8 columns; see above.
__global__ __launch_bounds__(256) void band_wfix_kernel(double *__restrict__ A, int64_t ld, int r0, int t,
                                                        double *__restrict__ Z, int64_t vs, int goff, int j,
                                                        const double *__restrict__ Ypart, int nsplit,
                                                        const double *__restrict__ Tm, const double *__restrict__ Mpart, int nparts,
                                                        const double *__restrict__ Gpart, int ngblk) {
    __shared__ double Ts[BW * BW], Ss[BW * BW], Mm[BW * BW], MT[BW * BW], red[16][BW * BW];
    __shared__ double G1[DG * BW * BW], G2[DG * BW * BW];          // [q][a][b]
    __shared__ double Yh[72][BW + 1], Wh[72][BW + 1], Vh[72][BW + 1];   // rows 0..63: the block's rows; 64..71: head rows 0..7
    __shared__ double Vhead[DG][BW][BW + 1], Whead[DG][BW][BW + 1];     // V_q / W_q at the head rows, q < j: [q][n][a]
    const int tid = threadIdx.x, i0 = blockIdx.x * 64;
    // ---- totals: M (as band_update_kernel<true>) and the Gram blocks
    double4 msum = {0.0, 0.0, 0.0, 0.0};
    {
        const int e4 = (tid & 15) * 4, grp = tid >> 4;
#pragma unroll 4
        for (int p = grp; p < nparts; p += 16) {
            const double4 m4 = *(const double4 *)(Mpart + (int64_t)p * (BW * BW) + e4);
            msum.x += m4.x; msum.y += m4.y; msum.z += m4.z; msum.w += m4.w;
        }
        red[grp][e4] = msum.x; red[grp][e4 + 1] = msum.y; red[grp][e4 + 2] = msum.z; red[grp][e4 + 3] = msum.w;
    }
    for (int e = tid; e < 2 * j * BW * BW; e += 256) {
        double g = 0.0;
        for (int b = 0; b < ngblk; ++b) g += Gpart[(int64_t)b * (2 * j * BW * BW) + e];
        if (e < j * BW * BW) G1[e] = g; else G2[e - j * BW * BW] = g;
    }
    if (tid < BW * BW) Ts[tid] = Tm[tid];
    __syncthreads();
    if (tid < BW * BW) {
        double m = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) m += red[q][tid];
        // M[b][b'] -= sum_q sum_a G1[q][a][b] G2[q][a][b'] + G2[q][a][b] G1[q][a][b']     (M stored as Mm[b + BW b'])
        const int b = tid % BW, b2 = tid / BW;
        for (int qa = 0; qa < j * BW; ++qa) m -= G1[qa * BW + b] * G2[qa * BW + b2] + G2[qa * BW + b] * G1[qa * BW + b2];
        Mm[tid] = m;
    }
    __syncthreads();
    if (tid < BW * BW) {  // MT = M T
        const int a2 = tid % BW, c = tid / BW;
        double m = 0.0;
        for (int b2 = 0; b2 <= c; ++b2) m += Mm[a2 + BW * b2] * Ts[b2 + BW * c];
        MT[a2 + BW * c] = m;
    }
    __syncthreads();
    if (tid < BW * BW) {  // S = T' MT, symmetrised
        const int a2 = tid % BW, c = tid / BW;
        double s1 = 0.0, s2 = 0.0;
        for (int d = 0; d <= a2; ++d) s1 += Ts[d + BW * a2] * MT[d + BW * c];
        for (int d = 0; d <= c; ++d) s2 += Ts[d + BW * c] * MT[d + BW * a2];
        Ss[a2 + BW * c] = 0.5 * (s1 + s2);
    }
    // ---- head rows of the earlier panels' V and W
    for (int e = tid; e < j * BW * BW; e += 256) {
        const int q = e / (BW * BW), n = (e / BW) % BW, a = e % BW;
        Vhead[q][n][a] = Z[(int64_t)(q * BW + a) * vs + goff + n];
        Whead[q][n][a] = Z[(int64_t)(DG * BW + q * BW + a) * vs + goff + n];
    }
    // ---- corrected Y for the block's 64 rows and the 8 head rows: thread (slot, bq) owns b = 2 bq, 2 bq + 1
    const double *Vp = Z + (int64_t)(j * BW) * vs + goff;
    double *Wp = Z + (int64_t)(DG * BW + j * BW) * vs + goff;
    for (int pass = 0; pass < 2; ++pass) {
        const int slot = pass == 0 ? (tid & 63) : 64 + (tid & 7);
        const int bq = pass == 0 ? (tid >> 6) : ((tid >> 3) & 3);
        const bool active = pass == 0 || tid < 32;
        const int i = pass == 0 ? i0 + (tid & 63) : (tid & 7);
        if (active) {
            const bool ok = i < t;
            const unsigned ii = ok ? (unsigned)i : 0u;
            double y0 = 0.0, y1 = 0.0;
            for (int sp = 0; sp < nsplit; ++sp) {
                y0 += Ypart[(int64_t)sp * BW * vs + (int64_t)(2 * bq) * vs + ii];
                y1 += Ypart[(int64_t)sp * BW * vs + (int64_t)(2 * bq + 1) * vs + ii];
            }
            for (int qa = 0; qa < j * BW; ++qa) {
                const double vq = Z[(int64_t)qa * vs + goff + ii], wq = Z[(int64_t)(DG * BW + qa) * vs + goff + ii];
                y0 -= vq * G2[qa * BW + 2 * bq] + wq * G1[qa * BW + 2 * bq];
                y1 -= vq * G2[qa * BW + 2 * bq + 1] + wq * G1[qa * BW + 2 * bq + 1];
            }
            Yh[slot][2 * bq] = ok ? y0 : 0.0; Yh[slot][2 * bq + 1] = ok ? y1 : 0.0;
            Vh[slot][2 * bq] = ok ? Vp[(int64_t)(2 * bq) * vs + ii] : 0.0;
            Vh[slot][2 * bq + 1] = ok ? Vp[(int64_t)(2 * bq + 1) * vs + ii] : 0.0;
        }
    }
    __syncthreads();
    // ---- W = Y T - 1/2 V S
    for (int pass = 0; pass < 2; ++pass) {
        const int slot = pass == 0 ? (tid & 63) : 64 + (tid & 7);
        const int bq = pass == 0 ? (tid >> 6) : ((tid >> 3) & 3);
        const bool active = pass == 0 || tid < 32;
        const int i = pass == 0 ? i0 + (tid & 63) : (tid & 7);
        if (active) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int a2 = 2 * bq + h;
                double x = 0.0, vsum = 0.0;
                for (int b = 0; b <= a2; ++b) x = fma(Yh[slot][b], Ts[b + BW * a2], x);
                for (int c = 0; c < BW; ++c) vsum = fma(Vh[slot][c], Ss[c + BW * a2], vsum);
                const double wv = x - 0.5 * vsum;
                Wh[slot][a2] = wv;
                if (pass == 0 && i < t) Wp[(int64_t)a2 * vs + i] = wv;
            }
        }
    }
    __syncthreads();
    // ---- fix-up of the next panel's columns n = 0 .. 7 (local) for the block's rows: thread (row, bq) owns n = 2 bq, 2 bq + 1
    {
        const int rr = tid & 63, bq = tid >> 6, i = i0 + rr;
        if (i < t) {
            double s0 = 0.0, s1 = 0.0;
            const int n0 = 2 * bq, n1 = 2 * bq + 1;
            for (int qa = 0; qa < j * BW; ++qa) {
                const int q = qa / BW, a = qa % BW;
                const double vq = Z[(int64_t)qa * vs + goff + i], wq = Z[(int64_t)(DG * BW + qa) * vs + goff + i];
                s0 += vq * Whead[q][n0][a] + wq * Vhead[q][n0][a];
                s1 += vq * Whead[q][n1][a] + wq * Vhead[q][n1][a];
            }
#pragma unroll
            for (int a = 0; a < BW; ++a) {
                s0 += Vh[rr][a] * Wh[64 + n0][a] + Wh[rr][a] * Vh[64 + n0][a];
                s1 += Vh[rr][a] * Wh[64 + n1][a] + Wh[rr][a] * Vh[64 + n1][a];
            }
            double *a0 = A + (int64_t)(r0 + n0) * ld + r0 + i;
            if (n0 < t) a0[0] -= s0;
            if (n1 < t) a0[ld] -= s1;
        }
    }
}

// A22 -= P Q' with P = [V | W] = Z, Q = [W | V] (K = 128) on 128 x 128 tiles, ALL tiles of the t x t block (the
// symmetric product reads both triangles); rows of Z and A22 from `zoff` / r0.  Same MFMA tile loop as the
// Cholesky's trailing update (tps_chol.hip): 4 waves x 64 x 64, K streamed through two LDS buffers in chunks of
// 16, the C tile preloaded into the accumulators.  col0_only: the first block column only (look-ahead).
typedef double d4r __attribute__((ext_vector_type(4)));
constexpr int RK_T = 128, RK_KC = 16, RK_S = RK_T + 16;
__global__ __launch_bounds__(256, 2) void band_rankk_kernel(double *__restrict__ A, int64_t ld, int r0, int t,
                                                            const double *__restrict__ Z, int64_t vs, int zoff, int nt, int col0_only) {
    __shared__ __attribute__((aligned(16))) double sI[2][RK_KC * RK_S];
    __shared__ __attribute__((aligned(16))) double sJ[2][RK_KC * RK_S];
    int bi, bj;
    if (col0_only) { bi = blockIdx.x; bj = 0; }
    else { bi = blockIdx.x % nt; bj = 1 + blockIdx.x / nt; }
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int wi = (wave & 1) * 64, wj = (wave >> 1) * 64;
    double *C = A + (int64_t)r0 * ld + r0;
    d4r acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = bj * RK_T + wj + a * 16 + l4 + 4 * r;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = bi * RK_T + wi + b * 16 + l15;
                acc[a][b][r] = (i < t && l < t) ? C[(int64_t)l * ld + i] : 0.0;
            }
        }
    // staging: thread -> column k = wave + 4 q of the chunk, row gr = lane (and lane + 64): scalar 8-byte loads (the rows
    // of Z start at an arbitrary offset, no 16-byte alignment), rows past the end read as zero
    const int gk = tid >> 6, gr = tid & 63;
    const int rI0 = bi * RK_T + gr, rI1 = rI0 + 64, rJ0 = bj * RK_T + gr, rJ1 = rJ0 + 64;
    double gI[4][2], gJ[4][2];
    auto zcol = [&](int kappa) { return Z + (int64_t)kappa * vs + zoff; };
#define RK_GLOAD(K0)                                                                                   \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                    \
        const int kp = (K0) + gk + 4 * q;                                                              \
        const double *cp = zcol(kp), *cq = zcol((kp + DG * BW) & (DG_K - 1));                          \
        gI[q][0] = rI0 < t ? cp[rI0] : 0.0; gI[q][1] = rI1 < t ? cp[rI1] : 0.0;                        \
        gJ[q][0] = rJ0 < t ? cq[rJ0] : 0.0; gJ[q][1] = rJ1 < t ? cq[rJ1] : 0.0;                        \
    }
#define RK_SSTORE(BUF)                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                    \
        sI[BUF][(gk + 4 * q) * RK_S + gr] = gI[q][0]; sI[BUF][(gk + 4 * q) * RK_S + gr + 64] = gI[q][1]; \
        sJ[BUF][(gk + 4 * q) * RK_S + gr] = gJ[q][0]; sJ[BUF][(gk + 4 * q) * RK_S + gr + 64] = gJ[q][1]; \
    }
    RK_GLOAD(0)
    RK_SSTORE(0)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): no prologue load (the C tile) pending into the loop, see chol_syrk_kernel
    __syncthreads();
    for (int c = 0; c < DG_K / RK_KC; ++c) {
        const int buf = c & 1;
        if (c + 1 < DG_K / RK_KC) { RK_GLOAD((c + 1) * RK_KC) }
#pragma unroll
        for (int kk = 0; kk < RK_KC; kk += 4) {
            double fi[4], fj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                fj[a] = -sJ[buf][(kk + l4) * RK_S + wj + a * 16 + l15];
                fi[a] = sI[buf][(kk + l4) * RK_S + wi + a * 16 + l15];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fj[a], fi[b], acc[a][b], 0, 0, 0);
        }
        if (c + 1 < DG_K / RK_KC) {
            RK_SSTORE(buf ^ 1)
            __syncthreads();
        }
    }
#undef RK_GLOAD
#undef RK_SSTORE
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = bj * RK_T + wj + a * 16 + l4 + 4 * r;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = bi * RK_T + wi + b * 16 + l15;
                if (i < t && l < t) C[(int64_t)l * ld + i] = acc[a][b][r];
            }
        }
}

// lower band of B -> ab[d + (BW+1) j]
__global__ void band_extract_kernel(const double *__restrict__ A, int64_t ld, int off0, int m,
                                    double *__restrict__ ab) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * (BW + 1)) return;
    const int j = e / (BW + 1), d = e - j * (BW + 1);
    ab[e] = (j + d < m) ? A[(int64_t)(off0 + j) * ld + off0 + j + d] : 0.0;
}

// r <- Q_0 Q_1 ... Q_{P-1} r,  Q_p = I - V_p T_p V_p'  (single block; reflectors read in place)
// r <- Q r, Q = H_0 H_1 ... (block reflectors, applied last to first).  One block (each step needs a sum over all
// rows), so it is a chain of npanels latencies: the vector stays in registers (thread = fixed rows), each panel's
// reflectors are read once and used for both the products and the update, and the reduction is the
// single-barrier one of the panel kernel.  (Touching the next panel's lines into L2 ahead of time measured slower.)
constexpr int BT_THREADS = 1024, BT_RPT = 5;
__global__ __launch_bounds__(BT_THREADS) void band_backtransform_reg_kernel(const double *__restrict__ A,
                                                                            int64_t ld, int off0, int m,
                                                                            int npanels,
                                                                            const double *__restrict__ Tall,
                                                                            double *__restrict__ r) {
    __shared__ double part[2][BT_THREADS / 64][BW];
    double rr[BT_RPT];
#pragma unroll
    for (int k = 0; k < BT_RPT; ++k) {
        const int q = threadIdx.x + BT_THREADS * k;
        rr[k] = q < m ? r[q] : 0.0;
    }
    int ph = 0;
    for (int p = npanels - 1; p >= 0; --p) {
        const int base = p * BW + BW;
        const double *P = A + (int64_t)(off0 + p * BW) * ld + off0 + base;
        const double *T = Tall + (int64_t)p * BW * BW;
        double v[BT_RPT][BW], s[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) s[a] = 0.0;
#pragma unroll
        for (int k = 0; k < BT_RPT; ++k) {
            const int q = threadIdx.x + BT_THREADS * k, i = q - base;
            const bool ok = i >= 0 && q < m;
            const unsigned ii = ok ? (unsigned)i : 0u;
#pragma unroll
            for (int a = 0; a < BW; ++a) v[k][a] = P[(int64_t)a * ld + ii];
        }
#pragma unroll
        for (int k = 0; k < BT_RPT; ++k) {
            const int q = threadIdx.x + BT_THREADS * k, i = q - base;
            const bool ok = i >= 0 && q < m;
#pragma unroll
            for (int a = 0; a < BW; ++a) {
                v[k][a] = (!ok || i < a) ? 0.0 : (i == a ? 1.0 : v[k][a]);
                s[a] = fma(v[k][a], rr[k], s[a]);
            }
        }
        wave_publish<BW>(s, part[ph]);
        __syncthreads();
        const double sb = block_total<BW, BT_THREADS / 64>(part[ph]);
        ph ^= 1;
        double sv[BW];
#pragma unroll
        for (int b = 0; b < BW; ++b) sv[b] = lane_value(sb, b);
        double z[BW];   // z = T s, T upper triangular
#pragma unroll
        for (int a = 0; a < BW; ++a) {
            z[a] = 0.0;
#pragma unroll
            for (int b = a; b < BW; ++b) z[a] += T[a + BW * b] * sv[b];
        }
#pragma unroll
        for (int k = 0; k < BT_RPT; ++k) {
#pragma unroll
            for (int a = 0; a < BW; ++a) rr[k] -= v[k][a] * z[a];
        }
    }
#pragma unroll
    for (int k = 0; k < BT_RPT; ++k) {
        const int q = threadIdx.x + BT_THREADS * k;
        if (q < m) r[q] = rr[k];
    }
}

// Tall form (m beyond the register-resident kernel): one MANY-block launch per panel.  Launch p applies panel p's block
// reflector, r -= V_p (T_p s_p) with s_p = V_p'r summed from the previous launch's partials, and in the same pass over
// its rows forms the partials of s_{p-1} = V_{p-1}'r for the next launch (panel p-1's rows contain panel p's).
constexpr int BTM_RPB = 256, BTM_MAXBLK = 256;
__global__ __launch_bounds__(256) void band_backtransform_step_kernel(const double *__restrict__ A, int64_t ld, int off0, int m,
                                                                      int p /* panel to apply, npanels = none yet */, int npanels,
                                                                      const double *__restrict__ Tall, double *__restrict__ r,
                                                                      double *__restrict__ part /* [2][BTM_MAXBLK][BW] */) {
    __shared__ double lds[4][BW];
    const int i = blockIdx.x * BTM_RPB + threadIdx.x;       // row of B (0 .. m-1)
    double ri = i < m ? r[i] : 0.0;
    if (p < npanels) {      // apply panel p: rows q >= base_p = 8 p + 8
        const int base = p * BW + BW;
        double sv[BW];      // thread b takes row block b's partials (blocks above the panel wrote zeros), then a block sum
#pragma unroll
        for (int a = 0; a < BW; ++a) sv[a] = threadIdx.x < gridDim.x ? part[(size_t)((p & 1) * BTM_MAXBLK + threadIdx.x) * BW + a] : 0.0;
        block_sum8(sv, lds);
        __syncthreads();
        const double *T = Tall + (int64_t)p * BW * BW;
        const int il = i - base;
        if (il >= 0 && i < m) {
            const double *P = A + (int64_t)(off0 + p * BW) * ld + off0 + base;
#pragma unroll
            for (int a = 0; a < BW; ++a) {
                double z = 0.0;
#pragma unroll
                for (int b = a; b < BW; ++b) z += T[a + BW * b] * sv[b];
                const double v = il < a ? 0.0 : (il == a ? 1.0 : P[(int64_t)a * ld + il]);
                ri -= v * z;
            }
            r[i] = ri;
        }
    }
    if (p > 0) {            // partials of s_{p-1} = V_{p-1}' r (updated r)
        const int q = p - 1, base = q * BW + BW, il = i - base;
        double acc[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) acc[a] = 0.0;
        if (il >= 0 && i < m) {
            const double *P = A + (int64_t)(off0 + q * BW) * ld + off0 + base;
#pragma unroll
            for (int a = 0; a < BW; ++a) {
                const double v = il < a ? 0.0 : (il == a ? 1.0 : P[(int64_t)a * ld + il]);
                acc[a] = v * ri;
            }
        }
        block_sum8(acc, lds);
        if (threadIdx.x < BW) part[(size_t)((q & 1) * BTM_MAXBLK + blockIdx.x) * BW + threadIdx.x] = acc[threadIdx.x];
    }
}

__global__ __launch_bounds__(1024) void band_backtransform_kernel(const double *__restrict__ A, int64_t ld,
                                                                  int off0, int m, int npanels,
                                                                  const double *__restrict__ Tall,
                                                                  double *__restrict__ r) {
    __shared__ double lds[17 * BW];
    __shared__ double zs[BW];
    for (int p = npanels - 1; p >= 0; --p) {
        const int c = p * BW, t = m - c - BW;
        const double *P = A + (int64_t)(off0 + c) * ld + off0 + c + BW;
        const double *T = Tall + (int64_t)p * BW * BW;
        double *rs = r + c + BW;
        double s[BW];
#pragma unroll
        for (int a = 0; a < BW; ++a) s[a] = 0.0;
        for (int i = threadIdx.x; i < t; i += blockDim.x) {
            const double ri = rs[i];
#pragma unroll
            for (int a = 0; a < BW; ++a) {
                const double v = i < a ? 0.0 : (i == a ? 1.0 : P[(int64_t)a * ld + i]);
                s[a] = fma(v, ri, s[a]);
            }
        }
        block_sum_vec<BW>(s, lds);
        if (threadIdx.x < BW) {  // z = T s
            const int a = threadIdx.x;
            double sum = 0.0;
            for (int b = a; b < BW; ++b) sum += T[a + BW * b] * s[b];
            zs[a] = sum;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < t; i += blockDim.x) {
            double ri = rs[i];
#pragma unroll
            for (int a = 0; a < BW; ++a) {
                const double v = i < a ? 0.0 : (i == a ? 1.0 : P[(int64_t)a * ld + i]);
                ri -= v * zs[a];
            }
            rs[i] = ri;
        }
        __syncthreads();
    }
}

// ================================================================================================ host side ==
constexpr int T_DELAY = 4000;      // trailing matrices taller than this take the delayed update scheme

int band8_npanels(int m) {
    int np = 0;
    for (int c = 0; m - c - BW >= 2; c += BW) ++np;
    return np;
}
bool band8_cacheable(int m) { return band8_npanels(m) > 0 && m - BW <= PANEL_THREADS * PANEL_RPT && m <= BT_THREADS * BT_RPT; }

static size_t band8_layout(Band8Ws *w, char *base, int m, int64_t n, bool gcv) {
    size_t off = 0;
    auto take = [&](size_t bytes) -> void * {
        off = (off + 255) & ~(size_t)255;
        void *p = base ? base + off : nullptr;
        off += bytes;
        return p;
    };
    auto dbl = [&](size_t doubles) { return (double *)take(doubles * sizeof(double)); };
    const size_t vs = (size_t)n, np = (size_t)std::max(band8_npanels(m), 1);
    const bool big = gcv && m - BW > T_DELAY;   // the delayed scheme's group buffers (large fits only)
    Band8Ws d;
    d.Vd = dbl(BW * vs);
    d.Vd2 = dbl(BW * vs);
    d.Wd = dbl(BW * vs);
    d.Wd2 = dbl(BW * vs);
    d.Yp = dbl((size_t)SYMM_MAX_SPLITS * BW * vs);
    d.Mp = dbl((size_t)((m + SYMM_COLS - 1) / SYMM_COLS + 1) * SYMM_MAX_SPLITS * BW * BW);
    d.Tall = dbl(np * BW * BW);
    d.aux = dbl(np * PANEL_AUX);
    d.Zb = dbl(big ? (size_t)DG_K * vs + 16 : 1);
    d.Zb2 = dbl(big ? (size_t)DG_K * vs + 16 : 1);
    d.Gp = dbl((size_t)GRAM_MAXBLK * 2 * DG * BW * BW);
    d.ab = dbl((size_t)m * (BW + 1));
    d.tall_sc = (TallScratch *)take(sizeof(TallScratch));
    if (w) *w = d;
    return off;
}
size_t band8_workspace_bytes(int m, int64_t n, bool gcv) { return band8_layout(nullptr, nullptr, m, n, gcv); }
void band8_carve(Band8Ws &w, char *base, int m, int64_t n, bool gcv) { (void)band8_layout(&w, base, m, n, gcv); }

int band8_reduce(FitLane &L, hipStream_t s, hipStream_t s2, double *A, int64_t ld, int m, int64_t vs, double *g_dev, Band8Ws &ws,
                 bool keep_aux, hipEvent_t *wake) {
    // Two streams: the panel factorisation of step p+1 needs only the first column block of the trailing
    // matrix as updated by step p.  That block is updated first, on the main stream, which goes straight on
    // to the (single-block, latency-bound) panel kernel of step p+1, while the rest of step p's update runs
    // on stream2 behind an event.  The panel block needs a whole CU's registers: it must reach the
    // dispatcher before the flood of update blocks, which the event's latency ensures.  Per step the
    // critical path is panel + symm + s + one column block instead of panel + symm + s + the whole update.
    const int npanels = band8_npanels(m);
    std::vector<hipEvent_t> &pool = L.pool;
    while ((int)pool.size() < 2 * npanels + 1) {
        hipEvent_t e;
        MHS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pool.push_back(e);
    }
    *wake = npanels > 0 ? pool[2 * npanels] : nullptr;
    // Panels 0 .. p_sw-1 run the DELAYED scheme (groups of DG panels, one MFMA rank-128 update per group) while the
    // trailing matrix is large -- there the eager scheme waits for HBM -- the rest the eager one (latency-optimal).
    int p_sw = 0;
    while (p_sw + DG <= npanels && m - p_sw * BW - BW > T_DELAY && m - p_sw * BW - BW <= GRAM_RPB * GRAM_MAXBLK) p_sw += DG;
    hipEvent_t pending_rest = nullptr;      // the update launch the next symmetric product has to wait for
    for (int p = 0; p < npanels; ++p) {
        const int c = p * BW, t = m - c - BW, c0 = 3 + c, r0 = 3 + c + BW;
        double *Tp = ws.Tall + (size_t)p * BW * BW;
        const bool delayed = p < p_sw;
        const int jg = p % DG;                                          // position in its group (delayed panels)
        double *Zg = ((p / DG) & 1) ? ws.Zb2 : ws.Zb;                   // the group's [V | W] columns, double-buffered
        double *Vp = delayed ? Zg + (int64_t)(jg * BW) * vs + jg * BW : ((p & 1) ? ws.Vd2 : ws.Vd);
        double *Wp = (p & 1) ? ws.Wd2 : ws.Wd;
        hipEvent_t ev_block = pool[2 * p], ev_rest = pool[2 * p + 1];
        if (t <= PANEL_THREADS * PANEL_RPT) {
            // 640 rows per wave up to one wave per SIMD; beyond that all 8 (5 .. 7 waves load the SIMDs unevenly:
            // t = 4197 took 44 us with 7 against 38.5 with 8)
            const int nw = t <= 256 * PANEL_RPT ? (t + 64 * PANEL_RPT - 1) / (64 * PANEL_RPT) : PANEL_THREADS / 64;
#define MHS_PANEL(NW) case NW: hipLaunchKernelGGL(band_panel_reg_kernel<NW>, dim3(1), dim3(64 * NW), 0, s, A, ld, c0, r0, t, Vp, vs, Tp, g_dev + c + BW, keep_aux ? ws.aux + (size_t)p * PANEL_AUX : nullptr); break;
            switch (nw) { MHS_PANEL(1) MHS_PANEL(2) MHS_PANEL(3) MHS_PANEL(4) default: MHS_PANEL(8) }
#undef MHS_PANEL
        }
        else if (t > TALL_RPB * TALL_MAXBLK)
            hipLaunchKernelGGL(band_panel_kernel, dim3(1), dim3(1024), 0, s, A, ld, c0, r0, t, Vp, vs, Tp, g_dev + c + BW);
        else {      // tall panel: one many-block launch per Householder step
            const unsigned nblk = (unsigned)((t + TALL_RPB - 1) / TALL_RPB);
            hipLaunchKernelGGL(tall_dots0_kernel, dim3(nblk), dim3(256), 0, s, A, ld, c0, r0, t, ws.tall_sc);
            for (int J = 0; J < BW; ++J)
                hipLaunchKernelGGL(tall_step_kernel, dim3(nblk), dim3(256), 0, s, A, ld, c0, r0, t, J, Vp, vs, ws.tall_sc);
            hipLaunchKernelGGL(tall_gram_kernel, dim3(nblk), dim3(256), 0, s, Vp, vs, t, g_dev + c + BW, ws.tall_sc);
            hipLaunchKernelGGL(tall_finish_kernel, dim3(nblk), dim3(256), 0, s, Vp, vs, t, g_dev + c + BW, Tp, ws.tall_sc);
        }
        if (p == std::max(0, npanels - 12)) MHS_HIP(hipEventRecord(*wake, s));   // ~1 ms before the end
        const int ncg = (t + SYMM_COLS - 1) / SYMM_COLS, nsplit = symm_splits(t);
        const unsigned nb = (unsigned)((t + 63) / 64);
        if (delayed) {
            int ngblk = 0;
            if (jg > 0) {      // G1 = V_q'V, G2 = W_q'V for the group's earlier panels (reads the panel's output only)
                ngblk = (t + GRAM_RPB - 1) / GRAM_RPB;
                hipLaunchKernelGGL(band_gram_kernel, dim3((unsigned)ngblk, (unsigned)(2 * jg)), dim3(256), 0, s, Zg, vs, jg * BW, t, jg, ws.Gp);
            }
            if (pending_rest) { MHS_HIP(hipStreamWaitEvent(s, pending_rest, 0)); pending_rest = nullptr; }
            hipLaunchKernelGGL(band_symm_kernel, dim3((unsigned)ncg, (unsigned)nsplit), dim3(256), 0, s, A, ld, r0, t, Vp, vs, ws.Yp, ws.Mp);
            hipLaunchKernelGGL(band_wfix_kernel, dim3(nb), dim3(256), 0, s, A, ld, r0, t, Zg, vs, jg * BW, jg, ws.Yp, nsplit, Tp, ws.Mp,
                               ncg * nsplit, ws.Gp, ngblk);
            if (jg == DG - 1 && t > BW) {      // group complete: A22 of the NEXT panel -= [V | W] [W | V]'
                const int t2 = t - BW, r2 = r0 + BW, nt = (t2 + RK_T - 1) / RK_T;
                hipLaunchKernelGGL(band_rankk_kernel, dim3((unsigned)nt), dim3(256), 0, s, A, ld, r2, t2, Zg, vs, DG * BW, nt, 1);
                MHS_HIP(hipEventRecord(ev_block, s));
                MHS_HIP(hipStreamWaitEvent(s2, ev_block, 0));
                if (nt > 1)
                    hipLaunchKernelGGL(band_rankk_kernel, dim3((unsigned)(nt * (nt - 1))), dim3(256), 0, s2, A, ld, r2, t2, Zg, vs, DG * BW, nt, 0);
                MHS_HIP(hipEventRecord(ev_rest, s2));
                pending_rest = ev_rest;
            }
            continue;
        }
        if (pending_rest) { MHS_HIP(hipStreamWaitEvent(s, pending_rest, 0)); pending_rest = nullptr; }     // rest of the previous update
        hipLaunchKernelGGL(band_symm_kernel, dim3((unsigned)ncg, (unsigned)nsplit), dim3(256), 0, s, A, ld, r0, t, Vp, vs, ws.Yp, ws.Mp);
        hipLaunchKernelGGL(band_update_kernel<true>, dim3(nb, 1), dim3(256), 0, s, A, ld, r0, t, Vp, ws.Yp, nsplit, vs, Tp, ws.Mp, ncg * nsplit, Wp);
        MHS_HIP(hipEventRecord(ev_block, s));
        MHS_HIP(hipStreamWaitEvent(s2, ev_block, 0));
        if (nb > 1)
            hipLaunchKernelGGL(band_update_kernel<false>, dim3(nb, nb - 1), dim3(256), 0, s2, A, ld, r0, t, Vp, ws.Yp, nsplit, vs, Tp, ws.Mp, ncg * nsplit, Wp);
        MHS_HIP(hipEventRecord(ev_rest, s2));
        pending_rest = ev_rest;
    }
    if (pending_rest) MHS_HIP(hipStreamWaitEvent(s, pending_rest, 0));
    hipLaunchKernelGGL(band_extract_kernel, dim3((unsigned)((m * (BW + 1) + 255) / 256)), dim3(256), 0, s, A, ld, 3, m, ws.ab);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

int band8_qt(hipStream_t s, const double *A, int64_t ld, int m, const double *aux, double *g_dev) {
    hipLaunchKernelGGL(band_qt_kernel, dim3(1), dim3(PANEL_THREADS), 0, s, A, ld, 3, m, band8_npanels(m), aux, g_dev);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

int band8_backtransform(hipStream_t s, const double *A, int64_t ld, int m, const double *Tall, double *r_dev, double *Gp) {
    const int npanels = band8_npanels(m);
    if (npanels > 0) {
        if (m <= BT_THREADS * BT_RPT)
            hipLaunchKernelGGL(band_backtransform_reg_kernel, dim3(1), dim3(BT_THREADS), 0, s, A, ld, 3, m, npanels, Tall, r_dev);
        else if (m <= BTM_RPB * BTM_MAXBLK) {
            const unsigned nblk = (unsigned)((m + BTM_RPB - 1) / BTM_RPB);
            for (int p = npanels; p >= 0; --p)      // launch p applies panel p (none for p = npanels) and prepares panel p - 1
                hipLaunchKernelGGL(band_backtransform_step_kernel, dim3(nblk), dim3(256), 0, s, A, ld, 3, m, p, npanels, Tall, r_dev, Gp);
        } else
            hipLaunchKernelGGL(band_backtransform_kernel, dim3(1), dim3(1024), 0, s, A, ld, 3, m, npanels, Tall, r_dev);
    }
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

}  // namespace mhs
