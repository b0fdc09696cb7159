// 8-column GCV route of the spline fit: blocked Householder reduction to a band of width 8, GCV on the band on the host
// (tps_band8.hip; BandGcv in tps_gcv_host.hip).  Takes the fits between the one-block tridiagonal route and B32_MIN_M,
// the fits beyond B32_MAX_M, every fit under MHS_FIT_LEGACY_BAND=1, and a fit whose 32-column reduction broke down.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "common.h"
#include "devmath.h"

namespace mhs {
constexpr int BW = 8;                    // band width of the reduction
constexpr int PANEL_AUX = BW + BW * BW;  // doubles a register-resident panel leaves for band8_qt: tau, then G = (v_l'v_j)

struct TallScratch;
// device work space of one fit on this route, carved from the lane's arena
struct Band8Ws {
    double *Vd, *Vd2, *Wd, *Wd2, *Yp, *Mp, *Tall, *aux, *Zb, *Zb2, *Gp, *ab;
    TallScratch *tall_sc;
};
// gcv = false: the arena slot of a fixed-lambda fit, which never runs the route (no group buffers of the delayed scheme)
size_t band8_workspace_bytes(int m, int64_t n, bool gcv);
void band8_carve(Band8Ws &w, char *base, int m, int64_t n, bool gcv);
int band8_npanels(int m);
// the reduction can be replayed for another right-hand side (band8_qt mirrors the register-resident panel kernel only,
// and the cached back-transform is the register-resident one)
bool band8_cacheable(int m);

// A: n x n projected matrix (column-major, ld; B = A[3:, 3:]), g_dev: Q2'y (m entries, rotated in place to Q'g).  Leaves the
// reflectors below the band, the T factors in ws.Tall, the band in ws.ab (device, ab[j * 9 + d]) and, with keep_aux, the
// panels' (tau, G) records in ws.aux.  Work goes to s and s2; everything is enqueued when the call returns.  *wake (NULL
// when the matrix has no panel) is recorded about a millisecond of GPU work before the end: the caller waits for it to
// wake the host's GCV workers under the last panels.
int band8_reduce(FitLane &L, hipStream_t s, hipStream_t s2, double *A, int64_t ld, int m, int64_t vs, double *g_dev, Band8Ws &ws,
                 bool keep_aux, hipEvent_t *wake);
// g <- Q'g for another right-hand side with a finished reduction (the reduction cache), bit for bit what band8_reduce did
int band8_qt(hipStream_t s, const double *A, int64_t ld, int m, const double *aux, double *g_dev);
// r <- Q r; Gp: ws.Gp
int band8_backtransform(hipStream_t s, const double *A, int64_t ld, int m, const double *Tall, double *r_dev, double *Gp);

// ---- wave / block reductions of the register-resident panel kernel, shared with the one-block tridiagonal kernels of
// tps_fit.hip (their partial buffers are rows of BW doubles)

// sum over the wave, valid in lanes 48..63: xor 1, xor 2, mirror within 8, mirror within 16, then the row totals
// are chained with row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3)
__device__ __forceinline__ double wave_sum_top(double x) {
    x += dpp_fetch<0xB1, 0xf>(x);
    x += dpp_fetch<0x4E, 0xf>(x);
    x += dpp_fetch<0x141, 0xf>(x);
    x += dpp_fetch<0x140, 0xf>(x);
    x += dpp_fetch<0x142, 0xa>(x);
    x += dpp_fetch<0x143, 0xc>(x);
    return x;
}
// gfx950 lane swaps: v_permlane32_swap exchanges the upper half-wave of one register with the lower half-wave of
// another, v_permlane16_swap the odd rows of one with the even rows of the other -- so "two swaps and an add" folds
// two values into one register holding the half-sums of the first in one half (even rows) and of the second in
// the other: a reduction of several values costs about one DPP row reduction per FOUR values.
__device__ __forceinline__ double swap_add32(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ double swap_add16(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// Wave-reduce K <= 8 values and publish them to a partial buffer buf[wave][k]; after the caller's barrier,
// block_total() adds them.  Two lane-swap stages leave row r = lane >> 4 with values 4 i + rho(r),
// rho = {0, 2, 1, 3}, i = 0, 1; a DPP reduction within the rows finishes them.
template <int K>
__device__ __forceinline__ void wave_publish(double (&v)[K], double (*buf)[BW]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if constexpr (K == 1) {
        const double tot = wave_sum_top(v[0]);
        if (lane == 63) buf[wave][0] = tot;
    } else {
        static_assert(K <= 8, "at most 8 values");
        double u[4], w[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = swap_add32(2 * i < K ? v[2 * i] : 0.0, 2 * i + 1 < K ? v[2 * i + 1] : 0.0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            w[i] = swap_add16(u[2 * i], u[2 * i + 1]);
            w[i] += dpp_fetch<0xB1, 0xf>(w[i]);
            w[i] += dpp_fetch<0x4E, 0xf>(w[i]);
            w[i] += dpp_fetch<0x141, 0xf>(w[i]);
            w[i] += dpp_fetch<0x140, 0xf>(w[i]);
        }
        if ((lane & 15) == 0) {
            const int row = lane >> 4, rho = (row & 1) << 1 | (row >> 1);
            if (rho < K) buf[wave][rho] = w[0];
            if (4 + rho < K) buf[wave][4 + rho] = w[1];
        }
    }
}
// lane k (< K; the other lanes repeat lane K-1's work) returns total k, added in wave order
template <int K, int NW>
__device__ __forceinline__ double block_total(const double (*buf)[BW]) {
    const int lane = threadIdx.x & 63, k = lane < K ? lane : K - 1;
    double s = buf[0][k];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += buf[w][k];
    return s;
}
}  // namespace mhs
