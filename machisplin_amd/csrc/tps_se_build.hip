// Q = -M^-1 of the prediction standard errors, built on gfx950 (the block formula stated above se_build in tps_se.hip is
// the specification; the host build there stays the yardstick).  Every O(n^2) and O(n^3) object lives on the device; the
// host sees vectors of length n, the 3 x 3 pieces (R^-1, S3, BR) and the scalars.
//
//   1. F = Q'(S K S)Q + lambda I in two passes over kernel entries computed on the fly with the exact log (ocml's double
//      log, phi(0) = 0): Y = (S K S) V for the three reflectors V (seb_kv_kernel), the 3 x 3 algebra of the compact WY
//      form on the host, then F = S K S - W V' - V W' + lambda I (seb_f_kernel) in the layout cholesky_solve_mfma reads
//      (off = 3, row 3 of every column 16-byte aligned, chol_padded(m) rows and columns).
//   2. cholesky_solve_mfma on F22 with rhs = wv[3:]: L in place, every panel's L_jj^-1 in the workspace, x = X wv2.
//   3. U = L^-T, upper triangular, in 128 x 128 blocks, right-looking: once block column k of U stands,
//          seb_inv_update_kernel    U[rb, i] += U[rb, k] L[i, k]'      for every rb <= k < i   (K = 128 per tile)
//          seb_inv_finish_kernel    U[rb, k+1] = -U[rb, k+1] L_{k+1,k+1}^-T  for every rb <= k (in place, accumulators)
//      with U[k, k] = L_kk^-T copied from the workspace.  Then X = U U' on 128 x 128 tiles of the lower triangle
//      (seb_xxt_kernel; the K range of tile (bi, bj) starts at panel bi, the later of the two), each value written to both
//      halves.  All three are the tile product of chol_syrk_kernel: 4 waves x 64 x 64 accumulators, K streamed through LDS
//      in double-buffered chunks of 16, v_mfma_f64_16x16x4_f64 throughout.  About 2 m^3 / 3 flop beyond the factorisation.
//      The identity padding of the factorisation makes the padded rows and columns of U and X inert: U is zeroed as a
//      whole before its blocks accumulate, so no kernel reads memory nothing has written.
//   4. One pass over X gives X [F21 | V] and diag X (seb_xb_kernel, a wave per column, fixed summation order); the host
//      finishes tr X, Y, S3, the top-right and bottom-right blocks (O(n)) and the WY vectors of Q diag(0, X) Q'; the last
//      kernel (seb_q_kernel) writes Q = -k^2 S (Z - W V' - V W') S with its borders straight into the handle's q_dev,
//      both halves from one computed value.
// Nothing here uses floating-point atomics: the same knots, weights and lambda give the same Q bit for bit.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>
#include "common.h"
#include "devmath.h"
#include "tps_host.h"
#include "tps_chol.h"
#include "tps_se.h"

namespace mhs {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int SB_T = 128;            // tile edge = the factorisation's panel width
constexpr int SB_KC = 16;            // K chunk
constexpr int SB_S = SB_T + 16;      // LDS row stride of a chunk (chol_syrk_kernel's)

// S K S entry with the host build's operations
__device__ __forceinline__ double seb_phi(double ui, double vi, double si, double uj, double vj, double sj) {
    const double dx = ui - uj, dy = vi - vj;
    const double d2 = dx * dx + dy * dy;
    return d2 > 0 ? si * sj * (PHI_K * d2 * log(d2)) : 0.0;
}

// Y = (S K S) V, V = the three reflectors (3 x n): one block per row, fixed summation order
__global__ __launch_bounds__(256) void seb_kv_kernel(const double *__restrict__ u, const double *__restrict__ v,
                                                     const double *__restrict__ sw, int n, const double *__restrict__ V,
                                                     double *__restrict__ Y) {
    __shared__ double scratch[17];
    const int i = blockIdx.x;
    const double ui = u[i], vi = v[i], si = sw[i];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double k = seb_phi(ui, vi, si, u[j], v[j], sw[j]);
        s0 = fma(k, V[j], s0);
        s1 = fma(k, V[(int64_t)n + j], s1);
        s2 = fma(k, V[2 * (int64_t)n + j], s2);
    }
    s0 = block_sum(s0, scratch);
    s1 = block_sum(s1, scratch);
    s2 = block_sum(s2, scratch);
    if (threadIdx.x == 0) { Y[i] = s0; Y[(int64_t)n + i] = s1; Y[2 * (int64_t)n + i] = s2; }
}

// F = S K S - W V' - V W' + lambda I, column-major with leading dimension ld; blockIdx.y = column
__global__ __launch_bounds__(256) void seb_f_kernel(const double *__restrict__ u, const double *__restrict__ v,
                                                    const double *__restrict__ sw, int n, const double *__restrict__ V,
                                                    const double *__restrict__ W, double lam, double *__restrict__ A, int64_t ld) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n) return;
    const double k = seb_phi(u[i], v[i], sw[i], u[j], v[j], sw[j]);
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int64_t o = (int64_t)q * n;
        t += W[o + i] * V[o + j] + V[o + i] * W[o + j];
    }
    A[i + (int64_t)j * ld] = (k - t) + (i == j ? lam : 0.0);
}

// acc[a][b][r] += sum_k I[wi + 16 b + l15][k] J[wj + 16 a + l4 + 4 r][k] over k in [0, 16 nchunk): the two operands are
// 128 rows each, element (row, k) at p[row + k * ld] (16-byte aligned rows, ld even).  The loop of chol_syrk_kernel.
struct SebLds {
    double sI[2][SB_KC * SB_S];
    double sJ[2][SB_KC * SB_S];
};
__device__ __forceinline__ void seb_tile_product(const double *__restrict__ pI, int64_t ldi, const double *__restrict__ pJ,
                                                 int64_t ldj, int nchunk, d4 (&acc)[4][4], SebLds &lds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int wi = (wave & 1) * 64, wj = (wave >> 1) * 64;
    // chunk = 16 columns k of 128 rows per operand: thread -> column k = wave + 4 q, rows 2 lane, 2 lane + 1
    const int gk = tid >> 6, gr = (tid & 63) * 2;
    const double *qI = pI + (int64_t)gk * ldi + gr, *qJ = pJ + (int64_t)gk * ldj + gr;
    double2 gI[4], gJ[4];
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            gI[q] = *(const double2 *)(qI + (int64_t)(k0 + 4 * q) * ldi);
            gJ[q] = *(const double2 *)(qJ + (int64_t)(k0 + 4 * q) * ldj);
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *(double2 *)&lds.sI[buf][(gk + 4 * q) * SB_S + gr] = gI[q];
            *(double2 *)&lds.sJ[buf][(gk + 4 * q) * SB_S + gr] = gJ[q];
        }
    };
    gload(0);
    sstore(0);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the accumulators' own loads retire before the loop (chol_syrk_kernel)
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunk) gload((c + 1) * SB_KC);
#pragma unroll
        for (int kk = 0; kk < SB_KC; kk += 4) {
            double fi[4], fj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                fj[a] = lds.sJ[buf][(kk + l4) * SB_S + wj + a * 16 + l15];
                fi[a] = lds.sI[buf][(kk + l4) * SB_S + wi + a * 16 + l15];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fj[a], fi[b], acc[a][b], 0, 0, 0);
        }
        if (c + 1 < nchunk) {
            sstore(buf ^ 1);
            __syncthreads();
        }
    }
}
// the accumulators' element (a, b, r) of this lane: row and column inside the 128 x 128 tile
__device__ __forceinline__ int seb_row(int b) { return ((threadIdx.x >> 6) & 1) * 64 + 16 * b + (threadIdx.x & 15); }
__device__ __forceinline__ int seb_col(int a, int r) { return (threadIdx.x >> 7) * 64 + 16 * a + ((threadIdx.x & 63) >> 4) + 4 * r; }

// U[k, k] = L_kk^-T for every panel: the transposed copy chol_diag_kernel leaves behind its L_kk^-1 (zeros below the diagonal)
__global__ __launch_bounds__(256) void seb_inv_diag_kernel(double *__restrict__ U, int64_t ldu, const double *__restrict__ work) {
    const int k = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;      // e = row + 128 col
    const int r = e & (SB_T - 1), c = e >> 7;
    U[(int64_t)(k * SB_T + c) * ldu + k * SB_T + r] = work[(size_t)k * 2 * SB_T * SB_T + SB_T * SB_T + e];
}

// U[rb, ci] += U[rb, k] L[ci, k]' for rb = 0 .. k and ci = k + 1 .. np - 1 (block indices); Lm = the factor (order m_pad, ld)
__global__ __launch_bounds__(256, 2) void seb_inv_update_kernel(double *__restrict__ U, int64_t ldu, const double *__restrict__ Lm,
                                                                int64_t ld, int k) {
    __shared__ __attribute__((aligned(16))) SebLds lds;
    const int rb = blockIdx.x % (k + 1), ci = k + 1 + blockIdx.x / (k + 1);
    double *C = U + (int64_t)ci * SB_T * ldu + (int64_t)rb * SB_T;
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b][r] = C[(int64_t)seb_col(a, r) * ldu + seb_row(b)];
    seb_tile_product(U + (int64_t)k * SB_T * ldu + (int64_t)rb * SB_T, ldu, Lm + (int64_t)k * SB_T * ld + (int64_t)ci * SB_T, ld,
                     SB_T / SB_KC, acc, lds);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < 4; ++b) C[(int64_t)seb_col(a, r) * ldu + seb_row(b)] = acc[a][b][r];
}

// U[rb, k] = -U[rb, k] L_kk^-T for rb = 0 .. k - 1, in place: the tile is read whole into the product before it is written
__global__ __launch_bounds__(256, 2) void seb_inv_finish_kernel(double *__restrict__ U, int64_t ldu, const double *__restrict__ Tinv,
                                                                int k) {
    __shared__ __attribute__((aligned(16))) SebLds lds;
    const int rb = blockIdx.x;
    double *C = U + (int64_t)k * SB_T * ldu + (int64_t)rb * SB_T;
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    seb_tile_product(C, ldu, Tinv, SB_T, SB_T / SB_KC, acc, lds);      // sum_c S[r][c] Tinv[c'][c]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < 4; ++b) C[(int64_t)seb_col(a, r) * ldu + seb_row(b)] = -acc[a][b][r];
}

// X = U U' on the tiles (bi, bj), bj <= bi, numbered row after row (the longest K ranges first); each value goes to both
// halves of X, a diagonal tile's from its lower triangle
__global__ __launch_bounds__(256, 2) void seb_xxt_kernel(const double *__restrict__ U, int64_t ldu, int np, double *__restrict__ X,
                                                         int64_t ld) {
    __shared__ __attribute__((aligned(16))) SebLds lds;
    int bi = 0, bj = (int)blockIdx.x;
    while (bj > bi) { bj -= bi + 1; ++bi; }
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    const double *Uk = U + (int64_t)bi * SB_T * ldu;      // the blocks left of column bi are zero in both rows
    seb_tile_product(Uk + (int64_t)bi * SB_T, ldu, Uk + (int64_t)bj * SB_T, ldu, (np - bi) * (SB_T / SB_KC), acc, lds);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t i = (int64_t)bi * SB_T + seb_row(b), j = (int64_t)bj * SB_T + seb_col(a, r);
                if (i < j) continue;
                X[i + j * ld] = acc[a][b][r];
                X[j + i * ld] = acc[a][b][r];
            }
}

// out[q][c] = sum_r X[r][c] B[r][q] for the six columns B = [F21 | V[3:]] and diag[c] = X[c][c]: a wave per column of X
// (X is symmetric: its column is its row), lanes stride the rows, then wave_sum -- a fixed order
__global__ __launch_bounds__(256) void seb_xb_kernel(const double *__restrict__ X, int64_t ld, int m, const double *__restrict__ F,
                                                     int64_t ldf, const double *__restrict__ V, int n, double *__restrict__ out,
                                                     int mp, double *__restrict__ diag) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= m) return;
    const double *col = X + (int64_t)c * ld;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = lane; r < m; r += 64) {
        const double x = col[r];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            s[q] = fma(x, F[(int64_t)q * ldf + 3 + r], s[q]);
            s[3 + q] = fma(x, V[(int64_t)q * n + 3 + r], s[3 + q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double t = wave_sum(s[q]);
        if (lane == 0) out[(int64_t)q * mp + c] = t;
    }
    if (lane == 0) diag[c] = col[c];
}

// Q (np x np, row-major) on 32 x 32 tiles of its lower triangle: the value of (i, j), i >= j, is computed once and
// written to both halves (the upper one directly, the lower one through an LDS transpose: both coalesced).
//   i, j < n        -k^2 sw_i sw_j (Z - W V' - V W')_ij,  Z = diag(0, X)
//   n <= i < n + 3  trv[i - n][j] (j < n), br[(i - n) + 3 (j - n)] otherwise
//   beyond          0 (the padding tps_se_kernel reads)
__global__ __launch_bounds__(256) void seb_q_kernel(const double *__restrict__ X, int64_t ld, const double *__restrict__ sw,
                                                    const double *__restrict__ V, const double *__restrict__ W,
                                                    const double *__restrict__ trv, const double *__restrict__ br, int n, int np,
                                                    double *__restrict__ q) {
    __shared__ double tile[32][33];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i = ti * 32 + tx;
    const double k2 = PHI_K * PHI_K;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int jl = ty + 8 * p, j = tj * 32 + jl;
        double val = 0.0;
        const bool own = i < np && j < np && i >= j;
        if (own) {
            if (i < n) {
                const double z = j >= 3 ? X[(int64_t)(i - 3) + (int64_t)(j - 3) * ld] : 0.0;
                double t = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int64_t o = (int64_t)c * n;
                    t += W[o + i] * V[o + j] + V[o + i] * W[o + j];
                }
                val = -k2 * sw[i] * sw[j] * (z - t);
            } else if (i < n + 3) {
                val = j < n ? trv[(int64_t)(i - n) * n + j] : br[(i - n) + 3 * (j - n)];
            }
            q[(int64_t)j * np + i] = val;
        }
        tile[jl][tx] = val;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int il = ty + 8 * p;
        const int64_t row = (int64_t)ti * 32 + il, colq = (int64_t)tj * 32 + tx;
        if (row < np && colq < np && row >= colq) q[row * np + colq] = tile[tx][il];
    }
}

// W of the compact WY form of a two-sided transformation by Q = H0 H1 H2 = I - V T V':
//   forward  Q' G Q = G - W V' - V W',  W = Y T  - 1/2 V (T' M T)     (Y = G V, M = V'Y, G symmetric)
//   reverse  Q G Q' = G - W V' - V W',  W = Y T' - 1/2 V (T M T')
// (the algebra of the fit's own projection, tps_fit.hip)
static void seb_wy(const std::vector<double> *hv, const double *htau, int64_t n, const std::vector<double> &Y, bool rev,
                   std::vector<double> &W) {
    double G[3][3], T[3][3] = {{0}}, M[3][3], A[3][3], MA[3][3], S[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double g = 0.0, mm = 0.0;
            for (int64_t i = 0; i < n; ++i) { g += hv[a][i] * hv[b][i]; mm += hv[a][i] * Y[(size_t)b * n + i]; }
            G[a][b] = g; M[a][b] = mm;
        }
    for (int j = 0; j < 3; ++j) {      // larft, forward, columnwise
        T[j][j] = htau[j];
        for (int i = 0; i < j; ++i) {
            double sum = 0.0;
            for (int l = i; l < j; ++l) sum += T[i][l] * G[l][j];
            T[i][j] = -htau[j] * sum;
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[a][b] = rev ? T[b][a] : T[a][b];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { double t = 0.0; for (int c = 0; c < 3; ++c) t += 0.5 * (M[a][c] + M[c][a]) * A[c][b]; MA[a][b] = t; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { double t = 0.0; for (int c = 0; c < 3; ++c) t += A[c][a] * MA[c][b]; S[a][b] = t; }
    W.assign(3 * (size_t)n, 0.0);
    for (int64_t i = 0; i < n; ++i)
        for (int b = 0; b < 3; ++b) {
            double t = 0.0;
            for (int c = 0; c < 3; ++c) t += Y[(size_t)c * n + i] * A[c][b] - 0.5 * hv[c][i] * 0.5 * (S[c][b] + S[b][c]);
            W[(size_t)b * n + i] = t;
        }
}

namespace {
struct PoolBlock {
    void *p = nullptr;
    ~PoolBlock() { pool_release(p); }
    template <typename T> T *get(size_t count) { p = pool_alloc(sizeof(T) * std::max<size_t>(count, 1)); return (T *)p; }
};
// declared after the blocks: nothing of the build is in flight when they go back to the pool, whatever the way out
struct StreamsIdle {
    hipStream_t s, s2;
    ~StreamsIdle() { (void)hipStreamSynchronize(s); (void)hipStreamSynchronize(s2); }
};
}  // namespace

int se_build_device(const mhs_tps *t, SeState &st) {
    // one build at a time on a slot: lane 0's streams and event pool are those of mhs_tps_fit_many, which holds this mutex too
    std::lock_guard<std::mutex> build_lock(batch_mutex());
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = t->n;
    const int m = (int)(n - 3);
    const double lam = t->lambda;
    const TpsPrep *P = t->prep.get();
    std::vector<double> sw((size_t)n, 1.0), hvl[3];
    double htl[3], Rl[9];
    const std::vector<double> *hv = hvl;
    const double *htau = htl, *R = Rl;
    const double *uv = t->knots_uv.data();
    if (P) { sw = P->sw; hv = P->hv; htau = P->htau; R = P->R; }
    else {   // mhs_tps_from_coef: unit weights, the QR of [1 u v]
        std::vector<double> T((size_t)(3 * n));
        for (int64_t i = 0; i < n; ++i) { T[i] = 1.0; T[n + i] = uv[i]; T[2 * n + i] = uv[n + i]; }
        qr_n3(T, n, hvl, htl, Rl);
        if (!(fabs(Rl[8]) > 1e-10 * fabs(Rl[0]) && fabs(Rl[4]) > 1e-10 * fabs(Rl[0]))) {
            set_error("mhs_tps_predict_se: collinear knots");
            return MHS_ERR_NUMERIC;
        }
    }
    FitLane *lane = nullptr;
    if (int rc = fit_lane(0, &lane)) return rc;
    hipStream_t s = lane->s;
    const int m_pad = chol_padded(m), npan = m_pad / SB_T;
    const int64_t ld = ((int64_t)(3 + m_pad) + 15) & ~(int64_t)15;      // tps_fit_lane's
    const int64_t np = (n + 3 + 15) / 16 * 16;

    PoolBlock bA, bU, bvec, bwork, bq;
    StreamsIdle idle{lane->s, lane->s2};
    // the matrix is shifted by one double: row 3, where F22 starts, sits on a 16-byte boundary in every column
    double *A = bA.get<double>((size_t)(ld * (3 + m_pad)) + 2);
    double *U = bU.get<double>((size_t)m_pad * m_pad);
    // vectors: u v (2n) | sw (n) | V (3n) | W (3n) | Y (3n) | trv (3n) | rhs (m_pad + 8) | xb (6 m_pad) | diag (m_pad) | br (16) | info
    const size_t nv = 15 * (size_t)n + 8 * (size_t)m_pad + 64;
    double *vec = bvec.get<double>(nv);
    double *work = bwork.get<double>(chol_work_doubles(m));
    if (!A || !U || !vec || !work) return MHS_ERR_ALLOC;
    A += 1;
    double *duv = vec, *dsw = duv + 2 * n, *dV = dsw + n, *dW = dV + 3 * n, *dY = dW + 3 * n, *dtrv = dY + 3 * n;
    double *drhs = dtrv + 3 * n + (n & 1);                 // 16-byte aligned (the block is, and every piece before it is even)
    double *dxb = drhs + m_pad + 8, *ddiag = dxb + 6 * (size_t)m_pad, *dbr = ddiag + m_pad;
    int *info = (int *)(dbr + 16);

    // ---- 1. F ----
    std::vector<double> Vh(3 * (size_t)n), Yh(3 * (size_t)n), Wh;
    for (int k = 0; k < 3; ++k) std::copy(hv[k].begin(), hv[k].begin() + n, Vh.begin() + (size_t)k * n);
    MHS_HIP(hipMemcpyAsync(duv, uv, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
    MHS_HIP(hipMemcpyAsync(dsw, sw.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
    MHS_HIP(hipMemcpyAsync(dV, Vh.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(seb_kv_kernel, dim3((unsigned)n), dim3(256), 0, s, duv, duv + n, dsw, (int)n, dV, dY);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(Yh.data(), dY, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    seb_wy(hv, htau, n, Yh, false, Wh);
    MHS_HIP(hipMemcpyAsync(dW, Wh.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(seb_f_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, s, duv, duv + n, dsw, (int)n, dV,
                       dW, lam, A, ld);
    MHS_HIP(hipGetLastError());
    // ---- 2. Cholesky of F22, x = X wv2 ----
    std::vector<double> rhs((size_t)m, 0.0);
    if (P) std::copy(P->wv.begin() + 3, P->wv.begin() + 3 + m, rhs.begin());
    MHS_HIP(hipMemcpyAsync(drhs, rhs.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
    if (int rc = cholesky_solve_mfma(*lane, A, ld, 3, m, drhs, work, info)) {
        if (rc == MHS_ERR_NUMERIC) set_error("mhs_tps_predict_se: B + lambda I is not positive definite");
        return rc;
    }
    // ---- 3. U = L^-T, X = U U' (X takes the place of L) ----
    double *a = A + 3 * ld + 3;
    MHS_HIP(hipMemsetAsync(U, 0, sizeof(double) * (size_t)m_pad * m_pad, s));
    hipLaunchKernelGGL(seb_inv_diag_kernel, dim3(SB_T * SB_T / 256, (unsigned)npan), dim3(256), 0, s, U, (int64_t)m_pad, work);
    for (int k = 0; k < npan; ++k) {
        if (k > 0)
            hipLaunchKernelGGL(seb_inv_finish_kernel, dim3((unsigned)k), dim3(256), 0, s, U, (int64_t)m_pad,
                               work + (size_t)k * 2 * SB_T * SB_T, k);
        if (k + 1 < npan)
            hipLaunchKernelGGL(seb_inv_update_kernel, dim3((unsigned)((k + 1) * (npan - k - 1))), dim3(256), 0, s, U, (int64_t)m_pad,
                               a, ld, k);
    }
    hipLaunchKernelGGL(seb_xxt_kernel, dim3((unsigned)(npan * (npan + 1) / 2)), dim3(256), 0, s, U, (int64_t)m_pad, npan, a, ld);
    MHS_HIP(hipGetLastError());
    // ---- 4. X [F21 | V], diag X; the O(n) remainder on the host ----
    hipLaunchKernelGGL(seb_xb_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, a, ld, m, A, ld, dV, (int)n, dxb, m_pad, ddiag);
    MHS_HIP(hipGetLastError());
    std::vector<double> xb(6 * (size_t)m_pad), dg((size_t)m), x((size_t)m), G3(3 * (size_t)n);
    MHS_HIP(hipMemcpyAsync(xb.data(), dxb, sizeof(double) * xb.size(), hipMemcpyDeviceToHost, s));
    MHS_HIP(hipMemcpyAsync(dg.data(), ddiag, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipMemcpyAsync(x.data(), drhs, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    for (int c = 0; c < 3; ++c)
        MHS_HIP(hipMemcpyAsync(G3.data() + (size_t)c * n, A + (int64_t)c * ld, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    const double *Y = xb.data();                               // Y = X F21: column c at Y + c m_pad
    double S3[9];
    for (int p = 0; p < 3; ++p)
        for (int b = 0; b < 3; ++b) {
            double sum = G3[p + (size_t)b * n];
            for (int64_t k = 0; k < m; ++k) sum -= G3[(3 + k) + (size_t)p * n] * Y[k + (size_t)b * m_pad];
            S3[p + 3 * b] = sum;
        }
    double trX = 0.0;
    for (int64_t i = 0; i < m; ++i) trX += dg[(size_t)i];
    st.eff_df = (double)n - lam * trX;
    if (P) {
        double rss = 0.0;
        for (int64_t i = 0; i < m; ++i) rss += x[(size_t)i] * x[(size_t)i];
        st.rss_w = lam * lam * rss;
        st.sigma2 = (st.rss_w + P->pure_ss) / ((double)P->N - st.eff_df);
    }
    double Ri[9] = {0};      // R^-1 (upper triangular)
    for (int c = 0; c < 3; ++c) {
        Ri[c + 3 * c] = 1.0 / R[c + 3 * c];
        for (int r = c - 1; r >= 0; --r) {
            double sum = 0.0;
            for (int k = r + 1; k <= c; ++k) sum += R[r + 3 * k] * Ri[k + 3 * c];
            Ri[r + 3 * c] = -sum / R[r + 3 * r];
        }
    }
    // top-right: S Q [[I], [-Y]] R^-T, scaled as Q stores it
    std::vector<double> TR((size_t)(n * 3), 0.0);
    for (int c = 0; c < 3; ++c) {
        for (int p = 0; p < 3; ++p) TR[p + (size_t)c * n] = Ri[c + 3 * p];
        for (int64_t i = 0; i < m; ++i) {
            double sum = 0.0;
            for (int p = 0; p < 3; ++p) sum += Y[i + (size_t)p * m_pad] * Ri[c + 3 * p];
            TR[(3 + i) + (size_t)c * n] = -sum;
        }
        for (int q = 2; q >= 0; --q) apply_reflector(hv[q], htau[q], TR.data() + (size_t)c * n, n);
        for (int64_t i = 0; i < n; ++i) TR[i + (size_t)c * n] = -PHI_K * sw[(size_t)i] * TR[i + (size_t)c * n];
    }
    // bottom-right: -R^-1 S3 R^-T; Q holds its negative, mirrored from one triangle
    double BR[16] = {0};
    for (int p = 0; p < 3; ++p)
        for (int b = 0; b <= p; ++b) {
            double sum = 0.0;
            for (int c = 0; c < 3; ++c)
                for (int q = 0; q < 3; ++q) sum += Ri[p + 3 * c] * S3[c + 3 * q] * Ri[b + 3 * q];
            BR[p + 3 * b] = BR[b + 3 * p] = sum;
        }
    // top-left: Q diag(0, X) Q' = Z - W V' - V W' with Y = Z V = [0; X V[3:]]
    for (int c = 0; c < 3; ++c) {
        for (int i = 0; i < 3; ++i) Yh[i + (size_t)c * n] = 0.0;
        for (int64_t i = 0; i < m; ++i) Yh[(3 + i) + (size_t)c * n] = xb[(size_t)(3 + c) * m_pad + i];
    }
    seb_wy(hv, htau, n, Yh, true, Wh);
    MHS_HIP(hipMemcpyAsync(dW, Wh.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    MHS_HIP(hipMemcpyAsync(dtrv, TR.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    MHS_HIP(hipMemcpyAsync(dbr, BR, sizeof(double) * 16, hipMemcpyHostToDevice, s));
    double *q = bq.get<double>((size_t)(np * np));
    if (!q) return MHS_ERR_ALLOC;
    const unsigned nt = (unsigned)((np + 31) / 32);
    hipLaunchKernelGGL(seb_q_kernel, dim3(nt, nt), dim3(256), 0, s, a, ld, dsw, dV, dW, dtrv, dbr, (int)n, (int)np, q);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipStreamSynchronize(s));
    st.q_dev = q;
    bq.p = nullptr;
    st.n = n; st.np = np; st.lambda = lam;
    st.built_on = MHS_SE_BUILD_DEVICE;
    st.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MHS_OK;
}

}  // namespace mhs
