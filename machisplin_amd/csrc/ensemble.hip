// Per-cell evaluation of the six ensemble members on gfx950 and their weighted sum:
// the terra::predict(rast_stack, model) loop of machisplin.mltps Step 2 (V73:447-619).
//
// Every kernel reads the C covariate planes once per cell (coalesced along columns),
// generates LONG/LAT from the grid affine, and writes  out (+)= pred * weight.
// Regimes: lm / nnet / earth are HBM-bound (a few dozen flops per cell);
// ksvm is FP64-VALU bound (nSV exp-pairs per cell, support vectors through the scalar
// cache, exp from a 64-entry 2^(j/64) table in LDS); gbm / randomForest are LDS-latency
// bound tree walks (node records staged chunk-wise in LDS, predictors parked in LDS so a
// lane can index them by the node's split variable).
//
// This file holds the kernels and every function that launches one, and nothing else: the build has no relocatable device
// code, so a kernel and its launch share a translation unit.  The model handle (loaders, replicas, release) is models.hip,
// the host-pointer pipelines are ensemble_host.hip; both are host code and reach the device through the launchers declared
// in ensemble_int.h.  The gbm kernels do NOT move to a gbm.hip beside forest.hip, although the code suggests that split:
// bench.py decides whether the PMC counters under profiles/ describe the build it runs by hashing a fixed list of member-kernel
// sources (this file, forest.hip, ensemble_int.h, devmath.h, the *.inc loops), and a kernel in a file that is not on the list
// would escape the hash for good.  Member kernels stay in this file and in forest.hip.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <type_traits>
#include <vector>
#include "common.h"
#include "devmath.h"

#include "ensemble_int.h"

namespace mhs {

// ------------------------------------------------------------------------- lm --
__global__ __launch_bounds__(256) void lm_kernel(const double *__restrict__ coef, int p, StackDev s,
                                                 PredGeom g, double weight, int accumulate,
                                                 double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.nr * g.nc) return;
    const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
    double acc = coef[0];
    for (int j = 0; j < p; ++j) acc = acc + coef[j + 1] * predictor(s, g, j, row, col);
    emit(out, (int64_t)row * g.ld_out + col, acc, weight, accumulate);
}

// ----------------------------------------------------------------------- nnet --
__device__ __forceinline__ double nnet_sigmoid(double z) {  // nnet.c sigmoid()
    if (z < -15.0) return 0.0;
    if (z > 15.0) return 1.0;
    return 1.0 / (1.0 + exp(-z));
}

template <int P>
__global__ __launch_bounds__(256) void nnet_kernel(const double *__restrict__ w, int H, double y_scale,
                                                   double y_shift, StackDev s, PredGeom g,
                                                   double weight, int accumulate,
                                                   double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.nr * g.nc) return;
    const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
    double x[P];
    bool na = false;
#pragma unroll
    for (int j = 0; j < P; ++j) { x[j] = predictor(s, g, j, row, col); na |= isnan(x[j]); }
    double acc = w[(P + 1) * H];
    for (int h = 0; h < H; ++h) {
        const double *wh = w + h * (P + 1);
        double z = wh[0];
#pragma unroll
        for (int j = 0; j < P; ++j) z = z + wh[1 + j] * x[j];
        acc = acc + w[(P + 1) * H + 1 + h] * nnet_sigmoid(z);
    }
    acc = acc * y_scale + y_shift;
    emit(out, (int64_t)row * g.ld_out + col, na ? NAN : acc, weight, accumulate);
}

// ---------------------------------------------------------------------- earth --
// terms as factor lists: term k owns factors tstart[k] .. tstart[k+1]-1, each (var, dir, cut)
__global__ __launch_bounds__(256) void earth_kernel(const double *__restrict__ coef,
                                                    const double *__restrict__ fcut,
                                                    const int *__restrict__ tstart,
                                                    const int *__restrict__ fvar,
                                                    const int *__restrict__ fdir, int nterms, int p,
                                                    StackDev s, PredGeom g, double weight, int accumulate,
                                                    double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.nr * g.nc) return;
    const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
    bool na = false;
    for (int j = 0; j < p; ++j) na |= isnan(predictor(s, g, j, row, col));
    double acc = 0.0;
    for (int k = 0; k < nterms; ++k) {
        double term = 1.0;
        for (int f = tstart[k]; f < tstart[k + 1]; ++f) {
            const double xv = predictor(s, g, fvar[f], row, col);
            const int d = fdir[f];
            const double fac = d == 2 ? xv : (d == 1 ? fmax(0.0, xv - fcut[f]) : fmax(0.0, fcut[f] - xv));
            term = term * fac;
        }
        acc = acc + coef[k] * term;
    }
    emit(out, (int64_t)row * g.ld_out + col, na ? NAN : acc, weight, accumulate);
}

// ------------------------------------------------- lm + nnet + earth in ONE pass --
// The three HBM-bound members are consecutive in the reference's model order (g, n, m -- V73:340-362): evaluated in
// one kernel the planes are read once and the output plane is read and written once (28 B per cell instead of 3 x
// 28), with exactly the arithmetic and accumulation order of the three separate kernels (bit-identical planes).
struct SmallArgs {
    const double *lm_coef;                                             // NULL: member absent
    const double *nn_w; int nn_H; double nn_scale, nn_shift;           // nn_w NULL: absent
    const double *ea_coef; const double *ea_cut; const int *ea_tstart, *ea_fvar, *ea_fdir; int ea_nterms;   // ea_coef NULL: absent
    double w_lm, w_nn, w_ea;
};
template <int P>
__global__ __launch_bounds__(256) void small_members_kernel(SmallArgs a, StackDev s, PredGeom g, int accumulate,
                                                            double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.nr * g.nc) return;
    const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
    double x[P];
    bool na = false;
#pragma unroll
    for (int j = 0; j < P; ++j) { x[j] = predictor(s, g, j, row, col); na |= isnan(x[j]); }
    const int64_t o = (int64_t)row * g.ld_out + col;
    double v = accumulate ? out[o] : 0.0;
    bool first = !accumulate;
    auto add = [&](double pred, double w) { const double t = pred * w; v = first ? t : v + t; first = false; };
    if (a.lm_coef) {
        double acc = a.lm_coef[0];
#pragma unroll
        for (int j = 0; j < P; ++j) acc = acc + a.lm_coef[j + 1] * x[j];
        add(acc, a.w_lm);
    }
    if (a.nn_w) {
        double acc = a.nn_w[(P + 1) * a.nn_H];
        for (int h = 0; h < a.nn_H; ++h) {
            const double *wh = a.nn_w + h * (P + 1);
            double z = wh[0];
#pragma unroll
            for (int j = 0; j < P; ++j) z = z + wh[1 + j] * x[j];
            acc = acc + a.nn_w[(P + 1) * a.nn_H + 1 + h] * nnet_sigmoid(z);
        }
        acc = acc * a.nn_scale + a.nn_shift;
        add(na ? NAN : acc, a.w_nn);
    }
    if (a.ea_coef) {
        double acc = 0.0;
        for (int k = 0; k < a.ea_nterms; ++k) {
            double term = 1.0;
            for (int f = a.ea_tstart[k]; f < a.ea_tstart[k + 1]; ++f) {
                const double xv = predictor(s, g, a.ea_fvar[f], row, col);
                const int d = a.ea_fdir[f];
                const double fac = d == 2 ? xv : (d == 1 ? fmax(0.0, xv - a.ea_cut[f]) : fmax(0.0, a.ea_cut[f] - xv));
                term = term * fac;
            }
            acc = acc + a.ea_coef[k] * term;
        }
        add(na ? NAN : acc, a.w_ea);
    }
    out[o] = v;
}

// ------------------------------------------------------------------------ svr --
// exp(-700 u) for u in [0, 1] (u = -x / 700: the factor is folded into the per-support-vector coefficients, and
// the range check is the free `clamp` output modifier of the fma that produces u).  In units of ln2/4096,
// y = -700 u 4096/ln2 = 4096 e + j + r, |r| <= 1/2; 2^(j/4096) from a 32 KB LDS table, exp(r ln2/4096) =
// 1 + c r + c^2 r^2 / 2 (truncation < 1e-13 relative).  The magic constant carries the exponent bias, so the low
// word of t is k = (e + 1023) 4096 + j and k << 8 has the finished exponent field on top and j in bits 8..19:
// one bit-field extract gives the table's byte offset and one and-or drops the exponent onto the table entry,
// which is stored as its mantissa bits only.  7 FP64-rate and 3 integer instructions (16 for a 64-entry
// table with a quartic).
constexpr int EXP_TAB_BITS = 12;
constexpr int EXP_TAB_N = 1 << EXP_TAB_BITS;
constexpr double EXP_SCALE = 4096.0 / 0.6931471805599453094;   // 4096 / ln 2
__device__ __forceinline__ double table_exp_neg_acc(double u, const double *tab, double acc) {   // acc + exp(-700 u)
    // k = round(y) by the 1.5*2^52 trick: the integer lands in the low word of t (no v_rndne / v_cvt),
    // kd = t - magic is its exact double; y itself only ever exists inside the two fmas
    const double MAGIC = 0x1.8p52 + 1023.0 * EXP_TAB_N, NK = -EXP_RANGE * EXP_SCALE;
    const double t = fma(u, NK, MAGIC);
    const double kd = t - MAGIC;
    unsigned k8 = (unsigned)__double2loint(t) << 8;   // k >= 1023 * 4096 - 700 * 5910 > 0
    asm("" : "+v"(k8));   // or the extract below is rewritten as a shift and a mask of t's low word
    const double r = fma(u, NK, -kd);
    const double mj = *(const double *)((const char *)tab + __builtin_amdgcn_ubfe(k8, 5, EXP_TAB_BITS + 3));
    const double sj = __hiloint2double((int)((k8 & 0xfff00000u) | (unsigned)__double2hiint(mj)), __double2loint(mj));
    const double C1 = 1.0 / EXP_SCALE, C2 = 0.5 / (EXP_SCALE * EXP_SCALE);
    double q = fma(r, C2, C1);
    q = fma(q, r, 1.0);
    return fma(sj, q, acc);
}

// The same exponential for svr_rt_kernel with TWO integer instructions instead of three; sj, and with it the result, is
// the same double.  k << 8 = ((e + 1023) << 20) + (j << 8), so an entry whose high word is stored as (mantissa's high 20
// bits) - (j << 8), mod 2^32, takes the finished exponent field by ONE shift-add (k < 2^23: the shift loses nothing, no mask).
// The byte offset is one 16-bit shift, (k << 3) & 0xffff = 8 (k mod 8192), which carries bit 12 of k, the exponent's
// lowest bit, along: the table has 8192 entries, the second half a copy of the first (64 KB; rt_exp_table_stage).
// The offset is only right where the 16-bit VALU forms write ZEROS to the destination's upper half.  The GFX9 encoding
// does (gfx90a, gfx942, gfx950; on gfx950 tests/test_ksvm_rowtile_exp_gpu.py shows it); GFX10 and later keep the upper
// half, and this function must not be compiled for them as it stands.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "table_exp_neg_acc_rt relies on v_lshlrev_b16 zeroing bits 16..31 of its destination (GFX9 encoding only)"
#endif
constexpr int EXP_TAB2_N = 2 * EXP_TAB_N;
__device__ __forceinline__ void rt_exp_table_stage(double *tab2, const double *__restrict__ gtab, int tid, int nthreads) {
    for (int i = tid; i < EXP_TAB2_N; i += nthreads) {
        const int j = i & (EXP_TAB_N - 1);
        const double e = gtab[j];
        tab2[i] = __hiloint2double((int)(((unsigned)__double2hiint(e) & 0x000fffffu) - ((unsigned)j << 8)), __double2loint(e));
    }
}
// magic and c1 are RT_EXP_MAGIC and RT_EXP_C1 in vector registers (rt_exp_consts): each is the second constant of an fma whose
// first already takes the instruction's one scalar operand.  Left to the compiler, inside the resident kernel's tile loop they
// live in scalar registers and are copied over in every trip of the support-vector loop, two more instructions per 145.
constexpr double RT_EXP_MAGIC = 0x1.8p52 + 1023.0 * EXP_TAB_N, RT_EXP_C1 = 1.0 / EXP_SCALE;
__device__ __forceinline__ void rt_exp_consts(double &magic, double &c1) {
    magic = RT_EXP_MAGIC; c1 = RT_EXP_C1;
    asm("" : "+v"(magic));
    asm("" : "+v"(c1));
}
__device__ __forceinline__ double table_exp_neg_acc_rt(double u, const double *tab2, double acc, double magic, double c1) {   // acc + exp(-700 u)
    const double MAGIC = RT_EXP_MAGIC, NK = -EXP_RANGE * EXP_SCALE;
    const double t = fma(u, NK, magic);
    const double kd = t - MAGIC;
    const unsigned k = (unsigned)__double2loint(t);
    unsigned off;
    asm("v_lshlrev_b16 %0, 3, %1" : "=v"(off) : "v"(k));
    const double r = fma(u, NK, -kd);
    const double mj = *(const double *)((const char *)tab2 + off);
    const double sj = __hiloint2double((int)((k << 8) + (unsigned)__double2hiint(mj)), __double2loint(mj));
    const double C2 = 0.5 / (EXP_SCALE * EXP_SCALE);
    double q = fma(r, C2, c1);
    q = fma(q, r, 1.0);
    return fma(sj, q, acc);
}

// per support vector: [b_0 .. b_{P-1}, a], b_k = -2 sigma sv_k / 700, a = (sigma |sv|^2 - ln(|alpha| / amax)) / 700:
// u = a + sigma |x|^2 / 700 + b.x = (sigma |x - sv|^2 - ln(|alpha| / amax)) / 700 >= 0 and exp(-700 u) =
// |alpha| / amax K(x, sv).  With the coefficient inside the exponent the term is accumulated by the fma that
// finishes the exponential (acc += 2^e 2^(j/4096) * q); the support vectors with alpha > 0 come first, the
// others are summed separately and subtracted.
template <int P, int R>
__global__ __launch_bounds__(256) void svr_kernel(const double *__restrict__ svp, int nsv, int stride,
                                                  int npos, const double *__restrict__ xcs,
                                                  const double *__restrict__ gtab, double sigma, double b,
                                                  double amax,
                                                  double y_center, double y_scale, StackDev s, PredGeom g,
                                                  double weight, int accumulate, double *__restrict__ out) {
    __shared__ double etab[EXP_TAB_N];
    for (int i = threadIdx.x; i < EXP_TAB_N; i += 256) {   // mantissa bits of 2^(j/4096)
        const double e = gtab[i];
        etab[i] = __hiloint2double(__double2hiint(e) & 0x000fffff, __double2loint(e));
    }
    __syncthreads();
    const int64_t total = (int64_t)g.nr * g.nc;
    const int64_t half = (total + R - 1) / R;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= half) return;
    double x[R][P], q[R], acc[R];
    bool na[R];
    int row[R], col[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        int64_t i = i0 + c * half;
        if (i >= total) i = total - 1;
        row[c] = (int)(i / g.nc); col[c] = (int)(i - (int64_t)row[c] * g.nc);
        na[c] = false; q[c] = 0.0; acc[c] = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double xv = predictor(s, g, j, row[c], col[c]);
            na[c] |= isnan(xv);
            x[c][j] = (xv - xcs[j]) / xcs[P + j];
            q[c] = fma(x[c][j], x[c][j], q[c]);
        }
        q[c] = (sigma / EXP_RANGE) * q[c];
    }
    double accn[R];
#pragma unroll
    for (int c = 0; c < R; ++c) accn[c] = 0.0;
    auto sum_range = [&](int v0, int v1, double (&a)[R]) {
        for (int v = v0; v < v1; ++v) {
            const double *sp = svp + (int64_t)v * stride;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                // the LAST predictor first: in grid mode it is LAT, constant along a raster row -- svr_rt_kernel forms this
                // term once per row and support vector with the same fma, so the two kernels agree bit for bit
                double arg = q[c] + fma(sp[P - 1], x[c][P - 1], sp[P]);
#pragma unroll
                for (int j = 0; j < P - 1; ++j) arg = fma(sp[j], x[c][j], arg);
                arg = fmin(fmax(arg, 0.0), 1.0);   // folds into the clamp modifier of the last fma
                a[c] = table_exp_neg_acc(arg, etab, a[c]);
            }
        }
    };
    sum_range(0, npos, acc);
    sum_range(npos, nsv, accn);
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int64_t i = i0 + c * half;
        if (i < total) {
            const double pred = ((acc[c] - accn[c]) * amax - b) * y_scale + y_center;
            emit(out, (int64_t)row[c] * g.ld_out + col[c], na[c] ? NAN : pred, weight, accumulate);
        }
    }
}

// ROW-TILE form of the ksvm kernel (round 3): a wave = 64 R consecutive cells of ONE raster row.  LAT is the last
// predictor of every model (V73:127-138) and the same for all of the wave's cells, so its term b_LAT x_LAT + a of the
// exponent is formed ONCE per wave and support vector -- 128 vectors at a time, two per lane, parked in a wave-private
// 1 KB of LDS and read back as a broadcast -- instead of once per cell.  A wave that does NOT fold its cells' q (below)
// adds exactly what svr_kernel adds, bit for bit; a folding wave's plane agrees with svr_kernel's to ~2e-13 of the
// prediction (tests: test_ksvm_row_tile_kernel_*).
// Vector instructions per (cell, SV) of the loop at P = 5, step by step: 15 lane per cell (svr_kernel), 14 with the LAT term
// per wave, 13 with q folded (below; 14 where the wave does not fold), and with TAB2 12 (13 where it does not fold).
// TAB2 chooses the exponential: table_exp_neg_acc_rt and its 64 KB table (the same bits as svr_kernel's form:
// tests/test_ksvm_rowtile_exp_gpu.py), or table_exp_neg_acc and the 32 KB table.  NW is the block's waves; launch_svr sets
// both (svr_rt_tab2, svr_rt_waves).  A wave has its own tile and its own slice of aw; the only block-wide barrier is the
// one behind the table's staging.  svr_rt_kernel gives every wave one tile; svr_rt_resident_kernel lets a wave pull tile
// after tile.
//
// exp() for a cell's back-scaling, as a CALL.  Inlined into the resident kernel's tile loop, its eleven polynomial constants
// are hoisted out of that loop into vector registers for the whole kernel (141 VGPRs at P = 5; held to 128 the compiler
// spills them, 44 bytes of scratch); the callee keeps them to itself.  The same function, the same bits.
__device__ __attribute__((noinline)) double svr_rt_exp_call(double z) { return exp(z); }
// HAND (P = 5, R = 3, TAB2; the resident kernel's default): the support-vector loop of a staged chunk is the hand-scheduled
// block of svr_rt_loop5.inc / svr_rt_loop5q.inc (tools/gen_svr_rt_asm.py) -- the same vector instructions on the same
// values in the same order as the compiler's loop below, so the same bits.  The compiler's loop drains lgkmcnt(0) directly
// behind every table read and behind every support vector's scalar load.  The block keeps two table reads in flight on
// three register sets and waits with counted lgkmcnt(N); the next support vector's record (double-buffered in 2 x 8
// scalar registers) and ap are requested a support vector ahead and drained once, where the drain is cheapest.
// One tile: the 64 R cells of row `row` from column `tcol` on, R cells per lane.  aw is the wave's own 1 KB of LDS.
template <int P, int R, bool TAB2, bool EXPCALL, bool HAND = false>
__device__ __forceinline__ void svr_rt_tile(const double *__restrict__ svp, int nsv, int stride, int npos,
                                            const double *__restrict__ xcs, const double *etab, double *aw, double sigma, double b,
                                            double amax, double y_center, double y_scale, const StackDev &s, const PredGeom &g,
                                            int row, int tcol, int lane, double weight, int accumulate, double *__restrict__ out) {
    constexpr int CH = 128;
    static_assert(!HAND || (P == 5 && R == 3 && TAB2), "svr_rt_loop5*.inc are written for P = 5, R = 3 and the 64 KB table");
    double x[R][P], q[R], acc[R], accn[R];
    bool na[R], ok[R];
    int col[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int cc = tcol + c * 64 + lane;
        ok[c] = cc < g.nc;
        col[c] = min(cc, g.nc - 1);
        na[c] = false; q[c] = 0.0; acc[c] = 0.0; accn[c] = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double xv = predictor(s, g, j, row, col[c]);
            na[c] |= isnan(xv);
            x[c][j] = (xv - xcs[j]) / xcs[P + j];
            q[c] = fma(x[c][j], x[c][j], q[c]);
        }
        q[c] = (sigma / EXP_RANGE) * q[c];
    }
    const double xlat = x[0][P - 1];                       // the row's scaled LAT: the same value in every lane and cell
    // The cell's own term q = sigma |x|^2 / 700 of the exponent is the one addition per (cell, SV) that is left beside the
    // P - 1 fmas.  With S the LARGEST q of the wave's cells, u + (S - q_c) is still >= 0 and is formed with S folded into the
    // per-wave term above; the cell's sum then comes out scaled by exp(-700 (S - q_c)), which ONE exact exponential per cell
    // undoes at the end -- one vector instruction per pair fewer.  Neighbouring cells: S - q_c is a few hundredths.
    // Where the wave's q spread more than 0.5 (terms would be flushed that the cell's scale brings back) the wave keeps
    // the per-pair addition.
    double qhi = -1.0, qlo = 2e300;
#pragma unroll
    for (int c = 0; c < R; ++c) { qhi = fmax(qhi, q[c]); qlo = fmin(qlo, q[c]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { qhi = fmax(qhi, __shfl_xor(qhi, o)); qlo = fmin(qlo, __shfl_xor(qlo, o)); }
    // (qhi, qlo are the same in every lane after the butterfly; readfirstlane tells the COMPILER so: with a wave-uniform
    // branch the support-vector loop keeps its counter and the LDS cursor on the scalar unit -- round 5: the loop spent 3 of
    // its 42 vector instructions per support vector on them, 14.0 -> 13.1 per (cell, SV))
    const bool fold = __builtin_amdgcn_readfirstlane((int)(qhi - qlo <= 0.5)) != 0;   // false too when every cell of the wave is NA (qhi = -1, qlo = 2e300)
    const double S = fold ? qhi : 0.0;
    double magic = 0.0, c1 = 0.0;
    if constexpr (TAB2 && !HAND) rt_exp_consts(magic, c1);      // the hand-scheduled loop sets its own two registers
    auto sum_range = [&](int v0, int v1, double (&a)[R], auto folded) {
        constexpr bool FOLD = decltype(folded)::value;
        auto pair = [&](const double *sp, const double ap) {
#pragma unroll
            for (int c = 0; c < R; ++c) {
                double arg = FOLD ? ap : q[c] + ap;
#pragma unroll
                for (int j = 0; j < P - 1; ++j) arg = fma(sp[j], x[c][j], arg);
                arg = fmin(fmax(arg, 0.0), 1.0);
                a[c] = TAB2 ? table_exp_neg_acc_rt(arg, etab, a[c], magic, c1) : table_exp_neg_acc(arg, etab, a[c]);
            }
        };
        for (int vb = v0; vb < v1; vb += CH) {
            const int n = min(CH, v1 - vb);
            __builtin_amdgcn_wave_barrier();
            for (int e = lane; e < n; e += 64) {
                const double *sp = svp + (int64_t)(vb + e) * stride;
                aw[e] = fma(sp[P - 1], xlat, sp[P]) + S;
            }
            __builtin_amdgcn_wave_barrier();
            if constexpr (HAND) {
                // nt pipelined trips of four, then rem = 1 .. 4 support vectors on their own (tools/gen_svr_rt_asm.py)
                int nt = (n - 1) >> 2;
                const int rem = n - 4 * nt;
                unsigned ca = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)aw;
                const double *rec = svp + (int64_t)vb * stride;          // the chunk's first record; stride * 8 bytes to the next
                const int rec_bytes = stride * (int)sizeof(double);
                const double NK = -EXP_RANGE * EXP_SCALE, NMAGIC = -RT_EXP_MAGIC, C2 = 0.5 / (EXP_SCALE * EXP_SCALE);
                constexpr unsigned long long MGB = __builtin_bit_cast(unsigned long long, RT_EXP_MAGIC),
                                             C1B = __builtin_bit_cast(unsigned long long, RT_EXP_C1);
#define MHS_SVR_LOOP_CLOBBERS                                                                                                       \
    "memory", "scc", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98",     \
        "s99", "s100", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114",       \
        "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127"
#define MHS_SVR_LOOP_X                                                                                                              \
    [x00] "v"(x[0][0]), [x01] "v"(x[0][1]), [x02] "v"(x[0][2]), [x03] "v"(x[0][3]), [x10] "v"(x[1][0]), [x11] "v"(x[1][1]),        \
        [x12] "v"(x[1][2]), [x13] "v"(x[1][3]), [x20] "v"(x[2][0]), [x21] "v"(x[2][1]), [x22] "v"(x[2][2]), [x23] "v"(x[2][3]),    \
        [mglo] "i"((unsigned)MGB), [mghi] "i"((unsigned)(MGB >> 32)), [c1lo] "i"((unsigned)C1B),                    \
        [c1hi] "i"((unsigned)(C1B >> 32)), [rem] "s"(rem), [sp] "s"(rec), [st] "s"(rec_bytes), [nk] "s"(NK), [nm] "s"(NMAGIC),     \
        [c2] "s"(C2)
                if constexpr (FOLD)
                    asm volatile(
#include "svr_rt_loop5.inc"
                        : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [ca] "+v"(ca), [nt] "+s"(nt)
                        : MHS_SVR_LOOP_X
                        : MHS_SVR_LOOP_CLOBBERS);
                else
                    asm volatile(
#include "svr_rt_loop5q.inc"
                        : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [ca] "+v"(ca), [nt] "+s"(nt)
                        : MHS_SVR_LOOP_X, [q0] "v"(q[0]), [q1] "v"(q[1]), [q2] "v"(q[2])
                        : MHS_SVR_LOOP_CLOBBERS);
#undef MHS_SVR_LOOP_X
#undef MHS_SVR_LOOP_CLOBBERS
                continue;
            }
            const double *sp = svp + (int64_t)vb * stride;
            const double *ar = aw;
            int e = 0;
            for (; e + 4 <= n; e += 4) {          // four support vectors per trip: one cursor bump, immediate LDS offsets
#pragma unroll
                for (int k = 0; k < 4; ++k) pair(sp + (int64_t)k * stride, ar[e + k]);
                sp += (int64_t)4 * stride;
            }
            for (; e < n; ++e) { pair(sp, ar[e]); sp += stride; }
        }
    };
    if (fold) {
        sum_range(0, npos, acc, std::true_type());
        sum_range(npos, nsv, accn, std::true_type());
    } else {
        sum_range(0, npos, acc, std::false_type());
        sum_range(npos, nsv, accn, std::false_type());
    }
#pragma unroll
    for (int c = 0; c < R; ++c)
        if (ok[c]) {
            const double back = fold ? (EXPCALL ? svr_rt_exp_call(EXP_RANGE * (S - q[c])) : exp(EXP_RANGE * (S - q[c]))) : 1.0;
            const double pred = ((acc[c] - accn[c]) * back * amax - b) * y_scale + y_center;
            emit(out, (int64_t)row * g.ld_out + col[c], na[c] ? NAN : pred, weight, accumulate);
        }
}

// A tile by its index, for the resident kernel (exp() as a call).
template <int P, int R, bool TAB2, bool HAND>
__device__ __forceinline__ void svr_rt_run(int64_t tile, const double *__restrict__ svp, int nsv, int stride, int npos,
                                           const double *__restrict__ xcs, const double *etab, double *aw, double sigma, double b,
                                           double amax, double y_center, double y_scale, const StackDev &s, const PredGeom &g,
                                           int tiles_per_row, int lane, double weight, int accumulate, double *__restrict__ out) {
    const int row = (int)(tile / tiles_per_row), tcol = (int)(tile - (int64_t)row * tiles_per_row) * (64 * R);
    svr_rt_tile<P, R, TAB2, true, HAND>(svp, nsv, stride, npos, xcs, etab, aw, sigma, b, amax, y_center, y_scale, s, g, row, tcol, lane, weight,
                                  accumulate, out);
}
template <int NW, bool TAB2>
__device__ __forceinline__ void svr_rt_stage(double *etab, const double *__restrict__ gtab) {
    if constexpr (TAB2) rt_exp_table_stage(etab, gtab, threadIdx.x, 64 * NW);
    else
        for (int i = threadIdx.x; i < EXP_TAB_N; i += 64 * NW) {   // mantissa bits of 2^(j/4096)
            const double e = gtab[i];
            etab[i] = __hiloint2double(__double2hiint(e) & 0x000fffff, __double2loint(e));
        }
}

// One tile per wave, three cells per lane everywhere: a block per NW tiles.
template <int P, int R, int NW, bool TAB2>
__global__ __launch_bounds__(64 * NW) void svr_rt_kernel(const double *__restrict__ svp, int nsv, int stride,
                                                         int npos, const double *__restrict__ xcs,
                                                         const double *__restrict__ gtab, double sigma, double b,
                                                         double amax, double y_center, double y_scale, StackDev s, PredGeom g,
                                                         int tiles_per_row, double weight, int accumulate, double *__restrict__ out) {
    __shared__ double etab[TAB2 ? EXP_TAB2_N : EXP_TAB_N];
    __shared__ double aw[NW][128];
    svr_rt_stage<NW, TAB2>(etab, gtab);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ntiles = (int64_t)g.nr * tiles_per_row;
    const int64_t tile = (int64_t)blockIdx.x * NW + wave;
    if (tile >= ntiles) return;
    const int row = (int)(tile / tiles_per_row), tcol = (int)(tile - (int64_t)row * tiles_per_row) * (64 * R);
    svr_rt_tile<P, R, TAB2, false>(svp, nsv, stride, npos, xcs, etab, aw[wave], sigma, b, amax, y_center, y_scale, s, g, row, tcol, lane,
                                   weight, accumulate, out);
}

// RESIDENT WAVES.  The launch holds only as many blocks as the device keeps resident at once, and after the staging barrier
// every wave pulls tile indices from *pool (one counter per launch: svr_pool_take) until the pool is empty.  A wave never
// waits for a block-mate or for another block -- nothing can hang --, so a SIMD whose oldest wave ends early gets the next
// tile at once instead of idling until the block's slowest wave is through.  A block that finds the pool empty (fewer tiles
// than waves; a CU-masked stream that runs the blocks in turns) leaves at once.  Which wave takes which tile has no bearing
// on the plane: a tile is the same cells, the same fold decision and the same order of additions whoever runs it.
// The arguments that are no pointers travel as ONE struct behind the five pointers, and every tile reads them afresh from
// the kernel-argument segment through a pointer the compiler cannot see through.  Held across the loop's back edge instead,
// the ~50 scalar registers of arguments and what the compiler hoists out of the tile (the scaling constants) come on top
// of the ~50 of the support-vector loop, and the overflow is parked in vector registers: 159 VGPRs at P = 5 against the
// tile's own 124.  The pointers stay plain __restrict__ arguments: that is what lets the support-vector records come
// through the scalar cache (read through a pointer that was itself loaded, they become vector loads of 32 registers).
struct SvrRtScalars {
    int nsv, stride, npos, tiles_per_row; double sigma, b, amax, y_center, y_scale;
    StackDev s; PredGeom g; double weight; int accumulate;
};
constexpr int SVR_RT_SCALARS_AT = 5 * sizeof(void *);     // byte offset of `sc` among the resident kernel's arguments: FIVE pointers ahead of it
static_assert(alignof(SvrRtScalars) <= 8, "svr_rt_resident_kernel: `sc` does not follow the pointers without padding");
// the kernel rebuilds g and s field by field from the argument segment: a field added to either must be added there
static_assert(sizeof(PredGeom) == 64 && sizeof(StackDev) == 48 && sizeof(SvrRtScalars) == 184,
              "svr_rt_resident_kernel copies PredGeom / StackDev field by field: update the copies and these sizes together");
inline void svr_rt_field_counts(const PredGeom &g, const StackDev &s) {      // never called: fails to compile when a field count changes
    const auto &[g0, g1, g2, g3, g4, g5, g6, g7, g8] = g;
    const auto &[s0, s1, s2, s3, s4, s5, s6, s7] = s;
    (void)g0; (void)g1; (void)g2; (void)g3; (void)g4; (void)g5; (void)g6; (void)g7; (void)g8;
    (void)s0; (void)s1; (void)s2; (void)s3; (void)s4; (void)s5; (void)s6; (void)s7;
}
// The block's LDS as ONE object, the table first: the hand-scheduled loop reads the table at the LDS address its 16-bit
// shift produces, with no base added, so the table must sit at address 0.
template <int NW, bool TAB2>
struct alignas(16) SvrRtLds {
    double etab[TAB2 ? EXP_TAB2_N : EXP_TAB_N];
    double aw[NW][128];
};
template <int P, int R, int NW, bool TAB2, int WPS, bool HAND>
__global__ __launch_bounds__(64 * NW, WPS) void svr_rt_resident_kernel(const double *__restrict__ svp, const double *__restrict__ xcs,
                                                                  const double *__restrict__ gtab, double *__restrict__ out,
                                                                  unsigned long long *__restrict__ pool, SvrRtScalars sc) {
    __shared__ SvrRtLds<NW, TAB2> lds;
    double *const etab = lds.etab;
    auto &aw = lds.aw;
    if constexpr (HAND)      // decided when the kernel is compiled: no instruction is left of it
        if ((unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds.etab != 0u) __builtin_trap();
    svr_rt_stage<NW, TAB2>(etab, gtab);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    typedef const __attribute__((address_space(4))) char *KBytes;
    typedef const __attribute__((address_space(4))) SvrRtScalars *KScalars;
    for (;;) {
        KScalars k = (KScalars)((KBytes)__builtin_amdgcn_kernarg_segment_ptr() + SVR_RT_SCALARS_AT);
        asm volatile("" : "+s"(k));
        unsigned long long t = 0;
        if (lane == 0) t = atomicAdd(pool, 1ull);         // relaxed, device scope: the index is all the waves share
        const int64_t tile = (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) |
                                       (unsigned)__builtin_amdgcn_readfirstlane((int)t));
        const PredGeom g = {k->g.xmin, k->g.ymax, k->g.xres, k->g.yres, k->g.r0, k->g.c0, k->g.nr, k->g.nc, k->g.ld_out};
        if (tile >= (int64_t)g.nr * k->tiles_per_row) return;
        const StackDev s = {k->s.data, k->s.C, k->s.dtype, k->s.plane_stride, k->s.ld, k->s.nodata, k->s.has_nodata, k->s.all_from_planes};
        svr_rt_run<P, R, TAB2, HAND>(tile, svp, k->nsv, k->stride, k->npos, xcs, etab, aw[wave], k->sigma, k->b, k->amax,
                               k->y_center, k->y_scale, s, g, k->tiles_per_row, lane, k->weight, k->accumulate, out);
    }
}

// ---------------------------------------------------------------------- trees --
// gbm_pred / predictRegTree walks.  Dynamic LDS: xs[p][R*256] predictors, then one chunk
// of node records (LDS_NODES) or nothing (nodes read from global, for trees too large).
// SPLIT (few cells, e.g. the station rows): blockIdx.y owns a contiguous share of the LDS chunks and writes its
// partial tree sum to out[blockIdx.y * total + cell] (NaN marks an NA row of a forest); tree_finalize_kernel adds
// the shares in order.  Without it the 5 000 station rows of a step occupy 10 blocks for 10 000 trees' worth of time.
template <bool GBM, bool LDS_NODES, int R, bool NA_ONLY, bool SPLIT = false>
__global__ __launch_bounds__(256) void tree_kernel(const Node *__restrict__ gnodes,
                                                   const int *__restrict__ tree_off,
                                                   const TreeChunk *__restrict__ chunks, int n_chunks,
                                                   int n_trees, double init_f, int p, StackDev s,
                                                   PredGeom g, double weight, int accumulate,
                                                   double *__restrict__ out, const unsigned *__restrict__ na_gate = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (NA_ONLY && na_gate && na_gate[1] == 0u) return;          // the compacted NA list held every NA cell: nothing left to do here
    double *xs = (double *)smem;                                  // [p][R*256]
    Node *lnodes = (Node *)(smem + (size_t)p * R * 256 * sizeof(double));
    const int64_t total = (int64_t)g.nr * g.nc;
    const int64_t half = (total + R - 1) / R;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int row[R], col[R];
    bool na[R];
    double acc[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        int64_t i = i0 + c * half;
        if (i >= total) i = total - 1;
        if (i < 0) i = 0;
        row[c] = (int)(i / g.nc); col[c] = (int)(i - (int64_t)row[c] * g.nc);
        na[c] = false; acc[c] = 0.0;
        for (int j = 0; j < p; ++j) {
            const double xv = predictor(s, g, j, row[c], col[c]);
            na[c] |= isnan(xv);
            xs[(j * R + c) * 256 + threadIdx.x] = xv;
        }
    }
    if (NA_ONLY) {  // fix-up pass after gbm_lut_kernel: only cells holding an NA covariate are walked
        bool any = false;
#pragma unroll
        for (int c = 0; c < R; ++c) any |= na[c] && i0 < half && (i0 + c * half) < total;
        if (!__syncthreads_or(any)) return;
    }
    int ch_begin = 0, ch_end = n_chunks;
    if (SPLIT) {
        const int per = (n_chunks + (int)gridDim.y - 1) / (int)gridDim.y;
        ch_begin = min((int)blockIdx.y * per, n_chunks);
        ch_end = min(ch_begin + per, n_chunks);
    }
    for (int ch = ch_begin; ch < ch_end; ++ch) {
        const TreeChunk tc = chunks[ch];
        if (LDS_NODES) {
            __syncthreads();
            const int4 *src = (const int4 *)(gnodes + tc.node_begin);
            int4 *dst = (int4 *)lnodes;
            for (int e = threadIdx.x; e < tc.node_count; e += 256) dst[e] = src[e];
            __syncthreads();
        }
        for (int t = tc.first_tree; t < tc.first_tree + tc.n_trees; ++t) {
            const int tbase = LDS_NODES ? tree_off[t] - tc.node_begin : tree_off[t];
#pragma unroll
            for (int c = 0; c < R; ++c) {
                if (NA_ONLY && !na[c]) continue;
                Node nd;
                if constexpr (LDS_NODES) nd = lnodes[tbase]; else nd = gnodes[tbase];
                while (nd.var >= 0) {
                    const double xv = xs[(nd.var * R + c) * 256 + threadIdx.x];
                    unsigned nxt;
                    if (GBM) nxt = isnan(xv) ? nd.missing : (xv < nd.val ? nd.left : nd.right);
                    else nxt = (xv <= nd.val) ? nd.left : nd.right;
                    if constexpr (LDS_NODES) nd = lnodes[tbase + nxt]; else nd = gnodes[tbase + nxt];
                }
                acc[c] = acc[c] + nd.val;
            }
        }
    }
    if (SPLIT) {
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int64_t i = i0 + c * half;
            if (i0 < half && i < total) out[(int64_t)blockIdx.y * total + i] = (!GBM && na[c]) ? NAN : acc[c];
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int64_t i = i0 + c * half;
        if (i0 < half && i < total && (!NA_ONLY || na[c])) {
            double pred;
            if (GBM) pred = init_f + acc[c];
            else pred = na[c] ? NAN : acc[c] / (double)n_trees;
            emit(out, (int64_t)row[c] * g.ld_out + col[c], pred, weight, accumulate);
        }
    }
}


// NA cells of a gbm window (round 4).  The predicate-LUT kernels skip cells with an NA covariate; gbm routes those through
// its MissingNode children (gbm_pred).  The strided NA-only pass above walks all 10 000 trees in every BLOCK that holds a
// single NA cell among its 1 024 -- on the reference's bundled rasters (0.09 % NoData along the coast) that was 214 of
// 401 ms per 1e8 cells.  Now: one pass over the planes appends the NA cells to a list (na_collect_kernel), and the walk
// runs over the list, 256 NA cells per block (gbm_na_list_kernel).  A window with more NA cells than the list holds sets
// the overflow word and the strided pass takes over.
__global__ __launch_bounds__(256) void na_collect_kernel(StackDev s, PredGeom g, unsigned cap, unsigned *__restrict__ list) {
    const int64_t total = (int64_t)g.nr * g.nc;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
    bool na = false;
    for (int j = 0; j < s.C; ++j) na |= isnan(predictor(s, g, j, row, col));
    if (na) {
        const unsigned slot = atomicAdd(&list[0], 1u);
        if (slot < cap) list[2 + slot] = (unsigned)i;
        else list[1] = 1u;
    }
}
template <bool LDS_NODES>
__global__ __launch_bounds__(256) void gbm_na_list_kernel(const Node *__restrict__ gnodes, const int *__restrict__ tree_off,
                                                          const TreeChunk *__restrict__ chunks, int n_chunks, double init_f, int p,
                                                          StackDev s, PredGeom g, double weight, int accumulate,
                                                          double *__restrict__ out, const unsigned *__restrict__ list, unsigned cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (list[1]) return;                                          // overflow: the strided pass does the work
    double *xs = (double *)smem;                                  // [p][256]
    Node *lnodes = (Node *)(smem + (size_t)p * 256 * sizeof(double));
    const unsigned count = min(list[0], cap);
    for (unsigned base = blockIdx.x * 256u; base < count; base += gridDim.x * 256u) {
        const bool live = base + threadIdx.x < count;
        const int64_t i = list[2 + (live ? base + threadIdx.x : base)];
        const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
        for (int j = 0; j < p; ++j) xs[j * 256 + threadIdx.x] = predictor(s, g, j, row, col);
        double acc = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const TreeChunk tc = chunks[ch];
            if (LDS_NODES) {
                __syncthreads();
                const int4 *src = (const int4 *)(gnodes + tc.node_begin);
                int4 *dst = (int4 *)lnodes;
                for (int e = threadIdx.x; e < tc.node_count; e += 256) dst[e] = src[e];
                __syncthreads();
            }
            for (int t = tc.first_tree; t < tc.first_tree + tc.n_trees; ++t) {
                const int tbase = LDS_NODES ? tree_off[t] - tc.node_begin : tree_off[t];
                Node nd;
                if constexpr (LDS_NODES) nd = lnodes[tbase]; else nd = gnodes[tbase];
                while (nd.var >= 0) {
                    const double xv = xs[nd.var * 256 + threadIdx.x];
                    const unsigned nxt = isnan(xv) ? nd.missing : (xv < nd.val ? nd.left : nd.right);
                    if constexpr (LDS_NODES) nd = lnodes[tbase + nxt]; else nd = gnodes[tbase + nxt];
                }
                acc = acc + nd.val;
            }
        }
        if (live) emit(out, (int64_t)row * g.ld_out + col, init_f + acc, weight, accumulate);
        __syncthreads();
    }
}

// ---------------------------------------------------------- gbm: predicate LUT --
// Trees grown with interaction.depth = 5 (V73:493) have <= 5 splits, so a tree is a function
// of its S <= 6 split predicates: leaf = LUT[b], b = the S predicate bits.  Per tree a wave
// evaluates S wave-uniform predicates (threshold and variable arrive through the scalar
// cache) instead of walking nodes lane by lane:
//   * every predictor is mapped to an order-preserving float KEY once per cell, thresholds
//     to key space on the host, so that  x < split  <=>  key < tkey  EXACTLY:
//       float32/int16 planes: key = the value, tkey = smallest float >= split;
//       LONG: key = column index, tkey = #columns whose centre is < split (same double formula);
//       LAT : key = -row index,   tkey = 0.5 - (first row whose centre is < split);
//   * the keys are then replaced by their RANK among the model's sorted distinct tkeys of that
//     predictor (rank = #{tkeys <= key}, found once per cell by a coarse LDS + fine global binary
//     search), and a split on the j-th tkey carries c = j + 1:  key < tkey_j  <=>  rank <= j
//     <=>  clamp(c - rank, 0, 1) = 1.  Ranks are small integers, exact in float32, so a
//     predicate and its accumulation into the leaf index are two PACKED-f32 instructions for
//     two cells (v_pk_add_f32 with the clamp modifier, v_pk_fma_f32 acc = 2 acc + bit) instead
//     of compare + add-with-carry per cell: half the VALU issue slots of the kernel's hot loop;
//   * -rank is parked in LDS as [var][lane][4 cells] so one ds_read_b128 at a wave-uniform var
//     offset fetches the keys of the lane's 4 cells.  The accumulator starts at 2^(23-S) + t, so
//     after S doublings its bit pattern is 0x4B000000 + (t << S) + b: the tree's LUT slot, turned
//     into an LDS address by one shift-add; the leaf comes from the tree's 2^S-entry LUT (one
//     256-byte LDS row for S = 5, conflict-free).
// Cells with an NA covariate are skipped here and walked through their MissingNode
// children by tree_kernel<GBM, .., NA_ONLY> afterwards (gbm_pred's NA routing).

// bit[c] = clamp(c_q - rank[c], 0, 1) for the lane's 4 cells (k holds -rank); HI selects which
// dword of the SGPR pair {c_q, c_q+1} is broadcast to both halves of the packed add
template <bool HI>
__device__ __forceinline__ void pred_bits(float2v &b01, float2v &b23, const float2v k01, const float2v k23,
                                          const unsigned long long cpair) {
    if (!HI)
        asm("v_pk_add_f32 %0, %2, %4 op_sel_hi:[1,0] clamp\n\t"
            "v_pk_add_f32 %1, %3, %4 op_sel_hi:[1,0] clamp"
            : "=&v"(b01), "=&v"(b23) : "v"(k01), "v"(k23), "s"(cpair));
    else
        asm("v_pk_add_f32 %0, %2, %4 op_sel:[0,1] op_sel_hi:[1,1] clamp\n\t"
            "v_pk_add_f32 %1, %3, %4 op_sel:[0,1] op_sel_hi:[1,1] clamp"
            : "=&v"(b01), "=&v"(b23) : "v"(k01), "v"(k23), "s"(cpair));
}


template <int S>
__global__ __launch_bounds__(256) void gbm_lut_kernel(const double *__restrict__ lut,
                                                      const int *__restrict__ meta,
                                                      const void *__restrict__ sorted, int key64,
                                                      const int *__restrict__ sorted_off, int n_trees_padded,
                                                      double init_f, int p, StackDev s, PredGeom g,
                                                      double weight, int accumulate,
                                                      double *__restrict__ out) {
    static_assert((LUT_CHUNK << S) * sizeof(double) >= LUT_COARSE * sizeof(float), "coarse table must fit");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *keys = (float *)smem;                                              // [p][256][4]
    double *slut = (double *)(smem + (size_t)p * 256 * LUT_R * sizeof(float));  // [LUT_CHUNK << S]
    float *coarse = (float *)slut;
    const int64_t total = (int64_t)g.nr * g.nc;
    const int64_t quarter = (total + LUT_R - 1) / LUT_R;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int row[LUT_R], col[LUT_R];
    bool na[LUT_R];
    double acc[LUT_R];
#pragma unroll
    for (int c = 0; c < LUT_R; ++c) {
        int64_t i = i0 + c * quarter;
        if (i >= total) i = total - 1;
        row[c] = (int)(i / g.nc); col[c] = (int)(i - (int64_t)row[c] * g.nc);
        na[c] = false; acc[c] = 0.0;
    }
    // keys -> ranks among the predictor's sorted distinct tkeys
    for (int j = 0; j < p; ++j) {
        float r[LUT_R];
        lut_ranks<LUT_R, 256>(j, sorted, key64, sorted_off, coarse, s, g, row, col, na, r);
#pragma unroll
        for (int c = 0; c < LUT_R; ++c) keys[(j * 256 + threadIdx.x) * LUT_R + c] = -r[c];
    }
    const char *kbase = (const char *)(keys + threadIdx.x * LUT_R);
    constexpr unsigned A0_BITS = (unsigned)(127 + 23 - S) << 23;   // float 2^(23-S)
    // byte offset of LUT slot 0 minus 8 * 0x4B000000 (mod 2^32), kept opaque so that slot -> address
    // stays one v_lshl_add_u32
    unsigned lut_base = (unsigned)p * 256u * LUT_R * (unsigned)sizeof(float) - 0x58000000u;
    asm volatile("" : "+s"(lut_base));
    for (int t0 = 0; t0 < n_trees_padded; t0 += LUT_CHUNK) {
        __syncthreads();
        for (int e = threadIdx.x; e < (LUT_CHUNK << S); e += 256) slut[e] = lut[((int64_t)t0 << S) + e];
        __syncthreads();
#pragma unroll 2
        for (int t = 0; t < LUT_CHUNK; ++t) {
            const int *m = meta + (int64_t)(t0 + t) * LUT_META_DW;
            const unsigned long long *mc = (const unsigned long long *)m;
            const unsigned long long a0 = A0_BITS + ((unsigned)t << S);      // float 2^(23-S) + t
            float2v a01, a23, b01, b23;
            {
                const float4 k = *(const float4 *)(kbase + m[6]);
                pred_bits<false>(b01, b23, float2v{k.x, k.y}, float2v{k.z, k.w}, mc[0]);
                asm("v_pk_fma_f32 %0, %2, 2.0, %3 op_sel_hi:[0,0,1]\n\t"
                    "v_pk_fma_f32 %1, %2, 2.0, %4 op_sel_hi:[0,0,1]"
                    : "=&v"(a01), "=&v"(a23) : "s"(a0), "v"(b01), "v"(b23));
            }
#pragma unroll
            for (int q = 1; q < S; ++q) {
                const float4 k = *(const float4 *)(kbase + m[6 + q]);
                if (q & 1) pred_bits<true>(b01, b23, float2v{k.x, k.y}, float2v{k.z, k.w}, mc[q >> 1]);
                else pred_bits<false>(b01, b23, float2v{k.x, k.y}, float2v{k.z, k.w}, mc[q >> 1]);
                asm("v_pk_fma_f32 %0, %0, 2.0, %2 op_sel_hi:[1,0,1]\n\t"
                    "v_pk_fma_f32 %1, %1, 2.0, %3 op_sel_hi:[1,0,1]"
                    : "+v"(a01), "+v"(a23) : "v"(b01), "v"(b23));
            }
            acc[0] = acc[0] + *(const double *)(smem + (__float_as_uint(a01.x) * 8u + lut_base));
            acc[1] = acc[1] + *(const double *)(smem + (__float_as_uint(a01.y) * 8u + lut_base));
            acc[2] = acc[2] + *(const double *)(smem + (__float_as_uint(a23.x) * 8u + lut_base));
            acc[3] = acc[3] + *(const double *)(smem + (__float_as_uint(a23.y) * 8u + lut_base));
        }
    }
#pragma unroll
    for (int c = 0; c < LUT_R; ++c) {
        const int64_t i = i0 + c * quarter;
        if (i0 < quarter && i < total && !na[c])
            emit(out, (int64_t)row[c] * g.ld_out + col[c], init_f + acc[c], weight, accumulate);
    }
}

// Same evaluation with the -rank keys held in 32 VGPRs (v[64:95] = [8 predictors][4 cells]) instead
// of LDS, for models with <= 8 predictors: a level's predictor is selected with the VGPR index
// mode (s_set_gpr_idx_on / _idx add the wave-uniform register offset in M0 to src0 of the packed
// adds), so a level costs no LDS read and no address arithmetic -- 28 VALU per tree and 4 cells
// (20 packed predicate ops, 4 shift-adds, 4 fp64 adds).  Inside the indexed region every VALU
// instruction keeps a constant in src0 except the two that are meant to be indexed.
typedef float float32v __attribute__((ext_vector_type(32)));
constexpr int LUT_REG_P = 8;

#define MHS_LUT_LEVEL(IDX, CP, SEL)                                                   \
    "s_set_gpr_idx_idx %[" IDX "]\n\t"                                               \
    "v_pk_add_f32 %[b01], v[64:65], %[" CP "] " SEL " clamp\n\t"                     \
    "v_pk_add_f32 %[b23], v[66:67], %[" CP "] " SEL " clamp\n\t"                     \
    "v_pk_fma_f32 %[a01], 2.0, %[a01], %[b01] op_sel_hi:[0,1,1]\n\t"                 \
    "v_pk_fma_f32 %[a23], 2.0, %[a23], %[b23] op_sel_hi:[0,1,1]\n\t"
#define MHS_SEL_LO "op_sel_hi:[1,0]"
#define MHS_SEL_HI "op_sel:[0,1] op_sel_hi:[1,1]"

template <int S>
__device__ __forceinline__ void lut_tree_reg(float2v &a01, float2v &a23, const float32v &keys, const int *m,
                                             const unsigned long long a0) {
    const unsigned long long *mc = (const unsigned long long *)m;
    const unsigned long long c01 = mc[0], c23 = mc[1], c45 = mc[2];
    const int i0 = m[6] >> 10, i1 = m[7] >> 10, i2 = m[8] >> 10, i3 = m[9] >> 10, i4 = m[10] >> 10;
    float2v b01, b23;
    if (S == 5) {
        asm("s_set_gpr_idx_on %[i0], 0x1\n\t"
            "v_pk_add_f32 %[b01], v[64:65], %[c01] op_sel_hi:[1,0] clamp\n\t"
            "v_pk_add_f32 %[b23], v[66:67], %[c01] op_sel_hi:[1,0] clamp\n\t"
            "v_pk_fma_f32 %[a01], 2.0, %[a0], %[b01] op_sel_hi:[0,0,1]\n\t"
            "v_pk_fma_f32 %[a23], 2.0, %[a0], %[b23] op_sel_hi:[0,0,1]\n\t"
            MHS_LUT_LEVEL("i1", "c01", MHS_SEL_HI)
            MHS_LUT_LEVEL("i2", "c23", MHS_SEL_LO)
            MHS_LUT_LEVEL("i3", "c23", MHS_SEL_HI)
            MHS_LUT_LEVEL("i4", "c45", MHS_SEL_LO)
            "s_set_gpr_idx_off"
            : [a01] "=&v"(a01), [a23] "=&v"(a23), [b01] "=&v"(b01), [b23] "=&v"(b23)
            : "{v[64:95]}"(keys), [i0] "s"(i0), [i1] "s"(i1), [i2] "s"(i2), [i3] "s"(i3), [i4] "s"(i4),
              [c01] "s"(c01), [c23] "s"(c23), [c45] "s"(c45), [a0] "s"(a0));
    } else {
        const int i5 = m[11] >> 10;
        asm("s_set_gpr_idx_on %[i0], 0x1\n\t"
            "v_pk_add_f32 %[b01], v[64:65], %[c01] op_sel_hi:[1,0] clamp\n\t"
            "v_pk_add_f32 %[b23], v[66:67], %[c01] op_sel_hi:[1,0] clamp\n\t"
            "v_pk_fma_f32 %[a01], 2.0, %[a0], %[b01] op_sel_hi:[0,0,1]\n\t"
            "v_pk_fma_f32 %[a23], 2.0, %[a0], %[b23] op_sel_hi:[0,0,1]\n\t"
            MHS_LUT_LEVEL("i1", "c01", MHS_SEL_HI)
            MHS_LUT_LEVEL("i2", "c23", MHS_SEL_LO)
            MHS_LUT_LEVEL("i3", "c23", MHS_SEL_HI)
            MHS_LUT_LEVEL("i4", "c45", MHS_SEL_LO)
            MHS_LUT_LEVEL("i5", "c45", MHS_SEL_HI)
            "s_set_gpr_idx_off"
            : [a01] "=&v"(a01), [a23] "=&v"(a23), [b01] "=&v"(b01), [b23] "=&v"(b23)
            : "{v[64:95]}"(keys), [i0] "s"(i0), [i1] "s"(i1), [i2] "s"(i2), [i3] "s"(i3), [i4] "s"(i4), [i5] "s"(i5),
              [c01] "s"(c01), [c23] "s"(c23), [c45] "s"(c45), [a0] "s"(a0));
    }
}

// K64: float64 planes (rank search in double).  A separate instantiation, so that the float-key kernel -- the one the
// resident-float32 bench runs -- keeps its 96 registers without the double search's temporaries.
template <int S, bool K64>
__global__ __launch_bounds__(256, 5) void gbm_lutreg_kernel(const double *__restrict__ lut,
                                                         const int *__restrict__ meta,
                                                         const void *__restrict__ sorted, int key64,
                                                         const int *__restrict__ sorted_off, int n_trees_padded,
                                                         double init_f, int p, StackDev s, PredGeom g,
                                                         double weight, int accumulate,
                                                         double *__restrict__ out) {
    static_assert((LUT_CHUNK << S) * sizeof(double) >= LUT_COARSE * sizeof(float), "coarse table must fit");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *slut = (double *)smem;                                            // [LUT_CHUNK << S]
    float *coarse = (float *)smem;
    const int64_t total = (int64_t)g.nr * g.nc;
    const int64_t quarter = (total + LUT_R - 1) / LUT_R;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int row[LUT_R], col[LUT_R];
    bool na[LUT_R];
    double acc[LUT_R];
#pragma unroll
    for (int c = 0; c < LUT_R; ++c) {
        int64_t i = i0 + c * quarter;
        if (i >= total) i = total - 1;
        row[c] = (int)(i / g.nc); col[c] = (int)(i - (int64_t)row[c] * g.nc);
        na[c] = false; acc[c] = 0.0;
    }
    float32v keys;
#pragma unroll
    for (int j = 0; j < LUT_REG_P; ++j) {
        float r[LUT_R] = {0.f, 0.f, 0.f, 0.f};
        if (j < p) {
            if constexpr (K64) lut_ranks_t<LUT_R, 256, double>(j, (const double *)sorted, sorted_off, (double *)coarse, s, g, row, col, na, r);
            else lut_ranks_t<LUT_R, 256, float>(j, (const float *)sorted, sorted_off, coarse, s, g, row, col, na, r);
        }
#pragma unroll
        for (int c = 0; c < LUT_R; ++c) keys[j * LUT_R + c] = -r[c];
    }
    constexpr unsigned A0_BITS = (unsigned)(127 + 23 - S) << 23;   // float 2^(23-S)
    unsigned lut_base = 0u - 0x58000000u;                          // see gbm_lut_kernel
    asm volatile("" : "+s"(lut_base));
    for (int t0 = 0; t0 < n_trees_padded; t0 += LUT_CHUNK) {
        __syncthreads();
        for (int e = threadIdx.x; e < (LUT_CHUNK << S); e += 256) slut[e] = lut[((int64_t)t0 << S) + e];
        __syncthreads();
#pragma unroll 2
        for (int t = 0; t < LUT_CHUNK; ++t) {
            float2v a01, a23;
            lut_tree_reg<S>(a01, a23, keys, meta + (int64_t)(t0 + t) * LUT_META_DW, A0_BITS + ((unsigned)t << S));
            acc[0] = acc[0] + *(const double *)(smem + (__float_as_uint(a01.x) * 8u + lut_base));
            acc[1] = acc[1] + *(const double *)(smem + (__float_as_uint(a01.y) * 8u + lut_base));
            acc[2] = acc[2] + *(const double *)(smem + (__float_as_uint(a23.x) * 8u + lut_base));
            acc[3] = acc[3] + *(const double *)(smem + (__float_as_uint(a23.y) * 8u + lut_base));
        }
    }
#pragma unroll
    for (int c = 0; c < LUT_R; ++c) {
        const int64_t i = i0 + c * quarter;
        if (i0 < quarter && i < total && !na[c])
            emit(out, (int64_t)row[c] * g.ld_out + col[c], init_f + acc[c], weight, accumulate);
    }
}

// ROW-TILE form of the register kernel (round 3; S = 5, the reference's interaction depth, V73:493).  A wave owns 256
// consecutive cells of ONE raster row (lane l: columns tile + l + 64 c, c = 0..3), so every split on LAT -- a
// predictor of every model, V73:127-138 -- is WAVE-UNIFORM for all four cells of all 64 lanes, and so is every
// padding level of a tree with fewer than 5 splits (its predicate is 0).  The geometry-dependent tables order each
// tree's levels uniform-first (up to two of them; the leaf LUT is permuted to match, per tree): the K uniform
// predicates are evaluated on the SCALAR unit (compare + select on the row's LAT rank, which sits in an SGPR) and
// folded into the accumulator's start value, and only the NV = 5 - K per-cell levels run as packed vector
// instructions -- 4 NV + 8 VALU per tree and 4 cells instead of 28.  The tree loop branches on NV (wave-uniform, scalar
// branches); the 64-byte record of the next tree is fetched into SGPRs while this one is evaluated.  Same leaf values
// added in the same tree order as gbm_lutreg_kernel and the generic walk: bit-identical results.
// Record (16 dwords): c[5] float rank thresholds of the vector levels | NV | idx[5] VGPR offsets of their predictors |
// uthr[5] int rank thresholds of the uniform levels (0 = never: a padding level).
constexpr int LUT_RT_DW = 16;
constexpr int LUT_RT_MAXK = 2;          // more uniform levels than this run as vector levels (their keys exist too)
typedef unsigned long long u64x8 __attribute__((ext_vector_type(8)));   // one record

// Which kernel for this window: PROBE instantiation of gbm_coherent_kernel (below) = its classification alone, on 64 tiles spread
// over the window and the first 256 trees, summing what the cell loops would cost (in hundredths of what the tree-order
// kernel spends per tree and wave; measured, profiles/r03_gbm_coherent.txt: 12 fixed, 85 + 26 n for a tree with n >= 1
// straddling splits).  Both product kernels are then launched and read the four blocks' sums: the one that loses returns
// at once.  No host synchronisation; smooth rasters run the coherent kernel (4x faster), white noise the tree-order one.
constexpr int GBC_PROBE_BLOCKS = 4, GBC_PROBE_CHUNKS = 4, GBC_PROBE_SLOTS = 1024;
__device__ __forceinline__ bool gbc_coherent_pays(const int *__restrict__ probe) {
    long long cost = 0, cnt = 0;
#pragma unroll
    for (int b = 0; b < GBC_PROBE_BLOCKS; ++b) { cost += probe[2 * b]; cnt += probe[2 * b + 1]; }
    return cost < 83 * cnt;
}
template <bool K64>
__global__ __launch_bounds__(256, 5) void gbm_lutreg_rt_kernel(const double *__restrict__ lut,
                                                            const u64x8 *__restrict__ meta,
                                                            const void *__restrict__ sorted,
                                                            const int *__restrict__ sorted_off, int n_trees_padded,
                                                            double init_f, int p, StackDev s, PredGeom g, int tiles_per_row,
                                                            double weight, int accumulate,
                                                            double *__restrict__ out, const int *__restrict__ probe) {
    constexpr int S = 5;
    static_assert((LUT_CHUNK << S) * sizeof(double) >= LUT_COARSE * sizeof(float), "coarse table must fit");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (probe && gbc_coherent_pays(probe)) return;                            // gbm_coherent_kernel takes this window
    double *slut = (double *)smem;                                            // [LUT_CHUNK << S]
    float *coarse = (float *)smem;
    const int lane = threadIdx.x & 63;
    const int64_t ntiles = (int64_t)g.nr * tiles_per_row;
    int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = tile < ntiles;
    if (!live) tile = ntiles - 1;
    const int trow = (int)(tile / tiles_per_row), tcol = (int)(tile - (int64_t)trow * tiles_per_row) * (64 * LUT_R);
    int row[LUT_R], col[LUT_R];
    bool na[LUT_R], ok[LUT_R];
    double acc[LUT_R];
#pragma unroll
    for (int c = 0; c < LUT_R; ++c) {
        const int cc = tcol + c * 64 + lane;
        ok[c] = live && cc < g.nc;
        row[c] = trow; col[c] = min(cc, g.nc - 1);
        na[c] = false; acc[c] = 0.0;
    }
    float32v keys;
    int latv = 0;
#pragma unroll
    for (int j = 0; j < LUT_REG_P; ++j) {
        float r[LUT_R] = {0.f, 0.f, 0.f, 0.f};
        if (j < p) {
            if constexpr (K64) lut_ranks_t<LUT_R, 256, double>(j, (const double *)sorted, sorted_off, (double *)coarse, s, g, row, col, na, r);
            else lut_ranks_t<LUT_R, 256, float>(j, (const float *)sorted, sorted_off, coarse, s, g, row, col, na, r);
            if (j == s.C + 1) latv = (int)r[0];
        }
#pragma unroll
        for (int c = 0; c < LUT_R; ++c) keys[j * LUT_R + c] = -r[c];
    }
    const int latrank = __builtin_amdgcn_readfirstlane(latv);      // the wave's row: one rank for all its cells
    unsigned lut_base = 0u - 0x58000000u;                          // see gbm_lut_kernel
    asm volatile("" : "+s"(lut_base));
    for (int t0 = 0; t0 < n_trees_padded; t0 += LUT_CHUNK) {
        __syncthreads();
        for (int e = threadIdx.x; e < (LUT_CHUNK << S); e += 256) slut[e] = lut[((int64_t)t0 << S) + e];
        __syncthreads();
        // the chunk's 64 trees: hand-scheduled loop (tools/gen_gbm_rt_asm.py; the table carries one record past the end)
        const u64x8 *mp = meta + t0;
        asm volatile(
#include "gbm_rt_loop.inc"
            : [acc0] "+v"(acc[0]), [acc1] "+v"(acc[1]), [acc2] "+v"(acc[2]), [acc3] "+v"(acc[3])
            : "{v[64:95]}"(keys), [mp] "s"(mp), [lat] "s"(latrank), [lb] "s"(lut_base)
            : "memory", "scc",
              "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51",
              "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67",
              "s68", "s69", "s70", "s71", "s72", "s73", "s74",
              "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55",
              "v56", "v57", "v58", "v59");
    }
#pragma unroll
    for (int c = 0; c < LUT_R; ++c)
        if (ok[c] && !na[c]) emit(out, (int64_t)row[c] * g.ld_out + col[c], init_f + acc[c], weight, accumulate);
}


// COHERENT form of the gbm evaluation (round 3; S = 5).  Neighbouring cells have neighbouring covariates, and a split is a
// threshold: over the 64 x 4 cells of a wave's tile most splits of most trees have the SAME outcome for
// every cell (cfg3's synthetic rasters: 67 % of the trees have no split at all whose threshold lies inside the wave's range
// of that predictor, and the others 1.2 such splits on average).  So, per wave and chunk of 64 trees, with LANE = TREE:
//   * from the wave's [min, max] rank of every predictor (one reduction at the start) each lane classifies the five splits
//     of its tree: all cells left, all cells right, or straddling;
//   * no straddling split: the tree's leaf is the same for all the wave's cells -- the lane adds it to ITS sum of such
//     leaves (the 64 sums are added at the very end and go to every cell);
//   * one straddling split (predictor v, rank threshold c): the cells take one of two leaves, B (bit 0) or A (bit 1); the
//     lane adds B to its sum and queues (v, c, A - B) in a wave-private list; then the wave runs down the list with
//     LANE = CELL: acc += rank_v < c ? A - B : 0 -- one compare, two selects and one fp64 add per cell;
//   * two or more: the tree is queued for the full five-level evaluation (lane = cell, class words broadcast from LDS).
// The same leaves reach every cell's sum; their ORDER differs from the other gbm kernels' (tree order), and A enters as
// B + (A - B): planes agree to ~1e-15 of the prediction, not bitwise.  Incoherent rasters (every tree straddling several
// times) fall to the last case for every tree, which is slower than gbm_lutreg_rt_kernel: launch_gbm_lut samples the
// grid first and takes this kernel only where it pays.
// Block = 16 waves; the chunk's leaf LUT (16 KB) and class words (1.25 KB) are staged in LDS for all of them, double-buffered.
// Class word of level q of tree t (lut_cls, private to this kernel): rank threshold << 3 | predictor, 0 for a padding level;
// thresholds stay below 2^20 (build_lut_meta_t publishes no class words otherwise and the model keeps off this kernel).
// The lane = tree code keeps per lane the 5-bit mask of the straddling levels, their count, the leaf index of the others
// (`known`), B, and for one or two straddling levels the scaled leaf differences plus the one or two class words, which it
// re-reads from LDS at the level the mask's leading bit names and repacks as (threshold as a float's bits | predictor).  The
// cell loops fetch that word with one v_readlane and split it on the scalar unit; the three-or-more loop reads the tree's mask
// and walks its set bits with scalar branches, one v_readlane of the level's word each.  There are no per-lane lists of
// (threshold, predictor, bit position) any more: they cost every lane 27 to ~100 vector instructions per chunk whenever one
// lane of the wave had a straddling level (profiles/gbm_coherent_classify.txt).
constexpr int GBC_WAVES = 16;
__device__ __forceinline__ double gbc_lds_f64(unsigned a) { return *(__attribute__((address_space(3))) const double *)(uintptr_t)a; }
typedef float float4v __attribute__((ext_vector_type(4)));
template <bool K64, bool PROBE = false>
__global__ __launch_bounds__(1024) void gbm_coherent_kernel(const double *__restrict__ lut, const unsigned *__restrict__ cls,
                                                            const void *__restrict__ sorted, const int *__restrict__ sorted_off,
                                                            int n_trees_padded, double init_f, int p, StackDev s, PredGeom g,
                                                            int tiles_per_row, double weight, int accumulate,
                                                            double *__restrict__ out, int *__restrict__ probe, int tile16,
                                                            const int *__restrict__ axis_rank, int axis_ncol) {
    constexpr int S = 5, CH = LUT_CHUNK, CLS_STRIDE = 384, R = LUT_R;
    if (!PROBE && probe && !gbc_coherent_pays(probe)) return;
    if (PROBE) n_trees_padded = min(n_trees_padded, GBC_PROBE_CHUNKS * CH);
    static_assert(R == 4, "four cells per lane: two packed predicate instructions");
    static_assert((CH << S) * sizeof(double) >= LUT_COARSE * sizeof(float), "coarse table must fit");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *slut = (double *)smem;                                             // 2 x [CH << S], from LDS address 0
    unsigned *scls = (unsigned *)(smem + 2 * (CH << S) * sizeof(double));      // 2 x CLS_STRIDE
    int2 *srange = (int2 *)(scls + 2 * CLS_STRIDE);                            // [waves][8] (min, max) rank
    float *coarse = (float *)smem;
    if ((unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)smem != 0u) __builtin_trap();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // a wave = 64 columns x R adjacent rows (lane = column, a lane's R cells one below the other): the most compact
    // footprint a wave can have, hence the narrowest rank ranges.  The tiles are anchored to the GRID (rows at multiples of
    // R, columns at multiples of 64 of the grid, clipped by the window), so that a cell meets the same companions -- and
    // its sum the same order -- whether the window is evaluated whole or in row bands cut at multiples of R
    // Round 4 (tile16): 16 columns x 4 R rows per wave (lane = column + 16 x row group, a lane's R cells one below the other)
    // instead of 64 columns x R rows -- the forest's tile (rf_walk_ld_kernel): narrower rank ranges on smooth rasters, more
    // trees without a straddling split.  Anchored to the grid at multiples of 16 rows and 16 columns (BAND_ALIGN = 16 rows).
    const int TW = tile16 ? 16 : 64, TH = tile16 ? 4 * R : R;
    const int roff = (int)(g.r0 % TH), coff = (int)(g.c0 % TW);
    const int64_t ntiles = (int64_t)((g.nr + roff + TH - 1) / TH) * tiles_per_row;
    int64_t tile = (int64_t)blockIdx.x * GBC_WAVES + wave;
    if (PROBE) tile = ntiles >= GBC_PROBE_BLOCKS * GBC_WAVES ? tile * (ntiles / (GBC_PROBE_BLOCKS * GBC_WAVES)) : tile % ntiles;
    const bool live = tile < ntiles;
    if (!live) tile = ntiles - 1;
    const int trow = (int)(tile / tiles_per_row) * TH - roff + (tile16 ? (lane >> 4) * R : 0);
    const int tcol = (int)(tile % tiles_per_row) * TW - coff + (tile16 ? (lane & 15) : lane);
    int row[R], col[R];
    bool na[R], ok[R];
    double acc[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int rr = trow + c, cc = tcol;
        ok[c] = live && cc >= 0 && cc < g.nc && rr >= 0 && rr < g.nr;
        row[c] = min(max(rr, 0), g.nr - 1); col[c] = min(max(cc, 0), g.nc - 1);
        na[c] = false; acc[c] = 0.0;
    }
    // MINUS the ranks (the packed predicate adds them to c), [predictor][cell] in 32 registers that the several-splits
    // loop addresses through the VGPR index mode, as gbm_lutreg_kernel does
    float32v keys;
#pragma unroll
    for (int j = 0; j < LUT_REG_P; ++j) {
        float r[R] = {0.f, 0.f, 0.f, 0.f};
        if (j < p) {
            if (axis_rank && j >= s.C && !s.all_from_planes) {      // LONG / LAT ranks by table (publish_axis_ranks)
#pragma unroll
                for (int c = 0; c < R; ++c)
                    r[c] = (float)(j == s.C ? axis_rank[g.c0 + col[c]] : axis_rank[(int64_t)axis_ncol + g.r0 + row[c]]);
            } else if constexpr (K64) lut_ranks_t<R, 1024, double>(j, (const double *)sorted, sorted_off, (double *)coarse, s, g, row, col, na, r);
            else lut_ranks_t<R, 1024, float>(j, (const float *)sorted, sorted_off, coarse, s, g, row, col, na, r);
        }
#pragma unroll
        for (int c = 0; c < R; ++c) keys[j * R + c] = -r[c];
        // the wave's rank range of predictor j, NA cells left out (they are walked separately)
        int mn = 0x7fffffff, mx = -1;
#pragma unroll
        for (int c = 0; c < R; ++c)
            if (!na[c]) { mn = min(mn, (int)r[c]); mx = max(mx, (int)r[c]); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o)); mx = max(mx, __shfl_xor(mx, o)); }
        if (lane == 0) srange[wave * 8 + j] = make_int2(mn, mx);
    }
    __syncthreads();                                               // the coarse table (it aliases the LUT buffers) is done with
    for (int e = tid; e < (CH << S); e += 1024) slut[e] = lut[e];
    if (tid < CH * S) scls[tid] = cls[tid];
    __syncthreads();
    double usum = 0.0;
    int pcost = 0;
    for (int t0 = 0, buf = 0; t0 < n_trees_padded; t0 += CH, buf ^= 1) {
        const bool more = t0 + CH < n_trees_padded;
        double pre0 = 0.0, pre1 = 0.0;
        unsigned prec = 0u;
        if (more) {
            const double *ln = lut + ((int64_t)(t0 + CH) << S);
            pre0 = ln[tid]; pre1 = ln[tid + 1024];
            if (tid < CH * S) prec = cls[(int64_t)(t0 + CH) * S + tid];
        }
        // ---- lane = tree: classify the five splits against the wave's rank ranges
        const unsigned *cw = scls + buf * CLS_STRIDE + lane * S;
        const double *L = slut + buf * (CH << S) + (lane << S);
        unsigned w[S];
        int2 mm[S];
#pragma unroll
        for (int q = 0; q < S; ++q) w[q] = cw[q];
#pragma unroll
        for (int q = 0; q < S; ++q) mm[q] = srange[wave * 8 + (int)(w[q] & 7u)];
        // the straddling levels as a 5-bit mask (most significant bit = first level) and the other levels' outcomes as the
        // leaf index `known`: the whole price of a tree without a straddling split.  No list of the straddling levels is kept
        // per lane: what a straddling tree's cell loop needs is taken from its class words when the loop reaches the tree
        unsigned known = 0u, smask = 0u;
#pragma unroll
        for (int q = 0; q < S; ++q) {
            const int c = (int)(w[q] >> 3);
            const bool all1 = mm[q].y < c, all0 = mm[q].x >= c;
            if (all1) known |= 16u >> q;
            if (!(all1 || all0)) smask |= 16u >> q;
        }
        const unsigned nstr = (unsigned)__popc(smask);
        if (PROBE) {
            if (nstr) pcost += 85 + 26 * (int)nstr;
            if (more) {
                double *ld = slut + (buf ^ 1) * (CH << S);
                ld[tid] = pre0; ld[tid + 1024] = pre1;
                if (tid < CH * S) scls[(buf ^ 1) * CLS_STRIDE + tid] = prec;
            }
            __syncthreads();
            continue;
        }
        const double B = L[known];
        const bool single = nstr == 1u, pair = nstr == 2u, multi = nstr >= 3u;
        if (!multi) usum = usum + B;
        // One or two straddling splits: with b1, b2 their predicates the leaf is
        //     B + b1 (A1 - B) + b2 ((A2 - B) + b1 (A12 - A1 - A2 + B)),     A1, A2, A12 = the leaves with bit 1 / bit 2 / both set.
        // The cell loops below form a predicate as the float clamp(c - rank) written into the HIGH word of a register pair
        // whose low word is 0: read as a double that is 0 or 2^-7, so the differences are scaled by 2^7 (2^14) here -- exact.
        // f1, f2: the class words of the first and the second straddling level, re-read from LDS at the position that the
        // mask's leading bit gives (level q = bit 4 - q of the leaf index) and put into the cell loops' form: the threshold
        // as a float's bits | predictor (thresholds stay below 2^20, or build_lut_meta_t publishes no class words: the
        // float's low three bits are zero)
        double d1 = 0.0, d2 = 0.0, d12 = 0.0;
        unsigned f1 = 0u, f2 = 0u;
        if (single || pair) {
            const int pos1 = 31 - __clz((int)(smask | 1u));
            const unsigned p1 = 1u << pos1;
            f1 = cw[S - 1 - pos1];
            const double A1 = L[known + p1];
            d1 = (A1 - B) * 128.0;
            if (pair) {
                const int pos2 = 31 - __clz((int)((smask & ~p1) | 1u));
                const unsigned p2 = 1u << pos2;
                f2 = cw[S - 1 - pos2];
                const double A2 = L[known + p2], A12 = L[known + p1 + p2];
                d2 = (A2 - B) * 128.0;
                d12 = (((A12 - A1) - A2) + B) * 16384.0;
            }
            f1 = __float_as_uint((float)(int)(f1 >> 3)) | (f1 & 7u);
            f2 = __float_as_uint((float)(int)(f2 >> 3)) | (f2 & 7u);      // (a single's f2 is 0 and stays 0: no branch for it)
        }
        // ---- lane = cell.  What a tree needs sits in the registers of the lane that classified it and is fetched from
        // there with v_readlane (no list in LDS, no wait): one class word per straddling level, whose two fields come apart
        // on the scalar unit; the predictor's ranks are picked with the VGPR index mode.
#define MHS_GBC_RL(x) __builtin_amdgcn_readlane((int)(x), t)
#define MHS_GBC_RLD(x) __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), t), __builtin_amdgcn_readlane(__double2loint(x), t))
#define MHS_GBC_THR(fw) (int)((unsigned)(fw) & ~7u)
#define MHS_GBC_VO(fw) (int)(((unsigned)(fw) & 7u) << 2)
#define MHS_GBC_BITS(h0, h1, h2, h3, vo, cc)                                                                 \
        asm volatile("s_set_gpr_idx_on %[v], 0x1\n\t"                                                        \
                     "v_add_f32_e64 %[a], v64, %[c] clamp\n\t"                                               \
                     "v_add_f32_e64 %[b], v65, %[c] clamp\n\t"                                               \
                     "v_add_f32_e64 %[d], v66, %[c] clamp\n\t"                                               \
                     "v_add_f32_e64 %[e], v67, %[c] clamp\n\t"                                               \
                     "s_set_gpr_idx_off"                                                                     \
                     : [a] "=&v"(h0), [b] "=&v"(h1), [d] "=&v"(h2), [e] "=&v"(h3)                            \
                     : "{v[64:95]}"(keys), [v] "s"(vo), [c] "s"(cc));
        for (unsigned long long m1 = __builtin_amdgcn_ballot_w64(single); m1; m1 &= m1 - 1ull) {
            const int t = (int)__builtin_ctzll(m1);
            const int fw = MHS_GBC_RL(f1);
            const int cc = MHS_GBC_THR(fw), vo = MHS_GBC_VO(fw);
            const double e1 = MHS_GBC_RLD(d1);
            int h[R];
            MHS_GBC_BITS(h[0], h[1], h[2], h[3], vo, cc)
#pragma unroll
            for (int c = 0; c < R; ++c) acc[c] = fma(__hiloint2double(h[c], 0), e1, acc[c]);
        }
        for (unsigned long long mp = __builtin_amdgcn_ballot_w64(pair); mp; mp &= mp - 1ull) {
            const int t = (int)__builtin_ctzll(mp);
            const int fa = MHS_GBC_RL(f1), fb = MHS_GBC_RL(f2);
            const int c1 = MHS_GBC_THR(fa), v1 = MHS_GBC_VO(fa), c2 = MHS_GBC_THR(fb), v2 = MHS_GBC_VO(fb);
            const double e1 = MHS_GBC_RLD(d1), e2 = MHS_GBC_RLD(d2), e12 = MHS_GBC_RLD(d12);
            int h[R], k[R];
            MHS_GBC_BITS(h[0], h[1], h[2], h[3], v1, c1)
            MHS_GBC_BITS(k[0], k[1], k[2], k[3], v2, c2)
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const double b1 = __hiloint2double(h[c], 0), b2 = __hiloint2double(k[c], 0);
                acc[c] = fma(b1, e1, acc[c]);
                acc[c] = fma(b2, fma(b1, e12, e2), acc[c]);
            }
        }
#undef MHS_GBC_BITS
#undef MHS_GBC_RLD
        // Three or more: their straddling levels only (the others' bits are in `known`), each a packed predicate and a packed
        // multiply-add that drops the bit into the slot, which is kept as a float 2^23 + slot (its bit pattern is the LUT's
        // dword index plus a constant)
        const unsigned abase = (unsigned)buf * (unsigned)((CH << S) * sizeof(double)) - 0x58000000u;
        unsigned long long m2 = __builtin_amdgcn_ballot_w64(multi);
        // the five class words in the cell loops' form, repacked only in a chunk where some lane has three or more (the
        // copy before gives wf a defined value in the others, where the loop below does not run)
        unsigned wf[S];
#pragma unroll
        for (int q = 0; q < S; ++q) wf[q] = w[q];
        if (m2) {
#pragma unroll
            for (int q = 0; q < S; ++q) wf[q] = __float_as_uint((float)(int)(w[q] >> 3)) | (w[q] & 7u);
        }
        for (; m2; m2 &= m2 - 1ull) {
            const int t = (int)__builtin_ctzll(m2);
            const unsigned sm = (unsigned)MHS_GBC_RL(smask);
            const float a0 = __uint_as_float(0x4B000000u + ((unsigned)t << S) + (unsigned)MHS_GBC_RL(known));
            float2v s01 = {a0, a0}, s23 = {a0, a0};
#pragma unroll
            for (int q = 0; q < S; ++q) {
                if (sm & (16u >> q)) {                                  // (the slot is a sum of exact integers: any order)
                    const int fw = MHS_GBC_RL(wf[q]);
                    const unsigned long long cc = (unsigned)MHS_GBC_THR(fw);
                    const int vo = MHS_GBC_VO(fw);
                    const unsigned long long wb = (127u + (unsigned)(S - 1 - q)) << 23;
                    float2v b01, b23;
                    asm volatile("s_set_gpr_idx_on %[vo], 0x1\n\t"
                                 "v_pk_add_f32 %[b01], v[64:65], %[cc] op_sel_hi:[1,0] clamp\n\t"
                                 "v_pk_add_f32 %[b23], v[66:67], %[cc] op_sel_hi:[1,0] clamp\n\t"
                                 "s_set_gpr_idx_off\n\t"
                                 "v_pk_fma_f32 %[s01], %[b01], %[wb], %[s01] op_sel_hi:[1,0,1]\n\t"
                                 "v_pk_fma_f32 %[s23], %[b23], %[wb], %[s23] op_sel_hi:[1,0,1]"
                                 : [s01] "+v"(s01), [s23] "+v"(s23), [b01] "=&v"(b01), [b23] "=&v"(b23)
                                 : "{v[64:95]}"(keys), [vo] "s"(vo), [cc] "s"(cc), [wb] "s"(wb));
                }
            }
            acc[0] = acc[0] + gbc_lds_f64(__float_as_uint(s01.x) * 8u + abase);
            acc[1] = acc[1] + gbc_lds_f64(__float_as_uint(s01.y) * 8u + abase);
            acc[2] = acc[2] + gbc_lds_f64(__float_as_uint(s23.x) * 8u + abase);
            acc[3] = acc[3] + gbc_lds_f64(__float_as_uint(s23.y) * 8u + abase);
        }
#undef MHS_GBC_VO
#undef MHS_GBC_THR
#undef MHS_GBC_RL
        // ---- the next chunk into the other buffer
        if (more) {
            double *ld = slut + (buf ^ 1) * (CH << S);
            ld[tid] = pre0; ld[tid + 1024] = pre1;
            if (tid < CH * S) scls[(buf ^ 1) * CLS_STRIDE + tid] = prec;
        }
        __syncthreads();
    }
    if (PROBE) {
        int *tot = (int *)srange;                                   // the ranges are done with
        __syncthreads();
        if (tid == 0) tot[0] = 0;
        __syncthreads();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pcost += __shfl_xor(pcost, o);
        if (lane == 0) atomicAdd(tot, pcost);
        __syncthreads();
        if (tid == 0) { probe[2 * blockIdx.x] = tot[0]; probe[2 * blockIdx.x + 1] = GBC_WAVES * n_trees_padded; }
        return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) usum = usum + __shfl_xor(usum, o);
#pragma unroll
    for (int c = 0; c < R; ++c)
        if (ok[c] && !na[c]) emit(out, (int64_t)row[c] * g.ld_out + col[c], init_f + (acc[c] + usum), weight, accumulate);
}
static size_t gbc_lds_bytes() {
    return 2 * ((size_t)LUT_CHUNK << 5) * sizeof(double) + 2 * 384 * sizeof(unsigned) + GBC_WAVES * 8 * sizeof(int2);
}

// predict.gbm(model, newdata, n.trees = step, 2 step, ...) at a table of points: what machisplin.gbm.step evaluates on
// every fold's hold-out rows after every gbm.more (V73:1843, 1919) -- here in one walk over the trees, the running sum
// written out every `step` trees (same additions in the same order as a model cut at that tree count)
__global__ __launch_bounds__(256) void gbm_staged_points_kernel(const Node *__restrict__ nodes, const int *__restrict__ tree_off,
                                                                int n_trees, double init_f, const double *__restrict__ X,
                                                                int64_t n, int step, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int t = 0; t < n_trees; ++t) {
        const int tb = tree_off[t];
        Node nd = nodes[tb];
        while (nd.var >= 0) {
            const double xv = X[(int64_t)nd.var * n + i];
            const unsigned nxt = isnan(xv) ? nd.missing : (xv < nd.val ? nd.left : nd.right);
            nd = nodes[tb + nxt];
        }
        acc = acc + nd.val;
        if ((t + 1) % step == 0) out[(int64_t)((t + 1) / step - 1) * n + i] = init_f + acc;
    }
}

// res.FINAL at the stations (V73:477-482 ... 608-611, 620): ((resp - pred_1) w_1 + (resp - pred_2) w_2 + ...) / wt.tot,
// member after member as the reference accumulates it
struct ResidualArgs { double w[8]; };
__global__ __launch_bounds__(256) void residual_points_kernel(const double *__restrict__ pred, const double *__restrict__ resp,
                                                              int64_t n, int n_models, ResidualArgs a, double wt_total,
                                                              double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double y = resp[i];
    double res = (y - pred[i]) * a.w[0];
    for (int k = 1; k < n_models; ++k) res = res + (y - pred[(int64_t)k * n + i]) * a.w[k];
    out[i] = res / wt_total;
}

__global__ __launch_bounds__(256) void scale_add_kernel(const double *__restrict__ a, double divisor,
                                                        const double *__restrict__ b,
                                                        double *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = a[i] / divisor;
    if (b) v = v + b[i];
    out[i] = v;
}

__global__ __launch_bounds__(256) void scale_window_kernel(double *__restrict__ out, int nr, int nc,
                                                           int64_t ld, double divisor) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)nr * nc) return;
    const int row = (int)(i / nc), col = (int)(i - (int64_t)row * nc);
    out[(int64_t)row * ld + col] = out[(int64_t)row * ld + col] / divisor;
}

// ------------------------------------------------------ launchers (host side) --

template <int P>
static void launch_nnet(const mhs_model *m, const StackDev &s, const PredGeom &g, double w, int acc,
                        double *out, hipStream_t st, unsigned blocks) {
    hipLaunchKernelGGL((nnet_kernel<P>), dim3(blocks), dim3(256), 0, st, m->dpar, m->n0, m->s0, m->s1, s, g, w, acc, out);
}
// The form of the row-tile kernel by P (figures: profiles/ksvm_resident_waves.txt, profiles/ksvm_exp_insertion.txt).
// P <= 5: table_exp_neg_acc_rt with its 64 KB table and RESIDENT waves that pull their tiles (svr_rt_resident_kernel), in ONE
// block of 16 waves per CU -- 126 / 116 / 128 VGPRs at P = 3 / 4 / 5 in the built object, no scratch, four waves per SIMD.
// With one tile per wave a CU took a new block only when the block's slowest wave was through, and one block of 16 was 23 %
// slower than two of 8; with resident waves no wave waits for a block-mate, the block's shape is free, and one block per CU
// stages the table once instead of twice: a cfg3 step takes 230.1 ms with the one-tile form in 2 x 8 and 224.3 resident in 1 x 16
// (resident in 2 x 8: 4.4 ms more than in 1 x 16).  Short tiles at row ends were measured on top and not kept (-0.7 ms, within noise).
// P = 5: the support-vector loop of a chunk is the hand-scheduled block of svr_rt_loop5*.inc (two table reads in flight,
// counted waits, the records double-buffered in scalar registers; profiles/ksvm_pair_schedule.txt); P = 3, 4 keep the
// compiler's loop, which MHS_SVR_CXX_LOOP selects at P = 5 as well (the same planes, bit for bit).
// Larger P keep the one-tile kernel with table_exp_neg_acc, the 32 KB table and blocks of 4 waves, as before.  P = 7 resident
// with the 64 KB table in one block of 12 was TIMED at cfg5 (3 087 -> 2 898 ms per step) but its planes were never checked
// on a device, so it is not used; P = 6 and P = 8 .. 12 were measured in no form.
constexpr bool svr_rt_tab2(int P) { return P <= 5; }       // and with it resident waves
constexpr int svr_rt_waves_per_simd(int P) { return P <= 5 ? 4 : 3; }   // what the resident form is compiled for (its register budget)
constexpr int svr_rt_waves(int P) { return svr_rt_tab2(P) ? 16 : 4; }
constexpr bool svr_rt_hand(int P) { return P == 5; }       // the hand-scheduled support-vector loop (svr_rt_loop5*.inc); P = 3, 4 keep the compiler's

// The tile counter of one resident launch.  A slot's ring holds SVR_POOL_SLOTS counters; a launch takes the next one, zeroes
// it on its OWN stream ahead of the kernel and records the slot's event behind the kernel.  The launch that takes the same
// counter SVR_POOL_SLOTS launches later first makes its stream wait for that event (a device-side wait; for an event that
// has fired or was never recorded, nothing), so no two launches in flight -- on whatever streams of the slot -- ever count
// in the same word, and the host never waits.  svr_pool_mu is held from the take to the record: host threads that launch
// on one slot pass through one at a time.
static std::mutex svr_pool_mu[MAX_SLOTS];
static int svr_pool_take(Context &c, hipStream_t st, int *idx, unsigned long long **counter) {
    if (!c.svr_pool) {      // the events first: the ring counts as made only when all of it is
        for (hipEvent_t &e : c.svr_pool_ev)
            if (!e) MHS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        MHS_HIP(hipMalloc((void **)&c.svr_pool, sizeof(unsigned long long) * SVR_POOL_SLOTS));
    }
    *idx = (int)(c.svr_pool_next++ % SVR_POOL_SLOTS);
    *counter = c.svr_pool + *idx;
    MHS_HIP(hipStreamWaitEvent(st, c.svr_pool_ev[*idx], 0));
    MHS_HIP(hipMemsetAsync(*counter, 0, sizeof(unsigned long long), st));
    return MHS_OK;
}

template <int P>
static int launch_svr(const mhs_model *m, const StackDev &s, const PredGeom &g, double w, int acc,
                      double *out, hipStream_t st, int64_t total) {
    constexpr int R = 3;      // cells per lane (2: 83.5, 3: 81.0, 4: 82.4 ms on 8000^2 cells x 3000 SVs)
    // grid mode with long rows: a wave = 192 cells of one row, the LAT term of the exponent once per wave (svr_rt_kernel)
    const int tpr = (g.nc + 64 * R - 1) / (64 * R);
    if (!s.all_from_planes && P == s.C + 2 && P >= 3 && !getenv("MHS_SVR_NO_ROWTILE") && (double)g.nc >= 0.93 * (double)tpr * (64 * R)) {
        const int64_t ntiles = (int64_t)g.nr * tpr;
        constexpr int NW = svr_rt_waves(P);
        const int64_t covering = (ntiles + NW - 1) / NW;       // blocks whose waves cover the tiles one each
        if constexpr (svr_rt_tab2(P)) {
            // MHS_SVR_CXX_LOOP: the compiler's support-vector loop where the hand-scheduled one is the default (the same planes)
            const bool hand = svr_rt_hand(P) && !getenv("MHS_SVR_CXX_LOOP");
            auto kern = svr_rt_resident_kernel<P, R, NW, true, svr_rt_waves_per_simd(P), false>;
            if constexpr (svr_rt_hand(P))
                if (hand) kern = svr_rt_resident_kernel<P, R, NW, true, svr_rt_waves_per_simd(P), true>;
            Context &c = ctx();
            std::lock_guard<std::mutex> lk(svr_pool_mu[current_slot()]);
            int &per_cu = c.svr_rt_blocks_per_cu[hand ? 0 : P];   // blocks of this form a compute unit holds (index 0: the hand loop, P = 5 only); the slot's own, under its mutex
            if (per_cu == 0) {
                int n = 0;
                MHS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kern, 64 * NW, 0));
                per_cu = std::max(1, n);
            }
            const int64_t resident = (int64_t)(c.n_cu > 0 ? c.n_cu : 256) * per_cu;
            int idx = 0;
            unsigned long long *counter = nullptr;
            if (int rc = svr_pool_take(c, st, &idx, &counter)) return rc;
            const SvrRtScalars sc = {m->n0, m->n1, m->n2, tpr, m->s1, m->s0, m->s4, m->s2, m->s3, s, g, w, acc};
            hipLaunchKernelGGL(kern, dim3((unsigned)std::min(resident, covering)), dim3(64 * NW), 0, st,
                               m->dpar, m->dpar + (size_t)m->n0 * m->n1, c.exp_tab, out, counter, sc);
            MHS_HIP(hipEventRecord(c.svr_pool_ev[idx], st));
            return MHS_OK;
        }
        else {
            hipLaunchKernelGGL((svr_rt_kernel<P, R, NW, false>), dim3((unsigned)covering), dim3(64 * NW), 0, st,
                               m->dpar, m->n0, m->n1, m->n2, m->dpar + (size_t)m->n0 * m->n1, ctx().exp_tab, m->s1, m->s0, m->s4,
                               m->s2, m->s3, s, g, tpr, w, acc, out);
            return MHS_OK;
        }
    }
    const int64_t half = (total + R - 1) / R;
    hipLaunchKernelGGL((svr_kernel<P, R>), dim3((unsigned)((half + 255) / 256)), dim3(256), 0, st,
                       m->dpar, m->n0, m->n1, m->n2, m->dpar + (size_t)m->n0 * m->n1, ctx().exp_tab, m->s1, m->s0, m->s4,
                       m->s2, m->s3,
                       s, g, w, acc, out);
    return MHS_OK;
}

#define MHS_DISPATCH_P(P_, CALL)                                                     \
    switch (P_) {                                                                    \
        case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;      \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break;      \
        case 8: CALL(8); break; case 9: CALL(9); break; case 10: CALL(10); break;    \
        case 11: CALL(11); break; case 12: CALL(12); break;                          \
        default: set_error("predict: p = %d exceeds the %d predictors this build supports for nnet/ksvm", P_, PMAX); \
                 return MHS_ERR_INVALID;                                             \
    }

template <bool GBM>
__global__ __launch_bounds__(256) void tree_finalize_kernel(const double *__restrict__ part, int shares, int64_t total,
                                                            double init_f, int n_trees, PredGeom g, double weight,
                                                            int accumulate, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double acc = 0.0;
    for (int y = 0; y < shares; ++y) acc = acc + part[(int64_t)y * total + i];
    const int row = (int)(i / g.nc), col = (int)(i - (int64_t)row * g.nc);
    emit(out, (int64_t)row * g.ld_out + col, GBM ? init_f + acc : acc / (double)n_trees, weight, accumulate);
}

constexpr int64_t TREE_SPLIT_MAX_CELLS = 16384;   // below this the tree loop is shared out over blockIdx.y
constexpr int TREE_SPLIT_SHARES = 64;

// A tree kernel in its two forms -- node records staged chunk-wise in LDS (`lds_kern`), or read from global memory where a
// tree does not fit (`global_kern`, !m->lds_ok) -- with the dynamic LDS the chosen one needs: xs_bytes of parked predictors,
// and a chunk of node records behind them for the first form.
template <typename K, typename... Args>
static int launch_tree_kernel(const mhs_model *m, K lds_kern, K global_kern, dim3 blocks, size_t xs_bytes, hipStream_t st, Args... args) {
    const K kern = m->lds_ok ? lds_kern : global_kern;
    const size_t bytes = xs_bytes + (m->lds_ok ? (size_t)m->max_chunk_nodes * sizeof(Node) : 0);
    MHS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(kern, blocks, dim3(256), bytes, st, args...);
    return MHS_OK;
}

// the generic node walk; NA_ONLY: only the cells with an NA covariate, and with `na_gate` (launch_gbm_na's compacted list) only
// if its overflow word is set
template <bool GBM, bool NA_ONLY>
static int launch_trees(const mhs_model *m, const StackDev &s, const PredGeom &g, double w, int acc,
                        double *out, hipStream_t st, int64_t total, const unsigned *na_gate = nullptr) {
    const size_t xs_bytes = (size_t)m->p * TREE_R * 256 * sizeof(double);
    if (xs_bytes > LDS_MAX) {
        // p >= 41 (the loaders take up to 64): the predictors of two cells per lane do not fit LDS at all -- one cell per lane,
        // nodes from global memory (finish_trees has cleared lds_ok: its budget is this xs_bytes)
        const size_t xs1 = (size_t)m->p * 256 * sizeof(double);
        const auto kern = tree_kernel<GBM, false, 1, NA_ONLY>;
        MHS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)xs1));
        hipLaunchKernelGGL(kern, dim3((unsigned)((total + 255) / 256)), dim3(256), xs1, st, m->nodes, m->tree_off, m->chunks, m->n_chunks,
                           m->n_trees, m->init_f, m->p, s, g, w, acc, out, na_gate);
        return MHS_OK;
    }
    const int64_t half = (total + TREE_R - 1) / TREE_R;
    const unsigned blocks = (unsigned)((half + 255) / 256);
    if (!NA_ONLY && m->lds_ok && total <= TREE_SPLIT_MAX_CELLS && m->n_chunks >= 4) {
        const int shares = std::min(m->n_chunks, TREE_SPLIT_SHARES);
        mhs_model *mm = const_cast<mhs_model *>(m);
        if (!mm->split_scratch) MHS_HIP(hipMalloc((void **)&mm->split_scratch, sizeof(double) * TREE_SPLIT_MAX_CELLS * TREE_SPLIT_SHARES));
        auto kern = tree_kernel<GBM, true, TREE_R, false, true>;      // lds_ok holds: the shared-out walk has no global-nodes form
        if (int rc = launch_tree_kernel(m, kern, kern, dim3(blocks, (unsigned)shares), xs_bytes, st, m->nodes, m->tree_off, m->chunks,
                                        m->n_chunks, m->n_trees, m->init_f, m->p, s, g, w, acc, mm->split_scratch, (const unsigned *)nullptr))
            return rc;
        hipLaunchKernelGGL(tree_finalize_kernel<GBM>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           mm->split_scratch, shares, total, m->init_f, m->n_trees, g, w, acc, out);
        return MHS_OK;
    }
    return launch_tree_kernel(m, tree_kernel<GBM, true, TREE_R, NA_ONLY>, tree_kernel<GBM, false, TREE_R, NA_ONLY>, dim3(blocks), xs_bytes, st,
                              m->nodes, m->tree_off, m->chunks, m->n_chunks, m->n_trees, m->init_f, m->p, s, g, w, acc, out, na_gate);
}

// key-space thresholds of every split for this grid, the sorted distinct thresholds of each
// predictor and every split's rank among them (see gbm_lut_kernel); cached per geometry and key type
template <typename KT>
static int build_lut_meta_t(mhs_model *m, const mhs_grid &grid, int C) {
    const int S = m->lut_S;
    std::vector<KT> tkey((size_t)m->n_trees * S, (KT)0);
    std::vector<std::vector<KT>> sorted((size_t)m->p);
    for (int t = 0; t < m->n_trees; ++t) {
        for (int q = 0; q < S; ++q) {
            const int v = m->lut_var[(size_t)t * S + q];
            if (v < 0) continue;
            const KT tk = split_tkey<KT, false>(v, C, m->lut_thr[(size_t)t * S + q], grid);
            tkey[(size_t)t * S + q] = tk;
            sorted[(size_t)v].push_back(tk);
        }
    }
    std::vector<int> off;
    std::vector<KT> flat;
    sort_unique(sorted, off, flat);
    for (int v = 0; v < m->p; ++v)
        if (sorted[(size_t)v].size() >= ((size_t)1 << 24)) { set_error("gbm: too many distinct split values"); return MHS_ERR_INVALID; }
    if (int rc = publish_axis_ranks(m, sorted, C, grid)) return rc;
    std::vector<int> meta((size_t)m->n_trees_padded * LUT_META_DW, 0);
    const float never = -33554432.f;   // c - rank <= 0 for every rank: the padded predicates read 0
    for (int t = 0; t < m->n_trees_padded; ++t) {
        int *mt = &meta[(size_t)t * LUT_META_DW];
        for (int q = 0; q < 6; ++q) { memcpy(&mt[q], &never, 4); mt[6 + q] = 0; }
        if (t >= m->n_trees) continue;
        for (int q = 0; q < S; ++q) {
            const int v = m->lut_var[(size_t)t * S + q];
            if (v < 0) continue;
            const std::vector<KT> &sv = sorted[(size_t)v];
            const KT tk = tkey[(size_t)t * S + q];
            const float c = (float)((std::lower_bound(sv.begin(), sv.end(), tk) - sv.begin()) + 1);
            memcpy(&mt[q], &c, 4);
            mt[6 + q] = v * 256 * LUT_R * (int)sizeof(float);
        }
    }
    // row-tile tables (gbm_lutreg_rt_kernel, S = 5): per tree, up to LUT_RT_MAXK of the levels that are uniform along
    // a raster row -- splits on LAT (predictor C + 1) and padding levels -- first, the other levels after them, the leaf
    // LUT permuted to that order; one all-padding record past the last tree (the kernel fetches a tree ahead)
    if (m->p <= LUT_REG_P && S == 5 && !m->lut_host.empty()) {
        const int lat = C + 1 < m->p ? C + 1 : -2;
        std::vector<int> rmeta(((size_t)m->n_trees_padded + 1) * LUT_RT_DW, 0);
        std::vector<double> rlut(m->lut_host.size(), 0.0);
        for (int t = 0; t <= m->n_trees_padded; ++t) {
            int *mt = &rmeta[(size_t)t * LUT_RT_DW];
            for (int q = 0; q < 5; ++q) { memcpy(&mt[q], &never, 4); mt[6 + q] = 0; mt[11 + q] = 0; }
            mt[5] = S - LUT_RT_MAXK;            // padded trees: two uniform padding levels, three vector ones that read 0
            if (t >= m->n_trees) continue;
            int perm[6], K = 0, n = 0;
            bool first[6] = {false, false, false, false, false, false};
            for (int q = 0; q < S && K < LUT_RT_MAXK; ++q) {
                const int v = m->lut_var[(size_t)t * S + q];
                if (v < 0 || v == lat) { perm[n++] = q; first[q] = true; ++K; }
            }
            for (int q = 0; q < S; ++q) if (!first[q]) perm[n++] = q;
            for (int i = 0; i < S; ++i) {
                const int q = perm[i], v = m->lut_var[(size_t)t * S + q];
                if (v < 0) continue;            // padding: uthr 0 / c = never
                const std::vector<KT> &sv = sorted[(size_t)v];
                const int c = (int)(std::lower_bound(sv.begin(), sv.end(), tkey[(size_t)t * S + q]) - sv.begin()) + 1;
                if (i < K) mt[11 + i] = c;
                else { const float cf = (float)c; memcpy(&mt[i - K], &cf, 4); mt[6 + i - K] = v * LUT_R; }
            }
            mt[5] = S - K;
            for (int b = 0; b < (1 << S); ++b) {        // b: slot in the new order (level i <-> bit S-1-i)
                int bo = 0;
                for (int i = 0; i < S; ++i) bo |= ((b >> (S - 1 - i)) & 1) << (S - 1 - perm[i]);
                rlut[((size_t)t << S) + b] = m->lut_host[((size_t)t << S) + bo];
            }
        }
        if (int rc = publish(m, rlut, &m->lut_rt)) return rc;
        if (int rc = publish(m, rmeta, &m->lut_rt_meta)) return rc;
        // class words (gbm_coherent_kernel): level q of tree t = rank threshold << 3 | predictor, 0 for a padding level
        std::vector<unsigned> cw((size_t)m->n_trees_padded * 5, 0u);
        for (int t = 0; t < m->n_trees; ++t)
            for (int q = 0; q < S; ++q) {
                const int v = m->lut_var[(size_t)t * S + q];
                if (v < 0) continue;
                const std::vector<KT> &sv = sorted[(size_t)v];
                const unsigned c = (unsigned)(std::lower_bound(sv.begin(), sv.end(), tkey[(size_t)t * S + q]) - sv.begin()) + 1u;
                cw[(size_t)t * 5 + q] = (c << 3) | (unsigned)v;
            }
        bool fits = true;                 // the kernel packs a threshold as a float with the predictor in its low three bits
        for (int v = 0; v < m->p; ++v) fits = fits && sorted[(size_t)v].size() < ((size_t)1 << 20);
        if (fits) { if (int rc = publish(m, cw, &m->lut_cls)) return rc; }
        else if (m->lut_cls) { m->retired.push_back((void *)m->lut_cls); m->lut_cls = nullptr; }
    }
    if (int rc = publish(m, flat, (KT **)&m->lut_sorted)) return rc;
    if (int rc = publish(m, off, &m->lut_sorted_off)) return rc;
    return publish(m, meta, &m->lut_meta);
}

static int build_lut_meta(mhs_model *m, const mhs_grid &grid, int C, int key64, TreeTables *tt) {
    std::lock_guard<std::mutex> lk(m->mu);
    if (!(m->lut_meta && same_meta(m, grid, C, key64))) {
        if (int rc = key64 ? build_lut_meta_t<double>(m, grid, C) : build_lut_meta_t<float>(m, grid, C)) return rc;
        m->meta_grid = grid; m->meta_C = C; m->meta_key64 = key64;
    }
    *tt = TreeTables{m->lut_sorted, m->lut_sorted_off, m->lut_meta, nullptr, nullptr, m->lut_rt, m->lut_rt_meta, m->lut_cls, m->axis_rank, m->axis_ncol};
    return MHS_OK;
}

// the MissingNode walk of a window's NA cells behind a predicate-LUT kernel: compacted list, strided pass on overflow
static int launch_gbm_na(const mhs_model *m, const StackDev &s, const PredGeom &g, double w, int acc, double *out, hipStream_t st,
                         int64_t total) {
    if (total >= (1LL << 32)) return launch_trees<true, true>(m, s, g, w, acc, out, st, total);
    mhs_model *mm = const_cast<mhs_model *>(m);
    const unsigned slot = mm->na_next.fetch_add(1) % 4;
    const size_t want = (size_t)std::max<int64_t>(4096, total / 8);      // up to 12.5 % NA cells; beyond: the strided pass
    unsigned *list = nullptr;
    unsigned cap = 0;
    {
        // One model predicted from several streams or host threads (round-4 advisor finding): launch k + 4 reuses launch k's
        // buffer, so it first waits -- on the device -- for the event recorded behind launch k's last reader, whichever stream
        // that ran on; list / cap are read under the lock that guards their reallocation.
        std::lock_guard<std::mutex> lk(mm->mu);
        if (!mm->na_done[slot]) MHS_HIP(hipEventCreateWithFlags(&mm->na_done[slot], hipEventDisableTiming));
        else if (mm->na_stream[slot] != st) MHS_HIP(hipStreamWaitEvent(st, mm->na_done[slot], 0));
        if (mm->na_cap[slot] < want) {
            if (mm->na_list[slot]) {
                MHS_HIP(hipEventSynchronize(mm->na_done[slot]));
                MHS_HIP(hipStreamSynchronize(st));
                (void)hipFree(mm->na_list[slot]); mm->na_list[slot] = nullptr; mm->na_cap[slot] = 0;
            }
            MHS_HIP(hipMalloc((void **)&mm->na_list[slot], sizeof(unsigned) * (want + 2)));
            mm->na_cap[slot] = want;
        }
        list = mm->na_list[slot];
        cap = (unsigned)mm->na_cap[slot];
        mm->na_stream[slot] = st;
    }
    MHS_HIP(hipMemsetAsync(list, 0, 2 * sizeof(unsigned), st));
    hipLaunchKernelGGL(na_collect_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, s, g, cap, list);
    const unsigned lblocks = (unsigned)std::min<int64_t>(2048, (total / 8 + 255) / 256 + 1);
    if (int rc = launch_tree_kernel(m, gbm_na_list_kernel<true>, gbm_na_list_kernel<false>, dim3(lblocks), (size_t)m->p * 256 * sizeof(double), st,
                                    m->nodes, m->tree_off, m->chunks, m->n_chunks, m->init_f, m->p, s, g, w, acc, out, list, cap))
        return rc;
    // the strided NA-only pass, gated on the overflow word (its blocks return at once otherwise)
    if (int rc = launch_trees<true, true>(m, s, g, w, acc, out, st, total, list)) return rc;
    MHS_HIP(hipGetLastError());
    {
        std::lock_guard<std::mutex> lk(mm->mu);
        MHS_HIP(hipEventRecord(mm->na_done[slot], st));
    }
    return MHS_OK;
}

// the predicate-LUT kernels take gbm in grid mode when every tree has at most 6 splits (lut_S) and the keys of a block's cells
// fit in LDS beside a chunk of leaf tables; the rank search runs in float for float32 / int16 planes, in double for float64 ones
static bool gbm_lut_applies(const mhs_model *m, const StackDev &s, const mhs_grid *grid) {
    return grid && m->lut_S > 0 && !s.all_from_planes && !getenv("MHS_TREES_GENERIC") &&
           (size_t)m->p * 256 * LUT_R * 4 + ((size_t)LUT_CHUNK << m->lut_S) * 8 <= LDS_LIMIT;
}

static int launch_gbm_lut(const mhs_model *m, const StackDev &s, const PredGeom &g, const mhs_grid &grid,
                          double w, int acc, double *out, hipStream_t st, int64_t total) {
    const int key64 = s.dtype == MHS_F64;
    TreeTables tt;
    if (int rc = build_lut_meta(const_cast<mhs_model *>(m), grid, s.C, key64, &tt)) return rc;
    const int64_t quarter = (total + LUT_R - 1) / LUT_R;
    const unsigned blocks = (unsigned)((quarter + 255) / 256);
    const size_t lut_bytes = ((size_t)LUT_CHUNK << m->lut_S) * sizeof(double);
    const bool in_regs = m->p <= LUT_REG_P;
    // row-tile form: a wave = 256 consecutive cells of one row (LAT splits and padding levels on the scalar unit); taken
    // when the rows are long enough that the ragged last tile of a row wastes little
    const int tpr = (g.nc + 64 * LUT_R - 1) / (64 * LUT_R);
    const int ctw = 16, cth = 4 * LUT_R;                                   // the coherent kernel's 16 x 16-cell wave tiles
    const int ctpr = (int)((g.nc + g.c0 % ctw + ctw - 1) / ctw);
    const bool rt_ok = in_regs && m->lut_S == 5 && tt.lut_rt && (double)g.nc >= 0.93 * (double)tpr * (64 * LUT_R);
    const bool coh_ok = in_regs && m->lut_S == 5 && tt.lut_cls && g.nr >= 2 * LUT_R && (double)g.nc >= 0.8 * (double)ctpr * ctw &&
                        !getenv("MHS_GBM_NO_COHERENT");
    // Grids: the coherent kernel where neighbouring cells share their trees' outcomes, the tree-order row-tile kernel where
    // they do not (white-noise rasters) -- decided on the device by a probe of 64 tiles (large windows; small ones are not
    // worth two more launches and take the coherent kernel; MHS_GBM_FORCE_COHERENT: no probe)
    int *probe = nullptr;
    if (coh_ok && rt_ok && total >= (1 << 20) && !getenv("MHS_GBM_FORCE_COHERENT")) {
        mhs_model *mm = const_cast<mhs_model *>(m);
        {
            std::lock_guard<std::mutex> lk(mm->mu);
            if (!mm->gbm_probe) MHS_HIP(hipMalloc(&mm->gbm_probe, sizeof(int) * 2 * GBC_PROBE_BLOCKS * GBC_PROBE_SLOTS));
        }
        probe = mm->gbm_probe + (size_t)(mm->gbm_probe_next.fetch_add(1) % GBC_PROBE_SLOTS) * 2 * GBC_PROBE_BLOCKS;
    }
    if (coh_ok) {
        const int64_t ntiles = (int64_t)((g.nr + g.r0 % cth + cth - 1) / cth) * ctpr;
        const unsigned cblocks = (unsigned)((ntiles + GBC_WAVES - 1) / GBC_WAVES);
        if (probe) {
            auto pk = key64 ? gbm_coherent_kernel<true, true> : gbm_coherent_kernel<false, true>;
            MHS_HIP(hipFuncSetAttribute((const void *)pk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gbc_lds_bytes()));
            hipLaunchKernelGGL(pk, dim3(GBC_PROBE_BLOCKS), dim3(1024), gbc_lds_bytes(), st, m->lut, tt.lut_cls, tt.sorted, tt.sorted_off,
                               m->n_trees_padded, m->init_f, m->p, s, g, ctpr, w, acc, out, probe, 1, tt.axis_rank, tt.axis_ncol);
        }
        auto ck = key64 ? gbm_coherent_kernel<true> : gbm_coherent_kernel<false>;
        MHS_HIP(hipFuncSetAttribute((const void *)ck, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gbc_lds_bytes()));
        hipLaunchKernelGGL(ck, dim3(cblocks), dim3(1024), gbc_lds_bytes(), st, m->lut, tt.lut_cls, tt.sorted, tt.sorted_off,
                           m->n_trees_padded, m->init_f, m->p, s, g, ctpr, w, acc, out, probe, 1, tt.axis_rank, tt.axis_ncol);
        if (!probe) return launch_gbm_na(m, s, g, w, acc, out, st, total);
    }
    if (rt_ok) {
        const int64_t ntiles = (int64_t)g.nr * tpr;
        const unsigned rblocks = (unsigned)((ntiles + 3) / 4);
        auto rk = key64 ? gbm_lutreg_rt_kernel<true> : gbm_lutreg_rt_kernel<false>;
        MHS_HIP(hipFuncSetAttribute((const void *)rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lut_bytes));
        hipLaunchKernelGGL(rk, dim3(rblocks), dim3(256), lut_bytes, st, tt.lut_rt, (const u64x8 *)tt.lut_rt_meta, tt.sorted, tt.sorted_off,
                           m->n_trees_padded, m->init_f, m->p, s, g, tpr, w, acc, out, (const int *)probe);
        return launch_gbm_na(m, s, g, w, acc, out, st, total);
    }
    const size_t bytes = in_regs ? lut_bytes : (size_t)m->p * 256 * LUT_R * sizeof(float) + lut_bytes;
    auto kern = in_regs ? (m->lut_S == 5 ? (key64 ? gbm_lutreg_kernel<5, true> : gbm_lutreg_kernel<5, false>)
                                         : (key64 ? gbm_lutreg_kernel<6, true> : gbm_lutreg_kernel<6, false>))
                        : (m->lut_S == 5 ? gbm_lut_kernel<5> : gbm_lut_kernel<6>);
    MHS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), bytes, st, m->lut, tt.lut_meta, tt.sorted, key64, tt.sorted_off,
                       m->n_trees_padded, m->init_f, m->p, s, g, w, acc, out);
    // cells with an NA covariate: walked through their MissingNode children
    return launch_gbm_na(m, s, g, w, acc, out, st, total);
}


// out (+)= weight * pred of one member; grid = NULL: points mode (no kernel that needs the grid's tables)
static int launch_model(const mhs_model *m, const StackDev &s, const PredGeom &g, double weight,
                        int accumulate, double *out, hipStream_t st, const mhs_grid *grid = nullptr) {
    const int64_t total = (int64_t)g.nr * g.nc;
    if (total == 0) return MHS_OK;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    switch (m->kind) {
        case K_LM:
            hipLaunchKernelGGL(lm_kernel, dim3(blocks), dim3(256), 0, st, m->dpar, m->p, s, g, weight, accumulate, out);
            break;
        case K_NNET: {
#define CALL_NNET(P) launch_nnet<P>(m, s, g, weight, accumulate, out, st, blocks)
            MHS_DISPATCH_P(m->p, CALL_NNET)
#undef CALL_NNET
            break;
        }
        case K_EARTH:
            hipLaunchKernelGGL(earth_kernel, dim3(blocks), dim3(256), 0, st, m->dpar, m->dpar + m->n0,
                               m->ipar, m->ipar + m->n0 + 1, m->ipar + m->n0 + 1 + m->n1, m->n0, m->p, s, g,
                               weight, accumulate, out);
            break;
        case K_SVR: {
#define CALL_SVR(P) if (int rc = launch_svr<P>(m, s, g, weight, accumulate, out, st, total)) return rc
            MHS_DISPATCH_P(m->p, CALL_SVR)
#undef CALL_SVR
            break;
        }
        case K_GBM:
            if (gbm_lut_applies(m, s, grid)) {
                if (int rc = launch_gbm_lut(m, s, g, *grid, weight, accumulate, out, st, total)) return rc;
            } else if (int rc = launch_trees<true, false>(m, s, g, weight, accumulate, out, st, total)) return rc;
            break;
        case K_RF: {
            bool launched = false;
            if (int rc = launch_forest(m, s, g, grid, weight, accumulate, out, st, total, &launched)) return rc;
            if (!launched) if (int rc = launch_trees<false, false>(m, s, g, weight, accumulate, out, st, total)) return rc;
            break;
        }
        default:
            set_error("predict: unknown model kind %d", m->kind);
            return MHS_ERR_INVALID;
    }
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

template <int P>
static void launch_small(const SmallArgs &a, const StackDev &s, const PredGeom &g, int acc, double *out, hipStream_t st, unsigned blocks) {
    hipLaunchKernelGGL((small_members_kernel<P>), dim3(blocks), dim3(256), 0, st, a, s, g, acc, out);
}

// out (+)= sum_k w_k pred_k for the members in order (V73:471 ... 606); a run of two or three of (lm, nnet, earth) --
// consecutive in the reference's model order -- goes through one fused pass.
int launch_members(const mhs_model *const *models, const double *weights, int n_models, const StackDev &s,
                          const PredGeom &g, int accumulate_first, double *out, hipStream_t st, const mhs_grid *grid) {
    const int64_t total = (int64_t)g.nr * g.nc;
    int k = 0;
    bool masked_done = false;
    // which member leaves the compute units free: randomForest if present -- LDS-bound, one block per CU, it loses the
    // least (+13 %; gbm +26 %, ksvm +50 % measured) -- else ksvm, else gbm
    int mask_kind = -1;
    for (int want : {K_RF, K_SVR, K_GBM})
        for (int q = 0; q < n_models && mask_kind < 0; ++q)
            if (models[q]->kind == want) mask_kind = want;
    // (round 4, measured and not kept: a SMALL reservation held for the forest's and ksvm's 190 ms instead of a large one for the
    // forest's 70 -- the 32-column fit wants the whole chip for its MFMA updates: confined to 8 / 16 / 32 units it ends after
    // 486 / 336 / 259 ms of a cfg3 step, so the calibration of sharded.py now reserves nothing)
    while (k < n_models) {
        const int acc = (k > 0 || accumulate_first) ? 1 : 0;
        // the longest run lm? nnet? earth? starting at k (each at most once, in that order)
        int e = k;
        const mhs_model *lm = nullptr, *nn = nullptr, *ea = nullptr;
        if (total > 0 && models[k]->p <= PMAX) {
            if (e < n_models && models[e]->kind == K_LM) lm = models[e++];
            if (e < n_models && models[e]->kind == K_NNET && models[e]->p == models[k]->p) nn = models[e++];
            if (e < n_models && models[e]->kind == K_EARTH && models[e]->p == models[k]->p) ea = models[e++];
        }
        if (e - k >= 2) {
            SmallArgs a{};
            if (lm) { a.lm_coef = lm->dpar; a.w_lm = weights[k]; }
            if (nn) { a.nn_w = nn->dpar; a.nn_H = nn->n0; a.nn_scale = nn->s0; a.nn_shift = nn->s1; a.w_nn = weights[k + (lm ? 1 : 0)]; }
            if (ea) {
                a.ea_coef = ea->dpar; a.ea_cut = ea->dpar + ea->n0; a.ea_tstart = ea->ipar; a.ea_fvar = ea->ipar + ea->n0 + 1;
                a.ea_fdir = ea->ipar + ea->n0 + 1 + ea->n1; a.ea_nterms = ea->n0; a.w_ea = weights[e - 1];
            }
            const unsigned blocks = (unsigned)((total + 255) / 256);
            const int P_ = models[k]->p;
#define CALL_SMALL(P) launch_small<P>(a, s, g, acc, out, st, blocks)
            MHS_DISPATCH_P(P_, CALL_SMALL)
#undef CALL_SMALL
            MHS_HIP(hipGetLastError());
            k = e;
            continue;
        }
        // mhs_fit_reserve_cus: the chosen long member runs on the masked stream, fenced by two events so that it keeps
        // its place in the caller's stream order
        const int kind = models[k]->kind;
        if (!masked_done && ctx().reserved_cus > 0 && grid && total >= (1 << 22) && kind == mask_kind) {
            Context &c = ctx();
            std::lock_guard<std::mutex> lk(mask_mutex());
            if (c.masked_stream) {
                masked_done = true;
                MHS_HIP(hipEventRecord(c.mask_ev0, st));
                MHS_HIP(hipStreamWaitEvent(c.masked_stream, c.mask_ev0, 0));
                if (int rc = launch_model(models[k], s, g, weights[k], acc, out, c.masked_stream, grid)) return rc;
                MHS_HIP(hipEventRecord(c.mask_ev1, c.masked_stream));
                MHS_HIP(hipStreamWaitEvent(st, c.mask_ev1, 0));
                ++k;
                continue;
            }
        }
        if (int rc = launch_model(models[k], s, g, weights[k], acc, out, st, grid)) return rc;
        ++k;
    }
    return MHS_OK;
}

static int make_stack(const mhs_model *m, const mhs_grid *g, const mhs_stack *c, StackDev *s) {
    MHS_REQUIRE(c && c->data, "covariate stack is NULL");
    MHS_REQUIRE(c->n_layers == m->p - 2, "stack has the wrong number of layers for this model (p = layers + 2)");
    MHS_REQUIRE(c->dtype == MHS_F64 || c->dtype == MHS_F32 || c->dtype == MHS_I16, "bad stack dtype");
    MHS_REQUIRE(c->ld >= g->ncol && c->plane_stride >= c->ld * g->nrow, "stack strides smaller than the grid");
    *s = StackDev{c->data, c->n_layers, c->dtype, c->plane_stride, c->ld, c->nodata, !std::isnan(c->nodata), 0};
    return MHS_OK;
}

// Rows [r0, r1) of every covariate plane in a device buffer (plane k at buf + k * (r1 - r0) * ld elements), described with the
// PARENT grid's affine so that cell centres stay bit-identical: plane k, absolute row r lives at base + (k * plane_stride +
// r * ld) elements, so the base is shifted back by r0 rows and plane_stride skips only the rows that are there.
StackDev rows_stack(const void *buf, int64_t r0, int64_t r1, int n_layers, int dtype, int64_t ld, double nodata) {
    return StackDev{(const char *)buf - (size_t)r0 * ld * dtype_bytes(dtype), n_layers, dtype, (r1 - r0) * ld, ld, nodata, !std::isnan(nodata), 0};
}

// points mode: the n x p table X (a column per predictor, LONG and LAT among them) as p "planes" of one row
static void points_stack(const double *X_dev, int p, int64_t n, StackDev *s, PredGeom *pg) {
    *s = StackDev{X_dev, p, MHS_F64, n, n, NAN, 0, 1};
    *pg = PredGeom{0, 0, 1, 1, 0, 0, 1, (int)n, n};
}

// out = out / wt_total on an nr x nc window: the last step of pred.elev
int scale_window(double *out, int64_t nr, int64_t nc, int64_t ld, double wt_total, hipStream_t st) {
    if (nr * nc == 0) return MHS_OK;
    hipLaunchKernelGGL(scale_window_kernel, dim3((unsigned)((nr * nc + 255) / 256)), dim3(256), 0, st, out, (int)nr, (int)nc, ld, wt_total);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

int make_geom(const mhs_grid *g, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int64_t ld, PredGeom *pg) {
    MHS_REQUIRE(g && g->nrow > 0 && g->ncol > 0 && g->xres > 0 && g->yres > 0, "bad grid geometry");
    MHS_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= g->nrow && 0 <= c0 && c0 <= c1 && c1 <= g->ncol, "window outside the grid");
    MHS_REQUIRE(ld >= c1 - c0, "ld smaller than the window width");
    MHS_REQUIRE((r1 - r0) * (c1 - c0) < (1LL << 40) && r1 - r0 < (1LL << 31) && c1 - c0 < (1LL << 31), "window too large");
    pg->xmin = g->xmin; pg->ymax = g->ymax; pg->xres = g->xres; pg->yres = g->yres;
    pg->r0 = r0; pg->c0 = c0; pg->nr = (int)(r1 - r0); pg->nc = (int)(c1 - c0); pg->ld_out = ld;
    return MHS_OK;
}

// Members k of `models` on rows [b0, b1) of the grid from a device buffer that holds rows [buf_r0, buf_r1) of every covariate
// plane (plane k at buf + k * (buf_r1 - buf_r0) * ld elements): the device copy is described with the PARENT grid's affine,
// so cell centres -- and with them every member's value -- are those of the one-piece evaluation (multi.hip: one row band
// per device, evaluated in sub-bands while the rest of the band still travels).  `accumulate`: add to out_dev instead of
// starting it; `scale`: divide by wt_total afterwards (the last members of a cell).  out_dev = row b0's first cell.
int members_rows_dev(const mhs_model *const *models, const double *weights, int n_models, int accumulate, int scale, double wt_total,
                     const mhs_grid *g, const void *buf, int64_t buf_r0, int64_t buf_r1, int n_layers, int dtype, int64_t ld,
                     double nodata, int64_t b0, int64_t b1, double *out_dev, int64_t ld_out, hipStream_t st) {
    MHS_REQUIRE(models && weights && n_models >= 0 && g && buf && out_dev, "bad ensemble arguments");
    MHS_REQUIRE(wt_total != 0.0 && !std::isnan(wt_total), "wt_total must be non-zero");
    MHS_REQUIRE(dtype == MHS_F64 || dtype == MHS_F32 || dtype == MHS_I16, "bad stack dtype");
    MHS_REQUIRE(buf_r0 <= b0 && b0 <= b1 && b1 <= buf_r1, "rows outside the buffer");
    for (int k = 0; k < n_models; ++k)
        MHS_REQUIRE(models[k] && n_layers == models[k]->p - 2, "stack has the wrong number of layers for a model");
    if (b1 == b0) return MHS_OK;
    PredGeom pg;
    if (int rc = make_geom(g, b0, b1, 0, g->ncol, ld_out, &pg)) return rc;
    const StackDev sd = rows_stack(buf, buf_r0, buf_r1, n_layers, dtype, ld, nodata);
    if (n_models > 0) if (int rc = launch_members(models, weights, n_models, sd, pg, accumulate, out_dev, st, g)) return rc;
    return scale ? scale_window(out_dev, b1 - b0, g->ncol, ld_out, wt_total, st) : MHS_OK;
}

// pred.elev on rows [b0, b1) from a buffer that holds exactly those rows
int ensemble_band_dev(const mhs_model *const *models, const double *weights, int n_models, double wt_total, const mhs_grid *g,
                      const void *band_data, int n_layers, int dtype, int64_t ld, double nodata, int64_t b0, int64_t b1,
                      double *out_dev, int64_t ld_out, hipStream_t st) {
    MHS_REQUIRE(n_models >= 1, "bad ensemble arguments");
    return members_rows_dev(models, weights, n_models, 0, 1, wt_total, g, band_data, b0, b1, n_layers, dtype, ld, nodata, b0, b1, out_dev,
                            ld_out, st);
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_predict_dev(const mhs_model *m, const mhs_grid *g, const mhs_stack *covars, int64_t r0,
                    int64_t r1, int64_t c0, int64_t c1, double weight, int accumulate, double *out_dev,
                    int64_t ld, void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(m && out_dev, "NULL argument");
    PredGeom pg;
    StackDev s;
    if (int rc = make_geom(g, r0, r1, c0, c1, ld, &pg)) return rc;
    if (int rc = make_stack(m, g, covars, &s)) return rc;
    return launch_model(m, s, pg, weight, accumulate, out_dev, pick_stream(stream), g);
}

int mhs_members_predict_dev(const mhs_model *const *models, const double *weights, int n_models, const mhs_grid *g,
                            const mhs_stack *covars, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int accumulate,
                            double *out_dev, int64_t ld, void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(models && weights && n_models >= 1 && out_dev, "bad arguments");
    PredGeom pg;
    StackDev s;
    if (int rc = make_geom(g, r0, r1, c0, c1, ld, &pg)) return rc;
    for (int k = 0; k < n_models; ++k) {
        MHS_REQUIRE(models[k] != nullptr, "NULL model");
        if (int rc = make_stack(models[k], g, covars, &s)) return rc;     // every member must fit the stack
    }
    return launch_members(models, weights, n_models, s, pg, accumulate, out_dev, pick_stream(stream), g);
}

int mhs_ensemble_predict_dev(const mhs_model *const *models, const double *weights, int n_models,
                             double wt_total, const mhs_grid *g, const mhs_stack *covars, int64_t r0,
                             int64_t r1, int64_t c0, int64_t c1, double *out_dev, int64_t ld, void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(models && weights && n_models >= 1 && out_dev, "bad ensemble arguments");
    MHS_REQUIRE(wt_total != 0.0 && !std::isnan(wt_total), "wt_total must be non-zero");
    if (int rc = mhs_members_predict_dev(models, weights, n_models, g, covars, r0, r1, c0, c1, 0, out_dev, ld, stream)) return rc;
    return scale_window(out_dev, r1 - r0, c1 - c0, ld, wt_total, pick_stream(stream));
}

int mhs_predict_points(const mhs_model *m, const double *X, int64_t n, double *out_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(m && out_host && (X || n == 0) && n >= 0 && n < (1LL << 31), "bad arguments");
    if (n == 0) return MHS_OK;
    hipStream_t s = ctx().stream;
    DevBuf<double> dx, dout;
    MHS_HIP(dx.alloc((size_t)n * m->p));
    MHS_HIP(dout.alloc((size_t)n));
    MHS_HIP(hipMemcpyAsync(dx.p, X, sizeof(double) * (size_t)n * m->p, hipMemcpyHostToDevice, s));
    PredGeom pg;
    StackDev sd;
    points_stack(dx.p, m->p, n, &sd, &pg);
    if (int rc = launch_model(m, sd, pg, 1.0, 0, dout.p, s)) return rc;
    MHS_HIP(hipMemcpyAsync(out_host, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    return MHS_OK;
}

int mhs_gbm_probe_last(const mhs_model *m, int64_t *cost, int64_t *count) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(m && cost && count, "NULL argument");
    *cost = 0; *count = 0;
    if (m->kind != K_GBM || !m->gbm_probe || m->gbm_probe_next.load() == 0) return MHS_OK;
    int h[2 * GBC_PROBE_BLOCKS];
    MHS_HIP(hipDeviceSynchronize());
    MHS_HIP(hipMemcpy(h, m->gbm_probe + (size_t)((m->gbm_probe_next.load() - 1) % GBC_PROBE_SLOTS) * 2 * GBC_PROBE_BLOCKS, sizeof(h),
                      hipMemcpyDeviceToHost));
    for (int b = 0; b < GBC_PROBE_BLOCKS; ++b) { *cost += h[2 * b]; *count += h[2 * b + 1]; }
    return MHS_OK;
}

int mhs_gbm_staged_points(const mhs_model *m, const double *X, int64_t n, int step, double *out_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(m && X && out_host && n >= 1 && n < (1LL << 31) && step >= 1, "bad arguments");
    MHS_REQUIRE(m->kind == K_GBM, "not a gbm model");
    const int stages = m->n_trees / step;
    if (stages == 0) return MHS_OK;
    hipStream_t s = ctx().stream;
    DevBuf<double> dx, dout;
    MHS_HIP(dx.alloc((size_t)n * m->p));
    MHS_HIP(dout.alloc((size_t)n * stages));
    MHS_HIP(hipMemcpyAsync(dx.p, X, sizeof(double) * (size_t)n * m->p, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(gbm_staged_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m->nodes, m->tree_off,
                       m->n_trees, m->init_f, dx.p, n, step, dout.p);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(out_host, dout.p, sizeof(double) * (size_t)n * stages, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    return MHS_OK;
}

int mhs_residual_points(const mhs_model *const *models, const double *weights, int n_models, double wt_total,
                        const double *X, const double *resp, int64_t n, double *out_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(models && weights && X && resp && out_host && n_models >= 1 && n >= 1 && n < (1LL << 31), "bad arguments");
    MHS_REQUIRE(n_models <= 8, "at most 8 members");
    const int p = models[0]->p;
    for (int k = 0; k < n_models; ++k) MHS_REQUIRE(models[k] && models[k]->p == p, "models disagree on the number of predictors");
    hipStream_t s = ctx().stream;
    // one grow-only scratch: X (n x p), the members' predictions (n x K), resp, out
    Context &c = ctx();
    const size_t need = (size_t)n * ((size_t)p + (size_t)n_models + 2);
    if (need > c.points_arena_cap) {
        if (c.points_arena) { (void)hipStreamSynchronize(s); (void)hipFree(c.points_arena); c.points_arena = nullptr; c.points_arena_cap = 0; }
        MHS_HIP(hipMalloc((void **)&c.points_arena, need * sizeof(double)));
        c.points_arena_cap = need;
    }
    double *dx = c.points_arena, *dpred = dx + (size_t)n * p, *dresp = dpred + (size_t)n * n_models, *dout = dresp + n;
    MHS_HIP(hipMemcpyAsync(dx, X, sizeof(double) * (size_t)n * p, hipMemcpyHostToDevice, s));
    MHS_HIP(hipMemcpyAsync(dresp, resp, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    PredGeom pg;
    StackDev sd;
    points_stack(dx, p, n, &sd, &pg);
    for (int k = 0; k < n_models; ++k)
        if (int rc = launch_model(models[k], sd, pg, 1.0, 0, dpred + (size_t)k * n, s)) return rc;
    ResidualArgs ra;
    for (int k = 0; k < 8; ++k) ra.w[k] = k < n_models ? weights[k] : 0.0;
    hipLaunchKernelGGL(residual_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dpred, dresp, n, n_models, ra,
                       wt_total, dout);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(out_host, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    return MHS_OK;
}

int mhs_scale_add_dev(const double *a, double divisor, const double *b, double *out, int64_t n, void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(a && out && n >= 0, "bad arguments");
    if (n == 0) return MHS_OK;
    hipLaunchKernelGGL(scale_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pick_stream(stream), a, divisor, b, out, n);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

}  // extern "C"
