// What the five device fits (gbm_fit.hip, rf_fit.hip, earth_fit.hip, and learn_fit.hip's nnet and ksvm) share: the wave
// primitives whose lane order fixes the last bits of every sum -- the fits promise models that are bit-identical from
// call to call and independent of what shares the launch, and that promise is the order written HERE -- and the host's
// staging of a batch (argument checks, the rows sorted per variable, the typed staging block of fit_stage.h on the device).
#pragma once
#include <cmath>
#include <numeric>
#include "common.h"
#include "fit_stage.h"

namespace mhs {

// The counter-based generator behind every draw the caller seeds (the header's mix(z)): randomForest's per-node variable draw
// (rf_fit.hip) and the keys of its permutation importance (rf_importance.hip).
__host__ __device__ inline unsigned long long fit_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------- device: one wave of 64 lanes

// The wave's sum by an xor butterfly: every lane adds the same pairs, so all lanes hold one value.  NOT devmath.h's
// wave_sum, which adds in another order.
template <typename T>
__device__ __forceinline__ T fit_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// Inclusive prefix sum over the lanes (Hillis-Steele): lane l gets v_0 + ... + v_l, added in log depth.
template <typename T>
__device__ __forceinline__ T fit_wave_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v = v + t;
    }
    return v;
}

// The wave's best of every lane's (val, pos): the greater value wins, equal positive values go to the lower position;
// val = 0 means none.  In: a lane's own best (its positions are unique over the wave); out, in every lane: the wave's.
// Returns the lane that owns the winner (0 without one), from which the caller fetches the payload with __shfl.
__device__ __forceinline__ int fit_wave_argbest(double &val, int &pos) {
    const double mine = val;
    const int mpos = pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(val, o);
        const int p2 = __shfl_xor(pos, o);
        if (v2 > val || (v2 == val && v2 > 0.0 && p2 < pos)) { val = v2; pos = p2; }
    }
    const unsigned long long own = __ballot(val > 0.0 && mine == val && mpos == pos);
    return own ? __ffsll((long long)own) - 1 : 0;
}

// dst[0 .. cap) <- the rows of src[0 .. n) with flag[row] > 0, in src's order (ballot / popcount; the whole wave calls).
template <typename F>
__device__ __forceinline__ void fit_compact_order(const int *src, int n, const F *flag, int *dst, int cap) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int at = 0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const int row = j < n ? src[j] : 0;
        const bool f = j < n && flag[row] > 0;
        const unsigned long long bl = __ballot(f);
        const int to = at + __popcll(bl & lt);
        if (f && to < cap) dst[to] = row;
        at += __popcll(bl);
    }
}

// Stable partition of src[0 .. m) into dst[0 .. m): the nl rows with mark[row] != 0 first, the others behind them, both
// in src's order (the whole wave calls).
__device__ __forceinline__ void fit_partition(const int *src, int *dst, int m, int nl, const unsigned char *mark) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int cl = 0, cr = 0;
    for (int base = 0; base < m; base += 64) {
        const int j = base + lane;
        const int row = j < m ? src[j] : 0;
        const bool f = j < m && mark[row], g = j < m && !mark[row];
        const unsigned long long bl = __ballot(f), br = __ballot(g);
        const int tl = cl + __popcll(bl & lt), tr = nl + cr + __popcll(br & lt);
        if (f && tl < nl) dst[tl] = row;
        if (g && tr < m) dst[tr] = row;
        cl += __popcll(bl); cr += __popcll(br);
    }
}

// ---------------------------------------------------------------- host: staging a batch of models

// A FitPlan with its device memory: ONE allocation of the planned bytes, and ONE hipMemcpyAsync per upload / download of
// a byte range [a, b) that the mirror holds.
struct FitBlock : FitPlan {
    DevBuf<char> d;
    hipError_t alloc() { return d.alloc(at); }
    template <typename T>
    T *dev(FitPiece<T> q) const { assert(d.p && q.off + q.bytes() <= d.n); return reinterpret_cast<T *>(d.p + q.off); }
    hipError_t upload(size_t a, size_t b, hipStream_t s) {
        assert(from <= a && a <= b && b <= to && b <= d.n);
        return hipMemcpyAsync(d.p + a, buf.data() + (a - from), b - a, hipMemcpyHostToDevice, s);
    }
    hipError_t download(size_t a, size_t b, hipStream_t s) {
        assert(from <= a && a <= b && b <= to && b <= d.n);
        return hipMemcpyAsync(buf.data() + (a - from), d.p + a, b - a, hipMemcpyDeviceToHost, s);
    }
    hipError_t zero(size_t a, size_t b, hipStream_t s) { assert(a <= b && b <= d.n); return hipMemsetAsync(d.p + a, 0, b - a, s); }
    template <typename T>
    hipError_t zero(FitPiece<T> q, hipStream_t s) { return zero(q.off, q.off + q.bytes(), s); }
};

// out (p x n) <- the rows in ascending order of every column of X (n x p column-major), ties in row order
inline void fit_sorted_orders(const double *X, int64_t n, int p, int *out) {
    for (int v = 0; v < p; ++v) {
        int *o = out + (size_t)v * n;
        const double *col = X + (size_t)v * n;
        std::iota(o, o + n, 0);
        std::stable_sort(o, o + n, [col](int a, int b) { return col[a] < col[b]; });
    }
}

// The arguments every batched fit takes, checked as MHS_REQUIRE would in the entry point fn: the batch (count, p), then,
// model by model, its X (n x p column-major) and y (n) -- present, n in range, every value finite.  FIT_REQUIRE is for
// the host code of a fit that has the entry point's name in `fn`.
#define FIT_REQUIRE(cond, msg)                                               \
    do {                                                                     \
        if (!(cond)) { set_error("%s: %s", fn, msg); return MHS_ERR_INVALID; } \
    } while (0)

inline int fit_check_batch(const char *fn, int count, int p, int max_p, int min_p = 2) {
    FIT_REQUIRE(count >= 1 && count <= 65535, "count out of range");
    if (!(p >= min_p && p <= max_p)) {
        set_error("%s: p (covariates + LONG + LAT) out of range: this fit takes %d .. %d predictors", fn, min_p, max_p);
        return MHS_ERR_INVALID;
    }
    return MHS_OK;
}

inline int fit_check_model(const char *fn, const double *X, const double *y, int64_t n, int p) {
    FIT_REQUIRE(X && y, "NULL array of a model");
    FIT_REQUIRE(n >= 1 && n * (int64_t)p < (1LL << 31), "n out of range");
    for (int64_t e = 0; e < n * p; ++e) FIT_REQUIRE(std::isfinite(X[e]), "NaN or infinite predictor (the training rows have no NA, V73:154)");
    for (int64_t i = 0; i < n; ++i) FIT_REQUIRE(std::isfinite(y[i]), "non-finite response");
    return MHS_OK;
}

}  // namespace mhs
