// pred.elev from covariates in HOST memory (mhs_ensemble_predict): what the R shim calls with terra's in-memory rasters
// (V73:468-606 reads, predicts and writes block by block).  Host code only -- streams, events, the persistent arena, band
// plans: it reaches the device through launch_members and scale_window (ensemble.hip, where the kernels and everything that
// launches one live) and through copies.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "ensemble_int.h"

using namespace mhs;

// Error returns of the host-pointer pipelines: copies between the caller's pageable buffers and the arena may still be in flight on
// the three pipe streams when a later call fails; the caller is free to release its buffers once the entry point has returned,
// so every exit that is not the normal one drains the streams first (round-3 advisor finding).
struct PipeDrain {
    Context &c;
    bool done = false;
    explicit PipeDrain(Context &ctx_) : c(ctx_) {}
    ~PipeDrain() {
        if (done) return;
        (void)hipStreamSynchronize(c.pipe_h2d); (void)hipStreamSynchronize(c.pipe_comp); (void)hipStreamSynchronize(c.pipe_d2h);
    }
};

// Host-pointer ensemble, large windows (round 3).  Cutting the WHOLE member sequence into row bands hides the copies but
// pays the partly filled last round of every member kernel once per band (measured: 3 bands +20 ms on a 497 ms pass).  Only
// two things have to be banded: the FIRST member launch, so that it can start on the rows that have arrived while the rest
// of the covariates still travels (bands of 4, 16, 40, 40 % of the rows: the exposed upload is the 4 %), and the LAST one, so
// that finished rows travel back under the rows still being computed (48, 30, 14, 6, 2 %: the exposed download is the 2 %; round 5: both band plans grow no faster than the copies outrun the kernels, see below).
// Everything between them runs once over the whole window.  Per cell the members are still accumulated in the caller's
// order, so the plane equals the one-piece evaluation bit for bit.  The window lives in the persistent arena.
static int host_window_pipeline(const mhs_model *const *models, const double *weights, int n_models, int first_end, int last_start,
                                double wt_total, const mhs_grid *g, const mhs_stack *covars, int64_t r0, int64_t r1, int64_t c0,
                                int64_t c1, double *out_host) {
    const int64_t nr = r1 - r0, nc = c1 - c0;
    const size_t esz = dtype_bytes(covars->dtype);
    const size_t plane_bytes = (size_t)nr * covars->ld * esz;
    const size_t in_bytes = (plane_bytes * (size_t)covars->n_layers + 255) & ~(size_t)255;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(in_bytes + (size_t)nr * nc * sizeof(double))) return rc;
    Context &c = ctx();
    PipeDrain drain(c);
    char *in = c.pipe_arena;
    double *outp = (double *)(c.pipe_arena + in_bytes);
    // Upload bands: band b + 1 must have arrived when band b's kernels end, and the copies (0.43 ms per % of cfg3's three
    // float64 planes) are only ~2.2 x faster than the members that run on them (gbm + forest: 0.93 ms per %): with 4, 16, 40,
    // 40 % the device waited 3 ms for the 16 % and 2 ms for the first 40 %.  Float64 planes therefore go in five bands that
    // grow by at most that factor (3, 6, 13, 28, 50 %); float32 / int16 planes (half / a quarter of the bytes) keep four.
    const bool wide = covars->dtype == MHS_F64;
    const int NU = wide ? 5 : 4;
    const int pct_up5[5] = {3, 6, 13, 28, 50}, pct_up4[4] = {4, 16, 40, 40};
    // ... and the last member (ksvm: 1.1 ms per %) runs ~2.3 x slower than its rows travel down (0.48 ms per %): the same rule mirrored
    constexpr int ND = 5;
    const int pct_down[ND] = {48, 30, 14, 6, 2};
    int64_t up[6], down[ND + 1];
    up[0] = down[0] = r0;
    // cut at multiples of BAND_ALIGN grid rows (gbm_coherent_kernel's tiles are anchored to the grid: a band sees whole tiles)
    for (int b = 0, a = 0; b < NU; ++b) {
        a += wide ? pct_up5[b] : pct_up4[b];
        up[b + 1] = b == NU - 1 ? r1 : std::min(r1, std::max(up[b], (r0 + nr * a / 100 + BAND_ALIGN / 2) / BAND_ALIGN * BAND_ALIGN));
    }
    for (int b = 0, d = 0; b < ND; ++b) {
        d += pct_down[b];
        down[b + 1] = b == ND - 1 ? r1 : std::min(r1, std::max(down[b], (r0 + nr * d / 100 + BAND_ALIGN / 2) / BAND_ALIGN * BAND_ALIGN));
    }
    const StackDev sd = rows_stack(in, r0, r1, covars->n_layers, covars->dtype, covars->ld, covars->nodata);
    const bool timing = getenv("MHS_TIMING") != nullptr;
    const double t_start = now_ms();
    auto upload = [&](int b) -> int {           // rows [up[b], up[b + 1]) of every layer; blocks the calling thread (pageable source)
        for (int k = 0; k < covars->n_layers; ++k)
            MHS_HIP(hipMemcpyAsync(in + plane_bytes * k + (size_t)(up[b] - r0) * covars->ld * esz,
                                   (const char *)covars->data + ((size_t)k * covars->plane_stride + (size_t)up[b] * covars->ld) * esz,
                                   (size_t)(up[b + 1] - up[b]) * covars->ld * esz, hipMemcpyHostToDevice, c.pipe_h2d));
        MHS_HIP(hipEventRecord(c.pipe_in[b], c.pipe_h2d));
        return MHS_OK;
    };
    auto members = [&](int k0, int k1, int64_t b0, int64_t b1, int acc) -> int {
        PredGeom pg;
        if (int rc = make_geom(g, b0, b1, c0, c1, nc, &pg)) return rc;
        return launch_members(models + k0, weights + k0, k1 - k0, sd, pg, acc, outp + (size_t)(b0 - r0) * nc, c.pipe_comp, g);
    };
    if (int rc = upload(0)) return rc;
    for (int b = 0; b < NU; ++b) {
        MHS_HIP(hipStreamWaitEvent(c.pipe_comp, c.pipe_in[b], 0));
        if (up[b + 1] > up[b]) if (int rc = members(0, first_end, up[b], up[b + 1], 0)) return rc;
        if (b + 1 < NU) if (int rc = upload(b + 1)) return rc;
    }
    const double t_up = now_ms();
    if (last_start > first_end) if (int rc = members(first_end, last_start, r0, r1, 1)) return rc;
    for (int b = 0; b < ND; ++b) {
        if (down[b + 1] > down[b]) {
            if (int rc = members(last_start, n_models, down[b], down[b + 1], 1)) return rc;
            if (int rc = scale_window(outp + (size_t)(down[b] - r0) * nc, down[b + 1] - down[b], nc, nc, wt_total, c.pipe_comp)) return rc;
        }
        MHS_HIP(hipEventRecord(c.pipe_done[b], c.pipe_comp));
    }
    for (int b = 0; b < ND; ++b) {
        if (down[b + 1] == down[b]) continue;
        MHS_HIP(hipStreamWaitEvent(c.pipe_d2h, c.pipe_done[b], 0));
        MHS_HIP(hipMemcpyAsync(out_host + (size_t)(down[b] - r0) * nc, outp + (size_t)(down[b] - r0) * nc,
                               sizeof(double) * (size_t)((down[b + 1] - down[b]) * nc), hipMemcpyDeviceToHost, c.pipe_d2h));
    }
    MHS_HIP(hipStreamSynchronize(c.pipe_d2h));
    MHS_HIP(hipStreamSynchronize(c.pipe_comp));
    drain.done = true;
    if (timing) fprintf(stderr, "[mhs_ensemble_predict] window pipeline: uploads issued by %.1f ms, all done at %.1f ms\n", t_up - t_start, now_ms() - t_start);
    return MHS_OK;
}

extern "C" {

// The host-pointer form -- what the R shim calls with terra's in-memory rasters (V73:468-606 reads, predicts and writes
// block by block) -- as a three-stream pipeline over ROW BANDS: while band k is predicted, band k + 1's covariate rows
// travel host -> device and band k - 1's result device -> host.  Buffers come from the library's persistent arena (two
// covariate bands + two result bands; no hipMalloc / hipFree per call).  The host side issues, in this order, "kernels of
// band k, upload of band k + 1, download of band k - 1": copies from / to pageable memory block the CALLING THREAD until
// they are staged, so the kernels must already be in the queue when the thread goes into them.  Cells are independent
// and a band is described with the parent grid's affine, so the plane equals the one-piece evaluation bit for bit.
// MHS_HOST_BANDS = n forces n equal bands (1 = the serial round-2 behaviour, minus the allocations).
int mhs_ensemble_predict(const mhs_model *const *models, const double *weights, int n_models,
                         double wt_total, const mhs_grid *g, const mhs_stack *covars, int64_t r0,
                         int64_t r1, int64_t c0, int64_t c1, double *out_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(models && n_models >= 1 && g && covars && covars->data && out_host, "bad ensemble arguments");
    MHS_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= g->nrow && 0 <= c0 && c0 <= c1 && c1 <= g->ncol, "window outside the grid");
    const int64_t nr = r1 - r0, nc = c1 - c0;
    if (nr == 0 || nc == 0) return MHS_OK;
    for (int k = 0; k < n_models; ++k)
        MHS_REQUIRE(models[k] && covars->n_layers == models[k]->p - 2, "stack has the wrong number of layers for a model");
    const size_t esz = dtype_bytes(covars->dtype);
    // Large windows with at least two member launches: bands only where bytes cross PCIe (host_window_pipeline)
    if (!getenv("MHS_HOST_BANDS") && nr * nc >= 16000000 && nr >= 64) {
        int first_end = 1, last_start = n_models - 1;
        auto small = [](const mhs_model *m) { return m->kind == K_LM || m->kind == K_NNET || m->kind == K_EARTH; };
        if (small(models[0])) while (first_end < n_models && small(models[first_end]) && models[first_end]->kind > models[first_end - 1]->kind) ++first_end;
        if (small(models[last_start])) while (last_start > first_end && small(models[last_start - 1]) && models[last_start - 1]->kind < models[last_start]->kind) --last_start;
        const size_t need = (size_t)nr * covars->ld * esz * (size_t)covars->n_layers + (size_t)nr * nc * sizeof(double) + 512;
        // Round 4: every member before the last group runs on the UPLOAD bands (no whole-window middle group): the coherent gbm
        // kernel (40 ms per 1e8 cells) is as short as the upload of three float64 planes (43 ms at 56 GB/s), so with gbm alone on
        // the upload bands the last band's gbm ran after the last upload, fully exposed (+22 ms on cfg3); the forest's bands
        // cover it.  A banded launch costs the partly filled last round of its blocks, < 1 ms per band and member.
        if (last_start > first_end) first_end = last_start;
        if (last_start >= first_end && need <= ((size_t)96 << 30))
            return host_window_pipeline(models, weights, n_models, first_end, last_start, wt_total, g, covars, r0, r1, c0, c1, out_host);
    }
    // Band plan.  Measured on cfg3 (tools/r03_host_abi.py): the copies do hide behind the kernels, what a band costs is the
    // partly filled last round of each member kernel, ~3-5 ms per band -- so FEW bands; and all that stays exposed is the
    // first band's upload and the last band's download -- so those two bands are SHORT (8 % of the rows each, at least one
    // round of blocks over the device) and the rows between them go in bands of at most ~100 M cells (they bound the
    // arena: two covariate bands + two result bands).  Small windows go in one piece.  MHS_HOST_BANDS = n: n equal bands.
    std::vector<int64_t> edge;       // band b = rows [edge[b], edge[b + 1])
    edge.push_back(r0);
    const int64_t cells = nr * nc;
    if (const char *e = getenv("MHS_HOST_BANDS")) {
        const int64_t n = std::max<int64_t>(1, std::min<int64_t>(nr, atoll(e))), rp = (nr + n - 1) / n;
        for (int64_t r = r0 + rp; r < r1; r += rp) edge.push_back(r);
    } else if (cells >= 16000000 && nr >= 8) {
        const int64_t ends = std::min<int64_t>(nr / 4, std::max<int64_t>((nr * 8 + 99) / 100, (1500000 + nc - 1) / nc));
        const int64_t mid = nr - 2 * ends, nmid = std::max<int64_t>(1, (mid * nc + 99999999) / 100000000), rp = (mid + nmid - 1) / nmid;
        for (int64_t r = r0 + ends; r < r1 - ends; r += rp) edge.push_back(r);
        edge.push_back(r1 - ends);
    }
    edge.push_back(r1);
    // cuts at multiples of BAND_ALIGN grid rows: gbm_coherent_kernel's tiles are anchored there, so a band sees whole tiles
    // and its cells the same sums as in a resident call
    for (size_t b = 1; b + 1 < edge.size(); ++b) edge[b] = std::min(r1, std::max(r0, (edge[b] + BAND_ALIGN / 2) / BAND_ALIGN * BAND_ALIGN));
    edge.erase(std::unique(edge.begin(), edge.end()), edge.end());
    const int64_t nb = (int64_t)edge.size() - 1;
    int64_t rows_per = 0;
    for (int64_t b = 0; b < nb; ++b) rows_per = std::max(rows_per, edge[(size_t)b + 1] - edge[(size_t)b]);
    const size_t in_bytes = ((size_t)rows_per * covars->ld * esz * (size_t)covars->n_layers + 255) & ~(size_t)255;
    const size_t out_bytes = ((size_t)rows_per * nc * sizeof(double) + 255) & ~(size_t)255;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(2 * (in_bytes + out_bytes))) return rc;
    Context &c = ctx();
    PipeDrain drain(c);
    char *in[2] = {c.pipe_arena, c.pipe_arena + in_bytes};
    double *outb[2] = {(double *)(c.pipe_arena + 2 * in_bytes), (double *)(c.pipe_arena + 2 * in_bytes + out_bytes)};
    const bool timing = getenv("MHS_TIMING") != nullptr;
    const double t_start = now_ms();
    auto band_rows = [&](int64_t b, int64_t *b0, int64_t *b1) { *b0 = edge[(size_t)b]; *b1 = edge[(size_t)b + 1]; };
    auto upload = [&](int64_t b) -> int {
        const int sl = (int)(b & 1);
        int64_t b0, b1;
        band_rows(b, &b0, &b1);
        if (b >= 2) MHS_HIP(hipStreamWaitEvent(c.pipe_h2d, c.pipe_done[sl], 0));      // band b - 2's kernels read this buffer
        const size_t plane_bytes = (size_t)(b1 - b0) * covars->ld * esz;
        for (int k = 0; k < covars->n_layers; ++k) {
            const char *src = (const char *)covars->data + ((size_t)k * covars->plane_stride + (size_t)b0 * covars->ld) * esz;
            MHS_HIP(hipMemcpyAsync(in[sl] + plane_bytes * k, src, plane_bytes, hipMemcpyHostToDevice, c.pipe_h2d));
        }
        MHS_HIP(hipEventRecord(c.pipe_in[sl], c.pipe_h2d));
        return MHS_OK;
    };
    auto download = [&](int64_t b) -> int {
        const int sl = (int)(b & 1);
        int64_t b0, b1;
        band_rows(b, &b0, &b1);
        MHS_HIP(hipStreamWaitEvent(c.pipe_d2h, c.pipe_done[sl], 0));
        MHS_HIP(hipMemcpyAsync(out_host + (size_t)(b0 - r0) * nc, outb[sl], sizeof(double) * (size_t)((b1 - b0) * nc), hipMemcpyDeviceToHost,
                               c.pipe_d2h));
        MHS_HIP(hipEventRecord(c.pipe_out[sl], c.pipe_d2h));
        return MHS_OK;
    };
    if (int rc = upload(0)) return rc;
    for (int64_t b = 0; b < nb; ++b) {
        const int sl = (int)(b & 1);
        int64_t b0, b1;
        band_rows(b, &b0, &b1);
        hipStream_t cs = c.pipe_comp;
        MHS_HIP(hipStreamWaitEvent(cs, c.pipe_in[sl], 0));
        if (b >= 2) MHS_HIP(hipStreamWaitEvent(cs, c.pipe_out[sl], 0));       // band b - 2's result has left this buffer
        PredGeom pg;
        if (int rc = make_geom(g, b0, b1, c0, c1, nc, &pg)) return rc;
        const StackDev sd = rows_stack(in[sl], b0, b1, covars->n_layers, covars->dtype, covars->ld, covars->nodata);
        if (int rc = launch_members(models, weights, n_models, sd, pg, 0, outb[sl], cs, g)) return rc;
        if (int rc = scale_window(outb[sl], b1 - b0, nc, nc, wt_total, cs)) return rc;
        MHS_HIP(hipEventRecord(c.pipe_done[sl], cs));
        const double t0 = now_ms();
        if (b + 1 < nb) if (int rc = upload(b + 1)) return rc;
        const double t1 = now_ms();
        if (b >= 1) if (int rc = download(b - 1)) return rc;
        if (timing) fprintf(stderr, "[mhs_ensemble_predict] band %lld launched at %.1f ms: upload of the next %.1f ms, download of the previous %.1f ms\n",
                            (long long)b, t0 - t_start, t1 - t0, now_ms() - t1);
    }
    if (int rc = download(nb - 1)) return rc;
    MHS_HIP(hipStreamSynchronize(c.pipe_d2h));
    MHS_HIP(hipStreamSynchronize(c.pipe_comp));
    drain.done = true;
    return MHS_OK;
}

}  // extern "C"
