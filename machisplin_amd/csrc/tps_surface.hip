// Step 3 + Step 4 of machisplin.mltps in ONE call (V73:636-897): tile grid, per-tile
// fields::Tps on the stations of the fit box, evaluation on the keep window, mean mosaic,
// seam feathering, overlay.  This is the entry point a .Call() shim binds so that the R
// side replaces the whole block by a single call; the Python mirror composes the same
// steps from the finer-grained entry points (machisplin_amd/mltps.py).
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "common.h"
#include "step3_plan.h"
#include "tps_batch.h"

using namespace mhs;

constexpr int64_t TILE_LANES = 8;   // tiles fitted side by side (mhs_tps_surface)

// MHS_TIMING: the host time since the previous lap, on stderr
struct Lap {
    const char *who; int width;
    bool on = getenv("MHS_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[%s] %-*s %8.3f ms\n", who, width, what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};

// Fit and evaluate a set of Step-3 tiles: job k = tile tile_ids[k] (or tile k), its keep-window plane (rows x cols of
// the window, contiguous) written to out_ptrs[k].  Returns after everything has finished.
//
// Round 6: every tile with 8..256 distinct stations -- all of them at the reference's tile size (105-250
// per tile) -- goes through ONE fit launch (tps_batch.hip: a workgroup per spline) and ONE pair of evaluation launches
// (tps_eval.hip: a window per spline, knots and polynomial part read where the fit left them): three kernels and two
// copies for the whole set, where rounds 1-5 drove a chain of ~10 launches and 4 host round trips per tile from eight
// host threads (41 ms for cfg3's 49 tiles; the launches were the time).  Tiles the batch cannot hold (more than 256
// stations: tile_edge far above the reference's 1500) still take that route, on the lanes, beside the batch.
// MHS_TILES_BATCH=0 sends every tile down the lanes (the parity tests compare the two).
static int run_tiles(const mhs_grid *g, const Step3Plan &P, const double *xy, const double *resid, int64_t n,
                     const double *cov1_at_stations, double lambda, int gcv_mode, const int64_t *tile_ids, int64_t njobs,
                     double *const *out_ptrs) {
    if (njobs <= 0) return MHS_OK;
    std::vector<int64_t> rows((size_t)n), cols((size_t)n);
    if (int rc = mhs_cells_from_xy(g, xy, n, rows.data(), cols.data())) return rc;
    Lap lap{"run_tiles", 36};
    const char *benv = getenv("MHS_TILES_BATCH");
    const bool use_batch = !(benv && benv[0] == '0');
    // ---- the tiles' stations (terra::extract(rb[[1]], Full.cords) + complete.cases, V73:701-706)
    struct Job {
        int64_t h = 0, m = 0, r0 = 0, r1 = 0, c0 = 0, c1 = 0;      // tile, stations, the keep window in the fit raster's rows / columns
        std::vector<double> txy, sr;
        int route = 0;      // 0 zeros, 1 batch, 2 lane
        int bjob = -1, rc = MHS_OK;
        std::string err;
        EvalPlanHandle *plan = nullptr;
        std::vector<int> perm;
    };
    std::vector<Job> jobs((size_t)njobs);
    std::vector<TpsPrep> preps((size_t)njobs);
    std::vector<int64_t> lane_jobs;
    std::vector<mhs_tps *> handles;     // the lane tiles' splines: freed after the last tile (hipFree synchronises the device)
    std::vector<FitLane *> lanes;
    std::lock_guard<std::mutex> batch_lock(batch_mutex());
    FitLane *Lb = nullptr;
    if (int rc = batch_lane(&Lb)) return rc;
    const hipStream_t sb = Lb->s;
    SmallBatch B;
    EvalBatch *EB = eval_batch_create();
    struct EbGuard { EvalBatch *p; ~EbGuard() { eval_batch_destroy(p); } } eb_guard{EB};
    // Every return from here on, the failures included: nothing launched below may still be writing out_ptrs or using the
    // batch's or a lane's arena when batch_mutex is released.  After a successful run every stream is idle already.
    struct Quiesce {
        std::vector<Job> &jobs; hipStream_t sb; std::vector<FitLane *> &lanes; std::vector<mhs_tps *> &handles;
        ~Quiesce() {
            for (Job &J : jobs) if (J.plan) eval_plan_drop(J.plan);
            (void)hipStreamSynchronize(sb);
            for (FitLane *L : lanes) if (L) { (void)hipStreamSynchronize(L->s); if (L->ms) (void)hipStreamSynchronize(L->ms); }
            for (mhs_tps *t : handles) tps_free_quiet(t);
        }
    } quiesce{jobs, sb, lanes, handles};
    // Everything the host does per tile before the launches -- its stations (an O(n) scan), Krig's replicate collapse, the
    // QR of [1 u v], the evaluation plan's counting sort -- is independent of the other tiles: a few host threads share
    // the tiles (2.1 ms on one thread for cfg3's 49 tiles, as long as the kernels they feed).
    auto prepare_one = [&](int64_t job) {
        Job &J = jobs[(size_t)job];
        J.h = tile_ids ? tile_ids[job] : job;
        P.keep_in_fit(J.h, &J.r0, &J.r1, &J.c0, &J.c1);
        step3_stations(P, J.h, rows.data(), cols.data(), xy, resid, cov1_at_stations, n, J.txy, J.sr);
        J.m = (int64_t)J.sr.size();
        if (J.m < STEP3_MIN_STATIONS) { J.route = 0; return; }      // V73:710-721: the tile is all zeros
        J.route = 2;
        if (use_batch && J.m <= 4 * SB_NMAX) {      // (replicates can only shrink the count)
            TpsPrep &Q = preps[(size_t)job];
            J.rc = tps_prepare(J.txy.data(), J.sr.data(), J.m, Q);
            if (J.rc) { J.err = mhs_last_error(); return; }
            if (Q.n >= SB_NMIN && Q.n <= SB_NMAX) {
                // terra::interpolate(terra::rast(rb), tps): cell centres of the FIT raster (V73:726), the keep window of it
                const mhs_grid gf = P.fit_grid(g, J.h);
                J.plan = eval_batch_plan(Q.uv.data(), (int)Q.n, Q.center, Q.scale, &gf, J.r0, J.r1, J.c0, J.c1, out_ptrs[job],
                                         J.c1 - J.c0, J.perm, &J.rc);
                if (J.rc) { J.err = mhs_last_error(); return; }
                J.route = 1;
            }
        }
    };
    {
        const int nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(njobs / 8, 6), cpu_budget()));
        std::atomic<int64_t> next{0};
        auto work = [&]() { for (;;) { const int64_t job = next.fetch_add(1); if (job >= njobs) break; prepare_one(job); } };
        std::vector<std::thread> threads;
        for (int q = 1; q < nthreads; ++q) threads.emplace_back(work);
        work();
        for (std::thread &th : threads) th.join();
    }
    for (int64_t job = 0; job < njobs; ++job) {      // in job order: errors, the zero tiles, the batch's entries
        Job &J = jobs[(size_t)job];
        if (J.rc) { set_error("%s", J.err.c_str()); return J.rc; }
        if (J.route == 0) MHS_HIP(hipMemsetAsync(out_ptrs[job], 0, sizeof(double) * (size_t)((J.r1 - J.r0) * (J.c1 - J.c0)), sb));
        else if (J.route == 1) {
            eval_batch_commit(EB, J.plan, B.count, B.knot_total);
            J.plan = nullptr;
            J.bjob = small_batch_add(B, preps[(size_t)job], lambda, gcv_mode, J.perm.data());
        } else lane_jobs.push_back(job);
    }
    lap("stations, preparation, plans (host)");
    // ---- the batch: fit launch, then the two evaluation launches behind it on the same stream
    char *extra = nullptr;
    if (int rc = small_batch_launch(B, *Lb, sb, eval_batch_device_bytes(EB), &extra)) return rc;
    if (B.count > 0)
        if (int rc = eval_batch_launch(EB, extra, B.knots_dev, B.res_dev, sb)) return rc;
    lap("uploads + launches");
    // ---- the other tiles: chains of small, latency-bound kernels, several side by side, each on its own lane (two streams +
    // work arena) driven by its own host thread
    int rc = MHS_OK;
    std::string err_msg;
    handles.assign(lane_jobs.size(), nullptr);
    if (!lane_jobs.empty()) {
        const int nlanes = (int)std::min<int64_t>((int64_t)lane_jobs.size(), TILE_LANES);
        lanes.assign((size_t)nlanes, nullptr);
        for (int l = 0; l < nlanes; ++l)
            if (int rc2 = fit_lane(1 + l, &lanes[(size_t)l])) return rc2;
        std::atomic<int64_t> next{0};
        std::atomic<int> first_rc{MHS_OK};
        std::mutex err_mu;
        const int slot = current_slot();
        auto worker = [&](int lane_id) {
            FitLane &L = *lanes[(size_t)lane_id];
            SlotBind bind(slot);                // the slot and HIP's current device are per host thread
            // mhs_fit_reserve_cus active: the tiles' evaluations stay, like their fits, on the reserved compute units
            const hipStream_t ls = (ctx().reserved_cus > 0 && L.ms) ? L.ms : L.s;
            for (;;) {
                const int64_t q = next.fetch_add(1);
                if (q >= (int64_t)lane_jobs.size() || first_rc.load() != MHS_OK) break;
                const int64_t job = lane_jobs[(size_t)q];
                Job &J = jobs[(size_t)job];
                mhs_tps *t = nullptr;
                int rc2 = tps_fit_lane(L, J.txy.data(), J.sr.data(), J.m, lambda, gcv_mode, J.m < 1500 ? 2 : 0, &t);
                if (!rc2) {
                    handles[(size_t)q] = t;
                    const mhs_grid gf = P.fit_grid(g, J.h);
                    rc2 = mhs_tps_predict_grid_dev(t, &gf, J.r0, J.r1, J.c0, J.c1, out_ptrs[job], J.c1 - J.c0, ls);
                }
                if (rc2) {
                    int expected = MHS_OK;
                    if (first_rc.compare_exchange_strong(expected, rc2)) {
                        std::lock_guard<std::mutex> lk(err_mu);
                        err_msg = mhs_last_error();   // thread-local in the worker: carry it to the caller
                    }
                    break;
                }
            }
        };
        {
            std::vector<std::thread> threads;
            for (int l = 1; l < nlanes; ++l) threads.emplace_back(worker, l);
            worker(0);
            for (std::thread &th : threads) th.join();
        }
        rc = first_rc.load();
        for (FitLane *L : lanes) {
            if (hipStreamSynchronize(L->s) != hipSuccess && !rc) rc = MHS_ERR_HIP;
            if (L->ms && hipStreamSynchronize(L->ms) != hipSuccess && !rc) rc = MHS_ERR_HIP;
        }
    }
    // ---- the batch's verdicts
    std::vector<SmallResult> res;
    if (int rc2 = small_batch_results(B, sb, res, nullptr)) { if (!rc) rc = rc2; }
    else if (hipStreamSynchronize(sb) != hipSuccess) { if (!rc) rc = MHS_ERR_HIP; }
    lap("wait for the kernels (+ lanes)");
    if (rc) { if (!err_msg.empty()) set_error("%s", err_msg.c_str()); return rc; }
    for (const SmallResult &r : res)
        if (r.status != 0.0) { set_error("mhs_tps_fit: GCV search failed"); return MHS_ERR_NUMERIC; }
    if (lap.on && !res.empty()) {
        double t[8] = {0};
        for (const SmallResult &r : res) for (int q = 0; q < 8; ++q) t[q] += r.t_us[q] / (double)res.size();
        fprintf(stderr, "[run_tiles] %d tiles batched, %d on the lanes; mean us per batched fit: gram %.1f projection %.1f tridiagonalisation %.1f "
                "eigenvalues %.1f bracket+grid %.1f golden section %.1f solve+back-transform %.1f\n", (int)res.size(), (int)lane_jobs.size(),
                t[6], t[0], t[1], t[2], t[3], t[4], t[5]);
    }
    return MHS_OK;
}

extern "C" int mhs_tps_surface_dev(const mhs_grid *g, const double *xy, const double *resid, int64_t n,
                                   const double *cov1_at_stations, int64_t tile_edge, double lambda,
                                   int gcv_mode, double *out_dev, int64_t ld, int64_t *tiles_out,
                                   void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(g && xy && resid && out_dev && n > 0 && ld >= g->ncol, "bad arguments");
    Step3Plan P;
    if (int rc = step3_plan(g, tile_edge, P)) return rc;
    if (tiles_out) { tiles_out[0] = P.nRx; tiles_out[1] = P.nCx; }
    hipStream_t s = pick_stream(stream);
    if (P.nt == 1) {  // V73:748-753
        mhs_tps *t = nullptr;
        if (int rc = mhs_tps_fit(xy, resid, n, lambda, gcv_mode, &t)) return rc;
        int rc = mhs_tps_predict_grid_dev(t, g, 0, g->nrow, 0, g->ncol, out_dev, ld, s);
        if (!rc) rc = (hipStreamSynchronize(s) == hipSuccess) ? MHS_OK : MHS_ERR_HIP;
        mhs_tps_free(t);
        return rc;
    }
    Lap lap{"mhs_tps_surface", 28};
    // the tiles' keep windows (~1.1 x the grid in total) live in one grow-only scratch buffer of the library
    const std::vector<size_t> off = P.pack();
    const size_t total = off[(size_t)P.nt];
    Context &c = ctx();
    if (total > c.surface_arena_cap) {
        if (c.surface_arena) { (void)hipDeviceSynchronize(); (void)hipFree(c.surface_arena); c.surface_arena = nullptr; c.surface_arena_cap = 0; }
        MHS_HIP(hipMalloc((void **)&c.surface_arena, total * sizeof(double)));
        c.surface_arena_cap = total;
    }
    std::vector<double *> outs((size_t)P.nt);
    for (int64_t h = 0; h < P.nt; ++h) outs[(size_t)h] = c.surface_arena + off[(size_t)h];
    lap("windows + tile buffers");
    int rc = run_tiles(g, P, xy, resid, n, cov1_at_stations, lambda, gcv_mode, nullptr, P.nt, outs.data());
    lap("tile fits + evaluation");
    if (rc) return rc;
    rc = mosaic_feather_impl(g, P.nRx, P.nCx, P.keep.data(), outs.data(), 0, out_dev, ld, nullptr, s, true);      // spline planes: no NA
    if (lap.on) { (void)hipStreamSynchronize(s); lap("mosaic + feather"); }
    return rc;
}

extern "C" int mhs_tps_surface(const mhs_grid *g, const double *xy, const double *resid, int64_t n,
                               const double *cov1_at_stations, int64_t tile_edge, double lambda, int gcv_mode,
                               double *out_host, int64_t *tiles_out) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(g && out_host && g->nrow > 0 && g->ncol > 0, "bad arguments");
    return plane_to_host(g->nrow, g->ncol, out_host, [&](double *out, hipStream_t s) {
        return mhs_tps_surface_dev(g, xy, resid, n, cov1_at_stations, tile_edge, lambda, gcv_mode, out, g->ncol, tiles_out, s); });
}

extern "C" int mhs_tps_tiles_dev(const mhs_grid *g, const double *xy, const double *resid, int64_t n,
                                 const double *cov1_at_stations, int64_t tile_edge, double lambda, int gcv_mode,
                                 const int64_t *tile_ids, int64_t n_ids, double *const *out_dev_ptrs) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(g && xy && resid && n > 0 && tile_edge > 0 && n_ids >= 0 && (n_ids == 0 || (tile_ids && out_dev_ptrs)), "bad arguments");
    Step3Plan P;
    if (int rc = step3_plan(g, tile_edge, P)) return rc;
    for (int64_t k = 0; k < n_ids; ++k) MHS_REQUIRE(tile_ids[k] >= 0 && tile_ids[k] < P.nt && out_dev_ptrs[k], "tile id out of range or NULL output");
    return run_tiles(g, P, xy, resid, n, cov1_at_stations, lambda, gcv_mode, tile_ids, n_ids, out_dev_ptrs);
}
