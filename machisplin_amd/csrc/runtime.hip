// Runtime of libmachisplin_hip.so: device selection, the library stream, error
// reporting, constant tables and HIP-event timers.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>
#include "common.h"

namespace mhs {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    (void)hipGetLastError();      // reported here: the next user of the runtime in this process (PyTorch) must not find it again
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? MHS_ERR_NODEVICE
         : e == hipErrorOutOfMemory ? MHS_ERR_ALLOC : MHS_ERR_HIP;
}

// ------------------------------------------------------------------ device slots --
namespace {
struct Slots {
    Context c[MAX_SLOTS];
    std::mutex pipe_mu[MAX_SLOTS], mask_mu[MAX_SLOTS], mosaic_mu[MAX_SLOTS][2], batch_mu[MAX_SLOTS];
    int count = 0;                        // slots 0 .. count - 1 are ready
};
Slots &slots() { static Slots s; return s; }
thread_local int t_slot = 0;
}  // namespace

int current_slot() { return t_slot; }
int slot_count() { return slots().count; }
Context &ctx_slot(int slot) { return slots().c[slot]; }
Context &ctx() { return slots().c[t_slot]; }

int bind_slot(int slot) {
    if (slot < 0 || slot >= MAX_SLOTS) { set_error("bind_slot: slot %d out of range", slot); return MHS_ERR_INVALID; }
    t_slot = slot;
    const Context &c = slots().c[slot];
    if (c.ready || c.device >= 0) MHS_HIP(hipSetDevice(c.device));
    return MHS_OK;
}

std::mutex &mask_mutex() { return slots().mask_mu[t_slot]; }
thread_local int t_mosaic_lane = 0;
int mosaic_lane() { return t_mosaic_lane; }
void set_mosaic_lane(int lane) { t_mosaic_lane = lane ? 1 : 0; }
std::mutex &mosaic_mutex() { return slots().mosaic_mu[t_slot][t_mosaic_lane]; }
std::mutex &batch_mutex() { return slots().batch_mu[t_slot]; }

namespace {
struct BlockPool {
    std::mutex mu;
    std::unordered_map<void *, size_t> cls;                 // every block handed out or parked -> its class (0 = direct)
    std::unordered_map<size_t, std::vector<void *>> parked;
};
BlockPool &block_pool(int slot) { static BlockPool p[MAX_SLOTS]; return p[slot]; }
constexpr size_t POOL_MAX_CLASS = (size_t)64 << 20;
}  // namespace

void *pool_alloc(size_t bytes) {
    size_t c = 256;
    while (c < bytes) c <<= 1;
    BlockPool &bp = block_pool(current_slot());
    if (c <= POOL_MAX_CLASS) {
        std::lock_guard<std::mutex> lk(bp.mu);
        auto it = bp.parked.find(c);
        if (it != bp.parked.end() && !it->second.empty()) { void *q = it->second.back(); it->second.pop_back(); return q; }
    }
    void *q = nullptr;
    const size_t want = c <= POOL_MAX_CLASS ? c : bytes;
    if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); set_error("out of device memory (%zu bytes)", want); return nullptr; }
    std::lock_guard<std::mutex> lk(bp.mu);
    bp.cls[q] = c <= POOL_MAX_CLASS ? c : 0;
    return q;
}

void pool_release(void *p) {
    if (!p) return;
    // the block goes back to the pool of the slot it came from, whichever slot the releasing thread is bound to (a
    // handle may be freed from the host's main thread after a worker thread of another slot built it)
    const int cur = current_slot();
    for (int k = 0; k < MAX_SLOTS; ++k) {
        const int slot = (cur + k) % MAX_SLOTS;
        BlockPool &bp = block_pool(slot);
        size_t c = 0;
        {
            std::lock_guard<std::mutex> lk(bp.mu);
            auto it = bp.cls.find(p);
            if (it == bp.cls.end()) continue;
            c = it->second;
            if (c) { bp.parked[c].push_back(p); return; }
            bp.cls.erase(it);
        }
        (void)hipFree(p);
        return;
    }
    // not ours (or the pool was cleared): leave it
}

void pool_clear() {
    BlockPool &bp = block_pool(current_slot());
    std::lock_guard<std::mutex> lk(bp.mu);
    for (auto &kv : bp.cls) (void)hipFree(kv.first);
    bp.cls.clear();
    bp.parked.clear();
}

std::mutex &pipe_mutex() { return slots().pipe_mu[t_slot]; }

int host_pipe(size_t arena_bytes) {
    Context &c = ctx();
    if (!c.pipe_h2d) {
        // copy streams at the lowest priority: they then do not share a hardware queue with a kernel stream, where a large copy
        // chunk would hold up every kernel queued behind it (multi.hip measured that on cfg4)
        int prio_lo = 0, prio_hi = 0;
        MHS_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        MHS_HIP(hipStreamCreateWithPriority(&c.pipe_h2d, hipStreamNonBlocking, prio_lo));
        MHS_HIP(hipStreamCreateWithPriority(&c.pipe_d2h, hipStreamNonBlocking, prio_lo));
        MHS_HIP(hipStreamCreateWithFlags(&c.pipe_comp, hipStreamNonBlocking));
        for (int i = 0; i < 8; ++i) {
            MHS_HIP(hipEventCreateWithFlags(&c.pipe_in[i], hipEventDisableTiming));
            MHS_HIP(hipEventCreateWithFlags(&c.pipe_done[i], hipEventDisableTiming));
            MHS_HIP(hipEventCreateWithFlags(&c.pipe_out[i], hipEventDisableTiming));
        }
    }
    if (arena_bytes > c.pipe_arena_cap) {      // grow-only; growing synchronises the device, the first calls only
        if (c.pipe_arena) {
            (void)hipStreamSynchronize(c.pipe_h2d); (void)hipStreamSynchronize(c.pipe_comp); (void)hipStreamSynchronize(c.pipe_d2h);
            (void)hipFree(c.pipe_arena); c.pipe_arena = nullptr; c.pipe_arena_cap = 0;
        }
        const size_t cap = arena_bytes + arena_bytes / 16;
        MHS_HIP(hipMalloc((void **)&c.pipe_arena, cap));
        c.pipe_arena_cap = cap;
    }
    return MHS_OK;
}

int plane_to_host(int64_t nr, int64_t nc, double *out_host, const std::function<int(double *dev, hipStream_t s)> &fill) {
    const size_t bytes = sizeof(double) * (size_t)(nr * nc);
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(std::max(bytes, sizeof(double)))) return rc;
    Context &c = ctx();
    if (int rc = fill((double *)c.pipe_arena, c.pipe_comp)) return rc;
    if (bytes == 0) return MHS_OK;
    MHS_HIP(hipMemcpyAsync(out_host, c.pipe_arena, bytes, hipMemcpyDeviceToHost, c.pipe_comp));
    MHS_HIP(hipStreamSynchronize(c.pipe_comp));
    return MHS_OK;
}

int fit_lane(int i, FitLane **out) {
    Context &c = ctx();
    // mhs_fit_reserve_cus walks c.lanes and rebuilds their masked streams under this mutex
    std::lock_guard<std::mutex> lk(mask_mutex());
    while ((int)c.lanes.size() <= i) {
        int prio_lo = 0, prio_hi = 0;
        MHS_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        FitLane *L = new FitLane();
        hipError_t e = hipStreamCreateWithPriority(&L->s, hipStreamNonBlocking, prio_hi);
        // the second stream carries the bulk of a trailing update while the first factorises the next panel: one priority
        // level down, so that the panel's few blocks win a freed compute unit against the update's hundreds of queued ones
        const int prio2 = prio_hi < prio_lo ? prio_hi + 1 : prio_hi;
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&L->s2, hipStreamNonBlocking, prio2);
        if (e == hipSuccess && c.masked_cus > 0 && !c.comp_mask.empty()) {
            e = hipExtStreamCreateWithCUMask(&L->ms, (uint32_t)c.comp_mask.size(), c.comp_mask.data());
            if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&L->ms2, (uint32_t)c.comp_mask.size(), c.comp_mask.data());
        }
        // The trailing update of the 32-column route (hundreds of blocks, two per compute unit, ~150 KB of LDS between
        // them) leaves the next panel's 10-20 blocks no compute unit to start on, whatever the priorities: beside it the
        // panel's first kernels ran 2-5 x slower (gram 9 -> 43 us, first pass 30 -> 72 us at n = 5 000).  Its stream is
        // therefore masked off the first 32 mask indices = four compute units of each XCD (the index order measured for
        // mhs_fit_reserve_cus below).
        if (e == hipSuccess && c.n_cu >= 128) {
            std::vector<uint32_t> mask((size_t)(c.n_cu + 31) / 32, 0u);
            for (int q = FIT_PANEL_CUS; q < c.n_cu; ++q) mask[(size_t)q / 32] |= 1u << (q % 32);
            e = hipExtStreamCreateWithCUMask(&L->s2r, (uint32_t)mask.size(), mask.data());
        }
        if (e != hipSuccess) {      // nothing half-built stays behind
            for (hipStream_t q : {L->s, L->s2, L->ms, L->ms2, L->s2r}) if (q) (void)hipStreamDestroy(q);
            delete L;
            return hip_fail(e, "fit_lane: stream creation", __FILE__, __LINE__);
        }
        c.lanes.push_back(L);
    }
    *out = c.lanes[(size_t)i];
    return MHS_OK;
}

int batch_lane(FitLane **out) {
    Context &c = ctx();
    std::lock_guard<std::mutex> lk(mask_mutex());
    if (!c.batch) {
        int prio_lo = 0, prio_hi = 0;
        MHS_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        FitLane *L = new FitLane();
        const hipError_t e = hipStreamCreateWithPriority(&L->s, hipStreamNonBlocking, prio_hi);
        if (e != hipSuccess) { delete L; return hip_fail(e, "batch_lane: stream creation", __FILE__, __LINE__); }
        c.batch = L;
    }
    *out = c.batch;
    return MHS_OK;
}

int h2d_sync(void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return MHS_OK;
    hipStream_t up = ctx().upload;
    MHS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, up));
    MHS_HIP(hipStreamSynchronize(up));
    return MHS_OK;
}

int require_ready() {
    if (!ctx().ready) {
        set_error("mhs_init() has not been called (or failed): no gfx950 device selected");
        return MHS_ERR_NODEVICE;
    }
    return MHS_OK;
}

// {2^1023 * (1/c_i rounded to double), -log(that 1/c_i)} with c_i the midpoint of
// [1 + i/N, 1 + (i+1)/N).  log(m) = logc_i + log1p(m*invc_i - 1), |m*invc_i - 1| <= 2^-11.
static void build_log_table(std::vector<double2> &tab) {
    tab.resize(LOG_TAB_N);
    for (int i = 0; i < LOG_TAB_N; ++i) {
        long double c = 1.0L + ((long double)i + 0.5L) / (long double)LOG_TAB_N;
        double invc = (double)(1.0L / c);
        double logc = (double)(-logl((long double)invc));
        // stored pre-scaled by 2^1023 (exact): table_log_biased subtracts the argument's exponent
        // field from it instead of extracting the argument's mantissa
        tab[i] = make_double2(ldexp(invc, 1023), logc);
    }
}

}  // namespace mhs

using namespace mhs;

extern "C" {

const char *mhs_last_error(void) { return g_err; }
const char *mhs_version(void) { return "machisplin_hip 0.1 (gfx950)"; }

int mhs_device_count(int *count) {
    MHS_REQUIRE(count != nullptr, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount", __FILE__, __LINE__); }
    *count = n;
    return MHS_OK;
}

// One slot = one Context on one physical device.  Called with the thread bound to nothing in particular; leaves the
// calling thread bound to the slot it found it on.
static int init_slot(int slot, int device) {
    Context &c = ctx_slot(slot);
    c.device = device;                          // bind_slot needs it before the context is ready
    SlotBind bind(slot);
    MHS_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MHS_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("mhs_init: device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return MHS_ERR_NODEVICE;
    }
    c.n_cu = prop.multiProcessorCount;
    // private streams for the host entry points (the fit's thousands of small dependent kernels): non-
    // blocking w.r.t. the default stream and high priority, so a fit can run beside long ensemble
    // kernels that a caller has enqueued on its own stream
    {
        FitLane *L0 = nullptr;
        if (int rc = fit_lane(0, &L0)) return rc;
        c.stream = L0->s;
    }
    MHS_HIP(hipStreamCreateWithFlags(&c.upload, hipStreamNonBlocking));
    MHS_HIP(hipEventCreate(&c.ev0));
    MHS_HIP(hipEventCreate(&c.ev1));
    std::vector<double2> tab;
    build_log_table(tab);
    MHS_HIP(hipMalloc((void **)&c.log_tab, sizeof(double2) * LOG_TAB_N));
    MHS_HIP(hipMemcpy(c.log_tab, tab.data(), sizeof(double2) * LOG_TAB_N, hipMemcpyHostToDevice));
    {   // 2^(j/4096), correctly rounded by the host libm (svr_kernel's exp)
        std::vector<double> et(4096);
        for (int j = 0; j < 4096; ++j) et[(size_t)j] = (double)exp2l((long double)j / 4096.0L);
        MHS_HIP(hipMalloc((void **)&c.exp_tab, sizeof(double) * et.size()));
        MHS_HIP(hipMemcpy(c.exp_tab, et.data(), sizeof(double) * et.size(), hipMemcpyHostToDevice));
    }
    c.ready = true;
    return MHS_OK;
}

static void shutdown_slot(int slot) {
    Context &c = ctx_slot(slot);
    if (!c.ready) { c = Context(); return; }
    SlotBind bind(slot);
    (void)hipStreamSynchronize(c.stream);
    reduction_cache_clear();              // device pointers of this device must not outlive it
    pool_clear();                         // (handles that outlive the shutdown release into an empty pool: ignored)
    if (c.log_tab) (void)hipFree(c.log_tab);
    if (c.surface_arena) (void)hipFree(c.surface_arena);
    for (char *&q : c.mosaic_arena) { if (q) (void)hipFree(q); q = nullptr; }
    c.mosaic_arena_cap[0] = c.mosaic_arena_cap[1] = 0;
    if (c.points_arena) (void)hipFree(c.points_arena);
    if (c.exp_tab) (void)hipFree(c.exp_tab);
    if (c.svr_pool) (void)hipFree(c.svr_pool);
    for (hipEvent_t pe : c.svr_pool_ev) if (pe) (void)hipEventDestroy(pe);
    if (c.upload) { (void)hipStreamSynchronize(c.upload); (void)hipStreamDestroy(c.upload); }
    for (hipStream_t ps : {c.pipe_h2d, c.pipe_comp, c.pipe_d2h})
        if (ps) { (void)hipStreamSynchronize(ps); (void)hipStreamDestroy(ps); }
    for (int i = 0; i < 8; ++i)
        for (hipEvent_t pe : {c.pipe_in[i], c.pipe_done[i], c.pipe_out[i]})
            if (pe) (void)hipEventDestroy(pe);
    if (c.pipe_arena) (void)hipFree(c.pipe_arena);
    if (c.ev0) (void)hipEventDestroy(c.ev0);
    if (c.ev1) (void)hipEventDestroy(c.ev1);
    if (c.masked_stream) { (void)hipStreamSynchronize(c.masked_stream); (void)hipStreamDestroy(c.masked_stream); }
    if (c.mask_ev0) (void)hipEventDestroy(c.mask_ev0);
    if (c.mask_ev1) (void)hipEventDestroy(c.mask_ev1);
    if (c.batch) {
        (void)hipStreamSynchronize(c.batch->s);
        if (c.batch->arena) (void)hipFree(c.batch->arena);
        (void)hipStreamDestroy(c.batch->s);
        delete c.batch;
    }
    for (FitLane *L : c.lanes) {
        (void)hipStreamSynchronize(L->s); (void)hipStreamSynchronize(L->s2);
        for (hipEvent_t e : L->pool) (void)hipEventDestroy(e);
        if (L->ms) { (void)hipStreamSynchronize(L->ms); (void)hipStreamSynchronize(L->ms2); (void)hipStreamDestroy(L->ms); (void)hipStreamDestroy(L->ms2); }
        if (L->arena) (void)hipFree(L->arena);
        if (L->pinned) (void)hipHostFree(L->pinned);
        if (L->s2r) { (void)hipStreamSynchronize(L->s2r); (void)hipStreamDestroy(L->s2r); }
        (void)hipStreamDestroy(L->s2); (void)hipStreamDestroy(L->s);
        delete L;
    }
    c = Context();
}

int mhs_init_devices(int n_devices, const int *device_ids) {
    MHS_REQUIRE(n_devices >= 1 && n_devices <= MAX_SLOTS, "n_devices must be between 1 and 16");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("mhs_init: no HIP device visible (%s)", e == hipSuccess ? "count 0" : hipGetErrorString(e));
        return MHS_ERR_NODEVICE;
    }
    for (int k = 0; k < n_devices; ++k) {
        const int d = device_ids ? device_ids[k] : k;
        MHS_REQUIRE(d >= 0 && d < n, "device index out of range");
    }
    Slots &S = slots();
    bool same = S.count == n_devices;
    for (int k = 0; same && k < n_devices; ++k)
        same = S.c[k].ready && S.c[k].device == (device_ids ? device_ids[k] : k);
    if (same) return bind_slot(0);
    if (S.count > 0) mhs_shutdown();
    multi_reset();                                    // per-device state of the multi-device drivers (multi.hip)
    for (int k = 0; k < n_devices; ++k) {
        if (int rc = init_slot(k, device_ids ? device_ids[k] : k)) {
            for (int q = 0; q <= k; ++q) shutdown_slot(q);
            S.count = 0;
            return rc;
        }
        S.count = k + 1;
    }
    // Peer access between every pair of distinct devices: the tile planes of multi.hip (hipMemcpyPeerAsync) then travel over
    // xGMI directly instead of through host memory.  A pair the hardware cannot connect keeps the staged copies; nothing
    // here is an error.
    for (int a = 0; a < n_devices; ++a)
        for (int b = 0; b < n_devices; ++b) {
            const int da = S.c[a].device, db = S.c[b].device;
            bool seen = da == db;
            for (int q = 0; q < b && !seen; ++q) seen = S.c[q].device == db;      // each peer once per owner
            for (int q = 0; q < a && !seen; ++q) seen = S.c[q].device == da;
            if (seen) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess || !can) { (void)hipGetLastError(); continue; }
            if (hipSetDevice(da) == hipSuccess) (void)hipDeviceEnablePeerAccess(db, 0);      // "already enabled" is fine
            (void)hipGetLastError();
        }
    // streams (CU-masked ones among them) are destroyed while the HIP runtime is still whole, whatever the host forgets:
    // handlers run in reverse order of registration, so this one runs before the runtime's own
    static bool registered = false;
    if (!registered) { registered = true; std::atexit([] { (void)mhs_shutdown(); }); }
    return bind_slot(0);
}

int mhs_init(int device) {
    Slots &S = slots();
    // slot 0 on `device` is all a one-device caller asks for: a host that has brought up several devices with
    // mhs_init_devices keeps them (the Python binding calls mhs_init from every helper)
    if (S.count >= 1 && S.c[0].ready && S.c[0].device == device) return bind_slot(0);
    return mhs_init_devices(1, &device);
}

int mhs_device_slots(int *n_slots, int *device_ids) {
    MHS_REQUIRE(n_slots != nullptr, "n_slots is NULL");
    *n_slots = slots().count;
    if (device_ids) for (int k = 0; k < slots().count; ++k) device_ids[k] = slots().c[k].device;
    return MHS_OK;
}

int mhs_shutdown(void) {
    Slots &S = slots();
    multi_reset();
    for (int k = 0; k < MAX_SLOTS; ++k) shutdown_slot(k);
    S.count = 0;
    (void)bind_slot(0);
    return MHS_OK;
}

int mhs_fit_reserve_cus(int n_cus, int *previous) {
    if (int rc = require_ready()) return rc;
    Context &c = ctx();
    MHS_REQUIRE(n_cus >= 0 && n_cus <= c.n_cu / 2 && n_cus % 8 == 0, "n_cus must be a multiple of 8 between 0 and half of the device's compute units");
    std::lock_guard<std::mutex> lk(mask_mutex());
    if (previous) *previous = c.reserved_cus;
    // Lifting the reservation gives the CU-masked streams back as well (round 6).  Rounds 2-5 kept them for the next time; but
    // while they exist -- the masked member's stream and every lane's pair confined to the reserved units -- a one-call tiled
    // Step 3 (mhs_tps_surface_dev: fits + evaluations on the library's own streams) leaves EVERY later kernel of the process,
    // on any stream, ~1.8 x slower until the streams are destroyed (tools/r06_masked_streams_probe.py,
    // profiles/r06_masked_streams_probe.txt: ksvm 115 -> 205 ms per 1e8 cells; neither the allocation, nor the mosaic, nor
    // stream priorities, nor a second stream reproduce it alone; mechanism inside the runtime not identified).  Creating three
    // masked streams again at the next reservation costs ~0.3 ms.  MHS_RESERVE_KEEP=1 restores the old behaviour.
    if (n_cus == 0 && !getenv("MHS_RESERVE_KEEP")) {
        if (c.masked_stream) { (void)hipStreamSynchronize(c.masked_stream); (void)hipStreamDestroy(c.masked_stream); c.masked_stream = nullptr; }
        for (FitLane *L : c.lanes)
            if (L->ms) { (void)hipStreamSynchronize(L->ms); (void)hipStreamSynchronize(L->ms2); (void)hipStreamDestroy(L->ms); (void)hipStreamDestroy(L->ms2); L->ms = L->ms2 = nullptr; }
        c.reserved_cus = c.masked_cus = 0;
        return MHS_OK;
    }
    if (n_cus == 0 || n_cus == c.masked_cus) { c.reserved_cus = n_cus; return MHS_OK; }   // the stream is kept for the next time
    if (c.masked_stream) { (void)hipStreamSynchronize(c.masked_stream); (void)hipStreamDestroy(c.masked_stream); c.masked_stream = nullptr; }
    c.reserved_cus = c.masked_cus = 0;
    std::vector<uint32_t> mask((size_t)(c.n_cu + 31) / 32, 0u), comp(mask.size(), 0u);
    for (int i = 0; i < c.n_cu; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    // Index i of the mask is compute unit i / 8 of XCD i % 8 (measured, tools/fit_beside_member.py: clearing every
    // 8th index -- one whole XCD -- is silently ignored, clearing the first n indices slows a masked kernel as n / 256
    // of the chip and more): the first n_cus indices = the same n_cus / 8 compute units of every XCD, so a grid's
    // blocks, which are dealt round-robin over the XCDs, find room in each of them.
    for (int i = 0; i < n_cus; ++i) {
        mask[(size_t)i / 32] &= ~(1u << (i % 32));
        comp[(size_t)i / 32] |= 1u << (i % 32);
    }
    MHS_HIP(hipExtStreamCreateWithCUMask(&c.masked_stream, (uint32_t)mask.size(), mask.data()));
    c.comp_mask = comp;
    for (FitLane *L : c.lanes) {
        if (L->ms) { (void)hipStreamSynchronize(L->ms); (void)hipStreamSynchronize(L->ms2); (void)hipStreamDestroy(L->ms); (void)hipStreamDestroy(L->ms2); L->ms = L->ms2 = nullptr; }
        MHS_HIP(hipExtStreamCreateWithCUMask(&L->ms, (uint32_t)comp.size(), comp.data()));
        MHS_HIP(hipExtStreamCreateWithCUMask(&L->ms2, (uint32_t)comp.size(), comp.data()));
    }
    if (!c.mask_ev0) {
        MHS_HIP(hipEventCreateWithFlags(&c.mask_ev0, hipEventDisableTiming));
        MHS_HIP(hipEventCreateWithFlags(&c.mask_ev1, hipEventDisableTiming));
    }
    c.reserved_cus = c.masked_cus = n_cus;
    return MHS_OK;
}

int mhs_sync(void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_HIP(hipStreamSynchronize(pick_stream(stream)));
    return MHS_OK;
}

int mhs_timer_start(void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_HIP(hipEventRecord(ctx().ev0, pick_stream(stream)));
    return MHS_OK;
}

int mhs_timer_stop(void *stream, double *elapsed_ms) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(elapsed_ms != nullptr, "elapsed_ms is NULL");
    MHS_HIP(hipEventRecord(ctx().ev1, pick_stream(stream)));
    MHS_HIP(hipEventSynchronize(ctx().ev1));
    float ms = 0.f;
    MHS_HIP(hipEventElapsedTime(&ms, ctx().ev0, ctx().ev1));
    *elapsed_ms = (double)ms;
    return MHS_OK;
}

}  // extern "C"
