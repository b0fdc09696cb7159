// What zonal.hip shares with quantile.hip and sort_keys.hip: the geometry and counter block of a zonal call, its block of
// stream-ordered scratch, phase 1 (the range and zone check) as a function, and the sort's internal entry.
#pragma once
#include <cmath>
#include "ensemble_int.h"
#include "sort_keys.h"
#include "zonal_rule.h"

namespace mhs {

struct ZonalGeom {
    int nrow, ncol;
    double nodata;
    int has_nodata;
    int tiles_c;             // tiles side by side
};

struct ZonalCounters {
    unsigned long long max_abs_bits;         // the bits of max|v|: non-negative doubles order like their bits
    unsigned long long n_nonfinite, n_in_zone, n_contrib, n_inexact, n_present;
    unsigned zones_end;                      // max(zone) + 1
    unsigned bad;                            // 1: a zone >= n_zones; 2: a value that does not fit the quantum
};
static_assert(sizeof(ZonalCounters) <= 256, "the counter block");
enum { ZN_BAD_ZONE = 1, ZN_BAD_QUANTUM = 2 };

MHS_ZONAL_HD inline bool zn_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }

#define ZN_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// a block of stream-ordered memory, given back behind whatever was enqueued last
struct ZonalScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~ZonalScratch() { if (p) (void)hipFreeAsync(p, st); }
    int get(const char *fn, size_t bytes, hipStream_t s, const char *what) {
        st = s;
        if (hipMallocAsync((void **)&p, bytes, s) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            set_error("%s: no device memory for %s (%zu bytes)", fn, what, bytes);
            return MHS_ERR_ALLOC;
        }
        return MHS_OK;
    }
};

inline size_t zn_align(size_t n) { return (n + 255) & ~(size_t)255; }

// zonal.hip.  Phase 1 of a zonal call on the zeroed counter block `counters`: max|v| over the layer's valid finite cells,
// max(zone) + 1 and the +-Inf cells with a zone; the stream is synchronised and the block read into *c.  Then what the host
// decides from it: *n_zones 0 becomes max(zone) + 1, a zone >= *n_zones is refused naming n_zones; *quantum 0 becomes the
// default, a quantum the layer does not fit is refused naming quantum.
int zonal_measure(const char *fn, const ZonalGeom &g, int dtype, const void *plane, int64_t ldz, const int32_t *zones, int64_t ldq, hipStream_t st,
                  ZonalCounters *counters, ZonalCounters *c, int64_t *n_zones, double *quantum);

// sort_keys.hip.  keys[0 .. n) ascending by the bits [bit_lo, bit_hi), n > 0, with the caller's scratch: `alt` holds n keys,
// `counts` sort_counts_bytes(n) bytes.  The stream is synchronised once (the host reads the upfront histograms and leaves out
// every digit with a single occupied bin).  *where = keys or alt, whichever holds the result; where == NULL: the result is
// copied to keys when it ended in alt.
int sort_keys_run(const char *fn, uint64_t *keys, uint64_t *alt, void *counts, int64_t n, int bit_lo, int bit_hi, hipStream_t st, int *passes_run,
                  uint64_t **where);

}  // namespace mhs
