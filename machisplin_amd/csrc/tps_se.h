// What the two builds of Q = -M^-1 share: the host build (tps_se.hip) and the device build (tps_se_build.hip).
#pragma once
#include <cmath>
#include <vector>
#include "common.h"

namespace mhs {

constexpr double PHI_K = 0.5 / (8.0 * M_PI);       // fields' radial constant, folded into Q

struct SeState {
    int64_t n = 0, np = 0;
    double lambda = 0;
    double sigma2 = NAN;        // sigma^2 hat (NaN without observations)
    double eff_df = NAN, rss_w = NAN;
    double *q_dev = nullptr;
    double build_ms = 0;
    int built_on = 0;           // MHS_SE_BUILD_HOST or MHS_SE_BUILD_DEVICE
};

// Q on the device (block formula above se_build in tps_se.hip): fills st, q_dev included (np x np, row-major, zero padding,
// phi's constant folded in -- what tps_se_kernel reads).  Builds on one slot run one after the other.
int se_build_device(const mhs_tps *t, SeState &st);

}  // namespace mhs
