// fbx_sim_shared.hpp -- device code that two translation units evaluate and whose results the tests pin bit for bit: the shot
// counting of the simulated experiments (fbx_tomo_sim.hip, fbx_dfe.hip) and the direct-fidelity formula (fbx_shots.hip, fbx_dfe.hip).
#pragma once
#include "fbx_common.hpp"

namespace fbx {

#ifndef FBX_TOMO_LANE_MIN_UNITS
#define FBX_TOMO_LANE_MIN_UNITS 131072           // 256 CUs x 4 SIMDs x 64 lanes x 2 wavefronts: a lane per setting fills the chip
#endif

#if defined(__HIPCC__)

// How many of the Philox blocks first, first + step, ... of the setting (g, k) hold words below t (< 2^32); the last block of a
// shot count that is no multiple of 4 counts its first n_shots & 3 words only.
__device__ __forceinline__ uint32_t tomo_count(uint32_t t, uint32_t g0, uint32_t g1, uint32_t k, uint32_t k0, uint32_t k1,
                                               uint32_t first, uint32_t step, uint32_t n_shots) {
    const uint32_t full = n_shots >> 2, tail = n_shots & 3u;
    uint32_t cnt = 0;
    for (uint32_t j = first; j < full; j += step) {
        uint32_t c[4] = {g0, g1, k, j};
        philox4x32_10(c, k0, k1);
        cnt += (uint32_t)(c[0] < t) + (uint32_t)(c[1] < t) + (uint32_t)(c[2] < t) + (uint32_t)(c[3] < t);
    }
    if (tail && full % step == first) {
        uint32_t c[4] = {g0, g1, k, full};
        philox4x32_10(c, k0, k1);
        cnt += (uint32_t)(c[0] < t) + (uint32_t)(tail > 1 && c[1] < t) + (uint32_t)(tail > 2 && c[2] < t);
    }
    return cnt;
}

// direct fidelity estimate (direct_fidelity_estimation.py:291-307) of one experiment by one wavefront: the mean of the m
// expectations and the sum of the squared standard errors, mapped to a state / average gate fidelity; d = 2^n_qubits as a double.
__device__ __forceinline__ void dfe_item(double d, int process, long long m, const double* __restrict__ e,
                                         const double* __restrict__ se, int lane, double* __restrict__ mean_out,
                                         double* __restrict__ err_out) {
    double s = 0.0, v = 0.0;
    for (long long k = lane; k < m; k += 64) { s += e[k]; const double x = se[k]; v += x * x; }
    s = wave_sum(s); v = wave_sum(v);
    if (lane == 0) {
        const double mean = s / (double)m;
        const double var_mean = v / ((double)m * (double)m);
        if (!process) {
            *mean_out = (d - 1.0) / d * mean + 1.0 / d;
            *err_out = sqrt((d - 1.0) * (d - 1.0) / (d * d) * var_mean);
        } else {
            const double d2 = d * d;
            const double p_mean = (d2 - 1.0) / d2 * mean + 1.0 / d2;
            *mean_out = (d2 * p_mean + d) / (d2 + d);
            *err_out = sqrt(d2 / ((d + 1.0) * (d + 1.0)) * (d2 - 1.0) * (d2 - 1.0) / (d2 * d2) * var_mean);
        }
    }
}

#endif

}  // namespace fbx
