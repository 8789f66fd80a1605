// fbx_sim_shared.hpp -- device code that two translation units evaluate and whose results the tests pin bit for bit: the shot
// counting of the simulated experiments (fbx_tomo_sim.hip, fbx_dfe.hip), the exact mean of a tomography setting (fbx_tomo_sim.hip,
// fbx_tomo_sim_grouped.hip), the direct-fidelity formula (fbx_shots.hip, fbx_dfe.hip) and the moments of a robust-phase-estimation
// record (fbx_rpe.hip, fbx_rpe_sim.hip).
#pragma once
#include "fbx_common.hpp"

namespace fbx {

// status[b] = 1 when item b has a non-finite truth entry or a flip probability outside [0, 1] (NaN included), else 0: one launch
// on the calling thread's stream (fbx_tomo_sim.hip); d_flips may be NULL
int tomo_poison_launch(int64_t B, int truth_len, int flip_len, const double* d_truth, const double* d_flips, int32_t* d_status);

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

__device__ __forceinline__ bool tomo_bad_probability(double v) { return !(v >= 0.0 && v <= 1.0); }      // NaN included

// tr[P rho] of the Pauli with index `pidx` (base-4 digits, qubit 0 most significant): P = i^ny X^x Z^z, P |c> = i^ny (-1)^{|c & z|} |c ^ x>
__device__ __forceinline__ double tomo_trace_state(const cplx* __restrict__ rho, int n, int pidx) {
    int x = 0, z = 0, ny = 0;
    for (int t = 0; t < n; ++t) {
        const int code = (pidx >> (2 * t)) & 3;
        x |= ((code == 1) | (code == 2)) << t; z |= ((code == 2) | (code == 3)) << t; ny += code == 2;
    }
    const int d = 1 << n;
    double acc = 0.0;
    for (int c = 0; c < d; ++c) {
        const cplx v = rho[c * d + (c ^ x)];
        double term = (ny & 1) ? v.im : v.re;               // Re(i^ny v): re, -im, -re, im
        if (((ny + 1) >> 1) & 1) term = -term;
        acc += (__popc(c & z) & 1) ? -term : term;
    }
    return acc;
}

// tr[P Lambda(rho_s)] = sum_j R[P][j] c_j(s): row `pidx` of the transfer matrix against the state's Bloch coefficients
__device__ __forceinline__ double tomo_trace_process(const double* __restrict__ R, const double* __restrict__ ct, int D, int pidx) {
    const double* row = R + (size_t)pidx * D;
    double acc = 0.0;
    for (int j = 0; j < D; ++j) acc = fma(row[j], ct[j], acc);
    return acc;
}

// The mean of the measured +-1 product of the setting with the packed (state, Pauli) `sp` (include/fbx.h): over the subsets T
// of the Pauli's support, prod_{S \ T} a_j prod_T b_j tr[P_T .]; without flips a = 0 and b = 1, and only T = S is left.
__device__ inline double tomo_mean(const DesignDev& des, const double* __restrict__ truth, const double* __restrict__ flip, uint32_t sp) {
    const int n = des.n, pidx = (int)(sp & 0xFFFFu), s = (int)(sp >> 16);
    int support = 0;
    double a[5], bb[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {                             // (fixed bounds: a and bb stay in registers)
        if (t >= n) { a[t] = 0.0; bb[t] = 1.0; continue; }
        if ((pidx >> (2 * t)) & 3) support |= 1 << t;
        const int q = n - 1 - t;                              // digit t belongs to qubit n - 1 - t
        const double f0 = flip ? flip[2 * q] : 0.0, f1 = flip ? flip[2 * q + 1] : 0.0;
        a[t] = f1 - f0; bb[t] = 1.0 - f0 - f1;
    }
    if (support == 0) return 1.0;
    const double* ct = des.Ct + (size_t)s * des.D;
    double mu = 0.0;
    for (int T = support;; T = (T - 1) & support) {
        double w = 1.0;
        int keep = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            if (!((support >> t) & 1)) continue;
            if ((T >> t) & 1) { w *= bb[t]; keep |= 3 << (2 * t); } else { w *= a[t]; }
        }
        if (w != 0.0) {
            const double tr = T == 0 ? 1.0
                            : des.kind == FBX_KIND_PROCESS ? tomo_trace_process(truth, ct, des.D, pidx & keep)
                                                           : tomo_trace_state(reinterpret_cast<const cplx*>(truth), n, pidx & keep);
            mu = fma(w, tr, mu);
        }
        if (T == 0) break;
    }
    return mu;
}

// counts of -1 outcomes -> mean of the +-1 values and the variance of that mean, fbx_shots_to_moments' formulas with coef = 1
// (fbx_rpe.hip from measured records, fbx_rpe_sim.hip from simulated ones)
__device__ __forceinline__ void rpe_moment(long long n_minus, long long n_shots, double& mean, double& var) {
#pragma clang fp contract(off)
    const long long n_plus = n_shots - n_minus;
    const double m = ((double)n_plus - (double)n_minus) / (double)n_shots;
    mean = m;
    var = (1.0 - m * m) / (double)n_shots;
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
