// fbx_sim_shared.hpp -- code that several translation units evaluate and whose results the tests pin bit for bit: the shot
// counting of the simulated experiments (sim_*, tomo_count: fbx_tomo_sim.hip, fbx_tomo_sim_grouped.hip, fbx_tomo_sim_symm.hip,
// fbx_dfe.hip, fbx_rpe_sim.hip, fbx_rb_acquire.hip) with the host checks and staging their entry points share, the exact mean
// of a tomography setting (fbx_tomo_sim.hip, fbx_tomo_sim_grouped.hip), the direct-fidelity formula (fbx_shots.hip,
// fbx_dfe.hip), the moments of a robust-phase-estimation record (fbx_rpe.hip, fbx_rpe_sim.hip, fbx_rb_acquire.hip) and the
// outcome distribution of a measured Pauli vector (fbx_rpe_sim.hip, fbx_rb_acquire.hip).
//
// Three compare loops stay where they are, different on purpose: tomog_sim_kernel<NQ> tests `thi == 0 && tlo <= w` on
// wave-uniform operands (fbx_tomo_sim_grouped.hip); the lane forms test `live && tlo <= w` (sim_count_word below); and
// rpes_shots_kernel without records tests `tlo <= w` alone and zeroes the dead thresholds' counts afterwards (fbx_rpe_sim.hip).
#pragma once
#include "fbx_common.hpp"

namespace fbx {

inline int tomo_truth_len(const DesignDev& d) { return d.kind == FBX_KIND_PROCESS ? d.D * d.D : 2 * d.D; }

// the batch arguments of the tomography simulators; per_unit: n_shots is the total of a unit (fbx_tomo_sim_symm.hip's wording)
inline int sim_check_batch(const char* who, int64_t B, int64_t n_shots, int64_t first_item, bool per_unit = false) {
    const std::string w(who);
    FBX_REQUIRE(B >= 0 && n_shots >= 0 && first_item >= 0,
                w + (per_unit ? ": need B >= 0, shots >= 0 and first_item >= 0" : ": need B >= 0, n_shots >= 0 and first_item >= 0"));
    FBX_REQUIRE(n_shots < ((int64_t)1 << 32), w + (per_unit ? ": the shots of a unit must be below 2^32" : ": n_shots must be below 2^32"));
    FBX_REQUIRE(B <= INT64_MAX / 65536 / 4096, w + ": B * m overflows");
    return FBX_OK;
}

// the outputs every simulator has, reserved through `io`: four of [units] doubles and the status [B]; NULL stays NULL
struct SimOut {
    double *expect, *counts, *std_err, *exact;
    int32_t* status;
    int stage(HostIO& io, size_t B, size_t units, double* h_expect, double* h_counts, double* h_std_err, double* h_exact,
              int32_t* h_status) {
        FBX_TRY(io.out_opt(h_expect, units, &expect));
        FBX_TRY(io.out_opt(h_counts, units, &counts));
        FBX_TRY(io.out_opt(h_std_err, units, &std_err));
        FBX_TRY(io.out_opt(h_exact, units, &exact));
        return io.out_opt(h_status, B, &status);
    }
};

// status[b] = 1 when item b has a non-finite truth entry or a flip probability outside [0, 1] (NaN included), else 0: one launch
// on the calling thread's stream (fbx_tomo_sim.hip); d_flips may be NULL
int tomo_poison_launch(int64_t B, int truth_len, int flip_len, const double* d_truth, const double* d_flips, int32_t* d_status);

#ifndef FBX_TOMO_LANE_MIN_UNITS
#define FBX_TOMO_LANE_MIN_UNITS 131072           // 256 CUs x 4 SIMDs x 64 lanes x 2 wavefronts: a lane per setting fills the chip
#endif

#if defined(__HIPCC__)

// The shots of one unit: f(word, shot) for the words of the Philox blocks first, first + step, ... of counter {g0, g1, g2, j}
// under the key (k0, k1), four shots a block.  The last block of a shot count that is no multiple of 4 gives its first
// n_shots & 3 words only and belongs to the walker with full % step == first.  (first, step) = (0, 1): one lane draws every
// shot; (lane, 64): a wavefront shares them.  Every simulator draws through this loop but toms_kernel (fbx_tomo_sim_symm.hip,
// which flattens (pattern, block) pairs over the lanes) and tomog_sim_lane_kernel (fbx_tomo_sim_grouped.hip: the same loop
// spelled out, because it measured 0.9 % slower through here).
template <class F>
__device__ __forceinline__ void sim_walk(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t k0, uint32_t k1, uint32_t first,
                                         uint32_t step, uint32_t n_shots, F&& f) {
    const uint32_t full = n_shots >> 2, tail = n_shots & 3u;
    for (uint32_t j = first; j < full; j += step) {
        uint32_t c[4] = {g0, g1, g2, j};
        philox4x32_10(c, k0, k1);
        f(c[0], 4 * j); f(c[1], 4 * j + 1); f(c[2], 4 * j + 2); f(c[3], 4 * j + 3);
    }
    if (tail && full % step == first) {
        uint32_t c[4] = {g0, g1, g2, full};
        philox4x32_10(c, k0, k1);
        f(c[0], 4 * full);
        if (tail > 1) f(c[1], 4 * full + 1);
        if (tail > 2) f(c[2], 4 * full + 2);
    }
}

// How many of those words of the setting (g, k) are below t (< 2^32)
__device__ __forceinline__ uint32_t tomo_count(uint32_t t, uint32_t g0, uint32_t g1, uint32_t k, uint32_t k0, uint32_t k1,
                                               uint32_t first, uint32_t step, uint32_t n_shots) {
    uint32_t cnt = 0;
    sim_walk(g0, g1, k, k0, k1, first, step, n_shots, [&](uint32_t w, uint32_t) { cnt += (uint32_t)(w < t); });
    return cnt;
}

// k_plus of N shots gave +1 -> the mean of the +-1 values times coef, N, and the standard error of that mean
// (fbx_dfe.hip calls it with coef = +-1: the product with |coef| is exact)
__device__ __forceinline__ void sim_write_pm1(double* __restrict__ expect, double* __restrict__ counts, double* __restrict__ std_err,
                                              long long out, double coef, unsigned long long k_plus, unsigned long long N) {
    const unsigned long long k_minus = N - k_plus;
    const double nd = (double)N;
    if (expect) expect[out] = coef * ((double)((long long)k_plus - (long long)k_minus) / nd);
    if (counts) counts[out] = nd;
    if (std_err) std_err[out] = fabs(coef) * sqrt((double)(k_plus * k_minus) * 4.0 / nd) / nd;
}

// ... and the same cells of a poisoned item: NaN, NaN, NaN and N
__device__ __forceinline__ void sim_write_poisoned(double* __restrict__ expect, double* __restrict__ counts, double* __restrict__ std_err,
                                                   double* __restrict__ exact, long long out, unsigned long long N) {
    const double nan = __builtin_nan("");
    if (expect) expect[out] = nan;
    if (std_err) std_err[out] = nan;
    if (exact) exact[out] = nan;
    if (counts) counts[out] = (double)N;
}

// One +-1 observable of mean mu (item gid, setting k, cell `out`), everything below the mean of tomo_sim_kernel and
// dfe_sim_kernel: the exact value, the threshold floor(q 2^32) of q = (1 + mu) / 2 clamped to [0, 1], the count of the words
// below it and the outputs.  LANE: the calling lane has the unit to itself; else its wavefront shares the shots and lane 0 writes.
template <bool LANE>
__device__ __forceinline__ void sim_bernoulli_unit(double mu, double coef, unsigned long long gid, uint32_t k, uint32_t k0, uint32_t k1,
                                                   int lane, unsigned n_shots, long long out, double* __restrict__ expect_out,
                                                   double* __restrict__ counts_out, double* __restrict__ std_err_out,
                                                   double* __restrict__ exact_out) {
    if (exact_out && (LANE || lane == 0)) exact_out[out] = coef * mu;
    if (n_shots == 0) return;
    double q = 0.5 * mu + 0.5;
    q = fmin(fmax(q, 0.0), 1.0);
    const unsigned long long t = (unsigned long long)(q * 0x1p32);
    unsigned long long k_plus;
    if (t >> 32) {
        k_plus = n_shots;                                       // every word is below 2^32: no draws
    } else if (t == 0) {
        k_plus = 0;
    } else if constexpr (LANE) {
        k_plus = tomo_count((uint32_t)t, (uint32_t)gid, (uint32_t)(gid >> 32), k, k0, k1, 0u, 1u, n_shots);
    } else {
        const uint32_t part = tomo_count((uint32_t)t, (uint32_t)gid, (uint32_t)(gid >> 32), k, k0, k1, (uint32_t)lane, 64u, n_shots);
        k_plus = (unsigned long long)wave_sum((double)part);    // integers below 2^32: the sum is exact
    }
    if (!LANE && lane != 0) return;
    sim_write_pm1(expect_out, counts_out, std_err_out, out, coef, k_plus, n_shots);
}

// Outcome o of M has the words in [thr[o - 1], thr[o]), thr[o] = floor(c[o] / c[M - 1] 2^32) from the running sums c of the
// clamped probabilities.  A counter holds tlo = the low word of each threshold, live = "it is below 2^32" (one of 2^32 is
// reached by no word) and reach[o] = the words seen with thr[o] <= word, i.e. with an outcome above o.
template <int M>
__device__ __forceinline__ void sim_thresholds(const double (&c)[M], uint32_t (&tlo)[M - 1], bool (&live)[M - 1], uint32_t (&reach)[M - 1]) {
#pragma unroll
    for (int o = 0; o < M - 1; ++o) {
        const unsigned long long t = (unsigned long long)(c[o] / c[M - 1] * 0x1p32);
        tlo[o] = (uint32_t)t; live[o] = (t >> 32) == 0; reach[o] = 0u;
    }
}

// one word into reach[]; returns its outcome
template <int M>
__device__ __forceinline__ int sim_count_word(uint32_t w, const uint32_t (&tlo)[M - 1], const bool (&live)[M - 1], uint32_t (&reach)[M - 1]) {
    int o = 0;
#pragma unroll
    for (int i = 0; i < M - 1; ++i) { const int hit = live[i] && tlo[i] <= w; reach[i] += (uint32_t)hit; o += hit; }
    return o;
}

// reach[] -> the histogram of n_shots shots.  LANE: reach is the calling lane's own; else the wavefront's lanes hold partial
// counts, which are summed (integers below 2^32: exactly, in double) and every lane gets the histogram.
template <int M, bool LANE>
__device__ __forceinline__ void sim_histogram(const uint32_t (&reach)[M - 1], uint32_t n_shots, uint32_t (&hist)[M]) {
    uint32_t above = n_shots;                                   // shots with outcome >= o
#pragma unroll
    for (int o = 0; o < M - 1; ++o) {
        const uint32_t next = LANE ? reach[o] : (uint32_t)wave_sum((double)reach[o]);
        hist[o] = above - next; above = next;
    }
    hist[M - 1] = above;
}

// The other way to a histogram, for many outcomes: every lane increments PRIVATE counters cnt[o * 64 + lane] in LDS (the lane
// is the bank) and lane o < d sums row o here, starting at its own column so that the lanes read different banks.
__device__ __forceinline__ void sim_column_sum(const uint32_t* cnt, int d, int lane, uint32_t* hist) {
    if (lane < d) {
        uint32_t h = 0;
        for (int l = 0; l < 64; ++l) h += cnt[lane * 64 + ((l + lane) & 63)];
        hist[lane] = h;
    }
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

// ... and of the simulators that measure a final Pauli vector (fbx_rpe_sim.hip, fbx_rb_acquire.hip)
__device__ __forceinline__ bool rpes_finite(double v) { return fabs(v) < __builtin_inf(); }              // false for NaN
__device__ __forceinline__ bool rpes_bad_total(double c) { return !(c > 0.0 && c < __builtin_inf()); }   // NaN included

// The outcome distribution of one basis at one depth from four components of the final Pauli vector: vI the identity (1 for a
// trace-preserving map), vP = <P_a>, vZ = <Z_b>, vPZ = <P_a Z_b>.  Outcome o = 2 s + t with a partner, o = s without.  fa / fb:
// the flips of the xy qubit / the partner, or NULL.  Returns the clamped sum.
template <bool PARTNER>
__device__ __forceinline__ double rpes_distribution(double vI, double vP, double vZ, double vPZ, const double* __restrict__ fa,
                                                    const double* __restrict__ fb, double (&p)[4]) {
    if constexpr (PARTNER) {
        const double a = vI + vP, b = vI - vP;
        p[0] = ((a + vZ) + vPZ) * 0.25; p[1] = ((a - vZ) - vPZ) * 0.25;
        p[2] = ((b + vZ) - vPZ) * 0.25; p[3] = ((b - vZ) + vPZ) * 0.25;
        if (fa) {
            const double f0 = fa[0], f1 = fa[1], g0 = fb[0], g1 = fb[1];
#pragma unroll
            for (int t = 0; t < 2; ++t) {                     // the bit s: pairs (t, 2 + t)
                const double x = p[t], y = p[2 + t];
                p[t] = fma(1.0 - f0, x, f1 * y); p[2 + t] = fma(1.0 - f1, y, f0 * x);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {                     // the bit t: pairs (2 s, 2 s + 1)
                const double x = p[2 * s], y = p[2 * s + 1];
                p[2 * s] = fma(1.0 - g0, x, g1 * y); p[2 * s + 1] = fma(1.0 - g1, y, g0 * x);
            }
        }
    } else {
        p[0] = (vI + vP) * 0.5; p[1] = (vI - vP) * 0.5; p[2] = 0.0; p[3] = 0.0;
        if (fa) {
            const double f0 = fa[0], f1 = fa[1], x = p[0], y = p[1];
            p[0] = fma(1.0 - f0, x, f1 * y); p[1] = fma(1.0 - f1, y, f0 * x);
        }
    }
    double run = 0.0;
#pragma unroll
    for (int o = 0; o < (PARTNER ? 4 : 2); ++o) run += p[o] < 0.0 ? 0.0 : p[o];
    return run;
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
