// fbx_rpe_sim.hip -- simulated robust phase estimation (fbx_rpe_simulate): from a noisy gate, given as a Pauli transfer matrix,
// to the shot counts, moments and bit records of an RPE experiment -- the acquisition half the reference gets from a QVM
// (generate_rpe_experiments + acquire_rpe_data, robust_phase_estimation.py:152-307).
//
// Two launches per call.
//   rpes_dist_kernel   the distributions.  Depth 2^j is j squarings of the gate's matrix, so depth j reuses depth j - 1 and all
//                      62 depths of the analysis cost 61 small matrix products.  One qubit (4 x 4): a LANE takes an item and
//                      keeps the matrix in registers.  Two qubits (16 x 16): a WAVEFRONT takes an item, the matrix lies in the
//                      wavefront's 2 KiB of LDS and every lane owns a 2 x 2 block of the square.  Per depth the final Pauli
//                      vector v = meas G^(2^j) prep init gives, per basis (X, Y), the M = 2 or 4 outcome probabilities with the
//                      readout flips folded in; they go to prob_out (or a scratch block).  This kernel also decides the item's
//                      status -- non-finite input, a flip outside [0, 1], a distribution whose clamped sum is not a positive
//                      finite number -- and overwrites what it wrote for a poisoned item with NaN.
//   rpes_shots_kernel  the shots, the hot path: a unit is (item, depth, basis); it reads its M probabilities back, forms the
//                      thresholds and counts Philox words as fbx_tomo_simulate_grouped does.  Two work splits, chosen by the
//                      number of units alone: below FBX_RPE_SIM_LANE_MIN_UNITS a wavefront takes a unit (lane l draws the
//                      blocks l, l + 64, ..., the partial counts are summed exactly), from there on a lane takes a unit and
//                      draws all its blocks; the lane form orders its units depth-major, so that the lanes of a wavefront
//                      share a shot count when the schedule depends on the depth.  Both read the same stored probabilities and
//                      count the same words: a value depends on (seed, item id, depth, basis, distribution, shots) only.
//                      The walk, the thresholds and the histogram step are those of fbx_sim_shared.hpp; without records the
//                      kernel keeps its own compare (`tlo <= w` alone, the dead thresholds' counts zeroed after the walk).
// The cost is the Philox blocks: n_shots / 4 blocks of about a hundred integer instructions per unit against a few dozen
// fused multiply-adds per depth for the distributions.
#include "fbx_sim_shared.hpp"      // rpe_moment, shared with fbx_rpe.hip: the moments of both come from one formula

#ifndef FBX_RPE_SIM_LANE_MIN_UNITS
#define FBX_RPE_SIM_LANE_MIN_UNITS 131072        // as FBX_TOMO_LANE_MIN_UNITS: from here on a lane per (item, depth, basis) fills the chip
#endif

namespace fbx {

constexpr int RPES_THREADS = 256, RPES_WAVES = RPES_THREADS / 64;
constexpr int RPES_MAX_DEPTHS = 62;              // as fbx_rpe_phase: depth 2^j must stay an exact integer
constexpr uint32_t RPES_KEY_TAG = 0x52504553u;   // "RPES": keeps the stream apart from the tomography simulators' under one seed

struct RpeSimIn {
    long long B;
    int K, n, per_item;                          // per_item: prep and meas are [B][D][D]
    int iP[2], iZ, iPZ[2];                       // Pauli indices of X / Y on the xy qubit, Z on the partner and their products
    int xy, zq;                                  // zq < 0: no partner
    const double *gate, *prep, *meas, *init, *flips;
};
struct RpeSimSchedule { int32_t n[RPES_MAX_DEPTHS]; };

// ------------------------------------------------------------------------------------------------ distributions, one qubit
// a lane per item: 4 x 4 matrices in registers, every row product one chain of fused multiply-adds in ascending column order
__device__ __forceinline__ void rpes_matvec4(const double (&A)[16], const double (&x)[4], double (&y)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fma(A[4 * r + k], x[k], acc);
        y[r] = acc;
    }
}

__global__ void __launch_bounds__(RPES_THREADS)
rpes_dist1_kernel(RpeSimIn in, double* __restrict__ prob, int* __restrict__ status) {
    const long long b = (long long)blockIdx.x * RPES_THREADS + threadIdx.x;
    if (b >= in.B) return;
    const int K = in.K;
    const double nan = __builtin_nan("");
    double* pb = prob + b * K * 4;                             // [K][2][2]
    bool bad = false;
    double A[16], Mm[16], w[4], u[4], v[4];
#pragma unroll
    for (int e = 0; e < 16; ++e) { A[e] = in.gate[b * 16 + e]; bad |= !rpes_finite(A[e]); }
#pragma unroll
    for (int e = 0; e < 4; ++e) { w[e] = in.init ? in.init[e] : (e < 2 ? 1.0 : 0.0); bad |= !rpes_finite(w[e]); }   // NULL: |+>
    if (in.prep) {
        const double* P = in.prep + (in.per_item ? b * 16 : 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) { Mm[e] = P[e]; bad |= !rpes_finite(Mm[e]); }
        rpes_matvec4(Mm, w, u);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = u[e];
    }
    if (in.meas) {
        const double* P = in.meas + (in.per_item ? b * 16 : 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) { Mm[e] = P[e]; bad |= !rpes_finite(Mm[e]); }
    }
    const double* fa = in.flips ? in.flips + b * 2 : nullptr;
    if (fa) bad |= tomo_bad_probability(fa[0]) || tomo_bad_probability(fa[1]);
    if (!bad) {
        for (int j = 0; j < K; ++j) {
            rpes_matvec4(A, w, u);
            if (in.meas) rpes_matvec4(Mm, u, v);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = u[e];
            }
#pragma unroll
            for (int basis = 0; basis < 2; ++basis) {
                double p[4];
                bad |= rpes_bad_total(rpes_distribution<false>(v[0], v[1 + basis], 0.0, 0.0, fa, nullptr, p));
                pb[j * 4 + basis * 2] = p[0]; pb[j * 4 + basis * 2 + 1] = p[1];
            }
            if (j + 1 < K) {
                double T[16];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc = fma(A[4 * r + k], A[4 * k + c], acc);
                        T[4 * r + c] = acc;
                    }
#pragma unroll
                for (int e = 0; e < 16; ++e) A[e] = T[e];
            }
        }
    }
    if (bad)
        for (int e = 0; e < K * 4; ++e) pb[e] = nan;           // (the lane that wrote them: program order)
    status[b] = bad ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ distributions, two qubits
// a wavefront per item: the 16 x 16 matrix in the wavefront's own LDS, lane l owns the 2 x 2 block (l / 8, l % 8) of the square
// (per k two row entries and two neighbouring column entries feed four chains: half the LDS bytes of an entry per lane and
// step); rows are RPES_LD = 17 doubles apart, so that neither the eight row addresses of such a read nor the sixteen of a
// matrix-vector row share a bank.  The vectors w = prep init, u = G^(2^j) w and v = meas u are 16 lanes wide.  One wavefront
// touches its slice only and its LDS instructions run in program order, so the phases need no barrier (FBX_WAVE_SYNC).
constexpr int RPES_LD = 17;
template <bool PARTNER>
__global__ void __launch_bounds__(RPES_THREADS)
rpes_dist2_kernel(RpeSimIn in, double* __restrict__ prob, int* __restrict__ status) {
    constexpr int M = PARTNER ? 4 : 2;
    __shared__ double A_all[RPES_WAVES][16 * RPES_LD];
    __shared__ double vec_all[RPES_WAVES][48];                 // w | u | v
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * RPES_WAVES + uniform(wave);
    if (b >= in.B) return;
    const int K = in.K;
    const double nan = __builtin_nan("");
    double* A = A_all[wave];
    double* vec = vec_all[wave];
    double* pb = prob + b * K * 2 * M;                          // [K][2][M]
    const double* G = in.gate + b * 256;
    const double* Pp = in.prep ? in.prep + (in.per_item ? b * 256 : 0) : nullptr;
    const double* Pm = in.meas ? in.meas + (in.per_item ? b * 256 : 0) : nullptr;
    const double* fl = in.flips ? in.flips + b * 4 : nullptr;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane + 64 * i;
        const double x = G[e];
        A[(e >> 4) * RPES_LD + (e & 15)] = x; bad |= !rpes_finite(x);
        if (Pp) bad |= !rpes_finite(Pp[e]);
        if (Pm) bad |= !rpes_finite(Pm[e]);
    }
    if (lane < 16) {
        int only_ix = 1;                                        // NULL init: |+>|+>, 1 on the products of I and X
#pragma unroll
        for (int t = 0; t < 2; ++t) only_ix &= ((lane >> (2 * t)) & 3) < 2;
        const double x = in.init ? in.init[lane] : (double)only_ix;
        vec[lane] = x; bad |= !rpes_finite(x);
    }
    if (fl && lane < 4) bad |= tomo_bad_probability(fl[lane]);
    bool any_bad = __ballot(bad) != 0ull;
    FBX_WAVE_SYNC();
    if (!any_bad) {
        if (Pp) {
            double acc = 0.0;
            if (lane < 16)
                for (int k = 0; k < 16; ++k) acc = fma(Pp[lane * 16 + k], vec[k], acc);
            FBX_WAVE_SYNC();
            if (lane < 16) vec[lane] = acc;
            FBX_WAVE_SYNC();
        }
        for (int j = 0; j < K; ++j) {
            if (lane < 16) {
                double acc = 0.0;
                for (int k = 0; k < 16; ++k) acc = fma(A[lane * RPES_LD + k], vec[k], acc);
                vec[16 + lane] = acc;
            }
            FBX_WAVE_SYNC();
            if (lane < 16) {
                double acc = vec[16 + lane];
                if (Pm) {
                    acc = 0.0;
                    for (int k = 0; k < 16; ++k) acc = fma(Pm[lane * 16 + k], vec[16 + k], acc);
                }
                vec[32 + lane] = acc;
            }
            FBX_WAVE_SYNC();
            bool bad_unit = false;
            if (lane < 2) {                                     // lane = basis
                const double* v = vec + 32;
                double p[4];
                const double total = rpes_distribution<PARTNER>(v[0], v[in.iP[lane]], PARTNER ? v[in.iZ] : 0.0,
                                                                PARTNER ? v[in.iPZ[lane]] : 0.0, fl ? fl + 2 * in.xy : nullptr,
                                                                fl && PARTNER ? fl + 2 * in.zq : nullptr, p);
                bad_unit = rpes_bad_total(total);
#pragma unroll
                for (int o = 0; o < M; ++o) pb[(j * 2 + lane) * M + o] = p[o];
            }
            any_bad |= __ballot(bad_unit) != 0ull;
            if (j + 1 < K) {
                const int r0 = 2 * (lane >> 3), c0 = 2 * (lane & 7);
                double t00 = 0.0, t01 = 0.0, t10 = 0.0, t11 = 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const double a0 = A[r0 * RPES_LD + k], a1 = A[(r0 + 1) * RPES_LD + k];
                    const double b0 = A[k * RPES_LD + c0], b1 = A[k * RPES_LD + c0 + 1];
                    t00 = fma(a0, b0, t00); t01 = fma(a0, b1, t01); t10 = fma(a1, b0, t10); t11 = fma(a1, b1, t11);
                }
                FBX_WAVE_SYNC();                                // every read of A is ahead of the writes
                A[r0 * RPES_LD + c0] = t00; A[r0 * RPES_LD + c0 + 1] = t01;
                A[(r0 + 1) * RPES_LD + c0] = t10; A[(r0 + 1) * RPES_LD + c0 + 1] = t11;
                FBX_WAVE_SYNC();
            }
        }
    }
    if (any_bad && lane < 2)                                    // (the lane that wrote a cell overwrites it: program order)
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int o = 0; o < M; ++o) pb[(j * 2 + lane) * M + o] = nan;
    if (lane == 0) status[b] = any_bad ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ shots
// unit (item b, depth j, basis): histogram, moments and, when asked for, the record of its shots.  LANE: a lane per unit, units
// ordered depth-major; else a wavefront per unit, units ordered item-major.  REC: the bit records are written, which needs the
// outcome of every word; without them a word is only compared with the thresholds (one compare and one add each), and a
// threshold of 2^32, which no word reaches, is sorted out after the loop.
template <bool LANE, bool PARTNER, bool REC>
__global__ void __launch_bounds__(RPES_THREADS)
rpes_shots_kernel(long long B, int K, int n, int xy, int zq, RpeSimSchedule sched, unsigned long long seed, long long first_item,
                  const double* __restrict__ prob, const int* __restrict__ status, uint32_t* __restrict__ hist_out,
                  double* __restrict__ moments_out, uint8_t* __restrict__ x_bits_out, uint8_t* __restrict__ y_bits_out) {
    constexpr int M = PARTNER ? 4 : 2;
    const int lane = threadIdx.x & 63;
    long long b;
    int j, basis;
    if constexpr (LANE) {
        const long long u = (long long)blockIdx.x * RPES_THREADS + threadIdx.x;
        if (u >= B * K * 2) return;
        j = (int)(u / (2 * B));
        const long long r = u - (long long)j * 2 * B;
        b = r >> 1; basis = (int)(r & 1);
    } else {
        const long long u = (long long)blockIdx.x * RPES_WAVES + uniform((int)(threadIdx.x >> 6));
        if (u >= B * K * 2) return;
        b = u / (2 * K);
        const int r = (int)(u - b * 2 * K);
        j = r >> 1; basis = r & 1;
    }
    const uint32_t N = (uint32_t)sched.n[j];
    const long long unit = (b * K + j) * 2 + basis, plane = B * K, at = b * K + j;
    uint8_t* rec = REC ? (basis ? y_bits_out : x_bits_out) : nullptr;
    if (rec) rec += (b * K + j) * (long long)N * n;             // (records: every depth has N shots; one of the two may be NULL)
    const uint32_t first = LANE ? 0u : (uint32_t)lane, step = LANE ? 1u : 64u;
    const bool writer = LANE || lane == 0;
    if (status[b]) {
        const double nan = __builtin_nan("");
        if (writer) {
            if (hist_out) {
#pragma unroll
                for (int o = 0; o < M; ++o) hist_out[unit * M + o] = 0u;
            }
            if (moments_out) {
#pragma unroll
                for (int q = 0; q < 4; ++q) moments_out[(2 * q + basis) * plane + at] = nan;
            }
        }
        if (rec)
            for (long long i = first; i < (long long)N * n; i += step) rec[i] = 0;
        return;
    }
    double run = 0.0, c[M];
#pragma unroll
    for (int o = 0; o < M; ++o) { const double p = prob[unit * M + o]; run += p < 0.0 ? 0.0 : p; c[o] = run; }
    uint32_t tlo[M - 1], reach[M - 1];
    bool live[M - 1];
    sim_thresholds<M>(c, tlo, live, reach);
    const unsigned long long gid = (unsigned long long)(first_item + b);
    const uint32_t g0 = (uint32_t)gid, g1 = (uint32_t)(gid >> 32), g2 = (uint32_t)(2 * j + basis);
    const uint32_t k0 = (uint32_t)seed ^ RPES_KEY_TAG, k1 = (uint32_t)(seed >> 32);
    sim_walk(g0, g1, g2, k0, k1, first, step, N, [&](uint32_t w, uint32_t shot) {
        if constexpr (REC) {
            const int o = sim_count_word<M>(w, tlo, live, reach);
            if (rec) {
                const int s = PARTNER ? o >> 1 : o, t = o & 1;
                for (int q = 0; q < n; ++q) rec[(long long)shot * n + q] = (uint8_t)(q == xy ? s : (PARTNER && q == zq) ? t : 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < M - 1; ++i) reach[i] += (uint32_t)(tlo[i] <= w);
        }
    });
    if constexpr (!REC) {
#pragma unroll
        for (int i = 0; i < M - 1; ++i) reach[i] = live[i] ? reach[i] : 0u;
    }
    uint32_t hist[M];
    sim_histogram<M, LANE>(reach, N, hist);
    if (!writer) return;
    if (hist_out) {
#pragma unroll
        for (int o = 0; o < M; ++o) hist_out[unit * M + o] = hist[o];
    }
    if (moments_out) {
        double mean, var;
        rpe_moment(PARTNER ? (long long)hist[2] + hist[3] : (long long)hist[1], (long long)N, mean, var);       // s = 1
        moments_out[basis * plane + at] = mean; moments_out[(4 + basis) * plane + at] = var;
        if constexpr (PARTNER) rpe_moment((long long)hist[1] + hist[2], (long long)N, mean, var);                // s ^ t = 1
        else { mean = __builtin_nan(""); var = mean; }
        moments_out[(2 + basis) * plane + at] = mean; moments_out[(6 + basis) * plane + at] = var;
    }
}

// uniform_shots: the common shot count, or -1 when the schedule is ragged
static int rpes_check(int n_qubits, int64_t B, int K, const void* gate, int xy_qubit, int z_qubit, const int32_t* n_shots,
                      int64_t first_item, const void* prob, const void* hist, const void* moments, const void* x_bits,
                      const void* y_bits, const void* status, int64_t* uniform_shots) {
    FBX_REQUIRE(n_qubits >= 1, "fbx_rpe_simulate: n_qubits must be 1 or 2");
    if (n_qubits > 2) {
        set_error("fbx_rpe_simulate: gates of 1 and 2 qubits are simulated (got " + std::to_string(n_qubits) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_REQUIRE(B >= 0 && K >= 1 && first_item >= 0, "fbx_rpe_simulate: need B >= 0, K >= 1 and first_item >= 0");
    if (K > RPES_MAX_DEPTHS) {
        set_error("fbx_rpe_simulate: at most 62 depths (depth 2^j must stay an exact integer; got " + std::to_string(K) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_REQUIRE(B == 0 || gate != nullptr, "fbx_rpe_simulate: NULL gate_ptm");
    FBX_REQUIRE(xy_qubit >= 0 && xy_qubit < n_qubits, "fbx_rpe_simulate: xy_qubit must be a qubit of the gate");
    FBX_REQUIRE(z_qubit >= -1 && z_qubit < n_qubits && z_qubit != xy_qubit,
                "fbx_rpe_simulate: z_qubit must be -1 or another qubit of the gate");
    FBX_REQUIRE(n_shots != nullptr, "fbx_rpe_simulate: NULL n_shots");
    int64_t same = n_shots[0];
    for (int j = 0; j < K; ++j) {
        FBX_REQUIRE(n_shots[j] >= 1, "fbx_rpe_simulate: every entry of n_shots must be at least 1");
        if (n_shots[j] != n_shots[0]) same = -1;
    }
    FBX_REQUIRE(prob || hist || moments || x_bits || y_bits || status, "fbx_rpe_simulate: every output is NULL");
    FBX_REQUIRE(same > 0 || !(x_bits || y_bits),
                "fbx_rpe_simulate: bit records need the same number of shots at every depth (ragged records are not written)");
    FBX_REQUIRE(B <= (INT64_MAX >> 24) / (same > 0 ? same : 1), "fbx_rpe_simulate: B * K * n_shots overflows");
    *uniform_shots = same;
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_rpe_simulate_dev(int n_qubits, int64_t B, int K, const double* d_gate_ptm, const double* d_prep_ptm,
                         const double* d_meas_ptm, int basis_per_item, const double* d_init, int xy_qubit, int z_qubit,
                         const double* d_flips, const int32_t* n_shots, uint64_t seed, int64_t first_item, double* d_prob_out,
                         uint32_t* d_hist_out, double* d_moments_out, uint8_t* d_x_bits_out, uint8_t* d_y_bits_out,
                         int32_t* d_status_out) {
    int64_t uniform_shots = -1;
    FBX_TRY(rpes_check(n_qubits, B, K, d_gate_ptm, xy_qubit, z_qubit, n_shots, first_item, d_prob_out, d_hist_out, d_moments_out,
                       d_x_bits_out, d_y_bits_out, d_status_out, &uniform_shots));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const bool partner = z_qubit >= 0;
    const int M = partner ? 4 : 2;
    const int64_t units = B * K * 2;
    const bool lane = units >= FBX_RPE_SIM_LANE_MIN_UNITS;
    const int64_t dist_blocks = n_qubits == 1 ? (B + RPES_THREADS - 1) / RPES_THREADS : (B + RPES_WAVES - 1) / RPES_WAVES;
    const int64_t per_block = lane ? RPES_THREADS : RPES_WAVES, blocks = (units + per_block - 1) / per_block;
    FBX_REQUIRE(dist_blocks < ((int64_t)1 << 31) && blocks < ((int64_t)1 << 31),
                "fbx_rpe_simulate: B * K is beyond one launch; cut the batch with first_item");
    DevBuf scratch_prob;                             // the distributions when the caller does not want them (stream order protects them)
    double* prob = d_prob_out;
    if (!prob) { FBX_TRY(scratch_prob.alloc(sizeof(double) * (size_t)units * M)); prob = scratch_prob.as<double>(); }
    StatusBuf status_buf;
    FBX_TRY(status_buf.take(d_status_out, B));
    int32_t* status = status_buf.p;
    RpeSimIn in{};
    in.B = B; in.K = K; in.n = n_qubits; in.per_item = basis_per_item ? 1 : 0;
    in.xy = xy_qubit; in.zq = z_qubit;
    const int sh_xy = 2 * (n_qubits - 1 - xy_qubit), sh_z = partner ? 2 * (n_qubits - 1 - z_qubit) : 0;   // qubit 0 most significant
    in.iZ = partner ? 3 << sh_z : 0;
    for (int basis = 0; basis < 2; ++basis) { in.iP[basis] = (1 + basis) << sh_xy; in.iPZ[basis] = in.iP[basis] | in.iZ; }
    in.gate = d_gate_ptm; in.prep = d_prep_ptm; in.meas = d_meas_ptm; in.init = d_init; in.flips = d_flips;
    if (n_qubits == 1)
        hipLaunchKernelGGL(rpes_dist1_kernel, dim3((unsigned)dist_blocks), dim3(RPES_THREADS), 0, stream(), in, prob, (int*)status);
    else if (partner)
        hipLaunchKernelGGL(rpes_dist2_kernel<true>, dim3((unsigned)dist_blocks), dim3(RPES_THREADS), 0, stream(), in, prob, (int*)status);
    else
        hipLaunchKernelGGL(rpes_dist2_kernel<false>, dim3((unsigned)dist_blocks), dim3(RPES_THREADS), 0, stream(), in, prob, (int*)status);
    FBX_HIP(hipGetLastError());
    if (!(d_hist_out || d_moments_out || d_x_bits_out || d_y_bits_out)) return FBX_OK;
    RpeSimSchedule sched{};
    for (int j = 0; j < K; ++j) sched.n[j] = n_shots[j];
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(RPES_THREADS), 0, stream(), (long long)B, K, n_qubits, xy_qubit,
                           z_qubit, sched, (unsigned long long)seed, (long long)first_item, (const double*)prob, (const int*)status,
                           d_hist_out, d_moments_out, d_x_bits_out, d_y_bits_out);
    };
    const bool records = d_x_bits_out || d_y_bits_out;
    if (lane) {
        if (records) { if (partner) launch(rpes_shots_kernel<true, true, true>); else launch(rpes_shots_kernel<true, false, true>); }
        else { if (partner) launch(rpes_shots_kernel<true, true, false>); else launch(rpes_shots_kernel<true, false, false>); }
    } else {
        if (records) { if (partner) launch(rpes_shots_kernel<false, true, true>); else launch(rpes_shots_kernel<false, false, true>); }
        else { if (partner) launch(rpes_shots_kernel<false, true, false>); else launch(rpes_shots_kernel<false, false, false>); }
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rpe_simulate(int n_qubits, int64_t B, int K, const double* gate_ptm, const double* prep_ptm, const double* meas_ptm,
                     int basis_per_item, const double* init, int xy_qubit, int z_qubit, const double* flips, const int32_t* n_shots,
                     uint64_t seed, int64_t first_item, double* prob_out, uint32_t* hist_out, double* moments_out,
                     uint8_t* x_bits_out, uint8_t* y_bits_out, int32_t* status_out) {
    int64_t uniform_shots = -1;
    FBX_TRY(rpes_check(n_qubits, B, K, gate_ptm, xy_qubit, z_qubit, n_shots, first_item, prob_out, hist_out, moments_out, x_bits_out,
                       y_bits_out, status_out, &uniform_shots));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B, DD = (size_t)1 << (4 * n_qubits), cells = n * (size_t)K * 2 * (z_qubit >= 0 ? 4 : 2);
    const size_t basis_items = basis_per_item ? n : 1;
    const size_t record = uniform_shots > 0 ? n * (size_t)K * (size_t)uniform_shots * (size_t)n_qubits : 0;
    HostIO io; double *dg, *dp = nullptr, *dm = nullptr, *di = nullptr, *df = nullptr, *dprob, *dmom; uint32_t* dh;
    uint8_t *dxb, *dyb; int32_t* dst;
    FBX_TRY(io.in(gate_ptm, n * DD, &dg));
    if (prep_ptm) FBX_TRY(io.in(prep_ptm, basis_items * DD, &dp));
    if (meas_ptm) FBX_TRY(io.in(meas_ptm, basis_items * DD, &dm));
    if (init) FBX_TRY(io.in(init, (size_t)1 << (2 * n_qubits), &di));
    if (flips) FBX_TRY(io.in(flips, n * 2 * (size_t)n_qubits, &df));
    FBX_TRY(io.out_opt(prob_out, cells, &dprob));
    FBX_TRY(io.out_opt(hist_out, cells, &dh));
    FBX_TRY(io.out_opt(moments_out, 8 * n * (size_t)K, &dmom));
    FBX_TRY(io.out_opt(x_bits_out, record, &dxb));
    FBX_TRY(io.out_opt(y_bits_out, record, &dyb));
    FBX_TRY(io.out_opt(status_out, n, &dst));
    FBX_TRY(fbx_rpe_simulate_dev(n_qubits, B, K, dg, dp, dm, basis_per_item, di, xy_qubit, z_qubit, df, n_shots, seed, first_item,
                                 dprob, dh, dmom, dxb, dyb, dst));
    return io.finish();
}

}  // fbx C ABI
