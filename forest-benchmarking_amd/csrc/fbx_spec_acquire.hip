// fbx_spec_acquire.hip -- the acquisition of qubit-spectroscopy experiments (fbx_spec_acquire): from the physical curve of B
// qubits at K points each -- an exponential and / or Gaussian envelope times a cosine, on a baseline -- through the readout flips
// to the shots of every point and the bit statistics the fit front ends of fbx/qubit_spectroscopy.py read: what do_t1_or_t2,
// acquire_rabi_data and acquire_cz_phase_ramsey_data (qubit_spectroscopy.py:81-112, 325-356, 421-447) get from a QuantumComputer.
//
// Two kernels.  spec_poison_kernel (a wavefront per item) looks at the six parameters, the two flips and the K points of an
// item once and writes its status.  spec_acquire_kernel takes a unit = (item b, point k), u = b K + k: one exp and one cos for
// the probability (include/fbx.h, steps 1-4, without fused multiply-adds), then sim_bernoulli_unit, the shot counting of
// fbx_tomo_simulate.  The work split is fbx_tomo_simulate's, chosen by the number of units alone: from FBX_TOMO_LANE_MIN_UNITS
// on a LANE takes a unit -- consecutive lanes take consecutive points of an item, so x and every output coalesce -- and below
// that a WAVEFRONT takes a unit (the item, its parameters and its point are wave-uniform), lane l counts the Philox blocks l,
// l + 64, ... and lane 0 writes.  Both evaluate the probability with the same code and count the same words.  The loops are
// grid-stride: no B reaches a grid cap.
#include "fbx_sim_shared.hpp"

namespace fbx {

constexpr int SPEC_THREADS = 256, SPEC_WAVES = SPEC_THREADS / 64;
constexpr int SPEC_MAX_POINTS = 65536;
constexpr int64_t SPEC_MAX_BLOCKS = 1 << 16;     // beyond that the kernels stride
constexpr uint32_t SPEC_KEY_TAG = 0x51535043u;   // "QSPC": keeps the shots apart from every other simulator's under one seed

struct SpecIn {
    long long B, first_item;
    int K;
    long long x_stride;
    unsigned n_shots;
    unsigned long long seed;
    const double *x, *params, *flips;
    double *prob, *exact, *expect, *std_err, *counts, *bit, *bit_err;
    int32_t* status;
};

#if defined(__HIPCC__)
// status[b] = 1 for a non-finite amplitude, omega, offset or baseline, a time that is not > 0 (NaN included; +inf passes), a
// non-finite point or a flip outside [0, 1] (NaN included), else 0
__global__ void __launch_bounds__(SPEC_THREADS)
spec_poison_kernel(SpecIn in) {
    const int lane = threadIdx.x & 63;
    for (long long b = (long long)blockIdx.x * SPEC_WAVES + uniform((int)(threadIdx.x >> 6)); b < in.B;
         b += (long long)gridDim.x * SPEC_WAVES) {
        bool bad = false;
        if (lane < 6) {
            const double v = in.params[b * 6 + lane];
            bad = lane == 1 || lane == 2 ? !(v > 0.0) : !rpes_finite(v);
        } else if (lane < 8 && in.flips) {
            bad = tomo_bad_probability(in.flips[b * 2 + (lane - 6)]);
        }
        const double* x = in.x + b * in.x_stride;
        for (int k = lane; k < in.K; k += 64) bad |= !rpes_finite(x[k]);
        const unsigned long long any = __ballot(bad);
        if (lane == 0) in.status[b] = any ? 1 : 0;
    }
}

// steps 1-4 of the contract: the probability of reading 1 at x, every operation rounded on its own
__device__ __forceinline__ double spec_probability(const double* __restrict__ p, const double* __restrict__ fl, double x) {
#pragma clang fp contract(off)
    const double amplitude = p[0], decay_time = p[1], gauss_time = p[2], omega = p[3], offset = p[4], baseline = p[5];
    const double a = x / decay_time, g = x / gauss_time;
    const double env = exp(-a - g * g);
    const double arg = omega * x + offset;
    const double p_true = baseline + (amplitude * env) * cos(arg);
    if (!fl) return p_true;
    const double f0 = fl[0], f1 = fl[1];
    return f0 * (1.0 - p_true) + (1.0 - f1) * p_true;
}

// unit u = (item u / K, point u % K); LANE: a lane per unit, else a wavefront per unit
template <bool LANE>
__global__ void __launch_bounds__(SPEC_THREADS)
spec_acquire_kernel(SpecIn in) {
#pragma clang fp contract(off)
    const long long units = in.B * in.K;
    const int lane = threadIdx.x & 63;
    const uint32_t k0 = (uint32_t)in.seed ^ SPEC_KEY_TAG, k1 = (uint32_t)(in.seed >> 32);
    const long long first = LANE ? (long long)blockIdx.x * SPEC_THREADS + threadIdx.x
                                 : (long long)blockIdx.x * SPEC_WAVES + uniform((int)(threadIdx.x >> 6));
    const long long step = (long long)gridDim.x * (LANE ? SPEC_THREADS : SPEC_WAVES);
    for (long long u = first; u < units; u += step) {
        const long long b = u / in.K;
        const int k = (int)(u - b * in.K);
        const bool writer = LANE || lane == 0;
        if (in.status[b]) {
            if (writer) {
                sim_write_poisoned(in.expect, in.counts, in.std_err, in.exact, u, in.n_shots);
                const double nan = __builtin_nan("");
                if (in.prob) in.prob[u] = nan;
                if (in.bit) in.bit[u] = nan;
                if (in.bit_err) in.bit_err[u] = nan;
            }
            continue;
        }
        const double p_read = spec_probability(in.params + b * 6, in.flips ? in.flips + b * 2 : nullptr, in.x[b * in.x_stride + k]);
        const double mu = 1.0 - 2.0 * p_read;
        // without shots these stay; with shots the writing lane gets what sim_write_pm1 writes
        double expect = mu, std_err = 0.0, counts = 0.0;
        sim_bernoulli_unit<LANE>(mu, 1.0, (unsigned long long)(in.first_item + b), (uint32_t)k, k0, k1, lane, in.n_shots, 0, &expect,
                                 &counts, &std_err, nullptr);
        if (!writer) continue;
        if (in.prob) in.prob[u] = p_read;
        if (in.exact) in.exact[u] = mu;
        if (in.expect) in.expect[u] = expect;
        if (in.std_err) in.std_err[u] = std_err;
        if (in.counts) in.counts[u] = counts;
        if (in.bit) in.bit[u] = ((-1.0 * expect) + 1.0) / 2.0;
        if (in.bit_err) in.bit_err[u] = sqrt((std_err * std_err) / 4.0);
    }
}
#endif

static int spec_check(int64_t B, int K, const void* x, int64_t x_stride, const void* params, int64_t n_shots, int64_t first_item,
                      bool any_out) {
    FBX_TRY(sim_check_batch("fbx_spec_acquire", B, n_shots, first_item));
    FBX_REQUIRE(K >= 1 && K <= SPEC_MAX_POINTS, "fbx_spec_acquire: K must be in 1 .. 65536");
    FBX_REQUIRE(x_stride == 0 || x_stride == K, "fbx_spec_acquire: x_stride must be 0 (one x for the batch) or K (one row per item)");
    FBX_REQUIRE(B == 0 || (x && params), "fbx_spec_acquire: NULL x / params");
    FBX_REQUIRE(any_out, "fbx_spec_acquire: every output is NULL");
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_spec_acquire_dev(int64_t B, int K, const double* d_x, int64_t x_stride, const double* d_params, const double* d_flips,
                         int64_t n_shots, uint64_t seed, int64_t first_item, double* d_prob_out, double* d_exact_out,
                         double* d_expect_out, double* d_std_err_out, double* d_counts_out, double* d_bit_out, double* d_bit_err_out,
                         int32_t* d_status_out) {
    FBX_TRY(spec_check(B, K, d_x, x_stride, d_params, n_shots, first_item,
                       d_prob_out || d_exact_out || d_expect_out || d_std_err_out || d_counts_out || d_bit_out || d_bit_err_out ||
                           d_status_out));
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    StatusBuf status;
    FBX_TRY(status.take(d_status_out, B));
    SpecIn in{};
    in.B = B; in.first_item = first_item; in.K = K; in.x_stride = x_stride; in.n_shots = (unsigned)n_shots; in.seed = seed;
    in.x = d_x; in.params = d_params; in.flips = d_flips;
    in.prob = d_prob_out; in.exact = d_exact_out; in.expect = d_expect_out; in.std_err = d_std_err_out; in.counts = d_counts_out;
    in.bit = d_bit_out; in.bit_err = d_bit_err_out; in.status = status.p;
    auto blocks = [](int64_t work, int per_block) {
        const int64_t want = (work + per_block - 1) / per_block;
        return dim3((unsigned)(want < SPEC_MAX_BLOCKS ? want : SPEC_MAX_BLOCKS));
    };
    hipLaunchKernelGGL(spec_poison_kernel, blocks(B, SPEC_WAVES), dim3(SPEC_THREADS), 0, stream(), in);
    FBX_HIP(hipGetLastError());
    const int64_t units = B * K;
    if (units >= FBX_TOMO_LANE_MIN_UNITS)
        hipLaunchKernelGGL(spec_acquire_kernel<true>, blocks(units, SPEC_THREADS), dim3(SPEC_THREADS), 0, stream(), in);
    else
        hipLaunchKernelGGL(spec_acquire_kernel<false>, blocks(units, SPEC_WAVES), dim3(SPEC_THREADS), 0, stream(), in);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_spec_acquire(int64_t B, int K, const double* x, int64_t x_stride, const double* params, const double* flips, int64_t n_shots,
                     uint64_t seed, int64_t first_item, double* prob_out, double* exact_out, double* expect_out, double* std_err_out,
                     double* counts_out, double* bit_out, double* bit_err_out, int32_t* status_out) {
    FBX_TRY(spec_check(B, K, x, x_stride, params, n_shots, first_item,
                       prob_out || exact_out || expect_out || std_err_out || counts_out || bit_out || bit_err_out || status_out));
    if (B == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const size_t n = (size_t)B, units = n * (size_t)K;
    HostIO io; SimOut o; double *dx, *dp, *df = nullptr, *dprob, *dbit, *dbit_err;
    FBX_TRY(io.in(x, x_stride ? units : (size_t)K, &dx));
    FBX_TRY(io.in(params, n * 6, &dp));
    if (flips) FBX_TRY(io.in(flips, n * 2, &df));
    FBX_TRY(o.stage(io, n, units, expect_out, counts_out, std_err_out, exact_out, status_out));
    FBX_TRY(io.out_opt(prob_out, units, &dprob));
    FBX_TRY(io.out_opt(bit_out, units, &dbit));
    FBX_TRY(io.out_opt(bit_err_out, units, &dbit_err));
    FBX_TRY(fbx_spec_acquire_dev(B, K, dx, x_stride, dp, df, n_shots, seed, first_item, dprob, o.exact, o.expect, o.std_err, o.counts, dbit,
                                 dbit_err, o.status));
    return io.finish();
}

}  // extern "C"
