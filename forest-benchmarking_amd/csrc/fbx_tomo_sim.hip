// fbx_tomo_sim.hip -- simulated tomography experiments (fbx_tomo_simulate): from true channels / states to the noisy
// (expectations, total_counts) that the tomography estimators read -- the acquisition half the reference gets from a QVM.
//
// Two kernels.  tomo_poison_kernel (a wavefront per item) looks at every truth entry and flip probability of an item once and
// writes its status.  tomo_sim_kernel takes a unit = (item b, grouped setting g): it computes the mean of the measured +-1
// product from the design's own tables -- tr[P Lambda(rho_s)] = sum_j R[P][j] c_j(s), a row of the item's transfer matrix against
// a row of DesignDev::Ct; for a state design the trace against the density matrix itself -- with the readout flips folded in
// exactly (include/fbx.h), and then counts the shots whose Philox word falls below the threshold.  The truth is read from L2:
// per setting the mean costs D fused multiply-adds per term, the counting n_shots / 4 Philox blocks of about a hundred
// instructions each, so the counting is the cost from a few dozen shots on.
//
// The work split is chosen by the number of units alone: from TOMO_LANE_MIN_UNITS on a LANE takes a unit and counts all its
// shots (the chip is full without cutting a setting); below, a WAVEFRONT takes a unit, lane l counts the Philox blocks l, l + 64,
// ... and the 64 partial counts are summed (integers, exactly, in double).  A value depends on (seed, item id, setting, mean, shots)
// only: both splits evaluate the mean with the same code in the same order and count the same words.
#include "fbx_sim_shared.hpp"      // sim_bernoulli_unit and the unit threshold, shared with fbx_dfe.hip; tomo_mean, with fbx_tomo_sim_grouped.hip

namespace fbx {

constexpr int TOMO_THREADS = 256;
constexpr uint32_t TOMO_KEY_TAG = 0x544F4D4Fu;   // "TOMO": keeps the stream apart from fbx_sample_bitstrings under one seed

// status[b] = 1 when item b has a non-finite truth entry or a flip probability outside [0, 1] (NaN included), else 0
__global__ void __launch_bounds__(TOMO_THREADS)
tomo_poison_kernel(long long B, int truth_len, int flip_len, const double* __restrict__ truth, const double* __restrict__ flips,
                   int* __restrict__ status) {
    const long long b = (long long)blockIdx.x * (TOMO_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const double* t = truth + b * truth_len;
    bool bad = false;
    for (int i = lane; i < truth_len; i += 64) {
        const double v = t[i];
        if (!(fabs(v) < __builtin_inf())) bad = true;
    }
    if (flips && lane < flip_len && tomo_bad_probability(flips[b * flip_len + lane])) bad = true;
    const unsigned long long any = __ballot(bad);
    if (lane == 0) status[b] = any ? 1 : 0;
}

int tomo_poison_launch(int64_t B, int truth_len, int flip_len, const double* d_truth, const double* d_flips, int32_t* d_status) {
    constexpr int WAVES = TOMO_THREADS / 64;
    hipLaunchKernelGGL(tomo_poison_kernel, dim3((unsigned)((B + WAVES - 1) / WAVES)), dim3(TOMO_THREADS), 0, stream(), (long long)B,
                       truth_len, flip_len, d_truth, d_flips, d_status);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

// unit u = (item u / m, grouped setting u % m); LANE: a lane per unit, else a wavefront per unit
template <bool LANE>
__global__ void __launch_bounds__(TOMO_THREADS)
tomo_sim_kernel(DesignDev des, long long B, const double* __restrict__ truth, int truth_len, const double* __restrict__ flips,
                unsigned n_shots, unsigned long long seed, long long first_item, const int* __restrict__ status,
                double* __restrict__ expect_out, double* __restrict__ counts_out, double* __restrict__ std_err_out,
                double* __restrict__ exact_out) {
    const long long units = B * des.m;
    const int lane = threadIdx.x & 63;
    const long long u = LANE ? (long long)blockIdx.x * TOMO_THREADS + threadIdx.x
                             : (long long)blockIdx.x * (TOMO_THREADS / 64) + uniform((int)(threadIdx.x >> 6));
    if (u >= units) return;
    const long long b = u / des.m;
    const int g = (int)(u - b * des.m), k = des.order[g];
    const double coef = des.coef[g];
    const long long out = b * des.m + k;
    if (status[b]) {
        if (LANE || lane == 0) sim_write_poisoned(expect_out, counts_out, std_err_out, exact_out, out, n_shots);
        return;
    }
    const double mu = tomo_mean(des, truth + b * truth_len, flips ? flips + b * 2 * des.n : nullptr, des.sp[g]);
    sim_bernoulli_unit<LANE>(mu, coef, (unsigned long long)(first_item + b), (uint32_t)k, (uint32_t)seed ^ TOMO_KEY_TAG,
                             (uint32_t)(seed >> 32), lane, n_shots, out, expect_out, counts_out, std_err_out, exact_out);
}

static int tomo_check(const fbx_design* design, int64_t B, const void* truth, int64_t n_shots, int64_t first_item,
                      const void* expect, const void* counts, const void* std_err, const void* exact) {
    FBX_TRY(sim_check_batch("fbx_tomo_simulate", B, n_shots, first_item));
    FBX_REQUIRE(truth != nullptr, "fbx_tomo_simulate: NULL truth");
    FBX_REQUIRE(expect || counts || std_err || exact, "fbx_tomo_simulate: every output is NULL");
    FBX_REQUIRE(n_shots > 0 || !(expect || counts || std_err),
                "fbx_tomo_simulate: n_shots == 0 gives exact_out only (expect_out, counts_out and std_err_out must be NULL)");
    return check_design(design, "fbx_tomo_simulate");
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_tomo_simulate_dev(const fbx_design* design, int64_t B, const double* d_truth, int64_t n_shots, const double* d_readout_flip,
                          uint64_t seed, int64_t first_item, double* d_expect_out, double* d_counts_out, double* d_std_err_out,
                          double* d_exact_out, int32_t* d_status_out) {
    FBX_TRY(tomo_check(design, B, d_truth, n_shots, first_item, d_expect_out, d_counts_out, d_std_err_out, d_exact_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const DesignDev& des = design->dev;
    const int truth_len = tomo_truth_len(des);
    StatusBuf status;
    FBX_TRY(status.take(d_status_out, B));
    constexpr int WAVES = TOMO_THREADS / 64;
    FBX_TRY(tomo_poison_launch(B, truth_len, 2 * des.n, d_truth, d_readout_flip, status.p));
    const int64_t units = B * des.m;
    if (units >= FBX_TOMO_LANE_MIN_UNITS) {
        const int64_t blocks = (units + TOMO_THREADS - 1) / TOMO_THREADS;
        FBX_REQUIRE(blocks < ((int64_t)1 << 31), "fbx_tomo_simulate: B * m is beyond one launch; cut the batch with first_item");
        hipLaunchKernelGGL(tomo_sim_kernel<true>, dim3((unsigned)blocks), dim3(TOMO_THREADS), 0, stream(), des, (long long)B, d_truth,
                           truth_len, d_readout_flip, (unsigned)n_shots, (unsigned long long)seed, (long long)first_item,
                           (const int*)status.p, d_expect_out, d_counts_out, d_std_err_out, d_exact_out);
    } else {
        hipLaunchKernelGGL(tomo_sim_kernel<false>, dim3((unsigned)((units + WAVES - 1) / WAVES)), dim3(TOMO_THREADS), 0, stream(), des,
                           (long long)B, d_truth, truth_len, d_readout_flip, (unsigned)n_shots, (unsigned long long)seed,
                           (long long)first_item, (const int*)status.p, d_expect_out, d_counts_out, d_std_err_out, d_exact_out);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_tomo_simulate(const fbx_design* design, int64_t B, const double* truth, int64_t n_shots, const double* readout_flip,
                      uint64_t seed, int64_t first_item, double* expect_out, double* counts_out, double* std_err_out,
                      double* exact_out, int32_t* status_out) {
    FBX_TRY(tomo_check(design, B, truth, n_shots, first_item, expect_out, counts_out, std_err_out, exact_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B, m = (size_t)design->dev.m;
    HostIO io; SimOut o; double *dt, *df = nullptr;
    FBX_TRY(io.in(truth, n * (size_t)tomo_truth_len(design->dev), &dt));
    if (readout_flip) FBX_TRY(io.in(readout_flip, n * 2 * (size_t)design->dev.n, &df));
    FBX_TRY(o.stage(io, n, n * m, expect_out, counts_out, std_err_out, exact_out, status_out));
    FBX_TRY(fbx_tomo_simulate_dev(design, B, dt, n_shots, df, seed, first_item, o.expect, o.counts, o.std_err, o.exact, o.status));
    return io.finish();
}

}  // fbx C ABI
