// fbx_rb_acquire.hip -- the acquisition of randomized-benchmarking and unitarity experiments (fbx_rb_acquire): from the noise
// channels of E qubits or pairs to the measured I/Z (or all-Pauli) expectations of every sequence, in one launch, with nothing
// but results leaving the device -- what generate_rb_experiment_sequences / generate_unitarity_experiment_sequences and
// acquire_rb_data / acquire_unitarity_data (randomized_benchmarking.py:129-305, 441-487) get from quilc and a QVM.
//
// rb_acquire_kernel<NQ, UNIT>: a lane per sequence, a wavefront per (experiment, 64 consecutive sequences of it); consecutive
// sequences share a depth (q = depth index * K + repetition), so the lanes of a wavefront run almost the same trip count.
//   draw      the lane draws its elements on the fly from the stream of fbx_rb_sequences (cl_draw / cl_from_index under the seed
//             seed + gid, sequence q), keeps the running composition and closes a standard sequence with its inverse: no element
//             array exists in memory.
//   simulate  the step of rb_simulate_kernel, operation for operation: the signed permutation through the lane's own LDS column
//             vec[k][256] (a register array under a lane-varying index would go to scratch), then the noise matrix, read as a
//             broadcast from the wavefront's slice of LDS, one chain of fused multiply-adds per row.
//   measure   per basis (all-Z, or the 3^n products of X, Y, Z for unitarity) the outcome distribution with the readout flips
//             (rpes_distribution), the shots through sim_walk / sim_count_word / sim_histogram in their lane form, and the
//             moments of every Pauli the basis is assigned (rpe_moment).
// The grid-stride loop runs over wavefront units whose trip counts differ, so it holds no workgroup barrier: a wavefront stages
// the G <= 2 matrices of its experiment into its own slice, and its LDS instructions execute in program order (FBX_WAVE_SYNC).
// A poisoned experiment is known to every wavefront that stages it, but a distribution without a positive finite sum is known
// to one lane only; the kernel therefore only RAISES status[e], and rb_acquire_poison_kernel, next on the stream, overwrites
// every output of a raised experiment.
//
// rb_depth_means_kernel: the mean over the K sequences of a depth and the standard error of that mean, a lane per output cell
// summing in ascending order.
#include "fbx_clifford_elems.hpp"
#include "fbx_sim_shared.hpp"

namespace fbx {

constexpr int RBA_THREADS = 256, RBA_WAVES = RBA_THREADS / 64;
constexpr int RBA_MAX_DEPTHS = 256;              // the depths travel with the launch; FBX_FIT_MAX_POINTS of them can be fitted
constexpr uint32_t RBA_KEY_TAG = 0x52424151u;    // "RBAQ": keeps the shots apart from every other simulator's under one seed

struct RbaDepths { int32_t d[RBA_MAX_DEPTHS]; };
struct RbaIn {
    long long E, SK, first_item;                 // SK = S K sequences per experiment
    int K, G;
    uint32_t interleaved, n_shots;
    unsigned long long seed;
    const double *ptms, *prep, *flips;
    double *vec, *prob, *expect, *std_err;
    uint32_t* hist;
    int32_t* status;
};

#if defined(__HIPCC__)
// one element: the signed permutation (perm, neg) through the lane's LDS column, then matrix `id` of the wavefront's slice --
// rb_simulate_kernel's step.  The slice does not change during a sequence, and nothing tells the compiler that 2 D^2 doubles are
// too many to keep: the offset passes through an empty asm, so that every step reads its matrix where it uses it.
template <int NQ>
__device__ __forceinline__ void rba_step(double (&v)[1 << (2 * NQ)], double* __restrict__ vec, int tid, unsigned long long perm,
                                         uint32_t neg, const double* __restrict__ lam, int id) {
    constexpr int D = 1 << (2 * NQ);
    int off = id * (D * D);
    asm volatile("" : "+s"(off));
    const double* Mx = lam + off;
#pragma unroll
    for (int k = 0; k < D; ++k)
        vec[(int)((perm >> (4 * k)) & 15ull) * RBA_THREADS + tid] = (neg >> k) & 1u ? -v[k] : v[k];
    double u[D];
#pragma unroll
    for (int k = 0; k < D; ++k) u[k] = vec[k * RBA_THREADS + tid];
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) acc = fma(Mx[r * D + c], u[c], acc);
        v[r] = acc;
    }
}

// UNIT: unitarity mode (not self-inverting, every Pauli measured); else standard / interleaved RB (self-inverting, all Z)
template <int NQ, bool UNIT>
__global__ void __launch_bounds__(RBA_THREADS)
rb_acquire_kernel(RbaIn in, RbaDepths depths) {
    constexpr int D = 1 << (2 * NQ), M = 1 << NQ, NB = UNIT ? (NQ == 1 ? 3 : 9) : 1, C = UNIT ? D - 1 : M - 1;
    __shared__ __attribute__((aligned(16))) double vec[D * RBA_THREADS];          // column tid belongs to lane tid alone
    __shared__ __attribute__((aligned(16))) double lam_all[RBA_WAVES][2 * D * D];   // the wavefront's own matrices
    const int tid = threadIdx.x, wave = uniform(tid >> 6), lane = tid & 63;
    double* lam = lam_all[wave];
    const long long chunks = (in.SK + 63) >> 6, units = in.E * chunks;
    const bool irb = !UNIT && in.interleaved != FBX_CLIFFORD_NONE;
    unsigned long long iperm = 0ull; uint32_t ineg = 0u;
    if (irb) cl_table<NQ>(in.interleaved, iperm, ineg);
    const uint32_t N = in.n_shots;
    const uint32_t k0 = (uint32_t)in.seed ^ RBA_KEY_TAG, k1 = (uint32_t)(in.seed >> 32);
    for (long long unit = (long long)blockIdx.x * RBA_WAVES + wave; unit < units; unit += (long long)gridDim.x * RBA_WAVES) {
        const long long e = unit / chunks, q0 = (unit - e * chunks) * 64, q = q0 + lane;
        FBX_WAVE_SYNC();                                        // the reads of the last unit are ahead of these writes
        bool bad = false;
        const double* P = in.ptms + e * (long long)(in.G * D * D);
        for (int i = lane; i < in.G * D * D; i += 64) { const double x = P[i]; lam[i] = x; bad |= !rpes_finite(x); }
        if (in.prep && lane < D) bad |= !rpes_finite(in.prep[lane]);
        const double* fl = in.flips ? in.flips + e * (2 * NQ) : nullptr;
        if (fl && lane < 2 * NQ) bad |= tomo_bad_probability(fl[lane]);
        FBX_WAVE_SYNC();
        if (__ballot(bad) != 0ull) {                            // every wavefront of the experiment sees the same inputs
            if (lane == 0) in.status[e] = 1;
            continue;
        }
        if (q < in.SK) {
            // the depth of sequence q: the depth indices of a unit are contiguous, and a wave-uniform index reads the launch arguments
            const int di = (int)(q / in.K), i_lo = (int)(q0 / in.K);
            const long long q_last = q0 + 63 < in.SK ? q0 + 63 : in.SK - 1;
            const int i_hi = (int)(q_last / in.K);
            int depth = 0;
            for (int i = i_lo; i <= i_hi; ++i) { const int d = depths.d[i]; if (di == i) depth = d; }
            const unsigned long long gid = (unsigned long long)(in.first_item + e), seq_seed = in.seed + gid;
            double v[D];
#pragma unroll
            for (int k = 0; k < D; ++k) v[k] = in.prep ? in.prep[k] : (((k & 0x5) ^ ((k >> 1) & 0x5)) == 0 ? 1.0 : 0.0);     // |0..0>
            // the elements of rb_sequences_kernel in its order: draws (at the even positions of an interleaved sequence), the
            // interleaved element, and last the inverse of everything before it; position i has the same noise id in every lane
            const int L = UNIT ? depth : (irb ? 2 * depth - 1 : depth);
            uint32_t total = ClGroup<NQ>::identity;             // everything so far, later elements on the left
            for (int i = 0; i < L; ++i) {
                const int id = irb ? (i & 1) : 0;
                unsigned long long perm; uint32_t neg;
                if (!UNIT && i == L - 1) {
                    cl_table<NQ>(total, perm, neg);
                    cl_table<NQ>(cl_inverse<NQ>(perm, neg), perm, neg);
                } else if (id) {
                    perm = iperm; neg = ineg;
                } else {
                    cl_table<NQ>(cl_from_index<NQ>(cl_draw(seq_seed, q, (uint32_t)(irb ? i >> 1 : i), ClGroup<NQ>::order)), perm, neg);
                }
                rba_step<NQ>(v, vec, tid, perm, neg, lam, id);
                if constexpr (!UNIT) total = cl_compose<NQ>(perm, neg, total);
            }
            const long long sq = e * in.SK + q;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                vec[k * RBA_THREADS + tid] = v[k];              // the bases below index the vector with a runtime (uniform) index
                if (in.vec) in.vec[sq * D + k] = v[k];
            }
            bool lane_bad = false;
            for (int basis = 0; basis < NB; ++basis) {
                // Pauli digits (1, 2, 3 = X, Y, Z) measured on qubit 0 and on qubit 1; index = digit of qubit 0 most significant
                const int a0 = UNIT ? 1 + (NQ == 1 ? basis : basis / 3) : 3, a1 = UNIT ? 1 + basis % 3 : 3;
                const int iA = NQ == 1 ? a0 : a0 << 2, iB = a1, iAB = iA | iB;
                const double vA = vec[iA * RBA_THREADS + tid];
                const double vB = NQ == 2 ? vec[iB * RBA_THREADS + tid] : 0.0, vAB = NQ == 2 ? vec[iAB * RBA_THREADS + tid] : 0.0;
                double p[4];
                const double sum = rpes_distribution<NQ == 2>(v[0], vA, vB, vAB, fl, fl && NQ == 2 ? fl + 2 : nullptr, p);
                if (rpes_bad_total(sum)) { lane_bad = true; in.status[e] = 1; }
                const long long cell = (sq * NB + basis) * M;
                if (in.prob) {
#pragma unroll
                    for (int o = 0; o < M; ++o) in.prob[cell + o] = p[o];
                }
                uint32_t hist[M];
#pragma unroll
                for (int o = 0; o < M; ++o) hist[o] = 0u;
                if (N != 0u && !lane_bad) {
                    double run = 0.0, c[M];
#pragma unroll
                    for (int o = 0; o < M; ++o) { run += p[o] < 0.0 ? 0.0 : p[o]; c[o] = run; }
                    uint32_t tlo[M - 1], reach[M - 1];
                    bool live[M - 1];
                    sim_thresholds<M>(c, tlo, live, reach);
                    sim_walk((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)(q * NB + basis), k0, k1, 0u, 1u, N,
                             [&](uint32_t w, uint32_t) { (void)sim_count_word<M>(w, tlo, live, reach); });
                    sim_histogram<M, true>(reach, N, hist);
                }
                if (in.hist) {
#pragma unroll
                    for (int o = 0; o < M; ++o) in.hist[cell + o] = hist[o];
                }
                if (!(in.expect || in.std_err)) continue;
                // column `col` holds the Pauli with index `pauli`, whose -1 outcomes this basis counted as n_odd
                auto put = [&](int col, int pauli, uint32_t n_odd) {
                    double mean, se = 0.0;
                    if (N == 0u) mean = vec[pauli * RBA_THREADS + tid];
                    else { double var; rpe_moment((long long)n_odd, (long long)N, mean, var); se = sqrt(var); }
                    if (in.expect) in.expect[sq * C + col] = mean;
                    if (in.std_err) in.std_err[sq * C + col] = se;
                };
                if constexpr (NQ == 1) {
                    put(UNIT ? basis : 0, iA, hist[1]);
                } else {
                    const uint32_t oddA = hist[2] + hist[3], oddB = hist[1] + hist[3], oddAB = hist[1] + hist[2];
                    if constexpr (UNIT) {
                        // a Pauli with an identity factor is read from the basis that has Z on the idle qubit
                        put(iAB - 1, iAB, oddAB);
                        if (a1 == 3) put(iA - 1, iA, oddA);
                        if (a0 == 3) put(iB - 1, iB, oddB);
                    } else {
                        put(0, iB, oddB); put(1, iA, oddA); put(2, iAB, oddAB);      // IZ, ZI, ZZ: the order of z_product_indices
                    }
                }
            }
        }
    }
}

// every output of an experiment whose status was raised: NaN in the doubles, 0 in the histograms; a thread per sequence
__global__ void __launch_bounds__(RBA_THREADS)
rb_acquire_poison_kernel(RbaIn in, int D, int NBM, int C) {
    const long long sq = (long long)blockIdx.x * RBA_THREADS + threadIdx.x;
    if (sq >= in.E * in.SK || in.status[sq / in.SK] == 0) return;
    const double nan = __builtin_nan("");
    if (in.vec) for (int k = 0; k < D; ++k) in.vec[sq * D + k] = nan;
    if (in.prob) for (int k = 0; k < NBM; ++k) in.prob[sq * NBM + k] = nan;
    if (in.hist) for (int k = 0; k < NBM; ++k) in.hist[sq * NBM + k] = 0u;
    if (in.expect) for (int k = 0; k < C; ++k) in.expect[sq * C + k] = nan;
    if (in.std_err) for (int k = 0; k < C; ++k) in.std_err[sq * C + k] = nan;
}

// values [E S][K][C] -> mean [E S][C] and the standard error of that mean; cell = (depth of an experiment, column)
__global__ void __launch_bounds__(RBA_THREADS)
rb_depth_means_kernel(long long cells, int K, int C, const double* __restrict__ values, const double* __restrict__ seq_std_errs,
                      double* __restrict__ mean_out, double* __restrict__ std_err_out) {
#pragma clang fp contract(off)
    const long long cell = (long long)blockIdx.x * RBA_THREADS + threadIdx.x;
    if (cell >= cells) return;
    const long long row = cell / C;
    const int c = (int)(cell - row * C);
    const double* x = values + row * K * C + c;
    double sum = 0.0;
    for (int s = 0; s < K; ++s) sum += x[(long long)s * C];
    const double mean = sum / (double)K;
    if (mean_out) mean_out[cell] = mean;
    if (!std_err_out) return;
    if (K == 1) { std_err_out[cell] = seq_std_errs ? seq_std_errs[row * C + c] : 0.0; return; }
    double ss = 0.0;
    for (int s = 0; s < K; ++s) { const double dx = x[(long long)s * C] - mean; ss += dx * dx; }
    std_err_out[cell] = sqrt(ss / (double)(K - 1) / (double)K);
}
#endif

struct RbaShape { int D, M, NB, C; };

static RbaShape rba_shape(int n, int mode) {
    const int D = 1 << (2 * n), M = 1 << n;
    const bool unit = mode == FBX_RB_UNITARITY;
    return {D, M, unit ? (n == 1 ? 3 : 9) : 1, unit ? D - 1 : M - 1};
}

static int rba_check(int n, int64_t E, int S, const int32_t* depths, int K, int mode, uint32_t interleaved, int G, const void* ptms,
                     int64_t n_shots, int64_t first_item, const void* vec, const void* prob, const void* hist, const void* expect,
                     const void* std_err, const void* status) {
    FBX_REQUIRE(n >= 1, "fbx_rb_acquire: n_qubits must be 1 or 2");
    if (n > 2) {
        set_error("fbx_rb_acquire: the Clifford group engine covers 1 and 2 qubits (got " + std::to_string(n) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_REQUIRE(E >= 0 && S >= 1 && K >= 1, "fbx_rb_acquire: need E >= 0, S >= 1 and K >= 1");
    FBX_REQUIRE(mode == FBX_RB_STANDARD || mode == FBX_RB_UNITARITY, "fbx_rb_acquire: mode must be FBX_RB_STANDARD or FBX_RB_UNITARITY");
    if (S > RBA_MAX_DEPTHS) {
        set_error("fbx_rb_acquire: at most 256 depths travel with a launch (got " + std::to_string(S) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_REQUIRE(depths != nullptr, "fbx_rb_acquire: NULL depths");
    const bool unit = mode == FBX_RB_UNITARITY;
    for (int i = 0; i < S; ++i)
        FBX_REQUIRE(depths[i] >= (unit ? 1 : 2),
                    "Sequence depth must be at least 2 for rb sequences, or at least 1 for unitarity sequences.");
    const bool irb = interleaved != FBX_CLIFFORD_NONE;
    FBX_REQUIRE(!(unit && irb), "fbx_rb_acquire: unitarity sequences take no interleaved element");
    FBX_REQUIRE(!irb || (n == 1 ? cl_valid<1>(interleaved) : cl_valid<2>(interleaved)),
                "fbx_rb_acquire: interleaved_elem is neither a valid element word nor FBX_CLIFFORD_NONE");
    FBX_REQUIRE(G == (irb ? 2 : 1), "fbx_rb_acquire: G must be 1 for a plain run and 2 with an interleaved element");
    FBX_REQUIRE(first_item >= 0, "fbx_rb_acquire: first_item must not be negative");
    FBX_REQUIRE(n_shots >= 0 && n_shots < ((int64_t)1 << 31), "fbx_rb_acquire: n_shots must be in 0 .. 2^31 - 1");
    const RbaShape sh = rba_shape(n, mode);
    FBX_REQUIRE((int64_t)S * K * sh.NB < ((int64_t)1 << 32), "fbx_rb_acquire: S * K * bases must be below 2^32");
    FBX_REQUIRE(E <= (INT64_MAX >> 12) / ((int64_t)S * K), "fbx_rb_acquire: E * S * K overflows");
    FBX_REQUIRE(vec || prob || hist || expect || std_err || status, "fbx_rb_acquire: every output is NULL");
    FBX_REQUIRE(!(hist && n_shots == 0), "fbx_rb_acquire: hist_out needs n_shots >= 1 (n_shots = 0 draws no shots)");
    FBX_REQUIRE(E == 0 || ptms != nullptr, "fbx_rb_acquire: NULL noise_ptms");
    return FBX_OK;
}

static int rb_depth_means_check(int64_t E, int S, int K, int C, const void* values, const void* mean, const void* std_err) {
    FBX_REQUIRE(E >= 0 && S >= 1 && K >= 1 && C >= 1, "fbx_rb_depth_means: need E >= 0, S >= 1, K >= 1 and C >= 1");
    FBX_REQUIRE(E <= (INT64_MAX >> 4) / ((int64_t)S * K) / C, "fbx_rb_depth_means: E * S * K * C overflows");
    FBX_REQUIRE(mean || std_err, "fbx_rb_depth_means: every output is NULL");
    FBX_REQUIRE(E == 0 || values != nullptr, "fbx_rb_depth_means: NULL values");
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_rb_acquire_dev(int n_qubits, int64_t E, int S, const int32_t* depths, int K, int mode, uint32_t interleaved_elem, int G,
                       const double* d_noise_ptms, const double* d_prep, const double* d_flips, int64_t n_shots, uint64_t seed,
                       int64_t first_item, double* d_vec_out, double* d_prob_out, uint32_t* d_hist_out, double* d_expect_out,
                       double* d_std_err_out, int32_t* d_status_out) {
    FBX_TRY(rba_check(n_qubits, E, S, depths, K, mode, interleaved_elem, G, d_noise_ptms, n_shots, first_item, d_vec_out, d_prob_out,
                      d_hist_out, d_expect_out, d_std_err_out, d_status_out));
    if (E == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const RbaShape sh = rba_shape(n_qubits, mode);
    RbaIn in{};
    in.E = E; in.SK = (long long)S * K; in.first_item = first_item; in.K = K; in.G = G;
    in.interleaved = interleaved_elem; in.n_shots = (uint32_t)n_shots; in.seed = seed;
    in.ptms = d_noise_ptms; in.prep = d_prep; in.flips = d_flips;
    in.vec = d_vec_out; in.prob = d_prob_out; in.expect = d_expect_out; in.std_err = d_std_err_out; in.hist = d_hist_out;
    const int64_t units = E * ((in.SK + 63) / 64), want = (units + RBA_WAVES - 1) / RBA_WAVES;
    const int64_t fix_blocks = (E * in.SK + RBA_THREADS - 1) / RBA_THREADS;
    FBX_REQUIRE(fix_blocks < ((int64_t)1 << 31), "fbx_rb_acquire: E * S * K is beyond one launch; cut the batch with first_item");
    StatusBuf status_buf;
    FBX_TRY(status_buf.take(d_status_out, E));
    in.status = status_buf.p;
    FBX_HIP(hipMemsetAsync(in.status, 0, sizeof(int32_t) * (size_t)E, stream()));
    RbaDepths dep{};
    for (int i = 0; i < S; ++i) dep.d[i] = depths[i];
    const dim3 grid((unsigned)(want < 256 * 16 ? want : 256 * 16)), block(RBA_THREADS);
    const bool unit = mode == FBX_RB_UNITARITY;
    if (n_qubits == 1) {
        if (unit) hipLaunchKernelGGL((rb_acquire_kernel<1, true>), grid, block, 0, stream(), in, dep);
        else hipLaunchKernelGGL((rb_acquire_kernel<1, false>), grid, block, 0, stream(), in, dep);
    } else {
        if (unit) hipLaunchKernelGGL((rb_acquire_kernel<2, true>), grid, block, 0, stream(), in, dep);
        else hipLaunchKernelGGL((rb_acquire_kernel<2, false>), grid, block, 0, stream(), in, dep);
    }
    FBX_HIP(hipGetLastError());
    hipLaunchKernelGGL(rb_acquire_poison_kernel, dim3((unsigned)fix_blocks), block, 0, stream(), in, sh.D, sh.NB * sh.M, sh.C);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rb_acquire(int n_qubits, int64_t E, int S, const int32_t* depths, int K, int mode, uint32_t interleaved_elem, int G,
                   const double* noise_ptms, const double* prep, const double* flips, int64_t n_shots, uint64_t seed,
                   int64_t first_item, double* vec_out, double* prob_out, uint32_t* hist_out, double* expect_out,
                   double* std_err_out, int32_t* status_out) {
    FBX_TRY(rba_check(n_qubits, E, S, depths, K, mode, interleaved_elem, G, noise_ptms, n_shots, first_item, vec_out, prob_out,
                      hist_out, expect_out, std_err_out, status_out));
    if (E == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const RbaShape sh = rba_shape(n_qubits, mode);
    const size_t n = (size_t)E, seqs = n * (size_t)S * (size_t)K;
    HostIO io; double *dl, *dp = nullptr, *df = nullptr, *dvec, *dprob, *dexp, *dse; uint32_t* dh; int32_t* dst;
    FBX_TRY(io.in(noise_ptms, n * (size_t)G * sh.D * sh.D, &dl));
    if (prep) FBX_TRY(io.in(prep, (size_t)sh.D, &dp));
    if (flips) FBX_TRY(io.in(flips, n * 2 * (size_t)n_qubits, &df));
    FBX_TRY(io.out_opt(vec_out, seqs * sh.D, &dvec));
    FBX_TRY(io.out_opt(prob_out, seqs * sh.NB * sh.M, &dprob));
    FBX_TRY(io.out_opt(hist_out, seqs * sh.NB * sh.M, &dh));
    FBX_TRY(io.out_opt(expect_out, seqs * sh.C, &dexp));
    FBX_TRY(io.out_opt(std_err_out, seqs * sh.C, &dse));
    FBX_TRY(io.out_opt(status_out, n, &dst));
    FBX_TRY(fbx_rb_acquire_dev(n_qubits, E, S, depths, K, mode, interleaved_elem, G, dl, dp, df, n_shots, seed, first_item, dvec, dprob,
                               dh, dexp, dse, dst));
    return io.finish();
}

int fbx_rb_depth_means_dev(int64_t E, int S, int K, int C, const double* d_values, const double* d_seq_std_errs, double* d_mean_out,
                           double* d_std_err_out) {
    FBX_TRY(rb_depth_means_check(E, S, K, C, d_values, d_mean_out, d_std_err_out));
    if (E == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const int64_t cells = E * S * C, blocks = (cells + RBA_THREADS - 1) / RBA_THREADS;
    FBX_REQUIRE(blocks < ((int64_t)1 << 31), "fbx_rb_depth_means: E * S * C is beyond one launch");
    hipLaunchKernelGGL(rb_depth_means_kernel, dim3((unsigned)blocks), dim3(RBA_THREADS), 0, stream(), (long long)cells, K, C, d_values,
                       d_seq_std_errs, d_mean_out, d_std_err_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rb_depth_means(int64_t E, int S, int K, int C, const double* values, const double* seq_std_errs, double* mean_out,
                       double* std_err_out) {
    FBX_TRY(rb_depth_means_check(E, S, K, C, values, mean_out, std_err_out));
    if (E == 0) return FBX_OK;
    FBX_TRY(ensure_device());
    const size_t cells = (size_t)E * (size_t)S * (size_t)C;
    HostIO io; double *dv, *ds = nullptr, *dm, *de;
    FBX_TRY(io.in(values, cells * (size_t)K, &dv));
    if (seq_std_errs && K == 1) FBX_TRY(io.in(seq_std_errs, cells, &ds));
    FBX_TRY(io.out_opt(mean_out, cells, &dm));
    FBX_TRY(io.out_opt(std_err_out, cells, &de));
    FBX_TRY(fbx_rb_depth_means_dev(E, S, K, C, dv, ds, dm, de));
    return io.finish();
}

}  // extern "C"
