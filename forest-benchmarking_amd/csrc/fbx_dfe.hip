// fbx_dfe.hip -- direct fidelity estimation of Clifford circuits on up to 64 qubits: the experiment generators of the reference
// (direct_fidelity_estimation.py:15-182), the conjugation quilc does for them, and the noisy expectations of every setting.
//
// A Pauli is two 64-bit masks and a sign bit, a gate one uint32 word (include/fbx.h), and conjugating by a gate is a handful of
// bit operations: every kernel here that walks a circuit gives a LANE one Pauli and lets all lanes read the same gate word, so
// the opcode, the qubit indices and the noise class of a gate are wave-uniform and are branched on with scalar branches.
//   conjugate_kernel   M Paulis through the circuit, forwards (U P U^+) or backwards (U^+ P U).
//   settings_kernel    setting k of one of the four generators: the input Pauli from k (exhaustive) or from the Philox blocks of
//                      (seed, k) (Monte Carlo), conjugated forwards.
//   propagate_kernel   the observable of setting k walked backwards: per noise class the number of gates it touches, and the
//                      ideal expectation of the Pauli it arrives as in the setting's product in-state.
//   dfe_sim_kernel     unit = (item b, setting k): the mean as a product of attenuations, then the shot counting of
//                      fbx_tomo_simulate (sim_bernoulli_unit, fbx_sim_shared.hpp) under a key tag of its own; a lane per unit from
//                      FBX_TOMO_LANE_MIN_UNITS units on, a wavefront per unit below, the same bits either way.
//   dfe_fidelity_kernel  dfe_item (fbx_sim_shared.hpp) with d = 2^n as a double, for the resident chain.
// The walks cost about twenty integer instructions per gate and lane and read nothing but the gate words (from L2 / the scalar
// cache); the simulation is bound by the Philox counting from a few dozen shots on, as in fbx_tomo_sim.hip.  The conjugation by one
// gate, the walk and the host checks of gate words are in fbx_clifford_gates.hpp, shared with fbx_frames.hip.
#include "fbx_sim_shared.hpp"
#include "fbx_clifford_gates.hpp"

namespace fbx {

constexpr int DFE_THREADS = 256;
constexpr uint32_t DFE_KEY_SETTINGS = 0x44464553u;      // "DFES": the Monte Carlo settings
constexpr uint32_t DFE_KEY_SHOTS = 0x44464530u;         // "DFE0": the shots of the experiment
constexpr uint32_t DFE_KEY_CALIBRATION = 0x44464543u;   // "DFEC": the shots of the calibration runs
constexpr int DFE_MAX_ATTEMPTS = 256;

#if defined(__HIPCC__)

__global__ void __launch_bounds__(DFE_THREADS)
conjugate_kernel(int n, long long G, const uint32_t* __restrict__ gates, int inverse, long long M, const uint64_t* __restrict__ x_in,
                 const uint64_t* __restrict__ z_in, const uint8_t* __restrict__ sign_in, uint64_t* __restrict__ x_out,
                 uint64_t* __restrict__ z_out, uint8_t* __restrict__ sign_out) {
    const long long i = (long long)blockIdx.x * DFE_THREADS + threadIdx.x;
    if (i >= M) return;
    const uint64_t valid = dfe_valid_mask(n);
    uint64_t x = x_in[i] & valid, z = z_in[i] & valid;
    uint32_t sign = sign_in[i] & 1u;
    dfe_walk(gates, G, inverse, x, z, sign);
    x_out[i] = x; z_out[i] = z; sign_out[i] = (uint8_t)sign;
}

// bit q of the result = bit n - 1 - q of v: "qubit 0 is the most significant digit"
__device__ __forceinline__ uint64_t dfe_reverse_bits(uint64_t v, int n) { return __brevll(v) >> (64 - n); }

__global__ void __launch_bounds__(DFE_THREADS)
settings_kernel(int n, int process, long long n_terms, unsigned long long seed, long long G, const uint32_t* __restrict__ gates,
                long long m, uint64_t* __restrict__ in_x, uint64_t* __restrict__ in_z, uint64_t* __restrict__ in_minus,
                uint64_t* __restrict__ obs_x, uint64_t* __restrict__ obs_z, uint8_t* __restrict__ obs_sign) {
    const long long k = (long long)blockIdx.x * DFE_THREADS + threadIdx.x;
    if (k >= m) return;
    const uint64_t valid = dfe_valid_mask(n);
    uint64_t px = 0, pz = 0, minus = 0;
    if (n_terms == 0) {
        if (!process) {
            pz = dfe_reverse_bits((uint64_t)k + 1u, n);                    // the (k + 1)-th string of product('IZ', repeat=n)
        } else {                                                           // m < 2^31: n <= 10 here
            const uint64_t j = ((uint64_t)k >> n) + 1u, e = (uint64_t)k & valid;
            for (int q = 0; q < n; ++q) {
                const uint64_t digit = (j >> (2 * (n - 1 - q))) & 3u;       // I X Y Z = 0 1 2 3
                px |= (uint64_t)(digit == 1u || digit == 2u) << q;
                pz |= (uint64_t)(digit == 2u || digit == 3u) << q;
            }
            minus = dfe_reverse_bits(e, n);
        }
    } else {
        const uint32_t k0 = (uint32_t)seed ^ DFE_KEY_SETTINGS, k1 = (uint32_t)(seed >> 32);
        const uint32_t c0 = (uint32_t)(unsigned long long)k, c1 = (uint32_t)((unsigned long long)k >> 32);
        uint32_t a = 0;
        for (; a < (uint32_t)DFE_MAX_ATTEMPTS; ++a) {
            uint32_t c[4] = {c0, c1, a, 0u};
            philox4x32_10(c, k0, k1);
            pz = ((uint64_t)c[0] | ((uint64_t)c[1] << 32)) & valid;
            if (process) { px = pz; pz = ((uint64_t)c[2] | ((uint64_t)c[3] << 32)) & valid; }
            if (px | pz) break;
        }
        if (a == (uint32_t)DFE_MAX_ATTEMPTS) { pz = valid; px = process ? valid : 0; }
        if (process) {
            uint32_t c[4] = {c0, c1, a, 1u};
            philox4x32_10(c, k0, k1);
            minus = ((uint64_t)c[0] | ((uint64_t)c[1] << 32)) & valid;
        }
    }
    const uint64_t support = px | pz;
    uint64_t x = px, z = pz;
    uint32_t sign = 0;
    dfe_walk(gates, G, 0, x, z, sign);
    in_x[k] = px;
    in_z[k] = pz | (~support & valid);                                       // I -> Z: |0> or |1> on the idle qubits
    in_minus[k] = minus;
    obs_x[k] = x; obs_z[k] = z;
    obs_sign[k] = (uint8_t)((sign ^ (uint32_t)__popcll(minus & support)) & 1u);
}

template <int K>
__global__ void __launch_bounds__(DFE_THREADS)
propagate_kernel(int n, long long G, const uint32_t* __restrict__ gates, const uint8_t* __restrict__ noise_class, int k_classes,
                 long long m, const uint64_t* __restrict__ in_x, const uint64_t* __restrict__ in_z,
                 const uint64_t* __restrict__ in_minus, const uint64_t* __restrict__ obs_x, const uint64_t* __restrict__ obs_z,
                 int8_t* __restrict__ sigma_out, uint32_t* __restrict__ touches_out) {
    const long long i = (long long)blockIdx.x * DFE_THREADS + threadIdx.x;
    const bool live = i < m;
    const uint64_t valid = dfe_valid_mask(n);
    uint64_t x = live ? obs_x[i] & valid : 0, z = live ? obs_z[i] & valid : 0;
    uint32_t sign = 0;
    uint32_t cnt[K];
#pragma unroll
    for (int c = 0; c < K; ++c) cnt[c] = 0;
    for (long long g = G - 1; g >= 0; --g) {
        const uint32_t w = gates[g];
        const uint32_t op = w & 0xFFu, q0 = (w >> 8) & 63u, q1 = (w >> 16) & 63u;
        const int cls = noise_class ? uniform((int)noise_class[g]) : 0;     // wave-uniform: the chain below is scalar branches
        if (cls < K) {
            uint64_t on = ((x | z) >> q0) & 1u;
            if (op >= FBX_GATE_CNOT) on |= ((x | z) >> q1) & 1u;
#pragma unroll
            for (int c = 0; c < K; ++c)
                if (cls == c) cnt[c] += (uint32_t)on;
        }
        dfe_apply_gate(dfe_inverse_opcode(op), q0, q1, x, z, sign);
    }
    if (!live) return;
    const uint64_t support = x | z;
    const uint64_t wrong = ((x ^ in_x[i]) | (z ^ in_z[i])) & support;
    const uint32_t parity = (sign + (uint32_t)__popcll(in_minus[i] & support)) & 1u;
    sigma_out[i] = wrong ? (int8_t)0 : (parity ? (int8_t)-1 : (int8_t)1);
#pragma unroll
    for (int c = 0; c < K; ++c)
        if (c < k_classes) touches_out[i * k_classes + c] = cnt[c];
}

// status[b] = 1 when item b has a class error or a flip probability outside [0, 1] (NaN included), else 0; a wavefront per item
__global__ void __launch_bounds__(DFE_THREADS)
dfe_poison_kernel(long long B, int K, int n, const double* __restrict__ class_error, const double* __restrict__ flips,
                  int* __restrict__ status) {
    const long long b = (long long)blockIdx.x * (DFE_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    bool bad = false;
    if (class_error && lane < K && dfe_bad_probability(class_error[b * K + lane])) bad = true;
    if (flips && lane < n && dfe_bad_probability(flips[b * n + lane])) bad = true;
    const unsigned long long any = __ballot(bad);
    if (lane == 0) status[b] = any ? 1 : 0;
}

// base^t by squaring: at most t - 1 roundings
__device__ __forceinline__ double dfe_pow(double base, uint32_t t) {
    double r = 1.0;
    while (t) {
        if (t & 1u) r *= base;
        t >>= 1;
        if (t) base *= base;
    }
    return r;
}

// the mean of the measured +-1 product of setting k under the noise of one item (include/fbx.h, THE MEAN)
__device__ __forceinline__ double dfe_mean(int n, int K, int calibration, int sigma, const uint32_t* __restrict__ touches,
                                           uint64_t support, const double* __restrict__ class_error,
                                           const double* __restrict__ flips) {
    double mu = 1.0;
    if (!calibration) {
        mu = (double)sigma;
        if (class_error)
            for (int c = 0; c < K; ++c) mu *= dfe_pow(1.0 - class_error[c], touches[c]);
    }
    if (flips)
        for (uint64_t s = support; s; s &= s - 1) mu *= 1.0 - 2.0 * flips[__builtin_ctzll(s)];
    return mu;
}

// unit u = (item u / m, setting u % m); LANE: a lane per unit, else a wavefront per unit
template <bool LANE>
__global__ void __launch_bounds__(DFE_THREADS)
dfe_sim_kernel(int n, long long m, int K, const int8_t* __restrict__ sigma, const uint32_t* __restrict__ touches,
               const uint64_t* __restrict__ obs_x, const uint64_t* __restrict__ obs_z, const uint8_t* __restrict__ obs_sign,
               long long B, const double* __restrict__ class_error, const double* __restrict__ flips, int calibration,
               unsigned n_shots, unsigned long long seed, long long first_item, const int* __restrict__ status,
               double* __restrict__ expect_out, double* __restrict__ counts_out, double* __restrict__ std_err_out,
               double* __restrict__ exact_out) {
    const long long units = B * m;
    const int lane = threadIdx.x & 63;
    const long long u = LANE ? (long long)blockIdx.x * DFE_THREADS + threadIdx.x
                             : (long long)blockIdx.x * (DFE_THREADS / 64) + uniform((int)(threadIdx.x >> 6));
    if (u >= units) return;
    const long long b = u / m, k = u - b * m;
    const double coef = (!calibration && (obs_sign[k] & 1u)) ? -1.0 : 1.0;     // the calibration measures the observable with coefficient 1
    if (status[b]) {
        if (LANE || lane == 0) sim_write_poisoned(expect_out, counts_out, std_err_out, exact_out, u, n_shots);
        return;
    }
    const double mu = dfe_mean(n, K, calibration, (int)sigma[k], touches + k * K, (obs_x[k] | obs_z[k]) & dfe_valid_mask(n),
                               class_error ? class_error + b * K : nullptr, flips ? flips + b * n : nullptr);
    sim_bernoulli_unit<LANE>(mu, coef, (unsigned long long)(first_item + b), (uint32_t)k,
                             (uint32_t)seed ^ (calibration ? DFE_KEY_CALIBRATION : DFE_KEY_SHOTS), (uint32_t)(seed >> 32), lane,
                             n_shots, u, expect_out, counts_out, std_err_out, exact_out);
}

// the calibration's standard errors -> variances, in place (what fbx_calibrate_expectations reads)
__global__ void __launch_bounds__(DFE_THREADS)
dfe_square_kernel(long long total, double* __restrict__ v) {
    for (long long i = (long long)blockIdx.x * DFE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * DFE_THREADS) {
        const double s = v[i];
        v[i] = s * s;
    }
}

// one wavefront per experiment (dfe_item), d = 2^n as a double: any n up to 64
__global__ void __launch_bounds__(64)
dfe_fidelity_kernel(double d, int process, long long B, long long m, const double* __restrict__ expect,
                    const double* __restrict__ std_err, double* __restrict__ mean_out, double* __restrict__ err_out) {
    for (long long item = blockIdx.x; item < B; item += gridDim.x)
        dfe_item(d, process, m, expect + item * m, std_err + item * m, (int)threadIdx.x, mean_out + item, err_out + item);
}

#endif

// ------------------------------------------------------------------ host: argument checks
static int dfe_blocks(const char* who, int64_t items, unsigned* out) {
    const int64_t blocks = (items + DFE_THREADS - 1) / DFE_THREADS;
    if (blocks >= ((int64_t)1 << 31)) { set_error(std::string(who) + ": too many items for one launch"); return FBX_ERR_BAD_ARG; }
    *out = (unsigned)blocks;
    return FBX_OK;
}

static int conjugate_check(int n, int64_t G, const void* gates, int64_t M, const void* x_in, const void* z_in, const void* s_in,
                           const void* x_out, const void* z_out, const void* s_out) {
    FBX_TRY(dfe_check_circuit("fbx_clifford_conjugate", n, G, gates));
    FBX_REQUIRE(M >= 0, "fbx_clifford_conjugate: negative M");
    FBX_REQUIRE(M == 0 || (x_in && z_in && s_in && x_out && z_out && s_out), "fbx_clifford_conjugate: NULL buffer");
    return FBX_OK;
}

static int settings_expected(int n, int kind, int64_t* m) {       // m of an exhaustive experiment, or -1 when it is 2^31 or more
    const int bits = kind == FBX_KIND_PROCESS ? 3 * n : n;
    if (bits > 31) { *m = -1; return FBX_OK; }
    const int64_t v = kind == FBX_KIND_PROCESS ? ((((int64_t)1 << (2 * n)) - 1) << n) : (((int64_t)1 << n) - 1);
    *m = v < ((int64_t)1 << 31) ? v : -1;
    return FBX_OK;
}

static int settings_check(int n, int kind, int64_t n_terms, int64_t G, const void* gates, int64_t m, const void* in_x,
                          const void* in_z, const void* in_minus, const void* obs_x, const void* obs_z, const void* obs_sign) {
    FBX_TRY(dfe_check_circuit("fbx_dfe_settings", n, G, gates));
    FBX_REQUIRE(kind == FBX_KIND_STATE || kind == FBX_KIND_PROCESS, "fbx_dfe_settings: kind must be FBX_KIND_STATE or FBX_KIND_PROCESS");
    FBX_REQUIRE(n_terms >= 0 && m >= 0, "fbx_dfe_settings: negative size");
    if (n_terms == 0) {
        int64_t want = 0;
        FBX_TRY(settings_expected(n, kind, &want));
        FBX_REQUIRE(want >= 0, "fbx_dfe_settings: an exhaustive experiment of this width has 2^31 settings or more; use n_terms > 0");
        FBX_REQUIRE(m == want, "fbx_dfe_settings: an exhaustive experiment has m = 2^n - 1 (state) or (4^n - 1) 2^n (process) settings");
    } else {
        FBX_REQUIRE(m == n_terms, "fbx_dfe_settings: a Monte Carlo experiment has m = n_terms settings");
    }
    FBX_REQUIRE(m == 0 || (in_x && in_z && in_minus && obs_x && obs_z && obs_sign), "fbx_dfe_settings: NULL buffer");
    return FBX_OK;
}

static int propagate_check(int n, int64_t G, const void* gates, int K, int64_t m, const void* in_x, const void* in_z,
                           const void* in_minus, const void* obs_x, const void* obs_z, const void* sigma, const void* touches) {
    FBX_TRY(dfe_check_circuit("fbx_dfe_propagate", n, G, gates));
    FBX_REQUIRE(K >= 1 && K <= DFE_MAX_CLASSES, "fbx_dfe_propagate: K must be 1..16");
    FBX_REQUIRE(m >= 0, "fbx_dfe_propagate: negative m");
    FBX_REQUIRE(m == 0 || (in_x && in_z && in_minus && obs_x && obs_z && sigma && touches), "fbx_dfe_propagate: NULL buffer");
    return FBX_OK;
}

static int simulate_check(const char* who, int n, int64_t m, int K, const void* sigma, const void* touches, const void* obs_x,
                          const void* obs_z, const void* obs_sign, int64_t B, int64_t n_shots, int64_t first_item) {
    FBX_TRY(dfe_check_width(who, n));
    const std::string w(who);
    if (K < 1 || K > DFE_MAX_CLASSES) { set_error(w + ": K must be 1..16"); return FBX_ERR_BAD_ARG; }
    if (m < 0 || B < 0 || n_shots < 0 || first_item < 0) { set_error(w + ": need m >= 0, B >= 0, n_shots >= 0 and first_item >= 0"); return FBX_ERR_BAD_ARG; }
    if (n_shots >= ((int64_t)1 << 32)) { set_error(w + ": n_shots must be below 2^32"); return FBX_ERR_BAD_ARG; }
    if (m >= ((int64_t)1 << 32)) { set_error(w + ": m must be below 2^32 (the setting index is one counter word)"); return FBX_ERR_BAD_ARG; }
    if (m > 0 && !(sigma && touches && obs_x && obs_z && obs_sign)) { set_error(w + ": NULL buffer"); return FBX_ERR_BAD_ARG; }
    if (m > 0 && B > INT64_MAX / 64 / m) { set_error(w + ": B * m overflows"); return FBX_ERR_BAD_ARG; }
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_clifford_conjugate_dev(int n_qubits, int64_t G, const uint32_t* d_gates, int inverse, int64_t M, const uint64_t* d_x_in,
                               const uint64_t* d_z_in, const uint8_t* d_sign_in, uint64_t* d_x_out, uint64_t* d_z_out,
                               uint8_t* d_sign_out) {
    FBX_TRY(conjugate_check(n_qubits, G, d_gates, M, d_x_in, d_z_in, d_sign_in, d_x_out, d_z_out, d_sign_out));
    unsigned blocks = 0;
    FBX_TRY(dfe_blocks("fbx_clifford_conjugate", M, &blocks));
    FBX_TRY(ensure_device());
    if (M == 0) return FBX_OK;
    hipLaunchKernelGGL(conjugate_kernel, dim3(blocks), dim3(DFE_THREADS), 0, stream(), n_qubits, (long long)G, d_gates,
                       inverse ? 1 : 0, (long long)M, d_x_in, d_z_in, d_sign_in, d_x_out, d_z_out, d_sign_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_clifford_conjugate(int n_qubits, int64_t G, const uint32_t* gates, int inverse, int64_t M, const uint64_t* x_in,
                           const uint64_t* z_in, const uint8_t* sign_in, uint64_t* x_out, uint64_t* z_out, uint8_t* sign_out) {
    FBX_TRY(conjugate_check(n_qubits, G, gates, M, x_in, z_in, sign_in, x_out, z_out, sign_out));
    FBX_TRY(dfe_check_gates("fbx_clifford_conjugate", n_qubits, G, gates));
    FBX_TRY(ensure_device());
    if (M == 0) return FBX_OK;
    HostIO io; uint32_t* dg; uint64_t *dx, *dz, *dxo, *dzo; uint8_t *ds, *dso;
    FBX_TRY(io.in(gates, (size_t)G, &dg));
    FBX_TRY(io.in(x_in, (size_t)M, &dx)); FBX_TRY(io.in(z_in, (size_t)M, &dz)); FBX_TRY(io.in(sign_in, (size_t)M, &ds));
    FBX_TRY(io.out(x_out, (size_t)M, &dxo)); FBX_TRY(io.out(z_out, (size_t)M, &dzo)); FBX_TRY(io.out(sign_out, (size_t)M, &dso));
    FBX_TRY(fbx_clifford_conjugate_dev(n_qubits, G, dg, inverse, M, dx, dz, ds, dxo, dzo, dso));
    return io.finish();
}

int fbx_dfe_settings_dev(int n_qubits, int kind, int64_t n_terms, uint64_t seed, int64_t G, const uint32_t* d_gates, int64_t m,
                         uint64_t* d_in_x, uint64_t* d_in_z, uint64_t* d_in_minus, uint64_t* d_obs_x, uint64_t* d_obs_z,
                         uint8_t* d_obs_sign) {
    FBX_TRY(settings_check(n_qubits, kind, n_terms, G, d_gates, m, d_in_x, d_in_z, d_in_minus, d_obs_x, d_obs_z, d_obs_sign));
    unsigned blocks = 0;
    FBX_TRY(dfe_blocks("fbx_dfe_settings", m, &blocks));
    FBX_TRY(ensure_device());
    if (m == 0) return FBX_OK;
    hipLaunchKernelGGL(settings_kernel, dim3(blocks), dim3(DFE_THREADS), 0, stream(), n_qubits, kind == FBX_KIND_PROCESS ? 1 : 0,
                       (long long)n_terms, (unsigned long long)seed, (long long)G, d_gates, (long long)m, d_in_x, d_in_z, d_in_minus,
                       d_obs_x, d_obs_z, d_obs_sign);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_dfe_settings(int n_qubits, int kind, int64_t n_terms, uint64_t seed, int64_t G, const uint32_t* gates, int64_t m,
                     uint64_t* in_x, uint64_t* in_z, uint64_t* in_minus, uint64_t* obs_x, uint64_t* obs_z, uint8_t* obs_sign) {
    FBX_TRY(settings_check(n_qubits, kind, n_terms, G, gates, m, in_x, in_z, in_minus, obs_x, obs_z, obs_sign));
    FBX_TRY(dfe_check_gates("fbx_dfe_settings", n_qubits, G, gates));
    FBX_TRY(ensure_device());
    if (m == 0) return FBX_OK;
    const size_t sm = (size_t)m;
    HostIO io; uint32_t* dg; uint64_t *dix, *diz, *dim_, *dox, *doz; uint8_t* dos;
    FBX_TRY(io.in(gates, (size_t)G, &dg));
    FBX_TRY(io.out(in_x, sm, &dix)); FBX_TRY(io.out(in_z, sm, &diz)); FBX_TRY(io.out(in_minus, sm, &dim_));
    FBX_TRY(io.out(obs_x, sm, &dox)); FBX_TRY(io.out(obs_z, sm, &doz)); FBX_TRY(io.out(obs_sign, sm, &dos));
    FBX_TRY(fbx_dfe_settings_dev(n_qubits, kind, n_terms, seed, G, dg, m, dix, diz, dim_, dox, doz, dos));
    return io.finish();
}

int fbx_dfe_propagate_dev(int n_qubits, int64_t G, const uint32_t* d_gates, const uint8_t* d_noise_class, int K, int64_t m,
                          const uint64_t* d_in_x, const uint64_t* d_in_z, const uint64_t* d_in_minus, const uint64_t* d_obs_x,
                          const uint64_t* d_obs_z, const uint8_t* d_obs_sign, int8_t* d_sigma_out, uint32_t* d_touches_out) {
    (void)d_obs_sign;                                    // sigma belongs to the unsigned observable
    FBX_TRY(propagate_check(n_qubits, G, d_gates, K, m, d_in_x, d_in_z, d_in_minus, d_obs_x, d_obs_z, d_sigma_out, d_touches_out));
    unsigned blocks = 0;
    FBX_TRY(dfe_blocks("fbx_dfe_propagate", m, &blocks));
    FBX_TRY(ensure_device());
    if (m == 0) return FBX_OK;
#define FBX_DFE_PROPAGATE(KK) hipLaunchKernelGGL(propagate_kernel<KK>, dim3(blocks), dim3(DFE_THREADS), 0, stream(), n_qubits, \
                                                 (long long)G, d_gates, d_noise_class, K, (long long)m, d_in_x, d_in_z, d_in_minus, \
                                                 d_obs_x, d_obs_z, d_sigma_out, d_touches_out)
    if (K == 1) FBX_DFE_PROPAGATE(1); else if (K <= 4) FBX_DFE_PROPAGATE(4); else FBX_DFE_PROPAGATE(16);
#undef FBX_DFE_PROPAGATE
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_dfe_propagate(int n_qubits, int64_t G, const uint32_t* gates, const uint8_t* noise_class, int K, int64_t m,
                      const uint64_t* in_x, const uint64_t* in_z, const uint64_t* in_minus, const uint64_t* obs_x,
                      const uint64_t* obs_z, const uint8_t* obs_sign, int8_t* sigma_out, uint32_t* touches_out) {
    (void)obs_sign;
    FBX_TRY(propagate_check(n_qubits, G, gates, K, m, in_x, in_z, in_minus, obs_x, obs_z, sigma_out, touches_out));
    FBX_TRY(dfe_check_gates("fbx_dfe_propagate", n_qubits, G, gates));
    FBX_TRY(dfe_check_classes("fbx_dfe_propagate", K, G, noise_class));
    const uint64_t valid = dfe_valid_mask(n_qubits);
    for (int64_t k = 0; k < m; ++k)
        FBX_REQUIRE(((in_x[k] | in_z[k]) & valid) == valid, "fbx_dfe_propagate: an in-state label is I (every qubit is prepared in an X, Y or Z eigenstate)");
    FBX_TRY(ensure_device());
    if (m == 0) return FBX_OK;
    const size_t sm = (size_t)m;
    HostIO io; uint32_t *dg, *dt; uint8_t* dc = nullptr; uint64_t *dix, *diz, *dim_, *dox, *doz; int8_t* dsg;
    FBX_TRY(io.in(gates, (size_t)G, &dg));
    if (noise_class) FBX_TRY(io.in(noise_class, (size_t)G, &dc));
    FBX_TRY(io.in(in_x, sm, &dix)); FBX_TRY(io.in(in_z, sm, &diz)); FBX_TRY(io.in(in_minus, sm, &dim_));
    FBX_TRY(io.in(obs_x, sm, &dox)); FBX_TRY(io.in(obs_z, sm, &doz));
    FBX_TRY(io.out(sigma_out, sm, &dsg)); FBX_TRY(io.out(touches_out, sm * (size_t)K, &dt));
    FBX_TRY(fbx_dfe_propagate_dev(n_qubits, G, dg, dc, K, m, dix, diz, dim_, dox, doz, nullptr, dsg, dt));
    return io.finish();
}

// poison status and one simulation (plain or calibration) on the calling thread's stream; `status` is a device buffer [B]
static int dfe_simulate_launch(int n, int64_t m, int K, const int8_t* sigma, const uint32_t* touches, const uint64_t* obs_x,
                               const uint64_t* obs_z, const uint8_t* obs_sign, int64_t B, const double* class_error,
                               const double* flips, int calibration, int64_t n_shots, uint64_t seed, int64_t first_item,
                               double* expect, double* counts, double* std_err, double* exact, int32_t* status, bool write_status) {
    constexpr int WAVES = DFE_THREADS / 64;
    if (write_status) {
        hipLaunchKernelGGL(dfe_poison_kernel, dim3((unsigned)((B + WAVES - 1) / WAVES)), dim3(DFE_THREADS), 0, stream(), (long long)B,
                           K, n, class_error, flips, status);
        FBX_HIP(hipGetLastError());
    }
    const int64_t units = B * m;
    const bool lane = units >= FBX_TOMO_LANE_MIN_UNITS;
    const int64_t blocks = lane ? (units + DFE_THREADS - 1) / DFE_THREADS : (units + WAVES - 1) / WAVES;
    FBX_REQUIRE(blocks < ((int64_t)1 << 31), "fbx_dfe_simulate: B * m is beyond one launch; cut the batch with first_item");
#define FBX_DFE_SIM(L) hipLaunchKernelGGL(dfe_sim_kernel<L>, dim3((unsigned)blocks), dim3(DFE_THREADS), 0, stream(), n, (long long)m, K, \
                                          sigma, touches, obs_x, obs_z, obs_sign, (long long)B, class_error, flips, calibration ? 1 : 0, \
                                          (unsigned)n_shots, (unsigned long long)seed, (long long)first_item, (const int*)status, \
                                          expect, counts, std_err, exact)
    if (lane) FBX_DFE_SIM(true); else FBX_DFE_SIM(false);
#undef FBX_DFE_SIM
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

static int dfe_simulate_check(int n, int64_t m, int K, const void* sigma, const void* touches, const void* obs_x, const void* obs_z,
                              const void* obs_sign, int64_t B, int64_t n_shots, int64_t first_item, const void* expect,
                              const void* counts, const void* std_err, const void* exact) {
    FBX_TRY(simulate_check("fbx_dfe_simulate", n, m, K, sigma, touches, obs_x, obs_z, obs_sign, B, n_shots, first_item));
    FBX_REQUIRE(expect || counts || std_err || exact, "fbx_dfe_simulate: every output is NULL");
    FBX_REQUIRE(n_shots > 0 || !(expect || counts || std_err),
                "fbx_dfe_simulate: n_shots == 0 gives exact_out only (expect_out, counts_out and std_err_out must be NULL)");
    return FBX_OK;
}

int fbx_dfe_simulate_dev(int n_qubits, int64_t m, int K, const int8_t* d_sigma, const uint32_t* d_touches, const uint64_t* d_obs_x,
                         const uint64_t* d_obs_z, const uint8_t* d_obs_sign, int64_t B, const double* d_class_error,
                         const double* d_readout_flip, int calibration, int64_t n_shots, uint64_t seed, int64_t first_item,
                         double* d_expect_out, double* d_counts_out, double* d_std_err_out, double* d_exact_out,
                         int32_t* d_status_out) {
    FBX_TRY(dfe_simulate_check(n_qubits, m, K, d_sigma, d_touches, d_obs_x, d_obs_z, d_obs_sign, B, n_shots, first_item, d_expect_out,
                               d_counts_out, d_std_err_out, d_exact_out));
    FBX_TRY(ensure_device());
    if (B == 0 || m == 0) return FBX_OK;
    StatusBuf status;
    FBX_TRY(status.take(d_status_out, B));
    return dfe_simulate_launch(n_qubits, m, K, d_sigma, d_touches, d_obs_x, d_obs_z, d_obs_sign, B, d_class_error, d_readout_flip,
                               calibration, n_shots, seed, first_item, d_expect_out, d_counts_out, d_std_err_out, d_exact_out,
                               status.p, true);
}

// the settings and noise of a simulate call, uploaded
struct DfeSimInputs {
    int8_t* sigma; uint32_t* touches; uint64_t *obs_x, *obs_z; uint8_t* obs_sign; double *class_error = nullptr, *flips = nullptr;
    int upload(HostIO& io, int n, int64_t m, int K, const int8_t* h_sigma, const uint32_t* h_touches, const uint64_t* h_obs_x,
               const uint64_t* h_obs_z, const uint8_t* h_obs_sign, int64_t B, const double* h_class_error, const double* h_flips) {
        const size_t sm = (size_t)m, sb = (size_t)B;
        FBX_TRY(io.in(h_sigma, sm, &sigma)); FBX_TRY(io.in(h_touches, sm * (size_t)K, &touches));
        FBX_TRY(io.in(h_obs_x, sm, &obs_x)); FBX_TRY(io.in(h_obs_z, sm, &obs_z)); FBX_TRY(io.in(h_obs_sign, sm, &obs_sign));
        if (h_class_error) FBX_TRY(io.in(h_class_error, sb * (size_t)K, &class_error));
        if (h_flips) FBX_TRY(io.in(h_flips, sb * (size_t)n, &flips));
        return FBX_OK;
    }
};

int fbx_dfe_simulate(int n_qubits, int64_t m, int K, const int8_t* sigma, const uint32_t* touches, const uint64_t* obs_x,
                     const uint64_t* obs_z, const uint8_t* obs_sign, int64_t B, const double* class_error, const double* readout_flip,
                     int calibration, int64_t n_shots, uint64_t seed, int64_t first_item, double* expect_out, double* counts_out,
                     double* std_err_out, double* exact_out, int32_t* status_out) {
    FBX_TRY(dfe_simulate_check(n_qubits, m, K, sigma, touches, obs_x, obs_z, obs_sign, B, n_shots, first_item, expect_out, counts_out,
                               std_err_out, exact_out));
    FBX_TRY(ensure_device());
    if (B == 0 || m == 0) return FBX_OK;
    const size_t units = (size_t)B * (size_t)m;
    HostIO io; DfeSimInputs in; SimOut o;
    FBX_TRY(in.upload(io, n_qubits, m, K, sigma, touches, obs_x, obs_z, obs_sign, B, class_error, readout_flip));
    FBX_TRY(o.stage(io, (size_t)B, units, expect_out, counts_out, std_err_out, exact_out, status_out));
    FBX_TRY(fbx_dfe_simulate_dev(n_qubits, m, K, in.sigma, in.touches, in.obs_x, in.obs_z, in.obs_sign, B, in.class_error, in.flips,
                                 calibration, n_shots, seed, first_item, o.expect, o.counts, o.std_err, o.exact, o.status));
    return io.finish();
}

static int dfe_chain_check(int n, int64_t m, int K, const void* sigma, const void* touches, const void* obs_x, const void* obs_z,
                           const void* obs_sign, int64_t B, int64_t n_shots, int64_t first_item, int kind, const void* fidelity,
                           const void* err) {
    FBX_TRY(simulate_check("fbx_dfe_simulate_fidelity", n, m, K, sigma, touches, obs_x, obs_z, obs_sign, B, n_shots, first_item));
    FBX_REQUIRE(kind == FBX_KIND_STATE || kind == FBX_KIND_PROCESS, "fbx_dfe_simulate_fidelity: kind must be FBX_KIND_STATE or FBX_KIND_PROCESS");
    FBX_REQUIRE(m >= 1 && n_shots >= 1, "fbx_dfe_simulate_fidelity: need m >= 1 and n_shots >= 1");
    FBX_REQUIRE(B == 0 || (fidelity && err), "fbx_dfe_simulate_fidelity: NULL output");
    return FBX_OK;
}

int fbx_dfe_simulate_fidelity_dev(int n_qubits, int64_t m, int K, const int8_t* d_sigma, const uint32_t* d_touches,
                                  const uint64_t* d_obs_x, const uint64_t* d_obs_z, const uint8_t* d_obs_sign, int64_t B,
                                  const double* d_class_error, const double* d_readout_flip, int64_t n_shots, uint64_t seed,
                                  int64_t first_item, int kind, int calibrate, double* d_fidelity_out, double* d_err_out,
                                  int32_t* d_status_out) {
    FBX_TRY(dfe_chain_check(n_qubits, m, K, d_sigma, d_touches, d_obs_x, d_obs_z, d_obs_sign, B, n_shots, first_item, kind,
                            d_fidelity_out, d_err_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t units = (size_t)B * (size_t)m;
    DevBuf work;                                       // [B][m] doubles: e, se (and the calibration's e, se, the corrected e, se)
    FBX_TRY(work.alloc(sizeof(double) * units * (calibrate ? 6 : 2)));
    double* e = work.as<double>(); double* se = e + units;
    StatusBuf status_buf;
    FBX_TRY(status_buf.take(d_status_out, B));
    int32_t* status = status_buf.p;
    FBX_TRY(dfe_simulate_launch(n_qubits, m, K, d_sigma, d_touches, d_obs_x, d_obs_z, d_obs_sign, B, d_class_error, d_readout_flip, 0,
                                n_shots, seed, first_item, e, nullptr, se, nullptr, status, true));
    if (calibrate) {
        double *ce = se + units, *cv = ce + units, *e2 = cv + units, *se2 = e2 + units;
        FBX_TRY(dfe_simulate_launch(n_qubits, m, K, d_sigma, d_touches, d_obs_x, d_obs_z, d_obs_sign, B, d_class_error,
                                    d_readout_flip, 1, n_shots, seed, first_item, ce, nullptr, cv, nullptr, status, false));
        const int64_t want = ((int64_t)units + DFE_THREADS - 1) / DFE_THREADS;
        hipLaunchKernelGGL(dfe_square_kernel, dim3((unsigned)(want < 256 * 32 ? want : 256 * 32)), dim3(DFE_THREADS), 0, stream(),
                           (long long)units, cv);
        FBX_HIP(hipGetLastError());
        // every (item, setting) has a calibration of its own: one "experiment" of B m settings, one calibration per setting
        FBX_TRY(fbx_calibrate_expectations_dev(1, (int64_t)units, e, se, nullptr, (int64_t)units, ce, cv, e2, se2));
        e = e2; se = se2;
    }
    hipLaunchKernelGGL(dfe_fidelity_kernel, dim3((unsigned)(B < 65536 ? B : 65536)), dim3(64), 0, stream(), ldexp(1.0, n_qubits),
                       kind == FBX_KIND_PROCESS ? 1 : 0, (long long)B, (long long)m, (const double*)e, (const double*)se,
                       d_fidelity_out, d_err_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_dfe_simulate_fidelity(int n_qubits, int64_t m, int K, const int8_t* sigma, const uint32_t* touches, const uint64_t* obs_x,
                              const uint64_t* obs_z, const uint8_t* obs_sign, int64_t B, const double* class_error,
                              const double* readout_flip, int64_t n_shots, uint64_t seed, int64_t first_item, int kind, int calibrate,
                              double* fidelity_out, double* err_out, int32_t* status_out) {
    FBX_TRY(dfe_chain_check(n_qubits, m, K, sigma, touches, obs_x, obs_z, obs_sign, B, n_shots, first_item, kind, fidelity_out,
                            err_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    HostIO io; DfeSimInputs in; double *df, *dr; int32_t* dst;
    FBX_TRY(in.upload(io, n_qubits, m, K, sigma, touches, obs_x, obs_z, obs_sign, B, class_error, readout_flip));
    FBX_TRY(io.out(fidelity_out, (size_t)B, &df)); FBX_TRY(io.out(err_out, (size_t)B, &dr));
    FBX_TRY(io.out_opt(status_out, (size_t)B, &dst));
    FBX_TRY(fbx_dfe_simulate_fidelity_dev(n_qubits, m, K, in.sigma, in.touches, in.obs_x, in.obs_z, in.obs_sign, B, in.class_error,
                                          in.flips, n_shots, seed, first_item, kind, calibrate, df, dr, dst));
    return io.finish();
}

}  // fbx C ABI
