// fbx_native.hip -- a circuit of native gates (I, RX, RZ, CZ, XY: what fbx.compilation.basic_compile emits) on a state vector of
// 1..13 qubits, with a Pauli error after every gate (include/fbx.h).
//
// fbx_native_trajectories: ONE circuit for B items of noise x P input words x T trajectories.  The structure is that of
// fbx_qvolume_noisy.hip: the whole state in LDS behind qv_slot, one wavefront per unit at widths 1..NAT_WAVE_MAX_QUBITS (four per
// workgroup, no workgroup barrier), one workgroup per unit above; the unit of work is (item b, input r, segment s of NAT_SEG
// consecutive trajectories), a thread owns the outputs tid, tid + nth, ... and keeps their running sums over the segment in
// registers, the partial sums go to the workspace WS_NATIVE [chunk of (b, r)][nseg][2^n], and nat_mean_kernel adds, per output of
// the marginal, its amplitudes in ascending index order -- each the sum of its segments in the order of s -- and divides by T: the
// order depends on T and the circuit's width alone, and no floating-point atomic is involved.  Without probs_mean_out every
// trajectory is a unit and nothing is summed.
//
// What differs from the quantum-volume kernel is the gate (fbx_native_gate.hpp: a pass per opcode, none of them a 4 x 4 product)
// and where a gate's numbers come from: the word, its noise class and the (cos, sin) of its half angle -- computed once per call by
// nat_table_kernel -- are read through `const __restrict__` kernel arguments at wave-uniform indices, i.e. as scalars.  A Philox
// block is computed only where a gate with a positive error probability needs it.  fbx_native_unitary runs the same gate loop
// without noise, a unit per column.
#include <algorithm>
#include <cmath>
#include "fbx_clifford_gates.hpp"
#include "fbx_native_gate.hpp"

namespace fbx {

constexpr uint32_t NAT_KEY_TAG = 0x4E415456u;           // "NATV": the key tag of this stream (include/fbx.h)
constexpr int NAT_SEG = 8;                              // trajectories per partial sum; part of the summation order of probs_mean_out
constexpr int NAT_WAVE_MAX_QUBITS = FBX_NAT_WAVE_MAX_QUBITS;

// the fields of a word (include/fbx.h)
__host__ __device__ __forceinline__ uint32_t nat_op(uint32_t w) { return w & 7u; }
__host__ __device__ __forceinline__ uint32_t nat_q0(uint32_t w) { return (w >> 3) & 15u; }
__host__ __device__ __forceinline__ uint32_t nat_q1(uint32_t w) { return (w >> 7) & 15u; }
__host__ __device__ __forceinline__ uint32_t nat_conditional(uint32_t w) { return (w >> 11) & 1u; }
__host__ __device__ __forceinline__ uint32_t nat_input_bit(uint32_t w) { return (w >> 12) & 63u; }
__host__ __device__ __forceinline__ bool nat_two_qubit(uint32_t op) { return op == FBX_NAT_CZ || op == FBX_NAT_XY; }

#if defined(__HIPCC__)

template <bool WAVE>
__device__ __forceinline__ void nat_sync() {
    if constexpr (WAVE) FBX_WAVE_SYNC(); else __syncthreads();
}

// the circuit and the tables every unit reads: kernel arguments of their own (scalar loads)
#define NAT_CIRCUIT_PARAMS const uint32_t* __restrict__ words, const double* __restrict__ cs /* [G][2]: cos, sin of angle / 2 */, \
                           const int* __restrict__ bad_angle /* [1]: an angle was not finite */
#define NAT_CIRCUIT_ARGS words, cs, bad_angle

// The gates of the circuit on the state S of 2^n slots, one after the other, by the team of nth threads.  ce: the K class errors
// of the item, or NULL for no noise; the Philox counter of gate l is (c0, c1, c2, l >> 1).  Returns 1 when a word does not fit
// the width (the gate is skipped: no access leaves the state), adds the gates that erred to nerr.  Everything here but the passes
// over S is wave-uniform.
template <bool WAVE>
__device__ __forceinline__ unsigned nat_run(int n, long long G, NAT_CIRCUIT_PARAMS, const uint8_t* __restrict__ noise_class,
                                            const double* __restrict__ ce, int K, unsigned long long input, uint32_t c0, uint32_t c1,
                                            uint32_t c2, uint32_t k0, uint32_t k1, cplx* S, int tid, int nth, int& nerr) {
    const int N = 1 << n;
    unsigned bad = 0;
    uint32_t blk[4] = {0u, 0u, 0u, 0u};
    long long have = -1;                                            // the pair of gates whose block is in blk
    for (long long l = 0; l < G; ++l) {
        const uint32_t w = words[l], op = nat_op(w);
        const int q0 = (int)nat_q0(w), q1 = (int)nat_q1(w);
        const bool two = nat_two_qubit(op);
        if (op > FBX_NAT_XY || q0 >= n || (two && (q1 >= n || q1 == q0))) { bad = 1; continue; }
        if (nat_conditional(w) && !((input >> nat_input_bit(w)) & 1ull)) continue;      // the gate and its error site do not exist
        const int cls = noise_class ? (int)noise_class[l] : 0;
        const double p = (ce && cls < K) ? ce[cls] : 0.0;
        int x = 0, z = 0;
        if (p > 0.0) {
            if (have != (l >> 1)) {
                blk[0] = c0; blk[1] = c1; blk[2] = c2; blk[3] = (uint32_t)(l >> 1);
                philox4x32_10(blk, k0, k1);
                have = l >> 1;
            }
            const uint32_t first = (l & 1) ? blk[2] : blk[0], second = (l & 1) ? blk[3] : blk[1];
            if (uniform((int)((double)first * 0x1p-32 < p))) {
                ++nerr;
                if (two) {
                    const uint32_t idx = second >> 28, a = idx >> 2, b = idx & 3u;      // a on q0, b on q1; I X Y Z = 0 1 2 3
                    x = (int)(((((a + 1u) >> 1) & 1u) << 1) | (((b + 1u) >> 1) & 1u));  // X and Y flip the bit
                    z = (int)(((a >> 1) << 1) | (b >> 1));                              // Y and Z sign it
                } else {
                    const uint32_t d = second >> 30;
                    x = (int)(((d + 1u) >> 1) & 1u); z = (int)(d >> 1);
                }
            }
        }
        const double c = cs[2 * l], s = cs[2 * l + 1];
        const int p0 = n - 1 - q0, p1 = n - 1 - q1;
        switch (op) {
            case FBX_NAT_I:
                if (!(x | z)) continue;                             // nothing to do, and no barrier to meet
                nat_apply_rx(S, N >> 1, p0, 1.0, 0.0, x, z, tid, nth);
                break;
            case FBX_NAT_RX: nat_apply_rx(S, N >> 1, p0, c, s, x, z, tid, nth); break;
            case FBX_NAT_RZ:
                if (x) nat_apply_rz_x(S, N >> 1, p0, c, s, z, tid, nth); else nat_apply_rz(S, N, p0, c, s, z, tid, nth);
                break;
            case FBX_NAT_CZ:
                if (x) nat_apply_group<false>(S, N >> 2, p0, p1, 1.0, 0.0, x, z, tid, nth); else nat_apply_cz(S, N, p0, p1, z, tid, nth);
                break;
            default: nat_apply_group<true>(S, N >> 2, p0, p1, c, s, x, z, tid, nth); break;
        }
        nat_sync<WAVE>();
    }
    return bad;
}

// the scalars of a trajectory launch
struct NatArgs {
    int n, K, seg;
    long long G, P, T, nseg, units, br0, first_item, first_input;
    uint32_t k0, k1;
};

#define NAT_POINTER_PARAMS                                                                                                    \
    NAT_CIRCUIT_PARAMS, const uint8_t* __restrict__ noise_class, const unsigned long long* __restrict__ inputs,              \
    const double* __restrict__ class_error, double* __restrict__ part /* [units][2^n] of this launch, or NULL */,            \
    int* __restrict__ nerr_out, int* __restrict__ status
#define NAT_POINTER_ARGS NAT_CIRCUIT_ARGS, noise_class, inputs, class_error, part, nerr_out, status

// One team runs unit u of the launch: segment s of the pair br = (item b, input r).  OWN: the outputs a thread owns, 2^n / nth
// rounded up; MEAN: running sums over the unit's trajectories are kept and stored.
template <bool WAVE, bool MEAN, int OWN>
__device__ void nat_unit(const NatArgs& A, NAT_POINTER_PARAMS, long long u, cplx* S, int tid, int nth) {
    const int n = A.n, N = 1 << n;
    const long long pr = u / A.nseg, s = u - pr * A.nseg, br = A.br0 + pr, b = br / A.P, r = br - b * A.P;
    const long long t_begin = s * A.seg, t_end = t_begin + A.seg < A.T ? t_begin + A.seg : A.T;
    const double* ce = class_error ? class_error + b * A.K : nullptr;
    unsigned bad_unit = bad_angle[0] != 0 ? 1u : 0u;
    if (ce)
        for (int k = 0; k < A.K; ++k) bad_unit |= dfe_bad_probability(ce[k]) ? 1u : 0u;
    const unsigned long long input = inputs[r];
    const uint32_t c0 = (uint32_t)(unsigned long long)(A.first_item + b), c1 = (uint32_t)(unsigned long long)(A.first_input + r);
    double acc[MEAN ? OWN : 1];
#pragma unroll
    for (int k = 0; k < (MEAN ? OWN : 1); ++k) acc[k] = 0.0;
    for (long long t = t_begin; t < t_end; ++t) {
        int nerr = 0;
        if (!bad_unit) {                                            // wave-uniform, and the same in every wavefront of the team
            for (int i = tid; i < N; i += nth) S[i] = cplx{i == 0 ? 1.0 : 0.0, 0.0};      // slot 0 = element 0
            nat_sync<WAVE>();
            bad_unit |= nat_run<WAVE>(n, A.G, NAT_CIRCUIT_ARGS, noise_class, ce, A.K, input, c0, c1, (uint32_t)t, A.k0, A.k1, S, tid,
                                      nth, nerr);
            if constexpr (MEAN) {
#pragma unroll
                for (int k = 0; k < OWN; ++k) {
                    const int i = tid + k * nth;
                    if (i < N) { const cplx a = S[qv_slot(i)]; acc[k] += a.re * a.re + a.im * a.im; }
                }
            }
            nat_sync<WAVE>();                                       // every read of the state is done before the next trajectory resets it
        }
        if (nerr_out && tid == 0) nerr_out[(b * A.P + r) * A.T + t] = bad_unit ? 0 : nerr;
    }
    if constexpr (MEAN) {
        double* dst = part + (size_t)u * N;
#pragma unroll
        for (int k = 0; k < OWN; ++k) {
            const int i = tid + k * nth;
            if (i < N) dst[i] = bad_unit ? __builtin_nan("") : acc[k];
        }
    }
    if (status && r == 0 && s == 0 && tid == 0) status[b] = (int)bad_unit;
}

extern __shared__ __attribute__((aligned(16))) unsigned char nat_lds[];

// widths above NAT_WAVE_MAX_QUBITS: one workgroup per unit
template <bool MEAN, int OWN>
__global__ void __launch_bounds__(1024) nat_block_kernel(NatArgs A, NAT_POINTER_PARAMS) {
    cplx* S = reinterpret_cast<cplx*>(nat_lds);
    for (long long u = blockIdx.x; u < A.units; u += gridDim.x)
        nat_unit<false, MEAN, OWN>(A, NAT_POINTER_ARGS, u, S, (int)threadIdx.x, (int)blockDim.x);
}

// widths 1..NAT_WAVE_MAX_QUBITS: one wavefront per unit, four per workgroup
template <bool MEAN>
__global__ void __launch_bounds__(256) nat_wave_kernel(NatArgs A, NAT_POINTER_PARAMS) {
    const int wave = uniform((int)(threadIdx.x >> 6));
    cplx* S = reinterpret_cast<cplx*>(nat_lds + (sizeof(cplx) << A.n) * wave);
    for (long long u = (long long)blockIdx.x * 4 + wave; u < A.units; u += (long long)gridDim.x * 4)
        nat_unit<true, MEAN, (1 << NAT_WAVE_MAX_QUBITS) / 64>(A, NAT_POINTER_ARGS, u, S, (int)(threadIdx.x & 63), 64);
}

// probs_mean_out of `count` = pairs x 2^m outputs.  Output j of a pair: column c of out_qubits is bit m - 1 - c of j and sits at
// index bit n - 1 - out_qubits[c]; the amplitudes with those bits run through the other index bits in ascending order.  An entry
// of out_qubits that is not below n or repeats gives NaN (the _dev form does not check them): no read leaves the workspace.
__global__ void __launch_bounds__(256) nat_mean_kernel(int n, int m, const uint8_t* __restrict__ out_qubits, long long count, long long nseg,
                                                       long long T, const double* __restrict__ part, double* __restrict__ out) {
    const long long N = 1ll << n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (long long)gridDim.x * 256) {
        const long long pr = idx >> m;
        const int j = (int)(idx & ((1ll << m) - 1));
        int used = 0, base = 0;
        bool ok = true;
        for (int c = 0; c < m; ++c) {
            const int q = out_qubits[c];
            if (q >= n) { ok = false; continue; }
            const int p = n - 1 - q;
            if ((used >> p) & 1) ok = false;
            used |= 1 << p;
            base |= ((j >> (m - 1 - c)) & 1) << p;
        }
        if (!ok) { out[idx] = __builtin_nan(""); continue; }
        const int rest = ((int)N - 1) & ~used;
        const double* p0 = part + (size_t)(pr * nseg) * N;
        double sum = 0.0;
        int sub = 0;
        do {                                                        // the subsets of `rest` in ascending order
            const double* p = p0 + (base | sub);
            double amp = 0.0;
            for (long long s = 0; s < nseg; ++s) amp += p[(size_t)s * N];
            sum += amp;
            sub = (sub - rest) & rest;
        } while (sub != 0);
        out[idx] = sum / (double)T;
    }
}

// (cos, sin) of every gate's half angle, once per call; *bad = 1 when an angle is not finite (an integer atomic)
__global__ void __launch_bounds__(256) nat_table_kernel(long long G, const double* __restrict__ angles, double* __restrict__ cs,
                                                        int* __restrict__ bad) {
    for (long long l = (long long)blockIdx.x * 256 + threadIdx.x; l < G; l += (long long)gridDim.x * 256) {
        const double a = angles[l];
        if (!(fabs(a) < __builtin_inf())) atomicOr(bad, 1);
        cs[2 * l] = cos(0.5 * a); cs[2 * l + 1] = sin(0.5 * a);
    }
}

// fbx_native_unitary: unit j is column j.  Row and column indices have qubit 0 as their LEAST significant bit, the state index
// as its most significant one: both are bit-reversed on the way.  A column with a word that does not fit the width, or any
// column when an angle is not finite, is NaN.
template <bool WAVE>
__device__ void nat_column(int n, long long G, NAT_CIRCUIT_PARAMS, long long j, cplx* S, cplx* __restrict__ U, int tid, int nth) {
    const int N = 1 << n, i0 = (int)(__brev((unsigned)j) >> (32 - n));
    for (int i = tid; i < N; i += nth) S[qv_slot(i)] = cplx{i == i0 ? 1.0 : 0.0, 0.0};
    nat_sync<WAVE>();
    int nerr = 0;
    unsigned bad = bad_angle[0] != 0 ? 1u : 0u;
    bad |= nat_run<WAVE>(n, G, NAT_CIRCUIT_ARGS, nullptr, nullptr, 0, 0ull, 0u, 0u, 0u, 0u, 0u, S, tid, nth, nerr);
    const double nan = __builtin_nan("");
    for (int i = tid; i < N; i += nth) {
        const size_t row = __brev((unsigned)i) >> (32 - n);
        U[row * (size_t)N + (size_t)j] = bad ? cplx{nan, nan} : S[qv_slot(i)];
    }
    nat_sync<WAVE>();
}

__global__ void __launch_bounds__(1024) nat_unitary_block_kernel(int n, long long G, NAT_CIRCUIT_PARAMS, cplx* __restrict__ U) {
    cplx* S = reinterpret_cast<cplx*>(nat_lds);
    for (long long j = blockIdx.x; j < (1ll << n); j += gridDim.x) nat_column<false>(n, G, NAT_CIRCUIT_ARGS, j, S, U, (int)threadIdx.x, (int)blockDim.x);
}

__global__ void __launch_bounds__(256) nat_unitary_wave_kernel(int n, long long G, NAT_CIRCUIT_PARAMS, cplx* __restrict__ U) {
    const int wave = uniform((int)(threadIdx.x >> 6));
    cplx* S = reinterpret_cast<cplx*>(nat_lds + (sizeof(cplx) << n) * wave);
    for (long long j = (long long)blockIdx.x * 4 + wave; j < (1ll << n); j += (long long)gridDim.x * 4)
        nat_column<true>(n, G, NAT_CIRCUIT_ARGS, j, S, U, (int)(threadIdx.x & 63), 64);
}

#endif

// ------------------------------------------------------------------ host: argument checks
static int nat_check_width(const char* who, int n_qubits) {
    if (n_qubits < 1 || n_qubits > 13) {
        set_error(std::string(who) + ": n_qubits must be 1..13 (a wider state does not fit the LDS of one CU; got " + std::to_string(n_qubits) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    return FBX_OK;
}

static int nat_check(int n, int64_t G, const void* words, const void* angles, int K, int64_t P, const void* inputs, int m,
                     const void* out_qubits, int64_t B, int64_t T, int64_t first_item, int64_t first_input, const void* probs_mean,
                     const void* n_errors) {
    const char* who = "fbx_native_trajectories";
    const int64_t two32 = (int64_t)1 << 32;
    FBX_TRY(nat_check_width(who, n));
    FBX_REQUIRE(G >= 0 && G < ((int64_t)1 << 31), "fbx_native_trajectories: G must be 0 .. 2^31 - 1 (the gate pair is one counter word)");
    FBX_REQUIRE(G == 0 || (words && angles), "fbx_native_trajectories: NULL words / angles");
    FBX_REQUIRE(m >= 1 && m <= n, "fbx_native_trajectories: m must be 1..n_qubits");
    FBX_REQUIRE(K >= 1 && K <= DFE_MAX_CLASSES, "fbx_native_trajectories: K must be 1..16");
    FBX_REQUIRE(B >= 0 && P >= 0 && T >= 0 && first_item >= 0 && first_input >= 0,
                "fbx_native_trajectories: need B, P, T, first_item and first_input >= 0");
    FBX_REQUIRE(T < two32, "fbx_native_trajectories: T must be below 2^32 (the trajectory is one counter word of the stream)");
    FBX_REQUIRE(first_item <= two32 && B <= two32 - first_item && first_input <= two32 && P <= two32 - first_input,
                "fbx_native_trajectories: item and input indices must stay below 2^32 (each is one counter word)");
    FBX_REQUIRE(out_qubits, "fbx_native_trajectories: NULL out_qubits");
    FBX_REQUIRE(P == 0 || inputs, "fbx_native_trajectories: NULL inputs");
    FBX_REQUIRE(probs_mean || n_errors, "fbx_native_trajectories: probs_mean_out and n_errors_out are both NULL");
    FBX_REQUIRE(B == 0 || P <= INT64_MAX / 65536 / B, "fbx_native_trajectories: B * P overflows");
    return FBX_OK;
}

// a circuit given by HOST words and angles: the rule of include/fbx.h
static int nat_check_words(const char* who, int n, int64_t G, const uint32_t* words, const double* angles, bool conditionals) {
    for (int64_t g = 0; g < G; ++g) {
        const uint32_t w = words[g], op = nat_op(w);
        bool ok = op <= FBX_NAT_XY && (w >> 18) == 0 && nat_q0(w) < (uint32_t)n;
        if (nat_two_qubit(op)) ok = ok && nat_q1(w) < (uint32_t)n && nat_q1(w) != nat_q0(w); else ok = ok && nat_q1(w) == 0;
        if (!nat_conditional(w)) ok = ok && nat_input_bit(w) == 0;
        if (!ok) { set_error(std::string(who) + ": word " + std::to_string(g) + " is not a valid native-gate word for this width"); return FBX_ERR_BAD_ARG; }
        if (!conditionals && nat_conditional(w)) { set_error(std::string(who) + ": gate " + std::to_string(g) + " is conditional: a unitary has no input word"); return FBX_ERR_BAD_ARG; }
        if (!std::isfinite(angles[g])) { set_error(std::string(who) + ": the angle of gate " + std::to_string(g) + " is not finite"); return FBX_ERR_BAD_ARG; }
    }
    return FBX_OK;
}

// the table of a call: [G][2] doubles and the flag behind them, filled on the calling thread's stream
struct NatTable {
    DevBuf buf;
    double* cs = nullptr;
    int* bad = nullptr;
    int make(int64_t G, const double* d_angles) {
        FBX_TRY(buf.alloc(16 * (size_t)G + 16));
        cs = buf.as<double>();
        bad = reinterpret_cast<int*>(buf.as<unsigned char>() + 16 * (size_t)G);
        FBX_HIP(hipMemsetAsync(bad, 0, sizeof(int), stream()));
        if (G > 0) {
            const int64_t blocks = (G + 255) / 256;
            hipLaunchKernelGGL(nat_table_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream(), (long long)G, d_angles, cs, bad);
            FBX_HIP(hipGetLastError());
        }
        return FBX_OK;
    }
};

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_native_trajectories_dev(int n_qubits, int64_t G, const uint32_t* d_words, const double* d_angles, const uint8_t* d_noise_class,
                                int K, int64_t P, const uint64_t* d_inputs, int m, const uint8_t* d_out_qubits, int64_t B, int64_t T,
                                const double* d_class_error, uint64_t seed, int64_t first_item, int64_t first_input,
                                double* d_probs_mean_out, int32_t* d_n_errors_out, int32_t* d_status_out) {
    FBX_TRY(nat_check(n_qubits, G, d_words, d_angles, K, P, d_inputs, m, d_out_qubits, B, T, first_item, first_input, d_probs_mean_out,
                      d_n_errors_out));
    FBX_TRY(ensure_device());
    if (B == 0 || P == 0 || T == 0) return FBX_OK;
    const size_t N = (size_t)1 << n_qubits, state = sizeof(cplx) << n_qubits;
    NatTable table;
    FBX_TRY(table.make(G, d_angles));
    NatArgs A;
    A.n = n_qubits; A.K = K; A.G = G; A.P = P; A.T = T; A.first_item = first_item; A.first_input = first_input;
    A.seg = d_probs_mean_out ? NAT_SEG : 1;
    A.nseg = (T + A.seg - 1) / A.seg;
    A.k0 = (uint32_t)(seed & 0xFFFFFFFFull) ^ NAT_KEY_TAG; A.k1 = (uint32_t)(seed >> 32);
    const unsigned long long* d_in = (const unsigned long long*)d_inputs;
    double* part = nullptr;
    // the chunk: as many (item, input) pairs as the workspace cap admits partial sums for, at least one (all of them without probs_mean_out)
    const int64_t pairs = B * P;
    int64_t chunk = pairs;
    if (d_probs_mean_out) {
        const double per = 8.0 * (double)N * (double)A.nseg;
        chunk = (int64_t)(option_native_workspace_mib() * 1048576.0 / per);
        chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, pairs));
        void* ws = nullptr;
        FBX_TRY(workspace(WS_NATIVE, 8 * N * (size_t)A.nseg * (size_t)chunk, &ws));
        part = static_cast<double*>(ws);
    }
    for (int64_t br0 = 0; br0 < pairs; br0 += chunk) {
        const int64_t cb = std::min<int64_t>(chunk, pairs - br0);
        A.br0 = br0; A.units = cb * A.nseg;
        if (n_qubits <= NAT_WAVE_MAX_QUBITS) {
            const int64_t wgs = (A.units + 3) / 4;
            const unsigned grid = (unsigned)(wgs < 256 * 16 ? wgs : 256 * 16);
            hipLaunchKernelGGL(part ? nat_wave_kernel<true> : nat_wave_kernel<false>, dim3(grid), dim3(256), 4 * state, stream(), A, d_words,
                               (const double*)table.cs, (const int*)table.bad, d_noise_class, d_in, d_class_error, part, d_n_errors_out,
                               d_status_out);
        } else {
            const int groups = 1 << (n_qubits - 2);
            const unsigned threads = (unsigned)(groups < 1024 ? groups : 1024);
            const unsigned grid = (unsigned)(A.units < 256 * 16 ? A.units : 256 * 16);
            auto kernel = n_qubits == 13 ? (part ? nat_block_kernel<true, 8> : nat_block_kernel<false, 8>)
                                         : (part ? nat_block_kernel<true, 4> : nat_block_kernel<false, 4>);
            if (state > 64 * 1024)                                       // widths 12 and 13; below, the default limit holds
                FBX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)state));
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), state, stream(), A, d_words, (const double*)table.cs,
                               (const int*)table.bad, d_noise_class, d_in, d_class_error, part, d_n_errors_out, d_status_out);
        }
        FBX_HIP(hipGetLastError());
        if (d_probs_mean_out) {
            const long long count = (long long)cb << m, blocks = (count + 255) / 256;
            hipLaunchKernelGGL(nat_mean_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream(), n_qubits, m,
                               d_out_qubits, count, (long long)A.nseg, (long long)T, (const double*)part,
                               d_probs_mean_out + ((size_t)br0 << m));
            FBX_HIP(hipGetLastError());
        }
    }
    return FBX_OK;
}

int fbx_native_trajectories(int n_qubits, int64_t G, const uint32_t* words, const double* angles, const uint8_t* noise_class, int K,
                            int64_t P, const uint64_t* inputs, int m, const uint8_t* out_qubits, int64_t B, int64_t T,
                            const double* class_error, uint64_t seed, int64_t first_item, int64_t first_input, double* probs_mean_out,
                            int32_t* n_errors_out, int32_t* status_out) {
    const char* who = "fbx_native_trajectories";
    FBX_TRY(nat_check(n_qubits, G, words, angles, K, P, inputs, m, out_qubits, B, T, first_item, first_input, probs_mean_out, n_errors_out));
    FBX_TRY(nat_check_words(who, n_qubits, G, words, angles, true));
    FBX_TRY(dfe_check_classes(who, K, G, noise_class));
    unsigned seen = 0;
    for (int j = 0; j < m; ++j) {
        FBX_REQUIRE(out_qubits[j] < n_qubits && !((seen >> out_qubits[j]) & 1u),
                    "fbx_native_trajectories: an entry of out_qubits is not below n_qubits or repeats");
        seen |= 1u << out_qubits[j];
    }
    FBX_TRY(ensure_device());
    if (B == 0 || P == 0 || T == 0) return FBX_OK;
    const size_t sb = (size_t)B, sp = (size_t)P;
    HostIO io; uint32_t* dw; double *da, *de = nullptr, *dmean; uint8_t *dc = nullptr, *dq; uint64_t* din; int32_t *dne, *dst;
    FBX_TRY(io.in(words, (size_t)G, &dw)); FBX_TRY(io.in(angles, (size_t)G, &da));
    if (noise_class) FBX_TRY(io.in(noise_class, (size_t)G, &dc));
    FBX_TRY(io.in(inputs, sp, &din)); FBX_TRY(io.in(out_qubits, (size_t)m, &dq));
    if (class_error) FBX_TRY(io.in(class_error, sb * (size_t)K, &de));
    FBX_TRY(io.out_opt(probs_mean_out, (sb * sp) << m, &dmean));
    FBX_TRY(io.out_opt(n_errors_out, sb * sp * (size_t)T, &dne));
    FBX_TRY(io.out_opt(status_out, sb, &dst));
    FBX_TRY(fbx_native_trajectories_dev(n_qubits, G, dw, da, dc, K, P, din, m, dq, B, T, de, seed, first_item, first_input, dmean, dne, dst));
    return io.finish();
}

int fbx_native_unitary_dev(int n_qubits, int64_t G, const uint32_t* d_words, const double* d_angles, double* d_U_out) {
    FBX_TRY(nat_check_width("fbx_native_unitary", n_qubits));
    FBX_REQUIRE(G >= 0 && G < ((int64_t)1 << 31), "fbx_native_unitary: G must be 0 .. 2^31 - 1");
    FBX_REQUIRE((G == 0 || (d_words && d_angles)) && d_U_out, "fbx_native_unitary: NULL argument");
    FBX_TRY(ensure_device());
    NatTable table;
    FBX_TRY(table.make(G, d_angles));
    const size_t state = sizeof(cplx) << n_qubits;
    const int64_t columns = (int64_t)1 << n_qubits;
    cplx* U = reinterpret_cast<cplx*>(d_U_out);
    if (n_qubits <= NAT_WAVE_MAX_QUBITS) {
        hipLaunchKernelGGL(nat_unitary_wave_kernel, dim3((unsigned)((columns + 3) / 4)), dim3(256), 4 * state, stream(), n_qubits, (long long)G,
                           d_words, (const double*)table.cs, (const int*)table.bad, U);
    } else {
        const int groups = 1 << (n_qubits - 2);
        if (state > 64 * 1024)
            FBX_HIP(hipFuncSetAttribute((const void*)nat_unitary_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)state));
        hipLaunchKernelGGL(nat_unitary_block_kernel, dim3((unsigned)(columns < 4096 ? columns : 4096)), dim3((unsigned)(groups < 1024 ? groups : 1024)),
                           state, stream(), n_qubits, (long long)G, d_words, (const double*)table.cs, (const int*)table.bad, U);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_native_unitary(int n_qubits, int64_t G, const uint32_t* words, const double* angles, double* U_out) {
    const char* who = "fbx_native_unitary";
    FBX_TRY(nat_check_width(who, n_qubits));
    FBX_REQUIRE(G >= 0 && G < ((int64_t)1 << 31), "fbx_native_unitary: G must be 0 .. 2^31 - 1");
    FBX_REQUIRE((G == 0 || (words && angles)) && U_out, "fbx_native_unitary: NULL argument");
    FBX_TRY(nat_check_words(who, n_qubits, G, words, angles, false));
    FBX_TRY(ensure_device());
    HostIO io; uint32_t* dw; double *da, *du;
    FBX_TRY(io.in(words, (size_t)G, &dw)); FBX_TRY(io.in(angles, (size_t)G, &da));
    FBX_TRY(io.out(U_out, (size_t)2 << (2 * n_qubits), &du));
    FBX_TRY(fbx_native_unitary_dev(n_qubits, G, dw, da, du));
    return io.finish();
}

}  // fbx C ABI
