// fbx_reversible.hip -- measured bitstrings of a noisy reversible circuit on up to 64 qubits (include/fbx.h): the
// ripple-carry adder and its like, whose state is a product of Z or X eigenstates throughout, so a shot is one 64-bit word of
// classical bits and a Pauli error a flip of some of them.
//   reversible_shots_kernel  a lane per shot, a wavefront per unit = 64 consecutive shots of one (item, input word), four units per
//                            workgroup, flattened.  The input word, the micro-op word, its noise class and the class's error
//                            probability are wave-uniform (scalar loads and branches, as in frames_shots_kernel of fbx_frames.hip);
//                            a Philox block is computed only where a gate with noise needs it.  The records of a wavefront are
//                            contiguous in memory: they are staged in LDS and stored with full-width stores.  The histogram of
//                            error weights is a ballot and a population count per weight; it is stored when one wavefront covers
//                            the unit's shots and added with integer atomics otherwise.
#include "fbx_clifford_gates.hpp"

namespace fbx {

constexpr int REV_THREADS = 256;
constexpr int REV_UNITS = REV_THREADS / 64;              // wavefronts, and so units, per workgroup
constexpr uint32_t REV_KEY = 0x52565253u;                // "RVRS"

// the fields of a micro-op word (include/fbx.h)
__host__ __device__ __forceinline__ uint32_t rev_op(uint32_t w) { return w & 7u; }
__host__ __device__ __forceinline__ uint32_t rev_arity(uint32_t w) { return (w >> 3) & 3u; }
__host__ __device__ __forceinline__ uint32_t rev_qubit(uint32_t w, int i) { return (w >> (5 + 6 * i)) & 63u; }
__host__ __device__ __forceinline__ uint32_t rev_on_z(uint32_t w, int i) { return (w >> (23 + i)) & 1u; }
__host__ __device__ __forceinline__ uint32_t rev_input_bit(uint32_t w) { return w >> 26; }

#if defined(__HIPCC__)

// whether the Pauli with index d (0 I, 1 X, 2 Y, 3 Z) flips a bit held in Z (on_z = 0: its X part) or in X (on_z = 1: its Z part)
__device__ __forceinline__ uint64_t rev_flips(uint32_t d, uint32_t on_z) { return (uint64_t)(((on_z ? d >> 1 : d ^ (d >> 1))) & 1u); }

// wavefront `wave` of workgroup blockIdx.x is unit u = blockIdx.x * 4 + wave = ((b * P) + r) * chunks + chunk: the shots
// chunk * 64 .. + 63 of input word r of item b
__global__ void __launch_bounds__(REV_THREADS)
reversible_shots_kernel(int n, long long G, const uint32_t* __restrict__ words, const uint8_t* __restrict__ noise_class, int K,
                        long long P, const uint64_t* __restrict__ inputs, int m, const uint8_t* __restrict__ out_qubits,
                        const uint64_t* __restrict__ expected, long long n_shots, long long chunks, long long units,
                        const double* __restrict__ class_error, const double* __restrict__ flips, unsigned long long seed,
                        long long first_item, long long first_input, uint8_t* __restrict__ bits_out,
                        uint64_t* __restrict__ words_out, unsigned long long* __restrict__ weight_counts,
                        int32_t* __restrict__ status_out) {
    __shared__ uint8_t stage_all[REV_THREADS * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long u = (long long)blockIdx.x * REV_UNITS + wave;
    const bool unit = u < units;                                    // wave-uniform; a wavefront past the end only meets the barrier
    const long long uu = unit ? u : 0;
    const long long br = uu / chunks, chunk = uu - br * chunks, b = br / P, r = br - b * P;
    const long long s = chunk * 64 + lane;
    const bool live = unit && s < n_shots;
    uint8_t* stage = stage_all + wave * (64 * 64);

    uint64_t rec = 0;
    bool poisoned = false;
    if (unit) {
        // the item's K class errors and 2 m flips, a lane each: K + 2 m <= 144
        bool bad = false;
        if (class_error && lane < K) bad = dfe_bad_probability(class_error[b * K + lane]);
        if (flips)
            for (int i = lane; i < 2 * m; i += 64) bad = bad || dfe_bad_probability(flips[b * 2 * m + i]);
        poisoned = __ballot(bad ? 1 : 0) != 0ull;
    }
    if (unit && !poisoned) {
        const uint64_t input = inputs[r];
        const uint32_t c0 = (uint32_t)(unsigned long long)(first_item + b), c1 = (uint32_t)(unsigned long long)(first_input + r);
        const uint32_t c2 = (uint32_t)(unsigned long long)s;
        const uint32_t k0 = (uint32_t)seed ^ REV_KEY, k1 = (uint32_t)(seed >> 32);
        uint64_t st = 0;
        uint32_t blk[4] = {0u, 0u, 0u, 0u};
        long long have = -1;                                        // the pair of gates whose block is in blk (wave-uniform)
        for (long long l = 0; l < G; ++l) {
            const uint32_t w = words[l], op = rev_op(w), q0 = rev_qubit(w, 0), q1 = rev_qubit(w, 1), q2 = rev_qubit(w, 2);
            bool exists = true;
            switch (op) {                                           // wave-uniform
                case FBX_REV_NOT:    st ^= (uint64_t)1 << q0; break;
                case FBX_REV_XOR:    st ^= ((st >> q1) & 1u) << q0; break;
                case FBX_REV_ANDXOR: st ^= ((st >> q1) & (st >> q2) & 1u) << q0; break;
                case FBX_REV_XIN:    exists = (input >> rev_input_bit(w)) & 1u; st ^= (uint64_t)(exists ? 1u : 0u) << q0; break;
                default: break;
            }
            const int cls = noise_class ? (int)noise_class[l] : 0;
            const double p = (class_error && cls < K && exists) ? class_error[b * K + cls] : 0.0;
            if (p > 0.0) {                                          // wave-uniform
                if (have != (l >> 1)) {
                    blk[0] = c0; blk[1] = c1; blk[2] = c2; blk[3] = (uint32_t)(l >> 1);
                    philox4x32_10(blk, k0, k1);
                    have = l >> 1;
                }
                const uint32_t first = (l & 1) ? blk[2] : blk[0], second = (l & 1) ? blk[3] : blk[1];
                if ((double)first * 0x1p-32 < p) {
                    const uint32_t k = rev_arity(w);
                    if (k >= 3u) {
                        const uint32_t idx = second >> 26;
                        st ^= (rev_flips(idx >> 4, rev_on_z(w, 0)) << q0) ^ (rev_flips((idx >> 2) & 3u, rev_on_z(w, 1)) << q1)
                              ^ (rev_flips(idx & 3u, rev_on_z(w, 2)) << q2);
                    } else if (k == 2u) {
                        const uint32_t idx = second >> 28;
                        st ^= (rev_flips(idx >> 2, rev_on_z(w, 0)) << q0) ^ (rev_flips(idx & 3u, rev_on_z(w, 1)) << q1);
                    } else {
                        st ^= rev_flips(second >> 30, rev_on_z(w, 0)) << q0;
                    }
                }
            }
        }
        for (int j = 0; j < m; ++j) rec |= ((st >> (out_qubits[j] & 63u)) & 1u) << j;
        if (flips) {
            const uint32_t J = (uint32_t)((G + 1) >> 1);
            const double* __restrict__ f = flips + b * 2 * m;
            for (int j0 = 0; j0 < m; j0 += 4) {
                uint32_t c[4] = {c0, c1, c2, J + (uint32_t)(j0 >> 2)};
                philox4x32_10(c, k0, k1);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = j0 + t;
                    if (j < m) {
                        const double f0 = f[2 * j], f1 = f[2 * j + 1];
                        const double fj = ((rec >> j) & 1u) ? f1 : f0;
                        if ((double)c[t] * 0x1p-32 < fj) rec ^= (uint64_t)1 << j;
                    }
                }
            }
        }
    }
    if (unit) {
        if (status_out && r == 0 && chunk == 0 && lane == 0) status_out[b] = poisoned ? 1 : 0;
        if (words_out && live) words_out[(b * P + r) * n_shots + s] = rec;
        if (weight_counts) {
            // entry w of the unit's histogram: lane w holds it (w < 64), and lane 0 also entry 64 of a 64-column record
            const int weight = __popcll((rec ^ expected[r]) & dfe_valid_mask(m));
            const bool counted = live && !poisoned;
            unsigned long long mine = 0, last = 0;
            for (int w = 0; w <= m; ++w) {
                const unsigned long long c = (unsigned long long)__popcll(__ballot(counted && weight == w ? 1 : 0));
                if (w < 64) { if (lane == w) mine = c; } else last = c;
            }
            unsigned long long* dst = weight_counts + (b * P + r) * (m + 1);
            if (chunks == 1) {                                      // this wavefront is the whole unit
                if (lane <= m && lane < 64) dst[lane] = mine;
                if (m == 64 && lane == 0) dst[64] = last;
            } else {
                if (lane <= m && lane < 64 && mine) atomicAdd(dst + lane, mine);
                if (m == 64 && lane == 0 && last) atomicAdd(dst + 64, last);
            }
        }
    }
    if (bits_out) {                                                 // every wavefront of the workgroup comes here: no early exit
        if (unit)
            for (int j = 0; j < m; ++j) stage[lane * m + j] = (uint8_t)((rec >> j) & 1u);
        __syncthreads();
        if (unit) {
            // the records of this wavefront's shots are one contiguous range: bytes up to a 4-byte boundary, words, the rest as bytes
            const long long left = n_shots - chunk * 64;
            const int len = (int)(left < 64 ? left : 64) * m;
            uint8_t* dst = bits_out + ((b * P + r) * n_shots + chunk * 64) * m;
            int head = (int)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
            head = head < len ? head : len;
            const int n_words = (len - head) >> 2, tail = head + 4 * n_words;
            if (lane < head) dst[lane] = stage[lane];
            for (int i = lane; i < n_words; i += 64) {
                const uint8_t* src = stage + head + 4 * i;
                const uint32_t v = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
                reinterpret_cast<uint32_t*>(dst + head)[i] = v;
            }
            if (tail + lane < len) dst[tail + lane] = stage[tail + lane];
        }
    }
}

#endif

// ------------------------------------------------------------------ host: argument checks
static const char* const REV_WHO = "fbx_reversible_sample_shots";

static int reversible_check(int n, int64_t G, const void* words, int K, int64_t P, const void* inputs, int m, const void* out_qubits,
                            const void* expected, int64_t B, int64_t n_shots, int64_t first_item, int64_t first_input,
                            const void* bits_out, const void* words_out, const void* weight_counts, int64_t* chunks, int64_t* units) {
    const int64_t two32 = (int64_t)1 << 32;
    FBX_TRY(dfe_check_circuit(REV_WHO, n, G, words));
    FBX_REQUIRE(m >= 1 && m <= 64, "fbx_reversible_sample_shots: m must be 1..64");
    FBX_REQUIRE(G < ((int64_t)1 << 31), "fbx_reversible_sample_shots: G must be below 2^31 (the gate pair is one counter word)");
    FBX_REQUIRE(K >= 1 && K <= DFE_MAX_CLASSES, "fbx_reversible_sample_shots: K must be 1..16");
    FBX_REQUIRE(B >= 0 && P >= 0 && n_shots >= 0 && first_item >= 0 && first_input >= 0,
                "fbx_reversible_sample_shots: need B, P, n_shots, first_item and first_input >= 0");
    FBX_REQUIRE(n_shots < two32, "fbx_reversible_sample_shots: n_shots must be below 2^32");
    FBX_REQUIRE(first_item <= two32 && B <= two32 - first_item && first_input <= two32 && P <= two32 - first_input,
                "fbx_reversible_sample_shots: item and input indices must stay below 2^32 (each is one counter word)");
    FBX_REQUIRE(out_qubits, "fbx_reversible_sample_shots: NULL out_qubits");
    FBX_REQUIRE(P == 0 || inputs, "fbx_reversible_sample_shots: NULL inputs");
    FBX_REQUIRE(bits_out || words_out || weight_counts, "fbx_reversible_sample_shots: bits_out, words_out and weight_counts are all NULL");
    FBX_REQUIRE(!weight_counts || expected, "fbx_reversible_sample_shots: weight_counts needs expected");
    *chunks = (n_shots + 63) / 64;
    *units = 0;
    if (B == 0 || P == 0 || *chunks == 0) return FBX_OK;
    const int64_t cap = (((int64_t)1 << 31) - 1) * REV_UNITS;       // units of the largest grid
    FBX_REQUIRE(B <= cap / P && B * P <= cap / *chunks,
                "fbx_reversible_sample_shots: B * P * ceil(n_shots / 64) is beyond one launch; cut the batch with first_item or first_input");
    *units = B * P * *chunks;
    return FBX_OK;
}

// a circuit given by HOST words: the rule of include/fbx.h
static int reversible_check_words(int n, int64_t G, const uint32_t* words) {
    for (int64_t g = 0; g < G; ++g) {
        const uint32_t w = words[g], op = rev_op(w), k = rev_arity(w);
        bool ok = op <= FBX_REV_XIN && k >= 1 && k <= 3;
        if (op == FBX_REV_NOT || op == FBX_REV_XIN) ok = ok && k == 1;
        if (op == FBX_REV_XOR) ok = ok && k == 2;
        if (op == FBX_REV_ANDXOR) ok = ok && k == 3;
        if (op != FBX_REV_XIN) ok = ok && rev_input_bit(w) == 0;
        for (int i = 0; i < 3 && ok; ++i) {
            if (i < (int)k) {
                ok = rev_qubit(w, i) < (uint32_t)n;
                for (int j = 0; j < i; ++j) ok = ok && rev_qubit(w, i) != rev_qubit(w, j);
            } else {
                ok = rev_qubit(w, i) == 0 && rev_on_z(w, i) == 0;
            }
        }
        if (op == FBX_REV_XIN) ok = ok && rev_on_z(w, 0) == 0;
        if (!ok) { set_error(std::string(REV_WHO) + ": word " + std::to_string(g) + " is not a valid micro-op word for this width"); return FBX_ERR_BAD_ARG; }
    }
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_reversible_sample_shots_dev(int n_qubits, int64_t G, const uint32_t* d_words, const uint8_t* d_noise_class, int K, int64_t P,
                                    const uint64_t* d_inputs, int m, const uint8_t* d_out_qubits, const uint64_t* d_expected,
                                    int64_t B, int64_t n_shots, const double* d_class_error, const double* d_readout_flip,
                                    uint64_t seed, int64_t first_item, int64_t first_input, uint8_t* d_bits_out,
                                    uint64_t* d_words_out, int64_t* d_weight_counts, int32_t* d_status_out) {
    int64_t chunks = 0, units = 0;
    FBX_TRY(reversible_check(n_qubits, G, d_words, K, P, d_inputs, m, d_out_qubits, d_expected, B, n_shots, first_item, first_input,
                             d_bits_out, d_words_out, d_weight_counts, &chunks, &units));
    FBX_TRY(ensure_device());
    if (units == 0) return FBX_OK;
    if (d_weight_counts && chunks > 1)
        FBX_HIP(hipMemsetAsync(d_weight_counts, 0, sizeof(int64_t) * (size_t)(B * P) * (size_t)(m + 1), stream()));
    const unsigned groups = (unsigned)((units + REV_UNITS - 1) / REV_UNITS);
    hipLaunchKernelGGL(reversible_shots_kernel, dim3(groups), dim3(REV_THREADS), 0, stream(), n_qubits, (long long)G, d_words,
                       d_noise_class, K, (long long)P, d_inputs, m, d_out_qubits, d_expected, (long long)n_shots, (long long)chunks,
                       (long long)units, d_class_error, d_readout_flip, (unsigned long long)seed, (long long)first_item,
                       (long long)first_input, d_bits_out, d_words_out, reinterpret_cast<unsigned long long*>(d_weight_counts),
                       d_status_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_reversible_sample_shots(int n_qubits, int64_t G, const uint32_t* words, const uint8_t* noise_class, int K, int64_t P,
                                const uint64_t* inputs, int m, const uint8_t* out_qubits, const uint64_t* expected, int64_t B,
                                int64_t n_shots, const double* class_error, const double* readout_flip, uint64_t seed,
                                int64_t first_item, int64_t first_input, uint8_t* bits_out, uint64_t* words_out,
                                int64_t* weight_counts, int32_t* status_out) {
    int64_t chunks = 0, units = 0;
    FBX_TRY(reversible_check(n_qubits, G, words, K, P, inputs, m, out_qubits, expected, B, n_shots, first_item, first_input, bits_out,
                             words_out, weight_counts, &chunks, &units));
    FBX_TRY(reversible_check_words(n_qubits, G, words));
    FBX_TRY(dfe_check_classes(REV_WHO, K, G, noise_class));
    for (int j = 0; j < m; ++j)
        FBX_REQUIRE(out_qubits[j] < n_qubits, "fbx_reversible_sample_shots: an entry of out_qubits is not below n_qubits");
    FBX_TRY(ensure_device());
    if (units == 0) return FBX_OK;
    const size_t sb = (size_t)B, sp = (size_t)P, sm = (size_t)m, records = sb * sp * (size_t)n_shots;
    HostIO io; uint32_t* dw; uint8_t *dc = nullptr, *dq, *dbits; uint64_t *din, *dexp = nullptr, *dwords;
    double *de = nullptr, *df = nullptr; int64_t* dcounts; int32_t* dst;
    FBX_TRY(io.in(words, (size_t)G, &dw));
    if (noise_class) FBX_TRY(io.in(noise_class, (size_t)G, &dc));
    FBX_TRY(io.in(inputs, sp, &din));
    FBX_TRY(io.in(out_qubits, sm, &dq));
    if (expected) FBX_TRY(io.in(expected, sp, &dexp));
    if (class_error) FBX_TRY(io.in(class_error, sb * (size_t)K, &de));
    if (readout_flip) FBX_TRY(io.in(readout_flip, sb * sm * 2, &df));
    FBX_TRY(io.out_opt(bits_out, records * sm, &dbits));
    FBX_TRY(io.out_opt(words_out, records, &dwords));
    FBX_TRY(io.out_opt(weight_counts, sb * sp * (sm + 1), &dcounts));
    FBX_TRY(io.out_opt(status_out, sb, &dst));
    FBX_TRY(fbx_reversible_sample_shots_dev(n_qubits, G, dw, dc, K, P, din, m, dq, dexp, B, n_shots, de, df, seed, first_item,
                                            first_input, dbits, dwords, dcounts, dst));
    return io.finish();
}

}  // fbx C ABI
