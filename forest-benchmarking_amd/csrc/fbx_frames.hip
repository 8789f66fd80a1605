// fbx_frames.hip -- measured bitstrings of a noisy Clifford circuit on up to 64 qubits without a state vector (include/fbx.h, DESIGN.md
// 4.19): one noiseless reference outcome per circuit, one Pauli frame per shot.
//   frames_reference_kernel  one wavefront.  Lane i holds the generator pair (U X_i U^+, U Z_i U^+) of the stabilizer tableau of
//                            U|0..0>, walked through the gate list as in fbx_dfe.hip; the qubits are then measured in the order
//                            0 .. n-1 (Aaronson, Gottesman, "Improved simulation of stabilizer circuits", 2004): a ballot finds the
//                            stabilizers that anticommute with Z_a, the first of them is broadcast and multiplied into the others
//                            (its outcome is taken as 0); without one the outcome is the sign of a product of stabilizers, formed by
//                            a butterfly over the lanes.  Products track the sign with four population counts.
//   frames_shots_kernel      a lane per shot, a workgroup per (item, 256 consecutive shots): the frame (fx, fz) lives in registers, the
//                            gate word, its noise class and the class's error probability are wave-uniform (scalar loads and
//                            branches), and a Philox block is computed only where a gate with noise needs it.  The bit record of
//                            the workgroup is contiguous in memory: it is staged in LDS and stored with full-width stores.
// The walk costs a dozen integer instructions per gate and lane; with noise every second gate adds a Philox block.
#include "fbx_clifford_gates.hpp"

namespace fbx {

constexpr int FRAMES_THREADS = 256;
constexpr uint32_t FRAMES_KEY = 0x43465253u;             // "CFRS"

#if defined(__HIPCC__)

__device__ __forceinline__ uint64_t frames_shfl(uint64_t v, int lane) { return (uint64_t)__shfl((unsigned long long)v, lane); }
__device__ __forceinline__ uint64_t frames_shfl_xor(uint64_t v, int mask) { return (uint64_t)__shfl_xor((unsigned long long)v, mask); }

// (x1, z1, r1) <- (x1, z1, r1) (x2, z2, r2) for Hermitian Paulis P = i^(x.z) X^x Z^z: the product is i^e times the Hermitian Pauli
// (x1 ^ x2, z1 ^ z2) with e = x1.z1 + x2.z2 - x3.z3 + 2 z1.x2 (mod 4).  e is even when the factors commute; bit 1 of e is the sign.
__device__ __forceinline__ void frames_multiply(uint64_t& x1, uint64_t& z1, uint32_t& r1, uint64_t x2, uint64_t z2, uint32_t r2) {
    const uint64_t x3 = x1 ^ x2, z3 = z1 ^ z2;
    const uint32_t e = (uint32_t)__popcll(x1 & z1) + (uint32_t)__popcll(x2 & z2) - (uint32_t)__popcll(x3 & z3)
                       + 2u * (uint32_t)__popcll(z1 & x2);
    r1 ^= r2 ^ ((e >> 1) & 1u);
    x1 = x3; z1 = z3;
}

__global__ void __launch_bounds__(64)
frames_reference_kernel(int n, long long G, const uint32_t* __restrict__ gates, uint64_t* __restrict__ reference_out) {
    const int lane = threadIdx.x;
    // lanes from n on carry the identity: every gate maps it to itself, and it never anticommutes with anything
    uint64_t dx = lane < n ? (uint64_t)1 << lane : 0, dz = 0, sx = 0, sz = dx;
    uint32_t dr = 0, sr = 0;
    for (long long g = 0; g < G; ++g) {
        const uint32_t w = gates[g], op = w & 0xFFu, q0 = (w >> 8) & 0xFFu, q1 = (w >> 16) & 0xFFu;
        dfe_apply_gate(op, q0, q1, dx, dz, dr);
        dfe_apply_gate(op, q0, q1, sx, sz, sr);
    }
    uint64_t x0 = 0;
    for (int a = 0; a < n; ++a) {
        const unsigned long long anti = __ballot((int)((sx >> a) & 1u));
        if (anti) {                                   // a random outcome, taken as 0
            const int p = __builtin_ctzll(anti);
            const uint64_t px = frames_shfl(sx, p), pz = frames_shfl(sz, p);
            const uint32_t pr = (uint32_t)__shfl((int)sr, p);
            if (lane == p) {
                dx = px; dz = pz;                     // the old stabilizer becomes the destabilizer of the new one, +Z_a
                sx = 0; sz = (uint64_t)1 << a; sr = 0;
            } else {
                if ((sx >> a) & 1u) frames_multiply(sx, sz, sr, px, pz, pr);
                if ((dx >> a) & 1u) { dx ^= px; dz ^= pz; }      // the sign of a destabilizer is never read
            }
        } else {                                      // determined: the product of the stabilizers whose destabilizer has X on a
            const bool in = (dx >> a) & 1u;
            uint64_t ax = in ? sx : 0, az = in ? sz : 0;
            uint32_t ar = in ? sr : 0u;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const uint64_t ox = frames_shfl_xor(ax, m), oz = frames_shfl_xor(az, m);
                const uint32_t orr = (uint32_t)__shfl_xor((int)ar, m);
                frames_multiply(ax, az, ar, ox, oz, orr);        // stabilizers commute: both partners hold the same product
            }
            x0 |= (uint64_t)(ar & 1u) << a;
        }
    }
    if (lane == 0) reference_out[0] = x0;
}

// Pauli index 0 I, 1 X, 2 Y, 3 Z -> its x bit and z bit
__device__ __forceinline__ uint64_t frames_pauli_x(uint32_t k) { return (uint64_t)((k == 1u) | (k == 2u)); }
__device__ __forceinline__ uint64_t frames_pauli_z(uint32_t k) { return (uint64_t)(k >> 1); }

// workgroup blockIdx.x = item b * chunks + chunk: the shots chunk * 256 .. + 255 of item b
__global__ void __launch_bounds__(FRAMES_THREADS)
frames_shots_kernel(int n, long long G, const uint32_t* __restrict__ gates, const uint8_t* __restrict__ noise_class, int K,
                    const uint64_t* __restrict__ reference, long long n_shots, long long chunks,
                    const double* __restrict__ class_error, const double* __restrict__ flips, unsigned long long seed,
                    long long first_item, uint8_t* __restrict__ bits_out, uint64_t* __restrict__ words_out,
                    int32_t* __restrict__ status_out) {
    __shared__ uint8_t stage[FRAMES_THREADS * 64];
    const int tid = threadIdx.x;
    const long long b = (long long)blockIdx.x / chunks, chunk = (long long)blockIdx.x - b * chunks;
    const long long s = chunk * FRAMES_THREADS + tid;
    const bool live = s < n_shots;

    // the item's K class errors and 2 n flips, one per thread: K + 2 n <= 144
    bool bad = false;
    if (class_error && tid < K) bad = dfe_bad_probability(class_error[b * K + tid]);
    if (flips && tid >= K && tid < K + 2 * n) bad = dfe_bad_probability(flips[b * 2 * n + (tid - K)]);
    const bool poisoned = __syncthreads_or(bad ? 1 : 0) != 0;

    uint64_t outcome = 0;
    if (!poisoned) {
        const uint64_t valid = dfe_valid_mask(n);
        const unsigned long long gid = (unsigned long long)(first_item + b);
        const uint32_t c0 = (uint32_t)gid, c1 = (uint32_t)(gid >> 32), c2 = (uint32_t)(unsigned long long)s;
        const uint32_t k0 = (uint32_t)seed ^ FRAMES_KEY, k1 = (uint32_t)(seed >> 32);
        uint64_t fx = 0, fz;
        {
            uint32_t c[4] = {c0, c1, c2, 0u};
            philox4x32_10(c, k0, k1);
            fz = ((uint64_t)c[0] | ((uint64_t)c[1] << 32)) & valid;
        }
        uint32_t blk[4] = {0u, 0u, 0u, 0u};
        long long have = -1;                                        // the pair of gates whose block is in blk (wave-uniform)
        uint32_t unused = 0;
        for (long long l = 0; l < G; ++l) {
            const uint32_t w = gates[l], op = w & 0xFFu, q0 = (w >> 8) & 63u, q1 = (w >> 16) & 63u;
            dfe_apply_gate(op, q0, q1, fx, fz, unused);
            const int cls = noise_class ? (int)noise_class[l] : 0;
            const double p = (class_error && cls < K) ? class_error[b * K + cls] : 0.0;
            if (p > 0.0) {                                          // wave-uniform
                if (have != (l >> 1)) {
                    blk[0] = c0; blk[1] = c1; blk[2] = c2; blk[3] = 1u + (uint32_t)(l >> 1);
                    philox4x32_10(blk, k0, k1);
                    have = l >> 1;
                }
                const uint32_t first = (l & 1) ? blk[2] : blk[0], second = (l & 1) ? blk[3] : blk[1];
                if ((double)first * 0x1p-32 < p) {
                    if (op >= FBX_GATE_CNOT) {
                        const uint32_t k = second >> 28, a = k >> 2, c = k & 3u;
                        fx ^= (frames_pauli_x(a) << q0) ^ (frames_pauli_x(c) << q1);
                        fz ^= (frames_pauli_z(a) << q0) ^ (frames_pauli_z(c) << q1);
                    } else {
                        const uint32_t k = second >> 30;
                        fx ^= frames_pauli_x(k) << q0;
                        fz ^= frames_pauli_z(k) << q0;
                    }
                }
            }
        }
        outcome = (reference[0] ^ fx) & valid;
        if (flips) {
            const uint32_t J = 1u + (uint32_t)((G + 1) >> 1);
            const double* __restrict__ f = flips + b * 2 * n;
            for (int j0 = 0; j0 < n; j0 += 4) {
                uint32_t c[4] = {c0, c1, c2, J + (uint32_t)(j0 >> 2)};
                philox4x32_10(c, k0, k1);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = j0 + t;
                    if (j < n) {
                        const double f0 = f[2 * j], f1 = f[2 * j + 1];
                        const double fj = ((outcome >> j) & 1u) ? f1 : f0;
                        if ((double)c[t] * 0x1p-32 < fj) outcome ^= (uint64_t)1 << j;
                    }
                }
            }
        }
    }
    if (status_out && chunk == 0 && tid == 0) status_out[b] = poisoned ? 1 : 0;
    if (words_out && live) words_out[b * n_shots + s] = outcome;
    if (bits_out) {
        for (int q = 0; q < n; ++q) stage[tid * n + q] = (uint8_t)((outcome >> q) & 1u);
        __syncthreads();
        // the records of this workgroup's shots are one contiguous range: bytes up to a 4-byte boundary, words, the rest as bytes
        const long long left = n_shots - chunk * FRAMES_THREADS;
        const int len = (int)(left < FRAMES_THREADS ? left : FRAMES_THREADS) * n;
        uint8_t* dst = bits_out + (b * n_shots + chunk * FRAMES_THREADS) * n;
        int head = (int)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
        head = head < len ? head : len;
        const int n_words = (len - head) >> 2, tail = head + 4 * n_words;
        if (tid < head) dst[tid] = stage[tid];
        for (int i = tid; i < n_words; i += FRAMES_THREADS) {
            const uint8_t* src = stage + head + 4 * i;
            const uint32_t v = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
            reinterpret_cast<uint32_t*>(dst + head)[i] = v;
        }
        if (tail + tid < len) dst[tail + tid] = stage[tail + tid];
    }
}

#endif

// ------------------------------------------------------------------ host: argument checks
static int reference_check(int n, int64_t G, const void* gates, const void* out) {
    FBX_TRY(dfe_check_circuit("fbx_clifford_reference_sample", n, G, gates));
    FBX_REQUIRE(out, "fbx_clifford_reference_sample: NULL reference_out");
    return FBX_OK;
}

static int shots_check(int n, int64_t G, const void* gates, int K, const void* reference, int64_t B, int64_t n_shots,
                       int64_t first_item, const void* bits_out, const void* words_out, int64_t* chunks) {
    FBX_TRY(dfe_check_circuit("fbx_clifford_sample_shots", n, G, gates));
    FBX_REQUIRE(G < ((int64_t)1 << 31), "fbx_clifford_sample_shots: G must be below 2^31 (the gate pair is one counter word)");
    FBX_REQUIRE(K >= 1 && K <= DFE_MAX_CLASSES, "fbx_clifford_sample_shots: K must be 1..16");
    FBX_REQUIRE(B >= 0 && n_shots >= 0 && first_item >= 0, "fbx_clifford_sample_shots: need B >= 0, n_shots >= 0 and first_item >= 0");
    FBX_REQUIRE(n_shots < ((int64_t)1 << 32), "fbx_clifford_sample_shots: n_shots must be below 2^32");
    FBX_REQUIRE(reference, "fbx_clifford_sample_shots: NULL reference");
    FBX_REQUIRE(bits_out || words_out, "fbx_clifford_sample_shots: both outputs are NULL");
    *chunks = (n_shots + FRAMES_THREADS - 1) / FRAMES_THREADS;
    FBX_REQUIRE(*chunks == 0 || B < ((int64_t)1 << 31) / *chunks,
                "fbx_clifford_sample_shots: B * ceil(n_shots / 256) is beyond one launch; cut the batch with first_item");
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_clifford_reference_sample_dev(int n_qubits, int64_t G, const uint32_t* d_gates, uint64_t* d_reference_out) {
    FBX_TRY(reference_check(n_qubits, G, d_gates, d_reference_out));
    FBX_TRY(ensure_device());
    hipLaunchKernelGGL(frames_reference_kernel, dim3(1), dim3(64), 0, stream(), n_qubits, (long long)G, d_gates, d_reference_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_clifford_reference_sample(int n_qubits, int64_t G, const uint32_t* gates, uint64_t* reference_out) {
    FBX_TRY(reference_check(n_qubits, G, gates, reference_out));
    FBX_TRY(dfe_check_gates("fbx_clifford_reference_sample", n_qubits, G, gates));
    FBX_TRY(ensure_device());
    HostIO io; uint32_t* dg; uint64_t* dr;
    FBX_TRY(io.in(gates, (size_t)G, &dg));
    FBX_TRY(io.out(reference_out, 1, &dr));
    FBX_TRY(fbx_clifford_reference_sample_dev(n_qubits, G, dg, dr));
    return io.finish();
}

int fbx_clifford_sample_shots_dev(int n_qubits, int64_t G, const uint32_t* d_gates, const uint8_t* d_noise_class, int K,
                                  const uint64_t* d_reference, int64_t B, int64_t n_shots, const double* d_class_error,
                                  const double* d_readout_flip, uint64_t seed, int64_t first_item, uint8_t* d_bits_out,
                                  uint64_t* d_words_out, int32_t* d_status_out) {
    int64_t chunks = 0;
    FBX_TRY(shots_check(n_qubits, G, d_gates, K, d_reference, B, n_shots, first_item, d_bits_out, d_words_out, &chunks));
    FBX_TRY(ensure_device());
    if (B == 0 || n_shots == 0) return FBX_OK;
    hipLaunchKernelGGL(frames_shots_kernel, dim3((unsigned)(B * chunks)), dim3(FRAMES_THREADS), 0, stream(), n_qubits, (long long)G,
                       d_gates, d_noise_class, K, d_reference, (long long)n_shots, (long long)chunks, d_class_error, d_readout_flip,
                       (unsigned long long)seed, (long long)first_item, d_bits_out, d_words_out, d_status_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_clifford_sample_shots(int n_qubits, int64_t G, const uint32_t* gates, const uint8_t* noise_class, int K,
                              const uint64_t* reference, int64_t B, int64_t n_shots, const double* class_error,
                              const double* readout_flip, uint64_t seed, int64_t first_item, uint8_t* bits_out, uint64_t* words_out,
                              int32_t* status_out) {
    int64_t chunks = 0;
    FBX_TRY(shots_check(n_qubits, G, gates, K, reference, B, n_shots, first_item, bits_out, words_out, &chunks));
    FBX_TRY(dfe_check_gates("fbx_clifford_sample_shots", n_qubits, G, gates));
    FBX_TRY(dfe_check_classes("fbx_clifford_sample_shots", K, G, noise_class));
    FBX_TRY(ensure_device());
    if (B == 0 || n_shots == 0) return FBX_OK;
    const size_t sb = (size_t)B, records = sb * (size_t)n_shots;
    HostIO io; uint32_t* dg; uint8_t *dc = nullptr, *dbits; uint64_t *dref, *dwords; double *de = nullptr, *df = nullptr; int32_t* dst;
    FBX_TRY(io.in(gates, (size_t)G, &dg));
    if (noise_class) FBX_TRY(io.in(noise_class, (size_t)G, &dc));
    FBX_TRY(io.in(reference, 1, &dref));
    if (class_error) FBX_TRY(io.in(class_error, sb * (size_t)K, &de));
    if (readout_flip) FBX_TRY(io.in(readout_flip, sb * (size_t)n_qubits * 2, &df));
    FBX_TRY(io.out_opt(bits_out, records * (size_t)n_qubits, &dbits));
    FBX_TRY(io.out_opt(words_out, records, &dwords));
    FBX_TRY(io.out_opt(status_out, sb, &dst));
    FBX_TRY(fbx_clifford_sample_shots_dev(n_qubits, G, dg, dc, K, dref, B, n_shots, de, df, seed, first_item, dbits, dwords, dst));
    return io.finish();
}

}  // fbx C ABI
