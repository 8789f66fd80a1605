// fbx_clifford_elems.hpp -- the packed Clifford element words on the device (include/fbx.h, "Clifford elements"): phase table,
// validity, signed-permutation table, composition, inverse, the enumeration of fbx/clifford.py and the uniform draw of an RB
// sequence's stream.  Shared by fbx_clifford.hip (sequences, simulation) and fbx_rb_acquire.hip (the fused acquisition), which
// must draw the same elements word for word.
#pragma once
#include "fbx_common.hpp"

namespace fbx {

constexpr uint32_t CL_PHASE_LUT = 0x344CD000u;    // 2-bit exponents of a b = i^ph P_(a ^ b), entry 4 a + b: XY = iZ, YZ = iX, ZX = iY

// exponent of i (unreduced) in the product of the Paulis with indices a, b < 16
__host__ __device__ __forceinline__ uint32_t cl_mul_phase(uint32_t a, uint32_t b) {
    return ((CL_PHASE_LUT >> (2 * ((a & 12u) | (b >> 2)))) & 3u) + ((CL_PHASE_LUT >> (2 * (((a & 3u) << 2) | (b & 3u)))) & 3u);
}

template <int NQ> struct ClGroup;
template <> struct ClGroup<1> { static constexpr uint32_t order = 24, identity = 1u | (3u << 5); };
template <> struct ClGroup<2> { static constexpr uint32_t order = 11520, identity = 4u | (12u << 5) | (1u << 10) | (3u << 15); };

template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_generator(int j) {       // Pauli index of X_0, Z_0[, X_1, Z_1]
    return (ClGroup<NQ>::identity >> (5 * j)) & 15u;
}

// every unused bit zero; images of X_q and Z_q anticommute; images of different qubits commute
template <int NQ>
__host__ __device__ __forceinline__ bool cl_valid(uint32_t w) {
    bool ok = (w >> (10 * NQ)) == 0u;
    uint32_t p[2 * NQ];
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) { p[j] = (w >> (5 * j)) & 15u; if (NQ == 1) ok = ok && p[j] < 4u; }
#pragma unroll
    for (int i = 0; i < 2 * NQ; ++i)
#pragma unroll
        for (int j = i + 1; j < 2 * NQ; ++j)
            ok = ok && ((cl_mul_phase(p[i], p[j]) & 1u) == ((i >> 1) == (j >> 1) ? 1u : 0u));
    return ok;
}

// The signed permutation of a valid word: C P_k C^+ = (neg bit k ? -1 : +1) P_perm[k], perm[k] in bits [4 k, 4 k + 4).
template <int NQ>
__host__ __device__ __forceinline__ void cl_table(uint32_t w, unsigned long long& perm, uint32_t& neg) {
    uint32_t qi[NQ][4], qp[NQ][4];                 // per qubit: image of I, X, Y, Z as (index, exponent of i)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint32_t px = (w >> (10 * q)) & 15u, sx = (w >> (10 * q + 4)) & 1u;
        const uint32_t pz = (w >> (10 * q + 5)) & 15u, sz = (w >> (10 * q + 9)) & 1u;
        qi[q][0] = 0u; qp[q][0] = 0u;
        qi[q][1] = px; qp[q][1] = 2u * sx;
        qi[q][3] = pz; qp[q][3] = 2u * sz;
        qi[q][2] = px ^ pz; qp[q][2] = 1u + 2u * (sx + sz) + cl_mul_phase(px, pz);      // Y = i X Z
    }
    perm = 0ull; neg = 0u;
#pragma unroll
    for (int k = 0; k < (1 << (2 * NQ)); ++k) {
        uint32_t idx, ph;
        if constexpr (NQ == 1) { idx = qi[0][k]; ph = qp[0][k]; }
        else {
            const uint32_t a = qi[0][k >> 2], b = qi[1][k & 3];
            idx = a ^ b; ph = qp[0][k >> 2] + qp[1][k & 3] + cl_mul_phase(a, b);
        }
        perm |= (unsigned long long)idx << (4 * k);
        neg |= ((ph >> 1) & 1u) << k;
    }
}

// a after b: the images of b's images under a
template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_compose(unsigned long long perm_a, uint32_t neg_a, uint32_t b) {
    uint32_t out = 0u;
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) {
        const uint32_t p = (b >> (5 * j)) & 15u, s = (b >> (5 * j + 4)) & 1u;
        out |= ((uint32_t)((perm_a >> (4 * p)) & 15ull) | ((s ^ ((neg_a >> p) & 1u)) << 4)) << (5 * j);
    }
    return out;
}

// the inverse from the table: generator g is the image of the one Pauli k with perm[k] = g, with the same sign
template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_inverse(unsigned long long perm, uint32_t neg) {
    uint32_t out = 0u;
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) {
        const uint32_t g = cl_generator<NQ>(j);
#pragma unroll
        for (int k = 1; k < (1 << (2 * NQ)); ++k)
            if ((uint32_t)((perm >> (4 * k)) & 15ull) == g) out |= ((uint32_t)k | (((neg >> k) & 1u) << 4)) << (5 * j);
    }
    return out;
}

// fbx/clifford.py from_index: idx = signs + 4^n r; the images are chosen one after the other, the c-th candidate in ascending Pauli
// index that commutes with the images of the earlier qubits and (for Z_q) anticommutes with the image of X_q.  idx < order.
template <int NQ>
__host__ __device__ __forceinline__ uint32_t cl_from_index(uint32_t idx) {
    const uint32_t signs = idx & ((1u << (2 * NQ)) - 1u);
    uint32_t r = idx >> (2 * NQ), chosen[2 * NQ], out = 0u;
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) {
        const uint32_t base = NQ == 1 ? (j == 0 ? 3u : 2u) : (j == 0 ? 15u : j == 1 ? 8u : j == 2 ? 3u : 2u);
        uint32_t c = r % base, pick = 0u;
        r /= base;
        // ascending scan with a running count (no early exit: every lane runs the same 4^n - 1 steps)
        uint32_t seen = 0u;
#pragma unroll
        for (uint32_t cand = 1u; cand < (1u << (2 * NQ)); ++cand) {
            bool ok = true;
#pragma unroll
            for (int e = 0; e < 2 * (j >> 1); ++e) ok = ok && (cl_mul_phase(cand, chosen[e]) & 1u) == 0u;
            if (j & 1) ok = ok && (cl_mul_phase(cand, chosen[j - 1]) & 1u) == 1u;
            if (ok) { if (seen == c) pick = cand; ++seen; }
        }
        chosen[j] = pick;
        out |= (pick | (((signs >> j) & 1u) << 4)) << (5 * j);
    }
    return out;
}

#if defined(__HIPCC__)
// Uniform on range(N), N < 2^16: x N / 2^32 of a 32-bit word x, rejected when the low half of the product falls below 2^32 mod N
// (Lemire, "Fast random integer generation in an interval", 2019) -- every value keeps exactly floor(2^32 / N) words.  Draw
// `draw` of sequence b takes the four words of block (b, draw, attempt) in turn; a rejection has probability < N / 2^32 < 3e-6, so
// eight blocks (32 words) never run out in practice, and the loop is bounded for the sake of a bound.
__device__ __forceinline__ uint32_t cl_draw(unsigned long long seed, long long b, uint32_t draw, uint32_t N) {
    const uint32_t thresh = (0u - N) % N;
    unsigned long long m = 0ull;
    for (uint32_t attempt = 0u; attempt < 8u; ++attempt) {
        uint32_t c[4] = {(uint32_t)b, (uint32_t)((unsigned long long)b >> 32), draw, 0x52420000u + attempt};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            m = (unsigned long long)c[w] * N;
            if ((uint32_t)m >= thresh) return (uint32_t)(m >> 32);
        }
    }
    return (uint32_t)(m >> 32);
}
#endif

}  // namespace fbx
