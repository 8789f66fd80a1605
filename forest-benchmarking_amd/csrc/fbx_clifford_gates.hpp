// fbx_clifford_gates.hpp -- what every translation unit that walks a Clifford circuit shares (fbx_dfe.hip, fbx_frames.hip): the
// conjugation of a Pauli (two 64-bit masks and a sign bit) by one gate word, the walk through a whole circuit, and the host checks
// of a circuit given by host words.  The table and the validation rule are those of include/fbx.h.
#pragma once
#include "fbx_common.hpp"

namespace fbx {

constexpr int DFE_MAX_CLASSES = 16;

__host__ __device__ __forceinline__ uint64_t dfe_valid_mask(int n) { return ~(uint64_t)0 >> (64 - n); }    // n in 1..64: no shift by 64

__host__ __device__ __forceinline__ uint32_t dfe_inverse_opcode(uint32_t op) {
    switch (op) {
        case FBX_GATE_S: return FBX_GATE_SDG;
        case FBX_GATE_SDG: return FBX_GATE_S;
        case FBX_GATE_RX_PLUS: return FBX_GATE_RX_MINUS;
        case FBX_GATE_RX_MINUS: return FBX_GATE_RX_PLUS;
        case FBX_GATE_RY_PLUS: return FBX_GATE_RY_MINUS;
        case FBX_GATE_RY_MINUS: return FBX_GATE_RY_PLUS;
        case FBX_GATE_RZ_PLUS: return FBX_GATE_RZ_MINUS;
        case FBX_GATE_RZ_MINUS: return FBX_GATE_RZ_PLUS;
        default: return op;
    }
}

#if defined(__HIPCC__)

// P <- U P U^+ for the gate with opcode `op` on q0 (and q1); the table of include/fbx.h.  The word is wave-uniform.  Qubit indices are
// reduced mod 64 and an unknown opcode does nothing: a word the caller did not validate gives an unspecified Pauli, nothing else.
__device__ __forceinline__ void dfe_apply_gate(uint32_t op, uint32_t q0, uint32_t q1, uint64_t& x, uint64_t& z, uint32_t& sign) {
    q0 &= 63u; q1 &= 63u;
    const uint64_t xa = (x >> q0) & 1u, za = (z >> q0) & 1u;
    uint64_t s = 0;
    switch (op) {
        case FBX_GATE_H:        s = xa & za;  x ^= (xa ^ za) << q0; z ^= (xa ^ za) << q0; break;
        case FBX_GATE_S:
        case FBX_GATE_RZ_PLUS:  s = xa & za;  z ^= xa << q0; break;
        case FBX_GATE_SDG:
        case FBX_GATE_RZ_MINUS: s = xa & ~za; z ^= xa << q0; break;
        case FBX_GATE_X:        s = za; break;
        case FBX_GATE_Y:        s = xa ^ za; break;
        case FBX_GATE_Z:        s = xa; break;
        case FBX_GATE_RX_PLUS:  s = za & ~xa; x ^= za << q0; break;
        case FBX_GATE_RX_MINUS: s = za & xa;  x ^= za << q0; break;
        case FBX_GATE_RY_PLUS:  s = xa & ~za; x ^= (xa ^ za) << q0; z ^= (xa ^ za) << q0; break;
        case FBX_GATE_RY_MINUS: s = za & ~xa; x ^= (xa ^ za) << q0; z ^= (xa ^ za) << q0; break;
        case FBX_GATE_CNOT: {
            const uint64_t xb = (x >> q1) & 1u, zb = (z >> q1) & 1u;
            s = xa & zb & ~(xb ^ za);
            x ^= xa << q1; z ^= zb << q0;
            break;
        }
        case FBX_GATE_CZ: {
            const uint64_t xb = (x >> q1) & 1u, zb = (z >> q1) & 1u;
            s = xa & xb & (za ^ zb);
            z ^= (xb << q0) ^ (xa << q1);
            break;
        }
        case FBX_GATE_SWAP: {
            const uint64_t xb = (x >> q1) & 1u, zb = (z >> q1) & 1u;
            x ^= ((xa ^ xb) << q0) | ((xa ^ xb) << q1);
            z ^= ((za ^ zb) << q0) | ((za ^ zb) << q1);
            break;
        }
        default: break;
    }
    sign ^= (uint32_t)(s & 1u);
}

// The whole circuit: inverse == 0 gives U P U^+ (gates in index order), 1 gives U^+ P U (backwards, each gate inverted).
__device__ __forceinline__ void dfe_walk(const uint32_t* __restrict__ gates, long long G, int inverse, uint64_t& x, uint64_t& z,
                                         uint32_t& sign) {
    if (!inverse) {
        for (long long g = 0; g < G; ++g) {
            const uint32_t w = gates[g];
            dfe_apply_gate(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, x, z, sign);
        }
    } else {
        for (long long g = G - 1; g >= 0; --g) {
            const uint32_t w = gates[g];
            dfe_apply_gate(dfe_inverse_opcode(w & 0xFFu), (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, x, z, sign);
        }
    }
}

__device__ __forceinline__ bool dfe_bad_probability(double v) { return !(v >= 0.0 && v <= 1.0); }      // NaN included

#endif

// ------------------------------------------------------------------ host: argument checks
static inline int dfe_check_width(const char* who, int n) {
    if (n < 1 || n > 64) { set_error(std::string(who) + ": n_qubits must be 1..64"); return FBX_ERR_BAD_ARG; }
    return FBX_OK;
}

// a circuit given by HOST words: every opcode known, every qubit index below n, q0 != q1 on a two-qubit gate, nothing above bit 23
static inline int dfe_check_gates(const char* who, int n, int64_t G, const uint32_t* gates) {
    for (int64_t g = 0; g < G; ++g) {
        const uint32_t w = gates[g], op = w & 0xFFu, q0 = (w >> 8) & 0xFFu, q1 = (w >> 16) & 0xFFu;
        const bool two = op >= FBX_GATE_CNOT;
        const bool ok = op <= FBX_GATE_SWAP && (w >> 24) == 0 && q0 < (uint32_t)n && (two ? (q1 < (uint32_t)n && q1 != q0) : q1 == 0);
        if (!ok) { set_error(std::string(who) + ": gate " + std::to_string(g) + " is not a valid gate word for this width"); return FBX_ERR_BAD_ARG; }
    }
    return FBX_OK;
}

static inline int dfe_check_circuit(const char* who, int n, int64_t G, const void* gates) {
    FBX_TRY(dfe_check_width(who, n));
    if (G < 0) { set_error(std::string(who) + ": negative gate count"); return FBX_ERR_BAD_ARG; }
    if (G > 0 && !gates) { set_error(std::string(who) + ": NULL gates"); return FBX_ERR_BAD_ARG; }
    return FBX_OK;
}

// the noise classes of a circuit given by HOST bytes: each below K or FBX_DFE_NOISELESS
static inline int dfe_check_classes(const char* who, int K, int64_t G, const uint8_t* noise_class) {
    if (noise_class)
        for (int64_t g = 0; g < G; ++g)
            if (!(noise_class[g] < K || noise_class[g] == FBX_DFE_NOISELESS)) {
                set_error(std::string(who) + ": a noise class is neither below K nor 255");
                return FBX_ERR_BAD_ARG;
            }
    return FBX_OK;
}

}  // namespace fbx
