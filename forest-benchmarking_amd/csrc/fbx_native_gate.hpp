// fbx_native_gate.hpp -- the passes of the native-gate simulator (fbx_native.hip) over a state that sits in LDS
// behind qv_slot (fbx_qv_gate.hpp, whose functions stay as they were timed).  A compiled circuit is almost all one-qubit gates,
// so none of them goes through the 4 x 4 product of qv_apply_gate: RX is a pass over the N / 2 pairs of its qubit, RZ and CZ
// are passes over the N amplitudes without pairing (one complex multiply, or only a sign), and XY -- which pairs |01> with |10> --
// and the diagonal gates that are followed by a Pauli with an X part take the pair / group form.  The Pauli X^x Z^z of an error is
// folded into the gate's own pass as in qv_apply_gate_pauli: output r goes to the slot of r ^ x with its sign flipped where
// z . r is odd.  p, p0, p1 are index bits (bit p = qubit n - 1 - p), (c, s) = (cos, sin) of half the gate's angle; all arguments
// but tid are wave-uniform.  The caller separates passes with its barrier.
#pragma once
#include "fbx_qv_gate.hpp"

namespace fbx {

// RX(theta) = [[c, -i s], [-i s, c]] on index bit p, then X^x Z^z (x, z in {0, 1}).  (c, s) = (1, 0) is the bare Pauli.
__device__ __forceinline__ void nat_apply_rx(cplx* S, int pairs, int p, double c, double s, int x, int z, int tid, int nth) {
    const int lomask = (1 << p) - 1, t = qv_slot(1 << p), tx = x ? t : 0, sg = (int)((unsigned)(z & 1) << 31);
    for (int g = tid; g < pairs; g += nth) {
        const int s0 = qv_slot(((g & ~lomask) << 1) | (g & lomask)), s1 = s0 ^ t;
        const cplx a0 = S[s0], a1 = S[s1];
        const cplx o0{c * a0.re + s * a1.im, c * a0.im - s * a1.re};
        const cplx o1{c * a1.re + s * a0.im, c * a1.im - s * a0.re};
        S[s0 ^ tx] = o0;
        S[s1 ^ tx] = cplx{qv_flip_sign(o1.re, sg), qv_flip_sign(o1.im, sg)};
    }
}

// RZ(theta) = diag(c - i s, c + i s) on index bit p, then Z^z: no pairing
__device__ __forceinline__ void nat_apply_rz(cplx* S, int N, int p, double c, double s, int z, int tid, int nth) {
    const int sg = (int)((unsigned)(z & 1) << 31);
    for (int i = tid; i < N; i += nth) {
        const int b = (i >> p) & 1, sl = qv_slot(i);
        const cplx a = S[sl];
        const double sb = b ? s : -s;
        const int f = b ? sg : 0;
        S[sl] = cplx{qv_flip_sign(c * a.re - sb * a.im, f), qv_flip_sign(c * a.im + sb * a.re, f)};
    }
}

// ... followed by X Z^z: the two amplitudes of a pair change places
__device__ __forceinline__ void nat_apply_rz_x(cplx* S, int pairs, int p, double c, double s, int z, int tid, int nth) {
    const int lomask = (1 << p) - 1, t = qv_slot(1 << p), sg = (int)((unsigned)(z & 1) << 31);
    for (int g = tid; g < pairs; g += nth) {
        const int s0 = qv_slot(((g & ~lomask) << 1) | (g & lomask)), s1 = s0 ^ t;
        const cplx a0 = S[s0], a1 = S[s1];
        S[s1] = cplx{c * a0.re + s * a0.im, c * a0.im - s * a0.re};
        S[s0] = cplx{qv_flip_sign(c * a1.re - s * a1.im, sg), qv_flip_sign(c * a1.im + s * a1.re, sg)};
    }
}

// CZ on index bits p0, p1, then Z^z (bit 1 of z = the qubit of p0, bit 0 = that of p1): a sign per amplitude, no arithmetic
__device__ __forceinline__ void nat_apply_cz(cplx* S, int N, int p0, int p1, int z, int tid, int nth) {
    const int z0 = (z >> 1) & 1, z1 = z & 1;
    for (int i = tid; i < N; i += nth) {
        const int b0 = (i >> p0) & 1, b1 = (i >> p1) & 1, sl = qv_slot(i);
        const int f = (int)((unsigned)((b0 & b1) ^ (b0 & z0) ^ (b1 & z1)) << 31);
        const cplx a = S[sl];
        S[sl] = cplx{qv_flip_sign(a.re, f), qv_flip_sign(a.im, f)};
    }
}

// The group form, a thread per group of four as qv_apply_gate_pauli: XY(theta) = 1 (+) [[c, i s], [i s, c]] (+) 1 (IS_XY), or CZ,
// then X^x Z^z with two-bit masks (bit 1 = the qubit of p0, bit 0 = that of p1)
template <bool IS_XY>
__device__ __forceinline__ void nat_apply_group(cplx* S, int groups, int p0, int p1, double c, double s, int x, int z, int tid, int nth) {
    const int lo = p0 < p1 ? p0 : p1, hi = p0 < p1 ? p1 : p0;
    const int lomask = (1 << lo) - 1, himask = (1 << hi) - 1;
    const int t0 = qv_slot(1 << p0), t1 = qv_slot(1 << p1);
    const int tx = ((x & 2) ? t0 : 0) ^ ((x & 1) ? t1 : 0);
    const int sg1 = (int)((unsigned)(z & 1) << 31), sg2 = (int)((unsigned)(z & 2) << 30);
    const int sg3 = sg1 ^ sg2 ^ (IS_XY ? 0 : (int)0x80000000u);                     // CZ: the sign of |11>
    for (int g = tid; g < groups; g += nth) {
        int base = ((g & ~lomask) << 1) | (g & lomask);
        base = ((base & ~himask) << 1) | (base & himask);
        const int s0 = qv_slot(base), s1 = s0 ^ t1, s2 = s0 ^ t0, s3 = s2 ^ t1;
        const cplx a0 = S[s0], a1 = S[s1], a2 = S[s2], a3 = S[s3];                 // (bit of p0, bit of p1) = 00, 01, 10, 11
        cplx o1 = a1, o2 = a2;
        if constexpr (IS_XY) {
            o1 = cplx{c * a1.re - s * a2.im, c * a1.im + s * a2.re};
            o2 = cplx{c * a2.re - s * a1.im, c * a2.im + s * a1.re};
        }
        S[s0 ^ tx] = a0;
        S[s1 ^ tx] = cplx{qv_flip_sign(o1.re, sg1), qv_flip_sign(o1.im, sg1)};
        S[s2 ^ tx] = cplx{qv_flip_sign(o2.re, sg2), qv_flip_sign(o2.im, sg2)};
        S[s3 ^ tx] = cplx{qv_flip_sign(a3.re, sg3), qv_flip_sign(a3.im, sg3)};
    }
}

}  // namespace fbx
