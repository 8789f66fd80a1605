// fbx_qv_gate.hpp -- what the quantum-volume simulators share: the LDS swizzle of a state (or of a tile of one) and the step that
// applies one two-qubit gate to it.  fbx_qvolume.hip (whole state in LDS, widths 2..13) and fbx_qvolume_wide.hip (state in HBM, a
// tile of it in LDS, widths 14..26) both go through qv_apply_gate, so the arithmetic of a 4-amplitude group is written once.
#pragma once
#include "fbx_common.hpp"

namespace fbx {

// The bank swizzle of fbx_qvolume.hip's header comment: linear over GF(2), a bijection of every aligned block of 128 slots.
__device__ __forceinline__ int qv_slot(int i) { return i ^ (((i >> 3) & 1) * 7) ^ ((i >> 1) & 8) ^ ((i >> 5) & 3); }

// inclusive prefix sum over the 64 lanes of a wavefront (all lanes active)
__device__ __forceinline__ unsigned wave_scan_u32(unsigned v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// One gate on the swizzled state S of 4 * groups slots: p0 / p1 are the index bits of q0 / q1 (wave-uniform), U the 32 doubles of
// the 4 x 4 matrix (wave-uniform pointer: scalar loads).  Thread tid of nth owns the groups tid, tid + nth, ...: the group counter
// with zero bits inserted at the two target places.  The caller separates gates with its barrier.
__device__ __forceinline__ void qv_apply_gate(cplx* S, int groups, int p0, int p1, const double* __restrict__ U, int tid, int nth) {
    const int lo = p0 < p1 ? p0 : p1, hi = p0 < p1 ? p1 : p0;
    const int m0 = 1 << p0, m1 = 1 << p1, lomask = (1 << lo) - 1, himask = (1 << hi) - 1;
    const int t0 = qv_slot(m0), t1 = qv_slot(m1);                                 // the swizzle is linear
    double ur[16], ui[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { ur[e] = U[2 * e]; ui[e] = U[2 * e + 1]; }
    for (int g = tid; g < groups; g += nth) {
        int base = ((g & ~lomask) << 1) | (g & lomask);
        base = ((base & ~himask) << 1) | (base & himask);
        const int s0 = qv_slot(base), s1 = s0 ^ t1, s2 = s0 ^ t0, s3 = s2 ^ t1;
        const cplx a0 = S[s0], a1 = S[s1], a2 = S[s2], a3 = S[s3];                 // (bit of q0, bit of q1) = 00, 01, 10, 11
        cplx o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double re = ur[4 * r] * a0.re - ui[4 * r] * a0.im;
            double im = ur[4 * r] * a0.im + ui[4 * r] * a0.re;
            re += ur[4 * r + 1] * a1.re - ui[4 * r + 1] * a1.im;
            im += ur[4 * r + 1] * a1.im + ui[4 * r + 1] * a1.re;
            re += ur[4 * r + 2] * a2.re - ui[4 * r + 2] * a2.im;
            im += ur[4 * r + 2] * a2.im + ui[4 * r + 2] * a2.re;
            re += ur[4 * r + 3] * a3.re - ui[4 * r + 3] * a3.im;
            im += ur[4 * r + 3] * a3.im + ui[4 * r + 3] * a3.re;
            o[r] = cplx{re, im};
        }
        S[s0] = o[0]; S[s1] = o[1]; S[s2] = o[2]; S[s3] = o[3];
    }
}

// multiply by -1 where bit 31 of `sign` is set (0 or 0x80000000, wave-uniform): one XOR on the high word
__device__ __forceinline__ double qv_flip_sign(double v, int sign) { return __hiloint2double(__double2hiint(v) ^ sign, __double2loint(v)); }

// qv_apply_gate followed by the Pauli X^x Z^z on the gate's pair, in the same pass (fbx_qvolume_noisy.hip): x and z are two-bit
// wave-uniform masks over the matrix index (bit 1 = q0, bit 0 = q1).  X^x Z^z |r> = (-1)^(z . r) |r ^ x>, so output r goes to the
// slot of r ^ x -- one XOR on the group's base slot -- with its sign flipped where z . r is odd.  The arithmetic of the group is
// that of qv_apply_gate term for term (which stays as it is for the two simulators that were timed with it): x = z = 0 gives its
// result bit for bit, and any (x, z) gives bit for bit what qv_apply_gate makes of the matrix (X^x Z^z) U.
__device__ __forceinline__ void qv_apply_gate_pauli(cplx* S, int groups, int p0, int p1, const double* __restrict__ U, int x, int z,
                                                    int tid, int nth) {
    const int lo = p0 < p1 ? p0 : p1, hi = p0 < p1 ? p1 : p0;
    const int m0 = 1 << p0, m1 = 1 << p1, lomask = (1 << lo) - 1, himask = (1 << hi) - 1;
    const int t0 = qv_slot(m0), t1 = qv_slot(m1);                                 // the swizzle is linear
    const int tx = ((x & 2) ? t0 : 0) ^ ((x & 1) ? t1 : 0);
    const int sg1 = (int)((unsigned)(z & 1) << 31), sg2 = (int)((unsigned)(z & 2) << 30), sg3 = sg1 ^ sg2;   // outputs r = 1, 2, 3 (r = 0: none)
    double ur[16], ui[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { ur[e] = U[2 * e]; ui[e] = U[2 * e + 1]; }
    for (int g = tid; g < groups; g += nth) {
        int base = ((g & ~lomask) << 1) | (g & lomask);
        base = ((base & ~himask) << 1) | (base & himask);
        const int s0 = qv_slot(base), s1 = s0 ^ t1, s2 = s0 ^ t0, s3 = s2 ^ t1;
        const cplx a0 = S[s0], a1 = S[s1], a2 = S[s2], a3 = S[s3];                 // (bit of q0, bit of q1) = 00, 01, 10, 11
        cplx o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double re = ur[4 * r] * a0.re - ui[4 * r] * a0.im;
            double im = ur[4 * r] * a0.im + ui[4 * r] * a0.re;
            re += ur[4 * r + 1] * a1.re - ui[4 * r + 1] * a1.im;
            im += ur[4 * r + 1] * a1.im + ui[4 * r + 1] * a1.re;
            re += ur[4 * r + 2] * a2.re - ui[4 * r + 2] * a2.im;
            im += ur[4 * r + 2] * a2.im + ui[4 * r + 2] * a2.re;
            re += ur[4 * r + 3] * a3.re - ui[4 * r + 3] * a3.im;
            im += ur[4 * r + 3] * a3.im + ui[4 * r + 3] * a3.re;
            o[r] = cplx{re, im};
        }
        S[s0 ^ tx] = o[0];
        S[s1 ^ tx] = cplx{qv_flip_sign(o[1].re, sg1), qv_flip_sign(o[1].im, sg1)};
        S[s2 ^ tx] = cplx{qv_flip_sign(o[2].re, sg2), qv_flip_sign(o[2].im, sg2)};
        S[s3 ^ tx] = cplx{qv_flip_sign(o[3].re, sg3), qv_flip_sign(o[3].im, sg3)};
    }
}

}  // namespace fbx
