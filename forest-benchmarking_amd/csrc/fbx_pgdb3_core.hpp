// fbx_pgdb3_core.hpp -- the building blocks of the 3-qubit (64 x 64 Choi) kernels of fbx_pgdb3.hip, one 1024-thread workgroup per
// reconstruction: the LDS carving, the workgroup reductions, the change of basis on the matrix cores, the CP / TP / TNI projections
// and Dykstra's loop over them, the Choi <-> Pauli transforms and the two table products of the gradient.
// Included by fbx_pgdb3.hip BEHIND its barrier-mode defines (FBX_LDS_ONLY_BARRIERS / -DFBX_FULL_BARRIERS, fbx_common.hpp).
//
// Reference: tomography.py:542-633, operator_tools/project_superoperators.py:19-144.
#pragma once
#include "fbx_choi.hpp"
#include "fbx_eigh64.hpp"
#include <type_traits>

namespace fbx {
#define FBX3_BASIS_STEP 3e-2           // outer step below which Dykstra iteration j starts from the previous call's basis j.  The 2-qubit kernel's
                                       // 1e-3 (FBX_BASIS_STEP) is too timid here: same-box A/B (scripts/ab_time3.py, 256 items) 331.6 ms at
                                       // 1e-3 / 3e-2, 324.4 at 1e-2 / 1e-1, 317.2 at 3e-2 / 3e-1, 317.1 at 1e-1 / 1 -- a starting basis only
                                       // changes how many sweeps a decomposition needs, never the tolerance it runs to
#define FBX3_BASIS_WRITE_STEP 3e-1     // outer step below which every basis is written back (10 x the threshold above, as in the 2-qubit kernel)
#define FBX3_BASIS_CHAIN_SWEEPS 216   // as FBX_BASIS_CHAIN_SWEEPS of the 2-qubit kernel (fbx_pgdb.hip)

namespace p3 {
constexpr int NQ = 3, d = 8, D = 64, NB = 32, NT = 1024, LD = 64, LDs = d + 1;
constexpr double EPS = 1e-6, GAMMA = 0.3, STOP = 1e-10, ALPHA_MIN = 1e-15;

struct Lds {
    cplx* Ms;        // [4096] Jacobi work matrix (element-major)
    cplx* Vs;        // [4096] eigenvectors
    cplx* Mw;        // = Vs: row-major 64 x 64 staging (partial trace, Pauli butterflies)
    double* T;       // = Ms..: prediction table [S][64] / gradient accumulator W[64][S]
    double* Rt;      // [4096] Pauli coefficients, TRANSPOSED: Rt[j * 64 + i] = R[i][j]
    // overlay on Rt (alive only while R is dead):
    cplx* pt; cplx* pts; cplx* ptV; cplx* ptold; double* lam; double* red;
    PhaseClock* pc;  // diagnostics (-DFBX_PHASE_TIMERS)
    int terms = 0;   // work accounting: eigenvalue terms rebuilt by the CP projections
    double jtol2 = FBX_JACOBI_TOL2;   // eigensolver tolerance of the CP projections (see fbx_pgdb.hip, FBX_JTOL_REL)
    __device__ void carve(char* p) {
        Ms = (cplx*)p; Vs = Ms + D * D; Mw = Vs; T = (double*)p;
        Rt = (double*)(p + 2 * sizeof(cplx) * D * D);
        char* q = (char*)Rt;
        pt = (cplx*)q; q += sizeof(cplx) * d * LDs;
        pts = (cplx*)q; q += sizeof(cplx) * d * d;
        ptV = (cplx*)q; q += sizeof(cplx) * d * d;
        ptold = (cplx*)q; q += sizeof(cplx) * d * LDs;
        lam = (double*)q; q += sizeof(double) * D;
        red = (double*)q;
    }
    static constexpr size_t bytes() { return 2 * sizeof(cplx) * D * D + sizeof(double) * D * D; }
};

__device__ __forceinline__ double bsum(double v, Lds& L) { return block_sum<NT>(v, L.red); }
// K <= 8 sums over the workgroup with ONE barrier pair instead of K (every thread gets all totals).  Second stage (round 5): lane
// 16 k + w of every wavefront reads the partial sum of wavefront w for value k (two loads per lane for K > 4) and the sixteen
// partials are added by four DPP steps inside the row -- instead of 16 K broadcast loads and additions per thread (128 LDS
// loads per thread and call for the Dykstra stopping functional: 17 k cycles of the ~420 k of a Dykstra iteration).
template <int K>
__device__ __forceinline__ void bsum_multi(double (&v)[K], Lds& L) {
    static_assert((K <= 4 || K == 8) && NT / 64 == 16, "sixteen wavefronts; the second-stage load of values 4 .. K - 1 indexes with a mask: K x 16 must be a power of two");
    const int lane = threadIdx.x & 63;
    double mine = 0.0;                                  // lane k < K publishes value k of this wavefront
#pragma unroll
    for (int k = 0; k < K; ++k) { const double w = wave_sum(v[k]); mine = lane == k ? w : mine; }
    FBX_BLOCK_SYNC();                                   // earlier readers of `red` are done
    if (lane < K) L.red[lane * (NT / 64) + (threadIdx.x >> 6)] = mine;
    FBX_BLOCK_SYNC();
    double a = L.red[lane], b = K > 4 ? L.red[(64 + lane) & (K * (NT / 64) - 1)] : 0.0;
    a += dpp_permute<0xB1>(a); a += dpp_permute<0x4E>(a); a += dpp_permute<0x141>(a); a += dpp_permute<0x140>(a);
    if constexpr (K > 4) { b += dpp_permute<0xB1>(b); b += dpp_permute<0x4E>(b); b += dpp_permute<0x141>(b); b += dpp_permute<0x140>(b); }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = k < 4 ? readlane_f64(a, 16 * k) : readlane_f64(b, 16 * (k - 4));
}

// ---- warm start: Ms <- V^H Ms V for the eigenvectors V of the previous projection (still in Vs), on the fp64 matrix cores.
// LDS is full, but the intermediate product T = Ms V can take the place of Ms itself once every wavefront holds its tile of it.
// Wavefront w owns the 16 x 16 output tile (w >> 2, w & 3) of
// each of the two 64^3 complex products, 16 k-steps of four v_mfma_f64_16x16x4_f64 (re.re, -im.im, re.im, im.re).
// Lane l feeds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; accumulator r is D[(l >> 4) + 4 r][l & 15].
// Both A operands are read TRANSPOSED so that the 16 lanes of a group walk along a row of the layout:
// H[m][k] = conj(H[k][m]) (H is exactly Hermitian: it was just symmetrised) and (V^H)[m][k] = conj(V[k][m]).
// 2 x 16 x 2 b128 loads and 8 stores per lane instead of 2 x 64 x 4 loads; the products themselves take
// 128 x 32 cycles per wavefront (the VALU form: 68.7 k cycles per decomposition, this one: see DESIGN.md 4.4).
__device__ void rotate_into_basis_mfma(Lds& L, int t) {
    typedef double v4d __attribute__((ext_vector_type(4)));
    t = opaque(t);
    const int w = t >> 6, l = t & 63, tm = w >> 2, tn = w & 3, g = l >> 4, c = l & 15;
    const int colA = 16 * tm + c, colB = 16 * tn + c;
    v4d tre = {0.0, 0.0, 0.0, 0.0}, tim = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {                   // T = H V
        const int k = 4 * ks + g;
        const cplx h = L.Ms[sys_index<D>(k, colA)];     // conj(H[colA][k])
        const cplx v = L.Vs[sys_index<D>(k, colB)];     // V[k][colB]
        tre = __builtin_amdgcn_mfma_f64_16x16x4f64(h.re, v.re, tre, 0, 0, 0);
        tim = __builtin_amdgcn_mfma_f64_16x16x4f64(h.re, v.im, tim, 0, 0, 0);
        tre = __builtin_amdgcn_mfma_f64_16x16x4f64(h.im, v.im, tre, 0, 0, 0);      // -(-im) im
        tim = __builtin_amdgcn_mfma_f64_16x16x4f64(-h.im, v.re, tim, 0, 0, 0);
    }
    FBX_BLOCK_SYNC();                                    // H is dead: T takes its place
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        cplx o; o.re = tre[r]; o.im = tim[r];
        L.Ms[sys_index<D>(16 * tm + g + 4 * r, colB)] = o;
    }
    FBX_BLOCK_SYNC();
    // M' = V^H T is Hermitian and the eigensolver reads its upper block triangle only: the ten tiles (tm2 <= tn2) go to wavefronts
    // 0-9 -- three tiles on two of the matrix-core pipes, two on the others, instead of four on each.  The six tiles below the
    // diagonal keep T (proj_cp's norm check counts the upper tiles twice instead).
    const bool upper = w < 10;
    const int tm2 = w < 4 ? 0 : w < 7 ? 1 : w < 9 ? 2 : 3, tn2 = w < 4 ? w : w < 7 ? w - 3 : w < 9 ? w - 5 : 3;
    const int colA2 = 16 * tm2 + c, colB2 = 16 * tn2 + c;
    v4d mre = {0.0, 0.0, 0.0, 0.0}, mim = {0.0, 0.0, 0.0, 0.0};
    if (upper) {
#pragma unroll 4
        for (int ks = 0; ks < 16; ++ks) {               // M' = V^H T
            const int k = 4 * ks + g;
            const cplx v = L.Vs[sys_index<D>(k, colA2)];    // conj((V^H)[colA2][k])
            const cplx q = L.Ms[sys_index<D>(k, colB2)];    // T[k][colB2]
            mre = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, q.re, mre, 0, 0, 0);
            mim = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, q.im, mim, 0, 0, 0);
            mre = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, q.im, mre, 0, 0, 0);
            mim = __builtin_amdgcn_mfma_f64_16x16x4f64(-v.im, q.re, mim, 0, 0, 0);
        }
    }
    FBX_BLOCK_SYNC();                                    // every wavefront is done reading T
    if (upper) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * tm2 + g + 4 * r;
            cplx o; o.re = mre[r]; o.im = row == colB2 ? 0.0 : mim[r];
            L.Ms[sys_index<D>(row, colB2)] = o;
        }
    }
    FBX_BLOCK_SYNC();
}

// The 64 x 64 eigensolver is INLINED into the kernels (behind a call boundary -- tried in round 4, when its per-thread address constants
// were hoisted out of the Dykstra loop and spilled -- the role-split solver needs more than the 80 caller-saved registers and saved 49
// more to scratch per call: 296 against 274 ms per 256 reconstructions).
__device__ __forceinline__
int jacobi64(cplx* Ms, cplx* Vs, int t, bool init_identity, double* red, double tol2) {
    t = opaque(t);
    return jacobi_eigh64<NT>(Ms, Vs, t, init_identity, red, tol2);     // fbx_eigh64.hpp
}

// ---- V diag(lam) V^H for the 64 x 64 eigenvectors in Vs: the block of thread (I, J) is sum_k lam_k V[2I + a][k] conj(V[2J + b][k]).
// The first factor is the same for the 32 lanes of a block row (a broadcast read); the second walks DOWN a column of the
// layout -- a stride of 32 entries, 8-way bank conflicts on two of the four b128 reads of every term: the generic
// reconstruct_blk was LDS-bound at ~1300 cycles per eigenvalue term (34 k cycles per call, 5.8 % of the kernel).  Here V is
// first copied TRANSPOSED into Ms (dead once the eigenvalues are in L.lam), block (J, I) at J * 32 + (I ^ J): the XOR makes the
// eight blocks a lane group writes AND the eight it later reads fall on eight different bank groups, so both factors are
// conflict-free reads.  Same terms in the same order: bit-identical to reconstruct_blk<64>.
__device__ Blk reconstruct64(Lds& L, int t) {
    constexpr int PS = sys_plane<D>();
    t = opaque(t);
    const int I = t / NB, J = t % NB;
#pragma unroll
    for (int e = 0; e < 4; ++e) {                          // V[2I + a][2J + b] -> VT[2J + b][2I + a]
        const int a = e >> 1, b = e & 1;
        L.Ms[(b * 2 + a) * PS + J * NB + (I ^ J)] = L.Vs[e * PS + sys_pos<D>(I, J, e)];
    }
    FBX_BLOCK_SYNC();
    Blk out = blk_zero();
    const int wl = t & 63;
    const double mine = L.lam[wl];
    unsigned long long todo = __ballot(mine != 0.0);
    while (todo) {
        const int k = __builtin_ctzll(todo);
        todo &= todo - 1;
        const double l = readlane_f64(mine, k);
        const int kb = k >> 1, ke = k & 1;
        const int rk = sys_pos<D>(I, kb, ke);
        const cplx r0 = L.Vs[(0 + ke) * PS + rk], r1 = L.Vs[(2 + ke) * PS + rk];
        const cplx c0 = L.Ms[(ke * 2 + 0) * PS + kb * NB + (J ^ kb)], c1 = L.Ms[(ke * 2 + 1) * PS + kb * NB + (J ^ kb)];
        const double w0r = l * r0.re, w0i = l * r0.im, w1r = l * r1.re, w1i = l * r1.im;
        out.re[0] += w0r * c0.re + w0i * c0.im; out.im[0] += w0i * c0.re - w0r * c0.im;
        out.re[1] += w0r * c1.re + w0i * c1.im; out.im[1] += w0i * c1.re - w0r * c1.im;
        out.re[2] += w1r * c0.re + w1i * c0.im; out.im[2] += w1i * c0.re - w1r * c0.im;
        out.re[3] += w1r * c1.re + w1i * c1.im; out.im[3] += w1i * c1.re - w1r * c1.im;
    }
    return out;
}

// ---- CP projection (project_superoperators.py:19-34)
// Hermitised copy of x into Ms (element-major layout); returns ||h||_F^2's per-thread part when asked
__device__ __forceinline__ double hermitise_into_ms(const Blk& x, Lds& L, int t, bool want_norm) {
    t = opaque(t);
    FBX_BLOCK_SYNC();
    // the transposed copy goes through a layout of its own: block (I, J) of plane e at e * PS + I * 32 + (I ^ J), so that the
    // eight blocks a lane group writes (eight column pairs of one row) AND the eight it reads back (eight ROW pairs of one column:
    // a stride of 32 entries in the solver's layout, 8-way bank conflicts on every b128 read) fall on eight different bank groups
    Blk xa;
    {
        constexpr int PS = sys_plane<D>();
        const int I = t / NB, J = t % NB, sw = I ^ J;
#pragma unroll
        for (int e = 0; e < 4; ++e) { cplx c; c.re = x.re[e]; c.im = x.im[e]; L.Ms[e * PS + I * NB + sw] = c; }
        FBX_BLOCK_SYNC();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int et = (e & 1) * 2 + (e >> 1);
            const cplx c = L.Ms[et * PS + J * NB + sw];
            xa.re[e] = c.re; xa.im[e] = -c.im;
        }
    }
    Blk h;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h.re[e] = 0.5 * (x.re[e] + xa.re[e]); h.im[e] = 0.5 * (x.im[e] + xa.im[e]); }
    FBX_BLOCK_SYNC();
    sys_store<D>(L.Ms, t, h);
    FBX_BLOCK_SYNC();
    return want_norm ? blk_norm2(h) : 0.0;
}
__device__ __forceinline__ Blk proj_cp(const Blk& x_, Lds& L, int t_, int& sweeps, bool warm = false, bool check_basis = false) {
    const Blk x = x_;
    int t = t_;
    // (the Hermitised matrix lives in LDS only: a register copy kept for the rare rejected basis would stay live
    // across the eigensolver -- 16 of 128 registers; the rejection path rebuilds it from x instead)
    double n2[2] = {0.0, 0.0};
    n2[0] = hermitise_into_ms(x, L, t, warm && check_basis);
    PH_STOP(*L.pc, 2);
    if (warm) {
        // a basis loaded from the store is only trusted if the change of basis kept ||.||_F^2 (unitary
        // similarity); otherwise the matrix is restored and the decomposition starts from the identity
        // (same guard as proj_cp_blk, fbx_choi.hpp)
        rotate_into_basis_mfma(L, t);
        if (check_basis) {
            {   // (the matrix-core form leaves the tiles below the diagonal unwritten: the upper ones count twice)
                const int ti = t / NB / 8, tj = t % NB / 8;      // tile of entry position t (the layout permutes column pairs inside aligned groups of 8 only)
                const double wgt = ti < tj ? 2.0 : ti == tj ? 1.0 : 0.0;
                double acc2 = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const cplx v = L.Ms[e * NT + t]; acc2 = fma(v.re, v.re, fma(v.im, v.im, acc2)); }
                n2[1] = wgt * acc2;
            }
            bsum_multi<2>(n2, L);
            if (!(fabs(n2[1] - n2[0]) <= FBX_BASIS_NORM_TOL * n2[0])) {
                (void)hermitise_into_ms(x, L, t, false);
                warm = false;
            }
        }
    }
    PH_STOP(*L.pc, 6);
    sweeps += jacobi64(L.Ms, L.Vs, t, !warm, L.red, L.jtol2);
    t = opaque(t);
    PH_STOP(*L.pc, 0);
    if (t < D) {
        const double l = L.Ms[sys_index<D>(t, t)].re;
        L.lam[t] = l < 0.0 ? 0.0 : l;
    }
    FBX_BLOCK_SYNC();
    // work accounting: eigenvalue terms the reconstruction walks (thread 0 reports it; every wavefront holds lam[lane])
    L.terms += __popcll(__ballot(L.lam[t & 63] != 0.0));
    const Blk out = reconstruct64(L, t);
    PH_STOP(*L.pc, 1);
    return out;
}

// ---- partial trace over the output space into L.pt (calculational.py:5-35); stages x through Mw
__device__ void partial_trace_out(const Blk& x, Lds& L, int t) {
    t = opaque(t);
    // staged row-major through Ms (dead between the reconstruction and the next projection), NOT
    // through Mw = Vs: the eigenvectors in Vs must survive for the warm start of the next projection
    cplx* St = L.Ms;
    FBX_BLOCK_SYNC();
    blk_store<D, LD>(St, t, x);
    FBX_BLOCK_SYNC();
    if (t < d * d) {
        const int i = t / d, ip = t % d;
        cplx s; s.re = 0.0; s.im = 0.0;
#pragma unroll
        for (int o = 0; o < d; ++o) { const cplx v = St[(i * d + o) * LD + ip * d + o]; s.re += v.re; s.im += v.im; }
        L.pt[i * LDs + ip] = s;
    }
    FBX_BLOCK_SYNC();
}
__device__ __forceinline__ Blk subtract_kron_pt(const Blk& x, const Lds& L, int t) {
    Blk r = x;
    t = opaque(t);
    const int I = t / NB, J = t % NB;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = 2 * I + (e >> 1), col = 2 * J + (e & 1);
        if ((row % d) == (col % d)) { const cplx c = L.pt[(row / d) * LDs + (col / d)]; r.re[e] -= c.re / d; r.im[e] -= c.im / d; }
    }
    return r;
}
__device__ Blk proj_tp(const Blk& x, Lds& L, int t) {                 // project_superoperators.py:62-84
    partial_trace_out(x, L, t);
    if (t < d) L.pt[t * LDs + t].re -= 1.0;
    FBX_BLOCK_SYNC();
    return subtract_kron_pt(x, L, t);
}
__device__ Blk proj_tni(const Blk& x, Lds& L, int t, int& sweeps) {   // project_superoperators.py:37-59
    partial_trace_out(x, L, t);
    const Blk ptb = blk_load<d, LDs>(L.pt, t);
    const Blk pta = blk_load_adjoint<d, LDs>(L.pt, t);
    Blk h;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h.re[e] = 0.5 * (ptb.re[e] + pta.re[e]); h.im[e] = 0.5 * (ptb.im[e] + pta.im[e]); }
    FBX_BLOCK_SYNC();
    sys_store<d>(L.pts, t, h);
    FBX_BLOCK_SYNC();
    sweeps += jacobi_eigh_simple<d, NT>(L.pts, L.ptV, t, true, L.red);
    if (t < d) { const double l = L.pts[sys_index<d>(t, t)].re; L.lam[t] = l > 1.0 ? 1.0 : l; }
    FBX_BLOCK_SYNC();
    const Blk proj = reconstruct_blk<d>(L.ptV, L.lam, t);
    FBX_BLOCK_SYNC();
    blk_store<d, LDs>(L.pt, t, blk_sub(ptb, proj));
    FBX_BLOCK_SYNC();
    return subtract_kron_pt(x, L, t);
}

// one stored basis (64 KiB, the layout of Vs) from HBM / L2 into LDS without passing through registers: every lane moves
// four 16-byte entries; the LDS address of a global_load_lds is wave-uniform base + lane * 16
// s_waitcnt vmcnt(0) (gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at their maxima): the consumer side
// of basis_fetch -- global_load_lds is a VMEM load whose completion is counted by vmcnt, not by the LDS counter
__device__ __forceinline__ void wait_global_loads() { __builtin_amdgcn_s_waitcnt(0x0070); }
// Ownership: thread t moves entries e * NT + t (e = 0..3) of a stored basis in BOTH directions -- write-back (store_index below) and
// fetch -- so no thread ever reads global memory another thread wrote, which is what lets the barriers order LDS only.
__device__ __forceinline__ int store_index(int e, int t) { return e * NT + t; }
__device__ __forceinline__ void basis_fetch(const cplx* g, cplx* Vs, int t) {
    typedef __attribute__((address_space(1))) const void* gptr;
    typedef __attribute__((address_space(3))) void* lptr;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        __builtin_amdgcn_global_load_lds((gptr)(g + store_index(e, t)), (lptr)(Vs + store_index(e, t & ~63)), 16, 0, 0);
}
// block of kron(C, I_d) for the d x d matrix C staged in LDS (leading dimension LDs)
__device__ __forceinline__ Blk kron_id_blk(const cplx* C, int t) {
    Blk r = blk_zero();
    t = opaque(t);
    const int I = t / NB, J = t % NB;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = 2 * I + (e >> 1), col = 2 * J + (e & 1);
        if ((row % d) == (col % d)) { const cplx c = C[(row / d) * LDs + (col / d)]; r.re[e] = c.re; r.im[e] = c.im; }
    }
    return r;
}

// ---- Dykstra (project_superoperators.py:87-144), carried with TWO matrices per thread.
// The reference's loop state is (last_state, old_CP_change, old_TP_change, last_CP_projection).  Here:
//   * old_TP_change = new_state - pre_TP = -kron(corr / d, I_d) with corr the d x d correction the TP / TNI projection
//     subtracted (proj_tp / proj_tni leave it in L.pt): kept as that 8 x 8 matrix in LDS (L.ptold), rebuilt per entry
//     where it is used;
//   * last_CP_projection only enters through <old_CP_change, CP_projection - last_CP_projection>: the second half is
//     the scalar <new_CP_change, CP_projection> of the previous iteration (one more term of the block reduction);
//   * last_state = pre_CP + old_CP_change.
// What stays live in registers across the eigensolver is pre_CP and old_CP_change -- 32 of the 128 registers a
// thread of a 1024-thread workgroup has, next to the solver's 80 (rounds 1-2 carried four matrices + the caller's
// estimate, gradient and counts: 1.4 KB of scratch per lane and 235 GB of spill traffic per 256-item launch).
// Differences to the literal expressions are rounding-level terms of the stopping functional (threshold 1e-4).
// (Parking the two in HBM around the solver instead was tried and dropped: docs/history/experiments.md.)
// `warm_starts`: every decomposition but the first starts from the eigenvectors of the one before it (the tomography kernel; the
// stand-alone projection decomposes from the identity every time, as the reference does).  A BasisStore needs them on.
__device__ __forceinline__ Blk proj_physical(const Blk& x, bool tp, Lds& L, int t_, int& iters, int& sweeps, bool warm_starts,
                             BasisStore* store = nullptr) {
    int t = t_;
    Blk u = x;                       // pre_CP = last_state - old_CP_change
    Blk p = blk_zero();              // old_CP_change
    Blk new_state = x;
    double c0r = 0.0, c0i = 0.0;     // <old_CP_change, last_CP_projection>
    bool pf_pending = false;         // the next iteration's stored basis is on its way from HBM / L2 into Vs
    FBX_BLOCK_SYNC();
    if (t < d * LDs) { cplx z; z.re = 0.0; z.im = 0.0; L.ptold[t] = z; }     // old_TP_change = 0
    int it = 0;
    for (; it < 100000; ++it) {
        ++iters;
        // consecutive Dykstra iterates are close: start from the previous eigenvectors; when the
        // outer step was small, from the basis the previous call found at the same Dykstra
        // iteration (BasisStore, fbx_choi.hpp) -- the first projection always, it has no other
        bool warm = it > 0 && warm_starts;
        bool from_slot = false;
        if (store && warm_starts && it < store->nprev && (it == 0 || store->use_prev)) {
            from_slot = true;
            if (!pf_pending) { FBX_BLOCK_SYNC(); basis_fetch(store->g + (size_t)it * D * D, L.Vs, t); }
            wait_global_loads();                      // this wave's share of the basis has landed in LDS
            FBX_BLOCK_SYNC();
            pf_pending = false;
            warm = true;
        }
        t = opaque(t);
        const Blk cp = proj_cp(u, L, t, sweeps, warm, from_slot);
        if (store && it < store->cap && (it == 0 || store->write_all)) {      // write-back policy: BasisStore, fbx_choi.hpp
            fbx_global_cplx_ptr dst = (fbx_global_cplx_ptr)(store->g + (size_t)it * D * D);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const cplx v = L.Vs[store_index(e, t)]; dst[store_index(e, t)] = fbx_v2d{v.re, v.im}; }
        }
        double red8[8];
        const Blk new_cp = blk_sub(cp, u);
        red8[0] = blk_norm2(blk_sub(new_cp, p));                           // ||new_CP_change - old_CP_change||^2
        blk_dotc(p, cp, red8[4], red8[5]);                                 // <old_CP_change, CP_projection>
        blk_dotc(new_cp, cp, red8[6], red8[7]);                            // next iteration's <old_CP_change, last_CP_projection>
        const Blk last_state = blk_axpy(u, 1.0, p);
        // pre_TP = CP_projection - old_TP_change = CP_projection + kron(corr_old / d, I)
        const Blk old_tp = blk_axpy(blk_zero(), -1.0 / d, kron_id_blk(L.ptold, t));
        const Blk pre_tp = blk_sub(cp, old_tp);
        new_state = tp ? proj_tp(pre_tp, L, t) : proj_tni(pre_tp, L, t, sweeps);
        const Blk new_tp = blk_axpy(blk_zero(), -1.0 / d, kron_id_blk(L.pt, t));
        red8[1] = blk_norm2(blk_sub(new_tp, old_tp));                      // ||new_TP_change - old_TP_change||^2
        blk_dotc(old_tp, blk_sub(new_state, last_state), red8[2], red8[3]); // <old_TP_change, state_change>
        // (measured and dropped, round 5: contracting the state change in two halves -- (new_CP_change - old_CP_change) in front
        //  of the TP projection, the Kronecker-structured TP half behind it -- so that only new_CP_change crosses the projection:
        //  200.5 against 197.4 ms per 256 reconstructions)
        bsum_multi<8>(red8, L);
        const double i2r = red8[4] - c0r, i2i = red8[5] - c0i;
        const double crit = red8[0] + red8[1] + 2.0 * sqrt(red8[2] * red8[2] + red8[3] * red8[3]) + 2.0 * sqrt(i2r * i2r + i2i * i2i);
        if (!(crit >= 1e-4)) { ++it; break; }        // converged -- or not finite (NaN input): never spin
        c0r = red8[6]; c0i = red8[7];
        p = new_cp;
        u = blk_sub(new_state, new_cp);
        if (t < d * LDs) L.ptold[t] = L.pt[t];       // (bsum_multi's barriers separate this from the readers above; the next
                                                     //  reader is behind the barriers of proj_cp)
        // The eigenvectors in Vs are dead when the next decomposition starts from a stored basis (reconstruction and
        // write-back have read them, behind the barriers above): that basis is requested NOW, straight into LDS
        // (global_load_lds_dwordx4), and arrives while the next iteration Hermitises its matrix.
        if (store && warm_starts && it + 1 < store->nprev && store->use_prev) { basis_fetch(store->g + (size_t)(it + 1) * D * D, L.Vs, t); pf_pending = true; }
    }
    if (store) {
        const int written = store->write_all ? it : 1;
        store->nprev = written < store->cap ? written : store->cap;
    }
    return new_state;
}

// ---- Choi (in registers) -> transposed Pauli coefficients Rt (uses Mw = Vs as staging)
__device__ void choi_to_pauli(const Blk& x, Lds& L, int t) {
    t = opaque(t);
    FBX_BLOCK_SYNC();
    blk_store<D, LD>(L.Mw, t, x);
    FBX_BLOCK_SYNC();
#pragma unroll
    for (int s = NQ - 1; s >= 0; --s) { pauli_site_stage<NQ, false, LD>(L.Mw, t, 2 * NQ + NQ + s, NQ + s, -1.0); FBX_BLOCK_SYNC(); }
#pragma unroll
    for (int s = NQ - 1; s >= 0; --s) { pauli_site_stage<NQ, false, LD>(L.Mw, t, 2 * NQ + s, s, +1.0); FBX_BLOCK_SYNC(); }
    for (int idx = t; idx < D * D; idx += NT) {
        const int i = idx % D, j = idx / D;           // idx = j * 64 + i: coalesced Rt writes
        int row, col;
        pauli_coeff_position<NQ>(i, j, row, col);
        L.Rt[idx] = L.Mw[row * LD + col].re / d;
    }
    FBX_BLOCK_SYNC();
}
// ---- transposed Pauli coefficients Rt -> Choi block (Mw = Vs as scratch)
__device__ Blk pauli_to_choi(Lds& L, int t) {
    t = opaque(t);
    FBX_BLOCK_SYNC();
    for (int idx = t; idx < D * D; idx += NT) {
        const int i = idx % D, j = idx / D;
        int row, col;
        pauli_coeff_position<NQ>(i, j, row, col);
        cplx v; v.re = L.Rt[idx] * d; v.im = 0.0;
        L.Mw[row * LD + col] = v;
    }
    FBX_BLOCK_SYNC();
#pragma unroll
    for (int s = 0; s < NQ; ++s) { pauli_site_stage<NQ, true, LD>(L.Mw, t, 2 * NQ + s, s, +1.0); FBX_BLOCK_SYNC(); }
#pragma unroll
    for (int s = 0; s < NQ; ++s) { pauli_site_stage<NQ, true, LD>(L.Mw, t, 2 * NQ + NQ + s, NQ + s, -1.0); FBX_BLOCK_SYNC(); }
    const Blk out = blk_load<D, LD>(L.Mw, t);
    FBX_BLOCK_SYNC();
    return out;
}
// ---- T[s][i] = sum_j R[i][j] C[j][s]: the dense basis-change GEMM of the 3-qubit path
// ([S x 64] = C^T [S x 64] . R^T [64 x 64]) on the fp64 matrix cores.  v_mfma_f64_16x16x4_f64:
// lane l feeds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; its four accumulators are
// D[row = (l >> 4) + 4 r][col = l & 15].  B = Rt is already [k][n] row-major in LDS; A = C^T comes
// from L2 (C is [64][S]).  16 waves share the ceil(S/16) x 4 output tiles.
typedef double v4d __attribute__((ext_vector_type(4)));
__device__ void predict_table(const DesignDev& des, Lds& L, int t) {
    const int S = des.S;
    t = opaque(t);
    const int lane = t & 63, wave = t >> 6;
    const int mtiles = (S + 15) / 16;
    FBX_BLOCK_SYNC();
    for (int tile = wave; tile < mtiles * 4; tile += NT / 64) {
        const int ms = tile / 4, ni = tile % 4;
        const int srow = ms * 16 + (lane & 15);
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int kk = 0; kk < D / 4; ++kk) {
            const int k = 4 * kk + (lane >> 4);
            const double a = srow < S ? des.C[k * S + srow] : 0.0;
            const double b = L.Rt[k * D + ni * 16 + (lane & 15)];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int srw = ms * 16 + (lane >> 4) + 4 * r;
            if (srw < S) L.T[srw * D + ni * 16 + (lane & 15)] = acc[r];
        }
    }
    FBX_BLOCK_SYNC();
}
// ---- Rt[j][i] = -(1/d^2) sum_s W[i][s] C[j][s]  ([64 x 64] = W [64 x S] . C^T [S x 64]), one
// 16 x 16 output tile per wave; W from LDS, C from L2.  S is padded with zero terms to a multiple of 4.
__device__ void gradient_coefficients(const DesignDev& des, Lds& L, const double* W, int t) {
    const int S = des.S;
    t = opaque(t);
    const int lane = t & 63, wave = t >> 6;
    const int mi = wave / 4, nj = wave % 4;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < S; k0 += 4) {
        const int k = k0 + (lane >> 4);
        const double a = k < S ? W[(mi * 16 + (lane & 15)) * S + k] : 0.0;
        const double b = k < S ? des.C[(nj * 16 + (lane & 15)) * S + k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    FBX_BLOCK_SYNC();                                   // Rt overlays the partial arrays read above
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = mi * 16 + (lane >> 4) + 4 * r, j = nj * 16 + (lane & 15);
        L.Rt[j * D + i] = -acc[r] / (double)(d * d);
    }
    FBX_BLOCK_SYNC();
}

// ---- the two outcome probabilities of setting g from the prediction table: (T[s][0] +- coef T[s][p]) / (2 d^2)
__device__ __forceinline__ void setting_probs(const DesignDev& des, const Lds& L, int g, double& pp, double& pm) {
    const uint32_t w = des.sp[g];
    const int s = w >> 16, p = w & 0xffff;
    const double cf = des.unit_coefs ? 1.0 : des.coef[g];
    const double tr = L.T[s * D], ex = cf * L.T[s * D + p];
    pp = (tr + ex) * (0.5 / (double)(d * d)); pm = (tr - ex) * (0.5 / (double)(d * d));
}

// A pass over the outcome slots of a thread.  Up to four slots the per-slot arrays are register-resident and need static indices: unrolled.
// Beyond that they do not fit the 128 registers of a thread and live in scratch anyway: a loop -- same terms in the same order.
template <int MAXJ, class F>
__device__ __forceinline__ void for_each_slot(F&& f) {
    if constexpr (MAXJ <= 4) {
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) f(j);
    } else {
#pragma unroll 1
        for (int j = 0; j < MAXJ; ++j) f(j);
    }
}

// ---- the gradient weights (tomography.py:617-633) W[i][s] = sum over the settings of state s, in the place of the prediction table
// (fully consumed by then); returns W for gradient_coefficients.  Thread t owns the settings [t nslots, (t + 1) nslots) of the
// state-grouped list and `eta(j, ep, em)` yields eta = n / clip(p) of its slot j.  `nslots` is a Slots<MAXJ> where the count is
// a compile-time constant (the pass is unrolled: eta reads register arrays) or an int.
// Threads own CONTIGUOUS runs of the settings, so the identity row W[0][s] (one term per setting of the state) is reduced
// deterministically: a run that lies inside one thread is written directly, the first / last run of every thread goes to a
// partial array that one thread per state adds up in thread order.  The W[p][s] cells receive one term each (LDS atomics only
// matter for designs that repeat a setting).
template <int N> struct Slots { static constexpr int value = N; constexpr operator int() const { return N; } };
template <class NS, class Eta>
__device__ __forceinline__ double* gradient_weights(const DesignDev& des, Lds& L, int t, NS nslots, Eta&& eta) {
    const int m = des.m, S = des.S, MJ = nslots;
    FBX_BLOCK_SYNC();                              // T fully consumed
    double* W = L.T;
    double* pfirst = L.Rt + 768;                  // overlays R (dead here), past the small scratch
    double* plast = pfirst + NT;
    int* sfirst = (int*)(plast + NT);
    int* slast = sfirst + NT;
    for (int idx = t; idx < D * S; idx += NT) W[idx] = 0.0;
    sfirst[t] = -1; slast[t] = -1; pfirst[t] = 0.0; plast[t] = 0.0;
    FBX_BLOCK_SYNC();
    {
        int run_state = -1; double run = 0.0; bool first_done = false;
        auto slot = [&](int j) __attribute__((always_inline)) {
            const int g = t * MJ + j;
            if (g < m) {
                const uint32_t w = des.sp[g];
                const int s = w >> 16, p = w & 0xffff;
                const double cf = des.unit_coefs ? 1.0 : des.coef[g];
                double ep, em;
                eta(j, ep, em);
                atomicAdd(&W[p * S + s], cf * 0.5 * (ep - em));
                if (s != run_state) {
                    if (run_state >= 0) {                      // flush the finished run
                        if (!first_done) { pfirst[t] = run; sfirst[t] = run_state; first_done = true; }
                        else atomicAdd(&W[run_state], run);    // interior run: sole contributor
                    }
                    run_state = s; run = 0.0;
                }
                run += 0.5 * (ep + em);
            }
        };
        if constexpr (std::is_same<NS, int>::value) {
            for (int j = 0; j < MJ; ++j) slot(j);
        } else {
#pragma unroll
            for (int j = 0; j < NS::value; ++j) slot(j);
        }
        if (run_state >= 0) {
            if (!first_done) { pfirst[t] = run; sfirst[t] = run_state; }
            else { plast[t] = run; slast[t] = run_state; }
        }
    }
    FBX_BLOCK_SYNC();
    for (int s = t; s < S; s += NT) {
        const int g0 = des.sptr[s], g1 = des.sptr[s + 1];
        if (g1 > g0) {
            double acc = 0.0;
            for (int tt = g0 / MJ; tt <= (g1 - 1) / MJ; ++tt) {
                if (sfirst[tt] == s) acc += pfirst[tt];
                if (slast[tt] == s) acc += plast[tt];
            }
            W[s] += acc;
        }
    }
    FBX_BLOCK_SYNC();
    return W;
}

// ---- the thread's 2 x 2 block of item `item` of a batch of row-major Choi matrices in global memory ([B][64][64] complex as pairs of doubles)
// (opaque: the block's indices are worked out at the access, not kept in registers across the kernel -- 16 B of scratch in pgdb3_kernel<4>)
__device__ __forceinline__ Blk choi_load(const double* g, long long item, int t) { return blk_load<D, D>((const cplx*)g + item * D * D, opaque(t)); }
__device__ __forceinline__ void choi_store(double* g, long long item, int t, const Blk& v) { blk_store<D, D>((cplx*)g + item * D * D, opaque(t), v); }
}  // namespace p3
}  // namespace fbx
