// fbx_convert.hip -- fbx_convert: batched changes of representation of a channel (Kraus operators, Choi matrix,
// superoperator, Pauli-Liouville matrix, chi matrix) for 1-5 qubits, and fbx_convert_general for the basis-free ones in any
// dimension.  Three primitives and a walk (fbx_superop_prims.hpp).
//
// Reference functions: forest/benchmarking/operator_tools/superoperator_transformations.py:82-371
#include "fbx_superop_prims.hpp"
#include "fbx_eigh64.hpp"
#include <cstdlib>
#include <algorithm>

namespace fbx {

// Is an entry that a route into chi reads not finite?  From a Choi matrix (`lower`) the route reads what the reference's eigh
// reads, the real part of the diagonal and the strict lower triangle; from a superoperator or a Pauli-Liouville matrix every
// entry (the walk to the Choi matrix may carry it anywhere).  This thread's share of a D x D matrix, NT threads.
template <int D, int LD, int NT>
__device__ __forceinline__ int nonfinite_share(const cplx* a, bool lower, int t) {
    int bad = 0;
    for (int idx = t; idx < D * D; idx += NT) {
        const int r = idx / D, c = idx % D;
        const cplx v = a[r * LD + c];
        if (!lower || r > c) bad |= !(isfinite(v.re) && isfinite(v.im));
        else if (r == c) bad |= !isfinite(v.re);
    }
    return bad;
}
__device__ __forceinline__ void fill_nan(double* __restrict__ o, int n, int t, int nt) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int idx = t; idx < n; idx += nt) o[idx] = nan;
}

// ---------------------------------------------------------------------------------------------
// The walk: chi -> choi <-> superop <-> pauli-liouville, choi -> chi, entered from Kraus operators (straight to the Choi matrix
// or the superoperator, whichever is nearer the target) or from a matrix.  `cur` / `nxt` are the ping-pong matrices of the
// item, `kb` stages its Kraus operators.  Ops is the size class: NQ, NT threads, leading dimension LD, to_pauli / from_pauli
// (nxt = the transform of cur, which may be destroyed) and, where ABS says so, abs_choi: nxt = |cur| for a Choi matrix on its
// way into chi that is not known to be PSD -- the reference goes through choi2kraus there (eigh, tol 1e-9).
// convert3_kernel below spells the same walk out: called from here its 64 x 64 Jacobi came out 2 % slower (docs/history/experiments.md).
// ---------------------------------------------------------------------------------------------
template <class Ops>
__device__ __forceinline__ void convert_walk(Ops op, int from, int to, const double* __restrict__ in, int K, double* __restrict__ out,
                                             cplx* cur, cplx* nxt, cplx* kb) {
    constexpr int NQ = Ops::NQ, NT = Ops::NT, LD = Ops::LD, d = 1 << NQ, D = d * d;
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    auto swap = [&]() { cplx* q = cur; cur = nxt; nxt = q; __syncthreads(); };
    const double inv_d = 1.0 / d;
    int rep = from;
    if (from == FBX_REP_KRAUS) {
        const bool sup = (to == FBX_REP_SUPEROP || to == FBX_REP_PAULI_LIOUVILLE);
        kraus_to<NQ, NT, LD>(in + item * (long long)K * D * 2, K, sup, cur, kb, t);
        __syncthreads();
        rep = sup ? FBX_REP_SUPEROP : FBX_REP_CHOI;
    } else {
        load_matrix<NQ, NT, LD>(in + item * (long long)D * D * 2, cur, t);
        __syncthreads();
        if constexpr (Ops::ABS) {
            // A non-finite item on its way into chi gives NaN in every entry (include/fbx.h): the eigensolver's stopping test is
            // false on a NaN or an infinite norm, so it would hand back the diagonal with the identity, and the cut below turns
            // a NaN eigenvalue into 0 -- a finite chi matrix of something else.  Nothing is converted.
            if (to == FBX_REP_CHI && op.nonfinite(cur, from == FBX_REP_CHOI, t)) {
                fill_nan(out + item * (long long)D * D * 2, 2 * D * D, t, NT);
                return;
            }
        }
    }
    const bool kraus_chi = (from == FBX_REP_KRAUS && to == FBX_REP_CHI);    // the Choi matrix of a Kraus set is PSD: |C| = C
    while (rep != to) {
        if (rep == FBX_REP_CHI) {                       // chi2choi: p2c chi p2c^H
            op.from_pauli(cur, nxt, 1.0, t); swap(); rep = FBX_REP_CHOI;
        } else if (rep == FBX_REP_CHOI) {
            if (to == FBX_REP_CHI) {
                if constexpr (Ops::ABS) {
                    if (!kraus_chi) { op.abs_choi(cur, nxt, t); swap(); }
                }
                op.to_pauli(cur, nxt, inv_d * inv_d, t); swap(); rep = FBX_REP_CHI;
            } else {
                reshuffle<NQ, NT, LD>(cur, nxt, t); swap(); rep = FBX_REP_SUPEROP;
            }
        } else if (rep == FBX_REP_SUPEROP) {
            if (to == FBX_REP_PAULI_LIOUVILLE) {
                op.to_pauli(cur, nxt, inv_d, t); swap(); rep = FBX_REP_PAULI_LIOUVILLE;
            } else {
                reshuffle<NQ, NT, LD>(cur, nxt, t); swap(); rep = FBX_REP_CHOI;
            }
        } else {                                        // pauli-liouville -> superop
            op.from_pauli(cur, nxt, inv_d, t); swap(); rep = FBX_REP_SUPEROP;
        }
    }
    store_matrix<NQ, NT, LD>(cur, out + item * (long long)D * D * 2, t);
}

// matrices in LDS: the site-factored transforms
template <int NQ_, int NT_, int LD_>
struct WalkLds {
    static constexpr int NQ = NQ_, NT = NT_, LD = LD_;
    __device__ __forceinline__ void to_pauli(cplx* a, cplx* b, double s, int t) const { to_pauli_sites<NQ, NT, LD>(a, b, s, t); }
    __device__ __forceinline__ void from_pauli(const cplx* a, cplx* b, double s, int t) const { from_pauli_sites<NQ, NT, LD>(a, b, s, t); }
};

// ---- one and two qubits: one wavefront per item.  EIGH = false: the conversions that never pass through choi2kraus need no
// eigensolver arrays -- 10 KB instead of 23 KB of LDS per wavefront (2 qubits), i.e. 15 instead of 6 wavefronts per CU on a
// kernel that only waits for HBM.
template <int NQ, bool EIGH>
struct WalkSmall : WalkLds<NQ, 64, (1 << (2 * NQ)) + 1> {
    static constexpr bool ABS = EIGH;
    ChoiLds<NQ> L;
    __device__ __forceinline__ void abs_choi(const cplx* a, cplx* b, int t) { abs_via_eigh<NQ>(a, b, L, 1e-9, t); }
    __device__ __forceinline__ bool nonfinite(const cplx* a, bool lower, int t) const {        // one wavefront per item
        constexpr int D = 1 << (2 * NQ);
        return __ballot(nonfinite_share<D, D + 1, 64>(a, lower, t)) != 0;
    }
};
template <int NQ, bool EIGH = true>
__global__ void __launch_bounds__(64)
convert_kernel(int from, int to, long long B, const double* __restrict__ in, int K, double* __restrict__ out) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* p = smem;
    WalkSmall<NQ, EIGH> op;
    if constexpr (EIGH) {
        op.L.carve(p);
        p = smem + ((ChoiLds<NQ>::bytes() + 15) & ~(size_t)15);  // (no pointer -> integer -> pointer: keeps the LDS address space)
    }
    cplx* A = (cplx*)p;
    cplx* Bm = A + D * LD;
    convert_walk(op, from, to, in, K, out, A, Bm, Bm + D * LD);
}

template <int NQ>
static int launch_convert(int from, int to, int64_t B, const double* in, int K, double* out) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1;
    const bool eigh = to == FBX_REP_CHI && from != FBX_REP_KRAUS;
    const size_t lds = (eigh ? ChoiLds<NQ>::bytes() + 16 : 0) + sizeof(cplx) * (2 * D * LD + (size_t)(K > 0 ? K : 1) * D);
    if (lds > 160 * 1024) { set_error("fbx_convert: too many Kraus operators for LDS staging"); return FBX_ERR_UNSUPPORTED; }
    return launch_lds(eigh ? convert_kernel<NQ, true> : convert_kernel<NQ, false>, dim3((unsigned)B), dim3(64), lds, from, to, B, in, K, out);
}

// ---- three qubits: 64 x 64 matrices, one 1024-thread workgroup per item.  The two ping-pong
// matrices (row-major, LD = 64) ARE the Jacobi work / eigenvector arrays of the |C| step: every
// hand-over goes through registers, so the aliasing is safe.  LDS: [A 64K | B 64K | Kraus + scratch 32K].
__global__ void __launch_bounds__(1024)
convert3_kernel(int from, int to, long long B, const double* __restrict__ in, int K, double* __restrict__ out) {
    constexpr int NQ = 3, d = 8, D = 64, LD = 64, NT = 1024, NB = 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* A = (cplx*)smem;
    cplx* Bm = A + D * D;
    double* lam = (double*)(Bm + D * D);
    double* red = lam + D;
    cplx* kb = (cplx*)(red + 64);
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    cplx* cur = A; cplx* nxt = Bm;
    auto swap = [&]() { cplx* q = cur; cur = nxt; nxt = q; __syncthreads(); };
    const double inv_d = 1.0 / d;

    int rep = from;
    if (from == FBX_REP_KRAUS) {
        const bool sup = (to == FBX_REP_SUPEROP || to == FBX_REP_PAULI_LIOUVILLE);
        kraus_to<NQ, NT, LD>(in + item * (long long)K * D * 2, K, sup, cur, kb, t);
        __syncthreads();
        rep = sup ? FBX_REP_SUPEROP : FBX_REP_CHOI;
    } else {
        load_matrix<NQ, NT, LD>(in + item * (long long)D * D * 2, cur, t);
        __syncthreads();
        if (to == FBX_REP_CHI) {        // a non-finite item on its way into chi: NaN in every entry (convert_walk)
            const bool wave_bad = __ballot(nonfinite_share<D, LD, NT>(cur, from == FBX_REP_CHOI, t)) != 0;
            if ((t & 63) == 0) red[t >> 6] = wave_bad ? 1.0 : 0.0;
            __syncthreads();
            double any = 0.0;
            for (int w = 0; w < NT / 64; ++w) any += red[w];
            __syncthreads();            // red is the Jacobi's scratch next
            if (any != 0.0) {
                fill_nan(out + item * (long long)D * D * 2, 2 * D * D, t, NT);
                return;
            }
        }
    }
    const bool kraus_chi = (from == FBX_REP_KRAUS && to == FBX_REP_CHI);
    while (rep != to) {
        if (rep == FBX_REP_CHI) {
            from_pauli_sites<NQ, NT, LD>(cur, nxt, 1.0, t); swap(); rep = FBX_REP_CHOI;
        } else if (rep == FBX_REP_CHOI) {
            if (to == FBX_REP_CHI) {
                if (!kraus_chi) {       // |C| = sum |lambda| v v^H, as choi2kraus -> kraus2chi (tol 1e-9)
                    const int I = t / NB, J = t % NB;
                    Blk h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {       // numpy eigh reads the lower triangle
                        const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
                        if (r > c) { const cplx v = cur[r * LD + c]; h.re[e] = v.re; h.im[e] = v.im; }
                        else if (r < c) { const cplx v = cur[c * LD + r]; h.re[e] = v.re; h.im[e] = -v.im; }
                        else { h.re[e] = cur[r * LD + c].re; h.im[e] = 0.0; }
                    }
                    __syncthreads();
                    sys_store<D>(A, t, h);
                    __syncthreads();
                    jacobi_eigh_block<D, NT>(A, Bm, t, true, red);
                    if (t < D) {
                        const double l = fabs(A[sys_index<D>(t, t)].re);
                        lam[t] = l > 1e-9 ? l : 0.0;
                    }
                    __syncthreads();
                    const Blk a = reconstruct_blk<D>(Bm, lam, t);
                    __syncthreads();
                    blk_store<D, LD>(nxt, t, a);
                    swap();
                }
                to_pauli_sites<NQ, NT, LD>(cur, nxt, inv_d * inv_d, t); swap(); rep = FBX_REP_CHI;
            } else {
                reshuffle<NQ, NT, LD>(cur, nxt, t); swap(); rep = FBX_REP_SUPEROP;
            }
        } else if (rep == FBX_REP_SUPEROP) {
            if (to == FBX_REP_PAULI_LIOUVILLE) {
                to_pauli_sites<NQ, NT, LD>(cur, nxt, inv_d, t); swap(); rep = FBX_REP_PAULI_LIOUVILLE;
            } else {
                reshuffle<NQ, NT, LD>(cur, nxt, t); swap(); rep = FBX_REP_CHOI;
            }
        } else {
            from_pauli_sites<NQ, NT, LD>(cur, nxt, inv_d, t); swap(); rep = FBX_REP_SUPEROP;
        }
    }
    store_matrix<NQ, NT, LD>(cur, out + item * (long long)D * D * 2, t);
}

// ---- 4 and 5 qubits: the `_big` forms of the transforms on work matrices in HBM, one 1024-thread workgroup per item.  Into chi
// only from a PSD Choi matrix (checked on the host), so there is no |C| step.
template <int NQ_>
struct WalkBig {
    static constexpr int NQ = NQ_, NT = 1024, LD = 1 << (2 * NQ_);
    static constexpr bool ABS = false;
    __device__ __forceinline__ void to_pauli(cplx* a, cplx* b, double s, int t) const { to_pauli_big<NQ, NT>(a, b, s, t); }
    __device__ __forceinline__ void from_pauli(const cplx* a, cplx* b, double s, int t) const { from_pauli_big<NQ, NT>(a, b, s, t); }
};
template <int NQ>
__global__ void __launch_bounds__(1024)
convert_big_kernel(int from, int to, long long B, const double* __restrict__ in, int K, double* __restrict__ out,
                   cplx* __restrict__ work) {
    constexpr size_t D = (size_t)1 << (2 * NQ);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* cur = work + (size_t)blockIdx.x * 2 * D * D;
    convert_walk(WalkBig<NQ>(), from, to, in, K, out, cur, cur + D * D, (cplx*)smem);     // LDS: the Kraus operators of the item
}

template <int NQ>
static int convert_into_chi_big(int from, int64_t B, const double* in, double* out);

// psd_choi: the caller vouches that the Choi matrix on the way into chi is positive semidefinite (|C| = C): the kernel's
// linear basis change then IS choi2chi (it is what kraus -> chi runs)
template <int NQ>
static int launch_convert_big(int from, int to, int64_t B, const double* in, int K, double* out, bool psd_choi = false) {
    constexpr size_t d = (size_t)1 << NQ, D = d * d;
    if (to == FBX_REP_CHI && from != FBX_REP_KRAUS && !(psd_choi && from == FBX_REP_CHOI))
        return convert_into_chi_big<NQ>(from, B, in, out);
    const size_t lds = sizeof(cplx) * (size_t)(K > 0 ? K : 1) * D;
    if (lds > 160 * 1024) { set_error("fbx_convert: too many Kraus operators for LDS staging"); return FBX_ERR_UNSUPPORTED; }
    const size_t per_item = 2 * D * D * sizeof(cplx);
    const int64_t chunk = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)512 << 20) / per_item));
    void* w = nullptr;
    { const int rc = workspace(WS_CONVERT, per_item * (size_t)chunk, &w); if (rc) return rc; }
    const size_t in_item = (from == FBX_REP_KRAUS ? (size_t)K * D : D * D) * 2;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = B - b0 < chunk ? B - b0 : chunk;
        FBX_TRY(launch_lds(convert_big_kernel<NQ>, dim3((unsigned)nb), dim3(1024), lds, from, to, nb, in + b0 * in_item, K,
                           out + b0 * D * D * 2, (cplx*)w));
    }
    return FBX_OK;
}

// Into chi from a Choi / superoperator / Pauli-Liouville matrix for 4 and 5 qubits (round 5).  The reference goes through
// choi2kraus -> kraus2chi (superoperator_transformations.py:241-250, 291-298, 339-348): chi of |C| = sum |lambda_i| v_i v_i^H
// over the eigenpairs with |lambda_i| > 1e-9.  Composed from the library's own primitives, everything resident: the walk to
// the Choi matrix, fbx_eigh_dev (the HBM-resident Jacobi: 25 ms per 256 x 256 matrix, 0.8 s per 1024 x 1024), |lambda| with
// the reference's cut, fbx_matmul_dev for V diag(|lambda|) V^H, and the kernel's linear basis change on that PSD matrix.
__global__ void __launch_bounds__(256) abs_cut_kernel(double* __restrict__ w, long long n, double tol) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const double a = fabs(w[i]); w[i] = a <= tol ? 0.0 : a; }        // (a NaN eigenvalue stays one)
}
// A superoperator or a Pauli-Liouville matrix with a non-finite entry gives NaN in every entry of its chi matrix (include/fbx.h),
// wherever the walk to the Choi matrix carried that entry -- above the diagonal fbx_eigh would not read it.  One workgroup per
// item: a NaN into the first diagonal entry of the item's Choi matrix, and fbx_eigh's own contract does the rest.
__global__ void __launch_bounds__(256) poison_nonfinite_kernel(const double* __restrict__ src, long long n_per_item, double* __restrict__ choi) {
    __shared__ int any;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    const double* s = src + (long long)blockIdx.x * n_per_item;
    int bad = 0;
    for (long long i = threadIdx.x; i < n_per_item; i += 256) bad |= !isfinite(s[i]);
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(&any, 1);
    __syncthreads();
    if (any && threadIdx.x == 0) choi[(long long)blockIdx.x * n_per_item] = __longlong_as_double(0x7ff8000000000000LL);
}
template <int NQ>
static int convert_into_chi_big(int from, int64_t B, const double* in, double* out) {
    constexpr size_t D = (size_t)1 << (2 * NQ);
    const int64_t chunk = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)256 << 20) / (D * D * sizeof(cplx))));
    DevBuf c, v, w;
    { int rc; if ((rc = c.alloc(D * D * sizeof(cplx) * chunk)) || (rc = v.alloc(D * D * sizeof(cplx) * chunk)) || (rc = w.alloc(D * sizeof(double) * chunk))) return rc; }
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = B - b0 < chunk ? B - b0 : chunk;
        const double* choi = in + (size_t)b0 * D * D * 2;
        if (from != FBX_REP_CHOI) {
            const int rc = launch_convert_big<NQ>(from, FBX_REP_CHOI, nb, choi, 0, c.as<double>()); if (rc) return rc;
            FBX_TRY(launch_lds(poison_nonfinite_kernel, dim3((unsigned)nb), dim3(256), 0, choi, (long long)(D * D * 2), c.as<double>()));
            choi = c.as<double>();
        }
        { const int rc = fbx_eigh_dev((int)D, nb, choi, w.as<double>(), v.as<double>()); if (rc) return rc; }
        FBX_TRY(launch_lds(abs_cut_kernel, dim3((unsigned)((nb * D + 255) / 256)), dim3(256), 0, w.as<double>(), nb * D, 1e-9));
        { const int rc = fbx_matmul_dev((int)D, nb, v.as<double>(), 0, w.as<double>(), v.as<double>(), 1, c.as<double>()); if (rc) return rc; }
        { const int rc = launch_convert_big<NQ>(FBX_REP_CHOI, FBX_REP_CHI, nb, c.as<double>(), 0, out + (size_t)b0 * D * D * 2, true); if (rc) return rc; }
    }
    return FBX_OK;
}

// ---------------------------------------------------------------------------------------------
// Any Hilbert-space dimension (qutrits, ...): the conversions that involve no operator basis --
// kraus2superop, kraus2choi, superop2choi, choi2superop (superoperator_transformations.py:100-182,267-277,351-361).
// One thread per output entry, straight from and to HBM.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
convert_general_kernel(int from, int to, int d, long long B, const double* __restrict__ in, int K, double* __restrict__ out) {
    const long long D = (long long)d * d, DD = D * D;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * DD) return;
    const long long item = gid / DD;
    const int row = (int)((gid % DD) / D), col = (int)(gid % D);
    double re = 0.0, im = 0.0;
    if (from == FBX_REP_KRAUS) {
        const cplx* k = (const cplx*)(in + item * K * D * 2);
        const cplx o = to == FBX_REP_SUPEROP ? kraus_superop_entry(k, K, d, row, col) : kraus_choi_entry(k, K, d, row, col);
        re = o.re; im = o.im;
    } else {        // the reshuffle, its own inverse: out[(p,q)][(r,s)] = in[(s,q)][(r,p)]
        const int p = row / d, q = row % d, r = col / d, s = col % d;
        const double* src = in + (item * DD + (long long)(s * d + q) * D + r * d + p) * 2;
        re = src[0]; im = src[1];
    }
    out[2 * gid] = re; out[2 * gid + 1] = im;
}

// ---- 3 qubits, the routes between Choi / superoperator / Pauli-Liouville: ONE 64 KB matrix in LDS instead of two,
// so that two workgroups share a CU and the HBM loads / stores of one overlap the butterfly stages of the other.
// The reshuffle rides on the global load (forward) or store (backward) as an index permutation, the bit-permuting
// copy of the site-factored transform on the other side.  ROUTE: 0 choi->PL, 1 PL->choi, 2 superop->PL, 3 PL->superop,
// 4 choi<->superop (pure permutation, no LDS).
template <int ROUTE>
__global__ void __launch_bounds__(1024)
convert3_fast_kernel(long long B, const double* __restrict__ in, double* __restrict__ out) {
    constexpr int NQ = 3, d = 8, D = 64, LD = 64, NT = 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* X = (cplx*)smem;
    const int t = threadIdx.x;
    const double inv_d = 1.0 / d;
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        const double* src = in + item * (long long)D * D * 2;
        double* dst = out + item * (long long)D * D * 2;
        auto shuffled = [](int idx) {                      // entry (p,q),(r,s) <- entry (s,q),(r,p): its own inverse
            const int row = idx / D, col = idx % D;
            const int p = row / d, q = row % d, r = col / d, s_ = col % d;
            return (s_ * d + q) * D + r * d + p;
        };
        if (ROUTE == 4) {
            for (int idx = t; idx < D * D; idx += NT) { const int j = shuffled(idx); dst[2 * idx] = src[2 * j]; dst[2 * idx + 1] = src[2 * j + 1]; }
            continue;
        }
        __syncthreads();                                   // the previous item's readers of X are done
        if (ROUTE == 0 || ROUTE == 2) {                    // -> Pauli-Liouville: (reshuffled) load, stages, permuted scaled store
            for (int idx = t; idx < D * D; idx += NT) {
                const int j = ROUTE == 0 ? shuffled(idx) : idx;
                cplx v; v.re = src[2 * j]; v.im = src[2 * j + 1];
                X[idx] = v;
            }
            __syncthreads();
            site_stages<NQ, false, NT, LD>(X, t);
            for (int idx = t; idx < D * D; idx += NT) {
                const cplx v = X[site_index<NQ>(idx / D) * LD + site_index<NQ>(idx % D)];
                dst[2 * idx] = v.re * inv_d; dst[2 * idx + 1] = v.im * inv_d;
            }
        } else {                                           // Pauli-Liouville ->: permuted scaled load, inverse stages, (reshuffled) store
            const double sc = inv_d * D;
            for (int idx = t; idx < D * D; idx += NT) {
                cplx v; v.re = src[2 * idx] * sc; v.im = src[2 * idx + 1] * sc;
                X[site_index<NQ>(idx / D) * LD + site_index<NQ>(idx % D)] = v;
            }
            __syncthreads();
            site_stages<NQ, true, NT, LD>(X, t);
            for (int idx = t; idx < D * D; idx += NT) {
                const cplx v = X[ROUTE == 1 ? shuffled(idx) : idx];
                dst[2 * idx] = v.re; dst[2 * idx + 1] = v.im;
            }
        }
    }
}
template <int ROUTE>
static int launch_convert3_fast(int64_t B, const double* in, double* out) {
    const size_t lds = ROUTE == 4 ? 0 : sizeof(cplx) * 64 * 64;
    return launch_lds(convert3_fast_kernel<ROUTE>, dim3((unsigned)std::min<int64_t>(B, 512 * 8)), dim3(1024), lds, B, in, out);
}

// The pairwise 3-qubit routes between Choi / superoperator / Pauli-Liouville in the same three register passes (round 4): 64 KB
// in, 64 KB out per item, 256-thread workgroups, one swizzled 64 KB tile.  ROUTE as convert3_fast_kernel: 0 choi->PL,
// 2 superop->PL, 3 PL->superop (route 1, PL->choi, keeps the one-stage-per-pass kernel: its result leaves reshuffled, i.e. as
// 16-byte pieces 8 KB apart from any register layout -- measured 7 x slower than a shuffle on the LDS side).  P1 loads the tile
// straight from HBM into its registers (route 0: reshuffled, scattered 16-byte reads that L2 absorbs; route 3: the Pauli index
// permuted to the site order, 256-byte runs), P3 stores whole rows; route 3 runs the inverse butterflies in the same order
// (the stages commute).
template <int ROUTE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
convert3_regs_kernel(long long B, const double* __restrict__ in, double* __restrict__ out) {
    static_assert(ROUTE == 0 || ROUTE == 2 || ROUTE == 3, "route 1 stays with convert3_fast_kernel");
    constexpr int d = 8, D = 64;
    constexpr bool TO_PL = ROUTE != 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* X = (cplx*)smem;
    const S3Tile tile(threadIdx.x);
    // Pauli label of a tile row / column (inverse of site_index: label bit 2t = index bit t, 2t + 1 = index bit 3 + t)
    auto label = [](int x) { return (x & 1) | ((x >> 3) & 1) << 1 | ((x >> 1) & 1) << 2 | ((x >> 4) & 1) << 3 | ((x >> 2) & 1) << 4 | ((x >> 5) & 1) << 5; };
    // HBM index the tile entry (row, col) is loaded from
    auto load_index = [&](int row, int col) {
        if (ROUTE == 2) return row * D + col;
        if (ROUTE == 3) return label(row) * D + label(col);
        const int p = row / d, q = row % d, r = col / d, s_ = col % d;       // route 0: entry (p,q),(r,s) <- Choi entry (s,q),(r,p)
        return (s_ * d + q) * D + r * d + p;
    };
    const double inv_d = 1.0 / d;
    const double sc_in = TO_PL ? 1.0 : inv_d * D, sc_out = TO_PL ? inv_d : 1.0;
    auto sites = [](cplx (&x)[16], double y1, double y2) { two_sites<!TO_PL>(x, y1, y2); };
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        const double* src = in + item * (long long)D * D * 2;
        double* dst = out + item * (long long)D * D * 2;
        cplx x[16];
        __syncthreads();                                   // the previous item's readers of X are done
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double2 v = *reinterpret_cast<const double2*>(src + 2 * load_index(tile.row1 | tile.reg_row1(r), tile.col1 | tile.reg_col1(r)));
            x[r].re = v.x * sc_in; x[r].im = v.y * sc_in;
        }
        sites(x, -1.0, +1.0);                              // row site 2 (-i), column site 2 (+i)
        tile.store1(X, x);
        __syncthreads();
        tile.passes23(X, sites, [&](int r, const cplx& xr) {
            double2 v; v.x = xr.re * sc_out; v.y = xr.im * sc_out;
            // towards PL: Pauli row 16 w + r, column = lane; route 3: tile row / column as they are
            const long long o = TO_PL ? ((long long)(tile.krow + r) * D + tile.lcol) : ((long long)(tile.row3 | tile.reg_row3(r)) * D + tile.col3);
            FBX_STREAM_STORE(reinterpret_cast<double2*>(dst + 2 * o), v);
        });
    }
}
template <int ROUTE>
static int launch_convert3_regs(int64_t B, const double* in, double* out) {
    const size_t lds = sizeof(cplx) * 64 * 64;
    return launch_lds(convert3_regs_kernel<ROUTE>, dim3((unsigned)std::min(B, S3_GRID)), dim3(256), lds, B, in, out);
}

static int launch_convert3(int from, int to, int64_t B, const double* in, int K, double* out) {
    constexpr size_t D = 64;
    const char* v1s = getenv("FBX_CONVERT3_V1");            // 1 = the one-stage-per-pass kernels (A/B, tests)
    const bool v1 = v1s && atoi(v1s) != 0;
    // from Kraus operators: the sweep kernel with one output (operators read once, the result written once, coalesced)
    if (!v1 && from == FBX_REP_KRAUS && K >= 1 && K <= 31 && (to == FBX_REP_CHOI || to == FBX_REP_PAULI_LIOUVILLE || to == FBX_REP_CHI))
        return launch_sweep3_regs(B, K, in, nullptr, to == FBX_REP_CHOI ? out : nullptr, to == FBX_REP_PAULI_LIOUVILLE ? out : nullptr,
                                  to == FBX_REP_CHI ? out : nullptr, nullptr);
    if (from == FBX_REP_CHOI && to == FBX_REP_PAULI_LIOUVILLE) return v1 ? launch_convert3_fast<0>(B, in, out) : launch_convert3_regs<0>(B, in, out);
    if (from == FBX_REP_PAULI_LIOUVILLE && to == FBX_REP_CHOI) return launch_convert3_fast<1>(B, in, out);
    if (from == FBX_REP_SUPEROP && to == FBX_REP_PAULI_LIOUVILLE) return v1 ? launch_convert3_fast<2>(B, in, out) : launch_convert3_regs<2>(B, in, out);
    if (from == FBX_REP_PAULI_LIOUVILLE && to == FBX_REP_SUPEROP) return v1 ? launch_convert3_fast<3>(B, in, out) : launch_convert3_regs<3>(B, in, out);
    if ((from == FBX_REP_CHOI && to == FBX_REP_SUPEROP) || (from == FBX_REP_SUPEROP && to == FBX_REP_CHOI)) return launch_convert3_fast<4>(B, in, out);
    const size_t lds = 2 * sizeof(cplx) * D * D + sizeof(double) * 128 + sizeof(cplx) * (size_t)(K > 0 ? K : 1) * D;
    if (lds > 160 * 1024) { set_error("fbx_convert: too many Kraus operators for LDS staging (3 qubits: at most 31)"); return FBX_ERR_UNSUPPORTED; }
    return launch_lds(convert3_kernel, dim3((unsigned)B), dim3(1024), lds, from, to, B, in, K, out);
}

int convert_launch(int n_qubits, int from, int to, int64_t B, const double* in, int K, double* out, bool psd_choi) {
    if (n_qubits == 5) return launch_convert_big<5>(from, to, B, in, K, out, psd_choi);
    if (n_qubits == 4) return launch_convert_big<4>(from, to, B, in, K, out, psd_choi);
    if (n_qubits == 3) return launch_convert3(from, to, B, in, K, out);
    if (n_qubits == 1) return launch_convert<1>(from, to, B, in, K, out);
    return launch_convert<2>(from, to, B, in, K, out);
}

}  // namespace fbx

using namespace fbx;

extern "C" {

static int convert_check(int from_rep, int to_rep, int n_qubits, int64_t B, const void* in, int K, const void* out) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 5, "fbx_convert: n_qubits must be 1..5");
    FBX_REQUIRE(from_rep >= FBX_REP_KRAUS && from_rep <= FBX_REP_CHI, "fbx_convert: bad source representation");
    FBX_REQUIRE(to_rep >= FBX_REP_CHOI && to_rep <= FBX_REP_CHI, "fbx_convert: bad target representation (Kraus output is not offered)");
    FBX_REQUIRE(from_rep != to_rep, "fbx_convert: source and target representation are the same");
    FBX_REQUIRE(B >= 0 && (B == 0 || (in && out)), "fbx_convert: bad batch / NULL buffer");
    FBX_REQUIRE(from_rep != FBX_REP_KRAUS || K >= 1, "fbx_convert: need K >= 1 Kraus operators");
    return FBX_OK;
}

int fbx_convert_dev(int from_rep, int to_rep, int n_qubits, int64_t B, const double* d_in, int K, double* d_out) {
    FBX_TRY(convert_check(from_rep, to_rep, n_qubits, B, d_in, K, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const int rc = convert_launch(n_qubits, from_rep, to_rep, B, d_in, K, d_out);
    // (from a Kraus set the launchers above return FBX_ERR_UNSUPPORTED for exactly one reason: K operators do not fit their LDS staging)
    if (rc != FBX_ERR_UNSUPPORTED || from_rep != FBX_REP_KRAUS) return rc;
    // More Kraus operators than the fused kernels stage in LDS (K x D x 16 B against 160 KiB: 40 operators for 4 qubits, 10 for
    // 5): the Choi matrix from the basis-free kernel, which takes any K (one thread per entry, operators read through L2),
    // then on from there -- the Choi matrix of a Kraus set is PSD, so the way into chi is the linear one.  In chunks of at
    // most 256 MiB of Choi matrices (a 5-qubit item is 16 MiB), like convert_into_chi_big.
    const size_t D = (size_t)1 << (2 * n_qubits), d = (size_t)1 << n_qubits;
    int rc2 = FBX_OK;
    if (to_rep == FBX_REP_CHOI) rc2 = fbx_convert_general_dev(FBX_REP_KRAUS, FBX_REP_CHOI, 1 << n_qubits, B, d_in, K, d_out);
    else {
        const size_t per_item = D * D * sizeof(cplx);
        const int64_t chunk = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)256 << 20) / per_item));
        DevBuf choi;
        FBX_TRY(choi.alloc(per_item * (size_t)chunk));
        for (int64_t b0 = 0; b0 < B && rc2 == FBX_OK; b0 += chunk) {
            const int64_t nb = std::min<int64_t>(chunk, B - b0);
            rc2 = fbx_convert_general_dev(FBX_REP_KRAUS, FBX_REP_CHOI, 1 << n_qubits, nb, d_in + (size_t)b0 * K * d * d * 2, K, choi.as<double>());
            if (rc2 == FBX_OK) rc2 = convert_launch(n_qubits, FBX_REP_CHOI, to_rep, nb, choi.as<double>(), 0, d_out + (size_t)b0 * D * D * 2, true);
        }
    }
    if (rc2 == FBX_OK) set_error("");              // the fused path's "too many Kraus operators" is not this call's outcome
    return rc2;
}

static int convert_general_check(int from_rep, int to_rep, int dim, int64_t B, const void* in, int K, const void* out) {
    FBX_REQUIRE(dim >= 1 && dim <= 256, "fbx_convert_general: dim must be 1..256");
    const bool ok = (from_rep == FBX_REP_KRAUS && (to_rep == FBX_REP_SUPEROP || to_rep == FBX_REP_CHOI)) ||
                    (from_rep == FBX_REP_SUPEROP && to_rep == FBX_REP_CHOI) || (from_rep == FBX_REP_CHOI && to_rep == FBX_REP_SUPEROP);
    FBX_REQUIRE(ok, "fbx_convert_general: only kraus -> superop / choi and superop <-> choi are basis free");
    FBX_REQUIRE(B >= 0 && (B == 0 || (in && out)), "fbx_convert_general: bad batch / NULL buffer");
    FBX_REQUIRE(from_rep != FBX_REP_KRAUS || K >= 1, "fbx_convert_general: need K >= 1 Kraus operators");
    return FBX_OK;
}

int fbx_convert_general_dev(int from_rep, int to_rep, int dim, int64_t B, const double* d_in, int K, double* d_out) {
    FBX_TRY(convert_general_check(from_rep, to_rep, dim, B, d_in, K, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long total = (long long)B * dim * dim * dim * dim;
    return launch_lds(convert_general_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, from_rep, to_rep, dim, B, d_in, K, d_out);
}

int fbx_convert_general(int from_rep, int to_rep, int dim, int64_t B, const double* in, int K, double* out) {
    FBX_TRY(convert_general_check(from_rep, to_rep, dim, B, in, K, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t D = (size_t)dim * dim;
    const size_t n_in = (from_rep == FBX_REP_KRAUS ? (size_t)K * D : D * D) * 2 * B, n_out = D * D * 2 * B;
    HostIO io; double *d_in, *d_out;
    FBX_TRY(io.in(in, n_in, &d_in)); FBX_TRY(io.out(out, n_out, &d_out));
    FBX_TRY(fbx_convert_general_dev(from_rep, to_rep, dim, B, d_in, K, d_out));
    return io.finish();
}

int fbx_convert(int from_rep, int to_rep, int n_qubits, int64_t B, const double* in, int K, double* out) {
    FBX_TRY(convert_check(from_rep, to_rep, n_qubits, B, in, K, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d;
    const size_t n_in = (from_rep == FBX_REP_KRAUS ? (size_t)K * D : D * D) * 2 * B, n_out = D * D * 2 * B;
    HostIO io; double *d_in, *d_out;
    FBX_TRY(io.in(in, n_in, &d_in)); FBX_TRY(io.out(out, n_out, &d_out));
    FBX_TRY(fbx_convert_dev(from_rep, to_rep, n_qubits, B, d_in, K, d_out));
    return io.finish();
}

}  // extern "C"
