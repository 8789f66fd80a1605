// fbx_sweep.hip -- fbx_kraus_sweep: Kraus operators -> Choi, Pauli-Liouville and chi matrix + process fidelity against a
// reference in one pass over the batch (BASELINE config 3), and fbx_process_fidelity.  One 64-lane wavefront per item or pair
// of items for 1-2 qubits, one workgroup per item for 3; the primitives are those of fbx_superop_prims.hpp.
//
// Reference functions (file:line under forest/benchmarking/):
//   operator_tools/superoperator_transformations.py:82-182,339-371   (kraus2choi / kraus2pauli_liouville / kraus2chi)
//   distance_measures.py:271-359                                     (entanglement / process fidelity)
#include "fbx_superop_prims.hpp"
#include <cstdlib>
#include <algorithm>

namespace fbx {

// ---------------------------------------------------------------------------------------------
// fused Kraus sweep (BASELINE config 3)
// ---------------------------------------------------------------------------------------------
template <int NQ>
__global__ void __launch_bounds__(64)
sweep_kernel(long long B, int K, const double* __restrict__ kraus, const double* __restrict__ ptm_ref,
             double* __restrict__ choi_out, double* __restrict__ ptm_out, double* __restrict__ chi_out,
             double* __restrict__ fid_out) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* C = (cplx*)smem;                 // Choi
    cplx* S = C + D * LD;                  // superop, then chi
    cplx* P = S + D * LD;                  // Pauli-Liouville
    cplx* R = P + D * LD;                  // reference PTM
    cplx* kb = R + D * LD;
    const int lane = threadIdx.x;
    if (ptm_ref) load_matrix<NQ>(ptm_ref, R, lane);
    const double inv_d = 1.0 / d;
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        __syncthreads();
        kraus_to<NQ>(kraus + item * (long long)K * D * 2, K, false, C, kb, lane);
        __syncthreads();
        if (choi_out) store_matrix<NQ>(C, choi_out + item * (long long)D * D * 2, lane);
        reshuffle<NQ>(C, S, lane);
        __syncthreads();
        to_pauli_basis<NQ>(S, P, inv_d, lane);
        __syncthreads();
        if (ptm_out) store_matrix<NQ>(P, ptm_out + item * (long long)D * D * 2, lane);
        if (fid_out && ptm_ref) {          // process_fidelity(ref, ptm): (d Fe + 1)/(d + 1), Fe = tr(ref^H ptm)/d^2
            double acc = 0.0;
            for (int idx = lane; idx < D * D; idx += 64) {
                const cplx a = R[(idx / D) * LD + idx % D], b = P[(idx / D) * LD + idx % D];
                acc += a.re * b.re + a.im * b.im;
            }
            acc = wave_sum(acc);
            if (lane == 0) fid_out[item] = (d * (acc / (double)(d * d)) + 1.0) / (d + 1.0);
        }
        if (chi_out) {                      // a Kraus set is CP: chi = c2p Choi c2p^H (= kraus2chi)
            to_pauli_basis<NQ>(C, S, inv_d * inv_d, lane);
            __syncthreads();
            store_matrix<NQ>(S, chi_out + item * (long long)D * D * 2, lane);
        }
    }
}


// ---------------------------------------------------------------------------------------------
// sweep2q_pair_kernel: the same pipeline with HALF the LDS traffic (round 1's one-item-per-wavefront kernel was LDS-bandwidth
// bound: ~100 KB per item).  A wavefront takes TWO Kraus sets; 16 lanes own one 16 x 16 matrix (A ->
// Pauli-Liouville and W -> chi of each item), 16 elements per lane, so that TWO butterfly stages run in
// registers per pass and one LDS transpose separates the two passes.  The passes are ordered so that the
// final registers of a lane are one column (PTM) / one column (chi) of the output in matrix order: the
// results go from registers to HBM in 256-byte runs, no gather through LDS.  The process fidelity uses
// tr(R_ref^H R) = tr(E_ref^H E) (the Pauli transform is unitary up to the factor d), so it is reduced from
// the Choi accumulators against the Choi form of the reference, before any transform.
// Element index = row * 16 + col (8 bits); lane-group roles: (lane >> 5) = item of the pair,
// (lane >> 4) & 1 = 0: A, 1: W; within the group, 4 index bits come from the lane and 4 from the register.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ constexpr int dep4(int v, int b3, int b2, int b1, int b0) {
    return (((v >> 3) & 1) << b3) | (((v >> 2) & 1) << b2) | (((v >> 1) & 1) << b1) | ((v & 1) << b0);
}
__device__ __forceinline__ constexpr int padded(int idx) { return idx + (idx >> 4); }     // (idx >> 4) * 17 + (idx & 15)

__global__ void __launch_bounds__(64)
sweep2q_pair_kernel(long long B, int K, const double* __restrict__ kraus, const double* __restrict__ choi_ref,
                    double* __restrict__ choi_out, double* __restrict__ ptm_out, double* __restrict__ chi_out,
                    double* __restrict__ fid_out) {
    constexpr int D = 16, MAT = 16 * 17;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* bufA = (cplx*)smem;              // [2][MAT] Choi of the item, then the A transpose
    cplx* bufW = bufA + 2 * MAT;           // [2][MAT] W transpose
    cplx* kbs = bufW + 2 * MAT;            // [2][K * 16] vec of the Kraus operators
    const int lane = threadIdx.x;
    const int h = lane >> 5, u = lane & 31, w = (lane >> 4) & 1, l = lane & 15;
    const int col = u & 15, row0 = (u >> 4) * 8;           // kraus2choi: this lane owns C[row0 .. row0 + 7][col]
    // LDS addresses of the 16 registers in the two passes (additive: lane part + register part, no carries)
    const int la1 = padded(w ? dep4(l, 7, 6, 5, 4) : dep4(l, 5, 4, 1, 0));
    const int la2 = padded(w ? dep4(l, 3, 2, 1, 0) : dep4(l, 7, 6, 3, 2));
    const int jcol = ((l >> 3) & 1) << 3 | ((l >> 1) & 1) << 2 | ((l >> 2) & 1) << 1 | (l & 1);   // output column of this lane
    cplx* mine = (w ? bufW : bufA) + h * MAT;              // where this lane's matrix is transposed
    const cplx* src = bufA + h * MAT;                      // the item's Choi matrix
    cplx* kb = kbs + h * K * D;
    // reference in Choi form, in the kraus2choi layout
    cplx ref[8];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        ref[rr].re = ref[rr].im = 0.0;
        if (choi_ref) { const double* q = choi_ref + 2 * ((row0 + rr) * D + col); ref[rr].re = q[0]; ref[rr].im = q[1]; }
    }
#define FBX_WAVE_FENCE() asm volatile("" ::: "memory")
    const int n_ld = (K * D + 31) / 32;                    // 16-byte loads per lane and item (K <= 16: at most 8)
    const long long n_pairs = (B + 1) / 2;
    double2 nxt[8];
    auto fetch = [&](long long pair) {
        const long long item = 2 * pair + h;
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8) {
            const int idx = u + 32 * t8;
            if (t8 < n_ld && idx < K * D && item < B)
                nxt[t8] = *reinterpret_cast<const double2*>(kraus + (item * (long long)K * D + idx) * 2);
        }
    };
#pragma unroll
    for (int t8 = 0; t8 < 8; ++t8) nxt[t8].x = nxt[t8].y = 0.0;
    if ((long long)blockIdx.x < n_pairs) fetch(blockIdx.x);
    for (long long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
        const long long item = 2 * pair + h;
        const bool live = item < B;
        // ---- Kraus operators -> LDS as vec(K_t)[c * 4 + r] = K_t[r][c]; next pair's operators from HBM meanwhile
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8) {
            const int idx = u + 32 * t8;
            if (t8 < n_ld && idx < K * D) {
                const int t = idx >> 4, rr = (idx >> 2) & 3, cc = idx & 3;
                cplx c; c.re = nxt[t8].x; c.im = nxt[t8].y;
                kb[t * D + cc * 4 + rr] = c;
            }
        }
        if (pair + gridDim.x < n_pairs) fetch(pair + gridDim.x);
        FBX_WAVE_FENCE();
        // ---- kraus2choi: C[row][col] = sum_t vK_t[row] conj(vK_t[col])
        cplx acc[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) acc[rr].re = acc[rr].im = 0.0;
        for (int t = 0; t < K; ++t) {
            const cplx b = kb[t * D + col];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const cplx a = kb[t * D + row0 + rr];
                acc[rr].re += a.re * b.re + a.im * b.im;
                acc[rr].im += a.im * b.re - a.re * b.im;
            }
        }
        double fr = 0.0;
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            bufA[h * MAT + (row0 + rr) * 17 + col] = acc[rr];
            fr += ref[rr].re * acc[rr].re + ref[rr].im * acc[rr].im;
            if (choi_out && live) {
                double2 v; v.x = acc[rr].re; v.y = acc[rr].im;
                FBX_STREAM_STORE(reinterpret_cast<double2*>(choi_out + (item * D * D + (row0 + rr) * D + col) * 2), v);
            }
        }
        if (fid_out) {                                     // sum over the 32 lanes of the item
            fr += dpp_permute<0xB1>(fr); fr += dpp_permute<0x4E>(fr);
            fr += dpp_permute<0x141>(fr); fr += dpp_permute<0x140>(fr);
            const double tot = readlane_f64(fr, 0) + readlane_f64(fr, 16), tot1 = readlane_f64(fr, 32) + readlane_f64(fr, 48);
            if (u == 0 && live) fid_out[item] = (4.0 * ((h ? tot1 : tot) / 16.0) + 1.0) / 5.0;
        }
        FBX_WAVE_FENCE();
        // ---- pass 1: A sites (7,3),(6,2) [-i: input qubits]; W sites (3,1),(2,0) [+i]
        cplx x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            x[r] = src[la1 + (w ? padded(dep4(r, 3, 1, 2, 0)) : padded(dep4(r, 7, 3, 6, 2)))];
        two_sites(x, w ? +1.0 : -1.0, w ? +1.0 : -1.0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            mine[la1 + (w ? padded(dep4(r, 3, 1, 2, 0)) : padded(dep4(r, 7, 3, 6, 2)))] = x[r];
        FBX_WAVE_FENCE();
        // ---- pass 2: A sites (5,1),(4,0) [+i: output qubits]; W sites (7,5),(6,4) [-i]
#pragma unroll
        for (int r = 0; r < 16; ++r)
            x[r] = mine[la2 + (w ? padded(dep4(r, 7, 5, 6, 4)) : padded(dep4(r, 5, 1, 4, 0)))];
        two_sites(x, w ? -1.0 : +1.0, w ? -1.0 : +1.0);
        // ---- register r = output row i, lane = output column jcol: 256-byte runs straight to HBM
        double* dst = w ? chi_out : ptm_out;
        const double scale = w ? 0.0625 : 0.25;
        if (dst && live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double2 o; o.x = x[r].re * scale; o.y = x[r].im * scale;
                FBX_STREAM_STORE(reinterpret_cast<double2*>(dst + (item * D * D + r * D + jcol) * 2), o);
            }
        }
        FBX_WAVE_FENCE();
    }
#undef FBX_WAVE_FENCE
}

// persistent grid of the 2-qubit sweep: 8 wavefronts resident per CU, the rest queued
#define FBX_SWEEP_GRID (256 * 16)
static_assert(FBX_SWEEP_GRID > 0, "FBX_SWEEP_GRID must be positive");

template <int NQ>
static int launch_sweep(int64_t B, int K, const double* kraus, const double* ptm_ref, double* choi,
                        double* ptm, double* chi, double* fid) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1;
    const size_t lds = sizeof(cplx) * (4 * D * LD + (size_t)K * D);
    if (lds > 160 * 1024) { set_error("fbx_kraus_sweep: too many Kraus operators"); return FBX_ERR_UNSUPPORTED; }
    if (NQ == 2 && K <= 16) {
        // reference in Choi form for the on-the-fly fidelity (one 16 x 16 conversion per call, into a
        // workspace of the calling thread)
        double* choi_ref = nullptr;
        if (ptm_ref) {
            void* w = nullptr;
            { const int rc = workspace(WS_SWEEP_REF, sizeof(cplx) * 256, &w); if (rc) return rc; }
            choi_ref = (double*)w;
            { const int rc = convert_launch(2, FBX_REP_PAULI_LIOUVILLE, FBX_REP_CHOI, 1, ptm_ref, 0, choi_ref); if (rc) return rc; }
        }
        const size_t ldsp = sizeof(cplx) * (4 * 16 * 17 + 2 * (size_t)K * 16);
        const unsigned gridp = (unsigned)std::min<int64_t>((B + 1) / 2, FBX_SWEEP_GRID);
        return launch_lds(sweep2q_pair_kernel, dim3(gridp), dim3(64), ldsp, B, K, kraus, choi_ref, choi, ptm, chi, fid);
    }
    return launch_lds(sweep_kernel<NQ>, dim3((unsigned)std::min<int64_t>(B, 256 * 8)), dim3(64), lds, B, K, kraus, ptm_ref, choi, ptm, chi, fid);
}

// ---------------------------------------------------------------------------------------------
// entanglement / process fidelity: Fe = Re tr(A^H B) / d^2 ; Fp = (d Fe + 1) / (d + 1)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
process_fidelity_kernel(int d, long long B, const double* __restrict__ a, int a_batched, const double* __restrict__ b,
                        double* __restrict__ fe_out, double* __restrict__ fp_out) {
    const int lane = threadIdx.x;
    const int DD = d * d * d * d;
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        const double* pa = a + (a_batched ? item : 0) * (long long)DD * 2;      // one shared reference or one per item
        const double* pb = b + item * (long long)DD * 2;
        double acc = 0.0;
        for (int idx = lane; idx < 2 * DD; idx += 64) acc += pa[idx] * pb[idx];
        acc = wave_sum(acc);
        if (lane == 0) {
            const double fe = acc / (double)(d * d);
            if (fe_out) fe_out[item] = fe;
            if (fp_out) fp_out[item] = (d * fe + 1.0) / (d + 1.0);
        }
    }
}

// Three qubits, fused (round 4): one 1024-thread workgroup walks its items through ONE 64 x 64 LDS matrix (68 KB with the
// Kraus operators: two workgroups per CU), kraus2superop -> six in-place butterfly stages -> Pauli-Liouville matrix out with the
// process fidelity reduced on the way, then kraus2choi -> Choi out -> the same stages -> chi out (a Kraus set is CP, so
// chi = c2p Choi c2p^H exactly as kraus2chi, superoperator_transformations.py:82-98).  The operators are read once (K KB), the
// three 64 KB results written once, coalesced 16 bytes per thread: 4 x 1024 + 3 x 65 536 + 8 algorithmic bytes per item for
// K = 4.  Replaces the composition of three general 64 x 64 conversions + a fidelity kernel behind fbx_kraus_sweep (each of
// which re-read the operators and kept two matrices in LDS).  Reference: superoperator_transformations.py:100-182, 339-371;
// distance_measures.py:315-360.
__global__ void __launch_bounds__(1024)
sweep3_kernel(long long B, int K, const double* __restrict__ kraus, const double* __restrict__ ptm_ref,
              double* __restrict__ choi_out, double* __restrict__ ptm_out, double* __restrict__ chi_out,
              double* __restrict__ fid_out) {
    constexpr int NQ = 3, d = 8, D = 64, LD = 64, NT = 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* X = (cplx*)smem;
    double* red = (double*)(X + D * D);
    cplx* kb = (cplx*)(red + 16);
    const int t = threadIdx.x;
    const double inv_d = 1.0 / d;
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        __syncthreads();                                   // the previous item's readers of X / kb / red are done
        const double* kr = kraus + item * (long long)K * D * 2;
        for (int idx = t; idx < K * D; idx += NT) { kb[idx].re = kr[2 * idx]; kb[idx].im = kr[2 * idx + 1]; }
        __syncthreads();
        if (ptm_out || fid_out) {
            for (int idx = t; idx < D * D; idx += NT) X[idx] = kraus_superop_entry(kb, K, d, idx / D, idx % D);
            __syncthreads();
            site_stages<NQ, false, NT, LD>(X, t);
            double acc = 0.0;
            double* dst = ptm_out ? ptm_out + item * (long long)D * D * 2 : nullptr;
            for (int idx = t; idx < D * D; idx += NT) {
                cplx v = X[site_index<NQ>(idx / D) * LD + site_index<NQ>(idx % D)];
                v.re *= inv_d; v.im *= inv_d;
                if (dst) { dst[2 * idx] = v.re; dst[2 * idx + 1] = v.im; }
                if (fid_out) acc += ptm_ref[2 * idx] * v.re + ptm_ref[2 * idx + 1] * v.im;
            }
            if (fid_out) {
                acc = block_sum<NT>(acc, red);
                if (t == 0) fid_out[item] = (d * (acc / (double)(d * d)) + 1.0) / (d + 1.0);
            }
            __syncthreads();                               // X is rebuilt below
        }
        if (choi_out || chi_out) {
            double* dst = choi_out ? choi_out + item * (long long)D * D * 2 : nullptr;
            // not kraus_choi_entry: this sum fuses the other product of its imaginary part (a.im b.re, not a.re b.im), as
            // sweep3_regs_kernel and sweep2q_pair_kernel do, and the three agree bit for bit
            for (int idx = t; idx < D * D; idx += NT) {    // vec(K)[c d + r] = K[r][c]; choi[row][col] = vK[row] conj(vK[col])
                const int row = idx / D, col = idx % D;
                double re = 0.0, im = 0.0;
                for (int q = 0; q < K; ++q) {
                    const cplx a = kb[q * D + (row % d) * d + row / d], b = kb[q * D + (col % d) * d + col / d];
                    re += a.re * b.re + a.im * b.im;
                    im += a.im * b.re - a.re * b.im;
                }
                if (dst) { dst[2 * idx] = re; dst[2 * idx + 1] = im; }
                cplx o; o.re = re; o.im = im;
                X[idx] = o;
            }
            if (chi_out) {
                __syncthreads();
                site_stages<NQ, false, NT, LD>(X, t);
                double* cx = chi_out + item * (long long)D * D * 2;
                const double sc = inv_d * inv_d;
                for (int idx = t; idx < D * D; idx += NT) {
                    const cplx v = X[site_index<NQ>(idx / D) * LD + site_index<NQ>(idx % D)];
                    cx[2 * idx] = v.re * sc; cx[2 * idx + 1] = v.im * sc;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
sweep3_regs_kernel(long long B, int K, const double* __restrict__ kraus, const double* __restrict__ ptm_ref,
                   double* __restrict__ choi_out, double* __restrict__ ptm_out, double* __restrict__ chi_out,
                   double* __restrict__ fid_out) {
    constexpr int d = 8, D = 64, NT = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* X = (cplx*)smem;
    double* red = (double*)(X + D * D);
    cplx* kb = (cplx*)(red + 16);
    const int t = threadIdx.x;
    const S3Tile tile(t);
    const int row1 = tile.row1, col1 = tile.col1;
    const double inv_d = 1.0 / d;
    const int n_ld = (K * D + NT - 1) / NT;                // operator entries per thread (K <= 31: at most 8)
    double2 nxt[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) nxt[q].x = nxt[q].y = 0.0;
    auto fetch = [&](long long item) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int idx = t + NT * q;
            if (q < n_ld && idx < K * D) nxt[q] = *reinterpret_cast<const double2*>(kraus + (item * (long long)K * D + idx) * 2);
        }
    };
    if ((long long)blockIdx.x < B) fetch(blockIdx.x);
    // passes 2 and 3 of one transform: X holds the tile after P1; `dst` gets the result times `scale`; returns the thread's share of
    // <ref, result> when asked
    auto finish = [&](double* __restrict__ dst, double scale, const double* __restrict__ ref) -> double {
        double acc = 0.0;
        tile.passes23(X, [](cplx (&x)[16], double y1, double y2) { two_sites(x, y1, y2); }, [&](int r, const cplx& xr) {
            const long long o = ((long long)(tile.krow + r) * D + tile.lcol) * 2;
            double2 v; v.x = xr.re * scale; v.y = xr.im * scale;
            if (dst) FBX_STREAM_STORE(reinterpret_cast<double2*>(dst + o), v);
            if (ref) { const double2 q = *reinterpret_cast<const double2*>(ref + o); acc += q.x * v.x + q.y * v.y; }
        });
        return acc;
    };
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        __syncthreads();                                   // the previous item's readers of X / kb / red are done
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int idx = t + NT * q;
            if (q < n_ld && idx < K * D) { cplx c; c.re = nxt[q].x; c.im = nxt[q].y; kb[idx] = c; }
        }
        if (item + gridDim.x < B) fetch(item + gridDim.x); // the next item's operators arrive behind this item's work
        __syncthreads();
        if (ptm_out || fid_out) {
            // P1 on kron(conj(K), K)[(i,k)][(j,l)] = conj(K[i][j]) K[k][l]: row = 8 i + k, col = 8 j + l
            cplx x[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r].re = x[r].im = 0.0;
            const int i0 = row1 >> 3, k0 = row1 & 7, j0 = col1 >> 3, l0 = col1 & 7;      // bit 2 of each comes from the register
            for (int q = 0; q < K; ++q) {
                cplx a[2][2], b[2][2];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 2; ++v) {
                        a[u][v] = kb[q * D + (i0 | u << 2) * d + (j0 | v << 2)];
                        b[u][v] = kb[q * D + (k0 | u << 2) * d + (l0 | v << 2)];
                    }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const cplx aa = a[(r >> 3) & 1][(r >> 1) & 1], bb = b[(r >> 2) & 1][r & 1];
                    x[r].re += aa.re * bb.re + aa.im * bb.im;
                    x[r].im += aa.re * bb.im - aa.im * bb.re;
                }
            }
            two_sites(x, -1.0, +1.0);                      // row site 2 (-i), column site 2 (+i)
            tile.store1(X, x);
            __syncthreads();
            double acc = finish(ptm_out ? ptm_out + item * (long long)D * D * 2 : nullptr, inv_d, fid_out ? ptm_ref : nullptr);
            if (fid_out) {
                acc = block_sum<NT>(acc, red);
                if (t == 0) fid_out[item] = (d * (acc / (double)(d * d)) + 1.0) / (d + 1.0);
            }
            __syncthreads();                               // X is rebuilt below
        }
        if (choi_out || chi_out) {
            // P1 on choi[row][col] = vK[row] conj(vK[col]), vK[8 c + r] = K[r][c]
            cplx x[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r].re = x[r].im = 0.0;
            for (int q = 0; q < K; ++q) {
                cplx a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = row1 | ((u >> 1) & 1) << 5 | (u & 1) << 2, col = col1 | ((u >> 1) & 1) << 5 | (u & 1) << 2;
                    a[u] = kb[q * D + (row % d) * d + row / d];
                    b[u] = kb[q * D + (col % d) * d + col / d];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const cplx aa = a[r >> 2], bb = b[r & 3];
                    x[r].re += aa.re * bb.re + aa.im * bb.im;
                    x[r].im += aa.im * bb.re - aa.re * bb.im;
                }
            }
            if (choi_out) {
                double* dst = choi_out + item * (long long)D * D * 2;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    double2 v; v.x = x[r].re; v.y = x[r].im;
                    FBX_STREAM_STORE(reinterpret_cast<double2*>(dst + ((long long)(row1 | tile.reg_row1(r)) * D + (col1 | tile.reg_col1(r))) * 2), v);
                }
            }
            if (chi_out) {
                two_sites(x, -1.0, +1.0);
                tile.store1(X, x);
                __syncthreads();
                (void)finish(chi_out + item * (long long)D * D * 2, inv_d * inv_d, nullptr);
            }
        }
    }
}
// LDS of both 3-qubit sweep kernels: the 64 x 64 tile, the reduction scratch, the Kraus operators
static size_t sweep3_lds(int K) { return sizeof(cplx) * 64 * 64 + sizeof(double) * 16 + sizeof(cplx) * (size_t)K * 64; }
int launch_sweep3_regs(int64_t B, int K, const double* kraus, const double* ptm_ref, double* choi, double* ptm, double* chi, double* fid) {
    return launch_lds(sweep3_regs_kernel, dim3((unsigned)std::min(B, S3_GRID)), dim3(256), sweep3_lds(K), B, K, kraus, ptm_ref, choi, ptm, chi, fid);
}
// one wavefront per item, at most this many
constexpr int64_t FIDELITY_GRID = 8192;

// Three qubits, unfused (kept as the reference form: FBX_SWEEP3_COMPOSED=1 in the environment of a diagnostics build, and the
// fallback for more than 31 Kraus operators): the composition of the pairwise 64 x 64 conversions and the fidelity reduction.
static int launch_sweep3_composed(int64_t B, int K, const double* kraus, const double* ptm_ref, double* choi, double* ptm,
                         double* chi, double* fid) {
    constexpr size_t D = 64;
    DevBuf tmp;
    double* ptm_buf = ptm;
    if (fid && !ptm_buf) {
        const int rc = tmp.alloc(sizeof(cplx) * D * D * (size_t)B);
        if (rc) return rc;
        ptm_buf = tmp.as<double>();
    }
    int rc = FBX_OK;
    if (choi && (rc = convert_launch(3, FBX_REP_KRAUS, FBX_REP_CHOI, B, kraus, K, choi))) return rc;
    if (ptm_buf && (rc = convert_launch(3, FBX_REP_KRAUS, FBX_REP_PAULI_LIOUVILLE, B, kraus, K, ptm_buf))) return rc;
    if (chi && (rc = convert_launch(3, FBX_REP_KRAUS, FBX_REP_CHI, B, kraus, K, chi))) return rc;
    if (fid) {
        FBX_TRY(launch_lds(process_fidelity_kernel, dim3((unsigned)std::min(B, FIDELITY_GRID)), dim3(64), 0, 8, B, ptm_ref, 0, ptm_buf, nullptr, fid));
        if (tmp.p) FBX_HIP(hipStreamSynchronize(stream()));      // the scratch PTMs go away with `tmp`
    }
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

static int kraus_sweep_check(int n_qubits, int64_t B, int K, const void* kraus, const void* ptm_ref, const void* fid_out) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 3, "fbx_kraus_sweep: n_qubits must be 1..3");
    FBX_REQUIRE(B >= 0 && K >= 1 && (B == 0 || kraus), "fbx_kraus_sweep: bad arguments");
    FBX_REQUIRE(!fid_out || ptm_ref, "fbx_kraus_sweep: fidelity output needs a reference PTM");
    return FBX_OK;
}

int fbx_kraus_sweep_dev(int n_qubits, int64_t B, int K, const double* d_kraus, const double* d_ptm_ref,
                        double* d_choi_out, double* d_ptm_out, double* d_chi_out, double* d_fid_out) {
    FBX_TRY(kraus_sweep_check(n_qubits, B, K, d_kraus, d_ptm_ref, d_fid_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    if (n_qubits == 3) {
        if (sweep3_lds(K) > 80 * 1024) return launch_sweep3_composed(B, K, d_kraus, d_ptm_ref, d_choi_out, d_ptm_out, d_chi_out, d_fid_out);
        const char* v1s = getenv("FBX_SWEEP3_V1");                   // 1 = the one-stage-per-pass form (A/B, tests)
        if (v1s && atoi(v1s) != 0)
            return launch_lds(sweep3_kernel, dim3((unsigned)std::min(B, S3_GRID)), dim3(1024), sweep3_lds(K), B, K, d_kraus, d_ptm_ref,
                              d_choi_out, d_ptm_out, d_chi_out, d_fid_out);
        return launch_sweep3_regs(B, K, d_kraus, d_ptm_ref, d_choi_out, d_ptm_out, d_chi_out, d_fid_out);
    }
    if (n_qubits == 1) return launch_sweep<1>(B, K, d_kraus, d_ptm_ref, d_choi_out, d_ptm_out, d_chi_out, d_fid_out);
    return launch_sweep<2>(B, K, d_kraus, d_ptm_ref, d_choi_out, d_ptm_out, d_chi_out, d_fid_out);
}

int fbx_kraus_sweep(int n_qubits, int64_t B, int K, const double* kraus, const double* ptm_ref,
                    double* choi_out, double* ptm_out, double* chi_out, double* fid_out) {
    FBX_TRY(kraus_sweep_check(n_qubits, B, K, kraus, ptm_ref, fid_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d, nm = D * D * 2 * B;
    // fbx_set_devices: contiguous blocks of the batch on the workers of the device list (the items are independent)
    if (device_list_size() > 1 && !in_device_worker() && B >= 2 * (int64_t)device_list_size()) {
        return run_on_devices([&](int g, int G) -> int {       // G: the list's length as run_on_devices read it, under its lock
            const int64_t per = (B + G - 1) / G;
            const int64_t lo = (int64_t)g * per < B ? (int64_t)g * per : B, nb = (B - lo < per ? B - lo : per);
            if (nb <= 0) return FBX_OK;
            const size_t om = (size_t)lo * D * D * 2;
            return fbx_kraus_sweep(n_qubits, nb, K, kraus + (size_t)lo * K * D * 2, ptm_ref, choi_out ? choi_out + om : nullptr,
                                   ptm_out ? ptm_out + om : nullptr, chi_out ? chi_out + om : nullptr, fid_out ? fid_out + lo : nullptr);
        });
    }
    HostIO io; double *dk, *dr = nullptr, *dc, *dp, *dx, *df;
    FBX_TRY(io.in(kraus, (size_t)K * D * 2 * B, &dk));
    if (ptm_ref) FBX_TRY(io.in(ptm_ref, D * D * 2, &dr));
    FBX_TRY(io.out_opt(choi_out, nm, &dc)); FBX_TRY(io.out_opt(ptm_out, nm, &dp));
    FBX_TRY(io.out_opt(chi_out, nm, &dx)); FBX_TRY(io.out_opt(fid_out, (size_t)B, &df));
    FBX_TRY(fbx_kraus_sweep_dev(n_qubits, B, K, dk, dr, dc, dp, dx, df));
    return io.finish();
}

static int process_fidelity_check(int n_qubits, int64_t B, const void* ptm0, const void* ptm1) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 5, "fbx_process_fidelity: n_qubits must be 1..5");
    FBX_REQUIRE(B >= 0 && (B == 0 || (ptm0 && ptm1)), "fbx_process_fidelity: bad batch / NULL buffer");
    return FBX_OK;
}

int fbx_process_fidelity_dev(int n_qubits, int64_t B, const double* d_ptm0, const double* d_ptm1, double* d_fe_out, double* d_fp_out) {
    FBX_TRY(process_fidelity_check(n_qubits, B, d_ptm0, d_ptm1));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    return launch_lds(process_fidelity_kernel, dim3((unsigned)std::min(B, FIDELITY_GRID)), dim3(64), 0, 1 << n_qubits, B, d_ptm0, 1, d_ptm1, d_fe_out, d_fp_out);
}

int fbx_process_fidelity(int n_qubits, int64_t B, const double* ptm0, const double* ptm1, double* fe_out, double* fp_out) {
    FBX_TRY(process_fidelity_check(n_qubits, B, ptm0, ptm1));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d, nm = D * D * 2 * B;
    HostIO io; double *da, *db, *dfe, *dfp;
    FBX_TRY(io.in(ptm0, nm, &da)); FBX_TRY(io.in(ptm1, nm, &db));
    FBX_TRY(io.out(fe_out, (size_t)B, &dfe)); FBX_TRY(io.out(fp_out, (size_t)B, &dfp));
    FBX_TRY(fbx_process_fidelity_dev(n_qubits, B, da, db, dfe, dfp));
    return io.finish();
}

}  // extern "C"
