// fbx_linalg.hip -- the library's general batched linear algebra on stacks of N x N complex matrices, N up to 1024: the
// Hermitian eigendecomposition (fbx_eigh: LDS-resident up to 64 x 64, HBM-resident or one matrix over the whole chip above),
// op(A) diag(s) op(B) (fbx_matmul) and choi2kraus on top of the eigensolver (fbx_choi2kraus).  What the superoperator
// conversions, the validators, sqrtm_psd and the projections at sizes without a kernel of their own are built from.
#include "fbx_eigh64.hpp"
#include <hip/hip_cooperative_groups.h>
#include <cmath>
#include <limits>
#include <algorithm>
#include <vector>
#include <cstring>

namespace fbx {

// generic batched eigh (lower triangle read, ascending eigenvalues, eigenvectors as columns).
// One workgroup of NT = max(64, (N/2)^2) threads per matrix: one wavefront up to 16 x 16, four for
// 32 x 32, sixteen for 64 x 64 (128 KiB of LDS for the matrix and the eigenvectors).
template <int N, int NT>
__global__ void __launch_bounds__(NT)
eigh_kernel(long long B, const double* __restrict__ a, double* __restrict__ w_out, double* __restrict__ v_out) {
    constexpr int NB = N / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* Ms = (cplx*)smem;
    cplx* Vs = Ms + sys_elems<N>();
    double* lam = (double*)(Vs + sys_elems<N>());
    double* red = lam + N;
    int* pos = (int*)(red + 64);
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    const double* src = a + item * (long long)N * N * 2;
    Blk h = blk_zero();
    int nonfinite = 0;                  // over the entries read: the diagonal's real parts and the strictly lower triangle
    if (lane < NB * NB) {
        const int I = lane / NB, J = lane % NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
            if (r > c) { h.re[e] = src[2 * (r * N + c)]; h.im[e] = src[2 * (r * N + c) + 1]; }
            else if (r < c) { h.re[e] = src[2 * (c * N + r)]; h.im[e] = -src[2 * (c * N + r) + 1]; }
            else { h.re[e] = src[2 * (r * N + c)]; h.im[e] = 0.0; }
            nonfinite |= !(isfinite(h.re[e]) && isfinite(h.im[e]));
        }
    }
    // A non-finite item gives NaN for itself only (include/fbx.h): the solver's stopping test is false on a NaN and would
    // hand back the sorted diagonal with the identity.  The item is solved as the zero matrix and NaN is written in its place.
    nonfinite = __syncthreads_or(nonfinite);
    if (nonfinite) h = blk_zero();
    sys_store<N>(Ms, lane, h);
    __syncthreads();
    jacobi_eigh_block<N, NT>(Ms, Vs, lane, true, red);
    if (nonfinite) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (lane < N) w_out[item * N + lane] = nan;
        if (v_out) for (int idx = lane; idx < 2 * N * N; idx += NT) v_out[item * N * N * 2 + idx] = nan;
        return;
    }
    if (lane < N) lam[lane] = Ms[sys_index<N>(lane, lane)].re;
    __syncthreads();
    if (lane < N) {                     // rank of eigenvalue `lane` in ascending order (stable)
        int rank = 0;
        for (int j = 0; j < N; ++j) rank += (lam[j] < lam[lane]) || (lam[j] == lam[lane] && j < lane);
        pos[lane] = rank;
        w_out[item * N + rank] = lam[lane];
    }
    __syncthreads();
    if (v_out) {
        for (int idx = lane; idx < N * N; idx += NT) {
            const int r = idx / N, k = idx % N;
            const cplx v = Vs[sys_index<N>(r, k)];
            double* o = v_out + ((item * N + r) * N + pos[k]) * 2;
            o[0] = v.re; o[1] = v.im;
        }
    }
}

// ---- Hermitian eigendecomposition for 64 < N <= 1024 (4- and 5-qubit Choi matrices, padded odd sizes): the same
// systolic two-sided Jacobi with the matrix and the eigenvectors in HBM / L2 instead of LDS.  One 1024-thread
// workgroup per matrix; a round = (a) the N/2 rotations from the pivot blocks into an LDS table, (b) every 2 x 2
// block rotated and written to the seats the tournament permutation assigns it -- from the `cur` copies into the
// `nxt` copies, so no entry is overwritten before it is read -- and the copies swap.  Correctness first: this
// serves validators, choi2kraus and sqrtm of large operators, not a benchmark (one CU per matrix, ~20 us per round).
__device__ __forceinline__ int jacobi_seat_rt(int NB, int s) {           // jacobi_seat<N> with N at run time
    if (NB == 1) return s;
    const int k = s >> 1;
    if ((s & 1) == 0) {
        if (k == 0) return 0;
        if (k == NB - 1) return 2 * (NB - 1) + 1;
        return 2 * (k + 1);
    }
    if (k == 0) return 2;
    return 2 * (k - 1) + 1;
}

__global__ void __launch_bounds__(1024)
eigh_big_kernel(int N, long long B, const double* __restrict__ a, double* __restrict__ w_out, double* __restrict__ v_out,
                cplx* __restrict__ work) {
    constexpr int NT = 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* rot = (double*)smem;                 // [N/2][4]: c, sr, si, -
    double* lam = rot + 2 * N;                   // [N]
    int* pos = (int*)(lam + N);                  // [N]
    double* red = (double*)(pos + N);            // [64]
    const int t = threadIdx.x, NB = N / 2;
    const long long item = blockIdx.x;
    const size_t NN = (size_t)N * N;
    cplx* M0 = work + (size_t)item * 4 * NN;
    cplx* M1 = M0 + NN; cplx* V0 = M1 + NN; cplx* V1 = V0 + NN;
    const double* src = a + item * (long long)NN * 2;
    int nonfinite = 0;
    for (size_t idx = t; idx < NN; idx += NT) {            // numpy eigh: the lower triangle defines the matrix
        const int r = (int)(idx / N), c = (int)(idx % N);
        cplx h, v;
        if (r > c) { h.re = src[2 * idx]; h.im = src[2 * idx + 1]; }
        else if (r < c) { h.re = src[2 * ((size_t)c * N + r)]; h.im = -src[2 * ((size_t)c * N + r) + 1]; }
        else { h.re = src[2 * idx]; h.im = 0.0; }
        nonfinite |= !(isfinite(h.re) && isfinite(h.im));
        v.re = r == c ? 1.0 : 0.0; v.im = 0.0;
        M0[idx] = h; V0[idx] = v;
    }
    if (__syncthreads_or(nonfinite)) {                     // a non-finite item gives NaN for itself only (include/fbx.h)
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int k = t; k < N; k += NT) w_out[item * N + k] = nan;
        if (v_out) for (size_t idx = t; idx < 2 * NN; idx += NT) v_out[(size_t)item * NN * 2 + idx] = nan;
        return;
    }
    cplx *Mc = M0, *Mn = M1, *Vc = V0, *Vn = V1;
    for (int sweep = 0; sweep < FBX_JACOBI_MAX_SWEEPS; ++sweep) {
        double o2 = 0.0, n2 = 0.0;
        for (size_t idx = t; idx < NN; idx += NT) {
            const cplx v = Mc[idx];
            const double a2 = v.re * v.re + v.im * v.im;
            n2 += a2;
            if (idx / N != idx % N) o2 += a2;
        }
        block_sum2<NT>(o2, n2, red);
        if (!(o2 > FBX_JACOBI_TOL2 * n2)) break;
        for (int r = 0; r < N - 1; ++r) {
            for (int p = t; p < NB; p += NT) {
                const cplx b = Mc[(size_t)(2 * p) * N + 2 * p + 1];
                const JRot q = jacobi_rotation(Mc[(size_t)(2 * p) * N + 2 * p].re, Mc[(size_t)(2 * p + 1) * N + 2 * p + 1].re, b.re, b.im);
                rot[4 * p] = q.c; rot[4 * p + 1] = q.sr; rot[4 * p + 2] = q.si;
            }
            __syncthreads();
            for (int blk = t; blk < NB * NB; blk += NT) {
                const int I = blk / NB, J = blk % NB;
                const size_t r0 = (size_t)(2 * I) * N + 2 * J, r1 = r0 + N;
                cplx m00 = Mc[r0], m01 = Mc[r0 + 1], m10 = Mc[r1], m11 = Mc[r1 + 1];
                cplx v0p = Vc[r0], v0q = Vc[r0 + 1], v1p = Vc[r1], v1q = Vc[r1 + 1];
                const double cJ = rot[4 * J], sJr = rot[4 * J + 1], sJi = rot[4 * J + 2];
                jacobi_apply_m(rot[4 * I], rot[4 * I + 1], rot[4 * I + 2], cJ, sJr, sJi, m00, m01, m10, m11);
                jacobi_apply_v(cJ, sJr, sJi, v0p, v0q, v1p, v1q);
                if (I == J) { m01.re = m01.im = 0.0; m10.re = m10.im = 0.0; m00.im = 0.0; m11.im = 0.0; }
                const size_t ra = (size_t)jacobi_seat_rt(NB, 2 * I) * N, rb = (size_t)jacobi_seat_rt(NB, 2 * I + 1) * N;
                const int ca = jacobi_seat_rt(NB, 2 * J), cb = jacobi_seat_rt(NB, 2 * J + 1);
                Mn[ra + ca] = m00; Mn[ra + cb] = m01; Mn[rb + ca] = m10; Mn[rb + cb] = m11;
                const size_t va = (size_t)(2 * I) * N, vb = va + N;                  // eigenvector ROWS stay, columns move
                Vn[va + ca] = v0p; Vn[va + cb] = v0q; Vn[vb + ca] = v1p; Vn[vb + cb] = v1q;
            }
            __syncthreads();
            cplx* q = Mc; Mc = Mn; Mn = q; q = Vc; Vc = Vn; Vn = q;
        }
    }
    // (after whole sweeps the seats are the indices again)
    for (int k = t; k < N; k += NT) lam[k] = Mc[(size_t)k * N + k].re;
    __syncthreads();
    for (int k = t; k < N; k += NT) {               // rank of eigenvalue k in ascending order (stable)
        int rank = 0;
        for (int j = 0; j < N; ++j) rank += (lam[j] < lam[k]) || (lam[j] == lam[k] && j < k);
        pos[k] = rank;
        w_out[item * N + rank] = lam[k];
    }
    __syncthreads();
    if (v_out) {
        for (size_t idx = t; idx < NN; idx += NT) {
            const int r = (int)(idx / N), k = (int)(idx % N);
            const cplx v = Vc[idx];
            double* o = v_out + ((item * N + r) * N + pos[k]) * 2;
            o[0] = v.re; o[1] = v.im;
        }
    }
}

// ---- the same decomposition with ONE matrix spread over the chip: a cooperative launch (every workgroup resident),
// each workgroup takes a share of the 2 x 2 blocks of a round, computes the round's N/2 rotations for itself (they
// are cheap and every block needs two of them), and a grid-wide barrier separates the rounds.  One CU moves the
// 4 N^2 x 16 bytes of a round at ~85 GB/s; the chip moves them at L2 / HBM speed, so the barrier (a few microseconds)
// becomes the cost of a round.  hipLaunchCooperativeKernel refuses a grid that cannot be co-resident, in which case
// (or with fbx_set_option("eigh_cooperative", 0)) the single-workgroup kernel above takes over.
__global__ void __launch_bounds__(256)
eigh_coop_kernel(int N, const double* __restrict__ a, double* __restrict__ w_out, double* __restrict__ v_out,
                 cplx* __restrict__ work, double* __restrict__ partial) {
    namespace cg = cooperative_groups;
    cg::grid_group grid = cg::this_grid();
    constexpr int NT = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* rot = (double*)smem;                 // [N/2][4]
    double* red = rot + 2 * N;                   // [16]
    const int t = threadIdx.x, NB = N / 2, G = gridDim.x, g = blockIdx.x;
    const size_t NN = (size_t)N * N;
    cplx* M0 = work; cplx* M1 = M0 + NN; cplx* V0 = M1 + NN; cplx* V1 = V0 + NN;
    int nonfinite = 0;
    for (size_t idx = (size_t)g * NT + t; idx < NN; idx += (size_t)G * NT) {
        const int r = (int)(idx / N), c = (int)(idx % N);
        cplx h, v;
        if (r > c) { h.re = a[2 * idx]; h.im = a[2 * idx + 1]; }
        else if (r < c) { h.re = a[2 * ((size_t)c * N + r)]; h.im = -a[2 * ((size_t)c * N + r) + 1]; }
        else { h.re = a[2 * idx]; h.im = 0.0; }
        nonfinite |= !(isfinite(h.re) && isfinite(h.im));
        v.re = r == c ? 1.0 : 0.0; v.im = 0.0;
        M0[idx] = h; V0[idx] = v;
    }
    // a non-finite matrix gives NaN (include/fbx.h): every workgroup publishes what it saw in the slots of `partial` that
    // are next written by the ranks at the end (G <= N), and all of them leave together
    nonfinite = __syncthreads_or(nonfinite);
    if (t == 0) partial[2 * G + g] = nonfinite ? 1.0 : 0.0;
    grid.sync();
    nonfinite = 0;
    for (int k = 0; k < G; ++k) nonfinite |= partial[2 * G + k] != 0.0;
    if (nonfinite) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (size_t idx = (size_t)g * NT + t; idx < (size_t)N; idx += (size_t)G * NT) w_out[idx] = nan;
        if (v_out) for (size_t idx = (size_t)g * NT + t; idx < 2 * NN; idx += (size_t)G * NT) v_out[idx] = nan;
        return;
    }
    cplx *Mc = M0, *Mn = M1, *Vc = V0, *Vn = V1;
    for (int sweep = 0; sweep < FBX_JACOBI_MAX_SWEEPS; ++sweep) {
        double o2 = 0.0, n2 = 0.0;
        for (size_t idx = (size_t)g * NT + t; idx < NN; idx += (size_t)G * NT) {
            const cplx v = Mc[idx];
            const double a2 = v.re * v.re + v.im * v.im;
            n2 += a2;
            if (idx / N != idx % N) o2 += a2;
        }
        block_sum2<NT>(o2, n2, red);
        if (t == 0) { partial[2 * g] = o2; partial[2 * g + 1] = n2; }
        grid.sync();
        o2 = 0.0; n2 = 0.0;
        for (int k = 0; k < G; ++k) { o2 += partial[2 * k]; n2 += partial[2 * k + 1]; }      // same order in every workgroup
        grid.sync();                                  // `partial` is rewritten at the next sweep
        if (!(o2 > FBX_JACOBI_TOL2 * n2)) break;
        for (int r = 0; r < N - 1; ++r) {
            for (int p = t; p < NB; p += NT) {
                const cplx b = Mc[(size_t)(2 * p) * N + 2 * p + 1];
                const JRot q = jacobi_rotation(Mc[(size_t)(2 * p) * N + 2 * p].re, Mc[(size_t)(2 * p + 1) * N + 2 * p + 1].re, b.re, b.im);
                rot[4 * p] = q.c; rot[4 * p + 1] = q.sr; rot[4 * p + 2] = q.si;
            }
            __syncthreads();
            for (int blk = g * NT + t; blk < NB * NB; blk += G * NT) {
                const int I = blk / NB, J = blk % NB;
                const size_t r0 = (size_t)(2 * I) * N + 2 * J, r1 = r0 + N;
                cplx m00 = Mc[r0], m01 = Mc[r0 + 1], m10 = Mc[r1], m11 = Mc[r1 + 1];
                cplx v0p = Vc[r0], v0q = Vc[r0 + 1], v1p = Vc[r1], v1q = Vc[r1 + 1];
                const double cJ = rot[4 * J], sJr = rot[4 * J + 1], sJi = rot[4 * J + 2];
                jacobi_apply_m(rot[4 * I], rot[4 * I + 1], rot[4 * I + 2], cJ, sJr, sJi, m00, m01, m10, m11);
                jacobi_apply_v(cJ, sJr, sJi, v0p, v0q, v1p, v1q);
                if (I == J) { m01.re = m01.im = 0.0; m10.re = m10.im = 0.0; m00.im = 0.0; m11.im = 0.0; }
                const size_t ra = (size_t)jacobi_seat_rt(NB, 2 * I) * N, rb = (size_t)jacobi_seat_rt(NB, 2 * I + 1) * N;
                const int ca = jacobi_seat_rt(NB, 2 * J), cb = jacobi_seat_rt(NB, 2 * J + 1);
                Mn[ra + ca] = m00; Mn[ra + cb] = m01; Mn[rb + ca] = m10; Mn[rb + cb] = m11;
                const size_t va = (size_t)(2 * I) * N, vb = va + N;
                Vn[va + ca] = v0p; Vn[va + cb] = v0q; Vn[vb + ca] = v1p; Vn[vb + cb] = v1q;
            }
            grid.sync();
            cplx* q = Mc; Mc = Mn; Mn = q; q = Vc; Vc = Vn; Vn = q;
        }
    }
    // eigenvalues ascending, eigenvectors as columns in that order (ranks recomputed by every thread that needs one)
    for (size_t idx = (size_t)g * NT + t; idx < (size_t)N; idx += (size_t)G * NT) {
        const int k = (int)idx;
        const double lk = Mc[(size_t)k * N + k].re;
        int rank = 0;
        for (int j = 0; j < N; ++j) { const double lj = Mc[(size_t)j * N + j].re; rank += (lj < lk) || (lj == lk && j < k); }
        w_out[rank] = lk;
        partial[2 * G + k] = (double)rank;            // column k goes to column `rank`
    }
    grid.sync();
    if (v_out) {
        for (size_t idx = (size_t)g * NT + t; idx < NN; idx += (size_t)G * NT) {
            const int r = (int)(idx / N), k = (int)(idx % N);
            const cplx v = Vc[idx];
            double* o = v_out + ((size_t)r * N + (int)partial[2 * G + k]) * 2;
            o[0] = v.re; o[1] = v.im;
        }
    }
}

static int launch_eigh_coop(int N, int64_t B, const double* da, double* dw, double* dv, bool* done) {
    *done = false;
    if (!option_eigh_cooperative()) return FBX_OK;
    int dev = current_device(), coop = 0, cus = 0;
    if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, dev) != hipSuccess || !coop) { (void)hipGetLastError(); return FBX_OK; }
    FBX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const size_t lds = sizeof(double) * (2 * (size_t)N + 16);
    int per_cu = 0;
    FBX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, eigh_coop_kernel, 256, lds));
    if (per_cu < 1) return FBX_OK;
    const long long blocks_needed = ((long long)(N / 2) * (N / 2) + 255) / 256;
    long long G = std::min<long long>(blocks_needed, (long long)cus * std::min(per_cu, 2));
    if (G < 2) return FBX_OK;
    const size_t NN = (size_t)N * N;
    void* w = nullptr;
    { const int rc = workspace(WS_CONVERT, 4 * NN * sizeof(cplx) + sizeof(double) * (2 * (size_t)G + N), &w); if (rc) return rc; }
    cplx* work = (cplx*)w;
    double* partial = (double*)(work + 4 * NN);
    for (int64_t b = 0; b < B; ++b) {
        const double* a = da + b * NN * 2;
        double* wo = dw + b * N;
        double* vo = dv ? dv + b * NN * 2 : nullptr;
        int n_arg = N;
        void* args[] = {&n_arg, (void*)&a, (void*)&wo, (void*)&vo, (void*)&work, (void*)&partial};
        const hipError_t e = hipLaunchCooperativeKernel((const void*)eigh_coop_kernel, dim3((unsigned)G), dim3(256), args, (unsigned)lds, stream());
        if (e != hipSuccess) { (void)hipGetLastError(); if (b == 0) return FBX_OK; return hip_fail(e, "hipLaunchCooperativeKernel", __FILE__, __LINE__); }
    }
    *done = true;
    return FBX_OK;
}

static int launch_eigh_big(int N, int64_t B, const double* da, double* dw, double* dv) {
    const size_t lds = sizeof(double) * (2 * (size_t)N + N + 64) + sizeof(int) * N;
    const size_t per_item = 4 * (size_t)N * N * sizeof(cplx);
    const int64_t chunk = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 30) / per_item));
    void* w = nullptr;
    { const int rc = workspace(WS_CONVERT, per_item * (size_t)chunk, &w); if (rc) return rc; }
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = B - b0 < chunk ? B - b0 : chunk;
        hipLaunchKernelGGL(eigh_big_kernel, dim3((unsigned)nb), dim3(1024), lds, stream(), N, (long long)nb,
                           da + b0 * (size_t)N * N * 2, dw + b0 * N, dv ? dv + b0 * (size_t)N * N * 2 : nullptr, (cplx*)w);
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

// ---- out = op(A) diag(s) op(B) for stacks of N x N complex matrices, N up to 1024: the products around the large
// eigensolver (V f(lambda) V^H of sqrtm_psd, calculational.py:77-91; sqrt(rho) sigma sqrt(rho) of fidelity,
// distance_measures.py:64-84).  16 x 16 output tiles staged through LDS; a utility, not a tuned GEMM.
__global__ void __launch_bounds__(256)
matmul_kernel(int N, long long B, const double* __restrict__ a, int conj_t_a, const double* __restrict__ scale,
              const double* __restrict__ b, int conj_t_b, double* __restrict__ out) {
    __shared__ cplx As[16][17], Bs[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int tiles = (N + 15) / 16;
    const long long item = blockIdx.x / (tiles * tiles);
    const int tile = (int)(blockIdx.x % (tiles * tiles)), row0 = (tile / tiles) * 16, col0 = (tile % tiles) * 16;
    const double* pa = a + item * (long long)N * N * 2;
    const double* pb = b + item * (long long)N * N * 2;
    double re = 0.0, im = 0.0;
    for (int k0 = 0; k0 < N; k0 += 16) {
        {   // As[ty][tx] = op(A)[row0 + ty][k0 + tx] * s[k0 + tx];  Bs[ty][tx] = op(B)[k0 + ty][col0 + tx]
            const int r = row0 + ty, k = k0 + tx;
            cplx v; v.re = 0.0; v.im = 0.0;
            if (r < N && k < N) {
                const long long idx = conj_t_a ? (long long)k * N + r : (long long)r * N + k;
                v.re = pa[2 * idx]; v.im = conj_t_a ? -pa[2 * idx + 1] : pa[2 * idx + 1];
                if (scale) { const double sc = scale[item * N + k]; v.re *= sc; v.im *= sc; }
            }
            As[ty][tx] = v;
            const int kk = k0 + ty, c = col0 + tx;
            cplx w; w.re = 0.0; w.im = 0.0;
            if (kk < N && c < N) {
                const long long idx = conj_t_b ? (long long)c * N + kk : (long long)kk * N + c;
                w.re = pb[2 * idx]; w.im = conj_t_b ? -pb[2 * idx + 1] : pb[2 * idx + 1];
            }
            Bs[ty][tx] = w;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const cplx x = As[ty][k], y = Bs[k][tx];
            re += x.re * y.re - x.im * y.im;
            im += x.re * y.im + x.im * y.re;
        }
        __syncthreads();
    }
    const int r = row0 + ty, c = col0 + tx;
    if (r < N && c < N) {
        double* o = out + (item * (long long)N * N + (long long)r * N + c) * 2;
        o[0] = re; o[1] = im;
    }
}

template <int N>
static int launch_eigh(int64_t B, const double* da, double* dw, double* dv) {
    constexpr int NT = (N / 2) * (N / 2) > 64 ? (N / 2) * (N / 2) : 64;
    const size_t lds = 2 * sizeof(cplx) * sys_elems<N>() + sizeof(double) * (N + 64) + sizeof(int) * N;
    auto kern = eigh_kernel<N, NT>;
    FBX_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(NT), lds, stream(), (long long)B, da, dw, dv);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_matmul_dev(int N, int64_t B, const double* d_a, int conj_t_a, const double* d_scale, const double* d_b, int conj_t_b,
                   double* d_out) {
    FBX_REQUIRE(N >= 1 && N <= 1024, "fbx_matmul: N must be in 1..1024");
    FBX_REQUIRE(B >= 0 && (B == 0 || (d_a && d_b && d_out)), "fbx_matmul: bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long tiles = (N + 15) / 16;
    FBX_REQUIRE(B * tiles * tiles < (1LL << 31), "fbx_matmul: batch too large for one launch");
    hipLaunchKernelGGL(matmul_kernel, dim3((unsigned)(B * tiles * tiles)), dim3(256), 0, stream(), N, (long long)B, d_a, conj_t_a,
                       d_scale, d_b, conj_t_b, d_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_matmul(int N, int64_t B, const double* a, int conj_t_a, const double* scale, const double* b, int conj_t_b, double* out) {
    FBX_REQUIRE(N >= 1 && N <= 1024, "fbx_matmul: N must be in 1..1024");
    FBX_REQUIRE(B >= 0 && (B == 0 || (a && b && out)), "fbx_matmul: bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t nn = (size_t)N * N * 2 * B;
    HostIO io; double *da, *db, *ds = nullptr, *dout;
    FBX_TRY(io.in(a, nn, &da)); FBX_TRY(io.in(b, nn, &db));
    if (scale) FBX_TRY(io.in(scale, (size_t)N * B, &ds));
    FBX_TRY(io.out(out, nn, &dout));
    FBX_TRY(fbx_matmul_dev(N, B, da, conj_t_a, ds, db, conj_t_b, dout));
    return io.finish();
}

int fbx_eigh_dev(int N, int64_t B, const double* d_a, double* d_w_out, double* d_v_out) {
    FBX_REQUIRE(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64 || (N > 64 && N <= 1024 && N % 2 == 0),
                "fbx_eigh_dev: N must be a power of two in 2..64 or an even number in 66..1024");
    FBX_REQUIRE(B >= 0 && (B == 0 || (d_a && d_w_out)), "fbx_eigh: bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    if (N > 64) {
        // few large matrices: one at a time over the whole chip; many: one CU each
        // (measured: one CU per matrix 14 / 108 / 1270 / 9300 ms for N = 128 / 256 / 512 / 1024, whatever the batch up to
        // the number of CUs; the whole chip on one matrix 6 / 25 / 200 / 820 ms each)
        const int64_t coop_up_to = N >= 768 ? 10 : N >= 384 ? 5 : 3;
        if (N >= 128 && B <= coop_up_to) { bool done = false; FBX_TRY(launch_eigh_coop(N, B, d_a, d_w_out, d_v_out, &done)); if (done) return FBX_OK; }
        return launch_eigh_big(N, B, d_a, d_w_out, d_v_out);
    }
    switch (N) {
        case 2: FBX_TRY(launch_eigh<2>(B, d_a, d_w_out, d_v_out)); break;
        case 4: FBX_TRY(launch_eigh<4>(B, d_a, d_w_out, d_v_out)); break;
        case 8: FBX_TRY(launch_eigh<8>(B, d_a, d_w_out, d_v_out)); break;
        case 16: FBX_TRY(launch_eigh<16>(B, d_a, d_w_out, d_v_out)); break;
        case 32: FBX_TRY(launch_eigh<32>(B, d_a, d_w_out, d_v_out)); break;
        default: FBX_TRY(launch_eigh<64>(B, d_a, d_w_out, d_v_out)); break;
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_eigh(int N, int64_t B, const double* a, double* w_out, double* v_out) {
    FBX_REQUIRE(N >= 1 && N <= 1024, "fbx_eigh: N must be in 1..1024");
    FBX_REQUIRE(B >= 0 && (B == 0 || (a && w_out)), "fbx_eigh: bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    int Np = 2;
    while (Np < N) Np *= 2;
    if (N > 64) Np = N + (N & 1);           // the HBM-resident solver takes any even size
    if (Np == N) {
        const size_t nn = (size_t)N * N * 2 * B;
        HostIO io; double *da, *dw, *dv;
        FBX_TRY(io.in(a, nn, &da)); FBX_TRY(io.out(w_out, (size_t)N * B, &dw)); FBX_TRY(io.out_opt(v_out, nn, &dv));
        FBX_TRY(fbx_eigh_dev(N, B, da, dw, dv));
        return io.finish();
    }
    // Any other size (e.g. a qutrit's 3 x 3, a 9 x 9 Choi matrix): embedded in the next power of two
    // with zero rows / columns.  The padding coordinates are decoupled and stay so exactly (a pivot
    // with a zero off-diagonal entry gets the identity rotation), so their eigenvectors come back as
    // unit vectors on the padding coordinates and are dropped here; the rest is the decomposition
    // of the N x N matrix, still ascending.
    const size_t np2 = (size_t)Np * Np;
    std::vector<double> ap(np2 * 2 * B, 0.0), wp((size_t)Np * B), vp(np2 * 2 * B);
    for (int64_t b = 0; b < B; ++b)
        for (int r = 0; r < N; ++r)
            memcpy(&ap[(b * np2 + (size_t)r * Np) * 2], &a[((size_t)b * N * N + (size_t)r * N) * 2], sizeof(double) * 2 * N);
    {
        HostIO io; double *da, *dw, *dv;
        FBX_TRY(io.in(ap.data(), ap.size(), &da));
        FBX_TRY(io.out(wp.data(), wp.size(), &dw)); FBX_TRY(io.out(vp.data(), vp.size(), &dv));
        FBX_TRY(fbx_eigh_dev(Np, B, da, dw, dv));
        FBX_TRY(io.finish());
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t b = 0; b < B; ++b) {
        // a non-finite item came back all NaN (no column can be told from padding): NaN for that item, as for direct sizes
        bool nonfinite = false;
        for (int k = 0; k < Np && !nonfinite; ++k) nonfinite = std::isnan(wp[b * Np + k]);
        if (nonfinite) {
            for (int k = 0; k < N; ++k) w_out[b * N + k] = nan;
            if (v_out) for (size_t k = 0; k < (size_t)N * N * 2; ++k) v_out[(size_t)b * N * N * 2 + k] = nan;
            continue;
        }
        int kept = 0;
        for (int k = 0; k < Np; ++k) {
            bool padding = false;
            for (int r = N; r < Np && !padding; ++r) {
                const double* e = &vp[(b * np2 + (size_t)r * Np + k) * 2];
                padding = e[0] != 0.0 || e[1] != 0.0;
            }
            if (padding) continue;
            if (kept < N) {
                w_out[b * N + kept] = wp[b * Np + k];
                if (v_out)
                    for (int r = 0; r < N; ++r) {
                        v_out[((size_t)b * N * N + (size_t)r * N + kept) * 2] = vp[(b * np2 + (size_t)r * Np + k) * 2];
                        v_out[((size_t)b * N * N + (size_t)r * N + kept) * 2 + 1] = vp[(b * np2 + (size_t)r * Np + k) * 2 + 1];
                    }
            }
            ++kept;
        }
        if (kept != N) { set_error("fbx_eigh: internal error separating the padding of a non-power-of-two matrix"); return FBX_ERR_HIP; }
    }
    return FBX_OK;
}

// ---- choi2kraus for a batch (superoperator_transformations.py:325-336): fbx_eigh_dev + one assembling kernel.
// One workgroup per item.  Eigenpair k is kept when |lambda_k| > tol (the reference's test); its operator is
// sqrt(lambda_k) unvec(v_k) -- numpy's scimath square root, i sqrt(|lambda|) for a negative eigenvalue -- with the phase of v_k
// fixed so that its first component above 1e-12 ||v_k|| is real and positive (the convention of the host form this replaces,
// fbx/operator_tools/superoperator_transformations.py: what LAPACK hands the reference on the operators its tests compare
// entry by entry).  unvec is column stacking: K[r][c] = v[c d + r].  Kept operators are packed at the front of the item's D
// slots in ascending eigenvalue order (the order of the reference's list), the other slots are zeroed.
__global__ void __launch_bounds__(256)
kraus_assemble_kernel(int D, int d, long long B, const double* __restrict__ w, const double* __restrict__ V, double tol,
                      double* __restrict__ out, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char kraus_smem[];
    double* fre = (double*)kraus_smem;
    double* fim = fre + D;
    int* keep = (int*)(fim + D);
    int* pos = keep + D;
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const cplx* Vb = (const cplx*)V + (size_t)b * D * D;
    const double* wb = w + (size_t)b * D;
    for (int k = tid; k < D; k += 256) {
        const double ev = wb[k];
        const bool kp = fabs(ev) > tol;
        double fr = 0.0, fi = 0.0;
        if (kp) {
            double n2 = 0.0;
            for (int i = 0; i < D; ++i) { const cplx x = Vb[(size_t)i * D + k]; n2 = fma(x.re, x.re, fma(x.im, x.im, n2)); }
            const double thr = 1e-12 * sqrt(n2);
            double pr = 1.0, pi = 0.0;
            for (int i = 0; i < D; ++i) {
                const cplx x = Vb[(size_t)i * D + k];
                const double a = sqrt(fma(x.re, x.re, x.im * x.im));
                if (a > thr) { pr = x.re / a; pi = -x.im / a; break; }       // |x| / x
            }
            const double sq = sqrt(fabs(ev));
            if (ev >= 0.0) { fr = pr * sq; fi = pi * sq; } else { fr = -pi * sq; fi = pr * sq; }    // i (pr + i pi)
        }
        keep[k] = kp ? 1 : 0; fre[k] = fr; fim[k] = fi;
    }
    __syncthreads();
    for (int k = tid; k < D; k += 256) { int c = 0; for (int j = 0; j < k; ++j) c += keep[j]; pos[k] = c; }
    __syncthreads();
    const int total = pos[D - 1] + keep[D - 1];
    cplx* ob = (cplx*)out + (size_t)b * D * D;
    for (int idx = tid; idx < D * D; idx += 256) {
        const int i = idx / D, k = idx % D;                    // k fastest: coalesced reads of V[i][.]
        if (!keep[k]) continue;
        const cplx x = Vb[idx];
        const int r = i % d, c = i / d;
        cplx o; o.re = fre[k] * x.re - fim[k] * x.im; o.im = fre[k] * x.im + fim[k] * x.re;
        ob[((size_t)pos[k] * d + r) * d + c] = o;
    }
    for (int idx = total * D + tid; idx < D * D; idx += 256) { cplx z; z.re = 0.0; z.im = 0.0; ob[idx] = z; }
    if (tid == 0 && count) count[b] = total;
}

int fbx_choi2kraus_dev(int n_qubits, int64_t B, const double* d_choi, double tol, double* d_kraus_out, int32_t* d_count_out) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 5, "fbx_choi2kraus: n_qubits must be 1..5");
    FBX_REQUIRE(B >= 0 && (B == 0 || (d_choi && d_kraus_out)), "fbx_choi2kraus: bad batch / NULL buffer");
    FBX_REQUIRE(tol >= 0.0, "fbx_choi2kraus: negative tolerance");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const int d = 1 << n_qubits, D = d * d;
    // the eigenvectors of a block of items at a time: 16 MiB per 5-qubit item
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 28) / ((int64_t)D * D * 16)));
    DevBuf dw, dv;
    FBX_TRY(dw.alloc(sizeof(double) * D * (size_t)chunk));
    FBX_TRY(dv.alloc(sizeof(double) * 2 * D * D * (size_t)chunk));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(chunk, B - b0);
        FBX_TRY(fbx_eigh_dev(D, nb, d_choi + (size_t)b0 * D * D * 2, dw.as<double>(), dv.as<double>()));
        hipLaunchKernelGGL(kraus_assemble_kernel, dim3((unsigned)nb), dim3(256), (size_t)D * 24, stream(), D, d, (long long)nb,
                           dw.as<double>(), dv.as<double>(), tol, d_kraus_out + (size_t)b0 * D * D * 2,
                           d_count_out ? d_count_out + b0 : nullptr);
        FBX_HIP(hipGetLastError());
    }
    return FBX_OK;
}

int fbx_choi2kraus(int n_qubits, int64_t B, const double* choi, double tol, double* kraus_out, int32_t* count_out) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 5, "fbx_choi2kraus: n_qubits must be 1..5");
    FBX_REQUIRE(B >= 0 && (B == 0 || (choi && kraus_out)), "fbx_choi2kraus: bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t D = (size_t)1 << (2 * n_qubits), nn = D * D * 2 * (size_t)B;
    HostIO io; double *dc, *dk; int32_t* dn;
    FBX_TRY(io.in(choi, nn, &dc)); FBX_TRY(io.out(kraus_out, nn, &dk)); FBX_TRY(io.out(count_out, (size_t)B, &dn));
    FBX_TRY(fbx_choi2kraus_dev(n_qubits, B, dc, tol, dk, dn));
    return io.finish();
}

}  // extern "C"
