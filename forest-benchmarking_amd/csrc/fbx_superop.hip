// fbx_superop.hip -- batched superoperator algebra other than the representation changes (fbx_convert.hip) and the Kraus
// sweeps (fbx_sweep.hip): Choi projections, channel application, linear-inversion process estimates, Kraus bookkeeping, the
// Pauli twirl and the partial trace.  One 64-lane wavefront per item with its matrices staged in LDS, or one thread per entry.
//
// Reference functions (file:line under forest/benchmarking/):
//   operator_tools/project_superoperators.py:19-144          (CP / TP / TNI / physical)
//   operator_tools/apply_superoperator.py:60-90              (apply_choi_matrix_2_state)
#include "fbx_superop_prims.hpp"
#include <algorithm>

namespace fbx {

// ---------------------------------------------------------------------------------------------
// fbx_proj_choi
// ---------------------------------------------------------------------------------------------
template <int NQ>
__device__ __forceinline__ void proj_choi_body(char* smem, int kind, long long B, const double* __restrict__ in,
                                               double* __restrict__ out, int* __restrict__ iters_out) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1;
    char* p = smem;
    ChoiLds<NQ> L; L.carve(p);
    PhaseClock pc; pc.reset(); L.pc = &pc;
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    load_matrix<NQ>(in + item * (long long)D * D * 2, L.Mw, lane);
    __syncthreads();
    const Blk x = blk_load<D, LD>(L.Mw, lane);
    __syncthreads();
    // A non-finite item gives NaN in every entry and, for the Dykstra kinds, the count 1 (include/fbx.h): the eigensolver's
    // stopping test is false on a NaN or an infinite norm, so it would hand back the diagonal with the identity, and the CP
    // projection of a matrix with a NaN off its diagonal would be the finite max(diag, 0).  Nothing is projected.
    int nonfinite = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) nonfinite |= !(isfinite(x.re[e]) && isfinite(x.im[e]));
    if (__ballot(nonfinite) != 0) {                            // one wavefront per item
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        double* o = out + item * (long long)D * D * 2;
        for (int idx = lane; idx < 2 * D * D; idx += 64) o[idx] = nan;
        if (lane == 0 && iters_out) iters_out[item] = kind >= FBX_PROJ_PHYSICAL_TP ? 1 : 0;
        return;
    }
    int iters = 0, sweeps = 0;
    Blk y;
    if (kind == FBX_PROJ_CP) y = proj_cp_blk<NQ>(x, L, lane, sweeps);
    else if (kind == FBX_PROJ_TP) y = proj_tp_blk<NQ>(x, L, lane);
    else if (kind == FBX_PROJ_TNI) y = proj_tni_blk<NQ>(x, L, lane, sweeps);
    else y = proj_physical_blk<NQ>(x, kind == FBX_PROJ_PHYSICAL_TP, L, lane, iters, sweeps);
    __syncthreads();
    blk_store<D, LD>(L.Mw, lane, y);
    __syncthreads();
    store_matrix<NQ>(L.Mw, out + item * (long long)D * D * 2, lane);
    if (lane == 0 && iters_out) iters_out[item] = iters;
}
// one wavefront per SIMD (every register the Dykstra state wants: 324 for two qubits) ...
template <int NQ>
__global__ void __launch_bounds__(64)
proj_choi_kernel(int kind, long long B, const double* __restrict__ in, double* __restrict__ out, int* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    proj_choi_body<NQ>(smem, kind, B, in, out, iters_out);
}
// ... or two per SIMD (at most 256 registers) for batches that put several items on a SIMD anyway: two dependent
// Jacobi chains interleave, as in pgdb_lean_kernel.  Same arithmetic, same results.
template <int NQ>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
proj_choi_w2_kernel(int kind, long long B, const double* __restrict__ in, double* __restrict__ out, int* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    proj_choi_body<NQ>(smem, kind, B, in, out, iters_out);
}

// ---------------------------------------------------------------------------------------------
// apply_choi_matrix_2_state: out[o][o'] = sum_{i,i'} rho[i'][i] C[(i',o)][(i,o')]
// ---------------------------------------------------------------------------------------------
__global__ void apply_choi_kernel(int d, long long B, const double* __restrict__ choi,
                                  const double* __restrict__ rho, double* __restrict__ out) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int dd = d * d, D = dd;
    if (t >= B * dd) return;
    const long long item = t / dd;
    const int o = (int)(t % dd) / d, op = (int)(t % dd) % d;
    const double* C = choi + item * (long long)D * D * 2;
    const double* r = rho + item * (long long)dd * 2;
    double re = 0.0, im = 0.0;
    for (int ip = 0; ip < d; ++ip)
        for (int i = 0; i < d; ++i) {
            const double ar = r[2 * (ip * d + i)], ai = r[2 * (ip * d + i) + 1];
            const long long ci = ((long long)(ip * d + o) * D + (i * d + op)) * 2;
            const double br = C[ci], bi = C[ci + 1];
            re += ar * br - ai * bi; im += ar * bi + ai * br;
        }
    out[t * 2] = re; out[t * 2 + 1] = im;
}

// ---------------------------------------------------------------------------------------------
// linear_inv_process_estimate (tomography.py:459-491): R[i][:] = pinv(Abar_i) e_i, Choi by the
// inverse Pauli transform, plus the explicit identity term I_D / d (tomography.py:491)
// ---------------------------------------------------------------------------------------------
// ITEMS experiments per wavefront: a row of the block pseudo-inverses (540 x 16 doubles for two qubits, more than the
// L1 holds) is loaded once and used for all of them -- one experiment per wavefront ran at the L2's pace (6.8e7 /s).
// Every experiment's sums run over the same settings in the same order as before.
template <int NQ, int ITEMS>
__global__ void __launch_bounds__(64)
linv_process_kernel(DesignDev des, long long B, const double* __restrict__ expect, double* __restrict__ out) {
    constexpr int d = 1 << NQ, D = d * d, NB = D / 2, PER = (D * D + 63) / 64;
    __shared__ double Rb[D * D];
    __shared__ cplx Mw[D * (D + 1)];
    const int lane = threadIdx.x;
    const long long first = (long long)blockIdx.x * ITEMS;
    double acc[PER][ITEMS];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int idx = lane + 64 * u;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) acc[u][k] = 0.0;
        if (idx < D * D) {
            const int i = idx / D, j = idx % D;
            for (int g = des.pptr[i]; g < des.pptr[i + 1]; ++g) {
                const double p = des.pinvT[(size_t)g * D + j];
                const int col = des.porder[g];
#pragma unroll
                for (int k = 0; k < ITEMS; ++k)
                    if (first + k < B) acc[u][k] += expect[(first + k) * des.m + col] * p;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const long long item = first + k;
        if (item >= B) break;                                   // uniform
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = lane + 64 * u;
            if (idx < D * D) Rb[(idx % D) * D + idx / D] = acc[u][k] + ((idx == 0) ? 1.0 : 0.0);   // transposed, as pauli_real_to_choi_blk reads it
        }
        __syncthreads();
        const Blk c = pauli_real_to_choi_blk<NQ>(Rb, Mw, lane);
        if (lane < NB * NB) {
            const int I = lane / NB, J = lane % NB;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 2 * I + (e >> 1), col = 2 * J + (e & 1);
                double* o = out + ((item * D + row) * D + col) * 2;
                o[0] = c.re[e]; o[1] = c.im[e];
            }
        }
    }
}

}  // namespace fbx

namespace fbx {     // fbx_pgdb3.hip
int proj_choi3_launch(int kind, int64_t B, const double* d_in, double* d_out, int32_t* d_iters);
int linv_process3_launch(const fbx_design* des, int64_t B, const double* d_expect, double* d_out);
}

using namespace fbx;

// ---- Kraus bookkeeping for batches (operator_tools/compose_superoperators.py:7-44) and the Pauli twirl
// (channel_approximation.py:31-49).  Output operator p = j * K2 + l (the reference's list order: k1 outer,
// k2 inner) is kron(k2[l], k1[j]) for the tensor form, k2[l] . k1[j] for the composition; one output
// element per thread, inputs read through L2 (every input element is used K times).
namespace fbx {
__global__ void __launch_bounds__(256)
kraus_pairs_kernel(int tensor, long long B, int K2, int r2, int c2, int K1, int r1, int c1,
                   const cplx* __restrict__ k2, const cplx* __restrict__ k1, cplx* __restrict__ out) {
    const int ro = tensor ? r2 * r1 : r2, co = tensor ? c2 * c1 : c1;
    const long long per = (long long)K1 * K2 * ro * co, total = B * per;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / per;
        long long rem = idx - b * per;
        const int p = (int)(rem / ((long long)ro * co)); rem -= (long long)p * ro * co;
        const int r = (int)(rem / co), c = (int)(rem % co);
        const int j = p / K2, l = p % K2;
        const cplx* A = k2 + ((size_t)b * K2 + l) * r2 * c2;
        const cplx* Bm = k1 + ((size_t)b * K1 + j) * r1 * c1;
        cplx o; o.re = 0.0; o.im = 0.0;
        if (tensor) {
            const cplx x = A[(r / r1) * c2 + (c / c1)], y = Bm[(r % r1) * c1 + (c % c1)];
            o.re = x.re * y.re - x.im * y.im; o.im = x.re * y.im + x.im * y.re;
        } else {
            for (int t = 0; t < c2; ++t) {
                const cplx x = A[r * c2 + t], y = Bm[t * c1 + c];
                o.re += x.re * y.re - x.im * y.im; o.im += x.re * y.im + x.im * y.re;
            }
        }
        out[idx] = o;
    }
}
__global__ void __launch_bounds__(256)
twirl_kernel(long long B, int D, const cplx* __restrict__ chi, cplx* __restrict__ out) {
    const long long total = B * D * D;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(idx % ((long long)D * D));
        cplx o; o.re = 0.0; o.im = 0.0;
        if (e / D == e % D) o = chi[idx];
        out[idx] = o;
    }
}
}  // namespace fbx

// ---- partial trace of an operator on A (x) B (calculational.py:5-35 with two subsystems): keep = 0 traces out B,
// keep = 1 traces out A.  Any dimensions; one thread per output entry.
__global__ void __launch_bounds__(256)
partial_trace2_kernel(int da, int db, int keep, long long B, const double* __restrict__ in, double* __restrict__ out) {
    const int n = keep == 0 ? da : db, m = keep == 0 ? db : da;
    const long long N = (long long)da * db;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * n * n) return;
    const long long item = gid / ((long long)n * n);
    const int r = (int)((gid / n) % n), c = (int)(gid % n);
    const double* src = in + item * N * N * 2;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < m; ++k) {
        const long long row = keep == 0 ? (long long)r * db + k : (long long)k * db + r;
        const long long col = keep == 0 ? (long long)c * db + k : (long long)k * db + c;
        re += src[(row * N + col) * 2]; im += src[(row * N + col) * 2 + 1];
    }
    out[2 * gid] = re; out[2 * gid + 1] = im;
}

extern "C" {

// grid cap of the grid-strided one-thread-per-entry kernels
constexpr long long ENTRY_GRID = 256 * 32;

static int kraus_pairs_check(int tensor, int64_t B, int K2, int rows2, int cols2, int K1, int rows1, int cols1,
                             const void* k2, const void* k1, const void* out) {
    FBX_REQUIRE(B >= 0 && K1 >= 1 && K2 >= 1 && rows1 >= 1 && cols1 >= 1 && rows2 >= 1 && cols2 >= 1,
                "fbx_kraus_pairs: sizes must be positive");
    FBX_REQUIRE(tensor || cols2 == rows1, "fbx_kraus_pairs: composition needs cols(k2) == rows(k1)");
    FBX_REQUIRE(B == 0 || (k2 && k1 && out), "fbx_kraus_pairs: NULL buffer");
    return FBX_OK;
}

int fbx_kraus_pairs_dev(int tensor, int64_t B, int K2, int rows2, int cols2, int K1, int rows1, int cols1,
                        const double* d_k2, const double* d_k1, double* d_out) {
    FBX_TRY(kraus_pairs_check(tensor, B, K2, rows2, cols2, K1, rows1, cols1, d_k2, d_k1, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long ro = tensor ? (long long)rows2 * rows1 : rows2, co = tensor ? (long long)cols2 * cols1 : cols1;
    const long long total = (long long)B * K1 * K2 * ro * co, want = (total + 255) / 256;
    return launch_lds(kraus_pairs_kernel, dim3((unsigned)std::min(want, ENTRY_GRID)), dim3(256), 0,
                      tensor, B, K2, rows2, cols2, K1, rows1, cols1, (const cplx*)d_k2, (const cplx*)d_k1, (cplx*)d_out);
}

int fbx_kraus_pairs(int tensor, int64_t B, int K2, int rows2, int cols2, int K1, int rows1, int cols1,
                    const double* k2, const double* k1, double* out) {
    FBX_TRY(kraus_pairs_check(tensor, B, K2, rows2, cols2, K1, rows1, cols1, k2, k1, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n2 = (size_t)B * K2 * rows2 * cols2 * 2, n1 = (size_t)B * K1 * rows1 * cols1 * 2;
    const size_t ro = tensor ? (size_t)rows2 * rows1 : rows2, co = tensor ? (size_t)cols2 * cols1 : cols1;
    const size_t no = (size_t)B * K1 * K2 * ro * co * 2;
    HostIO io; double *d2, *d1, *dout;
    FBX_TRY(io.in(k2, n2, &d2)); FBX_TRY(io.in(k1, n1, &d1)); FBX_TRY(io.out(out, no, &dout));
    FBX_TRY(fbx_kraus_pairs_dev(tensor, B, K2, rows2, cols2, K1, rows1, cols1, d2, d1, dout));
    return io.finish();
}

static int pauli_twirl_chi_check(int64_t B, int D, const void* chi, const void* out) {
    FBX_REQUIRE(B >= 0 && D >= 1, "fbx_pauli_twirl_chi: bad size");
    FBX_REQUIRE(B == 0 || (chi && out), "fbx_pauli_twirl_chi: NULL buffer");
    return FBX_OK;
}

int fbx_pauli_twirl_chi_dev(int64_t B, int D, const double* d_chi, double* d_out) {
    FBX_TRY(pauli_twirl_chi_check(B, D, d_chi, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long total = (long long)B * D * D, want = (total + 255) / 256;
    return launch_lds(twirl_kernel, dim3((unsigned)std::min(want, ENTRY_GRID)), dim3(256), 0, B, D, (const cplx*)d_chi, (cplx*)d_out);
}

int fbx_pauli_twirl_chi(int64_t B, int D, const double* chi, double* out) {
    FBX_TRY(pauli_twirl_chi_check(B, D, chi, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t n = (size_t)B * D * D * 2;
    HostIO io; double *dc, *dout;
    FBX_TRY(io.in(chi, n, &dc)); FBX_TRY(io.out(out, n, &dout));
    FBX_TRY(fbx_pauli_twirl_chi_dev(B, D, dc, dout));
    return io.finish();
}

static int linv_process_check(const fbx_design* design, int64_t B, const void* expect, const void* choi_out) {
    FBX_TRY(check_design(design, "fbx_linv_process"));
    FBX_REQUIRE(design->dev.kind == FBX_KIND_PROCESS, "fbx_linv_process: needs a process design");
    FBX_REQUIRE(B >= 0 && (B == 0 || (expect && choi_out)), "fbx_linv_process: bad batch / NULL buffer");
    return FBX_OK;
}

int fbx_linv_process_dev(const fbx_design* design, int64_t B, const double* d_expect, double* d_choi_out) {
    FBX_TRY(linv_process_check(design, B, d_expect, d_choi_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const int n = design->dev.n;
    const dim3 grid((unsigned)((B + 3) / 4));
    if (n == 3) return linv_process3_launch(design, B, d_expect, d_choi_out);
    if (n == 1) return launch_lds(linv_process_kernel<1, 4>, grid, dim3(64), 0, design->dev, B, d_expect, d_choi_out);
    return launch_lds(linv_process_kernel<2, 4>, grid, dim3(64), 0, design->dev, B, d_expect, d_choi_out);
}

int fbx_linv_process(const fbx_design* design, int64_t B, const double* expect, double* choi_out) {
    FBX_TRY(linv_process_check(design, B, expect, choi_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t m = design->dev.m, D = design->dev.D;
    HostIO io; double *de, *dout;
    FBX_TRY(io.in(expect, m * B, &de)); FBX_TRY(io.out(choi_out, D * D * 2 * B, &dout));
    FBX_TRY(fbx_linv_process_dev(design, B, de, dout));
    return io.finish();
}

static int partial_trace_check(int dim_a, int dim_b, int keep, int64_t B, const void* in, const void* out) {
    FBX_REQUIRE(dim_a >= 1 && dim_b >= 1 && (long long)dim_a * dim_b <= 4096, "fbx_partial_trace: dimensions must be >= 1 with dim_a * dim_b <= 4096");
    FBX_REQUIRE(keep == 0 || keep == 1, "fbx_partial_trace: keep must be 0 (first subsystem) or 1 (second)");
    FBX_REQUIRE(B >= 0 && (B == 0 || (in && out)), "fbx_partial_trace: bad batch / NULL buffer");
    return FBX_OK;
}

int fbx_partial_trace_dev(int dim_a, int dim_b, int keep, int64_t B, const double* d_in, double* d_out) {
    FBX_TRY(partial_trace_check(dim_a, dim_b, keep, B, d_in, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const long long n = keep == 0 ? dim_a : dim_b, total = (long long)B * n * n;
    return launch_lds(partial_trace2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dim_a, dim_b, keep, B, d_in, d_out);
}

int fbx_partial_trace(int dim_a, int dim_b, int keep, int64_t B, const double* in, double* out) {
    FBX_TRY(partial_trace_check(dim_a, dim_b, keep, B, in, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t N = (size_t)dim_a * dim_b, n = keep == 0 ? dim_a : dim_b;
    HostIO io; double *d_in, *d_out;
    FBX_TRY(io.in(in, N * N * 2 * B, &d_in)); FBX_TRY(io.out(out, n * n * 2 * B, &d_out));
    FBX_TRY(fbx_partial_trace_dev(dim_a, dim_b, keep, B, d_in, d_out));
    return io.finish();
}

static int proj_choi_check(int proj_kind, int n_qubits, int64_t B, const void* choi, const void* out) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 3, "fbx_proj_choi: n_qubits must be 1..3");
    FBX_REQUIRE(B >= 0 && (B == 0 || (choi && out)), "fbx_proj_choi: bad batch / NULL buffer");
    FBX_REQUIRE(proj_kind >= FBX_PROJ_CP && proj_kind <= FBX_PROJ_PHYSICAL_TNI, "fbx_proj_choi: bad projection kind");
    return FBX_OK;
}

int fbx_proj_choi_dev(int proj_kind, int n_qubits, int64_t B, const double* d_choi, double* d_out, int32_t* d_iters_out) {
    FBX_TRY(proj_choi_check(proj_kind, n_qubits, B, d_choi, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const dim3 grid((unsigned)B), block(64);
    if (n_qubits == 3) return proj_choi3_launch(proj_kind, B, d_choi, d_out, d_iters_out);
    if (n_qubits == 1) return launch_lds(proj_choi_kernel<1>, grid, block, ChoiLds<1>::bytes() + 64, proj_kind, B, d_choi, d_out, d_iters_out);
    return launch_lds(B >= 2048 ? proj_choi_w2_kernel<2> : proj_choi_kernel<2>, grid, block, ChoiLds<2>::bytes() + 64, proj_kind, B, d_choi, d_out, d_iters_out);
}

int fbx_proj_choi(int proj_kind, int n_qubits, int64_t B, const double* choi, double* out, int32_t* iters_out) {
    FBX_TRY(proj_choi_check(proj_kind, n_qubits, B, choi, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d, nm = D * D * 2 * B;
    HostIO io; double *d_in, *d_out; int32_t* d_it;
    FBX_TRY(io.in(choi, nm, &d_in)); FBX_TRY(io.out(out, nm, &d_out)); FBX_TRY(io.out(iters_out, (size_t)B, &d_it));
    FBX_TRY(fbx_proj_choi_dev(proj_kind, n_qubits, B, d_in, d_out, d_it));
    return io.finish();
}

static int apply_choi_check(int n_qubits, int64_t B, const void* choi, const void* rho, const void* out) {
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 3, "fbx_apply_choi: n_qubits must be 1..3");
    FBX_REQUIRE(B >= 0 && (B == 0 || (choi && rho && out)), "fbx_apply_choi: bad batch / NULL buffer");
    return FBX_OK;
}

int fbx_apply_choi_dev(int n_qubits, int64_t B, const double* d_choi, const double* d_rho, double* d_out) {
    FBX_TRY(apply_choi_check(n_qubits, B, d_choi, d_rho, d_out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d;
    const long long total = (long long)B * D;
    return launch_lds(apply_choi_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (int)d, B, d_choi, d_rho, d_out);
}

int fbx_apply_choi(int n_qubits, int64_t B, const double* choi, const double* rho, double* out) {
    FBX_TRY(apply_choi_check(n_qubits, B, choi, rho, out));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d;
    HostIO io; double *dc, *dr, *dout;
    FBX_TRY(io.in(choi, D * D * 2 * B, &dc)); FBX_TRY(io.in(rho, D * 2 * B, &dr)); FBX_TRY(io.out(out, D * 2 * B, &dout));
    FBX_TRY(fbx_apply_choi_dev(n_qubits, B, dc, dr, dout));
    return io.finish();
}

}  // extern "C"
