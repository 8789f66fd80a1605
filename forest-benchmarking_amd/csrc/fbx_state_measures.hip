// fbx_state_measures.hip -- what follows a state reconstruction, batched, on d x d (d = 2^n, n <= 5) matrices: the projection to the
// closest physical state, the state measures and the Pauli-Liouville vector.
//   1-3 qubits: one 64-lane wavefront per item (WaveTeam, the LDS of StateLds); lane t < d*d owns matrix entry (t / d, t % d).
//   4-5 qubits: one workgroup of (d/2)^2 threads -- the Jacobi solver's grid -- per item.
// The estimators are fbx_state.hip; what the two units share is fbx_state_core.hpp.
//
// Reference functions (file:line under forest/benchmarking/):
//   project_state_matrix_to_physical operator_tools/project_state_matrix.py:6-52
//   purity / fidelity / trace_distance / hilbert_schmidt_ip   distance_measures.py:14-114,198-216
//   computational2pauli_basis_matrix operator_tools/superoperator_transformations.py:413-424
#include "fbx_state_core.hpp"
#include <string>

namespace fbx {

// project_state_matrix.py:37-48 on the d eigenvalues `ev` in descending order: how many of them stay (each shifted by acc / that
// number; the others become zero), acc = the sum of those that go
__device__ __forceinline__ int spectrum_cut(const double* ev, int d, double& acc) {
    int i = d; acc = 0.0;
    while (i > 0 && ev[i - 1] + acc / (double)i < 0.0) { acc += ev[i - 1]; --i; }
    return i;
}

// a non-finite pair of states: NaN in every measure asked for
__device__ __forceinline__ void measures_nan(long long item, double* purity, double* fidelity, double* tdist, double* hsip) {
    if (purity) purity[item] = NAN;
    if (fidelity) fidelity[item] = NAN;
    if (tdist) tdist[item] = NAN;
    if (hsip) hsip[item] = NAN;
}

// project_state_matrix_to_physical, project_state_matrix.py:6-52
template <int NQ>
__global__ void __launch_bounds__(64)
proj_state_kernel(const double* __restrict__ rho_in, double* __restrict__ out) {
    constexpr int d = 1 << NQ, D = d * d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    StateLds<NQ> L; L.carve(smem, 1);
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    const bool act = lane < D;
    cplx v; v.re = 0.0; v.im = 0.0;
    if (act) { v.re = rho_in[(item * D + lane) * 2]; v.im = rho_in[(item * D + lane) * 2 + 1]; }
    double tr_re = (act && lane / d == lane % d) ? v.re : 0.0, tr_im = (act && lane / d == lane % d) ? v.im : 0.0;
    tr_re = wave_sum(tr_re); tr_im = wave_sum(tr_im);
    // A non-finite item gives NaN in every entry, as proj_state_big_kernel: the minimum below drops a NaN eigenvalue, and such an
    // item would pass for physical and come back with its finite entries in place.
    if (!(wave_sum(fabs(v.re) + fabs(v.im)) <= DBL_MAX)) {
        if (act) { out[(item * D + lane) * 2] = NAN; out[(item * D + lane) * 2 + 1] = NAN; }
        return;
    }
    const cplx q = div_by_trace(v, tr_re, tr_im);
    if (act) L.rho[lane] = q;
    FBX_WAVE_SYNC();
    // eigh (lower triangle, like scipy.linalg.eigh)
    constexpr int NB = d / 2;
    Blk h = blk_zero();
    if (lane < NB * NB) h = lower_blk<d>(L.rho, lane);
    sys_store<d>(L.Ms, lane, h);
    FBX_WAVE_SYNC();
    jacobi_eigh_lds<d>(L.Ms, L.Vs, L.rec, lane);
    __shared__ int physical;
    if (lane == 0) {
        double ev[d]; int idx[d];
        double mn = 1e300;
        for (int k = 0; k < d; ++k) { ev[k] = L.Ms[sys_index<d>(k, k)].re; idx[k] = k; mn = fmin(mn, ev[k]); }
        physical = mn >= 0.0;
        // descending order
        for (int a = 0; a < d; ++a) for (int b = a + 1; b < d; ++b)
            if (ev[b] > ev[a]) { double t = ev[a]; ev[a] = ev[b]; ev[b] = t; int u = idx[a]; idx[a] = idx[b]; idx[b] = u; }
        double acc;
        const int i = spectrum_cut(ev, d, acc);
        for (int j = 0; j < d; ++j) L.lam[idx[j]] = (j < i) ? ev[j] + acc / (double)i : 0.0;
    }
    FBX_WAVE_SYNC();
    cplx o = q;
    if (!physical) {
        const Blk pb = reconstruct_blk<d>(L.Vs, L.lam, lane);
        blk_store<d, d>(L.tmp, lane, pb);
        FBX_WAVE_SYNC();
        if (act) o = L.tmp[lane];
    }
    if (act) { out[(item * D + lane) * 2] = o.re; out[(item * D + lane) * 2 + 1] = o.im; }
}

// purity / fidelity / trace distance / Hilbert-Schmidt inner product
template <int NQ>
__global__ void __launch_bounds__(64)
state_measures_kernel(const double* __restrict__ rho_in, const double* __restrict__ sig_in,
                      double* __restrict__ purity, double* __restrict__ fidelity, double* __restrict__ tdist,
                      double* __restrict__ hsip) {
    constexpr int d = 1 << NQ, D = d * d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    StateLds<NQ> L; L.carve(smem, 1);
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    const WaveTeam<NQ> tm;
    const bool act = lane < D;
    cplx a, b; a.re = a.im = b.re = b.im = 0.0;
    if (act) {
        a.re = rho_in[(item * D + lane) * 2]; a.im = rho_in[(item * D + lane) * 2 + 1];
        b.re = sig_in[(item * D + lane) * 2]; b.im = sig_in[(item * D + lane) * 2 + 1];
        L.rho[lane] = a; L.U[lane] = b;
    }
    // A non-finite pair gives NaN in every output asked for, as state_measures_big_kernel: the column maximum of the trace
    // distance drops a NaN, and the clipped square roots of the fidelity turn NaN eigenvalues into zeros.
    if (!(wave_sum(fabs(a.re) + fabs(a.im) + fabs(b.re) + fabs(b.im)) <= DBL_MAX)) {
        if (lane == 0) measures_nan(item, purity, fidelity, tdist, hsip);
        return;
    }
    FBX_WAVE_SYNC();
    if (purity) {                                  // Re tr(rho rho)
        double p = 0.0;
        if (act) { const cplx t = L.rho[(lane % d) * d + lane / d]; p = a.re * t.re - a.im * t.im; }
        p = wave_sum(p);
        if (lane == 0) purity[item] = p;
    }
    if (hsip) {                                    // Re tr(A^H B)
        double p = act ? a.re * b.re + a.im * b.im : 0.0;
        p = wave_sum(p);
        if (lane == 0) hsip[item] = p;
    }
    if (tdist) {                                   // 0.5 * max_c sum_r |rho - sigma|[r][c]
        if (act) { const double dr = a.re - b.re, di = a.im - b.im; L.r[lane] = sqrt(dr * dr + di * di); }
        FBX_WAVE_SYNC();
        double cs = 0.0;
        if (lane < d) for (int r = 0; r < d; ++r) cs += L.r[r * d + lane];
        cs = wave_max(cs);
        if (lane == 0) tdist[item] = 0.5 * cs;
        FBX_WAVE_SYNC();
    }
    if (fidelity) {                                // (tr sqrtm_psd(sqrt_rho sigma sqrt_rho))^2
        herm_function<true>(tm, lane, L.rho, L.aux, 2, L);            // sqrt_rho
        const cplx t1 = team_matmul(tm, lane, L.aux, L.U);                // sqrt_rho sigma
        if (act) L.tmp[lane] = t1;
        FBX_WAVE_SYNC();
        const cplx t2 = team_matmul(tm, lane, L.tmp, L.aux);            // ... sqrt_rho
        FBX_WAVE_SYNC();
        if (act) L.tmp[lane] = t2;
        FBX_WAVE_SYNC();
        herm_function<true>(tm, lane, L.tmp, L.aux, 2, L);            // lam = sqrt(max(mu, 0))
        double s = (lane < d) ? L.lam[lane] : 0.0;
        s = wave_sum(s);
        if (lane == 0) fidelity[item] = s * s;
    }
}



}  // namespace fbx

using namespace fbx;

// ---- 4 and 5 qubits after the reconstruction: physical projection and state measures.  One workgroup of (d/2)^2 threads per
// item (one wavefront at 16 x 16, four at 32 x 32), thread t = (I, J) owns the 2 x 2 block of rows {2I, 2I+1} x columns
// {2J, 2J+1} -- the thread grid of the Jacobi solver, the one fbx_eigh runs at these sizes, so no thread idles through the
// eigensolves and the 16 x 16 solve needs no workgroup barrier.  Whole matrices stay in LDS buffers of PostBigLds<NQ>::MAT
// entries, each of which holds a matrix row-major or in the solver's block layout; the buffers are reused as the comments say.
template <int NQ>
struct PostBigLds {
    static constexpr int d = 1 << NQ, D = d * d, NB = d / 2, NT = NB * NB;
    static constexpr int MAT = sys_elems<d>() > D ? sys_elems<d>() : D;
    static constexpr int RED = 2 * (NT / 64) + 2;                      // block_sum2 scratch, then {shift, cut, physical}
    static constexpr size_t bytes(int mats) { return sizeof(cplx) * MAT * (size_t)mats + sizeof(double) * (2 * d + RED + 2); }
};
template <int NT>
__device__ __forceinline__ void post_sync() { if constexpr (NT > 64) __syncthreads(); else FBX_WAVE_SYNC(); }

// block t of A * Bm (row-major d x d)
template <int d>
__device__ __forceinline__ Blk matmul_blk(const cplx* A, const cplx* Bm, int t) {
    constexpr int NB = d / 2;
    const int I = t / NB, J = t % NB;
    Blk o = blk_zero();
#pragma unroll 8
    for (int k = 0; k < d; ++k) {
        const cplx a[2] = {A[(2 * I) * d + k], A[(2 * I + 1) * d + k]};
        const cplx b[2] = {Bm[k * d + 2 * J], Bm[k * d + 2 * J + 1]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o.re[e] += a[e >> 1].re * b[e & 1].re - a[e >> 1].im * b[e & 1].im;
            o.im[e] += a[e >> 1].re * b[e & 1].im + a[e >> 1].im * b[e & 1].re;
        }
    }
    return o;
}

// purity / fidelity / trace distance / Hilbert-Schmidt inner product as state_measures_kernel has them; an output whose pointer
// is NULL is skipped, and without the fidelity there is no eigensolve.  A non-finite pair gives NaN in every output asked for.
template <int NQ>
__global__ void __launch_bounds__(PostBigLds<NQ>::NT)
state_measures_big_kernel(const double* __restrict__ rho_in, const double* __restrict__ sig_in,
                          double* __restrict__ purity, double* __restrict__ fidelity, double* __restrict__ tdist,
                          double* __restrict__ hsip) {
    using P = PostBigLds<NQ>;
    constexpr int d = P::d, D = P::D, NT = P::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* X = (cplx*)smem;                   // |rho - sigma|, then the solver's matrix, then sqrt_rho
    cplx* Y = X + P::MAT;                    // rho, then the solver's eigenvectors, then sqrt_rho sigma
    cplx* Z = Y + P::MAT;                    // sigma, then sqrt_rho sigma sqrt_rho
    double* lam = (double*)(Z + P::MAT);
    double* red = lam + 2 * d;
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    const double* ra = rho_in + item * D * 2;
    const double* sb = sig_in + item * D * 2;
    double mag = 0.0, hs = 0.0;
    double* ad = (double*)X;
#pragma unroll
    for (int k = 0; k < D / NT; ++k) {
        const int idx = t + k * NT;
        cplx a, b;
        a.re = ra[2 * idx]; a.im = ra[2 * idx + 1]; b.re = sb[2 * idx]; b.im = sb[2 * idx + 1];
        Y[idx] = a; Z[idx] = b;
        mag += fabs(a.re) + fabs(a.im) + fabs(b.re) + fabs(b.im);
        hs += a.re * b.re + a.im * b.im;                                // Re tr(A^H B)
        const double dr = a.re - b.re, di = a.im - b.im;
        ad[idx] = sqrt(dr * dr + di * di);
    }
    block_sum2<NT>(mag, hs, red);                                       // (its barriers publish Y, Z and ad as well)
    post_sync<NT>();
    if (!(mag <= DBL_MAX)) {
        if (t == 0) measures_nan(item, purity, fidelity, tdist, hsip);
        return;
    }
    if (t == 0 && hsip) hsip[item] = hs;
    if (purity) {                                                       // Re tr(rho rho)
        double p = 0.0;
#pragma unroll
        for (int k = 0; k < D / NT; ++k) {
            const int idx = t + k * NT;
            const cplx a = Y[idx], at = Y[(idx % d) * d + idx / d];
            p += a.re * at.re - a.im * at.im;
        }
        p = block_sum<NT>(p, red);
        if (t == 0) purity[item] = p;
    }
    if (tdist) {                                                        // 0.5 * max_c sum_r |rho - sigma|[r][c]
        double cs = 0.0;
        if (t < d) for (int r = 0; r < d; ++r) cs += ad[r * d + t];
        if (t < 64) cs = wave_max(cs);                                  // d <= 32: the columns sit in the first wavefront
        if (t == 0) tdist[item] = 0.5 * cs;
    }
    if (!fidelity) return;
    // (tr sqrtm_psd(sqrt_rho sigma sqrt_rho))^2, both roots through the clipped spectrum
    Blk h = lower_blk<d>(Y, t);
    post_sync<NT>();                                                    // ad and rho are read: X and Y are free
    sys_store<d>(X, t, h);
    post_sync<NT>();
    jacobi_eigh_simple<d, NT>(X, Y, t, true, red);
    post_sync<NT>();
    if (t < d) { const double l = X[sys_index<d>(t, t)].re; lam[t] = sqrt(l > 0.0 ? l : 0.0); }
    post_sync<NT>();
    h = reconstruct_blk<d>(Y, lam, t);
    blk_store<d, d>(X, t, h);                                           // sqrt_rho
    post_sync<NT>();
    h = matmul_blk<d>(X, Z, t);
    blk_store<d, d>(Y, t, h);                                           // sqrt_rho sigma
    post_sync<NT>();
    h = matmul_blk<d>(Y, X, t);
    blk_store<d, d>(Z, t, h);                                           // ... sqrt_rho
    post_sync<NT>();
    h = lower_blk<d>(Z, t);
    sys_store<d>(X, t, h);
    post_sync<NT>();
    jacobi_eigh_simple<d, NT>(X, Y, t, true, red);
    post_sync<NT>();
    double s = 0.0;
    if (t < d) { const double l = X[sys_index<d>(t, t)].re; s = sqrt(l > 0.0 ? l : 0.0); }
    s = block_sum<NT>(s, red);
    if (t == 0) fidelity[item] = s * s;
}

// project_state_matrix_to_physical, project_state_matrix.py:6-52, as proj_state_kernel: a state that is physical after the
// division by its trace is written as divided, not rebuilt.  A non-finite item gives NaN in every entry.
template <int NQ>
__global__ void __launch_bounds__(PostBigLds<NQ>::NT)
proj_state_big_kernel(const double* __restrict__ rho_in, double* __restrict__ out) {
    using P = PostBigLds<NQ>;
    constexpr int d = P::d, D = P::D, NB = P::NB, NT = P::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* X = (cplx*)smem;                   // the solver's matrix
    cplx* Y = X + P::MAT;                    // rho / tr(rho), then the solver's eigenvectors
    double* lam = (double*)(Y + P::MAT);
    double* sorted = lam + d;
    double* red = sorted + d;
    const int t = threadIdx.x, I = t / NB, J = t % NB;
    const long long item = blockIdx.x;
    const double* ra = rho_in + item * D * 2;
    double* oa = out + item * D * 2;
    Blk q;
    double mag = 0.0, tr_re = 0.0, tr_im = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
        q.re[e] = ra[2 * (r * d + c)]; q.im[e] = ra[2 * (r * d + c) + 1];
        mag += fabs(q.re[e]) + fabs(q.im[e]);
        if (r == c) { tr_re += q.re[e]; tr_im += q.im[e]; }
    }
    block_sum2<NT>(tr_re, tr_im, red);
    mag = block_sum<NT>(mag, red);
    if (!(mag <= DBL_MAX)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
            oa[2 * (r * d + c)] = NAN; oa[2 * (r * d + c) + 1] = NAN;
        }
        return;
    }
    const double den = tr_re * tr_re + tr_im * tr_im;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double vr = q.re[e], vi = q.im[e];
        q.re[e] = (vr * tr_re + vi * tr_im) / den; q.im[e] = (vi * tr_re - vr * tr_im) / den;
    }
    post_sync<NT>();
    blk_store<d, d>(Y, t, q);
    post_sync<NT>();
    const Blk h = lower_blk<d>(Y, t);
    post_sync<NT>();
    sys_store<d>(X, t, h);
    post_sync<NT>();
    jacobi_eigh_simple<d, NT>(X, Y, t, true, red);
    post_sync<NT>();
    double ev = 0.0;
    if (t < d) { ev = X[sys_index<d>(t, t)].re; lam[t] = ev; }
    post_sync<NT>();
    int rank = 0;                                                       // place in descending order (stable)
    if (t < d) {
        for (int j = 0; j < d; ++j) rank += (lam[j] > ev) || (lam[j] == ev && j < t);
        sorted[rank] = ev;
    }
    post_sync<NT>();
    if (t == 0) {                                                       // project_state_matrix.py:37-48
        double acc;
        const int i = spectrum_cut(sorted, d, acc);
        red[0] = acc; red[1] = (double)i; red[2] = sorted[d - 1] >= 0.0 ? 1.0 : 0.0;
    }
    post_sync<NT>();
    const double acc = red[0];
    const int cut = (int)red[1];
    const bool physical = red[2] != 0.0;
    post_sync<NT>();
    if (t < d) lam[t] = rank < cut ? ev + acc / (double)cut : 0.0;
    post_sync<NT>();
    if (!physical) q = reconstruct_blk<d>(Y, lam, t);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
        oa[2 * (r * d + c)] = q.re[e]; oa[2 * (r * d + c) + 1] = q.im[e];
    }
}

// ---- Pauli-Liouville vector of a state: c2p vec(rho) = tr[P_k rho] / d, k in the order of
// itertools.product('IXYZ', repeat=n) (first letter = most significant qubit), the input of
// plotting/state_process.py:10-87 (computational2pauli_basis_matrix, superoperator_transformations.py:413-424).
// One thread per coefficient: P_k has one non-zero per row, P_k[i][i ^ x] = prod_q (I, X: 1; Y: -i / +i for row
// bit 0 / 1; Z: +1 / -1), so tr[P_k rho] = sum_i P_k[i][i ^ x] rho[i ^ x][i].
__global__ void __launch_bounds__(256)
pauli_vector_kernel(int n, long long total, const double* __restrict__ rho, double* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int d = 1 << n, DD = d * d;
    const long long item = gid / DD;
    const int k = (int)(gid % DD);
    int x = 0, z = 0, ny = 0;                   // X/Y positions, Z/Y positions, number of Y
    for (int q = 0; q < n; ++q) {
        const int op = (k >> (2 * (n - 1 - q))) & 3, bit = 1 << (n - 1 - q);
        if (op == 1 || op == 2) x |= bit;
        if (op == 2 || op == 3) z |= bit;
        ny += op == 2;
    }
    const double* r = rho + item * (long long)DD * 2;
    double re = 0.0, im = 0.0;
    for (int i = 0; i < d; ++i) {
        const int j = i ^ x;
        // Y on row bit b contributes -i (b = 0) or +i (b = 1) = -i * (-1)^b; Z contributes (-1)^b
        const double sgn = (__popc(i & z) & 1) ? -1.0 : 1.0;
        const double vr = r[2 * (j * d + i)], vi = r[2 * (j * d + i) + 1];
        re += sgn * vr; im += sgn * vi;
    }
    // times (-i)^ny
    double o;
    switch (ny & 3) { case 0: o = re; break; case 1: o = im; break; case 2: o = -re; break; default: o = -im; }
    out[gid] = o / d;
}

namespace {
// The argument checks of an entry point, shared by its device-pointer and its host-pointer form; *go = false for an empty batch.
// `buffers`: every required pointer is there.
int check_call(int n_qubits, const char* who, int64_t B, bool buffers, bool* go) {
    *go = false;
    FBX_REQUIRE(n_qubits >= 1 && n_qubits <= 5, std::string(who) + ": n_qubits must be 1..5");
    FBX_REQUIRE(B >= 0 && (B == 0 || buffers), std::string(who) + ": bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    *go = B > 0;
    return FBX_OK;
}
}  // namespace

extern "C" {

// Every entry point below comes as a device-pointer form (`_dev`: checks + launch on the library
// stream, no synchronisation) and a host-pointer form (staging buffers, H2D, the `_dev` form, D2H, sync).

int fbx_proj_state_physical_dev(int n_qubits, int64_t B, const double* d_rho, double* d_out) {
    bool go;
    FBX_TRY(check_call(n_qubits, "fbx_proj_state_physical", B, d_rho && d_out, &go));
    if (!go) return FBX_OK;
    return with_qubits(n_qubits, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if constexpr (NQ >= 4) return launch_lds(proj_state_big_kernel<NQ>, dim3((unsigned)B), dim3(PostBigLds<NQ>::NT), PostBigLds<NQ>::bytes(2), d_rho, d_out);
        else return launch_lds(proj_state_kernel<NQ>, dim3((unsigned)B), dim3(64), StateLds<NQ>::launch_bytes(1), d_rho, d_out);
    });
}

int fbx_proj_state_physical(int n_qubits, int64_t B, const double* rho, double* out) {
    bool go;
    FBX_TRY(check_call(n_qubits, "fbx_proj_state_physical", B, rho && out, &go));
    if (!go) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d;
    HostIO io; double *dr, *dout;
    FBX_TRY(io.in(rho, D * 2 * B, &dr)); FBX_TRY(io.out(out, D * 2 * B, &dout));
    FBX_TRY(fbx_proj_state_physical_dev(n_qubits, B, dr, dout));
    return io.finish();
}

int fbx_state_measures_dev(int n_qubits, int64_t B, const double* d_rho, const double* d_sigma, double* d_purity_out,
                           double* d_fidelity_out, double* d_trace_dist_out, double* d_hs_ip_out) {
    bool go;
    FBX_TRY(check_call(n_qubits, "fbx_state_measures", B, d_rho && d_sigma, &go));
    if (!go) return FBX_OK;
    return with_qubits(n_qubits, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if constexpr (NQ >= 4) return launch_lds(state_measures_big_kernel<NQ>, dim3((unsigned)B), dim3(PostBigLds<NQ>::NT), PostBigLds<NQ>::bytes(3),
                                                 d_rho, d_sigma, d_purity_out, d_fidelity_out, d_trace_dist_out, d_hs_ip_out);
        else return launch_lds(state_measures_kernel<NQ>, dim3((unsigned)B), dim3(64), StateLds<NQ>::launch_bytes(1), d_rho, d_sigma,
                               d_purity_out, d_fidelity_out, d_trace_dist_out, d_hs_ip_out);
    });
}

int fbx_state_measures(int n_qubits, int64_t B, const double* rho, const double* sigma, double* purity_out,
                       double* fidelity_out, double* trace_dist_out, double* hs_ip_out) {
    bool go;
    FBX_TRY(check_call(n_qubits, "fbx_state_measures", B, rho && sigma, &go));
    if (!go) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d;
    HostIO io; double *dr, *ds, *dp, *df, *dt, *dh;
    FBX_TRY(io.in(rho, D * 2 * B, &dr)); FBX_TRY(io.in(sigma, D * 2 * B, &ds));
    FBX_TRY(io.out_opt(purity_out, (size_t)B, &dp)); FBX_TRY(io.out_opt(fidelity_out, (size_t)B, &df));
    FBX_TRY(io.out_opt(trace_dist_out, (size_t)B, &dt)); FBX_TRY(io.out_opt(hs_ip_out, (size_t)B, &dh));
    FBX_TRY(fbx_state_measures_dev(n_qubits, B, dr, ds, dp, df, dt, dh));
    return io.finish();
}

int fbx_pauli_vector_dev(int n_qubits, int64_t B, const double* d_rho, double* d_out) {
    bool go;
    FBX_TRY(check_call(n_qubits, "fbx_pauli_vector", B, d_rho && d_out, &go));
    if (!go) return FBX_OK;
    const long long total = (long long)B << (2 * n_qubits);
    return launch_lds(pauli_vector_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, n_qubits, total, d_rho, d_out);
}

int fbx_pauli_vector(int n_qubits, int64_t B, const double* rho, double* out) {
    bool go;
    FBX_TRY(check_call(n_qubits, "fbx_pauli_vector", B, rho && out, &go));
    if (!go) return FBX_OK;
    const size_t DD = (size_t)1 << (2 * n_qubits);
    HostIO io; double *dr, *dout;
    FBX_TRY(io.in(rho, DD * 2 * B, &dr)); FBX_TRY(io.out(out, DD * B, &dout));
    FBX_TRY(fbx_pauli_vector_dev(n_qubits, B, dr, dout));
    return io.finish();
}

}  // extern "C"
