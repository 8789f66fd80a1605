// fbx_chernoff.hip -- batched quantum Chernoff bound of pairs of states, with a certified lower bound
// (distance_measures.py:153-195).
//
// With rho = V diag(a) V^H, sigma = W diag(b) W^H (lower triangles read, as fbx_eigh and numpy do) and O_ij = |<v_i|w_j>|^2:
//     Q(s) = tr(rho^s sigma^(1-s)) = sum_ij O_ij a_i^s b_j^(1-s),   qcb = min over s in [0, 1] of Q(s).
// An eigenvalue <= zero_tol * lambda_max of its own matrix (negative ones included) is exactly zero and its terms are left out
// at every s, the endpoints included (support projectors: Q is continuous on [0, 1]).  Every kept term is
// O_ij b_j exp(s ln(a_i / b_j)), so Q is convex; with g_ij = ln a_i - ln b_j, Q' = sum t_ij g_ij and Q'' = sum t_ij g_ij^2.
//
// Search (chernoff_search): Q, Q', Q'' at s = 0 and 1; the minimum is at 0 when Q'(0) >= 0 and at 1 when Q'(1) <= 0, otherwise
// a safeguarded Newton iteration on Q' inside the bracket [l, r] (bisection when a Newton step leaves the bracket or does not
// halve the step before it).  qcb is the smallest evaluated Q and s its point.  Lower bound: a tangent of a convex function lies
// below it, so for the tangents T_l, T_r at the two bracket ends and any lam in [0, 1], min over t in {0, 1} of
// lam T_l(t) + (1 - lam) T_r(t) <= min_t max(T_l, T_r) <= min Q.  lam in {0, 1, the lam that makes the combined slope zero} are
// tried and the largest kept: the bound holds for any two evaluated points whatever the signs of the computed derivatives.
// Against rounding each tangent is lowered by (2 e0 + e1) Q(p) + 4 u (Q(p) + |Q'(p)|) (u = 2^-52), with
//     e0 = u (8 L + 16 + n_terms)        relative error of Q (per term exp / log / product, L = max over kept terms |ln a| + |ln b|)
//     e1 = (1 + 2 e0) (G e0 + 4 u L)    error of Q' per unit Q (G = max |g|; the error of g itself is the 4 u L part)
// and |t - p| <= 1 bounds the slope error's effect.  Stop: qcb - lower <= tol * max(qcb, 1e-12), or max_iters evaluations.
//
// 1-3 qubits (chernoff_kernel<NQ>): one wavefront per pair, both matrices diagonalised in LDS by jacobi_eigh_lds<d>, O formed one
// entry per lane; ln a_i, ln b_j, O_ij and the mask stay in registers and each evaluation is one pass with three wave_sums.
// 4-5 qubits: a composition -- chernoff_stage_kernel (copies the pair into one stack, a shared sigma once per item, non-finite
// items zeroed and flagged), fbx_eigh_dev over the stack, fbx_matmul_dev (V^H W) and chernoff_search_kernel<NQ> (one 256-thread
// workgroup per pair over the d^2 terms, the same search routine with a workgroup reduction).  Items never interact.
#include "fbx_eigh.hpp"
#include <cfloat>

namespace fbx {
namespace {

constexpr int CHERNOFF_BIG_NT = 256;          // 4-5 qubits: threads per pair
constexpr int64_t CHERNOFF_BIG_CHUNK = 4096;  // 4-5 qubits: pairs per pass through the workspace
constexpr double CHERNOFF_U = DBL_EPSILON;

// three sums (Q, Q', Q'') and a maximum, over one wavefront
struct WaveRed {
    __device__ void sum3(double& a, double& b, double& c) const { a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); }
    __device__ double max(double v) const { return wave_max(v); }
};
// the same over a workgroup of NT threads; `red` holds 3 NT / 64 doubles of LDS.  Every thread gets the same values, summed in one
// fixed order.
template <int NT>
struct BlockRed {
    static constexpr int NW = NT / 64;
    double* red;
    __device__ void sum3(double& a, double& b, double& c) const {
        a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
        const int w = threadIdx.x >> 6;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) { red[w] = a; red[NW + w] = b; red[2 * NW + w] = c; }
        __syncthreads();
        a = b = c = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { a += red[k]; b += red[NW + k]; c += red[2 * NW + k]; }
    }
    __device__ double max(double v) const {
        v = wave_max(v);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        double m = red[0];
#pragma unroll
        for (int k = 1; k < NW; ++k) m = fmax(m, red[k]);
        return m;
    }
};

struct ChernoffResult { double qcb, lower, s; int iters; };

// The search of the header comment over the terms this thread holds (TPT per thread; a left-out term has ov = la = lb = 0).
// Every quantity that steers control flow comes out of `red`, so every branch is uniform across the wavefront / workgroup.
template <int TPT, class Red>
__device__ ChernoffResult chernoff_search(const double (&la)[TPT], const double (&lb)[TPT], const double (&ov)[TPT], int n_terms,
                                          double tol, int max_iters, const Red& red) {
    constexpr double u = CHERNOFF_U;
    double lm = 0.0, gm = 0.0;
#pragma unroll
    for (int k = 0; k < TPT; ++k)
        if (ov[k] > 0.0) { lm = fmax(lm, fabs(la[k]) + fabs(lb[k])); gm = fmax(gm, fabs(la[k] - lb[k])); }
    lm = red.max(lm);
    gm = red.max(gm);
    const double e0 = u * (8.0 * lm + 16.0 + n_terms);
    const double e1 = (1.0 + 2.0 * e0) * (gm * e0 + 4.0 * u * lm);

    auto eval = [&](double s, double& q, double& dq, double& h) {
        q = 0.0; dq = 0.0; h = 0.0;
        const double s1 = 1.0 - s;
#pragma unroll
        for (int k = 0; k < TPT; ++k) {
            const double t = ov[k] * exp(s * la[k] + s1 * lb[k]);
            const double g = la[k] - lb[k];
            q += t; dq += t * g; h += t * g * g;
        }
        red.sum3(q, dq, h);
    };
    // the tangent at p, lowered against rounding: its values at t = 0 and t = 1
    auto tangent = [&](double p, double q, double dq, double& v0, double& v1) {
        const double c = q - ((2.0 * e0 + e1) * q + 4.0 * u * (q + fabs(dq)));
        v0 = c - dq * p;
        v1 = c + dq * (1.0 - p);
    };
    auto bound = [&](double l0, double l1, double ml, double r0, double r1, double mr) {
        double b = fmax(fmin(l0, l1), fmin(r0, r1));                   // lam = 1, lam = 0
        if (ml < 0.0 && mr > 0.0) {                                    // lam with combined slope zero
            const double lam = mr / (mr - ml), mu = 1.0 - lam;
            const double v = fmin(lam * l0 + mu * r0, lam * l1 + mu * r1) - 4.0 * u * (fabs(l0) + fabs(r0) + fabs(l1) + fabs(r1));
            b = fmax(b, v);
        }
        return b;
    };

    ChernoffResult o;
    double q0, d0, h0, q1, d1, h1;
    eval(0.0, q0, d0, h0);
    eval(1.0, q1, d1, h1);
    o.qcb = q0; o.s = 0.0;
    if (q1 < q0) { o.qcb = q1; o.s = 1.0; }
    double l = 0.0, ql = q0, dl = d0, r = 1.0, qr = q1, dr = d1;
    double l0, l1, r0, r1;
    tangent(l, ql, dl, l0, l1);
    tangent(r, qr, dr, r0, r1);
    o.lower = bound(l0, l1, dl, r0, r1, dr);
    int it = 0;
    if (!(o.qcb - o.lower <= tol * fmax(o.qcb, 1e-12)) && dl < 0.0 && dr > 0.0) {
        double x = q0 <= q1 ? 0.0 : 1.0, xd = q0 <= q1 ? d0 : d1, xh = q0 <= q1 ? h0 : h1;
        double step = 1.0, step_old = 1.0;
        while (it < max_iters) {
            double xn = x - xd / xh;
            if (!(xh > 0.0 && xn > l && xn < r && 2.0 * fabs(xd) <= fabs(step_old * xh))) xn = 0.5 * (l + r);   // bisection
            if (!(xn > l && xn < r)) break;                            // the bracket is exhausted at working precision
            step_old = step; step = xn - x;
            double qn, dn, hn;
            eval(xn, qn, dn, hn);
            ++it;
            if (qn < o.qcb) { o.qcb = qn; o.s = xn; }
            if (dn < 0.0) { l = xn; ql = qn; dl = dn; }
            else if (dn > 0.0) { r = xn; qr = qn; dr = dn; }
            else { l = r = xn; ql = qr = qn; dl = dr = 0.0; }
            tangent(l, ql, dl, l0, l1);
            tangent(r, qr, dr, r0, r1);
            o.lower = fmax(o.lower, bound(l0, l1, dl, r0, r1, dr));
            if (o.qcb - o.lower <= tol * fmax(o.qcb, 1e-12) || dn == 0.0) break;
            x = xn; xd = dn; xh = hn;
        }
    }
    // lower <= exact minimum holds; when it exceeds qcb, qcb is below the exact minimum too and serves as the bound
    o.lower = fmin(o.lower, o.qcb);
    o.iters = (o.qcb - o.lower <= tol * fmax(o.qcb, 1e-12)) ? it : -(it > 0 ? it : 1);
    return o;
}

// the Hermitian matrix of the lower triangle of row-major d x d `src` (numpy's eigh), block `lane`; |entries| summed into `mag`
template <int d>
__device__ __forceinline__ Blk load_lower(const double* __restrict__ src, int lane, double& mag) {
    constexpr int NB = d / 2;
    Blk h = blk_zero();
    if (lane < NB * NB) {
        const int I = lane / NB, J = lane % NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 2 * I + (e >> 1), c = 2 * J + (e & 1);
            const int rr = r >= c ? r : c, cc = r >= c ? c : r;
            const double re = src[2 * (rr * d + cc)], im = src[2 * (rr * d + cc) + 1];
            h.re[e] = re;
            h.im[e] = r > c ? im : r < c ? -im : 0.0;
            mag += fabs(re) + fabs(im);
        }
    }
    return h;
}

__device__ __forceinline__ void write_result(long long item, const ChernoffResult& o, double* qcb_out, double* lower_out,
                                             double* s_out, int32_t* iters_out) {
    qcb_out[item] = o.qcb;
    if (lower_out) lower_out[item] = o.lower;
    if (s_out) s_out[item] = o.s;
    if (iters_out) iters_out[item] = o.iters;
}
__device__ __forceinline__ ChernoffResult nan_result() {
    ChernoffResult o; o.qcb = NAN; o.lower = NAN; o.s = NAN; o.iters = -1; return o;
}

template <int NQ>
__global__ void __launch_bounds__(64)
chernoff_kernel(long long B, const double* __restrict__ rho, const double* __restrict__ sigma, int shared, double tol, int max_iters,
                double zero_tol, double* __restrict__ qcb_out, double* __restrict__ lower_out, double* __restrict__ s_out,
                int32_t* __restrict__ iters_out) {
    constexpr int d = 1 << NQ, DD = d * d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx* Ma = (cplx*)smem;
    cplx* Va = Ma + sys_elems<d>();
    cplx* Mb = Va + sys_elems<d>();
    cplx* Vb = Mb + sys_elems<d>();
    const int lane = threadIdx.x;
    const int i = lane / d, j = lane % d;
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        double mag = 0.0;
        const Blk ha = load_lower<d>(rho + item * DD * 2, lane, mag);
        const Blk hb = load_lower<d>(sigma + (shared ? 0 : item * DD * 2), lane, mag);
        mag = wave_sum(mag);
        if (!(mag <= DBL_MAX)) {                                        // non-finite input: NaN for this item only
            if (lane == 0) write_result(item, nan_result(), qcb_out, lower_out, s_out, iters_out);
            continue;
        }
        FBX_WAVE_SYNC();
        sys_store<d>(Ma, lane, ha);
        sys_store<d>(Mb, lane, hb);
        FBX_WAVE_SYNC();
        jacobi_eigh_lds<d>(Ma, Va, nullptr, lane);
        jacobi_eigh_lds<d>(Mb, Vb, nullptr, lane);
        FBX_WAVE_SYNC();
        double amax = -INFINITY, bmax = -INFINITY;
#pragma unroll
        for (int k = 0; k < d; ++k) {
            amax = fmax(amax, Ma[sys_index<d>(k, k)].re);
            bmax = fmax(bmax, Mb[sys_index<d>(k, k)].re);
        }
        double la[1] = {0.0}, lb[1] = {0.0}, ov[1] = {0.0};
        if (lane < DD) {
            const double a = Ma[sys_index<d>(i, i)].re, b = Mb[sys_index<d>(j, j)].re;
            double re = 0.0, im = 0.0;                                  // <v_i|w_j>
#pragma unroll
            for (int k = 0; k < d; ++k) {
                const cplx v = Va[sys_index<d>(k, i)], w = Vb[sys_index<d>(k, j)];
                re += v.re * w.re + v.im * w.im;
                im += v.re * w.im - v.im * w.re;
            }
            const double o = re * re + im * im;
            if (a > 0.0 && a > zero_tol * amax && b > 0.0 && b > zero_tol * bmax && o > 0.0) {
                la[0] = log(a); lb[0] = log(b); ov[0] = o;
            }
        }
        const ChernoffResult res = chernoff_search<1>(la, lb, ov, DD, tol, max_iters, WaveRed{});
        if (lane == 0) write_result(item, res, qcb_out, lower_out, s_out, iters_out);
    }
}

// 4-5 qubits, stage: stack[c] = rho[first + c], stack[n + c] = sigma (shared or per item); a non-finite pair is zeroed and flagged
template <int NQ>
__global__ void __launch_bounds__(CHERNOFF_BIG_NT)
chernoff_stage_kernel(long long n, long long first, const double* __restrict__ rho, const double* __restrict__ sigma, int shared,
                      double* __restrict__ stack, int* __restrict__ bad) {
    constexpr int d = 1 << NQ, E = d * d * 2;
    __shared__ double red[CHERNOFF_BIG_NT / 64];
    const long long c = blockIdx.x, item = first + c;
    const double* ra = rho + item * E;
    const double* sb = sigma + (shared ? 0 : item * E);
    double mag = 0.0;
    for (int k = threadIdx.x; k < E; k += CHERNOFF_BIG_NT) mag += fabs(ra[k]) + fabs(sb[k]);
    mag = block_sum<CHERNOFF_BIG_NT>(mag, red);
    const bool ok = mag <= DBL_MAX;
    for (int k = threadIdx.x; k < E; k += CHERNOFF_BIG_NT) {
        stack[c * E + k] = ok ? ra[k] : 0.0;
        stack[(n + c) * E + k] = ok ? sb[k] : 0.0;
    }
    if (threadIdx.x == 0) bad[c] = ok ? 0 : 1;
}

// 4-5 qubits, search: w[2n][d] ascending eigenvalues (rho items first), m[n][d][d] = V^H W
template <int NQ>
__global__ void __launch_bounds__(CHERNOFF_BIG_NT)
chernoff_search_kernel(long long n, long long first, const double* __restrict__ w, const double* __restrict__ m,
                       const int* __restrict__ bad, double tol, int max_iters, double zero_tol, double* __restrict__ qcb_out,
                       double* __restrict__ lower_out, double* __restrict__ s_out, int32_t* __restrict__ iters_out) {
    constexpr int d = 1 << NQ, DD = d * d, TPT = DD / CHERNOFF_BIG_NT;
    __shared__ double red[3 * CHERNOFF_BIG_NT / 64];
    const long long c = blockIdx.x, item = first + c;
    if (bad[c]) {                                                       // uniform across the workgroup
        if (threadIdx.x == 0) write_result(item, nan_result(), qcb_out, lower_out, s_out, iters_out);
        return;
    }
    const double* wa = w + c * d;
    const double* wb = w + (n + c) * d;
    const double amax = wa[d - 1], bmax = wb[d - 1];
    double la[TPT], lb[TPT], ov[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const int idx = threadIdx.x + k * CHERNOFF_BIG_NT, i = idx / d, j = idx % d;
        const double a = wa[i], b = wb[j];
        const double re = m[(c * DD + idx) * 2], im = m[(c * DD + idx) * 2 + 1];
        const double o = re * re + im * im;
        la[k] = 0.0; lb[k] = 0.0; ov[k] = 0.0;
        if (a > 0.0 && a > zero_tol * amax && b > 0.0 && b > zero_tol * bmax && o > 0.0) { la[k] = log(a); lb[k] = log(b); ov[k] = o; }
    }
    const ChernoffResult res = chernoff_search<TPT>(la, lb, ov, DD, tol, max_iters, BlockRed<CHERNOFF_BIG_NT>{red});
    if (threadIdx.x == 0) write_result(item, res, qcb_out, lower_out, s_out, iters_out);
}

static_assert((1 << 8) % CHERNOFF_BIG_NT == 0 && (1 << 10) % CHERNOFF_BIG_NT == 0, "4-5 qubits: whole terms per thread");

template <int NQ>
int launch_small(int64_t B, const double* rho, const double* sigma, int shared, double tol, int max_iters, double zero_tol,
                 double* qcb, double* lower, double* s, int32_t* iters) {
    constexpr int d = 1 << NQ;
    const long long grid = B < (1LL << 20) ? B : (1LL << 20);
    const size_t lds = sizeof(cplx) * 4 * sys_elems<d>();
    hipLaunchKernelGGL(chernoff_kernel<NQ>, dim3((unsigned)grid), dim3(64), lds, stream(), (long long)B, rho, sigma, shared, tol,
                       max_iters, zero_tol, qcb, lower, s, iters);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

template <int NQ>
int launch_big(int64_t B, const double* rho, const double* sigma, int shared, double tol, int max_iters, double zero_tol,
               double* qcb, double* lower, double* s, int32_t* iters) {
    constexpr int d = 1 << NQ;
    constexpr size_t DD = (size_t)d * d;
    const int64_t chunk = B < CHERNOFF_BIG_CHUNK ? B : CHERNOFF_BIG_CHUNK;
    // workspace of one pass (stream-ordered reuse from pass to pass): stack and eigenvectors [2 chunk][d][d], eigenvalues
    // [2 chunk][d], V^H W [chunk][d][d], flags [chunk]
    const size_t mat = sizeof(double) * 2 * DD;
    const size_t bytes = mat * (2 * chunk) * 2 + sizeof(double) * d * (2 * chunk) + mat * chunk + sizeof(int) * chunk;
    void* p = nullptr;
    FBX_TRY(workspace(WS_CHERNOFF, bytes, &p));
    char* q = (char*)p;
    double* stack = (double*)q; q += mat * (2 * chunk);
    double* vecs = (double*)q;  q += mat * (2 * chunk);
    double* vals = (double*)q;  q += sizeof(double) * d * (2 * chunk);
    double* prod = (double*)q;  q += mat * chunk;
    int* bad = (int*)q;
    for (int64_t first = 0; first < B; first += chunk) {
        const int64_t n = B - first < chunk ? B - first : chunk;
        hipLaunchKernelGGL(chernoff_stage_kernel<NQ>, dim3((unsigned)n), dim3(CHERNOFF_BIG_NT), 0, stream(), (long long)n,
                           (long long)first, rho, sigma, shared, stack, bad);
        FBX_HIP(hipGetLastError());
        FBX_TRY(fbx_eigh_dev(d, 2 * n, stack, vals, vecs));
        FBX_TRY(fbx_matmul_dev(d, n, vecs, 1, nullptr, vecs + n * DD * 2, 0, prod));
        hipLaunchKernelGGL(chernoff_search_kernel<NQ>, dim3((unsigned)n), dim3(CHERNOFF_BIG_NT), 0, stream(), (long long)n,
                           (long long)first, vals, prod, bad, tol, max_iters, zero_tol, qcb, lower, s, iters);
        FBX_HIP(hipGetLastError());
    }
    return FBX_OK;
}

int chernoff_check(const char* who, int n_qubits, int64_t B, const void* rho, const void* sigma, const void* qcb, int max_iters,
                   double zero_tol) {
    if (n_qubits < 1 || n_qubits > 5) { set_error(std::string(who) + ": n_qubits must be 1..5"); return FBX_ERR_UNSUPPORTED; }
    FBX_REQUIRE(B >= 0 && (B == 0 || (rho && sigma && qcb)), "fbx_chernoff_bound: bad batch / NULL buffer");
    FBX_REQUIRE(max_iters >= 0, "fbx_chernoff_bound: max_iters must be >= 0");
    FBX_REQUIRE(zero_tol >= 0.0 && zero_tol < 1.0, "fbx_chernoff_bound: zero_tol must be in [0, 1)");
    return FBX_OK;
}

}  // namespace
}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_chernoff_bound_dev(int n_qubits, int64_t B, const double* d_rho, const double* d_sigma, int sigma_shared, double tol,
                           int max_iters, double zero_tol, double* d_qcb_out, double* d_lower_out, double* d_s_out,
                           int32_t* d_iters_out) {
    FBX_TRY(chernoff_check("fbx_chernoff_bound_dev", n_qubits, B, d_rho, d_sigma, d_qcb_out, max_iters, zero_tol));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    if (!(tol > 0.0)) tol = 1e-10;
    const int sh = sigma_shared ? 1 : 0;
    switch (n_qubits) {
        case 1: return launch_small<1>(B, d_rho, d_sigma, sh, tol, max_iters, zero_tol, d_qcb_out, d_lower_out, d_s_out, d_iters_out);
        case 2: return launch_small<2>(B, d_rho, d_sigma, sh, tol, max_iters, zero_tol, d_qcb_out, d_lower_out, d_s_out, d_iters_out);
        case 3: return launch_small<3>(B, d_rho, d_sigma, sh, tol, max_iters, zero_tol, d_qcb_out, d_lower_out, d_s_out, d_iters_out);
        case 4: return launch_big<4>(B, d_rho, d_sigma, sh, tol, max_iters, zero_tol, d_qcb_out, d_lower_out, d_s_out, d_iters_out);
        default: return launch_big<5>(B, d_rho, d_sigma, sh, tol, max_iters, zero_tol, d_qcb_out, d_lower_out, d_s_out, d_iters_out);
    }
}

int fbx_chernoff_bound(int n_qubits, int64_t B, const double* rho, const double* sigma, int sigma_shared, double tol,
                       int max_iters, double zero_tol, double* qcb_out, double* lower_out, double* s_out, int32_t* iters_out) {
    FBX_TRY(chernoff_check("fbx_chernoff_bound", n_qubits, B, rho, sigma, qcb_out, max_iters, zero_tol));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t nm = ((size_t)2 << (2 * n_qubits));      // doubles per d x d complex matrix
    HostIO io; double *dr, *ds, *dq, *dl, *dsv; int32_t* dit;
    FBX_TRY(io.in(rho, nm * B, &dr)); FBX_TRY(io.in(sigma, nm * (sigma_shared ? 1 : B), &ds));
    FBX_TRY(io.out_opt(qcb_out, (size_t)B, &dq)); FBX_TRY(io.out_opt(lower_out, (size_t)B, &dl));
    FBX_TRY(io.out_opt(s_out, (size_t)B, &dsv)); FBX_TRY(io.out_opt(iters_out, (size_t)B, &dit));
    FBX_TRY(fbx_chernoff_bound_dev(n_qubits, B, dr, ds, sigma_shared, tol, max_iters, zero_tol, dq, dl, dsv, dit));
    return io.finish();
}

}  // extern "C"
