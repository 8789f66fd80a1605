// fbx_diamond.hip -- batched diamond-norm distance of pairs of channels given as Choi matrices, with a certified
// upper bound (distance_measures.py:378-437).
//
// With J the Hermitian part of choi0 - choi1 (D x D, D = d^2) and S = 1_d (x) T (identity on the LEFT factor, as
// cvx.kron(np.eye(dim), rho) in the reference), T = rho^(1/2):
//     g(rho) = tr[(S J S)_+],   distance = 2 max over density matrices rho of g(rho)   (g is concave in rho).
// Lower bound (primal): L-BFGS over the d^2 real parameters of a Hermitian T on the scale-free quotient
// q(T) = g(T) / tr(T^2) (the host solver's objective, fbx/distance_measures.py _watrous_sdp_value), Armijo backtracking,
// from T = 1 / sqrt(d); grad g = Tr_1(X S J + J S X), X the projector onto the positive eigenspace of S J S.
// Upper bound (dual certificate): for a full-rank rho, M = S J S and Z = S^-1 M_+ S^-1 satisfy Z >= J and Z >= 0, so
// distance <= 2 lambda_max(Tr_1 Z) (Watrous' dual).  The optimum rho is often rank deficient, so the certificate is evaluated
// at rho_eps = (1 - eps) rho + eps 1/d for eps = 1e-1 .. 1e-12 and the smallest value kept; against rounding, Z is shifted by
// max(0, -lambda_min(Z - J), -lambda_min(Z)) 1 before its partial trace is taken.
// The certificate runs at the start (rho = 1/d: the closed-form cases are exact there) and once the primal has stalled.
//
// One item per workgroup: one wavefront for 1 and 2 qubits (D = 4, 16; every matrix in LDS, jacobi_eigh_wave for 16 x 16),
// sixteen wavefronts for 3 qubits (D = 64; the eigensolver's two 64 x 64 buffers fill LDS, the three row-major D x D work
// matrices live in a per-workgroup block of HBM that stays in L2).  The optimiser's vectors (d^2 <= 64 entries) sit one entry per
// lane and every wavefront of the workgroup runs the same (deterministic) arithmetic on them, so every branch is uniform across the
// workgroup without broadcasting decisions; the L-BFGS history is in LDS, written by wavefront 0.  Items never interact: a result
// depends on its own inputs only.
#include "fbx_eigh64.hpp"
#include <cfloat>

namespace fbx {
namespace {

constexpr int DIAMOND_HIST = 8;          // L-BFGS memory
constexpr int DIAMOND_LS_MAX = 40;       // Armijo halvings per line search
constexpr int DIAMOND_NEPS = 12;
constexpr int DIAMOND_GRID3 = 512;       // 3 qubits: resident workgroups (HBM work block each), items strided over them
__constant__ double kDiamondEps[DIAMOND_NEPS] = {1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12};

template <int NQ>
struct Dia {
    static constexpr int d = 1 << NQ, D = d * d, NP = d * d, NT = NQ == 3 ? 1024 : 64;
    static constexpr bool MATS_IN_LDS = NQ <= 2;
    // LDS: Ms, Vs (D x D Jacobi layout), two d x d Jacobi buffers, T, S, S^-1, W, H (d x d), lam[D], lam_s[d], t_k[d], red[64],
    // history s / y [HIST][64] and rho [HIST]; for NQ <= 2 also the work matrices J, X, Z (row-major D x D)
    static constexpr size_t small_bytes = sizeof(cplx) * (2 * sys_elems<D>() + 2 * sys_elems<d>() + 5 * d * d)
                                          + sizeof(double) * (D + 2 * d + 64 + 2 * DIAMOND_HIST * 64 + DIAMOND_HIST);
    static constexpr size_t mats_bytes = sizeof(cplx) * 3 * D * D;
    static constexpr size_t lds_bytes = small_bytes + (MATS_IN_LDS ? mats_bytes : 0);
};

__device__ __forceinline__ void cmac(cplx& acc, const cplx a, const cplx b) {            // acc += a b
    acc.re += a.re * b.re - a.im * b.im; acc.im += a.re * b.im + a.im * b.re;
}
__device__ __forceinline__ void cmacc(cplx& acc, const cplx a, const cplx b) {           // acc += a conj(b)
    acc.re += a.re * b.re + a.im * b.im; acc.im += a.im * b.re - a.re * b.im;
}
__device__ __forceinline__ cplx czero() { cplx z; z.re = 0.0; z.im = 0.0; return z; }

// parameter k of a Hermitian d x d matrix: k < d the diagonal, then Re and Im of the upper triangle (row-major), as the host's pack()
__device__ __forceinline__ void param_entry(int d, int k, int& a, int& b, int& kind) {
    if (k < d) { a = b = k; kind = 0; return; }
    const int nd = d * (d - 1) / 2;
    kind = k < d + nd ? 1 : 2;
    int j = k - d - (kind == 2 ? nd : 0);
    a = 0;
    while (j >= d - 1 - a) { j -= d - 1 - a; ++a; }
    b = a + 1 + j;
}

// Hermitian part (A - Sub)_H of row-major N x N matrices into the Jacobi layout (exactly Hermitian, real diagonal)
template <int N, int NT>
__device__ void herm_to_sys(cplx* Ms, const cplx* A, const cplx* Sub, int t) {
    for (int idx = t; idx < N * N; idx += NT) {
        const int r = idx / N, c = idx % N;
        cplx a = A[r * N + c], b = A[c * N + r];
        if (Sub) {
            const cplx sa = Sub[r * N + c], sb = Sub[c * N + r];
            a.re -= sa.re; a.im -= sa.im; b.re -= sb.re; b.im -= sb.im;
        }
        cplx v; v.re = 0.5 * (a.re + b.re); v.im = r == c ? 0.0 : 0.5 * (a.im - b.im);
        Ms[sys_index<N>(r, c)] = v;
    }
}

// eigenvalues of the Hermitian matrix staged in Ms into lam (Jacobi order), eigenvectors as the columns of Vs
template <int N, int NT>
__device__ __attribute__((noinline)) void eig(cplx* Ms, cplx* Vs, double* lam, double* red, int t) {
    __syncthreads();
    jacobi_eigh_block<N, NT>(Ms, Vs, t, true, red);
    __syncthreads();
    if (t < N) lam[t] = Ms[sys_index<N>(t, t)].re;
    __syncthreads();
}

// dst[r][(j, b)] = sum_b' src[r][(j, b')] A[b'][b]   (src (1 (x) A))
template <int NQ>
__device__ void rmul(cplx* dst, const cplx* src, const cplx* A, int t) {
    constexpr int d = Dia<NQ>::d, D = Dia<NQ>::D, NT = Dia<NQ>::NT;
    for (int idx = t; idx < D * D; idx += NT) {
        const int r = idx / D, c = idx % D, j = c / d, b = c % d;
        cplx acc = czero();
#pragma unroll
        for (int bp = 0; bp < d; ++bp) cmac(acc, src[r * D + j * d + bp], A[bp * d + b]);
        dst[idx] = acc;
    }
    __syncthreads();
}
// dst[(i, a)][c] = sum_a' A[a][a'] src[(i, a')][c]   ((1 (x) A) src)
template <int NQ>
__device__ void lmul(cplx* dst, const cplx* src, const cplx* A, int t) {
    constexpr int d = Dia<NQ>::d, D = Dia<NQ>::D, NT = Dia<NQ>::NT;
    for (int idx = t; idx < D * D; idx += NT) {
        const int r = idx / D, c = idx % D, i = r / d, a = r % d;
        cplx acc = czero();
#pragma unroll
        for (int ap = 0; ap < d; ++ap) cmac(acc, A[a * d + ap], src[(i * d + ap) * D + c]);
        dst[idx] = acc;
    }
    __syncthreads();
}
// dst = sum_k w_k v_k v_k^H over the eigenvectors in Vs; w_k = [lam_k > 0] (POS_PART false) or max(lam_k, 0) (true)
template <int N, int NT, bool POS_PART>
__device__ void recon(cplx* dst, const cplx* Vs, const double* lam, int t) {
    for (int idx = t; idx < N * N; idx += NT) {
        const int r = idx / N, c = idx % N;
        cplx acc = czero();
        for (int k = 0; k < N; ++k) {
            const double l = lam[k];
            if (!(l > 0.0)) continue;
            cplx u = Vs[sys_index<N>(r, k)];
            if (POS_PART) { u.re *= l; u.im *= l; }
            cmacc(acc, u, Vs[sys_index<N>(c, k)]);
        }
        dst[idx] = acc;
    }
    __syncthreads();
}

template <int NQ>
struct DiamondItem {
    static constexpr int d = Dia<NQ>::d, D = Dia<NQ>::D, NP = Dia<NQ>::NP, NT = Dia<NQ>::NT;
    cplx *Ms, *Vs, *ms_s, *vs_s, *Tm, *Sm, *Si, *Wm, *Hm, *Jm, *Xm, *Zm;
    double *lam, *lam_s, *tk, *red, *hs, *hy, *hr;
    int t, lane;

    __device__ void carve(char* p, cplx* mats) {
        Ms = (cplx*)p; p += sizeof(cplx) * sys_elems<D>();
        Vs = (cplx*)p; p += sizeof(cplx) * sys_elems<D>();
        ms_s = (cplx*)p; p += sizeof(cplx) * sys_elems<d>();
        vs_s = (cplx*)p; p += sizeof(cplx) * sys_elems<d>();
        Tm = (cplx*)p; p += sizeof(cplx) * d * d;
        Sm = (cplx*)p; p += sizeof(cplx) * d * d;
        Si = (cplx*)p; p += sizeof(cplx) * d * d;
        Wm = (cplx*)p; p += sizeof(cplx) * d * d;
        Hm = (cplx*)p; p += sizeof(cplx) * d * d;
        lam = (double*)p; p += sizeof(double) * D;
        lam_s = (double*)p; p += sizeof(double) * d;
        tk = (double*)p; p += sizeof(double) * d;
        red = (double*)p; p += sizeof(double) * 64;
        hs = (double*)p; p += sizeof(double) * DIAMOND_HIST * 64;
        hy = (double*)p; p += sizeof(double) * DIAMOND_HIST * 64;
        hr = (double*)p; p += sizeof(double) * DIAMOND_HIST;
        if (mats == nullptr) mats = (cplx*)p;
        Jm = mats; Xm = mats + D * D; Zm = mats + 2 * D * D;
    }

    // T from the parameters (lane k of every wavefront holds x_k; wavefront 0 writes)
    __device__ void write_T(double x) {
        __syncthreads();
        if (t < NP) {
            int a, b, kind;
            param_entry(d, lane, a, b, kind);
            if (kind == 0) { Tm[a * d + a].re = x; Tm[a * d + a].im = 0.0; }
            else if (kind == 1) { Tm[a * d + b].re = x; Tm[b * d + a].re = x; }
            else { Tm[a * d + b].im = x; Tm[b * d + a].im = -x; }
        }
        __syncthreads();
    }

    // g(T) = tr[(S J S)_+] and H = Tr_1(X S J) (X the positive-eigenspace projector); grad g = H + H^H
    __device__ double eval_g() {
        rmul<NQ>(Zm, Jm, Tm, t);                 // J S
        lmul<NQ>(Xm, Zm, Tm, t);                 // S J S
        herm_to_sys<D, NT>(Ms, Xm, nullptr, t);
        eig<D, NT>(Ms, Vs, lam, red, t);
        double g = 0.0;
        for (int k = 0; k < D; ++k) g += lam[k] > 0.0 ? lam[k] : 0.0;
        recon<D, NT, false>(Xm, Vs, lam, t);     // X
        rmul<NQ>(Zm, Xm, Tm, t);                 // Y = X S
        if (t < d * d) {
            const int a = t / d, b = t % d;
            cplx acc = czero();
            for (int i = 0; i < d; ++i)
                for (int c = 0; c < D; ++c) cmac(acc, Zm[(i * d + a) * D + c], Jm[c * D + i * d + b]);
            Hm[t] = acc;
        }
        __syncthreads();
        return g;
    }

    // gradient of F = -q = -g / n2 with respect to this lane's parameter
    __device__ double gradF(double x, double q, double n2) const {
        if (lane >= NP) return 0.0;
        int a, b, kind;
        param_entry(d, lane, a, b, kind);
        const cplx hab = Hm[a * d + b], hba = Hm[b * d + a];
        double pg, pt;
        if (kind == 0) { pg = 2.0 * hab.re; pt = x; }
        else if (kind == 1) { pg = 2.0 * (hab.re + hba.re); pt = 2.0 * x; }
        else { pg = 2.0 * (hab.im - hba.im); pt = 2.0 * x; }
        return -(pg - 2.0 * q * pt) / n2;
    }

    __device__ double norm2(double x) const {                  // tr(T^2)
        double w = 0.0;
        if (lane < NP) w = (lane < d ? 1.0 : 2.0) * x * x;
        return wave_sum(w);
    }

    // smallest certified upper bound on max g over the eps list (or the first eps only); stops early once within tol of q
    __device__ double certificate(double n2, double q, double tol, bool first_only) {
        herm_to_sys<d, NT>(ms_s, Tm, nullptr, t);
        eig<d, NT>(ms_s, vs_s, tk, red, t);
        if (t < d * d) Wm[t] = vs_s[sys_index<d>(t / d, t % d)];
        __syncthreads();
        double best = INFINITY;
        const int neps = first_only ? 1 : DIAMOND_NEPS;
        for (int e = 0; e < neps; ++e) {
            const double eps = kDiamondEps[e];
            if (t < d * d) {
                const int a = t / d, b = t % d;
                cplx s = czero(), si = czero();
                for (int k = 0; k < d; ++k) {
                    const double mu = (1.0 - eps) * (tk[k] * tk[k] / n2) + eps / d;
                    const double r = sqrt(mu), ri = 1.0 / r;
                    cplx u = Wm[a * d + k], ui = u;
                    u.re *= r; u.im *= r; ui.re *= ri; ui.im *= ri;
                    cmacc(s, u, Wm[b * d + k]); cmacc(si, ui, Wm[b * d + k]);
                }
                Sm[t] = s; Si[t] = si;
            }
            __syncthreads();
            rmul<NQ>(Zm, Jm, Sm, t);
            lmul<NQ>(Xm, Zm, Sm, t);                         // M = S J S
            herm_to_sys<D, NT>(Ms, Xm, nullptr, t);
            eig<D, NT>(Ms, Vs, lam, red, t);
            recon<D, NT, true>(Xm, Vs, lam, t);             // M_+
            rmul<NQ>(Zm, Xm, Si, t);
            lmul<NQ>(Xm, Zm, Si, t);                         // S^-1 M_+ S^-1
            for (int idx = t; idx < D * D; idx += NT) {      // Z = its Hermitian part
                const int r = idx / D, c = idx % D;
                const cplx a = Xm[r * D + c], b = Xm[c * D + r];
                cplx v; v.re = 0.5 * (a.re + b.re); v.im = r == c ? 0.0 : 0.5 * (a.im - b.im);
                Zm[idx] = v;
            }
            __syncthreads();
            if (t < d * d) {                                 // Tr_1 Z
                const int a = t / d, b = t % d;
                cplx acc = czero();
                for (int i = 0; i < d; ++i) { const cplx z = Zm[(i * d + a) * D + i * d + b]; acc.re += z.re; acc.im += z.im; }
                Hm[t] = acc;
            }
            __syncthreads();
            herm_to_sys<d, NT>(ms_s, Hm, nullptr, t);
            eig<d, NT>(ms_s, vs_s, lam_s, red, t);
            double u0 = -INFINITY;
            for (int k = 0; k < d; ++k) u0 = fmax(u0, lam_s[k]);
            if (!(u0 < best)) continue;
            herm_to_sys<D, NT>(Ms, Zm, Jm, t);              // lambda_min(Z - J)
            eig<D, NT>(Ms, Vs, lam, red, t);
            double m1 = INFINITY;
            for (int k = 0; k < D; ++k) m1 = fmin(m1, lam[k]);
            herm_to_sys<D, NT>(Ms, Zm, nullptr, t);         // lambda_min(Z)
            eig<D, NT>(Ms, Vs, lam, red, t);
            double m2 = INFINITY;
            for (int k = 0; k < D; ++k) m2 = fmin(m2, lam[k]);
            const double shift = fmax(0.0, fmax(-m1, -m2));
            const double u = u0 + d * shift;                 // lambda_max(Tr_1 (Z + shift 1))
            if (u < best) best = u;
            if (2.0 * best - 2.0 * q <= tol * fmax(2.0 * q, 1e-12)) break;
        }
        return best;
    }
};

template <int NQ>
__global__ void __launch_bounds__(Dia<NQ>::NT)
diamond_kernel(long long B, const double* __restrict__ choi0, const double* __restrict__ choi1, int shared_target, double tol,
               int max_iters, cplx* __restrict__ work, double* __restrict__ dist_out, double* __restrict__ upper_out,
               double* __restrict__ rho_out, int32_t* __restrict__ iters_out) {
    using C = Dia<NQ>;
    constexpr int d = C::d, D = C::D, NP = C::NP, NT = C::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DiamondItem<NQ> it;
    it.t = threadIdx.x; it.lane = threadIdx.x & 63;
    it.carve(smem, C::MATS_IN_LDS ? nullptr : work + (size_t)blockIdx.x * 3 * D * D);
    const int t = it.t, lane = it.lane;
    for (long long item = blockIdx.x; item < B; item += gridDim.x) {
        const cplx* c0 = (const cplx*)choi0 + item * D * D;
        const cplx* c1 = (const cplx*)choi1 + (shared_target ? 0 : item * D * D);
        double bad = 0.0;
        __syncthreads();
        for (int idx = t; idx < D * D; idx += NT) {          // J = Hermitian part of choi0 - choi1
            const int r = idx / D, c = idx % D;
            const cplx a0 = c0[r * D + c], a1 = c1[r * D + c], b0 = c0[c * D + r], b1 = c1[c * D + r];
            const double dar = a0.re - a1.re, dai = a0.im - a1.im, dbr = b0.re - b1.re, dbi = b0.im - b1.im;
            cplx v; v.re = 0.5 * (dar + dbr); v.im = r == c ? 0.0 : 0.5 * (dai - dbi);
            it.Jm[idx] = v;
            bad += fabs(dar) + fabs(dai);
        }
        __syncthreads();
        bad = block_sum<NT>(bad, it.red);
        if (!(bad <= DBL_MAX)) {                             // non-finite input: non-finite result for this item only
            if (t == 0) {
                dist_out[item] = NAN;
                if (upper_out) upper_out[item] = NAN;
                if (iters_out) iters_out[item] = -1;
            }
            if (rho_out)
                for (int idx = t; idx < d * d * 2; idx += NT) rho_out[item * d * d * 2 + idx] = NAN;
            continue;
        }
        double x = lane < d ? 1.0 / sqrt((double)d) : 0.0;     // T = 1 / sqrt(d): rho = 1 / d
        if (lane >= NP) x = 0.0;
        it.write_T(x);
        double n2 = it.norm2(x);
        double q = it.eval_g() / n2;
        double gF = it.gradF(x, q, n2), F = -q;
        double upper = it.certificate(n2, q, tol, true);
        int iters = 0;
        bool conv = 2.0 * upper - 2.0 * q <= tol * fmax(2.0 * q, 1e-12);
        if (!conv) {
            int hn = 0, head = 0;                            // history entries, next slot
            for (; iters < max_iters;) {
                // two-loop recursion: r = H grad F
                double r = gF, alpha[DIAMOND_HIST];
#pragma unroll
                for (int j = 0; j < DIAMOND_HIST; ++j) {
                    alpha[j] = 0.0;
                    if (j < hn) {
                        const int s = (head - 1 - j + DIAMOND_HIST) % DIAMOND_HIST;
                        alpha[j] = it.hr[s] * wave_sum(it.hs[s * 64 + lane] * r);
                        r -= alpha[j] * it.hy[s * 64 + lane];
                    }
                }
                if (hn > 0) {
                    const int s = (head - 1 + DIAMOND_HIST) % DIAMOND_HIST;
                    const double yy = wave_sum(it.hy[s * 64 + lane] * it.hy[s * 64 + lane]);
                    r *= 1.0 / (it.hr[s] * yy);                 // gamma = s.y / y.y
                } else {
                    r *= 1.0 / sqrt(wave_sum(gF * gF));        // first step: unit length
                }
#pragma unroll
                for (int j = DIAMOND_HIST - 1; j >= 0; --j) {
                    if (j < hn) {
                        const int s = (head - 1 - j + DIAMOND_HIST) % DIAMOND_HIST;
                        const double bta = it.hr[s] * wave_sum(it.hy[s * 64 + lane] * r);
                        r += (alpha[j] - bta) * it.hs[s * 64 + lane];
                    }
                }
                double dir = -r, gd = wave_sum(gF * dir);
                if (!(gd < 0.0)) {                           // not a descent direction: restart from steepest descent
                    hn = 0;
                    dir = -gF / sqrt(wave_sum(gF * gF));
                    gd = wave_sum(gF * dir);
                    if (!(gd < 0.0)) break;                  // zero gradient
                }
                double step = 1.0, xn = x, qn = q, n2n = n2, Fn = F;
                bool ok = false;
                for (int ls = 0; ls < DIAMOND_LS_MAX; ++ls, step *= 0.5) {
                    xn = lane < NP ? x + step * dir : 0.0;
                    it.write_T(xn);
                    n2n = it.norm2(xn);
                    qn = it.eval_g() / n2n;
                    Fn = -qn;
                    if (Fn <= F + 1e-4 * step * gd) { ok = true; break; }
                }
                if (!ok) break;
                const double gFn = it.gradF(xn, qn, n2n);
                const double sv = xn - x, yv = gFn - gF, sy = wave_sum(sv * yv);
                if (sy > 0.0) {
                    if (t < 64) { it.hs[head * 64 + lane] = sv; it.hy[head * 64 + lane] = yv; }
                    if (t == 0) it.hr[head] = 1.0 / sy;
                    head = (head + 1) % DIAMOND_HIST;
                    hn = hn < DIAMOND_HIST ? hn + 1 : DIAMOND_HIST;
                }
                __syncthreads();
                const double gain = F - Fn;
                x = xn; gF = gFn; q = qn; n2 = n2n; F = Fn; ++iters;
                if (!(gain > 1e-15 * fabs(F))) break;       // stalled
            }
            it.write_T(x);
            const double u = it.certificate(n2, q, tol, false);
            if (u < upper) upper = u;
            conv = 2.0 * upper - 2.0 * q <= tol * fmax(2.0 * q, 1e-12);
        }
        if (t == 0) {
            dist_out[item] = 2.0 * q;
            // (at an exact start the computed lower bound can exceed the certificate by an ulp: the upper bound is never below it)
            if (upper_out) upper_out[item] = fmax(2.0 * upper, 2.0 * q);
            if (iters_out) iters_out[item] = conv ? iters : -(iters > 0 ? iters : 1);
        }
        if (rho_out && t < d * d) {                          // rho = T^2 / tr(T^2)
            const int a = t / d, b = t % d;
            cplx acc = czero();
            for (int c = 0; c < d; ++c) cmac(acc, it.Tm[a * d + c], it.Tm[c * d + b]);
            rho_out[(item * d * d + t) * 2] = acc.re / n2;
            rho_out[(item * d * d + t) * 2 + 1] = acc.im / n2;
        }
    }
}

template <int NQ>
int launch_diamond(int64_t B, const double* c0, const double* c1, int shared, double tol, int max_iters, double* dist,
                   double* upper, double* rho, int32_t* iters) {
    using C = Dia<NQ>;
    cplx* work = nullptr;
    long long grid = B < (1LL << 20) ? B : (1LL << 20);
    if (!C::MATS_IN_LDS) {
        grid = B < DIAMOND_GRID3 ? B : DIAMOND_GRID3;
        void* p = nullptr;
        const int rc = workspace(WS_DIAMOND, C::mats_bytes * (size_t)grid, &p);
        if (rc) return rc;
        work = (cplx*)p;
    }
    auto kern = diamond_kernel<NQ>;
    FBX_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(C::NT), C::lds_bytes, stream(), (long long)B, c0, c1, shared, tol, max_iters,
                       work, dist, upper, rho, iters);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

static_assert(Dia<3>::lds_bytes <= 160 * 1024, "3-qubit diamond kernel: LDS");

int diamond_check(const char* who, int n_qubits, int64_t B, const void* c0, const void* c1, const void* dist, int max_iters) {
    if (n_qubits > 3) { set_error(std::string(who) + ": n_qubits must be 1..3 (larger pairs are not implemented)"); return FBX_ERR_UNSUPPORTED; }
    FBX_REQUIRE(n_qubits >= 1, "fbx_diamond_norm: n_qubits must be 1..3");
    FBX_REQUIRE(B >= 0 && (B == 0 || (c0 && c1 && dist)), "fbx_diamond_norm: bad batch / NULL buffer");
    FBX_REQUIRE(max_iters >= 0, "fbx_diamond_norm: max_iters must be >= 0");
    return FBX_OK;
}

}  // namespace
}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_diamond_norm_dev(int n_qubits, int64_t B, const double* d_choi0, const double* d_choi1, int choi1_shared, double tol,
                         int max_iters, double* d_dist_out, double* d_upper_out, double* d_rho_out, int32_t* d_iters_out) {
    FBX_TRY(diamond_check("fbx_diamond_norm_dev", n_qubits, B, d_choi0, d_choi1, d_dist_out, max_iters));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    if (!(tol > 0.0)) tol = 1e-7;
    const int sh = choi1_shared ? 1 : 0;
    switch (n_qubits) {
        case 1: return launch_diamond<1>(B, d_choi0, d_choi1, sh, tol, max_iters, d_dist_out, d_upper_out, d_rho_out, d_iters_out);
        case 2: return launch_diamond<2>(B, d_choi0, d_choi1, sh, tol, max_iters, d_dist_out, d_upper_out, d_rho_out, d_iters_out);
        default: return launch_diamond<3>(B, d_choi0, d_choi1, sh, tol, max_iters, d_dist_out, d_upper_out, d_rho_out, d_iters_out);
    }
}

int fbx_diamond_norm(int n_qubits, int64_t B, const double* choi0, const double* choi1, int choi1_shared, double tol, int max_iters,
                     double* dist_out, double* upper_out, double* rho_out, int32_t* iters_out) {
    FBX_TRY(diamond_check("fbx_diamond_norm", n_qubits, B, choi0, choi1, dist_out, max_iters));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t d = (size_t)1 << n_qubits, D = d * d, nm = D * D * 2;
    HostIO io; double *dc0, *dc1, *ddist, *dup, *drho; int32_t* dit;
    FBX_TRY(io.in(choi0, nm * B, &dc0)); FBX_TRY(io.in(choi1, nm * (choi1_shared ? 1 : B), &dc1));
    FBX_TRY(io.out_opt(dist_out, (size_t)B, &ddist)); FBX_TRY(io.out_opt(upper_out, (size_t)B, &dup));
    FBX_TRY(io.out_opt(rho_out, d * d * 2 * B, &drho)); FBX_TRY(io.out_opt(iters_out, (size_t)B, &dit));
    FBX_TRY(fbx_diamond_norm_dev(n_qubits, B, dc0, dc1, choi1_shared, tol, max_iters, ddist, dup, drho, dit));
    return io.finish();
}

}  // extern "C"
