// fbx_fit.hip -- batched weighted non-linear least squares for the four curve models of analysis/fitting.py (:16-149), and the
// reductions that feed them: RB survival statistics (randomized_benchmarking.py:308-383), shifted purity and its error
// (:490-533), and the weights / default guess every fitting front end builds (:423-436, :577-589).
//
// fbx_curve_fit: ONE FIT PER LANE.  A fit is K <= 256 points and P <= 5 parameters: the normal matrix J^T J (packed into P x P
// registers), the gradient J^T r, the Cholesky factor of the damped system and the step all live in registers; there is no LDS and
// no communication between lanes.  The data are first transposed into a [K][B] workspace (one tiled pass), so that the 64 lanes of
// a wavefront read 64 consecutive doubles per point; a shared x is read through a wave-uniform (scalar) load.
//
// The iteration is Levenberg-Marquardt on the column-scaled normal equations: with D_j the largest column norm of J seen so far
// (MINPACK's diag, lmder.f), A = D^-1 J^T J D^-1 and gs = D^-1 J^T r, the step solves (A + lambda I) h = -gs, delta = D^-1 h.  A has
// a diagonal <= 1, so lambda is dimensionless (start 1e-3).  The damping follows the gain ratio rho = actual / predicted reduction
// (Nielsen's update: accepted steps multiply lambda by max(1/3, 1 - (2 rho - 1)^3), rejected ones by 2, 4, 8, ...).  A trial point
// whose cost, gradient or normal matrix is not finite (a negative decay under a non-integer power, decay_time -> 0) is a rejected
// step.  One pass over the K points evaluates cost, gradient AND normal matrix at the trial point, so an accepted step costs one
// pass, not two.  The stop tests are MINPACK's (relative actual and predicted reduction <= ftol; scaled step <= xtol * scaled
// parameters), but a test only marks the item: it is declared converged at the top of the next iteration, where the gradient at
// the NEW point is known, and only if grad_norm is below the bound fbx.h documents -- otherwise it iterates on.  Lanes of one
// wavefront stop at different iterations; a finished lane idles until its wavefront is done (iters[] gives the accounting).
//
// Non-finite data or guess: the first evaluation is not finite, the item reports FBX_FIT_BAD_START with NaN results, and no other
// item reads anything of it.  Every comparison that keeps an item iterating is written so that a NaN ends it.
#include "fbx_common.hpp"
#include <cmath>

namespace fbx {

template <int MODEL> struct FitP { static constexpr int P = MODEL == FBX_FIT_DECAYING_COSINE ? 5 : MODEL == FBX_FIT_SHIFTED_COSINE ? 4 : 3; };

static int fit_param_count(int model) {
    switch (model) {
        case FBX_FIT_BASE_DECAY: case FBX_FIT_TIME_DECAY: return 3;
        case FBX_FIT_DECAYING_COSINE: return 5;
        case FBX_FIT_SHIFTED_COSINE: return 4;
    }
    return 0;
}

// model value f and its derivatives d[] with respect to the parameters (the reference's order) at one point.  The value is
// computed operation by operation in the order of the reference's numpy expressions, without contraction into fused
// multiply-adds: the argument of a cosine at x = 50 periods is then bit-identical to numpy's, and the value differs from it by
// the last bits of pow / exp / cos only (tests compare chisqr with a numpy evaluation at the returned parameters).
template <int MODEL, int P>
__device__ __forceinline__ void fit_point(const double (&p)[P], double x, double& f, double (&d)[P]) {
#pragma clang fp contract(off)
    if constexpr (MODEL == FBX_FIT_BASE_DECAY) {                      // baseline + amplitude * decay**x
        const double t = pow(p[1], x);
        f = p[2] + p[0] * t;
        d[0] = t;
        d[1] = p[0] * x * (p[1] != 0.0 ? t / p[1] : pow(p[1], x - 1.0));
        d[2] = 1.0;
    } else if constexpr (MODEL == FBX_FIT_TIME_DECAY) {               // amplitude * exp(-(x - offset) / decay_time)
        const double it = 1.0 / p[1], xo = x - p[2], e = exp(-xo / p[1]);
        f = p[0] * e;
        d[0] = e;
        d[1] = f * xo * it * it;
        d[2] = f * it;
    } else if constexpr (MODEL == FBX_FIT_DECAYING_COSINE) {          // amplitude * exp(-x / decay_time) * cos(2 pi frequency x + offset) + baseline
        const double it = 1.0 / p[1], e = exp(-x / p[1]);
        double s, c;
        sincos(6.283185307179586476925 * p[4] * x + p[2], &s, &c);
        const double ae = p[0] * e;
        f = ae * c + p[3];
        d[0] = e * c;
        d[1] = ae * c * x * it * it;
        d[2] = -ae * s;
        d[3] = 1.0;
        d[4] = d[2] * (6.283185307179586476925 * x);
    } else {                                                          // amplitude * cos(frequency x + offset) + baseline
        double s, c;
        sincos(p[3] * x + p[1], &s, &c);
        f = p[0] * c + p[2];
        d[0] = c;
        d[1] = -p[0] * s;
        d[2] = 1.0;
        d[3] = d[1] * x;
    }
}

struct FitData {
    const double* xs;      // shared x [K], or NULL
    const double* xT;      // per-item x, transposed [K][ld], or NULL
    const double* yT;      // [K][ld]
    const double* wT;      // [K][ld], or NULL
    size_t ld;
    int K;
};

// cost S = sum r^2, gradient g = J^T r and normal matrix H = J^T J (full, symmetric) of the weighted residual r = (f - y) w at p.
// A fixed parameter gets a zero gradient and a unit row / column, so the P x P algebra below never has to know about it.
template <int MODEL, int P>
__device__ __forceinline__ void fit_eval(const double (&p)[P], const FitData& da, size_t col, unsigned vary, double& S,
                                         double (&g)[P], double (&H)[P][P]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        g[i] = 0.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) H[i][j] = 0.0;
    }
    for (int k = 0; k < da.K; ++k) {
        const size_t at = (size_t)k * da.ld + col;
        const double x = da.xs ? da.xs[k] : da.xT[at];
        const double y = da.yT[at];
        const double w = da.wT ? da.wT[at] : 1.0;
        double f, d[P];
        fit_point<MODEL, P>(p, x, f, d);
        const double r = (f - y) * w;
        s = fma(r, r, s);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            d[i] *= w;
            g[i] = fma(d[i], r, g[i]);
#pragma unroll
            for (int j = 0; j <= i; ++j) H[i][j] = fma(d[i], d[j], H[i][j]);
        }
    }
    S = s;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const bool fi = !((vary >> i) & 1u);
        if (fi) g[i] = 0.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const bool fj = !((vary >> j) & 1u);
            if (fi || fj) H[i][j] = (i == j) ? 1.0 : 0.0;
            H[j][i] = H[i][j];
        }
    }
}

// Cholesky factor (lower, in place of the lower triangle of M); returns the smallest pivot (<= 0 or NaN: not positive definite)
template <int P>
__device__ __forceinline__ double fit_cholesky(double (&M)[P][P]) {
    double minpiv = 1e300;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double piv = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) piv = fma(-M[j][k], M[j][k], piv);
        minpiv = (piv < minpiv) ? piv : (piv == piv ? minpiv : piv);       // a NaN pivot is kept
        const double l = sqrt(piv), il = 1.0 / l;
        M[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < P; ++i) {
            double v = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = fma(-M[i][k], M[j][k], v);
            M[i][j] = v * il;
        }
    }
    return minpiv;
}

__device__ __forceinline__ bool fit_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN

template <int MODEL>
__global__ void __launch_bounds__(256)
fit_kernel(long long B, FitData da, const double* __restrict__ guess, unsigned vary, double ftol, double xtol, int max_iters,
           double* __restrict__ params_out, double* __restrict__ covar_out, double* __restrict__ chisqr_out,
           double* __restrict__ redchi_out, int* __restrict__ iters_out, int* __restrict__ status_out,
           double* __restrict__ gnorm_out) {
    constexpr int P = FitP<MODEL>::P;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = b < B;
    const size_t col = live ? (size_t)b : 0;
    int nfree = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) nfree += (int)((vary >> j) & 1u);
    const double tolmax = ftol > xtol ? ftol : xtol;

    double p[P], g[P], H[P][P], D[P], S = 0.0, floor_ = 0.0, gn = 0.0, lam = 1e-3, nu = 2.0;
    int it = 0, status = 0, pend = 0;
    bool done = !live;
#pragma unroll
    for (int j = 0; j < P; ++j) { p[j] = 0.0; D[j] = 0.0; g[j] = 0.0; }
    if (live) {
#pragma unroll
        for (int j = 0; j < P; ++j) p[j] = guess[col * P + j];
        double yn = 0.0;                                              // || w y ||^2: the scale of the rounding floor of a residual
        for (int k = 0; k < da.K; ++k) {
            const size_t at = (size_t)k * da.ld + col;
            const double wy = da.yT[at] * (da.wT ? da.wT[at] : 1.0);
            yn = fma(wy, wy, yn);
        }
        floor_ = FBX_FIT_GRAD_FLOOR * sqrt(yn);
        fit_eval<MODEL, P>(p, da, col, vary, S, g, H);
        bool fin = fit_finite(S) && fit_finite(floor_);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            fin = fin && fit_finite(g[i]) && fit_finite(p[i]);
#pragma unroll
            for (int j = 0; j <= i; ++j) fin = fin && fit_finite(H[i][j]);
        }
        if (!fin) { status = FBX_FIT_BAD_START; done = true; }
    }
    while (!done) {
        // ---- top of an iteration: S, g, H belong to p
        gn = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double cn = sqrt(H[j][j]);
            D[j] = cn > D[j] ? cn : D[j];
            if (((vary >> j) & 1u) && cn > 0.0) gn = fmax(gn, fabs(g[j]) / cn);
        }
        const double gbound = sqrt((double)(nfree + 1) * tolmax * S) + floor_;
        if (S == 0.0 || (pend && gn <= gbound)) { status = pend ? pend : FBX_FIT_CONVERGED_FTOL; done = true; continue; }
        if (!(it < max_iters)) { status = FBX_FIT_MAX_ITERS; done = true; continue; }
        pend = 0;
        // ---- the damped, column-scaled step
        double dj[P], A[P][P], M[P][P], h[P];
#pragma unroll
        for (int j = 0; j < P; ++j) dj[j] = 1.0 / (D[j] > 0.0 ? D[j] : 1.0);
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) { A[i][j] = H[i][j] * dj[i] * dj[j]; M[i][j] = A[i][j] + (i == j ? lam : 0.0); }
        const double minpiv = fit_cholesky<P>(M);
#pragma unroll
        for (int i = 0; i < P; ++i) {                                 // L z = -gs
            double v = -g[i] * dj[i];
#pragma unroll
            for (int k = 0; k < i; ++k) v = fma(-M[i][k], h[k], v);
            h[i] = v / M[i][i];
        }
#pragma unroll
        for (int i = P - 1; i >= 0; --i) {                            // L^T h = z
            double v = h[i];
#pragma unroll
            for (int k = i + 1; k < P; ++k) v = fma(-M[k][i], h[k], v);
            h[i] = v / M[i][i];
        }
        double pred = 0.0, hn2 = 0.0, xn2 = 0.0, pt[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double ah = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) ah = fma(A[i][j], h[j], ah);
            const bool fr = (vary >> i) & 1u;
            if (!fr) h[i] = 0.0;
            pred = fma(h[i], ah + 2.0 * lam * h[i], pred);
            hn2 = fma(h[i], h[i], hn2);
            const double dp = fr ? p[i] / dj[i] : 0.0;
            xn2 = fma(dp, dp, xn2);
            pt[i] = fr ? p[i] + h[i] * dj[i] : p[i];
        }
        double St, gt[P], Ht[P][P];
        fit_eval<MODEL, P>(pt, da, col, vary, St, gt, Ht);
        bool fin = fit_finite(St) && fit_finite(pred);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            fin = fin && fit_finite(gt[i]) && fit_finite(pt[i]);
#pragma unroll
            for (int j = 0; j <= i; ++j) fin = fin && fit_finite(Ht[i][j]);
        }
        const double rho = (S - St) / pred;
        const bool accept = minpiv > 0.0 && fin && rho > 0.0;     // a NaN anywhere: rejected
        if (accept) {
            const double actred = 1.0 - St / S, prered = pred / S;
            if (!(fabs(actred) > ftol) && !(prered > ftol) && !(rho > 2.0)) pend = FBX_FIT_CONVERGED_FTOL;
            S = St;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                p[i] = pt[i]; g[i] = gt[i];
#pragma unroll
                for (int j = 0; j < P; ++j) H[i][j] = Ht[i][j];
            }
            const double t = 2.0 * rho - 1.0;
            lam *= fmax(1.0 / 3.0, 1.0 - t * t * t);
            lam = fmax(lam, 1e-15);
            nu = 2.0;
        } else {
            lam = fmin(lam * nu, 1e100);
            nu = fmin(2.0 * nu, 1e30);
        }
        if (!pend && !(hn2 > xtol * xtol * xn2)) pend = FBX_FIT_CONVERGED_XTOL;
        ++it;
    }
    if (!live) return;
    // ---- results
    const bool bad = status == FBX_FIT_BAD_START;
    const double nan = __builtin_nan("");
    const int dof = da.K - nfree;
    const double redchi = S / (double)(dof > 1 ? dof : 1);
    bool singular = false;
    if (covar_out) {
        // inv(J^T J) * redchi through the Cholesky factor of the matrix scaled to a unit diagonal; a pivot at the rounding level of
        // that matrix means that some combination of parameters does not move the model: no covariance
        double cn[P], M[P][P];
#pragma unroll
        for (int j = 0; j < P; ++j) { cn[j] = sqrt(H[j][j]); if (!(cn[j] > 0.0)) singular = true; cn[j] = 1.0 / cn[j]; }
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) M[i][j] = H[i][j] * cn[i] * cn[j];
        const double minpiv = fit_cholesky<P>(M);
        if (!(minpiv > FBX_FIT_SINGULAR_PIVOT)) singular = true;
        double Li[P][P];                                              // inverse of L (lower)
#pragma unroll
        for (int i = 0; i < P; ++i) {
            Li[i][i] = 1.0 / M[i][i];
#pragma unroll
            for (int j = 0; j < i; ++j) {
                double v = 0.0;
#pragma unroll
                for (int k = j; k < i; ++k) v = fma(M[i][k], Li[k][j], v);
                Li[i][j] = -v * Li[i][i];
            }
        }
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) {
                double v = 0.0;
#pragma unroll
                for (int k = (i > j ? i : j); k < P; ++k) v = fma(Li[k][i], Li[k][j], v);
                const bool fr = ((vary >> i) & 1u) && ((vary >> j) & 1u);
                covar_out[(col * P + i) * P + j] = (bad || singular) ? nan : (fr ? v * cn[i] * cn[j] * redchi : 0.0);
            }
    }
    if (params_out)
#pragma unroll
        for (int j = 0; j < P; ++j) params_out[col * P + j] = bad ? nan : p[j];
    if (chisqr_out) chisqr_out[col] = bad ? nan : S;
    if (redchi_out) redchi_out[col] = bad ? nan : redchi;
    if (iters_out) iters_out[col] = it;
    if (status_out) status_out[col] = status | ((singular && !bad) ? FBX_FIT_SINGULAR_COVAR : 0);
    if (gnorm_out) gnorm_out[col] = bad ? nan : gn;
}

// in [B][K] -> out [K][B]
__global__ void __launch_bounds__(256)
fit_transpose_kernel(long long B, int K, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double tile[32][33];
    const long long b0 = (long long)blockIdx.x * 32;
    const int k0 = (int)blockIdx.y * 32, tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    for (int r = ty; r < 32; r += 8) {
        const long long b = b0 + r;
        const int k = k0 + tx;
        if (b < B && k < K) tile[r][tx] = in[(size_t)b * K + k];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long long b = b0 + tx;
        const int k = k0 + r;
        if (b < B && k < K) out[(size_t)k * B + b] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One thread per sequence; the rows are short (dim - 1 <= 31, dim^2 - 1 <= 63 doubles) and are re-read from the cache.
__global__ void __launch_bounds__(256)
rb_survival_kernel(int dim, long long S, const double* __restrict__ e, const double* __restrict__ se, double shots,
                   double* __restrict__ surv_out, double* __restrict__ var_out) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int n = dim - 1;
    const double* er = e + (size_t)s * n;
    const double* sr = se + (size_t)s * n;
    double sum = 0.0, sq = 0.0;
    for (int i = 0; i < n; ++i) { sum += er[i]; sq = fma(sr[i], sr[i], sq); }
    const double dd = (double)dim * (double)dim;
    double var = sq / dd;
    if (dim > 2 && shots > 0.0) {                                     // the pairwise covariances of observables from one set of shots
        double cross = 0.0;
        for (int i = 0; i < n; ++i) {
            double inner = 0.0;
            for (int j = 0; j < n; ++j) inner += (j != i) ? er[j] : 0.0;
            cross = fma(er[i], inner, cross);
        }
        var += ((2.0 * sum - cross) / shots) / dd;
    }
    if (surv_out) surv_out[s] = (sum + 1.0) / (double)dim;
    if (var_out) var_out[s] = var;
}

__global__ void __launch_bounds__(256)
rb_purity_kernel(int dim, long long S, const double* __restrict__ e, const double* __restrict__ se, int renorm,
                 double* __restrict__ purity_out, double* __restrict__ err_out) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int n = dim * dim - 1;
    const double* er = e + (size_t)s * n;
    const double* sr = se + (size_t)s * n;
    double sum = 1.0, vs = 0.0;                                       // the identity: expectation 1, variance 0
    for (int i = 0; i < n; ++i) {
        const double x = er[i], var = sr[i] * sr[i];
        sum = fma(x, x, sum);
        const double t = 2.0 * fabs(x);
        double v = t * t * var;
        if (fabs(v) <= 1e-6 + 1e-5 * fabs(v)) v = var * var;         // numpy.isclose(0, v, atol=1e-6) with the default rtol
        vs += v;
    }
    const double d = (double)dim;
    double purity = sum / d, pvar = vs / (d * d);
    if (renorm) {
        const double f = d / (d - 1.0);
        purity = f * (purity - 1.0 / d);
        pvar *= f * f;
    }
    if (purity_out) purity_out[s] = purity;
    if (err_out) err_out[s] = sqrt(pvar);
}

// weights 1 / err with every error that is not above zero replaced by the item's smallest one that is (none: unit weights,
// has_weights = 0), and the default (amplitude, decay, baseline) guess of the decay fit.  "Not above zero" includes the NaN that
// the square root of a negative variance gives -- the covariance sum of fbx_rb_survival can be negative -- as the reference's
// `v if v > 0 else min_non_zero` does.
__global__ void __launch_bounds__(256)
fit_prepare_kernel(int kind, long long B, int K, const double* __restrict__ values, const double* __restrict__ errs,
                   int errs_are_variances, double* __restrict__ weights_out, double* __restrict__ guess_out,
                   int* __restrict__ has_weights_out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* v = values + (size_t)b * K;
    if (guess_out) {
        double* gq = guess_out + (size_t)b * 3;
        if (kind == FBX_FIT_PREPARE_RB) { gq[0] = v[0] - v[K - 1]; gq[1] = 0.95; gq[2] = v[K - 1]; }
        else { gq[0] = v[0]; gq[1] = 0.95; gq[2] = 0.0; }
    }
    if (!errs) return;
    const double* er = errs + (size_t)b * K;
    double mn = 0.0;
    bool any = false;
    for (int k = 0; k < K; ++k) {
        const double x = errs_are_variances ? sqrt(er[k]) : er[k];
        if (x > 0.0 && (!any || x < mn)) { mn = x; any = true; }
    }
    if (weights_out)
        for (int k = 0; k < K; ++k) {
            const double x = errs_are_variances ? sqrt(er[k]) : er[k];
            weights_out[(size_t)b * K + k] = any ? 1.0 / (x > 0.0 ? x : mn) : 1.0;
        }
    if (has_weights_out) has_weights_out[b] = any ? 1 : 0;
}

static int fit_check(int model, int64_t B, int K, const void* x, int64_t x_stride, const void* y, const void* guess, unsigned vary,
                     double ftol, double xtol, int max_iters) {
    const int P = fit_param_count(model);
    FBX_REQUIRE(P != 0, "fbx_curve_fit: unknown model id (FBX_FIT_BASE_DECAY .. FBX_FIT_SHIFTED_COSINE)");
    FBX_REQUIRE(B >= 0, "fbx_curve_fit: need B >= 0");
    FBX_REQUIRE(K >= 2, "fbx_curve_fit: need at least 2 points per fit");
    if (K > FBX_FIT_MAX_POINTS) {
        set_error("fbx_curve_fit: at most " + std::to_string(FBX_FIT_MAX_POINTS) + " points per fit (got " + std::to_string(K) + ")");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_REQUIRE(x_stride == 0 || x_stride == K, "fbx_curve_fit: x_stride must be 0 (one x for the batch) or K (one row per item)");
    FBX_REQUIRE((vary >> P) == 0u, "fbx_curve_fit: vary has bits beyond the model's parameters");
    FBX_REQUIRE(ftol >= 0.0 && xtol >= 0.0 && max_iters >= 0, "fbx_curve_fit: need ftol >= 0, xtol >= 0, max_iters >= 0");
    FBX_REQUIRE(B == 0 || (x && y && guess), "fbx_curve_fit: NULL x / y / guess");
    return FBX_OK;
}

static int rb_check(const char* who, int dim, int max_dim, int64_t S, const void* expectations, const void* std_errs) {
    if (dim < 2 || dim > max_dim || (dim & (dim - 1))) {
        set_error(std::string(who) + ": dim must be a power of two in 2.." + std::to_string(max_dim) + " (got " + std::to_string(dim) + ")");
        return (dim > max_dim && !(dim & (dim - 1))) ? FBX_ERR_UNSUPPORTED : FBX_ERR_BAD_ARG;
    }
    FBX_REQUIRE(S >= 0, std::string(who) + ": need S >= 0");
    FBX_REQUIRE(S == 0 || (expectations && std_errs), std::string(who) + ": NULL expectations / std_errs");
    return FBX_OK;
}

static int rb_survival_check(int dim, int64_t S, const void* expectations, const void* std_errs, int64_t num_shots) {
    FBX_TRY(rb_check("fbx_rb_survival", dim, 32, S, expectations, std_errs));
    FBX_REQUIRE(num_shots >= 0, "fbx_rb_survival: need num_shots >= 0 (0: the observables are independent)");
    return FBX_OK;
}

static unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace fbx

using namespace fbx;

extern "C" {

int fbx_curve_fit_dev(int model, int64_t B, int K, const double* d_x, int64_t x_stride, const double* d_y, const double* d_weights,
                      const double* d_guess, unsigned vary, double ftol, double xtol, int max_iters, double* d_params_out,
                      double* d_covar_out, double* d_chisqr_out, double* d_redchi_out, int32_t* d_iters_out, int32_t* d_status_out,
                      double* d_grad_norm_out) {
    FBX_TRY(fit_check(model, B, K, d_x, x_stride, d_y, d_guess, vary, ftol, xtol, max_iters));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t plane = sizeof(double) * (size_t)B * (size_t)K;
    const int planes = 1 + (d_weights ? 1 : 0) + (x_stride ? 1 : 0);
    void* ws = nullptr;
    FBX_TRY(workspace(WS_FIT, plane * planes, &ws));
    double* yT = reinterpret_cast<double*>(ws);
    double* wT = d_weights ? yT + (size_t)B * K : nullptr;
    double* xT = x_stride ? yT + (size_t)B * K * (d_weights ? 2 : 1) : nullptr;
    const dim3 tgrid((unsigned)((B + 31) / 32), (unsigned)((K + 31) / 32)), tblock(32, 8);
    hipLaunchKernelGGL(fit_transpose_kernel, tgrid, tblock, 0, stream(), (long long)B, K, d_y, yT);
    if (wT) hipLaunchKernelGGL(fit_transpose_kernel, tgrid, tblock, 0, stream(), (long long)B, K, d_weights, wT);
    if (xT) hipLaunchKernelGGL(fit_transpose_kernel, tgrid, tblock, 0, stream(), (long long)B, K, d_x, xT);
    FitData da{x_stride ? nullptr : d_x, xT, yT, wT, (size_t)B, K};
    switch (model) {
#define FBX_FIT_LAUNCH(M)                                                                                                        \
        case M:                                                                                                                  \
            hipLaunchKernelGGL(fit_kernel<M>, dim3(grid_for(B)), dim3(256), 0, stream(), (long long)B, da, d_guess, vary, ftol,  \
                               xtol, max_iters, d_params_out, d_covar_out, d_chisqr_out, d_redchi_out, (int*)d_iters_out,        \
                               (int*)d_status_out, d_grad_norm_out);                                                             \
            break
        FBX_FIT_LAUNCH(FBX_FIT_BASE_DECAY); FBX_FIT_LAUNCH(FBX_FIT_TIME_DECAY);
        FBX_FIT_LAUNCH(FBX_FIT_DECAYING_COSINE); FBX_FIT_LAUNCH(FBX_FIT_SHIFTED_COSINE);
#undef FBX_FIT_LAUNCH
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_curve_fit(int model, int64_t B, int K, const double* x, int64_t x_stride, const double* y, const double* weights,
                  const double* guess, unsigned vary, double ftol, double xtol, int max_iters, double* params_out,
                  double* covar_out, double* chisqr_out, double* redchi_out, int32_t* iters_out, int32_t* status_out,
                  double* grad_norm_out) {
    FBX_TRY(fit_check(model, B, K, x, x_stride, y, guess, vary, ftol, xtol, max_iters));
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    const size_t P = (size_t)fit_param_count(model), n = (size_t)B, nk = n * (size_t)K, nx = x_stride ? nk : (size_t)K;
    HostIO io; double *dx, *dy, *dg, *dw = nullptr, *dpar, *dcov, *dchi, *dred, *dgn; int32_t *dit, *dst;
    FBX_TRY(io.in(x, nx, &dx)); FBX_TRY(io.in(y, nk, &dy)); FBX_TRY(io.in(guess, n * P, &dg));
    if (weights) FBX_TRY(io.in(weights, nk, &dw));
    FBX_TRY(io.out_opt(params_out, n * P, &dpar)); FBX_TRY(io.out_opt(covar_out, n * P * P, &dcov));
    FBX_TRY(io.out_opt(chisqr_out, n, &dchi)); FBX_TRY(io.out_opt(redchi_out, n, &dred));
    FBX_TRY(io.out_opt(iters_out, n, &dit)); FBX_TRY(io.out_opt(status_out, n, &dst));
    FBX_TRY(io.out_opt(grad_norm_out, n, &dgn));
    FBX_TRY(fbx_curve_fit_dev(model, B, K, dx, x_stride, dy, dw, dg, vary, ftol, xtol, max_iters, dpar, dcov, dchi, dred, dit, dst, dgn));
    return io.finish();
}

int fbx_rb_survival_dev(int dim, int64_t S, const double* d_expectations, const double* d_std_errs, int64_t num_shots,
                        double* d_survival_out, double* d_variance_out) {
    FBX_TRY(rb_survival_check(dim, S, d_expectations, d_std_errs, num_shots));
    FBX_TRY(ensure_device());
    if (S == 0) return FBX_OK;
    hipLaunchKernelGGL(rb_survival_kernel, dim3(grid_for(S)), dim3(256), 0, stream(), dim, (long long)S, d_expectations, d_std_errs,
                       (double)num_shots, d_survival_out, d_variance_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rb_survival(int dim, int64_t S, const double* expectations, const double* std_errs, int64_t num_shots,
                    double* survival_out, double* variance_out) {
    FBX_TRY(rb_survival_check(dim, S, expectations, std_errs, num_shots));
    FBX_TRY(ensure_device());
    if (S == 0) return FBX_OK;
    const size_t n = (size_t)S, row = n * (size_t)(dim - 1);
    HostIO io; double *de, *ds, *dp, *dv;
    FBX_TRY(io.in(expectations, row, &de)); FBX_TRY(io.in(std_errs, row, &ds));
    FBX_TRY(io.out(survival_out, n, &dp)); FBX_TRY(io.out(variance_out, n, &dv));
    FBX_TRY(fbx_rb_survival_dev(dim, S, de, ds, num_shots, dp, dv));
    return io.finish();
}

int fbx_rb_purity_dev(int dim, int64_t S, const double* d_expectations, const double* d_std_errs, int renorm, double* d_purity_out,
                      double* d_purity_err_out) {
    FBX_TRY(rb_check("fbx_rb_purity", dim, 8, S, d_expectations, d_std_errs));
    FBX_TRY(ensure_device());
    if (S == 0) return FBX_OK;
    hipLaunchKernelGGL(rb_purity_kernel, dim3(grid_for(S)), dim3(256), 0, stream(), dim, (long long)S, d_expectations, d_std_errs,
                       renorm, d_purity_out, d_purity_err_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int fbx_rb_purity(int dim, int64_t S, const double* expectations, const double* std_errs, int renorm, double* purity_out,
                  double* purity_err_out) {
    FBX_TRY(rb_check("fbx_rb_purity", dim, 8, S, expectations, std_errs));
    FBX_TRY(ensure_device());
    if (S == 0) return FBX_OK;
    const size_t n = (size_t)S, row = n * (size_t)(dim * dim - 1);
    HostIO io; double *de, *ds, *dp, *dv;
    FBX_TRY(io.in(expectations, row, &de)); FBX_TRY(io.in(std_errs, row, &ds));
    FBX_TRY(io.out(purity_out, n, &dp)); FBX_TRY(io.out(purity_err_out, n, &dv));
    FBX_TRY(fbx_rb_purity_dev(dim, S, de, ds, renorm, dp, dv));
    return io.finish();
}

int fbx_fit_prepare_dev(int kind, int64_t B, int K, const double* d_values, const double* d_errors, int errors_are_variances,
                        double* d_weights_out, double* d_guess_out, int32_t* d_has_weights_out) {
    FBX_REQUIRE(kind == FBX_FIT_PREPARE_RB || kind == FBX_FIT_PREPARE_UNITARITY, "fbx_fit_prepare: unknown kind");
    FBX_REQUIRE(B >= 0 && K >= 1, "fbx_fit_prepare: need B >= 0 and K >= 1");
    FBX_REQUIRE(B == 0 || d_values, "fbx_fit_prepare: NULL values");
    FBX_REQUIRE(d_errors || (!d_weights_out && !d_has_weights_out), "fbx_fit_prepare: weights asked for without errors");
    FBX_TRY(ensure_device());
    if (B == 0) return FBX_OK;
    hipLaunchKernelGGL(fit_prepare_kernel, dim3(grid_for(B)), dim3(256), 0, stream(), kind, (long long)B, K, d_values, d_errors,
                       errors_are_variances, d_weights_out, d_guess_out, (int*)d_has_weights_out);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

}  // extern "C"
