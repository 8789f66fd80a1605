// fbx_state.hip -- batched state-tomography estimators on d x d (d = 2^n, n <= 5) density matrices: linear inversion,
// diluted iterative MLE with its max-entropy and hedged variants, the R operator and the log-likelihood.  Pauli
// expectations and the R operator are evaluated through the sparsity of the Pauli matrices (P_p[r][c] != 0 iff
// c = r ^ x_p), never by building d x d operators.
//   1-3 qubits: one 64-lane wavefront per item (WaveTeam), or, for the plain 1-2 qubit reconstruction, a group of d*d lanes
//   per item (GroupTeam);  4-5 qubits: one workgroup of d*d threads per item (BlockTeam).
// The update rule, its two variants and the R operator are written once over the team (fbx_state_core.hpp); the kernels
// keep their own control flow.  The work after a reconstruction (physical projection, state measures, the Pauli vector) is
// fbx_state_measures.hip; the general eigensolver, matrix product and choi2kraus live in fbx_linalg.hip.
//
// Reference functions (file:line under forest/benchmarking/):
//   linear_inv_state_estimate        tomography.py:130-165
//   iterative_mle_state_estimate     tomography.py:168-270   (+ _R, :273-338)
//   state_log_likelihood             tomography.py:341-375
#include "fbx_state_core.hpp"
#include <string>

namespace fbx {

// One setting of the design held by a lane for the whole reconstruction (designs of at most 64
// settings -- every state-tomography design of the reference has 4^n - 1 <= 63): Pauli index,
// coefficient and measured expectation are fetched from HBM once instead of once per iteration.
struct LaneSetting { int p; double cf, e; bool valid; };
__device__ __forceinline__ LaneSetting load_lane_setting(const DesignDev& des, const double* __restrict__ e, int lane) {
    LaneSetting s; s.valid = des.m <= 64 && lane < des.m; s.p = 0; s.cf = 1.0; s.e = 0.0;
    if (s.valid) { s.p = des.sp[lane] & 0xffff; s.cf = des.unit_coefs ? 1.0 : des.coef[lane]; s.e = e[des.order[lane]]; }
    return s;
}

// One setting of the R operator (tomography.py:326-336): from its coefficient, the measured expectation `me` and the state's
// expectation `pe` of its observable, the half-sum of the two outcome ratios (the identity's weight) and their half-difference
// times the coefficient (the observable's weight).  (0.5 * x is exact, so a sum that adds `hs` rounds as one that fuses the product.)
struct SettingRatio { double hs, hd; };
__device__ __forceinline__ SettingRatio setting_ratio(double cf, double me, double pe) {
    const double gp = ((1.0 + me) * 0.5) / ((1.0 + pe) * 0.5 + DBL_MIN);
    const double gm = ((1.0 - me) * 0.5) / ((1.0 - pe) * 0.5 + DBL_MIN);
    SettingRatio q; q.hs = 0.5 * (gp + gm); q.hd = cf * 0.5 * (gp - gm);
    return q;
}

// This thread's share of the log-likelihood (log10) of tomography.py:341-375: settings t, t + NT, ... of one item (`e`, `cnt`: its
// expectations and counts), r = the state's Pauli expectations
template <int NT>
__device__ __forceinline__ double loglik_partial(const DesignDev& des, const double* __restrict__ e, const double* __restrict__ cnt,
                                                 const double* r, int t) {
    double ll = 0.0;
    for (int g = t; g < des.m; g += NT) {
        const int k = des.order[g], p = des.sp[g] & 0xffff;
        const double cf = des.unit_coefs ? 1.0 : des.coef[g];
        const double n = cnt[k], me = e[k], pe = cf * r[p];
        const double pp = (1.0 + pe) / 2, pm = (1.0 - pe) / 2;
        if (pp > 0.0) ll += n * (1.0 + me) / 2 * log10(pp);
        if (pm > 0.0) ll += n * (1.0 - me) / 2 * log10(pm);
    }
    return ll;
}

// R operator of tomography.py:273-338 for the state in `rho`; result element of this thread.  Two forms.
// ONE SETTING RESIDENT PER THREAD (`mine`; designs of at most as many settings as the team has threads), the Pauli passes as
// tables: what the iterative-MLE loops of 1-3 qubits run.
template <class Team, class Tables>
__device__ __forceinline__ cplx r_operator_resident(const Team& tm, int t, int m, const cplx* rho, double* r, double* w,
                                                    const LaneSetting& mine, const Tables& tab) {
    if (tm.active(t)) { r[t] = tab.expectation(rho); w[t] = 0.0; }
    tm.sync();
    double s0 = 0.0;
    if (mine.valid) {
        const SettingRatio q = setting_ratio(mine.cf, mine.e, mine.cf * r[mine.p]);
        s0 = q.hs;
        atomicAdd(&w[mine.p], q.hd);
    }
    s0 = tm.sum(s0);
    if (tm.active(t)) w[t] = w[t] / m;
    tm.sync();
    cplx out; out.re = 0.0; out.im = 0.0;
    if (tm.active(t)) out = tab.synthesis(w, s0 / m + 0.0, tm.diag(t));
    return out;
}

// SETTINGS WALKED IN STRIDES OF THE TEAM SIZE: any number of settings (the reference loops over whatever list it is given,
// tomography.py:326-336).  The weighted half-differences are STAGED in `hd` (a wavefront, up to 64 KiB of per-setting scratch:
// StateLds::staged) and thread p adds those of its Pauli in setting order; without staging (`hd` NULL) they are STREAMED: added
// to w[p] with LDS atomics as every thread walks its settings (one wavefront: the same order in every run; a workgroup: the same
// result only while no two settings measure the same Pauli operator, as in every design of the reference).  Ends behind a sync.
template <int NQ, class Team>
__device__ cplx r_operator_strided(const Team& tm, int t, const DesignDev& des, const double* __restrict__ e, const cplx* rho, double* r,
                                   double* w, double* hs, double* hd) {
    constexpr int d = 1 << NQ;
    const int m = des.m;
    const bool staged = Team::NT == 64 && hd != nullptr;
    pauli_expectations<NQ>(rho, r, t);
    if (!staged && tm.active(t)) w[t] = 0.0;
    tm.sync();
    double s0 = 0.0;
    for (int g = t; g < m; g += Team::NT) {
        const int p = des.sp[g] & 0xffff;
        const double cf = des.unit_coefs ? 1.0 : des.coef[g];
        const SettingRatio q = setting_ratio(cf, e[des.order[g]], cf * r[p]);
        if (staged) { hs[g] = q.hs; hd[g] = q.hd; }
        else atomicAdd(&w[p], q.hd);
        s0 += q.hs;
    }
    s0 = tm.sum(s0);                                    // (the atomics above are complete behind it)
    if (tm.active(t)) {
        double acc = 0.0;
        if (staged) { for (int g = 0; g < m; ++g) if ((int)(des.sp[g] & 0xffff) == t) acc += hd[g]; }
        else acc = w[t];
        w[t] = acc / m;
    }
    tm.sync();
    cplx out; out.re = 0.0; out.im = 0.0;
    if (tm.active(t)) out = pauli_synthesis<NQ>(w, s0 / m + 0.0, t / d, t % d);
    // identity-observable settings contribute through w[0] as well as through s0: P_0 = I
    tm.sync();
    return out;
}

// ---- The diluted update of tomography.py:262-268, once for every team: U = I + epsilon Tk, rho' = U rho U / tr(U rho U).
// `rho`: this thread's entry of the state that is staged in `rho_s`; U and tmp: [D] of LDS.  Returns the thread's entry of rho'
// and, in step2, the squared Frobenius norm of rho' - rho; the caller stores rho' and decides whether to go on.
template <class Team>
__device__ __forceinline__ cplx diluted_update(const Team& tm, int t, const cplx T, double epsilon, const cplx rho, const cplx* rho_s,
                                               cplx* U, cplx* tmp, double& step2) {
    const bool act = tm.active(t), diag = tm.diag(t);
    cplx Um; Um.re = epsilon * T.re + (diag ? 1.0 : 0.0); Um.im = epsilon * T.im;
    tm.sync();
    if (act) U[t] = Um;
    tm.sync();
    const cplx t1 = team_matmul(tm, t, rho_s, U);                 // rho U
    if (act) tmp[t] = t1;
    tm.sync();
    cplx nr = team_matmul(tm, t, U, tmp);                       // U rho U
    double tr_re = diag ? nr.re : 0.0, tr_im = diag ? nr.im : 0.0;
    tr_re = tm.sum(tr_re); tr_im = tm.sum(tr_im);
    nr = div_by_trace(nr, tr_re, tr_im);
    step2 = tm.sum(act ? (nr.re - rho.re) * (nr.re - rho.re) + (nr.im - rho.im) * (nr.im - rho.im) : 0.0);
    return nr;
}

// The two variants, on Tk = R - I of the state in L.rho (L: StateLds or StateBigLds).
// Entropy penalty, tomography.py:252-254: Tk -= penalty * (logm(rho) - tr(rho logm(rho)) I)
template <class Team, class Lds>
__device__ __forceinline__ void entropy_term(const Team& tm, int t, Lds& L, double entropy_penalty, cplx& T) {
    herm_function<false>(tm, t, L.rho, L.aux, 0, L);              // logm(rho)
    cplx lg; lg.re = 0.0; lg.im = 0.0;
    if (tm.active(t)) lg = L.aux[t];
    const cplx rl = team_matmul(tm, t, L.rho, L.aux);           // rho @ logm(rho)
    double tr_re = tm.diag(t) ? rl.re : 0.0, tr_im = tm.diag(t) ? rl.im : 0.0;
    tr_re = tm.sum(tr_re); tr_im = tm.sum(tr_im);
    if (tm.diag(t)) { lg.re -= tr_re; lg.im -= tr_im; }
    T.re -= entropy_penalty * lg.re; T.im -= entropy_penalty * lg.im;
}
// Hedging, tomography.py:257-260: Tk = Tk * num_meas / 2 + beta / 2 * (pinv(rho) - d I)
template <class Team, class Lds>
__device__ __forceinline__ void hedging_term(const Team& tm, int t, Lds& L, double beta, double num_meas, cplx& T) {
    T.re *= num_meas / 2; T.im *= num_meas / 2;
    herm_function<false>(tm, t, L.rho, L.aux, 1, L);              // pinv(rho)
    cplx pi; pi.re = 0.0; pi.im = 0.0;
    if (tm.active(t)) pi = L.aux[t];
    if (tm.diag(t)) pi.re -= Team::d;
    T.re += beta * pi.re / 2; T.im += beta * pi.im / 2;
}

// ---------------------------------------------------------------------------------------------
// PLAIN: no entropy penalty, no hedging, a design of at most 64 settings (every state design of the reference) -- the variants'
// code (two Hermitian matrix functions through the Jacobi) is compiled out
template <int NQ, bool PLAIN, class Tables>
__device__ __forceinline__ void
mle_state_body(char* smem, const DesignDev& des, const double* __restrict__ expect, const double* __restrict__ counts,
               double epsilon, double entropy_penalty, double beta, double tol, int maxiter,
               double* __restrict__ rho_out, int* __restrict__ iters_out, int* __restrict__ hit_out) {
    constexpr int d = 1 << NQ, D = d * d;
    const bool staged = StateLds<NQ>::staged(des.m);
    StateLds<NQ> L; L.carve(smem, staged ? des.m : 0);
    const int lane = threadIdx.x;
    const WaveTeam<NQ> tm;
    const long long item = blockIdx.x;
    const double* e = expect + item * des.m;
    const bool act = lane < D;
    const int row = act ? lane / d : 0, col = act ? lane % d : 0;
    double num_meas = 0.0;
    for (int g = lane; g < des.m; g += 64) num_meas += counts[item * des.m + g];
    num_meas = wave_sum(num_meas);
    cplx rho; rho.re = (act && row == col) ? 1.0 / d : 0.0; rho.im = 0.0;
    if (act) L.rho[lane] = rho;
    FBX_WAVE_SYNC();
    const LaneSetting mine = load_lane_setting(des, e, lane);
    Tables tab; tab.init(act ? lane : 0, row, col);
    int iteration = 1, hit = 0;
    while (true) {
        if (iteration >= maxiter) { hit = 1; break; }            // tomography.py:244-246
        cplx T;                                                    // R(rho)
        if constexpr (PLAIN) T = r_operator_resident(tm, lane, des.m, L.rho, L.r, L.w, mine, tab);
        else T = des.m <= 64 ? r_operator_resident(tm, lane, des.m, L.rho, L.r, L.w, mine, tab)
                             : r_operator_strided<NQ>(tm, lane, des, e, L.rho, L.r, L.w, staged ? L.hs : nullptr, staged ? L.hd : nullptr);
        if (act && row == col) T.re -= 1.0;                        // Tk = R - I
        if (!PLAIN && entropy_penalty > 0.0) entropy_term(tm, lane, L, entropy_penalty, T);
        if (!PLAIN && beta > 0.0) hedging_term(tm, lane, L, beta, num_meas, T);
        double diff;
        rho = diluted_update(tm, lane, T, epsilon, rho, L.rho, L.U, L.tmp, diff);
        diff = uniform(diff);
        FBX_WAVE_SYNC();
        if (act) L.rho[lane] = rho;
        FBX_WAVE_SYNC();
        if (sqrt(diff) < tol) break;
        ++iteration;
    }
    if (act) { rho_out[(item * D + lane) * 2] = rho.re; rho_out[(item * D + lane) * 2 + 1] = rho.im; }
    if (lane == 0) { if (iters_out) iters_out[item] = iteration; if (hit_out) hit_out[item] = hit; }
}

template <int NQ>
__global__ void __launch_bounds__(64)
mle_state_kernel(DesignDev des, const double* __restrict__ expect, const double* __restrict__ counts,
                 double epsilon, double entropy_penalty, double beta, double tol, int maxiter,
                 double* __restrict__ rho_out, int* __restrict__ iters_out, int* __restrict__ hit_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    mle_state_body<NQ, false, PauliTables<NQ>>(smem, des, expect, counts, epsilon, entropy_penalty, beta, tol, maxiter, rho_out, iters_out, hit_out);
}

// The plain 3-qubit reconstruction (what bench.py --workload mle_state3 times): the body without the variants and with the ordered
// tables (PauliTablesLean: d indices + d signs per pass instead of d + 2 d coefficients), held to 128 registers = FOUR wavefronts per
// SIMD -- with the tables of PauliTables it needs 236 registers (two wavefronts), and two wavefronts do not fill the vector pipe
// (docs/history/experiments.md has the measurements).
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
mle_state_plain3_kernel(DesignDev des, const double* __restrict__ expect, const double* __restrict__ counts,
                        double epsilon, double tol, int maxiter, double* __restrict__ rho_out, int* __restrict__ iters_out,
                        int* __restrict__ hit_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    mle_state_body<3, true, PauliTablesLean<3>>(smem, des, expect, counts, epsilon, 0.0, 0.0, tol, maxiter, rho_out, iters_out, hit_out);
}

// ---- plain diluted MLE (no entropy penalty, no hedging) for 1 and 2 qubits with SEVERAL items per
// wavefront: a d x d state needs d^2 = 4 / 16 lanes, so 16 / 4 reconstructions share a wave, each in
// its own group of D consecutive lanes (GroupTeam) with its own slice of LDS.  Needs m <= D settings (every
// state-tomography design of the reference has 4^n - 1); groups that have converged idle until the
// last one of the wave has.  Same arithmetic per item as mle_state_kernel.
template <int NQ>
__global__ void __launch_bounds__(64)
mle_state_packed_kernel(DesignDev des, long long B, const double* __restrict__ expect, double epsilon, double tol,
                        int maxiter, double* __restrict__ rho_out, int* __restrict__ iters_out, int* __restrict__ hit_out) {
    constexpr int d = 1 << NQ, D = d * d, G = 64 / D;
    static_assert(D == 4 || D == 16, "one or two qubits");
    __shared__ cplx s_rho[G * D], s_U[G * D], s_tmp[G * D];
    __shared__ double s_r[G * D], s_w[G * D];
    const int lane = threadIdx.x, sub = lane / D;
    const GroupTeam<NQ> tm;
    const int t = lane % D, row = t / d, col = t % d;
    const long long item = (long long)blockIdx.x * G + sub;
    const bool valid = item < B;
    const int m = des.m;
    cplx* rho_l = s_rho + sub * D; cplx* U_l = s_U + sub * D; cplx* tmp_l = s_tmp + sub * D;
    double* r_l = s_r + sub * D; double* w_l = s_w + sub * D;
    LaneSetting mine; mine.valid = valid && t < m; mine.p = 0; mine.cf = 1.0; mine.e = 0.0;      // this lane's setting (t < m <= D)
    if (mine.valid) { mine.p = des.sp[t] & 0xffff; mine.cf = des.unit_coefs ? 1.0 : des.coef[t]; mine.e = expect[item * m + des.order[t]]; }
    cplx rho; rho.re = (row == col) ? 1.0 / d : 0.0; rho.im = 0.0;
    rho_l[t] = rho;
    FBX_WAVE_SYNC();
    PauliTables<NQ> tab; tab.init(t, row, col);
    int iteration = 1, hit = 0;
    bool running = valid;
    while (__ballot(running)) {
        if (running && iteration >= maxiter) { hit = 1; running = false; }     // tomography.py:244-246
        if (!__ballot(running)) break;
        cplx T = r_operator_resident(tm, t, m, rho_l, r_l, w_l, mine, tab);
        if (row == col) T.re -= 1.0;                                           // Tk = R - I
        // (the update of diluted_update, spelled out: through the shared form the 2-qubit loop is scheduled differently, and
        // bench.py --workload mle_state left the parent's range by 0.1 % in one of two sessions; profiles/r15/ab_summary.txt)
        cplx Um; Um.re = epsilon * T.re + ((row == col) ? 1.0 : 0.0); Um.im = epsilon * T.im;
        FBX_WAVE_SYNC();
        U_l[t] = Um;
        FBX_WAVE_SYNC();
        const cplx t1 = team_matmul(tm, t, rho_l, U_l);                         // rho U
        tmp_l[t] = t1;
        FBX_WAVE_SYNC();
        cplx nr = team_matmul(tm, t, U_l, tmp_l);                               // U rho U
        const double tr_re = group_sum<D>((row == col) ? nr.re : 0.0), tr_im = group_sum<D>((row == col) ? nr.im : 0.0);
        nr = div_by_trace(nr, tr_re, tr_im);
        const double diff = group_sum<D>((nr.re - rho.re) * (nr.re - rho.re) + (nr.im - rho.im) * (nr.im - rho.im));
        FBX_WAVE_SYNC();
        if (running) { rho = nr; rho_l[t] = rho; }
        FBX_WAVE_SYNC();
        if (running) {
            if (sqrt(diff) < tol) running = false; else ++iteration;
        }
    }
    if (valid) {
        rho_out[(item * D + t) * 2] = rho.re; rho_out[(item * D + t) * 2 + 1] = rho.im;
        if (t == 0) { if (iters_out) iters_out[item] = iteration; if (hit_out) hit_out[item] = hit; }
    }
}

template <int NQ>
__global__ void __launch_bounds__(64)
r_operator_kernel(DesignDev des, const double* __restrict__ rho_in, const double* __restrict__ expect, double* __restrict__ r_out) {
    constexpr int d = 1 << NQ, D = d * d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool staged = StateLds<NQ>::staged(des.m);
    StateLds<NQ> L; L.carve(smem, staged ? des.m : 0);
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    if (lane < D) { L.rho[lane].re = rho_in[(item * D + lane) * 2]; L.rho[lane].im = rho_in[(item * D + lane) * 2 + 1]; }
    FBX_WAVE_SYNC();
    const cplx R = r_operator_strided<NQ>(WaveTeam<NQ>(), lane, des, expect + item * des.m, L.rho, L.r, L.w, staged ? L.hs : nullptr,
                                          staged ? L.hd : nullptr);
    if (lane < D) { r_out[(item * D + lane) * 2] = R.re; r_out[(item * D + lane) * 2 + 1] = R.im; }
}

// log-likelihood (log10), tomography.py:341-375
template <int NQ>
__global__ void __launch_bounds__(64)
loglik_kernel(DesignDev des, const double* __restrict__ rho_in, const double* __restrict__ expect,
              const double* __restrict__ counts, double* __restrict__ ll_out) {
    constexpr int d = 1 << NQ, D = d * d;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    StateLds<NQ> L; L.carve(smem, des.m);
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    if (lane < D) { L.rho[lane].re = rho_in[(item * D + lane) * 2]; L.rho[lane].im = rho_in[(item * D + lane) * 2 + 1]; }
    FBX_WAVE_SYNC();
    pauli_expectations<NQ>(L.rho, L.r, lane);
    FBX_WAVE_SYNC();
    const double ll = wave_sum(loglik_partial<64>(des, expect + item * des.m, counts + item * des.m, L.r, lane));
    if (lane == 0) ll_out[item] = ll;
}

// linear inversion, tomography.py:130-165: per Pauli a least-squares coefficient, then synthesis
template <int NQ>
__global__ void __launch_bounds__(64)
linv_state_kernel(DesignDev des, const double* __restrict__ expect, double* __restrict__ rho_out) {
    constexpr int d = 1 << NQ, D = d * d;
    __shared__ double w[D];
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    if (lane < D) {
        double num = 0.0, den = 0.0;
        for (int g = 0; g < des.m; ++g) {
            if ((int)(des.sp[g] & 0xffff) != lane) continue;
            const double cf = des.unit_coefs ? 1.0 : des.coef[g];
            num += cf * expect[item * des.m + des.order[g]];
            den += cf * cf;
        }
        w[lane] = den > 0.0 ? num / (den * d) : 0.0;     // pinv of orthogonal rows c_k vec(P)^H
    }
    FBX_WAVE_SYNC();
    if (lane < D) {
        const cplx v = pauli_synthesis<NQ>(w, 1.0 / d, lane / d, lane % d);   // + I/d, tomography.py:165
        rho_out[(item * D + lane) * 2] = v.re; rho_out[(item * D + lane) * 2 + 1] = v.im;
    }
}

}  // namespace fbx

using namespace fbx;


// =====================================================================================================
// 4 and 5 qubits (16 x 16 and 32 x 32 density matrices, 255 / 1023 settings): ONE WORKGROUP OF d*d THREADS per state
// (256 / 1024), thread t owns matrix entry (t / d, t % d) as a lane does above: the same update, variants and R operator over
// a BlockTeam -- workgroup barriers and workgroup sums.  A 16 x 16 density matrix has the size of a 2-qubit Choi matrix: its
// Hermitian functions (logm for the entropy penalty, pinv for hedging) run on the solver of the 2- / 3-qubit process kernels
// (jacobi_eigh_simple<d, NT>).  Weights of the R operator are summed with LDS atomics (several settings on the same Pauli
// operator -- not in the reference's designs -- would add in an order that differs between runs at rounding level).
template <int NQ>
struct StateBigLds {
    static constexpr int d = 1 << NQ, D = d * d, NT = D;
    cplx *rho, *U, *tmp, *aux, *Ms, *Vs;
    double *w, *r, *lam, *red;
    static constexpr size_t bytes() { return sizeof(cplx) * (4 * (size_t)D + 2 * (size_t)sys_elems<d>()) + sizeof(double) * (2 * (size_t)D + d + 2 * (NT / 64) + 8); }
    __device__ void carve(char* p) {
        rho = (cplx*)p; p += sizeof(cplx) * D;  U = (cplx*)p; p += sizeof(cplx) * D;
        tmp = (cplx*)p; p += sizeof(cplx) * D;  aux = (cplx*)p; p += sizeof(cplx) * D;
        Ms = (cplx*)p; p += sizeof(cplx) * sys_elems<d>();  Vs = (cplx*)p; p += sizeof(cplx) * sys_elems<d>();
        w = (double*)p; p += sizeof(double) * D; r = (double*)p; p += sizeof(double) * D;
        lam = (double*)p; p += sizeof(double) * d; red = (double*)p;
    }
};

// iterative_mle_state_estimate, tomography.py:168-270: the loop of mle_state_body over a workgroup
template <int NQ>
__global__ void __launch_bounds__(1 << (2 * NQ))
mle_state_big_kernel(DesignDev des, const double* __restrict__ expect, const double* __restrict__ counts,
                     double epsilon, double entropy_penalty, double beta, double tol, int maxiter,
                     double* __restrict__ rho_out, int* __restrict__ iters_out, int* __restrict__ hit_out) {
    constexpr int d = 1 << NQ, D = d * d, NT = D;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    StateBigLds<NQ> L; L.carve(smem);
    const int t = threadIdx.x;
    const BlockTeam<NQ> tm{L.red};
    const long long item = blockIdx.x;
    const double* e = expect + item * des.m;
    const int row = t / d, col = t % d;
    double num_meas = 0.0;
    for (int g = t; g < des.m; g += NT) num_meas += counts[item * des.m + g];
    num_meas = tm.sum(num_meas);
    cplx rho; rho.re = (row == col) ? 1.0 / d : 0.0; rho.im = 0.0;
    L.rho[t] = rho;
    __syncthreads();
    int iteration = 1, hit = 0;
    while (true) {
        if (iteration >= maxiter) { hit = 1; break; }
        cplx T = r_operator_strided<NQ>(tm, t, des, e, L.rho, L.r, L.w, nullptr, nullptr);
        if (row == col) T.re -= 1.0;
        if (entropy_penalty > 0.0) entropy_term(tm, t, L, entropy_penalty, T);
        if (beta > 0.0) hedging_term(tm, t, L, beta, num_meas, T);
        double diff;
        rho = diluted_update(tm, t, T, epsilon, rho, L.rho, L.U, L.tmp, diff);
        __syncthreads();
        L.rho[t] = rho;
        __syncthreads();
        if (sqrt(diff) < tol) break;
        ++iteration;
    }
    rho_out[(item * D + t) * 2] = rho.re; rho_out[(item * D + t) * 2 + 1] = rho.im;
    if (t == 0) { if (iters_out) iters_out[item] = iteration; if (hit_out) hit_out[item] = hit; }
}

// op 0: R operator of a given state, 1: log-likelihood (log10) of a given state, 2: linear inversion
template <int NQ>
__global__ void __launch_bounds__(1 << (2 * NQ))
state_big_kernel(int op, DesignDev des, const double* __restrict__ rho_in, const double* __restrict__ expect,
                 const double* __restrict__ counts, double* __restrict__ out) {
    constexpr int d = 1 << NQ, D = d * d, NT = D;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    StateBigLds<NQ> L; L.carve(smem);
    const int t = threadIdx.x;
    const BlockTeam<NQ> tm{L.red};
    const long long item = blockIdx.x;
    const int m = des.m;
    if (op == 2) {                                         // tomography.py:130-165, as linv_state_kernel
        double* num = L.w; double* den = L.r;
        num[t] = 0.0; den[t] = 0.0;
        __syncthreads();
        for (int g = t; g < m; g += NT) {
            const int p = des.sp[g] & 0xffff;
            const double cf = des.unit_coefs ? 1.0 : des.coef[g];
            atomicAdd(&num[p], cf * expect[item * m + des.order[g]]);
            atomicAdd(&den[p], cf * cf);
        }
        __syncthreads();
        const double wv = den[t] > 0.0 ? num[t] / (den[t] * d) : 0.0;
        __syncthreads();
        L.w[t] = wv;
        __syncthreads();
        const cplx v = pauli_synthesis<NQ>(L.w, 1.0 / d, t / d, t % d);
        out[(item * D + t) * 2] = v.re; out[(item * D + t) * 2 + 1] = v.im;
        return;
    }
    L.rho[t].re = rho_in[(item * D + t) * 2]; L.rho[t].im = rho_in[(item * D + t) * 2 + 1];
    __syncthreads();
    if (op == 0) {
        const cplx R = r_operator_strided<NQ>(tm, t, des, expect + item * m, L.rho, L.r, L.w, nullptr, nullptr);
        out[(item * D + t) * 2] = R.re; out[(item * D + t) * 2 + 1] = R.im;
        return;
    }
    pauli_expectations<NQ>(L.rho, L.r, t);
    __syncthreads();
    const double ll = tm.sum(loglik_partial<NT>(des, expect + item * m, counts + item * m, L.r, t));
    if (t == 0) out[item] = ll;
}

namespace {
// state_big_kernel<4 | 5>: op as the kernel has it
template <int NQ>
int launch_state_big(int op, const fbx_design* des, int64_t B, const double* rho, const double* e, const double* c, double* out) {
    return launch_lds(state_big_kernel<NQ>, dim3((unsigned)B), dim3(1 << (2 * NQ)), StateBigLds<NQ>::bytes(), op, des->dev, rho, e, c, out);
}

// The argument checks of an entry point, shared by its device-pointer and its host-pointer form; *go = false for an empty batch.
// `buffers`: every required pointer is there; `both_variants`: entropy penalty and hedging at once (fbx_mle_state).
int check_call(const fbx_design* des, const char* who, int64_t B, bool buffers, bool* go, bool both_variants = false) {
    *go = false;
    { const int rc = check_design(des, who); if (rc) return rc; }
    if (des->dev.kind != FBX_KIND_STATE) { set_error(std::string(who) + ": needs a state design"); return FBX_ERR_BAD_ARG; }
    FBX_REQUIRE(!both_variants, "One can't sensibly do entropy penalty and hedging. Do one or the other but not both.");
    FBX_REQUIRE(B >= 0 && (B == 0 || buffers), std::string(who) + ": bad batch / NULL buffer");
    FBX_TRY(ensure_device());
    *go = B > 0;
    return FBX_OK;
}
}  // namespace

extern "C" {

// Every estimator below comes as a device-pointer form (`_dev`: checks + launch on the library
// stream, no synchronisation) and a host-pointer form (staging buffers, H2D, the `_dev` form, D2H, sync).

int fbx_linv_state_dev(const fbx_design* design, int64_t B, const double* d_expect, double* d_rho_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_linv_state", B, d_expect && d_rho_out, &go));
    if (!go) return FBX_OK;
    return with_qubits(design->dev.n, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if constexpr (NQ >= 4) return launch_state_big<NQ>(2, design, B, nullptr, d_expect, nullptr, d_rho_out);
        else return launch_lds(linv_state_kernel<NQ>, dim3((unsigned)B), dim3(64), 0, design->dev, d_expect, d_rho_out);
    });
}

int fbx_linv_state(const fbx_design* design, int64_t B, const double* expect, double* rho_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_linv_state", B, expect && rho_out, &go));
    if (!go) return FBX_OK;
    const size_t m = design->dev.m, D = design->dev.D;
    HostIO io; double *de, *dr;
    FBX_TRY(io.in(expect, m * B, &de)); FBX_TRY(io.out(rho_out, D * 2 * B, &dr));
    FBX_TRY(fbx_linv_state_dev(design, B, de, dr));
    return io.finish();
}

// With D = 4^n, m settings and `plain` for no entropy penalty and no hedging:  n >= 4: mle_state_big_kernel<n>;  plain, n <= 2,
// m <= D: mle_state_packed_kernel<n>;  plain, n == 3, m <= 64: mle_state_plain3_kernel;  otherwise mle_state_kernel<n> (designs
// beyond 64 KiB of per-setting staging take the streamed R operator: StateLds::staged)
int fbx_mle_state_dev(const fbx_design* design, int64_t B, const double* d_expect, const double* d_counts,
                      double epsilon, double entropy_penalty, double beta, double tol, int maxiter,
                      double* d_rho_out, int32_t* d_iters_out, int32_t* d_hit_max_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_mle_state", B, d_expect && d_counts && d_rho_out, &go, entropy_penalty != 0.0 && beta != 0.0));
    if (!go) return FBX_OK;
    const int m = design->dev.m;
    const bool plain = entropy_penalty == 0.0 && beta == 0.0;
    return with_qubits(design->dev.n, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value, D = 1 << (2 * NQ);
        if constexpr (NQ >= 4) {
            return launch_lds(mle_state_big_kernel<NQ>, dim3((unsigned)B), dim3(D), StateBigLds<NQ>::bytes(), design->dev, d_expect,
                              d_counts, epsilon, entropy_penalty, beta, tol, maxiter, d_rho_out, d_iters_out, d_hit_max_out);
        } else {
            const size_t lds = StateLds<NQ>::launch_bytes(m);
            if constexpr (NQ <= 2) {
                if (plain && m <= D)
                    return launch_lds(mle_state_packed_kernel<NQ>, dim3((unsigned)((B + 64 / D - 1) / (64 / D))), dim3(64), 0, design->dev,
                                      B, d_expect, epsilon, tol, maxiter, d_rho_out, d_iters_out, d_hit_max_out);
            } else {
                if (plain && m <= 64)
                    return launch_lds(mle_state_plain3_kernel, dim3((unsigned)B), dim3(64), lds, design->dev, d_expect, d_counts, epsilon,
                                      tol, maxiter, d_rho_out, d_iters_out, d_hit_max_out);
            }
            return launch_lds(mle_state_kernel<NQ>, dim3((unsigned)B), dim3(64), lds, design->dev, d_expect, d_counts, epsilon,
                              entropy_penalty, beta, tol, maxiter, d_rho_out, d_iters_out, d_hit_max_out);
        }
    });
}

int fbx_mle_state(const fbx_design* design, int64_t B, const double* expect, const double* counts,
                  double epsilon, double entropy_penalty, double beta, double tol, int maxiter,
                  double* rho_out, int32_t* iters_out, int32_t* hit_max_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_mle_state", B, expect && counts && rho_out, &go, entropy_penalty != 0.0 && beta != 0.0));
    if (!go) return FBX_OK;
    const size_t m = design->dev.m, D = design->dev.D;
    HostIO io; double *de, *dc, *dr; int32_t *di, *dh;
    FBX_TRY(io.in(expect, m * B, &de)); FBX_TRY(io.in(counts, m * B, &dc));
    FBX_TRY(io.out(rho_out, D * 2 * B, &dr)); FBX_TRY(io.out(iters_out, (size_t)B, &di)); FBX_TRY(io.out(hit_max_out, (size_t)B, &dh));
    FBX_TRY(fbx_mle_state_dev(design, B, de, dc, epsilon, entropy_penalty, beta, tol, maxiter, dr, di, dh));
    return io.finish();
}

int fbx_r_operator_dev(const fbx_design* design, int64_t B, const double* d_rho, const double* d_expect, double* d_r_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_r_operator", B, d_rho && d_expect && d_r_out, &go));
    if (!go) return FBX_OK;
    return with_qubits(design->dev.n, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if constexpr (NQ >= 4) return launch_state_big<NQ>(0, design, B, d_rho, d_expect, nullptr, d_r_out);
        else return launch_lds(r_operator_kernel<NQ>, dim3((unsigned)B), dim3(64), StateLds<NQ>::launch_bytes(design->dev.m), design->dev,
                               d_rho, d_expect, d_r_out);
    });
}

int fbx_r_operator(const fbx_design* design, int64_t B, const double* rho, const double* expect, double* r_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_r_operator", B, rho && expect && r_out, &go));
    if (!go) return FBX_OK;
    const size_t m = design->dev.m, D = design->dev.D;
    HostIO io; double *dr, *de, *dout;
    FBX_TRY(io.in(rho, D * 2 * B, &dr)); FBX_TRY(io.in(expect, m * B, &de)); FBX_TRY(io.out(r_out, D * 2 * B, &dout));
    FBX_TRY(fbx_r_operator_dev(design, B, dr, de, dout));
    return io.finish();
}

int fbx_state_log_likelihood_dev(const fbx_design* design, int64_t B, const double* d_rho, const double* d_expect,
                                 const double* d_counts, double* d_ll_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_state_log_likelihood", B, d_rho && d_expect && d_counts && d_ll_out, &go));
    if (!go) return FBX_OK;
    return with_qubits(design->dev.n, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if constexpr (NQ >= 4) return launch_state_big<NQ>(1, design, B, d_rho, d_expect, d_counts, d_ll_out);
        else return launch_lds(loglik_kernel<NQ>, dim3((unsigned)B), dim3(64), StateLds<NQ>::launch_bytes(1), design->dev, d_rho, d_expect,
                               d_counts, d_ll_out);
    });
}

int fbx_state_log_likelihood(const fbx_design* design, int64_t B, const double* rho, const double* expect,
                             const double* counts, double* ll_out) {
    bool go;
    FBX_TRY(check_call(design, "fbx_state_log_likelihood", B, rho && expect && counts && ll_out, &go));
    if (!go) return FBX_OK;
    const size_t m = design->dev.m, D = design->dev.D;
    HostIO io; double *dr, *de, *dc, *dout;
    FBX_TRY(io.in(rho, D * 2 * B, &dr)); FBX_TRY(io.in(expect, m * B, &de)); FBX_TRY(io.in(counts, m * B, &dc));
    FBX_TRY(io.out(ll_out, (size_t)B, &dout));
    FBX_TRY(fbx_state_log_likelihood_dev(design, B, dr, de, dc, dout));
    return io.finish();
}

}  // extern "C"
