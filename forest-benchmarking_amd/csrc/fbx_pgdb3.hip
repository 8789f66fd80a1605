// fbx_pgdb3.hip -- 3-qubit (64 x 64 Choi) projected-gradient process tomography
// (BASELINE config 4).  Same algorithm and the same device routines as the 2-qubit kernel
// (fbx_pgdb.hip), re-mapped to ONE 1024-THREAD WORKGROUP PER RECONSTRUCTION: the 64 x 64 matrices
// are held as one 2x2 block per thread on a 32 x 32 thread grid, the systolic Jacobi runs with all
// 16 wavefronts (63 rounds per sweep, two workgroup barriers per round), and the 160 KiB of LDS are
// used to the byte:
//     [ Ms 64 KiB | Vs 64 KiB (aliased by the row-major staging matrix Mw) | R 32 KiB ]
// with the prediction tables T[s][i] / the gradient accumulator W[i][s] (up to 108 KiB for the
// Pauli in-basis) overlaying Ms + Vs between projections, and the small Dykstra scratch overlaying R.
// The Bloch matrix C (D x S doubles, 108 KiB for the Pauli in-basis) is read from L2.
//
// The building blocks (namespace p3) are in fbx_pgdb3_core.hpp; this file holds the park slab, the four kernels and their launchers.
//
// Reference: tomography.py:542-633, operator_tools/project_superoperators.py:19-144.
// no thread of these kernels reads global memory another thread of the same launch wrote (basis store and parked state
// are per thread, tables go through LDS): barriers order LDS only and leave global traffic in flight (fbx_common.hpp)
#ifndef FBX_FULL_BARRIERS          // (-DFBX_FULL_BARRIERS: every barrier a full __syncthreads() -- libfbx_fullbar.so, the reference build of
#define FBX_LDS_ONLY_BARRIERS      //  tests/test_barriers_gpu.py, which must reproduce this one bit for bit)
#endif
#include "fbx_pgdb3_core.hpp"
#include <cstdlib>

namespace fbx {

#ifdef FBX_DIAGNOSTICS
extern long long* g_phase_out;      // fbx_pgdb.hip (diagnostics builds only)
#define FBX_PHASE_OUT3(b0) (g_phase_out ? g_phase_out + (b0) * 8 : nullptr)
#else
#define FBX_PHASE_OUT3(b0) ((long long*)nullptr)
#endif

// Per-workgroup slab in HBM / L2 for what must survive the projection but is not touched by it -- the estimate, the
// gradient's Pauli coefficients, the model probabilities of the estimate and the normalised counts: written once and
// read once (counts: twice) per OUTER iteration with coalesced 8 / 16-byte accesses, instead of living in registers the
// compiler then spills around every one of the ~10 eigendecompositions of the projection.
template <int MAXJ>
struct Park3 {
    static constexpr size_t doubles() { return 2 * (size_t)p3::D * p3::D + (size_t)p3::D * p3::D + 4 * (size_t)MAXJ * p3::NT; }
    double* base;
    __device__ cplx* est() const { return (cplx*)base; }                              // [4][1024] blocks, element-major
    __device__ double* rg() const { return base + 2 * p3::D * p3::D; }                // [4096] gradient coefficients (Rt layout)
    __device__ double* pp() const { return rg() + p3::D * p3::D; }                    // [2 MAXJ][1024] probabilities of the estimate
    __device__ double* nn() const { return pp() + 2 * MAXJ * p3::NT; }                // [2 MAXJ][1024] normalised counts
};

template <int MAXJ>
__global__ void __launch_bounds__(1024)
pgdb3_kernel(DesignDev des, long long B, const double* __restrict__ expect, const double* __restrict__ counts,
             int trace_preserving, int mode, int max_iters, double* __restrict__ choi_out,
             int* __restrict__ iters_out, int* __restrict__ dykstra_out, int* __restrict__ backtracks_out,
             double* __restrict__ cost_out, long long* __restrict__ phase_out, int* __restrict__ sweeps_out,
             cplx* __restrict__ basis_scratch, int basis_cap, int* __restrict__ trace_out, int trace_iters,
             double* __restrict__ park_base) {
    using namespace p3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Lds L; L.carve(smem);
    PhaseClock pc; pc.reset(); L.pc = &pc;
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    const int m = des.m;
    Park3<MAXJ> park; park.base = park_base + (size_t)blockIdx.x * Park3<MAXJ>::doubles();

    // ---- data: n+-[k] = counts * (1 +- e)/2 / grand_total   (tomography.py:528-538), parked
    {
        double npl[MAXJ], nmi[MAXJ];
        double tot = 0.0;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int g = t * MAXJ + j;
            npl[j] = 0.0; nmi[j] = 0.0;
            if (g < m) {
                const int k = des.order[g];
                const double e = expect[item * m + k], c = counts[item * m + k];
                const double plus = (1.0 + e) / 2.0;
                npl[j] = c * plus; nmi[j] = c * (1.0 - plus);
                tot += c;
            }
        }
        tot = bsum(tot, L);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) { park.nn()[(2 * j) * NT + t] = npl[j] / tot; park.nn()[(2 * j + 1) * NT + t] = nmi[j] / tot; }
    }
    const double inv_mu = (2.0 * d * d) / 3.0;

    // model probabilities of this thread's outcomes from the prediction table in LDS
    auto probs_of = [&](int j, double& pp, double& pm, double missing) __attribute__((always_inline)) {
        const int g = t * MAXJ + j;
        pp = missing; pm = missing;
        if (g < m) setting_probs(des, L, g, pp, pm);
    };

    Blk est = blk_zero();
    { const int I = t / NB, J = t % NB; if (I == J) { est.re[0] = 1.0 / d; est.re[3] = 1.0 / d; } }
    int iters = 0, dyk = 0, backtracks = 0, sweeps = 0, cost_evals = 0, chain_start = 0;
    double old_cost = 0.0, new_cost = 0.0;
    bool have_cost = false;
    BasisStore basis;
    basis.g = basis_scratch ? basis_scratch + (size_t)blockIdx.x * basis_cap * D * D : nullptr;
    basis.cap = basis_cap; basis.nprev = 0; basis.use_prev = false; basis.write_all = false;
    double outer_step = 1.0;

    PH_START(pc);
    while (true) {
        if (mode == FBX_MODE_FIXED && iters >= max_iters) break;
        const int dyk_before = dyk, bt_before = backtracks;       // per-iteration trace (fbx_pgdb_process_ex)
        choi_to_pauli(est, L, t);
        PH_STOP(pc, 3);
        predict_table(des, L, t);
        PH_STOP(pc, 7);

        // ---- probabilities of the estimate (parked for the line search), initial cost, and the gradient
        // (tomography.py:617-633)
        double ep[MAXJ], em[MAXJ];                     // eta = n / clip(p) of this thread's outcomes
        {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                double pp, pm;
                probs_of(j, pp, pm, 1.0);
                park.pp()[(2 * j) * NT + t] = pp; park.pp()[(2 * j + 1) * NT + t] = pm;
                pp = pp < EPS ? EPS : pp; pm = pm < EPS ? EPS : pm;
                const double np_ = park.nn()[(2 * j) * NT + t], nm_ = park.nn()[(2 * j + 1) * NT + t];
                if (!have_cost && t * MAXJ + j < m) acc -= np_ * fast_log_pos(pp) + nm_ * fast_log_pos(pm);
                ep[j] = np_ / pp; em[j] = nm_ / pm;
            }
            if (!have_cost) { old_cost = bsum(acc, L); have_cost = true; ++cost_evals; }   // tomography.py:565
        }
        PH_STOP(pc, 5);
        double* W = gradient_weights(des, L, t, Slots<MAXJ>(), [&](int j, double& p_, double& m_) __attribute__((always_inline)) { p_ = ep[j]; m_ = em[j]; });
        gradient_coefficients(des, L, W, t);
        // the gradient is needed once more after the projection, for <update, gradient>: as its Pauli coefficients
        // (the transform is unitary up to the factor d: <E1, E2> = sum_ij R1_ij R2_ij), parked
        for (int idx = t; idx < D * D; idx += NT) park.rg()[idx] = L.Rt[idx];
        PH_STOP(pc, 4);
        Blk x;
        {
            const Blk grad = pauli_to_choi(L, t);
            x = blk_axpy(est, -inv_mu, grad);
        }
        PH_STOP(pc, 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) { cplx v; v.re = est.re[e]; v.im = est.im[e]; park.est()[e * NT + t] = v; }

        // bounds the accumulated loss of unitarity of the chained bases: a cold restart once the chains have
        // absorbed 54 sweeps per slot (what 16 converging iterations apply; see fbx_pgdb.hip)
        if (iters == 0 || sweeps - chain_start >= FBX3_BASIS_CHAIN_SWEEPS * (basis.nprev > 0 ? basis.nprev : 1)) { basis.nprev = 0; chain_start = sweeps; }
        basis.use_prev = outer_step < FBX3_BASIS_STEP;
        basis.write_all = outer_step < FBX3_BASIS_WRITE_STEP;
        { const double tr_ = des.eig_rel_tol * outer_step; L.jtol2 = fmax(FBX_JACOBI_TOL2, tr_ * tr_); }   // as in fbx_pgdb.hip
        const Blk proj = proj_physical(x, trace_preserving != 0, L, t, dyk, sweeps,
                                       true, basis.g ? &basis : nullptr);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const cplx v = park.est()[e * NT + t]; est.re[e] = v.re; est.im[e] = v.im; }
        const Blk upd = blk_sub(proj, est);
        PH_STOP(pc, 2);

        choi_to_pauli(upd, L, t);
        PH_STOP(pc, 3);
        double ipr = 0.0;                             // <update, gradient> = sum_ij R^upd_ij R^grad_ij
        for (int idx = t; idx < D * D; idx += NT) ipr = fma(L.Rt[idx], park.rg()[idx], ipr);
        predict_table(des, L, t);
        ipr = bsum(ipr, L);                           // (after the table product: the reduction scratch overlays Rt)
        PH_STOP(pc, 7);

        // ---- backtracking line search (tomography.py:575-585)
        double alpha = 1.0;
        {
            double npl[MAXJ], nmi[MAXJ], pep[MAXJ], pem[MAXJ], pup[MAXJ], pum[MAXJ];
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                probs_of(j, pup[j], pum[j], 0.0);
                pep[j] = park.pp()[(2 * j) * NT + t]; pem[j] = park.pp()[(2 * j + 1) * NT + t];
                npl[j] = park.nn()[(2 * j) * NT + t]; nmi[j] = park.nn()[(2 * j + 1) * NT + t];
            }
            auto cost_at = [&](double a) -> double {
                double acc = 0.0;
                auto slot = [&](int j) __attribute__((always_inline)) {
                    if (t * MAXJ + j < m) {
                        double pp = fma(a, pup[j], pep[j]), pm = fma(a, pum[j], pem[j]);
                        pp = pp < EPS ? EPS : pp; pm = pm < EPS ? EPS : pm;
                        acc -= npl[j] * fast_log_pos(pp) + nmi[j] * fast_log_pos(pm);
                    }
                };
                for_each_slot<MAXJ>(slot);
                return bsum(acc, L);
            };
            // Round 6: once two halvings have failed -- the long runs of a stalled iteration, ~50 halvings each -- the NEXT KL halvings
            // are evaluated in ONE pass over the thread's outcomes (one read of the six per-slot arrays, which live in scratch for the
            // Pauli in-basis: 1.4 KB per thread = 0.7 MB per workgroup through L2 / HBM per evaluation, what bounded this phase) and the
            // loop below walks them in order.  Every cost is the same sum in the same order as cost_at's (per-thread terms by slot, the
            // wavefront reduction, the sixteen partials added in wavefront order): the accepted step and every count are
            // BIT-IDENTICAL to the one-at-a-time loop; what changes is that up to KL - 1 evaluations behind the accepted one are wasted.
            constexpr int KL = 4;       // (eight: 168.2 against 162.4 ms for the Pauli in-basis -- sixteen logarithm chains in flight spill; two: 163.8)
            auto cost_ladder = [&](double a0, double (&out)[KL]) __attribute__((always_inline)) {
                double acc[KL];
#pragma unroll
                for (int k = 0; k < KL; ++k) acc[k] = 0.0;
                auto slot = [&](int j) __attribute__((always_inline)) {
                    if (t * MAXJ + j < m) {
                        const double ep_ = pep[j], em_ = pem[j], up_ = pup[j], um_ = pum[j], np_ = npl[j], nm_ = nmi[j];
                        double a = a0;
#pragma unroll
                        for (int k = 0; k < KL; ++k) {
                            double pp = fma(a, up_, ep_), pm = fma(a, um_, em_);
                            pp = pp < EPS ? EPS : pp; pm = pm < EPS ? EPS : pm;
                            acc[k] -= np_ * fast_log_pos(pp) + nm_ * fast_log_pos(pm);
                            a *= 0.5;
                            __builtin_amdgcn_sched_barrier(0);      // one step's two logarithms at a time: interleaved chains spill
                        }
                    }
                };
                for_each_slot<MAXJ>(slot);
#pragma unroll
                for (int k = 0; k < KL; ++k) acc[k] = wave_sum(acc[k]);
                FBX_BLOCK_SYNC();                               // earlier readers of `red` are done
                if ((t & 63) == 0) {
#pragma unroll
                    for (int k = 0; k < KL; ++k) L.red[k * (NT / 64) + (t >> 6)] = acc[k];
                }
                FBX_BLOCK_SYNC();
#pragma unroll
                for (int k = 0; k < KL; ++k) {
                    double sum = 0.0;
#pragma unroll
                    for (int w = 0; w < NT / 64; ++w) sum += L.red[k * (NT / 64) + w];
                    out[k] = sum;
                }
            };
            new_cost = cost_at(alpha); ++cost_evals;
            double change = GAMMA * alpha * ipr;
            int fails = 0;
            while (new_cost > old_cost + change) {
                if (fails >= 2) {
                    double lad[KL];
                    cost_ladder(0.5 * alpha, lad); cost_evals += KL;
                    bool stop = false;
#pragma unroll
                    for (int k = 0; k < KL; ++k) {
                        if (!stop) {
                            alpha *= 0.5; change *= 0.5; new_cost = lad[k]; ++backtracks;
                            stop = alpha < ALPHA_MIN || !(new_cost > old_cost + change);
                        }
                    }
                    if (stop) break;
                    continue;
                }
                alpha *= 0.5; change *= 0.5;
                new_cost = cost_at(alpha); ++cost_evals;
                ++backtracks; ++fails;
                if (alpha < ALPHA_MIN) break;
            }
        }
        est = blk_axpy(est, alpha, upd);
        outer_step = alpha * sqrt(bsum(blk_norm2(upd), L));
        if (trace_out && iters < trace_iters && t == 0) {
            int* tr = trace_out + ((size_t)item * trace_iters + iters) * 2;
            tr[0] = dyk - dyk_before; tr[1] = backtracks - bt_before;
        }
        ++iters;
        PH_STOP(pc, 5);
        if (mode == FBX_MODE_CONVERGE) {
            if (!(old_cost - new_cost >= STOP)) break;          // tomography.py:589; a NaN cost also ends the loop
            if (max_iters > 0 && iters >= max_iters) break;
        }
        old_cost = new_cost;
    }
    choi_store(choi_out, item, t, est);
#ifdef FBX_PHASE_TIMERS
    if (t == 0 && phase_out) for (int i = 0; i < FBX_NPHASE; ++i) phase_out[item * FBX_NPHASE + i] = pc.acc[i];
#endif
    if (t == 0) {
        if (iters_out) iters_out[item] = iters;
        if (dykstra_out) dykstra_out[item] = dyk;
        if (backtracks_out) backtracks_out[item] = backtracks;
        if (cost_out) cost_out[item] = have_cost ? new_cost : 0.0;
        if (sweeps_out) {     // work_out[4]: Jacobi sweeps, eigenvalue terms rebuilt, cost evaluations, 0
            sweeps_out[4 * item] = sweeps; sweeps_out[4 * item + 1] = L.terms;
            sweeps_out[4 * item + 2] = cost_evals; sweeps_out[4 * item + 3] = 0;
        }
    }
}

// one 1024-thread workgroup per item with all of Lds::bytes() as dynamic LDS, on `s`; the launch is checked
template <class... P, class... A>
static int launch_p3(void (*kern)(P...), int64_t items, hipStream_t s, A... args) {
    const size_t lds = p3::Lds::bytes();
    FBX_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)items), dim3(p3::NT), lds, s, args...);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}
// the prediction table T[S][64] / the gradient weights W[64][S] must fit Ms + Vs
static bool states_fit(const fbx_design* des, const char* who) {
    if ((size_t)des->dev.S * p3::D * sizeof(double) <= 2 * sizeof(cplx) * p3::D * p3::D) return true;
    set_error(std::string(who) + ": too many distinct input states for the 3-qubit kernel");
    return false;
}

template <int MAXJ>
static int launch3(const PgdbCall& call) {
    const fbx_design* des = call.des;
    const int64_t B = call.B;
    if (!states_fit(des, "fbx_pgdb_process")) return FBX_ERR_UNSUPPORTED;
    // per-workgroup store of Dykstra eigenvector bases (BASIS_CAP x 64 KiB); batches are processed in
    // chunks so the store stays bounded (512 workgroups = 768 MiB)
    constexpr int64_t CHUNK = 512;
#define FBX_BASIS_CAP3 24
    constexpr int BASIS_CAP = FBX_BASIS_CAP3;   // Dykstra iterations per projection with a stored basis (64 KiB each)
    // (a grow-only workspace of the calling thread, released by fbx_release_workspace)
    void* w = nullptr;
    const size_t in_flight = (size_t)(B < CHUNK ? B : CHUNK);
    const size_t basis_bytes = sizeof(cplx) * p3::D * p3::D * in_flight * BASIS_CAP;
    { const int rc = workspace(WS_PGDB3_BASIS, basis_bytes + sizeof(double) * Park3<MAXJ>::doubles() * in_flight, &w); if (rc) return rc; }
    cplx* basis = (cplx*)w;
    double* park = (double*)((char*)w + basis_bytes);
    DesignDev dev = des->dev;
    dev.eig_rel_tol = call.eig_rel_tol >= 0.0 ? call.eig_rel_tol : option_pgdb_eig_rel_tol(3);
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
        const PgdbCall s = call.slice(b0, B - b0 < CHUNK ? B - b0 : CHUNK);
        FBX_TRY(launch_p3(pgdb3_kernel<MAXJ>, s.B, s.launch_stream ? s.launch_stream : stream(), dev, (long long)s.B,
                          s.e, s.c, s.tp, s.mode, s.max_iters, s.choi, s.it, s.dy, s.bt, s.cost,
                          FBX_PHASE_OUT3(b0), s.sw, basis, BASIS_CAP, s.trace, s.trace_iters, park));
    }
    return FBX_OK;
}

// _cost / _grad_cost (tomography.py:597-633) for 3 qubits as a function of their own (fbx_pgdb_cost_grad; the 1- / 2-qubit form and
// the reasons are in fbx_pgdb.hip): one evaluation with the device functions of pgdb3_kernel -- choi_to_pauli, the matrix-core
// table product, the run-wise deterministic identity row of W, gradient_coefficients, pauli_to_choi.  Any number of settings:
// thread t owns the contiguous run [t MJ, (t + 1) MJ) of the state-grouped settings, MJ = ceil(m / 1024) at run time; eta = n / p
// waits in `eta` (HBM, [2 m] per item) between the pass that consumes the table and the pass that fills W in its place.
__global__ void __launch_bounds__(1024)
pgdb3_cost_grad_kernel(DesignDev des, long long B, const double* __restrict__ nvec, const double* __restrict__ choi_in, double eps,
                       double* __restrict__ cost_out, double* __restrict__ grad_out, double* __restrict__ eta) {
    using namespace p3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Lds L; L.carve(smem);
    PhaseClock pc; pc.reset(); L.pc = &pc;
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    const int m = des.m, MJ = (m + NT - 1) / NT;
    choi_to_pauli(choi_load(choi_in, item, t), L, t);
    predict_table(des, L, t);
    const double* nv = nvec + item * 2 * m;
    double* et = eta + item * 2 * m;
    double acc = 0.0;
    for (int j = 0; j < MJ; ++j) {
        const int g = t * MJ + j;
        if (g < m) {
            const int k = des.order[g];
            double pp, pm;
            setting_probs(des, L, g, pp, pm);
            pp = pp < eps ? eps : pp; pm = pm < eps ? eps : pm;
            const double np_ = nv[2 * k], nm_ = nv[2 * k + 1];
            acc -= np_ * fast_log_pos(pp) + nm_ * fast_log_pos(pm);
            et[2 * g] = np_ / pp; et[2 * g + 1] = nm_ / pm;
        }
    }
    acc = bsum(acc, L);
    if (t == 0 && cost_out) cost_out[item] = acc;
    if (!grad_out) return;
    double* W = gradient_weights(des, L, t, MJ, [&](int j, double& ep, double& em) __attribute__((always_inline)) {
        const int g = t * MJ + j;
        ep = et[2 * g]; em = et[2 * g + 1];               // (written by this very thread)
    });
    gradient_coefficients(des, L, W, t);
    choi_store(grad_out, item, t, pauli_to_choi(L, t));
}

int pgdb3_cost_grad_launch(const fbx_design* des, int64_t B, const double* nvec, const double* choi, double eps, double* cost,
                           double* grad) {
    if (!states_fit(des, "fbx_pgdb_cost_grad")) return FBX_ERR_UNSUPPORTED;
    // (a grow-only workspace of the calling thread: it outlives the kernel, and growing it waits for the stream)
    void* eta = nullptr;
    { const int rc = workspace(WS_PGDB3_ETA, sizeof(double) * 2 * (size_t)B * des->dev.m, &eta); if (rc) return rc; }
    return launch_p3(pgdb3_cost_grad_kernel, B, stream(), des->dev, (long long)B, nvec, choi, eps, cost, grad, (double*)eta);
}

// ---- 3-qubit Choi projections (fbx_proj_choi) and linear inversion (fbx_linv_process) on the same
// 1024-thread building blocks
__global__ void __launch_bounds__(1024)
proj_choi3_kernel(int kind, long long B, const double* __restrict__ in, double* __restrict__ out,
                  int* __restrict__ iters_out) {
    using namespace p3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Lds L; L.carve(smem);
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    const Blk x = choi_load(in, item, t);
    // a non-finite item: NaN in every entry, the count 1 for the Dykstra kinds, nothing projected (proj_choi_body, fbx_superop.hip)
    int nonfinite = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) nonfinite |= !(isfinite(x.re[e]) && isfinite(x.im[e]));
    if (bsum(nonfinite ? 1.0 : 0.0, L) != 0.0) {               // (not __syncthreads_or: its static LDS word would not fit beside Lds::bytes())
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        Blk nans;
#pragma unroll
        for (int e = 0; e < 4; ++e) { nans.re[e] = nan; nans.im[e] = nan; }
        choi_store(out, item, t, nans);
        if (t == 0 && iters_out) iters_out[item] = kind >= FBX_PROJ_PHYSICAL_TP ? 1 : 0;
        return;
    }
    int iters = 0, sweeps = 0;
    Blk y;
    if (kind == FBX_PROJ_CP) y = proj_cp(x, L, t, sweeps);
    else if (kind == FBX_PROJ_TP) y = proj_tp(x, L, t);
    else if (kind == FBX_PROJ_TNI) y = proj_tni(x, L, t, sweeps);
    else y = proj_physical(x, kind == FBX_PROJ_PHYSICAL_TP, L, t, iters, sweeps, false);
    choi_store(out, item, t, y);
    if (t == 0 && iters_out) iters_out[item] = iters;
}

__global__ void __launch_bounds__(1024)
linv_process3_kernel(DesignDev des, long long B, const double* __restrict__ expect, double* __restrict__ out) {
    using namespace p3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Lds L; L.carve(smem);
    const int t = threadIdx.x;
    const long long item = blockIdx.x;
    for (int idx = t; idx < D * D; idx += NT) {       // Rt[j * 64 + i] = R[i][j] (+ the identity term)
        const int i = idx % D, j = idx / D;
        double acc = 0.0;
        for (int g = des.pptr[i]; g < des.pptr[i + 1]; ++g)
            acc += expect[item * des.m + des.porder[g]] * des.pinvT[(size_t)g * D + j];
        L.Rt[idx] = acc + ((idx == 0) ? 1.0 : 0.0);
    }
    FBX_BLOCK_SYNC();
    choi_store(out, item, t, pauli_to_choi(L, t));
}

int proj_choi3_launch(int kind, int64_t B, const double* d_in, double* d_out, int32_t* d_iters) {
    return launch_p3(proj_choi3_kernel, B, stream(), kind, (long long)B, d_in, d_out, d_iters);
}
int linv_process3_launch(const fbx_design* des, int64_t B, const double* d_expect, double* d_out) {
    return launch_p3(linv_process3_kernel, B, stream(), des->dev, (long long)B, d_expect, d_out);
}

// called from fbx_pgdb.hip's dispatcher
int pgdb3_dispatch(const PgdbCall& in) {
    const int m = in.des->dev.m;
    PgdbCall call = in;
    call.mode &= 0xff;     // FBX_MODE_LS_REFERENCE: this kernel's line search always evaluates the full cost with the rounded test
    if (m <= 4096) return launch3<4>(call);
    if (m <= 14336) return launch3<14>(call);
    // Merged / repeated datasets (the reference takes any result list, tomography.py:494-539): the same kernel with 32 / 64 outcome
    // slots per thread.  Their per-slot arrays no longer fit 128 registers and live in scratch: slow (a few times the resident
    // instantiations per outer iteration outside the projection) and complete up to 65 536 settings.
    if (m <= 32768) return launch3<32>(call);
    if (m <= 65536) return launch3<64>(call);
    set_error("fbx_pgdb_process: 3-qubit designs are limited to 65536 settings");
    return FBX_ERR_UNSUPPORTED;
}

}  // namespace fbx
