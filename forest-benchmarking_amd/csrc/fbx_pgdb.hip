// fbx_pgdb.hip -- batched projected-gradient-descent-with-backtracking process tomography.
//
// One 64-lane wavefront owns one reconstruction for its whole life: the Choi estimate and
// the Dykstra state live in registers (one 2x2 block per lane), work matrices and the
// predicted-expectation tables in LDS; HBM is read once (expectations + counts) and written
// once (Choi + counters) -- plus the per-item store of Dykstra eigenvector bases (BasisStore,
// fbx_choi.hpp), working state in HBM/L2 that lets an outer iteration start its decompositions
// from the bases the previous one found.
//
// Replaces, for a batch that shares one design (file:line under forest/benchmarking/):
//   pgdb_process_estimate   tomography.py:542-594
//   _extract_from_results   tomography.py:494-539  (A never materialised: the Kronecker
//                           structure A_row = vec(rho_in (x) Pi^T)/d^2 is applied as
//                           T[s][i] = sum_j R_ij c_j(s), R = Pauli-Liouville form of E)
//   _cost / _grad_cost      tomography.py:597-633
//   proj_choi_to_physical   operator_tools/project_superoperators.py:87-144
#include "fbx_pgdb_body.hpp"
#include <cstdlib>

namespace fbx {

// The product kernel: one wavefront per SIMD (up to 512 registers, 39 KB of LDS) -- the fastest form while
// there are no more reconstructions in flight than SIMDs (B <= 1024 on 256 CUs).
template <int NQ, int MAXJ>
__global__ void __launch_bounds__(64)
pgdb_kernel(DesignDev des, long long B, const double* __restrict__ expect,
            const double* __restrict__ counts, int trace_preserving, int mode, int max_iters,
            double* __restrict__ choi_out, int* __restrict__ iters_out,
            int* __restrict__ dykstra_out, int* __restrict__ backtracks_out,
            double* __restrict__ cost_out, int* __restrict__ work_out,
            long long* __restrict__ phase_out, cplx* __restrict__ basis_scratch, int basis_cap,
            int* __restrict__ trace_out, int trace_iters) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    pgdb_body<NQ, MAXJ, false>(smem, blockIdx.x, des, B, expect, counts, trace_preserving, mode, max_iters, choi_out, iters_out,
                               dykstra_out, backtracks_out, cost_out, work_out, phase_out, basis_scratch, basis_cap, nullptr,
                               trace_out, trace_iters);
}

// The same kernel in PIECES (fbx_pgdb_lean.hip has the description): for launches that put more than one reconstruction on a
// SIMD but cannot use the two-waves kernel -- single-qubit designs on the wavefront-per-item kernel (1025 .. 8191 / 16 383
// experiments), 2-qubit designs with more than 50 input states.  1024 persistent workgroups.
template <int NQ, int MAXJ>
__global__ void __launch_bounds__(64)
pgdb_pieces_kernel(DesignDev des, long long B, const double* __restrict__ expect,
                   const double* __restrict__ counts, int trace_preserving, int mode, int max_iters,
                   double* __restrict__ choi_out, int* __restrict__ iters_out,
                   int* __restrict__ dykstra_out, int* __restrict__ backtracks_out,
                   double* __restrict__ cost_out, int* __restrict__ work_out,
                   long long* __restrict__ phase_out, cplx* __restrict__ basis_scratch, int basis_cap,
                   int* __restrict__ trace_out, int trace_iters,
                   int pieces, int piece_iters, int* __restrict__ queue, int* __restrict__ flags, double* __restrict__ recs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    pgdb_pieces_run<NQ, MAXJ, false>(smem, des, B, expect, counts, trace_preserving, mode, max_iters, choi_out, iters_out, dykstra_out,
                                     backtracks_out, cost_out, work_out, phase_out, basis_scratch, basis_cap, nullptr, trace_out,
                                     trace_iters, pieces, piece_iters, queue, flags, recs);
}

#ifdef FBX_DIAGNOSTICS
__global__ void debug_log_kernel(const double* x, double* out, long long n) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) out[i] = fast_log_pos(x[i]);
}
#endif

// _cost / _grad_cost (tomography.py:597-633) as functions of their own: ONE evaluation of the negative log-likelihood and of its
// gradient at a given Choi matrix, with the very device functions the reconstruction kernels use -- Choi -> Pauli coefficients
// (choi_to_pauli_real), T = R C (predict_table), the clipped probabilities and fast_log_pos, the per-state weights through LDS
// atomics, R^G = -(W C^T) / d^2 and the inverse transform (pauli_real_to_choi_blk) -- so that the gradient, which the reconstruction
// never outputs, can be held against the oracle directly (tests/test_cost_grad_gpu.py).  `nvec` is the reference's `n`: row 2 k /
// 2 k + 1 = normalised +1 / -1 counts of result k.  Any number of settings (the outcome slots are walked from HBM).
template <int NQ>
__global__ void __launch_bounds__(64)
pgdb_cost_grad_kernel(DesignDev des, long long B, const double* __restrict__ nvec, const double* __restrict__ choi_in, double eps,
                      double* __restrict__ cost_out, double* __restrict__ grad_out) {
    constexpr int d = 1 << NQ, D = d * d, LD = D + 1, NB = D / 2, NACT = NB * NB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    const int m = des.m, S = des.S;
    PgdbLds<NQ, false> L;
    L.carve(smem, S, 0);
    for (int idx = lane; idx < D * S; idx += 64) L.Cl[(idx % S) * D + idx / S] = des.C[idx];     // des.C is [D][S]
    Blk est = blk_zero();
    if (lane < NACT) {
        const int I = lane / NB, J = lane % NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = 2 * I + (e >> 1), col = 2 * J + (e & 1);
            const double* o = choi_in + ((item * D + row) * D + col) * 2;
            est.re[e] = o[0]; est.im[e] = o[1];
        }
    }
    FBX_WAVE_SYNC();
    blk_store<D, LD>(L.choi.Mw, lane, est);
    FBX_WAVE_SYNC();
    choi_to_pauli_real<NQ>(L.choi.Mw, L.Rb, lane);
    FBX_WAVE_SYNC();
    predict_table<NQ, 3>(L.Rb, L.Cl, L.Test, S, lane);
    double* Wt = L.Tupd;                        // [S][D]
    for (int idx = lane; idx < D * S; idx += 64) Wt[idx] = 0.0;
    FBX_WAVE_SYNC();
    const double half_dd = 0.5 / (double)(d * d);
    const bool unit_coefs = des.unit_coefs != 0;
    const double* nv = nvec + item * 2 * m;
    double acc = 0.0;
    for (int g = lane; g < m; g += 64) {
        const uint32_t dw = des.sp[g];
        const int st = dw >> 16, p = dw & 0xffff, k = des.order[g];
        const double cf = unit_coefs ? 1.0 : des.coef[g];
        const double tr = L.Test[st * D], ex = cf * L.Test[st * D + p];
        double pp = (tr + ex) * half_dd, pm = (tr - ex) * half_dd;
        pp = pp < eps ? eps : pp; pm = pm < eps ? eps : pm;
        const double np_ = nv[2 * k], nm_ = nv[2 * k + 1];
        acc -= np_ * fast_log_pos(pp) + nm_ * fast_log_pos(pm);
        const double ep = np_ / pp, em = nm_ / pm;
        atomicAdd(&Wt[st * D], 0.5 * (ep + em));
        atomicAdd(&Wt[st * D + p], cf * 0.5 * (ep - em));
    }
    acc = uniform(wave_sum(acc));
    if (lane == 0 && cost_out) cost_out[item] = acc;
    FBX_WAVE_SYNC();
    if (!grad_out) return;
    grad_coefficients<NQ>(Wt, L.Cl, L.Rb, S, lane);
    FBX_WAVE_SYNC();
    const Blk grad = pauli_real_to_choi_blk<NQ>(L.Rb, L.choi.Mw, lane);
    if (lane < NACT) {
        const int I = lane / NB, J = lane % NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = 2 * I + (e >> 1), col = 2 * J + (e & 1);
            double* o = grad_out + ((item * D + row) * D + col) * 2;
            o[0] = grad.re[e]; o[1] = grad.im[e];
        }
    }
}

int pgdb3_cost_grad_launch(const fbx_design* des, int64_t B, const double* nvec, const double* choi, double eps, double* cost,
                           double* grad);     // fbx_pgdb3.hip

template <int NQ>
static int launch_cost_grad(const fbx_design* des, int64_t B, const double* nvec, const double* choi, double eps, double* cost,
                            double* grad) {
    const size_t lds = PgdbLds<NQ, false>::bytes(des->dev.S, 0);
    if (lds > 160 * 1024) {
        set_error("fbx_pgdb_cost_grad: too many distinct input states for the LDS-resident tables");
        return FBX_ERR_UNSUPPORTED;
    }
    FBX_HIP(hipFuncSetAttribute((const void*)pgdb_cost_grad_kernel<NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((pgdb_cost_grad_kernel<NQ>), dim3((unsigned)B), dim3(64), lds, stream(), des->dev, (long long)B, nvec, choi, eps,
                       cost, grad);
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

constexpr int BASIS_CAP = 32;              // Dykstra iterations per projection that get a stored basis

#ifdef FBX_DIAGNOSTICS
long long* g_phase_out = nullptr;          // diagnostics builds only: set by fbx_debug_set_phase_buffer (also read by fbx_pgdb3.hip)
#define FBX_PHASE_OUT(b0) (g_phase_out ? g_phase_out + (b0) * 8 : nullptr)
#else
#define FBX_PHASE_OUT(b0) ((long long*)nullptr)
#endif

// what the kernels of fbx_pgdb.hip / fbx_pgdb_lean.hip get of a call (already cut to the items of one launch)
static PgdbLaunch pgdb_launch_args(const PgdbCall& s, const DesignDev& dev, int mode) {
    PgdbLaunch a;
    a.dev = dev; a.nb = s.B; a.e = s.e; a.c = s.c; a.tp = s.tp; a.mode = mode; a.max_iters = s.max_iters;
    a.choi = s.choi; a.it = s.it; a.dy = s.dy; a.bt = s.bt; a.cost = s.cost; a.sw = s.sw;
    a.trace = s.trace; a.trace_iters = s.trace_iters;
    return a;
}

template <int NQ, int MAXJ>
static int launch_pgdb(const PgdbCall& call) {
    const fbx_design* des = call.des;
    const int64_t B = call.B;
    const int max_iters = call.max_iters;
    const bool ls_reference = (call.mode & FBX_MODE_LS_REFERENCE) != 0;      // per call: the line search taken literally (include/fbx.h)
    const int mode = call.mode & 0xff;
    // batches that put several reconstructions on a SIMD take the lean two-waves-per-SIMD kernel (2 qubits)
    // MAXJ = 0: the STREAMED instantiation (fbx_pgdb_body.hpp) -- any number of settings, outcome slots read from HBM / L2
    constexpr bool STREAM = MAXJ == 0;
    const int slots = STREAM ? (des->dev.m + 63) / 64 : MAXJ;            // outcome slots per lane
    bool lean = STREAM || (NQ == 2 && (call.total_batch > B ? call.total_batch : B) >= FBX_LEAN_MIN_BATCH);
    size_t lds = STREAM ? pgdb_stream_lds(NQ, des->dev.S) : PgdbLds<NQ, false>::bytes(des->dev.S, 64 * MAXJ);      // Ln has one row pair per outcome slot of the kernel
    if constexpr (NQ == 2 && !STREAM) {
        lean = lean && pgdb_lean_eligible(des->dev.S);
        if (lean) lds = pgdb_lean_lds(MAXJ, des->dev.S);
    }
    if (lds > 160 * 1024) {
        set_error("fbx_pgdb_process: too many distinct input states for the prediction tables of the LDS-resident kernel");
        return FBX_ERR_UNSUPPORTED;
    }
    if constexpr (!STREAM) {
        if (!lean) FBX_HIP(hipFuncSetAttribute((const void*)pgdb_kernel<NQ, MAXJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    // per-item store of Dykstra eigenvector bases (BASIS_CAP x D x D complex each = 128 KiB per 2-qubit
    // item): a grow-only workspace of the calling thread (released by fbx_release_workspace).  A single
    // outer iteration has no previous iteration to take a basis from: no store then.
    constexpr int D = 1 << (2 * NQ);
    // One launch for up to 65 536 reconstructions: the store is 128 KiB per 2-qubit item (8 GiB for 65 536 -- this part
    // has 288 GB), and a launch that holds the whole batch keeps every SIMD busy until the last items, where a
    // sequence of 8192-item launches idles at the end of each (the items of a launch differ by +-15 % in work).
    // When the device cannot give that much, the launch size is halved until the store fits.
    const bool want_basis = !(mode == FBX_MODE_FIXED && max_iters <= 1) && !(mode == FBX_MODE_CONVERGE && max_iters == 1);
    const size_t basis_item = want_basis ? sizeof(cplx) * D * D * BASIS_CAP : 0;
    const size_t counts_item = lean ? sizeof(double) * 2 * (size_t)slots * 64 : 0;      // normalised counts of the lean kernel (fbx_pgdb_body.hpp)
    int64_t CHUNK = 65536;
    char* wsp = nullptr;
    int64_t ws_items = call.ws_items > 0 ? call.ws_items : (B < CHUNK ? B : CHUNK);
    if (basis_item + counts_item) {
        for (;;) {
            // the pipelined host entry point says how many slots its stages need between them; everybody else min(B, CHUNK)
            const size_t total = (basis_item + counts_item) * (size_t)ws_items;
            void* w = nullptr;
            const int rc = workspace(WS_PGDB_BASIS, total, &w);
            if (rc == FBX_OK) { wsp = (char*)w; break; }
            // (the streamed instantiations keep 16 B x m of normalised counts per slot: a huge merged design may need fewer slots than 1024)
            if (rc != FBX_ERR_NOMEM || call.ws_items > 0 || ws_items <= (STREAM ? 1 : 1024)) return rc;
            (void)hipGetLastError();
            ws_items /= 2; CHUNK = ws_items;
        }
    }
    const int64_t n_slots = ws_items;
    cplx* basis = basis_item ? (cplx*)wsp + (size_t)call.ws_offset * D * D * BASIS_CAP : nullptr;
    double* ncounts = counts_item ? (double*)(wsp + basis_item * (size_t)n_slots) + (size_t)call.ws_offset * 2 * (size_t)slots * 64 : nullptr;
    DesignDev dev = des->dev;
    dev.eig_rel_tol = call.eig_rel_tol >= 0.0 ? call.eig_rel_tol : option_pgdb_eig_rel_tol(NQ);     // per call, else the process default
    dev.ls_reference = ls_reference ? 1 : 0;
    hipStream_t st = call.launch_stream ? call.launch_stream : stream();
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
        const int64_t nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        PgdbLaunch a = pgdb_launch_args(call.slice(b0, nb), dev, mode);
        a.phase = FBX_PHASE_OUT(b0); a.basis = basis; a.basis_cap = BASIS_CAP; a.ncounts = ncounts;
        // more than one reconstruction per SIMD on the one-wave kernel: in pieces too -- except single-qubit batches to convergence,
        // whose outer iterations last microseconds (a piece's set-up and hand-over then cost what the tail saves: 8000 Pauli
        // experiments 8.6 -> 10.3 ms, while 100 fixed iterations of the SIC design gain 25-35 %; scripts/pieces_time_1q.py)
        const bool fat_pieces = !lean && nb > 1024 && (NQ == 2 || mode == FBX_MODE_FIXED);
        if constexpr (STREAM) {                             // whole reconstructions, one workgroup each
            const int rc = pgdb_stream_launch(NQ, lds, st, a);
            if (rc) return rc;
            continue;
        } else {
        {
            // the two-waves kernel runs its reconstructions in pieces (fbx_pgdb_lean.hip): fbx_set_option("pgdb_pieces"), 1 = whole
            // reconstructions.  FBX_LEAN_PIECES / FBX_LEAN_PIECE_ITERS (environment, experiments and tests) override it per call.
            if (lean || fat_pieces) {
                const char* pv = getenv("FBX_LEAN_PIECES");
                const char* wv = getenv("FBX_LEAN_PIECE_ITERS");
                int pieces = pv && *pv ? atoi(pv) : option_pgdb_pieces();     // default 8 (measured 2048 .. 65 536 experiments: 8 >= 4, 16; scripts/pieces_time.py)
                if (pieces > 64) pieces = 64;
                if (pieces > 1) {
                    const int span = mode == FBX_MODE_FIXED || max_iters > 0 ? max_iters : 64;      // to convergence: ~45 iterations on average
                    a.piece_iters = wv && *wv ? atoi(wv) : (span + pieces - 1) / pieces;
                    if (a.piece_iters < 1) a.piece_iters = 1;
                    // A consumer waits for its predecessor piece with a BOUNDED spin (pgdb_pieces_run) that scales with piece_iters
                    // and allows ~10 ms per outer iteration -- 50 x what one costs on a device that several launches share.  Long
                    // pieces buy nothing (the tail of a launch is one piece either way): a caller with a huge fixed iteration
                    // count gets more pieces (up to 64) and, beyond 512 iterations per piece, whole reconstructions.
                    // (an explicit FBX_LEAN_PIECE_ITERS is taken as given: no doubling)
                    while (!(wv && *wv) && a.piece_iters > 64 && pieces < 64 && (int64_t)pieces * 2 * nb < (int64_t)1 << 30) { pieces *= 2; a.piece_iters = (span + pieces - 1) / pieces; }
                    if (a.piece_iters > 512) pieces = 1;
                }
                if (pieces > 1) {
                    // per workspace slot a progress flag and a record; two ticket counters: the pipelined host entry point has one
                    // launch in flight on each of its two compute streams, on disjoint slot ranges (ws_offset 0 / > 0)
                    void* w = nullptr;
                    const size_t fbytes = (sizeof(int) * (size_t)n_slots + 255) & ~(size_t)255;
                    if (workspace(WS_PGDB_PIECES, 512 + fbytes + sizeof(double) * PGDB_REC * (size_t)n_slots, &w) == FBX_OK) {
                        a.pieces = pieces; a.queue = (int*)w + (call.ws_offset ? 64 : 0);
                        a.flags = (int*)((char*)w + 512) + call.ws_offset;
                        a.recs = (double*)((char*)w + 512 + fbytes) + (size_t)call.ws_offset * PGDB_REC;
                    } else (void)hipGetLastError();                  // no room: whole reconstructions
                }
            }
        }
        if constexpr (NQ == 2) {
            if (lean) {
                const int rc = pgdb_lean_launch(MAXJ, lds, st, a);
                if (rc) return rc;
                continue;
            }
        }
        if (fat_pieces && a.pieces > 1) {
            FBX_HIP(hipFuncSetAttribute((const void*)pgdb_pieces_kernel<NQ, MAXJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            FBX_HIP(hipMemsetAsync(a.queue, 0, sizeof(int), st));
            FBX_HIP(hipMemsetAsync(a.flags, 0, sizeof(int) * (size_t)a.nb, st));
            hipLaunchKernelGGL((pgdb_pieces_kernel<NQ, MAXJ>), dim3(1024), dim3(64), lds, st, a.dev, a.nb, a.e, a.c, a.tp, a.mode, a.max_iters,
                               a.choi, a.it, a.dy, a.bt, a.cost, a.sw, a.phase, a.basis, a.basis_cap, a.trace, a.trace_iters,
                               a.pieces, a.piece_iters, a.queue, a.flags, a.recs);
            continue;
        }
        hipLaunchKernelGGL((pgdb_kernel<NQ, MAXJ>), dim3((unsigned)nb), dim3(64), lds, st, a.dev, a.nb, a.e, a.c, a.tp, a.mode, a.max_iters,
                           a.choi, a.it, a.dy, a.bt, a.cost, a.sw, a.phase, a.basis, a.basis_cap, a.trace, a.trace_iters);
        }
    }
    FBX_HIP(hipGetLastError());
    return FBX_OK;
}

int pgdb3_dispatch(const PgdbCall& call);                 // fbx_pgdb3.hip
bool pgdb1_eligible(const fbx_design* des);               // fbx_pgdb1.hip: the lane-per-item single-qubit kernel
int pgdb1_dispatch(const PgdbCall& call);

static int pgdb_dispatch(const PgdbCall& call) {
    const fbx_design* des = call.des;
    const int64_t B = call.B;
    const int n = des->dev.n, m = des->dev.m;
    if (n == 1) {
        // Large batches: 64 reconstructions per wavefront, one per lane (fbx_pgdb1.hip; the eigensolver at its full tolerance --
        // eig_rel_tol does not apply).  A lane is ~3x slower on one reconstruction than a wavefront and a launch lasts as long as
        // its slowest reconstruction (12-14 ms for the Pauli design, 5 ms for SIC, whatever the batch up to 65 536), while the
        // wave-per-item kernel below scales with the batch (1.0 / 0.76 us per reconstruction): the measured crossover
        // (scripts/pgdb1_crossover.py) is ~7000 experiments for the 12-setting SIC design and ~16 000 for the 18-setting Pauli
        // design.  fbx_set_option("pgdb_packed_1q", 0 | 2) forces one or the other.
        {
            const int packed = option_pgdb_packed_1q();
            const int64_t total = call.total_batch > B ? call.total_batch : B;
            const int64_t from = m <= 12 ? FBX_PACKED_1Q_MIN_BATCH : 2 * FBX_PACKED_1Q_MIN_BATCH;
            // the lane-per-item kernel always solves to full tolerance: a caller who passes an explicit eigensolver tolerance
            // (fbx_pgdb_process_ex, eig_rel_tol >= 0) gets the wavefront-per-item kernel, which honours it, whatever the batch size
            // -- so that an experiment's iterates do not depend on how many neighbours it is batched with (packed == 2 forces
            // the lane-per-item kernel all the same: a test / diagnostics setting, documented in include/fbx.h)
            const bool explicit_tol = call.eig_rel_tol >= 0.0 || (call.mode & FBX_MODE_LS_REFERENCE);      // (the flag too: the wave kernel honours it)
            if (pgdb1_eligible(des) && (packed == 2 || (packed == 1 && total >= from && !explicit_tol)))
                return pgdb1_dispatch(call);
        }
        if (m <= 64) return launch_pgdb<1, 1>(call);
        if (m <= 256) return launch_pgdb<1, 4>(call);
        // merged / repeated datasets (the reference takes any result list, tomography.py:494-539): outcome slots streamed from HBM
        return launch_pgdb<1, 0>(call);
    } else if (n == 2) {
        if (m <= 256) return launch_pgdb<2, 4>(call);
        if (m <= 576) return launch_pgdb<2, 9>(call);
        if (m <= 1024) return launch_pgdb<2, 16>(call);
        return launch_pgdb<2, 0>(call);
    }
    else if (n == 3) {
        return pgdb3_dispatch(call);
    }
    set_error("fbx_pgdb_process: process designs of 1 to 3 qubits");
    return FBX_ERR_UNSUPPORTED;
}

// The checks of fbx_pgdb_process_ex[_dev] on the record its entry point has filled in (pointers all host or all device), and the
// strides, which it takes from the design
static int pgdb_prepare(PgdbCall& call) {
    FBX_TRY(ensure_device());
    FBX_TRY(check_design(call.des, "fbx_pgdb_process"));
    FBX_REQUIRE(call.des->dev.kind == FBX_KIND_PROCESS, "fbx_pgdb_process: needs a process design");
    FBX_REQUIRE(call.B >= 0, "fbx_pgdb_process: negative batch");
    FBX_REQUIRE(call.B == 0 || (call.e && call.c && call.choi), "fbx_pgdb_process: NULL buffer");
    const int mode = call.mode & ~FBX_MODE_LS_REFERENCE;
    FBX_REQUIRE(mode == FBX_MODE_CONVERGE || mode == FBX_MODE_FIXED, "fbx_pgdb_process: bad mode");
    FBX_REQUIRE(call.max_iters >= 0, "fbx_pgdb_process: negative max_iters");
    FBX_REQUIRE(call.eig_rel_tol < 0.0 || call.eig_rel_tol <= 1e-3, "fbx_pgdb_process_ex: eig_rel_tol must be negative (default) or in [0, 1e-3]");
    FBX_REQUIRE(call.eig_rel_tol == call.eig_rel_tol, "fbx_pgdb_process_ex: eig_rel_tol is NaN");
    FBX_REQUIRE(call.trace_iters >= 0 && (call.trace == nullptr || call.trace_iters > 0), "fbx_pgdb_process_ex: trace_out needs trace_iters > 0");
    if (!call.trace) call.trace_iters = 0;
    call.m = (size_t)call.des->dev.m; call.DD = (size_t)call.des->dev.D * call.des->dev.D;
    return FBX_OK;
}

// The three extra streams of the pipelined path.  Left any other way than through finish(), it waits for them: copies and
// kernels may be queued there on staging blocks that go back to the thread's pool next (declare it AFTER the HostIO that owns
// them, which waits for the calling thread's own stream).
struct PipelineStreams {
    hipStream_t in = nullptr, out = nullptr, c2 = nullptr;
    bool queued = false;
    PipelineStreams() = default;
    PipelineStreams(const PipelineStreams&) = delete;
    PipelineStreams& operator=(const PipelineStreams&) = delete;
    ~PipelineStreams() { drain(); }
    int acquire() { FBX_TRY(copy_streams(&in, &out, &c2)); queued = true; return FBX_OK; }
    void drain() {
        if (queued) { (void)hipStreamSynchronize(in); (void)hipStreamSynchronize(c2); (void)hipStreamSynchronize(out); }
        queued = false;
    }
    // success: the downloads have arrived (the calling thread's stream, already waited for, followed the second compute stream)
    int finish() {
        if (!queued) return FBX_OK;
        FBX_HIP(hipStreamSynchronize(out));
        FBX_HIP(hipStreamSynchronize(in));
        queued = false;
        return FBX_OK;
    }
};

// Page-locked caller buffers and more than one stage of work (pgdb_stage_plan, fbx_pgdb_call.hpp, has the reasons): uploads on
// one stream, the stages' kernels on the calling thread's and the high-priority second compute stream, the Choi matrices down
// on a fourth.  The small outputs follow on the calling thread's stream (HostIO::finish).
static int pgdb_host_pipelined(const PgdbCall& host, const PgdbCall& dev, int64_t host_chunk, const PipelineStreams& s) {
    // (the 3-qubit launcher has one workspace: one compute stream)
    const PgdbStagePlan plan = pgdb_stage_plan(host.B, host_chunk, host.des->dev.n <= 2);
    const int nst = (int)plan.stages.size();
    hipEvent_t* ev = nullptr;
    FBX_TRY(ordering_events(2 * nst + 1, &ev));
    // (the staging buffers may still be in use by earlier work of this thread's stream)
    FBX_HIP(hipEventRecord(ev[2 * nst], stream()));
    FBX_HIP(hipStreamWaitEvent(s.in, ev[2 * nst], 0));
    FBX_HIP(hipStreamWaitEvent(s.out, ev[2 * nst], 0));
    FBX_HIP(hipStreamWaitEvent(s.c2, ev[2 * nst], 0));
    for (int k = 0; k < nst; ++k) {                        // uploads in stage order, back to back
        const PgdbStage& stage = plan.stages[k];
        const PgdbCall h = host.slice(stage.b0, stage.nb), d = dev.slice(stage.b0, stage.nb);
        const size_t bytes = sizeof(double) * (size_t)h.B * h.m;
        FBX_HIP(hipMemcpyAsync(const_cast<double*>(d.e), h.e, bytes, hipMemcpyHostToDevice, s.in));
        FBX_HIP(hipMemcpyAsync(const_cast<double*>(d.c), h.c, bytes, hipMemcpyHostToDevice, s.in));
        FBX_HIP(hipEventRecord(ev[2 * k], s.in));
    }
    for (int k = 0; k < nst; ++k) {
        const PgdbStage& stage = plan.stages[k];
        PgdbCall d = dev.slice(stage.b0, stage.nb);
        d.launch_stream = stage.second ? s.c2 : stream(); d.ws_items = plan.ws_total; d.ws_offset = stage.ws_offset;
        FBX_HIP(hipStreamWaitEvent(d.launch_stream, ev[2 * k], 0));
        // (FBX_ERR_NOMEM: the pipeline wants workspace slots for the whole bulk at once; the caller then runs the batch staged)
        FBX_TRY(pgdb_dispatch(d));
        FBX_HIP(hipEventRecord(ev[2 * k + 1], d.launch_stream));
        FBX_HIP(hipStreamWaitEvent(s.out, ev[2 * k + 1], 0));
        FBX_HIP(hipMemcpyAsync(host.slice(stage.b0, stage.nb).choi, d.choi, sizeof(double) * 2 * (size_t)d.B * d.DD, hipMemcpyDeviceToHost, s.out));
    }
    FBX_HIP(hipEventRecord(ev[2 * nst], s.c2));            // the small outputs follow BOTH compute streams
    FBX_HIP(hipStreamWaitEvent(stream(), ev[2 * nst], 0));
    return FBX_OK;
}

// everything on the calling thread's stream, in launches that fit the device (launch_pgdb halves them until the store does)
static int pgdb_host_staged(const PgdbCall& host, const PgdbCall& dev) {
    const size_t bytes = sizeof(double) * (size_t)host.B * host.m;
    FBX_HIP(hipMemcpyAsync(const_cast<double*>(dev.e), host.e, bytes, hipMemcpyHostToDevice, stream()));
    FBX_HIP(hipMemcpyAsync(const_cast<double*>(dev.c), host.c, bytes, hipMemcpyHostToDevice, stream()));
    FBX_TRY(pgdb_dispatch(dev));
    FBX_HIP(hipMemcpyAsync(host.choi, dev.choi, sizeof(double) * 2 * (size_t)host.B * host.DD, hipMemcpyDeviceToHost, stream()));
    return FBX_OK;
}

// The host-pointer call (`host`: every pointer a host pointer) on the calling thread's device; host.total_batch = size of the
// caller's whole batch when this is one device's block of it (kernels are chosen by the whole, so that the split does not
// change a single bit of any item)
static int pgdb_process_host(const PgdbCall& host) {
    const size_t B = (size_t)host.B, n_in = B * host.m, n_choi = 2 * B * host.DD;
    // `dev`: the same call on device blocks.  Expectations, counts and Choi matrices are moved by whichever path runs (blocks
    // only: no host pointer given); the small outputs come down in finish() on both.
    HostIO io;
    PipelineStreams streams;
    PgdbCall dev = host;
    double *de = nullptr, *dc = nullptr;
    FBX_TRY(io.in<double>(nullptr, n_in, &de)); FBX_TRY(io.in<double>(nullptr, n_in, &dc));
    dev.e = de; dev.c = dc;
    FBX_TRY(io.out<double>(nullptr, n_choi, &dev.choi));
    FBX_TRY(io.out(host.it, B, &dev.it)); FBX_TRY(io.out(host.dy, B, &dev.dy)); FBX_TRY(io.out(host.bt, B, &dev.bt));
    FBX_TRY(io.out(host.cost, B, &dev.cost)); FBX_TRY(io.out(host.sw, 4 * B, &dev.sw));
    FBX_TRY(io.out_opt(host.trace, 2 * B * host.trace_iters, &dev.trace));
    if (dev.trace) FBX_HIP(hipMemsetAsync(dev.trace, 0, sizeof(int32_t) * 2 * B * host.trace_iters, stream()));
    const int64_t host_chunk = option_pgdb_host_chunk();
    bool staged = !(host.B > host_chunk && host_pointer_is_pinned(host.e, sizeof(double) * n_in) &&
                    host_pointer_is_pinned(host.c, sizeof(double) * n_in) && host_pointer_is_pinned(host.choi, sizeof(double) * n_choi));
    if (!staged) {
        FBX_TRY(streams.acquire());
        const int rc = pgdb_host_pipelined(host, dev, host_chunk, streams);
        if (rc == FBX_ERR_NOMEM) { streams.drain(); (void)hipGetLastError(); staged = true; }
        else if (rc) return rc;
    }
    if (staged) FBX_TRY(pgdb_host_staged(host, dev));
    FBX_TRY(io.finish());
    return streams.finish();
}

}  // namespace fbx

using namespace fbx;

extern "C" {

#ifdef FBX_DIAGNOSTICS
// diagnostics builds only (libfbx_prof.so / libfbx_cor.so; not part of include/fbx.h, not in libfbx.so):
// device buffer of 8 int64 per item that a -DFBX_PHASE_TIMERS build fills with per-phase shader cycles
int fbx_debug_set_phase_buffer(long long* d_buf) { g_phase_out = d_buf; return FBX_OK; }

// the device natural log used by the PGDB line search, on host arrays
int fbx_debug_log(const double* x, double* out, int64_t n) {
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf dx, dout;
    if ((rc = dx.alloc(sizeof(double) * n)) || (rc = dout.alloc(sizeof(double) * n))) return rc;
    FBX_HIP(hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(debug_log_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream(),
                       dx.as<double>(), dout.as<double>(), (long long)n);
    FBX_HIP(hipGetLastError());
    FBX_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, stream()));
    FBX_HIP(hipStreamSynchronize(stream()));
    return FBX_OK;
}
#endif

int fbx_pgdb_process_ex_dev(const fbx_design* design, int64_t B, const double* d_expect,
                            const double* d_counts, int trace_preserving, int mode, int max_iters,
                            double eig_rel_tol, double* d_choi_out, int32_t* d_iters_out, int32_t* d_dykstra_out,
                            int32_t* d_backtracks_out, double* d_cost_out, int32_t* d_work_out,
                            int32_t* d_trace_out, int trace_iters) {
    PgdbCall call;
    call.des = design; call.B = B; call.e = d_expect; call.c = d_counts; call.tp = trace_preserving; call.mode = mode; call.max_iters = max_iters;
    call.choi = d_choi_out; call.it = d_iters_out; call.dy = d_dykstra_out; call.bt = d_backtracks_out; call.cost = d_cost_out;
    call.sw = d_work_out; call.eig_rel_tol = eig_rel_tol; call.trace = d_trace_out; call.trace_iters = trace_iters;
    FBX_TRY(pgdb_prepare(call));
    if (B == 0) return FBX_OK;
    if (call.trace) FBX_HIP(hipMemsetAsync(call.trace, 0, sizeof(int32_t) * 2 * (size_t)B * trace_iters, stream()));
    return pgdb_dispatch(call);
}

int fbx_pgdb_process_dev(const fbx_design* design, int64_t B, const double* d_expect,
                         const double* d_counts, int trace_preserving, int mode, int max_iters,
                         double* d_choi_out, int32_t* d_iters_out, int32_t* d_dykstra_out,
                         int32_t* d_backtracks_out, double* d_cost_out, int32_t* d_work_out) {
    return fbx_pgdb_process_ex_dev(design, B, d_expect, d_counts, trace_preserving, mode, max_iters, -1.0, d_choi_out,
                                   d_iters_out, d_dykstra_out, d_backtracks_out, d_cost_out, d_work_out, nullptr, 0);
}

int fbx_pgdb_process_ex(const fbx_design* design, int64_t B, const double* expect,
                        const double* counts, int trace_preserving, int mode, int max_iters, double eig_rel_tol,
                        double* choi_out, int32_t* iters_out, int32_t* dykstra_out,
                        int32_t* backtracks_out, double* cost_out, int32_t* work_out,
                        int32_t* trace_out, int trace_iters) {
    PgdbCall host;
    host.des = design; host.B = B; host.e = expect; host.c = counts; host.tp = trace_preserving; host.mode = mode; host.max_iters = max_iters;
    host.choi = choi_out; host.it = iters_out; host.dy = dykstra_out; host.bt = backtracks_out; host.cost = cost_out;
    host.sw = work_out; host.eig_rel_tol = eig_rel_tol; host.trace = trace_out; host.trace_iters = trace_iters; host.total_batch = B;
    FBX_TRY(pgdb_prepare(host));
    if (B == 0) return FBX_OK;
    // fbx_set_devices: contiguous blocks of the batch, one per entry of the device list, each on that entry's
    // worker thread with its own context and a replica of the design; no exchange between devices
    if (device_list_size() > 1 && !in_device_worker() && B >= 2 * (int64_t)device_list_size()) {
        return run_on_devices([&](int g, int G) -> int {       // G: the list's length as run_on_devices read it, under its lock
            const int64_t per = (B + G - 1) / G;
            const int64_t lo = (int64_t)g * per < B ? (int64_t)g * per : B, nb = (B - lo < per ? B - lo : per);
            if (nb <= 0) return FBX_OK;
            int r = ensure_device();
            if (r) return r;
            PgdbCall block = host.slice(lo, nb);
            block.des = design_on_this_device(design, &r);
            if (r) return r;
            return pgdb_process_host(block);
        });
    }
    return pgdb_process_host(host);
}

// _cost / _grad_cost (tomography.py:597-633); include/fbx.h
int fbx_pgdb_cost_grad_dev(const fbx_design* design, int64_t B, const double* d_nvec, const double* d_choi_in, double eps,
                           double* d_cost_out, double* d_grad_out) {
    int rc = ensure_device();
    if (rc) return rc;
    { const int r = check_design(design, "fbx_pgdb_cost_grad"); if (r) return r; }
    FBX_REQUIRE(design->dev.kind == FBX_KIND_PROCESS, "fbx_pgdb_cost_grad: needs a process design");
    FBX_REQUIRE(B >= 0, "fbx_pgdb_cost_grad: negative batch");
    FBX_REQUIRE(B == 0 || (d_nvec && d_choi_in && (d_cost_out || d_grad_out)), "fbx_pgdb_cost_grad: NULL buffer");
    FBX_REQUIRE(eps >= 0.0, "fbx_pgdb_cost_grad: eps must be a non-negative number");      // (also rejects NaN)
    if (B == 0) return FBX_OK;
    switch (design->dev.n) {
        case 1: return launch_cost_grad<1>(design, B, d_nvec, d_choi_in, eps, d_cost_out, d_grad_out);
        case 2: return launch_cost_grad<2>(design, B, d_nvec, d_choi_in, eps, d_cost_out, d_grad_out);
        case 3: return pgdb3_cost_grad_launch(design, B, d_nvec, d_choi_in, eps, d_cost_out, d_grad_out);
    }
    set_error("fbx_pgdb_cost_grad: process designs of 1 to 3 qubits");
    return FBX_ERR_UNSUPPORTED;
}

int fbx_pgdb_cost_grad(const fbx_design* design, int64_t B, const double* nvec, const double* choi_in, double eps,
                       double* cost_out, double* grad_out) {
    FBX_TRY(ensure_device());
    FBX_TRY(check_design(design, "fbx_pgdb_cost_grad"));
    FBX_REQUIRE(B >= 0, "fbx_pgdb_cost_grad: negative batch");
    FBX_REQUIRE(B == 0 || (nvec && choi_in && (cost_out || grad_out)), "fbx_pgdb_cost_grad: NULL buffer");
    if (B == 0) return FBX_OK;
    const size_t m = design->dev.m, DD = (size_t)design->dev.D * design->dev.D;
    HostIO io; double *dn, *dchoi, *dcost, *dgrad;
    FBX_TRY(io.in(nvec, 2 * B * m, &dn)); FBX_TRY(io.in(choi_in, 2 * B * DD, &dchoi));
    FBX_TRY(io.out(cost_out, (size_t)B, &dcost)); FBX_TRY(io.out_opt(grad_out, 2 * B * DD, &dgrad));
    FBX_TRY(fbx_pgdb_cost_grad_dev(design, B, dn, dchoi, eps, dcost, dgrad));
    return io.finish();
}

int fbx_pgdb_process(const fbx_design* design, int64_t B, const double* expect,
                     const double* counts, int trace_preserving, int mode, int max_iters,
                     double* choi_out, int32_t* iters_out, int32_t* dykstra_out,
                     int32_t* backtracks_out, double* cost_out, int32_t* work_out) {
    return fbx_pgdb_process_ex(design, B, expect, counts, trace_preserving, mode, max_iters, -1.0, choi_out, iters_out,
                               dykstra_out, backtracks_out, cost_out, work_out, nullptr, 0);
}

}  // extern "C"
