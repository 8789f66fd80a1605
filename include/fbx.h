/*
 * fbx.h -- C ABI of libfbx.so, the MI355X (gfx950) tomography-reconstruction library.
 *
 * This is the drop-in boundary for the hot path of rigetti/forest-benchmarking
 * (forest/benchmarking/tomography.py:130-633, operator_tools/, distance_measures.py).
 * The reference has no FFI of its own (it is 100 % Python); each entry point below names
 * the reference function it replaces (file:line relative to forest/benchmarking/).
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *  - every entry point returns int: FBX_OK or an FBX_ERR_* category; the message is
 *    available per thread through fbx_last_error().  No exceptions / abort() cross the ABI.
 *  - threading: the library is re-entrant.  Every host thread that calls in owns its own HIP
 *    stream, timer events, staging-buffer pool and cached device workspaces (the 2-qubit PGDB
 *    kernel keeps 128 KiB of Dykstra bases per reconstruction of a launch -- 8 GiB for a 65 536-item
 *    batch, less when the device cannot give that much -- the 3-qubit one 768 MiB);
 *    fbx_release_workspace() gives the calling thread's cached device memory back.  The only
 *    process-wide state is the selected device (one process per GPU: fbx_set_device once,
 *    before other threads use the library) and the RCCL communicator (fbx_comm_*, one thread
 *    at a time).  "The library stream" below is the calling thread's stream.
 *  - all buffers are caller-owned, C-contiguous; complex128 is interleaved (re, im) doubles
 *    (binary compatible with `double _Complex` and numpy complex128); matrices are
 *    row-major [B][row][col].  Plain entry points take HOST pointers and do H2D/D2H
 *    themselves; *_dev entry points take DEVICE pointers (HBM-resident data) and are
 *    asynchronous on the library stream until fbx_synchronize().
 *  - column-stacking vec; un-normalised Choi on H_in (x) H_out; n-qubit Pauli order
 *    itertools.product('IXYZ', repeat=n) with qubits[0] the left-most tensor factor.
 *  - sizes: the estimators, projections, state measures and channel application take 1..3 qubits
 *    (fbx_kraus_sweep is one fused kernel for 1..2 and a composition of the pairwise conversions for 3);
 *    the state estimators on a state design, fbx_proj_state_physical and fbx_state_measures 1..5 qubits;
 *    fbx_convert and fbx_process_fidelity 1..5 qubits; fbx_diamond_norm 1..3 qubits; fbx_chernoff_bound 1..5 qubits;
 *    fbx_eigh / fbx_matmul any N <= 1024;
 *    fbx_convert_general and fbx_partial_trace any dimension (each entry point states its own range).
 *  - label codes: one-qubit input states 0:X+ 1:X- 2:Y+ 3:Y- 4:Z+ 5:Z- 6:SIC0 7:SIC1
 *    8:SIC2 9:SIC3; one-qubit Paulis 0:I 1:X 2:Y 3:Z.
 */
#ifndef FBX_H
#define FBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBX_OK               0
#define FBX_ERR_BAD_ARG      1   /* -> ValueError in the Python shim */
#define FBX_ERR_HIP          2   /* HIP runtime / kernel failure */
#define FBX_ERR_NO_DEVICE    3   /* no gfx950 device visible: the product fails loudly */
#define FBX_ERR_UNSUPPORTED  4   /* valid request outside what this build implements */
#define FBX_ERR_NOMEM        5
#define FBX_ERR_RCCL         6   /* RCCL (multi-GPU) failure, or librccl.so could not be opened */

#define FBX_KIND_STATE    0
#define FBX_KIND_PROCESS  1

/* pgdb modes */
#define FBX_MODE_CONVERGE 0   /* reference loop: stop when old_cost - new_cost < 1e-10
                                 (tomography.py:589); max_iters > 0 adds a cap */
#define FBX_MODE_FIXED    1   /* exactly max_iters outer iterations (benchmark mode) */
/* Flag, OR-ed into either mode of fbx_pgdb_process* (per call): the backtracking line search of tomography.py:575-585 taken
 * LITERALLY -- every halving evaluates the full cost sum and the acceptance test is the reference's rounded comparison
 * `new_cost > old_cost + change` -- instead of the default, which knows the cost DIFFERENCE of a small step exactly (a power
 * series in alpha) and tests that.  The two agree wherever the comparison is not decided by the rounding of the cost sums,
 * i.e. in every iteration up to the reference's own stopping point (tests hold the halving counts equal there); past it
 * (FBX_MODE_FIXED beyond convergence) the reference performs a rounding-driven walk that no other summation order
 * reproduces, and this flag yields ANOTHER such walk, not the reference's.  Slower: ~50 full cost
 * evaluations per stalled iteration.  Ignored for 3 qubits, whose kernel always evaluates this way. */
#define FBX_MODE_LS_REFERENCE 0x100

/* superoperator representations for fbx_convert */
#define FBX_REP_KRAUS   0
#define FBX_REP_CHOI    1
#define FBX_REP_SUPEROP 2
#define FBX_REP_PAULI_LIOUVILLE 3
#define FBX_REP_CHI     4

/* Choi projections for fbx_proj_choi */
#define FBX_PROJ_CP        0  /* project_superoperators.py:19  proj_choi_to_completely_positive */
#define FBX_PROJ_TP        1  /* project_superoperators.py:62  proj_choi_to_trace_preserving    */
#define FBX_PROJ_TNI       2  /* project_superoperators.py:37  proj_choi_to_trace_non_increasing */
#define FBX_PROJ_PHYSICAL_TP  3  /* project_superoperators.py:87 proj_choi_to_physical(.., True)  */
#define FBX_PROJ_PHYSICAL_TNI 4  /* project_superoperators.py:87 proj_choi_to_physical(.., False) */

typedef struct fbx_design fbx_design;   /* opaque: owns the device copy of a design */
typedef struct fbx_grouping fbx_grouping;   /* opaque: owns the device tables of a grouping of a design's settings */

/* ---------------------------------------------------------------- library / device */
int         fbx_version(void);
const char* fbx_last_error(void);
int         fbx_device_count(int* count);
int         fbx_set_device(int device_id);          /* one process per GPU: call once */
/* One call, several GPUs (SURVEY.md 8b "fbx_set_devices(ids, count)", 8e "host thread per device does H2D of its slab,
 * launches, D2H"; the unit that is split is the reference's independent experiment, e.g. one entry of
 * get_results_by_qubit_groups, observable_estimation.py:1145-1173).  ids[0] becomes the process's device (fbx_set_device);
 * with count > 1 the HOST-POINTER batch entry points fbx_pgdb_process[_ex] and fbx_kraus_sweep split a batch of at least
 * 2 x count items into contiguous blocks and run block g on entry g of the list, on a long-lived worker thread of the
 * library that owns that device's stream, staging pool, workspaces and a replica of the design -- no exchange between
 * devices, results bit-identical to the single-device call.  A device may be listed more than once (two workers share
 * it).  count <= 1 restores the single-device behaviour.  The *_dev entry points and everything else stay on the calling
 * thread's device; multi-PROCESS runs (one rank per GPU, fbx_comm_*) do not need this call. */
int         fbx_set_devices(const int* device_ids, int count);
int         fbx_device_name(char* buf, size_t len, int* compute_units);
int         fbx_device_id(int* ordinal, char* pci_bus_id, size_t len);   /* the selected device; "0000:05:00.0"-style id (len >= 16) */
int         fbx_synchronize(void);                  /* the calling thread's stream */
/* Frees the calling thread's cached device workspaces / staging pool.  With a device list of more than one entry
 * (fbx_set_devices) it ALSO asks every device worker to free its own and waits for them: it takes the device-list lock, so it
 * blocks while a multi-device call of any thread is running, and returns the first worker's error code if one fails. */
int         fbx_release_workspace(void);
/* Process-wide DEFAULTS, read when a kernel is launched.  A thread that needs its own value passes it per call
 * (fbx_pgdb_process_ex): changing an option changes the arithmetic of every thread's later launches.
 *   "pgdb_eig_rel_tol"  (default 1e-8), "pgdb3_eig_rel_tol" (default 1e-7; 3 qubits): while the projected-gradient
 *   iteration of fbx_pgdb_process is far from its fixed point, the eigensolver of its CP projections stops at an
 *   off-diagonal norm of <value> x the previous outer step (relative to ||H||_F) instead of always at 1e-13 --
 *   an inexact projection whose error is that fraction of the distance the estimate still moves per iteration.
 *   0 reproduces the reference's eigh-to-machine-precision trajectory iteration by iteration (tests use it);
 *   the defaults leave the converged estimates within 1e-9 of the reference's.  Range [0, 1e-3].
 *   "pgdb_host_chunk" (default 4096): items of the first and of the last stage of the pipelined host-pointer form of
 *   fbx_pgdb_process (see fbx_host_alloc); the bulk in between goes in one launch per 65 536 items.
 *   "eigh_cooperative" (default 1): fbx_eigh of a few matrices with N >= 128 spreads each matrix over the whole chip with a
 *   cooperative launch; 0 keeps one workgroup per matrix.
 *   "pgdb_packed_1q" (default 1): single-qubit fbx_pgdb_process* with at most 64 settings and at least 8192 experiments (16 384 for designs of more than 12 settings) runs
 *   64 reconstructions per wavefront, one per lane (csrc/fbx_pgdb1.hip; same line-search rule as the other kernels, the
 *   eigensolver always at full tolerance; a call that passes an explicit eig_rel_tol >= 0 to fbx_pgdb_process_ex[_dev]
 *   therefore stays on the wavefront-per-reconstruction kernel whatever its batch size, so that an experiment's iterates do
 *   not depend on how many neighbours it is batched with); 2 = the lane-per-item kernel for every batch size and every
 *   tolerance argument (diagnostics / tests), 0 = never (the wavefront-per-reconstruction kernel, which smaller batches and
 *   larger designs use).
 *   "pgdb_pieces" (default 8): two-qubit fbx_pgdb_process* of more than 1024 experiments (and single-qubit ones of 1025 .. 8191
 *   with a fixed iteration count) runs every reconstruction as that many pieces of outer iterations, drawn from a ticket counter by persistent workgroups, so that a launch does not wait for
 *   whole reconstructions at its end (csrc/fbx_pgdb_lean.hip); 1 = whole reconstructions.  Results do not depend on it.
 *   "pgdb1_binned" (default 1): the lane-per-reconstruction single-qubit kernel runs one launch per outer iteration with the
 *   reconstructions re-binned by Dykstra count in between from 2^20 experiments to convergence (2^19 for at most 12 settings;
 *   2^17 for a fixed iteration count); 2 = always, 0 = never (one persistent launch).  Results do not depend on it; the binned
 *   form holds 3.5 KB + 16 m bytes of device workspace per reconstruction and synchronises the calling thread's stream.
 *   "qv_wide_workspace_mib" (default 128, range [1, 65536]): fbx_qv_heavy_outputs_wide[_dev] runs its batch in chunks of as many
 *   circuits as fit this many MiB of device workspace (always at least one circuit).  Results do not depend on it.
 *   "sample_wide_workspace_mib" (default 128, range [1, 65536]): fbx_sample_bitstrings_wide[_dev] runs its batch in chunks of as
 *   many items as fit this many MiB of device workspace (always at least one item).  Results do not depend on it.
 *   "qv_noisy_workspace_mib" (default 128, range [1, 65536]): fbx_qv_noisy_trajectories[_dev] with probs_mean_out runs its batch
 *   in chunks of as many circuits as fit this many MiB of partial sums (always at least one circuit).  Results do not depend on it.
 *   "native_workspace_mib" (default 128, range [1/64, 65536]): fbx_native_trajectories[_dev] with probs_mean_out runs its batch in
 *   chunks of as many (item, input) pairs as fit this many MiB of partial sums (always at least one pair).  Results do not depend
 *   on it. */
int         fbx_set_option(const char* name, double value);
int         fbx_get_option(const char* name, double* value);

/* ---------------------------------------------------------------- multi-GPU
 * One process per GPU; RCCL over xGMI.  The reconstruction path shards on the batch axis (the
 * independent units of observable_estimation.py:1145-1173 get_results_by_qubit_groups,
 * tomography.py:440-451 bootstrap resamples) with NO collective on the data path; these entry
 * points cover what ranks exchange around it: broadcast of design-sized constants, all-gather
 * of result slabs, all-reduce of a summary vector.  Rank 0 obtains an id with
 * fbx_comm_unique_id, hands the FBX_COMM_ID_BYTES bytes to the other ranks by any host channel,
 * every rank calls fbx_comm_init (collective).  Collectives are enqueued on the calling thread's
 * stream (the *_dev forms are asynchronous like every other *_dev entry point).  librccl.so is
 * opened on first use. */
#define FBX_COMM_ID_BYTES 128
#define FBX_COMM_SUM 0
#define FBX_COMM_MAX 1
#define FBX_COMM_MIN 2
int fbx_comm_unique_id(uint8_t* id_out /* [FBX_COMM_ID_BYTES] */);
int fbx_comm_init(const uint8_t* id, int rank, int world);   /* = fbx_comm_init_timeout with 180 s (env FBX_RCCL_INIT_TIMEOUT) */
/* ncclCommInitRank is a collective: it blocks for as long as a peer is missing.  It runs in a helper thread of the
 * library (no library lock is held meanwhile); when it has not returned after timeout_seconds the call fails with
 * FBX_ERR_RCCL and the process can form no further communicator (every later fbx_comm_* call says so at once). */
int fbx_comm_init_timeout(const uint8_t* id, int rank, int world, double timeout_seconds);
int fbx_comm_info(int* rank, int* world, int* rccl_version);   /* world = 0 without a communicator */
/* rank / size / device as the COMMUNICATOR reports them (ncclCommUserRank, ncclCommCount, ncclCommCuDevice) */
int fbx_comm_query(int* rank, int* world, int* device);
int fbx_comm_destroy(void);
int fbx_comm_allgather_dev(const void* d_send, void* d_recv /* [world][bytes_per_rank] */,
                           size_t bytes_per_rank);
int fbx_comm_broadcast_dev(void* d_buf, size_t bytes, int root);
int fbx_comm_allreduce_f64_dev(const double* d_send, double* d_recv, size_t n, int op);
int fbx_comm_allreduce_f64(double* host_inout, size_t n, int op);   /* host vector of any length (meant for summary vectors); synchronises */
int fbx_comm_barrier(void);   /* all ranks' work enqueued by the calling threads is complete */

/* device memory helpers so callers can keep batches resident in HBM */
int fbx_malloc(void** dev_ptr, size_t bytes);
int fbx_free(void* dev_ptr);
int fbx_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes);
int fbx_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes);

/* page-locked host memory: caller buffers allocated here cross PCIe at the full rate and asynchronously; when
 * expect, counts and choi_out of fbx_pgdb_process[_ex] are all page-locked and the batch exceeds one stage
 * (fbx_set_option "pgdb_host_chunk", default 4096 items), the call overlaps H2D, kernels and D2H: a small first stage covers the
 * upload of the rest, the bulk runs on a high-priority stream, a small last stage covers the download of the bulk's results */
int fbx_host_alloc(void** host_ptr, size_t bytes);
int fbx_host_free(void* host_ptr);

/* HIP-event timing of everything enqueued on the library stream between begin and end */
int fbx_timer_begin(void);
int fbx_timer_end(double* elapsed_ms);

/* ---------------------------------------------------------------- designs
 * A design is the data-independent half of an experiment: m settings on n qubits, shared by
 * every item of a batch.  Replaces the per-call rebuilding of measurement operators in
 * tomography.py:159-160 (linear inversion), :326-327 (_R), :482-486, :494-539
 * (_extract_from_results).  in_labels / paulis are [m][n_qubits] codes (in_labels may be
 * NULL for FBX_KIND_STATE); coefs[m] are the observables' real coefficients (NULL = 1).
 * n_qubits: 1..3 for process designs (4^n x 4^n Choi matrices up to 64 x 64), 1..5 for state designs
 * (density matrices up to 32 x 32, 1023 settings). */
int fbx_design_create(int n_qubits, int kind, int m, const uint8_t* in_labels,
                      const uint8_t* paulis, const double* coefs, fbx_design** out);
int fbx_design_destroy(fbx_design* design);
int fbx_design_info(const fbx_design* design, int* n_qubits, int* kind, int* m,
                    int* n_input_states);

/* ---------------------------------------------------------------- process estimators
 * fbx_pgdb_process replaces pgdb_process_estimate (tomography.py:542-594) together with
 * _extract_from_results (:494-539), _cost (:597-614), _grad_cost (:617-633) and
 * proj_choi_to_physical (operator_tools/project_superoperators.py:87-144), for a batch of B
 * independent experiments that share `design`.
 *   expect[B][m], counts[B][m]  -- ExperimentResult.expectation / .total_counts
 *   choi_out[B][D][D] complex128, D = 4^n
 *   iters_out / dykstra_out / backtracks_out [B] (may be NULL): outer iterations, total
 *   Dykstra (= eigendecomposition) iterations, total step halvings; cost_out[B] (may be
 *   NULL): final negative log-likelihood; work_out[B][4] (may be NULL): work accounting --
 *   Jacobi sweeps of the eigensolver, eigenvalue terms rebuilt by the CP projections, cost
 *   evaluations over all outcomes, power-sum reductions of the small-step line search
 *   (bench.py derives the executed flops from these counters).
 * Design sizes: 1 and 2 qubits any number of settings (above 256 / 1024 the outcome slots are streamed from HBM, slower);
 * 3 qubits up to 65 536 settings (FBX_ERR_UNSUPPORTED beyond); process designs above 3 qubits are refused by
 * fbx_design_create. */
int fbx_pgdb_process(const fbx_design* design, int64_t B, const double* expect,
                     const double* counts, int trace_preserving, int mode, int max_iters,
                     double* choi_out, int32_t* iters_out, int32_t* dykstra_out,
                     int32_t* backtracks_out, double* cost_out, int32_t* work_out);
int fbx_pgdb_process_dev(const fbx_design* design, int64_t B, const double* d_expect,
                         const double* d_counts, int trace_preserving, int mode,
                         int max_iters, double* d_choi_out, int32_t* d_iters_out,
                         int32_t* d_dykstra_out, int32_t* d_backtracks_out,
                         double* d_cost_out, int32_t* d_work_out);

/* The same estimator with per-call arguments (what concurrent callers use instead of the process-wide option):
 *   eig_rel_tol   tolerance factor of the CP projections' eigensolver for THIS call (see fbx_set_option
 *                 "pgdb_eig_rel_tol"); negative = the process default; 0 = the reference's eigh-to-machine-precision
 *                 trajectory; range [0, 1e-3]
 *   trace_out     [B][trace_iters][2] int32 (may be NULL): for every outer iteration k < trace_iters of item b the
 *                 Dykstra iterations (proj_choi_to_physical, project_superoperators.py:112-144) and the step halvings
 *                 (tomography.py:578-585) of that iteration; rows beyond the item's last iteration are zero. */
int fbx_pgdb_process_ex(const fbx_design* design, int64_t B, const double* expect,
                        const double* counts, int trace_preserving, int mode, int max_iters,
                        double eig_rel_tol, double* choi_out, int32_t* iters_out,
                        int32_t* dykstra_out, int32_t* backtracks_out, double* cost_out,
                        int32_t* work_out, int32_t* trace_out, int trace_iters);
int fbx_pgdb_process_ex_dev(const fbx_design* design, int64_t B, const double* d_expect,
                            const double* d_counts, int trace_preserving, int mode, int max_iters,
                            double eig_rel_tol, double* d_choi_out, int32_t* d_iters_out,
                            int32_t* d_dykstra_out, int32_t* d_backtracks_out, double* d_cost_out,
                            int32_t* d_work_out, int32_t* d_trace_out, int trace_iters);

/* _cost and _grad_cost (tomography.py:597-614, :617-633) as functions of their own: ONE evaluation of the negative log-likelihood
 * -n^T log(clip(A vec(E), eps)) and of its gradient -unvec(A^H (n / clip(A vec(E), eps))) at the Choi matrices choi_in[B][D][D]
 * (Hermitian, as every iterate of the estimator is), computed with the device functions of the reconstruction kernels (Pauli
 * transform, prediction table T = R C, per-state weights, R^G = -(W C^T) / d^2, inverse transform): a diagnostic that pins the
 * gradient -- which fbx_pgdb_process never outputs -- directly.  `nvec` is the reference's n of _extract_from_results
 * (tomography.py:528-538): [B][2 m], row 2 k / 2 k + 1 = the +1 / -1 counts of result k over the grand total.  `design` stands
 * for A (never materialised).  cost_out[B] or grad_out[B][D][D] may be NULL (not both).  1..3 qubits, any number of settings. */
int fbx_pgdb_cost_grad(const fbx_design* design, int64_t B, const double* nvec, const double* choi_in, double eps,
                       double* cost_out, double* grad_out);
int fbx_pgdb_cost_grad_dev(const fbx_design* design, int64_t B, const double* d_nvec, const double* d_choi_in, double eps,
                           double* d_cost_out, double* d_grad_out);

/* linear_inv_process_estimate (tomography.py:459-491): choi_out[B][D][D]. */
int fbx_linv_process(const fbx_design* design, int64_t B, const double* expect,
                     double* choi_out);
int fbx_linv_process_dev(const fbx_design* design, int64_t B, const double* d_expect,
                         double* d_choi_out);

/* ---------------------------------------------------------------- state estimators (1..5 qubits)
 * linear_inv_state_estimate (tomography.py:130-165): rho_out[B][d][d], d = 2^n. */
int fbx_linv_state(const fbx_design* design, int64_t B, const double* expect, double* rho_out);
int fbx_linv_state_dev(const fbx_design* design, int64_t B, const double* d_expect,
                       double* d_rho_out);

/* iterative_mle_state_estimate (tomography.py:168-270) incl. _R (:273-338): diluted
 * iterative MLE with optional max-entropy (entropy_penalty > 0) or hedging (beta > 0).
 * Performs at most maxiter-1 updates like the reference; hit_max_out[b] = 1 where the cap was
 * reached (the shim then emits the reference's warning). */
int fbx_mle_state(const fbx_design* design, int64_t B, const double* expect,
                  const double* counts, double epsilon, double entropy_penalty, double beta,
                  double tol, int maxiter, double* rho_out, int32_t* iters_out,
                  int32_t* hit_max_out);
int fbx_mle_state_dev(const fbx_design* design, int64_t B, const double* d_expect,
                      const double* d_counts, double epsilon, double entropy_penalty, double beta,
                      double tol, int maxiter, double* d_rho_out, int32_t* d_iters_out,
                      int32_t* d_hit_max_out);

/* _R (tomography.py:273-338): r_out[B][d][d] for given states rho[B][d][d]. */
int fbx_r_operator(const fbx_design* design, int64_t B, const double* rho, const double* expect,
                   double* r_out);
int fbx_r_operator_dev(const fbx_design* design, int64_t B, const double* d_rho,
                       const double* d_expect, double* d_r_out);

/* state_log_likelihood (tomography.py:341-375): ll_out[B] (log10). */
int fbx_state_log_likelihood(const fbx_design* design, int64_t B, const double* rho,
                             const double* expect, const double* counts, double* ll_out);
int fbx_state_log_likelihood_dev(const fbx_design* design, int64_t B, const double* d_rho,
                                 const double* d_expect, const double* d_counts,
                                 double* d_ll_out);

/* ---------------------------------------------------------------- operator tools
 * fbx_convert: the pairwise conversions of operator_tools/superoperator_transformations.py
 * :82-371.  `in` is [B][K][d][d] for FBX_REP_KRAUS (K operators per item), else [B][D][D];
 * `out` is [B][D][D].  Conversions *to* Kraus are fbx_choi2kraus below (eigenvector-valued outputs
 * are only defined up to phase, superoperator_transformations.py:325-336).  n_qubits 1..5; for
 * 4 and 5 qubits (256^2 / 1024^2 matrices, work matrices in HBM) the conversions INTO chi from a Choi /
 * superoperator / Pauli-Liouville matrix -- which the reference routes through a D x D eigendecomposition
 * (choi2kraus: chi of |C|, eigenvalues within 1e-9 dropped) -- are composed from fbx_eigh_dev, fbx_matmul_dev and the
 * linear basis change (25 ms per 256 x 256 item, ~1 s per 1024 x 1024 item: complete, not fast).  Kraus sets with more
 * operators than the fused kernels stage in LDS (K x D x 16 B against 160 KiB) go through the basis-free kernel
 * (fbx_convert_general: any K) to the Choi matrix and on from there.
 * Non-finite input: on a route INTO chi from a Choi / superoperator / Pauli-Liouville matrix, an item with a NaN or an Inf in an
 * entry the route reads is not converted.  Every entry of its output is NaN, the call returns FBX_OK, and every other item is
 * bit-identical to the same call with a finite matrix in that place.  From a Choi matrix the route reads what the reference's
 * eigh reads: the real parts of the diagonal and the strict lower triangle (the strict upper triangle and the diagonal's
 * imaginary parts are never read: NaN or Inf there changes nothing).  From a superoperator or a Pauli-Liouville matrix it reads
 * every entry.  (Left to the arithmetic, the eigensolver's stopping test is false on a NaN or an infinite norm and the cut at
 * 1e-9 turns a NaN eigenvalue into 0: the result would be a finite chi matrix of some other input.)  The other routes are linear
 * maps, entry by entry: a non-finite entry reaches the output entries that depend on it -- through superop <-> choi, a
 * permutation, exactly one -- and no other item. */
int fbx_convert(int from_rep, int to_rep, int n_qubits, int64_t B, const double* in, int K,
                double* out);
/* same with device pointers (buffers from fbx_malloc): the batch stays resident in HBM */
int fbx_convert_dev(int from_rep, int to_rep, int n_qubits, int64_t B, const double* d_in, int K,
                    double* d_out);
/* The conversions that involve no operator basis, for ANY Hilbert-space dimension `dim` (qutrits, ...;
 * 1..256): kraus -> superop (superoperator_transformations.py:100-145), kraus -> choi (:159-182),
 * superop <-> choi (:267-277, :351-361).  Shapes as above with d = dim, D = dim^2. */
int fbx_convert_general(int from_rep, int to_rep, int dim, int64_t B, const double* in, int K, double* out);
int fbx_convert_general_dev(int from_rep, int to_rep, int dim, int64_t B, const double* d_in, int K,
                            double* d_out);

/* Fused conversion sweep of BASELINE config 3: kraus2choi -> choi2pauli_liouville ->
 * choi2chi -> process_fidelity(ptm_ref, ptm) (superoperator_transformations.py:159,364,339;
 * distance_measures.py:315).  Any of choi_out / ptm_out / chi_out / fid_out may be NULL. */
int fbx_kraus_sweep(int n_qubits, int64_t B, int K, const double* kraus, const double* ptm_ref,
                    double* choi_out, double* ptm_out, double* chi_out, double* fid_out);
int fbx_kraus_sweep_dev(int n_qubits, int64_t B, int K, const double* d_kraus,
                        const double* d_ptm_ref, double* d_choi_out, double* d_ptm_out,
                        double* d_chi_out, double* d_fid_out);

/* Choi projections (operator_tools/project_superoperators.py:19-144): out[B][D][D];
 * iters_out[B] (may be NULL) = Dykstra iterations for the PHYSICAL kinds, 0 for the others.
 * Non-finite input: an item with a NaN or an Inf in any entry is not projected.  Every entry of its output is NaN, its count is
 * 1 for the PHYSICAL kinds (the iteration in which the reference's check_finite raises), the call returns FBX_OK, and every
 * other item is bit-identical to the same call with a finite matrix in that place.  (Left to the arithmetic, the eigensolver's
 * stopping test is false on a NaN or an infinite norm: the CP projection of a matrix with a NaN off its diagonal would be the
 * finite max(diag, 0).)  The input need not be Hermitian: CP projects its Hermitian part, TNI Hermitises the partial trace for
 * the eigensolver only. */
int fbx_proj_choi(int proj_kind, int n_qubits, int64_t B, const double* choi, double* out,
                  int32_t* iters_out);

int fbx_proj_choi_dev(int proj_kind, int n_qubits, int64_t B, const double* d_choi, double* d_out,
                      int32_t* d_iters_out);

/* project_state_matrix_to_physical (operator_tools/project_state_matrix.py:6-52): rho[B][d][d] -> out[B][d][d], d = 2^n_qubits,
 * n_qubits 1..5 (others FBX_ERR_BAD_ARG).  The lower triangle of rho / tr(rho) is diagonalised; when no eigenvalue is negative
 * the output is rho / tr(rho) as it stands, else the rebuilt matrix.  A non-finite item gives non-finite entries for that item
 * only (NaN in every entry at 4 and 5 qubits).  The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_proj_state_physical(int n_qubits, int64_t B, const double* rho, double* out);
int fbx_proj_state_physical_dev(int n_qubits, int64_t B, const double* d_rho, double* d_out);

/* apply_choi_matrix_2_state (operator_tools/apply_superoperator.py:60-90): out[B][d][d]. */
int fbx_apply_choi(int n_qubits, int64_t B, const double* choi, const double* rho, double* out);
int fbx_apply_choi_dev(int n_qubits, int64_t B, const double* d_choi, const double* d_rho,
                       double* d_out);

/* tensor_channel_kraus / compose_channel_kraus (operator_tools/compose_superoperators.py:7-44) for
 * batches: k2[B][K2][rows2][cols2], k1[B][K1][rows1][cols1]; out[B][K1*K2][.][.] with operator
 * p = j*K2 + l (the reference's list order) = kron(k2[l], k1[j]) when tensor != 0, else k2[l] . k1[j]
 * (needs cols2 == rows1). */
int fbx_kraus_pairs(int tensor, int64_t B, int K2, int rows2, int cols2, int K1, int rows1, int cols1,
                    const double* k2, const double* k1, double* out);
int fbx_kraus_pairs_dev(int tensor, int64_t B, int K2, int rows2, int cols2, int K1, int rows1,
                        int cols1, const double* d_k2, const double* d_k1, double* d_out);

/* pauli_twirl_chi_matrix (operator_tools/channel_approximation.py:31-49): out[B][D][D] keeps the
 * diagonal of chi[B][D][D]. */
int fbx_pauli_twirl_chi(int64_t B, int D, const double* chi, double* out);
int fbx_pauli_twirl_chi_dev(int64_t B, int D, const double* d_chi, double* d_out);

/* entanglement_fidelity / process_fidelity (distance_measures.py:271-359) on
 * Pauli-Liouville matrices [B][D][D] (real parts of tr(A^H B) / d^2): fe_out, fp_out may be
 * NULL.  n_qubits 1..5. */
int fbx_process_fidelity(int n_qubits, int64_t B, const double* ptm0, const double* ptm1,
                         double* fe_out, double* fp_out);
int fbx_process_fidelity_dev(int n_qubits, int64_t B, const double* d_ptm0, const double* d_ptm1,
                             double* d_fe_out, double* d_fp_out);

/* Diamond-norm distance of B pairs of channels (distance_measures.py:378-437), Choi matrices [B][D][D], D = 4^n_qubits,
 * n_qubits 1..3 (others FBX_ERR_UNSUPPORTED).  choi1 is [B][D][D], or one shared [D][D] when choi1_shared != 0.  Every pair is
 * solved to a certified relative gap: dist_out[b] = 2 g(rho) for the returned input state rho (a lower bound, g(rho) =
 * tr[((1 (x) rho^1/2) J (1 (x) rho^1/2))_+], J the Hermitian part of choi0 - choi1), upper_out[b] an upper bound from a
 * dual-feasible certificate; the search stops once upper - dist <= tol * max(dist, 1e-12) (tol <= 0: 1e-7) or after
 * max_iters quasi-Newton steps.  rho_out [B][d][d] (the maximising input state), iters_out[B] (steps taken; negative when
 * tol was not reached -- the bounds still hold).  upper_out, rho_out, iters_out may be NULL.  A non-finite input gives a NaN
 * result for that pair only. */
int fbx_diamond_norm(int n_qubits, int64_t B, const double* choi0, const double* choi1, int choi1_shared, double tol,
                     int max_iters, double* dist_out, double* upper_out, double* rho_out, int32_t* iters_out);
int fbx_diamond_norm_dev(int n_qubits, int64_t B, const double* d_choi0, const double* d_choi1, int choi1_shared, double tol,
                         int max_iters, double* d_dist_out, double* d_upper_out, double* d_rho_out, int32_t* d_iters_out);

/* Quantum Chernoff bound of B pairs of states (distance_measures.py:153-195): qcb = min over s in [0, 1] of
 * Q(s) = tr(rho^s sigma^(1-s)), rho [B][d][d] and sigma [B][d][d] or one shared [d][d] (sigma_shared != 0), d = 2^n_qubits,
 * n_qubits 1..5 (others FBX_ERR_UNSUPPORTED).  The LOWER triangles are read (numpy's eigh).  An eigenvalue <= zero_tol * lambda_max
 * of its own matrix (negative ones included; zero_tol in [0, 1), the Python default 1e-12) counts as exactly zero and its terms are
 * left out at every s, the endpoints included (support projectors); zero_tol = 0 keeps every eigenvalue > 0, as
 * quantum_chernoff_bound does.  Q is convex; per pair a safeguarded Newton search on Q' gives qcb_out[b] (the smallest evaluated
 * Q, an upper bound up to rounding) and s_out[b] (where it was reached), and the tangents at the two ends of the final bracket give
 * lower_out[b] <= the exact minimum.  The search stops once qcb - lower <= tol * max(qcb, 1e-12) (tol <= 0: 1e-10) or after
 * max_iters evaluations besides the two endpoints.  iters_out[b] = those evaluations, negative when tol was not reached (both
 * bounds still hold).  lower_out, s_out, iters_out may be NULL.  A non-finite item gives NaN (iters -1) in that item only.
 * Rounding: lower is shifted down by a bound on the rounding of Q and Q' (fbx_chernoff.hip), so it is a lower bound of the exact
 * minimum over the COMPUTED eigendecompositions; qcb may fall below that minimum by at most (8 L + 16 + d^2) 2^-52 relative,
 * L = the largest |ln a_i| + |ln b_j| over the kept terms (below 2e-13 for unit-trace states at zero_tol = 1e-12).  The
 * eigensolver's own backward error (~1e-15 relative to lambda_max) is outside both statements.  A shared sigma gives the same bits
 * as the same sigma passed per item; results do not depend on the batch. */
int fbx_chernoff_bound(int n_qubits, int64_t B, const double* rho, const double* sigma, int sigma_shared, double tol,
                       int max_iters, double zero_tol, double* qcb_out, double* lower_out, double* s_out, int32_t* iters_out);
int fbx_chernoff_bound_dev(int n_qubits, int64_t B, const double* d_rho, const double* d_sigma, int sigma_shared, double tol,
                           int max_iters, double zero_tol, double* d_qcb_out, double* d_lower_out, double* d_s_out,
                           int32_t* d_iters_out);

/* State measures (distance_measures.py:14-114, :198): purity tr(rho^2), fidelity
 * (tr sqrt(sqrt(rho) sigma sqrt(rho)))^2, trace_distance = 0.5 * induced 1-norm,
 * hilbert_schmidt_ip Re tr(rho^H sigma); rho, sigma are [B][d][d], d = 2^n_qubits, n_qubits 1..5 (others FBX_ERR_BAD_ARG);
 * out arrays [B], NULL to skip (without the fidelity no eigendecomposition runs).  Both square roots of the fidelity go through
 * the spectrum clipped at zero; rho enters it through its lower triangle.  At 4 and 5 qubits a non-finite pair gives NaN in every
 * output asked for.  The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_state_measures(int n_qubits, int64_t B, const double* rho, const double* sigma,
                       double* purity_out, double* fidelity_out, double* trace_dist_out,
                       double* hs_ip_out);
int fbx_state_measures_dev(int n_qubits, int64_t B, const double* d_rho, const double* d_sigma,
                           double* d_purity_out, double* d_fidelity_out,
                           double* d_trace_dist_out, double* d_hs_ip_out);

/* ---------------------------------------------------------------- plot inputs
 * Pauli-Liouville vector of a state, the input of plotting/state_process.py:10-87:
 * out[b][k] = (computational2pauli_basis_matrix(2 n) vec(rho_b))[k] = tr[P_k rho_b] / d (real part), P_k in the
 * order of n_qubit_pauli_basis(n).labels (utils.py:398-409; itertools.product('IXYZ', repeat=n)).
 * rho is [B][d][d] complex, out [B][d^2] real; n_qubits 1..5.  (The Pauli transfer matrix that
 * plot_pauli_transfer_matrix (:90) draws is fbx_convert(FBX_REP_CHOI -> FBX_REP_PAULI_LIOUVILLE).) */
int fbx_pauli_vector(int n_qubits, int64_t B, const double* rho, double* out);
int fbx_pauli_vector_dev(int n_qubits, int64_t B, const double* d_rho, double* d_out);

/* ---------------------------------------------------------------- shots -> moments
 * shots_to_obs_moments (observable_estimation.py:804-853), the reduction immediately before the
 * estimators: for each of n_settings settings, bits[s] is a [n_shots][n_qubits] array of 0/1 bytes
 * (one row per shot, as qc.run returns it), obs_mask[s][q] != 0 where the setting's observable acts
 * on column q, coefs[s] its real coefficient (NULL = 1).  mean_out[s] = coef * mean of the +-1
 * products, var_out[s] = variance of that mean (coef^2 (1 - m^2) / n_shots), or the Beta(n+ + 1,
 * n- + 1) moments when beta_prior != 0 (use_beta_dist_unbiased_prior).  An all-zero mask is the
 * identity term: (coef, 0).  Only bit 0 of a byte of bits is read; any non-zero byte of obs_mask
 * selects its column. */
int fbx_shots_to_moments(int n_qubits, int64_t n_settings, int64_t n_shots, const uint8_t* bits,
                         const uint8_t* obs_mask, const double* coefs, int beta_prior,
                         double* mean_out, double* var_out);
int fbx_shots_to_moments_dev(int n_qubits, int64_t n_settings, int64_t n_shots, const uint8_t* d_bits,
                             const uint8_t* d_obs_mask, const double* d_coefs, int beta_prior,
                             double* d_mean_out, double* d_var_out);

/* Readout-calibration rescale, the arithmetic of calibrate_observable_estimates
 * (observable_estimation.py:1028-1037) with ratio_variance (:1052-1090), for B experiments x m settings:
 * mean_out = expect / cal_mean[c], err_out = sqrt(std_err^2 / cal_mean[c]^2 + expect^2 cal_var[c] /
 * cal_mean[c]^4) with c = cal_index[k] (the calibration of setting k's observable; cal_index NULL =
 * one calibration per setting, n_cal == m).  cal_mean / cal_var are the shots_to_obs_moments of the
 * calibration runs (fbx_shots_to_moments). */
int fbx_calibrate_expectations(int64_t B, int64_t m, const double* expect, const double* std_err,
                               const int32_t* cal_index, int64_t n_cal, const double* cal_mean,
                               const double* cal_var, double* mean_out, double* err_out);
int fbx_calibrate_expectations_dev(int64_t B, int64_t m, const double* d_expect,
                                   const double* d_std_err, const int32_t* d_cal_index, int64_t n_cal,
                                   const double* d_cal_mean, const double* d_cal_var,
                                   double* d_mean_out, double* d_err_out);

/* estimate_dfe (direct_fidelity_estimation.py:224-307), batched: for each of B experiments with m
 * settings on n_qubits, expect[B][m] and std_err[B][m] -> the direct fidelity estimate and its standard
 * error; kind = FBX_KIND_STATE (state fidelity) or FBX_KIND_PROCESS (average gate fidelity). */
int fbx_dfe_estimate(int n_qubits, int kind, int64_t B, int64_t m, const double* expect,
                     const double* std_err, double* mean_out, double* err_out);

/* Bootstrap resampling of expectations, _resample_expectations_with_beta (tomography.py:378-409), for
 * all resamples at once: out[r][i] = 2 Beta(n_plus_i + prior, n_minus_i + prior) - 1 with
 * n_plus = (expect_i + 1) / 2 * counts_i, i < n (= batch * settings, flattened), r < R.  The reference
 * draws from numpy's global stream; here element (r, i) owns a counter-based Philox4x32-10 stream
 * keyed by `seed` (counter = (r * n + i, draw number)), so results are reproducible and independent
 * of R and of the launch shape; parity with the reference is distributional.  Elements whose Beta
 * parameters are not positive come out as NaN.  The _dev form optionally also writes
 * d_counts_out[r][i] = counts[i] so that the R * batch resampled experiments can be handed to a
 * batched estimator as one launch. */
int fbx_beta_resample(int64_t n, int64_t R, const double* expect, const double* counts,
                      double prior_counts, uint64_t seed, double* out);
int fbx_beta_resample_dev(int64_t n, int64_t R, const double* d_expect, const double* d_counts,
                          double prior_counts, uint64_t seed, double* d_out, double* d_counts_out);

/* ---------------------------------------------------------------- quantum volume (quantum_volume.py)
 * collect_heavy_outputs (quantum_volume.py:94-123) for B model circuits of one width: the ideal output distribution of each
 * circuit from a state-vector simulation in LDS, its median and its heavy outputs.  A circuit is a flat list of L two-qubit gates:
 * pairs [B][L][2] qubit indices (q0, q1), q0 != q1, both < n_qubits; gates [B][L][4][4] complex128, applied in order l = 0 .. L-1.
 * The state starts as |0...0>; amplitude index i has qubit 0 as its MOST significant bit (:115), and of the 4 x 4 matrix index q0
 * is the more significant bit: for every assignment of the other qubits the amplitudes at (bit of q0, bit of q1) = 00, 01, 10, 11
 * are replaced by U times that 4-vector.  probs_out [B][2^n] = |amp|^2; median_out [B] = half the sum of the two middle order
 * statistics (statistics.median, :118; exact order statistics, no tolerance); output i is heavy iff probs[i] > median, strictly
 * (:121) -- ties are not heavy; heavy_mask_out [B][W], W = max(1, 2^n / 64), bit i % 64 of word i / 64; heavy_prob_out [B] = sum of
 * the heavy probabilities; heavy_count_out [B] = number of heavy outputs.  Every output may be NULL, not all of them.
 * n_qubits 2..13 (the state lives in the LDS of one CU; others FBX_ERR_UNSUPPORTED).  L = 0: probs (1, 0, ...), median 0, heavy {0}.
 * The host-pointer form checks every pair (FBX_ERR_BAD_ARG); the _dev form cannot, and turns a circuit with a bad pair into a
 * poisoned item.  A poisoned item (bad pair, non-finite gate entry) gets NaN probabilities, median and heavy probability and an
 * empty heavy set; its neighbours are untouched.  Results do not depend on the batch.  The _dev form enqueues on the calling
 * thread's stream and does not synchronise. */
int fbx_qv_heavy_outputs(int n_qubits, int64_t B, int L, const uint8_t* pairs, const double* gates, double* probs_out,
                         double* median_out, uint64_t* heavy_mask_out, double* heavy_prob_out, int32_t* heavy_count_out);
int fbx_qv_heavy_outputs_dev(int n_qubits, int64_t B, int L, const uint8_t* d_pairs, const double* d_gates, double* d_probs_out,
                             double* d_median_out, uint64_t* d_heavy_mask_out, double* d_heavy_prob_out,
                             int32_t* d_heavy_count_out);

/* count_heavy_hitters_sampled (quantum_volume.py:322-341) for B circuits: bits [B][n_shots][n_qubits] 0/1 bytes as qc.run returns
 * them; every shot row becomes an integer by bit_array_to_int (utils.py:32-42: first column most significant) and is looked up in
 * the circuit's heavy_mask [B][W] (fbx_qv_heavy_outputs); counts_out [B].  Only bit 0 of every byte is read.  n_qubits 2..13. */
int fbx_qv_count_heavy(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* bits, const uint64_t* heavy_mask,
                       int64_t* counts_out);
int fbx_qv_count_heavy_dev(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* d_bits, const uint64_t* d_heavy_mask,
                           int64_t* d_counts_out);

/* The same two computations for n_qubits 14..26 (others FBX_ERR_UNSUPPORTED; widths up to 13 belong to the functions above): the
 * state of a circuit is 16 B x 2^n in device memory and is worked on in LDS a tile of 2^tile_bits amplitudes at a time
 * (csrc/fbx_qvolume_wide.hip).  Layouts, conventions, the exact median, the tie rule and the poisoned-item rule are
 * those of fbx_qv_heavy_outputs; W = 2^n / 64.  tile_bits: 0 = the library's default (13), else 8..13 (FBX_ERR_BAD_ARG otherwise).
 * No result depends on tile_bits, on B or on how the batch was cut into chunks; the probabilities are bitwise the same for every
 * tile_bits.  heavy_prob_out is summed in one fixed order: blocks of 4096 outputs, the blocks in order.  The batch runs in chunks of
 * as many circuits as fbx_set_option "qv_wide_workspace_mib" (default 128, range [1, 65536]; at least one circuit) admits at
 * 16 B x 2^n per circuit, plus 8 B x 2^n when probs_out is NULL.  The _dev form enqueues on the calling thread's stream and does
 * not synchronise (growing the workspace does, as everywhere). */
int fbx_qv_heavy_outputs_wide(int n_qubits, int64_t B, int L, const uint8_t* pairs, const double* gates, int tile_bits,
                              double* probs_out, double* median_out, uint64_t* heavy_mask_out, double* heavy_prob_out,
                              int32_t* heavy_count_out);
int fbx_qv_heavy_outputs_wide_dev(int n_qubits, int64_t B, int L, const uint8_t* d_pairs, const double* d_gates, int tile_bits,
                                  double* d_probs_out, double* d_median_out, uint64_t* d_heavy_mask_out, double* d_heavy_prob_out,
                                  int32_t* d_heavy_count_out);
int fbx_qv_count_heavy_wide(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* bits, const uint64_t* heavy_mask,
                            int64_t* counts_out);
int fbx_qv_count_heavy_wide_dev(int n_qubits, int64_t B, int64_t n_shots, const uint8_t* d_bits, const uint64_t* d_heavy_mask,
                                int64_t* d_counts_out);
/* What the planner of fbx_qv_heavy_outputs_wide decided (host pointers; the planner itself runs on the device): circuit b runs
 * n_passes_out[b] passes; pass k applies the gates pass_first_gate_out[b][k] .. pass_first_gate_out[b][k + 1] - 1 with the index bits
 * of pass_local_mask_out[b][k] local (bit p of the mask = index bit p = qubit n - 1 - p; exactly tile_bits bits, always bits 0..2).
 * Entries past the last pass: first gate L, mask 0.  Bad pairs: FBX_ERR_BAD_ARG. */
int fbx_qv_wide_plan(int n_qubits, int64_t B, int L, const uint8_t* pairs, int tile_bits, int32_t* n_passes_out /* [B] */,
                     int32_t* pass_first_gate_out /* [B][L + 1] */, uint32_t* pass_local_mask_out /* [B][L] */);

/* Quantum-volume circuits under gate noise: T stochastic Pauli-error trajectories of each of B circuits of one width
 * (csrc/fbx_qvolume_noisy.hip).  pairs [B][L][2], gates [B][L][4][4] complex128, the bit order (qubit 0 = most
 * significant) and W = max(1, 2^n / 64) are those of fbx_qv_heavy_outputs; heavy_mask [B][W] or NULL is that function's
 * heavy_mask_out for the IDEAL circuits.  gate_error [B][L]: the error probability of every gate.
 *
 * THE MODEL.  After gate l of circuit b, in trajectory t, an error happens with probability gate_error[b][l]: one of the 15
 * non-identity two-qubit Paulis on that gate's pair (q0, q1), chosen uniformly.  Pauli index k = 4 a + c in 1..15, a on q0 and c on
 * q1, 0 = I, 1 = X, 2 = Y, 3 = Z.  Averaged over trajectories this is the channel rho -> (1 - 16 p / 15) rho + (16 p / 15) I/4 on
 * the pair.  Only probabilities leave the kernel, so Y is applied as X Z (a global phase).
 *
 * THE STREAM (part of the contract: it is what a host check restates; the conventions are those of fbx_sample_bitstrings).
 * Trajectory t of the circuit with the global id g = first_item + b owns the Philox4x32-10 blocks with counter (g low, g high, t, j)
 * and key (seed low ^ 0x51564745, seed high).  Block j serves gates 2 j and 2 j + 1: words (x0, x1) for gate 2 j, (x2, x3) for gate
 * 2 j + 1.  A gate errs iff (double) x_first * 2^-32 < gate_error; if it errs, k = 1 + (uint32)(((uint64) x_second * 15) >> 32).
 * A trajectory depends on (seed, g, t) and its circuit's inputs only: not on B, T, the launch shape or the workgroup that ran it.
 *
 * Outputs, each may be NULL, not all of the first three.  probs_mean_out [B][2^n]: the mean over the T trajectories of the output
 * distribution, summed in an order that depends on T alone (partial sums over 4 consecutive trajectories in the order of t, the
 * partial sums in order, one division by T; no floating-point atomics), so an item repeats bit for bit under another B, another
 * first_item offset, another launch shape or another "qv_noisy_workspace_mib" (fbx_set_option; default 128, range [1, 65536]: the
 * batch runs in chunks of as many circuits as that many MiB of partial sums admit, at least one).  hprob_traj_out [B][T]: the
 * weight trajectory t puts on the heavy set of heavy_mask (required for it), summed in one fixed order.  n_errors_out [B][T]: the
 * number of Paulis inserted.  status_out [B]: 0 for a good item, 1 for a poisoned one.
 *
 * n_qubits 2..13 (others FBX_ERR_UNSUPPORTED, before any buffer is touched; a wider trajectory is an ordinary circuit for
 * fbx_qv_heavy_outputs_wide once its Paulis are multiplied into its gates).  B == 0 or T == 0: nothing is done.  T >= 2^32, a
 * negative size, first_item < 0, NULL pairs / gates / gate_error, hprob_traj_out without heavy_mask, no result asked for:
 * FBX_ERR_BAD_ARG.  A poisoned item -- a non-finite gate entry, a pair that is not two different qubits below n_qubits (neither
 * form checks pairs on the host), a gate_error outside [0, 1] or NaN -- gets status 1, NaN in probs_mean_out and hprob_traj_out
 * and 0 in n_errors_out; its neighbours are untouched and the kernel never indexes outside the state.
 * The _dev form enqueues on the calling thread's stream and does not synchronise (growing the workspace does, as everywhere). */
int fbx_qv_noisy_trajectories(int n_qubits, int64_t B, int L, int64_t T, const uint8_t* pairs, const double* gates,
                              const double* gate_error, const uint64_t* heavy_mask, uint64_t seed, int64_t first_item,
                              double* probs_mean_out, double* hprob_traj_out, int32_t* n_errors_out, int32_t* status_out);
int fbx_qv_noisy_trajectories_dev(int n_qubits, int64_t B, int L, int64_t T, const uint8_t* d_pairs, const double* d_gates,
                                  const double* d_gate_error, const uint64_t* d_heavy_mask, uint64_t seed, int64_t first_item,
                                  double* d_probs_mean_out, double* d_hprob_traj_out, int32_t* d_n_errors_out,
                                  int32_t* d_status_out);

/* ---------------------------------------------------------------- measured bitstrings from outcome distributions
 * The step between a distribution and a bit record (what a QVM's run-and-measure does for the reference): B items of one width,
 * n_shots shots each.  probs [B][2^n] outcome weights, non-negative and finite, not necessarily normalised; outcome index i has
 * qubit 0 as its MOST significant bit (as fbx_qv_heavy_outputs).  depolarizing [B] or NULL (= 0): with T = sum_i p_i and lambda
 * the item's value the sampled weights are w_i = p_i for lambda == 0, else (1 - lambda) p_i + lambda T / 2^n.  readout_flip
 * [B][n][2] or NULL (= no flips): [j][0] = P(read 1 | drawn 0), [j][1] = P(read 0 | drawn 1) of column j, applied independently
 * per bit after the draw.  bits_out [B][n_shots][n] uint8 0 / 1, first column = qubit 0: the records fbx_shots_to_moments,
 * fbx_qv_count_heavy and fbx_bit_histogram read.  status_out [B] or NULL: 0 for a good item, 1 for a poisoned one.
 *
 * n_qubits 1..13 (the table of prefix sums lives in the LDS of one CU; others FBX_ERR_UNSUPPORTED, before any buffer is touched).
 * B == 0 or n_shots == 0: nothing is done.  n_shots >= 2^32, a negative size, first_item < 0, NULL probs / bits_out: FBX_ERR_BAD_ARG.
 *
 * A poisoned item -- a weight that is negative or not finite, T not positive and finite, lambda outside [0, 1] or NaN, a flip
 * probability outside [0, 1] or NaN -- gets status 1 and a record of zeros; its neighbours are untouched.
 *
 * THE STREAM (part of the contract: it is what a host check restates).  Shot s of the item with the global id g = first_item + b
 * owns the Philox4x32-10 blocks with counter (g low, g high, s, t) and key (seed low, seed high), t = 0..3 for widths up to 13, up
 * to 6 for the wide form (fbx_sample_bitstrings_wide below); their words, in order, are x_0 .. x_15 (x_0 .. x_27 for the wide form;
 * only the blocks that are needed are computed).  The draw is u = k * 2^-53, k = ((x_0 >> 5) << 26) |
 * (x_1 >> 6): exact, in [0, 1).  With C the inclusive prefix sums of w, the outcome is the smallest i with C_i > u * C_{N-1}; if
 * rounding leaves none, the last i with w_i > 0.  C is non-decreasing in i and repeats its predecessor exactly where w_i == 0 (the
 * order in which it is summed is otherwise not specified), so an outcome of weight zero is never produced.  Column j, whose
 * drawn bit is d, flips iff (double) x_{2 + j} * 2^-32 < readout_flip[j][d].  A record depends on (seed, g, s) and its item's
 * inputs only: not on B, n_shots, the launch shape or the workgroup that drew it -- a call of B' items from first_item + k repeats
 * items k .. k + B' - 1, and a call of fewer shots repeats the first shots.
 * The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_sample_bitstrings(int n_qubits, int64_t B, int64_t n_shots, const double* probs, const double* depolarizing,
                          const double* readout_flip, uint64_t seed, int64_t first_item, uint8_t* bits_out, int32_t* status_out);
int fbx_sample_bitstrings_dev(int n_qubits, int64_t B, int64_t n_shots, const double* d_probs, const double* d_depolarizing,
                              const double* d_readout_flip, uint64_t seed, int64_t first_item, uint8_t* d_bits_out,
                              int32_t* d_status_out);

/* The same sampler for n_qubits 14..26 (others FBX_ERR_UNSUPPORTED, before any buffer is touched; widths up to 13 belong to the
 * functions above): the table of prefix sums of an item is 8 B x 2^n in device memory (csrc/fbx_sample_wide.hip).
 * Layouts, the meaning of probs, depolarizing, readout_flip, bits_out and status_out, the argument errors, the poisoned-item rule
 * and THE STREAM are those of fbx_sample_bitstrings, with t = 0..6: column j reads x_{2 + j}, j = 0 .. n - 1, of the words
 * x_0 .. x_27.  C is summed in one fixed order per width (blocks of 4096 entries, the block offsets chained in order), is
 * non-decreasing and repeats its predecessor bit for bit where w_i == 0.  The batch runs in chunks of as many items as
 * fbx_set_option "sample_wide_workspace_mib" (default 128, range [1, 65536]; at least one item) admits at 8 B x 2^n (+ 32 B per
 * 4096 entries + 456 B) per item.  A record depends on (seed, g, s) and its item's inputs only: not on B, n_shots, the cut into shot
 * ranges, the chunks or the option.  The _dev form enqueues on the calling thread's stream and does not synchronise (growing the
 * workspace does, as everywhere). */
int fbx_sample_bitstrings_wide(int n_qubits, int64_t B, int64_t n_shots, const double* probs, const double* depolarizing,
                               const double* readout_flip, uint64_t seed, int64_t first_item, uint8_t* bits_out,
                               int32_t* status_out);
int fbx_sample_bitstrings_wide_dev(int n_qubits, int64_t B, int64_t n_shots, const double* d_probs, const double* d_depolarizing,
                                   const double* d_readout_flip, uint64_t seed, int64_t first_item, uint8_t* d_bits_out,
                                   int32_t* d_status_out);

/* ---------------------------------------------------------------- simulated tomography experiments: truth to noisy expectations
 * The acquisition half of a tomography experiment (what do_tomography / estimate_observables, observable_estimation.py:856-920,
 * get from a QVM): B true channels or states measured with the settings of `design`, n_shots shots per setting, as the
 * (expectations, total_counts) every estimator here reads.
 *
 * truth: for a process design (1..3 qubits) the Pauli transfer matrices [B][D][D], real, row-major, in the reference's
 * pauli-liouville convention and Pauli order (what fbx_convert(..., FBX_REP_PAULI_LIOUVILLE) writes); for a state design (1..5
 * qubits) the density matrices [B][d][d] complex128 (interleaved re, im), as the other state entry points take them.
 * readout_flip [B][n][2] or NULL (= no flips), with the meaning of fbx_sample_bitstrings: [j][0] = P(read 1 | drawn 0), [j][1] =
 * P(read 0 | drawn 1) of qubit j, independent per bit.
 *
 * Outputs: expect_out, counts_out, std_err_out, exact_out [B][m] in the CALLER's setting order (the order of
 * fbx_design_create), status_out [B].  Each may be NULL, not all of them.  n_shots == 0 is the exact-expectations-only mode: it
 * is allowed only when expect_out, counts_out and std_err_out are NULL.
 *
 * THE MEAN.  Setting k of item b has the input state s_k, the Pauli P_k, the coefficient c_k and the set S of qubits on which
 * P_k is not the identity.  Without flips mu = tr[P_k Lambda_b(rho_{s_k})] (process) or tr[P_k rho_b] (state).  With flips, a_j =
 * f1_j - f0_j and b_j = 1 - f0_j - f1_j (f0 = [j][0], f1 = [j][1]), the mean of the MEASURED +-1 product is
 *     mu = sum_{T subset of S} prod_{j in S \ T} a_j prod_{j in T} b_j tr[P_T .],
 * P_T = P_k with the factors outside T replaced by I and the term of the empty T equal to 1: exact for independent per-bit flips
 * (E[z' | z] = a + b z), at most 2^w terms for a Pauli of weight w <= 5.  An all-identity observable has mu = 1 and uses no
 * draws.  exact_out = c_k mu.
 *
 * THE STREAM (part of the contract: it is what a host check restates).  q = 0.5 mu + 0.5 clamped to [0, 1] (an unphysical truth
 * is clamped, not refused); t = floor(q 2^32), a 64-bit integer in [0, 2^32].  Shot s of setting k (the caller's index) of the
 * global item g = first_item + b reads word s & 3 of the Philox4x32-10 block with counter (g low, g high, k, s >> 2) and key
 * (seed low ^ 0x544F4D4F, seed high); the tag keeps a caller who reuses a seed away from the stream of fbx_sample_bitstrings.
 * The shot counts +1 iff word < t; k_plus = the number of such shots, k_minus = N - k_plus (N = n_shots), and
 *     expect_out  = c_k * ((double) (k_plus - k_minus) / (double) N)
 *     counts_out  = N
 *     std_err_out = |c_k| * sqrt((double) (4 k_plus k_minus) / N) / N
 * (the reference's sqrt(np.var(vals) / N), observable_estimation.py:849-851, written so that nothing cancels).  A value depends
 * on (seed, g, k), mu and N only: not on B, the launch shape or which lanes counted which shots -- a call of B' items from
 * first_item + i repeats items i .. i + B' - 1.
 *
 * n_shots >= 2^32, a negative size, first_item < 0, NULL truth, every output NULL, n_shots == 0 with a sampled output requested:
 * FBX_ERR_BAD_ARG before any buffer is touched; a NULL design or one of another device likewise.  B == 0: nothing is done.
 * A poisoned item -- a non-finite truth entry, a flip probability outside [0, 1] or NaN -- gets status 1, NaN in expect_out /
 * std_err_out / exact_out and N in counts_out; its neighbours are untouched.
 * The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_tomo_simulate(const fbx_design* design, int64_t B, const double* truth, int64_t n_shots, const double* readout_flip,
                      uint64_t seed, int64_t first_item, double* expect_out, double* counts_out, double* std_err_out,
                      double* exact_out, int32_t* status_out);
int fbx_tomo_simulate_dev(const fbx_design* design, int64_t B, const double* d_truth, int64_t n_shots, const double* d_readout_flip,
                          uint64_t seed, int64_t first_item, double* d_expect_out, double* d_counts_out, double* d_std_err_out,
                          double* d_exact_out, int32_t* d_status_out);

/* ---------------------------------------------------------------- simulated tomography with grouped settings: one set of shots per basis
 * What do_tomography(..., group_tpb_settings=True) acquires (observable_estimation.py:470-692, group_settings): settings that are
 * diagonal in one tensor-product basis form a group and are estimated from the SAME bitstrings, so that within a group the
 * results carry the correlations of real data -- in every shot the ZZ result is the product of the IZ and ZI results.
 *
 * fbx_grouping_create: group_of [m] gives the group id, in [0, n_groups), of every setting of `design` (the caller's order).
 * FBX_ERR_BAD_ARG with a message for an id out of range, a group without a member, members of one group with different
 * in_labels rows, or members whose Paulis differ on a qubit where both are not the identity.  The grouping holds per group the
 * input state, the BASIS -- per qubit the one non-identity Pauli its members use there and Z where no member uses the qubit, so
 * that every group measures all n qubits and the outcome space is always 2^n <= 32 -- and the members sorted by group, each
 * with its parity mask (bit t set where base-4 digit t of its Pauli index is not the identity).  It belongs to `design` (which
 * must outlive it) and to the device it was created on.
 *
 * fbx_tomo_simulate_grouped: truth, readout_flip, n_shots, seed, first_item, the limits (1..3 qubit process designs, 1..5
 * qubit state designs, n_shots < 2^32) and expect_out / counts_out / std_err_out / exact_out [B][m] / status_out [B] are those of
 * fbx_tomo_simulate; prob_out [B][G][2^n] double and hist_out [B][G][2^n] uint32 are per group.  Every output may be NULL, not
 * all of them.  n_shots == 0 gives exact_out and prob_out only (the others must be NULL).  A unit is (item b, group g):
 *  1. CLEAN MEANS.  For every subset T of the n qubits t_T = tr[P_T Lambda_b(rho_s)] (state designs: tr[P_T rho_b]), t of the
 *     empty set = 1; P_T is the group's basis with the factors outside T replaced by I.
 *  2. DISTRIBUTION.  p(o) = 2^-n sum_T (-1)^{|o & T|} t_T.  Bit t of an outcome belongs to the qubit of base-4 digit t of a
 *     Pauli index (qubit n - 1 - t); bit value 1 = eigenvalue -1.  Then, per qubit j, the confusion matrix of readout_flip:
 *     p'(bit = 0) = (1 - f0_j) p(bit = 0) + f1_j p(bit = 1), p'(bit = 1) = f0_j p(bit = 0) + (1 - f1_j) p(bit = 1).  prob_out
 *     receives this p, unclamped, flips included.
 *  3. THRESHOLDS.  c_o = the running sum of max(p(o'), 0) in outcome order, one addition per outcome (numpy.cumsum restates
 *     it bit for bit); thr_o = floor(c_o / c_last 2^32) for every outcome but the last, which gets 2^32.  If c_last is not a
 *     positive finite number the ITEM is poisoned.
 *  4. SHOTS.  Shot s reads word s & 3 of the Philox4x32-10 block with counter (gid low, gid high, g, s >> 2) and key (seed low ^
 *     0x544F4D47, seed high), gid = first_item + b; the tag "TOMG" keeps the stream apart from that of fbx_tomo_simulate under
 *     the same seed.  The outcome of a word is the number of thresholds <= the word; hist_out[o] counts the outcomes.
 *  5. MEMBERS.  For member k with parity mask z_k, k_plus = sum_o hist[o] [popcount(o & z_k) even], k_minus = N - k_plus, and
 *     expect_out / counts_out / std_err_out follow the integer formulas of fbx_tomo_simulate, written at the caller's setting
 *     index.  An all-identity observable gives its coefficient and std_err 0.
 *  6. EXACT MEANS.  exact_out[k] is the very value fbx_tomo_simulate writes for setting k (the same code), bit for bit.
 * A value depends on (seed, gid, g, p, n_shots) only: not on B or the launch shape.
 * A poisoned item -- a non-finite truth entry, a flip probability outside [0, 1] or NaN, or a group whose c_last is not a
 * positive finite number -- gets status 1, NaN in expect_out / std_err_out / exact_out / prob_out, N in counts_out and 0 in
 * hist_out, for ALL its groups; its neighbours are untouched.  Bad arguments (those of fbx_tomo_simulate, a NULL grouping or
 * one of another design or device): FBX_ERR_BAD_ARG before any buffer is touched.  B == 0: nothing is done.
 * The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_grouping_create(const fbx_design* design, int n_groups, const int32_t* group_of, fbx_grouping** out);
int fbx_grouping_destroy(fbx_grouping* grouping);
int fbx_tomo_simulate_grouped(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* truth,
                              int64_t n_shots, const double* readout_flip, uint64_t seed, int64_t first_item, double* expect_out,
                              double* counts_out, double* std_err_out, double* exact_out, double* prob_out, uint32_t* hist_out,
                              int32_t* status_out);
int fbx_tomo_simulate_grouped_dev(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* d_truth,
                                  int64_t n_shots, const double* d_readout_flip, uint64_t seed, int64_t first_item,
                                  double* d_expect_out, double* d_counts_out, double* d_std_err_out, double* d_exact_out,
                                  double* d_prob_out, uint32_t* d_hist_out, int32_t* d_status_out);

/* ---------------------------------------------------------------- symmetrized readout and calibration under a joint confusion matrix
 * The two defaults of the reference's do_tomography that the calls above do not model: symm_type = -1 (every group is measured
 * under exhaustive readout symmetrization: every combination of pre-measurement bit flips, undone in the record) and
 * calibrate_observables = True (every distinct observable is measured on its +1 eigenstate with the same symmetrization, and
 * every expectation is divided by that calibration: fbx_calibrate_expectations).  The readout error is a JOINT confusion matrix,
 * so correlated (crosstalk) errors are covered; fbx/readout.py estimates such matrices from shots.
 *
 * design, grouping, truth, seed, first_item, the limits on the designs and the outputs expect_out / counts_out / std_err_out /
 * exact_out [B][m], hist_out [B][G][2^n] uint32 and status_out [B] are those of fbx_tomo_simulate_grouped.  confusion [B][2^n][2^n]
 * doubles, [drawn][read], rows summing to 1; bit t of an index is qubit n - 1 - t (the outcome convention of
 * fbx_tomo_simulate_grouped, so that index = the bitstring read as a binary number, qubit 0 first).  prob_out
 * [B][G][2^n][2^n]: row f of a unit is the distribution of pattern f (below).  Every output may be NULL, not all of them;
 * n_shots == 0 gives exact_out and prob_out only.  A unit is (item b, group g); U_g = the union of the parity masks of the
 * group's members, w = popcount(U_g):
 *  1. PATTERNS.  symm_type = -1: the 2^w flip masks f that are subsets of U_g; symm_type = 0: f = 0 alone (the plain correlated
 *     readout error, without symmetrization).  Qubits outside U_g are never flipped; they are still drawn and still pass through
 *     the matrix (their state matters to crosstalk), and their read bits are ignored by the parities.  symm_type 1, 2, 3 (the
 *     reference's orthogonal arrays): FBX_ERR_UNSUPPORTED.
 *  2. SHOTS PER PATTERN.  s = floor(n_shots / patterns) for the unit, n_shots being the total of a group; the shots a member
 *     is estimated from are N = s x patterns <= n_shots, which counts_out reports -- it CAN DIFFER between the groups of one
 *     call.  (The floor is this library's rule: pyquil's run_symmetrized_readout, which the reference calls, was not at hand to
 *     compare against.)  A call in which s would be 0 or >= 2^29 for any group is refused.
 *  3. DISTRIBUTIONS.  p = the ideal outcome distribution of the group (steps 1-2 of fbx_tomo_simulate_grouped without flips,
 *     the same code).  The un-flipped record of pattern f has q_f(r) = sum_o p(o) C[o ^ f][r ^ f], summed in ascending o with one
 *     fused multiply-add per term from 0.  prob_out[f] = q_f, unclamped; a zero row for a mask that is not a pattern.
 *  4. THE STREAM, per pattern, as step 3-4 of fbx_tomo_simulate_grouped: c_r = the running sum of max(q_f(r'), 0) in outcome
 *     order, thr_r = floor(c_r / c_last 2^32) for every outcome but the last; shot t (0 <= t < s) of pattern f reads word t & 3 of
 *     the Philox4x32-10 block with counter (gid low, gid high, g, (f << 27) | (t >> 2)) -- f the n-bit mask itself -- and key
 *     (seed low ^ 0x544F4D53, seed high), gid = first_item + b; the tag "TOMS" keeps the stream apart from the others under one
 *     seed.  The outcome of a word is the number of thresholds <= the word.  hist_out = the integer sum of the patterns'
 *     histograms (of the un-flipped record).
 *  5. MEMBERS.  k_plus, k_minus and the integer formulas of fbx_tomo_simulate_grouped on the merged histogram with N = s x
 *     patterns.
 *  6. EXACT MEANS.  exact_out[k] = c_k sum_r (-1)^{|r & z_k|} qbar(r), r ascending, qbar(r) = (the sum of q_f(r) over the patterns
 *     in ascending f) / patterns: the mean of what is measured, matrix included (not the value fbx_tomo_simulate writes).
 * A value depends on (seed, gid, g, f, t), the distributions and s only: not on B or on how lanes share the work.
 * A poisoned item -- a non-finite truth entry, a confusion entry that is not finite or outside [0, 1], or a pattern whose c_last
 * is not a positive finite number -- gets status 1, NaN in expect_out / std_err_out / exact_out / prob_out (all 2^n rows), N in
 * counts_out and 0 in hist_out, for all its groups; its neighbours are untouched.  Rows are NOT required to sum to 1 here: the
 * thresholds normalise by c_last (the Python layer refuses rows that do not).
 * Refusals, before any buffer is touched: the bad arguments of fbx_tomo_simulate_grouped, NULL confusion, symm_type outside
 * [-1, 3], s == 0 or s >= 2^29 for a group (FBX_ERR_BAD_ARG); symm_type 1..3 (FBX_ERR_UNSUPPORTED).  B == 0: nothing is done.
 *
 * fbx_tomo_calibration_list: the calibrations of a design are its distinct non-identity Pauli indices (base-4 digits, qubit 0
 * most significant) in order of first appearance in the caller's setting order.  n_cal_out receives their number, cal_pauli_out
 * (room for m, may be NULL) the indices, cal_index_out [m] (may be NULL) the calibration of every setting, -1 for an
 * all-identity observable.  The list is made on the first call that needs it (this one or fbx_tomo_simulate_calibration[_dev])
 * and kept on the design: that first call uploads the masks with one blocking copy.
 *
 * fbx_tomo_simulate_calibration: a unit is (item b, calibration c) with the parity mask z_c of its Pauli.  The drawn outcome is
 * all zeros -- the +1 eigenstate on the support and |0> elsewhere, as get_calibration_program prepares it -- so p = (1, 0, ...)
 * and q_f(r) = C[f][r ^ f]; the patterns are the subsets of z_c (f = 0 alone for symm_type = 0); s = floor(cal_shots / patterns)
 * with the refusals above; the stream is that of step 4 with counter (gid low, gid high, c, (f << 27) | (t >> 2)) and key (seed low
 * ^ 0x544F4D43, seed high) ("TOMC").  Outputs [B][n_cal], each may be NULL, not all: cal_mean_out = (k_plus - k_minus) / N,
 * cal_var_out = (double) (4 k_plus k_minus) / N / N / N (the reference's var / N of the +-1 values), cal_exact_out as step 6 with
 * coefficient 1, cal_counts_out = N; cal_shots == 0 gives cal_exact_out only.  Poison as above (there is no truth): NaN in the
 * mean, the variance and the exact value, N in the counts.
 * The _dev forms enqueue on the calling thread's stream and do not synchronise. */
int fbx_tomo_simulate_symmetrized(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* truth,
                                  const double* confusion, int symm_type, int64_t n_shots, uint64_t seed, int64_t first_item,
                                  double* expect_out, double* counts_out, double* std_err_out, double* exact_out, double* prob_out,
                                  uint32_t* hist_out, int32_t* status_out);
int fbx_tomo_simulate_symmetrized_dev(const fbx_design* design, const fbx_grouping* grouping, int64_t B, const double* d_truth,
                                      const double* d_confusion, int symm_type, int64_t n_shots, uint64_t seed, int64_t first_item,
                                      double* d_expect_out, double* d_counts_out, double* d_std_err_out, double* d_exact_out,
                                      double* d_prob_out, uint32_t* d_hist_out, int32_t* d_status_out);
int fbx_tomo_calibration_list(const fbx_design* design, int32_t* n_cal_out, int32_t* cal_pauli_out, int32_t* cal_index_out);
int fbx_tomo_simulate_calibration(const fbx_design* design, int64_t B, const double* confusion, int symm_type, int64_t cal_shots,
                                  uint64_t seed, int64_t first_item, double* cal_mean_out, double* cal_var_out,
                                  double* cal_exact_out, double* cal_counts_out, int32_t* status_out);
int fbx_tomo_simulate_calibration_dev(const fbx_design* design, int64_t B, const double* d_confusion, int symm_type,
                                      int64_t cal_shots, uint64_t seed, int64_t first_item, double* d_cal_mean_out,
                                      double* d_cal_var_out, double* d_cal_exact_out, double* d_cal_counts_out,
                                      int32_t* d_status_out);

/* ---------------------------------------------------------------- curve fits (analysis/fitting.py, randomized_benchmarking.py,
 * qubit_spectroscopy.py)
 * fbx_curve_fit: B independent weighted non-linear least-squares fits, one per GPU lane, of the four models of
 * analysis/fitting.py:16-149 (what lmfit's Model.fit does for fit_base_param_decay, fit_decay_time_param_decay,
 * fit_decaying_cosine and fit_shifted_cosine, one data set at a time).  Parameter order is the reference's:
 *   FBX_FIT_BASE_DECAY       baseline + amplitude * decay**x                            (amplitude, decay, baseline)
 *   FBX_FIT_TIME_DECAY       amplitude * exp(-(x - offset) / decay_time)                (amplitude, decay_time, offset)
 *   FBX_FIT_DECAYING_COSINE  amplitude * exp(-x / decay_time) * cos(2 pi frequency x + offset) + baseline
 *                                                                       (amplitude, decay_time, offset, baseline, frequency)
 *   FBX_FIT_SHIFTED_COSINE   amplitude * cos(frequency x + offset) + baseline            (amplitude, offset, baseline, frequency)
 * x is [K] for the whole batch (x_stride = 0) or [B][K] (x_stride = K); y is [B][K]; weights is [B][K] or NULL; the residual is
 * (model - y) * weight, as in lmfit.  guess is [B][P].  Bit j of `vary` set: parameter j is fitted; cleared: it keeps its guess,
 * bit for bit.  K is 2..FBX_FIT_MAX_POINTS (more: FBX_ERR_UNSUPPORTED).
 * Method: Levenberg-Marquardt with analytic Jacobians in fp64 on the normal equations, columns scaled by the largest column norm
 * seen so far (MINPACK's diag); the damped P x P system is solved in registers.  A trial point at which the cost or a derivative
 * is not finite is a rejected step.  MINPACK's tests (relative actual and predicted reduction of the cost <= ftol; scaled step <=
 * xtol * scaled parameters) propose a stop; the item is declared converged once, in addition,
 *   grad_norm <= sqrt((n_free + 1) * max(ftol, xtol) * chisqr) + FBX_FIT_GRAD_FLOOR * ||weights * y||_2
 * holds at the new point (the first term follows from the ftol test when the step is a Gauss-Newton step; the second is the
 * rounding floor of a residual) -- every item with a CONVERGED status satisfies this bound.  max_iters counts trial points.
 * Outputs, each may be NULL: params[B][P]; covar[B][P][P] = inv(J^T J) * redchi at the returned point (lmfit's
 * scale_covar=True; rows and columns of fixed parameters zero; NaN when FBX_FIT_SINGULAR_COVAR is reported); chisqr[B];
 * redchi[B] = chisqr / max(1, K - n_free); iters[B]; grad_norm[B] = max over free j of |J_j^T r| / ||J_j|| at the returned point;
 * status[B] = one of FBX_FIT_CONVERGED_FTOL / _XTOL / FBX_FIT_MAX_ITERS / FBX_FIT_BAD_START, with FBX_FIT_SINGULAR_COVAR
 * OR-ed in when the unit-diagonal scaling of J^T J has a Cholesky pivot <= FBX_FIT_SINGULAR_PIVOT (some combination of the free
 * parameters does not move the model -- all three parameters of FBX_FIT_TIME_DECAY free is such a case; FBX_FIT_SINGULAR_COVAR is
 * only looked for when covar is asked for).  A non-finite x, y, weight or guess makes that item FBX_FIT_BAD_START with NaN results
 * and touches no other item.  Results do not depend on B or on an item's position in the batch. */
#define FBX_FIT_BASE_DECAY       0
#define FBX_FIT_TIME_DECAY       1
#define FBX_FIT_DECAYING_COSINE  2
#define FBX_FIT_SHIFTED_COSINE   3
#define FBX_FIT_MAX_POINTS       256
#define FBX_FIT_CONVERGED_FTOL   1
#define FBX_FIT_CONVERGED_XTOL   2
#define FBX_FIT_MAX_ITERS        3
#define FBX_FIT_BAD_START        4
#define FBX_FIT_SINGULAR_COVAR   16      /* flag, OR-ed onto one of the four above */
#define FBX_FIT_GRAD_FLOOR       9.094947017729282e-13   /* 4096 * 2^-52 */
#define FBX_FIT_SINGULAR_PIVOT   1e-11
int fbx_curve_fit(int model, int64_t B, int K, const double* x, int64_t x_stride, const double* y, const double* weights,
                  const double* guess, unsigned vary, double ftol, double xtol, int max_iters, double* params_out,
                  double* covar_out, double* chisqr_out, double* redchi_out, int32_t* iters_out, int32_t* status_out,
                  double* grad_norm_out);
int fbx_curve_fit_dev(int model, int64_t B, int K, const double* d_x, int64_t x_stride, const double* d_y, const double* d_weights,
                      const double* d_guess, unsigned vary, double ftol, double xtol, int max_iters, double* d_params_out,
                      double* d_covar_out, double* d_chisqr_out, double* d_redchi_out, int32_t* d_iters_out, int32_t* d_status_out,
                      double* d_grad_norm_out);

/* z_obs_stats_to_survival_statistics with covariances_of_all_iz_obs (randomized_benchmarking.py:308-383) for S sequences:
 * expectations / std_errs [S][dim - 1] of the non-trivial I/Z observables, dim a power of two in 2..32.  survival[S] =
 * (sum + 1) / dim; variance[S] = sum of squared standard errors / dim^2, plus, for dim > 2 and num_shots > 0, the summed pairwise
 * covariance (2 sum_i e_i - sum_{i != j} e_i e_j) / num_shots / dim^2.  num_shots = 0 is the reference's
 * obs_are_independent=True; for dim = 2 the term does not exist. */
int fbx_rb_survival(int dim, int64_t S, const double* expectations, const double* std_errs, int64_t num_shots,
                    double* survival_out, double* variance_out);
int fbx_rb_survival_dev(int dim, int64_t S, const double* d_expectations, const double* d_std_errs, int64_t num_shots,
                        double* d_survival_out, double* d_variance_out);

/* estimate_purity and estimate_purity_err (randomized_benchmarking.py:490-533) for S sequences: expectations / std_errs
 * [S][dim^2 - 1] of the non-identity Paulis (the identity term, expectation 1 and variance 0, is appended inside), dim a power
 * of two in 2..8.  purity[S] = sum e^2 / dim, shifted to (dim / (dim - 1)) (purity - 1 / dim) when renorm != 0; purity_err[S]
 * propagates v_i = (2 |e_i|)^2 var_i, replaced by var_i^2 where numpy.isclose(0, v_i, atol=1e-6) holds, as the reference does. */
int fbx_rb_purity(int dim, int64_t S, const double* expectations, const double* std_errs, int renorm, double* purity_out,
                  double* purity_err_out);
int fbx_rb_purity_dev(int dim, int64_t S, const double* d_expectations, const double* d_std_errs, int renorm,
                      double* d_purity_out, double* d_purity_err_out);

/* What fit_rb_results (:423-436) and fit_unitarity_results (:577-589) do between their statistics and the fit, for B items of
 * K values on the device: weights[B][K] = 1 / error with every error that is not above zero (zero, or the NaN of a negative variance)
 * replaced by the item's smallest one that is (error = sqrt(d_errors) when errors_are_variances != 0); an item without one gets unit weights and has_weights[b] = 0
 * (the reference passes weights=None, the same fit).  guess[B][3] = (y[0] - y[K-1], 0.95, y[K-1]) for FBX_FIT_PREPARE_RB and
 * (y[0], 0.95, 0) for FBX_FIT_PREPARE_UNITARITY.  d_errors may be NULL when neither weights nor has_weights is asked for.  With
 * it fbx_rb_survival_dev -> fbx_fit_prepare_dev -> fbx_curve_fit_dev never leaves the device. */
#define FBX_FIT_PREPARE_RB         0
#define FBX_FIT_PREPARE_UNITARITY  1
int fbx_fit_prepare_dev(int kind, int64_t B, int K, const double* d_values, const double* d_errors, int errors_are_variances,
                        double* d_weights_out, double* d_guess_out, int32_t* d_has_weights_out);

/* ---------------------------------------------------------------- robust phase estimation (robust_phase_estimation.py)
 * fbx_rpe_phase: estimate_phase_from_moments (robust_phase_estimation.py:361-404) for B estimates of K depths, one estimate per GPU
 * lane.  x, y, x_err, y_err are [B][K]: the expectations of X and Y after 2^j applications of the rotation, j = 0 .. K-1, and the
 * standard errors of those means (their variances when errors_are_variances != 0, as in fbx_fit_prepare_dev: what
 * fbx_shots_to_moments_dev writes goes in directly).  K is 1..62 (more: FBX_ERR_UNSUPPORTED; 2^j must stay an exact integer).
 * xz, yz, xz_err, yz_err ([B][K], all four or none) are the expectations of the same observables times a Z on a partner qubit: with
 * them the recursion runs on the post-selected combination of robust_phase_estimate (:496-504), x + xz for post_select = 0 and
 * x - xz for post_select = 1, with the two errors added in quadrature.
 * The recursion is the reference's, operation for operation in fp64 without fused multiply-adds (:377-404): at iteration j, k = 2^j,
 * r = sqrt(x^2 + y^2), r_std = sqrt(x_err^2 + y_err^2); r < r_std (strictly) ends the item; otherwise theta_j = atan2(y, x) / k is
 * moved into the window of width 2 pi / k around the running estimate with Python's float % (the result carries the divisor's
 * sign); the result is the estimate % 2 pi.  Where the reference's own assert (:399) would fire -- the offset rounded up to the
 * window's width -- the item keeps the computed value.
 * Outputs, each may be NULL, not all: phase[B] in [0, 2 pi); depth_reached[B] = the number of iterations used (K when the item was
 * never cut short; the reference's warning (:385) reports 2^depth_reached / 2); bloch[B][K][2] = (r, theta_est * k) per iteration,
 * the reference's bloch_data, NaN beyond the cut.  A non-finite moment among the iterations an item uses makes that item's phase and
 * all of its bloch rows NaN (depth_reached = the iteration at which it was met) and touches no other item.  Results do not depend
 * on B or on an item's position in the batch.  The _dev forms enqueue on the calling thread's stream and do not synchronise. */
int fbx_rpe_phase(int64_t B, int K, const double* x, const double* y, const double* x_err, const double* y_err,
                  int errors_are_variances, const double* xz, const double* yz, const double* xz_err, const double* yz_err,
                  int post_select, double* phase_out, int32_t* depth_reached_out, double* bloch_out);
int fbx_rpe_phase_dev(int64_t B, int K, const double* d_x, const double* d_y, const double* d_x_err, const double* d_y_err,
                      int errors_are_variances, const double* d_xz, const double* d_yz, const double* d_xz_err,
                      const double* d_yz_err, int post_select, double* d_phase_out, int32_t* d_depth_reached_out,
                      double* d_bloch_out);

/* The same estimate straight from measured bits, one wavefront per estimate: x_bits and y_bits are [B][K][n_shots][n_qubits] 0/1
 * bytes (the records of fbx_shots_to_moments; only bit 0 of a byte is read), col the column measured in X / Y, zcol a column
 * measured in Z or -1 for none (with it post_select chooses x + xz or x - xz as above).  n_qubits 1..8, n_shots >= 1 and the same
 * at every depth (depth-dependent shot counts: fbx_shots_to_moments_dev -> fbx_rpe_phase_dev).  Per record the shots with
 * b[col] = 1 and the shots with b[col] ^ b[zcol] = 1 are counted (exact integers); mean = (n_plus - n_minus) / n_shots and the
 * variance of the mean (1 - mean^2) / n_shots as fbx_shots_to_moments documents them (coefficient 1, no Beta prior), then the
 * recursion of fbx_rpe_phase.  Outputs as there, plus moments_out[B][K][4] = (x, y, x_err, y_err) as the recursion consumed them
 * (after post-selection, errors as standard errors).  Without moments_out the records of an item beyond its cut are not read. */
int fbx_rpe_from_shots(int n_qubits, int64_t B, int K, int64_t n_shots, const uint8_t* x_bits, const uint8_t* y_bits, int col,
                       int zcol, int post_select, double* phase_out, int32_t* depth_reached_out, double* bloch_out,
                       double* moments_out);
int fbx_rpe_from_shots_dev(int n_qubits, int64_t B, int K, int64_t n_shots, const uint8_t* d_x_bits, const uint8_t* d_y_bits,
                           int col, int zcol, int post_select, double* d_phase_out, int32_t* d_depth_reached_out,
                           double* d_bloch_out, double* d_moments_out);

/* Circular statistics of angles[R][B] over R (the layout fbx_beta_resample_dev -> fbx_rpe_phase_dev leaves bootstrap phases in):
 * mean[B] = atan2(mean sin, mean cos) mod 2 pi, std[B] = sqrt(-2 ln Rbar) with Rbar the length of the mean vector,
 * nan_count[B] = the number of NaN entries, which are skipped (an item with nothing left gets NaN).  One item per thread, entries in
 * order, compensated sums: repeated calls agree bit for bit.  Each output may be NULL, not all. */
int fbx_circular_stats(int64_t R, int64_t B, const double* angles, double* mean_out, double* std_out, int32_t* nan_count_out);
int fbx_circular_stats_dev(int64_t R, int64_t B, const double* d_angles, double* d_mean_out, double* d_std_out,
                           int32_t* d_nan_count_out);

/* ---------------------------------------------------------------- simulated robust phase estimation: noisy gates to shot counts
 * What generate_rpe_experiments + acquire_rpe_data (robust_phase_estimation.py:152-307) get from a QVM, for B experiments of K
 * depths at once.  The gate is a Pauli transfer matrix, so depth 2^j is j squarings and every depth the analysis accepts (K in
 * 1..62) can be simulated.  n_qubits is 1 or 2, D = 4^n_qubits; Pauli order and normalisation are those of fbx_rb_simulate: a
 * Pauli vector has component k = tr[P_k rho] (identity component 1), an index is read in base 4 with qubit 0 most significant
 * (I, X, Y, Z = 0, 1, 2, 3), and a matrix is row-major.
 *
 * Inputs.  gate_ptm [B][D][D].  prep_ptm and meas_ptm, the change of basis and its inverse, given separately so that each may
 * be noisy: [D][D] shared by the batch, or [B][D][D] when basis_per_item != 0; NULL = the identity.  init [D]: the Pauli vector
 * of the input state; NULL = |+> on every qubit.  xy_qubit: the qubit measured in X and in Y; z_qubit: a partner measured in Z, or
 * -1 for none.  flips [B][n_qubits][2] or NULL: [q][0] = P(read 1 | 0), [q][1] = P(read 0 | 1) of qubit q, independent per bit,
 * as in fbx_tomo_simulate.  n_shots [K]: the shots at depth 2^j, each >= 1; a HOST array in both forms (its K numbers travel
 * with the launch).  seed, first_item: as in fbx_tomo_simulate.
 *
 * Outputs, each may be NULL, not all.  M = 4 outcomes with a partner, 2 without; basis index 0 = X, 1 = Y.
 *   prob_out    [B][K][2][M] double     hist_out [B][K][2][M] uint32     status_out [B] int32
 *   moments_out [8][B][K] double: the planes x, y, xz, yz, var x, var y, var xz, var yz -- what fbx_rpe_phase_dev takes with
 *               errors_are_variances = 1; without a partner the four xz / yz planes are NaN
 *   x_bits_out, y_bits_out [B][K][S][n_qubits] bytes: the records fbx_rpe_from_shots reads with col = xy_qubit and zcol =
 *               z_qubit.  Only when every n_shots[j] equals one S; asked for with a ragged schedule: FBX_ERR_BAD_ARG.
 *
 * Per item b, depth j and basis P in {X, Y}:
 *  1. FINAL PAULI VECTOR.  v_j = meas G^(2^j) prep init, all in fp64: w = prep init once, G^(2^j) by squaring the matrix of
 *     depth j - 1, u = G^(2^j) w, v = meas u; a NULL factor is skipped.  Every row of every product is one chain of fused
 *     multiply-adds in ascending column order from 0.0.
 *  2. DISTRIBUTION.  The bits are (s, t): s belongs to xy_qubit, measured in P, t to z_qubit, measured in Z; bit value 1 =
 *     eigenvalue -1.  With v_I the identity component of v_j (1 for a trace-preserving map; a map that loses trace loses it
 *     here), outcome o = 2 s + t has
 *         p(s, t) = (v_I + (-1)^s <P_a> + (-1)^t <Z_b> + (-1)^(s+t) <P_a Z_b>) / 4,
 *     and without a partner outcome o = s has p(s) = (v_I + (-1)^s <P_a>) / 2; <.> are the components of v_j.  Then per
 *     measured bit the confusion matrix of its qubit's flips, exactly as step 2 of fbx_tomo_simulate_grouped.  prob_out
 *     receives this p, unclamped, flips included: it is what a host check restates the shots from.
 *  3. SHOTS.  c_o = the running sum of max(p(o'), 0) in outcome order; thr_o = floor(c_o / c_last 2^32) for every outcome but
 *     the last.  Shot s of N = n_shots[j] reads word s & 3 of the Philox4x32-10 block with counter (gid low, gid high, 2 j +
 *     basis, s >> 2) and key (seed low ^ 0x52504553, seed high), gid = first_item + b; the tag "RPES" keeps the stream apart
 *     from the tomography simulators' under one seed.  The outcome of a word is the number of thresholds <= the word; hist_out
 *     counts the outcomes.  X and XZ of a depth are read off the SAME shots, as the grouped settings of
 *     generate_rpe_experiments are: the post-selected sums x +- xz see that correlation.
 *  4. MOMENTS.  With n_minus the shots of odd parity -- s for x / y, s ^ t for xz / yz -- mean = ((N - n_minus) - n_minus) / N
 *     and the variance of the mean (1 - mean^2) / N, the formulas of fbx_rpe_from_shots, without fused multiply-adds.
 *  5. RECORDS.  Shot s of the record has column xy_qubit = s, column z_qubit = t and 0 in any other column.
 * A value depends on (seed, gid, j, basis), the item's inputs and n_shots[j] only: not on B, the item's position or the launch
 * shape (csrc/fbx_rpe_sim.hip has two work splits for the shots, chosen by B K alone).
 *
 * A poisoned item -- a non-finite entry of its gate, of init or of the prep / meas it uses, a flip outside [0, 1] or NaN, or a
 * distribution whose c_last is not a positive finite number (an all-zero matrix, a power that overflows) -- gets status 1, NaN in
 * prob_out and moments_out, 0 in hist_out and the records, at ALL its depths; its neighbours are untouched.
 * n_qubits >= 3 and K > 62: FBX_ERR_UNSUPPORTED.  n_qubits < 1, K < 1, a negative size, first_item < 0, NULL gate_ptm or
 * n_shots, an n_shots entry below 1, xy_qubit outside the gate, z_qubit neither -1 nor another qubit of the gate, every output
 * NULL, records with a ragged schedule: FBX_ERR_BAD_ARG before any buffer is touched.  B == 0: nothing is done.
 * The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_rpe_simulate(int n_qubits, int64_t B, int K, const double* gate_ptm, const double* prep_ptm, const double* meas_ptm,
                     int basis_per_item, const double* init, int xy_qubit, int z_qubit, const double* flips, const int32_t* n_shots,
                     uint64_t seed, int64_t first_item, double* prob_out, uint32_t* hist_out, double* moments_out,
                     uint8_t* x_bits_out, uint8_t* y_bits_out, int32_t* status_out);
int fbx_rpe_simulate_dev(int n_qubits, int64_t B, int K, const double* d_gate_ptm, const double* d_prep_ptm,
                         const double* d_meas_ptm, int basis_per_item, const double* d_init, int xy_qubit, int z_qubit,
                         const double* d_flips, const int32_t* n_shots, uint64_t seed, int64_t first_item, double* d_prob_out,
                         uint32_t* d_hist_out, double* d_moments_out, uint8_t* d_x_bits_out, uint8_t* d_y_bits_out,
                         int32_t* d_status_out);

/* ---------------------------------------------------------------- histograms of measured bitstrings
 * How often each bitstring, or each Hamming weight, occurred in every one of B records: the reduction under the joint readout
 * confusion matrices (readout.py:69-180, 236-335: row = the prepared string, one record per row), the ripple-carry adder's success
 * probabilities and error-weight distributions (classical_logic/ripple_carry_adder.py:317-384) and ghz_state_statistics
 * (entangled_states.py:36-51).  bits is [B][n_shots][n_cols] bytes, the records of fbx_shots_to_moments; only bit 0 of a byte is read.
 * cols selects k columns in any order (repeats allowed): [k] shared by the batch when cols_shared != 0, else [B][k]; NULL = columns
 * 0..k-1.  expected ([B][k] of 0 / 1, or NULL) is XORed onto the selected bits.
 *   FBX_HIST_JOINT   2^k bins, k in 1..10: bin = sum_i bit_i 2^(k-1-i), the first selected column most significant (the order of
 *                    itertools.product([0, 1], repeat=k) and of utils.bit_array_to_int)
 *   FBX_HIST_WEIGHT  k + 1 bins, k in 1..64: bin = the Hamming weight of the selected bits after the XOR (bin 0 = the shot matches
 *                    `expected` bit for bit)
 * counts_out[B][bins] are exact integers that sum to n_shots per record: they depend on nothing but the record, and two runs agree
 * bit for bit.  n_cols 1..64; n_shots 1..2^31 - 1 (32-bit counters on the chip).  The host form rejects a column index >= n_cols;
 * the _dev form cannot read the selection and instead fills the bins of a record whose selection has such an entry with -1, reading
 * nothing of that record.  One wavefront per record below 16 KB, one workgroup per longer record; a record is never split over
 * workgroups.  B == 0 returns FBX_OK.  The _dev forms enqueue on the calling thread's stream and do not synchronise. */
#define FBX_HIST_JOINT  0
#define FBX_HIST_WEIGHT 1
int fbx_bit_histogram(int n_cols, int64_t B, int64_t n_shots, const uint8_t* bits, int k, const uint8_t* cols, int cols_shared,
                      const uint8_t* expected, int kind, int64_t* counts_out);
int fbx_bit_histogram_dev(int n_cols, int64_t B, int64_t n_shots, const uint8_t* d_bits, int k, const uint8_t* d_cols, int cols_shared,
                          const uint8_t* d_expected, int kind, int64_t* d_counts_out);

/* out[i] = counts[i] / denom, one IEEE division per element on the device: the relative frequencies of a histogram (denom = n_shots;
 * the number of trials for the reset confusion matrices).  denom >= 1. */
int fbx_counts_to_frequencies(int64_t n, const int64_t* counts, int64_t denom, double* out);
int fbx_counts_to_frequencies_dev(int64_t n, const int64_t* d_counts, int64_t denom, double* d_out);

/* marginalize_confusion_matrix (readout.py:183-233) for a batch in[B][2^n][2^n] of float64 matrices, n = n_qubits in 1..10: keep[k]
 * lists the qubit positions that stay (position 0 = the most significant bit of a row / column index), strictly ascending, k in
 * 1..n; out[B][2^k][2^k], element = the sum of the 4^(n-k) inputs whose row and column bits agree with it on the kept positions,
 * divided by 2^(n-k).  The sum has one fixed order, so repeated calls agree bit for bit and an item does not depend on B.  keep is a
 * HOST pointer in both forms (a design argument, read and checked before any device work). */
int fbx_marginalize_confusion(int n_qubits, int64_t B, int k, const uint8_t* keep, const double* in, double* out);
int fbx_marginalize_confusion_dev(int n_qubits, int64_t B, int k, const uint8_t* keep, const double* d_in, double* d_out);

/* ---------------------------------------------------------------- random operators
 * operator_tools/random_operators.py:21-157 for batches, generated on the device.  Item b (global id
 * first_item + b) owns a counter-based Philox4x32-10 stream keyed by `seed`, so an item's matrices
 * depend on (seed, item id) only -- not on B, the launch shape or the split over GPUs.  The
 * reference draws from numpy's global Mersenne-Twister stream: parity is distributional (the
 * host generators of the Python shim keep the reference's draw order for seeded reproduction).
 *   FBX_RAND_GINIBRE        out[B][dim][cols]  ginibre_matrix_complex(dim, cols)           :21-46
 *   FBX_RAND_UNITARY        out[B][dim][dim]   haar_rand_unitary(dim)                      :49-72
 *   FBX_RAND_STATE_VECTOR   out[B][dim]        haar_rand_state(dim)                        :75-89
 *   FBX_RAND_GINIBRE_STATE  out[B][dim][dim]   ginibre_state_matrix(dim, rank)             :92-112
 *   FBX_RAND_BURES_STATE    out[B][dim][dim]   bures_measure_state_matrix(dim)             :115-132
 * dim in {2, 4, 8} except for FBX_RAND_GINIBRE (any shape); complex128 outputs.
 * fbx_random_kraus: CPTP Kraus sets out[B][K][d][d], K_j = G_j S^{-1/2}, S = sum_j G_j^H G_j with
 * Ginibre G_j -- kraus2choi of a set is a rand_map_with_BCSZ_dist(d, K) draw (:135-157).
 * Every argument is checked before anything is sized from it (host form included); B = 0 is FBX_OK and writes nothing.
 *
 * Stated accuracy (u = 2^-53; kappa_2 from the singular values of the fp64 Ginibre entries; max-abs over the entries;
 * the reference is mpmath at 50 digits on those same entries -- tests/random_cases.py, tests/test_random_exact_gpu.py):
 *   Ginibre entries and Ginibre states   1e-13 absolute against the float64 restatement of the stream
 *   Haar U:  |U^H U - 1| <= 1e-13;       |U - Q_exact| <= C_Q d u kappa_2(G),                C_Q = 8.8
 *   Kraus:   |K - K_exact| and |sum_j K_j^H K_j - 1| <= C_S d u kappa_2(S) + 32 d u,         C_S = 7.6
 * C_Q and C_S are 4 times what numpy's qr / eigh route measures against the same reference (2.11 and 1.83).  A flat bound
 * is not a contract S^{-1/2} can keep: with K = 1, S = G^H G reaches kappa_2(S) = 4.4e6 within 20 000 items at d = 8, and
 * numpy itself leaves a TP defect of 1.3e-10 there.  Measured on an MI355X, as multiples of d u kappa_2:
 *   worst-conditioned S of items 0..19999 of seed 17, K = 1      d = 2 (1.5e5)   d = 4 (7.6e5)   d = 8 (4.4e6)
 *     |K - K_exact|                                               0.006           0.007           0.004
 *     TP defect, and |K_1 K_1^H - 1|                              0.013           0.015           0.009
 *     |U - Q_exact| of the same item (kappa_2(G) = 382, 873, 2106) 0.020          0.004           0.006
 *   everything else tested (K = 1..64, items past the grid caps, 64-bit seeds and item ids): at most 0.07 of the Kraus
 *   bound against the oracle, 0.11 of it in the TP defect, 0.15 of the bound on U.
 * The eigensolver behind S^{-1/2} sweeps until its off-diagonal norm is below 2^-52 ||S||_F; at the solver's default stop of
 * 1e-13 ||S||_F a well-conditioned set (d = 4, K = 2, kappa_2(S) = 14) was 7.1e-14 from the exact one, outside this bound. */
#define FBX_RAND_GINIBRE        0
#define FBX_RAND_UNITARY        1
#define FBX_RAND_STATE_VECTOR   2
#define FBX_RAND_GINIBRE_STATE  3
#define FBX_RAND_BURES_STATE    4
int fbx_random_operators(int kind, int dim, int cols_or_rank, int64_t B, uint64_t seed,
                         int64_t first_item, double* out);
int fbx_random_operators_dev(int kind, int dim, int cols_or_rank, int64_t B, uint64_t seed,
                             int64_t first_item, double* d_out);
int fbx_random_kraus(int n_qubits, int64_t B, int K, uint64_t seed, int64_t first_item,
                     double* kraus_out);
int fbx_random_kraus_dev(int n_qubits, int64_t B, int K, uint64_t seed, int64_t first_item,
                         double* d_kraus_out);

/* ---------------------------------------------------------------- Clifford elements, RB sequences and their simulation
 * The reference hands the Clifford group work of randomized benchmarking to quilc through a BenchmarkConnection
 * (randomized_benchmarking.py:105-174: sample a uniform Clifford, compose, invert, conjugate a Pauli); here it is on the device, for
 * n_qubits = 1 and 2 as in the reference (get_rb_gateset, :77-90).  n_qubits > 2: FBX_ERR_UNSUPPORTED; < 1: FBX_ERR_BAD_ARG.
 *
 * Clifford elements.  An element C of the group modulo global phase is one uint32 word: the signed Pauli images C g C^+ of the
 * generators g_0 = X_0, g_1 = Z_0 (n = 1) and g_2 = X_1, g_3 = Z_1 (n = 2), image j in bits [5 j, 5 j + 5) --
 *     bits 5 j .. 5 j + 3   Pauli index of the image (the order of the project's PTMs: base-4 digits I X Y Z = 0 1 2 3, qubit 0
 *                           the most significant digit; 0..3 for n = 1, 0..15 for n = 2)
 *     bit  5 j + 4          1 when the image carries a minus sign
 * and every bit from 10 n on zero.  The identity is 0x61 (n = 1) and 0x18584 (n = 2).  A word is VALID when the images of X_q and
 * Z_q anticommute and images that belong to different qubits commute (which makes every image a non-identity Pauli); 24 and
 * 11 520 words are.  FBX_CLIFFORD_NONE is no element: "no interleaved gate" on the way in, "no such index" on the way out.
 * The Pauli transfer matrix of an element is the signed permutation with C P_k C^+ = +- P_perm(k); fbx/clifford.py is the host
 * mirror (from_index, compose, inverse, apply_to_pauli, to_ptm, to_gates) and documents the enumeration behind
 * fbx_clifford_from_index: elems_out[i] = the idx[i]-th element, a bijection from range(24) / range(11520) onto the group.  The
 * host form rejects an index that is not below the order; the _dev form writes FBX_CLIFFORD_NONE for it. */
#define FBX_CLIFFORD_NONE 0xFFFFFFFFu
int fbx_clifford_from_index(int n_qubits, int64_t B, const uint32_t* idx, uint32_t* elems_out);
int fbx_clifford_from_index_dev(int n_qubits, int64_t B, const uint32_t* d_idx, uint32_t* d_elems_out);

/* B randomized-benchmarking sequences (the quilc call behind generate_rb_sequence, randomized_benchmarking.py:105-126).  Sequence b
 * fills elems_out[offsets[b] .. offsets[b + 1]) (offsets[B + 1] int64, starting at 0, never decreasing; its length L_b may be 0):
 *   - interleaved_elem == FBX_CLIFFORD_NONE: elements 0, 1, 2, ... are independent uniform draws from the group;
 *     otherwise (interleaved RB) the even positions are the draws and every odd position holds interleaved_elem;
 *   - self_inverting != 0: the LAST element is instead the inverse of the composition of everything before it, interleaved
 *     elements included, so that the sequence composes to the identity (L_b = 1: the identity).  self_inverting == 0: that last
 *     element is simply not there -- the sequence equals the first L_b elements of the self-inverting sequence of length L_b + 1.
 * noise_id_out (may be NULL) marks interleaved elements 1 and every other element 0: the `noise_ids` of fbx_rb_simulate.
 * Sequence b owns the Philox4x32-10 stream keyed by (seed, b) (as fbx_random_operators' items do): its content depends on neither B
 * nor the launch shape, and the draws at the even positions of an interleaved sequence are the draws of the plain one.  A draw is
 * exactly uniform (multiply-high with rejection, no modulo).  The host form rejects offsets that do not start at 0 or decrease
 * and an interleaved_elem that is not a valid word; the _dev form cannot read its offsets and trusts them. */
int fbx_rb_sequences(int n_qubits, int64_t B, const int64_t* offsets, uint64_t seed, uint32_t interleaved_elem, int self_inverting,
                     uint32_t* elems_out, uint8_t* noise_id_out);
int fbx_rb_sequences_dev(int n_qubits, int64_t B, const int64_t* d_offsets, uint64_t seed, uint32_t interleaved_elem, int self_inverting,
                         uint32_t* d_elems_out, uint8_t* d_noise_id_out);

/* Noisy simulation of B sequences in the Pauli basis, D = 4^n_qubits: sequence b starts from the Pauli vector prep[D] (component
 * k = tr(P_k rho); NULL = |0..0>, 1 on the I/Z products and 0 elsewhere) and for each of its elements applies the element's signed
 * permutation and then the D x D Pauli transfer matrix noise_ptms[noise_ids[.]] (row-major [G][D][D], G in 1..16; noise_ids NULL =
 * all 0); out[B][D] is the final vector, prep itself for a sequence of length 0.  elems must not be NULL when B > 0, even if every
 * sequence is empty.  The RB observables are the I/Z-product columns
 * of out, the unitarity ones all of them.  The permutation is exact and a row of the noise step is one chain of D fused
 * multiply-adds in ascending column order from 0.0, so a sequence's result depends on nothing but the sequence.
 * Bad input: the host form rejects (FBX_ERR_BAD_ARG) an invalid element word, a noise id >= G and malformed offsets before any
 * device work; the _dev form reads nothing through such a value and fills out[b] with NaN for that sequence only.  A non-finite
 * PTM entry reaches only the sequences that use that PTM; every other sequence is bit-identical to a run with finite PTMs. */
int fbx_rb_simulate(int n_qubits, int64_t B, const int64_t* offsets, const uint32_t* elems, const uint8_t* noise_ids, int G,
                    const double* noise_ptms, const double* prep, double* out);
int fbx_rb_simulate_dev(int n_qubits, int64_t B, const int64_t* d_offsets, const uint32_t* d_elems, const uint8_t* d_noise_ids, int G,
                        const double* d_noise_ptms, const double* d_prep, double* d_out);

/* ---------------------------------------------------------------- simulated RB and unitarity experiments: channels to expectations
 * What generate_rb_experiment_sequences / generate_unitarity_experiment_sequences with acquire_rb_data / acquire_unitarity_data
 * (randomized_benchmarking.py:129-305, 441-487) get from quilc and a QVM, for E experiments at once and in one launch: every
 * experiment draws S K sequences, runs them under its own noise and measures them; no element word reaches memory.  n_qubits is 1
 * or 2, D = 4^n_qubits, M = 2^n_qubits; Pauli order, normalisation and element words are those of fbx_rb_simulate.
 *
 * Inputs.  depths [S]: the depth of the sequences q = i K .. i K + K - 1 (depth index i, repetition s = q - i K: the order of
 * fbx/randomized_benchmarking.py generate_rb_sequences_batch), counted as generate_rb_sequence counts it; a HOST array in both
 * forms (its S <= 256 numbers travel with the launch).  K: the sequences per depth.  mode: FBX_RB_STANDARD -- self-inverting
 * sequences measured in Z on every qubit -- or FBX_RB_UNITARITY -- sequences without the inverse, every Pauli measured.
 * interleaved_elem: as in fbx_rb_sequences, FBX_CLIFFORD_NONE for a plain run.  noise_ptms [E][G][D][D]: G = 1, or 2 with an
 * interleaved element; matrix 0 follows every random Clifford and the inverse, matrix 1 the interleaved element.  prep [D] or NULL
 * (|0..0>), shared by the batch, as in fbx_rb_simulate.  flips [E][n_qubits][2] or NULL: [q][0] = P(read 1 | 0), [q][1] =
 * P(read 0 | 1) of qubit q, independent per bit, as in fbx_tomo_simulate.  n_shots: the shots of every sequence and basis; 0 = the
 * exact expectations, no shots.  seed, first_item: as in fbx_tomo_simulate; gid = first_item + e.
 *
 * Outputs, each may be NULL, not all.  NB bases are measured and C Paulis estimated per sequence:
 *   FBX_RB_STANDARD    NB = 1 (Z on every qubit), C = M - 1: the I/Z products in the order Z (n = 1) and IZ, ZI, ZZ (n = 2)
 *   FBX_RB_UNITARITY   NB = 3^n_qubits, C = D - 1: column c is the Pauli with index c + 1.  Basis index in base 3, digits X, Y, Z
 *                      = 0, 1, 2, qubit 0 most significant.
 *   vec_out    [E][S K][D] double         the exact final Pauli vectors
 *   prob_out   [E][S K][NB][M] double     the outcome distributions, flips included, unclamped; outcome o = the measured bits,
 *                                         qubit 0 most significant, bit value 1 = eigenvalue -1
 *   hist_out   [E][S K][NB][M] uint32     the counted outcomes (n_shots >= 1 only)
 *   expect_out, std_err_out [E][S K][C] double          status_out [E] int32
 *
 * Per experiment e and sequence q:
 *  1. SEQUENCE.  The elements are exactly those fbx_rb_sequences writes for sequence b = q under the seed (seed + gid) mod 2^64,
 *     with the same interleaved_elem, self_inverting = 1 (FBX_RB_STANDARD) or 0 (FBX_RB_UNITARITY) and the length of the depth:
 *     depth - 1 draws (each followed by the interleaved element, if any) and the inverse, or `depth` draws.  The draws are those
 *     of its stream (Philox4x32-10, key = that seed, counter (q low, q high, draw, 0x52420000 + attempt)).
 *  2. FINAL VECTOR.  From prep, each element's signed permutation and then its noise matrix, a row being one chain of fused
 *     multiply-adds in ascending column order from 0.0: vec_out equals fbx_rb_simulate's out on those sequences bit for bit.
 *  3. DISTRIBUTION.  For the basis (P_0[, P_1]) and the final vector v, outcome o has
 *         p(o) = 2^-n sum_T (-1)^|o & T| v[P_T],
 *     T over the subsets of the qubits, P_T the product of the basis' Paulis on T, v[P_{}] = v_I (1 for a trace-preserving
 *     map).  Then per bit the confusion matrix of its qubit's flips, exactly as step 2 of fbx_tomo_simulate_grouped.
 *  4. SHOTS.  c_o = the running sum of max(p(o'), 0) in outcome order; thr_o = floor(c_o / c_last 2^32) for every outcome but
 *     the last.  Shot s of n_shots reads word s & 3 of the Philox4x32-10 block with counter (gid low, gid high, q NB + basis,
 *     s >> 2) and key (seed low ^ 0x52424151, seed high); the tag "RBAQ" keeps the stream apart from every other simulator's
 *     under one seed.  The outcome of a word is the number of thresholds <= the word; hist_out counts the outcomes.
 *  5. EXPECTATIONS.  Every Pauli is read from exactly ONE basis: the one that measures its non-identity factors and Z on
 *     every qubit where it has the identity (IX from ZX, YI from YZ).  With n_odd the shots of that basis' histogram whose bits
 *     on the Pauli's support have odd parity, mean = ((N - n_odd) - n_odd) / N and std_err = sqrt((1 - mean^2) / N), without
 *     fused multiply-adds (the moments of fbx_rpe_simulate).  In FBX_RB_STANDARD IZ, ZI and ZZ come from the same shots: in
 *     every shot the ZZ value is the product of the other two, which is what fbx_rb_survival's covariance term assumes.
 *     n_shots = 0: expect_out holds the exact components of the final vector and std_err_out 0.
 * A value depends on (seed, gid, q, basis), the experiment's inputs and n_shots only: not on E, the experiment's position in the
 * batch or the launch shape; a batch is cut with first_item.
 *
 * A poisoned experiment -- a non-finite entry of its matrices or of prep, a flip outside [0, 1] or NaN, or a distribution whose
 * c_last is not a positive finite number (an all-zero matrix, a product that overflows) -- gets status 1, NaN in every double
 * output and 0 in hist_out, for ALL its sequences; its neighbours are bit-identical to a clean call.
 * n_qubits >= 3 and S > 256: FBX_ERR_UNSUPPORTED.  FBX_ERR_BAD_ARG before any buffer is touched: n_qubits < 1, E < 0, S < 1,
 * K < 1, an unknown mode, NULL depths, a depth below 2 (FBX_RB_STANDARD) or 1 (FBX_RB_UNITARITY), an interleaved element that is
 * no valid word or comes with FBX_RB_UNITARITY, G other than 1 (plain) / 2 (interleaved), first_item < 0, n_shots outside
 * 0 .. 2^31 - 1, S K NB >= 2^32, every output NULL, hist_out with n_shots = 0, NULL noise_ptms.  E == 0: nothing is done.
 * The _dev form enqueues on the calling thread's stream and does not synchronise. */
#define FBX_RB_STANDARD   0
#define FBX_RB_UNITARITY  1
int fbx_rb_acquire(int n_qubits, int64_t E, int S, const int32_t* depths, int K, int mode, uint32_t interleaved_elem, int G,
                   const double* noise_ptms, const double* prep, const double* flips, int64_t n_shots, uint64_t seed,
                   int64_t first_item, double* vec_out, double* prob_out, uint32_t* hist_out, double* expect_out,
                   double* std_err_out, int32_t* status_out);
int fbx_rb_acquire_dev(int n_qubits, int64_t E, int S, const int32_t* depths, int K, int mode, uint32_t interleaved_elem, int G,
                       const double* d_noise_ptms, const double* d_prep, const double* d_flips, int64_t n_shots, uint64_t seed,
                       int64_t first_item, double* d_vec_out, double* d_prob_out, uint32_t* d_hist_out, double* d_expect_out,
                       double* d_std_err_out, int32_t* d_status_out);

/* values [E][S][K][C] -> mean_out [E][S][C], the mean over the K sequences of a depth, and std_err_out [E][S][C], the standard
 * error of that mean: sqrt(var(ddof = 1) / K) for K > 1; for K = 1 the sequence's own standard error seq_std_errs [E][S][C], or 0
 * when that is NULL (it is not read for K > 1).  One lane per output cell sums in ascending s, without fused multiply-adds: a
 * result depends on its K values only.  C is free: the expectations of fbx_rb_acquire (C = M - 1 or D - 1), survival
 * probabilities or purities (C = 1).  Each output may be NULL, not both.  The _dev form enqueues on the calling thread's stream. */
int fbx_rb_depth_means(int64_t E, int S, int K, int C, const double* values, const double* seq_std_errs, double* mean_out,
                       double* std_err_out);
int fbx_rb_depth_means_dev(int64_t E, int S, int K, int C, const double* d_values, const double* d_seq_std_errs, double* d_mean_out,
                           double* d_std_err_out);

/* ---------------------------------------------------------------- qubit spectroscopy, acquisition (qubit_spectroscopy.py)
 * fbx_spec_acquire: what do_t1_or_t2, acquire_rabi_data and acquire_cz_phase_ramsey_data (qubit_spectroscopy.py:81-112, 325-356,
 * 421-447) get from a QuantumComputer, for B experiments (a qubit each) of K points in one launch: the probability of reading 1
 * from a physical curve and the readout flips, the shots of every point, and the bit statistics the fit front ends read.
 *
 * Inputs.  x: the K points (delay times, rotation angles), [K] shared by the batch (x_stride = 0) or [B][K] (x_stride = K), as in
 * fbx_curve_fit.  params [B][6] = (amplitude, decay_time, gauss_time, omega, offset, baseline).  flips [B][2] or NULL: [0] =
 * P(read 1 | 0), [1] = P(read 0 | 1).  n_shots: the shots of every point; 0 = the exact expectations, no shots.  seed,
 * first_item: as in fbx_tomo_simulate; gid = first_item + b.
 *
 * Outputs, each may be NULL, not all; every one is [B][K] double but status_out [B] int32.
 *
 * Per item b and point k, all in fp64, every operation but exp and cos rounded once on its own (no fused multiply-adds), so
 * that numpy doing the same operations in the same order differs through the two functions only:
 *  1. ENVELOPE.  env = exp(-(x / decay_time) - (x / gauss_time) * (x / gauss_time)).  +inf is allowed for either time; its term
 *     is then 0.
 *  2. CURVE.  arg = omega * x + offset;  p_true = baseline + (amplitude * env) * cos(arg).
 *  3. READOUT.  Without flips p_read = p_true; with flips p_read = f0 * (1 - p_true) + (1 - f1) * p_true.  prob_out = p_read,
 *     unclamped.
 *  4. MEAN.  mu = 1 - 2 * p_read, the expectation of the measured Pauli (bit 1 = eigenvalue -1).  exact_out = mu.
 *  5. SHOTS.  The unit of fbx_tomo_simulate with coefficient 1: t = floor(clamp(0.5 mu + 0.5, 0, 1) 2^32); shot s of n_shots
 *     counts +1 iff word s & 3 of the Philox4x32-10 block with counter (gid low, gid high, k, s >> 2) and key (seed low ^
 *     0x51535043, seed high) is below t; the tag "QSPC" keeps the stream apart from every other simulator's under one seed.
 *     t = 0 and t = 2^32 (p_read >= 1, p_read <= 0) give all -1 / all +1 without draws.  expect_out = (k_plus - k_minus) / N,
 *     std_err_out = sqrt(4 k_plus k_minus / N) / N, counts_out = N.
 *     n_shots = 0: expect_out = mu, std_err_out = 0, counts_out = 0, and nothing is drawn.
 *  6. BIT FORM, what the fit front ends of fbx/qubit_spectroscopy.py build from (expectation, standard error), bit for bit:
 *     bit_out = ((-1 * expect) + 1) / 2, the estimated probability of reading 1;  bit_err_out = sqrt((std_err * std_err) / 4).
 * A value depends on (seed, gid, k), the item's inputs and n_shots only: not on B, the item's position in the batch or the
 * launch shape; a batch is cut with first_item.  From B K >= 131072 units on a lane takes a unit, below that a wavefront; both
 * give the same bits.
 *
 * A poisoned item -- a non-finite amplitude, omega, offset or baseline; a decay_time or gauss_time that is not > 0 (NaN included;
 * +inf is fine); a non-finite x among its K points; a flip outside [0, 1] or NaN -- gets status 1, NaN in every double output
 * and counts_out = n_shots; its neighbours are bit-identical to a clean call.  A p_read outside [0, 1] is not poison: it is
 * clamped for the threshold only.
 * FBX_ERR_BAD_ARG before any buffer is touched: B < 0, n_shots outside 0 .. 2^32 - 1, first_item < 0, K outside 1 .. 65536,
 * x_stride neither 0 nor K, NULL x or params with B > 0, every output NULL.  B == 0: nothing is done.
 * The _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_spec_acquire(int64_t B, int K, const double* x, int64_t x_stride, const double* params, const double* flips, int64_t n_shots,
                     uint64_t seed, int64_t first_item, double* prob_out, double* exact_out, double* expect_out, double* std_err_out,
                     double* counts_out, double* bit_out, double* bit_err_out, int32_t* status_out);
int fbx_spec_acquire_dev(int64_t B, int K, const double* d_x, int64_t x_stride, const double* d_params, const double* d_flips,
                         int64_t n_shots, uint64_t seed, int64_t first_item, double* d_prob_out, double* d_exact_out,
                         double* d_expect_out, double* d_std_err_out, double* d_counts_out, double* d_bit_out, double* d_bit_err_out,
                         int32_t* d_status_out);

/* ---------------------------------------------------------------- Clifford circuits and direct fidelity estimation, 1..64 qubits
 * The experiment generators of direct_fidelity_estimation.py:15-182 and the noisy expectations of their settings for a Clifford
 * circuit with Pauli noise, exact in the Heisenberg picture: the observable walks backwards through the circuit as a signed Pauli
 * and picks up a factor 1 - p at every noisy gate it touches.  n_qubits outside 1..64: FBX_ERR_BAD_ARG.
 *
 * Pauli.  (x, z, sign): two uint64 masks and a uint8.  Bit q of a mask belongs to qubit q, which is index q of a label string (as
 * in str_to_pauli_term, utils.py:127-143).  Per qubit (x, z) = 00 I, 10 X, 11 Y, 01 Z, Y being the Hermitian Y; the operator is
 * (-1)^sign times the tensor product.  Bits from n_qubits on are ignored on the way in and zero on the way out; only bit 0 of a
 * sign byte is read.
 *
 * Gate word.  uint32: opcode in bits 0..7, q0 in bits 8..15, q1 in bits 16..23, the rest zero (q1 is zero for a one-qubit gate).
 * The one-qubit gates act on q0; CNOT has q0 as control and q1 as target; CZ and SWAP need q0 != q1.  A circuit is gates[G],
 * applied in index order, G >= 0.  fbx/clifford_circuit.py is the host mirror and encodes the (name, qubits) tuples that
 * fbx.clifford.to_gates emits. */
#define FBX_GATE_H 0
#define FBX_GATE_S 1
#define FBX_GATE_SDG 2
#define FBX_GATE_X 3
#define FBX_GATE_Y 4
#define FBX_GATE_Z 5
#define FBX_GATE_RX_PLUS 6   /* RX(pi/2)  */
#define FBX_GATE_RX_MINUS 7  /* RX(-pi/2) */
#define FBX_GATE_RY_PLUS 8   /* RY(pi/2)  */
#define FBX_GATE_RY_MINUS 9  /* RY(-pi/2) */
#define FBX_GATE_RZ_PLUS 10  /* RZ(pi/2)  */
#define FBX_GATE_RZ_MINUS 11 /* RZ(-pi/2) */
#define FBX_GATE_CNOT 12
#define FBX_GATE_CZ 13
#define FBX_GATE_SWAP 14
#define FBX_DFE_NOISELESS 255 /* noise class of a gate without noise */
/* Conjugation U P U^+ by one gate; s is the sign flip, evaluated on the values BEFORE the update (a = q0, b = q1):
 *     H                  s = x&z               swap x, z
 *     S,   RZ(pi/2)      s = x&z               z ^= x
 *     SDG, RZ(-pi/2)     s = x&~z              z ^= x
 *     X                  s = z
 *     Y                  s = x^z
 *     Z                  s = x
 *     RX(pi/2)           s = z&~x              x ^= z
 *     RX(-pi/2)          s = z&x               x ^= z
 *     RY(pi/2)           s = x&~z              swap x, z
 *     RY(-pi/2)          s = z&~x              swap x, z
 *     CNOT(a, b)         s = xa&zb&~(xb^za)    xb ^= xa; za ^= zb
 *     CZ(a, b)           s = xa&xb&(za^zb)     za ^= xb; zb ^= xa
 *     SWAP                                     swap both pairs
 * The inverse direction U^+ P U walks the list backwards with every gate's inverse (S <-> SDG, RX / RY / RZ(+) <-> (-), the rest
 * are their own inverses).
 *
 * GATE WORDS ARE VALIDATED BY WHOEVER CAN READ THEM.  The host-pointer forms refuse (FBX_ERR_BAD_ARG, before any buffer is
 * touched) an unknown opcode, a qubit index >= n_qubits, q0 == q1 on a two-qubit gate and a word with other bits set.  The _dev
 * forms cannot read their words and take them as validated by the caller (run them through the host form or through
 * clifford_circuit.encode_gates once).  A word that was not is harmless but meaningless: qubit indices are reduced mod 64, an
 * unknown opcode does nothing, an unknown noise class is not counted -- no access depends on a word's content.
 *
 * fbx_clifford_conjugate: M Paulis, one per lane, through the circuit: inverse == 0 gives U P U^+, otherwise U^+ P U.  It stands in
 * for BenchmarkConnection.apply_clifford_to_pauli.  M == 0: nothing is done. */
int fbx_clifford_conjugate(int n_qubits, int64_t G, const uint32_t* gates, int inverse, int64_t M, const uint64_t* x_in,
                           const uint64_t* z_in, const uint8_t* sign_in, uint64_t* x_out, uint64_t* z_out, uint8_t* sign_out);
int fbx_clifford_conjugate_dev(int n_qubits, int64_t G, const uint32_t* d_gates, int inverse, int64_t M, const uint64_t* d_x_in,
                               const uint64_t* d_z_in, const uint8_t* d_sign_in, uint64_t* d_x_out, uint64_t* d_z_out,
                               uint8_t* d_sign_out);

/* Setting.  in_x, in_z, in_minus, obs_x, obs_z (uint64) and obs_sign (uint8), one entry per setting.  The in-state is a product of
 * one-qubit Pauli eigenstates: (in_x, in_z) bit q is the label of qubit q (X, Y or Z, never I), in_minus bit q is set for the -1
 * eigenstate; |0..0> is Z everywhere with in_minus = 0.  The observable is (-1)^obs_sign times the Pauli (obs_x, obs_z).
 *
 * fbx_dfe_settings writes the m settings of one of the reference's four generators for the circuit, conjugation included.
 * n_terms == 0 is exhaustive (m >= 2^31 is refused):
 *   FBX_KIND_STATE    m = 2^n - 1.  Setting k is string k + 1 (counting from 0: the all-identity string is skipped) of
 *                     itertools.product('IZ', repeat=n), qubit 0 the most significant digit; the in-state is |0..0>, the observable
 *                     U Z-string U^+ (direct_fidelity_estimation.py:91-94).
 *   FBX_KIND_PROCESS  m = (4^n - 1) 2^n.  Setting k = (j - 1) 2^n + e has string j of product('IXYZ', repeat=n) as its Pauli P; the
 *                     in-state labels are P with I replaced by Z, the eigenvalue bits are e (qubit 0 most significant), and the
 *                     observable is U P U^+ times (-1)^(minus bits on the qubits where P is not I) (:46-66).
 * n_terms > 0 is Monte Carlo with m = n_terms (:117-129, :153-182), from a documented stream in place of np.random.  With
 * valid = the mask of the n low bits: attempt a = 0, 1, ... of setting k reads the words w0..w3 of the Philox4x32-10 block with
 * counter (k low, k high, a, 0) and key (seed low ^ 0x44464553, seed high).  State: the Z mask is (w0 | w1 << 32) & valid.
 * Process: x = (w0 | w1 << 32) & valid, z = (w2 | w3 << 32) & valid.  The first attempt that is not the identity is kept (the
 * reference's resampling loop); the process kind then reads the block (k low, k high, a, 1) of that attempt for the eigenvalue
 * bits (w0 | w1 << 32) & valid.  After 256 rejected attempts z = valid (and x = valid for a process) is taken with a = 256, so the
 * loop is finite.  A setting depends on (seed, k) only.  A wrong m, a negative size, an unknown kind: FBX_ERR_BAD_ARG. */
int fbx_dfe_settings(int n_qubits, int kind, int64_t n_terms, uint64_t seed, int64_t G, const uint32_t* gates, int64_t m,
                     uint64_t* in_x, uint64_t* in_z, uint64_t* in_minus, uint64_t* obs_x, uint64_t* obs_z, uint8_t* obs_sign);
int fbx_dfe_settings_dev(int n_qubits, int kind, int64_t n_terms, uint64_t seed, int64_t G, const uint32_t* d_gates, int64_t m,
                         uint64_t* d_in_x, uint64_t* d_in_z, uint64_t* d_in_minus, uint64_t* d_obs_x, uint64_t* d_obs_z,
                         uint8_t* d_obs_sign);

/* fbx_dfe_propagate: one lane per setting walks the UNSIGNED observable (obs_x, obs_z) backwards through the circuit (obs_sign is
 * not read and may be NULL).  noise_class[G] is uint8: a class < K, 1 <= K <= 16, or FBX_DFE_NOISELESS; NULL means every gate is
 * class 0.  touches_out [m][K] uint32: touches[k][c] = the number of gates of class c on whose qubits the walking Pauli is not the
 * identity.  A gate maps Paulis that are the identity on its qubits to themselves and no others, so whether this is looked at
 * before or after passing the gate makes no difference.  sigma_out [m] int8 = the ideal expectation of the unsigned observable in
 * the in-state: with O_0 the Pauli that arrives at the start of the circuit, 0 if O_0 differs from the in-state's label on any
 * qubit where O_0 is not I, otherwise (-1)^(sign of O_0 + popcount(in_minus & support of O_0)).
 * The host form also refuses a class that is neither below K nor 255 and an in-state label of I. */
int fbx_dfe_propagate(int n_qubits, int64_t G, const uint32_t* gates, const uint8_t* noise_class, int K, int64_t m,
                      const uint64_t* in_x, const uint64_t* in_z, const uint64_t* in_minus, const uint64_t* obs_x,
                      const uint64_t* obs_z, const uint8_t* obs_sign, int8_t* sigma_out, uint32_t* touches_out);
int fbx_dfe_propagate_dev(int n_qubits, int64_t G, const uint32_t* d_gates, const uint8_t* d_noise_class, int K, int64_t m,
                          const uint64_t* d_in_x, const uint64_t* d_in_z, const uint64_t* d_in_minus, const uint64_t* d_obs_x,
                          const uint64_t* d_obs_z, const uint8_t* d_obs_sign, int8_t* d_sigma_out, uint32_t* d_touches_out);

/* fbx_dfe_simulate: B items share the m settings (sigma, touches of fbx_dfe_propagate and the observables) and differ in noise.
 * class_error [B][K]: the depolarizing probability of every gate of class c; readout_flip [B][n]: a symmetric flip probability per
 * qubit.  Either may be NULL (= 0).  Outputs [B][m] and status_out [B] as those of fbx_tomo_simulate; each may be NULL, not all.
 *
 * THE MEAN.  mu = sigma_k prod_c (1 - p_{b,c})^touches[k][c] prod_{q in S_k} (1 - 2 f_{b,q}), S_k = the support obs_x | obs_z.
 * A depolarizing channel rho -> (1 - p) rho + p tr_g(rho) (x) I / d_g on the qubits of gate g, applied after the gate, scales
 * every Pauli that is not the identity there by 1 - p and leaves the others alone; symmetric flips scale a product of bits by
 * 1 - 2 f each.  Only symmetric flips are modelled: the reference's default for DFE is exhaustive symmetrization, which makes the
 * effective readout error symmetric.  The powers are formed by repeated squaring and the factors multiplied in ascending class
 * and qubit order: at most one rounding per factor.  calibration != 0: mu is the readout product alone and c_k = 1 -- the
 * observable with coefficient 1 measured on its own +1 eigenstate, what calibrate_observable_estimates acquires
 * (observable_estimation.py:1005-1020) -- under a key tag of its own.  exact_out = c_k mu, c_k = (-1)^obs_sign.
 *
 * THE STREAM and the three sampled outputs are, word for word, those of fbx_tomo_simulate -- t = floor((0.5 mu + 0.5) 2^32) after
 * clamping, shot s of setting k of the global item g = first_item + b reads word s & 3 of the block with counter (g low, g high, k,
 * s >> 2), expect_out = c_k (k_plus - k_minus) / N, counts_out = N, std_err_out = sqrt(4 k_plus k_minus / N) / N, n_shots == 0 the
 * exact-only mode -- with the key (seed low ^ 0x44464530, seed high), or (seed low ^ 0x44464543, seed high) when calibrating.
 * From B m = 131072 units on a lane takes a unit, below a wavefront does; both give the same bits.
 * A poisoned item -- a class error or a flip outside [0, 1], or NaN -- gets status 1, NaN in expect_out / std_err_out / exact_out
 * and N in counts_out; its neighbours are untouched.  n_shots >= 2^32, m >= 2^32, a negative size, first_item < 0, K outside
 * 1..16, a NULL settings buffer, every output NULL, n_shots == 0 with a sampled output requested: FBX_ERR_BAD_ARG before any
 * buffer is touched.  B == 0 or m == 0: nothing is done.  The _dev forms enqueue on the calling thread's stream. */
int fbx_dfe_simulate(int n_qubits, int64_t m, int K, const int8_t* sigma, const uint32_t* touches, const uint64_t* obs_x,
                     const uint64_t* obs_z, const uint8_t* obs_sign, int64_t B, const double* class_error, const double* readout_flip,
                     int calibration, int64_t n_shots, uint64_t seed, int64_t first_item, double* expect_out, double* counts_out,
                     double* std_err_out, double* exact_out, int32_t* status_out);
int fbx_dfe_simulate_dev(int n_qubits, int64_t m, int K, const int8_t* d_sigma, const uint32_t* d_touches, const uint64_t* d_obs_x,
                         const uint64_t* d_obs_z, const uint8_t* d_obs_sign, int64_t B, const double* d_class_error,
                         const double* d_readout_flip, int calibration, int64_t n_shots, uint64_t seed, int64_t first_item,
                         double* d_expect_out, double* d_counts_out, double* d_std_err_out, double* d_exact_out,
                         int32_t* d_status_out);

/* The resident chain: the simulation above (expectations and standard errors), with calibrate != 0 a second one in calibration
 * mode whose (expectation, standard error^2) of item b and setting k are the calibration of that result
 * (fbx_calibrate_expectations' arithmetic), then estimate_dfe (direct_fidelity_estimation.py:291-307) with d = 2^n as a double,
 * for any n up to 64: fidelity_out [B], err_out [B], status_out [B] or NULL.  Nothing of size [B][m] leaves the device.  m >= 1
 * and n_shots >= 1 are required; a poisoned item comes out as NaN. */
int fbx_dfe_simulate_fidelity(int n_qubits, int64_t m, int K, const int8_t* sigma, const uint32_t* touches, const uint64_t* obs_x,
                              const uint64_t* obs_z, const uint8_t* obs_sign, int64_t B, const double* class_error,
                              const double* readout_flip, int64_t n_shots, uint64_t seed, int64_t first_item, int kind, int calibrate,
                              double* fidelity_out, double* err_out, int32_t* status_out);
int fbx_dfe_simulate_fidelity_dev(int n_qubits, int64_t m, int K, const int8_t* d_sigma, const uint32_t* d_touches,
                                  const uint64_t* d_obs_x, const uint64_t* d_obs_z, const uint8_t* d_obs_sign, int64_t B,
                                  const double* d_class_error, const double* d_readout_flip, int64_t n_shots, uint64_t seed,
                                  int64_t first_item, int kind, int calibrate, double* d_fidelity_out, double* d_err_out,
                                  int32_t* d_status_out);

/* ---------------------------------------------------------------- shots of a noisy Clifford circuit: Pauli frames, 1..64 qubits
 * Measured bitstrings of a Clifford circuit with Pauli noise without a state vector (csrc/fbx_frames.hip): the
 * experiment half of entangled_states.py (create_ghz_program, create_graph_state, measure_graph_state are Clifford circuits) at
 * any width up to 64.  The circuit is gates[G] (the gate words above) on |0..0>, followed by a Z measurement of every qubit.
 *
 * fbx_clifford_reference_sample: reference_out[0] = x0, one outcome of the NOISELESS circuit, bit q = qubit q: the outcome of
 * non-zero probability with the smallest outcome index, qubit 0 being the most significant bit of the index as everywhere in this
 * library -- equivalently, what comes out when the qubits 0, 1, .., n - 1 are measured in this order and every random result is
 * taken as 0.  It runs on the device, one wavefront: a stabilizer tableau with one generator pair per lane.  n_qubits outside
 * 1..64, G < 0, NULL gates with G > 0, NULL reference_out: FBX_ERR_BAD_ARG.  G == 0 gives 0.  The host form validates the gate
 * words; the _dev form enqueues on the calling thread's stream and does not synchronise. */
int fbx_clifford_reference_sample(int n_qubits, int64_t G, const uint32_t* gates, uint64_t* reference_out);
int fbx_clifford_reference_sample_dev(int n_qubits, int64_t G, const uint32_t* d_gates, uint64_t* d_reference_out);

/* fbx_clifford_sample_shots: B items share the circuit and differ in noise; n_shots shots each, one lane per shot.
 * noise_class [G] uint8: a class < K, 1 <= K <= 16, or FBX_DFE_NOISELESS; NULL = every gate is class 0.  class_error [B][K] or NULL
 * (= 0).  readout_flip [B][n][2] or NULL (= no flips) with the meaning of fbx_sample_bitstrings: [j][0] = P(read 1 | drawn 0),
 * [j][1] = P(read 0 | drawn 1).  reference: one uint64, the output of fbx_clifford_reference_sample for the same circuit (a DEVICE
 * pointer in the _dev form: the chain reference -> shots needs no synchronisation).  Outputs, either may be NULL, not both:
 * bits_out [B][n_shots][n] uint8 0 / 1, first column = qubit 0 (the records fbx_shots_to_moments and fbx_bit_histogram read);
 * words_out [B][n_shots] uint64, the same outcome packed, bit q = qubit q.  status_out [B] or NULL: 0 good, 1 poisoned.
 *
 * THE MODEL.  After a gate of class c, item b applies the depolarizing channel of fbx_dfe_simulate to that gate's qubits: with
 * probability class_error[b][c] a Pauli drawn uniformly from ALL 4 (one-qubit gate) or 16 (two-qubit gate) Paulis, the identity
 * included, is applied -- rho -> (1 - p) rho + p tr_g(rho) (x) I / d_g, which scales a Pauli that is not the identity there by
 * 1 - p, so the shots of this function have the means of fbx_dfe_simulate.  A shot carries a Pauli frame (fx, fz), its difference
 * from the reference run.  It starts as fx = 0, fz = a uniformly random mask: Z on |0> is a stabilizer, so this changes nothing
 * physical, and it is what spreads the shots over the whole support of the outcome distribution.  Every gate conjugates the frame
 * with the table above (signs are not tracked: a frame is a Pauli up to phase), an error XORs its Pauli in, and the outcome is
 * reference ^ fx.  Readout flips follow.  The shots are exact samples of the noisy circuit.
 *
 * THE STREAM (part of the contract: it is what a host check restates).  Shot s of the global item g = first_item + b owns the
 * Philox4x32-10 blocks with counter (g low, g high, s, j) and key (seed low ^ 0x43465253, seed high), words x0 .. x3 each.
 *   Block 0:             fz = (x0 | (uint64) x1 << 32) & valid, valid = the mask of the n low bits.
 *   Block 1 + (l >> 1):  gate l, words (x0, x1) for even l and (x2, x3) for odd l.  A gate whose class is not FBX_DFE_NOISELESS errs
 *                        iff (double) x_first * 2^-32 < class_error[b][c]; the Pauli index is then x_second >> 30 for a one-qubit
 *                        gate and x_second >> 28 = 4 a + c for a two-qubit gate, a on q0 and c on q1; 0 I, 1 X, 2 Y, 3 Z.
 *   Readout:             with J = 1 + ((G + 1) >> 1), column j reads word j & 3 of block J + (j >> 2) and flips iff
 *                        (double) x * 2^-32 < readout_flip[b][j][d], d the drawn bit.
 * Only the blocks that are needed are computed: a gate block when one of its gates has a class with a non-zero error probability,
 * the readout blocks when readout_flip is given.  A record depends on (seed, g, s), the circuit and its item's noise only: not on
 * B, n_shots or the launch shape -- a call of B' items from first_item + k repeats items k .. k + B' - 1, and a call of fewer shots
 * repeats the first shots.
 *
 * n_qubits outside 1..64, G >= 2^31, n_shots >= 2^32, K outside 1..16, a negative size, first_item < 0, NULL gates with G > 0,
 * NULL reference, both outputs NULL, B * ceil(n_shots / 256) >= 2^31: FBX_ERR_BAD_ARG before any buffer is touched.  B == 0 or
 * n_shots == 0: nothing is done.  A poisoned item -- a class error or a flip outside [0, 1], or NaN -- gets status 1 and a record
 * of zeros; its neighbours are untouched.  The host form also refuses an invalid gate word or class; the _dev form takes them as
 * validated (see above: no access depends on a word's content).  The _dev form enqueues on the calling thread's stream and does
 * not synchronise. */
int fbx_clifford_sample_shots(int n_qubits, int64_t G, const uint32_t* gates, const uint8_t* noise_class, int K,
                              const uint64_t* reference, int64_t B, int64_t n_shots, const double* class_error,
                              const double* readout_flip, uint64_t seed, int64_t first_item, uint8_t* bits_out, uint64_t* words_out,
                              int32_t* status_out);
int fbx_clifford_sample_shots_dev(int n_qubits, int64_t G, const uint32_t* d_gates, const uint8_t* d_noise_class, int K,
                                  const uint64_t* d_reference, int64_t B, int64_t n_shots, const double* d_class_error,
                                  const double* d_readout_flip, uint64_t seed, int64_t first_item, uint8_t* d_bits_out,
                                  uint64_t* d_words_out, int32_t* d_status_out);

/* ---------------------------------------------------------------- shots of a noisy reversible circuit: classical bits, 1..64 qubits
 * Measured bitstrings of a circuit that only ever holds a product of Z or X eigenstates and whose gates act classically on them
 * (csrc/fbx_reversible.hip): the experiment half of classical_logic/ripple_carry_adder.py (adder,
 * get_n_bit_adder_results).  CCNOT is not Clifford, so the Pauli frames above do not apply; a shot is instead ONE 64-bit word
 * of classical bits, bit q = the bit qubit q holds, and which basis a qubit holds its bit in (Z: |0>, |1>; X: |+>, |->) is a
 * static property of the circuit that fbx.classical_logic.reversible.encode_reversible resolves into the micro-op words below.
 *
 * THE WORD (uint32):
 *   bits  0..2   micro-op, FBX_REV_*
 *   bits  3..4   k = the number of qubits of the gate, 1..3: its operands are q0 .. q(k-1), all different
 *   bits  5..10  q0, bits 11..16 q1, bits 17..22 q2 (0 when the gate has no such operand)
 *   bits 23..25  for operand 0, 1, 2: 1 when the qubit holds its bit in X AFTER the gate -- a Pauli error flips it through its Z
 *                part; 0: it holds it in Z and a Pauli error flips it through its X part (0 when there is no such operand)
 *   bits 26..31  XIN only: the bit of the unit's input word that decides whether the gate exists (0 otherwise)
 * FBX_REV_SITE    no change of a bit (H; X on a bit held in X; CZ on two bits held in Z): an error site only
 * FBX_REV_NOT     bit q0 ^= 1                    (X on a bit held in Z), k = 1
 * FBX_REV_XOR     bit q0 ^= bit q1               (CNOT(c, t) in Z: q0 = t, q1 = c; in X: q0 = c, q1 = t; CZ on a Z-held and an
 *                                                 X-held bit: q0 = the X-held one, q1 = the Z-held one), k = 2
 * FBX_REV_ANDXOR  bit q0 ^= bit q1 & bit q2      (CCNOT(c1, c2, t), all in Z: q0 = t, q1 = c1, q2 = c2), k = 3
 * FBX_REV_XIN     bit q0 ^= 1 iff the input bit is set, and the gate -- its error site included -- exists only then
 *                 (bitstring_prep's RX(pi * bit)), k = 1, the bit held in Z */
#define FBX_REV_SITE 0
#define FBX_REV_NOT 1
#define FBX_REV_XOR 2
#define FBX_REV_ANDXOR 3
#define FBX_REV_XIN 4

/* fbx_reversible_sample_shots: the circuit words[G] on |0..0>, run for B items (noise) x P units (input words) x n_shots shots,
 * followed by a Z measurement of the m qubits out_qubits[m] (uint8, m in 1..64; column j of a record is qubit out_qubits[j]).
 * noise_class [G] uint8: a class < K, 1 <= K <= 16, or FBX_DFE_NOISELESS; NULL = every gate is class 0.  inputs [P] uint64: the
 * input word of unit r, read by XIN.  class_error [B][K] or NULL (= 0).  readout_flip [B][m][2] or NULL, per record column:
 * [j][0] = P(read 1 | drawn 0), [j][1] = P(read 0 | drawn 1).  expected [P] uint64 or NULL: the expected record of unit r, packed
 * in record-column order (bit j = column j).  Unit r is the global input index first_input + r, item b the global item
 * first_item + b.  Outputs, each may be NULL, not all of the first three:
 *   bits_out      [B][P][n_shots][m] uint8 0 / 1 -- for one item the layout of get_n_bit_adder_results;
 *   words_out     [B][P][n_shots] uint64, the same record packed, bit j = column j;
 *   weight_counts [B][P][m + 1] int64: entry w = the number of shots whose record differs from expected[r] in w columns (the
 *                 weight-kind histogram of fbx_bit_histogram over bits_out, exactly); needs expected; zeroed by the call;
 *   status_out    [B]: 0 good, 1 poisoned.
 *
 * THE MODEL.  A Pauli error flips the bit of a qubit iff it has an X part (X, Y) on a qubit that holds its bit in Z or a Z part
 * (Y, Z) on a qubit that holds it in X; every other part is a phase that the final Z measurement never sees.  After a gate of
 * class c, item b applies the depolarizing channel of fbx_clifford_sample_shots to the gate's k qubits: with probability
 * class_error[b][c] a Pauli drawn uniformly from ALL 4^k Paulis, the identity included.  Under this noise the shots are exact
 * samples of the circuit's outcome distribution.
 *
 * THE STREAM (part of the contract: it is what a host check restates).  Shot s of unit R = first_input + r of item
 * g = first_item + b owns the Philox4x32-10 blocks with counter (g, R, s, j) and key (seed low ^ 0x52565253, seed high), words
 * x0 .. x3 each; g and R are below 2^32.
 *   Block l >> 1:  gate l, words (x0, x1) for even l and (x2, x3) for odd l.  A gate that exists and whose class is not
 *                  FBX_DFE_NOISELESS errs iff (double) x_first * 2^-32 < class_error[b][c]; the Pauli index is then
 *                  x_second >> (32 - 2 k): operand i has the Pauli (index >> 2 (k - 1 - i)) & 3; 0 I, 1 X, 2 Y, 3 Z.
 *   Readout:       with J = (G + 1) >> 1, column j reads word j & 3 of block J + (j >> 2) and flips iff
 *                  (double) x * 2^-32 < readout_flip[b][j][d], d the drawn bit of the column.
 * Only the blocks that are needed are computed.  A record depends on (seed, g, R, s), the circuit and its item's noise only: not
 * on B, P, n_shots or the launch shape.
 *
 * n_qubits or m outside 1..64, K outside 1..16, G >= 2^31, n_shots >= 2^32, a negative size or first index, first_item + B or
 * first_input + P above 2^32, 2^31 or more workgroups (of four units of 64 shots: B * P * ceil(n_shots / 64) / 4), a NULL words (G > 0), inputs (P > 0) or
 * out_qubits, weight_counts without expected, bits_out, words_out and weight_counts all NULL: FBX_ERR_BAD_ARG before any buffer is
 * touched.  B, P or n_shots of 0: nothing is done.  A poisoned item -- a class error or a flip outside [0, 1], or NaN -- gets
 * status 1, records of zeros and counts of zero; its neighbours are untouched.  The host form also refuses an invalid word (an
 * unknown micro-op, k not that of the micro-op, an operand that is not below n_qubits or repeats, a set bit in an unused field),
 * an invalid class and an out_qubits entry that is not below n_qubits; the _dev form takes them as validated (qubit indices are
 * six bits: no access depends on a word's content), enqueues on the calling thread's stream and does not synchronise. */
int fbx_reversible_sample_shots(int n_qubits, int64_t G, const uint32_t* words, const uint8_t* noise_class, int K, int64_t P,
                                const uint64_t* inputs, int m, const uint8_t* out_qubits, const uint64_t* expected, int64_t B,
                                int64_t n_shots, const double* class_error, const double* readout_flip, uint64_t seed,
                                int64_t first_item, int64_t first_input, uint8_t* bits_out, uint64_t* words_out,
                                int64_t* weight_counts, int32_t* status_out);
int fbx_reversible_sample_shots_dev(int n_qubits, int64_t G, const uint32_t* d_words, const uint8_t* d_noise_class, int K, int64_t P,
                                    const uint64_t* d_inputs, int m, const uint8_t* d_out_qubits, const uint64_t* d_expected,
                                    int64_t B, int64_t n_shots, const double* d_class_error, const double* d_readout_flip,
                                    uint64_t seed, int64_t first_item, int64_t first_input, uint8_t* d_bits_out,
                                    uint64_t* d_words_out, int64_t* d_weight_counts, int32_t* d_status_out);

/* ---------------------------------------------------------------- circuits of native gates on a state vector, 1..13 qubits
 * A circuit as the hardware runs it -- compiled to I, RX, RZ, CZ and XY (fbx.compilation.basic_compile, the reference's
 * compilation.py) -- on a state vector, with a Pauli error after every native gate (csrc/fbx_native.hip).  This
 * is the simulator under the Toffoli's decomposition, which is neither Clifford nor classical.  Amplitude index i has qubit 0 as
 * its MOST significant bit, as fbx_qv_heavy_outputs.
 *
 * THE WORD (uint32):
 *   bits  0..2   opcode, FBX_NAT_*
 *   bits  3..6   q0
 *   bits  7..10  q1 of CZ and XY, different from q0 (0 for the one-qubit gates)
 *   bit   11     1: the gate is conditional
 *   bits 12..17  a conditional gate: the bit of the unit's input word that decides whether the gate -- its error site included --
 *                exists (0 otherwise)
 *   bits 18..31  0
 * angles [G] float64 holds the angle of RX, RZ and XY, and 0 for I and CZ (it is not read for them, but must be finite):
 *   FBX_NAT_I    nothing: an error site only
 *   FBX_NAT_RX   [[cos a/2, -i sin a/2], [-i sin a/2, cos a/2]], any finite angle
 *   FBX_NAT_RZ   diag(exp(-i a/2), exp(i a/2))
 *   FBX_NAT_CZ   diag(1, 1, 1, -1)
 *   FBX_NAT_XY   1 (+) [[cos a/2, i sin a/2], [i sin a/2, cos a/2]] (+) 1 on |00>, (|01>, |10>), |11> */
#define FBX_NAT_I 0
#define FBX_NAT_RX 1
#define FBX_NAT_RZ 2
#define FBX_NAT_CZ 3
#define FBX_NAT_XY 4
/* the largest width at which one wavefront runs a trajectory; above it a workgroup does (tests straddle it) */
#define FBX_NAT_WAVE_MAX_QUBITS 8

/* fbx_native_trajectories: the circuit words[G], angles[G] on |0..0>, run for B items (noise) x P units (input words) x T
 * stochastic Pauli-error trajectories.  noise_class [G] uint8: a class < K, 1 <= K <= 16, or FBX_DFE_NOISELESS; NULL = every gate
 * is class 0.  inputs [P] uint64: the input word of unit r, read by the conditional gates.  class_error [B][K] or NULL (= 0).
 * out_qubits [m] uint8, 1 <= m <= n_qubits, all different.  Unit r is the global input index first_input + r, item b the global
 * item first_item + b.  Outputs, not both of the first two NULL:
 *   probs_mean_out [B][P][2^m]  the mean over the T trajectories of the outcome distribution of the m qubits out_qubits: column c of
 *                               out_qubits is bit m - 1 - c of the index (column 0 the most significant), so a row feeds
 *                               fbx_sample_bitstrings_dev directly; m = n_qubits with out_qubits = 0 .. n - 1 is the full distribution;
 *   n_errors_out   [B][P][T]    int32: the gates of the trajectory that erred (a draw of the identity Pauli counts);
 *   status_out     [B]          0 good, 1 poisoned; may be NULL.
 *
 * THE MODEL is that of fbx_clifford_sample_shots and fbx_reversible_sample_shots.  After a gate that exists and whose class c is not
 * FBX_DFE_NOISELESS, with probability class_error[b][c], a Pauli drawn uniformly from ALL 4^k Paulis of the gate's k qubits, the
 * identity included, is applied.  Only probabilities leave the kernel, so Y is applied as X Z (a global phase).
 *
 * THE STREAM (part of the contract: it is what a host check restates).  Trajectory t of unit R = first_input + r of item
 * g = first_item + b owns the Philox4x32-10 blocks with counter (g, R, t, j) and key (seed low ^ 0x4E415456, seed high) ("NATV"),
 * words x0 .. x3 each; g and R are below 2^32.  Block l >> 1 serves gate l: words (x0, x1) for even l and (x2, x3) for odd l.  A
 * gate errs iff (double) x_first * 2^-32 < class_error[b][c]; the Pauli index is then x_second >> (32 - 2 k): operand i (q0, q1)
 * has the Pauli (index >> 2 (k - 1 - i)) & 3; 0 I, 1 X, 2 Y, 3 Z.  Only the blocks that are needed are computed.  A trajectory
 * depends on (seed, g, R, t), the circuit and its item's noise only.
 *
 * THE MEAN is summed in an order that depends on T and n_qubits alone, without floating-point atomics: a trajectory's
 * probabilities |amplitude|^2 are added up over 8 consecutive trajectories in the order of t; an output of the marginal is the sum,
 * over its amplitudes in ascending index order, of each amplitude's partial sums in order, divided once by T.  An item repeats bit
 * for bit under another B, another P, another first_item / first_input offset and another "native_workspace_mib" (fbx_set_option).
 *
 * n_qubits outside 1..13: FBX_ERR_UNSUPPORTED, before any buffer is touched.  m outside 1..n_qubits, K outside 1..16, T >= 2^32,
 * G >= 2^31, a negative size or first index, first_item + B or first_input + P above 2^32, a NULL words or angles (G > 0), inputs
 * (P > 0) or out_qubits, both outputs NULL: FBX_ERR_BAD_ARG, before any buffer is touched.  B, P or T of 0: nothing is done.
 * G = 0 gives the distribution of |0..0>.  A poisoned item -- a class error outside [0, 1], or NaN -- gets status 1, NaN
 * probabilities and zero error counts; its neighbours are untouched.  The host form also refuses an invalid word (an unknown
 * opcode, a qubit that is not below n_qubits, q1 == q0 or a q1 of a one-qubit gate, a set bit in an unused field), a non-finite
 * angle, an invalid class and an out_qubits entry that repeats or is not below n_qubits.  The _dev form takes them as validated,
 * enqueues on the calling thread's stream and does not synchronise (growing the workspace does); it never indexes outside the
 * state or its workspace whatever the words hold: a gate whose qubits do not fit the width is skipped and, like a non-finite
 * angle, makes EVERY item poisoned, and with a bad out_qubits entry the probabilities are NaN. */
int fbx_native_trajectories(int n_qubits, int64_t G, const uint32_t* words, const double* angles, const uint8_t* noise_class, int K,
                            int64_t P, const uint64_t* inputs, int m, const uint8_t* out_qubits, int64_t B, int64_t T,
                            const double* class_error, uint64_t seed, int64_t first_item, int64_t first_input,
                            double* probs_mean_out, int32_t* n_errors_out, int32_t* status_out);
int fbx_native_trajectories_dev(int n_qubits, int64_t G, const uint32_t* d_words, const double* d_angles,
                                const uint8_t* d_noise_class, int K, int64_t P, const uint64_t* d_inputs, int m,
                                const uint8_t* d_out_qubits, int64_t B, int64_t T, const double* d_class_error, uint64_t seed,
                                int64_t first_item, int64_t first_input, double* d_probs_mean_out, int32_t* d_n_errors_out,
                                int32_t* d_status_out);

/* The unitary of a circuit of native gates, U_out [2^n][2^n] complex128 row-major: column j is the circuit applied to basis state j,
 * through the gate loop of fbx_native_trajectories without noise.  Rows and columns are indexed as pyquil's program_unitary (and
 * fbx.compilation.program_unitary) does: qubit 0 is the LEAST significant bit.  n_qubits 1..13 (others FBX_ERR_UNSUPPORTED); the
 * buffer is the caller's (16 * 4^n bytes).  The host form refuses invalid words, non-finite angles and conditional gates
 * (FBX_ERR_BAD_ARG); in the _dev form a conditional gate does not exist, and a column is NaN where a gate does not fit the width
 * or an angle is not finite. */
int fbx_native_unitary(int n_qubits, int64_t G, const uint32_t* words, const double* angles, double* U_out);
int fbx_native_unitary_dev(int n_qubits, int64_t G, const uint32_t* d_words, const double* d_angles, double* d_U_out);

/* out[b] = op(a[b]) diag(scale[b]) op(b[b]) for stacks of N x N complex matrices, N in 1..1024: op = the matrix itself
 * (conj_t = 0) or its conjugate transpose (conj_t = 1); scale is [B][N] real or NULL.  The products around fbx_eigh:
 * V f(lambda) V^H (sqrtm_psd, calculational.py:77-91), sqrt(rho) sigma sqrt(rho) (fidelity, distance_measures.py:64-84). */
int fbx_matmul(int N, int64_t B, const double* a, int conj_t_a, const double* scale, const double* b, int conj_t_b,
               double* out);
int fbx_matmul_dev(int N, int64_t B, const double* d_a, int conj_t_a, const double* d_scale, const double* d_b,
                   int conj_t_b, double* d_out);

/* partial_trace (calculational.py:5-35) of operators on A (x) B, any dimensions with dim_a * dim_b <= 4096:
 * keep = 0 traces out B (out [B][dim_a][dim_a]), keep = 1 traces out A (out [B][dim_b][dim_b]); in is
 * [B][dim_a dim_b][dim_a dim_b].  Tr_out of a Choi matrix (trace preservation, validate_superoperator.py:80-97)
 * is keep = 0 with dim_a = dim_b = d; its action on the identity (unitality, :130-145) is keep = 1. */
int fbx_partial_trace(int dim_a, int dim_b, int keep, int64_t B, const double* in, double* out);
int fbx_partial_trace_dev(int dim_a, int dim_b, int keep, int64_t B, const double* d_in, double* d_out);

/* Batched Hermitian eigendecomposition with numpy.linalg.eigh / scipy.linalg.eigh semantics (the
 * LOWER triangle of a[B][N][N] is read, eigenvalues ascending).  The host form takes any N in 1..1024
 * (up to 64: in LDS, sizes that are not a power of two -- a qutrit, a 9 x 9 Choi matrix -- embedded in the
 * next power of two with decoupled zero padding; above 64: the same Jacobi with matrix and eigenvectors in
 * HBM -- one workgroup per matrix for batches, a cooperative launch over the whole chip for a few matrices; 4- and
 * 5-qubit Choi matrices, not a fast path: 25 ms for 256 x 256, 0.8 s for 1024 x 1024); the _dev form N in
 * {2, 4, 8, 16, 32, 64} or even in 66..1024.  This is the
 * primitive under choi2kraus (superoperator_transformations.py:325-336), the PSD validators
 * (validate_operator.py:118-150), proj_choi_to_unitary (project_superoperators.py:147-175),
 * sqrtm_psd (calculational.py:77-91) and the spectral distance measures (distance_measures.py:153-195,440-460).
 * w_out[B][N]; v_out[B][N][N] holds the eigenvectors as columns (phases arbitrary), may be NULL.
 * Supported magnitudes: entries (and gaps that matter) between about 1e-150 and 1e+150 -- beyond that squares under- or
 * overflow in the rotations and the stopping test (off-norm^2 <= 1e-26 norm^2), and smaller entries count as zero.
 * Non-finite input: an item with a NaN or Inf on its diagonal (real part) or in its strictly lower triangle returns all-NaN
 * w and all-NaN v; every other item of the batch is bit-identical to what it is beside a finite item, and the call returns
 * FBX_OK.  This holds for both forms, at every N (padded sizes included) and from either large-N kernel.  The strictly
 * upper triangle and the diagonal's imaginary parts are never read: NaN or Inf there changes nothing. */
int fbx_eigh(int N, int64_t B, const double* a, double* w_out, double* v_out);
int fbx_eigh_dev(int N, int64_t B, const double* d_a, double* d_w_out, double* d_v_out);

/* choi2kraus (superoperator_transformations.py:325-336) for a batch of n-qubit Choi matrices, n in 1..5 (D = 4^n, d = 2^n):
 * kraus_out[B][D][d][d] complex128, row-major d x d operators; operator i of an item is sqrt(lambda_i) unvec(v_i) for the
 * i-th eigenpair with |lambda_i| > tol in ascending eigenvalue order (the order of the reference's list; numpy's scimath
 * square root: i sqrt(|lambda|) for a negative eigenvalue), the remaining slots are zero; count_out[B] (may be NULL) = the
 * number of operators kept.  Kraus operators are defined up to the phase of each eigenvector: it is fixed so that the
 * eigenvector's first component above 1e-12 of its norm is real and positive -- the convention under which the reference's
 * entry-by-entry tests hold (tests/test_superoperator_transformations.py:215-216); compare |K| or kraus2choi(K) otherwise,
 * as :219-224, :263-271 do.  Also the tail of superop2kraus (:229-238), pauli_liouville2kraus (:280-288) and chi2kraus
 * (:195-204): fbx_convert to Choi first.  fbx_eigh + one assembling kernel; the result may alias nothing. */
int fbx_choi2kraus(int n_qubits, int64_t B, const double* choi, double tol, double* kraus_out, int32_t* count_out);
int fbx_choi2kraus_dev(int n_qubits, int64_t B, const double* d_choi, double tol, double* d_kraus_out, int32_t* d_count_out);

#ifdef __cplusplus
}
#endif
#endif /* FBX_H */
