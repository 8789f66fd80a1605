"""Bit-for-bit comparison of two builds of the library on the same inputs: PGDB (2 qubits on both kernels, 1 and 3 qubits -- both
in-bases -- and the 3-qubit _cost / _grad_cost), the
state estimators and measures for 1-5 qubits incl. designs of more than 64 settings, Choi projections, every conversion route and
Kraus sweep kernel (both forms of the 3-qubit ones, batches past the persistent grid, Kraus counts on either side of each kernel
switch), the Kraus-pair / twirl / partial-trace / apply / fidelity / linear-inversion entry points, and fbx_eigh / fbx_matmul /
fbx_choi2kraus at every size class, and the simulated acquisitions (tomography plain / grouped / symmetrized / calibration, DFE,
RPE) on both of their work splits, and the four readers of shot records (shots to moments, bit histograms, RPE from shots, QV heavy
counts) on both of their teams, host form and _dev form at a 1-byte offset.
usage: python scripts/compare_libs.py libA.so libB.so      (names inside forest-benchmarking_amd/; FBX_LIBRARY selects each build)"""
import os, subprocess, sys, hashlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, os, hashlib
sys.path.insert(0, os.path.join(sys.argv[1], "forest-benchmarking_amd"))
import numpy as np
from fbx import synthetic, tomography, _lib
_lib.set_device(0)
out = []
for n, basis, B, kw in ((2, "pauli", 256, dict(mode="fixed", max_iters=100)), (2, "pauli", 2304, {}), (2, "sic", 64, {}), (1, "pauli", 32, {}),
                        (3, "sic", 4, dict(mode="fixed", max_iters=12)), (3, "pauli", 2, dict(mode="fixed", max_iters=6))):
    design, _, e, c = synthetic.process_batch(n, basis, min(B, 256))
    if B > 256:
        e = np.tile(e, (B // 256, 1)); c = np.tile(c, (B // 256, 1))
    choi, st = tomography.pgdb_process_estimate_batch(design, e, c, return_stats=True, **kw)
    h = hashlib.sha256(np.ascontiguousarray(choi).tobytes())
    for k in ("iterations", "dykstra", "backtracks"):
        h.update(np.ascontiguousarray(st[k]).tobytes())
    out.append(h.hexdigest()[:16])
# 3-qubit _cost / _grad_cost (pgdb3_cost_grad_kernel) at estimates three iterations in
design, _, e, c = synthetic.process_batch(3, "sic", 2)
est = tomography.pgdb_process_estimate_batch(design, e, c, mode="fixed", max_iters=3)
cost, grad = tomography.cost_and_gradient_batch(design, tomography.normalised_counts(e, c), est)
out.append(hashlib.sha256(np.ascontiguousarray(cost).tobytes() + np.ascontiguousarray(grad).tobytes()).hexdigest()[:16])
# everything else that shares the touched headers: state MLE, Choi projections, conversions (incl. the eigh routes), the sweeps
import warnings
warnings.simplefilter("ignore")
def H(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]
from fbx.operator_tools import project_superoperators as ps, superoperator_transformations as st_
from fbx.operator_tools import project_state_matrix as psm
for n, B in ((1, 64), (2, 64), (3, 16)):
    design, _, e, c = synthetic.state_batch(n, B, mixed=0.05)
    out.append(H(tomography.iterative_mle_state_estimate_batch(design, e, c, maxiter=60)))
    out.append(H(tomography.iterative_mle_state_estimate_batch(design, e, c, maxiter=30, beta=0.5)))
rs = np.random.RandomState(3)
for n, B in ((1, 16), (2, 16), (3, 4)):
    D = 4 ** n
    x = rs.randn(B, D, D) + 1j * rs.randn(B, D, D)
    x = x + x.conj().transpose(0, 2, 1) + np.eye(D) * 2
    for kind in range(4):
        out.append(H(*ps.proj_choi_batch(kind, x, return_iters=True)))
    out.append(H(st_.convert_batch("choi", "chi", x)))
    out.append(H(st_.convert_batch("choi", "pauli_liouville", x)))
    k = synthetic.kraus_batch(n, 4, B, seed=5)
    out.append(H(st_.convert_batch("kraus", "chi", k)))
    out.append(H(psm.project_state_matrix_to_physical_batch(x[:, :2 ** n, :2 ** n])))
lib = _lib.lib()
for n, B in ((2, 1001), (3, 33)):
    K, D = 4, 4 ** n
    k = np.ascontiguousarray(synthetic.kraus_batch(n, K, B, seed=9))
    ref = np.ascontiguousarray(st_.convert_batch("kraus", "pauli_liouville", k[:1])[0])
    choi, ptm, chi = (np.empty((B, D, D), dtype=np.complex128) for _ in range(3))
    fid = np.empty(B)
    _lib.check(lib.fbx_kraus_sweep(n, B, K, _lib.dptr(k.view(np.float64)), _lib.dptr(ref.view(np.float64)), _lib.dptr(choi.view(np.float64)),
                                   _lib.dptr(ptm.view(np.float64)), _lib.dptr(chi.view(np.float64)), _lib.dptr(fid)))
    out.append(H(choi, ptm, chi, fid))
# the state path entry point by entry point (1-5 qubits; designs of 66-126 settings: the staged R operator, 4200: the streamed one)
# and the general linear algebra of csrc/fbx_linalg.hip
from fbx import design as fd, distance_measures as dm
def rand_states(B, d, seed):
    r = np.random.RandomState(seed)
    a = r.randn(B, d, d) + 1j * r.randn(B, d, d)
    a = a @ a.conj().transpose(0, 2, 1)
    return a / np.trace(a, axis1=1, axis2=2)[:, None, None]
def state_calls(design, e, c, rho, mle_kws):
    for kw in mle_kws:
        out.append(H(tomography.iterative_mle_state_estimate_batch(design, e, c, **kw)))
    out.append(H(tomography._R_batch(rho, design, e)))
    out.append(H(tomography.state_log_likelihood_batch(rho, design, e, c)))
    out.append(H(tomography.linear_inv_state_estimate_batch(design, e)))
def measures(rho, sig):
    m = dm.state_measures_batch(rho, sig)
    out.append(H(*[m[k] for k in ("purity", "fidelity", "trace_distance", "hs_ip")]))
for n, B in ((1, 64), (2, 64), (3, 16)):
    design, _, e, c = synthetic.state_batch(n, B, mixed=0.05)
    state_calls(design, e, c, rand_states(B, 2 ** n, 11 + n), (dict(maxiter=30, entropy_penalty=0.005),))
    measures(rand_states(B, 2 ** n, 21 + n), rand_states(B, 2 ** n, 31 + n))
design, _, e, c = synthetic.state_batch(4, 2, mixed=0.05)
state_calls(design, e, c, rand_states(2, 16, 15), (dict(maxiter=8), dict(maxiter=8, beta=0.5), dict(maxiter=8, entropy_penalty=0.005)))
out.append(H(psm.project_state_matrix_to_physical_batch(rs.randn(2, 16, 16) + 1j * rs.randn(2, 16, 16) + np.eye(16))))
measures(rand_states(2, 16, 25), rand_states(2, 16, 35))
design, _, e, c = synthetic.state_batch(5, 1, mixed=0.05)                  # 5 qubits: one item through the workgroup kernels
out.append(H(tomography.iterative_mle_state_estimate_batch(design, e, c, maxiter=3)))
r5 = np.random.RandomState(5)
out.append(H(psm.project_state_matrix_to_physical_batch(r5.randn(1, 32, 32) + 1j * r5.randn(1, 32, 32) + np.eye(32))))
measures(rand_states(1, 32, 26), rand_states(1, 32, 36))
variants = (dict(maxiter=40), dict(beta=0.5, epsilon=1e-4, maxiter=12), dict(entropy_penalty=0.005, maxiter=12))
for n, reps in ((1, 22), (2, 5), (3, 2)):
    p = np.tile(fd.traceless_pauli_codes(n), (reps, 1))
    design = fd.Design(n, "state", None, p)
    e = np.random.RandomState(40 + n).uniform(-0.6, 0.6, (4, design.m))
    state_calls(design, e, np.full(e.shape, 500.0), rand_states(4, 2 ** n, 41 + n), variants)
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "repeated.npz"))
state_calls(fd.Design(1, "state", None, g["s1_paulis"]), g["s1_e"], g["s1_c"], g["s1_mle40"], variants[:2])
for N in (2, 4, 8, 16, 32, 64, 66, 130, 3):
    a = rs.randn(3, N, N) + 1j * rs.randn(3, N, N)
    out.append(H(*_lib.eigh_batch(a), _lib.eigh_batch(a, eigenvectors=False)))
for N in (5, 33):
    a, b, sc = rs.randn(3, N, N) + 1j * rs.randn(3, N, N), rs.randn(3, N, N) + 1j * rs.randn(3, N, N), rs.randn(3, N)
    out.append(H(*[_lib.matmul_batch(a, b, conj_t_a=ta, conj_t_b=tb, scale=sc) for ta in (False, True) for tb in (False, True)]))
for n in (1, 2):
    choi = st_.convert_batch("kraus", "choi", synthetic.kraus_batch(n, 3, 8, seed=7))
    out.append(H(*st_.choi2kraus_batch(choi)))
# csrc/fbx_convert.hip, fbx_sweep.hip, fbx_superop.hip route by route: arbitrary complex matrices where the route is linear,
# Hermitian non-PSD ones into chi (the |C| step)
from fbx.operator_tools import compose_superoperators as cs, channel_approximation as ca, calculational as calc, apply_superoperator as ap
REPS = ("choi", "superop", "pauli_liouville", "chi")
PL_ROUTES = (("choi", "pauli_liouville"), ("superop", "pauli_liouville"), ("pauli_liouville", "choi"), ("pauli_liouville", "superop"))
def mats(B, D, seed):
    r = np.random.RandomState(seed)
    x = r.randn(B, D, D) + 1j * r.randn(B, D, D)
    return x, x + x.conj().transpose(0, 2, 1)
def sweep(n, K, B, seed):
    D = 4 ** n
    k = np.ascontiguousarray(synthetic.kraus_batch(n, K, min(B, 8), seed=seed)[np.arange(B) % min(B, 8)])
    ref = np.ascontiguousarray(st_.convert_batch("kraus", "pauli_liouville", synthetic.kraus_batch(n, 1, 1, seed=99))[0])
    choi, ptm, chi = (np.empty((B, D, D), dtype=np.complex128) for _ in range(3))
    fid = np.empty(B)
    _lib.check(lib.fbx_kraus_sweep(n, B, K, _lib.dptr(k.view(np.float64)), _lib.dptr(ref.view(np.float64)), _lib.dptr(choi.view(np.float64)),
                                   _lib.dptr(ptm.view(np.float64)), _lib.dptr(chi.view(np.float64)), _lib.dptr(fid)))
    out.append(H(choi, ptm, chi, fid))
for n in (1, 2, 3):
    x, h = mats(5, 4 ** n, 50 + n)
    k = synthetic.kraus_batch(n, 3, 5, seed=6)
    out.append(H(*[st_.convert_batch("kraus", dst, k) for dst in ("superop",) + REPS]))
    for src in REPS:
        out.append(H(*[st_.convert_batch(src, dst, h if dst == "chi" else x) for dst in REPS if dst != src]))
x, h = mats(2049, 64, 54)                                  # past the persistent grid of the 3-qubit register kernels
out.append(H(*[st_.convert_batch(src, dst, x) for src, dst in PL_ROUTES]))
sweep(3, 4, 2049, 8)
os.environ["FBX_CONVERT3_V1"] = os.environ["FBX_SWEEP3_V1"] = "1"      # the first forms of the 3-qubit kernels
out.append(H(*[st_.convert_batch(src, dst, x[:5]) for src, dst in PL_ROUTES]))
out.append(H(*[st_.convert_batch("kraus", dst, synthetic.kraus_batch(3, 3, 5, seed=6)) for dst in REPS]))
sweep(3, 4, 33, 9)
del os.environ["FBX_CONVERT3_V1"], os.environ["FBX_SWEEP3_V1"]
x, h = mats(2, 256, 55)
k = synthetic.kraus_batch(4, 3, 2, seed=6)
out.append(H(*[st_.convert_batch("kraus", dst, k) for dst in REPS]))
out.append(H(*[st_.convert_batch(src, dst, x) for src in REPS for dst in REPS[:3] if dst != src], st_.convert_batch("choi", "chi", h)))
k = rs.randn(5, 3, 3, 3) + 1j * rs.randn(5, 3, 3, 3)     # qutrits: the basis-free kernel
sup = st_.convert_batch("kraus", "superop", k)
out.append(H(sup, st_.convert_batch("kraus", "choi", k), st_.convert_batch("superop", "choi", sup), st_.convert_batch("choi", "superop", sup)))
for n, K in ((2, 16), (2, 17), (3, 15), (3, 16)):           # either side of the pair kernel / of the composed form
    sweep(n, K, 3, 100 * n + K)
out.append(H(*[st_.convert_batch("kraus", dst, synthetic.kraus_batch(3, 40, 2, seed=340)) for dst in REPS[:1] + REPS[2:]]))   # past every LDS staging
k2, k1 = rs.randn(4, 3, 4, 4) + 1j * rs.randn(4, 3, 4, 4), rs.randn(4, 2, 4, 4) + 1j * rs.randn(4, 2, 4, 4)
x, h = mats(6, 16, 56)
out.append(H(cs.tensor_channel_kraus_batch(k2, k1), cs.compose_channel_kraus_batch(k2, k1), ca.pauli_twirl_chi_matrix_batch(x),
             calc.partial_trace_bipartite_batch(x, 2, 8, 0), calc.partial_trace_bipartite_batch(x, 2, 8, 1),
             ap.apply_choi_matrix_2_state_batch(x, rand_states(6, 4, 57)), dm.process_fidelity_batch(x[:1], h), dm.process_fidelity_batch(x, h, entanglement=True)))
for n in (1, 2):
    design, _, e, c = synthetic.process_batch(n, "pauli", 9)
    out.append(H(tomography.linear_inv_process_estimate_batch(design, e)))
# the simulated acquisitions (csrc/fbx_sim_shared.hpp and its five users), one hash per entry point and work split: the smallest
# design at B = 3 (a wavefront per unit) and at the batch that reaches 131072 units (a lane per unit), 37 shots (nine Philox blocks
# and a tail of one), without and with readout noise, and with item 1 poisoned; every output array goes into the hash
from fbx import direct_fidelity_estimation as dfe, robust_phase_estimation as rpe
LANE = 131072
def unitaries(B, d, seed):
    r = np.random.RandomState(seed)
    return np.linalg.qr(r.randn(B, d, d) + 1j * r.randn(B, d, d))[0]
def poisoned(x):
    x = np.array(x); x[(1,) + (0,) * (x.ndim - 1)] = np.nan
    return x
def noises(make):                     # without noise, with noise, with noise and a poisoned item
    return (dict(noise=None), dict(noise=make()), dict(noise=make(), poison=True))
def sim_hash(call, truth, noise_kw, make_noise):
    parts = []
    for v in noises(make_noise):
        t = poisoned(truth) if v.get("poison") else truth
        parts += list(call(t, **{noise_kw: v["noise"]}, seed=77, first_item=3, return_status=True))
    out.append(H(*parts))
ALL = dict(return_std_errs=True, return_exact=True)
GROUPED = dict(ALL, return_probabilities=True, return_histograms=True)
sic1, st4, st2 = fd.process_design(1, "sic"), fd.state_design(4), fd.state_design(2)
def confusion(B, d, seed):
    r = np.random.RandomState(seed).uniform(0, 1, (B, d, d)) ** 3
    return 0.875 * np.eye(d)[None] + 0.125 * r / r.sum(axis=2, keepdims=True)
for B in (3, LANE // sic1.m + 1):
    flips = lambda: np.random.RandomState(60).uniform(0, 0.2, (B, 1, 2))
    sim_hash(lambda t, **kw: tomography.simulate_process_tomography_batch(sic1, t, 37, rep="unitary", **ALL, **kw),
             unitaries(B, 2, 61), "readout_flip", flips)
    sim_hash(lambda t, **kw: tomography.simulate_grouped_process_tomography_batch(sic1, t, 37, rep="unitary", **GROUPED, **kw),
             unitaries(B, 2, 62), "readout_flip", flips)
sim_hash(lambda t, **kw: tomography.simulate_grouped_state_tomography_batch(st4, t, 37, **GROUPED, **kw), rand_states(3, 16, 63),
         "readout_flip", lambda: np.random.RandomState(64).uniform(0, 0.2, (3, 4, 2)))             # the LDS counters
for symm in (-1, 0):                  # the symmetrized entry points: the product confusion matrix of no flips, then a correlated one
    for conf in (np.tile(np.eye(4), (3, 1, 1)), confusion(3, 4, 65)):
        out.append(H(*tomography.simulate_symmetrized_state_tomography_batch(st2, rand_states(3, 4, 66), 37, conf, symm, seed=77,
                                                                             first_item=3, return_status=True, **GROUPED),
                     *tomography.simulate_symmetrized_state_tomography_batch(st2, poisoned(rand_states(3, 4, 66)), 37, conf, symm,
                                                                             seed=77, first_item=3, return_status=True, **GROUPED),
                     *tomography.simulate_readout_calibration_batch(st2, conf, 37, symm, seed=77, first_item=3, return_exact=True,
                                                                    return_status=True),
                     *tomography.simulate_readout_calibration_batch(st2, poisoned(conf), 37, symm, seed=77, first_item=3,
                                                                    return_exact=True, return_status=True)))
expt = dfe.generate_exhaustive_state_dfe_experiment(None, [("H", (0,)), ("S", (0,)), ("H", (0,))], [0])
for B in (3, LANE // expt.m):
    for calibrate in (False, True):
        sim_hash(lambda p, **kw: dfe.simulate_dfe_batch(expt, p, 37, calibrate=calibrate, **ALL, **kw),
                 np.random.RandomState(67).uniform(0, 0.1, (B, 1)), "readout_flip", lambda: np.random.RandomState(68).uniform(0, 0.3, (B, 1)))
for B in (3, LANE // 2):
    ang = np.random.RandomState(69).uniform(0, 6.28, B)
    gate = np.zeros((B, 4, 4)); gate[:, 0, 0] = gate[:, 3, 3] = 1.0
    gate[:, 1, 1] = gate[:, 2, 2] = 0.9 * np.cos(ang); gate[:, 2, 1] = 0.9 * np.sin(ang); gate[:, 1, 2] = -gate[:, 2, 1]
    for records in (False, True):
        sim_hash(lambda g, **kw: rpe.simulate_rpe_batch(g, num_depths=1, num_shots=37, return_probabilities=True, return_histograms=True,
                                                        return_records=records, **kw),
                 gate, "flips", lambda: np.random.RandomState(70).uniform(0, 0.2, (B, 1, 2)))
# the four readers of shot records (fbx_shots, fbx_histogram, fbx_rpe, fbx_qvolume), one hash per entry point: records of 33 shots (a run
# and a tail, and for odd widths an odd number of bytes, so that later records start off the 16-byte grid and have a head), B = 3 (a
# workgroup per record) and B = 5 (a wavefront per record), the host form and the _dev form with the records 1 byte into their buffer
import ctypes as C
from fbx import quantum_volume as qv
U8, U64, I64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
rr = np.random.default_rng(16)
def u8(a): return a.ctypes.data_as(U8)
def shifted(a):                       # a device copy of a that starts 1 byte into its allocation
    buf = _lib.DeviceBuffer(a.nbytes + 16)
    _lib.check(lib.fbx_memcpy_h2d(buf.ptr.value + 1, a.ctypes.data, a.nbytes))
    return buf, buf.ptr.value + 1
def fetch(bufs_shapes, *inputs):       # the outputs as arrays; they and the inputs named are freed
    _lib.synchronize()
    arrays = [b.to_array(dt, shape) for b, dt, shape in bufs_shapes]
    for b in [b for b, _, _ in bufs_shapes] + list(inputs):
        b.free()
    return arrays
parts = {"shots": [], "hist": [], "rpe": [], "qv": []}
for B in (3, 5):
    for n in (2, 3, 9):
        bits = rr.integers(0, 256, size=(B, 33, n), dtype=np.uint8)
        mask = rr.integers(0, 2, size=(B, n), dtype=np.uint8); mask[0] = 0
        coefs = rr.uniform(-2, 2, B)
        d_bits, at = shifted(bits)
        d_mask, d_coefs = _lib.DeviceBuffer.from_array(mask), _lib.DeviceBuffer.from_array(coefs)
        for prior in (0, 1):
            mean, var = np.empty(B), np.empty(B)
            _lib.check(lib.fbx_shots_to_moments(n, B, 33, u8(bits), u8(mask), _lib.dptr(coefs), prior, _lib.dptr(mean), _lib.dptr(var)))
            d_mean, d_var = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 8)
            _lib.check(lib.fbx_shots_to_moments_dev(n, B, 33, at, d_mask.ptr, d_coefs.ptr, prior, d_mean.ptr, d_var.ptr))
            parts["shots"] += [mean, var] + fetch([(d_mean, np.float64, (B,)), (d_var, np.float64, (B,))])
        for b in (d_bits, d_mask, d_coefs):
            b.free()
    for n in (1, 3, 11):
        bits = rr.integers(0, 256, size=(B, 33, n), dtype=np.uint8)
        k = min(n, 10)
        for kind in (0, 1):
            bins = (1 << k) if kind == 0 else k + 1
            counts = np.empty((B, bins), dtype=np.int64)
            _lib.check(lib.fbx_bit_histogram(n, B, 33, u8(bits), k, None, 1, None, kind, counts.ctypes.data_as(I64)))
            d_bits, at = shifted(bits)
            d_counts = _lib.DeviceBuffer(B * bins * 8)
            _lib.check(lib.fbx_bit_histogram_dev(n, B, 33, at, k, None, 1, None, kind, d_counts.ptr))
            parts["hist"] += [counts] + fetch([(d_counts, np.int64, (B, bins))], d_bits)
    for n, col, zcol in ((1, 0, -1), (3, 2, 0), (8, 0, 7)):
        xb, yb = rr.integers(0, 256, size=(B, 2, 33, n), dtype=np.uint8), rr.integers(0, 256, size=(B, 2, 33, n), dtype=np.uint8)
        phase, depth, bloch, mom = np.empty(B), np.empty(B, dtype=np.int32), np.empty((B, 2, 2)), np.empty((B, 2, 4))
        _lib.check(lib.fbx_rpe_from_shots(n, B, 2, 33, u8(xb), u8(yb), col, zcol, 1, _lib.dptr(phase), _lib.iptr(depth), _lib.dptr(bloch),
                                          _lib.dptr(mom)))
        (d_x, at_x), (d_y, at_y) = shifted(xb), shifted(yb)
        d_p, d_d, d_m = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 4), _lib.DeviceBuffer(B * 2 * 4 * 8)
        _lib.check(lib.fbx_rpe_from_shots_dev(n, B, 2, 33, at_x, at_y, col, zcol, 1, d_p.ptr, d_d.ptr, None, d_m.ptr))
        parts["rpe"] += [phase, depth, bloch, mom] + fetch([(d_p, np.float64, (B,)), (d_d, np.int32, (B,)), (d_m, np.float64, (B, 2, 4))],
                                                           d_x, d_y)
    for n in (2, 9):
        bits = rr.integers(0, 256, size=(B, 33, n), dtype=np.uint8)
        mask = qv.pack_heavy_mask(rr.integers(0, 2, size=(B, 1 << n)).astype(bool))
        counts = np.empty(B, dtype=np.int64)
        _lib.check(lib.fbx_qv_count_heavy(n, B, 33, u8(bits), mask.ctypes.data_as(U64), counts.ctypes.data_as(I64)))
        d_bits, at = shifted(bits)
        d_mask, d_counts = _lib.DeviceBuffer.from_array(mask), _lib.DeviceBuffer(B * 8)
        _lib.check(lib.fbx_qv_count_heavy_dev(n, B, 33, at, d_mask.ptr, d_counts.ptr))
        parts["qv"] += [counts] + fetch([(d_counts, np.int64, (B,))], d_bits, d_mask)
out += [H(*parts[k]) for k in ("shots", "hist", "rpe", "qv")]
print(" ".join(out))
'''
res = []
for lib in sys.argv[1:3]:
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, FBX_LIBRARY=os.path.join(ROOT, "forest-benchmarking_amd", lib)),
                       capture_output=True, text=True)
    print(f"{lib:24s} {r.stdout.strip()} {r.stderr.strip()[-300:]}")
    if r.returncode != 0:                     # a build that failed is not followed by another run on the same device
        sys.exit(f"{lib}: exit status {r.returncode}")
    res.append(r.stdout.strip())
print("IDENTICAL" if res[0] == res[1] and res[0] else "DIFFERENT")
