"""The Choi projections where ONE wavefront runs them (proj_choi_kernel, the one-wave PGDB kernels) request the operands of a
step together: the eigenvalue terms of the CP reconstruction three per trip with a pair / a single term left over, the
clamped eigenvalues from registers, the partial trace's entries in one go with `- I` folded into its store (csrc/fbx_choi.hpp,
csrc/fbx_eigh.hpp).  Every term count, both projection kinds and the kernels that carry the basis store, against the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _haar(D, rs):
    q, r = np.linalg.qr(rs.randn(D, D) + 1j * rs.randn(D, D))
    return q * (np.diag(r) / np.abs(np.diag(r)))


@pytest.mark.parametrize("n", [1, 2])
def test_cp_projection_every_term_count(gpu, n):
    """One matrix per r = 0 .. D with exactly r positive eigenvalues (|lambda| in [0.1, 1]), plus an anti-Hermitian part of
    norm ~0.1 that the Hermitisation has to remove: every number of whole trips and every leftover of the reconstruction.
    The zero matrix (no term: exactly zero) and the identity (D terms) ride along."""
    from fbx import _lib
    from fbx.operator_tools.project_superoperators import proj_choi_batch
    from fbx_oracle import superops as so
    D = 4 ** n
    rs = np.random.RandomState(100 + n)
    xs = []
    for r in range(D + 1):
        v = _haar(D, rs)
        lam = rs.uniform(0.1, 1.0, D) * np.where(np.arange(D) < r, 1.0, -1.0)
        lam = lam[rs.permutation(D)]
        h = (v * lam) @ v.conj().T
        a = rs.randn(D, D) + 1j * rs.randn(D, D)
        a = a - a.conj().T
        xs.append(h + 0.1 * a / np.linalg.norm(a))
        assert (np.linalg.eigvalsh((xs[-1] + xs[-1].conj().T) / 2) > 0).sum() == r
    xs += [np.zeros((D, D), dtype=complex), np.eye(D, dtype=complex)]
    xs = np.array(xs)
    got = proj_choi_batch(_lib.PROJ_CP, xs)
    want = np.array([so.proj_choi_to_completely_positive(x) for x in xs])
    err = np.abs(got - want).reshape(len(xs), -1).max(1)
    print("n", n, "max |err| per term count", err)
    assert err.max() < 1e-11
    assert not got[D + 1].any()                     # zero matrix: no term, exact zeros
    assert np.abs(got[D + 2] - np.eye(D)).max() < 1e-11


@pytest.mark.parametrize("n", [1, 2])
def test_tp_and_tni_projection(gpu, n):
    from fbx import _lib
    from fbx.operator_tools.project_superoperators import proj_choi_batch
    from fbx_oracle import superops as so
    d, D = 2 ** n, 4 ** n
    rs = np.random.RandomState(200 + n)
    xs = rs.randn(8, D, D) + 1j * rs.randn(8, D, D)
    tp = proj_choi_batch(_lib.PROJ_TP, xs)
    tni = proj_choi_batch(_lib.PROJ_TNI, xs)
    e_tp = np.abs(tp - np.array([so.proj_choi_to_trace_preserving(x) for x in xs])).max()
    e_tni = np.abs(tni - np.array([so.proj_choi_to_trace_non_increasing(x) for x in xs])).max()
    e_pt = max(np.abs(so.partial_trace(y, keep=[0], dims=[d, d]) - np.eye(d)).max() for y in tp)
    print("n", n, "TP", e_tp, "TNI", e_tni, "tr_out(TP) - I", e_pt)
    assert e_tp < 1e-12
    assert e_tni < 1e-11
    assert e_pt < 1e-13


@pytest.mark.parametrize("n", [1, 2])
def test_dykstra_both_kinds(gpu, n):
    from fbx import _lib
    from fbx.operator_tools.project_superoperators import proj_choi_batch
    from fbx_oracle import superops as so
    xs = np.load(os.path.join(GOLD, f"superops_{n}q.npz"))["proj_near_in"]
    for kind, tp in ((_lib.PROJ_PHYSICAL_TP, True), (_lib.PROJ_PHYSICAL_TNI, False)):
        got, iters = proj_choi_batch(kind, xs, return_iters=True)
        want = [so.proj_choi_to_physical(x, tp, return_iters=True) for x in xs]
        err = max(np.abs(g - w[0]).max() for g, w in zip(got, want))
        print("n", n, "TP" if tp else "TNI", "max |err|", err, "iterations", list(iters))
        assert err < 1e-10
        assert list(iters) == [w[1] for w in want]


@pytest.mark.parametrize("n,basis", [(2, "pauli"), (2, "sic"), (1, "pauli")])
def test_one_wave_pgdb_with_basis_store(gpu, n, basis):
    """Four reconstructions to convergence on the one-wave kernels: every projection of every outer iteration goes through the
    rebuilt loops, warm starts from the stored bases and their write-back included.  Tolerances and the halving comparison of
    tests/test_pgdb_gpu.py (halvings of the stalled last iteration are rounding-defined in the reference too)."""
    from fbx import synthetic, tomography
    from fbx_oracle import design as od, estimators as oe
    design, _, e, c = synthetic.process_batch(n, basis, 4)
    got, st = tomography.pgdb_process_estimate_batch(design, e, c, return_stats=True, trace_iters=256)
    o = od.Design(design.n_qubits, design.kind, design.in_labels, design.paulis, design.coefs)
    A = oe.design_matrix_A(o)
    for b in range(4):
        want, ws = oe.pgdb_process_estimate(o, e[b], c[b], A=A, return_stats=True)
        k = ws["iterations"]
        wtr = np.array(ws["trace"])
        print(n, basis, b, "max |err|", np.abs(got[b] - want).max(), "iterations", st["iterations"][b], k,
              "dykstra", st["dykstra"][b], ws["dykstra"], "halvings", st["backtracks"][b], ws["backtracks"])
        assert np.abs(got[b] - want).max() < 1e-9
        assert st["iterations"][b] == k
        assert st["dykstra"][b] == ws["dykstra"]
        assert np.array_equal(st["trace"][b, :k, 0], wtr[:, 0])
        assert np.array_equal(st["trace"][b, :k - 1, 1], wtr[:k - 1, 1])
