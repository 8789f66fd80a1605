"""The lean wave reductions of the one-wave PGDB kernels (csrc/fbx_common.hpp: wave_sum_lean -- bound_ctrl DPP levels, the row sums
through row_bcast:15 / row_bcast:31 and one readlane; wave_sum_n -- several sums level by level; wave_max_lean) take the same
tree on the same operands as wave_sum / wave_max.  libfbx_oldred.so is the same source with every one of them mapped back to
wave_sum / wave_max (-DFBX_WAVE_REDUCE_PARENT, build.py build_reductions_test): both builds must agree BIT FOR BIT on every
one-wave instantiation -- pgdb_kernel<1,1>, <1,4>, <2,4>, <2,9>, <2,16> -- trace preserving and not, 100 fixed iterations and to
convergence, three seeded items each: the Choi matrices as raw bits, the costs, the iteration / Dykstra / halving counts and the
four work counters.  A further call per instantiation has a NaN expectation in its middle item: both builds must end it (the
loops of tomography.py:542-594 and project_superoperators.py:87-144 restated with `!(x >= tol)` tests never spin on a NaN) and
report NaN in the same places."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "forest-benchmarking_amd")

# instantiation -> (qubits, number of settings taken from the Pauli design, repeating it from the start where it is shorter)
KERNELS = {"1_1": (1, 18), "1_4": (1, 90), "2_4": (2, 240), "2_9": (2, 540), "2_16": (2, 577)}
KEYS = ("iterations", "dykstra", "backtracks", "jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes")

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from fbx import synthetic, tomography, _lib
from fbx.design import Design
_lib.set_device(0)
KERNELS = {"1_1": (1, 18), "1_4": (1, 90), "2_4": (2, 240), "2_9": (2, 540), "2_16": (2, 577)}
KEYS = ("iterations", "dykstra", "backtracks", "jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes")
out = {}
def record(tag, design, e, c, **kw):
    choi, st = tomography.pgdb_process_estimate_batch(design, e, c, return_stats=True, **kw)
    out[tag + "/choi"] = np.ascontiguousarray(choi).view(np.float64).copy()
    out[tag + "/cost"] = np.array(st["cost"], dtype=np.float64)
    for k in KEYS:
        out[tag + "/" + k] = np.array(st[k], dtype=np.int32)
for name, (n, m) in KERNELS.items():
    base, _, e, c = synthetic.process_batch(n, "pauli", 3)
    assert base.m == (18 if n == 1 else 540), base.m
    idx = np.arange(m) % base.m
    design = Design(n, "process", base.in_labels[idx], base.paulis[idx], None)
    e, c = np.ascontiguousarray(e[:, idx]), np.ascontiguousarray(c[:, idx])
    for tp in (True, False):
        for mode, iters in (("fixed", 100), ("converge", 0)):
            record(f"{name}/tp{int(tp)}/{mode}", design, e, c, trace_preserving=tp, mode=mode, max_iters=iters)
    bad = e.copy()
    bad[1, m // 2] = np.nan
    record(f"{name}/nan/fixed", design, bad, c, trace_preserving=True, mode="fixed", max_iters=100)
    record(f"{name}/nan/converge", design, bad, c, trace_preserving=True, mode="converge", max_iters=0)
np.savez(sys.argv[2], **out)
"""


def _run(lib, out):
    env = dict(os.environ, FBX_LIBRARY=os.path.join(PKG, lib))
    subprocess.run([sys.executable, "-c", _CHILD, PKG, out], check=True, env=env, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def both(gpu, tmp_path_factory):
    assert os.path.exists(os.path.join(PKG, "libfbx_oldred.so")), "libfbx_oldred.so missing: run __graft_entry__.build()"
    tmp = tmp_path_factory.mktemp("reductions_ab")
    return _run("libfbx.so", str(tmp / "lean.npz")), _run("libfbx_oldred.so", str(tmp / "old.npz"))


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_lean_reductions_reproduce_wave_sum_bit_for_bit(both, kernel):
    new, old = both
    assert sorted(new) == sorted(old)
    tags = [f"{kernel}/tp{tp}/{mode}" for tp in (1, 0) for mode in ("fixed", "converge")]
    for tag in tags:
        for k in ("choi", "cost") + KEYS:
            a, b = new[f"{tag}/{k}"], old[f"{tag}/{k}"]
            assert a.shape == b.shape and a.dtype == b.dtype and a.shape[0] == 3, (tag, k)
            if a.dtype == np.float64:
                assert np.isfinite(a).all(), (tag, k)
                a, b = a.view(np.uint64), b.view(np.uint64)
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"{tag}/{k}: {len(bad)} of {a.size} entries differ, first at {bad[0].tolist()}"
        fixed = tag.endswith("fixed")
        assert (new[tag + "/iterations"] == 100).all() if fixed else (new[tag + "/iterations"] > 3).all(), tag
        # the converted reductions were exercised: Dykstra iterations (stop test, Jacobi sweeps), cost sums, power sums
        assert (new[tag + "/dykstra"] >= new[tag + "/iterations"]).all() and (new[tag + "/jacobi_sweeps"] > 0).all(), tag
        assert (new[tag + "/cost_evals"] > 0).all(), tag
    assert any((new[t + "/power_sum_passes"] > 0).any() for t in tags), kernel


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_nan_item_ends_and_reports_nan_in_the_same_places(both, kernel):
    new, old = both
    for mode in ("fixed", "converge"):
        tag = f"{kernel}/nan/{mode}"
        for k in ("choi", "cost"):
            a, b = new[f"{tag}/{k}"], old[f"{tag}/{k}"]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (tag, k)
            assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)), (tag, k)
        assert np.isnan(new[tag + "/cost"][1]) and np.isnan(new[tag + "/choi"][1]).any(), tag
        assert np.isfinite(new[tag + "/choi"][[0, 2]]).all() and np.isfinite(new[tag + "/cost"][[0, 2]]).all(), tag
        for k in KEYS:
            assert np.array_equal(new[f"{tag}/{k}"], old[f"{tag}/{k}"]), (tag, k)
        # the poisoned item ended by itself: one outer iteration to convergence (a NaN cost ends the loop), the fixed count otherwise
        assert new[tag + "/iterations"][1] == (100 if mode == "fixed" else 1), (tag, new[tag + "/iterations"])
