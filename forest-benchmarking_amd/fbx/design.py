"""Designs: the data-independent half of a tomography experiment, shared by a batch.

Mirrors the setting generators of the reference (tomography.py:31-123) and flattens
``List[ExperimentResult]`` (observable_estimation.py:694-733) into the SoA layout of the C
ABI.  Label codes are those of include/fbx.h.
"""
import ctypes as C
import itertools

import numpy as np

from . import _lib

STATE_CODES = {("X", 0): 0, ("X", 1): 1, ("Y", 0): 2, ("Y", 1): 3, ("Z", 0): 4, ("Z", 1): 5,
               ("SIC", 0): 6, ("SIC", 1): 7, ("SIC", 2): 8, ("SIC", 3): 9}
STATE_LABELS = {v: k for k, v in STATE_CODES.items()}
PAULI_CODES = {"I": 0, "X": 1, "Y": 2, "Z": 3}
PAULI_LABELS = "IXYZ"


class Design:
    """m settings on n qubits + the device handle created from them."""

    def __init__(self, n_qubits, kind, in_labels, paulis, coefs=None):
        self.n_qubits = int(n_qubits)
        self.kind = kind
        self.paulis = np.ascontiguousarray(paulis, dtype=np.uint8).reshape(-1, self.n_qubits)
        self.m = self.paulis.shape[0]
        if in_labels is None:
            in_labels = np.full_like(self.paulis, 4)
        self.in_labels = np.ascontiguousarray(in_labels, dtype=np.uint8).reshape(self.m, self.n_qubits)
        self.coefs = (np.ones(self.m) if coefs is None
                      else np.ascontiguousarray(coefs, dtype=np.float64).reshape(self.m))
        self._handle = None

    @property
    def dim(self):
        return 2 ** self.n_qubits

    @property
    def n_states(self):
        """Distinct product input states of the design (S of the device tables)."""
        return len({r.tobytes() for r in self.in_labels})

    def key(self):
        return (self.n_qubits, self.kind, self.in_labels.tobytes(), self.paulis.tobytes(),
                self.coefs.tobytes())

    @property
    def handle(self):
        if self._handle is None:
            h = C.c_void_p()
            kind = _lib.KIND_PROCESS if self.kind == "process" else _lib.KIND_STATE
            _lib.check(_lib.lib().fbx_design_create(
                self.n_qubits, kind, self.m,
                self.in_labels.ctypes.data_as(C.POINTER(C.c_uint8)),
                self.paulis.ctypes.data_as(C.POINTER(C.c_uint8)),
                self.coefs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
            self._handle = h
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().fbx_design_destroy(self._handle)
                self._handle = None
        except Exception:
            pass


def traceless_pauli_codes(n):
    """utils.py:146-156 order: itertools.product('IXYZ', repeat=n) without the identity."""
    return np.array(list(itertools.product(range(4), repeat=n))[1:], dtype=np.uint8)


def state_design(n_qubits) -> Design:
    """Settings of generate_state_tomography_experiment (tomography.py:31-60)."""
    return Design(n_qubits, "state", None, traceless_pauli_codes(n_qubits))


def process_design(n_qubits, in_basis="pauli") -> Design:
    """Settings of generate_process_tomography_experiment (tomography.py:63-123)."""
    if in_basis.upper() == "SIC":
        states = [6, 7, 8, 9]
    elif in_basis.upper() == "PAULI":
        states = [0, 1, 2, 3, 4, 5]
    else:
        raise ValueError(f"Unknown basis {in_basis}")
    p = traceless_pauli_codes(n_qubits)
    ins = np.repeat(np.array(list(itertools.product(states, repeat=n_qubits)), dtype=np.uint8),
                    len(p), axis=0)
    outs = np.tile(p, (len(states) ** n_qubits, 1))
    return Design(n_qubits, "process", ins, outs)


_design_cache = {}


def flatten_results(results, qubits, kind):
    """List[ExperimentResult] (duck-typed) -> (Design, expectations[m], total_counts[m]).

    ``qubits[0]`` is the left-most tensor factor (tomography.py:149-158).  Designs are cached
    by content so repeated calls with the same settings reuse the device copy."""
    qubits = list(qubits)
    n, m = len(qubits), len(results)
    ins = np.full((m, n), 4, dtype=np.uint8)
    outs = np.zeros((m, n), dtype=np.uint8)
    coefs = np.ones(m)
    e = np.zeros(m)
    c = np.zeros(m)
    for k, r in enumerate(results):
        obs = r.setting.observable
        if not set(obs.get_qubits()) <= set(qubits):
            raise ValueError(f"observable {obs} acts on qubits outside {qubits}")
        for pos, q in enumerate(qubits):
            outs[k, pos] = PAULI_CODES[obs[q]]
        coef = complex(getattr(obs, "coefficient", 1.0))
        if abs(coef.imag) > 0:
            raise ValueError("observable coefficients must be real")
        coefs[k] = coef.real
        if kind == "process":
            by_qubit = {s.qubit: s for s in r.setting.in_state}
            for pos, q in enumerate(qubits):
                s = by_qubit[q]
                ins[k, pos] = STATE_CODES[(s.label, s.index)]
        e[k] = np.real(r.expectation)
        c[k] = r.total_counts
    d = Design(n, kind, ins, outs, coefs)
    cached = _design_cache.get(d.key())
    if cached is None:
        if len(_design_cache) > 64:
            _design_cache.clear()
        _design_cache[d.key()] = d
        cached = d
    return cached, e, c


# --------------------------------------------------------------------------------------------------
# compact structure-of-arrays archive for the batched estimators: one design shared
# by B experiments, label codes as in include/fbx.h
# --------------------------------------------------------------------------------------------------
def save_batch(fn, design: "Design", expectations, total_counts=None):
    """Write (design, expectations[B, m], total_counts[B, m]) to a compressed ``.npz``."""
    e = np.asarray(expectations, dtype=np.float64).reshape(-1, design.m)
    arrays = dict(format=np.array("fbx-soa-1"), n_qubits=np.array(design.n_qubits),
                  kind=np.array(design.kind), in_labels=design.in_labels, paulis=design.paulis,
                  coefs=design.coefs, expectations=e)
    if total_counts is not None:
        arrays["total_counts"] = np.asarray(total_counts, dtype=np.float64).reshape(e.shape)
    np.savez_compressed(fn, **arrays)
    return fn


def load_batch(fn):
    """Inverse of :func:`save_batch`: ``(Design, expectations, total_counts or None)``; the design is
    taken from the content-keyed cache when an identical one already lives on the device."""
    with np.load(fn) as z:
        if str(z["format"]) != "fbx-soa-1":
            raise ValueError(f"{fn}: not an fbx structure-of-arrays archive")
        d = Design(int(z["n_qubits"]), str(z["kind"]), z["in_labels"], z["paulis"], z["coefs"])
        e = z["expectations"]
        c = z["total_counts"] if "total_counts" in z.files else None
    d = _design_cache.setdefault(d.key(), d)
    return d, e, c


# --------------------------------------------------------------------------------------------------
# groupings: which settings of a design are estimated from the same shots (observable_estimation.group_settings on label arrays)
# --------------------------------------------------------------------------------------------------
class Grouping:
    """A partition of a design's settings into groups that share one input state and one tensor-product basis + the device
    handle created from it (``fbx_grouping_create``).  ``group_of [m]`` int32 is the group of every setting, ``groups`` the
    same as index lists (members in the order given), ``n_groups`` their number.  Built from a ``group_of`` array, from index
    lists (:meth:`from_groups`) or from an ``ObservablesExperiment`` (:meth:`from_experiment`); a group with mixed input states,
    with Paulis that disagree on a qubit, without a member, or an id out of range raises ``ValueError`` here, before the
    library is touched."""

    def __init__(self, design: Design, group_of, groups=None):
        self.design = design
        g = np.asarray(group_of)
        if g.shape != (design.m,) or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"group_of must be {design.m} integers, one per setting")
        n_groups = len(groups) if groups is not None else (int(g.max()) + 1 if g.size else 0)
        if g.size and (g.min() < 0 or g.max() >= n_groups):
            raise ValueError(f"group ids must be in [0, {n_groups})")
        self.group_of = np.ascontiguousarray(g, dtype=np.int32)
        self.n_groups = n_groups
        if groups is None:
            order = np.argsort(self.group_of, kind="stable")
            cuts = np.searchsorted(self.group_of[order], np.arange(1, n_groups))
            groups = [part.tolist() for part in np.split(order, cuts)]
        self.groups = [list(map(int, grp)) for grp in groups]
        self.basis = np.zeros((n_groups, design.n_qubits), dtype=np.uint8)      # Z where no member acts
        for i, grp in enumerate(self.groups):
            if not grp:
                raise ValueError(f"group {i} has no member")
            if np.any(design.in_labels[grp] != design.in_labels[grp[0]]):
                raise ValueError(f"group {i} mixes input states: its settings cannot share shots")
            p = design.paulis[grp]
            top = p.max(axis=0)
            if np.any((p != 0) & (p != top)):
                raise ValueError(f"group {i} holds Paulis that differ on a qubit: they are not diagonal in one tensor-product basis")
            self.basis[i] = np.where(top == 0, 3, top)
        self._handle = None

    @classmethod
    def from_groups(cls, design: Design, groups):
        """From index lists; every setting index must appear exactly once."""
        groups = [list(map(int, grp)) for grp in groups]
        flat = [k for grp in groups for k in grp]
        if sorted(flat) != list(range(design.m)):
            raise ValueError("the groups must hold every setting index of the design exactly once")
        group_of = np.empty(design.m, dtype=np.int32)
        for i, grp in enumerate(groups):
            group_of[grp] = i
        return cls(design, group_of, groups)

    @classmethod
    def from_experiment(cls, design: Design, obs_expt, qubits=None):
        """From a grouped ``ObservablesExperiment`` whose settings are those of ``design`` on ``qubits`` (default 0..n-1): a
        setting that occurs several times takes the design's indices of its twins in ascending order."""
        from .tomography import _settings_of
        qubits = list(range(design.n_qubits)) if qubits is None else list(qubits)
        where = {}
        for k, s in enumerate(_settings_of(design, qubits)):
            where.setdefault(_setting_key(s), []).append(k)
        where = {key: ks[::-1] for key, ks in where.items()}
        try:
            groups = [[where[_setting_key(s)].pop() for s in grp] for grp in obs_expt]
        except (KeyError, IndexError):
            raise ValueError("the experiment holds a setting the design does not (or holds it more often)") from None
        return cls.from_groups(design, groups)

    @property
    def handle(self):
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(_lib.lib().fbx_grouping_create(self.design.handle, self.n_groups, _lib.iptr(self.group_of), C.byref(h)))
            self._handle = h
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().fbx_grouping_destroy(self._handle)
                self._handle = None
        except Exception:
            pass


def _setting_key(setting):
    """a setting without its coefficient (``_settings_of`` drops the coefficients of a design)"""
    return setting.in_state, frozenset(setting.observable)


def _greedy_groups(design: Design):
    """observable_estimation._max_tpb_overlap on the label arrays: the buckets are rows of (input-state id, basis codes, rank);
    a setting fits a bucket of its input state whose basis agrees with it wherever both are not the identity, takes the fitting
    bucket of the lowest rank, and a bucket whose basis grows gets a new highest rank (it moves to the end)."""
    m, n = design.m, design.n_qubits
    _, state_of = np.unique(design.in_labels, axis=0, return_inverse=True)
    state_of = state_of.reshape(m)
    b_state, b_rank = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64)
    b_basis = np.zeros((m, n), dtype=np.uint8)
    members, nb, rank = [], 0, 0
    for k in range(m):
        p = design.paulis[k]
        basis = b_basis[:nb]
        fits = (b_state[:nb] == state_of[k]) & np.all((basis == 0) | (p == 0) | (basis == p), axis=1)
        hit = np.flatnonzero(fits)
        if hit.size:
            i = hit[np.argmin(b_rank[hit])]
            members[i].append(k)
            if np.any((b_basis[i] == 0) & (p != 0)):
                b_basis[i] |= p                              # (codes agree where both are set: OR fills the empty places)
                b_rank[i] = rank
                rank += 1
        else:
            b_state[nb], b_basis[nb], b_rank[nb] = state_of[k], p, rank
            members.append([k])
            nb += 1
            rank += 1
    return [members[i] for i in np.argsort(b_rank[:nb])]


def group_design(design: Design, method="greedy") -> Grouping:
    """The settings of ``design`` grouped by a shared tensor-product basis: the groups, their order and the order of their
    members are those of ``observable_estimation.group_settings(..., method)`` on the design's setting objects.  'greedy' works
    on the label arrays; 'clique-removal' goes through the objects (networkx)."""
    if method == "greedy":
        return Grouping.from_groups(design, _greedy_groups(design))
    if method != "clique-removal":
        raise ValueError("method must be 'greedy' or 'clique-removal'")
    from .observable_estimation import ObservablesExperiment, group_settings
    from .tomography import _settings_of
    expt = ObservablesExperiment(_settings_of(design, range(design.n_qubits)))
    return Grouping.from_experiment(design, group_settings(expt, method))
