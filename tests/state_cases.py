"""State-tomography designs and data that place the dispatch of fbx_mle_state on purpose (tests/test_state_dispatch_gpu.py), with
the oracle-only checks of the conditions those tests rely on in tests/test_state_cases_cpu.py.  Everything is deterministic in its
seed and built on fbx_oracle.design; nothing here needs a device.

With D = 4^n the kernels switch at m <= D (several items per wavefront), m <= 64 (one setting per lane) and beyond (settings
walked in strides of 64); the kinds below sit on either side of each switch:

    kind            m, n = 1 / 2 / 3     settings
    standard        3 / 15 / 63          every traceless Pauli, the reference's order
    with_identity   4 / 16 / 64          the all-identity observable first, then the standard ones
    twice           6 / 30 / 126         the standard design measured twice
    d_plus_1        5 / 17 / -           the standard design and its first two settings again
    sixty_four      64 / 64 / -          the standard design repeated and cut after 64 settings
    sixty_five      65 / 65 / -          ... after 65

`signed=True` gives the settings the coefficients {1, -1, 0.5, -0.5} in equal shares and a random order (magnitudes of at most
one keep both outcome probabilities of a setting valid); the identity of with_identity then carries -0.5, so that its two outcome ratios differ and its weight on P_0 = I
is not zero.
"""
import numpy as np

import chernoff_cases as cc
from fbx_oracle import design as od

KINDS = {1: ("standard", "with_identity", "twice", "d_plus_1", "sixty_four", "sixty_five"),
         2: ("standard", "with_identity", "twice", "d_plus_1", "sixty_four", "sixty_five"),
         3: ("standard", "with_identity", "twice"),
         4: ("standard",)}
COEF_VALUES = np.array([1.0, -1.0, 0.5, -0.5])
COUNTS = 500.0


def design_variant(n, kind, signed=False, seed=0):
    """(paulis [m, n] uint8, coefs [m]) of one kind"""
    if kind not in KINDS[n]:
        raise ValueError(f"no design {kind!r} on {n} qubits")
    base = od.traceless_pauli_codes(n)
    D = 4 ** n
    if kind == "standard":
        p = base
    elif kind == "with_identity":
        p = np.concatenate([np.zeros((1, n), dtype=np.uint8), base])
    elif kind == "twice":
        p = np.concatenate([base, base])
    else:
        p = np.resize(base, ({"d_plus_1": D + 1, "sixty_four": 64, "sixty_five": 65}[kind], n))     # repeats in order, cut
    coefs = np.ones(len(p))
    if signed:
        rng = np.random.default_rng([seed, n, sorted(KINDS[1]).index(kind)])
        coefs = rng.permutation(np.resize(COEF_VALUES[[1, 2, 3, 0]], len(p)))      # every value, as evenly as m allows
        if kind == "with_identity":
            coefs[0] = -0.5
    return np.ascontiguousarray(p, dtype=np.uint8), coefs


def oracle_design(n, paulis, coefs):
    return od.Design(n, "state", np.full_like(paulis, 4), paulis, np.asarray(coefs, dtype=float))


def device_design(n, paulis, coefs):
    from fbx.design import Design
    return Design(n, "state", None, paulis, coefs)


def data(n, paulis, coefs, B, seed):
    """(expectations [B, m], counts [B, m]): the coefficient times the Pauli expectation of 0.8 (random state) + 0.2 (maximally
    mixed), Gaussian noise of 0.02 -- 0.5 on every second item, so that the items of a batch need different numbers of iterations
    -- clipped to +-|coefficient|; 500 counts per setting.

    An identity observable of coefficient +-1 keeps its exact expectation: one of its outcomes has probability zero in every
    state, and a non-zero frequency for it divides by the reference's 2.2e-308 guard and overflows in the reference as on the
    device.  (Every shot of the identity returns +1.)"""
    rng = np.random.default_rng([seed, n, len(paulis)])
    d = 2 ** n
    coefs = np.asarray(coefs, dtype=float)
    ops = np.array([od.pauli_matrix(p) for p in paulis])
    index = paulis.astype(int) @ (4 ** np.arange(n - 1, -1, -1))         # which Pauli operator a setting measures
    e = np.empty((B, len(paulis)))
    for b in range(B):
        rho = 0.8 * cc.random_state(d, rng) + 0.2 * np.eye(d) / d
        clean = coefs * np.einsum("kij,ji->k", ops, rho).real
        if b % 2:
            noisy = clean + 0.1 * rng.standard_normal(4 ** n)[index]
        else:
            noisy = clean + 0.02 * rng.standard_normal(len(paulis))
        e[b] = np.clip(noisy, -np.abs(coefs), np.abs(coefs))
        certain = (paulis.max(axis=1) == 0) & (np.abs(coefs) == 1.0)
        e[b, certain] = coefs[certain]
    return e, np.full(e.shape, COUNTS)


# epsilon, tol, maxiter of the converge mode per number of qubits: tests/test_state_cases_cpu.py holds the oracle to "every item
# stops before maxiter, after a few hundred iterations at the most" with these and lists its counts
CONVERGE = {1: dict(epsilon=0.5, tol=1e-6, maxiter=2000),
            2: dict(epsilon=1.0, tol=1e-4, maxiter=2000),
            3: dict(epsilon=0.5, tol=1e-3, maxiter=2000)}


def mode_kwargs(mode, n, m, maxiter=None):
    """keyword arguments of iterative_mle_state_estimate for `mode`: 'plain' (maxiter 40), 'converge', 'hedged', 'maxent'
    (maxiter 12).  Hedging multiplies the R operator by half the total counts (tomography.py:257-260): its epsilon is scaled so
    that the step stays the size of a plain step of 0.1."""
    if mode == "plain":
        kw = dict(maxiter=40)
    elif mode == "converge":
        kw = dict(CONVERGE[n])
    elif mode == "hedged":
        kw = dict(beta=0.5, epsilon=0.2 / (COUNTS * m), maxiter=12)
    elif mode == "maxent":
        kw = dict(entropy_penalty=0.005, maxiter=12)
    else:
        raise ValueError(mode)
    if maxiter is not None:
        kw["maxiter"] = maxiter
    return kw


MODES = ("plain", "converge", "hedged", "maxent")
# the bounds the suite already holds the estimators to (tests/test_state_gpu.py, tests/test_state_big_gpu.py)
MLE_BOUND = {"plain": 1e-11, "converge": 1e-9, "hedged": 1e-10, "maxent": 1e-10}


def permuted(paulis, coefs, e, c, seed):
    """the same list of results in another order"""
    perm = np.random.default_rng([seed, len(paulis)]).permutation(len(paulis))
    return paulis[perm], np.asarray(coefs)[perm], e[..., perm], c[..., perm]


# The rows of the dispatch table of tests/test_state_dispatch_gpu.py: (n, kind, B, modes).  Each runs with unit and with signed
# coefficients; `standard` at n = 1, 2 carries the largest batch of the partial / full wave test (smaller ones are its prefixes).
ROWS = [(1, "with_identity", 5, ("plain", "converge")), (2, "with_identity", 5, ("plain", "converge")),
        (1, "standard", 33, ("converge",)), (2, "standard", 9, ("converge",)),
        (1, "d_plus_1", 4, ("plain", "converge")), (2, "d_plus_1", 4, ("plain", "converge")),
        (1, "twice", 4, ("plain", "converge")), (2, "twice", 4, ("plain", "converge")),
        (1, "sixty_four", 4, ("plain", "converge")), (2, "sixty_four", 4, ("plain", "converge")),
        (1, "sixty_five", 4, ("plain",)), (2, "sixty_five", 4, ("plain",)),
        (3, "standard", 3, ("hedged", "maxent", "plain", "converge")),
        (3, "with_identity", 3, ("hedged", "maxent", "plain", "converge")),
        (4, "standard", 2, ("plain", "hedged"))]
# seed of data() per (n, kind, signed): the first, tried in the order 7, 0, 1, ..., with which the oracle's converge mode does what
# tests/test_state_cases_cpu.py asks for (found with the oracle alone; a step that shrinks by a few per cent per iteration often
# ends within 1 % of tol, and a batch of 33 holds many).  Rows without the converge mode take the default.
DEFAULT_SEED = 7
SEEDS = {(1, "with_identity", False): 2, (1, "with_identity", True): 7, (1, "standard", False): 0, (1, "standard", True): 102,
         (1, "d_plus_1", False): 2, (1, "d_plus_1", True): 7, (1, "twice", False): 1, (1, "twice", True): 6,
         (1, "sixty_four", False): 1, (1, "sixty_four", True): 0,
         (2, "with_identity", False): 7, (2, "with_identity", True): 41, (2, "standard", False): 13, (2, "standard", True): 508,
         (2, "d_plus_1", False): 0, (2, "d_plus_1", True): 8, (2, "twice", False): 7, (2, "twice", True): 17,
         (2, "sixty_four", False): 1, (2, "sixty_four", True): 5,
         (3, "standard", False): 6, (3, "standard", True): 144, (3, "with_identity", False): 12, (3, "with_identity", True): 174}


def case(n, kind, signed, B):
    """(paulis, coefs, expectations, counts) of one row"""
    p, cf = design_variant(n, kind, signed)
    e, c = data(n, p, cf, B, SEEDS.get((n, kind, signed), DEFAULT_SEED))
    return p, cf, e, c
