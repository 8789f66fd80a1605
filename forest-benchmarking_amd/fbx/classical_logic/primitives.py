"""Circuit primitives for classical reversible logic (forest/benchmarking/classical_logic/primitives.py) as gate lists: each
function returns the ``(name, qubits)`` tuples that ``reversible.encode_reversible`` takes, in the reference's gate order.  The
adder construction is that of Cuccaro, Draper, Kutin and Moulton, "A new quantum ripple-carry addition circuit"
(arXiv:quant-ph/0410184)."""

__all__ = ["CNOT_X_basis", "CCNOT_X_basis", "majority_gate", "unmajority_add_gate", "unmajority_add_parallel_gate"]


def CNOT_X_basis(control, target):
    """The CNOT in the X basis, ``|+X+| * I + |-X-| * Z``: H(control), CZ(control, target), H(control)."""
    return [("H", (control,)), ("CZ", (control, target)), ("H", (control,))]


def CCNOT_X_basis(control1, control2, target):
    """The CCNOT in the X basis (Z on the target iff both controls are ``|->``): H on all three, CCNOT, H on all three."""
    hs = [("H", (control1,)), ("H", (control2,)), ("H", (target,))]
    return hs + [("CCNOT", (control1, control2, target))] + hs


def _gates(in_x_basis):
    if in_x_basis:
        return CNOT_X_basis, CCNOT_X_basis
    return (lambda c, t: [("CNOT", (c, t))]), (lambda c1, c2, t: [("CCNOT", (c1, c2, t))])


def majority_gate(a, b, c, in_x_basis=False):
    """MAJ: (c xor a) on the c line, (b xor a) on the b line and the majority of the three inputs on the a line."""
    cnot, ccnot = _gates(in_x_basis)
    return cnot(a, b) + cnot(a, c) + ccnot(c, b, a)


def unmajority_add_gate(a, b, c, in_x_basis=False):
    """UMA: run on the output of ``majority_gate(a, b, c)`` it restores the a and c lines and leaves a + b + c (mod 2) on b."""
    cnot, ccnot = _gates(in_x_basis)
    return ccnot(c, b, a) + cnot(a, c) + cnot(c, b)


def unmajority_add_parallel_gate(a, b, c, in_x_basis=False):
    """The form of UMA with three CNOTs and more parallelism (figure 3 of the paper): the same logic as ``unmajority_add_gate``
    on every input, in either basis.  Two departures from the reference's text (primitives.py:147-154), which as written is not
    UMA: there the a and c lines are exchanged against the paper's figure, and its ``X(b)`` is a NOT only in the Z basis -- in the
    X basis the NOT is H, X, H here, built as ``CNOT_X_basis`` is."""
    cnot, ccnot = _gates(in_x_basis)
    flip = [("H", (b,)), ("X", (b,)), ("H", (b,))] if in_x_basis else [("X", (b,))]
    return flip + cnot(c, b) + ccnot(c, b, a) + flip + cnot(a, c) + cnot(a, b)
