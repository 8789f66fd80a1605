"""LDS bank conflicts of the quantum-volume simulator's gate step (csrc/fbx_qvolume.hip), enumerated on the host.

A 16-byte LDS read of a wavefront is served in four groups of 16 lanes over 64 four-byte banks, a 16-byte write in eight groups of
8 consecutive lanes over 32 banks; the lanes of a group conflict when their 16-byte elements coincide modulo 16 (modulo 8 for a
write).  For every width and every pair of target bit positions this script maps lane -> element exactly as the kernel does
(group counter with zero bits inserted at the targets, then the slot swizzle) and prints the worst multiplicity per lane group, with
and without the swizzle.  Usage: python scripts/qv_lds_conflicts.py [--all]
"""
import itertools
import sys

READ_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
               list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
WRITE_GROUPS = [list(range(8 * k, 8 * k + 8)) for k in range(8)]


def slot(i, swizzle):
    return i ^ (((i >> 3) & 1) * 7) ^ ((i >> 1) & 8) ^ ((i >> 5) & 3) if swizzle else i


def insert_zero(x, pos):
    return ((x >> pos) << (pos + 1)) | (x & ((1 << pos) - 1))


def worst(n, p0, p1, swizzle):
    """(read, write) worst multiplicity over the lane groups of the first wavefront and the four amplitudes of a group"""
    lo, hi = min(p0, p1), max(p0, p1)
    groups = 1 << (n - 2)
    out = []
    for lane_groups, modulus in ((READ_GROUPS, 16), (WRITE_GROUPS, 8)):
        w = 1
        for add in (0, 1 << p1, 1 << p0, (1 << p0) | (1 << p1)):
            for lanes in lane_groups:
                seen = {}
                for t in lanes:
                    if t >= groups:
                        continue
                    e = slot(insert_zero(insert_zero(t, lo), hi) | add, swizzle)
                    seen.setdefault(e % modulus, set()).add(e)
                w = max([w] + [len(v) for v in seen.values()])
        out.append(w)
    return tuple(out)


if __name__ == "__main__":
    for n in range(2, 14):
        rows = {}
        for p0, p1 in itertools.permutations(range(n), 2):
            rows[(p0, p1)] = (worst(n, p0, p1, False), worst(n, p0, p1, True))
        plain_r = max(v[0][0] for v in rows.values()); plain_w = max(v[0][1] for v in rows.values())
        swz_r = max(v[1][0] for v in rows.values()); swz_w = max(v[1][1] for v in rows.values())
        hit_plain = sum(1 for v in rows.values() if max(v[0]) > 1) / len(rows)
        hit_swz = sum(1 for v in rows.values() if max(v[1]) > 1) / len(rows)
        print(f"width {n:2d}: plain worst read x{plain_r} write x{plain_w} ({100 * hit_plain:.0f} % of pairs conflict)   "
              f"swizzled worst read x{swz_r} write x{swz_w} ({100 * hit_swz:.0f} %)")
        if "--all" in sys.argv:
            for k, v in sorted(rows.items()):
                if max(v[1]) > 1:
                    print("   bits", k, "plain", v[0], "swizzled", v[1])
