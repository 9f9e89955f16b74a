"""The partition stage of the particle weight (include/RBPHDFilter.hpp:865-990, src/CostMatrix.cpp:92-157) in exact arithmetic.

Input: a gated likelihood table L (evaluation points x measurements, Pd included), the evaluation points' Pd, the clutter
intensity -- all doubles, taken as the rationals they are.  Every sum and product below is a fractions.Fraction; the result is
rounded to a double once, at the end.

What the reference does, restated here from its description and not from the device code:

- the connected components of the bipartite graph of L's non-zero cells, numbered by their smallest vertex (rows 0 .. nE-1 first,
  then columns);
- a component without rows or without columns is a zero partition; all of them are pooled into the FIRST one, which counts
  prod(Pd of its rows) * clutter^(its columns) -- Pd, not 1 - Pd;
- the pooled ones stay in the component list, but the caller only walks the first  n_components - (n_zero - 1)  entries: a pooled
  singleton inside that range is visited AGAIN as an ordinary partition (a lone row counts 1 - Pd, a lone column the clutter) and
  as many trailing components are never visited -- also the first zero partition itself when it lies beyond the range;
- an ordinary partition with rows + columns <= 8 counts the sum over all its partial assignments
      sum over matchings M:  prod_{(i,j) in M} L[i][j] * prod_{rows i not in M} (1 - Pd_i) * clutter^(columns not in M);
- a larger one counts the 200 best terms of that sum (Murty); in the engine's opt-in exact mode it counts the whole sum when its
  smaller side has at most 9 items.

The Murty-200 rule is decided here only where it can be decided without a ranked-assignment solver: when the partition has at
most 200 assignments with a non-zero term (the truncated sum is the whole sum), or when rows + columns <= 10
(tests/support/murty_reference.py's brute force over the extended table).  Anything else raises Undecidable.
"""
import math
from fractions import Fraction

import numpy as np

from tests.support import murty_reference as mr

ENUM_MAX = 8            # rows + columns of a partition the reference enumerates
EXACT_MAX_SMALL = 9     # exact mode: the smaller side
MURTY_MAX = 64          # rows + columns of a Murty partition the device accepts


class Undecidable(Exception):
    """A Murty-200 partition whose sum this module cannot decide on its own."""


class Refused(Exception):
    """A partition the device has to refuse (a Murty partition with rows + columns > 64)."""


def components(L):
    """[(rows, cols)] of the connected components of L's non-zero cells, ordered by smallest vertex (rows first)."""
    L = np.asarray(L)
    nE, nZ = L.shape
    adj_r = [[int(n) for n in np.nonzero(L[e])[0]] for e in range(nE)]
    adj_c = [[int(e) for e in np.nonzero(L[:, n])[0]] for n in range(nZ)]
    seen = [False] * (nE + nZ)
    out = []
    for v0 in range(nE + nZ):
        if seen[v0]:
            continue
        seen[v0] = True
        todo, rows, cols = [v0], [], []
        while todo:
            v = todo.pop()
            if v < nE:
                rows.append(v)
                nxt = [nE + n for n in adj_r[v]]
            else:
                cols.append(v - nE)
                nxt = adj_c[v - nE]
            for u in nxt:
                if not seen[u]:
                    seen[u] = True
                    todo.append(u)
        out.append((sorted(rows), sorted(cols)))
    return out


def count_matchings(L, rows, cols):
    """Number of partial assignments of the partition that use non-zero cells only (the empty one included)."""
    small, large, by_cols = (cols, rows, True) if len(cols) <= len(rows) else (rows, cols, False)
    k = len(small)
    f = [0] * (1 << k)
    f[0] = 1
    for it in large:
        a = [1 if (L[it][b] if by_cols else L[b][it]) != 0 else 0 for b in small]
        for S in range((1 << k) - 1, -1, -1):
            acc = f[S]
            for b in range(k):
                if (S >> b) & 1 and a[b]:
                    acc += f[S ^ (1 << b)]
            f[S] = acc
    return sum(f)


def partial_assignment_sum(L, pd, clutter, rows, cols):
    """The sum over ALL partial assignments of one partition, as a Fraction: the recurrence over the subsets S of the smaller
    side -- the items of the larger side one at a time,  f'[S] = f[S] * u + sum_{b in S} f[S - b] * L[item, b],  u the item's
    unmatched factor -- closed with the unmatched factors of the smaller side."""
    c = Fraction(clutter)
    miss = {e: 1 - Fraction(float(pd[e])) for e in rows}
    by_cols = len(cols) <= len(rows)
    small, large = (cols, rows) if by_cols else (rows, cols)
    k = len(small)
    f = [Fraction(0)] * (1 << k)
    f[0] = Fraction(1)
    for it in large:
        u = miss[it] if by_cols else c
        a = [Fraction(float(L[it][b] if by_cols else L[b][it])) for b in small]
        for S in range((1 << k) - 1, -1, -1):
            acc = f[S] * u
            for b in range(k):
                if (S >> b) & 1 and a[b]:
                    acc += f[S ^ (1 << b)] * a[b]
            f[S] = acc
    h = [c if by_cols else miss[b] for b in small]
    tot = Fraction(0)
    for S in range(1 << k):
        g = f[S]
        if g:
            for b in range(k):
                if not (S >> b) & 1:
                    g *= h[b]
            tot += g
    return tot


def extended_table(L, pd, clutter, rows, cols):
    """The extended log table the reference hands to Murty (RBPHDFilter.hpp:907-940; tests/support/murty_reference.py)."""
    nR, nC = len(rows), len(cols)
    n = nR + nC
    C = np.full((n, n), mr.BIG_NEG)
    for a, e in enumerate(rows):
        for b, z in enumerate(cols):
            v = float(L[e][z])
            C[a, b] = mr.BIG_NEG if v == 0 else max(math.log(v), mr.BIG_NEG)
        C[a, nC + a] = math.log(1 - float(pd[e]))
    for b in range(nC):
        C[nR + b, b] = math.log(clutter)
    C[nR:, nC:] = 0.0
    return C


def murty200_route(L, pd, clutter, rows, cols):
    """How this module decides a Murty-200 partition: 'all' (<= 200 non-zero terms), 'brute' (rows + columns <= 10) or None."""
    if len(rows) + len(cols) > MURTY_MAX:
        raise Refused((len(rows), len(cols)))
    if any(float(pd[e]) >= 1.0 for e in rows):
        return None          # (log(1 - Pd) = -inf: the reference's solver fails at the root; that rule is the oracle's to state)
    if min(len(rows), len(cols)) <= 12 and count_matchings(L, rows, cols) <= mr.KBEST:     # (2^k subset states: small sides only)
        return "all"
    if len(rows) + len(cols) <= 10:
        return "brute"
    return None


def plan(L, exact=False):
    """The walk over the partitions, from the table alone: a dict with the components, the zero partitions' indices, `combined`
    (index of the first zero partition or None), `n_partitions` (how many entries the caller visits) and `visited`: a list of
    (index, kind, rows, cols), kind in 'zero', 'enum', 'exact', 'murty'."""
    comps = components(L)
    zero = [k for k, (r, c) in enumerate(comps) if not r or not c]
    combined = zero[0] if zero else None
    nP = len(comps) - max(len(zero) - 1, 0)
    visited = []
    for p in range(nP):
        r, c = comps[p]
        if p == combined:
            visited.append((p, "zero", [e for k in zero for e in comps[k][0]], [z for k in zero for z in comps[k][1]]))
        elif len(r) + len(c) <= ENUM_MAX:
            visited.append((p, "enum", r, c))
        elif exact and min(len(r), len(c)) <= EXACT_MAX_SMALL:
            visited.append((p, "exact", r, c))
        else:
            visited.append((p, "murty", r, c))
    return dict(components=comps, zero=zero, combined=combined, n_partitions=nP, visited=visited)


def partition_likelihood(L, pd, clutter, exact=False, factors=False):
    """The product over the visited partitions (before the clutter-integral division), rounded once.  factors=True: also the
    list of (index, kind, rows, cols, value as float) per visited partition."""
    L = np.asarray(L, dtype=np.float64)
    c = Fraction(clutter)
    total = Fraction(1)
    out = []
    for p, kind, rows, cols in plan(L, exact)["visited"]:
        if kind == "zero":
            v = Fraction(1)
            for e in rows:
                v *= Fraction(float(pd[e]))
            v *= c ** len(cols)
        elif kind in ("enum", "exact"):
            v = partial_assignment_sum(L, pd, clutter, rows, cols)
        else:
            how = murty200_route(L, pd, clutter, rows, cols)
            if how == "all":
                v = partial_assignment_sum(L, pd, clutter, rows, cols)
            elif how == "brute":
                v = Fraction(mr.partial_bruteforce_sum(extended_table(L, pd, clutter, rows, cols), len(rows), len(cols)))
            else:
                raise Undecidable((p, len(rows), len(cols)))
        total *= v
        out.append((p, kind, rows, cols, float(v)))
    return (float(total), out) if factors else float(total)


def bruteforce_partial_sum(L, pd, clutter, rows, cols):
    """The same sum as partial_assignment_sum by walking every partial assignment (itertools), in Fractions: the check of the
    recurrence, for rows + columns <= 10."""
    import itertools
    assert len(rows) + len(cols) <= 10
    c = Fraction(clutter)
    tot = Fraction(0)
    for k in range(0, min(len(rows), len(cols)) + 1):
        for rs in itertools.combinations(rows, k):
            for cs in itertools.permutations(cols, k):
                t = Fraction(1)
                for e, z in zip(rs, cs):
                    t *= Fraction(float(L[e][z]))
                if not t:
                    continue
                for e in rows:
                    if e not in rs:
                        t *= 1 - Fraction(float(pd[e]))
                tot += t * c ** (len(cols) - k)
    return tot
