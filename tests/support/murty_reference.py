"""Exact Murty-200 partition sums for the extended tables of include/RBPHDFilter.hpp:907-959, without the oracle.

An extended table of a partition with nR rows (evaluation points) and nC columns (measurements) has dimension n = nR + nC:

    [ L  (nR x nC, logs floored at -1000) | miss  (nR x nR: log(1 - Pd) on the diagonal, -1000 elsewhere) ]
    [ clutter (nC x nC: diagonal, -1000)  | zero  (nC x nR)                                              ]

Murty with setRealAssignmentBlock(nR, nC) returns one assignment per distinct REAL assignment -- each real row to a distinct
real column or to its miss -- best first; the reference sums exp(score) over the first 200 of them and stops at the first
score below -1000 (RBPHDFilter.hpp:948-959).  Both functions here return that sum, computed in plain Python with math.fsum:

- partial_bruteforce_sum: every partial assignment of a small finite table, scored from the table's own cells;
- separable_table: a table built so that its ranking is known in closed form (a hidden injection of row/column pairs, each
  either detected or missed + clutter, every other real cell -1000), for any dimension up to 64.
"""
import heapq
import itertools
import math

import numpy as np

BIG_NEG = -1000.0
KBEST = 200


def _ranked_sum(scores):
    """sum of exp over the best <= 200 scores that are >= -1000 (the reference's loop, RBPHDFilter.hpp:948-959)"""
    top = sorted(scores, reverse=True)[:KBEST]
    return math.fsum(math.exp(s) for s in top if s >= BIG_NEG)


def partial_scores(C, nR, nC):
    """The score of every partial assignment of a finite extended table (the real block's cells, the missed rows' diagonal
    miss cells, the unused columns' diagonal clutter cells), one per distinct real assignment."""
    C = np.asarray(C, dtype=np.float64)
    n = nR + nC
    assert C.shape == (n, n)
    assert np.all(np.isfinite(C)), "partial_bruteforce_sum: finite tables only"
    out = []
    # each row r: a real column or None (missed); the real columns taken are distinct
    for choice in itertools.product(*[list(range(nC)) + [None] for _ in range(nR)]):
        used = [c for c in choice if c is not None]
        if len(set(used)) != len(used):
            continue
        terms = []
        for r, c in enumerate(choice):
            terms.append(C[r, c] if c is not None else C[r, nC + r])
        taken = set(used)
        for c in range(nC):
            if c not in taken:
                terms.append(C[nR + c, c])
        out.append(math.fsum(terms))
    return out


def partial_bruteforce_sum(C, nR, nC):
    """Murty-200 partition sum of a finite extended table with nR + nC <= 10, by enumeration of every partial assignment."""
    assert nR + nC <= 10, "partial_bruteforce_sum: nR + nC <= 10"
    return _ranked_sum(partial_scores(C, nR, nC))


def _k_smallest_subset_sums(gains, k):
    """The k smallest subset sums of non-negative `gains` (index sets into it), smallest first: the usual heap walk over the
    gains sorted ascending -- from a set whose largest index is i, 'add i + 1' and 'replace i by i + 1'."""
    order = sorted(range(len(gains)), key=lambda i: gains[i])
    g = [gains[i] for i in order]
    out = [()]
    if not g:
        return out
    heap = [(g[0], (0,))]
    while heap and len(out) < k:
        s, idx = heapq.heappop(heap)
        out.append(tuple(order[i] for i in idx))
        i = idx[-1]
        if i + 1 < len(g):
            heapq.heappush(heap, (s + g[i + 1], idx + (i + 1,)))
            heapq.heappush(heap, (s - g[i] + g[i + 1], idx[:-1] + (i + 1,)))
    return out


def _grid(x):
    return np.round(np.asarray(x, dtype=np.float64) * 1024.0) / 1024.0


def separable_table(rng, nR, nC, ties=False, shift=0.0, spread=3.0, gap=0.0, first_rows=False, return_scores=False):
    """A table whose Murty-200 sum is known exactly, for any nR + nC <= 64.  Returns (C, exact_sum)
    (and the ranked scores >= -1000, best first, with return_scores).

    A hidden random injection pairs min(nR, nC) rows with as many columns; each pair is either 'detected' (its real cell) or
    'missed + clutter' (the row's miss cell + the column's clutter cell).  Unpaired rows always miss, unpaired columns are
    always clutter.  Every other real cell is -1000, and every cell an assignment can take is strictly negative, so an
    assignment through a -1000 cell scores below -1000 and is cut.  The legitimate assignments are the 2^m choices of the m
    pairs; the best is every pair at its better option, and the next ones are the k smallest subset sums of the per-pair gains.
    ties=True gives every pair the same two cells: C(m, j) exactly equal scores per level j, so the cut at 200 falls inside a
    block of ties.  shift moves every legitimate score by the same amount (spread over the pairs and the unpaired rows and
    columns); no score lies within 1e-6 of -1000.  spread: the range of the cells' magnitudes; gap: each pair's worse option
    lies a further U(0, gap) below (wide gaps between the ranked scores while the best stays near 0).  first_rows: the pairs
    take rows 0 .. m-1 (every ranked assignment differs from the best in its first rows: Murty's nodes sit at low partition
    indices and each expansion has many children).
    Every cell is a multiple of 2^-10, so every score -- a sum of at most 64 cells -- is exact in fp64 whatever order a solver
    adds it in: the sum's only rounding is exp's and the summation's."""
    n = nR + nC
    assert 1 <= n <= 64
    m = min(nR, nC)
    rows = rng.permutation(nR)[:m]
    if first_rows:
        rows = rng.permutation(m)
    cols = rng.permutation(nC)[:m]
    C = np.zeros((n, n))
    C[:nR, :nC] = BIG_NEG
    C[:nR, nC:] = BIG_NEG
    C[nR:, :nC] = BIG_NEG
    lo = 0.05 * spread
    if ties:
        det = np.full(m, -0.5 * spread)
        mis = np.full(nR, -0.35 * spread)
        clu = np.full(nC, -0.4 * spread)
    else:
        det = -rng.uniform(lo, spread, m)
        mis = -rng.uniform(lo, spread, nR)
        clu = -rng.uniform(lo, spread, nC)
    if gap > 0 and not ties:
        for k in range(m):
            extra = rng.uniform(0.0, gap)
            if det[k] < mis[rows[k]] + clu[cols[k]]:
                det[k] -= extra
            else:
                mis[rows[k]] -= extra
    # the shift: the same amount into both options of every pair and into every unpaired row's miss / column's clutter
    per = _grid(shift / max(nR, nC))
    det, mis, clu = _grid(det) + per, _grid(mis), _grid(clu)
    mis = mis + per      # (a paired row: both its options move, the detection above and the miss here)
    paired_r, paired_c = set(rows.tolist()), set(cols.tolist())
    for c in range(nC):
        if c not in paired_c:
            clu[c] += per
    for k in range(m):
        C[rows[k], cols[k]] = det[k]
    for r in range(nR):
        C[r, nC + r] = mis[r]
    for c in range(nC):
        C[nR + c, c] = clu[c]
    assert np.all(C[:nR, :nC][C[:nR, :nC] != BIG_NEG] < 0) and np.all(np.diag(C[:nR, nC:]) < 0) and np.all(np.diag(C[nR:, :nC]) < 0)

    # per pair: its two options' cells; the better one is in the best assignment
    opt_det = [[C[rows[k], cols[k]]] for k in range(m)]
    opt_mis = [[C[rows[k], nC + rows[k]], C[nR + cols[k], cols[k]]] for k in range(m)]
    val_det = [math.fsum(x) for x in opt_det]
    val_mis = [math.fsum(x) for x in opt_mis]
    better = [opt_det[k] if val_det[k] >= val_mis[k] else opt_mis[k] for k in range(m)]
    worse = [opt_mis[k] if val_det[k] >= val_mis[k] else opt_det[k] for k in range(m)]
    gains = [abs(val_det[k] - val_mis[k]) for k in range(m)]
    fixed = [C[r, nC + r] for r in range(nR) if r not in paired_r] + [C[nR + c, c] for c in range(nC) if c not in paired_c]
    scores = []
    for flip in _k_smallest_subset_sums(gains, KBEST + 1):
        fl = set(flip)
        cells = list(fixed)
        for k in range(m):
            cells += worse[k] if k in fl else better[k]
        scores.append(math.fsum(cells))
    scores.sort(reverse=True)
    top = [s for s in scores[:KBEST] if s >= BIG_NEG]
    assert all(abs(s - BIG_NEG) >= 1e-6 for s in scores[:KBEST]), "a score within 1e-6 of the cut: pick another shift"
    exact = math.fsum(math.exp(s) for s in top)    # (with ties the 201st score may equal the 200th: either gives the same term)
    if return_scores:
        return C, exact, top
    return C, exact
