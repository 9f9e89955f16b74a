"""The weighting's partition stage (rfs-slam_amd/csrc/weighting.h steps 5-6, rfs_partitions_wave) on planted likelihood tables at
its limits, through the table-level hook rfsgpu_partition_likelihoods -- a harness around the production device function -- against
the exact rational reference of tests/support/partition_reference.py and against the oracle.

Families (each a handful of tables; the packed ones are 64 x 64 with every row and column in use, so row 63, column 63, labels up
to 127 and the top bit of every 64-bit mask are always in play):

  shapes      all 28 (r, c) with r + c <= 8, each complete-bipartite and tree-connected, at permuted positions
  boundary    the same partitions at r + c = 8 (enumerated) and with one more measurement (9: Murty-200; decided by the reference
              because they have <= 200 non-zero terms or r + c <= 10)
  exact       exact mode, smaller side k = 1 .. 9 against a larger side up to 20, both orientations, plus 9 x 9; a 10 x 10 double
              star (101 terms) that must fall through to Murty-200 in exact mode
  components  64, 65, 92, 100 and 128 components; no / one / many zero partitions; the first zero partition at index 0, 63, last;
              isolated rows and columns interleaved with 1 x 1 pairs (pooled singletons revisited, trailing components dropped)
  chains      path-shaped components numbered so that the smallest label starts at one end; a 32 + 32 path (Murty dimension 64,
              against the oracle ONLY -- 10946+ terms, the reference cannot decide its 200 best) and a 33 + 32 path that must be refused
  values      Pd == 1.0, denormal cells (one of them the only link of a row to its component), nE = 0, nZ = 0

What the tables cannot reach, by counting (asserted in test_families_reach_what_they_claim): every non-zero partition holds a row
and a column, so there are at most min(nE, nZ) <= 64 of them; with a zero partition present at most 63 (one vertex is isolated).
Hence n_partitions = non-zero + (1 if any zero) <= 64 -- the partition loop never makes a second pass -- and the first zero
partition, preceded by non-zero components only, has index <= 63 and < n_partitions: a first zero partition "at 64" or "at or beyond
n_partitions" does not exist for tables within RFSGPU_MAX_EVAL x RFSGPU_MAX_Z.  The upper halves of the component arrays (index 64
.. 127) ARE reached: by the pooled zero partitions beyond 64.

Tolerances.  Ceiling: SURVEY 8c, relative 1e-9 on a weight factor.  Working bound of the hook against the exact reference: 8 x the
oracle's largest relative deviation from the exact reference over the tables without a Murty partition (different summation order,
fused multiply-adds), measured in two classes: the table with denormal cells, where the oracle forms exp(log x) at log x = -710
(measured 4.47e-14: ORACLE_DEV_DENORMAL = 4.5e-14 -> bound 3.6e-13), and every other table (measured 9.42e-15, shapes[2]:
ORACLE_DEV_MEASURED = 9.5e-15 -> bound 7.6e-14); test_oracle_equals_the_exact_reference_on_every_table keeps both constants honest.  A Murty-200 partition keeps the bounds of
test_device_murty_sums_against_the_reference_bruteforce_fixture: 1e-12 against the exact rule, 1e-13 against the oracle -- per
Murty partition of the table, since the hook returns the product over partitions.
"""
import itertools
import math

import numpy as np
import pytest

from tests.support import partition_reference as pr

CEILING = 1e-9
ORACLE_DEV_MEASURED = 9.5e-15          # largest |oracle / exact - 1| over the tables without a Murty partition (both modes) ...
ORACLE_DEV_DENORMAL = 4.5e-14          # ... and on the table with denormal cells, ("values", 2)
WORKING = 8 * ORACLE_DEV_MEASURED
WORKING_DENORMAL = 8 * ORACLE_DEV_DENORMAL
MURTY_VS_EXACT, MURTY_VS_ORACLE = 1e-12, 1e-13
assert WORKING <= WORKING_DENORMAL <= CEILING


# ---- table construction -----------------------------------------------------------------------------------------------------

def complete(r, c):
    return np.ones((r, c), dtype=bool)


def tree(rng, r, c):
    """A random spanning tree of K(r, c): r + c - 1 cells, connected, zeros inside."""
    m = np.zeros((r, c), dtype=bool)
    rows, cols = [0], [0]
    m[0, 0] = True
    todo = [("r", i) for i in range(1, r)] + [("c", j) for j in range(1, c)]
    for k in rng.permutation(len(todo)):
        side, v = todo[k]
        if side == "r":
            m[v, cols[rng.integers(len(cols))]] = True
            rows.append(v)
        else:
            m[rows[rng.integers(len(rows))], v] = True
            cols.append(v)
    return m


def path(nr, nc):
    """r0 - c0 - r1 - c1 - ...: a path over nr rows and nc columns (nr - nc in {0, 1}) or c0 - r0 - c1 - ... (nc - nr == 1)."""
    m = np.zeros((nr, nc), dtype=bool)
    if nc > nr:
        return path(nc, nr).T
    for i in range(nr):
        if i < nc:
            m[i, i] = True
        if i >= 1 and i - 1 < nc:
            m[i, i - 1] = True
    return m


def double_star(n):
    """n x n: row 0 to every column, column 0 to every row -- a tree with 1 + n^2 partial assignments (the cell (0, 0), or any of
    row 0's other n - 1 columns or none times any of column 0's other n - 1 rows or none)."""
    m = np.zeros((n, n), dtype=bool)
    m[0, :] = True
    m[:, 0] = True
    return m


def random_connected(rng, r, c, density):
    m = tree(rng, r, c) | (rng.random((r, c)) < density)
    return m


def filler(lr, lc, small=True):
    """Stars (r x 1 or 1 x c) that use up lr rows and lc columns; small: each within r + c <= 8."""
    if lr == 0 and lc == 0:
        return []
    assert lr >= 1 and lc >= 1 and (not small or max(lr, lc) <= 7 * min(lr, lc)), (lr, lc)
    m = min(lr, lc)
    big, flip = (lr, False) if lr >= lc else (lc, True)
    sizes = [big // m + (1 if k < big % m else 0) for k in range(m)]
    return [complete(1, s) if flip else complete(s, 1) for s in sizes]


class Table:
    """A likelihood table with its Pd and clutter, and what was planted in it."""
    def __init__(self, L, pd, clutter, note):
        self.L, self.pd, self.clutter, self.note = np.ascontiguousarray(L, dtype=np.float64), np.asarray(pd, dtype=np.float64), float(clutter), note


def pack(rng, masks, nE=64, nZ=64, clutter=0.3, fill=True, ordered=False, miss=(1e-3, 0.9), note="", small_filler=True):
    """Plants the given partitions (boolean r x c cell masks) on disjoint random row / column sets of an nE x nZ table; fill: the
    rows and columns left over get partitions of their own (filler).  ordered: a partition's rows and columns keep their order (a
    path stays numbered from one end), otherwise they are shuffled.  Values: L[e][z] = (1 - Pd_e) * clutter * 10^U(-1.5, 1.5), so
    that every term of a partition's sum -- a product over its rows of a cell or 1 - Pd, times the clutter of the columns left
    over -- lies within a few decades of the others; 1 - Pd log-uniform in `miss`, which spreads the partitions' values."""
    masks = list(masks)
    ur, uc = sum(m.shape[0] for m in masks), sum(m.shape[1] for m in masks)
    assert ur <= nE and uc <= nZ, (ur, uc)
    if fill:
        masks += filler(nE - ur, nZ - uc, small_filler)
    rperm, cperm = rng.permutation(nE), rng.permutation(nZ)
    a = 10.0 ** rng.uniform(math.log10(miss[0]), math.log10(miss[1]), nE)
    pd = 1.0 - a
    L = np.zeros((nE, nZ))
    r0 = c0 = 0
    for m in masks:
        rows, cols = rperm[r0:r0 + m.shape[0]], cperm[c0:c0 + m.shape[1]]
        if ordered:
            rows, cols = np.sort(rows), np.sort(cols)
        r0 += m.shape[0]
        c0 += m.shape[1]
        for i, e in enumerate(rows):
            for j, z in enumerate(cols):
                if m[i, j]:
                    L[e, z] = (1.0 - pd[e]) * clutter * 10.0 ** rng.uniform(-1.5, 1.5)
    return Table(L, pd, clutter, note)


def bins(rng, masks, cap=64):
    """The masks dealt into groups that fit a cap x cap table (rows and columns), leaving room the filler can use."""
    out, cur, r, c = [], [], 0, 0
    for k in rng.permutation(len(masks)):
        m = masks[k]
        if r + m.shape[0] > cap - 1 or c + m.shape[1] > cap - 1:
            out.append(cur)
            cur, r, c = [], 0, 0
        cur.append(m)
        r += m.shape[0]
        c += m.shape[1]
    out.append(cur)
    return out


SHAPES28 = [(r, c) for r in range(1, 8) for c in range(1, 8) if r + c <= 8]
EXACT_LARGE = {1: 9, 2: 12, 3: 20, 4: 9, 5: 16, 6: 11, 7: 8, 8: 20, 9: 10}     # smaller side k -> the larger side


def family_shapes():
    rng = np.random.default_rng(2801)
    masks = [complete(r, c) for r, c in SHAPES28] + [tree(rng, r, c) for r, c in SHAPES28]
    return [pack(rng, g, clutter=cl, miss=(1e-5, 0.9), note="shapes") for g, cl in zip(bins(rng, masks), itertools.cycle([0.3, 3.0, 0.1]))]


def boundary_pairs():
    """(mask at r + c = 9, the same without its last column) for every r + c = 8 shape, tree-connected and complete."""
    rng = np.random.default_rng(89)
    out = []
    for r in range(1, 8):
        c = 8 - r
        m9 = np.concatenate([tree(rng, r, c), np.zeros((r, 1), dtype=bool)], axis=1)     # the extra column hangs on one row
        m9[rng.integers(r), c] = True
        out += [m9, complete(r, c + 1)]
    return out


def family_boundary():
    """Tables 0, 2: seven 9-vertex partitions each (trees / complete; Murty-200 in the default mode); tables 1, 3: the same tables
    with one measurement (a whole column of the table) taken out of each of those partitions: r + c = 8, enumerated, same cells."""
    m9 = boundary_pairs()
    tabs = []
    for half in (m9[0::2], m9[1::2]):
        rng = np.random.default_rng(890 + len(tabs))
        t9 = pack(rng, half, clutter=0.4, fill=True, note="boundary-9")
        drop = []
        for rows, cols in pr.components(t9.L):
            if len(rows) + len(cols) == 9:
                # a column whose removal keeps the rest connected: one with a single cell if there is one, else any
                sub = t9.L[np.ix_(rows, cols)] != 0
                single = [j for j in range(len(cols)) if sub[:, j].sum() == 1 and all(sub[i].sum() > 1 for i in np.nonzero(sub[:, j])[0])]
                drop.append(cols[single[0]] if single else cols[-1])
        keep = [z for z in range(64) if z not in drop]
        t8 = Table(t9.L[:, keep], t9.pd, t9.clutter, "boundary-8")
        tabs += [t9, t8]
    return tabs


def family_exact():
    rng = np.random.default_rng(919)
    masks = []
    for k, m in EXACT_LARGE.items():
        for shape in ((k, m), (m, k)):
            masks.append(complete(*shape) if k in (1, 4, 7, 9) else random_connected(rng, *shape, density=0.5))
    masks.append(random_connected(rng, 9, 9, density=0.6))
    return [pack(rng, g, clutter=cl, miss=(0.05, 0.9), note="exact", small_filler=False) for g, cl in zip(bins(rng, masks), itertools.cycle([0.5, 0.2, 1.0]))]


def family_fallthrough():
    """A 10 x 10 double star (101 non-zero terms: the reference decides it) beside small partitions: smaller side 10 -> Murty-200
    even in exact mode; and the 9 x 10 star-like neighbour that exact mode still takes."""
    rng = np.random.default_rng(1010)
    return [pack(rng, [double_star(10)], clutter=0.5, miss=(0.05, 0.9), note="k10"),
            pack(rng, [double_star(10)[:9]], clutter=0.5, miss=(0.05, 0.9), note="k9")]


def pairs_table(rng, n_pairs, iso_rows, iso_cols, extra=(), first_row=None, last_iso_row=False, clutter=0.8, note=""):
    """64 x 64: n_pairs 1 x 1 partitions, `extra` masks, and isolated rows / columns, interleaved at random.  first_row: 'iso' / 'pair'
    forces what row 0 is; last_iso_row: row 63 is the (only) isolated row."""
    masks = [complete(1, 1)] * n_pairs + list(extra)
    ur, uc = sum(m.shape[0] for m in masks), sum(m.shape[1] for m in masks)
    assert ur + iso_rows == 64 and uc + iso_cols == 64, (ur, uc)
    for _ in range(1000):
        t = pack(rng, masks, clutter=clutter, fill=False, miss=(0.05, 0.9), note=note)
        used = (t.L != 0).any(axis=1)
        if first_row == "iso" and used[0]:
            continue
        if first_row == "pair" and not used[0]:
            continue
        if last_iso_row and (used[63] or not used[:63].all()):
            continue
        return t
    raise AssertionError("no such layout drawn")


def family_components():
    rng = np.random.default_rng(6465)
    T = []
    T.append(pairs_table(rng, 64, 0, 0, note="64 components, no zero partition"))
    T.append(pairs_table(rng, 63, 1, 1, last_iso_row=True, note="65 components, first zero partition at 63, one trailing component dropped"))
    T.append(pairs_table(rng, 28, 36, 36, first_row="iso", note="100 components, first zero partition at 0"))
    T.append(pairs_table(rng, 36, 28, 28, first_row="pair", note="92 components, first zero partition inside"))
    T.append(Table(np.zeros((64, 64)), 1.0 - 10.0 ** rng.uniform(-1.3, -0.05, 64), 0.9, "128 components, all isolated"))
    # exactly one zero partition: at index 0 (row 0 isolated; a 1 x 2 takes the spare column) and at the last index (an isolated column; a 2 x 1)
    T.append(pairs_table(rng, 62, 1, 0, extra=[complete(1, 2)], first_row="iso", note="one zero partition, at 0"))
    T.append(pairs_table(rng, 62, 0, 1, extra=[complete(2, 1)], note="one zero partition, last"))
    T.append(pairs_table(rng, 10, 0, 1, extra=[complete(2, 1), complete(4, 4), complete(3, 5), tree(rng, 7, 1), complete(6, 2), tree(rng, 5, 3), complete(1, 7),
                                               tree(rng, 4, 4), tree(rng, 2, 6), complete(5, 2), complete(4, 3), complete(4, 3), complete(2, 2),
                                               complete(1, 4), complete(2, 3), tree(rng, 2, 3)],
                         note="one zero partition, last of a mixed table"))
    return T


def family_chains():
    """Tables 0 (both modes): short paths the default mode sends to Murty-200 with <= 200 terms, and enumerated ones; table 1 (exact
    mode): paths with smaller side up to 9; table 2: the 32 + 32 path; table 3: the 33 + 32 path."""
    rng = np.random.default_rng(3232)
    short = [path(5, 4), path(4, 5), path(6, 5), path(5, 6), path(5, 5), path(4, 4), path(4, 3), path(3, 4), path(2, 2)]
    long = [path(9, 9), path(10, 9), path(9, 10), path(8, 8), path(8, 7), path(5, 5)]
    return [pack(rng, short, clutter=0.6, ordered=True, miss=(0.05, 0.9), note="short paths"),
            pack(rng, long, clutter=0.6, ordered=True, miss=(0.05, 0.9), note="long paths"),
            pack(rng, [path(32, 32)], clutter=0.6, ordered=True, miss=(0.2, 0.9), note="32 + 32 path"),
            pack(rng, [path(33, 32)], nE=64, nZ=64, clutter=0.6, ordered=True, fill=False, miss=(0.2, 0.9), note="33 + 32 path")]


DENORMAL = float.fromhex("0x0.123456789abcdp-1022")


def family_values():
    rng = np.random.default_rng(1000)
    T = []
    # Pd == 1.0: one such row in each of several enumerated partitions (never alone on its side), and as the isolated row 0 (the zero
    # partition counts Pd = 1; exactly one zero partition, so it is not visited again as 1 - Pd = 0)
    t = pairs_table(rng, 19, 1, 0, extra=[complete(1, 5), complete(4, 4), tree(rng, 4, 4), complete(2, 6), complete(6, 2), tree(rng, 3, 5), complete(5, 3),
                                          complete(2, 2), complete(3, 3), tree(rng, 7, 1), complete(1, 6), complete(2, 2), complete(4, 2)],
                    first_row="iso", note="Pd == 1")
    for rows, cols in pr.components(t.L):
        if len(rows) >= 2 and cols:
            e = rows[len(rows) // 2]
            t.L[e] = np.where(t.L[e] != 0, t.L[e] / (1.0 - t.pd[e]), 0.0)     # (keep the cells in range: they carried the factor 1 - Pd)
            t.pd[e] = 1.0
    t.pd[0] = 1.0
    T.append(t)
    # exact mode with Pd == 1 rows (the default mode's Murty table would hold log(0) = -inf: the oracle's rule, pinned in test_murty_edges)
    t = pack(rng, [complete(3, 8), random_connected(rng, 12, 5, 0.5), complete(9, 9)], clutter=0.5, miss=(0.05, 0.9), note="Pd == 1, exact mode")
    for rows, cols in pr.components(t.L):
        if len(rows) + len(cols) > 8:
            e = rows[1]
            t.L[e] = np.where(t.L[e] != 0, t.L[e] / (1.0 - t.pd[e]), 0.0)
            t.pd[e] = 1.0
    T.append(t)
    # denormal cells.  (a) a denormal cell is the only link between row 2 and the pair (row 1, column 1): flushed to zero, row 2 would
    # be a second zero partition, pooled with Pd instead of 1 - Pd, and the last component would be dropped; (b) a 1 x 1 partition
    # with Pd == 1 whose sum IS its denormal cell, after partitions large enough that the running product stays normal
    L = np.zeros((8, 8))
    pd = np.array([0.5, 0.6, 0.7, 0.5, 0.5, 0.5, 0.5, 1.0])
    L[1, 1] = 0.3; L[2, 1] = DENORMAL * 3
    for e in (3, 4, 5, 6):
        L[e, e] = 10.0 ** (4 + e)
    L[7, 7] = DENORMAL
    L[0, 0] = 0.2; L[0, 2] = 5e-324                                           # (the smallest denormal joins column 2 to row 0)
    T.append(Table(L, pd, 0.25, "denormal cells"))
    for nZ in (0, 1, 5, 64):
        T.append(Table(np.zeros((0, nZ)), np.zeros(0), 0.7, "nE = 0"))
    for nE in (1, 7, 64):
        T.append(Table(np.zeros((nE, 0)), 1.0 - 10.0 ** rng.uniform(-1.3, -0.05, nE), 0.7, "nZ = 0"))
    return T


_FAMILIES = {}


def families():
    """name -> [Table]; built once."""
    if not _FAMILIES:
        _FAMILIES.update(shapes=family_shapes(), boundary=family_boundary(), exact=family_exact(), fallthrough=family_fallthrough(),
                         components=family_components(), chains=family_chains(), values=family_values())
    return _FAMILIES


# which (family, table index) run in which mode against the exact reference; everything else is listed in ORACLE_ONLY / REFUSED
ORACLE_ONLY = {("chains", 2)}
REFUSED = {("chains", 3)}
EXACT_MODE_ONLY = {("exact", k) for k in range(8)} | {("chains", 1), ("values", 1)}


def cases(exact):
    """[(family, index, Table)] that run in the given mode against the exact reference."""
    out = []
    for name, tabs in families().items():
        for k, t in enumerate(tabs):
            if (name, k) in ORACLE_ONLY or (name, k) in REFUSED:
                continue
            if not exact and (name, k) in EXACT_MODE_ONLY:
                continue
            out.append((name, k, t))
    return out


_REF = {}


def reference(name, k, exact):
    """(value, [(index, kind, rows, cols, value)]) of one table by the exact reference; computed once."""
    key = (name, k, bool(exact))
    if key not in _REF:
        t = families()[name][k]
        _REF[key] = pr.partition_likelihood(t.L, t.pd, t.clutter, exact=exact, factors=True)
    return _REF[key]


def n_murty(name, k, exact):
    return sum(1 for f in reference(name, k, exact)[1] if f[1] == "murty")


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else (0.0 if a == 0 else math.inf)


def oracle_dev(name, k):
    return ORACLE_DEV_DENORMAL if (name, k) == ("values", 2) else ORACLE_DEV_MEASURED


def bound_vs_exact(name, k, exact):
    m = n_murty(name, k, exact)
    rest = len(reference(name, k, exact)[1]) - m
    return m * MURTY_VS_EXACT + (8 * oracle_dev(name, k) if rest else 0.0)


def bound_vs_oracle(m, rest=True, dev=ORACLE_DEV_MEASURED):
    # both sides within their bounds of the exact value: the device's working bound + the oracle's measured deviation
    return m * MURTY_VS_ORACLE + (9 * dev if rest else 0.0)


# ---- CPU: the reference, the oracle, the certification ------------------------------------------------------------------------

def test_rational_recurrence_equals_the_bruteforce_walk():
    """partial_assignment_sum against itertools over every partial assignment, r + c <= 10, complete and sparse, both orientations,
    with a Pd == 1 row -- equal as rationals."""
    rng = np.random.default_rng(5)
    for r, c in [(1, 1), (1, 7), (7, 1), (2, 6), (6, 2), (3, 5), (5, 3), (4, 4), (5, 5), (4, 6), (6, 4), (1, 9), (9, 1), (3, 7), (0, 3), (3, 0)]:
        for mask in ([complete(r, c), tree(rng, r, c)] if r and c else [np.zeros((r, c), dtype=bool)]):
            L = np.where(mask, 10.0 ** rng.uniform(-3, 1, (r, c)), 0.0)
            pd = rng.uniform(0.05, 0.99, r)
            if r > 1:
                pd[1] = 1.0
            rows, cols = list(range(r)), list(range(c))
            assert pr.partial_assignment_sum(L, pd, 0.37, rows, cols) == pr.bruteforce_partial_sum(L, pd, 0.37, rows, cols), (r, c)
            assert pr.count_matchings(L, rows, cols) == pr.count_matchings(L.T, cols, rows) >= 1


def test_reference_decides_every_murty_partition_it_is_asked():
    """Every Murty-200 partition of the cases held to the exact reference has <= 200 non-zero terms (the truncated sum is the whole
    sum) or r + c <= 10 (brute force over the extended table); both kinds occur."""
    how = set()
    for exact in (False, True):
        for name, k, t in cases(exact):
            for p, kind, rows, cols, v in reference(name, k, exact)[1]:
                if kind == "murty":
                    route = pr.murty200_route(t.L, t.pd, t.clutter, rows, cols)
                    assert route in ("all", "brute"), (name, k, len(rows), len(cols))
                    assert pr.count_matchings(t.L, rows, cols) <= 200 or len(rows) + len(cols) <= 10
                    how.add(route)
    assert how == {"all", "brute"}
    with pytest.raises(pr.Undecidable):
        t = families()["chains"][2]
        pr.partition_likelihood(t.L, t.pd, t.clutter)
    with pytest.raises(pr.Refused):
        t = families()["chains"][3]
        pr.partition_likelihood(t.L, t.pd, t.clutter)


def test_oracle_equals_the_exact_reference_on_every_table(ob):
    """ob.partition_likelihood on every table of every family, both modes: within ORACLE_DEV_MEASURED of the exact value where no
    Murty partition is involved (this is the measurement behind the device's working bound: the largest deviation is printed), and
    within 1e-12 per Murty partition where one is."""
    worst = {ORACLE_DEV_MEASURED: 0.0, ORACLE_DEV_DENORMAL: 0.0}
    for exact in (False, True):
        for name, k, t in cases(exact):
            want, fac = reference(name, k, exact)
            got = ob.partition_likelihood(t.L, t.pd, t.clutter, 1.0, exact=exact)[0]
            m = n_murty(name, k, exact)
            d = rel(got, want)
            if m == 0:
                worst[oracle_dev(name, k)] = max(worst[oracle_dev(name, k)], d)
                assert d <= oracle_dev(name, k), (name, k, exact, got, want, d)
            else:
                assert d <= m * MURTY_VS_EXACT + ORACLE_DEV_MEASURED, (name, k, exact, got, want, d)
    print("largest oracle deviation from the exact reference, tables without a Murty partition: %r" % worst)
    for const, seen in worst.items():
        assert seen >= const / 4, "the constant %.2e is stale: measured %.3e" % (const, seen)


def test_no_table_underflows():
    """No product leaves the normal range on the way: every prefix of every table's product lies in [1e-290, 1e290], and no factor
    is 0 -- so a wrong factor cannot hide in an underflow.  The partitions of the shapes family spread over many decades."""
    for exact in (False, True):
        for name, k, t in cases(exact):
            run = 1.0
            for p, kind, rows, cols, v in reference(name, k, exact)[1]:
                assert v > 0, (name, k, p)
                run *= v
                assert 1e-290 < run < 1e290, (name, k, p, run)
    vals = [f[4] for k in range(len(families()["shapes"])) for f in reference("shapes", k, False)[1]]
    assert min(vals) < 1e-20 and max(vals) > 1e2, (min(vals), max(vals))


def test_families_reach_what_they_claim():
    """From the tables alone."""
    F = families()
    plan = lambda t, exact=False: pr.plan(t.L, exact)
    # every packed table: 64 x 64, row 63 and column 63 in a non-zero partition somewhere in each family
    for name in ("shapes", "boundary", "exact", "components", "chains", "values"):
        assert any(t.L.shape == (64, 64) and t.L[63].any() and t.L[:, 63].any() for t in F[name]), name
    # shapes: all 28, each complete and each as a tree (r + c - 1 cells), all enumerated, nothing dropped
    seen = set()
    for t in F["shapes"]:
        pl = plan(t)
        assert not pl["zero"] and pl["n_partitions"] == len(pl["components"])
        for p, kind, rows, cols in pl["visited"]:
            assert kind == "enum"
            cells = int((t.L[np.ix_(rows, cols)] != 0).sum())
            if cells == len(rows) * len(cols):
                seen.add((len(rows), len(cols), "complete"))
            if cells == len(rows) + len(cols) - 1:
                seen.add((len(rows), len(cols), "tree"))
    assert {(r, c, k) for r, c in SHAPES28 for k in ("complete", "tree")} <= seen
    # boundary: each r + c = 8 shape enumerated in the 8-tables, and the same rows with one more column on the Murty route in the 9-tables
    for t9, t8 in ((F["boundary"][0], F["boundary"][1]), (F["boundary"][2], F["boundary"][3])):
        nine = {tuple(rows): cols for p, kind, rows, cols in plan(t9)["visited"] if kind == "murty"}
        eight = {tuple(rows): cols for p, kind, rows, cols in plan(t8)["visited"] if len(rows) + len(cols) == 8 and kind == "enum"}
        assert len(nine) == 7 and {len(r) for r in nine} == set(range(1, 8))
        for rows, cols in nine.items():
            assert len(rows) + len(cols) == 9 and rows in eight and len(eight[rows]) == len(cols) - 1, (rows, cols)
        assert not plan(t9)["zero"] and not plan(t8)["zero"]
        assert all(kind == "exact" for p, kind, rows, cols in plan(t9, True)["visited"] if len(rows) + len(cols) == 9)
    # exact: smaller side 1 .. 9 in both orientations (and 9 x 9), on the exact route
    got = set()
    for t in F["exact"]:
        for p, kind, rows, cols in plan(t, True)["visited"]:
            if kind == "exact":
                got.add((len(rows), len(cols)))
    assert {(k, m) for k, m in EXACT_LARGE.items()} | {(m, k) for k, m in EXACT_LARGE.items()} | {(9, 9)} <= got
    assert max(max(s) for s in got) >= 20
    k10, k9 = F["fallthrough"]
    assert [(len(r), len(c)) for p, kind, r, c in plan(k10, True)["visited"] if kind == "murty"] == [(10, 10)]
    assert [(len(r), len(c)) for p, kind, r, c in plan(k9, True)["visited"] if kind == "exact"] == [(9, 10)] and not any(
        kind == "murty" for p, kind, r, c in plan(k9, True)["visited"])
    # components: the counts, the position of the first zero partition, revisited singletons and dropped components
    C = [plan(t) for t in F["components"]]
    assert [len(c["components"]) for c in C[:5]] == [64, 65, 100, 92, 128]
    assert [len(c["zero"]) for c in C] == [0, 2, 72, 56, 128, 1, 1, 1]
    assert [c["combined"] for c in C[:3]] == [None, 63, 0] and 0 < C[3]["combined"] < 63 and C[4]["combined"] == 0 and C[5]["combined"] == 0
    assert C[6]["combined"] == len(C[6]["components"]) - 1 == 63 and C[7]["combined"] == len(C[7]["components"]) - 1 < 63
    assert C[1]["n_partitions"] == 64 and C[4]["n_partitions"] == 1
    for c in C[2:4]:
        vis = c["visited"]
        revisited = [v for v in vis if v[1] == "enum" and (not v[2] or not v[3])]
        dropped = c["components"][c["n_partitions"]:]
        assert len(revisited) >= 5 and all(len(v[2]) == 1 and not v[3] for v in revisited)      # (lone rows; a lone column is never inside the range)
        assert any(r and cc for r, cc in dropped), "no non-zero partition among the dropped trailing components"
        assert max(c["zero"]) >= 64 and min(c["zero"]) < 64          # zero partitions in both halves of the component arrays
    # chains: paths numbered from one end (each row's column neighbours carry higher numbers than its own earlier ones); their sizes
    sizes = lambda t, exact: sorted((len(r), len(c)) for p, kind, r, c in plan(t, exact)["visited"] if kind in ("murty", "exact"))
    assert sizes(F["chains"][0], False) == [(4, 5), (5, 4), (5, 5), (5, 6), (6, 5)]
    assert sizes(F["chains"][1], True) == [(5, 5), (8, 7), (8, 8), (9, 9), (9, 10), (10, 9)]
    assert all(kind != "murty" for p, kind, r, c in plan(F["chains"][1], True)["visited"])
    for t, shape in ((F["chains"][2], (32, 32)), (F["chains"][3], (33, 32))):
        big = [(r, c) for r, c in pr.components(t.L) if len(r) + len(c) > 8]
        assert [(len(r), len(c)) for r, c in big] == [shape]
        rows, cols = big[0]
        sub = t.L[np.ix_(rows, cols)] != 0
        assert sub.sum() == len(rows) + len(cols) - 1 and sub.sum(axis=1).max() == 2 and sub.sum(axis=0).max() == 2   # a path
        assert all(sub[i, i] for i in range(min(sub.shape)))                      # ... taken in ascending order from its first row
    # the limits no table can reach (module docstring), on every table here
    for tabs in F.values():
        for t in tabs:
            for exact in (False, True):
                pl = pr.plan(t.L, exact)
                assert pl["n_partitions"] <= 64
                assert pl["combined"] is None or (pl["combined"] <= 63 and pl["combined"] < pl["n_partitions"])
    # values
    V = F["values"]
    assert (V[0].pd == 1.0).sum() >= 8 and V[0].pd[0] == 1.0 and plan(V[0])["combined"] == 0 and len(plan(V[0])["zero"]) == 1
    assert (V[1].pd == 1.0).sum() == 3
    d = V[2]
    assert 0 < d.L[2, 1] < 2.3e-308 and d.L[0, 2] == 5e-324 and not plan(d)["zero"]
    flushed = np.where(np.abs(d.L) < 2.3e-308, 0.0, d.L)
    assert len(pr.plan(flushed)["zero"]) == 4 and pr.partition_likelihood(flushed, d.pd, d.clutter) != reference("values", 2, False)[0]
    assert [t.L.shape for t in V[3:]] == [(0, 0), (0, 1), (0, 5), (0, 64), (1, 0), (7, 0), (64, 0)]
    assert reference("values", 5, False)[0] == 0.7 ** 5 or rel(reference("values", 5, False)[0], 0.7 ** 5) < 1e-15


# ---- GPU: the hook against the exact reference and the oracle --------------------------------------------------------------------

def run_hook(pkg, tables, exact, n=32):
    dev = pkg.RBPHDFilter(n, gm_capacity=64)
    try:
        dev.set_partition_mode(exact)
        w0 = dev.get_weights()
        out = np.zeros(len(tables))
        for cl in sorted({t.clutter for t in tables}):      # (one launch per clutter value of the family)
            idx = [i for i, t in enumerate(tables) if t.clutter == cl]
            out[idx] = dev.partition_likelihoods([tables[i].L for i in idx], [tables[i].pd for i in idx], cl)
        assert np.array_equal(dev.get_weights(), w0), "the hook must leave the weights as they were"
        return out
    finally:
        dev.close()


FAMILY_NAMES = ["shapes", "boundary", "exact", "fallthrough", "components", "chains", "values"]


HOOK_RUNS = [(name, exact) for name in FAMILY_NAMES for exact in (False, True) if exact or name != "exact"]    # (the exact family: that mode only)


@pytest.mark.gpu
@pytest.mark.parametrize("name,exact", HOOK_RUNS, ids=["%s-%s" % (n, "exact" if e else "murty200") for n, e in HOOK_RUNS])
def test_hook_equals_the_exact_reference_and_the_oracle(pkg, ob, name, exact):
    sel = [(k, t) for n_, k, t in cases(exact) if n_ == name]
    assert sel
    got = run_hook(pkg, [t for k, t in sel], exact)
    for (k, t), g in zip(sel, got):
        want = reference(name, k, exact)[0]
        orc = ob.partition_likelihood(t.L, t.pd, t.clutter, 1.0, exact=exact)[0]
        m = n_murty(name, k, exact)
        rest = len(reference(name, k, exact)[1]) > m
        print("%s[%d] %s exact=%d: hook %.17g exact %.17g (rel %.2e, bound %.2e) oracle rel %.2e" % (
            name, k, t.note, exact, g, want, rel(g, want), bound_vs_exact(name, k, exact), rel(g, orc)))
        assert rel(g, want) <= bound_vs_exact(name, k, exact) <= CEILING, (name, k, t.note, g, want)
        assert rel(g, orc) <= bound_vs_oracle(m, rest, oracle_dev(name, k)) <= CEILING, (name, k, t.note, g, orc)


@pytest.mark.gpu
def test_smaller_side_ten_falls_through_to_murty_in_exact_mode(pkg):
    """Exact mode: the 9 x 10 table leaves the handle without Murty work (rfsgpu_murty_seen == 0), the 10 x 10 one queues a job; its
    sum equals the default mode's (the same Murty-200 job) and the exact value (101 terms)."""
    import ctypes as C
    k10, k9 = families()["fallthrough"]
    lib = pkg.load_library()
    lib.rfsgpu_murty_seen.restype = C.c_int
    dev = pkg.RBPHDFilter(8, gm_capacity=64)
    try:
        dev.set_partition_mode(True)
        v9 = dev.partition_likelihoods([k9.L], [k9.pd], k9.clutter)[0]
        assert lib.rfsgpu_murty_seen(dev._h) == 0
        assert rel(v9, reference("fallthrough", 1, True)[0]) <= WORKING
        v10 = dev.partition_likelihoods([k10.L], [k10.pd], k10.clutter)[0]
        assert lib.rfsgpu_murty_seen(dev._h) == 1
        dev.set_partition_mode(False)
        v10d = dev.partition_likelihoods([k10.L], [k10.pd], k10.clutter)[0]
        assert rel(v10, v10d) <= MURTY_VS_EXACT                 # (the first launch ran the light instance of the job kernel, this one the capped)
        assert rel(v10, reference("fallthrough", 0, True)[0]) <= MURTY_VS_EXACT + WORKING
    finally:
        dev.close()


@pytest.mark.gpu
def test_path_of_murty_dimension_64_and_the_refusal_beyond(pkg, ob):
    """The 32 + 32 path is one Murty-200 job of dimension 64 = MURTY_MAXN: against the ORACLE ONLY (its 200 best of > 10^6 terms are
    the solver's to rank; the exact reference does not decide it).  The 33 + 32 path is refused -- ERRBIT_MURTY, named by
    rfsgpu_last_error, no number -- in both modes (smaller side 32 > 9), and the handle works afterwards."""
    t64, t65 = families()["chains"][2], families()["chains"][3]
    dev = pkg.RBPHDFilter(8, gm_capacity=64)
    try:
        got = dev.partition_likelihoods([t64.L], [t64.pd], t64.clutter)[0]
        orc, mc, _ = ob.partition_likelihood(t64.L, t64.pd, t64.clutter, 1.0)
        assert mc == 1
        print("32 + 32 path: hook %.17g oracle %.17g rel %.2e" % (got, orc, rel(got, orc)))
        assert rel(got, orc) <= bound_vs_oracle(1)
        for exact in (False, True):
            dev.set_partition_mode(exact)
            with pytest.raises(pkg.capi.EngineError, match="MURTY_MAXN") as e:
                dev.partition_likelihoods([t64.L, t65.L], [t64.pd, t65.pd], t65.clutter)
            assert e.value.status == pkg.capi.ERR_UNSUPPORTED
        dev.set_partition_mode(False)
        again = dev.partition_likelihoods([t64.L], [t64.pd], t64.clutter)[0]
        assert rel(again, orc) <= bound_vs_oracle(1)
    finally:
        dev.close()


@pytest.mark.gpu
def test_hook_refuses_bad_arguments(pkg):
    dev = pkg.RBPHDFilter(4, gm_capacity=64)
    try:
        one = np.full((1, 1), 0.5)
        with pytest.raises(pkg.capi.EngineError) as e:
            dev.partition_likelihoods([one] * 5, [[0.5]] * 5, 0.5)              # more tables than particles
        assert e.value.status == pkg.capi.ERR_INVALID
        with pytest.raises(pkg.capi.EngineError) as e:
            dev.partition_likelihoods([np.zeros((65, 1))], [np.full(65, 0.5)], 0.5)
        assert e.value.status == pkg.capi.ERR_INVALID
        with pytest.raises(pkg.capi.EngineError) as e:
            dev.partition_likelihoods([np.zeros((1, 65))], [[0.5]], 0.5)
        assert e.value.status == pkg.capi.ERR_INVALID
    finally:
        dev.close()
    batch = pkg.FilterBatch(2, 4, gm_capacity=64)        # a filter batch has its own calls: refused, its weights untouched
    try:
        w0 = batch.get_weights()
        with pytest.raises(pkg.capi.EngineError) as e:
            pkg.capi.CFilter.partition_likelihoods(batch, [np.full((1, 1), 0.5)], [[0.5]], 0.5)
        assert e.value.status == pkg.capi.ERR_UNSUPPORTED
        assert np.array_equal(batch.get_weights(), w0)
    finally:
        batch.close()


# ---- the limits through the real kernels -------------------------------------------------------------------------------------

def limit_scenario(sc, n_eval=64, seed=1, n=8):
    """8 particles, 64 measurements (all detections), 64 evaluation points; half of the 136 landmarks lie outside the field of view
    (Pd = 0: they keep their weight and sit BETWEEN the candidates in the sorted order)."""
    return sc.make_scenario(n, 136, 64, seed=seed, frac_in_fov=0.5, weights=(0.8, 1.0), n_eval=n_eval, n_clutter=0, params=dict(min_weight=0.5))


def selected_ranks(P, pose, w, mu):
    """The selection rule of np_importance_weight (tests/test_oracle_numpy.py): the sorted ranks of the evaluation points."""
    from tests.support.prefilter_reference import np_pd
    order = np.argsort(-w, kind="stable")
    ranks = []
    for r, m in enumerate(order):
        if w[m] < P["min_weight"]:
            break
        if np_pd(P, np.linalg.norm(mu[m] - pose[:2]))[0] > 0:
            ranks.append(r)
        if len(ranks) >= min(P["n_eval"], len(w)):
            break
    return ranks


NUMPY_PARTICLES = (0, 3)      # the two particles of the scenario that pick 64 evaluation points
_NUMPY = {}


def numpy_weights(sc):
    """particle -> (ranks of its evaluation points, its weight after one update from weight 1) by np_update_map + np_importance_weight:
    numpy / scipy from the equations, nothing of the device or the oracle.  Computed once."""
    if not _NUMPY:
        from tests.support.prefilter_reference import np_update_map
        from tests.test_oracle_numpy import np_importance_weight
        scen = limit_scenario(sc)
        P = scen["params"]
        cov = np.asarray(scen["pose_cov"], dtype=np.float64).reshape(3, 3)
        for i in NUMPY_PARTICLES:
            w, wp, mu, Sg, *_ = np_update_map(P, scen["poses"][i], scen["pose_cov"], scen["w"][i], scen["mean"][i], scen["cov"][i], scen["Z"])
            w, wp, mu, Sg = (np.asarray(x) for x in (w, wp, mu, Sg))
            _NUMPY[i] = (selected_ranks(P, scen["poses"][i], w, mu), np_importance_weight(P, scen["poses"][i], cov, w, wp, mu, Sg, scen["Z"], 1.0))
    return _NUMPY


def check_against_numpy(sc, weights):
    """The device's raw weights of NUMPY_PARTICLES against the numpy formulation, at the standing 1e-9."""
    for i, (ranks, want) in numpy_weights(sc).items():
        assert abs(weights[i] / want - 1) <= 1e-9, (i, weights[i], want)


def test_limit_scenario_selects_64_points_across_rank_chunks(ob, sc):
    """np_update_map + the selection rule: particles 0 and 3 pick 64 evaluation points, the last one beyond sorted rank 127 --
    select_eval_points (weighting.h) collects them over three 64-rank chunks, the Pd = 0 landmarks in between.  And the oracle's
    weights of those particles equal np_importance_weight's to 1e-9 (64 x 64 tables: the oracle pinned where it never was)."""
    scen = limit_scenario(sc)
    orc = ob.OracleFilter(scen["n"])
    sc.load_scenario(orc, scen)
    orc.update(scen["Z"])
    wo = orc.get_weights()
    for i, (ranks, want) in numpy_weights(sc).items():
        assert len(ranks) == 64 and ranks[-1] >= 128 and ranks[63] - ranks[0] > 64, (i, len(ranks), ranks[-1])
        assert abs(wo[i] / want - 1) <= 1e-9, (i, wo[i], want)


STEP_PATHS = [("stepwise", {}), ("unfused", {"RFSGPU_FUSED_STEP": "0"}), ("fused_wpp2", {"RFSGPU_STEP_WPP": "2"}), ("fused_wpp3", {"RFSGPU_STEP_WPP": "3"}),
              ("update_async", {})]


@pytest.mark.gpu
@pytest.mark.parametrize("path_name,env", STEP_PATHS, ids=[p[0] for p in STEP_PATHS])
def test_64_measurements_and_64_evaluation_points_through_the_step(pkg, ob, sc, path_name, env, monkeypatch):
    """nZ = nE = 64 through the weighting kernels themselves, each way a step of one handle can run: weights against the oracle
    (1e-9 normalised, 1e-8 raw as tests/test_gpu_parity.py) and against np_importance_weight on np_update_map's maps (1e-9).  The launch
    variant of each run is recorded and asserted: the forced waves per particle took effect, the unfused run ran three kernels."""
    for k in ("RFSGPU_FUSED_STEP", "RFSGPU_STEP_WPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scen = limit_scenario(sc)
    dev = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=512)
    orc = ob.OracleFilter(scen["n"])
    try:
        for f in (dev, orc):
            sc.load_scenario(f, scen)
        if path_name == "stepwise":
            dev.update_map(scen["Z"])
            for i, (ranks, _) in numpy_weights(sc).items():      # the device's own maps give the same evaluation points
                g = dev.export_gm(i)
                assert selected_ranks(scen["params"], scen["poses"][i], np.asarray(g[0]), np.asarray(g[2])) == ranks
            dev.importance_weighting()
            orc.update_map(scen["Z"])
            orc.importance_weighting()
        else:
            if path_name in ("unfused", "update_async"):
                dev.update_async(scen["Z"])
            else:
                dev.step_async(scen["Z"], False)
            dev.synchronize()
            orc.update(scen["Z"])
            variant = dev.last_step_variant()
            print(path_name, "launch variant", variant)
            if path_name == "unfused":
                assert variant == (0, 0, 0, 0), variant
            else:
                assert variant[3] >= 1, variant                   # a fused step
                if "RFSGPU_STEP_WPP" in env:
                    assert variant[0] == int(env["RFSGPU_STEP_WPP"]), variant
                else:
                    assert variant[0] in (2, 3), variant
        wd, wo = dev.get_weights(), orc.get_weights()
        assert np.all(np.isfinite(wd)) and np.all(wd > 0)
        np.testing.assert_allclose(wd / wd.sum(), wo / wo.sum(), rtol=1e-9, atol=0)
        np.testing.assert_allclose(wd, wo, rtol=1e-8, atol=0)
        check_against_numpy(sc, wd)
    finally:
        dev.close()
        orc.close()


@pytest.mark.gpu
def test_64_measurements_and_64_evaluation_points_in_a_filter_batch(pkg, ob, sc):
    """The same scenario as filter 1 of a batch of three (the batch kernels carve their LDS for the largest filter: 64 evaluation
    points x 64 measurements), between a small filter and a second 64 x 64 one: every filter against its oracle, filter 1 against numpy."""
    nP = 8
    scens = [sc.make_scenario(nP, 40, 12, seed=31), limit_scenario(sc), limit_scenario(sc, seed=2)]
    nF = len(scens)
    batch = pkg.FilterBatch(nF, nP, gm_capacity=512)
    orcs = [ob.OracleFilter(nP) for _ in scens]
    try:
        pcov = [np.asarray(s_["pose_cov"], dtype=np.float64) for s_ in scens]
        batch.set_poses(np.vstack([s_["poses"] for s_ in scens]), np.vstack([np.tile(c.ravel(), (nP, 1)) for c in pcov]))
        batch.set_weights(np.concatenate([s_["particle_w"] for s_ in scens]))
        for b, s_ in enumerate(scens):
            P = s_["params"]
            cfg = batch.default_filter_config()
            cfg.birthGaussianWeight = P["birth_w"]
            cfg.newGaussianCreateInnovMDThreshold = P["new_gaussian_md"]
            cfg.importanceWeightingEvalPointCount = P["n_eval"]
            cfg.importanceWeightingEvalPointGuassianWeight = P["min_weight"]
            cfg.importanceWeightingMeasurementLikelihoodMDThreshold = P["weighting_md"]
            cfg.gaussianMergingThreshold = P["merge_thr"]
            cfg.gaussianMergingCovarianceInflationFactor = P["merge_infl"]
            cfg.gaussianPruningThreshold = P["prune_thr"]
            cfg.useClusterProcess = P["use_cluster"]
            batch.configure(b, cfg, R=P["R"], Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"],
                            kf=(P["kf_range"], P["kf_bearing"]), Q=P["Q_lm"])
            for i in range(nP):
                batch.import_gm(b * nP + i, s_["w"][i], s_["mean"][i], s_["cov"][i])
            sc.load_scenario(orcs[b], s_)
        batch.cycle_async(None, [s_["Z"] for s_ in scens], normalize=False)
        batch.synchronize()
        wb = batch.get_weights()
        for b, (s_, o) in enumerate(zip(scens, orcs)):
            o.update(s_["Z"])
            wd, wo = wb[b * nP:(b + 1) * nP], o.get_weights()
            assert np.all(np.isfinite(wd)) and np.all(wd > 0)
            np.testing.assert_allclose(wd / wd.sum(), wo / wo.sum(), rtol=1e-9, atol=0, err_msg="filter %d" % b)
            np.testing.assert_allclose(wd, wo, rtol=1e-8, atol=0, err_msg="filter %d" % b)
        check_against_numpy(sc, wb[nP:2 * nP])
    finally:
        batch.close()
        for o in orcs:
            o.close()


def vp_limit_scenario(sc, n_eval=64):
    """Victoria Park: 64 measurements, 80 landmarks (64 in view), no weight threshold on the evaluation points."""
    return sc.make_vp_scenario(6, 80, 64, seed=6, params=dict(n_eval=n_eval, min_weight=0.0))


@pytest.mark.gpu
def test_victoria_park_with_64_measurements_and_64_evaluation_points(pkg, ob, sc):
    """vp.h carves its own LDS view (vp_weight_lds_bytes_per_wave) for the same rfs_partitions_wave: 64 x 64 stepwise and through the
    step, against the oracle.  That 64 evaluation points are reached is shown on the device itself: with 65 requested the same scenario
    is refused (some particle filled all 64)."""
    VP = pkg.capi.MODEL_VICTORIAPARK_3D
    scen = vp_limit_scenario(sc)
    for how in ("stepwise", "update"):
        dev = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=512, model=VP)
        orc = ob.OracleFilter(scen["n"], model=VP)
        try:
            for f in (dev, orc):
                sc.load_scenario(f, scen)
                if how == "stepwise":
                    f.update_map(scen["Z"])
                    f.importance_weighting()
                else:
                    f.update(scen["Z"])
            wd, wo = dev.get_weights(), orc.get_weights()
            assert np.all(np.isfinite(wd)) and np.all(wd > 0)
            np.testing.assert_allclose(wd / wd.sum(), wo / wo.sum(), rtol=1e-9, atol=0, err_msg=how)
            np.testing.assert_allclose(wd, wo, rtol=1e-8, atol=0, err_msg=how)
        finally:
            dev.close()
            orc.close()
    scen65 = vp_limit_scenario(sc, n_eval=65)
    dev = pkg.RBPHDFilter(scen65["n"], device_id=0, gm_capacity=512, model=VP)
    try:
        sc.load_scenario(dev, scen65)
        dev.update_map(scen65["Z"])
        with pytest.raises(pkg.capi.EngineError, match="RFSGPU_MAX_EVAL") as e:
            dev.importance_weighting()
        assert e.value.status == pkg.capi.ERR_UNSUPPORTED
    finally:
        dev.close()


@pytest.mark.gpu
def test_65_evaluation_points_are_refused(pkg, sc):
    """importanceWeightingEvalPointCount = 65 with 64 eligible points in some particle: RFSGPU_ERR_UNSUPPORTED, not a truncated set."""
    scen = limit_scenario(sc, n_eval=65)
    dev = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=512)
    try:
        sc.load_scenario(dev, scen)
        dev.update_map(scen["Z"])
        with pytest.raises(pkg.capi.EngineError, match="RFSGPU_MAX_EVAL") as e:
            dev.importance_weighting()
        assert e.value.status == pkg.capi.ERR_UNSUPPORTED
    finally:
        dev.close()
