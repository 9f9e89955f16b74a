"""Murty-200 partition sums (include/RBPHDFilter.hpp:942-959) on the tables where the device search can go wrong: dimensions at
every boundary of its forms (MURTY_WARM_N / HQ_N 16, MURTY_LDS_N 20, MURTY_N 64), dense exact ties, rankings that cross the
-1000 cut, non-finite cells, and partitions whose search tree outgrows the node pool.  The finite cases are held to exact sums
computed without the oracle (tests/support/murty_reference.py); the non-finite ones to the oracle, which restates the
reference's solver and its failure rule.

Device tests go through rfsgpu_murty_partition_sums (the step's post kernel, murty_jobs_kernel) twice per handle: the first
call runs the light instance, the second the capped one a filter uses after it has shown Murty work."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import murty_reference as mr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def oracle_sum(ob, C, nR, nC):
    """The reference's loop over the oracle's Murty: add exp(score) until rank == -1, 200 terms, or a score below -1000
    (a NaN score is not below -1000: it is added)."""
    s, _ = ob.murty(np.asarray(C, dtype=np.float64), nR, nC, kmax=200)
    t = 0.0
    for x in s:
        if x < mr.BIG_NEG:
            break
        t += math.exp(x)
    return t


def random_extended_table(rng, nR, nC, kind):
    """An extended table as RBPHDFilter.hpp:907-940 builds it: 'random' log-likelihoods, 'tied' (quantised to a few levels, so
    many assignments score exactly alike) or 'floored' (most real cells at -1000)."""
    n = nR + nC
    C = np.full((n, n), mr.BIG_NEG)
    q = lambda x: np.round(np.asarray(x) * 2.0**20) / 2.0**20    # (a grid: every score exact, whatever order it is added in)
    if kind == "random":
        L = q(-rng.uniform(0.0, 4.0, (nR, nC)))
    elif kind == "tied":
        L = -rng.integers(0, 3, (nR, nC)).astype(np.float64)
    else:
        L = np.where(rng.random((nR, nC)) < 0.6, mr.BIG_NEG, q(-rng.uniform(0.0, 4.0, (nR, nC))))
    C[:nR, :nC] = L
    for r in range(nR):
        C[r, nC + r] = q(-rng.uniform(0.1, 3.0)) if kind != "tied" else -1.0
    for c in range(nC):
        C[nR + c, c] = q(-rng.uniform(0.1, 3.0)) if kind != "tied" else -2.0
    C[nR:, nC:] = 0.0
    return C


# ---- the references against the fixture and the oracle (CPU) ----------------------------------------------------------------

def test_partial_bruteforce_equals_the_reference_fixture():
    """tests/golden/murty_extended_ranked.json: the reference's BruteForceLinearAssignment over all n! assignments."""
    import json
    with open(os.path.join(HERE, "golden", "murty_extended_ranked.json")) as fh:
        cases = json.load(fh)
    for c in cases:
        want = math.fsum(math.exp(s) for s in c["scores"])
        got = mr.partial_bruteforce_sum(np.array(c["C"]), c["nR"], c["nC"])
        assert abs(got - want) <= 1e-13 * want, (c["nR"], c["nC"], got, want)


@pytest.mark.parametrize("kind", ["random", "tied", "floored"])
def test_partial_bruteforce_equals_the_oracle(ob, kind):
    rng = np.random.default_rng({"random": 1, "tied": 2, "floored": 3}[kind])
    for nR, nC in [(1, 1), (2, 3), (3, 4), (4, 4), (5, 3), (3, 5), (6, 2), (2, 7), (5, 5), (9, 1), (1, 9), (10, 0), (0, 10)]:
        C = random_extended_table(rng, nR, nC, kind)
        want = mr.partial_bruteforce_sum(C, nR, nC)
        got = oracle_sum(ob, C, nR, nC)
        assert abs(got - want) <= 1e-13 * want, (kind, nR, nC, got, want)


SEPARABLE_SHAPES = [(1, 0), (0, 1), (1, 1), (8, 8), (16, 16), (17, 3), (20, 1), (21, 0), (32, 32), (48, 16), (63, 1)]


@pytest.mark.parametrize("ties", [False, True])
def test_separable_tables_equal_the_oracle(ob, ties):
    rng = np.random.default_rng(11 + ties)
    for nR, nC in SEPARABLE_SHAPES:
        C, want = mr.separable_table(rng, nR, nC, ties=ties)
        got = oracle_sum(ob, C, nR, nC)
        assert want > 0 and abs(got - want) <= 1e-12 * want, (nR, nC, ties, got, want)


def test_separable_shift_puts_the_cut_inside_the_ranking(ob):
    C, want, scores = cut_table()
    assert 50 <= len(scores) <= 150 and want > 0
    got = oracle_sum(ob, C, 10, 8)
    assert abs(got - want) <= 1e-12 * want


def cut_table():
    """A separable 10 x 8 table shifted so that the -1000 cut falls at the 100th term, with the best terms still above
    fp64's underflow.  The cut itself cannot be seen in an fp64 sum: the terms next to it are exp(< -745) = 0, and at 1e-12
    only the terms within ~28 of the best count.  What a test of it checks is that a ranking which crosses -1000 runs without
    an error and gives the exact sum of the terms that matter."""
    rng = np.random.default_rng(77)
    _, _, s0 = mr.separable_table(np.random.default_rng(77), 10, 8, gap=400.0, return_scores=True)
    shift = -1000.0 - 0.5 * (s0[99] + s0[100])
    C, want, scores = mr.separable_table(rng, 10, 8, gap=400.0, shift=shift, return_scores=True)
    assert scores[0] > -700.0
    return C, want, scores


def nonfinite_variants(C0, nR, nC, ob):
    """The non-finite tables of the issue list, built from one finite table: name -> table."""
    _, a = ob.murty(C0, nR, nC, kmax=1)
    a = a[0]
    opt = [(r, int(a[r])) for r in range(nR) if a[r] < nC]
    off = max(((r, c) for r in range(nR) for c in range(nC) if a[r] != c), key=lambda rc: C0[rc])   # (a pair cell if there is one)
    V = {}
    C = C0.copy(); C[np.arange(nR), nC + np.arange(nR)] = -np.inf; V["miss_diagonal_minus_inf"] = C     # Pd = 1
    C = C0.copy(); C[nR + np.arange(nC), np.arange(nC)] = -np.inf; V["clutter_diagonal_minus_inf"] = C
    C = C0.copy(); C[1, :] = np.nan; V["nan_row"] = C
    C = C0.copy(); C[nR + 1, nC + 1] = np.nan; V["nan_zero_block_cell"] = C
    C = C0.copy(); C[nR:, nC:] = np.nan; V["nan_zero_block"] = C
    C = C0.copy(); C[opt[0]] = np.nan; V["nan_optimal_real_cell"] = C
    C = C0.copy(); C[off] = np.nan; V["nan_real_cell_off_the_optimum"] = C
    C = C0.copy(); C[:] = np.nan; V["all_nan"] = C
    return V


NONFINITE_SHAPES = [(5, 4), (9, 7), (12, 4)]


def test_oracle_sums_of_non_finite_tables(ob):
    """The reference's rule on non-finite cells, pinned: HungarianMethod::run offsets the table by its extreme cell
    (include/HungarianMethod.hpp:123-140), so a -inf cell turns the offset table into NaN / inf and the solver fails with
    'Cannot find alternating path' (:505-522); findNextBest then returns -1 and RBPHDFilter.hpp:953-955 adds nothing -- the
    partition's likelihood is 0.  The same happens when a row or the zero block has no finite cell.  A NaN cell the solver can
    go round is never chosen (every comparison with it is false): the sum is finite, at most that of the finite table, and
    below it when the NaN sits on the optimum."""
    rng = np.random.default_rng(5)
    for nR, nC in NONFINITE_SHAPES:
        C0, _ = mr.separable_table(rng, nR, nC)
        full = oracle_sum(ob, C0, nR, nC)
        V = nonfinite_variants(C0, nR, nC, ob)
        for name in ("miss_diagonal_minus_inf", "clutter_diagonal_minus_inf", "nan_row", "nan_zero_block", "all_nan"):
            assert oracle_sum(ob, V[name], nR, nC) == 0.0, (name, nR, nC)
        for name in ("nan_zero_block_cell", "nan_optimal_real_cell", "nan_real_cell_off_the_optimum"):
            s = oracle_sum(ob, V[name], nR, nC)
            assert 0.0 < s <= full * (1 + 1e-12), (name, nR, nC, s, full)
        assert oracle_sum(ob, V["nan_optimal_real_cell"], nR, nC) < 0.5 * full


# ---- the device against them ---------------------------------------------------------------------------------------------------

def dev_sums(dev, mats, nR, nC):
    return dev.murty_partition_sums(mats, list(nR), list(nC))


def check_both_instances(pkg, tables, shapes, want, rtol=1e-12):
    """Every table through both instances of the job kernel (the light one first): each sum equal to its exact value."""
    dev = pkg.RBPHDFilter(8, gm_capacity=64)
    try:
        out = []
        for _ in range(2):
            got = dev_sums(dev, tables, [s[0] for s in shapes], [s[1] for s in shapes])
            for g, w, s in zip(got, want, shapes):
                assert abs(g - w) <= rtol * w, (s, g, w)
            out.append(got)
        return out
    finally:
        dev.close()


# each boundary of the search: 1, 2; 16 | 17 (the small form: LDS table, warm starts, open nodes as a scanned array -- HQ_N,
# MURTY_WARM_N); 20 | 21 (sub-problems in the LDS tile or the arena, MURTY_LDS_N); 32, 33, 63, 64 (MURTY_N); nR > nC, nR < nC,
# nR = 0 and nC = 0.  (The cells are multiples of 2^-10, so every score is exact; the sum's only roundings are rfs_exp's
# 1e-14 and those of <= 200 additions: 1e-12 holds at every size.)
SIZE_SHAPES = [(1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (9, 7), (7, 9), (16, 0), (0, 16), (10, 7), (7, 10), (17, 0), (0, 17),
               (12, 8), (8, 12), (20, 0), (13, 8), (8, 13), (21, 0), (0, 21), (16, 16), (20, 12), (12, 20), (32, 0),
               (17, 16), (16, 17), (33, 0), (40, 23), (23, 40), (63, 0), (0, 63), (32, 32), (40, 24), (24, 40), (64, 0), (0, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("ties", [False, True])
def test_device_sums_at_every_size_boundary(pkg, ties):
    rng = np.random.default_rng(101 + ties)
    tabs = [mr.separable_table(rng, nR, nC, ties=ties) for nR, nC in SIZE_SHAPES]
    check_both_instances(pkg, [t[0] for t in tabs], SIZE_SHAPES, [t[1] for t in tabs])


TIE_SHAPES = [(6, 6), (8, 8), (12, 12), (32, 32)]   # n = 12, 16, 24, 64


def tied_tables():
    rng = np.random.default_rng(303)
    return [mr.separable_table(rng, nR, nC, ties=True) for nR, nC in TIE_SHAPES]


@pytest.mark.gpu
def test_device_sums_of_dense_ties(pkg):
    """Every pair of the table alike: C(m, j) exactly equal scores per level, the cut at 200 inside one block of them, and at
    n = 64 an open set past the shipped library's MURTY_HEAP_LDS = 512 LDS positions (the arena overflow path).  The sums are
    exact and the same bits call after call."""
    tabs = tied_tables()
    runs = check_both_instances(pkg, [t[0] for t in tabs], TIE_SHAPES, [t[1] for t in tabs])
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["small_queue", "cold"])
def test_device_sums_of_dense_ties_against_the_variant_libraries(pkg, tmp_path, variant):
    """The tied tables through a variant library in a child process: the same bits as the shipped library for the one with 16
    LDS positions of the open-node store (rfs-slam_amd/build.py: build_small_queue_variant), within 1e-12 for the one that
    solves every child from scratch (MURTY_WARM=0: the open nodes in the heap, equal terms added in another order)."""
    lib, exact = {"small_queue": (pkg.build_mod.SMALLQ_LIB, True), "cold": (pkg.build_mod.COLD_LIB, False)}[variant]
    if not os.path.exists(lib):
        pytest.skip("%s was not built (built by __graft_entry__.build())" % os.path.relpath(lib, ROOT))
    tabs = tied_tables()
    runs = check_both_instances(pkg, [t[0] for t in tabs], TIE_SHAPES, [t[1] for t in tabs])
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import __graft_entry__ as g; pkg = g.load_package(); pkg.engine.LIB = %r; "
            "from tests.test_murty_edges import tied_tables, TIE_SHAPES; tabs = tied_tables(); f = pkg.RBPHDFilter(8, gm_capacity=64); "
            "np.save(%r, np.stack([f.murty_partition_sums([t[0] for t in tabs], [s[0] for s in TIE_SHAPES], [s[1] for s in TIE_SHAPES]) for _ in range(2)])); "
            "print('variant ok')")
    out = os.path.join(str(tmp_path), "v.npy")
    p = subprocess.run([sys.executable, "-c", code % (ROOT, lib, out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "variant ok" in p.stdout, p.stderr[-3000:]
    for row in np.load(out):
        if exact:
            assert np.array_equal(row, runs[0]), (variant, row, runs[0])
        else:
            np.testing.assert_allclose(row, runs[0], rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_device_cut_and_early_stop(pkg):
    """A ranking that crosses the -1000 cut at its 100th term (cut_table: the cut itself is not visible in the sum); then a table whose cells all lie in [-1000, 1000] (the early stop on,
    murty_partition_sum_block) against the same table with one -1000.5 cell no assignment above the cut can take (the
    early stop off, the loop runs on to the cut): the same bits -- every term the early stop leaves out rounds to no change."""
    C, want, _ = cut_table()
    check_both_instances(pkg, [C], [(10, 8)], [want])
    rng = np.random.default_rng(9)
    shapes, tabs, want = [], [], []
    for nR, nC in [(5, 4), (9, 7), (12, 9), (20, 6)]:
        T, w = mr.separable_table(rng, nR, nC)
        assert T.min() == mr.BIG_NEG      # (cells of exactly -1000: the early stop stays on)
        r, c = [(r, c) for r in range(nR) for c in range(nC) if T[r, c] == mr.BIG_NEG][0]
        T2 = T.copy()
        T2[r, c] = -1000.5
        shapes += [(nR, nC), (nR, nC)]
        tabs += [T, T2]
        want += [w, w]
    runs = check_both_instances(pkg, tabs, shapes, want)
    for got in runs:
        assert np.array_equal(got[0::2], got[1::2]), got


NONFINITE_NAMES = ["miss_diagonal_minus_inf", "clutter_diagonal_minus_inf", "nan_row", "nan_zero_block_cell", "nan_zero_block",
                   "nan_optimal_real_cell", "nan_real_cell_off_the_optimum", "all_nan"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE_NAMES)
def test_device_sums_of_non_finite_tables_equal_the_oracle(pkg, ob, name):
    """Each non-finite table between finite jobs: its sum equals the oracle's (both NaN, or equal to 1e-12; a solve that fails
    at the root -- -inf on a diagonal, a row without a non-NaN cell -- is the reference's rank == -1, a partition likelihood of
    0, no error), and the finite neighbours come out with the same bits as in a call without it (nothing overwrote them).
    Small form (n <= 16) and the large one; each table on a fresh handle, so that it goes through the light instance (first
    call) and the capped one (second call), each compared with the neighbours' sums from the same instance."""
    rng = np.random.default_rng(5)
    fin_shapes = [(4, 3), (9, 7), (12, 8), (5, 5)]
    fin = [mr.separable_table(rng, nR, nC) for nR, nC in fin_shapes]
    ref = pkg.RBPHDFilter(8, gm_capacity=64)
    try:
        base = [dev_sums(ref, [t[0] for t in fin], [s[0] for s in fin_shapes], [s[1] for s in fin_shapes]) for _ in range(2)]
    finally:
        ref.close()
    for (nR, nC), (C0, _) in zip([(5, 4), (9, 7), (12, 9)], [mr.separable_table(rng, *s) for s in [(5, 4), (9, 7), (12, 9)]]):
        C = nonfinite_variants(C0, nR, nC, ob)[name]
        want = oracle_sum(ob, C, nR, nC)
        mats = [fin[0][0], fin[1][0], C, fin[2][0], fin[3][0]]
        shapes = [fin_shapes[0], fin_shapes[1], (nR, nC), fin_shapes[2], fin_shapes[3]]
        dev = pkg.RBPHDFilter(8, gm_capacity=64)
        try:
            for inst in range(2):        # 0: light instance, 1: capped
                got = dev_sums(dev, mats, [s[0] for s in shapes], [s[1] for s in shapes])
                if math.isnan(want):
                    assert math.isnan(got[2]), (name, nR, nC, inst, got[2])
                else:
                    assert abs(got[2] - want) <= 1e-12 * want, (name, nR, nC, inst, got[2], want)
                assert np.array_equal(np.delete(got, 2), base[inst]), (name, nR, nC, inst)
        finally:
            dev.close()


POOL_SHAPES = [(48, 16), (40, 24), (63, 1), (1, 63)]


@pytest.mark.gpu
@pytest.mark.parametrize("ties", [False, True])
def test_device_sums_where_the_search_tree_is_widest(pkg, ties):
    """nR up to 63: an expansion at partition index p has nR - p children, against MURTY_MAX_NODES = 1 + 200 x 32
    (include/rfsgpu.h).  Each table alone, both instances: the exact sum for the shapes of POOL_SHAPES (random pairs: their
    trees stay inside the pool).  Then a tied 48 x 16 table whose pairs take rows 0 .. 15 -- every one of the 200 pops expands
    at least 33 children, more than the pool holds -- must be refused with the pool's own error, not truncated."""
    rng = np.random.default_rng(707 + ties)
    for nR, nC in POOL_SHAPES:
        C, want = mr.separable_table(rng, nR, nC, ties=ties)
        dev = pkg.RBPHDFilter(8, gm_capacity=64)
        try:
            for _ in range(2):
                got = dev_sums(dev, [C], [nR], [nC])[0]
                assert abs(got - want) <= 1e-12 * want, (nR, nC, ties, got, want)
        finally:
            dev.close()
    if ties:
        C, _ = mr.separable_table(rng, 48, 16, ties=True, first_rows=True)
        dev = pkg.RBPHDFilter(8, gm_capacity=64)
        try:
            for _ in range(2):
                with pytest.raises(pkg.capi.EngineError, match="outgrew the node pool"):
                    dev_sums(dev, [C], [48], [16])
        finally:
            dev.close()


def raw_weights_pair(pkg, ob, sc, scen, cap):
    dev = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=cap)
    orc = ob.OracleFilter(scen["n"])
    for f in (dev, orc):
        sc.load_scenario(f, scen)
        f.update_map(scen["Z"])
        f.importance_weighting()
    return dev, orc


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(seed=21, n_eval=25, weighting_md=10.0), dict(seed=22, n_eval=60, weighting_md=12.0)])
def test_device_weights_with_pd_one_equal_the_oracle(pkg, ob, sc, kw):
    """Pd = 1: every miss cell is log(1 - Pd) = -inf (weighting.h), the reference's solver fails at the root of every Murty
    partition, and those particles' likelihoods are 0.  The update must not raise; the raw weights equal the oracle's -- 0
    exactly where its are, within 1e-8 elsewhere (not normalised: nearly every weight is 0)."""
    scen = sc.make_scenario(24, 60, 30, weights=(0.8, 1.0), params=dict(Pd=1.0), **kw)
    dev, orc = raw_weights_pair(pkg, ob, sc, scen, cap=512)
    try:
        assert orc.murty_calls() > 10, "scenario does not reach the Murty path"
        wd, wo = dev.get_weights(), orc.get_weights()
        assert np.array_equal(wd == 0.0, wo == 0.0), (wd, wo)
        nz = wo != 0.0
        np.testing.assert_allclose(wd[nz], wo[nz], rtol=1e-8, atol=0)
    finally:
        dev.close()
