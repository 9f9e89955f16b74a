"""The merge's speculative replay on planted conflict structures ("planted replay structures").

Phase 2 of gm_merge_particle (csrc/merge_prune.h) replays up to 64 candidate rows per round, one per lane, against the states the
round started with, and then validates: claims in the row records, the alive / claimed fixed point, the prefix commit, the sub-round
re-walks and seq_replay.  The Victoria Park merge (csrc/vp.h, N <= 64) has the same shape: every lane walks its row against the
initial mixture, ordered validation, serial_row for collisions.  The cases of tests/support/merge_replay_cases.py plant what those
stages must get right, at sizes around the 64-row round:

  chain   row k lives exactly when row k - 1 died (the fixed point needs as many trips as the chain is long);
  fan     k rows contest one entry (one wins; with private partners every loser must end as a + p from its INITIAL state);
  comb    every re-walk changes what the next row must do (d sub-rounds, each settling one row);
  family 4  dead and overflowing rows inside a conflict (a row that leaves its list absorbed by a heavier one; the same row losing a
          claim and redone by the sequential scan; an unlistable row whose partner an earlier listable row takes).

The library exposes no replay counters.  The CPU tests below certify the INPUTS: every decision in exact arithmetic, the structure
(rows, isolated walks S, certified truth), the margins by which phase 1a lists or does not list and by which a walk stays inside or
leaves its slack, and that three deliberately wrong schedulers give other results.  They do not observe the branch the device took;
the GPU tests compare every particle of every case with the certified merge, numpy and the oracle."""
import functools

import numpy as np
import pytest

from tests.support import merge_replay_cases as mc
from tests.support import prefilter_reference as pr
from tests.test_prefilter_margins import GM_ATOL, GM_RTOL, _cap, _run_merge_paths, _scenario, value_atol

CHAIN_L = [3, 64, 65, 66, 129, 130]            # candidate rows: 2, 63, 64, 65, 128, 129
FAN_K = [2, 8, 63, 64, 65, 70]                 # 65, 70: the last rows fall into the second round and see a committed hole
FAN_PARTNERS_K = [8, 63]
COMB_D = [1, 3, 62, 63, 64, 70]                # rows: d + 1
CASES_2D = ([f"chain:{L}" for L in CHAIN_L] + ["chain2:33"] + [f"fan:{k}" for k in FAN_K] + [f"fanp:{k}" for k in FAN_PARTNERS_K]
            + [f"comb:{d}" for d in COMB_D] + ["absorbed_slack_row", "contested_slack_row", "contested_ring"])
CASES_VP = ["chain:63", "chain:64", "chain:65", "fan:30", "comb:30"]   # total sizes 63, 64 (lane-parallel scan), 65 (row by row), 31, 61
SCHEDULERS = ["W1", "W2", "W3"]


@functools.lru_cache(maxsize=None)
def case(name, dim=2):
    """Built once per session (the certification replays every merge in rationals).  The Victoria Park forms carry no anchors: that
    merge has no grid, and the mixture's size decides which scan runs."""
    kind, _, arg = name.partition(":")
    kw = dict(dim=dim, anchors=dim == 2)
    if kind == "chain":
        return mc.chain_case(int(arg), seed=100 + int(arg), **kw)
    if kind == "chain2":
        return mc.chain_case(int(arg), chains=2, seed=200 + int(arg), **kw)
    if kind == "fan":
        return mc.fan_case(int(arg), seed=300 + int(arg), **kw)
    if kind == "fanp":
        return mc.fan_case(int(arg), partners=True, seed=400 + int(arg), **kw)
    if kind == "comb":
        return mc.comb_case(int(arg), seed=500 + int(arg), **kw)
    if kind == "absorbed_slack_row":
        return mc.absorbed_slack_row_case(seed=5)
    if kind == "contested_slack_row":
        return mc.contested_slack_row_case(seed=5)
    if kind == "contested_ring":
        return mc.contested_ring_case(seed=9)
    raise ValueError(name)


def all_cases():
    return [(n, case(n)) for n in CASES_2D] + [("vp " + n, case(n, 3)) for n in CASES_VP]


def family(name):
    kind = name.replace("vp ", "").partition(":")[0]
    return {"chain2": "chain", "fanp": "fan", "absorbed_slack_row": "family4", "contested_slack_row": "family4",
            "contested_ring": "family4"}.get(kind, kind)


# ---- CPU: the planted cases have their structure --------------------------------------------------------------------------

def test_every_planted_case_is_certified_and_free_of_ties():
    """Every decision sits at least CERT_REL from the threshold in exact arithmetic (the planted ones: at least 0.1), the fp64 greedy
    merge makes the certified decisions, and no two weights tie, before or after merging: every later comparison is ordered."""
    for name, c in all_cases():
        assert c["margin"] >= pr.CERT_REL, name
        assert c["margin"] >= 0.1, (name, c["margin"])
        for i in range(len(c["w"])):
            mw, _, _ = pr.np_merge(c["w"][i], c["mean"][i], c["cov"][i], c["t"], c["f"])
            assert len(mw) == c["sizes"][i], name
            np.testing.assert_allclose(mw, c["merged_w"][i], rtol=1e-15)
            assert len(np.unique(c["w"][i])) == len(c["w"][i]), f"{name}: tied input weights"
            assert np.all(np.diff(c["w"][i]) < 0), f"{name}: the inputs are in merge order"
            assert len(np.unique(mw)) == len(mw), f"{name}: tied merged weights"
            assert np.min(mw) >= pr.PRUNE_T, f"{name}: a survivor below the prune threshold"


def _chain_predicates(name, c, i, chains):
    ro = c["roles"][i]
    idx = [ro[f"chain{k}"] for k in range(chains)]
    assert mc.rows(c, i) == sorted(m for ch in idx for m in ch[:-1]), name
    for ch in idx:
        assert ch == sorted(ch)                                            # weights descend along the chain
        for k in range(len(ch) - 1):
            assert mc.isolated(c, i, ch[k]) == [ch[k + 1]], (name, k)
            assert mc.truth(c, i, ch[k]) == ([ch[k + 1]] if k % 2 == 0 else []), (name, k)
    assert len(c["merges"][i]) == sum(len(ch) // 2 for ch in idx), name
    if chains == 2:                                                        # the two chains' rows alternate over the lanes
        rws = mc.rows(c, i)
        assert [m in idx[0] for m in rws[:8]] == [True, False] * 4, name


def _comb_predicates(name, c, i):
    r, e = c["roles"][i]["r"], [None] + c["roles"][i]["e"]                 # e[k] = e_k, k = 1 .. d
    d = len(r) - 1
    assert r == list(range(d + 1)) and e[1:] == list(range(d + 1, 2 * d + 1)), name
    assert mc.rows(c, i) == r, name
    for k in range(d + 1):
        assert mc.isolated(c, i, r[k]) == [e[max(k, 1)]], (name, k)
        assert mc.truth(c, i, r[k]) == ([e[k + 1]] if k < d else []), (name, k)
    assert len(c["merges"][i]) == d, name


def _fan_predicates(name, c, i, partners):
    ro = c["roles"][i]
    rw, cc = sorted(ro["row"]), ro["c"][0]
    assert cc > max(rw), name
    if not partners:
        assert mc.rows(c, i) == rw and len(rw) == len(ro["row"]), name
        for a in rw:
            assert mc.isolated(c, i, a) == [cc], (name, a)
        assert c["merges"][i] == [(rw[0], cc)], name                       # exactly one merge: the first row gets c
        return
    assert mc.rows(c, i) == rw + [cc], name                                # (c passes every p_i: a row too, dead in truth)
    assert min(ro["p"]) > cc, name
    for a, p in zip(ro["row"], ro["p"]):
        assert mc.isolated(c, i, a) == [cc, p], (name, a)
        assert mc.truth(c, i, a) == ([cc, p] if a == rw[0] else [p]), (name, a)
    assert not c["alive"][i][cc] and mc.truth(c, i, cc) == [], name


def _family4_predicates(name, c, i):
    ro = c["roles"][i]
    rws = mc.rows(c, i)
    if name == "absorbed_slack_row":
        for h, a, b, cc in zip(ro["H"], ro["A"], ro["B"], ro["C"]):
            assert h < a < b < cc and a in rws, name
            assert mc.truth(c, i, h) == [a, b, cc], name                  # the heavier row absorbs A (and then A's partners)
            assert mc.isolated(c, i, a) == [b, cc] and mc.truth(c, i, a) == [] and not c["alive"][i][a], name
    elif name == "contested_slack_row":
        assert max(ro["G"]) < min(ro["A"]), name                            # every G is an earlier row than every A
        for g, a, b0, b, cc in zip(ro["G"], ro["A"], ro["B0"], ro["B"], ro["C"]):
            assert g < a < b0 < b < cc and g in rws and a in rws, name
            assert mc.truth(c, i, g)[0] == b0 and mc.isolated(c, i, g) == mc.truth(c, i, g), name
            assert mc.isolated(c, i, a) == [b0, b, cc], name               # A claims B0 first, and loses it to G
            assert mc.truth(c, i, a) == [b, cc], name
    else:
        for q, ctr, e in zip(ro["Q"], ro["centre"], ro["E"]):
            assert q < ctr < e and q in rws and ctr in rws, name
            assert mc.isolated(c, i, q) == [e] and mc.truth(c, i, q) == [e], name
            assert e in mc.isolated(c, i, ctr) and e not in mc.truth(c, i, ctr) and len(mc.truth(c, i, ctr)) > 0, name


def test_every_family_has_its_structure():
    """rows, the isolated walks S and the certified truth of every case are the ones its family is defined by (see the constructors):
    chain S(a_k) = [a_{k+1}], truth (a_0, a_1), (a_2, a_3), ...; fan S(a_i) = [c], one merge; comb S(r_i) = [e_i], truth(r_i) =
    [e_{i+1}]; family 4 the dead, contested and unlistable rows."""
    for name, c in all_cases():
        base = name.replace("vp ", "")
        kind, _, arg = base.partition(":")
        for i in range(len(c["w"])):
            if kind in ("chain", "chain2"):
                _chain_predicates(name, c, i, 2 if kind == "chain2" else 1)
                n_rows = (int(arg) - 1) * (2 if kind == "chain2" else 1)
            elif kind == "comb":
                _comb_predicates(name, c, i)
                n_rows = int(arg) + 1
            elif kind in ("fan", "fanp"):
                _fan_predicates(name, c, i, kind == "fanp")
                n_rows = int(arg) + (kind == "fanp")
            else:
                _family4_predicates(base, c, i)
                continue
            assert len(mc.rows(c, i)) == n_rows, name
    # the sizes straddle the 64-row round: 63, 64 and 65 candidate rows in every family of the 2-D merge
    for names in (["chain:64", "chain:65", "chain:66"], ["fan:63", "fan:64", "fan:65"], ["comb:62", "comb:63", "comb:64"]):
        assert [len(mc.rows(case(n), 0)) for n in names] == [63, 64, 65]
    assert len(mc.rows(case("chain2:33"), 0)) == 64 and len(mc.rows(case("fanp:63"), 0)) == 64
    assert [case(n, 3)["w"].shape[1] for n in CASES_VP[:3]] == [63, 64, 65]        # the Victoria Park scan switches at 64 entries


def test_rows_stay_on_or_leave_their_lists_by_a_margin():
    """Phase 1a (merge_prune.h): entry a lists every j > a with |x_j - x_a| <= max(r_a, r_j) (+ the fp32 allowance 1.5 errAbs) as a
    survivor and every j within twice that as a reserve, r = t sqrt(tr S); a row with more than MERGE_ROW_SLOTS = 8 of them is not
    listed at all.  Its slack is half the distance to the nearest j > a beyond that, capped by cell edge - largest radius (- 3 errAbs);
    a walk whose path length plus radius growth reaches the slack goes to the sequential scan.

    Rows meant to be finished from their lists: at most 8 listed, no entry within 5 % of a listing boundary, and the excursion of
    both the isolated walk S(a) and the certified walk truth(a) below 0.4 of the slack bound.  Rows meant to leave (family 4): more
    than 8 listed, or an excursion above 1 / 0.4 of the bound, again with no entry within 5 % of a boundary.  The fp32 allowance is
    below 2 % of the smallest radius and the cells are at least four largest radii wide: fp32 rounding cannot move either decision."""
    for name in CASES_2D:
        c = case(name)
        for i in range(len(c["w"])):
            assert mc.fp32_allowance(c, i) < 0.02, (name, mc.fp32_allowance(c, i))
            assert mc.cell_edge(c, i) >= 4.0 * float(mc.radii(c, i).max()), name
            assert set(c["stay"][i]) | set(c["leave"][i]) >= {a for a in mc.rows(c, i) if c["alive"][i][a]}, name
            for a in c["stay"][i]:
                if a not in mc.rows(c, i):
                    continue                                                       # (the last entry of a chain is no row)
                surv, res, ratio = mc.listing(c, i, a)
                assert len(surv) + len(res) <= 8 and ratio >= mc.LIST_MARGIN, (name, a, len(surv) + len(res), ratio)
                absorbed, exc_t = [], 0.0                                          # (a row that is absorbed itself has no certified walk)
                if c["alive"][i][a]:
                    absorbed, exc_t = mc.walk(c, i, a, mc.alive_before(c, i, a))
                    assert absorbed == mc.truth(c, i, a), (name, a)
                assert set(mc.isolated(c, i, a)) | set(absorbed) <= set(surv) | set(res), (name, a)
                exc = max(mc.walk(c, i, a)[1], exc_t)
                assert exc < mc.SLACK_STAY * mc.slack_bound(c, i, a), (name, a, exc / mc.slack_bound(c, i, a))
            for a in c["leave"][i]:
                surv, res, ratio = mc.listing(c, i, a)
                assert ratio >= mc.LIST_MARGIN, (name, a, ratio)
                if len(surv) + len(res) > 8:
                    continue
                walks = [mc.walk(c, i, a)]
                if c["alive"][i][a]:
                    walks.append(mc.walk(c, i, a, mc.alive_before(c, i, a)))
                    assert walks[1][0] == mc.truth(c, i, a), (name, a)
                for absorbed, exc in walks:
                    assert len(absorbed) > 0 and exc > mc.slack_bound(c, i, a) / mc.SLACK_STAY, (name, a, exc / mc.slack_bound(c, i, a))


def sensitivity_table():
    """family -> scheduler -> the cases of the family whose certified result differs from the wrong scheduler's."""
    table = {}
    for name, c in all_cases():
        row = table.setdefault(family(name), {k: [] for k in SCHEDULERS})
        for k in SCHEDULERS:
            if mc.distinguishes(c, k):
                row[k].append(name)
    return table


def test_wrong_schedulers_are_told_apart():
    """W1 (no claim handling), W2 (a losing row keeps its initial state), W3 (liveness and re-walks from the isolated walks' holes):
    every family's certified result differs from at least one of them, and each of them is caught by at least one family -- W3 by the
    chain, W2 by the comb, W1 by the fan."""
    table = sensitivity_table()
    assert set(table) == {"chain", "fan", "comb", "family4"}
    for fam, row in table.items():
        assert any(row[k] for k in SCHEDULERS), fam
    for k in SCHEDULERS:
        assert any(table[fam][k] for fam in table), k
    assert table["chain"]["W3"] and table["comb"]["W2"] and table["fan"]["W1"] and table["fan"]["W2"]
    assert "fanp:63" in table["fan"]["W2"] and "comb:62" in table["comb"]["W1"]


# ---- GPU: 2-D merge -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES_2D)
def test_planted_structures_in_every_form_of_the_merge(pkg, ob, sc, name, monkeypatch):
    """Every particle of every planted case through the stand-alone merge, the unfused update and the fused step with 2 and 3 waves
    on both grids: the certified sizes and survivor weights, and weights, means and covariances against the oracle and numpy."""
    _run_merge_paths(pkg, ob, sc, case(name), monkeypatch)


@pytest.mark.gpu
def test_planted_structures_in_a_filter_batch(pkg, ob, sc):
    """Two filters of a batch, one holding the comb with d = 62 (63 rows, 62 sub-rounds), one the fan with k = 63 and private partners
    (64 rows, every loser re-walked): the batch's fused step merges both as merged_then_pruned does."""
    cases = [case("comb:62"), case("fanp:63")]
    nP = len(cases[0]["w"])
    assert all(len(c["w"]) == nP for c in cases)
    batch = pkg.FilterBatch(2, nP, gm_capacity=max(_cap(c) for c in cases))
    scens = [_scenario(sc, c) for c in cases]
    batch.set_poses(np.vstack([s_["poses"] for s_ in scens]), np.tile(np.asarray(sc.C1_PARAMS["pose_cov"]).ravel(), (2 * nP, 1)))
    batch.set_weights(np.ones(2 * nP))
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
    batch.cycle_async(None, [s_["Z"] for s_ in scens], normalize=True)
    batch.synchronize()
    sizes = batch.gm_sizes()
    for b, c in enumerate(cases):
        np.testing.assert_array_equal(sizes[b * nP:(b + 1) * nP], c["sizes"], err_msg=f"filter {b}: mixture sizes")
        for i in range(nP):
            d = batch.export_gm(b * nP + i)
            ew, emu, eS = pr.merged_then_pruned(c["w"][i], c["mean"][i], c["cov"][i], c["t"], c["f"], pr.PRUNE_T)
            np.testing.assert_allclose(d[0], np.sort(c["merged_w"][i])[::-1], rtol=1e-15, atol=0, err_msg=f"filter {b}: particle {i}: survivors")
            np.testing.assert_allclose(d[0], ew, rtol=GM_RTOL, atol=GM_ATOL)
            np.testing.assert_allclose(d[2], emu, rtol=GM_RTOL, atol=value_atol(c))
            np.testing.assert_allclose(d[3], eS, rtol=GM_RTOL, atol=value_atol(c))


# ---- GPU: Victoria Park merge -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES_VP)
def test_planted_structures_in_the_vp_merge(pkg, ob, sc, name):
    """The chain (63 and 64 entries: the lane-parallel scan; 65: row by row), a fan of 30 and a comb of 30 as 3-D (x, y, diameter)
    mixtures through the stand-alone Victoria Park merge and the fused step, poses far from every landmark and one measurement that
    nobody gates: the certified sizes and survivors, numpy and the oracle."""
    c = case(name, 3)
    n = len(c["w"])
    scen = dict(sc.make_vp_scenario(n, c["w"].shape[1], 3, seed=77))
    scen["w"], scen["mean"], scen["cov"] = c["w"], c["mean"], c["cov"]
    far = np.max(c["mean"][..., :2].reshape(-1, 2), axis=0) + 1e3
    scen["poses"] = np.tile(np.array([far[0], far[1], 0.3]), (n, 1))
    atol = value_atol(c)
    for fused in (False, True):
        dev = pkg.RBPHDFilter(n, device_id=0, gm_capacity=128, model=pkg.capi.MODEL_VICTORIAPARK_3D)
        orc = ob.OracleFilter(n, model=pkg.capi.MODEL_VICTORIAPARK_3D)
        for f in (dev, orc):
            sc.load_scenario(f, scen)
            f.update(np.array([[75.0, 0.1, 0.4]])) if fused else f.merge()
        np.testing.assert_array_equal(dev.gm_sizes(), c["sizes"], err_msg=f"fused={fused}: sizes vs the certified merge")
        np.testing.assert_array_equal(orc.gm_sizes(), c["sizes"])
        for i in range(n):
            d, o = dev.export_gm(i), orc.export_gm(i)
            if fused:
                ew, emu, eS = pr.merged_then_pruned(c["w"][i], c["mean"][i], c["cov"][i], c["t"], c["f"], pr.PRUNE_T)
                cw = np.sort(c["merged_w"][i])[::-1]
            else:
                ew, emu, eS = pr.np_merge_vp(c["w"][i], c["mean"][i], c["cov"][i], c["t"], c["f"])
                cw = c["merged_w"][i]
            np.testing.assert_allclose(d[0], cw, rtol=1e-15, atol=0, err_msg=f"fused={fused}: particle {i}: survivors (weights)")
            for y in (o, (ew, None, emu, eS)):
                np.testing.assert_allclose(d[0], y[0], rtol=GM_RTOL, atol=GM_ATOL)
                np.testing.assert_allclose(d[2], y[2], rtol=GM_RTOL, atol=atol)
                np.testing.assert_allclose(d[3], y[3], rtol=GM_RTOL, atol=atol)
