"""The fp32 prefilters in front of the exact merge and gate tests, at their margins ("fp32 prefilters").

Each kernel screens pairs in fp32 before the exact fp64 test of the reference decides: the 2-D merge grid and candidate scan
(csrc/merge_prune.h), the Victoria Park merge sweep (csrc/vp.h) and the innovation-gate sweeps of both map updates (csrc/update_map.h,
csrc/vp.h).  The inputs here put pairs where those screens are tightest -- kilometres from the origin, near-rank-1 covariances lined
up with the pair, rows at the listing limits, grid spans at the fine-grid switch, innovations within 1e-6 of the gates -- and every
decision is certified in exact arithmetic (tests/support/prefilter_reference.py).  The device must make exactly the certified decisions
(mixture sizes, which entries were absorbed, the new Gaussians and their order) and agree with the oracle.

Value tolerances: GM_RTOL / GM_ATOL as in test_gpu_parity, plus, for means and covariances only, 8 eps X (1 + 2 f r) where X is the
largest coordinate and r the largest merge displacement.  A merged mean (x_a w_a + x_j w_j) / w_m carries a few roundings of size
eps X / 2, differently placed on the device and in the references; the inflation term f d d^T, d = x_m - x_a (|d| <= r), inherits them
times 2 f r.  At the origin the extra term is below GM_ATOL."""
import functools

import numpy as np
import pytest

from tests.support import prefilter_reference as pr

GM_RTOL, GM_ATOL = 1e-10, 1e-12
EPS = 2.0 ** -52
ENV_KEYS = ("RFSGPU_FUSED_STEP", "RFSGPU_STEP_WPP", "RFSGPU_MERGE_GRID")
# every form that merges a 2-D map: (name, environment)
MERGE_PATHS = [("merge", {}), ("update_unfused", {"RFSGPU_FUSED_STEP": "0"}), ("fused_wpp2", {"RFSGPU_STEP_WPP": "2"}),
               ("fused_wpp3", {"RFSGPU_STEP_WPP": "3"}), ("fused_grid5", {"RFSGPU_STEP_WPP": "3", "RFSGPU_MERGE_GRID": "5"}),
               ("fused_grid6", {"RFSGPU_STEP_WPP": "3", "RFSGPU_MERGE_GRID": "6"})]
STRADDLE = [(off, ax) for off, ax in [((1e3, 0.0), "x"), ((-1e3, 0.0), "x"), ((1e4, 0.0), "x"), ((-1e4, 0.0), "x"), ((0.0, 1e4), "y"),
                                       ((3e4, 0.0), "x"), ((0.0, -3e4), "y"), ((1e4, 1e4), "x"), ((1e5, 0.0), "x"), ((-1e5, 1e5), "y")]]
DELTAS = [1e-3, 1e-6]


# ---- cases (built once per session: the certification replays every merge in rationals) --------------------------------------

@functools.lru_cache(maxsize=None)
def straddle(off, ax, delta, at_origin=False, dim=2):
    if dim == 3:
        return pr.straddle_case(off, ax, delta, n_pairs=24, groups=6, dim=3, t=1.0, f=1.5, at_origin=at_origin, seed=31)
    return pr.straddle_case(off, ax, delta, at_origin=at_origin, seed=17)


@functools.lru_cache(maxsize=None)
def limit_case(name):
    if name == "issue":
        return pr.issue_regression_case()
    if name.startswith("ring"):
        _, k, ring, off = name.split(":")
        return pr.listing_limit_case(int(k), float(ring), offset=(float(off), 0.0), seed=int(k))
    if name.startswith("paircap"):
        return pr.pair_cap_case(int(name.split(":")[1]), seed=3)
    if name == "slack":
        return pr.slack_case(seed=5)
    if name.startswith("fine"):
        return pr.fine_grid_case(float(name.split(":")[1]), seed=9)
    raise ValueError(name)


LIMIT_CASES = ["issue", "ring:8:0.9:0", "ring:9:0.9:0", "ring:8:1.3:0", "ring:9:1.3:0", "ring:8:0.9:1e4", "ring:9:1.3:1e4",
               "paircap:32", "paircap:33", "slack", "fine:1.01", "fine:0.99"]
GATE_KINDS = pr.GATE_SETS


def all_cases():
    """Every constructed merge case (for the CPU certification test)."""
    out = [(f"straddle{off}{ax}{d}", straddle(off, ax, d)) for off, ax in STRADDLE for d in DELTAS]
    out += [(f"straddle{off}{ax}-1e-6", straddle(off, ax, -1e-6)) for off, ax in STRADDLE[::3]]
    out += [(f"origin{off}{ax}{d}", straddle(off, ax, d, True)) for off, ax in STRADDLE[::3] for d in (1e-6, -1e-6)]
    out += [(f"vp{off}{ax}{d}", straddle(off, ax, d, False, 3)) for off, ax in STRADDLE[::2] for d in (1e-6, -1e-6)]
    out += [(n, limit_case(n)) for n in LIMIT_CASES]
    return out


def value_atol(case):
    X = float(np.max(np.abs(case["mean"])))
    r = max(float(np.sqrt(np.max(case["cov"][..., 0, 0] + case["cov"][..., 1, 1]))) * case["t"], 1.0)
    return GM_ATOL + 8 * EPS * X * (1 + 2 * case["f"] * r)


# ---- CPU: certification ---------------------------------------------------------------------------------------------------

def test_every_constructed_case_is_certified():
    """Each constructed merge decision and gate decision sits at least CERT_REL on its side of its threshold, in exact arithmetic,
    and the near-threshold constructions really are near: within 1e-5 (inside the fp32 prefilters' own margins)."""
    for name, c in all_cases():
        assert c["margin"] >= pr.CERT_REL, name
        if name.startswith(("straddle", "origin", "vp")):
            assert c["margin"] < 2e-3, name
            if "e-06" in name or "e-6" in name:
                assert c["margin"] < 1e-5, (name, c["margin"])
        for i in range(min(len(c["w"]), 8)):                                  # (np_merge is O(M^2) solves: the first particles)
            mw, mmu, mS = pr.np_merge(c["w"][i], c["mean"][i], c["cov"][i], c["t"], c["f"])
            assert len(mw) == c["sizes"][i], name                         # fp64 greedy merge makes the certified decisions
            np.testing.assert_allclose(mw, c["merged_w"][i], rtol=1e-15)
    for kind in GATE_KINDS:
        for maker in (pr.rngbrg_gate_case, pr.vp_gate_case):
            g = maker(kind, seed=1)
            assert g["margin"] >= pr.CERT_REL
            assert g["margin"] < 2e-6, (kind, g["margin"])                # some pair sits at g (1 -+ 1e-6)
            assert 0 < sum(len(e) for e in g["expect"]) < g["n"] * g["nM"] * len(g["Z"])
    for maker in (pr.rngbrg_gate_case, pr.vp_gate_case):             # some passing pair needs the range threshold's rounding term
        g = maker("range", seed=1)
        worst = max(pr.fp32_range_innovation(g["Z"][z, 0], g["ranges"][m]) for e in g["expect"] for m, z in e)
        assert worst > g["g_range"] * (1 + 1e-5), (maker.__name__, worst / g["g_range"])


def _prefilter_survivors(c, i, a):
    """Entries j > a within max(radius_a, radius_j) of entry a (radius sqrt(t^2 tr S)): what the candidate scan lists for row a."""
    tr = c["cov"][i][:, 0, 0] + c["cov"][i][:, 1, 1]
    r2 = c["t"] ** 2 * tr
    d2 = np.sum((c["mean"][i] - c["mean"][i][a]) ** 2, axis=1)
    j = np.arange(len(tr))
    return int(np.sum((j > a) & (d2 <= np.maximum(r2[a], r2))))


def test_listing_and_slack_cases_reach_their_paths():
    """Every centre of a ring case is a row with exactly n_ring prefilter survivors above it.  In the slack case every A absorbs B and
    then C, which starts more than twice A's prefilter radius away from A (so it is not listed for A and only bounds A's slack)."""
    for n_ring in (8, 9):
        for ring in (0.9, 1.3):
            c = limit_case(f"ring:{n_ring}:{ring}:0")
            for i in range(len(c["w"])):
                centres = np.nonzero(np.isclose(c["cov"][i][:, 0, 0], 0.04))[0]
                assert len(centres) == 6
                assert [_prefilter_survivors(c, i, a) for a in centres] == [n_ring] * 6
    c = limit_case("slack")
    for i in range(len(c["w"])):
        assert len(c["roles"][i]) == 5
        for a, b, cc in c["roles"][i]:
            mg = c["merges"][i]
            assert (a, b) in mg and (a, cc) in mg and mg.index((a, b)) < mg.index((a, cc))
            assert a < b < cc
            ra = c["t"] * np.sqrt(np.trace(c["cov"][i][a]))
            assert np.linalg.norm(c["mean"][i][cc] - c["mean"][i][a]) > 2 * ra


def test_straddle_cases_merge_pairs_and_the_issue_case_is_exact():
    c = limit_case("issue")
    assert c["merges"] == [[(1, 2)]]
    assert abs(c["margin"] - 6e-4) < 1e-5                                 # md2 = 0.9994 t^2
    for d, merges in ((1e-6, True), (-1e-6, False)):
        s = straddle((1e4, 0.0), "x", d)
        n_pairs = (s["w"].shape[1] - 1) // 2
        assert np.all(s["sizes"] == (1 + n_pairs if merges else 1 + 2 * n_pairs))


def test_wrap_reference_is_the_while_loop():
    assert pr.wrap_reference(pr.PI) == pr.PI
    assert pr.wrap_reference(-pr.PI) == -pr.PI
    x = pr.wrap_reference(60.0)
    assert -pr.PI <= x <= pr.PI and abs(float(x) - (60.0 - 20 * np.pi)) < 1e-12
    assert pr.gate_rngbrg(1.0, 0.0, 1.0, 0.2)[0] and not pr.gate_rngbrg(1.0 + 1e-12, 0.0, 1.0, 0.2)[0]
    assert pr.gate_rngbrg(0.0, 2 * np.pi + 0.1, 1.0, 0.2)[0] and not pr.gate_vp(0.0, 0.3, 1.0, 0.2)[0]


# ---- GPU: 2-D merge -------------------------------------------------------------------------------------------------------

def _scenario(sc, case):
    """A range-bearing scenario holding the case's maps, with every pose far from every landmark (Pd = 0: the update only merges)."""
    n = len(case["w"])
    P = dict(sc.C1_PARAMS)
    P["merge_thr"], P["merge_infl"] = case["t"], case["f"]
    far = np.max(case["mean"][..., :2].reshape(-1, 2), axis=0) + 1e3
    poses = np.tile(np.array([far[0], far[1], 0.1]), (n, 1))
    return dict(n=n, poses=poses, pose_cov=np.asarray(P["pose_cov"]), particle_w=np.ones(n), params=P, w=case["w"], mean=case["mean"],
                cov=case["cov"], Z=np.array([[1.0, 0.1], [2.0, -0.5]]))


def _cap(case):
    return int(max(128, -(-case["w"].shape[1] // 64) * 64 + 64))


def _check_merged(sc, dev, orc, case, stand_alone, label):
    atol = value_atol(case)
    n = len(case["w"])
    np.testing.assert_array_equal(dev.gm_sizes(), case["sizes"], err_msg=f"{label}: mixture sizes against the certified merge")
    np.testing.assert_array_equal(orc.gm_sizes(), case["sizes"], err_msg=f"{label}: oracle sizes against the certified merge")
    for i in range(n):
        d, o = dev.export_gm(i), orc.export_gm(i)
        if stand_alone:
            ew, emu, eS = pr.np_merge(case["w"][i], case["mean"][i], case["cov"][i], case["t"], case["f"])
            cw = case["merged_w"][i]
        else:
            ew, emu, eS = pr.merged_then_pruned(case["w"][i], case["mean"][i], case["cov"][i], case["t"], case["f"], pr.PRUNE_T)
            cw = np.sort(case["merged_w"][i])[::-1]
        np.testing.assert_allclose(d[0], cw, rtol=1e-15, atol=0, err_msg=f"{label}: particle {i}: survivors (weights)")
        if len(np.unique(ew)) < len(ew):     # tied weights (the issue's case): the order of equal keys is std::sort's; numpy as a multiset
            sc.assert_gm_close(d, (ew, ew, emu, eS), GM_RTOL, atol)
            np.testing.assert_allclose(d[0], o[0], rtol=GM_RTOL, atol=GM_ATOL)
            np.testing.assert_allclose(d[2], o[2], rtol=GM_RTOL, atol=atol)
            np.testing.assert_allclose(d[3], o[3], rtol=GM_RTOL, atol=atol)
            continue
        for x, y, what in ((d, o, "oracle"), ((d[0], None, d[2], d[3]), (ew, None, emu, eS), "numpy")):
            np.testing.assert_allclose(x[0], y[0], rtol=GM_RTOL, atol=GM_ATOL, err_msg=f"{label}: particle {i}: weights vs {what}")
            np.testing.assert_allclose(x[2], y[2], rtol=GM_RTOL, atol=atol, err_msg=f"{label}: particle {i}: means vs {what}")
            np.testing.assert_allclose(x[3], y[3], rtol=GM_RTOL, atol=atol, err_msg=f"{label}: particle {i}: covariances vs {what}")


def _run_merge_paths(pkg, ob, sc, case, monkeypatch, paths=MERGE_PATHS):
    scen = _scenario(sc, case)
    for name, env in paths:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dev = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=_cap(case))
        orc = ob.OracleFilter(scen["n"])
        for f in (dev, orc):
            sc.load_scenario(f, scen)
        for f in (dev, orc):
            if name == "merge":
                f.merge()
            else:
                f.update(scen["Z"])
        _check_merged(sc, dev, orc, case, name == "merge", name)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("off,ax", STRADDLE)
def test_straddling_pairs_far_from_the_origin(pkg, ob, sc, off, ax, delta, monkeypatch):
    """Lined-up near-rank-1 pairs at md2 = t^2 (1 - delta), swept through the merge grid's cells kilometres from the origin: every
    pair merges, in every form of the merge."""
    _run_merge_paths(pkg, ob, sc, straddle(off, ax, delta), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("off,ax", STRADDLE[::3])
def test_the_same_pairs_at_the_origin_and_just_outside_the_threshold(pkg, ob, sc, off, ax, monkeypatch):
    for c in (straddle(off, ax, 1e-6, True), straddle(off, ax, -1e-6, True), straddle(off, ax, -1e-6)):
        _run_merge_paths(pkg, ob, sc, c, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIMIT_CASES)
def test_listing_limits_slack_and_fine_grid(pkg, ob, sc, name, monkeypatch):
    """The issue's three-Gaussian case; rows with exactly MERGE_ROW_SLOTS (8) and 9 prefilter survivors; a mixture that lists exactly
    MERGE_PAIR_CAP (320) pairs and one that overflows it; a row that moves onto a partner it first failed by more than twice its
    radius; spans just above and below the 64 x 64 grid's fall-back to 32 x 32 cells."""
    _run_merge_paths(pkg, ob, sc, limit_case(name), monkeypatch)


@pytest.mark.gpu
def test_straddling_pairs_in_a_filter_batch(pkg, ob, sc):
    """Two filters of a batch, one holding far-away straddling pairs, one at the origin: the batch's fused step merges both."""
    cases = [straddle((1e4, 0.0), "x", 1e-6), straddle((1e4, 0.0), "x", 1e-6, True)]
    nP = min(len(c["w"]) for c in cases)
    batch = pkg.FilterBatch(2, nP, gm_capacity=128)
    scens = [_scenario(sc, c) for c in cases]
    poses = np.vstack([s_["poses"][:nP] for s_ in scens])
    batch.set_poses(poses, np.tile(np.asarray(sc.C1_PARAMS["pose_cov"]).ravel(), (2 * nP, 1)))
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
        np.testing.assert_array_equal(sizes[b * nP:(b + 1) * nP], c["sizes"][:nP], err_msg=f"filter {b}: mixture sizes")
        for i in range(nP):
            d = batch.export_gm(b * nP + i)
            ew, emu, eS = pr.merged_then_pruned(c["w"][i], c["mean"][i], c["cov"][i], c["t"], c["f"], pr.PRUNE_T)
            np.testing.assert_allclose(d[0], ew, rtol=GM_RTOL, atol=GM_ATOL)
            np.testing.assert_allclose(d[2], emu, rtol=GM_RTOL, atol=value_atol(c))
            np.testing.assert_allclose(d[3], eS, rtol=GM_RTOL, atol=value_atol(c))


TRANSLATE_KINDS = [("clusters", 150, 256), ("crowded", 120, 128), ("coincident", 200, 256), ("mixed_scales", 180, 192), ("chain", 100, 128)]
TRANSLATE_OFFSETS = [(1e3, -1e3), (-1e4, 0.0), (3e4, 1e4), (1e5, 1e5)]


def _clustered(sc, kind, M):
    from tests.test_gpu_parity import _clustered_mixtures
    return _clustered_mixtures(sc, 8, M, kind, seed=2100 + M)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,M,cap", TRANSLATE_KINDS)
def test_translated_clustered_mixtures(pkg, ob, sc, kind, M, cap, monkeypatch):
    """Every _clustered_mixtures kind, shifted by offsets up to 1e5 m: the device makes the decisions of the unshifted device run and
    of the oracle on the shifted input (stand-alone merge, and the fused step with three waves on both grids)."""
    base = _clustered(sc, kind, M)
    ref = pkg.RBPHDFilter(base["n"], device_id=0, gm_capacity=cap)
    sc.load_scenario(ref, base)
    ref.merge()
    ref_sizes = ref.gm_sizes()
    ref_w = [ref.export_gm(i)[0] for i in range(base["n"])]
    for off in TRANSLATE_OFFSETS:
        scen = dict(base)
        scen["mean"] = base["mean"] + np.array(off)
        scen["poses"] = base["poses"] + np.array([off[0] + 500.0, off[1], 0.0])
        for name, env in [("merge", {})] + MERGE_PATHS[4:]:
            for k in ENV_KEYS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            dev = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=cap)
            orc = ob.OracleFilter(scen["n"])
            for f in (dev, orc):
                sc.load_scenario(f, scen)
                f.merge() if name == "merge" else f.update(scen["Z"])
            np.testing.assert_array_equal(dev.gm_sizes(), orc.gm_sizes(), err_msg=f"{off} {name}: sizes vs oracle")
            atol = value_atol(dict(mean=scen["mean"], cov=scen["cov"], t=sc.C1_PARAMS["merge_thr"], f=sc.C1_PARAMS["merge_infl"]))
            for i in range(scen["n"]):
                d, o = dev.export_gm(i), orc.export_gm(i)
                np.testing.assert_allclose(d[0], o[0], rtol=GM_RTOL, atol=GM_ATOL, err_msg=f"{off} {name}: weights vs oracle")
                np.testing.assert_allclose(d[2], o[2], rtol=GM_RTOL, atol=atol)
                np.testing.assert_allclose(d[3], o[3], rtol=GM_RTOL, atol=atol)
                if name == "merge":
                    np.testing.assert_array_equal(dev.gm_sizes(), ref_sizes, err_msg=f"{off}: sizes vs the unshifted run")
                    np.testing.assert_allclose(d[0], ref_w[i], rtol=1e-14, atol=0, err_msg=f"{off}: survivors vs the unshifted run")
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


# ---- GPU: Victoria Park merge ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("delta", [1e-6, -1e-6])
@pytest.mark.parametrize("off,ax", STRADDLE[::2])
def test_vp_merge_near_the_threshold_far_from_the_origin(pkg, ob, sc, off, ax, delta):
    """3-D (x, y, diameter) lined-up near-rank-1 pairs at md2 = t^2 (1 -+ 1e-6), offsets up to 1e5 m: the stand-alone VP merge and
    the fused VP step make the certified decisions."""
    case = straddle(off, ax, delta, False, 3)
    n = len(case["w"])
    base = sc.make_vp_scenario(n, case["w"].shape[1], 3, seed=77)
    scen = dict(base)
    scen["w"], scen["mean"], scen["cov"] = case["w"], case["mean"], case["cov"]
    far = np.max(case["mean"][..., :2].reshape(-1, 2), axis=0) + 1e3
    scen["poses"] = np.tile(np.array([far[0], far[1], 0.3]), (n, 1))
    atol = value_atol(case)
    for fused in (False, True):
        dev = pkg.RBPHDFilter(n, device_id=0, gm_capacity=128, model=pkg.capi.MODEL_VICTORIAPARK_3D)
        orc = ob.OracleFilter(n, model=pkg.capi.MODEL_VICTORIAPARK_3D)
        for f in (dev, orc):
            sc.load_scenario(f, scen)
            f.update(np.array([[75.0, 0.1, 0.4]])) if fused else f.merge()
        np.testing.assert_array_equal(dev.gm_sizes(), case["sizes"], err_msg=f"fused={fused}: sizes vs the certified merge")
        np.testing.assert_array_equal(orc.gm_sizes(), case["sizes"])
        for i in range(n):
            d, o = dev.export_gm(i), orc.export_gm(i)
            if fused:
                ew, emu, eS = pr.merged_then_pruned(case["w"][i], case["mean"][i], case["cov"][i], case["t"], case["f"], pr.PRUNE_T)
            else:
                ew, emu, eS = pr.np_merge_vp(case["w"][i], case["mean"][i], case["cov"][i], case["t"], case["f"])
            for y in (o, (ew, None, emu, eS)):
                np.testing.assert_allclose(d[0], y[0], rtol=GM_RTOL, atol=GM_ATOL)
                np.testing.assert_allclose(d[2], y[2], rtol=GM_RTOL, atol=atol)
                np.testing.assert_allclose(d[3], y[3], rtol=GM_RTOL, atol=atol)


# ---- GPU: innovation gates ------------------------------------------------------------------------------------------------

def _check_update_map(dev, orc, g, label, np_ref=True):
    n, nM = g["n"], g["nM"]
    np.testing.assert_array_equal(dev.gm_sizes(), [nM + len(e) for e in g["expect"]], err_msg=f"{label}: new Gaussians vs the certified gates")
    np.testing.assert_array_equal(orc.gm_sizes(), dev.gm_sizes())
    for i in range(n):
        d, o = dev.export_gm(i), orc.export_gm(i)
        for k in (0, 1):
            np.testing.assert_allclose(d[k], o[k], rtol=GM_RTOL, atol=GM_ATOL * 1e-3, err_msg=f"{label}: particle {i}")
        np.testing.assert_allclose(d[2], o[2], rtol=GM_RTOL, atol=GM_ATOL)
        np.testing.assert_allclose(d[3], o[3], rtol=GM_RTOL, atol=GM_ATOL)
        assert np.array_equal(dev.get_unused(i), orc.get_unused(i)), label
        assert dev.landmarks_in_fov(i) == orc.landmarks_in_fov(i) == nM, label
        used = sorted({z for _, z in g["expect"][i]})
        assert set(dev.get_unused(i)) | set(used) == set(range(len(g["Z"]))), label
        if np_ref:
            w, wp, mu, Sg, unused, nfov, _ = pr.np_update_map(g["params"], g["poses"][i], g["pose_cov"], g["w"][i], g["mean"][i], g["cov"][i], g["Z"])
            assert len(w) == len(d[0]), label
            np.testing.assert_allclose(d[0], w, rtol=1e-9, atol=1e-300, err_msg=label)
            np.testing.assert_allclose(d[2], mu, rtol=1e-10, atol=1e-12, err_msg=label)
            np.testing.assert_allclose(d[3], Sg, rtol=1e-8, atol=1e-14, err_msg=label)
            assert list(dev.get_unused(i)) == unused, label
            assert nfov == nM


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind", GATE_KINDS)
def test_rngbrg_innovation_gates_at_their_thresholds(pkg, ob, sc, kind, seed):
    """|range innovation| = kf_range (1 -+ delta), |wrapped bearing innovation| = kf_bearing (1 -+ delta), delta = 1e-3 and 1e-6;
    expected bearings on either side of +-pi; measurement bearings up to and past 50 rad; ranges up to 1e4 m.  update_map makes the
    certified gate decisions and agrees with the oracle and with np_update_map."""
    g = pr.rngbrg_gate_case(kind, seed=seed)
    dev = pkg.RBPHDFilter(g["n"], device_id=0, gm_capacity=512)
    orc = ob.OracleFilter(g["n"])
    for f in (dev, orc):
        sc.load_scenario(f, g)
        f.update_map(g["Z"])
    _check_update_map(dev, orc, g, f"{kind}/{seed}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kind", GATE_KINDS)
def test_vp_innovation_gates_at_their_thresholds(pkg, ob, sc, kind, seed):
    """The same for the Victoria Park model (wrap first, then the gates), against the oracle and the certified decisions."""
    g = pr.vp_gate_case(kind, seed=seed)
    dev = pkg.RBPHDFilter(g["n"], device_id=0, gm_capacity=512, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    orc = ob.OracleFilter(g["n"], model=pkg.capi.MODEL_VICTORIAPARK_3D)
    for f in (dev, orc):
        sc.load_scenario(f, g)
        f.update_map(g["Z"])
    _check_update_map(dev, orc, g, f"vp {kind}/{seed}", np_ref=False)
