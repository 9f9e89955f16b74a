"""Multi-hypothesis FastSLAM association (csrc/fastslam_mh.h with murty.h's block form and hungarian_wave.h inside) at its
size boundaries: the LDS tile (sub-problems up to 32) against the HBM block with its other leading dimension (33 and up), the
second register of the solver's breadth-first queue (n > 32), the largest table (64) and the refusal at 65, rectangular tables
padded in both directions, CostMatrix::reduce fixing none, some or all rows, the likelihood-difference window, and hypotheses
of one parent that really differ.

Three-way comparison.  The device runs against the oracle (particle count, parents, weights, maps in order, candidate lists, at
the tolerances of tests/test_gpu_parity.py), and both run against tests/support/mh_fastslam_reference.py, a numpy / scipy
formulation that shares nothing with either solver: per parent the SORTED weights of its copies (tie order among assignments
that differ only in floor cells is not observable: such copies are identical).

Reference against oracle, measured on the CPU over every case of this file (first and second updates): the largest relative
difference of a child weight is 8.54e-14 (the reference adds an assignment's cells in another order and takes log N from
np.linalg.inv / det; a few ulps times the dimension, amplified by exp of a sum of magnitude up to ~100).  REF_RTOL is ten
times that, far below the 1e-9 of compare_weights, and the device is held to it as well.  The figure belongs to the numpy,
scipy and libm it was measured with: if these assertions start to fail by a small factor after a library upgrade while device
against oracle still holds at 1e-9, measure again (the CPU test prints the figure per case) before suspecting a kernel.

The window: no score of the reference lies within 1e-6 of the cut best - maxDiff in any case -- the kept scores and the
first score beyond the cut, which is the one that ends the list (asserted) -- so no near-tie at the cut decides nH.

Every case asserts on the oracle's counters that it reached the boundary it was written for: fs_assoc_dims (nMZ, nRed, nH
per particle) and, for the solver's second queue register, hungarian_max_queue_tail -- the most entries an augmenting search of
the oracle's restatement of the solver had enqueued before the expansion that finds its target (the device's search visits in
the same order and stops there; entries from index 64 on live in the second register): 69 ... 125 in the cases marked "q1".
"""
import math

import numpy as np
import pytest

from tests.support import mh_fastslam_reference as mhref

REF_RTOL = 8.54e-13
CUT_MARGIN = 1e-6
N0 = 4
NOISE = 3e-3


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def paired_scenario(sc, n_pairs, seed, sep=0.12):
    """As many in-range landmarks as measurements, no clutter, the landmarks in close pairs along a ray (`sep` metres apart,
    one to two measurement sigmas): every row and column of the table is live, and the 2nd to k-th best assignments are the
    swaps inside the pairs -- copies of one parent that correct different landmarks."""
    n = 2 * n_pairs
    scen = sc.make_scenario(N0, n, n, seed=seed, n_clutter=0)
    rng = np.random.default_rng(seed)
    Rm = np.asarray(scen["params"]["R"])
    a = -np.pi + 2 * np.pi * (np.arange(n_pairs) + 0.5) / n_pairs
    r = rng.uniform(0.8, 2.1, n_pairs)
    rr, aa = np.concatenate([r, r + sep]), np.concatenate([a, a])
    gt = np.stack([rr * np.cos(aa), rr * np.sin(aa)], 1)
    s = rng.uniform(0.02, 0.04, (N0, n, 2))
    cov = np.zeros((N0, n, 2, 2))
    cov[..., 0, 0], cov[..., 1, 1] = s[..., 0] ** 2, s[..., 1] ** 2
    Z = np.stack([rr + rng.normal(0, 0.5 * np.sqrt(Rm[0, 0]), n), aa + rng.normal(0, 0.5 * np.sqrt(Rm[1, 1]), n)], 1)
    scen.update(gt=gt, mean=gt[None] + rng.normal(0, 0.01, (N0, n, 2)), cov=cov, Z=Z[rng.permutation(n)], w=np.ones((N0, n)))
    return scen


def _case(name, hyp, diff, kind="crowded", steps=1, expect=(), **kw):
    return pytest.param(dict(name=name, hyp=hyp, diff=diff, kind=kind, steps=steps, expect=tuple(expect), kw=kw), id=name)


SHAPES = [(12, 8), (31, 20), (32, 32), (33, 20), (20, 33), (48, 40), (63, 30), (64, 64), (30, 64)]
TWO_STEPS = {(33, 20, 4), (48, 40, 16)}      # on through normalise, resample(n0), resampleOccured and a second update
SHAPE_EXPECT = {(12, 8): ["partial"], (33, 20): ["partial"], (20, 33): ["partial"], (48, 40): ["nred33", "partial"],
                (63, 30): ["nred33", "partial", "q1"], (64, 64): ["nred33", "nmz64", "q1"], (30, 64): ["nred33", "nmz64", "partial"]}

CASES = []
for _nl, _nz in SHAPES:
    for _hyp, _diff in [(4, 5.0), (16, 50.0)] + ([(2, 5.0)] if (_nl, _nz) in ((32, 32), (33, 20)) else []):
        CASES.append(_case("lm%d_z%d_h%d" % (_nl, _nz, _hyp), _hyp, _diff, steps=2 if (_nl, _nz, _hyp) in TWO_STEPS else 1,
                           expect=["full"] + SHAPE_EXPECT.get((_nl, _nz), []), n_landmarks=_nl, n_z=_nz))
CASES += [
    _case("pairs20_h16", 16, 50.0, kind="paired", expect=["full", "distinct", "nred33", "q1"], n_pairs=20, seed=7),
    _case("pairs32_h4", 4, 5.0, kind="paired", expect=["full", "distinct", "nred33", "nmz64", "q1"], n_pairs=32, seed=9),
    _case("pairs32_h16", 16, 3.0, kind="paired", expect=["full", "distinct", "nred33", "nmz64", "q1"], n_pairs=32, seed=9),
    _case("pairs16_h16", 16, 50.0, kind="paired", expect=["full", "distinct", "nred32"], n_pairs=16, seed=11),
    _case("pairs17_window", 16, 2.0, kind="paired", expect=["window", "distinct", "nred33"], n_pairs=17, seed=2),
    _case("sparse_all_fixed", 4, 5.0, kind="sparse", expect=["nred0"], n_landmarks=8, n_z=8, seed=201),
]


def _scenario(sc, c):
    kw = c["kw"]
    if c["kind"] == "paired":
        return paired_scenario(sc, kw["n_pairs"], kw["seed"]), kw["seed"]
    if c["kind"] == "sparse":      # a 25 m disc with few landmarks, each detected once, no clutter: reduce fixes every row
        return sc.make_scenario(N0, kw["n_landmarks"], kw["n_z"], seed=kw["seed"], n_clutter=0, rmax=25.0), kw["seed"]
    seed = 100 + kw["n_landmarks"]
    return sc.make_scenario(N0, kw["n_landmarks"], kw["n_z"], seed=seed), seed


def _configure(f, sc, scen, c):
    sc.load_scenario(f, scen)
    for i in range(scen["n"]):
        f.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
    cfg = f.default_fastslam_config()
    cfg.maxNDataAssocHypotheses = c["hyp"]
    cfg.maxDataAssocLogLikelihoodDiff = c["diff"]
    cfg.landmarkCandidateMeasurementCountThreshold = 2
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementCheckThreshold = 3
    f.set_fastslam_config(cfg)
    return cfg


# ---- the reference, computed once per (case, step) and shared by the CPU and the GPU tests ----------------------------------------

_REF = {}


def _reference(key, P, poses, pose_cov, maps, Z, floor, hyp, diff):
    if key not in _REF:
        _REF[key] = [mhref.particle_hypotheses(P, poses[i], pose_cov, maps[i][2], maps[i][3], Z, floor, hyp, diff) for i in range(len(poses))]
    return _REF[key]


def _sorted_children(w, parents, n_parents):
    return [np.sort(w[parents == i]) for i in range(n_parents)]


def _check_expectations(c, nMZ, nRed, nH, ref, queue_tail):
    hyp = c["hyp"]
    for e in c["expect"]:
        if e == "full":
            assert np.all(nH == hyp), nH
        elif e == "nred33":
            assert nRed.max() >= 33, nRed
        elif e == "nred32":              # the root exactly fills the LDS tile; beside pairs17 (34), the tile limit has distinct copies on both sides
            assert np.all(nRed == 32), nRed
        elif e == "nmz64":
            assert np.all(nMZ == 64), nMZ
        elif e == "partial":
            assert np.any((nRed > 0) & (nRed < nMZ)), (nRed, nMZ)
        elif e == "nred0":
            assert np.all(nRed == 0) and np.all(nH == 1), (nRed, nH)
        elif e == "window":
            assert np.any((nH > 1) & (nH < hyp)), nH
        elif e == "q1":                  # some augmenting search had 65 or more queue entries before it found its target
            assert queue_tail >= 65, queue_tail
        elif e == "distinct":
            assert any(len(set(h["cells"])) == h["nH"] > 1 for h in ref)
        else:
            raise AssertionError(e)


def run_case(c, ob, sc, pkg, device=False):
    """One case on the oracle (and on the device, if asked): returns the largest relative difference reference / oracle."""
    scen, seed = _scenario(sc, c)
    P = scen["params"]
    pose_cov = np.asarray(scen["pose_cov"], dtype=np.float64).reshape(3, 3)
    orc = ob.OracleFilter(N0)
    fs = [orc]
    if device:
        from tests.test_gpu_parity import _compare_fastslam
        dev = pkg.RBPHDFilter(N0, gm_capacity=256, max_particles=N0 * c["hyp"])
        fs.append(dev)
    for f in fs:
        cfg = _configure(f, sc, scen, c)
    rz, ru = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    poses = scen["poses"].copy()
    worst = 0.0
    for step in range(c["steps"]):
        Z = scen["Z"] + rz.normal(0, NOISE, scen["Z"].shape)
        for f in fs:
            f.predict_map(False)
        n_before = orc.n
        assert n_before == N0
        w_before = orc.get_weights().copy()
        maps = [orc.export_gm(i) for i in range(n_before)]
        cand_before = sum(len(orc.export_birth_candidates(i)[2]) for i in range(n_before))
        ob.hungarian_max_queue_tail(reset=True)
        orc.fastslam_update(Z)
        queue_tail = ob.hungarian_max_queue_tail()
        if device:
            dev.fastslam_update(Z)
        nMZ, nRed, nH = orc.fs_assoc_dims()
        par = orc.particle_parents()
        ref = _reference((c["name"], step), P, poses, pose_cov, maps, Z, cfg.minLogMeasurementLikelihood, c["hyp"], c["diff"])
        if step == 0:
            _check_expectations(c, nMZ, nRed, nH, ref, queue_tail)
        else:
            assert cand_before > 0 and orc.n > n_before, "the second update multiplied no particle that carries candidates"
        # the reference against the oracle: table and reduced dimensions, hypotheses kept, sorted child weights
        assert [h["nMZ"] for h in ref] == list(nMZ) and [h["nRed"] for h in ref] == list(nRed)
        assert [h["nH"] for h in ref] == list(nH)
        assert orc.n == int(nH.sum()) and np.array_equal(np.bincount(par, minlength=n_before), nH)
        for h in ref:                    # no score within 1e-6 of the window's cut, the first one beyond it included
            assert all(abs(h["scores"][0] - c["diff"] - s) >= CUT_MARGIN for s in h["scores"] + h["rejected"])
        want = [np.sort(w_before[i] / h["nH"] * np.exp(np.array(h["logw"]))) for i, h in enumerate(ref)]
        got = _sorted_children(orc.get_weights(), par, n_before)
        for i in range(n_before):
            worst = max(worst, float(np.max(np.abs(got[i] / want[i] - 1))))
            np.testing.assert_allclose(got[i], want[i], rtol=REF_RTOL, atol=0, err_msg="oracle vs reference, parent %d" % i)
        if device:
            assert dev.n == orc.n
            assert np.array_equal(dev.particle_parents(), par)
            _compare_fastslam(sc, dev, orc, dev.n)
            gd = _sorted_children(dev.get_weights(), par, n_before)
            for i in range(n_before):
                np.testing.assert_allclose(gd[i], want[i], rtol=REF_RTOL, atol=0, err_msg="device vs reference, parent %d" % i)
        if step + 1 < c["steps"]:
            poses = poses[par]
            for f in fs:
                f.normalize_weights(f.weight_sums()[0])
            plan = pkg.engine.systematic_resample_plan(orc.get_weights(), float(ru.random()), n_out=N0)
            for f in fs:
                f.resample_apply(plan, n_out=N0)
                f.fastslam_set_resample_occured(True)
            poses = poses[plan]
            for f in fs:
                f.set_poses(poses, scen["pose_cov"])
            if device:
                assert dev.n == N0
                _compare_fastslam(sc, dev, orc, N0)
    if device:
        dev.close()
    return worst


# ---- CPU: the reference itself, and the reference against the oracle -----------------------------------------------------------

def _golden(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", name)) as fh:
        return json.load(fh)


def test_reference_ranking_against_the_bruteforce_fixture():
    """murty_ranked on the reference project's recorded known answers (BruteForceLinearAssignment, every assignment ranked)."""
    for case in _golden("bruteforce_ranked.json"):
        Cm = np.array(case["C"])
        want = np.array(case["scores"])
        got = mhref.murty_ranked(Cm, len(want))
        assert len(got) == len(want)
        np.testing.assert_allclose([s for s, _ in got], want, rtol=0, atol=1e-9)
        assert len({tuple(a.tolist()) for _, a in got}) == len(got)
        for s, a in got:
            assert sorted(a.tolist()) == list(range(len(Cm))) and np.isclose(s, Cm[np.arange(len(Cm)), a].sum(), rtol=0, atol=1e-12)
        if len(want) == math.factorial(len(Cm)):               # listed whole: the solver runs dry exactly there
            assert len(mhref.murty_ranked(Cm, len(want) + 5)) == len(want)


def test_reference_ranking_against_the_extended_fixture():
    """murty_ranked on the 20 extended tables of dimension 7 ... 9: the fixture lists the DISTINCT scores >= -1000 of the
    reference's brute force (equal consecutive scores counted once: assignments that differ only inside the zero block), so the
    plain ranking is de-duplicated the same way and must give the same scores, as far as 600 ranked assignments reach."""
    reached = 0
    for case in _golden("murty_extended_ranked.json"):
        Cm = np.array(case["C"])
        want = case["scores"]
        got = []
        for s, _ in mhref.murty_ranked(Cm, 600):
            if s < -1000.0:
                break
            if not got or s != got[-1]:
                got.append(s)
        whole = len(got) >= len(want)
        k = len(want) if whole else len(got) - 1               # (the last distinct score may have equals beyond the 600th)
        assert k >= min(len(want), 20), (case["nR"], case["nC"], k)
        np.testing.assert_allclose(got[:k], want[:k], rtol=1e-12, atol=0)
        reached += whole
    assert reached >= 10


def test_reference_ranking_against_permutations_and_its_window():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5, 7):
        Cm = rng.uniform(-10, 3, (n, n))
        Cm[rng.uniform(size=(n, n)) < 0.4] = -10.0            # floor cells: exact ties
        want = mhref.bruteforce_ranked(Cm, math.factorial(n))
        got = [s for s, _ in mhref.murty_ranked(Cm, 40)]
        assert len(got) == min(40, len(want))
        np.testing.assert_allclose(got, want[:40], rtol=0, atol=1e-12)
        for cut in (0.5, 4.0, 12.0):                          # the window: the list ends before the first score at or beyond the cut
            assert all(abs(want[0] - cut - s) > 1e-9 for s in want)
            inside = sum(1 for s in want if want[0] - s < cut)
            assert len(mhref.murty_ranked(Cm, 40, cut)) == min(40, inside)


def test_reference_reduce_against_the_oracle(ob):
    import ctypes as C
    lib = ob.load()
    rng = np.random.default_rng(6)
    lim = -10.0
    for trial in range(80):
        n = int(rng.integers(1, 14))
        T = np.full((n, n), lim)
        for _ in range(int(rng.integers(0, 2 * n + 1))):
            T[rng.integers(0, n), rng.integers(0, n)] = rng.uniform(-9.5, 2.0)
        fixed, iRed, jRed = mhref.reduce_table(T, lim)
        a = np.zeros(n, np.int32); ir = np.zeros(n, np.int32); jr = np.zeros(n, np.int32)
        Tc = np.ascontiguousarray(T.copy())
        nRed = lib.rfsor_cost_matrix_reduce(Tc.ctypes.data_as(C.c_void_p), C.c_int(n), C.c_double(lim), a.ctypes.data_as(C.c_void_p),
                                            ir.ctypes.data_as(C.c_void_p), jr.ctypes.data_as(C.c_void_p))
        assert nRed == len(iRed)
        assert [fixed.get(x, -1) for x in range(n)] == a.tolist()
        if nRed:
            assert ir[:nRed].tolist() == iRed and jr[:nRed].tolist() == jRed


@pytest.mark.parametrize("c", CASES)
def test_reference_against_oracle(pkg, ob, sc, c):
    """The independent reference against the oracle at every shape of the GPU list: nMZ, nRed and nH per parent, the sorted
    child weights within REF_RTOL, the boundary each case was written for (oracle counters), and the window's margin."""
    worst = run_case(c, ob, sc, pkg)
    print("reference vs oracle, largest relative difference of a child weight: %.3g" % worst)
    assert worst <= REF_RTOL


def test_oracle_reports_the_refused_and_the_victoria_park_shapes(ob, sc, pkg):
    """The shapes of the two device-against-oracle-only GPU cases below, on the oracle's counters."""
    for n_lm, want in ((65, 65), (64, 64)):
        orc = ob.OracleFilter(N0)
        scen = sc.make_scenario(N0, n_lm, 10, seed=165)
        _configure(orc, sc, scen, dict(hyp=2, diff=5.0))
        orc.fastslam_update(scen["Z"])
        assert np.all(orc.fs_assoc_dims()[0] == want)
    orc, scen = _vp_pair(ob, sc, pkg)[1:]
    orc.predict_map(False)
    orc.fastslam_update(scen["Z"])
    nMZ, nRed, nH = orc.fs_assoc_dims()
    assert nRed.max() > 32 and np.all(nH == 16), (nRed, nH)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_mh_fastslam_at_murty_size_boundaries(pkg, ob, sc, c):
    run_case(c, ob, sc, pkg, device=True)


def _vp_pair(ob, sc, pkg, device=False):
    scen = sc.make_vp_scenario(N0, 60, 30, seed=300)
    orc = ob.OracleFilter(N0, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    dev = pkg.RBPHDFilter(N0, gm_capacity=256, max_particles=N0 * 16, model=pkg.capi.MODEL_VICTORIAPARK_3D) if device else None
    for f in (orc, dev):
        if f is not None:
            _configure(f, sc, scen, dict(hyp=16, diff=50.0))
    return dev, orc, scen


@pytest.mark.gpu
def test_mh_fastslam_victoria_park_beyond_the_lds_tile(pkg, ob, sc):
    """fs_mh_associate_kernel<3> (built with another occupancy attribute) on reduced tables beyond 32: device against oracle."""
    from tests.test_gpu_parity import _compare_fastslam
    dev, orc, scen = _vp_pair(ob, sc, pkg, device=True)
    for f in (dev, orc):
        f.predict_map(False)
        f.fastslam_update(scen["Z"])
    nMZ, nRed, nH = orc.fs_assoc_dims()
    assert nRed.max() > 32 and np.all(nH == 16), (nRed, nH)
    assert dev.n == orc.n == 64
    assert np.array_equal(dev.particle_parents(), orc.particle_parents())
    _compare_fastslam(sc, dev, orc, dev.n)
    dev.close()


@pytest.mark.gpu
def test_mh_fastslam_refuses_a_table_of_65_and_accepts_64(pkg, ob, sc):
    """65 landmarks in range: the update raises the engine's Murty-capacity error (ERR_UNSUPPORTED) and leaves particle count, weights and maps exactly as they were; the same map with 64 in range is accepted."""
    from tests.test_gpu_parity import _compare_fastslam
    c = dict(hyp=2, diff=5.0)
    scen = sc.make_scenario(N0, 65, 10, seed=165)
    dev = pkg.RBPHDFilter(N0, gm_capacity=256, max_particles=N0 * 2)
    _configure(dev, sc, scen, c)
    w0 = dev.get_weights().copy()
    maps0 = [dev.export_gm(i) for i in range(N0)]
    with pytest.raises(pkg.capi.EngineError) as e:
        dev.fastslam_update(scen["Z"])
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED
    assert dev.n == N0
    assert np.array_equal(dev.get_weights(), w0)
    for i in range(N0):
        for x, y in zip(dev.export_gm(i), maps0[i]):
            assert np.array_equal(x, y)
    dev.close()
    scen = sc.make_scenario(N0, 64, 10, seed=165)
    dev = pkg.RBPHDFilter(N0, gm_capacity=256, max_particles=N0 * 2)
    orc = ob.OracleFilter(N0)
    for f in (dev, orc):
        _configure(f, sc, scen, c)
        f.fastslam_update(scen["Z"])
    assert np.all(orc.fs_assoc_dims()[0] == 64)
    assert dev.n == orc.n and np.array_equal(dev.particle_parents(), orc.particle_parents())
    _compare_fastslam(sc, dev, orc, dev.n)
    dev.close()
