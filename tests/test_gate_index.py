"""The measurement index of the map update's gate prefilter against the dense sweep it replaces (csrc/update_map.h).

The index only proposes candidates; the exact fp64 gates decide as before, in the same order.  So a handle created under
RFSGPU_GATE_INDEX=0 (the sweep) and one created without it (the index) must leave bit-identical results: particle weights, mixture
sizes, unused-measurement lists, landmarks in the field of view and every exported mixture, in order.  The indexed run is also held
against the oracle at test_gpu_parity's tolerances, ordered.  Every case has at most 8 particles and capacity 256.

One input cannot be put to the oracle and is compared index against sweep only: an infinite measurement bearing (the reference's
`while (a > PI) a -= 2 PI` never ends on it; the device turns it into a NaN that passes no Mahalanobis gate).  Sets with an infinity
or a NaN go through the map update alone, in both of its forms: what the later phases make of a NaN is not this prefilter's business.

On the CPU: the bin and window rule, restated in numpy (tests/support/gate_index_reference.py), contains every pair the exact gates
accept, for the margin and seam inputs."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.support import gate_index_reference as gi
from tests.support import prefilter_reference as pr

GM_RTOL, GM_ATOL = 1e-10, 1e-12          # test_gpu_parity
WEIGHT_RTOL = 1e-9
CAP = 256
ENV_KEYS = ("RFSGPU_GATE_INDEX", "RFSGPU_FUSED_STEP", "RFSGPU_STEP_WPP", "RFSGPU_UPDMAP_WPP")
F32 = np.float32


# ---- scenarios -----------------------------------------------------------------------------------------------------------

def polar_scenario(sc, poses, rel, Z, params=None, cov=2.5e-3):
    """Landmark m of particle i at range rel[m][0], bearing rel[m][1] from pose i (so that the expected measurement is rel[m] to a
    rounding or two); weights 0.4 .. 0.7; C1's parameters unless overridden."""
    P = dict(sc.C1_PARAMS)
    P.update(params or {})
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 2)
    n, nM = len(poses), len(rel)
    mean = np.zeros((n, nM, 2))
    for i, (x, y, th) in enumerate(poses):
        mean[i, :, 0] = x + rel[:, 0] * np.cos(th + rel[:, 1])
        mean[i, :, 1] = y + rel[:, 0] * np.sin(th + rel[:, 1])
    return dict(n=n, nM=nM, params=P, poses=poses, pose_cov=np.asarray(P["pose_cov"]), w=np.tile(np.linspace(0.4, 0.7, nM), (n, 1)),
                mean=mean, cov=np.tile(np.diag([cov, cov]), (n, nM, 1, 1)), Z=np.asarray(Z, dtype=np.float64).reshape(-1, 2),
                particle_w=np.ones(n))


@functools.lru_cache(maxsize=None)
def _base(nM=70, nZ=20, seed=910, n=6):
    """make_scenario with half the set clutter, and -- from 128 landmarks up -- only 16 of them inside the sensing range, so that the
    new Gaussians of 64 measurements fit a capacity of 256 next to 200 old ones."""
    from __graft_entry__ import load_package
    sc = load_package().scenarios
    return sc.make_scenario(n, nM, nZ, seed=seed, n_clutter=(nZ // 2 if nZ > 1 else 0), frac_in_fov=(16.0 / nM if nM >= 128 else 1.0))


def base(**kw):
    s = _base(**kw)
    return dict(s, params=dict(s["params"]), Z=s["Z"].copy())


def _off_fp32(nominal, g):
    """pr._range_off_fp32 at the first range from `nominal` up (in steps of 1 m) for which its construction works."""
    for k in range(64):
        try:
            return pr._range_off_fp32(nominal + k, g)
        except AssertionError:
            continue
    raise ValueError(nominal)


def gate_margin_measurements(zexp, g_r, g_b, turns=0, deltas=(1e-6,)):
    """Measurements with an innovation within delta (relative) on either side of each gate, for one expected measurement."""
    out = []
    for dl in deltas:
        for sgn in (-1.0, 1.0):
            for side in (-1.0, 1.0):
                q = 1.0 + side * dl
                out.append((zexp[0] + sgn * g_r * q, zexp[1] + 0.3 * sgn * g_b))
                out.append((zexp[0] - 0.3 * sgn * g_r, zexp[1] + sgn * g_b * q + 2 * math.pi * turns))
    return out


# ---- running a case ------------------------------------------------------------------------------------------------------

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def snapshot(f, n, weights=True):
    """Everything the map update and the step leave, as arrays that compare bit for bit (a NaN equals itself)."""
    out = {"sizes": np.asarray(f.gm_sizes()).copy(), "fov": np.array([f.landmarks_in_fov(i) for i in range(n)])}
    if weights:
        out["weights"] = _bits(f.get_weights())
    for i in range(n):
        out[f"unused{i}"] = np.asarray(f.get_unused(i)).copy()
        w, wp, mu, S = f.export_gm(i)
        out[f"gm{i}"] = np.concatenate([_bits(w), _bits(wp), _bits(mu).ravel(), _bits(S).ravel()])
    return out


def assert_identical(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{label}: {k} differs between the index and the sweep"


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_both(pkg, sc, monkeypatch, scen, call="update", env=None, label=""):
    """The same case on a handle that uses the index and on one created under RFSGPU_GATE_INDEX=0: bit-identical.  Returns the
    indexed handle."""
    handles = []
    for idx in ("1", "0"):
        set_env(monkeypatch, dict(env or {}, RFSGPU_GATE_INDEX=idx))
        f = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=CAP)
        sc.load_scenario(f, scen)
        getattr(f, call)(scen["Z"])
        handles.append(f)
    set_env(monkeypatch, {})
    snaps = [snapshot(f, scen["n"]) for f in handles]
    assert_identical(snaps[0], snaps[1], f"{label} {call} {env or ''}")
    return handles[0]


def against_oracle(ob, sc, dev, scen, call="update", label="", weights=True):
    orc = ob.OracleFilter(scen["n"])
    sc.load_scenario(orc, scen)
    getattr(orc, call)(scen["Z"])
    assert np.array_equal(dev.gm_sizes(), orc.gm_sizes()), label
    for i in range(scen["n"]):
        sc.assert_gm_close(dev.export_gm(i), orc.export_gm(i), GM_RTOL, GM_ATOL, ordered=True)
        assert np.array_equal(dev.get_unused(i), orc.get_unused(i)), label
        assert dev.landmarks_in_fov(i) == orc.landmarks_in_fov(i), label
    if weights and call == "update":
        wd, wo = dev.get_weights(), orc.get_weights()
        np.testing.assert_allclose(wd / wd.sum(), wo / wo.sum(), rtol=WEIGHT_RTOL, atol=1e-300, err_msg=label)
    return orc


def check(pkg, ob, sc, monkeypatch, scen, label, calls=("update", "update_map"), oracle=True):
    for call in calls:
        dev = run_both(pkg, sc, monkeypatch, scen, call, label=label)
        if oracle:
            against_oracle(ob, sc, dev, scen, call, label)


# ---- CPU: the rule is a superset -----------------------------------------------------------------------------------------

def seam_case(sc):
    """Expected bearings within 1e-7 of +-pi (and a few farther in), a heading that is not zero, measurements at the gates on the
    other side of the seam."""
    th = 0.7
    eps = [0.0, 3e-8, 1e-7, 1e-3, 0.19, 0.21]
    rel = [(1.0 + 0.12 * k, s * (math.pi - e)) for k, (e, s) in enumerate([(e, s) for e in eps for s in (1.0, -1.0)])]
    Z = []
    for r, b in rel[:6]:
        Z += gate_margin_measurements((r, b), 1.0, 0.2)[1::2]            # bearing gate, from both sides: half of them past +-pi
    Z += [(r, -b) for r, b in rel[:6]]                                     # the mirror image: the other side of the seam
    Z = [(r, pr.wrap(b)) if k % 3 else (r, b) for k, (r, b) in enumerate(Z)]   # a third of them left outside [-pi, pi]
    poses = [[0.3, -0.2, th], [0.0, 0.0, -2.9], [-0.1, 0.1, 3.1]]
    return polar_scenario(sc, poses, rel, Z[:64])


def exact_pairs(scen, zexp):
    """(m, z) the innovation gates accept, in exact arithmetic on the given expected measurements."""
    P, Z = scen["params"], scen["Z"]
    out = []
    for m, (x0, x1) in enumerate(zexp):
        for z in range(len(Z)):
            ok, _ = pr.gate_rngbrg(Fraction(float(Z[z, 0])) - Fraction(float(x0)), Fraction(float(Z[z, 1])) - Fraction(float(x1)),
                                   P["kf_range"], P["kf_bearing"])
            if ok:
                out.append((m, z))
    return out


def test_index_windows_contain_every_accepted_pair(sc):
    """For the gate-margin sets (innovations at g (1 -+ 1e-6), expected bearings on either side of +-pi, up to 7 turns away) and the
    seam case, the numpy restatement of the bin and window rule lists every pair the exact gates accept -- and far fewer than all."""
    n_pairs = n_cand = n_acc = 0
    for kind in pr.GATE_SETS:
        for seed in (1, 2, 3):
            g = pr.rngbrg_gate_case(kind, seed=seed)
            P = g["params"]
            if kind == "past_50":
                assert not gi.usable(P["kf_range"], P["kf_bearing"], g["Z"])   # |bearing| >= 50: the sweep's business
                continue
            assert gi.usable(P["kf_range"], P["kf_bearing"], g["Z"])
            for i in range(g["n"]):
                cand = [gi.candidates(P["kf_range"], P["kf_bearing"], g["Z"], g["ranges"][m], -g["poses"][i][2]) for m in range(g["nM"])]
                for m, z in g["expect"][i]:
                    assert z in cand[m], (kind, seed, i, m, z)
                n_acc += len(g["expect"][i]); n_cand += sum(len(c) for c in cand); n_pairs += g["nM"] * len(g["Z"])
    s = seam_case(sc)
    P = s["params"]
    assert gi.usable(P["kf_range"], P["kf_bearing"], s["Z"])
    for i in range(s["n"]):
        zexp = []
        for m in range(s["nM"]):
            ze, _, _, _, _ = pr.np_measure(dict(P, R=np.asarray(P["R"])), s["poses"][i], s["pose_cov"], s["mean"][i][m], s["cov"][i][m])
            zexp.append(ze)
        acc = exact_pairs(s, zexp)
        assert len(acc) >= 4
        for m, z in acc:
            assert z in gi.candidates(P["kf_range"], P["kf_bearing"], s["Z"], zexp[m][0], zexp[m][1]), ("seam", i, m, z)
    assert n_acc > 100 and n_cand < 0.5 * n_pairs


def test_index_is_not_used_where_it_cannot_bound_the_set():
    Z = np.array([[1.0, 0.1], [2.0, -0.5]])
    assert gi.usable(1.0, 0.2, Z)
    assert not gi.usable(0.0, 0.2, Z) and not gi.usable(1.0, -1.0, Z) and not gi.usable(1.0, 3.2, Z)
    assert gi.usable(1e30, 0.2, Z) and not gi.usable(1e39, 0.2, Z)
    assert not gi.usable(1.0, 0.2, [[1.0, 0.1], [1.0, -0.5]])              # zero range span
    assert not gi.usable(1.0, 0.2, [[1.0, 0.1]])
    assert not gi.usable(1.0, 0.2, [[1.0, 50.0], [2.0, 0.0]]) and not gi.usable(1.0, 0.2, [[np.inf, 0.1], [2.0, 0.0]])
    assert not gi.usable(1.0, 0.2, [[1.0, np.inf], [2.0, 0.0]])
    assert gi.usable(1.0, 0.2, [[1.0, np.nan], [2.0, 0.0], [np.nan, 0.3]])  # a NaN is a candidate of every landmark instead
    assert gi.candidates(1.0, 0.2, [[1.0, np.nan], [2.0, 0.0], [np.nan, 0.3]], 30.0, 2.0) == {0, 2}


# ---- GPU -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nM", [1, 63, 64, 65, 128, 129, 200])
@pytest.mark.parametrize("nZ", [1, 2, 31, 32, 33, 63, 64])
def test_size_limits(pkg, ob, sc, monkeypatch, nZ, nM):
    scen = base(nM=nM, nZ=nZ, seed=1000 + 7 * nZ + nM, n=4)
    check(pkg, ob, sc, monkeypatch, scen, f"nZ={nZ} nM={nM}")


@pytest.mark.gpu
def test_the_seam(pkg, ob, sc, monkeypatch):
    check(pkg, ob, sc, monkeypatch, seam_case(sc), "seam")


def _shifted(scen):
    out = dict(scen, Z=scen["Z"].copy())
    out["Z"][:, 1] += np.array([2 * math.pi, -2 * math.pi, 4 * math.pi, 0.0])[np.arange(len(scen["Z"])) % 4]
    return out


def test_bearings_outside_minus_pi_pi_have_the_candidates_of_the_unshifted_set(sc):
    """Measurement bearings shifted by +-2 pi and +4 pi fall into the bins of the unshifted ones: every landmark keeps its candidates
    (the bearing threshold grows with max |bearing|, so a window may gain a bin, never lose one), and they hold every pair the exact
    gates accept -- the same pairs as unshifted, since the gates wrap."""
    scen = base()
    shifted = _shifted(scen)
    P = scen["params"]
    assert gi.usable(P["kf_range"], P["kf_bearing"], shifted["Z"])
    assert np.array_equal(gi.bearing_bins(scen["Z"][:, 1]), gi.bearing_bins(shifted["Z"][:, 1]))
    n_cand = 0
    for i in range(2):
        zexp = [pr.np_measure(dict(P, R=np.asarray(P["R"])), scen["poses"][i], scen["pose_cov"], scen["mean"][i][m], scen["cov"][i][m])[0]
                for m in range(scen["nM"])]
        acc, acc_s = exact_pairs(scen, zexp), exact_pairs(shifted, zexp)
        assert acc == acc_s and len(acc) > 20
        for m in range(scen["nM"]):
            a = gi.candidates(P["kf_range"], P["kf_bearing"], scen["Z"], zexp[m][0], zexp[m][1])
            b = gi.candidates(P["kf_range"], P["kf_bearing"], shifted["Z"], zexp[m][0], zexp[m][1])
            assert a <= b and len(b - a) <= 1, (i, m, a, b)
            assert {z for mm, z in acc if mm == m} <= b
            n_cand += len(b)
    assert n_cand < 0.2 * 2 * scen["nM"] * len(scen["Z"])


@pytest.mark.gpu
def test_bearings_outside_minus_pi_pi(pkg, ob, sc, monkeypatch):
    """Measurement bearings shifted by +-2 pi and +4 pi: index and sweep agree bit for bit, and with the oracle.  (A shifted measurement
    passes the innovation gates, which wrap, and then fails the Mahalanobis gate, which takes the raw difference: it creates nothing,
    in the reference as here.  That its CANDIDATES are those of the unshifted set is the CPU test above.)"""
    scen = base()
    ref = run_both(pkg, sc, monkeypatch, scen, "update_map", label="unshifted")
    shifted = _shifted(scen)
    for call in ("update", "update_map"):
        dev = run_both(pkg, sc, monkeypatch, shifted, call, label="shifted")
        against_oracle(ob, sc, dev, shifted, call, "shifted")
    assert np.all(dev.gm_sizes() <= ref.gm_sizes()) and np.all(dev.gm_sizes() > scen["nM"])
    for i in range(scen["n"]):
        assert dev.landmarks_in_fov(i) == ref.landmarks_in_fov(i)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["past_50", "inf_range", "inf_bearing", "nan_range", "nan_bearing", "nan_both"])
def test_sets_the_sweep_keeps(pkg, ob, sc, monkeypatch, what):
    """|bearing| >= 50 and infinities send the whole particle to the sweep; a NaN stays a candidate of every landmark, as in the
    sweep, and the exact gates deal with it."""
    scen = base()
    Z = scen["Z"]
    if what == "past_50":
        Z[3, 1] += 16 * math.pi
        Z[7, 1] -= 18 * math.pi
    elif what == "inf_range":
        Z[3, 0] = np.inf
    elif what == "inf_bearing":
        Z[3, 1] = np.inf
    elif what == "nan_range":
        Z[3, 0] = np.nan
    elif what == "nan_bearing":
        Z[3, 1] = np.nan
    else:
        Z[3] = np.nan
        Z[11, 1] = np.nan
    for env in ({}, {"RFSGPU_UPDMAP_WPP": "1"}):              # the workgroup form and the one-wave form of the map update
        dev = run_both(pkg, sc, monkeypatch, scen, "update_map", env=env, label=what)
        if what != "inf_bearing":
            against_oracle(ob, sc, dev, scen, "update_map", what)
    if what == "past_50":
        against_oracle(ob, sc, run_both(pkg, sc, monkeypatch, scen, "update", label=what), scen, "update", what)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", pr.GATE_SETS)
def test_gate_margins(pkg, ob, sc, monkeypatch, kind):
    """Innovations within 1e-6 (relative) on either side of kf_range and of kf_bearing: the certified decisions, by the index."""
    g = pr.rngbrg_gate_case(kind, seed=1)
    for call in ("update_map", "update"):
        dev = run_both(pkg, sc, monkeypatch, g, call, label=kind)
        if call == "update_map":
            against_oracle(ob, sc, dev, g, call, kind)
            np.testing.assert_array_equal(dev.gm_sizes(), [g["nM"] + len(e) for e in g["expect"]])


def bin_edge_case(sc):
    """Measurement bearings and ranges one fp32 ulp on either side of bin boundaries (the ranges span [1, 2] exactly: 64 bins of
    1/64), and landmarks whose windows end within an ulp or two of a boundary; every landmark also gets measurements at its gates."""
    kfr, kfb = 0.25, 0.2
    edges_b = [F32(-np.pi + k * 2 * np.pi / 256) for k in (0, 1, 37, 128, 200, 255, 256)]
    edges_r = [F32(1 + k / 64) for k in (1, 17, 32, 63)]
    Z = [(1.0, 0.05), (2.0, -0.05)]
    for e in edges_b:
        for d in (-1, 0, 1):
            b = e if d == 0 else np.nextafter(e, F32(d * 10))
            Z.append((1.5, float(b)))
    for e in edges_r:
        for d in (-1, 0, 1):
            r = e if d == 0 else np.nextafter(e, F32(d * 10))
            Z.append((float(r), float(edges_b[2])))
    zb_max = max(abs(b) for _, b in Z)
    thr_b, _ = gi.thresholds(kfr, kfb, 2.0, zb_max, 1.5)
    rel = []
    for e in (edges_b[2], edges_b[4]):
        for j in (-2, 0, 1):                                    # fl(c + thrB) within an ulp or two of the boundary, and c - thrB likewise
            c = F32(e - thr_b)
            for _ in range(abs(j)):
                c = np.nextafter(c, F32(j * 10))
            rel.append((1.5, float(c)))
            rel.append((1.25, float(F32(e + thr_b))))
    for e in edges_r[:2]:
        _, thr_r = gi.thresholds(kfr, kfb, 2.0, zb_max, float(e))
        rel.append((float(F32(e - thr_r)), float(edges_b[2])))
        rel.append((float(F32(e + thr_r)), float(edges_b[2])))
    for r, b in rel[:2] + rel[-2:]:
        Z += gate_margin_measurements((r, b), kfr, kfb)[:4]
    assert len(Z) <= 64
    return polar_scenario(sc, [[0.0, 0.0, 0.0], [0.0, 0.0, 0.4]], rel, Z, params=dict(kf_range=kfr, kf_bearing=kfb, rmax=3.0, rmin=0.2))


@pytest.mark.gpu
def test_bin_edges(pkg, ob, sc, monkeypatch):
    check(pkg, ob, sc, monkeypatch, bin_edge_case(sc), "bin edges")


@pytest.mark.gpu
@pytest.mark.parametrize("gates", [dict(kf_bearing=0.0), dict(kf_bearing=-1.0), dict(kf_bearing=3.2), dict(kf_range=0.0), dict(kf_range=-2.0),
                                   dict(kf_range=1e30), dict(kf_range=1e30, kf_bearing=3.2)])
def test_gates_disabled_or_wide_open(pkg, ob, sc, monkeypatch, gates):
    scen = base(nM=40, nZ=16, seed=77)
    scen["params"].update(gates)
    check(pkg, ob, sc, monkeypatch, scen, str(gates))


def ob_sizes_min(ob, sc, scen):
    orc = ob.OracleFilter(scen["n"])
    sc.load_scenario(orc, scen)
    orc.update_map(scen["Z"])
    return orc.gm_sizes().min()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["identical", "equal_ranges", "far"])
def test_degenerate_measurement_sets(pkg, ob, sc, monkeypatch, what):
    """64 identical measurements (one bin holds every bit; zero range span); all ranges equal; ranges of order 1e4 seen from a pose
    1e4 from the origin (an fp32 ulp of 1e-3 m: the range guards at work)."""
    if what == "identical":
        scen = base(nM=12, nZ=8, seed=31, n=4)
        gt = scen["gt"][np.nonzero(scen["in_fov"])[0][0]]                  # a landmark every particle holds: 64 new Gaussians each
        scen["Z"] = np.tile([[math.hypot(gt[0], gt[1]), math.atan2(gt[1], gt[0])]], (64, 1))
        for env in ({}, {"RFSGPU_UPDMAP_WPP": "1"}):      # (the map update alone: 64 equal measurements are beyond the weighting's partition limits)
            against_oracle(ob, sc, run_both(pkg, sc, monkeypatch, scen, "update_map", env=env, label=what), scen, "update_map", what)
        assert int(ob_sizes_min(ob, sc, scen)) >= 12 + 64
        return
    elif what == "equal_ranges":
        scen = base(nM=40, nZ=24, seed=32)
        scen["Z"][:, 0] = 1.5
    else:
        g_r, g_b = pr.RNGBRG_GATE_RANGE, 0.2
        rel = [(_off_fp32(1e4 + 37.0 * k, g_r), -2.5 + 0.9 * k) for k in range(6)]
        Z = []
        for r, b in rel:
            Z += gate_margin_measurements((r, b), g_r, g_b)
        P = dict(pr.rngbrg_gate_case("range", seed=1)["params"])
        scen = polar_scenario(sc, [[1e4, 0.0, 0.0], [0.0, -1e4, 0.0], [-7e3, 7e3, 0.0]], rel, Z, params=P, cov=1e-2)
        run_both(pkg, sc, monkeypatch, scen, "update", label=what)       # (the oracle on the map update only, as test_prefilter_margins)
        check(pkg, ob, sc, monkeypatch, scen, what, calls=("update_map",))
        return
    check(pkg, ob, sc, monkeypatch, scen, what)


@pytest.mark.gpu
@pytest.mark.parametrize("env,call", [({"RFSGPU_STEP_WPP": "2"}, "update"), ({"RFSGPU_STEP_WPP": "3"}, "update"),
                                      ({"RFSGPU_FUSED_STEP": "0"}, "update"), ({"RFSGPU_UPDMAP_WPP": "1"}, "update_map"),
                                      ({"RFSGPU_UPDMAP_WPP": "3"}, "update_map"), ({"RFSGPU_UPDMAP_WPP": "4"}, "update_map")])
def test_kernel_forms(pkg, ob, sc, monkeypatch, env, call):
    """The fused step with two and three waves per particle, the unfused step, and the stand-alone map update as one wave per
    particle and as workgroups of three and four waves."""
    for scen in (base(nM=130, nZ=30, seed=5), seam_case(sc)):
        dev = run_both(pkg, sc, monkeypatch, scen, call, env=env, label=str(env))
        against_oracle(ob, sc, dev, scen, call, str(env))


@pytest.mark.gpu
def test_the_predict_head_and_a_batch_of_two(pkg, ob, sc, monkeypatch):
    """The step with the predict at its head (a cycle), and one batch of two filters with different measurement counts, one of them
    zero: index and sweep bit-identical; the batch's filters against the oracle."""
    from tests.test_filter_batch import _configure_from_scenario
    nP = 4
    scens = [base(nM=70, nZ=20, seed=910, n=nP), base(nM=40, nZ=16, seed=77, n=nP)]
    Zs = [scens[0]["Z"], np.zeros((0, 2))]
    snaps = []
    for idx in ("1", "0"):
        set_env(monkeypatch, {"RFSGPU_GATE_INDEX": idx})
        f = pkg.RBPHDFilter(nP, device_id=0, gm_capacity=CAP)
        sc.load_scenario(f, scens[0])
        f.cycle_async(None, scens[0]["Z"], normalize=True)
        f.cycle_async(True, scens[0]["Z"][:13], normalize=True)
        f.synchronize()
        batch = pkg.FilterBatch(2, nP, gm_capacity=CAP)
        batch.set_poses(np.vstack([s["poses"] for s in scens]), np.vstack([np.tile(np.asarray(s["pose_cov"]).ravel(), (nP, 1)) for s in scens]))
        batch.set_weights(np.ones(2 * nP))
        for b, s in enumerate(scens):
            _configure_from_scenario(pkg.capi, batch, b, s["params"])
            for i in range(nP):
                batch.import_gm(b * nP + i, s["w"][i], s["mean"][i], s["cov"][i])
        batch.cycle_async(None, Zs, normalize=True)
        batch.synchronize()
        snaps.append((snapshot(f, nP), snapshot(batch, 2 * nP)))
    set_env(monkeypatch, {})
    assert_identical(snaps[0][0], snaps[1][0], "cycle with the predict head")
    assert_identical(snaps[0][1], snaps[1][1], "batch")
    orc = ob.OracleFilter(nP)
    sc.load_scenario(orc, scens[0])
    orc.update(scens[0]["Z"])
    sizes, w = batch.gm_sizes(), batch.get_weights()
    assert np.array_equal(sizes[:nP], orc.gm_sizes())
    wo = orc.get_weights()
    np.testing.assert_allclose(w[:nP] / w[:nP].sum(), wo / wo.sum(), rtol=WEIGHT_RTOL)
    for i in range(nP):
        sc.assert_gm_close(batch.export_gm(i), orc.export_gm(i), GM_RTOL, GM_ATOL, ordered=True)
        assert np.array_equal(batch.get_unused(i), orc.get_unused(i))
        d = batch.export_gm(nP + i)                                   # the filter without measurements: its mixture as it was
        assert np.array_equal(d[0], scens[1]["w"][i]) and np.array_equal(d[2], scens[1]["mean"][i])
