"""The whole RBPHDFilter::update on the device (rfsgpu_rbphd_cycle_async; csrc/birth_walk.h) and the birth predict behind it, whose
inheritance walk (RBPHDFilter.hpp:1005-1011) is made on the device from the ids the device holds.

Yardstick: the host-stop route on a second handle given the same state, measurements, scan and draws
(tests/support/rbphd_device_cycle_reference.py, HostRoute): the same kernels on the same inputs in the same order, so weights,
ordered maps, unused lists, candidate lists, FOV counts, poses, ids, parent ids, resampleOccured, fired, N_eff and the plan are
compared bit for bit."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.support import rbphd_device_cycle_reference as ref

gpu = pytest.mark.gpu
ROOT = ref.ROOT

CYCLE_ARGS = {
    "rfsgpu_rbphd_set_resampling": "rfsgpu_filter *f, double eff_n, double eff_n_percent",
    "rfsgpu_rbphd_cycle_async": "rfsgpu_filter *f, const double *z, int n_z, const double *scan, int n_scan, double u01",
    "rfsgpu_rbphd_cycle_counts": "rfsgpu_filter *f, int *n_cycles, int *n_gate_open, int *n_resamplings, int *max_level",
    "rfsgpu_rbphd_last_cycle": "rfsgpu_filter *f, int *gate_open, int *fired, double *n_eff, int *plan, int max_n, int *walk_levels",
}


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_with_the_headers_argument_lists(pkg):
    lib = pkg.load_library()
    for name, args in CYCLE_ARGS.items():
        assert hasattr(lib, name), name
        assert ref.declared_args(name) == args, (name, ref.declared_args(name))
        assert name[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    assert hasattr(lib, "rfsgpu_rbphd_cycle_pending")
    assert ref.walk_levels_constant() >= 1


def test_null_handle_is_invalid(pkg):
    lib = pkg.load_library()
    z = (C.c_double * 2)(1.0, 0.1)
    i4 = [C.c_int() for _ in range(4)]
    d = C.c_double()
    for fn, args in ((lib.rfsgpu_rbphd_set_resampling, (None, C.c_double(1.0), C.c_double(0.25))),
                     (lib.rfsgpu_rbphd_cycle_async, (None, z, C.c_int(1), None, C.c_int(0), C.c_double(0.5))),
                     (lib.rfsgpu_rbphd_cycle_counts, (None, C.byref(i4[0]), C.byref(i4[1]), C.byref(i4[2]), C.byref(i4[3]))),
                     (lib.rfsgpu_rbphd_last_cycle, (None, C.byref(i4[0]), C.byref(i4[1]), C.byref(d), None, C.c_int(0), C.byref(i4[2])))):
        fn.restype = C.c_int
        assert fn(*args) == pkg.capi.ERR_INVALID
    lib.rfsgpu_rbphd_cycle_pending.restype = C.c_int
    assert lib.rfsgpu_rbphd_cycle_pending(None) == 0


def test_n_eff_restatement_rounds_once_per_particle():
    """On weights whose squares are exact the fused chain is the plain slot-ordered sum; on random weights it stays within n
    roundings of it and is not always equal to it (it is the kernel's arithmetic, not numpy's)."""
    w = np.array([0.5, 0.25, 0.125, 0.125])
    assert ref.n_eff_slot_order(w) == 1.0 / float(np.cumsum(w * w)[-1]) == 1.0 / 0.34375
    rng = np.random.default_rng(2)
    differs = 0
    for _ in range(200):
        w = rng.random(16)
        w /= np.cumsum(w)[-1]
        fused, plain = ref.n_eff_slot_order(w), 1.0 / float(np.cumsum(w * w)[-1])
        assert abs(fused - plain) <= 16 * 2.0 ** -52 * plain
        s = Fraction(0)
        for v in w:                                    # the first step on its own: one rounding of the exact square
            s = Fraction(float(s + Fraction(float(v)) ** 2))
        assert fused == 1.0 / float(s)
        differs += fused != plain
    assert differs > 0


def _planted_chain(n):
    return np.maximum(np.arange(n) - 1, 0)


def test_levels_rule_equals_the_loop_of_predict_launch():
    rng = np.random.default_rng(11)
    cases = [_planted_chain(n) for n in (1, 2, ref.walk_levels_constant() + 4, 70)]
    cases += [np.arange(9), np.array([3, 3, 3, 3]), np.array([-1, 0, 1, 99, 3])]          # identity | parents above | ids that are no slot
    for n in (1, 2, 24, 65, 257):
        for _ in range(20):
            cases.append(rng.integers(-2, n + 2, n))
            src = np.sort(rng.integers(0, n, n))                                          # ids as resamplings leave them: many copies of a few
            cases.append(src[rng.permutation(n)] if rng.random() < 0.5 else src)
    for ppid in cases:
        a, b = ref.levels_loop(ppid), ref.levels_chase(ppid)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3], ppid
    n = ref.walk_levels_constant() + 4
    assert ref.levels_loop(_planted_chain(n))[3] == n - 1 and list(ref.levels_chase(_planted_chain(n))[1]) == list(range(n))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _scenario(sc, model, n, n_landmarks=3, n_z=4, seed=31):
    if model == "vp":
        return sc.make_vp_scenario(n, n_landmarks + 1, n_z, seed=seed)
    return sc.make_scenario(n, n_landmarks, n_z, seed=seed)


BRANCHES = {"closed": dict(min_updates=5, eff=None), "open": dict(min_updates=1, eff=(0.0, 0.0)), "fire": dict(min_updates=1, eff="n+1")}
ONE_CYCLE = [(n, m, t) for n in (1, 2, 63, 65, 257) for m in ("2d", "vp") for t in (1, 3)] + [(2049, "2d", 3)]


@gpu
@pytest.mark.parametrize("n,model,thr", ONE_CYCLE)
def test_one_cycle_on_each_branch(pkg, sc, n, model, thr):
    """Gate closed (minUpdatesBeforeResample 5 at the first update), gate open without firing (thresholds 0: N_eff > 0 always) and
    firing (eff_n = n + 1 > N_eff always): the host route alone shows the branch, then everything is compared."""
    scen = _scenario(sc, model, n)
    for branch, b in BRANCHES.items():
        eff = (n + 1.0, 0.0) if b["eff"] == "n+1" else (b["eff"] or (n / 4.0, 0.25))
        host, dev = ref.make_pair(pkg, sc, scen, thr, b["min_updates"], eff[0], eff[1])
        h = host.update(scen["Z"], 0.37, scan=scen.get("scan"))
        assert (h["gate_open"], h["fired"]) == {"closed": (False, False), "open": (True, False), "fire": (True, True)}[branch]
        ref.device_update(dev, scen["Z"], 0.37, scan=scen.get("scan"))
        assert dev.rbphd_cycle_pending()
        lc = dev.rbphd_last_cycle()
        assert not dev.rbphd_cycle_pending()
        ref.same_outcome(h, lc)
        cnt = dev.rbphd_cycle_counts()
        assert (cnt["n_cycles"], cnt["n_gate_open"], cnt["n_resamplings"]) == (1, int(h["gate_open"]), int(h["fired"]))
        a, b2 = ref.state(host.f), ref.state(dev)
        assert a["resampled"] == h["fired"]
        ref.assert_same_state(a, b2)
        host.f.close(); dev.close()


@gpu
def test_update_without_measurements_is_only_counted(pkg, sc):
    """minUpdatesBeforeResample 2: an empty update changes nothing but the count, and the first update with measurements behind it
    finds the gate open -- without it the gate is closed."""
    scen = _scenario(sc, "2d", 9)
    host, dev = ref.make_pair(pkg, sc, scen, 1, 2, 10.0, 0.0)
    before = ref.state(dev)
    empty = np.zeros((0, 2))
    host.update(empty, 0.0)
    ref.device_update(dev, empty, 0.0)
    assert dev.rbphd_cycle_pending()
    lc = dev.rbphd_last_cycle()
    assert not lc["gate_open"] and not lc["fired"] and lc["n_eff"] == 0.0 and np.array_equal(lc["plan"], np.arange(9))
    ref.assert_same_state(before, ref.state(dev))
    h = host.update(scen["Z"], 0.6)
    ref.device_update(dev, scen["Z"], 0.6)
    assert h["gate_open"] and h["fired"]
    ref.same_outcome(h, dev.rbphd_last_cycle())
    assert dev.rbphd_cycle_counts()["n_cycles"] == 2
    ref.assert_same_state(ref.state(host.f), ref.state(dev))
    host.f.close(); dev.close()
    host, dev = ref.make_pair(pkg, sc, scen, 1, 2, 10.0, 0.0)
    assert not host.update(scen["Z"], 0.6)["gate_open"]
    ref.device_update(dev, scen["Z"], 0.6)
    assert not dev.rbphd_last_cycle()["gate_open"]
    host.f.close(); dev.close()


def _perturbed(scen, rng):
    Z = scen["Z"].copy()
    Z[:, 0] += rng.normal(0, 2e-3, Z.shape[0])
    return Z


@gpu
@pytest.mark.parametrize("model", ["vp", "2d", "2d-eager"])
def test_birth_predict_behind_a_pending_cycle(pkg, sc, model):
    """cycle that fires -> birth predict -> a second birth predict (resampleOccured_ still set) -> cycle -> birth predict.  On one
    device handle nothing is read before the end (the predicate says so); a second one is compared after every step.  2d-eager:
    RFSGPU_INHERIT_EAGER, where the lists travel with the copies and the predict has no walk to make."""
    n = 24
    eager = model.endswith("-eager")
    model = model.split("-")[0]
    scen = sc.make_vp_scenario(n, 10, 7, seed=3) if model == "vp" else sc.make_scenario(n, 8, 9, seed=21)
    rng = np.random.default_rng(5)
    Zs = [_perturbed(scen, rng), _perturbed(scen, rng)]
    host, dev = ref.make_pair(pkg, sc, scen, 5 if model == "vp" else 3, 1, n + 1.0, 0.0, cap=192)
    _, step = ref.make_pair(pkg, sc, scen, 5 if model == "vp" else 3, 1, n + 1.0, 0.0, cap=192)
    _.f.close()
    if eager:
        for f in (host.f, dev, step):
            f.set_birth_inheritance(pkg.capi.INHERIT_EAGER)
    fired = []

    def both(fn_host, fn_dev):
        fn_host(host.f)
        for f in (dev, step):
            fn_dev(f)
        assert dev.rbphd_cycle_pending()
        ref.assert_same_state(ref.state(host.f), ref.state(step))

    for f in (host.f, dev, step):
        f.predict_map(True)
    for k, Z in enumerate(Zs):
        fired.append(host.update(Z, 0.3 + 0.2 * k, scan=scen.get("scan"))["fired"])
        for f in (dev, step):
            ref.device_update(f, Z, 0.3 + 0.2 * k, scan=scen.get("scan"))
        assert dev.rbphd_cycle_pending()
        ref.assert_same_state(ref.state(host.f), ref.state(step))
        for _ in range(2 if k == 0 else 1):
            both(lambda f: f.predict_map(True), lambda f: f.predict_map_async(True))
    assert fired == [True, True]
    assert np.any(ref.state(host.f)["parents"] != np.arange(n)), "no slot has a foreign parent: the walk was not exercised"
    assert dev.rbphd_cycle_pending()            # nothing has resolved on this handle: two cycles and three birth predicts are enqueued
    ref.assert_same_state(ref.state(host.f), ref.state(dev))
    assert not dev.rbphd_cycle_pending()
    assert dev.rbphd_cycle_counts()["n_resamplings"] == 2
    for f in (host.f, dev, step):
        f.close()


def _chain_pair(pkg, sc, model, thr, n, n_z=5, n_cand=1):
    """N particles with equal weights after every update.  thr 1: empty maps, every measurement unused (test_birth_inheritance's
    _setup_immediate).  thr 3: every particle holds particle 0's pose and one-landmark map (a landmark in the FOV keeps the births
    out of the immediate branch), and slot i carries n_cand + i imported candidates."""
    if thr == 1:
        scen = sc.make_scenario(n, 0, n_z, seed=5)
        host, dev = ref.make_pair(pkg, sc, scen, 1, 1, n + 1.0, 0.0)
    else:
        scen = sc.make_vp_scenario(n, 1, n_z, seed=8, frac_in_fov=1.0) if model == "vp" else sc.make_scenario(n, 1, n_z, seed=8)
        host, dev = ref.make_pair(pkg, sc, scen, 3, 1, n + 1.0, 0.0, check_thr=100, same_particles=True)
        for f in (host.f, dev):
            for i in range(n):
                f.import_birth_candidates(i, *ref.far_candidates(n_cand + i, f.dm, 1000.0 + 100.0 * i))
    ids = np.maximum(np.arange(n) - 1, 0).astype(np.int32)
    for f in (host.f, dev):
        f.set_particle_ids(ids, ids)
    return scen, host, dev


@gpu
@pytest.mark.parametrize("model,thr,n_cand", [("2d", 1, 0), ("2d", 3, 1), ("vp", 3, 1), ("2d", 3, 70), ("vp", 3, 70)])
def test_chain_beyond_the_fixed_level_launches(pkg, sc, model, thr, n_cand):
    """id[i] = parent_id[i] = max(i - 1, 0), equal weights, u01 = 0.5: the resampling fires, every slot keeps itself and takes its
    own id as parent, and the walk is one chain of depth N - 1 = RFSGPU_RBPHD_WALK_LEVELS + 3: the last three levels are the tail
    kernel's.  n_cand 70: slot 0's list, which every slot ends up walking, is longer than a wavefront, so every birth step --
    the tail kernel's included, by both of its waves -- is the one that stages the list in LDS (birth_step_lds)."""
    n = ref.walk_levels_constant() + 4
    scen, host, dev = _chain_pair(pkg, sc, model, thr, n, n_cand=max(n_cand, 1))
    h = host.update(scen["Z"], 0.5, scan=scen.get("scan"))
    assert h["fired"] and np.array_equal(h["plan"], np.arange(n)), "the weights are not equal: a slot was copied"
    assert np.all(host.f.get_weights() == 1.0)
    parents = host.f.get_particle_ids()[1]
    assert list(parents) == [max(i - 1, 0) for i in range(n)]
    assert ref.levels_loop(parents)[3] == n - 1
    ref.device_update(dev, scen["Z"], 0.5, scan=scen.get("scan"))
    host.f.predict_map(True)
    dev.predict_map_async(True)
    assert dev.rbphd_cycle_pending()
    a, b = ref.state(host.f), ref.state(dev)
    lc, cnt = dev.rbphd_last_cycle(), dev.rbphd_cycle_counts()
    assert cnt["max_level"] == n - 1 and lc["walk_levels"] == n - 1
    if thr == 1:
        nz = scen["Z"].shape[0]
        assert list(a["sizes"]) == [nz] + [0] * (n - 1)         # slot 0 bears its own list; every later slot copies a list already consumed
        assert list(b["sizes"]) == [nz] + [0] * (n - 1)
    else:
        chk = [list(c[3]) for c in a["cands"]]
        assert all(len(c) == len(chk[0]) and len(c) >= max(n_cand, 1) for c in chk), "every slot ends with slot 0's list"
        assert [c[0] for c in chk] == list(range(1, n + 1)), "the check counts grow along the chain"
    ref.assert_same_state(a, b)
    host.f.close(); dev.close()


@gpu
@pytest.mark.parametrize("bad", [float("nan"), -0.25, float("inf")])
def test_bad_weights_are_reported_once_and_the_tail_touches_nothing(pkg, sc, bad):
    """A weight that cannot be resampled in front of a cycle whose gate is open: the cycle is enqueued without complaint, its tail
    normalises, moves and resets nothing -- the handle equals one that ran the update alone --, and the next resolving call returns
    RFSGPU_ERR_INVALID once."""
    n = 9
    scen = _scenario(sc, "2d", n)
    host, dev = ref.make_pair(pkg, sc, scen, 1, 1, n + 1.0, 0.0)
    w = np.linspace(0.5, 1.5, n)
    w[4] = bad
    for f in (host.f, dev):
        f.set_weights(w)
    host.f.cycle_async(None, scen["Z"], normalize=False)            # the update and nothing behind it
    ref.device_update(dev, scen["Z"], 0.5)
    assert dev.rbphd_cycle_pending()
    with pytest.raises(pkg.capi.EngineError) as e:
        dev.synchronize()
    assert e.value.status == pkg.capi.ERR_INVALID and "weight" in str(e.value)
    dev.synchronize()                                                # once
    lc, cnt = dev.rbphd_last_cycle(), dev.rbphd_cycle_counts()
    assert not lc["fired"] and np.array_equal(lc["plan"], np.arange(n)) and lc["n_eff"] == 0.0
    assert (cnt["n_cycles"], cnt["n_gate_open"], cnt["n_resamplings"]) == (1, 0, 0)
    a, b = ref.state(host.f), ref.state(dev)
    assert np.array_equal(a["w"], b["w"], equal_nan=True) and not np.all(np.isfinite(b["w"]) & (b["w"] >= 0))
    a["w"] = b["w"] = np.zeros(n)
    ref.assert_same_state(a, b)
    assert not b["resampled"] and np.array_equal(b["ids"], np.arange(n))
    ref.device_update(dev, scen["Z"], 0.5)                           # the handle goes on: the next cycle meets the same weights again
    with pytest.raises(pkg.capi.EngineError):
        dev.synchronize()
    host.f.close(); dev.close()


PLANTED = [[2, 5, 10, 17], [2, 13]]


@gpu
@pytest.mark.parametrize("mode", ["immediate", "candidates", "vp"])
def test_random_plans_over_ten_steps(pkg, sc, mode):
    """After test_device_resampling_cycles_match_oracle: predict / cycle over ten steps, two predicts after some cycles, the gate
    closed on every other update (minUpdatesBeforeResample 2).  A systematic plan from real weights does not build a chain of
    lower-slot parents by itself, so the weights in front of the first two resamplings are planted (set_weights resolves: fine here):
    survivors 2, 5, 10, 17 put copies of slot 10 into slots above it (13 among them), then survivors 2 and 13 put slot 2 into slot 10
    while slot 13 (id 10) is copied upwards -- two levels.  Later resamplings use the weights as they come."""
    rng = np.random.default_rng(17)
    n = 24
    scen = sc.make_vp_scenario(n, 10, 7, seed=3) if mode == "vp" else sc.make_scenario(n, 8, 9, seed=21)
    host, dev = ref.make_pair(pkg, sc, scen, 1 if mode == "immediate" else 3, 2, n + 1.0, 0.0, cap=192)
    max_level, n_res = 0, 0
    for step in range(10):
        Z = _perturbed(scen, rng)
        if step % 3 == 1:
            Z[-2:, 0] = rng.uniform(6.0, 9.0, 2) if mode == "vp" else rng.uniform(1.0, 2.0, 2)
        for k in range(2 if step % 4 == 2 else 1):
            host.f.predict_map(True)
            dev.predict_map_async(True)
        if step % 2 == 1 and n_res < len(PLANTED):      # the gate opens on this update
            w = np.full(n, 1e-12)
            w[PLANTED[n_res]] = 1.0
            for f in (host.f, dev):
                f.set_weights(w)
        u01 = float(rng.uniform())
        h = host.update(Z, u01, scan=scen.get("scan"))
        ref.device_update(dev, Z, u01, scan=scen.get("scan"))
        assert h["gate_open"] == (step % 2 == 1) and h["fired"] == h["gate_open"]
        n_res += int(h["fired"])
        if h["fired"]:
            max_level = max(max_level, ref.levels_loop(host.f.get_particle_ids()[1])[3])
        if step % 3 != 0:
            assert dev.rbphd_cycle_pending()
            ref.same_outcome(h, dev.rbphd_last_cycle())
            ref.assert_same_state(ref.state(host.f), ref.state(dev))
    assert n_res == 5 and max_level >= 2
    ref.assert_same_state(ref.state(host.f), ref.state(dev))
    cnt = dev.rbphd_cycle_counts()
    assert (cnt["n_cycles"], cnt["n_gate_open"], cnt["n_resamplings"]) == (10, 5, 5) and cnt["max_level"] >= 2
    host.f.close(); dev.close()


@gpu
def test_refusals_leave_the_state_untouched(pkg, sc):
    capi = pkg.capi
    scen = _scenario(sc, "2d", 8)

    def refused(f, status, word, Z=None, u01=0.5):
        Z = np.ascontiguousarray(scen["Z"] if Z is None else Z, dtype=np.float64)
        with pytest.raises(capi.EngineError) as e:
            f._call("rbphd_cycle_async", f._ptr(Z), C.c_int(Z.shape[0]), None, C.c_int(0), C.c_double(u01))
        assert e.value.status == status and word in str(e.value), str(e.value)

    batch = pkg.FilterBatch(2, 16, gm_capacity=32)
    w0 = batch.get_weights().copy()
    refused(batch, capi.ERR_UNSUPPORTED, "batch")
    assert np.array_equal(batch.get_weights(), w0)
    batch.close()
    group = pkg.FilterGroup(8, [0, 0], gm_capacity=64)
    refused(group.shards[0], capi.ERR_UNSUPPORTED, "rfsgpu_group")
    group.close()
    f = pkg.RBPHDFilter(8, gm_capacity=64)
    sc.load_scenario(f, scen)
    before = ref.state(f)
    f.set_birth_inheritance(capi.INHERIT_EXTERNAL)
    refused(f, capi.ERR_UNSUPPORTED, "RFSGPU_INHERIT_EXTERNAL")
    f.set_birth_inheritance(capi.INHERIT_REFERENCE)
    for u in (1.0, -1e-9, float("nan")):
        refused(f, capi.ERR_INVALID, "u01", u01=u)
    refused(f, capi.ERR_INVALID, "RFSGPU_MAX_Z", Z=np.ones((capi.MAX_Z + 1, 2)))
    assert not f.rbphd_cycle_pending()
    with pytest.raises(capi.EngineError) as e:
        f.rbphd_last_cycle()
    assert e.value.status == capi.ERR_INVALID
    ref.assert_same_state(before, ref.state(f))
    # the host route first and the cycle later is allowed (the host's ids go up); the other direction is refused
    f.update(scen["Z"])
    f.normalize_weights(f.weight_sums()[0])
    plan = np.array([0, 0, 2, 2, 4, 5, 5, 7], dtype=np.int32)
    f.resample_apply(plan)
    ids = f.get_particle_ids()
    f.rbphd_set_resampling(0.0, 0.0)
    f.rbphd_cycle_async(scen["Z"], 0.5)
    assert not f.rbphd_last_cycle()["fired"]
    assert np.array_equal(f.get_particle_ids()[0], ids[0]) and np.array_equal(f.get_particle_ids()[1], ids[1])
    w0 = f.get_weights().copy()
    for call in (lambda: f.resample_apply(plan), lambda: f.resample_async(2.0, 0.25, 0.5)):
        with pytest.raises(capi.EngineError) as e:
            call()
        assert e.value.status == capi.ERR_UNSUPPORTED and "rfsgpu_rbphd_cycle_async" in str(e.value)
    assert np.array_equal(f.get_weights(), w0)
    f.close()
    fs = pkg.RBPHDFilter(4, gm_capacity=64, max_particles=64)
    scen4 = sc.make_scenario(4, 6, 5, seed=2)
    sc.load_scenario(fs, scen4)
    fs.set_fastslam_config(fs.default_fastslam_config())
    fs.fastslam_update(scen4["Z"])
    w0 = fs.get_weights().copy()
    with pytest.raises(capi.EngineError) as e:
        fs.rbphd_cycle_async(scen4["Z"], 0.5)
    assert e.value.status == capi.ERR_UNSUPPORTED and "FastSLAM" in str(e.value)
    assert np.array_equal(fs.get_weights(), w0)
    fs.close()
    vp = pkg.RBPHDFilter(4, gm_capacity=64, model=capi.MODEL_VICTORIAPARK_3D)       # a Victoria Park handle that has never seen a scan
    with pytest.raises(capi.EngineError) as e:
        vp.rbphd_cycle_async(np.array([[10.0, 1.0, 0.5]]), 0.5)
    assert e.value.status == capi.ERR_INVALID and "scan" in str(e.value)
    vp.close()


# The XML's values (scenarios.VP_PARAMS holds them: minUpdates 2, minMeasurements 15) and the driver's default threshold
# eff_n = n / 2 = 50 give, on the 900-message extract, both a resampling and an update behind a closed gate: asserted below on the
# host-stop route alone.
VP_DRIVER_EFF_N = None


def _driver_run(pkg, sc, n, **opts):
    f = pkg.RBPHDFilter(n, gm_capacity=192, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    P = dict(sc.VP_PARAMS)
    sc.apply_vp_params(f, P, np.full(361, 70.0))
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    return pkg.vp_driver.VictoriaParkRun(f, data, P, seed=5, filter="rbphd", eff_n=VP_DRIVER_EFF_N, **opts).run(n_messages=900)


@gpu
def test_victoria_park_driver_on_three_routes(pkg, sc):
    """900 messages of the extract (89 lidar updates), 100 particles, the XML's values: the host-stop route with device motion and
    one draw per update, the device cycle, and the device cycle read after every update leave the same filter."""
    n = 100
    host = _driver_run(pkg, sc, n, device_motion=True, draw_every_update=True)
    assert host.n_lidar > 50 and host.n_resamples >= 1
    assert host.n_gate_closed >= 1, "no update behind a closed gate"
    a = ref.state(host.f)
    for opts in (dict(device_cycle=True), dict(device_cycle=True, sync_every_update=True)):
        dev = _driver_run(pkg, sc, n, **opts)
        print("lidar updates %d, resamplings host %d device %d" % (host.n_lidar, host.n_resamples, dev.n_resamples))
        assert dev.n_lidar == host.n_lidar and dev.n_resamples == host.n_resamples
        ref.assert_same_state(a, ref.state(dev.f))
        dev.f.close()
    assert a["sizes"].max() > 3
    host.f.close()


def _vp_driver(pkg, extra, out_dir=None):
    cmd = [pkg.build_mod.SIM_VP, "-c", os.path.join(ROOT, "tests", "golden", "rbphdslam_VictoriaPark_c4.xml"), "-d", os.path.join(ROOT, "tests", "golden", "vp_extract"),
           "-n", "100", "-s", "3"] + (["-o", out_dir] if out_dir else []) + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
    m = re.search(r"RESULT (lidar=\d+ resamples=(\d+) best=\d+ map=\d+ strong=\d+ pose=\S+) ms_per_update", out.stdout)
    assert m, out.stdout[-800:]
    return m.group(1), int(m.group(2))


@gpu
def test_cpp_driver_device_cycle_writes_the_files_of_its_host_stop_route(pkg, tmp_path):
    """rbphdslam_vp --device-cycle against the same driver's host-stop route of that realisation (--draw-every-update: one drand48()
    per update with measurements, every decision on the host): the same particlePose.dat, landmarkEst.dat and finalMap.dat (17
    digits) and the same RESULT line; and --device-cycle without log files, which reads nothing before the end, prints it too.
    (The driver's default route draws only when a resampling fires and normalises inside the step's post kernel: another
    realisation, which --device-cycle is not held to.)"""
    pkg.build_mod.build_host()
    res, dirs = [], []
    for name, extra in (("host", ["--draw-every-update"]), ("cycle", ["--device-cycle"])):
        d = os.path.join(tmp_path, name)
        os.makedirs(d)
        dirs.append(d)
        res.append(_vp_driver(pkg, extra, d))
    assert res[0] == res[1] and res[0][1] >= 1
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and {"particlePose.dat", "landmarkEst.dat", "finalMap.dat"} <= set(names)
    for nm in names:
        assert open(os.path.join(dirs[0], nm), "rb").read() == open(os.path.join(dirs[1], nm), "rb").read(), nm
    assert _vp_driver(pkg, ["--device-cycle"]) == res[0]
