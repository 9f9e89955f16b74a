"""The device route of a batch of Victoria Park RB-PHD filters (include/rfsgpu.h [batch]: rfsgpu_batch_vp_set_motion,
_vp_set_resampling, _vp_propagate_run_async, _vp_resample_async, _vp_last_resample, _vp_loop_counts; csrc/vp_batch_loop.h).  The
propagation is held to a plain Victoria Park handle under rfsgpu_propagate_ackerman_run_async; everything else to a host-stop twin
(tests/support/vp_batch_loop_reference.py): a second batch on the unchanged host-stop route that receives the device route's poses and
resamples by the restated rule.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import vp_batch_loop_reference as ref
from test_vp_filter_batch import _filter_params, _sets

gpu = pytest.mark.gpu
VP_LOOP_SYMBOLS = ["rfsgpu_batch_vp_set_motion", "rfsgpu_batch_vp_set_resampling", "rfsgpu_batch_vp_propagate_run_async", "rfsgpu_batch_vp_resample_async",
                   "rfsgpu_batch_vp_last_resample", "rfsgpu_batch_vp_loop_counts"]
GEOM = (0.76, 2.83, 3.78, 0.50)
VAR = np.array([4.0, 0.5])


def _walk_levels():
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    return int(re.search(r"#define\s+RFSGPU_RBPHD_WALK_LEVELS\s+(\d+)", txt).group(1))


def _run_max():
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    return int(re.search(r"#define\s+RFSGPU_BATCH_VP_RUN_MAX\s+(\d+)", txt).group(1))


def _empty(nF):
    return [np.zeros((0, 3))] * nF


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_vp_device_route_and_the_library_exports_it(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    sec = txt.index("[batch]")
    for s in VP_LOOP_SYMBOLS:
        assert s not in core, s
        assert txt.index(s + "(") > sec, s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    assert _run_max() >= 16
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in VP_LOOP_SYMBOLS:
        assert hasattr(lib, s), s


def test_driver_restates_the_resampling_draw(pkg):
    from tests.support import device_loop_reference as dl
    rng = np.random.default_rng(3)
    for _ in range(50):
        seed, call = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
        assert pkg.vp_driver.philox_resample_draw(seed, call) == dl.resample_draw(seed, call)


# ---- 1. propagation ----------------------------------------------------------------------------------------------------------

def _run_inputs():
    u = np.array([[1.5, 0.02], [2.0, -0.05], [2.5, 0.11], [2.2, -0.2], [1.1, 0.07]])
    dt = np.array([0.025, 0.03, 0.025, 0.021, 0.04])
    noisy = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    return u, dt, noisy


@gpu
@pytest.mark.parametrize("nPer", [1, 65, 257])
def test_propagation_equals_a_handle_per_filter(pkg, nPer):
    capi = pkg.capi
    nF = 3
    keys = [5, 0x1234567890ABCDEF, 2 ** 64 - 3]
    rng = np.random.default_rng(41 + nPer)
    x0 = np.column_stack([rng.uniform(-40, 40, nF * nPer), rng.uniform(-40, 40, nF * nPer), rng.uniform(-3.1, 3.1, nF * nPer)])
    u, dt, noisy = _run_inputs()
    batch = pkg.VPFilterBatch(nF, nPer, gm_capacity=32)
    batch.set_poses(x0, None)
    covs = batch.get_pose_covs()
    for b in range(nF):
        batch.set_motion(b, VAR, GEOM, keys[b])
    handles = [pkg.RBPHDFilter(nPer, gm_capacity=32, model=capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
    for b, h in enumerate(handles):
        h.set_poses(x0[batch.block(b)], None)
    var = noisy[:, None] * VAR[None, :]
    for call0 in (7, 12):                                   # the second call continues the first
        batch.propagate_run_async(u, dt, call0, noisy=noisy)
        got = batch.get_poses()
        for b, h in enumerate(handles):
            h.propagate_ackerman_run_async(u, var, dt, GEOM, keys[b], call0)
            np.testing.assert_array_equal(ref._bits(got[batch.block(b)]), ref._bits(h.get_poses()), err_msg=f"call0 {call0} filter {b}")
    if nPer > 1:
        assert np.abs(got[batch.block(0)] - got[batch.block(1)] - (x0[batch.block(0)] - x0[batch.block(1)])).max() > 1e-3, "the keys draw alike"
    np.testing.assert_array_equal(batch.get_pose_covs(), covs)                 # the pose covariances are left as they are
    # a filter's poses do not depend on its place in the batch
    other = pkg.VPFilterBatch(nF, nPer, gm_capacity=32)
    perm = [2, 0, 1]
    other.set_poses(np.concatenate([x0[batch.block(p)] for p in perm], 0), None)
    for b, p in enumerate(perm):
        other.set_motion(b, VAR, GEOM, keys[p])
    for call0 in (7, 12):
        other.propagate_run_async(u, dt, call0, noisy=noisy)
    po = other.get_poses()
    for b, p in enumerate(perm):
        np.testing.assert_array_equal(ref._bits(po[other.block(b)]), ref._bits(got[batch.block(p)]), err_msg=f"filter {p} at index {b}")
    # a run beyond the documented maximum is refused, the state untouched
    n = _run_max() + 1
    with pytest.raises(capi.EngineError) as e:
        batch.propagate_run_async(np.tile(u[:1], (n, 1)), np.full(n, 0.025), 20)
    assert e.value.status == capi.ERR_INVALID and "RFSGPU_BATCH_VP_RUN_MAX" in str(e.value)
    np.testing.assert_array_equal(ref._bits(batch.get_poses()), ref._bits(got))
    batch.close(); other.close()
    for h in handles:
        h.close()


# ---- 2. the resampling tail ---------------------------------------------------------------------------------------------------

def _tail_params(sc, nPer):
    """Filter 0 fires whenever its gates are open (eff_n above the particle count), filter 1 the same behind minUpdatesBeforeResample = 3,
    filter 2 never (eff_n 0)."""
    gates = [(1, 1), (3, 1), (1, 1)]
    eff = [(2.0 * nPer, 2.0), (2.0 * nPer, 2.0), (0.0, 0.0)]

    def params_of(b):
        P = _filter_params(sc, b)
        P["min_updates"], P["min_measurements"] = gates[b]
        return P
    return gates, eff, params_of


@gpu
@pytest.mark.parametrize("nPer", [3, 65, 257])
def test_resampling_tail_equals_the_host_stop_twin(pkg, nPer):
    sc = pkg.scenarios
    nF, keys = 3, [11, 0xABCDEF0123456789, 77]
    gates, eff, params_of = _tail_params(sc, nPer)
    scens, (dev, twin) = ref.make_batches(pkg, nF, nPer, params_of)
    for b in range(nF):
        dev.set_motion(b, VAR, GEOM, keys[b])
        dev.set_resampling(b, *eff[b])
    tail = ref.TwinTail(pkg, twin, gates, eff, keys)
    sets = _sets(scens, 4, seed=5, nz_max_at=(9, 9))
    sets[1][2] = np.zeros((0, 3))                            # filter 2 has no measurements in cycle 1
    u, dt, noisy = _run_inputs()
    seen = dict(mixed=0, held=0, empty=0, fired=np.zeros(nF, dtype=int))
    for c in range(4):
        n_z = np.array([len(z) for z in sets[c]])
        # the birth predict of the run, the propagation behind it, the update at the new poses, the tail
        dev.cycle_async(True, _empty(nF), normalize=False)
        twin.cycle_async(True, _empty(nF), normalize=False)
        a, b = ref.state(dev, mixtures=False), ref.state(twin, mixtures=False)
        ref.assert_same_state(a, b, f"cycle {c}, after the birth predict")      # candidate lists and unused masks included
        dev.propagate_run_async(u[:2 + c % 2], dt[:2 + c % 2], 10 * c, noisy=noisy[:2 + c % 2])
        twin.set_poses(dev.get_poses(), np.zeros((3, 3)))
        dev.cycle_async(None, sets[c], normalize=True)
        twin.cycle_async(None, sets[c], normalize=True)
        dev.resample_async(n_z, c)
        fired_t, plan_t, neff_t = tail(n_z, c)
        fired, plan, neff = dev.last_resample()
        np.testing.assert_array_equal(fired, fired_t, err_msg=f"cycle {c}: fired")
        np.testing.assert_array_equal(plan, plan_t, err_msg=f"cycle {c}: plans")
        np.testing.assert_array_equal(ref._bits(neff), ref._bits(neff_t), err_msg=f"cycle {c}: N_eff")
        ref.assert_same_state(ref.state(dev), ref.state(twin), f"cycle {c}, after the tail")
        np.testing.assert_array_equal(dev.batch_resample_occured(), fired | (a["occured"] & (n_z == 0)), err_msg=f"cycle {c}: resampleOccured_")
        seen["mixed"] += int(fired.any() and (~fired & (n_z > 0)).any())
        seen["held"] += int(tail.held[1])
        seen["empty"] += int(n_z[2] == 0)
        seen["fired"] += fired
        seen["copied"] = seen.get("copied", 0) + int((plan != np.arange(nF * nPer)).sum())
    assert seen["copied"] > 0 or nPer < 65, "no slot was copied in any resampling: the gather moved nothing"
    assert seen["mixed"] > 0, "no call in which one filter fired and another, with measurements, did not"
    assert seen["held"] > 0, "minUpdatesBeforeResample held no filter"
    assert seen["empty"] > 0, "no filter without measurements"
    assert seen["fired"][0] > 0 and seen["fired"][1] > 0 and seen["fired"][2] == 0, seen["fired"]
    counts, _ = dev.loop_counts()
    np.testing.assert_array_equal(counts, seen["fired"])
    dev.close(); twin.close()


# ---- 3. a walk deeper than the fixed launches ----------------------------------------------------------------------------------

@gpu
def test_walk_deeper_than_the_fixed_launches(pkg):
    sc = pkg.scenarios
    nF, nPer, keys = 2, 9, [3, 4]
    depth = _walk_levels() + 3
    assert depth == nPer - 2
    gates, eff = [(1, 1), (1, 1)], [(0.0, 0.0), (2.0 * nPer, 2.0)]      # filter 1 fires, filter 0 never

    def params_of(b):
        P = _filter_params(sc, b, cluster_filter=9)
        P["birth_count_thr"], P["birth_check_thr"] = 2, 20      # (a marker candidate survives the checks of the whole chain)
        P["min_updates"], P["min_measurements"] = gates[b]
        return P
    scens, (dev, twin) = ref.make_batches(pkg, nF, nPer, params_of)
    for b in range(nF):
        dev.set_motion(b, VAR, GEOM, keys[b])
        dev.set_resampling(b, *eff[b])
    tail = ref.TwinTail(pkg, twin, gates, eff, keys)
    sets = _sets(scens, 3, seed=21, nz_max_at=(9, 9))
    for c in range(2):
        Zs = sets[c]                                         # (cycle 1 carries two clutter points: unused measurements for the walk's births)
        n_z = np.array([len(z) for z in Zs])
        for f in (dev, twin):
            f.cycle_async(True, Zs, normalize=True)
        dev.resample_async(n_z, c)
        fired_t, _, _ = tail(n_z, c)
        np.testing.assert_array_equal(dev.last_resample()[0], fired_t)
    np.testing.assert_array_equal(fired_t, [False, True])
    np.testing.assert_array_equal(dev.batch_resample_occured(), [False, True])
    # filter 1: the chain 7 -> 6 -> ... -> 0, slot 8 keeps itself; filter 0: the same parents, stale (its flag is clear)
    local = np.array([0, 0, 1, 2, 3, 4, 5, 6, 8])
    parents = np.concatenate([local, nPer + local]).astype(np.int32)
    ids = np.arange(nF * nPer, dtype=np.int32)
    marker = np.array([[-400.0, 650.0, 1.0]])
    for f in (dev, twin):
        f.set_particle_ids(ids, parents)
        for slot in (0, nPer):                               # slot 0 of either filter holds a candidate no other slot has
            m, cv, s, k = f.export_birth_candidates(slot)
            f.import_birth_candidates(slot, np.concatenate([m, marker], 0), np.concatenate([cv, np.diag([0.5, 0.5, 0.01])[None]], 0),
                                      np.append(s, 1).astype(np.int32), np.append(k, 0).astype(np.int32))
    assert dev.get_unused_masks().any(), "no unused measurement: the births of the walk would have nothing to do"
    has_marker = lambda f, slot: bool((f.export_birth_candidates(slot)[0] == marker[0]).all(axis=1).any())
    for f in (dev, twin):
        f.cycle_async(True, _empty(nF), normalize=False)      # the birth predict
    a, b = ref.state(dev), ref.state(twin)
    ref.assert_same_state(a, b, "after the birth predict")
    assert dev.loop_counts()[1] == depth
    assert [has_marker(dev, nPer + i) for i in range(nPer)] == [True] * (nPer - 1) + [False], "filter 1's chain did not carry slot 0's list"
    def marker_checks(slot):
        m, _, _, k = dev.export_birth_candidates(slot)
        return int(k[np.nonzero((m == marker[0]).all(axis=1))[0][0]])
    chk = [marker_checks(nPer + i) for i in range(nPer - 1)]
    assert chk == list(range(1, nPer)), chk                 # the marker is one check older at every link of the chain
    assert [has_marker(dev, i) for i in range(nPer)] == [True] + [False] * (nPer - 1), "filter 0 (flag clear) inherited a list"
    for f in (dev, twin):
        f.cycle_async(None, sets[2], normalize=True)          # the update
    ref.assert_same_state(ref.state(dev), ref.state(twin), "after the update")
    assert not dev.batch_resample_occured().any()            # both filters were updated: the flags have fallen
    assert dev.loop_counts()[1] == depth
    dev.close(); twin.close()


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------

@gpu
def test_driver_device_loop_equals_the_twin_message_by_message(pkg):
    sc, drv = pkg.scenarios, pkg.vp_driver
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    nF, n, cap = 3, 33, 384
    seeds, clutter = [31, 38, 45], [3.0, 1.0, 5.0]
    eff_n = [n + 1.0, n / 2.0, n + 1.0]                     # filters 0 and 2 resample whenever their gates are open
    Ps = []
    for b in range(nF):
        P = dict(sc.VP_PARAMS)
        P["expected_clutter"] = [6.0, 3.0, 9.0][b]
        P["birth_count_thr"], P["birth_check_thr"] = [(5, 10), (2, 4), (3, 6)][b]
        P["min_updates"], P["min_measurements"] = [(2, 15), (3, 15), (2, 30)][b]
        Ps.append(P)
    dev, twin = (pkg.VPFilterBatch(nF, n, gm_capacity=cap) for _ in range(2))
    for f in (dev, twin):
        for b in range(nF):
            sc.apply_vp_batch_params(f, b, Ps[b])
        f.set_laser_scan(np.full(361, 70.0))
    twin.set_poses(np.zeros((nF * n, 3)), None)
    tail = ref.TwinTail(pkg, twin, [(P["min_updates"], P["min_measurements"]) for P in Ps], [(e, e / n) for e in eff_n], seeds)
    log = dict(fired=np.zeros(nF, dtype=int), lidar=0)

    class Run(drv.VictoriaParkBatchRun):
        """The driver, with the twin stepped behind every lidar message from what the driver issued."""

        def _cycle_device(self, q, dts, Zs):
            super()._cycle_device(q, dts, Zs)
            self.issued = (q, Zs, dev.get_poses())           # the poses the update saw: read in front of the tail, which gathers them

        def _resample_device(self, n_z):
            fired, plans = super()._resample_device(n_z)
            q, Zs, poses = self.issued
            k = self.n_lidar - 1
            twin.set_lmk_process_noise(q[0])
            twin.cycle_async(True, _empty(nF), normalize=False)
            if len(q) > 1:
                twin.static_steps_async(len(q) - 1, q[1:])
            twin.set_poses(poses, None)
            twin.cycle_async(None, Zs, scan=self.scan, normalize=True)
            fired_t, plan_t, neff_t = tail(n_z, k)
            _, plan, neff = dev.last_resample()
            np.testing.assert_array_equal(fired, fired_t, err_msg=f"lidar message {k}: fired")
            np.testing.assert_array_equal(plan, plan_t, err_msg=f"lidar message {k}: plans")
            np.testing.assert_array_equal(ref._bits(neff), ref._bits(neff_t), err_msg=f"lidar message {k}: N_eff")
            ref.assert_same_state(ref.state(dev), ref.state(twin), f"lidar message {k}")
            log["fired"] += fired
            log["lidar"] += 1
            return fired, plans

    run = Run(dev, data, Ps, seeds, added_clutter=clutter, eff_n=eff_n, keep_history=True, device_loop=True).run(200)
    assert log["lidar"] == run.n_lidar == len(run.history) == 20
    assert log["fired"].sum() > 0 and log["fired"][0] > 0, log["fired"]      # the twin's decisions are the restated rule's
    np.testing.assert_array_equal(run.n_resamples, log["fired"])
    np.testing.assert_array_equal(ref._bits(run.x), ref._bits(dev.get_poses()))
    assert np.ptp(run.x[:n, 0]) > 0, "the particles of filter 0 never parted: no noisy propagation in the run"
    dev.close(); twin.close()


# ---- 5. route rules -----------------------------------------------------------------------------------------------------------

def _raw_calls(batch_like, nF):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    keep = dict(var=np.ones(2), geom=np.array(GEOM), u=np.array([[1.0, 0.1]]), dt=np.array([0.025]), nz=np.ones(max(nF, 1), dtype=np.int32))
    calls = [("batch_vp_set_motion", (C.c_int(-1), vp(keep["var"]), vp(keep["geom"]), C.c_ulonglong(1))),
             ("batch_vp_set_resampling", (C.c_int(-1), C.c_double(2.0), C.c_double(0.5))),
             ("batch_vp_propagate_run_async", (C.c_int(1), vp(keep["u"]), None, vp(keep["dt"]), C.c_ulonglong(0))),
             ("batch_vp_resample_async", (vp(keep["nz"]), C.c_ulonglong(0))),
             ("batch_vp_last_resample", (None, None, None)),
             ("batch_vp_loop_counts", (None, None))]
    return calls, keep


@gpu
def test_route_rules(pkg):
    sc, capi = pkg.scenarios, pkg.capi
    lib = pkg.load_library()
    lib.rfsgpu_last_error.restype = C.c_char_p
    nF, nPer = 3, 5
    gates, eff = [(1, 1)] * nF, [(2.0 * nPer, 2.0), (0.0, 0.0), (0.0, 0.0)]

    def params_of(b):
        P = _filter_params(sc, b)
        P["min_updates"], P["min_measurements"] = gates[b]
        return P
    scens, (dev, twin) = ref.make_batches(pkg, nF, nPer, params_of)
    sets = _sets(scens, 4, seed=11, nz_max_at=(9, 9))
    u, dt, noisy = _run_inputs()
    nz1 = np.ones(nF, dtype=np.int32)
    # before set_motion / set_resampling the calls name the filter they miss
    with pytest.raises(capi.EngineError) as e:
        dev.propagate_run_async(u, dt, 0)
    assert e.value.status == capi.ERR_INVALID and "filter 0" in str(e.value)
    dev.set_motion(0, VAR, GEOM, 1)
    with pytest.raises(capi.EngineError) as e:
        dev.propagate_run_async(u, dt, 0)
    assert e.value.status == capi.ERR_INVALID and "filter 1" in str(e.value)
    dev.set_motion(None, VAR, GEOM, 1)
    with pytest.raises(capi.EngineError) as e:
        dev.resample_async(nz1, 0)
    assert e.value.status == capi.ERR_INVALID and "filter 0" in str(e.value) and "resampling" in str(e.value)
    dev.set_resampling(0, *eff[0])
    with pytest.raises(capi.EngineError) as e:
        dev.resample_async(nz1, 0)
    assert e.value.status == capi.ERR_INVALID and "filter 1" in str(e.value)
    assert not dev.batch_resample_occured().any()
    dev.batch_resample_apply(np.arange(nF * nPer, dtype=np.int32), np.zeros(nF, dtype=np.uint8))      # still on the host-stop route
    # a 2-D batch and an ordinary handle refuse the section, their state untouched
    flat = pkg.FilterBatch(2, 4, gm_capacity=64)
    plain = pkg.RBPHDFilter(4, gm_capacity=64, model=capi.MODEL_VICTORIAPARK_3D)
    for f, n_f in ((flat, 2), (plain, 1)):
        x = np.random.default_rng(1).uniform(-1, 1, (f.n, 3))
        f.set_poses(x, None)
        f.set_weights(np.linspace(0.5, 1.5, f.n))
        calls, keep = _raw_calls(f, n_f)
        for name, args in calls:
            fn = getattr(lib, "rfsgpu_" + name)
            fn.restype = C.c_int
            assert fn(f._h, *args) == capi.ERR_UNSUPPORTED, name
            assert len(lib.rfsgpu_last_error(f._h)) > 20, name
        f.synchronize()
        np.testing.assert_array_equal(f.get_poses(), x)
        np.testing.assert_array_equal(f.get_weights(), np.linspace(0.5, 1.5, f.n))
        f.close()
    # host-stop route first, device route later: the ids and flags move over.  Two cycles and a resampling of filters 0 and 2 on the
    # host-stop route; filter 0 has no measurements in cycle 2, so its flag still stands when the handle enters the device route
    # behind that cycle, and cycle 3's birth predict walks its levels on the device from the ids that moved
    for c in range(2):
        for f in (dev, twin):
            f.cycle_async(True, sets[c], normalize=True)
    plan = np.arange(nF * nPer, dtype=np.int32)
    plan[0:5] = [1, 1, 2, 3, 2]
    plan[10:15] = 10 + np.array([0, 1, 0, 3, 4])
    for f in (dev, twin):
        f.batch_resample_apply(plan, np.array([1, 0, 1], dtype=np.uint8))
    sets[2][0] = np.zeros((0, 3))
    for b in range(1, nF):
        dev.set_resampling(b, *eff[b])
    tail = ref.TwinTail(pkg, twin, gates, eff, [1] * nF)
    for c in (2, 3):
        n_z = np.array([len(z) for z in sets[c]])
        for f in (dev, twin):
            f.cycle_async(True, sets[c], normalize=True)
        dev.resample_async(n_z, c)
        fired_t, plan_t, _ = tail(n_z, c)
        fired, plan_d, _ = dev.last_resample()
        np.testing.assert_array_equal(fired, fired_t)
        np.testing.assert_array_equal(plan_d, plan_t)
        ref.assert_same_state(ref.state(dev), ref.state(twin), f"cycle {c}")
        if c == 2:
            np.testing.assert_array_equal(dev.batch_resample_occured(), [True, False, False])      # filter 0: the host's flag, on the device now
            assert (ref.state(dev, lists=False, mixtures=False)["par"][0:5] != np.arange(5)).any()
    assert fired_t[0]
    # from the first resample_async on the host-stop route is closed
    with pytest.raises(capi.EngineError) as e:
        dev.batch_resample_apply(np.arange(nF * nPer, dtype=np.int32), np.zeros(nF, dtype=np.uint8))
    assert e.value.status == capi.ERR_UNSUPPORTED
    ref.assert_same_state(ref.state(dev), ref.state(twin), "after the refusal")
    dev.close(); twin.close()
