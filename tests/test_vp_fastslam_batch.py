"""A batch of Victoria Park single-hypothesis FastSLAM filters (rfsgpu_batch_vp_serve_fastslam, rfsgpu_batch_vp_fastslam_cycle_async;
include/rfsgpu.h [batch]).  The reference result is the Victoria Park FastSLAM handle, which tests/test_gpu_parity.py holds to the
oracle: filter b of a batch must give the bits its own handle gives through predict_map(False) / fastslam_update on the same inputs --
mixture sizes, every Gaussian plane, the landmark candidate lists (means, covariances, support and check counts), unused masks and
particle ids exactly, unnormalised weights exactly, normalised weights to rtol 1e-12 (each filter's sum has its own workgroup: the
bound tests/test_vp_filter_batch.py uses for the same summation order)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import vp_batch_loop_reference as ref
from test_vp_filter_batch import _driver_filters, _filter_params, _sets

gpu = pytest.mark.gpu
VP_FS_SYMBOLS = {
    "rfsgpu_batch_vp_serve_fastslam": ["rfsgpu_filter *f", "int on"],
    "rfsgpu_batch_vp_fastslam_cycle_async": ["rfsgpu_filter *f", "int predict", "const double *x", "const double *x_cov", "int cov_stride", "const double *z",
                                             "const int *n_z", "const double *scan", "int n_scan", "int normalize"],
}
CAP = 256
GEOM = (0.76, 2.83, 3.78, 0.50)
VAR = np.array([4.0, 0.5])
COUNT_THR = [1, 2, 4]        # landmarkCandidateMeasurementCountThreshold per filter
CHECK_THR = 3


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_calls_with_the_headers_argument_lists(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    for s, args in VP_FS_SYMBOLS.items():
        assert hasattr(lib, s), s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
        m = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, s
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args, s


def test_header_declares_the_calls_outside_the_stable_core():
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    sec = txt.index("[batch]")
    for s in VP_FS_SYMBOLS:
        assert s not in core, s
        assert txt.index(s + "(") > sec, s


def test_null_handle_is_an_error_not_a_crash(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    lib.rfsgpu_batch_vp_serve_fastslam.restype = C.c_int
    lib.rfsgpu_batch_vp_fastslam_cycle_async.restype = C.c_int
    assert lib.rfsgpu_batch_vp_serve_fastslam(None, C.c_int(1)) == pkg.capi.ERR_INVALID
    assert lib.rfsgpu_batch_vp_fastslam_cycle_async(None, C.c_int(0), None, None, C.c_int(0), None, None, None, C.c_int(0), C.c_int(1)) == pkg.capi.ERR_INVALID


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _fs_config(f, b):
    cfg = f.default_fastslam_config()
    cfg.landmarkCandidateMeasurementCountThreshold = COUNT_THR[b % 3]
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementCheckThreshold = CHECK_THR
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    cfg.mapExistencePruneThreshold = -5.0
    cfg.pruningMeasurementsThreshold = 2 if b == 0 else 0      # (filter 0's set of one measurement does not prune)
    return cfg


class _Pair:
    """A VPFastSLAMBatch and one Victoria Park FastSLAM handle per filter, loaded with the same state.  The filters differ in Pd table
    and expected clutter (test_vp_filter_batch._filter_params) and in their candidate count thresholds (1, 2, 4)."""

    def __init__(self, pkg, nF, nPer, cap=CAP, n_landmarks=12, seed0=900):
        sc = pkg.scenarios
        self.pkg, self.nF, self.nPer = pkg, nF, nPer
        self.scens = [sc.make_vp_scenario(nPer, n_landmarks, 6, seed=seed0 + b, params=_filter_params(sc, b)) for b in range(nF)]
        self.batch = pkg.VPFastSLAMBatch(nF, nPer, gm_capacity=cap)
        self.handles = [pkg.FastSLAM(nPer, gm_capacity=cap, model=pkg.capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
        for b, (h, scen) in enumerate(zip(self.handles, self.scens)):
            sc.load_scenario(h, scen)
            h.set_fastslam_config(_fs_config(h, b))
            sc.apply_vp_batch_params(self.batch, b, scen["params"])
            self.batch.configure_fastslam(b, _fs_config(self.batch, b))
            for i in range(nPer):
                self.batch.import_gm(b * nPer + i, scen["w"][i], scen["mean"][i], scen["cov"][i])
        self.batch.set_laser_scan(self.scens[0]["scan"])
        self.poses = np.concatenate([s["poses"] for s in self.scens], 0)
        self.batch.set_poses(self.poses, np.zeros((3, 3)))
        self.batch.set_weights(np.ones(nF * nPer))
        self.q = np.asarray(self.scens[0]["params"]["Q_lm"], dtype=np.float64)[None]

    def cycle(self, Zs, predict=True, poses=None, scan=None, normalize=True):
        """predict True: the static step runs inside the cycle; None: rfsgpu_static_steps_async in front of a cycle without predict."""
        if predict is None:
            self.batch.static_steps_async(1, self.q)
        self.batch.cycle_async(predict, Zs, poses=poses, scan=scan, normalize=normalize)
        for b, h in enumerate(self.handles):
            if scan is not None:
                h.set_laser_scan(scan)
            if poses is not None:
                h.set_poses(poses[b * self.nPer:(b + 1) * self.nPer], np.zeros((3, 3)))
            h.predict_map(False)
            if len(Zs[b]):
                h.fastslam_update(Zs[b])
                if normalize:
                    h.normalize_weights(h.weight_sums()[0])

    def resample(self, plans):
        glob = np.arange(self.nF * self.nPer, dtype=np.int32)
        flags = np.zeros(self.nF, dtype=np.uint8)
        for b, p in plans.items():
            glob[b * self.nPer:(b + 1) * self.nPer] = b * self.nPer + np.asarray(p)
            flags[b] = 1
            self.handles[b].resample_apply(np.asarray(p, dtype=np.int32))
        self.batch.batch_resample_apply(glob, flags)

    def candidates(self, b):
        return [tuple(map(tuple, np.stack(self.handles[b].export_birth_candidates(i)[2:4], 1))) for i in range(self.nPer)]

    def compare(self, what, exact_weights=False):
        batch, nP = self.batch, self.nPer
        batch.synchronize()
        sizes, wb, masks = batch.gm_sizes(), batch.get_weights(), batch.get_unused_masks()
        ids, par = batch.get_particle_ids()
        for b, h in enumerate(self.handles):
            h.synchronize()
            blk = slice(b * nP, (b + 1) * nP)
            np.testing.assert_array_equal(sizes[blk], h.gm_sizes(), err_msg=f"{what} filter {b}: mixture sizes")
            np.testing.assert_array_equal(masks[blk], h.get_unused_masks(), err_msg=f"{what} filter {b}: unused masks")
            hid, hpar = h.get_particle_ids()
            np.testing.assert_array_equal(ids[blk] - b * nP, hid, err_msg=f"{what} filter {b}: ids")
            np.testing.assert_array_equal(par[blk] - b * nP, hpar, err_msg=f"{what} filter {b}: parent ids")
            if exact_weights:
                np.testing.assert_array_equal(ref._bits(wb[blk]), ref._bits(h.get_weights()), err_msg=f"{what} filter {b}: weights")
            else:
                np.testing.assert_allclose(wb[blk], h.get_weights(), rtol=1e-12, atol=0, err_msg=f"{what} filter {b}: weights")
            for i in range(nP):
                for x, y in zip(batch.export_gm(b * nP + i), h.export_gm(i)):
                    np.testing.assert_array_equal(ref._bits(x), ref._bits(y), err_msg=f"{what} filter {b} particle {i}: mixture")
                for x, y in zip(batch.export_birth_candidates(b * nP + i), h.export_birth_candidates(i)):
                    np.testing.assert_array_equal(x, y, err_msg=f"{what} filter {b} particle {i}: candidate list")

    def close(self):
        self.batch.close()
        for h in self.handles:
            h.close()


def _list_events(before, after, count_thr, ev):
    """What one update did to a slot's candidate list, from its (support, checks) pairs before and after.  The list keeps its order:
    a survivor has more checks (one per unassociated measurement of the update) and at least its support, new candidates stand at the
    end.  A candidate that left was promoted when its support could have reached the count threshold (one measurement supports a
    candidate once per walk step, so by at most the number of checks it gained -- bounded here by one supporting measurement per
    update, which is what the planted clutter gives), else it expired at the check threshold."""
    j = 0
    for sup, chk in before:
        if j < len(after) and after[j][1] > chk and after[j][0] >= sup:
            ev["supported"] += int(after[j][0] > sup)
            j += 1
        elif sup + 1 >= count_thr:
            ev["promoted"] += 1
        else:
            ev["expired"] += 1
    ev["created"] += len(after) - j


def _run_shapes(pkg, predict, cap=CAP, n_cycles=8):
    """3 filters x 5 particles (slots 4|5 and 9|10 share a two-wave workgroup across filters), eight cycles compared after each.
    Returns the candidate events seen on the handles' lists, the particles per workgroup of every cycle and the LDS of the last."""
    nPer = 5
    p = _Pair(pkg, 3, nPer, cap=cap)
    sets = _sets(p.scens, n_cycles, seed=5)
    ev = dict(created=0, supported=0, promoted=0, expired=0)
    rng = np.random.default_rng(77)
    sizes, wpb = set(), set()
    for c in range(n_cycles):
        before = [p.candidates(b) for b in range(3)]
        poses = p.poses + rng.normal(0, 0.004, p.poses.shape) if c == 3 else None     # (one cycle hands new poses over)
        normalize = c % 2 == 0                                                        # (odd cycles: the unnormalised weights, bit for bit)
        p.cycle(sets[c], predict=predict, poses=poses, normalize=normalize)
        wpb.add(p.batch.last_step_variant()[2])
        p.compare(f"cycle {c}", exact_weights=not normalize)
        # both sides start the next cycle from the same weights, bit for bit (a normalised cycle leaves them equal to 1e-12 only: the
        # batch sums each filter in its own workgroup), so that the unnormalised weights of the next cycle can be compared exactly
        w = p.batch.get_weights()
        for b, h in enumerate(p.handles):
            blk = slice(b * nPer, (b + 1) * nPer)
            if not normalize:
                w[blk] = w[blk] / w[blk].sum()
            h.set_weights(w[blk])
        p.batch.set_weights(w)
        for b in range(3):
            sizes.add(len(sets[c][b]))
            for i in range(nPer):
                _list_events(before[b][i], p.candidates(b)[i], COUNT_THR[b], ev)
    assert {0, 1, 64} <= sizes
    lds = p.batch.last_cycle_lds()
    p.close()
    return ev, wpb, lds


@gpu
@pytest.mark.parametrize("predict", [True, None])
def test_smallest_shapes_equal_the_handles(pkg, predict):
    """predict True: the static step at the head of the associate kernel; None: RFSGPU_CYCLE_NO_PREDICT behind rfsgpu_static_steps_async."""
    ev, wpb, lds = _run_shapes(pkg, predict)
    for k, v in ev.items():
        assert v > 0, f"no candidate was {k} in the whole run: {ev}"
    assert wpb == {2}, wpb
    assert 0 < lds <= 64 * 1024


@gpu
def test_one_particle_per_workgroup_form(pkg):
    """gm_capacity 512: two waves' areas and Pd scratch do not fit in 64 KiB, fs_associate_update_batch_kernel<1, 3> runs."""
    ev, wpb, lds = _run_shapes(pkg, True, cap=512)
    assert wpb == {1}, wpb
    assert 0 < lds <= 64 * 1024
    for k, v in ev.items():
        assert v > 0, f"no candidate was {k} in the whole run: {ev}"


@gpu
def test_candidates_travel_with_a_host_stop_resampling(pkg):
    nPer = 6
    p = _Pair(pkg, 3, nPer)
    sets = _sets(p.scens, 4, seed=21, nz_max_at=(9, 9))
    for c in range(2):      # (clutter A and B of cycle 1 leave candidates in the filters whose count threshold is above 1)
        p.cycle(sets[c])
    p.compare("before the resampling")
    lens = [[len(c) for c in p.candidates(b)] for b in range(3)]
    assert max(lens[2]) > 0 and max(lens[1]) > 0, lens
    # make the lists of filter 2's slots differ, so that a copy is visible: slot 1 gets one more candidate of its own, far from everything
    m1, c1, s1, k1 = p.handles[2].export_birth_candidates(1)
    own = (np.concatenate([m1, [[-400.0, 650.0, 1.0]]], 0), np.concatenate([c1, np.diag([0.5, 0.5, 0.01])[None]], 0), np.append(s1, 1).astype(np.int32),
           np.append(k1, 0).astype(np.int32))
    p.handles[2].import_birth_candidates(1, *own)
    p.batch.import_birth_candidates(2 * nPer + 1, *own)
    moved = len(own[2])
    assert moved > 0
    # filters 0 and 2: slot 1 (holding a list in filter 2) is duplicated into slot 4, slot 4's own list is dropped; filter 1 is left alone
    p.resample({0: [0, 1, 2, 3, 1, 5], 2: [0, 1, 2, 3, 1, 5]})
    np.testing.assert_array_equal(p.batch.batch_resample_occured(), [True, False, True])
    p.compare("after the resampling")
    got = p.batch.export_birth_candidates(2 * nPer + 4)
    assert len(got[2]) == moved and (got[0][-1] == [-400.0, 650.0, 1.0]).all(), "the list did not travel with the particle"
    for c in range(2, 4):
        p.cycle(sets[c])
        p.compare(f"cycle {c}")
    p.close()


@gpu
def test_device_route_equals_the_host_stop_route(pkg):
    sc = pkg.scenarios
    nF, nPer, keys = 3, 5, [11, 0xABCDEF0123456789, 77]
    gates = [(1, 1), (3, 1), (1, 1)]      # filter 0 fires whenever its gates are open, filter 1 behind minUpdatesBeforeResample = 3, filter 2 never
    eff = [(2.0 * nPer, 2.0), (2.0 * nPer, 2.0), (0.0, 0.0)]
    batches = []
    scens = [sc.make_vp_scenario(nPer, 12, 6, seed=900 + b, params=_filter_params(sc, b)) for b in range(nF)]
    poses = np.concatenate([s["poses"] for s in scens], 0)
    for _ in range(2):
        f = pkg.VPFastSLAMBatch(nF, nPer, gm_capacity=CAP)
        for b, scen in enumerate(scens):
            sc.apply_vp_batch_params(f, b, scen["params"])
            cfg = _fs_config(f, b)
            cfg.minUpdatesBeforeResample, cfg.minMeasurementsBeforeResample = gates[b]
            f.configure_fastslam(b, cfg)
            for i in range(nPer):
                f.import_gm(b * nPer + i, scen["w"][i], scen["mean"][i], scen["cov"][i])
        f.set_laser_scan(scens[0]["scan"])
        f.set_poses(poses, np.zeros((3, 3)))
        f.set_weights(np.ones(nF * nPer))
        batches.append(f)
    dev, twin = batches
    for b in range(nF):
        dev.set_motion(b, VAR, GEOM, keys[b])
        dev.set_resampling(b, *eff[b])
    tail = ref.TwinTail(pkg, twin, gates, eff, keys)
    sets = _sets(scens, 5, seed=5, nz_max_at=(9, 9))
    u = np.array([[1.5, 0.02], [2.0, -0.05], [2.5, 0.11]])
    dt = np.array([0.025, 0.03, 0.025])
    noisy = np.array([0, 1, 1], dtype=np.uint8)
    q = np.asarray(scens[0]["params"]["Q_lm"], dtype=np.float64)[None]
    seen = dict(held=0, fired=np.zeros(nF, dtype=int), lists=0)
    for c in range(5):
        n_z = np.array([len(z) for z in sets[c]])
        for f in (dev, twin):
            f.static_steps_async(1, q)
        dev.propagate_run_async(u[:2 + c % 2], dt[:2 + c % 2], 10 * c, noisy=noisy[:2 + c % 2])
        twin.set_poses(dev.get_poses(), np.zeros((3, 3)))
        dev.cycle_async(None, sets[c], normalize=True)
        twin.cycle_async(None, sets[c], normalize=True)
        seen["lists"] += int(sum(len(twin.export_birth_candidates(i)[2]) for i in range(twin.n)) > 0)
        dev.resample_async(n_z, c)
        fired_t, plan_t, neff_t = tail(n_z, c)
        fired, plan, neff = dev.last_resample()
        np.testing.assert_array_equal(fired, fired_t, err_msg=f"cycle {c}: fired")
        np.testing.assert_array_equal(plan, plan_t, err_msg=f"cycle {c}: plans")
        np.testing.assert_array_equal(ref._bits(neff), ref._bits(neff_t), err_msg=f"cycle {c}: N_eff")
        ref.assert_same_state(ref.state(dev), ref.state(twin), f"cycle {c}, after the tail")
        seen["held"] += int(tail.held[1])
        seen["fired"] += fired
    assert seen["held"] > 0, "the gates never closed"
    assert seen["fired"][0] > 0 and seen["fired"][2] == 0, seen["fired"]
    assert seen["lists"] > 0, "no candidate list was alive at any resampling"
    np.testing.assert_array_equal(dev.loop_counts()[0], seen["fired"])
    dev.close(); twin.close()


@gpu
def test_batch_of_one_is_bit_identical_to_a_plain_handle(pkg):
    p = _Pair(pkg, 1, 7)
    sets = _sets(p.scens, 5, seed=3, nz_max_at=(9, 9))
    for c in range(5):
        p.cycle(sets[c], normalize=False)
        p.compare(f"cycle {c}", exact_weights=True)
    p.close()


@gpu
def test_one_filter_against_the_cpu_oracle(pkg, ob, sc):
    """The D = 3 batch instantiation tied to the oracle directly: one update at the tolerances of test_fastslam_victoria_park_model."""
    from test_gpu_parity import _compare_fastslam
    kw = dict(n_particles=10, n_landmarks=30, n_z=9, seed=91, scan="const")
    scen = sc.make_vp_scenario(**kw)
    n = scen["n"]
    batch = pkg.VPFastSLAMBatch(1, n, gm_capacity=192)
    orc = ob.OracleFilter(n, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    sc.load_scenario(orc, scen)
    sc.apply_vp_batch_params(batch, 0, scen["params"])
    batch.set_laser_scan(scen["scan"])
    batch.set_poses(scen["poses"], scen["pose_cov"])
    batch.set_weights(scen["particle_w"])
    for f in (batch, orc):
        for i in range(n):
            f.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
        cfg = f.default_fastslam_config()
        cfg.landmarkCandidateMeasurementCountThreshold = 2
        cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
        cfg.landmarkCandidateMeasurementCheckThreshold = 3
        cfg.landmarkCandidateMeasurementSupportDist = 3.0
        cfg.mapExistencePruneThreshold = -5.0
        if f is batch:
            f.configure_fastslam(0, cfg)
        else:
            f.set_fastslam_config(cfg)
    batch.cycle_async(True, [scen["Z"]], normalize=False)
    orc.predict_map(False)
    orc.fastslam_update(scen["Z"])
    batch.synchronize()
    _compare_fastslam(sc, batch, orc, n)
    assert sum(batch.landmarks_in_fov(i) for i in range(n)) > 0
    batch.close()


def _state(batch):
    batch.synchronize()
    return batch.get_weights(), batch.gm_sizes(), batch.get_unused_masks()


@gpu
def test_refusals_leave_the_state_untouched(pkg):
    capi = pkg.capi
    lib = pkg.load_library()
    lib.rfsgpu_last_error.restype = C.c_char_p
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    z3 = np.zeros((3, capi.MAX_Z, 3))
    z2 = np.zeros((3, capi.MAX_Z, 2))
    nz = np.array([1, 1, 1], dtype=np.int32)
    t = np.zeros(3)

    def refused(batch, name, args, code=capi.ERR_UNSUPPORTED):
        fn = getattr(lib, "rfsgpu_" + name)
        fn.restype = C.c_int
        assert fn(batch._h, *args) == code, name
        msg = lib.rfsgpu_last_error(batch._h)
        assert len(msg) > 20, name
        return msg

    # the switch off: a batch of Victoria Park filters refuses the FastSLAM calls and the new cycle, as it was published
    sc = pkg.scenarios
    from test_vp_filter_batch import _Pair as _RbPair
    r = _RbPair(pkg, 3, 5)
    rsets = _sets(r.scens, 2, seed=11, nz_max_at=(9, 9))
    fs = r.batch.default_fastslam_config()
    state = _state(r.batch)
    refused(r.batch, "batch_set_fastslam_config", (C.c_int(-1), C.byref(fs)))
    refused(r.batch, "batch_fastslam_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z2), vp(nz), C.c_int(1)))
    refused(r.batch, "batch_vp_fastslam_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1)))
    # ... and once an RB-PHD cycle has run the switch refuses: a batch is of one kind
    r.cycle(rsets[0])
    state = _state(r.batch)
    assert b"one kind" in refused(r.batch, "batch_vp_serve_fastslam", (C.c_int(1),))
    for x, y in zip(state, _state(r.batch)):
        np.testing.assert_array_equal(x, y)
    r.cycle(rsets[1])
    r.compare("the RB-PHD batch after the refusals")
    r.close()
    # not a batch of Victoria Park filters
    flat = pkg.FilterBatch(2, 4, gm_capacity=64)
    refused(flat, "batch_vp_serve_fastslam", (C.c_int(1),))
    refused(flat, "batch_vp_fastslam_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1)))
    flat.close()
    one = pkg.RBPHDFilter(4, gm_capacity=64, model=capi.MODEL_VICTORIAPARK_3D)
    refused(one, "batch_vp_serve_fastslam", (C.c_int(1),))
    refused(one, "batch_vp_fastslam_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1)))
    one.close()

    # the switch on
    p = _Pair(pkg, 3, 5)
    sets = _sets(p.scens, 2, seed=11, nz_max_at=(9, 9))
    p.cycle(sets[0])
    batch = p.batch
    state = _state(batch)
    two = batch.default_fastslam_config()
    two.maxNDataAssocHypotheses = 2
    assert b"filter 1" in refused(batch, "batch_set_fastslam_config", (C.c_int(1), C.byref(two)))
    refused(batch, "batch_vp_cycle_async", (C.c_int(1), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1)))
    refused(batch, "batch_fastslam_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z2), vp(nz), C.c_int(1)))
    refused(batch, "batch_vp_serve_estimates", (C.c_int(1),))
    refused(batch, "estimate_log_create", (C.c_int(4), C.c_int(8), C.c_int(0)))
    refused(batch, "error_log_create", (C.c_int(4),))
    refused(batch, "step_error_async", (vp(t), None, C.c_double(0.75), C.c_double(0.2), C.c_double(1.0)))
    refused(batch, "batch_sense_async", (vp(np.zeros((3, 3))), C.c_ulonglong(0)))
    refused(batch, "batch_fastslam_serve_sensor", (C.c_int(1),))
    refused(batch, "batch_generate_truth", (C.c_int(4),))
    refused(batch, "batch_resample_async", (vp(nz), C.c_ulonglong(0)))
    refused(batch, "batch_fastslam_mh_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z2), vp(nz), vp(t)))
    refused(batch, "batch_vp_serve_fastslam", (C.c_int(0),))        # a FastSLAM cycle has run
    # argument errors follow the other batch cycles
    many = np.array([1, capi.MAX_Z + 1, 0], dtype=np.int32)
    cyc = "batch_vp_fastslam_cycle_async"
    assert b"filter 1" in refused(batch, cyc, (C.c_int(1), None, None, C.c_int(0), vp(z3), vp(many), None, C.c_int(0), C.c_int(1)), capi.ERR_INVALID)
    assert b"null measurement buffer" in refused(batch, cyc, (C.c_int(1), None, None, C.c_int(0), None, vp(nz), None, C.c_int(0), C.c_int(1)), capi.ERR_INVALID)
    assert b"null measurement counts" in refused(batch, cyc, (C.c_int(1), None, None, C.c_int(0), vp(z3), None, None, C.c_int(0), C.c_int(1)), capi.ERR_INVALID)
    assert b"predict" in refused(batch, cyc, (C.c_int(2), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1)), capi.ERR_INVALID)
    assert b"scan" in refused(batch, cyc, (C.c_int(1), None, None, C.c_int(0), vp(z3), vp(nz), vp(np.ones(4)), C.c_int(1), C.c_int(1)), capi.ERR_INVALID)
    for x, y in zip(state, _state(batch)):
        np.testing.assert_array_equal(x, y)
    # a 2-D FastSLAM batch keeps refusing count thresholds other than 1
    flat = pkg.FastSLAMBatch(2, 4, gm_capacity=64)
    four = flat.default_fastslam_config()
    four.landmarkCandidateMeasurementCountThreshold = 4
    refused(flat, "batch_set_fastslam_config", (C.c_int(-1), C.byref(four)))
    flat.close()
    # ... and the batch still steps with its handles
    p.cycle(sets[1], scan=np.full(361, 65.0))              # (the call's own scan: every filter's clutter density follows it)
    p.compare("after the refusals")
    p.close()


@gpu
def test_capacity_overflow_names_the_filter(pkg):
    """Filter 1 only stands at gm_capacity, with landmarks out of range; a measurement nothing takes asks for a new landmark (count
    threshold 1: at once)."""
    sc, capi = pkg.scenarios, pkg.capi
    nF, nPer, cap = 3, 4, 64
    batch = pkg.VPFastSLAMBatch(nF, nPer, gm_capacity=cap)
    scens = [sc.make_vp_scenario(nPer, 10, 8, seed=40 + b, frac_in_fov=1.0) for b in range(nF)]
    far = np.stack([np.linspace(200.0, 900.0, cap), np.full(cap, -300.0), np.full(cap, 1.0)], 1)
    for b, scen in enumerate(scens):
        sc.apply_vp_batch_params(batch, b, scen["params"])
        for i in range(nPer):
            if b == 1:
                batch.import_gm(b * nPer + i, np.full(cap, 2.0), far, np.tile(np.diag([0.5, 0.5, 0.01]), (cap, 1, 1)))
            else:
                batch.import_gm(b * nPer + i, scen["w"][i], scen["mean"][i], scen["cov"][i])
    batch.set_laser_scan(scens[0]["scan"])
    batch.set_poses(np.concatenate([s["poses"] for s in scens], 0), np.zeros((3, 3)))
    batch.cycle_async(None, [s["Z"] for s in scens])
    with pytest.raises(capi.EngineError) as e:
        batch.synchronize()
    assert e.value.status == capi.ERR_CAPACITY and "filter 1" in str(e.value), str(e.value)
    sizes = batch.gm_sizes().reshape(nF, nPer)
    assert (sizes[1] == cap).all() and (sizes[0] < cap).all() and (sizes[2] < cap).all()
    batch.close()


@gpu
def test_driver_batch_run_equals_the_handles_in_turn(pkg):
    """VictoriaParkBatchRun(filter="fastslam") over the first messages of the dataset extract, 3 filters x 20 particles with their own
    seeds, clutter rates and parameter sets, against the same realisations through three FastSLAM handles: every lidar message's
    counts, decisions and plans, and the states at the end.  Both routes."""
    sc, drv, capi = pkg.scenarios, pkg.vp_driver, pkg.capi
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    nF, n, cap, n_msgs = 3, 20, 256, 400
    Ps, seeds, clutter = _driver_filters(sc, nF)

    def fs_cfg(f, b):
        cfg = f.default_fastslam_config()
        cfg.landmarkCandidateMeasurementCountThreshold = 4      # the reference's Victoria Park FastSLAM configuration
        cfg.landmarkCandidateMeasurementCheckThreshold = 6
        cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
        cfg.landmarkCandidateMeasurementSupportDist = 3.0
        cfg.minUpdatesBeforeResample = int(Ps[b]["min_updates"])
        cfg.minMeasurementsBeforeResample = int(Ps[b]["min_measurements"])
        return cfg

    for device_loop in (False, True):
        batch = pkg.VPFastSLAMBatch(nF, n, gm_capacity=cap)
        handles = [pkg.FastSLAM(n, gm_capacity=cap, model=capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
        for b in range(nF):
            sc.apply_vp_batch_params(batch, b, Ps[b])
            batch.configure_fastslam(b, fs_cfg(batch, b))
            sc.apply_vp_params(handles[b], Ps[b], np.full(361, 70.0))
            handles[b].set_fastslam_config(fs_cfg(handles[b], b))
        kw = dict(added_clutter=clutter, keep_history=True, device_loop=device_loop, filter="fastslam")
        rh = drv.VictoriaParkBatchRun(handles, data, Ps, seeds, **kw).run(n_msgs)
        assert rh.n_resamples.sum() > 0, "no resampling fired on the handles: the run is too short"
        rb = drv.VictoriaParkBatchRun(batch, data, Ps, seeds, **kw).run(n_msgs)
        assert rb.n_lidar == rh.n_lidar > 5 and len(rb.history) == len(rh.history) == rb.n_lidar
        for k, ((nzb, fb, pb), (nzh, fh, ph)) in enumerate(zip(rb.history, rh.history)):
            np.testing.assert_array_equal(nzb, nzh, err_msg=f"lidar message {k}: counts")
            np.testing.assert_array_equal(fb, fh, err_msg=f"lidar message {k}: resampling decisions")
            for b in range(nF):
                np.testing.assert_array_equal(pb[b], ph[b], err_msg=f"lidar message {k} filter {b}: plan")
        np.testing.assert_array_equal(rb.x, rh.x)
        sizes, w, masks = batch.gm_sizes(), batch.get_weights(), batch.get_unused_masks()
        for b, h in enumerate(handles):
            blk = slice(b * n, (b + 1) * n)
            np.testing.assert_array_equal(sizes[blk], h.gm_sizes())
            np.testing.assert_array_equal(masks[blk], h.get_unused_masks())
            np.testing.assert_allclose(w[blk], h.get_weights(), rtol=1e-12, atol=0)
            for i in range(n):
                for x, y in zip(batch.export_gm(b * n + i), h.export_gm(i)):
                    np.testing.assert_array_equal(x, y, err_msg=f"filter {b} particle {i}: mixture")
                for x, y in zip(batch.export_birth_candidates(b * n + i), h.export_birth_candidates(i)):
                    np.testing.assert_array_equal(x, y, err_msg=f"filter {b} particle {i}: candidate list")
        batch.close()
        for h in handles:
            h.close()
