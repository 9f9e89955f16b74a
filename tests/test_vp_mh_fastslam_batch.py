"""A batch of Victoria Park multi-hypothesis FastSLAM filters (rfsgpu_create_batch_vp_mh, rfsgpu_batch_vp_fastslam_mh_cycle_async;
include/rfsgpu.h).  The yardstick is one Victoria Park FastSLAM handle per filter, created with max_particles = max_per_filter and
stepped by rfsgpu_static_steps_async / rfsgpu_propagate_ackerman_run_async / rfsgpu_fastslam_cycle_full_async on the same poses, sets,
scan and draws (tests/test_fastslam_vp_device_cycle.py holds that handle to the host-stop route and the oracle).  Filter b of the batch
must give its handle's bits: mixtures, counts, landmark candidate lists (means, covariances, support and check counters), unused masks,
in-view counts, poses, ids, parents, plans, live counts and the fired / forced decisions exactly; weights and N_eff to 1e-12 relative,
the bound tests/support/mh_batch_reference.py holds the 2-D batch to (the batch sums each filter in its own tree).

The events a scenario has to show -- growth, an unforced and a forced resampling, candidate lists that travel with the copies and lists
that do not -- are asserted on the HANDLES' fastslam_last_cycle and lists, so a scenario that shows nothing fails.  More than one
hypothesis arises because every map holds pairs of landmarks five centimetres apart: both lie in the window of the pair's measurement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import mh_batch_reference as mb
from tests.support import mh_device_cycle_reference as mh
from tests.support import vp_device_cycle_reference as vref
from test_vp_filter_batch import _filter_params

gpu = pytest.mark.gpu
SYMBOLS = {
    "rfsgpu_create_batch_vp_mh": "rfsgpu_filter **out, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity",
    "rfsgpu_batch_vp_fastslam_mh_cycle_async": "rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, "
                                               "const int *n_z, const double *scan, int n_scan, const double *u01",
}
CAP = 64
N_PER = 4
HYPS = (2, 3, 3)
THRS = (1, 2, 4)             # landmarkCandidateMeasurementCountThreshold per filter
GEOM = (0.76, 2.83, 3.78, 0.50)
VAR = np.array([0.04, 1e-4])
NEVER = mb.NEVER
ALWAYS = 1e9                 # an N_eff threshold no set reaches: the test fires whenever the gates let it run


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_outside_the_stable_core():
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    for s in SYMBOLS:
        assert s not in core, s
        assert txt.index(s + "(") > txt.index("[batch]"), s


def test_library_exports_the_calls_with_the_headers_argument_lists(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    for s, args in SYMBOLS.items():
        assert hasattr(lib, s), s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
        m = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, s
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == [a.strip() for a in args.split(",")], s


def test_null_handle_and_null_out_are_errors_not_crashes(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    lib.rfsgpu_create_batch_vp_mh.restype = C.c_int
    lib.rfsgpu_batch_vp_fastslam_mh_cycle_async.restype = C.c_int
    null = C.c_void_p(None)
    assert lib.rfsgpu_create_batch_vp_mh(null, C.c_int(1), C.c_int(1), C.c_int(1), C.c_int(0), C.c_int(64)) == pkg.capi.ERR_INVALID
    assert lib.rfsgpu_batch_vp_fastslam_mh_cycle_async(null, C.c_int(0), null, null, C.c_int(0), null, null, null, C.c_int(0), null) == pkg.capi.ERR_INVALID
    out = C.c_void_p()       # the argument errors come before any device is touched
    assert lib.rfsgpu_create_batch_vp_mh(C.byref(out), C.c_int(2), C.c_int(8), C.c_int(4), C.c_int(0), C.c_int(64)) == pkg.capi.ERR_INVALID
    assert lib.rfsgpu_create_batch_vp_mh(C.byref(out), C.c_int(2), C.c_int(8), C.c_int(4096), C.c_int(0), C.c_int(64)) == pkg.capi.ERR_UNSUPPORTED
    assert not out.value


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _scenario(sc, b, n_per, seed0=112):
    """Filter b's scene: test_vp_filter_batch's parameter set of the filter, ten landmarks, and the first three of them once more
    five centimetres away (the planted ambiguity)."""
    s = sc.make_vp_scenario(n_per, 10, 8, seed=seed0 + b, scan="const", params=_filter_params(sc, b))
    off = np.array([0.05, -0.05, 0.0])
    s["mean"] = np.concatenate([s["mean"], s["mean"][:, :3] + off], 1)
    s["cov"] = np.concatenate([s["cov"], s["cov"][:, :3]], 1)
    s["w"] = np.concatenate([s["w"], s["w"][:, :3]], 1)
    return s


def _sets(scens, n_cycles, seed, empty=None):
    """Per cycle and filter 2 ... 5 measurements: a rotating choice of the scene's own plus one far return no landmark takes (it feeds
    the candidate lists); empty = (cycle, filter): that set is empty."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_cycles):
        row = []
        for b, s in enumerate(scens):
            k = 1 + (c + b) % 4
            Z = np.roll(s["Z"], -(c + b), 0)[:k] + rng.normal(0, 1e-3, (k, 3))
            far = np.array([[45.0 + 2.0 * ((c + 2 * b) % 3), 0.35 + 0.4 * ((c + b) % 5), 0.9]])
            row.append(np.zeros((0, 3)) if empty == (c, b) else np.concatenate([Z, far], 0))
        out.append(row)
    return out


class _Rig:
    """A VPMHFastSLAMBatch and its handles on the same state.  tune(b, fs_config): the filter's gates."""

    def __init__(self, pkg, sc, nF, stride, tune, n_per=N_PER, cap=CAP, hyps=HYPS, thrs=THRS, check_thr=3):
        self.pkg, self.sc, self.nF, self.n_per, self.stride = pkg, sc, nF, n_per, stride
        self.scens = [_scenario(sc, b, n_per) for b in range(nF)]
        self.batch = pkg.VPMHFastSLAMBatch(nF, n_per, stride, gm_capacity=cap)
        self.handles = []
        x = np.zeros((nF * stride, 3))
        for b, scen in enumerate(self.scens):
            h = pkg.FastSLAM(n_per, gm_capacity=cap, max_hypotheses=hyps[b % 3], device_cycle=True, max_particles=stride,
                             model=pkg.capi.MODEL_VICTORIAPARK_3D)
            sc.load_scenario(h, scen, maps=False)
            h.config = h.get_filter_config()
            vref.candidate_config(h.fs_config, thrs[b % 3], 0)
            h.fs_config.landmarkCandidateMeasurementCheckThreshold = check_thr
            h.fs_config.maxNDataAssocHypotheses = hyps[b % 3]
            h.fs_config.maxDataAssocLogLikelihoodDiff = 50.0
            h.fs_config.pruningMeasurementsThreshold = 3          # (the sets of two measurements do not prune)
            tune(b, h.fs_config)
            h.set_fastslam_config(h.fs_config)
            self.handles.append(h)
            sc.apply_vp_batch_params(self.batch, b, scen["params"])
            self.batch.configure_fastslam(b, mb.copy_struct(h.fs_config))
            x[b * stride:b * stride + n_per] = scen["poses"]
            for i in range(n_per):
                z = np.zeros(scen["w"][i].shape)
                h.import_gm(i, z, scen["mean"][i], scen["cov"][i])
                self.batch.import_gm(b * stride + i, z, scen["mean"][i], scen["cov"][i])
            self.batch.set_motion(b, VAR, GEOM, 40 + b)
        self.scan = self.scens[0]["scan"]
        self.batch.set_laser_scan(self.scan)
        self.batch.set_poses(x, self.scens[0]["pose_cov"])
        self.batch.set_weights(np.ones(nF * stride))
        for h in self.handles:
            h.set_laser_scan(self.scan)
            h.set_weights(np.ones(n_per))
        self.q = np.asarray(self.scens[0]["params"]["Q_lm"], dtype=np.float64).reshape(1, 3, 3)
        self.call = 0
        for b in range(nF):
            self.set_resampling(b, n_per / 4.0, 0.25)

    def set_resampling(self, b, eff_n, eff_n_percent):
        self.handles[b].effNParticles_t, self.handles[b].effNParticles_t_percent = eff_n, eff_n_percent
        self.batch.set_resampling(b, eff_n, eff_n_percent)

    def plant_lists(self, b, k):
        for i in range(self.n_per):
            c = vref_far_candidates(k)
            self.handles[b].import_birth_candidates(i, *c)
            self.batch.import_birth_candidates(b * self.stride + i, *c)

    def cycle(self, Zs, u01, predict=False, scan=None, skip=()):
        self.batch.cycle_async(predict, Zs, u01, scan=scan)
        for b, h in enumerate(self.handles):
            if b not in skip:
                h.cycle_async(Zs[b], u01[b], predict=predict, scan=scan)

    def static_step(self, skip=()):
        self.batch.static_steps_async(1, self.q)
        for b, h in enumerate(self.handles):
            if b not in skip:
                h.static_steps_async(1, self.q)

    def propagate(self, u, dt, skip=()):
        u = np.asarray(u, dtype=np.float64).reshape(-1, 2)
        self.batch.propagate_run_async(u, dt, self.call)
        for b, h in enumerate(self.handles):
            if b not in skip:
                h.propagate_ackerman_run_async(u, np.tile(VAR, (u.shape[0], 1)), dt, GEOM, 40 + b, self.call)
        self.call += u.shape[0]

    def block_state(self, b, n):
        B, s = self.batch, self.stride
        blk = B.block(b, n)
        ids = B.get_particle_ids()
        return dict(n=n, w=B.get_weights()[blk].copy(), poses=B.get_poses()[blk].copy(), sizes=np.asarray(B.gm_sizes())[blk].copy(),
                    fov=np.array([B.landmarks_in_fov(b * s + i) for i in range(n)]), unused=np.asarray(B.get_unused_masks())[blk].copy(),
                    maps=[tuple(np.array(x) for x in B.export_gm(b * s + i)) for i in range(n)],
                    cands=[tuple(np.array(x) for x in B.export_birth_candidates(b * s + i)) for i in range(n)],
                    ids=tuple(np.array(x[blk]) for x in ids))

    def compare(self, what, only=None):
        """Counts, decisions, parents, plans, ids and N_eff through mh_batch_reference's comparison; then every live slot's state."""
        rig = mb.Rig.of(self.pkg, self.sc, self.batch, self.handles, self.n_per, self.stride)
        lc, _ = rig.compare(maps=False, only=only)
        for b, h in enumerate(self.handles):
            if only is not None and b not in only:
                continue
            a, c = vref.state(h), self.block_state(b, h.n)
            mh.assert_same_state(a, c, weights=1e-12)
            for i, (ca, cb) in enumerate(zip(a["cands"], c["cands"])):
                for x, y, k in zip(ca, cb, ("mean", "cov", "support", "check")):
                    assert x.shape == y.shape and np.array_equal(x, y), "%s filter %d particle %d: candidate %s" % (what, b, i, k)
            for x, y in zip(a["ids"], c["ids"]):
                assert np.array_equal(x, y), "%s filter %d: ids" % (what, b)
        return lc

    def list_sizes(self, b):
        h = self.handles[b]
        return [len(h.export_birth_candidates(i)[2]) for i in range(h.n)]

    def close(self):
        self.batch.close()
        for h in self.handles:
            h.close()


def vref_far_candidates(k):
    """k landmark candidates no measurement supports (a kilometre away), young enough not to expire in a test."""
    mean = np.zeros((k, 3))
    mean[:, 0] = 1000.0 + 10.0 * np.arange(k)
    mean[:, 1] = 1000.0
    mean[:, 2] = 0.5
    return mean, np.tile(np.eye(3) * 0.01, (k, 1, 1)), np.ones(k, np.int32), np.zeros(k, np.int32)


def _gates(b, c):
    """Filter 0 (two hypotheses) stays below nParticlesMax and meets an N_eff test it cannot pass (unforced: _run_shapes sets the
    thresholds); filters 1 and 2 (three) exceed nParticlesMax with every update (forced)."""
    if b % 3 == 0:
        c.nParticlesMax, c.minUpdatesBeforeResample, c.minMeasurementsBeforeResample = 16, 1, 0
    else:
        c.nParticlesMax, c.minUpdatesBeforeResample, c.minMeasurementsBeforeResample = 8, NEVER, 0


def _run_shapes(pkg, sc, stride, n_cycles=8):
    r = _Rig(pkg, sc, 3, stride, _gates)
    r.set_resampling(0, ALWAYS, ALWAYS)
    r.plant_lists(2, 2)                       # filter 2 meets its first update, which follows no resampling, with lists
    sets = _sets(r.scens, n_cycles, seed=5, empty=(3, 0))
    rng = np.random.default_rng(9)
    seen = dict(grew=[0, 0, 0], unforced=0, forced=0, travel=0, stay=0)
    prev_fired = [False] * 3
    for c in range(n_cycles):
        before = [(h.n, r.list_sizes(b)) for b, h in enumerate(r.handles)]
        u01 = rng.uniform(0, 1, 3)
        if c % 2:
            r.static_step()
        r.cycle(sets[c], u01, predict=(c % 2 == 0), scan=(r.scan * 0.995 if c == 4 else None))
        lc = r.compare("cycle %d" % c)
        for b, h in enumerate(r.handles):
            hl = h.fastslam_last_cycle()
            n0, lists = before[b]
            if not len(sets[c][b]):
                assert hl["n_after_update"] == n0 and not hl["fired"]
                continue
            copies = [s for s in range(n0, hl["n_after_update"]) if lists[hl["parent"][s]] > 0]
            seen["grew"][b] += hl["n_after_update"] > n0
            seen["travel" if prev_fired[b] else "stay"] += len(copies)
            if hl["fired"]:
                seen["forced" if hl["n_after_update"] > h.fs_config.nParticlesMax else "unforced"] += 1
            prev_fired[b] = hl["fired"]
        assert not lc["overflowed"].any()
    r.close()
    return seen


@gpu
@pytest.mark.parametrize("stride", [16, 15])
def test_every_filter_equals_its_handle_over_eight_cycles(pkg, sc, stride):
    """B = 3, 4 particles per filter, stride 16 or 15 (blocks that do not align with the four-particle workgroups of the static step
    and the prune), hypotheses (2, 3, 3), candidate thresholds (1, 2, 4), 2 ... 5 measurements, one empty set."""
    seen = _run_shapes(pkg, sc, stride)
    print("stride %d: %r" % (stride, seen))
    assert all(g > 0 for g in seen["grew"]), "a filter never grew"
    assert seen["unforced"] > 0 and seen["forced"] > 0, "the resamplings did not show both kinds"
    assert seen["travel"] > 0, "no copy was made of a particle with a candidate list directly after a resampling"
    assert seen["stay"] > 0, "no copy was made of a particle with a candidate list where no resampling preceded"


def _snapshot(r, b, n):
    s = r.block_state(b, n)
    return s


def _assert_block(a, c, what):
    mh.assert_same_state(a, c)
    for ca, cb in zip(a["cands"], c["cands"]):
        for x, y in zip(ca, cb):
            assert np.array_equal(x, y), what
    for x, y in zip(a["ids"], c["ids"]):
        assert np.array_equal(x, y), what


@gpu
@pytest.mark.parametrize("stride", [16, 15])
def test_overflow_is_per_filter(pkg, sc, stride):
    """Filter 1 (three hypotheses, no resampling) grows 4 -> 12 and would pass the stride with its second update: it is left as before
    that cycle, untouched by the propagation, the static step and two further cycles behind it; the others match their handles."""
    def gates(b, c):
        _gates(b, c)
        if b == 1:
            c.nParticlesMax = 64
    r = _Rig(pkg, sc, 3, stride, gates)
    r.set_resampling(0, ALWAYS, ALWAYS)
    sets = _sets(r.scens, 4, seed=6)
    u01 = np.array([0.2, 0.5, 0.8])
    r.cycle(sets[0], u01)
    r.compare("cycle 0")
    n1 = r.handles[1].n
    assert 3 * n1 > 2 * stride, "filter 1 did not grow enough for its next update to pass the stride"
    keep = _snapshot(r, 1, n1)
    r.cycle(sets[1], u01, skip=(1,))
    r.propagate([[1.0, 0.02], [1.2, 0.01]], [0.025, 0.025], skip=(1,))
    r.static_step(skip=(1,))
    r.cycle(sets[2], u01, predict=True, skip=(1,))
    r.cycle(sets[3], u01, skip=(1,))
    with pytest.raises(pkg.capi.EngineError) as e:
        r.batch.synchronize()
    assert e.value.status == pkg.capi.ERR_CAPACITY and "filter 1" in str(e.value), str(e.value)
    r.batch.synchronize()                                        # reported once
    lc = r.compare("behind the overflow", only=(0, 2))
    assert list(lc["overflowed"]) == [False, True, False]
    assert r.batch.live_counts()[1] == n1
    _assert_block(keep, _snapshot(r, 1, n1), "the overflowed filter was touched")
    r.close()


@gpu
def test_propagation_on_ragged_counts(pkg, sc):
    r = _Rig(pkg, sc, 3, 16, lambda b, c: setattr(c, "minUpdatesBeforeResample", NEVER))
    sets = _sets(r.scens, 1, seed=7)
    r.cycle(sets[0], np.array([0.1, 0.4, 0.7]))
    u = np.array([[1.0, 0.02], [1.2, -0.01], [0.8, 0.03]])
    r.propagate(u, np.full(3, 0.025))
    r.compare("after the run")
    counts = r.batch.live_counts()
    assert len(set(counts)) > 1 and (counts > N_PER).all(), counts
    poses = r.batch.get_poses()
    for b, h in enumerate(r.handles):
        got = poses[r.batch.block(b, h.n)]
        assert np.array_equal(got, h.get_poses())
        assert not np.array_equal(got[:N_PER], r.scens[b]["poses"])       # the poses did move
    r.close()


@gpu
def test_back_to_back_cycles_equal_synchronised_ones(pkg, sc):
    """Five cycles with propagation and static steps in between, enqueued with no read, against the same sequence with a
    synchronising call after each cycle."""
    out = []
    for wait in (True, False):
        r = _Rig(pkg, sc, 3, 15, _gates)
        r.set_resampling(0, ALWAYS, ALWAYS)
        for h in r.handles:
            h.close()
        r.handles = []
        sets = _sets(r.scens, 5, seed=8, empty=(2, 1))
        rng = np.random.default_rng(4)
        for c in range(5):
            r.cycle(sets[c], rng.uniform(0, 1, 3), predict=(c % 2 == 1))
            if wait:
                r.batch.synchronize()
            r.propagate([[1.0, 0.02], [1.1, 0.0]], [0.025, 0.025])
            r.static_step()
        counts = r.batch.live_counts()
        out.append(([r.block_state(b, int(counts[b])) for b in range(3)], r.batch.last_cycle()))
        r.close()
    (a, la), (c, lb) = out
    for b in range(3):
        _assert_block(a[b], c[b], "filter %d" % b)
    for k in la:
        assert np.array_equal(la[k], lb[k]), k


@gpu
def test_a_batch_of_one_equals_a_plain_handle(pkg, sc):
    def gates(b, c):
        c.nParticlesMax, c.minUpdatesBeforeResample, c.minMeasurementsBeforeResample = 6, NEVER, 0
    r = _Rig(pkg, sc, 1, 16, gates, hyps=(3,), thrs=(2,))
    sets = _sets(r.scens, 3, seed=3)
    grew = 0
    for c in range(3):
        r.cycle(sets[c], np.array([0.3 + 0.2 * c]), predict=True)
        r.compare("cycle %d" % c)
        grew += r.handles[0].fastslam_last_cycle()["n_after_update"] > N_PER
    assert grew
    r.close()


@gpu
def test_capacity_and_candidate_list_errors_name_the_lowest_filter(pkg, sc):
    # gm_capacity: every map padded to 62 landmarks of the 64 a slab holds (the padding lies a kilometre away), and four returns that
    # found landmarks at once (count threshold 1) in filters 1 and 2
    gates = lambda b, c: setattr(c, "minUpdatesBeforeResample", NEVER)
    r = _Rig(pkg, sc, 3, 16, gates, thrs=(1, 1, 1))
    for b, scen in enumerate(r.scens):
        for i in range(N_PER):
            k = 62 - scen["mean"][i].shape[0]
            pm, pc = vref_far_candidates(k)[:2]
            r.batch.import_gm(b * 16 + i, np.zeros(62), np.concatenate([scen["mean"][i], pm], 0), np.concatenate([scen["cov"][i], pc], 0))
    assert (np.asarray(r.batch.gm_sizes()).reshape(3, 16)[:, :N_PER] == 62).all()
    # (returns between the scene's in-range landmarks, which end at 60 m, and its out-of-range ones, which start at 80 m: no landmark takes them)
    far = np.array([[66.0 + 2 * k, 0.4 + 0.5 * k, 0.8] for k in range(4)])
    r.batch.cycle_async(False, [r.scens[0]["Z"][:2], far, far], np.full(3, 0.5))
    with pytest.raises(pkg.capi.EngineError) as e:
        r.batch.synchronize()
    assert e.value.status == pkg.capi.ERR_CAPACITY and "filter 1" in str(e.value) and "filter 2" not in str(e.value), str(e.value)
    r.close()
    # the 65th candidate in filters 1 and 2
    r = _Rig(pkg, sc, 3, 16, gates, thrs=(4, 4, 4), check_thr=100)
    for b in (1, 2):
        r.plant_lists(b, 64)
    # (three of the scene's own returns beside the unassociated one: with no landmark updated the whole list would be promoted, :656-688)
    r.batch.cycle_async(False, [np.concatenate([s["Z"][:3], far[:1]], 0) for s in r.scens], np.full(3, 0.5))
    with pytest.raises(pkg.capi.EngineError) as e:
        r.batch.synchronize()
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED and "candidate" in str(e.value), str(e.value)
    assert "filter 1" in str(e.value) and "filter 2" not in str(e.value), str(e.value)
    r.batch.synchronize()
    r.close()


def _refused(pkg, fn, needle=None):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED, str(e.value)
    assert len(str(e.value)) > 20
    if needle:
        assert needle in str(e.value), str(e.value)


@gpu
def test_refusals_leave_the_state_untouched(pkg, sc):
    r = _Rig(pkg, sc, 3, 16, _gates)
    B, nF = r.batch, 3
    r.cycle(_sets(r.scens, 1, seed=2)[0], np.array([0.2, 0.5, 0.8]))
    r.compare("before")
    counts = B.live_counts()
    keep = [r.block_state(b, int(counts[b])) for b in range(nF)]
    Z3 = [s["Z"][:2] for s in r.scens]
    Z2 = [s["Z"][:2, :2] for s in r.scens]
    V = pkg.capi.CVPBatch
    nz = np.full(nF, 2, dtype=np.int32)
    est_t = np.zeros(nF)
    calls = [
        lambda: V.batch_vp_cycle_async(B, True, Z3),
        lambda: V.batch_vp_fastslam_cycle_async(B, True, Z3),
        lambda: B.batch_cycle_async(True, Z2),
        lambda: B.batch_fastslam_cycle_async(True, Z2),
        lambda: B.batch_fastslam_mh_cycle_async(True, Z2, np.full(nF, 0.5)),
        lambda: V.batch_vp_resample_async(B, nz, 0),
        lambda: B.batch_resample_apply(np.arange(B.n, dtype=np.int32), np.ones(nF, dtype=np.uint8)),
        lambda: B.batch_weight_sums(),
        lambda: B.set_sensor(0, np.eye(2).ravel(), 0.9, 1e-3, 20.0, 1.0, np.zeros((2, 2)), 8, 1),
        lambda: B.sense_async(np.zeros((nF, 3)), 0),
        lambda: B.generate_truth(4),
        lambda: B.set_ground_truth(np.zeros((2, 2)), np.zeros(2), filter=0),
        lambda: B.step_error_async(np.zeros(nF), np.zeros((nF, 3))),
        lambda: B.estimate_log_create(4, 8),
        lambda: B.step_estimate_async(est_t),
        lambda: V.batch_vp_serve_fastslam(B, True),
        lambda: V.serve_estimates(B, True),
        lambda: B.serve_metrics(True),
        lambda: B.set_motion_odometry(0, np.ones(3) * 1e-3, 1),
        lambda: B.propagate_async(np.zeros((nF, 3)), 0),
        lambda: B.resample_async(nz, 0),
    ]
    for k, fn in enumerate(calls):
        try:
            _refused(pkg, fn)
        except (TypeError, AttributeError) as e:      # a wrapper whose arguments this test got wrong must not pass for a refusal
            raise AssertionError("call %d: %r" % (k, e))
    cfg = mb.copy_struct(r.handles[1].fs_config)
    cfg.maxNDataAssocHypotheses = 1
    _refused(pkg, lambda: B.batch_set_fastslam_config(1, cfg), "filter 1")
    counts2 = B.live_counts()
    assert np.array_equal(counts, counts2)
    for b in range(nF):
        _assert_block(keep[b], r.block_state(b, int(counts[b])), "filter %d changed under a refused call" % b)
    r.cycle(_sets(r.scens, 2, seed=2)[1], np.array([0.3, 0.6, 0.9]))       # and the batch still steps with its handles
    r.compare("after")
    r.close()


@gpu
def test_the_cycle_is_refused_on_every_other_kind_of_handle(pkg, sc):
    M = pkg.capi.CBatchVPMH
    z3, nz = np.zeros((2, pkg.capi.MAX_Z, 3)), np.zeros(2, dtype=np.int32)
    others = [pkg.VPFilterBatch(2, 4, gm_capacity=CAP), pkg.VPFastSLAMBatch(2, 4, gm_capacity=CAP), pkg.MHFastSLAMBatch(2, 4, 8, gm_capacity=CAP),
              pkg.FilterBatch(2, 4, gm_capacity=CAP)]
    for o in others:
        _refused(pkg, lambda: M.batch_vp_fastslam_mh_cycle_async_packed(o, False, z3, nz, np.full(2, 0.5)), "rfsgpu_create_batch_vp_mh")
        o.close()
    h = pkg.RBPHDFilter(4, gm_capacity=CAP, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    u = np.full(2, 0.5)
    _refused(pkg, lambda: h._call("batch_vp_fastslam_mh_cycle_async", C.c_int(0), None, None, C.c_int(0), h._ptr(z3), h._ptr(nz), None, C.c_int(0), h._ptr(u)),
             "rfsgpu_create_batch_vp_mh")
    h.close()
    with pytest.raises(pkg.capi.EngineError) as e:               # and the 2-D creator keeps refusing the model
        pkg.capi.CBatchMH(pkg.load_library(), "rfsgpu_", 2, 4, 8, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED


@gpu
def test_driver_batch_run_equals_the_handles_in_turn(pkg, sc):
    """VictoriaParkBatchRun(filter="mhfastslam") over a prefix of the dataset extract: 3 filters x 6 particles with their own seeds,
    clutter rates and parameter sets on the reference configuration's hypotheses, window and candidate threshold, against the same
    realisations through three handles -- every lidar message's counts, decisions, plans and grown counts, and the states at the end."""
    from test_vp_filter_batch import _driver_filters
    drv, capi = pkg.vp_driver, pkg.capi
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    nF, n, cap, hyp, n_msgs = 3, 6, 256, 3, 300
    Ps, seeds, clutter = _driver_filters(sc, nF)

    def fs_cfg(cfg):
        cfg.maxNDataAssocHypotheses = hyp
        cfg.maxDataAssocLogLikelihoodDiff = 3.0
        cfg.landmarkCandidateMeasurementCountThreshold = 4
        cfg.landmarkCandidateMeasurementCheckThreshold = 6
        cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
        cfg.landmarkCandidateMeasurementSupportDist = 3.0
        cfg.nParticlesMax = 3 * n
        return cfg

    batch = pkg.VPMHFastSLAMBatch(nF, n, gm_capacity=cap, max_hypotheses=hyp)
    stride = batch.max_per_filter
    assert stride == 3 * n * hyp
    handles = [pkg.FastSLAM(n, gm_capacity=cap, max_hypotheses=hyp, device_cycle=True, max_particles=stride, model=capi.MODEL_VICTORIAPARK_3D)
               for _ in range(nF)]
    for b in range(nF):
        sc.apply_vp_batch_params(batch, b, Ps[b])
        batch.configure_fastslam(b, fs_cfg(batch.fs_configs[b]))
        sc.apply_vp_params(handles[b], Ps[b], np.full(361, 70.0))
        handles[b].config = handles[b].get_filter_config()
        fs_cfg(handles[b].fs_config)
    for bad in (dict(device_loop=False), dict(device_loop=True, log_estimates=True)):
        with pytest.raises(ValueError):
            drv.VictoriaParkBatchRun(batch, data, Ps, seeds, filter="mhfastslam", **bad)
    kw = dict(added_clutter=clutter, keep_history=True, device_loop=True, filter="mhfastslam")
    rh = drv.VictoriaParkBatchRun(handles, data, Ps, seeds, **kw).run(n_msgs)
    grown, fired = np.array(rh.grown), np.array([h[1] for h in rh.history])
    assert (grown.max(0) > n).all(), "a handle never grew: %r" % grown.max(0)
    assert fired.any(0).all(), "a handle never resampled: the prefix is too short"
    rb = drv.VictoriaParkBatchRun(batch, data, Ps, seeds, **kw).run(n_msgs)
    assert rb.n_lidar == rh.n_lidar > 5 and len(rb.history) == len(rh.history) == rb.n_lidar
    for k, ((nzb, fb, pb), (nzh, fh, ph)) in enumerate(zip(rb.history, rh.history)):
        np.testing.assert_array_equal(nzb, nzh, err_msg=f"lidar message {k}: counts")
        np.testing.assert_array_equal(fb, fh, err_msg=f"lidar message {k}: resampling decisions")
        np.testing.assert_array_equal(rb.grown[k], rh.grown[k], err_msg=f"lidar message {k}: grown counts")
        for b in range(nF):
            np.testing.assert_array_equal(pb[b], ph[b], err_msg=f"lidar message {k} filter {b}: plan")
    counts = batch.live_counts()
    r = _Rig.__new__(_Rig)
    r.pkg, r.sc, r.nF, r.n_per, r.stride, r.batch, r.handles = pkg, sc, nF, n, stride, batch, handles
    for b, h in enumerate(handles):
        assert counts[b] == h.n
        np.testing.assert_array_equal(rb.x[batch.block(b, h.n)], h.get_poses())
    r.compare("end of the run")
    r.close()
