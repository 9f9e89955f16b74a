"""A batch of Victoria Park RB-PHD filters (rfsgpu_create_batch with the Victoria Park model, rfsgpu_batch_configure_vp,
rfsgpu_batch_vp_cycle_async; include/rfsgpu.h [batch]).  The reference result is the plain Victoria Park handle, which the rest of the
suite holds to the oracle: every filter of a batch must give what its own handle gives on the same inputs -- mixture sizes, unused
masks, candidate lists (means, covariances, support and check counts), ids and parent ids exactly, mixtures bit for bit, weights to
rtol 1e-12 (each filter's sum has its own workgroup; the bound the 2-D batch tests use)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

VP_BATCH_SYMBOLS = ["rfsgpu_batch_configure_vp", "rfsgpu_batch_vp_cycle_async"]
CAP = 256           # gm_capacity of every handle here
TH0 = 0.3           # the scenarios' vehicle heading (scenarios.make_vp_scenario)
# two clutter points no landmark of the scenarios comes near (their landmarks in view lie within 60 m): A returns, B is seen once
CLUTTER_A = np.array([66.0, np.deg2rad(166.0), 1.0])
CLUTTER_B = np.array([66.0, np.deg2rad(17.0), 1.0])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_vp_batch_entry_points(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in VP_BATCH_SYMBOLS:
        assert hasattr(lib, s), s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS


def test_header_declares_the_vp_batch_calls_outside_the_stable_core():
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    sec = txt.index("[batch]")
    for s in VP_BATCH_SYMBOLS:
        assert s not in core, s
        assert txt.index(s + "(") > sec, s


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _detections(scen, rng, n):
    """n noisy (range, bearing, diameter) detections of landmarks in view, seen from the scenario's nominal pose."""
    gt = scen["gt"]
    r = np.hypot(gt[:, 0], gt[:, 1])
    b = np.arctan2(gt[:, 1], gt[:, 0]) - TH0 + np.pi / 2
    idx = np.nonzero(r < 62.0)[0]
    pick = rng.choice(idx, size=min(n, idx.size), replace=False)
    return np.stack([r[pick] + rng.normal(0, 0.1, pick.size), b[pick] + rng.normal(0, 0.002, pick.size), gt[pick, 2] + rng.normal(0, 0.02, pick.size)], 1)


def _filter_params(sc, b, all_heavy=False, cluster_filter=1):
    """Filters that differ in Pd table, expected clutter, evaluation points, cluster process and birth thresholds.  Filter
    cluster_filter runs the cluster process (useClusterProcess = 1: no importance weighting, its waves go from the map update straight
    to the merge beside waves of the other filters that weight); the others weight with 1, 15 and 64 evaluation points."""
    tweaks = [dict(pd_table=[0.0, 0.05, 0.35, 0.76, 0.89, 0.90], expected_clutter=6.0, n_eval=1, birth_count_thr=1),
              dict(pd_table=[0.0, 0.1, 0.5, 0.8, 0.95], expected_clutter=2.0, n_eval=15, birth_count_thr=2, birth_check_thr=3),
              dict(pd_table=[0.0, 0.3, 0.6, 0.85], expected_clutter=11.0, n_eval=64, birth_count_thr=3, birth_check_thr=3)]
    P = dict(sc.VP_PARAMS)
    P.update(tweaks[b % len(tweaks)])
    P["use_cluster"] = int(b == cluster_filter)
    if all_heavy:
        P["n_eval"] = 64
    return P


def _sets(scens, n_cycles, seed, nz_max_at=(6, 2)):
    """Per cycle and filter a measurement set [n_z, 3].  Sizes 0 (filter 1, cycles 4 and 6, while the others have measurements), 1
    (filter 0, cycle 5) and RFSGPU_MAX_Z (nz_max_at: cycle, filter).  Clutter A is in every filter's set in cycles 1, 2 and 3 -- a
    candidate is created from it, supported, and promoted at the filter's count threshold --, clutter B in cycle 1 only: its candidate
    expires once its check count passes the threshold."""
    rng = np.random.default_rng(seed)
    nF = len(scens)
    out = []
    for c in range(n_cycles):
        row = []
        for b in range(nF):
            Z = _detections(scens[b], rng, 4 + (c + 2 * b) % 5)
            if c in (1, 2, 3):
                Z = np.concatenate([Z, CLUTTER_A[None]], 0)
            if c == 1:
                Z = np.concatenate([Z, CLUTTER_B[None]], 0)
            if b == 1 and c in (4, 6):
                Z = np.zeros((0, 3))
            if b == 0 and c == 5:
                Z = Z[:1]
            if (c, b) == tuple(nz_max_at):
                extra = np.stack([rng.uniform(5.0, 70.0, 64), rng.uniform(0.2, 3.0, 64), rng.uniform(0.3, 1.5, 64)], 1)
                Z = np.concatenate([Z, extra], 0)[:64]
            row.append(Z)
        out.append(row)
    return out


class _Pair:
    """A VPFilterBatch and one plain Victoria Park handle per filter, loaded with the same state."""

    def __init__(self, pkg, nF, nPer, all_heavy=False, n_landmarks=12, cluster_filter=1):
        sc = pkg.scenarios
        self.pkg, self.nF, self.nPer = pkg, nF, nPer
        self.scens = [sc.make_vp_scenario(nPer, n_landmarks, 6, seed=900 + b, params=_filter_params(sc, b, all_heavy, cluster_filter)) for b in range(nF)]
        self.batch = pkg.VPFilterBatch(nF, nPer, gm_capacity=CAP)
        self.handles = [pkg.RBPHDFilter(nPer, gm_capacity=CAP, model=pkg.capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
        for b, (h, scen) in enumerate(zip(self.handles, self.scens)):
            sc.load_scenario(h, scen)
            sc.apply_vp_batch_params(self.batch, b, scen["params"])
            for i in range(nPer):
                self.batch.import_gm(b * nPer + i, scen["w"][i], scen["mean"][i], scen["cov"][i])
        # the configurations that reached the engine differ in the cluster process: exactly filter cluster_filter runs it
        assert [int(c.useClusterProcess) for c in self.batch.configs] == [int(b == cluster_filter) for b in range(nF)]
        assert [int(h.get_filter_config().useClusterProcess) for h in self.handles] == [int(b == cluster_filter) for b in range(nF)]
        self.batch.set_laser_scan(self.scens[0]["scan"])
        self.poses = np.concatenate([s["poses"] for s in self.scens], 0)
        self.batch.set_poses(self.poses, np.zeros((3, 3)))
        self.batch.set_weights(np.ones(nF * nPer))
        self.variants = []

    def cycle(self, Zs, predict=True, poses=None, scan=None, normalize=True):
        self.batch.cycle_async(predict, Zs, poses=poses, scan=scan, normalize=normalize)
        self.variants.append(self.batch.last_step_variant()[2])
        for b, h in enumerate(self.handles):
            if scan is not None:
                h.set_laser_scan(scan)
            h.cycle_async(predict, Zs[b], poses=None if poses is None else poses[b * self.nPer:(b + 1) * self.nPer], normalize=normalize)

    def resample(self, plans):
        """plans: {filter: local source slots}; the other filters are not resampled."""
        glob = np.arange(self.nF * self.nPer, dtype=np.int32)
        flags = np.zeros(self.nF, dtype=np.uint8)
        for b, p in plans.items():
            glob[b * self.nPer:(b + 1) * self.nPer] = b * self.nPer + np.asarray(p)
            flags[b] = 1
            self.handles[b].resample_apply(np.asarray(p, dtype=np.int32))
        self.batch.batch_resample_apply(glob, flags)

    def candidates(self, b):
        """[(support, checks) lists per slot] of filter b's handle."""
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
                np.testing.assert_array_equal(wb[blk], h.get_weights(), err_msg=f"{what} filter {b}: weights")
            else:
                np.testing.assert_allclose(wb[blk], h.get_weights(), rtol=1e-12, atol=0, err_msg=f"{what} filter {b}: weights")
            for i in range(nP):
                for x, y in zip(batch.export_gm(b * nP + i), h.export_gm(i)):
                    np.testing.assert_array_equal(x, y, err_msg=f"{what} filter {b} particle {i}: mixture")
                for x, y in zip(batch.export_birth_candidates(b * nP + i), h.export_birth_candidates(i)):
                    np.testing.assert_array_equal(x, y, err_msg=f"{what} filter {b} particle {i}: candidate list")

    def close(self):
        self.batch.close()
        for h in self.handles:
            h.close()


def _list_events(before, after, count_thr, check_thr, ev):
    """What one birth predict did to a slot's candidate list, from its (support, checks) pairs before and after: the list keeps its order,
    survivors are one check older, new candidates stand at the end with one check."""
    j = 0
    for sup, chk in before:
        if j < len(after) and after[j][1] == chk + 1 and after[j][0] >= sup:
            ev["supported"] += int(after[j][0] > sup)
            j += 1
        elif chk + 1 > check_thr and sup + 1 < count_thr:
            ev["expired"] += 1      # (one measurement supports a candidate once: it cannot have reached the count threshold)
        else:
            ev["promoted"] += 1
    ev["created"] += sum(1 for sup, chk in after[j:] if chk == 1)


def _run_shapes(pkg, nPer, order=None, n_cycles=8):
    """The smallest-shapes run: nF = 3 (filter 1 runs the cluster process, filters 0 and 2 weight with 1 and 64 evaluation points),
    eight cycles of predict = 1 + update, compared after every cycle."""
    p = _Pair(pkg, 3, nPer)
    if order is not None:
        p.batch.step_launch_order(order=order, want_costs=False)
    sets = _sets(p.scens, n_cycles, seed=5)
    ev = dict(created=0, supported=0, promoted=0, expired=0)
    rng = np.random.default_rng(77)
    sizes = set()
    for c in range(n_cycles):
        before = [p.candidates(b) for b in range(3)]
        poses = p.poses + rng.normal(0, 0.004, p.poses.shape) if c == 3 else None     # (one cycle hands new poses over)
        p.cycle(sets[c], predict=True, poses=poses)
        p.compare(f"cycle {c}")
        for b in range(3):
            P = p.scens[b]["params"]
            sizes.add(len(sets[c][b]))
            for i in range(nPer):
                _list_events(before[b][i], p.candidates(b)[i], P["birth_count_thr"], P["birth_check_thr"], ev)
    assert {0, 1, 64} <= sizes
    variants = set(p.variants)
    p.close()
    return ev, variants


@pytest.mark.gpu
def test_create_vp_batch(pkg):
    capi = pkg.capi
    lib = pkg.load_library()
    h = C.c_void_p()
    lib.rfsgpu_create_batch.restype = C.c_int
    assert lib.rfsgpu_create_batch(C.byref(h), C.c_int(capi.MODEL_VICTORIAPARK_3D), C.c_int(3), C.c_int(5), C.c_int(0), C.c_int(128)) == capi.OK
    lib.rfsgpu_n_filters.restype = C.c_int
    lib.rfsgpu_n_particles.restype = C.c_int
    assert lib.rfsgpu_n_filters(h) == 3 and lib.rfsgpu_n_particles(h) == 15
    lib.rfsgpu_destroy.restype = None
    lib.rfsgpu_destroy(h)
    batch = pkg.VPFilterBatch(3, 5, gm_capacity=128)
    assert batch.n_filters_abi() == 3 and batch.n == 15 and batch.gm_capacity == 128
    assert batch.gm_sizes().shape == (15,)
    batch.close()
    h = C.c_void_p()
    lib.rfsgpu_create_batch_mh.restype = C.c_int       # the multi-hypothesis batch keeps refusing the model
    assert lib.rfsgpu_create_batch_mh(C.byref(h), C.c_int(capi.MODEL_VICTORIAPARK_3D), C.c_int(2), C.c_int(4), C.c_int(8), C.c_int(0), C.c_int(64)) == capi.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_smallest_shapes_equal_the_handles(pkg):
    """nPer = 5: slots 4|5 and 9|10 share a two-particle workgroup across filters."""
    ev, variants = _run_shapes(pkg, 5)
    for k, v in ev.items():
        assert v > 0, f"no candidate was {k} in the whole run: {ev}"
    assert variants >= {1, 2}, variants      # (the cycle with 64 measurements beside 64 evaluation points runs one particle per workgroup)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["reversed", "interleaved"])
def test_cost_ordered_launch_keeps_the_bits(pkg, kind):
    """A host-given launch order puts every workgroup across filters; the run compares against the handles after every cycle."""
    n = 15
    order = np.arange(n)[::-1] if kind == "reversed" else np.array([(k % 3) * 5 + k // 3 for k in range(n)])
    assert sorted(order) == list(range(n))
    ev, _ = _run_shapes(pkg, 5, order=order)
    assert ev["created"] > 0 and ev["promoted"] > 0


@pytest.mark.gpu
def test_one_particle_per_workgroup_form(pkg):
    """64 evaluation points beside sets of 64 at gm_capacity 256: two waves' areas do not fit in 64 KiB, the WPB = 1 form runs."""
    p = _Pair(pkg, 3, 5, all_heavy=True, cluster_filter=0)      # (the filter with the full set runs the cluster process here)
    sets = _sets(p.scens, 3, seed=8, nz_max_at=(1, 0))
    for c in range(3):
        p.cycle(sets[c])
        p.compare(f"cycle {c}")
    assert p.variants[1] == 1 and p.variants[0] == 2, p.variants
    lds = p.batch.last_cycle_lds()
    assert 0 < lds <= 64 * 1024
    p.close()


@pytest.mark.gpu
def test_resampling_and_the_inheritance_walk(pkg):
    nPer = 6
    p = _Pair(pkg, 3, nPer, cluster_filter=2)      # (filter 2, with the deeper chain and the long list, runs the cluster process)
    sets = _sets(p.scens, 7, seed=21, nz_max_at=(5, 2))
    for c in range(2):
        p.cycle(sets[c])
    # an earlier resampling of every filter: its ids stay, its flag is cleared by the next update with measurements
    p.resample({0: [0, 1, 2, 3, 4, 3], 1: [0, 1, 1, 3, 4, 5], 2: [0, 1, 2, 3, 2, 5]})
    p.compare("first resampling")
    for c in range(2, 4):
        p.cycle(sets[c])
        p.compare(f"cycle {c}")
    assert not p.batch.batch_resample_occured().any()
    # filters 0 and 2 only.  Filter 0: slot 0 takes a higher slot, slot 4 a lower one, slot 5 keeps a copy whose id is slot 3's
    # (levels 0 / 1 / 1).  Filter 2: slot 2 takes slot 0, slot 4 keeps the copy of slot 2 it got earlier: the chain 4 -> 2 -> 0.
    p.resample({0: [1, 1, 2, 3, 2, 5], 2: [0, 1, 0, 3, 4, 5]})
    np.testing.assert_array_equal(p.batch.batch_resample_occured(), [True, False, True])
    _, par = p.handles[2].get_particle_ids()
    assert par[4] == 2 and par[2] == 0
    _, par1 = p.handles[1].get_particle_ids()
    assert par1[2] == 1                                  # filter 1: idParent_ != slot from the earlier resampling, flag clear
    # a list longer than a wavefront where the walk copies it: 70 far candidates in filter 2's slot 0 (the source of slot 2)
    k = 70
    mean = np.stack([np.linspace(200.0, 900.0, k), np.full(k, -300.0), np.full(k, 1.0)], 1)
    cov = np.tile(np.diag([0.5, 0.5, 0.01]), (k, 1, 1))
    for f, slot in ((p.batch, 2 * nPer), (p.handles[2], 0)):
        f.import_birth_candidates(slot, mean, cov, np.ones(k, dtype=np.int32), np.zeros(k, dtype=np.int32))
    # filter 1's slots 1 and 2 have held the same state since the first resampling, so a copy between them would change no bit: slot 1
    # gets a candidate of its own, far from everything, that a walk in filter 1 would carry into slot 2
    marker = np.array([[-400.0, 650.0, 1.0]])
    m1, c1, s1, k1 = p.handles[1].export_birth_candidates(1)
    own = (np.concatenate([m1, marker], 0), np.concatenate([c1, np.diag([0.5, 0.5, 0.01])[None]], 0), np.append(s1, 1).astype(np.int32),
           np.append(k1, 0).astype(np.int32))
    for f, slot in ((p.batch, nPer + 1), (p.handles[1], 1)):
        f.import_birth_candidates(slot, *own)
    has_marker = lambda f, slot: bool((f.export_birth_candidates(slot)[0] == marker[0]).all(axis=1).any())
    assert has_marker(p.batch, nPer + 1) and not has_marker(p.batch, nPer + 2)
    p.cycle(sets[4])                                      # (filter 1 has no measurements in this cycle: its flag would stay anyway)
    p.compare("first birth predict after the resampling")
    assert len(p.handles[2].export_birth_candidates(2)[2]) >= 64, "the long list did not travel with the walk"
    for f, s1, s2 in ((p.batch, nPer + 1, nPer + 2), (p.handles[1], 1, 2)):
        assert has_marker(f, s1) and not has_marker(f, s2), "filter 1 (flag clear) copied a parent's candidate list"
    p.cycle(sets[5])
    p.compare("second birth predict")
    p.cycle(sets[6])
    p.compare("last cycle")
    p.close()


@pytest.mark.gpu
def test_batch_of_one_is_bit_identical_to_a_plain_handle(pkg):
    p = _Pair(pkg, 1, 7)
    sets = _sets(p.scens, 5, seed=3, nz_max_at=(9, 9))
    for c in range(5):
        p.cycle(sets[c])
        p.compare(f"cycle {c}", exact_weights=True)
    p.close()


def _driver_filters(sc, nF):
    Ps, seeds, clutter = [], [], []
    for b in range(nF):
        P = dict(sc.VP_PARAMS)
        P["expected_clutter"] = [6.0, 3.0, 9.0, 6.0][b % 4]
        P["pd_table"] = [[0.0, 0.05, 0.35, 0.76, 0.89, 0.90], [0.0, 0.1, 0.5, 0.8, 0.95]][b % 2]
        P["min_updates"] = [2, 3, 2, 4][b % 4]             # (the resampling gates open at different messages in different filters)
        P["min_measurements"] = [15, 15, 30, 15][b % 4]
        Ps.append(P)
        seeds.append(31 + 7 * b)
        clutter.append([3.0, 1.0, 5.0, 0.0][b % 4])
    return Ps, seeds, clutter


@pytest.mark.gpu
def test_driver_batch_run_equals_the_handles_in_turn(pkg):
    """VictoriaParkBatchRun over the 900-message dataset extract, 4 filters x 20 particles with their own seeds, clutter rates and
    parameter sets: the batch against the same realisations through four handles -- every lidar message's counts, decisions and
    plans, and the states at the end."""
    sc, drv, capi = pkg.scenarios, pkg.vp_driver, pkg.capi
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    nF, n = 4, 20
    Ps, seeds, clutter = _driver_filters(sc, nF)
    cap = 384       # (192, the benchmark's capacity, is transiently short for the filter with the heaviest clutter: the handle alone says so too)
    batch = pkg.VPFilterBatch(nF, n, gm_capacity=cap)
    handles = [pkg.RBPHDFilter(n, gm_capacity=cap, model=capi.MODEL_VICTORIAPARK_3D) for _ in range(nF)]
    for b in range(nF):
        sc.apply_vp_batch_params(batch, b, Ps[b])
        sc.apply_vp_params(handles[b], Ps[b], np.full(361, 70.0))
    rb = drv.VictoriaParkBatchRun(batch, data, Ps, seeds, added_clutter=clutter, keep_history=True).run()
    rh = drv.VictoriaParkBatchRun(handles, data, Ps, seeds, added_clutter=clutter, keep_history=True).run()
    assert rb.n_lidar == rh.n_lidar > 50 and len(rb.history) == len(rh.history) == rb.n_lidar
    partial = 0
    for k, ((nzb, fb, pb), (nzh, fh, ph)) in enumerate(zip(rb.history, rh.history)):
        np.testing.assert_array_equal(nzb, nzh, err_msg=f"lidar message {k}: counts")
        np.testing.assert_array_equal(fb, fh, err_msg=f"lidar message {k}: resampling decisions")
        for b in range(nF):
            np.testing.assert_array_equal(pb[b], ph[b], err_msg=f"lidar message {k} filter {b}: plan")
        partial += int(fh.any() and not fh.all())
    assert (rh.n_resamples > 0).sum() >= 2, rh.n_resamples
    assert partial > 0, "no update after which only some filters resampled"
    np.testing.assert_array_equal(rb.x, rh.x)
    sizes, w, masks = batch.gm_sizes(), batch.get_weights(), batch.get_unused_masks()
    ids, par = batch.get_particle_ids()
    for b, h in enumerate(handles):
        blk = slice(b * n, (b + 1) * n)
        np.testing.assert_array_equal(sizes[blk], h.gm_sizes())
        np.testing.assert_array_equal(masks[blk], h.get_unused_masks())
        np.testing.assert_allclose(w[blk], h.get_weights(), rtol=1e-12, atol=0)
        hid, hpar = h.get_particle_ids()
        np.testing.assert_array_equal(ids[blk] - b * n, hid)
        np.testing.assert_array_equal(par[blk] - b * n, hpar)
        for i in range(n):
            for x, y in zip(batch.export_gm(b * n + i), h.export_gm(i)):
                np.testing.assert_array_equal(x, y, err_msg=f"filter {b} particle {i}: mixture")
            for x, y in zip(batch.export_birth_candidates(b * n + i), h.export_birth_candidates(i)):
                np.testing.assert_array_equal(x, y, err_msg=f"filter {b} particle {i}: candidate list")
    batch.close()
    for h in handles:
        h.close()


@pytest.mark.gpu
def test_capacity_overflow_names_the_filter(pkg):
    """Filter 1 only stands at gm_capacity when its update wants room for new Gaussians."""
    sc = pkg.scenarios
    capi = pkg.capi
    nF, nPer, cap = 3, 4, 64
    batch = pkg.VPFilterBatch(nF, nPer, gm_capacity=cap)
    scens = [sc.make_vp_scenario(nPer, cap if b == 1 else 10, 8, seed=40 + b, frac_in_fov=1.0) for b in range(nF)]
    for b, scen in enumerate(scens):
        sc.apply_vp_batch_params(batch, b, scen["params"])
        for i in range(nPer):
            batch.import_gm(b * nPer + i, scen["w"][i], scen["mean"][i], scen["cov"][i])
    batch.set_laser_scan(scens[0]["scan"])
    batch.set_poses(np.concatenate([s["poses"] for s in scens], 0), np.zeros((3, 3)))
    batch.cycle_async(None, [s["Z"] for s in scens])
    with pytest.raises(capi.EngineError) as e:
        batch.synchronize()
    assert e.value.status == capi.ERR_CAPACITY and "filter 1" in str(e.value), str(e.value)
    batch.close()


@pytest.mark.gpu
def test_full_candidate_list_names_the_filter(pkg):
    """Filter 1 only: one slot's list stands at RFSGPU_MAX_CANDIDATES when its birth predict has an unused measurement to add."""
    capi = pkg.capi
    nPer = 4
    p = _Pair(pkg, 3, nPer)
    sets = _sets(p.scens, 2, seed=13, nz_max_at=(9, 9))
    batch = p.batch
    batch.cycle_async(True, [np.concatenate([z, CLUTTER_A[None]], 0) for z in sets[0]])      # (the clutter point is used by no landmark)
    batch.synchronize()
    slot = nPer + 2
    assert batch.get_unused_masks()[slot] != 0
    k = capi.MAX_CANDIDATES
    mean = np.stack([np.linspace(200.0, 900.0, k), np.full(k, -300.0), np.full(k, 1.0)], 1)      # far from every measurement: none is supported
    batch.import_birth_candidates(slot, mean, np.tile(np.diag([0.5, 0.5, 0.01]), (k, 1, 1)), np.ones(k, dtype=np.int32), np.zeros(k, dtype=np.int32))
    batch.cycle_async(True, sets[1])
    with pytest.raises(capi.EngineError) as e:
        batch.synchronize()
    assert e.value.status == capi.ERR_UNSUPPORTED and "candidate list full in filter 1" in str(e.value), str(e.value)
    p.close()


@pytest.mark.gpu
def test_refusals_leave_the_state_untouched(pkg):
    capi = pkg.capi
    lib = pkg.load_library()
    lib.rfsgpu_last_error.restype = C.c_char_p
    p = _Pair(pkg, 3, 5)
    sets = _sets(p.scens, 2, seed=11, nz_max_at=(9, 9))
    p.cycle(sets[0])
    batch = p.batch
    batch.synchronize()
    state = (batch.get_weights(), batch.gm_sizes(), batch.get_unused_masks())
    z2 = np.zeros((3, capi.MAX_Z, 2))
    z3 = np.zeros((3, capi.MAX_Z, 3))
    nz = np.array([1, 1, 1], dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    var3 = np.ones(3)
    fs = batch.default_fastslam_config()
    t = np.zeros(3)
    refused = [
        ("batch_cycle_async", (C.c_int(1), None, None, C.c_int(0), vp(z2), vp(nz), C.c_int(1))),
        ("batch_fastslam_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z2), vp(nz), C.c_int(1))),
        ("batch_set_fastslam_config", (C.c_int(-1), C.byref(fs))),
        ("batch_fastslam_mh_cycle_async", (C.c_int(0), None, None, C.c_int(0), vp(z2), vp(nz), vp(t))),
        ("batch_set_motion_odometry", (C.c_int(-1), vp(var3), C.c_ulonglong(1))),
        ("batch_set_resampling", (C.c_int(-1), C.c_double(2.0), C.c_double(0.5))),
        ("batch_propagate_async", (vp(np.zeros((3, 3))), None, None, C.c_ulonglong(0))),
        ("batch_resample_async", (vp(nz), C.c_ulonglong(0))),
        ("batch_sense_async", (vp(np.zeros((3, 3))), C.c_ulonglong(0))),
        ("batch_cycle_sensed_async", (C.c_int(1), None, None, C.c_int(0), C.c_int(1))),
        ("batch_generate_truth", (C.c_int(4),)),
        ("error_log_create", (C.c_int(4),)),
        ("step_error_async", (vp(t), None, C.c_double(0.75), C.c_double(0.2), C.c_double(1.0))),
        ("estimate_log_create", (C.c_int(4), C.c_int(8), C.c_int(0))),
        ("step_estimate_async", (vp(t), C.c_double(0.75))),
        ("rbphd_cycle_async", (vp(z3), C.c_int(1), None, C.c_int(0), C.c_double(0.5))),
    ]
    for name, args in refused:
        fn = getattr(lib, "rfsgpu_" + name)
        fn.restype = C.c_int
        assert fn(batch._h, *args) == capi.ERR_UNSUPPORTED, name
        assert len(lib.rfsgpu_last_error(batch._h)) > 20, name
    with pytest.raises(capi.EngineError) as e:
        batch.set_birth_inheritance(2)                      # RFSGPU_INHERIT_EXTERNAL
    assert e.value.status == capi.ERR_UNSUPPORTED
    # the other model's configuration call, both ways round
    fn = lib.rfsgpu_batch_configure
    fn.restype = C.c_int
    assert fn(batch._h, C.c_int(0), None, None, None, None) == capi.ERR_INVALID and b"another model" in lib.rfsgpu_last_error(batch._h)
    flat = pkg.FilterBatch(2, 4, gm_capacity=64)
    fn = lib.rfsgpu_batch_configure_vp
    fn.restype = C.c_int
    assert fn(flat._h, C.c_int(0), None, None, None, None) == capi.ERR_INVALID and b"another model" in lib.rfsgpu_last_error(flat._h)
    cyc = lib.rfsgpu_batch_vp_cycle_async
    cyc.restype = C.c_int
    nz2 = np.array([1, 1], dtype=np.int32)
    assert cyc(flat._h, C.c_int(1), None, None, C.c_int(0), vp(z3), vp(nz2), None, C.c_int(0), C.c_int(1)) == capi.ERR_UNSUPPORTED
    flat.close()
    # bad arguments name the call and, where one is at fault, the filter
    def bad(*args):
        assert cyc(batch._h, *args) == capi.ERR_INVALID
        return lib.rfsgpu_last_error(batch._h)
    many = np.array([1, capi.MAX_Z + 1, 0], dtype=np.int32)
    assert b"batch_vp_cycle" in bad(C.c_int(1), None, None, C.c_int(0), vp(z3), vp(many), None, C.c_int(0), C.c_int(1)) and b"filter 1" in lib.rfsgpu_last_error(batch._h)
    assert b"null measurement buffer" in bad(C.c_int(1), None, None, C.c_int(0), None, vp(nz), None, C.c_int(0), C.c_int(1))
    assert b"null measurement counts" in bad(C.c_int(1), None, None, C.c_int(0), vp(z3), None, None, C.c_int(0), C.c_int(1))
    assert b"cov_stride" in bad(C.c_int(1), vp(np.zeros((15, 3))), vp(np.zeros(9)), C.c_int(4), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1))
    assert b"predict" in bad(C.c_int(2), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1))
    assert b"scan" in bad(C.c_int(1), None, None, C.c_int(0), vp(z3), vp(nz), vp(np.ones(4)), C.c_int(1), C.c_int(1))
    fresh = pkg.VPFilterBatch(3, 5, gm_capacity=CAP)      # a batch that has never been given a scan
    assert cyc(fresh._h, C.c_int(1), None, None, C.c_int(0), vp(z3), vp(nz), None, C.c_int(0), C.c_int(1)) == capi.ERR_INVALID
    assert b"scan" in lib.rfsgpu_last_error(fresh._h)
    fresh.close()
    batch.synchronize()
    for x, y in zip(state, (batch.get_weights(), batch.gm_sizes(), batch.get_unused_masks())):
        np.testing.assert_array_equal(x, y)
    # ... and the batch still steps with its handles
    p.cycle(sets[1], scan=np.full(361, 65.0))              # (the call's own scan: every filter's clutter density follows it)
    p.compare("after the refusals")
    p.close()
