"""Filter batches (rfsgpu_create_batch, include/rfsgpu.h [batch]): many independent 2-D RB-PHD filters stepped together in one launch
chain.  Each filter of a batch must give what a separate handle gives with the same inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

BATCH_SYMBOLS = ["rfsgpu_create_batch", "rfsgpu_n_filters", "rfsgpu_batch_configure", "rfsgpu_batch_cycle_async", "rfsgpu_batch_weight_sums",
                 "rfsgpu_batch_resample_apply", "rfsgpu_batch_resample_occured"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_batch_entry_points(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in BATCH_SYMBOLS + ["rfsgpu_murty_seen"]:
        assert hasattr(lib, s), s


def test_header_declares_the_batch_section_outside_the_stable_core():
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    m = re.search(r"STABLE CORE.*?\*/", head, flags=re.S)
    assert m is not None
    core = m.group(0)
    sec = txt.index("[batch]")
    for s in BATCH_SYMBOLS:
        assert s not in core, s
        k = txt.index(s + "(")
        assert k > sec, s


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _grid(sim, n):
    """(Pd, clutter, seed) of batchSim_rbphdslam.bash's kind, one per filter."""
    pds = [0.99, 0.8, 0.5, 0.9, 0.7, 0.95]
    clutters = [1e-4, 5e-3, 2e-2, 1e-3, 1e-2, 2e-3]
    out = []
    for b in range(n):
        P = dict(sim.C1_SIM)
        P["Pd"] = pds[b % len(pds)]
        P["clutter"] = clutters[(b * 5 + 1) % len(clutters)]
        out.append((P, 11 + b))
    return out


def _setup(sim, n_filters, K, tweak=None):
    Ps, datas, seeds = [], [], []
    for b, (P, seed) in enumerate(_grid(sim, n_filters)):
        if tweak:
            tweak(b, P)
        Ps.append(P)
        datas.append(sim.generate(P, traj_seed=seed, kmax=K))
        seeds.append(1000 + seed)
    return Ps, datas, seeds


def _compare(batch, handles, nP, mixtures):
    """Every filter of the batch against its own handle: sizes, unused masks, ids exactly; weights to 1e-12; mixtures bit for bit."""
    sizes = batch.gm_sizes()
    wb = batch.get_weights()
    masks = batch.get_unused_masks()
    ids, par = batch.get_particle_ids()
    for b, f in enumerate(handles):
        blk = slice(b * nP, (b + 1) * nP)
        np.testing.assert_array_equal(sizes[blk], f.gm_sizes(), err_msg=f"filter {b}: mixture sizes")
        np.testing.assert_array_equal(masks[blk], f.get_unused_masks(), err_msg=f"filter {b}: unused lists")
        hid, hpar = f.get_particle_ids()
        np.testing.assert_array_equal(ids[blk] - b * nP, hid, err_msg=f"filter {b}: ids")
        np.testing.assert_array_equal(par[blk] - b * nP, hpar, err_msg=f"filter {b}: parent ids")
        np.testing.assert_allclose(wb[blk], f.get_weights(), rtol=1e-12, atol=0, err_msg=f"filter {b}: weights")
        if mixtures:
            for i in range(nP):
                for x, y in zip(batch.export_gm(b * nP + i), f.export_gm(i)):
                    np.testing.assert_array_equal(x, y, err_msg=f"filter {b} particle {i}: mixture")


@pytest.mark.gpu
def test_batch_equals_independent_handles_over_whole_trajectories(pkg):
    sim = pkg.sim2d_driver
    nF, nP, K = 6, 200, 301

    def tweak(b, P):
        if b == 2:
            P["use_cluster"] = 1
        if b == 4:
            P["n_eval"] = 1

    Ps, datas, seeds = _setup(sim, nF, K, tweak)
    batch = pkg.FilterBatch(nF, nP, gm_capacity=512)
    handles = [pkg.RBPHDFilter(nP, gm_capacity=512) for _ in range(nF)]
    rb = sim.Sim2dBatchRun(batch, datas, Ps, seeds)
    rh = sim.Sim2dBatchRun(handles, datas, Ps, seeds)
    mixed_empty = 0
    partial_resample_then_predict = 0
    prev_partial = False
    for k in range(1, K):
        fb = rb.step(k)
        fh = rh.step(k)
        np.testing.assert_array_equal(rb.last_n_z, rh.last_n_z)
        np.testing.assert_array_equal(fb, fh, err_msg=f"step {k}: resampling decisions")
        for b in range(nF):
            np.testing.assert_array_equal(rb.last_plans[b], rh.last_plans[b], err_msg=f"step {k} filter {b}: plan")
        if (rb.last_n_z == 0).any() and (rb.last_n_z > 0).any():
            mixed_empty += 1
        if prev_partial:
            partial_resample_then_predict += 1
        prev_partial = bool(fb.any() and not fb.all())
        _compare(batch, handles, nP, mixtures=(k % 10 == 0 or k == K - 1))
    assert mixed_empty > 0, "no cycle had empty and non-empty measurement sets side by side"
    assert partial_resample_then_predict > 0, "no cycle followed one in which only some filters resampled"
    assert (rb.n_resamples > 0).sum() >= 2


@pytest.mark.gpu
def test_batch_of_one_is_bit_identical_to_a_plain_handle(pkg):
    sim = pkg.sim2d_driver
    Ps, datas, seeds = _setup(sim, 1, 160)
    batch = pkg.FilterBatch(1, 64, gm_capacity=256)
    plain = pkg.RBPHDFilter(64, gm_capacity=256)
    assert batch.n_filters_abi() == 1 and batch.n == 64
    rb = sim.Sim2dBatchRun(batch, datas, Ps, seeds)
    rh = sim.Sim2dBatchRun([plain], datas, Ps, seeds)
    for k in range(1, 160):
        rb.step(k)
        rh.step(k)
    np.testing.assert_array_equal(batch.get_weights(), plain.get_weights())
    _compare(batch, [plain], 64, mixtures=True)


@pytest.mark.gpu
def test_batch_of_64_at_capacity_256(pkg):
    sim = pkg.sim2d_driver
    nF, nP, K = 64, 200, 41
    Ps, datas, seeds = _setup(sim, nF, K)
    batch = pkg.FilterBatch(nF, nP, gm_capacity=256)
    rb = sim.Sim2dBatchRun(batch, datas, Ps, seeds)
    rb.run(1, K)
    batch.synchronize()       # raises on a device error word
    sample = [0, 17, 42, 63]
    handles = [pkg.RBPHDFilter(nP, gm_capacity=256) for _ in sample]
    rh = sim.Sim2dBatchRun(handles, [datas[b] for b in sample], [Ps[b] for b in sample], [seeds[b] for b in sample])
    rh.run(1, K)
    sizes, w = batch.gm_sizes(), batch.get_weights()
    for j, b in enumerate(sample):
        blk = slice(b * nP, (b + 1) * nP)
        np.testing.assert_array_equal(sizes[blk], handles[j].gm_sizes())
        np.testing.assert_allclose(w[blk], handles[j].get_weights(), rtol=1e-12, atol=0)
        for i in (0, 77, 199):
            for x, y in zip(batch.export_gm(b * nP + i), handles[j].export_gm(i)):
                np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_batch_refusals(pkg):
    capi = pkg.capi
    with pytest.raises(capi.EngineError) as e:
        pkg.FilterBatch(2, 8, model=capi.MODEL_VICTORIAPARK_3D)
    assert e.value.status == capi.ERR_UNSUPPORTED and "Victoria Park" in str(e.value)
    batch = pkg.FilterBatch(3, 8, gm_capacity=64)
    assert batch.n_filters_abi() == 3
    plain = pkg.RBPHDFilter(8, gm_capacity=64)
    lib = pkg.load_library()
    lib.rfsgpu_n_filters.restype = C.c_int
    assert lib.rfsgpu_n_filters(plain._h) == 1
    # a resampling source outside its filter's block
    plan = np.arange(24, dtype=np.int32)
    plan[9] = 3
    with pytest.raises(capi.EngineError) as e:
        batch.batch_resample_apply(plan, np.array([0, 1, 0]))
    assert e.value.status == capi.ERR_INVALID and "outside" in str(e.value)
    # too many measurements for one filter
    z = np.zeros((3, capi.MAX_Z, 2))
    nz = np.array([1, capi.MAX_Z + 1, 0], dtype=np.int32)
    fn = lib.rfsgpu_batch_cycle_async
    fn.restype = C.c_int
    rc = fn(batch._h, C.c_int(1), None, None, C.c_int(0), z.ctypes.data_as(C.c_void_p), nz.ctypes.data_as(C.c_void_p), C.c_int(1))
    assert rc == capi.ERR_INVALID
    lib.rfsgpu_last_error.restype = C.c_char_p
    assert b"filter 1" in lib.rfsgpu_last_error(batch._h)
    # calls a batch does not take
    vp = capi.VPConfig()
    vp.nPd = 1
    refused = [
        ("set_model_victoriapark", (C.byref(vp),)),
        ("set_laser_scan", (np.zeros(4).ctypes.data_as(C.c_void_p), C.c_int(4))),
        ("update", (z.ctypes.data_as(C.c_void_p), C.c_int(1))),
        ("update_async", (z.ctypes.data_as(C.c_void_p), C.c_int(1))),
        ("update_map", (z.ctypes.data_as(C.c_void_p), C.c_int(1))),
        ("update_io", (C.c_int(1), None, None, C.c_int(0), None, z.ctypes.data_as(C.c_void_p), C.c_int(1), None)),
        ("step_async", (z.ctypes.data_as(C.c_void_p), C.c_int(1), C.c_int(1))),
        ("step_async_deferred", (z.ctypes.data_as(C.c_void_p), C.c_int(1), None, None)),
        ("step_async_trailing", (z.ctypes.data_as(C.c_void_p), C.c_int(1), None, C.c_int(0))),
        ("cycle_async", (C.c_int(1), None, None, C.c_int(0), None, z.ctypes.data_as(C.c_void_p), C.c_int(1), C.c_int(1))),
        ("collective_gate", (None,)),
        ("collective_publish", (None,)),
        ("collective_probe", (None, None)),
        ("fastslam_update", (z.ctypes.data_as(C.c_void_p), C.c_int(1))),
        ("resample_apply", (np.arange(24, dtype=np.int32).ctypes.data_as(C.c_void_p),)),
    ]
    for name, args in refused:
        fn = getattr(lib, "rfsgpu_" + name)
        fn.restype = C.c_int
        rc = fn(batch._h, *args)
        assert rc == capi.ERR_UNSUPPORTED, name
        msg = lib.rfsgpu_last_error(batch._h)
        assert b"filter batch" in msg, (name, msg)
    with pytest.raises(capi.EngineError) as e:
        batch.set_birth_inheritance(capi.INHERIT_EAGER)
    assert e.value.status == capi.ERR_UNSUPPORTED


def _configure_from_scenario(capi, batch, b, P):
    """scenarios.apply_params for filter b of a batch."""
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
    cfg.minUpdatesBeforeResample = P.get("min_updates", 2)
    batch.configure(b, cfg, R=P["R"], Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"],
                    kf=(P["kf_range"], P["kf_bearing"]), Q=P["Q_lm"])


@pytest.mark.gpu
def test_murty_partitions_inside_a_batch(pkg, sc):
    """Two of four filters carry configs[4]'s dense form (10-sigma gate, 40 evaluation points, clutter): partitions above r + c = 8 go
    through Murty-200 in the batch's post kernel.  Each filter equals its own handle."""
    nF, nP = 4, 32
    scens = [sc.make_scenario(nP, 200, 50, seed=701 + b, n_clutter=10, n_eval=40, weighting_md=10.0, weights=(0.8, 1.0)) if b in (0, 2)
             else sc.make_scenario(nP, 40, 12, seed=701 + b) for b in range(nF)]
    batch = pkg.FilterBatch(nF, nP, gm_capacity=448)
    handles = [pkg.RBPHDFilter(nP, gm_capacity=448) for _ in range(nF)]
    poses = np.vstack([s_["poses"] for s_ in scens])
    pcov = [np.asarray(s_["pose_cov"], dtype=np.float64) for s_ in scens]
    assert all(c.size == 9 for c in pcov)
    cov = np.vstack([np.tile(c.ravel(), (nP, 1)) for c in pcov])
    batch.set_poses(poses, cov)
    batch.set_weights(np.concatenate([s_["particle_w"] for s_ in scens]))
    for b, (s_, f) in enumerate(zip(scens, handles)):
        _configure_from_scenario(pkg.capi, batch, b, s_["params"])
        for i in range(nP):
            batch.import_gm(b * nP + i, s_["w"][i], s_["mean"][i], s_["cov"][i])
        sc.load_scenario(f, s_)
        f.set_poses(s_["poses"], np.tile(pcov[b].ravel(), (nP, 1)))
    for cycle in range(2):
        pred = None if cycle == 0 else True
        batch.cycle_async(pred, [s_["Z"] for s_ in scens], normalize=True)
        for s_, f in zip(scens, handles):
            f.cycle_async(pred, s_["Z"], normalize=True)
        _compare(batch, handles, nP, mixtures=True)
    lib = pkg.load_library()
    lib.rfsgpu_murty_seen.restype = C.c_int
    assert lib.rfsgpu_murty_seen(batch._h) == 1, "no Murty-200 job ran in the batch"
    assert lib.rfsgpu_murty_seen(handles[0]._h) == 1 and lib.rfsgpu_murty_seen(handles[1]._h) == 0


@pytest.mark.gpu
def test_batch_against_the_cpu_oracle(pkg, ob, sc):
    """Three filters x 64 particles with different configurations over 60 simulator steps, each against an OracleFilter driven by
    the same per-filter randomness: test_c1_trajectory_device_vs_oracle's tolerances."""
    sim = pkg.sim2d_driver
    nF, nP, K = 3, 64, 61

    def tweak(b, P):
        if b == 1:
            P["use_cluster"] = 1
        if b == 2:
            P["n_eval"] = 5
            P["merge_thr"] = 1.0

    Ps, datas, seeds = _setup(sim, nF, K, tweak)
    batch = pkg.FilterBatch(nF, nP, gm_capacity=256)
    orcs = [ob.OracleFilter(nP) for _ in range(nF)]
    rb = sim.Sim2dBatchRun(batch, datas, Ps, seeds)
    ro = sim.Sim2dBatchRun(orcs, datas, Ps, seeds)
    updates = 0
    for k in range(1, K):
        fb = rb.step(k)
        fo = ro.step(k)
        np.testing.assert_array_equal(fb, fo, err_msg=f"step {k}: resampling decisions")
        sizes, w = batch.gm_sizes(), batch.get_weights()
        for b, o in enumerate(orcs):
            np.testing.assert_array_equal(rb.last_plans[b], ro.last_plans[b])
            blk = slice(b * nP, (b + 1) * nP)
            np.testing.assert_array_equal(sizes[blk], o.gm_sizes(), err_msg=f"step {k} filter {b}")
            np.testing.assert_allclose(w[blk], o.get_weights(), rtol=1e-8, atol=1e-300, err_msg=f"step {k} filter {b}")
            for i in range(0, nP, 7 if k % 10 else 1):
                sc.assert_gm_close(batch.export_gm(b * nP + i), o.export_gm(i), 1e-7, 1e-9)
                assert list(batch.get_unused(b * nP + i)) == list(o.get_unused(i)), (k, b, i)
        updates += int((rb.last_n_z > 0).sum())
    assert updates > nF * K * 0.3



@pytest.mark.gpu
def test_one_filter_batch_run_resamples_where_sim2drun_does(pkg):
    """The resampling gate of Sim2dBatchRun / FilterBatch.update_and_resample counts every cycle as an update, empty scans included
    (RBPHDFilter::update increments nUpdatesSinceResample_ before its empty-set return), and draws as Sim2dRun draws: a one-filter
    batch run on a realisation with empty scans resamples at the same steps, with the same plans, as Sim2dRun on a plain handle."""
    sim = pkg.sim2d_driver
    K, nP, seed = 301, 64, 21
    P = dict(sim.C1_SIM)
    P["Pd"] = 0.5                      # (detections missed often: empty scans between non-empty ones)
    data = sim.generate(P, traj_seed=5, kmax=K)
    empty = [k for k in range(1, K) if len(data["Z"][k]) == 0]
    assert len(empty) > 10
    plain = pkg.RBPHDFilter(nP, gm_capacity=256)
    fired_plain, plans_plain = [], []

    def note(k, run, fired):
        if fired:
            fired_plain.append(k)
            plans_plain.append(None)

    run = sim.Sim2dRun([plain], data, P=P, seed=seed).run(on_step=note)
    batch = pkg.FilterBatch(1, nP, gm_capacity=256)
    rb = sim.Sim2dBatchRun(batch, [data], [P], [seed]).run()
    assert rb.resample_steps[0] == fired_plain
    assert len(fired_plain) >= 3
    # a resampling whose minimum-update gate was met by counting an empty scan
    assert any(any(j in empty for j in range(a + 1, b)) for a, b in zip(fired_plain, fired_plain[1:]))
    np.testing.assert_array_equal(batch.get_particle_ids()[1], plain.get_particle_ids()[1])
    np.testing.assert_array_equal(batch.gm_sizes(), plain.gm_sizes())
    assert run.n_resamples == rb.n_resamples[0]


@pytest.mark.gpu
def test_birth_inheritance_before_the_first_update(pkg):
    """A filter resampled before its first update, with unused masks set by hand: the next predict copies the masks as the handle's
    level-ordered walk does (a lower parent has not emptied its mask yet: its birth step needs a previous update)."""
    nF, nP = 2, 16
    batch = pkg.FilterBatch(nF, nP, gm_capacity=64)
    handles = [pkg.RBPHDFilter(nP, gm_capacity=64) for _ in range(nF)]
    rng = np.random.default_rng(3)
    masks = rng.integers(1, 2 ** 40, size=nF * nP, dtype=np.uint64)
    batch.set_unused_masks(masks)
    for b, f in enumerate(handles):
        f.set_unused_masks(masks[b * nP:(b + 1) * nP])
    plan = np.arange(nP, dtype=np.int32)
    plan[5], plan[9], plan[7], plan[3] = 2, 0, 2, 12       # lower parents (one of them twice) and a higher one
    handles[1].resample_apply(plan)
    gplan = np.arange(nF * nP, dtype=np.int32)
    gplan[nP:] = nP + plan
    batch.batch_resample_apply(gplan, np.array([0, 1]))
    assert list(batch.batch_resample_occured()) == [False, True]
    empty = np.zeros((0, 2))
    for cycle in range(2):                                  # the flag stays up without an update: the walk runs again
        batch.cycle_async(True, [empty, empty], normalize=True)
        for f in handles:
            f.cycle_async(True, empty, normalize=True)
        _compare(batch, handles, nP, mixtures=True)


@pytest.mark.gpu
def test_batch_capacity_error_names_the_filter(pkg, sc):
    """One filter of a batch outgrows gm_capacity: the batch's error (RFSGPU_ERR_CAPACITY) names that filter."""
    nF, nP = 4, 8
    big = sc.make_scenario(nP, 60, 30, seed=801)
    batch = pkg.FilterBatch(nF, nP, gm_capacity=64)
    for b in range(nF):
        _configure_from_scenario(pkg.capi, batch, b, big["params"])
    batch.set_poses(np.vstack([big["poses"]] * nF), np.asarray(big["pose_cov"], dtype=np.float64))
    for b in range(nF):
        for i in range(nP):
            m = 60 if b == 2 else 5
            batch.import_gm(b * nP + i, big["w"][i][:m], big["mean"][i][:m], big["cov"][i][:m])
    batch.cycle_async(None, [big["Z"]] * nF, normalize=True)
    with pytest.raises(pkg.capi.EngineError) as e:
        batch.synchronize()
    assert e.value.status == pkg.capi.ERR_CAPACITY
    assert "filter 2" in str(e.value) and "filter 0" not in str(e.value), str(e.value)
    # cleared: the next cycle within capacity reports nothing
    for i in range(nP):
        batch.import_gm(2 * nP + i, big["w"][i][:5], big["mean"][i][:5], big["cov"][i][:5])
    small = [big["Z"][:3]] * nF
    batch.cycle_async(None, small, normalize=True)
    batch.synchronize()
    # the whole-handle weight calls are refused on a batch
    for call in (lambda: batch.weight_sums(), lambda: batch.normalize_weights(1.0)):
        with pytest.raises(pkg.capi.EngineError) as e:
            call()
        assert e.value.status == pkg.capi.ERR_UNSUPPORTED and "filter batch" in str(e.value)
    lib = pkg.load_library()
    lib.rfsgpu_resample_occured.restype = C.c_int
    assert lib.rfsgpu_resample_occured(batch._h) == -1
