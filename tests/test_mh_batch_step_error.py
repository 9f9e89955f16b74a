"""The [metric] calls on a batch of multi-hypothesis FastSLAM filters (rfsgpu_batch_mh_serve_metrics; the live-count form of
map_metric_kernel, csrc/map_metric.h): filter b's record goes over the global slots [b * max_per_filter, b * max_per_filter + n_b),
n_b read on the device where the kernel runs, and no slot at or beyond n_b is looked at.

The yardstick is tests/test_step_error.py's: tools/analysis2d_sim.py (scipy's assignment) plus plain numpy, fed what live_counts() and
the per-slot getters return for the LIVE slots, with every Gaussian's log-odds w turned into 1 - 1 / (1 + exp(w)) as
test_fastslam_batch.py::test_step_error_on_a_fastslam_batch does.  Tolerance 1e-12 (tests/test_step_error.py's figure; its 1e-13 for the
cardinality); integer fields and status exact.

Two premises are asserted on the yardstick's own inputs before a record is compared, so that no rounding decides an integer field:
every transformed weight of the best particle is at least 1e-9 (planted: 1e-6) away from the threshold 0.75, and the cost matrix has one
optimum up to cells equal to the cutoff (the same matrix under a random row / column permutation through scipy gives the same sum and
the same number of cutoff cells, as tests/test_step_error.py checks its planted cases)."""
import ctypes as C
import inspect
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from conftest import ROOT
from tests.support import mh_batch_reference as mb
from tests.support import mh_device_cycle_reference as ref

THR, CUT, ORD = 0.75, 0.20, 1.0
SIGNATURE = "rfsgpu_filter *f, int on"


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_the_switch_is_declared_exported_and_wrapped(pkg):
    pkg.build_mod.build()
    lib = pkg.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfsgpu.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+rfsgpu_batch_mh_serve_metrics\s*\(([^)]*)\)", txt)
    assert m, "rfsgpu_batch_mh_serve_metrics is not declared"
    assert " ".join(m.group(1).split()) == SIGNATURE
    assert hasattr(lib, "rfsgpu_batch_mh_serve_metrics")
    assert "batch_mh_serve_metrics" in pkg.capi.ABI_SYMBOLS
    assert hasattr(pkg.capi.CBatchMH, "serve_metrics") and hasattr(pkg.MHFastSLAMBatch, "serve_metrics")
    assert inspect.signature(pkg.MHFastSLAMBatch.__init__).parameters["metrics"].default is False
    run = pkg.sim2d_driver.Sim2dMHBatchRun
    p = inspect.signature(run.__init__).parameters
    assert p["track_errors"].default is False and p["device_loop"].default is False
    for meth in ("step", "errors", "synchronize"):
        assert hasattr(run, meth)
    lib.rfsgpu_batch_mh_serve_metrics.restype = C.c_int
    assert lib.rfsgpu_batch_mh_serve_metrics(C.c_void_p(), C.c_int(1)) == pkg.capi.ERR_INVALID


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------

def _tse():
    import test_step_error as tse
    return tse


class _View:
    """An MH batch with log-odds turned into the logged existence probability: what analysis2dSim reads."""

    def __init__(self, batch):
        self.b = batch

    def get_weights(self):
        return self.b.get_weights()

    def get_poses(self):
        return self.b.get_poses()

    def export_gm(self, slot):
        w, wp, mean, cov = self.b.export_gm(slot)
        return 1 - 1 / (1 + np.exp(w)), wp, mean, cov


def _one_optimum(est, truth, c, seed):
    """The premise of comparing e_dist / e_card (module docstring)."""
    from scipy.optimize import linear_sum_assignment
    n = max(len(est), len(truth))
    if n == 0:
        return
    Cm = _tse()._cost_matrix(est, truth, c)
    rng = np.random.default_rng(seed)
    got = []
    for trial in range(2):
        pr, pc = (np.arange(n), np.arange(n)) if trial == 0 else (rng.permutation(n), rng.permutation(n))
        M = Cm[pr][:, pc]
        r, q = linear_sum_assignment(M)
        cells = M[r, q]
        got.append((cells.sum(), int((cells == c).sum())))
    assert got[0][1] == got[1][1] and abs(got[0][0] - got[1][0]) <= 1e-13 * max(got[0][0], 1e-300), got


def _want(a, batch, b, n_live, truth, first_seen, t, gt_pose, margin=1e-9):
    """The yardstick's record of filter b from its first n_live slots, with both premises asserted."""
    tse = _tse()
    view = _View(batch)
    want = tse._host_row(a, view, batch.block(b, n_live), truth, first_seen, t, gt_pose, THR, CUT, ORD)
    pr, _, mean, _ = view.export_gm(int(want["best_slot"]))
    assert pr.size == 0 or np.abs(pr - THR).min() >= margin, "a transformed weight at the threshold"
    seen = np.asarray(truth).reshape(-1, 2)[np.asarray(first_seen) <= t]
    _one_optimum(mean[pr >= THR], seen, CUT, 17 + b)
    return want


def _check_all(a, batch, counts, truths, firsts, ts, gt_pose, rows, what, margin=1e-9):
    tse = _tse()
    wants = []
    for b in range(batch.n_filters):
        want = _want(a, batch, b, int(counts[b]), truths[b], firsts[b], float(ts[b]), gt_pose[b], margin)
        tse._check_row(rows[b], want, "%s: filter %d (%d live)" % (what, b, counts[b]))
        assert rows[b]["t"] == ts[b] and np.isfinite(rows[b]["weight_sum"])
        wants.append(want)
    return wants


def _planted_map(rng, truth, m):
    """m Gaussians near the truth whose log-odds lie on both sides of the threshold, no transformed weight within 1e-3 of it."""
    pr = rng.uniform(0.05, 0.98, m)
    pr[np.abs(pr - THR) < 1e-3] = 0.9
    pr[0], pr[1] = 0.9, 0.3                                   # both sides in every map
    lo = np.log(pr / (1 - pr))
    mean = truth[rng.integers(0, len(truth), m)] + rng.normal(0, 0.03, (m, 2))
    return lo, mean


def _plant(batch, slot, lo, mean):
    batch.import_gm(slot, lo, mean, np.tile(np.eye(2) * 0.01, (len(lo), 1, 1)))


def _poison(rng, w, x, batch, b, n_live, stride):
    """Everything beyond filter b's count: the largest weight of all in the first tail slot, NaN weights after it, poses of 1e300, maps of
    far-away Gaussians that would all pass the threshold."""
    lo = b * stride
    w[lo + n_live] = 50.0
    w[lo + n_live + 1:lo + stride] = np.nan
    x[lo + n_live:lo + stride] = 1e300
    far = np.full(9, 6.0), rng.uniform(1e5, 2e5, (9, 2))
    for s in range(lo + n_live, lo + stride):
        _plant(batch, s, *far)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_per", [1, 63, 64, 65, 200])
def test_count_boundaries_with_poisoned_tails(pkg, n_per):
    """Two filters of n_per live particles in blocks of n_per + 70: the records and the map estimates are those of the live slots."""
    a = _tse()._tool()
    nF, stride = 2, n_per + 70
    rng = np.random.default_rng(500 + n_per)
    B = pkg.MHFastSLAMBatch(nF, n_per, stride, gm_capacity=64, metrics=True)
    w = np.zeros(nF * stride)
    x = np.zeros((nF * stride, 3))
    truths, planted, best = [], {}, []
    for b in range(nF):
        truth = rng.uniform(-3, 3, (9 + b, 2))
        truths.append(truth)
        B.set_ground_truth(truth, None, filter=b)
        live = slice(b * stride, b * stride + n_per)
        w[live] = rng.uniform(0.05, 1.0, n_per)
        x[live] = rng.normal(0, 0.2, (n_per, 3))
        for i in range(n_per):
            planted[b * stride + i] = _planted_map(rng, truth, 6 + (i + b) % 5)
            _plant(B, b * stride + i, *planted[b * stride + i])
        _poison(rng, w, x, B, b, n_per, stride)
        best.append(b * stride + int(np.argmax(w[live])))
    B.set_weights(w)
    B.set_poses(x)
    assert list(B.live_counts()) == [n_per] * nF
    gt_pose = rng.normal(0, 0.1, (nF, 3))
    ts = np.array([0.5, 1.5])
    rows = B.step_error(ts, gt_pose, THR, CUT, ORD)
    firsts = [np.full(len(t), -1.0) for t in truths]
    wants = _check_all(a, B, [n_per] * nF, truths, firsts, ts, gt_pose, rows, "n_per %d" % n_per, margin=1e-6)
    for b in range(nF):
        assert int(rows[b]["best_slot"]) == best[b] == wants[b]["best_slot"]
        lo, mean = planted[best[b]]
        pr = 1 - 1 / (1 + np.exp(lo))
        assert (pr >= THR).any() and (pr < THR).any()
        m, cv, ww = B.get_map_estimate(THR, filter=b)
        assert len(ww) == wants[b]["n_est"] == int((pr >= THR).sum())
        assert np.array_equal(m, mean[pr >= THR]) and np.array_equal(cv, np.tile(np.eye(2) * 0.01, (len(ww), 1, 1)))
        np.testing.assert_allclose(ww, pr[pr >= THR], rtol=1e-13, atol=0)
    B.close()


@pytest.mark.gpu
def test_the_same_tree_as_a_full_block(pkg):
    """One state in a FastSLAMBatch(2, 65) and in the first 65 slots of an MH batch's blocks of 140: every field of the two records has
    the same bits, best_slot apart, which differs by the block offsets."""
    nF, n, stride = 2, 65, 140
    rng = np.random.default_rng(65)
    sim = pkg.sim2d_driver
    full = pkg.FastSLAMBatch(nF, n, gm_capacity=64)
    mh = pkg.MHFastSLAMBatch(nF, n, stride, gm_capacity=64, metrics=True)
    for b in range(nF):
        sim.configure_fastslam_batch_filter(full, b)          # (a FastSLAM batch: log-odds weights)
    wf, xf = rng.uniform(0.05, 1.0, nF * n), rng.normal(0, 0.2, (nF * n, 3))
    wm, xm = np.zeros(nF * stride), np.zeros((nF * stride, 3))
    for b in range(nF):
        truth = rng.uniform(-3, 3, (10, 2))
        for f in (full, mh):
            f.set_ground_truth(truth, None, filter=b)
        wm[b * stride:b * stride + n] = wf[b * n:(b + 1) * n]
        xm[b * stride:b * stride + n] = xf[b * n:(b + 1) * n]
        for i in range(n):
            lo, mean = _planted_map(rng, truth, 6 + i % 5)
            _plant(full, b * n + i, lo, mean)
            _plant(mh, b * stride + i, lo, mean)
        _poison(rng, wm, xm, mh, b, n, stride)
    full.set_weights(wf); full.set_poses(xf)
    mh.set_weights(wm); mh.set_poses(xm)
    gt_pose = rng.normal(0, 0.1, (nF, 3))
    ts = np.array([0.25, 0.75])
    ra, rm = full.step_error(ts, gt_pose, THR, CUT, ORD), mh.step_error(ts, gt_pose, THR, CUT, ORD)
    for b in range(nF):
        for name in ra.dtype.names:
            if name == "best_slot":
                assert int(ra[b][name]) - b * n == int(rm[b][name]) - b * stride == int(np.argmax(wf[b * n:(b + 1) * n]))
            else:
                assert ra[b][name].tobytes() == rm[b][name].tobytes(), (b, name, ra[b][name], rm[b][name])
        assert int(ra[b]["status"]) == 0 and int(ra[b]["n_est"]) > 0 and np.isfinite(ra[b]["pose_ed"])
    full.close()
    mh.close()


def _truths(scens):
    return [np.asarray(s["gt"]).reshape(-1, 2) for s in scens], [np.full(len(s["gt"]), -1.0) for s in scens]


@pytest.mark.gpu
def test_counts_that_cycles_made(pkg, sc):
    """Filters of 3, 2, 1 and 2 hypotheses on crowded and sparse scenes: after a cycle that grows them to different counts, after one
    whose resampling brings a filter back with the larger set's data beyond its count, and after one in which a filter has no
    measurements, every record equals the yardstick on live_counts() and the getters."""
    a = _tse()._tool()
    n, stride = 8, 32
    scens = [ref.crowded(sc, n), ref.sparse(sc, n), ref.crowded(sc, n, seed=114), ref.crowded(sc, n, seed=115)]
    rig = mb.Rig(pkg, sc, scens, [3, 2, 1, 2], [50.0] * 4, n, stride)
    B = rig.batch
    B.serve_metrics(True)
    truths, firsts = _truths(scens)
    for b in range(4):
        B.set_ground_truth(truths[b], firsts[b], filter=b)
    rng = np.random.default_rng(3)
    gt_pose = rng.normal(0, 0.05, (4, 3))
    ts = np.arange(4) * 0.1

    def check(what):
        rows = B.step_error(ts, gt_pose, THR, CUT, ORD)
        counts = B.live_counts()
        _check_all(a, B, counts, truths, firsts, ts, gt_pose, rows, what)
        return rows, counts

    rows, counts = check("before any cycle")
    assert list(counts) == [n] * 4
    # 1: the gates shut, the sets grow
    def shut(b, c):
        c.minUpdatesBeforeResample = mb.NEVER
        c.nParticlesMax = stride
    rig.each_config(shut)
    Zs = [s["Z"] for s in scens]
    rig.cycle(Zs, [0.25] * 4, handles=False)
    rows, counts = check("after the growing cycle")
    print("counts after the growing cycle", counts, "n_est", rows["n_est"])
    assert list(counts) == [24, 8, 8, 16]
    assert (rows["n_est"] > 0).any()
    sizes_grown = np.asarray(B.gm_sizes()).copy()
    # 2: one hypothesis from now on; filter 0 resamples (N_eff threshold above any count) and shrinks back to 8
    def open_(b, c):
        c.maxNDataAssocHypotheses = 1
        c.minUpdatesBeforeResample = 0 if b == 0 else mb.NEVER
    rig.each_config(open_)
    rig.set_resampling(0, 1e9, 0.0)
    rz = np.random.default_rng(5)
    Zs2 = [s["Z"] + rz.normal(0, 3e-3, s["Z"].shape) for s in scens]
    rig.cycle(Zs2, [0.6] * 4, handles=False)
    rows, counts = check("after the resampling cycle")
    lc = B.last_cycle()
    assert list(counts) == [8, 8, 8, 16] and list(lc["fired"]) == [True, False, False, False]
    stale = np.asarray(B.gm_sizes())[B.block(0)][8:24]
    assert (stale > 0).all() and (sizes_grown[B.block(0)][8:24] > 0).all()      # the larger set's maps sit beyond the count
    assert (B.get_weights()[B.block(0, 8)] == 1.0).all() and int(rows[0]["best_slot"]) == 0 and rows[0]["weight_sum"] == 8.0
    # 3: no measurements for filter 1
    Zs3 = [s["Z"] + rz.normal(0, 3e-3, s["Z"].shape) for s in scens]
    Zs3[1] = np.zeros((0, 2))
    before1 = B.get_weights()[B.block(1, 8)].copy()
    rig.cycle(Zs3, [0.4] * 4, handles=False)
    rows, counts = check("after a cycle without measurements for filter 1")
    assert np.array_equal(B.get_weights()[B.block(1, 8)], before1)
    rig.close()


@pytest.mark.gpu
def test_an_overflowed_filter_is_evaluated_on_its_state_before_the_cycle(pkg, sc):
    """3 filters x 4 in blocks of 15, 4 hypotheses: crowded filter 1 would need 16.  step_error_async behind the cycle enqueues; the first
    synchronising call reports filter 1 once; the logged row holds filter 1 as it was and the others as their cycles left them."""
    a = _tse()._tool()
    n, stride = 4, 15
    scens = [ref.sparse(sc, n), ref.crowded(sc, n), ref.sparse(sc, n, seed=202)]
    rig = mb.Rig(pkg, sc, scens, [4, 4, 4], [50.0] * 3, n, stride)

    def shut(b, c):
        c.minUpdatesBeforeResample = mb.NEVER
        c.nParticlesMax = stride
    rig.each_config(shut)
    B = rig.batch
    B.serve_metrics(True)
    truths, firsts = _truths(scens)
    for b in range(3):
        B.set_ground_truth(truths[b], firsts[b], filter=b)
    B.error_log_create(2)
    rng = np.random.default_rng(4)
    w = np.ones(3 * stride)
    for b in range(3):
        w[b * stride:b * stride + n] = rng.uniform(0.2, 1.0, n)      # (distinct weights: the selection is not slot 0 by default)
    B.set_weights(w)
    gt_pose = rng.normal(0, 0.05, (3, 3))
    ts = np.array([0.1, 0.2, 0.3])
    before = _want(a, B, 1, n, truths[1], firsts[1], ts[1], gt_pose[1])
    Zs = [s["Z"] for s in scens]
    B.cycle_async(False, Zs, [0.5] * 3)
    B.step_error_async(ts, gt_pose, THR, CUT, ORD)                    # enqueues although filter 1 has overflowed
    with pytest.raises(pkg.capi.EngineError) as e:
        B.error_log_read()
    assert e.value.status == pkg.capi.ERR_CAPACITY and "filter 1" in str(e.value), str(e.value)
    rows = B.error_log_read()                                         # reported once
    B.synchronize()
    assert rows.shape == (1, 3)
    lc = B.last_cycle()
    assert list(lc["overflowed"]) == [False, True, False] and list(B.live_counts()) == [4, 4, 4]
    tse = _tse()
    tse._check_row(rows[0, 1], before, "the overflowed filter, on its state before the cycle")
    for b in (0, 2):
        want = _want(a, B, b, n, truths[b], firsts[b], ts[b], gt_pose[b])
        tse._check_row(rows[0, b], want, "filter %d beside the overflowed one" % b)
    rig.close()


def _sim_params(drv):
    t = ET.parse(os.path.join(ROOT, "tests", "golden", "mhfastslam2dSim_c1.xml")).getroot()
    return dict(drv.C1_FASTSLAM_SIM, max_hypotheses=int(t.find("filter/update/maxNDataAssocHypotheses").text),
                max_loglik_diff=float(t.find("filter/update/maxDataAssocLogLikelihoodDiff").text),
                min_log_likelihood=float(t.find("filter/weighting/minLogMeasurementLikelihood").text),
                existence_prune_thr=float(t.find("filter/prune/threshold").text),
                eff_n=float(t.find("filter/resampling/effNParticle").text), min_updates=int(t.find("filter/resampling/minTimesteps").text))


def _end_state(B):
    counts = B.live_counts()
    ids, pids = B.get_particle_ids()
    w, x, sizes = B.get_weights(), B.get_poses(), np.asarray(B.gm_sizes())
    out = [counts.tobytes()]
    for b in range(B.n_filters):
        blk = B.block(b, counts[b])
        out += [w[blk].tobytes(), x[blk].tobytes(), sizes[blk].tobytes(), np.asarray(ids)[blk].tobytes(), np.asarray(pids)[blk].tobytes()]
        for s in range(blk.start, blk.stop):
            out += [np.asarray(v).tobytes() for v in B.export_gm(s)]
    return out


@pytest.mark.gpu
def test_device_loop_with_nothing_read_back(pkg):
    """Three filters (different Pd, clutter and hypothesis limits) x 16 particles in blocks of 144, 40 simulator steps on the device
    loop with tracking, one read at the end; the same run without tracking, the yardstick evaluated after every step: every logged row
    agrees, and the two runs end with the same bits."""
    a = _tse()._tool()
    drv = pkg.sim2d_driver
    nF, n, stride, K = 3, 16, 16 * 9, 41
    P0 = _sim_params(drv)
    Ps = [dict(P0, Pd=pd, clutter=cl, max_hypotheses=h) for pd, cl, h in ((0.99, 1e-4, 3), (0.9, 5e-3, 2), (0.7, 1e-3, 1))]
    datas = [drv.generate(P, traj_seed=3 + b, kmax=K) for b, P in enumerate(Ps)]
    firsts = [drv.first_seen_times(d, P) for d, P in zip(datas, Ps)]
    seeds = [41, 42, 43]
    tracked = pkg.MHFastSLAMBatch(nF, n, stride, gm_capacity=64)
    run = drv.Sim2dMHBatchRun(tracked, datas, Ps, seeds, n, device_loop=True, track_errors=True)
    run.run(1, K)                                                     # nothing between the steps reads or waits
    log = run.errors()
    assert log.shape == (K - 1, nF) and (log["status"] == 0).all()
    plain = pkg.MHFastSLAMBatch(nF, n, stride, gm_capacity=64)
    run2 = drv.Sim2dMHBatchRun(plain, datas, Ps, seeds, n, device_loop=True)
    seen_counts = set()
    for k in range(1, K):
        run2.step(k)
        counts = plain.live_counts()
        seen_counts.update(counts.tolist())
        ts = np.array([k * P["dt"] for P in Ps])
        gts = np.array([d["gt"][k] for d in datas])
        _check_all(a, plain, counts, [d["landmarks"] for d in datas], firsts, ts, gts, log[k - 1], "step %d" % k)
    print("live counts met over the run:", sorted(seen_counts), " final n_est", log["n_est"][-1], "n_truth", log["n_truth"][-1])
    assert len(seen_counts) >= 2 and (log["n_truth"][-1] > 0).all() and (log["n_est"] > 0).any()
    assert _end_state(tracked) == _end_state(plain)
    tracked.close()
    plain.close()


@pytest.mark.gpu
def test_switch_and_refusals(pkg):
    U, CAP = pkg.capi.ERR_UNSUPPORTED, pkg.capi.ERR_CAPACITY
    lib = pkg.load_library()
    lib.rfsgpu_batch_mh_serve_metrics.restype = C.c_int
    # the switch is a multi-hypothesis batch's alone
    others = [pkg.FilterBatch(2, 4, gm_capacity=64), pkg.FastSLAMBatch(2, 4, gm_capacity=64), pkg.RBPHDFilter(8, gm_capacity=64)]
    pkg.sim2d_driver.configure_fastslam_batch_filter(others[1], 0)
    for f in others:
        for on in (1, 0):
            assert lib.rfsgpu_batch_mh_serve_metrics(f._h, C.c_int(on)) == U
            lib.rfsgpu_last_error.restype = C.c_char_p
            assert b"rfsgpu_create_batch_mh" in lib.rfsgpu_last_error(f._h)
        f.close()
    n, stride = 4, 12
    B = pkg.MHFastSLAMBatch(2, n, stride, gm_capacity=64)
    truth = np.random.default_rng(1).uniform(0, 3, (5, 2))
    metric_calls = {
        "set_ground_truth": lambda: B.set_ground_truth(truth),
        "error_log_create": lambda: B.error_log_create(2),
        "error_log_reset": lambda: B.error_log_reset(),
        "step_error_async": lambda: B.step_error_async(np.zeros(2), np.zeros((2, 3))),
        "error_log_read": lambda: B.error_log_read(),
        "step_error": lambda: B.step_error(np.zeros(2), np.zeros((2, 3))),
        "get_map_estimate": lambda: B.get_map_estimate(),
    }

    def refused():
        for name, call in metric_calls.items():
            with pytest.raises(pkg.capi.EngineError) as e:
                call()
            assert e.value.status == U and "multi-hypothesis" in str(e.value), (name, str(e.value))

    refused()                                                         # off at creation
    B.serve_metrics(True)
    with pytest.raises(pkg.capi.EngineError) as e:                    # what assumes full blocks stays refused
        B.batch_weight_sums()
    assert e.value.status == U and "multi-hypothesis" in str(e.value)
    B.set_ground_truth(truth, filter=0)
    for s in range(n):
        B.import_gm(s, np.full(3, 2.0), truth[:3] + 0.01, np.tile(np.eye(2) * 0.01, (3, 1, 1)))
    with pytest.raises(pkg.capi.EngineError) as e:                    # no log yet
        B.step_error_async(0.0)
    assert e.value.status == CAP
    B.error_log_create(2)
    assert B.error_log_read().shape == (0, 2)
    B.step_error_async(0.1)
    B.step_error_async(0.2)
    with pytest.raises(pkg.capi.EngineError) as e:                    # full
        B.step_error_async(0.3)
    assert e.value.status == CAP and "full" in str(e.value)
    rows = B.error_log_read()
    assert rows.shape == (2, 2) and np.array_equal(rows["t"][:, 0], [0.1, 0.2]) and int(rows[0, 0]["n_est"]) == 3 and int(rows[0, 1]["n_truth"]) == 0
    B.error_log_reset()
    assert B.error_log_read().shape == (0, 2)
    B.step_error_async(0.7)
    assert B.error_log_read()["t"][0, 0] == 0.7
    m, cv, w = B.get_map_estimate(THR, filter=0)
    assert len(w) == 3 and np.allclose(w, 1 - 1 / (1 + np.exp(2.0)), rtol=1e-13)
    B.serve_metrics(False)
    refused()                                                         # and back, with the wording they had
    B.close()
