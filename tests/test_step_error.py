"""Per-step map error and pose error on the device (include/rfsgpu.h [metric], csrc/map_metric.h): one launch gives, per filter, what
the reference's analysis2dSim writes per time step -- the weighted-mean pose error of the particle set and the OSPA / COLA error of the
highest-weight particle's map against the observable ground truth -- into a device-side log.

The yardstick is never the code under test: tools/analysis2d_sim.py::ospa / cola (scipy's linear_sum_assignment: the optimum the
reference's Hungarian method finds) plus plain numpy for the selection and the pose error, on data read back with the calls that
existed before (get_weights, get_poses, export_gm).

Why order 2 and the e_dist / e_card split can be compared at all: the assignment minimises sum C (order 1, OSPA.hpp:167-171), and a
solver may return any optimum.  The planted inputs are continuous random draws, so two perfect matchings that differ in their cells
below c have different sums: the optimum is unique up to permuting cells that all equal c, and sum C^p and the number of c cells do not
depend on which optimum comes out.  test_planted_cases_have_one_optimum_up_to_c_cells checks exactly that premise on every generated
case (the same cost matrix under a random row / column permutation through scipy gives the same sum C, sum C^2 and c-cell count); a
case that failed it would be dropped from the generator by seed, not given a wider tolerance (none had to be)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT

METRIC_SYMBOLS = ["rfsgpu_set_ground_truth", "rfsgpu_error_log_create", "rfsgpu_error_log_reset", "rfsgpu_step_error_async", "rfsgpu_error_log_read",
                  "rfsgpu_step_error", "rfsgpu_get_map_estimate"]
RECORD_FIELDS = ["t", "status", "best_slot", "n_est", "n_truth", "cardinality", "ospa", "cola", "e_dist", "e_card", "pose_ex", "pose_ey", "pose_eth",
                 "pose_ed", "weight_sum"]
CUTOFFS, ORDERS = (0.2, 0.5, 1.0), (1.0, 2.0)
SPECIAL = (0, 1, 63, 64, 65, 200, 511, 512)
W_THR = 0.75
CAP = 576          # gm_capacity of the planted-set handles: 512 estimates + the Gaussians below the threshold


def _tool():
    spec = importlib.util.spec_from_file_location("analysis2d_sim", os.path.join(ROOT, "tools", "analysis2d_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------

def _cost_matrix(est, truth, c):
    """The padded square of tools/analysis2d_sim.py::ospa (OSPA.hpp:132-158)."""
    n1, n2 = len(est), len(truth)
    n = max(n1, n2)
    Cm = np.full((n, n), float(c))
    if n1 and n2:
        d = np.linalg.norm(np.asarray(est)[:, None, :] - np.asarray(truth)[None, :, :], axis=2)
        Cm[:n1, :n2] = np.minimum(d, c)
    return Cm


def _yardstick(a, est, truth, c, p):
    """(ospa, cola, e_dist, e_card): the first two are the tool's own functions, the split comes from scipy's assignment on the tool's matrix."""
    from scipy.optimize import linear_sum_assignment
    o, n = a.ospa(est, truth, c, p)
    co = a.cola(est, truth, c, p) if n else 0.0
    if n == 0:
        return 0.0, 0.0, 0.0, 0.0
    Cm = _cost_matrix(est, truth, c)
    r, q = linear_sum_assignment(Cm)
    cells = Cm[r, q]
    return o, co, float(cells[cells != c].sum()), float(cells[cells == c].sum())


def _close(got, want, rtol, what):
    got, want = float(got), float(want)
    if want == 0.0:
        assert abs(got) <= 1e-15, f"{what}: {got!r} against 0"
    else:
        assert abs(got - want) <= rtol * abs(want), f"{what}: {got!r} against {want!r} (rel {abs(got - want) / abs(want):.3e})"


# ---- planted sets ------------------------------------------------------------------------------------------------------------------

def _sizes():
    """(n_est, n_truth) of every planted case: all pairs of the special sizes, then pairs drawn from 0 ... 80."""
    rng = np.random.default_rng(2024)
    pairs = [(a, b) for a in SPECIAL for b in SPECIAL]
    pairs += [(int(rng.integers(0, 81)), int(rng.integers(0, 81))) for _ in range(24)]
    return pairs


DROPPED_SEEDS = ()     # cases whose optimum is not unique up to c cells (none)


def _planted(seed, n_est, n_truth):
    """Truth: uniform in a square whose side grows with sqrt(n) (neighbours 0.3 ... 1 apart, the scale of the cutoffs).  Estimate: a
    jittered subset of the truth (sigma 0.08: most within every cutoff, some beyond 0.2) plus strays drawn over the same square, in a
    random order; `extra` Gaussians below the weight threshold are interleaved.  Returns (truth [n_truth, 2], w, mean of the mixture)."""
    rng = np.random.default_rng(seed)
    side = 0.6 * max(1.0, np.sqrt(max(n_est, n_truth)))
    truth = rng.uniform(0, side, (n_truth, 2))
    k = int(rng.integers(0, min(n_est, n_truth) + 1)) if min(n_est, n_truth) else 0
    if min(n_est, n_truth) >= 63:
        k = max(k, min(n_est, n_truth) - int(rng.integers(0, 12)))        # large cases: mostly matched, as a converged map is
    sub = rng.permutation(n_truth)[:k]
    est = np.vstack([truth[sub] + 0.08 * rng.standard_normal((k, 2)), rng.uniform(0, side, (n_est - k, 2))])
    est = est[rng.permutation(n_est)] if n_est else est.reshape(0, 2)
    extra = int(rng.integers(0, min(40, CAP - n_est) + 1))
    w = np.concatenate([rng.uniform(W_THR, 1.5, n_est), rng.uniform(0.01, W_THR * 0.99, extra)])
    mean = np.vstack([est, rng.uniform(0, side, (extra, 2))])
    order = rng.permutation(n_est + extra)
    return truth, w[order], mean[order]


def _cases():
    return [(1000 + i, a, b) for i, (a, b) in enumerate(_sizes()) if 1000 + i not in DROPPED_SEEDS]


def test_planted_cases_have_one_optimum_up_to_c_cells():
    """The premise of the order-2 and e_dist / e_card comparisons (module docstring), on every generated case."""
    from scipy.optimize import linear_sum_assignment
    for seed, n_est, n_truth in _cases():
        truth, w, mean = _planted(seed, n_est, n_truth)
        est = mean[w >= W_THR]
        assert len(est) == n_est and len(truth) == n_truth
        n = max(n_est, n_truth)
        if n == 0:
            continue
        rng = np.random.default_rng(seed + 7)
        for c in CUTOFFS:
            Cm = _cost_matrix(est, truth, c)
            ref = None
            for trial in range(2):
                pr, pc = (np.arange(n), np.arange(n)) if trial == 0 else (rng.permutation(n), rng.permutation(n))
                M = Cm[pr][:, pc]
                r, q = linear_sum_assignment(M)
                cells = M[r, q]
                got = (cells.sum(), (cells ** 2).sum(), int((cells == c).sum()))
                if ref is None:
                    ref = got
                else:
                    assert got[2] == ref[2], (seed, c, got, ref)
                    assert abs(got[0] - ref[0]) <= 1e-13 * max(ref[0], 1e-300) and abs(got[1] - ref[1]) <= 1e-13 * max(ref[1], 1e-300), (seed, c, got, ref)


# ---- not GPU: layout, header, first_seen_times -----------------------------------------------------------------------------------------

def test_step_error_struct_matches_the_header(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    m = re.search(r"struct rfsgpu_step_error \{(.*?)\n\};", txt, flags=re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        mm = re.match(r"(double|long long)\s+(.*)$", decl, flags=re.S)
        assert mm is not None, decl                       # every field 8 bytes wide
        fields += [(nm.strip(), mm.group(1)) for nm in mm.group(2).split(",")]
    assert [n for n, _ in fields] == RECORD_FIELDS
    S = pkg.capi.StepError
    assert [n for n, _ in S._fields_] == RECORD_FIELDS
    assert C.sizeof(S) == 8 * len(RECORD_FIELDS) == 120
    for k, (name, ctype) in enumerate(fields):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8
        assert dict(S._fields_)[name] is (C.c_double if ctype == "double" else C.c_longlong)
    dt = pkg.capi.STEP_ERROR_DTYPE
    assert dt.itemsize == 120 and list(dt.names) == RECORD_FIELDS
    for k, (name, ctype) in enumerate(fields):
        assert dt.fields[name][1] == 8 * k and dt.fields[name][0] == (np.float64 if ctype == "double" else np.int64)
    assert int(re.search(r"#define RFSGPU_MAX_METRIC_SET (\d+)", txt).group(1)) == 512 == pkg.capi.MAX_METRIC_SET


def test_header_declares_the_metric_section_outside_the_stable_core(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    names = {w for line in re.findall(r"RFSGPU_CORE(?:_MULTI)?:(.*)", txt) for w in line.split()}
    sec = txt.index("---- [metric]")
    for s in METRIC_SYMBOLS:
        assert s not in names, s
        assert re.search(r"\b" + s + r"\b", core.split("Everything else is OPTIONAL")[0]) is None, s
        assert txt.index(s + "(") > sec, s
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in METRIC_SYMBOLS:
        assert hasattr(lib, s), s


def test_first_seen_times_against_a_loop_and_generate_is_untouched(pkg):
    sim = pkg.sim2d_driver
    P = sim.C1_SIM
    before = sim.generate(P, traj_seed=3, kmax=400)
    fs = sim.first_seen_times(before, P)
    after = sim.generate(P, traj_seed=3, kmax=400)
    for key in ("gt", "odom", "landmarks"):
        assert np.array_equal(before[key], after[key]), key
    assert len(before["Z"]) == len(after["Z"]) and all(np.array_equal(x, y) for x, y in zip(before["Z"], after["Z"]))
    gt, lm = before["gt"], before["landmarks"]
    want = np.full(len(lm), -1.0)
    for m in range(len(lm)):
        for k in range(1, before["K"]):
            r = np.hypot(lm[m, 0] - gt[k, 0], lm[m, 1] - gt[k, 1])
            if P["rmin"] <= r <= P["rmax"]:
                want[m] = k * P["dt"]
                break
    assert fs.shape == want.shape and np.array_equal(fs, want)
    assert (fs >= 0).any()
    # never in range -> -1; in range from step 1 (step 0 does not count, as in the reference's loop); too close until step 3
    toy = dict(gt=np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [1.0, 0.0, 0.0]]), K=4,
               landmarks=np.array([[100.0, 100.0], [1.0, 0.0], [-0.2, 0.0]]))
    assert np.array_equal(sim.first_seen_times(toy, P), [-1.0, 1 * P["dt"], 3 * P["dt"]])
    assert sim.first_seen_times(dict(gt=toy["gt"], K=4, landmarks=np.zeros((0, 2))), P).shape == (0,)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

def _host_row(a, f, blk, truth, first_seen, t, gt_pose, w_thr, c, p):
    """The yardstick's record for one filter from get_weights / get_poses / export_gm (analysis2dSim.cpp:150-249, tools/analysis2d_sim.py)."""
    w = f.get_weights()[blk]
    x = f.get_poses()[blk]
    best, w_hi = 0, 0.0
    for i, wi in enumerate(w):                                         # :159-167
        if wi > w_hi:
            best, w_hi = i, wi
    slot = blk.start + best
    gw, _, gmean, _ = f.export_gm(slot)
    est = gmean[gw >= w_thr]
    seen = np.asarray(truth).reshape(-1, 2)[np.asarray(first_seen) <= t]
    o, co, ed, ec = _yardstick(a, est, seen, c, p)
    row = dict(best_slot=slot, n_est=len(est), n_truth=len(seen), cardinality=float(gw.sum()), ospa=o, cola=co, e_dist=ed, e_card=ec,
               weight_sum=float(w.sum()))
    if gt_pose is not None:
        ws = w.sum() if w.sum() != 0 else np.nan                      # (all weights zero: the means are 0 / 0)
        ex, ey, er = x[:, 0] - gt_pose[0], x[:, 1] - gt_pose[1], a.wrap(x[:, 2] - gt_pose[2])
        row.update(pose_ex=(ex * w).sum() / ws, pose_ey=(ey * w).sum() / ws, pose_eth=(er * w).sum() / ws, pose_ed=(np.hypot(ex, ey) * w).sum() / ws)
    return row


def _check_row(got, want, what, rtol=1e-12):
    assert int(got["status"]) == 0, what
    for k in ("best_slot", "n_est", "n_truth"):
        assert int(got[k]) == int(want[k]), f"{what}: {k} {int(got[k])} against {int(want[k])}"
    _close(got["cardinality"], want["cardinality"], 1e-13, what + ": cardinality")
    for k in ("ospa", "cola", "e_dist", "e_card", "weight_sum", "pose_ex", "pose_ey", "pose_eth", "pose_ed"):
        if k in want:
            _close(got[k], want[k], rtol, what + ": " + k)


def _plant(f, slot, w, mean):
    f.import_gm(slot, w, mean, np.tile(np.eye(2) * 0.01, (len(w), 1, 1)))


@pytest.mark.gpu
def test_metric_on_planted_sets(pkg):
    a = _tool()
    f = pkg.RBPHDFilter(8, gm_capacity=CAP)
    wp = np.array([0.1, 0.2, 0.05, 0.4, 0.1, 0.05, 0.05, 0.05])       # slot 3 is the highest-weight particle
    f.set_weights(wp)
    rng = np.random.default_rng(5)
    for i in range(8):                                                 # the other particles hold maps that must not be looked at
        k = int(rng.integers(1, 30))
        _plant(f, i, rng.uniform(0.8, 1.2, k), rng.uniform(0, 5, (k, 2)))
    worst = 0.0
    for seed, n_est, n_truth in _cases():
        truth, w, mean = _planted(seed, n_est, n_truth)
        _plant(f, 3, w, mean)
        f.set_ground_truth(truth)
        for c in CUTOFFS:
            for p in ORDERS:
                got = f.step_error(0.0, None, W_THR, c, p)[0]
                want = _host_row(a, f, slice(0, 8), truth, np.full(n_truth, -1.0), 0.0, None, W_THR, c, p)
                assert want["best_slot"] == 3 and want["n_est"] == n_est and want["n_truth"] == n_truth
                what = f"seed {seed} n_est {n_est} n_truth {n_truth} c {c} p {p}"
                for k in ("ospa", "cola", "e_dist", "e_card"):
                    if want[k]:
                        worst = max(worst, abs(float(got[k]) - want[k]) / abs(want[k]))
                _check_row(got, want, what)
                assert np.isnan(got["pose_ex"]) and np.isnan(got["pose_ed"])      # no gt_pose given
    print(f"planted sets: largest relative deviation of ospa / cola / e_dist / e_card {worst:.3e}")
    # the closed-form cases of test_cpp_host_driver_map_quality_ospa
    gt = np.random.default_rng(9).uniform(0, 10, (50, 2))
    f.set_ground_truth(gt)
    ones = np.ones(50)
    _plant(f, 3, ones, gt)
    r = f.step_error(0.0, None, 0.5, 0.5, 1.0)[0]
    assert r["ospa"] == 0.0 and r["cola"] == 0.0 and r["e_dist"] == 0.0 and r["e_card"] == 0.0 and r["n_est"] == 50
    _plant(f, 3, ones[:48], gt[:48])
    r = f.step_error(0.0, None, 0.5, 0.5, 1.0)[0]
    assert abs(r["ospa"] - 2 * 0.5 / 50) < 1e-12 and abs(r["e_card"] - 1.0) < 1e-12 and r["e_dist"] == 0.0
    _plant(f, 3, ones, gt + 0.03)
    r = f.step_error(0.0, None, 0.5, 0.5, 2.0)[0]
    assert abs(r["ospa"] - 0.03 * np.sqrt(2)) < 1e-9
    # the estimate as the host gets it
    truth, w, mean = _planted(1003, 65, 64)
    _plant(f, 3, w, mean)
    m, cv, ww = f.get_map_estimate(W_THR)
    assert np.array_equal(ww, w[w >= W_THR]) and np.array_equal(m, mean[w >= W_THR]) and np.array_equal(cv, np.tile(np.eye(2) * 0.01, (65, 1, 1)))
    f.close()


@pytest.mark.gpu
def test_limit_is_loud_and_local(pkg):
    a = _tool()
    nP = 4
    batch = pkg.FilterBatch(3, nP, gm_capacity=CAP)
    rng = np.random.default_rng(12)
    truths = []
    for b, n_est in enumerate((40, 513, 512)):
        truth = rng.uniform(0, 12, (60, 2))
        truths.append(truth)
        batch.set_ground_truth(truth, filter=b)
        est = np.vstack([truth[:30] + 0.05 * rng.standard_normal((30, 2)), rng.uniform(0, 12, (n_est - 30, 2))])
        _plant(batch, b * nP + 1, rng.uniform(0.8, 1.3, n_est), est)
    w = np.full(3 * nP, 0.1)
    w[1::nP] = 0.7
    batch.set_weights(w)
    rows = batch.step_error(np.zeros(3), None, W_THR, 0.5, 1.0)
    assert int(rows[1]["status"]) == 1 and int(rows[1]["n_est"]) == 513 and int(rows[1]["best_slot"]) == nP + 1
    for k in ("ospa", "cola", "e_dist", "e_card"):
        assert np.isnan(rows[1][k]), k
    for b in (0, 2):
        want = _host_row(a, batch, batch.block(b), truths[b], np.full(60, -1.0), 0.0, None, W_THR, 0.5, 1.0)
        _check_row(rows[b], want, f"filter {b} beside an over-limit filter")
    with pytest.raises(pkg.capi.EngineError) as e:
        batch.set_ground_truth(rng.uniform(0, 1, (513, 2)), filter=0)
    assert e.value.status == pkg.capi.ERR_INVALID
    batch.set_ground_truth(rng.uniform(0, 1, (512, 2)), filter=0)      # the limit itself is served
    assert int(batch.step_error(np.zeros(3), None, W_THR, 0.5, 1.0)[0]["n_truth"]) == 512
    batch.close()


@pytest.mark.gpu
def test_selection_and_pose_error(pkg):
    a = _tool()
    nP = 200
    rng = np.random.default_rng(21)
    f = pkg.RBPHDFilter(nP, gm_capacity=64)
    batch = pkg.FilterBatch(3, nP, gm_capacity=64)
    truth = rng.uniform(0, 5, (10, 2))
    seen = np.array([-1, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0])
    f.set_ground_truth(truth, seen)
    for b in range(3):
        batch.set_ground_truth(truth, seen, filter=b)
    for i in range(nP):                                                 # every particle its own small map
        k = 3 + i % 5
        _plant(f, i, rng.uniform(0.5, 1.2, k), truth[:k] + 0.02 * rng.standard_normal((k, 2)))
    for s in range(3 * nP):
        k = 3 + s % 4
        _plant(batch, s, rng.uniform(0.5, 1.2, k), truth[:k] + 0.02 * rng.standard_normal((k, 2)))
    gt_pose = np.array([1.0, -2.0, np.pi - 0.05])
    # poses around the ground truth, bearings on both sides of +-pi (theta - rtheta beyond +-pi needs the one correction)
    x = np.column_stack([gt_pose[0] + 0.1 * rng.standard_normal(nP), gt_pose[1] + 0.1 * rng.standard_normal(nP),
                         np.where(rng.random(nP) < 0.5, np.pi - rng.uniform(0, 0.2, nP), -np.pi + rng.uniform(0, 0.2, nP))])
    t = 2.2
    cases = {}
    w = rng.uniform(0.1, 1.0, nP)
    w[[17, 150]] = 2.0                                                  # ties at the maximum: the first wins
    cases["ties"] = (w, 17)
    w = rng.uniform(0.1, 1.0, nP)
    w[199] = 3.0
    cases["last"] = (w, 199)
    cases["zero"] = (np.zeros(nP), 0)                                   # no weight > 0: slot 0
    for name, (w, best) in cases.items():
        f.set_weights(w)
        f.set_poses(x)
        got = f.step_error(t, gt_pose[None, :], W_THR, 0.2, 1.0)[0]
        assert int(got["best_slot"]) == best, name
        want = _host_row(a, f, slice(0, nP), truth, seen, t, gt_pose, W_THR, 0.2, 1.0)
        assert int(got["n_truth"]) == 6
        if name == "zero":                                              # the weighted means are 0 / 0
            assert all(np.isnan(got[k]) for k in ("pose_ex", "pose_ey", "pose_eth", "pose_ed")) and got["weight_sum"] == 0.0
            want = {k: v for k, v in want.items() if not k.startswith("pose_")}
        _check_row(got, want, name)
        assert abs(want.get("pose_eth", 0.0)) < 0.3                     # (wrapped: without the correction it would be near +-2 pi for half the set)
    # after a resampling all weights are 1: slot 0 of the block
    f.set_weights(cases["ties"][0] / cases["ties"][0].sum())
    plan = pkg.engine.systematic_resample_plan(f.get_weights(), 0.37)
    f.resample_apply(plan)
    got = f.step_error(t, gt_pose[None, :], W_THR, 0.2, 1.0)[0]
    assert int(got["best_slot"]) == 0 and got["weight_sum"] == nP
    _check_row(got, _host_row(a, f, slice(0, nP), truth, seen, t, gt_pose, W_THR, 0.2, 1.0), "after resampling")
    # a batch: the selection is per block, best_slot is global; each filter has its own pose and time
    wb = rng.uniform(0.1, 1.0, 3 * nP)
    wb[[nP + 5, nP + 90]] = 5.0
    wb[2 * nP:] = 0.0
    batch.set_weights(wb)
    xb = np.vstack([x, x[::-1], x])
    batch.set_poses(xb)
    ts = np.array([0.2, 1.7, 9.0])
    gts = np.array([gt_pose, [1.1, -2.1, -np.pi + 0.02], [0.9, -1.9, 3.0]])
    rows = batch.step_error(ts, gts, W_THR, 0.2, 1.0)
    assert [int(r["best_slot"]) for r in rows] == [int(np.argmax(wb[:nP])), nP + 5, 2 * nP]
    assert [int(r["n_truth"]) for r in rows] == [2, 5, 10] and np.array_equal(rows["t"], ts)
    for b in range(3):
        want = _host_row(a, batch, batch.block(b), truth, seen, ts[b], gts[b], W_THR, 0.2, 1.0)
        if b == 2:
            want = {k: v for k, v in want.items() if not k.startswith("pose_")}
        _check_row(rows[b], want, f"batch filter {b}")
    f.close()
    batch.close()


def _grid(sim, n):
    """The grid of test_filter_batch.py::_grid."""
    pds = [0.99, 0.8, 0.5, 0.9, 0.7, 0.95]
    clutters = [1e-4, 5e-3, 2e-2, 1e-3, 1e-2, 2e-3]
    Ps, datas, seeds = [], [], []
    for b in range(n):
        P = dict(sim.C1_SIM)
        P["Pd"] = pds[b % len(pds)]
        P["clutter"] = clutters[(b * 5 + 1) % len(clutters)]
        Ps.append(P)
        seeds.append(1011 + b)
    return Ps, seeds


def _bytes_equal(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_through_a_run(pkg):
    """Six filters x 200 particles, 300 simulator steps with track_errors: every 10th step the row just logged against the host
    yardstick; tracking changes nothing (the same run without it ends with the same bits); a batch of one logs what a handle logs."""
    a = _tool()
    sim = pkg.sim2d_driver
    nF, nP, K = 6, 200, 301
    Ps, seeds = _grid(sim, nF)
    datas = [sim.generate(P, traj_seed=11 + b, kmax=K) for b, P in enumerate(Ps)]
    firsts = [sim.first_seen_times(d, P) for d, P in zip(datas, Ps)]
    batch = pkg.FilterBatch(nF, nP, gm_capacity=256)
    run = sim.Sim2dBatchRun(batch, datas, Ps, seeds, track_errors=True)
    checked = [0]
    worst = [0.0]

    def on_step(k, r, fired):
        if k % 10:
            return
        rows = r.errors()
        assert rows.shape == (k, nF)
        for b in range(nF):
            t = k * Ps[b]["dt"]
            assert rows[-1, b]["t"] == t
            want = _host_row(a, batch, batch.block(b), datas[b]["landmarks"], firsts[b], t, datas[b]["gt"][k], sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF,
                             sim.ERROR_ORDER)
            for key in ("ospa", "cola", "e_dist", "e_card", "pose_ex", "pose_ey", "pose_eth", "pose_ed"):
                if want[key]:
                    worst[0] = max(worst[0], abs(float(rows[-1, b][key]) - want[key]) / abs(want[key]))
            _check_row(rows[-1, b], want, f"step {k} filter {b}")
            checked[0] += 1

    run.run(on_step=on_step)
    print(f"through a run: {checked[0]} rows checked, largest relative deviation {worst[0]:.3e}")
    log = run.errors()
    assert log.shape == (K - 1, nF) and checked[0] == 30 * nF
    assert (log["n_est"][-1] > 0).all() and (log["n_truth"][-1] > 0).all() and (log["status"] == 0).all()    # maps were built and scored
    w_on, sizes_on = batch.get_weights(), batch.gm_sizes()
    plain = pkg.FilterBatch(nF, nP, gm_capacity=256)
    sim.Sim2dBatchRun(plain, datas, Ps, seeds).run()
    assert _bytes_equal(w_on, plain.get_weights()) and np.array_equal(sizes_on, plain.gm_sizes())
    for s in range(nF * nP):
        for u, v in zip(batch.export_gm(s), plain.export_gm(s)):
            assert _bytes_equal(u, v), s
    batch.close()
    plain.close()
    # a batch of one against an ordinary handle
    K1 = 151
    one = pkg.FilterBatch(1, nP, gm_capacity=256)
    h = pkg.RBPHDFilter(nP, gm_capacity=256)
    r1 = sim.Sim2dBatchRun(one, [datas[0]], [Ps[0]], [seeds[0]], track_errors=True).run(k_to=K1)
    r2 = sim.Sim2dBatchRun([h], [datas[0]], [Ps[0]], [seeds[0]], track_errors=True).run(k_to=K1)
    l1, l2 = r1.errors(), r2.errors()
    assert l1.shape == (K1 - 1, 1) and _bytes_equal(l1, l2)
    one.close()
    h.close()


@pytest.mark.gpu
def test_log_mechanics_and_refusals(pkg):
    rng = np.random.default_rng(33)
    f = pkg.RBPHDFilter(16, gm_capacity=64)
    truth = rng.uniform(0, 4, (12, 2))
    f.set_ground_truth(truth)
    _plant(f, 0, np.ones(9), truth[:9] + 0.01)
    with pytest.raises(pkg.capi.EngineError) as e:                      # no log yet
        f.step_error_async(0.0)
    assert e.value.status == pkg.capi.ERR_CAPACITY
    f.error_log_create(3)
    assert f.error_log_read().shape == (0, 1)
    for k in range(3):
        f.step_error_async(0.1 * k, np.array([[0.0, 0.0, 0.1 * k]]))
    with pytest.raises(pkg.capi.EngineError) as e:                      # full
        f.step_error_async(0.3)
    assert e.value.status == pkg.capi.ERR_CAPACITY and "full" in str(e.value)
    rows = f.error_log_read()
    assert rows.shape == (3, 1) and np.array_equal(rows["t"][:, 0], [0.0, 0.1, 0.2])
    again = f.error_log_read()                                          # rows stay until the log is reset
    assert _bytes_equal(rows, again) and f.error_log_read(max_rows=2).shape == (2, 1)
    sync = f.step_error(0.2, np.array([[0.0, 0.0, 0.2]]))               # the synchronous form: the same record, the log untouched
    assert sync.shape == (1,) and sync[0].tobytes() == rows[2, 0].tobytes()
    assert f.error_log_read().shape == (3, 1)
    f.error_log_reset()
    assert f.error_log_read().shape == (0, 1)
    f.step_error_async(0.7)
    rows = f.error_log_read()
    assert rows.shape == (1, 1) and rows[0, 0]["t"] == 0.7 and int(rows[0, 0]["n_est"]) == 9 and int(rows[0, 0]["n_truth"]) == 12
    assert abs(rows[0, 0]["cola"] - (9 * 0.01 * np.sqrt(2) / 0.2 + 3)) < 1e-12
    for bad in (dict(cutoff=0.0), dict(order=0.5)):
        with pytest.raises(pkg.capi.EngineError) as e:
            f.step_error(0.0, None, **bad)
        assert e.value.status == pkg.capi.ERR_INVALID
    f.close()
    # Victoria Park and FastSLAM handles refuse, with a message
    vp = pkg.RBPHDFilter(8, gm_capacity=64, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    fs = pkg.FastSLAM(8, gm_capacity=64)
    fs.set_model_rngbrg(np.diag([0.01, 0.001]), 0.95, 0.01, 5.0, 0.3, 0.25)
    fs.set_fastslam_config(fs.fs_config)
    fs.set_poses(np.zeros((8, 3)))
    fs.fastslam_update(np.array([[1.0, 0.1], [2.0, -0.4]]))
    for h, word in ((vp, "Victoria Park"), (fs, "FastSLAM")):
        for call in (lambda: h.set_ground_truth(truth), lambda: h.error_log_create(4), lambda: h.error_log_reset(), lambda: h.step_error_async(0.0),
                     lambda: h.error_log_read(), lambda: h.step_error(0.0), lambda: h.get_map_estimate()):
            with pytest.raises(pkg.capi.EngineError) as e:
                call()
            assert e.value.status == pkg.capi.ERR_UNSUPPORTED and word in str(e.value)
        h.close()
    g = pkg.FilterGroup(16, [0, 0], gm_capacity=64)                      # the shards of a group refuse too
    with pytest.raises(pkg.capi.EngineError) as e:
        g.shards[0].step_error(0.0)
    assert e.value.status == pkg.capi.ERR_UNSUPPORTED and "rfsgpu_group" in str(e.value)
    g.close()
