"""The device-side estimate log (include/rfsgpu.h [estimate], csrc/estimate_log.h): per step and filter the particle set and the map of
the highest-weight particle -- what the reference's simulators write into particlePose.dat and landmarkEst.dat -- appended to a log on
the device by one launch that changes nothing of the filter.

The yardstick is the host route that existed before: rfsgpu_step_error for the selection and the two tree sums (best_slot, cardinality,
weight_sum: bit for bit), rfsgpu_get_map_estimate for the Gaussian planes (bit for bit), get_poses / get_weights for the copied fields
and the particle planes (bit for bit), numpy's float64 sums for the four weighted means within 4 N eps max(1, max|q|)
(tests/support/estimate_reference.py::mean_bound), and the numpy restatement of the record for the integer fields.  best_slot is a
GLOBAL slot, as in rfsgpu_step_error: where one filter's rows are compared at two places of a batch, best_slot is compared after
taking the block's first slot off and every other byte as it is."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import estimate_reference as er

ESTIMATE_SYMBOLS = ["rfsgpu_estimate_log_create", "rfsgpu_estimate_log_reset", "rfsgpu_step_estimate_async", "rfsgpu_estimate_log_read",
                    "rfsgpu_batch_run_log_estimates"]
RECORD_FIELDS = ["t", "status", "best_slot", "n_particles", "n_est", "n_logged", "cardinality", "best_weight", "weight_sum", "best_x", "best_y",
                 "best_theta", "mean_x", "mean_y", "mean_cos", "mean_sin"]
THR = 0.75
MIX_SIZES = (0, 1, 63, 64, 65, 130)
CAP = 160


def _tool():
    spec = importlib.util.spec_from_file_location("analysis2d_sim", os.path.join(ROOT, "tools", "analysis2d_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_step_estimate_struct_matches_the_header_and_the_section_is_optional(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    m = re.search(r"struct rfsgpu_step_estimate \{(.*?)\n\};", txt, flags=re.S)
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
    S = pkg.capi.StepEstimate
    assert [n for n, _ in S._fields_] == RECORD_FIELDS
    assert C.sizeof(S) == 8 * len(RECORD_FIELDS) == 128
    dt = pkg.capi.STEP_ESTIMATE_DTYPE
    assert dt.itemsize == 128 and list(dt.names) == RECORD_FIELDS
    for k, (name, ctype) in enumerate(fields):
        assert getattr(S, name).offset == 8 * k and getattr(S, name).size == 8
        assert dict(S._fields_)[name] is (C.c_double if ctype == "double" else C.c_longlong)
        assert dt.fields[name][1] == 8 * k and dt.fields[name][0] == (np.float64 if ctype == "double" else np.int64)
    # outside the STABLE CORE, behind [truth], exported and wrapped
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    names = {w for line in re.findall(r"RFSGPU_CORE(?:_MULTI)?:(.*)", txt) for w in line.split()}
    sec = txt.index("---- [estimate]")
    assert sec > txt.index("---- [truth]") and "[estimate]" in core.split("Everything else is OPTIONAL")[1]
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in ESTIMATE_SYMBOLS:
        assert s not in names, s
        assert re.search(r"\b" + s + r"\b", core.split("Everything else is OPTIONAL")[0]) is None, s
        assert txt.index(s + "(") > sec, s
        assert hasattr(lib, s), s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    for meth in ("estimate_log_create", "estimate_log_reset", "estimate_log_read", "step_estimate_async"):
        assert hasattr(pkg.capi.CFilter, meth), meth
    assert hasattr(pkg.capi.CBatch, "run_log_estimates")
    sim = pkg.sim2d_driver
    for run in (sim.Sim2dRun, sim.Sim2dBatchRun, sim.Sim2dMHBatchRun):
        p = inspect.signature(run.__init__).parameters
        assert p["track_estimates"].default is False and "estimate_threshold" in p and hasattr(run, "estimates")
    for fn in (lib.rfsgpu_estimate_log_reset,):
        fn.restype = C.c_int
        assert fn(C.c_void_p()) == pkg.capi.ERR_INVALID


@pytest.mark.parametrize("precision", [None, 17])
def test_write_run_logs_round_trip(pkg, tmp_path, precision):
    """A synthetic trace (3 steps, 5 particles, 0 / 1 / 4 Gaussians; every number a multiple of 1/64, which %f prints exactly) through
    write_run_logs and tools/analysis2d_sim.analyse: the pose-error and map rows equal the numbers computed from the arrays directly."""
    pytest.importorskip("scipy")
    a = _tool()
    sim = pkg.sim2d_driver
    est, truths = er.synthetic_trace(pkg.capi.STEP_ESTIMATE_DTYPE)
    hdr, gauss, part = est
    b = 1
    d = sim.write_run_logs(str(tmp_path / "filter_001"), b, est, truths[b], precision=precision)
    for name in ("gtPose.dat", "gtLandmark.dat", "deadReckoning.dat", "particlePose.dat", "landmarkEst.dat"):
        assert os.path.exists(os.path.join(d, name)), name
    txt = open(os.path.join(d, "particlePose.dat")).read()
    assert txt.count("\n\n") == hdr.shape[0] and txt.endswith("\n\n")          # one blank line after a step's particles
    first = txt.split("\n")[0].split()
    assert len(first) == 6 and first[1] == "0" and (precision is not None or re.fullmatch(r"-?\d+\.\d{6}", first[0]))
    rows_dr, rows_pose, rows_map = a.analyse(d, write=False)
    T = truths[b]
    assert rows_pose.shape == (hdr.shape[0], 5) and rows_map.shape == (hdr.shape[0], 4) and rows_dr.shape == (hdr.shape[0], 5)
    for r in range(hdr.shape[0]):
        k = r + 1
        t = k * T["dt"]
        x, y, th, w = part[r, b]
        gx, gy, gth = T["gt"][k]
        ws = w.sum()
        ex, ey, eth = x - gx, y - gy, a.wrap(th - gth)
        want = [t, (ex * w).sum() / ws, (ey * w).sum() / ws, (eth * w).sum() / ws, (np.hypot(ex, ey) * w).sum() / ws]
        np.testing.assert_allclose(rows_pose[r], want, rtol=0, atol=1e-12)
        m = int(hdr[r, b]["n_logged"])
        gw = gauss[r, b, 5, :m]
        est_xy = gauss[r, b, 0:2, :m].T[gw >= 0.75]
        seen = T["landmarks"][T["first_seen"] <= t]
        want = [t, len(seen), gw.sum(), a.cola(est_xy, seen)]
        np.testing.assert_allclose(rows_map[r], want, rtol=0, atol=1e-12)
        assert int(hdr[r, b]["best_slot"]) - b * part.shape[3] == int(np.argmax(w))
    # dead reckoning: chained with odometry_step from the odometry (exact only in the lossless files)
    if precision == 17:
        dr = np.loadtxt(os.path.join(d, "deadReckoning.dat"), ndmin=2)
        x = T["gt"][0].copy()
        for k in range(1, dr.shape[0]):
            x = sim.odometry_step(x, T["odom"][k])
            assert np.array_equal(dr[k, 1:], x)
        assert np.array_equal(np.loadtxt(os.path.join(d, "gtPose.dat"), ndmin=2)[:, 1:], T["gt"])
    with pytest.raises(ValueError):
        sim.write_run_logs(str(tmp_path / "none"), b, (hdr, gauss, None), T)


# ---- GPU: the host route ---------------------------------------------------------------------------------------------------------

def _plant(f, slot, w, mean, cov=None):
    n = len(w)
    cov = np.tile(np.eye(2) * 0.01, (n, 1, 1)) if cov is None else cov
    f.import_gm(slot, np.asarray(w, dtype=np.float64), np.asarray(mean, dtype=np.float64).reshape(n, 2), cov)


def _mixture(rng, m, thr=THR):
    """m Gaussians with weights on both sides of the threshold and (m >= 3) exactly on it; distinct covariances."""
    w = rng.uniform(0.05, 1.4, m)
    if m >= 3:
        w[0], w[1], w[m // 2] = thr, np.nextafter(thr, 0.0), thr
    mean = rng.uniform(-5, 5, (m, 2))
    s = rng.uniform(0.01, 0.1, (m, 3))
    cov = np.zeros((m, 2, 2))
    cov[:, 0, 0], cov[:, 1, 1] = s[:, 0] + 0.1, s[:, 1] + 0.1
    cov[:, 0, 1] = cov[:, 1, 0] = s[:, 2] - 0.05
    return w, mean, cov


def _check_against_host_route(f, b, lo, n_live, stride, hdr, gauss, part, thr, max_est, what, log_odds=False):
    """One filter's row against rfsgpu_step_error, rfsgpu_get_map_estimate, get_poses and get_weights (module docstring)."""
    nF = f.n_metric_filters
    err = f.step_error(np.zeros(nF), None, thr, 1.0, 1.0)[b]
    x, w = f.get_poses(), f.get_weights()
    h = hdr[b]
    best = int(h["best_slot"])
    assert best == int(err["best_slot"]), what
    assert lo <= best < lo + max(n_live, 1), what
    assert int(h["n_particles"]) == n_live and int(h["n_est"]) == int(err["n_est"]), what
    for k in ("cardinality", "weight_sum"):
        assert h[k].tobytes() == err[k].tobytes(), (what, k, h[k], err[k])
    m, cv, gw = f.get_map_estimate(thr, filter=b)
    n_est = len(gw)
    n_log = min(n_est, max_est)
    assert int(h["n_est"]) == n_est and int(h["n_logged"]) == n_log and int(h["status"]) == int(n_est > max_est), what
    G = gauss[b]
    want = [m[:n_log, 0], m[:n_log, 1], cv[:n_log, 0, 0], cv[:n_log, 0, 1], cv[:n_log, 1, 1], gw[:n_log]]
    for q, name in enumerate(("mx", "my", "sxx", "sxy", "syy", "w")):
        assert _same(G[q, :n_log], want[q]), (what, name)
    assert not G[:, n_log:].any(), what
    for k, v in (("best_x", x[best, 0]), ("best_y", x[best, 1]), ("best_theta", x[best, 2]), ("best_weight", w[best])):
        assert h[k].tobytes() == np.float64(v).tobytes(), (what, k)
    live = slice(lo, lo + n_live)
    if part is not None:
        P = part[b]
        assert P.shape == (4, stride)
        for q, v in enumerate((x[live, 0], x[live, 1], x[live, 2], w[live])):
            assert _same(P[q, :n_live], v), (what, "part plane", q)
    wl, xl = w[live], x[live]
    ref, planes = er.reference_row(wl, xl, lambda s: (f.export_gm(s)[0], f.export_gm(s)[2], f.export_gm(s)[3]), thr, max_est, lo=lo, log_odds=log_odds)
    for k in ("best_slot", "n_particles", "status"):
        assert int(h[k]) == ref[k], (what, k)
    if not log_odds:                                      # (log-odds: exp on the device and in numpy may round a weight at the threshold apart)
        assert int(h["n_est"]) == ref["n_est"] and _same(G[:5], planes[:5]), what
    if np.isfinite(wl).all() and wl.sum() > 0:
        for k, q in (("mean_x", xl[:, 0]), ("mean_y", xl[:, 1]), ("mean_cos", np.cos(xl[:, 2])), ("mean_sin", np.sin(xl[:, 2]))):
            bound = er.mean_bound(n_live, q)
            assert abs(float(h[k]) - ref[k]) <= bound, (what, k, float(h[k]), ref[k], bound)
    return err


def _one_row(f, t, thr, max_est, particles=True):
    f.estimate_log_create(1, max_est, particles)
    f.step_estimate_async(t, thr)
    hdr, gauss, part = f.estimate_log_read()
    assert hdr.shape[0] == 1
    return hdr[0], gauss[0], None if part is None else part[0]


@pytest.mark.gpu
def test_planted_state_on_an_ordinary_handle(pkg):
    """N = 70 (lanes own one and two slots); the best particle's mixture of 0, 1, 63, 64, 65, 130 Gaussians with weights on both sides
    of the threshold and exactly on it; then the cut (n_est 65 into max_est 64, and max_est 0)."""
    N = 70
    rng = np.random.default_rng(70)
    f = pkg.RBPHDFilter(N, gm_capacity=CAP)
    w = rng.uniform(0.05, 1.0, N)
    w[66] = 2.0
    x = np.column_stack([rng.normal(0, 3, N), rng.normal(0, 3, N), rng.uniform(-np.pi, np.pi, N)])
    f.set_weights(w)
    f.set_poses(x)
    for i in range(N):
        _plant(f, i, *_mixture(rng, 2 + i % 7))
    for m in MIX_SIZES:
        gw, mean, cov = _mixture(rng, m)
        _plant(f, 66, gw, mean, cov)
        for thr in (THR, -np.inf):
            hdr, gauss, part = _one_row(f, 1.25, thr, CAP)
            assert hdr[0]["t"] == 1.25 and int(hdr[0]["best_slot"]) == 66
            n_est = int((gw >= thr).sum())
            assert int(hdr[0]["n_est"]) == n_est and (m < 3 or thr != THR or n_est >= 2)      # (>= keeps the weights exactly on it)
            _check_against_host_route(f, 0, 0, N, N, hdr, gauss, part, thr, CAP, "mixture %d thr %r" % (m, thr))
    # the cut: exactly 65 Gaussians at or above the threshold
    gw = np.concatenate([np.full(65, 0.9), np.full(20, 0.3)])
    gw[:3] = THR
    order = rng.permutation(85)
    mean, cov = rng.uniform(-5, 5, (85, 2)), _mixture(rng, 85)[2]
    _plant(f, 66, gw[order], mean, cov)
    hdr, gauss, part = _one_row(f, 0.5, THR, 64)
    assert (int(hdr[0]["status"]), int(hdr[0]["n_logged"]), int(hdr[0]["n_est"])) == (1, 64, 65) and gauss.shape == (1, 6, 64)
    kept = np.flatnonzero(gw[order] >= THR)[:64]
    assert _same(gauss[0, 0], mean[kept, 0]) and _same(gauss[0, 5], gw[order][kept]) and _same(gauss[0, 3], cov[kept, 0, 1])
    _check_against_host_route(f, 0, 0, N, N, hdr, gauss, part, THR, 64, "cut to 64")
    hdr65, gauss65, _ = _one_row(f, 0.5, THR, 65, particles=False)
    assert (int(hdr65[0]["status"]), int(hdr65[0]["n_logged"])) == (0, 65) and _same(gauss65[0, :, :64], gauss[0])
    hdr0, gauss0, part0 = _one_row(f, 0.5, THR, 0, particles=False)
    assert gauss0.shape == (1, 6, 0) and part0 is None and (int(hdr0[0]["status"]), int(hdr0[0]["n_logged"]), int(hdr0[0]["n_est"])) == (1, 0, 65)
    for k in RECORD_FIELDS:
        if k not in ("status", "n_logged"):
            assert hdr0[0][k].tobytes() == hdr[0][k].tobytes(), k
    f.close()


@pytest.mark.gpu
def test_selection_agrees_with_step_error(pkg):
    N = 70
    rng = np.random.default_rng(71)
    f = pkg.RBPHDFilter(N, gm_capacity=16)
    f.set_poses(np.column_stack([rng.normal(0, 3, (N, 2)), rng.uniform(-3, 3, N)]))
    for i in range(N):
        _plant(f, i, *_mixture(rng, 1 + i % 4))
    base = rng.uniform(0.1, 1.0, N)
    nan = float("nan")
    cases = {}
    w = base.copy(); w[[9, 40]] = 2.0; cases["the maximum held twice: the lower slot"] = (w, 9)
    w = base.copy(); w[[68, 5]] = 2.0; cases["held twice across a lane's two slots"] = (w, 5)
    w = base.copy(); w[67] = 3.0; cases["the maximum at a slot >= 64"] = (w, 67)
    cases["all weights zero: slot 0"] = (np.zeros(N), 0)
    w = base.copy(); w[3] = nan; w[20] = 2.0; cases["a NaN beside a maximum"] = (w, 20)
    w = base.copy(); w[0] = nan; cases["a NaN in slot 0"] = (w, None)
    w = base.copy(); w[64] = nan; w[65] = 5.0; cases["a NaN before the maximum in one lane"] = (w, 65)
    cases["all NaN"] = (np.full(N, nan), 0)
    w = -base; w[7] = nan; cases["negative and NaN: slot 0"] = (w, 0)
    for what, (w, best) in cases.items():
        f.set_weights(w)
        hdr, gauss, part = _one_row(f, 0.0, THR, 16)
        err = _check_against_host_route(f, 0, 0, N, N, hdr, gauss, part, THR, 16, what)
        assert int(hdr[0]["best_slot"]) == int(err["best_slot"]), what
        if best is not None:
            assert int(hdr[0]["best_slot"]) == best, what
        assert hdr[0]["best_weight"].tobytes() == np.float64(w[int(hdr[0]["best_slot"])]).tobytes(), what
    f.close()


def _planted_batch(pkg, make, nF, n_per, rng, log_odds=False):
    B = make(nF, n_per)
    n = nF * n_per
    w = rng.uniform(0.05, 1.0, n)
    x = np.column_stack([rng.normal(0, 3, (n, 2)), rng.uniform(-np.pi, np.pi, n)])
    maps = []
    for s in range(n):
        gw, mean, cov = _mixture(rng, 3 + s % 6)
        if log_odds:                                       # log-odds whose existence probabilities lie on both sides of 0.75
            pr = np.clip(gw / 1.45, 0.03, 0.97)
            pr[0], pr[1] = 0.9, 0.3                        # both sides in every map
            gw = np.log(pr / (1 - pr))
        maps.append((gw, mean, cov))
        _plant(B, s, gw, mean, cov)
    B.set_weights(w)
    B.set_poses(x)
    return B, w, x, maps


@pytest.mark.gpu
@pytest.mark.parametrize("n_per", [64, 65])
def test_rbphd_batch_against_the_host_route_and_the_place_in_the_batch(pkg, n_per):
    rng = np.random.default_rng(300 + n_per)
    B, w, x, maps = _planted_batch(pkg, lambda nF, n: pkg.FilterBatch(nF, n, gm_capacity=16), 3, n_per, rng)
    ts = np.array([0.1, 0.2, 0.3])
    hdr, gauss, part = _one_row(B, ts, THR, 16)
    assert np.array_equal(hdr["t"], ts) and part.shape == (3, 4, n_per)
    for b in range(3):
        _check_against_host_route(B, b, b * n_per, n_per, n_per, hdr, gauss, part, THR, 16, "filter %d of 3 x %d" % (b, n_per))
    one = pkg.FilterBatch(1, n_per, gm_capacity=16)
    blk = slice(2 * n_per, 3 * n_per)
    one.set_weights(w[blk])
    one.set_poses(x[blk])
    for i in range(n_per):
        _plant(one, i, *maps[2 * n_per + i])
    h1, g1, p1 = _one_row(one, ts[2:], THR, 16)
    for k in RECORD_FIELDS:
        if k == "best_slot":
            assert int(h1[0][k]) == int(hdr[2][k]) - 2 * n_per
        else:
            assert h1[0][k].tobytes() == hdr[2][k].tobytes(), k
    assert _same(g1[0], gauss[2]) and _same(p1[0], part[2])
    B.close()
    one.close()


@pytest.mark.gpu
def test_fastslam_batch_logs_the_converted_log_odds(pkg):
    rng = np.random.default_rng(400)
    sim = pkg.sim2d_driver

    def make(nF, n):
        B = pkg.FastSLAMBatch(nF, n, gm_capacity=16)
        for b in range(nF):
            sim.configure_fastslam_batch_filter(B, b)
        return B

    B, w, x, maps = _planted_batch(pkg, make, 2, 65, rng, log_odds=True)
    for thr in (THR, -np.inf):
        hdr, gauss, part = _one_row(B, np.array([0.1, 0.2]), thr, 16)
        for b in range(2):
            _check_against_host_route(B, b, b * 65, 65, 65, hdr, gauss, part, thr, 16, "FastSLAM filter %d thr %r" % (b, thr), log_odds=True)
            lo = maps[int(hdr[b]["best_slot"])][0]
            n = int(hdr[b]["n_logged"])
            assert n > 0 and ((gauss[b, 5, :n] > 0) & (gauss[b, 5, :n] < 1)).all()
            if thr == -np.inf:
                assert n == len(lo)
                np.testing.assert_allclose(gauss[b, 5, :n], er.existence(lo), rtol=1e-13, atol=0)
    B.close()


@pytest.mark.gpu
def test_multi_hypothesis_batch_covers_live_slots_only(pkg, sc):
    """Two filters of 8 in blocks of 32 through a cycle that grows filter 0's set and one whose resampling shrinks it back: n_particles
    is live_counts(), selection and particle planes cover the live slots, and without the metric switch every call is refused."""
    from tests.support import mh_batch_reference as mb
    from tests.support import mh_device_cycle_reference as ref
    n, stride = 8, 32
    scens = [ref.crowded(sc, n), ref.sparse(sc, n)]
    rig = mb.Rig(pkg, sc, scens, [3, 2], [50.0] * 2, n, stride)
    B = rig.batch
    U = pkg.capi.ERR_UNSUPPORTED
    calls = {"estimate_log_create": lambda: B.estimate_log_create(2, 8, True), "estimate_log_reset": lambda: B.estimate_log_reset(),
             "step_estimate_async": lambda: B.step_estimate_async(np.zeros(2)), "estimate_log_read": lambda: B.estimate_log_read(),
             "run_log_estimates": lambda: B.run_log_estimates(True)}
    for name, call in calls.items():
        with pytest.raises(pkg.capi.EngineError) as e:
            call()
        assert e.value.status == U and "multi-hypothesis" in str(e.value), (name, str(e.value))
    B.serve_metrics(True)
    ts = np.array([0.1, 0.2])

    def check(what, want_counts):
        hdr, gauss, part = _one_row(B, ts, THR, 64)
        counts = B.live_counts()
        assert list(counts) == want_counts, (what, counts)
        assert list(hdr["n_particles"]) == want_counts and part.shape == (2, 4, stride)
        for b in range(2):
            _check_against_host_route(B, b, b * stride, int(counts[b]), stride, hdr, gauss, part, THR, 64, "%s: filter %d" % (what, b), log_odds=True)
            assert not part[b][:, int(counts[b]):].any()
        return hdr

    check("before any cycle", [n, n])

    def shut(b, c):
        c.minUpdatesBeforeResample = mb.NEVER
        c.nParticlesMax = stride
    rig.each_config(shut)
    Zs = [s["Z"] for s in scens]
    rig.cycle(Zs, [0.25] * 2, handles=False)
    hdr = check("after the growing cycle", [24, 8])
    assert (hdr["n_est"] > 0).any()

    def open_(b, c):
        c.maxNDataAssocHypotheses = 1
        c.minUpdatesBeforeResample = 0 if b == 0 else mb.NEVER
    rig.each_config(open_)
    rig.set_resampling(0, 1e9, 0.0)
    rz = np.random.default_rng(5)
    rig.cycle([s["Z"] + rz.normal(0, 3e-3, s["Z"].shape) for s in scens], [0.6] * 2, handles=False)
    hdr = check("after the resampling cycle", [8, 8])
    assert (np.asarray(B.gm_sizes())[B.block(0)][8:24] > 0).all()      # the larger set's maps sit beyond the count, unread
    assert int(hdr[0]["best_slot"]) == 0 and hdr[0]["weight_sum"] == 8.0
    B.serve_metrics(False)
    with pytest.raises(pkg.capi.EngineError) as e:
        B.step_estimate_async(ts)
    assert e.value.status == U
    rig.close()


# ---- GPU: one run call against per-step calls, and the files -----------------------------------------------------------------------

RUN_K, N_PINNED = 26, 4


def _run_batch(pkg, estimates=True, errors=True):
    """Two RB-PHD filters of 16 particles, gm_capacity 32, device sensor and truth of RUN_K steps that move from step 3 on and are pinned
    up to step N_PINNED."""
    sim = pkg.sim2d_driver
    base = dict(sim.C1_SIM, kmax=RUN_K, n_landmarks=10, n_segments=5, eff_n=14.0)
    Ps = [dict(base, Pd=0.99, clutter=1e-4), dict(base, Pd=0.8, clutter=5e-3, eff_n=13.0)]
    seeds = [21, 22]
    batch = pkg.FilterBatch(2, 16, gm_capacity=32)
    for b, P in enumerate(Ps):
        sim.configure_batch_filter(batch, b, P)
        Q = np.array([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2
        batch.set_motion_odometry(b, Q, seeds[b])
        batch.set_resampling(b, P["eff_n"], 0.75)
        c = sim.truth_config(P, b)
        c.n_still, c.n_pinned = 2, N_PINNED
        batch.set_truth(b, c, seeds[b])
    batch.generate_truth(RUN_K)
    truth = [batch.get_truth(b) for b in range(2)]
    for b, (P, d) in enumerate(zip(Ps, truth)):
        batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"],
                         max_nz=sim.sensor_max_nz_of(d["n_det_max"], P), seed=seeds[b])
        batch.set_ground_truth(d["landmarks"], d["first_seen"], filter=b)
        d["dt"] = P["dt"]
    if errors:
        batch.error_log_create(RUN_K)
    if estimates:
        batch.estimate_log_create(RUN_K, 32, True)
    return batch, Ps, truth


def _state(batch):
    s = dict(w=batch.get_weights(), x=batch.get_poses(), sizes=batch.gm_sizes(), counts=batch.resample_counts())
    for i in range(batch.n):
        for q, a in enumerate(batch.export_gm(i)):
            s["gm%d_%d" % (i, q)] = a
    return s


@pytest.fixture(scope="module")
def run_trace(pkg):
    """The one-call run with the switch on, shared by the two tests below: (estimates, error log, truth, final state)."""
    sim = pkg.sim2d_driver
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    A, Ps, truth = _run_batch(pkg)
    A.run_log_estimates(True, -np.inf)
    A.run_truth_async(1, RUN_K, True, *consts)
    est = A.estimate_log_read()
    out = dict(est=est, errors=A.error_log_read(), truth=truth, state=_state(A), Ps=Ps)
    # drained in two chunks: read(row_from, ...), reset
    h1, g1, p1 = A.estimate_log_read(0, 10)
    h2, g2, p2 = A.estimate_log_read(10)
    out["chunks"] = (np.concatenate([h1, h2]), np.concatenate([g1, g2]), np.concatenate([p1, p2]), h1.shape[0], h2.shape[0])
    A.estimate_log_reset()
    out["after_reset"] = A.estimate_log_read()[0].shape
    A.close()
    return out


@pytest.mark.gpu
def test_one_run_call_against_per_step_calls(pkg, run_trace):
    sim = pkg.sim2d_driver
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    hdrA, gaussA, partA = run_trace["est"]
    assert hdrA.shape == (RUN_K - 1, 2) and gaussA.shape == (RUN_K - 1, 2, 6, 32) and partA.shape == (RUN_K - 1, 2, 4, 16)
    assert (hdrA["n_particles"] == 16).all() and (hdrA["n_logged"][-1] > 0).all() and (hdrA["status"] == 0).all()
    for b, P in enumerate(run_trace["Ps"]):
        assert _same(hdrA["t"][:, b], np.arange(1, RUN_K) * P["dt"])
    assert _same(hdrA["best_slot"], run_trace["errors"]["best_slot"]) and _same(hdrA["weight_sum"], run_trace["errors"]["weight_sum"])
    assert _same(hdrA["cardinality"], run_trace["errors"]["cardinality"])
    ch, cg, cp, n1, n2 = run_trace["chunks"]
    assert (n1, n2) == (10, RUN_K - 11) and _same(ch, hdrA) and _same(cg, gaussA) and _same(cp, partA) and run_trace["after_reset"] == (0, 2)
    # the per-step calls, each followed by step_estimate_async
    B, Ps, truthB = _run_batch(pkg)
    gt = np.ascontiguousarray(np.stack([d["gt"] for d in truthB], axis=1))
    od = np.ascontiguousarray(np.stack([d["odom"] for d in truthB], axis=1))
    pin = np.ones(2, dtype=np.uint8)
    for k in range(1, RUN_K):
        if k <= N_PINNED:
            B.propagate_async(od[k], k, pin=pin, pin_pose=gt[k])
        else:
            B.propagate_async(od[k], k)
        B.sense_async(gt[k], k)
        B.cycle_sensed_async(True, normalize=True)
        B.resample_sensed_async(k)
        t = np.array([k * P["dt"] for P in Ps])
        B.step_error_async(t, gt[k], *consts)
        B.step_estimate_async(t, -np.inf)
    hdrB, gaussB, partB = B.estimate_log_read()
    assert _same(hdrA, hdrB) and _same(gaussA, gaussB) and _same(partA, partB)
    assert _same(run_trace["errors"], B.error_log_read())
    B.close()
    # the switch off: the same final state and error log
    D, _, _ = _run_batch(pkg, estimates=False)
    D.run_truth_async(1, RUN_K, True, *consts)
    sD = _state(D)
    assert sD.keys() == run_trace["state"].keys()
    for k in sD:
        assert _same(sD[k], run_trace["state"][k]), k
    assert _same(D.error_log_read(), run_trace["errors"])
    assert sD["counts"].sum() > 0                          # (the run resampled: the rows were taken behind it)
    D.close()


@pytest.mark.gpu
def test_end_to_end_through_the_files(pkg, run_trace, tmp_path):
    """The run's trace through write_run_logs(precision=17) and analysis2d_sim.analyse against the device error log's rows, at the
    tolerances of tests/test_step_error.py::test_through_a_run (1e-12 relative, 1e-13 for the cardinality, integers exact)."""
    pytest.importorskip("scipy")
    a = _tool()
    sim = pkg.sim2d_driver
    rel = lambda got, want, tol: abs(got - want) <= (tol * abs(want) if want != 0.0 else 1e-15)
    for b in range(2):
        d = sim.write_run_logs(str(tmp_path / ("filter_%03d" % b)), b, run_trace["est"], run_trace["truth"][b], precision=17)
        _, rows_pose, rows_map = a.analyse(d, write=False)
        log = run_trace["errors"][:, b]
        assert rows_pose.shape[0] == rows_map.shape[0] == RUN_K - 1
        for r in range(RUN_K - 1):
            what = "filter %d step %d" % (b, r + 1)
            assert rows_pose[r, 0] == log[r]["t"] == rows_map[r, 0], what
            for q, k in enumerate(("pose_ex", "pose_ey", "pose_eth", "pose_ed")):
                assert rel(rows_pose[r, 1 + q], float(log[r][k]), 1e-12), (what, k, rows_pose[r, 1 + q], float(log[r][k]))
            assert int(rows_map[r, 1]) == int(log[r]["n_truth"]), what
            assert rel(rows_map[r, 2], float(log[r]["cardinality"]), 1e-13), (what, rows_map[r, 2], float(log[r]["cardinality"]))
            assert rel(rows_map[r, 3], float(log[r]["cola"]), 1e-12), (what, rows_map[r, 3], float(log[r]["cola"]))


# ---- GPU: mechanics and refusals ---------------------------------------------------------------------------------------------------

def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


@pytest.mark.gpu
def test_log_mechanics_and_refusals(pkg):
    capi = pkg.capi
    rng = np.random.default_rng(33)
    f = pkg.RBPHDFilter(16, gm_capacity=64)
    _plant(f, 0, np.ones(9), rng.uniform(0, 4, (9, 2)))
    w0 = f.get_weights().copy()
    _raises(pkg, capi.ERR_CAPACITY, lambda: f.step_estimate_async(0.0), "no estimate log")
    _raises(pkg, capi.ERR_INVALID, lambda: f.estimate_log_create(2, -1))
    _raises(pkg, capi.ERR_INVALID, lambda: f.estimate_log_create(2, 65))
    _raises(pkg, capi.ERR_INVALID, lambda: f.estimate_log_create(-1, 4))
    _raises(pkg, capi.ERR_CAPACITY, lambda: f.step_estimate_async(0.0), "no estimate log")      # a refused create leaves no log
    f.estimate_log_create(3, 64, True)                                  # max_est = gm_capacity is served
    assert f.estimate_log_read()[0].shape == (0, 1)
    for k in range(3):
        f.step_estimate_async(0.1 * k)
    _raises(pkg, capi.ERR_CAPACITY, lambda: f.step_estimate_async(0.3), "full")
    hdr, gauss, part = f.estimate_log_read()
    assert hdr.shape == (3, 1) and np.array_equal(hdr["t"][:, 0], [0.0, 0.1, 0.2]) and (hdr["n_est"] == 9).all()
    again = f.estimate_log_read()
    assert _same(hdr, again[0]) and _same(gauss, again[1]) and _same(part, again[2])      # rows stay until the log is reset
    h, g, p = f.estimate_log_read(1, 1)
    assert _same(h, hdr[1:2]) and _same(g, gauss[1:2]) and _same(p, part[1:2])
    assert f.estimate_log_read(3)[0].shape == (0, 1)                    # row_from == rows: nothing, no error
    n = C.c_int()
    for bad in (-1, 4):
        _raises(pkg, capi.ERR_INVALID, lambda: f._call("estimate_log_read", C.c_int(bad), C.c_int(1), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.byref(n)))
    _raises(pkg, capi.ERR_INVALID, lambda: f._call("estimate_log_read", C.c_int(0), C.c_int(-1), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.byref(n)))
    f.estimate_log_reset()
    assert f.estimate_log_read()[0].shape == (0, 1)
    f.step_estimate_async(0.7)
    assert f.estimate_log_read()[0]["t"][0, 0] == 0.7
    f.estimate_log_create(0, 0)                                         # capacity 0 frees everything
    _raises(pkg, capi.ERR_CAPACITY, lambda: f.step_estimate_async(0.0), "no estimate log")
    _raises(pkg, capi.ERR_UNSUPPORTED, lambda: f._call("batch_run_log_estimates", C.c_int(1), C.c_double(0.75)))
    assert _same(f.get_weights(), w0)
    f.close()
    # Victoria Park, FastSLAM handles and group shards refuse with [metric]'s wording
    vp = pkg.RBPHDFilter(8, gm_capacity=64, model=capi.MODEL_VICTORIAPARK_3D)
    fs = pkg.FastSLAM(8, gm_capacity=64)
    fs.set_model_rngbrg(np.diag([0.01, 0.001]), 0.95, 0.01, 5.0, 0.3, 0.25)
    fs.set_fastslam_config(fs.fs_config)
    fs.set_poses(np.zeros((8, 3)))
    fs.fastslam_update(np.array([[1.0, 0.1], [2.0, -0.4]]))
    g = pkg.FilterGroup(16, [0, 0], gm_capacity=64)
    for h, word in ((vp, "Victoria Park"), (fs, "FastSLAM"), (g.shards[0], "rfsgpu_group")):
        for call in (lambda: h.estimate_log_create(4, 4), lambda: h.estimate_log_reset(), lambda: h.step_estimate_async(0.0), lambda: h.estimate_log_read(),
                     lambda: h._call("batch_run_log_estimates", C.c_int(1), C.c_double(0.75))):
            _raises(pkg, capi.ERR_UNSUPPORTED, call, word, "the device-side map / pose error serves")
    vp.close()
    fs.close()
    g.close()


@pytest.mark.gpu
def test_a_run_with_too_few_estimate_rows_is_refused_before_anything_is_enqueued(pkg):
    sim = pkg.sim2d_driver
    consts = (sim.ERROR_W_THRESHOLD, sim.ERROR_CUTOFF, sim.ERROR_ORDER)
    A, Ps, truth = _run_batch(pkg, estimates=False)
    A.run_log_estimates(True, THR)
    w0, x0 = A.get_weights().copy(), A.get_poses().copy()
    _raises(pkg, pkg.capi.ERR_CAPACITY, lambda: A.run_truth_async(1, 6, True, *consts), "without an estimate log")
    A.estimate_log_create(4, 8, False)
    _raises(pkg, pkg.capi.ERR_CAPACITY, lambda: A.run_truth_async(1, 6, True, *consts), "estimate log has fewer free rows")
    assert A.error_log_read().shape == (0, 2) and A.estimate_log_read()[0].shape == (0, 2)
    assert _same(A.get_weights(), w0) and _same(A.get_poses(), x0)
    A.run_truth_async(1, 5, True, *consts)                              # exactly as many free rows as steps: served
    assert A.error_log_read().shape == (4, 2) and A.estimate_log_read()[0].shape == (4, 2)
    _raises(pkg, pkg.capi.ERR_CAPACITY, lambda: A.run_truth_async(5, 6, True, *consts), "estimate log has fewer free rows")
    A.run_log_estimates(False)
    A.run_truth_async(5, 6, True, *consts)                              # off: the run needs no estimate rows
    assert A.error_log_read().shape == (5, 2) and A.estimate_log_read()[0].shape == (4, 2)
    A.close()
