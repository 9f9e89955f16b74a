"""The device-side estimate log on ORDINARY handles (include/rfsgpu.h [estimate], rfsgpu_handle_serve_estimates): the Victoria Park
model and handles that run FastSLAM updates or cycles, and rows appended behind pending device cycles without resolving them.

Yardsticks: the numpy restatement of a row (tests/support/estimate_reference.py::reference_row) fed the per-slot getters -- integer
fields exact, copied fields bit for bit, the sums within mean_bound; and, for rows behind device cycles, the rows the same kernel
writes on the host-stop route of the same realisation (tests/support/*_device_cycle_reference.py) -- every byte equal, because both
come from one kernel on one state."""
import ctypes as C
import os
import subprocess
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np
import pytest

from conftest import ROOT
from tests.support import estimate_reference as er
from tests.support import mh_device_cycle_reference as mh
from tests.support import rbphd_device_cycle_reference as rb
from tests.support import vp_device_cycle_reference as vpref

THR = 0.75
CAP = 96
COPIED = ("best_x", "best_y", "best_theta", "best_weight")
SUMS = ("weight_sum", "mean_x", "mean_y", "mean_cos", "mean_sin")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


def _same_rows(a, b, what=""):
    """Two (hdr, gauss, part) reads: every byte equal."""
    assert _same(a[0], b[0]), (what, "headers", a[0], b[0])
    assert _same(a[1], b[1]), (what, "Gaussian planes")
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or _same(a[2], b[2])), (what, "particle planes")


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_switch_is_exported_with_the_headers_arguments(pkg):
    assert rb.declared_args("rfsgpu_handle_serve_estimates") == "rfsgpu_filter *f, int on"
    assert "handle_serve_estimates" in pkg.capi.ABI_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    assert txt.index("rfsgpu_handle_serve_estimates(rfsgpu_filter") > txt.index("---- [estimate]")
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    assert hasattr(lib, "rfsgpu_handle_serve_estimates") and hasattr(pkg.capi.CFilter, "handle_serve_estimates")


def test_null_handle_is_invalid(pkg):
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    lib.rfsgpu_handle_serve_estimates.restype = C.c_int
    for on in (0, 1):
        assert lib.rfsgpu_handle_serve_estimates(C.c_void_p(), C.c_int(on)) == pkg.capi.ERR_INVALID


def _fixed(v, width):
    """std::fixed, precision 3, the exact binary value rounded half-even in decimal arithmetic."""
    return str(Decimal(float(v)).quantize(Decimal("0.001"), rounding=ROUND_HALF_EVEN)).rjust(width)


def test_write_vp_logs_prints_the_references_format(pkg, tmp_path):
    """A synthetic trace of one filter (3 rows, 5 particles, 0 / 1 / 4 Gaussians; every number a multiple of 1/64): the two files hold
    exactly the text built here field by field in decimal arithmetic."""
    (hdr, gauss, part), _ = er.synthetic_trace(pkg.capi.STEP_ESTIMATE_DTYPE, n_filters=1)
    assert [int(v) for v in hdr["n_logged"][:, 0]] == [0, 1, 4]                      # one row without Gaussians
    w1 = part[1, 0, 3]
    assert (w1 == w1.max()).sum() == 2 and int(hdr["best_slot"][1, 0]) == int(np.flatnonzero(w1 == w1.max())[0])   # the maximum held twice
    poses, lms = "", ""
    for r in range(3):
        t = hdr["t"][r, 0]
        for i in range(5):
            poses += _fixed(t, 10) + str(i).rjust(5) + "".join(_fixed(part[r, 0, q, i], 10) for q in range(4)) + "\n"
        for m in range(int(hdr["n_logged"][r, 0])):
            lms += _fixed(t, 10) + str(int(hdr["best_slot"][r, 0])).rjust(5) + "".join(_fixed(gauss[r, 0, q, m], 10) for q in range(6)) + "\n"
    p_pose, p_lm = pkg.vp_driver.write_vp_logs(str(tmp_path / "logs"), (hdr, gauss, part))
    assert os.path.basename(p_pose) == "particlePose.dat" and os.path.basename(p_lm) == "landmarkEst.dat"
    assert open(p_pose).read() == poses and open(p_lm).read() == lms
    assert len(poses.splitlines()) == 15 and len(lms.splitlines()) == 5 and len(poses.splitlines()[0]) == 55 and len(lms.splitlines()[0]) == 75
    p_pose, p_lm = pkg.vp_driver.write_vp_logs(str(tmp_path / "none"), (hdr, gauss, None))      # a log without particles
    assert open(p_pose).read() == "" and open(p_lm).read() == lms


# ---- GPU: switch and refusals ----------------------------------------------------------------------------------------------------

def _metric_calls(f):
    return (lambda: f.step_error(0.0), lambda: f.error_log_create(2), lambda: f.get_map_estimate(), lambda: f.set_ground_truth(np.zeros((1, 2))),
            lambda: f._call("batch_run_log_estimates", C.c_int(1), C.c_double(THR)))


def _log_calls(f):
    return (lambda: f.estimate_log_create(2, 4), lambda: f.estimate_log_reset(), lambda: f.step_estimate_async(0.0), lambda: f.estimate_log_read())


@pytest.mark.gpu
def test_switch_and_refusals(pkg):
    capi = pkg.capi
    U = capi.ERR_UNSUPPORTED
    rng = np.random.default_rng(5)
    vp = pkg.RBPHDFilter(6, gm_capacity=16, model=capi.MODEL_VICTORIAPARK_3D)
    fs = pkg.RBPHDFilter(6, gm_capacity=16)
    fs.fastslam_update(np.zeros((0, 2)))                                   # an update without measurements: the handle is a FastSLAM handle
    for f, word, dm in ((vp, "the Victoria Park model", 3), (fs, "a FastSLAM handle", 2)):
        f.set_weights(rng.uniform(0.1, 1.0, 6))
        for i in range(6):
            f.import_gm(i, rng.uniform(0.2, 1.0, 3), rng.uniform(-4, 4, (3, dm)), np.tile(np.eye(dm) * 0.02, (3, 1, 1)))
        before = rb.state(f)
        for call in _log_calls(f) + _metric_calls(f):                      # off at creation: today's refusals, today's texts
            _raises(pkg, U, call, word, "the device-side map / pose error serves")
        f.handle_serve_estimates(True)
        f.estimate_log_create(3, 16, True)
        f.step_estimate_async(0.5, -np.inf)
        f.step_estimate_async(1.5, -np.inf)
        hdr, gauss, part = f.estimate_log_read()
        assert hdr.shape == (2, 1) and gauss.shape == (2, 1, 6, 16) and part.shape == (2, 1, 4, f.max_particles)
        assert list(hdr["t"][:, 0]) == [0.5, 1.5] and (hdr["n_particles"] == 6).all() and (hdr["n_est"] == 3).all() and (hdr["status"] == 0).all()
        f.estimate_log_reset()
        assert f.estimate_log_read()[0].shape == (0, 1)
        for call in _metric_calls(f):                                      # [metric] is not part of the switch
            _raises(pkg, U, call, word)
        f.handle_serve_estimates(False)                                    # the refusals are back, the log is gone, the filter is as it was
        for call in _log_calls(f):
            _raises(pkg, U, call, word, "the device-side map / pose error serves")
        rb.assert_same_state(before, rb.state(f))
        f.handle_serve_estimates(True)
        _raises(pkg, capi.ERR_CAPACITY, lambda: f.step_estimate_async(0.0), "no estimate log")
        f.close()
    g = pkg.FilterGroup(16, [0, 0], gm_capacity=16)
    batches = (pkg.FilterBatch(2, 4, gm_capacity=16), pkg.FastSLAMBatch(2, 4, gm_capacity=16), pkg.MHFastSLAMBatch(2, 4, 8, gm_capacity=16))
    for h, word in [(b, "batch") for b in batches] + [(g.shards[0], "rfsgpu_group")]:
        for on in (True, False):
            _raises(pkg, U, lambda: h.handle_serve_estimates(on), "handle_serve_estimates", word)
    for b in batches:
        b.close()
    g.close()


# ---- GPU: planted Victoria Park rows ------------------------------------------------------------------------------------------------

def _mixture3(rng, m, log_odds=False):
    """m Victoria Park Gaussians; weights on both sides of the threshold and (m >= 3, plain weights) exactly on it."""
    if log_odds:
        w = rng.uniform(-3.0, 3.0, m)
        w = np.where(np.abs(w - np.log(3.0)) < 1e-3, w + 0.01, w)            # (exp on the device and in numpy must not round a weight across 0.75)
    else:
        w = rng.uniform(0.05, 1.4, m)
        if m >= 3:
            w[0], w[1], w[m // 2] = THR, np.nextafter(THR, 0.0), THR
    mean = rng.uniform(-5, 5, (m, 3))
    A = rng.normal(0, 0.2, (m, 3, 3))
    cov = A @ np.swapaxes(A, -1, -2) + np.eye(3) * 0.05
    return w, mean, cov


def _gm2(f, s):
    w, _, mean, cov = f.export_gm(s)
    return w, mean[:, :2], cov[:, :2, :2]


def _one_row(f, t, thr, max_est, particles=True):
    f.estimate_log_create(1, max_est, particles)
    f.step_estimate_async(t, thr)
    hdr, gauss, part = f.estimate_log_read()
    assert hdr.shape == (1, 1)
    return hdr[0, 0], gauss[0, 0], None if part is None else part[0, 0]


def _check_row(f, h, G, P, thr, max_est, what, log_odds=False):
    """One row of a served handle against reference_row fed the getters' mean[:, :2] and cov[:, :2, :2]."""
    n = f.n
    x, w = f.get_poses(), f.get_weights()
    ref, planes = er.reference_row(w, x, lambda s: _gm2(f, s), thr, max_est, log_odds=log_odds)
    for k in ("status", "best_slot", "n_particles", "n_est", "n_logged"):
        assert int(h[k]) == ref[k], (what, k, int(h[k]), ref[k])
    best, k = ref["best_slot"], ref["n_logged"]
    for name, v in zip(COPIED, (x[best, 0], x[best, 1], x[best, 2], w[best])):
        assert h[name].tobytes() == np.float64(v).tobytes(), (what, name)
    assert _same(G[:5], planes[:5]), (what, "means and covariances")
    assert not G[:, k:].any(), what
    if log_odds:
        assert np.all(np.abs(G[5, :k] - planes[5, :k]) <= 4 * er.EPS), (what, "existence probabilities")
    else:
        assert _same(G[5], planes[5]), (what, "weights")
    gw = _gm2(f, best)[0]
    gw = er.existence(gw) if log_odds else gw
    assert abs(float(h["cardinality"]) - ref["cardinality"]) <= er.mean_bound(max(len(gw), 1), gw), (what, "cardinality")
    if np.isfinite(w).all() and w.sum() > 0:
        assert abs(float(h["weight_sum"]) - ref["weight_sum"]) <= er.mean_bound(n, w), (what, "weight_sum")
        for name, q in (("mean_x", x[:, 0]), ("mean_y", x[:, 1]), ("mean_cos", np.cos(x[:, 2])), ("mean_sin", np.sin(x[:, 2]))):
            bound = er.mean_bound(n, q)
            assert abs(float(h[name]) - ref[name]) <= bound, (what, name, float(h[name]), ref[name], bound)
    else:                                                                 # all zero: 0 / 0; a NaN weight: NaN sums
        assert all(np.isnan(float(h[name])) for name in SUMS[1:]), what
        assert (float(h["weight_sum"]) == 0.0) if np.isfinite(w).all() else np.isnan(float(h["weight_sum"])), what
    if P is not None:
        assert P.shape == (4, f.max_particles)
        for q, v in enumerate((x[:, 0], x[:, 1], x[:, 2], w)):
            assert _same(P[q, :n], v), (what, "particle plane", q)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257])
def test_planted_victoria_park_rows(pkg, N):
    """Every mixture size of the best particle (0, 1, 63, 64, 65, 96 at capacity 96) under max_est 0, 1, 64, 96 (n_est > max_est: status
    1) and both thresholds; the weight cases (held twice, all zero, one NaN); log-odds weights after a FastSLAM update; and the sums
    of a 2-D handle with the same weights and poses, bit for bit."""
    rng = np.random.default_rng(100 + N)
    VP = pkg.capi.MODEL_VICTORIAPARK_3D
    f = pkg.RBPHDFilter(N, gm_capacity=CAP, model=VP)
    f.handle_serve_estimates(True)
    base = rng.uniform(0.05, 1.0, N)
    best = N - 1 if N < 3 else N - 2
    w = base.copy()
    w[best] = 2.0
    x = np.column_stack([rng.normal(0, 3, N), rng.normal(0, 3, N), rng.uniform(-np.pi, np.pi, N)])
    f.set_weights(w)
    f.set_poses(x)
    for i in range(N):
        f.import_gm(i, *_mixture3(rng, 1 + i % 5))
    for m in (0, 1, 63, 64, 65, 96):
        gw, mean, cov = _mixture3(rng, m)
        f.import_gm(best, gw, mean, cov)
        for max_est in (0, 1, 64, 96):
            for thr in (THR, -np.inf):
                h, G, P = _one_row(f, 2.5, thr, max_est, particles=max_est == 96)
                assert h["t"] == 2.5 and int(h["best_slot"]) == best and int(h["n_est"]) == int((gw >= thr).sum())
                assert int(h["status"]) == int(int(h["n_est"]) > max_est)
                _check_row(f, h, G, P, thr, max_est, "N %d mixture %d max_est %d thr %r" % (N, m, max_est, thr))
    # the same weights and poses on an ordinary 2-D handle, which the section serves without the switch: the tree is the same code
    f2 = pkg.RBPHDFilter(N, gm_capacity=CAP)
    f2.set_weights(w)
    f2.set_poses(x)
    h3, _, _ = _one_row(f, 0.0, THR, 4, particles=False)
    f2.estimate_log_create(1, 4)
    f2.step_estimate_async(0.0, THR)
    h2 = f2.estimate_log_read()[0][0, 0]
    for k in SUMS + ("best_slot", "n_particles") + COPIED:
        assert h3[k].tobytes() == h2[k].tobytes(), (k, h3[k], h2[k])
    f2.close()
    # weights: the maximum held twice (the first holder), all zero (slot 0), one NaN
    nan = float("nan")
    cases = {"all zero": (np.zeros(N), 0)}
    if N >= 2:
        wc = base.copy(); wc[[N - 1, (N - 1) // 2]] = 2.0; cases["held twice"] = (wc, (N - 1) // 2)
        wc = base.copy(); wc[0] = nan; wc[N - 1] = 3.0; cases["a NaN beside the maximum"] = (wc, N - 1)
    else:
        cases["a NaN alone"] = (np.array([nan]), 0)
    for what, (wc, want) in cases.items():
        f.set_weights(wc)
        h, G, P = _one_row(f, 1.0, -np.inf, CAP)
        assert int(h["best_slot"]) == want, what
        _check_row(f, h, G, P, -np.inf, CAP, "N %d %s" % (N, what))
    # log-odds: after a FastSLAM update on the handle a Gaussian's logged weight is 1 - 1 / (1 + exp(w))
    f.set_weights(w)
    f.fastslam_update(np.zeros((0, 3)))
    f.import_gm(best, *_mixture3(rng, 65, log_odds=True))
    for thr in (THR, -np.inf):
        h, G, P = _one_row(f, 1.0, thr, 64)
        assert 0 < int(h["n_est"]) and (thr == THR or (int(h["n_est"]), int(h["status"])) == (65, 1))
        assert np.all((G[5, :int(h["n_logged"])] > 0) & (G[5, :int(h["n_logged"])] < 1))
        _check_row(f, h, G, P, thr, 64, "N %d log-odds thr %r" % (N, thr), log_odds=True)
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [256, 257, 513])
def test_particle_planes_at_the_workgroup_boundary(pkg, N):
    rng = np.random.default_rng(N)
    f = pkg.RBPHDFilter(N, gm_capacity=8, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    f.handle_serve_estimates(True)
    w = rng.uniform(0.05, 1.0, N)
    x = np.column_stack([rng.normal(0, 30, (N, 2)), rng.uniform(-np.pi, np.pi, N)])
    f.set_weights(w)
    f.set_poses(x)
    h, G, P = _one_row(f, 0.25, THR, 8, particles=True)
    assert int(h["n_particles"]) == N and P.shape == (4, N)
    for q, v in enumerate((x[:, 0], x[:, 1], x[:, 2], w)):
        assert _same(P[q, :N], v), q
    h0, _, P0 = _one_row(f, 0.25, THR, 8, particles=False)
    assert P0 is None and h0.tobytes() == h.tobytes()
    f.close()


# ---- GPU: rows behind pending device cycles ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,model", [(2, "2d"), (65, "2d"), (2, "vp"), (65, "vp")])
def test_rows_behind_pending_rbphd_cycles(pkg, sc, n, model):
    """Four cycles -- gate closed, open without firing, fired, closed again -- with a row behind each: nothing waited, the rows equal
    those of the host-stop route byte for byte, and the handle ends where a handle without a log ends."""
    scen = sc.make_vp_scenario(n, 4, 4, seed=31) if model == "vp" else sc.make_scenario(n, 3, 4, seed=31)
    host, dev = rb.make_pair(pkg, sc, scen, 1, 2, 0.0, 0.0)
    other, plain = rb.make_pair(pkg, sc, scen, 1, 2, 0.0, 0.0)
    other.f.close()
    rz = np.random.default_rng(9)
    Zs = [scen["Z"] + rz.normal(0, 1e-3, scen["Z"].shape) for _ in range(4)]
    eff = [(0.0, 0.0), (0.0, 0.0), (n + 1.0, 0.0), (n + 1.0, 0.0)]
    draws = [0.37, 0.81, 0.12, 0.55]
    for f in (host.f, dev):
        f.handle_serve_estimates(True)
        f.estimate_log_create(4, CAP, True)
    outcomes = []
    for k in range(4):
        host.eff_n, host.eff_pct = eff[k]
        h = host.update(Zs[k], draws[k], scan=scen.get("scan"))
        outcomes.append((h["gate_open"], h["fired"]))
        host.f.step_estimate_async(0.1 * (k + 1), -np.inf)
        for f in (dev, plain):
            f.rbphd_set_resampling(*eff[k])
            rb.device_update(f, Zs[k], draws[k], scan=scen.get("scan"))
        dev.step_estimate_async(0.1 * (k + 1), -np.inf)
        assert dev.rbphd_cycle_pending(), "the row resolved the pending cycles"
    assert outcomes == [(False, False), (True, False), (True, True), (False, False)]
    assert dev.rbphd_cycle_pending()
    rows_host, rows_dev = host.f.estimate_log_read(), dev.estimate_log_read()
    assert not dev.rbphd_cycle_pending()
    assert rows_dev[0].shape == (4, 1) and (rows_dev[0]["n_particles"] == n).all() and (rows_dev[0]["status"] == 0).all()
    _same_rows(rows_host, rows_dev)
    assert len({rows_dev[0]["weight_sum"][k, 0].tobytes() + rows_dev[1][k].tobytes() for k in range(4)}) == 4      # the rows follow the updates
    rb.assert_same_state(rb.state(dev), rb.state(plain))
    rb.assert_same_state(rb.state(dev), rb.state(host.f))
    host.f.close(); dev.close(); plain.close()


def _mh_rows(pkg, sc, host, dev, Zs, draws, scan=None):
    """The same updates on the host-stop route (a row after each) and as device cycles (a row behind each, nothing resolved)."""
    for f in (host, dev):
        f.handle_serve_estimates(True)
        f.estimate_log_create(len(Zs), f.gm_capacity, True)
    counts = []
    for k, (Z, u) in enumerate(zip(Zs, draws)):
        dev.cycle_async(Z, u, predict=True)
        dev.step_estimate_async(0.5 * (k + 1), -np.inf)
        assert dev.fastslam_cycle_pending(), "the row took the particle count over"
    for k, (Z, u) in enumerate(zip(Zs, draws)):
        host.predict_map()
        host.update_and_resample(Z, u01_fn=lambda: u)
        counts.append(host.n)
        host.step_estimate_async(0.5 * (k + 1), -np.inf)
    assert dev.fastslam_cycle_pending()
    rows_host, rows_dev = host.estimate_log_read(), dev.estimate_log_read()
    assert not dev.fastslam_cycle_pending()
    assert [int(v) for v in rows_dev[0]["n_particles"][:, 0]] == counts, (rows_dev[0]["n_particles"][:, 0], counts)
    assert (rows_dev[0]["status"] == 0).all() and (rows_dev[0]["n_est"] > 0).all()
    _same_rows(rows_host, rows_dev)
    assert rows_dev[2].shape[-1] == dev.max_particles
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("hyp", [3, 1])
def test_rows_behind_victoria_park_fastslam_cycles(pkg, sc, hyp):
    """8 particles, 48 slots: a three-hypothesis update grows the set and nParticlesMax 16 forces it back; each row's n_particles is the
    device's count behind that update's resampling."""
    scen = sc.make_vp_scenario(n_particles=8, n_landmarks=12, n_z=8, seed=112, scan="const")
    host, dev = vpref.make_pair(pkg, sc, scen, hyp, 2, 0, 48)
    for f in (host, dev):
        f.fs_config.nParticlesMax = 16
    rz = np.random.default_rng(4)
    Zs = [scen["Z"] + rz.normal(0, 3e-3, scen["Z"].shape) for _ in range(3)]
    counts = _mh_rows(pkg, sc, host, dev, Zs, [0.11, 0.52, 0.93])
    print("hypotheses %d: counts behind the updates %r" % (hyp, counts))
    assert all(1 <= c <= 16 for c in counts)
    vpref.assert_same_state(vpref.state(host), vpref.state(dev))
    host.close(); dev.close()


def _mh_pair(pkg, sc, scen, hyp, cap):
    out = []
    for dc in (False, True):
        f = pkg.FastSLAM(scen["n"], gm_capacity=64, max_hypotheses=max(hyp, 2), n_particles_max=cap // max(hyp, 2), device_cycle=dc)
        mh.load(f, sc, scen, hyp, 50.0)
        out.append(f)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("hyp", [2, 1])
def test_rows_behind_2d_fastslam_cycles(pkg, sc, hyp):
    """rfsgpu_fastslam_cycle_async, five cycles back to back (one with an empty scan): 8 -> 16 stays, 16 -> 32 is forced back to 8."""
    scen = mh.crowded(sc, 8)
    host, dev = _mh_pair(pkg, sc, scen, hyp, 32)
    assert not dev.uses_full_cycle()
    rz = np.random.default_rng(4)
    Zs = [scen["Z"] + rz.normal(0, 3e-3, scen["Z"].shape) for _ in range(5)]
    Zs[3] = np.zeros((0, 2))
    for f in (host, dev):
        f.fs_config.minUpdatesBeforeResample = 2
    counts = _mh_rows(pkg, sc, host, dev, Zs, [0.11, 0.52, 0.93, 0.34, 0.75])
    print("hypotheses %d: counts behind the updates %r" % (hyp, counts))
    if hyp == 2:
        assert counts == [16, 8, 16, 16, 8]
    mh.assert_same_state(mh.state(host), mh.state(dev))
    host.close(); dev.close()


@pytest.mark.gpu
def test_row_behind_an_overflowed_cycle_has_status_2(pkg, sc):
    """4 particles with 4 hypotheses each into 15 slots: the cycle is abandoned.  The row behind it reads nothing of the filter, the
    error comes out of the next synchronising call once, and the row after that is the row from before the cycle."""
    n0, hyp, cap = 4, 4, 15
    scen = mh.crowded(sc, n0)
    dev = pkg.RBPHDFilter(n0, gm_capacity=64, max_particles=cap)
    sc.load_scenario(dev, scen)
    for i in range(n0):
        dev.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
    cfg = dev.default_fastslam_config()
    cfg.maxNDataAssocHypotheses = hyp
    cfg.maxDataAssocLogLikelihoodDiff = 50.0
    cfg.minUpdatesBeforeResample = 1000
    cfg.nParticlesMax = cap
    dev.set_fastslam_config(cfg)
    dev.fastslam_update(np.zeros((0, 2)))                                  # a FastSLAM handle from the first row on
    dev.handle_serve_estimates(True)
    dev.estimate_log_create(4, 64, True)
    before = mh.state(dev)
    dev.step_estimate_async(0.0, -np.inf)
    dev.fastslam_cycle_async(scen["Z"], 0.5, n0)
    dev.step_estimate_async(1.0, -np.inf)
    assert dev.fastslam_cycle_pending()
    _raises(pkg, pkg.capi.ERR_CAPACITY, lambda: dev.estimate_log_read(), "max_particles")
    dev.synchronize()                                                      # reported once
    dev.step_estimate_async(2.0, -np.inf)
    hdr, gauss, part = dev.estimate_log_read()
    assert hdr.shape == (3, 1) and [int(v) for v in hdr["status"][:, 0]] == [0, 2, 0]
    bad = hdr[1, 0]
    assert bad["t"] == 1.0 and (int(bad["n_particles"]), int(bad["n_est"]), int(bad["n_logged"]), int(bad["best_slot"])) == (0, 0, 0, 0)
    assert float(bad["cardinality"]) == 0.0 and float(bad["best_weight"]) == 0.0 and float(bad["weight_sum"]) == 0.0
    assert all(np.isnan(float(bad[k])) for k in ("best_x", "best_y", "best_theta", "mean_x", "mean_y", "mean_cos", "mean_sin"))
    assert not gauss[1].any() and not part[1].any()
    assert int(hdr["n_particles"][0, 0]) == n0 and int(hdr["n_est"][0, 0]) == len(scen["w"][int(hdr["best_slot"][0, 0])])
    for k in hdr.dtype.names:
        if k != "t":
            assert hdr[0, 0][k].tobytes() == hdr[2, 0][k].tobytes(), k   # the state is the one before the abandoned cycle
    assert _same(gauss[0], gauss[2]) and _same(part[0], part[2])
    mh.assert_same_state(before, mh.state(dev))
    dev.close()


@pytest.mark.gpu
def test_full_log_enqueues_nothing_and_drains_in_chunks(pkg, sc):
    scen = sc.make_vp_scenario(5, 4, 4, seed=31)
    f = pkg.RBPHDFilter(5, gm_capacity=64, model=pkg.capi.MODEL_VICTORIAPARK_3D)
    sc.load_scenario(f, scen)
    f.handle_serve_estimates(True)
    f.rbphd_set_resampling(0.0, 0.0)
    f.estimate_log_create(2, 64, True)
    for k in range(2):
        rb.device_update(f, scen["Z"], 0.5, scan=scen["scan"])
        f.step_estimate_async(float(k), -np.inf)
    _raises(pkg, pkg.capi.ERR_CAPACITY, lambda: f.step_estimate_async(2.0, -np.inf), "full")
    assert f.rbphd_cycle_pending()                                         # the refused call resolved nothing either
    first = f.estimate_log_read()
    assert list(first[0]["t"][:, 0]) == [0.0, 1.0]
    f.estimate_log_reset()
    rb.device_update(f, scen["Z"], 0.5, scan=scen["scan"])
    f.step_estimate_async(2.0, -np.inf)
    second = f.estimate_log_read()
    assert list(second[0]["t"][:, 0]) == [2.0] and not _same(second[1][0], first[1][1])
    _raises(pkg, pkg.capi.ERR_INVALID, lambda: f.estimate_log_create(2, 65))       # max_est stays within 0 ... gm_capacity
    f.close()


# ---- GPU: the drivers ------------------------------------------------------------------------------------------------------------------

def _extract():
    return np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))


def _driver(pkg, sc, kind, hyp, **opts):
    n = 16
    VP = pkg.capi.MODEL_VICTORIAPARK_3D
    P = dict(sc.VP_PARAMS)
    if kind == "rbphd":
        f = pkg.RBPHDFilter(n, gm_capacity=192, model=VP)
        sc.apply_vp_params(f, P, np.full(361, 70.0))
        return pkg.vp_driver.VictoriaParkRun(f, _extract(), P, seed=5, filter="rbphd", log_estimates=True, **opts).run(n_messages=300)
    f = pkg.RBPHDFilter(n, gm_capacity=192, model=VP, max_particles=(48 * 3 if hyp > 1 else n))
    sc.apply_vp_params(f, P, np.full(361, 70.0))
    cfg = f.default_fastslam_config()
    cfg.minLogMeasurementLikelihood = -15.0
    cfg.mapExistencePruneThreshold = -5.0
    cfg.landmarkCandidateMeasurementCountThreshold = 4 if hyp > 1 else 3
    cfg.landmarkCandidateCurrentMeasurementCountThreshold = 0
    cfg.landmarkCandidateMeasurementCheckThreshold = 5
    cfg.landmarkCandidateMeasurementSupportDist = 3.0
    cfg.maxNDataAssocHypotheses = hyp
    cfg.maxDataAssocLogLikelihoodDiff = 3.0
    f.set_fastslam_config(cfg)
    return pkg.vp_driver.VictoriaParkRun(f, _extract(), P, seed=5, filter="fastslam", max_hypotheses=hyp, n_particles_max=(48 if hyp > 1 else n),
                                         log_estimates=True, **opts).run(n_messages=300)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,hyp", [("rbphd", 1), ("fastslam", 1), ("fastslam", 3)])
def test_python_driver_device_log_equals_the_host_stop_routes_files(pkg, sc, tmp_path, kind, hyp):
    """The first 300 messages of the Victoria Park extract, 16 particles: the device cycle with the device log against the host-stop
    route of the same realisation, through write_vp_logs."""
    host = _driver(pkg, sc, kind, hyp, device_motion=True, draw_every_update=True)
    dev = _driver(pkg, sc, kind, hyp, device_cycle=True)
    eh, ed = host.estimates(), dev.estimates()
    n_lidar_msgs = int(sum(1 for m in _extract()["manager"][:300] if m[1] == 3))
    assert ed[0].shape == (1 + n_lidar_msgs, 1) and dev.n_lidar == host.n_lidar > 10
    assert int(ed[0]["n_logged"][0, 0]) == 0 and int(ed[0]["n_particles"][0, 0]) == 16       # the row before the loop
    assert int(ed[0]["n_logged"].max()) > 3 and (ed[0]["status"] == 0).all()
    print("%s hyp %d: %d rows, counts %d ... %d, largest map %d" % (kind, hyp, ed[0].shape[0], ed[0]["n_particles"].min(), ed[0]["n_particles"].max(), ed[0]["n_logged"].max()))
    files = [pkg.vp_driver.write_vp_logs(str(tmp_path / d), e) for d, e in (("host", eh), ("dev", ed))]
    for a, b in zip(*files):
        ta, tb = open(a, "rb").read(), open(b, "rb").read()
        assert ta == tb and len(ta) > 0, os.path.basename(a)
    _same_rows(eh, ed)
    host.f.close(); dev.f.close()


@pytest.mark.gpu
def test_cpp_driver_device_log_writes_the_getter_routes_files(pkg, tmp_path):
    """rbphdslam_vp --device-cycle -o A against --device-cycle --device-log -o B: the two log files byte for byte."""
    pkg.build_mod.build_host()
    dirs = []
    for name, extra in (("getters", []), ("devlog", ["--device-log"])):
        d = os.path.join(tmp_path, name)
        os.makedirs(d)
        dirs.append(d)
        cmd = [pkg.build_mod.SIM_VP, "-c", os.path.join(ROOT, "tests", "golden", "rbphdslam_VictoriaPark_c4.xml"), "-d", os.path.join(ROOT, "tests", "golden", "vp_extract"),
               "-n", "32", "-m", "300", "--device-cycle", "-o", d] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
        assert ("device log: read and printed once" in out.stdout) == bool(extra)
    for nm in ("particlePose.dat", "landmarkEst.dat", "finalMap.dat"):
        a, b = (open(os.path.join(d, nm), "rb").read() for d in dirs)
        assert a == b and len(a) > 0, nm
    out = subprocess.run([pkg.build_mod.SIM_VP, "-c", os.path.join(ROOT, "tests", "golden", "rbphdslam_VictoriaPark_c4.xml"), "-d", os.path.join(ROOT, "tests", "golden", "vp_extract"),
                          "-n", "32", "-m", "300", "--device-log", "-o", dirs[0]],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--device-log goes with --device-cycle" in out.stderr
