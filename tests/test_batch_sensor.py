"""The device sensor of a filter batch (include/rfsgpu.h [sensor]; csrc/batch_sensor.h): rfsgpu_batch_set_sensor /
rfsgpu_batch_sense_async / rfsgpu_batch_last_scan against the numpy restatement of tests/support/sensor_reference.py, the restatement
against the reference's own loop and its statistics, and the refusals of the section."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import sensor_reference as sr

SENSOR_SYMBOLS = ["rfsgpu_batch_set_sensor", "rfsgpu_batch_sense_async", "rfsgpu_batch_cycle_sensed_async", "rfsgpu_batch_resample_sensed_async",
                  "rfsgpu_batch_last_scan", "rfsgpu_batch_last_cycle_lds"]
CALLS = (0, 1, 7, 1 << 33)
DENSE = 12.0 / (2 * math.pi * 2.0)        # clutter intensity whose mean over [0.5, 2.5] is 12
R_DIAG = np.diag([5e-4, 5e-5])
R_FULL = np.array([[5e-4, 1e-4], [1e-4, 5e-5]])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_sensor_section_and_the_library_exports_it(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    assert "[sensor]" in head
    sec = txt.index("---- [sensor]")
    for s in SENSOR_SYMBOLS:
        assert s not in core.replace("[sensor]", ""), s
        assert sec < txt.index(s + "("), s
        assert s[len("rfsgpu_"):] in pkg.capi.ABI_SYMBOLS
    assert re.search(r"#define RFSGPU_SENSOR_MAX_LANDMARKS\s+512\b", txt)
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in SENSOR_SYMBOLS:
        assert hasattr(lib, s), s
    for m in ("set_sensor", "sense_async", "cycle_sensed_async", "resample_sensed_async", "last_scan"):
        assert callable(getattr(pkg.capi.CBatch, m))


def _reference_cmf_loop(meanClutter):
    """src/rbphdslam2dSim.cpp:294-306, line for line."""
    expNegMeanClutter = math.exp(-meanClutter)
    poissonPmf = [0.0] * 100
    poissonCmf = [0.0] * 100
    mean_pow_i = 1.0
    i_factorial = 1.0
    poissonPmf[0] = expNegMeanClutter
    poissonCmf[0] = poissonPmf[0]
    for i in range(1, 100):
        mean_pow_i *= meanClutter
        i_factorial *= i
        poissonPmf[i] = mean_pow_i / i_factorial * expNegMeanClutter
        poissonCmf[i] = poissonCmf[i - 1] + poissonPmf[i]
    return poissonCmf


def test_restated_poisson_table_is_the_reference_loop():
    for mean in (0.0, 1e-4 * 2 * math.pi * 2, 12.6):
        want = _reference_cmf_loop(mean)
        got = sr.poisson_cmf(mean)
        assert got.shape == (100,) and [float(v) for v in got] == want
        assert np.all(np.diff(got) >= 0)
    cmf0 = sr.poisson_cmf(0.0)
    for u in (0.0, 0.25, 1.0 - 2.0 ** -53):
        assert sr.clutter_count(u, cmf0) == 0
    assert sr.mean_clutter(1e-4, 0.5, 2.5) == 1e-4 * (2 * math.pi * 2.0)
    # the walk is capped where the reference would leave its table
    assert sr.clutter_count(2.0, sr.poisson_cmf(3.0)) == 99


def test_restated_scans_have_the_clutter_mean_and_the_detection_rate():
    """20 000 scans of one landmark well inside the limits: the clutter count's mean against the Poisson mean, the detection rate
    against Pd, each within four standard errors."""
    n, Pd, mean = 20000, 0.7, 3.0
    clutter = mean / (2 * math.pi * 2.0)
    lm = np.array([[1.5, 0.0]])
    args = ((0.0, 0.0, 0.3), lm, R_DIAG, Pd, clutter, 0.5, 2.5, 0xC0FFEE)
    n_d, n_c = sr.scan_counts(*args, np.arange(n))
    for call in range(40):                      # the many-call form is the per-call restatement
        Z, info = sr.scan(*args, call, max_nz=64)
        assert (info["n_det"], info["n_clutter"]) == (n_d[call], n_c[call]) and len(Z) == n_d[call] + n_c[call]
    assert abs(n_c.mean() - mean) < 4 * math.sqrt(mean / n), n_c.mean()
    assert abs(n_d.mean() - Pd) < 4 * math.sqrt(Pd * (1 - Pd) / n), n_d.mean()


def test_generate_without_measurements_leaves_everything_else_as_it_was(pkg):
    sim = pkg.sim2d_driver
    full = sim.generate(sim.C1_SIM, traj_seed=3, kmax=120)
    bare = sim.generate(sim.C1_SIM, traj_seed=3, kmax=120, measurements=False)
    assert bare["Z"] is None and bare["K"] == full["K"] == 120 and len(full["Z"]) == 120
    for key in ("gt", "odom", "landmarks"):
        np.testing.assert_array_equal(bare[key], full[key], err_msg=key)


def test_the_drivers_scan_bound_holds_for_the_restated_scans(pkg):
    """sim2d_driver.sensor_max_nz (what Sim2dBatchRun passes as max_nz): no restated scan of the run exceeds it, and it stays below
    RFSGPU_MAX_Z where the scans are small -- the step kernel's launch is sized by it."""
    sim = pkg.sim2d_driver
    for b, (pd, c) in enumerate(((0.99, 1e-4), (0.6, 1e-1), (1.0, 2e-2))):
        P = dict(sim.C1_SIM, kmax=60, Pd=pd, clutter=c)
        d = sim.generate(P, traj_seed=5 + b, kmax=60, measurements=False)
        bound = sim.sensor_max_nz(d, P)
        worst = 0
        for k in range(1, 60):
            _, info = sr.scan(d["gt"][k], d["landmarks"], np.diag([P["varzr"], P["varzb"]]), pd, c, P["rmin"], P["rmax"], 100 + b, k)
            worst = max(worst, info["n_det"] + info["n_clutter"])
        assert 0 < worst <= bound <= 64, (worst, bound)
    empty = dict(gt=np.zeros((5, 3)), landmarks=np.zeros((0, 2)))
    assert sim.sensor_max_nz(empty, dict(sim.C1_SIM, clutter=0.0)) == 2                  # nothing to see: the margin alone
    dense = sim.sensor_max_nz(empty, dict(sim.C1_SIM, clutter=12.0 / (4 * math.pi)), margin=0)      # clutter mean 12
    cmf = sr.poisson_cmf(12.0)
    assert cmf[dense] >= 1 - 2.0 ** -40 > cmf[dense - 1]                                 # the first count whose CMF leaves 2^-40 above it


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cases():
    """Six sensors: landmark counts at and around the wavefront, Pd 0 / 0.5 / 1, clutter mean 0 / tiny / 12, rmin 0 and 0.5, one
    non-diagonal R.  Landmarks uniform in a square around the origin (part of them beyond the limits)."""
    rng = np.random.default_rng(2024)
    spec = [dict(nL=0, Pd=0.5, clutter=DENSE, rmin=0.5, R=R_DIAG, half=3.0),
            dict(nL=1, Pd=1.0, clutter=0.0, rmin=0.0, R=R_DIAG, half=1.0),
            dict(nL=63, Pd=0.5, clutter=DENSE, rmin=0.5, R=R_DIAG, half=3.0),
            dict(nL=64, Pd=0.0, clutter=0.0, rmin=0.5, R=R_DIAG, half=3.0),
            dict(nL=65, Pd=1.0, clutter=0.0, rmin=0.0, R=R_DIAG, half=3.0),
            dict(nL=130, Pd=0.5, clutter=1e-4, rmin=0.5, R=R_FULL, half=4.0)]
    for q, s in enumerate(spec):
        s["lm"] = rng.uniform(-s["half"], s["half"], (s["nL"], 2))
        s["rmax"] = 2.5
        s["seed"] = [11, 0x1234567890ABCDEF, 77, 2 ** 64 - 1, 5, 0xDEADBEEF00000001][q]
    return spec


def _set(batch, b, s, max_nz=64):
    batch.set_sensor(b, s["R"], s["Pd"], s["clutter"], s["rmax"], s["rmin"], s["lm"], max_nz=max_nz, seed=s["seed"])


def _restated(s, pose, call, max_nz=64):
    return sr.scan(pose, s["lm"], s["R"], s["Pd"], s["clutter"], s["rmin"], s["rmax"], s["seed"], call, max_nz=max_nz)


@pytest.mark.gpu
def test_scans_match_the_restatement(pkg):
    spec = _cases()
    nF = len(spec)
    rng = np.random.default_rng(99)
    poses = {call: np.column_stack([rng.uniform(-0.3, 0.3, nF), rng.uniform(-0.3, 0.3, nF), rng.uniform(-np.pi, np.pi, nF)]) for call in CALLS}
    # condition, on the restatement alone: no decision hangs on a range nearer than 1e-9 (ten times the value bound) to a limit
    want = {}
    for call in CALLS:
        for b, s in enumerate(spec):
            Z, info = _restated(s, poses[call][b], call)
            assert not info["cut"]
            for lim in (s["rmin"], s["rmax"]):
                assert info["ranges"].size == 0 or np.abs(info["ranges"] - lim).min() > 1e-9, (call, b)
            want[call, b] = Z
    assert max(len(want[c, 2]) for c in CALLS) > 12 and max(len(want[c, 5]) for c in CALLS) > 12      # detections and clutter, several chunks
    assert all(len(want[c, 0]) > 0 for c in CALLS) and all(len(want[c, 3]) == 0 for c in CALLS)
    batch = pkg.FilterBatch(nF, 4, gm_capacity=16)
    for b, s in enumerate(spec):
        _set(batch, b, s)
    got = {}
    for call in CALLS:
        batch.sense_async(poses[call], call)
        scans = batch.last_scan()
        for b in range(nF):
            got[call, b] = scans[b]
            assert scans[b].shape == want[call, b].shape, f"call {call} filter {b}: {len(scans[b])} entries, restated {len(want[call, b])}"
            np.testing.assert_allclose(scans[b], want[call, b], rtol=1e-10, atol=1e-10, err_msg=f"call {call} filter {b}")
    # a scan does not depend on the filter's place in the batch, nor on the others: block 0 ... 2 and 5 of this batch as blocks of another
    other = pkg.FilterBatch(5, 7, gm_capacity=16)
    place = {3: 0, 1: 2, 4: 5}                    # block of `other` -> sensor of `spec`
    for b in range(5):
        if b in place:
            _set(other, b, spec[place[b]])
        else:
            other.set_sensor(b, R_DIAG * 4, 0.8, 0.3, 3.0, 0.1, rng.uniform(-2, 2, (20, 2)), seed=4242 + b)
    call = 1 << 33
    po = np.column_stack([rng.uniform(-0.3, 0.3, 5), rng.uniform(-0.3, 0.3, 5), rng.uniform(-np.pi, np.pi, 5)])
    for b, q in place.items():
        po[b] = poses[call][q]
    other.sense_async(po, call)
    so = other.last_scan()
    for b, q in place.items():
        np.testing.assert_array_equal(_bits(so[b]), _bits(got[call, q]), err_msg=f"sensor {q} at block {b}")
    assert len(so[3]) > 0


@pytest.mark.gpu
def test_a_scan_beyond_max_nz_is_cut_and_reported_once(pkg):
    max_nz = 8
    ang = np.linspace(0.1, 5.0, max_nz + 1)
    lm = np.column_stack([1.5 * np.cos(ang), 1.5 * np.sin(ang)])          # well inside [0.5, 2.5]: Pd 1 keeps every one
    s = dict(R=R_DIAG, Pd=1.0, clutter=0.0, rmin=0.5, rmax=2.5, seed=31337)
    pose = np.array([[0.0, 0.0, 0.0], [0.05, -0.02, 0.4]])
    batch = pkg.FilterBatch(2, 4, gm_capacity=16)
    batch.set_sensor(0, R_DIAG, 0.5, 0.0, 2.5, 0.5, lm, max_nz=64, seed=1)
    batch.set_sensor(1, s["R"], s["Pd"], s["clutter"], s["rmax"], s["rmin"], lm[:max_nz], max_nz=max_nz, seed=s["seed"])
    batch.sense_async(pose, 3)
    batch.synchronize()                                                    # exactly max_nz entries: not flagged
    scans = batch.last_scan()
    want, info = sr.scan(pose[1], lm[:max_nz], s["R"], 1.0, 0.0, 0.5, 2.5, s["seed"], 3, max_nz=max_nz)
    assert len(want) == max_nz and not info["cut"] and len(scans[1]) == max_nz
    np.testing.assert_allclose(scans[1], want, rtol=1e-10, atol=1e-10)
    batch.set_sensor(1, s["R"], s["Pd"], s["clutter"], s["rmax"], s["rmin"], lm, max_nz=max_nz, seed=s["seed"])     # one more landmark
    batch.sense_async(pose, 3)
    with pytest.raises(pkg.capi.EngineError) as e:
        batch.synchronize()
    assert e.value.status == pkg.capi.ERR_CAPACITY and "filter 1" in str(e.value) and "scan" in str(e.value)
    batch.synchronize()                                                    # reported once
    scans = batch.last_scan()
    full, info = sr.scan(pose[1], lm, s["R"], 1.0, 0.0, 0.5, 2.5, s["seed"], 3, max_nz=max_nz)
    assert info["cut"] and info["n_det"] == max_nz + 1 and len(scans[1]) == max_nz
    np.testing.assert_allclose(scans[1], full, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(scans[1], want, rtol=1e-10, atol=1e-10)     # the first max_nz: the same landmarks as before


def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


def _section_calls(capi, f, nF):
    """Every call of the section on handle f through the raw ABI (a handle that is no CBatch has no wrappers for them)."""
    m = C
    rb = capi.RngBrgConfig()
    rb.R[0], rb.R[3] = 5e-4, 5e-5
    rb.probabilityOfDetection, rb.uniformClutterIntensity, rb.rangeLimMax, rb.rangeLimMin = 0.9, 0.0, 2.5, 0.5
    lm = np.array([[1.0, 0.0]])
    g = np.zeros((nF, 3))
    z = np.zeros((nF, capi.MAX_Z, 2))
    nz = np.zeros(nF, dtype=np.int32)
    p = f._ptr
    return [lambda: f._call("batch_set_sensor", m.c_int(-1), m.byref(rb), p(lm), m.c_int(1), m.c_int(8), m.c_ulonglong(1)),
            lambda: f._call("batch_sense_async", p(g), m.c_ulonglong(1)),
            lambda: f._call("batch_cycle_sensed_async", m.c_int(1), m.c_void_p(None), m.c_void_p(None), m.c_int(0), m.c_int(1)),
            lambda: f._call("batch_resample_sensed_async", m.c_ulonglong(1)),
            lambda: f._call("batch_last_scan", p(z), p(nz))]


@pytest.mark.gpu
def test_the_section_refuses_what_it_does_not_serve(pkg):
    U = pkg.capi.ERR_UNSUPPORTED
    single = pkg.RBPHDFilter(8, gm_capacity=16)
    group = pkg.FilterGroup(16, [0, 0], gm_capacity=16)
    fs = pkg.FastSLAMBatch(2, 4, gm_capacity=16)
    fs.configure_fastslam(0, pkg.sim2d_driver.fastslam_config(fs))
    mh = pkg.MHFastSLAMBatch(2, 4, gm_capacity=16)
    for f, nF, what in ((single, 1, "ordinary handle"), (group.shards[0], 1, "shard"), (fs, 2, "FastSLAM"), (mh, 2, "multi-hypothesis")):
        w0 = f.get_weights().copy()
        for call in _section_calls(pkg.capi, f, nF):
            _raises(pkg, U, call, what)
        np.testing.assert_array_equal(f.get_weights(), w0)
    group.close()


@pytest.mark.gpu
def test_invalid_sensor_configurations_and_call_orders_leave_the_state_untouched(pkg):
    I, U = pkg.capi.ERR_INVALID, pkg.capi.ERR_UNSUPPORTED
    nF, nP = 2, 8
    lm = np.array([[1.0, 0.2], [-1.2, 0.8], [0.3, -1.6]])
    pose = np.zeros((nF, 3))
    batch = pkg.FilterBatch(nF, nP, gm_capacity=32)
    batch.set_motion_odometry(None, [1e-4, 1e-4, 1e-4], 9)
    batch.set_resampling(None, 4.0, 0.5)
    batch.set_sensor(0, R_DIAG, 1.0, 0.0, 2.5, 0.5, lm, seed=5)
    # a filter without a sensor: named by the sense call and by the sensed cycle
    _raises(pkg, I, lambda: batch.sense_async(pose, 1), "filter 1", "rfsgpu_batch_set_sensor")
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "filter 1")
    batch.set_sensor(1, R_DIAG, 1.0, 0.0, 2.5, 0.5, lm[:2], seed=6)
    # no sense call yet / none since the last cycle
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "rfsgpu_batch_sense_async", "filter")
    _raises(pkg, I, lambda: batch.resample_sensed_async(1), "rfsgpu_batch_cycle_sensed_async")
    batch.sense_async(pose, 1)
    ref = [z.copy() for z in batch.last_scan()]
    assert [len(z) for z in ref] == [3, 2]
    # invalid configurations: refused with a message, the sensor stays as it was
    bad = [dict(R=np.diag([-1.0, 1.0])), dict(R=np.array([[1.0, 2.0], [2.0, 1.0]])), dict(R=np.zeros((2, 2))), dict(rmin=2.5), dict(rmin=3.0),
           dict(Pd=1.5), dict(Pd=-0.1), dict(Pd=float("nan")), dict(clutter=-1e-3), dict(max_nz=0), dict(max_nz=65), dict(lm=np.zeros((513, 2))), dict(b=2)]
    for kw in bad:
        a = dict(b=0, R=R_DIAG, Pd=1.0, clutter=0.0, rmax=2.5, rmin=0.5, lm=lm, max_nz=64)
        a.update(kw)
        with pytest.raises(pkg.capi.EngineError) as e:
            batch.set_sensor(a["b"], a["R"], a["Pd"], a["clutter"], a["rmax"], a["rmin"], a["lm"], max_nz=a["max_nz"], seed=77)
        assert e.value.status == I and "batch_set_sensor" in str(e.value), (kw, str(e.value))
    batch.sense_async(pose, 1)
    for z, w in zip(batch.last_scan(), ref):
        np.testing.assert_array_equal(_bits(z), _bits(w))
    # sense -> set_sensor (a smaller max_nz than the records on the device hold) -> cycle_sensed: the sense call's validity has ended,
    # the cycle is refused until the next one and nothing has moved
    w0, s0, m0 = batch.get_weights().copy(), batch.gm_sizes().copy(), batch.get_unused_masks().copy()
    batch.set_sensor(1, R_DIAG, 1.0, 0.0, 2.5, 0.5, lm[:2], max_nz=1, seed=6)
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "rfsgpu_batch_sense_async")
    np.testing.assert_array_equal(_bits(batch.get_weights()), _bits(w0))
    np.testing.assert_array_equal(batch.gm_sizes(), s0)
    np.testing.assert_array_equal(batch.get_unused_masks(), m0)
    for z, w in zip(batch.last_scan(), ref):                               # (the sets of that sense call are still there to be read)
        np.testing.assert_array_equal(_bits(z), _bits(w))
    batch.set_sensor(1, R_DIAG, 1.0, 0.0, 2.5, 0.5, lm[:2], seed=6)
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "rfsgpu_batch_sense_async")
    # sense -> a configuration with another evaluation-point count -> cycle_sensed: the record carries the old cap, the filter is named
    batch.sense_async(pose, 1)
    cfg = batch.default_filter_config()
    n_eval = cfg.importanceWeightingEvalPointCount
    cfg.importanceWeightingEvalPointCount = n_eval + 3
    batch.configure(1, cfg)
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "filter 1", "importanceWeightingEvalPointCount")
    np.testing.assert_array_equal(_bits(batch.get_weights()), _bits(w0))
    np.testing.assert_array_equal(batch.gm_sizes(), s0)
    cfg.importanceWeightingEvalPointCount = n_eval
    batch.configure(1, cfg)
    batch.sense_async(pose, 1)
    for z, w in zip(batch.last_scan(), ref):
        np.testing.assert_array_equal(_bits(z), _bits(w))
    # host-fed cycles before the first sensed one are served (and end the sense call's validity) ...
    batch.cycle_async(True, [np.zeros((0, 2))] * nF, normalize=True)
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "rfsgpu_batch_sense_async")
    batch.sense_async(pose, 2)
    batch.cycle_sensed_async(True, normalize=True)
    _raises(pkg, I, lambda: batch.cycle_sensed_async(True), "rfsgpu_batch_sense_async")      # one cycle per sense call
    batch.resample_sensed_async(2)
    batch.synchronize()
    # ... after it the host-fed cycle and resampling refuse: the host no longer knows nZprev
    w0, s0, m0, x0 = batch.get_weights().copy(), batch.gm_sizes().copy(), batch.get_unused_masks().copy(), batch.get_poses().copy()
    ids0 = batch.get_particle_ids()
    _raises(pkg, U, lambda: batch.cycle_async(True, ref, normalize=True), "sensed")
    _raises(pkg, U, lambda: batch.resample_async([3, 2], 3), "sensed")
    np.testing.assert_array_equal(_bits(batch.get_weights()), _bits(w0))
    np.testing.assert_array_equal(batch.gm_sizes(), s0)
    np.testing.assert_array_equal(batch.get_unused_masks(), m0)
    np.testing.assert_array_equal(_bits(batch.get_poses()), _bits(x0))
    for a, b in zip(batch.get_particle_ids(), ids0):
        np.testing.assert_array_equal(a, b)
