"""What every kind of handle answers to the calls that belong to one kind of batch: a table of handle kinds x entry points, each cell
the status code and, for a refusal, how the message begins and a name it must carry (the creator, or the call that serves the handle
instead; where the message names no call, the words that say what the handle is).  The expectations were taken from the library as
it stood before the batch's kind became one field (profiles/batch_kind_refactor.txt has that run), and hold for it and for every
library since: the names are those both wordings of a message share.

Rows: a fresh handle each -- an ordinary 2-D handle, an ordinary Victoria Park handle, a 2-D batch whose kind is open, after an RB-PHD
cycle, after rfsgpu_batch_set_fastslam_config, a 2-D multi-hypothesis batch, a Victoria Park batch, one with the FastSLAM switch on,
a Victoria Park multi-hypothesis batch; 2 filters x 4 particles (stride 8), every call through the C ABI with the same arguments.
The refused cells of a row are called on one handle, each leaving weights and live counts as they were; every accepted cell then
gets a handle of its own in the row's state (an accepted cycle or switch may close the row's other calls), followed by a
synchronisation that returns OK.  The measurement sets are empty, as the neighbouring tests show them on each path, except in the
Victoria Park FastSLAM cycle, where none does: its filters get the first measurement of their scene."""
import ctypes as C

import numpy as np
import pytest

from test_vp_filter_batch import _filter_params

OK, I, U = 0, "invalid", "unsupported"
NF, N_PER, STRIDE = 2, 4, 8
CAP2, CAP3 = 16, 64

CALLS = ("batch_cycle_async", "batch_fastslam_cycle_async", "batch_fastslam_mh_cycle_async", "batch_vp_cycle_async", "batch_vp_fastslam_cycle_async",
         "batch_vp_fastslam_mh_cycle_async", "batch_vp_serve_fastslam", "batch_fastslam_serve_sensor", "batch_vp_serve_estimates", "batch_resample_async")
NOT_BATCH = (I, "not a filter batch", "rfsgpu_create_batch")


def _na(call, name):
    return (U, "rfsgpu_" + call + " is not available on ", name)


# row -> one cell per call of CALLS: OK, or (status, the message's first words, a name in it)
TABLE = {
    "handle": (
        NOT_BATCH, NOT_BATCH, NOT_BATCH, NOT_BATCH,
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_fastslam_update"),
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_create_batch_vp_mh"),
        (U, "batch_vp_serve_fastslam: ", "rfsgpu_fastslam_update"),
        (U, "batch_fastslam_serve_sensor: ", "ordinary handle"),
        (U, "batch_vp_serve_estimates: ", "rfsgpu_handle_serve_estimates"),
        NOT_BATCH),
    "open": (
        OK, OK,
        (U, "batch_fastslam_mh_cycle: ", "rfsgpu_create_batch_mh"),
        (U, "batch_vp_cycle: ", "rfsgpu_batch_cycle_async"),
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_batch_fastslam_cycle_async"),
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_batch_cycle_async"),
        (U, "batch_vp_serve_fastslam: ", "rfsgpu_batch_set_fastslam_config"),
        (U, "batch_fastslam_serve_sensor: ", "rfsgpu_batch_set_fastslam_config"),
        (U, "batch_vp_serve_estimates: ", "rfsgpu_estimate_log_create"),
        OK),
    "rbphd": (
        OK,
        (U, "batch_fastslam_cycle: ", "rfsgpu_batch_cycle_async"),
        (U, "batch_fastslam_mh_cycle: ", "rfsgpu_create_batch_mh"),
        (U, "batch_vp_cycle: ", "rfsgpu_batch_cycle_async"),
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_batch_vp_serve_fastslam"),
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_batch_cycle_async"),
        (U, "batch_vp_serve_fastslam: ", "rfsgpu_create_batch"),
        (U, "batch_fastslam_serve_sensor: ", "RB-PHD"),
        (U, "batch_vp_serve_estimates: ", "rfsgpu_estimate_log_create"),
        OK),
    "fastslam": (
        (U, "batch_cycle: ", "rfsgpu_batch_fastslam_cycle_async"),
        OK,
        (U, "batch_fastslam_mh_cycle: ", "rfsgpu_create_batch_mh"),
        (U, "batch_vp_cycle: ", "rfsgpu_batch_fastslam_cycle_async"),
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_batch_fastslam_cycle_async"),
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_batch_fastslam_cycle_async"),
        (U, "batch_vp_serve_fastslam: ", "rfsgpu_create_batch"),
        OK,
        (U, "batch_vp_serve_estimates: ", "rfsgpu_estimate_log_create"),
        OK),
    "mh": (
        _na("batch_cycle_async", "rfsgpu_create_batch_mh"),
        _na("batch_fastslam_cycle_async", "rfsgpu_create_batch_mh"),
        OK,
        (U, "batch_vp_cycle: ", "rfsgpu_batch_fastslam_mh_cycle_async"),
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_batch_fastslam_mh_cycle_async"),
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_batch_fastslam_mh_cycle_async"),
        (U, "batch_vp_serve_fastslam: ", "rfsgpu_create_batch_mh"),
        OK,
        (U, "batch_vp_serve_estimates: ", "rfsgpu_batch_mh_serve_metrics"),
        _na("batch_resample_async", "rfsgpu_create_batch_mh")),
    "vp": (
        _na("batch_cycle_async", "rfsgpu_batch_vp_cycle_async"),
        _na("batch_fastslam_cycle_async", "rfsgpu_batch_vp_cycle_async"),
        (U, "batch_fastslam_mh_cycle: ", "rfsgpu_create_batch_mh"),
        OK,
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_batch_vp_cycle_async"),
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_batch_vp_cycle_async"),
        OK,
        (U, "batch_fastslam_serve_sensor: ", "Victoria Park"),
        OK,
        _na("batch_resample_async", "rfsgpu_batch_vp_cycle_async")),
    "vp_fastslam": (
        _na("batch_cycle_async", "rfsgpu_create_batch"),
        _na("batch_fastslam_cycle_async", "rfsgpu_create_batch"),
        (U, "batch_fastslam_mh_cycle: ", "rfsgpu_create_batch_mh"),
        (U, "batch_vp_cycle: ", "rfsgpu_batch_vp_fastslam_cycle_async"),
        OK,
        (U, "batch_vp_fastslam_mh_cycle: ", "rfsgpu_batch_vp_fastslam_cycle_async"),
        OK,
        (U, "batch_fastslam_serve_sensor: ", "Victoria Park"),
        (U, "batch_vp_serve_estimates: ", "rfsgpu_batch_vp_serve_fastslam"),
        _na("batch_resample_async", "rfsgpu_create_batch")),
    "vp_mh": (
        _na("batch_cycle_async", "rfsgpu_create_batch"),
        _na("batch_fastslam_cycle_async", "rfsgpu_create_batch"),
        (U, "batch_fastslam_mh_cycle: ", "rfsgpu_batch_vp_fastslam_mh_cycle_async"),
        (U, "batch_vp_cycle: ", "rfsgpu_batch_vp_fastslam_mh_cycle_async"),
        (U, "batch_vp_fastslam_cycle: ", "rfsgpu_batch_vp_fastslam_mh_cycle_async"),
        OK,
        (U, "batch_vp_serve_fastslam: ", "rfsgpu_create_batch"),
        (U, "batch_fastslam_serve_sensor: ", "Victoria Park"),
        (U, "batch_vp_serve_estimates: ", "multi-hypothesis"),
        _na("batch_resample_async", "rfsgpu_create_batch")),
}
TABLE["vp_handle"] = TABLE["handle"]
ROWS = ("handle", "vp_handle", "open", "rbphd", "fastslam", "mh", "vp", "vp_fastslam", "vp_mh")


def test_the_table_has_a_cell_for_every_call_of_every_kind():
    assert set(TABLE) == set(ROWS) and len(ROWS) == 9 and len(CALLS) == 10
    for row in ROWS:
        assert len(TABLE[row]) == len(CALLS), row
        for cell in TABLE[row]:
            assert cell == OK or (cell[0] in (I, U) and cell[1] and cell[2]), (row, cell)


def _vp_setup(sc, f):
    """Every filter's Victoria Park configuration and the batch's 361-beam constant scan; returns the scenes."""
    scens = [sc.make_vp_scenario(N_PER, 10, 8, seed=112 + b, scan="const", params=_filter_params(sc, b)) for b in range(NF)]
    for b, s in enumerate(scens):
        sc.apply_vp_batch_params(f, b, s["params"])
    assert scens[0]["scan"].shape == (361,) and np.ptp(scens[0]["scan"]) == 0.0
    f.set_laser_scan(scens[0]["scan"])
    return scens


def _make(pkg, sc, row):
    """A fresh handle in the row's state, and its filters' scenes where it has any."""
    VP = pkg.capi.MODEL_VICTORIAPARK_3D
    scens = None
    if row == "handle":
        f = pkg.RBPHDFilter(NF * N_PER, gm_capacity=CAP2)
    elif row == "vp_handle":
        f = pkg.RBPHDFilter(NF * N_PER, gm_capacity=CAP3, model=VP)
    elif row in ("open", "rbphd", "fastslam"):
        f = (pkg.FastSLAMBatch if row == "fastslam" else pkg.FilterBatch)(NF, N_PER, gm_capacity=CAP2)
        f.set_motion_odometry(None, np.full(3, 1e-4), 5)       # (so that the device resampling has its key and thresholds)
        f.set_resampling(None, N_PER / 4.0, 0.25)
        if row == "rbphd":
            f.cycle_async(True, [np.zeros((0, 2))] * NF, normalize=True)
        if row == "fastslam":
            f.configure_fastslam(0, pkg.sim2d_driver.fastslam_config(f))
    elif row == "mh":
        f = pkg.MHFastSLAMBatch(NF, N_PER, STRIDE, gm_capacity=CAP2)
    elif row == "vp":
        f = pkg.VPFilterBatch(NF, N_PER, gm_capacity=CAP3)
        scens = _vp_setup(sc, f)
    elif row == "vp_fastslam":
        f = pkg.VPFastSLAMBatch(NF, N_PER, gm_capacity=CAP3)
        scens = _vp_setup(sc, f)
    else:
        f = pkg.VPMHFastSLAMBatch(NF, N_PER, STRIDE, gm_capacity=CAP3)
        scens = _vp_setup(sc, f)
        f.configure_fastslam(None, f.fs_configs[0])           # (the class's default: three hypotheses)
    return f, scens


def _invoke(pkg, f, call, scens):
    """The call through the C ABI with the smallest valid arguments; returns (status, message)."""
    MAX_Z = pkg.capi.MAX_Z
    d = 3 if "_vp_" in call else 2
    z = np.zeros((NF, MAX_Z, d))
    nz = np.zeros(NF, dtype=np.int32)
    if call == "batch_vp_fastslam_cycle_async" and scens is not None:
        for b, s in enumerate(scens):
            z[b, 0], nz[b] = s["Z"][0], 1
    u01 = np.full(NF, 0.5)
    null, p = C.c_void_p(None), f._ptr
    poses = (C.c_int(0), null, null, C.c_int(0))                # predict 0, no new poses
    args = {"batch_cycle_async": poses + (p(z), p(nz), C.c_int(1)),
            "batch_fastslam_cycle_async": poses + (p(z), p(nz), C.c_int(1)),
            "batch_fastslam_mh_cycle_async": poses + (p(z), p(nz), p(u01)),
            "batch_vp_cycle_async": poses + (p(z), p(nz), null, C.c_int(0), C.c_int(1)),
            "batch_vp_fastslam_cycle_async": poses + (p(z), p(nz), null, C.c_int(0), C.c_int(1)),
            "batch_vp_fastslam_mh_cycle_async": poses + (p(z), p(nz), null, C.c_int(0), p(u01)),
            "batch_vp_serve_fastslam": (C.c_int(1),),
            "batch_fastslam_serve_sensor": (C.c_int(1),),
            "batch_vp_serve_estimates": (C.c_int(1),),
            "batch_resample_async": (p(nz), C.c_ulonglong(1))}[call]
    fn = f._fn(call)
    fn.restype = C.c_int
    rc = fn(f._h, *args)
    le = f._fn("last_error")
    le.restype = C.c_char_p
    return rc, (le(f._h) or b"").decode()


def _state(f):
    live = f.live_counts() if hasattr(f, "live_counts") else np.array([f.n])
    return f.get_weights().copy(), np.array(live).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS)
def test_every_call_on_every_kind_of_handle(pkg, sc, row):
    code = {I: pkg.capi.ERR_INVALID, U: pkg.capi.ERR_UNSUPPORTED}
    f, scens = _make(pkg, sc, row)
    w0, n0 = _state(f)
    for call, cell in zip(CALLS, TABLE[row]):
        if cell == OK:
            continue
        rc, msg = _invoke(pkg, f, call, scens)
        print("%s | %s -> %d %s" % (row, call, rc, msg))
        assert rc == code[cell[0]], (row, call, rc, msg)
        assert msg.startswith(cell[1]) and cell[2] in msg, (row, call, msg)
        w, n = _state(f)
        assert np.array_equal(w, w0) and np.array_equal(n, n0), (row, call)
    f.close()
    for call, cell in zip(CALLS, TABLE[row]):
        if cell != OK:
            continue
        f, scens = _make(pkg, sc, row)
        rc, msg = _invoke(pkg, f, call, scens)
        print("%s | %s -> %d %s" % (row, call, rc, msg if rc else ""))
        assert rc == pkg.capi.OK, (row, call, rc, msg)
        f.synchronize()
        f.close()
