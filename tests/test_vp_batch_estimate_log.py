"""The device-side estimate log on a BATCH of Victoria Park filters (include/rfsgpu.h [estimate], rfsgpu_batch_vp_serve_estimates;
csrc/estimate_log.h, the EstimateBatch<3> instantiation), on both routes of such a batch.

Yardstick: one Victoria Park handle per filter, served by rfsgpu_handle_serve_estimates and holding the same state.  The batch form is
the handle form's code in the same order with b = blockIdx.x, so every comparison is of 64-bit patterns; the only tolerance is the
1e-12 relative that tests/test_vp_filter_batch.py already allows the weights of the host-stop route.

The sentinel of the raw reads: rfsgpu_estimate_log_read copies whole rows, so inside a row that exists the entries at or beyond
n_logged / n_particles come back as whatever the device allocation held -- they are not compared.  The sentinel is asserted where the
read writes nothing: in the rows of the buffers beyond the rows the log has, and in a part buffer given to a log without particles."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from tests.support import estimate_reference as er
from tests.support import rbphd_device_cycle_reference as rb
from tests.support import vp_batch_loop_reference as ref
from test_vp_filter_batch import _filter_params, _sets

gpu = pytest.mark.gpu
CAP = 80
SENT = -7.25e300
INTS = ("status", "best_slot", "n_particles", "n_est", "n_logged")
GEOM = (0.76, 2.83, 3.78, 0.50)
VAR = np.array([4.0, 0.5])
TODAY = "the device-side map / pose error serves"          # the text of the batch's refusal of [estimate] and [metric]
NAME = "rfsgpu_batch_vp_serve_estimates"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _raises(pkg, status, fn, *needles):
    with pytest.raises(pkg.capi.EngineError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for n in needles:
        assert n in str(e.value), str(e.value)


def _vp_handle(pkg, n, cap=CAP):
    return pkg.RBPHDFilter(n, gm_capacity=cap, model=pkg.capi.MODEL_VICTORIAPARK_3D)


def _raw_read(pkg, f, n_f, max_est, slots, ask_rows, row_from=0, with_part=True):
    """rfsgpu_estimate_log_read into sentinel-filled buffers of ask_rows rows: (hdr, gauss, part, rows the log holds)."""
    hdr = np.zeros((ask_rows, n_f), dtype=pkg.capi.STEP_ESTIMATE_DTYPE)
    hdr.view(np.float64)[...] = SENT
    gauss = np.full((ask_rows, n_f, 6, max(max_est, 1)), SENT)
    part = np.full((ask_rows, n_f, 4, max(slots, 1)), SENT)
    n = C.c_int(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f._call("estimate_log_read", C.c_int(row_from), C.c_int(ask_rows), vp(hdr), vp(gauss) if max_est else C.c_void_p(None),
            vp(part) if with_part else C.c_void_p(None), C.byref(n))
    return hdr, gauss[..., :max_est] if max_est else gauss[..., :0], part, n.value


def _assert_rows_equal(hb, Gb, Pb, hh, Gh, Ph, b, n_per, what):
    """Filter b's row of a batch (hb, Gb [6, max_est], Pb [4, slots]) against the handle's (hh, Gh, Ph): every header field, every
    written plane entry and the first n_particles particle entries as 64-bit patterns; best_slot after the block offset."""
    for k in hb.dtype.names:
        vb, vh = hb[k], hh[k]
        if k == "best_slot":
            assert b * n_per <= int(vb) < (b + 1) * n_per, (what, "best_slot outside the filter's block", int(vb))
            vb = vb - b * n_per
        assert np.asarray(vb).tobytes() == np.asarray(vh).tobytes(), (what, k, vb, vh)
    k, n = int(hb["n_logged"]), int(hb["n_particles"])
    np.testing.assert_array_equal(_bits(Gb[:, :k]), _bits(Gh[:, :k]), err_msg=f"{what}: Gaussian planes")
    if Pb is not None:
        np.testing.assert_array_equal(_bits(Pb[:, :n]), _bits(Ph[:, :n]), err_msg=f"{what}: particle planes")


# ---- 1. switch and refusals -----------------------------------------------------------------------------------------------------

def test_switch_is_exported_with_the_headers_arguments(pkg):
    assert rb.declared_args(NAME) == "rfsgpu_filter *f, int on"
    assert "batch_vp_serve_estimates" in pkg.capi.ABI_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    core = txt[: txt.index("#ifdef __cplusplus")]
    assert NAME not in core.split("Everything else is OPTIONAL")[0]
    assert txt.index(NAME + "(rfsgpu_filter") > txt.index("rfsgpu_handle_serve_estimates(rfsgpu_filter") > txt.index("---- [estimate]")
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    assert hasattr(lib, NAME) and hasattr(pkg.capi.CVPBatch, "serve_estimates")
    fn = getattr(lib, NAME)
    fn.restype = C.c_int
    for on in (0, 1):
        assert fn(C.c_void_p(), C.c_int(on)) == pkg.capi.ERR_INVALID      # a null handle


def _plant(rng, f, n, cap, lo=0, sizes=None):
    """Weights, poses and a small mixture per slot [lo, lo + n) through the setters of f's own slots; returns (w, x, mixtures)."""
    w = rng.uniform(0.05, 1.0, n)
    x = np.column_stack([rng.normal(0, 30, n), rng.normal(0, 30, n), rng.uniform(-np.pi, np.pi, n)])
    gms = [_mixture(rng, (1 + i % 3) if sizes is None else sizes[i]) for i in range(n)]
    return w, x, gms


def _mixture(rng, m):
    """m Victoria Park Gaussians, weights on both sides of 0.5."""
    w = rng.uniform(0.05, 1.4, m)
    mean = np.column_stack([rng.uniform(-80, 80, (m, 2)), rng.uniform(0.3, 1.5, m)]) if m else np.zeros((0, 3))
    A = rng.normal(0, 0.2, (m, 3, 3))
    cov = A @ np.swapaxes(A, -1, -2) + np.eye(3) * 0.05 if m else np.zeros((0, 3, 3))
    return w, mean, cov


def _log_calls(f):
    return (lambda: f.estimate_log_create(2, 4), lambda: f.estimate_log_reset(), lambda: f.step_estimate_async(0.0), lambda: f.estimate_log_read())


def _snapshot(f):
    f.synchronize()
    return dict(w=f.get_weights().copy(), x=f.get_poses().copy(), sizes=np.asarray(f.gm_sizes()).copy(), gm=[f.export_gm(i) for i in range(f.n)])


def _assert_snapshot(a, b, what):
    for k in ("w", "x"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(a["sizes"], b["sizes"], err_msg=what)
    for i, (p, q) in enumerate(zip(a["gm"], b["gm"])):
        for u, v in zip(p, q):
            np.testing.assert_array_equal(u, v, err_msg=f"{what}: mixture of slot {i}")


@gpu
def test_switch_and_refusals(pkg):
    capi = pkg.capi
    U, rng = capi.ERR_UNSUPPORTED, np.random.default_rng(5)
    nF, n = 3, 5
    batch = pkg.VPFilterBatch(nF, n, gm_capacity=64)          # (a multiple of 64: the capacity the handle keeps)
    w, x, gms = _plant(rng, batch, nF * n, 64)
    batch.set_weights(w)
    batch.set_poses(x, None)
    for i, gm in enumerate(gms):
        batch.import_gm(i, *gm)
    before = _snapshot(batch)
    for call in _log_calls(batch):                                           # off at creation: today's code and text
        _raises(pkg, U, call, "the Victoria Park model", TODAY)
    batch.serve_estimates(True)
    _raises(pkg, capi.ERR_CAPACITY, lambda: batch.step_estimate_async(0.0), "no estimate log")
    _raises(pkg, capi.ERR_INVALID, lambda: batch.estimate_log_create(2, 65), "max_est")
    batch.estimate_log_create(2, 64)                                         # max_est 0 ... gm_capacity
    batch.estimate_log_create(2, 0)
    batch.estimate_log_create(3, 16, True)
    assert batch.n_estimate_slots == n
    batch.step_estimate_async(0.5, -np.inf)
    batch.step_estimate_async([1.5, 2.5, 3.5], -np.inf)
    hdr, gauss, part = batch.estimate_log_read()
    assert hdr.shape == (2, nF) and gauss.shape == (2, nF, 6, 16) and part.shape == (2, nF, 4, n)
    assert list(hdr["t"][0]) == [0.5] * 3 and list(hdr["t"][1]) == [1.5, 2.5, 3.5]
    assert (hdr["n_particles"] == n).all() and (hdr["status"] == 0).all()
    for b in range(nF):
        best = b * n + int(np.argmax(w[b * n:(b + 1) * n]))
        assert (hdr["best_slot"][:, b] == best).all() and (hdr["n_est"][:, b] == len(gms[best][0])).all()
    # what the switch does not open
    _raises(pkg, U, lambda: batch.run_log_estimates(True), "batch_run_log_estimates", TODAY)
    _raises(pkg, U, lambda: batch.step_error_async(0.0), "step_error_async", TODAY)
    _raises(pkg, U, lambda: batch.error_log_create(2), TODAY)
    _raises(pkg, U, lambda: batch.handle_serve_estimates(True), "handle_serve_estimates", "batch")
    batch.serve_estimates(False)                                             # the refusals are back, the log is gone
    for call in _log_calls(batch):
        _raises(pkg, U, call, "the Victoria Park model", TODAY)
    batch.serve_estimates(True)
    _raises(pkg, capi.ERR_CAPACITY, lambda: batch.step_estimate_async(0.0), "no estimate log")
    batch.serve_estimates(False)
    _assert_snapshot(before, _snapshot(batch), "the Victoria Park batch")
    batch.close()
    # everything else: UNSUPPORTED, naming the call that serves it, the state untouched and nothing switched on
    g = pkg.FilterGroup(16, [0, 0], gm_capacity=16)
    plain = _vp_handle(pkg, 4, 16)
    others = [(pkg.FilterBatch(2, 4, gm_capacity=16), "rfsgpu_estimate_log_create"), (pkg.FastSLAMBatch(2, 4, gm_capacity=16), "rfsgpu_estimate_log_create"),
              (pkg.MHFastSLAMBatch(2, 4, 8, gm_capacity=16), "rfsgpu_batch_mh_serve_metrics"), (plain, "rfsgpu_handle_serve_estimates"),
              (g.shards[0], "rfsgpu_group")]
    for h, word in others:
        kept = (h.get_weights().copy(), h.get_poses().copy(), np.asarray(h.gm_sizes()).copy())
        for on in (1, 0):
            _raises(pkg, U, lambda: h._call("batch_vp_serve_estimates", C.c_int(on)), "batch_vp_serve_estimates", word)
        for a, b in zip(kept, (h.get_weights(), h.get_poses(), h.gm_sizes())):
            np.testing.assert_array_equal(a, b)
    _raises(pkg, U, lambda: plain.estimate_log_create(2, 4), "the Victoria Park model")      # (the refused switch switched nothing)
    _raises(pkg, U, lambda: others[2][0].estimate_log_create(2, 4), "rfsgpu_batch_mh_serve_metrics")
    for h, _ in others[:4]:
        h.close()
    g.close()


# ---- 2. planted rows against a handle per filter, bit for bit ----------------------------------------------------------------------

SIZES = (0, 1, 64, 65)                                    # the would-be best particle's mixture: the ballot round's boundary
LOGS = ((40, -np.inf), (CAP, 0.5))                        # (max_est, w_threshold): below the largest size (status 1, cut planes) | capacity


def _pattern(kind, base, n):
    """(weights [n], the slot that must win): 0 a unique maximum in the last slot; 1 the same maximum in two slots; 2 all zero."""
    w = base.copy()
    if kind == 0 or n == 1 and kind == 1:
        w[n - 1] = 2.0
        return w, n - 1
    if kind == 1:
        lo = (n - 1) // 2
        w[[lo, n - 1]] = 2.0
        return w, lo
    return np.zeros(n), 0


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nF", [1, 3])
def test_planted_rows_equal_a_served_handle_per_filter(pkg, nF, n):
    """Four rounds; in round r filter b carries weight pattern (b + r) % 3 and its would-be best particle SIZES[(b + r) % 4] Gaussians,
    so every filter meets every pattern and every size; per round one row under each of LOGS, with the particle planes."""
    rng = np.random.default_rng(1000 * nF + n)
    batch = pkg.VPFilterBatch(nF, n, gm_capacity=CAP)
    handles = [_vp_handle(pkg, n) for _ in range(nF)]
    batch.serve_estimates(True)
    for h in handles:
        h.handle_serve_estimates(True)
    base, x, gms = _plant(rng, batch, nF * n, CAP)
    batch.set_poses(x, None)
    for i, gm in enumerate(gms):
        batch.import_gm(i, *gm)
        handles[i // n].import_gm(i % n, *gm)
    for b, h in enumerate(handles):
        h.set_poses(x[b * n:(b + 1) * n], None)
    seen = dict(status1=0, sizes=set(), kinds=set())
    for r in range(4):
        w, want, size = np.empty(nF * n), [], []
        for b in range(nF):
            kind = (b + r) % 3
            w[b * n:(b + 1) * n], s = _pattern(kind, base[b * n:(b + 1) * n], n)
            gm = _mixture(rng, SIZES[(b + r) % 4])
            batch.import_gm(b * n + s, *gm)
            handles[b].import_gm(s, *gm)
            handles[b].set_weights(w[b * n:(b + 1) * n])
            want.append(s)
            size.append(len(gm[0]))
            seen["sizes"].add(len(gm[0]))
            seen["kinds"].add(kind if n > 1 or kind != 1 else 0)
        batch.set_weights(w)
        t = 10.0 * r + np.arange(nF) + 0.125
        for max_est, thr in LOGS:
            batch.estimate_log_create(1, max_est, True)
            batch.step_estimate_async(t, thr)
            hb, Gb, Pb, rows = _raw_read(pkg, batch, nF, max_est, n, 2)
            assert rows == 1
            for buf in (hb.view(np.float64)[1], Gb[1], Pb[1]):                 # the row the log does not have: not written
                assert (buf == SENT).all()
            for b, h in enumerate(handles):
                what = f"round {r} filter {b} max_est {max_est} thr {thr}"
                h.estimate_log_create(1, max_est, True)
                h.step_estimate_async(t[b], thr)
                hh, Gh, Ph, rows = _raw_read(pkg, h, 1, max_est, n, 1)
                assert rows == 1
                _assert_rows_equal(hb[0, b], Gb[0, b], Pb[0, b], hh[0, 0], Gh[0, 0], Ph[0, 0], b, n, what)
                assert int(hb[0, b]["best_slot"]) == b * n + want[b] and int(hb[0, b]["n_particles"]) == n and hb[0, b]["t"] == t[b], what
                if thr == -np.inf:
                    assert int(hb[0, b]["n_est"]) == size[b], what
                assert int(hb[0, b]["status"]) == int(int(hb[0, b]["n_est"]) > max_est), what
                seen["status1"] += int(hb[0, b]["status"])
        # a log without particle planes: the headers are the same, the part buffer is not touched
        batch.estimate_log_create(1, CAP, False)
        batch.step_estimate_async(t, 0.5)
        h2, _, P2, _ = _raw_read(pkg, batch, nF, CAP, n, 1)
        assert h2.tobytes() == hb[:1].tobytes() and (P2 == SENT).all()
    assert seen["status1"] > 0 and seen["sizes"] == set(SIZES) and seen["kinds"] == ({0, 2} if n == 1 else {0, 1, 2}), seen
    batch.close()
    for h in handles:
        h.close()


# ---- 3. rows behind the device route -----------------------------------------------------------------------------------------------

def _gm2(f, s):
    w, _, mean, cov = f.export_gm(s)
    return w, mean[:, :2], cov[:, :2, :2]


@gpu
@pytest.mark.parametrize("n", [3, 65])
def test_rows_behind_the_device_route(pkg, n):
    """Four lidar updates through the calls of the device route with a row behind each resampling step; nothing of the logged batch
    is read until the end.  An unlogged twin on the same route is read after every update: the row's integers by the restated
    selection rule, its copies bit for bit, and the whole header against a served handle loaded with the twin's state."""
    sc = pkg.scenarios
    nF, keys, cap = 3, [11, 0xABCDEF0123456789, 77], ref.CAP
    gates = [(1, 1), (3, 1), (1, 1)]
    eff = [(2.0 * n, 2.0), (2.0 * n, 2.0), (0.0, 0.0)]          # filter 0 fires whenever its gates are open, filter 2 never

    def params_of(b):
        P = _filter_params(sc, b)
        P["min_updates"], P["min_measurements"] = gates[b]
        return P
    scens, (dev, twin) = ref.make_batches(pkg, nF, n, params_of)
    for f in (dev, twin):
        for b in range(nF):
            f.set_motion(b, VAR, GEOM, keys[b])
            f.set_resampling(b, *eff[b])
    handles = [_vp_handle(pkg, n, cap) for _ in range(nF)]
    for h in handles:
        h.handle_serve_estimates(True)
        h.estimate_log_create(4, cap, True)
    dev.serve_estimates(True)
    dev.estimate_log_create(4, cap, True)
    sets = _sets(scens, 4, seed=5, nz_max_at=(9, 9))
    u = np.array([[1.5, 0.02], [2.0, -0.05], [2.5, 0.11]])
    dt = np.array([0.025, 0.03, 0.025])
    thr, expect = 0.5, []
    for c in range(4):
        n_z = np.array([len(z) for z in sets[c]])
        k = 2 + c % 2
        q = np.diag([5e-4, 5e-4, 1e-4])[None] * (dt[:k] ** 2)[:, None, None]
        for f in (dev, twin):
            f.set_lmk_process_noise(q[0])
            f.cycle_async(True, [np.zeros((0, 3))] * nF, normalize=False)      # the birth cycle
            f.static_steps_async(k - 1, q[1:])
            f.propagate_run_async(u[:k], dt[:k], 10 * c)
            f.cycle_async(None, sets[c], poses=None, normalize=True)           # x = NULL: at the propagated poses
            f.resample_async(n_z, c)
        t = 100.0 + c + 0.25 * np.arange(nF)
        dev.step_estimate_async(t, thr)
        # the twin, read where the row stands in the logged batch's stream
        w, x = twin.get_weights(), twin.get_poses()
        rows = []
        for b, h in enumerate(handles):
            blk = slice(b * n, (b + 1) * n)
            fields, planes = er.reference_row(w[blk], x[blk], lambda s: _gm2(twin, s), thr, cap, lo=b * n)
            best = fields["best_slot"] - b * n
            gw, _, mean, cov = twin.export_gm(fields["best_slot"])
            h.set_weights(w[blk])
            h.set_poses(x[blk], None)
            h.import_gm(best, gw, mean, cov)
            h.step_estimate_async(t[b], thr)
            rows.append((fields, planes, w[blk].copy(), x[blk].copy()))
        expect.append(rows)
    counts, _ = dev.loop_counts()
    assert (counts > 0).any() and (counts == 0).any(), ("both a filter that fired and one that never did are needed", counts)
    np.testing.assert_array_equal(counts, twin.loop_counts()[0])
    hdr, G, P, n_rows = _raw_read(pkg, dev, nF, cap, n, 5)
    assert n_rows == 4 and (hdr.view(np.float64)[4] == SENT).all() and (G[4] == SENT).all() and (P[4] == SENT).all()
    for b, h in enumerate(handles):
        hh, Gh, Ph, n_h = _raw_read(pkg, h, 1, cap, n, 4)
        assert n_h == 4
        for c in range(4):
            what = f"update {c} filter {b}"
            fields, planes, wb, xb = expect[c][b]
            row = hdr[c, b]
            for k in INTS:
                assert int(row[k]) == fields[k], (what, k, int(row[k]), fields[k])
            best = fields["best_slot"] - b * n
            for name, v in (("best_x", xb[best, 0]), ("best_y", xb[best, 1]), ("best_theta", xb[best, 2]), ("best_weight", wb[best])):
                assert row[name].tobytes() == np.float64(v).tobytes(), (what, name)
            kk = fields["n_logged"]
            np.testing.assert_array_equal(_bits(G[c, b][:, :kk]), _bits(planes[:, :kk]), err_msg=f"{what}: Gaussians")
            for p, v in enumerate((xb[:, 0], xb[:, 1], xb[:, 2], wb)):
                np.testing.assert_array_equal(_bits(P[c, b, p, :n]), _bits(v), err_msg=f"{what}: particle plane {p}")
            _assert_rows_equal(row, G[c, b], P[c, b], hh[c, 0], Gh[c, 0], Ph[c, 0], b, n, what)      # the sums: the handle's tree
    ref.assert_same_state(ref.state(dev), ref.state(twin), "the logged batch against the unlogged twin")
    dev.close(); twin.close()
    for h in handles:
        h.close()


# ---- 4. a full log ----------------------------------------------------------------------------------------------------------------

@gpu
def test_full_log_enqueues_nothing(pkg):
    capi, rng = pkg.capi, np.random.default_rng(9)
    nF, n = 3, 5
    batch = pkg.VPFilterBatch(nF, n, gm_capacity=16)
    w, x, gms = _plant(rng, batch, nF * n, 16)
    batch.set_poses(x, None)
    for i, gm in enumerate(gms):
        batch.import_gm(i, *gm)
    batch.serve_estimates(True)
    batch.estimate_log_create(2, 16, True)
    batch.set_weights(w)
    batch.step_estimate_async(1.0, -np.inf)
    batch.step_estimate_async(2.0, -np.inf)
    first = _raw_read(pkg, batch, nF, 16, n, 2)
    w2 = w[::-1].copy()
    batch.set_weights(w2)                                                   # a third row would differ from both
    _raises(pkg, capi.ERR_CAPACITY, lambda: batch.step_estimate_async(3.0, -np.inf), "the estimate log is full")
    batch.synchronize()
    again = _raw_read(pkg, batch, nF, 16, n, 2)
    assert again[3] == first[3] == 2
    for a, b in zip(first[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    lo, hi = _raw_read(pkg, batch, nF, 16, n, 1, row_from=0), _raw_read(pkg, batch, nF, 16, n, 1, row_from=1)      # two chunks
    for k in range(3):
        assert lo[k].tobytes() + hi[k].tobytes() == first[k].tobytes()
    batch.estimate_log_reset()
    assert _raw_read(pkg, batch, nF, 16, n, 1)[3] == 0
    batch.step_estimate_async(3.0, -np.inf)
    hdr, _, part, rows = _raw_read(pkg, batch, nF, 16, n, 2)
    assert rows == 1 and (hdr["t"][0] == 3.0).all() and (hdr.view(np.float64)[1] == SENT).all()
    for b in range(nF):
        assert int(hdr["best_slot"][0, b]) == b * n + int(np.argmax(w2[b * n:(b + 1) * n]))
        np.testing.assert_array_equal(_bits(part[0, b, 3, :n]), _bits(w2[b * n:(b + 1) * n]))
    batch.close()


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------

def _driver_setup(pkg, nF, n, cap):
    sc = pkg.scenarios
    seeds, clutter = [31, 38, 45], [3.0, 1.0, 5.0]
    eff_n = [n + 1.0, n / 2.0, n + 1.0]                     # filters 0 and 2 resample whenever their gates are open
    Ps = []
    for b in range(nF):
        P = dict(sc.VP_PARAMS)
        P["expected_clutter"] = [6.0, 3.0, 9.0][b]
        P["birth_count_thr"], P["birth_check_thr"] = [(5, 10), (2, 4), (3, 6)][b]
        P["min_updates"], P["min_measurements"] = [(2, 15), (3, 15), (2, 30)][b]
        Ps.append(P)
    batch = pkg.VPFilterBatch(nF, n, gm_capacity=cap)
    handles = [_vp_handle(pkg, n, cap) for _ in range(nF)]
    for b in range(nF):
        sc.apply_vp_batch_params(batch, b, Ps[b])
        sc.apply_vp_params(handles[b], Ps[b], np.full(361, 70.0))
    return batch, handles, Ps, seeds, clutter, eff_n


def _run_both(pkg, device_loop):
    drv = pkg.vp_driver
    data = np.load(os.path.join(ROOT, "tests", "golden", "victoria_park_extract.npz"))
    nF, n, cap = 3, 33, 384
    batch, handles, Ps, seeds, clutter, eff_n = _driver_setup(pkg, nF, n, cap)
    kw = dict(added_clutter=clutter, eff_n=eff_n, device_loop=device_loop, log_estimates=True)
    rb_ = drv.VictoriaParkBatchRun(batch, data, Ps, seeds, **kw).run(200)
    rh = drv.VictoriaParkBatchRun(handles, data, Ps, seeds, **kw).run(200)
    return rb_, rh, batch, handles, nF, n, cap


@gpu
def test_driver_device_loop_log_equals_the_handles(pkg, tmp_path):
    drv = pkg.vp_driver
    rb_, rh, batch, handles, nF, n, cap = _run_both(pkg, True)
    eb, eh = rb_.estimates(), rh.estimates()
    assert rb_.n_lidar == rh.n_lidar == 20
    assert eb[0].shape == eh[0].shape == (21, nF) and eb[1].shape == eh[1].shape == (21, nF, 6, cap) and eb[2].shape == eh[2].shape == (21, nF, 4, n)
    assert rb_.n_resamples.sum() > 0 and (eb[0]["n_est"][-1] > 0).any()
    for r in range(21):
        for b in range(nF):
            _assert_rows_equal(eb[0][r, b], eb[1][r, b], eb[2][r, b], eh[0][r, b], eh[1][r, b], eh[2][r, b], b, n, f"row {r} filter {b}")
    assert (eb[0]["t"][0] == float(rb_.mgr[0][0])).all()
    pairs = drv.write_vp_batch_logs(str(tmp_path / "batch"), eb)
    assert [os.path.basename(os.path.dirname(p[0])) for p in pairs] == ["filter_%03d" % b for b in range(nF)]
    for b, h in enumerate(handles):
        ph = drv.write_vp_logs(str(tmp_path / ("handle%d" % b)), h.estimate_log_read())
        for got, want in zip(pairs[b], ph):
            data = open(got, "rb").read()
            assert data == open(want, "rb").read() and len(data) > 0, (b, got)
    batch.close()
    for h in handles:
        h.close()


@gpu
def test_driver_host_stop_log_equals_the_handles(pkg):
    """The host-stop route: integers and best_slot exact, the poses exact (both runs push the same host arrays), weights and
    Gaussian values at the 1e-12 relative that tests/test_vp_filter_batch.py holds that route to.  The weighted means sum w q / sum w:
    weights that differ by at most 1e-12 relative move a mean by at most 2e-12 max|q|, the two summations add n eps max|q| each
    (n = 33: 1.5e-14 max|q|) -- held to 4e-12 max(1, max|q|) absolute, since a mean may cancel to near zero."""
    rb_, rh, batch, handles, nF, n, cap = _run_both(pkg, False)
    (hb, Gb, Pb), (hh, Gh, Ph) = rb_.estimates(), rh.estimates()
    assert hb.shape == hh.shape == (21, nF) and rb_.n_resamples.sum() > 0
    np.testing.assert_array_equal(rb_.n_resamples, rh.n_resamples)
    for k in INTS:
        np.testing.assert_array_equal(hb[k] - (np.arange(nF) * n if k == "best_slot" else 0), hh[k], err_msg=k)
    np.testing.assert_array_equal(hb["t"], hh["t"])
    for k in ("cardinality", "best_weight", "weight_sum"):
        np.testing.assert_allclose(hb[k], hh[k], rtol=1e-12, atol=0, err_msg=k)
    for k in ("best_x", "best_y", "best_theta"):
        np.testing.assert_array_equal(_bits(hb[k]), _bits(hh[k]), err_msg=k)
    for k, q in (("mean_x", Ph[:, :, 0]), ("mean_y", Ph[:, :, 1]), ("mean_cos", None), ("mean_sin", None)):
        bound = 4e-12 * (1.0 if q is None else np.maximum(1.0, np.abs(q).max(axis=-1)))
        assert (np.abs(hb[k] - hh[k]) <= bound).all(), (k, np.abs(hb[k] - hh[k]).max())
    np.testing.assert_allclose(Gb, Gh, rtol=1e-12, atol=0)                   # (beyond n_logged both reads hold zeros)
    np.testing.assert_array_equal(_bits(Pb[:, :, :3]), _bits(Ph[:, :, :3]))
    np.testing.assert_allclose(Pb[:, :, 3], Ph[:, :, 3], rtol=1e-12, atol=0)
    batch.close()
    for h in handles:
        h.close()


# ---- 6. write_vp_logs ---------------------------------------------------------------------------------------------------------------

def test_write_vp_logs_filter_argument(pkg, tmp_path):
    """A hand-made log of two filters: filter 1's lines with best_slot relative to its block; filter 0 of a one-filter log prints what
    the function printed before it had the argument -- the docstring's format strings over hdr[r, 0]."""
    drv = pkg.vp_driver
    (hdr, gauss, part), _ = er.synthetic_trace(pkg.capi.STEP_ESTIMATE_DTYPE, n_filters=2)
    n = part.shape[-1]
    assert (hdr["best_slot"][:, 1] >= n).all() and (hdr["best_slot"][:, 0] < n).all()

    def today(b, rel):
        poses, lms = "", ""
        for r in range(hdr.shape[0]):
            h = hdr[r, b]
            for i in range(int(h["n_particles"])):
                poses += "%10.3f%5d%10.3f%10.3f%10.3f%10.3f\n" % ((float(h["t"]), i) + tuple(part[r, b, :, i]))
            for m in range(int(h["n_logged"])):
                lms += "%10.3f%5d%10.3f%10.3f%10.3f%10.3f%10.3f%10.3f\n" % ((float(h["t"]), int(h["best_slot"]) - rel) + tuple(gauss[r, b, :, m]))
        return poses, lms
    p1 = drv.write_vp_logs(str(tmp_path / "f1"), (hdr, gauss, part), filter=1)
    assert (open(p1[0]).read(), open(p1[1]).read()) == today(1, n)
    p0 = drv.write_vp_logs(str(tmp_path / "f0"), (hdr[:, :1], gauss[:, :1], part[:, :1]))
    assert (open(p0[0]).read(), open(p0[1]).read()) == today(0, 0) and len(open(p0[1]).read()) > 0
    assert open(p1[1]).read() != open(p0[1]).read()
    pairs = drv.write_vp_batch_logs(str(tmp_path / "all"), (hdr, gauss, part))
    assert [os.path.relpath(p[0], str(tmp_path / "all")) for p in pairs] == ["filter_000/particlePose.dat", "filter_001/particlePose.dat"]
    assert open(pairs[1][1]).read() == open(p1[1]).read() and open(pairs[0][0]).read() == open(p0[0]).read()
