"""The device loop of a filter batch (include/rfsgpu.h [batch]; csrc/batch_loop.h): rfsgpu_batch_propagate_async and
rfsgpu_batch_resample_async against a numpy restatement of their Philox draws (tests/support/device_loop_reference.py) and against
the host route (FilterBatch.update_and_resample + rfsgpu_batch_resample_apply) driven with the restated draws."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests.support import device_loop_reference as dl

LOOP_SYMBOLS = ["rfsgpu_batch_set_motion_odometry", "rfsgpu_batch_set_resampling", "rfsgpu_batch_propagate_async", "rfsgpu_batch_resample_async",
                "rfsgpu_batch_last_resample", "rfsgpu_batch_resample_counts", "rfsgpu_batch_get_pose_covs"]
LIMIT = 2048      # RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_device_loop_in_the_batch_section_and_the_library_exports_it(pkg):
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    head = txt[: txt.index("#ifdef __cplusplus")]
    core = re.search(r"STABLE CORE.*?\*/", head, flags=re.S).group(0)
    sec, nxt = txt.index("[batch]"), txt.index("[metric] per-step")
    for s in LOOP_SYMBOLS:
        assert s not in core, s
        assert sec < txt.index(s + "(") < nxt, s
    assert re.search(r"#define RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER\s+%d\b" % LIMIT, txt)
    pkg.build_mod.build()
    lib = C.CDLL(pkg.build_mod.LIB)
    for s in LOOP_SYMBOLS:
        assert hasattr(lib, s), s


def test_philox_restatement_meets_the_known_answers():
    """Random123's kat_vectors for philox4x32, 10 rounds (the ones tests/test_motion.py quotes)."""
    M = dl.MASK
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((M, M, M, M), (M, M), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = dl.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
        assert tuple(int(g[0]) for g in got) == want
    # the three uses are blocks (i, 0), (i, 1) and (0, 2) of (call lo, call hi) under (seed lo, seed hi)
    seed, call = 0x299f31d0a4093822, 0x0370734413198a2e
    r = dl._block(3, 0, seed, call)
    want = dl.philox4x32_10([np.array([2], dtype=np.uint64), np.array([0], dtype=np.uint64), np.array([0x13198a2e], dtype=np.uint64),
                             np.array([0x03707344], dtype=np.uint64)], (0xa4093822, 0x299f31d0))
    assert [int(x[2]) for x in r] == [int(x[0]) for x in want]
    g = dl.propagation_deviates(20000, 12345, 9)
    assert np.isfinite(g).all() and np.abs(g.mean(axis=0)).max() < 0.03 and np.abs(g.var(axis=0) - 1).max() < 0.04


def test_restated_resampling_draw_is_never_one():
    top = (1 << 53) - 1
    assert top * (1.0 / 9007199254740992.0) < 1.0            # the largest 53-bit value still lies below 1
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, call = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
        bits = dl.resample_draw_bits(seed, call)
        assert 0 <= bits <= top
        assert 0.0 <= dl.resample_draw(seed, call) < 1.0
    assert dl.u01_open_low(np.uint64(0), np.uint64(0)) > 0.0   # and the Box-Muller uniform is never 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _empty(nF):
    return [np.zeros((0, 2))] * nF


@pytest.mark.gpu
def test_propagation_matches_the_restatement(pkg):
    nF, nP = 6, 300
    rng = np.random.default_rng(17)
    x0 = np.column_stack([rng.uniform(-50, 50, nF * nP), rng.uniform(-50, 50, nF * nP), rng.uniform(-np.pi, np.pi, nF * nP)])
    var = np.array([[2e-3, 1e-3, 5e-4], [0.2, 0.1, 0.05], [0, 0, 0], [1e-6, 3e-2, 2e-3], [1e-3, 0, 2e-3], [0, 0, 0]])
    seeds = [1, 0x1234567890ABCDEF, 77, 2 ** 64 - 1, 5, 6]
    u = rng.uniform(-0.3, 0.3, (nF, 3))
    batch = pkg.FilterBatch(nF, nP, gm_capacity=64)
    batch.set_poses(x0)
    for b in range(nF):
        batch.set_motion_odometry(b, var[b], seeds[b])
    want = x0.copy()
    for call in (0, 1, 7, 1 << 33):
        pin = np.array([0, 1 if call == 1 else 0, 0, 0, 1 if call == 7 else 0, 0], dtype=np.uint8)
        pin_pose = rng.uniform(-3, 3, (nF, 3))
        batch.propagate_async(u, call, pin=pin if pin.any() else None, pin_pose=pin_pose if pin.any() else None)
        for b in range(nF):
            blk = batch.block(b)
            want[blk] = np.tile(pin_pose[b], (nP, 1)) if pin[b] else dl.propagate(want[blk], u[b], var[b], seeds[b], call)
        got = batch.get_poses()
        covs = batch.get_pose_covs()
        for b in range(nF):
            blk = batch.block(b)
            np.testing.assert_array_equal(covs[blk], np.tile(np.diag(var[b] * (0 if pin[b] else 1)), (nP, 1, 1)), err_msg=f"call {call} filter {b}: covariances")
            if pin[b]:
                np.testing.assert_array_equal(got[blk], want[blk], err_msg=f"call {call} filter {b}: pinned poses")
            elif not var[b].any():
                np.testing.assert_allclose(got[blk], want[blk], rtol=1e-13, atol=1e-13, err_msg=f"call {call} filter {b}: noise-free")
            else:
                np.testing.assert_allclose(got[blk], want[blk], rtol=1e-10, atol=1e-10, err_msg=f"call {call} filter {b}")
        batch.cycle_async(True, _empty(nF), normalize=True)      # an empty cycle: nothing else moves
        np.testing.assert_array_equal(batch.get_poses(), got)
    assert np.abs(batch.get_poses()[batch.block(1)] - batch.get_poses()[batch.block(2)]).max() > 0.1
    # a filter's result does not depend on its place in the batch: the filter at block 0 of this batch as block 3 of another, the one at
    # block 1 as block 4
    other = pkg.FilterBatch(5, nP, gm_capacity=64)
    x1 = rng.uniform(-1, 1, (5 * nP, 3))
    x1[3 * nP:4 * nP] = x0[batch.block(0)]
    x1[4 * nP:] = x0[batch.block(1)]
    other.set_poses(x1)
    other.set_motion_odometry(None, [9.0, 9.0, 9.0], 4242)
    other.set_motion_odometry(3, var[0], seeds[0])
    other.set_motion_odometry(4, var[1], seeds[1])
    uo = rng.uniform(-0.3, 0.3, (5, 3))
    uo[3], uo[4] = u[0], u[1]
    first = pkg.FilterBatch(nF, nP, gm_capacity=64)
    first.set_poses(x0)
    for b in range(nF):
        first.set_motion_odometry(b, var[b], seeds[b])
    first.propagate_async(u, 1 << 33)
    other.propagate_async(uo, 1 << 33)
    np.testing.assert_array_equal(_bits(first.get_poses()[first.block(0)]), _bits(other.get_poses()[other.block(3)]))
    np.testing.assert_array_equal(_bits(first.get_poses()[first.block(1)]), _bits(other.get_poses()[other.block(4)]))
    assert np.abs(first.get_poses()[first.block(0)] - x0[first.block(0)]).max() > 1e-3


def _scenario_batches(pkg, sc, nF, nP, count):
    scens = [sc.make_scenario(nP, 40, 10, seed=901 + b) for b in range(nF)]
    from test_filter_batch import _configure_from_scenario
    out = []
    for _ in range(count):
        batch = pkg.FilterBatch(nF, nP, gm_capacity=128)
        batch.set_poses(np.vstack([s["poses"] for s in scens]), np.vstack([np.tile(np.asarray(s["pose_cov"], dtype=np.float64).ravel(), (nP, 1)) for s in scens]))
        batch.set_weights(np.concatenate([s["particle_w"] for s in scens]))
        for b, s in enumerate(scens):
            _configure_from_scenario(pkg.capi, batch, b, s["params"])
            for i in range(nP):
                batch.import_gm(b * nP + i, s["w"][i], s["mean"][i], s["cov"][i])
        out.append(batch)
    return scens, out


def _assert_same_state(a, b, mixtures=True, what=""):
    """mixtures: True = every slot's; "nonempty" = those of the slots that hold a Gaussian on either side."""
    sa, sb = a.gm_sizes(), b.gm_sizes()
    np.testing.assert_array_equal(sa, sb, err_msg=what + ": sizes")
    np.testing.assert_array_equal(_bits(a.get_weights()), _bits(b.get_weights()), err_msg=what + ": weights")
    np.testing.assert_array_equal(a.get_unused_masks(), b.get_unused_masks(), err_msg=what + ": unused masks")
    if mixtures:
        for i in (np.nonzero((sa > 0) | (sb > 0))[0] if mixtures == "nonempty" else range(a.n)):
            i = int(i)
            for x, y in zip(a.export_gm(i), b.export_gm(i)):
                np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{what}: mixture of slot {i}")


@pytest.mark.gpu
def test_births_after_a_propagation_see_the_old_poses(pkg, sc):
    """Twin batches: one propagates on the device and cycles with poses=None; the other is handed the propagated poses and
    covariances (both read back) through cycle_async."""
    nF, nP = 3, 24
    scens, (a, b) = _scenario_batches(pkg, sc, nF, nP, 2)
    var = np.array([[2e-3, 1e-3, 5e-4], [4e-3, 2e-3, 1e-3], [1e-3, 1e-3, 1e-3]])
    for q in range(nF):
        a.set_motion_odometry(q, var[q], 100 + q)
    Zs = [s["Z"] for s in scens]
    for bt in (a, b):
        bt.cycle_async(None, Zs, normalize=True)                 # an update first: unused measurements for the births
    _assert_same_state(a, b, what="before")
    u = np.array([[0.05, 0.01, 0.02], [0.03, -0.02, -0.04], [0.1, 0.0, 0.3]])
    pin = np.array([0, 0, 1], dtype=np.uint8)
    pin_pose = np.vstack([s["poses"][0] for s in scens]) + 0.01
    for call in (3, 4):
        assert a.get_unused_masks().any()                        # births are pending
        old = a.get_poses()
        a.propagate_async(u, call, pin=pin, pin_pose=pin_pose)
        new = a.get_poses()
        assert np.abs(new - old).max() > 1e-3
        cov = a.get_pose_covs().reshape(-1, 9)
        np.testing.assert_array_equal(cov, np.vstack([np.tile(np.diag(var[q] * (0 if pin[q] else 1)).ravel(), (nP, 1)) for q in range(nF)]))
        a.cycle_async(True, Zs, normalize=True)
        b.cycle_async(True, Zs, poses=new, pose_cov=cov, normalize=True)
        np.testing.assert_array_equal(_bits(a.get_poses()), _bits(new))
        _assert_same_state(a, b, what=f"call {call}")
    # poses set by hand after a propagation are the ones the next births happen at, as without the propagation
    a.propagate_async(u, 5, pin=pin, pin_pose=pin_pose)
    y = a.get_poses() + 0.02
    cov = np.tile(np.diag([1e-3, 2e-3, 3e-3]).ravel(), (nF * nP, 1))
    assert a.get_unused_masks().any()
    for bt in (a, b):
        bt.set_poses(y, cov)
        bt.cycle_async(True, Zs, normalize=True)
    _assert_same_state(a, b, what="set_poses after a propagation")


def _weights_case(name, n, rng):
    if name == "uniform":
        w = np.full(n, 1.0)
    elif name == "dominant":
        w = np.full(n, 1e-6)
        w[n // 3] = 1.0
    elif name == "zeros":
        w = rng.uniform(0, 1, n) ** 4
        w[rng.random(n) < 0.4] = 0.0
        w[0] = 0.0
        w[-1] = 0.0
        if n == 1:
            w[0] = 1.0
        elif not w.any():
            w[n // 2] = 1.0
    elif name == "runs":
        w = np.repeat(rng.uniform(0, 1, (n + 6) // 7) ** 8, 7)[:n]
    else:
        w = rng.uniform(0, 1, n) ** 6
    return w / w.sum()


def _sequential_neff(w):
    s = 0.0
    for v in w:
        s += float(v) * float(v)
    return 1.0 / s


@pytest.mark.gpu
@pytest.mark.parametrize("nP", [1, 63, 64, 65, 200, LIMIT])
def test_resampling_rule_against_the_host_route(pkg, nP):
    """Weights set by hand, then resample_async against FilterBatch.update_and_resample on a twin with the restated draws."""
    names = ["uniform", "dominant", "zeros", "runs", "random", "gate_updates", "gate_measurements", "no_measurements"]
    nF = len(names)
    rng = np.random.default_rng(1000 + nP)
    seeds = [31 + 7 * b for b in range(nF)]
    eff_n = np.full(nF, 0.5 * nP)
    a, b = pkg.FilterBatch(nF, nP, gm_capacity=16), pkg.FilterBatch(nF, nP, gm_capacity=16)
    x0 = rng.uniform(-5, 5, (nF * nP, 3))
    masks = rng.integers(1, 2 ** 40, size=nF * nP, dtype=np.uint64)
    for bt in (a, b):
        rng = np.random.default_rng(2000 + nP)                   # the same mixtures for both
        bt.set_poses(x0, np.tile(np.diag([1e-3, 2e-3, 3e-3]).ravel(), (nF * nP, 1)))
        bt.set_unused_masks(masks)
        for q in range(nF):
            cfg = bt.default_filter_config()
            cfg.minUpdatesBeforeResample = 3 if names[q] == "gate_updates" else 1
            cfg.minMeasurementsBeforeResample = 50 if names[q] == "gate_measurements" else 1
            bt.configure(q, cfg)
        for q in range(nF):                                       # mixtures at the dominant particle's slot, at regular slots and at random ones
            slots = set(range(0, nP, max(1, nP // 5))) | {nP // 3} | set(int(v) for v in rng.choice(nP, size=min(nP, 6), replace=False))
            for i in sorted(slots):
                m = 1 + (i + q) % 3
                bt.import_gm(q * nP + i, rng.uniform(0.2, 1, m), rng.normal(0, 3, (m, 2)), np.tile(np.eye(2) * 0.01, (m, 1, 1)))
    filled0 = (a.gm_sizes() > 0).reshape(nF, nP).sum(axis=1)
    assert (filled0 >= min(nP, 5)).all()
    for q in range(nF):
        a.set_motion_odometry(q, [0, 0, 0], seeds[q])
        a.set_resampling(q, eff_n[q], eff_n[q] / nP)
    rng = np.random.default_rng(3000 + nP)
    total = np.zeros(nF, dtype=np.int64)
    for call in (0, 5, 1 << 33, 9):
        w = np.concatenate([_weights_case(n if not n.startswith(("gate", "no_")) else "dominant", nP, rng) for n in names])
        n_z = np.array([0 if n == "no_measurements" else 4 for n in names], dtype=np.int32)
        for q in range(nF):                                      # no case may sit at its threshold
            ne = _sequential_neff(w[a.block(q)])
            assert abs(ne - eff_n[q]) > 1e-9 * eff_n[q], (names[q], ne)
        for bt in (a, b):
            bt.set_weights(w)
        a.resample_async(n_z, call)
        draws = np.array([dl.resample_draw(seeds[q], call) for q in range(nF)])
        fired_b, plan_b = b.update_and_resample(n_z, draws, eff_n)
        fired_a, plan_a, neff_a = a.last_resample()
        np.testing.assert_array_equal(fired_a, fired_b, err_msg=f"call {call}: decisions")
        np.testing.assert_array_equal(plan_a, plan_b, err_msg=f"call {call}: plans")
        for q in range(nF):
            if names[q] in ("no_measurements",) or (names[q].startswith("gate") and not fired_a[q] and neff_a[q] == 0.0):
                continue
            np.testing.assert_allclose(neff_a[q], _sequential_neff(w[a.block(q)]), rtol=1e-14, err_msg=names[q])
        assert not fired_a[names.index("uniform")] and not fired_a[names.index("no_measurements")]
        if nP > 2:
            assert fired_a[names.index("dominant")]
        total += fired_a
        np.testing.assert_array_equal(a.resample_counts(), total)
        np.testing.assert_array_equal(_bits(a.get_poses()), _bits(b.get_poses()), err_msg="poses")
        ia, ib = a.get_particle_ids(), b.get_particle_ids()
        np.testing.assert_array_equal(ia[0], ib[0], err_msg="ids")
        np.testing.assert_array_equal(ia[1], ib[1], err_msg="parent ids")
        np.testing.assert_array_equal(a.batch_resample_occured(), b.batch_resample_occured())
        _assert_same_state(a, b, mixtures="nonempty" if nP > 200 else True, what=f"call {call}")
        if call == 0 and nP > 2:                                  # the gather on the device plan moved real mixtures
            d = names.index("dominant")
            assert (a.gm_sizes()[a.block(d)] > 0).sum() > filled0[d]
            assert (plan_a[a.block(d)] == d * nP + nP // 3).sum() > nP // 2
        # the next predict inherits the unused lists the same way on both routes (no update has happened: the serial walk)
        for bt in (a, b):
            bt.cycle_async(True, _empty(nF), normalize=False)
        _assert_same_state(a, b, mixtures=False, what=f"call {call}, after the predict")
    if nP > 2:
        # held by the gates at first, released later: gate_updates fires from its third call on, gate_measurements never (4 per call < 50)
        assert total[names.index("gate_updates")] >= 1 and total[names.index("gate_measurements")] == 0


def _trajectory_setup(pkg, K):
    from test_filter_batch import _setup
    sim = pkg.sim2d_driver

    def tweak(b, P):
        if b == 2:
            P["use_cluster"] = 1

    return _setup(sim, 6, K, tweak)


@pytest.fixture(scope="module")
def lockstep(pkg):
    """Batch A on the device loop, read after every call; batch B on the host route with A's propagated poses and the restated draws.
    The filters, realisations and seeds are those of test_batch_equals_independent_handles_over_whole_trajectories, whose coverage
    assertions (partial resamplings, mixed empty sets) hold for them under the host loop's numpy draws."""
    sim = pkg.sim2d_driver
    nF, nP, K = 6, 200, 301
    Ps, datas, seeds = _trajectory_setup(pkg, K)
    A = pkg.FilterBatch(nF, nP, gm_capacity=512)
    B = pkg.FilterBatch(nF, nP, gm_capacity=512)
    ra = sim.Sim2dBatchRun(A, datas, Ps, seeds, track_errors=True, device_loop=True)
    rb = sim.Sim2dBatchRun(B, datas, Ps, seeds)                  # (configures B; its own randomness is not used)
    mixed_empty = partial_then_predict = 0
    prev_partial = False
    counts = np.zeros(nF, dtype=np.int64)
    for k in range(1, K):
        ra._device_propagate(k)
        x = A.get_poses()
        cov = A.get_pose_covs().reshape(-1, 9)
        ra._device_update(k)
        Zs = [d["Z"][k] for d in datas]
        n_z = np.array([len(Z) for Z in Zs])
        B.cycle_async(True, Zs, poses=x, pose_cov=cov, normalize=True)
        draws = np.array([dl.resample_draw(seeds[b], k) for b in range(nF)])
        fired_b, plan_b = B.update_and_resample(n_z, draws, rb.eff_n)
        fired_a, plan_a, _ = A.last_resample()
        np.testing.assert_array_equal(fired_a, fired_b, err_msg=f"step {k}: decisions")
        np.testing.assert_array_equal(plan_a, plan_b, err_msg=f"step {k}: plans")
        counts += fired_a
        if (n_z == 0).any() and (n_z > 0).any():
            mixed_empty += 1
        if prev_partial:
            partial_then_predict += 1
        prev_partial = bool(fired_a.any() and not fired_a.all())
        np.testing.assert_allclose(A.get_weights(), B.get_weights(), rtol=1e-12, atol=0, err_msg=f"step {k}: weights")
        np.testing.assert_array_equal(A.gm_sizes(), B.gm_sizes(), err_msg=f"step {k}: sizes")
        np.testing.assert_array_equal(A.get_unused_masks(), B.get_unused_masks(), err_msg=f"step {k}: unused masks")
        ia, ib = A.get_particle_ids(), B.get_particle_ids()
        np.testing.assert_array_equal(ia[0], ib[0], err_msg=f"step {k}: ids")
        np.testing.assert_array_equal(ia[1], ib[1], err_msg=f"step {k}: parent ids")
        if k % 10 == 0 or k == K - 1:
            for i in range(A.n):
                for p, q in zip(A.export_gm(i), B.export_gm(i)):
                    np.testing.assert_array_equal(_bits(p), _bits(q), err_msg=f"step {k} slot {i}: mixture")
    assert mixed_empty > 0, "no cycle had empty and non-empty measurement sets side by side"
    assert partial_then_predict > 0, "no cycle followed one in which only some filters resampled"
    assert (counts > 0).sum() >= 2
    np.testing.assert_array_equal(A.resample_counts(), counts)
    return dict(w=A.get_weights(), x=A.get_poses(), sizes=A.gm_sizes(), gm=[A.export_gm(i) for i in range(A.n)], counts=counts, log=ra.errors())


@pytest.mark.gpu
def test_device_loop_in_lock_step_with_the_host_route(lockstep):
    """The comparison is the fixture's (a failure there is reported as this test's and the next one's set-up error)."""
    assert lockstep["counts"].sum() > 0


@pytest.mark.gpu
def test_free_running_device_loop_equals_the_lock_step_run(pkg, lockstep):
    """The same run with nothing read until the end: asynchrony and the reuse of the pinned rings change no bit."""
    want = lockstep
    sim = pkg.sim2d_driver
    nF, nP, K = 6, 200, 301
    Ps, datas, seeds = _trajectory_setup(pkg, K)
    Cb = pkg.FilterBatch(nF, nP, gm_capacity=512)
    rc = sim.Sim2dBatchRun(Cb, datas, Ps, seeds, track_errors=True, device_loop=True).run(1, K)
    np.testing.assert_array_equal(rc.resample_counts(), want["counts"])
    np.testing.assert_array_equal(_bits(Cb.get_weights()), _bits(want["w"]))
    np.testing.assert_array_equal(_bits(Cb.get_poses()), _bits(want["x"]))
    np.testing.assert_array_equal(Cb.gm_sizes(), want["sizes"])
    for i in range(Cb.n):
        for p, q in zip(Cb.export_gm(i), want["gm"][i]):
            np.testing.assert_array_equal(_bits(p), _bits(q), err_msg=f"slot {i}: mixture")
    log = rc.errors()
    assert log.shape == want["log"].shape
    assert log.tobytes() == want["log"].tobytes()


@pytest.mark.gpu
def test_device_loop_refusals(pkg):
    capi = pkg.capi
    lib = pkg.load_library()
    batch = pkg.FilterBatch(3, 8, gm_capacity=16)
    nz = np.array([1, 1, 1], dtype=np.int32)
    u = np.zeros((3, 3))
    batch.set_motion_odometry(0, [1e-3, 1e-3, 1e-3], 1)
    batch.set_motion_odometry(2, [1e-3, 1e-3, 1e-3], 3)
    with pytest.raises(capi.EngineError) as e:
        batch.propagate_async(u, 0)
    assert e.value.status == capi.ERR_INVALID and "filter 1" in str(e.value)
    batch.set_motion_odometry(1, [0, 0, 0], 2)
    batch.propagate_async(u, 0)
    batch.set_resampling(0, 4.0, 0.5)
    batch.set_resampling(1, 4.0, 0.5)
    with pytest.raises(capi.EngineError) as e:
        batch.resample_async(nz, 0)
    assert e.value.status == capi.ERR_INVALID and "filter 2" in str(e.value)
    with pytest.raises(capi.EngineError) as e:
        batch.set_motion_odometry(3, [0, 0, 0], 1)
    assert e.value.status == capi.ERR_INVALID
    # a plain handle is no batch
    plain = pkg.RBPHDFilter(8, gm_capacity=16)
    var = np.zeros(3)
    for name, args in [("batch_set_motion_odometry", (C.c_int(0), var.ctypes.data_as(C.c_void_p), C.c_ulonglong(1))),
                       ("batch_set_resampling", (C.c_int(0), C.c_double(1.0), C.c_double(0.5))),
                       ("batch_propagate_async", (u.ctypes.data_as(C.c_void_p), None, None, C.c_ulonglong(0))),
                       ("batch_resample_async", (nz.ctypes.data_as(C.c_void_p), C.c_ulonglong(0))),
                       ("batch_last_resample", (None, None, None)),
                       ("batch_resample_counts", (np.zeros(1, dtype=np.int64).ctypes.data_as(C.c_void_p),)),
                       ("batch_get_pose_covs", (np.zeros(72).ctypes.data_as(C.c_void_p),))]:
        fn = getattr(lib, "rfsgpu_" + name)
        fn.restype = C.c_int
        assert fn(plain._h, *args) == capi.ERR_INVALID, name
    # beyond the limit of the one-workgroup form
    big = pkg.FilterBatch(1, LIMIT + 1, gm_capacity=16)
    big.set_motion_odometry(None, [0, 0, 0], 1)
    big.set_resampling(None, 10.0, 0.5)
    with pytest.raises(capi.EngineError) as e:
        big.resample_async(np.array([1], dtype=np.int32), 0)
    assert e.value.status == capi.ERR_UNSUPPORTED
    # the routes do not mix: host route first is carried over, host route after the device route is refused
    batch.set_resampling(2, 4.0, 0.5)
    plan = np.arange(24, dtype=np.int32)
    plan[9] = 10
    batch.batch_resample_apply(plan, np.array([0, 1, 0]))
    ids_before = batch.get_particle_ids()
    batch.resample_async(np.zeros(3, dtype=np.int32), 1)
    assert list(batch.batch_resample_occured()) == [False, True, False]
    ids_after = batch.get_particle_ids()
    np.testing.assert_array_equal(ids_before[0], ids_after[0])
    np.testing.assert_array_equal(ids_before[1], ids_after[1])
    with pytest.raises(capi.EngineError) as e:
        batch.batch_resample_apply(plan, np.array([0, 1, 0]))
    assert e.value.status == capi.ERR_UNSUPPORTED and "device" in str(e.value)
