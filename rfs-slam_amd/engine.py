"""Loader for librfsgpu.so + the host-side mirror of rfs::RBPHDFilter for the device path.

`RBPHDFilter` mirrors the reference class's public members for the hot path
(include/RBPHDFilter.hpp:72-251): predict-side map ops, update(), getGMSize(), getLandmark(),
getTimingInfo(), public `config`; resampling follows ParticleFilter::resample
(include/ParticleFilter.hpp:399-492) on the host exactly like the reference (host RNG), and hands
the copy plan to the device through rfsgpu_resample_apply.
"""
import ctypes as C
import os
import numpy as np

from . import capi
from .build import LIB

_lib = None


def load_library():
    """dlopen the in-tree HIP extension.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError(
                f"{LIB} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no CPU fallback for the device path.")
        _lib = C.CDLL(LIB)
        _lib.rfsgpu_abi_version.restype = C.c_int
    return _lib


def mat_perm(A, device_id=0):
    return capi.mat_perm(load_library(), "rfsgpu_", A, device_id)


def FilterGroup(n_particles, device_ids, gm_capacity=512, model=capi.MODEL_RNGBRG_2D):
    """One filter over several GPUs from this process (rfsgpu_group_*): contiguous particle blocks, one shard per device id."""
    return capi.Group(load_library(), n_particles, device_ids, gm_capacity=gm_capacity, model=model)


class RBPHDFilter(capi.CFilter):
    """Device-resident RB-PHD filter shard (one GPU).  Mirrors rfs::RBPHDFilter for the update path."""

    def __init__(self, n_particles, device_id=0, gm_capacity=512, model=capi.MODEL_RNGBRG_2D, max_particles=None):
        super().__init__(load_library(), "rfsgpu_", n_particles, model=model, device_id=device_id, gm_capacity=gm_capacity,
                         max_particles=max_particles)
        self.config = self.default_filter_config()
        self.n_init = n_particles
        self.effNParticles_t = n_particles / 4.0  # ParticleFilter.hpp:232
        self.effNParticles_t_percent = self.effNParticles_t / n_particles
        self.nUpdatesSinceResample = 0
        self.nMeasurementsSinceResample = 0
        self.resampleOccured = False
        self.last_resample_plan = None    # src slot per slot of the last resampling that fired (None when the last call did not)
        self.last_n_eff = None            # N_eff of the last resample(device=True) (0 when forced)
        self._pending_u01 = None          # the draw a device resampling that did not fire has left unused (the next call's)

    # ParticleFilter::setEffectiveParticleCountThreshold (ParticleFilter.hpp:386-391)
    def setEffectiveParticleCountThreshold(self, t):
        self.effNParticles_t = float(t)
        self.effNParticles_t_percent = float(t) / self.n   # the particle count at the time of the call (:390)

    def apply_config(self):
        self.set_filter_config(self.config)

    def last_kernel_ns(self):
        ns = (C.c_longlong * 4)()
        self._call("last_kernel_ns", ns)
        return list(ns)

    def last_step_variant(self):
        """{waves per particle, phase priorities, merge grid log2, fused} of the last stream-ordered step."""
        out = (C.c_int * 4)()
        self._call("last_step_variant", out)
        return tuple(out)

    def update_async(self, Z):
        """Stream-ordered update: no host sync; errors surface at synchronize()."""
        Z, n = self._z(Z)
        self._call("update_async", self._ptr(Z), n)

    def step_async(self, Z, normalize=True):
        """update_async + the weight reduction (and, with normalize, the division) in the step's post kernel."""
        Z, n = self._z(Z)
        self._call("step_async", self._ptr(Z), n, C.c_int(1 if normalize else 0))

    def step_async_deferred(self, Z, prev_total_ptr=None, wait_event=None):
        """rfsgpu_step_async_deferred: the step of a sharded host whose normalisation trails by one step (the post kernel divides by
        the previous step's all-reduced total, device pointer, and waits for `wait_event` -- a hipEvent_t handle -- just before it)."""
        Z, n = self._z(Z)
        self._call("step_async_deferred", self._ptr(Z), n, C.c_void_p(prev_total_ptr), C.c_void_p(wait_event))

    def step_async_trailing(self, Z, total_ptr, have_prev):
        """rfsgpu_step_async_trailing: the deferred step without stream events (pair with collective_gate / collective_publish on the side stream)."""
        Z, n = self._z(Z)
        self._call("step_async_trailing", self._ptr(Z), n, C.c_void_p(total_ptr), C.c_int(1 if have_prev else 0))

    def collective_gate(self, hip_stream):
        self._call("collective_gate", C.c_void_p(hip_stream))

    def collective_publish(self, hip_stream):
        self._call("collective_publish", C.c_void_p(hip_stream))

    def collective_probe(self, hip_stream):
        """rfsgpu_collective_probe: do the engine's stream and `hip_stream` make progress side by side (what the sequence-number
        hand-over needs)?  Synchronises both streams."""
        ok = C.c_int(0)
        self._call("collective_probe", C.c_void_p(hip_stream), C.byref(ok))
        return bool(ok.value)

    def _opt(self, a, shape=None):
        if a is None:
            return None, C.c_void_p(None)
        a = np.ascontiguousarray(a, dtype=np.float64)
        if shape is not None:
            assert a.shape == shape, (a.shape, shape)
        return a, self._ptr(a)

    def cycle_async(self, predict, Z, poses=None, pose_cov=None, weights=None, normalize=True):
        """One submission per predict + update cycle (rfsgpu_cycle_async): predict = None (no predict part), False (static step
        only) or True (births + static step); poses / pose_cov / weights = the host's new inputs or None (unchanged)."""
        Z, n = self._z(Z)
        x, px = self._opt(poses, (self.n, 3))
        stride = 0
        if pose_cov is not None:
            pose_cov = np.ascontiguousarray(pose_cov, dtype=np.float64)
            assert pose_cov.size in (9, 9 * self.n)
            stride = 0 if pose_cov.size == 9 else 9
        cv, pc = self._opt(pose_cov)
        w, pw = self._opt(weights, (self.n,))
        self._call("cycle_async", C.c_int(-1 if predict is None else (1 if predict else 0)), px, pc, C.c_int(stride), pw, self._ptr(Z), n,
                   C.c_int(1 if normalize else 0))

    def update_io(self, Z, predict=None, poses=None, pose_cov=None, weights=None, want_weights=True):
        """RBPHDFilter::update with its inputs and outputs in one synchronous call (rfsgpu_update_io); returns the updated
        (un-normalised) particle weights."""
        Z, n = self._z(Z)
        x, px = self._opt(poses, (self.n, 3))
        stride = 0
        if pose_cov is not None:
            pose_cov = np.ascontiguousarray(pose_cov, dtype=np.float64)
            assert pose_cov.size in (9, 9 * self.n)
            stride = 0 if pose_cov.size == 9 else 9
        cv, pc = self._opt(pose_cov)
        w, pw = self._opt(weights, (self.n,))
        out = np.empty(self.n, dtype=np.float64) if want_weights else None
        self._call("update_io", C.c_int(-1 if predict is None else (1 if predict else 0)), px, pc, C.c_int(stride), pw, self._ptr(Z), n,
                   self._ptr(out) if want_weights else C.c_void_p(None))
        return out

    def kernel_time_stats(self):
        avg = (C.c_double * 3)()
        n = C.c_int()
        self._call("kernel_time_stats", avg, C.byref(n))
        return list(avg), n.value

    def post_kernel_avg_ns(self):
        """Average duration of the step's post kernel over the fused steps the last kernel_time_stats() call covered."""
        fn = self._fn("post_kernel_avg_ns")
        fn.restype = C.c_double
        return float(fn(self._h))

    def step_launch_order(self, order=None, mode=None, want_costs=True):
        """rfsgpu_step_launch_order: the last Victoria Park step's per-particle durations (ticks) out; launch order in: `order` (slot ->
        particle, frozen: mode 1), or mode 0 (slot == particle) / mode 2 (re-sorted by every step's post kernel, the default)."""
        cost = np.zeros(self.n, dtype=np.float32) if want_costs else None
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        m = 1 if order is not None else (2 if mode is None else int(mode))
        self._call("step_launch_order", C.c_int(m), None if o is None else o.ctypes.data_as(C.c_void_p),
                   None if cost is None else cost.ctypes.data_as(C.c_void_p))
        return cost

    def set_step_timing_stride(self, every):
        """HIP events (kernel_time_stats / post_kernel_avg_ns) on every `every`-th fused stream-ordered step only."""
        self._call("set_step_timing_stride", C.c_int(int(every)))

    def weight_sums_async(self):
        self._call("weight_sums_async")

    def weight_sums_device_ptr(self):
        fn = self._fn("weight_sums_device_ptr")
        fn.restype = C.c_void_p
        return fn(self._h)

    def set_stream(self, hip_stream):
        self._call("set_stream", C.c_void_p(hip_stream))

    def bind_weight_sums_buffer(self, dev_ptr):
        self._call("bind_weight_sums_buffer", C.c_void_p(dev_ptr))

    def save_state(self):
        self._call("save_state")

    def restore_state(self):
        self._call("restore_state")

    def state_ring_create(self, n_slots):
        """n_slots pre-seeded copies of the saved state (bench.py: the inputs of the timed steps are resident before the timed region)."""
        self._call("state_ring_create", C.c_int(int(n_slots)))

    def state_ring_seed(self):
        self._call("state_ring_seed")

    def state_ring_next(self):
        self._call("state_ring_next")

    def stream(self):
        fn = self._fn("stream")
        fn.restype = C.c_void_p
        return fn(self._h)

    # RBPHDFilter::update (RBPHDFilter.hpp:444-541) including the resample-or-normalise tail.
    def update_and_resample(self, Z, u01_fn=np.random.random, device_resample=False):
        """device_resample: the resample-or-normalise tail runs on the device (rfsgpu_resample_async) when the two gates let
        resample() run; same weights, maps, ids and decisions as the host tail."""
        self.apply_config()
        self.nUpdatesSinceResample += 1
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, self.dz)
        if Z.shape[0] == 0:
            return False
        self.nMeasurementsSinceResample += Z.shape[0]
        self.update(Z)
        self.resampleOccured = False
        tail_done = False
        if (self.nUpdatesSinceResample >= self.config.minUpdatesBeforeResample and
                self.nMeasurementsSinceResample >= self.config.minMeasurementsBeforeResample):
            self.resampleOccured = self.resample(u01_fn, device=device_resample, renormalize=device_resample)
            tail_done = bool(device_resample)       # (the device has normalised a second time where nothing fired)
        if self.resampleOccured:
            self.nUpdatesSinceResample = 0
            self.nMeasurementsSinceResample = 0
        elif not tail_done:
            s = self.weight_sums()
            self.normalize_weights(s[0])
        return self.resampleOccured

    # ParticleFilter::resample (ParticleFilter.hpp:399-492): host logic on the N weights.
    # resample(n, forceResample): n == 0 or n > nParticles_ keeps the count (:417-418); a smaller n shrinks the particle set
    # (FastSLAM::resampleWithMapCopy after multi-hypothesis growth).  The plan of the last resampling stays in
    # `last_resample_plan` so that a caller holding per-particle host data (poses) can apply the same copies.
    # device=True: the whole of it as one rfsgpu_resample_async.  The device needs the draw before the decision is known, so a
    # draw that a non-firing call leaves unused is kept for the next call: the k-th resampling uses the k-th draw of u01_fn, as
    # on the host route.  renormalize: RBPHDFilter::update's second normalisation when nothing fired (device route only).
    def resample(self, u01_fn=np.random.random, n_out=0, force=False, device=False, renormalize=False):
        self.last_resample_plan = None
        if device:
            if self._pending_u01 is None:
                self._pending_u01 = float(u01_fn())
            self.resample_async(self.effNParticles_t, self.effNParticles_t_percent, self._pending_u01, n_out, force, renormalize)
            lr = self.last_resample()
            self.last_n_eff = lr["n_eff"]
            if not lr["fired"]:
                return False
            self._pending_u01 = None
            self.last_resample_plan = lr["plan"]
            return True
        s = self.weight_sums()
        self.normalize_weights(s[0])
        w = self.get_weights()
        n = self.n
        if not force:
            neff = 1.0 / float(np.sum(w * w))
            if neff > self.effNParticles_t and neff / n > self.effNParticles_t_percent:
                return False
        if n_out == 0 or n_out > n:
            n_out = n
        src = systematic_resample_plan(w, float(u01_fn()), n_out)
        self.resample_apply(src, n_out)
        self.last_resample_plan = src
        return True

    # RBPHDFilter::update as one rfsgpu_rbphd_cycle_async: the two counters, the gate and the resampling are the device's.
    def cycle_on_device(self, Z, u01, scan=None, push_config=True):
        """One whole update enqueued, nothing read back: u01 is the draw a resampling would use (made whether or not one happens:
        the decision is the device's), scan this update's laser scan (Victoria Park model).  Cycles, static steps, Ackerman
        propagations and predict_map_async -- births included -- may follow one another without a synchronisation; sync_cycle()
        brings resampleOccured and last_resample_plan up to date.  push_config=False: the configuration and the thresholds were
        pushed by an earlier call and have not changed."""
        if push_config:
            self.apply_config()
            self.rbphd_set_resampling(self.effNParticles_t, self.effNParticles_t_percent)
        self.rbphd_cycle_async(np.asarray(Z, dtype=np.float64).reshape(-1, self.dz), u01, scan=scan)

    def sync_cycle(self):
        """The results of the last cycle_on_device (resolves)."""
        lc = self.rbphd_last_cycle()
        self.resampleOccured = bool(self.resample_occured())
        self.last_n_eff = lc["n_eff"]
        self.last_resample_plan = lc["plan"] if lc["fired"] else None
        return lc


class FastSLAM(RBPHDFilter):
    """rfs::FastSLAM (include/FastSLAM.hpp) for the 2-D range-bearing model on the same engine: the handle's mixtures are
    the landmark maps (weights = log-odds of existence).  With fs_config.maxNDataAssocHypotheses > 1 (MH-FastSLAM) an update
    multiplies particles (one per kept association hypothesis, :462-476): build the filter with `max_hypotheses` so that the
    handle has room for nParticlesMax * max_hypotheses particles; `parents` (slot -> the particle it was copied from in the
    last update) and `last_resample_plan` let a caller holding poses follow the copies."""

    def __init__(self, n_particles, device_id=0, gm_capacity=512, max_hypotheses=1, n_particles_max=None, device_cycle=False, max_particles=None,
                 model=capi.MODEL_RNGBRG_2D):
        n_max = 3 * n_particles if n_particles_max is None else int(n_particles_max)    # FastSLAM.hpp:250
        cap = max(n_particles, n_max) * max(1, int(max_hypotheses)) if max_hypotheses > 1 else None
        if max_particles is not None:       # the handle's particle slots, given outright (the yardstick of one filter of an MHFastSLAMBatch)
            cap = int(max_particles)
        super().__init__(n_particles, device_id=device_id, gm_capacity=gm_capacity, max_particles=cap, model=model)
        self.model = model
        self.fs_config = self.default_fastslam_config()
        self.fs_config.nParticlesMax = n_max
        self.fs_config.maxNDataAssocHypotheses = max(1, int(max_hypotheses))
        self.parents = np.arange(n_particles, dtype=np.int32)
        self.last_resample_plan = None
        # device_cycle: update_and_resample runs as one rfsgpu_fastslam_cycle_async (copy plan and resampleWithMapCopy on the device,
        # no host round trip inside the cycle); the handle must hold max_particles <= 2048.  The Victoria Park model and landmark
        # candidate lists (landmarkCandidateMeasurementCountThreshold != 1) go through rfsgpu_fastslam_cycle_full_async.
        self.device_cycle = bool(device_cycle)
        self.last_cycle = None

    def uses_full_cycle(self):
        """Whether device_cycle goes through rfsgpu_fastslam_cycle_full_async: the Victoria Park model, or landmark candidate lists."""
        return self.model != capi.MODEL_RNGBRG_2D or int(self.fs_config.landmarkCandidateMeasurementCountThreshold) != 1

    def cycle_async(self, Z, u01, predict=False, scan=None, push_config=True):
        """One whole FastSLAM::update enqueued, nothing read back (rfsgpu_fastslam_cycle_async, or rfsgpu_fastslam_cycle_full_async
        where uses_full_cycle()): u01 is the draw a resampling would use; scan: this update's laser scan (Victoria Park model).
        Cycles may follow one another without a synchronisation; sync_cycle() brings parents / last_resample_plan / resampleOccured
        up to date.  push_config=False: the configuration was pushed by an earlier call and has not changed."""
        if push_config:
            self.apply_config()
            self.set_fastslam_config(self.fs_config)
            self.fastslam_set_resampling(self.effNParticles_t, self.effNParticles_t_percent)
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, self.dz)
        if scan is not None or self.uses_full_cycle():
            self.fastslam_cycle_full_async(Z, u01, self.n_init, predict, scan=scan)
        else:
            self.fastslam_cycle_async(Z, u01, self.n_init, predict)

    def sync_cycle(self):
        """The results of the last cycle_async (synchronises)."""
        lc = self.fastslam_last_cycle()
        self.last_cycle = lc
        self.parents = lc["parent"]
        self.resampleOccured = lc["fired"]
        self.last_resample_plan = lc["plan"] if lc["fired"] else None
        return lc

    # FastSLAM::predict (:362-385), map part: staticStep on every landmark, no births
    def predict_map(self, add_birth=False):
        super().predict_map(False)

    # FastSLAM::update (:387-421) + resampleWithMapCopy (:708-735)
    def update_and_resample(self, Z, u01_fn=np.random.random):
        if self.device_cycle:
            # the draw is made whether or not the cycle resamples: the decision is the device's, and the host reads nothing before it.
            # The two counters the gates use live on the device on this route; the host's copies follow them.
            Z = np.asarray(Z, dtype=np.float64).reshape(-1, self.dz)
            self.cycle_async(Z, float(u01_fn()))
            self.nUpdatesSinceResample += 1
            if Z.shape[0] == 0:
                return False
            self.nMeasurementsSinceResample += Z.shape[0]
            lc = self.sync_cycle()
            if lc["fired"]:
                self.nUpdatesSinceResample = 0
                self.nMeasurementsSinceResample = 0
            return lc["fired"]
        self.apply_config()
        self.set_fastslam_config(self.fs_config)
        self.nUpdatesSinceResample += 1
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, self.dz)
        if Z.shape[0] == 0:
            return False
        self.nMeasurementsSinceResample += Z.shape[0]
        self.fastslam_update(Z)                               # the particle count may have grown (self.n)
        self.parents = self.particle_parents()
        self.resampleOccured = False
        self.last_resample_plan = None
        if self.n > self.fs_config.nParticlesMax:             # :711-712 forced, back to the initial count
            self.resampleOccured = self.resample(u01_fn, self.n_init, True)
        elif (self.nUpdatesSinceResample >= self.fs_config.minUpdatesBeforeResample and
                self.nMeasurementsSinceResample >= self.fs_config.minMeasurementsBeforeResample):
            self.resampleOccured = self.resample(u01_fn, self.n_init)   # landmark candidates travel with their particle
        self.fastslam_set_resample_occured(self.resampleOccured)
        if self.resampleOccured:
            self.nUpdatesSinceResample = 0
            self.nMeasurementsSinceResample = 0
        else:
            s = self.weight_sums()
            self.normalize_weights(s[0])
        return self.resampleOccured


def systematic_resample_plan(w, u01, n_out=None):
    """Systematic sampling + slot assignment of ParticleFilter::resample (ParticleFilter.hpp:419-479).
    Returns src_slot[k]: which (kept-in-place) particle slot k copies; k itself when it is kept.
    n_out < len(w): resample(n) as FastSLAM::resampleWithMapCopy calls it -- n_out samples from all particles, kept or
    copied into the first n_out slots (cases 1-4 of :459-478); the returned plan has n_out entries."""
    if n_out is not None and n_out < w.size:
        return _systematic_resample_plan_shrink(w, u01, int(n_out))
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    if n >= 256 and not (w < 0).any() and np.isfinite(w).all():
        return _systematic_resample_plan_vectorised(w, u01)
    return _systematic_resample_plan_loop(w, u01)


def _systematic_resample_plan_vectorised(w, u01):
    """The same plan without Python loops (20 000 particles at configs[2]).  np.cumsum adds sequentially in index order, i.e.
    the reference's `cumulative_weight += w[idx]` and `sample_point += sample_interval` roundings exactly; with non-negative
    weights the running sum is non-decreasing, so `while (sample_point > cumulative && idx < n-1) idx++` is a search."""
    n = w.size
    interval = 1.0 / float(n)
    cum = np.cumsum(w)
    steps = np.full(n, interval)
    steps[0] = interval * u01
    sp = np.cumsum(steps)
    sampled_idx = np.minimum(np.searchsorted(cum, sp, side="left"), n - 1)
    sampled_idx = np.maximum.accumulate(sampled_idx)      # (idx never moves back; a no-op for monotone sums)
    sampled = np.zeros(n, dtype=bool)
    sampled[sampled_idx] = True
    first = np.ones(n, dtype=bool)
    first[1:] = sampled_idx[1:] != sampled_idx[:-1]
    dups = sampled_idx[~first]                             # sources of the copies, in sampling order
    free = np.nonzero(~sampled)[0]                         # un-sampled slots, ascending: they take the copies in order
    src = np.arange(n, dtype=np.int32)
    src[free[:dups.size]] = dups
    return src


def _systematic_resample_plan_loop(w, u01):
    n = w.size
    interval = 1.0 / float(n)
    sample_point = interval * u01
    idx = 0
    cumulative = w[0]
    sampled = np.zeros(n, dtype=bool)
    sampled_idx = np.zeros(n, dtype=np.int64)
    for i in range(n):
        while sample_point > cumulative and idx < n - 1:
            idx += 1
            cumulative += w[idx]
        sampled_idx[i] = idx
        sampled[idx] = True
        sample_point += interval
    src = np.arange(n, dtype=np.int32)
    nxt = 0
    prev = -1
    for i in range(n):
        idx = int(sampled_idx[i])
        first = not (i > 0 and idx == prev)
        prev = idx
        if first:
            continue
        while nxt < n and sampled[nxt]:
            nxt += 1
        src[nxt] = idx
        nxt += 1
    return src


def _systematic_resample_plan_shrink(w, u01, n):
    N = w.size
    interval = 1.0 / float(n)
    sample_point = interval * u01
    idx = 0
    cumulative = w[0]
    sampled = np.zeros(N, dtype=bool)
    sampled_idx = np.zeros(n, dtype=np.int64)
    for i in range(n):
        while sample_point > cumulative and idx < N - 1:
            idx += 1
            cumulative += w[idx]
        sampled_idx[i] = idx
        sampled[idx] = True
        sample_point += interval
    src = np.arange(n, dtype=np.int32)
    nxt = 0
    prev = -1
    for i in range(n):
        idx = int(sampled_idx[i])
        first = not (i > 0 and idx == prev)
        prev = idx
        if idx < n and first:          # case 1: stays where it is
            continue
        while nxt < N and sampled[nxt]:
            nxt += 1
        assert nxt < n, "copies always land below the new count"
        src[nxt] = idx
        nxt += 1
    return src


class FilterBatch(capi.CBatch):
    """n_filters independent 2-D RB-PHD filters stepped together (rfsgpu_create_batch): one fused launch + one post launch per cycle for
    all of them.  Filter b owns the global slots [b * n_per_filter, (b + 1) * n_per_filter); each filter has its own configuration,
    measurement set, weights, normalisation and resampling, and equals a separate RBPHDFilter given the same inputs."""

    def __init__(self, n_filters, n_per_filter, device_id=0, gm_capacity=512, model=capi.MODEL_RNGBRG_2D):
        super().__init__(load_library(), "rfsgpu_", n_filters, n_per_filter, model=model, device_id=device_id, gm_capacity=gm_capacity)
        self.configs = [self.default_filter_config() for _ in range(n_filters)]
        self.nUpdatesSinceResample = np.zeros(n_filters, dtype=np.int64)
        self.nMeasurementsSinceResample = np.zeros(n_filters, dtype=np.int64)

    def configure(self, b, cfg=None, **model):
        """Filter b's configuration (see CBatch.batch_configure); cfg also becomes self.configs[b] (the resampling thresholds)."""
        if cfg is not None:
            self.configs[b] = cfg
        self.batch_configure(b, cfg=cfg, **model)

    def cycle_async(self, predict, Zs, poses=None, pose_cov=None, normalize=True):
        """One predict + update cycle of every filter (rfsgpu_batch_cycle_async)."""
        self.batch_cycle_async(predict, Zs, poses=poses, pose_cov=pose_cov, normalize=normalize)

    def _gate_config(self, b):
        """The configuration whose minUpdatesBeforeResample / minMeasurementsBeforeResample gate filter b's resampling."""
        return self.configs[b]

    def weight_sums_per_filter(self):
        """{sum w, sum w^2} of each filter: [n_filters, 2]."""
        return self.batch_weight_sums()

    def normalize_per_filter(self):
        """Divide each filter's weights by their own sum (ParticleFilter::normalizeWeights per filter)."""
        w = self.get_weights()
        for b in range(self.n_filters):
            blk = self.block(b)
            w[blk] = w[blk] / np.sum(w[blk])
        self.set_weights(w)

    def update_and_resample(self, n_z, u01, eff_n):
        """The tail of RBPHDFilter::update after a batch cycle with normalize (:444-539), per filter, as RBPHDFilter.update_and_resample
        does it for one handle: every cycle counts as an update (nUpdatesSinceResample_ grows before the empty-set return, :448-452), a
        filter without measurements stops there; otherwise ParticleFilter::resample's minimum-update / minimum-measurement gate and
        N_eff test, and the systematic plan (systematic_resample_plan) with that filter's draw.  u01: a callable u01(b) -> [0, 1),
        called only for a filter whose N_eff test fires (as Sim2dRun draws), or an array of draws.  One rfsgpu_batch_resample_apply for
        the filters that fire.  n_z: the cycle's measurement counts; eff_n: the N_eff threshold per filter.
        Returns (fired [n_filters] bool, plan [N] global source slots)."""
        nF, nP = self.n_filters, self.n_per_filter
        n_z = np.asarray(n_z)
        w = self.get_weights()
        fired = np.zeros(nF, dtype=bool)
        plan = np.arange(self.n, dtype=np.int32)
        for b in range(nF):
            self.nUpdatesSinceResample[b] += 1
            if n_z[b] == 0:
                continue
            self.nMeasurementsSinceResample[b] += int(n_z[b])
            c = self._gate_config(b)
            if self.nUpdatesSinceResample[b] < c.minUpdatesBeforeResample or self.nMeasurementsSinceResample[b] < c.minMeasurementsBeforeResample:
                continue
            wb = w[self.block(b)]
            neff = 1.0 / float(np.sum(wb * wb))
            if neff > eff_n[b] and neff / nP > eff_n[b] / nP:
                continue
            u = float(u01(b)) if callable(u01) else float(u01[b])
            plan[self.block(b)] = b * nP + systematic_resample_plan(wb, u)
            fired[b] = True
            self.nUpdatesSinceResample[b] = 0
            self.nMeasurementsSinceResample[b] = 0
        if fired.any():
            self.batch_resample_apply(plan, fired)
        return fired, plan


class VPFilterBatch(capi.CVPBatch):
    """n_filters independent Victoria Park RB-PHD filters stepped together (rfsgpu_create_batch with the Victoria Park model,
    rfsgpu_batch_vp_cycle_async): per cycle the births and the static step, the fused Victoria Park step and the post launch, one chain
    for all filters.  Filter b owns the global slots [b * n_per_filter, (b + 1) * n_per_filter) and has its own configuration (any
    birth thresholds: the candidate lists are per slot), model, measurement set, weights, normalisation and resampling; the laser scan
    is the batch's.  Each filter equals a separate Victoria Park RBPHDFilter given the same inputs.  serve_estimates(True) opens the
    device-side estimate log to the batch (estimate_log_create / step_estimate_async / estimate_log_read: one row per call and filter)."""

    def __init__(self, n_filters, n_per_filter, device_id=0, gm_capacity=512):
        super().__init__(load_library(), "rfsgpu_", n_filters, n_per_filter, device_id=device_id, gm_capacity=gm_capacity)
        self.configs = [self.default_filter_config() for _ in range(n_filters)]
        self.nUpdatesSinceResample = np.zeros(n_filters, dtype=np.int64)
        self.nMeasurementsSinceResample = np.zeros(n_filters, dtype=np.int64)

    def configure(self, b, cfg=None, model=None, kf=None, Q=None):
        """Filter b's configuration (see CVPBatch.batch_configure_vp); cfg also becomes self.configs[b] (the resampling thresholds)."""
        if cfg is not None:
            self.configs[b] = cfg
        self.batch_configure_vp(b, cfg=cfg, model=model, kf=kf, Q=Q)

    def cycle_async(self, predict, Zs, poses=None, pose_cov=None, scan=None, normalize=True):
        """One predict + update cycle of every filter (rfsgpu_batch_vp_cycle_async)."""
        self.batch_vp_cycle_async(predict, Zs, poses=poses, pose_cov=pose_cov, scan=scan, normalize=normalize)

    # -- the device route: a run of messages without a stop on the host (the 2-D device loop's names, on the batch's own calls) --
    def set_motion(self, b, var, geom, seed):
        """Filter b's (None: every filter's) input-noise variances (speed, steering), vehicle geometry (h, l, dx, dy) and Philox key."""
        self.batch_vp_set_motion(b, var, geom, seed)

    def set_resampling(self, b, eff_n, eff_n_percent):
        """ParticleFilter::resample's two thresholds for filter b (None: every filter); the gates are self.configs[b]'s."""
        self.batch_vp_set_resampling(b, eff_n, eff_n_percent)

    def propagate_run_async(self, u, dt, call0, noisy=None):
        """A run of odometry messages for every slot in one launch, in place (rfsgpu_batch_vp_propagate_run_async): behind the run's
        birth cycle, in front of its update cycle, which then passes poses=None."""
        self.batch_vp_propagate_run_async(u, dt, call0, noisy=noisy)

    def resample_async(self, n_z, call):
        """The tail of RBPHDFilter::update for every filter on the device (rfsgpu_batch_vp_resample_async); from the first call on
        the ids, resampleOccured_ and the counters are the device's, and update_and_resample (the host-stop route) is refused."""
        self.batch_vp_resample_async(n_z, call)

    def last_resample(self):
        """(fired, plan in global slots, n_eff) of the last resample_async (synchronising)."""
        return self.batch_vp_last_resample()

    def loop_counts(self):
        """(resamplings per filter, deepest inheritance level any device walk has met) (synchronising)."""
        return self.batch_vp_loop_counts()

    last_step_variant = RBPHDFilter.last_step_variant      # after a cycle: (1, 0, particles per workgroup of the step kernel, 1)
    step_launch_order = RBPHDFilter.step_launch_order      # the step's launch order, across the whole batch
    _gate_config = FilterBatch._gate_config
    weight_sums_per_filter = FilterBatch.weight_sums_per_filter
    update_and_resample = FilterBatch.update_and_resample


class VPFastSLAMBatch(VPFilterBatch):
    """n_filters independent Victoria Park single-hypothesis FastSLAM filters stepped together (rfsgpu_batch_vp_serve_fastslam,
    rfsgpu_batch_vp_fastslam_cycle_async): per cycle the static landmark step, the association / Kalman update / weights, the existence
    prune, the new landmarks and candidates and each filter's normalisation, one launch chain for all filters.  Each filter equals a
    separate Victoria Park FastSLAM handle given the same inputs; landmark candidate lists of any count threshold are kept, and both
    resampling routes (update_and_resample; resample_async) move them with the particle.  The model / Kalman filter / landmark noise
    of a filter come through configure(b, None, model=..., ...), the FastSLAM configuration through configure_fastslam(b, fs_cfg),
    whose two gates also decide the resampling."""

    def __init__(self, n_filters, n_per_filter, device_id=0, gm_capacity=512):
        super().__init__(n_filters, n_per_filter, device_id=device_id, gm_capacity=gm_capacity)
        self.batch_vp_serve_fastslam(True)
        self.fs_configs = [self.default_fastslam_config() for _ in range(n_filters)]

    def configure_fastslam(self, b, fs_cfg):
        """Filter b's (None: every filter's) FastSlamConfig (rfsgpu_batch_set_fastslam_config; refused for more than one hypothesis)."""
        self.batch_set_fastslam_config(b, fs_cfg)
        for q in (range(self.n_filters) if b is None else [b]):
            self.fs_configs[q] = fs_cfg

    def cycle_async(self, predict, Zs, poses=None, pose_cov=None, scan=None, normalize=True):
        """One predict (static landmark step; None: none) + FastSLAM update cycle of every filter."""
        self.batch_vp_fastslam_cycle_async(predict, Zs, poses=poses, pose_cov=pose_cov, scan=scan, normalize=normalize)

    def _gate_config(self, b):
        return self.fs_configs[b]


class FastSLAMBatch(FilterBatch):
    """n_filters independent 2-D single-hypothesis FastSLAM filters stepped together (rfsgpu_batch_fastslam_cycle_async): per cycle the
    static landmark step, the association / Kalman update / weights, the existence prune, the new landmarks and each filter's
    normalisation, one launch chain for all filters.  Each filter equals a separate FastSLAM handle given the same inputs.  The
    model / Kalman filter / landmark noise of a filter come through configure(b, None, R=..., ...) as for a FilterBatch; the FastSLAM
    configuration through configure_fastslam(b, fs_cfg), whose two gates also decide the resampling (update_and_resample, resample_async).
    serve_sensor(True) (after the first configure_fastslam) opens the device sensor and truth to the batch: set_sensor, sense_async,
    fastslam_cycle_sensed_async, resample_sensed_async, last_scan and run_truth_async; the host-fed cycle refuses once a sensed one has run."""

    def __init__(self, n_filters, n_per_filter, device_id=0, gm_capacity=512):
        super().__init__(n_filters, n_per_filter, device_id=device_id, gm_capacity=gm_capacity)
        self.fs_configs = [self.default_fastslam_config() for _ in range(n_filters)]

    def configure_fastslam(self, b, fs_cfg):
        """Filter b's (None: every filter's) FastSlamConfig (rfsgpu_batch_set_fastslam_config; refused for more than one hypothesis or a
        landmark-candidate count threshold other than 1)."""
        self.batch_set_fastslam_config(b, fs_cfg)
        for q in (range(self.n_filters) if b is None else [b]):
            self.fs_configs[q] = fs_cfg

    def cycle_async(self, predict, Zs, poses=None, pose_cov=None, normalize=True):
        """One predict (static landmark step) + FastSLAM update cycle of every filter."""
        self.batch_fastslam_cycle_async(predict, Zs, poses=poses, pose_cov=pose_cov, normalize=normalize)

    def _gate_config(self, b):
        return self.fs_configs[b]


class MHFastSLAMBatch(capi.CBatchMH):
    """n_filters independent 2-D multi-hypothesis FastSLAM filters stepped together (rfsgpu_create_batch_mh,
    rfsgpu_batch_fastslam_mh_cycle_async): per cycle one launch chain runs every filter's whole FastSLAM::update -- association with
    Murty's k best, particle copies, Kalman update, prune, new landmarks, normalisation and resampleWithMapCopy -- with each filter's
    live particle count on the device.  Filter b owns max_per_filter global slots (block(b)), of which the first live_counts()[b] are
    live; each filter equals a FastSLAM(n_per_filter, max_hypotheses=..., device_cycle=True) handle with max_particles =
    max_per_filter given the same inputs.  The model / Kalman filter / landmark noise of a filter come through configure(b, None,
    R=..., ...), the FastSLAM configuration through configure_fastslam(b, fs_cfg), the N_eff thresholds through set_resampling.
    metrics=True switches the device-side map / pose error on at construction (serve_metrics): the [metric] calls refuse otherwise.
    serve_sensor(True) opens the device sensor and truth to the batch: set_sensor, sense_async, fastslam_mh_cycle_sensed_async(predict,
    call) -- every filter's resampling draw is then the device's, of (its motion key, call) -- last_scan and run_truth_async."""

    def __init__(self, n_filters, n_per_filter, max_per_filter=None, device_id=0, gm_capacity=512, max_hypotheses=3, metrics=False):
        # default: nParticlesMax x max_hypotheses slots (a set at nParticlesMax = 3 n is not forced back, and the next update can multiply
        # it once more before any resampling), at most the 2048 one resampling workgroup holds
        m = min(2048, 3 * int(n_per_filter) * max(1, int(max_hypotheses))) if max_per_filter is None else int(max_per_filter)
        super().__init__(load_library(), "rfsgpu_", n_filters, n_per_filter, m, device_id=device_id, gm_capacity=gm_capacity)
        self.fs_configs = [self.default_fastslam_config() for _ in range(n_filters)]
        for c in self.fs_configs:
            c.nParticlesMax = 3 * int(n_per_filter)          # FastSLAM.hpp:250
        if metrics:
            self.serve_metrics(True)

    def configure(self, b, cfg=None, **model):
        """Filter b's model / Kalman filter / landmark noise (see CBatch.batch_configure)."""
        self.batch_configure(b, cfg=cfg, **model)

    def configure_fastslam(self, b, fs_cfg):
        """Filter b's (None: every filter's) FastSlamConfig: maxNDataAssocHypotheses 1 ... 16; a landmark-candidate count threshold other
        than 1 is refused."""
        self.batch_set_fastslam_config(b, fs_cfg)
        for q in (range(self.n_filters) if b is None else [b]):
            self.fs_configs[q] = fs_cfg

    def cycle_async(self, predict, Zs, u01, poses=None, pose_cov=None):
        """One whole FastSLAM::update of every filter, enqueued; nothing is read back.  u01 [n_filters]: the draws a resampling would use."""
        self.batch_fastslam_mh_cycle_async(predict, Zs, u01, poses=poses, pose_cov=pose_cov)

    def last_cycle(self):
        """What the last cycle did, per filter (synchronises): see CBatchMH.batch_fastslam_last_cycle."""
        return self.batch_fastslam_last_cycle()

    def live_counts(self):
        """The live particle count of every filter (synchronises)."""
        return self.batch_live_counts()


class VPMHFastSLAMBatch(capi.CBatchVPMH):
    """n_filters independent Victoria Park multi-hypothesis FastSLAM filters stepped together (rfsgpu_create_batch_vp_mh,
    rfsgpu_batch_vp_fastslam_mh_cycle_async): per cycle one launch chain runs every filter's whole FastSLAM::update on the Victoria Park
    models with each filter's live particle count on the device; landmark candidate lists of any count threshold are kept and travel
    with the copies of a filter whose previous cycle resampled and with every resampling.  Filter b owns max_per_filter global slots
    (block(b)) and equals a Victoria Park FastSLAM handle with max_particles = max_per_filter stepped by fastslam_cycle_full_async on
    the same inputs.  configure(b, None, model=..., kf=..., Q=...) as on a VPFilterBatch; configure_fastslam(b, fs_cfg) with 2 ... 16
    hypotheses; set_resampling for the N_eff thresholds; set_motion / propagate_run_async / static_steps_async between the cycles."""

    def __init__(self, n_filters, n_per_filter, max_per_filter=None, device_id=0, gm_capacity=512, max_hypotheses=3):
        # (the default stride: MHFastSLAMBatch's -- a set at nParticlesMax is not forced back and can multiply once more)
        m = min(2048, 3 * int(n_per_filter) * max(1, int(max_hypotheses))) if max_per_filter is None else int(max_per_filter)
        super().__init__(load_library(), "rfsgpu_", n_filters, n_per_filter, m, device_id=device_id, gm_capacity=gm_capacity)
        self.fs_configs = [self.default_fastslam_config() for _ in range(n_filters)]
        for c in self.fs_configs:
            c.nParticlesMax = 3 * int(n_per_filter)          # FastSLAM.hpp:250
            c.maxNDataAssocHypotheses = max(2, int(max_hypotheses))

    def configure(self, b, cfg=None, model=None, kf=None, Q=None):
        """Filter b's model / Kalman filter / landmark noise (see CVPBatch.batch_configure_vp)."""
        self.batch_configure_vp(b, cfg=cfg, model=model, kf=kf, Q=Q)

    def configure_fastslam(self, b, fs_cfg):
        """Filter b's (None: every filter's) FastSlamConfig: maxNDataAssocHypotheses 2 ... 16 (1 is refused, naming the filter), any
        landmark-candidate count threshold."""
        self.batch_set_fastslam_config(b, fs_cfg)
        for q in (range(self.n_filters) if b is None else [b]):
            self.fs_configs[q] = fs_cfg

    def set_motion(self, b, var, geom, seed):
        """Filter b's (None: every filter's) input-noise variances (speed, steering), vehicle geometry (h, l, dx, dy) and Philox key."""
        self.batch_vp_set_motion(b, var, geom, seed)

    def propagate_run_async(self, u, dt, call0, noisy=None):
        """A run of odometry messages for every slot of every block in one launch, behind the cycles in flight."""
        self.batch_vp_propagate_run_async(u, dt, call0, noisy=noisy)

    def cycle_async(self, predict, Zs, u01, poses=None, pose_cov=None, scan=None):
        """One whole FastSLAM::update of every filter, enqueued; nothing is read back.  u01 [n_filters]: the draws a resampling would use."""
        self.batch_vp_fastslam_mh_cycle_async(predict, Zs, u01, poses=poses, pose_cov=pose_cov, scan=scan)

    def last_cycle(self):
        """What the last cycle did, per filter (synchronises): see CBatchMH.batch_fastslam_last_cycle."""
        return self.batch_fastslam_last_cycle()

    def live_counts(self):
        """The live particle count of every filter (synchronises)."""
        return self.batch_live_counts()
