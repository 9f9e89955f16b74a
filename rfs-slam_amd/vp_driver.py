"""Event-driven Victoria Park host loop over a filter handle (device engine in production).

Mirrors the reference driver's run() (src/rbphdslam_VictoriaPark.cpp:471-628): `Input` messages -> predict only;
`Lidar` messages -> predict, optional artificial clutter (:555-580), setLaserScan (:582), update (:583); the Ackerman
motion model (src/ProcessModel_Ackerman2D.cpp:47-78) and the input-noise sampling stay on the host like every RNG-bound
piece of the reference; resampling follows ParticleFilter::resample through engine.systematic_resample_plan.
The dataset's raw LASER.txt is missing from the reference, so the scan is the synthetic constant-70 m one.

FastSLAM options (filter="fastslam"):
  max_hypotheses     MH-FastSLAM: an update multiplies particles; `n` is the live count, `n_init` the configured one, and a grown
                     count above n_particles_max forces the resampling back to n_init (FastSLAM::resampleWithMapCopy).  On the
                     host-stop route host poses follow particle_parents() and then the resampling plan.
  device_motion      the poses live on the device: Ackerman propagation under `motion_seed` (csrc/motion.h), every run of messages
                     up to a lidar message as one propagate_ackerman_run_async + one static_steps_async.
  device_cycle       every lidar message is one rfsgpu_fastslam_cycle_full_async that carries the scan (implies device_motion);
                     nothing is read until the end of the run, or until sync().  sync_every_update reads each cycle's results.
  draw_every_update  one resampling draw per lidar update with measurements, used or not, so that the host-stop route and the
                     device cycle (which needs the draw before the decision exists) share a realisation.

The RB-PHD filter (filter="rbphd") takes device_motion, device_cycle, draw_every_update and sync_every_update in the same sense:
  device_motion      per run of messages the first predict with its births (predict_map_async, at the poses from before the run's
                     propagation), the rest as one static_steps_async, then one propagate_ackerman_run_async.
  device_cycle       every lidar message is one rfsgpu_rbphd_cycle_async that carries the scan: the two counters, the gate and the
                     resampling are the device's, and the birth predict behind it walks the inheritance levels there.
Logging (either filter, every route):
  log_estimates      the reference's particlePose.dat / landmarkEst.dat content is kept on the device (rfsgpu.h [estimate], switched on
                     for the handle by rfsgpu_handle_serve_estimates): one row taken before the loop at the first message's time (the
                     reference's initial block of poses), then one row behind every lidar update with the message's time.  On the
                     device-cycle route the rows go behind the pending cycles and nothing is read; estimates() is the one read at the
                     end and write_vp_logs prints the two files from it.  log_particles: keep the particle set (particlePose.dat);
                     log_w_threshold: the least weight of a logged Gaussian (-inf: every one, what landmarkEst.dat holds).
N_eff: the host-stop route takes 1 / np.sum(w * w); the device adds the squares in slot order with one fused multiply-add per
particle (csrc/resample_plan.h).  The two agree to rounding, so a run whose N_eff comes within an ulp or so of a threshold could
decide differently on the two routes; the runs the tests compare do not.
"""
import numpy as np

from .engine import systematic_resample_plan

ACKERMAN = dict(h=0.76, l=2.83, dx=3.78, dy=0.50)   # cfg/rbphdslam_VictoriaPark*.xml <AckermanModel>
VP_BATCH_RUN_MAX = 16                                # RFSGPU_BATCH_VP_RUN_MAX (include/rfsgpu.h): steps of one propagate_run_async


def philox_resample_draw(seed, call):
    """The resampling draw a batch's device route takes for (filter key, call): 53 bits of Philox4x32-10 block (0, 2, call low word,
    call high word) under the key, over 2^53 -- in [0, 1) (csrc/batch_loop.h, batch_resample_draw)."""
    m = 0xFFFFFFFF
    c = [0, 2, int(call) & m, (int(call) >> 32) & m]
    k0, k1 = int(seed) & m, (int(seed) >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & m, (p0 >> 32) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return float(((c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0)


def ackerman_step(x, u_v, u_r, dt, a=ACKERMAN):
    """MotionModel_Ackerman2d::step, vectorised over particles (x: [N,3], u_v/u_r: [N])."""
    r = x[:, 2]
    c, s, t = np.cos(r), np.sin(r), np.tan(u_r)
    v = u_v / (1 - t * a["h"] / a["l"])
    out = x.copy()
    out[:, 0] += dt * (v * c - v / a["l"] * t * (a["dx"] * s + a["dy"] * c))
    out[:, 1] += dt * (v * s + v / a["l"] * t * (a["dx"] * c - a["dy"] * s))
    out[:, 2] += dt * v / a["l"] * t
    th = out[:, 2]
    out[:, 2] = np.where(th > np.pi, th - 2 * np.pi, np.where(th < -np.pi, th + 2 * np.pi, th))
    return out


class VictoriaParkRun:
    def __init__(self, f, data, params, seed=1, var_uv=0.2, var_ur=0.025, noise_inflation=20.0, added_clutter=3.0, eff_n=None,
                 filter="rbphd", device_resample=False, max_hypotheses=1, n_particles_max=None, device_cycle=False, draw_every_update=False,
                 device_motion=False, motion_seed=1, sync_every_update=False, log_estimates=False, log_particles=True,
                 log_w_threshold=-np.inf):
        # device_resample: the resample-or-normalise tail of an update as one rfsgpu_resample_async (same realisation and results)
        # filter = "rbphd": src/rbphdslam_VictoriaPark.cpp; "fastslam": src/fastslam_VictoriaPark.cpp (same event loop around
        # FastSLAM::predict / update: no births in predict, rfsgpu_fastslam_update)
        self.f, self.P = f, params
        self.fastslam = filter == "fastslam"
        self.device_resample = bool(device_resample)
        self.mgr, self.inputs, self.meas = data["manager"], data["inputs"], data["measurements"]
        self.rng = np.random.default_rng(seed)
        self.n = f.n
        self.x = np.zeros((self.n, 3))
        self.var = np.array([var_uv, var_ur]) * noise_inflation
        self.added_clutter = added_clutter
        self.eff_n = eff_n if eff_n is not None else self.n / 2.0
        self.scan = np.full(361, 70.0)
        self.n_updates_since = 0
        self.n_meas_since = 0
        self.n_resamples = 0
        self.n_lidar = 0
        self.n_gate_closed = 0            # RB-PHD host-stop route: updates with measurements that found a gate closed
        self.n_init = self.n
        self.hyp = int(max_hypotheses)
        self.n_max = int(n_particles_max) if n_particles_max is not None else (3 * self.n if self.hyp > 1 else self.n)
        self.device_cycle = bool(device_cycle)
        self.device_motion = bool(device_motion) or self.device_cycle
        self.draw_every_update = bool(draw_every_update) or self.device_cycle
        self.sync_every_update = bool(sync_every_update)
        self.motion_seed, self.n_calls = int(motion_seed), 0
        self.n_grown_max, self.n_forced = self.n, 0
        self._run = []                    # (u, var, dt) of the predicts not yet enqueued (device_motion)
        if self.hyp > 1 and not self.fastslam:
            raise ValueError("max_hypotheses belongs to filter='fastslam'")
        if self.fastslam and (self.hyp > 1 or self.device_cycle):
            cfg = f.get_fastslam_config()
            cfg.maxNDataAssocHypotheses = self.hyp
            cfg.nParticlesMax = self.n_max
            cfg.minUpdatesBeforeResample = int(params["min_updates"])
            cfg.minMeasurementsBeforeResample = int(params["min_measurements"])
            f.set_fastslam_config(cfg)
        if self.device_cycle and not self.fastslam:
            cfg = f.get_filter_config()
            cfg.minUpdatesBeforeResample = int(params["min_updates"])
            cfg.minMeasurementsBeforeResample = int(params["min_measurements"])
            f.set_filter_config(cfg)
            if hasattr(f, "config"):
                f.config = cfg
            f.rbphd_set_resampling(self.eff_n, self.eff_n / self.n_init)
        elif self.device_cycle:
            f.fastslam_set_resampling(self.eff_n, self.eff_n / self.n_init)
        if self.device_motion:
            f.set_poses(self.x, None)
        self.log_estimates, self.log_particles, self.log_w_threshold = bool(log_estimates), bool(log_particles), float(log_w_threshold)
        if self.log_estimates:
            f.handle_serve_estimates(True)

    def _log_row(self, t):
        """One row of the estimate log behind whatever is enqueued (a pending device cycle stays pending)."""
        if self.log_estimates:
            self.f.step_estimate_async(t, self.log_w_threshold)

    def estimates(self):
        """(hdr, gauss, part) of the run's rows, as estimate_log_read returns them: the one read at the end."""
        return self.f.estimate_log_read()

    def _predict(self, u, dt, stationary, birth):
        f = self.f
        if self.device_motion:            # queued: the run goes to the device at the next lidar message (or at sync())
            self._run.append((float(u[0]), float(u[1]), 0.0 if stationary else self.var[0], 0.0 if stationary else self.var[1], float(dt),
                              1.0 if (birth and not self.fastslam) else 0.0))
            return
        f.set_lmk_process_noise(np.diag([5e-4, 5e-4, 1e-4]) * dt * dt)   # varlm* x dt^2 (:497-500)
        f.set_poses(self.x, None)                                          # poses BEFORE propagation: birth uses them
        f.predict_map(False if self.fastslam else birth)
        if stationary:
            uv = np.full(self.n, u[0]); ur = np.full(self.n, u[1])
        else:                                                              # predict(u, dt, false, true): noise from the input
            uv = u[0] + np.sqrt(self.var[0]) * self.rng.standard_normal(self.n)
            ur = u[1] + np.sqrt(self.var[1]) * self.rng.standard_normal(self.n)
        self.x = ackerman_step(self.x, uv, ur, dt)

    def _flush_run(self):
        """The queued predicts as one propagation run and one run of static steps (same bits as one call per message)."""
        if not self._run:
            return
        r = np.array(self._run, dtype=np.float64)
        self._run = []
        a = ACKERMAN
        q = np.diag([5e-4, 5e-4, 1e-4])[None, :, :] * (r[:, 4] ** 2)[:, None, None]      # varlm* x dt^2 (:497-500)
        if r[0, 5] != 0.0:                # RB-PHD: the run's first predict adds the births, at the poses the last update used
            self.f.set_lmk_process_noise(q[0])
            self.f.predict_map_async(True)
            if len(r) > 1:
                self.f.static_steps_async(len(r) - 1, q[1:])
        else:
            self.f.static_steps_async(len(r), q)
        self.f.propagate_ackerman_run_async(r[:, 0:2], r[:, 2:4], r[:, 4], (a["h"], a["l"], a["dx"], a["dy"]), self.motion_seed, self.n_calls)
        self.n_calls += len(r)

    def sync(self):
        """Bring the host's view up to date on the device-cycle route (synchronises): the live count and the number of resamplings."""
        self._flush_run()
        self.f.synchronize()
        self.n = self.f.n
        if self.device_cycle and not self.fastslam:
            self.n_resamples = self.f.rbphd_cycle_counts()["n_resamplings"]
        elif self.device_cycle and self.n_lidar:
            self.n_resamples = self.f.fastslam_cycle_counts()[1]
        return self

    def _update_fastslam(self, Z):
        """FastSLAM::update's tail for one lidar message with measurements: the update, then resampleWithMapCopy."""
        f, P = self.f, self.P
        u01 = float(self.rng.uniform()) if self.draw_every_update else None
        draw = (lambda: u01) if self.draw_every_update else (lambda: float(self.rng.uniform()))
        if self.device_cycle:
            f.fastslam_cycle_full_async(Z, u01, self.n_init, predict=False, scan=self.scan)
            if self.sync_every_update:
                lc = f.fastslam_last_cycle()
                self.n_grown_max = max(self.n_grown_max, lc["n_after_update"])
                self.n = lc["n_after_resample"]
            return
        f.fastslam_update(Z)
        if self.hyp > 1:
            par = f.particle_parents()
            if not self.device_motion:
                self.x = self.x[par]
            self.n = f.n
            self.n_grown_max = max(self.n_grown_max, self.n)
        fired, forced = False, self.n > self.n_max
        if forced or (self.n_updates_since >= P["min_updates"] and self.n_meas_since >= P["min_measurements"]):
            fired = self._resample(draw, force=forced)
            self.n_forced += int(forced and fired)
        if self.hyp > 1:
            f.fastslam_set_resample_occured(fired)
        if fired:
            self.n_updates_since = self.n_meas_since = 0
        else:
            s = f.weight_sums()
            f.normalize_weights(s[0])

    def run(self, n_messages=None):
        f, P = self.f, self.P
        t_km, u_km, stationary, birth, z_idx = 0.0, np.zeros(2), True, True, 0
        msgs = self.mgr if n_messages is None else self.mgr[:n_messages]
        if self.log_estimates:            # a row before the loop and one per lidar message, counted here
            f.estimate_log_create(1 + int(sum(1 for m in msgs if m[1] == 3)), f.gm_capacity, self.log_particles)
            if not self.device_motion:
                f.set_poses(self.x, None)
            if len(msgs):
                self._log_row(float(msgs[0][0]))
        for t_k, typ, idx in msgs:
            idx = int(idx) - 1
            dt = t_k - t_km
            if typ == 2:          # Input
                self._predict(u_km, dt, stationary, birth)
                birth = False
                u_km = self.inputs[idx, 1:3].copy()
                if u_km[0] != 0:
                    stationary = False
                t_km = t_k
            elif typ == 3:        # Lidar
                self._predict(u_km, dt, stationary, birth)
                birth = False
                Z = []
                while z_idx < len(self.meas) and abs(self.meas[z_idx, 0] - t_k) < 1e-9:
                    Z.append(self.meas[z_idx, 1:4])
                    z_idx += 1
                if self.added_clutter > 0:
                    for _ in range(self.rng.poisson(self.added_clutter)):
                        r = self.rng.uniform() * (P["rmax"] - P["rmin"]) + P["rmin"]
                        b = self.rng.uniform() * ((np.rad2deg(P["bmax"]) - np.rad2deg(P["bmin"])) + np.rad2deg(P["bmin"])) * np.pi / 180  # sic (:563)
                        Z.append(np.array([r, b, 1.0]))
                Z = np.array(Z).reshape(-1, 3)[:60]
                self._flush_run()
                if self.device_cycle and not self.fastslam:     # one call per lidar message: counters, scan, step, gate, tail
                    u01 = float(self.rng.uniform()) if len(Z) else 0.0
                    f.rbphd_cycle_async(Z, u01, scan=self.scan)
                    self.n_lidar += 1 if len(Z) else 0
                    if self.sync_every_update and len(Z):
                        f.rbphd_last_cycle()
                    self._log_row(t_k)
                    birth = True
                    t_km = t_k
                    continue
                if self.device_cycle:
                    if not len(Z):        # an update without measurements is only counted (FastSLAM.hpp:399-402)
                        f.fastslam_cycle_full_async(Z, 0.0, self.n_init, predict=False, scan=self.scan)
                else:
                    f.set_laser_scan(self.scan)
                    if not self.device_motion:
                        f.set_poses(self.x, None)
                self.n_updates_since += 1
                if len(Z) and self.fastslam and (self.device_cycle or self.hyp > 1 or self.draw_every_update or self.device_motion):
                    self.n_meas_since += len(Z)
                    self.n_lidar += 1
                    self._update_fastslam(Z)
                elif len(Z):
                    self.n_meas_since += len(Z)
                    if self.fastslam:
                        f.fastslam_update(Z)
                    else:
                        f.update(Z)
                    self.n_lidar += 1
                    fired, tail_done = False, False
                    draw = None
                    if self.draw_every_update:        # taken whether or not it is used: the device cycle's realisation
                        u01 = float(self.rng.uniform())
                        draw = lambda: u01
                    if self.n_updates_since >= P["min_updates"] and self.n_meas_since >= P["min_measurements"]:
                        fired = self._resample_device(draw) if self.device_resample else self._resample(draw)
                        tail_done = self.device_resample
                    else:
                        self.n_gate_closed += 1
                    if fired:
                        self.n_updates_since = self.n_meas_since = 0
                    elif not tail_done:
                        s = f.weight_sums()
                        f.normalize_weights(s[0])
                self._log_row(t_k)
                birth = True
                t_km = t_k
        if self.device_motion:
            self.sync()
        return self

    def _resample_device(self, draw=None):
        # the draw is looked at before the decision is known and taken from the stream only when the resampling fired; with
        # draw_every_update it is this update's own draw, already taken
        f = self.f
        if draw is None:
            state = self.rng.bit_generator.state
            u01 = float(self.rng.uniform())
            self.rng.bit_generator.state = state
        else:
            u01 = draw()
        f.resample_async(self.eff_n, self.eff_n / self.n, u01, 0, False, True)
        lr = f.last_resample()
        if not lr["fired"]:
            return False
        if draw is None:
            self.rng.uniform()
        self.x = self.x[lr["plan"]]
        self.n_resamples += 1
        return True

    def _resample(self, draw=None, force=False):
        """ParticleFilter::resample(n_init, force): draw() gives the uniform of the systematic plan (default: the run's stream)."""
        f = self.f
        s = f.weight_sums()
        f.normalize_weights(s[0])
        w = f.get_weights()
        if not force:
            neff = 1.0 / float(np.sum(w * w))
            if neff > self.eff_n and neff / self.n > self.eff_n / self.n_init:
                return False
        u01 = float(self.rng.uniform()) if draw is None else draw()
        if self.n > self.n_init:          # a grown set comes back to its initial count
            plan = systematic_resample_plan(w, u01, n_out=self.n_init)
            f.resample_apply(plan, n_out=self.n_init)
            self.n = self.n_init
        else:
            plan = systematic_resample_plan(w, u01)
            f.resample_apply(plan)
        if not self.device_motion:
            self.x = self.x[plan]
        self.n_resamples += 1
        return True


class VictoriaParkBatchRun:
    """VictoriaParkRun's loop (the RB-PHD filter on the host-stop route) for B filters in lock-step over one dataset: the sweep of
    cfg/rbphdslam_VictoriaPark_artificialClutter.xml -- the same messages under different input-noise, clutter and resampling
    realisations and different parameter sets.  target: a VPFilterBatch, or a list of B plain Victoria Park handles, which then take
    the same realisations in turn (the comparison route of the tests and of tools/vp_bench.py).

    Every filter has its own generator (seeds[b]) for its input noise, artificial clutter and resampling draws, taken in
    VictoriaParkRun's order; the Ackerman propagation is one vectorised step over all slots on the host.  The device work of a run of
    messages is issued at its lidar message: the run's first predict with its births (at the poses the last update used; a cycle call
    without measurement sets, or predict_map_async on a handle), the other predicts as one static_steps_async, then one cycle call with
    the sets, the new poses and the scan; a lidar message that follows another directly is one cycle call.  Then each filter's gate and
    N_eff decision on the host and one resample_apply for the filters that fire.  keep_history: (n_z, fired, plans) per lidar message.
    One difference from VictoriaParkRun, on both routes alike: the cycle call's normalize flag is the whole batch's, so a filter whose
    set is empty at a lidar message has its (already normalised) weights divided by their sum once more, where VictoriaParkRun leaves
    them alone (RBPHDFilter.hpp:451-452); the batch is held to the handles stepped through this class, not to VictoriaParkRun.

    filter="fastslam": the loop of VictoriaParkRun(filter="fastslam") per filter -- the FastSLAM half of the sweep
    (cfg/fastslam_VictoriaPark_artificialClutter.xml).  target: a VPFastSLAMBatch, or a list of Victoria Park FastSLAM handles.  No
    births: every predict of a run is a static step with the dt^2-scaled landmark noise (one static_steps_async), the update cycle
    runs with predict = None.  A filter whose set is empty is only counted (FastSLAM.hpp:399-402), on both kinds of target.  The
    gates are params_per_filter's min_updates / min_measurements, which the constructor writes into a batch's FastSLAM
    configurations; both resampling routes move the landmark candidate lists with the particle.  Not with log_estimates.

    filter="mhfastslam": the multi-hypothesis third of the sweep (cfg/mhfastslam_VictoriaPark_artificialClutter.xml), on the device route
    only (device_loop=False and log_estimates=True raise ValueError).  target: a VPMHFastSLAMBatch, or a list of Victoria Park FastSLAM
    handles created with max_particles and device_cycle=True, which take the same realisations through fastslam_cycle_full_async.  Per
    run of messages: static_steps_async, the run propagation, then one cycle (predict off, poses=None, the scan) whose resampling is
    inside it.  Per filter and lidar message with measurements one u01 is drawn from rngs[b], behind that message's clutter draws, on
    both kinds of target -- VictoriaParkRun's draw_every_update -- so the streams stay aligned.  The gates are params_per_filter's
    min_updates / min_measurements and the N_eff thresholds eff_n, which the constructor writes into the batch or the handles.
    Nothing is read until synchronize(); keep_history reads batch_fastslam_last_cycle (fastslam_last_cycle per handle) per lidar
    message: (n_z, fired, plans in slots of the filter), and grown gets the counts after that message's update.

    device_loop: the run is enqueued and nothing is read until synchronize().  The artificial clutter and the measurement sets are
    still drawn on the host from seeds[b] (they depend on no device state); the poses live on the device.  Per run of messages a
    batch gets the birth cycle (no sets, at the poses the last update used), static_steps_async, one propagate_run_async (noisy = not
    stationary, calls numbered by message index), the update cycle with poses=None and resample_async(n_z, call = lidar index): the
    gates, N_eff, plan, ids and the next birth predict's inheritance walk are the device's.  keep_history reads last_resample per lidar
    message, which synchronises there.  A list of handles takes the same realisations: propagate_ackerman_run_async under the same key
    and the same calls, and the host-side decision with the draw the device would take (philox_resample_draw) and the squares added in
    slot order.  The noise and resampling realisations are Philox's under seeds[b], not numpy's: the same model, another generator
    (as for the 2-D batch loop), so a device_loop run is compared with a device_loop run.  The normalise-flag difference above stays.

    log_estimates: VictoriaParkRun's log for every filter, on both routes and both kinds of target -- one row before the loop at the
    first message's time (the poses set on the device), then one row per lidar message behind that message's resampling step.  A batch
    goes through rfsgpu_batch_vp_serve_estimates with the time repeated per filter, a list of handles through handle_serve_estimates
    per handle.  run() creates the log (1 + number of lidar messages rows, log_max_est Gaussians per row: None = gm_capacity); with
    device_loop the rows go behind the enqueued work and nothing is read; estimates() is the one read."""

    def __init__(self, target, data, params_per_filter, seeds, var_uv=0.2, var_ur=0.025, noise_inflation=20.0, added_clutter=3.0, eff_n=None,
                 keep_history=False, device_loop=False, log_estimates=False, log_particles=True, log_w_threshold=-np.inf, log_max_est=None,
                 filter="rbphd"):
        if filter not in ("rbphd", "fastslam", "mhfastslam"):
            raise ValueError("filter is 'rbphd', 'fastslam' or 'mhfastslam'")
        self.fastslam = filter == "fastslam"
        self.mh = filter == "mhfastslam"
        if self.mh and not device_loop:
            raise ValueError("a batch of Victoria Park multi-hypothesis FastSLAM filters runs on the device route only (device_loop=True)")
        if self.mh and log_estimates:
            raise ValueError("the estimate log does not serve a batch of Victoria Park multi-hypothesis FastSLAM filters")
        if self.fastslam and log_estimates:
            raise ValueError("the estimate log does not serve a batch of Victoria Park FastSLAM filters")
        self.batch = None if isinstance(target, (list, tuple)) else target
        self.handles = list(target) if self.batch is None else None
        self.nF = len(params_per_filter)
        self.n = self.batch.n_per_filter if self.batch is not None else self.handles[0].n
        assert len(seeds) == self.nF and (self.batch.n_filters if self.batch is not None else len(self.handles)) == self.nF
        self.Ps = list(params_per_filter)
        self.mgr, self.inputs, self.meas = data["manager"], data["inputs"], data["measurements"]
        self.rngs = [np.random.default_rng(s) for s in seeds]
        self.x = np.zeros(((self.batch.n if self.mh and self.batch is not None else self.nF * self.n), 3))     # (mh: every slot of every block)
        self.sd = np.sqrt(np.array([var_uv, var_ur]) * noise_inflation)
        self.added_clutter = np.broadcast_to(np.asarray(added_clutter, dtype=np.float64), (self.nF,)).copy()
        self.eff_n = np.broadcast_to(np.asarray(self.n / 2.0 if eff_n is None else eff_n, dtype=np.float64), (self.nF,)).copy()
        self.scan = np.full(361, 70.0)
        if self.batch is not None:
            self.batch.set_laser_scan(self.scan)      # (a cycle call needs one, the run's first birth predict included)
        self.n_updates_since = np.zeros(self.nF, dtype=np.int64)
        self.n_meas_since = np.zeros(self.nF, dtype=np.int64)
        self.n_resamples = np.zeros(self.nF, dtype=np.int64)
        self.n_lidar = 0
        self.history = [] if keep_history else None
        self.grown = []                   # mhfastslam with keep_history: every filter's count after each lidar message's update
        self._dts = []                    # the intervals of the predicts not yet issued (the first of a run adds the births)
        self.device_loop = bool(device_loop)
        if self.fastslam and self.batch is not None:      # the batch's gates (update_and_resample, resample_async) are its FastSLAM configurations'
            for b in range(self.nF):
                cfg = self.batch.fs_configs[b]
                cfg.minUpdatesBeforeResample = int(self.Ps[b]["min_updates"])
                cfg.minMeasurementsBeforeResample = int(self.Ps[b]["min_measurements"])
                self.batch.configure_fastslam(b, cfg)
        if self.mh:                       # the gates and N_eff thresholds of the resampling inside the cycle
            for b in range(self.nF):
                cfg = self.batch.fs_configs[b] if self.batch is not None else self.handles[b].fs_config
                cfg.minUpdatesBeforeResample = int(self.Ps[b]["min_updates"])
                cfg.minMeasurementsBeforeResample = int(self.Ps[b]["min_measurements"])
                if self.batch is not None:
                    self.batch.configure_fastslam(b, cfg)
                else:
                    f = self.handles[b]
                    f.set_fastslam_config(cfg)
                    f.effNParticles_t, f.effNParticles_t_percent = float(self.eff_n[b]), float(self.eff_n[b] / self.n)
        self.seeds = [int(s) for s in seeds]
        self.var = np.array([var_uv, var_ur]) * noise_inflation
        self._run = []                    # device_loop: (uv, ur, noisy) of the predicts not yet issued
        self._n_calls = 0                 # ... and the message index of the first of them: the propagation's call number
        if self.device_loop:
            a = ACKERMAN
            self._geom = (a["h"], a["l"], a["dx"], a["dy"])
            if self.batch is not None:
                for b in range(self.nF):
                    self.batch.set_motion(b, self.var, self._geom, self.seeds[b])
                    self.batch.set_resampling(b, self.eff_n[b], self.eff_n[b] / self.n)
                self.batch.set_poses(self.x, None)
            else:
                for b, f in enumerate(self.handles):
                    f.set_poses(self.x[self._block(b)] if not self.mh else np.zeros((f.n, 3)), None)
        self.log_estimates, self.log_particles, self.log_w_threshold = bool(log_estimates), bool(log_particles), float(log_w_threshold)
        self.log_max_est = None if log_max_est is None else int(log_max_est)
        if self.log_estimates:
            if self.batch is not None:
                self.batch.serve_estimates(True)
            else:
                for f in self.handles:
                    f.handle_serve_estimates(True)

    def _targets(self):
        return [self.batch] if self.batch is not None else self.handles

    def _log_row(self, t):
        """One row of every filter's estimate log behind whatever is enqueued (a batch: the time repeated per filter)."""
        if self.log_estimates:
            for f in self._targets():
                f.step_estimate_async(float(t), self.log_w_threshold)

    def estimates(self):
        """(hdr, gauss, part) with the filter axis ([rows, n_filters, ...]): the one read at the end.  A batch's best_slot is a global
        slot; a list of handles is stacked onto the same axes with best_slot as each handle reports it (a slot of its own)."""
        if self.batch is not None:
            return self.batch.estimate_log_read()
        logs = [f.estimate_log_read() for f in self.handles]
        part = None if logs[0][2] is None else np.concatenate([l[2] for l in logs], axis=1)
        return np.concatenate([l[0] for l in logs], axis=1), np.concatenate([l[1] for l in logs], axis=1), part

    def _block(self, b):
        return slice(b * self.n, (b + 1) * self.n)

    def _predict(self, u, dt, stationary):
        self._dts.append(float(dt))
        if self.device_loop:              # queued: the run goes to the device at the next lidar message
            self._run.append((float(u[0]), float(u[1]), 0.0 if stationary else 1.0))
            return
        N = self.nF * self.n
        if stationary:
            uv, ur = np.full(N, u[0]), np.full(N, u[1])
        else:                             # predict(u, dt, false, true): each filter's noise from its own generator, uv then ur
            uv, ur = np.empty(N), np.empty(N)
            for b, rng in enumerate(self.rngs):
                uv[self._block(b)] = u[0] + self.sd[0] * rng.standard_normal(self.n)
                ur[self._block(b)] = u[1] + self.sd[1] * rng.standard_normal(self.n)
        self.x = ackerman_step(self.x, uv, ur, dt)

    def _clutter(self, b):
        P, rng, out = self.Ps[b], self.rngs[b], []
        if self.added_clutter[b] > 0:
            for _ in range(rng.poisson(self.added_clutter[b])):
                r = rng.uniform() * (P["rmax"] - P["rmin"]) + P["rmin"]
                a = rng.uniform() * ((np.rad2deg(P["bmax"]) - np.rad2deg(P["bmin"])) + np.rad2deg(P["bmin"])) * np.pi / 180  # sic (:563)
                out.append(np.array([r, a, 1.0]))
        return out

    def _cycle(self, Zs):
        """The queued predicts and this lidar message's update on the device."""
        q = np.diag([5e-4, 5e-4, 1e-4])[None, :, :] * (np.array(self._dts) ** 2)[:, None, None]      # varlm* x dt^2 (:497-500)
        dts = np.array(self._dts, dtype=np.float64)
        self._dts = []
        if self.device_loop:
            return self._cycle_device(q, dts, Zs)
        if self.fastslam:
            for f in self._targets():
                f.static_steps_async(len(q), q)
            if Zs is not None:
                self._update_fastslam(Zs, self.x)
            return
        one = len(q) == 1 and Zs is not None      # (Zs None: the predicts behind the last lidar message, no update)
        if self.batch is not None:
            f = self.batch
            f.set_lmk_process_noise(q[0])
            if not one:
                f.cycle_async(True, [np.zeros((0, 3))] * self.nF, normalize=False)
                if len(q) > 1:
                    f.static_steps_async(len(q) - 1, q[1:])
            if Zs is not None:
                f.cycle_async(True if one else None, Zs, poses=self.x, scan=self.scan, normalize=True)
            return
        for b, f in enumerate(self.handles):
            f.set_lmk_process_noise(q[0])
            if not one:
                f.predict_map_async(True)
                if len(q) > 1:
                    f.static_steps_async(len(q) - 1, q[1:])
            if Zs is not None:
                f.set_step_inputs_async(scan=self.scan)      # (through the pinned ring: no stop behind the predicts just enqueued)
                f.cycle_async(True if one else None, Zs[b], poses=self.x[self._block(b)], normalize=True)

    def _cycle_device(self, q, dts, Zs):
        """device_loop: the queued predicts and this lidar message's update, with the propagation between the births (which see the
        poses of the last update) and the update.  Nothing is read."""
        r = np.array(self._run, dtype=np.float64).reshape(-1, 3)
        self._run = []
        call0 = self._n_calls
        self._n_calls += len(r)
        if self.fastslam or self.mh:
            var = r[:, 2:3] * self.var[None, :]
            for b, f in enumerate(self._targets()):
                f.static_steps_async(len(q), q)
                if self.batch is None:
                    f.propagate_ackerman_run_async(r[:, 0:2], var, dts, self._geom, self.seeds[b], call0)
                    continue
                for k0 in range(0, len(r), VP_BATCH_RUN_MAX):
                    k1 = min(len(r), k0 + VP_BATCH_RUN_MAX)
                    f.propagate_run_async(r[k0:k1, 0:2], dts[k0:k1], call0 + k0, noisy=r[k0:k1, 2] != 0)
            if Zs is not None and self.mh:
                u01 = np.array([float(self.rngs[b].uniform()) if len(Zs[b]) else 0.5 for b in range(self.nF)])
                if self.batch is not None:
                    self.batch.cycle_async(False, Zs, u01, poses=None, scan=self.scan)
                else:
                    for b, f in enumerate(self.handles):
                        f.cycle_async(Zs[b], u01[b], predict=False, scan=self.scan, push_config=self.n_lidar == 0)
            elif Zs is not None:
                self._update_fastslam(Zs, None)
            return
        if self.batch is not None:
            f = self.batch
            f.set_lmk_process_noise(q[0])
            f.cycle_async(True, [np.zeros((0, 3))] * self.nF, normalize=False)
            if len(q) > 1:
                f.static_steps_async(len(q) - 1, q[1:])
            for k0 in range(0, len(r), VP_BATCH_RUN_MAX):
                k1 = min(len(r), k0 + VP_BATCH_RUN_MAX)
                f.propagate_run_async(r[k0:k1, 0:2], dts[k0:k1], call0 + k0, noisy=r[k0:k1, 2] != 0)
            if Zs is not None:
                f.cycle_async(None, Zs, poses=None, scan=self.scan, normalize=True)
            return
        var = r[:, 2:3] * self.var[None, :]
        for b, f in enumerate(self.handles):
            f.set_lmk_process_noise(q[0])
            f.predict_map_async(True)
            if len(q) > 1:
                f.static_steps_async(len(q) - 1, q[1:])
            f.propagate_ackerman_run_async(r[:, 0:2], var, dts, self._geom, self.seeds[b], call0)
            if Zs is not None:
                f.set_step_inputs_async(scan=self.scan)
                f.cycle_async(None, Zs[b], poses=None, normalize=True)

    def _update_fastslam(self, Zs, x):
        """This lidar message's FastSLAM update of every filter (x None: the poses are the device's) and the normalisation of the
        filters that had measurements: one batch cycle, or rfsgpu_fastslam_update and the division per handle."""
        if self.batch is not None:
            self.batch.cycle_async(None, Zs, poses=x, scan=self.scan, normalize=True)
            return
        for b, f in enumerate(self.handles):
            if not len(Zs[b]):
                continue
            f.set_laser_scan(self.scan)
            if x is not None:
                f.set_poses(x[self._block(b)], None)
            f.fastslam_update(Zs[b])
            s = f.weight_sums()
            f.normalize_weights(s[0])

    def _resample_device(self, n_z):
        """device_loop: a batch resamples on the device (nothing is read unless the history is kept); the handles' decision is made
        here by the rule the device states -- squares added in slot order, the draw of (seeds[b], lidar index)."""
        call = self.n_lidar - 1
        if self.mh:                       # (the resampling ran inside the cycle; the history is the one read)
            if self.history is None:
                return None, None
            if self.batch is not None:
                lc = self.batch.last_cycle()
                self.grown.append(lc["n_after_update"].copy())
                return lc["fired"].copy(), [lc["plan"][b, :lc["n_after_resample"][b]].copy() for b in range(self.nF)]
            lcs = [f.fastslam_last_cycle() for f in self.handles]
            self.grown.append(np.array([l["n_after_update"] for l in lcs], dtype=np.int32))
            return np.array([l["fired"] for l in lcs]), [l["plan"] for l in lcs]
        if self.batch is not None:
            self.batch.resample_async(n_z, call)
            if self.history is None:
                return None, None
            fired, glob, _ = self.batch.last_resample()
            return fired, [glob[self._block(b)] - b * self.n for b in range(self.nF)]
        fired = np.zeros(self.nF, dtype=bool)
        plans = [np.arange(self.n) for _ in range(self.nF)]
        for b, f in enumerate(self.handles):
            self.n_updates_since[b] += 1
            if n_z[b] == 0:
                continue
            self.n_meas_since[b] += int(n_z[b])
            P = self.Ps[b]
            if self.n_updates_since[b] < P["min_updates"] or self.n_meas_since[b] < P["min_measurements"]:
                continue
            wb = f.get_weights()
            neff = 1.0 / float(np.cumsum(wb * wb)[-1])
            if neff > self.eff_n[b] and neff / self.n > self.eff_n[b] / self.n:
                continue
            plans[b] = systematic_resample_plan(wb, philox_resample_draw(self.seeds[b], call))
            fired[b] = True
            self.n_updates_since[b] = self.n_meas_since[b] = 0
            f.resample_apply(plans[b])
        self.n_resamples += fired
        return fired, plans

    def _resample(self, n_z):
        """RBPHDFilter::update's tail per filter: counters, the two gates, N_eff, the systematic plan with the filter's own draw.  A batch
        makes it itself (update_and_resample, from the configurations it was given: params_per_filter's); the handles' is made here."""
        if self.batch is not None:
            fired, glob = self.batch.update_and_resample(n_z, lambda b: float(self.rngs[b].uniform()), self.eff_n)
            plans = [glob[self._block(b)] - b * self.n for b in range(self.nF)]
            self.n_updates_since[:] = self.batch.nUpdatesSinceResample
            self.n_meas_since[:] = self.batch.nMeasurementsSinceResample
            for b in np.nonzero(fired)[0]:
                self.x[self._block(b)] = self.x[self._block(b)][plans[b]]
            self.n_resamples += fired
            return fired, plans
        w = np.concatenate([f.get_weights() for f in self.handles])
        fired = np.zeros(self.nF, dtype=bool)
        plans = [np.arange(self.n) for _ in range(self.nF)]
        for b in range(self.nF):
            self.n_updates_since[b] += 1
            if n_z[b] == 0:
                continue
            self.n_meas_since[b] += int(n_z[b])
            P = self.Ps[b]
            if self.n_updates_since[b] < P["min_updates"] or self.n_meas_since[b] < P["min_measurements"]:
                continue
            wb = w[self._block(b)]
            neff = 1.0 / float(np.sum(wb * wb))
            if neff > self.eff_n[b] and neff / self.n > self.eff_n[b] / self.n:
                continue
            plans[b] = systematic_resample_plan(wb, float(self.rngs[b].uniform()))
            fired[b] = True
            self.n_updates_since[b] = self.n_meas_since[b] = 0
        for b in np.nonzero(fired)[0]:
            self.handles[b].resample_apply(plans[b])
            self.x[self._block(b)] = self.x[self._block(b)][plans[b]]
        self.n_resamples += fired
        return fired, plans

    def run(self, n_messages=None):
        t_km, u_km, stationary, z_idx = 0.0, np.zeros(2), True, 0
        msgs = self.mgr if n_messages is None else self.mgr[:n_messages]
        if self.log_estimates:            # a row before the loop and one per lidar message, counted here
            rows = 1 + int(sum(1 for m in msgs if m[1] == 3))
            for f in self._targets():
                f.estimate_log_create(rows, f.gm_capacity if self.log_max_est is None else self.log_max_est, self.log_particles)
            if not self.device_loop:      # (device_loop: the constructor has set the poses on the device)
                if self.batch is not None:
                    self.batch.set_poses(self.x, None)
                else:
                    for b, f in enumerate(self.handles):
                        f.set_poses(self.x[self._block(b)], None)
            if len(msgs):
                self._log_row(msgs[0][0])
        for t_k, typ, idx in msgs:
            idx = int(idx) - 1
            dt = t_k - t_km
            if typ == 2:          # Input
                self._predict(u_km, dt, stationary)
                u_km = self.inputs[idx, 1:3].copy()
                if u_km[0] != 0:
                    stationary = False
                t_km = t_k
            elif typ == 3:        # Lidar
                self._predict(u_km, dt, stationary)
                Z = []
                while z_idx < len(self.meas) and abs(self.meas[z_idx, 0] - t_k) < 1e-9:
                    Z.append(self.meas[z_idx, 1:4])
                    z_idx += 1
                Zs = [np.array(Z + self._clutter(b)).reshape(-1, 3)[:60] for b in range(self.nF)]
                n_z = np.array([len(z) for z in Zs])
                self._cycle(Zs)
                self.n_lidar += 1
                fired, plans = self._resample_device(n_z) if self.device_loop else self._resample(n_z)
                if self.history is not None:
                    self.history.append((n_z, fired, plans))
                self._log_row(t_k)
                t_km = t_k
        if self._dts:
            self._cycle(None)
        self.synchronize()
        return self

    def synchronize(self):
        for f in ([self.batch] if self.batch is not None else self.handles):
            f.synchronize()
        if self.device_loop:              # the poses (and a batch's counts) are the device's: the one read at the end
            if self.batch is not None:
                self.x = self.batch.get_poses()
                if not self.mh:
                    self.n_resamples = self.batch.loop_counts()[0]
            else:
                self.x = np.concatenate([f.get_poses() for f in self.handles], 0)


def write_vp_logs(log_dir, estimates, filter=0):
    """particlePose.dat and landmarkEst.dat in the reference's Victoria Park format (std::fixed, precision 3, widths 10 / 5 / 10 ...:
    src/rbphdslam_VictoriaPark.cpp:427-440, :586-622) from (hdr, gauss, part) as VictoriaParkRun.estimates() returns them: per row
    the row's n_particles particles (a log without particles: none), then its n_logged Gaussians under the best slot's index.
    The lines are "%10.3f%5d" + 4 * "%10.3f" (time, particle, x, y, theta, weight) and "%10.3f%5d" + 6 * "%10.3f" (time, best slot,
    the six planes).  filter: which filter of a log with a filter axis (VictoriaParkBatchRun.estimates()); its best slot is printed
    relative to the filter's block of n_particles slots, so a batch's file equals the file of the same filter run as a handle.
    Returns the two paths."""
    import os
    hdr, gauss, part = estimates
    b = int(filter)
    poses, lms = [], []
    for r in range(hdr.shape[0]):
        h = hdr[r, b]
        t = float(h["t"])
        if part is not None:
            p = part[r, b]
            for i in range(int(h["n_particles"])):
                poses.append("%10.3f%5d%10.3f%10.3f%10.3f%10.3f\n" % (t, i, p[0, i], p[1, i], p[2, i], p[3, i]))
        g, best = gauss[r, b], int(h["best_slot"])
        if b:                     # (a global slot of a batch: within the filter's block; a handle's own slot stays what it is)
            best %= max(int(h["n_particles"]), 1)
        for m in range(int(h["n_logged"])):
            lms.append("%10.3f%5d%10.3f%10.3f%10.3f%10.3f%10.3f%10.3f\n" % (t, best, g[0, m], g[1, m], g[2, m], g[3, m], g[4, m], g[5, m]))
    os.makedirs(log_dir, exist_ok=True)
    paths = os.path.join(log_dir, "particlePose.dat"), os.path.join(log_dir, "landmarkEst.dat")
    for path, lines in zip(paths, (poses, lms)):
        with open(path, "w") as fh:
            fh.writelines(lines)
    return paths


def write_vp_batch_logs(root, estimates):
    """write_vp_logs for every filter of (hdr, gauss, part) with a filter axis, into root/filter_%03d/.  Returns the list of path pairs."""
    import os
    return [write_vp_logs(os.path.join(root, "filter_%03d" % b), estimates, filter=b) for b in range(estimates[0].shape[1])]
