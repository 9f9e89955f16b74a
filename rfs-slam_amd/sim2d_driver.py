"""The 2-D simulator's host loop (config C1) over one or MORE filter handles in lock-step.

Mirrors the reference driver `src/rbphdslam2dSim.cpp`: the data generation (`generateTrajectory` :146-206, `generateOdometry`
:209-246, `generateLandmarks` :249-284, `generateMeasurements` :287-366, numpy's generator instead of drand48 / boost: a seed
does not name the same realisation as in the reference) and the filter loop `run()` :540-643 -- `predict` (births at the
pre-propagation pose, host propagation with additive process noise, static landmark step), `setParticlePose` to the ground truth
for k <= 100, the measurements of the time step, `update`, and the resample-or-normalise tail of RBPHDFilter::update
(include/RBPHDFilter.hpp:524-539) with ParticleFilter::resample's N_eff test and systematic plan.

Everything random (process noise, the resampling draw) is drawn ONCE per step by this loop and applied to every handle, and the
particle poses live here, so that the device engine and the CPU oracle can be driven through the same realisation and compared
after every call (tests/test_gpu_parity.py::test_c1_trajectory_device_vs_oracle).  The filters only have to offer the C-ABI
methods of capi.CFilter.
"""
import numpy as np

from . import capi
from .engine import systematic_resample_plan

# values of the shipped cfg/rbphdslam2dSim.xml (tests/golden/rbphdslam2dSim_c1.xml)
C1_SIM = dict(kmax=3000, dt=0.1, n_segments=20, max_dx=0.30, max_dy=0.0, max_dz=0.50, min_dx=0.10, vardx=0.002, vardy=0.002, vardz=0.002,
              n_landmarks=50, varlmx=2e-4, varlmy=2e-4, rmax=2.5, rmin=0.5, rbuf=0.05, Pd=0.99, clutter=1e-4, varzr=5e-4, varzb=5e-5,
              p_noise_inflation=1.5, z_noise_inflation=10.0, birth_w=0.01, kf_range=1.0, kf_bearing=0.2, new_gaussian_md=3.0,
              n_eval=15, min_weight=0.75, weighting_md=3.0, use_cluster=0, eff_n=100.0, min_updates=2, merge_thr=0.5, merge_infl=1.5,
              prune_thr=0.01)

# values of the shipped cfg/fastslam2dSim.xml (tests/golden/fastslam2dSim_c1.xml): the simulator's own keys are those of C1_SIM; the
# FastSLAM filter's: minLogMeasurementLikelihood, maxNDataAssocHypotheses, maxDataAssocLogLikelihoodDiff, the existence prune threshold;
# landmarkExistencePrior is set to 0.5 by the driver (src/fastslam2dSim.cpp:481); pruning_meas_threshold is the constructor default
C1_FASTSLAM_SIM = dict(C1_SIM, min_log_likelihood=-10.0, max_hypotheses=1, max_loglik_diff=3.0, existence_prune_thr=-5.0, existence_prior=0.5,
                       pruning_meas_threshold=0)


def odometry_step(x, u):
    """MotionModel_Odometry2d::step (src/ProcessModel_Odometry2D.cpp:40-90), vectorised: x [N,3] or [3], u [3] or [N,3]."""
    x = np.asarray(x, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    th = x[..., 2]
    ct, st = np.cos(th), np.sin(th)
    out = np.empty(np.broadcast(x, u).shape)
    out[..., 0] = x[..., 0] + (ct * u[..., 0] - st * u[..., 1])       # p_k = p_km + C_km^T dp
    out[..., 1] = x[..., 1] + (st * u[..., 0] + ct * u[..., 1])
    cd, sd = np.cos(u[..., 2]), np.sin(u[..., 2])
    # C_k = C_d C_km with C = [c s; -s c];  theta_k = atan2(C_k(0,1), C_k(0,0))
    out[..., 2] = np.arctan2(cd * st + sd * ct, cd * ct - sd * st)
    return out


def generate(P=C1_SIM, traj_seed=1, kmax=None, measurements=True):
    """gt poses [K,3], odometry [K,3], landmarks [L,2], per-step measurement lists.  measurements=False: the scans are not drawn
    (Z is None) -- for runs whose sensor is the device's (Sim2dBatchRun(device_sensor=True)); the trajectory, landmarks and odometry
    are drawn before the scans from the one generator, so they are the same either way."""
    K = int(kmax or P["kmax"])
    K_full = int(P["kmax"])           # segment / landmark spacing follows the configured length even when fewer steps are run
    dt = P["dt"]
    rng = np.random.default_rng(traj_seed)
    Qd = np.array([P["vardx"], P["vardy"], P["vardz"]])
    gt = np.zeros((K, 3))
    disp = np.zeros((K, 3))
    seg = 0
    u = np.zeros(3)
    for k in range(1, K):
        if k <= 50:
            u = np.zeros(3)
        elif k >= K_full // P["n_segments"] * seg:
            seg += 1
            dx = rng.random() * P["max_dx"] * dt
            while dx < P["min_dx"] * dt:
                dx = rng.random() * P["max_dx"] * dt
            dy = (rng.random() * P["max_dy"] * 2 - P["max_dy"]) * dt
            dz = (rng.random() * P["max_dz"] * 2 - P["max_dz"]) * dt
            u = np.array([dx, dy, dz])
        disp[k] = u
        gt[k] = odometry_step(gt[k - 1], u)
    # landmarks: inverse measurement of a random (r, b) from the pose at regular intervals (:249-284)
    lm = []
    for k in range(1, K_full):
        if k >= K_full // P["n_landmarks"] * len(lm) and k < K:
            r, b = rng.random() * P["rmax"], rng.random() * 2 * np.pi
            x = gt[k]
            lm.append([x[0] + r * np.cos(x[2] + b), x[1] + r * np.sin(x[2] + b)])
    lm = np.array(lm).reshape(-1, 2)
    # odometry = displacement + N(0, Q dt^2) (:209-246)
    odom = np.zeros((K, 3))
    for k in range(1, K):
        odom[k] = disp[k] + np.sqrt(Qd) * dt * rng.standard_normal(3)
    if not measurements:
        return dict(gt=gt, odom=odom, landmarks=lm, Z=None, K=K)
    # measurements (:287-366): noisy range-bearing of the landmarks in range with probability Pd + Poisson clutter
    mean_clutter = P["clutter"] * (2 * np.pi) * (P["rmax"] - P["rmin"])      # MeasurementModel_RngBrg::clutterIntensityIntegral
    sr, sb = np.sqrt(P["varzr"]), np.sqrt(P["varzb"])
    Z = [np.zeros((0, 2))]
    for k in range(1, K):
        x = gt[k]
        zs = []
        for m in range(len(lm)):
            dxm, dym = lm[m, 0] - x[0], lm[m, 1] - x[1]
            r = np.hypot(dxm, dym) + sr * rng.standard_normal()
            b = np.arctan2(dym, dxm) - x[2] + sb * rng.standard_normal()
            b = (b + np.pi) % (2 * np.pi) - np.pi
            if P["rmin"] <= r <= P["rmax"] and rng.random() <= P["Pd"]:
                zs.append([r, b])
        for _ in range(rng.poisson(mean_clutter)):
            r = rng.random() * P["rmax"]
            while r < P["rmin"]:
                r = rng.random() * P["rmax"]
            zs.append([r, rng.random() * 2 * np.pi - np.pi])
        Z.append(np.array(zs, dtype=np.float64).reshape(-1, 2))
    return dict(gt=gt, odom=odom, landmarks=lm, Z=Z, K=K)


def first_seen_times(data, P=C1_SIM):
    """Per ground-truth landmark the time k * dt of the first step k >= 1 whose TRUE range from gt[k] lies in [rmin, rmax], -1 if
    there is none: the third column of the reference's gtLandmark.dat (lmkFirstObsTime_, src/rbphdslam2dSim.cpp:308-339, :404).
    Reads `data` only: no random draw, nothing of generate() changes."""
    gt, lm = data["gt"], data["landmarks"]
    out = np.full(len(lm), -1.0)
    if len(lm) == 0:
        return out
    r = np.hypot(lm[None, :, 0] - gt[1:, None, 0], lm[None, :, 1] - gt[1:, None, 1])     # [K - 1, L]
    ok = (r >= P["rmin"]) & (r <= P["rmax"])
    seen = ok.any(axis=0)
    out[seen] = (np.argmax(ok, axis=0)[seen] + 1) * P["dt"]
    return out


# the reference's evaluation constants (src/analysis2dSim.cpp:182, :232-233): estimate weight threshold, COLA cutoff and order
ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER = 0.75, 0.20, 1.0
# the estimate log's default threshold: every Gaussian of the best particle, as the reference's landmarkEst.dat holds them
ESTIMATE_W_THRESHOLD = -np.inf


def configure(f, P=C1_SIM):
    """setupRBPHDFilter (:444-492) through the C ABI."""
    dt = P["dt"]
    cfg = f.default_filter_config()
    cfg.birthGaussianWeight = P["birth_w"]
    cfg.minUpdatesBeforeResample = P["min_updates"]
    cfg.newGaussianCreateInnovMDThreshold = P["new_gaussian_md"]
    cfg.importanceWeightingMeasurementLikelihoodMDThreshold = P["weighting_md"]
    cfg.importanceWeightingEvalPointCount = P["n_eval"]
    cfg.importanceWeightingEvalPointGuassianWeight = P["min_weight"]
    cfg.gaussianMergingThreshold = P["merge_thr"]
    cfg.gaussianMergingCovarianceInflationFactor = P["merge_infl"]
    cfg.gaussianPruningThreshold = P["prune_thr"]
    cfg.useClusterProcess = P["use_cluster"]
    f.set_filter_config(cfg)
    f.set_model_rngbrg(np.diag([P["varzr"], P["varzb"]]) * P["z_noise_inflation"], P["Pd"], P["clutter"], P["rmax"], P["rmin"], P["rbuf"])
    f.set_kf_config(P["kf_range"], P["kf_bearing"])
    f.set_lmk_process_noise(np.diag([P["varlmx"], P["varlmy"]]) * dt * dt)
    return cfg


def fastslam_config(f, P=C1_FASTSLAM_SIM):
    """The FastSLAM::Config of setupFastSLAMFilter (src/fastslam2dSim.cpp:474-481) as a capi.FastSlamConfig (f: anything with
    default_fastslam_config)."""
    c = f.default_fastslam_config()
    c.minUpdatesBeforeResample = P["min_updates"]
    c.minLogMeasurementLikelihood = P["min_log_likelihood"]
    c.maxNDataAssocHypotheses = P["max_hypotheses"]
    c.maxDataAssocLogLikelihoodDiff = P["max_loglik_diff"]
    c.mapExistencePruneThreshold = P["existence_prune_thr"]
    c.landmarkExistencePrior = P["existence_prior"]
    c.pruningMeasurementsThreshold = P.get("pruning_meas_threshold", 0)
    return c


def configure_fastslam(f, P=C1_FASTSLAM_SIM):
    """setupFastSLAMFilter (src/fastslam2dSim.cpp:438-482) for one handle through the C ABI."""
    dt = P["dt"]
    f.set_model_rngbrg(np.diag([P["varzr"], P["varzb"]]) * P["z_noise_inflation"], P["Pd"], P["clutter"], P["rmax"], P["rmin"], P["rbuf"])
    f.set_kf_config(P["kf_range"], P["kf_bearing"])
    f.set_lmk_process_noise(np.diag([P["varlmx"], P["varlmy"]]) * dt * dt)
    c = fastslam_config(f, P)
    f.set_fastslam_config(c)
    return c


def configure_fastslam_batch_filter(batch, b, P=C1_FASTSLAM_SIM):
    """setupFastSLAMFilter for filter b of a FastSLAMBatch."""
    dt = P["dt"]
    R = np.diag([P["varzr"], P["varzb"]]) * P["z_noise_inflation"]
    batch.configure(b, None, R=R, Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"], kf=(P["kf_range"], P["kf_bearing"]),
                    Q=np.diag([P["varlmx"], P["varlmy"]]) * dt * dt)
    c = fastslam_config(batch, P)
    batch.configure_fastslam(b, c)
    return c


class Sim2dRun:
    """run() :540-643 over `filters` (all driven through the same realisation); `on_step(k, run)` is called after every update."""

    def __init__(self, filters, data, P=C1_SIM, seed=1, eff_n=None, track_errors=False, device_resample=False, track_estimates=False,
                 estimate_threshold=ESTIMATE_W_THRESHOLD, estimate_max=None, log_particles=False):
        """device_resample: the resample-or-normalise tail of an update runs on the device (rfsgpu_resample_async): the host reads the
        decision and the plan (it keeps the poses) instead of the weights; same realisation, same results.
        track_errors: every filter gets the realisation's ground truth and a device-side error log; each cycle ends with one
        stream-ordered step_error_async (after the resampling, where the reference driver logs its particle set); errors() reads
        the logs once.  Off (the default) nothing is enqueued.
        track_estimates: every filter gets a device-side estimate log ([estimate] in include/rfsgpu.h: estimate_max Gaussians per row,
        None: gm_capacity; the particle set too with log_particles); each cycle ends with one stream-ordered
        step_estimate_async(t, estimate_threshold) at the point where the error row is taken; estimates() reads the logs once."""
        self.filters = list(filters)
        self.n = self.filters[0].n
        assert all(f.n == self.n for f in self.filters)
        self.data, self.P = data, P
        self.rng = np.random.default_rng(seed)
        self.x = np.zeros((self.n, 3))
        self.cov = np.zeros((3, 3))          # pose covariance shared by all particles: 0 (ground-truth poses) or Q (after sample())
        self.Q = np.diag([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2
        self.eff_n = float(P["eff_n"] if eff_n is None else eff_n)
        self.cfgs = [configure(f, P) for f in self.filters]
        self.n_updates_since = 0
        self.n_meas_since = 0
        self.n_resamples = 0
        self.n_updates = 0
        self.resample_steps = []
        self.z_of_step = None
        self.track_errors = bool(track_errors)
        self.device_resample = bool(device_resample)
        if self.track_errors:
            fs = first_seen_times(data, P)
            for f in self.filters:
                f.set_ground_truth(data["landmarks"], fs)
                f.error_log_create(int(data["K"]))
        self.track_estimates = bool(track_estimates)
        self.estimate_threshold = float(estimate_threshold)
        if self.track_estimates:
            for f in self.filters:
                f.estimate_log_create(int(data["K"]), f.gm_capacity if estimate_max is None else int(estimate_max), log_particles)

    def _each(self, fn):
        return [fn(f) for f in self.filters]

    def step(self, k):
        fired = self._step(k)
        if self.track_errors:
            t, g = k * self.P["dt"], self.data["gt"][k][None, :]
            self._each(lambda f: f.step_error_async(t, g, ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER))
        if self.track_estimates:
            self._each(lambda f: f.step_estimate_async(k * self.P["dt"], self.estimate_threshold))
        return fired

    def estimates(self):
        """One (hdr [steps, 1], gauss [steps, 1, 6, max_est], part [steps, 1, 4, n] or None) per filter: the estimate rows logged so
        far (capi.CFilter.estimate_log_read; one read each) -- what write_run_logs takes with b = 0."""
        assert self.track_estimates, "Sim2dRun(..., track_estimates=True)"
        return [f.estimate_log_read() for f in self.filters]

    def errors(self):
        """One structured array [steps] (capi.STEP_ERROR_DTYPE) per filter: the rows logged so far (one read each)."""
        assert self.track_errors, "Sim2dRun(..., track_errors=True)"
        return [f.error_log_read()[:, 0] for f in self.filters]

    def _step(self, k):
        P, d = self.P, self.data
        # predict (:588): births at the poses the last update used, then the static landmark step; host propagation
        self._each(lambda f: (f.set_poses(self.x, self.cov), f.predict_map(True)))
        noise = self.rng.standard_normal((self.n, 3)) * np.sqrt(np.diag(self.Q))     # s_k.setCov(Q); s_k.sample()  (ProcessModel.hpp:143-149)
        self.x = odometry_step(self.x, d["odom"][k]) + noise
        self.cov = self.Q.copy()
        if k <= 100:                                                                    # :590-593
            self.x = np.tile(d["gt"][k], (self.n, 1))
            self.cov = np.zeros((3, 3))
        Z = d["Z"][k]
        self.z_of_step = Z
        self.n_updates_since += 1
        if len(Z) == 0:                                                                 # RBPHDFilter.hpp:450-452
            return False
        self.n_meas_since += len(Z)
        self.n_updates += 1
        self._each(lambda f: (f.set_poses(self.x, self.cov), f.update(Z)))
        fired, tail_done = False, False
        if self.n_updates_since >= P["min_updates"] and self.n_meas_since >= 1:        # (minMeasurementsBeforeResample_ = 1, :381)
            fired = self._resample_device() if self.device_resample else self._resample()
            tail_done = self.device_resample
        if fired:
            self.n_updates_since = self.n_meas_since = 0
        elif not tail_done:
            self._each(lambda f: f.normalize_weights(f.weight_sums()[0]))
        return fired

    def _resample_device(self):
        # the device needs the draw before the decision is known: it is looked at here and taken from the stream only when the
        # resampling fired, so the realisation is the host route's
        state = self.rng.bit_generator.state
        u01 = float(self.rng.random())
        self.rng.bit_generator.state = state
        self._each(lambda f: f.resample_async(self.eff_n, self.eff_n / self.n, u01, 0, False, True))
        lrs = self._each(lambda f: f.last_resample())
        if any(lr["fired"] != lrs[0]["fired"] for lr in lrs[1:]):
            raise AssertionError("the handles' weights lead to different resampling decisions")
        if not lrs[0]["fired"]:
            return False
        for lr in lrs[1:]:
            if not np.array_equal(lr["plan"], lrs[0]["plan"]):
                raise AssertionError("the handles' weights lead to different resampling plans")
        self.rng.random()
        self.x = self.x[lrs[0]["plan"]]
        self.n_resamples += 1
        self.resample_steps.append(self.n_updates)
        return True

    def _resample(self):
        self._each(lambda f: f.normalize_weights(f.weight_sums()[0]))
        ws = self._each(lambda f: f.get_weights())
        w = ws[0]
        neff = 1.0 / float(np.sum(w * w))
        if neff > self.eff_n and neff / self.n > self.eff_n / self.n:
            return False
        u01 = float(self.rng.random())
        plans = [systematic_resample_plan(wi, u01) for wi in ws]
        for p in plans[1:]:
            if not np.array_equal(p, plans[0]):
                raise AssertionError("the handles' weights lead to different resampling plans")
        self._each(lambda f: f.resample_apply(plans[0]))
        self.x = self.x[plans[0]]
        self.n_resamples += 1
        self.resample_steps.append(self.n_updates)
        return True

    def run(self, k_from=1, k_to=None, on_step=None):
        for k in range(k_from, int(k_to or self.data["K"])):
            fired = self.step(k)
            if on_step is not None:
                on_step(k, self, fired)
        return self


def sensor_max_nz(data, P=C1_SIM, margin=2):
    """A bound that no scan of the device sensor (rfsgpu_batch_set_sensor) exceeds along data["gt"]: the most landmarks whose TRUE range
    lies within the limits at any step (only those can be detected) + the clutter count that a draw exceeds with probability below
    2^-40 per scan (the first n whose CMF reaches 1 - 2^-40; the rounded table of a larger mean never reaches the largest draw itself)
    + `margin` for a range that rounds differently on the device; at most capi.MAX_Z.  A scan beyond the bound would be cut and
    reported (RFSGPU_ERR_CAPACITY), not silently wrong.  The step kernel's LDS block, and with it how many workgroups a CU holds, is
    sized for the batch's largest bound."""
    gt, lm = data["gt"], data["landmarks"]
    n_det = 0
    if len(lm):
        r = np.hypot(lm[None, :, 0] - gt[1:, None, 0], lm[None, :, 1] - gt[1:, None, 1])
        n_det = int(((r >= P["rmin"]) & (r <= P["rmax"])).sum(axis=1).max()) if len(r) else 0
    return sensor_max_nz_of(n_det, P, margin)


def sensor_max_nz_of(n_det, P=C1_SIM, margin=2):
    """sensor_max_nz from its first term, the most landmarks in range at any step (the device truth's n_det_max, or the count
    sensor_max_nz takes along data["gt"]): + the clutter quantile + margin, at most capi.MAX_Z."""
    mean = P["clutter"] * (2 * np.pi * (P["rmax"] - P["rmin"]))
    e = np.exp(-mean)
    cmf, p, fact, n_c = e, 1.0, 1.0, 0
    while n_c < 99 and cmf < 1.0 - 2.0 ** -40:      # (src/rbphdslam2dSim.cpp:294-306 and the walk of :347-349)
        n_c += 1
        p *= mean
        fact *= n_c
        cmf += p / fact * e
    return int(min(capi.MAX_Z, max(1, n_det + n_c + margin)))


def configure_batch_filter(batch, b, P=C1_SIM):
    """setupRBPHDFilter for filter b of a FilterBatch (what configure() does for a handle)."""
    dt = P["dt"]
    cfg = batch.default_filter_config()
    cfg.birthGaussianWeight = P["birth_w"]
    cfg.minUpdatesBeforeResample = P["min_updates"]
    cfg.newGaussianCreateInnovMDThreshold = P["new_gaussian_md"]
    cfg.importanceWeightingMeasurementLikelihoodMDThreshold = P["weighting_md"]
    cfg.importanceWeightingEvalPointCount = P["n_eval"]
    cfg.importanceWeightingEvalPointGuassianWeight = P["min_weight"]
    cfg.gaussianMergingThreshold = P["merge_thr"]
    cfg.gaussianMergingCovarianceInflationFactor = P["merge_infl"]
    cfg.gaussianPruningThreshold = P["prune_thr"]
    cfg.useClusterProcess = P["use_cluster"]
    R = np.diag([P["varzr"], P["varzb"]]) * P["z_noise_inflation"]
    batch.configure(b, cfg, R=R, Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"], kf=(P["kf_range"], P["kf_bearing"]),
                    Q=np.diag([P["varlmx"], P["varlmy"]]) * dt * dt)
    return cfg


def truth_config(P=C1_SIM, b=None):
    """The generation keys of a configuration dict like C1_SIM as a capi.TruthConfig (rfsgpu_batch_set_truth): k_full = P["kmax"], the
    50 still and 100 pinned steps of generate() and the run loop.  b (a filter index, optional) is for the caller's bookkeeping only: a
    configuration does not depend on the filter's place."""
    c = capi.TruthConfig()
    c.k_full, c.n_segments, c.n_landmarks = int(P["kmax"]), int(P["n_segments"]), int(P["n_landmarks"])
    c.n_still, c.n_pinned = 50, 100
    c.dt, c.max_dx, c.max_dy, c.max_dz, c.min_dx = P["dt"], P["max_dx"], P["max_dy"], P["max_dz"], P["min_dx"]
    c.var_odo[0], c.var_odo[1], c.var_odo[2] = P["vardx"], P["vardy"], P["vardz"]
    c.rmax, c.rmin = P["rmax"], P["rmin"]
    return c


def device_truth_datas(batch, Ps, seeds, kmax):
    """The device's ground truth for every filter of `batch` ([truth] in include/rfsgpu.h): each filter's generation keys from Ps[b]
    under the key seeds[b], one generate_truth of kmax steps, and the one read of what the host needs -- landmarks, first_seen,
    n_det_max -- as a list of dicts in generate()'s layout (gt, odom and Z are None: the steps' inputs stay on the device)."""
    for b, P in enumerate(Ps):
        batch.set_truth(b, truth_config(P, b), seeds[b])
    batch.generate_truth(int(kmax))
    return [batch.get_truth(b, trajectory=False) for b in range(len(Ps))]


class Sim2dBatchRun:
    """run() :540-643 for MANY independent filters, each with its own realisation (`datas[b]`, its own generate(traj_seed=...)), its
    own configuration dict `Ps[b]` and its own host RNG stream (`seeds[b]`: process noise, resampling draws).  `target` is either a
    FilterBatch (every filter's cycle in one batch launch chain) or a list of ordinary handles, one per filter (cycled one after
    another): the same per-filter randomness drives both, so that the two can be compared.  Per cycle and filter: predict (births +
    static step) with the new poses, the update with the step's measurements (none: no update), normalisation, and
    ParticleFilter::resample's gate / N_eff test / systematic plan (FilterBatch.update_and_resample; the same rule per handle).  As in
    Sim2dRun, every cycle counts as an update for the gate (empty ones included), a filter draws its process noise every step and its
    resampling draw only when its N_eff test fires: a one-filter run takes the draws Sim2dRun takes with the same seed.

    device_loop=True (a FilterBatch only): the whole cycle on the device.  Per step propagate_async -> cycle_async(poses=None) ->
    resample_async (-> step_error_async when tracking), all stream-ordered: nothing is read back until errors(), resample_counts()
    or the end of the run, so the host only feeds the pinned rings.  The randomness is then the device's (Philox under seeds[b],
    call number = the step k), not the numpy streams of the host loop: the two loops run the same model on different realisations
    of the noise.  step() returns None in this form (the decisions stay on the device; FilterBatch.last_resample reads the last ones).

    device_sensor=True (with device_loop; with fastslam=True the batch's sensor service is switched on, serve_sensor, and the sensed
    cycle is the FastSLAM one): the scans are the device's too ([sensor] in include/rfsgpu.h).  Each filter's
    sensor is configured from Ps[b] -- the unpadded varzr / varzb, Pd, clutter, the range limits -- with the landmarks of datas[b] and
    the key seeds[b]; a step is propagate_async -> sense_async(gt[k]) -> cycle_sensed_async -> resample_sensed_async (->
    step_error_async), and no table of scans is built: datas[b]["Z"] is not read (generate(..., measurements=False) leaves it None).

    fastslam=True: the loop of src/fastslam2dSim.cpp:530-600 instead -- the same flow with FastSLAM::predict (propagation, static
    landmark step, no births) and FastSLAM::update; `target` is a FastSLAMBatch or a list of FastSLAM handles (or oracle filters),
    `Ps` dicts like C1_FASTSLAM_SIM.  A filter whose scan is empty is neither updated nor normalised that step (FastSLAM.hpp:402-403).

    device_truth=True (a FilterBatch, or a FastSLAMBatch with fastslam=True; implies device_loop and device_sensor; datas=None, kmax = the steps to generate): the
    ground truth is the device's as well ([truth] in include/rfsgpu.h).  Each filter's generation keys come from Ps[b]
    (truth_config) under the key seeds[b]; one generate_truth draws every trajectory, and the landmarks, first-seen times and
    n_det_max are read back once, for the sensors (max_nz = sensor_max_nz_of(n_det_max)) and the metric's ground truth.  run() is
    then ONE run_truth_async -- the loop over steps is the library's -- and errors() the one read.  The realisations are not
    generate()'s: the same model under another generator, as with the device loop."""

    def __init__(self, target, datas, Ps, seeds, track_errors=False, device_loop=False, fastslam=False, device_sensor=False, device_truth=False,
                 kmax=None, track_estimates=False, estimate_threshold=ESTIMATE_W_THRESHOLD, estimate_max=None, log_particles=False):
        """track_errors: as in Sim2dRun -- each filter's ground truth is uploaded, every cycle ends with one step_error_async (one
        launch for the whole batch; one per handle otherwise), errors() reads the log(s) once at the end.
        track_estimates: as in Sim2dRun -- an estimate log of estimate_max Gaussians per filter and row (None: gm_capacity), with the
        particle sets when log_particles; every cycle ends with one step_estimate_async where the error row is taken, and the one-call
        run (device_truth) logs through run_log_estimates; estimates() is the one read."""
        self.device_truth = bool(device_truth)
        if self.device_truth:
            assert datas is None and kmax is not None and isinstance(target, capi.CBatch), "device_truth: a FilterBatch or FastSLAMBatch, datas=None, kmax given"
            device_loop = device_sensor = True
            datas = device_truth_datas(target, Ps, seeds, kmax)
        self.device_loop = bool(device_loop)
        self.device_sensor = bool(device_sensor)
        assert not self.device_sensor or self.device_loop, "the device sensor serves the device loop of a FilterBatch or FastSLAMBatch"
        self.fastslam = bool(fastslam)
        self.batch = target if isinstance(target, capi.CBatch) else None
        self.handles = None if self.batch is not None else list(target)
        self.nF = len(datas)
        self.n = self.batch.n_per_filter if self.batch is not None else self.handles[0].n
        assert len(Ps) == self.nF and len(seeds) == self.nF
        assert self.batch is None or self.batch.n_filters == self.nF
        assert self.handles is None or len(self.handles) == self.nF
        self.datas, self.Ps = list(datas), list(Ps)
        self.rngs = [np.random.default_rng(s) for s in seeds]
        self.x = [np.zeros((self.n, 3)) for _ in range(self.nF)]
        self.cov = [np.zeros((3, 3)) for _ in range(self.nF)]
        self.Q = [np.diag([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2 for P in self.Ps]
        self.eff_n = np.array([float(P["eff_n"]) for P in self.Ps])
        if self.fastslam:
            if self.batch is not None:
                self.cfgs = [configure_fastslam_batch_filter(self.batch, b, P) for b, P in enumerate(self.Ps)]
                if self.device_sensor:      # (after the configuration, which decides the batch's kind: the switch is per kind)
                    self.batch.serve_sensor(True)
            else:
                self.cfgs = [configure_fastslam(f, P) for f, P in zip(self.handles, self.Ps)]
        elif self.batch is not None:
            self.cfgs = [configure_batch_filter(self.batch, b, P) for b, P in enumerate(self.Ps)]
        else:
            self.cfgs = [configure(f, P) for f, P in zip(self.handles, self.Ps)]
        self.n_updates_since = np.zeros(self.nF, dtype=np.int64)
        self.n_meas_since = np.zeros(self.nF, dtype=np.int64)
        self.last_n_z = np.zeros(self.nF, dtype=np.int64)
        self.last_fired = np.zeros(self.nF, dtype=bool)
        self.last_plans = [np.arange(self.n) for _ in range(self.nF)]
        self.n_resamples = np.zeros(self.nF, dtype=np.int64)
        self.resample_steps = [[] for _ in range(self.nF)]    # the steps k at which each filter resampled
        self.track_errors = bool(track_errors)
        if self.track_errors:
            rows = int(min(d["K"] for d in self.datas))
            for b, (d, P) in enumerate(zip(self.datas, self.Ps)):
                fs = d["first_seen"] if self.device_truth else first_seen_times(d, P)
                if self.batch is not None:
                    self.batch.set_ground_truth(d["landmarks"], fs, filter=b)
                else:
                    self.handles[b].set_ground_truth(d["landmarks"], fs)
                    self.handles[b].error_log_create(rows)
            if self.batch is not None:
                self.batch.error_log_create(rows)
        self.track_estimates = bool(track_estimates)
        self.estimate_threshold = float(estimate_threshold)
        if self.track_estimates:
            rows = int(min(d["K"] for d in self.datas))
            for f in ([self.batch] if self.batch is not None else self.handles):
                f.estimate_log_create(rows, f.gm_capacity if estimate_max is None else int(estimate_max), log_particles)
            if self.device_truth:
                self.batch.run_log_estimates(True, self.estimate_threshold)
        if self.device_loop:
            assert self.batch is not None, "the device loop needs a FilterBatch"
            self._device_loop_setup(seeds)

    def _device_loop_setup(self, seeds):
        """The filters' motion / resampling parameters, and every step's inputs in the layout the calls take (packed once: the
        measurements are pre-generated, the per-step host work is three calls)."""
        K = int(min(d["K"] for d in self.datas))
        nF = self.nF
        for b in range(nF):
            self.batch.set_motion_odometry(b, np.diag(self.Q[b]), seeds[b])
            self.batch.set_resampling(b, self.eff_n[b], self.eff_n[b] / self.n)
        if self.device_truth:       # no per-step host table at all: the steps' inputs are rows of the truth tables on the device
            for b, (d, P) in enumerate(zip(self.datas, self.Ps)):
                self.batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"],
                                      max_nz=sensor_max_nz_of(d["n_det_max"], P), seed=seeds[b])
            return
        self._u = np.ascontiguousarray(np.stack([d["odom"][:K] for d in self.datas], axis=1))          # [K, nF, 3]
        self._gt = np.ascontiguousarray(np.stack([d["gt"][:K] for d in self.datas], axis=1))
        self._t = np.array([[k * P["dt"] for P in self.Ps] for k in range(K)])
        self._pin_all = np.ones(nF, dtype=np.uint8)
        if self.device_sensor:      # each filter's simulated sensor: the UNPADDED noise (the filter's own R is inflated); no table of scans
            for b, (d, P) in enumerate(zip(self.datas, self.Ps)):
                self.batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"],
                                      max_nz=sensor_max_nz(d, P), seed=seeds[b])
            return
        self._z = np.zeros((K, nF, capi.MAX_Z, 2))
        self._nz = np.zeros((K, nF), dtype=np.int32)
        for b, d in enumerate(self.datas):
            for k in range(K):
                Z = d["Z"][k] if k < len(d["Z"]) else np.zeros((0, 2))
                m = len(Z)
                assert m <= capi.MAX_Z
                self._nz[k, b] = m
                if m:
                    self._z[k, b, :m] = Z

    def _device_propagate(self, k):
        bt = self.batch
        if k <= 100:                                                                    # :590-593
            bt.propagate_async(self._u[k], k, pin=self._pin_all, pin_pose=self._gt[k])
        else:
            bt.propagate_async(self._u[k], k)

    def _device_step(self, k):
        self._device_propagate(k)
        return self._device_update(k)

    def _device_update(self, k):
        bt = self.batch
        if self.device_sensor:
            bt.sense_async(self._gt[k], k)
            if self.fastslam:
                bt.fastslam_cycle_sensed_async(True, normalize=True)
            else:
                bt.cycle_sensed_async(True, normalize=True)
            bt.resample_sensed_async(k)
            self.last_n_z = None            # (on the device: FilterBatch.last_scan reads the sets)
            if self.track_errors:
                bt.step_error_async(self._t[k], self._gt[k], ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
            if self.track_estimates:
                bt.step_estimate_async(self._t[k], self.estimate_threshold)
            return None
        if self.fastslam:
            bt.batch_fastslam_cycle_async_packed(True, self._z[k], self._nz[k], normalize=True)
        else:
            bt.batch_cycle_async_packed(True, self._z[k], self._nz[k], normalize=True)
        bt.resample_async(self._nz[k], k)
        self.last_n_z = self._nz[k]
        if self.track_errors:
            bt.step_error_async(self._t[k], self._gt[k], ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
        if self.track_estimates:
            bt.step_estimate_async(self._t[k], self.estimate_threshold)
        return None

    def resample_counts(self):
        """Resamplings per filter so far (the device loop: one read-back; the host loop: its own count)."""
        return self.batch.resample_counts() if self.device_loop else self.n_resamples.copy()

    def step(self, k):
        if self.device_truth:
            self.batch.run_truth_async(k, k + 1, self.track_errors, ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
            self.last_n_z = None
            return None
        if self.device_loop:
            return self._device_step(k)
        fired = self._step(k)
        if self.track_errors:
            t = np.array([k * P["dt"] for P in self.Ps])
            g = np.array([d["gt"][k] for d in self.datas])
            if self.batch is not None:
                self.batch.step_error_async(t, g, ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
            else:
                for b, f in enumerate(self.handles):
                    f.step_error_async(t[b], g[b][None, :], ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
        if self.track_estimates:
            t = np.array([k * P["dt"] for P in self.Ps])
            if self.batch is not None:
                self.batch.step_estimate_async(t, self.estimate_threshold)
            else:
                for b, f in enumerate(self.handles):
                    f.step_estimate_async(t[b], self.estimate_threshold)
        return fired

    def errors(self):
        """The rows logged so far as one structured array [steps, n_filters] (capi.STEP_ERROR_DTYPE): one read (per handle)."""
        assert self.track_errors, "Sim2dBatchRun(..., track_errors=True)"
        if self.batch is not None:
            return self.batch.error_log_read()
        return np.stack([f.error_log_read()[:, 0] for f in self.handles], axis=1)

    def estimates(self):
        """(hdr [steps, n_filters], gauss [steps, n_filters, 6, max_est], part [steps, n_filters, 4, slots] or None): the estimate
        rows logged so far (capi.CFilter.estimate_log_read): one read (per handle) -- what write_run_logs takes."""
        assert self.track_estimates, "Sim2dBatchRun(..., track_estimates=True)"
        if self.batch is not None:
            return self.batch.estimate_log_read()
        each = [f.estimate_log_read() for f in self.handles]
        return tuple(None if each[0][q] is None else np.concatenate([e[q] for e in each], axis=1) for q in range(3))

    def _step(self, k):
        Zs = []
        for b in range(self.nF):
            d = self.datas[b]
            noise = self.rngs[b].standard_normal((self.n, 3)) * np.sqrt(np.diag(self.Q[b]))
            self.x[b] = odometry_step(self.x[b], d["odom"][k]) + noise
            self.cov[b] = self.Q[b].copy()
            if k <= 100:
                self.x[b] = np.tile(d["gt"][k], (self.n, 1))
                self.cov[b] = np.zeros((3, 3))
            Zs.append(d["Z"][k] if k < len(d["Z"]) else np.zeros((0, 2)))
        n_z = np.array([len(Z) for Z in Zs])
        covs = [np.tile(c.ravel(), (self.n, 1)) for c in self.cov]
        if self.batch is not None:
            self.batch.cycle_async(True, Zs, poses=np.vstack(self.x), pose_cov=np.vstack(covs), normalize=True)
            fired, plan = self.batch.update_and_resample(n_z, lambda b: self.rngs[b].random(), self.eff_n)
            plans = [plan[self.batch.block(b)] - b * self.n for b in range(self.nF)]
        else:
            fired = np.zeros(self.nF, dtype=bool)
            plans = []
            for b, f in enumerate(self.handles):
                if self.fastslam:   # FastSLAM::predict's map part, then FastSLAM::update; an empty scan: no update, no normalisation
                    f.set_poses(self.x[b], covs[b])
                    f.predict_map(False)
                    if n_z[b]:
                        f.fastslam_update(Zs[b])
                        f.normalize_weights(f.weight_sums()[0])
                elif hasattr(f, "cycle_async"):
                    f.cycle_async(True, Zs[b], poses=self.x[b], pose_cov=covs[b], normalize=True)
                else:       # a handle with the plain calls only (the CPU oracle): the same cycle call by call
                    f.predict_map(True)
                    f.set_poses(self.x[b], covs[b])
                    if n_z[b]:
                        f.update(Zs[b])
                    f.normalize_weights(f.weight_sums()[0])
                plan = np.arange(self.n)
                self.n_updates_since[b] += 1                 # (every cycle counts, RBPHDFilter.hpp:448 before :450-452)
                if n_z[b]:
                    self.n_meas_since[b] += int(n_z[b])
                    c = self.cfgs[b]
                    if self.n_updates_since[b] >= c.minUpdatesBeforeResample and self.n_meas_since[b] >= c.minMeasurementsBeforeResample:
                        w = f.get_weights()
                        neff = 1.0 / float(np.sum(w * w))
                        if not (neff > self.eff_n[b] and neff / self.n > self.eff_n[b] / self.n):
                            plan = systematic_resample_plan(w, float(self.rngs[b].random()))
                            f.resample_apply(plan)
                            fired[b] = True
                            self.n_updates_since[b] = self.n_meas_since[b] = 0
                plans.append(plan)
        for b in range(self.nF):
            if fired[b]:
                self.x[b] = self.x[b][plans[b]]
                self.resample_steps[b].append(k)
        self.n_resamples += fired
        self.last_n_z, self.last_fired, self.last_plans = n_z, fired, plans
        return fired

    def run(self, k_from=1, k_to=None, on_step=None):
        k_to = int(k_to or min(d["K"] for d in self.datas))
        if self.device_truth and on_step is None:      # the loop over steps is the library's: one call
            self.batch.run_truth_async(k_from, k_to, self.track_errors, ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
            self.last_n_z = None
            return self
        for k in range(k_from, k_to):
            fired = self.step(k)
            if on_step is not None:
                on_step(k, self, fired)
        return self


class Sim2dMHBatchRun:
    """The simulator loop for multi-hypothesis FastSLAM filters in one of three forms: an MHFastSLAMBatch with its host loop (the host
    reads the counts and poses back, propagates the live slots and passes them with the cycle) or its device loop (propagate_async +
    cycle, nothing read back), or handles on rfsgpu_fastslam_cycle_async stepped in turn.  Every filter's draws are pre-drawn from its
    seed, so the device loop waits for nothing.  `n`: the particles a filter starts with (None: the target's own count).

    track_errors=True (a batch target only; the contract of Sim2dBatchRun): the batch's metric service is switched on
    (serve_metrics), each filter's ground truth is uploaded with its first_seen_times, the log is sized to the run, every step ends
    with one step_error_async(t = k * dt, gt_pose) -- the kernel reads each filter's live count on the device, so the device loop
    still reads nothing back -- and errors() is the one read at the end.

    device_sensor=True (a batch target; implies device_loop): the batch's sensor service is switched on (serve_sensor), each filter's
    sensor is configured as Sim2dBatchRun configures it, a step is propagate_async -> sense_async(gt[k]) ->
    fastslam_mh_cycle_sensed_async(True, k), and neither a table of scans nor the resampling draws are made on the host: a filter's draw
    is the device's resampling draw of (seeds[b], k).  device_truth=True (implies device_sensor; datas=None, kmax = the steps to
    generate): the ground truth is the device's too (device_truth_datas), and run() without on_step is ONE run_truth_async."""

    def __init__(self, target, datas, Ps, seeds, n=None, device_loop=False, track_errors=False, device_sensor=False, device_truth=False, kmax=None,
                 track_estimates=False, estimate_threshold=ESTIMATE_W_THRESHOLD, estimate_max=None, log_particles=False):
        self.device_truth = bool(device_truth)
        self.device_sensor = bool(device_sensor) or self.device_truth
        if self.device_sensor:
            assert isinstance(target, capi.CBatchMH), "the device sensor and truth need an MHFastSLAMBatch"
            device_loop = True
        if self.device_truth:
            assert datas is None and kmax is not None, "device_truth: datas=None, kmax given"
            datas = device_truth_datas(target, Ps, seeds, kmax)
        self.datas, self.Ps, self.nF = list(datas), list(Ps), len(datas)
        self.batch = target if isinstance(target, capi.CBatchMH) else None
        self.handles = None if self.batch is not None else list(target)
        self.n = n = int(n if n is not None else (self.batch.n_per_filter if self.batch is not None else self.handles[0].n))
        self.device_loop = bool(device_loop)
        self.track_errors = bool(track_errors)
        self.track_estimates = bool(track_estimates)
        self.estimate_threshold = float(estimate_threshold)
        assert self.batch is not None or not (self.device_loop or self.track_errors or self.track_estimates), "the device loop and the error tracking need an MHFastSLAMBatch"
        K = int(min(d["K"] for d in datas))
        self.rngs = [np.random.default_rng(s) for s in seeds]
        if not self.device_sensor:
            self.u01 = np.ascontiguousarray(np.stack([np.random.default_rng(10_000 + s).random(K) for s in seeds], axis=1))      # [K, nF]
        self.Q = [np.diag([P["vardx"], P["vardy"], P["vardz"]]) * P["p_noise_inflation"] * P["dt"] ** 2 for P in Ps]
        for b, P in enumerate(Ps):
            if self.batch is not None:
                c = configure_fastslam_batch_filter(self.batch, b, P)
                c.nParticlesMax = 3 * n
                self.batch.configure_fastslam(b, c)
                self.batch.set_resampling(b, P["eff_n"], P["eff_n"] / n)
                self.batch.set_motion_odometry(b, np.diag(self.Q[b]), seeds[b])
            else:
                h = self.handles[b]
                h.fs_config = configure_fastslam(h, P)
                h.fs_config.nParticlesMax = 3 * n
                h.setEffectiveParticleCountThreshold(P["eff_n"])
        if self.device_sensor:      # each filter's simulated sensor: the UNPADDED noise (the filter's own R is inflated); no table of scans
            self.batch.serve_sensor(True)
            for b, (d, P) in enumerate(zip(self.datas, self.Ps)):
                self.batch.set_sensor(b, np.diag([P["varzr"], P["varzb"]]), P["Pd"], P["clutter"], P["rmax"], P["rmin"], d["landmarks"],
                                      max_nz=sensor_max_nz_of(d["n_det_max"], P) if self.device_truth else sensor_max_nz(d, P), seed=seeds[b])
        if not self.device_truth:      # (else no per-step host table at all: the steps' inputs are rows of the truth tables on the device)
            self._u = np.ascontiguousarray(np.stack([d["odom"][:K] for d in datas], axis=1))
            self._gt = np.ascontiguousarray(np.stack([d["gt"][:K] for d in datas], axis=1))
            self._t = np.array([[k * P["dt"] for P in Ps] for k in range(K)])
            self._pin_all = np.ones(self.nF, dtype=np.uint8)
        if not self.device_sensor:
            self._z = np.zeros((K, self.nF, capi.MAX_Z, 2))
            self._nz = np.zeros((K, self.nF), dtype=np.int32)
            for b, d in enumerate(datas):
                for k in range(K):
                    Z = d["Z"][k] if k < len(d["Z"]) else np.zeros((0, 2))
                    self._nz[k, b] = len(Z)
                    self._z[k, b, :len(Z)] = Z
        if self.track_errors:
            self.batch.serve_metrics(True)
            for b, (d, P) in enumerate(zip(self.datas, self.Ps)):
                self.batch.set_ground_truth(d["landmarks"], d["first_seen"] if self.device_truth else first_seen_times(d, P), filter=b)
            self.batch.error_log_create(K)
        if self.track_estimates:    # (served where the metric is: the same switch; the kernel reads each filter's live count on the device)
            self.batch.serve_metrics(True)
            self.batch.estimate_log_create(K, self.batch.gm_capacity if estimate_max is None else int(estimate_max), log_particles)
            if self.device_truth:
                self.batch.run_log_estimates(True, self.estimate_threshold)

    def _moved(self, b, x, k):
        """ParticleFilter::propagate of filter b's live particles on the host (the ground truth for the first 100 steps, :590-593)."""
        if k <= 100:
            return np.tile(self._gt[k, b], (x.shape[0], 1)), np.zeros(9)
        noise = self.rngs[b].standard_normal(x.shape) * np.sqrt(np.diag(self.Q[b]))
        return odometry_step(x, self._u[k, b]) + noise, self.Q[b].ravel()

    def step(self, k):
        bt = self.batch
        if self.device_truth:
            bt.run_truth_async(k, k + 1, self.track_errors, ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
            return
        if self.device_sensor:
            bt.propagate_async(self._u[k], k, pin=self._pin_all if k <= 100 else None, pin_pose=self._gt[k] if k <= 100 else None)
            bt.sense_async(self._gt[k], k)
            bt.fastslam_mh_cycle_sensed_async(True, k)
        elif self.device_loop:
            bt.propagate_async(self._u[k], k, pin=self._pin_all if k <= 100 else None, pin_pose=self._gt[k] if k <= 100 else None)
            bt.batch_fastslam_mh_cycle_async_packed(True, self._z[k], self._nz[k], self.u01[k])
        elif bt is not None:
            counts = bt.live_counts()
            x = bt.get_poses()
            cov = np.zeros((bt.n, 9))
            for b in range(self.nF):
                blk = bt.block(b, counts[b])
                x[blk], cov[blk] = self._moved(b, x[blk], k)
            bt.batch_fastslam_mh_cycle_async_packed(True, self._z[k], self._nz[k], self.u01[k], poses=x, pose_cov=cov)
        else:
            for b, h in enumerate(self.handles):
                x, c = self._moved(b, h.get_poses(), k)
                h.set_poses(x, np.tile(c, (x.shape[0], 1)))
                h.cycle_async(self._z[k, b, :self._nz[k, b]], float(self.u01[k, b]), predict=True)
        if self.track_errors:
            bt.step_error_async(self._t[k], self._gt[k], ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
        if self.track_estimates:
            bt.step_estimate_async(self._t[k], self.estimate_threshold)

    def estimates(self):
        """(hdr, gauss, part) as Sim2dBatchRun.estimates(): part [steps, n_filters, 4, max_per_filter], a row's first n_particles
        entries per plane being the filter's live set."""
        assert self.track_estimates, "Sim2dMHBatchRun(..., track_estimates=True)"
        return self.batch.estimate_log_read()

    def errors(self):
        """The rows logged so far as one structured array [steps, n_filters] (capi.STEP_ERROR_DTYPE): the one read (it also waits for
        the queued work)."""
        assert self.track_errors, "Sim2dMHBatchRun(..., track_errors=True)"
        return self.batch.error_log_read()

    def run(self, k_from=1, k_to=None, on_step=None):
        k_to = int(k_to or min(d["K"] for d in self.datas))
        if self.device_truth and on_step is None:      # the loop over steps is the library's: one call
            self.batch.run_truth_async(k_from, k_to, self.track_errors, ERROR_W_THRESHOLD, ERROR_CUTOFF, ERROR_ORDER)
            return self
        for k in range(k_from, k_to):
            self.step(k)
            if on_step is not None:
                on_step(k, self)
        return self

    def synchronize(self):
        for f in ([self.batch] if self.batch is not None else self.handles):
            f.synchronize()


def write_run_logs(log_dir, b, estimates, truth, precision=None):
    """Filter b's log files in the formats of the reference's simulators (src/rbphdslam2dSim.cpp:388-437, :620-638), from the rows of
    an estimate log: `estimates` = (hdr, gauss, part) as estimates() / capi.CFilter.estimate_log_read return them (part needs
    log_particles), `truth` a dict with gt [K, 3], odom [K, 3], landmarks [L, 2], dt and optionally first_seen [L] (absent: all -1) --
    generate()'s dict plus dt, or FilterBatch.get_truth(b)'s.  Writes into log_dir (created if missing)
        gtPose.dat         `t x y theta`                      one line per step k, t = k dt
        gtLandmark.dat     `x y t_first_in_range`
        deadReckoning.dat  `t x y theta`                      pose[0] = gt[0], pose[k] = odometry_step(pose[k - 1], odom[k])
        particlePose.dat   `t i x y theta w`                  per logged row the filter's n_particles particles, then one blank line
        landmarkEst.dat    `t i mx my sxx sxy syy w`          per logged row the n_logged Gaussians of the best particle i
    with i the slot inside the filter.  Numbers are printed with %f as the reference prints them; precision = p prints %.pg instead
    (17: every double comes back exactly).  tools/analysis2d_sim.py reads the directory."""
    import os
    hdr, gauss, part = estimates
    if part is None:
        raise ValueError("write_run_logs: particlePose.dat needs the particle planes (estimate_log_create(..., log_particles=True))")
    os.makedirs(log_dir, exist_ok=True)
    num = "%f" if precision is None else "%%.%dg" % int(precision)
    sep = "   "
    gt, odom = np.asarray(truth["gt"], dtype=np.float64), np.asarray(truth["odom"], dtype=np.float64)
    lm = np.asarray(truth["landmarks"], dtype=np.float64).reshape(-1, 2)
    fs = truth.get("first_seen")
    fs = np.full(len(lm), -1.0) if fs is None else np.asarray(fs, dtype=np.float64)
    dt = float(truth["dt"])
    K = gt.shape[0]

    def line(*cols):
        return sep.join(("%d" % c) if isinstance(c, (int, np.integer)) else (num % c) for c in cols) + "\n"

    with open(os.path.join(log_dir, "gtPose.dat"), "w") as fh:
        for k in range(K):
            fh.write(line(k * dt, gt[k, 0], gt[k, 1], gt[k, 2]))
    with open(os.path.join(log_dir, "gtLandmark.dat"), "w") as fh:
        for m in range(len(lm)):
            fh.write(line(lm[m, 0], lm[m, 1], fs[m]))
    with open(os.path.join(log_dir, "deadReckoning.dat"), "w") as fh:
        x = gt[0].copy()
        for k in range(K):
            if k:
                x = odometry_step(x, odom[k])
            fh.write(line(k * dt, x[0], x[1], x[2]))
    stride = part.shape[3]
    with open(os.path.join(log_dir, "particlePose.dat"), "w") as fp, open(os.path.join(log_dir, "landmarkEst.dat"), "w") as fl:
        for r in range(hdr.shape[0]):
            h = hdr[r, b]
            t = float(h["t"])
            P = part[r, b]
            for i in range(int(h["n_particles"])):
                fp.write(line(t, i, P[0, i], P[1, i], P[2, i], P[3, i]))
            fp.write("\n")
            G = gauss[r, b]
            i_best = int(h["best_slot"]) - b * stride
            for m in range(int(h["n_logged"])):
                fl.write(line(t, i_best, G[0, m], G[1, m], G[2, m], G[3, m], G[4, m], G[5, m]))
    return log_dir


def map_error(f, i, landmarks, w_min=0.5, cutoff=0.5):
    """Matched landmarks / mean error of particle i's strong Gaussians against the ground truth (greedy nearest, as the C++ driver's summary)."""
    w, _, mean, _ = f.export_gm(i)
    strong = mean[w >= w_min]
    taken = np.zeros(len(landmarks), dtype=bool)
    errs = []
    for m in strong:
        dist = np.linalg.norm(landmarks - m, axis=1)
        dist[taken] = np.inf
        j = int(np.argmin(dist)) if len(dist) else -1
        if j >= 0 and dist[j] < cutoff:
            taken[j] = True
            errs.append(dist[j])
    return int(taken.sum()), (float(np.mean(errs)) if errs else float("nan")), len(strong)
