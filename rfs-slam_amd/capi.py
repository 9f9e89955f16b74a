"""ctypes binding of the C ABI in include/rfsgpu.h.

The binding is prefix-parametrised (`rfsgpu_` for the product library) so that test infrastructure can
drive a second library exposing the same call shapes through identical Python calls.  Nothing here loads
anything but the library it is handed.

Mirrors the public surface of rfs::RBPHDFilter (reference include/RBPHDFilter.hpp:72-251): method
names follow the reference (predict / update / getGMSize / getLandmark / ...), error behaviour too
(getGMSize -> -1, getLandmark -> None on bad indices, update/predict raise only on engine failure).
"""
import ctypes as C
import numpy as np

OK = 0
ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_NO_DEVICE, ERR_UNSUPPORTED = 1, 2, 3, 4, 5
INHERIT_REFERENCE, INHERIT_EAGER, INHERIT_EXTERNAL = 0, 1, 2
MODEL_RNGBRG_2D = 0
MODEL_VICTORIAPARK_3D = 1
VP_MAX_PD = 16
MAX_CANDIDATES = 256
MAX_Z = 64
MAX_EVAL = 64
MAX_METRIC_SET = 512
SENSOR_MAX_LANDMARKS = 512
TRUTH_MAX_STEPS = 4096


class FilterConfig(C.Structure):
    """RBPHDFilter::Config (include/RBPHDFilter.hpp:90-146)."""
    _fields_ = [
        ("birthGaussianWeight", C.c_double),
        ("birthGaussianMeasurementCountThreshold", C.c_uint),
        ("birthGaussianMeasurementCheckThreshold", C.c_uint),
        ("birthGaussianMeasurementSupportDist", C.c_double),
        ("birthGaussianCurrentMeasurementCountThreshold", C.c_uint),
        ("newGaussianCreateInnovMDThreshold", C.c_double),
        ("importanceWeightingEvalPointCount", C.c_int),
        ("importanceWeightingEvalPointGuassianWeight", C.c_double),
        ("importanceWeightingMeasurementLikelihoodMDThreshold", C.c_double),
        ("gaussianMergingThreshold", C.c_double),
        ("gaussianMergingCovarianceInflationFactor", C.c_double),
        ("gaussianPruningThreshold", C.c_double),
        ("minUpdatesBeforeResample", C.c_int),
        ("minMeasurementsBeforeResample", C.c_int),
        ("useClusterProcess", C.c_int),
    ]


class RngBrgConfig(C.Structure):
    """MeasurementModel_RngBrg::Config + R (include/MeasurementModel_RngBrg.hpp:65-71)."""
    _fields_ = [
        ("R", C.c_double * 4),
        ("probabilityOfDetection", C.c_double),
        ("uniformClutterIntensity", C.c_double),
        ("rangeLimMax", C.c_double),
        ("rangeLimMin", C.c_double),
        ("rangeLimBuffer", C.c_double),
    ]


class VPConfig(C.Structure):
    """MeasurementModel_VictoriaPark::Config + R, Slb (include/MeasurementModel_VictoriaPark.hpp:150-158)."""
    _fields_ = [
        ("R", C.c_double * 9),
        ("Slb", C.c_double),
        ("PdTable", C.c_double * VP_MAX_PD),
        ("nPd", C.c_int),
        ("expectedClutterNumber", C.c_double),
        ("rangeLimMax", C.c_double),
        ("rangeLimMin", C.c_double),
        ("bearingLimitMax", C.c_double),
        ("bearingLimitMin", C.c_double),
        ("bufferZonePd", C.c_double),
    ]


class KFConfig(C.Structure):
    """KalmanFilter_RngBrg::Config (include/KalmanFilter_RngBrg.hpp:55-60)."""
    _fields_ = [("rangeInnovationThreshold", C.c_double), ("bearingInnovationThreshold", C.c_double)]


class FastSlamConfig(C.Structure):
    """FastSLAM::Config (include/FastSLAM.hpp:106-132)."""
    _fields_ = [
        ("minUpdatesBeforeResample", C.c_int),
        ("minMeasurementsBeforeResample", C.c_int),
        ("landmarkExistencePrior", C.c_double),
        ("mapExistencePruneThreshold", C.c_double),
        ("minLogMeasurementLikelihood", C.c_double),
        ("nParticlesMax", C.c_int),
        ("maxNDataAssocHypotheses", C.c_uint),
        ("maxDataAssocLogLikelihoodDiff", C.c_double),
        ("landmarkCandidateMeasurementSupportDist", C.c_double),
        ("landmarkCandidateMeasurementCountThreshold", C.c_uint),
        ("landmarkCandidateCurrentMeasurementCountThreshold", C.c_uint),
        ("landmarkCandidateMeasurementCheckThreshold", C.c_uint),
        ("landmarkLockWeight", C.c_double),
        ("pruningMeasurementsThreshold", C.c_uint),
    ]


class TruthConfig(C.Structure):
    """rfsgpu_truth_config: the simulator's generation keys of one filter ([truth] in include/rfsgpu.h)."""
    _fields_ = [("k_full", C.c_int), ("n_segments", C.c_int), ("n_landmarks", C.c_int), ("n_still", C.c_int), ("n_pinned", C.c_int),
                ("dt", C.c_double), ("max_dx", C.c_double), ("max_dy", C.c_double), ("max_dz", C.c_double), ("min_dx", C.c_double),
                ("var_odo", C.c_double * 3), ("rmax", C.c_double), ("rmin", C.c_double)]


class Timing(C.Structure):
    """RBPHDFilter::TimingInfo (include/RBPHDFilter.hpp:152-167), ns."""
    _fields_ = [(n + s, C.c_longlong) for n in
                ("predict", "mapUpdate", "mapUpdate_kf", "particleWeighting", "mapMerge", "mapPrune", "particleResample")
                for s in ("_wall", "_cpu")]


class StepError(C.Structure):
    """rfsgpu_step_error: one filter's record of one rfsgpu_step_error[_async] call (every field 8 bytes wide)."""
    _fields_ = [("t", C.c_double), ("status", C.c_longlong), ("best_slot", C.c_longlong), ("n_est", C.c_longlong), ("n_truth", C.c_longlong),
                ("cardinality", C.c_double), ("ospa", C.c_double), ("cola", C.c_double), ("e_dist", C.c_double), ("e_card", C.c_double),
                ("pose_ex", C.c_double), ("pose_ey", C.c_double), ("pose_eth", C.c_double), ("pose_ed", C.c_double), ("weight_sum", C.c_double)]


# the same layout as a numpy structured dtype (error_log_read / step_error return arrays of it)
STEP_ERROR_DTYPE = np.dtype([(n, np.int64 if t is C.c_longlong else np.float64) for n, t in StepError._fields_])


class StepEstimate(C.Structure):
    """rfsgpu_step_estimate: one filter's header of one row of the estimate log (every field 8 bytes wide)."""
    _fields_ = [("t", C.c_double), ("status", C.c_longlong), ("best_slot", C.c_longlong), ("n_particles", C.c_longlong), ("n_est", C.c_longlong),
                ("n_logged", C.c_longlong), ("cardinality", C.c_double), ("best_weight", C.c_double), ("weight_sum", C.c_double),
                ("best_x", C.c_double), ("best_y", C.c_double), ("best_theta", C.c_double),
                ("mean_x", C.c_double), ("mean_y", C.c_double), ("mean_cos", C.c_double), ("mean_sin", C.c_double)]


STEP_ESTIMATE_DTYPE = np.dtype([(n, np.int64 if t is C.c_longlong else np.float64) for n, t in StepEstimate._fields_])
# the planes of the estimate log's gauss [rows, n_filters, 6, max_est] and part [rows, n_filters, 4, slots] arrays
ESTIMATE_GAUSS_PLANES = ("mx", "my", "sxx", "sxy", "syy", "w")
ESTIMATE_PART_PLANES = ("x", "y", "theta", "w")


# every symbol include/rfsgpu.h declares, without prefix (tests check the product .so exports them all)
ABI_SYMBOLS = [
    "abi_version", "create", "destroy", "last_error", "default_filter_config", "set_filter_config",
    "get_filter_config", "set_model_rngbrg", "set_kf_config", "set_lmk_process_noise", "set_poses", "get_poses",
    "set_weights", "get_weights", "gm_size", "get_landmark", "import_gm", "export_gm", "gm_sizes", "predict_map",
    "update", "update_map", "importance_weighting", "merge", "prune", "get_unused", "landmarks_in_fov",
    "weight_sums", "weight_sums_async", "weight_sums_device_ptr", "normalize_weights", "resample_apply",
    "get_timing", "reset_timing", "synchronize", "stream", "last_kernel_ns", "last_step_variant", "mat_perm", "mat_perm_last_kernel_ms",
    "set_stream", "bind_weight_sums_buffer", "save_state", "restore_state", "state_ring_create", "state_ring_seed", "state_ring_next", "import_aux",
    "set_model_victoriapark", "set_laser_scan", "export_birth_candidates", "import_birth_candidates",
    "update_async", "kernel_time_stats", "post_kernel_avg_ns", "set_step_timing_stride", "step_launch_order",
    "default_fastslam_config", "set_fastslam_config", "get_fastslam_config", "fastslam_update",
    "normalize_weights_parts", "create_ex", "n_particles", "max_particles", "resample_apply_n",
    "fastslam_set_resample_occured", "particle_parents", "vp_probe_pd", "fastslam_cycle_async", "fastslam_last_cycle", "fastslam_set_resampling",
    "fastslam_cycle_full_async", "fastslam_cycle_pending", "fastslam_cycle_counts", "debug_slot",
    "slab_row_bytes", "export_slab_rows", "import_slab_rows", "weights_device_ptr", "step_async", "set_step_inputs_async", "predict_map_async", "set_phase_timing", "static_steps_async", "propagate_ackerman_async", "propagate_ackerman_run_async", "set_partition_mode", "get_partition_mode",
    "set_birth_inheritance", "get_birth_inheritance", "get_particle_ids", "set_particle_ids", "resample_occured", "get_unused_masks", "set_unused_masks", "has_birth_candidates", "predict_map_level", "murty_partition_sums", "partition_likelihoods", "cycle_async", "update_io", "step_async_deferred", "step_async_trailing", "collective_gate", "collective_publish", "collective_probe",
    "group_create", "group_destroy", "group_last_error", "group_n_shards", "group_n_particles", "group_shard", "group_locate",
    "group_set_filter_config", "group_set_model_rngbrg", "group_set_kf_config", "group_set_lmk_process_noise", "group_set_poses",
    "group_get_poses", "group_set_weights", "group_get_weights", "group_predict_map", "group_update", "group_normalize",
    "group_resample", "group_apply_plan", "group_migration_stats", "group_gm_size", "group_get_landmark", "group_synchronize", "group_set_birth_inheritance", "group_get_particle_ids",
    "group_update_io", "group_update_deferred", "group_set_model_victoriapark", "group_set_laser_scan", "group_set_phase_timing", "group_get_timing", "group_collective",
    "create_batch", "n_filters", "batch_configure", "batch_cycle_async", "batch_weight_sums", "batch_resample_apply", "batch_resample_occured", "murty_seen",
    "batch_set_motion_odometry", "batch_set_resampling", "batch_propagate_async", "batch_resample_async", "batch_last_resample", "batch_resample_counts", "batch_get_pose_covs",
    "batch_set_fastslam_config", "batch_fastslam_cycle_async",
    "create_batch_mh", "batch_fastslam_mh_cycle_async", "batch_fastslam_last_cycle", "batch_live_counts", "batch_mh_serve_metrics",
    "set_ground_truth", "error_log_create", "error_log_reset", "step_error_async", "error_log_read", "step_error", "get_map_estimate",
    "resample_async", "last_resample", "get_pose_covs",
    "rbphd_set_resampling", "rbphd_cycle_async", "rbphd_cycle_counts", "rbphd_last_cycle", "rbphd_cycle_pending",
    "batch_set_sensor", "batch_sense_async", "batch_cycle_sensed_async", "batch_resample_sensed_async", "batch_last_scan", "batch_last_cycle_lds",
    "batch_set_truth", "batch_generate_truth", "batch_get_truth", "batch_run_truth_async",
    "batch_fastslam_serve_sensor", "batch_fastslam_cycle_sensed_async", "batch_fastslam_mh_cycle_sensed_async",
    "estimate_log_create", "estimate_log_reset", "step_estimate_async", "estimate_log_read", "batch_run_log_estimates",
    "handle_serve_estimates", "batch_vp_serve_estimates",
    "batch_configure_vp", "batch_vp_cycle_async",
    "batch_vp_set_motion", "batch_vp_set_resampling", "batch_vp_propagate_run_async", "batch_vp_resample_async", "batch_vp_last_resample", "batch_vp_loop_counts",
    "batch_vp_serve_fastslam", "batch_vp_fastslam_cycle_async",
    "create_batch_vp_mh", "batch_vp_fastslam_mh_cycle_async",
]

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


class EngineError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"rfsgpu status {status}: {msg}")
        self.status = status


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


class CFilter:
    """One filter handle behind the C ABI (one GPU / one shard of particles)."""

    def __init__(self, lib, prefix, n_particles, model=MODEL_RNGBRG_2D, device_id=0, gm_capacity=512, max_particles=None, borrowed=None):
        self._lib, self._p = lib, prefix
        self.model = model
        self.device_id = device_id
        self.dm = self.dz = 3 if model == MODEL_VICTORIAPARK_3D else 2
        self._borrowed = borrowed is not None
        self.gm_capacity = int(gm_capacity)
        if self._borrowed:          # a shard handle owned by an rfsgpu_group
            self._h = C.c_void_p(borrowed)
            return
        self._h = C.c_void_p()
        fn = self._fn("create_ex")
        fn.restype = C.c_int
        rc = fn(C.byref(self._h), C.c_int(model), C.c_int(int(n_particles)), C.c_int(device_id), C.c_int(gm_capacity),
                C.c_int(int(max_particles) if max_particles is not None else int(n_particles)))
        if rc != OK:
            self._h = C.c_void_p()
            raise EngineError(rc, "create failed (no gfx950 device / bad arguments)")

    @property
    def n(self):
        """nParticles_: the particle count NOW (the multi-hypothesis FastSLAM update and resample_apply_n change it)."""
        fn = self._fn("n_particles")
        fn.restype = C.c_int
        return fn(self._h)

    @property
    def max_particles(self):
        """The particle capacity the handle was created with (rfsgpu_create_ex)."""
        fn = self._fn("max_particles")
        fn.restype = C.c_int
        return fn(self._h)

    # -- plumbing ------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _call(self, name, *args):
        fn = self._fn(name)
        fn.restype = C.c_int
        rc = fn(self._h, *args)
        if rc != OK:
            le = self._fn("last_error")
            le.restype = C.c_char_p
            raise EngineError(rc, (le(self._h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = C.c_void_p()
            return
        if getattr(self, "_h", None) and self._h.value:
            d = self._fn("destroy")
            d.restype = None
            d(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    # -- configuration -------------------------------------------------------------------------
    def default_filter_config(self):
        cfg = FilterConfig()
        fn = self._fn("default_filter_config")
        fn.restype = None
        fn(C.byref(cfg))
        return cfg

    def set_filter_config(self, cfg):
        self._call("set_filter_config", C.byref(cfg))

    def get_filter_config(self):
        cfg = FilterConfig()
        self._call("get_filter_config", C.byref(cfg))
        return cfg

    # -- FastSLAM on the same handle (include/FastSLAM.hpp) -------------------------------------
    def default_fastslam_config(self):
        cfg = FastSlamConfig()
        fn = self._fn("default_fastslam_config")
        fn.restype = None
        fn(C.byref(cfg))
        return cfg

    def set_fastslam_config(self, cfg):
        self._call("set_fastslam_config", C.byref(cfg))

    def get_fastslam_config(self):
        cfg = FastSlamConfig()
        self._call("get_fastslam_config", C.byref(cfg))
        return cfg

    def vp_probe_pd(self, slot):
        """Probe: Pd and the near-limit flag of every Gaussian of particle `slot` (Victoria Park model), as the kernels see them."""
        n = int(self.gm_sizes()[slot])
        pd = np.empty(max(n, 1), dtype=np.float64)
        cl = np.empty(max(n, 1), dtype=np.int32)
        self._call("vp_probe_pd", C.c_int(int(slot)), self._ptr(pd), self._ptr(cl), C.c_int(n))
        return pd[:n], cl[:n].astype(bool)

    def fastslam_set_resample_occured(self, flag):
        self._call("fastslam_set_resample_occured", C.c_int(1 if flag else 0))

    def particle_parents(self):
        """Which slot each particle was copied from by the last (multi-hypothesis) fastslam_update."""
        n = self.n
        p = np.empty(n, dtype=np.int32)
        self._call("particle_parents", self._ptr(p), C.c_int(n))
        return p

    def fastslam_update(self, Z):
        """FastSLAM::updateMap for every particle (:387-418); resampleWithMapCopy stays with the caller."""
        Z = _f64(Z).reshape(-1, self.dz)
        self._call("fastslam_update", self._ptr(Z), C.c_int(Z.shape[0]))

    def fastslam_cycle_async(self, Z, u01, n_init, predict=False):
        """One whole FastSLAM::update (association, particle copies, correction, map management, resampleWithMapCopy) enqueued on the
        handle's stream; nothing is read back.  The particle count is the device's until the next call that synchronises."""
        Z = _f64(Z).reshape(-1, self.dz)
        self._call("fastslam_cycle_async", C.c_int(1 if predict else 0), self._ptr(Z), C.c_int(Z.shape[0]), C.c_double(float(u01)), C.c_int(int(n_init)))

    def fastslam_cycle_full_async(self, Z, u01, n_init, predict=False, scan=None):
        """fastslam_cycle_async for either model and any landmark candidate threshold (rfsgpu_fastslam_cycle_full_async); scan: the
        laser scan of this update (Victoria Park model), None leaves it as it is."""
        Z = _f64(Z).reshape(-1, self.dz)
        sp, ns = None, 0
        if scan is not None:
            scan = _f64(scan).reshape(-1)
            sp, ns = self._ptr(scan), scan.size
        self._call("fastslam_cycle_full_async", C.c_int(1 if predict else 0), self._ptr(Z), C.c_int(Z.shape[0]), sp, C.c_int(ns),
                   C.c_double(float(u01)), C.c_int(int(n_init)))

    def fastslam_cycle_counts(self):
        """(cycles with measurements completed, resamplings among them) of the device-cycle route; synchronises."""
        a, b = C.c_int(), C.c_int()
        self._call("fastslam_cycle_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    def debug_slot(self, slot, values=None):
        """[test] (weight, count, cand_count, first Gaussian [planes]) of any slot below max_particles; values: write them instead."""
        npl = 7 if self.dm == 2 else 11
        w, c, k = C.c_double(), C.c_int(), C.c_int()
        g = np.zeros(npl)
        if values is not None:
            w.value, c.value, k.value = float(values[0]), int(values[1]), int(values[2])
            g[:] = values[3]
        self._call("debug_slot", C.c_int(int(slot)), C.c_int(0 if values is None else 1), C.byref(w), C.byref(c), C.byref(k), self._ptr(g))
        return w.value, c.value, k.value, g

    def fastslam_cycle_pending(self):
        """Whether the particle count is still the device's (cycles are pending); waits for nothing."""
        fn = self._fn("fastslam_cycle_pending")
        fn.restype = C.c_int
        return bool(fn(self._h))

    def fastslam_last_cycle(self):
        """What the last fastslam_cycle_async did (synchronises): dict of n_after_update, n_after_resample, fired, n_eff, parent
        (slot -> the slot it was copied from by the update, over the grown set) and plan (slot -> the grown-set slot it now holds)."""
        cap = self.max_particles
        na, nr, fired, neff = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        parent = np.empty(cap, dtype=np.int32)
        plan = np.empty(cap, dtype=np.int32)
        self._call("fastslam_last_cycle", C.byref(na), C.byref(nr), C.byref(fired), C.byref(neff), self._ptr(parent), self._ptr(plan), C.c_int(cap))
        return {"n_after_update": na.value, "n_after_resample": nr.value, "fired": bool(fired.value), "n_eff": neff.value,
                "parent": parent[:na.value].copy(), "plan": plan[:nr.value].copy()}

    def fastslam_set_resampling(self, eff_n, eff_n_percent):
        """ParticleFilter::resample's two N_eff thresholds for fastslam_cycle_async."""
        self._call("fastslam_set_resampling", C.c_double(float(eff_n)), C.c_double(float(eff_n_percent)))

    def set_model_rngbrg(self, R, Pd, c, rmax, rmin, rbuf):
        m = RngBrgConfig()
        R = _f64(R, (4,))
        for k in range(4):
            m.R[k] = R[k]
        m.probabilityOfDetection, m.uniformClutterIntensity = Pd, c
        m.rangeLimMax, m.rangeLimMin, m.rangeLimBuffer = rmax, rmin, rbuf
        self._call("set_model_rngbrg", C.byref(m))

    def set_model_victoriapark(self, R, Slb, pd_table, expected_clutter, rmax, rmin, bmax, bmin, buffer_pd):
        m = VPConfig()
        R = _f64(R, (9,))
        for k in range(9):
            m.R[k] = R[k]
        m.Slb = Slb
        pd_table = list(pd_table)
        assert len(pd_table) <= VP_MAX_PD
        for k, v in enumerate(pd_table):
            m.PdTable[k] = v
        m.nPd = len(pd_table)
        m.expectedClutterNumber = expected_clutter
        m.rangeLimMax, m.rangeLimMin, m.bearingLimitMax, m.bearingLimitMin, m.bufferZonePd = rmax, rmin, bmax, bmin, buffer_pd
        self._call("set_model_victoriapark", C.byref(m))

    def set_laser_scan(self, scan):
        s = _f64(scan).reshape(-1)
        self._call("set_laser_scan", self._ptr(s), C.c_int(s.size))

    def export_birth_candidates(self, i):
        n = MAX_CANDIDATES
        mean, cov = np.empty((n, self.dm)), np.empty((n, self.dm, self.dm))
        sup, chk = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        nout = C.c_int()
        self._call("export_birth_candidates", C.c_int(i), C.c_int(n), C.byref(nout), self._ptr(mean), self._ptr(cov), self._ptr(sup), self._ptr(chk))
        k = min(nout.value, n)
        return mean[:k], cov[:k], sup[:k], chk[:k]

    def import_birth_candidates(self, i, mean, cov, sup, chk):
        sup = np.ascontiguousarray(sup, dtype=np.int32)
        k = sup.size
        mean = _f64(mean, (k, self.dm)) if k else np.zeros((0, self.dm))
        cov = _f64(cov, (k, self.dm, self.dm)) if k else np.zeros((0, self.dm, self.dm))
        chk = np.ascontiguousarray(chk, dtype=np.int32)
        self._call("import_birth_candidates", C.c_int(i), C.c_int(k), self._ptr(mean), self._ptr(cov), self._ptr(sup), self._ptr(chk))

    def set_kf_config(self, range_thr, bearing_thr):
        k = KFConfig(range_thr, bearing_thr)
        self._call("set_kf_config", C.byref(k))

    def set_lmk_process_noise(self, Q):
        self._call("set_lmk_process_noise", self._ptr(_f64(Q, (self.dm * self.dm,))))

    # -- particle state ------------------------------------------------------------------------
    def set_poses(self, x, cov=None):
        x = _f64(x, (self.n, 3))
        if cov is None:
            self._call("set_poses", self._ptr(x), C.c_void_p(), C.c_int(0))
        else:
            cov = _f64(cov)
            stride = 0 if cov.size == 9 else 9
            assert cov.size in (9, 9 * self.n)
            self._call("set_poses", self._ptr(x), self._ptr(cov), C.c_int(stride))

    def get_poses(self):
        x = np.empty((self.n, 3))
        self._call("get_poses", self._ptr(x))
        return x

    def set_weights(self, w):
        self._call("set_weights", self._ptr(_f64(w, (self.n,))))

    def get_weights(self):
        w = np.empty(self.n)
        self._call("get_weights", self._ptr(w))
        return w

    def get_pose_covs(self):
        """Every particle's pose covariance as the update reads it: [n, 3, 3] (rfsgpu_get_pose_covs)."""
        c = np.empty((self.n, 3, 3))
        self._call("get_pose_covs", self._ptr(c))
        return c

    # -- map access ----------------------------------------------------------------------------
    def getGMSize(self, i):
        fn = self._fn("gm_size")
        fn.restype = C.c_int
        return fn(self._h, C.c_int(i))

    def gm_sizes(self):
        s = np.empty(self.n, dtype=np.int32)
        self._call("gm_sizes", self._ptr(s))
        return s

    def getLandmark(self, i, m):
        mean = np.empty(self.dm)
        cov = np.empty((self.dm, self.dm))
        w = C.c_double()
        fn = self._fn("get_landmark")
        fn.restype = C.c_int
        rc = fn(self._h, C.c_int(i), C.c_int(m), self._ptr(mean), self._ptr(cov), C.byref(w))
        if rc != OK:
            return None
        return mean, cov, w.value

    def import_gm(self, i, w, mean, cov):
        w = _f64(w).reshape(-1)
        n = w.size
        mean = _f64(mean, (n, self.dm))
        cov = _f64(cov, (n, self.dm, self.dm))
        self._call("import_gm", C.c_int(i), C.c_int(n), self._ptr(w), self._ptr(mean), self._ptr(cov))

    def export_gm(self, i):
        n = max(self.getGMSize(i), 0)
        w, wp = np.empty(n), np.empty(n)
        mean, cov = np.empty((n, self.dm)), np.empty((n, self.dm, self.dm))
        nout = C.c_int()
        self._call("export_gm", C.c_int(i), C.c_int(n), C.byref(nout), self._ptr(w), self._ptr(wp), self._ptr(mean), self._ptr(cov))
        k = min(nout.value, n)
        return w[:k], wp[:k], mean[:k], cov[:k]

    def import_aux(self, i, unused_idx, n_in_fov):
        u = np.ascontiguousarray(unused_idx, dtype=np.int32)
        self._call("import_aux", C.c_int(i), self._ptr(u), C.c_int(u.size), C.c_int(int(n_in_fov)))

    # -- hot path ------------------------------------------------------------------------------
    def predict_map(self, add_birth=True):
        self._call("predict_map", C.c_int(1 if add_birth else 0))

    def _z(self, Z):
        Z = _f64(Z).reshape(-1, self.dz) if np.size(Z) else np.zeros((0, self.dz))
        return Z, C.c_int(Z.shape[0])

    def update(self, Z):
        Z, n = self._z(Z)
        self._call("update", self._ptr(Z), n)

    def update_map(self, Z):
        Z, n = self._z(Z)
        self._call("update_map", self._ptr(Z), n)

    def importance_weighting(self):
        self._call("importance_weighting")

    def merge(self):
        self._call("merge")

    def prune(self):
        self._call("prune")

    def get_unused(self, i):
        idx = np.empty(MAX_Z, dtype=np.int32)
        n = C.c_int()
        self._call("get_unused", C.c_int(i), self._ptr(idx), C.c_int(MAX_Z), C.byref(n))
        return idx[: n.value].copy()

    def landmarks_in_fov(self, i):
        n = C.c_int()
        self._call("landmarks_in_fov", C.c_int(i), C.byref(n))
        return n.value

    # -- weights / resampling ------------------------------------------------------------------
    def weight_sums(self):
        out = np.empty(2)
        self._call("weight_sums", self._ptr(out))
        return out

    def normalize_weights(self, total, sum_dev_ptr=None, n_parts=1):
        if n_parts == 1:
            self._call("normalize_weights", C.c_double(total), C.c_void_p(sum_dev_ptr))
        else:
            self._call("normalize_weights_parts", C.c_double(total), C.c_void_p(sum_dev_ptr), C.c_int(n_parts))

    def resample_apply(self, src_slot, n_out=None):
        """ParticleFilter::resample's copies; n_out < n shrinks the particle set (resample(n), ParticleFilter.hpp:417-483)."""
        s = np.ascontiguousarray(src_slot, dtype=np.int32)
        if n_out is None:
            assert s.size == self.n
            self._call("resample_apply", self._ptr(s))
        else:
            assert s.size == n_out
            self._call("resample_apply_n", self._ptr(s), C.c_int(int(n_out)))

    def resample_async(self, eff_n, eff_n_percent, u01, n_out=0, force=False, renormalize=False):
        """ParticleFilter::resample(n_out, force) enqueued on the handle's stream, nothing read back (rfsgpu_resample_async): u01 is the
        draw a resampling would use; renormalize asks for RBPHDFilter::update's second normalisation when the test does not fire."""
        self._call("resample_async", C.c_double(float(eff_n)), C.c_double(float(eff_n_percent)), C.c_double(float(u01)), C.c_int(int(n_out)),
                   C.c_int(1 if force else 0), C.c_int(1 if renormalize else 0))

    def last_resample(self):
        """What the last resample_async did (synchronises): dict of fired, n_eff, n_after and plan (slot -> the slot it now holds)."""
        cap = self.max_particles
        fired, neff, na = C.c_int(), C.c_double(), C.c_int()
        plan = np.empty(cap, dtype=np.int32)
        self._call("last_resample", C.byref(fired), C.byref(neff), C.byref(na), self._ptr(plan), C.c_int(cap))
        return {"fired": bool(fired.value), "n_eff": neff.value, "n_after": na.value, "plan": plan[:na.value].copy()}

    # the whole RBPHDFilter::update on the device (rfsgpu.h [rbphd-cycle])
    def rbphd_set_resampling(self, eff_n, eff_n_percent):
        """ParticleFilter::resample's two N_eff thresholds for rbphd_cycle_async."""
        self._call("rbphd_set_resampling", C.c_double(float(eff_n)), C.c_double(float(eff_n_percent)))

    def rbphd_cycle_async(self, Z, u01, scan=None):
        """One whole RBPHDFilter::update (the counters, the step, the gate, the resample-or-normalise tail) enqueued on the handle's
        stream; nothing is read back.  u01: the draw a resampling would use; scan: this update's laser scan (Victoria Park model),
        None leaves it as it is."""
        Z = _f64(Z).reshape(-1, self.dz)
        sp, ns = None, 0
        if scan is not None:
            scan = _f64(scan).reshape(-1)
            sp, ns = self._ptr(scan), scan.size
        self._call("rbphd_cycle_async", self._ptr(Z), C.c_int(Z.shape[0]), sp, C.c_int(ns), C.c_double(float(u01)))

    def rbphd_cycle_counts(self):
        """dict of n_cycles, n_gate_open, n_resamplings and max_level (the deepest inheritance level a walk on the device has met) of
        the device-cycle route; resolves."""
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._call("rbphd_cycle_counts", C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return {"n_cycles": a.value, "n_gate_open": b.value, "n_resamplings": c.value, "max_level": d.value}

    def rbphd_last_cycle(self):
        """What the last rbphd_cycle_async did (resolves): dict of gate_open, fired, n_eff, plan and walk_levels (the deepest level of
        the last inheritance walk made on the device)."""
        cap = self.max_particles
        gate, fired, neff, wl = C.c_int(), C.c_int(), C.c_double(), C.c_int()
        plan = np.empty(cap, dtype=np.int32)
        self._call("rbphd_last_cycle", C.byref(gate), C.byref(fired), C.byref(neff), self._ptr(plan), C.c_int(cap), C.byref(wl))
        return {"gate_open": bool(gate.value), "fired": bool(fired.value), "n_eff": neff.value, "plan": plan[:self.n].copy(), "walk_levels": wl.value}

    def rbphd_cycle_pending(self):
        """[test] whether cycles are pending (the ids and resampleOccured_ are the device's); waits for nothing."""
        fn = self._fn("rbphd_cycle_pending")
        fn.restype = C.c_int
        return bool(fn(self._h))

    # birth-state inheritance after a resampling (rfsgpu.h: RFSGPU_INHERIT_*; include/RBPHDFilter.hpp:1005-1011)
    def set_birth_inheritance(self, mode):
        self._call("set_birth_inheritance", C.c_int(int(mode)))

    def get_birth_inheritance(self):
        fn = self._fn("get_birth_inheritance")
        fn.restype = C.c_int
        return int(fn(self._h))

    def get_particle_ids(self):
        """(Particle::getId, Particle::getParentId) of the particle in every slot."""
        ids = np.zeros(self.n, dtype=np.int32)
        par = np.zeros(self.n, dtype=np.int32)
        self._call("get_particle_ids", self._ptr(ids), self._ptr(par))
        return ids, par

    def set_particle_ids(self, ids=None, parent_ids=None):
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        b = None if parent_ids is None else np.ascontiguousarray(parent_ids, dtype=np.int32)
        self._call("set_particle_ids", C.c_void_p(None) if a is None else self._ptr(a), C.c_void_p(None) if b is None else self._ptr(b))

    def resample_occured(self):
        fn = self._fn("resample_occured")
        fn.restype = C.c_int
        return bool(fn(self._h))

    def predict_map_level(self, add_birth, level_of_slot, level, do_static):
        lv = np.ascontiguousarray(level_of_slot, dtype=np.int32)
        assert lv.size == self.n
        self._call("predict_map_level", C.c_int(1 if add_birth else 0), self._ptr(lv), C.c_int(int(level)), C.c_int(1 if do_static else 0))

    def has_birth_candidates(self):
        """Has this handle ever held birth-candidate lists (rfsgpu_has_birth_candidates)?"""
        fn = self._fn("has_birth_candidates")
        fn.restype = C.c_int
        rc = fn(self._h)
        if rc < 0:
            raise EngineError(rc, "has_birth_candidates: null handle")
        return bool(rc)

    def murty_partition_sums(self, mats, nR, nC):
        """[test] Murty-200 sums of the given extended tables by the step's post kernel (rfsgpu_murty_partition_sums)."""
        flat = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.float64).ravel() for m in mats]))
        r = np.ascontiguousarray(nR, dtype=np.int32)
        c = np.ascontiguousarray(nC, dtype=np.int32)
        out = np.zeros(len(mats), dtype=np.float64)
        self._call("murty_partition_sums", self._ptr(flat), self._ptr(r), self._ptr(c), C.c_int(len(mats)), self._ptr(out))
        return out

    def partition_likelihoods(self, tables, pds, clutter):
        """[test] The weighting phase's partition stage on given likelihood tables (rfsgpu_partition_likelihoods): one number per
        table, the product over its visited partitions before the clutter-integral division."""
        tabs = [np.asarray(t, dtype=np.float64) for t in tables]
        assert all(t.ndim == 2 for t in tabs) and len(tabs) == len(pds)
        nE = np.ascontiguousarray([t.shape[0] for t in tabs], dtype=np.int32)
        nZ = np.ascontiguousarray([t.shape[1] for t in tabs], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([t.ravel() for t in tabs] + [np.zeros(1)]))
        pd = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in pds] + [np.zeros(1)]))
        assert pd.size == int(nE.sum()) + 1
        out = np.zeros(len(tabs), dtype=np.float64)
        self._call("partition_likelihoods", self._ptr(flat), self._ptr(pd), self._ptr(nE), self._ptr(nZ), C.c_int(len(tabs)), C.c_double(clutter),
                   self._ptr(out))
        return out

    def get_unused_masks(self):
        m = np.zeros(self.n, dtype=np.uint64)
        self._call("get_unused_masks", self._ptr(m))
        return m

    def set_unused_masks(self, masks):
        m = np.ascontiguousarray(masks, dtype=np.uint64)
        assert m.size == self.n
        self._call("set_unused_masks", self._ptr(m))

    def set_partition_mode(self, exact):
        """Partitions with nR + nC > 8: Murty-200 as the reference (False, default) or the exact subset recurrence (True)."""
        self._call("set_partition_mode", C.c_int(1 if exact else 0))

    # -- asynchronous host loop -----------------------------------------------------------------------------------
    def set_step_inputs_async(self, x=None, cov=None, scan=None):
        xp = cp = sp = C.c_void_p()
        stride, ns = 0, 0
        if x is not None:
            x = _f64(x, (self.n, 3))
            xp = self._ptr(x)
            if cov is not None:
                cov = _f64(cov)
                stride = 0 if cov.size == 9 else 9
                cp = self._ptr(cov)
        if scan is not None:
            scan = _f64(scan).reshape(-1)
            sp, ns = self._ptr(scan), scan.size
        self._call("set_step_inputs_async", xp, cp, C.c_int(stride), sp, C.c_int(ns))

    def set_phase_timing(self, on=True):
        """update() as three launches with per-phase TimingInfo / last_kernel_ns (True) or as one fused launch (False, default)."""
        self._call("set_phase_timing", C.c_int(1 if on else 0))

    def predict_map_async(self, add_birth=True):
        self._call("predict_map_async", C.c_int(1 if add_birth else 0))

    def static_steps_async(self, n, noises=None):
        """A run of n birth-less predicts (Sigma += Q_k each) in one launch; noises [n][D][D] or None = the current noise n times."""
        q = None
        if noises is not None:
            q = _f64(noises, (int(n), self.dm, self.dm))
        self._call("static_steps_async", C.c_int(int(n)), self._ptr(q) if q is not None else None)

    def propagate_ackerman_async(self, u, var, dt, geom, seed, call):
        """ParticleFilter::propagate with MotionModel_Ackerman2d on the device (csrc/motion.h); var None: noise-free."""
        up = (C.c_double * 2)(float(u[0]), float(u[1]))
        vp = (C.c_double * 2)(float(var[0]), float(var[1])) if var is not None else None
        gp = (C.c_double * 4)(*[float(g) for g in geom])
        self._call("propagate_ackerman_async", up, vp, C.c_double(float(dt)), gp, C.c_ulonglong(int(seed)), C.c_ulonglong(int(call)))

    def propagate_ackerman_run_async(self, u, var, dt, geom, seed, call0):
        """n propagations in one launch: u [n][2], var [n][2] or None, dt [n]."""
        u = _f64(u).reshape(-1, 2)
        n = u.shape[0]
        v = _f64(var, (n, 2)) if var is not None else None
        d = _f64(dt, (n,))
        gp = (C.c_double * 4)(*[float(g) for g in geom])
        self._call("propagate_ackerman_run_async", C.c_int(n), self._ptr(u), self._ptr(v) if v is not None else None, self._ptr(d), gp,
                   C.c_ulonglong(int(seed)), C.c_ulonglong(int(call0)))

    # -- cross-shard migration (packed rows in the backend's own memory space: device memory for the engine) ----------
    def slab_row_bytes(self):
        fn = self._fn("slab_row_bytes")
        fn.restype = C.c_size_t
        return int(fn(self._h))

    def export_slab_rows(self, slots, rows_ptr):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        self._call("export_slab_rows", self._ptr(s), C.c_int(s.size), C.c_void_p(rows_ptr))

    def import_slab_rows(self, slots, rows_ptr):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        self._call("import_slab_rows", self._ptr(s), C.c_int(s.size), C.c_void_p(rows_ptr))

    def weights_device_ptr(self):
        fn = self._fn("weights_device_ptr")
        fn.restype = C.c_void_p
        return fn(self._h)

    # -- [metric] per-step map error and pose error on the device (rfsgpu_step_error*, csrc/map_metric.h) ------------
    @property
    def n_metric_filters(self):
        """Records per row: the batch's filters, 1 for an ordinary handle."""
        return int(getattr(self, "n_filters", 1))

    def set_ground_truth(self, xy, first_seen=None, filter=0):
        """Filter `filter`'s ground-truth landmarks xy [n, 2] and the time each first came into sensor range (None: all -1)."""
        xy = _f64(xy).reshape(-1, 2)
        fs = None if first_seen is None else _f64(first_seen, (xy.shape[0],))
        self._call("set_ground_truth", C.c_int(int(filter)), self._ptr(xy), C.c_void_p(None) if fs is None else self._ptr(fs), C.c_int(xy.shape[0]))

    def error_log_create(self, log_capacity):
        self._call("error_log_create", C.c_int(int(log_capacity)))

    def error_log_reset(self):
        self._call("error_log_reset")

    def _metric_inputs(self, t, gt_pose):
        nF = self.n_metric_filters
        t = _f64(np.broadcast_to(np.asarray(t, dtype=np.float64), (nF,)))
        g = None if gt_pose is None else _f64(gt_pose, (nF, 3))
        return t, g

    def step_error_async(self, t, gt_pose=None, w_threshold=0.75, cutoff=0.20, order=1.0):
        """Append one row to the device-side log: t [n_filters] (or a scalar), gt_pose [n_filters, 3] or None (pose fields NaN); the
        defaults are the reference's constants (src/analysis2dSim.cpp:182, :232-233).  Stream-ordered, no host wait."""
        t, g = self._metric_inputs(t, gt_pose)
        self._call("step_error_async", self._ptr(t), C.c_void_p(None) if g is None else self._ptr(g), C.c_double(w_threshold), C.c_double(cutoff),
                   C.c_double(order))

    def error_log_read(self, max_rows=None):
        """The rows written so far as a structured array [rows, n_filters] (STEP_ERROR_DTYPE).  Synchronises; the log keeps its rows."""
        nF = self.n_metric_filters
        n = C.c_int()
        if max_rows is None:
            self._call("error_log_read", C.c_void_p(None), C.c_int(0), C.byref(n))
            max_rows = n.value
        out = np.zeros((int(max_rows), nF), dtype=STEP_ERROR_DTYPE)
        self._call("error_log_read", self._ptr(out), C.c_int(int(max_rows)), C.byref(n))
        return out[: min(n.value, int(max_rows))]

    def step_error(self, t, gt_pose=None, w_threshold=0.75, cutoff=0.20, order=1.0):
        """The synchronous form: this call's row [n_filters] (STEP_ERROR_DTYPE); needs no log."""
        t, g = self._metric_inputs(t, gt_pose)
        out = np.zeros(self.n_metric_filters, dtype=STEP_ERROR_DTYPE)
        self._call("step_error", self._ptr(t), C.c_void_p(None) if g is None else self._ptr(g), C.c_double(w_threshold), C.c_double(cutoff),
                   C.c_double(order), self._ptr(out))
        return out

    def get_map_estimate(self, w_threshold=0.75, filter=0):
        """(mean [n, 2], cov [n, 2, 2], w [n]) of the Gaussians with weight >= w_threshold of filter `filter`'s highest-weight particle."""
        n = C.c_int()
        self._call("get_map_estimate", C.c_int(int(filter)), C.c_double(w_threshold), C.c_int(0), C.byref(n), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None))
        k = n.value
        mean, cov, w = np.empty((k, 2)), np.empty((k, 2, 2)), np.empty(k)
        self._call("get_map_estimate", C.c_int(int(filter)), C.c_double(w_threshold), C.c_int(k), C.byref(n), self._ptr(mean), self._ptr(cov), self._ptr(w))
        k = min(k, n.value)
        return mean[:k], cov[:k], w[:k]

    # -- [estimate] per-step pose and map estimates in a device-side log (rfsgpu_step_estimate*, csrc/estimate_log.h) ------------
    @property
    def n_estimate_slots(self):
        """Slots per particle plane of the estimate log: max_per_filter, n_per_filter (a Victoria Park batch included), or the particle
        count of an ordinary handle."""
        if getattr(self, "_est_served", False):
            return int(self.max_particles)
        return int(getattr(self, "max_per_filter", getattr(self, "n_per_filter", None) or self.n))

    def handle_serve_estimates(self, on=True):
        """rfsgpu_handle_serve_estimates (synchronising): the estimate log calls serve this ordinary handle -- the Victoria Park model and
        FastSLAM handles included -- and step_estimate_async goes behind pending device cycles without resolving them.  Off frees the
        log and restores the refusals."""
        self._call("handle_serve_estimates", C.c_int(1 if on else 0))
        self._est_served = bool(on)
        if not on:
            self._est_shape = None

    def estimate_log_create(self, log_capacity, max_est, log_particles=False):
        """The device-side estimate log: log_capacity rows, max_est Gaussians kept per filter and row, the particle set too with
        log_particles.  Capacity 0 frees it."""
        slots = self.n_estimate_slots if log_particles else 0
        self._call("estimate_log_create", C.c_int(int(log_capacity)), C.c_int(int(max_est)), C.c_int(1 if log_particles else 0))
        self._est_shape = (int(max_est), slots) if int(log_capacity) > 0 else None

    def estimate_log_reset(self):
        self._call("estimate_log_reset")

    def step_estimate_async(self, t, w_threshold=0.75):
        """Append one row to the estimate log: t [n_filters] (or a scalar); w_threshold -inf keeps every Gaussian of the best particle.
        Stream-ordered, no host wait."""
        t, _ = self._metric_inputs(t, None)
        self._call("step_estimate_async", self._ptr(t), C.c_double(w_threshold))

    def estimate_log_read(self, row_from=0, max_rows=None):
        """(hdr, gauss, part): the rows [row_from, row_from + max_rows) that exist (None: all from row_from) -- hdr a structured array
        [rows, n_filters] (STEP_ESTIMATE_DTYPE), gauss [rows, n_filters, 6, max_est] (ESTIMATE_GAUSS_PLANES), part
        [rows, n_filters, 4, slots] (ESTIMATE_PART_PLANES; None for a log without particles).  Gaussians at or beyond a header's n_logged
        and particles at or beyond its n_particles are not the log's: they come back as zeros.  Synchronises; the log keeps its rows."""
        nF = self.n_metric_filters
        max_est, slots = getattr(self, "_est_shape", None) or (0, 0)
        n = C.c_int()
        null = C.c_void_p(None)
        self._call("estimate_log_read", C.c_int(int(row_from)), C.c_int(0), null, null, null, C.byref(n))
        rows = max(0, n.value - int(row_from))
        if max_rows is not None:
            rows = min(rows, int(max_rows))
        hdr = np.zeros((rows, nF), dtype=STEP_ESTIMATE_DTYPE)
        gauss = np.zeros((rows, nF, 6, max_est))
        part = np.zeros((rows, nF, 4, slots)) if slots else None
        self._call("estimate_log_read", C.c_int(int(row_from)), C.c_int(rows), self._ptr(hdr), self._ptr(gauss) if max_est else null,
                   self._ptr(part) if part is not None else null, C.byref(n))
        # what the kernel did not write (Gaussians beyond n_logged, particles beyond n_particles) is uninitialised device memory: zeros here
        if max_est:
            np.copyto(gauss, 0.0, where=(np.arange(max_est) >= hdr["n_logged"][..., None])[:, :, None, :])
        if part is not None:
            np.copyto(part, 0.0, where=(np.arange(slots) >= hdr["n_particles"][..., None])[:, :, None, :])
        return hdr, gauss, part

    # -- timing --------------------------------------------------------------------------------
    def getTimingInfo(self):
        t = Timing()
        self._call("get_timing", C.byref(t))
        return t

    def reset_timing(self):
        self._call("reset_timing")

    def synchronize(self):
        self._call("synchronize")


class CBatch(CFilter):
    """A filter batch behind the C ABI ([batch] in include/rfsgpu.h): n_filters independent 2-D filters of n_per_filter particles in one
    handle, filter b in the global slots [b * n_per_filter, (b + 1) * n_per_filter).  Every per-slot method of CFilter works on it."""

    MODELS = (MODEL_RNGBRG_2D,)      # what this class steps (CVPBatch: the Victoria Park model)

    def __init__(self, lib, prefix, n_filters, n_per_filter, model=MODEL_RNGBRG_2D, device_id=0, gm_capacity=512):
        self._lib, self._p = lib, prefix
        self.model = model
        self.device_id = device_id
        self.dm = self.dz = 3 if model == MODEL_VICTORIAPARK_3D else 2
        self._borrowed = False
        self._h = C.c_void_p()
        if model not in self.MODELS:
            raise EngineError(ERR_UNSUPPORTED, "create_batch: this class steps 2-D range-bearing filters; a batch of Victoria Park filters is a CVPBatch "
                                               "(engine.VPFilterBatch), whose cycle is rfsgpu_batch_vp_cycle_async" if model == MODEL_VICTORIAPARK_3D
                              else "create_batch: this class steps Victoria Park filters only")
        fn = self._fn("create_batch")
        fn.restype = C.c_int
        rc = fn(C.byref(self._h), C.c_int(model), C.c_int(int(n_filters)), C.c_int(int(n_per_filter)), C.c_int(device_id), C.c_int(gm_capacity))
        if rc != OK:
            self._h = C.c_void_p()
            raise EngineError(rc, "create_batch failed: no gfx950 device / bad arguments")
        self.n_filters = int(n_filters)
        self.n_per_filter = int(n_per_filter)
        self.gm_capacity = int(gm_capacity)

    def block(self, b):
        """The global slots of filter b."""
        return slice(b * self.n_per_filter, (b + 1) * self.n_per_filter)

    def batch_configure(self, b, cfg=None, R=None, Pd=None, clutter=None, rmax=None, rmin=None, rbuf=None, kf=None, Q=None):
        """Filter b's configuration: cfg a FilterConfig; the range-bearing model (R, Pd, clutter, rmax, rmin, rbuf: all or none);
        kf = (range_thr, bearing_thr); Q the 2x2 landmark process noise.  What is None stays."""
        m = None
        if R is not None:
            m = RngBrgConfig()
            R = _f64(R, (4,))
            for k in range(4):
                m.R[k] = R[k]
            m.probabilityOfDetection, m.uniformClutterIntensity = Pd, clutter
            m.rangeLimMax, m.rangeLimMin, m.rangeLimBuffer = rmax, rmin, rbuf
        k = None if kf is None else KFConfig(*kf)
        q = None if Q is None else _f64(Q, (4,))
        self._call("batch_configure", C.c_int(int(b)), C.c_void_p(None) if cfg is None else C.byref(cfg), C.c_void_p(None) if m is None else C.byref(m),
                   C.c_void_p(None) if k is None else C.byref(k), C.c_void_p(None) if q is None else self._ptr(q))

    def _cycle_call(self, name, predict, Zs, poses, pose_cov, normalize):
        """The two cycle calls share one argument layout: the sets packed as z [n_filters, MAX_Z, 2] / nz [n_filters]."""
        assert len(Zs) == self.n_filters
        z = np.zeros((self.n_filters, MAX_Z, 2))
        nz = np.zeros(self.n_filters, dtype=np.int32)
        for b, Z in enumerate(Zs):
            Z = _f64(Z).reshape(-1, 2) if np.size(Z) else np.zeros((0, 2))
            nz[b] = Z.shape[0]
            z[b, : min(Z.shape[0], MAX_Z)] = Z[:MAX_Z]
        x = None if poses is None else _f64(poses, (self.n, 3))
        stride = 0
        cv = None
        if pose_cov is not None:
            cv = _f64(pose_cov)
            assert cv.size in (9, 9 * self.n)
            stride = 0 if cv.size == 9 else 9
        self._call(name, C.c_int(-1 if predict is None else (1 if predict else 0)), C.c_void_p(None) if x is None else self._ptr(x),
                   C.c_void_p(None) if cv is None else self._ptr(cv), C.c_int(stride), self._ptr(z), self._ptr(nz), C.c_int(1 if normalize else 0))

    def batch_cycle_async(self, predict, Zs, poses=None, pose_cov=None, normalize=True):
        """rfsgpu_batch_cycle_async: Zs = one measurement array per filter ([n_z, 2], possibly empty); predict None / False / True as
        rfsgpu_cycle_async."""
        self._cycle_call("batch_cycle_async", predict, Zs, poses, pose_cov, normalize)

    def batch_cycle_async_packed(self, predict, z, nz, normalize=True):
        """rfsgpu_batch_cycle_async with the sets already in the call's layout (z [n_filters, MAX_Z, 2] float64, nz [n_filters] int32,
        both C-contiguous) and no new poses: what a loop that packs its measurement sets once issues per step."""
        assert z.dtype == np.float64 and nz.dtype == np.int32 and z.shape == (self.n_filters, MAX_Z, 2) and z.flags.c_contiguous and nz.flags.c_contiguous
        self._call("batch_cycle_async", C.c_int(-1 if predict is None else (1 if predict else 0)), C.c_void_p(None), C.c_void_p(None), C.c_int(0),
                   self._ptr(z), self._ptr(nz), C.c_int(1 if normalize else 0))

    # -- a batch of FastSLAM filters ------------------------------------------------------------------------------------------
    def batch_set_fastslam_config(self, b, cfg):
        """rfsgpu_batch_set_fastslam_config: filter b's (None: every filter's) FastSlamConfig."""
        self._call("batch_set_fastslam_config", C.c_int(-1 if b is None else int(b)), C.byref(cfg))

    def batch_fastslam_cycle_async(self, predict, Zs, poses=None, pose_cov=None, normalize=True):
        """rfsgpu_batch_fastslam_cycle_async: arguments as batch_cycle_async (predict None: no static landmark step)."""
        self._cycle_call("batch_fastslam_cycle_async", predict, Zs, poses, pose_cov, normalize)

    def batch_fastslam_cycle_async_packed(self, predict, z, nz, normalize=True):
        """rfsgpu_batch_fastslam_cycle_async with the sets already in the call's layout and no new poses (as batch_cycle_async_packed)."""
        assert z.dtype == np.float64 and nz.dtype == np.int32 and z.shape == (self.n_filters, MAX_Z, 2) and z.flags.c_contiguous and nz.flags.c_contiguous
        self._call("batch_fastslam_cycle_async", C.c_int(-1 if predict is None else (1 if predict else 0)), C.c_void_p(None), C.c_void_p(None), C.c_int(0),
                   self._ptr(z), self._ptr(nz), C.c_int(1 if normalize else 0))

    def batch_weight_sums(self):
        out = np.empty((self.n_filters, 2))
        self._call("batch_weight_sums", self._ptr(out))
        return out

    def batch_resample_apply(self, src_slot, resampled):
        s = np.ascontiguousarray(src_slot, dtype=np.int32)
        r = np.ascontiguousarray(resampled, dtype=np.uint8)
        assert s.size == self.n and r.size == self.n_filters
        self._call("batch_resample_apply", self._ptr(s), self._ptr(r))

    def batch_resample_occured(self):
        out = np.zeros(self.n_filters, dtype=np.uint8)
        fn = self._fn("batch_resample_occured")
        fn.restype = C.c_int
        fn(self._h, self._ptr(out))
        return out.astype(bool)

    # -- the device loop ([batch] in include/rfsgpu.h: propagation and resampling without the host) ---------------------------
    def set_motion_odometry(self, b, var, seed):
        """rfsgpu_batch_set_motion_odometry: filter b's (None: every filter's) process noise N(0, diag(var)) and Philox key."""
        v = _f64(var, (3,))
        self._call("batch_set_motion_odometry", C.c_int(-1 if b is None else int(b)), self._ptr(v), C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_resampling(self, b, eff_n, eff_n_percent):
        """rfsgpu_batch_set_resampling: ParticleFilter::resample's two thresholds for filter b (None: every filter)."""
        self._call("batch_set_resampling", C.c_int(-1 if b is None else int(b)), C.c_double(float(eff_n)), C.c_double(float(eff_n_percent)))

    def propagate_async(self, u, call, pin=None, pin_pose=None):
        """rfsgpu_batch_propagate_async: u [n_filters, 3]; pin [n_filters] bool and pin_pose [n_filters, 3], or None."""
        u = _f64(u, (self.n_filters, 3))
        pn = None if pin is None else np.ascontiguousarray(pin, dtype=np.uint8).reshape(self.n_filters)
        pp = None if pin_pose is None else _f64(pin_pose, (self.n_filters, 3))
        self._call("batch_propagate_async", self._ptr(u), C.c_void_p(None) if pp is None else self._ptr(pp),
                   C.c_void_p(None) if pn is None else self._ptr(pn), C.c_ulonglong(int(call)))

    def resample_async(self, n_z, call):
        """rfsgpu_batch_resample_async: n_z [n_filters] the cycle's measurement counts."""
        nz = np.ascontiguousarray(n_z, dtype=np.int32).reshape(self.n_filters)
        self._call("batch_resample_async", self._ptr(nz), C.c_ulonglong(int(call)))

    def last_resample(self):
        """(fired [n_filters] bool, plan [N] global source slots, n_eff [n_filters]) of the last resample_async (synchronising)."""
        fired = np.zeros(self.n_filters, dtype=np.uint8)
        plan = np.zeros(self.n, dtype=np.int32)
        neff = np.zeros(self.n_filters)
        self._call("batch_last_resample", self._ptr(fired), self._ptr(plan), self._ptr(neff))
        return fired.astype(bool), plan, neff

    def get_pose_covs(self):
        """Every slot's pose covariance [N, 3, 3] as the next update reads it (synchronising)."""
        out = np.zeros((self.n, 9))
        self._call("batch_get_pose_covs", self._ptr(out))
        return out.reshape(self.n, 3, 3)

    def resample_counts(self):
        """Resamplings per filter by resample_async so far (synchronising)."""
        out = np.zeros(self.n_filters, dtype=np.int64)
        self._call("batch_resample_counts", self._ptr(out))
        return out

    # -- the device sensor ([sensor] in include/rfsgpu.h: every filter's scan drawn on the device) -----------------------------
    def set_sensor(self, b, R, Pd, clutter, rmax, rmin, landmarks, max_nz=MAX_Z, seed=0):
        """rfsgpu_batch_set_sensor: filter b's (None: every filter's) simulated sensor -- ITS noise R [2, 2], Pd, clutter intensity and
        range limits -- the landmarks [n, 2] it sees, the largest set it may deliver and its Philox key."""
        m = RngBrgConfig()
        R = _f64(R, (4,))
        for k in range(4):
            m.R[k] = R[k]
        m.probabilityOfDetection, m.uniformClutterIntensity = float(Pd), float(clutter)
        m.rangeLimMax, m.rangeLimMin, m.rangeLimBuffer = float(rmax), float(rmin), 0.0
        lm = _f64(landmarks).reshape(-1, 2) if np.size(landmarks) else np.zeros((0, 2))
        self._call("batch_set_sensor", C.c_int(-1 if b is None else int(b)), C.byref(m), self._ptr(lm) if len(lm) else C.c_void_p(None), C.c_int(len(lm)),
                   C.c_int(int(max_nz)), C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF))

    def sense_async(self, gt_pose, call):
        """rfsgpu_batch_sense_async: gt_pose [n_filters, 3]; every filter's scan of call `call` is drawn on the device."""
        g = _f64(gt_pose, (self.n_filters, 3))
        self._call("batch_sense_async", self._ptr(g), C.c_ulonglong(int(call)))

    def cycle_sensed_async(self, predict, poses=None, pose_cov=None, normalize=True):
        """rfsgpu_batch_cycle_sensed_async: batch_cycle_async on the sets the last sense_async left on the device."""
        x = None if poses is None else _f64(poses, (self.n, 3))
        stride = 0
        cv = None
        if pose_cov is not None:
            cv = _f64(pose_cov)
            assert cv.size in (9, 9 * self.n)
            stride = 0 if cv.size == 9 else 9
        self._call("batch_cycle_sensed_async", C.c_int(-1 if predict is None else (1 if predict else 0)), C.c_void_p(None) if x is None else self._ptr(x),
                   C.c_void_p(None) if cv is None else self._ptr(cv), C.c_int(stride), C.c_int(1 if normalize else 0))

    def resample_sensed_async(self, call):
        """rfsgpu_batch_resample_sensed_async: resample_async with the measurement counts the device holds."""
        self._call("batch_resample_sensed_async", C.c_ulonglong(int(call)))

    def serve_sensor(self, on=True):
        """rfsgpu_batch_fastslam_serve_sensor (synchronising): from now on set_sensor, sense_async, last_scan and run_truth_async serve
        this batch of FastSLAM filters (or, on a CBatchMH, of multi-hypothesis FastSLAM filters), resample_sensed_async a FastSLAM
        batch; on=False: they refuse again (refused itself once a sensed cycle has run)."""
        self._call("batch_fastslam_serve_sensor", C.c_int(1 if on else 0))

    def _pose_args(self, poses, pose_cov):
        """(x, x_cov, cov_stride) of a cycle call as ctypes arguments; the arrays ride along so that they outlive the call."""
        x = None if poses is None else _f64(poses, (self.n, 3))
        stride = 0
        cv = None
        if pose_cov is not None:
            cv = _f64(pose_cov)
            assert cv.size in (9, 9 * self.n)
            stride = 0 if cv.size == 9 else 9
        return C.c_void_p(None) if x is None else self._ptr(x), C.c_void_p(None) if cv is None else self._ptr(cv), C.c_int(stride), (x, cv)

    def fastslam_cycle_sensed_async(self, predict, poses=None, pose_cov=None, normalize=True):
        """rfsgpu_batch_fastslam_cycle_sensed_async: batch_fastslam_cycle_async on the sets the last sense_async left on the device."""
        px, pc, stride, keep = self._pose_args(poses, pose_cov)
        self._call("batch_fastslam_cycle_sensed_async", C.c_int(-1 if predict is None else (1 if predict else 0)), px, pc, stride, C.c_int(1 if normalize else 0))

    def last_scan(self):
        """The sets of the last sense_async as a list of [n_z, 2] arrays, one per filter (synchronising)."""
        z = np.zeros((self.n_filters, MAX_Z, 2))
        nz = np.zeros(self.n_filters, dtype=np.int32)
        try:
            self._call("batch_last_scan", self._ptr(z), self._ptr(nz))
        except EngineError as e:
            e.scans = [z[b, : nz[b]].copy() for b in range(self.n_filters)]      # (a scan that was cut: the sets as delivered ride on the error)
            raise
        return [z[b, : nz[b]].copy() for b in range(self.n_filters)]

    # -- the device truth ([truth] in include/rfsgpu.h: trajectory, odometry and landmarks drawn on the device; a run in one call) ----
    def set_truth(self, b, cfg, seed):
        """rfsgpu_batch_set_truth: filter b's (None: every filter's) TruthConfig and Philox key for the next generate_truth."""
        self._call("batch_set_truth", C.c_int(-1 if b is None else int(b)), C.c_void_p(None) if cfg is None else C.byref(cfg),
                   C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF))

    def generate_truth(self, n_steps):
        """rfsgpu_batch_generate_truth: n_steps rows of every filter's truth in one launch (synchronous); earlier tables are replaced."""
        self._call("batch_generate_truth", C.c_int(int(n_steps)))
        self.truth_steps = int(n_steps)

    def get_truth(self, b, trajectory=True):
        """rfsgpu_batch_get_truth: filter b's tables as a dict -- landmarks [L, 2], first_seen [L], n_det_max, K and, unless
        trajectory=False, gt [K, 3] and odom [K, 3] (else None).  Synchronising."""
        K = int(getattr(self, "truth_steps", 0))
        gt = np.zeros((K, 3)) if trajectory else None
        od = np.zeros((K, 3)) if trajectory else None
        lm = np.zeros((SENSOR_MAX_LANDMARKS, 2))
        fs = np.zeros(SENSOR_MAX_LANDMARKS)
        n, nd = C.c_int(0), C.c_int(0)
        self._call("batch_get_truth", C.c_int(int(b)), C.c_void_p(None) if gt is None else self._ptr(gt), C.c_void_p(None) if od is None else self._ptr(od),
                   self._ptr(lm), self._ptr(fs), C.byref(n), C.byref(nd))
        return dict(gt=gt, odom=od, landmarks=lm[: n.value].copy(), first_seen=fs[: n.value].copy(), n_det_max=int(nd.value), K=K, Z=None)

    def run_truth_async(self, k_from, k_to, track_errors=False, w_threshold=0.75, cutoff=0.20, order=1.0):
        """rfsgpu_batch_run_truth_async: the steps k_from ... k_to - 1 of the device loop with the device sensor, their inputs read from
        the truth tables; enqueued in one call, nothing waits for the GPU."""
        self._call("batch_run_truth_async", C.c_int(int(k_from)), C.c_int(int(k_to)), C.c_int(1 if track_errors else 0), C.c_double(w_threshold),
                   C.c_double(cutoff), C.c_double(order))

    def run_log_estimates(self, on=True, w_threshold=0.75):
        """rfsgpu_batch_run_log_estimates: while on, every step of run_truth_async appends one row to the estimate log
        (estimate_log_create), taken where the step's error row is taken."""
        self._call("batch_run_log_estimates", C.c_int(1 if on else 0), C.c_double(w_threshold))

    def last_cycle_lds(self):
        """Bytes of LDS a workgroup of the step kernel had in the batch's last cycle (0 before the first)."""
        out = C.c_longlong(0)
        self._call("batch_last_cycle_lds", C.byref(out))
        return int(out.value)

    def n_filters_abi(self):
        fn = self._fn("n_filters")
        fn.restype = C.c_int
        return int(fn(self._h))


def vp_config(R, Slb, pd_table, expected_clutter, rmax, rmin, bmax, bmin, buffer_pd):
    """A VPConfig from the arguments of CFilter.set_model_victoriapark."""
    m = VPConfig()
    R = _f64(R, (9,))
    for k in range(9):
        m.R[k] = R[k]
    m.Slb = Slb
    pd_table = list(pd_table)
    assert len(pd_table) <= VP_MAX_PD
    for k, v in enumerate(pd_table):
        m.PdTable[k] = v
    m.nPd = len(pd_table)
    m.expectedClutterNumber = expected_clutter
    m.rangeLimMax, m.rangeLimMin, m.bearingLimitMax, m.bearingLimitMin, m.bufferZonePd = rmax, rmin, bmax, bmin, buffer_pd
    return m


class CVPBatch(CBatch):
    """A batch of Victoria Park RB-PHD filters behind the C ABI (rfsgpu_create_batch with the Victoria Park model,
    rfsgpu_batch_configure_vp, rfsgpu_batch_vp_cycle_async): filter b in the global slots [b * n_per_filter, (b + 1) * n_per_filter), one
    laser scan for the handle, everything else per filter.  The per-slot methods of CFilter, set_laser_scan, set_lmk_process_noise,
    static_steps_async, batch_weight_sums, batch_resample_apply and batch_resample_occured work on it; the 2-D batch calls refuse."""

    MODELS = (MODEL_VICTORIAPARK_3D,)

    def __init__(self, lib, prefix, n_filters, n_per_filter, device_id=0, gm_capacity=512):
        super().__init__(lib, prefix, n_filters, n_per_filter, model=MODEL_VICTORIAPARK_3D, device_id=device_id, gm_capacity=gm_capacity)

    def batch_configure_vp(self, b, cfg=None, model=None, kf=None, Q=None):
        """Filter b's configuration: cfg a FilterConfig (any birth thresholds); model a VPConfig (vp_config) or the tuple of its
        arguments; kf = (range_thr, bearing_thr); Q the 3x3 landmark process noise.  What is None stays."""
        m = model if (model is None or isinstance(model, VPConfig)) else vp_config(*model)
        k = None if kf is None else KFConfig(*kf)
        q = None if Q is None else _f64(Q, (9,))
        self._call("batch_configure_vp", C.c_int(int(b)), C.c_void_p(None) if cfg is None else C.byref(cfg), C.c_void_p(None) if m is None else C.byref(m),
                   C.c_void_p(None) if k is None else C.byref(k), C.c_void_p(None) if q is None else self._ptr(q))

    def batch_vp_cycle_async(self, predict, Zs, poses=None, pose_cov=None, scan=None, normalize=True, name="batch_vp_cycle_async"):
        """rfsgpu_batch_vp_cycle_async: Zs = one measurement array per filter ([n_z, 3], possibly empty); predict None / False / True as
        rfsgpu_cycle_async; scan: the laser scan that goes with the sets (None: the one the handle holds)."""
        assert len(Zs) == self.n_filters
        z = np.zeros((self.n_filters, MAX_Z, 3))
        nz = np.zeros(self.n_filters, dtype=np.int32)
        for b, Z in enumerate(Zs):
            Z = _f64(Z).reshape(-1, 3) if np.size(Z) else np.zeros((0, 3))
            nz[b] = Z.shape[0]
            z[b, : min(Z.shape[0], MAX_Z)] = Z[:MAX_Z]
        self.batch_vp_cycle_async_packed(predict, z, nz, poses=poses, pose_cov=pose_cov, scan=scan, normalize=normalize, name=name)

    # -- a batch of Victoria Park FastSLAM filters (rfsgpu_batch_vp_serve_fastslam) ---------------------------------------------
    def batch_vp_serve_fastslam(self, on=True):
        """rfsgpu_batch_vp_serve_fastslam: the batch steps single-hypothesis FastSLAM filters from here on (batch_set_fastslam_config,
        batch_vp_fastslam_cycle_async); refused once a cycle of the other kind has run."""
        self._call("batch_vp_serve_fastslam", C.c_int(1 if on else 0))

    def batch_vp_fastslam_cycle_async(self, predict, Zs, poses=None, pose_cov=None, scan=None, normalize=True):
        """rfsgpu_batch_vp_fastslam_cycle_async: the arguments of batch_vp_cycle_async; predict None (RFSGPU_CYCLE_NO_PREDICT) or
        False / True (the static landmark step with each filter's own Q; FastSLAM has no births)."""
        self.batch_vp_cycle_async(predict, Zs, poses=poses, pose_cov=pose_cov, scan=scan, normalize=normalize, name="batch_vp_fastslam_cycle_async")

    def batch_vp_fastslam_cycle_async_packed(self, predict, z, nz, poses=None, pose_cov=None, scan=None, normalize=True):
        self.batch_vp_cycle_async_packed(predict, z, nz, poses=poses, pose_cov=pose_cov, scan=scan, normalize=normalize, name="batch_vp_fastslam_cycle_async")

    def batch_vp_cycle_async_packed(self, predict, z, nz, poses=None, pose_cov=None, scan=None, normalize=True, name="batch_vp_cycle_async"):
        """The same with the sets already in the call's layout (z [n_filters, MAX_Z, 3] float64, nz [n_filters] int32, C-contiguous).
        name: the cycle call (rfsgpu_batch_vp_fastslam_cycle_async has the same argument list)."""
        assert z.dtype == np.float64 and nz.dtype == np.int32 and z.shape == (self.n_filters, MAX_Z, 3) and z.flags.c_contiguous and nz.flags.c_contiguous
        x = None if poses is None else _f64(poses, (self.n, 3))
        stride = 0
        cv = None
        if pose_cov is not None:
            cv = _f64(pose_cov)
            assert cv.size in (9, 9 * self.n)
            stride = 0 if cv.size == 9 else 9
        s = None if scan is None else _f64(scan).reshape(-1)
        self._call(name, C.c_int(-1 if predict is None else (1 if predict else 0)), C.c_void_p(None) if x is None else self._ptr(x),
                   C.c_void_p(None) if cv is None else self._ptr(cv), C.c_int(stride), self._ptr(z), self._ptr(nz),
                   C.c_void_p(None) if s is None else self._ptr(s), C.c_int(0 if s is None else s.size), C.c_int(1 if normalize else 0))

    # -- the device route ([batch] in include/rfsgpu.h: a run of messages without a stop on the host) --------------------------
    def batch_vp_set_motion(self, b, var, geom, seed):
        """rfsgpu_batch_vp_set_motion: filter b's (None: every filter's) input-noise variances (speed, steering), the vehicle geometry
        (h, l, dx, dy) and its Philox key."""
        v, g = _f64(var, (2,)), _f64(geom, (4,))
        self._call("batch_vp_set_motion", C.c_int(-1 if b is None else int(b)), self._ptr(v), self._ptr(g), C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF))

    def batch_vp_set_resampling(self, b, eff_n, eff_n_percent):
        """rfsgpu_batch_vp_set_resampling: ParticleFilter::resample's two thresholds for filter b (None: every filter)."""
        self._call("batch_vp_set_resampling", C.c_int(-1 if b is None else int(b)), C.c_double(float(eff_n)), C.c_double(float(eff_n_percent)))

    def batch_vp_propagate_run_async(self, u, dt, call0, noisy=None):
        """rfsgpu_batch_vp_propagate_run_async: u [n, 2], dt [n], noisy [n] bool (None: every step is noisy); calls call0, call0 + 1, ..."""
        u = _f64(u).reshape(-1, 2)
        dt = _f64(dt).reshape(-1)
        assert u.shape[0] == dt.shape[0]
        ny = None if noisy is None else np.ascontiguousarray(noisy, dtype=np.uint8).reshape(dt.shape[0])
        self._call("batch_vp_propagate_run_async", C.c_int(dt.shape[0]), self._ptr(u), C.c_void_p(None) if ny is None else self._ptr(ny), self._ptr(dt),
                   C.c_ulonglong(int(call0)))

    def batch_vp_resample_async(self, n_z, call):
        """rfsgpu_batch_vp_resample_async: n_z [n_filters] the cycle's measurement counts."""
        nz = np.ascontiguousarray(n_z, dtype=np.int32).reshape(self.n_filters)
        self._call("batch_vp_resample_async", self._ptr(nz), C.c_ulonglong(int(call)))

    def batch_vp_last_resample(self):
        """(fired [n_filters] bool, plan [N] global source slots, n_eff [n_filters]) of the last batch_vp_resample_async (synchronising)."""
        fired = np.zeros(self.n_filters, dtype=np.uint8)
        plan = np.zeros(self.n, dtype=np.int32)
        neff = np.zeros(self.n_filters)
        self._call("batch_vp_last_resample", self._ptr(fired), self._ptr(plan), self._ptr(neff))
        return fired.astype(bool), plan, neff

    def batch_vp_loop_counts(self):
        """(resamplings [n_filters], the deepest inheritance level any walk on the device has met) (synchronising)."""
        out = np.zeros(self.n_filters, dtype=np.int64)
        lv = C.c_int(0)
        self._call("batch_vp_loop_counts", self._ptr(out), C.byref(lv))
        return out, int(lv.value)

    def serve_estimates(self, on=True):
        """rfsgpu_batch_vp_serve_estimates (synchronising): estimate_log_create / _reset / _read and step_estimate_async serve this batch on
        both routes -- one row per call and filter, a Victoria Park handle's row with best_slot a global slot; step_estimate_async waits
        for nothing.  Off frees the log and restores the refusals."""
        self._call("batch_vp_serve_estimates", C.c_int(1 if on else 0))
        if not on:
            self._est_shape = None


class CBatchMH(CBatch):
    """A batch of multi-hypothesis FastSLAM filters behind the C ABI (rfsgpu_create_batch_mh): filter b owns the global slots
    [b * max_per_filter, (b + 1) * max_per_filter), of which the first live_counts()[b] are live; n_per_filter is the count a filter
    starts with and returns to at a resampling.  Slots beyond a filter's count hold nothing meaningful."""

    def __init__(self, lib, prefix, n_filters, n_per_filter, max_per_filter, model=MODEL_RNGBRG_2D, device_id=0, gm_capacity=512):
        self._lib, self._p = lib, prefix
        self.model = model
        self.device_id = device_id
        self.dm = self.dz = 2
        self._borrowed = False
        self._h = C.c_void_p()
        fn = self._fn("create_batch_mh")
        fn.restype = C.c_int
        rc = fn(C.byref(self._h), C.c_int(model), C.c_int(int(n_filters)), C.c_int(int(n_per_filter)), C.c_int(int(max_per_filter)), C.c_int(device_id),
                C.c_int(gm_capacity))
        if rc != OK:
            self._h = C.c_void_p()
            raise EngineError(rc, "create_batch_mh failed: " + ("max_per_filter beyond 2048 (one workgroup resamples a filter), or the Victoria Park model" if rc == ERR_UNSUPPORTED
                                                                else "no gfx950 device / bad arguments (max_per_filter < n_per_filter?)"))
        self.n_filters = int(n_filters)
        self.n_per_filter = int(n_per_filter)
        self.gm_capacity = int(gm_capacity)
        self.max_per_filter = int(max_per_filter)

    def block(self, b, n=None):
        """The global slots of filter b: all max_per_filter of them, or the first n."""
        return slice(b * self.max_per_filter, b * self.max_per_filter + (self.max_per_filter if n is None else int(n)))

    def batch_fastslam_mh_cycle_async(self, predict, Zs, u01, poses=None, pose_cov=None):
        """rfsgpu_batch_fastslam_mh_cycle_async: Zs one measurement array per filter, u01 [n_filters] the draws in [0, 1)."""
        assert len(Zs) == self.n_filters
        z = np.zeros((self.n_filters, MAX_Z, 2))
        nz = np.zeros(self.n_filters, dtype=np.int32)
        for b, Z in enumerate(Zs):
            Z = _f64(Z).reshape(-1, 2) if np.size(Z) else np.zeros((0, 2))
            nz[b] = Z.shape[0]
            z[b, : min(Z.shape[0], MAX_Z)] = Z[:MAX_Z]
        self.batch_fastslam_mh_cycle_async_packed(predict, z, nz, u01, poses=poses, pose_cov=pose_cov)

    def batch_fastslam_mh_cycle_async_packed(self, predict, z, nz, u01, poses=None, pose_cov=None):
        """The same with the sets already in the call's layout (z [n_filters, MAX_Z, 2] float64, nz [n_filters] int32)."""
        assert z.dtype == np.float64 and nz.dtype == np.int32 and z.shape == (self.n_filters, MAX_Z, 2) and z.flags.c_contiguous and nz.flags.c_contiguous
        u = _f64(u01, (self.n_filters,))
        x = None if poses is None else _f64(poses, (self.n, 3))
        stride = 0
        cv = None
        if pose_cov is not None:
            cv = _f64(pose_cov)
            assert cv.size in (9, 9 * self.n)
            stride = 0 if cv.size == 9 else 9
        self._call("batch_fastslam_mh_cycle_async", C.c_int(1 if predict else 0), C.c_void_p(None) if x is None else self._ptr(x),
                   C.c_void_p(None) if cv is None else self._ptr(cv), C.c_int(stride), self._ptr(z), self._ptr(nz), self._ptr(u))

    def fastslam_mh_cycle_sensed_async(self, predict, call, poses=None, pose_cov=None):
        """rfsgpu_batch_fastslam_mh_cycle_sensed_async: the multi-hypothesis cycle on the sets the last sense_async left on the device;
        every filter's draw is the resampling draw of (its motion key, call)."""
        px, pc, stride, keep = self._pose_args(poses, pose_cov)
        self._call("batch_fastslam_mh_cycle_sensed_async", C.c_int(1 if predict else 0), px, pc, stride, C.c_ulonglong(int(call)))

    def batch_fastslam_last_cycle(self):
        """rfsgpu_batch_fastslam_last_cycle (synchronising): per filter the counts after the update and after the resampling, whether it
        fired, N_eff, whether the filter overflowed; parent / plan [n_filters, max_per_filter] in slots local to the filter (-1 beyond
        the counts)."""
        nF, m = self.n_filters, self.max_per_filter
        nu, nr = np.zeros(nF, dtype=np.int32), np.zeros(nF, dtype=np.int32)
        fired, ovf = np.zeros(nF, dtype=np.uint8), np.zeros(nF, dtype=np.uint8)
        neff = np.zeros(nF)
        parent, plan = np.zeros((nF, m), dtype=np.int32), np.zeros((nF, m), dtype=np.int32)
        self._call("batch_fastslam_last_cycle", self._ptr(nu), self._ptr(nr), self._ptr(fired), self._ptr(neff), self._ptr(ovf), self._ptr(parent), self._ptr(plan))
        return dict(n_after_update=nu, n_after_resample=nr, fired=fired.astype(bool), n_eff=neff, overflowed=ovf.astype(bool), parent=parent, plan=plan)

    def batch_live_counts(self):
        """rfsgpu_batch_live_counts (synchronising): the live particle count of every filter."""
        out = np.zeros(self.n_filters, dtype=np.int32)
        self._call("batch_live_counts", self._ptr(out))
        return out

    def serve_metrics(self, on=True):
        """rfsgpu_batch_mh_serve_metrics (synchronising): from now on the [metric] calls (set_ground_truth, error_log_*, step_error_async,
        step_error, get_map_estimate) serve this batch, each filter's record over its live slots as the device counts them where the
        kernel runs; on=False: they refuse again."""
        self._call("batch_mh_serve_metrics", C.c_int(1 if on else 0))


class CBatchVPMH(CBatchMH, CVPBatch):
    """A batch of Victoria Park multi-hypothesis FastSLAM filters behind the C ABI (rfsgpu_create_batch_vp_mh): CBatchMH's layout and
    read-backs (block, batch_fastslam_last_cycle, batch_live_counts), CVPBatch's configuration, scan, motion and run propagation.  Its
    cycle is batch_vp_fastslam_mh_cycle_async; every other cycle, the resampling calls and the serve_* switches refuse."""

    def __init__(self, lib, prefix, n_filters, n_per_filter, max_per_filter, device_id=0, gm_capacity=512):
        self._lib, self._p = lib, prefix
        self.model = MODEL_VICTORIAPARK_3D
        self.device_id = device_id
        self.dm = self.dz = 3
        self._borrowed = False
        self._h = C.c_void_p()
        fn = self._fn("create_batch_vp_mh")
        fn.restype = C.c_int
        rc = fn(C.byref(self._h), C.c_int(int(n_filters)), C.c_int(int(n_per_filter)), C.c_int(int(max_per_filter)), C.c_int(device_id), C.c_int(gm_capacity))
        if rc != OK:
            self._h = C.c_void_p()
            raise EngineError(rc, "create_batch_vp_mh failed: " + ("max_per_filter beyond 2048 (one workgroup resamples a filter)" if rc == ERR_UNSUPPORTED
                                                                   else "no gfx950 device / bad arguments (max_per_filter < n_per_filter?)"))
        self.n_filters = int(n_filters)
        self.n_per_filter = int(n_per_filter)
        self.gm_capacity = int(gm_capacity)
        self.max_per_filter = int(max_per_filter)

    def batch_vp_fastslam_mh_cycle_async(self, predict, Zs, u01, poses=None, pose_cov=None, scan=None):
        """rfsgpu_batch_vp_fastslam_mh_cycle_async: Zs one measurement array per filter ([n_z, 3], possibly empty), u01 [n_filters] the
        draws in [0, 1); scan: the laser scan that goes with the sets (None: the one the handle holds)."""
        assert len(Zs) == self.n_filters
        z = np.zeros((self.n_filters, MAX_Z, 3))
        nz = np.zeros(self.n_filters, dtype=np.int32)
        for b, Z in enumerate(Zs):
            Z = _f64(Z).reshape(-1, 3) if np.size(Z) else np.zeros((0, 3))
            nz[b] = Z.shape[0]
            z[b, : min(Z.shape[0], MAX_Z)] = Z[:MAX_Z]
        self.batch_vp_fastslam_mh_cycle_async_packed(predict, z, nz, u01, poses=poses, pose_cov=pose_cov, scan=scan)

    def batch_vp_fastslam_mh_cycle_async_packed(self, predict, z, nz, u01, poses=None, pose_cov=None, scan=None):
        """The same with the sets already in the call's layout (z [n_filters, MAX_Z, 3] float64, nz [n_filters] int32, C-contiguous)."""
        assert z.dtype == np.float64 and nz.dtype == np.int32 and z.shape == (self.n_filters, MAX_Z, 3) and z.flags.c_contiguous and nz.flags.c_contiguous
        u = _f64(u01, (self.n_filters,))
        px, pc, stride, keep = self._pose_args(poses, pose_cov)
        s = None if scan is None else _f64(scan).reshape(-1)
        self._call("batch_vp_fastslam_mh_cycle_async", C.c_int(1 if predict else 0), px, pc, stride, self._ptr(z), self._ptr(nz),
                   C.c_void_p(None) if s is None else self._ptr(s), C.c_int(0 if s is None else s.size), self._ptr(u))


def mat_perm(lib, prefix, A, device_id=0):
    """MatPerm::calc (src/MatrixPermanent.cpp:41-112), batched: A is (batch, n, n)."""
    A = _f64(A)
    if A.ndim == 2:
        A = A[None]
    b, n, _ = A.shape
    out = np.empty(b)
    fn = getattr(lib, prefix + "mat_perm")
    fn.restype = C.c_int
    rc = fn(A.ctypes.data_as(C.c_void_p), C.c_int(n), C.c_int(b), out.ctypes.data_as(C.c_void_p), C.c_int(device_id))
    if rc != OK:
        raise EngineError(rc, "mat_perm failed")
    return out


class Group:
    """rfsgpu_group_*: one filter over several GPUs from one host thread (contiguous particle blocks, one shard per device)."""

    def __init__(self, lib, n_particles, device_ids, gm_capacity=512, model=MODEL_RNGBRG_2D):
        self._lib = lib
        self._g = C.c_void_p()
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        lib.rfsgpu_group_create.restype = C.c_int
        rc = lib.rfsgpu_group_create(C.byref(self._g), C.c_int(model), C.c_int(int(n_particles)), ids.ctypes.data_as(C.c_void_p), C.c_int(ids.size),
                                     C.c_int(gm_capacity))
        if rc != OK:
            self._g = C.c_void_p()
            raise EngineError(rc, "group_create failed")
        self.n = int(n_particles)
        self.dm = self.dz = 3 if model == MODEL_VICTORIAPARK_3D else 2
        lib.rfsgpu_group_shard.restype = C.c_void_p
        self.shards = [CFilter(lib, "rfsgpu_", 0, model=model, device_id=int(ids[k]), gm_capacity=gm_capacity,
                               borrowed=lib.rfsgpu_group_shard(self._g, C.c_int(k))) for k in range(ids.size)]

    def _call(self, name, *args):
        fn = getattr(self._lib, "rfsgpu_group_" + name)
        fn.restype = C.c_int
        rc = fn(self._g, *args)
        if rc != OK:
            le = self._lib.rfsgpu_group_last_error
            le.restype = C.c_char_p
            raise EngineError(rc, (le(self._g) or b"").decode())

    def close(self):
        if self._g and self._g.value:
            for s in self.shards:
                s.close()
            self._lib.rfsgpu_group_destroy.restype = None
            self._lib.rfsgpu_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def locate(self, particle):
        k, s = C.c_int(), C.c_int()
        self._call("locate", C.c_int(int(particle)), C.byref(k), C.byref(s))
        return k.value, s.value

    def set_filter_config(self, cfg):
        self._call("set_filter_config", C.byref(cfg))

    def set_model_rngbrg(self, R, Pd, c, rmax, rmin, rbuf):
        m = RngBrgConfig()
        R = _f64(R, (4,))
        for k in range(4):
            m.R[k] = R[k]
        m.probabilityOfDetection, m.uniformClutterIntensity = Pd, c
        m.rangeLimMax, m.rangeLimMin, m.rangeLimBuffer = rmax, rmin, rbuf
        self._call("set_model_rngbrg", C.byref(m))

    def set_kf_config(self, range_thr, bearing_thr):
        self._call("set_kf_config", C.byref(KFConfig(range_thr, bearing_thr)))

    def set_lmk_process_noise(self, Q):
        self._call("set_lmk_process_noise", _f64(Q, (self.dm * self.dm,)).ctypes.data_as(C.c_void_p))

    def default_filter_config(self):
        return self.shards[0].default_filter_config()

    def set_poses(self, x, cov=None):
        x = _f64(x, (self.n, 3))
        if cov is None:
            self._call("set_poses", x.ctypes.data_as(C.c_void_p), C.c_void_p(), C.c_int(0))
        else:
            cov = _f64(cov)
            self._call("set_poses", x.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p), C.c_int(0 if cov.size == 9 else 9))

    def get_poses(self):
        x = np.empty((self.n, 3))
        self._call("get_poses", x.ctypes.data_as(C.c_void_p))
        return x

    def set_weights(self, w):
        self._call("set_weights", _f64(w, (self.n,)).ctypes.data_as(C.c_void_p))

    def get_weights(self):
        w = np.empty(self.n)
        self._call("get_weights", w.ctypes.data_as(C.c_void_p))
        return w

    def import_gm(self, i, w, mean, cov):
        k, s = self.locate(i)
        self.shards[k].import_gm(s, w, mean, cov)

    def export_gm(self, i):
        k, s = self.locate(i)
        return self.shards[k].export_gm(s)

    def get_unused(self, i):
        k, s = self.locate(i)
        return self.shards[k].get_unused(s)

    def gm_sizes(self):
        return np.concatenate([s.gm_sizes() for s in self.shards])

    def predict_map(self, add_birth=True):
        self._call("predict_map", C.c_int(1 if add_birth else 0))

    def set_birth_inheritance(self, mode):
        self._call("set_birth_inheritance", C.c_int(int(mode)))

    def get_particle_ids(self):
        ids = np.zeros(self.n, dtype=np.int32)
        par = np.zeros(self.n, dtype=np.int32)
        self._call("get_particle_ids", ids.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p))
        return ids, par

    def update(self, Z):
        Z = _f64(Z).reshape(-1, self.dz)
        sums = np.empty(2)
        self._call("update", Z.ctypes.data_as(C.c_void_p), C.c_int(Z.shape[0]), sums.ctypes.data_as(C.c_void_p))
        return sums

    def normalize(self):
        sums = np.empty(2)
        self._call("normalize", sums.ctypes.data_as(C.c_void_p))
        return sums

    def resample(self, eff_n_threshold, u01):
        fired = C.c_int()
        plan = np.empty(self.n, dtype=np.int32)
        self._call("resample", C.c_double(eff_n_threshold), C.c_double(u01), C.byref(fired), plan.ctypes.data_as(C.c_void_p))
        return bool(fired.value), (plan if fired.value else None)

    def migration_stats(self):
        r, b = C.c_longlong(), C.c_longlong()
        self._call("migration_stats", C.byref(r), C.byref(b))
        return r.value, b.value

    def collective(self):
        """"rccl" (the weight sums are all-reduced over RCCL on the shards' streams) or "host: <why not>"."""
        fn = self._lib.rfsgpu_group_collective
        fn.restype = C.c_char_p
        return (fn(self._g) or b"").decode()

    def set_model_victoriapark(self, R, Slb, pd_table, expected_clutter, rmax, rmin, bmax, bmin, buffer_pd):
        m = VPConfig()
        R = _f64(R, (9,))
        for k in range(9):
            m.R[k] = R[k]
        m.Slb = Slb
        pd_table = list(pd_table)
        for k, v in enumerate(pd_table):
            m.PdTable[k] = v
        m.nPd = len(pd_table)
        m.expectedClutterNumber = expected_clutter
        m.rangeLimMax, m.rangeLimMin, m.bearingLimitMax, m.bearingLimitMin, m.bufferZonePd = rmax, rmin, bmax, bmin, buffer_pd
        self._call("set_model_victoriapark", C.byref(m))

    def set_laser_scan(self, scan):
        s = _f64(scan).reshape(-1)
        self._call("set_laser_scan", s.ctypes.data_as(C.c_void_p), C.c_int(s.size))

    def set_phase_timing(self, on=True):
        self._call("set_phase_timing", C.c_int(1 if on else 0))

    def getTimingInfo(self):
        t = Timing()
        self._call("get_timing", C.byref(t))
        return t

    def get_filter_config(self):
        return self.shards[0].get_filter_config()

    def update_deferred(self, Z):
        """rfsgpu_group_update_deferred: the normalisation trails by one step, the collective runs beside the next step's kernel."""
        Z = _f64(Z).reshape(-1, self.dz)
        self._call("update_deferred", Z.ctypes.data_as(C.c_void_p), C.c_int(Z.shape[0]))

    def update_nosums(self, Z):
        """rfsgpu_group_update without the host copy of the sums: with the RCCL collective nothing waits for the GPUs."""
        Z = _f64(Z).reshape(-1, self.dz)
        self._call("update", Z.ctypes.data_as(C.c_void_p), C.c_int(Z.shape[0]), C.c_void_p())

    def synchronize(self):
        self._call("synchronize")
