/*
 * rfsgpu.h -- C ABI of the MI355X-native RB-PHD SLAM update engine.
 *
 * This is the drop-in boundary for ONE hot path of kykleung/RFS-SLAM: the per-particle
 * Gaussian-mixture PHD map update + particle weighting + GM merge/prune that runs inside
 * rfs::RBPHDFilter<...>::update() (reference include/RBPHDFilter.hpp:444-541), plus the few
 * map-side pieces either side of it (static landmark predict + birth Gaussians, resample copy).
 *
 * The reference has no FFI / plugin registry; the surface a replacement has to sit behind is the
 * public interface of the RBPHDFilter class template (include/RBPHDFilter.hpp:72-251) and what it
 * inherits from ParticleFilter (include/ParticleFilter.hpp:72-186).  Every entry point below
 * names the reference member it replaces.  INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C, opaque handle, int status returns (0 = RFSGPU_OK), no exceptions / STL / torch types.
 *   - all host buffers are caller-owned; the engine owns its device memory (one handle == one GPU,
 *     one host thread per handle, one process per GPU).
 *   - everything is fp64; matrices are row-major; d_m = landmark dim, d_z = measurement dim
 *     (both 2 for RFSGPU_MODEL_RNGBRG_2D, both 3 for RFSGPU_MODEL_VICTORIAPARK_3D).
 *   - "slot" = particle index 0..n_particles-1.
 *   - the engine fails loudly: there is NO CPU fallback anywhere behind this ABI.
 *
 * STABLE CORE -- the 24 entry points a reference-side binding needs (round 5: + rfsgpu_update_io, the update with its inputs and outputs in one call); integration/RBPHDFilter_rfsgpu.hpp (the class template that
 * stands where rfs::RBPHDFilter stands, compiled under the unmodified reference drivers) uses 20 of them and nothing else
 * (tests/test_abi.py checks the list against the linked drivers):
 *   RFSGPU_CORE: rfsgpu_abi_version rfsgpu_create rfsgpu_destroy rfsgpu_last_error rfsgpu_default_filter_config
 *   RFSGPU_CORE: rfsgpu_set_filter_config rfsgpu_set_model_rngbrg rfsgpu_set_model_victoriapark rfsgpu_set_laser_scan
 *   RFSGPU_CORE: rfsgpu_set_kf_config rfsgpu_set_lmk_process_noise rfsgpu_set_poses rfsgpu_set_weights rfsgpu_get_weights
 *   RFSGPU_CORE: rfsgpu_predict_map rfsgpu_update rfsgpu_resample_apply rfsgpu_set_birth_inheritance rfsgpu_gm_size
 *   RFSGPU_CORE: rfsgpu_get_landmark rfsgpu_get_timing rfsgpu_set_phase_timing rfsgpu_synchronize rfsgpu_update_io
 * The same binding over SEVERAL GPUs (RFSGPU_DEVICES=0,1,...: integration/RBPHDFilter_rfsgpu.hpp, rfsgpu_engine_facade) uses the group
 * counterparts of those calls and nothing else:
 *   RFSGPU_CORE_MULTI: rfsgpu_group_create rfsgpu_group_destroy rfsgpu_group_last_error rfsgpu_group_set_filter_config
 *   RFSGPU_CORE_MULTI: rfsgpu_group_set_model_rngbrg rfsgpu_group_set_model_victoriapark rfsgpu_group_set_laser_scan rfsgpu_group_set_kf_config
 *   RFSGPU_CORE_MULTI: rfsgpu_group_set_lmk_process_noise rfsgpu_group_set_poses rfsgpu_group_set_weights rfsgpu_group_get_weights
 *   RFSGPU_CORE_MULTI: rfsgpu_group_predict_map rfsgpu_group_update rfsgpu_group_apply_plan rfsgpu_group_gm_size rfsgpu_group_get_landmark
 *   RFSGPU_CORE_MULTI: rfsgpu_group_get_timing rfsgpu_group_set_phase_timing rfsgpu_group_update_io
 * Everything else is OPTIONAL and grouped below by who needs it:
 *   [async]    stream-ordered forms for host loops that pipeline (rfsgpu_*_async, rfsgpu_step_async, rfsgpu_set_stream, ...);
 *   [multi]    several GPUs: rfsgpu_group_* (one host thread), slab rows / device pointers (one process per GPU over RCCL);
 *   [state]    state injection and probes for tests and tools (import / export of mixtures, candidate lists, ids, masks);
 *   [bench]    snapshot / restore, kernel timing statistics, debug counters, test probes: declared only under
 *              RFSGPU_ENABLE_BENCH_API (a maintainer reading this header for the binding never meets them);
 *   [fastslam] FastSLAM / MH-FastSLAM on the same handle, the optional device-side Ackerman propagation, rfsgpu_mat_perm; the whole
 *              FastSLAM::update enqueued without a host stop (rfsgpu_fastslam_cycle_async: 2-D model, no candidate lists;
 *              rfsgpu_fastslam_cycle_full_async: either model, candidate lists, the scan with the call), behind which the
 *              propagation and static-step calls enqueue without taking the particle count over;
 *   [batch]    many independent 2-D filters in one handle, stepped together in one launch chain;
 *   [metric]   per-step OSPA / COLA map error and pose error computed on the device, kept in a device-side log;
 *   [resample] ParticleFilter::resample for an ordinary handle of any size on the device, without a host stop;
 *   [rbphd-cycle] the whole RBPHDFilter::update -- its counters, its gate, the resampling -- enqueued without a host stop, and the
 *              birth predict behind it with the inheritance walk made on the device;
 *   [sensor]   the simulator's range-bearing sensor of every filter of a batch (RB-PHD; FastSLAM kinds by a switch) drawn on the device, for batch sweeps;
 *   [truth]    the simulator's trajectory, odometry and landmarks of every filter of a batch drawn on the device, and a run of steps in one call;
 *   [estimate] every filter's pose and map estimate per step (the reference's particlePose.dat / landmarkEst.dat) kept in a device-side log.
 * A maintainer wiring the reference to the library reads the CORE entries and INTEGRATION.md; nothing optional is required
 * for correct results.
 */
#ifndef RFSGPU_H
#define RFSGPU_H

#include <stddef.h>   /* size_t */

#ifdef __cplusplus
extern "C" {
#endif

#define RFSGPU_ABI_VERSION 1

/* Maximum measurements per update() (one 64-bit association mask per landmark). */
/* Hard limits of the device path (the reference has none; all are refused LOUDLY -- an error status, never a silent
 * truncation -- and all are far above BASELINE.json's configurations): RFSGPU_MAX_Z measurements per update,
 * RFSGPU_MAX_EVAL evaluation points, Murty extended dimension nR + nC <= 64 (a partition's search that outgrows the
 * 1 + 200 x 32 node pool -- possible only with more than 32 rows -- is refused with its own message, not truncated), gm_capacity <= 2048 Gaussians per particle,
 * RFSGPU_MAX_CANDIDATES birth candidates per particle on the RB-PHD path (64 landmark candidates on the FastSLAM path). */
#define RFSGPU_MAX_Z 64
/* Maximum evaluation points for the multi-feature particle weight. */
#define RFSGPU_MAX_EVAL 64

typedef struct rfsgpu_filter rfsgpu_filter;

enum rfsgpu_status {
  RFSGPU_OK = 0,
  RFSGPU_ERR_INVALID = 1,     /* bad argument / bad index                                      */
  RFSGPU_ERR_HIP = 2,         /* a HIP runtime call failed (rfsgpu_last_error has the string)  */
  RFSGPU_ERR_CAPACITY = 3,    /* a particle's Gaussian mixture outgrew gm_capacity             */
  RFSGPU_ERR_NO_DEVICE = 4,   /* no gfx950 device visible                                      */
  RFSGPU_ERR_UNSUPPORTED = 5  /* configuration outside what the device path implements         */
};

enum rfsgpu_model {
  RFSGPU_MODEL_RNGBRG_2D = 0,       /* MeasurementModel_RngBrg + KalmanFilter_RngBrg + Landmark2d (d_m = d_z = 2)            */
  RFSGPU_MODEL_VICTORIAPARK_3D = 1  /* MeasurementModel_VictoriaPark + KalmanFilter_VictoriaPark + Landmark3d (d_m = d_z = 3:
                                       landmark (x, y, diameter), measurement (range, bearing, diameter))                    */
};

/* Maximum entries of the Victoria Park Pd table / beams of a laser scan / birth candidates per particle. */
#define RFSGPU_VP_MAX_PD 16
#define RFSGPU_VP_MAX_SCAN 720
#define RFSGPU_MAX_CANDIDATES 256

/* Mirrors RBPHDFilter::Config, include/RBPHDFilter.hpp:90-146 (same meaning, same defaults
 * :370-382 when filled by rfsgpu_default_filter_config). */
typedef struct rfsgpu_filter_config {
  double birthGaussianWeight;
  unsigned int birthGaussianMeasurementCountThreshold;
  unsigned int birthGaussianMeasurementCheckThreshold;
  double birthGaussianMeasurementSupportDist;
  unsigned int birthGaussianCurrentMeasurementCountThreshold;
  double newGaussianCreateInnovMDThreshold;
  int importanceWeightingEvalPointCount;          /* -1 => all (reference :737 unsigned compare) */
  double importanceWeightingEvalPointGuassianWeight;
  double importanceWeightingMeasurementLikelihoodMDThreshold;
  double gaussianMergingThreshold;
  double gaussianMergingCovarianceInflationFactor;
  double gaussianPruningThreshold;
  int minUpdatesBeforeResample;
  int minMeasurementsBeforeResample;
  int useClusterProcess;                          /* bool in the reference */
} rfsgpu_filter_config;

/* Mirrors MeasurementModel_RngBrg::Config (include/MeasurementModel_RngBrg.hpp:65-71) plus the
 * additive noise R set through MeasurementModel::setNoise (src/rbphdslam2dSim.cpp:466-469). */
typedef struct rfsgpu_rngbrg_config {
  double R[4];                     /* 2x2 row-major measurement covariance */
  double probabilityOfDetection;
  double uniformClutterIntensity;
  double rangeLimMax;
  double rangeLimMin;
  double rangeLimBuffer;
} rfsgpu_rngbrg_config;

/* Mirrors MeasurementModel_VictoriaPark::Config (include/MeasurementModel_VictoriaPark.hpp:150-158) plus the noise set
 * through setNoise(R, Slb) (src/MeasurementModel_VictoriaPark.cpp:66-73).  Angles in radians. */
typedef struct rfsgpu_vp_config {
  double R[9];                       /* 3x3 row-major measurement covariance (range, bearing, diameter) */
  double Slb;                        /* variance of the lidar beam angle                                 */
  double PdTable[RFSGPU_VP_MAX_PD];  /* config.probabilityOfDetection_ (Pd by number of visible beams)   */
  int nPd;
  double expectedClutterNumber;
  double rangeLimMax, rangeLimMin;
  double bearingLimitMax, bearingLimitMin;
  double bufferZonePd;
} rfsgpu_vp_config;

/* Mirrors KalmanFilter_RngBrg::Config (include/KalmanFilter_RngBrg.hpp:55-60). <=0 disables. */
typedef struct rfsgpu_kf_config {
  double rangeInnovationThreshold;
  double bearingInnovationThreshold;
} rfsgpu_kf_config;

/* Mirrors FastSLAM::Config (include/FastSLAM.hpp:106-132), same member names without the trailing '_'.
 * Defaults: FastSLAM constructor (:243-257). */
typedef struct rfsgpu_fastslam_config {
  int minUpdatesBeforeResample;
  int minMeasurementsBeforeResample;
  double landmarkExistencePrior;
  double mapExistencePruneThreshold;
  double minLogMeasurementLikelihood;
  int nParticlesMax;
  unsigned maxNDataAssocHypotheses;
  double maxDataAssocLogLikelihoodDiff;
  double landmarkCandidateMeasurementSupportDist;
  unsigned landmarkCandidateMeasurementCountThreshold;
  unsigned landmarkCandidateCurrentMeasurementCountThreshold;
  unsigned landmarkCandidateMeasurementCheckThreshold;
  double landmarkLockWeight;
  unsigned pruningMeasurementsThreshold;
} rfsgpu_fastslam_config;

/* Mirrors RBPHDFilter::TimingInfo (include/RBPHDFilter.hpp:152-167), nanoseconds, accumulated.
 * *_wall come from HIP events around each phase's kernels; *_cpu is the host time spent inside
 * the corresponding ABI calls (launch + sync). */
typedef struct rfsgpu_timing {
  long long predict_wall, predict_cpu;
  long long mapUpdate_wall, mapUpdate_cpu;
  long long mapUpdate_kf_wall, mapUpdate_kf_cpu;
  long long particleWeighting_wall, particleWeighting_cpu;
  long long mapMerge_wall, mapMerge_cpu;
  long long mapPrune_wall, mapPrune_cpu;
  long long particleResample_wall, particleResample_cpu;
} rfsgpu_timing;

/* ---- [core] lifetime ------------------------------------------------------------------------------ */

/* ABI version of the loaded library (== RFSGPU_ABI_VERSION). */
int rfsgpu_abi_version(void);

/* Replaces the RBPHDFilter constructor (include/RBPHDFilter.hpp:350-393): n_particles particles
 * of weight 1, pose 0, empty maps, default config.  device_id: HIP ordinal.  gm_capacity: per-particle
 * Gaussian slots (rounded up to a multiple of 64); must cover the transient size right after the
 * map update (nM + new Gaussians).  Exceeding it sets RFSGPU_ERR_CAPACITY, never corrupts memory. */
int rfsgpu_create(rfsgpu_filter **out, int model, int n_particles, int device_id, int gm_capacity);
/* The same with room for the particle set to GROW up to max_particles (>= n_particles): FastSLAM's multi-hypothesis
 * update multiplies particles (FastSLAM.hpp:543-551, ParticleFilter::copyParticle) until resampleWithMapCopy brings the
 * set back to its initial size.  rfsgpu_n_particles = nParticles_ now; every array argument of the other calls has that
 * many entries. */
int rfsgpu_create_ex(rfsgpu_filter **out, int model, int n_particles, int device_id, int gm_capacity, int max_particles);
int rfsgpu_n_particles(const rfsgpu_filter *f);
int rfsgpu_max_particles(const rfsgpu_filter *f);
/* Replaces ~RBPHDFilter (:395-403). */
void rfsgpu_destroy(rfsgpu_filter *f);
/* Human-readable text for the last non-OK status on this handle (never NULL). */
const char *rfsgpu_last_error(const rfsgpu_filter *f);

/* ---- [core] configuration (the three public config structs of the reference) ---------------------- */

void rfsgpu_default_filter_config(rfsgpu_filter_config *cfg);            /* RBPHDFilter.hpp:370-382 */
int rfsgpu_set_filter_config(rfsgpu_filter *f, const rfsgpu_filter_config *cfg);   /* filter.config.* */
int rfsgpu_get_filter_config(const rfsgpu_filter *f, rfsgpu_filter_config *cfg);
/* How rfsMeasurementLikelihood evaluates a partition with nR + nC > 8 (include/RBPHDFilter.hpp:920-959):
 *   RFSGPU_PARTITION_MURTY200 (default) the reference's way, bug-compatible: Murty's ranked assignments on the extended matrix,
 *                             sum of at most 200 terms, stop below score -1000 (murty.h);
 *   RFSGPU_PARTITION_EXACT    the untruncated sum over all partial assignments (the quantity the truncation approximates) by a
 *                             subset recurrence over the smaller side of the partition (<= 9 items; larger partitions still
 *                             go to Murty).  Not the reference's numbers: an opt-in, timed beside the default. */
#define RFSGPU_PARTITION_MURTY200 0
#define RFSGPU_PARTITION_EXACT 1
int rfsgpu_set_partition_mode(rfsgpu_filter *f, int mode);
int rfsgpu_get_partition_mode(const rfsgpu_filter *f);
int rfsgpu_set_model_rngbrg(rfsgpu_filter *f, const rfsgpu_rngbrg_config *cfg);    /* getMeasurementModel()->config / setNoise */
int rfsgpu_set_kf_config(rfsgpu_filter *f, const rfsgpu_kf_config *cfg);           /* getKalmanFilter()->config */
/* Victoria Park model: getMeasurementModel()->config / setNoise(R, Slb) (src/rbphdslam_VictoriaPark.cpp:371-378). */
int rfsgpu_set_model_victoriapark(rfsgpu_filter *f, const rfsgpu_vp_config *cfg);
/* MeasurementModel_VictoriaPark::setLaserScan (src/MeasurementModel_VictoriaPark.cpp:267-281): the raw scan used by the
 * occlusion-based Pd and by the clutter intensity (expected clutter / field-of-view area); n <= RFSGPU_VP_MAX_SCAN. */
int rfsgpu_set_laser_scan(rfsgpu_filter *f, const double *scan, int n);
#ifdef RFSGPU_ENABLE_BENCH_API   /* [bench] / [test]: exported by the library, declared only for callers that ask (bench.py, the tests) */
/* Probe for tests: MeasurementModel_VictoriaPark::probabilityOfDetection (src/MeasurementModel_VictoriaPark.cpp:153-199) of the
 * first max_n Gaussians of particle `slot` under the current pose and scan, as the kernels evaluate it: Pd and the
 * isCloseToSensingLimit flag. */
int rfsgpu_vp_probe_pd(rfsgpu_filter *f, int slot, double *pd, int *close_to_limit, int max_n);
#endif /* RFSGPU_ENABLE_BENCH_API */
/* getLmkProcessModel()->setNoise(Q) (include/ProcessModel.hpp:195-208); Q is d_m x d_m. */
int rfsgpu_set_lmk_process_noise(rfsgpu_filter *f, const double *Q);

/* ---- [core] particle state crossing the boundary --------------------------------------------------- */

/* Poses after the host-side ParticleFilter::propagate / setParticlePose
 * (include/ParticleFilter.hpp:322-341, RBPHDFilter.hpp:1181-1186).  x: 3 doubles per particle
 * (x, y, theta).  cov: 3x3 pose covariance (enters S, src/MeasurementModel_RngBrg.cpp:102);
 * cov_stride = 0 -> one shared 3x3 (or cov==NULL -> zero), 9 -> one per particle. */
int rfsgpu_set_poses(rfsgpu_filter *f, const double *x, const double *cov, int cov_stride);
int rfsgpu_get_poses(rfsgpu_filter *f, double *x);
/* [state] The pose covariances as the update reads them: cov [n_particles][9] row-major (a shared matrix, cov_stride 0, is repeated). */
int rfsgpu_get_pose_covs(rfsgpu_filter *f, double *cov);
/* Particle::setWeight / getWeight (include/Particle.hpp), n_particles doubles. */
int rfsgpu_set_weights(rfsgpu_filter *f, const double *w);
int rfsgpu_get_weights(rfsgpu_filter *f, double *w);

/* ---- [core] map access (getGMSize / getLandmark, RBPHDFilter.hpp:1152-1178) + [state] injection ------ */

int rfsgpu_gm_size(rfsgpu_filter *f, int slot);                        /* -1 on bad index */
/* returns RFSGPU_OK, or RFSGPU_ERR_INVALID on a bad index (reference returns false). */
int rfsgpu_get_landmark(rfsgpu_filter *f, int slot, int m, double *mean, double *cov, double *w);
/* Replace particle `slot`'s mixture with n Gaussians (GaussianMixture::addGaussian order). */
int rfsgpu_import_gm(rfsgpu_filter *f, int slot, int n, const double *w, const double *mean, const double *cov);
/* Copy out up to max_n Gaussians in storage order; *n_out = mixture size.  w_prev may be NULL. */
int rfsgpu_export_gm(rfsgpu_filter *f, int slot, int max_n, int *n_out, double *w, double *w_prev,
                     double *mean, double *cov);
/* Set particle `slot`'s birth bookkeeping (unused_measurements_[slot] as ascending indices, nLandmarksInFOV_[slot]);
 * needed when a particle migrates between shards during a multi-GPU resample (RBPHDFilter.hpp:1005-1011). */
int rfsgpu_import_aux(rfsgpu_filter *f, int slot, const int *unused_idx, int n_unused, int n_in_fov);
/* birthGaussians_[slot] (RBPHDFilter.hpp:253, :173-177): the particle's birth-Gaussian candidates in list order. */
int rfsgpu_export_birth_candidates(rfsgpu_filter *f, int slot, int max_n, int *n_out, double *mean, double *cov, int *n_support, int *n_checks);
int rfsgpu_import_birth_candidates(rfsgpu_filter *f, int slot, int n, const double *mean, const double *cov, const int *n_support, const int *n_checks);
/* All mixture sizes at once (n_particles ints). */
int rfsgpu_gm_sizes(rfsgpu_filter *f, int *sizes);

/* ---- [core] the hot path (+ its [async] forms) --------------------------------------------------------------------------- */

/* Map part of RBPHDFilter::predict (:415-442): if add_birth, addBirthGaussians (:1000-1084) from
 * the previous update's measurements / unused lists at the CURRENT (pre-propagation) poses, then
 * StaticProcessModel::staticStep (Sigma += Q) on every Gaussian (:433-439). */
int rfsgpu_predict_map(rfsgpu_filter *f, int add_birth);

/* The particle-parallel body of RBPHDFilter::update (:444-523): updateMap, importanceWeighting
 * (unless useClusterProcess), merge, prune.  z: n_z x d_z doubles.  n_z == 0 returns OK without
 * touching anything (:450-452).  Resampling / normalisation stay with the caller (below). */
int rfsgpu_update(rfsgpu_filter *f, const double *z, int n_z);
/* RBPHDFilter::update (:444-541) with everything it consumes and returns in ONE synchronous call: [optionally the predict that
 * precedes it, see rfsgpu_cycle_async: `predict` = RFSGPU_CYCLE_NO_PREDICT | 0 | 1], poses `x` (+ covariance; NULL = unchanged),
 * particle weights `w_in` (NULL = unchanged), the measurement set, and the updated (un-normalised) weights back in `w_out`
 * (NULL = not wanted).  One wait for the device, one error check: what set_poses + set_weights + update + get_weights do in four
 * calls and two waits.  The reference-side binding's update() is this call. */
int rfsgpu_update_io(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *w_in,
                     const double *z, int n_z, double *w_out);
/* rfsgpu_update runs the 2-D model's step as ONE fused launch by default and books its time under TimingInfo::mapUpdate.
 * on != 0: the phases run as separate launches instead (updateMap, importanceWeighting, merge + prune), so that the
 * mapUpdate / particleWeighting / mapMerge buckets of RBPHDFilter::TimingInfo (:152-167) are filled separately, as the
 * reference's timing printout expects -- same results bit for bit, about a third more device time. */
int rfsgpu_set_phase_timing(rfsgpu_filter *f, int on);
/* Stream-ordered form of rfsgpu_update: enqueues the step and returns without waiting for the GPU.  With the 2-D model the
 * step is ONE kernel (a workgroup takes its particle through updateMap, importanceWeighting, merge and prune; results are
 * bit-identical to rfsgpu_update; the environment variable RFSGPU_FUSED_STEP=0 selects the three-kernel form).  Device-side
 * errors (capacity overflow, ...) surface at the next rfsgpu_synchronize() / synchronous call; per-phase HIP-event pairs of
 * up to RFSGPU_ASYNC_RING outstanding steps are harvested there into TimingInfo and rfsgpu_kernel_time_stats.  A host loop
 * that does not need the weights every step (no resampling decision pending) pipelines its steps with this. */
#define RFSGPU_ASYNC_RING 256
int rfsgpu_update_async(rfsgpu_filter *f, const double *z, int n_z);
/* The same step followed -- in the same post kernel that runs the Murty partitions -- by the weight reduction of
 * ParticleFilter::normalizeWeights (include/ParticleFilter.hpp:352-363): {sum w, sum w^2} of this shard go to the bound sums
 * buffer (rfsgpu_bind_weight_sums_buffer / rfsgpu_weight_sums_device_ptr); with normalize != 0 (a filter that lives on one
 * GPU) the weights are divided by the sum right there, otherwise the caller all-reduces the pair across its shards and calls
 * rfsgpu_normalize_weights.  Two launches per step (fused step + post) instead of five. */
int rfsgpu_step_async(rfsgpu_filter *f, const double *z, int n_z, int normalize);
/* One submission per predict + update cycle (round 5).  RBPHDFilter::predict's map part (include/RBPHDFilter.hpp:415-442: birth
 * Gaussians at the poses the previous update used, then StaticProcessModel::staticStep) -- `predict` = 1 with births, 0 without,
 * RFSGPU_CYCLE_NO_PREDICT for none --, then the host's new poses `x` (+ covariance; NULL = unchanged) and particle weights `w_in`
 * (NULL = unchanged), then RBPHDFilter::update's body (:444-523) with the post kernel's weight sums / division as in
 * rfsgpu_step_async.  Stream-ordered, the caller's buffers are copied before the call returns.  Where the configuration allows it
 * (2-D model, immediate births, no inheritance walk pending, n_z > 0) the predict runs at the head of the fused step kernel --
 * one launch chain per cycle, no separate predict launch; otherwise the stand-alone kernels are enqueued in the same order.
 * Same results either way as rfsgpu_predict_map + rfsgpu_set_poses + rfsgpu_set_weights + rfsgpu_step_async. */
/* [multi] rfsgpu_step_async(normalize = 0) for hosts that shard the particles over several GPUs, with the weight normalisation
 * trailing by one step: the post kernel divides the weights by *prev_total_dev ({sum w, sum w^2} of the PREVIOUS step over all
 * shards, device memory, NULL = none) before it takes this step's sums into the bound sums buffer, and the stream waits for
 * `wait_event` (a hipEvent_t recorded on another stream behind the collective that wrote that total; NULL = none) only between
 * the step kernel and the post kernel.  The one collective of the path then runs beside the next step kernel, not in front of
 * it.  (w L) / T instead of (w / T) L: an ulp apart from the call-by-call order.  A host that needs the normalised weights or
 * N_eff (the resample test, include/ParticleFilter.hpp:405-415) finishes with rfsgpu_normalize_weights(f, 0, total_dev). */
int rfsgpu_step_async_deferred(rfsgpu_filter *f, const double *z, int n_z, const void *prev_total_dev, void *wait_event);
/* [multi] The same hand-over without stream events (an event record and an event wait are a marker and a barrier packet on the step's
 * stream).  Per step: rfsgpu_step_async_trailing(h, z, n, total_dev, have_prev) on the engine's stream, then ON THE SIDE STREAM
 * rfsgpu_collective_gate(h, side) -> the collective of the shards' sums (the bound sums buffer) into total_dev ->
 * rfsgpu_collective_publish(h, side).  The gate kernel waits on the device for this step's sums, the next step's post kernel waits on
 * the device for the published total (bounded spins; a protocol that is never completed raises RFSGPU_ERR_UNSUPPORTED at the next
 * synchronising call instead of hanging).  have_prev = 0 for the first step of a run or after the pending total has been applied. */
int rfsgpu_step_async_trailing(rfsgpu_filter *f, const double *z, int n_z, const void *total_dev, int have_prev);
int rfsgpu_collective_gate(rfsgpu_filter *f, void *hip_stream);
int rfsgpu_collective_publish(rfsgpu_filter *f, void *hip_stream);
/* [multi] Whether the engine's stream and `hip_stream` make progress side by side on this runtime -- what the sequence-number form
 * above needs (its post kernel waits for a word a LATER submission on the other stream publishes; two streams mapped onto one
 * hardware queue serialise, and the wait can only run out: RFSGPU_ERR_UNSUPPORTED, "collective hand-over timed out").  Plays the
 * hand-over once with nothing at stake (bounded 0.2 s, synchronises both streams); *side_by_side = 1 | 0.  Probe once per stream
 * pair; on 0 use rfsgpu_step_async_deferred (stream events: two packets on the step's stream, ~+9 us per step) -- which is why both
 * forms stay.  rfsgpu_group_update_deferred and the Python hosts do exactly that. */
int rfsgpu_collective_probe(rfsgpu_filter *f, void *hip_stream, int *side_by_side);
#define RFSGPU_CYCLE_NO_PREDICT (-1)
int rfsgpu_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *w_in,
                       const double *z, int n_z, int normalize);
/* The host side of an asynchronous filter loop (what the Victoria Park driver needs per lidar message: one call for the
 * inputs, one for the step, no host wait -- src/rbphdslam_VictoriaPark.cpp:555-583):
 *   rfsgpu_set_step_inputs_async  poses (+ covariance; x == NULL leaves them) and, Victoria Park model, the laser scan
 *                                 (MeasurementModel_VictoriaPark::setLaserScan; scan == NULL leaves it) through a pinned ring;
 *   rfsgpu_predict_map_async      rfsgpu_predict_map without the error-word readback.  With add_birth != 0 it resolves a pending
 *                                 rfsgpu_resample_async first (the inheritance walk reads the ids on the host); behind pending
 *                                 rfsgpu_rbphd_cycle_async cycles it resolves nothing: the walk is made on the device ([rbphd-cycle]).
 * Device-side errors (capacity, ...) of asynchronous calls surface at the next synchronising call (rfsgpu_synchronize,
 * rfsgpu_weight_sums, rfsgpu_get_weights, ...). */
int rfsgpu_set_step_inputs_async(rfsgpu_filter *f, const double *x, const double *cov, int cov_stride, const double *scan, int n_scan);
int rfsgpu_predict_map_async(rfsgpu_filter *f, int add_birth);
/* A run of n consecutive predicts that add no births (each one: rfsgpu_set_lmk_process_noise(Q_k) + rfsgpu_predict_map_async(f, 0),
 * i.e. StaticProcessModel::staticStep, Sigma += Q_k, include/ProcessModel.hpp:195-208) in ONE launch -- the additions are made
 * one after the other, so the result has the same bits.  noises: [n][D*D] row-major, one per predict of the run (the drivers
 * scale Q with the message interval), or NULL = the noise that is set now, n times.  A driver whose odometry messages outnumber
 * its sensor messages (Victoria Park: 9 to 1) collects the birth-less predicts and flushes them before the next call that
 * reads the maps. */
int rfsgpu_static_steps_async(rfsgpu_filter *f, int n, const double *noises);
/* ParticleFilter::propagate (include/ParticleFilter.hpp:322-339) for the Victoria Park driver's process model, on the device:
 * MotionModel_Ackerman2d::step (src/ProcessModel_Ackerman2D.cpp:47-78) applied to every particle's pose with its own noisy
 * input u + N(0, diag(var)) (ProcessModel::sample's input-noise branch, include/ProcessModel.hpp:126-150).  u = {speed,
 * steering angle}; var = their variances (NULL: no noise); geom = {h, l, dx, dy} (setAckermanParams).  The normal deviates come
 * from Philox4x32-10 keyed by `seed` with counter (particle, call): the reference's single serial boost stream has no parallel
 * form, the distribution is what is kept (csrc/motion.h).  Stream-ordered, no host wait.  OPTIONAL: a host that keeps the
 * reference's own ParticleFilter::propagate sends poses with rfsgpu_set_poses / rfsgpu_set_step_inputs_async instead; the
 * Victoria Park driver of this repository uses it because its host loop, not a kernel, was what bounded a run. */
int rfsgpu_propagate_ackerman_async(rfsgpu_filter *f, const double *u, const double *var, double dt, const double *geom, unsigned long long seed,
                                    unsigned long long call);
/* A run of n such propagations (consecutive odometry messages: u [n][2], var [n][2] or NULL, dt [n], calls numbered call0,
 * call0 + 1, ...) in ONE launch; every particle takes the steps one after the other: the same poses, bit for bit. */
int rfsgpu_propagate_ackerman_run_async(rfsgpu_filter *f, int n, const double *u, const double *var, const double *dt, const double *geom,
                                        unsigned long long seed, unsigned long long call0);
#ifdef RFSGPU_ENABLE_BENCH_API   /* [bench] / [test]: exported by the library, declared only for callers that ask (bench.py, the tests) */
/* [bench] Average duration (ns) of each hot-path kernel group over the async steps harvested since the last call / reset:
 * [0]=phd_update_map [1]=phd_weight_multifeature [2]=gm_merge(+prune); *n_steps = steps averaged.  Steps that ran as one
 * fused kernel report its duration in [0] and 0 in [1], [2] (their TimingInfo share is booked under mapUpdate). */
int rfsgpu_kernel_time_stats(rfsgpu_filter *f, double *avg_ns3, int *n_steps);
/* [bench] Average duration (ns) of the step's post kernel (Murty-200 partitions when any were queued, queue reset, weight sums /
 * division) over the fused steps the last rfsgpu_kernel_time_stats call covered. */
double rfsgpu_post_kernel_avg_ns(const rfsgpu_filter *f);
/* [bench] The HIP events behind the two calls above (and behind TimingInfo's device buckets) ride on every `every`-th fused step only
 * (default 8 since round 5; a filter's first step always carries them).  Three event records per step cost a step of configs[1] 8 us
 * of its 144 (each is a marker packet the queue drains before the next kernel starts).  Statistics average over the sampled steps;
 * TimingInfo (rfsgpu_get_timing) books a sampled step once for itself and once for every un-sampled step since the previous
 * sample, i.e. it stays an estimate of the whole run's device time.  `every` = 1 restores per-step events. */
int rfsgpu_set_step_timing_stride(rfsgpu_filter *f, int every);
/* [bench] Launch order of the fused step's particles, for launches with more workgroups than the GPU holds at once (the Victoria Park
 * step: one wavefront per particle; the 2-D step when its instantiation runs without phase priorities): such a launch lasts as long as
 * whatever started last, so the step kernel records every particle's duration and the post kernel sorts them for the next step, longest
 * first (mode 2, the default; RFSGPU_VP_COST_ORDER=0 in the environment: mode 0).  cost_out (N floats, may be NULL) receives every
 * particle's duration in the last step (100 MHz ticks; 0 where the launch did not capture them); mode 1 + order_in (a permutation of
 * 0..N-1: launch slot -> particle) freezes that order for the following steps, mode 0 goes back to slot == particle.  Results do not
 * depend on the order. */
int rfsgpu_step_launch_order(rfsgpu_filter *f, int mode, const int *order_in, float *cost_out);
#endif /* RFSGPU_ENABLE_BENCH_API */
/* The same four phases one at a time (used by the parity tests and by profiling):          */
/* [test] Murty-200 partition sums of n_jobs given extended tables (n_k x n_k row-major, back to back, n_k = nR[k] + nC[k] <= 64) by the
 * step's own post kernel: sums_out[k] = the sum of exp(score) over the <= 200 best assignments Murty returns with
 * setRealAssignmentBlock(nR, nC) (include/RBPHDFilter.hpp:942-959, src/MurtyAlgorithm.cpp:141-336).  The handle's weights are
 * left as they were.  (tests/test_gpu_parity.py pins it to the reference's BruteForceLinearAssignment fixture.) */
int rfsgpu_murty_partition_sums(rfsgpu_filter *f, const double *mats, const int *nR, const int *nC, int n_jobs, double *sums_out);
/* [test] The partition stage of the particle weight (connected components of the likelihood table, the zero-partition merge and its
 * indexing quirk, the <= 8 enumeration, the exact mode, the Murty-200 jobs: include/RBPHDFilter.hpp:865-990) on n_tables given
 * likelihood tables by the weighting kernels' own device function, one wavefront per table; table k plays particle k
 * (n_tables <= the handle's particle count).  Table k is nE[k] x nZ[k] row-major, already gated and including Pd; the tables lie
 * back to back in L, the evaluation points' Pd (nE[k] each) back to back in pd; 0 <= nE[k], nZ[k] <= 64.  The handle's partition
 * mode and Murty queue are used and its post kernel multiplies the Murty factors in, as in a step.  out[k] = the product over the
 * visited partitions, before the division by the clutter integral.  The handle's weights are left as they were; a table the
 * step would refuse (a Murty partition beyond 64) gives RFSGPU_ERR_UNSUPPORTED and no numbers. */
int rfsgpu_partition_likelihoods(rfsgpu_filter *f, const double *L, const double *pd, const int *nE, const int *nZ, int n_tables,
                                 double clutter, double *out);
int rfsgpu_update_map(rfsgpu_filter *f, const double *z, int n_z);      /* updateMap       :543-725 */
int rfsgpu_importance_weighting(rfsgpu_filter *f);                       /* importanceWeighting :728-997 */
int rfsgpu_merge(rfsgpu_filter *f);                                      /* GaussianMixture::merge  GaussianMixture.hpp:394-475 */
int rfsgpu_prune(rfsgpu_filter *f);                                      /* GaussianMixture::prune  :477-534 */

/* unused_measurements_[slot] (:709-720) as indices in ascending order; returns count via *n_out. */
int rfsgpu_get_unused(rfsgpu_filter *f, int slot, int *idx, int max_n, int *n_out);
/* nLandmarksInFOV_[slot] (:601-613). */
int rfsgpu_landmarks_in_fov(rfsgpu_filter *f, int slot, int *n_out);

/* ---- [core] resampling, [multi] weight normalisation (ParticleFilter.hpp:352-363, 399-492) ---------------- */

/* Device reduction of this shard's {sum w, sum w^2}; out[2] on the host. */
int rfsgpu_weight_sums(rfsgpu_filter *f, double *out);
/* Device pointer to the same two doubles (valid after rfsgpu_weight_sums_async) so a multi-GPU
 * host can all-reduce them in place over RCCL without a host round trip. */
int rfsgpu_weight_sums_async(rfsgpu_filter *f);
void *rfsgpu_weight_sums_device_ptr(rfsgpu_filter *f);
/* w_i /= sum (sum = global sum over all shards).  If sum_dev != NULL the divisor is read on the
 * device from sum_dev[0] (after an in-place all-reduce) and `sum` is ignored. */
int rfsgpu_normalize_weights(rfsgpu_filter *f, double sum, const void *sum_dev);
/* The same when several shards (handles on one GPU and / or other GPUs) share the normalisation: sum_dev points to
 * n_parts consecutive {sum w, sum w^2} pairs (each shard's rfsgpu_bind_weight_sums_buffer slot, all-reduced in place
 * across GPUs); the divisor is the sum of their first elements, added in index order on the device. */
int rfsgpu_normalize_weights_parts(rfsgpu_filter *f, double sum, const void *sum_dev, int n_parts);
/* Apply a resampling decision (the copy loop of ParticleFilter::resample, include/ParticleFilter.hpp:446-479): slot k takes what
 * Particle::copy (include/Particle.hpp:218-223) carries from slot src_slot[k] -- the pose and a deep copy of the mixture -- and its
 * id; src_slot[k] == k keeps the slot (case 1, :466-467).  All weights are reset to 1 (:486-489).  Sources must be slots that
 * keep themselves.  The engine keeps the particles' id_ / idParent_ per slot exactly as that loop leaves them (a copy has its
 * SOURCE's id; idParent_ = the source's id; a survivor's idParent_ = its own id, which differs from its slot once it has been
 * a copy itself) and remembers that a resampling occurred (RBPHDFilter::resampleOccured_, cleared by the next update with
 * measurements, include/RBPHDFilter.hpp:526).  What happens to the three per-SLOT arrays of RBPHDFilter -- unused_measurements_,
 * birthGaussians_, nLandmarksInFOV_ -- is selected by rfsgpu_set_birth_inheritance (below).
 * Stream-ordered since round 6: src_slot is copied before the call returns, the device copy is enqueued behind whatever is on the handle's
 * stream and nothing waits for it (every reader of maps / weights does, on that stream); TimingInfo's particleResample buckets hold the
 * host time of the call. */
int rfsgpu_resample_apply(rfsgpu_filter *f, const int *src_slot);
/* Birth-state inheritance after a resampling (include/RBPHDFilter.hpp:1005-1011).
 *   RFSGPU_INHERIT_REFERENCE (default)  the reference, statement for statement: nothing but pose + mixture moves at resampling
 *       time; every rfsgpu_predict_map(add_birth = 1) while resampleOccured_ is set walks the slots in ascending order and, where
 *       idParent_ != slot, first copies unused_measurements_ and birthGaussians_ from SLOT idParent_ in the state that slot is
 *       in at that moment (a lower slot has already been through this predict's birth step, so its unused list is empty and
 *       its candidates are one check older; a higher slot has not), then runs the slot's own birth step.  nLandmarksInFOV_ is
 *       never copied.  On the device: a snapshot-ordered gather for the children of higher slots, then the birth step level by
 *       level along the chains of lower-slot parents (csrc/birth.h).
 *   RFSGPU_INHERIT_EAGER      rounds 1-2 of this engine ("the evident intent"): a child takes its parent's unused list, FOV count
 *       and candidate list at resampling time, predict copies nothing.  NOT the reference's results in the step after a
 *       resampling.  A handle on which rfsgpu_fastslam_update has run behaves this way whatever the mode: rfs::FastSLAM copies its
       landmark-candidate lists right at resampling time (FastSLAM::resampleWithMapCopy, include/FastSLAM.hpp:747-753).
 *   RFSGPU_INHERIT_EXTERNAL   resampling moves pose + mixture only and predict copies nothing: the host owns the rule (the
 *       multi-GPU hosts, whose parent slot may live on another shard: rfsgpu_get/set_unused_masks).
 * The environment variable RFSGPU_BIRTH_INHERITANCE=eager makes RFSGPU_INHERIT_EAGER the initial mode of new handles (A/B runs
 * of unmodified hosts). */
#define RFSGPU_INHERIT_REFERENCE 0
#define RFSGPU_INHERIT_EAGER 1
#define RFSGPU_INHERIT_EXTERNAL 2
int rfsgpu_set_birth_inheritance(rfsgpu_filter *f, int mode);
int rfsgpu_get_birth_inheritance(const rfsgpu_filter *f);
/* Particle::getId / getParentId of the particle in every slot (either pointer may be NULL); set: for a host that keeps the ids
 * itself (the sharded hosts: ids are GLOBAL slot numbers there). */
int rfsgpu_get_particle_ids(rfsgpu_filter *f, int *id, int *parent_id);
int rfsgpu_set_particle_ids(rfsgpu_filter *f, const int *id, const int *parent_id);
/* RBPHDFilter::resampleOccured_ as the engine tracks it (1 / 0). */
int rfsgpu_resample_occured(const rfsgpu_filter *f);
/* unused_measurements_ of all slots at once, one 64-bit mask per slot (bit z = measurement z of the last update is unused). */
/* [multi] One level of the level-ordered birth step, for a host that carries out the reference's slot-ordered copy of the per-slot
 * birth lists itself because parent slots live on other shards (ids are global there): the birth step runs for the slots whose
 * level_of_slot[] == level; the static step of every Gaussian in the call with do_static != 0 (births of later calls get their
 * + Q where they are created).  Between the calls the host moves lists with rfsgpu_get/set_unused_masks and
 * rfsgpu_export/import_birth_candidates (rfs-slam_amd/sharded.py, rfsgpu_group_predict_map). */
int rfsgpu_predict_map_level(rfsgpu_filter *f, int add_birth, const int *level_of_slot, int level, int do_static);
int rfsgpu_get_unused_masks(rfsgpu_filter *f, unsigned long long *masks);   /* a read: does NOT acknowledge the rule to an EXTERNAL-mode handle */
int rfsgpu_set_unused_masks(rfsgpu_filter *f, const unsigned long long *masks);
/* [multi] 1 if this handle has ever held birth-candidate lists (birthGaussians_, include/RBPHDFilter.hpp:1014-1083: a configuration
 * that keeps them has run a birth predict, or lists were imported with rfsgpu_import_birth_candidates), else 0; -1 for a null
 * handle.  The multi-GPU hosts take the closed form of the inheritance rule over the unused masks only while this is 0 on
 * EVERY shard (rfsgpu_group_predict_map and rfs-slam_amd/sharded.py use this one predicate). */
int rfsgpu_has_birth_candidates(const rfsgpu_filter *f);
/* ParticleFilter::resample(n) with n < nParticles_ (:417-483; FastSLAM::resampleWithMapCopy): the first n_out slots
 * receive src_slot[0..n_out), the particle count becomes n_out.  A source below n_out must keep itself; sources at or
 * beyond n_out are dropped after the copy. */
int rfsgpu_resample_apply_n(rfsgpu_filter *f, const int *src_slot, int n_out);

/* ---- [multi] cross-shard migration for GLOBAL resampling over several GPUs ---------------------------------------
 * The reference resamples over the whole particle set (ParticleFilter::resample, include/ParticleFilter.hpp:399-492) and a
 * child is a deep copy of its parent (Particle::copy, include/Particle.hpp:218-223: pose + mixture).  When parent and child
 * live on different GPUs the parent travels as one packed ROW of rfsgpu_slab_row_bytes() bytes -- pose (+ covariance) and
 * mixture; with RFSGPU_INHERIT_EAGER (and on FastSLAM handles) also the unused-measurement list, FOV count and birth candidates --
 * between DEVICE buffers: export on the source handle, transport by the caller (RCCL send/recv between processes,
 * hipMemcpyPeerAsync inside one process: rfsgpu_group_*), import on the destination handle.  Both calls are stream-ordered
 * on the handle's stream and never synchronise the host; `slots` is a host array that is free again on return.
 * Rows are only meaningful between handles of the same model and gm_capacity. */
size_t rfsgpu_slab_row_bytes(const rfsgpu_filter *f);
int rfsgpu_export_slab_rows(rfsgpu_filter *f, const int *slots, int n, void *dev_rows);        /* rows[k] <- particle slots[k] */
int rfsgpu_import_slab_rows(rfsgpu_filter *f, const int *slots, int n, const void *dev_rows);  /* particle slots[k] <- rows[k] */
/* Device pointer of the N particle weights (for an all-gather that stays on the GPUs); valid for the handle's lifetime. */
void *rfsgpu_weights_device_ptr(rfsgpu_filter *f);

/* ---- [multi] one filter over several GPUs from ONE host thread (SURVEY 8(b) "device_ids[], n_dev"; 8(e)) ------------------------
 * The particle set of rfs::RBPHDFilter is cut into contiguous blocks, one shard (an rfsgpu_filter) per listed device.  What a
 * C++ host standing where rfs::RBPHDFilter stands needs to use more than one GPU:
 *   predict / update / normalise / resample over the whole set, configuration broadcast to all shards, map access by global
 *   particle index.  Shards run their fused steps concurrently; they meet in the weight normalisation (an RCCL all-reduce of
 *   {sum w, sum w^2} on the shards' streams -- single-process communicators from ncclCommInitAll, librccl loaded with dlopen -- or,
 *   with repeated device ids, per-shard sums added on the host in shard order) and in resampling, which stays GLOBAL (ParticleFilter::resample, include/ParticleFilter.hpp:399-492):
 *   cross-device children travel as packed rows with hipMemcpyPeerAsync (rfsgpu_export/import_slab_rows).
 * device_ids may repeat a device (several shards on one GPU: how the single-GPU tests drive this code). */
typedef struct rfsgpu_group rfsgpu_group;
int rfsgpu_group_create(rfsgpu_group **out, int model, int n_particles, const int *device_ids, int n_dev, int gm_capacity);
void rfsgpu_group_destroy(rfsgpu_group *g);
const char *rfsgpu_group_last_error(const rfsgpu_group *g);
int rfsgpu_group_n_shards(const rfsgpu_group *g);
int rfsgpu_group_n_particles(const rfsgpu_group *g);
rfsgpu_filter *rfsgpu_group_shard(rfsgpu_group *g, int k);                    /* the shard's own handle (map import/export, timing) */
int rfsgpu_group_locate(const rfsgpu_group *g, int particle, int *shard, int *slot);
int rfsgpu_group_set_filter_config(rfsgpu_group *g, const rfsgpu_filter_config *c);
int rfsgpu_group_set_model_rngbrg(rfsgpu_group *g, const rfsgpu_rngbrg_config *c);
int rfsgpu_group_set_kf_config(rfsgpu_group *g, const rfsgpu_kf_config *c);
int rfsgpu_group_set_lmk_process_noise(rfsgpu_group *g, const double *Q);
int rfsgpu_group_set_model_victoriapark(rfsgpu_group *g, const rfsgpu_vp_config *c);   /* configs[3] sharded: the 3-D model on every shard */
int rfsgpu_group_set_laser_scan(rfsgpu_group *g, const double *scan, int n);
int rfsgpu_group_set_phase_timing(rfsgpu_group *g, int on);
/* RBPHDFilter::TimingInfo of the group: *_wall = the largest of the shards' (they run side by side), *_cpu = their sum. */
int rfsgpu_group_get_timing(rfsgpu_group *g, rfsgpu_timing *t);
/* How the shards' weight sums meet: "rccl" (all-reduce over RCCL / xGMI on the shards' streams, totals stay on the devices) or
 * "host: <why>" (repeated device ids, RFSGPU_GROUP_RCCL=0, librccl not loadable ...: pairs added on the host in shard order). */
const char *rfsgpu_group_collective(const rfsgpu_group *g);
int rfsgpu_group_set_poses(rfsgpu_group *g, const double *x, const double *cov, int cov_stride);   /* N poses, as rfsgpu_set_poses */
int rfsgpu_group_get_poses(rfsgpu_group *g, double *x);
int rfsgpu_group_set_weights(rfsgpu_group *g, const double *w);
int rfsgpu_group_get_weights(rfsgpu_group *g, double *w);
/* RBPHDFilter::predict, map part (:415-442), incl. the reference's birth-state inheritance after a resampling over GLOBAL slots:
 * a gather over the unused masks for immediate-birth configurations (birthGaussianMeasurementCountThreshold == 1), the
 * level-ordered walk with the lists moved between shards for configurations that keep candidate lists. */
int rfsgpu_group_predict_map(rfsgpu_group *g, int add_birth);
int rfsgpu_group_set_birth_inheritance(rfsgpu_group *g, int mode);          /* RFSGPU_INHERIT_REFERENCE (default) | RFSGPU_INHERIT_EAGER */
int rfsgpu_group_get_particle_ids(rfsgpu_group *g, int *id, int *parent_id); /* Particle::getId / getParentId by global slot */
/* RBPHDFilter::update body (:444-523) on every shard; weights stay un-normalised; sums_out (may be null) = {sum w, sum w^2}. */
int rfsgpu_group_update(rfsgpu_group *g, const double *z, int n_z, double *sums_out);
/* rfsgpu_group_update whose weight normalisation trails by one step (RCCL path: the all-reduce of {sum w, sum w^2} on a side stream
 * per shard beside the next step's kernel; each shard's post kernel divides by the previous call's total, rfsgpu_step_async_deferred).
 * Nothing waits for the GPUs; the next rfsgpu_group_* call that reads or replaces the weights applies the pending total first.
 * For steps after which the host does not need N_eff (the resample test is not due). */
int rfsgpu_group_update_deferred(rfsgpu_group *g, const double *z, int n_z);
/* The group form of rfsgpu_update_io: global poses (+ covariances, NULL = unchanged) and weights (NULL = unchanged) in, the update on every
 * shard (all chains enqueued before the first wait), the updated un-normalised weights of all particles out (NULL = not wanted);
 * device-side errors of any shard are reported by this call. */
int rfsgpu_group_update_io(rfsgpu_group *g, const double *x, const double *x_cov, int cov_stride, const double *w_in, const double *z, int n_z, double *w_out);
int rfsgpu_group_normalize(rfsgpu_group *g, double *sums_out);               /* normalizeWeights over all N (:352-363) */
/* ParticleFilter::resample (:399-492) with the caller's uniform draw (the reference's one drand48()); *fired tells whether the
 * N_eff test let it happen; plan_out (may be null, N ints): global source slot of every slot, for per-particle host data. */
int rfsgpu_group_resample(rfsgpu_group *g, double eff_n_threshold, double u01, int *fired, int *plan_out);
int rfsgpu_group_apply_plan(rfsgpu_group *g, const int *src);                /* a resampling plan computed elsewhere */
int rfsgpu_group_migration_stats(const rfsgpu_group *g, long long *rows, long long *bytes);
int rfsgpu_group_gm_size(rfsgpu_group *g, int particle);                     /* getGMSize, global index */
int rfsgpu_group_get_landmark(rfsgpu_group *g, int particle, int m, double *mean, double *cov, double *w);
int rfsgpu_group_synchronize(rfsgpu_group *g);

/* ---- [core] timing, [bench] / misc ---------------------------------------------------------------------------- */

/* getTimingInfo (:1219-1232).  The device buckets (mapUpdate_wall, ...) come from HIP events, and on the fused one-launch step those
 * events ride on every 8th step only (three marker packets per step cost a configs[1] step 8 us): a SAMPLED step is booked once for
 * itself and once for every un-sampled step since the previous sample, and un-sampled steps behind the last sample are booked at
 * that sample's duration at the next synchronising call -- so the bucket covers every step, as an estimate, not a per-step
 * measurement like the reference's timer_mapUpdate_.  rfsgpu_set_step_timing_stride(f, 1) (bench API) or rfsgpu_set_phase_timing
 * (per-phase launches with their own event pairs) give measured per-step values. */
int rfsgpu_get_timing(rfsgpu_filter *f, rfsgpu_timing *t);
int rfsgpu_reset_timing(rfsgpu_filter *f);
/* Block until all queued device work of this handle is complete; reports a pending device-side error of async steps. */
int rfsgpu_synchronize(rfsgpu_filter *f);
/* Native HIP stream of this handle (hipStream_t as void*), for callers that enqueue around it. */
void *rfsgpu_stream(rfsgpu_filter *f);
/* Run this handle's kernels on a caller-owned stream (e.g. the host framework's current stream) so
 * that collectives / events of the caller order against the engine without host round trips.
 * NULL restores the engine's own stream. */
int rfsgpu_set_stream(rfsgpu_filter *f, void *hip_stream);
/* Let rfsgpu_weight_sums_async write {sum w, sum w^2} into a caller-owned device buffer (2 doubles),
 * e.g. a tensor the multi-GPU host all-reduces in place over RCCL.  NULL restores the internal one. */
int rfsgpu_bind_weight_sums_buffer(rfsgpu_filter *f, void *dev_ptr);
#ifdef RFSGPU_ENABLE_BENCH_API   /* [bench] / [test]: exported by the library, declared only for callers that ask (bench.py, the tests) */
/* Device-side snapshot / restore of the MAP state of every particle (mixtures, sizes, particle weights, unused-measurement
 * lists, FOV counts): one snapshot slot per handle, allocated on first use.  A benchmarking / testing helper -- it is how a
 * timed step is re-seeded -- NOT a checkpoint: poses, the birth-candidate lists and the staged measurement set are not part of
 * it (callers that use candidate lists re-import them).  The reference has no equivalent (it has no checkpointing at all). */
int rfsgpu_save_state(rfsgpu_filter *f);
int rfsgpu_restore_state(rfsgpu_filter *f);
/* A ring of n_slots pre-seeded copies of the saved state, so that the input of every timed step is resident in HBM BEFORE the timed
 * region instead of being copied inside it (restore_state is a 45 MB copy per step at configs[1]).  _create allocates and fills the
 * slots from the snapshot (rfsgpu_save_state first; 0 frees the ring); _next makes the next slot the handle's current state by
 * swapping device pointers -- host work only, nothing is launched; a slot is consumed by the step that runs on it, _next past the
 * last slot is an error, _seed fills all slots again.  A swap moves the handle's weight array: a pointer obtained from
 * rfsgpu_weights_device_ptr before it is stale afterwards.  Results are those of rfsgpu_restore_state + the same step
 * (tests/test_gpu_parity.py::test_state_ring_steps_equal_restore_and_step). */
int rfsgpu_state_ring_create(rfsgpu_filter *f, int n_slots);
int rfsgpu_state_ring_seed(rfsgpu_filter *f);
int rfsgpu_state_ring_next(rfsgpu_filter *f);
/* Duration in ns of the most recent launch of each hot-path kernel, from HIP events on the
 * engine's stream: [0]=phd_update_map [1]=phd_weight_multifeature [2]=gm_merge [3]=gm_prune. */
int rfsgpu_last_kernel_ns(rfsgpu_filter *f, long long *ns4);
/* [test] Which instantiation the last stream-ordered step (rfsgpu_update / _update_async / _step_async) launched: out4 = {waves per
 * particle of the fused step kernel, phase priorities on (1 / 0), log2 of the merge grid's side (5 | 6), fused (1) or three
 * kernels (0)} -- so that the full-size parity tests can say which kernel they checked (phd_step_fused_kernel<2, true, 5> is the
 * one bench.py times at configs[1]). */
int rfsgpu_last_step_variant(const rfsgpu_filter *f, int *out4);
#endif /* RFSGPU_ENABLE_BENCH_API */

/* MatPerm::calc (src/MatrixPermanent.cpp:41-112), batched: `batch` row-major n x n matrices in A
 * (host), permanents to out (host).  n <= 24.  Standalone (no filter handle needed). */
int rfsgpu_mat_perm(const double *A, int n, int batch, double *out, int device_id);
#ifdef RFSGPU_ENABLE_BENCH_API
/* [bench] Device time (ms, HIP events) of the kernel of the last rfsgpu_mat_perm call of this process. */
double rfsgpu_mat_perm_last_kernel_ms(void);
#endif

/* ---- [fastslam] FastSLAM 1.0 on the same handle (reference include/FastSLAM.hpp) --------------------------------
 * The handle's mixtures double as FastSLAM's per-particle landmark maps: a Gaussian's weight is the landmark's
 * log-odds of existence (FastSLAM.hpp:598-617), the birth-candidate lists are the landmark candidates
 * (landmarkCandidates_, :84-88).  Both measurement models.  The map part of FastSLAM::predict (:376-383, staticStep on
 * every landmark) is rfsgpu_predict_map(f, 0). */
void rfsgpu_default_fastslam_config(rfsgpu_fastslam_config *cfg);                       /* constructor defaults :243-257 */
int rfsgpu_set_fastslam_config(rfsgpu_filter *f, const rfsgpu_fastslam_config *cfg);    /* public member `config`        */
int rfsgpu_get_fastslam_config(const rfsgpu_filter *f, rfsgpu_fastslam_config *cfg);
/* FastSLAM::updateMap for every particle (:387-418, 424-706): in-range landmarks, log-likelihood table, CostMatrix::reduce +
 * best data association, Kalman correction of the associated landmarks, existence log-odds, pruning, new landmarks /
 * candidates from the unassociated measurements, particle weight *= exp(sum of the associated log-likelihoods).
 * n_z == 0 returns OK without touching anything (:401-402).  resampleWithMapCopy (:708-735) stays with the caller
 * (rfsgpu_weight_sums / rfsgpu_normalize_weights / rfsgpu_resample_apply[_n]).
 * Multi-hypothesis FastSLAM (config.maxNDataAssocHypotheses in 2..16): every particle keeps Murty's k best associations
 * within maxDataAssocLogLikelihoodDiff of the best and is copied once per extra hypothesis (:506-556,
 * ParticleFilter::copyParticle): the particle set GROWS (rfsgpu_n_particles; room from rfsgpu_create_ex, else
 * RFSGPU_ERR_CAPACITY).  The copies are appended in particle order; rfsgpu_particle_parents tells the host which slot each
 * particle was copied from (itself for the originals) so that it can duplicate its poses.  Limit of this path: landmarks in
 * range and measurements <= 64 each (Murty runs on the dense reduced table like the reference). */
int rfsgpu_fastslam_update(rfsgpu_filter *f, const double *z, int n_z);
/* FastSLAM::resampleOccured_ (whether the previous update ended in a resampling): decides if the copies of a multiplied
 * particle inherit its landmark candidates (:551-553).  The host mirror sets it after its resampleWithMapCopy. */
int rfsgpu_fastslam_set_resample_occured(rfsgpu_filter *f, int flag);
/* parent[k] = the slot particle k was copied from by the last rfsgpu_fastslam_update (k itself when it was not a copy). */
int rfsgpu_particle_parents(rfsgpu_filter *f, int *parent, int max_n);

/* -- the whole FastSLAM::update on the device, without a host stop (outside the STABLE CORE) --
 * rfsgpu_fastslam_update stops in the middle of a multi-hypothesis update (the hypothesis counts come back, the host lays out the
 * copies) and leaves resampleWithMapCopy to the caller.  rfsgpu_fastslam_cycle_async enqueues one whole FastSLAM::update
 * (FastSLAM.hpp:387-421) on the handle's stream and returns without synchronising: with `predict`, the static landmark step of
 * FastSLAM::predict (:376-383, what rfsgpu_predict_map_async(f, 0) does); the association (Murty's k best with
 * maxNDataAssocHypotheses > 1; 1 runs the same pipeline with one hypothesis); the particle copies, laid out on the device in the
 * reference's order; Kalman correction, existence, weights; pruning and new landmarks; and resampleWithMapCopy (:729-757): forced
 * down to n_init when the grown count exceeds nParticlesMax, else -- once minUpdatesBeforeResample / minMeasurementsBeforeResample
 * are met -- ParticleFilter::resample(n_init) with its N_eff test (thresholds: rfsgpu_fastslam_set_resampling); weights 1 after a
 * resampling, normalised otherwise.  u01 in [0, 1) is the caller's draw for the systematic plan (the reference's drand48()).  n_init:
 * nParticles_init_ (0: the count stays).  n_z == 0 returns after counting the update (:399-402).  The two counters and
 * resampleOccured_ live on the device for this route (resampleOccured_ starts from rfsgpu_fastslam_set_resample_occured's value).
 *
 * After the call the particle count is known to the device only.  rfsgpu_synchronize and every call that reads or sizes by the count
 * (rfsgpu_n_particles, the getters and setters, exports, ...) first wait for the stream and take the count over; a further
 * rfsgpu_fastslam_cycle_async does not (it is launched at max_particles and reads the count on the device), so cycles can be enqueued
 * back to back.  A grown set that would exceed max_particles abandons its cycle and every cycle enqueued behind it: the state stays
 * what it was before that cycle, and the next synchronising call returns RFSGPU_ERR_CAPACITY once.
 *
 * RFSGPU_ERR_UNSUPPORTED, state untouched: batch handles, shards of a group, the Victoria Park model, landmark candidate lists
 * (landmarkCandidateMeasurementCountThreshold != 1), maxNDataAssocHypotheses outside [1, 16], rfsgpu_max_particles(f) >
 * RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES (the resampling kernel holds the whole filter in LDS). */
#define RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES 2048
int rfsgpu_fastslam_cycle_async(rfsgpu_filter *f, int predict, const double *z, int n_z, double u01, int n_init);
/* The same cycle for either model and with landmark candidate lists: the rules above (the counters and the overflow word on the
 * device, cycles enqueued back to back, rfsgpu_fastslam_last_cycle for the results), and in addition
 *  - RFSGPU_MODEL_VICTORIAPARK_3D is served, z is then [n_z][3];
 *  - any landmarkCandidateMeasurementCountThreshold is served: the candidate lists are walked by the new-landmark step, travel with
 *    the copies of a multiplied particle exactly when the previous cycle resampled (FastSLAM.hpp:551-553), and with every
 *    resampling copy.  A 65th candidate of a particle, or a map beyond gm_capacity, is reported by the next synchronising call
 *    (RFSGPU_ERR_UNSUPPORTED / RFSGPU_ERR_CAPACITY), as rfsgpu_fastslam_update reports them;
 *  - scan [n_scan] is the laser scan of this update (setLaserScan), or NULL to leave the scan as it is.  It goes through the pinned
 *    staging ring of rfsgpu_set_step_inputs_async without a wait for the device; the clutter density is computed from it on the
 *    host, as rfsgpu_set_laser_scan computes it, and travels by value with the launches.  The Victoria Park model with no scan ever
 *    set: RFSGPU_ERR_INVALID;
 *  - maxNDataAssocHypotheses == 1 associates as rfsgpu_fastslam_update does for one hypothesis (the sparse table and the
 *    per-component assignment of the single-hypothesis path, no limit of 64 landmarks in range), so the two routes give the same
 *    bits for every configuration; rfsgpu_fastslam_cycle_async runs the multi-hypothesis pipeline with a limit of one.
 * RFSGPU_ERR_UNSUPPORTED, state untouched: batch handles, shards of a group, maxNDataAssocHypotheses outside [1, 16],
 * rfsgpu_max_particles(f) > RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES.
 *
 * While cycles of either call are pending, rfsgpu_propagate_ackerman_async, rfsgpu_propagate_ackerman_run_async,
 * rfsgpu_static_steps_async and rfsgpu_set_step_inputs_async with x == NULL enqueue behind them without taking the count over:
 * their kernels are launched at max_particles and read the count and the overflow word on the device (a propagation behind an
 * abandoned cycle is abandoned with it).  The generator's counter stays (slot, call).  rfsgpu_set_step_inputs_async with poses
 * still waits: it sizes a host buffer by the count. */
int rfsgpu_fastslam_cycle_full_async(rfsgpu_filter *f, int predict, const double *z, int n_z, const double *scan, int n_scan, double u01,
                                     int n_init);
/* How many cycles with measurements have completed on this handle and how many of them resampled (synchronises): for a host that
 * enqueues a whole run and reads nothing in between.  Abandoned cycles are not counted.  Either pointer may be NULL. */
int rfsgpu_fastslam_cycle_counts(rfsgpu_filter *f, int *n_cycles, int *n_resamplings);
#ifdef RFSGPU_ENABLE_BENCH_API   /* [test]: 1 while the particle count is the device's (cycles are pending); reads nothing, waits for nothing */
int rfsgpu_fastslam_cycle_pending(rfsgpu_filter *f);
/* [test]: one slot's weight, mixture size, candidate count and first Gaussian (entry 0 of every plane: gauss [7], or [11] for the
 * Victoria Park model), read (write == 0) or written for any slot below rfsgpu_max_particles(f), live or not.  Synchronises. */
int rfsgpu_debug_slot(rfsgpu_filter *f, int slot, int write, double *weight, int *count, int *cand_count, double *gauss);
#endif /* RFSGPU_ENABLE_BENCH_API */
/* What the last rfsgpu_fastslam_cycle_async did (synchronises): the count after its update, the count after its resampling, whether
 * that fired, N_eff (0 where the test did not run), parent[k] of the update for the *n_after_update grown slots (what
 * rfsgpu_particle_parents gives after rfsgpu_fastslam_update), plan[k] for the *n_after_resample slots (the slot -- of the grown set
 * -- that slot k now holds a copy of; k itself where it kept its particle or nothing fired).  Any pointer may be NULL; max_n: entries
 * of parent and plan.  A cycle without measurements reports the unchanged count, identity arrays and no resampling. */
int rfsgpu_fastslam_last_cycle(rfsgpu_filter *f, int *n_after_update, int *n_after_resample, int *fired, double *n_eff, int *parent,
                               int *plan, int max_n);
/* ParticleFilter::resample's thresholds for rfsgpu_fastslam_cycle_async: no resampling while N_eff > eff_n && N_eff / n >
 * eff_n_percent.  Default: n_particles / 4 and 0.25 (ParticleFilter.hpp:232-233). */
int rfsgpu_fastslam_set_resampling(rfsgpu_filter *f, double eff_n, double eff_n_percent);

/* ---- [batch] many independent 2-D RB-PHD or FastSLAM filters in one handle (outside the STABLE CORE) -------------------------
 * A batch handle holds n_filters independent range-bearing filters of n_per_filter particles each, stepped together: one cycle is
 * one fused step launch + one post launch for all of them.  Particle slots are global -- filter b owns slots
 * [b * n_per_filter, (b + 1) * n_per_filter) -- so the per-slot calls work unchanged (rfsgpu_set_poses, rfsgpu_get_weights,
 * rfsgpu_gm_size(s), rfsgpu_get_landmark, rfsgpu_export_gm, rfsgpu_get_unused, particle ids).  Each filter has its own configuration,
 * measurement set, weights, normalisation, resampling and resampleOccured_; each equals a separate handle given the same inputs.
 * The whole-handle setters (rfsgpu_set_filter_config, _set_model_rngbrg, _set_kf_config, _set_lmk_process_noise) set every filter.
 * Not on a batch handle (RFSGPU_ERR_UNSUPPORTED, with a rfsgpu_last_error message): the Victoria Park model, rfsgpu_set_laser_scan
 * and rfsgpu_import_birth_candidates on a 2-D batch (a batch of Victoria Park filters has them: see below), the single-handle
 * FastSLAM calls (rfsgpu_set_fastslam_config, rfsgpu_fastslam_update: a batch of FastSLAM filters has
 * rfsgpu_batch_set_fastslam_config / rfsgpu_batch_fastslam_cycle_async below), multi-hypothesis FastSLAM and landmark candidate
 * lists (count threshold != 1), rfsgpu_update* and the phase calls, rfsgpu_step_async*, rfsgpu_cycle_async, rfsgpu_predict_map*,
 * the collective calls, rfsgpu_resample_apply[_n], rfsgpu_weight_sums[_async], rfsgpu_normalize_weights[_parts] (one total for all
 * filters: rfsgpu_batch_weight_sums and the cycle's normalize instead), rfsgpu_import_birth_candidates, birth inheritance modes other
 * than RFSGPU_INHERIT_REFERENCE, and configurations with birthGaussianMeasurementCountThreshold != 1 (the births are immediate).
 * rfsgpu_resample_occured returns -1 on a batch (rfsgpu_batch_resample_occured has the per-filter flags).
 * Groups (rfsgpu_group_*) create their own handles and are not batches.  Limits per filter: RFSGPU_MAX_Z, RFSGPU_MAX_EVAL,
 * gm_capacity.  Shared by the whole batch: the Murty-200 job queue (4 jobs per particle of the batch, at most 8192 -- fewer in all
 * than the same filters get as separate handles, so a dense sweep can overflow it where the handles would not) and the device error
 * word: rfsgpu_last_error names a filter that exceeded gm_capacity (the lowest such filter) or asks for more than RFSGPU_MAX_EVAL
 * evaluation points; a Murty error is not attributed. */
int rfsgpu_create_batch(rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int device_id, int gm_capacity);
int rfsgpu_n_filters(const rfsgpu_filter *f);    /* 1 for an ordinary handle */
/* Filter `filter`'s configuration; a NULL pointer leaves that part as it is.  lmk_Q: the 2x2 landmark process noise, row-major. */
int rfsgpu_batch_configure(rfsgpu_filter *f, int filter, const rfsgpu_filter_config *cfg, const rfsgpu_rngbrg_config *model,
                           const rfsgpu_kf_config *kf, const double *lmk_Q);
/* rfsgpu_cycle_async for every filter at once (predict as there; x [N][3], x_cov [9] or [N][9] by cov_stride, or NULL).
 * z: [n_filters][RFSGPU_MAX_Z][2], n_z: [n_filters].  A filter with n_z == 0 is not updated this cycle (its predict part runs, its
 * weights are summed and divided as asked).  normalize != 0: each filter's weights are divided by their own sum. */
int rfsgpu_batch_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride,
                             const double *z, const int *n_z, int normalize);
/* -- a batch of Victoria Park RB-PHD filters: rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D (rfsgpu_create_batch_mh still
 * refuses the model).  Each filter equals a separate Victoria Park handle given the same inputs: its own rfsgpu_filter_config with
 * ANY birth thresholds (the birth-candidate lists are per slot, as on a handle), its own rfsgpu_vp_config, Kalman thresholds,
 * landmark noise, measurement set and count per cycle.  All filters see the same dataset: the laser scan is the handle's
 * (rfsgpu_set_laser_scan, rfsgpu_set_step_inputs_async, or the cycle call's scan) and each filter's clutter density is derived from
 * it with the filter's own expectedClutterNumber, by rfsgpu_set_laser_scan's rule.  rfsgpu_set_lmk_process_noise sets every
 * filter's Q (and nothing else of its configuration); rfsgpu_set_model_victoriapark sets every filter's model;
 * rfsgpu_static_steps_async serves the batch as it serves a handle.  The host-stop route: rfsgpu_batch_weight_sums,
 * rfsgpu_batch_resample_apply (pose and mixture move; the birth state follows lazily in the next birth predicts of a filter that
 * resampled, level by level as on a handle, until its next update with measurements) and rfsgpu_batch_resample_occured work as on a
 * 2-D batch, and so do the per-slot getters and setters, rfsgpu_export / _import_birth_candidates and rfsgpu_get / _set_unused_masks
 * included.  The device route, on which nothing is read back between the messages of a run: rfsgpu_batch_vp_set_motion,
 * _vp_set_resampling, _vp_propagate_run_async, _vp_resample_async, _vp_last_resample and _vp_loop_counts, below the 2-D device loop.
 * RFSGPU_ERR_UNSUPPORTED on such a batch, with a message and the state untouched: rfsgpu_batch_cycle_async, the FastSLAM
 * and multi-hypothesis batch calls, the 2-D device loop (rfsgpu_batch_set_motion_odometry, _set_resampling, _propagate_async,
 * _resample_async, _last_resample, _resample_counts), [sensor], [truth], [metric] and rfsgpu_rbphd_cycle_async -- fifteen standing
 * refusals -- and, until rfsgpu_batch_vp_serve_estimates(f, 1) switches it on for the batch, [estimate] (with the switch on, the four
 * log calls of that section serve the batch on both routes; rfsgpu_batch_run_log_estimates stays refused).  rfsgpu_batch_vp_serve_fastslam(f, 1), below the cycle call, makes such a batch step
 * FastSLAM filters instead; until then the FastSLAM calls stay refused as listed.  rfsgpu_batch_configure on such a batch,
 * and rfsgpu_batch_configure_vp on a 2-D batch, return RFSGPU_ERR_INVALID.  rfsgpu_last_error names the lowest filter that exceeded
 * gm_capacity, and for a full candidate list (RFSGPU_MAX_CANDIDATES) the lowest filter with a slot whose list, with the unused
 * measurements that could join it, stood beyond the limit in a birth predict that reported one: the filter at fault where one
 * filter is near the limit; where several are, possibly a lower one that stayed just inside it.
 *
 * Filter `filter`'s configuration; a NULL pointer leaves that part as it is.  lmk_Q: the 3x3 landmark process noise, row-major. */
int rfsgpu_batch_configure_vp(rfsgpu_filter *f, int filter, const rfsgpu_filter_config *cfg, const rfsgpu_vp_config *model,
                              const rfsgpu_kf_config *kf, const double *lmk_Q);
/* rfsgpu_cycle_async for every filter of a Victoria Park batch at once.  predict, x, x_cov, cov_stride, normalize: as
 * rfsgpu_batch_cycle_async.  z: [n_filters][RFSGPU_MAX_Z][3], n_z: [n_filters]; a filter with n_z == 0 is not updated (its predict
 * part runs, its weights are summed and divided as asked).  scan, n_scan: the laser scan that goes with the sets (2 ...
 * RFSGPU_VP_MAX_SCAN beams), or NULL: the scan the handle holds; a batch that has never been given one: RFSGPU_ERR_INVALID.
 * Stream-ordered, nothing is read back.  On a 2-D, FastSLAM or multi-hypothesis batch: RFSGPU_ERR_UNSUPPORTED.  A call in which
 * every n_z is 0 is its predict part and the sums, with no step launch (a driver's birth predict at the head of a run of messages).
 * rfsgpu_last_step_variant after it: {1, 0, particles per workgroup of the step kernel (2, or 1 where two do not fit in LDS; 0: no
 * step launch), 1 (0: no step launch)}. */
int rfsgpu_batch_vp_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride,
                                const double *z, const int *n_z, const double *scan, int n_scan, int normalize);
/* -- a batch of Victoria Park FastSLAM filters (single hypothesis): the switch that makes a batch created with
 * RFSGPU_MODEL_VICTORIAPARK_3D step FastSLAM filters instead of RB-PHD filters.  Off at creation, like
 * rfsgpu_batch_vp_serve_estimates and rfsgpu_batch_mh_serve_metrics: with the switch off every refusal above stands.
 * on != 0: the batch is a FastSLAM batch from here on.  rfsgpu_batch_set_fastslam_config serves it, per filter or -1, with
 * landmarkCandidateMeasurementCountThreshold free (the lists live one candidate per lane: at most 64 per particle, a fuller list
 * raises the candidate-list error as on a handle; a 2-D batch keeps refusing thresholds other than 1) and maxNDataAssocHypotheses
 * != 1 still refused, naming the filter.  Its cycle is rfsgpu_batch_vp_fastslam_cycle_async; rfsgpu_batch_vp_cycle_async refuses.
 * Each filter equals a separate Victoria Park handle stepped by rfsgpu_predict_map(f, 0) / rfsgpu_fastslam_update on the same
 * inputs, bit for bit.  The host-stop route (rfsgpu_batch_weight_sums, rfsgpu_batch_resample_apply, rfsgpu_batch_resample_occured)
 * and the device route (rfsgpu_batch_vp_set_motion, _vp_set_resampling, _vp_propagate_run_async, _vp_resample_async,
 * _vp_last_resample, _vp_loop_counts) and rfsgpu_static_steps_async serve it.  Both resampling routes move the landmark candidate
 * lists, the unused mask and the in-view count with the particle, as rfsgpu_resample_apply does on a FastSLAM handle; the two gates
 * of rfsgpu_batch_vp_resample_async are the FastSLAM configuration's minUpdatesBeforeResample / minMeasurementsBeforeResample, as on
 * a 2-D FastSLAM batch; no birth predict and no inheritance walk is launched.  Still refused on such a batch: [sensor], [truth],
 * [metric], [estimate] (rfsgpu_batch_vp_serve_estimates included), the 2-D device loop, rfsgpu_batch_fastslam_cycle_async and the
 * RB-PHD and multi-hypothesis batch calls.
 * RFSGPU_ERR_UNSUPPORTED with a message and the state untouched: not a batch of Victoria Park filters; on != 0 after
 * rfsgpu_batch_vp_cycle_async has run, or while rfsgpu_batch_vp_serve_estimates is on (a batch is of one kind); on == 0 after
 * rfsgpu_batch_vp_fastslam_cycle_async has run.  RFSGPU_ERR_INVALID: a null handle. */
int rfsgpu_batch_vp_serve_fastslam(rfsgpu_filter *f, int on);
/* FastSLAM::predict's map part + the single-hypothesis FastSLAM::update for every filter of such a batch at once.  Semantics are
 * those of rfsgpu_batch_fastslam_cycle_async: predict 0 / 1 runs the static step with each filter's own Q (also for a filter with
 * n_z == 0), RFSGPU_CYCLE_NO_PREDICT runs none; a filter with n_z == 0 is neither updated nor normalised; the prune runs only from
 * the filter's pruningMeasurementsThreshold.  z: [n_filters][RFSGPU_MAX_Z][3], n_z: [n_filters]; scan, n_scan: as
 * rfsgpu_batch_vp_cycle_async (NULL: the scan the batch holds).  A filter's clutter term is its own expectedClutterNumber / n_z, the
 * handle's expression.  Stream-ordered, nothing is read back: errors arrive through the shared error word, with the lowest filter
 * that exceeded gm_capacity named.  RFSGPU_ERR_INVALID: the argument errors of the other batch cycles.  RFSGPU_ERR_UNSUPPORTED with
 * the state untouched: any other kind of handle, a batch of Victoria Park filters whose switch is off included.
 * rfsgpu_last_step_variant after it: {2, 0, particles per workgroup of the associate kernel (2, or 1 where two do not fit in LDS),
 * 1}; rfsgpu_batch_last_cycle_lds: the bytes of LDS of a workgroup of that kernel. */
int rfsgpu_batch_vp_fastslam_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride,
                                         const double *z, const int *n_z, const double *scan, int n_scan, int normalize);
/* {sum w, sum w^2} of each filter's current weights: out [n_filters][2].  Synchronising. */
int rfsgpu_batch_weight_sums(rfsgpu_filter *f, double *out);
/* Resample the filters with resampled[b] != 0: slot k takes slot src_slot[k] (global slots; a source lies in k's own block and keeps
 * itself, else RFSGPU_ERR_INVALID); their weights become 1.  Other filters' entries of src_slot are not read. */
int rfsgpu_batch_resample_apply(rfsgpu_filter *f, const int *src_slot, const unsigned char *resampled);
/* resampleOccured_ of each filter: out [n_filters]. */
int rfsgpu_batch_resample_occured(const rfsgpu_filter *f, unsigned char *out);
/* -- the device loop: ParticleFilter::propagate and the resampling tail of RBPHDFilter::update for every filter of a batch, as
 * stream-ordered launches.  With them a batch run is propagate -> cycle(x = NULL) -> resample per step and the host waits for nothing.
 * Random numbers: Philox4x32-10 under the filter's 64-bit key (low word k0, high word k1) with counter
 * (slot within the filter, block, call low word, call high word): a filter's draws do not depend on its place in the batch.
 *
 * Process noise of filter `filter` (-1: every filter): additive N(0, diag(var)) on (x, y, theta) after MotionModel_Odometry2d::step;
 * seed is the filter's Philox key (propagation and resampling draws). */
int rfsgpu_batch_set_motion_odometry(rfsgpu_filter *f, int filter, const double var[3], unsigned long long seed);
/* The two thresholds of ParticleFilter::resample of filter `filter` (-1: every filter): it does NOT resample when
 * N_eff > eff_n && N_eff / n_per_filter > eff_n_percent.  The minimum-update / minimum-measurement gates are those of the filter's
 * rfsgpu_filter_config. */
int rfsgpu_batch_set_resampling(rfsgpu_filter *f, int filter, double eff_n, double eff_n_percent);
/* u [n_filters][3] the odometry inputs; pin [n_filters] (or NULL: none), pin_pose [n_filters][3] (may be NULL when nothing is pinned).
 * Particle i of filter b becomes step(pose, u[b]) + sqrt(var_b) * g with g three standard normal deviates by Box-Muller
 * (rad = sqrt(-2 ln u1), ang = 2 pi u2, u in (0, 1] from 53 bits of two words each): block 0 gives g_x = rad cos ang and
 * g_y = rad sin ang, block 1's rad cos ang gives g_theta.  Its pose covariance becomes diag(var_b) (the handle goes to one pose
 * covariance per particle).  Where pin[b] != 0 every particle of filter b takes pin_pose[b] with a zero covariance.  The inputs are
 * copied into a pinned ring before the call returns; nothing waits for the GPU.  rfsgpu_get_poses returns the new poses; the births
 * of the next rfsgpu_batch_cycle_async still happen at the poses from before the call (RBPHDFilter::predict), whether that cycle
 * passes x or NULL; rfsgpu_set_poses in between ends that: the births then happen at the poses it set, as without a propagation.  A filter without rfsgpu_batch_set_motion_odometry: RFSGPU_ERR_INVALID, naming it. */
int rfsgpu_batch_propagate_async(rfsgpu_filter *f, const double *u, const double *pin_pose, const unsigned char *pin, unsigned long long call);
/* The tail of RBPHDFilter::update with ParticleFilter::resample for every filter, after a cycle with normalize != 0: n_z [n_filters]
 * that cycle's measurement counts.  Every call counts as an update; a filter with n_z == 0 or under either gate stops there.
 * N_eff = 1 / sum w^2 (summed in slot order); a filter that does not pass the test above is resampled by the reference's systematic
 * plan with the draw u = (53 bits of block (0, 2, call)) / 2^53 in [0, 1): its mixtures, poses and pose covariances are gathered,
 * its weights become 1, its resampleOccured_ is set, its counters go to 0.  The weights must be non-negative (normalised).
 * Stream-ordered, nothing waits.  One workgroup resamples a filter: n_per_filter <= RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER, beyond
 * it RFSGPU_ERR_UNSUPPORTED.  A filter without rfsgpu_batch_set_resampling or _set_motion_odometry: RFSGPU_ERR_INVALID, naming it.
 * From the first call on, the particle ids, resampleOccured_ and the counters of this handle live on the device:
 * rfsgpu_get_particle_ids / _set_particle_ids and rfsgpu_batch_resample_occured read / write them there (synchronising), the next
 * predict's inheritance of the unused-measurement lists is computed there, and rfsgpu_batch_resample_apply (the host route) is
 * refused with RFSGPU_ERR_UNSUPPORTED: the two routes do not mix on one handle.  Host route first, device route later is allowed
 * (the host's ids and flags move to the device). */
#define RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER 2048
int rfsgpu_batch_resample_async(rfsgpu_filter *f, const int *n_z, unsigned long long call);
/* The last rfsgpu_batch_resample_async: fired [n_filters], src_slot [N] its plan in global slots (identity where not fired),
 * n_eff [n_filters] (0 where a filter stopped before the N_eff test); any may be NULL.  Synchronising. */
int rfsgpu_batch_last_resample(rfsgpu_filter *f, unsigned char *fired, int *src_slot, double *n_eff);
/* The pose covariance of every slot as the next update will read it: out [N][9], row-major (a handle with one shared covariance
 * returns it N times).  Synchronising; for tests and drivers that want to see what rfsgpu_batch_propagate_async left. */
int rfsgpu_batch_get_pose_covs(rfsgpu_filter *f, double *out);
/* Resamplings of each filter by rfsgpu_batch_resample_async so far: out [n_filters].  Synchronising. */
int rfsgpu_batch_resample_counts(rfsgpu_filter *f, long long *out);
/* -- the device route of a batch of Victoria Park filters: ParticleFilter::propagate with MotionModel_Ackerman2d::step for a run of
 * odometry messages, the resampling tail of RBPHDFilter::update, and the birth predict's inheritance walk from the ids the device
 * holds.  With them a run of messages is birth cycle -> rfsgpu_static_steps_async -> propagate_run -> update cycle (x = NULL) ->
 * resample, and the host waits for nothing.  Each filter equals the host-stop route of the same batch bit for bit, given the same
 * poses and draws.  On a 2-D batch, a shard or an ordinary handle every call of the section returns RFSGPU_ERR_UNSUPPORTED with the
 * state untouched.
 *
 * Filter `filter`'s (-1: every filter's) input noise N(0, diag(var)) on (speed, steering), the vehicle geometry {h, l, dx, dy}
 * (l != 0) and its 64-bit Philox key (propagation and resampling draws). */
int rfsgpu_batch_vp_set_motion(rfsgpu_filter *f, int filter, const double var[2], const double geom[4], unsigned long long seed);
/* The two thresholds of ParticleFilter::resample of filter `filter` (-1: every filter): the rule stated for
 * rfsgpu_batch_set_resampling; the gates are those of the filter's rfsgpu_filter_config. */
int rfsgpu_batch_vp_set_resampling(rfsgpu_filter *f, int filter, double eff_n, double eff_n_percent);
/* n consecutive odometry messages: u [n][2] = {speed, steering}, dt [n], noisy [n] (NULL: every step is noisy).  The inputs are the
 * dataset's, shared by all filters; every slot takes the steps one after the other in ONE launch.  Slot i of filter b draws what a
 * handle draws for particle i under rfsgpu_propagate_ackerman_run_async(seed = key_b, call0): counter (i within the filter, 0,
 * call low word, call high word) with call = call0 + step, Box-Muller as there (rad cos ang on the speed, rad sin ang on the
 * steering); no draw is made for a step with noisy[k] == 0 (a driver's stationary predicts) or with both variances 0.  The run is
 * copied into a block of the batch's pinned ring before the call returns: n <= RFSGPU_BATCH_VP_RUN_MAX, beyond it
 * RFSGPU_ERR_INVALID with the state untouched (split the run; the calls continue at call0 + n).  The propagation is IN PLACE and
 * stream-ordered: the caller issues it behind the birth predict of the run (rfsgpu_batch_vp_cycle_async with predict = 1), which must
 * still see the poses of the last update, and in front of the update cycle, which then passes x = NULL.  The pose covariances are
 * left as they are.  A filter without rfsgpu_batch_vp_set_motion: RFSGPU_ERR_INVALID, naming it. */
#define RFSGPU_BATCH_VP_RUN_MAX 16
int rfsgpu_batch_vp_propagate_run_async(rfsgpu_filter *f, int n, const double *u, const unsigned char *noisy, const double *dt, unsigned long long call0);
/* rfsgpu_batch_resample_async for such a batch, after an rfsgpu_batch_vp_cycle_async with normalize != 0: counters, both gates,
 * N_eff, the systematic plan with the draw of (key_b, call), ids, gather, weights 1, resampleOccured_, counters back to 0.
 * n_per_filter <= RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER, beyond it RFSGPU_ERR_UNSUPPORTED; a filter without
 * rfsgpu_batch_vp_set_resampling or _vp_set_motion: RFSGPU_ERR_INVALID, naming it.  From the first call on the handle is on the device
 * route: the particle ids, resampleOccured_ and the counters live on the device (rfsgpu_get_particle_ids / _set_particle_ids and
 * rfsgpu_batch_resample_occured read / write them there, synchronising), rfsgpu_batch_resample_apply is refused with
 * RFSGPU_ERR_UNSUPPORTED, and a birth predict computes its inheritance levels on the device: the staging pair and the level-0
 * births, RFSGPU_RBPHD_WALK_LEVELS (copy, birth) pairs that find nothing to do where the walk is shallower, and one workgroup per
 * filter for deeper chains.  A filter's resampleOccured_ falls in the cycle that updates it (n_z > 0).  Host-stop route first,
 * device route later is allowed (the host's ids and flags move to the device). */
int rfsgpu_batch_vp_resample_async(rfsgpu_filter *f, const int *n_z, unsigned long long call);
/* The last rfsgpu_batch_vp_resample_async, as rfsgpu_batch_last_resample reports it; any output may be NULL.  Synchronising. */
int rfsgpu_batch_vp_last_resample(rfsgpu_filter *f, unsigned char *fired, int *src_slot, double *n_eff);
/* resamplings [n_filters]: each filter's resamplings by rfsgpu_batch_vp_resample_async so far; max_level: the deepest inheritance
 * level any walk on the device has met.  Either may be NULL.  Synchronising. */
int rfsgpu_batch_vp_loop_counts(rfsgpu_filter *f, long long *resamplings, int *max_level);
/* -- a batch of FastSLAM filters: every filter is a 2-D single-hypothesis rfs::FastSLAM (include/FastSLAM.hpp) with its own
 * configuration, measurement set, weights, resampling and seed; each equals a separate handle driven through
 * rfsgpu_predict_map(add_birth = 0) / rfsgpu_fastslam_update given the same inputs.  A batch is of ONE kind: the first of
 * rfsgpu_batch_set_fastslam_config / rfsgpu_batch_fastslam_cycle_async (FastSLAM) or rfsgpu_batch_cycle_async (RB-PHD) decides, and
 * from then on the other kind's calls return RFSGPU_ERR_UNSUPPORTED with a message.  The model, Kalman filter and
 * landmark process noise of a filter come from rfsgpu_batch_configure as for an RB-PHD batch; propagation, resampling
 * (rfsgpu_batch_propagate_async, _resample_async, _last_resample, _resample_counts, _resample_apply), rfsgpu_batch_weight_sums and the
 * per-slot getters work unchanged.  The [metric] calls accept a FastSLAM batch (there a Gaussian's weight is a log-odds: see below).
 *
 * Filter `filter`'s (-1: every filter's) FastSLAM configuration.  RFSGPU_ERR_UNSUPPORTED, naming the filter, for
 * maxNDataAssocHypotheses != 1 (the multi-hypothesis update grows the particle set) and for
 * landmarkCandidateMeasurementCountThreshold != 1 (candidate lists would have to travel with a resampling).  On a FastSLAM batch the
 * two gates of rfsgpu_batch_resample_async are this configuration's minUpdatesBeforeResample / minMeasurementsBeforeResample. */
int rfsgpu_batch_set_fastslam_config(rfsgpu_filter *f, int filter, const rfsgpu_fastslam_config *cfg);
/* FastSLAM::predict's map part and FastSLAM::update of every filter, arguments as rfsgpu_batch_cycle_async.  predict 0 or 1: the
 * static landmark step (Sigma += Q_b, no births; it also runs for a filter with n_z == 0), RFSGPU_CYCLE_NO_PREDICT: none.  A filter
 * with n_z == 0 is not updated and not normalised this cycle (FastSLAM.hpp:402-403).  A filter prunes only when n_z >= its
 * pruningMeasurementsThreshold.  normalize != 0: each updated filter's weights are divided by their own sum (the summation order of
 * rfsgpu_batch_weight_sums).  Stream-ordered, nothing synchronises; errors reach the host as with rfsgpu_batch_cycle_async (the shared
 * device error word at the next synchronising call; rfsgpu_last_error names the lowest filter that ran out of gm_capacity). */
int rfsgpu_batch_fastslam_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride,
                                      const double *z, const int *n_z, int normalize);
/* -- a batch of multi-hypothesis FastSLAM filters: every filter is a 2-D rfs::FastSLAM with maxNDataAssocHypotheses in [1, 16]
 * (include/FastSLAM.hpp:492-556), whose update multiplies its particles and whose resampleWithMapCopy (:729-757) brings them back.
 * Filter b owns the global slots [b * max_per_filter, (b + 1) * max_per_filter); its live particles are the first n_b of them, and
 * n_b -- n_per_filter at creation, which is also the count a resampling brings the filter back to (nParticles_init_) -- lives in a
 * word on the device.  SLOTS AT OR BEYOND A FILTER'S COUNT HOLD NOTHING MEANINGFUL: the per-slot getters and setters work on global
 * slots as on any batch (rfsgpu_n_particles stays n_filters * max_per_filter, so they wait for no count), and what they return for
 * such a slot is whatever an earlier, larger set left there; rfsgpu_batch_live_counts says where each filter ends.  Particle ids
 * start as the slot within the filter.  max_per_filter < n_per_filter: RFSGPU_ERR_INVALID; max_per_filter >
 * RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES: RFSGPU_ERR_UNSUPPORTED (one workgroup resamples a filter in LDS); the 2-D model only.
 * rfsgpu_create_batch and the handles it makes are unchanged and still refuse more than one hypothesis.
 *
 * On such a handle rfsgpu_batch_set_fastslam_config accepts maxNDataAssocHypotheses 1 ... 16 per filter (filters of one batch may
 * differ, 1 included; nParticlesMax defaults to 3 * n_per_filter, FastSLAM.hpp:250); landmarkCandidateMeasurementCountThreshold != 1
 * stays refused.  The N_eff thresholds are rfsgpu_batch_set_resampling's; unset: n_per_filter / 4 and 0.25 (ParticleFilter.hpp:232).
 * rfsgpu_batch_propagate_async is allowed and moves every slot of every block (its draws are keyed by the slot within the filter, so
 * a live slot's draw does not depend on the counts).  Refused with RFSGPU_ERR_UNSUPPORTED, state untouched, because each assumes
 * that every filter fills its block: rfsgpu_batch_cycle_async, rfsgpu_batch_fastslam_cycle_async, rfsgpu_batch_resample_async /
 * _resample_apply / _last_resample / _resample_counts, rfsgpu_batch_weight_sums and -- until rfsgpu_batch_mh_serve_metrics below
 * switches their live-count form on -- the [metric] calls. */
int rfsgpu_create_batch_mh(rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int max_per_filter, int device_id,
                           int gm_capacity);
/* One whole FastSLAM::update (FastSLAM.hpp:387-421) of every filter, enqueued as one launch chain: per filter what
 * rfsgpu_fastslam_cycle_async does on a handle created with max_particles = max_per_filter -- with predict != 0 the static landmark
 * step (:376-383; it also runs for a filter with n_z == 0); the association with Murty's k best; the copy plan in the reference's
 * order (:543-556); copies, weight split, Kalman correction / existence / weights; prune (when n_z >= the filter's
 * pruningMeasurementsThreshold, :611-612) and new landmarks; normalisation; resampleWithMapCopy (:729-757) with its two gates, the
 * N_eff test, the forced resampling above nParticlesMax, the shrink to n_per_filter, ids and weights; and the second normalisation
 * when resample() ran its test and returned false (:743).  x [N][3], x_cov, cov_stride: as rfsgpu_batch_cycle_async (every global
 * slot; NULL: the poses on the device stay).  z [n_filters][RFSGPU_MAX_Z][2], n_z [n_filters]; a filter with n_z == 0 only counts the
 * update (:399-402).  u01 [n_filters]: the caller's draws in [0, 1) for the systematic plans; a value outside is RFSGPU_ERR_INVALID
 * and names the filter.  The tables travel through the batch's pinned ring; nothing in the call waits for the GPU, cycles queue back
 * to back.
 *
 * Overflow is per filter: a filter whose grown set would exceed max_per_filter is left as it was before the cycle's update (a static
 * step asked for by `predict` has run) while the other filters' cycles complete; further cycles enqueued behind it are abandoned for
 * that filter only.  The next synchronising call returns RFSGPU_ERR_CAPACITY once, names the lowest such filter and clears the
 * condition. */
int rfsgpu_batch_fastslam_mh_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride,
                                         const double *z, const int *n_z, const double *u01);
/* What the last rfsgpu_batch_fastslam_mh_cycle_async did (synchronises; any pointer may be NULL).  [n_filters]: the count after the
 * update, the count after the resampling, whether that fired, N_eff (0 where the test did not run), whether the filter overflowed.
 * parent and plan: [n_filters * max_per_filter], as rfsgpu_fastslam_last_cycle's but in slots local to the filter; identity where
 * nothing happened (no measurements, overflow), -1 at and beyond the respective count. */
int rfsgpu_batch_fastslam_last_cycle(rfsgpu_filter *f, int *n_after_update, int *n_after_resample, unsigned char *fired,
                                     double *n_eff, unsigned char *overflowed, int *parent, int *plan);
/* The live particle count of every filter: out [n_filters].  Synchronising. */
int rfsgpu_batch_live_counts(rfsgpu_filter *f, int *out);
/* on != 0: from this call on the [metric] calls serve this multi-hypothesis batch (see below); on == 0: they refuse again.
 * Not a handle of rfsgpu_create_batch_mh: RFSGPU_ERR_UNSUPPORTED with a message.  Synchronising; the filters' state is untouched.
 * The switch is off at creation: the refusal of the [metric] calls is what such a handle was published with.
 *
 * With the switch on, rfsgpu_set_ground_truth, rfsgpu_error_log_create / _reset / _read, rfsgpu_step_error_async, rfsgpu_step_error
 * and rfsgpu_get_map_estimate work on the handle with the signatures, records, log semantics and error codes of the [metric] section.
 * A record of filter b then means:
 *   - its particle set is the global slots [b * max_per_filter, b * max_per_filter + n_b), n_b being the filter's live count AS THE
 *     DEVICE HOLDS IT AT THE KERNEL'S POINT OF THE STREAM (n_per_filter before the first cycle), not a host copy: so
 *     rfsgpu_batch_propagate_async -> rfsgpu_batch_fastslam_mh_cycle_async -> rfsgpu_step_error_async queue back to back, and
 *     rfsgpu_step_error_async waits for nothing (cycles in flight stay in flight);
 *   - slots at or beyond n_b are never read -- weight, pose, count or mixture: after a shrink they hold what a larger set left;
 *   - best_slot is global: the first live slot holding the maximum weight, slot 0 of the block when no live weight is > 0;
 *   - weight_sum and the four pose means go over the live slots in the kernel's fixed tree (lane l adds the slots l, l + 64, ... < n_b
 *     in ascending order, then the wave's butterfly): the bits of a full block of n_b particles holding the same values;
 *   - a Gaussian's weight is a log-odds w, as on a FastSLAM batch: every "weight" of the record and of rfsgpu_get_map_estimate is
 *     1 - 1 / (1 + exp(w));
 *   - a filter that overflowed in the last cycle was left as before that cycle's update and is evaluated on that state with status 0;
 *     the pending RFSGPU_ERR_CAPACITY is reported by the next synchronising call as always (once, naming the lowest filter), and
 *     rfsgpu_step_error_async itself still enqueues.  A filter with n_z == 0 in the last cycle, or one that was just resampled (all
 *     weights 1: slot 0 of the block is the best), is evaluated like any other.
 * Everything else that is refused on such a batch stays refused (rfsgpu_batch_weight_sums, the resampling calls). */
int rfsgpu_batch_mh_serve_metrics(rfsgpu_filter *f, int on);
/* -- a batch of Victoria Park multi-hypothesis FastSLAM filters (outside the STABLE CORE): n_filters independent rfs::FastSLAM filters
 * on the Victoria Park models, each with maxNDataAssocHypotheses in [2, 16].  The layout is rfsgpu_create_batch_mh's: filter b owns the
 * global slots [b * max_per_filter, (b + 1) * max_per_filter), its first n_b are live, n_b is a word on the device.  Filter b equals a
 * Victoria Park handle made by rfsgpu_create_ex(max_particles = max_per_filter) and stepped by rfsgpu_static_steps_async /
 * rfsgpu_propagate_ackerman_run_async / rfsgpu_fastslam_cycle_full_async(predict = 0, n_init = n_per_filter) on the same poses, sets,
 * scan and draws: mixtures, counts, candidate lists, unused masks, in-view counts, poses, ids, parents, plans, live counts and the
 * fired / forced decisions bit for bit; weights and N_eff to rounding (the batch sums in its own tree).  The argument errors are those
 * of rfsgpu_create_batch_mh (which keeps refusing the Victoria Park model); nParticlesMax defaults to 3 * n_per_filter.
 *
 * Configuration: rfsgpu_batch_configure_vp, rfsgpu_set_model_victoriapark, rfsgpu_set_lmk_process_noise and rfsgpu_set_laser_scan as on
 * a batch of Victoria Park filters (one scan for the handle; each filter's clutter term comes from its own expectedClutterNumber);
 * rfsgpu_batch_set_fastslam_config with maxNDataAssocHypotheses 2 ... 16 and ANY landmarkCandidateMeasurementCountThreshold -- one
 * hypothesis is refused, naming the filter: single-hypothesis filters belong to rfsgpu_batch_vp_serve_fastslam (a handle associates one
 * hypothesis by the sparse single-hypothesis kernel, whose bits Murty's search with a limit of one does not reproduce);
 * rfsgpu_batch_set_resampling for the N_eff thresholds (unset: n_per_filter / 4 and 0.25).
 *
 * Also served: rfsgpu_batch_fastslam_last_cycle and rfsgpu_batch_live_counts; rfsgpu_batch_vp_set_motion and
 * rfsgpu_batch_vp_propagate_run_async (every slot of every block moves; a slot's draw is keyed by its index within the filter, so a live
 * slot draws what its handle's particle draws); rfsgpu_static_steps_async (the live slots).  The last two enqueue behind pending cycles
 * without waiting, and skip a filter whose overflow word is up, as a handle abandons them behind an abandoned cycle.
 *
 * Refused with RFSGPU_ERR_UNSUPPORTED and a message, state untouched: rfsgpu_batch_cycle_async, rfsgpu_batch_vp_cycle_async,
 * rfsgpu_batch_fastslam_cycle_async, rfsgpu_batch_vp_fastslam_cycle_async, rfsgpu_batch_fastslam_mh_cycle_async;
 * rfsgpu_batch_vp_resample_async / _vp_last_resample / _vp_set_resampling / _vp_loop_counts, rfsgpu_batch_resample_async /
 * _resample_apply / _last_resample / _resample_counts, rfsgpu_batch_weight_sums; the [sensor], [truth], [metric] and [estimate] calls;
 * rfsgpu_batch_vp_serve_fastslam, rfsgpu_batch_vp_serve_estimates and rfsgpu_batch_mh_serve_metrics; rfsgpu_batch_set_motion_odometry,
 * rfsgpu_batch_propagate_async (the 2-D device loop). */
int rfsgpu_create_batch_vp_mh(rfsgpu_filter **out, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity);
/* One whole FastSLAM::update of every filter of such a batch as one launch chain; nothing is read back.  Counts, per-filter overflow,
 * the u01 range check (naming the filter) and x == NULL are rfsgpu_batch_fastslam_mh_cycle_async's; z is [n_filters][RFSGPU_MAX_Z][3];
 * scan / n_scan follow rfsgpu_batch_vp_cycle_async (NULL: the scan the batch holds; none held: RFSGPU_ERR_INVALID).  A particle's
 * copies take its landmark candidate lists exactly when THAT FILTER's previous cycle resampled (FastSLAM.hpp:551-553); the resampling
 * gather moves the lists, the unused mask and the in-view count with the particle.  A 65th candidate, a map beyond gm_capacity or a
 * Murty table beyond 64 reaches the host through the shared error word at the next synchronising call; rfsgpu_last_error names the
 * lowest filter for gm_capacity and for the candidate list.  Any other kind of handle: RFSGPU_ERR_UNSUPPORTED, state untouched. */
int rfsgpu_batch_vp_fastslam_mh_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride,
                                            const double *z, const int *n_z, const double *scan, int n_scan, const double *u01);
#ifdef RFSGPU_ENABLE_BENCH_API
/* [test] 1 once a step of this handle (batch or not) has queued Murty-200 partitions, else 0.  Synchronising. */
int rfsgpu_murty_seen(rfsgpu_filter *f);
#endif

/* ---- [metric] per-step map error and pose error on the device (outside the STABLE CORE) ------------------------------------------
 * What the reference's analysis2dSim computes per time step from a run's log files (src/analysis2dSim.cpp:150-249), as one launch on
 * the handle's stream for an ordinary 2-D handle (one filter) or for every filter of a batch: the weighted-mean pose error of the
 * particle set (:265-317, getAverageError) and the OSPA / COLA error (include/OSPA.hpp:122-203, include/COLA.hpp:91-98) between the map estimate of
 * the highest-weight particle and the ground-truth landmarks that have been in sensor range so far.  The kernel (csrc/map_metric.h)
 * reads the filter state as it is at that point of the stream and writes one record per filter; nothing else changes.
 * 2-D landmarks only: Victoria Park handles, ordinary handles on which rfsgpu_fastslam_update has run and the shard handles of an
 * rfsgpu_group return RFSGPU_ERR_UNSUPPORTED (with a rfsgpu_last_error message) from every call of this section.
 * A batch of FastSLAM filters (rfsgpu_batch_fastslam_cycle_async) is served: a Gaussian's weight is a log-odds w there, and wherever
 * this section says "weight" of a Gaussian (n_est, cardinality, rfsgpu_get_map_estimate's w) it means 1 - 1 / (1 + exp(w)), the
 * number the reference's fastslam2dSim logs (src/fastslam2dSim.cpp:628) and analysis2dSim thresholds.  Lifting the refusal for an
 * ordinary FastSLAM handle is a later change ([estimate] alone serves one once rfsgpu_handle_serve_estimates is on).
 * A batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh) returns RFSGPU_ERR_UNSUPPORTED from every call of this section
 * until rfsgpu_batch_mh_serve_metrics(f, 1); from then on it is served as a FastSLAM batch is (log-odds weights), with "the filter's
 * block" read as its LIVE slots -- the first n_b of its max_per_filter, n_b taken from the device where the kernel runs: see
 * rfsgpu_batch_mh_serve_metrics for what a record means there. */
#define RFSGPU_MAX_METRIC_SET 512   /* hard limit of either set of one comparison (estimates, observable ground truth) */
/* One record per filter and call; every field is 8 bytes wide.  status: 0 = ok; 1 = n_est or n_truth exceeds
 * RFSGPU_MAX_METRIC_SET; 2 = no finite cost met (non-finite coordinates).  With status != 0 ospa, cola, e_dist, e_card are NaN
 * and the other fields stand.  (A struct tag, not a typedef: the synchronous call below bears the same name.) */
struct rfsgpu_step_error {
  double t;              /* the time given with the call                                                                   */
  long long status;
  long long best_slot;   /* global slot of the highest-weight particle: the first slot of the filter's block whose weight is
                            strictly greater than every earlier one, starting from 0 (analysis2dSim.cpp:159-167); slot 0 of the
                            block when no weight is > 0                                                                    */
  long long n_est;       /* its Gaussians with weight >= w_threshold (:187)                                                */
  long long n_truth;     /* ground-truth landmarks with first_seen <= t (:213-220)                                         */
  double cardinality;    /* the sum of ALL its Gaussians' weights (:194)                                                   */
  double ospa;           /* (sum C^p / n)^(1/p) over an assignment that minimises sum C, n = max(n_est, n_truth); 0 for n = 0
                            (OSPA.hpp:179-199)                                                                             */
  double cola;           /* ospa * n^(1/p) / c (COLA.hpp:91-98)                                                            */
  double e_dist;         /* sum of the assignment's cells != c (OSPA.hpp:191-192)                                          */
  double e_card;         /* sum of the assignment's cells == c (:189-190)                                                  */
  double pose_ex, pose_ey, pose_eth, pose_ed;   /* weighted means (weights w / sum w) of x - rx, y - ry, theta - rtheta with one
                            +-2 pi correction, hypot(x - rx, y - ry) (analysis2dSim.cpp:265-317); NaN without a gt_pose     */
  double weight_sum;     /* sum of the block's particle weights (:163)                                                     */
};
/* Ground-truth landmarks of filter `filter` (0 on an ordinary handle): xy [n][2], first_seen [n] = the time each landmark first came
 * into sensor range (third column of the reference's gtLandmark.dat, src/rbphdslam2dSim.cpp:249-284; -1 = never, which counts from
 * the start as in analysis2dSim.cpp:216) or NULL = all -1.  n <= RFSGPU_MAX_METRIC_SET, else RFSGPU_ERR_INVALID.  Uploaded once
 * (synchronising); a filter without ground truth is compared with the empty set. */
int rfsgpu_set_ground_truth(rfsgpu_filter *f, int filter, const double *xy, const double *first_seen, int n);
/* The device-side log: log_capacity rows of n_filters records.  _create (re)allocates it empty (0 frees it), _reset empties it;
 * rows stay where they are until then. */
int rfsgpu_error_log_create(rfsgpu_filter *f, int log_capacity);
int rfsgpu_error_log_reset(rfsgpu_filter *f);
/* Appends one row: t [n_filters] the time of each filter's step, gt_pose [n_filters][3] its ground-truth pose (x, y, theta) or
 * NULL (pose fields NaN); w_threshold, cutoff c > 0 and order p >= 1 as analysis2dSim.cpp:182, :232-233 (0.75, 0.20, 1.0).
 * Stream-ordered on the handle's stream: t and gt_pose are copied into the pinned staging ring before the call returns, the kernel
 * reads them there, nothing waits for the GPU.  A full log (or none): RFSGPU_ERR_CAPACITY, nothing is enqueued. */
int rfsgpu_step_error_async(rfsgpu_filter *f, const double *t, const double *gt_pose, double w_threshold, double cutoff, double order);
/* Synchronises the stream and copies the rows written so far ([row][filter], at most max_rows of them) to out; *n_rows = the
 * number of rows in the log.  The log keeps them. */
int rfsgpu_error_log_read(rfsgpu_filter *f, struct rfsgpu_step_error *out, int max_rows, int *n_rows);
/* The synchronous form: the same kernel, its row delivered to out [n_filters]; needs no log and leaves the log alone. */
int rfsgpu_step_error(rfsgpu_filter *f, const double *t, const double *gt_pose, double w_threshold, double cutoff, double order,
                      struct rfsgpu_step_error *out);
/* The map estimate of filter `filter`'s highest-weight particle for the host -- the selection of best_slot and n_est above, what the
 * reference's landmarkEst.dat holds of that particle: up to max_n Gaussians with weight >= w_threshold in mixture order (mean [n][2],
 * cov [n][4] row-major, w [n]; any may be NULL), *n = their number.  Synchronising. */
int rfsgpu_get_map_estimate(rfsgpu_filter *f, int filter, double w_threshold, int max_n, int *n, double *mean, double *cov, double *w);

/* ---- [resample] ParticleFilter::resample on the device, for an ordinary handle of any size (outside the STABLE CORE) --------------
 * The host route of a resampling -- rfsgpu_weight_sums, rfsgpu_normalize_weights, rfsgpu_get_weights, the N_eff test and the plan
 * on the host, rfsgpu_resample_apply[_n] -- stops the host three times per update.  rfsgpu_resample_async enqueues the whole of
 * ParticleFilter::resample(n, forceResample) (include/ParticleFilter.hpp:399-492) on the handle's stream and waits for nothing:
 *   1. normalizeWeights (:402): the reduction and the division of rfsgpu_weight_sums + rfsgpu_normalize_weights, bit for bit;
 *   2. unless force != 0, N_eff = 1 / sum w^2 added in slot order (:405-411); nothing more happens when
 *      N_eff > eff_n && N_eff / n_particles > eff_n_percent (:412-414);
 *   3. else the systematic plan of n_out samples (:417-444; n_out == 0 or >= n_particles: the count stays) from the caller's draw
 *      u01 in [0, 1) (the reference's one drand48(), :421), the copies of cases 1-4 (:446-479) with the ids and parent ids
 *      (:466, :475), the new count (:482-483) and weights of 1 (:486-488).  What a copy carries follows the birth inheritance mode
 *      as in rfsgpu_resample_apply; on a handle on which rfsgpu_fastslam_update has run the landmark candidates travel too;
 *   4. where the test ran and did not fire and renormalize != 0, the weights are summed and divided once more: the else branch of
 *      RBPHDFilter::update (include/RBPHDFilter.hpp:536-538; FastSLAM.hpp:743).
 * The gates on updates and measurements since the last resampling (RBPHDFilter.hpp:528-529) and their counters stay with the
 * caller.  Any particle count up to rfsgpu_max_particles, both models, all three inheritance modes.  RFSGPU_ERR_UNSUPPORTED, with
 * the state untouched: a filter batch, a shard of an rfsgpu_group, a handle on which rfsgpu_fastslam_cycle_async has run.
 * RFSGPU_ERR_INVALID: u01 outside [0, 1), n_out < 0.
 * A negative or non-finite weight, or a sum that is not positive: the device normalises, moves and resets nothing, and the next
 * call that resolves (below) returns RFSGPU_ERR_INVALID once, with a message.  (The sums buffer of the handle,
 * rfsgpu_weight_sums_device_ptr, then holds the sums of the weights as they were given: the first reduction has run.)
 * What rfsgpu_resample_apply_n books on the host -- the ids, resampleOccured_ (:530), the acknowledgement of
 * RFSGPU_INHERIT_EXTERNAL, the new particle count -- is taken over from the device by the next call that needs it ("resolves":
 * one small copy and a wait), so an rfsgpu_predict_map after it walks the inheritance levels (RBPHDFilter.hpp:1005-1011) from the
 * right ids.  Resolving also reads the device's error word, as rfsgpu_synchronize does: an error of an asynchronous call
 * enqueued before the resampling (RFSGPU_ERR_CAPACITY, ...) is returned by the resolving call, and the resampling's own
 * bookkeeping is still taken over.  While a call that keeps the count is pending, rfsgpu_static_steps_async, rfsgpu_propagate_ackerman_async /
 * _run_async, rfsgpu_set_step_inputs_async, rfsgpu_predict_map_async(f, 0) and the configuration setters enqueue behind it
 * without resolving; every other call, and every call while one with n_out < n_particles is pending, resolves first.
 * RFSGPU_ERR_UNSUPPORTED as well on a handle on which rfsgpu_rbphd_cycle_async has run ([rbphd-cycle]: the ids and the gate's
 * counters are the device's there). */
int rfsgpu_resample_async(rfsgpu_filter *f, double eff_n, double eff_n_percent, double u01, int n_out, int force, int renormalize);
/* The last rfsgpu_resample_async (resolves): *fired whether it resampled (the return value of :400), *n_eff its N_eff (0 when
 * forced, :405), *n_after the particle count behind it (:482), plan[k] for those slots: the slot whose particle slot k now holds
 * a copy of (:474), k itself where the particle stayed (case 1, :465) or nothing fired.  Any pointer may be NULL; max_n >= the
 * count when plan is given. */
int rfsgpu_last_resample(rfsgpu_filter *f, int *fired, double *n_eff, int *n_after, int *plan, int max_n);

/* ---- [rbphd-cycle] the whole RBPHDFilter::update on the device (outside the STABLE CORE) ----------------------------------------------
 * rfsgpu_resample_async leaves the two gates of RBPHDFilter::update (include/RBPHDFilter.hpp:528-529) and their counters with the
 * caller, who must therefore read `fired` back after every update.  rfsgpu_rbphd_cycle_async enqueues one whole update (:444-541)
 * on the handle's stream and waits for nothing:
 *   1. nUpdatesSinceResample_ is counted on the device (:448); with n_z == 0 the call ends there (:451-452);
 *   2. nMeasurementsSinceResample_ is counted (:453); the scan (Victoria Park model; NULL leaves it) goes through the pinned ring of
 *      rfsgpu_set_step_inputs_async, its clutter density computed as rfsgpu_set_laser_scan computes it;
 *   3. the step: the launches of rfsgpu_cycle_async(f, RFSGPU_CYCLE_NO_PREDICT, NULL, NULL, 0, NULL, z, n_z, 0), z [n_z][2] or [n_z][3];
 *   4. resampleOccured_ is cleared (:526) and the gate tested on the device against minUpdatesBeforeResample and
 *      minMeasurementsBeforeResample of the handle's rfsgpu_filter_config.  Closed: the weights are normalised once (:537).  Open:
 *      ParticleFilter::resample as rfsgpu_resample_async(f, eff_n, eff_n_percent, u01, 0, 0, 1) does it, with the thresholds of
 *      rfsgpu_rbphd_set_resampling (never set: n_particles / 4 and 1 / 4); where it fires the device zeroes both counters and sets
 *      resampleOccured_ (:530-535).  The plan, gather and second-normalisation launches are enqueued either way and leave on
 *      device-side guards behind a closed gate.
 * The poses are the device's and follow the copies.  The particle count never changes on this route.  Cycles may follow one
 * another without a resolving call between them.  A weight set that cannot be resampled behaves as under rfsgpu_resample_async:
 * that cycle's tail touches nothing and the next resolving call returns RFSGPU_ERR_INVALID once.
 * While cycles are pending, rfsgpu_static_steps_async, rfsgpu_propagate_ackerman_async / _run_async,
 * rfsgpu_set_step_inputs_async(x == NULL), rfsgpu_set_lmk_process_noise, rfsgpu_set_filter_config, rfsgpu_rbphd_set_resampling and
 * rfsgpu_predict_map_async enqueue behind them without resolving (rfsgpu_set_kf_config and the model setters resolve).  A call that
 * returns an error has counted no update and leaves the host route open; a scan it carried may have been installed.  With
 * n_z == 0 a scan that comes with the call is installed too.  rfsgpu_predict_map_async(f, 1) then makes the inheritance walk of
 * RBPHDFilter.hpp:1005-1011 on the device, from the ids and the resampleOccured_ the device holds: a levels kernel, the staging
 * pair and the level-0 births, RFSGPU_RBPHD_WALK_LEVELS (copy, birth) pairs that find nothing to do where the walk is shallower,
 * and a one-workgroup kernel that finishes any deeper levels -- the same bits as rfsgpu_predict_map after a resolve, at any depth.
 * Every other call resolves first (one small copy and a wait) and takes over the ids, resampleOccured_ and the device's error
 * word, as for rfsgpu_resample_async.  Once a cycle has run on a handle, rfsgpu_resample_apply[_n] and rfsgpu_resample_async
 * return RFSGPU_ERR_UNSUPPORTED on it (the counters are the device's); the host route first and cycles later is allowed.
 * Both models, every birthGaussianMeasurementCountThreshold, RFSGPU_INHERIT_REFERENCE and _EAGER, any particle count up to
 * rfsgpu_max_particles.  RFSGPU_ERR_UNSUPPORTED with the state untouched: a filter batch, a shard of an rfsgpu_group,
 * RFSGPU_INHERIT_EXTERNAL, a handle on which FastSLAM updates have run.  RFSGPU_ERR_INVALID: a NULL handle, u01 outside [0, 1),
 * n_z beyond RFSGPU_MAX_Z, a Victoria Park handle that has never been given a scan. */
#define RFSGPU_RBPHD_WALK_LEVELS 4   /* inheritance levels >= 1 with launches of their own; deeper ones are the tail kernel's */
int rfsgpu_rbphd_set_resampling(rfsgpu_filter *f, double eff_n, double eff_n_percent);
int rfsgpu_rbphd_cycle_async(rfsgpu_filter *f, const double *z, int n_z, const double *scan, int n_scan, double u01);
/* Resolving.  Cycles enqueued so far, those that found the gate open, those that resampled, and the deepest inheritance level any
 * walk on the device has met.  Any pointer may be NULL. */
int rfsgpu_rbphd_cycle_counts(rfsgpu_filter *f, int *n_cycles, int *n_gate_open, int *n_resamplings, int *max_level);
/* Resolving.  The last cycle: whether its gate was open, whether it resampled, its N_eff (0 where the test did not run), plan[k]
 * as rfsgpu_last_resample reports it (identity where nothing fired; max_n >= n_particles when plan is given); *walk_levels the
 * deepest level of the last walk made on the device.  Any pointer may be NULL. */
int rfsgpu_rbphd_last_cycle(rfsgpu_filter *f, int *gate_open, int *fired, double *n_eff, int *plan, int max_n, int *walk_levels);
#ifdef RFSGPU_ENABLE_BENCH_API   /* [test]: 1 while cycles are pending (the ids and resampleOccured_ are the device's); reads nothing, waits for nothing */
int rfsgpu_rbphd_cycle_pending(rfsgpu_filter *f);
#endif /* RFSGPU_ENABLE_BENCH_API */

/* ---- [sensor] every filter's scan drawn on the device, for batches of RB-PHD filters (outside the STABLE CORE) --------------------
 * generateMeasurements of the reference's 2-D simulator (src/rbphdslam2dSim.cpp:283-366) for one time step and every filter of a
 * batch (rfsgpu_create_batch handles stepped by rfsgpu_batch_cycle_async) in one launch: per step the host hands over one ground-truth
 * pose per filter, the device draws each filter's scan into the batch's measurement table and writes the cycle's per-filter record,
 * and the cycle and the resampling tail read both there.  A batch run is then
 *   rfsgpu_batch_propagate_async -> rfsgpu_batch_sense_async -> rfsgpu_batch_cycle_sensed_async -> rfsgpu_batch_resample_sensed_async
 * per step and the host builds no measurement table.
 * Random numbers: Philox4x32-10 under the SENSOR's 64-bit key (low word k0, high word k1) with counter
 * (index, block | attempt << 8, call low word, call high word):
 *   block 3, index = landmark m:  g = (rad cos ang, rad sin ang) with rad = sqrt(-2 ln u1), ang = 2 pi u2, u in (0, 1] from 53 bits
 *                                 of two words each (the Box-Muller form of rfsgpu_batch_propagate_async);
 *   block 4, index = landmark m:  the detection draw, v = (53 bits of words 0, 1) / 2^53 in [0, 1), as every draw below;
 *   block 5, index = 0:           the clutter-count draw;
 *   block 6, index = clutter j:   attempt a = 0, 1, ... (in bits 8 and up of the block word) of point j's range draw;
 *   block 7, index = clutter j:   point j's bearing draw.
 * Propagation uses blocks 0 and 1 and the resampling draw block 2, so one key may serve a filter's motion and its sensor; every draw is
 * a pure function of (key, call, block, index, attempt): a filter's scan depends neither on its place in the batch nor on the others.
 * The scan of one filter, in this order:
 *   detections (:321-342, MeasurementModel::sample / MeasurementModel_RngBrg::measure): a landmark whose TRUE range lies in
 *     [rangeLimMin, rangeLimMax] gets z = (range, bearing wrapped to [-pi, pi]) + L g, L the lower Cholesky factor of R (the bearing is
 *     not wrapped again); it is kept when the NOISY range lies in the limits and v <= probabilityOfDetection.  Kept detections stand
 *     in landmark order;
 *   clutter (:344-362): the count is the first n with v <= CMF[n] of the 100-entry Poisson table of mean
 *     uniformClutterIntensity * 2 pi (rangeLimMax - rangeLimMin), computed on the host by the loop of :294-306 -- and 99 where no
 *     n < 99 does (the reference walks off its table there).  Point j has r = v rangeLimMax, drawn again (next attempt) while
 *     r < rangeLimMin -- after 64 attempts the last draw is mapped into the limits, r = rangeLimMin + v (rangeLimMax - rangeLimMin)
 *     (probability (rangeLimMin / rangeLimMax)^64) -- and b = v 2 pi - pi.
 * A set beyond max_nz is cut to its first max_nz entries (detections before clutter) and reported through the device error word: the
 * next synchronising call returns RFSGPU_ERR_CAPACITY once, and rfsgpu_last_error names the lowest such filter and its scan.
 * Every call of the section returns RFSGPU_ERR_UNSUPPORTED, with a message and the state untouched, on an ordinary handle, a shard of
 * an rfsgpu_group and -- until rfsgpu_batch_fastslam_serve_sensor below switches the section on for it -- a batch of FastSLAM
 * filters and a batch of multi-hypothesis FastSLAM filters: their per-filter records carry three count-dependent fields, which only
 * the sensed cycle of their own kind derives on the device.
 *
 * Filter `filter`'s (-1: every filter's) simulated sensor: model = ITS R, probabilityOfDetection, uniformClutterIntensity and range
 * limits (rangeLimBuffer is not read; the filter's own model, rfsgpu_batch_configure, usually has an inflated R), landmarks_xy
 * [n_landmarks][2] with 0 <= n_landmarks <= RFSGPU_SENSOR_MAX_LANDMARKS, 1 <= max_nz <= RFSGPU_MAX_Z, seed the sensor's Philox key.
 * RFSGPU_ERR_INVALID with a message: R not symmetric positive definite, rangeLimMin >= rangeLimMax, probabilityOfDetection outside
 * [0, 1], a negative clutter intensity, a clutter mean whose table is not finite, a landmark that is not finite.  Synchronising. */
#define RFSGPU_SENSOR_MAX_LANDMARKS 512
int rfsgpu_batch_set_sensor(rfsgpu_filter *f, int filter, const rfsgpu_rngbrg_config *model, const double *landmarks_xy, int n_landmarks,
                            int max_nz, unsigned long long seed);
/* Draw every filter's scan of call `call` at gt_pose [n_filters][3] (finite, |heading| <= 64 rad) and write this cycle's records:
 * the count, the set's place, the count of the filter's last non-empty update (its births) and the evaluation-point cap and weighting
 * switch of its configuration.  One kernel, one wavefront per filter; the poses travel through the batch's pinned ring and nothing
 * waits for the GPU.  A filter without rfsgpu_batch_set_sensor: RFSGPU_ERR_INVALID, naming it. */
int rfsgpu_batch_sense_async(rfsgpu_filter *f, const double *gt_pose, unsigned long long call);
/* rfsgpu_batch_cycle_async on the sets and records the last rfsgpu_batch_sense_async left (predict, x, x_cov, cov_stride, normalize as
 * there).  The launch is sized for what that sense call could write: the filters' largest max_nz and evaluation-point cap AT THE SENSE
 * CALL; results do not depend on the max_nz bound.  The records carry each filter's evaluation-point cap and weighting switch as the
 * sense call found them, and the step kernel lays out its LDS by them: a rfsgpu_batch_configure between the sense call and the cycle
 * that changes either (importanceWeightingEvalPointCount, useClusterProcess) makes the cycle return RFSGPU_ERR_INVALID, naming the
 * filter, until the next rfsgpu_batch_sense_async; any other field may change and holds from this cycle on, as with the host-fed
 * cycle.  A rfsgpu_batch_set_sensor between the two, for any filter, ends the sense call's validity in the same way.  The call puts the handle on the
 * device route, as the first rfsgpu_batch_resample_async does (ids, resampleOccured_ and the inheritance of the unused-measurement
 * lists on the device), and from the first sensed cycle on the count of each filter's last update lives on the device too: the
 * host-fed rfsgpu_batch_cycle_async and rfsgpu_batch_resample_async then return RFSGPU_ERR_UNSUPPORTED on this handle.  (Host-fed
 * cycles BEFORE the first sensed one are allowed: their counts move to the device.)  RFSGPU_ERR_INVALID, naming the filter: no
 * rfsgpu_batch_sense_async since the last cycle of either kind, a filter without a sensor.  Beyond
 * RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER particles per filter: RFSGPU_ERR_UNSUPPORTED. */
int rfsgpu_batch_cycle_sensed_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, int normalize);
/* rfsgpu_batch_resample_async with each filter's n_z taken from its record on the device.  After the sensed cycle and before the next
 * rfsgpu_batch_sense_async (else RFSGPU_ERR_INVALID: the records would be another cycle's). */
int rfsgpu_batch_resample_sensed_async(rfsgpu_filter *f, unsigned long long call);
/* The sets of the last rfsgpu_batch_sense_async: z [n_filters][RFSGPU_MAX_Z][2] (zeros beyond a filter's set), n_z [n_filters].
 * Synchronising, for tests and logging; a scan that was cut is reported here like by any synchronising call, with the outputs filled. */
int rfsgpu_batch_last_scan(rfsgpu_filter *f, double *z, int *n_z);
/* The section's switch for the other two kinds of batch: a batch of FastSLAM filters (rfsgpu_batch_set_fastslam_config or
 * rfsgpu_batch_fastslam_cycle_async has run) and a batch made by rfsgpu_create_batch_mh.  Off at creation; on = 0 restores the
 * refusals, and is itself refused with RFSGPU_ERR_INVALID once a sensed cycle has run on the handle.  RFSGPU_ERR_UNSUPPORTED, naming
 * which: an RB-PHD batch (it is served as it is), a batch whose kind is not decided yet, an ordinary handle, a shard of an
 * rfsgpu_group.  Synchronising.  With the switch on
 *   rfsgpu_batch_set_sensor, rfsgpu_batch_sense_async and rfsgpu_batch_last_scan serve the batch unchanged (the same kernel, the same
 *     draws, filter b's set at b * 2 * RFSGPU_MAX_Z of the measurement table);
 *   rfsgpu_batch_resample_sensed_async serves a FastSLAM batch after its sensed cycle and refuses a multi-hypothesis batch, which
 *     resamples inside its cycle;
 *   rfsgpu_batch_cycle_sensed_async keeps refusing both kinds (RFSGPU_ERR_UNSUPPORTED) and names the call of the kind below;
 *   rfsgpu_batch_run_truth_async ([truth]) serves both kinds.
 * A kind's per-filter record is configuration but for three fields: pfa = clutterIntensityIntegral / n_z (uniformClutterIntensity *
 * 2 pi (rangeLimMax - rangeLimMin) on the host, one correctly rounded division by the count on the device: the host-fed cycle's bits),
 * prune = n_z >= pruningMeasurementsThreshold, and the multi-hypothesis cycle's draw.  One kernel at the head of a sensed cycle, one
 * lane per filter, derives them from the sense call's records and a table of the static fields that is staged only when a
 * configuration has changed -- at the CYCLE, so a rfsgpu_batch_set_fastslam_config / rfsgpu_batch_configure between the sense call and
 * the cycle holds from this cycle on, as with the host-fed cycle (there is no "sense again" refusal here).  Results do not depend on
 * a sensor's max_nz.  Once a sensed cycle has returned RFSGPU_OK the filters' counts live on the device: the host-fed cycle of the
 * kind and rfsgpu_batch_resample_async return RFSGPU_ERR_UNSUPPORTED on this handle (host-fed cycles BEFORE the first sensed one are
 * allowed), and rfsgpu_batch_fastslam_last_cycle takes each filter's last count from the device records in its own read-back. */
int rfsgpu_batch_fastslam_serve_sensor(rfsgpu_filter *f, int on);
/* rfsgpu_batch_fastslam_cycle_async on the sets the last rfsgpu_batch_sense_async left (predict, x, x_cov, cov_stride, normalize as
 * there).  Puts the handle on the device route, as rfsgpu_batch_cycle_sensed_async does.  RFSGPU_ERR_INVALID, naming the filter: no
 * rfsgpu_batch_sense_async since the last cycle or the last rfsgpu_batch_set_sensor, a filter without a sensor.
 * RFSGPU_ERR_UNSUPPORTED: the switch is off, a batch of another kind (the text names its call). */
int rfsgpu_batch_fastslam_cycle_sensed_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, int normalize);
/* rfsgpu_batch_fastslam_mh_cycle_async likewise.  Filter b's u01 is the resampling draw of (its motion key, call): 53 bits of words
 * 0, 1 of Philox block (0, 2, call low word, call high word) over 2^53, the draw rfsgpu_batch_resample_async makes.  Refusals as
 * above, and RFSGPU_ERR_INVALID for a filter without rfsgpu_batch_set_motion_odometry (it has no key).  Nothing waits for the GPU. */
int rfsgpu_batch_fastslam_mh_cycle_sensed_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, unsigned long long call);
/* [test] Bytes of LDS that a workgroup of the step kernel had in the last cycle of this batch (host-fed or sensed; 0 before the
 * first) -- so that a test can say that two max_nz bounds gave two launch sizes and the same results.  Any batch; never waits. */
int rfsgpu_batch_last_cycle_lds(rfsgpu_filter *f, long long *bytes);

/* ---- [truth] every filter's ground truth drawn on the device, and a run of steps in one call (outside the STABLE CORE) -------------
 * generateTrajectory, generateOdometry and generateLandmarks of the reference's 2-D simulator (src/rbphdslam2dSim.cpp:146-284) for every
 * filter of a batch in one launch (csrc/batch_truth.h), by the rules the Python driver's generate() follows: n_steps poses, the noisy
 * odometry between them and the landmarks, plus each landmark's first-seen time (the third column of gtLandmark.dat) and the most
 * landmarks whose true range lies in [rmin, rmax] at any step.  The tables are step-major on the device: row k holds what call k of
 * the batch's device loop takes from the host -- the propagation input (odometry, the pose to pin to, the pin flag), the sensing
 * pose, the step error's time and pose -- so that a run of steps needs nothing from the host and is one call here.
 * Random numbers: Philox4x32-10 under the TRUTH's 64-bit key with counter (index, block | attempt << 8, 0, 0); the blocks follow the
 * sensor's (3 ... 7), so one key may serve a filter's motion, sensor and truth:
 *   block 8,  index = segment s:   attempt a of the segment's dx = u max_dx dt, u in [0, 1) from 53 bits of words 0, 1; drawn again while
 *                                  dx < min_dx dt; after 64 attempts the last draw is mapped: dx = (min_dx + u (max_dx - min_dx)) dt;
 *   block 9,  index = segment s:   dy = (u max_dy 2 - max_dy) dt from words 0, 1; dz likewise from words 2, 3 and max_dz;
 *   block 10, index = landmark j:  r = u1 rmax, b = u2 2 pi; the landmark is (x + r cos(theta + b), y + r sin(theta + b)) from the pose
 *                                  of the step that places it;
 *   block 11, index = step k:      g_x = rad cos ang, g_y = rad sin ang (the Box-Muller form of the batch's propagation);
 *   block 12, index = step k:      g_theta = rad cos ang;  odometry[k] = displacement[k] + sqrt(var_odo) dt g.
 * The steps up to n_still do not move; segment s starts at step max((k_full / n_segments) s, n_still + 1 + s); landmark j is placed at
 * step max((k_full / n_landmarks) j, j + 1) when that lies below n_steps (n_landmarks 0: none); pose[0] = 0 and pose[k] is
 * MotionModel_Odometry2d::step of pose[k - 1] by displacement[k].  A filter's truth depends neither on its place in the batch nor on
 * the other filters.  The realisations are the device's, not those of the Python driver's numpy generator: same model, other draws.
 * Every call of the section: RFSGPU_ERR_UNSUPPORTED on a handle that is not a filter batch (an ordinary handle, a shard of an
 * rfsgpu_group). */
#define RFSGPU_TRUTH_MAX_STEPS 4096   /* 112 bytes of tables per step and filter: at most 448 KiB a filter */
typedef struct rfsgpu_truth_config {
  int k_full;          /* the configured run length (kmax): segment and landmark spacing follow it, whatever n_steps is */
  int n_segments;      /* k_full / n_segments steps between two draws of the displacement                                */
  int n_landmarks;     /* k_full / n_landmarks steps between two landmarks (0: no landmarks)                             */
  int n_still;         /* the first steps, which do not move (the simulator's 50)                                        */
  int n_pinned;        /* steps k <= n_pinned pin the particles to the true pose (the simulator's 100)                   */
  double dt;
  double max_dx, max_dy, max_dz, min_dx;
  double var_odo[3];   /* vardx, vardy, vardz of the odometry noise                                                      */
  double rmax, rmin;   /* landmark placement and the first-seen limits                                                   */
} rfsgpu_truth_config;
/* Filter `filter`'s (-1: every filter's) configuration and Philox key for the next rfsgpu_batch_generate_truth.  Any kind of batch.
 * RFSGPU_ERR_INVALID with a message: a field that is negative or not finite, min_dx > max_dx, rmin >= rmax, n_segments < 1,
 * k_full / n_segments == 0, n_landmarks > 0 and k_full / n_landmarks == 0, more than RFSGPU_SENSOR_MAX_LANDMARKS landmarks that a run
 * of k_full steps could place.  Nothing waits for the GPU. */
int rfsgpu_batch_set_truth(rfsgpu_filter *f, int filter, const rfsgpu_truth_config *cfg, unsigned long long seed);
/* Draws n_steps steps (rows 0 ... n_steps - 1) of every filter's truth in one launch and waits for it; the tables of an earlier call
 * are replaced.  2 <= n_steps <= RFSGPU_TRUTH_MAX_STEPS and n_steps <= every filter's k_full, else RFSGPU_ERR_INVALID; a filter
 * without rfsgpu_batch_set_truth: RFSGPU_ERR_INVALID, naming the lowest such filter.  A refused call leaves the tables as they were. */
int rfsgpu_batch_generate_truth(rfsgpu_filter *f, int n_steps);
/* Filter `filter`'s tables for the host (synchronising; any pointer may be NULL): gt [n_steps][3], odom [n_steps][3], landmarks_xy and
 * first_seen with room for RFSGPU_SENSOR_MAX_LANDMARKS landmarks, of which the first *n_landmarks are written (first_seen = k dt of
 * the first step k >= 1 with the true range in [rmin, rmax], -1: none), *n_det_max the most landmarks in range at any step k >= 1.
 * The host configures the sensor (rfsgpu_batch_set_sensor) and the metric's ground truth (rfsgpu_set_ground_truth) from them.
 * RFSGPU_ERR_INVALID before the first rfsgpu_batch_generate_truth. */
int rfsgpu_batch_get_truth(rfsgpu_filter *f, int filter, double *gt, double *odom, double *landmarks_xy, double *first_seen, int *n_landmarks,
                           int *n_det_max);
/* Steps k_from ... k_to - 1 of a batch of RB-PHD filters (1 <= k_from <= k_to <= n_steps), each one the device loop's sequence with
 * the device sensor, its inputs read from row k of the tables: the propagation (call k), the scan at gt[k] (call k), the sensed cycle
 * (predict 1, no new poses, normalize 1), the sensed resampling (call k) and, with track_errors != 0, one row of the error log with
 * t = k dt and gt[k] (w_threshold, cutoff, order as rfsgpu_step_error_async).  Everything is enqueued here and stream-ordered;
 * nothing is read back, and device-side errors (gm_capacity, a cut scan) surface at the next synchronising call.  The same kernels
 * with the same arguments as the per-step calls: the same bits.  A batch of FastSLAM filters with rfsgpu_batch_fastslam_serve_sensor
 * on runs the same sequence with its own sensed cycle (rfsgpu_batch_fastslam_cycle_sensed_async); a multi-hypothesis batch with the
 * switch on runs propagation, scan, rfsgpu_batch_fastslam_mh_cycle_sensed_async with call k (its resampling is inside the cycle; the
 * thresholds of rfsgpu_batch_set_resampling have defaults there) and the log row, which needs rfsgpu_batch_mh_serve_metrics.
 * Refused before anything is enqueued -- RFSGPU_ERR_UNSUPPORTED: a batch of FastSLAM or multi-hypothesis FastSLAM filters whose
 * switch is off (as the [sensor] section refuses them), delayed births (RB-PHD), more than
 * RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER particles per filter; RFSGPU_ERR_INVALID, naming the filter: no rfsgpu_batch_generate_truth
 * yet, a range outside [1, n_steps], a filter without sensor, motion parameters or resampling thresholds, track_errors with a filter
 * that has no ground truth (rfsgpu_set_ground_truth) or without an error log; RFSGPU_ERR_CAPACITY: a log with fewer free rows than
 * the run has steps. */
int rfsgpu_batch_run_truth_async(rfsgpu_filter *f, int k_from, int k_to, int track_errors, double w_threshold, double cutoff, double order);

/* ---- [estimate] every filter's pose and map estimate per step, kept on the device (outside the STABLE CORE) ---------------------------
 * What the reference's simulators write per time step into particlePose.dat and landmarkEst.dat (src/rbphdslam2dSim.cpp:620-638,
 * src/fastslam2dSim.cpp:613-632) -- the particle set, and the map of the highest-weight particle with means, covariances and weights --
 * as one launch on the handle's stream (csrc/estimate_log.h) that appends one row to a device-side log beside the error log of
 * [metric].  The kernel reads the filter state as it is at that point of the stream and changes nothing of it; without a log nothing
 * runs.  The section is served exactly where [metric] is served, with [metric]'s refusals and texts: ordinary 2-D RB-PHD handles,
 * RB-PHD and FastSLAM batches, a multi-hypothesis batch once rfsgpu_batch_mh_serve_metrics(f, 1) has been called; everything else
 * gets RFSGPU_ERR_UNSUPPORTED from every call below.  The selection of the best particle, the weight of a Gaussian (a FastSLAM kind:
 * 1 - 1 / (1 + exp(log-odds))), the skipping of holes and the summation trees are [metric]'s, so best_slot, cardinality and
 * weight_sum of a row equal those of an rfsgpu_step_error record taken at the same point, bit for bit.
 * An ordinary handle that [metric] refuses -- the Victoria Park model, a handle that has run rfsgpu_fastslam_update or a FastSLAM
 * cycle -- is served by the four log calls once rfsgpu_handle_serve_estimates(f, 1) has been called (below), and a batch of Victoria
 * Park filters once rfsgpu_batch_vp_serve_estimates(f, 1) has been called (below it).
 * One record per filter and row; every field is 8 bytes wide. */
struct rfsgpu_step_estimate {
  double t;                 /* the time given with the call                                                                  */
  long long status;         /* 0 ok; 1: n_est > max_est, the Gaussians are cut to the first max_est in mixture order; 2 (a served
                               handle behind rfsgpu_fastslam_cycle_async / _cycle_full_async cycles only): a pending cycle overflowed
                               max_particles and was abandoned -- nothing of the filter state was read, the other fields are those
                               of a live count of 0 (n_particles, n_est, n_logged, cardinality 0, best_slot 0, pose and mean fields
                               NaN); the RFSGPU_ERR_CAPACITY itself comes from the next synchronising call, as always          */
  long long best_slot;      /* global slot of the highest-weight particle: the first slot of the filter's block whose weight is
                               strictly greater than every earlier one, starting from 0 (analysis2dSim.cpp:159-167); slot 0 of the
                               block when no weight is > 0                                                                   */
  long long n_particles;    /* slots the selection ran over: N, n_per_filter, or the LIVE count of a multi-hypothesis filter (or
                               of a served handle behind pending FastSLAM cycles)                                             */
  long long n_est;          /* the best particle's Gaussians with weight >= w_threshold (holes skipped, log-odds converted as in [metric]) */
  long long n_logged;       /* min(n_est, max_est)                                                                           */
  double cardinality;       /* sum of ALL its Gaussians' weights, the fixed tree of map_metric.h                             */
  double best_weight, weight_sum;   /* the best particle's weight, copied; the sum of the block's weights (the same tree)   */
  double best_x, best_y, best_theta;            /* the best particle's pose, copied                                          */
  double mean_x, mean_y, mean_cos, mean_sin;    /* sum w q / sum w over the block for q = x, y, cos theta, sin theta; the host takes atan2 */
};
/* The log: log_capacity rows; 0 <= max_est <= the handle's gm_capacity Gaussians kept per filter and row (else RFSGPU_ERR_INVALID);
 * log_particles != 0 keeps the particle set too.  Three arrays on the device, row-major:
 *   hdr   [cap][n_filters]                      one rfsgpu_step_estimate (128 bytes) per filter and row;
 *   gauss [cap][n_filters][6][max_est]          planes mx, my, sxx, sxy, syy, w (48 max_est bytes per filter and row);
 *   part  [cap][n_filters][4][slots]            planes x, y, theta, w; slots = n_particles of an ordinary handle (max_particles once
 *                                               rfsgpu_handle_serve_estimates is on: a multi-hypothesis set grows), n_per_filter of a
 *                                               batch, max_per_filter of a multi-hypothesis batch (32 slots bytes per filter and row);
 *                                               only the first n_particles entries of each plane of a row are written.
 * _create (re)allocates the log empty (synchronising; capacity 0 frees everything); an allocation that fails: RFSGPU_ERR_HIP and no
 * log is left.  _reset empties it; rows stay where they are until then. */
int rfsgpu_estimate_log_create(rfsgpu_filter *f, int log_capacity, int max_est, int log_particles);
int rfsgpu_estimate_log_reset(rfsgpu_filter *f);
/* Appends one row: t [n_filters] the time of each filter's step, copied into the pinned staging ring before the call returns (the
 * kernel reads it there); w_threshold as rfsgpu_step_error_async's (-inf: every Gaussian of the particle, what landmarkEst.dat holds).
 * Stream-ordered, nothing waits for the GPU.  A full log (or none): RFSGPU_ERR_CAPACITY, nothing is enqueued. */
int rfsgpu_step_estimate_async(rfsgpu_filter *f, const double *t, double w_threshold);
/* Synchronises the stream and copies those of the rows [row_from, row_from + max_rows) that exist: hdr [rows][n_filters], gauss
 * [rows][n_filters][6][max_est], part [rows][n_filters][4][slots] (any may be NULL; part is ignored by a log without particles);
 * *n_rows = the number of rows in the log.  row_from outside [0, rows] or max_rows < 0: RFSGPU_ERR_INVALID.  The log keeps its rows:
 * with _reset a long run is drained in chunks. */
int rfsgpu_estimate_log_read(rfsgpu_filter *f, int row_from, int max_rows, struct rfsgpu_step_estimate *hdr, double *gauss, double *part,
                             int *n_rows);
/* on != 0: from now on every step of rfsgpu_batch_run_truth_async also appends one estimate row (w_threshold as above), taken at the
 * point of the stream where that step's error row is taken (behind the step's resampling), its t read from the truth table row on the
 * device; all three kinds of batch.  The run call then also checks, before anything is enqueued, that an estimate log exists and has
 * as many free rows as the run has steps (else RFSGPU_ERR_CAPACITY), and that [metric] serves the handle.  Off (the default) the run
 * enqueues exactly what it enqueues without this section.  RFSGPU_ERR_UNSUPPORTED on a handle that is not a filter batch. */
int rfsgpu_batch_run_log_estimates(rfsgpu_filter *f, int on, double w_threshold);
/* The switch of an ORDINARY handle, of either model and either filter class; off at creation, and while it is off every call of this
 * section behaves as described above, with the same codes and texts.  on != 0 (synchronising; before or after the first
 * rfsgpu_fastslam_update or cycle): rfsgpu_estimate_log_create, _reset, _read and rfsgpu_step_estimate_async work on the handle with
 * the signatures and log semantics above; rfsgpu_batch_run_log_estimates and every [metric] call keep refusing as they do.  What a
 * row means there:
 *   - the Victoria Park model: the six Gaussian planes are u(0), u(1), S(0,0), S(0,1), S(1,1) and w of the 3-D landmarks -- what the
 *     reference's Victoria Park drivers print (src/rbphdslam_VictoriaPark.cpp:586-622, src/fastslam_VictoriaPark.cpp:576-611); the
 *     diameter and its covariances are not logged;
 *   - a handle on which rfsgpu_fastslam_update or a FastSLAM cycle has run: a Gaussian's weight is 1 - 1 / (1 + exp(w)) of its
 *     log-odds w, as on a FastSLAM batch (fastslam_VictoriaPark.cpp:609);
 *   - the part planes have max_particles slots, max_est stays within 0 ... gm_capacity;
 *   - n_particles is the host's count while nothing of a FastSLAM cycle is pending, and the device's count (the cycle block's word,
 *     clamped to [0, max_particles], read by the kernel where it runs) behind pending rfsgpu_fastslam_cycle_async / _cycle_full_async
 *     cycles; no slot at or beyond it is read.  Status 2 (above) where such a cycle overflowed.
 * rfsgpu_step_estimate_async then enqueues WITHOUT resolving the pending device cycles where only rfsgpu_rbphd_cycle_async cycles
 * are pending, or only FastSLAM cycles (no stashed error, no rfsgpu_resample_async): a device-cycle run carries its log with it and
 * reads it once at the end.  In every other pending state it resolves first; _create and _read synchronise.
 * on == 0: synchronises, frees an existing log and restores the refusals.  RFSGPU_ERR_UNSUPPORTED, naming the reason: a batch of any
 * kind, a shard of an rfsgpu_group.  RFSGPU_ERR_INVALID: a null handle. */
int rfsgpu_handle_serve_estimates(rfsgpu_filter *f, int on);
/* The switch of a BATCH OF VICTORIA PARK FILTERS (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D); off at creation, and while it
 * is off every call of this section refuses such a batch as described above, with the same codes and texts.  on != 0 (synchronising):
 * rfsgpu_estimate_log_create, _reset, _read and rfsgpu_step_estimate_async serve the batch with the signatures and log semantics above:
 * hdr [cap][n_filters], gauss [cap][n_filters][6][max_est] with 0 <= max_est <= gm_capacity, part [cap][n_filters][4][n_per_filter],
 * t [n_filters].  A filter's row is the row of a Victoria Park handle that rfsgpu_handle_serve_estimates serves, from the same code in
 * the same order, so it carries the bits such a handle holding the same state produces: the six planes are u(0), u(1), S(0,0), S(0,1),
 * S(1,1) and w of the best particle's 3-D landmarks (no diameter), weights are plain weights, best_slot is a GLOBAL slot (filter b's
 * lies in [b n_per_filter, (b + 1) n_per_filter)), n_particles is n_per_filter, status is 0 or 1.
 * rfsgpu_step_estimate_async is stream-ordered on both routes of such a batch and waits for nothing: it reads weights, poses, counts
 * and the current slab where it stands in the stream and changes nothing; on the device route it neither resolves anything nor takes
 * the ids, flags or counters over (a row enqueued behind rfsgpu_batch_vp_resample_async sees the gathered state).  A full log, or no
 * log: RFSGPU_ERR_CAPACITY, nothing is enqueued.  rfsgpu_batch_run_log_estimates, every [metric] call and
 * rfsgpu_handle_serve_estimates keep refusing the batch as they do.
 * on == 0: synchronises, frees an existing log and restores the refusals.  RFSGPU_ERR_UNSUPPORTED with the state untouched, naming
 * the call that serves it: a 2-D, FastSLAM or multi-hypothesis batch, an ordinary handle, a shard of an rfsgpu_group.
 * RFSGPU_ERR_INVALID: a null handle. */
int rfsgpu_batch_vp_serve_estimates(rfsgpu_filter *f, int on);

#ifdef __cplusplus
}
#endif
#endif /* RFSGPU_H */
