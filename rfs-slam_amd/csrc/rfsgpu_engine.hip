// rfsgpu_engine.hip -- host side of the C ABI in include/rfsgpu.h: device memory, kernel launches, timing.
// One handle == one GPU == one shard of particles.  No CPU fallback: every entry point either runs the HIP
// kernels or returns an error status.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define RFSGPU_ENABLE_BENCH_API 1   // the library defines (and exports) the [bench] / [test] entry points too
#include "rfsgpu.h"
#include "common.h"
#include "update_map.h"
#include "weighting.h"
#include "merge_prune.h"
#include "step_fused.h"
#include "murty.h"
#include "mat_perm.h"
#include "vp.h"
#include "birth.h"
#include "fastslam.h"
#include "fastslam_mh.h"
#include "fastslam_cycle.h"
#include "motion.h"
#include "map_metric.h"
#include "estimate_log.h"
#include "batch_loop.h"
#include "batch_sensor.h"
#include "batch_truth.h"
#include "fastslam_sensed.h"
#include "resample_plan.h"
#include "birth_walk.h"
#include "vp_batch.h"
#include "vp_batch_loop.h"
#include "scan_fov.h"

namespace {

inline long long now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

enum { EV_UM0 = 0, EV_UM1, EV_W1, EV_MG1, EV_PR1, EV_P0, EV_P1, EV_R0, EV_R1, EV_COUNT };

// A ring of pinned staging blocks (ring_acquire): a call writes its inputs into the next block, enqueues the copies or kernels that read
// it and records the block's event behind the last of them; the block is handed out again once that event has passed.
struct PinnedRing {
  unsigned char *h[8] = {};
  hipEvent_t ev[8] = {};
  int depth = 4, next = 0;   // blocks in use (4 or 8), cursor
  size_t bytes = 0;          // of one block (set where the handle is created)
};

// What a filter batch steps.  A 2-D batch is created undecided and its first cycle call (or rfsgpu_batch_set_fastslam_config) decides
// for good; a Victoria Park batch is created stepping RB-PHD filters and rfsgpu_batch_vp_serve_fastslam moves it until a cycle has
// run; rfsgpu_create_batch_mh / _vp_mh create the multi-hypothesis kinds.
enum BatchSteps { STEPS_UNDECIDED = 0, STEPS_RBPHD, STEPS_FASTSLAM, STEPS_MH };

}  // namespace

struct rfsgpu_filter {
  int device = 0;
  int N = 0, cap = 0;       // particles in use, Gaussians per particle
  int snapN = 0;            // particle count of the saved state
  int Ncap = 0;             // particle slots allocated (rfsgpu_create_ex >= N): the multi-hypothesis FastSLAM update grows N up to it
  int model = RFSGPU_MODEL_RNGBRG_2D;
  int D = 2;          // d_m == d_z
  rfsgpu_vp_config vp{};
  double vpClutter = 0.0;
  hipStream_t stream = nullptr;
  hipStream_t ownStream = nullptr;
  double *ownSums = nullptr;
  // snapshot slot (rfsgpu_save_state)
  double *snapSlab = nullptr, *snapWeight = nullptr;
  int *snapCount = nullptr, *snapFov = nullptr;
  unsigned long long *snapUnused = nullptr;
  int snapNZ = 0;
  // ring of pre-seeded copies of the saved state (rfsgpu_state_ring_*): a timed step takes its input from the next slot by a pointer swap
  struct RingSlot { double *slab = nullptr, *weight = nullptr; int *count = nullptr, *fov = nullptr; unsigned long long *unused = nullptr; };
  std::vector<RingSlot> stateRing;
  size_t stateRingPos = 0;
  hipEvent_t ev[EV_COUNT] = {};
  Buffers B{};
  int cur = 0;
  Params P{};
  rfsgpu_filter_config cfg{};
  rfsgpu_rngbrg_config rb{};
  rfsgpu_kf_config kf{};
  double Qlm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int nZ = 0;  // measurements of the last update (birth uses them)
  double *dSums = nullptr;  // [2]
  int *dSrcSlot = nullptr;  // [N]
  int *dRowSlots = nullptr; // slots of the rows being exported / imported (allocated on first use, grown on demand)
  int rowSlotsCap = 0;
  PinnedRing stage;                   // staging ring of rfsgpu_set_step_inputs_async and every other call that hands the device a few host arrays
  double *hWeights = nullptr;         // pinned landing buffer of rfsgpu_get_weights
  double *hOutW = nullptr;            // pinned: where the post kernel leaves the weights of a synchronous rfsgpu_update_io ...
  int *hOutFlag = nullptr;            // ... and {error word, sequence number} behind them (same allocation)
  int outSeq = 0;                     // sequence number of the last delivery asked for
  bool outArmed = false;              // the step in flight delivers through hOutW / hOutFlag (update_io_end spins instead of synchronising)

  int stagePendingSlot = -1;          // a staging slot whose event must be recorded behind the step that reads it
  bool gateIndex = true;              // RFSGPU_GATE_INDEX=0 at create: the map update finds its gate candidates by the dense sweep (update_map.h), for A/B runs against the index
  bool denseIntensity = false;        // RFSGPU_DENSE_INTENSITY=1 at create: deviation 9 off (the dense loop for every mixture size), for runs against a future pinned fixture
  bool ioPull = true;                 // RFSGPU_IO_PULL=0: inputs by copy commands, outputs by copies + a stream synchronisation (A/B, rounds 3-4 form)
  int vpParity = 0;                   // which pair of duration extrema (vpCost[Ncap ..]) the next post kernel reads
  float *vpCost = nullptr;            // [Ncap + 4] Victoria Park fused step: last measured duration per particle (100 MHz ticks)
  int *vpOrder = nullptr;             // [Ncap] launch slot -> particle (identity until the first post kernel has sorted the costs)
  int vpOrderN = -1;                  // particle count the order array is valid for
  int vpOrderMode = 2;                // 0 slot == particle | 1 a host-given order, frozen | 2 re-sorted by every step's post kernel (default; RFSGPU_VP_COST_ORDER=0: 0)
  int collProbeSeq = 0;               // probes made so far (rfsgpu_collective_probe)
  int *dCollSeq = nullptr;            // [2 + 2] device: {number of the last step whose sums are out, number of the last step whose collective is done} (rfsgpu_step_async_trailing)
  int collStep = 0;                   // steps issued in the event-free trailing form
  double *poseAlt = nullptr;          // [Ncap][3] second pose buffer: a fused predict + update cycle births at the old poses and updates at the new ones (rfsgpu_cycle_async)
  bool predPending = false;  // rfsgpu_predict_map_async's event pair has not been accumulated yet
  bool candUsed = false;     // candidate lists were imported or the FastSLAM path ran with landmark candidates: migration rows carry them
  bool poseCovZero = false;  // B.poseCov[0..9) holds zeros (the "no covariance" form), so a further cov == NULL push need not rewrite it
  MurtyQueue Q{};
  MurtyScratch MS{};
  int *hErr = nullptr;      // pinned
  int *hJobCount = nullptr; // pinned
  double *hSums = nullptr;  // pinned [2]
  rfsgpu_timing timing{};
  long long lastKernelNs[4] = {0, 0, 0, 0};
  int lastStepVariant[4] = {0, 0, 0, 0};   // the last stream-ordered step: {waves per particle, phase priorities, merge grid log2, fused}
  bool phaseOpen = false;   // update_map ran, weighting/merge/prune may follow
  bool normPending = false; // a normalize_kernel event pair has not been accumulated yet
  // async steps: ring of per-phase event sets, harvested at the next sync
  hipEvent_t ring[RFSGPU_ASYNC_RING][5] = {};  // step phases: 0 start, 1 map update done, 2 weighting (+Murty) done, 3 merge done, 4 weighting kernel done
  bool ringHasMid[RFSGPU_ASYNC_RING] = {};
  bool ringFused[RFSGPU_ASYNC_RING] = {};   // the step ran as ONE kernel: only events 0 and 3 were recorded
  rfsgpu_fastslam_config fs;          // FastSLAM::Config (rfsgpu_fastslam_update)
  unsigned char *fsArena = nullptr;   // per-particle Hungarian scratch (allocated on first use)
  unsigned char *mhArena = nullptr;   // multi-hypothesis FastSLAM: per-particle table / Murty arena / assignments
  int *mhInts = nullptr;              // [5][Ncap] slotSrc, slotHyp, slotNH, copyDst, copySrc
  bool fsResampleOccured = false;     // FastSLAM::resampleOccured_ of the previous update (rfsgpu_fastslam_set_resample_occured)
  std::vector<int> parents;           // source slot of every particle after the last FastSLAM update (identity when none multiplied)
  // rfsgpu_fastslam_cycle_async (fastslam_cycle.h): the whole FastSLAM::update on the device
  unsigned char *mhcBlock = nullptr;  // device: the FsCycleState block
  unsigned char *hMhcBlock = nullptr; // pinned: where it lands when the host next synchronises
  int *mhcInts = nullptr;             // [4][Ncap] slotHyp, slotNH, copyDst, copySrc (slotSrc is in the block)
  FsCycleState mhc{};                 // the block's device view
  bool mhcPending = false;            // cycles are enqueued and N, fsResampleOccured, the ids and `parents` are behind the device
  bool mhcIdsDirty = true;            // pid / ppid changed on the host since the device copy was written
  bool mhcHave = false;               // a cycle has run (rfsgpu_fastslam_last_cycle has something to report)
  bool mhcLastEmpty = false;          // the last enqueued cycle had no measurements
  int mhcStashedRc = 0;               // a pending cycle's error met by a call that cannot return it: returned by the next call that can
  std::vector<char> mhcFlips;         // per pending cycle with measurements: whether it flipped `cur` (its prune ran)
  int mhcDone = 0;                    // FSC_DONE as last read
  int mhcNFired = 0;                  // FSC_NFIRED as last read
  double fsEffN = -1.0, fsEffNPercent = -1.0;   // rfsgpu_fastslam_set_resampling (negative: n_particles / 4 and 1 / 4 at the first cycle)
  int mhcNGrown = 0, mhcNAfter = 0, mhcFired = 0;   // the last cycle, as resolved
  double mhcNEff = 0.0;
  std::vector<int> mhcPlan;
  // rfsgpu_resample_async (resample_plan.h): ParticleFilter::resample on the device for an ordinary handle
  unsigned char *rsBlock = nullptr;   // device: the ResampleState block (allocated on first use)
  unsigned char *hRsBlock = nullptr;  // pinned: where its head lands when the host next resolves | [2][Ncap] the ids on their way up
  ResampleState rs{};                 // the block's device view
  bool rsPending = false;             // a call is enqueued: the ids, resampleOccured, externalAck (and N when it shrinks) are behind the device
  bool rsShrink = false;              // ... and it may change the particle count (n_out < N): every call resolves it first
  bool rsHave = false;                // a call has run (rfsgpu_last_resample has something to report)
  std::vector<int> rsIdsDev;          // [2][Ncap] pid | ppid as the device block holds them (empty: never written)
  int rsFired = 0, rsNAfter = 0;      // the last call, as resolved
  double rsNEff = 0.0;
  std::vector<int> rsPlan;
  // rfsgpu_rbphd_cycle_async (birth_walk.h): RBPHDFilter::update's counters, gate and resampling on the device, in words of rsBlock
  bool rcPending = false;             // cycles are enqueued: the ids and resampleOccured are behind the device (the count never changes)
  bool rcHave = false;                // a cycle has run: the host route of the resampling is closed on this handle
  bool rcLastEmpty = false;           // the last enqueued cycle had no measurements
  double rcEffN = -1.0, rcEffNPercent = -1.0;   // rfsgpu_rbphd_set_resampling (negative: n_particles / 4 and 1 / 4)
  int rcGate = 0, rcFired = 0, rcWalkMax = 0;   // the last cycle and the last walk, as resolved
  double rcNEff = 0.0;
  std::vector<int> rcPlan;
  int rcCounts[4] = {0, 0, 0, 0};     // cycles | with an open gate | that resampled | the deepest inheritance level of a walk
  // birth-state inheritance after a resampling (rfsgpu_set_birth_inheritance; RBPHDFilter.hpp:1005-1011)
  int inheritMode = RFSGPU_INHERIT_REFERENCE;
  std::vector<int> pid, ppid;         // Particle::id_ / idParent_ of the particle in each slot (ParticleFilter.hpp:446-479)
  bool resampleOccured = false;       // RBPHDFilter::resampleOccured_
  bool externalAck = true;            // RFSGPU_INHERIT_EXTERNAL: the host has taken care of the inheritance rule since the last resampling (rfsgpu.h)
  bool fastSlamHandle = false;        // rfsgpu_fastslam_update has run: the filter class is rfs::FastSLAM, whose resampleWithMapCopy
                                      // copies the candidate lists right at resampling time (FastSLAM.hpp:747-753) -> eager copies
  int *dInhParent = nullptr, *dInhLevel = nullptr;   // [Ncap] each (allocated on first use)
  BirthLists inhTmp{};                // staging area of birth_inherit_kernel<0/1> (allocated on first use)
  std::vector<int> hInhParent, hInhLevel;
  bool holes = false;       // between rfsgpu_merge and rfsgpu_prune merged-away entries sit in the slab with w = -1; at any other
                            // time a negative weight is a value (FastSLAM's log-odds) and every stored entry counts
  int nCU = 256;            // multiProcessorCount of the device
  bool fuseSteps = true;    // rfsgpu_update / _update_async / _step_async use phd_step_fused_kernel (2-D model); RFSGPU_FUSED_STEP=0 turns it off
  bool phaseTiming = false; // rfsgpu_set_phase_timing: rfsgpu_update runs its phases as separate launches (TimingInfo per phase)
  int stepWppOverride = 0;  // RFSGPU_STEP_WPP: waves per particle of the fused step kernel (2 or 3); 0 = chosen per launch
  int updMapWppOverride = 0;  // RFSGPU_UPDMAP_WPP at create: waves per particle of the stand-alone map update (1 .. 4); 0 = chosen by capacity
  unsigned stepSeq = 0;      // fused steps launched so far
  int timingStride = 8;      // every timingStride-th of them carries the timing events (rfsgpu_set_step_timing_stride; round 5: 8 by default --
                             // three marker packets per step cost a configs[1] step 8 us; the FIRST step of a filter is always timed)
  int untimedSince = 0;      // fused steps launched since the last one that carried events (and not yet booked into TimingInfo)
  long long lastFusedNs = 0; // duration of the last sampled fused step (what an un-sampled step is booked at)
  int ringStands[RFSGPU_ASYNC_RING] = {};   // how many steps a timed ring entry stands for in TimingInfo (itself + the untimed ones before it)
  int mergeGridOverride = 0; // RFSGPU_MERGE_GRID: log2 of the merge grid's cells per side in the three-wave fused kernel (5 or 6); 0 = chosen per launch
  hipEvent_t evAfterWeightKernel = nullptr;   // where launch_weighting drops its mid-phase event (async steps only)
  int ringCount = 0;        // async steps recorded since the last harvest
  double statNs[3] = {0, 0, 0};
  double lastPostNs = 0;
  double statPostNs = 0;    // fused steps: the post kernel's share (rfsgpu_post_kernel_time_stats)
  int statSteps = 0;
  std::string err;
  int maxLds = 0;
  int wpbUpdate = 4, wpbWeight = 4, wpbMerge = 4, wpbPrune = 4;
  // filter batch (rfsgpu_create_batch): nF independent filters of nPer particles, filter b in slots [b * nPer, (b + 1) * nPer)
  bool batch = false;
  int nF = 1, nPer = 0;
  std::vector<rfsgpu_filter_config> bCfg;
  std::vector<rfsgpu_rngbrg_config> bRb;
  std::vector<rfsgpu_kf_config> bKf;
  std::vector<double> bQ;             // [nF][9]
  std::vector<rfsgpu_vp_config> bVp;  // a batch of Victoria Park filters: each filter's model ...
  std::vector<double> bVpClutter;     // ... and its clutter density, expectedClutterNumber / FoV area of the scan that was current when it was last derived
  std::vector<int> bNZ;               // measurements of each filter's last update (its next births)
  std::vector<char> bResampled;       // RBPHDFilter::resampleOccured_ per filter
  bool bParamsDirty = true;           // the device Params table is behind the host configuration
  int bHandleWide[3] = {-1, -1, -1};  // the handle-wide Params fields the table was built with (pose covariance stride, partition mode, dense intensity)
  BatchFilter *dBFilt = nullptr;      // [nF]
  Params *dBParams = nullptr;         // [nF]
  double *dBZ = nullptr;              // [nF][RFSGPU_MAX_Z * D] this cycle's sets, packed
  double *dBZPrev = nullptr;          // [nF][RFSGPU_MAX_Z * D]
  double *dBSums = nullptr;           // [nF][2]
  int *dBErrFilter = nullptr;         // [2] BatchArg::errFilter
  unsigned long long *dBMaskTmp = nullptr;   // [N] birth inheritance: the masks before the walk
  int *dBInhSrc = nullptr;            // [N]
  PinnedRing bStage;                  // ring of the per-cycle tables (batch_push_tables)
  // the device loop of a batch (batch_loop.h): propagation and resampling without the host
  std::vector<char> bMotionSet, bResSet;       // rfsgpu_batch_set_motion_odometry / _set_resampling have been called for the filter
  std::vector<BatchMotion> bMotion;
  std::vector<double> bEffN;                   // [nF][2] eff_n, eff_n_percent
  bool bMotionDirty = true;
  bool bBirthAlt = false;                      // poseAlt holds the poses from before the last rfsgpu_batch_propagate_async: the next cycle's births
  bool bDevRoute = false;                      // the ids, resampleOccured_ and the resampling counters live on the device (first rfsgpu_batch_resample_async)
  BatchMotion *dBMotion = nullptr;             // [nF]
  BatchPropIn *dBPropIn = nullptr;             // [nF]
  BatchResIn *dBResIn = nullptr;               // [nF]
  BatchLoopState BL{};
  PinnedRing bLoop;                            // ring of the loop calls' per-filter inputs, a block per call (eight blocks: propagate + resample, four cycles; with a sense call three per cycle, 2 2/3 cycles)
  // the device route of a batch of Victoria Park filters (vp_batch_loop.h)
  std::vector<VpBatchMotion> bVpMotion;        // [nF] rfsgpu_batch_vp_set_motion
  VpBatchMotion *dBVpMotion = nullptr;         // [nF]
  VpBatchRun *dBVpRun = nullptr;               // [1] the run of the last rfsgpu_batch_vp_propagate_run_async
  int *dBVpWalk = nullptr;                     // [VBW_FILTER + nF] the walk's words
  // the sensor of a batch (batch_sensor.h): every filter's scan drawn on the device
  std::vector<char> bSensorSet;                // rfsgpu_batch_set_sensor has been called for the filter
  std::vector<int> bSensorMaxNz;               // [nF] its max_nz
  std::vector<int> bSensorCaps;                // [nF][2] evalCap, useW as the device table holds them (-1: not staged yet)
  BatchSensor *dBSensor = nullptr;             // [nF]
  double *dBSensorLm = nullptr;                // [nF][SENSOR_MAX_LANDMARKS][2]
  double *dBSensorPose = nullptr;              // [nF][3]
  int *dBSensorCaps = nullptr;                 // [nF][2]
  int *dBSensorPrev = nullptr;                 // [nF] BatchSensorArg::prevCount
  int *dBSensorErrFilter = nullptr;            // [1] BatchSensorArg::errFilter
  bool bSenseFresh = false;                    // a sense call has run since the last cycle and no rfsgpu_batch_set_sensor since: the records and sets on the device are this cycle's
  long long bLastCycleLds = 0;                 // bytes of LDS a workgroup of the last batch cycle's step kernel had (rfsgpu_batch_last_cycle_lds)
  int bSenseNzMax = 0, bSenseEcMax = 1;       // the largest max_nz and evalCap that sense call's records can carry: the sensed cycle's launch is sized for them
  bool bScanHeld = false;                      // the records and sets on the device are a sense call's (no host-fed cycle has written over them): rfsgpu_batch_last_scan may read them
  bool bSensedTail = false;                   // a sensed cycle has run since the last sense call: rfsgpu_batch_resample_sensed_async may read its records
  bool bSensed = false;                        // a sensed cycle has run on this handle: nZprev lives on the device, the host-fed cycle and resampling refuse
  // the truth of a batch (batch_truth.h): every filter's trajectory, odometry and landmarks drawn on the device, in step-major tables
  std::vector<char> bTruthSet;                 // rfsgpu_batch_set_truth has been called for the filter
  std::vector<BatchTruth> bTruth;              // [nF] as the next generation uploads it
  int truthK = 0;                              // steps the tables hold (0: no generation yet)
  size_t truthRows = 0;                        // rows the step tables have room for
  BatchTruth *dTruthCfg = nullptr;             // [nF]
  BatchPropIn *dTruthProp = nullptr;           // [truthRows][nF]
  double *dTruthGt = nullptr;                  // [truthRows][nF][3]
  double *dTruthTgt = nullptr;                 // [truthRows][nF][4]
  double *dTruthLm = nullptr;                  // [nF][SENSOR_MAX_LANDMARKS][2]
  double *dTruthSeen = nullptr;                // [nF][SENSOR_MAX_LANDMARKS]
  int *dTruthCounts = nullptr;                 // [nF][2]
  // a batch of FastSLAM filters (rfsgpu_batch_fastslam_cycle_async; fastslam.h FsBatchArg)
  BatchSteps bSteps = STEPS_UNDECIDED;         // what the batch steps; with D (the model) and bStepsLocked, all there is to its kind: the predicates and transitions below the struct
  bool bStepsLocked = false;                   // bSteps no longer moves
  std::vector<rfsgpu_fastslam_config> bFs;     // [nF]
  std::vector<Params> bParamsHost;             // [nF] the device Params table as last written (each filter's pfa comes from its own model)
  FsBatchFilter *dFsFilt = nullptr;            // [nF]
  // a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh; fastslam_cycle.h): nPer is the stride max_per_filter, every
  // filter has its own cycle block on the device and its live count is a word of it
  int nInitPer = 0;                            // n_per_filter: the count a filter starts with and a resampling brings it back to
  unsigned char *mhbBlock = nullptr;           // device: nF cycle blocks of fs_cycle_state_bytes(nPer) bytes
  unsigned char *hMhbBlock = nullptr;          // pinned: where they land when the host next synchronises
  MhBatchFilter *dMhFilt = nullptr;            // [nF] this cycle's per-filter records
  bool mhbPending = false;                     // cycles are enqueued: the counts, ids and flags on the host are behind the device
  bool mhbHave = false;                        // a cycle has run
  std::vector<int> mhbLastNZ;                  // [nF] the last enqueued cycle's measurement counts
  // the device sensor on a FastSLAM / multi-hypothesis batch (rfsgpu_batch_fastslam_serve_sensor; fastslam_sensed.h)
  bool mhbLastSensed = false;                  // the last enqueued multi-hypothesis cycle was a sensed one: mhb_resolve reads mhbLastNZ back from its records
  bool bServeSensor = false;                 // the switch: the [sensor] and [truth] calls serve this batch
  void *dFsTmpl = nullptr;                     // [nF] FsSensedTemplate<FsBatchFilter | MhBatchFilter>: the records' static part (allocated by the switch)
  std::vector<unsigned char> bFsTmplHost;      // the table as the device holds it (empty: not staged yet)
  int *dFsLastNZ = nullptr, *hFsLastNZ = nullptr;   // [nF] a multi-hypothesis batch: the counts of the last sensed cycle's records, compact on the device | pinned, where mhb_resolve lands them
  bool mhbMetrics = false;                     // rfsgpu_batch_mh_serve_metrics: the [metric] calls serve this batch (the kernel's live-count form)
  // [metric] per-step map / pose error (map_metric.h): ground truth per filter, the device-side log, one row for the synchronous calls
  double *dGtXY = nullptr, *dGtSeen = nullptr;   // [nF][RFSGPU_MAX_METRIC_SET][2], [nF][RFSGPU_MAX_METRIC_SET] (allocated by the first rfsgpu_set_ground_truth)
  int *dGtN = nullptr;                           // [nF]
  std::vector<char> gtSet;                       // [nF] rfsgpu_set_ground_truth has been called for the filter
  struct rfsgpu_step_error *dErrLog = nullptr;          // [errLogCap][nF]
  int errLogCap = 0, errLogRows = 0;
  struct rfsgpu_step_error *dErrRow = nullptr;          // [nF]
  // [estimate] per-step pose / map estimates (estimate_log.h): the device-side log beside dErrLog
  struct rfsgpu_step_estimate *dEstHdr = nullptr;       // [estLogCap][nF]
  double *dEstGauss = nullptr;                          // [estLogCap][nF][6][estMax] (nullptr with estMax 0)
  double *dEstPart = nullptr;                           // [estLogCap][nF][4][estSlots] (nullptr: the log keeps no particles)
  int estLogCap = 0, estLogRows = 0, estMax = 0, estSlots = 0;
  bool estRunOn = false;                                // rfsgpu_batch_run_log_estimates: rfsgpu_batch_run_truth_async appends a row per step
  double estRunThr = 0.0;
  bool estServe = false;                                // rfsgpu_handle_serve_estimates: the [estimate] log calls serve this ordinary handle (either model, either filter class)
  bool estServeVpBatch = false;                         // rfsgpu_batch_vp_serve_estimates: the [estimate] log calls serve this batch of Victoria Park filters
  bool groupShard = false;                       // a shard of an rfsgpu_group: the [metric] calls refuse
};

// ---- the kind of a filter batch: bSteps, bStepsLocked and D (the model).  What the code asks of it ...
static inline bool batch_is_vp(const rfsgpu_filter *f) { return f->batch && f->D == 3; }     // a batch of Victoria Park filters, whatever it steps
static inline bool batch_is_mh(const rfsgpu_filter *f) { return f->bSteps == STEPS_MH; }      // multi-hypothesis filters, either model: a filter's live count is a word of its cycle block
static inline bool batch_fills_blocks(const rfsgpu_filter *f) { return !batch_is_mh(f); }     // every filter fills its block
static inline bool batch_is_vp_fastslam(const rfsgpu_filter *f) { return batch_is_vp(f) && f->bSteps == STEPS_FASTSLAM; }
static inline bool batch_is_vp_mh(const rfsgpu_filter *f) { return batch_is_vp(f) && batch_is_mh(f); }
// (resample_gather_kernel's mapOnly: the candidate lists, the mask and the in-view count travel with the particle only on a batch of
//  Victoria Park FastSLAM filters -- a 2-D FastSLAM batch keeps no lists)
static inline int batch_map_only(const rfsgpu_filter *f) { return batch_is_vp_fastslam(f) ? 0 : 1; }
static inline bool batch_log_odds(const rfsgpu_filter *f) { return f->bSteps == STEPS_FASTSLAM || f->bSteps == STEPS_MH; }
// ... and how it moves.  rfsgpu_create_batch: a Victoria Park batch steps RB-PHD filters until its switch says otherwise
static inline void batch_born(rfsgpu_filter *f) { f->bSteps = f->D == 3 ? STEPS_RBPHD : STEPS_UNDECIDED; }
// A 2-D batch's first cycle call, or rfsgpu_batch_set_fastslam_config: decides an undecided batch for good and moves no other (the
// caller has refused a batch of another kind under its own wording)
static inline void batch_decide(rfsgpu_filter *f, BatchSteps s) {
  if (f->bSteps == STEPS_UNDECIDED) { f->bSteps = s; f->bStepsLocked = true; }
}
// rfsgpu_batch_vp_serve_fastslam moves a Victoria Park batch between RB-PHD and FastSLAM filters until a cycle of either kind has run
static inline bool batch_vp_may_step(const rfsgpu_filter *f, BatchSteps s) { return !f->bStepsLocked || f->bSteps == s; }
static inline void batch_vp_cycle_ran(rfsgpu_filter *f) { f->bStepsLocked = true; }
// rfsgpu_create_batch_mh, rfsgpu_create_batch_vp_mh: a kind of its own from creation
static inline void batch_born_mh(rfsgpu_filter *f) { f->bSteps = STEPS_MH; f->bStepsLocked = true; }
// What a handle is and the cycle call that serves it: the tail of every "..., not <this>" and "not available on <this>" refusal
static const char *handle_kind_text(const rfsgpu_filter *f) {
  if (!f->batch)
    return f->groupShard ? "a shard of an rfsgpu_group (the rfsgpu_group_* calls step it)"
                         : "an ordinary handle (rfsgpu_cycle_async or rfsgpu_rbphd_cycle_async; with rfsgpu_set_fastslam_config, rfsgpu_fastslam_update or rfsgpu_fastslam_cycle_full_async)";
  if (f->D == 3) {
    if (f->bSteps == STEPS_MH) return "a batch of Victoria Park multi-hypothesis FastSLAM filters (rfsgpu_create_batch_vp_mh; its cycle is rfsgpu_batch_vp_fastslam_mh_cycle_async)";
    if (f->bSteps == STEPS_FASTSLAM)
      return "a batch of Victoria Park FastSLAM filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D, rfsgpu_batch_vp_serve_fastslam on; its cycle is rfsgpu_batch_vp_fastslam_cycle_async)";
    return "a batch of Victoria Park RB-PHD filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D; its cycle is rfsgpu_batch_vp_cycle_async)";
  }
  switch (f->bSteps) {
    case STEPS_MH: return "a 2-D batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh; its cycle is rfsgpu_batch_fastslam_mh_cycle_async)";
    case STEPS_FASTSLAM: return "a 2-D batch of FastSLAM filters (rfsgpu_create_batch, then rfsgpu_batch_set_fastslam_config; its cycle is rfsgpu_batch_fastslam_cycle_async)";
    case STEPS_RBPHD: return "a 2-D batch of RB-PHD filters (rfsgpu_create_batch; its cycle is rfsgpu_batch_cycle_async)";
    default: break;
  }
  return "a 2-D batch whose kind is not decided yet (rfsgpu_create_batch; rfsgpu_batch_cycle_async makes it a batch of RB-PHD filters, rfsgpu_batch_set_fastslam_config or "
         "rfsgpu_batch_fastslam_cycle_async a batch of FastSLAM filters)";
}

#define HIPCHK(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      f->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
      return RFSGPU_ERR_HIP;                                                               \
    }                                                                                      \
  } while (0)

// (a handle whose particle count is still on the device -- rfsgpu_fastslam_cycle_async -- takes it over first: every entry point
//  that reads or sizes by N starts here)
static int mhc_resolve(rfsgpu_filter *f);
static inline bool rc_only_pending(const rfsgpu_filter *f) { return f->rcPending && !f->mhcStashedRc; }   // (never pending next to a FastSLAM cycle or rfsgpu_resample_async)
#define CHECK_HANDLE(f)                                                       \
  if (!(f)) return RFSGPU_ERR_INVALID;                                        \
  if ((f)->mhcPending || (f)->mhcStashedRc || (f)->mhbPending || (f)->rsPending || (f)->rcPending) { \
    const int rcMhc_ = mhc_resolve(f);                                        \
    if (rcMhc_ != RFSGPU_OK) return rcMhc_;                                   \
  }
// ... the stream-ordered calls that neither read the ids nor care whether a resampling occurred start here: behind a pending
// rfsgpu_resample_async that keeps the particle count they enqueue without waiting for it (one that may shrink the set is resolved)
#define CHECK_HANDLE_ENQ(f)                                                   \
  if (!(f)) return RFSGPU_ERR_INVALID;                                        \
  if ((f)->mhcPending || (f)->mhcStashedRc || (f)->mhbPending || ((f)->rsPending && (f)->rsShrink) || (f)->rcPending) { \
    const int rcMhc_ = mhc_resolve(f);                                        \
    if (rcMhc_ != RFSGPU_OK) return rcMhc_;                                   \
  }
// ... and the setters that neither read nor size by N (their values travel by value with each launch) start here: a host that
// pushes its configuration before every cycle does not wait for the cycles in flight
#define CHECK_HANDLE_HOST(f) \
  if (!(f)) return RFSGPU_ERR_INVALID;
// ... and the motion and static-step calls start here: behind pending device cycles of a FastSLAM handle (and nothing else pending)
// they do not take the count over -- `behind` comes back true and the call launches its LiveCount form at the handle's capacity,
// which reads the count and the overflow word of the cycle block on the device.  Otherwise as CHECK_HANDLE_ENQ.
#define CHECK_HANDLE_BEHIND_CYCLE(f, behind)                                  \
  if (!(f)) return RFSGPU_ERR_INVALID;                                        \
  const bool behind = (f)->mhcPending && !(f)->mhcStashedRc && !(f)->mhbPending && !(f)->rsPending; \
  if (!behind && !rc_only_pending(f)) { CHECK_HANDLE_ENQ(f); }
// ... and the calls that go behind pending rfsgpu_rbphd_cycle_async cycles start here: the particle count is the host's on that route, so
// what neither reads the ids nor resampleOccured_ (or reads them on the device: rfsgpu_predict_map_async(f, 1)) enqueues as it is.
// Otherwise as CHECK_HANDLE.
#define CHECK_HANDLE_BEHIND_RBPHD(f)                                          \
  if (!(f)) return RFSGPU_ERR_INVALID;                                        \
  if (!rc_only_pending(f)) { CHECK_HANDLE(f); }

static int fail(rfsgpu_filter *f, int code, const char *msg) {
  f->err = msg;
  return code;
}
// "<what> is not available on <what this handle is>: <why>", for the calls that a kind of batch does not have
static int refuse_on_kind(rfsgpu_filter *f, const char *what, const char *why) {
  f->err = std::string(what) + " is not available on " + handle_kind_text(f) + ": " + why;
  return RFSGPU_ERR_UNSUPPORTED;
}
// "<who>: <what the call serves>, not <what this handle is>[<hint>]", for the calls that belong to one kind of handle
static int refuse_not(rfsgpu_filter *f, const char *head, const char *hint = "") {
  f->err = std::string(head) + ", not " + handle_kind_text(f) + hint;
  return RFSGPU_ERR_UNSUPPORTED;
}
static const char ON_BATCH[] = "a filter batch takes the rfsgpu_batch_* calls";
static const char ON_MH_BATCH[] = "the call assumes that every filter fills its block";     // (!batch_fills_blocks)
static const char ON_VP_BATCH[] = "a batch of Victoria Park filters is configured, stepped and resampled by the rfsgpu_batch_vp_* calls";

// The next block of a pinned ring (created on first use): waits until whatever was enqueued from it one turn of the ring ago is done.
// The caller writes into *h, enqueues its host-to-device copies (or the kernels that read the block in place) on the stream and
// records R.ev[*k_out] behind the last of them.
template <class T>
static int ring_acquire(rfsgpu_filter *f, PinnedRing &R, T **h, int *k_out) {
  const int k = R.next;
  R.next = (k + 1) & (R.depth - 1);
  const bool fresh = !R.h[k] || !R.ev[k];               // (either creation may have failed on an earlier call: each is retried on its own)
  if (!R.h[k]) HIPCHK(hipHostMalloc(&R.h[k], R.bytes));
  if (!R.ev[k]) HIPCHK(hipEventCreateWithFlags(&R.ev[k], hipEventDisableTiming));
  if (fresh) HIPCHK(hipStreamSynchronize(f->stream));   // nothing recorded on this block's event yet
  else HIPCHK(hipEventSynchronize(R.ev[k]));            // what this block fed one turn of the ring ago
  *h = reinterpret_cast<T *>(R.h[k]);
  *k_out = k;
  return RFSGPU_OK;
}
static int push_scan(rfsgpu_filter *f, double *hs, const double *scan, int n_scan);
// The pose covariance that goes with a push of poses, through hc (pinned, inside the block the caller holds): one shared [9]
// (cov_stride 0), one per particle [N][9] (cov_stride 9) or none -- then B.poseCov[0 .. 9) gets zeros, once (poseCovZero).  inPacked:
// the per-particle covariances ride in the step kernel's packed block (its pull form) and no copy command is issued.  The stride is
// the caller's to set: a single handle writes f->P.poseCovStride, a batch goes through batch_handle_wide and bParamsDirty.
static int push_pose_cov(rfsgpu_filter *f, double *hc, const double *cov, int cov_stride, bool inPacked = false) {
  if (cov) {
    if (!inPacked) {
      const size_t n = cov_stride == 9 ? (size_t)f->N * 9 : 9;
      memcpy(hc, cov, n * sizeof(double));
      HIPCHK(hipMemcpyAsync(f->B.poseCov, hc, n * sizeof(double), hipMemcpyHostToDevice, f->stream));
    }
    f->poseCovZero = false;
  } else if (!f->poseCovZero) {   // (the shared all-zero covariance is written once, not per call)
    memset(hc, 0, 9 * sizeof(double));
    HIPCHK(hipMemcpyAsync(f->B.poseCov, hc, 9 * sizeof(double), hipMemcpyHostToDevice, f->stream));
    f->poseCovZero = true;
  }
  return RFSGPU_OK;
}
// Poses by copy command through the staging block h: x [N][3] to dst, the covariance behind it (push_pose_cov)
static int push_poses(rfsgpu_filter *f, double *h, double *dst, const double *x, const double *cov, int cov_stride) {
  memcpy(h, x, (size_t)f->N * 3 * sizeof(double));
  HIPCHK(hipMemcpyAsync(dst, h, (size_t)f->N * 3 * sizeof(double), hipMemcpyHostToDevice, f->stream));
  return push_pose_cov(f, h + (size_t)f->Ncap * 3, cov, cov_stride);
}

// rfsgpu_partition_likelihoods: one wavefront per table.  dims[4 k ..]: nE, nZ, the table's offset in L, its offset in pd.  The LDS view is
// carved for the largest table (64 x 64, no mixture); the table keeps its own row stride nZ, as in the weighting kernels.
__global__ __launch_bounds__(64) void partition_tables_kernel(const double *L, const double *pd, const int *dims, double clutter, MurtyQueue Q, int *err,
                                                              int exactMode, double *weight) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int nE = dims[4 * k], nZ = dims[4 * k + 1];
  const double *Lk = L + dims[4 * k + 2], *pdk = pd + dims[4 * k + 3];
  WeightLDS s;
  carve_weight_lds(smem_raw, 0, RFSGPU_MAX_EVAL, RFSGPU_MAX_Z, s);
  for (int idx = lane; idx < nE * nZ; idx += 64) s.L[idx] = Lk[idx];
  if (lane < nE) {
    const double p = pdk[lane];
    s.evPd[lane] = p;
    s.evLog1mPd[lane] = log(1 - p);
  }
  wave_sync();
  const double l = rfs_partitions_wave(s, nE, nZ, clutter, lane, k, Q, err, exactMode);
  if (lane == 0) weight[k] = l;
}

static void batch_set_all(rfsgpu_filter *f);
static std::string batch_error_note(rfsgpu_filter *f, int e);
// The Params of one filter from its configuration: a function of its arguments.  The fields it does not set (poseCovStride,
// exactPartitions, ...) stay what P holds.  Q: the landmark process noise, D x D row-major.
static void rebuild_params(Params &P, const rfsgpu_filter_config &cfg, const rfsgpu_rngbrg_config &rb, const rfsgpu_kf_config &kf, const double *Qlm,
                           const rfsgpu_vp_config &vp, double vpClutter, int D, bool denseIntensity, bool gateIndex) {
  P.denseIntensity = denseIntensity ? 1 : 0;
  P.gateIndex = gateIndex ? 1 : 0;
  for (int k = 0; k < 4; k++) P.R[k] = rb.R[k];
  P.Pd = rb.probabilityOfDetection;
  P.clutter = rb.uniformClutterIntensity;
  P.rmax = rb.rangeLimMax;
  P.rmin = rb.rangeLimMin;
  P.rbuf = rb.rangeLimBuffer;
  P.rmaxIn = P.rmax - P.rbuf; P.rmaxOut = P.rmax + P.rbuf; P.rminIn = P.rmin + P.rbuf; P.rminOut = P.rmin - P.rbuf;
  P.kfRange = kf.rangeInnovationThreshold;
  P.kfBearing = kf.bearingInnovationThreshold;
  P.birthW = cfg.birthGaussianWeight;
  P.newGaussMd2 = cfg.newGaussianCreateInnovMDThreshold * cfg.newGaussianCreateInnovMDThreshold;
  P.evalMinW = cfg.importanceWeightingEvalPointGuassianWeight;
  P.weightingMd2 = cfg.importanceWeightingMeasurementLikelihoodMDThreshold * cfg.importanceWeightingMeasurementLikelihoodMDThreshold;
  P.mergeT2 = cfg.gaussianMergingThreshold * cfg.gaussianMergingThreshold;
  P.mergeInfl = cfg.gaussianMergingCovarianceInflationFactor;
  P.pruneT = cfg.gaussianPruningThreshold;
  if (D == 2) {
    P.Qlm[0] = Qlm[0];
    P.Qlm[1] = Qlm[1];
    P.Qlm[2] = Qlm[3];
    P.twoPiPowD = pow(2 * acos(-1), 2);
  } else {
    P.Qlm6[0] = Qlm[0]; P.Qlm6[1] = Qlm[1]; P.Qlm6[2] = Qlm[2];
    P.Qlm6[3] = Qlm[4]; P.Qlm6[4] = Qlm[5]; P.Qlm6[5] = Qlm[8];
    P.twoPiPowD = pow(2 * acos(-1), 3);
    for (int k = 0; k < 9; k++) P.R9[k] = vp.R[k];
    P.R[0] = vp.R[0]; P.R[1] = vp.R[1]; P.R[2] = vp.R[3]; P.R[3] = vp.R[4];  // 2x2 range-bearing block
    P.Slb = vp.Slb;
    for (int k = 0; k < RFSGPU_VP_MAX_PD; k++) P.PdTable[k] = vp.PdTable[k];
    P.nPd = vp.nPd;
    P.vpClutter = vpClutter;
    P.vpExpClutter = vp.expectedClutterNumber;
    P.rmax = vp.rangeLimMax; P.rmin = vp.rangeLimMin;
    P.bmax = vp.bearingLimitMax; P.bmin = vp.bearingLimitMin;
    P.bufferPd = vp.bufferZonePd;
  }
  P.birthCheckThr = cfg.birthGaussianMeasurementCheckThreshold;
  P.birthSupportD2 = cfg.birthGaussianMeasurementSupportDist * cfg.birthGaussianMeasurementSupportDist;
  P.evalCount = cfg.importanceWeightingEvalPointCount;
  P.useCluster = cfg.useClusterProcess ? 1 : 0;
  P.birthCountThr = cfg.birthGaussianMeasurementCountThreshold;
  P.birthCurThr = cfg.birthGaussianCurrentMeasurementCountThreshold;
}
// ... of a handle, from its own members
static void rebuild_params(rfsgpu_filter *f) {
  rebuild_params(f->P, f->cfg, f->rb, f->kf, f->Qlm, f->vp, f->vpClutter, f->D, f->denseIntensity, f->gateIndex);
}
// setLaserScan's clutter density, expectedClutterNumber over the scan's field-of-view area: the handle's and, on a batch of Victoria
// Park filters, every filter's from its own expectedClutterNumber as it is configured now (a later rfsgpu_batch_configure_vp leaves
// it until the next scan, as the handle's setter does).  One scan for the handle; a batch's densities travel in its Params table.
static void scan_clutter(rfsgpu_filter *f, const double *scan, int n) {
  const double area = scan_fov_area(scan, n);
  f->vpClutter = f->vp.expectedClutterNumber / area;
  if (!f->batch) return;
  for (int b = 0; b < f->nF; b++) f->bVpClutter[b] = f->bVp[b].expectedClutterNumber / area;
  f->bParamsDirty = true;
}

static int check_device_errors(rfsgpu_filter *f) {
  // one 4-byte D2H + stream sync per phase group
  HIPCHK(hipMemcpyAsync(f->hErr, f->B.err, sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  const int e = *f->hErr;
  if (e == 0) return RFSGPU_OK;
  HIPCHK(hipMemsetAsync(f->B.err, 0, sizeof(int), f->stream));
  // every flag that was raised goes into the message; the status code is the first one's
  std::string msg;
  int code = RFSGPU_OK;
  auto add = [&](int bit, int c, const char *m) {
    if (!(e & bit)) return;
    if (!msg.empty()) msg += "; ";
    msg += m;
    if (code == RFSGPU_OK) code = c;
  };
  add(ERRBIT_CAPACITY, RFSGPU_ERR_CAPACITY, "a particle's Gaussian mixture outgrew gm_capacity (raise it in rfsgpu_create)");
  add(ERRBIT_MURTY, RFSGPU_ERR_UNSUPPORTED, "Murty job queue overflow, a partition larger than MURTY_MAXN, or a FastSLAM association component beyond the in-kernel solver");
  add(ERRBIT_MURTY_POOL, RFSGPU_ERR_UNSUPPORTED, "a Murty-200 partition's search outgrew the node pool (MURTY_MAX_NODES = 1 + 200 expansions x 32 children; a partition with more than 32 rows can need more)");
  add(ERRBIT_EVALPTS, RFSGPU_ERR_UNSUPPORTED, "more than RFSGPU_MAX_EVAL evaluation points requested");
  add(ERRBIT_BIRTHLIST, RFSGPU_ERR_UNSUPPORTED, "a particle's birth-candidate / landmark-candidate list outgrew RFSGPU_MAX_CANDIDATES");
  add(ERRBIT_COLLECTIVE, RFSGPU_ERR_UNSUPPORTED, "collective hand-over timed out: the sequence number of the weight all-reduce was not published within 0.5 s (rfsgpu_step_async_trailing / rfsgpu_collective_gate / _publish)");
  add(ERRBIT_SCAN, RFSGPU_ERR_CAPACITY, "a sensed scan outgrew its sensor's max_nz and was cut to its first max_nz entries (rfsgpu_batch_set_sensor)");
  if (code != RFSGPU_OK && f->batch) msg += batch_error_note(f, e);
  if (code != RFSGPU_OK) { f->err = msg; return code; }
  return fail(f, RFSGPU_ERR_HIP, "unknown device error flag");
}

static void accumulate(hipEvent_t a, hipEvent_t b, long long &acc, long long *last) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) == hipSuccess) {
    long long ns = (long long)(ms * 1e6);
    acc += ns;
    if (last) *last = ns;
  }
}

extern "C" {

int rfsgpu_abi_version(void) { return RFSGPU_ABI_VERSION; }

void rfsgpu_default_filter_config(rfsgpu_filter_config *c) {  // RBPHDFilter.hpp:370-382
  memset(c, 0, sizeof(*c));
  c->birthGaussianWeight = 0.25;
  c->birthGaussianMeasurementCountThreshold = 1;
  c->birthGaussianMeasurementCheckThreshold = 1;
  c->birthGaussianMeasurementSupportDist = 1;
  c->birthGaussianCurrentMeasurementCountThreshold = 1;
  c->gaussianMergingThreshold = 0.5;
  c->gaussianMergingCovarianceInflationFactor = 1.5;
  c->gaussianPruningThreshold = 0.2;
  c->importanceWeightingEvalPointCount = 8;
  c->importanceWeightingEvalPointGuassianWeight = 0;
  c->importanceWeightingMeasurementLikelihoodMDThreshold = 3.0;
  c->newGaussianCreateInnovMDThreshold = 0.2;
  c->minUpdatesBeforeResample = 1;
  c->minMeasurementsBeforeResample = 1;
  c->useClusterProcess = 0;
}

int rfsgpu_create(rfsgpu_filter **out, int model, int n_particles, int device_id, int gm_capacity) {
  return rfsgpu_create_ex(out, model, n_particles, device_id, gm_capacity, n_particles);
}
int rfsgpu_create_ex(rfsgpu_filter **out, int model, int n_particles, int device_id, int gm_capacity, int max_particles) {
  if (max_particles < n_particles) return RFSGPU_ERR_INVALID;
  if (!out || n_particles <= 0 || (model != RFSGPU_MODEL_RNGBRG_2D && model != RFSGPU_MODEL_VICTORIAPARK_3D) || gm_capacity <= 0) return RFSGPU_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return RFSGPU_ERR_NO_DEVICE;
  rfsgpu_filter *f = new rfsgpu_filter();
  f->device = device_id;
  f->N = n_particles;
  f->Ncap = max_particles;
  f->stage.bytes = ((size_t)f->Ncap * 22 + RFSGPU_VP_MAX_SCAN) * sizeof(double);   // poses | pose covariances | weights (or the 13-per-particle packed form) | covariances of the packed form's copy path | laser scan
  f->model = model;
  f->D = (model == RFSGPU_MODEL_VICTORIAPARK_3D) ? 3 : 2;
  f->cap = ((gm_capacity + 63) / 64) * 64;
  rfsgpu_default_fastslam_config(&f->fs);
  f->fs.nParticlesMax = 3 * n_particles;
  { const char *e = getenv("RFSGPU_FUSED_STEP"); if (e && e[0] == '0') f->fuseSteps = false; }
  { const char *e = getenv("RFSGPU_IO_PULL"); if (e && e[0] == '0') f->ioPull = false; }
  { const char *e = getenv("RFSGPU_DENSE_INTENSITY"); if (e && e[0] == '1') f->denseIntensity = true; }
  { const char *e = getenv("RFSGPU_GATE_INDEX"); if (e && e[0] == '0') f->gateIndex = false; }
  { const char *e = getenv("RFSGPU_STEP_WPP"); if (e) f->stepWppOverride = atoi(e); }
  { const char *e = getenv("RFSGPU_UPDMAP_WPP"); if (e) f->updMapWppOverride = atoi(e); }
  { const char *e = getenv("RFSGPU_BIRTH_INHERITANCE"); if (e && !strcmp(e, "eager")) f->inheritMode = RFSGPU_INHERIT_EAGER; }   // (initial mode; rfsgpu_set_birth_inheritance)
  { const char *e = getenv("RFSGPU_MERGE_GRID"); if (e) f->mergeGridOverride = atoi(e); }
  if (f->cap > 2048) { delete f; return RFSGPU_ERR_INVALID; }
  auto bail = [&](int code) { rfsgpu_destroy(f); return code; };
  if (hipSetDevice(device_id) != hipSuccess) return bail(RFSGPU_ERR_NO_DEVICE);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return bail(RFSGPU_ERR_NO_DEVICE);
  f->maxLds = (int)prop.sharedMemPerBlock;
  f->nCU = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (hipStreamCreateWithFlags(&f->ownStream, hipStreamNonBlocking) != hipSuccess) return bail(RFSGPU_ERR_HIP);
  f->stream = f->ownStream;
  for (int k = 0; k < EV_COUNT; k++)
    if (hipEventCreate(&f->ev[k]) != hipSuccess) return bail(RFSGPU_ERR_HIP);
  Buffers &B = f->B;
  B.N = f->N;
  B.cap = f->cap;
  B.npl = (f->D == 3) ? (int)P3_COUNT : (int)PL_COUNT;
  const size_t slabBytes = (size_t)f->Ncap * B.npl * f->cap * sizeof(double);
  bool ok = true;
  ok &= hipMalloc(&B.slab[0], slabBytes) == hipSuccess;
  ok &= hipMalloc(&B.slab[1], slabBytes) == hipSuccess;
  ok &= hipMalloc(&B.count, f->Ncap * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&B.pose, (size_t)f->Ncap * 3 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&B.poseCov, (size_t)f->Ncap * 9 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->poseAlt, (size_t)f->Ncap * 3 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->dCollSeq, 4 * sizeof(int)) == hipSuccess;      // + [2] probe word, [3] probe verdict (rfsgpu_collective_probe)
  if (ok) ok &= hipMemset(f->dCollSeq, 0, 4 * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&B.weight, f->Ncap * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&B.unusedMask, f->Ncap * sizeof(unsigned long long)) == hipSuccess;
  ok &= hipMalloc(&B.nInFov, f->Ncap * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&B.err, sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&B.Z, RFSGPU_MAX_Z * 3 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&B.scan, RFSGPU_VP_MAX_SCAN * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&B.candMean, (size_t)f->Ncap * RFSGPU_MAX_CANDIDATES * 3 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&B.candCov, (size_t)f->Ncap * RFSGPU_MAX_CANDIDATES * 6 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&B.candSup, (size_t)f->Ncap * RFSGPU_MAX_CANDIDATES * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&B.candChk, (size_t)f->Ncap * RFSGPU_MAX_CANDIDATES * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&B.candCount, (size_t)f->Ncap * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->ownSums, 2 * sizeof(double)) == hipSuccess;
  f->dSums = f->ownSums;
  ok &= hipMalloc(&f->dSrcSlot, f->Ncap * sizeof(int)) == hipSuccess;
  ok &= hipHostMalloc(&f->hErr, sizeof(int)) == hipSuccess;
  ok &= hipHostMalloc(&f->hJobCount, sizeof(int)) == hipSuccess;
  if (ok) *f->hJobCount = 0;   // set by the post kernel once a step has queued Murty jobs (murty_launch)
  ok &= hipHostMalloc(&f->hSums, 2 * sizeof(double)) == hipSuccess;
  for (int k = 0; k < RFSGPU_ASYNC_RING; k++)
    for (int e = 0; e < 5; e++) ok &= hipEventCreate(&f->ring[k][e]) == hipSuccess;
  if (!ok) return bail(RFSGPU_ERR_HIP);
  if (murty_alloc(f->Q, f->MS, f->Ncap) != 0) return bail(RFSGPU_ERR_HIP);
  hipMemsetAsync(B.slab[0], 0, slabBytes, f->stream);
  hipMemsetAsync(B.slab[1], 0, slabBytes, f->stream);
  hipMemsetAsync(B.count, 0, f->Ncap * sizeof(int), f->stream);
  hipMemsetAsync(B.pose, 0, (size_t)f->Ncap * 3 * sizeof(double), f->stream);
  hipMemsetAsync(B.poseCov, 0, (size_t)f->Ncap * 9 * sizeof(double), f->stream);
  hipMemsetAsync(B.unusedMask, 0, f->Ncap * sizeof(unsigned long long), f->stream);
  hipMemsetAsync(B.nInFov, 0, f->Ncap * sizeof(int), f->stream);
  hipMemsetAsync(B.err, 0, sizeof(int), f->stream);
  hipMemsetAsync(B.Z, 0, RFSGPU_MAX_Z * 3 * sizeof(double), f->stream);
  hipMemsetAsync(B.scan, 0, RFSGPU_VP_MAX_SCAN * sizeof(double), f->stream);
  hipMemsetAsync(B.candCount, 0, (size_t)f->Ncap * sizeof(int), f->stream);
  B.nScan = 0;
  set_weights_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(B.weight, f->N, 1.0);
  if (hipStreamSynchronize(f->stream) != hipSuccess) return bail(RFSGPU_ERR_HIP);
  rfsgpu_default_filter_config(&f->cfg);
  memset(&f->rb, 0, sizeof(f->rb));  // MeasurementModel_RngBrg defaults, src/MeasurementModel_RngBrg.cpp:35-43
  f->rb.probabilityOfDetection = 0.95;
  f->rb.uniformClutterIntensity = 0.1;
  f->rb.rangeLimMax = 5;
  f->rb.rangeLimMin = 0.3;
  f->rb.rangeLimBuffer = 0.25;
  memset(&f->vp, 0, sizeof(f->vp));
  f->kf.rangeInnovationThreshold = -1;
  f->kf.bearingInnovationThreshold = -1;
  f->P.poseCovStride = 0;
  rebuild_params(f);
  *out = f;
  return RFSGPU_OK;
}

void rfsgpu_destroy(rfsgpu_filter *f) {
  if (!f) return;
  hipSetDevice(f->device);
  if (f->stream) hipStreamSynchronize(f->stream);
  if (f->ownStream) hipStreamSynchronize(f->ownStream);
  Buffers &B = f->B;
  hipFree(f->snapSlab); hipFree(f->snapWeight); hipFree(f->snapCount); hipFree(f->snapFov); hipFree(f->snapUnused);
  for (auto &r : f->stateRing) { hipFree(r.slab); hipFree(r.weight); hipFree(r.count); hipFree(r.fov); hipFree(r.unused); }
  hipFree(B.slab[0]); hipFree(B.slab[1]); hipFree(B.count); hipFree(B.pose); hipFree(f->poseAlt); hipFree(f->dCollSeq); if (f->vpCost) hipFree(f->vpCost); if (f->vpOrder) hipFree(f->vpOrder); hipFree(B.poseCov); hipFree(B.weight);
  hipFree(B.unusedMask); hipFree(B.nInFov); hipFree(B.err); hipFree(B.Z); hipFree(f->ownSums); hipFree(f->dSrcSlot); hipFree(f->rsBlock); if (f->hRsBlock) hipHostFree(f->hRsBlock); if (f->dRowSlots) hipFree(f->dRowSlots); if (f->fsArena) hipFree(f->fsArena); if (f->mhArena) hipFree(f->mhArena); if (f->mhInts) hipFree(f->mhInts); if (f->mhcBlock) hipFree(f->mhcBlock); if (f->mhcInts) hipFree(f->mhcInts); if (f->hMhcBlock) hipHostFree(f->hMhcBlock);
  if (f->dInhParent) hipFree(f->dInhParent);
  if (f->dInhLevel) hipFree(f->dInhLevel);
  hipFree(f->inhTmp.unused); hipFree(f->inhTmp.count); hipFree(f->inhTmp.sup); hipFree(f->inhTmp.chk); hipFree(f->inhTmp.mean); hipFree(f->inhTmp.cov);  // (hipFree(nullptr) is a no-op)
  hipFree(B.scan); hipFree(B.candMean); hipFree(B.candCov); hipFree(B.candSup); hipFree(B.candChk); hipFree(B.candCount);
  murty_free(f->Q, f->MS);
  hipFree(f->dBFilt); hipFree(f->dBParams); hipFree(f->dBZ); hipFree(f->dBZPrev); hipFree(f->dBSums); hipFree(f->dBErrFilter); hipFree(f->dBMaskTmp); hipFree(f->dBInhSrc);
  hipFree(f->dFsFilt); hipFree(f->dFsTmpl); hipFree(f->dFsLastNZ); if (f->hFsLastNZ) hipHostFree(f->hFsLastNZ);
  hipFree(f->dMhFilt); hipFree(f->mhbBlock); if (f->hMhbBlock) hipHostFree(f->hMhbBlock);
  hipFree(f->dBMotion); hipFree(f->dBPropIn); hipFree(f->dBResIn); hipFree(f->BL.counters); hipFree(f->BL.nResamples); hipFree(f->BL.resampled);
  hipFree(f->BL.fired); hipFree(f->BL.nEff); hipFree(f->BL.plan); hipFree(f->BL.pid); hipFree(f->BL.ppid);
  hipFree(f->dBVpMotion); hipFree(f->dBVpRun); hipFree(f->dBVpWalk);
  hipFree(f->dBSensor); hipFree(f->dBSensorLm); hipFree(f->dBSensorPose); hipFree(f->dBSensorCaps); hipFree(f->dBSensorPrev); hipFree(f->dBSensorErrFilter);
  hipFree(f->dTruthCfg); hipFree(f->dTruthProp); hipFree(f->dTruthGt); hipFree(f->dTruthTgt); hipFree(f->dTruthLm); hipFree(f->dTruthSeen); hipFree(f->dTruthCounts);
  hipFree(f->dGtXY); hipFree(f->dGtSeen); hipFree(f->dGtN); hipFree(f->dErrLog); hipFree(f->dErrRow);
  hipFree(f->dEstHdr); hipFree(f->dEstGauss); hipFree(f->dEstPart);
  if (f->hErr) hipHostFree(f->hErr);
  if (f->hJobCount) hipHostFree(f->hJobCount);
  if (f->hSums) hipHostFree(f->hSums);
  if (f->hWeights) hipHostFree(f->hWeights);
  if (f->hOutW) hipHostFree(f->hOutW);
  for (PinnedRing *R : {&f->stage, &f->bStage, &f->bLoop})
    for (int k = 0; k < 8; k++) { if (R->h[k]) hipHostFree(R->h[k]); if (R->ev[k]) hipEventDestroy(R->ev[k]); }
  for (int k = 0; k < RFSGPU_ASYNC_RING; k++)
    for (int e = 0; e < 5; e++) if (f->ring[k][e]) hipEventDestroy(f->ring[k][e]);
  for (int k = 0; k < EV_COUNT; k++) if (f->ev[k]) hipEventDestroy(f->ev[k]);
  if (f->ownStream) hipStreamDestroy(f->ownStream);
  delete f;
}

const char *rfsgpu_last_error(const rfsgpu_filter *f) { return f ? f->err.c_str() : "null handle"; }

int rfsgpu_set_filter_config(rfsgpu_filter *f, const rfsgpu_filter_config *c) {
  CHECK_HANDLE_HOST(f);
  if (!c) return RFSGPU_ERR_INVALID;
  f->cfg = *c;
  rebuild_params(f);
  if (f->batch) batch_set_all(f);
  return RFSGPU_OK;
}
int rfsgpu_set_partition_mode(rfsgpu_filter *f, int mode) {
  CHECK_HANDLE(f);
  if (mode != RFSGPU_PARTITION_MURTY200 && mode != RFSGPU_PARTITION_EXACT) return fail(f, RFSGPU_ERR_INVALID, "unknown partition mode");
  f->P.exactPartitions = mode == RFSGPU_PARTITION_EXACT ? 1 : 0;
  return RFSGPU_OK;
}
// [test] The Murty-200 partition sums of given extended tables by the step's own post kernel (murty_jobs_kernel): what
// rfsMeasurementLikelihood's loop (include/RBPHDFilter.hpp:942-959) leaves in partition_likelihood for each table.  The tables
// go into the handle's job queue exactly as the weighting phase writes them (n x n row-major, n = nR + nC, slot k), the kernel
// runs once, the results come back; the particle weights are put back afterwards (the kernel multiplies the factors into them).
int rfsgpu_murty_partition_sums(rfsgpu_filter *f, const double *mats, const int *nR, const int *nC, int n_jobs, double *sums_out) {
  CHECK_HANDLE(f);
  if (!mats || !nR || !nC || !sums_out || n_jobs < 1 || n_jobs > f->Q.maxJobs) return fail(f, RFSGPU_ERR_INVALID, "murty_partition_sums: bad arguments");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  std::vector<double> w((size_t)f->N);
  HIPCHK(hipMemcpy(w.data(), f->B.weight, (size_t)f->N * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<MurtyJob> jobs((size_t)n_jobs);
  size_t off = 0;
  for (int k = 0; k < n_jobs; k++) {
    const int n = nR[k] + nC[k];
    if (nR[k] < 0 || nC[k] < 0 || n < 1 || n > MURTY_N) return fail(f, RFSGPU_ERR_INVALID, "murty_partition_sums: extended dimension out of range");
    jobs[k].particle = k % f->N; jobs[k].nR = nR[k]; jobs[k].nC = nC[k]; jobs[k].slot = k / f->N;
    HIPCHK(hipMemcpy(f->Q.mats + (size_t)k * MURTY_MAXN * MURTY_MAXN, mats + off, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
    off += (size_t)n * n;
  }
  HIPCHK(hipMemcpy(f->Q.jobs, jobs.data(), (size_t)n_jobs * sizeof(MurtyJob), hipMemcpyHostToDevice));
  const int cnt[2] = {n_jobs, 0};
  HIPCHK(hipMemcpy(f->Q.count, cnt, sizeof(cnt), hipMemcpyHostToDevice));
  if (murty_launch(f->Q, f->MS, f->B, f->stream, nullptr, 0, nullptr, 0, f->hJobCount) != 0) return fail(f, RFSGPU_ERR_HIP, "murty launch failed");
  HIPCHK(hipMemcpyAsync(sums_out, f->Q.results, (size_t)n_jobs * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.weight, w.data(), (size_t)f->N * sizeof(double), hipMemcpyHostToDevice, f->stream));
  return check_device_errors(f);
}
// [test] The weighting phase's partition stage (weighting.h steps 5-6, rfs_partitions_wave) on given likelihood tables: table k plays
// particle k.  One wavefront per table lays the table, the evaluation points' Pd and log(1 - Pd) into the LDS view the weighting
// kernels use and calls the production device function with the handle's partition mode and Murty queue; the handle's post kernel
// then multiplies the queued Murty-200 factors in, as in a step.  Nothing of the partition logic is restated here.
int rfsgpu_partition_likelihoods(rfsgpu_filter *f, const double *L, const double *pd, const int *nE, const int *nZ, int n_tables, double clutter,
                                 double *out) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_partition_likelihoods", ON_BATCH);
  if (!L || !pd || !nE || !nZ || !out || n_tables < 1 || n_tables > f->N) return fail(f, RFSGPU_ERR_INVALID, "partition_likelihoods: bad arguments");
  std::vector<int> dims((size_t)n_tables * 4);
  size_t offL = 0, offPd = 0;
  for (int k = 0; k < n_tables; k++) {
    if (nE[k] < 0 || nE[k] > RFSGPU_MAX_EVAL || nZ[k] < 0 || nZ[k] > RFSGPU_MAX_Z)
      return fail(f, RFSGPU_ERR_INVALID, "partition_likelihoods: table dimensions out of range (0 .. 64 evaluation points and measurements)");
    dims[4 * k] = nE[k]; dims[4 * k + 1] = nZ[k]; dims[4 * k + 2] = (int)offL; dims[4 * k + 3] = (int)offPd;
    offL += (size_t)nE[k] * nZ[k];
    offPd += (size_t)nE[k];
  }
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  std::vector<double> w((size_t)f->N), got((size_t)n_tables);
  HIPCHK(hipMemcpy(w.data(), f->B.weight, (size_t)f->N * sizeof(double), hipMemcpyDeviceToHost));
  struct Tmp { void *p = nullptr; ~Tmp() { if (p) hipFree(p); } } dL, dPd, dDims;
  HIPCHK(hipMalloc(&dL.p, (offL + 1) * sizeof(double)));
  HIPCHK(hipMalloc(&dPd.p, (offPd + 1) * sizeof(double)));
  HIPCHK(hipMalloc(&dDims.p, dims.size() * sizeof(int)));
  if (offL) HIPCHK(hipMemcpy(dL.p, L, offL * sizeof(double), hipMemcpyHostToDevice));
  if (offPd) HIPCHK(hipMemcpy(dPd.p, pd, offPd * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dDims.p, dims.data(), dims.size() * sizeof(int), hipMemcpyHostToDevice));
  const int cnt[2] = {0, 0};
  HIPCHK(hipMemcpy(f->Q.count, cnt, sizeof(cnt), hipMemcpyHostToDevice));
  const size_t lds = weight_lds_bytes_per_wave(0, RFSGPU_MAX_EVAL, RFSGPU_MAX_Z);
  partition_tables_kernel<<<n_tables, 64, lds, f->stream>>>((const double *)dL.p, (const double *)dPd.p, (const int *)dDims.p, clutter, f->Q, f->B.err,
                                                            f->P.exactPartitions, f->B.weight);
  // from here on the weights are overwritten: whatever fails, they are put back before the call returns
  hipError_t he = hipGetLastError();
  const bool launched = he == hipSuccess && murty_launch(f->Q, f->MS, f->B, f->stream, nullptr, 0, nullptr, 0, f->hJobCount) == 0;
  if (launched) he = hipMemcpyAsync(got.data(), f->B.weight, (size_t)n_tables * sizeof(double), hipMemcpyDeviceToHost, f->stream);
  const hipError_t hr = hipMemcpyAsync(f->B.weight, w.data(), (size_t)f->N * sizeof(double), hipMemcpyHostToDevice, f->stream);
  if (he != hipSuccess || hr != hipSuccess) {
    hipStreamSynchronize(f->stream);
    f->err = std::string("partition_likelihoods: ") + hipGetErrorString(he != hipSuccess ? he : hr);
    return RFSGPU_ERR_HIP;
  }
  if (!launched) { hipStreamSynchronize(f->stream); return fail(f, RFSGPU_ERR_HIP, "murty launch failed"); }
  const int rc = check_device_errors(f);   // (synchronises)
  if (rc != RFSGPU_OK) return rc;          // a refused table: no number comes back
  for (int k = 0; k < n_tables; k++) out[k] = got[k];
  return RFSGPU_OK;
}
int rfsgpu_get_partition_mode(const rfsgpu_filter *f) { return f ? (f->P.exactPartitions ? RFSGPU_PARTITION_EXACT : RFSGPU_PARTITION_MURTY200) : -1; }
int rfsgpu_get_filter_config(const rfsgpu_filter *f, rfsgpu_filter_config *c) {
  if (!f || !c) return RFSGPU_ERR_INVALID;
  *c = f->cfg;
  return RFSGPU_OK;
}
int rfsgpu_set_model_rngbrg(rfsgpu_filter *f, const rfsgpu_rngbrg_config *c) {
  CHECK_HANDLE(f);
  if (!c) return RFSGPU_ERR_INVALID;
  if (f->model != RFSGPU_MODEL_RNGBRG_2D) return fail(f, RFSGPU_ERR_INVALID, "set_model_rngbrg on a handle created for another model");
  f->rb = *c;
  rebuild_params(f);
  if (f->batch) batch_set_all(f);
  return RFSGPU_OK;
}
int rfsgpu_set_model_victoriapark(rfsgpu_filter *f, const rfsgpu_vp_config *c) {
  CHECK_HANDLE(f);
  if (f->batch && !batch_is_vp(f)) return refuse_on_kind(f, "the Victoria Park model", ON_BATCH);
  if (!c) return RFSGPU_ERR_INVALID;
  if (f->model != RFSGPU_MODEL_VICTORIAPARK_3D) return fail(f, RFSGPU_ERR_INVALID, "set_model_victoriapark on a handle created for another model");
  if (c->nPd < 1 || c->nPd > RFSGPU_VP_MAX_PD) return fail(f, RFSGPU_ERR_INVALID, "Pd table size out of range");
  f->vp = *c;
  rebuild_params(f);
  if (f->batch) {     // (a whole-handle setter sets every filter, as on a 2-D batch; the densities stay until the next scan, as on a handle)
    for (int b = 0; b < f->nF; b++) f->bVp[b] = *c;
    f->bParamsDirty = true;
  }
  return RFSGPU_OK;
}
// MeasurementModel_VictoriaPark::setLaserScan (src/MeasurementModel_VictoriaPark.cpp:267-281): the FoV area / clutter
// intensity are a 361-term host sum; the raw scan goes to the device for the occlusion-based Pd.
int rfsgpu_set_laser_scan(rfsgpu_filter *f, const double *scan, int n) {
  CHECK_HANDLE(f);
  if (f->batch && !batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_set_laser_scan", ON_BATCH);
  if (f->model != RFSGPU_MODEL_VICTORIAPARK_3D) return fail(f, RFSGPU_ERR_INVALID, "set_laser_scan needs the Victoria Park model");
  if (!scan || n < 2 || n > RFSGPU_VP_MAX_SCAN) return fail(f, RFSGPU_ERR_INVALID, "laser scan size out of range");
  scan_clutter(f, scan, n);
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(f->B.scan, scan, (size_t)n * sizeof(double), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  f->B.nScan = n;
  rebuild_params(f);
  return RFSGPU_OK;
}
int rfsgpu_vp_probe_pd(rfsgpu_filter *f, int slot, double *pd, int *close_to_limit, int max_n) {
  CHECK_HANDLE(f);
  if (f->model != RFSGPU_MODEL_VICTORIAPARK_3D || slot < 0 || slot >= f->N || !pd || !close_to_limit) return fail(f, RFSGPU_ERR_INVALID, "vp_probe_pd: bad arguments");
  if (f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "vp_probe_pd: rfsgpu_set_laser_scan first");
  hipSetDevice(f->device);
  const int n = std::min(max_n, f->cap);
  double *dPd = nullptr;
  int *dCl = nullptr;
  HIPCHK(hipMalloc(&dPd, (size_t)f->cap * sizeof(double)));
  if (hipMalloc(&dCl, (size_t)f->cap * sizeof(int)) != hipSuccess) { hipFree(dPd); return fail(f, RFSGPU_ERR_HIP, "vp_probe_pd: out of device memory"); }
  vp_probe_pd_kernel<<<1, 64, 0, f->stream>>>(f->B, f->P, f->cur, slot, dPd, dCl);
  hipError_t e1 = hipMemcpyAsync(pd, dPd, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream);
  hipError_t e2 = hipMemcpyAsync(close_to_limit, dCl, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, f->stream);
  hipError_t e3 = hipStreamSynchronize(f->stream);
  hipFree(dPd);
  hipFree(dCl);
  HIPCHK(e1); HIPCHK(e2); HIPCHK(e3);
  return RFSGPU_OK;
}
int rfsgpu_set_kf_config(rfsgpu_filter *f, const rfsgpu_kf_config *c) {
  CHECK_HANDLE(f);
  if (!c) return RFSGPU_ERR_INVALID;
  f->kf = *c;
  rebuild_params(f);
  if (f->batch) batch_set_all(f);
  return RFSGPU_OK;
}
int rfsgpu_set_lmk_process_noise(rfsgpu_filter *f, const double *Q) {
  CHECK_HANDLE_BEHIND_RBPHD(f);     // (the noise travels by value with each launch)
  if (!Q) return RFSGPU_ERR_INVALID;
  memcpy(f->Qlm, Q, (size_t)f->D * f->D * sizeof(double));
  rebuild_params(f);
  if (f->batch && f->D == 3) {      // a batch of Victoria Park filters: every filter's Q, and nothing else of its configuration
    for (int b = 0; b < f->nF; b++) memcpy(&f->bQ[(size_t)9 * b], Q, 9 * sizeof(double));
    f->bParamsDirty = true;
  } else if (f->batch) batch_set_all(f);
  return RFSGPU_OK;
}

// (r04: poses and weights go through the pinned staging ring of rfsgpu_set_step_inputs_async -- the caller's buffers are copied
//  before the call returns, the host-to-device copies are stream-ordered and nothing waits for the GPU.  The synchronous forms
//  these replaced -- a copy from pageable memory + a stream synchronisation each -- were 46 + 23 us of the 261 us that one
//  RBPHDFilter::update costs through the binding at configs[1], bench.py `boundary`.)
int rfsgpu_set_poses(rfsgpu_filter *f, const double *x, const double *cov, int cov_stride) {
  CHECK_HANDLE(f);
  if (!x || (cov_stride != 0 && cov_stride != 9)) return fail(f, RFSGPU_ERR_INVALID, "set_poses: bad arguments");
  return rfsgpu_set_step_inputs_async(f, x, cov, cov_stride, nullptr, 0);
}
int rfsgpu_get_poses(rfsgpu_filter *f, double *x) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(x, f->B.pose, (size_t)f->N * 3 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}
int rfsgpu_set_weights(rfsgpu_filter *f, const double *w) {
  CHECK_HANDLE(f);
  if (!w) return fail(f, RFSGPU_ERR_INVALID, "set_weights: null buffer");
  hipSetDevice(f->device);
  double *h = nullptr;
  int k = 0;
  { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
  memcpy(h, w, (size_t)f->N * sizeof(double));
  HIPCHK(hipMemcpyAsync(f->B.weight, h, (size_t)f->N * sizeof(double), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
  return RFSGPU_OK;
}
int rfsgpu_get_weights(rfsgpu_filter *f, double *w) {
  CHECK_HANDLE(f);
  if (!w) return fail(f, RFSGPU_ERR_INVALID, "get_weights: null buffer");
  hipSetDevice(f->device);
  if (!f->hWeights) HIPCHK(hipHostMalloc(&f->hWeights, (size_t)f->Ncap * sizeof(double)));   // pinned: a real DMA, no staging inside the runtime
  HIPCHK(hipMemcpyAsync(f->hWeights, f->B.weight, (size_t)f->N * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  memcpy(w, f->hWeights, (size_t)f->N * sizeof(double));
  return RFSGPU_OK;
}

int rfsgpu_gm_sizes(rfsgpu_filter *f, int *sizes) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  if (f->holes) {
    valid_count_kernel<<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, f->dSrcSlot);  // dSrcSlot doubles as int scratch
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sizes, f->dSrcSlot, (size_t)f->N * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  } else {
    HIPCHK(hipMemcpyAsync(sizes, f->B.count, (size_t)f->N * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  }
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

// Host staging of one particle's planes (valid entries only: holes carry w < 0 between merge and prune).
static int fetch_particle(rfsgpu_filter *f, int slot, std::vector<double> &planes, int &n) {
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(&n, f->B.count + slot, sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  planes.resize((size_t)f->B.npl * f->cap);
  HIPCHK(hipMemcpyAsync(planes.data(), f->B.slab[f->cur] + (size_t)slot * f->B.npl * f->cap, planes.size() * sizeof(double),
                        hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

// plane index of mean component d / of covariance entry (r,c) in the slab layout of the handle's model
static inline int mean_plane(const rfsgpu_filter *f, int d) { return 2 + d; }
static inline int cov_plane(const rfsgpu_filter *f, int r, int c) {
  if (r > c) { int t = r; r = c; c = t; }
  if (f->D == 2) return PL_SXX + (r == 0 ? c : 2);          // xx, xy, yy
  static const int idx[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};  // xx, xy, xd, yy, yd, dd
  return P3_SXX + idx[r][c];
}

int rfsgpu_gm_size(rfsgpu_filter *f, int slot) {
  if (!f || slot < 0 || slot >= f->N) return -1;
  std::vector<double> pl;
  int n = 0;
  if (fetch_particle(f, slot, pl, n) != RFSGPU_OK) return -1;
  int k = 0;
  for (int m = 0; m < n; m++) if (!f->holes || pl[m] >= 0) k++;  // plane 0 = weight
  return k;
}

int rfsgpu_export_gm(rfsgpu_filter *f, int slot, int max_n, int *n_out, double *w, double *w_prev, double *mean, double *cov) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N) return fail(f, RFSGPU_ERR_INVALID, "export_gm: bad slot");
  std::vector<double> pl;
  int n = 0;
  int rc = fetch_particle(f, slot, pl, n);
  if (rc != RFSGPU_OK) return rc;
  const size_t c = f->cap;
  const int D = f->D;
  int k = 0;
  for (int m = 0; m < n; m++) {
    if (f->holes && pl[m] < 0) continue;  // hole left by merge
    if (k < max_n) {
      if (w) w[k] = pl[m];
      if (w_prev) w_prev[k] = pl[1 * c + m];
      if (mean) for (int d = 0; d < D; d++) mean[D * k + d] = pl[(size_t)mean_plane(f, d) * c + m];
      if (cov)
        for (int r = 0; r < D; r++)
          for (int q = 0; q < D; q++) cov[(size_t)D * D * k + D * r + q] = pl[(size_t)cov_plane(f, r, q) * c + m];
    }
    k++;
  }
  if (n_out) *n_out = k;
  return RFSGPU_OK;
}

int rfsgpu_get_landmark(rfsgpu_filter *f, int slot, int m, double *mean, double *cov, double *w) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N || m < 0) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  int n = 0;
  HIPCHK(hipMemcpyAsync(&n, f->B.count + slot, sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  if (m >= n) return RFSGPU_ERR_INVALID;
  double v[P3_COUNT];
  for (int pl = 0; pl < f->B.npl; pl++)
    HIPCHK(hipMemcpyAsync(&v[pl], f->B.slab[f->cur] + ((size_t)slot * f->B.npl + pl) * f->cap + m, sizeof(double), hipMemcpyDeviceToHost,
                          f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  const int D = f->D;
  for (int d = 0; d < D; d++) mean[d] = v[mean_plane(f, d)];
  for (int r = 0; r < D; r++)
    for (int q = 0; q < D; q++) cov[D * r + q] = v[cov_plane(f, r, q)];
  *w = v[0];
  return RFSGPU_OK;
}

int rfsgpu_import_gm(rfsgpu_filter *f, int slot, int n, const double *w, const double *mean, const double *cov) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N || n < 0) return fail(f, RFSGPU_ERR_INVALID, "import_gm: bad arguments");
  if (n > f->cap) return fail(f, RFSGPU_ERR_CAPACITY, "import_gm: more Gaussians than gm_capacity");
  hipSetDevice(f->device);
  const size_t c = f->cap;
  const int D = f->D;
  std::vector<double> pl((size_t)f->B.npl * c, 0.0);
  for (int m = 0; m < n; m++) {
    pl[m] = w[m];
    pl[1 * c + m] = 0.0;
    for (int d = 0; d < D; d++) pl[(size_t)mean_plane(f, d) * c + m] = mean[D * m + d];
    for (int r = 0; r < D; r++)
      for (int q = r; q < D; q++) pl[(size_t)cov_plane(f, r, q) * c + m] = cov[(size_t)D * D * m + D * r + q];  // upper triangle
  }
  HIPCHK(hipMemcpyAsync(f->B.slab[f->cur] + (size_t)slot * f->B.npl * c, pl.data(), pl.size() * sizeof(double), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.count + slot, &n, sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

int rfsgpu_import_aux(rfsgpu_filter *f, int slot, const int *unused_idx, int n_unused, int n_in_fov) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N || n_unused < 0 || (n_unused > 0 && !unused_idx)) return fail(f, RFSGPU_ERR_INVALID, "import_aux: bad arguments");
  unsigned long long m = 0;
  for (int k = 0; k < n_unused; k++) {
    if (unused_idx[k] < 0 || unused_idx[k] >= RFSGPU_MAX_Z) return fail(f, RFSGPU_ERR_INVALID, "import_aux: measurement index out of range");
    m |= 1ull << unused_idx[k];
  }
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(f->B.unusedMask + slot, &m, sizeof(m), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.nInFov + slot, &n_in_fov, sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

int rfsgpu_export_birth_candidates(rfsgpu_filter *f, int slot, int max_n, int *n_out, double *mean, double *cov, int *n_support, int *n_checks) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N) return fail(f, RFSGPU_ERR_INVALID, "export_birth_candidates: bad slot");
  hipSetDevice(f->device);
  int nc = 0;
  std::vector<double> m((size_t)RFSGPU_MAX_CANDIDATES * 3), c((size_t)RFSGPU_MAX_CANDIDATES * 6);
  std::vector<int> su(RFSGPU_MAX_CANDIDATES), ch(RFSGPU_MAX_CANDIDATES);
  HIPCHK(hipMemcpyAsync(&nc, f->B.candCount + slot, sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipMemcpyAsync(m.data(), f->B.candMean + (size_t)slot * RFSGPU_MAX_CANDIDATES * 3, m.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipMemcpyAsync(c.data(), f->B.candCov + (size_t)slot * RFSGPU_MAX_CANDIDATES * 6, c.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipMemcpyAsync(su.data(), f->B.candSup + (size_t)slot * RFSGPU_MAX_CANDIDATES, su.size() * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipMemcpyAsync(ch.data(), f->B.candChk + (size_t)slot * RFSGPU_MAX_CANDIDATES, ch.size() * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  const int D = f->D;
  static const int idx3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  for (int k = 0; k < nc && k < max_n; k++) {
    for (int d = 0; d < D; d++) mean[D * k + d] = m[3 * k + d];
    for (int r = 0; r < D; r++)
      for (int q = 0; q < D; q++) cov[(size_t)D * D * k + D * r + q] = c[6 * k + idx3[r][q]];
    n_support[k] = su[k];
    n_checks[k] = ch[k];
  }
  if (n_out) *n_out = nc;
  return RFSGPU_OK;
}
int rfsgpu_import_birth_candidates(rfsgpu_filter *f, int slot, int n, const double *mean, const double *cov, const int *n_support, const int *n_checks) {
  CHECK_HANDLE(f);
  if (f->batch && !batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_import_birth_candidates", ON_BATCH);
  if (slot < 0 || slot >= f->N || n < 0 || n > RFSGPU_MAX_CANDIDATES) return fail(f, RFSGPU_ERR_INVALID, "import_birth_candidates: bad arguments");
  hipSetDevice(f->device);
  if (n > 0) f->candUsed = true;
  const int D = f->D;
  static const int idx3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  std::vector<double> m((size_t)RFSGPU_MAX_CANDIDATES * 3, 0.0), c((size_t)RFSGPU_MAX_CANDIDATES * 6, 0.0);
  std::vector<int> su(RFSGPU_MAX_CANDIDATES, 0), ch(RFSGPU_MAX_CANDIDATES, 0);
  for (int k = 0; k < n; k++) {
    for (int d = 0; d < D; d++) m[3 * k + d] = mean[D * k + d];
    for (int r = 0; r < D; r++)
      for (int q = r; q < D; q++) c[6 * k + idx3[r][q]] = cov[(size_t)D * D * k + D * r + q];
    su[k] = n_support[k];
    ch[k] = n_checks[k];
  }
  HIPCHK(hipMemcpyAsync(f->B.candMean + (size_t)slot * RFSGPU_MAX_CANDIDATES * 3, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.candCov + (size_t)slot * RFSGPU_MAX_CANDIDATES * 6, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.candSup + (size_t)slot * RFSGPU_MAX_CANDIDATES, su.data(), su.size() * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.candChk + (size_t)slot * RFSGPU_MAX_CANDIDATES, ch.data(), ch.size() * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->B.candCount + slot, &n, sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

// ---- the hot path ----------------------------------------------------------------------------------

static int set_lds_impl(rfsgpu_filter *f, const void *kernel, size_t bytes) {
  if ((long long)bytes > 160 * 1024) return fail(f, RFSGPU_ERR_CAPACITY, "kernel needs more than 160 KiB of LDS: lower gm_capacity");
  if (bytes > 48 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return RFSGPU_OK;
}
#define set_lds(f, kernel, bytes) set_lds_impl(f, reinterpret_cast<const void *>(&kernel), bytes)

static int launch_update_map(rfsgpu_filter *f) {
  const int nZ = f->nZ;
  if (f->D == 3) {
    if (f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "Victoria Park model: rfsgpu_set_laser_scan must precede the update");
    const size_t b = vp_shared_lds_bytes(nZ, f->B.nScan) + 2 * vp_update_lds_bytes_per_wave(f->cap);
    int rc3;
    if ((rc3 = set_lds(f, vp_update_map_kernel<2>, b)) != RFSGPU_OK) return rc3;
    vp_update_map_kernel<2><<<(f->N + 1) / 2, 128, b, f->stream>>>(f->B, f->P, f->cur, nZ);
    HIPCHK(hipGetLastError());
    return RFSGPU_OK;
  }
  auto bytes = [&](int wpb) { return (size_t)RFS_Z_LDS_BYTES + (size_t)wpb * update_map_lds_bytes_per_wave(f->cap); };
  int rc;
  // The workgroup form of the phase (the fused step's), several waves per particle: two up to capacity 512, four above (a pass
  // covers 64 landmarks per wave).  configs[1] (cap 384): 47.0 us with the one-wave kernel, 38.9 with two waves, 57.4 with three,
  // 43.7 with four; configs[2]'s shard (cap 640): 106.8 / 75.4 / 77.1 / 67.8.  RFSGPU_UPDMAP_WPP = 1 .. 4 overrides (1: the
  // one-wave kernels below).
  const size_t bb = (size_t)RFS_Z_LDS_BYTES + update_map_block_lds_bytes(f->cap);
  const int wppEnv = f->updMapWppOverride;   // (read at create, like the other switches)
  const int wppU = (wppEnv >= 1 && wppEnv <= 4) ? wppEnv : (f->cap > 512 ? 4 : 2);
  if (wppU != 1 && bb <= 64 * 1024) {
    if (wppU == 2) {
      if ((rc = set_lds(f, phd_update_map_block_kernel<2>, bb)) != RFSGPU_OK) return rc;
      phd_update_map_block_kernel<2><<<f->N, 128, bb, f->stream>>>(f->B, f->P, f->cur, nZ, f->B.Z);
    } else if (wppU == 3) {
      if ((rc = set_lds(f, phd_update_map_block_kernel<3>, bb)) != RFSGPU_OK) return rc;
      phd_update_map_block_kernel<3><<<f->N, 192, bb, f->stream>>>(f->B, f->P, f->cur, nZ, f->B.Z);
    } else {
      if ((rc = set_lds(f, phd_update_map_block_kernel<4>, bb)) != RFSGPU_OK) return rc;
      phd_update_map_block_kernel<4><<<f->N, 256, bb, f->stream>>>(f->B, f->P, f->cur, nZ, f->B.Z);
    }
    HIPCHK(hipGetLastError());
    return RFSGPU_OK;
  }
  if (bytes(4) <= 64 * 1024) {
    if ((rc = set_lds(f, phd_update_map_kernel<4>, bytes(4))) != RFSGPU_OK) return rc;
    phd_update_map_kernel<4><<<(f->N + 3) / 4, 256, bytes(4), f->stream>>>(f->B, f->P, f->cur, nZ, f->B.Z);
  } else {
    if ((rc = set_lds(f, phd_update_map_kernel<1>, bytes(1))) != RFSGPU_OK) return rc;
    phd_update_map_kernel<1><<<f->N, 64, bytes(1), f->stream>>>(f->B, f->P, f->cur, nZ, f->B.Z);
  }
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}

static int eval_cap(const rfsgpu_filter *f) {
  int c = f->cfg.importanceWeightingEvalPointCount;
  if (c < 0 || c > RFSGPU_MAX_EVAL) c = RFSGPU_MAX_EVAL;
  if (c < 1) c = 1;
  return c;
}

#ifndef WEIGHT_WPP
#define WEIGHT_WPP 2
#endif
static int launch_weighting(rfsgpu_filter *f) {
  const int nZ = f->nZ, ec = eval_cap(f);
  const size_t per = weight_lds_bytes_per_wave(f->cap, ec, nZ);
  const int src = f->cur, dst = f->cur ^ 1;
  int rc;  // (the Murty job counter was cleared by stage_step_kernel)
  if (f->D == 3) {
    const size_t b = vp_shared_lds_bytes(nZ, f->B.nScan) + 2 * vp_weight_lds_bytes_per_wave(f->cap, ec, nZ);
    if ((rc = set_lds(f, vp_weighting_kernel<2>, b)) != RFSGPU_OK) return rc;
    vp_weighting_kernel<2><<<(f->N + 1) / 2, 128, b, f->stream>>>(f->B, f->P, src, dst, nZ, ec, f->Q);
    HIPCHK(hipGetLastError());
    f->cur = dst;
    if (murty_launch(f->Q, f->MS, f->B, f->stream, nullptr, 0, nullptr, 0, f->hJobCount) != 0) return fail(f, RFSGPU_ERR_HIP, "murty launch failed");
    return RFSGPU_OK;
  }
  {  // one workgroup of WEIGHT_WPP waves per particle
    const size_t b = (size_t)RFS_Z_LDS_BYTES + per + WEIGHT_SCRATCH_BYTES;
    if ((rc = set_lds(f, phd_weight_multifeature_kernel<WEIGHT_WPP>, b)) != RFSGPU_OK) return rc;
    phd_weight_multifeature_kernel<WEIGHT_WPP><<<f->N, WEIGHT_WPP * 64, b, f->stream>>>(f->B, f->P, src, dst, nZ, ec, f->Q);
  }
  HIPCHK(hipGetLastError());
  f->cur = dst;
  if (f->evAfterWeightKernel) HIPCHK(hipEventRecord(f->evAfterWeightKernel, f->stream));
  // Murty-200 for partitions with nR + nC > 8: runs only when the queue is non-empty (device-side early exit)
  rc = murty_launch(f->Q, f->MS, f->B, f->stream, nullptr, 0, nullptr, 0, f->hJobCount);
  if (rc != 0) return fail(f, RFSGPU_ERR_HIP, "murty launch failed");
  return RFSGPU_OK;
}

}  // extern "C" (templates need C++ linkage)
#ifndef MERGE_WPP
#define MERGE_WPP 2
#endif
template <bool FUSE>
static int launch_merge_t(rfsgpu_filter *f) {
  const int cur = f->cur, dst = f->cur ^ 1;
  int rc;
  if (f->D == 3) {
    const size_t b = vp_merge_lds_bytes_per_wave(f->cap);
    if ((rc = set_lds(f, (vp_merge_kernel<1, FUSE>), b)) != RFSGPU_OK) return rc;
    vp_merge_kernel<1, FUSE><<<f->N, 64, b, f->stream>>>(f->B, f->P, cur, dst);
    HIPCHK(hipGetLastError());
    if (FUSE) f->cur = dst;
    return RFSGPU_OK;
  }
  // one workgroup of MERGE_WPP waves per particle
  const size_t per = merge_lds_bytes_per_block(f->cap, MERGE_WPP);
  if ((rc = set_lds(f, (gm_merge_kernel<MERGE_WPP, FUSE>), per)) != RFSGPU_OK) return rc;
  gm_merge_kernel<MERGE_WPP, FUSE><<<f->N, MERGE_WPP * 64, per, f->stream>>>(f->B, f->P, cur, dst);
  HIPCHK(hipGetLastError());
  if (FUSE) f->cur = dst;
  return RFSGPU_OK;
}
extern "C" {
static int launch_merge(rfsgpu_filter *f) { return launch_merge_t<false>(f); }
static int launch_merge_prune(rfsgpu_filter *f) { return launch_merge_t<true>(f); }

static int launch_prune(rfsgpu_filter *f) {
  const size_t per = gm_prune_lds_bytes_per_wave(f->cap);
  const int src = f->cur, dst = f->cur ^ 1;
  int rc;
  if ((rc = set_lds(f, gm_prune_kernel<4>, 4 * per)) != RFSGPU_OK) return rc;
  gm_prune_kernel<4><<<(f->N + 3) / 4, 256, 4 * per, f->stream>>>(f->B, f->P, src, dst);
  HIPCHK(hipGetLastError());
  f->cur = dst;
  return RFSGPU_OK;
}

static int stage_measurements(rfsgpu_filter *f, const double *z, int n_z) {
  if (n_z < 0 || n_z > RFSGPU_MAX_Z) return fail(f, RFSGPU_ERR_INVALID, "at most RFSGPU_MAX_Z measurements per update");
  if (n_z > 0 && !z) return fail(f, RFSGPU_ERR_INVALID, "null measurement buffer");
  hipSetDevice(f->device);
  {
    // The measurement set (<= 1.5 KB) travels in the kernel-argument block of one tiny kernel that also clears the Murty
    // queue for this step: no staging buffer, no copy-engine hop between compute kernels, and the caller's buffer is
    // free again when this call returns.
    ZArg za;
    const int nd = n_z * f->D;
    if (nd > 0) memcpy(za.v, z, (size_t)nd * sizeof(double));
    stage_step_kernel<<<1, 256, 0, f->stream>>>(za, f->B.Z, nd, f->Q.count);
    HIPCHK(hipGetLastError());
  }
  f->nZ = n_z;
  if (n_z > 0) f->resampleOccured = false;   // RBPHDFilter.hpp:526 (an update with measurements; its resampling decision follows)
  return RFSGPU_OK;
}

int rfsgpu_update_map(rfsgpu_filter *f, const double *z, int n_z) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_update_map", ON_BATCH);
  long long t0 = now_ns();
  int rc = stage_measurements(f, z, n_z);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_UM0], f->stream));
  if ((rc = launch_update_map(f)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_UM1], f->stream));
  rc = check_device_errors(f);
  accumulate(f->ev[EV_UM0], f->ev[EV_UM1], f->timing.mapUpdate_wall, &f->lastKernelNs[0]);
  f->timing.mapUpdate_kf_wall = f->timing.mapUpdate_wall;  // KF correct is fused into the same kernel
  f->timing.mapUpdate_cpu += now_ns() - t0;
  return rc;
}
int rfsgpu_importance_weighting(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_importance_weighting", ON_BATCH);
  long long t0 = now_ns();
  hipSetDevice(f->device);
  HIPCHK(hipEventRecord(f->ev[EV_UM1], f->stream));
  int rc = launch_weighting(f);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_W1], f->stream));
  rc = check_device_errors(f);
  accumulate(f->ev[EV_UM1], f->ev[EV_W1], f->timing.particleWeighting_wall, &f->lastKernelNs[1]);
  f->timing.particleWeighting_cpu += now_ns() - t0;
  return rc;
}
int rfsgpu_merge(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_merge", ON_BATCH);
  f->holes = true;
  long long t0 = now_ns();
  hipSetDevice(f->device);
  HIPCHK(hipEventRecord(f->ev[EV_W1], f->stream));
  int rc = launch_merge(f);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_MG1], f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  accumulate(f->ev[EV_W1], f->ev[EV_MG1], f->timing.mapMerge_wall, &f->lastKernelNs[2]);
  f->timing.mapMerge_cpu += now_ns() - t0;
  return RFSGPU_OK;
}
int rfsgpu_prune(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_prune", ON_BATCH);
  f->holes = false;
  long long t0 = now_ns();
  hipSetDevice(f->device);
  HIPCHK(hipEventRecord(f->ev[EV_MG1], f->stream));
  int rc = launch_prune(f);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_PR1], f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  accumulate(f->ev[EV_MG1], f->ev[EV_PR1], f->timing.mapPrune_wall, &f->lastKernelNs[3]);
  f->timing.mapPrune_cpu += now_ns() - t0;
  return RFSGPU_OK;
}

// The fused step's variant for a launch of N particles: waves per particle, phase priorities, the LDS block of a workgroup (and how
// many workgroups a CU holds at that).  stepWppOverride 2 | 3 and prioOverride 0 | 1 replace the rule's choices (0 / negative: none).
struct StepVariant { int wpp, phasePrio, perCU; size_t ldsBytes; };
static StepVariant step_variant(int cap, int evalCap, int nZ, int N, int nCU, int stepWppOverride, int prioOverride) {
  // Waves per particle: two, unless the two-wave grid cannot be resident at once (large mixtures: the LDS block limits the
  // workgroups per CU) -- then three waves per particle finish each workgroup sooner and free its slot (measured on the
  // configs[2] shard, 2500 x 500 x 30 at cap 640: fused step 327 -> 263 us; at C2a, where all 2000 two-wave workgroups are
  // resident, three waves lose: 133 -> 180 us).  RFSGPU_STEP_WPP = 2 | 3 overrides.
  const size_t b2 = step_fused_lds_total(cap, evalCap, nZ, 2);
  const int perCU2 = (int)std::min<size_t>(8, b2 ? (size_t)(160 * 1024) / b2 : 8);
  // (three waves only where it is the LDS block that keeps two-wave workgroups below the 8 per CU the wave slots allow: at
  //  capacity 384 -- 9 blocks of LDS per CU -- a launch of more than 2048 particles is better off with two waves per particle
  //  in several rounds: 3000 particles 229 us against 389, 8000: 474 against 882)
  StepVariant v;
  v.wpp = ((long long)perCU2 * nCU >= N || perCU2 >= 8) ? 2 : 3;
  {  // (round 5) a launch small enough for every THREE-wave workgroup to be resident at once takes three waves per particle: a
     // particle's own chain is what such a launch lasts, and the third wave shortens it -- fused step at configs[1]'s shape with
     // 1000 / 500 / 250 particles 103.6 / 95.4 / 102.4 -> 99.3 / 86.1 / 94.6 us; at 2000 particles (1280 three-wave workgroups
     // resident) two waves stay: 112 against 180 us
    const size_t b3 = step_fused_lds_total(cap, evalCap, nZ, 3);
    const int perCU3 = (int)std::min<size_t>(16 / 3, b3 ? (size_t)(160 * 1024) / b3 : 16 / 3);
    if ((long long)perCU3 * nCU >= N) v.wpp = 3;
  }
  if (stepWppOverride == 2 || stepWppOverride == 3) v.wpp = stepWppOverride;
  v.ldsBytes = step_fused_lds_total(cap, evalCap, nZ, v.wpp);
  // phase priorities only when every workgroup is resident at once: 16 waves per CU at 128 VGPRs, LDS permitting
  v.perCU = (int)std::min<size_t>(16 / v.wpp, v.ldsBytes ? (size_t)(160 * 1024) / v.ldsBytes : 16);
  v.phasePrio = prioOverride >= 0 ? (prioOverride ? 1 : 0) : ((long long)v.perCU * nCU >= N ? 1 : 0);
  return v;
}
// All four phases back to back on the stream, ONE host sync at the end (RBPHDFilter::update body :444-523).
static const StepOut NO_OUT{nullptr, nullptr, 0, nullptr, nullptr, 0, 0};
static const StepPredict NO_HEAD{0, 0, nullptr, nullptr, 0};
static int vp_order_buffers(rfsgpu_filter *f);
static int update_async_impl(rfsgpu_filter *f, const double *z, int n_z, bool with_sums, int normalize, const StepPredict &sp = NO_HEAD, const StepOut &so = NO_OUT,
                             hipEvent_t waitBeforePost = nullptr);
int rfsgpu_update(rfsgpu_filter *f, const double *z, int n_z) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_update", ON_BATCH);
  f->holes = false;
  if (n_z == 0) return RFSGPU_OK;  // :450-452
  // 2-D model: ONE fused launch (+ the post kernel) unless the caller asked for phase-resolved timing (rfsgpu_set_phase_timing):
  // the same bits either way, 26 % less device time at configs[1]; the whole step is then booked under TimingInfo::mapUpdate
  if (f->fuseSteps && !f->phaseTiming) {   // (r3: the Victoria Park model too -- vp_step_fused_kernel)
    const int rc = update_async_impl(f, z, n_z, false, 0);
    return rc != RFSGPU_OK ? rc : rfsgpu_synchronize(f);
  }
  long long t0 = now_ns();
  int rc = stage_measurements(f, z, n_z);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_UM0], f->stream));
  if ((rc = launch_update_map(f)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_UM1], f->stream));
  if (!f->cfg.useClusterProcess) {
    if ((rc = launch_weighting(f)) != RFSGPU_OK) return rc;
  }
  HIPCHK(hipEventRecord(f->ev[EV_W1], f->stream));
  // merge + prune fused in one kernel (the mapPrune bucket stays 0 on this path; rfsgpu_merge / rfsgpu_prune keep
  // the two-kernel form for phase-by-phase use)
  if ((rc = launch_merge_prune(f)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_MG1], f->stream));
  HIPCHK(hipEventRecord(f->ev[EV_PR1], f->stream));
  rc = check_device_errors(f);  // syncs
  accumulate(f->ev[EV_UM0], f->ev[EV_UM1], f->timing.mapUpdate_wall, &f->lastKernelNs[0]);
  f->timing.mapUpdate_kf_wall = f->timing.mapUpdate_wall;
  accumulate(f->ev[EV_UM1], f->ev[EV_W1], f->timing.particleWeighting_wall, &f->lastKernelNs[1]);
  accumulate(f->ev[EV_W1], f->ev[EV_MG1], f->timing.mapMerge_wall, &f->lastKernelNs[2]);
  accumulate(f->ev[EV_MG1], f->ev[EV_PR1], f->timing.mapPrune_wall, &f->lastKernelNs[3]);
  f->timing.mapUpdate_cpu += now_ns() - t0;
  return rc;
}

// Does the fused step being launched carry the timing events?  Every timingStride-th one does (the first of a filter always); a
// timed ring entry stands for itself + the untimed steps launched since the previous booking (2-D and Victoria Park steps alike).
static bool step_carries_events(rfsgpu_filter *f) {
  const bool timed = (f->stepSeq++ % (unsigned)f->timingStride) == 0;
  if (timed) { f->ringStands[f->ringCount] = f->untimedSince + 1; f->untimedSince = 0; }
  else f->untimedSince++;
  return timed;
}

// Fold the event pairs of the async steps recorded since the last harvest into TimingInfo / the kernel statistics.
// Caller has synchronised the stream.
static void harvest_async(rfsgpu_filter *f) {
  const int n = f->ringCount < RFSGPU_ASYNC_RING ? f->ringCount : RFSGPU_ASYNC_RING;
  for (int k = 0; k < n; k++) {
    hipEvent_t *e = f->ring[k];
    long long ns[3] = {0, 0, 0};
    if (f->ringFused[k]) {  // one kernel for the whole step: booked under mapUpdate, reported as kernel 0
      accumulate(e[0], e[3], f->timing.mapUpdate_wall, &ns[0]);
      // (only every timingStride-th fused step carries events: TimingInfo books the sampled step once for each step it stands for)
      if (f->ringStands[k] > 1) f->timing.mapUpdate_wall += ns[0] * (long long)(f->ringStands[k] - 1);
      for (int q = 0; q < 3; q++) { f->statNs[q] += (double)ns[q]; f->lastKernelNs[q] = ns[q]; }
      f->lastFusedNs = ns[0];
      {   // the post kernel (Murty jobs if any, queue reset, weight sums / division): event 1 is free on this path
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e[3], e[1]) == hipSuccess) f->statPostNs += (double)ms * 1.0e6;
      }
      f->statSteps++;
      continue;
    }
    accumulate(e[0], e[1], f->timing.mapUpdate_wall, &ns[0]);
    accumulate(e[1], e[2], f->timing.particleWeighting_wall, &ns[1]);
    if (f->ringHasMid[k]) {  // kernel statistics: the weighting kernel alone, without the (usually empty) Murty launch
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, e[1], e[4]) == hipSuccess) ns[1] = (long long)(ms * 1.0e6);
    }
    accumulate(e[2], e[3], f->timing.mapMerge_wall, &ns[2]);
    for (int q = 0; q < 3; q++) { f->statNs[q] += (double)ns[q]; f->lastKernelNs[q] = ns[q]; }
    f->statSteps++;
  }
  // un-sampled steps launched since the last sampled one: booked now at the last sample's duration (the stream is drained, they have
  // run), so that TimingInfo covers every step at every harvest instead of trailing by up to timingStride - 1 steps
  if (f->untimedSince > 0 && f->lastFusedNs > 0) {
    f->timing.mapUpdate_wall += f->lastFusedNs * (long long)f->untimedSince;
    f->untimedSince = 0;
  }
  f->timing.mapUpdate_kf_wall = f->timing.mapUpdate_wall;
  f->ringCount = 0;
}

// Shared body of the stream-ordered steps.  with_sums: the step's post kernel also leaves {sum w, sum w^2} in the bound sums
// buffer (and divides the weights by the sum when normalize != 0).
static int update_async_impl(rfsgpu_filter *f, const double *z, int n_z, bool with_sums, int normalize, const StepPredict &sp, const StepOut &so,
                             hipEvent_t waitBeforePost) {
  f->holes = false;
  if (n_z == 0) return RFSGPU_OK;  // :450-452
  long long t0 = now_ns();
  if (f->ringCount >= RFSGPU_ASYNC_RING) {  // ring full: drain (one sync per RFSGPU_ASYNC_RING steps)
    hipSetDevice(f->device);
    HIPCHK(hipStreamSynchronize(f->stream));
    harvest_async(f);
  }
  int rc;
  hipEvent_t *e = f->ring[f->ringCount];
  f->ringFused[f->ringCount] = false;
  if (f->D == 2 && f->fuseSteps) {
    // the whole step in one launch (step_fused.h), the measurement set riding in its kernel arguments; then the post kernel:
    // Murty partitions (if any), queue reset, weight sums / normalisation
    if (n_z < 0 || n_z > RFSGPU_MAX_Z) return fail(f, RFSGPU_ERR_INVALID, "at most RFSGPU_MAX_Z measurements per update");
    if (!z) return fail(f, RFSGPU_ERR_INVALID, "null measurement buffer");
    hipSetDevice(f->device);
    ZArg za;
    memcpy(za.v, z, (size_t)n_z * 2 * sizeof(double));
    f->nZ = n_z;
    if (n_z > 0) f->resampleOccured = false;
    const bool timed = step_carries_events(f);   // (rfsgpu_set_step_timing_stride)
    if (timed) HIPCHK(hipEventRecord(e[0], f->stream));
    const int ec = eval_cap(f), useW = f->cfg.useClusterProcess ? 0 : 1;
    // (RFSGPU_STEP_PHASE_PRIO = 0 | 1: tuning override of the rule's choice)
    static const int prioOverride = [] { const char *e = getenv("RFSGPU_STEP_PHASE_PRIO"); return e ? atoi(e) : -1; }();
    const StepVariant sv = step_variant(f->cap, ec, f->nZ, f->N, f->nCU, f->stepWppOverride, prioOverride);
    const int wpp = sv.wpp, phasePrio = sv.phasePrio, perCU = sv.perCU;
    const size_t b = sv.ldsBytes;
    f->lastStepVariant[0] = wpp; f->lastStepVariant[1] = phasePrio; f->lastStepVariant[2] = 5; f->lastStepVariant[3] = sp.mode ? 2 : (sp.inMask ? 3 : 1);   // ([3]: 1 = fused step, 2 = with the predict at its head, 3 = with the input pull only)
    // (one instantiation per {waves per particle, phase priorities, merge grid} x {plain step, step with the predict at its head})
    // cost-ordered launch for the instantiations without phase priorities (several rounds of workgroups; step_fused.h StepLaunchOrder)
    if ((rc = vp_order_buffers(f)) != RFSGPU_OK) return rc;
    const StepLaunchOrder sloOn{f->vpOrderMode ? f->vpCost : nullptr, f->vpOrderMode ? f->vpOrder : nullptr}, sloOff{nullptr, nullptr};
    bool orderedLaunch = false;
#define STEP_LAUNCH(WPPV, PRIO, GLV, BYTES)                                                                                            \
    do {                                                                                                                                \
      if (sp.mode || sp.inMask) {                                                                                                        \
        if ((rc = set_lds(f, (phd_step_fused_kernel<WPPV, PRIO, GLV, true>), BYTES)) != RFSGPU_OK) return rc;                           \
        phd_step_fused_kernel<WPPV, PRIO, GLV, true><<<f->N, WPPV * 64, BYTES, f->stream>>>(f->B, f->P, f->cur, f->nZ, ec, useW, f->Q, za, sp, PRIO ? sloOff : sloOn);  \
      } else {                                                                                                                          \
        if ((rc = set_lds(f, (phd_step_fused_kernel<WPPV, PRIO, GLV, false>), BYTES)) != RFSGPU_OK) return rc;                          \
        phd_step_fused_kernel<WPPV, PRIO, GLV, false><<<f->N, WPPV * 64, BYTES, f->stream>>>(f->B, f->P, f->cur, f->nZ, ec, useW, f->Q, za, sp, PRIO ? sloOff : sloOn); \
      }                                                                                                                                 \
      orderedLaunch = !(PRIO);                                                                                                          \
    } while (0)
    if (wpp == 2) {
      if (phasePrio) STEP_LAUNCH(2, true, 5, b);
      else STEP_LAUNCH(2, false, 5, b);
    } else {
      // the 64 x 64 merge grid where its 6 KB of extra cursors leave as many three-wave workgroups resident (merge_prune.h);
      // RFSGPU_MERGE_GRID = 5 | 6 overrides
      const size_t b6 = step_fused_lds_total(f->cap, ec, f->nZ, 3, 6);
      const int perCU6 = (int)std::min<size_t>(16 / 3, b6 ? (size_t)(160 * 1024) / b6 : 16);
      const bool fine = f->mergeGridOverride ? f->mergeGridOverride == 6 : (perCU6 == perCU && perCU6 > 0);
      if (fine) {
        const int prio6 = (long long)perCU6 * f->nCU >= f->N ? 1 : 0;
        f->lastStepVariant[1] = prio6; f->lastStepVariant[2] = 6;
        if (prio6) STEP_LAUNCH(3, true, 6, b6);
        else STEP_LAUNCH(3, false, 6, b6);
      } else {
        if (phasePrio) STEP_LAUNCH(3, true, 5, b);
        else STEP_LAUNCH(3, false, 5, b);
      }
    }
#undef STEP_LAUNCH
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(e[3], f->stream));
    if (waitBeforePost) HIPCHK(hipStreamWaitEvent(f->stream, waitBeforePost, 0));   // (the collective that produced so.preDiv, on another stream)
    const bool sortCosts = orderedLaunch && f->vpOrderMode == 2;
    const StepOrderArg sord{sortCosts ? f->vpCost : nullptr, f->vpOrder, f->N, f->vpCost + f->Ncap, f->vpParity};
    if (sortCosts) f->vpParity ^= 1;
    if (murty_launch(f->Q, f->MS, f->B, f->stream, with_sums ? f->dSums : nullptr, normalize, &za, 2 * n_z, f->hJobCount, so, sord) != 0) return fail(f, RFSGPU_ERR_HIP, "post kernel launch failed");
    if (timed) HIPCHK(hipEventRecord(e[1], f->stream));
    f->cur ^= 1;  // the map update works in place, the weighting phase leaves only a permutation in LDS, merge + prune write the other slab
    if (timed) {
      f->ringFused[f->ringCount] = true;
      f->ringCount++;
    }
    f->timing.mapUpdate_cpu += now_ns() - t0;
    return RFSGPU_OK;
  }
  if (f->D == 3 && f->fuseSteps) {
    // Victoria Park: the whole step in one launch (vp.h, vp_step_fused_kernel: one wavefront per particle through updateMap ->
    // importanceWeighting -> merge + prune, the sorted order a permutation in LDS), then the post kernel as for the 2-D model
    if (n_z < 0 || n_z > RFSGPU_MAX_Z) return fail(f, RFSGPU_ERR_INVALID, "at most RFSGPU_MAX_Z measurements per update");
    if (!z) return fail(f, RFSGPU_ERR_INVALID, "null measurement buffer");
    if (f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "Victoria Park model: rfsgpu_set_laser_scan must precede the update");
    hipSetDevice(f->device);
    ZArg za;
    memcpy(za.v, z, (size_t)n_z * 3 * sizeof(double));
    f->nZ = n_z;
    if (n_z > 0) f->resampleOccured = false;
    const bool timed = step_carries_events(f);
    if (timed) HIPCHK(hipEventRecord(e[0], f->stream));
    const int ec = eval_cap(f), useW = f->cfg.useClusterProcess ? 0 : 1;
    const size_t shared = vp_shared_lds_bytes(f->nZ, f->B.nScan), per = vp_step_lds_bytes_per_wave(f->cap, ec, f->nZ);
    f->lastStepVariant[0] = 1; f->lastStepVariant[1] = 0; f->lastStepVariant[2] = 0; f->lastStepVariant[3] = 1;
    // cost-ordered launch (round 6, murty.h step_cost_order_class): this step's particles in the order the previous step's post kernel
    // left -- longest first --, this step's durations captured for the next one
    if ((rc = vp_order_buffers(f)) != RFSGPU_OK) return rc;
    const int *vpOrd = f->vpOrderMode ? f->vpOrder : nullptr;
    const StepOrderArg sord{f->vpOrderMode == 2 ? f->vpCost : nullptr, f->vpOrder, f->N, f->vpCost + f->Ncap, f->vpParity};
    if (f->vpOrderMode == 2) f->vpParity ^= 1;
    if (shared + 2 * per <= (size_t)64 * 1024) {
      const size_t b = shared + 2 * per;
      if ((rc = set_lds(f, vp_step_fused_kernel<2>, b)) != RFSGPU_OK) return rc;
      vp_step_fused_kernel<2><<<(f->N + 1) / 2, 128, b, f->stream>>>(f->B, f->P, f->cur, f->nZ, ec, useW, f->Q, za, f->vpCost, vpOrd);
    } else {
      const size_t b = shared + per;
      if ((rc = set_lds(f, vp_step_fused_kernel<1>, b)) != RFSGPU_OK) return rc;
      vp_step_fused_kernel<1><<<f->N, 64, b, f->stream>>>(f->B, f->P, f->cur, f->nZ, ec, useW, f->Q, za, f->vpCost, vpOrd);
    }
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(e[3], f->stream));
    if (waitBeforePost) HIPCHK(hipStreamWaitEvent(f->stream, waitBeforePost, 0));
    if (murty_launch(f->Q, f->MS, f->B, f->stream, with_sums ? f->dSums : nullptr, normalize, &za, 3 * n_z, f->hJobCount, so, sord) != 0) return fail(f, RFSGPU_ERR_HIP, "post kernel launch failed");
    if (timed) HIPCHK(hipEventRecord(e[1], f->stream));
    f->cur ^= 1;
    if (timed) {
      f->ringFused[f->ringCount] = true;
      f->ringCount++;
    }
    f->timing.mapUpdate_cpu += now_ns() - t0;
    return RFSGPU_OK;
  }
  f->lastStepVariant[0] = f->lastStepVariant[1] = f->lastStepVariant[2] = f->lastStepVariant[3] = 0;   // three kernels
  rc = stage_measurements(f, z, n_z);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(e[0], f->stream));
  if ((rc = launch_update_map(f)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(e[1], f->stream));
  f->ringHasMid[f->ringCount] = false;
  if (!f->cfg.useClusterProcess) {
    f->evAfterWeightKernel = (f->D == 2) ? e[4] : nullptr;
    rc = launch_weighting(f);
    f->ringHasMid[f->ringCount] = f->evAfterWeightKernel != nullptr;
    f->evAfterWeightKernel = nullptr;
    if (rc != RFSGPU_OK) return rc;
  }
  HIPCHK(hipEventRecord(e[2], f->stream));
  if ((rc = launch_merge_prune(f)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(e[3], f->stream));
  f->ringCount++;
  f->timing.mapUpdate_cpu += now_ns() - t0;
  if (with_sums) {
    if ((rc = rfsgpu_weight_sums_async(f)) != RFSGPU_OK) return rc;
    if (normalize) return rfsgpu_normalize_weights(f, 0.0, f->dSums);
  }
  return RFSGPU_OK;
}
int rfsgpu_update_async(rfsgpu_filter *f, const double *z, int n_z) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_update_async", ON_BATCH);
  return update_async_impl(f, z, n_z, false, 0);
}
int rfsgpu_step_async(rfsgpu_filter *f, const double *z, int n_z, int normalize) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_step_async", ON_BATCH);
  if (n_z == 0) {  // no update (:450-452), but the weights are still summed / normalised as the caller asked
    int rc = rfsgpu_weight_sums_async(f);
    if (rc != RFSGPU_OK) return rc;
    return normalize ? rfsgpu_normalize_weights(f, 0.0, f->dSums) : RFSGPU_OK;
  }
  return update_async_impl(f, z, n_z, true, normalize);
}

// The step of a multi-GPU host whose weight normalisation trails by one step (round 5).  As rfsgpu_step_async
// with normalize = 0 -- this shard's {sum w, sum w^2} go to the bound sums buffer -- except that the post kernel first divides
// the weights by *prev_total_dev, the all-reduced total of the PREVIOUS step (NULL: no division), and waits for `wait_event` (a
// hipEvent_t recorded on ANOTHER stream behind the collective that produced that total; NULL: none) only between the step kernel
// and the post kernel: the collective of step k runs beside the step kernel of step k + 1 instead of in front of it.
int rfsgpu_step_async_deferred(rfsgpu_filter *f, const double *z, int n_z, const void *prev_total_dev, void *wait_event) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_step_async_deferred", ON_BATCH);
  hipSetDevice(f->device);
  if (n_z == 0 || !f->fuseSteps || f->phaseTiming) {        // no fused step: the same arithmetic with the stand-alone kernels, in stream order
    if (wait_event) HIPCHK(hipStreamWaitEvent(f->stream, (hipEvent_t)wait_event, 0));
    if (n_z > 0) { const int rc = update_async_impl(f, z, n_z, false, 0); if (rc != RFSGPU_OK) return rc; }
    if (prev_total_dev) { const int rc = rfsgpu_normalize_weights(f, 0.0, prev_total_dev); if (rc != RFSGPU_OK) return rc; }
    return rfsgpu_weight_sums_async(f);
  }
  StepOut so = NO_OUT;
  so.preDiv = reinterpret_cast<const double *>(prev_total_dev);
  return update_async_impl(f, z, n_z, true, 0, NO_HEAD, so, (hipEvent_t)wait_event);
}

// The same without stream events.  The caller pairs every call with rfsgpu_collective_gate(side stream) -> its collective over the
// shards' sums into total_dev -> rfsgpu_collective_publish(side stream): the gate kernel waits on the device for this step's post
// kernel to have written the sums, the publish kernel raises the number the NEXT step's post kernel waits for (on the device, just
// before it divides by total_dev).  have_prev == 0: the first step of a run (or the first after a flush): nothing to divide by.
int rfsgpu_step_async_trailing(rfsgpu_filter *f, const double *z, int n_z, const void *total_dev, int have_prev) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_step_async_trailing", ON_BATCH);
  hipSetDevice(f->device);
  if (!total_dev) return fail(f, RFSGPU_ERR_INVALID, "step_async_trailing: null total buffer");
  const int k = ++f->collStep;
  if (n_z == 0 || !f->fuseSteps || f->phaseTiming || f->D != 2) {   // no 2-D fused step: stand-alone kernels in stream order, the hand-over by the same two small kernels
    if (have_prev) coll_gate_kernel<<<1, 64, 0, f->stream>>>(f->dCollSeq + 1, k - 1, f->B.err);
    if (n_z > 0) { const int rc = update_async_impl(f, z, n_z, false, 0); if (rc != RFSGPU_OK) return rc; }
    if (have_prev) { const int rc = rfsgpu_normalize_weights(f, 0.0, total_dev); if (rc != RFSGPU_OK) return rc; }
    const int rc = rfsgpu_weight_sums_async(f);
    coll_publish_kernel<<<1, 1, 0, f->stream>>>(f->dCollSeq, k);         // word [0]: "the sums of step k are out"
    HIPCHK(hipGetLastError());
    return rc;
  }
  StepOut so = NO_OUT;
  so.preDiv = have_prev ? reinterpret_cast<const double *>(total_dev) : nullptr;
  so.collSeq = f->dCollSeq; so.collNeed = have_prev ? k - 1 : 0; so.collPost = k;
  return update_async_impl(f, z, n_z, true, 0, NO_HEAD, so, nullptr);
}
// [multi] on `hip_stream` (the side stream of the collective): wait, on the device, until the post kernel of the last
// rfsgpu_step_async_trailing call has written this shard's sums.
int rfsgpu_collective_gate(rfsgpu_filter *f, void *hip_stream) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_collective_gate", ON_BATCH);
  hipSetDevice(f->device);
  coll_gate_kernel<<<1, 64, 0, (hipStream_t)hip_stream>>>(f->dCollSeq, f->collStep, f->B.err);
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
// [multi] on the same stream, behind the collective: the total of the last step is in place.
int rfsgpu_collective_publish(rfsgpu_filter *f, void *hip_stream) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_collective_publish", ON_BATCH);
  hipSetDevice(f->device);
  coll_publish_kernel<<<1, 1, 0, (hipStream_t)hip_stream>>>(f->dCollSeq + 1, f->collStep);   // word [1]: "the total of step k is in place"
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
// [multi] Do the engine's stream and `hip_stream` make progress SIDE BY SIDE?  The sequence-number hand-over above needs it: a post
// kernel on the engine's stream waits, on the device, for a word that a kernel on the side stream publishes LATER in submission
// order.  Two streams that a runtime maps onto one hardware queue (GPU_MAX_HW_QUEUES streams share four by default) serialise instead,
// and the wait can only run out.  The probe plays the hand-over once with nothing at stake: a one-thread waiter on the engine's
// stream (bounded: 0.2 s), then the publish on the side stream; *side_by_side = 1 if the waiter saw the word.  Hosts probe once
// per (stream, side stream) pair and use the stream-event form (rfsgpu_step_async_deferred) when the answer is 0
// (ShardedRBPHDFilter, rfsgpu_group_update_deferred, bench.py).  RFSGPU_COLL_PROBE_DELAY_MS (test hook): the publish is held back by
// a spinning kernel for that long -- past the bound the probe must answer 0 and the hosts must take the event form.
int rfsgpu_collective_probe(rfsgpu_filter *f, void *hip_stream, int *side_by_side) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_collective_probe", ON_BATCH);
  if (!side_by_side) return fail(f, RFSGPU_ERR_INVALID, "collective_probe: null result pointer");
  hipSetDevice(f->device);
  const int k = ++f->collProbeSeq;
  hipStream_t side = (hipStream_t)hip_stream;
  coll_probe_kernel<<<1, 64, 0, f->stream>>>(f->dCollSeq + 2, k, f->dCollSeq + 3, COLL_PROBE_TICKS);
  HIPCHK(hipGetLastError());
  if (const char *d = getenv("RFSGPU_COLL_PROBE_DELAY_MS")) {
    const long long ms = atoll(d);
    if (ms > 0) coll_spin_kernel<<<1, 64, 0, side>>>(ms * 100000ll);      // (100 MHz constant clock)
  }
  coll_publish_kernel<<<1, 1, 0, side>>>(f->dCollSeq + 2, k);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(f->stream));
  HIPCHK(hipStreamSynchronize(side));
  int verdict = 0;
  HIPCHK(hipMemcpy(&verdict, f->dCollSeq + 3, sizeof(int), hipMemcpyDeviceToHost));
  *side_by_side = verdict == k ? 1 : 0;
  return RFSGPU_OK;
}

// Buffers of the fused step's cost-ordered launch (Victoria Park step; 2-D step when its workgroups are not all resident), created with the first fused step: durations (zero) and the identity order.
__global__ void iota_kernel(int *p, int n) { const int k = blockIdx.x * blockDim.x + threadIdx.x; if (k < n) p[k] = k; }
static int vp_order_buffers(rfsgpu_filter *f) {
  if (f->vpCost && f->vpOrder && f->vpOrderN == f->N) return RFSGPU_OK;
  static const bool off = [] { const char *e = getenv("RFSGPU_VP_COST_ORDER"); return e && atoi(e) == 0; }();
  if (off) f->vpOrderMode = 0;
  if (!f->vpCost) { HIPCHK(hipMalloc(&f->vpCost, (size_t)(f->Ncap + 4) * sizeof(float))); HIPCHK(hipMemsetAsync(f->vpCost, 0, (size_t)(f->Ncap + 4) * sizeof(float), f->stream)); }
  if (!f->vpOrder) HIPCHK(hipMalloc(&f->vpOrder, (size_t)f->Ncap * sizeof(int)));
  iota_kernel<<<(f->Ncap + 255) / 256, 256, 0, f->stream>>>(f->vpOrder, f->Ncap);      // (first use, or the particle count has changed: every slot its own particle)
  HIPCHK(hipGetLastError());
  f->vpOrderN = f->N;
  return RFSGPU_OK;
}
// [bench] / [test] The Victoria Park step's launch order.  mode 0: slot == particle; 1: order_in (slot -> particle, a permutation of 0..N-1),
// frozen; 2: re-sorted by every step's post kernel from that step's durations, longest first (the default).  cost_out (N floats, may be
// null): the last step's duration per particle, 100 MHz ticks.
int rfsgpu_step_launch_order(rfsgpu_filter *f, int mode, const int *order_in, float *cost_out) {
  CHECK_HANDLE(f);
  if (mode < 0 || mode > 2 || (mode == 1 && !order_in)) return fail(f, RFSGPU_ERR_INVALID, "step_launch_order: mode 0, 1 (with an order) or 2");
  hipSetDevice(f->device);
  int rc = vp_order_buffers(f);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipStreamSynchronize(f->stream));
  if (cost_out) HIPCHK(hipMemcpy(cost_out, f->vpCost, (size_t)f->N * sizeof(float), hipMemcpyDeviceToHost));
  if (mode == 1) {
    std::vector<char> seen((size_t)f->N, 0);
    for (int k = 0; k < f->N; k++) { const int p = order_in[k]; if (p < 0 || p >= f->N || seen[p]) return fail(f, RFSGPU_ERR_INVALID, "step_launch_order: not a permutation"); seen[p] = 1; }
    HIPCHK(hipMemcpy(f->vpOrder, order_in, (size_t)f->N * sizeof(int), hipMemcpyHostToDevice));
  }
  f->vpOrderMode = mode;
  return RFSGPU_OK;
}

// ---- one submission per predict + update cycle (round 5) --------------------------------------------------------------------
// RBPHDFilter::predict's map part (:415-442) + the host's new poses / weights + RBPHDFilter::update's body (:444-523) as ONE
// stream-ordered chain.  Where the configuration allows it the predict runs at the head of the fused step kernel
// (step_fused.h): 2-D model, immediate births (no candidate lists), no slot-ordered inheritance walk pending, fused steps on, a
// non-empty measurement set; the births then read the OLD poses from the buffer the previous update used while the update reads
// the new ones from the other buffer (the two swap roles).  Otherwise the same calls a host would make one by one are issued
// here, in the reference's order: predict kernels, input copies, step.  Either way the results are those of
// rfsgpu_predict_map + rfsgpu_set_poses + rfsgpu_set_weights + rfsgpu_step_async, bit for bit.
static void ensure_ids(rfsgpu_filter *f);
// RFSGPU_IO_PROFILE=1: host-side shares of rfsgpu_update_io, printed when the process ends (tuning aid: tools/boundary_trace.py)
struct IoProfile {
  bool on = getenv("RFSGPU_IO_PROFILE") != nullptr;
  long long n = 0, stage = 0, launch = 0, wait = 0, copyOut = 0;
  ~IoProfile() {
    if (on && n) fprintf(stderr, "rfsgpu_update_io x %lld: inputs into the pinned slot %.2f us, launches %.2f us, wait for the delivery %.2f us, weights out %.2f us\n", n,
                         stage / 1e3 / n, launch / 1e3 / n, wait / 1e3 / n, copyOut / 1e3 / n);
  }
};
static IoProfile g_ioProf;
static int cycle_impl(rfsgpu_filter *f, int predict, const double *x, const double *cov, int cov_stride, const double *w_in, const double *z, int n_z,
                      bool with_sums, int normalize, bool deliver = false) {
  if (predict < -1 || predict > 1) return fail(f, RFSGPU_ERR_INVALID, "cycle: predict is RFSGPU_CYCLE_NO_PREDICT (-1), 0 (static step only) or 1 (births + static step)");
  if (cov && cov_stride != 0 && cov_stride != 9) return fail(f, RFSGPU_ERR_INVALID, "cycle: cov_stride must be 0 or 9");
  if (n_z < 0 || n_z > RFSGPU_MAX_Z || (n_z > 0 && !z)) return fail(f, RFSGPU_ERR_INVALID, "cycle: bad measurement set");
  hipSetDevice(f->device);
  f->outArmed = false;
  // is this step the 2-D fused kernel (whose head can take the predict and pull the inputs)?
  const bool head = n_z > 0 && f->D == 2 && f->fuseSteps && !f->phaseTiming;
  bool fuse = head && predict >= 0 && f->cfg.birthGaussianMeasurementCountThreshold == 1u && !f->fastSlamHandle;
  if (fuse && predict == 1 && f->resampleOccured) {
    if (f->inheritMode == RFSGPU_INHERIT_REFERENCE) {      // a slot with a foreign parent: the level-ordered walk, stand-alone kernels
      ensure_ids(f);
      for (int i = 0; i < f->N && fuse; i++) fuse = f->ppid[i] == i || f->ppid[i] < 0 || f->ppid[i] >= f->N;
    } else if (f->inheritMode == RFSGPU_INHERIT_EXTERNAL && !f->externalAck) {
      fuse = false;                                        // (rfsgpu_predict_map_async below refuses with the full message)
    }
  }
  if (predict >= 0 && !fuse) { const int rc = rfsgpu_predict_map_async(f, predict); if (rc != RFSGPU_OK) return rc; }
  StepPredict sp = NO_HEAD;
  if (fuse) { sp.mode = predict ? 2 : 1; sp.nZprev = f->nZ; sp.birthPose = f->B.pose; }
  const long long tp0 = g_ioProf.on ? now_ns() : 0;
  const bool pull = head && f->ioPull;                    // the step kernel reads the pinned slot itself (step_fused.h, StepPredict)
  if (x || w_in) {
    double *h = nullptr;
    int k = 0;
    { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
    const bool pullCov = pull && x && cov && cov_stride == 9;
    if (pull) {
      // 13 doubles per particle side by side: the workgroup that owns a particle reads them in one go (step_fused.h, StepPredict)
      sp.inPacked = h;
      sp.inMask = (x ? 1 : 0) | (pullCov ? 2 : 0) | (w_in ? 4 : 0);
      for (int i = 0; i < f->N; i++) {
        double *d = h + (size_t)13 * i;
        if (x) { d[0] = x[3 * i]; d[1] = x[3 * i + 1]; d[2] = x[3 * i + 2]; }
        if (pullCov) memcpy(d + 3, cov + (size_t)9 * i, 9 * sizeof(double));
        if (w_in) d[12] = w_in[i];
      }
    }
    if (x) {
      if (!pull) {
        memcpy(h, x, (size_t)f->N * 3 * sizeof(double));
        double *dst = fuse ? f->poseAlt : f->B.pose;       // fused predict + copy commands: the births still need the old poses
        HIPCHK(hipMemcpyAsync(dst, h, (size_t)f->N * 3 * sizeof(double), hipMemcpyHostToDevice, f->stream));
        if (fuse) { f->poseAlt = f->B.pose; f->B.pose = dst; }
      }
      // (the covariance's small / copy-command forms go behind the packed block; the births do not read the pose covariance)
      { const int rc = push_pose_cov(f, h + (size_t)f->Ncap * 13, cov, cov_stride, pullCov); if (rc != RFSGPU_OK) return rc; }
      f->P.poseCovStride = cov ? cov_stride : 0;
    }
    if (w_in && !pull) {
      double *hw = h + (size_t)f->Ncap * 12;
      memcpy(hw, w_in, (size_t)f->N * sizeof(double));
      HIPCHK(hipMemcpyAsync(f->B.weight, hw, (size_t)f->N * sizeof(double), hipMemcpyHostToDevice, f->stream));
    }
    if (!pull) HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
    else f->stagePendingSlot = k;
  }
  if (n_z == 0) {       // no update (:450-452); the weights are still summed / normalised as the caller asked
    if (!with_sums) return RFSGPU_OK;
    const int rc = rfsgpu_weight_sums_async(f);
    if (rc != RFSGPU_OK) return rc;
    return normalize ? rfsgpu_normalize_weights(f, 0.0, f->dSums) : RFSGPU_OK;
  }
  StepOut so = NO_OUT;
  if (deliver && pull) {
    if (!f->hOutW) {
      HIPCHK(hipHostMalloc(&f->hOutW, (size_t)f->Ncap * sizeof(double) + 2 * sizeof(int)));
      f->hOutFlag = reinterpret_cast<int *>(f->hOutW + f->Ncap);
      f->hOutFlag[0] = 0; f->hOutFlag[1] = 0;
    }
    so.hostW = f->hOutW; so.hostFlag = f->hOutFlag; so.seq = ++f->outSeq;
    f->outArmed = true;
  }
  const long long tp1 = g_ioProf.on ? now_ns() : 0;
  const int rc = update_async_impl(f, z, n_z, with_sums, normalize, sp, so);
  if (g_ioProf.on) { const long long tp2 = now_ns(); g_ioProf.stage += tp1 - tp0; g_ioProf.launch += tp2 - tp1; }
  if (f->stagePendingSlot >= 0) {            // the pinned slot is read by the kernels just enqueued: its event goes behind them
    if (rc == RFSGPU_OK) HIPCHK(hipEventRecord(f->stage.ev[f->stagePendingSlot], f->stream));
    f->stagePendingSlot = -1;
  }
  return rc;
}
int rfsgpu_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *w_in, const double *z, int n_z,
                       int normalize) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_cycle_async", ON_BATCH);
  return cycle_impl(f, predict, x, x_cov, cov_stride, w_in, z, n_z, true, normalize);
}
// The synchronous form for a host that stands where RBPHDFilter::update stands (:444-541): everything the update consumes goes in,
// the particle weights come back, ONE wait for the device and one error check -- in place of set_poses + set_weights + update +
// get_weights (four calls, two waits: 199 us per update at configs[1] against 125 us stream-ordered, bench.py `boundary`).
// (two halves, so that a group of shards can have every shard's chain in flight before it waits for the first: csrc/group.h)
static int update_io_begin(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *w_in, const double *z, int n_z,
                           bool want_weights) {
  int rc;
  if (f->phaseTiming) {
    // rfsgpu_set_phase_timing (the binding's RFSGPU_PHASE_TIMING=1): the caller wants TimingInfo's per-phase buckets, i.e. the phases as
    // separate launches with their own event pairs -- the call-by-call sequence, synchronous rfsgpu_update included
    f->outArmed = false;
    if (predict < -1 || predict > 1) return fail(f, RFSGPU_ERR_INVALID, "update_io: predict is RFSGPU_CYCLE_NO_PREDICT (-1), 0 or 1");
    if (predict >= 0 && (rc = rfsgpu_predict_map(f, predict)) != RFSGPU_OK) return rc;
    if (x && (rc = rfsgpu_set_poses(f, x, x_cov, x_cov ? cov_stride : 0)) != RFSGPU_OK) return rc;
    if (w_in && (rc = rfsgpu_set_weights(f, w_in)) != RFSGPU_OK) return rc;
    rc = rfsgpu_update(f, z, n_z);
  } else {
    rc = cycle_impl(f, predict, x, x_cov, cov_stride, w_in, z, n_z, false, 0, true);
  }
  if (rc != RFSGPU_OK) return rc;
  if (want_weights && !f->outArmed) {      // (3-D model, phase timing, an empty measurement set, RFSGPU_IO_PULL=0: copy commands)
    if (!f->hWeights) HIPCHK(hipHostMalloc(&f->hWeights, (size_t)f->Ncap * sizeof(double)));
    HIPCHK(hipMemcpyAsync(f->hWeights, f->B.weight, (size_t)f->N * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  }
  return RFSGPU_OK;
}
static int update_io_end(rfsgpu_filter *f, double *w_out) {
  hipSetDevice(f->device);
  if (f->outArmed) {
    // the post kernel's last workgroup writes weights, error word and -- behind a system-scope release -- the sequence number
    // into pinned memory: spin on it (bounded: after ~2 s the stream is asked instead, which also surfaces a launch failure)
    f->outArmed = false;
    const long long t0 = now_ns();
    bool seen = false;
    for (unsigned spin = 0;; spin++) {
      if (__atomic_load_n(&f->hOutFlag[1], __ATOMIC_ACQUIRE) == f->outSeq) { seen = true; break; }
      if ((spin & 1023u) == 1023u && now_ns() - t0 > 2000000000LL) break;
      __builtin_ia32_pause();
    }
    if (seen && f->hOutFlag[0] == 0) {
      const long long t1 = g_ioProf.on ? now_ns() : 0;
      if (w_out) memcpy(w_out, f->hOutW, (size_t)f->N * sizeof(double));
      if (g_ioProf.on) { g_ioProf.n++; g_ioProf.wait += t1 - t0; g_ioProf.copyOut += now_ns() - t1; }
      return RFSGPU_OK;
    }
    const int rc = check_device_errors(f);     // an error bit (or no answer): synchronise, read and clear the word, build the message
    harvest_async(f);
    // the stream is drained now: a step that merely outlasted the spin (large N, Murty-heavy, a profiler attached) HAS delivered
    if (!seen) seen = __atomic_load_n(&f->hOutFlag[1], __ATOMIC_ACQUIRE) == f->outSeq;
    if (w_out) memcpy(w_out, f->hOutW, (size_t)f->N * sizeof(double));
    if (rc == RFSGPU_OK && !seen) return fail(f, RFSGPU_ERR_HIP, "update_io: the post kernel never delivered its results");
    return rc;
  }
  const int rc = check_device_errors(f);      // the one wait (error word + weights land together)
  harvest_async(f);
  if (w_out && f->hWeights) memcpy(w_out, f->hWeights, (size_t)f->N * sizeof(double));
  return rc;
}
int rfsgpu_update_io(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *w_in, const double *z, int n_z,
                     double *w_out) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_update_io", ON_BATCH);
  long long t0 = now_ns();
  int rc = update_io_begin(f, predict, x, x_cov, cov_stride, w_in, z, n_z, w_out != nullptr);
  if (rc != RFSGPU_OK) return rc;
  rc = update_io_end(f, w_out);
  f->timing.mapUpdate_cpu += now_ns() - t0;
  return rc;
}

int rfsgpu_kernel_time_stats(rfsgpu_filter *f, double *avg_ns3, int *n_steps) {
  CHECK_HANDLE(f);
  if (!avg_ns3 || !n_steps) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  harvest_async(f);
  for (int q = 0; q < 3; q++) avg_ns3[q] = f->statSteps ? f->statNs[q] / f->statSteps : 0.0;
  *n_steps = f->statSteps;
  f->lastPostNs = f->statSteps ? f->statPostNs / f->statSteps : 0.0;
  f->statSteps = 0;
  f->statNs[0] = f->statNs[1] = f->statNs[2] = 0.0;
  f->statPostNs = 0.0;
  return RFSGPU_OK;
}
// Average duration (ns) of the step's POST kernel (murty_jobs_kernel: the Murty-200 partitions when the queue is not empty, queue
// reset, weight sums / division) over the fused steps covered by the last rfsgpu_kernel_time_stats call.
double rfsgpu_post_kernel_avg_ns(const rfsgpu_filter *f) { return f ? f->lastPostNs : 0.0; }
int rfsgpu_set_step_timing_stride(rfsgpu_filter *f, int every) {
  CHECK_HANDLE(f);
  if (every < 1) return fail(f, RFSGPU_ERR_INVALID, "the timing stride is at least 1");
  f->timingStride = every;
  return RFSGPU_OK;
}

// The birth + static-step launches of one predict.  LV selects the particles whose birth step runs (birth.h).
static void launch_predict_kernels(rfsgpu_filter *f, int add_birth, const BirthLevel &LV) {
  if (f->D == 3)
  {
    predict_map_general_kernel<3, 4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->P, f->cur, add_birth ? 1 : 0, f->nZ, LV);
    if (add_birth) predict_map_long_kernel<3, 2><<<(f->N + 1) / 2, 128, 0, f->stream>>>(f->B, f->P, f->cur, f->nZ, LV);   // (lists longer than a wavefront; the others exit at once)
  }
  else if (f->cfg.birthGaussianMeasurementCountThreshold != 1u)
  {
    predict_map_general_kernel<2, 4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->P, f->cur, add_birth ? 1 : 0, f->nZ, LV);
    if (add_birth) predict_map_long_kernel<2, 2><<<(f->N + 1) / 2, 128, 0, f->stream>>>(f->B, f->P, f->cur, f->nZ, LV);
  }
  else  // CountThreshold == 1: every unused measurement is born at once, no candidate can exist -> lane-parallel kernel
    predict_map_kernel<4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->P, f->cur, add_birth ? 1 : 0, f->nZ, LV);
}

// what a resampling copy / a migration row carries: pose + mixture only (RBPHDFilter: the per-slot birth state is copied
// lazily by the next predict, or by the host), or the birth bookkeeping as well (RFSGPU_INHERIT_EAGER, and FastSLAM handles)
static int map_only(const rfsgpu_filter *f) { return (f->inheritMode != RFSGPU_INHERIT_EAGER && !f->fastSlamHandle) ? 1 : 0; }
// ... of a batch: the lists travel where the batch keeps landmark candidates (Victoria Park FastSLAM filters, as on a FastSLAM handle)
static void ensure_ids(rfsgpu_filter *f) {
  while ((int)f->pid.size() < f->Ncap) { f->pid.push_back((int)f->pid.size()); f->ppid.push_back((int)f->ppid.size()); }
}

// the level and parent arrays and the staging area of birth_inherit_kernel<0/1>
static int inherit_buffers(rfsgpu_filter *f) {
  if (!f->dInhLevel) HIPCHK(hipMalloc(&f->dInhLevel, (size_t)f->Ncap * sizeof(int)));
  {  // every buffer under its own guard: a failed allocation leaves the others usable and is retried by the next call
    const size_t nc = (size_t)f->Ncap * RFSGPU_MAX_CANDIDATES;
    if (!f->dInhParent) HIPCHK(hipMalloc(&f->dInhParent, (size_t)f->Ncap * sizeof(int)));
    if (!f->inhTmp.unused) HIPCHK(hipMalloc(&f->inhTmp.unused, (size_t)f->Ncap * sizeof(unsigned long long)));
    if (!f->inhTmp.count) HIPCHK(hipMalloc(&f->inhTmp.count, (size_t)f->Ncap * sizeof(int)));
    if (!f->inhTmp.sup) HIPCHK(hipMalloc(&f->inhTmp.sup, nc * sizeof(int)));
    if (!f->inhTmp.chk) HIPCHK(hipMalloc(&f->inhTmp.chk, nc * sizeof(int)));
    if (!f->inhTmp.mean) HIPCHK(hipMalloc(&f->inhTmp.mean, nc * 3 * sizeof(double)));
    if (!f->inhTmp.cov) HIPCHK(hipMalloc(&f->inhTmp.cov, nc * 6 * sizeof(double)));
  }
  return RFSGPU_OK;
}
// The same predict behind pending rfsgpu_rbphd_cycle_async cycles: the ids and resampleOccured_ are the device's, so the levels are
// computed there (birth_walk.h) and the launches cannot depend on them: the staging pair and level 0 as above, a fixed
// RFSGPU_RBPHD_WALK_LEVELS of (copy, birth) pairs that find no slot of theirs where the walk is shallower, and one workgroup that
// finishes whatever lies deeper.  Nothing is read back.
static int predict_walk_device(rfsgpu_filter *f) {
  { const int rcb = inherit_buffers(f); if (rcb != RFSGPU_OK) return rcb; }
  const int N = f->N;
  const ResampleState &S = f->rs;
  HIPCHK(hipMemsetAsync(S.w + RCW_WALK_MAX, 0, sizeof(int), f->stream));
  birth_walk_levels_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(S, N, 1, f->dInhParent, f->dInhLevel);
  birth_inherit_kernel<0><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
  birth_inherit_kernel<1><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
  launch_predict_kernels(f, 1, BirthLevel{f->dInhLevel, 0, 1});
  for (int L = 1; L <= RFSGPU_RBPHD_WALK_LEVELS; L++) {
    birth_inherit_kernel<2><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, L);
    launch_predict_kernels(f, 1, BirthLevel{f->dInhLevel, L, 0});
  }
  const int first = RFSGPU_RBPHD_WALK_LEVELS + 1;
  if (f->D == 3) birth_walk_tail_kernel<3, false><<<1, BIRTH_TAIL_WAVES * 64, 0, f->stream>>>(f->B, f->P, f->cur, f->nZ, S, f->dInhParent, f->dInhLevel, first);
  else if (f->cfg.birthGaussianMeasurementCountThreshold != 1u) birth_walk_tail_kernel<2, false><<<1, BIRTH_TAIL_WAVES * 64, 0, f->stream>>>(f->B, f->P, f->cur, f->nZ, S, f->dInhParent, f->dInhLevel, first);
  else birth_walk_tail_kernel<2, true><<<1, BIRTH_TAIL_WAVES * 64, 0, f->stream>>>(f->B, f->P, f->cur, f->nZ, S, f->dInhParent, f->dInhLevel, first);
  f->candUsed = f->candUsed || f->D == 3 || f->cfg.birthGaussianMeasurementCountThreshold != 1u;
  return RFSGPU_OK;
}

// RBPHDFilter::predict's map part.  In the predicts that follow a resampling (resampleOccured_, RFSGPU_INHERIT_REFERENCE) the
// reference's slot-ordered lazy copy of unused_measurements_ / birthGaussians_ (RBPHDFilter.hpp:1005-1011) precedes each slot's
// birth step: see birth_inherit_kernel (birth.h) for how the walk is cut into levels.
static int predict_launch(rfsgpu_filter *f, int add_birth) {
  const BirthLevel all{nullptr, 0, 1};
  if (add_birth && rc_only_pending(f) && f->inheritMode == RFSGPU_INHERIT_REFERENCE && !f->fastSlamHandle) return predict_walk_device(f);
  if (!(add_birth && f->resampleOccured && f->inheritMode == RFSGPU_INHERIT_REFERENCE && !f->fastSlamHandle) || rc_only_pending(f)) {
    launch_predict_kernels(f, add_birth, all);
    return RFSGPU_OK;
  }
  ensure_ids(f);
  const int N = f->N;
  bool any = false;
  int maxLevel = 0;
  f->hInhParent.resize(N);
  f->hInhLevel.resize(N);
  for (int i = 0; i < N; i++) {
    int p = f->ppid[i];
    if (p < 0 || p >= N) p = i;     // (an id beyond the current particle count: a slot the reference would index out of range)
    f->hInhParent[i] = p;
    f->hInhLevel[i] = (p >= i) ? 0 : f->hInhLevel[p] + 1;
    any |= p != i;
    if (f->hInhLevel[i] > maxLevel) maxLevel = f->hInhLevel[i];
  }
  if (!any) { launch_predict_kernels(f, add_birth, all); return RFSGPU_OK; }
  { const int rcb = inherit_buffers(f); if (rcb != RFSGPU_OK) return rcb; }
  // (pageable host vectors: hipMemcpyAsync from them returns after the copy has been staged, so they may be reused at once)
  HIPCHK(hipMemcpyAsync(f->dInhParent, f->hInhParent.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->dInhLevel, f->hInhLevel.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, f->stream));
  birth_inherit_kernel<0><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
  birth_inherit_kernel<1><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
  launch_predict_kernels(f, add_birth, BirthLevel{f->dInhLevel, 0, 1});
  for (int L = 1; L <= maxLevel; L++) {
    birth_inherit_kernel<2><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, L);
    launch_predict_kernels(f, add_birth, BirthLevel{f->dInhLevel, L, 0});
  }
  f->candUsed = f->candUsed || f->D == 3 || f->cfg.birthGaussianMeasurementCountThreshold != 1u;
  return RFSGPU_OK;
}

// One level of the level-ordered birth step, for hosts that move the per-slot birth lists between shards themselves (rfsgpu.h).
int rfsgpu_predict_map_level(rfsgpu_filter *f, int add_birth, const int *level_of_slot, int level, int do_static) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_predict_map_level", ON_BATCH);
  if (!level_of_slot) return fail(f, RFSGPU_ERR_INVALID, "predict_map_level: null level array");
  f->externalAck = true;
  hipSetDevice(f->device);
  if (!f->dInhLevel) HIPCHK(hipMalloc(&f->dInhLevel, (size_t)f->Ncap * sizeof(int)));
  f->hInhLevel.assign(level_of_slot, level_of_slot + f->N);
  HIPCHK(hipMemcpyAsync(f->dInhLevel, f->hInhLevel.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipEventRecord(f->ev[EV_P0], f->stream));
  launch_predict_kernels(f, add_birth, BirthLevel{f->dInhLevel, level, do_static ? 1 : 0});
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[EV_P1], f->stream));
  const int rc = check_device_errors(f);
  accumulate(f->ev[EV_P0], f->ev[EV_P1], f->timing.predict_wall, nullptr);
  f->candUsed = f->candUsed || f->D == 3 || f->cfg.birthGaussianMeasurementCountThreshold != 1u;
  return rc;
}

int rfsgpu_predict_map(rfsgpu_filter *f, int add_birth) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_predict_map", ON_BATCH);
  if (add_birth && f->resampleOccured && f->inheritMode == RFSGPU_INHERIT_EXTERNAL && !f->externalAck)
    return fail(f, RFSGPU_ERR_INVALID, "predict_map with births after a resampling in RFSGPU_INHERIT_EXTERNAL mode, but the host has not applied the "
                "inheritance rule (rfsgpu_set_unused_masks, rfsgpu_predict_map_level, or rfsgpu_set_birth_inheritance(EXTERNAL) again to acknowledge): "
                "go through the multi-GPU host's own predict (ShardedRBPHDFilter.predict_map / rfsgpu_group_predict_map)");
  long long t0 = now_ns();
  hipSetDevice(f->device);
  HIPCHK(hipEventRecord(f->ev[EV_P0], f->stream));
  { const int rcl = predict_launch(f, add_birth); if (rcl != RFSGPU_OK) return rcl; }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[EV_P1], f->stream));
  int rc = check_device_errors(f);
  accumulate(f->ev[EV_P0], f->ev[EV_P1], f->timing.predict_wall, nullptr);
  f->timing.predict_cpu += now_ns() - t0;
  return rc;
}

// RBPHDFilter::predict's map part without the error-word readback: stream-ordered, errors surface at the next synchronising call.
int rfsgpu_predict_map_async(rfsgpu_filter *f, int add_birth) {
  if (f && rc_only_pending(f)) { }                                    // behind pending RB-PHD cycles the births walk the ids on the device (predict_walk_device)
  else if (add_birth) { CHECK_HANDLE(f); } else { CHECK_HANDLE_ENQ(f); }   // (the births read the ids and resampleOccured)
  if (f->batch) return refuse_on_kind(f, "rfsgpu_predict_map_async", ON_BATCH);
  if (add_birth && !f->rcPending && f->resampleOccured && f->inheritMode == RFSGPU_INHERIT_EXTERNAL && !f->externalAck)
    return fail(f, RFSGPU_ERR_INVALID, "predict_map with births after a resampling in RFSGPU_INHERIT_EXTERNAL mode, but the host has not applied the "
                "inheritance rule (rfsgpu_set_unused_masks, rfsgpu_predict_map_level, or rfsgpu_set_birth_inheritance(EXTERNAL) again to acknowledge): "
                "go through the multi-GPU host's own predict (ShardedRBPHDFilter.predict_map / rfsgpu_group_predict_map)");
  long long t0 = now_ns();
  hipSetDevice(f->device);
  if (f->predPending && hipEventQuery(f->ev[EV_P1]) == hipSuccess) {   // the previous async predict has long finished: book it
    accumulate(f->ev[EV_P0], f->ev[EV_P1], f->timing.predict_wall, nullptr);
    f->predPending = false;
  }
  const bool rec = !f->predPending;
  if (rec) HIPCHK(hipEventRecord(f->ev[EV_P0], f->stream));
  { const int rcl = predict_launch(f, add_birth); if (rcl != RFSGPU_OK) return rcl; }
  HIPCHK(hipGetLastError());
  if (rec) { HIPCHK(hipEventRecord(f->ev[EV_P1], f->stream)); f->predPending = true; }
  f->timing.predict_cpu += now_ns() - t0;
  return RFSGPU_OK;
}

// A run of `n` predicts that add no births, in one launch (birth.h, static_steps_kernel): the same bits as n calls of
// rfsgpu_set_lmk_process_noise(Q_k) + rfsgpu_predict_map_async(f, 0).  noises: [n][D*D] row-major, or NULL = the noise that is set
// now, n times.  Stream-ordered.
int rfsgpu_static_steps_async(rfsgpu_filter *f, int n, const double *noises) {
  if (f && batch_is_vp_mh(f)) {     // a batch of Victoria Park multi-hypothesis filters: behind its cycles, the counts and overflow words read on the device
    if (n < 0) return fail(f, RFSGPU_ERR_INVALID, "static_steps: negative count");
    hipSetDevice(f->device);
    FsCycleState S0;
    mhb_state(f->mhbBlock, f->nF, f->nPer, 0, S0);
    for (int k0 = 0; k0 < n; k0 += STATIC_RUN_MAX) {
      StaticRun R;
      R.n = std::min(STATIC_RUN_MAX, n - k0);
      for (int r = 0; r < R.n; r++) {
        const double *Q = noises ? noises + (size_t)(k0 + r) * 9 : f->Qlm;
        R.q[r][0] = Q[0]; R.q[r][1] = Q[1]; R.q[r][2] = Q[2]; R.q[r][3] = Q[4]; R.q[r][4] = Q[5]; R.q[r][5] = Q[8];
      }
      static_steps_guard_kernel<3, 4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, R, f->nPer, S0.w, FSC_WORDS, FSC_N, FSC_OVF);
      HIPCHK(hipGetLastError());
    }
    return RFSGPU_OK;
  }
  CHECK_HANDLE_BEHIND_CYCLE(f, behind);
  if (n < 0) return fail(f, RFSGPU_ERR_INVALID, "static_steps: negative count");
  hipSetDevice(f->device);
  const int D = f->D;
  for (int k0 = 0; k0 < n; k0 += STATIC_RUN_MAX) {
    StaticRun R;
    R.n = std::min(STATIC_RUN_MAX, n - k0);
    for (int r = 0; r < R.n; r++) {
      const double *Q = noises ? noises + (size_t)(k0 + r) * D * D : f->Qlm;
      if (D == 2) { R.q[r][0] = Q[0]; R.q[r][1] = Q[1]; R.q[r][2] = Q[3]; R.q[r][3] = R.q[r][4] = R.q[r][5] = 0.0; }
      else { R.q[r][0] = Q[0]; R.q[r][1] = Q[1]; R.q[r][2] = Q[2]; R.q[r][3] = Q[4]; R.q[r][4] = Q[5]; R.q[r][5] = Q[8]; }
    }
    if (behind) {
      const LiveCount live{f->mhc.w + FSC_N, f->mhc.w + FSC_OVF};
      if (D == 3) static_steps_live_kernel<3, 4><<<(f->Ncap + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, R, f->Ncap, live);
      else static_steps_live_kernel<2, 4><<<(f->Ncap + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, R, f->Ncap, live);
    }
    else if (D == 3) static_steps_kernel<3, 4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, R);
    else static_steps_kernel<2, 4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, R);
    HIPCHK(hipGetLastError());
  }
  return RFSGPU_OK;
}

// ParticleFilter::propagate for the Ackerman model on the device (motion.h): stream-ordered, no host wait.  u = {speed,
// steering}, var = their noise variances (null or zeros: noise-free), geom = {h, l, dx, dy}; (seed, call) key the generator.
int rfsgpu_propagate_ackerman_async(rfsgpu_filter *f, const double *u, const double *var, double dt, const double *geom, unsigned long long seed,
                                    unsigned long long call) {
  CHECK_HANDLE_BEHIND_CYCLE(f, behind);
  if (!u || !geom || !(dt == dt)) return fail(f, RFSGPU_ERR_INVALID, "propagate_ackerman: bad arguments");
  if (var && (var[0] < 0 || var[1] < 0)) return fail(f, RFSGPU_ERR_INVALID, "propagate_ackerman: negative variance");
  hipSetDevice(f->device);
  AckermanStep A;
  A.uv = u[0]; A.ur = u[1];
  A.sv = var ? std::sqrt(var[0]) : 0.0; A.sr = var ? std::sqrt(var[1]) : 0.0;
  A.dt = dt;
  A.h = geom[0]; A.l = geom[1]; A.dx = geom[2]; A.dy = geom[3];
  A.seed = seed; A.call = call;
  if (behind) propagate_ackerman_live_kernel<<<(f->Ncap + 255) / 256, 256, 0, f->stream>>>(f->B.pose, f->Ncap, A, LiveCount{f->mhc.w + FSC_N, f->mhc.w + FSC_OVF});
  else propagate_ackerman_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.pose, f->N, A);
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}

// A run of n propagations (consecutive odometry messages) in one launch: u [n][2], var [n][2] or NULL, dt [n]; the calls are
// numbered call0, call0 + 1, ...  Same poses, bit for bit, as n calls of rfsgpu_propagate_ackerman_async.
int rfsgpu_propagate_ackerman_run_async(rfsgpu_filter *f, int n, const double *u, const double *var, const double *dt, const double *geom,
                                        unsigned long long seed, unsigned long long call0) {
  CHECK_HANDLE_BEHIND_CYCLE(f, behind);
  if (n < 0 || (n > 0 && (!u || !dt || !geom))) return fail(f, RFSGPU_ERR_INVALID, "propagate_ackerman_run: bad arguments");
  for (int k = 0; k < n; k++)
    if (!(dt[k] == dt[k]) || (var && (var[2 * k] < 0 || var[2 * k + 1] < 0))) return fail(f, RFSGPU_ERR_INVALID, "propagate_ackerman_run: bad interval / negative variance");
  hipSetDevice(f->device);
  for (int k0 = 0; k0 < n; k0 += ACKERMAN_RUN_MAX) {
    AckermanRun R;
    R.n = std::min(ACKERMAN_RUN_MAX, n - k0);
    for (int r = 0; r < R.n; r++) {
      const int k = k0 + r;
      R.uv[r] = u[2 * k]; R.ur[r] = u[2 * k + 1];
      R.sv[r] = var ? std::sqrt(var[2 * k]) : 0.0; R.sr[r] = var ? std::sqrt(var[2 * k + 1]) : 0.0;
      R.dt[r] = dt[k];
    }
    R.h = geom[0]; R.l = geom[1]; R.dx = geom[2]; R.dy = geom[3];
    R.seed = seed; R.call0 = call0 + (unsigned long long)k0;
    if (behind) propagate_ackerman_run_live_kernel<<<(f->Ncap + 255) / 256, 256, 0, f->stream>>>(f->B.pose, f->Ncap, R, LiveCount{f->mhc.w + FSC_N, f->mhc.w + FSC_OVF});
    else propagate_ackerman_run_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.pose, f->N, R);
    HIPCHK(hipGetLastError());
  }
  return RFSGPU_OK;
}

// Everything a step consumes from the host in ONE stream-ordered call: poses (+ covariance) and, for the Victoria Park model,
// the laser scan (MeasurementModel_VictoriaPark::setLaserScan, src/MeasurementModel_VictoriaPark.cpp:267-281).  The caller's
// buffers are copied into a pinned staging ring before the call returns; the host never waits for the device (except when all
// four ring slots are still in flight).  x may be null (poses unchanged), scan may be null (scan unchanged / 2-D model).
int rfsgpu_set_step_inputs_async(rfsgpu_filter *f, const double *x, const double *cov, int cov_stride, const double *scan, int n_scan) {
  if (x) { CHECK_HANDLE_ENQ(f); }      // (poses size a host buffer by N)
  else { CHECK_HANDLE_BEHIND_CYCLE(f, behind); (void)behind; }   // a scan alone goes behind pending cycles: nothing below reads N
  if (cov && cov_stride != 0 && cov_stride != 9) return fail(f, RFSGPU_ERR_INVALID, "set_step_inputs: cov_stride must be 0 or 9");
  if (scan && (f->model != RFSGPU_MODEL_VICTORIAPARK_3D || n_scan < 2 || n_scan > RFSGPU_VP_MAX_SCAN)) return fail(f, RFSGPU_ERR_INVALID, "set_step_inputs: laser scan needs the Victoria Park model and 2..RFSGPU_VP_MAX_SCAN beams");
  if (!x && !scan) return RFSGPU_OK;
  hipSetDevice(f->device);
  double *h = nullptr;
  int k = 0;
  { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
  if (x) {
    f->bBirthAlt = false;   // (a batch: poses set after rfsgpu_batch_propagate_async are the ones the next predict's births happen at, as on the host route)
    { const int rc = push_poses(f, h, f->B.pose, x, cov, cov_stride); if (rc != RFSGPU_OK) return rc; }
    f->P.poseCovStride = cov ? cov_stride : 0;
  }
  if (scan) { const int rc = push_scan(f, h + (size_t)f->Ncap * 22, scan, n_scan); if (rc != RFSGPU_OK) return rc; }
  HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
  return RFSGPU_OK;
}
// setLaserScan through hs, the scan's place in a block of the pinned ring: the FoV area and the clutter density on the host, the raw
// scan to the device by a stream-ordered copy
static int push_scan(rfsgpu_filter *f, double *hs, const double *scan, int n_scan) {
  scan_clutter(f, scan, n_scan);
  memcpy(hs, scan, (size_t)n_scan * sizeof(double));
  HIPCHK(hipMemcpyAsync(f->B.scan, hs, (size_t)n_scan * sizeof(double), hipMemcpyHostToDevice, f->stream));
  f->B.nScan = n_scan;
  rebuild_params(f);
  return RFSGPU_OK;
}

int rfsgpu_get_unused(rfsgpu_filter *f, int slot, int *idx, int max_n, int *n_out) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  unsigned long long m = 0;
  HIPCHK(hipMemcpyAsync(&m, f->B.unusedMask + slot, sizeof(m), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  int k = 0;
  for (int z = 0; z < 64; z++)
    if ((m >> z) & 1ull) { if (k < max_n && idx) idx[k] = z; k++; }
  if (n_out) *n_out = k;
  return RFSGPU_OK;
}
int rfsgpu_landmarks_in_fov(rfsgpu_filter *f, int slot, int *n_out) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->N || !n_out) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(n_out, f->B.nInFov + slot, sizeof(int), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

// ---- weights / resampling ---------------------------------------------------------------------------

int rfsgpu_weight_sums_async(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_weight_sums_async", ON_BATCH);
  hipSetDevice(f->device);
  weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, f->N, f->dSums);
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
void *rfsgpu_weight_sums_device_ptr(rfsgpu_filter *f) { return f ? (void *)f->dSums : nullptr; }
int rfsgpu_weight_sums(rfsgpu_filter *f, double *out) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_weight_sums (use rfsgpu_batch_weight_sums)", ON_BATCH);
  int rc = rfsgpu_weight_sums_async(f);
  if (rc != RFSGPU_OK) return rc;
  HIPCHK(hipMemcpyAsync(f->hSums, f->dSums, 2 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  out[0] = f->hSums[0];
  out[1] = f->hSums[1];
  return RFSGPU_OK;
}
int rfsgpu_normalize_weights(rfsgpu_filter *f, double sum, const void *sum_dev) { return rfsgpu_normalize_weights_parts(f, sum, sum_dev, 1); }
int rfsgpu_normalize_weights_parts(rfsgpu_filter *f, double sum, const void *sum_dev, int n_parts) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_normalize_weights", ON_BATCH);
  if (n_parts < 1) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  long long t0 = now_ns();
  HIPCHK(hipEventRecord(f->ev[EV_R0], f->stream));
  normalize_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, f->N, sum, (const double *)sum_dev, n_parts);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[EV_R1], f->stream));
  // stream-ordered, no host sync: the next call that syncs (or rfsgpu_synchronize) completes it; its event pair is
  // folded into the Resampling bucket by rfsgpu_get_timing
  f->normPending = true;
  f->timing.particleResample_cpu += now_ns() - t0;
  return RFSGPU_OK;
}
int rfsgpu_n_particles(const rfsgpu_filter *f) {
  if (!f) return -1;
  if (f->mhcPending || (f->rsPending && f->rsShrink)) {      // the count is on the device: take it over; an error of the pending cycles goes to the next call that returns a status
    rfsgpu_filter *g = const_cast<rfsgpu_filter *>(f);
    const int rc = mhc_resolve(g);
    if (rc != RFSGPU_OK) g->mhcStashedRc = rc;
  }
  return f->N;
}
int rfsgpu_max_particles(const rfsgpu_filter *f) { return f ? f->Ncap : -1; }
int rfsgpu_resample_apply(rfsgpu_filter *f, const int *src_slot) { return f ? rfsgpu_resample_apply_n(f, src_slot, f->N) : RFSGPU_ERR_INVALID; }
int rfsgpu_resample_apply_n(rfsgpu_filter *f, const int *src_slot, int n_out) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_resample_apply", ON_BATCH);
  if (f->rcHave) return fail(f, RFSGPU_ERR_UNSUPPORTED, "resample_apply: this handle runs rfsgpu_rbphd_cycle_async, which resamples inside the cycle and keeps the ids and the counters of its gate on the device");
  if (!src_slot || n_out < 1 || n_out > f->N) return RFSGPU_ERR_INVALID;
  const int nIn = f->N;
  for (int k = 0; k < n_out; k++) {
    const int s = src_slot[k];
    // a source is either a surviving slot that keeps itself or a slot beyond the new count (dropped after the copy)
    if (s < 0 || s >= nIn || (s < n_out && src_slot[s] != s)) return fail(f, RFSGPU_ERR_INVALID, "resample_apply: a source slot below the new count must keep itself");
  }
  f->N = n_out;
  f->B.N = n_out;
  // ids as ParticleFilter::resample leaves them (:446-479): a copy has its source's id (Particle::copy) and idParent_ = that id;
  // a slot that keeps its particle gets idParent_ = its own id (case 1).  Sources are never destinations, so in place is safe.
  ensure_ids(f);
  for (int k = 0; k < n_out; k++) {
    const int s = src_slot[k];
    if (s != k) { f->pid[k] = f->pid[s]; f->ppid[k] = f->pid[s]; }
    else f->ppid[k] = f->pid[k];
  }
  f->resampleOccured = true;
  f->externalAck = false;
  f->mhcIdsDirty = true;
  hipSetDevice(f->device);
  long long t0 = now_ns();
  // Round 6: stream-ordered.  The plan goes into a slot of the pinned staging ring (the caller's buffer is free when the call returns) and
  // the gather kernel reads it from there -- one 4-byte PCIe read per workgroup -- instead of a pageable host-to-device copy (staged and
  // waited for by the runtime), two timing events and a stream synchronisation: 125 -> 84 us per call at 2000 particles under the
  // unmodified 2-D driver.  Nothing after it needs the host to wait: every reader of the maps synchronises on the stream itself, the next
  // predict / update is ordered behind the gather.  TimingInfo's particleResample_wall books the host time of the call (the device part
  // overlaps whatever the host does next).  RFSGPU_RESAMPLE_SYNC=1 keeps the synchronous form (A/B).
  static const bool syncForm = [] { const char *e = getenv("RFSGPU_RESAMPLE_SYNC"); return e && atoi(e) != 0; }();
  if (syncForm) {
    HIPCHK(hipMemcpyAsync(f->dSrcSlot, src_slot, (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipEventRecord(f->ev[EV_R0], f->stream));
    resample_gather_kernel<<<f->N, 256, 0, f->stream>>>(f->B, f->cur, f->dSrcSlot, f->P.poseCovStride, map_only(f));
    set_weights_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, f->N, 1.0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(f->ev[EV_R1], f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    accumulate(f->ev[EV_R0], f->ev[EV_R1], f->timing.particleResample_wall, nullptr);
    f->timing.particleResample_cpu += now_ns() - t0;
    return RFSGPU_OK;
  }
  double *hs;
  int ks;
  int rc = ring_acquire(f, f->stage, &hs, &ks);
  if (rc != RFSGPU_OK) return rc;
  memcpy(hs, src_slot, (size_t)f->N * sizeof(int));
  resample_gather_kernel<<<f->N, 256, 0, f->stream>>>(f->B, f->cur, reinterpret_cast<const int *>(hs), f->P.poseCovStride, map_only(f));
  set_weights_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, f->N, 1.0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->stage.ev[ks], f->stream));      // the slot is free again once the gather has read it
  const long long dtn = now_ns() - t0;
  f->timing.particleResample_wall += dtn;
  f->timing.particleResample_cpu += dtn;
  return RFSGPU_OK;
}

int rfsgpu_set_birth_inheritance(rfsgpu_filter *f, int mode) {
  CHECK_HANDLE(f);
  if (mode != RFSGPU_INHERIT_REFERENCE && mode != RFSGPU_INHERIT_EAGER && mode != RFSGPU_INHERIT_EXTERNAL) return fail(f, RFSGPU_ERR_INVALID, "set_birth_inheritance: unknown mode");
  if (f->batch && mode != RFSGPU_INHERIT_REFERENCE) return fail(f, RFSGPU_ERR_UNSUPPORTED, "a filter batch keeps the reference birth inheritance (RFSGPU_INHERIT_REFERENCE) only");
  f->inheritMode = mode;
  f->externalAck = true;    // (EXTERNAL: the caller asserts that it owns the rule from here on, incl. for the coming predict)
  return RFSGPU_OK;
}
int rfsgpu_get_birth_inheritance(const rfsgpu_filter *f) { return f ? f->inheritMode : -1; }
int rfsgpu_get_particle_ids(rfsgpu_filter *f, int *id, int *parent_id) {
  CHECK_HANDLE(f);
  ensure_ids(f);
  if (f->bDevRoute) {      // (a batch that resamples on the device: the ids live there)
    hipSetDevice(f->device);
    HIPCHK(hipMemcpyAsync(f->pid.data(), f->BL.pid, (size_t)f->N * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipMemcpyAsync(f->ppid.data(), f->BL.ppid, (size_t)f->N * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
  }
  for (int k = 0; k < f->N; k++) { if (id) id[k] = f->pid[k]; if (parent_id) parent_id[k] = f->ppid[k]; }
  return RFSGPU_OK;
}
int rfsgpu_set_particle_ids(rfsgpu_filter *f, const int *id, const int *parent_id) {
  CHECK_HANDLE(f);
  ensure_ids(f);
  if (f->bDevRoute && (!id || !parent_id)) {      // the part that is not given stays what the device holds
    int rc = rfsgpu_get_particle_ids(f, nullptr, nullptr);
    if (rc != RFSGPU_OK) return rc;
  }
  for (int k = 0; k < f->N; k++) { if (id) f->pid[k] = id[k]; if (parent_id) f->ppid[k] = parent_id[k]; }
  f->mhcIdsDirty = true;
  if (batch_is_mh(f)) {      // (the ids live in the filters' cycle state on the device)
    FsCycleState S0;
    mhb_state(f->mhbBlock, f->nF, f->nPer, 0, S0);
    hipSetDevice(f->device);
    HIPCHK(hipMemcpyAsync(S0.pid, f->pid.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(S0.ppid, f->ppid.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
  }
  if (f->bDevRoute) {
    hipSetDevice(f->device);
    HIPCHK(hipMemcpyAsync(f->BL.pid, f->pid.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->BL.ppid, f->ppid.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
  }
  return RFSGPU_OK;
}
int rfsgpu_resample_occured(const rfsgpu_filter *f) {
  if (f && (f->rsPending || f->rcPending)) {  // the decision is on the device: take it over; an error goes to the next call that returns a status
    rfsgpu_filter *g = const_cast<rfsgpu_filter *>(f);
    const int rc = mhc_resolve(g);
    if (rc != RFSGPU_OK) g->mhcStashedRc = rc;
  }
  return (f && !f->batch) ? (f->resampleOccured ? 1 : 0) : -1;
}   // (a batch: rfsgpu_batch_resample_occured)
// every particle's pose covariance as the update reads it: [n_particles][9] row-major (one shared matrix is repeated)
int rfsgpu_get_pose_covs(rfsgpu_filter *f, double *cov) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_get_pose_covs (use rfsgpu_batch_get_pose_covs)", ON_BATCH);
  if (!cov) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  const bool per = f->P.poseCovStride == 9;
  HIPCHK(hipMemcpyAsync(cov, f->B.poseCov, (per ? (size_t)f->N * 9 : 9) * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  if (!per) for (int k = 1; k < f->N; k++) memcpy(cov + (size_t)9 * k, cov, 9 * sizeof(double));
  return RFSGPU_OK;
}
int rfsgpu_get_unused_masks(rfsgpu_filter *f, unsigned long long *masks) {
  CHECK_HANDLE(f);
  if (!masks) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(masks, f->B.unusedMask, (size_t)f->N * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;   // (a read acknowledges nothing: only set_unused_masks / predict_map_level / set_birth_inheritance do)
}
int rfsgpu_has_birth_candidates(const rfsgpu_filter *f) { return f ? (f->candUsed ? 1 : 0) : -1; }
int rfsgpu_set_unused_masks(rfsgpu_filter *f, const unsigned long long *masks) {
  CHECK_HANDLE(f);
  if (!masks) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(f->B.unusedMask, masks, (size_t)f->N * sizeof(unsigned long long), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  f->externalAck = true;
  return RFSGPU_OK;
}

// ---- cross-shard migration (multi-GPU resampling): packed rows in DEVICE buffers, stream-ordered, no host sync -----------
// candidates a migration row carries: the whole list for a filter that keeps one, nothing for a configuration that never does
static int row_cand(const rfsgpu_filter *f) {
  if (map_only(f)) return 0;   // a migrant carries what Particle::copy carries: pose + mixture
  return (f->model == RFSGPU_MODEL_VICTORIAPARK_3D || f->cfg.birthGaussianMeasurementCountThreshold != 1u || f->candUsed) ? RFSGPU_MAX_CANDIDATES : 0;
}
size_t rfsgpu_slab_row_bytes(const rfsgpu_filter *f) { return f ? slab_row_bytes(f->B.npl, f->cap, row_cand(f)) : 0; }
static int slab_rows(rfsgpu_filter *f, const int *slots, int n, void *dev_rows, bool exporting) {
  if (n == 0) return RFSGPU_OK;
  if (!slots || !dev_rows || n < 0) return fail(f, RFSGPU_ERR_INVALID, "slab rows: bad arguments");
  for (int k = 0; k < n; k++)
    if (slots[k] < 0 || slots[k] >= f->N) return fail(f, RFSGPU_ERR_INVALID, "slab rows: slot out of range");
  hipSetDevice(f->device);
  if (n > f->rowSlotsCap) {   // (a slot may be exported many times -- one heavy parent, many children elsewhere -- so n is not bounded by N)
    HIPCHK(hipStreamSynchronize(f->stream));
    if (f->dRowSlots) HIPCHK(hipFree(f->dRowSlots));
    f->dRowSlots = nullptr;
    f->rowSlotsCap = 0;
    const int want = std::max(n, f->Ncap);
    HIPCHK(hipMalloc(&f->dRowSlots, (size_t)want * sizeof(int)));
    f->rowSlotsCap = want;
  }
  HIPCHK(hipMemcpyAsync(f->dRowSlots, slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, f->stream));
  if (exporting) slab_rows_kernel<true><<<n, 256, 0, f->stream>>>(f->B, f->cur, f->dRowSlots, (unsigned char *)dev_rows, f->P.poseCovStride, row_cand(f), map_only(f));
  else slab_rows_kernel<false><<<n, 256, 0, f->stream>>>(f->B, f->cur, f->dRowSlots, (unsigned char *)dev_rows, f->P.poseCovStride, row_cand(f), map_only(f));
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
int rfsgpu_export_slab_rows(rfsgpu_filter *f, const int *slots, int n, void *dev_rows) {
  CHECK_HANDLE(f);
  return slab_rows(f, slots, n, dev_rows, true);
}
int rfsgpu_import_slab_rows(rfsgpu_filter *f, const int *slots, int n, const void *dev_rows) {
  CHECK_HANDLE(f);
  return slab_rows(f, slots, n, const_cast<void *>(dev_rows), false);
}
void *rfsgpu_weights_device_ptr(rfsgpu_filter *f) { return f ? (void *)f->B.weight : nullptr; }

// ---- timing / misc -----------------------------------------------------------------------------------

int rfsgpu_get_timing(rfsgpu_filter *f, rfsgpu_timing *t) {
  CHECK_HANDLE(f);
  if (!t) return RFSGPU_ERR_INVALID;
  if (f->normPending || f->predPending || f->ringCount > 0) {   // (steps whose results were delivered through pinned memory have not been harvested yet)
    hipSetDevice(f->device);
    HIPCHK(hipStreamSynchronize(f->stream));
    harvest_async(f);
    if (f->normPending) accumulate(f->ev[EV_R0], f->ev[EV_R1], f->timing.particleResample_wall, nullptr);
    if (f->predPending) accumulate(f->ev[EV_P0], f->ev[EV_P1], f->timing.predict_wall, nullptr);
    f->normPending = f->predPending = false;
  }
  *t = f->timing;
  return RFSGPU_OK;
}
int rfsgpu_reset_timing(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  memset(&f->timing, 0, sizeof(f->timing));
  return RFSGPU_OK;
}
int rfsgpu_synchronize(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  const int rc = check_device_errors(f);  // syncs the stream, reports errors of async steps
  harvest_async(f);
  return rc;
}
int rfsgpu_set_phase_timing(rfsgpu_filter *f, int on) {
  CHECK_HANDLE(f);
  f->phaseTiming = on != 0;
  return RFSGPU_OK;
}
void *rfsgpu_stream(rfsgpu_filter *f) { return f ? (void *)f->stream : nullptr; }
int rfsgpu_set_stream(rfsgpu_filter *f, void *hip_stream) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  f->stream = hip_stream ? (hipStream_t)hip_stream : f->ownStream;
  return RFSGPU_OK;
}
int rfsgpu_bind_weight_sums_buffer(rfsgpu_filter *f, void *dev_ptr) {
  CHECK_HANDLE(f);
  f->dSums = dev_ptr ? (double *)dev_ptr : f->ownSums;
  return RFSGPU_OK;
}

int rfsgpu_save_state(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  const size_t slabBytes = (size_t)f->Ncap * f->B.npl * f->cap * sizeof(double);
  if (!f->snapSlab) {
    bool ok = true;
    ok &= hipMalloc(&f->snapSlab, slabBytes) == hipSuccess;
    ok &= hipMalloc(&f->snapWeight, f->Ncap * sizeof(double)) == hipSuccess;
    ok &= hipMalloc(&f->snapCount, f->Ncap * sizeof(int)) == hipSuccess;
    ok &= hipMalloc(&f->snapFov, f->Ncap * sizeof(int)) == hipSuccess;
    ok &= hipMalloc(&f->snapUnused, f->Ncap * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
      hipFree(f->snapSlab); hipFree(f->snapWeight); hipFree(f->snapCount); hipFree(f->snapFov); hipFree(f->snapUnused);
      f->snapSlab = nullptr; f->snapWeight = nullptr; f->snapCount = nullptr; f->snapFov = nullptr; f->snapUnused = nullptr;
      return fail(f, RFSGPU_ERR_HIP, "save_state: out of device memory");
    }
  }
  HIPCHK(hipMemcpyAsync(f->snapSlab, f->B.slab[f->cur], slabBytes, hipMemcpyDeviceToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->snapWeight, f->B.weight, f->N * sizeof(double), hipMemcpyDeviceToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->snapCount, f->B.count, f->N * sizeof(int), hipMemcpyDeviceToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->snapFov, f->B.nInFov, f->N * sizeof(int), hipMemcpyDeviceToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->snapUnused, f->B.unusedMask, f->N * sizeof(unsigned long long), hipMemcpyDeviceToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  f->snapNZ = f->nZ;
  f->snapN = f->N;
  return RFSGPU_OK;
}
int rfsgpu_restore_state(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (!f->snapSlab) return fail(f, RFSGPU_ERR_INVALID, "restore_state: nothing saved");
  hipSetDevice(f->device);
  f->N = f->snapN;  // (the particle count is part of the state: the multi-hypothesis FastSLAM update changes it)
  f->B.N = f->N;
  // only the live entries are copied (one block per particle); asynchronous on the handle's stream
  if (f->B.npl == 7) restore_state_kernel<7><<<f->N, 256, 0, f->stream>>>(f->B, f->cur, f->snapSlab, f->snapWeight, f->snapCount, f->snapFov, f->snapUnused);
  else restore_state_kernel<11><<<f->N, 256, 0, f->stream>>>(f->B, f->cur, f->snapSlab, f->snapWeight, f->snapCount, f->snapFov, f->snapUnused);
  HIPCHK(hipGetLastError());
  f->nZ = f->snapNZ;
  return RFSGPU_OK;
}
// ---- ring of pre-seeded states (bench.py): the input of a timed step is resident BEFORE the timed region -----------------------
// rfsgpu_restore_state inside a timed loop is a 45 MB copy per step at configs[1] (restore_state_kernel 8.8 us of a 124 us step) that
// is not part of the path.  Instead: n slots, each a full copy of what restore_state writes (slab, particle weights, sizes, FOV
// counts, unused lists), filled from the snapshot once; rfsgpu_state_ring_next swaps the handle's current-state pointers with the
// next slot's -- host work only, nothing is launched.  A slot is consumed by the step that runs on it (the map update works in
// place); rfsgpu_state_ring_seed fills all of them again.
static void ring_seed_slot(rfsgpu_filter *f, rfsgpu_filter::RingSlot &r) {
  Buffers Bs = f->B;
  Bs.slab[f->cur] = r.slab; Bs.weight = r.weight; Bs.count = r.count; Bs.nInFov = r.fov; Bs.unusedMask = r.unused;
  Bs.N = f->snapN;
  if (f->B.npl == 7) restore_state_kernel<7><<<f->snapN, 256, 0, f->stream>>>(Bs, f->cur, f->snapSlab, f->snapWeight, f->snapCount, f->snapFov, f->snapUnused);
  else restore_state_kernel<11><<<f->snapN, 256, 0, f->stream>>>(Bs, f->cur, f->snapSlab, f->snapWeight, f->snapCount, f->snapFov, f->snapUnused);
}
int rfsgpu_state_ring_seed(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (!f->snapSlab || f->stateRing.empty()) return fail(f, RFSGPU_ERR_INVALID, "state_ring_seed: no snapshot / no ring");
  hipSetDevice(f->device);
  for (auto &r : f->stateRing) ring_seed_slot(f, r);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(f->stream));
  f->stateRingPos = 0;
  return RFSGPU_OK;
}
int rfsgpu_state_ring_create(rfsgpu_filter *f, int n_slots) {
  CHECK_HANDLE(f);
  if (!f->snapSlab) return fail(f, RFSGPU_ERR_INVALID, "state_ring_create: rfsgpu_save_state first");
  if (n_slots < 0) return fail(f, RFSGPU_ERR_INVALID, "state_ring_create: negative slot count");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  const size_t slabBytes = (size_t)f->Ncap * f->B.npl * f->cap * sizeof(double);
  while ((int)f->stateRing.size() > n_slots) {
    auto &r = f->stateRing.back();
    hipFree(r.slab); hipFree(r.weight); hipFree(r.count); hipFree(r.fov); hipFree(r.unused);
    f->stateRing.pop_back();
  }
  while ((int)f->stateRing.size() < n_slots) {
    rfsgpu_filter::RingSlot r;
    bool ok = true;
    ok &= hipMalloc(&r.slab, slabBytes) == hipSuccess;
    ok &= hipMalloc(&r.weight, f->Ncap * sizeof(double)) == hipSuccess;
    ok &= hipMalloc(&r.count, f->Ncap * sizeof(int)) == hipSuccess;
    ok &= hipMalloc(&r.fov, f->Ncap * sizeof(int)) == hipSuccess;
    ok &= hipMalloc(&r.unused, f->Ncap * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
      hipFree(r.slab); hipFree(r.weight); hipFree(r.count); hipFree(r.fov); hipFree(r.unused);
      (void)hipGetLastError();
      return fail(f, RFSGPU_ERR_HIP, "state_ring_create: out of device memory");
    }
    // (rows beyond the live entries are never read before they are written; the small arrays are written in full by the seed)
    f->stateRing.push_back(r);
  }
  return n_slots > 0 ? rfsgpu_state_ring_seed(f) : RFSGPU_OK;
}
int rfsgpu_state_ring_next(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  if (f->stateRing.empty()) return fail(f, RFSGPU_ERR_INVALID, "state_ring_next: no ring");
  if (f->stateRingPos >= f->stateRing.size()) return fail(f, RFSGPU_ERR_INVALID, "state_ring_next: every slot has been consumed (rfsgpu_state_ring_seed fills them again)");
  auto &r = f->stateRing[f->stateRingPos++];
  std::swap(f->B.slab[f->cur], r.slab);
  std::swap(f->B.weight, r.weight);
  std::swap(f->B.count, r.count);
  std::swap(f->B.nInFov, r.fov);
  std::swap(f->B.unusedMask, r.unused);
  f->N = f->snapN;
  f->B.N = f->N;
  f->nZ = f->snapNZ;
  return RFSGPU_OK;
}
int rfsgpu_last_step_variant(const rfsgpu_filter *f, int *out4) {
  if (!f || !out4) return RFSGPU_ERR_INVALID;
  for (int k = 0; k < 4; k++) out4[k] = f->lastStepVariant[k];
  return RFSGPU_OK;
}
int rfsgpu_last_kernel_ns(rfsgpu_filter *f, long long *ns4) {
  CHECK_HANDLE(f);
  if (!ns4) return RFSGPU_ERR_INVALID;
  for (int k = 0; k < 4; k++) ns4[k] = f->lastKernelNs[k];
  return RFSGPU_OK;
}

#ifdef RFS_PROFILE
// tuning builds only (not declared in rfsgpu.h): 64 s_memtime stamps of one particle's last kernels
int rfsgpu_debug_sections(rfsgpu_filter *f, long long *out64) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  if (!f->B.dbg) {
    HIPCHK(hipMalloc(&f->B.dbg, (64 + 8 * (size_t)f->Ncap) * sizeof(long long)));
    HIPCHK(hipMemset(f->B.dbg, 0, (64 + 8 * (size_t)f->Ncap) * sizeof(long long)));
  }
  HIPCHK(hipMemcpy(out64, f->B.dbg, 64 * sizeof(long long), hipMemcpyDeviceToHost));
  return RFSGPU_OK;
}
// four counters per particle written by the last instrumented kernel (see the RFS_PROFILE blocks in the kernels)
int rfsgpu_debug_per_particle(rfsgpu_filter *f, long long *out4n) {
  CHECK_HANDLE(f);
  if (!f->B.dbg) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpy(out4n, f->B.dbg + 64, 4 * (size_t)f->N * sizeof(long long), hipMemcpyDeviceToHost));
  return RFSGPU_OK;
}
// second block of four: the fused step kernel's phase clock per particle (start, after map update, after weighting, end)
int rfsgpu_debug_per_particle_fused(rfsgpu_filter *f, long long *out4n) {
  CHECK_HANDLE(f);
  if (!f->B.dbg) return RFSGPU_ERR_INVALID;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpy(out4n, f->B.dbg + 64 + 4 * (size_t)f->N, 4 * (size_t)f->N * sizeof(long long), hipMemcpyDeviceToHost));
  return RFSGPU_OK;
}
#endif

// ---- FastSLAM 1.0 (include/FastSLAM.hpp) on the same handle ----------------------------------------------------------
void rfsgpu_default_fastslam_config(rfsgpu_fastslam_config *c) {  // constructor defaults, :243-257 (nParticlesMax = 3n is set per handle)
  if (!c) return;
  c->minUpdatesBeforeResample = 1;
  c->minMeasurementsBeforeResample = 1;
  c->landmarkExistencePrior = 0.5;
  c->mapExistencePruneThreshold = -3.0;
  c->minLogMeasurementLikelihood = -10.0;
  c->nParticlesMax = 0;
  c->maxNDataAssocHypotheses = 1;
  c->maxDataAssocLogLikelihoodDiff = 5;
  c->landmarkCandidateMeasurementSupportDist = 1;
  c->landmarkCandidateMeasurementCountThreshold = 1;
  c->landmarkCandidateCurrentMeasurementCountThreshold = 1;
  c->landmarkCandidateMeasurementCheckThreshold = 2;
  c->landmarkLockWeight = 10;
  c->pruningMeasurementsThreshold = 0;
}
int rfsgpu_set_fastslam_config(rfsgpu_filter *f, const rfsgpu_fastslam_config *cfg) {
  CHECK_HANDLE_HOST(f);
  if (f->batch) return refuse_on_kind(f, "FastSLAM", ON_BATCH);
  if (!cfg) return RFSGPU_ERR_INVALID;
  f->fs = *cfg;
  return RFSGPU_OK;
}
int rfsgpu_get_fastslam_config(const rfsgpu_filter *f, rfsgpu_fastslam_config *cfg) {
  if (!f || !cfg) return RFSGPU_ERR_INVALID;
  *cfg = f->fs;
  return RFSGPU_OK;
}
// (one expression for a handle and for every filter of a batch: a filter's bits do not depend on being in a batch)
// clutterIntensityIntegral(nZ) (:561-562): c * sensing area (RngBrg.cpp:175-178) or the expected clutter number (VictoriaPark).  One
// function for the host-fed records and the sensed cycle's template (fastslam_sensed.h), whose kernel does the division below.
static double fs_pfa_num(const Params &P, int D) { return (D == 2) ? P.clutter * (2 * RFS_PI * (P.rmax - P.rmin)) : P.vpExpClutter; }
static FsParams fs_params_of(const rfsgpu_fastslam_config &fs, const Params &P, int D, int n_z) {
  FsParams F;
  F.prior = fs.landmarkExistencePrior;
  F.minLog = fs.minLogMeasurementLikelihood;
  F.lockW = fs.landmarkLockWeight;
  F.pfa = fs_pfa_num(P, D) / n_z;     // clutterIntensityIntegral(nZ) / nZ
  F.newW = log(F.prior / (1 - F.prior));
  F.supportD2 = fs.landmarkCandidateMeasurementSupportDist * fs.landmarkCandidateMeasurementSupportDist;
  F.countThr = fs.landmarkCandidateMeasurementCountThreshold;
  F.curThr = fs.landmarkCandidateCurrentMeasurementCountThreshold;
  F.checkThr = fs.landmarkCandidateMeasurementCheckThreshold;
  return F;
}
static FsParams fs_params(const rfsgpu_filter *f, int n_z) {
  const FsParams F = fs_params_of(f->fs, f->P, f->D, n_z);
  if (F.countThr != 1u) const_cast<rfsgpu_filter *>(f)->candUsed = true;   // (migration rows carry the lists from now on)
  return F;
}
// prune by the existence threshold (:611-612) + new landmarks / candidates (:615-690) over all f->N particles
static int fastslam_map_management(rfsgpu_filter *f, const FsParams &F, int n_z) {
  int rc;
  if ((unsigned)n_z >= f->fs.pruningMeasurementsThreshold) {
    Params Pp = f->P;
    Pp.pruneT = f->fs.mapExistencePruneThreshold;
    const size_t pb = gm_prune_lds_bytes_per_wave(f->cap);
    if ((rc = set_lds(f, (gm_prune_kernel<4, false>), 4 * pb)) != RFSGPU_OK) return rc;
    gm_prune_kernel<4, false><<<(f->N + 3) / 4, 256, 4 * pb, f->stream>>>(f->B, Pp, f->cur, f->cur ^ 1);
    HIPCHK(hipGetLastError());
    f->cur ^= 1;
  }
  if (f->D == 2) fs_new_landmarks_kernel<2><<<(f->N + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z);
  else fs_new_landmarks_kernel<3><<<(f->N + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z);
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
// Multi-hypothesis update (fastslam_mh.h).  Host part: the slots of the particle copies, in particle order.
static int fastslam_update_mh(rfsgpu_filter *f, const double *z, int n_z) {
  if (f->D == 3 && f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "Victoria Park model: rfsgpu_set_laser_scan must precede the update");
  int rc = stage_measurements(f, z, n_z);
  if (rc != RFSGPU_OK) return rc;
  hipSetDevice(f->device);
  const long long t0 = now_ns();
  const FsMhLayout L = fs_mh_layout();
  if (!f->mhArena) HIPCHK(hipMalloc(&f->mhArena, (size_t)f->Ncap * L.total));
  if (!f->mhInts) HIPCHK(hipMalloc(&f->mhInts, (size_t)5 * f->Ncap * sizeof(int)));
  const FsParams F = fs_params(f, n_z);
  const int N0 = f->N, kmax = (int)f->fs.maxNDataAssocHypotheses;
  HIPCHK(hipEventRecord(f->ev[EV_UM0], f->stream));
  if (f->D == 2) fs_mh_associate_kernel<2><<<N0, 64 * FSMH_WAVES, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, kmax, f->fs.maxDataAssocLogLikelihoodDiff, f->mhArena);
  else fs_mh_associate_kernel<3><<<N0, 64 * FSMH_WAVES, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, kmax, f->fs.maxDataAssocLogLikelihoodDiff, f->mhArena);
  HIPCHK(hipGetLastError());
  std::vector<int> nH(N0);
  HIPCHK(hipMemcpy2DAsync(nH.data(), sizeof(int), f->mhArena + L.offHdr + 2 * sizeof(int), L.total, sizeof(int), N0, hipMemcpyDeviceToHost, f->stream));
  if ((rc = check_device_errors(f)) != RFSGPU_OK) return rc;  // syncs
  // pi[0] = i; after particle i's nH - 1 copies were appended: pi[h] = nParticles_ - h (:543-556)
  std::vector<int> slotSrc(N0), slotHyp(N0), slotNH(N0), cDst, cSrc;
  int n = N0;
  for (int i = 0; i < N0; i++) { slotSrc[i] = i; slotHyp[i] = nH[i] > 0 ? 0 : -1; slotNH[i] = nH[i]; }
  for (int i = 0; i < N0; i++) {
    if (nH[i] <= 1) continue;
    const int first = n;
    n += nH[i] - 1;
    if (n > f->Ncap) return fail(f, RFSGPU_ERR_CAPACITY, "the particle copies of the multi-hypothesis update exceed max_particles (rfsgpu_create_ex)");
    slotSrc.resize(n); slotHyp.resize(n); slotNH.resize(n);
    for (int h = 1; h < nH[i]; h++) {
      const int slot = n - h;
      slotSrc[slot] = i; slotHyp[slot] = h; slotNH[slot] = nH[i];
      cDst.push_back(slot); cSrc.push_back(i);
    }
    (void)first;
  }
  int *dSlotSrc = f->mhInts, *dSlotHyp = dSlotSrc + f->Ncap, *dSlotNH = dSlotHyp + f->Ncap, *dDst = dSlotNH + f->Ncap, *dSrc = dDst + f->Ncap;
  HIPCHK(hipMemcpyAsync(dSlotSrc, slotSrc.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(dSlotHyp, slotHyp.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(dSlotNH, slotNH.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, f->stream));
  const int nNew = n - N0;
  if (nNew > 0) {
    HIPCHK(hipMemcpyAsync(dDst, cDst.data(), (size_t)nNew * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(dSrc, cSrc.data(), (size_t)nNew * sizeof(int), hipMemcpyHostToDevice, f->stream));
    fs_mh_copy_kernel<<<nNew, 256, 0, f->stream>>>(f->B, f->cur, dDst, dSrc, f->fsResampleOccured ? 1 : 0, f->P.poseCovStride);
    HIPCHK(hipGetLastError());
    f->N = n;
    f->B.N = n;
    fs_mh_split_weights_kernel<<<(n + 255) / 256, 256, 0, f->stream>>>(f->B.weight, dSlotSrc, dSlotNH, n, 0);
    fs_mh_split_weights_kernel<<<(n + 255) / 256, 256, 0, f->stream>>>(f->B.weight, dSlotSrc, dSlotNH, n, 1);
    HIPCHK(hipGetLastError());
  }
  if (f->D == 2) fs_mh_apply_kernel<2><<<n, 64, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, dSlotSrc, dSlotHyp, f->mhArena);
  else fs_mh_apply_kernel<3><<<n, 64, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, dSlotSrc, dSlotHyp, f->mhArena);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[EV_UM1], f->stream));
  if ((rc = fastslam_map_management(f, F, n_z)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_PR1], f->stream));
  f->parents = slotSrc;
  rc = check_device_errors(f);
  accumulate(f->ev[EV_UM0], f->ev[EV_UM1], f->timing.mapUpdate_wall, &f->lastKernelNs[0]);
  f->timing.mapUpdate_kf_wall = f->timing.mapUpdate_wall;
  accumulate(f->ev[EV_UM1], f->ev[EV_PR1], f->timing.mapPrune_wall, &f->lastKernelNs[3]);
  f->timing.mapUpdate_cpu += now_ns() - t0;
  return rc;
}
int rfsgpu_fastslam_set_resample_occured(rfsgpu_filter *f, int flag) {
  CHECK_HANDLE(f);
  f->fsResampleOccured = flag != 0;
  return RFSGPU_OK;
}
int rfsgpu_particle_parents(rfsgpu_filter *f, int *parent, int max_n) {
  CHECK_HANDLE(f);
  if (!parent || max_n < f->N) return RFSGPU_ERR_INVALID;
  for (int k = 0; k < f->N; k++) parent[k] = (k < (int)f->parents.size()) ? f->parents[k] : k;
  return RFSGPU_OK;
}
// ---- the whole FastSLAM::update on the device (fastslam_cycle.h) ------------------------------------------------------------------
// The particle count comes back: one stream-ordered copy of the cycle block into pinned memory, then the wait.  Cycles that an
// overflow abandoned did not prune, so the slab flips the host made for them are taken back.
static int mhb_resolve(rfsgpu_filter *f);
static int rs_resolve(rfsgpu_filter *f);
static int rc_resolve(rfsgpu_filter *f);
static int mhc_resolve(rfsgpu_filter *f) {
  if (f->mhbPending) return mhb_resolve(f);     // (a batch of multi-hypothesis filters: its own blocks)
  if (f->mhcStashedRc) { const int rc = f->mhcStashedRc; f->mhcStashedRc = 0; return rc; }   // (f->err still holds its message)
  if (f->rsPending) return rs_resolve(f);       // (rfsgpu_resample_async: never pending next to a cycle)
  if (f->rcPending) return rc_resolve(f);       // (rfsgpu_rbphd_cycle_async: an RB-PHD handle, no FastSLAM cycle beside it)
  if (!f->mhcPending) return RFSGPU_OK;
  f->mhcPending = false;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(f->hMhcBlock, f->mhcBlock, fs_cycle_state_bytes(f->Ncap), hipMemcpyDeviceToHost, f->stream));
  const int rc = check_device_errors(f);   // waits for the stream
  harvest_async(f);
  FsCycleState H;
  fs_cycle_carve(f->hMhcBlock, f->Ncap, H);
  const int done = H.w[FSC_DONE] - f->mhcDone;      // of the pending cycles with measurements, the first `done` ran
  f->mhcDone = H.w[FSC_DONE];
  f->mhcNFired = H.w[FSC_NFIRED];
  for (size_t k = (size_t)std::max(done, 0); k < f->mhcFlips.size(); k++) f->cur ^= f->mhcFlips[k] ? 1 : 0;
  const bool lastRan = f->mhcFlips.empty() || done >= (int)f->mhcFlips.size();
  f->mhcFlips.clear();
  const int n = H.w[FSC_N];
  if (n < 1 || n > f->Ncap) return fail(f, RFSGPU_ERR_HIP, "fastslam_cycle: the device returned a particle count outside [1, max_particles]");
  f->N = n;
  f->B.N = n;
  f->fsResampleOccured = H.w[FSC_RESAMPLED] != 0;
  ensure_ids(f);
  memcpy(f->pid.data(), H.pid, (size_t)f->Ncap * sizeof(int));
  memcpy(f->ppid.data(), H.ppid, (size_t)f->Ncap * sizeof(int));
  f->mhcIdsDirty = false;
  if (f->mhcLastEmpty && lastRan) {
    f->mhcNGrown = f->mhcNAfter = n; f->mhcFired = 0; f->mhcNEff = 0.0;
    f->mhcPlan.resize(n);
    f->parents.resize(n);
    for (int k = 0; k < n; k++) { f->mhcPlan[k] = k; f->parents[k] = k; }
  } else if (lastRan) {
    f->mhcNGrown = H.w[FSC_NGROWN]; f->mhcNAfter = n; f->mhcFired = H.w[FSC_FIRED]; f->mhcNEff = H.nEff[0];
    const int ng = std::min(std::max(f->mhcNGrown, 0), f->Ncap);
    f->parents.assign(H.slotSrc, H.slotSrc + ng);
    f->mhcPlan.assign(H.plan, H.plan + n);
    if (f->mhcFired) { f->resampleOccured = true; f->externalAck = false; }
  }
  if (H.w[FSC_OVF]) {
    HIPCHK(hipMemsetAsync(f->mhc.w + FSC_OVF, 0, sizeof(int), f->stream));
    if (rc == RFSGPU_OK)
      return fail(f, RFSGPU_ERR_CAPACITY, "fastslam_cycle: the particle copies of a multi-hypothesis update exceed max_particles (rfsgpu_create_ex); that cycle and "
                                          "those enqueued behind it were abandoned, the state is the one before it");
  }
  return rc;
}
// ---- [resample] ParticleFilter::resample on the device (resample_plan.h) ---------------------------------------------------------
// What rfsgpu_resample_apply_n does on the host, once the device has decided: one stream-ordered copy of the block's head into
// pinned memory, then the wait -- through check_device_errors, as mhc_resolve and rfsgpu_synchronize: an error word that an
// asynchronous call before the resampling raised (a mixture beyond gm_capacity, ...) comes out of the resolving call.  The host
// route meets it in the call it waits in; a host that resamples on the device must not lose it.
static int rs_resolve(rfsgpu_filter *f) {
  if (!f->rsPending) return RFSGPU_OK;
  f->rsPending = false;
  f->rsShrink = false;
  hipSetDevice(f->device);
  const long long t0 = now_ns();
  HIPCHK(hipMemcpyAsync(f->hRsBlock, f->rsBlock, resample_state_head_bytes(f->Ncap), hipMemcpyDeviceToHost, f->stream));
  const int rc = check_device_errors(f);   // waits for the stream
  harvest_async(f);
  ResampleState H;
  resample_state_carve(f->hRsBlock, f->Ncap, H);
  const int n = f->N;
  f->rsFired = 0; f->rsNEff = 0.0; f->rsNAfter = n;
  f->rsPlan.resize(n);
  for (int k = 0; k < n; k++) f->rsPlan[k] = k;
  if (H.w[RSW_BAD] != 0) {
    if (rc != RFSGPU_OK) return rc;         // (the earlier calls' error first; its message stands)
    return fail(f, RFSGPU_ERR_INVALID, "resample_async: a particle weight is negative or not finite, or the weights do not sum to a positive number; nothing was "
                                       "normalised, moved or reset");
  }
  f->rsNEff = H.nEff[0];
  if (H.w[RSW_FIRED] == 0) return rc;
  const int na = H.w[RSW_N_AFTER];
  if (na < 1 || na > n) return fail(f, RFSGPU_ERR_HIP, "resample_async: the device returned a particle count outside [1, n_particles]");
  f->rsFired = 1;
  f->rsNAfter = na;
  f->rsPlan.assign(H.plan, H.plan + na);
  f->N = na;
  f->B.N = na;
  ensure_ids(f);
  memcpy(f->pid.data(), H.pid, (size_t)na * sizeof(int));
  memcpy(f->ppid.data(), H.ppid, (size_t)na * sizeof(int));
  memcpy(f->rsIdsDev.data(), H.pid, (size_t)na * sizeof(int));
  memcpy(f->rsIdsDev.data() + f->Ncap, H.ppid, (size_t)na * sizeof(int));
  f->resampleOccured = true;
  f->externalAck = false;
  f->mhcIdsDirty = true;
  f->timing.particleResample_cpu += now_ns() - t0;
  return rc;                                // (the bookkeeping above is done either way: the device did resample)
}
// The ResampleState block and its pinned landing buffer (allocated on first use).  upload: the ids go up when the host has changed them
// since the device last held them (the first call, rfsgpu_resample_apply, rfsgpu_set_particle_ids, ...) -- every earlier call has been
// resolved then, so the pinned buffer's tail is free.
static int rs_block_ready(rfsgpu_filter *f, bool upload) {
  const int Ncap = f->Ncap;
  if (!f->hRsBlock) HIPCHK(hipHostMalloc(&f->hRsBlock, resample_state_head_bytes(Ncap) + (size_t)2 * Ncap * sizeof(int)));
  if (!f->rsBlock) {
    HIPCHK(hipMalloc(&f->rsBlock, resample_state_bytes(Ncap)));
    HIPCHK(hipMemsetAsync(f->rsBlock, 0, resample_state_bytes(Ncap), f->stream));
    resample_state_carve(f->rsBlock, Ncap, f->rs);
  }
  if (!upload) return RFSGPU_OK;
  const ResampleState &S = f->rs;
  ensure_ids(f);
  bool same = (int)f->rsIdsDev.size() == 2 * Ncap;
  if (same) same = !memcmp(f->rsIdsDev.data(), f->pid.data(), (size_t)Ncap * sizeof(int)) && !memcmp(f->rsIdsDev.data() + Ncap, f->ppid.data(), (size_t)Ncap * sizeof(int));
  if (!same) {
    f->rsIdsDev.resize((size_t)2 * Ncap);
    memcpy(f->rsIdsDev.data(), f->pid.data(), (size_t)Ncap * sizeof(int));
    memcpy(f->rsIdsDev.data() + Ncap, f->ppid.data(), (size_t)Ncap * sizeof(int));
    int *up = reinterpret_cast<int *>(f->hRsBlock + resample_state_head_bytes(Ncap));
    memcpy(up, f->rsIdsDev.data(), (size_t)2 * Ncap * sizeof(int));
    HIPCHK(hipMemcpyAsync(S.pid, up, (size_t)2 * Ncap * sizeof(int), hipMemcpyHostToDevice, f->stream));     // (pid and ppid lie back to back)
  }
  return RFSGPU_OK;
}
int rfsgpu_resample_async(rfsgpu_filter *f, double eff_n, double eff_n_percent, double u01, int n_out, int force, int renormalize) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_resample_async (use rfsgpu_batch_resample_async)", ON_BATCH);
  if (f->groupShard) return fail(f, RFSGPU_ERR_UNSUPPORTED, "resample_async: not available on a shard of an rfsgpu_group (the resampling is global: rfsgpu_group_resample)");
  if (f->mhcHave) return fail(f, RFSGPU_ERR_UNSUPPORTED, "resample_async: this handle runs rfsgpu_fastslam_cycle_async, which resamples inside the cycle and keeps the ids in its own block");
  if (f->rcHave) return fail(f, RFSGPU_ERR_UNSUPPORTED, "resample_async: this handle runs rfsgpu_rbphd_cycle_async, which resamples inside the cycle and keeps the ids and the counters of its gate on the device");
  if (!(u01 >= 0.0 && u01 < 1.0)) return fail(f, RFSGPU_ERR_INVALID, "resample_async: u01 must lie in [0, 1)");
  if (n_out < 0) return fail(f, RFSGPU_ERR_INVALID, "resample_async: negative n_out");
  hipSetDevice(f->device);
  const long long t0 = now_ns();
  const int N = f->N;
  { const int rcb = rs_block_ready(f, true); if (rcb != RFSGPU_OK) return rcb; }
  const ResampleState &S = f->rs;
  ResampleArg A;
  A.effN = eff_n; A.effNPercent = eff_n_percent; A.u01 = u01;
  A.n = N; A.nOut = (n_out == 0 || n_out >= N) ? N : n_out;     // ParticleFilter.hpp:417-418
  A.force = force ? 1 : 0; A.renorm = renormalize ? 1 : 0;
  const LiveCount live{S.w + RSW_N, S.w + RSW_BAD}, moved{S.w + RSW_GATHER_N, S.w + RSW_BAD}, renorm{S.w + RSW_RENORM_N, S.w + RSW_NO_RENORM};
  weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, N, f->dSums);
  resample_check_kernel<<<1, RSP_THREADS, 0, f->stream>>>(f->B.weight, N, f->dSums, S);
  normalize_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, 0, 0.0, (const double *)f->dSums, 1, live);
  resample_plan_kernel<<<1, RSP_THREADS, 0, f->stream>>>(f->B.weight, S, A);
  resample_gather_kernel<<<N, 256, 0, f->stream>>>(f->B, f->cur, S.plan, f->P.poseCovStride, map_only(f), moved);
  if (renormalize) {      // RBPHDFilter::update's else branch: the weights are normalised once more when resample() returned false
    weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, 0, f->dSums, renorm);
    normalize_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, 0, 0.0, (const double *)f->dSums, 1, renorm);
  }
  HIPCHK(hipGetLastError());
  f->rsPending = true;
  f->rsShrink = A.nOut < N;
  f->rsHave = true;
  const long long dtn = now_ns() - t0;
  f->timing.particleResample_wall += dtn;
  f->timing.particleResample_cpu += dtn;
  return RFSGPU_OK;
}
int rfsgpu_last_resample(rfsgpu_filter *f, int *fired, double *n_eff, int *n_after, int *plan, int max_n) {
  CHECK_HANDLE(f);
  if (!f->rsHave) return fail(f, RFSGPU_ERR_INVALID, "last_resample: no rfsgpu_resample_async has run on this handle");
  if (plan && max_n < f->rsNAfter) return fail(f, RFSGPU_ERR_INVALID, "last_resample: max_n is below the particle count");
  if (fired) *fired = f->rsFired;
  if (n_eff) *n_eff = f->rsNEff;
  if (n_after) *n_after = f->rsNAfter;
  if (plan) for (int k = 0; k < f->rsNAfter; k++) plan[k] = f->rsPlan[k];
  return RFSGPU_OK;
}
// ---- [rbphd-cycle] the whole RBPHDFilter::update on the device (birth_walk.h) ------------------------------------------------------
// What the pending cycles left on the device comes back as rs_resolve brings a resampling back: one copy of the block's head, one
// wait (through check_device_errors, so an error word raised by an earlier asynchronous call comes out of the resolving call).
static int rc_resolve(rfsgpu_filter *f) {
  if (!f->rcPending) return RFSGPU_OK;
  f->rcPending = false;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(f->hRsBlock, f->rsBlock, resample_state_head_bytes(f->Ncap), hipMemcpyDeviceToHost, f->stream));
  const int rc = check_device_errors(f);   // waits for the stream
  harvest_async(f);
  ResampleState H;
  resample_state_carve(f->hRsBlock, f->Ncap, H);
  const int n = f->N;
  ensure_ids(f);
  memcpy(f->pid.data(), H.pid, (size_t)n * sizeof(int));
  memcpy(f->ppid.data(), H.ppid, (size_t)n * sizeof(int));
  memcpy(f->rsIdsDev.data(), H.pid, (size_t)n * sizeof(int));
  memcpy(f->rsIdsDev.data() + f->Ncap, H.ppid, (size_t)n * sizeof(int));
  f->resampleOccured = H.w[RCW_RESAMPLED] != 0;
  if (H.w[RCW_NFIRED] != f->rcCounts[2]) { f->externalAck = false; f->mhcIdsDirty = true; }
  f->rcCounts[0] = H.w[RCW_NCYCLES]; f->rcCounts[1] = H.w[RCW_NGATE]; f->rcCounts[2] = H.w[RCW_NFIRED]; f->rcCounts[3] = H.w[RCW_MAXLEVEL];
  f->rcWalkMax = H.w[RCW_WALK_MAX];
  f->rcGate = f->rcLastEmpty ? 0 : H.w[RCW_GATE];
  f->rcFired = f->rcLastEmpty ? 0 : H.w[RSW_FIRED];
  f->rcNEff = f->rcLastEmpty ? 0.0 : H.nEff[0];
  f->rcPlan.resize(n);
  for (int k = 0; k < n; k++) f->rcPlan[k] = (f->rcLastEmpty || !f->rcFired) ? k : H.plan[k];
  if (H.w[RCW_BADSEEN] != 0) {
    HIPCHK(hipMemsetAsync(f->rs.w + RCW_BADSEEN, 0, sizeof(int), f->stream));
    if (rc == RFSGPU_OK)
      return fail(f, RFSGPU_ERR_INVALID, "rbphd_cycle: a particle weight was negative or not finite, or the weights did not sum to a positive number, behind an "
                                         "update; that cycle normalised, moved and reset nothing");
  }
  return rc;
}
int rfsgpu_rbphd_set_resampling(rfsgpu_filter *f, double eff_n, double eff_n_percent) {
  CHECK_HANDLE_HOST(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_rbphd_set_resampling (use rfsgpu_batch_set_resampling)", ON_BATCH);
  if (!(eff_n >= 0.0) || !(eff_n_percent >= 0.0)) return fail(f, RFSGPU_ERR_INVALID, "rbphd_set_resampling: thresholds must be non-negative");
  f->rcEffN = eff_n;
  f->rcEffNPercent = eff_n_percent;
  return RFSGPU_OK;
}
int rfsgpu_rbphd_cycle_async(rfsgpu_filter *f, const double *z, int n_z, const double *scan, int n_scan, double u01) {
  if (!f) return RFSGPU_ERR_INVALID;
  if (f->mhcStashedRc || f->rsPending || f->mhcPending || f->mhbPending) { const int rc = mhc_resolve(f); if (rc != RFSGPU_OK) return rc; }
  if (f->batch) return refuse_on_kind(f, "rfsgpu_rbphd_cycle_async", ON_BATCH);
  if (f->groupShard) return fail(f, RFSGPU_ERR_UNSUPPORTED, "rbphd_cycle: not available on a shard of an rfsgpu_group (the resampling is global: rfsgpu_group_resample)");
  if (f->fastSlamHandle || f->mhcHave) return fail(f, RFSGPU_ERR_UNSUPPORTED, "rbphd_cycle: this handle runs FastSLAM updates (rfsgpu_fastslam_cycle_async is their device cycle)");
  if (f->inheritMode == RFSGPU_INHERIT_EXTERNAL) return fail(f, RFSGPU_ERR_UNSUPPORTED, "rbphd_cycle: RFSGPU_INHERIT_EXTERNAL leaves the birth lists to a host that must learn of every resampling; the cycle tells nobody");
  if (!(u01 >= 0.0 && u01 < 1.0)) return fail(f, RFSGPU_ERR_INVALID, "rbphd_cycle: u01 must lie in [0, 1)");
  if (n_z < 0 || n_z > RFSGPU_MAX_Z) return fail(f, RFSGPU_ERR_INVALID, "at most RFSGPU_MAX_Z measurements per update");
  if (n_z > 0 && !z) return fail(f, RFSGPU_ERR_INVALID, "null measurement buffer");
  if (scan && (f->model != RFSGPU_MODEL_VICTORIAPARK_3D || n_scan < 2 || n_scan > RFSGPU_VP_MAX_SCAN))
    return fail(f, RFSGPU_ERR_INVALID, "rbphd_cycle: a laser scan needs the Victoria Park model and 2..RFSGPU_VP_MAX_SCAN beams");
  if (n_z > 0 && f->D == 3 && !scan && f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "Victoria Park model: a laser scan must come with the first update or precede it (rfsgpu_set_laser_scan)");
  hipSetDevice(f->device);
  const int N = f->N;
  { const int rcb = rs_block_ready(f, !f->rcPending); if (rcb != RFSGPU_OK) return rcb; }
  const ResampleState &S = f->rs;
  // (the step below clears the host's flag: what the device starts from is taken first)
  const int resampledInit = f->rcPending ? -1 : (f->resampleOccured ? 1 : 0);
  // The update is counted, and the handle goes over to the device route, only behind the last host step that can fail: a call that
  // returns an error has counted nothing (a scan it carried may have been installed, as by rfsgpu_set_step_inputs_async).
  auto counted = [&]() {
    rbphd_count_kernel<<<1, 64, 0, f->stream>>>(S, resampledInit, n_z);
    f->rcPending = true;
    f->rcHave = true;
    f->rcLastEmpty = n_z == 0;
  };
  if (scan) {     // through the pinned ring, as rfsgpu_set_step_inputs_async: no wait for the device; the clutter density goes by value in Params
    double *h = nullptr;
    int k = 0;
    { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
    { const int rc = push_scan(f, h + (size_t)f->Ncap * 22, scan, n_scan); if (rc != RFSGPU_OK) return rc; }
    HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
  }
  if (n_z == 0) {                          // :451-452 (the scan, if one came, is installed: setLaserScan precedes the update)
    counted();
    HIPCHK(hipGetLastError());
    return RFSGPU_OK;
  }
  { const int rc = cycle_impl(f, RFSGPU_CYCLE_NO_PREDICT, nullptr, nullptr, 0, nullptr, z, n_z, true, 0); if (rc != RFSGPU_OK) return rc; }
  const long long t0 = now_ns();           // (the step's host time is booked by the step; what follows is the resampling's)
  counted();
  // the tail (:526-539): rfsgpu_resample_async's launches with renormalize = 1, the gate in front of the plan
  ResampleArg A;
  A.effN = f->rcEffN >= 0.0 ? f->rcEffN : (double)N / 4.0;
  A.effNPercent = f->rcEffNPercent >= 0.0 ? f->rcEffNPercent : 0.25;
  A.u01 = u01;
  A.n = N; A.nOut = N; A.force = 0; A.renorm = 1;
  const LiveCount first{S.w + RSW_N, S.w + RCW_BADNOW}, moved{S.w + RSW_GATHER_N, S.w + RSW_BAD}, renorm{S.w + RSW_RENORM_N, S.w + RSW_NO_RENORM};
  weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, N, f->dSums);
  resample_check_kernel<<<1, RSP_THREADS, 0, f->stream>>>(f->B.weight, N, f->dSums, S);
  rbphd_gate_kernel<<<1, 64, 0, f->stream>>>(S, (int)std::min<unsigned>(f->cfg.minUpdatesBeforeResample, 0x7fffffffu), (int)std::min<unsigned>(f->cfg.minMeasurementsBeforeResample, 0x7fffffffu));
  normalize_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, 0, 0.0, (const double *)f->dSums, 1, first);
  resample_plan_kernel<<<1, RSP_THREADS, 0, f->stream>>>(f->B.weight, S, A);
  resample_gather_kernel<<<N, 256, 0, f->stream>>>(f->B, f->cur, S.plan, f->P.poseCovStride, map_only(f), moved);
  weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, 0, f->dSums, renorm);
  normalize_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, 0, 0.0, (const double *)f->dSums, 1, renorm);
  rbphd_fired_kernel<<<1, 64, 0, f->stream>>>(S);
  HIPCHK(hipGetLastError());
  const long long dtn = now_ns() - t0;
  f->timing.particleResample_wall += dtn;
  f->timing.particleResample_cpu += dtn;
  return RFSGPU_OK;
}
int rfsgpu_rbphd_cycle_counts(rfsgpu_filter *f, int *n_cycles, int *n_gate_open, int *n_resamplings, int *max_level) {
  CHECK_HANDLE(f);
  if (n_cycles) *n_cycles = f->rcCounts[0];
  if (n_gate_open) *n_gate_open = f->rcCounts[1];
  if (n_resamplings) *n_resamplings = f->rcCounts[2];
  if (max_level) *max_level = f->rcCounts[3];
  return RFSGPU_OK;
}
int rfsgpu_rbphd_last_cycle(rfsgpu_filter *f, int *gate_open, int *fired, double *n_eff, int *plan, int max_n, int *walk_levels) {
  CHECK_HANDLE(f);
  if (!f->rcHave) return fail(f, RFSGPU_ERR_INVALID, "rbphd_last_cycle: no rfsgpu_rbphd_cycle_async has run on this handle");
  if (plan && max_n < f->N) return fail(f, RFSGPU_ERR_INVALID, "rbphd_last_cycle: max_n is below the particle count");
  if (gate_open) *gate_open = f->rcGate;
  if (fired) *fired = f->rcFired;
  if (n_eff) *n_eff = f->rcNEff;
  if (walk_levels) *walk_levels = f->rcWalkMax;
  if (plan) for (int k = 0; k < f->N && k < (int)f->rcPlan.size(); k++) plan[k] = f->rcPlan[k];
  return RFSGPU_OK;
}
int rfsgpu_rbphd_cycle_pending(rfsgpu_filter *f) { return (f && f->rcPending) ? 1 : 0; }
int rfsgpu_fastslam_set_resampling(rfsgpu_filter *f, double eff_n, double eff_n_percent) {
  CHECK_HANDLE_HOST(f);
  if (f->batch) return refuse_on_kind(f, "rfsgpu_fastslam_set_resampling (use rfsgpu_batch_set_resampling)", ON_BATCH);
  if (!(eff_n >= 0.0) || !(eff_n_percent >= 0.0)) return fail(f, RFSGPU_ERR_INVALID, "fastslam_set_resampling: thresholds must be non-negative");
  f->fsEffN = eff_n;
  f->fsEffNPercent = eff_n_percent;
  return RFSGPU_OK;
}
// One cycle enqueued.  full: rfsgpu_fastslam_cycle_full_async -- either model, any candidate threshold, the scan of this update, and
// one hypothesis associated as rfsgpu_fastslam_update associates it; without it the launches are rfsgpu_fastslam_cycle_async's.
static int fastslam_cycle_enqueue(rfsgpu_filter *f, int predict, const double *z, int n_z, const double *scan, int n_scan, double u01, int n_init, bool full);
int rfsgpu_fastslam_cycle_async(rfsgpu_filter *f, int predict, const double *z, int n_z, double u01, int n_init) {
  if (!f) return RFSGPU_ERR_INVALID;
  if (f->mhcStashedRc || f->rsPending) { const int rc = mhc_resolve(f); if (rc != RFSGPU_OK) return rc; }
  if (f->batch) return refuse_on_kind(f, "rfsgpu_fastslam_cycle_async", ON_BATCH);
  if (f->groupShard) return fail(f, RFSGPU_ERR_UNSUPPORTED, "fastslam_cycle: not available on a shard of an rfsgpu_group (the particle count would be known to one device only)");
  if (f->D != 2) return fail(f, RFSGPU_ERR_UNSUPPORTED, "fastslam_cycle: the Victoria Park model is not served (the 2-D range-bearing model only)");
  if (f->fs.landmarkCandidateMeasurementCountThreshold != 1u)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "fastslam_cycle: landmarkCandidateMeasurementCountThreshold must be 1 (landmark candidate lists are not served on this route)");
  return fastslam_cycle_enqueue(f, predict, z, n_z, nullptr, 0, u01, n_init, false);
}
int rfsgpu_fastslam_cycle_full_async(rfsgpu_filter *f, int predict, const double *z, int n_z, const double *scan, int n_scan, double u01, int n_init) {
  if (!f) return RFSGPU_ERR_INVALID;
  if (f->mhcStashedRc || f->rsPending) { const int rc = mhc_resolve(f); if (rc != RFSGPU_OK) return rc; }
  if (f->batch) return refuse_on_kind(f, "rfsgpu_fastslam_cycle_full_async", ON_BATCH);
  if (f->groupShard) return fail(f, RFSGPU_ERR_UNSUPPORTED, "fastslam_cycle: not available on a shard of an rfsgpu_group (the particle count would be known to one device only)");
  return fastslam_cycle_enqueue(f, predict, z, n_z, scan, n_scan, u01, n_init, true);
}
static int fastslam_cycle_enqueue(rfsgpu_filter *f, int predict, const double *z, int n_z, const double *scan, int n_scan, double u01, int n_init, bool full) {
  if (f->fs.maxNDataAssocHypotheses < 1 || f->fs.maxNDataAssocHypotheses > FSMH_MAX_HYP)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "fastslam_cycle: maxNDataAssocHypotheses must be in [1, 16]");
  if (f->Ncap > RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "fastslam_cycle: max_particles exceeds RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES (2048): the resampling kernel holds the whole filter in LDS");
  if (n_z < 0 || n_z > RFSGPU_MAX_Z) return fail(f, RFSGPU_ERR_INVALID, "at most RFSGPU_MAX_Z measurements per update");
  if (n_z > 0 && !z) return fail(f, RFSGPU_ERR_INVALID, "null measurement buffer");
  if (!(u01 >= 0.0 && u01 < 1.0)) return fail(f, RFSGPU_ERR_INVALID, "fastslam_cycle: u01 must lie in [0, 1)");
  if (n_init < 0) return fail(f, RFSGPU_ERR_INVALID, "fastslam_cycle: negative n_init");
  if (scan && (f->model != RFSGPU_MODEL_VICTORIAPARK_3D || n_scan < 2 || n_scan > RFSGPU_VP_MAX_SCAN))
    return fail(f, RFSGPU_ERR_INVALID, "fastslam_cycle: a laser scan needs the Victoria Park model and 2..RFSGPU_VP_MAX_SCAN beams");
  if (f->D == 3 && !scan && f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "Victoria Park model: no laser scan has been set (pass one, or rfsgpu_set_laser_scan first)");
  hipSetDevice(f->device);
  const int Ncap = f->Ncap, D = f->D;
  const bool single = full && f->fs.maxNDataAssocHypotheses == 1;     // (the association of rfsgpu_fastslam_update's single-hypothesis branch)
  const FsMhLayout L = fs_mh_layout();
  if (single) { if (!f->fsArena) HIPCHK(hipMalloc(&f->fsArena, (size_t)Ncap * fs_arena_bytes())); }
  else if (!f->mhArena) HIPCHK(hipMalloc(&f->mhArena, (size_t)Ncap * L.total));
  if (!f->mhcInts) HIPCHK(hipMalloc(&f->mhcInts, (size_t)4 * Ncap * sizeof(int)));
  if (!f->hMhcBlock) HIPCHK(hipHostMalloc(&f->hMhcBlock, fs_cycle_state_bytes(Ncap)));
  if (!f->mhcBlock) {
    HIPCHK(hipMalloc(&f->mhcBlock, fs_cycle_state_bytes(Ncap)));
    HIPCHK(hipMemsetAsync(f->mhcBlock, 0, fs_cycle_state_bytes(Ncap), f->stream));
    fs_cycle_carve(f->mhcBlock, Ncap, f->mhc);
    f->mhcIdsDirty = true;
  }
  if (f->fsEffN < 0.0) { f->fsEffN = f->N / 4.0; f->fsEffNPercent = 0.25; }   // ParticleFilter.hpp:232
  const FsCycleState &S = f->mhc;
  if (!f->mhcPending && f->mhcIdsDirty) {
    ensure_ids(f);
    HIPCHK(hipMemcpyAsync(S.pid, f->pid.data(), (size_t)Ncap * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(S.ppid, f->ppid.data(), (size_t)Ncap * sizeof(int), hipMemcpyHostToDevice, f->stream));
    f->mhcIdsDirty = false;
  }
  f->holes = false;
  f->fastSlamHandle = true;
  f->mhcHave = true;
  if (scan) {     // through the pinned ring, as rfsgpu_set_step_inputs_async: no wait for the device; the clutter density goes by value in Params
    double *h = nullptr;
    int k = 0;
    { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
    { const int rc = push_scan(f, h + (size_t)Ncap * 22, scan, n_scan); if (rc != RFSGPU_OK) return rc; }
    HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
  }
  const LiveCount live{S.w + FSC_N, S.w + FSC_OVF};
  fs_cycle_begin_kernel<<<1, 64, 0, f->stream>>>(S, f->mhcPending ? -1 : f->N, f->mhcPending ? -1 : (f->fsResampleOccured ? 1 : 0), n_z == 0 ? 1 : 0);
  if (predict && D == 3) fs_cycle_static_step3_kernel<<<(Ncap + 3) / 4, 256, 0, f->stream>>>(f->B, f->P, f->cur, live);
  else if (predict) fs_cycle_static_step_kernel<<<(Ncap + 3) / 4, 256, 0, f->stream>>>(f->B, f->P, f->cur, live);
  HIPCHK(hipGetLastError());
  if (n_z == 0) {    // :399-402: the update is counted, nothing else happens
    f->mhcLastEmpty = true;
    if (!f->mhcPending) {       // (the count is still the host's: nothing to wait for)
      f->mhcNGrown = f->mhcNAfter = f->N; f->mhcFired = 0; f->mhcNEff = 0.0;
      f->mhcPlan.resize(f->N);
      f->parents.resize(f->N);
      for (int k = 0; k < f->N; k++) { f->mhcPlan[k] = k; f->parents[k] = k; }
    }
    return RFSGPU_OK;
  }
  int rc = stage_measurements(f, z, n_z);
  if (rc != RFSGPU_OK) return rc;
  const FsParams F = fs_params(f, n_z);
  int *dSlotHyp = f->mhcInts, *dSlotNH = dSlotHyp + Ncap, *dDst = dSlotNH + Ncap, *dSrc = dDst + Ncap;
  if (single) {
    const size_t b1 = (size_t)(3 * RFSGPU_MAX_Z * 8) + fs_lds_bytes_per_wave(f->cap);
    Buffers Bc = f->B;
    Bc.N = Ncap;      // (the kernel's bound is its LiveCount)
    if (D == 2) {
      if ((rc = set_lds(f, (fs_associate_update_live_kernel<2>), b1)) != RFSGPU_OK) return rc;
      fs_associate_update_live_kernel<2><<<Ncap, 64, b1, f->stream>>>(Bc, f->P, F, f->cur, n_z, f->fsArena, live);
    } else {
      if ((rc = set_lds(f, (fs_associate_update_live_kernel<3>), b1)) != RFSGPU_OK) return rc;
      fs_associate_update_live_kernel<3><<<Ncap, 64, b1, f->stream>>>(Bc, f->P, F, f->cur, n_z, f->fsArena, live);
    }
    fs_cycle_identity_plan_kernel<<<1, FS_CYCLE_THREADS, 0, f->stream>>>(S, Ncap);
  } else {
    const int kmax = (int)f->fs.maxNDataAssocHypotheses;
    if (D == 2) fs_mh_associate_kernel<2><<<Ncap, 64 * FSMH_WAVES, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, kmax, f->fs.maxDataAssocLogLikelihoodDiff, f->mhArena, live);
    else fs_mh_associate_kernel<3><<<Ncap, 64 * FSMH_WAVES, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, kmax, f->fs.maxDataAssocLogLikelihoodDiff, f->mhArena, live);
    fs_mh_plan_kernel<<<1, FS_CYCLE_THREADS, 0, f->stream>>>(f->mhArena, S, dSlotHyp, dSlotNH, dDst, dSrc, Ncap);
    LiveCopy lc;
    lc.n = S.w + FSC_NCOPY; lc.ovf = S.w + FSC_OVF; lc.copyCand = S.w + FSC_RESAMPLED;
    fs_mh_copy_kernel<<<Ncap, 256, 0, f->stream>>>(f->B, f->cur, dDst, dSrc, 0, f->P.poseCovStride, lc);
    fs_mh_split_weights_kernel<<<(Ncap + 255) / 256, 256, 0, f->stream>>>(f->B.weight, S.slotSrc, dSlotNH, 0, 0, live);
    fs_mh_split_weights_kernel<<<(Ncap + 255) / 256, 256, 0, f->stream>>>(f->B.weight, S.slotSrc, dSlotNH, 0, 1, live);
    if (D == 2) fs_mh_apply_kernel<2><<<Ncap, 64, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, S.slotSrc, dSlotHyp, f->mhArena, live);
    else fs_mh_apply_kernel<3><<<Ncap, 64, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, S.slotSrc, dSlotHyp, f->mhArena, live);
  }
  HIPCHK(hipGetLastError());
  bool flipped = false;
  if ((unsigned)n_z >= f->fs.pruningMeasurementsThreshold) {   // :611-612
    Params Pp = f->P;
    Pp.pruneT = f->fs.mapExistencePruneThreshold;
    const size_t pb = gm_prune_lds_bytes_per_wave(f->cap);
    if ((rc = set_lds(f, (gm_prune_kernel<4, false, false, LiveCount>), 4 * pb)) != RFSGPU_OK) return rc;
    gm_prune_kernel<4, false, false, LiveCount><<<(Ncap + 3) / 4, 256, 4 * pb, f->stream>>>(f->B, Pp, f->cur, f->cur ^ 1, live);
    HIPCHK(hipGetLastError());
    f->cur ^= 1;
    flipped = true;
  }
  if (D == 2) fs_new_landmarks_kernel<2, false, LiveCount><<<(Ncap + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, live);
  else fs_new_landmarks_kernel<3, false, LiveCount><<<(Ncap + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, F, f->cur, n_z, live);
  // resampleWithMapCopy: the normalisation that ParticleFilter::resample starts with (or, where the gates keep it from running, the
  // one of :743), the decision and the plan, the copies, and the second normalisation of a resample() that returned false
  weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, 0, f->dSums, live);
  normalize_kernel<<<(Ncap + 255) / 256, 256, 0, f->stream>>>(f->B.weight, 0, 0.0, (const double *)f->dSums, 1, live);
  FsShrinkArg A;
  A.effN = f->fsEffN; A.effNPercent = f->fsEffNPercent; A.u01 = u01;
  A.nInit = n_init; A.nMax = f->fs.nParticlesMax; A.nZ = n_z;
  A.minUpdates = f->fs.minUpdatesBeforeResample; A.minMeasurements = f->fs.minMeasurementsBeforeResample;
  fs_resample_shrink_kernel<<<1, FS_CYCLE_THREADS, 0, f->stream>>>(f->B.weight, S, A);
  resample_gather_kernel<<<Ncap, 256, 0, f->stream>>>(f->B, f->cur, S.plan, f->P.poseCovStride, map_only(f), live);
  const LiveCount renorm{S.w + FSC_RENORM_N, S.w + FSC_OVF};
  weight_sums_kernel<<<1, 1024, 0, f->stream>>>(f->B.weight, 0, f->dSums, renorm);
  normalize_kernel<<<(Ncap + 255) / 256, 256, 0, f->stream>>>(f->B.weight, 0, 0.0, (const double *)f->dSums, 1, renorm);
  HIPCHK(hipGetLastError());
  f->mhcFlips.push_back(flipped ? 1 : 0);
  f->mhcLastEmpty = false;
  f->mhcPending = true;
  return RFSGPU_OK;
}
int rfsgpu_fastslam_cycle_counts(rfsgpu_filter *f, int *n_cycles, int *n_resamplings) {
  CHECK_HANDLE(f);
  if (!f->mhcHave) return fail(f, RFSGPU_ERR_INVALID, "fastslam_cycle_counts: no device cycle has run on this handle");
  if (n_cycles) *n_cycles = f->mhcDone;
  if (n_resamplings) *n_resamplings = f->mhcNFired;
  return RFSGPU_OK;
}
// [test] One slot's weight, mixture size, candidate count and first Gaussian (entry 0 of every plane: gauss [7] or [11]), read or
// written for ANY slot below max_particles: how a test plants a pattern beyond the live count and finds it again.
int rfsgpu_debug_slot(rfsgpu_filter *f, int slot, int write, double *weight, int *count, int *cand_count, double *gauss) {
  CHECK_HANDLE(f);
  if (slot < 0 || slot >= f->Ncap || !weight || !count || !cand_count || !gauss) return fail(f, RFSGPU_ERR_INVALID, "debug_slot: bad arguments");
  hipSetDevice(f->device);
  const hipMemcpyKind kind = write ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  auto mv = [&](void *dev, void *host, size_t bytes) { return write ? hipMemcpyAsync(dev, host, bytes, kind, f->stream) : hipMemcpyAsync(host, dev, bytes, kind, f->stream); };
  HIPCHK(mv(f->B.weight + slot, weight, sizeof(double)));
  HIPCHK(mv(f->B.count + slot, count, sizeof(int)));
  HIPCHK(mv(f->B.candCount + slot, cand_count, sizeof(int)));
  for (int pl = 0; pl < f->B.npl; pl++) {     // (written into both slabs: a prune flips them)
    HIPCHK(mv(f->B.slab[f->cur] + ((size_t)slot * f->B.npl + pl) * (size_t)f->B.cap, gauss + pl, sizeof(double)));
    if (write) HIPCHK(mv(f->B.slab[f->cur ^ 1] + ((size_t)slot * f->B.npl + pl) * (size_t)f->B.cap, gauss + pl, sizeof(double)));
  }
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}
int rfsgpu_fastslam_cycle_pending(rfsgpu_filter *f) { return (f && f->mhcPending) ? 1 : 0; }
int rfsgpu_fastslam_last_cycle(rfsgpu_filter *f, int *n_after_update, int *n_after_resample, int *fired, double *n_eff, int *parent, int *plan, int max_n) {
  CHECK_HANDLE(f);
  if (!f->mhcHave) return fail(f, RFSGPU_ERR_INVALID, "fastslam_last_cycle: no rfsgpu_fastslam_cycle_async has run on this handle");
  if ((parent && max_n < f->mhcNGrown) || (plan && max_n < f->mhcNAfter)) return fail(f, RFSGPU_ERR_INVALID, "fastslam_last_cycle: max_n is below the particle count");
  if (n_after_update) *n_after_update = f->mhcNGrown;
  if (n_after_resample) *n_after_resample = f->mhcNAfter;
  if (fired) *fired = f->mhcFired;
  if (n_eff) *n_eff = f->mhcNEff;
  if (parent) for (int k = 0; k < f->mhcNGrown; k++) parent[k] = k < (int)f->parents.size() ? f->parents[k] : k;
  if (plan) for (int k = 0; k < f->mhcNAfter; k++) plan[k] = f->mhcPlan[k];
  return RFSGPU_OK;
}
int rfsgpu_fastslam_update(rfsgpu_filter *f, const double *z, int n_z) {
  CHECK_HANDLE(f);
  if (f->batch) return refuse_on_kind(f, "FastSLAM", ON_BATCH);
  f->holes = false;
  f->fastSlamHandle = true;
  if (n_z == 0) return RFSGPU_OK;  // :401-402
  if (f->D == 3 && f->B.nScan < 2) return fail(f, RFSGPU_ERR_INVALID, "Victoria Park model: rfsgpu_set_laser_scan must precede the update");
  if (f->fs.maxNDataAssocHypotheses < 1 || f->fs.maxNDataAssocHypotheses > FSMH_MAX_HYP)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "maxNDataAssocHypotheses must be in [1, 16]");
  if (f->fs.maxNDataAssocHypotheses > 1) return fastslam_update_mh(f, z, n_z);
  int rc = stage_measurements(f, z, n_z);
  if (rc != RFSGPU_OK) return rc;
  hipSetDevice(f->device);
  if (!f->fsArena) HIPCHK(hipMalloc(&f->fsArena, (size_t)f->Ncap * fs_arena_bytes()));
  const FsParams F = fs_params(f, n_z);
  const long long t0 = now_ns();
  HIPCHK(hipEventRecord(f->ev[EV_UM0], f->stream));
  const size_t per = fs_lds_bytes_per_wave(f->cap);
  const size_t b2 = (size_t)(3 * RFSGPU_MAX_Z * 8) + 2 * per, b1 = (size_t)(3 * RFSGPU_MAX_Z * 8) + per;
  if (f->D == 2) {
    if (b2 <= 64 * 1024) {
      if ((rc = set_lds(f, (fs_associate_update_kernel<2, 2>), b2)) != RFSGPU_OK) return rc;
      fs_associate_update_kernel<2, 2><<<(f->N + 1) / 2, 128, b2, f->stream>>>(f->B, f->P, F, f->cur, n_z, f->fsArena);
    } else {
      if ((rc = set_lds(f, (fs_associate_update_kernel<1, 2>), b1)) != RFSGPU_OK) return rc;
      fs_associate_update_kernel<1, 2><<<f->N, 64, b1, f->stream>>>(f->B, f->P, F, f->cur, n_z, f->fsArena);
    }
  } else {
    if ((rc = set_lds(f, (fs_associate_update_kernel<1, 3>), b1)) != RFSGPU_OK) return rc;
    fs_associate_update_kernel<1, 3><<<f->N, 64, b1, f->stream>>>(f->B, f->P, F, f->cur, n_z, f->fsArena);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[EV_UM1], f->stream));
  if ((rc = fastslam_map_management(f, F, n_z)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->ev[EV_PR1], f->stream));
  f->parents.clear();
  rc = check_device_errors(f);  // syncs
  // FastSLAM::TimingInfo buckets folded onto the handle's: data association + KF + weighting (one kernel) under
  // mapUpdate / mapUpdate_kf, prune + new landmarks ("map management", :606-693) under mapPrune
  accumulate(f->ev[EV_UM0], f->ev[EV_UM1], f->timing.mapUpdate_wall, &f->lastKernelNs[0]);
  f->timing.mapUpdate_kf_wall = f->timing.mapUpdate_wall;
  accumulate(f->ev[EV_UM1], f->ev[EV_PR1], f->timing.mapPrune_wall, &f->lastKernelNs[3]);
  f->timing.mapUpdate_cpu += now_ns() - t0;
  return rc;
}

static double g_matPermLastKernelMs = 0.0;
double rfsgpu_mat_perm_last_kernel_ms(void) { return g_matPermLastKernelMs; }
int rfsgpu_mat_perm(const double *A, int n, int batch, double *out, int device_id) {
  if (!A || !out || n < 1 || n > 24 || batch < 0) return RFSGPU_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return RFSGPU_ERR_NO_DEVICE;
  if (batch == 0) return RFSGPU_OK;
  if (hipSetDevice(device_id) != hipSuccess) return RFSGPU_ERR_NO_DEVICE;
  double *dA = nullptr, *dO = nullptr;
  const size_t bytes = (size_t)batch * n * n * sizeof(double);
  if (hipMalloc(&dA, bytes) != hipSuccess) return RFSGPU_ERR_HIP;
  if (hipMalloc(&dO, (size_t)batch * sizeof(double)) != hipSuccess) { hipFree(dA); return RFSGPU_ERR_HIP; }
  int rc = RFSGPU_OK;
  if (hipMemcpy(dA, A, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = RFSGPU_ERR_HIP;
  if (rc == RFSGPU_OK) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (timed) hipEventRecord(e0, 0);
    if (mat_perm_launch(dA, n, batch, dO) != hipSuccess) rc = RFSGPU_ERR_HIP;
    if (timed) hipEventRecord(e1, 0);
    if (hipDeviceSynchronize() != hipSuccess) rc = RFSGPU_ERR_HIP;
    float ms = 0.f;
    if (timed && rc == RFSGPU_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) g_matPermLastKernelMs = (double)ms;
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
  }
  if (rc == RFSGPU_OK && hipMemcpy(out, dO, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = RFSGPU_ERR_HIP;
  hipFree(dA);
  hipFree(dO);
  return rc;
}

// ---- filter batches (rfsgpu_create_batch; step_fused.h BatchArg) --------------------------------------------------------------
// n_filters independent 2-D filters in one handle: slot s belongs to filter s / n_per_filter.  One batch cycle is one fused step launch
// (the BATCH instantiation: each workgroup takes its filter's Params / measurement set / counts from device tables) + one post launch
// (the BATCH instantiation of the post kernel: per-filter write-back of the set, sums and division).  Per-slot calls work unchanged.
__global__ void batch_inherit_kernel(unsigned long long *mask, const unsigned long long *before, const int *src, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int s = src[k];
  if (s != k) mask[k] = s < 0 ? 0ull : before[s];
}
__global__ void batch_reset_weights_kernel(double *w, int n, int nPer, const int *flag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n && flag[k / nPer]) w[k] = 1.0;
}
__global__ __launch_bounds__(256) void batch_weight_sums_kernel(double *w, int nPer, double *sums) {
  step_post_tail(w + (size_t)blockIdx.x * nPer, nPer, sums + 2 * blockIdx.x, 0);
}

// Which filter of a batch raised the error word e (the stream is drained): gm_capacity -- the filter the step kernel found at the
// capacity (BatchArg::errFilter, reset here); too many evaluation points -- a filter whose configuration asks for more than
// RFSGPU_MAX_EVAL; the Murty bits come from the post kernel, which the filters share.
static std::string batch_error_note(rfsgpu_filter *f, int e) {
  std::string note;
  auto add = [&](const std::string &t) { note += note.empty() ? " (filter batch: " + t : "; " + t; };
  if (e & ERRBIT_CAPACITY) {
    int b = INT_MAX;
    const int none = INT_MAX;
    if (hipMemcpy(&b, f->dBErrFilter, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
      hipMemcpy(f->dBErrFilter, &none, sizeof(int), hipMemcpyHostToDevice);
    add(b >= 0 && b < f->nF ? "gm_capacity exceeded in filter " + std::to_string(b) : std::string("gm_capacity exceeded, filter not identified"));
  }
  if ((e & ERRBIT_BIRTHLIST) && f->D == 3) {     // (vp_batch.h: the second word of errFilter)
    int b = INT_MAX;
    const int none = INT_MAX;
    if (hipMemcpy(&b, f->dBErrFilter + 1, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
      hipMemcpy(f->dBErrFilter + 1, &none, sizeof(int), hipMemcpyHostToDevice);
    add(b >= 0 && b < f->nF ? "candidate list full in filter " + std::to_string(b) : std::string("candidate list full, filter not identified"));
  }
  if (e & ERRBIT_EVALPTS) {
    int b = -1;
    for (int q = 0; q < f->nF && b < 0; q++) {
      const int c = f->bCfg[q].importanceWeightingEvalPointCount;
      if (c < 0 || c > RFSGPU_MAX_EVAL) b = q;
    }
    add(b >= 0 ? "evaluation points beyond RFSGPU_MAX_EVAL in filter " + std::to_string(b) : std::string("evaluation points beyond RFSGPU_MAX_EVAL"));
  }
  if (e & (ERRBIT_MURTY | ERRBIT_MURTY_POOL)) add("raised by the Murty-200 post kernel, which all filters share");
  if (e & ERRBIT_SCAN) {
    int b = INT_MAX;
    const int none = INT_MAX;
    if (f->dBSensorErrFilter && hipMemcpy(&b, f->dBSensorErrFilter, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
      hipMemcpy(f->dBSensorErrFilter, &none, sizeof(int), hipMemcpyHostToDevice);
    add(b >= 0 && b < f->nF ? "scan of filter " + std::to_string(b) + " beyond max_nz" : std::string("scan beyond max_nz, filter not identified"));
  }
  return note.empty() ? note : note + ")";
}
static void batch_set_all(rfsgpu_filter *f) {
  for (int b = 0; b < f->nF; b++) {
    f->bCfg[b] = f->cfg; f->bRb[b] = f->rb; f->bKf[b] = f->kf;
    memcpy(&f->bQ[(size_t)9 * b], f->Qlm, 9 * sizeof(double));
  }
  f->bParamsDirty = true;
}
// Params of filter b: the handle's own rule (rebuild_params) on the filter's configuration; the handle-wide fields (pose covariance
// stride, partition mode, dense intensity) are the handle's.
static Params batch_params(const rfsgpu_filter *f, int b) {
  Params P = f->P;
  rebuild_params(P, f->bCfg[b], f->bRb[b], f->bKf[b], &f->bQ[(size_t)9 * b], f->D == 3 ? f->bVp[b] : f->vp, f->D == 3 ? f->bVpClutter[b] : f->vpClutter, f->D,
                 f->denseIntensity, f->gateIndex);
  return P;
}
static size_t batch_stage_bytes(const rfsgpu_filter *f) {
  return (size_t)f->nF * (std::max(sizeof(MhBatchFilter), std::max(sizeof(BatchFilter), sizeof(FsBatchFilter))) + sizeof(Params) + RFSGPU_MAX_Z * (size_t)f->D * sizeof(double) + sizeof(int)) + (size_t)f->N * sizeof(int);
}
// The handle-wide Params fields of a cycle (both kinds of batch): the pose covariance stride the call's x / x_cov ask for, and whatever
// else of f->P every filter's record repeats; the table is rewritten when one of them has changed.
static void batch_handle_wide(rfsgpu_filter *f, const double *x, const double *x_cov, int cov_stride) {
  if (x) {
    const int stride = x_cov ? cov_stride : 0;
    if (f->P.poseCovStride != stride) { f->P.poseCovStride = stride; f->bParamsDirty = true; }
  }
  const int hw[3] = {f->P.poseCovStride, f->P.exactPartitions, f->P.denseIntensity};
  for (int q = 0; q < 3; q++)
    if (hw[q] != f->bHandleWide[q]) { f->bHandleWide[q] = hw[q]; f->bParamsDirty = true; }
}
static int batch_check(rfsgpu_filter *f, int filter) {
  if (!f->batch) return fail(f, RFSGPU_ERR_INVALID, "not a filter batch (rfsgpu_create_batch)");
  if (filter < -1 || filter >= f->nF) return fail(f, RFSGPU_ERR_INVALID, "batch: filter index out of range");
  return RFSGPU_OK;
}
// The argument checks that the batch's cycle calls and rfsgpu_batch_resample_async share, each under the call's own prefix and wording.
// predictIs: what the call's predict may be, from predictMin to 1 (nullptr: a call without predict, pose and measurement arguments).
struct BatchCall { const char *who; int predictMin; const char *predictIs, *nullCounts; };
static const BatchCall BATCH_CYCLE{"batch_cycle", -1, "RFSGPU_CYCLE_NO_PREDICT (-1), 0 (static step only) or 1 (births + static step)", "null measurement counts"};
static const BatchCall BATCH_FS_CYCLE{"batch_fastslam_cycle", -1, "RFSGPU_CYCLE_NO_PREDICT (-1), or 0 / 1 (the static landmark step; FastSLAM has no births)", "null measurement counts"};
static const BatchCall BATCH_MH_CYCLE{"batch_fastslam_mh_cycle", 0, "0 or 1 (the static landmark step; FastSLAM has no births)", "null measurement counts or draws"};
static const BatchCall BATCH_RESAMPLE{"batch_resample", 0, nullptr, "null measurement counts"};
static int batch_fail(rfsgpu_filter *f, const BatchCall &C, const std::string &msg) {
  f->err = std::string(C.who) + ": " + msg;
  return RFSGPU_ERR_INVALID;
}
// ... the call as a whole: predict, cov_stride, the counts array (counts: n_z, or null when another per-filter array of the call is)
static int batch_check_call(rfsgpu_filter *f, const BatchCall &C, int predict, const double *x_cov, int cov_stride, const void *counts) {
  if (C.predictIs && (predict < C.predictMin || predict > 1)) return batch_fail(f, C, std::string("predict is ") + C.predictIs);
  if (C.predictIs && x_cov && cov_stride != 0 && cov_stride != 9) return batch_fail(f, C, "cov_stride must be 0 or 9");
  if (C.nullCounts && !counts) return batch_fail(f, C, C.nullCounts);     // (nullCounts null: a call without a counts array)
  return RFSGPU_OK;
}
// ... and filter b's measurement set; the caller's own per-filter checks follow it in the caller's loop, so that the first offending
// filter is reported whichever check it fails
static int batch_check_filter(rfsgpu_filter *f, const BatchCall &C, int b, const double *z, const int *n_z) {
  if (n_z[b] < 0 || n_z[b] > RFSGPU_MAX_Z) return batch_fail(f, C, "filter " + std::to_string(b) + " has " + std::to_string(n_z[b]) + " measurements (0 ... RFSGPU_MAX_Z)");
  if (C.predictIs && n_z[b] > 0 && !z) return batch_fail(f, C, "null measurement buffer");
  return RFSGPU_OK;
}
}  // extern "C" (templates need C++ linkage)
// One cycle's per-filter tables, through a block of the batch's pinned ring to the device: {records [nF] | Params [nF] | z, packed |
// extra}.  The Params table is rebuilt and pushed when the configuration or a handle-wide field has changed (bParamsDirty; bParamsHost
// keeps what the device holds).  Every record is zeroed (its padding travels too), gets its filter's count and offset into the packed
// sets, and goes to fill(record, b) for the rest.  extra: one more host table for the block's tail, copied to dExtra (null: none).
template <class Rec, class Fill>
static int batch_push_tables(rfsgpu_filter *f, Rec *dRec, const double *z, const int *n_z, const void *extra, size_t extraBytes, void *dExtra, Fill fill) {
  const int nF = f->nF;
  unsigned char *h = nullptr;
  int k = 0;
  { const int rc = ring_acquire(f, f->bStage, &h, &k); if (rc != RFSGPU_OK) return rc; }
  Rec *hf = reinterpret_cast<Rec *>(h);
  Params *hp = reinterpret_cast<Params *>(h + (size_t)nF * sizeof(Rec));
  double *hz = reinterpret_cast<double *>(h + (size_t)nF * (sizeof(Rec) + sizeof(Params)));
  if (f->bParamsDirty) {
    for (int b = 0; b < nF; b++) hp[b] = f->bParamsHost[b] = batch_params(f, b);
    HIPCHK(hipMemcpyAsync(f->dBParams, hp, (size_t)nF * sizeof(Params), hipMemcpyHostToDevice, f->stream));
    f->bParamsDirty = false;
  }
  int zOff = 0;
  const int zd = f->D;     // doubles per measurement (3: a batch of Victoria Park filters)
  for (int b = 0; b < nF; b++) {
    Rec &T = hf[b];
    memset(&T, 0, sizeof T);
    T.nZ = n_z[b];
    T.zOff = zOff;
    fill(T, b);
    if (n_z[b] > 0) memcpy(hz + zOff, z + (size_t)b * RFSGPU_MAX_Z * zd, (size_t)n_z[b] * zd * sizeof(double));
    zOff += zd * n_z[b];
  }
  HIPCHK(hipMemcpyAsync(dRec, hf, (size_t)nF * sizeof(Rec), hipMemcpyHostToDevice, f->stream));
  if (zOff) HIPCHK(hipMemcpyAsync(f->dBZ, hz, (size_t)zOff * sizeof(double), hipMemcpyHostToDevice, f->stream));
  if (extra) {
    void *he = hz + (size_t)nF * RFSGPU_MAX_Z * zd;
    memcpy(he, extra, extraBytes);
    HIPCHK(hipMemcpyAsync(dExtra, he, extraBytes, hipMemcpyHostToDevice, f->stream));
  }
  HIPCHK(hipEventRecord(f->bStage.ev[k], f->stream));
  return RFSGPU_OK;
}
// The Params table alone, when it is behind the configuration (a sensed cycle: the records and sets are on the device already)
static int batch_push_params(rfsgpu_filter *f) {
  if (!f->bParamsDirty) return RFSGPU_OK;
  unsigned char *h = nullptr;
  int k = 0;
  { const int rc = ring_acquire(f, f->bStage, &h, &k); if (rc != RFSGPU_OK) return rc; }
  Params *hp = reinterpret_cast<Params *>(h + (size_t)f->nF * sizeof(BatchFilter));     // (where batch_push_tables keeps it in the block)
  for (int b = 0; b < f->nF; b++) hp[b] = f->bParamsHost[b] = batch_params(f, b);
  HIPCHK(hipMemcpyAsync(f->dBParams, hp, (size_t)f->nF * sizeof(Params), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipEventRecord(f->bStage.ev[k], f->stream));
  f->bParamsDirty = false;
  return RFSGPU_OK;
}
// The records of a sensed FastSLAM / multi-hypothesis cycle (fastslam_sensed.h): the Params table when it is behind, the template table
// when a filter's static part has changed since the device got it (fill(record, b) writes that part, as it does for batch_push_tables),
// then the one launch that makes dRec from the sensor's records.  call: the multi-hypothesis cycle's draw counter.
template <class Rec, class Fill>
static int batch_sensed_records(rfsgpu_filter *f, Rec *dRec, unsigned long long call, Fill fill) {
  typedef FsSensedTemplate<Rec> Tmpl;
  static_assert(sizeof(Tmpl) <= sizeof(Rec) + sizeof(Params), "a block of the staging ring holds the template table");
  const int nF = f->nF;
  int rc = batch_push_params(f);     // (first: a record's pfaNum comes from bParamsHost)
  if (rc != RFSGPU_OK) return rc;
  std::vector<unsigned char> now((size_t)nF * sizeof(Tmpl), 0);     // (zeroed: the padding is compared and travels too)
  Tmpl *t = reinterpret_cast<Tmpl *>(now.data());
  for (int b = 0; b < nF; b++) {
    fill(t[b].rec, b);
    t[b].rec.F.pfa = 0.0;     // (derived on the device, like nZ, zOff, prune and u01, which fill leaves at zero)
    t[b].pfaNum = fs_pfa_num(f->bParamsHost[b], 2);
    t[b].pruneThr = f->bFs[b].pruningMeasurementsThreshold;
  }
  if (now != f->bFsTmplHost) {
    unsigned char *h = nullptr;
    int k = 0;
    if ((rc = ring_acquire(f, f->bStage, &h, &k)) != RFSGPU_OK) return rc;
    memcpy(h, now.data(), now.size());
    HIPCHK(hipMemcpyAsync(f->dFsTmpl, h, now.size(), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipEventRecord(f->bStage.ev[k], f->stream));
    f->bFsTmplHost.swap(now);
  }
  fs_sensed_records_kernel<Rec><<<(nF + 63) / 64, 64, 0, f->stream>>>(reinterpret_cast<const Tmpl *>(f->dFsTmpl), f->dBFilt, dRec, f->dBMotion, nF, call,
                                                                      batch_is_mh(f) ? f->dFsLastNZ : nullptr);
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
static int batch_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, int normalize);
static int batch_fs_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, int normalize,
                               const double *scan = nullptr, int n_scan = 0);
static int batch_mh_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, const double *u01,
                               unsigned long long call, const double *scan = nullptr, int n_scan = 0);
static int batch_push_motion(rfsgpu_filter *f);
static int batch_resample_core(rfsgpu_filter *f, const BatchCall &C, const int *n_z, unsigned long long call, bool stageIn = true);
static int batch_enter_dev_route(rfsgpu_filter *f);
static int batch_last_resample_core(rfsgpu_filter *f, unsigned char *fired, int *src_slot, double *n_eff);
static int batch_propagate_core(rfsgpu_filter *f, const double *u, const double *pin_pose, const unsigned char *pin, const BatchPropIn *devRow, unsigned long long call);
static int batch_sense_core(rfsgpu_filter *f, const double *gt_pose, const double *devPose, unsigned long long call);
extern "C" {
// The host's new poses / covariances of a batch by copy command, through a block of the staging ring (batch_handle_wide has the stride)
static int batch_push_poses(rfsgpu_filter *f, const double *x, const double *x_cov, int cov_stride) {
  double *hx = nullptr;
  int ks = 0;
  int rc = ring_acquire(f, f->stage, &hx, &ks);
  if (rc != RFSGPU_OK) return rc;
  if ((rc = push_poses(f, hx, f->B.pose, x, x_cov, cov_stride)) != RFSGPU_OK) return rc;
  HIPCHK(hipEventRecord(f->stage.ev[ks], f->stream));
  return RFSGPU_OK;
}
// ... and, on a batch of Victoria Park filters, the call's scan with them: poses (when given) and scan through one block of the
// staging ring, the scan at h + Ncap * 22 (rfsgpu_set_step_inputs_async's layout); it becomes the scan the batch holds.  No scan:
// batch_push_poses, when there are poses.
static int batch_push_poses_scan(rfsgpu_filter *f, const double *x, const double *x_cov, int cov_stride, const double *scan, int n_scan) {
  if (!scan) return x ? batch_push_poses(f, x, x_cov, cov_stride) : RFSGPU_OK;
  double *h = nullptr;
  int ks = 0;
  int rc = ring_acquire(f, f->stage, &h, &ks);
  if (rc != RFSGPU_OK) return rc;
  if (x && (rc = push_poses(f, h, f->B.pose, x, x_cov, cov_stride)) != RFSGPU_OK) return rc;
  double *hs = h + (size_t)f->Ncap * 22;
  memcpy(hs, scan, (size_t)n_scan * sizeof(double));
  HIPCHK(hipMemcpyAsync(f->B.scan, hs, (size_t)n_scan * sizeof(double), hipMemcpyHostToDevice, f->stream));
  f->B.nScan = n_scan;
  HIPCHK(hipEventRecord(f->stage.ev[ks], f->stream));
  return RFSGPU_OK;
}
// Whether the call's scan or the one the batch holds can serve a Victoria Park cycle, under the call's own prefix
static int batch_check_scan(rfsgpu_filter *f, const BatchCall &C, const double *scan, int n_scan) {
  if (scan && (n_scan < 2 || n_scan > RFSGPU_VP_MAX_SCAN)) return batch_fail(f, C, "laser scan size out of range (2 ... RFSGPU_VP_MAX_SCAN beams)");
  if (!scan && f->B.nScan < 2) return batch_fail(f, C, "the batch has not been given a laser scan (rfsgpu_set_laser_scan, or this call's scan)");
  return RFSGPU_OK;
}
// The draws of a multi-hypothesis cycle call, one per filter
static int batch_check_u01(rfsgpu_filter *f, const BatchCall &C, int b, const double *u01) {
  if (u01[b] >= 0.0 && u01[b] < 1.0) return RFSGPU_OK;
  return batch_fail(f, C, "filter " + std::to_string(b) + ": u01 must lie in [0, 1)");
}
// The host's bookkeeping at the end of a cycle core, the launches enqueued.  n_z null: a sensed cycle, whose counts stay on the device.
// flipCur: the chain wrote the other slab and has not flipped `cur` itself (the Victoria Park RB-PHD cycle: only with an update).
// mh: a multi-hypothesis cycle -- the counts are kept for rfsgpu_batch_fastslam_last_cycle as well, resampleOccured_ is the device's
// (mhb_resolve) and, the resampling being inside the cycle, no sensed resampling may follow.
static void batch_cycle_done(rfsgpu_filter *f, const int *n_z, bool flipCur, bool mh, long long t0) {
  const bool sensed = n_z == nullptr;
  if (flipCur) f->cur ^= 1;   // (filters without an update had their mixture moved to the new slab by the step kernel)
  if (!sensed)
    for (int b = 0; b < f->nF; b++) {
      if (mh) f->mhbLastNZ[b] = n_z[b];
      if (n_z[b] > 0) { f->bNZ[b] = n_z[b]; if (!mh) f->bResampled[b] = 0; }
    }
  f->bSenseFresh = false;     // (either kind of cycle: the next sensed cycle needs a sense call of its own)
  f->bSensedTail = sensed && !mh;
  if (!sensed) f->bScanHeld = false;     // (the host's sets lie over the sensor's)
  f->holes = false;
  f->timing.mapUpdate_cpu += now_ns() - t0;
}

int rfsgpu_create_batch(rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int device_id, int gm_capacity) {
  if (!out) return RFSGPU_ERR_INVALID;
  *out = nullptr;
  if ((model != RFSGPU_MODEL_RNGBRG_2D && model != RFSGPU_MODEL_VICTORIAPARK_3D) || n_filters < 1 || n_per_filter < 1 || (long long)n_filters * n_per_filter > (1 << 24)) return RFSGPU_ERR_INVALID;
  rfsgpu_filter *f = nullptr;
  int rc = rfsgpu_create(&f, model, n_filters * n_per_filter, device_id, gm_capacity);
  if (rc != RFSGPU_OK) return rc;
  f->batch = true;
  f->nF = n_filters;
  f->nPer = n_per_filter;
  const size_t zd = (size_t)f->D;     // doubles per measurement in the sets' tables
  batch_born(f);
  f->bVp.assign(n_filters, f->vp); f->bVpClutter.assign(n_filters, 0.0);
  f->bCfg.resize(n_filters); f->bRb.resize(n_filters); f->bKf.resize(n_filters); f->bQ.assign((size_t)9 * n_filters, 0.0);
  f->bNZ.assign(n_filters, 0);
  f->bResampled.assign(n_filters, 0);
  f->bFs.resize(n_filters);
  for (auto &c : f->bFs) rfsgpu_default_fastslam_config(&c);
  f->bParamsHost.resize(n_filters);
  f->bStage.bytes = batch_stage_bytes(f);
  f->bLoop.bytes = (size_t)n_filters * std::max(sizeof(BatchMotion), std::max(sizeof(BatchPropIn), sizeof(BatchResIn)));
  if (f->D == 3) f->bLoop.bytes = std::max(f->bLoop.bytes, std::max((size_t)n_filters * sizeof(VpBatchMotion), sizeof(VpBatchRun)));
  f->bLoop.depth = 8;
  batch_set_all(f);
  bool ok = true;
  ok &= hipMalloc(&f->dBFilt, (size_t)n_filters * sizeof(BatchFilter)) == hipSuccess;
  ok &= hipMalloc(&f->dBParams, (size_t)n_filters * sizeof(Params)) == hipSuccess;
  ok &= hipMalloc(&f->dFsFilt, (size_t)n_filters * sizeof(FsBatchFilter)) == hipSuccess;
  ok &= hipMalloc(&f->dBZ, (size_t)n_filters * RFSGPU_MAX_Z * zd * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->dBZPrev, (size_t)n_filters * RFSGPU_MAX_Z * zd * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->dBSums, (size_t)n_filters * 2 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->dBErrFilter, 2 * sizeof(int)) == hipSuccess;
  if (ok) { const int none[2] = {INT_MAX, INT_MAX}; ok &= hipMemcpy(f->dBErrFilter, none, sizeof none, hipMemcpyHostToDevice) == hipSuccess; }
  ok &= hipMalloc(&f->dBMaskTmp, (size_t)f->Ncap * sizeof(unsigned long long)) == hipSuccess;
  ok &= hipMalloc(&f->dBInhSrc, (size_t)f->Ncap * sizeof(int)) == hipSuccess;
  if (ok) ok &= hipMemset(f->dBZPrev, 0, (size_t)n_filters * RFSGPU_MAX_Z * zd * sizeof(double)) == hipSuccess;
  if (ok) ok &= hipMemset(f->dBSums, 0, (size_t)n_filters * 2 * sizeof(double)) == hipSuccess;
  // the device loop's tables (batch_loop.h)
  f->bMotionSet.assign(n_filters, 0); f->bResSet.assign(n_filters, 0);
  f->bMotion.assign(n_filters, BatchMotion{});
  f->bEffN.assign((size_t)2 * n_filters, 0.0);
  ok &= hipMalloc(&f->dBMotion, (size_t)n_filters * sizeof(BatchMotion)) == hipSuccess;
  ok &= hipMalloc(&f->dBPropIn, (size_t)n_filters * sizeof(BatchPropIn)) == hipSuccess;
  ok &= hipMalloc(&f->dBResIn, (size_t)n_filters * sizeof(BatchResIn)) == hipSuccess;
  ok &= hipMalloc(&f->BL.counters, (size_t)n_filters * 2 * sizeof(long long)) == hipSuccess;
  ok &= hipMalloc(&f->BL.nResamples, (size_t)n_filters * sizeof(long long)) == hipSuccess;
  ok &= hipMalloc(&f->BL.resampled, (size_t)n_filters * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->BL.fired, (size_t)n_filters * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->BL.nEff, (size_t)n_filters * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->BL.plan, (size_t)f->Ncap * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->BL.pid, (size_t)f->Ncap * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->BL.ppid, (size_t)f->Ncap * sizeof(int)) == hipSuccess;
  if (ok) ok &= hipMemset(f->BL.counters, 0, (size_t)n_filters * 2 * sizeof(long long)) == hipSuccess;
  if (ok) ok &= hipMemset(f->BL.nResamples, 0, (size_t)n_filters * sizeof(long long)) == hipSuccess;
  if (ok) ok &= hipMemset(f->BL.resampled, 0, (size_t)n_filters * sizeof(int)) == hipSuccess;
  if (ok) ok &= hipMemset(f->BL.fired, 0, (size_t)n_filters * sizeof(int)) == hipSuccess;
  if (ok) ok &= hipMemset(f->BL.nEff, 0, (size_t)n_filters * sizeof(double)) == hipSuccess;
  if (f->D == 3) {     // the device route of a Victoria Park batch (vp_batch_loop.h)
    f->bVpMotion.assign(n_filters, VpBatchMotion{});
    ok &= hipMalloc(&f->dBVpMotion, (size_t)n_filters * sizeof(VpBatchMotion)) == hipSuccess;
    ok &= hipMalloc(&f->dBVpRun, sizeof(VpBatchRun)) == hipSuccess;
    ok &= hipMalloc(&f->dBVpWalk, (size_t)(VBW_FILTER + n_filters) * sizeof(int)) == hipSuccess;
    if (ok) ok &= hipMemset(f->dBVpRun, 0, sizeof(VpBatchRun)) == hipSuccess;
    if (ok) ok &= hipMemset(f->dBVpWalk, 0, (size_t)(VBW_FILTER + n_filters) * sizeof(int)) == hipSuccess;
  }
  // the sensor's tables (batch_sensor.h)
  f->bSensorSet.assign(n_filters, 0);
  f->bSensorMaxNz.assign(n_filters, 0);
  f->bSensorCaps.assign((size_t)2 * n_filters, -1);
  f->bTruthSet.assign(n_filters, 0);
  f->bTruth.assign(n_filters, BatchTruth{});
  ok &= hipMalloc(&f->dBSensor, (size_t)n_filters * sizeof(BatchSensor)) == hipSuccess;
  ok &= hipMalloc(&f->dBSensorLm, (size_t)n_filters * SENSOR_MAX_LANDMARKS * 2 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->dBSensorPose, (size_t)n_filters * 3 * sizeof(double)) == hipSuccess;
  ok &= hipMalloc(&f->dBSensorCaps, (size_t)n_filters * 2 * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->dBSensorPrev, (size_t)n_filters * sizeof(int)) == hipSuccess;
  ok &= hipMalloc(&f->dBSensorErrFilter, sizeof(int)) == hipSuccess;
  if (ok) ok &= hipMemset(f->dBSensor, 0, (size_t)n_filters * sizeof(BatchSensor)) == hipSuccess;
  if (ok) ok &= hipMemset(f->dBSensorPrev, 0, (size_t)n_filters * sizeof(int)) == hipSuccess;
  if (ok) { const int none = INT_MAX; ok &= hipMemcpy(f->dBSensorErrFilter, &none, sizeof(int), hipMemcpyHostToDevice) == hipSuccess; }
  if (!ok) { rfsgpu_destroy(f); return RFSGPU_ERR_HIP; }
  *out = f;
  return RFSGPU_OK;
}
int rfsgpu_n_filters(const rfsgpu_filter *f) { return f ? (f->batch ? f->nF : 1) : -1; }
int rfsgpu_batch_configure(rfsgpu_filter *f, int filter, const rfsgpu_filter_config *cfg, const rfsgpu_rngbrg_config *model, const rfsgpu_kf_config *kf,
                           const double *lmk_Q) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, filter);
  if (rc != RFSGPU_OK) return rc;
  if (filter < 0) return fail(f, RFSGPU_ERR_INVALID, "batch_configure: filter index out of range");
  if (f->model != RFSGPU_MODEL_RNGBRG_2D) return fail(f, RFSGPU_ERR_INVALID, "batch_configure on a batch created for another model (rfsgpu_batch_configure_vp)");
  if (cfg && cfg->birthGaussianMeasurementCountThreshold != 1u)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_configure: a filter batch takes immediate births only (birthGaussianMeasurementCountThreshold 1)");
  if (cfg) f->bCfg[filter] = *cfg;
  if (model) f->bRb[filter] = *model;
  if (kf) f->bKf[filter] = *kf;
  if (lmk_Q) memcpy(&f->bQ[(size_t)9 * filter], lmk_Q, 4 * sizeof(double));
  f->bParamsDirty = true;
  return RFSGPU_OK;
}
// The same for a filter of a Victoria Park batch: every birth threshold is allowed (the candidate lists are per slot, as on a handle).
// lmk_Q: 3x3, row-major.  The filter's clutter density stays what the last scan made it until the next one, as rfsgpu_set_model_victoriapark leaves it on a handle.
int rfsgpu_batch_configure_vp(rfsgpu_filter *f, int filter, const rfsgpu_filter_config *cfg, const rfsgpu_vp_config *model, const rfsgpu_kf_config *kf,
                              const double *lmk_Q) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, filter);
  if (rc != RFSGPU_OK) return rc;
  if (filter < 0) return fail(f, RFSGPU_ERR_INVALID, "batch_configure_vp: filter index out of range");
  if (f->model != RFSGPU_MODEL_VICTORIAPARK_3D) return fail(f, RFSGPU_ERR_INVALID, "batch_configure_vp on a batch created for another model (rfsgpu_batch_configure)");
  if (model && (model->nPd < 1 || model->nPd > RFSGPU_VP_MAX_PD)) return fail(f, RFSGPU_ERR_INVALID, "batch_configure_vp: Pd table size out of range");
  if (cfg) f->bCfg[filter] = *cfg;
  if (model) f->bVp[filter] = *model;
  if (kf) f->bKf[filter] = *kf;
  if (lmk_Q) memcpy(&f->bQ[(size_t)9 * filter], lmk_Q, 9 * sizeof(double));
  f->bParamsDirty = true;
  return RFSGPU_OK;
}

// One predict + update cycle of every filter (rfsgpu_cycle_async per filter, in one launch chain).  z: [n_filters][RFSGPU_MAX_Z][2],
// n_z: [n_filters]; a filter with n_z 0 is not updated (its predict part runs; its weights are summed / divided as asked).
int rfsgpu_batch_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z,
                             int normalize) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_cycle_async", ON_MH_BATCH);
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_cycle_async", ON_VP_BATCH);
  if ((rc = batch_check_call(f, BATCH_CYCLE, predict, x_cov, cov_stride, n_z)) != RFSGPU_OK) return rc;
  for (int b = 0; b < f->nF; b++) {
    if ((rc = batch_check_filter(f, BATCH_CYCLE, b, z, n_z)) != RFSGPU_OK) return rc;
    if (f->bCfg[b].birthGaussianMeasurementCountThreshold != 1u)
      return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_cycle: a filter batch takes immediate births only (birthGaussianMeasurementCountThreshold 1)");
  }
  if (f->bSteps == STEPS_FASTSLAM)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_cycle: this batch steps FastSLAM filters (rfsgpu_batch_set_fastslam_config or rfsgpu_batch_fastslam_cycle_async has run): a batch is of one kind");
  if (f->bSensed)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_cycle: this batch has run a sensed cycle (rfsgpu_batch_cycle_sensed_async): the count of each filter's last update lives on the device, the host-fed cycle no longer knows it");
  batch_decide(f, STEPS_RBPHD);
  return batch_cycle_core(f, predict, x, x_cov, cov_stride, z, n_z, normalize);
}
// eval_cap() of filter b's configuration, as its BatchFilter record carries it
static int batch_eval_cap(const rfsgpu_filter *f, int b) {
  int c = f->bCfg[b].importanceWeightingEvalPointCount;
  if (c < 0 || c > RFSGPU_MAX_EVAL) c = RFSGPU_MAX_EVAL;
  return c < 1 ? 1 : c;
}
// The cycle behind rfsgpu_batch_cycle_async (n_z given: the host's sets and records go to the device first) and
// rfsgpu_batch_cycle_sensed_async (n_z null: the sets and records are where the last rfsgpu_batch_sense_async left them, and the launch
// is sized for the sensors' largest max_nz).  The arguments have been checked.
static int batch_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, int normalize) {
  const bool sensed = n_z == nullptr;
  const int nF = f->nF, nPer = f->nPer;
  int rc = RFSGPU_OK, nZmax = 0, ecMax = 1;
  // (a sensed cycle: the step kernel takes nZ and evalCap from the records the sense call wrote, so the launch is sized by what that
  //  call could write; rfsgpu_batch_cycle_sensed_async has checked that the sensors and the configuration still say the same)
  if (sensed) { nZmax = f->bSenseNzMax; ecMax = f->bSenseEcMax; }
  else for (int b = 0; b < nF; b++) nZmax = std::max(nZmax, n_z[b]);
  hipSetDevice(f->device);
  long long t0 = now_ns();
  batch_handle_wide(f, x, x_cov, cov_stride);   // (the pose covariance stride: handle-wide, as rfsgpu_cycle_async sets it)
  // the reference's lazy birth-state copy after a resampling (birth.h): with immediate births only the unused-measurement mask moves.
  // A slot copies from a HIGHER slot what that slot held before this predict, and from a LOWER slot what that one holds after its own
  // birth step: nothing once that filter has had an update (its births consume the whole mask), else what it inherited in turn.
  ensure_ids(f);
  std::vector<int> src;
  if (predict == 1 && !f->bDevRoute) {     // (the device route: batch_inherit_dev_kernel below, from the ids on the device)
    for (int b = 0; b < nF; b++) {
      if (!f->bResampled[b]) continue;
      const int lo = b * nPer, hi = lo + nPer;
      for (int k = lo; k < hi; k++) {
        int p = f->ppid[k];
        if (p < lo || p >= hi) p = k;
        if (p == k && src.empty()) continue;
        if (src.empty()) { src.resize(f->N); for (int q = 0; q < f->N; q++) src[q] = q; }
        // (a lower slot's birth step -- predict_map_particle, immediate births -- empties its mask only when the filter has had an
        //  update; before that the lower slot still holds what it inherited)
        src[k] = p > k ? p : (p == k ? k : (f->bNZ[b] > 0 ? -1 : src[p]));
      }
    }
  }
  // per-cycle tables (the host route's inheritance table at their tail)
  if (!sensed) for (int b = 0; b < nF; b++) ecMax = std::max(ecMax, batch_eval_cap(f, b));
  if (sensed) rc = batch_push_params(f);
  else rc = batch_push_tables(f, f->dBFilt, z, n_z, src.empty() ? nullptr : src.data(), (size_t)f->N * sizeof(int), f->dBInhSrc, [&](BatchFilter &F, int b) {
    F.nZprev = f->bNZ[b];
    F.evalCap = batch_eval_cap(f, b);
    F.useW = f->bCfg[b].useClusterProcess ? 0 : 1;
  });
  if (rc != RFSGPU_OK) return rc;
  if (!src.empty()) {
    HIPCHK(hipMemcpyAsync(f->dBMaskTmp, f->B.unusedMask, (size_t)f->N * sizeof(unsigned long long), hipMemcpyDeviceToDevice, f->stream));
    batch_inherit_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.unusedMask, f->dBMaskTmp, f->dBInhSrc, f->N);
  }
  if (f->bDevRoute) {
    batch_inherit_dev_kernel<<<nF, BATCH_LOOP_THREADS, 0, f->stream>>>(f->B.unusedMask, f->BL.ppid, f->BL.resampled, f->dBFilt, nPer, predict == 1 ? 1 : 0,
                                                                           sensed ? f->dBSensorPrev : nullptr);
    HIPCHK(hipGetLastError());
  }
  // the host's new poses / covariances, pulled by the step kernel from a slot of the staging ring (rfsgpu_cycle_async's form)
  StepPredict sp = NO_HEAD;
  sp.mode = predict < 0 ? 0 : (predict ? 2 : 1);
  sp.birthPose = f->bBirthAlt ? f->poseAlt : f->B.pose;   // after rfsgpu_batch_propagate_async the births still see the poses from before it
  f->bBirthAlt = false;
  int ks = -1;
  if (x) {
    double *hx = nullptr;
    if ((rc = ring_acquire(f, f->stage, &hx, &ks)) != RFSGPU_OK) return rc;
    const bool pullCov = x_cov && cov_stride == 9;
    sp.inPacked = hx;
    sp.inMask = 1 | (pullCov ? 2 : 0);
    for (int i = 0; i < f->N; i++) {
      double *d = hx + (size_t)13 * i;
      d[0] = x[3 * i]; d[1] = x[3 * i + 1]; d[2] = x[3 * i + 2];
      if (pullCov) memcpy(d + 3, x_cov + (size_t)9 * i, 9 * sizeof(double));
    }
    if ((rc = push_pose_cov(f, hx + (size_t)f->Ncap * 13, x_cov, cov_stride, pullCov)) != RFSGPU_OK) return rc;
  }
  BatchArg A{f->dBFilt, f->dBParams, f->dBZ, f->dBZPrev, f->dBSums, f->dBErrFilter, nF, nPer};
  // waves per particle and phase priorities: the single handle's rule (step_variant) for the whole launch, LDS sized for the batch's
  // largest evalCap and set (every filter's own layout lies inside it)
  const StepVariant sv = step_variant(f->cap, ecMax, nZmax, f->N, f->nCU, f->stepWppOverride, -1);
  const int wpp = sv.wpp, phasePrio = sv.phasePrio;
  const size_t lds = sv.ldsBytes;
  f->lastStepVariant[0] = wpp; f->lastStepVariant[1] = phasePrio; f->lastStepVariant[2] = 5; f->lastStepVariant[3] = sp.mode ? 2 : (sp.inMask ? 3 : 1);
  f->bLastCycleLds = (long long)lds;
  if ((rc = vp_order_buffers(f)) != RFSGPU_OK) return rc;
  const StepLaunchOrder sloOn{f->vpOrderMode ? f->vpCost : nullptr, f->vpOrderMode ? f->vpOrder : nullptr}, sloOff{nullptr, nullptr};
  static const ZArg noZ{};
  (void)noZ;
#define BATCH_LAUNCH(WPPV, PRIO)                                                                                                      \
  do {                                                                                                                                \
    if (sp.mode || sp.inMask) {                                                                                                       \
      if ((rc = set_lds(f, (phd_step_fused_kernel<WPPV, PRIO, 5, true, true>), lds)) != RFSGPU_OK) return rc;                        \
      phd_step_fused_kernel<WPPV, PRIO, 5, true, true><<<f->N, WPPV * 64, lds, f->stream>>>(f->B, f->P, f->cur, 0, 1, 1, f->Q, A, sp, PRIO ? sloOff : sloOn);   \
    } else {                                                                                                                          \
      if ((rc = set_lds(f, (phd_step_fused_kernel<WPPV, PRIO, 5, false, true>), lds)) != RFSGPU_OK) return rc;                       \
      phd_step_fused_kernel<WPPV, PRIO, 5, false, true><<<f->N, WPPV * 64, lds, f->stream>>>(f->B, f->P, f->cur, 0, 1, 1, f->Q, A, sp, PRIO ? sloOff : sloOn); \
    }                                                                                                                                 \
  } while (0)
  if (wpp == 2) { if (phasePrio) BATCH_LAUNCH(2, true); else BATCH_LAUNCH(2, false); }
  else { if (phasePrio) BATCH_LAUNCH(3, true); else BATCH_LAUNCH(3, false); }
#undef BATCH_LAUNCH
  HIPCHK(hipGetLastError());
  const bool sortCosts = !phasePrio && f->vpOrderMode == 2;
  const StepOrderArg sord{sortCosts ? f->vpCost : nullptr, f->vpOrder, f->N, f->vpCost + f->Ncap, f->vpParity};
  if (sortCosts) f->vpParity ^= 1;
  if (murty_launch_batch(f->Q, f->MS, f->B, f->stream, A, normalize, f->hJobCount, sord) != 0) return fail(f, RFSGPU_ERR_HIP, "batch post kernel launch failed");
  if (ks >= 0) HIPCHK(hipEventRecord(f->stage.ev[ks], f->stream));   // the pinned input slot is free once the step kernel has read it
  batch_cycle_done(f, n_z, true, false, t0);
  return RFSGPU_OK;
}
// ---- a batch of Victoria Park RB-PHD filters (vp_batch.h): rfsgpu_cycle_async of every filter's own handle in one launch chain --
// the per-cycle tables -> [inheritance walk +] births + static step (the BATCH forms of the general birth kernels) -> the host's
// poses and scan by copy command -> the BATCH form of the Victoria Park step -> the batch post kernel (sets kept per filter, Murty
// jobs, per-filter sums / division).  Nothing is read back.
static const BatchCall BATCH_VP_CYCLE{"batch_vp_cycle", -1, "RFSGPU_CYCLE_NO_PREDICT (-1), 0 (static step only) or 1 (births + static step)", "null measurement counts"};
static void launch_predict_kernels_vp_batch(rfsgpu_filter *f, int add_birth, const BirthLevel &LV, const BatchArg &A) {
  predict_map_general_batch_kernel<3, 4><<<(f->N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, add_birth ? 1 : 0, LV, A);
  if (add_birth) predict_map_long_batch_kernel<3, 2><<<(f->N + 1) / 2, 128, 0, f->stream>>>(f->B, f->cur, LV, A);   // (lists longer than a wavefront; the others exit at once)
}
static int batch_vp_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, const double *scan,
                               int n_scan, int normalize) {
  const int nF = f->nF, nPer = f->nPer, N = f->N;
  int rc = RFSGPU_OK, nZmax = 0, ecMax = 1;
  for (int b = 0; b < nF; b++) { nZmax = std::max(nZmax, n_z[b]); ecMax = std::max(ecMax, batch_eval_cap(f, b)); }
  hipSetDevice(f->device);
  long long t0 = now_ns();
  batch_handle_wide(f, x, x_cov, cov_stride);
  // the call's scan: every filter's clutter density on the host (it travels in the Params table), the beams by copy command below
  if (scan) scan_clutter(f, scan, n_scan);     // every filter's clutter density on the host (it travels in the Params table); the beams by copy command below
  // The reference's lazy copy of the per-slot birth state (RBPHDFilter.hpp:1005-1011) for the filters that have resampled since their
  // last update with measurements: predict_launch's parent and level tables, built across the batch.  A parent lies inside its filter's
  // block; a filter whose flag is clear keeps every slot its own parent, whatever idParent_ an older resampling left it.
  // On the device route (rfsgpu_batch_vp_resample_async has run) the ids and the flags are the device's: the tables are computed
  // there (vp_batch_loop.h) and the launches cannot depend on them -- predict_walk_device's chain, across the batch.
  const bool devWalk = f->bDevRoute;
  if (!devWalk) ensure_ids(f);
  bool walk = false;
  int maxLevel = 0;
  if (predict == 1 && !devWalk) {
    f->hInhParent.resize(N);
    f->hInhLevel.resize(N);
    for (int b = 0; b < nF; b++) {
      const int lo = b * nPer, hi = lo + nPer;
      for (int i = lo; i < hi; i++) {
        int p = f->bResampled[b] ? f->ppid[i] : i;
        if (p < lo || p >= hi) p = i;
        f->hInhParent[i] = p;
        f->hInhLevel[i] = (p >= i) ? 0 : f->hInhLevel[p] + 1;
        walk |= p != i;
        maxLevel = std::max(maxLevel, f->hInhLevel[i]);
      }
    }
  }
  rc = batch_push_tables(f, f->dBFilt, z, n_z, nullptr, 0, nullptr, [&](BatchFilter &F, int b) {
    F.nZprev = f->bNZ[b];
    F.evalCap = batch_eval_cap(f, b);
    F.useW = f->bCfg[b].useClusterProcess ? 0 : 1;
  });
  if (rc != RFSGPU_OK) return rc;
  const BatchArg A{f->dBFilt, f->dBParams, f->dBZ, f->dBZPrev, f->dBSums, f->dBErrFilter, nF, nPer};
  if (predict >= 0) {
    const BirthLevel all{nullptr, 0, 1};
    if (devWalk && predict == 1) {
      // the levels from the device's ids, the staging pair and level 0, a fixed RFSGPU_RBPHD_WALK_LEVELS of (copy, birth) pairs that
      // find no slot of theirs where the walk is shallower, and one workgroup per filter for whatever lies deeper
      if ((rc = inherit_buffers(f)) != RFSGPU_OK) return rc;
      vp_batch_walk_levels_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->BL.ppid, f->BL.resampled, N, nPer, RFSGPU_RBPHD_WALK_LEVELS, f->dInhParent, f->dInhLevel,
                                                                          f->dBVpWalk);
      birth_inherit_kernel<0><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
      birth_inherit_kernel<1><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
      launch_predict_kernels_vp_batch(f, 1, BirthLevel{f->dInhLevel, 0, 1}, A);
      for (int L = 1; L <= RFSGPU_RBPHD_WALK_LEVELS; L++) {
        birth_inherit_kernel<2><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, L);
        launch_predict_kernels_vp_batch(f, 1, BirthLevel{f->dInhLevel, L, 0}, A);
      }
      vp_batch_walk_tail_kernel<3><<<nF, BIRTH_TAIL_WAVES * 64, 0, f->stream>>>(f->B, f->cur, A, f->dInhParent, f->dInhLevel, RFSGPU_RBPHD_WALK_LEVELS + 1, f->dBVpWalk);
    } else if (!walk) {
      launch_predict_kernels_vp_batch(f, predict, all, A);
    } else {
      if ((rc = inherit_buffers(f)) != RFSGPU_OK) return rc;
      // (pageable host vectors: hipMemcpyAsync from them returns after the copy has been staged, so they may be reused at once)
      HIPCHK(hipMemcpyAsync(f->dInhParent, f->hInhParent.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, f->stream));
      HIPCHK(hipMemcpyAsync(f->dInhLevel, f->hInhLevel.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, f->stream));
      birth_inherit_kernel<0><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
      birth_inherit_kernel<1><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, 0);
      launch_predict_kernels_vp_batch(f, 1, BirthLevel{f->dInhLevel, 0, 1}, A);
      for (int L = 1; L <= maxLevel; L++) {     // (the deepest chain over all filters)
        birth_inherit_kernel<2><<<N, 128, 0, f->stream>>>(f->B, f->inhTmp, f->dInhParent, f->dInhLevel, L);
        launch_predict_kernels_vp_batch(f, 1, BirthLevel{f->dInhLevel, L, 0}, A);
      }
    }
    HIPCHK(hipGetLastError());
    f->candUsed = true;
  }
  // the host's new poses / covariances and the scan, behind the births (which happen at the poses the last update used)
  if (x) f->bBirthAlt = false;
  if ((rc = batch_push_poses_scan(f, x, x_cov, cov_stride, scan, n_scan)) != RFSGPU_OK) return rc;
  // two particles per workgroup where two waves' areas fit beside the scan (the handle's rule and its 64 KiB bound), else one
  const size_t scanB = vp_batch_scan_lds_bytes(f->B.nScan), stride = vp_batch_lds_stride(f->cap, ecMax, nZmax);
  const int wpb = scanB + 2 * stride <= (size_t)64 * 1024 ? 2 : 1;
  const size_t lds = scanB + (size_t)wpb * stride;
  f->lastStepVariant[0] = 1; f->lastStepVariant[1] = 0; f->lastStepVariant[2] = wpb; f->lastStepVariant[3] = 1;
  f->bLastCycleLds = (long long)lds;
  if ((rc = vp_order_buffers(f)) != RFSGPU_OK) return rc;
  // A cycle in which no filter has measurements is its predict and the sums (what rfsgpu_cycle_async does for an empty set): no step
  // launch, the mixtures stay in their slab.  The drivers use it for the birth predict at the head of a run of input messages.
  const bool anyUpdate = nZmax > 0;
  const int *vpOrd = f->vpOrderMode ? f->vpOrder : nullptr;
  const bool sortCosts = anyUpdate && f->vpOrderMode == 2;
  const StepOrderArg sord{sortCosts ? f->vpCost : nullptr, f->vpOrder, N, f->vpCost + f->Ncap, f->vpParity};
  if (sortCosts) f->vpParity ^= 1;
  if (!anyUpdate) {
    f->lastStepVariant[2] = 0; f->lastStepVariant[3] = 0;
  } else if (wpb == 2) {
    if ((rc = set_lds(f, vp_step_fused_batch_kernel<2>, lds)) != RFSGPU_OK) return rc;
    vp_step_fused_batch_kernel<2><<<(N + 1) / 2, 128, lds, f->stream>>>(f->B, f->cur, f->Q, A, nZmax, ecMax, f->vpCost, vpOrd);
  } else {
    if ((rc = set_lds(f, vp_step_fused_batch_kernel<1>, lds)) != RFSGPU_OK) return rc;
    vp_step_fused_batch_kernel<1><<<N, 64, lds, f->stream>>>(f->B, f->cur, f->Q, A, nZmax, ecMax, f->vpCost, vpOrd);
  }
  HIPCHK(hipGetLastError());
  if (murty_launch_batch<3>(f->Q, f->MS, f->B, f->stream, A, normalize, f->hJobCount, sord) != 0) return fail(f, RFSGPU_ERR_HIP, "batch post kernel launch failed");
  if (devWalk && anyUpdate) {     // resampleOccured_ of the filters this cycle updates falls on the device, behind the walk's read
    vp_batch_clear_flags_kernel<<<(nF + 255) / 256, 256, 0, f->stream>>>(f->BL.resampled, f->dBFilt, nF);
    HIPCHK(hipGetLastError());
  }
  batch_cycle_done(f, n_z, anyUpdate, false, t0);     // (never sensed: the device sensor does not serve the Victoria Park model, and its flags stay down)
  return RFSGPU_OK;
}
int rfsgpu_batch_vp_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z,
                                const double *scan, int n_scan, int normalize) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (f->D != 3)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_cycle: this batch steps 2-D filters (rfsgpu_batch_cycle_async, rfsgpu_batch_fastslam_cycle_async or rfsgpu_batch_fastslam_mh_cycle_async): the Victoria Park cycle needs a batch created with RFSGPU_MODEL_VICTORIAPARK_3D");
  if (batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_cycle: this is the RB-PHD cycle; a batch of Victoria Park multi-hypothesis FastSLAM filters (rfsgpu_create_batch_vp_mh) takes rfsgpu_batch_vp_fastslam_mh_cycle_async");
  if ((rc = batch_check_call(f, BATCH_VP_CYCLE, predict, x_cov, cov_stride, n_z)) != RFSGPU_OK) return rc;
  for (int b = 0; b < f->nF; b++)
    if ((rc = batch_check_filter(f, BATCH_VP_CYCLE, b, z, n_z)) != RFSGPU_OK) return rc;
  if ((rc = batch_check_scan(f, BATCH_VP_CYCLE, scan, n_scan)) != RFSGPU_OK) return rc;
  if (f->bSteps == STEPS_FASTSLAM)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_cycle: this batch steps FastSLAM filters (rfsgpu_batch_vp_serve_fastslam is on; its cycle is rfsgpu_batch_vp_fastslam_cycle_async): a batch is of one kind");
  batch_vp_cycle_ran(f);
  return batch_vp_cycle_core(f, predict, x, x_cov, cov_stride, z, n_z, scan, n_scan, normalize);
}

// ---- a batch of FastSLAM filters: FastSLAM::predict's map part + the single-hypothesis FastSLAM::update (include/FastSLAM.hpp:376-383,
// :387-706) of every filter in one launch chain -- [predict] -> associate + Kalman update + weights -> prune -> new landmarks -> per-filter
// sums / division.  Nothing synchronises: errors reach the host through the shared error word, as with rfsgpu_batch_cycle_async.
int rfsgpu_batch_set_fastslam_config(rfsgpu_filter *f, int filter, const rfsgpu_fastslam_config *cfg) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, filter);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f) && f->bSteps == STEPS_RBPHD) return refuse_on_kind(f, "rfsgpu_batch_set_fastslam_config", ON_VP_BATCH);     // (rfsgpu_batch_vp_serve_fastslam switches it on; rfsgpu_create_batch_vp_mh has it from creation)
  if (!cfg) return fail(f, RFSGPU_ERR_INVALID, "batch_set_fastslam_config: null configuration");
  const std::string who = filter < 0 ? std::string("every filter") : "filter " + std::to_string(filter);
  if (batch_is_vp_mh(f)) {     // (one hypothesis is the sparse single-hypothesis association on a handle, whose bits Murty with a limit of one does not give)
    if (cfg->maxNDataAssocHypotheses < 2u || cfg->maxNDataAssocHypotheses > (unsigned)FSMH_MAX_HYP) {
      f->err = "batch_set_fastslam_config: " + who + ": maxNDataAssocHypotheses must be in [2, 16] on a batch of Victoria Park multi-hypothesis filters (rfsgpu_create_batch_vp_mh); "
               "single-hypothesis filters belong to a batch with rfsgpu_batch_vp_serve_fastslam";
      return RFSGPU_ERR_UNSUPPORTED;
    }
  } else if (batch_is_mh(f)) {
    if (cfg->maxNDataAssocHypotheses < 1u || cfg->maxNDataAssocHypotheses > (unsigned)FSMH_MAX_HYP) {
      f->err = "batch_set_fastslam_config: " + who + ": maxNDataAssocHypotheses must be in [1, 16]";
      return RFSGPU_ERR_UNSUPPORTED;
    }
  } else if (cfg->maxNDataAssocHypotheses != 1u) {
    f->err = "batch_set_fastslam_config: " + who + ": maxNDataAssocHypotheses must be 1 on a filter batch (the multi-hypothesis update grows the particle set)";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  // (a batch of Victoria Park FastSLAM filters keeps candidate lists: both of its resampling routes move them with the particle)
  if (cfg->landmarkCandidateMeasurementCountThreshold != 1u && !batch_is_vp(f)) {
    f->err = "batch_set_fastslam_config: " + who + ": landmarkCandidateMeasurementCountThreshold must be 1 on a filter batch (landmark candidate lists would have to travel with a resampling)";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  if (f->bSteps == STEPS_RBPHD)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_set_fastslam_config: this batch steps RB-PHD filters (rfsgpu_batch_cycle_async has run): a batch is of one kind");
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) f->bFs[b] = *cfg;
  batch_decide(f, STEPS_FASTSLAM);      // an undecided batch is a FastSLAM batch from here on: the [metric] calls read the Gaussians' weights as log-odds
  return RFSGPU_OK;
}
int rfsgpu_batch_fastslam_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z,
                                      int normalize) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_fastslam_cycle_async", ON_VP_BATCH);
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_fastslam_cycle_async", ON_MH_BATCH);
  if ((rc = batch_check_call(f, BATCH_FS_CYCLE, predict, x_cov, cov_stride, n_z)) != RFSGPU_OK) return rc;
  const int nF = f->nF;
  for (int b = 0; b < nF; b++)
    if ((rc = batch_check_filter(f, BATCH_FS_CYCLE, b, z, n_z)) != RFSGPU_OK) return rc;
  if (f->bSteps == STEPS_RBPHD)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_cycle: this batch steps RB-PHD filters (rfsgpu_batch_cycle_async has run): a batch is of one kind");
  if (f->bSensed)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_cycle: this batch has run a sensed cycle (rfsgpu_batch_fastslam_cycle_sensed_async): its measurement counts live on the device, the host-fed cycle no longer knows them");
  batch_decide(f, STEPS_FASTSLAM);
  return batch_fs_cycle_core(f, predict, x, x_cov, cov_stride, z, n_z, normalize);
}
// ---- ... of Victoria Park filters: the switch that makes a batch created with RFSGPU_MODEL_VICTORIAPARK_3D a batch of FastSLAM filters,
// and its cycle (the D = 3 forms of the chain above; the scan as in rfsgpu_batch_vp_cycle_async).  Off at creation, so every refusal such
// a batch was published with stands until a caller asks.
static const BatchCall BATCH_VP_FS_CYCLE{"batch_vp_fastslam_cycle", -1, "RFSGPU_CYCLE_NO_PREDICT (-1), or 0 / 1 (the static landmark step; FastSLAM has no births)", "null measurement counts"};
int rfsgpu_batch_vp_serve_fastslam(rfsgpu_filter *f, int on) {
  CHECK_HANDLE(f);
  if (!batch_is_vp(f) || batch_is_mh(f))
    return refuse_not(f, "batch_vp_serve_fastslam: the switch is for a batch of Victoria Park filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D)");
  const BatchSteps want = on ? STEPS_FASTSLAM : STEPS_RBPHD;
  if (on && !batch_vp_may_step(f, want))
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_serve_fastslam: this batch steps RB-PHD filters (rfsgpu_batch_vp_cycle_async has run): a batch is of one kind");
  if (on && f->estServeVpBatch)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_serve_fastslam: this batch serves the [estimate] log of RB-PHD filters (rfsgpu_batch_vp_serve_estimates is on): switch that off first");
  if (!on && !batch_vp_may_step(f, want))
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_serve_fastslam: this batch steps FastSLAM filters (rfsgpu_batch_vp_fastslam_cycle_async has run): a batch is of one kind");
  f->bSteps = want;     // (FastSLAM: the device route's gates are the FastSLAM configuration's, batch_resample_core)
  return RFSGPU_OK;
}
int rfsgpu_batch_vp_fastslam_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z,
                                         const double *scan, int n_scan, int normalize) {
  CHECK_HANDLE(f);
  if (!batch_is_vp_fastslam(f))
    return refuse_not(f, "batch_vp_fastslam_cycle: the call serves a batch of Victoria Park FastSLAM filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D, then rfsgpu_batch_vp_serve_fastslam)");
  int rc = RFSGPU_OK;
  if ((rc = batch_check_call(f, BATCH_VP_FS_CYCLE, predict, x_cov, cov_stride, n_z)) != RFSGPU_OK) return rc;
  for (int b = 0; b < f->nF; b++)
    if ((rc = batch_check_filter(f, BATCH_VP_FS_CYCLE, b, z, n_z)) != RFSGPU_OK) return rc;
  if ((rc = batch_check_scan(f, BATCH_VP_FS_CYCLE, scan, n_scan)) != RFSGPU_OK) return rc;
  batch_vp_cycle_ran(f);
  return batch_fs_cycle_core(f, predict, x, x_cov, cov_stride, z, n_z, normalize, scan, n_scan);
}
// The cycle behind rfsgpu_batch_fastslam_cycle_async (n_z given: the host's sets and records go to the device first) and
// rfsgpu_batch_fastslam_cycle_sensed_async (n_z null: the sets are where the last rfsgpu_batch_sense_async left them, the records are
// made from that call's on the device).  The arguments have been checked.
// A batch of Victoria Park filters (rfsgpu_batch_vp_fastslam_cycle_async; never sensed): the D = 3 forms of the same chain; scan, when
// given, becomes the scan the batch holds, as in batch_vp_cycle_core.
static int batch_fs_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, int normalize,
                               const double *scan, int n_scan) {
  const bool sensed = n_z == nullptr;
  const int nF = f->nF, D = f->D;
  int rc = RFSGPU_OK;
  hipSetDevice(f->device);
  long long t0 = now_ns();
  if (!f->fsArena) HIPCHK(hipMalloc(&f->fsArena, (size_t)f->Ncap * fs_arena_bytes()));   // the Hungarian scratch of every slot of the batch, once
  batch_handle_wide(f, x, x_cov, cov_stride);
  if (scan) scan_clutter(f, scan, n_scan);     // every filter's clutter density on the host (it travels in the Params table); the beams by copy command below
  if (sensed) rc = batch_sensed_records(f, f->dFsFilt, 0ull, [&](FsBatchFilter &T, int b) {
    T.F = fs_params_of(f->bFs[b], f->bParamsHost[b], 2, 1);
    T.pruneT = f->bFs[b].mapExistencePruneThreshold;
  });
  else rc = batch_push_tables(f, f->dFsFilt, z, n_z, nullptr, 0, nullptr, [&](FsBatchFilter &T, int b) {
    T.F = fs_params_of(f->bFs[b], f->bParamsHost[b], D, n_z[b]);
    T.pruneT = f->bFs[b].mapExistencePruneThreshold;
    T.prune = ((unsigned)n_z[b] >= f->bFs[b].pruningMeasurementsThreshold) ? 1 : 0;
  });
  if (rc != RFSGPU_OK) return rc;
  if ((rc = batch_push_poses_scan(f, x, x_cov, cov_stride, scan, n_scan)) != RFSGPU_OK) return rc;
  f->bBirthAlt = false;      // (no births here: the poses from before a propagation are not needed)
  FsBatchArg A{f->dFsFilt, f->dBParams, f->dBZ, f->dBErrFilter, f->nPer, predict >= 0 ? 1 : 0};
  const size_t b2 = fs_batch_lds_bytes(f->cap, 2, D), b1 = fs_batch_lds_bytes(f->cap, 1, D);
  if (D == 3) {
    // two particles per workgroup where both waves' areas and Pd scratch fit the same 64 KiB, else one
    const size_t pdB = (VP_PD_SCRATCH_BYTES + 15) & ~(size_t)15;
    const int wpb = b2 + 2 * pdB <= 64 * 1024 ? 2 : 1;
    f->lastStepVariant[0] = 2; f->lastStepVariant[1] = 0; f->lastStepVariant[2] = wpb; f->lastStepVariant[3] = 1;
    f->bLastCycleLds = (long long)(wpb == 2 ? b2 + 2 * pdB : b1 + pdB);
    if (wpb == 2) {
      if ((rc = set_lds(f, (fs_associate_update_batch_kernel<2, 3>), b2)) != RFSGPU_OK) return rc;
      fs_associate_update_batch_kernel<2, 3><<<(f->N + 1) / 2, 128, b2, f->stream>>>(f->B, f->cur, f->fsArena, A);
    } else {
      if ((rc = set_lds(f, (fs_associate_update_batch_kernel<1, 3>), b1)) != RFSGPU_OK) return rc;
      fs_associate_update_batch_kernel<1, 3><<<f->N, 64, b1, f->stream>>>(f->B, f->cur, f->fsArena, A);
    }
  } else if (b2 <= 64 * 1024) {      // (the single handle's rule)
    if ((rc = set_lds(f, (fs_associate_update_batch_kernel<2, 2>), b2)) != RFSGPU_OK) return rc;
    fs_associate_update_batch_kernel<2, 2><<<(f->N + 1) / 2, 128, b2, f->stream>>>(f->B, f->cur, f->fsArena, A);
  } else {
    if ((rc = set_lds(f, (fs_associate_update_batch_kernel<1, 2>), b1)) != RFSGPU_OK) return rc;
    fs_associate_update_batch_kernel<1, 2><<<f->N, 64, b1, f->stream>>>(f->B, f->cur, f->fsArena, A);
  }
  HIPCHK(hipGetLastError());
  const size_t pb = gm_prune_lds_bytes_per_wave(f->cap);
  if ((rc = set_lds(f, (gm_prune_kernel<4, false, true, FsBatchArg>), 4 * pb)) != RFSGPU_OK) return rc;
  gm_prune_kernel<4, false, true, FsBatchArg><<<(f->N + 3) / 4, 256, 4 * pb, f->stream>>>(f->B, f->P, f->cur, f->cur ^ 1, A);
  f->cur ^= 1;     // (filters that do not prune this cycle had their mixtures moved to the new slab)
  if (D == 3) fs_new_landmarks_kernel<3, true, FsBatchArg><<<(f->N + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, A);
  else fs_new_landmarks_kernel<2, true, FsBatchArg><<<(f->N + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, A);
  fs_batch_post_kernel<<<nF, 256, 0, f->stream>>>(f->B.weight, A, f->dBSums, normalize, f->bDevRoute ? f->BL.resampled : nullptr);
  HIPCHK(hipGetLastError());
  batch_cycle_done(f, n_z, false, false, t0);     // (`cur` was flipped behind the prune)
  return RFSGPU_OK;
}
// ---- a batch of multi-hypothesis FastSLAM filters (fastslam_cycle.h, the kernels at its end) -------------------------------------
// rfsgpu_fastslam_cycle_async for every filter of the batch in one launch chain.  Filter b owns max_per_filter slots of which the
// first n_b are live; n_b, the overflow word, the counters, the plans and the ids are in the filter's own cycle block on the device.
static inline size_t mhb_bytes(const rfsgpu_filter *f) { return mhb_state_bytes(f->nF, f->nPer); }
static void mhb_view(const rfsgpu_filter *f, unsigned char *base, int b, FsCycleState &S) { mhb_state(base, f->nF, f->nPer, b, S); }
static int create_batch_mh_of(rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity);
int rfsgpu_create_batch_mh(rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity) {
  if (!out) return RFSGPU_ERR_INVALID;
  *out = nullptr;
  if (model == RFSGPU_MODEL_VICTORIAPARK_3D) return RFSGPU_ERR_UNSUPPORTED;    // (2-D range-bearing filters only; rfsgpu_create_batch_vp_mh)
  if (model != RFSGPU_MODEL_RNGBRG_2D) return RFSGPU_ERR_INVALID;
  return create_batch_mh_of(out, model, n_filters, n_per_filter, max_per_filter, device_id, gm_capacity);
}
// ... of Victoria Park filters: a kind of its own from creation (rfsgpu_batch_vp_fastslam_mh_cycle_async steps it)
int rfsgpu_create_batch_vp_mh(rfsgpu_filter **out, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity) {
  if (!out) return RFSGPU_ERR_INVALID;
  *out = nullptr;
  return create_batch_mh_of(out, RFSGPU_MODEL_VICTORIAPARK_3D, n_filters, n_per_filter, max_per_filter, device_id, gm_capacity);
}
static int create_batch_mh_of(rfsgpu_filter **out, int model, int n_filters, int n_per_filter, int max_per_filter, int device_id, int gm_capacity) {
  if (n_filters < 1 || n_per_filter < 1 || max_per_filter < n_per_filter) return RFSGPU_ERR_INVALID;
  if (max_per_filter > RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES) return RFSGPU_ERR_UNSUPPORTED;   // (the resampling workgroup holds one filter in LDS)
  rfsgpu_filter *f = nullptr;
  int rc = rfsgpu_create_batch(&f, model, n_filters, max_per_filter, device_id, gm_capacity);
  if (rc != RFSGPU_OK) return rc;
  batch_born_mh(f);
  f->nInitPer = n_per_filter;
  f->mhbLastNZ.assign(n_filters, 0);
  for (auto &c : f->bFs) c.nParticlesMax = 3 * n_per_filter;      // FastSLAM.hpp:250
  // the cycle blocks: every filter starts with n_per_filter particles whose ids are their slots within the filter
  const size_t bytes = mhb_bytes(f);
  bool ok = hipMalloc(&f->mhbBlock, bytes) == hipSuccess;
  ok &= hipHostMalloc(&f->hMhbBlock, bytes) == hipSuccess;
  ok &= hipMalloc(&f->dMhFilt, (size_t)n_filters * sizeof(MhBatchFilter)) == hipSuccess;
  if (ok) {
    memset(f->hMhbBlock, 0, bytes);
    f->pid.resize(f->Ncap); f->ppid.resize(f->Ncap);
    for (int b = 0; b < n_filters; b++) {
      FsCycleState H;
      mhb_view(f, f->hMhbBlock, b, H);
      H.w[FSC_N] = n_per_filter; H.w[FSC_NGROWN] = n_per_filter;
      for (int k = 0; k < max_per_filter; k++) {
        H.slotSrc[k] = k; H.plan[k] = k; H.pid[k] = k; H.ppid[k] = k;
        f->pid[(size_t)b * max_per_filter + k] = k; f->ppid[(size_t)b * max_per_filter + k] = k;
      }
    }
    ok &= hipMemcpy(f->mhbBlock, f->hMhbBlock, bytes, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) { rfsgpu_destroy(f); return RFSGPU_ERR_HIP; }
  *out = f;
  return RFSGPU_OK;
}
// The blocks come back: one stream-ordered copy into pinned memory, then the wait.  The ids and resampleOccured_ follow the device; a
// filter whose overflow word is up is reported once (the lowest such filter is named) and the words are cleared.
static int mhb_resolve(rfsgpu_filter *f) {
  if (!f->mhbPending) return RFSGPU_OK;
  f->mhbPending = false;
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(f->hMhbBlock, f->mhbBlock, mhb_bytes(f), hipMemcpyDeviceToHost, f->stream));
  if (f->mhbLastSensed)     // (the last cycle's counts are the device's own: the nZ of its records, in the same read-back)
    HIPCHK(hipMemcpyAsync(f->hFsLastNZ, f->dFsLastNZ, (size_t)f->nF * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  const int rc = check_device_errors(f);   // waits for the stream
  if (f->mhbLastSensed) memcpy(f->mhbLastNZ.data(), f->hFsLastNZ, (size_t)f->nF * sizeof(int));
  int first = -1;
  bool badCount = false;
  for (int b = 0; b < f->nF; b++) {
    FsCycleState H;
    mhb_view(f, f->hMhbBlock, b, H);
    memcpy(f->pid.data() + (size_t)b * f->nPer, H.pid, (size_t)f->nPer * sizeof(int));
    memcpy(f->ppid.data() + (size_t)b * f->nPer, H.ppid, (size_t)f->nPer * sizeof(int));
    f->bResampled[b] = H.w[FSC_RESAMPLED] ? 1 : 0;
    if (H.w[FSC_OVF] && first < 0) first = b;
    badCount |= H.w[FSC_N] < 1 || H.w[FSC_N] > f->nPer;
  }
  if (rc != RFSGPU_OK) {      // another device error comes first; an overflow word that is up stays up (its filter stays abandoned) and
    if (first >= 0) f->mhbPending = true;     // is reported by the next synchronising call
    return rc;
  }
  if (badCount) return fail(f, RFSGPU_ERR_HIP, "batch_fastslam_mh_cycle: the device returned a particle count outside [1, max_per_filter]");
  if (first >= 0) {
    HIPCHK(hipMemset2DAsync(f->mhbBlock + (size_t)24 * f->nF + sizeof(int) * FSC_OVF, sizeof(int) * FSC_WORDS, 0, sizeof(int), (size_t)f->nF, f->stream));
    f->err = "batch_fastslam_mh_cycle: filter " + std::to_string(first) + ": the particle copies of a multi-hypothesis update exceed max_per_filter (rfsgpu_create_batch_mh); "
             "that cycle of the filter and those enqueued behind it were abandoned for it, its state is the one before (the other filters' cycles completed)";
    return RFSGPU_ERR_CAPACITY;
  }
  return RFSGPU_OK;
}
int rfsgpu_batch_fastslam_mh_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z,
                                         const double *u01) {
  if (!f) return RFSGPU_ERR_INVALID;
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_mh_cycle: not a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh)");
  if (batch_is_vp(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_mh_cycle: this is the 2-D cycle; a batch of Victoria Park multi-hypothesis filters (rfsgpu_create_batch_vp_mh) takes rfsgpu_batch_vp_fastslam_mh_cycle_async");
  if ((rc = batch_check_call(f, BATCH_MH_CYCLE, predict, x_cov, cov_stride, u01 ? n_z : nullptr)) != RFSGPU_OK) return rc;
  const int nF = f->nF;
  for (int b = 0; b < nF; b++) {
    if ((rc = batch_check_filter(f, BATCH_MH_CYCLE, b, z, n_z)) != RFSGPU_OK) return rc;
    if ((rc = batch_check_u01(f, BATCH_MH_CYCLE, b, u01)) != RFSGPU_OK) return rc;
  }
  if (f->bSensed)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_mh_cycle: this batch has run a sensed cycle (rfsgpu_batch_fastslam_mh_cycle_sensed_async): its measurement counts live on the device, the host-fed cycle no longer knows them");
  return batch_mh_cycle_core(f, predict, x, x_cov, cov_stride, z, n_z, u01, 0ull);
}
// ... of Victoria Park filters (rfsgpu_create_batch_vp_mh): z [n_filters][RFSGPU_MAX_Z][3]; the scan as in rfsgpu_batch_vp_cycle_async.
static const BatchCall BATCH_VP_MH_CYCLE{"batch_vp_fastslam_mh_cycle", 0, "0 or 1 (the static landmark step; FastSLAM has no births)", "null measurement counts or draws"};
int rfsgpu_batch_vp_fastslam_mh_cycle_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z,
                                            const double *scan, int n_scan, const double *u01) {
  if (!f) return RFSGPU_ERR_INVALID;
  if (!batch_is_vp_mh(f)) {
    if (f->mhcPending || f->mhcStashedRc || f->mhbPending || f->rsPending || f->rcPending) { const int rcp = mhc_resolve(f); if (rcp != RFSGPU_OK) return rcp; }
    return refuse_not(f, "batch_vp_fastslam_mh_cycle: the call serves a batch of Victoria Park multi-hypothesis FastSLAM filters (rfsgpu_create_batch_vp_mh)");
  }
  int rc = RFSGPU_OK;
  if ((rc = batch_check_call(f, BATCH_VP_MH_CYCLE, predict, x_cov, cov_stride, u01 ? n_z : nullptr)) != RFSGPU_OK) return rc;
  const int nF = f->nF;
  for (int b = 0; b < nF; b++) {
    if ((rc = batch_check_filter(f, BATCH_VP_MH_CYCLE, b, z, n_z)) != RFSGPU_OK) return rc;
    if ((rc = batch_check_u01(f, BATCH_VP_MH_CYCLE, b, u01)) != RFSGPU_OK) return rc;
    if (f->bFs[b].maxNDataAssocHypotheses < 2u || f->bFs[b].maxNDataAssocHypotheses > (unsigned)FSMH_MAX_HYP) {
      f->err = "batch_vp_fastslam_mh_cycle: filter " + std::to_string(b) + ": maxNDataAssocHypotheses must be in [2, 16] (rfsgpu_batch_set_fastslam_config)";
      return RFSGPU_ERR_UNSUPPORTED;
    }
  }
  if ((rc = batch_check_scan(f, BATCH_VP_MH_CYCLE, scan, n_scan)) != RFSGPU_OK) return rc;
  return batch_mh_cycle_core(f, predict, x, x_cov, cov_stride, z, n_z, u01, 0ull, scan, n_scan);
}
// The cycle behind rfsgpu_batch_fastslam_mh_cycle_async (n_z, u01 given: the host's sets and records go to the device first) and
// rfsgpu_batch_fastslam_mh_cycle_sensed_async (n_z null: the sets are where the last rfsgpu_batch_sense_async left them, the records are
// made from that call's on the device, each filter's draw is the resampling draw of (its motion key, call)).  The arguments have been checked.
// A batch of Victoria Park filters (rfsgpu_batch_vp_fastslam_mh_cycle_async; never sensed): the D = 3 forms of the same chain, the
// candidate lists travelling with the copies of a filter whose previous cycle resampled and with every resampling; scan, when given,
// becomes the scan the batch holds, as in batch_fs_cycle_core.
static int batch_mh_cycle_core(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, const double *z, const int *n_z, const double *u01,
                               unsigned long long call, const double *scan, int n_scan) {
  const bool sensed = n_z == nullptr;
  const int nF = f->nF, N = f->N, stride = f->nPer, D = f->D;
  int rc = RFSGPU_OK;
  hipSetDevice(f->device);
  long long t0 = now_ns();
  const FsMhLayout L = fs_mh_layout();
  if (!f->mhArena) HIPCHK(hipMalloc(&f->mhArena, (size_t)N * L.total));          // every slot's table / Murty arena / assignments, once
  if (!f->mhcInts) HIPCHK(hipMalloc(&f->mhcInts, (size_t)4 * N * sizeof(int)));
  batch_handle_wide(f, x, x_cov, cov_stride);
  if (scan) scan_clutter(f, scan, n_scan);     // every filter's clutter density on the host (it travels in the Params table); the beams by copy command below
  // (the record's static part: one filler for both routes; nz 1 where the device derives pfa)
  auto fillStatic = [&](MhBatchFilter &T, int b, int nz) {
    const rfsgpu_fastslam_config &c = f->bFs[b];
    T.F = fs_params_of(c, f->bParamsHost[b], D, nz);
    T.pruneT = c.mapExistencePruneThreshold;
    T.kmax = (int)c.maxNDataAssocHypotheses;
    T.maxDiff = c.maxDataAssocLogLikelihoodDiff;
    T.effN = f->bResSet[b] ? f->bEffN[2 * (size_t)b] : f->nInitPer / 4.0;        // ParticleFilter.hpp:232
    T.effNPercent = f->bResSet[b] ? f->bEffN[2 * (size_t)b + 1] : 0.25;
    T.nInit = f->nInitPer;
    T.nMax = (int)c.nParticlesMax;
    T.minUpdates = (int)c.minUpdatesBeforeResample;
    T.minMeasurements = (int)c.minMeasurementsBeforeResample;
  };
  if (sensed) {
    if ((rc = batch_push_motion(f)) != RFSGPU_OK) return rc;     // (the keys of the draws)
    rc = batch_sensed_records(f, f->dMhFilt, call, [&](MhBatchFilter &T, int b) { fillStatic(T, b, 1); });
  } else {
    rc = batch_push_tables(f, f->dMhFilt, z, n_z, nullptr, 0, nullptr, [&](MhBatchFilter &T, int b) {
      fillStatic(T, b, n_z[b]);
      T.prune = ((unsigned)n_z[b] >= f->bFs[b].pruningMeasurementsThreshold) ? 1 : 0;
      T.u01 = u01[b];
    });
  }
  if (rc != RFSGPU_OK) return rc;
  if ((rc = batch_push_poses_scan(f, x, x_cov, cov_stride, scan, n_scan)) != RFSGPU_OK) return rc;     // (every slot of every block)
  f->bBirthAlt = false;
  FsCycleState S0;      // filter 0's view: its slot arrays are the batch's, [N] each, holding slots local to each filter's block
  mhb_view(f, f->mhbBlock, 0, S0);
  MhBatchArg A{f->dMhFilt, f->dBParams, f->dBZ, f->dBErrFilter, stride, predict, nF, S0.w, FSC_WORDS, FSC_N};
  MhBatchArg Acopy = A, Arenorm = A;
  Acopy.word = FSC_NCOPY;
  Arenorm.word = FSC_RENORM_N;
  int *dSlotHyp = f->mhcInts, *dSlotNH = dSlotHyp + N, *dDst = dSlotNH + N, *dSrc = dDst + N;
  fs_cycle_begin_batch_kernel<<<(nF + 63) / 64, 64, 0, f->stream>>>(f->mhbBlock, A, nF);
  if (predict && D == 3) fs_cycle_static_step3_batch_kernel<<<(N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, A);
  else if (predict) fs_cycle_static_step_batch_kernel<<<(N + 3) / 4, 256, 0, f->stream>>>(f->B, f->cur, A);
  if (D == 3) fs_mh_associate_kernel<3><<<N, 64 * FSMH_WAVES, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, 0, 0.0, f->mhArena, A);
  else fs_mh_associate_kernel<2><<<N, 64 * FSMH_WAVES, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, 0, 0.0, f->mhArena, A);
  fs_mh_plan_batch_kernel<<<nF, FS_CYCLE_THREADS, 0, f->stream>>>(f->mhArena, f->mhbBlock, dSlotHyp, dSlotNH, dDst, dSrc, A);
  if (D == 3) {     // the lists travel with the copies of a filter whose resampleOccured_ is up, read where the kernel runs (:551-553)
    MhBatchCopy Ac;
    static_cast<MhBatchArg &>(Ac) = Acopy;
    Ac.candWord = FSC_RESAMPLED;
    fs_mh_copy_kernel<<<N, 256, 0, f->stream>>>(f->B, f->cur, dDst, dSrc, 0, f->P.poseCovStride, Ac);
  } else fs_mh_copy_kernel<<<N, 256, 0, f->stream>>>(f->B, f->cur, dDst, dSrc, 0, f->P.poseCovStride, Acopy);
  fs_mh_split_weights_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, S0.slotSrc, dSlotNH, N, 0, A);
  fs_mh_split_weights_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, S0.slotSrc, dSlotNH, N, 1, A);
  if (D == 3) fs_mh_apply_kernel<3><<<N, 64, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, S0.slotSrc, dSlotHyp, f->mhArena, A);
  else fs_mh_apply_kernel<2><<<N, 64, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, S0.slotSrc, dSlotHyp, f->mhArena, A);
  HIPCHK(hipGetLastError());
  // the prune of the filters that prune this cycle (:611-612); the others' mixtures -- no measurements, below their
  // pruningMeasurementsThreshold, overflowed -- move unchanged to the other slab, because the batch flips `cur` as one
  const size_t pb = gm_prune_lds_bytes_per_wave(f->cap);
  if ((rc = set_lds(f, (gm_prune_kernel<4, false, true, MhBatchArg>), 4 * pb)) != RFSGPU_OK) return rc;
  gm_prune_kernel<4, false, true, MhBatchArg><<<(N + 3) / 4, 256, 4 * pb, f->stream>>>(f->B, f->P, f->cur, f->cur ^ 1, A);
  f->cur ^= 1;
  if (D == 3) fs_new_landmarks_kernel<3, true, MhBatchArg><<<(N + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, A);
  else fs_new_landmarks_kernel<2, true, MhBatchArg><<<(N + FS_NEWLM_WPB - 1) / FS_NEWLM_WPB, 64 * FS_NEWLM_WPB, 0, f->stream>>>(f->B, f->P, FsParams{}, f->cur, 0, A);
  // resampleWithMapCopy per filter, as rfsgpu_fastslam_cycle_async: normalisation, decision and plan, copies, and the second
  // normalisation of a resample() that returned false
  mhb_weight_sums_kernel<<<nF, 1024, 0, f->stream>>>(f->B.weight, f->dBSums, A);
  mhb_normalize_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, N, f->dBSums, A);
  fs_resample_shrink_batch_kernel<<<nF, FS_CYCLE_THREADS, 0, f->stream>>>(f->B.weight, f->mhbBlock, A);
  resample_gather_kernel<<<N, 256, 0, f->stream>>>(f->B, f->cur, S0.plan, f->P.poseCovStride, 0, A);     // (mapOnly 0: lists, mask and in-view count move with the particle)
  mhb_weight_sums_kernel<<<nF, 1024, 0, f->stream>>>(f->B.weight, f->dBSums, Arenorm);
  mhb_normalize_kernel<<<(N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, N, f->dBSums, Arenorm);
  HIPCHK(hipGetLastError());
  f->mhbLastSensed = sensed;      // (a sensed cycle: mhb_resolve takes the counts from the records on the device)
  f->mhbPending = true;
  f->mhbHave = true;
  batch_cycle_done(f, n_z, false, true, t0);     // (`cur` was flipped behind the prune)
  return RFSGPU_OK;
}
// The last cycle of every filter (synchronising).  Per-filter arrays [n_filters]; parent and plan [n_filters * max_per_filter] in slots
// local to the filter: identity where nothing happened, -1 beyond the counts.
int rfsgpu_batch_fastslam_last_cycle(rfsgpu_filter *f, int *n_after_update, int *n_after_resample, unsigned char *fired, double *n_eff, unsigned char *overflowed,
                                     int *parent, int *plan) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_last_cycle: not a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh)");
  if (!f->mhbHave) return fail(f, RFSGPU_ERR_INVALID, "batch_fastslam_last_cycle: no rfsgpu_batch_fastslam_mh_cycle_async has run on this handle");
  const int stride = f->nPer;
  for (int b = 0; b < f->nF; b++) {
    FsCycleState H;
    mhb_view(f, f->hMhbBlock, b, H);
    const bool ovf = H.w[FSC_OVF] != 0, idle = ovf || f->mhbLastNZ[b] == 0;     // (nothing happened to this filter in the last cycle)
    const int n = H.w[FSC_N], ng = idle ? n : H.w[FSC_NGROWN];
    if (n_after_update) n_after_update[b] = ng;
    if (n_after_resample) n_after_resample[b] = n;
    if (fired) fired[b] = (!idle && H.w[FSC_FIRED]) ? 1 : 0;
    if (n_eff) n_eff[b] = idle ? 0.0 : H.nEff[0];
    if (overflowed) overflowed[b] = ovf ? 1 : 0;
    for (int k = 0; k < stride; k++) {
      if (parent) parent[(size_t)b * stride + k] = k < ng ? (idle ? k : H.slotSrc[k]) : -1;
      if (plan) plan[(size_t)b * stride + k] = k < n ? (idle ? k : H.plan[k]) : -1;
    }
  }
  return RFSGPU_OK;
}
int rfsgpu_batch_live_counts(rfsgpu_filter *f, int *out) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_live_counts: not a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh)");
  if (!out) return fail(f, RFSGPU_ERR_INVALID, "batch_live_counts: null output");
  for (int b = 0; b < f->nF; b++) {
    FsCycleState H;
    mhb_view(f, f->hMhbBlock, b, H);
    out[b] = H.w[FSC_N];
  }
  return RFSGPU_OK;
}
// {sum w, sum w^2} of every filter's current weights, [n_filters][2] (synchronising).
int rfsgpu_batch_weight_sums(rfsgpu_filter *f, double *out) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_weight_sums", ON_MH_BATCH);
  if (!out) return fail(f, RFSGPU_ERR_INVALID, "batch_weight_sums: null output");
  hipSetDevice(f->device);
  batch_weight_sums_kernel<<<f->nF, 256, 0, f->stream>>>(f->B.weight, f->nPer, f->dBSums);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, f->dBSums, (size_t)f->nF * 2 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}
// Resampling of the filters whose flag is set: slot k takes slot src_slot[k] (global slots, a source in k's own block that keeps
// itself); their weights become 1 and their resampleOccured_ is set.  The other filters' entries of src_slot are not read.
int rfsgpu_batch_resample_apply(rfsgpu_filter *f, const int *src_slot, const unsigned char *resampled) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_resample_apply", ON_MH_BATCH);
  if (!src_slot || !resampled) return fail(f, RFSGPU_ERR_INVALID, "batch_resample_apply: null argument");
  if (f->bDevRoute)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_resample_apply: this batch resamples on the device (rfsgpu_batch_resample_async or rfsgpu_batch_vp_resample_async has run): the particle ids, resampleOccured_ "
                                           "and the resampling counters live there, and the two routes do not mix on one handle");
  const int nF = f->nF, nPer = f->nPer;
  bool any = false;
  for (int b = 0; b < nF; b++) {
    if (!resampled[b]) continue;
    any = true;
    const int lo = b * nPer, hi = lo + nPer;
    for (int k = lo; k < hi; k++) {
      const int s = src_slot[k];
      if (s < lo || s >= hi) {
        f->err = "batch_resample_apply: filter " + std::to_string(b) + ": source slot " + std::to_string(s) + " of slot " + std::to_string(k) + " lies outside the filter's block";
        return RFSGPU_ERR_INVALID;
      }
      if (src_slot[s] != s) {
        f->err = "batch_resample_apply: filter " + std::to_string(b) + ": a source slot must keep itself";
        return RFSGPU_ERR_INVALID;
      }
    }
  }
  if (!any) return RFSGPU_OK;
  ensure_ids(f);
  hipSetDevice(f->device);
  long long t0 = now_ns();
  double *hs;
  int ks;
  if ((rc = ring_acquire(f, f->stage, &hs, &ks)) != RFSGPU_OK) return rc;
  int *hsrc = reinterpret_cast<int *>(hs);
  int *hflag = hsrc + f->N;
  for (int b = 0; b < nF; b++) {
    hflag[b] = resampled[b] ? 1 : 0;
    const int lo = b * nPer, hi = lo + nPer;
    for (int k = lo; k < hi; k++) {
      const int s = resampled[b] ? src_slot[k] : k;
      hsrc[k] = s;
      if (!resampled[b]) continue;
      if (s != k) { f->pid[k] = f->pid[s]; f->ppid[k] = f->pid[s]; }
      else f->ppid[k] = f->pid[k];
    }
    if (resampled[b]) f->bResampled[b] = 1;
  }
  resample_gather_kernel<<<f->N, 256, 0, f->stream>>>(f->B, f->cur, hsrc, f->P.poseCovStride, batch_map_only(f));
  batch_reset_weights_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.weight, f->N, nPer, hflag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->stage.ev[ks], f->stream));
  const long long dtn = now_ns() - t0;
  f->timing.particleResample_wall += dtn;
  f->timing.particleResample_cpu += dtn;
  return RFSGPU_OK;
}
// [test] 1 once a step of this handle has queued Murty-200 partitions (the post kernel's pinned flag, see murty_launch)
int rfsgpu_murty_seen(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  return *f->hJobCount ? 1 : 0;
}
// resampleOccured_ of every filter, [n_filters]
int rfsgpu_batch_resample_occured(const rfsgpu_filter *f, unsigned char *out) {
  if (!f || !f->batch || !out) return RFSGPU_ERR_INVALID;
  if (f->mhbPending) {     // (a batch of multi-hypothesis filters with cycles in flight: the flags are the device's; synchronising)
    const int rc = mhb_resolve(const_cast<rfsgpu_filter *>(f));
    if (rc != RFSGPU_OK) return rc;
  }
  if (f->bDevRoute) {      // (a batch that resamples on the device: the flags live there; synchronising)
    std::vector<int> r(f->nF);
    hipSetDevice(f->device);
    if (hipMemcpyAsync(r.data(), f->BL.resampled, (size_t)f->nF * sizeof(int), hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess) return RFSGPU_ERR_HIP;
    for (int b = 0; b < f->nF; b++) out[b] = r[b] ? 1 : 0;
    return RFSGPU_OK;
  }
  for (int b = 0; b < f->nF; b++) out[b] = f->bResampled[b] ? 1 : 0;
  return RFSGPU_OK;
}

// ---- the device loop of a batch (batch_loop.h): propagation and resampling as stream-ordered launches -------------------------------
int rfsgpu_batch_set_motion_odometry(rfsgpu_filter *f, int filter, const double *var, unsigned long long seed) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, filter);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_set_motion_odometry", ON_VP_BATCH);
  if (!var || !(var[0] >= 0.0) || !(var[1] >= 0.0) || !(var[2] >= 0.0)) return fail(f, RFSGPU_ERR_INVALID, "batch_set_motion_odometry: var is three variances >= 0");
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) {
    BatchMotion &M = f->bMotion[b];
    for (int q = 0; q < 3; q++) { M.var[q] = var[q]; M.sd[q] = sqrt(var[q]); }
    M.seed = seed;
    f->bMotionSet[b] = 1;
  }
  f->bMotionDirty = true;
  return RFSGPU_OK;
}
int rfsgpu_batch_set_resampling(rfsgpu_filter *f, int filter, double eff_n, double eff_n_percent) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, filter);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f) && !batch_is_mh(f)) return refuse_on_kind(f, "rfsgpu_batch_set_resampling", ON_VP_BATCH);     // (the thresholds of the resampling inside its cycle, as on a 2-D multi-hypothesis batch)
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) {
    f->bEffN[2 * (size_t)b] = eff_n; f->bEffN[2 * (size_t)b + 1] = eff_n_percent;
    f->bResSet[b] = 1;
  }
  return RFSGPU_OK;
}
// The filters' motion parameters, when they have changed: through a slot of the pinned ring, like the per-call tables (nothing waits)
static int batch_push_motion(rfsgpu_filter *f) {
  if (!f->bMotionDirty) return RFSGPU_OK;
  unsigned char *h = nullptr;
  int k = 0;
  int rc = ring_acquire(f, f->bLoop, &h, &k);
  if (rc != RFSGPU_OK) return rc;
  memcpy(h, f->bMotion.data(), (size_t)f->nF * sizeof(BatchMotion));
  HIPCHK(hipMemcpyAsync(f->dBMotion, h, (size_t)f->nF * sizeof(BatchMotion), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipEventRecord(f->bLoop.ev[k], f->stream));
  if (f->D == 3) {     // a batch of Victoria Park filters: the Ackerman table beside it (rfsgpu_batch_vp_set_motion), a block of its own
    if ((rc = ring_acquire(f, f->bLoop, &h, &k)) != RFSGPU_OK) return rc;
    memcpy(h, f->bVpMotion.data(), (size_t)f->nF * sizeof(VpBatchMotion));
    HIPCHK(hipMemcpyAsync(f->dBVpMotion, h, (size_t)f->nF * sizeof(VpBatchMotion), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipEventRecord(f->bLoop.ev[k], f->stream));
  }
  f->bMotionDirty = false;
  return RFSGPU_OK;
}
int rfsgpu_batch_propagate_async(rfsgpu_filter *f, const double *u, const double *pin_pose, const unsigned char *pin, unsigned long long call) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_propagate_async", ON_VP_BATCH);
  if (!u) return fail(f, RFSGPU_ERR_INVALID, "batch_propagate: null odometry input");
  const int nF = f->nF;
  for (int b = 0; b < nF; b++) {
    if (pin && pin[b] && !pin_pose) return fail(f, RFSGPU_ERR_INVALID, "batch_propagate: a pinned filter without pin_pose");
    if (!f->bMotionSet[b]) {
      f->err = "batch_propagate: filter " + std::to_string(b) + " has no motion parameters (rfsgpu_batch_set_motion_odometry)";
      return RFSGPU_ERR_INVALID;
    }
  }
  return batch_propagate_core(f, u, pin_pose, pin, nullptr, call);
}
// The propagation behind rfsgpu_batch_propagate_async (devRow null: the host's row goes through a block of the loop ring) and
// rfsgpu_batch_run_truth_async (devRow: the call's row of the truth tables on the device).  The arguments have been checked.
static int batch_propagate_core(rfsgpu_filter *f, const double *u, const double *pin_pose, const unsigned char *pin, const BatchPropIn *devRow, unsigned long long call) {
  int rc = RFSGPU_OK;
  const int nF = f->nF;
  hipSetDevice(f->device);
  if ((rc = batch_push_motion(f)) != RFSGPU_OK) return rc;
  if (!devRow) {
    unsigned char *h = nullptr;
    int k = 0;
    if ((rc = ring_acquire(f, f->bLoop, &h, &k)) != RFSGPU_OK) return rc;
    BatchPropIn *hi = reinterpret_cast<BatchPropIn *>(h);
    for (int b = 0; b < nF; b++) {
      BatchPropIn &I = hi[b];
      memset(&I, 0, sizeof I);
      memcpy(I.u, u + 3 * (size_t)b, 3 * sizeof(double));
      I.pin = (pin && pin[b]) ? 1 : 0;
      if (I.pin) memcpy(I.pinPose, pin_pose + 3 * (size_t)b, 3 * sizeof(double));
    }
    HIPCHK(hipMemcpyAsync(f->dBPropIn, hi, (size_t)nF * sizeof(BatchPropIn), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipEventRecord(f->bLoop.ev[k], f->stream));
  }
  // every particle gets its own pose covariance (handle-wide stride, as rfsgpu_batch_cycle_async sets it with x_cov [N][9])
  if (f->P.poseCovStride != 9) { f->P.poseCovStride = 9; f->bParamsDirty = true; }
  f->poseCovZero = false;
  // the new poses go to the second pose buffer and the two change places: the next cycle's births read the old ones there.  A
  // second propagation before that cycle works in place, so that the births still see the poses the last update used.
  double *dst = f->bBirthAlt ? f->B.pose : f->poseAlt;
  batch_propagate_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.pose, dst, f->B.poseCov, f->dBMotion, devRow ? devRow : f->dBPropIn, f->N, f->nPer,
                                                                     (unsigned)(call & 0xffffffffull), (unsigned)(call >> 32));
  HIPCHK(hipGetLastError());
  if (!f->bBirthAlt) { f->poseAlt = f->B.pose; f->B.pose = dst; f->bBirthAlt = true; }
  return RFSGPU_OK;
}
int rfsgpu_batch_resample_async(rfsgpu_filter *f, const int *n_z, unsigned long long call) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_resample_async", ON_VP_BATCH);
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_resample_async", ON_MH_BATCH);
  if ((rc = batch_check_call(f, BATCH_RESAMPLE, 0, nullptr, 0, n_z)) != RFSGPU_OK) return rc;
  if (f->bSensed)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_resample: this batch has run a sensed cycle (rfsgpu_batch_cycle_sensed_async or rfsgpu_batch_fastslam_cycle_sensed_async): its measurement counts live on the device (rfsgpu_batch_resample_sensed_async)");
  return batch_resample_core(f, BATCH_RESAMPLE, n_z, call);
}
// From here on the ids and resampleOccured_ live on the device.  Once per handle, and host-synchronous: the sources are pageable host
// vectors, which the runtime copies before the call returns; the synchronisation says so instead of relying on it.
static int batch_enter_dev_route(rfsgpu_filter *f) {
  if (f->bDevRoute) return RFSGPU_OK;
  const int nF = f->nF;
  ensure_ids(f);
  std::vector<int> r(nF);
  for (int b = 0; b < nF; b++) r[b] = f->bResampled[b] ? 1 : 0;
  HIPCHK(hipMemcpyAsync(f->BL.pid, f->pid.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->BL.ppid, f->ppid.data(), (size_t)f->N * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipMemcpyAsync(f->BL.resampled, r.data(), (size_t)nF * sizeof(int), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  f->bDevRoute = true;
  return RFSGPU_OK;
}
// The resampling tail behind rfsgpu_batch_resample_async (n_z: the host's counts) and rfsgpu_batch_resample_sensed_async (n_z null:
// each filter's count is the nZ of its record on the device).  stageIn false (the later steps of rfsgpu_batch_run_truth_async, n_z null):
// the per-filter table on the device is still the one the run's first step staged -- thresholds and gates cannot change inside the call
static int batch_resample_core(rfsgpu_filter *f, const BatchCall &C, const int *n_z, unsigned long long call, bool stageIn) {
  int rc = RFSGPU_OK;
  const int nF = f->nF;
  if (f->nPer > RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER) {
    f->err = std::string(C.who) + ": more than RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER particles per filter (one workgroup resamples a filter)";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  for (int b = 0; b < nF; b++) {
    if (n_z && (rc = batch_check_filter(f, C, b, nullptr, n_z)) != RFSGPU_OK) return rc;
    if ((!f->bMotionSet[b] || !f->bResSet[b]) && f->D == 3)
      return batch_fail(f, C, "filter " + std::to_string(b) + (f->bResSet[b] ? " has no Philox key (rfsgpu_batch_vp_set_motion)" : " has no resampling thresholds (rfsgpu_batch_vp_set_resampling)"));
    if (!f->bMotionSet[b] || !f->bResSet[b])
      return batch_fail(f, C, "filter " + std::to_string(b) + (f->bResSet[b] ? " has no Philox key (rfsgpu_batch_set_motion_odometry)" : " has no resampling thresholds (rfsgpu_batch_set_resampling)"));
  }
  hipSetDevice(f->device);
  long long t0 = now_ns();
  if ((rc = batch_enter_dev_route(f)) != RFSGPU_OK) return rc;
  if ((rc = batch_push_motion(f)) != RFSGPU_OK) return rc;
  if (stageIn) {
    unsigned char *h = nullptr;
    int k = 0;
    if ((rc = ring_acquire(f, f->bLoop, &h, &k)) != RFSGPU_OK) return rc;
    BatchResIn *hi = reinterpret_cast<BatchResIn *>(h);
    for (int b = 0; b < nF; b++) {
      BatchResIn &I = hi[b];
      I.effN = f->bEffN[2 * (size_t)b]; I.effNPercent = f->bEffN[2 * (size_t)b + 1];
      I.nZ = n_z ? n_z[b] : 0;
      if (f->bSteps == STEPS_FASTSLAM) { I.minUpdates = (int)f->bFs[b].minUpdatesBeforeResample; I.minMeasurements = (int)f->bFs[b].minMeasurementsBeforeResample; }   // (a FastSLAM batch: FastSLAM.hpp:729-733)
      else { I.minUpdates = f->bCfg[b].minUpdatesBeforeResample; I.minMeasurements = f->bCfg[b].minMeasurementsBeforeResample; }
      I.pad = 0;
    }
    HIPCHK(hipMemcpyAsync(f->dBResIn, hi, (size_t)nF * sizeof(BatchResIn), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipEventRecord(f->bLoop.ev[k], f->stream));
  }
  batch_resample_kernel<<<nF, BATCH_LOOP_THREADS, 0, f->stream>>>(f->B.weight, f->BL, f->dBMotion, f->dBResIn, f->nPer, call, n_z ? nullptr : f->dBFilt);
  resample_gather_kernel<<<f->N, 256, 0, f->stream>>>(f->B, f->cur, f->BL.plan, f->P.poseCovStride, batch_map_only(f));
  HIPCHK(hipGetLastError());
  const long long dtn = now_ns() - t0;
  f->timing.particleResample_wall += dtn;
  f->timing.particleResample_cpu += dtn;
  return RFSGPU_OK;
}
int rfsgpu_batch_last_resample(rfsgpu_filter *f, unsigned char *fired, int *src_slot, double *n_eff) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_last_resample", ON_VP_BATCH);
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_last_resample", ON_MH_BATCH);
  return batch_last_resample_core(f, fired, src_slot, n_eff);
}
// (the arguments have been checked: rfsgpu_batch_last_resample, rfsgpu_batch_vp_last_resample)
static int batch_last_resample_core(rfsgpu_filter *f, unsigned char *fired, int *src_slot, double *n_eff) {
  hipSetDevice(f->device);
  if (!f->bDevRoute) {     // no rfsgpu_batch_resample_async yet: nothing fired
    for (int b = 0; b < f->nF; b++) { if (fired) fired[b] = 0; if (n_eff) n_eff[b] = 0.0; }
    if (src_slot) for (int q = 0; q < f->N; q++) src_slot[q] = q;
    return RFSGPU_OK;
  }
  std::vector<int> fi(f->nF);
  HIPCHK(hipMemcpyAsync(fi.data(), f->BL.fired, (size_t)f->nF * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  if (src_slot) HIPCHK(hipMemcpyAsync(src_slot, f->BL.plan, (size_t)f->N * sizeof(int), hipMemcpyDeviceToHost, f->stream));
  if (n_eff) HIPCHK(hipMemcpyAsync(n_eff, f->BL.nEff, (size_t)f->nF * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  if (fired) for (int b = 0; b < f->nF; b++) fired[b] = fi[b] ? 1 : 0;
  return RFSGPU_OK;
}
int rfsgpu_batch_get_pose_covs(rfsgpu_filter *f, double *out) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!out) return fail(f, RFSGPU_ERR_INVALID, "batch_get_pose_covs: null output");
  hipSetDevice(f->device);
  const bool each = f->P.poseCovStride == 9;
  HIPCHK(hipMemcpyAsync(out, f->B.poseCov, (each ? (size_t)f->N : 1) * 9 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  if (!each) for (int k = 1; k < f->N; k++) memcpy(out + 9 * (size_t)k, out, 9 * sizeof(double));   // (one covariance shared by all slots)
  return RFSGPU_OK;
}
int rfsgpu_batch_resample_counts(rfsgpu_filter *f, long long *out) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_vp(f)) return refuse_on_kind(f, "rfsgpu_batch_resample_counts", ON_VP_BATCH);
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_resample_counts", ON_MH_BATCH);
  if (!out) return fail(f, RFSGPU_ERR_INVALID, "batch_resample_counts: null output");
  hipSetDevice(f->device);
  HIPCHK(hipMemcpyAsync(out, f->BL.nResamples, (size_t)f->nF * sizeof(long long), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}

// ---- the device route of a batch of Victoria Park filters (vp_batch_loop.h): Ackerman propagation of a run of odometry messages and
// the resampling tail as stream-ordered launches; the birth predict's inheritance walk behind them is batch_vp_cycle_core's ----------
static const BatchCall BATCH_VP_RESAMPLE{"batch_vp_resample", 0, nullptr, "null measurement counts"};
static_assert(RFSGPU_BATCH_VP_RUN_MAX == ACKERMAN_RUN_MAX, "a run of a batch is what a handle's run launch takes (VpBatchRun, motion.h)");
// What the section serves, else RFSGPU_ERR_UNSUPPORTED with the state untouched
// resampling: a call of the resampling tail, which a batch of multi-hypothesis filters runs inside its cycle
static int vp_loop_check(rfsgpu_filter *f, const char *who, int filter, bool resampling = false) {
  if (!f->batch || f->D != 3) {
    f->err = std::string(who) + ": the call serves a batch of Victoria Park filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D), not " +
             (f->batch ? "a 2-D batch (its device loop is rfsgpu_batch_set_motion_odometry, _set_resampling, _propagate_async, _resample_async)"
                       : (f->groupShard ? "a shard of an rfsgpu_group" : "an ordinary handle (rfsgpu_propagate_ackerman_run_async, rfsgpu_rbphd_cycle_async)"));
    return RFSGPU_ERR_UNSUPPORTED;
  }
  if (filter < -1 || filter >= f->nF) { f->err = std::string(who) + ": filter index out of range"; return RFSGPU_ERR_INVALID; }
  if (resampling && batch_is_mh(f)) {
    f->err = std::string(who) + ": not available on " + handle_kind_text(f) + ": its resampling runs inside that cycle (thresholds: rfsgpu_batch_set_resampling; outcome: rfsgpu_batch_fastslam_last_cycle)";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  return RFSGPU_OK;
}
int rfsgpu_batch_vp_set_motion(rfsgpu_filter *f, int filter, const double *var, const double *geom, unsigned long long seed) {
  CHECK_HANDLE(f);
  int rc = vp_loop_check(f, "batch_vp_set_motion", filter);
  if (rc != RFSGPU_OK) return rc;
  if (!var || !(var[0] >= 0.0) || !(var[1] >= 0.0)) return fail(f, RFSGPU_ERR_INVALID, "batch_vp_set_motion: var is two variances >= 0 (speed, steering)");
  if (!geom || !(geom[0] == geom[0]) || !(geom[1] == geom[1]) || !(geom[2] == geom[2]) || !(geom[3] == geom[3]) || geom[1] == 0.0)
    return fail(f, RFSGPU_ERR_INVALID, "batch_vp_set_motion: geom is {h, l, dx, dy} with l != 0");
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) {
    VpBatchMotion &M = f->bVpMotion[b];
    M.sv = std::sqrt(var[0]); M.sr = std::sqrt(var[1]);
    M.h = geom[0]; M.l = geom[1]; M.dx = geom[2]; M.dy = geom[3];
    M.seed = seed;
    f->bMotion[b].seed = seed;     // (batch_resample_kernel takes the resampling draw's key from this table)
    f->bMotionSet[b] = 1;
  }
  f->bMotionDirty = true;
  return RFSGPU_OK;
}
int rfsgpu_batch_vp_set_resampling(rfsgpu_filter *f, int filter, double eff_n, double eff_n_percent) {
  CHECK_HANDLE(f);
  int rc = vp_loop_check(f, "batch_vp_set_resampling", filter, true);
  if (rc != RFSGPU_OK) return rc;
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) {
    f->bEffN[2 * (size_t)b] = eff_n; f->bEffN[2 * (size_t)b + 1] = eff_n_percent;
    f->bResSet[b] = 1;
  }
  return RFSGPU_OK;
}
int rfsgpu_batch_vp_propagate_run_async(rfsgpu_filter *f, int n, const double *u, const unsigned char *noisy, const double *dt, unsigned long long call0) {
  if (!f) return RFSGPU_ERR_INVALID;
  if (!batch_is_vp_mh(f)) { CHECK_HANDLE(f); }     // (a batch of multi-hypothesis filters: behind its cycles, nothing is read back)
  int rc = vp_loop_check(f, "batch_vp_propagate_run", -1);
  if (rc != RFSGPU_OK) return rc;
  if (n < 0 || (n > 0 && (!u || !dt))) return fail(f, RFSGPU_ERR_INVALID, "batch_vp_propagate_run: bad arguments");
  if (n > RFSGPU_BATCH_VP_RUN_MAX)
    return fail(f, RFSGPU_ERR_INVALID, "batch_vp_propagate_run: more than RFSGPU_BATCH_VP_RUN_MAX steps in one call (the run travels through one block of the pinned ring): split it");
  for (int k = 0; k < n; k++)
    if (!(dt[k] == dt[k])) return fail(f, RFSGPU_ERR_INVALID, "batch_vp_propagate_run: bad interval");
  for (int b = 0; b < f->nF; b++)
    if (!f->bMotionSet[b]) {
      f->err = "batch_vp_propagate_run: filter " + std::to_string(b) + " has no motion parameters (rfsgpu_batch_vp_set_motion)";
      return RFSGPU_ERR_INVALID;
    }
  if (n == 0) return RFSGPU_OK;
  hipSetDevice(f->device);
  if ((rc = batch_push_motion(f)) != RFSGPU_OK) return rc;
  unsigned char *h = nullptr;
  int k = 0;
  if ((rc = ring_acquire(f, f->bLoop, &h, &k)) != RFSGPU_OK) return rc;
  VpBatchRun *R = reinterpret_cast<VpBatchRun *>(h);
  memset(R, 0, sizeof *R);
  R->n = n;
  R->call0 = call0;
  for (int r = 0; r < n; r++) {
    R->uv[r] = u[2 * r]; R->ur[r] = u[2 * r + 1]; R->dt[r] = dt[r];
    R->noisy[r] = (!noisy || noisy[r]) ? 1 : 0;
  }
  HIPCHK(hipMemcpyAsync(f->dBVpRun, R, sizeof *R, hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipEventRecord(f->bLoop.ev[k], f->stream));
  // in place: the caller orders the call behind the birth predict, which must still see the poses of the last update
  if (batch_is_mh(f)) {     // (a filter whose overflow word is up stays where its abandoned cycle found it)
    FsCycleState S0;
    mhb_state(f->mhbBlock, f->nF, f->nPer, 0, S0);
    vp_batch_propagate_run_guard_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.pose, f->N, f->nPer, f->dBVpMotion, f->dBVpRun, S0.w, FSC_WORDS, FSC_OVF);
  } else vp_batch_propagate_run_kernel<<<(f->N + 255) / 256, 256, 0, f->stream>>>(f->B.pose, f->N, f->nPer, f->dBVpMotion, f->dBVpRun);
  HIPCHK(hipGetLastError());
  return RFSGPU_OK;
}
int rfsgpu_batch_vp_resample_async(rfsgpu_filter *f, const int *n_z, unsigned long long call) {
  CHECK_HANDLE(f);
  int rc = vp_loop_check(f, "batch_vp_resample", -1, true);
  if (rc != RFSGPU_OK) return rc;
  if ((rc = batch_check_call(f, BATCH_VP_RESAMPLE, 0, nullptr, 0, n_z)) != RFSGPU_OK) return rc;
  return batch_resample_core(f, BATCH_VP_RESAMPLE, n_z, call);
}
int rfsgpu_batch_vp_last_resample(rfsgpu_filter *f, unsigned char *fired, int *src_slot, double *n_eff) {
  CHECK_HANDLE(f);
  int rc = vp_loop_check(f, "batch_vp_last_resample", -1, true);
  if (rc != RFSGPU_OK) return rc;
  return batch_last_resample_core(f, fired, src_slot, n_eff);
}
int rfsgpu_batch_vp_loop_counts(rfsgpu_filter *f, long long *resamplings, int *max_level) {
  CHECK_HANDLE(f);
  int rc = vp_loop_check(f, "batch_vp_loop_counts", -1, true);
  if (rc != RFSGPU_OK) return rc;
  hipSetDevice(f->device);
  int w[2] = {0, 0};
  if (resamplings) HIPCHK(hipMemcpyAsync(resamplings, f->BL.nResamples, (size_t)f->nF * sizeof(long long), hipMemcpyDeviceToHost, f->stream));
  if (max_level) HIPCHK(hipMemcpyAsync(w, f->dBVpWalk, sizeof w, hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  if (max_level) *max_level = std::max(w[VBW_MAXEVER], w[VBW_LAST]);
  return RFSGPU_OK;
}

// ---- [sensor] every filter's scan drawn on the device (batch_sensor.h) ----------------------------------------------------------------
static const BatchCall BATCH_SET_SENSOR{"batch_set_sensor", 0, nullptr, nullptr};
static const BatchCall BATCH_SENSE{"batch_sense", 0, nullptr, nullptr};
static const BatchCall BATCH_CYCLE_SENSED{"batch_cycle_sensed", -1, "RFSGPU_CYCLE_NO_PREDICT (-1), 0 (static step only) or 1 (births + static step)", nullptr};
static const BatchCall BATCH_RESAMPLE_SENSED{"batch_resample_sensed", 0, nullptr, nullptr};
static const BatchCall BATCH_LAST_SCAN{"batch_last_scan", 0, nullptr, nullptr};
// What the section serves: RB-PHD filter batches, and -- once rfsgpu_batch_fastslam_serve_sensor has switched it on -- batches of
// FastSLAM and of multi-hypothesis FastSLAM filters.  Their records carry three count-dependent fields (pfa, prune, the multi-hypothesis
// draw), which the sensed cycle of their kind derives on the device (fastslam_sensed.h); the switch is off at creation, so the refusals
// the section was published with stand until a caller asks.
static int sensor_check(rfsgpu_filter *f, const BatchCall &C) {
  if (batch_is_vp(f)) {
    f->err = std::string(C.who) + ": the device sensor is a 2-D range-bearing sensor: it does not serve a batch of Victoria Park filters";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  // (a batch that has not decided serves as the RB-PHD batch its first sensed cycle makes it)
  if (f->batch && (f->bServeSensor || !batch_log_odds(f))) return RFSGPU_OK;
  f->err = std::string(C.who) + ": the device sensor serves batches of RB-PHD filters (rfsgpu_create_batch, rfsgpu_batch_cycle_async) only, not " + handle_kind_text(f);
  if (f->batch) f->err += " (rfsgpu_batch_fastslam_serve_sensor switches the section on for it)";
  return RFSGPU_ERR_UNSUPPORTED;
}
// The switch of a FastSLAM or multi-hypothesis batch: off at creation (rfsgpu_batch_mh_serve_metrics is the precedent).
int rfsgpu_batch_fastslam_serve_sensor(rfsgpu_filter *f, int on) {
  CHECK_HANDLE(f);
  if (batch_is_vp(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_serve_sensor: the device sensor is a 2-D range-bearing sensor: it does not serve a batch of Victoria Park filters");
  if (!f->batch || !batch_log_odds(f))
    return refuse_not(f, "batch_fastslam_serve_sensor: the switch is for batches of FastSLAM or multi-hypothesis FastSLAM filters",
                      f->bSteps == STEPS_RBPHD ? ": the [sensor] calls serve it as it is" : "");
  if (!on && f->bSensed)
    return fail(f, RFSGPU_ERR_INVALID, "batch_fastslam_serve_sensor: a sensed cycle has run on this handle: its measurement counts live on the device, the host-fed calls could not take over");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  if (on && !f->dFsTmpl)
    HIPCHK(hipMalloc(&f->dFsTmpl, (size_t)f->nF * std::max(sizeof(FsSensedTemplate<FsBatchFilter>), sizeof(FsSensedTemplate<MhBatchFilter>))));
  if (on && batch_is_mh(f) && !f->dFsLastNZ) HIPCHK(hipMalloc(&f->dFsLastNZ, (size_t)f->nF * sizeof(int)));
  if (on && batch_is_mh(f) && !f->hFsLastNZ) HIPCHK(hipHostMalloc(&f->hFsLastNZ, (size_t)f->nF * sizeof(int)));
  f->bServeSensor = on != 0;
  if (!on) f->bSenseFresh = false;
  return RFSGPU_OK;
}
int rfsgpu_batch_set_sensor(rfsgpu_filter *f, int filter, const rfsgpu_rngbrg_config *model, const double *landmarks_xy, int n_landmarks, int max_nz,
                            unsigned long long seed) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_SET_SENSOR;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (filter < -1 || filter >= f->nF) return batch_fail(f, C, "filter index out of range");
  if (!model) return batch_fail(f, C, "null sensor model");
  if (n_landmarks < 0 || n_landmarks > RFSGPU_SENSOR_MAX_LANDMARKS) return batch_fail(f, C, "n_landmarks must lie in 0 ... RFSGPU_SENSOR_MAX_LANDMARKS");
  if (n_landmarks > 0 && !landmarks_xy) return batch_fail(f, C, "null landmark array");
  if (max_nz < 1 || max_nz > RFSGPU_MAX_Z) return batch_fail(f, C, "max_nz must lie in 1 ... RFSGPU_MAX_Z");
  for (int q = 0; q < 2 * n_landmarks; q++)
    if (!std::isfinite(landmarks_xy[q])) return batch_fail(f, C, "landmark " + std::to_string(q / 2) + " is not finite");
  BatchSensor S;
  memset(&S, 0, sizeof S);
  // the lower Cholesky factor of R (Eigen's LLT reads the lower triangle; RandomVec::sample multiplies it with the deviates)
  const double *R = model->R;
  S.L[0] = sqrt(R[0]);
  S.L[1] = R[2] / S.L[0];
  S.L[2] = sqrt(R[3] - S.L[1] * S.L[1]);
  if (!(R[0] > 0.0) || R[1] != R[2] || !(R[3] - S.L[1] * S.L[1] > 0.0) || !std::isfinite(S.L[0]) || !std::isfinite(S.L[1]) || !std::isfinite(S.L[2]))
    return batch_fail(f, C, "R is not (symmetric) positive definite");
  if (!std::isfinite(model->rangeLimMin) || !std::isfinite(model->rangeLimMax) || !(model->rangeLimMin < model->rangeLimMax))
    return batch_fail(f, C, "rangeLimMin must lie below rangeLimMax");
  if (!(model->probabilityOfDetection >= 0.0 && model->probabilityOfDetection <= 1.0)) return batch_fail(f, C, "probabilityOfDetection must lie in [0, 1]");
  if (!(model->uniformClutterIntensity >= 0.0)) return batch_fail(f, C, "uniformClutterIntensity must not be negative");
  S.Pd = model->probabilityOfDetection; S.rmin = model->rangeLimMin; S.rmax = model->rangeLimMax;
  S.seed = seed; S.nLm = n_landmarks; S.maxNz = max_nz;
  {   // the Poisson table of src/rbphdslam2dSim.cpp:292-306: same loop, same order of operations
    const double PI = acos(-1);
    const double sensingArea = 2 * PI * (model->rangeLimMax - model->rangeLimMin);     // MeasurementModel_RngBrg::clutterIntensityIntegral
    const double meanClutter = model->uniformClutterIntensity * sensingArea;
    const double expNegMeanClutter = exp(-meanClutter);
    double poissonPmf[SENSOR_CMF];
    double mean_pow_i = 1;
    double i_factorial = 1;
    poissonPmf[0] = expNegMeanClutter;
    S.cmf[0] = poissonPmf[0];
    for (int i = 1; i < SENSOR_CMF; i++) {
      mean_pow_i *= meanClutter;
      i_factorial *= i;
      poissonPmf[i] = mean_pow_i / i_factorial * expNegMeanClutter;
      S.cmf[i] = S.cmf[i - 1] + poissonPmf[i];
    }
    for (int i = 0; i < SENSOR_CMF; i++)
      if (!std::isfinite(S.cmf[i])) return batch_fail(f, C, "the mean clutter count is beyond what the 100-entry Poisson table can hold (a term of it is not finite)");
  }
  // configuration is rare: the tables are written in place once the stream has drained (a sense kernel in flight reads them)
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) {
    HIPCHK(hipMemcpy(f->dBSensor + b, &S, sizeof S, hipMemcpyHostToDevice));
    if (n_landmarks > 0)
      HIPCHK(hipMemcpy(f->dBSensorLm + (size_t)b * SENSOR_MAX_LANDMARKS * 2, landmarks_xy, (size_t)n_landmarks * 2 * sizeof(double), hipMemcpyHostToDevice));
    f->bSensorSet[b] = 1;
    f->bSensorMaxNz[b] = max_nz;
  }
  f->bSenseFresh = false;     // (a scan drawn before this call is not this sensor's: the next sensed cycle needs a sense call of its own)
  return RFSGPU_OK;
}
int rfsgpu_batch_sense_async(rfsgpu_filter *f, const double *gt_pose, unsigned long long call) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_SENSE;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (!gt_pose) return batch_fail(f, C, "null ground-truth poses");
  const int nF = f->nF;
  for (int b = 0; b < nF; b++) {
    if (!f->bSensorSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no sensor (rfsgpu_batch_set_sensor)");
    const double *p = gt_pose + 3 * (size_t)b;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !(fabs(p[2]) <= 64.0))
      return batch_fail(f, C, "filter " + std::to_string(b) + ": the pose must be finite, its heading within +-64 rad");
  }
  return batch_sense_core(f, gt_pose, nullptr, call);
}
// The scan behind rfsgpu_batch_sense_async (devPose null: the host's poses go through a block of the loop ring) and
// rfsgpu_batch_run_truth_async (devPose: the call's row of the truth tables on the device; the generator's headings come out of atan2).
// The arguments have been checked.
static int batch_sense_core(rfsgpu_filter *f, const double *gt_pose, const double *devPose, unsigned long long call) {
  int rc = RFSGPU_OK;
  const int nF = f->nF;
  hipSetDevice(f->device);
  unsigned char *h = nullptr;
  int k = 0;
  // One block of the loop ring per call: {poses [nF][3] | counts [nF] | evalCap, useW [nF][2]} (36 bytes a filter, inside the block's
  // size).  The block is acquired before the host's tables change, so that a failure leaves them as they were.  (A call with its
  // poses on the device takes a block only when it has one of the other two tables to send.)
  static_assert(sizeof(BatchPropIn) >= 3 * sizeof(double) + 3 * sizeof(int), "a block of the loop ring holds a sense call's tables");
  bool needBlock = !devPose || !f->bSensed;
  for (int b = 0; b < nF && !needBlock; b++)
    needBlock = batch_eval_cap(f, b) != f->bSensorCaps[2 * (size_t)b] || (f->bCfg[b].useClusterProcess ? 0 : 1) != f->bSensorCaps[2 * (size_t)b + 1];
  if (needBlock && (rc = ring_acquire(f, f->bLoop, &h, &k)) != RFSGPU_OK) return rc;
  if (!devPose) {
    memcpy(h, gt_pose, (size_t)nF * 3 * sizeof(double));
    HIPCHK(hipMemcpyAsync(f->dBSensorPose, h, (size_t)nF * 3 * sizeof(double), hipMemcpyHostToDevice, f->stream));
  }
  // ... until a sensed cycle has run, the counts of the filters' last updates as the host-fed cycles left them
  if (!f->bSensed) {
    int *hp = reinterpret_cast<int *>(h + (size_t)nF * 3 * sizeof(double));
    memcpy(hp, f->bNZ.data(), (size_t)nF * sizeof(int));
    HIPCHK(hipMemcpyAsync(f->dBSensorPrev, hp, (size_t)nF * sizeof(int), hipMemcpyHostToDevice, f->stream));
  }
  // ... evalCap / useW of the records: a table on the device, staged again when a filter's configuration has changed
  bool capsDirty = false;
  int ecMax = 1, nzMax = 0;
  for (int b = 0; b < nF; b++) {
    const int c[2] = {batch_eval_cap(f, b), f->bCfg[b].useClusterProcess ? 0 : 1};
    if (c[0] != f->bSensorCaps[2 * (size_t)b] || c[1] != f->bSensorCaps[2 * (size_t)b + 1]) { f->bSensorCaps[2 * (size_t)b] = c[0]; f->bSensorCaps[2 * (size_t)b + 1] = c[1]; capsDirty = true; }
    ecMax = std::max(ecMax, c[0]);
    nzMax = std::max(nzMax, f->bSensorMaxNz[b]);
  }
  if (capsDirty) {
    int *hc = reinterpret_cast<int *>(h + (size_t)nF * (3 * sizeof(double) + sizeof(int)));
    memcpy(hc, f->bSensorCaps.data(), (size_t)nF * 2 * sizeof(int));
    HIPCHK(hipMemcpyAsync(f->dBSensorCaps, hc, (size_t)nF * 2 * sizeof(int), hipMemcpyHostToDevice, f->stream));
  }
  if (needBlock) HIPCHK(hipEventRecord(f->bLoop.ev[k], f->stream));
  BatchSensorArg A{f->dBSensor, f->dBSensorLm, devPose ? devPose : f->dBSensorPose, f->dBSensorCaps, f->dBSensorPrev, f->dBZ, f->dBFilt, f->B.err, f->dBSensorErrFilter, nF};
  batch_sense_kernel<<<nF, 64, 0, f->stream>>>(A, (unsigned)(call & 0xffffffffull), (unsigned)(call >> 32));
  HIPCHK(hipGetLastError());
  f->bSenseFresh = true;
  f->bSenseNzMax = nzMax; f->bSenseEcMax = ecMax;
  f->bScanHeld = true;
  f->bSensedTail = false;
  return RFSGPU_OK;
}
int rfsgpu_batch_cycle_sensed_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, int normalize) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_CYCLE_SENSED;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_cycle_sensed: this is the RB-PHD cycle; a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh) takes rfsgpu_batch_fastslam_mh_cycle_sensed_async");
  if (f->bSteps == STEPS_FASTSLAM) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_cycle_sensed: this is the RB-PHD cycle; a batch of FastSLAM filters takes rfsgpu_batch_fastslam_cycle_sensed_async");
  if ((rc = batch_check_call(f, C, predict, x_cov, cov_stride, nullptr)) != RFSGPU_OK) return rc;
  for (int b = 0; b < f->nF; b++) {
    if (!f->bSensorSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no sensor (rfsgpu_batch_set_sensor)");
    if (f->bCfg[b].birthGaussianMeasurementCountThreshold != 1u) {
      f->err = "batch_cycle_sensed: a filter batch takes immediate births only (birthGaussianMeasurementCountThreshold 1)";
      return RFSGPU_ERR_UNSUPPORTED;
    }
  }
  if (!f->bSenseFresh) return batch_fail(f, C, "no rfsgpu_batch_sense_async has run since the last cycle or the last rfsgpu_batch_set_sensor: filter 0 (and every other) has no scan for this one");
  // (the step kernel lays out a filter's LDS by the record's evalCap and picks its evaluation points by the Params table's count: the
  //  record, written at the sense call, must still be the configuration's)
  for (int b = 0; b < f->nF; b++)
    if (batch_eval_cap(f, b) != f->bSensorCaps[2 * (size_t)b] || (f->bCfg[b].useClusterProcess ? 0 : 1) != f->bSensorCaps[2 * (size_t)b + 1])
      return batch_fail(f, C, "filter " + std::to_string(b) + ": importanceWeightingEvalPointCount or useClusterProcess has changed since the last rfsgpu_batch_sense_async, whose record carries them: sense again");
  if (f->nPer > RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER) {
    f->err = "batch_cycle_sensed: more than RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER particles per filter (the device route's inheritance kernel takes a filter per workgroup)";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  hipSetDevice(f->device);
  // the inheritance then reads the records where the sensor wrote them.  (Entering the device route is what the first
  // rfsgpu_batch_resample_async does too: it moves the ids, it refuses nothing, and it stays if the cycle below fails.)
  if ((rc = batch_enter_dev_route(f)) != RFSGPU_OK) return rc;
  if ((rc = batch_cycle_core(f, predict, x, x_cov, cov_stride, nullptr, nullptr, normalize)) != RFSGPU_OK) return rc;
  batch_decide(f, STEPS_RBPHD);
  f->bSensed = true;     // (only now: a cycle that failed leaves the host-fed calls open)
  return RFSGPU_OK;
}
// ---- the sensed cycles of the other two kinds (rfsgpu_batch_fastslam_serve_sensor) ----------------------------------------------------
static const BatchCall BATCH_FS_CYCLE_SENSED{"batch_fastslam_cycle_sensed", -1, "RFSGPU_CYCLE_NO_PREDICT (-1), or 0 / 1 (the static landmark step; FastSLAM has no births)", nullptr};
static const BatchCall BATCH_MH_CYCLE_SENSED{"batch_fastslam_mh_cycle_sensed", 0, "0 or 1 (the static landmark step; FastSLAM has no births)", nullptr};
// What the two calls check alike, after the kind: the call's arguments, every filter's sensor (mh: and its motion key, the key of
// its draw), a sense call since the last cycle.  Nothing has been enqueued or changed when one of them refuses.
static int fs_sensed_check(rfsgpu_filter *f, const BatchCall &C, int predict, const double *x_cov, int cov_stride, bool mh) {
  int rc = batch_check_call(f, C, predict, x_cov, cov_stride, nullptr);
  if (rc != RFSGPU_OK) return rc;
  for (int b = 0; b < f->nF; b++) {
    if (!f->bSensorSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no sensor (rfsgpu_batch_set_sensor)");
    if (mh && !f->bMotionSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no Philox key for its resampling draw (rfsgpu_batch_set_motion_odometry)");
  }
  if (!f->bSenseFresh) return batch_fail(f, C, "no rfsgpu_batch_sense_async has run since the last cycle or the last rfsgpu_batch_set_sensor: filter 0 (and every other) has no scan for this one");
  return RFSGPU_OK;
}
int rfsgpu_batch_fastslam_cycle_sensed_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, int normalize) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_FS_CYCLE_SENSED;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_fastslam_cycle_sensed: a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh) takes rfsgpu_batch_fastslam_mh_cycle_sensed_async");
  if (f->bSteps != STEPS_FASTSLAM)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, f->bSteps == STEPS_RBPHD ? "batch_fastslam_cycle_sensed: this batch steps RB-PHD filters (rfsgpu_batch_cycle_async has run): it takes rfsgpu_batch_cycle_sensed_async"
                                                         : "batch_fastslam_cycle_sensed: not a batch of FastSLAM filters yet (rfsgpu_batch_set_fastslam_config, then rfsgpu_batch_fastslam_serve_sensor)");
  if ((rc = fs_sensed_check(f, C, predict, x_cov, cov_stride, false)) != RFSGPU_OK) return rc;
  hipSetDevice(f->device);
  // (as rfsgpu_batch_cycle_sensed_async: resampleOccured_ falls with an update on the device, where the sensed resampling keeps it)
  if ((rc = batch_enter_dev_route(f)) != RFSGPU_OK) return rc;
  if ((rc = batch_fs_cycle_core(f, predict, x, x_cov, cov_stride, nullptr, nullptr, normalize)) != RFSGPU_OK) return rc;
  f->bSensed = true;     // (only now: a cycle that failed leaves the host-fed calls open)
  return RFSGPU_OK;
}
int rfsgpu_batch_fastslam_mh_cycle_sensed_async(rfsgpu_filter *f, int predict, const double *x, const double *x_cov, int cov_stride, unsigned long long call) {
  if (!f) return RFSGPU_ERR_INVALID;     // (as rfsgpu_batch_fastslam_mh_cycle_async: cycles in flight stay in flight)
  const BatchCall &C = BATCH_MH_CYCLE_SENSED;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_is_mh(f))
    return fail(f, RFSGPU_ERR_UNSUPPORTED, f->bSteps == STEPS_FASTSLAM ? "batch_fastslam_mh_cycle_sensed: not a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh): a batch of FastSLAM filters takes rfsgpu_batch_fastslam_cycle_sensed_async"
                                                         : "batch_fastslam_mh_cycle_sensed: not a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh): an RB-PHD batch takes rfsgpu_batch_cycle_sensed_async");
  if ((rc = fs_sensed_check(f, C, predict, x_cov, cov_stride, true)) != RFSGPU_OK) return rc;
  if ((rc = batch_mh_cycle_core(f, predict, x, x_cov, cov_stride, nullptr, nullptr, nullptr, call)) != RFSGPU_OK) return rc;
  f->bSensed = true;
  return RFSGPU_OK;
}
int rfsgpu_batch_resample_sensed_async(rfsgpu_filter *f, unsigned long long call) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_RESAMPLE_SENSED;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (!batch_fills_blocks(f)) return refuse_on_kind(f, "rfsgpu_batch_resample_sensed_async (a multi-hypothesis cycle resamples inside the cycle)", ON_MH_BATCH);
  if (!f->bSensedTail) return batch_fail(f, C, "no rfsgpu_batch_cycle_sensed_async has run since the last rfsgpu_batch_sense_async: the records on the device are not those of a finished cycle");
  return batch_resample_core(f, C, nullptr, call);
}
int rfsgpu_batch_last_scan(rfsgpu_filter *f, double *z, int *n_z) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_LAST_SCAN;
  int rc = sensor_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (!z || !n_z) return batch_fail(f, C, "null output");
  if (!f->bScanHeld) return batch_fail(f, C, "no rfsgpu_batch_sense_async has run on this handle since its last host-fed cycle");
  const int nF = f->nF;
  hipSetDevice(f->device);
  std::vector<BatchFilter> rec(nF);
  HIPCHK(hipMemcpyAsync(rec.data(), f->dBFilt, (size_t)nF * sizeof(BatchFilter), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipMemcpyAsync(z, f->dBZ, (size_t)nF * RFSGPU_MAX_Z * 2 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  for (int b = 0; b < nF; b++) {
    n_z[b] = rec[b].nZ;
    memset(z + ((size_t)b * RFSGPU_MAX_Z + (size_t)n_z[b]) * 2, 0, (size_t)(RFSGPU_MAX_Z - n_z[b]) * 2 * sizeof(double));     // (beyond the set: whatever an earlier scan left)
  }
  return check_device_errors(f);     // (a scan that was cut: RFSGPU_ERR_CAPACITY once; the outputs hold the sets as delivered)
}
int rfsgpu_batch_last_cycle_lds(rfsgpu_filter *f, long long *bytes) {
  CHECK_HANDLE(f);
  int rc = batch_check(f, -1);
  if (rc != RFSGPU_OK) return rc;
  if (!bytes) return fail(f, RFSGPU_ERR_INVALID, "batch_last_cycle_lds: null output");
  *bytes = f->bLastCycleLds;
  return RFSGPU_OK;
}

// ---- [metric] per-step map error and pose error (map_metric.h) ------------------------------------------------------------------------
static int metric_check(rfsgpu_filter *f, const char *what) {
  const bool mhOff = batch_is_mh(f) && !f->mhbMetrics;     // (the step-error kernel assumes that every filter fills its block, until the switch turns its live-count form on)
  if (f->D == 2 && !f->fastSlamHandle && !f->groupShard && !mhOff) return RFSGPU_OK;
  f->err = std::string(what) + ": the device-side map / pose error serves ordinary 2-D RB-PHD handles and filter batches (RB-PHD or FastSLAM) only, not " +
           (f->D != 2 ? "the Victoria Park model" : (f->fastSlamHandle ? "a FastSLAM handle" : handle_kind_text(f)));
  if (f->D == 2 && !f->fastSlamHandle && mhOff) f->err += ": rfsgpu_batch_mh_serve_metrics switches the live-count form of the step-error kernel on";
  return RFSGPU_ERR_UNSUPPORTED;
}
static inline int metric_nf(const rfsgpu_filter *f) { return f->batch ? f->nF : 1; }
// One launch into `row` ([nF] records): the call's t / gt_pose go into a slot of the pinned staging ring, which the kernel reads in place.
// devIn (rfsgpu_batch_run_truth_async): the call's {t, pose} block is a row of the truth tables on the device instead, with a pose.
static int metric_launch(rfsgpu_filter *f, const double *t, const double *gt_pose, double w_threshold, double cutoff, double order, struct rfsgpu_step_error *row,
                         const double *devIn = nullptr) {
  const int nF = metric_nf(f);
  hipSetDevice(f->device);
  double *h = nullptr;
  int k = 0;
  if (!devIn) {
    { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
    for (int b = 0; b < nF; b++) {
      h[4 * b] = t ? t[b] : 0.0;
      for (int q = 0; q < 3; q++) h[4 * b + 1 + q] = gt_pose ? gt_pose[3 * b + q] : 0.0;
    }
  }
  MetricArg A{devIn ? devIn : h, f->dGtXY, f->dGtSeen, f->dGtN, row, w_threshold, cutoff, order, f->batch ? f->nPer : f->N, (gt_pose || devIn) ? 1 : 0, f->holes ? 1 : 0, batch_log_odds(f) ? 1 : 0};
  if (batch_is_mh(f)) {     // every filter's count is a word of its cycle block, read by the kernel where it runs: nothing waits for it
    FsCycleState S0;
    mhb_view(f, f->mhbBlock, 0, S0);
    map_metric_kernel<<<nF, 64, 0, f->stream>>>(f->B, f->cur, A, MetricLive{S0.w, FSC_WORDS, FSC_N});
  } else {
    map_metric_kernel<<<nF, 64, 0, f->stream>>>(f->B, f->cur, A);
  }
  HIPCHK(hipGetLastError());
  if (!devIn) HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
  return RFSGPU_OK;
}
static int metric_args(rfsgpu_filter *f, const char *what, const double *t, double cutoff, double order) {
  if (!t) { f->err = std::string(what) + ": null time array"; return RFSGPU_ERR_INVALID; }
  if (!(cutoff > 0) || !(order >= 1)) { f->err = std::string(what) + ": cutoff must be > 0 and order >= 1"; return RFSGPU_ERR_INVALID; }
  return RFSGPU_OK;
}
static int metric_row(rfsgpu_filter *f) {
  if (!f->dErrRow) HIPCHK(hipMalloc(&f->dErrRow, (size_t)metric_nf(f) * sizeof(struct rfsgpu_step_error)));
  return RFSGPU_OK;
}

// The switch of a multi-hypothesis batch: off at creation, so the refusals it was published with stand until a caller asks.
int rfsgpu_batch_mh_serve_metrics(rfsgpu_filter *f, int on) {
  CHECK_HANDLE(f);
  if (!batch_is_mh(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_mh_serve_metrics: not a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh)");
  if (batch_is_vp(f)) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_mh_serve_metrics: the device-side map / pose error is 2-D: it does not serve a batch of Victoria Park multi-hypothesis FastSLAM filters (rfsgpu_create_batch_vp_mh)");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  f->mhbMetrics = on != 0;
  return RFSGPU_OK;
}
int rfsgpu_set_ground_truth(rfsgpu_filter *f, int filter, const double *xy, const double *first_seen, int n) {
  CHECK_HANDLE(f);
  int rc = metric_check(f, "set_ground_truth");
  if (rc != RFSGPU_OK) return rc;
  const int nF = metric_nf(f);
  if (filter < 0 || filter >= nF) return fail(f, RFSGPU_ERR_INVALID, "set_ground_truth: filter index out of range");
  if (n < 0 || (n > 0 && !xy)) return fail(f, RFSGPU_ERR_INVALID, "set_ground_truth: bad arguments");
  if (n > RFSGPU_MAX_METRIC_SET) return fail(f, RFSGPU_ERR_INVALID, "set_ground_truth: more than RFSGPU_MAX_METRIC_SET (512) landmarks");
  hipSetDevice(f->device);
  if (!f->dGtN) {
    HIPCHK(hipMalloc(&f->dGtXY, (size_t)nF * RFSGPU_MAX_METRIC_SET * 2 * sizeof(double)));
    HIPCHK(hipMalloc(&f->dGtSeen, (size_t)nF * RFSGPU_MAX_METRIC_SET * sizeof(double)));
    int *cnt = nullptr;
    HIPCHK(hipMalloc(&cnt, (size_t)nF * sizeof(int)));
    if (hipMemset(cnt, 0, (size_t)nF * sizeof(int)) != hipSuccess) { hipFree(cnt); return fail(f, RFSGPU_ERR_HIP, "set_ground_truth: hipMemset failed"); }
    f->dGtN = cnt;
  }
  HIPCHK(hipStreamSynchronize(f->stream));   // (an enqueued metric kernel may still be reading the old set)
  std::vector<double> seen((size_t)std::max(n, 1), -1.0);
  if (first_seen) for (int m = 0; m < n; m++) seen[m] = first_seen[m];
  if (n > 0) {
    HIPCHK(hipMemcpy(f->dGtXY + (size_t)filter * RFSGPU_MAX_METRIC_SET * 2, xy, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->dGtSeen + (size_t)filter * RFSGPU_MAX_METRIC_SET, seen.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(f->dGtN + filter, &n, sizeof(int), hipMemcpyHostToDevice));
  if (f->gtSet.empty()) f->gtSet.assign(nF, 0);
  f->gtSet[filter] = 1;
  return RFSGPU_OK;
}
int rfsgpu_error_log_create(rfsgpu_filter *f, int log_capacity) {
  CHECK_HANDLE(f);
  int rc = metric_check(f, "error_log_create");
  if (rc != RFSGPU_OK) return rc;
  if (log_capacity < 0) return fail(f, RFSGPU_ERR_INVALID, "error_log_create: negative capacity");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  hipFree(f->dErrLog);
  f->dErrLog = nullptr;
  f->errLogCap = f->errLogRows = 0;
  if (log_capacity > 0) {
    HIPCHK(hipMalloc(&f->dErrLog, (size_t)log_capacity * metric_nf(f) * sizeof(struct rfsgpu_step_error)));
    f->errLogCap = log_capacity;
  }
  return RFSGPU_OK;
}
int rfsgpu_error_log_reset(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  int rc = metric_check(f, "error_log_reset");
  if (rc != RFSGPU_OK) return rc;
  f->errLogRows = 0;   // (stream order keeps a row that is still being written ahead of the next one that lands there)
  return RFSGPU_OK;
}
int rfsgpu_step_error_async(rfsgpu_filter *f, const double *t, const double *gt_pose, double w_threshold, double cutoff, double order) {
  if (!f) return RFSGPU_ERR_INVALID;
  if (!(batch_is_mh(f) && f->mhbMetrics)) {    // (a served multi-hypothesis batch: the kernel reads the counts on the device, so cycles in
    CHECK_HANDLE(f);                       //  flight stay in flight and a pending overflow is the next synchronising call's to report)
  }
  int rc = metric_check(f, "step_error_async");
  if (rc != RFSGPU_OK) return rc;
  if ((rc = metric_args(f, "step_error_async", t, cutoff, order)) != RFSGPU_OK) return rc;
  if (f->errLogRows >= f->errLogCap)
    return fail(f, RFSGPU_ERR_CAPACITY, f->errLogCap ? "step_error_async: the error log is full (rfsgpu_error_log_read, then rfsgpu_error_log_reset)"
                                                      : "step_error_async: no error log (rfsgpu_error_log_create)");
  rc = metric_launch(f, t, gt_pose, w_threshold, cutoff, order, f->dErrLog + (size_t)f->errLogRows * metric_nf(f));
  if (rc == RFSGPU_OK) f->errLogRows++;
  return rc;
}
int rfsgpu_error_log_read(rfsgpu_filter *f, struct rfsgpu_step_error *out, int max_rows, int *n_rows) {
  CHECK_HANDLE(f);
  int rc = metric_check(f, "error_log_read");
  if (rc != RFSGPU_OK) return rc;
  if (max_rows < 0 || (max_rows > 0 && !out)) return fail(f, RFSGPU_ERR_INVALID, "error_log_read: bad arguments");
  hipSetDevice(f->device);
  const int rows = std::min(max_rows, f->errLogRows);
  if (rows > 0) HIPCHK(hipMemcpyAsync(out, f->dErrLog, (size_t)rows * metric_nf(f) * sizeof(struct rfsgpu_step_error), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  if (n_rows) *n_rows = f->errLogRows;
  return RFSGPU_OK;
}
int rfsgpu_step_error(rfsgpu_filter *f, const double *t, const double *gt_pose, double w_threshold, double cutoff, double order, struct rfsgpu_step_error *out) {
  CHECK_HANDLE(f);
  int rc = metric_check(f, "step_error");
  if (rc != RFSGPU_OK) return rc;
  if ((rc = metric_args(f, "step_error", t, cutoff, order)) != RFSGPU_OK) return rc;
  if (!out) return fail(f, RFSGPU_ERR_INVALID, "step_error: null output");
  hipSetDevice(f->device);
  if ((rc = metric_row(f)) != RFSGPU_OK) return rc;
  if ((rc = metric_launch(f, t, gt_pose, w_threshold, cutoff, order, f->dErrRow)) != RFSGPU_OK) return rc;
  HIPCHK(hipMemcpyAsync(out, f->dErrRow, (size_t)metric_nf(f) * sizeof(struct rfsgpu_step_error), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return RFSGPU_OK;
}
int rfsgpu_get_map_estimate(rfsgpu_filter *f, int filter, double w_threshold, int max_n, int *n, double *mean, double *cov, double *w) {
  CHECK_HANDLE(f);
  int rc = metric_check(f, "get_map_estimate");
  if (rc != RFSGPU_OK) return rc;
  const int nF = metric_nf(f);
  if (filter < 0 || filter >= nF || max_n < 0) return fail(f, RFSGPU_ERR_INVALID, "get_map_estimate: bad arguments");
  // the selection is the kernel's own (one rule, one implementation): a launch with no pose and the metric's cheapest arguments
  std::vector<struct rfsgpu_step_error> row(nF);
  std::vector<double> t(nF, 0.0);
  if ((rc = rfsgpu_step_error(f, t.data(), nullptr, w_threshold, 1.0, 1.0, row.data())) != RFSGPU_OK) return rc;
  const int slot = (int)row[filter].best_slot;
  std::vector<double> pl;
  int cnt = 0;
  if ((rc = fetch_particle(f, slot, pl, cnt)) != RFSGPU_OK) return rc;
  const size_t c = f->cap;
  int k = 0;
  for (int m = 0; m < cnt; m++) {
    double wm = pl[m];
    if (batch_log_odds(f)) wm = 1 - 1 / (1 + exp(wm));     // a FastSLAM batch: the existence probability of the log-odds (fastslam2dSim.cpp:628)
    if ((f->holes && wm < 0) || !(wm >= w_threshold)) continue;
    if (k < max_n) {
      if (w) w[k] = wm;
      if (mean) { mean[2 * k] = pl[(size_t)PL_MX * c + m]; mean[2 * k + 1] = pl[(size_t)PL_MY * c + m]; }
      if (cov) { cov[4 * k] = pl[(size_t)PL_SXX * c + m]; cov[4 * k + 1] = cov[4 * k + 2] = pl[(size_t)PL_SXY * c + m]; cov[4 * k + 3] = pl[(size_t)PL_SYY * c + m]; }
    }
    k++;
  }
  if (n) *n = k;
  return RFSGPU_OK;
}

// ---- [estimate] per-step pose and map estimates in a device-side log (estimate_log.h) -------------------------------------------------
// Served where [metric] is served -- every call starts with metric_check -- and on an ordinary handle whose switch
// (rfsgpu_handle_serve_estimates) is on, and on a batch of Victoria Park filters whose switch (rfsgpu_batch_vp_serve_estimates) is on:
// the four log calls start with estimate_check there.
static inline int estimate_slots(const rfsgpu_filter *f) { return f->batch ? f->nPer : (f->estServe ? f->Ncap : f->N); }
static int estimate_check(rfsgpu_filter *f, const char *what) { return (f->estServe || f->estServeVpBatch) ? RFSGPU_OK : metric_check(f, what); }
// (a served handle that has run FastSLAM updates or cycles: log-odds weights, as on a FastSLAM batch)
static inline bool estimate_log_odds(const rfsgpu_filter *f) { return batch_log_odds(f) || (f->estServe && f->fastSlamHandle); }
static void estimate_log_free(rfsgpu_filter *f) {
  hipFree(f->dEstHdr); hipFree(f->dEstGauss); hipFree(f->dEstPart);
  f->dEstHdr = nullptr; f->dEstGauss = nullptr; f->dEstPart = nullptr;
  f->estLogCap = f->estLogRows = f->estMax = f->estSlots = 0;
}
// One launch into row `row` of the log: the call's times go into a slot of the pinned staging ring (metric_launch's), which the kernel
// reads in place.  devIn (rfsgpu_batch_run_truth_async): the times are the first of every four doubles of a truth table row on the device.
// behind (a served handle with nothing but FastSLAM cycles pending): the count is a word of the handle's cycle block, the launch is sized
// for max_particles.
static int estimate_launch(rfsgpu_filter *f, const double *t, double w_threshold, int row, const double *devIn = nullptr, bool behind = false) {
  const int nF = metric_nf(f);
  hipSetDevice(f->device);
  const int nPer = f->batch ? f->nPer : (behind ? f->Ncap : f->N);
  if (f->dEstPart && nPer > f->estSlots) {
    f->err = "step_estimate: the handle holds more particles than the estimate log's particle planes were created for (rfsgpu_estimate_log_create)";
    return RFSGPU_ERR_INVALID;
  }
  double *h = nullptr;
  int k = 0;
  if (!devIn) {
    { const int rc = ring_acquire(f, f->stage, &h, &k); if (rc != RFSGPU_OK) return rc; }
    for (int b = 0; b < nF; b++) h[b] = t[b];
  }
  const size_t at = (size_t)row * nF;
  EstimateArg A{devIn ? devIn : h, devIn ? 4 : 1, f->dEstHdr + at, f->dEstGauss ? f->dEstGauss + at * 6 * (size_t)f->estMax : nullptr,
                f->dEstPart ? f->dEstPart + at * 4 * (size_t)f->estSlots : nullptr, w_threshold, nPer, f->estSlots, f->estMax, f->holes ? 1 : 0,
                estimate_log_odds(f) ? 1 : 0};
  const dim3 grid(nF, 1 + (f->dEstPart ? (nPer + ESTIMATE_PART_SLOTS - 1) / ESTIMATE_PART_SLOTS : 0));
  if (batch_is_mh(f)) {     // every filter's count is a word of its cycle block, read by the kernel where it runs: nothing waits for it
    FsCycleState S0;
    mhb_view(f, f->mhbBlock, 0, S0);
    estimate_log_kernel<<<grid, 64, 0, f->stream>>>(f->B, f->cur, A, MetricLive{S0.w, FSC_WORDS, FSC_N});
  } else if (behind) {  // f->cur counts the flips of the pending cycles; a cycle that did not flip was abandoned by an overflow, and its row reads no slab
    if (f->D == 3) estimate_log_kernel<<<grid, 64, 0, f->stream>>>(f->B, f->cur, A, EstimateHandle<3, true>{f->mhc.w + FSC_N, f->mhc.w + FSC_OVF});
    else estimate_log_kernel<<<grid, 64, 0, f->stream>>>(f->B, f->cur, A, EstimateHandle<2, true>{f->mhc.w + FSC_N, f->mhc.w + FSC_OVF});
  } else if (f->batch && f->D == 3) {     // a served batch of Victoria Park filters: every filter fills its block, on both routes
    estimate_log_kernel<<<grid, 64, 0, f->stream>>>(f->B, f->cur, A, EstimateBatch<3>{});
  } else if (f->D == 3) {
    estimate_log_kernel<<<grid, 64, 0, f->stream>>>(f->B, f->cur, A, EstimateHandle<3, false>{nullptr, nullptr});
  } else {
    estimate_log_kernel<<<grid, 64, 0, f->stream>>>(f->B, f->cur, A);
  }
  HIPCHK(hipGetLastError());
  if (!devIn) HIPCHK(hipEventRecord(f->stage.ev[k], f->stream));
  return RFSGPU_OK;
}
// The switch of an ordinary handle: off at creation, so the refusals the section was published with stand until a caller asks.
int rfsgpu_handle_serve_estimates(rfsgpu_filter *f, int on) {
  CHECK_HANDLE(f);
  if (f->batch) return fail(f, RFSGPU_ERR_UNSUPPORTED, "handle_serve_estimates: a filter batch is served by [estimate] as [metric] serves it (a multi-hypothesis batch: rfsgpu_batch_mh_serve_metrics); the switch is for ordinary handles");
  if (f->groupShard) return fail(f, RFSGPU_ERR_UNSUPPORTED, "handle_serve_estimates: not available on a shard of an rfsgpu_group (the highest-weight particle and the sums would be those of one shard only)");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  if (!on) estimate_log_free(f);
  f->estServe = on != 0;
  return RFSGPU_OK;
}
// The switch of a batch of Victoria Park filters: off at creation, so the batch's refusals of the section stand until a caller asks.
// Nothing of such a batch is ever pending on the host's side (the device route keeps its ids, flags and counters on the device and
// the host never sizes by them), so rfsgpu_step_estimate_async enqueues as it stands on both routes.
int rfsgpu_batch_vp_serve_estimates(rfsgpu_filter *f, int on) {
  CHECK_HANDLE_HOST(f);
  if (!batch_is_vp(f) || batch_is_mh(f))     // (the hint: what serves [estimate] on that handle instead)
    return refuse_not(f, "batch_vp_serve_estimates: the switch is for a batch of Victoria Park filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D)",
                      !f->batch ? (f->groupShard ? ": no call of [estimate] serves a shard (rfsgpu_group_get_poses, rfsgpu_group_get_weights and rfsgpu_group_get_landmark read its state)"
                                                 : ": rfsgpu_handle_serve_estimates is its switch")
                                : (batch_is_vp(f) ? ": [estimate] does not serve it"
                                                  : (batch_is_mh(f) ? ": [estimate] serves it once rfsgpu_batch_mh_serve_metrics is on" : ": [estimate] serves it as it is (rfsgpu_estimate_log_create)")));
  if (f->bSteps == STEPS_FASTSLAM)
    return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_vp_serve_estimates: this batch steps FastSLAM filters (rfsgpu_batch_vp_serve_fastslam): the [estimate] log does not serve it");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  if (!on) estimate_log_free(f);
  f->estServeVpBatch = on != 0;
  return RFSGPU_OK;
}
int rfsgpu_estimate_log_create(rfsgpu_filter *f, int log_capacity, int max_est, int log_particles) {
  CHECK_HANDLE(f);
  int rc = estimate_check(f, "estimate_log_create");
  if (rc != RFSGPU_OK) return rc;
  if (log_capacity < 0) return fail(f, RFSGPU_ERR_INVALID, "estimate_log_create: negative capacity");
  if (max_est < 0 || max_est > f->cap) return fail(f, RFSGPU_ERR_INVALID, "estimate_log_create: max_est must lie in 0 ... gm_capacity");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));
  estimate_log_free(f);
  if (log_capacity == 0) return RFSGPU_OK;
  const size_t cells = (size_t)log_capacity * metric_nf(f);
  const int slots = estimate_slots(f);
  hipError_t e = hipMalloc(&f->dEstHdr, cells * sizeof(struct rfsgpu_step_estimate));
  if (e == hipSuccess && max_est > 0) e = hipMalloc(&f->dEstGauss, cells * 6 * (size_t)max_est * sizeof(double));
  if (e == hipSuccess && log_particles && slots > 0) e = hipMalloc(&f->dEstPart, cells * 4 * (size_t)slots * sizeof(double));
  if (e != hipSuccess) {
    estimate_log_free(f);
    f->err = std::string("estimate_log_create: hipMalloc: ") + hipGetErrorString(e);
    return RFSGPU_ERR_HIP;
  }
  f->estLogCap = log_capacity;
  f->estMax = max_est;
  f->estSlots = f->dEstPart ? slots : 0;
  return RFSGPU_OK;
}
int rfsgpu_estimate_log_reset(rfsgpu_filter *f) {
  CHECK_HANDLE(f);
  int rc = estimate_check(f, "estimate_log_reset");
  if (rc != RFSGPU_OK) return rc;
  f->estLogRows = 0;   // (stream order keeps a row that is still being written ahead of the next one that lands there)
  return RFSGPU_OK;
}
int rfsgpu_step_estimate_async(rfsgpu_filter *f, const double *t, double w_threshold) {
  if (!f) return RFSGPU_ERR_INVALID;
  // A served handle keeps its device cycles in flight: behind rfsgpu_rbphd_cycle_async cycles the count is the host's and the kernel
  // reads the state at its point of the stream; behind FastSLAM cycles (nothing stashed, no resampling call pending) it reads the
  // count on the device too.  A pending error is the next synchronising call's to report.
  const bool behind = f->estServe && f->mhcPending && !f->mhcStashedRc && !f->mhbPending && !f->rsPending;
  if (f->estServe) {
    if (!behind && !rc_only_pending(f)) { CHECK_HANDLE(f); }
  } else if (!(batch_is_mh(f) && f->mhbMetrics)) {    // (as rfsgpu_step_error_async: a served multi-hypothesis batch keeps its cycles in flight)
    CHECK_HANDLE(f);
  }
  int rc = estimate_check(f, "step_estimate_async");
  if (rc != RFSGPU_OK) return rc;
  if (!t) return fail(f, RFSGPU_ERR_INVALID, "step_estimate_async: null time array");
  if (f->estLogRows >= f->estLogCap)
    return fail(f, RFSGPU_ERR_CAPACITY, f->estLogCap ? "step_estimate_async: the estimate log is full (rfsgpu_estimate_log_read, then rfsgpu_estimate_log_reset)"
                                                      : "step_estimate_async: no estimate log (rfsgpu_estimate_log_create)");
  rc = estimate_launch(f, t, w_threshold, f->estLogRows, nullptr, behind);
  if (rc == RFSGPU_OK) f->estLogRows++;
  return rc;
}
int rfsgpu_estimate_log_read(rfsgpu_filter *f, int row_from, int max_rows, struct rfsgpu_step_estimate *hdr, double *gauss, double *part, int *n_rows) {
  CHECK_HANDLE(f);
  int rc = estimate_check(f, "estimate_log_read");
  if (rc != RFSGPU_OK) return rc;
  if (max_rows < 0) return fail(f, RFSGPU_ERR_INVALID, "estimate_log_read: negative max_rows");
  if (row_from < 0 || row_from > f->estLogRows) return fail(f, RFSGPU_ERR_INVALID, "estimate_log_read: row_from outside 0 ... the number of rows in the log");
  hipSetDevice(f->device);
  const size_t nF = (size_t)metric_nf(f), at = (size_t)row_from * nF;
  const size_t cells = (size_t)std::min(max_rows, f->estLogRows - row_from) * nF;
  if (cells > 0) {
    if (hdr) HIPCHK(hipMemcpyAsync(hdr, f->dEstHdr + at, cells * sizeof(struct rfsgpu_step_estimate), hipMemcpyDeviceToHost, f->stream));
    if (gauss && f->dEstGauss)
      HIPCHK(hipMemcpyAsync(gauss, f->dEstGauss + at * 6 * (size_t)f->estMax, cells * 6 * (size_t)f->estMax * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    if (part && f->dEstPart)
      HIPCHK(hipMemcpyAsync(part, f->dEstPart + at * 4 * (size_t)f->estSlots, cells * 4 * (size_t)f->estSlots * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  }
  HIPCHK(hipStreamSynchronize(f->stream));
  if (n_rows) *n_rows = f->estLogRows;
  return RFSGPU_OK;
}
int rfsgpu_batch_run_log_estimates(rfsgpu_filter *f, int on, double w_threshold) {
  CHECK_HANDLE_HOST(f);
  int rc = metric_check(f, "batch_run_log_estimates");
  if (rc != RFSGPU_OK) return rc;
  if (!f->batch) return fail(f, RFSGPU_ERR_UNSUPPORTED, "batch_run_log_estimates: rfsgpu_batch_run_truth_async serves filter batches only, not an ordinary handle");
  f->estRunOn = on != 0;
  f->estRunThr = w_threshold;
  return RFSGPU_OK;
}

// ---- [truth] every filter's ground truth drawn on the device, and a run of steps in one call (batch_truth.h) --------------------------
static const BatchCall BATCH_SET_TRUTH{"batch_set_truth", 0, nullptr, nullptr};
static const BatchCall BATCH_GENERATE_TRUTH{"batch_generate_truth", 0, nullptr, nullptr};
static const BatchCall BATCH_GET_TRUTH{"batch_get_truth", 0, nullptr, nullptr};
static const BatchCall BATCH_RUN_TRUTH{"batch_run_truth", 0, nullptr, nullptr};
static int truth_check(rfsgpu_filter *f, const BatchCall &C) {
  if (f->batch && f->D == 3) {
    f->err = std::string(C.who) + ": the device truth draws 2-D odometry runs: it does not serve a batch of Victoria Park filters";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  if (f->batch) return RFSGPU_OK;
  f->err = std::string(C.who) + ": the device truth serves filter batches only, not " + (f->groupShard ? "a shard of an rfsgpu_group" : "an ordinary handle");
  return RFSGPU_ERR_UNSUPPORTED;
}
// Landmarks that a run of k_full steps could place: the j with max(spacing j, j + 1) < k_full (batch_truth.h)
static long long truth_landmarks_possible(int k_full, int n_landmarks) {
  if (n_landmarks <= 0) return 0;
  const long long sp = k_full / n_landmarks;
  long long n = 0;
  while (n <= RFSGPU_SENSOR_MAX_LANDMARKS && std::max(sp * n, n + 1) < k_full) n++;
  return n;
}
int rfsgpu_batch_set_truth(rfsgpu_filter *f, int filter, const rfsgpu_truth_config *cfg, unsigned long long seed) {
  CHECK_HANDLE_HOST(f);
  const BatchCall &C = BATCH_SET_TRUTH;
  int rc = truth_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if (filter < -1 || filter >= f->nF) return batch_fail(f, C, "filter index out of range");
  if (!cfg) return batch_fail(f, C, "null configuration");
  const double d[11] = {cfg->dt, cfg->max_dx, cfg->max_dy, cfg->max_dz, cfg->min_dx, cfg->var_odo[0], cfg->var_odo[1], cfg->var_odo[2], cfg->rmax, cfg->rmin, 0.0};
  static const char *const dn[10] = {"dt", "max_dx", "max_dy", "max_dz", "min_dx", "var_odo[0]", "var_odo[1]", "var_odo[2]", "rmax", "rmin"};
  for (int q = 0; q < 10; q++)
    if (!std::isfinite(d[q]) || d[q] < 0.0) return batch_fail(f, C, std::string(dn[q]) + " must be finite and not negative");
  const int iv[5] = {cfg->k_full, cfg->n_segments, cfg->n_landmarks, cfg->n_still, cfg->n_pinned};
  static const char *const in[5] = {"k_full", "n_segments", "n_landmarks", "n_still", "n_pinned"};
  for (int q = 0; q < 5; q++)
    if (iv[q] < 0) return batch_fail(f, C, std::string(in[q]) + " must not be negative");
  if (cfg->min_dx > cfg->max_dx) return batch_fail(f, C, "min_dx must not exceed max_dx");
  if (!(cfg->rmin < cfg->rmax)) return batch_fail(f, C, "rmin must lie below rmax");
  if (cfg->n_segments < 1) return batch_fail(f, C, "n_segments must be at least 1");
  if (cfg->k_full / cfg->n_segments == 0) return batch_fail(f, C, "k_full / n_segments is 0: fewer steps than segments");
  if (cfg->n_landmarks > 0 && cfg->k_full / cfg->n_landmarks == 0) return batch_fail(f, C, "k_full / n_landmarks is 0: fewer steps than landmarks");
  if (truth_landmarks_possible(cfg->k_full, cfg->n_landmarks) > RFSGPU_SENSOR_MAX_LANDMARKS)
    return batch_fail(f, C, "a run of k_full steps could place more than RFSGPU_SENSOR_MAX_LANDMARKS landmarks");
  BatchTruth T;
  memset(&T, 0, sizeof T);
  T.dt = cfg->dt; T.maxDx = cfg->max_dx; T.maxDy = cfg->max_dy; T.maxDz = cfg->max_dz; T.minDx = cfg->min_dx;
  for (int q = 0; q < 3; q++) T.sdOdoDt[q] = sqrt(cfg->var_odo[q]) * cfg->dt;
  T.rmax = cfg->rmax; T.rmin = cfg->rmin;
  T.seed = seed;
  T.kFull = cfg->k_full; T.nSegments = cfg->n_segments; T.nLandmarks = cfg->n_landmarks; T.nStill = cfg->n_still; T.nPinned = cfg->n_pinned;
  for (int b = (filter < 0 ? 0 : filter); b < (filter < 0 ? f->nF : filter + 1); b++) { f->bTruth[b] = T; f->bTruthSet[b] = 1; }
  return RFSGPU_OK;
}
int rfsgpu_batch_generate_truth(rfsgpu_filter *f, int n_steps) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_GENERATE_TRUTH;
  int rc = truth_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  const int nF = f->nF;
  if (n_steps < 2 || n_steps > RFSGPU_TRUTH_MAX_STEPS) return batch_fail(f, C, "n_steps must lie in 2 ... RFSGPU_TRUTH_MAX_STEPS");
  for (int b = 0; b < nF; b++)
    if (!f->bTruthSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no truth configuration (rfsgpu_batch_set_truth)");
  for (int b = 0; b < nF; b++)
    if (n_steps > f->bTruth[b].kFull) return batch_fail(f, C, "filter " + std::to_string(b) + ": n_steps exceeds its k_full");
  hipSetDevice(f->device);
  HIPCHK(hipStreamSynchronize(f->stream));     // (a run in flight reads the tables)
  if (!f->dTruthCfg) {
    HIPCHK(hipMalloc(&f->dTruthCfg, (size_t)nF * sizeof(BatchTruth)));
    HIPCHK(hipMalloc(&f->dTruthLm, (size_t)nF * SENSOR_MAX_LANDMARKS * 2 * sizeof(double)));
    HIPCHK(hipMalloc(&f->dTruthSeen, (size_t)nF * SENSOR_MAX_LANDMARKS * sizeof(double)));
    HIPCHK(hipMalloc(&f->dTruthCounts, (size_t)nF * 2 * sizeof(int)));
  }
  f->truthK = 0;     // (from here on the old tables are gone)
  if ((size_t)n_steps > f->truthRows) {
    hipFree(f->dTruthProp); hipFree(f->dTruthGt); hipFree(f->dTruthTgt);
    f->dTruthProp = nullptr; f->dTruthGt = nullptr; f->dTruthTgt = nullptr;
    f->truthRows = 0;
    HIPCHK(hipMalloc(&f->dTruthProp, (size_t)n_steps * nF * sizeof(BatchPropIn)));
    HIPCHK(hipMalloc(&f->dTruthGt, (size_t)n_steps * nF * 3 * sizeof(double)));
    HIPCHK(hipMalloc(&f->dTruthTgt, (size_t)n_steps * nF * 4 * sizeof(double)));
    f->truthRows = (size_t)n_steps;
  }
  HIPCHK(hipMemcpy(f->dTruthCfg, f->bTruth.data(), (size_t)nF * sizeof(BatchTruth), hipMemcpyHostToDevice));
  BatchTruthArg A{f->dTruthCfg, f->dTruthProp, f->dTruthGt, f->dTruthTgt, f->dTruthLm, f->dTruthSeen, f->dTruthCounts, nF, n_steps};
  batch_truth_kernel<<<nF, TRUTH_THREADS, 0, f->stream>>>(A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(f->stream));
  f->truthK = n_steps;
  return RFSGPU_OK;
}
int rfsgpu_batch_get_truth(rfsgpu_filter *f, int filter, double *gt, double *odom, double *landmarks_xy, double *first_seen, int *n_landmarks, int *n_det_max) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_GET_TRUTH;
  int rc = truth_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  const int nF = f->nF, K = f->truthK;
  if (filter < 0 || filter >= nF) return batch_fail(f, C, "filter index out of range");
  if (K <= 0) return batch_fail(f, C, "no rfsgpu_batch_generate_truth has run on this handle");
  hipSetDevice(f->device);
  int cnt[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(cnt, f->dTruthCounts + 2 * (size_t)filter, sizeof cnt, hipMemcpyDeviceToHost, f->stream));
  if (gt) HIPCHK(hipMemcpy2DAsync(gt, 3 * sizeof(double), f->dTruthGt + 3 * (size_t)filter, (size_t)nF * 3 * sizeof(double), 3 * sizeof(double), (size_t)K, hipMemcpyDeviceToHost, f->stream));
  if (odom) HIPCHK(hipMemcpy2DAsync(odom, 3 * sizeof(double), f->dTruthProp[filter].u, (size_t)nF * sizeof(BatchPropIn), 3 * sizeof(double), (size_t)K, hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  const int L = std::min(std::max(cnt[0], 0), RFSGPU_SENSOR_MAX_LANDMARKS);
  if (L > 0 && landmarks_xy) HIPCHK(hipMemcpy(landmarks_xy, f->dTruthLm + (size_t)filter * SENSOR_MAX_LANDMARKS * 2, (size_t)L * 2 * sizeof(double), hipMemcpyDeviceToHost));
  if (L > 0 && first_seen) HIPCHK(hipMemcpy(first_seen, f->dTruthSeen + (size_t)filter * SENSOR_MAX_LANDMARKS, (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
  if (n_landmarks) *n_landmarks = L;
  if (n_det_max) *n_det_max = cnt[1];
  return RFSGPU_OK;
}
int rfsgpu_batch_run_truth_async(rfsgpu_filter *f, int k_from, int k_to, int track_errors, double w_threshold, double cutoff, double order) {
  CHECK_HANDLE(f);
  const BatchCall &C = BATCH_RUN_TRUTH;
  int rc = truth_check(f, C);
  if (rc != RFSGPU_OK) return rc;
  if ((rc = sensor_check(f, C)) != RFSGPU_OK) return rc;
  const int nF = f->nF;
  if (f->truthK <= 0) return batch_fail(f, C, "no rfsgpu_batch_generate_truth has run on this handle: filter 0 (and every other) has no truth tables");
  if (k_from < 1 || k_to < k_from || k_to > f->truthK) return batch_fail(f, C, "the steps must satisfy 1 <= k_from <= k_to <= n_steps (" + std::to_string(f->truthK) + ")");
  // everything the per-step calls would refuse, before the first of them enqueues anything
  // (the kind: a FastSLAM or multi-hypothesis batch gets here with its switch on only, sensor_check above; a multi-hypothesis cycle
  //  resamples inside the cycle, by thresholds that have defaults, and only RB-PHD filters have births)
  const BatchSteps kind = f->bSteps == STEPS_UNDECIDED ? STEPS_RBPHD : f->bSteps;     // (an undecided batch: its first sensed cycle makes it an RB-PHD batch)
  for (int b = 0; b < nF; b++) {
    if (!f->bSensorSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no sensor (rfsgpu_batch_set_sensor)");
    if (!f->bMotionSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no motion parameters (rfsgpu_batch_set_motion_odometry)");
    if (kind != STEPS_MH && !f->bResSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no resampling thresholds (rfsgpu_batch_set_resampling)");
    if (kind == STEPS_RBPHD && f->bCfg[b].birthGaussianMeasurementCountThreshold != 1u) {
      f->err = "batch_run_truth: a filter batch takes immediate births only (birthGaussianMeasurementCountThreshold 1)";
      return RFSGPU_ERR_UNSUPPORTED;
    }
  }
  if (kind != STEPS_MH && f->nPer > RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER) {
    f->err = "batch_run_truth: more than RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER particles per filter (one workgroup resamples a filter)";
    return RFSGPU_ERR_UNSUPPORTED;
  }
  if (track_errors) {
    if ((rc = metric_check(f, "batch_run_truth")) != RFSGPU_OK) return rc;
    if (!(cutoff > 0) || !(order >= 1)) return batch_fail(f, C, "cutoff must be > 0 and order >= 1");
    for (int b = 0; b < nF; b++)
      if (f->gtSet.empty() || !f->gtSet[b]) return batch_fail(f, C, "filter " + std::to_string(b) + " has no ground truth for its step errors (rfsgpu_set_ground_truth)");
    if (f->errLogCap <= 0) return batch_fail(f, C, "track_errors without an error log (rfsgpu_error_log_create)");
    if (f->errLogRows + (k_to - k_from) > f->errLogCap) {
      f->err = "batch_run_truth: the error log has fewer free rows than the run has steps (rfsgpu_error_log_read, then rfsgpu_error_log_reset)";
      return RFSGPU_ERR_CAPACITY;
    }
  }
  if (f->estRunOn) {     // rfsgpu_batch_run_log_estimates: one estimate row per step, beside the error row
    if ((rc = metric_check(f, "batch_run_truth")) != RFSGPU_OK) return rc;
    if (f->estLogRows + (k_to - k_from) > f->estLogCap) {
      f->err = f->estLogCap ? "batch_run_truth: the estimate log has fewer free rows than the run has steps (rfsgpu_estimate_log_read, then rfsgpu_estimate_log_reset)"
                            : "batch_run_truth: rfsgpu_batch_run_log_estimates is on without an estimate log (rfsgpu_estimate_log_create)";
      return RFSGPU_ERR_CAPACITY;
    }
  }
  for (int k = k_from; k < k_to; k++) {
    const size_t row = (size_t)k * nF;
    const unsigned long long call = (unsigned long long)k;
    if ((rc = batch_propagate_core(f, nullptr, nullptr, nullptr, f->dTruthProp + row, call)) != RFSGPU_OK) return rc;
    if ((rc = batch_sense_core(f, nullptr, f->dTruthGt + 3 * row, call)) != RFSGPU_OK) return rc;
    if (kind == STEPS_RBPHD) {
      if ((rc = rfsgpu_batch_cycle_sensed_async(f, 1, nullptr, nullptr, 0, 1)) != RFSGPU_OK) return rc;
    } else if (kind == STEPS_FASTSLAM) {
      if ((rc = batch_enter_dev_route(f)) != RFSGPU_OK) return rc;     // (as rfsgpu_batch_fastslam_cycle_sensed_async; once per handle)
      if ((rc = batch_fs_cycle_core(f, 1, nullptr, nullptr, 0, nullptr, nullptr, 1)) != RFSGPU_OK) return rc;
      f->bSensed = true;
    } else {
      if ((rc = batch_mh_cycle_core(f, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, call)) != RFSGPU_OK) return rc;
      f->bSensed = true;
    }
    if (kind != STEPS_MH && (rc = batch_resample_core(f, BATCH_RESAMPLE_SENSED, nullptr, call, k == k_from)) != RFSGPU_OK) return rc;
    if (track_errors) {
      if ((rc = metric_launch(f, nullptr, nullptr, w_threshold, cutoff, order, f->dErrLog + (size_t)f->errLogRows * nF, f->dTruthTgt + 4 * row)) != RFSGPU_OK) return rc;
      f->errLogRows++;
    }
    if (f->estRunOn) {
      if ((rc = estimate_launch(f, nullptr, f->estRunThr, f->estLogRows, f->dTruthTgt + 4 * row)) != RFSGPU_OK) return rc;
      f->estLogRows++;
    }
  }
  return RFSGPU_OK;
}

}  // extern "C"

#include "group.h"
