// fastslam_sensed.h -- the per-cycle records of a FastSLAM or multi-hypothesis FastSLAM batch whose scans the device sensor drew
// (batch_sensor.h): the one kernel at the head of rfsgpu_batch_fastslam_cycle_sensed_async / rfsgpu_batch_fastslam_mh_cycle_sensed_async.
//
// Why here: a FastSLAM record (FsBatchFilter / MhBatchFilter, fastslam.h) is configuration but for three fields that depend on the
// scan's count or on the call -- pfa = clutterIntensityIntegral / nZ (FastSLAM.hpp:561-562), prune = nZ >= pruningMeasurementsThreshold
// (:611) and, multi-hypothesis, the cycle's resampling draw.  The host-fed cycle computes them from the caller's counts; a sensed cycle
// has no count on the host, so one lane per filter derives them from the sensor's BatchFilter record (nZ, zOff) and a template table
// that the host stages only when a configuration has changed.  The update kernels read the finished records as they always have.
#pragma once
#include "common.h"
#include "fastslam.h"
#include "batch_loop.h"

// The static part of filter b's record, with the two values the count-dependent fields are derived from
template <class Rec>
struct FsSensedTemplate {
  Rec rec;               // every static field as the host-fed cycle fills it; nZ, zOff, F.pfa, prune (and u01) are zero
  double pfaNum;         // clutterIntensityIntegral: clutter * 2 pi (rmax - rmin), by the host-fed route's own expression (fs_pfa_num)
  unsigned pruneThr;     // pruningMeasurementsThreshold
  int pad;
};

// (the draw of a multi-hypothesis cycle's systematic plan: the resampling draw of (the filter's motion key, call), batch_loop.h)
__device__ __forceinline__ void fs_sensed_draw(FsBatchFilter &, const BatchMotion *, int, unsigned long long) {}
__device__ __forceinline__ void fs_sensed_draw(MhBatchFilter &T, const BatchMotion *mot, int b, unsigned long long call) { T.u01 = batch_resample_draw(mot[b].seed, call); }

// One lane per filter; nF is the host's, lastNZ [nF] or null.  The count is the sensor's own (it never exceeds the sensor's max_nz <= RFSGPU_MAX_Z; the
// clamp keeps a record that was never written from carrying the update kernels past their set).
template <class Rec>
__global__ __launch_bounds__(64) void fs_sensed_records_kernel(const FsSensedTemplate<Rec> *tmpl, const BatchFilter *sensed, Rec *out, const BatchMotion *mot, int nF,
                                                               unsigned long long call, int *lastNZ) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nF) return;
  Rec T = tmpl[b].rec;
  const int nZ = min(max(sensed[b].nZ, 0), RFSGPU_MAX_Z);
  T.nZ = nZ;
  T.zOff = b * (RFSGPU_MAX_Z * 2);                        // == the sensor record's zOff: every filter's set at its fixed offset
  T.F.pfa = __ddiv_rn(tmpl[b].pfaNum, (double)nZ);        // one correctly rounded division, as the host's (inf / NaN at 0: never read)
  T.prune = ((unsigned)nZ >= tmpl[b].pruneThr) ? 1 : 0;
  fs_sensed_draw(T, mot, b, call);
  out[b] = T;
  if (lastNZ) lastNZ[b] = nZ;      // (compact, for the host's read-back of a multi-hypothesis cycle's counts; null: nobody reads them)
}
