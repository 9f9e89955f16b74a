// batch_sensor.h -- the simulated range-bearing sensor of every filter of a batch on the device: generateMeasurements of the
// reference's 2-D simulator (src/rbphdslam2dSim.cpp:283-366) for one time step -- MeasurementModel::sample
// (include/MeasurementModel.hpp:129-159) with MeasurementModel_RngBrg::measure (src/MeasurementModel_RngBrg.cpp:70-115) per landmark,
// the Pd draw, the Poisson clutter count by the 100-entry table, the clutter points -- for every filter in one launch.
//
// Why here: the scans were the one per-step table of a batch's device loop that the host still built (two Python loops over steps x
// landmarks and steps x filters: longer than the filtering itself, and nothing of it could be enqueued ahead).  A filter's scan depends
// on the ground-truth pose, the landmarks and the sensor's parameters only, so the kernel draws it where the step kernel reads it and
// writes the cycle's BatchFilter record next to it: the host hands over one pose per filter.
//
// Random numbers: Philox4x32-10 (motion.h) under the SENSOR's key with counter (index, block | attempt << 8, call lo, call hi):
//   block 3, index = landmark m   g = (rad cos ang, rad sin ang), rad = sqrt(-2 ln u1), ang = 2 pi u2, u in (0, 1] (philox_u01)
//   block 4, index = landmark m   the detection draw u = sensor_u01(r0, r1) in [0, 1)
//   block 5, index = 0            the clutter-count draw
//   block 6, index = clutter j    attempt a = 0, 1, ... of point j's range draw
//   block 7, index = clutter j    point j's bearing draw
// (propagation has blocks 0 and 1, the resampling draw block 2: batch_loop.h).  Every value is a pure function of (key, call, block,
// index, attempt): a scan depends neither on the filter's place in the batch nor on what the other filters hold.
#pragma once
#include "common.h"
#include "motion.h"

#define SENSOR_MAX_LANDMARKS 512      // == RFSGPU_SENSOR_MAX_LANDMARKS (rfsgpu.h)
#define SENSOR_CMF 100                // the reference's table (rbphdslam2dSim.cpp:295-296)
#define SENSOR_MAX_REDRAWS 64         // attempts 0 ... 63 of a clutter range; then the fall-back below
#define SENSOR_BLOCK_NOISE 3u
#define SENSOR_BLOCK_DETECT 4u
#define SENSOR_BLOCK_COUNT 5u
#define SENSOR_BLOCK_RANGE 6u
#define SENSOR_BLOCK_BEARING 7u

struct BatchSensor {                  // rfsgpu_batch_set_sensor, per filter
  double L[3];                        // lower Cholesky factor of R: L00, L10, L11
  double Pd, rmin, rmax;
  double cmf[SENSOR_CMF];             // Poisson CMF of the mean clutter count, as the reference's loop rounds it
  unsigned long long seed;            // the sensor's Philox key
  int nLm, maxNz;
};
struct BatchSensorArg {
  const BatchSensor *sensor;          // [nF]
  const double *lm;                   // [nF][SENSOR_MAX_LANDMARKS][2]
  const double *pose;                 // [nF][3] this call's ground-truth poses
  const int *caps;                    // [nF][2] evalCap, useW of the filter's configuration
  int *prevCount;                     // [nF] the count of the last non-empty set a cycle has consumed (batch_inherit_dev_kernel keeps it)
  double *z;                          // [nF][RFSGPU_MAX_Z * 2] the batch's measurement table: filter b's set at the fixed offset b * 2 * RFSGPU_MAX_Z
  BatchFilter *filt;                  // [nF] this cycle's records
  int *err, *errFilter;               // the device error word; [1] the lowest filter whose scan was cut (INT_MAX: none)
  int nF;
};

// (a, b) -> uniform in [0, 1): 53 bits, as drand48 never 1
__host__ __device__ inline double sensor_u01(unsigned a, unsigned b) {
  const unsigned long long m = (((unsigned long long)a << 32) | b) >> 11;
  return (double)m * (1.0 / 9007199254740992.0);
}

// One wavefront per filter.  Detections: landmarks in chunks of 64, one per lane; kept ones are compacted in landmark order by
// ballot + popcount.  Clutter: the count is the number of table entries 0 ... 98 below the draw (the table does not fall, so this is
// the first n with u <= cmf[n], and 99 where the reference walks off its table); point j goes to lane j & 63.  A set beyond maxNz is cut
// to its first maxNz entries (detections before clutter) and the filter is reported through the error word.
__global__ __launch_bounds__(64) void batch_sense_kernel(BatchSensorArg A, unsigned callLo, unsigned callHi) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= A.nF) return;
  const BatchSensor &S = A.sensor[b];
  const int nLm = min(max(S.nLm, 0), SENSOR_MAX_LANDMARKS), maxNz = min(max(S.maxNz, 0), RFSGPU_MAX_Z);
  const double rmin = S.rmin, rmax = S.rmax, Pd = S.Pd;
  const double px = A.pose[3 * b], py = A.pose[3 * b + 1], pth = A.pose[3 * b + 2];
  const unsigned k0 = (unsigned)(S.seed & 0xffffffffull), k1 = (unsigned)(S.seed >> 32);
  const double *lm = A.lm + (size_t)b * (SENSOR_MAX_LANDMARKS * 2);
  double *zs = A.z + (size_t)b * (RFSGPU_MAX_Z * 2);
  const unsigned long long below = (1ull << lane) - 1ull;     // the lanes before this one
  unsigned r[4];
  int n = 0;     // entries so far, stored or cut (wave-uniform)
  for (int m0 = 0; m0 < nLm; m0 += 64) {
    const int m = m0 + lane;
    bool keep = false;
    double zr = 0.0, zb = 0.0;
    if (m < nLm) {
      const double dx = lm[2 * m] - px, dy = lm[2 * m + 1] - py;
      const double range = sqrt(dx * dx + dy * dy);
      if (!(range > rmax || range < rmin)) {                 // measure() succeeded (:111-114)
        double bearing = atan2(dy, dx) - pth;
        for (int q = 0; q < 16 && bearing > RFS_PI; q++) bearing -= 2 * RFS_PI;     // (the host bounds |theta|: the walks end)
        for (int q = 0; q < 16 && bearing < -RFS_PI; q++) bearing += 2 * RFS_PI;
        philox4x32_10((unsigned)m, SENSOR_BLOCK_NOISE, callLo, callHi, k0, k1, r);
        const double rad = sqrt(-2.0 * log(philox_u01(r[0], r[1]))), ang = 2.0 * RFS_PI * philox_u01(r[2], r[3]);
        const double g0 = rad * cos(ang), g1 = rad * sin(ang);
        zr = range + S.L[0] * g0;                            // z + L g (RandomVec::sample); the bearing is not wrapped again
        zb = bearing + (S.L[1] * g0 + S.L[2] * g1);
        philox4x32_10((unsigned)m, SENSOR_BLOCK_DETECT, callLo, callHi, k0, k1, r);
        keep = zr <= rmax && zr >= rmin && sensor_u01(r[0], r[1]) <= Pd;            // (:331)
      }
    }
    const unsigned long long mask = __ballot(keep);
    const int pos = n + __popcll(mask & below);
    if (keep && pos < maxNz) { zs[2 * pos] = zr; zs[2 * pos + 1] = zb; }
    n += __popcll(mask);
  }
  // clutter (:344-362)
  philox4x32_10(0u, SENSOR_BLOCK_COUNT, callLo, callHi, k0, k1, r);
  const double uc = sensor_u01(r[0], r[1]);
  const int nC = __popcll(__ballot(uc > S.cmf[lane])) + __popcll(__ballot(lane + 64 < SENSOR_CMF - 1 && uc > S.cmf[min(lane + 64, SENSOR_CMF - 1)]));
  for (int j = lane; j < nC; j += 64) {
    const int pos = n + j;
    if (pos >= maxNz) break;
    // r = u rmax, drawn again while r < rmin: attempt a is block (6 | a << 8).  After SENSOR_MAX_REDRAWS attempts below rmin (probability
    // (rmin / rmax)^64) the last draw is mapped into the range instead: r = rmin + u (rmax - rmin).
    double u = 0.0, cr = 0.0;
    bool ok = false;
    for (unsigned a = 0; a < SENSOR_MAX_REDRAWS && !ok; a++) {
      philox4x32_10((unsigned)j, SENSOR_BLOCK_RANGE | (a << 8), callLo, callHi, k0, k1, r);
      u = sensor_u01(r[0], r[1]);
      cr = u * rmax;
      ok = !(cr < rmin);
    }
    if (!ok) cr = rmin + u * (rmax - rmin);
    philox4x32_10((unsigned)j, SENSOR_BLOCK_BEARING, callLo, callHi, k0, k1, r);
    zs[2 * pos] = cr;
    zs[2 * pos + 1] = sensor_u01(r[0], r[1]) * 2 * RFS_PI - RFS_PI;
  }
  n += nC;
  if (lane == 0) {
    BatchFilter F;
    F.nZ = min(n, maxNz);
    F.nZprev = A.prevCount[b];
    F.evalCap = A.caps[2 * b];
    F.useW = A.caps[2 * b + 1];
    F.zOff = b * (RFSGPU_MAX_Z * 2);
    F.pad[0] = F.pad[1] = F.pad[2] = 0;
    A.filt[b] = F;
    if (n > maxNz) { atomicOr(A.err, ERRBIT_SCAN); atomicMin(A.errFilter, b); }
  }
}
