// batch_truth.h -- the ground truth of every filter of a batch drawn on the device: generateTrajectory, generateOdometry and
// generateLandmarks of the reference's 2-D simulator (src/rbphdslam2dSim.cpp:146-284) by the rules of sim2d_driver.generate, statement
// by statement, plus the two tables the host built from them per filter (first_seen_times, the first term of sensor_max_nz) -- for
// every filter in one launch, written as the step-major tables that the per-step kernels of a batch read their inputs from.
//
// Why here: with propagation, resampling, the error curves and the scans on the device, drawing the trajectories in three Python loops
// over steps and building a [K, L] range table per filter twice cost more than filtering the sweep (README, device-sensor row), and a
// step's four or five calls each copied a row of host tables into the pinned ring.  With the truth in device tables, row k of them IS
// call k's input, and the loop over steps can live behind one entry point (rfsgpu_batch_run_truth_async).
//
// Random numbers: Philox4x32-10 (motion.h) under the TRUTH key with counter (index, block | attempt << 8, 0, 0); the blocks are numbered
// after the sensor's (batch_sensor.h: 3 ... 7; propagation 0, 1; the resampling draw 2), so one key may serve everything:
//   block 8,  index = segment s   attempt a = 0, 1, ... of the segment's dx draw, u = sensor_u01(r0, r1) in [0, 1)
//   block 9,  index = segment s   dy from words 0, 1 and dz from words 2, 3
//   block 10, index = landmark j  r = u1 rmax (words 0, 1), b = u2 2 pi (words 2, 3)
//   block 11, index = step k      g_x = rad cos ang, g_y = rad sin ang (the Box-Muller form of batch_propagate_kernel)
//   block 12, index = step k      g_theta = rad cos ang
// Every value is a pure function of (key, block, index, attempt): a filter's truth depends neither on its place in the batch nor on
// the others.  The realisations are not numpy's: the model is generate()'s, the generator is not.
//
// Which step starts segment s, which step places landmark j (generate() walks the steps with a counter; here each step finds its own):
//   segment s starts at max(spacing s, n_still + 1 + s), spacing = k_full / n_segments: the walk starts at most one segment per step,
//     so where the spacing is small the segments catch up one step at a time.  Step k > n_still is in segment
//     min(k / spacing, k - n_still - 1); the steps up to n_still do not move.
//   landmark j is placed at step k_j = max(lspacing j, j + 1), lspacing = k_full / n_landmarks, when k_j < n_steps; n_landmarks is
//     the spacing's source only: the walk places a landmark wherever the rule allows (51 of them with k_full 3001, n_landmarks 50).
#pragma once
#include "common.h"
#include "motion.h"
#include "batch_loop.h"
#include "batch_sensor.h"

#define TRUTH_MAX_STEPS 4096          // == RFSGPU_TRUTH_MAX_STEPS (rfsgpu.h)
#define TRUTH_THREADS 256
#define TRUTH_CHUNK 256               // steps whose displacements and poses a workgroup holds in LDS at a time
#define TRUTH_MAX_REDRAWS 64          // == SENSOR_MAX_REDRAWS: attempts 0 ... 63 of a segment's dx, then the fall-back below
#define TRUTH_BLOCK_DX 8u
#define TRUTH_BLOCK_DYZ 9u
#define TRUTH_BLOCK_LANDMARK 10u
#define TRUTH_BLOCK_ODO_XY 11u
#define TRUTH_BLOCK_ODO_TH 12u

struct BatchTruth {                   // rfsgpu_batch_set_truth, per filter
  double dt, maxDx, maxDy, maxDz, minDx;
  double sdOdoDt[3];                  // sqrt(var_odo) * dt
  double rmax, rmin;
  unsigned long long seed;            // the truth's Philox key
  int kFull, nSegments, nLandmarks, nStill, nPinned, pad;
};
struct BatchTruthArg {
  const BatchTruth *cfg;              // [nF]
  BatchPropIn *prop;                  // [K][nF] row k: call k's propagation input (u = odometry, pinPose = gt[k], pin = k <= n_pinned)
  double *gt;                         // [K][nF][3] row k: call k's sensing poses
  double *tgt;                        // [K][nF][4] row k: {t = k dt, gt[k]}, the step-error kernel's input block
  double *lm;                         // [nF][SENSOR_MAX_LANDMARKS][2]
  double *firstSeen;                  // [nF][SENSOR_MAX_LANDMARKS] the time of the first step k >= 1 with the true range in [rmin, rmax]; -1: none
  int *counts;                        // [nF][2] landmarks placed, n_det_max
  int nF, K;
};

// The dx of a segment from its attempts' draws: the first u whose u max_dx dt is not below min_dx dt, or -- after TRUTH_MAX_REDRAWS
// attempts -- the LAST draw mapped into the limits (the fall-back rule of SENSOR_MAX_REDRAWS).  No fused multiply-add: the products
// and sums round as numpy's do.
__device__ __forceinline__ double truth_dx_of_draw(double u, bool ok, double maxDx, double minDx, double dt) {
  return ok ? __dmul_rn(__dmul_rn(u, maxDx), dt) : __dmul_rn(__dadd_rn(minDx, __dmul_rn(u, __dsub_rn(maxDx, minDx))), dt);
}

// One workgroup per filter.  The draws and the odometry are parallel over steps (every step draws its own segment's three numbers:
// a segment is a handful of Philox blocks, and no table of segments is needed, whose length only n_steps bounds); the pose chain is
// sequential in k by lane 0, a chunk of TRUTH_CHUNK steps at a time from LDS, with cos / sin of the heading change computed by all
// lanes beforehand; landmarks are parallel over j; the L x K range tests are spread over all lanes, lanes over steps: per step the
// count of landmarks in range (an LDS maximum), per landmark the smallest such step (an LDS minimum).  Every loop is bounded by a
// number the host validated, clamped here: K by TRUTH_MAX_STEPS, the landmarks by SENSOR_MAX_LANDMARKS, the redraws by their define.
__global__ __launch_bounds__(TRUTH_THREADS) void batch_truth_kernel(BatchTruthArg A) {
  __shared__ double sU0[TRUTH_CHUNK], sU1[TRUTH_CHUNK], sCd[TRUTH_CHUNK], sSd[TRUTH_CHUNK];
  __shared__ double sGt[TRUTH_CHUNK * 3];
  __shared__ double sLm[SENSOR_MAX_LANDMARKS * 2];
  __shared__ int sFirst[SENSOR_MAX_LANDMARKS];
  __shared__ int sNLm, sDetMax;
  const int b = blockIdx.x, t = threadIdx.x, nF = A.nF;
  if (b >= nF) return;
  const BatchTruth C = A.cfg[b];
  const int K = min(max(A.K, 0), TRUTH_MAX_STEPS);
  const unsigned k0 = (unsigned)(C.seed & 0xffffffffull), k1 = (unsigned)(C.seed >> 32);
  const int spacing = max(C.kFull / max(C.nSegments, 1), 1);
  unsigned r[4];
  double px = 0.0, py = 0.0, pth = 0.0;      // (lane 0: the chain's pose, carried from chunk to chunk)
  for (int c0 = 0; c0 < K; c0 += TRUTH_CHUNK) {
    const int k = c0 + t, nc = min(TRUTH_CHUNK, K - c0);
    if (k < K) {
      double dx = 0.0, dy = 0.0, dz = 0.0, ox = 0.0, oy = 0.0, oth = 0.0;
      if (k > C.nStill) {
        const unsigned s = (unsigned)min(k / spacing, k - C.nStill - 1);
        double u = 0.0;
        bool ok = false;
        for (unsigned a = 0; a < TRUTH_MAX_REDRAWS && !ok; a++) {
          philox4x32_10(s, TRUTH_BLOCK_DX | (a << 8), 0u, 0u, k0, k1, r);
          u = sensor_u01(r[0], r[1]);
          ok = !(__dmul_rn(__dmul_rn(u, C.maxDx), C.dt) < __dmul_rn(C.minDx, C.dt));
        }
        dx = truth_dx_of_draw(u, ok, C.maxDx, C.minDx, C.dt);
        philox4x32_10(s, TRUTH_BLOCK_DYZ, 0u, 0u, k0, k1, r);
        dy = __dmul_rn(__dsub_rn(__dmul_rn(__dmul_rn(sensor_u01(r[0], r[1]), C.maxDy), 2.0), C.maxDy), C.dt);
        dz = __dmul_rn(__dsub_rn(__dmul_rn(__dmul_rn(sensor_u01(r[2], r[3]), C.maxDz), 2.0), C.maxDz), C.dt);
      }
      if (k >= 1) {      // odom[k] = disp[k] + sqrt(var_odo) dt g; odom[0] = 0
        philox4x32_10((unsigned)k, TRUTH_BLOCK_ODO_XY, 0u, 0u, k0, k1, r);
        double rad = sqrt(-2.0 * log(philox_u01(r[0], r[1]))), ang = 2.0 * RFS_PI * philox_u01(r[2], r[3]);
        ox = dx + C.sdOdoDt[0] * (rad * cos(ang));
        oy = dy + C.sdOdoDt[1] * (rad * sin(ang));
        philox4x32_10((unsigned)k, TRUTH_BLOCK_ODO_TH, 0u, 0u, k0, k1, r);
        rad = sqrt(-2.0 * log(philox_u01(r[0], r[1]))); ang = 2.0 * RFS_PI * philox_u01(r[2], r[3]);
        oth = dz + C.sdOdoDt[2] * (rad * cos(ang));
      }
      sU0[t] = dx; sU1[t] = dy; sCd[t] = cos(dz); sSd[t] = sin(dz);
      BatchPropIn &I = A.prop[(size_t)k * nF + b];
      I.u[0] = ox; I.u[1] = oy; I.u[2] = oth;
      I.pin = k <= C.nPinned ? 1 : 0;
      I.pad = 0;
    }
    __syncthreads();
    if (t == 0) {      // gt[k] = step(gt[k - 1], disp[k]) in the expression order of batch_propagate_kernel; gt[0] = 0
      for (int i = 0; i < nc; i++) {
        if (c0 + i >= 1) {
          const double ct = cos(pth), st = sin(pth), cd = sCd[i], sd = sSd[i];
          px = px + (ct * sU0[i] - st * sU1[i]);
          py = py + (st * sU0[i] + ct * sU1[i]);
          pth = atan2(cd * st + sd * ct, cd * ct - sd * st);
        }
        sGt[3 * i] = px; sGt[3 * i + 1] = py; sGt[3 * i + 2] = pth;
      }
    }
    __syncthreads();
    if (k < K) {
      const double gx = sGt[3 * t], gy = sGt[3 * t + 1], gth = sGt[3 * t + 2];
      const size_t row = (size_t)k * nF + b;
      BatchPropIn &I = A.prop[row];
      I.pinPose[0] = gx; I.pinPose[1] = gy; I.pinPose[2] = gth;
      A.gt[3 * row] = gx; A.gt[3 * row + 1] = gy; A.gt[3 * row + 2] = gth;
      A.tgt[4 * row] = (double)k * C.dt; A.tgt[4 * row + 1] = gx; A.tgt[4 * row + 2] = gy; A.tgt[4 * row + 3] = gth;
    }
    __syncthreads();      // (the next chunk writes the LDS arrays again; the rows written so far are visible to the whole workgroup)
  }
  // landmarks: the inverse measurement of a random (r, b) from the pose at step k_j (:249-284)
  if (t == 0) { sNLm = 0; sDetMax = 0; }
  for (int j = t; j < SENSOR_MAX_LANDMARKS; j += TRUTH_THREADS) sFirst[j] = INT_MAX;
  __syncthreads();
  const int lspacing = C.nLandmarks > 0 ? max(C.kFull / C.nLandmarks, 1) : 0;
  double *lm = A.lm + (size_t)b * (SENSOR_MAX_LANDMARKS * 2);
  for (int j = t; j < SENSOR_MAX_LANDMARKS; j += TRUTH_THREADS) {
    const long long kj = max((long long)lspacing * j, (long long)j + 1);
    if (C.nLandmarks > 0 && kj < K) {
      const double *g = A.gt + 3 * ((size_t)kj * nF + b);
      philox4x32_10((unsigned)j, TRUTH_BLOCK_LANDMARK, 0u, 0u, k0, k1, r);
      const double rr = sensor_u01(r[0], r[1]) * C.rmax, bb = sensor_u01(r[2], r[3]) * 2 * RFS_PI;
      const double x = g[0] + rr * cos(g[2] + bb), y = g[1] + rr * sin(g[2] + bb);
      sLm[2 * j] = x; sLm[2 * j + 1] = y;
      lm[2 * j] = x; lm[2 * j + 1] = y;
      atomicAdd(&sNLm, 1);      // (k_j rises with j: the placed landmarks are 0 ... count - 1)
    }
  }
  __syncthreads();
  const int L = min(sNLm, SENSOR_MAX_LANDMARKS);
  // first-seen steps and the most landmarks in range at any step k >= 1 (first_seen_times, sensor_max_nz)
  for (int k = 1 + t; k < K; k += TRUTH_THREADS) {
    const double *g = A.gt + 3 * ((size_t)k * nF + b);
    const double gx = g[0], gy = g[1];
    int cnt = 0;
    for (int j = 0; j < L; j++) {
      const double dx = sLm[2 * j] - gx, dy = sLm[2 * j + 1] - gy;
      const double range = sqrt(dx * dx + dy * dy);
      if (range >= C.rmin && range <= C.rmax) {
        cnt++;
        if (k < sFirst[j]) atomicMin(&sFirst[j], k);
      }
    }
    if (cnt > sDetMax) atomicMax(&sDetMax, cnt);
  }
  __syncthreads();
  double *seen = A.firstSeen + (size_t)b * SENSOR_MAX_LANDMARKS;
  for (int j = t; j < L; j += TRUTH_THREADS) seen[j] = sFirst[j] == INT_MAX ? -1.0 : (double)sFirst[j] * C.dt;
  if (t == 0) { A.counts[2 * b] = L; A.counts[2 * b + 1] = sDetMax; }
}
