// batch_loop.h -- the two pieces of RBPHDFilter's loop that kept the host inside every cycle of a filter batch, on the device:
// ParticleFilter::propagate with the 2-D odometry model (reference include/ParticleFilter.hpp:322-339,
// src/ProcessModel_Odometry2D.cpp:40-90) and the resampling tail of RBPHDFilter::update (include/RBPHDFilter.hpp:524-539) with
// ParticleFilter::resample (include/ParticleFilter.hpp:399-492), both for every filter of a batch in one launch.
//
// Why here: a batch cycle is one step kernel and one post kernel, but the host drew 3 n normal deviates per filter, waited for the
// weights, built the systematic plan in numpy and validated it in a loop -- one host <-> device round trip per cycle, nothing could
// be enqueued ahead (README, batch row).  The random numbers come from Philox4x32-10 (motion.h) keyed by each filter's seed with
// counters that name the slot WITHIN the filter, so a filter's draws do not depend on where it sits in the batch.
#pragma once
#include "common.h"
#include "motion.h"

struct BatchMotion {       // rfsgpu_batch_set_motion_odometry
  double sd[3];            // sqrt(var): the additive process noise on (x, y, theta)
  double var[3];           // the pose covariance every propagated particle gets: diag(var)
  unsigned long long seed; // the filter's Philox key
};
struct BatchPropIn {       // per filter and call, through the pinned ring
  double u[3];             // odometry input
  double pinPose[3];
  int pin, pad;
};
struct BatchResIn {        // per filter and call, through the pinned ring
  double effN, effNPercent;       // ParticleFilter::resample's two thresholds (rfsgpu_batch_set_resampling)
  int nZ;                         // this cycle's measurement count
  int minUpdates, minMeasurements;   // the gates of the filter's rfsgpu_filter_config
  int pad;
};
struct BatchLoopState {
  long long *counters;     // [nF][2] nUpdatesSinceResample_, nMeasurementsSinceResample_
  long long *nResamples;   // [nF]
  int *resampled;          // [nF] RBPHDFilter::resampleOccured_
  int *fired;              // [nF] the last call's decisions ...
  double *nEff;            // [nF] ... its N_eff values (0 where a filter stopped before the test) ...
  int *plan;               // [N]  ... and its plan in global slots (identity where not fired)
  int *pid, *ppid;         // [N]  Particle::id_ / idParent_ of the particle in each slot
};

// The resampling draw of (filter key, call): 53 bits of Philox block (0, 2, call lo, call hi) over 2^53 -- in [0, 1), never 1.
__host__ __device__ inline double batch_resample_draw(unsigned long long seed, unsigned long long call) {
  unsigned r[4];
  philox4x32_10(0u, 2u, (unsigned)(call & 0xffffffffull), (unsigned)(call >> 32), (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), r);
  const unsigned long long m = (((unsigned long long)r[0] << 32) | r[1]) >> 11;
  return (double)m * (1.0 / 9007199254740992.0);
}

// ParticleFilter::propagate for every particle of every filter: MotionModel_Odometry2d::step + N(0, diag(var_b)), the pose
// covariance diag(var_b); a pinned filter's particles take pinPose with a zero covariance.  One thread per global slot.  poseIn and
// poseOut may be the same array (a thread reads and writes its own slot only).
__global__ __launch_bounds__(256) void batch_propagate_kernel(const double *poseIn, double *poseOut, double *poseCov, const BatchMotion *mot,
                                                              const BatchPropIn *in, int N, int nPer, unsigned callLo, unsigned callHi) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const int b = k / nPer, i = k - b * nPer;
  const BatchPropIn I = in[b];
  const BatchMotion M = mot[b];
  double ox, oy, oth, v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (I.pin) {
    ox = I.pinPose[0]; oy = I.pinPose[1]; oth = I.pinPose[2];
  } else {
    const double x = poseIn[3 * (size_t)k], y = poseIn[3 * (size_t)k + 1], th = poseIn[3 * (size_t)k + 2];
    const double ct = cos(th), st = sin(th);
    ox = x + (ct * I.u[0] - st * I.u[1]);                  // p_k = p_km + C_km^T dp
    oy = y + (st * I.u[0] + ct * I.u[1]);
    const double cd = cos(I.u[2]), sd = sin(I.u[2]);
    oth = atan2(cd * st + sd * ct, cd * ct - sd * st);     // C_k = C_d C_km; theta_k = atan2(C_k(0,1), C_k(0,0))
    const unsigned k0 = (unsigned)(M.seed & 0xffffffffull), k1 = (unsigned)(M.seed >> 32);
    unsigned r[4];
    philox4x32_10((unsigned)i, 0u, callLo, callHi, k0, k1, r);
    double rad = sqrt(-2.0 * log(philox_u01(r[0], r[1]))), ang = 2.0 * RFS_PI * philox_u01(r[2], r[3]);
    ox += M.sd[0] * (rad * cos(ang));
    oy += M.sd[1] * (rad * sin(ang));
    philox4x32_10((unsigned)i, 1u, callLo, callHi, k0, k1, r);
    rad = sqrt(-2.0 * log(philox_u01(r[0], r[1]))); ang = 2.0 * RFS_PI * philox_u01(r[2], r[3]);
    oth += M.sd[2] * (rad * cos(ang));
    v0 = M.var[0]; v1 = M.var[1]; v2 = M.var[2];
  }
  poseOut[3 * (size_t)k] = ox; poseOut[3 * (size_t)k + 1] = oy; poseOut[3 * (size_t)k + 2] = oth;
  double *c = poseCov + 9 * (size_t)k;
  c[0] = v0; c[1] = 0.0; c[2] = 0.0; c[3] = 0.0; c[4] = v1; c[5] = 0.0; c[6] = 0.0; c[7] = 0.0; c[8] = v2;
}

// s + w * w with the product rounded before it is added.  (__dmul_rn and __dadd_rn are plain operators in this toolchain's headers:
// under the build's contraction mode the pair became one v_fmac_f64, and N_eff differed from the stated sum in its last bit.)
__device__ __forceinline__ double batch_add_square(double s, double w) {
#pragma clang fp contract(off)
  const double p = w * w;
  return s + p;
}

#define BATCH_LOOP_THREADS 256
#define BATCH_LOOP_MAX_PER_FILTER 2048     // == RFSGPU_BATCH_RESAMPLE_MAX_PER_FILTER (rfsgpu.h); the LDS arrays below

// Exclusive prefix sums of one int per thread over the workgroup (Hillis-Steele in LDS; 256 entries, 8 rounds).
__device__ __forceinline__ int batch_block_exscan(int v, int *sc) {
  const int t = threadIdx.x;
  sc[t] = v;
  __syncthreads();
  for (int d = 1; d < BATCH_LOOP_THREADS; d <<= 1) {
    const int a = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += a;
    __syncthreads();
  }
  const int incl = sc[t];
  __syncthreads();
  return incl - v;
}

// The tail of RBPHDFilter::update for every filter, one workgroup per filter: counters and gates, N_eff by the sequential sum in
// slot order, the reference's systematic plan (the two running sums by one lane, as the reference rounds them; the search of every
// sample point, the first-occurrence flags and the two compactions by all lanes), ids, weights, resampleOccured_.  The mixtures
// and poses move afterwards (resample_gather_kernel on S.plan: slots that keep themselves exit at once).
__global__ __launch_bounds__(BATCH_LOOP_THREADS) void batch_resample_kernel(double *weight, BatchLoopState S, const BatchMotion *mot, const BatchResIn *in,
                                                                            int nPer, unsigned long long call, const BatchFilter *filt) {
  __shared__ double cum[BATCH_LOOP_MAX_PER_FILTER];     // the weights, then their running sum
  __shared__ double sp[BATCH_LOOP_MAX_PER_FILTER];      // the sample points
  __shared__ int sidx[BATCH_LOOP_MAX_PER_FILTER];       // the particle each sample point falls on
  __shared__ int dupl[BATCH_LOOP_MAX_PER_FILTER];       // sources of the copies, in sampling order
  __shared__ int sampled[BATCH_LOOP_MAX_PER_FILTER];
  __shared__ int sc[BATCH_LOOP_THREADS];
  __shared__ int sFire;
  const int b = blockIdx.x, t = threadIdx.x, n = nPer, lo = b * nPer;
  if (n > BATCH_LOOP_MAX_PER_FILTER) return;            // (refused by the host)
  BatchResIn I = in[b];
  if (filt) I.nZ = filt[b].nZ;      // (rfsgpu_batch_resample_sensed_async: the count of the set the device drew; null: the host's)
  for (int j = t; j < n; j += BATCH_LOOP_THREADS) { cum[j] = weight[lo + j]; sampled[j] = 0; }
  __syncthreads();
  if (t == 0) {
    int fire = 0;
    double neff = 0.0;
    long long nu = S.counters[2 * b] + 1, nm = S.counters[2 * b + 1];      // every call counts as an update (:448)
    if (I.nZ > 0) {
      nm += I.nZ;
      if (nu >= I.minUpdates && nm >= I.minMeasurements) {
        double ss = 0.0;
        for (int j = 0; j < n; j++) ss = batch_add_square(ss, cum[j]);   // (no fused multiply-add: the reference's rounding)
        neff = 1.0 / ss;
        fire = !(neff > I.effN && neff / (double)n > I.effNPercent);
      }
    }
    if (fire) {
      const double interval = 1.0 / (double)n;
      double c = cum[0], p = interval * batch_resample_draw(mot[b].seed, call);
      sp[0] = p;
      for (int j = 1; j < n; j++) { c = __dadd_rn(c, cum[j]); cum[j] = c; p = __dadd_rn(p, interval); sp[j] = p; }
      nu = 0; nm = 0;
      S.nResamples[b] += 1;
      S.resampled[b] = 1;
    }
    S.counters[2 * b] = nu; S.counters[2 * b + 1] = nm;
    S.fired[b] = fire;
    S.nEff[b] = neff;
    sFire = fire;
  }
  __syncthreads();
  if (!sFire) {      // (workgroup-uniform)
    for (int j = t; j < n; j += BATCH_LOOP_THREADS) S.plan[lo + j] = lo + j;
    return;
  }
  // `while (sample_point > cumulative_weight && idx < n - 1) idx++`: with non-negative weights the running sum does not fall, so
  // the walk ends on the first j with cum[j] >= sp[i], or on n - 1
  for (int i = t; i < n; i += BATCH_LOOP_THREADS) {
    const double p = sp[i];
    int a = 0, e = n - 1;              // the answer lies in [a, e]
    while (a < e) {
      const int m = (a + e) >> 1;
      if (p > cum[m]) a = m + 1; else e = m;
    }
    sidx[i] = a;
    sampled[a] = 1;
  }
  __syncthreads();
  // a sampled particle stays in its slot; the copies (every further sample of a particle) take the un-sampled slots in ascending
  // order, in sampling order (:446-479).  Each thread owns a run of consecutive indices: ranks by an exclusive scan of the counts.
  const int ch = (n + BATCH_LOOP_THREADS - 1) / BATCH_LOOP_THREADS, e0 = t * ch, e1 = min(n, e0 + ch);
  int nd = 0, nf = 0;
  for (int i = e0; i < e1; i++) {
    nd += (i > 0 && sidx[i] == sidx[i - 1]) ? 1 : 0;
    nf += sampled[i] ? 0 : 1;
  }
  int rd = batch_block_exscan(nd, sc);
  int rf = batch_block_exscan(nf, sc);
  for (int i = e0; i < e1; i++)
    if (i > 0 && sidx[i] == sidx[i - 1]) dupl[rd++] = sidx[i];
  __syncthreads();
  for (int j = e0; j < e1; j++) {
    const int s = sampled[j] ? j : dupl[min(rf, n - 1)];
    if (!sampled[j]) rf++;
    S.plan[lo + j] = lo + s;
    // ids as ParticleFilter::resample leaves them: a copy has its source's id and idParent_ = that id; a kept particle
    // idParent_ = its own id.  Sources are never destinations: in place.
    if (s != j) { const int id = S.pid[lo + s]; S.pid[lo + j] = id; S.ppid[lo + j] = id; }
    else S.ppid[lo + j] = S.pid[lo + j];
    weight[lo + j] = 1.0;
  }
}

// The reference's lazy copy of the unused-measurement lists in the predict after a resampling (RBPHDFilter.hpp:1005-1011; birth.h),
// as rfsgpu_batch_cycle_async does it on the host: a slot copies from a HIGHER slot what that slot held before this predict, from
// a LOWER slot what that one holds after its own birth step -- nothing once the filter has had an update (nZprev > 0: its births
// consume the whole list), else what it inherited in turn (a serial walk, by one lane).  One workgroup per filter, with the
// particle ids and the resampleOccured_ flags where the device route left them.  The flag falls when this cycle updates the filter.
// prevCount (null: the host keeps it): the count of each filter's last update, which rfsgpu_batch_sense_async's records carry as nZprev.
__global__ __launch_bounds__(BATCH_LOOP_THREADS) void batch_inherit_dev_kernel(unsigned long long *mask, const int *ppid, int *resampled, const BatchFilter *filt,
                                                                               int nPer, int doInherit, int *prevCount) {
  __shared__ unsigned long long before[BATCH_LOOP_MAX_PER_FILTER];
  __shared__ int par[BATCH_LOOP_MAX_PER_FILTER];
  __shared__ int src[BATCH_LOOP_MAX_PER_FILTER];
  const int b = blockIdx.x, t = threadIdx.x, n = nPer, lo = b * nPer;
  if (n > BATCH_LOOP_MAX_PER_FILTER) return;
  const int r = resampled[b];
  const int nZ = filt[b].nZ, nZprev = filt[b].nZprev;
  if (r && doInherit) {
    for (int k = t; k < n; k += BATCH_LOOP_THREADS) {
      int p = ppid[lo + k] - lo;
      if (p < 0 || p >= n) p = k;
      par[k] = p;
      src[k] = p > k ? p : (p == k ? k : -1);
      before[k] = mask[lo + k];
    }
    __syncthreads();
    if (nZprev <= 0 && t == 0)
      for (int k = 0; k < n; k++) { const int p = par[k]; if (p < k) src[k] = src[p]; }
    __syncthreads();
    for (int k = t; k < n; k += BATCH_LOOP_THREADS) {
      const int s = src[k];
      if (s != k) mask[lo + k] = s < 0 ? 0ull : before[s];
    }
  }
  __syncthreads();
  if (t == 0 && nZ > 0 && r) resampled[b] = 0;
  if (t == 0 && nZ > 0 && prevCount) prevCount[b] = nZ;     // (a sensed cycle, batch_sensor.h: the next sense call's nZprev)
}
