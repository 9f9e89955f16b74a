// resample_plan.h -- ParticleFilter::resample(n, forceResample) (reference include/ParticleFilter.hpp:399-492) for an ordinary
// handle of any particle count, on the device (rfsgpu_resample_async):
//
//  resample_check_kernel   whether the weights can be resampled at all (none negative, all finite, a positive sum): the
//                          normalisation, the plan, the copies and the renormalisation behind it all leave when they cannot
//  resample_plan_kernel    the N_eff test and the systematic plan: fs_resample_shrink_body's contract (fastslam_cycle.h) without its
//                          limit of one filter per LDS -- the weights pass through LDS in chunks of RSP_CHUNK, the running sums,
//                          sample indices, flags and copy sources live in a scratch block in device memory
//
// Between them run weight_sums_kernel and normalize_kernel (merge_prune.h) and behind them resample_gather_kernel, each with a
// LiveCount (common.h) over words of the block: those are the launches of the host route, so the bits are the host route's.
#pragma once
#include "common.h"

enum ResampleWord {
  RSW_N = 0,        // the particle count the call was made at
  RSW_BAD,          // the weights cannot be resampled (a negative or non-finite weight, a sum that is not positive): nothing is touched
  RSW_FIRED,        // whether the call resampled
  RSW_GATHER_N,     // the count after a resampling that fired, else 0 (resample_gather_kernel's LiveCount)
  RSW_RENORM_N,     // the count when the test ran and did not fire and the caller asked for the second normalisation, else 0
  RSW_NO_RENORM,    // != 0: the second normalisation's two launches leave at once
  RSW_N_AFTER,      // the count after the call
  // rfsgpu_rbphd_cycle_async (birth_walk.h): what RBPHDFilter::update keeps between calls, and what the cycles report
  RCW_UPD,          // nUpdatesSinceResample_
  RCW_MEAS,         // nMeasurementsSinceResample_
  RCW_RESAMPLED,    // resampleOccured_
  RCW_GATE,         // the last cycle: both gates were open (0 for a cycle without measurements)
  RCW_BADNOW,       // the last cycle: resample_check_kernel's verdict (RSW_BAD also closes the plan kernel behind a closed gate)
  RCW_BADSEEN,      // a cycle since the last resolving call met weights that cannot be resampled
  RCW_NCYCLES,      // cycles so far | with an open gate | that resampled
  RCW_NGATE,
  RCW_NFIRED,
  RCW_WALK_MAX,     // the deepest level of the last inheritance walk made on the device
  RCW_MAXLEVEL,     // the deepest level of any walk so far
  RSW_WORDS = 24
};
// One allocation; the head up to the end of ppid is what the host takes back when it resolves the call.
// nEff | words | plan | pid | ppid || sidx | sampled | dupl | cum
struct ResampleState {
  double *nEff;     // [1] N_eff of the last call (0 where the test did not run)
  int *w;           // [RSW_WORDS]
  int *plan;        // [Ncap] the last plan (identity where the call did not fire)
  int *pid, *ppid;  // [Ncap] Particle::id_ / idParent_
  int *sidx;        // [Ncap] the particle each sample point falls on
  int *sampled;     // [Ncap]
  int *dupl;        // [Ncap] sources of the copies, in sampling order
  double *cum;      // [Ncap] running sum of the weights
};
__host__ __device__ inline size_t resample_state_head_bytes(int Ncap) { return 8 + (size_t)RSW_WORDS * 4 + (size_t)3 * Ncap * 4; }
__host__ __device__ inline size_t resample_state_bytes(int Ncap) { return ((resample_state_head_bytes(Ncap) + (size_t)3 * Ncap * 4 + 7) & ~(size_t)7) + (size_t)Ncap * 8; }
__host__ __device__ inline void resample_state_carve(unsigned char *base, int Ncap, ResampleState &S) {
  S.nEff = (double *)base;
  S.w = (int *)(base + 8);
  S.plan = S.w + RSW_WORDS;
  S.pid = S.plan + Ncap;
  S.ppid = S.pid + Ncap;
  S.sidx = S.ppid + Ncap;
  S.sampled = S.sidx + Ncap;
  S.dupl = S.sampled + Ncap;
  S.cum = (double *)(base + ((resample_state_head_bytes(Ncap) + (size_t)3 * Ncap * 4 + 7) & ~(size_t)7));
}

struct ResampleArg {
  double effN, effNPercent;   // ParticleFilter::resample's two thresholds
  double u01;                 // the caller's draw for the systematic plan
  int n;                      // the particle count
  int nOut;                   // samples to draw (1 ... n)
  int force;                  // forceResample: no N_eff test
  int renorm;                 // the caller wants the second normalisation of RBPHDFilter::update's else branch when the test does not fire
};

#define RSP_THREADS 1024
#define RSP_CHUNK 2048
#define RSP_PER (RSP_CHUNK / RSP_THREADS)     // consecutive slots a thread owns in a chunk's compaction

// sums[0] is weight_sums_kernel's sum of the same weights.  One workgroup.
__global__ __launch_bounds__(RSP_THREADS) void resample_check_kernel(const double *weight, int n, const double *sums, ResampleState S) {
  int bad = 0;
  for (int j = threadIdx.x; j < n; j += RSP_THREADS) {
    const double v = weight[j];
    bad |= !(v >= 0.0 && v <= 1.79769313486231570815e308) ? 1 : 0;      // (a NaN fails both comparisons)
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    const double s = sums[0];
    S.w[RSW_N] = n;
    S.w[RSW_BAD] = (bad || !(s > 0.0 && s <= 1.79769313486231570815e308)) ? 1 : 0;
  }
}

// Exclusive prefix sums of one int per thread over the workgroup, and their total (fs_cycle_exscan for RSP_THREADS threads).
// sw: RSP_THREADS / 64 ints.
__device__ __forceinline__ int rsp_exscan(int v, int *sw, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_up(incl, d, 64);
    if (lane >= d) incl += a;
  }
  __syncthreads();                      // (the previous scan's readers are done with sw)
  if (lane == 63) sw[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < RSP_THREADS / 64; k++) {
    const int s = sw[k];
    before += k < wave ? s : 0;
    all += s;
  }
  total = all;
  return before + incl - v;
}

// The weights are normalised (the launches before this one).  One workgroup.  Lane 0 carries N_eff's sum, the running sum of the
// weights and the sample points across the chunks, each a chain in the reference's order.  The running sum and the sample points are
// plain additions in the reference's rounding; N_eff's sum is NOT: the compiler contracts __dadd_rn(ss, __dmul_rn(v, v)) into one
// fused multiply-add per particle (v_fmac_f64 in the code object), so it carries one rounding per particle where the reference
// rounds the square first -- N_eff agrees with the reference's to rounding, not bit for bit; every lane searches sample points, and the two compactions -- the copies in sampling order, the un-sampled slots
// ascending -- are scans over chunks of RSP_CHUNK slots whose totals carry into the next chunk.  The plan for nOut samples out of n
// (cases 1-4 of ParticleFilter.hpp:459-478) is fs_resample_shrink_body's: a sampled slot below nOut keeps its particle; every other
// sample -- a repeat, or a first sample of a slot at or beyond nOut -- is copied, in sampling order, into the un-sampled slots in
// ascending order, all of which lie below nOut.
__global__ __launch_bounds__(RSP_THREADS) void resample_plan_kernel(double *weight, ResampleState S, ResampleArg A) {
  __shared__ double buf[RSP_CHUNK];        // a chunk of weights (zeros behind the last one); a chunk of sample points
  __shared__ double run[RSP_CHUNK];        // a chunk of running sums
  __shared__ int sIdx[RSP_CHUNK + 1];      // a chunk of sample indices behind the last one of the chunk before
  __shared__ int sw[RSP_THREADS / 64];
  __shared__ int sFire;
  const int t = threadIdx.x;
  const int n = A.n, nOut = A.nOut;
  if (S.w[RSW_BAD] != 0) {                 // (workgroup-uniform) the state stays as it is; the host reports it
    for (int j = t; j < n; j += RSP_THREADS) S.plan[j] = j;
    if (t == 0) {
      S.nEff[0] = 0.0;
      S.w[RSW_FIRED] = 0; S.w[RSW_GATHER_N] = 0; S.w[RSW_RENORM_N] = 0; S.w[RSW_NO_RENORM] = 1; S.w[RSW_N_AFTER] = n;
    }
    return;
  }
  // (the running sum starts from 0: 0 + w_0 is w_0, the weights are not negative; lane 0 takes eight weights at a time so that
  //  their loads do not wait for the sums' stores; the zeros behind the last weight of a chunk leave both sums as they are)
  double ss = 0.0, c = 0.0;                // lane 0's
  for (int base = 0; base < n; base += RSP_CHUNK) {
    const int m = min(RSP_CHUNK, n - base), m8 = (m + 7) & ~7;
    for (int j = t; j < m8; j += RSP_THREADS) {
      buf[j] = j < m ? weight[base + j] : 0.0;
      if (j < m) S.sampled[base + j] = 0;
    }
    __syncthreads();
    if (t == 0) {
      for (int j = 0; j < m8; j += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = buf[j + q];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          ss = __dadd_rn(ss, __dmul_rn(v[q], v[q]));
          c = __dadd_rn(c, v[q]);
          run[j + q] = c;
        }
      }
    }
    __syncthreads();
    for (int j = t; j < m; j += RSP_THREADS) S.cum[base + j] = run[j];
  }
  if (t == 0) {
    double neff = 0.0;
    int fire = 1;
    if (!A.force) {
      neff = 1.0 / ss;
      fire = !(neff > A.effN && neff / (double)n > A.effNPercent);
    }
    const int renorm = (!fire && A.renorm) ? 1 : 0;
    S.nEff[0] = neff;
    S.w[RSW_FIRED] = fire;
    S.w[RSW_GATHER_N] = fire ? nOut : 0;
    S.w[RSW_RENORM_N] = renorm ? n : 0;
    S.w[RSW_NO_RENORM] = renorm ? 0 : 1;
    S.w[RSW_N_AFTER] = fire ? nOut : n;
    sFire = fire;
  }
  __syncthreads();
  if (!sFire) {                            // (workgroup-uniform)
    for (int j = t; j < n; j += RSP_THREADS) S.plan[j] = j;
    return;
  }
  // `while (sample_point > cumulative_weight) idx++` (bounded by the last particle): the running sum does not fall, so the walk
  // ends on the first j with cum[j] >= the sample point, or on n - 1
  const double interval = 1.0 / (double)nOut;
  double p = 0.0;                          // lane 0's
  for (int base = 0; base < nOut; base += RSP_CHUNK) {
    const int m = min(RSP_CHUNK, nOut - base);
    if (t == 0) {
      for (int j = 0; j < m; j++) {
        p = (base + j == 0) ? __dmul_rn(interval, A.u01) : __dadd_rn(p, interval);
        buf[j] = p;
      }
    }
    __syncthreads();
    for (int j = t; j < m; j += RSP_THREADS) {
      const double q = buf[j];
      int a = 0, e = n - 1;
      while (a < e) {
        const int mid = (a + e) >> 1;
        if (q > S.cum[mid]) a = mid + 1; else e = mid;
      }
      S.sidx[base + j] = a;
      S.sampled[a] = 1;
    }
    __syncthreads();
  }
  // the sources of the copies, in sampling order
  int carry = 0;
  for (int base = 0; base < nOut; base += RSP_CHUNK) {
    const int m = min(RSP_CHUNK, nOut - base);
    for (int j = t; j < m; j += RSP_THREADS) sIdx[j + 1] = S.sidx[base + j];
    if (t == 0) sIdx[0] = base > 0 ? S.sidx[base - 1] : -1;
    __syncthreads();
    const int e0 = min(m, t * RSP_PER), e1 = min(m, e0 + RSP_PER);
    int nd = 0;
    for (int j = e0; j < e1; j++) {
      const bool keep = sIdx[j + 1] < nOut && sIdx[j + 1] != sIdx[j];      // case 1
      nd += keep ? 0 : 1;
    }
    int tot;
    int rd = carry + rsp_exscan(nd, sw, tot);
    for (int j = e0; j < e1; j++) {
      const bool keep = sIdx[j + 1] < nOut && sIdx[j + 1] != sIdx[j];
      if (!keep) S.dupl[rd++] = sIdx[j + 1];
    }
    carry += tot;
    __syncthreads();                       // (sIdx is free for the next chunk; the copies' sources are out)
  }
  // the un-sampled slots take them in ascending order
  carry = 0;
  for (int base = 0; base < nOut; base += RSP_CHUNK) {
    const int m = min(RSP_CHUNK, nOut - base);
    const int e0 = min(m, t * RSP_PER), e1 = min(m, e0 + RSP_PER);
    int nf = 0;
    for (int j = e0; j < e1; j++) nf += S.sampled[base + j] ? 0 : 1;
    int tot;
    int rf = carry + rsp_exscan(nf, sw, tot);
    for (int j = e0; j < e1; j++) {
      const int k = base + j;
      const bool kept = S.sampled[k] != 0;
      const int s = kept ? k : S.dupl[min(rf, nOut - 1)];
      if (!kept) rf++;
      S.plan[k] = s;
      // ids as ParticleFilter::resample leaves them (:446-479): a copy has its source's id and idParent_ = that id; a kept particle
      // idParent_ = its own id.  Sources are sampled slots, destinations un-sampled ones: in place.
      if (s != k) { const int id = S.pid[s]; S.pid[k] = id; S.ppid[k] = id; }
      else S.ppid[k] = S.pid[k];
      weight[k] = 1.0;
    }
    carry += tot;
  }
}
