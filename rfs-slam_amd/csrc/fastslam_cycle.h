// fastslam_cycle.h -- the two host stops of a multi-hypothesis FastSLAM cycle, on the device (rfsgpu_fastslam_cycle_async):
//
//  fs_mh_plan_kernel           the slots of the particle copies (reference include/FastSLAM.hpp:543-556; the host loop of
//                              fastslam_update_mh): an exclusive scan of max(nH - 1, 0) in place of the running particle count
//  fs_resample_shrink_kernel   FastSLAM::resampleWithMapCopy (:729-757) with ParticleFilter::resample(n, force)
//                              (include/ParticleFilter.hpp:399-492) for n <= the grown count: batch_resample_kernel's method
//                              (batch_loop.h) for one filter whose input count is on the device
//
// Between the two the particle count is known to the device only: the kernels of the update (fastslam_mh.h, gm_prune_kernel,
// fs_new_landmarks_kernel, the weight sum and the normalisation) are launched at the handle's capacity with a LiveCount (common.h).
// These are latency-bound bookkeeping kernels of one workgroup; what they buy is the two host <-> device round trips they replace.
#pragma once
#include "fastslam_mh.h"
#include "batch_loop.h"

enum FsCycleWord {
  FSC_N = 0,        // the live particle count
  FSC_OVF,          // the grown set would exceed max_particles: every later kernel leaves at once, the host reports and clears it
  FSC_NCOPY,        // copies of the last update (the copy kernel's LiveCount)
  FSC_RESAMPLED,    // FastSLAM::resampleOccured_
  FSC_RENORM_N,     // the count again when resample() returned false after normalising (a second normalisation follows, :743), else 0
  FSC_NGROWN,       // the count after the last update, before its resampling
  FSC_FIRED,        // whether the last cycle resampled
  FSC_DONE,         // cycles with measurements completed so far (the host undoes the slab flips of abandoned ones)
  FSC_NFIRED,       // ... and how many of them resampled (a host that reads nothing between cycles still learns the number)
  FSC_WORDS = 16
};
// One allocation, which a stream-ordered copy takes whole into pinned memory when the host next synchronises: that is how the
// particle count comes back.  {nEff, counters} | words | slotSrc | plan | pid | ppid
struct FsCycleState {
  double *nEff;            // [1] N_eff of the last cycle (0 where the test did not run)
  long long *counters;     // [2] nUpdatesSinceResample_, nMeasurementsSinceResample_
  int *w;                  // [FSC_WORDS]
  int *slotSrc;            // [Ncap] parent slot of every slot after the last update
  int *plan;               // [Ncap] the last resampling plan (identity where it did not fire)
  int *pid, *ppid;         // [Ncap] Particle::id_ / idParent_
};
__host__ __device__ inline size_t fs_cycle_state_bytes(int Ncap) { return 24 + (size_t)FSC_WORDS * 4 + (size_t)4 * Ncap * 4; }
__host__ __device__ inline void fs_cycle_carve(unsigned char *base, int Ncap, FsCycleState &S) {
  S.nEff = (double *)base;
  S.counters = (long long *)(base + 8);
  S.w = (int *)(base + 24);
  S.slotSrc = S.w + FSC_WORDS;
  S.plan = S.slotSrc + Ncap;
  S.pid = S.plan + Ncap;
  S.ppid = S.pid + Ncap;
}
// (LiveCopy, the copy kernel's LiveCount: fastslam_mh.h)

#define FS_CYCLE_THREADS 256
#define FS_CYCLE_MAX_PARTICLES BATCH_LOOP_MAX_PER_FILTER     // == RFSGPU_FASTSLAM_CYCLE_MAX_PARTICLES (rfsgpu.h)

// Exclusive prefix sums of one int per thread over the workgroup, and their total: a shuffle scan inside each wavefront, the four
// wave totals through LDS.  sw: FS_CYCLE_THREADS / 64 + 1 ints.
__device__ __forceinline__ int fs_cycle_exscan(int v, int *sw, int &total) {
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
  for (int k = 0; k < FS_CYCLE_THREADS / 64; k++) {
    const int s = sw[k];
    before += k < wave ? s : 0;
    all += s;
  }
  total = all;
  return before + incl - v;
}

// FastSLAM::predict's map part (:376-383) for a handle whose count is on the device: Sigma += Q on every landmark, no births.
__global__ __launch_bounds__(256) void fs_cycle_static_step_kernel(Buffers B, Params P, int cur, LiveCount live) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (live_beyond(live, i)) return;
  predict_map_particle<64>(B, P, cur, i, lane, false, 0, B.pose, true);
}

// ... for the Victoria Park model's 3-D landmarks (rfsgpu_fastslam_cycle_full_async): predict_map_general_kernel<3>'s static step
__global__ __launch_bounds__(256) void fs_cycle_static_step3_kernel(Buffers B, Params P, int cur, LiveCount live) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (live_beyond(live, i)) return;
  const int cap = B.cap, n = B.count[i];
  double *slab = B.slab[cur];
  for (int t = 0; t < 6; t++) {
    double *p = plane3(slab, cap, i, P3_SXX + t);
    for (int m = lane; m < n; m += 64) p[m] += P.Qlm6[t];
  }
}

// The plan of an update with one hypothesis (rfsgpu_fastslam_cycle_full_async, maxNDataAssocHypotheses == 1: the single-hypothesis
// association of fastslam.h makes no copies): every slot is its own parent and the count stays.
__global__ __launch_bounds__(FS_CYCLE_THREADS) void fs_cycle_identity_plan_kernel(FsCycleState S, int Ncap) {
  if (S.w[FSC_OVF] != 0) return;
  const int n = min(S.w[FSC_N], Ncap);
  for (int j = threadIdx.x; j < n; j += FS_CYCLE_THREADS) S.slotSrc[j] = j;
  if (threadIdx.x == 0) { S.w[FSC_NCOPY] = 0; S.w[FSC_NGROWN] = n; }
}

// The head of a cycle.  nHost / flagHost: the particle count and resampleOccured_ where the host still knows them (no cycle is
// pending), else -1: the device words hold them.  tick: an update without measurements (:399-402), only nUpdatesSinceResample_ moves.
__global__ void fs_cycle_begin_kernel(FsCycleState S, int nHost, int flagHost, int tick) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (nHost >= 0) S.w[FSC_N] = nHost;
  if (flagHost >= 0) S.w[FSC_RESAMPLED] = flagHost;
  if (tick && S.w[FSC_OVF] == 0) S.counters[0] += 1;
}

// The slots of the copies.  Particle i (nH_i hypotheses, arena header word 2) keeps hypothesis 0 in its own slot; its copies take
// [first_i, first_i + nH_i - 1) with first_i = N0 + sum_{j < i} max(nH_j - 1, 0), hypothesis h in first_i + (nH_i - 1) - h -- the
// reference appends a copy per hypothesis and then addresses them as nParticles_ - h.  copyDst / copySrc list the copies in the
// order the reference makes them.  One workgroup; a thread owns a run of consecutive particles.
// (the body: fs_mh_plan_kernel for a handle, fs_mh_plan_batch_kernel for one filter of a batch, whose pointers start at its block)
__device__ __forceinline__ void fs_mh_plan_body(const unsigned char *arena, const FsCycleState &S, int *slotHyp, int *slotNH, int *copyDst, int *copySrc, int Ncap) {
  __shared__ int sw[FS_CYCLE_THREADS / 64 + 1];
  const int t = threadIdx.x;
  if (S.w[FSC_OVF] != 0) return;                                     // (workgroup-uniform: an earlier cycle overflowed)
  const int N0 = S.w[FSC_N];
  if (N0 > Ncap || N0 > FS_CYCLE_MAX_PARTICLES) return;              // (cannot happen: refused by the host)
  const FsMhLayout L = fs_mh_layout();
  const int ch = (N0 + FS_CYCLE_THREADS - 1) / FS_CYCLE_THREADS, e0 = min(N0, t * ch), e1 = min(N0, e0 + ch);
  int extra = 0;
  for (int i = e0; i < e1; i++) {
    const int nH = min(((const int *)(arena + (size_t)i * L.total + L.offHdr))[2], FSMH_MAX_HYP);
    extra += nH > 1 ? nH - 1 : 0;
  }
  int total;
  int first = fs_cycle_exscan(extra, sw, total);
  const int n = N0 + total;
  if (n > Ncap) {                                                    // refused: nothing but the flag is written
    if (t == 0) S.w[FSC_OVF] = 1;
    return;
  }
  for (int i = e0; i < e1; i++) {
    const int nH = min(((const int *)(arena + (size_t)i * L.total + L.offHdr))[2], FSMH_MAX_HYP);
    S.slotSrc[i] = i; slotHyp[i] = nH > 0 ? 0 : -1; slotNH[i] = nH;
    for (int h = 1; h < nH; h++) {
      const int slot = N0 + first + (nH - 1) - h;
      S.slotSrc[slot] = i; slotHyp[slot] = h; slotNH[slot] = nH;
      copyDst[first + h - 1] = slot; copySrc[first + h - 1] = i;
    }
    first += nH > 1 ? nH - 1 : 0;
  }
  if (t == 0) {
    S.w[FSC_N] = n; S.w[FSC_NCOPY] = total; S.w[FSC_NGROWN] = n;
  }
}
__global__ __launch_bounds__(FS_CYCLE_THREADS) void fs_mh_plan_kernel(const unsigned char *arena, FsCycleState S, int *slotHyp, int *slotNH, int *copyDst,
                                                                      int *copySrc, int Ncap) {
  fs_mh_plan_body(arena, S, slotHyp, slotNH, copyDst, copySrc, Ncap);
}

struct FsShrinkArg {
  double effN, effNPercent;   // ParticleFilter::resample's two thresholds
  double u01;                 // the caller's draw for the systematic plan
  int nInit;                  // the count a resampling brings the set back to (0 or more than the count: the count stays)
  int nMax;                   // config.nParticlesMax_: above it the resampling is forced
  int nZ;
  int minUpdates, minMeasurements;
};

// resampleWithMapCopy for the particle set the update left (its count is S.w[FSC_N] <= FS_CYCLE_MAX_PARTICLES), whose weights the
// launches before this one have normalised (ParticleFilter::resample's first statement; where the gates keep resample() from
// running it is the normalisation of :743).  One workgroup: the gates, counters, N_eff and the two running sums by one lane in the
// reference's order and rounding, the search of every sample point, the flags and the two compactions by all lanes.  The plan for
// n samples out of the count (cases 1-4 of ParticleFilter.hpp:459-478): a sampled slot below n keeps its particle; every other
// sample -- a repeat, or a first sample of a slot at or beyond n -- is copied, in sampling order, into the un-sampled slots in
// ascending order, all of which lie below n.  The mixtures and poses move afterwards (resample_gather_kernel on S.plan).
__device__ __forceinline__ void fs_resample_shrink_body(double *weight, const FsCycleState &S, const FsShrinkArg &A) {
  __shared__ double cum[FS_CYCLE_MAX_PARTICLES];     // the weights, then their running sum
  __shared__ double sp[FS_CYCLE_MAX_PARTICLES];      // the sample points
  __shared__ int sidx[FS_CYCLE_MAX_PARTICLES];       // the particle each sample point falls on
  __shared__ int dupl[FS_CYCLE_MAX_PARTICLES];       // sources of the copies, in sampling order
  __shared__ int sampled[FS_CYCLE_MAX_PARTICLES];
  __shared__ int sw[FS_CYCLE_THREADS / 64 + 1];
  __shared__ int sFire, sOut;
  const int t = threadIdx.x;
  if (S.w[FSC_OVF] != 0) return;                        // (workgroup-uniform)
  const int n = S.w[FSC_N];
  if (n < 1 || n > FS_CYCLE_MAX_PARTICLES) return;      // (cannot happen: max_particles is refused beyond it)
  for (int j = t; j < n; j += FS_CYCLE_THREADS) { cum[j] = weight[j]; sampled[j] = 0; }
  __syncthreads();
  if (t == 0) {
    int fire = 0, renorm = 0, nOut = n;
    double neff = 0.0;
    long long nu = S.counters[0] + 1, nm = S.counters[1] + A.nZ;
    if (n > A.nMax) {
      fire = 1;                                         // :732-733 resample(nParticles_init_, true)
    } else if (nu >= (long long)A.minUpdates && nm >= (long long)A.minMeasurements) {
      double ss = 0.0;
      for (int j = 0; j < n; j++) ss = __dadd_rn(ss, __dmul_rn(cum[j], cum[j]));   // (no fused multiply-add: the reference's rounding)
      neff = 1.0 / ss;
      fire = !(neff > A.effN && neff / (double)n > A.effNPercent);
      renorm = !fire;
    }
    if (fire) {
      if (A.nInit > 0 && A.nInit < n) nOut = A.nInit;   // ParticleFilter.hpp:417-418
      const double interval = 1.0 / (double)nOut;
      double c = cum[0], p = interval * A.u01;
      sp[0] = p;
      for (int j = 1; j < n; j++) { c = __dadd_rn(c, cum[j]); cum[j] = c; }
      for (int j = 1; j < nOut; j++) { p = __dadd_rn(p, interval); sp[j] = p; }
      nu = 0; nm = 0;
    }
    S.counters[0] = nu; S.counters[1] = nm;
    S.nEff[0] = neff;
    S.w[FSC_FIRED] = fire;
    S.w[FSC_RESAMPLED] = fire;
    S.w[FSC_RENORM_N] = renorm ? n : 0;
    S.w[FSC_N] = nOut;
    S.w[FSC_DONE] += 1;
    S.w[FSC_NFIRED] += fire;
    sFire = fire; sOut = nOut;
  }
  __syncthreads();
  if (!sFire) {      // (workgroup-uniform)
    for (int j = t; j < n; j += FS_CYCLE_THREADS) S.plan[j] = j;
    return;
  }
  const int nOut = sOut;
  // `while (sample_point > cumulative_weight) idx++` (bounded by the last particle): the running sum does not fall, so the walk
  // ends on the first j with cum[j] >= sp[i], or on n - 1
  for (int i = t; i < nOut; i += FS_CYCLE_THREADS) {
    const double p = sp[i];
    int a = 0, e = n - 1;
    while (a < e) {
      const int m = (a + e) >> 1;
      if (p > cum[m]) a = m + 1; else e = m;
    }
    sidx[i] = a;
    sampled[a] = 1;
  }
  __syncthreads();
  const int ch = (nOut + FS_CYCLE_THREADS - 1) / FS_CYCLE_THREADS, e0 = min(nOut, t * ch), e1 = min(nOut, e0 + ch);
  int nd = 0, nf = 0;
  for (int i = e0; i < e1; i++) {
    const bool keep = sidx[i] < nOut && !(i > 0 && sidx[i] == sidx[i - 1]);   // case 1
    nd += keep ? 0 : 1;
    nf += sampled[i] ? 0 : 1;
  }
  int tot;
  int rd = fs_cycle_exscan(nd, sw, tot);
  int rf = fs_cycle_exscan(nf, sw, tot);
  for (int i = e0; i < e1; i++) {
    const bool keep = sidx[i] < nOut && !(i > 0 && sidx[i] == sidx[i - 1]);
    if (!keep) dupl[rd++] = sidx[i];
  }
  __syncthreads();
  for (int j = e0; j < e1; j++) {
    const int s = sampled[j] ? j : dupl[min(rf, nOut - 1)];
    if (!sampled[j]) rf++;
    S.plan[j] = s;
    // ids as ParticleFilter::resample leaves them: a copy has its source's id and idParent_ = that id; a kept particle
    // idParent_ = its own id.  Sources are sampled slots, destinations un-sampled ones: in place.
    if (s != j) { const int id = S.pid[s]; S.pid[j] = id; S.ppid[j] = id; }
    else S.ppid[j] = S.pid[j];
    weight[j] = 1.0;
  }
}
__global__ __launch_bounds__(FS_CYCLE_THREADS) void fs_resample_shrink_kernel(double *weight, FsCycleState S, FsShrinkArg A) {
  fs_resample_shrink_body(weight, S, A);
}

// ---- a batch of multi-hypothesis FastSLAM filters (rfsgpu_batch_fastslam_mh_cycle_async; MhBatchArg, fastslam.h) -------------------
// One allocation holds every filter's cycle state as arrays over the filters and over the slots of the batch:
// nEff [nF] | counters [nF][2] | words [nF][FSC_WORDS] | slotSrc | plan | pid | ppid, [nF * stride] each.  Filter b's FsCycleState
// is the view that starts at its entries, so the count, the overflow word, the counters, N_eff, the plans and the ids are per
// filter, and the two one-workgroup kernels above run with one workgroup per filter on pointers that start at the filter's block:
// every slot number they write is local to it.
static_assert(FSC_OVF == MHB_OVF_WORD, "MhBatchArg reads the overflow word by this index");
__host__ __device__ inline size_t mhb_state_bytes(int nF, int stride) { return (size_t)nF * (24 + (size_t)FSC_WORDS * 4) + (size_t)4 * nF * stride * 4; }
__host__ __device__ inline void mhb_state(unsigned char *base, int nF, int stride, int b, FsCycleState &S) {
  S.nEff = (double *)base + b;
  S.counters = (long long *)(base + (size_t)8 * nF) + 2 * b;
  int *w0 = (int *)(base + (size_t)24 * nF);
  S.w = w0 + (size_t)FSC_WORDS * b;
  const size_t n = (size_t)nF * stride;
  S.slotSrc = w0 + (size_t)FSC_WORDS * nF + (size_t)b * stride;
  S.plan = S.slotSrc + n;
  S.pid = S.plan + n;
  S.ppid = S.pid + n;
}
// The head of a cycle: a filter without measurements only counts the update (:399-402).
__global__ void fs_cycle_begin_batch_kernel(unsigned char *state, MhBatchArg A, int nF) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nF) return;
  FsCycleState S;
  mhb_state(state, A.nF, A.nPer, b, S);
  if (A.filt[b].nZ == 0 && S.w[FSC_OVF] == 0) S.counters[0] += 1;
}
// FastSLAM::predict's map part for every live slot, also of a filter whose scan is empty.  Four waves of a workgroup may belong to
// four filters: no workgroup barrier.
__global__ __launch_bounds__(256) void fs_cycle_static_step_batch_kernel(Buffers B, int cur, MhBatchArg A) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (i >= B.N) return;
  const int bf = __builtin_amdgcn_readfirstlane(i / A.nPer);
  if (mhb_ovf(A, bf) || mhb_beyond_count(A, i)) return;
  predict_map_particle<64>(B, A.params[bf], cur, i, lane, false, 0, B.pose, true);
}
// ... of a batch of Victoria Park filters: fs_cycle_static_step3_kernel's additions with the slot's own filter's Q
__global__ __launch_bounds__(256) void fs_cycle_static_step3_batch_kernel(Buffers B, int cur, MhBatchArg A) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (i >= B.N) return;
  const int bf = __builtin_amdgcn_readfirstlane(i / A.nPer);
  if (mhb_ovf(A, bf) || mhb_beyond_count(A, i)) return;
  const Params &P = A.params[bf];
  const int cap = B.cap, n = B.count[i];
  double *slab = B.slab[cur];
  for (int t = 0; t < 6; t++) {
    double *p = plane3(slab, cap, i, P3_SXX + t);
    for (int m = lane; m < n; m += 64) p[m] += P.Qlm6[t];
  }
}
__global__ __launch_bounds__(FS_CYCLE_THREADS) void fs_mh_plan_batch_kernel(const unsigned char *arena, unsigned char *state, int *slotHyp, int *slotNH, int *copyDst,
                                                                            int *copySrc, MhBatchArg A) {
  const int b = blockIdx.x, base = b * A.nPer;
  if (A.filt[b].nZ == 0) return;                                     // (workgroup-uniform)
  FsCycleState S;
  mhb_state(state, A.nF, A.nPer, b, S);
  fs_mh_plan_body(arena + (size_t)base * fs_mh_layout().total, S, slotHyp + base, slotNH + base, copyDst + base, copySrc + base, A.nPer);
}
// {sum w, sum w^2} of every filter's live weights in weight_sums_kernel's order (thread t adds the slots t, t + 1024, ... of the
// filter; a wave reduction; the 16 wave sums in order), so a filter's sum has the bits its own handle's has.  A.word names the count.
__global__ __launch_bounds__(1024) void mhb_weight_sums_kernel(const double *w, double *sums, MhBatchArg A) {
  __shared__ double s0[16], s1[16];
  const int b = blockIdx.x;
  if (live_beyond(A, b * A.nPer)) return;                            // (workgroup-uniform: overflowed, no measurements, or a count of 0)
  const int N = __builtin_amdgcn_readfirstlane(A.words[(size_t)b * A.wordStride + A.word]);
  w += (size_t)b * A.nPer;
  double a = 0, c = 0;
  for (int k = threadIdx.x; k < N; k += 1024) { double v = w[k]; a += v; c += v * v; }
  a = wave_sum(a); c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) { s0[threadIdx.x >> 6] = a; s1[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double x = 0, y = 0;
    for (int k = 0; k < 16; k++) { x += s0[k]; y += s1[k]; }
    sums[2 * b] = x; sums[2 * b + 1] = y;
  }
}
__global__ void mhb_normalize_kernel(double *w, int nSlots, const double *sums, MhBatchArg A) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nSlots || live_beyond_lane(A, k)) return;
  w[k] = w[k] / sums[2 * (k / A.nPer)];
}
__global__ __launch_bounds__(FS_CYCLE_THREADS) void fs_resample_shrink_batch_kernel(double *weight, unsigned char *state, MhBatchArg A) {
  const int b = blockIdx.x;
  const MhBatchFilter &T = A.filt[b];
  if (T.nZ == 0) return;                                             // (workgroup-uniform)
  FsCycleState S;
  mhb_state(state, A.nF, A.nPer, b, S);
  FsShrinkArg R;
  R.effN = T.effN; R.effNPercent = T.effNPercent; R.u01 = T.u01;
  R.nInit = T.nInit; R.nMax = T.nMax; R.nZ = T.nZ;
  R.minUpdates = T.minUpdates; R.minMeasurements = T.minMeasurements;
  fs_resample_shrink_body(weight + (size_t)b * A.nPer, S, R);
}
