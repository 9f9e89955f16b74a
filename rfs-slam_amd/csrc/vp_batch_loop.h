// vp_batch_loop.h -- the device route of a batch of Victoria Park RB-PHD filters (rfsgpu_batch_vp_propagate_run_async,
// rfsgpu_batch_vp_resample_async and the birth predict of rfsgpu_batch_vp_cycle_async behind them): what kept the host inside every
// message of such a batch's run, on the device.
//
//  vp_batch_propagate_run_kernel
//        ParticleFilter::propagate with MotionModel_Ackerman2d::step (motion.h) for a run of consecutive odometry messages and every
//        filter of the batch: the run's inputs are the dataset's, shared by all filters; the input noise and the Philox key are the
//        filter's, and the counter names the slot WITHIN the filter, so a filter draws what its own handle draws under
//        rfsgpu_propagate_ackerman_run_async, wherever it sits in the batch.
//  vp_batch_walk_levels_kernel
//        birth_walk_levels_kernel (birth_walk.h) across the batch: the parent and level tables batch_vp_cycle_core builds on the host
//        from ppid and bResampled, from the ids and flags the device holds (batch_loop.h, BatchLoopState).
//  vp_batch_walk_tail_kernel
//        birth_walk_tail_kernel per filter: the levels beyond the RFSGPU_RBPHD_WALK_LEVELS that get launches of their own, one
//        workgroup per filter, with the filter's Params, previous set and count from the BatchArg tables.
//  vp_batch_clear_flags_kernel
//        resampleOccured_ of the filters this cycle updates (batch_inherit_dev_kernel does it for a 2-D batch).
//
// The resampling tail itself is batch_resample_kernel + resample_gather_kernel (batch_loop.h, resample_plan.h): model-agnostic.
#pragma once
#include "common.h"
#include "motion.h"
#include "birth.h"
#include "birth_walk.h"
#include "vp_batch.h"

struct VpBatchMotion {      // rfsgpu_batch_vp_set_motion
  double sv, sr;            // sqrt(var): the input noise on (speed, steering)
  double h, l, dx, dy;      // MotionModel_Ackerman2d::setAckermanParams
  unsigned long long seed;  // the filter's Philox key (the same word BatchMotion::seed carries for the resampling draw)
};
struct VpBatchRun {         // one call's run of odometry messages, through the pinned ring
  int n, pad;
  unsigned long long call0;
  double uv[ACKERMAN_RUN_MAX], ur[ACKERMAN_RUN_MAX], dt[ACKERMAN_RUN_MAX];
  int noisy[ACKERMAN_RUN_MAX];      // 0: the step carries no input noise and makes no draw (the driver's stationary predicts)
};

// One thread per global slot; every slot takes the run's steps one after the other, in place.  The filter's block of the pose array
// is handed to ackerman_step_particle with the slot's index INSIDE the block: the counter of its draw and the address of its pose
// are then what a handle of nPer particles has for particle i.
__device__ __forceinline__ void vp_batch_propagate_run_slot(double *pose, int k, int nPer, const VpBatchMotion *mot, const VpBatchRun *run) {
  const int b = k / nPer, i = k - b * nPer;
  const VpBatchMotion M = mot[b];
  double *blk = pose + 3 * (size_t)b * nPer;
  const int n = min(run->n, ACKERMAN_RUN_MAX);
  const unsigned long long call0 = run->call0;
  for (int r = 0; r < n; r++) {
    AckermanStep A;
    A.uv = run->uv[r]; A.ur = run->ur[r]; A.dt = run->dt[r];
    const bool noisy = run->noisy[r] != 0;
    A.sv = noisy ? M.sv : 0.0; A.sr = noisy ? M.sr : 0.0;
    A.h = M.h; A.l = M.l; A.dx = M.dx; A.dy = M.dy;
    A.seed = M.seed; A.call = call0 + (unsigned long long)r;
    ackerman_step_particle(blk, i, A);
  }
}
__global__ __launch_bounds__(256) void vp_batch_propagate_run_kernel(double *pose, int N, int nPer, const VpBatchMotion *mot, const VpBatchRun *run) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  vp_batch_propagate_run_slot(pose, k, nPer, mot, run);
}
// ... of a batch of multi-hypothesis filters (rfsgpu_create_batch_vp_mh): every slot of every block moves, live or not (a slot beyond
// its filter's count is overwritten by the copy that makes it live), except those of a filter whose overflow word is up -- it has
// abandoned its cycle and what is enqueued behind it, as a handle's LiveCount forms do.  words: filter 0's cycle words, wordStride
// ints per filter, ovfWord the overflow word's index (FsCycleState, fastslam_cycle.h).
__global__ __launch_bounds__(256) void vp_batch_propagate_run_guard_kernel(double *pose, int N, int nPer, const VpBatchMotion *mot, const VpBatchRun *run,
                                                                           const int *words, int wordStride, int ovfWord) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  if (words[(size_t)(k / nPer) * wordStride + ovfWord] != 0) return;
  vp_batch_propagate_run_slot(pose, k, nPer, mot, run);
}

// The words of a batch's walk: walk[VBW_MAXEVER] the deepest level any walk has met (folded by the tail), walk[VBW_LAST] the batch's
// maximum of the walk in flight, walk[VBW_FILTER + b] filter b's, entered only where it lies beyond the fixed launches.  The tail
// kernel zeroes the last two kinds behind its reads, so a walk finds them clear without a memset of its own.
enum { VBW_MAXEVER = 0, VBW_LAST = 1, VBW_FILTER = 2 };

// parent[i] = ppid[i], or i where that is no slot of i's filter or the filter's resampleOccured_ is clear (whatever idParent_ an
// older resampling left); level[i] = 0 where parent >= i, else level[parent] + 1, by chasing the chain of lower-slot parents (it
// descends strictly inside the filter's block, so it ends).
__global__ __launch_bounds__(256) void vp_batch_walk_levels_kernel(const int *ppid, const int *resampled, int N, int nPer, int fixedLevels, int *parent, int *level,
                                                                   int *walk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int lv = 0;
  if (i < N) {
    const int b = i / nPer, lo = b * nPer, hi = lo + nPer;
    int p = i;
    if (resampled[b] != 0) {
      p = ppid[i];
      if (p < lo || p >= hi) p = i;
      int c = i, q = p;
      while (q < c) {
        lv++;
        c = q;
        q = ppid[c];
        if (q < lo || q >= hi) q = c;
      }
    }
    parent[i] = p;
    level[i] = lv;
    if (lv > fixedLevels) atomicMax(&walk[VBW_FILTER + b], lv);
  }
  int mx = lv;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
  if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(&walk[VBW_LAST], mx);
}

// Levels firstLevel ... the filter's deepest, one after the other in the filter's own workgroup (blockIdx.x: the filter): a slot of
// level L reads the lists its lower-slot parent (level L - 1, same filter) holds after its own birth step, so a workgroup barrier
// orders the levels and no other workgroup takes part.  The copy and the birth step are the handle's (birth_walk.h, birth.h) on the
// filter's Params, previous set and count, as predict_map_general_batch_kernel / predict_map_long_batch_kernel take them.  A filter
// whose walk ended within the fixed launches leaves at once.
template <int D>
__global__ __launch_bounds__(BIRTH_TAIL_WAVES * 64) void vp_batch_walk_tail_kernel(Buffers B, int cur, BatchArg A, const int *parent, const int *level, int firstLevel,
                                                                                   int *walk) {
  __shared__ CandLDS<D> sCand[BIRTH_TAIL_WAVES];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int bf = blockIdx.x;
  const int maxLevel = walk[VBW_FILTER + bf];
  __syncthreads();                         // every wave has read the filter's word before it is cleared for the next walk
  if (threadIdx.x == 0) {
    walk[VBW_FILTER + bf] = 0;
    if (bf == 0) {
      const int m = walk[VBW_LAST];
      if (m > walk[VBW_MAXEVER]) walk[VBW_MAXEVER] = m;
      walk[VBW_LAST] = 0;
    }
  }
  if (maxLevel < firstLevel) return;       // (workgroup-uniform)
  const Params &P = A.params[bf];
  const int nZprev = A.filt[bf].nZprev;
  Buffers Bf = B;
  Bf.Z = A.zPrev + (size_t)bf * (RFSGPU_MAX_Z * D);
  const BirthLists live{B.unusedMask, B.candCount, B.candSup, B.candChk, B.candMean, B.candCov};
  const int lo = bf * A.nPer, hi = min(lo + A.nPer, B.N);
  for (int L = firstLevel; L <= maxLevel; L++) {
    for (int i = lo + wave; i < hi; i += BIRTH_TAIL_WAVES) {
      if (__builtin_amdgcn_readfirstlane(level[i]) != L) continue;
      birth_lists_copy_wave(live, parent[i], live, i, lane);
      __threadfence();                     // the copy is in memory before the lanes of this wave read it back
      const int listBefore = B.candCount[i] + ((nZprev > 0) ? __popcll(B.unusedMask[i]) : 0);
      if (listBefore <= 64) birth_step_lanes<D>(Bf, P, cur, i, lane, nZprev, B.count[i]);
      else birth_step_lds<D>(Bf, P, cur, i, lane, nZprev, sCand[wave]);
      vp_batch_note_birth_errors(B, A, i, bf, lane, listBefore);
    }
    __threadfence();                       // this level's lists are in memory before the next level's waves copy them
    __syncthreads();
  }
}

// Behind the walk's read: resampleOccured_ falls in the cycle that updates the filter (RBPHDFilter.hpp:526).
__global__ __launch_bounds__(256) void vp_batch_clear_flags_kernel(int *resampled, const BatchFilter *filt, int nF) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < nF && filt[b].nZ > 0) resampled[b] = 0;
}
