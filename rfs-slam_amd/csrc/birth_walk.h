// birth_walk.h -- the device side of rfsgpu_rbphd_cycle_async (RBPHDFilter::update, reference include/RBPHDFilter.hpp:444-541, with
// nothing read back) and of the birth predict that follows it:
//
//  rbphd_count_kernel / rbphd_gate_kernel / rbphd_fired_kernel
//        nUpdatesSinceResample_, nMeasurementsSinceResample_ and resampleOccured_ (:448-453, :526-535) as words of the handle's
//        ResampleState block (resample_plan.h), and the gate of :528-529 tested on the device.  Behind a closed gate the plan
//        kernel takes the early exit it has for weights that cannot be resampled, and the gather and the second normalisation leave
//        on their count guards.
//  birth_walk_levels_kernel
//        the inheritance levels of RBPHDFilter.hpp:1005-1011 (birth.h, birth_inherit_kernel) from the ids the device holds: what
//        predict_launch computes on the host from ppid, for a predict enqueued behind cycles that have not been resolved.
//  birth_walk_tail_kernel
//        the levels beyond the RFSGPU_RBPHD_WALK_LEVELS that get launches of their own: one workgroup, a workgroup barrier between
//        two levels, each wave taking slots of the level through the same copy and the same birth step (birth.h).
#pragma once
#include "birth.h"
#include "merge_prune.h"
#include "resample_plan.h"

// ---- the update's counters and its gate -----------------------------------------------------------------------------------------
// resampled: -1 keeps the device's word (cycles are pending), else the host's resampleOccured_ (the first cycle after a resolve).
__global__ __launch_bounds__(64) void rbphd_count_kernel(ResampleState S, int resampled, int nZ) {
  if (threadIdx.x != 0) return;
  if (resampled >= 0) S.w[RCW_RESAMPLED] = resampled;
  S.w[RCW_UPD] += 1;                                      // :448
  S.w[RCW_MEAS] += nZ;                                    // :453 (an update without measurements stops in front of it)
  S.w[RCW_NCYCLES] += 1;
  if (nZ == 0) { S.w[RCW_GATE] = 0; S.w[RSW_FIRED] = 0; }
}
// Behind resample_check_kernel.  resampleOccured_ = false (:526), then the gate (:528-529).  The weights' own verdict moves to
// RCW_BADNOW (the first normalisation's guard) and, sticky, to RCW_BADSEEN (what the resolving call reports); RSW_BAD then also
// closes the plan kernel when the gate is closed.
__global__ __launch_bounds__(64) void rbphd_gate_kernel(ResampleState S, int minUpdates, int minMeasurements) {
  if (threadIdx.x != 0) return;
  const int bad = S.w[RSW_BAD];
  const int gate = (S.w[RCW_UPD] >= minUpdates && S.w[RCW_MEAS] >= minMeasurements) ? 1 : 0;
  S.w[RCW_RESAMPLED] = 0;
  S.w[RCW_GATE] = gate;
  S.w[RCW_NGATE] += (gate && !bad) ? 1 : 0;
  S.w[RCW_BADNOW] = bad;
  S.w[RCW_BADSEEN] |= bad;
  S.w[RSW_BAD] = (bad || !gate) ? 1 : 0;
}
// Behind the tail: where the resampling fired both counters restart and resampleOccured_ is set (:530-535).
__global__ __launch_bounds__(64) void rbphd_fired_kernel(ResampleState S) {
  if (threadIdx.x != 0) return;
  if (S.w[RSW_FIRED] != 0) {
    S.w[RCW_UPD] = 0;
    S.w[RCW_MEAS] = 0;
    S.w[RCW_RESAMPLED] = 1;
    S.w[RCW_NFIRED] += 1;
  }
  S.w[RSW_BAD] = S.w[RCW_BADNOW];
}

// ---- the inheritance walk from the device's ids -----------------------------------------------------------------------------------
// parent[i] = ppid[i], or i where that is no slot of the filter; level[i] = 0 where parent >= i, else level[parent] + 1: every slot
// chases its own chain of lower-slot parents and counts the links (a chain descends strictly, so it ends).  reference == 0
// (RFSGPU_INHERIT_EAGER: the lists travelled with the copies) or a clear resampleOccured_: every slot keeps itself at level 0, and
// the staging kernels and the level launches behind this one find nothing to do.  S.w[RCW_WALK_MAX] is zeroed in front of the
// launch.
__global__ __launch_bounds__(256) void birth_walk_levels_kernel(ResampleState S, int n, int reference, int *parent, int *level) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int p = i, lv = 0;
  if (i < n && reference && S.w[RCW_RESAMPLED] != 0) {
    p = S.ppid[i];
    if (p < 0 || p >= n) p = i;
    int c = i, q = p;
    while (q < c) {
      lv++;
      c = q;
      q = S.ppid[c];
      if (q < 0 || q >= n) q = c;
    }
  }
  if (i < n) { parent[i] = p; level[i] = lv; }
  int mx = lv;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
  if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(&S.w[RCW_WALK_MAX], mx);
}

// birth_lists_copy (birth.h) by the lanes of one wave.
__device__ inline void birth_lists_copy_wave(const BirthLists &S, int s, const BirthLists &Dst, int d, int lane) {
  const int nc = S.count[s];
  const size_t sb = (size_t)s * RFSGPU_MAX_CANDIDATES, db = (size_t)d * RFSGPU_MAX_CANDIDATES;
  for (int t = lane; t < nc * 3; t += 64) Dst.mean[db * 3 + t] = S.mean[sb * 3 + t];
  for (int t = lane; t < nc * 6; t += 64) Dst.cov[db * 6 + t] = S.cov[sb * 6 + t];
  for (int t = lane; t < nc; t += 64) { Dst.sup[db + t] = S.sup[sb + t]; Dst.chk[db + t] = S.chk[sb + t]; }
  if (lane == 0) { Dst.count[d] = nc; Dst.unused[d] = S.unused[s]; }
}

// Levels firstLevel ... S.w[RCW_WALK_MAX], one after the other in ONE workgroup: a slot of level L reads the lists its lower-slot
// parent (level L - 1) holds after its own birth step, so the levels are ordered by a workgroup barrier -- no other workgroup
// takes part, nothing waits on memory.  LANES: the 2-D model with immediate births (predict_map_particle, merge_prune.h) in place
// of the candidate-list walk.  The static step has been done by the level-0 launch.  Lane 0 of the workgroup also folds this
// walk's depth into the deepest one seen (rfsgpu_rbphd_cycle_counts).
#define BIRTH_TAIL_WAVES 2
template <int D, bool LANES>
__global__ __launch_bounds__(BIRTH_TAIL_WAVES * 64) void birth_walk_tail_kernel(Buffers B, Params P, int cur, int nZprev, ResampleState S, const int *parent,
                                                                                 const int *level, int firstLevel) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int maxLevel = S.w[RCW_WALK_MAX];
  if (threadIdx.x == 0 && maxLevel > S.w[RCW_MAXLEVEL]) S.w[RCW_MAXLEVEL] = maxLevel;
  const BirthLists live{B.unusedMask, B.candCount, B.candSup, B.candChk, B.candMean, B.candCov};
  for (int L = firstLevel; L <= maxLevel; L++) {
    for (int i = wave; i < B.N; i += BIRTH_TAIL_WAVES) {
      if (__builtin_amdgcn_readfirstlane(level[i]) != L) continue;
      birth_lists_copy_wave(live, parent[i], live, i, lane);
      __threadfence();                     // the copy is in memory before the lanes of this wave read it back
      if constexpr (LANES) {
        predict_map_particle<64>(B, P, cur, i, lane, true, nZprev, B.pose, false);
      } else {
        __shared__ CandLDS<D> sCand[BIRTH_TAIL_WAVES];
        if (B.candCount[i] + ((nZprev > 0) ? __popcll(B.unusedMask[i]) : 0) <= 64) birth_step_lanes<D>(B, P, cur, i, lane, nZprev, B.count[i]);
        else birth_step_lds<D>(B, P, cur, i, lane, nZprev, sCand[wave]);
      }
    }
    __threadfence();                       // this level's lists are in memory before the next level's waves copy them
    __syncthreads();
  }
}
