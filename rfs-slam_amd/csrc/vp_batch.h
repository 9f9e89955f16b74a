// vp_batch.h -- a batch of Victoria Park RB-PHD filters (rfsgpu_create_batch with RFSGPU_MODEL_VICTORIAPARK_3D,
// rfsgpu_batch_vp_cycle_async): the BATCH forms of the Victoria Park step (vp.h, vp_step_fused_kernel) and of the general birth
// kernels (birth.h).  Slot s belongs to filter s / nPer; what a handle passes as kernel arguments -- Params, the measurement set and
// its count, the eval-point cap, the weighting switch, the previous set and its count -- comes from the BatchArg tables (common.h), by
// the particle's filter.  The laser scan is the handle's: all filters of a batch see the same dataset.  The phases are the device
// functions the handle's kernels call, on the same values: every filter gets the bits its own handle gets.
#pragma once
#include "common.h"
#include "vp.h"
#include "birth.h"
#include "step_fused.h"

// LDS of the batch step.  Shared by the workgroup: the laser scan.  Per wave, at a stride that is the same for every wave of the
// launch: the wave's own copy of its filter's measurement set, then the step's area.  The stride is sized for the batch's largest
// evalCap and set, which bounds every filter's own layout (vp_step_lds_bytes_per_wave grows with both); inside its area a wave lays
// out the phases by ITS filter's evalCap and count, as that filter's handle does, and finds the sort permutation and the Pd cache at
// the tail of the stride.
__host__ __device__ inline size_t vp_batch_scan_lds_bytes(int nScan) { return ((size_t)nScan * 8 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t vp_batch_set_lds_bytes(int nZmax) { return ((size_t)3 * nZmax * 8 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t vp_batch_lds_stride(int cap, int evalCapMax, int nZmax) {
  return vp_batch_set_lds_bytes(nZmax) + vp_step_lds_bytes_per_wave(cap, evalCapMax, nZmax);
}

// Which filter filled its candidate list: a slot whose list could have reached RFSGPU_MAX_CANDIDATES in this birth step (candidates +
// unused measurements before it) while the list bit is up enters its filter in errFilter[1], as batch_note_capacity does for
// gm_capacity in errFilter[0].
__device__ __forceinline__ void vp_batch_note_birth_errors(const Buffers &B, const BatchArg &A, const int i, const int bf, const int lane, const int listBefore) {
  batch_note_capacity(B, A, i, bf, lane);
  if (lane != 0 || listBefore <= RFSGPU_MAX_CANDIDATES) return;
  if (__hip_atomic_load(B.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ERRBIT_BIRTHLIST) atomicMin(A.errFilter + 1, bf);
}

// One wavefront per particle, WPB particles per workgroup, as in vp_step_fused_kernel.  The waves of a workgroup may belong to
// different filters (an odd nPer, or the cost-ordered launch, which maps launch slots to particles across the whole batch), so the
// measurement set is staged per WAVE, by the wave's own lanes; only the scan is staged by the workgroup, and the one workgroup
// barrier follows it before any wave can leave (a slot beyond N, a filter without an update).
template <int WPB>
__global__ __launch_bounds__(WPB * 64) void vp_step_fused_batch_kernel(Buffers B, int cur, MurtyQueue Q, BatchArg A, int nZmax, int evalCapMax, float *stepCost,
                                                                      const int *stepOrder) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double *sScan = reinterpret_cast<double *>(smem_raw);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (int t = threadIdx.x; t < B.nScan; t += WPB * 64) sScan[t] = B.scan[t];
  __syncthreads();
  const int slot = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + wave);
  if (slot >= B.N) return;
  const int i = stepOrder ? __builtin_amdgcn_readfirstlane(stepOrder[slot]) : slot;
  const int bf = __builtin_amdgcn_readfirstlane(i / A.nPer);
  const BatchFilter &F = A.filt[bf];
  const int nZ = __builtin_amdgcn_readfirstlane(F.nZ);
  if (nZ == 0) {
    // no update for this filter this cycle (RBPHDFilter.hpp:450-452): its mixture moves to the slab the others' prune writes (the batch flips `cur` as one)
    const int n = B.count[i];
    for (int pl = 0; pl < P3_COUNT; pl++) {
      const double *src = plane3(B.slab[cur], B.cap, i, pl);
      double *dst = plane3(B.slab[cur ^ 1], B.cap, i, pl);
      for (int m = lane; m < n; m += 64) dst[m] = src[m];
    }
    if (stepCost && lane == 0) stepCost[i] = 0.f;
    return;
  }
  const long long tStart = stepCost ? (long long)wall_clock64() : 0ll;
  const Params &P = A.params[bf];
  const int evalCap = __builtin_amdgcn_readfirstlane(F.evalCap), useWeighting = __builtin_amdgcn_readfirstlane(F.useW);
  const size_t per = vp_step_lds_bytes_per_wave(B.cap, evalCapMax, nZmax);
  unsigned char *wbase = smem_raw + vp_batch_scan_lds_bytes(B.nScan) + (size_t)wave * (vp_batch_set_lds_bytes(nZmax) + per);
  double *sZ = reinterpret_cast<double *>(wbase);
  unsigned char *wmem = wbase + vp_batch_set_lds_bytes(nZmax);
  unsigned char *sPdIdx = wmem + per - (((size_t)B.cap + 15) & ~(size_t)15);
  unsigned short *sPerm = reinterpret_cast<unsigned short *>(sPdIdx - (((size_t)B.cap * 2 + 15) & ~(size_t)15));
  const double *zs = A.z + F.zOff;
  for (int t = lane; t < 3 * nZ; t += 64) sZ[t] = zs[t];
  wave_sync();
  const int nBefore = vp_update_map_particle(B, P, cur, nZ, i, lane, sZ, sScan, wmem, sPdIdx);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  wave_sync();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  batch_note_capacity(B, A, i, bf, lane);
  const unsigned short *perm = nullptr;
  if (useWeighting) {
    vp_weight_particle(B, P, cur, cur ^ 1, nZ, evalCap, Q, i, lane, sZ, sScan, wmem, sPerm, sPdIdx, nBefore);
    wave_sync();
    perm = sPerm;
  }
  vp_merge_particle<true>(B, P, cur, cur ^ 1, i, lane, wmem, perm);
  if (stepCost && lane == 0) stepCost[i] = (float)((long long)wall_clock64() - tStart);
}

// predict_map_general_kernel / predict_map_long_kernel for a batch: the filter's Params, previous set and its count.  BirthLevel and
// birth_inherit_kernel are the handle's, on parent and level tables the host builds across the batch (parents lie inside a filter's block).
template <int D, int WPB>
__global__ __launch_bounds__(WPB * 64) void predict_map_general_batch_kernel(Buffers B, int cur, int addBirth, BirthLevel LV, BatchArg A) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + wave);
  if (i >= B.N) return;
  const int bf = __builtin_amdgcn_readfirstlane(i / A.nPer);
  const int nZprev = __builtin_amdgcn_readfirstlane(A.filt[bf].nZprev);
  Buffers Bf = B;
  Bf.Z = A.zPrev + (size_t)bf * (RFSGPU_MAX_Z * D);
  const int listBefore = B.candCount[i] + ((nZprev > 0) ? __popcll(B.unusedMask[i]) : 0);
  predict_map_general_particle<D>(Bf, A.params[bf], cur, addBirth, nZprev, LV, i, lane);
  if (addBirth && LV.mine(i)) vp_batch_note_birth_errors(B, A, i, bf, lane, listBefore);
}
template <int D, int WPB>
__global__ __launch_bounds__(WPB * 64) void predict_map_long_batch_kernel(Buffers B, int cur, BirthLevel LV, BatchArg A) {
  __shared__ CandLDS<D> sCand[WPB];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + wave);
  if (i >= B.N) return;
  if (!LV.mine(i)) return;
  const int bf = __builtin_amdgcn_readfirstlane(i / A.nPer);
  const int nZprev = __builtin_amdgcn_readfirstlane(A.filt[bf].nZprev);
  const int listBefore = B.candCount[i] + ((nZprev > 0) ? __popcll(B.unusedMask[i]) : 0);
  if (listBefore <= 64) return;     // (predict_map_general_batch_kernel has done it)
  Buffers Bf = B;
  Bf.Z = A.zPrev + (size_t)bf * (RFSGPU_MAX_Z * D);
  birth_step_lds<D>(Bf, A.params[bf], cur, i, lane, nZprev, sCand[wave]);
  vp_batch_note_birth_errors(B, A, i, bf, lane, listBefore);
}
