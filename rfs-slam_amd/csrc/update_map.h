// update_map.h -- phd_update_map: RBPHDFilter::updateMap (reference include/RBPHDFilter.hpp:543-725) with
// KalmanFilter::correct (include/KalmanFilter.hpp:261-342), KalmanFilter_RngBrg::calculateInnovation
// (src/KalmanFilter_RngBrg.cpp:52-65) and MeasurementModel_RngBrg::{measure, probabilityOfDetection}
// fused into one kernel.
//
// Two forms of the same per-particle routine (see the comments above each): phd_update_map_particle, one wavefront per
// particle (the stand-alone kernel), and phd_update_map_block, a workgroup per particle (inside the fused step kernel).
// The measurement set is staged once per workgroup in LDS and, where the index is wave-uniform, read through the scalar
// cache.  The nM x nZ weight table of the reference never exists: phase 1 builds each landmark's innovation-gate bitmask,
// puts only the gated pairs through the Mahalanobis gate and the Gaussian, and writes the survivors into a dense
// (m, z)-row-major list in LDS (list position == output slot); lane z folds the survivors of measurement z into its
// normaliser in the reference's summation order (clutter, then landmarks ascending).  Phase 2 is dense over the list:
// normalise, recompute the landmark's KF quantities, emit.  Phase 3: missed-detection weights + near-limit heuristic.
// HBM traffic per particle = one read of the mixture + the appended records + the weight planes.
#pragma once
#include "common.h"

// Landmark-level quantities of KalmanFilter::correct that are shared by all measurements.
struct LmKF {
  double zx0, zx1;            // expected measurement
  double i00, i01, i10, i11;  // S^-1
  double factor;              // sqrt((2pi)^2 |S|)
  double k00, k01, k10, k11;  // Kalman gain
  double p00, p01, p11;       // updated covariance (symmetrised)
  bool ok;                    // measure() returned true
};

__device__ __forceinline__ void lm_precompute(const Params &P, const PoseReg &pr, double mx, double my, double sxx, double sxy, double syy,
                                              LmKF &k, double &range) {
  MeasOut mo;
  rb_measure(P, pr, mx, my, sxx, sxy, syy, mo);
  range = mo.range;
  k.ok = mo.inRange;
  k.zx0 = mo.z0;
  k.zx1 = mo.z1;
  double det;
  inv2(mo.s00, mo.s01, mo.s10, mo.s11, k.i00, k.i01, k.i10, k.i11, det);
  k.factor = pdf_factor2(det);
  // K = (P * H^T) * S^-1
  double t00 = sxx * mo.h00 + sxy * mo.h01, t01 = sxx * mo.h10 + sxy * mo.h11;
  double t10 = sxy * mo.h00 + syy * mo.h01, t11 = sxy * mo.h10 + syy * mo.h11;
  k.k00 = t00 * k.i00 + t01 * k.i10;
  k.k01 = t00 * k.i01 + t01 * k.i11;
  k.k10 = t10 * k.i00 + t11 * k.i10;
  k.k11 = t10 * k.i01 + t11 * k.i11;
  // P+ = (I - K H) P, then (P+ + P+^T)/2
  double kh00 = k.k00 * mo.h00 + k.k01 * mo.h10, kh01 = k.k00 * mo.h01 + k.k01 * mo.h11;
  double kh10 = k.k10 * mo.h00 + k.k11 * mo.h10, kh11 = k.k10 * mo.h01 + k.k11 * mo.h11;
  double a00 = 1.0 - kh00, a01 = 0.0 - kh01, a10 = 0.0 - kh10, a11 = 1.0 - kh11;
  double q00 = a00 * sxx + a01 * sxy, q01 = a00 * sxy + a01 * syy;
  double q10 = a10 * sxx + a11 * sxy, q11 = a10 * sxy + a11 * syy;
  k.p00 = (q00 + q00) / 2;
  k.p01 = (q01 + q10) / 2;
  k.p11 = (q11 + q11) / 2;
}

// One (landmark, measurement) pair: returns Pd*w*likelihood, or 0 when any gate rejects it
// (include/KalmanFilter.hpp:311-338 + include/RBPHDFilter.hpp:622-632).  nu = wrapped innovation.
__device__ __forceinline__ double pair_weight(const Params &P, const LmKF &k, double pdw, double z0, double z1, double &nu0, double &nu1) {
  if (!k.ok) return 0.0;
  double e0 = z0 - k.zx0, e1 = z1 - k.zx1;
  if (P.kfRange > 0 && fabs(e0) > P.kfRange) return 0.0;
  double w1 = wrap_pi(e1);
  if (P.kfBearing > 0 && fabs(w1) > P.kfBearing) return 0.0;
  nu0 = e0;
  nu1 = w1;
  // likelihood uses the UNWRAPPED difference (KalmanFilter.hpp:317-320)
  double t0 = e0 * k.i00 + e1 * k.i10;
  double t1 = e0 * k.i01 + e1 * k.i11;
  double md2 = t0 * e0 + t1 * e1;
  if (md2 > P.newGaussMd2) return 0.0;
  double lik = gauss_from_md2(md2, k.factor);
  if (lik == 0.0) return 0.0;
  return pdw * lik;
}

// The measurement index of the gate prefilter (below): cumulative bearing masks [256], cumulative range masks [64], header.
#define GATE_INDEX_BBINS 256
#define GATE_INDEX_RBINS 64
#define GATE_INDEX_BYTES ((GATE_INDEX_BBINS + GATE_INDEX_RBINS) * 8 + 32)
// LDS per wave: survivor list (value, packed (m,z)) + per-landmark segment (start, count) + final normalisers + the measurement index.
__host__ __device__ inline size_t update_map_lds_bytes_per_wave(int cap) {
  return (size_t)cap * (8 + 4 + 4) + RFSGPU_MAX_Z * 8 + GATE_INDEX_BYTES;
}
// where the index starts inside a wave's / workgroup's block (behind sV | sCol | sMZ | sSeg)
__host__ __device__ inline size_t update_map_index_offset(int cap) {
  return (size_t)cap * (8 + 4 + 4) + RFSGPU_MAX_Z * 8;
}

// Gates of KalmanFilter_RngBrg::calculateInnovation only (cheap part of pair_weight).
__device__ __forceinline__ bool pair_gate(const Params &P, const LmKF &k, double z0, double z1) {
  const double e0 = z0 - k.zx0;
  if (P.kfRange > 0 && fabs(e0) > P.kfRange) return false;
  const double w1 = wrap_pi(z1 - k.zx1);
  if (P.kfBearing > 0 && fabs(w1) > P.kfBearing) return false;
  return true;
}
// Mahalanobis distance of the pair as pair_value forms it (same expression, same bits)
__device__ __forceinline__ double pair_md2(const LmKF &k, double z0, double z1) {
  const double e0 = z0 - k.zx0, e1 = z1 - k.zx1;  // UNWRAPPED difference
  const double t0 = e0 * k.i00 + e1 * k.i10;
  const double t1 = e0 * k.i01 + e1 * k.i11;
  return t0 * e0 + t1 * e1;
}
// Likelihood part for a pair that passed the innovation gates: Pd*w*lik or 0 (KalmanFilter.hpp:317-326, RBPHDFilter.hpp:622-632).
__device__ __forceinline__ double pair_value(const Params &P, const LmKF &k, double pdw, double z0, double z1) {
  const double e0 = z0 - k.zx0, e1 = z1 - k.zx1;  // UNWRAPPED difference
  const double t0 = e0 * k.i00 + e1 * k.i10;
  const double t1 = e0 * k.i01 + e1 * k.i11;
  const double md2 = t0 * e0 + t1 * e1;
  if (md2 > P.newGaussMd2) return 0.0;
  const double lik = gauss_from_md2(md2, k.factor);
  if (lik == 0.0) return 0.0;
  return pdw * lik;
}

// ---- innovation-gate prefilter in packed fp32 ------------------------------------------------------------------------------
// The gates of KalmanFilter_RngBrg::calculateInnovation (src/KalmanFilter_RngBrg.cpp:52-65) reject almost every
// (landmark, measurement) pair, and evaluating them in fp64 for all nM x nZ pairs was the largest single item of the map
// update.  The sweep over the measurement set therefore runs in fp32, two measurements per packed instruction (v_pk_*), with
// thresholds widened by a bound on the fp32 rounding of the operands, the difference and the 2-pi reduction: it can only
// let extra pairs through, never drop one.  Every candidate then goes through the exact fp64 gate (pair_gate) before its
// likelihood is evaluated, so results are unchanged.
typedef float f2_t __attribute__((ext_vector_type(2)));

// Stages the measurement set into the LDS head (RFS_Z_LDS_BYTES): doubles, the fp32 copy, and the two maxima the prefilter's
// error bound needs.  All threads of the block call it; the caller synchronises afterwards.
// `zsrc(t)` yields double t of the set (a device buffer, or the kernel-argument block indexed in place -- taking the
// address of a by-value kernel argument would make the compiler copy it to scratch).
template <class ZSrc>
__device__ __forceinline__ void stage_measurements_lds(unsigned char *smem_raw, ZSrc zsrc, int nZ, int tid, int nThreads) {
  double *sZ = reinterpret_cast<double *>(smem_raw);
  float *sZf = reinterpret_cast<float *>(smem_raw + 2 * RFSGPU_MAX_Z * 8);
  for (int t = tid; t < 2 * nZ; t += nThreads) sZ[t] = zsrc(t);
  if (tid < 64) {
    float ar = 0.f, ab = 0.f;
    const int z = tid < nZ ? tid : 0;
    const float zr = nZ > 0 ? (float)zsrc(2 * z) : 0.f, zb = nZ > 0 ? (float)zsrc(2 * z + 1) : 0.f;
    sZf[tid] = zr;                       // (entries beyond nZ repeat measurement 0: the sweep reads whole pairs)
    sZf[RFSGPU_MAX_Z + tid] = zb;
    ar = wave_max_f32(fabsf(zr));
    ab = wave_max_f32(fabsf(zb));
    if (tid == 0) { sZf[2 * RFSGPU_MAX_Z] = ar; sZf[2 * RFSGPU_MAX_Z + 1] = ab; }
  }
}

// Candidate mask of one landmark: bit z set if measurement z MAY pass both innovation gates.  The dense form: every measurement
// against the landmark.  gate_candidates (below) takes it for the sets its index cannot bound.
__device__ __forceinline__ unsigned long long gate_candidates_sweep(const Params &P, const LmKF &k, const bool live, const int nZ, const float *sZf) {
  const float zx0 = (float)k.zx0, zx1 = (float)k.zx1;
  const float zrMax = sZf[2 * RFSGPU_MAX_Z], zbMax = sZf[2 * RFSGPU_MAX_Z + 1];
  const float inf = __builtin_huge_valf();
  // |computed - exact| <= 2^-23 (|a| + |b|) for the rounded operands and difference; the bearing also carries the fp32 2-pi
  // reduction (|k| <= (zbMax + pi) / 2pi + 1 multiples of a constant that is off by < 2e-7)
  float thrR = (P.kfRange > 0) ? (float)P.kfRange * (1.f + 1e-6f) + 2.5e-7f * (zrMax + fabsf(zx0)) + 1e-30f : inf;
  float thrB = (P.kfBearing > 0) ? (float)P.kfBearing * (1.f + 1e-6f) + 1e-6f * (zbMax + 3.2f) + 1e-6f : inf;
  if (!(zbMax < 50.f)) thrB = inf;       // far outside any sensible bearing range (or NaN): the exact test decides
  if (!(zrMax < 1.0e30f)) thrR = inf;
  const f2_t vx0 = {zx0, zx0}, vx1 = {zx1, zx1};
  const f2_t twoPi = {6.2831853071795864769f, 6.2831853071795864769f}, inv2Pi = {0.15915494309189533577f, 0.15915494309189533577f};
  unsigned lo = 0, hi = 0;
#pragma unroll 1
  for (int half = 0; half < 2; half++) {
    const int zBase = 32 * half;
    if (zBase >= nZ) break;
    unsigned bits = 0;
    const f2_t *pr = reinterpret_cast<const f2_t *>(sZf + zBase), *pb = reinterpret_cast<const f2_t *>(sZf + RFSGPU_MAX_Z + zBase);
    const int nPairs = (min(nZ - zBase, 32) + 1) >> 1;
#pragma unroll 4
    for (int q = 0; q < nPairs; q++) {
      const f2_t zr = pr[q], zb = pb[q];     // uniform address: LDS broadcast reads of two measurements each
      const f2_t e0 = zr - vx0;
      f2_t w = zb - vx1;
      f2_t kk = w * inv2Pi;
      kk.x = __builtin_rintf(kk.x); kk.y = __builtin_rintf(kk.y);
      w = w - kk * twoPi;
      // !(x > t) form: a NaN is a candidate
      const bool c0 = ((int)!(fabsf(e0.x) > thrR) & (int)!(fabsf(w.x) > thrB)) != 0;
      const bool c1 = ((int)!(fabsf(e0.y) > thrR) & (int)!(fabsf(w.y) > thrB)) != 0;
      bits |= (c0 ? 1u : 0u) << (2 * q);
      bits |= (c1 ? 2u : 0u) << (2 * q);
    }
    if (half == 0) lo = bits; else hi = bits;
  }
  unsigned long long m = ((unsigned long long)hi << 32) | lo;
  m &= (nZ >= 64) ? ~0ull : ((1ull << nZ) - 1ull);
  return live ? m : 0ull;
}

// ---- measurement index ------------------------------------------------------------------------------------------------------
// The sweep tests all nZ measurements against every landmark to find the one or two inside its gates (the bearing gate alone
// passes a few per cent of the circle).  The index turns that round: once per particle, before the pass loop, the measurement
// set is binned -- 256 bearing bins over [-pi, pi), 64 range bins between the set's smallest and largest range -- and two
// tables of cumulative masks are left in LDS: cumB[b] / cumR[b] = the measurements whose bin is <= b.  A landmark's candidates
// are then two table differences: (cumB[hi] & ~cumB[lo - 1]) & (cumR[hi'] & ~cumR[lo' - 1]), a few dozen instructions instead
// of a loop over the set.  As with the sweep the mask may only be too large, never too small -- every candidate still goes
// through pair_gate in fp64 -- and that is argued as follows.
//  Bearing: a measurement's bin comes from its fp32 bearing reduced like the sweep's difference (b - rint(b / 2pi) 2pi); the
//    window is the landmark's fp32 bearing +- thrB, the sweep's threshold, whose allowances (rounded operands, |k| multiples of
//    an fp32 2pi) cover the reduction of the measurement alone as they cover that of the difference; one guard bin on either
//    side (2pi / 256 = 0.0245 rad, four orders above any of those errors) takes up the bin arithmetic, a reduced bearing that
//    lands a rounding beyond +-pi (clamped into the end bins) and the rounding of the window's ends.  A window that crosses
//    +-pi is the union of its two end pieces.
//  Range: bin(x) = clamp(floor((x - rMin) * scale)) is a monotone function of the fp32 range, and the SAME function is applied
//    to the window's ends: lo <= r <= hi implies bin(lo) <= bin(r) <= bin(hi), whatever the rounding inside bin().  The window is
//    the landmark's fp32 range +- (thrR + guard), where thrR is the sweep's threshold and the guard, another 2.5e-7 (max |range|
//    + |landmark range|), covers the rounding of the two ends themselves.
//  A measurement with a NaN coordinate is a candidate of every landmark (as in the sweep, whose comparisons a NaN passes).
// The sweep stays for what the index cannot bound, decided once per particle and wave-uniformly: a gate that is disabled, a
// threshold that is not finite (|bearing| >= 50, |range| >= 1e30, inf), a bearing window that would cover the circle (thrB >= 3),
// a range span that is zero or not finite -- and for handles created under RFSGPU_GATE_INDEX=0 (Params::gateIndex).
struct GateIndex {   // wave-uniform: lives in SGPRs
  const unsigned long long *cumB, *cumR;
  float rMin, rMax, rScale;     // range bins: (r - rMin) * rScale
  float thrB, kfR1, zrMax;      // the sweep's bearing threshold; (float)kfRange (1 + 1e-6); max |range| of the set
  unsigned long long always;    // measurements with a NaN coordinate
  bool use;
};
#define GATE_INDEX_THRB_MAX 3.0f   // 2 thrB * 256 / 2pi + 3 bins (floors, guards) must stay below 255 bins: thrB < 3.08

__device__ __forceinline__ unsigned gate_or_scan_u32(unsigned x) {   // inclusive OR-scan over the lanes (wave_excl_scan's moves)
  x |= (unsigned)dpp_i32<0x111, 0xf>((int)x);  // row_shr:1
  x |= (unsigned)dpp_i32<0x112, 0xf>((int)x);  // row_shr:2
  x |= (unsigned)dpp_i32<0x114, 0xf>((int)x);  // row_shr:4
  x |= (unsigned)dpp_i32<0x118, 0xf>((int)x);  // row_shr:8
  x |= (unsigned)dpp_i32<0x142, 0xa>((int)x);  // row_bcast:15 into rows 1 and 3
  x |= (unsigned)dpp_i32<0x143, 0xc>((int)x);  // row_bcast:31 into rows 2 and 3
  return x;
}
__device__ __forceinline__ unsigned long long gate_or_scan_u64(unsigned long long v) {
  return ((unsigned long long)gate_or_scan_u32((unsigned)(v >> 32)) << 32) | gate_or_scan_u32((unsigned)v);
}
// bin coordinate of a bearing in [-pi, pi]: 256 bins over the circle
__device__ __forceinline__ float gate_bearing_coord(float b) { return (b + 3.14159265358979323846f) * (float)(GATE_INDEX_BBINS / (2 * RFS_PI)); }
__device__ __forceinline__ int gate_range_bin(float r, float rMin, float rScale) {
  return (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf((r - rMin) * rScale), 0.f), (float)(GATE_INDEX_RBINS - 1));
}

// One wave bins the staged set's bearings and leaves cumB in `tab` (its first 256 entries).
__device__ __forceinline__ void gate_index_build_bearing(unsigned char *tabRaw, const float *sZf, const int nZ, const int lane) {
  unsigned long long *cumB = reinterpret_cast<unsigned long long *>(tabRaw);
#pragma unroll
  for (int j = 0; j < GATE_INDEX_BBINS / 64; j++) cumB[64 * j + lane] = 0ull;
  wave_sync();
  if (lane < nZ) {
    const float zb = sZf[RFSGPU_MAX_Z + lane];
    const float red = zb - __builtin_rintf(zb * 0.15915494309189533577f) * 6.2831853071795864769f;
    const int bin = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf(gate_bearing_coord(red)), 0.f), (float)(GATE_INDEX_BBINS - 1));  // (NaN: bin 0, and `always`)
    atomicOr(&cumB[bin], 1ull << lane);
  }
  wave_sync();
  unsigned long long carry = 0ull;   // the bins of the segments before: wave-uniform
#pragma unroll
  for (int j = 0; j < GATE_INDEX_BBINS / 64; j++) {   // lane l holds bin 64 j + l
    const unsigned long long v = gate_or_scan_u64(cumB[64 * j + lane]) | carry;
    cumB[64 * j + lane] = v;
    carry = readlane_u64(v, 63);
  }
}
// One wave bins the ranges, leaves cumR and the header: {rMin, rMax, rScale, span usable} | always.
__device__ __forceinline__ void gate_index_build_range(unsigned char *tabRaw, const float *sZf, const int nZ, const int lane) {
  unsigned long long *cumR = reinterpret_cast<unsigned long long *>(tabRaw) + GATE_INDEX_BBINS;
  float *hdr = reinterpret_cast<float *>(cumR + GATE_INDEX_RBINS);
  const float zr = sZf[lane], zb = sZf[RFSGPU_MAX_Z + lane];   // (lanes beyond nZ read measurement 0 again: stage_measurements_lds)
  const float rMin = wave_min_f32(zr), rMax = wave_max_f32(zr);
  const float span = rMax - rMin, rScale = (float)GATE_INDEX_RBINS / span;
  const bool ok = nZ > 0 && span > 0.f && rScale < __builtin_huge_valf();
  const unsigned long long always = __ballot(lane < nZ && (zr != zr || zb != zb));
  cumR[lane] = 0ull;
  wave_sync();
  if (ok && lane < nZ) atomicOr(&cumR[gate_range_bin(zr, rMin, rScale)], 1ull << lane);
  wave_sync();
  cumR[lane] = gate_or_scan_u64(cumR[lane]);
  if (lane == 0) {
    hdr[0] = rMin; hdr[1] = rMax; hdr[2] = rScale;
    reinterpret_cast<int *>(hdr)[3] = ok ? 1 : 0;
    reinterpret_cast<unsigned long long *>(hdr)[2] = always;
  }
}
// After the build (and a barrier): the wave's view of the index, and whether this set can use it at all.
__device__ __forceinline__ GateIndex gate_index_load(const Params &P, const unsigned char *tabRaw, const float *sZf) {
  GateIndex G;
  G.cumB = reinterpret_cast<const unsigned long long *>(tabRaw);
  G.cumR = G.cumB + GATE_INDEX_BBINS;
  const float *hdr = reinterpret_cast<const float *>(G.cumR + GATE_INDEX_RBINS);
  const float zrMax = sZf[2 * RFSGPU_MAX_Z], zbMax = sZf[2 * RFSGPU_MAX_Z + 1];
  const float inf = __builtin_huge_valf();
  const float thrB = (float)P.kfBearing * (1.f + 1e-6f) + 1e-6f * (zbMax + 3.2f) + 1e-6f;   // as in the sweep
  const float kfR1 = (float)P.kfRange * (1.f + 1e-6f);
  int use = 0;
  if (P.gateIndex) {
    const bool ok = P.kfRange > 0 && P.kfBearing > 0 && zbMax < 50.f && zrMax < 1.0e30f && thrB < GATE_INDEX_THRB_MAX && kfR1 < inf &&
                    reinterpret_cast<const int *>(hdr)[3] != 0;
    use = ok ? 1 : 0;
  }
  auto sf = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
  G.use = __builtin_amdgcn_readfirstlane(use) != 0;
  G.rMin = sf(hdr[0]); G.rMax = sf(hdr[1]); G.rScale = sf(hdr[2]);
  G.thrB = sf(thrB); G.kfR1 = sf(kfR1); G.zrMax = sf(zrMax);
  const unsigned long long al = reinterpret_cast<const unsigned long long *>(hdr)[2];
  G.always = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(al >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)al);
  return G;
}

// Candidate mask of one landmark: bit z set if measurement z MAY pass both innovation gates.
__device__ __forceinline__ unsigned long long gate_candidates(const Params &P, const LmKF &k, const bool live, const int nZ, const float *sZf,
                                                              const GateIndex &G) {
  if (!G.use) return gate_candidates_sweep(P, k, live, nZ, sZf);
  const float zx0 = (float)k.zx0, zx1 = (float)k.zx1;
  const float inf = __builtin_huge_valf();
  const unsigned long long zmask = (nZ >= 64) ? ~0ull : ((1ull << nZ) - 1ull);
  // bearing: bins [ilo, ihi] modulo 256 (zx1 lies in [-pi, pi] and thrB < 3, so ilo >= -130, ihi <= 386 and ihi - ilo < 255)
  const int ilo = (int)__builtin_floorf(gate_bearing_coord(zx1 - G.thrB)) - 1, ihi = (int)__builtin_floorf(gate_bearing_coord(zx1 + G.thrB)) + 1;
  const int bl = ilo & (GATE_INDEX_BBINS - 1), bh = ihi & (GATE_INDEX_BBINS - 1);
  unsigned long long bA = G.cumB[(bl - 1) & (GATE_INDEX_BBINS - 1)];
  const unsigned long long bH = G.cumB[bh];
  bA = (bl == 0) ? 0ull : bA;
  const unsigned long long mB = (bl > bh) ? (bH | ~bA) : (bH & ~bA);   // across the seam: [bl, 255] and [0, bh]
  // range
  const float thrR = G.kfR1 + 2.5e-7f * (G.zrMax + fabsf(zx0)) + 1e-30f;   // as in the sweep
  const float guard = 2.5e-7f * (G.zrMax + fabsf(zx0));
  const float lo = zx0 - thrR - guard, hi = zx0 + thrR + guard;
  const int rl = gate_range_bin(lo, G.rMin, G.rScale), rh = gate_range_bin(hi, G.rMin, G.rScale);
  unsigned long long rA = G.cumR[(rl - 1) & (GATE_INDEX_RBINS - 1)];
  const unsigned long long rH = G.cumR[rh];
  rA = (rl == 0) ? 0ull : rA;
  unsigned long long mR = rH & ~rA;
  mR = (hi < G.rMin || lo > G.rMax) ? 0ull : mR;   // (every fp32 range of the set lies in [rMin, rMax])
  unsigned long long m = (mB & mR) | G.always;
  m = (fabsf(zx0) < inf && fabsf(zx1) < inf) ? m : ~0ull;   // a landmark without a finite expected measurement: the exact test decides
  m &= zmask;
  return live ? m : 0ull;
}

// New Gaussian of a surviving (landmark, measurement) pair: KalmanFilter::correct's mean (include/KalmanFilter.hpp:311-316)
// with the wrapped innovation, and the landmark's updated covariance.
__device__ __forceinline__ void emit_updated(const LmKF &k, double mx, double my, double z0, double z1, double *pMX, double *pMY, double *pSXX,
                                             double *pSXY, double *pSYY, int pos) {
  const double nu0 = z0 - k.zx0;
  const double nu1 = wrap_pi(z1 - k.zx1);
  pMX[pos] = mx + (k.k00 * nu0 + k.k01 * nu1);
  pMY[pos] = my + (k.k10 * nu0 + k.k11 * nu1);
  pSXX[pos] = k.p00;
  pSXY[pos] = k.p01;
  pSYY[pos] = k.p11;
}

#define UPDMAP_KEEP 4  // survivor values a lane keeps in registers between the likelihood loop and the list write

// Structure (one wavefront per particle):
//  phase 1, per pass of 64 landmarks: KF quantities once per landmark; the packed-fp32 sweep over the measurements gives each
//    landmark's candidate mask; only the set bits (a few per landmark) go through the exact innovation gates, the Mahalanobis
//    gate and the Gaussian; survivors are written into a dense (m,z)-row-major list in LDS through a wave prefix sum -- list
//    position == output slot of the new Gaussian, whose mean and covariance are written to the slab right there (the lane
//    still holds the landmark's gain and updated covariance); lane z then folds this pass's survivors of measurement z into
//    its normaliser in landmark order, i.e. in the reference's summation order (clutter first, then m ascending).
//  phase 2, dense over the survivor list: normalise, write the weights.  (A new Gaussian whose normalised weight is not
//    positive -- only through inf / NaN arithmetic -- is dropped by an in-place compaction of the appended block.)
//  phase 3: missed-detection weights (+ near-limit heuristic from the landmark's list segment), unused mask.
#ifndef UPDMAP_WAVES_PER_EU
#define UPDMAP_WAVES_PER_EU 2
#endif

// In-place, order-preserving removal of the appended Gaussians whose normalised weight (sV[q]) is not > 0; executed by ONE
// wave (the rare path of phase 2).  Returns the number kept.
__device__ __forceinline__ int compact_appended(const double *sV, int nM, int nSurv, int lane, double *pW, double *pWP, double *pMX, double *pMY,
                                                double *pSXX, double *pSXY, double *pSYY) {
  int out = 0;
  for (int s0 = 0; s0 < nSurv; s0 += 64) {
    const int q = s0 + lane;
    const bool keep = (q < nSurv) && (sV[q] > 0.0);
    const unsigned long long km = __ballot(keep);
    double v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0;
    if (keep) { v0 = sV[q]; v1 = pMX[nM + q]; v2 = pMY[nM + q]; v3 = pSXX[nM + q]; v4 = pSXY[nM + q]; v5 = pSYY[nM + q]; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    wave_sync();
    if (keep) {
      const int d = nM + out + __popcll(km & ((1ull << lane) - 1ull));
      pW[d] = v0; pWP[d] = 0.0; pMX[d] = v1; pMY[d] = v2; pSXX[d] = v3; pSXY[d] = v4; pSYY[d] = v5;
    }
    out += __popcll(km);
  }
  return out;
}

// One particle, one wavefront: `lane` of the calling wave, `smemZ` the workgroup's staged measurement set (RFS_Z_LDS_BYTES), `wb`
// this wave's LDS block (update_map_lds_bytes_per_wave).  The stand-alone kernel's form.
__device__ __forceinline__ void phd_update_map_particle(const Buffers &B, const Params &P, const int cur, const int nZ, const int i,
                                                        const int lane, const unsigned char *smemZ, unsigned char *wb) {
  const double *sZ = reinterpret_cast<const double *>(smemZ);
  const float *sZf = reinterpret_cast<const float *>(smemZ + 2 * RFSGPU_MAX_Z * 8);
  const int cap = B.cap;
  double *sV = reinterpret_cast<double *>(wb);                 // [cap] survivor values Pd*w*lik, later the normalised weights
  double *sCol = sV + cap;                                      // [MAX_Z] final normalisers
  unsigned *sMZ = reinterpret_cast<unsigned *>(sCol + RFSGPU_MAX_Z);  // [cap] (m << 8) | z
  unsigned *sSeg = sMZ + cap;                                   // [cap] per landmark: (start << 8) | count

  const int nM = B.count[i];
  const unsigned long long zmask = (nZ >= 64) ? ~0ull : ((1ull << nZ) - 1ull);
  if (nM == 0) {  // :559-564
    if (lane == 0) {
      B.unusedMask[i] = zmask;
      B.nInFov[i] = 0;
    }
    return;
  }
  double *slab = B.slab[cur];
  double *pW = plane(slab, cap, i, PL_W), *pWP = plane(slab, cap, i, PL_WP);
  double *pMX = plane(slab, cap, i, PL_MX), *pMY = plane(slab, cap, i, PL_MY);
  double *pSXX = plane(slab, cap, i, PL_SXX), *pSXY = plane(slab, cap, i, PL_SXY), *pSYY = plane(slab, cap, i, PL_SYY);

  DBG_T(0, 0);
  PoseReg pr;
  load_pose(B, P, i, pr);

  // the measurement index of the gate prefilter, in this wave's own block
  unsigned char *gTab = wb + update_map_index_offset(cap);
  if (P.gateIndex) {
    gate_index_build_bearing(gTab, sZf, nZ, lane);
    gate_index_build_range(gTab, sZf, nZ, lane);
    wave_sync();
  }
  const GateIndex G = gate_index_load(P, gTab, sZf);

  const int nPass = (nM + 63) >> 6;
  const int room = cap - nM;  // survivors that still fit as new Gaussians
  int nFov = 0;
  double wsum = 0.0;           // SC-PHD: sum of prior weights
  double cs = P.clutter;       // lane z: normaliser of measurement z (reference: sum = clutter; sum += W[m][z] ...)
  int nSurv = 0;
  bool overflow = false;

  // ---------------- phase 1 ----------------
  for (int p = 0; p < nPass; p++) {
    const int m = p * 64 + lane;
    const bool act = m < nM;
    double w = 0, mx = 0, my = 0, sxx = 1, sxy = 0, syy = 1;
    if (act) { w = pW[m]; mx = pMX[m]; my = pMY[m]; sxx = pSXX[m]; sxy = pSXY[m]; syy = pSYY[m]; }
    LmKF k;
    double range;
    lm_precompute(P, pr, mx, my, sxx, sxy, syy, k, range);
    bool close;
    double pd = rb_pd(P, range, close);
    if (close) pd = 1;  // :604-606
    const bool fov = act && (pd != 0);
    const double pdw = pd * w;
    nFov += __popcll(__ballot(fov));
    if (P.useCluster) wsum += act ? w : 0.0;
    if (p == 0) DBG_T(0, 4);
    const unsigned long long cand = gate_candidates(P, k, fov && k.ok, nZ, sZf, G);
    if (p == 0) DBG_T(0, 5);
    // exact innovation gates + Mahalanobis gate + likelihood for the candidates
    unsigned long long surv = 0;
    double keepV[UPDMAP_KEEP];
#pragma unroll
    for (int t = 0; t < UPDMAP_KEEP; t++) keepV[t] = 0.0;
    int cnt = 0;
    // two loops, each as long as its busiest lane: the candidates of the fp32 sweep (a handful per landmark) through the exact
    // innovation gates and the Mahalanobis gate -- distance only --, then the few that are left (seldom more than one per landmark)
    // through the Gaussian: as one loop every trip paid for the exp and the division because SOME lane's candidate had passed
    unsigned long long gated = 0;
    for (unsigned long long g = cand; g; g &= g - 1) {
      const int z = __builtin_ctzll(g);
      const double z0 = sZ[2 * z], z1 = sZ[2 * z + 1];
      if (!pair_gate(P, k, z0, z1)) continue;
      if (pair_md2(k, z0, z1) > P.newGaussMd2) continue;
      gated |= 1ull << z;
    }
    for (unsigned long long g = gated; g; g &= g - 1) {
      const int z = __builtin_ctzll(g);
      const double z0 = sZ[2 * z], z1 = sZ[2 * z + 1];
      const double v = pair_value(P, k, pdw, z0, z1);
      if (v != 0.0) {
        surv |= (1ull << z);
#pragma unroll
        for (int t = 0; t < UPDMAP_KEEP; t++) keepV[t] = (cnt == t) ? v : keepV[t];
        cnt++;
      }
    }
    if (p == 0) DBG_T(0, 6);
    const int off = wave_excl_scan(cnt, lane);
    const int total = __builtin_amdgcn_readlane(off + cnt, 63);
    if (act) sSeg[m] = ((unsigned)(nSurv + off) << 8) | (unsigned)cnt;
    {
      int pos = nSurv + off, q = 0;
      for (unsigned long long g = surv; g; g &= g - 1, q++, pos++) {
        const int z = __builtin_ctzll(g);
        if (pos < room) {
          const double z0 = sZ[2 * z], z1 = sZ[2 * z + 1];
          double v = keepV[0];
#pragma unroll
          for (int t = 1; t < UPDMAP_KEEP; t++) v = (q == t) ? keepV[t] : v;
          if (q >= UPDMAP_KEEP) v = pair_value(P, k, pdw, z0, z1);
          sV[pos] = v;
          sMZ[pos] = ((unsigned)m << 8) | (unsigned)z;
          emit_updated(k, mx, my, z0, z1, pMX, pMY, pSXX, pSXY, pSYY, nM + pos);
        } else {
          overflow = true;
        }
      }
    }
    wave_sync();
    if (p == 0) DBG_T(0, 7);
    // lane z folds this pass's survivors of measurement z into its normaliser, in landmark order
    {
      const int lo = nSurv, hi = (nSurv + total < room) ? nSurv + total : room;
      int sIdx = lo;
      for (; sIdx + 4 <= hi; sIdx += 4) {  // broadcast reads, four in flight; the adds stay in list (= landmark) order
        const unsigned mz0 = sMZ[sIdx], mz1 = sMZ[sIdx + 1], mz2 = sMZ[sIdx + 2], mz3 = sMZ[sIdx + 3];
        const double v0 = sV[sIdx], v1 = sV[sIdx + 1], v2 = sV[sIdx + 2], v3 = sV[sIdx + 3];
        if ((int)(mz0 & 0xffu) == lane) cs += v0;
        if ((int)(mz1 & 0xffu) == lane) cs += v1;
        if ((int)(mz2 & 0xffu) == lane) cs += v2;
        if ((int)(mz3 & 0xffu) == lane) cs += v3;
      }
      for (; sIdx < hi; sIdx++) {
        const unsigned mz = sMZ[sIdx];
        const double v = sV[sIdx];
        if ((int)(mz & 0xffu) == lane) cs += v;
      }
    }
    nSurv += total;
    if (p == 0) DBG_T(0, 8);
  }
  DBG_T(0, 1);
  if (__ballot(overflow) != 0ull || nSurv > room) {
    if (lane == 0) atomicOr(B.err, ERRBIT_CAPACITY);
    nSurv = room < 0 ? 0 : (nSurv > room ? room : nSurv);
  }
  sCol[lane] = cs;
  wave_sync();

  // ---------------- phase 2: normalise, write the weights of the appended Gaussians ----------------
  unsigned long long used = 0;
  bool dropAny = false;
  for (int s0 = 0; s0 < nSurv; s0 += 64) {
    const int sIdx = s0 + lane;
    const bool act = sIdx < nSurv;
    double wn = 0.0;
    int z = 0;
    if (act) { z = (int)(sMZ[sIdx] & 0xffu); wn = sV[sIdx] / sCol[z]; sV[sIdx] = wn; }
    if (act && wn != 0.0) used |= (1ull << z);
    if (act) { pW[nM + sIdx] = wn; pWP[nM + sIdx] = 0.0; }  // addGaussian: weight_prev = 0 (GaussianMixture.hpp:267-284)
    dropAny |= act && !(wn > 0.0);  // :677
  }
  int outBase = nM + nSurv;
  if (__ballot(dropAny) != 0ull) {
    wave_sync();
    outBase = nM + compact_appended(sV, nM, nSurv, lane, pW, pWP, pMX, pMY, pSXX, pSXY, pSYY);
  }
  wave_sync();

  // ---------------- phase 3: missed-detection weights (:686-706); setWeight keeps the old weight in w_prev ----------------
  for (int m = lane; m < nM; m += 64) {
    const double w = pW[m];
    const double dx = pMX[m] - pr.x, dy = pMY[m] - pr.y;
    bool close;
    double pd = rb_pd(P, sqrt(dx * dx + dy * dy), close);
    if (close) pd = 1;
    double w_k = (1 - pd) * w;
    if (close && w > P.birthW) {
      const unsigned seg = sSeg[m];
      const int st = (int)(seg >> 8), c = (int)(seg & 0xffu);
      double rowsum = 0.0;
      for (int q = st; q < st + c && q < nSurv; q++) rowsum += sV[q];  // (already divided by the normaliser)
      const double delta_w = pd * w - rowsum;
      if (delta_w > 0) {
        w_k += delta_w;
        if (w_k > 1) w_k = 1;
      }
    }
    pWP[m] = w;
    pW[m] = w_k;
  }
  DBG_T(0, 2);
  used = wave_or_u64(used);
  if (lane == 0) {
    B.count[i] = outBase;
    B.unusedMask[i] = (~used) & zmask;  // :709-720
    B.nInFov[i] = nFov;
  }
  if (P.useCluster) {  // :570-580, :652-668
    const double s = RFS_DENORM_MIN + wave_sum_dpp(wsum);
    double prod = 1.0;
    for (int z = 0; z < nZ; z++) prod *= readlane_f64(cs, z);
    if (lane == 0) B.weight[i] = exp(s) * prod * B.weight[i];
  }
}

// Words of the survivor list's per-measurement bit table (workgroup form): one bit per list position.
__host__ __device__ inline int update_map_zpos_words(int cap) { return (cap + 31) >> 5; }
// LDS of the workgroup form below: the single-wave layout + cross-wave scratch + the bit table [words][MAX_Z].
__host__ __device__ inline size_t update_map_block_lds_bytes(int cap) {
  return update_map_lds_bytes_per_wave(cap) + 128 + (size_t)update_map_zpos_words(cap) * RFSGPU_MAX_Z * 4;
}

// The same map update by a workgroup of WPP waves (used inside the fused step kernel, where the particle's workgroup has
// more than one wave): passes cover WPP*64 landmarks; the survivor list keeps its (m, z) order through a cross-wave
// offset exchange, wave 0 folds the normalisers in list order (the reference's summation order) -- once, behind the passes,
// each lane finding its measurement's list positions in a bit table the emitting lanes fill --, phases 2 and 3 are
// split over all threads.  Bit-identical to phd_update_map_particle, which walks the list and is the reference for the table.
template <int WPP>
__device__ __forceinline__ void phd_update_map_block(const Buffers &B, const Params &P, const int cur, const int nZ, const int i, const int tid,
                                                     const unsigned char *smemZ, unsigned char *wb, const bool phasePrio = false) {
  constexpr int NT = WPP * 64;
  const double *sZ = reinterpret_cast<const double *>(smemZ);
  const float *sZf = reinterpret_cast<const float *>(smemZ + 2 * RFSGPU_MAX_Z * 8);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int cap = B.cap;
  double *sV = reinterpret_cast<double *>(wb);                 // [cap] survivor values Pd*w*lik, later the normalised weights
  double *sCol = sV + cap;                                      // [MAX_Z] final normalisers
  unsigned *sMZ = reinterpret_cast<unsigned *>(sCol + RFSGPU_MAX_Z);  // [cap] (m << 8) | z
  unsigned *sSeg = sMZ + cap;                                   // [cap] per landmark: (start << 8) | count
  unsigned char *gTab = wb + update_map_index_offset(cap);      // the measurement index of the gate prefilter (GATE_INDEX_BYTES)
  int *sTot = reinterpret_cast<int *>(wb + update_map_lds_bytes_per_wave(cap));  // [2][8] survivors per wave of a pass (double-buffered)
  int *sMisc = sTot + 16;                                       // [0] overflow flag [1] landmarks in FOV [2] a new Gaussian has to be dropped
  unsigned *sUsed = reinterpret_cast<unsigned *>(sMisc + 4);    // [2] used-measurement mask (lo, hi)
  // [words][MAX_Z] bit (pos & 31) of word pos >> 5, column z: list position pos holds a survivor of measurement z (word-major: the
  // words a particle can reach, those below `room`, are one contiguous block to clear, and lane z's reads of a word are conflict-free)
  unsigned *sZPos = reinterpret_cast<unsigned *>(wb + update_map_lds_bytes_per_wave(cap) + 128);

  const int nM = B.count[i];
  const unsigned long long zmask = (nZ >= 64) ? ~0ull : ((1ull << nZ) - 1ull);
  if (nM == 0) {  // :559-564
    if (tid == 0) {
      B.unusedMask[i] = zmask;
      B.nInFov[i] = 0;
    }
    return;
  }
  double *slab = B.slab[cur];
  double *pW = plane(slab, cap, i, PL_W), *pWP = plane(slab, cap, i, PL_WP);
  double *pMX = plane(slab, cap, i, PL_MX), *pMY = plane(slab, cap, i, PL_MY);
  double *pSXX = plane(slab, cap, i, PL_SXX), *pSXY = plane(slab, cap, i, PL_SXY), *pSYY = plane(slab, cap, i, PL_SYY);

  PoseReg pr;
  load_pose(B, P, i, pr);
  if (tid < 6) { if (tid < 4) sMisc[tid] = 0; else sUsed[tid - 4] = 0u; }
  {  // clear the bit table's words below `room` (no bit is set or read beyond); the first barrier of pass 0 stands before the first bit set
    const int nQuad = (cap - nM > 0) ? ((cap - nM + 31) >> 5) * (RFSGPU_MAX_Z / 4) : 0;
    uint4 *q = reinterpret_cast<uint4 *>(sZPos);
    for (int j = tid; j < nQuad; j += NT) q[j] = make_uint4(0u, 0u, 0u, 0u);
  }
  // the measurement index, once per workgroup: wave 0 bins the bearings, wave 1 the ranges
  if (P.gateIndex) {
    if (wave == 0) gate_index_build_bearing(gTab, sZf, nZ, lane);
    if (wave == (WPP > 1 ? 1 : 0)) gate_index_build_range(gTab, sZf, nZ, lane);
    __syncthreads();
  }
  const GateIndex G = gate_index_load(P, gTab, sZf);

  const int nPass = (nM + NT - 1) / NT;
  const int room = cap - nM;  // survivors that still fit as new Gaussians
  int nFov = 0;
  double cs = P.clutter;       // wave 0, lane z: normaliser of measurement z (reference: sum = clutter; sum += W[m][z] ...)
  int nSurv = 0;
  bool overflow = false;

  // (step_fused.h: issue priority falls from phase to phase; raised here rather than at the kernel's first instruction,
  //  where the scheduling barrier it forms made the register allocator spill 84 B per lane)
  //  Inside this phase, where all workgroups of a CU start together, the waves in the last hardware slot of their SIMD
  //  (HW_ID.wave_id: the last arrivals, which the arbiter ranks lowest) get the level above the others.
#ifndef STEP_MAP_PRIO
#define STEP_MAP_PRIO 2
#endif
  if (phasePrio) { if ((__builtin_amdgcn_s_getreg((4 - 1) << 11 | 4) & 0xfu) >= 3u) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(STEP_MAP_PRIO); }
  // ---------------- phase 1 ----------------
  for (int p = 0; p < nPass; p++) {
    const int m = p * NT + tid;
    const bool act = m < nM;
    double w = 0, mx = 0, my = 0, sxx = 1, sxy = 0, syy = 1;
    if (act) { w = pW[m]; mx = pMX[m]; my = pMY[m]; sxx = pSXX[m]; sxy = pSXY[m]; syy = pSYY[m]; }
    LmKF k;
    double range;
    lm_precompute(P, pr, mx, my, sxx, sxy, syy, k, range);
    bool close;
    double pd = rb_pd(P, range, close);
    if (close) pd = 1;  // :604-606
    const bool fov = act && (pd != 0);
    const double pdw = pd * w;
    nFov += __popcll(__ballot(fov));
    RFS_CUT(1);
    const unsigned long long cand = gate_candidates(P, k, fov && k.ok, nZ, sZf, G);
    RFS_CUT(2);
    unsigned long long surv = 0;
    double keepV[UPDMAP_KEEP];
#pragma unroll
    for (int t = 0; t < UPDMAP_KEEP; t++) keepV[t] = 0.0;
    int cnt = 0;
    // two loops, each as long as its busiest lane: the candidates of the fp32 sweep (a handful per landmark) through the exact
    // innovation gates and the Mahalanobis gate -- distance only --, then the few that are left (seldom more than one per landmark)
    // through the Gaussian: as one loop every trip paid for the exp and the division because SOME lane's candidate had passed
    unsigned long long gated = 0;
    for (unsigned long long g = cand; g; g &= g - 1) {
      const int z = __builtin_ctzll(g);
      const double z0 = sZ[2 * z], z1 = sZ[2 * z + 1];
      if (!pair_gate(P, k, z0, z1)) continue;
      if (pair_md2(k, z0, z1) > P.newGaussMd2) continue;
      gated |= 1ull << z;
    }
    for (unsigned long long g = gated; g; g &= g - 1) {
      const int z = __builtin_ctzll(g);
      const double z0 = sZ[2 * z], z1 = sZ[2 * z + 1];
      const double v = pair_value(P, k, pdw, z0, z1);
      if (v != 0.0) {
        surv |= (1ull << z);
#pragma unroll
        for (int t = 0; t < UPDMAP_KEEP; t++) keepV[t] = (cnt == t) ? v : keepV[t];
        cnt++;
      }
    }
    RFS_CUT(3);
    const int off = wave_excl_scan(cnt, lane);
    const int totalW = __builtin_amdgcn_readlane(off + cnt, 63);
    int *tot = sTot + 8 * (p & 1);
    if (lane == 0) tot[wave] = totalW;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w2 = 0; w2 < WPP; w2++) { const int t = tot[w2]; before += (w2 < wave) ? t : 0; total += t; }
    if (act) sSeg[m] = ((unsigned)(nSurv + before + off) << 8) | (unsigned)cnt;
    {
      int pos = nSurv + before + off, q = 0;
      for (unsigned long long g = surv; g; g &= g - 1, q++, pos++) {
        const int z = __builtin_ctzll(g);
        if (pos < room) {
          const double z0 = sZ[2 * z], z1 = sZ[2 * z + 1];
          double v = keepV[0];
#pragma unroll
          for (int t = 1; t < UPDMAP_KEEP; t++) v = (q == t) ? keepV[t] : v;
          if (q >= UPDMAP_KEEP) v = pair_value(P, k, pdw, z0, z1);
          sV[pos] = v;
          sMZ[pos] = ((unsigned)m << 8) | (unsigned)z;
          __hip_atomic_fetch_or(&sZPos[(pos >> 5) * RFSGPU_MAX_Z + z], 1u << (pos & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          emit_updated(k, mx, my, z0, z1, pMX, pMY, pSXX, pSXY, pSYY, nM + pos);
        } else {
          overflow = true;
        }
      }
    }
    // No barrier at the end of a pass: what it writes (sSeg, sV, sMZ, table bits -- every list position and landmark once) is read
    // only behind the barrier that follows the loop, and sTot alternates between two buffers -- a wave overwrites tot[p & 1] in pass
    // p + 2, behind the barrier of pass p + 1, which every wave reaches only after its reads of pass p.
    RFS_CUT(4);
    nSurv += total;
  }
  RFS_CUT(6);
  if (__ballot(overflow) != 0ull && lane == 0) atomicOr(&sMisc[0], 1);
  if (lane == 0) atomicAdd(&sMisc[1], nFov);
  __syncthreads();
  // lane z of wave 0 folds the survivors of measurement z into its normaliser, once, in list (= landmark) order: its column of the
  // bit table names their positions, so it reads the handful that are its own instead of walking the whole list
  if (wave == 0 && lane < nZ) {
    const int nList = nSurv < room ? nSurv : room;   // (bits exist below this only)
    const int nWord = (nList + 31) >> 5;
    for (int w = 0; w < nWord; w++)
      for (unsigned bits = sZPos[w * RFSGPU_MAX_Z + lane]; bits; bits &= bits - 1) cs += sV[32 * w + __builtin_ctz(bits)];
  }
  if (wave == 0) sCol[lane] = cs;
  RFS_CUT(5);   // (behind the store: a cut in front of it leaves the sums dead, and the compiler drops the fold from the cut build)
  __syncthreads();
  if (sMisc[0] != 0 || nSurv > room) {
    if (tid == 0) atomicOr(B.err, ERRBIT_CAPACITY);
    nSurv = room < 0 ? 0 : (nSurv > room ? room : nSurv);
  }

  // ---------------- phase 2: normalise in place, write the weights of the appended Gaussians ----------------
  {
    unsigned long long used = 0;
    bool dropAny = false;
    for (int s0 = wave * 64; s0 < nSurv; s0 += NT) {
      const int sIdx = s0 + lane;
      const bool act = sIdx < nSurv;
      double wn = 0.0;
      int z = 0;
      if (act) { z = (int)(sMZ[sIdx] & 0xffu); wn = sV[sIdx] / sCol[z]; sV[sIdx] = wn; }
      if (act && wn != 0.0) used |= (1ull << z);
      if (act) { pW[nM + sIdx] = wn; pWP[nM + sIdx] = 0.0; }  // addGaussian: weight_prev = 0 (GaussianMixture.hpp:267-284)
      dropAny |= act && !(wn > 0.0);  // :677
    }
    used = wave_or_u64(used);
    if (lane == 0) { atomicOr(&sUsed[0], (unsigned)(used & 0xffffffffull)); atomicOr(&sUsed[1], (unsigned)(used >> 32)); }
    if (__ballot(dropAny) != 0ull && lane == 0) atomicOr(&sMisc[2], 1);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  int outBase = nM + nSurv;
  if (sMisc[2] != 0) {  // rare: a normalised weight that is not positive (inf / NaN arithmetic) -- drop it, keep the order
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (wave == 0) {
      const int kept = compact_appended(sV, nM, nSurv, lane, pW, pWP, pMX, pMY, pSXX, pSXY, pSYY);
      if (lane == 0) sMisc[3] = kept;
    }
    __syncthreads();
    outBase = nM + sMisc[3];
  }

  RFS_CUT(7);
  // ---------------- phase 3: missed-detection weights (:686-706); setWeight keeps the old weight in w_prev ----------------
  for (int m = tid; m < nM; m += NT) {
    const double w = pW[m];
    const double dx = pMX[m] - pr.x, dy = pMY[m] - pr.y;
    bool close;
    double pd = rb_pd(P, sqrt(dx * dx + dy * dy), close);
    if (close) pd = 1;
    double w_k = (1 - pd) * w;
    if (close && w > P.birthW) {
      const unsigned seg = sSeg[m];
      const int st = (int)(seg >> 8), c = (int)(seg & 0xffu);
      double rowsum = 0.0;
      for (int q = st; q < st + c && q < nSurv; q++) rowsum += sV[q];  // (already divided by the normaliser)
      const double delta_w = pd * w - rowsum;
      if (delta_w > 0) {
        w_k += delta_w;
        if (w_k > 1) w_k = 1;
      }
    }
    pWP[m] = w;
    pW[m] = w_k;
  }
  if (tid == 0) {
    B.count[i] = outBase;
    const unsigned long long used = (unsigned long long)sUsed[0] | ((unsigned long long)sUsed[1] << 32);
    B.unusedMask[i] = (~used) & zmask;  // :709-720
    B.nInFov[i] = sMisc[1];
  }
  if (P.useCluster) __syncthreads();  // (phase 3 left the prior weights in w_prev)
  if (P.useCluster && wave == 0) {  // :570-580, :652-668 -- sum of the prior weights in the single-wave order
    double wsum = 0.0;
    for (int m = lane; m < nM; m += 64) wsum += pWP[m];
    const double s2 = RFS_DENORM_MIN + wave_sum_dpp(wsum);
    double prod = 1.0;
    for (int z = 0; z < nZ; z++) prod *= readlane_f64(cs, z);
    if (lane == 0) B.weight[i] = exp(s2) * prod * B.weight[i];
  }
}

template <int WPB>
__global__ __launch_bounds__(WPB * 64) __attribute__((amdgpu_waves_per_eu(UPDMAP_WAVES_PER_EU, UPDMAP_WAVES_PER_EU))) void phd_update_map_kernel(Buffers B, Params P, int cur, int nZ, const double *__restrict__ Zg) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  stage_measurements_lds(smem_raw, [&](int t) { return Zg[t]; }, nZ, (int)threadIdx.x, WPB * 64);
  __syncthreads();
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + wave);
  if (i >= B.N) return;
  phd_update_map_particle(B, P, cur, nZ, i, lane, smem_raw, smem_raw + RFS_Z_LDS_BYTES + (size_t)wave * update_map_lds_bytes_per_wave(B.cap));
}

// The stand-alone kernel in the workgroup form: WPP waves per particle (phd_update_map_block, bit-identical to the single-wave
// routine).  One wave per particle leaves a 2000-particle launch at two waves per SIMD; with two waves per particle the phase
// hides its latencies as it does inside the fused step.
template <int WPP>
__global__ __launch_bounds__(WPP * 64) __attribute__((amdgpu_waves_per_eu(UPDMAP_WAVES_PER_EU, 4))) void phd_update_map_block_kernel(Buffers B, Params P, int cur, int nZ, const double *__restrict__ Zg) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  stage_measurements_lds(smem_raw, [&](int t) { return Zg[t]; }, nZ, (int)threadIdx.x, WPP * 64);
  __syncthreads();
  phd_update_map_block<WPP>(B, P, cur, nZ, (int)blockIdx.x, (int)threadIdx.x, smem_raw, smem_raw + RFS_Z_LDS_BYTES);
}

