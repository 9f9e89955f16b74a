// estimate_log.h -- what each filter ESTIMATED at a step, kept on the device (rfsgpu.h [estimate]): the reference's simulators write
// particlePose.dat and landmarkEst.dat per time step (src/rbphdslam2dSim.cpp:620-638, src/fastslam2dSim.cpp:613-632); this kernel writes
// the same content into a row of a device-side log, for an ordinary 2-D handle (one filter) or every filter of a batch, in ONE launch
// that reads weights, poses, counts and the current slab as they are at its point of the stream and changes nothing of them.
//
// Grid (nF, 1 + ceil(slots / 256)), 64 lanes per workgroup (one wave: wave-synchronous, no barrier, no LDS):
//   blockIdx.y == 0 -- the header and the Gaussians of filter blockIdx.x.  The SELECTION is map_metric_kernel's steps 1 and 2,
//     restated: lane l scans slots l, l + 64, ... of the block in ascending order for the first weight strictly greater than
//     everything before it, starting from 0; the 64 candidates meet in an xor butterfly that prefers the larger weight, then the lower
//     slot; no weight > 0 (all zero, negative or NaN): the block's slot 0.  The sums (weights, w x, w y, w cos theta, w sin theta, the
//     cardinality) run over the metric's FIXED TREE: every lane adds its own entries in ascending order, then wave_sum's butterfly
//     (32, 16, ..., 1) -- so weight_sum and cardinality carry the bits rfsgpu_step_error reports.  The PREDICATE is the metric's step 3:
//     entries beyond the count do not exist, log-odds become 1 - 1 / (1 + exp(w)), holes (w < 0) are skipped, w >= w_threshold keeps, and
//     a ballot prefix per 64 entries gives each kept Gaussian its position in mixture order.  Where the metric fills LDS tables, this
//     kernel stores the six planes (mx, my, sxx, sxy, syy, w) to global memory for positions < max_est: the lanes of one ballot round
//     hold consecutive positions, so each plane's stores are consecutive doubles.
//   blockIdx.y >= 1 -- the particle planes (x, y, theta, w) of slots [256 (y - 1), 256 y) of the filter, four slots per lane at a
//     stride of 64: they need nothing from the selection.  Launched only when the log keeps particles.
//
// live: nothing, or a MetricLive (map_metric.h) for a batch of multi-hypothesis FastSLAM filters: the wave reads the filter's live
// count once (a scalar read), clamps it to [0, stride], and no slot at or beyond it is read -- by either kind of workgroup.  A count of
// 0 reads nothing of the block at all: best_slot is the block's first slot, n_est and cardinality are 0, pose and mean fields NaN.
//
// An EstimateHandle as the trailing argument: an ordinary handle that rfsgpu_handle_serve_estimates serves -- the same code in the same
// order with the layout as a compile-time parameter, and behind pending FastSLAM cycles the live count and the overflow word of the
// handle's cycle block read where the kernel runs (status 2 and a count of 0 once a cycle overflowed).  The instantiations without one
// compile to what they compiled to before it existed.
//
// An EstimateBatch<3> as the trailing argument: a batch of Victoria Park filters that rfsgpu_batch_vp_serve_estimates serves -- the 3-D
// layout of the handle form with the batch's b = blockIdx.x and lo = b * nPer, the count the host's n_per_filter.  Code and order are
// those of the handle form, so a filter's row carries the bits a served handle holding the same state produces.
//
// Bounds: a Gaussian is stored at pos < maxEst <= cap (the engine checks max_est against gm_capacity), a particle at s < nLive <=
// nPer <= slots (the stride the part array was allocated with; a served handle: s < n_live <= max_particles <= slots); nothing else is
// written but lane 0's header.
#pragma once

struct EstimateArg {
  const double *in;        // the call's times: filter b's at in[inStride * b] (a slot of the pinned staging ring read in place, stride 1; or a
  int inStride;            //  row of the truth tables on the device, {t, x, y, theta} per filter: stride 4)
  struct rfsgpu_step_estimate *hdr;   // [nF] the row's headers
  double *gauss;           // [nF][6][maxEst] the row's Gaussian planes (nullptr with maxEst 0)
  double *part;            // [nF][4][slots] the row's particle planes (nullptr: not kept)
  double wThr;
  int nPer;                // particles per filter (a multi-hypothesis batch: the stride)
  int slots;               // the part array's slots per plane (>= nPer)
  int maxEst;
  int holes;               // merged-away entries (w < 0) sit in the slab: skip them
  int logOdds;             // FastSLAM kinds: a Gaussian's weight is the log-odds of existence
};

#define ESTIMATE_PART_SLOTS 256   // slots per particle-plane workgroup

// The trailing argument of an ordinary handle that rfsgpu_handle_serve_estimates serves (one filter, b = 0).  D: the slab layout the
// Gaussians are read from -- 2: the planes of common.h; 3: the Victoria Park planes of vp.h (Plane3), of which the row keeps u(0), u(1),
// S(0,0), S(0,1), S(1,1) and w, what the reference's Victoria Park drivers print (the diameter and its covariances are not logged).
// kBehind: the launch stands behind pending FastSLAM cycles (fastslam_cycle.h) -- n and ovf are the count and the overflow word of
// the handle's cycle block; otherwise neither is read and the count is the host's, A.nPer.
template <int D, bool kBehind>
struct EstimateHandle {
  const int *n;     // [1] live particle count (FSC_N)
  const int *ovf;   // [1] != 0: a pending cycle overflowed max_particles and was abandoned (FSC_OVF)
};
// The trailing tag of a filter batch whose slabs have the layout D (3: a batch of Victoria Park filters): every filter fills its block,
// nothing is read through it.
template <int D>
struct EstimateBatch {};
template <typename... T> struct estimate_traits { static constexpr int D = 2; static constexpr bool handle = false, behind = false, live = sizeof...(T) == 1; };
template <int D_, bool kBehind> struct estimate_traits<EstimateHandle<D_, kBehind>> { static constexpr int D = D_; static constexpr bool handle = true, behind = kBehind, live = false; };
template <int D_> struct estimate_traits<EstimateBatch<D_>> { static constexpr int D = D_; static constexpr bool handle = false, behind = false, live = false; };

template <typename... TLive>
__global__ __launch_bounds__(64) void estimate_log_kernel(Buffers B, int cur, EstimateArg A, TLive... live) {
  using TR = estimate_traits<TLive...>;
  constexpr int NPL = TR::D == 3 ? (int)P3_COUNT : (int)PL_COUNT, KW = TR::D == 3 ? (int)P3_W : (int)PL_W;
  constexpr int KMX = TR::D == 3 ? (int)P3_MX : (int)PL_MX, KMY = TR::D == 3 ? (int)P3_MY : (int)PL_MY;
  constexpr int KSXX = TR::D == 3 ? (int)P3_SXX : (int)PL_SXX, KSXY = TR::D == 3 ? (int)P3_SXY : (int)PL_SXY, KSYY = TR::D == 3 ? (int)P3_SYY : (int)PL_SYY;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nPer = A.nPer, lo = b * nPer;
  int nLive = nPer;
  [[maybe_unused]] int ovf = 0;
  if constexpr (TR::handle) {              // a served handle: the host's count, or -- behind FastSLAM cycles -- MetricLive's form with b = 0
    if constexpr (TR::behind) {            // and the overflow word beside it: once set, the host's `cur` is ahead of the device and the
      const auto &L = pack_first(live...); // row is that of a count of 0 -- nothing of the filter state is read
      ovf = __builtin_amdgcn_readfirstlane(*L.ovf);
      nLive = __builtin_amdgcn_readfirstlane(*L.n);
      nLive = (ovf != 0 || nLive < 0) ? 0 : (nLive > nPer ? nPer : nLive);
    }
  } else if constexpr (TR::live) {   // a MetricLive: the filter's count lives on the device (wave-uniform: one scalar read)
    const MetricLive &L = pack_first(live...);
    nLive = __builtin_amdgcn_readfirstlane(L.words[(size_t)b * L.wordStride + L.word]);
    nLive = nLive < 0 ? 0 : (nLive > nPer ? nPer : nLive);
  }

  if (blockIdx.y >= 1) {   // ---- the particle planes: a plain copy of the live slots -----------------------------------------------
    if (!A.part) return;
    double *px = A.part + (size_t)b * 4 * A.slots, *py = px + A.slots, *pth = py + A.slots, *pwt = pth + A.slots;
    const int s0 = ((int)blockIdx.y - 1) * ESTIMATE_PART_SLOTS;
#pragma unroll
    for (int q = 0; q < ESTIMATE_PART_SLOTS / 64; q++) {
      const int s = s0 + q * 64 + lane;
      if (s < nLive) {
        const double *x = B.pose + (size_t)3 * (lo + s);
        px[s] = x[0]; py[s] = x[1]; pth[s] = x[2]; pwt[s] = B.weight[lo + s];
      }
    }
    return;
  }

  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double t = A.in[(size_t)A.inStride * b];

  // ---- 1 + 2 of map_metric_kernel: highest-weight particle, weight sum, the weighted pose sums ------------------------------------
  double bw = 0.0, sw = 0.0, sx = 0.0, sy = 0.0, sc = 0.0, ss = 0.0;
  int bi = -1;
  for (int s = lane; s < nLive; s += 64) {
    const double w = B.weight[lo + s];
    if (w > bw) { bw = w; bi = s; }
    sw += w;
    const double *x = B.pose + (size_t)3 * (lo + s);
    double sn, cs;
    sincos(x[2], &sn, &cs);
    sx += x[0] * w; sy += x[1] * w; sc += cs * w; ss += sn * w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ow = __shfl_xor(bw, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (ow > bw || (ow == bw && (bi < 0 || oi < bi)))) { bw = ow; bi = oi; }
  }
  const int best = lo + (bi < 0 ? 0 : bi);
  sw = wave_sum(sw);
  sx = wave_sum(sx) / sw; sy = wave_sum(sy) / sw; sc = wave_sum(sc) / sw; ss = wave_sum(ss) / sw;

  // ---- 3 of map_metric_kernel: the best particle's Gaussians, compacted in mixture order, straight to the row's planes -------------
  double card = 0.0, bestW = 0.0, bx = qnan, by = qnan, bth = qnan;
  int n1 = 0;
  if (nLive > 0) {
    int cnt = B.count[best];
    cnt = cnt < 0 ? 0 : (cnt > B.cap ? B.cap : cnt);
    const double *pl = B.slab[cur] + (size_t)best * NPL * (size_t)B.cap;
    const double *pw = pl + (size_t)KW * B.cap, *pmx = pl + (size_t)KMX * B.cap, *pmy = pl + (size_t)KMY * B.cap;
    const double *pxx = pl + (size_t)KSXX * B.cap, *pxy = pl + (size_t)KSXY * B.cap, *pyy = pl + (size_t)KSYY * B.cap;
    const size_t me = (size_t)A.maxEst;
    double *g = A.gauss + (size_t)b * 6 * me;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < cnt; base += 64) {
      const int m = base + lane;
      bool valid = m < cnt;
      double w = valid ? pw[m] : 0.0;
      if (A.logOdds) w = valid ? 1 - 1 / (1 + exp(w)) : 0.0;
      if (A.holes && w < 0) valid = false;
      if (valid) card += w;
      const bool keep = valid && w >= A.wThr;
      const unsigned long long mask = __ballot(keep);
      const int pos = n1 + __popcll(mask & below);
      if (keep && pos < A.maxEst) {
        g[pos] = pmx[m]; g[me + pos] = pmy[m]; g[2 * me + pos] = pxx[m]; g[3 * me + pos] = pxy[m]; g[4 * me + pos] = pyy[m]; g[5 * me + pos] = w;
      }
      n1 += __popcll(mask);
    }
    card = wave_sum(card);
    const double *x = B.pose + (size_t)3 * best;
    bestW = B.weight[best]; bx = x[0]; by = x[1]; bth = x[2];
  } else {
    sx = sy = sc = ss = qnan;
  }
  if (lane == 0) {
    struct rfsgpu_step_estimate &o = A.hdr[b];
    o.t = t; o.status = n1 > A.maxEst ? 1 : 0; o.best_slot = best; o.n_particles = nLive; o.n_est = n1; o.n_logged = n1 < A.maxEst ? n1 : A.maxEst;
    o.cardinality = card; o.best_weight = bestW; o.weight_sum = sw;
    o.best_x = bx; o.best_y = by; o.best_theta = bth;
    o.mean_x = sx; o.mean_y = sy; o.mean_cos = sc; o.mean_sin = ss;
    if constexpr (TR::behind) { if (ovf != 0) o.status = 2; }
  }
}
