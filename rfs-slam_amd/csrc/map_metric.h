// map_metric.h -- per-step evaluation on the device (rfsgpu.h [metric]): what the reference's analysis2dSim writes per time step
// (src/analysis2dSim.cpp:150-249) -- the weighted-mean pose error of the particle set and the OSPA / COLA map error
// (include/OSPA.hpp:122-203, include/COLA.hpp:91-98) of the highest-weight particle -- as ONE launch for an ordinary 2-D handle
// (one filter) or for every filter of a batch.  The kernel reads weights, poses, counts and the current slab as they are at its
// point of the stream and writes nothing but one rfsgpu_step_error record per filter.
//
// One workgroup of ONE wave (64 lanes) per filter: everything below is wave-synchronous (wave_sync(), no hardware barrier).
//   1. highest-weight particle: lane l scans slots l, l + 64, ... of the filter's block in ascending order for the first weight
//      strictly greater than everything before it, starting from 0 (:159-167); the 64 candidates meet in an xor butterfly that
//      prefers the larger weight and, among equal weights, the lower slot -- the first slot holding the block's maximum, as the
//      reference's serial scan finds it.  No weight > 0 (all zero, negative or NaN): slot 0 of the block.
//   2. pose error: the five sums (w, w ex, w ey, w wrap(eth), w hypot(ex, ey)) are taken over a FIXED TREE: every lane adds its
//      slots l, l + 64, ... in ascending order, then the 64 partial sums are added in wave_sum's xor butterfly (32, 16, ..., 1).
//      The same tree adds the cardinality (lanes over the mixture's entries) and the OSPA sums (lanes over the assignment's rows).
//   3. the estimate (Gaussians with w >= w_threshold, mixture order) and the observable ground truth (first_seen <= t) are
//      compacted into LDS with a ballot prefix per 64 entries.
//   4. the assignment: a shortest-augmenting-path solver (Jonker-Volgenant form: one Dijkstra search per row over reduced costs,
//      dual update, augmentation), minimising the sum of C over the n x n padded square, n = max(n_est, n_truth) <= 512.  No table
//      exists anywhere: cell (i, j) = min(|e_i - g_j|, c) for i < n_est and j < n_truth, else c, is recomputed from the two
//      coordinates wherever a search needs it.  Lanes over columns (column j belongs to lane j & 63, up to 8 per lane; each lane keeps
//      the "column scanned" flags of its own columns in one register), one wave-wide arg-min per search step (a DPP minimum of the
//      64 lane minima, then a ballot: among equal values a column without a row wins, then the lowest lane), so a search step at
//      n <= 64 is one cost cell per lane.  Only the optimum's VALUE is the metric's (as with deviation 11 of DESIGN 4): which of
//      several optimal assignments comes out is this solver's own business.  The structure of the problem (padded rows / columns
//      and pairs further apart than c all cost exactly c) is NOT exploited: every row runs the same search.
//
// LDS per workgroup: both point sets (4 x 512 doubles), the dual variables u, v and the per-column path cost (3 x 512 doubles), the
// per-column predecessor and the two match arrays (3 x 512 ints): 28 672 + 6 144 = 34 816 bytes (34 KB) -- four filters per CU.
//
// A filter whose n_est or n_truth exceeds RFSGPU_MAX_METRIC_SET gets status 1 and NaN metrics (its n_est / n_truth / cardinality /
// pose fields are still filled); nothing beyond entry 511 of any LDS array is ever addressed.  Status 2: the search met no finite
// reduced cost (non-finite coordinates): NaN metrics as well.
//
// live: nothing, or a MetricLive for a batch of multi-hypothesis FastSLAM filters (rfsgpu_create_batch_mh), where filter b owns A.nPer
// slots (the stride) of which only the first n_b are live and n_b is a word of the filter's cycle state on the device
// (fastslam_cycle.h).  The wave reads that word once, as it is at the kernel's point of the stream (a scalar read), clamps it to
// [0, stride], and steps 1 and 2 run to it: no slot at or beyond the count is read (weight, pose, count or slab -- they hold whatever
// a larger set left there).  Lane l adds the slots l, l + 64, ... < n_b, so a filter of n_b live slots sums in the tree of a full
// block of n_b.  Steps 3 and 4 are the same code.
#pragma once

#define METRIC_MAXS RFSGPU_MAX_METRIC_SET

struct MetricArg {
  const double *in;        // [nF][4] {t, rx, ry, rtheta} of this call (a slot of the pinned staging ring, read in place)
  const double *gtXY;      // [nF][METRIC_MAXS][2] ground-truth landmarks (nullptr: none uploaded on this handle)
  const double *gtSeen;    // [nF][METRIC_MAXS] first_seen
  const int *gtN;          // [nF]
  struct rfsgpu_step_error *out;  // [nF] the row to write
  double wThr, cutoff, order;
  int nPer;                // particles per filter
  int havePose;            // 0: pose fields NaN
  int holes;               // merged-away entries (w < 0) sit in the slab: skip them
  int logOdds;             // a FastSLAM batch: a Gaussian's weight is the log-odds of existence; the estimate's weight is 1 - 1 / (1 + exp(w))
};

struct MetricLive {
  const int *words;        // filter 0's cycle words; filter b's start wordStride ints further (as MhBatchArg, fastslam.h)
  int wordStride;
  int word;                // which word is the live count (FSC_N)
};

// (wave_min_f64: hungarian_wave.h -- DPP moves, the result in every lane)
__device__ __forceinline__ double metric_pow(double x, double p) { return p == 1.0 ? x : (p == 2.0 ? x * x : pow(x, p)); }

template <typename... TLive>
__global__ __launch_bounds__(64) void map_metric_kernel(Buffers B, int cur, MetricArg A, TLive... live) {
  __shared__ double sEx[METRIC_MAXS], sEy[METRIC_MAXS], sGx[METRIC_MAXS], sGy[METRIC_MAXS];
  __shared__ double sU[METRIC_MAXS], sV[METRIC_MAXS], sSpc[METRIC_MAXS];
  __shared__ int sPath[METRIC_MAXS], sRow4Col[METRIC_MAXS], sCol4Row[METRIC_MAXS];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nPer = A.nPer, lo = b * nPer;
  int nLive = nPer;
  if constexpr (sizeof...(TLive) == 1) {   // a MetricLive: the filter's count lives on the device (wave-uniform: one scalar read)
    const MetricLive &L = pack_first(live...);
    nLive = __builtin_amdgcn_readfirstlane(L.words[(size_t)b * L.wordStride + L.word]);
    nLive = nLive < 0 ? 0 : (nLive > nPer ? nPer : nLive);
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double t = A.in[4 * b], rx = A.in[4 * b + 1], ry = A.in[4 * b + 2], rth = A.in[4 * b + 3];

  // ---- 1 + 2: highest-weight particle, weight sum, pose error -------------------------------------------------------------------
  double bw = 0.0, sw = 0.0, sx = 0.0, sy = 0.0, sth = 0.0, sd = 0.0;
  int bi = -1;
  for (int s = lane; s < nLive; s += 64) {
    const double w = B.weight[lo + s];
    if (w > bw) { bw = w; bi = s; }
    sw += w;
    if (A.havePose) {
      const double *x = B.pose + (size_t)3 * (lo + s);
      const double ex = x[0] - rx, ey = x[1] - ry;
      double eth = x[2] - rth;
      if (eth > M_PI) eth -= 2 * M_PI;
      else if (eth < -M_PI) eth += 2 * M_PI;
      sx += ex * w; sy += ey * w; sth += eth * w; sd += hypot(ex, ey) * w;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ow = __shfl_xor(bw, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (ow > bw || (ow == bw && (bi < 0 || oi < bi)))) { bw = ow; bi = oi; }
  }
  const int best = lo + (bi < 0 ? 0 : bi);
  sw = wave_sum(sw);
  if (A.havePose) { sx = wave_sum(sx) / sw; sy = wave_sum(sy) / sw; sth = wave_sum(sth) / sw; sd = wave_sum(sd) / sw; }
  else sx = sy = sth = sd = qnan;

  // ---- 3: the estimate of that particle, its cardinality, the observable ground truth ---------------------------------------------
  int cnt = B.count[best];
  cnt = cnt < 0 ? 0 : (cnt > B.cap ? B.cap : cnt);
  const double *pw = B.slab[cur] + ((size_t)best * PL_COUNT + PL_W) * (size_t)B.cap;
  const double *pmx = B.slab[cur] + ((size_t)best * PL_COUNT + PL_MX) * (size_t)B.cap;
  const double *pmy = B.slab[cur] + ((size_t)best * PL_COUNT + PL_MY) * (size_t)B.cap;
  const unsigned long long below = (1ull << lane) - 1ull;
  double card = 0.0;
  int n1 = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int m = base + lane;
    bool valid = m < cnt;
    double w = valid ? pw[m] : 0.0;
    if (A.logOdds) w = valid ? 1 - 1 / (1 + exp(w)) : 0.0;   // what fastslam2dSim.cpp:628 logs and analysis2dSim thresholds
    if (A.holes && w < 0) valid = false;
    if (valid) card += w;
    const bool keep = valid && w >= A.wThr;
    const unsigned long long mask = __ballot(keep);
    const int pos = n1 + __popcll(mask & below);
    if (keep && pos < METRIC_MAXS) { sEx[pos] = pmx[m]; sEy[pos] = pmy[m]; }
    n1 += __popcll(mask);
  }
  card = wave_sum(card);
  int n2 = 0;
  {
    int gn = A.gtN ? A.gtN[b] : 0;
    gn = gn < 0 ? 0 : (gn > METRIC_MAXS ? METRIC_MAXS : gn);
    const double *gxy = A.gtXY + (size_t)b * METRIC_MAXS * 2;
    const double *gs = A.gtSeen + (size_t)b * METRIC_MAXS;
    for (int base = 0; base < gn; base += 64) {
      const int m = base + lane;
      const bool keep = m < gn && gs[m] <= t;
      const unsigned long long mask = __ballot(keep);
      const int pos = n2 + __popcll(mask & below);
      if (keep) { sGx[pos] = gxy[2 * m]; sGy[pos] = gxy[2 * m + 1]; }   // (pos < gn <= METRIC_MAXS)
      n2 += __popcll(mask);
    }
  }
  const int n = n1 > n2 ? n1 : n2;
  const double c = A.cutoff, p = A.order;
  int status = (n1 > METRIC_MAXS || n2 > METRIC_MAXS) ? 1 : 0;
  double ospa = 0.0, cola = 0.0, eDist = 0.0, eCard = 0.0;

  // ---- 4: the assignment (rows: estimates + padding, columns: ground truth + padding) ----------------------------------------------
  if (status == 0 && n > 0) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int j = lane; j < n; j += 64) { sU[j] = 0.0; sV[j] = 0.0; sRow4Col[j] = -1; sCol4Row[j] = -1; }
    wave_sync();
    for (int curRow = 0; curRow < n && status == 0; curRow++) {
      for (int j = lane; j < n; j += 64) sSpc[j] = inf;
      unsigned scanned = 0;          // bit k: this lane's column lane + 64 k is in the search tree
      int i = curRow, sink = -1;
      double minVal = 0.0;
      for (int it = 0; it < n && sink < 0; it++) {
        const bool realRow = i < n1;
        const double ui = sU[i], xi = realRow ? sEx[i] : 0.0, yi = realRow ? sEy[i] : 0.0;
        double bv = inf;
        int bj = -1;
        bool bfree = false;
        for (int j = lane, k = 0; j < n; j += 64, k++) {
          if (scanned & (1u << k)) continue;
          double cij = c;
          if (realRow && j < n2) {
            const double dx = xi - sGx[j], dy = yi - sGy[j];
            cij = fmin(sqrt(dx * dx + dy * dy), c);
          }
          const double r = minVal + cij - ui - sV[j];
          double s = sSpc[j];
          if (r < s) { s = r; sSpc[j] = r; sPath[j] = i; }
          const bool fr = sRow4Col[j] < 0;
          if (s < bv || (s == bv && fr && !bfree)) { bv = s; bj = j; bfree = fr; }
        }
        const double m = wave_min_f64(bv);
        if (!(m < inf)) { status = 2; break; }
        unsigned long long win = __ballot(bv == m && bfree);
        if (!win) win = __ballot(bv == m);
        const int wl = __ffsll((long long)win) - 1;
        const int j = __builtin_amdgcn_readlane(bj, wl);
        if (lane == wl) scanned |= 1u << (j >> 6);
        minVal = m;
        const int r4c = sRow4Col[j];
        if (r4c < 0) sink = j; else i = r4c;
      }
      if (sink < 0) { if (status == 0) status = 2; break; }
      // dual update: every scanned column j (and the row matched to it, which is in the tree through j) moves by minVal - spc[j]
      if (lane == 0) sU[curRow] += minVal;
      for (int j = lane, k = 0; j < n; j += 64, k++) {
        if (!(scanned & (1u << k))) continue;
        const double d = minVal - sSpc[j];
        sV[j] -= d;
        const int r = sRow4Col[j];
        if (r >= 0) sU[r] += d;
      }
      wave_sync();
      if (lane == 0) {
        int j = sink;
        for (int guard = 0; guard <= n; guard++) {
          const int r = sPath[j];
          sRow4Col[j] = r;
          const int prev = sCol4Row[r];
          sCol4Row[r] = j;
          j = prev;
          if (r == curRow) break;
        }
      }
      wave_sync();
    }
    if (status == 0) {
      double sp = 0.0;
      for (int r = lane; r < n; r += 64) {
        const int j = sCol4Row[r];
        double cij = c;
        if (r < n1 && j < n2) {
          const double dx = sEx[r] - sGx[j], dy = sEy[r] - sGy[j];
          cij = fmin(sqrt(dx * dx + dy * dy), c);
        }
        if (cij == c) eCard += cij; else eDist += cij;   // OSPA.hpp:189-193
        sp += metric_pow(cij, p);
      }
      sp = wave_sum(sp); eCard = wave_sum(eCard); eDist = wave_sum(eDist);
      ospa = p == 1.0 ? sp / n : pow(sp / n, 1.0 / p);
      cola = ospa * (p == 1.0 ? (double)n : pow((double)n, 1.0 / p)) / c;
    }
  }
  if (status != 0) ospa = cola = eDist = eCard = qnan;
  if (lane == 0) {
    struct rfsgpu_step_error &o = A.out[b];
    o.t = t; o.status = status; o.best_slot = best; o.n_est = n1; o.n_truth = n2; o.cardinality = card;
    o.ospa = ospa; o.cola = cola; o.e_dist = eDist; o.e_card = eCard;
    o.pose_ex = sx; o.pose_ey = sy; o.pose_eth = sth; o.pose_ed = sd; o.weight_sum = sw;
  }
}
