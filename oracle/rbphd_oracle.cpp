/*
 * rbphd_oracle.cpp -- CPU restatement of the RB-PHD update hot path of kykleung/RFS-SLAM.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product: only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library, and only as the
 * checker / the timed CPU baseline.  The product path (rfs-slam_amd/) never links, imports or calls it.
 *
 * PARITY PIN STATUS (see DESIGN.md "Oracle"): the reference needs Eigen3 + Boost, neither of which
 * exists in this image, and stand-in headers are not allowed, so the reference filter itself is
 * UNBUILDABLE here.  What IS pinned against the reference:
 *   - mat_perm            : the reference's own known-answer test (test/MatrixPermanentTest.hpp:55-87),
 *   - PermutationLexicographic restatement : the reference's own src/PermutationLexicographic.cpp compiled
 *     from /root/reference into oracle/_ref (oracle/Makefile), compared sequence-for-sequence,
 *   - Hungarian / Murty k-best scores : the reference's own src/BruteForceAssignment.cpp (its example
 *     checker for Murty, src/examples/linearAssignment_MurtyAlgorithm.cpp:99-130) compiled into oracle/_ref.
 * Everything else (updateMap, KF correct, RngBrg / VictoriaPark models, importanceWeighting, CostMatrixGeneral
 * partition, merge, prune, birth Gaussians, resample, and the FastSLAM / MH-FastSLAM update incl. CostMatrix::reduce and Murty's k best associations) is a
 * line-by-line restatement with NO reference-produced golden vectors: "parity unpinned" for those rows; they are
 * cross-checked only against independent numpy/scipy formulations in tests/ (CostMatrix::reduce: the reduced
 * problem keeps the optimum of the full one, scipy's Hungarian as the solver).
 *
 * Each function cites the reference file:line it follows (paths relative to /root/reference).
 * Arithmetic follows the reference's expression order (Eigen fixed-size closed forms written out).
 * The filter is a template over the measurement model, like the reference's RBPHDFilter<..., MeasurementModel, KF>.
 */
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <list>
#include <memory>
#include <queue>
#include <string>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/rfsgpu.h"

namespace orc {

static const double PI = acos(-1); /* include/RandomVec.hpp:55 */

/* ------------------------------------------------------------------------------------------------
 * Fixed-size algebra, written the way Eigen's fixed-size expression templates evaluate it
 * (coefficient (i,j) = sum over k in ascending order; nested products evaluated into temporaries).
 * ---------------------------------------------------------------------------------------------- */
template <int D>
struct Mat {
  double a[D * D];
  double &operator()(int i, int j) { return a[D * i + j]; }
  double operator()(int i, int j) const { return a[D * i + j]; }
};
template <int D>
static inline Mat<D> zeroM() {
  Mat<D> m;
  for (int k = 0; k < D * D; k++) m.a[k] = 0;
  return m;
}
template <int D>
static inline Mat<D> mul(const Mat<D> &A, const Mat<D> &B) {
  Mat<D> C;
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) {
      double s = A(i, 0) * B(0, j);
      for (int k = 1; k < D; k++) s += A(i, k) * B(k, j);
      C(i, j) = s;
    }
  return C;
}
template <int D>
static inline Mat<D> mulT(const Mat<D> &A, const Mat<D> &B) { /* A * B^T */
  Mat<D> C;
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) {
      double s = A(i, 0) * B(j, 0);
      for (int k = 1; k < D; k++) s += A(i, k) * B(j, k);
      C(i, j) = s;
    }
  return C;
}
typedef Mat<2> M2;
typedef Mat<3> M3;

static inline double det(const M2 &m) { return m(0, 0) * m(1, 1) - m(1, 0) * m(0, 1); } /* Eigen determinant_impl<.,2> */
static inline M2 inv(const M2 &m) {                                                          /* Eigen compute_inverse_size2_helper */
  double invdet = 1.0 / det(m);
  M2 r;
  r(0, 0) = m(1, 1) * invdet;
  r(1, 0) = -m(1, 0) * invdet;
  r(0, 1) = -m(0, 1) * invdet;
  r(1, 1) = m(0, 0) * invdet;
  return r;
}
/* Eigen bruteforce_det3_helper / determinant_impl<.,3> */
static inline double det3h(const M3 &m, int a, int b, int c) { return m(0, a) * (m(1, b) * m(2, c) - m(1, c) * m(2, b)); }
static inline double det(const M3 &m) { return det3h(m, 0, 1, 2) - det3h(m, 1, 0, 2) + det3h(m, 2, 0, 1); }
/* Eigen cofactor_3x3 + compute_inverse<.,3> / compute_inverse_size3_helper */
static inline double cof3(const M3 &m, int i, int j) {
  int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m(i1, j1) * m(i2, j2) - m(i1, j2) * m(i2, j1);
}
static inline M3 inv(const M3 &m) {
  double c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
  double d = (c0 * m(0, 0) + c1 * m(1, 0)) + c2 * m(2, 0);
  double invdet = 1.0 / d;
  M3 r;
  r(0, 0) = c0 * invdet; r(0, 1) = c1 * invdet; r(0, 2) = c2 * invdet;
  r(1, 0) = cof3(m, 0, 1) * invdet; r(1, 1) = cof3(m, 1, 1) * invdet; r(1, 2) = cof3(m, 2, 1) * invdet;
  r(2, 0) = cof3(m, 0, 2) * invdet; r(2, 1) = cof3(m, 1, 2) * invdet; r(2, 2) = cof3(m, 2, 2) * invdet;
  return r;
}

/* A Gaussian of the mixture: GaussianMixture<Landmark>::Gaussian (include/GaussianMixture.hpp:60-64).
 * valid == (landmark != NULL). */
template <int D>
struct GaussT {
  bool valid;
  double w, w_prev;
  double x[D];
  Mat<D> S;
};

/* RandomVec<n>::mahalanobisDist2 (include/RandomVec.hpp:387-394): e = to - x; (e^T * Sinv) * e. */
template <int D>
static inline double md2(const double *x, const Mat<D> &Sinv, const double *to) {
  double e[D], t[D];
  for (int k = 0; k < D; k++) e[k] = to[k] - x[k];
  for (int j = 0; j < D; j++) {
    double s = e[0] * Sinv(0, j);
    for (int i = 1; i < D; i++) s += e[i] * Sinv(i, j);
    t[j] = s;
  }
  double r = t[0] * e[0];
  for (int j = 1; j < D; j++) r += t[j] * e[j];
  return r;
}
/* RandomVec<n>::evalGaussianLikelihood (include/RandomVec.hpp:417-434). */
template <int D>
static inline double gauss_lik(const double *x, const Mat<D> &S, const double *at, double *md2_out) {
  double dt = det(S);
  double factor = sqrt(pow(2 * PI, D) * dt);
  Mat<D> Sinv = inv(S);
  double m = md2<D>(x, Sinv, at);
  double l = exp(-0.5 * m) / factor;
  if (l != l) l = 0;
  if (md2_out) *md2_out = m;
  return l;
}

struct Pose {
  double x[3];
  double P[9]; /* 3x3 row-major covariance */
};

/* ------------------------------------------------------------------------------------------------
 * MeasurementModel_RngBrg  (src/MeasurementModel_RngBrg.cpp) -- free functions on (config, R)
 * ---------------------------------------------------------------------------------------------- */
/* measure(): :70-115.  Returns false outside [rmin, rmax] (:111). */
static bool rb_measure_core(const double R[4], double rmax, double rmin, const Pose &pose, const double lx[2], const M2 &lS, double z[2],
                            M2 &S, M2 *Hout) {
  double dx = lx[0] - pose.x[0], dy = lx[1] - pose.x[1];
  double range2 = pow(dx, 2) + pow(dy, 2);
  double range = sqrt(range2);
  double bearing = atan2(dy, dx) - pose.x[2];
  while (bearing > PI) bearing -= 2 * PI;
  while (bearing < -PI) bearing += 2 * PI;
  z[0] = range;
  z[1] = bearing;
  M2 H;
  H(0, 0) = dx / range;   H(0, 1) = dy / range;
  H(1, 0) = -dy / range2; H(1, 1) = dx / range2;
  double Hr[2][3] = {{-dx / range, -dy / range, 0}, {dy / range2, -dx / range2, -1}};
  /* cov = H_lmk * Sl * H_lmk^T + H_robot * Sp * H_robot^T + R   (:102) */
  M2 A = mulT(mul(H, lS), H);
  double T[2][3];
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) T[i][j] = Hr[i][0] * pose.P[0 * 3 + j] + Hr[i][1] * pose.P[1 * 3 + j] + Hr[i][2] * pose.P[2 * 3 + j];
  M2 B;
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++) B(i, j) = T[i][0] * Hr[j][0] + T[i][1] * Hr[j][1] + T[i][2] * Hr[j][2];
  for (int k = 0; k < 4; k++) S.a[k] = (A.a[k] + B.a[k]) + R[k];
  if (Hout) *Hout = H;
  if (range > rmax || range < rmin) return false;
  return true;
}
/* inverseMeasure(): :117-136. */
static void rb_inverse_measure_core(const double R[4], const Pose &pose, const double z[2], double lx[2], M2 &lS) {
  double a = pose.x[2] + z[1];
  lx[0] = pose.x[0] + z[0] * cos(a);
  lx[1] = pose.x[1] + z[0] * sin(a);
  M2 Hinv;
  Hinv(0, 0) = cos(a); Hinv(0, 1) = -z[0] * sin(a);
  Hinv(1, 0) = sin(a); Hinv(1, 1) = z[0] * cos(a);
  M2 Rm;
  memcpy(Rm.a, R, sizeof(Rm.a));
  lS = mulT(mul(Hinv, Rm), Hinv);
}

/* ---- model policy: 2-D range-bearing (MeasurementModel_RngBrg + KalmanFilter_RngBrg) ---- */
struct ModelRB {
  enum { D = 2 };
  rfsgpu_rngbrg_config c;
  rfsgpu_kf_config kf;
  ModelRB() {
    memset(&c, 0, sizeof(c)); /* defaults: src/MeasurementModel_RngBrg.cpp:35-43 */
    c.probabilityOfDetection = 0.95; c.uniformClutterIntensity = 0.1;
    c.rangeLimMax = 5; c.rangeLimMin = 0.3; c.rangeLimBuffer = 0.25;
    kf.rangeInnovationThreshold = -1; kf.bearingInnovationThreshold = -1;
  }
  bool measure(const Pose &pose, const double *lx, const M2 &lS, double *z, M2 &S, M2 *H) const {
    return rb_measure_core(c.R, c.rangeLimMax, c.rangeLimMin, pose, lx, lS, z, S, H);
  }
  void inverse_measure(const Pose &pose, const double *z, double *lx, M2 &lS) const { rb_inverse_measure_core(c.R, pose, z, lx, lS); }
  /* probabilityOfDetection(): :138-167. */
  double pd(const Pose &pose, const double *lx, const M2 &, bool &close) const {
    close = false;
    double range = sqrt(pow(lx[0] - pose.x[0], 2) + pow(lx[1] - pose.x[1], 2));
    double Pd;
    if (range <= c.rangeLimMax && range >= c.rangeLimMin) {
      Pd = c.probabilityOfDetection;
      if (range >= (c.rangeLimMax - c.rangeLimBuffer) || range <= (c.rangeLimMin + c.rangeLimBuffer)) close = true;
    } else {
      Pd = 0;
      if (range <= (c.rangeLimMax + c.rangeLimBuffer) && range >= (c.rangeLimMin - c.rangeLimBuffer)) close = true;
    }
    return Pd;
  }
  double clutter() const { return c.uniformClutterIntensity; }                          /* :169-172 */
  double clutter_integral() const {                                                       /* :175-178 */
    double sensingArea = 2 * PI * (c.rangeLimMax - c.rangeLimMin);
    return c.uniformClutterIntensity * sensingArea;
  }
  /* KalmanFilter_RngBrg::calculateInnovation: src/KalmanFilter_RngBrg.cpp:52-65 (range gate BEFORE wrap). */
  bool innovation(const double *z_exp, const double *z_act, double *nu) const {
    nu[0] = z_act[0] - z_exp[0];
    nu[1] = z_act[1] - z_exp[1];
    if (kf.rangeInnovationThreshold > 0 && fabs(nu[0]) > kf.rangeInnovationThreshold) return false;
    while (nu[1] > PI) nu[1] -= 2 * PI;
    while (nu[1] < -PI) nu[1] += 2 * PI;
    if (kf.bearingInnovationThreshold > 0 && fabs(nu[1]) > kf.bearingInnovationThreshold) return false;
    return true;
  }
};

/* ---- model policy: Victoria Park (range, bearing, diameter)  src/MeasurementModel_VictoriaPark.cpp,
 *      include/KalmanFilter_VictoriaPark.hpp ---- */
struct ModelVP {
  enum { D = 3 };
  rfsgpu_vp_config c;
  rfsgpu_kf_config kf;
  std::vector<double> scan;
  double clutterIntensity_;
  ModelVP() {
    memset(&c, 0, sizeof(c));
    kf.rangeInnovationThreshold = -1; kf.bearingInnovationThreshold = -1;
    clutterIntensity_ = 0;
  }
  /* measure(): :104-151.  Pose rebuilt from its MEAN only (covariance dropped, :112-114), heading - pi/2, 2-D
   * model on (x,y) -- the embedded rangeBearingModel keeps its default range limits and its return value is
   * ignored -- diameter passes through, S33 = Sigma33 + R33 + r^2 * Slb, H = blockdiag(H2, 1); always true. */
  bool measure(const Pose &pose, const double *lx, const M3 &lS, double *z, M3 &S, M3 *H) const {
    Pose tp;
    tp.x[0] = pose.x[0]; tp.x[1] = pose.x[1]; tp.x[2] = pose.x[2] - PI / 2;
    memset(tp.P, 0, sizeof(tp.P));
    M2 S2l, S2, H2;
    S2l(0, 0) = lS(0, 0); S2l(0, 1) = lS(0, 1); S2l(1, 0) = lS(1, 0); S2l(1, 1) = lS(1, 1);
    double R2[4] = {c.R[0], c.R[1], c.R[3], c.R[4]};
    double z2[2];
    rb_measure_core(R2, 5, 0.3, tp, lx, S2l, z2, S2, &H2);
    z[0] = z2[0]; z[1] = z2[1]; z[2] = lx[2];
    S = zeroM<3>();
    S(0, 0) = S2(0, 0); S(0, 1) = S2(0, 1); S(1, 0) = S2(1, 0); S(1, 1) = S2(1, 1);
    S(2, 2) = lS(2, 2) + c.R[8] + pow(z2[0], 2) * c.Slb;
    if (H) {
      *H = zeroM<3>();
      (*H)(0, 0) = H2(0, 0); (*H)(0, 1) = H2(0, 1); (*H)(1, 0) = H2(1, 0); (*H)(1, 1) = H2(1, 1);
      (*H)(2, 2) = 1;
    }
    return true;
  }
  /* inverseMeasure(): :75-102. */
  void inverse_measure(const Pose &pose, const double *z, double *lx, M3 &lS) const {
    Pose tp;
    tp.x[0] = pose.x[0]; tp.x[1] = pose.x[1]; tp.x[2] = pose.x[2] - PI / 2;
    memset(tp.P, 0, sizeof(tp.P));
    double R2[4] = {c.R[0], c.R[1], c.R[3], c.R[4]};
    M2 c2;
    rb_inverse_measure_core(R2, tp, z, lx, c2);
    lS = zeroM<3>();
    lS(0, 0) = c2(0, 0); lS(0, 1) = c2(0, 1); lS(1, 0) = c2(1, 0); lS(1, 1) = c2(1, 1);
    lS(2, 2) = c.R[8];
    lx[2] = z[2];
  }
  /* probabilityOfDetection2(): :202-265 (occlusion count against the raw scan, Pd table). */
  double pd2(const Pose &pose, const double *lx, const M3 &lS, bool &close) const {
    close = false;
    double z[3];
    M3 S;
    measure(pose, lx, lS, z, S, nullptr);
    double dist = z[0], angle = z[1];
    if (angle > c.bearingLimitMax || angle < c.bearingLimitMin || dist < c.rangeLimMin || dist > c.rangeLimMax) return 0;
    double modified_radius = z[2] / 2;
    double gamma = atan(modified_radius / z[0]);
    int maxNumPoints = (int)floor(2 * gamma * 720.0 / (2 * PI));
    const int tab = c.nPd;
    if (tab > maxNumPoints && maxNumPoints >= 0 && c.PdTable[maxNumPoints] == 0) return 0;
    if (tab > maxNumPoints && maxNumPoints >= 0 && c.PdTable[maxNumPoints] < c.bufferZonePd) close = true;
    int minb = (int)ceil((angle - gamma) * 720.0 / (2 * PI));
    int maxb = minb + maxNumPoints;
    while (minb >= 720) minb -= 720;
    while (minb < 0) minb += 720;
    while (maxb >= 720) maxb -= 720;
    while (maxb < 0) maxb += 720;
    int numPoints = 0;
    double minrange = dist - modified_radius - 6 * 0.03;
    if ((maxb - minb + 720) % 720 > 0) {
      for (int b = minb; b != maxb; b = (b + 1) % 720) {
        double s = (b < (int)scan.size()) ? scan[b] : 0.0; /* the reference reads past a 361-entry scan here (UB); 0 counts as visible */
        if (s > minrange || s == 0) numPoints++;
      }
    }
    if (numPoints >= tab) numPoints = tab - 1;
    if (c.PdTable[numPoints] == 0) close = false;
    return c.PdTable[numPoints];
  }
  /* probabilityOfDetection(): :153-199 (max over laterally shifted copies; `angle` formed as written). */
  double pd(const Pose &pose, const double *lx, const M3 &lS, bool &close) const {
    double z[3];
    M3 S;
    measure(pose, lx, lS, z, S, nullptr);
    double angle = atan2(z[1], z[0]) + pose.x[2]; /* sic (:165-166) */
    double perp[2] = {-sin(angle), cos(angle)};
    double r0 = perp[0] * lS(0, 0) + perp[1] * lS(1, 0), r1 = perp[0] * lS(0, 1) + perp[1] * lS(1, 1);
    double sd = r0 * perp[0] + r1 * perp[1];
    sd = 3 * sqrt(sd);
    sd = std::max(sd, 0.2);
    double mn = DBL_MAX, mx = -DBL_MAX;
    double l2[3] = {lx[0], lx[1], lx[2]};
    for (int i = 1; (i - 1) * (2 * lx[2]) < sd; i++) {
      if (i > 100000) break; /* non-positive diameter: the reference never terminates */
      double s = i * 2 * lx[2];
      l2[0] = lx[0] + s * perp[0]; l2[1] = lx[1] + s * perp[1];
      double p = pd2(pose, l2, lS, close);
      mn = std::min(mn, p); mx = std::max(mx, p);
      l2[0] = lx[0] - s * perp[0]; l2[1] = lx[1] - s * perp[1];
      p = pd2(pose, l2, lS, close);
      mn = std::min(mn, p); mx = std::max(mx, p);
    }
    double p = pd2(pose, lx, lS, close);
    mn = std::min(mn, p); mx = std::max(mx, p);
    if (mn == 0 && mx > 0) close = true;
    return mx;
  }
  /* setLaserScan(): :267-281. */
  void set_scan(const double *s, int n) {
    scan.assign(s, s + n);
    double FoVArea = 0;
    for (int i = 1; i < n; i++) FoVArea += scan[i] * scan[i - 1];
    FoVArea += scan[0] * scan[n - 1];
    FoVArea *= sin(PI / 360) / 2;
    clutterIntensity_ = c.expectedClutterNumber / FoVArea;
  }
  double clutter() const { return clutterIntensity_; }
  double clutter_integral() const { return c.expectedClutterNumber; }
  /* KalmanFilter_VictoriaPark::calculateInnovation: include/KalmanFilter_VictoriaPark.hpp:56-73 (wrap FIRST). */
  bool innovation(const double *z_exp, const double *z_act, double *nu) const {
    for (int k = 0; k < 3; k++) nu[k] = z_act[k] - z_exp[k];
    while (nu[1] > PI) nu[1] -= 2 * PI;
    while (nu[1] < -PI) nu[1] += 2 * PI;
    if (kf.rangeInnovationThreshold > 0 && fabs(nu[0]) > kf.rangeInnovationThreshold) return false;
    if (kf.bearingInnovationThreshold > 0 && fabs(nu[1]) > kf.bearingInnovationThreshold) return false;
    return true;
  }
};

/* ------------------------------------------------------------------------------------------------
 * PermutationLexicographic  (src/PermutationLexicographic.cpp:38-96), restated literally.
 * ---------------------------------------------------------------------------------------------- */
struct PermLex {
  unsigned nM_, nZ_, nP_, oSize_;
  bool last_;
  std::vector<unsigned> o_;
  PermLex(unsigned nM, unsigned nZ, bool includeClutter) : nM_(nM), nZ_(nZ), nP_(0), last_(false) {
    if (nM != nZ) includeClutter = true;
    oSize_ = includeClutter ? nM + nZ : nM;
    o_.resize(oSize_);
    for (unsigned i = 0; i < oSize_; i++) o_[i] = (i < nZ) ? i : nZ;
  }
  unsigned next(unsigned *permutation) {
    if (last_) {
      for (unsigned i = 0; i < oSize_; i++) permutation[i] = 0;
      return 0;
    }
    for (unsigned i = 0; i < oSize_; i++) permutation[i] = o_[i];
    unsigned u = nM_;
    unsigned v = oSize_ - 1; /* oSize_ == 0 cannot occur from the filter */
    while (u < v) { std::swap(o_[u], o_[v]); u++; v--; }
    last_ = !std::next_permutation(o_.begin(), o_.end());
    nP_++;
    return nP_;
  }
};

/* ------------------------------------------------------------------------------------------------
 * HungarianMethod::run<double**>  (include/HungarianMethod.hpp:91-587), maximize = true path,
 * restated literally incl. the in-place offset add/subtract (:137-148, :244-250) and the
 * 1e-14 / 1e-12 tolerances (:293, :487, :500, :538).
 * ---------------------------------------------------------------------------------------------- */
static long g_hungarian_fail = 0;
/* Test probe: the largest number of entries an augmenting search had put into its breadth-first queue when the expansion that
 * discovers the target column began (what a solver that stops at the discovery has enqueued: the device keeps entries from
 * index 64 on in a second register, csrc/hungarian_wave.h). */
static long g_hungarian_max_queue_tail = 0;
static inline void hungarian_note_queue_tail(long v) {
  long cur = __atomic_load_n(&g_hungarian_max_queue_tail, __ATOMIC_RELAXED);
  while (v > cur && !__atomic_compare_exchange_n(&g_hungarian_max_queue_tail, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
static bool hungarian_run(double **C, int n, int *soln, double *cost) {
  std::vector<double> lx(n), ly(n), slack(n);
  std::vector<int> xy(n, -1), yx(n, -1), p(2 * n);
  std::vector<char> S(n, 0), T(n, 0), NS(n, 0), x_q(n), y_q(n);
  int x, x_t, y, root = 0;
  bool pickFreeVertex = true, updateLabel;
  double offset = 0;
  for (int xx = 0; xx < n; xx++)
    for (int yy = 0; yy < n; yy++)
      if (C[xx][yy] < offset) offset = C[xx][yy];
  for (int xx = 0; xx < n; xx++)
    for (int yy = 0; yy < n; yy++) C[xx][yy] -= offset;
  /* Step 1 (:162-190) */
  for (int xx = 0; xx < n; xx++) {
    lx[xx] = 0.0;
    ly[xx] = 0.0;
    for (int yy = 0; yy < n; yy++) {
      if (C[xx][yy] >= lx[xx]) { lx[xx] = C[xx][yy]; xy[xx] = yy; }
    }
    int yy = xy[xx];
    x_t = yx[yy];
    if (yx[yy] != -1) {
      if (C[xx][yy] > C[x_t][yy]) { xy[x_t] = -1; yx[yy] = xx; }
      else { xy[xx] = -1; }
    } else {
      yx[yy] = xx;
    }
  }
  while (true) {
    if (pickFreeVertex) { /* Step 2 (:222-318) */
      for (x = 0; x < n; x++) S[x] = 0;
      for (y = 0; y < n; y++) { T[y] = 0; NS[y] = 0; }
      for (x = 0; x < n; x++) if (xy[x] == -1) break;
      if (x == n) {
        if (offset != 0)
          for (x = 0; x < n; x++)
            for (y = 0; y < n; y++) C[x][y] = C[x][y] + offset;
        *cost = 0;
        for (x = 0; x < n; x++) { soln[x] = xy[x]; *cost += C[x][xy[x]]; }
        return true;
      }
      root = x;
      S[x] = 1;
      for (y = 0; y < n; y++) {
        slack[y] = lx[x] + ly[y] - C[x][y];
        if (fabs(slack[y]) < 1e-14) { slack[y] = 0; NS[y] = 1; }
      }
    }
    /* Step 3 (:320-390) */
    updateLabel = true;
    for (y = 0; y < n; y++) if (NS[y] != T[y]) { updateLabel = false; break; }
    if (updateLabel) {
      double a = DBL_MAX;
      for (y = 0; y < n; y++) if (!T[y]) a = fmin(a, slack[y]);
      for (x = 0; x < n; x++) if (S[x]) lx[x] -= a;
      for (y = 0; y < n; y++) if (T[y]) ly[y] += a;
      for (y = 0; y < n; y++) {
        if (!T[y]) slack[y] -= a;
        if (slack[y] == 0) NS[y] = 1;
      }
    }
    /* Step 4 (:392-) */
    for (y = 0; y < n; y++) if (NS[y] && !T[y]) break;
    if (y >= n) { g_hungarian_fail++; return false; } /* reference reads yx[n] (UB); treated as failure */
    x_t = yx[y];
    if (x_t == -1) {
      bool augmentingPathFound = false;
      int target = y + n;
      std::queue<int> q;
      long nPushed = 1, tailAtDiscovery = -1;
      q.push(root);
      for (x = 0; x < n; x++) { x_q[x] = 0; y_q[x] = 0; }
      x_q[root] = 1;
      for (x = 0; x < 2 * n; x++) p[x] = -1;
      int t = q.front();
      while (!q.empty()) {
        t = q.front();
        if (t == target) {
          while (t != root) {
            if (t >= n) { x_t = p[t]; xy[x_t] = t - n; yx[t - n] = x_t; }
            t = p[t];
          }
          augmentingPathFound = true;
          break;
        }
        q.pop();
        if (t < n) {
          const long tailBefore = nPushed;
          for (y = 0; y < n; y++) {
            if (fabs(lx[t] + ly[y] - C[t][y]) < 1e-12 && !y_q[y] && xy[t] != y) {
              y_q[y] = 1; p[y + n] = t; q.push(y + n); nPushed++;
              if (y + n == target && tailAtDiscovery < 0) tailAtDiscovery = tailBefore;
            }
          }
        } else {
          t -= n;
          for (x = 0; x < n; x++) {
            if (fabs(lx[x] + ly[t] - C[x][t]) < 1e-12 && S[x] && !x_q[x] && yx[t] == x) { x_q[x] = 1; p[x] = t + n; q.push(x); nPushed++; }
          }
        }
      }
      if (tailAtDiscovery >= 0) hungarian_note_queue_tail(tailAtDiscovery);
      if (!augmentingPathFound) { g_hungarian_fail++; return false; } /* :513-523 ("Cannot find alternating path") */
      pickFreeVertex = true;
    } else {
      S[x_t] = 1;
      T[y] = 1;
      for (int y_t = 0; y_t < n; y_t++)
        if (fabs(lx[x_t] + ly[y_t] - C[x_t][y_t]) < 1e-14) NS[y_t] = 1;
      for (int yy = 0; yy < n; yy++) {
        double slack_x_t = lx[x_t] + ly[yy] - C[x_t][yy];
        if (slack_x_t < slack[yy]) slack[yy] = slack_x_t;
      }
      pickFreeVertex = false;
    }
  }
}

/* ------------------------------------------------------------------------------------------------
 * Murty k-best  (src/MurtyAlgorithm.cpp:107-336, include/MurtyAlgorithm.hpp), restated literally:
 * same node tree, same std::priority_queue (so identical tie behaviour), same dummy-column
 * duplicate-suppression quirk comparing the REDUCED column index (:256-262).
 * ---------------------------------------------------------------------------------------------- */
struct MurtyNode {
  int id;
  MurtyNode *parent;
  std::vector<int> a;
  double s;
};
struct MurtyNodeCompare {
  bool operator()(const MurtyNode *p1, const MurtyNode *p2) const { return p1->s < p2->s; }
};
struct Murty {
  int k_;
  int n_;
  double bigNumber_;
  double **C_;
  std::vector<std::vector<double>> Ct_store;
  std::vector<double *> C_t_;
  std::vector<std::unique_ptr<MurtyNode>> pool;
  MurtyNode *root_;
  std::priority_queue<MurtyNode *, std::vector<MurtyNode *>, MurtyNodeCompare> pq;
  int realAssign_nC_, realAssign_nR_;
  Murty(double **C, int n, double bigNum = 10000) : k_(0), n_(n), bigNumber_(bigNum), C_(C), realAssign_nC_(n), realAssign_nR_(n) {
    Ct_store.assign(n, std::vector<double>(n));
    C_t_.resize(n);
    for (int i = 0; i < n; i++) C_t_[i] = Ct_store[i].data();
    pool.emplace_back(new MurtyNode{0, nullptr, {}, 0});
    root_ = pool.back().get();
  }
  void setRealAssignmentBlock(int nR, int nC) {
    realAssign_nC_ = nC; realAssign_nR_ = nR;
    if (realAssign_nC_ > n_) realAssign_nC_ = n_;
    if (realAssign_nR_ > n_) realAssign_nR_ = n_;
  }
  int findNextBest(std::vector<int> &assignment, double &score) {
    if (k_ == 0) { /* :147-158 */
      std::vector<int> a(n_);
      double s;
      if (!hungarian_run(C_, n_, a.data(), &s)) { assignment.clear(); score = 0; return -1; }
      root_->a = a; root_->s = s;
      k_++;
      pq.push(root_);
      assignment = a; score = s;
      return k_;
    }
    if (pq.empty()) { assignment.clear(); score = 0; return -1; }
    MurtyNode *parent = pq.top();
    int parent_partition = parent->id;
    pq.pop();
    const std::vector<int> a_parent = parent->a;
    int partitionMax = realAssign_nR_;
    if (realAssign_nR_ == n_) partitionMax = n_ - 1;
    for (int n = parent_partition; n < partitionMax; n++) { /* :188 */
      pool.emplace_back(new MurtyNode{n, parent, {}, 0});
      MurtyNode *p = pool.back().get();
      std::vector<int> a(n_, 0);
      std::vector<char> freeCol(n_, 1);
      double assignmentFixedScore = 0;
      for (int i = 0; i < parent_partition; i++) { a[i] = a_parent[i]; freeCol[a[i]] = 0; assignmentFixedScore += C_[i][a[i]]; }
      for (int i = parent_partition; i < n; i++) { a[i] = a_parent[i]; freeCol[a[i]] = 0; assignmentFixedScore += C_[i][a[i]]; }
      int nFree = n_ - n;
      std::vector<int> rowRemap(nFree), rowRemapR(n_, -1), colRemap(nFree), colRemapR(n_, -1);
      int nFreeCols = 0;
      for (int i = 0; i < nFree; i++) { rowRemap[i] = n + i; rowRemapR[n + i] = i; }
      for (int j = 0; j < n_; j++) if (freeCol[j]) { colRemap[nFreeCols] = j; colRemapR[j] = nFreeCols; nFreeCols++; }
      for (int i = 0; i < nFree; i++)
        for (int j = 0; j < nFree; j++) C_t_[i][j] = C_[rowRemap[i]][colRemap[j]];
      /* negative constraints (:247-265) */
      MurtyNode *current = p, *next;
      do {
        int currentPart = current->id;
        next = current->parent;
        int doNotAssign_i = rowRemapR[currentPart];
        int doNotAssign_j = colRemapR[next->a[currentPart]];
        C_t_[doNotAssign_i][doNotAssign_j] = -bigNumber_;
        if (doNotAssign_j >= realAssign_nC_) {
          for (int y = 0; y < nFree; y++)
            if (y >= realAssign_nC_) C_t_[doNotAssign_i][y] = -bigNumber_;
        }
        current = next;
      } while (current != root_ && current->id >= p->id);
      bool solutionPossible = false;
      int constraintRow = rowRemapR[p->id];
      for (int j = 0; j < nFree; j++) if (C_t_[constraintRow][j] != -bigNumber_) { solutionPossible = true; break; }
      if (solutionPossible) {
        std::vector<int> aTmp(nFree);
        double s = 0;
        if (!hungarian_run(C_t_.data(), nFree, aTmp.data(), &s)) continue; /* reference ignores the failure (UB) */
        double s_more_accurate = 0;
        for (int i = 0; i < nFree; i++) {
          int i_actual = rowRemap[i];
          int j_actual = colRemap[aTmp[i]];
          a[i_actual] = j_actual;
          s_more_accurate += C_[i_actual][a[i_actual]];
        }
        s_more_accurate += assignmentFixedScore;
        p->a = a; p->s = s_more_accurate;
        pq.push(p);
      }
    }
    if (pq.empty()) { assignment.clear(); score = 0; return -1; }
    MurtyNode *hi = pq.top();
    assignment = hi->a; score = hi->s;
    k_++;
    return k_;
  }
};

/* ------------------------------------------------------------------------------------------------
 * CostMatrixGeneral  (src/CostMatrix.cpp:12-28, 92-227) restated, incl. the partition-count /
 * indexing quirk the caller exposes (SURVEY §7 hard part 2).
 * Component ids = BGL connected_components DFS discovery order over vertices 0..nR+nC-1, i.e.
 * components numbered by their smallest vertex (rows first, then columns).
 * ---------------------------------------------------------------------------------------------- */
struct CostMatrixGeneral {
  int nR_, nC_;
  std::vector<std::vector<double>> C_;
  std::vector<std::vector<unsigned>> components_i, components_j;
  int combinedZeroPartition_ = -1;
  int nPartitions_ = 0;
  int ncc_ = 0;
  CostMatrixGeneral(int nR, int nC) : nR_(nR), nC_(nC), C_(nR, std::vector<double>(nC, 0.0)) {}
  int partition() {
    if (nPartitions_ != 0) return nPartitions_;
    int V = nR_ + nC_;
    std::vector<int> cc(V, -1);
    int ncc = 0;
    std::vector<int> stack;
    for (int v0 = 0; v0 < V; v0++) {
      if (cc[v0] != -1) continue;
      cc[v0] = ncc;
      stack.clear();
      stack.push_back(v0);
      while (!stack.empty()) {
        int v = stack.back();
        stack.pop_back();
        if (v < nR_) {
          for (int j = 0; j < nC_; j++)
            if (C_[v][j] != 0 && cc[nR_ + j] == -1) { cc[nR_ + j] = ncc; stack.push_back(nR_ + j); }
        } else {
          int j = v - nR_;
          for (int i = 0; i < nR_; i++)
            if (C_[i][j] != 0 && cc[i] == -1) { cc[i] = ncc; stack.push_back(i); }
        }
      }
      ncc++;
    }
    ncc_ = ncc;
    components_i.assign(ncc, {});
    components_j.assign(ncc, {});
    for (int i = 0; i < nR_; i++) components_i[cc[i]].push_back(i);
    for (int j = nR_; j < V; j++) components_j[cc[j]].push_back(j - nR_);
    combinedZeroPartition_ = -1;
    int nMerged = 0;
    for (int n = 0; n < ncc; n++) {
      if (components_i[n].size() == 0 || components_j[n].size() == 0) {
        if (combinedZeroPartition_ == -1) combinedZeroPartition_ = n;
        else if (components_i[n].size() != 0) { components_i[combinedZeroPartition_].push_back(components_i[n][0]); nMerged++; }
        else { components_j[combinedZeroPartition_].push_back(components_j[n][0]); nMerged++; }
      }
    }
    nPartitions_ = ncc - nMerged;
    return nPartitions_;
  }
  /* getPartitionSize (:160-173) */
  bool getPartitionSize(int p, unsigned &nRows, unsigned &nCols) {
    nRows = components_i[p].size();
    nCols = components_j[p].size();
    return p != combinedZeroPartition_;
  }
  /* getPartition (:175-227): Cp is (nRows [+nCols]) x (nCols [+nRows]); only [0,nRows)x[0,nCols) filled. */
  bool getPartition(int p, std::vector<std::vector<double>> &Cp, unsigned &nRows, unsigned &nCols,
                    std::vector<unsigned> &rowIdx, std::vector<unsigned> &colIdx, bool extended) {
    nRows = components_i[p].size();
    nCols = components_j[p].size();
    unsigned nR = extended ? nRows + nCols : nRows;
    unsigned nC = extended ? nRows + nCols : nCols;
    Cp.assign(nR, std::vector<double>(nC, 0.0));
    for (unsigned i = 0; i < nRows; i++)
      for (unsigned j = 0; j < nCols; j++) Cp[i][j] = C_[components_i[p][i]][components_j[p][j]];
    rowIdx = components_i[p];
    colIdx = components_j[p];
    return p != combinedZeroPartition_;
  }
};

/* The partition / enumeration / Murty part of rfsMeasurementLikelihood (include/RBPHDFilter.hpp:865-996) on a filled
 * likelihood table.  Returns prod over partitions (NOT yet divided by the clutter integral). */
/* Checker for the engine's opt-in RFSGPU_PARTITION_EXACT mode (NOT reference behaviour): the untruncated sum over all partial
 * assignments of one partition, by dynamic programming over the subsets of its smaller side (raw likelihoods, not logs). */
static double exact_partition_sum(const std::vector<std::vector<double>> &L, unsigned nRows, unsigned nCols, const std::vector<double> &oneMinusPd,
                                  const std::vector<double> &clut) {
  const bool colsSmall = nCols <= nRows;
  const unsigned k = colsSmall ? nCols : nRows, nItems = colsSmall ? nRows : nCols;
  std::vector<double> f((size_t)1 << k, 0.0);
  f[0] = 1.0;
  for (unsigned it = 0; it < nItems; it++) {
    const double u = colsSmall ? oneMinusPd[it] : clut[it];
    for (size_t S = f.size(); S-- > 0;) {
      double acc = f[S] * u;
      for (unsigned b = 0; b < k; b++)
        if ((S >> b) & 1) acc += f[S ^ ((size_t)1 << b)] * (colsSmall ? L[it][b] : L[b][it]);
      f[S] = acc;
    }
  }
  double tot = 0;
  for (size_t S = 0; S < f.size(); S++) {
    double g = f[S];
    for (unsigned b = 0; b < k; b++)
      if (!((S >> b) & 1)) g *= colsSmall ? clut[b] : oneMinusPd[b];
    tot += g;
  }
  return tot;
}

static double partitions_likelihood(CostMatrixGeneral &cm, const std::vector<double> &evalPtPd, const std::vector<double> &clutter,
                                    long *murty_calls, long *lonerow_hits, bool exact_mode = false) {
  int nP = cm.partition();
  double l = 1;
  const double BIG_NEG_NUM = -1000;
  for (int p = 0; p < nP; p++) {
    double partition_likelihood = 0;
    unsigned nCols, nRows;
    std::vector<std::vector<double>> Cp;
    std::vector<unsigned> rowIdx, colIdx;
    bool isZeroPartition = !cm.getPartitionSize(p, nRows, nCols);
    bool useMurty = true;
    if (nRows + nCols <= 8 || isZeroPartition) useMurty = false;
    isZeroPartition = !cm.getPartition(p, Cp, nRows, nCols, rowIdx, colIdx, useMurty);
    if (isZeroPartition) {
      partition_likelihood = 1;
      for (unsigned r = 0; r < nRows; r++) partition_likelihood *= evalPtPd[rowIdx[r]]; /* sic: Pd, not 1-Pd (:893-896) */
      for (unsigned c = 0; c < nCols; c++) partition_likelihood *= clutter[colIdx[c]];
    } else {
      if (nCols == 0 && nRows == 1 && lonerow_hits) (*lonerow_hits)++;
      if (exact_mode && useMurty && std::min(nRows, nCols) <= 9) { /* RFSGPU_PARTITION_EXACT: see exact_partition_sum */
        std::vector<std::vector<double>> Lp(nRows, std::vector<double>(nCols));
        std::vector<double> omp(nRows), cl(nCols);
        for (unsigned r = 0; r < nRows; r++) { omp[r] = 1 - evalPtPd[rowIdx[r]]; for (unsigned c = 0; c < nCols; c++) Lp[r][c] = Cp[r][c]; }
        for (unsigned c = 0; c < nCols; c++) cl[c] = clutter[colIdx[c]];
        l *= exact_partition_sum(Lp, nRows, nCols, omp, cl);
        continue;
      }
      for (unsigned r = 0; r < nRows; r++)
        for (unsigned c = 0; c < nCols; c++) {
          if (Cp[r][c] == 0) Cp[r][c] = BIG_NEG_NUM;
          else { Cp[r][c] = log(Cp[r][c]); if (Cp[r][c] < BIG_NEG_NUM) Cp[r][c] = BIG_NEG_NUM; }
        }
      if (useMurty) {
        for (unsigned r = 0; r < nRows; r++)
          for (unsigned c = nCols; c < nRows + nCols; c++) Cp[r][c] = (r == c - nCols) ? log(1 - evalPtPd[rowIdx[r]]) : BIG_NEG_NUM;
        for (unsigned r = nRows; r < nRows + nCols; r++)
          for (unsigned c = 0; c < nCols; c++) Cp[r][c] = (r - nRows == c) ? log(clutter[colIdx[c]]) : BIG_NEG_NUM;
        for (unsigned r = nRows; r < nRows + nCols; r++)
          for (unsigned c = nCols; c < nRows + nCols; c++) Cp[r][c] = 0;
        std::vector<double *> rows(nRows + nCols);
        for (unsigned r = 0; r < nRows + nCols; r++) rows[r] = Cp[r].data();
        Murty murty(rows.data(), nRows + nCols);
        if (murty_calls) (*murty_calls)++;
        std::vector<int> a;
        partition_likelihood = 0;
        double pll = 0;
        murty.setRealAssignmentBlock(nRows, nCols);
        /* study hook (tools/murty_early_stop_study.py; RFSOR_MURTY_STUDY=<file>): per partition, the first call after which no later
         * term can change the running sum (exp(score) < 2^-56 of it: below half an ulp with a factor 4 to spare), the calls the
         * reference makes, and whether the returned scores ever INCREASED (the early stop's premise is that they do not). */
        static const char *study = getenv("RFSOR_MURTY_STUDY");
        int kStop = -1, kTotal = 0;
        double prev = 0, maxInc = 0;
        for (int k = 0; k < 200; k++) {
          int rank = murty.findNextBest(a, pll);
          if (rank == -1 || pll < BIG_NEG_NUM) break;
          const double term = exp(pll);
          partition_likelihood += term;
          if (study) {
            if (k > 0 && pll - prev > maxInc) maxInc = pll - prev;
            prev = pll;
            kTotal = k + 1;
            if (kStop < 0 && term < partition_likelihood * 0x1p-56) kStop = k + 1;
          }
        }
        if (study) {
#pragma omp critical(murty_study)
          {
            FILE *fp = fopen(study, "a");
            if (fp) { fprintf(fp, "%u %u %u %d %d %.3e\n", nRows + nCols, nRows, nCols, kStop, kTotal, maxInc); fclose(fp); }
          }
        }
      } else {
        partition_likelihood = 0;
        double pll = 0;
        std::vector<unsigned> o(nRows + nCols);
        PermLex pl(nRows, nCols, true);
        unsigned nPerm = pl.next(o.data());
        while (nPerm != 0) {
          pll = 0;
          for (unsigned a = 0; a < nRows; a++) {
            if (o[a] < nCols) pll += Cp[a][o[a]];
            else pll += log(1 - evalPtPd[rowIdx[a]]);
          }
          for (unsigned a = nRows; a < nRows + nCols; a++)
            if (o[a] < nCols) pll += log(clutter[colIdx[o[a]]]);
          partition_likelihood += exp(pll);
          nPerm = pl.next(o.data());
        }
      }
    }
    l *= partition_likelihood;
  }
  return l;
}

/* ------------------------------------------------------------------------------------------------
 * MatPerm::calc  (src/MatrixPermanent.cpp:41-112): Nijenhuis-Wilf / Gray-code Ryser.
 * ---------------------------------------------------------------------------------------------- */
static double mat_perm(const double *A, int n) {
  std::vector<double> x(n);
  std::vector<int> g(n, 0);
  double p = 0, s = -1;
  for (int i = 0; i < n; i++) {
    double row_i_sum = 0;
    for (int j = 0; j < n; j++) row_i_sum += A[i * n + j];
    x[i] = A[i * n + (n - 1)] - 0.5 * row_i_sum;
  }
  p = s;
  for (int i = 0; i < n; i++) p *= x[i];
  for (long long k = 2; k <= (long long)pow(2, n - 1); k++) {
    int j = 0;
    if (k % 2 == 0) j = 0;
    else { j = 1; while (g[j - 1] == 0) j++; }
    s *= -1;
    double z = 1 - 2 * g[j];
    g[j] = !g[j];
    double x_prod = 1;
    for (int i = 0; i < n; i++) { x[i] += z * A[i * n + j]; x_prod *= x[i]; }
    p += s * x_prod;
  }
  double retval = 2 * p;
  if (n % 2 != 0) retval *= -1;
  return retval;
}

static inline long long now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* ------------------------------------------------------------------------------------------------
 * The filter (model-independent interface + template over the model)
 * ---------------------------------------------------------------------------------------------- */
struct FilterBase {
  int n = 0, dm = 2, dz = 2;
  rfsgpu_filter_config cfg;
  std::vector<Pose> pose;
  std::vector<double> weight;
  std::vector<std::vector<unsigned>> unused;
  std::vector<unsigned> nInFov;
  std::vector<double> Z; /* measurements_ (dz doubles each) */
  int nZ = 0;
  bool exact_partitions = false; /* checker for RFSGPU_PARTITION_EXACT (not reference behaviour) */
  bool stable_sort = false; /* false: std::sort exactly as the reference (GaussianMixture.hpp:523-534);
                               true : (weight desc, index asc) == what the device path implements */
  long murty_calls = 0, lonerow_bug_hits = 0;
  long fs_solver_calls = 0, fs_solver_max_dim = 0; /* FastSLAM: reduced tables that needed the assignment solver */
  std::vector<int> fs_last_nMZ, fs_last_nRed, fs_last_nH; /* per particle of the last FastSLAM update: table dimension, reduced
                                                             dimension handed to Murty (0: skipped), hypotheses kept */
  rfsgpu_timing timing;
  std::string err;
  virtual ~FilterBase() {}
  virtual int gm_size(int slot) = 0;
  virtual void import_gm(int slot, int cnt, const double *w, const double *mean, const double *cov) = 0;
  virtual int export_gm(int slot, int max_n, double *w, double *wp, double *mean, double *cov) = 0;
  virtual int get_landmark(int slot, int m, double *mean, double *cov, double *w) = 0;
  virtual int predict_map(int add_birth) = 0;
  virtual int predict_map_level(int add_birth, const int *level_of_slot, int level, int do_static) = 0;
  virtual void update_map() = 0;
  virtual void importance_weighting() = 0;
  virtual void merge() = 0;
  virtual void prune() = 0;
  virtual void copy_particle(int dst, int src) = 0;
  virtual void set_lmk_noise(const double *Q) = 0;
  virtual int export_candidates(int slot, int max_n, double *mean, double *cov, int *support, int *checks) = 0;
  virtual void import_candidates(int slot, int cnt, const double *mean, const double *cov, const int *support, const int *checks) = 0;
  /* FastSLAM (include/FastSLAM.hpp) on the same state: mixtures = landmark maps with log-odds weights */
  rfsgpu_fastslam_config fs;
  std::vector<int> parents; /* source slot of every particle after the last FastSLAM update */
  bool fs_resample_occured = false; /* FastSLAM::resampleOccured_: the previous update ended in a resampling */
  virtual int fastslam_update() = 0;
  virtual void shrink(int n_out) = 0;
  /* Birth-state inheritance after a resampling.  The reference keeps three per-SLOT arrays in RBPHDFilter
   * (unused_measurements_, birthGaussians_, nLandmarksInFOV_) that Particle::copy does not carry; the first two are copied
   * lazily by the next addBirthGaussians, indexed with the particle's parent ID (include/RBPHDFilter.hpp:1005-1011) --
   * RFSGPU_INHERIT_REFERENCE restates exactly that (ids as in include/ParticleFilter.hpp:446-479 + Particle::copy,
   * include/Particle.hpp:218-223: a copy keeps its source's id_).  RFSGPU_INHERIT_EAGER is rounds 1-2's reading of the
   * intent (child takes the parent's lists and FOV count at resampling time); RFSGPU_INHERIT_EXTERNAL: the host does it. */
  int inherit_mode = RFSGPU_INHERIT_REFERENCE;
  std::vector<unsigned> pid, ppid; /* Particle::id_ / idParent_ of the particle in each slot */
  bool resample_occured = false;   /* RBPHDFilter::resampleOccured_ */
  bool cand_used = false;          /* candidate lists have been imported (the stand-in of the engine's flag behind rfsgpu_has_birth_candidates) */
  bool fastslam_handle = false;    /* rfsor_fastslam_update has run: rfs::FastSLAM copies its candidate lists at resampling time (FastSLAM.hpp:747-753) */
  bool eager() const { return inherit_mode == RFSGPU_INHERIT_EAGER || fastslam_handle; }
  void ensure_ids() { while ((int)pid.size() < n) { pid.push_back((unsigned)pid.size()); ppid.push_back((unsigned)ppid.size()); } }
  virtual void copy_map(int dst, int src) = 0; /* what Particle::copy carries besides the pose: the mixture */
};

static void fastslam_defaults(rfsgpu_fastslam_config *c, int n) { /* FastSLAM constructor, include/FastSLAM.hpp:243-257 */
  c->minUpdatesBeforeResample = 1;
  c->minMeasurementsBeforeResample = 1;
  c->landmarkExistencePrior = 0.5;
  c->mapExistencePruneThreshold = -3.0;
  c->minLogMeasurementLikelihood = -10.0;
  c->nParticlesMax = n * 3;
  c->maxNDataAssocHypotheses = 1;
  c->maxDataAssocLogLikelihoodDiff = 5;
  c->landmarkCandidateMeasurementSupportDist = 1;
  c->landmarkCandidateMeasurementCountThreshold = 1;
  c->landmarkCandidateCurrentMeasurementCountThreshold = 1;
  c->landmarkCandidateMeasurementCheckThreshold = 2;
  c->landmarkLockWeight = 10;
  c->pruningMeasurementsThreshold = 0;
}

/* CostMatrix::reduce + getCostMatrixReduced (src/CostMatrix.cpp:263-369) for an n x n table C with a LOWER limit `lim`
 * (minVal == true, the FastSLAM call).  a_fixed[i] = column of row i if that pairing is the only possibility for both, else
 * -1 (rows with no possibility at all included); iRed / jRed = the rows / columns left for the assignment solver; a
 * 1 x 1 remainder is assigned directly (:331-336) and the reduced size reported as 0. */
struct ReducedCost {
  std::vector<int> a_fixed, iRed, jRed;
  int nRed = 0;
};
static ReducedCost cost_matrix_reduce(std::vector<std::vector<double>> &C, int n, double lim) {
  ReducedCost R;
  std::vector<int> nMatch_i(n, 0), nMatch_j(n, 0), a_rev(n, -1);
  R.a_fixed.assign(n, -1);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      if (C[i][j] <= lim) {
        C[i][j] = lim;
      } else {
        nMatch_i[i]++;
        nMatch_j[j]++;
        if (nMatch_i[i] == 1 && nMatch_j[j] == 1) { R.a_fixed[i] = j; a_rev[j] = i; }
        if (nMatch_i[i] > 1) R.a_fixed[i] = -1;
        if (nMatch_j[j] > 1) a_rev[j] = -1;
      }
    }
  for (int k = 0; k < n; k++) {
    if (R.a_fixed[k] != -1 && nMatch_j[R.a_fixed[k]] != 1) R.a_fixed[k] = -1;
    if (a_rev[k] != -1 && nMatch_i[a_rev[k]] != 1) a_rev[k] = -1;
    if (R.a_fixed[k] == -1) R.iRed.push_back(k);
    if (a_rev[k] == -1) R.jRed.push_back(k);
  }
  R.nRed = (int)R.iRed.size(); /* == jRed.size() (asserted by the reference, :318) */
  if (R.nRed == 1) {
    R.a_fixed[R.iRed[0]] = R.jRed[0];
    R.nRed = 0;
  }
  return R;
}

template <class M>
struct FilterT : FilterBase {
  enum { D = M::D };
  typedef GaussT<D> Gauss;
  typedef Mat<D> MatD;
  struct Candidate { /* RBPHDFilter::BirthGaussianCandidate (:173-177) */
    double x[D];
    MatD S;
    unsigned nSupportingMeasurements, nChecks;
  };
  M model;
  MatD Qlm;
  std::vector<std::vector<Gauss>> gm; /* gList_ (may contain holes between merge and prune) */
  std::vector<int> gm_n;              /* n_ */
  std::vector<std::list<Candidate>> cand; /* birthGaussians_ */

  explicit FilterT(int n_) {
    n = n_; dm = D; dz = D;
    Qlm = zeroM<D>();
    pose.assign(n, Pose{});
    weight.assign(n, 1.0);
    gm.assign(n, {});
    gm_n.assign(n, 0);
    cand.assign(n, {});
    unused.assign(n, {});
    nInFov.assign(n, 0);
    memset(&timing, 0, sizeof(timing));
    fastslam_defaults(&fs, n);
  }

  /* KalmanFilter::correct, vector overload: include/KalmanFilter.hpp:261-342.  One landmark against all measurements.
   * lik uses the RAW difference z - z_exp (:317-320), the updated mean uses the wrapped/gated innovation.
   * NOTE (:302): `P_updated = (P_updated + P_updated.transpose())/2` aliases in real Eigen release builds (<= 1 ulp
   * asymmetry left behind); restated here as the intended exact symmetrisation. */
  bool kf_correct_all(const Pose &ps, const Gauss &lm, std::vector<Gauss> &lmNew, std::vector<double> &lik, std::vector<double> &md2v) {
    double z_exp[D];
    MatD S, H;
    if (!model.measure(ps, lm.x, lm.S, z_exp, S, &H)) {
      for (int i = 0; i < nZ; i++) { lik[i] = 0; md2v[i] = 0; }
      return false;
    }
    MatD S_inv = inv(S);
    const MatD &P = lm.S;
    MatD Kg = mul(mulT(P, H), S_inv); /* K = P * H^T * S_inv */
    MatD KH = mul(Kg, H);
    MatD IKH;
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++) IKH(i, j) = (i == j ? 1.0 : 0.0) - KH(i, j);
    MatD Pu = mul(IKH, P);
    MatD Ps;
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++) Ps(i, j) = (Pu(i, j) + Pu(j, i)) / 2;
    for (int i = 0; i < nZ; i++) {
      const double *z = &Z[(size_t)D * i];
      double nu[D];
      if (model.innovation(z_exp, z, nu)) {
        lmNew[i].valid = true;
        for (int r = 0; r < D; r++) {
          double s = Kg(r, 0) * nu[0];
          for (int k = 1; k < D; k++) s += Kg(r, k) * nu[k];
          lmNew[i].x[r] = lm.x[r] + s;
        }
        lmNew[i].S = Ps;
        double m2;
        double zl = gauss_lik<D>(z_exp, S, z, &m2); /* innov.set(z_exp,S); innov.evalGaussianLikelihood(measurement[i], &md2) */
        if (zl != zl) zl = 0;
        lik[i] = zl;
        md2v[i] = m2;
      } else {
        lik[i] = 0;
        md2v[i] = 0;
      }
    }
    return true;
  }
  /* KalmanFilter::correct, single-measurement overload (:209-259), used by addBirthGaussians. */
  bool kf_correct_one(const Pose &ps, const double *z, const double *lx, const MatD &lS, double *ox, MatD &oS) {
    double z_exp[D];
    MatD S, H;
    if (!model.measure(ps, lx, lS, z_exp, S, &H)) return false;
    MatD S_inv = inv(S);
    double nu[D];
    if (!model.innovation(z_exp, z, nu)) return false;
    MatD Kg = mul(mulT(lS, H), S_inv);
    MatD KH = mul(Kg, H);
    MatD IKH;
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++) IKH(i, j) = (i == j ? 1.0 : 0.0) - KH(i, j);
    MatD Pu = mul(IKH, lS);
    double nx[D];
    for (int r = 0; r < D; r++) {
      double s = Kg(r, 0) * nu[0];
      for (int k = 1; k < D; k++) s += Kg(r, k) * nu[k];
      nx[r] = lx[r] + s;
    }
    MatD Ps;
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++) Ps(i, j) = (Pu(i, j) + Pu(j, i)) / 2;
    oS = Ps;
    for (int r = 0; r < D; r++) ox[r] = nx[r];
    return true;
  }

  /* RBPHDFilter::updateMap  (include/RBPHDFilter.hpp:543-725) for one particle. */
  void update_map_particle(int i) {
    std::vector<Gauss> &G = gm[i];
    const unsigned nM = gm_n[i]; /* getGaussianCount(); storage has no holes at this point */
    unused[i].clear();
    nInFov[i] = 0;
    if (nM == 0) {
      for (int z = 0; z < nZ; z++) unused[i].push_back(z);
      return;
    }
    /* per-thread scratch that persists across particles, like the reference's per-thread wTables_/mTables_ (:352-393) */
    static thread_local std::vector<double> Pd, W, lik, md2v;
    static thread_local std::vector<int> closeLim;
    static thread_local std::vector<char> Mvalid;
    static thread_local std::vector<Gauss> Mtab, lmNew;
    Pd.assign(nM, 0.0);
    closeLim.assign(nM, 0);
    double w_km_sum = std::numeric_limits<double>::denorm_min();
    double likelihoodProd = 1;
    if (cfg.useClusterProcess)
      for (unsigned m = 0; m < nM; m++) w_km_sum += G[m].w;
    W.assign((size_t)nM * nZ, 0.0);
    Mvalid.assign((size_t)nM * nZ, 0);
    if (Mtab.size() < (size_t)nM * nZ) Mtab.resize((size_t)nM * nZ);
    const Pose &ps = pose[i];
    const double thr = cfg.newGaussianCreateInnovMDThreshold * cfg.newGaussianCreateInnovMDThreshold;
    lik.assign(nZ, 0.0);
    md2v.assign(nZ, 0.0);
    if (lmNew.size() < (size_t)nZ) lmNew.resize(nZ);
    for (unsigned m = 0; m < nM; m++) {
      bool close;
      Pd[m] = model.pd(ps, G[m].x, G[m].S, close);
      if (close) { closeLim[m] = 1; Pd[m] = 1; } else closeLim[m] = 0;
      double w_km = G[m].w;
      double Pd_times_w_km = Pd[m] * w_km;
      if (Pd[m] != 0) {
        nInFov[i]++;
        kf_correct_all(ps, G[m], lmNew, lik, md2v);
        for (int z = 0; z < nZ; z++) {
          if (lik[z] == 0 || md2v[z] > thr) { Mvalid[(size_t)m * nZ + z] = 0; W[(size_t)m * nZ + z] = 0; }
          else { Mvalid[(size_t)m * nZ + z] = 1; Mtab[(size_t)m * nZ + z] = lmNew[z]; W[(size_t)m * nZ + z] = Pd_times_w_km * lik[z]; }
        }
      }
    }
    for (int z = 0; z < nZ; z++) {
      double clutter = model.clutter();
      double sum = clutter;
      for (unsigned m = 0; m < nM; m++) sum += W[(size_t)m * nZ + z];
      if (cfg.useClusterProcess) likelihoodProd *= sum;
      for (unsigned m = 0; m < nM; m++) W[(size_t)m * nZ + z] = W[(size_t)m * nZ + z] / sum;
    }
    if (cfg.useClusterProcess) {
      double prev = weight[i];
      weight[i] = exp(w_km_sum) * likelihoodProd * prev;
    }
    /* 3. add new Gaussians in (m,z) row-major order (:675-683); addGaussian => w_prev = 0 */
    for (unsigned m = 0; m < nM; m++)
      for (int z = 0; z < nZ; z++)
        if (Mvalid[(size_t)m * nZ + z] && W[(size_t)m * nZ + z] > 0) {
          Gauss g = Mtab[(size_t)m * nZ + z];
          g.valid = true; g.w = W[(size_t)m * nZ + z]; g.w_prev = 0;
          G.push_back(g);
          gm_n[i]++;
        }
    /* 4. missed-detection weights (:686-706); setWeight stores the old weight in w_prev */
    for (unsigned m = 0; m < nM; m++) {
      double w_km = G[m].w;
      double w_k = (1 - Pd[m]) * w_km;
      if (closeLim[m] == 1 && w_km > cfg.birthGaussianWeight) {
        double weight_sum_m = 0;
        for (int z = 0; z < nZ; z++) weight_sum_m += W[(size_t)m * nZ + z];
        double delta_w = Pd[m] * w_km - weight_sum_m;
        if (delta_w > 0) { w_k += delta_w; if (w_k > 1) w_k = 1; }
      }
      G[m].w_prev = G[m].w;
      G[m].w = w_k;
    }
    /* 5. unused measurements (:709-720) */
    unused[i].clear();
    for (int z = 0; z < nZ; z++) {
      bool used = false;
      for (unsigned m = 0; m < nM; m++) if (W[(size_t)m * nZ + z] != 0) { used = true; break; }
      if (!used) unused[i].push_back(z);
    }
  }

  /* GaussianMixture::sortByWeight (include/GaussianMixture.hpp:523-534). */
  static bool weightCompare(const Gauss &a, const Gauss &b) { return a.w > b.w; }
  void sort_by_weight(std::vector<Gauss> &G) {
    if (stable_sort) std::stable_sort(G.begin(), G.end(), weightCompare);
    else std::sort(G.begin(), G.end(), weightCompare);
  }

  /* RBPHDFilter::rfsMeasurementLikelihood (include/RBPHDFilter.hpp:821-997). */
  double rfs_measurement_likelihood(int i, const std::vector<unsigned> &evalPtIdx, const std::vector<double> &evalPtPd, long *mc, long *lr) {
    const Pose &x = pose[i];
    const int nE = (int)evalPtIdx.size();
    const double threshold = cfg.importanceWeightingMeasurementLikelihoodMDThreshold * cfg.importanceWeightingMeasurementLikelihoodMDThreshold;
    CostMatrixGeneral cm(nE, nZ);
    MatD zeroCov = zeroM<D>();
    for (int m = 0; m < nE; m++) {
      const Gauss &ev = gm[i][evalPtIdx[m]];
      double z_exp[D];
      MatD S;
      model.measure(x, ev.x, zeroCov, z_exp, S, nullptr); /* evalPt_copy.setCov(Zero); return value ignored (:850-852) */
      double Pd = evalPtPd[m];
      for (int nn = 0; nn < nZ; nn++) {
        double m2;
        double L = gauss_lik<D>(z_exp, S, &Z[(size_t)D * nn], &m2) * Pd;
        if (m2 > threshold) L = 0;
        cm.C_[m][nn] = L;
      }
    }
    std::vector<double> clutter(nZ);
    for (int nn = 0; nn < nZ; nn++) clutter[nn] = model.clutter();
    double l = partitions_likelihood(cm, evalPtPd, clutter, mc, lr, exact_partitions);
    return l / model.clutter_integral();
  }

  /* RBPHDFilter::importanceWeighting (include/RBPHDFilter.hpp:728-819) for one particle. */
  void importance_weighting_particle(int idx, long *mc, long *lr) {
    const Pose &x = pose[idx];
    std::vector<Gauss> &G = gm[idx];
    const unsigned nM = gm_n[idx];
    int nEvalPoints = (unsigned)cfg.importanceWeightingEvalPointCount > nM ? (int)nM : cfg.importanceWeightingEvalPointCount;
    std::vector<unsigned> evalPointIdx;
    std::vector<double> evalPointPd;
    if (nEvalPoints == 0) {
      weight[idx] = std::numeric_limits<double>::denorm_min();
      return;
    }
    sort_by_weight(G);
    for (unsigned m = 0; m < nM; m++) {
      double w = G[m].w;
      if (w < cfg.importanceWeightingEvalPointGuassianWeight) break;
      bool close;
      double Pd = model.pd(x, G[m].x, G[m].S, close);
      if (Pd > 0) { evalPointIdx.push_back(m); evalPointPd.push_back(Pd); }
      if (nEvalPoints != -1 && evalPointIdx.size() >= (size_t)nEvalPoints) break;
    }
    nEvalPoints = (int)evalPointIdx.size();
    double sumBefore = 0, sumAfter = 0;
    for (unsigned m = 0; m < nM; m++) { sumBefore += G[m].w_prev; sumAfter += G[m].w; }
    double prodBefore = 1, prodAfter = 1;
    for (int e = 0; e < nEvalPoints; e++) {
      const Gauss &ev = G[evalPointIdx[e]];
      double ib = std::numeric_limits<double>::denorm_min();
      double ia = std::numeric_limits<double>::denorm_min();
      for (unsigned m = 0; m < nM; m++) {
        double likelihood = gauss_lik<D>(G[m].x, G[m].S, ev.x, nullptr);
        ib += G[m].w_prev * likelihood;
        ia += G[m].w * likelihood;
      }
      prodBefore *= ib;
      prodAfter *= ia;
    }
    double measurementLikelihood = rfs_measurement_likelihood(idx, evalPointIdx, evalPointPd, mc, lr);
    double overall_weight = measurementLikelihood * prodBefore / prodAfter * exp(sumAfter - sumBefore);
    double prev_weight = weight[idx];
    weight[idx] = overall_weight * prev_weight;
  }

  /* GaussianMixture::merge(idx1, idx2)  (include/GaussianMixture.hpp:419-475). */
  bool merge_pair(std::vector<Gauss> &G, int &n_, unsigned i1, unsigned i2, double t, double f) {
    if (!G[i1].valid || !G[i2].valid) return false;
    double w_1 = G[i1].w, w_2 = G[i2].w;
    double t2 = t * t;
    double d1 = md2<D>(G[i1].x, inv(G[i1].S), G[i2].x);
    if (d1 > t2) {
      double d2 = md2<D>(G[i2].x, inv(G[i2].S), G[i1].x);
      if (d2 > t2) return false;
    }
    double w_m = w_1 + w_2;
    if (w_m == 0) return false;
    double x_m[D], d_1[D], d_2[D];
    for (int k = 0; k < D; k++) x_m[k] = (G[i1].x[k] * w_1 + G[i2].x[k] * w_2) / w_m;
    for (int k = 0; k < D; k++) { d_1[k] = x_m[k] - G[i1].x[k]; d_2[k] = x_m[k] - G[i2].x[k]; }
    MatD S_m;
    for (int r = 0; r < D; r++)
      for (int c = 0; c < D; c++) {
        /* S_m = ( w_1*(S_1 + f*d_1*d_1^T) + w_2*(S_2 + f*d_2*d_2^T) ) / w_m ; (f*d) is formed first */
        double a = w_1 * (G[i1].S(r, c) + (f * d_1[r]) * d_1[c]);
        double b = w_2 * (G[i2].S(r, c) + (f * d_2[r]) * d_2[c]);
        S_m(r, c) = (a + b) / w_m;
      }
    for (int k = 0; k < D; k++) G[i1].x[k] = x_m[k];
    G[i1].S = S_m;
    G[i1].w = w_m;
    G[i1].w_prev = 0;
    G[i2].valid = false; G[i2].w = 0; G[i2].w_prev = 0; /* removeGaussian(idx2) (:310-322) */
    n_--;
    return true;
  }
  /* GaussianMixture::merge(t, f)  (:394-416). */
  void merge_particle(int i) {
    std::vector<Gauss> &G = gm[i];
    unsigned nG = G.size();
    for (unsigned a = 0; a < nG; a++) {
      if (!G[a].valid) continue;
      for (unsigned b = a + 1; b < nG; b++) merge_pair(G, gm_n[i], a, b, cfg.gaussianMergingThreshold, cfg.gaussianMergingCovarianceInflationFactor);
    }
  }
  /* GaussianMixture::prune(t)  (:477-521), binary search + linear walk restated literally. */
  void prune_particle(int i) { prune_particle_t(i, cfg.gaussianPruningThreshold); }
  void prune_particle_t(int i, const double t) { /* GaussianMixture::prune(t) :477-521 */
    std::vector<Gauss> &G = gm[i];
    unsigned nPruned = 0;
    if (G.size() < 1) return;
    sort_by_weight(G);
    unsigned min_idx = 0, max_idx = G.size() - 1;
    unsigned idx = (max_idx + min_idx) / 2;
    unsigned idx_old = idx + 1;
    double w = G[idx].w;
    while (idx != idx_old) {
      if (w <= t) max_idx = idx;
      else if (w > t) min_idx = idx;
      idx_old = idx;
      idx = (max_idx + min_idx) / 2;
      w = G[idx].w;
    }
    while (w >= t) {
      idx++;
      if (idx >= G.size()) break;
      w = G[idx].w;
    }
    while (idx < G.size()) {
      if (G[idx].valid) { G[idx].valid = false; G[idx].w = 0; G[idx].w_prev = 0; gm_n[i]--; }
      idx++;
      nPruned++;
    }
    G.resize(G.size() - nPruned);
  }

  void add_gaussian(int i, const double *x, const MatD &S, double w) { /* GaussianMixture::addGaussian(p, w, true) :267-284 */
    Gauss g;
    g.valid = true; g.w = w; g.w_prev = 0;
    for (int k = 0; k < D; k++) g.x[k] = x[k];
    g.S = S;
    gm[i].push_back(g);
    gm_n[i]++;
  }
  /* RBPHDFilter::addBirthGaussians (include/RBPHDFilter.hpp:1000-1084) for one particle (the parent-state copy at
   * :1005-1011 is done when the resample plan is applied).  The promotion loop (:1062-1080) increments the iterator after
   * erase() may have returned end(): with libstdc++'s circular std::list, ++end() is begin(), so when the LAST candidate
   * is erased while others remain the loop wraps and visits the survivors again.  Restated as that behaviour. */
  void add_birth_particle(int i) {
    std::list<Candidate> &L = cand[i];
    while (unused[i].size() > 0) {
      int zi = unused[i].back();
      const double *uz = &Z[(size_t)D * zi];
      unused[i].pop_back();
      bool isNew = true;
      for (auto it = L.begin(); it != L.end(); it++) {
        double z_exp[D];
        MatD S;
        model.measure(pose[i], it->x, it->S, z_exp, S, nullptr);
        double d2 = md2<D>(z_exp, inv(S), uz); /* z_exp.mahalanobisDist2(unused_z) */
        if (d2 <= cfg.birthGaussianMeasurementSupportDist * cfg.birthGaussianMeasurementSupportDist) {
          kf_correct_one(pose[i], uz, it->x, it->S, it->x, it->S);
          (it->nSupportingMeasurements)++;
          isNew = false;
          break;
        }
      }
      if (isNew) {
        Candidate c;
        c.nSupportingMeasurements = 1;
        c.nChecks = 0;
        model.inverse_measure(pose[i], uz, c.x, c.S);
        if (cfg.birthGaussianMeasurementCountThreshold == 1 || nInFov[i] <= cfg.birthGaussianCurrentMeasurementCountThreshold)
          add_gaussian(i, c.x, c.S, cfg.birthGaussianWeight);
        else
          L.push_back(c);
      }
    }
    auto it = L.begin();
    while (it != L.end()) {
      it->nChecks++;
      while (it->nSupportingMeasurements >= cfg.birthGaussianMeasurementCountThreshold || it->nChecks > cfg.birthGaussianMeasurementCheckThreshold ||
             nInFov[i] <= cfg.birthGaussianCurrentMeasurementCountThreshold) {
        if (it->nSupportingMeasurements >= cfg.birthGaussianMeasurementCountThreshold) add_gaussian(i, it->x, it->S, cfg.birthGaussianWeight);
        else if (nInFov[i] <= cfg.birthGaussianCurrentMeasurementCountThreshold) add_gaussian(i, it->x, it->S, cfg.birthGaussianWeight);
        it = L.erase(it);
        if (it != L.end()) it->nChecks++;
        else break;
      }
      if (it == L.end()) it = L.begin(); /* for-loop's it++ on end(): wraps to begin() (== end() when the list is empty) */
      else ++it;
    }
  }

  /* FastSLAM::updateMap (include/FastSLAM.hpp:424-706), split the way the reference's own control flow falls apart:
   * (1) data association of one particle -> up to maxNDataAssocHypotheses_ assignments (:430-541), (2) particle copies for
   * the extra hypotheses (:543-556, ParticleFilter::copyParticle), (3) the map / weight update of one particle under one
   * assignment (:559-703). */
  struct FsAssoc {
    std::vector<int> idx_inRange;
    std::vector<double> pd_inRange;
    std::vector<std::vector<double>> T;     /* likelihoodTable after reduce() */
    std::vector<std::vector<int>> da;       /* da[h][m] */
  };
  void fastslam_associate(int i, FsAssoc &A) {
    const int nZl = nZ;
    const Pose &ps = pose[i];
    std::vector<Gauss> &G = gm[i];
    unsigned nM = gm_n[i];
    std::vector<int> &idx_inRange = A.idx_inRange;
    std::vector<double> &pd_inRange = A.pd_inRange;
    for (unsigned m = 0; m < nM; m++) { /* :440-449 */
      bool closeToLimit = false;
      double pd = model.pd(ps, G[m].x, G[m].S, closeToLimit);
      if (pd != 0 || closeToLimit) { idx_inRange.push_back((int)m); pd_inRange.push_back(pd); }
    }
    nM = idx_inRange.size();
    unsigned nMZ = nM;
    if ((unsigned)nZl > nM) nMZ = nZl;
    const double lim = fs.minLogMeasurementLikelihood;
    std::vector<std::vector<double>> &T = A.T;
    T.assign(nMZ, std::vector<double>(nMZ, lim)); /* :458-465 */
    for (unsigned m = 0; m < nM; m++) {           /* :468-481 */
      const Gauss &lm = G[idx_inRange[m]];
      double z_exp[D];
      MatD S;
      bool ok = model.measure(ps, lm.x, lm.S, z_exp, S, nullptr);
      for (int z = 0; z < nZl; z++)
        if (ok) T[m][z] = fmax(lim, log(gauss_lik<D>(z_exp, S, &Z[(size_t)D * z], nullptr)));
    }
    ReducedCost R = cost_matrix_reduce(T, (int)nMZ, lim); /* :484-490 */
    fs_last_nMZ[i] = (int)nMZ; /* (each particle writes its own entry) */
    fs_last_nRed[i] = R.nRed;
    if (R.nRed == 0) {                                     /* :498-505 */
      std::vector<int> da(nMZ, -1);
      for (unsigned m = 0; m < nM; m++) da[m] = R.a_fixed[m];
      A.da.push_back(da);
      fs_last_nH[i] = 1;
      return;
    }
    std::vector<std::vector<double>> Cr(R.nRed, std::vector<double>(R.nRed));
    std::vector<double *> rows(R.nRed);
    for (int a = 0; a < R.nRed; a++) {
      for (int b = 0; b < R.nRed; b++) Cr[a][b] = T[R.iRed[a]][R.jRed[b]];
      rows[a] = Cr[a].data();
    }
#pragma omp critical(fs_counters)
    {
      fs_solver_calls++;
      /* rows / columns of the reduced table that still have a possibility (the rest only see the floor) */
      int live = 0;
      for (int a = 0; a < R.nRed; a++) { bool any = false; for (int b = 0; b < R.nRed; b++) any |= Cr[a][b] > lim; live += any; }
      if (live > fs_solver_max_dim) fs_solver_max_dim = live;
    }
    Murty murty(rows.data(), R.nRed);
    unsigned nH = 0;                                       /* :506-541 */
    double bestScore = 0;
    while (nH < fs.maxNDataAssocHypotheses) {
      std::vector<int> daVar;
      double logLikelihoodSum = 0;
      const unsigned nH_old = nH;
      const int k = murty.findNextBest(daVar, logLikelihoodSum);
      if (k == -1) { nH = nH_old; break; }
      nH = (unsigned)k;
      if (k == 1) bestScore = logLikelihoodSum;            /* Murty::getBestScore() */
      if (bestScore - logLikelihoodSum >= fs.maxDataAssocLogLikelihoodDiff) { nH--; break; }
      std::vector<int> da(nMZ, -1);
      for (unsigned m = 0; m < nM; m++) da[m] = R.a_fixed[m];
      for (int m = 0; m < R.nRed; m++) {
        int z_o = R.jRed[daVar[m]];
        int m_o = R.iRed[m];
        da[m_o] = (z_o < nZl) ? z_o : -2;
      }
      A.da.push_back(da);
    }
    fs_last_nH[i] = (int)A.da.size();
    /* nH == 0 (the solver failed at once): no hypothesis, the particle is left untouched (:543-551 runs 0 times) */
  }
  void fastslam_apply(int i, const FsAssoc &A, const std::vector<int> &da) {
    const int nZl = nZ;
    const Pose &ps = pose[i];
    std::vector<Gauss> &G = gm[i];
    const std::vector<int> &idx_inRange = A.idx_inRange;
    const std::vector<double> &pd_inRange = A.pd_inRange;
    const std::vector<std::vector<double>> &T = A.T;
    const unsigned nM = idx_inRange.size();
    const double lim = fs.minLogMeasurementLikelihood;
    /* one hypothesis: :559-703 */
    const double nExpectedClutter = model.clutter_integral();
    const double probFalseAlarm = nExpectedClutter / nZl;
    double p_exist_given_Z = 0;
    double logParticleWeight = 0;
    nInFov[i] = 0;
    std::vector<char> zUsed(nZl, 0);
    const double prior = fs.landmarkExistencePrior;
    for (unsigned m = 0; m < nM; m++) { /* :573-604 */
      Gauss &lm = G[idx_inRange[m]];
      int z = da[m];
      bool isUpdatePerformed = false;
      if (z < nZl && z >= 0 && T[m][z] > lim) isUpdatePerformed = kf_correct_one(ps, &Z[(size_t)D * z], lm.x, lm.S, lm.x, lm.S);
      double w = lm.w;
      if (isUpdatePerformed) {
        nInFov[i]++;
        zUsed[z] = 1;
        logParticleWeight += T[m][z];
        p_exist_given_Z = ((1 - pd_inRange[m]) * probFalseAlarm * prior + pd_inRange[m] * prior) /
                          (probFalseAlarm + (1 - probFalseAlarm) * pd_inRange[m] * prior);
      } else {
        p_exist_given_Z = ((1 - pd_inRange[m]) * prior) / ((1 - prior) + (1 - pd_inRange[m]) * prior);
        if (w > fs.landmarkLockWeight) p_exist_given_Z = 0.5;
      }
      w += log((p_exist_given_Z) / (1 - p_exist_given_Z));
      lm.w_prev = lm.w; /* setWeight keeps the previous value (GaussianMixture.hpp:368-375) */
      lm.w = w;
    }
    if ((unsigned)nZl >= fs.pruningMeasurementsThreshold) prune_particle_t(i, fs.mapExistencePruneThreshold); /* :611-612 */
    const double newLandmarkWeight = log(prior / (1 - prior));
    std::list<Candidate> &L = cand[i];
    for (int z = 0; z < nZl; z++) { /* :615-690 */
      if (zUsed[z]) continue;
      const double *uz = &Z[(size_t)D * z];
      bool isNewCandidate = true;
      for (auto it = L.begin(); it != L.end(); it++) {
        double z_exp[D];
        MatD S;
        model.measure(ps, it->x, it->S, z_exp, S, nullptr);
        double d2 = md2<D>(z_exp, inv(S), uz);
        if (d2 <= fs.landmarkCandidateMeasurementSupportDist * fs.landmarkCandidateMeasurementSupportDist) {
          kf_correct_one(ps, uz, it->x, it->S, it->x, it->S);
          (it->nSupportingMeasurements)++;
          isNewCandidate = false;
          break;
        }
      }
      if (isNewCandidate) {
        Candidate c;
        c.nSupportingMeasurements = 1;
        c.nChecks = 0;
        model.inverse_measure(ps, uz, c.x, c.S);
        if (fs.landmarkCandidateMeasurementCountThreshold == 1 || nInFov[i] <= fs.landmarkCandidateCurrentMeasurementCountThreshold)
          add_gaussian(i, c.x, c.S, newLandmarkWeight);
        else
          L.push_back(c);
      }
      /* the promotion loop sits INSIDE the unused-measurement loop (:656-688); ++it after erase() returned end() wraps
       * to begin() with libstdc++'s circular list, as in addBirthGaussians */
      auto it = L.begin();
      while (it != L.end()) {
        it->nChecks++;
        while (it->nSupportingMeasurements >= fs.landmarkCandidateMeasurementCountThreshold || it->nChecks > fs.landmarkCandidateMeasurementCheckThreshold ||
               nInFov[i] <= fs.landmarkCandidateCurrentMeasurementCountThreshold) {
          if (it->nSupportingMeasurements >= fs.landmarkCandidateMeasurementCountThreshold) add_gaussian(i, it->x, it->S, newLandmarkWeight * it->nChecks);
          else if (nInFov[i] <= fs.landmarkCandidateCurrentMeasurementCountThreshold) add_gaussian(i, it->x, it->S, newLandmarkWeight * it->nChecks);
          it = L.erase(it);
          if (it != L.end()) it->nChecks++;
          else break;
        }
        if (it == L.end()) it = L.begin();
        else ++it;
      }
    }
    weight[i] = weight[i] * exp(logParticleWeight); /* :696-697 */
  }
  int fastslam_update() override {
    const int n0 = n; /* stopIdx: particles added during this update are not visited (:389-391) */
    std::vector<FsAssoc> assoc(n0);
    fs_last_nMZ.assign(n0, 0);
    fs_last_nRed.assign(n0, 0);
    fs_last_nH.assign(n0, 0);
#pragma omp parallel for schedule(dynamic, 4)
    for (int i = 0; i < n0; i++) fastslam_associate(i, assoc[i]);
    /* landmarkCandidates_.resize(nParticles * maxNDataAssocHypotheses) (:392-395): only ever grows, old lists stay */
    if (cand.size() < (size_t)n0 * fs.maxNDataAssocHypotheses) cand.resize((size_t)n0 * fs.maxNDataAssocHypotheses);
    /* particle copies, in particle order (the reference does this inside an omp critical section, i.e. in arrival order;
     * its single-threaded order is restated): pi[0] = i, pi[h] = nParticles_ - h after the copies (:543-556) */
    std::vector<std::vector<int>> pi(n0);
    parents.resize(n0);
    for (int i = 0; i < n0; i++) parents[i] = i;
    for (int i = 0; i < n0; i++) {
      const int nH = (int)assoc[i].da.size();
      pi[i].assign(nH > 0 ? nH : 1, i);
      if (nH > 1) {
        const double newWeight = weight[i] / nH;
        weight[i] = newWeight;
        for (int c = 0; c < nH - 1; c++) { /* ParticleFilter::copyParticle (ParticleFilter.hpp:273-294) */
          pose.push_back(pose[i]);
          weight.push_back(newWeight);
          gm.push_back(gm[i]);
          gm_n.push_back(gm_n[i]);
          unused.push_back(unused[i]);
          nInFov.push_back(nInFov[i]);
          parents.push_back(i);
          n++;
          if (cand.size() < (size_t)n) cand.resize(n);
        }
        for (int h = 1; h < nH; h++) {
          pi[i][h] = n - h;
          if (fs_resample_occured) cand[pi[i][h]] = cand[pi[i][0]];
        }
      }
    }
    /* the updates, one per (particle, hypothesis) */
    std::vector<std::pair<int, int>> work;
    for (int i = 0; i < n0; i++)
      for (int h = 0; h < (int)assoc[i].da.size(); h++) work.push_back({i, h});
#pragma omp parallel for schedule(dynamic, 4)
    for (int t = 0; t < (int)work.size(); t++) {
      const int i = work[t].first, h = work[t].second;
      fastslam_apply(pi[i][h], assoc[i], assoc[i].da[h]);
    }
    return RFSGPU_OK;
  }

  /* ---- FilterBase ---- */
  int gm_size(int slot) override { return gm_n[slot]; }
  void import_gm(int slot, int cnt, const double *w, const double *mean, const double *cov) override {
    gm[slot].clear();
    for (int m = 0; m < cnt; m++) {
      Gauss g;
      g.valid = true; g.w = w[m]; g.w_prev = 0;
      for (int k = 0; k < D; k++) g.x[k] = mean[D * m + k];
      memcpy(g.S.a, cov + (size_t)D * D * m, D * D * sizeof(double));
      gm[slot].push_back(g);
    }
    gm_n[slot] = cnt;
  }
  int export_gm(int slot, int max_n, double *w, double *wp, double *mean, double *cov) override {
    int k = 0;
    for (const Gauss &g : gm[slot]) {
      if (!g.valid) continue;
      if (k < max_n) {
        if (w) w[k] = g.w;
        if (wp) wp[k] = g.w_prev;
        if (mean) for (int d = 0; d < D; d++) mean[D * k + d] = g.x[d];
        if (cov) memcpy(cov + (size_t)D * D * k, g.S.a, D * D * sizeof(double));
      }
      k++;
    }
    return k;
  }
  int get_landmark(int slot, int m, double *mean, double *cov, double *w) override {
    if (m < 0 || m >= gm_n[slot] || m >= (int)gm[slot].size()) return RFSGPU_ERR_INVALID;
    const Gauss &g = gm[slot][m];
    for (int d = 0; d < D; d++) mean[d] = g.x[d];
    memcpy(cov, g.S.a, D * D * sizeof(double));
    *w = g.w;
    return RFSGPU_OK;
  }
  int predict_map(int add_birth) override {
    long long t0 = now_ns();
    ensure_ids();
    for (int i = 0; i < n; i++) {
      if (add_birth && inherit_mode == RFSGPU_INHERIT_REFERENCE && !fastslam_handle && resample_occured) { /* :1005-1011, slot by slot, as written */
        const unsigned i_prev = ppid[i];
        if (i_prev != (unsigned)i && i_prev < unused.size() && i_prev < cand.size()) {
          unused[i] = unused[i_prev];
          cand[i] = cand[i_prev];
        }
      }
      if (add_birth) add_birth_particle(i);
      for (Gauss &g : gm[i]) /* staticStep: S += Q (include/ProcessModel.hpp:195-208) */
        for (int k = 0; k < D * D; k++) g.S.a[k] += Qlm.a[k];
    }
    timing.predict_wall += now_ns() - t0;
    return RFSGPU_OK;
  }
  /* One level of the level-ordered form of predict's birth step (the multi-GPU hosts, which move the per-slot lists between
   * shards themselves): the birth step of the slots whose level is `level`; the static step of EVERY Gaussian in the call
   * with do_static, later births receive their + Q where they are created (a predict adds Q to births and old Gaussians alike). */
  int predict_map_level(int add_birth, const int *level_of_slot, int level, int do_static) override {
    for (int i = 0; i < n; i++) {
      const size_t n0 = gm[i].size();
      if (add_birth && level_of_slot[i] == level) add_birth_particle(i);
      const size_t from = do_static ? 0 : n0;
      for (size_t m = from; m < gm[i].size(); m++)
        for (int k = 0; k < D * D; k++) gm[i][m].S.a[k] += Qlm.a[k];
    }
    return RFSGPU_OK;
  }
  void update_map() override {
    long long t0 = now_ns();
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; i++) update_map_particle(i);
    timing.mapUpdate_wall += now_ns() - t0;
  }
  void importance_weighting() override {
    long long t0 = now_ns();
    long mc = 0, lr = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : mc, lr)
    for (int i = 0; i < n; i++) importance_weighting_particle(i, &mc, &lr);
    murty_calls += mc; lonerow_bug_hits += lr;
    timing.particleWeighting_wall += now_ns() - t0;
  }
  void merge() override {
    long long t0 = now_ns();
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; i++) merge_particle(i);
    timing.mapMerge_wall += now_ns() - t0;
  }
  void prune() override {
    long long t0 = now_ns();
#pragma omp parallel for schedule(dynamic, 1)
    for (int i = 0; i < n; i++) prune_particle(i);
    timing.mapPrune_wall += now_ns() - t0;
  }
  void copy_particle(int dst, int src) override {
    gm[dst] = gm[src]; gm_n[dst] = gm_n[src];
    unused[dst] = unused[src]; nInFov[dst] = nInFov[src];
    cand[dst] = cand[src]; /* birthGaussians_[i] = birthGaussians_[i_prev] (:1005-1011) */
  }
  void copy_map(int dst, int src) override { gm[dst] = gm[src]; gm_n[dst] = gm_n[src]; }
  void set_lmk_noise(const double *Q) override { memcpy(Qlm.a, Q, D * D * sizeof(double)); }
  void shrink(int n_out) override {
    n = n_out;
    pose.resize(n); weight.resize(n); gm.resize(n); gm_n.resize(n); unused.resize(n); nInFov.resize(n);
    /* cand (landmarkCandidates_ / birthGaussians_) keeps its size: stale lists stay in the slots beyond n */
  }
  int export_candidates(int slot, int max_n, double *mean, double *cov, int *support, int *checks) override {
    int k = 0;
    for (const Candidate &c : cand[slot]) {
      if (k < max_n) {
        for (int d = 0; d < D; d++) mean[D * k + d] = c.x[d];
        memcpy(cov + (size_t)D * D * k, c.S.a, D * D * sizeof(double));
        support[k] = (int)c.nSupportingMeasurements;
        checks[k] = (int)c.nChecks;
      }
      k++;
    }
    return k;
  }
  void import_candidates(int slot, int cnt, const double *mean, const double *cov, const int *support, const int *checks) override {
    cand[slot].clear();
    for (int k = 0; k < cnt; k++) {
      Candidate c;
      for (int d = 0; d < D; d++) c.x[d] = mean[D * k + d];
      memcpy(c.S.a, cov + (size_t)D * D * k, D * D * sizeof(double));
      c.nSupportingMeasurements = (unsigned)support[k];
      c.nChecks = (unsigned)checks[k];
      cand[slot].push_back(c);
    }
  }
};

} /* namespace orc */

/* ================================================================================================
 * C API: same shape as include/rfsgpu.h with prefix rfsor_, so one ctypes wrapper drives both.
 * ============================================================================================== */
using orc::FilterBase;
#define F_(f) (reinterpret_cast<FilterBase *>(f))
#define FRB_(f) (dynamic_cast<orc::FilterT<orc::ModelRB> *>(F_(f)))
#define FVP_(f) (dynamic_cast<orc::FilterT<orc::ModelVP> *>(F_(f)))

extern "C" {

int rfsor_abi_version(void) { return RFSGPU_ABI_VERSION; }

void rfsor_default_filter_config(rfsgpu_filter_config *c) { /* RBPHDFilter.hpp:370-382 */
  memset(c, 0, sizeof(*c));
  c->birthGaussianWeight = 0.25;
  c->birthGaussianMeasurementCountThreshold = 1;
  c->birthGaussianMeasurementCheckThreshold = 1;
  c->birthGaussianMeasurementSupportDist = 1;
  c->birthGaussianCurrentMeasurementCountThreshold = 1;
  c->gaussianMergingThreshold = 0.5;
  c->gaussianMergingCovarianceInflationFactor = 1.5;
  c->gaussianPruningThreshold = 0.2;
  c->importanceWeightingEvalPointCount = 8;
  c->importanceWeightingEvalPointGuassianWeight = 0; /* uninitialised in the reference ctor */
  c->importanceWeightingMeasurementLikelihoodMDThreshold = 3.0;
  c->newGaussianCreateInnovMDThreshold = 0.2;
  c->minUpdatesBeforeResample = 1;
  c->minMeasurementsBeforeResample = 1;
  c->useClusterProcess = 0;
}

int rfsor_create(void **out, int model, int n_particles, int device_id, int gm_capacity) {
  (void)device_id; (void)gm_capacity;
  if (!out || n_particles <= 0) return RFSGPU_ERR_INVALID;
  FilterBase *F = nullptr;
  if (model == RFSGPU_MODEL_RNGBRG_2D) F = new orc::FilterT<orc::ModelRB>(n_particles);
  else if (model == RFSGPU_MODEL_VICTORIAPARK_3D) F = new orc::FilterT<orc::ModelVP>(n_particles);
  else return RFSGPU_ERR_INVALID;
  rfsor_default_filter_config(&F->cfg);
  *out = F;
  return RFSGPU_OK;
}
int rfsor_create_ex(void **out, int model, int n_particles, int device_id, int gm_capacity, int max_particles) {
  if (max_particles < n_particles) return RFSGPU_ERR_INVALID;
  return rfsor_create(out, model, n_particles, device_id, gm_capacity); /* the CPU state grows on demand */
}
int rfsor_n_particles(const void *f) { return f ? reinterpret_cast<const FilterBase *>(f)->n : -1; }
int rfsor_max_particles(const void *f) { return f ? 1 << 30 : -1; }
void rfsor_destroy(void *f) { delete F_(f); }
const char *rfsor_last_error(const void *f) { return f ? reinterpret_cast<const FilterBase *>(f)->err.c_str() : "null handle"; }

int rfsor_set_filter_config(void *f, const rfsgpu_filter_config *c) { F_(f)->cfg = *c; return RFSGPU_OK; }
int rfsor_set_partition_mode(void *f, int mode) { F_(f)->exact_partitions = mode == RFSGPU_PARTITION_EXACT; return RFSGPU_OK; }
int rfsor_get_filter_config(const void *f, rfsgpu_filter_config *c) { *c = reinterpret_cast<const FilterBase *>(f)->cfg; return RFSGPU_OK; }
int rfsor_set_model_rngbrg(void *f, const rfsgpu_rngbrg_config *c) {
  auto *F = FRB_(f);
  if (!F) return RFSGPU_ERR_INVALID;
  F->model.c = *c;
  return RFSGPU_OK;
}
int rfsor_set_model_victoriapark(void *f, const rfsgpu_vp_config *c) {
  auto *F = FVP_(f);
  if (!F) return RFSGPU_ERR_INVALID;
  F->model.c = *c;
  return RFSGPU_OK;
}
int rfsor_set_laser_scan(void *f, const double *scan, int n) {
  auto *F = FVP_(f);
  if (!F || n <= 0) return RFSGPU_ERR_INVALID;
  F->model.set_scan(scan, n);
  return RFSGPU_OK;
}
int rfsor_set_kf_config(void *f, const rfsgpu_kf_config *c) {
  if (auto *F = FRB_(f)) { F->model.kf = *c; return RFSGPU_OK; }
  if (auto *F = FVP_(f)) { F->model.kf = *c; return RFSGPU_OK; }
  return RFSGPU_ERR_INVALID;
}
int rfsor_set_lmk_process_noise(void *f, const double *Q) { F_(f)->set_lmk_noise(Q); return RFSGPU_OK; }

int rfsor_set_poses(void *f, const double *x, const double *cov, int cov_stride) {
  FilterBase *F = F_(f);
  for (int i = 0; i < F->n; i++) {
    memcpy(F->pose[i].x, x + 3 * i, 3 * sizeof(double));
    if (cov) memcpy(F->pose[i].P, cov + (size_t)cov_stride * i, 9 * sizeof(double));
    else memset(F->pose[i].P, 0, 9 * sizeof(double));
  }
  return RFSGPU_OK;
}
int rfsor_get_poses(void *f, double *x) {
  FilterBase *F = F_(f);
  for (int i = 0; i < F->n; i++) memcpy(x + 3 * i, F->pose[i].x, 3 * sizeof(double));
  return RFSGPU_OK;
}
int rfsor_set_weights(void *f, const double *w) { FilterBase *F = F_(f); F->weight.assign(w, w + F->n); return RFSGPU_OK; }
int rfsor_get_weights(void *f, double *w) { FilterBase *F = F_(f); memcpy(w, F->weight.data(), F->n * sizeof(double)); return RFSGPU_OK; }

int rfsor_gm_size(void *f, int slot) { FilterBase *F = F_(f); return (slot >= 0 && slot < F->n) ? F->gm_size(slot) : -1; }
int rfsor_gm_sizes(void *f, int *sizes) { FilterBase *F = F_(f); for (int i = 0; i < F->n; i++) sizes[i] = F->gm_size(i); return RFSGPU_OK; }

int rfsor_import_gm(void *f, int slot, int n, const double *w, const double *mean, const double *cov) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n || n < 0) return RFSGPU_ERR_INVALID;
  F->import_gm(slot, n, w, mean, cov);
  return RFSGPU_OK;
}
/* Exports VALID Gaussians in storage order (holes skipped). */
int rfsor_export_gm(void *f, int slot, int max_n, int *n_out, double *w, double *w_prev, double *mean, double *cov) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  int k = F->export_gm(slot, max_n, w, w_prev, mean, cov);
  if (n_out) *n_out = k;
  return RFSGPU_OK;
}
int rfsor_get_landmark(void *f, int slot, int m, double *mean, double *cov, double *w) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  return F->get_landmark(slot, m, mean, cov, w);
}
int rfsor_import_aux(void *f, int slot, const int *unused_idx, int n_unused, int n_in_fov) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  F->unused[slot].assign(unused_idx, unused_idx + n_unused);
  F->nInFov[slot] = (unsigned)n_in_fov;
  return RFSGPU_OK;
}
int rfsor_export_birth_candidates(void *f, int slot, int max_n, int *n_out, double *mean, double *cov, int *support, int *checks) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  int k = F->export_candidates(slot, max_n, mean, cov, support, checks);
  if (n_out) *n_out = k;
  return RFSGPU_OK;
}
int rfsor_import_birth_candidates(void *f, int slot, int n, const double *mean, const double *cov, const int *support, const int *checks) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n || n < 0) return RFSGPU_ERR_INVALID;
  F->import_candidates(slot, n, mean, cov, support, checks);
  if (n > 0) F->cand_used = true;
  return RFSGPU_OK;
}
int rfsor_has_birth_candidates(const void *f) { return f ? (reinterpret_cast<const FilterBase *>(f)->cand_used ? 1 : 0) : -1; }

int rfsor_predict_map(void *f, int add_birth) { return F_(f)->predict_map(add_birth); }
int rfsor_predict_map_level(void *f, int add_birth, const int *level_of_slot, int level, int do_static) {
  if (!level_of_slot) return RFSGPU_ERR_INVALID;
  FilterBase *F = F_(f);
  F->cand_used = F->cand_used || F->cfg.birthGaussianMeasurementCountThreshold != 1u;   /* (as the engine: lists exist from here on) */
  return F->predict_map_level(add_birth, level_of_slot, level, do_static);
}

int rfsor_update_map(void *f, const double *z, int n_z) {
  FilterBase *F = F_(f);
  if (n_z < 0) return RFSGPU_ERR_INVALID;
  F->Z.assign(z, z + (size_t)F->dz * n_z);
  F->nZ = n_z;
  if (n_z > 0) F->resample_occured = false; /* :526 (an update with measurements; the resampling decision follows it) */
  F->update_map();
  return RFSGPU_OK;
}
int rfsor_importance_weighting(void *f) { F_(f)->importance_weighting(); return RFSGPU_OK; }
int rfsor_merge(void *f) { F_(f)->merge(); return RFSGPU_OK; }
int rfsor_prune(void *f) { F_(f)->prune(); return RFSGPU_OK; }
/* RBPHDFilter::update body (:444-523). */
/* probe: CostMatrix::reduce + getCostMatrixReduced on an n x n row-major table (modified in place like the reference's);
 * a_fixed[n], iRed[n], jRed[n] filled, returns the reduced dimension */
int rfsor_cost_matrix_reduce(double *C, int n, double lim, int *a_fixed, int *iRed, int *jRed) {
  std::vector<std::vector<double>> T(n, std::vector<double>(n));
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) T[i][j] = C[(size_t)i * n + j];
  orc::ReducedCost R = orc::cost_matrix_reduce(T, n, lim);
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) C[(size_t)i * n + j] = T[i][j];
  for (int i = 0; i < n; i++) { a_fixed[i] = R.a_fixed[i]; iRed[i] = i < (int)R.iRed.size() ? R.iRed[i] : -1; jRed[i] = i < (int)R.jRed.size() ? R.jRed[i] : -1; }
  return R.nRed;
}
/* the probe above; reset != 0 clears it after the read */
long rfsor_hungarian_max_queue_tail(int reset) {
  long v = __atomic_load_n(&orc::g_hungarian_max_queue_tail, __ATOMIC_RELAXED);
  if (reset) __atomic_store_n(&orc::g_hungarian_max_queue_tail, 0L, __ATOMIC_RELAXED);
  return v;
}
long rfsor_fs_solver_max_dim(void *f) { return F_(f)->fs_solver_max_dim; }
/* per particle of the last FastSLAM update: nMZ, nRed (0 when Murty was skipped) and the number of hypotheses kept; returns
 * the number of particles that update visited (-1: max_n is too small) */
int rfsor_fs_last_assoc_dims(void *f, int *nMZ, int *nRed, int *nH, int max_n) {
  FilterBase *F = F_(f);
  const int k = (int)F->fs_last_nMZ.size();
  if (max_n < k) return -1;
  for (int i = 0; i < k; i++) { nMZ[i] = F->fs_last_nMZ[i]; nRed[i] = F->fs_last_nRed[i]; nH[i] = F->fs_last_nH[i]; }
  return k;
}
void rfsor_default_fastslam_config(rfsgpu_fastslam_config *c) { orc::fastslam_defaults(c, 0); }
int rfsor_set_fastslam_config(void *f, const rfsgpu_fastslam_config *c) { F_(f)->fs = *c; return RFSGPU_OK; }
int rfsor_get_fastslam_config(const void *f, rfsgpu_fastslam_config *c) { *c = reinterpret_cast<const FilterBase *>(f)->fs; return RFSGPU_OK; }
int rfsor_fastslam_update(void *f, const double *z, int n_z) {
  FilterBase *F = F_(f);
  if (n_z < 0) return RFSGPU_ERR_INVALID;
  F->fastslam_handle = true;
  if (n_z == 0) return RFSGPU_OK; /* include/FastSLAM.hpp:401-402 */
  F->Z.assign(z, z + (size_t)F->dz * n_z);
  F->nZ = n_z;
  return F->fastslam_update();
}

int rfsor_update(void *f, const double *z, int n_z) {
  FilterBase *F = F_(f);
  if (n_z == 0) return RFSGPU_OK; /* :450-452 */
  rfsor_update_map(f, z, n_z);
  if (!F->cfg.useClusterProcess) F->importance_weighting();
  F->merge();
  F->prune();
  return RFSGPU_OK;
}

int rfsor_get_unused(void *f, int slot, int *idx, int max_n, int *n_out) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  int k = 0;
  for (unsigned u : F->unused[slot]) { if (k < max_n) idx[k] = (int)u; k++; }
  if (n_out) *n_out = k;
  return RFSGPU_OK;
}
int rfsor_landmarks_in_fov(void *f, int slot, int *n_out) {
  FilterBase *F = F_(f);
  if (slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  *n_out = (int)F->nInFov[slot];
  return RFSGPU_OK;
}

/* ParticleFilter::normalizeWeights (include/ParticleFilter.hpp:352-363) split in its two loops. */
int rfsor_weight_sums(void *f, double *out) {
  FilterBase *F = F_(f);
  double s = 0, s2 = 0;
  for (int i = 0; i < F->n; i++) { s += F->weight[i]; s2 += F->weight[i] * F->weight[i]; }
  out[0] = s; out[1] = s2;
  return RFSGPU_OK;
}
int rfsor_normalize_weights(void *f, double sum, const void *sum_dev) {
  (void)sum_dev;
  FilterBase *F = F_(f);
  for (int i = 0; i < F->n; i++) F->weight[i] = F->weight[i] / sum;
  return RFSGPU_OK;
}
int rfsor_normalize_weights_parts(void *f, double sum, const void *sum_dev, int n_parts) {
  (void)n_parts;
  return rfsor_normalize_weights(f, sum, sum_dev); /* the CPU side always gets the total on the host */
}
int rfsor_resample_apply_n(void *f, const int *src, int n_out) {
  FilterBase *F = F_(f);
  if (n_out < 1 || n_out > F->n) return RFSGPU_ERR_INVALID;
  for (int k = 0; k < n_out; k++) if (src[k] < 0 || src[k] >= F->n || (src[k] < n_out && src[src[k]] != src[k])) return RFSGPU_ERR_INVALID;
  F->ensure_ids();
  for (int k = 0; k < n_out; k++) {
    if (src[k] != k) {
      if (F->eager()) F->copy_particle(k, src[k]);
      else F->copy_map(k, src[k]);        /* Particle::copy: pose + mixture; the per-slot arrays of RBPHDFilter stay */
      F->pose[k] = F->pose[src[k]];       /* Particle::copy carries the pose (Particle.hpp:218-223) */
      F->pid[k] = F->pid[src[k]];         /* ... and the id (copy constructor); setParentId(source's id), ParticleFilter.hpp:473-474 */
      F->ppid[k] = F->pid[src[k]];
    } else {
      F->ppid[k] = F->pid[k];             /* case 1, ParticleFilter.hpp:466-467 */
    }
    F->weight[k] = 1;
  }
  F->resample_occured = true;
  F->shrink(n_out); /* particleSet_.resize(n) (ParticleFilter.hpp:481-483); the candidate lists beyond n stay where they are */
  return RFSGPU_OK;
}
int rfsor_resample_apply(void *f, const int *src) { return rfsor_resample_apply_n(f, src, F_(f)->n); }

/* Cross-shard migration rows (the CPU stand-in of rfsgpu_{slab_row_bytes, export_slab_rows, import_slab_rows}): the same
 * content -- pose (+ covariance), mixture, unused list, FOV count, birth candidates (Particle::copy,
 * include/Particle.hpp:218-223; RBPHDFilter.hpp:1005-1011) -- in a fixed-size record in HOST memory, so that the multi-GPU
 * host logic (rfs-slam_amd/sharded.py) runs unchanged over gloo with this library on every rank. */
enum { ROW_MAXG = 1024, ROW_HDR = 96 };
static size_t row_doubles(const FilterBase *F) {
  return ROW_HDR + (size_t)ROW_MAXG * (2 + F->dm + F->dm * F->dm) + (size_t)RFSGPU_MAX_CANDIDATES * (F->dm + F->dm * F->dm + 2);
}
size_t rfsor_slab_row_bytes(const void *f) { return row_doubles((const FilterBase *)f) * sizeof(double); }
int rfsor_export_slab_rows(void *f, const int *slots, int n, void *rows) {
  FilterBase *F = F_(f);
  const int D = F->dm;
  for (int k = 0; k < n; k++) {
    const int s = slots[k];
    if (s < 0 || s >= F->n) return RFSGPU_ERR_INVALID;
    double *r = (double *)rows + (size_t)k * row_doubles(F);
    const int cnt = F->gm_size(s);
    if (cnt > ROW_MAXG || (int)F->unused[s].size() > 64) return RFSGPU_ERR_CAPACITY;
    r[0] = cnt; r[1] = F->nInFov[s]; r[2] = (double)F->unused[s].size();
    for (size_t u = 0; u < F->unused[s].size(); u++) r[3 + u] = F->unused[s][u];
    memcpy(r + 67, F->pose[s].x, 3 * sizeof(double));
    memcpy(r + 70, F->pose[s].P, 9 * sizeof(double));
    double *g = r + ROW_HDR, *gw = g, *gwp = g + ROW_MAXG, *gm = gwp + ROW_MAXG, *gc = gm + (size_t)ROW_MAXG * D;
    F->export_gm(s, ROW_MAXG, gw, gwp, gm, gc);
    double *c = gc + (size_t)ROW_MAXG * D * D, *cmean = c, *ccov = cmean + RFSGPU_MAX_CANDIDATES * D;
    std::vector<int> sup(RFSGPU_MAX_CANDIDATES), chk(RFSGPU_MAX_CANDIDATES);
    const int nc = F->export_candidates(s, RFSGPU_MAX_CANDIDATES, cmean, ccov, sup.data(), chk.data());
    if (nc > RFSGPU_MAX_CANDIDATES) return RFSGPU_ERR_CAPACITY;
    r[79] = nc;
    double *ci = ccov + (size_t)RFSGPU_MAX_CANDIDATES * D * D;
    for (int q = 0; q < nc; q++) { ci[2 * q] = sup[q]; ci[2 * q + 1] = chk[q]; }
  }
  return RFSGPU_OK;
}
int rfsor_import_slab_rows(void *f, const int *slots, int n, const void *rows) {
  FilterBase *F = F_(f);
  const int D = F->dm;
  for (int k = 0; k < n; k++) {
    const int s = slots[k];
    if (s < 0 || s >= F->n) return RFSGPU_ERR_INVALID;
    const double *r = (const double *)rows + (size_t)k * row_doubles(F);
    const int cnt = (int)r[0];
    const bool eager = F->eager(); /* otherwise only what Particle::copy carries is taken */
    if (eager) {
      F->nInFov[s] = (unsigned)r[1];
      F->unused[s].clear();
      for (int u = 0; u < (int)r[2]; u++) F->unused[s].push_back((unsigned)r[3 + u]);
    }
    memcpy(F->pose[s].x, r + 67, 3 * sizeof(double));
    memcpy(F->pose[s].P, r + 70, 9 * sizeof(double));
    const double *g = r + ROW_HDR, *gw = g, *gm = g + 2 * (size_t)ROW_MAXG, *gc = gm + (size_t)ROW_MAXG * D;
    F->import_gm(s, cnt, gw, gm, gc);
    const double *c = gc + (size_t)ROW_MAXG * D * D, *cmean = c, *ccov = cmean + RFSGPU_MAX_CANDIDATES * D;
    const double *ci = ccov + (size_t)RFSGPU_MAX_CANDIDATES * D * D;
    const int nc = (int)r[79];
    std::vector<int> sup(nc), chk(nc);
    for (int q = 0; q < nc; q++) { sup[q] = (int)ci[2 * q]; chk[q] = (int)ci[2 * q + 1]; }
    if (eager) F->import_candidates(s, nc, cmean, ccov, sup.data(), chk.data());
  }
  return RFSGPU_OK;
}
int rfsor_set_birth_inheritance(void *f, int mode) {
  if (mode != RFSGPU_INHERIT_REFERENCE && mode != RFSGPU_INHERIT_EAGER && mode != RFSGPU_INHERIT_EXTERNAL) return RFSGPU_ERR_INVALID;
  F_(f)->inherit_mode = mode;
  return RFSGPU_OK;
}
int rfsor_get_birth_inheritance(const void *f) { return reinterpret_cast<const FilterBase *>(f)->inherit_mode; }
int rfsor_get_particle_ids(void *f, int *id, int *parent_id) {
  FilterBase *F = F_(f);
  F->ensure_ids();
  for (int k = 0; k < F->n; k++) { if (id) id[k] = (int)F->pid[k]; if (parent_id) parent_id[k] = (int)F->ppid[k]; }
  return RFSGPU_OK;
}
int rfsor_set_particle_ids(void *f, const int *id, const int *parent_id) {
  FilterBase *F = F_(f);
  F->ensure_ids();
  for (int k = 0; k < F->n; k++) { if (id) F->pid[k] = (unsigned)id[k]; if (parent_id) F->ppid[k] = (unsigned)parent_id[k]; }
  return RFSGPU_OK;
}
int rfsor_resample_occured(const void *f) { return reinterpret_cast<const FilterBase *>(f)->resample_occured ? 1 : 0; }
int rfsor_get_unused_masks(void *f, unsigned long long *masks) {
  FilterBase *F = F_(f);
  for (int k = 0; k < F->n; k++) { unsigned long long m = 0; for (unsigned u : F->unused[k]) m |= 1ull << u; masks[k] = m; }
  return RFSGPU_OK;
}
int rfsor_set_unused_masks(void *f, const unsigned long long *masks) {
  FilterBase *F = F_(f);
  for (int k = 0; k < F->n; k++) { F->unused[k].clear(); for (unsigned u = 0; u < 64; u++) if (masks[k] >> u & 1ull) F->unused[k].push_back(u); }
  return RFSGPU_OK;
}
void *rfsor_weights_device_ptr(void *f) { return (void *)F_(f)->weight.data(); }
int rfsor_fastslam_set_resample_occured(void *f, int flag) { F_(f)->fs_resample_occured = flag != 0; return RFSGPU_OK; }
int rfsor_particle_parents(void *f, int *parent, int max_n) {
  FilterBase *F = F_(f);
  if (max_n < F->n) return RFSGPU_ERR_INVALID;
  for (int k = 0; k < F->n; k++) parent[k] = (k < (int)F->parents.size()) ? F->parents[k] : k;
  return RFSGPU_OK;
}

/* ParticleFilter::resample (include/ParticleFilter.hpp:399-492) decision + systematic sampling +
 * slot assignment, given the uniform draw u01 (= the reference's single drand48()).
 * weights: in = unnormalised, out = normalised.  Returns 1 if resampling fires (src_slot filled),
 * 0 if not (weights only normalised). */
int rfsor_resample_decide(double *weights, int n, double effNParticles_t, double u01, int *src_slot) {
  double sum = 0;
  for (int i = 0; i < n; i++) sum += weights[i];
  for (int i = 0; i < n; i++) weights[i] = weights[i] / sum;
  double s2 = 0;
  for (int i = 0; i < n; i++) s2 += weights[i] * weights[i];
  double nEff = 1.0 / s2;
  double t_percent = effNParticles_t / n;
  if (nEff > effNParticles_t && nEff / n > t_percent) return 0;
  unsigned idx = 0;
  const double sample_interval = 1.0 / double(n);
  double sample_point = sample_interval * u01;
  double cumulative_weight = weights[0];
  std::vector<char> sampled(n, 0);
  std::vector<unsigned> sampled_idx(n, 0);
  for (int i = 0; i < n; i++) {
    while (sample_point > cumulative_weight) {
      idx++;
      if ((int)idx >= n) { idx = n - 1; break; } /* guard: reference reads past the end on round-off */
      cumulative_weight += weights[idx];
    }
    sampled_idx[i] = idx;
    sampled[idx] = 1;
    sample_point += sample_interval;
  }
  for (int i = 0; i < n; i++) src_slot[i] = i;
  unsigned idx_prev = 0, next_unsampled = 0;
  for (int i = 0; i < n; i++) {
    bool firstTime = true;
    idx = sampled_idx[i];
    if (i > 0 && idx == idx_prev) firstTime = false;
    idx_prev = idx;
    if (firstTime) continue; /* case 1 (idx < n always here since n == nParticles_) */
    while (next_unsampled < (unsigned)n && sampled[next_unsampled] == 1) next_unsampled++;
    src_slot[next_unsampled] = (int)idx;
    next_unsampled++;
  }
  return 1;
}

int rfsor_get_timing(void *f, rfsgpu_timing *t) { *t = F_(f)->timing; return RFSGPU_OK; }
int rfsor_reset_timing(void *f) { memset(&F_(f)->timing, 0, sizeof(rfsgpu_timing)); return RFSGPU_OK; }
int rfsor_synchronize(void *f) { (void)f; return RFSGPU_OK; }

int rfsor_mat_perm(const double *A, int n, int batch, double *out, int device_id) {
  (void)device_id;
  if (n < 1 || n > 24) return RFSGPU_ERR_INVALID;
  for (int b = 0; b < batch; b++) out[b] = orc::mat_perm(A + (size_t)b * n * n, n);
  return RFSGPU_OK;
}

/* ---- oracle-only controls and probes (not part of the product ABI) ---------------------------- */
void rfsor_set_stable_sort(void *f, int on) { F_(f)->stable_sort = on != 0; }
void rfsor_set_threads(int n) {
#ifdef _OPENMP
  omp_set_num_threads(n);
#else
  (void)n;
#endif
}
int rfsor_max_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}
long rfsor_murty_calls(void *f) { return F_(f)->murty_calls; }
long rfsor_lonerow_bug_hits(void *f) { return F_(f)->lonerow_bug_hits; }
long rfsor_hungarian_failures(void) { return orc::g_hungarian_fail; }

/* Victoria Park model probes for unit tests: Pd (with near-limit flag) and measure(). */
double rfsor_vp_pd(void *f, const double *pose3, const double *lx3, const double *lS9, int *close_out) {
  auto *F = FVP_(f);
  orc::Pose p;
  memcpy(p.x, pose3, sizeof(p.x));
  memset(p.P, 0, sizeof(p.P));
  orc::M3 S;
  memcpy(S.a, lS9, sizeof(S.a));
  bool close;
  double v = F->model.pd(p, lx3, S, close);
  if (close_out) *close_out = close ? 1 : 0;
  return v;
}
void rfsor_vp_measure(void *f, const double *pose3, const double *lx3, const double *lS9, double *z3, double *S9, double *H9) {
  auto *F = FVP_(f);
  orc::Pose p;
  memcpy(p.x, pose3, sizeof(p.x));
  memset(p.P, 0, sizeof(p.P));
  orc::M3 lS, S, H;
  memcpy(lS.a, lS9, sizeof(lS.a));
  F->model.measure(p, lx3, lS, z3, S, &H);
  memcpy(S9, S.a, sizeof(S.a));
  memcpy(H9, H.a, sizeof(H.a));
}
double rfsor_vp_clutter(void *f) { return FVP_(f)->model.clutter(); }
/* mirror of rfsgpu_vp_probe_pd: Pd / near-limit flag of the first max_n Gaussians of particle `slot` */
int rfsor_vp_probe_pd(void *f, int slot, double *pd, int *close_to_limit, int max_n) {
  auto *F = FVP_(f);
  if (!F || slot < 0 || slot >= F->n) return RFSGPU_ERR_INVALID;
  const int n = std::min(max_n, F->gm_size(slot));
  std::vector<double> w(n), wp(n), mean(3 * (size_t)n), cov(9 * (size_t)n);
  F->export_gm(slot, n, w.data(), wp.data(), mean.data(), cov.data());
  for (int m = 0; m < n; m++) {
    orc::M3 S;
    memcpy(S.a, &cov[9 * (size_t)m], sizeof(S.a));
    bool close;
    pd[m] = F->model.pd(F->pose[slot], &mean[3 * (size_t)m], S, close);
    close_to_limit[m] = close ? 1 : 0;
  }
  return RFSGPU_OK;
}

/* PermutationLexicographic restatement, flattened: writes up to max_perm permutations of length nM+nZ. */
int rfsor_permlex_all(unsigned nM, unsigned nZ, unsigned *out, int max_perm) {
  orc::PermLex pl(nM, nZ, true);
  std::vector<unsigned> o(nM + nZ);
  int k = 0;
  while (pl.next(o.data()) != 0) {
    if (k < max_perm) memcpy(out + (size_t)k * (nM + nZ), o.data(), (nM + nZ) * sizeof(unsigned));
    k++;
  }
  return k;
}
/* Hungarian restatement: C row-major n x n (restored in place like the reference). */
int rfsor_hungarian(double *C, int n, int *soln, double *cost) {
  std::vector<double *> rows(n);
  for (int i = 0; i < n; i++) rows[i] = C + (size_t)i * n;
  return orc::hungarian_run(rows.data(), n, soln, cost) ? 1 : 0;
}
/* Murty restatement: up to k best; real-assignment block (nR,nC) (pass n,n for plain k-best).
 * Returns the number found; scores[k], assignments[k*n]. */
int rfsor_murty(double *C, int n, int nR, int nC, int kmax, double *scores, int *assignments) {
  std::vector<double *> rows(n);
  for (int i = 0; i < n; i++) rows[i] = C + (size_t)i * n;
  orc::Murty m(rows.data(), n);
  m.setRealAssignmentBlock(nR, nC);
  std::vector<int> a;
  double s;
  int k = 0;
  for (; k < kmax; k++) {
    int rank = m.findNextBest(a, s);
    if (rank == -1) break;
    scores[k] = s;
    if (assignments) memcpy(assignments + (size_t)k * n, a.data(), n * sizeof(int));
  }
  return k;
}
/* rfsMeasurementLikelihood on an explicit likelihood table (nE x nZ, already gated, incl. Pd):
 * the partition / enumeration / Murty part only (RBPHDFilter.hpp:865-996) -- for unit tests. */
double rfsor_partition_likelihood(const double *L, int nE, int nZ, const double *evalPd, double clutter, double clutterIntegral,
                                  long *murty_calls, long *lonerow_hits) {
  orc::CostMatrixGeneral cm(nE, nZ);
  for (int m = 0; m < nE; m++)
    for (int n = 0; n < nZ; n++) cm.C_[m][n] = L[m * nZ + n];
  std::vector<double> pd(evalPd, evalPd + nE), cl(nZ, clutter);
  return orc::partitions_likelihood(cm, pd, cl, murty_calls, lonerow_hits) / clutterIntegral;
}
/* The same in either partition mode: exact != 0 is the checker of the engine's opt-in RFSGPU_PARTITION_EXACT (exact_partition_sum). */
double rfsor_partition_likelihood_mode(const double *L, int nE, int nZ, const double *evalPd, double clutter, double clutterIntegral,
                                       long *murty_calls, long *lonerow_hits, int exact) {
  orc::CostMatrixGeneral cm(nE, nZ);
  for (int m = 0; m < nE; m++)
    for (int n = 0; n < nZ; n++) cm.C_[m][n] = L[m * nZ + n];
  std::vector<double> pd(evalPd, evalPd + nE), cl(nZ, clutter);
  return orc::partitions_likelihood(cm, pd, cl, murty_calls, lonerow_hits, exact != 0) / clutterIntegral;
}

} /* extern "C" */
