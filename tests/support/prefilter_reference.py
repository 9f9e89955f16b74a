"""Independent references for the fp32 prefilters in front of the exact merge and gate tests, and inputs placed at their margins.

The merge and map-update kernels screen pairs in fp32 (csrc/merge_prune.h, csrc/vp.h, csrc/update_map.h) before the exact fp64 test
of the reference decides.  The screens claim to let extra pairs through but never to drop one.  This module gives

- the reference's rules, written from the equations: GaussianMixture::merge (include/GaussianMixture.hpp:394-475) for 2-D and 3-D
  Gaussians, RBPHDFilter::updateMap for the range-bearing model, and the innovation gates of KalmanFilter_RngBrg::calculateInnovation
  (src/KalmanFilter_RngBrg.cpp:52-65: range gate, while-loop wrap, bearing gate) and of the Victoria Park filter (wrap first);
- a replay of the greedy merge in exact rational arithmetic (fractions.Fraction) that certifies every decision: each pair test the
  reference makes must sit at least CERT_REL (relative) on its side of t^2, so that no fp64 rounding, on the device or in the oracle,
  can flip it, while it may still sit well inside the fp32 prefilters' 1e-6 .. 1e-5 margins;
- case constructors that put pairs at those margins: far from the origin, near-rank-1 covariances lined up with the pair's offset
  (the shape where the trace bound of the prefilter radius is tight), rows at the listing limits, grid spans at the fine-grid switch,
  and (landmark, measurement) pairs at the innovation gates.  Every constructor returns the certified decisions with its inputs.
"""
import math
from fractions import Fraction

import numpy as np

CERT_REL = 1e-9          # a certified decision's deciding quantity is at least this far (relative) from its threshold
PI = Fraction(math.pi)   # the reference's PI is the double M_PI


# ---- range-bearing model and updateMap (moved from test_oracle_numpy.py) ------------------------------------------------------

def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def np_measure(P, pose, pose_cov, mu, Sig):
    d = mu - pose[:2]
    r2 = d @ d
    r = np.sqrt(r2)
    zexp = np.array([r, wrap(np.arctan2(d[1], d[0]) - pose[2])])
    H = np.array([[d[0] / r, d[1] / r], [-d[1] / r2, d[0] / r2]])
    Hr = np.array([[-d[0] / r, -d[1] / r, 0], [d[1] / r2, -d[0] / r2, -1]])
    S = H @ Sig @ H.T + Hr @ pose_cov @ Hr.T + np.asarray(P["R"])
    return zexp, H, S, (P["rmin"] <= r <= P["rmax"]), r


def np_pd(P, r):
    if P["rmin"] <= r <= P["rmax"]:
        return P["Pd"], (r >= P["rmax"] - P["rbuf"] or r <= P["rmin"] + P["rbuf"])
    return 0.0, (P["rmin"] - P["rbuf"] <= r <= P["rmax"] + P["rbuf"])


def np_update_map(P, pose, pose_cov, w, mu, Sig, Z):
    nM, nZ = len(w), len(Z)
    W = np.zeros((nM, nZ))
    new = {}
    Pd = np.zeros(nM)
    close = np.zeros(nM, bool)
    for m in range(nM):
        zexp, H, S, ok, r = np_measure(P, pose, pose_cov, mu[m], Sig[m])
        Pd[m], close[m] = np_pd(P, r)
        if close[m]:
            Pd[m] = 1.0
        if Pd[m] == 0 or not ok:
            continue
        Si = np.linalg.inv(S)
        K = Sig[m] @ H.T @ Si
        Pn = (np.eye(2) - K @ H) @ Sig[m]
        Pn = (Pn + Pn.T) / 2
        for z in range(nZ):
            e = Z[z] - zexp
            if P["kf_range"] > 0 and abs(e[0]) > P["kf_range"]:
                continue
            nu = np.array([e[0], wrap(e[1])])
            if P["kf_bearing"] > 0 and abs(nu[1]) > P["kf_bearing"]:
                continue
            md2 = e @ Si @ e                                  # raw difference on purpose
            if md2 > P["new_gaussian_md"] ** 2:
                continue
            lik = np.exp(-0.5 * md2) / np.sqrt((2 * np.pi) ** 2 * np.linalg.det(S))
            if lik == 0:
                continue
            W[m, z] = Pd[m] * w[m] * lik
            new[(m, z)] = (mu[m] + K @ nu, Pn)
    colsum = P["clutter"] + W.sum(0)
    Wn = W / colsum
    out_w, out_mu, out_S = [], [], []
    for (m, z), (x, Pn) in sorted(new.items()):
        if Wn[m, z] > 0:
            out_w.append(Wn[m, z]); out_mu.append(x); out_S.append(Pn)
    wk = (1 - Pd) * w
    for m in range(nM):
        if close[m] and w[m] > P["birth_w"]:
            dw = Pd[m] * w[m] - Wn[m].sum()
            if dw > 0:
                wk[m] = min(wk[m] + dw, 1.0)
    unused = [z for z in range(nZ) if not np.any(Wn[:, z] != 0)]
    return (np.concatenate([wk, out_w]), np.concatenate([w, np.zeros(len(out_w))]),
            np.array(list(mu) + out_mu), np.array(list(Sig) + out_S), unused, int((Pd != 0).sum()), colsum)


# ---- GaussianMixture::merge (moved from test_oracle_numpy.py) ------------------------------------------------------------------

def np_merge(w, mu, Sg, t, f):
    w, mu, Sg = w.copy(), mu.copy(), Sg.copy()
    alive = np.ones(len(w), bool)
    for a in range(len(w)):
        if not alive[a]:
            continue
        for b in range(a + 1, len(w)):
            if not alive[b]:
                continue
            e = mu[b] - mu[a]
            if e @ np.linalg.solve(Sg[a], e) > t * t and e @ np.linalg.solve(Sg[b], e) > t * t:
                continue
            wm = w[a] + w[b]
            if wm == 0:
                continue
            xm = (mu[a] * w[a] + mu[b] * w[b]) / wm
            d1, d2 = xm - mu[a], xm - mu[b]
            Sg[a] = (w[a] * (Sg[a] + f * np.outer(d1, d1)) + w[b] * (Sg[b] + f * np.outer(d2, d2))) / wm
            mu[a], w[a], alive[b] = xm, wm, False
    return w[alive], mu[alive], Sg[alive]


def np_merge_vp(w, mu, Sg, t, f):
    """GaussianMixture::merge for the Victoria Park landmarks (x, y, diameter; include/GaussianMixture.hpp:394-475 with
    Landmark3d): i ascending, j ascending > i, j absorbed into i as soon as md2_i(j) <= t^2 or md2_j(i) <= t^2 and w_i + w_j != 0;
    x_m = (w_i x_i + w_j x_j) / w_m, S_m = (w_i (S_i + f d_i d_i^T) + w_j (S_j + f d_j d_j^T)) / w_m, i's state changes before j + 1
    is tested.  The rule has no dimension in it: this is np_merge on 3-vectors."""
    assert mu.shape[1:] == (3,) and Sg.shape[1:] == (3, 3)
    return np_merge(w, mu, Sg, t, f)


def merged_then_pruned(w, mu, Sg, t, f, prune_thr):
    """What the fused update leaves of a map nobody measures (Pd = 0 everywhere): sortByWeight (include/RBPHDFilter.hpp:733),
    merge, prune (GaussianMixture::prune: keep w >= threshold) and sort by weight again.  With tied weights the order of equal keys
    is the stable sort's here and std::sort's in the reference: compare such mixtures as multisets."""
    o = np.argsort(-w, kind="stable")
    mw, mmu, mS = np_merge(w[o], mu[o], Sg[o], t, f)
    keep = mw >= prune_thr
    mw, mmu, mS = mw[keep], mmu[keep], mS[keep]
    o = np.argsort(-mw, kind="stable")
    return mw[o], mmu[o], mS[o]


# ---- exact replay of the greedy merge ------------------------------------------------------------------------------------

def _md2_exact(e, S):
    """e^T S^-1 e in rationals (Cramer's rule); None when S is singular."""
    n = len(e)
    if n == 2:
        det = S[0][0] * S[1][1] - S[0][1] * S[1][0]
        if det == 0:
            return None
        return (e[0] * e[0] * S[1][1] - e[0] * e[1] * (S[0][1] + S[1][0]) + e[1] * e[1] * S[0][0]) / det
    a, b, c = S[0]
    d, g, h = S[1]
    k, l, m = S[2]
    det = a * (g * m - h * l) - b * (d * m - h * k) + c * (d * l - g * k)
    if det == 0:
        return None
    adj = [[g * m - h * l, c * l - b * m, b * h - c * g],
           [h * k - d * m, a * m - c * k, c * d - a * h],
           [d * l - g * k, b * k - a * l, a * g - b * d]]
    return sum(e[r] * sum(adj[r][q] * e[q] for q in range(3)) for r in range(3)) / det


def _to_frac(x):
    return [Fraction(float(v)) for v in np.asarray(x).ravel()]


def certified_merge(w, mu, Sg, t, f, rel=CERT_REL):
    """Replays GaussianMixture::merge in exact arithmetic on the given doubles.  Returns (alive, merges, margin): the surviving entries,
    the (row, absorbed) pairs in the order the reference makes them, and the smallest |md2 / t^2 - 1| over every test that decided
    something.  Raises ValueError when a decision sits closer than `rel` to t^2.

    A test is decided by d1 = md2_a(j) alone when d1 <= t^2, else by both d1 and d2 = md2_j(a).  Pairs whose fp64 Mahalanobis
    distances both exceed 4 t^2 are settled without rationals: fp64 is far more accurate than a factor of 4 (the covariances used here
    have condition numbers up to 1e8)."""
    n, dim = mu.shape
    t2 = Fraction(t) * Fraction(t)
    F = Fraction(f)
    W = [Fraction(float(v)) for v in w]
    X = [_to_frac(mu[k]) for k in range(n)]
    S = [[_to_frac(Sg[k])[r * dim:(r + 1) * dim] for r in range(dim)] for k in range(n)]
    Xf = np.array(mu, dtype=np.float64)
    Sf = np.array(Sg, dtype=np.float64)
    alive = np.ones(n, bool)
    merges = []
    margin = math.inf

    def exact_md2(a, j):
        e = [X[j][r] - X[a][r] for r in range(dim)]
        return _md2_exact(e, S[a]), _md2_exact([-v for v in e], S[j])

    def check(md2):
        nonlocal margin
        if md2 is None:
            raise ValueError("singular covariance in a certified case")
        m = abs(float(md2 / t2) - 1.0)
        if m < rel:
            raise ValueError(f"merge decision within {m:.3g} of the threshold")
        margin = min(margin, m)

    with np.errstate(all="ignore"):
        Sinv = np.linalg.inv(Sf)
    lim = 4 * t * t

    def screen(a, lo):
        """Entries j >= lo, alive, that fp64 cannot settle as far (both md2 > 4 t^2), ascending."""
        js = np.arange(lo, n)
        js = js[alive[lo:]]
        if js.size == 0:
            return js
        e = Xf[js] - Xf[a]
        with np.errstate(all="ignore"):
            q1 = np.einsum("ki,ij,kj->k", e, Sinv[a], e)
            q2 = np.einsum("ki,kij,kj->k", e, Sinv[js], e)
        far = (q1 > lim) & (q2 > lim) & np.isfinite(q1) & np.isfinite(q2)
        return js[~far]

    for a in range(n):
        if not alive[a]:
            continue
        cand = list(screen(a, a + 1))
        while cand:
            j = int(cand.pop(0))
            if not alive[j]:
                continue
            d1, d2 = exact_md2(a, j)
            check(d1)
            passes = d1 <= t2
            if not passes:
                check(d2)
                passes = d2 <= t2
            if not passes:
                continue
            wm = W[a] + W[j]
            if wm == 0:
                continue
            xm = [(X[a][r] * W[a] + X[j][r] * W[j]) / wm for r in range(dim)]
            da = [xm[r] - X[a][r] for r in range(dim)]
            dj = [xm[r] - X[j][r] for r in range(dim)]
            S[a] = [[(W[a] * (S[a][r][c] + F * da[r] * da[c]) + W[j] * (S[j][r][c] + F * dj[r] * dj[c])) / wm for c in range(dim)]
                    for r in range(dim)]
            X[a], W[a] = xm, wm
            Xf[a] = [float(v) for v in xm]
            Sf[a] = [[float(v) for v in row] for row in S[a]]
            with np.errstate(all="ignore"):
                Sinv[a] = np.linalg.inv(Sf[a])
            alive[j] = False
            merges.append((a, j))
            cand = list(screen(a, j + 1))        # the row's new state: everything above j again
    return alive, merges, margin


# ---- merge cases ---------------------------------------------------------------------------------------------------------

MERGE_T, MERGE_F, PRUNE_T = 0.5, 1.5, 0.01     # scenarios.C1_PARAMS
RANK1 = 1e-8                                   # smallest / largest eigenvalue of the lined-up covariances


def _rank1_cov(s, u, dim=2):
    """Covariance with variance s^2 along the unit vector u (first two coordinates) and RANK1 s^2 across."""
    C = np.zeros((dim, dim))
    C[:2, :2] = s * s * (np.outer(u, u) + RANK1 * (np.eye(2) - np.outer(u, u)))
    if dim == 3:
        C[2, 2] = RANK1 * s * s
    return C


def _finish_merge_case(w, mean, cov, t, f, jitter=True):
    """Sort every mixture by weight, descending (the order the fused update merges in: then the stand-alone merge and the update make
    the same decisions), certify it, and return the case dict.  jitter: perturb the weights by up to 1e-4 first, so that neither the
    weights nor the sums of merged weights tie (the update's final sort would then follow std::sort's order of equal keys)."""
    if jitter:
        w = w + np.random.default_rng(12345).uniform(0.0, 1e-4, w.shape)
    for i in range(len(w)):
        o = np.argsort(-w[i], kind="stable")
        w[i], mean[i], cov[i] = w[i][o], mean[i][o], cov[i][o]
    alive, merges, margins = [], [], []
    for i in range(len(w)):
        al, mg, mr = certified_merge(w[i], mean[i], cov[i], t, f)
        alive.append(al); merges.append(mg); margins.append(mr)
    exp_w = []
    for i in range(len(w)):
        ww = list(w[i])
        for a, j in merges[i]:
            ww[a] = ww[a] + ww[j]
        exp_w.append(np.array([ww[k] for k in range(len(ww)) if alive[i][k]]))
    return dict(w=w, mean=mean, cov=cov, t=t, f=f, alive=alive, merges=merges, margin=min(margins),
                sizes=np.array([int(a.sum()) for a in alive]), merged_w=exp_w)


def _f32_ulp(x):
    """Spacing of the fp32 numbers at |x|."""
    return float(np.spacing(np.float32(abs(x))))


def straddle_case(offset, axis="x", delta=1e-3, groups=8, n_per_group=None, n_pairs=40, seed=0, dim=2, t=MERGE_T, f=MERGE_F,
                  at_origin=False):
    """Lined-up near-rank-1 pairs at md2 = t^2 (1 - delta) (delta < 0: t^2 (1 + |delta|), no merge), far from the origin.

    The fp32 copy of a coordinate is off by up to half an fp32 ulp u.  Each pair's doubles are placed 0.499 u inside two fp32 numbers
    D u apart, so that the fp32 difference of the pair exceeds the exact one by ~u, the most rounding can add.  The covariance makes
    the exact difference md2 = t^2 (1 - delta); the prefilter radius is then ~D u.  D is as small as keeps the radius above span / 32
    (the box is at least 1e-3 |offset| wide), so that a cell edge of the merge grid is about one radius, and the fp32 difference is
    longer than that edge by a fraction of u.  The lower members of the pairs sweep D + 20 consecutive fp32 numbers along the axis
    (n_pairs per particle, stacked across the axis, the particles of a group sharing one anchor at the box's low corner): whatever
    the grid's formulas are, cell boundaries of width ~D u fall inside the sweep, and some pair straddles one.  `groups` anchors
    give different alignments of the boundaries against the fp32 numbers.  at_origin: the same pairs with the offset taken out."""
    rng = np.random.default_rng(seed)
    off = np.array(offset, dtype=np.float64)
    ax = {"x": 0, "y": 1}[axis]
    S = max(abs(off[ax]), 1e3)
    u = _f32_ulp(S)
    D = int(math.ceil(1.03 * (1e-3 * S / u + 20) / 30)) + 2
    L = D + 20
    if n_per_group is None:
        n_per_group = int(math.ceil(L / n_pairs))
    d = (D - 0.998) * u
    s = d / (t * math.sqrt(1.0 - delta))
    rad = t * s
    uvec = np.zeros(2); uvec[ax] = 1.0
    vvec = np.zeros(2); vvec[1 - ax] = 1.0
    C = _rank1_cov(s, uvec, dim)
    M = 1 + 2 * n_pairs
    n_particles = groups * n_per_group
    w = np.zeros((n_particles, M))
    mean = np.zeros((n_particles, M, dim))
    cov = np.zeros((n_particles, M, dim, dim))
    base0 = float(np.float32(off[ax])) if not at_origin else 0.0
    perp = off[1 - ax] if not at_origin else 0.0
    for g in range(groups):
        a0 = base0 + int(rng.integers(0, 4 * D)) * u if not at_origin else base0 + rng.uniform(0, 4 * rad)
        for p in range(n_per_group):
            i = g * n_per_group + p
            pts = np.zeros((M, 2))
            pts[0, ax] = a0 - 5 * u
            pts[0, 1 - ax] = perp - 3 * rad
            for k in range(n_pairs):
                step = p * n_pairs + k
                lo = a0 + (step % L) * u
                if at_origin:
                    pts[1 + 2 * k, ax] = lo - base0 + 0.499 * u
                    pts[2 + 2 * k, ax] = lo - base0 + 0.499 * u + d
                else:
                    pts[1 + 2 * k, ax] = lo + 0.499 * u
                    pts[2 + 2 * k, ax] = lo + D * u - 0.499 * u
                pts[1 + 2 * k, 1 - ax] = pts[2 + 2 * k, 1 - ax] = perp + 3.0 * rad * k
            if at_origin:
                pts[0, ax] -= base0
            o = rng.permutation(M)                     # entries in random order: rows and partners on either side
            mean[i, :, :2] = pts[o]
            if dim == 3:
                mean[i, :, 2] = 0.5
            cov[i] = C
            w[i] = rng.permutation(np.linspace(0.3, 0.9, M)) + rng.uniform(0, 1e-3, M)
    return _finish_merge_case(w, mean, cov, t, f)


def issue_regression_case(t=MERGE_T, f=MERGE_F):
    """Three Gaussians at y = 0, covariance diag(0.88, 0.88e-8): an anchor at x = 9997 and a pair at md2 = 0.9994 t^2 whose fp32
    coordinates are farther apart than the merge grid's cell edge without a rounding term (they fall two cells apart)."""
    w = np.array([[0.5, 0.5, 0.5]])
    mean = np.array([[[9997.0, 0.0], [10000.620556640624, 0.0], [10001.089457504133, 0.0]]])
    cov = np.tile(np.diag([0.88, 0.88e-8]), (1, 3, 1, 1))
    return _finish_merge_case(w, mean, cov, t, f, jitter=False)


def listing_limit_case(n_ring, ring, n_clusters=6, n_particles=8, seed=0, offset=(0.0, 0.0), t=MERGE_T, f=MERGE_F):
    """Rows with exactly n_ring prefilter survivors: a centre with covariance s_a^2 I and n_ring entries on a ring of radius
    ring * t * s_a around it, with covariances (0.05 s_a)^2 I (they neither merge nor list one another).  The centres carry the top
    weights, so after the weight sort every centre is a row with all n_ring ring entries above it.  ring < 1: every ring entry passes
    against the row's initial state; 1 < ring < sqrt(2): none passes, but all lie inside the prefilter radius t s_a sqrt(2)."""
    rng = np.random.default_rng(seed)
    sa = 0.2
    M = n_clusters * (1 + n_ring)
    w = np.zeros((n_particles, M)); mean = np.zeros((n_particles, M, 2)); cov = np.zeros((n_particles, M, 2, 2))
    for i in range(n_particles):
        pts, cs, ws = [], [], []
        for c in range(n_clusters):
            ctr = np.array(offset) + np.array([c * 12 * t * sa * 1.5, rng.uniform(0, 0.3)])
            pts.append(ctr); cs.append(sa * sa * np.eye(2)); ws.append(rng.uniform(0.8, 0.9))
            ph = rng.uniform(0, 2 * np.pi)
            for k in range(n_ring):
                a = ph + 2 * np.pi * k / n_ring
                pts.append(ctr + ring * t * sa * np.array([math.cos(a), math.sin(a)]) * rng.uniform(0.99, 1.0))
                cs.append((0.05 * sa) ** 2 * np.eye(2)); ws.append(rng.uniform(0.3, 0.7))
        mean[i] = pts; cov[i] = cs; w[i] = ws
    return _finish_merge_case(w, mean, cov, t, f)


def pair_cap_case(n_clusters, k=5, n_particles=6, seed=0, t=MERGE_T, f=MERGE_F):
    """n_clusters isolated clusters of k entries that all lie within one another's prefilter radius: every cluster lists k(k-1)/2
    pairs, so the mixture lists n_clusters k (k - 1) / 2 in all (32 clusters of 5: exactly 320, MERGE_PAIR_CAP of a 192-entry
    slab; 33: one more row than fits)."""
    rng = np.random.default_rng(seed)
    s = 0.1
    M = n_clusters * k
    w = np.zeros((n_particles, M)); mean = np.zeros((n_particles, M, 2)); cov = np.zeros((n_particles, M, 2, 2))
    side = int(math.ceil(math.sqrt(n_clusters)))
    for i in range(n_particles):
        pts = []
        for c in range(n_clusters):
            ctr = np.array([c % side, c // side], dtype=np.float64) * 8 * t * s * 1.5 + rng.uniform(0, 0.01, 2)
            pts.extend(ctr + rng.uniform(-0.15, 0.15, (k, 2)) * t * s)
        o = rng.permutation(M)
        mean[i] = np.array(pts)[o]
        cov[i] = s * s * np.eye(2)
        w[i] = rng.permutation(np.linspace(0.3, 0.9, M))
    return _finish_merge_case(w, mean, cov, t, f)


def slack_case(n_particles=8, seed=0, t=MERGE_T, f=MERGE_F):
    """Five clusters of three: A (small covariance, the heaviest, so the row), B (wide covariance, next) at md2_A = 0.81 t^2, and C
    (light, last) more than twice A's prefilter radius from A.  C is not listed for A; it only bounds A's slack.  A absorbs B, and its
    covariance grows far past the slack; C passes against that state, so the row must leave its list (the walk's slack test falls back
    to the sequential scan) to absorb C.  `roles[i]` lists (A, B, C) per cluster, as merge indices."""
    rng = np.random.default_rng(seed)
    M = 3 * 5
    w = np.zeros((n_particles, M)); mean = np.zeros((n_particles, M, 2)); cov = np.zeros((n_particles, M, 2, 2))
    sa, sb, sc_ = 0.1, 2.0, 0.05
    ra = t * sa * math.sqrt(2.0)
    for i in range(n_particles):
        pts, cs, ws = [], [], []
        for c in range(5):
            ctr = np.array([c * 40.0, rng.uniform(0, 1)])
            ang = rng.uniform(0, 2 * np.pi)
            u = np.array([math.cos(ang), math.sin(ang)])
            pts += [ctr, ctr + 0.9 * t * sa * u, ctr + (2.3 + 0.5 * rng.uniform()) * ra * u]
            cs += [sa * sa * np.eye(2), sb * sb * np.eye(2), sc_ * sc_ * np.eye(2)]
            ws += [0.9 - 0.01 * c, 0.6 - 0.01 * c, 0.3 + 0.01 * c]
        mean[i] = pts; cov[i] = cs; w[i] = np.array(ws) + 1e-4 * i
    case = _finish_merge_case(w, mean, cov, t, f)
    roles = []
    for i in range(n_particles):
        xx = case["cov"][i][:, 0, 0]
        idx = {v: np.nonzero(np.isclose(xx, v * v))[0] for v in (sa, sb, sc_)}
        near = lambda a, js: int(js[np.argmin(np.linalg.norm(case["mean"][i][js] - case["mean"][i][a], axis=1))])
        roles.append([(int(a), near(a, idx[sb]), near(a, idx[sc_])) for a in idx[sa]])
    case["roles"] = roles
    return case


def fine_grid_case(span_factor, n=150, n_particles=8, seed=0, t=MERGE_T, f=MERGE_F):
    """A mixture whose bounding box is span_factor * 1.5 * 64 prefilter radii on each side: just above (> 1) or below (< 1) the
    span at which the 64 x 64 merge grid falls back to 32 x 32 cells (MERGE_FINE_MIN = 1.5).  The box's corners are pinned; the
    rest is random, with a few near-threshold pairs."""
    rng = np.random.default_rng(seed)
    s = 0.1
    rad = t * s * math.sqrt(2.0) * (1 + 1e-6) * 1.0001
    E = span_factor * 1.5 * 64 * rad
    w = np.zeros((n_particles, n)); mean = np.zeros((n_particles, n, 2)); cov = np.zeros((n_particles, n, 2, 2))
    for i in range(n_particles):
        p = rng.uniform(0, E, (n, 2))
        p[0] = [0, 0]; p[1] = [E, E]
        for k in range(2, 40, 2):                    # near-threshold pairs: md2 = t^2 (1 -+ 1e-3)
            u = rng.normal(size=2); u /= np.linalg.norm(u)
            p[k + 1] = p[k] + t * s * math.sqrt(1 + (1e-3 if k % 4 else -1e-3)) * u
        p = np.clip(p, 0, E)
        mean[i] = p + np.array([-E / 2, 5.0])         # (x0 = xmin - 1e-3 |xmin|: the box is E (1 + 5e-4) wide)
        cov[i] = s * s * np.eye(2)
        w[i] = rng.permutation(np.linspace(0.3, 0.9, n))
    return _finish_merge_case(w, mean, cov, t, f)


# ---- innovation gates ----------------------------------------------------------------------------------------------------

def wrap_reference(a):
    """while (a > PI) a -= 2 PI; while (a < -PI) a += 2 PI; in exact arithmetic, PI the double M_PI."""
    a = Fraction(a)
    while a > PI:
        a -= 2 * PI
    while a < -PI:
        a += 2 * PI
    return a


def gate_rngbrg(e0, e1, g_range, g_bearing):
    """KalmanFilter_RngBrg::calculateInnovation for the raw innovation (e0, e1) (exact rationals): range gate, while-loop wrap, bearing
    gate.  Returns (passes, margin): margin is |q / g - 1| of every gate quantity the decision consulted (the smallest)."""
    e0, e1 = Fraction(e0), Fraction(e1)
    gr, gb = Fraction(g_range), Fraction(g_bearing)
    margin = math.inf
    if gr > 0:
        margin = abs(float(abs(e0) / gr) - 1.0)
        if abs(e0) > gr:
            return False, margin
    nu1 = wrap_reference(e1)
    if gb > 0:
        margin = min(margin, abs(float(abs(nu1) / gb) - 1.0))
        if abs(nu1) > gb:
            return False, margin
    return True, margin


def gate_vp(e0, e1, g_range, g_bearing):
    """KalmanFilter_VictoriaPark::calculateInnovation: wrap the bearing first, then the range gate, then the bearing gate.  Both gates
    are consulted whenever the range gate passes; the decision is the same as gate_rngbrg's."""
    e0, e1 = Fraction(e0), Fraction(e1)
    nu1 = wrap_reference(e1)
    gr, gb = Fraction(g_range), Fraction(g_bearing)
    margin = math.inf
    if gr > 0:
        margin = abs(float(abs(e0) / gr) - 1.0)
        if abs(e0) > gr:
            return False, margin
    if gb > 0:
        margin = min(margin, abs(float(abs(nu1) / gb) - 1.0))
        if abs(nu1) > gb:
            return False, margin
    return True, margin


GATE_SETS = ["range", "bearing", "wrap", "wrap_far", "past_50"]


def _gate_measurements(kind, zexp, g_r, g_b, deltas, rng):
    """Measurements for one expected measurement zexp = (range, bearing) at the gates."""
    out = []
    for dl in deltas:
        for sgn in (-1.0, 1.0):
            for side in (-1.0, 1.0):                 # inside (1 - delta) / outside (1 + delta)
                q = 1.0 + side * dl
                if kind == "range":
                    out.append((zexp[0] + sgn * g_r * q, zexp[1] + rng.uniform(-0.5, 0.5) * g_b))
                else:
                    k = {"bearing": 0, "wrap": int(rng.integers(-1, 2)), "wrap_far": int(rng.integers(2, 8)) * int(rng.choice([-1, 1])),
                         "past_50": int(rng.integers(8, 11)) * int(rng.choice([-1, 1]))}[kind]
                    out.append((zexp[0] + rng.uniform(-0.5, 0.5) * g_r, zexp[1] + sgn * g_b * q + 2 * math.pi * k))
    return out


# Gates that are no multiple of an fp32 ulp of any tested range: see _range_off_fp32.
RNGBRG_GATE_RANGE = 1.0 + 2.0 ** -10 / 3
VP_GATE_RANGE = 7.5 + 2.0 ** -10 / 3


def _range_off_fp32(nominal, g, delta=1e-6):
    """An expected range near `nominal` placed between fp32 numbers so that the fp32 range innovation of a measurement at
    r + g (1 - delta) is longer than the exact one by most of an ulp u: with g (1 - delta) = (K - phi) u, the range sits phi u / 2 above
    the fp32 number R (rounds down to R) and the measurement phi u / 2 below R + K u (rounds up to it), so the fp32 difference is K u,
    beyond g (1 + 1e-6).  Only the rounding term of the prefilter's range threshold keeps such a pair."""
    R = np.float32(nominal)
    u = float(np.spacing(R))
    q = g * (1.0 - delta) / u
    phi = math.ceil(q) - q
    assert 0.1 < phi < 0.98, phi                # (phi u is what the fp32 difference gains; phi / 2 stays below half an ulp)
    return float(R) + 0.5 * phi * u


def fp32_range_innovation(z, r):
    """|fl32(z) - fl32(r)| as the gate prefilter forms it (both in one binade: the fp32 subtraction is exact)."""
    return abs(float(np.float32(z) - np.float32(r)))


def rngbrg_gate_case(kind, seed=0, deltas=(1e-3, 1e-6), g_range=RNGBRG_GATE_RANGE, g_bearing=0.2):
    """(landmark, measurement) pairs at the innovation gates of the 2-D model.  Landmark m of every particle sits at (r_m, 0) with
    r_m up to 1e4 m, the pose at the origin with heading th_i, so that the expected measurement is exact in doubles: range
    sqrt(r_m^2) = r_m, bearing wrap(atan2(0, r_m) - th_i) = -th_i (|th_i| <= pi).  Headings near -+pi put the expected bearing on
    either side of +-pi.  kind: 'range' (|range innovation| = g (1 -+ delta); the ranges are placed by _range_off_fp32, so that the
    fp32 innovation of r + g (1 - 1e-6) exceeds g (1 + 1e-6)), 'bearing' (|bearing innovation| = g (1 -+ delta),
    measurement bearing within one turn), 'wrap' (plus 0 or +-1 turn), 'wrap_far' (+-2..7 turns: |bearing| < 50 rad),
    'past_50' (8..10 turns: beyond 50 rad, where the fp32 sweep leaves the bearing to the exact test).  The measurement noise R is
    wide enough that the raw (unwrapped) Mahalanobis gate passes every pair the innovation gates pass, so those gates decide.

    Returns the scenario fields (params, poses, w, mean, cov, Z) and `expect[i]`: the sorted (m, z) pairs that create a Gaussian."""
    rng = np.random.default_rng(seed)
    ths = [0.3, math.pi - 1e-3, -(math.pi - 1e-3), 2.0, -1.2, math.pi - 0.05]
    ranges = [_range_off_fp32(r, g_range) for r in (5.5, 37.0, 900.0, 9500.0)]
    n, nM = len(ths), len(ranges)
    P = dict(R=np.diag([4.0 * g_range ** 2, 1.0e3]), Pd=0.9, clutter=1e-4, rmax=2.0e4, rmin=0.5, rbuf=0.05,
             kf_range=g_range, kf_bearing=g_bearing, new_gaussian_md=3.0, n_eval=15, min_weight=0.75, weighting_md=3.0,
             merge_thr=MERGE_T, merge_infl=MERGE_F, prune_thr=PRUNE_T, birth_w=0.01, use_cluster=0,
             Q_lm=np.diag([2e-4, 2e-4]) * 0.01, pose_cov=np.diag([1e-6, 1e-6, 1e-6]))
    poses = np.array([[0.0, 0.0, th] for th in ths])
    mean = np.tile(np.array([[r, 0.0] for r in ranges]), (n, 1, 1))
    cov = np.tile(np.diag([1e-2, 1e-2]), (n, nM, 1, 1))
    w = np.tile(np.linspace(0.4, 0.7, nM), (n, 1))
    Z = []
    targets = [(i, m) for i in range(n) for m in range(nM)]
    rng.shuffle(targets)
    for i, m in targets:
        zexp = (ranges[m], -ths[i])
        Z += _gate_measurements(kind, zexp, g_range, g_bearing, deltas[:1] if len(Z) > 40 else deltas, rng)
        if len(Z) >= 56:
            break
    Z = np.array(Z[:64])
    expect, margin = [], math.inf
    for i in range(n):
        ex = []
        for m in range(nM):
            zx0, zx1 = Fraction(ranges[m]), -Fraction(ths[i])
            for z in range(len(Z)):
                ok, mg = gate_rngbrg(Fraction(float(Z[z, 0])) - zx0, Fraction(float(Z[z, 1])) - zx1, g_range, g_bearing)
                if mg < CERT_REL:
                    raise ValueError(f"gate decision within {mg:.3g} of its threshold")
                margin = min(margin, mg)
                if ok:
                    ex.append((m, z))
        expect.append(ex)
    return dict(n=n, nM=nM, params=P, poses=poses, pose_cov=np.asarray(P["pose_cov"]), w=w, mean=mean, cov=cov, Z=Z,
                particle_w=np.ones(n), expect=expect, margin=margin, ranges=ranges, g_range=g_range)


def vp_gate_case(kind, seed=0, deltas=(1e-3, 1e-6), g_range=VP_GATE_RANGE, g_bearing=0.2):
    """The same for the Victoria Park model.  Its sensor frame is the heading - pi/2: landmark m at (r_m, 0), heading th_i, expected
    bearing wrap(0 - fl(th_i - pi/2)), the double the device and the reference form.  The detection table is flat (Pd = 0.9 at any
    number of visible beams) and the scan reaches past every landmark, so that every landmark is detected; the diameter of the
    measurement equals the landmark's.  Expected bearings lie on either side of +-pi."""
    rng = np.random.default_rng(seed)
    th_sensor = [0.3, math.pi - 1e-3, -(math.pi - 1e-3), 2.0, -1.2]
    ths = [ts + math.pi / 2 for ts in th_sensor]
    zb = []
    for th in ths:
        tp = th - math.pi / 2                          # the device's tp.th, rounded as it rounds it
        a = 0.0 - tp
        assert -math.pi <= a <= math.pi
        zb.append(a)
    ranges = [_range_off_fp32(r, g_range) for r in (24.0, 45.0, 900.0, 9500.0)]
    n, nM = len(ths), len(ranges)
    P = dict(R=np.diag([4.0 * g_range ** 2, 1.0e3, 0.08]), Slb=1e-5, pd_table=[0.9] * 6, expected_clutter=6.0,
             rmax=2.0e4, rmin=0.5, bmax=math.pi, bmin=-math.pi, buffer_pd=0.4,
             kf_range=g_range, kf_bearing=g_bearing, new_gaussian_md=3.0, n_eval=15, min_weight=0.75, weighting_md=3.0,
             merge_thr=1.0, merge_infl=1.5, prune_thr=0.01, birth_w=0.01, use_cluster=0,
             birth_count_thr=5, birth_check_thr=10, birth_support_dist=2.0, birth_cur_thr=2,
             Q_lm=np.diag([5e-4, 5e-4, 1e-4]) * 0.025 ** 2, min_updates=2, min_measurements=15)
    poses = np.array([[0.0, 0.0, th] for th in ths])
    mean = np.tile(np.array([[r, 0.0, 0.5] for r in ranges]), (n, 1, 1))
    cov = np.tile(np.diag([1e-2, 1e-2, 1e-3]), (n, nM, 1, 1))
    w = np.tile(np.linspace(0.4, 0.7, nM), (n, 1))
    Z = []
    targets = [(i, m) for i in range(n) for m in range(nM)]
    rng.shuffle(targets)
    for i, m in targets:
        Z += _gate_measurements(kind, (ranges[m], zb[i]), g_range, g_bearing, deltas[:1] if len(Z) > 40 else deltas, rng)
        if len(Z) >= 56:
            break
    Z = np.array([(r, b, 0.5) for r, b in Z[:64]])
    expect, margin = [], math.inf
    for i in range(n):
        ex = []
        for m in range(nM):
            for z in range(len(Z)):
                ok, mg = gate_vp(Fraction(float(Z[z, 0])) - Fraction(ranges[m]), Fraction(float(Z[z, 1])) - Fraction(zb[i]), g_range, g_bearing)
                if mg < CERT_REL:
                    raise ValueError(f"gate decision within {mg:.3g} of its threshold")
                margin = min(margin, mg)
                if ok:
                    ex.append((m, z))
        expect.append(ex)
    scan = np.full(361, 3.0e4)
    return dict(n=n, nM=nM, params=P, poses=poses, pose_cov=np.zeros((3, 3)), w=w, mean=mean, cov=cov, Z=Z, scan=scan, model="vp",
                particle_w=np.ones(n), expect=expect, margin=margin, ranges=ranges, g_range=g_range)
