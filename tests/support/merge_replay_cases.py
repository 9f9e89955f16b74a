"""Mixtures with planted conflict structures for the merge's speculative replay (csrc/merge_prune.h phase 2; csrc/vp.h, N <= 64).

Phase 2 of gm_merge_particle walks up to 64 candidate rows at once, every lane against the states the round started with, and
then has to find out which of those walks the reference's sequential scan would have made: claims, the alive / claimed fixed point,
the prefix commit, the re-walks of the sub-rounds and seq_replay.  The random mixtures of the suite meet those stages by chance.
The constructors here plant them: how long a chain of "row k lives only if row k - 1 died" gets, how many rows contest one entry,
whether a re-walked row changes what the next row must do, and where the 64-row round boundary falls.

Vocabulary (all in MERGE ORDER, the weight-descending order _finish_merge_case leaves):
  rows(a)    entries with some j > a that passes the reference's pair test against the initial states;
  S(a)       the isolated walk: what row a absorbs when it scans the initial mixture alone (what a lane computes speculatively);
  truth(a)   what the certified replay of the whole merge (prefilter_reference.certified_merge) says a absorbs;
  listed(a)  what the candidate scan lists for a: survivors j > a with |x_j - x_a| <= max(r_a, r_j), reserves within twice that,
             r = t sqrt(tr S) (merge_prune.h phase 1a; 2-D only).

Every constructor returns the case dict of _finish_merge_case (inputs, certified merges, sizes, merged weights) plus
  roles[i]   name -> merge indices of the structure's members in particle i,
  stay[i]    rows that must be finished from their lists (listing and slack margins hold),
  leave[i]   rows that must leave their lists (the opposite conditions, same margins).
Three deliberately wrong schedulers (W1-W3) give the results a broken validation would produce; the tests assert that the planted
cases tell them from the certified result."""
import math

import numpy as np

from tests.support import prefilter_reference as pr

SPACING = 0.9            # neighbours on a line: md2 = 0.81 t^2
CROSS = 1e-2             # variance across the line / along it
BOX_RADII = 256.0        # bounding box per side, in largest prefilter radii
LIST_MARGIN = 0.05       # no entry within 5 % of a listing boundary (r or 2 r)
SLACK_STAY = 0.4         # rows that stay use less than 0.4 of their slack bound; rows that leave more than 1 / 0.4 of it


# ---- the reference's rule on one row (fp64; the certified replay decides, these only describe structure) --------------------

def _md2(e, Sinv):
    return np.einsum("...i,...ij,...j->...", e, Sinv, e)


def pass_matrix(case, i):
    """P[a, j] (j > a): j passes the pair test against a, both in their initial states."""
    mu, Sg, t2 = case["mean"][i], case["cov"][i], case["t"] ** 2
    Si = np.linalg.inv(Sg)
    e = mu[None, :, :] - mu[:, None, :]                       # e[a, j] = x_j - x_a
    d1 = np.einsum("aji,aik,ajk->aj", e, Si, e)
    d2 = np.einsum("aji,jik,ajk->aj", e, Si, e)
    P = (d1 <= t2) | (d2 <= t2)
    return np.triu(P, 1)


def rows(case, i):
    memo = case.setdefault("_rows", {})                       # (the cases are built once and never changed)
    if i not in memo:
        memo[i] = [int(a) for a in np.nonzero(pass_matrix(case, i).any(axis=1))[0]]
    return list(memo[i])


def walk(case, i, a, alive=None):
    """The greedy scan of row a alone: j ascending above a, against a's current state, entries with alive[j] False skipped.
    Returns (absorbed, excursion): excursion is the largest (path length of the mean so far + growth of the prefilter radius)."""
    w, mu, Sg, t, f = case["w"][i], case["mean"][i], case["cov"][i], case["t"], case["f"]
    n = len(w)
    alive = np.ones(n, bool) if alive is None else alive
    memo = case.setdefault("_sinv", {})
    if i not in memo:
        memo[i] = np.linalg.inv(Sg)
    Sinv = memo[i]
    x, S, wa = mu[a].copy(), Sg[a].copy(), w[a]
    r0 = t * math.sqrt(S[0, 0] + S[1, 1])
    absorbed, shift, exc, lo = [], 0.0, 0.0, a + 1
    while lo < n:
        js = np.arange(lo, n)[alive[lo:]]
        if js.size == 0:
            break
        e = mu[js] - x
        ok = (_md2(e, np.linalg.inv(S)) <= t * t) | (_md2(e, Sinv[js]) <= t * t)
        ok &= (wa + w[js]) != 0
        if not ok.any():
            break
        j = int(js[np.argmax(ok)])
        wm = wa + w[j]
        xm = (x * wa + mu[j] * w[j]) / wm
        d1, d2 = xm - x, xm - mu[j]
        S = (wa * (S + f * np.outer(d1, d1)) + w[j] * (Sg[j] + f * np.outer(d2, d2))) / wm
        shift += float(np.linalg.norm(d1[:2]))
        x, wa = xm, wm
        exc = max(exc, shift + max(t * math.sqrt(S[0, 0] + S[1, 1]) - r0, 0.0))
        absorbed.append(j)
        lo = j + 1
    return absorbed, exc


def isolated(case, i, a):
    memo = case.setdefault("_isolated", {})
    if (i, a) not in memo:
        memo[(i, a)] = walk(case, i, a)[0]
    return list(memo[(i, a)])


def truth(case, i, a):
    return [j for r, j in case["merges"][i] if r == a]


def alive_before(case, i, a):
    """Liveness when the reference reaches row a: everything rows below a absorbed is gone."""
    al = np.ones(len(case["w"][i]), bool)
    for r, j in case["merges"][i]:
        if r < a:
            al[j] = False
    return al


# ---- phase 1a's listing and slack (2-D) ---------------------------------------------------------------------------------

def radii(case, i):
    return case["t"] * np.sqrt(case["cov"][i][:, 0, 0] + case["cov"][i][:, 1, 1])


def listing(case, i, a):
    """(survivors, reserves, ratio): the entries j > a the scan lists for a, and how close any j > a comes to a listing boundary
    (the smallest |d / r - 1| and |d / 2 r - 1|, r = max(r_a, r_j))."""
    r = radii(case, i)
    d = np.linalg.norm(case["mean"][i][:, :2] - case["mean"][i][a, :2], axis=1)
    j = np.arange(len(r))
    rm = np.maximum(r, r[a])
    up = j > a
    surv = j[up & (d <= rm)]
    res = j[up & (d > rm) & (d < 2 * rm)]
    q = d[up] / rm[up]
    ratio = float(np.min(np.minimum(np.abs(q - 1), np.abs(q / 2 - 1)))) if up.any() else math.inf
    return [int(v) for v in surv], [int(v) for v in res], ratio


def cell_edge(case, i):
    """The thinnest cell either merge grid can use: the bounding box's shorter side over 64."""
    xy = case["mean"][i][:, :2]
    return float(np.min(xy.max(axis=0) - xy.min(axis=0))) / 64.0


def slack_bound(case, i, a):
    """Half the distance to the nearest entry above a that the scan does not list, capped by cell edge - largest radius."""
    r = radii(case, i)
    d = np.linalg.norm(case["mean"][i][:, :2] - case["mean"][i][a, :2], axis=1)
    j = np.arange(len(r))
    far = (j > a) & (d >= 2 * np.maximum(r, r[a]))
    cap = cell_edge(case, i) - float(r.max())
    return min(0.5 * float(d[far].min()), cap) if far.any() else cap


def fp32_allowance(case, i):
    """What the scan adds to a radius for the fp32 coordinates (1.5 errAbs, errAbs = 3e-7 max|x|), relative to the smallest radius."""
    return 1.5 * 3.0e-7 * float(np.max(np.abs(case["mean"][i][:, :2]))) / float(radii(case, i).min())


# ---- deliberately wrong schedulers -----------------------------------------------------------------------------------------

def _weights_after(case, i, commits):
    """Survivor weights, descending, when every (row, absorbed list) of `commits` is applied (an entry may be absorbed twice: it is
    gone and both rows carry its weight)."""
    w = case["w"][i].copy()
    gone = np.zeros(len(w), bool)
    for a, js in commits:
        for j in js:
            w[a] += case["w"][i][j]
            gone[j] = True
    return np.sort(w[~gone])[::-1]


def wrong_scheduler(case, i, kind):
    """Survivor weights (descending) under a broken validation of the speculative walks.
    W1: every row commits its isolated walk unless the row itself was absorbed; no claim handling.
    W2: a row that loses a claim keeps its initial state and absorbs nothing.
    W3: liveness and the one re-walk of a losing row use the holes of the earlier rows' ISOLATED walks, not the committed ones."""
    rws = rows(case, i)
    S = {a: isolated(case, i, a) for a in rws}
    n = len(case["w"][i])
    dead = np.zeros(n, bool)             # committed holes
    spec = np.zeros(n, bool)             # holes of the isolated walks of the rows so far
    commits = []
    for a in rws:
        if kind == "W3":
            if spec[a]:
                spec[S[a]] = True
                continue
            js = S[a] if not spec[S[a]].any() else walk(case, i, a, ~spec)[0]
            spec[S[a]] = True
        else:
            if dead[a]:
                continue
            if kind == "W1":
                js = S[a]
            elif kind == "W2":
                js = S[a] if not dead[S[a]].any() else []
            else:
                raise ValueError(kind)
        dead[js] = True
        commits.append((a, js))
    return _weights_after(case, i, commits)


def certified_weights(case, i):
    return np.sort(case["merged_w"][i])[::-1]


def distinguishes(case, kind):
    """Some particle's certified result differs from the wrong scheduler's, in size or in a survivor weight."""
    for i in range(len(case["w"])):
        ww, cw = wrong_scheduler(case, i, kind), certified_weights(case, i)
        if len(ww) != len(cw) or np.max(np.abs(ww / cw - 1)) > 1e-12:
            return True
    return False


# ---- construction ----------------------------------------------------------------------------------------------------------

def _line_cov(s, u, dim):
    """Variance s^2 along the unit vector u (x, y), CROSS s^2 across and in the third coordinate."""
    C = np.zeros((dim, dim))
    C[:2, :2] = s * s * (np.outer(u, u) + CROSS * (np.eye(2) - np.outer(u, u)))
    if dim == 3:
        C[2, 2] = CROSS * s * s
    return C


def _iso_cov(s, dim):
    C = s * s * np.eye(dim)
    if dim == 3:
        C[2, 2] = CROSS * s * s
    return C


def _desc_weights(rng, n, lo, hi):
    """n distinct weights in (lo, hi), descending, no two closer than 1e-3 of the range."""
    while True:
        w = np.sort(rng.uniform(lo, hi, n))[::-1]
        if n < 2 or np.min(-np.diff(w)) > 1e-3 * (hi - lo) / n:
            return w


class _Particle:
    """Entries of one particle with a tag each; `finish` pins the bounding box with two anchors."""

    def __init__(self, dim):
        self.dim, self.w, self.x, self.S, self.tag = dim, [], [], [], []

    def add(self, tag, w, xy, S):
        x = np.full(self.dim, 0.5)
        x[:2] = xy
        self.w.append(float(w)); self.x.append(x); self.S.append(np.array(S, dtype=np.float64)); self.tag.append(tag)

    def arrays(self, t, rng, anchors):
        w, x, S = np.array(self.w), np.array(self.x), np.array(self.S)
        tags = list(self.tag)
        # a random rotation and translation of everything planted
        th = rng.uniform(0, 2 * np.pi)
        R = np.eye(self.dim)
        R[:2, :2] = [[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]
        ctr = 0.5 * (x[:, :2].max(axis=0) + x[:, :2].min(axis=0))
        x[:, :2] = (x[:, :2] - ctr) @ R[:2, :2].T
        S = R @ S @ R.T
        S = 0.5 * (S + np.swapaxes(S, 1, 2))
        if anchors:
            rmax = t * math.sqrt(float(np.max(S[:, 0, 0] + S[:, 1, 1])))
            half = 0.5 * max(BOX_RADII * 1.02 * rmax, 1.5 * float(np.max(np.abs(x[:, :2]))) * 2)
            sa = math.sqrt(float(np.min(S[:, 0, 0] + S[:, 1, 1])) / 2)
            for k, corner in enumerate(([-half, -half], [half, half])):
                c = np.full(self.dim, 0.5); c[:2] = corner
                x = np.vstack([x, c]); S = np.concatenate([S, _iso_cov(sa, self.dim)[None]])
                w = np.append(w, 0.02 + 0.002 * k); tags.append(("anchor", k))      # (above the prune threshold: the anchors survive)
        x[:, :2] += rng.uniform(-20.0, 20.0, 2)
        return w, x, S, tags


def _finish(parts, t, f, rng, anchors=True, stay=(), leave=()):
    """Sort every particle by weight (descending), certify, and name the structure's members by merge index."""
    ws, xs, Ss, tags = [], [], [], []
    for p in parts:
        w, x, S, tg = p.arrays(t, rng, anchors)
        o = np.argsort(-w, kind="stable")
        ws.append(w[o]); xs.append(x[o]); Ss.append(S[o]); tags.append([tg[k] for k in o])
    case = pr._finish_merge_case(np.array(ws), np.array(xs), np.array(Ss), t, f, jitter=False)
    roles = []
    for tg in tags:
        r = {}
        for m, (name, k) in enumerate(tg):
            r.setdefault(name, {})[k] = m
        roles.append({name: [d[k] for k in sorted(d)] for name, d in r.items()})
    case["roles"] = roles
    case["stay"] = [sorted(m for name in stay for m in r.get(name, [])) for r in roles]
    case["leave"] = [sorted(m for name in leave for m in r.get(name, [])) for r in roles]
    return case


def _params(dim):
    return (pr.MERGE_T, pr.MERGE_F, 0.2) if dim == 2 else (1.0, 1.5, 0.2)


def chain_case(L, dim=2, n_particles=8, seed=0, chains=1, anchors=True):
    """`chains` alternating chains of L entries each: a_0 .. a_{L-1} on a line, SPACING t s apart, weights descending along it (the
    chains' weights interleave, so their rows alternate over the lanes).  Every a_k passes a_{k+1}; a merged pair does not reach the
    next entry: S(a_k) = [a_{k+1}], truth (a_0, a_1), (a_2, a_3), ...: lane k is alive exactly when lane k - 1 is not."""
    t, f, s = _params(dim)
    rng = np.random.default_rng(seed)
    u = np.array([1.0, 0.0])
    parts = []
    for _ in range(n_particles):
        p = _Particle(dim)
        w = _desc_weights(rng, chains * L, 0.3, 0.9)
        for c in range(chains):
            for k in range(L):
                xy = np.array([k * SPACING * t * s, c * 40.0 * t * s]) + rng.uniform(-1e-3, 1e-3, 2) * t * s
                p.add((f"chain{c}", k), w[k * chains + c], xy, _line_cov(s, u, dim))
        parts.append(p)
    return _finish(parts, t, f, rng, anchors, stay=[f"chain{c}" for c in range(chains)])


def comb_case(d, dim=2, n_particles=8, seed=0, anchors=True):
    """The chain's geometry with the top weights on the even positions r_0 .. r_d and the lower ones on the odd positions e_1 .. e_d
    (e_i between r_{i-1} and r_i).  Alone, r_i absorbs e_i, moves away and fails e_{i+1}: S(r_i) = [e_i].  In truth r_0 takes e_1, so
    r_1 stays where it is and takes e_2, and so on down the line: truth(r_i) = [e_{i+1}], r_d ends alone.  Every re-walk changes what
    the next row must do."""
    t, f, s = _params(dim)
    rng = np.random.default_rng(seed)
    u = np.array([1.0, 0.0])
    parts = []
    for _ in range(n_particles):
        p = _Particle(dim)
        wr, we = _desc_weights(rng, d + 1, 0.65, 0.9), _desc_weights(rng, d, 0.3, 0.55)
        for k in range(d + 1):
            p.add(("r", k), wr[k], np.array([2 * k * SPACING * t * s, 0.0]) + rng.uniform(-1e-3, 1e-3, 2) * t * s, _line_cov(s, u, dim))
        for k in range(1, d + 1):
            p.add(("e", k), we[k - 1], np.array([(2 * k - 1) * SPACING * t * s, 0.0]) + rng.uniform(-1e-3, 1e-3, 2) * t * s, _line_cov(s, u, dim))
        parts.append(p)
    return _finish(parts, t, f, rng, anchors, stay=["r"])


FAN_WC = 1.5e-4          # the contested entry's weight
FAN_TIGHT = 0.02         # a fan row's standard deviation over the contested entry's


def fan_case(k, partners=False, dim=2, n_particles=8, seed=0, anchors=True):
    """k heavy, tight rows on a circle of radius SPACING t s_c around one wide, very light entry c with the highest index among them:
    every row passes c through c's covariance, no row passes another: S(a_i) = [c], and only the first row gets c.  The rows are as
    far apart as the circle allows (2 pi R / k), which bounds their slack: c's weight is FAN_WC (not 1e-3) so that a row that
    absorbs c grows by less than 0.4 of that slack at k = 70 too.
    partners: every row has a private partner p_i with an index above c that passes from the row's initial state and from its state
    after c: the winner ends as a + c + p, every loser as a + p from its INITIAL state.  (c passes every p_i too, so c is a row, dead
    in truth; with k > 8 it is not listable.)"""
    t, f, _ = _params(dim)
    rng = np.random.default_rng(seed)
    sc_ = 0.4
    sa = FAN_TIGHT * sc_
    R = SPACING * t * sc_
    parts = []
    for _ in range(n_particles):
        p = _Particle(dim)
        w = rng.permutation(_desc_weights(rng, k, 0.5, 0.9))
        wp = _desc_weights(rng, k, 0.2 * FAN_WC, 0.8 * FAN_WC)
        ph = rng.uniform(0, 2 * np.pi)
        for q in range(k):
            a = ph + 2 * np.pi * q / k
            ur = np.array([math.cos(a), math.sin(a)])
            p.add(("row", q), w[q], R * ur * (1 + rng.uniform(-1e-3, 1e-3)), _iso_cov(sa, dim))
            if partners:
                p.add(("p", q), wp[q], (R + 0.6 * t * sa) * ur, _iso_cov(0.3 * sa, dim))
        p.add(("c", 0), FAN_WC, rng.uniform(-1e-3, 1e-3, 2) * R, _iso_cov(sc_, dim))
        parts.append(p)
    return _finish(parts, t, f, rng, anchors, stay=["row"])


def _from_base(base, i, dim=2):
    p = _Particle(dim)
    for m in range(len(base["w"][i])):
        p.add(("base", m), base["w"][i][m], base["mean"][i][m], base["cov"][i][m])
    return p


def absorbed_slack_row_case(n_particles=8, seed=0):
    """(4a) slack_case's clusters (A absorbs the wide B, outgrows its slack and then takes C) with a heavier row H next to every A:
    H absorbs A (then B, then C).  A is a row whose own walk would leave its list; it is dead and must be neither replayed nor
    committed."""
    base = pr.slack_case(n_particles=n_particles, seed=seed)
    rng = np.random.default_rng(seed + 1)
    parts = []
    for i in range(n_particles):
        p = _from_base(base, i)
        for c, (a, b, cc) in enumerate(base["roles"][i]):
            xa, xc = base["mean"][i][a], base["mean"][i][cc]
            u = (xc - xa) / np.linalg.norm(xc - xa)
            p.tag[a], p.tag[b], p.tag[cc] = ("A", c), ("B", c), ("C", c)
            p.add(("H", c), 0.99 - 0.01 * c + 1e-4 * i, xa - 0.8 * base["t"] * 0.1 * u, 0.1 * 0.1 * np.eye(2))
        parts.append(p)
    return _finish(parts, base["t"], base["f"], rng, leave=["H", "A"])


def contested_slack_row_case(n_particles=8, seed=0):
    """(4b) slack_case's clusters with a second wide entry B0 (heavier than B) 0.8 m from A and an earlier, tight row G beyond it, with
    a light fence entry F next to G that bounds G's slack.  Alone, A takes B0 first and leaves its list at once; G takes B0 too, and
    wins.  With B0 gone A takes B, outgrows its slack again and must be finished by the sequential scan (then C): truth(A) = [B, C]
    against S(A) = [B0, B, C]."""
    base = pr.slack_case(n_particles=n_particles, seed=seed)
    rng = np.random.default_rng(seed + 2)
    parts = []
    for i in range(n_particles):
        p = _from_base(base, i)
        for c, (a, b, cc) in enumerate(base["roles"][i]):
            xa, xc = base["mean"][i][a], base["mean"][i][cc]
            u = (xc - xa) / np.linalg.norm(xc - xa)
            v = np.array([-u[1], u[0]])
            p.tag[a], p.tag[b], p.tag[cc] = ("A", c), ("B", c), ("C", c)
            p.add(("B0", c), 0.75 - 0.01 * c + 1e-4 * i, xa + 0.8 * v, 2.0 * 2.0 * np.eye(2))
            p.add(("G", c), 0.99 - 0.01 * c + 1e-4 * i, xa + 1.65 * v, 0.05 * 0.05 * np.eye(2))
            p.add(("F", c), 0.2 - 0.01 * c + 1e-4 * i, xa + 1.73 * v, 0.01 * 0.01 * np.eye(2))
        parts.append(p)
    return _finish(parts, base["t"], base["f"], rng, leave=["G", "A"])


def contested_ring_case(n_particles=8, seed=0):
    """(4c) listing_limit_case's ring-9 clusters (a centre with nine prefilter survivors: not listable, the sequential scan's) with an
    earlier, listable row Q just outside the heaviest ring entry E of every centre -- the entry the centre's own scan would absorb
    first: Q takes E, and the centre's scan must find it gone and go on to the next."""
    base = pr.listing_limit_case(9, 0.9, n_particles=n_particles, seed=seed)
    rng = np.random.default_rng(seed + 3)
    t = base["t"]
    parts = []
    for i in range(n_particles):
        p = _from_base(base, i)
        centres = np.nonzero(np.isclose(base["cov"][i][:, 0, 0], 0.04))[0]
        for c, a in enumerate(centres):
            xa = base["mean"][i][a]
            d = np.linalg.norm(base["mean"][i] - xa, axis=1)
            ring = [int(m) for m in np.nonzero((d > 0) & (d < 0.2))[0]]
            assert len(ring) == 9
            e = min(ring)                    # the heaviest ring entry: the first the centre's own scan would absorb
            ur = (base["mean"][i][e] - xa) / d[e]
            p.tag[a], p.tag[e] = ("centre", c), ("E", c)
            for q, m in enumerate(ring):
                if m != e:
                    p.tag[m] = ("ring", 8 * c + q)
            p.add(("Q", c), 0.95 + 0.005 * c + 1e-4 * i, base["mean"][i][e] + 0.025 * ur, 0.06 * 0.06 * np.eye(2))
        parts.append(p)
    return _finish(parts, t, base["f"], rng, stay=["Q"], leave=["centre"])
