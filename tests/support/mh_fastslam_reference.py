"""An independent reference for the multi-hypothesis FastSLAM association of one particle (include/FastSLAM.hpp:430-556,
584-588, 696 with maxNDataAssocHypotheses_ > 1), in plain numpy and scipy.  It shares no code with the device path
(csrc/fastslam_mh.h, murty.h, hungarian_wave.h) nor with the oracle's restatement of the reference solver.

Per particle it gives

- the table: the dense nMZ x nMZ table of :458-481, nMZ = max(landmarks in range, measurements); a cell is
  fmax(floor, log N(z; z_exp, S)) of the range-bearing model, on the RAW difference z - z_exp as evalGaussianLikelihood takes it;
- the reduction: pairs that are each other's only cell above the floor are fixed (CostMatrix::reduce, written from its
  outcome -- row and column counts -- not from its scan), a 1 x 1 remainder is assigned, the rest goes to the solver;
- the ranked assignments: a textbook Murty (partition of a node's solution row by row; every child one call of
  scipy.optimize.linear_sum_assignment on the sub-table left after the fixed rows) with the reference's stop rules: the solver
  runs dry, kmax is reached, or best - score >= maxDiff;
- the effective log-weight of every kept assignment: the sum of its assigned cells that lie above the floor and whose Kalman
  correction passes the innovation gates (the weight is multiplied by exp of exactly that sum, :584-588 and :696; a gated
  correction is not performed and adds nothing).

Tie order is not modelled: assignments that differ only in which floor cell an unmatched row takes tie exactly and give
identical copies, so callers compare per parent the SORTED weights of its copies.
"""
import heapq
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests.support.prefilter_reference import np_measure, np_pd, wrap


def fastslam_table(P, pose, pose_cov, mu, Sig, Z, floor):
    """-> (rows, T, ok): rows = map indices of the landmarks in range (Pd != 0 or close to the sensing limit), T the
    nMZ x nMZ table, ok[k, z] whether the Kalman correction of row k with measurement z passes the innovation gates."""
    Z = np.asarray(Z, dtype=np.float64)
    nZ = len(Z)
    rows, exp = [], []
    for m in range(len(mu)):
        zexp, _, S, valid, r = np_measure(P, pose, pose_cov, mu[m], Sig[m])
        pd, close = np_pd(P, r)
        if pd != 0 or close:
            rows.append(m)
            exp.append((zexp, S, valid))
    n = max(len(rows), nZ)
    T = np.full((n, n), float(floor))
    ok = np.zeros((len(rows), nZ), dtype=bool)
    for k, (zexp, S, valid) in enumerate(exp):
        if not valid:
            continue
        Si = np.linalg.inv(S)
        norm = -0.5 * np.log((2 * np.pi) ** 2 * np.linalg.det(S))
        for z in range(nZ):
            e = Z[z] - zexp
            T[k, z] = max(floor, norm - 0.5 * (e @ Si @ e))
            ok[k, z] = not ((P["kf_range"] > 0 and abs(e[0]) > P["kf_range"]) or (P["kf_bearing"] > 0 and abs(wrap(e[1])) > P["kf_bearing"]))
    return rows, T, ok


def reduce_table(T, floor):
    """-> (fixed, iRed, jRed): fixed[x] = y for the pairs (x, y) that are each other's only cell above the floor; iRed / jRed
    the rows / columns left (a 1 x 1 remainder is assigned and both lists come back empty)."""
    live = T > floor
    rc, cc = live.sum(1), live.sum(0)
    fixed = {}
    for x in range(len(T)):
        if rc[x] == 1:
            y = int(np.argmax(live[x]))
            if cc[y] == 1:
                fixed[x] = y
    iRed = [x for x in range(len(T)) if x not in fixed]
    taken = set(fixed.values())
    jRed = [y for y in range(len(T)) if y not in taken]
    if len(iRed) == 1:
        fixed[iRed[0]] = jRed[0]
        iRed, jRed = [], []
    return fixed, iRed, jRed


def _solve(C, a, nf, banned):
    """Best completion of rows nf.. of C given rows 0 .. nf-1 fixed to a[:nf] and row nf barred from the columns `banned`."""
    n = len(C)
    cols = np.setdiff1d(np.arange(n), a[:nf], assume_unique=True)
    sub = C[nf:][:, cols].copy()
    if banned:
        sub[0, np.isin(cols, list(banned))] = -np.inf
    try:
        r, c = linear_sum_assignment(sub, maximize=True)
    except ValueError:          # no assignment avoids the barred cells
        return None
    full = np.concatenate([a[:nf], cols[c[np.argsort(r)]]]).astype(np.int64)
    return float(C[np.arange(n), full].sum()), full


def murty_ranked(C, kmax, max_diff=None, rejected=None):
    """The kmax best assignments of the square table C (largest sum first) as [(score, columns of the rows)]; with max_diff
    the list ends before the first score with best - score >= max_diff, and that score is appended to the list `rejected`
    (if given) when the window is what ended the list."""
    C = np.asarray(C, dtype=np.float64)
    n = len(C)
    tick = itertools.count()
    first = _solve(C, np.zeros(0, np.int64), 0, frozenset())
    heap = [(-first[0], next(tick), first[1], 0, frozenset())]
    out = []
    while heap and len(out) < kmax:
        neg, _, a, nf, banned = heapq.heappop(heap)
        if max_diff is not None and ((out and out[0][0] - (-neg) >= max_diff) or (not out and 0.0 >= max_diff)):
            if rejected is not None:
                rejected.append(-neg)
            break
        out.append((-neg, a))
        for i in range(nf, n):          # child i: rows < i as in a, row i anywhere but a[i] (and the node's own bars at i == nf)
            bar = (banned if i == nf else frozenset()) | {int(a[i])}
            got = _solve(C, a, i, bar)
            if got is not None:
                heapq.heappush(heap, (-got[0], next(tick), got[1], i, bar))
    return out


def particle_hypotheses(P, pose, pose_cov, mu, Sig, Z, floor, kmax, max_diff):
    """-> dict(nMZ, nRed, nH, logw (sorted, one per kept assignment), scores (of the reduced table, ranked), rejected, cells):
    what one particle's association keeps.  rejected: the first score beyond the window when the window ended the list (else
    empty).  cells[h] is the set of (row, measurement) pairs whose correction hypothesis h performs."""
    rows, T, ok = fastslam_table(P, pose, pose_cov, mu, Sig, Z, floor)
    nIn, nZ = len(rows), len(Z)
    fixed, iRed, jRed = reduce_table(T, floor)
    rejected = []
    if not iRed:
        ranked = [(0.0, np.zeros(0, np.int64))]
    else:
        ranked = murty_ranked(T[np.ix_(iRed, jRed)], kmax, max_diff, rejected)
    logw, cells = [], []
    for _, a in ranked:
        da = dict(fixed)
        da.update({iRed[r]: jRed[int(c)] for r, c in enumerate(a)})
        used = [(k, da[k]) for k in range(nIn) if da[k] < nZ and T[k, da[k]] > floor and ok[k, da[k]]]
        cells.append(frozenset(used))
        logw.append(float(sum(T[k, z] for k, z in used)))
    return dict(nMZ=len(T), nRed=len(iRed), nH=len(ranked), logw=sorted(logw), scores=[s for s, _ in ranked], rejected=rejected, cells=cells)


def bruteforce_ranked(C, kmax):
    """Every assignment of a table of dimension <= 7, ranked (a check of murty_ranked that needs no solver)."""
    C = np.asarray(C, dtype=np.float64)
    n = len(C)
    assert n <= 7
    s = sorted((float(sum(C[i, p[i]] for i in range(n))) for p in itertools.permutations(range(n))), reverse=True)
    return s[:kmax]
