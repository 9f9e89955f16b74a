"""A numpy restatement of one rfsgpu_step_estimate record and its planes (include/rfsgpu.h [estimate], csrc/estimate_log.h), from
arrays the per-slot getters return; plus a synthetic trace in the layout estimate_log_read returns, for tests without a GPU."""
import numpy as np

EPS = np.finfo(np.float64).eps


def select_best(w):
    """The serial rule of analysis2dSim.cpp:159-167: the first slot whose weight is strictly greater than every earlier one, starting
    from 0; slot 0 when no weight is > 0 (all zero, negative or NaN)."""
    best, hi = 0, 0.0
    for i, wi in enumerate(np.asarray(w, dtype=np.float64)):
        if wi > hi:
            best, hi = i, wi
    return best


def existence(w):
    """A FastSLAM Gaussian's logged weight from its log-odds."""
    return 1 - 1 / (1 + np.exp(np.asarray(w, dtype=np.float64)))


def reference_row(w, x, gm_of, thr, max_est, lo=0, log_odds=False):
    """w [n], x [n, 3]: the block's LIVE weights and poses; gm_of(global slot) -> (weights [m], means [m, 2], covs [m, 2, 2]) in
    mixture order; lo the block's first global slot.  Returns (fields, planes [6, max_est]) with the integer fields exact, the copied
    fields as they are and the sums in numpy's float64."""
    w, x = np.asarray(w, dtype=np.float64), np.asarray(x, dtype=np.float64).reshape(-1, 3)
    n = len(w)
    planes = np.zeros((6, max_est))
    if n == 0:
        nan = float("nan")
        return dict(status=0, best_slot=lo, n_particles=0, n_est=0, n_logged=0, cardinality=0.0, best_x=nan, best_y=nan, best_theta=nan,
                    mean_x=nan, mean_y=nan, mean_cos=nan, mean_sin=nan), planes
    best = select_best(w)
    gw, mean, cov = gm_of(lo + best)
    gw = existence(gw) if log_odds else np.asarray(gw, dtype=np.float64)
    exists = gw >= 0                                   # (merged-away entries carry a negative weight)
    keep = exists & (gw >= thr)
    n_est = int(keep.sum())
    k = min(n_est, max_est)
    planes[0, :k], planes[1, :k] = mean[keep][:k, 0], mean[keep][:k, 1]
    planes[2, :k], planes[3, :k], planes[4, :k] = cov[keep][:k, 0, 0], cov[keep][:k, 0, 1], cov[keep][:k, 1, 1]
    planes[5, :k] = gw[keep][:k]
    with np.errstate(invalid="ignore", divide="ignore"):
        ws = w.sum()
        means = [float((q * w).sum() / ws) for q in (x[:, 0], x[:, 1], np.cos(x[:, 2]), np.sin(x[:, 2]))]
    return dict(status=int(n_est > max_est), best_slot=lo + best, n_particles=n, n_est=n_est, n_logged=k, cardinality=float(gw[exists].sum()),
                best_weight=w[best], weight_sum=float(ws), best_x=x[best, 0], best_y=x[best, 1], best_theta=x[best, 2],
                mean_x=means[0], mean_y=means[1], mean_cos=means[2], mean_sin=means[3]), planes


def mean_bound(n, q):
    """4 N eps max(1, max|q|): the standard bound N eps max|q| for a sum of N non-negative-weighted terms against its exact value,
    taken for both sums being compared and doubled for the division and the device's sincos."""
    q = np.asarray(q, dtype=np.float64)
    return 4 * n * EPS * max(1.0, float(np.abs(q).max()) if q.size else 0.0)


def synthetic_trace(dtype, n_filters=2, n_steps=3, n_particles=5, sizes=(0, 1, 4), max_est=4, seed=1):
    """(hdr, gauss, part), truth per filter: a made-up run in estimate_log_read's layout.  Every number is a multiple of 1/64 of modest
    size, which %f prints exactly; row r of every filter holds sizes[r] Gaussians on both sides of the analysis' 0.75."""
    rng = np.random.default_rng(seed)
    g64 = lambda lo, hi, shape: rng.integers(int(lo * 64), int(hi * 64) + 1, shape) / 64.0
    dt = 0.125
    hdr = np.zeros((n_steps, n_filters), dtype=dtype)
    gauss = np.zeros((n_steps, n_filters, 6, max_est))
    part = np.zeros((n_steps, n_filters, 4, n_particles))
    truths = []
    for b in range(n_filters):
        K = n_steps + 1
        truths.append(dict(gt=g64(-2, 2, (K, 3)), odom=g64(-0.25, 0.25, (K, 3)), landmarks=g64(-3, 3, (6, 2)),
                           first_seen=np.array([-1.0, 0.125, 0.125, 0.25, 0.375, 4.0]), dt=dt))
        truths[b]["gt"][0] = 0.0
        for r in range(n_steps):
            part[r, b, :3] = g64(-2, 2, (3, n_particles))
            w = g64(1 / 64, 1, n_particles)
            best = (2 * r + b) % n_particles
            w[best] = 1.5
            if r == 1:
                w[(best + 2) % n_particles] = 1.5          # the maximum held twice: the first holder is the best
                best = min(best, (best + 2) % n_particles)
            part[r, b, 3] = w
            m = sizes[r]
            gauss[r, b, 0:2, :m] = truths[b]["landmarks"][:m].T + g64(-0.125, 0.125, (2, m))
            gauss[r, b, 2, :m], gauss[r, b, 3, :m], gauss[r, b, 4, :m] = 1 / 64, 0.0, 2 / 64
            gauss[r, b, 5, :m] = [1.0, 0.75, 0.5, 1.25][:m]
            h = hdr[r, b]
            h["t"], h["best_slot"], h["n_particles"], h["n_est"], h["n_logged"] = (r + 1) * dt, b * n_particles + best, n_particles, m, m
            h["cardinality"], h["best_weight"], h["weight_sum"] = gauss[r, b, 5, :m].sum(), 1.5, w.sum()
            h["best_x"], h["best_y"], h["best_theta"] = part[r, b, 0, best], part[r, b, 1, best], part[r, b, 2, best]
    return (hdr, gauss, part), truths
