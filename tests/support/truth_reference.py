"""numpy restatement of csrc/batch_truth.h (batch_truth_kernel): the ground truth of one filter -- trajectory, odometry, landmarks, first-seen
times and n_det_max -- from the Philox draws the kernel takes, by the rules of sim2d_driver.generate.  Counter layout:
(index, block | attempt << 8, 0, 0) under the truth key; blocks 8 (dx attempts), 9 (dy, dz), 10 (landmark), 11 / 12 (odometry noise)."""
import math

import numpy as np

from tests.support import device_loop_reference as dl
from tests.support import sensor_reference as sr

U64 = np.uint64
MASK = dl.MASK
MAX_REDRAWS = 64
BLOCK_DX, BLOCK_DYZ, BLOCK_LANDMARK, BLOCK_ODO_XY, BLOCK_ODO_TH = 8, 9, 10, 11, 12


def config(P, kmax=None):
    """The generation keys of a dict like sim2d_driver.C1_SIM (what sim2d_driver.truth_config puts into the C struct)."""
    return dict(k_full=int(P["kmax"]), n_segments=int(P["n_segments"]), n_landmarks=int(P["n_landmarks"]), n_still=50, n_pinned=100, dt=P["dt"],
                max_dx=P["max_dx"], max_dy=P["max_dy"], max_dz=P["max_dz"], min_dx=P["min_dx"], var_odo=[P["vardx"], P["vardy"], P["vardz"]],
                rmax=P["rmax"], rmin=P["rmin"])


def _blocks(index, block, seed):
    i = np.atleast_1d(np.asarray(index)).astype(U64)
    z = np.zeros(i.shape, dtype=U64)
    return dl.philox4x32_10([i, z + U64(block), z, z], (seed & MASK, seed >> 32))


def segment_of_step(k, c):
    """The segment step k > n_still lies in: segment s starts at max(spacing s, n_still + 1 + s)."""
    spacing = max(c["k_full"] // max(c["n_segments"], 1), 1)
    return min(k // spacing, k - c["n_still"] - 1)


def segment_start_steps(K, c):
    """The steps < K at which a new segment starts (generate(): the steps where a displacement is drawn)."""
    return [k for k in range(c["n_still"] + 1, K) if k == c["n_still"] + 1 or segment_of_step(k, c) != segment_of_step(k - 1, c)]


def landmark_steps(K, c):
    """k_j = max(lspacing j, j + 1) for the landmarks a run of K steps places."""
    if c["n_landmarks"] <= 0:
        return []
    lsp = max(c["k_full"] // c["n_landmarks"], 1)
    out, j = [], 0
    while max(lsp * j, j + 1) < K:
        out.append(max(lsp * j, j + 1))
        j += 1
    return out


def dx_from_draws(us, c):
    """A segment's dx from its attempts' draws us[0 ... 63]: the first whose u max_dx dt is not below min_dx dt; none: the LAST draw
    mapped into the limits.  Returns (dx, attempts used, fell back)."""
    dt = c["dt"]
    for a, u in enumerate(us[:MAX_REDRAWS]):
        dx = float(u) * c["max_dx"] * dt
        if not dx < c["min_dx"] * dt:
            return dx, a + 1, False
    u = float(us[MAX_REDRAWS - 1])
    return (c["min_dx"] + u * (c["max_dx"] - c["min_dx"])) * dt, MAX_REDRAWS, True


def segment_draws(s, c, seed):
    """(dx, dy, dz) of segment s, and (attempts, fell back)."""
    att = np.arange(MAX_REDRAWS, dtype=U64)
    i = np.full(MAX_REDRAWS, s, dtype=U64)
    z = np.zeros(MAX_REDRAWS, dtype=U64)
    r = dl.philox4x32_10([i, U64(BLOCK_DX) | (att << U64(8)), z, z], (seed & MASK, seed >> 32))
    dx, n_att, fell = dx_from_draws(sr.u01_half_open(r[0], r[1]), c)
    r = _blocks([s], BLOCK_DYZ, seed)
    dt = c["dt"]
    dy = (float(sr.u01_half_open(r[0], r[1])[0]) * c["max_dy"] * 2 - c["max_dy"]) * dt
    dz = (float(sr.u01_half_open(r[2], r[3])[0]) * c["max_dz"] * 2 - c["max_dz"]) * dt
    return (dx, dy, dz), (n_att, fell)


def displacements(K, c, seed):
    """disp [K, 3] and per drawn segment (attempts, fell back)."""
    disp = np.zeros((K, 3))
    info, cache = {}, {}
    for k in range(c["n_still"] + 1, K):
        s = segment_of_step(k, c)
        if s not in cache:
            cache[s], info[s] = segment_draws(s, c, seed)
        disp[k] = cache[s]
    return disp, info


def odometry_deviates(K, seed):
    """g [K, 3]: block 11 gives g_x = rad cos, g_y = rad sin; block 12's rad cos gives g_theta (row 0 is not used)."""
    g = np.zeros((K, 3))
    r = _blocks(np.arange(K), BLOCK_ODO_XY, seed)
    rad, ang = np.sqrt(-2.0 * np.log(dl.u01_open_low(r[0], r[1]))), 2.0 * np.pi * dl.u01_open_low(r[2], r[3])
    g[:, 0], g[:, 1] = rad * np.cos(ang), rad * np.sin(ang)
    r = _blocks(np.arange(K), BLOCK_ODO_TH, seed)
    rad, ang = np.sqrt(-2.0 * np.log(dl.u01_open_low(r[0], r[1]))), 2.0 * np.pi * dl.u01_open_low(r[2], r[3])
    g[:, 2] = rad * np.cos(ang)
    return g


def odometry(disp, c, seed):
    K = disp.shape[0]
    odom = disp + np.sqrt(np.asarray(c["var_odo"], dtype=np.float64)) * c["dt"] * odometry_deviates(K, seed)
    odom[0] = 0.0
    return odom


def step(x, u):
    """MotionModel_Odometry2d::step of one pose."""
    return dl.odometry_step(np.asarray(x, dtype=np.float64).reshape(1, 3), np.asarray(u, dtype=np.float64))[0]


def trajectory(disp):
    gt = np.zeros_like(disp)
    for k in range(1, disp.shape[0]):
        gt[k] = step(gt[k - 1], disp[k])
    return gt


def landmarks(gt, c, seed):
    """The landmarks placed from the poses gt (the device's or the restatement's own)."""
    ks = landmark_steps(gt.shape[0], c)
    if not ks:
        return np.zeros((0, 2))
    r = _blocks(np.arange(len(ks)), BLOCK_LANDMARK, seed)
    rr, bb = sr.u01_half_open(r[0], r[1]) * c["rmax"], sr.u01_half_open(r[2], r[3]) * 2 * np.pi
    x = gt[ks]
    return np.stack([x[:, 0] + rr * np.cos(x[:, 2] + bb), x[:, 1] + rr * np.sin(x[:, 2] + bb)], axis=1)


def ranges(gt, lm):
    """True ranges [K - 1, L] of the steps k >= 1."""
    return np.hypot(lm[None, :, 0] - gt[1:, None, 0], lm[None, :, 1] - gt[1:, None, 1])


def first_seen_and_det_max(gt, lm, c):
    """(first_seen [L] = k dt of the first step k >= 1 in range or -1, n_det_max, the smallest distance of any range from a limit)."""
    if len(lm) == 0:
        return np.zeros(0), 0, math.inf
    r = ranges(gt, lm)
    ok = (r >= c["rmin"]) & (r <= c["rmax"])
    fs = np.full(len(lm), -1.0)
    seen = ok.any(axis=0)
    fs[seen] = (np.argmax(ok, axis=0)[seen] + 1) * c["dt"]
    margin = float(min(np.abs(r - c["rmin"]).min(), np.abs(r - c["rmax"]).min()))
    return fs, int(ok.sum(axis=1).max()), margin


def generate(K, c, seed):
    """Everything of one filter from the restatement's own chain."""
    disp, info = displacements(K, c, seed)
    gt = trajectory(disp)
    lm = landmarks(gt, c, seed)
    fs, ndm, margin = first_seen_and_det_max(gt, lm, c)
    return dict(disp=disp, gt=gt, odom=odometry(disp, c, seed), landmarks=lm, first_seen=fs, n_det_max=ndm, margin=margin, segments=info,
                t=np.arange(K, dtype=np.float64) * c["dt"], pin=np.arange(K) <= c["n_pinned"])
