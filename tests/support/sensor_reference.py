"""numpy restatement of a batch's device sensor (csrc/batch_sensor.h, include/rfsgpu.h [sensor]): one filter's scan of one call --
generateMeasurements of the reference's 2-D simulator (src/rbphdslam2dSim.cpp:283-366) for one time step -- on the Philox restatement
of tests/support/device_loop_reference.py.  Counter layout: (index, block | attempt << 8, call lo, call hi) under the sensor's key;
block 3 the detection noise of landmark `index`, 4 its detection draw, 5 the clutter count (index 0), 6 attempt `attempt` of clutter
point `index`'s range, 7 its bearing."""
import math

import numpy as np

from tests.support import device_loop_reference as dl

U64 = np.uint64
MASK = dl.MASK
MAX_Z = 64
CMF_LEN = 100
MAX_REDRAWS = 64
BLOCK_NOISE, BLOCK_DETECT, BLOCK_COUNT, BLOCK_RANGE, BLOCK_BEARING = 3, 4, 5, 6, 7


def _blocks(index, block, seed, call):
    i = np.atleast_1d(np.asarray(index)).astype(U64)
    z = np.zeros(i.shape, dtype=U64)
    return dl.philox4x32_10([i, z + U64(block), z + U64(call & MASK), z + U64(call >> 32)], (seed & MASK, seed >> 32))


def u01_half_open(a, b):
    """batch_sensor.h sensor_u01: 53 bits -> [0, 1)."""
    m = ((a << U64(32)) | b) >> U64(11)
    return m.astype(np.float64) * (1.0 / 9007199254740992.0)


def mean_clutter(clutter, rmin, rmax):
    """MeasurementModel_RngBrg::clutterIntensityIntegral: intensity * (2 pi (rmax - rmin))."""
    return clutter * (2 * math.pi * (rmax - rmin))


def poisson_cmf(mean):
    """The table of src/rbphdslam2dSim.cpp:294-306, in its order of operations."""
    e = math.exp(-mean)
    cmf = [e]
    p, fact = 1.0, 1.0
    for i in range(1, CMF_LEN):
        p *= mean
        fact *= i
        cmf.append(cmf[i - 1] + p / fact * e)
    return np.array(cmf)


def clutter_count(u, cmf):
    """The first n with u <= cmf[n]; 99 where no n < 99 does (the reference walks off its table there)."""
    n = 0
    while n < CMF_LEN - 1 and u > cmf[n]:
        n += 1
    return n


def cholesky_lower(R):
    R = np.asarray(R, dtype=np.float64).reshape(2, 2)
    l00 = math.sqrt(R[0, 0])
    l10 = R[1, 0] / l00
    return l00, l10, math.sqrt(R[1, 1] - l10 * l10)


def scan_counts(pose, landmarks, R, Pd, clutter, rmin, rmax, seed, calls):
    """(n_det [len(calls)], n_clutter [len(calls)]) of scan() before any cut, for many calls at once: the same draws and decisions,
    with the call number as the array axis (for statistics over many scans)."""
    calls = np.asarray(calls, dtype=U64)
    lo, hi = calls & U64(MASK), calls >> U64(32)
    key = (seed & MASK, seed >> 32)

    def blocks(index, block):
        z = np.zeros(calls.shape, dtype=U64)
        return dl.philox4x32_10([z + U64(index), z + U64(block), lo, hi], key)

    lm = np.asarray(landmarks, dtype=np.float64).reshape(-1, 2)
    L = cholesky_lower(R)
    x, y, _ = (float(v) for v in pose)
    n_det = np.zeros(calls.shape, dtype=np.int64)
    for m in range(len(lm)):
        dx, dy = lm[m, 0] - x, lm[m, 1] - y
        rng_true = math.sqrt(dx * dx + dy * dy)
        if rng_true > rmax or rng_true < rmin:
            continue
        r = blocks(m, BLOCK_NOISE)
        rad, ang = np.sqrt(-2.0 * np.log(dl.u01_open_low(r[0], r[1]))), 2.0 * np.pi * dl.u01_open_low(r[2], r[3])
        zr = rng_true + L[0] * (rad * np.cos(ang))
        r = blocks(m, BLOCK_DETECT)
        n_det += (zr <= rmax) & (zr >= rmin) & (u01_half_open(r[0], r[1]) <= Pd)
    r = blocks(0, BLOCK_COUNT)
    cmf = poisson_cmf(mean_clutter(clutter, rmin, rmax))
    n_clutter = np.searchsorted(cmf[: CMF_LEN - 1], u01_half_open(r[0], r[1]), side="left")      # the first n with u <= cmf[n], else 99
    return n_det, n_clutter


def scan(pose, landmarks, R, Pd, clutter, rmin, rmax, seed, call, max_nz=MAX_Z):
    """(Z [n, 2], info): the set as the device delivers it (cut to max_nz: detections in landmark order, then clutter) and what the
    decisions hung on -- info["ranges"]: every true range and every noisy range that was compared with the limits; info["n_det"],
    info["n_clutter"] before the cut; info["cut"]."""
    lm = np.asarray(landmarks, dtype=np.float64).reshape(-1, 2)
    L = cholesky_lower(R)
    x, y, th = (float(v) for v in pose)
    det = []
    ranges = []
    if len(lm):
        dx, dy = lm[:, 0] - x, lm[:, 1] - y
        rng_true = np.sqrt(dx * dx + dy * dy)
        bearing = np.arctan2(dy, dx) - th
        for _ in range(16):
            bearing = np.where(bearing > np.pi, bearing - 2 * np.pi, bearing)
        for _ in range(16):
            bearing = np.where(bearing < -np.pi, bearing + 2 * np.pi, bearing)
        idx = np.arange(len(lm))
        r = _blocks(idx, BLOCK_NOISE, seed, call)
        rad, ang = np.sqrt(-2.0 * np.log(dl.u01_open_low(r[0], r[1]))), 2.0 * np.pi * dl.u01_open_low(r[2], r[3])
        g0, g1 = rad * np.cos(ang), rad * np.sin(ang)
        zr = rng_true + L[0] * g0
        zb = bearing + (L[1] * g0 + L[2] * g1)
        r = _blocks(idx, BLOCK_DETECT, seed, call)
        v = u01_half_open(r[0], r[1])
        ok = ~((rng_true > rmax) | (rng_true < rmin))
        keep = ok & (zr <= rmax) & (zr >= rmin) & (v <= Pd)
        ranges += list(rng_true) + list(zr[ok])
        det = [[zr[m], zb[m]] for m in idx[keep]]
    r = _blocks([0], BLOCK_COUNT, seed, call)
    n_c = clutter_count(float(u01_half_open(r[0], r[1])[0]), poisson_cmf(mean_clutter(clutter, rmin, rmax)))
    clut = []
    for j in range(n_c):
        u = cr = 0.0
        ok = False
        for a in range(MAX_REDRAWS):
            r = _blocks([j], BLOCK_RANGE | (a << 8), seed, call)
            u = float(u01_half_open(r[0], r[1])[0])
            cr = u * rmax                  # (one exact product on either side: no margin needed)
            if not cr < rmin:
                ok = True
                break
        if not ok:
            cr = rmin + u * (rmax - rmin)
        r = _blocks([j], BLOCK_BEARING, seed, call)
        clut.append([cr, float(u01_half_open(r[0], r[1])[0]) * 2 * np.pi - np.pi])
    Z = np.array(det + clut, dtype=np.float64).reshape(-1, 2)
    info = dict(ranges=np.array(ranges, dtype=np.float64), n_det=len(det), n_clutter=n_c, cut=len(Z) > max_nz)
    return Z[:max_nz], info
