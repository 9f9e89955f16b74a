"""The measurement index of the map update's gate prefilter (csrc/update_map.h), restated in numpy fp32.

The device bins the measurement set once per particle -- 256 bearing bins over [-pi, pi), 64 range bins between the set's smallest
and largest range -- and finds a landmark's candidates as the measurements whose bins fall inside the landmark's bearing window
(+- one guard bin, across the +-pi seam as the union of the two end pieces) and range window.  This module states the bin rule, the
window rule and the conditions under which the device uses the index at all; the tests hold the candidate sets it gives against
the exact gates.  (The device contracts a few multiply-adds; a candidate set can differ from this one by a measurement that sits
within an fp32 rounding of a bin edge.  The claim under test is the rule's: no accepted pair outside the windows.)"""
import numpy as np

F = np.float32
B_BINS, R_BINS = 256, 64
PI_F = F(np.pi)
TWO_PI_F = F(2 * np.pi)
INV_2PI_F = F(1 / (2 * np.pi))
B_SCALE = F(B_BINS / (2 * np.pi))
THRB_MAX = F(3.0)


def bearing_coord(b):
    return (F(b) + PI_F) * B_SCALE


def bearing_bins(zb):
    zb = np.asarray(zb, dtype=F)
    red = zb - np.rint(zb * INV_2PI_F) * TWO_PI_F
    return np.nan_to_num(np.clip(np.floor(bearing_coord(red)), 0, B_BINS - 1), nan=0.0).astype(int)      # (a NaN: bin 0, and a candidate of every landmark)


def range_bin(r, r_min, scale):
    return np.nan_to_num(np.clip(np.floor((np.asarray(r, dtype=F) - r_min) * scale), 0, R_BINS - 1), nan=0.0).astype(int)


def thresholds(kf_range, kf_bearing, zr_max, zb_max, zx0):
    """thrB, thrR of the sweep (fp32)."""
    thr_b = F(kf_bearing) * (F(1) + F(1e-6)) + F(1e-6) * (F(zb_max) + F(3.2)) + F(1e-6)
    thr_r = F(kf_range) * (F(1) + F(1e-6)) + F(2.5e-7) * (F(zr_max) + abs(F(zx0))) + F(1e-30)
    return thr_b, thr_r


def usable(kf_range, kf_bearing, Z):
    """Whether the device looks this set up in its index (otherwise it sweeps)."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 2)
    if len(Z) == 0 or not (kf_range > 0 and kf_bearing > 0):
        return False
    with np.errstate(all="ignore"):
        zr, zb = Z[:, 0].astype(F), Z[:, 1].astype(F)
        zr_max, zb_max = np.fmax.reduce(np.abs(zr)), np.fmax.reduce(np.abs(zb))
        thr_b, _ = thresholds(kf_range, kf_bearing, zr_max, zb_max, 0.0)
        span = np.fmax.reduce(zr) - np.fmin.reduce(zr)
        return bool(zb_max < 50 and zr_max < 1e30 and thr_b < THRB_MAX and np.isfinite(F(kf_range) * (F(1) + F(1e-6)))
                    and span > 0 and np.isfinite(F(R_BINS) / span))


def candidates(kf_range, kf_bearing, Z, zx0, zx1):
    """The measurements the index hands to the exact gates for a landmark with expected measurement (zx0, zx1)."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 2)
    zr, zb = Z[:, 0].astype(F), Z[:, 1].astype(F)
    always = np.isnan(zr) | np.isnan(zb)
    zr_max, zb_max = np.fmax.reduce(np.abs(zr)), np.fmax.reduce(np.abs(zb))
    r_min, r_max = np.fmin.reduce(zr), np.fmax.reduce(zr)
    scale = F(R_BINS) / (r_max - r_min)
    bb, rb = bearing_bins(zb), range_bin(zr, r_min, scale)
    x0, x1 = F(zx0), F(zx1)
    if not (np.isfinite(x0) and np.isfinite(x1)):
        return set(range(len(Z)))
    thr_b, thr_r = thresholds(kf_range, kf_bearing, zr_max, zb_max, x0)
    ilo = int(np.floor(bearing_coord(x1 - thr_b))) - 1
    ihi = int(np.floor(bearing_coord(x1 + thr_b))) + 1
    assert ihi - ilo < B_BINS - 1
    in_b = np.isin(bb, [k % B_BINS for k in range(ilo, ihi + 1)])
    guard = F(2.5e-7) * (zr_max + abs(x0))
    lo, hi = x0 - thr_r - guard, x0 + thr_r + guard
    in_r = (rb >= range_bin(lo, r_min, scale)) & (rb <= range_bin(hi, r_min, scale))
    if hi < r_min or lo > r_max:
        in_r[:] = False
    return set(np.nonzero((in_b & in_r) | always)[0].tolist())
