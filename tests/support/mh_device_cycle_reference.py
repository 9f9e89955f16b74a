"""Helpers of tests/test_mh_fastslam_device_cycle.py: the copy plan of a multi-hypothesis FastSLAM update in its two forms (the
host loop of fastslam_update_mh, reference include/FastSLAM.hpp:543-556, and the scan form fs_mh_plan_kernel uses), the margins
of a systematic resampling decision, and the scenarios that force a given number of hypotheses per particle."""
import numpy as np


def host_loop_plan(nH):
    """The arrays the host loop of fastslam_update_mh builds from the hypothesis counts: the running particle count grows by
    nH - 1 after every multiplied particle, whose copies are then addressed as count - h.
    -> (n, slotSrc, slotHyp, slotNH, copyDst, copySrc)"""
    nH = [int(v) for v in nH]
    N0 = len(nH)
    src, hyp, cnt = list(range(N0)), [0 if v > 0 else -1 for v in nH], list(nH)
    dst, csrc = [], []
    n = N0
    for i in range(N0):
        if nH[i] <= 1:
            continue
        n += nH[i] - 1
        src += [0] * (nH[i] - 1); hyp += [0] * (nH[i] - 1); cnt += [0] * (nH[i] - 1)
        for h in range(1, nH[i]):
            slot = n - h
            src[slot], hyp[slot], cnt[slot] = i, h, nH[i]
            dst.append(slot); csrc.append(i)
    a = lambda v: np.asarray(v, dtype=np.int32)
    return n, a(src), a(hyp), a(cnt), a(dst), a(csrc)


def scan_plan(nH):
    """The same arrays from an exclusive scan of max(nH - 1, 0): particle i's copies occupy [first_i, first_i + nH_i - 1) with
    first_i = N0 + scan_i, hypothesis h in first_i + (nH_i - 1) - h; copy number scan_i + h - 1 is (that slot, i)."""
    nH = np.asarray(nH, dtype=np.int64)
    N0 = nH.size
    extra = np.maximum(nH - 1, 0)
    scan = np.concatenate([[0], np.cumsum(extra)[:-1]]) if N0 else np.zeros(0, np.int64)
    n = N0 + int(extra.sum())
    src, hyp, cnt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    src[:N0] = np.arange(N0); hyp[:N0] = np.where(nH > 0, 0, -1); cnt[:N0] = nH
    dst, csrc = np.zeros(n - N0, np.int32), np.zeros(n - N0, np.int32)
    i = np.repeat(np.arange(N0), extra)                     # the particle of every copy, in particle order
    h = np.arange(n - N0) - scan[i] + 1                     # its hypothesis 1 ... nH - 1
    slot = N0 + scan[i] + (nH[i] - 1) - h
    src[slot], hyp[slot], cnt[slot] = i, h, nH[i]
    dst[scan[i] + h - 1], csrc[scan[i] + h - 1] = slot, i
    return n, src, hyp, cnt, dst, csrc


def resample_margins(w, u01, n_out):
    """For normalised weights w and a systematic plan of n_out samples from draw u01: the smallest distance of a sample point from
    a cumulative sum (a decision of the search flips only if the two cross), and N_eff."""
    w = np.asarray(w, dtype=np.float64)
    cum = np.cumsum(w)
    step = np.full(n_out, 1.0 / n_out)
    step[0] = u01 / n_out
    sp = np.cumsum(step)
    k = np.searchsorted(cum, sp)
    near = np.minimum(np.abs(cum[np.minimum(k, w.size - 1)] - sp), np.abs(cum[np.maximum(k - 1, 0)] - sp))
    return float(near.min()), 1.0 / float(np.sum(w * w))


def crowded(sc, n0, seed=112):
    """n0 particles, 12 landmarks in range and 8 measurements (the lm12_z8 shape of tests/test_mh_fastslam_edges.py): with a wide
    likelihood window every particle keeps as many hypotheses as it is allowed, up to 16."""
    return sc.make_scenario(n0, 12, 8, seed=seed)


def sparse(sc, n0, seed=201):
    """Few landmarks over a 25 m disc, each detected once, no clutter: CostMatrix::reduce fixes every row, one hypothesis per
    particle whatever the limit."""
    return sc.make_scenario(n0, 8, 8, seed=seed, n_clutter=0, rmax=25.0)


def windowed(sc, n0, seed=6):
    """Nine landmarks within 3 m, eight detections, no clutter, for a likelihood window of 1 and a limit of 4: at 65 particles
    some keep one hypothesis and the others two (checked on the oracle: 9 and 56)."""
    return sc.make_scenario(n0, 9, 8, seed=seed, n_clutter=0, rmax=3.0)


def mixed(sc, n0, seed=2):
    """The same shape with one clutter measurement, for a window of 8 and a limit of 16: at 65 particles 2, 4 or 6 hypotheses per
    particle (checked on the oracle: 48, 15 and 2 particles)."""
    return sc.make_scenario(n0, 9, 8, seed=seed, n_clutter=1, rmax=3.0)


def load(f, sc, scen, hyp, diff):
    """The scenario into a pkg.FastSLAM object (maps with zero log-odds, as the edge tests load them) with no landmark candidate
    lists (landmarkCandidateMeasurementCountThreshold = 1, the constructor default)."""
    sc.load_scenario(f, scen)
    for i in range(scen["n"]):
        f.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
    f.config = f.get_filter_config()
    f.fs_config.maxNDataAssocHypotheses = hyp
    f.fs_config.maxDataAssocLogLikelihoodDiff = diff
    f.set_fastslam_config(f.fs_config)


def state(f):
    """Everything a cycle leaves behind that the C ABI shows: count, weights, poses, per-particle sizes, FOV counts, unused masks,
    ordered mixtures."""
    n = f.n
    return dict(n=n, w=f.get_weights().copy(), poses=f.get_poses().copy(), sizes=np.asarray(f.gm_sizes()).copy(),
                fov=np.array([f.landmarks_in_fov(i) for i in range(n)]), unused=np.asarray(f.get_unused_masks()).copy(),
                maps=[tuple(np.array(x) for x in f.export_gm(i)) for i in range(n)])


def assert_same_state(a, b, weights="equal"):
    """Bit-equal states; weights: "equal", or a relative tolerance."""
    assert a["n"] == b["n"]
    for k in ("poses", "sizes", "fov", "unused"):
        assert np.array_equal(a[k], b[k]), k
    if weights == "equal":
        assert np.array_equal(a["w"], b["w"])
    else:
        np.testing.assert_allclose(a["w"], b["w"], rtol=weights, atol=0)
    for i, (ma, mb) in enumerate(zip(a["maps"], b["maps"])):
        for x, y in zip(ma, mb):
            assert np.array_equal(x, y), "mixture of particle %d" % i
