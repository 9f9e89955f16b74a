"""The pose / pose covariance protocol of the three batch cycles, walked through every transition: poses without a covariance (the
shared all-zero form, written once), with one shared [9] covariance, with one covariance per particle [N][9], without a covariance
again, and no poses at all.  After every cycle each filter's poses, pose covariances, weights and mixtures equal, bit for bit, those of
a plain handle fed the same sequence."""
import numpy as np
import pytest

from tests.support import mh_batch_reference as mb

N_F, N_PER, MH_STRIDE, CAP, N_Z = 2, 4, 8, 64, 3
FORMS = ["none", "shared", "each", "none", "no poses"]       # what each of the five cycles passes
EMPTY = (2, 1)                                               # (cycle, filter): that filter has no measurements in that cycle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _spd(rng, n):
    A = rng.normal(0, 1e-2, (n, 3, 3))
    return A @ np.swapaxes(A, 1, 2) + np.diag([1e-4, 1e-4, 1e-5])


def _inputs(scens, slots):
    """Per cycle: poses [N_F][slots][3] or None, the covariance argument of the batch (None | [9] | [N_F * slots][9]), measurement sets."""
    rng = np.random.default_rng(20)
    out = []
    for k, form in enumerate(FORMS):
        x = None if form == "no poses" else np.stack([np.resize(s["poses"], (slots, 3)) + rng.normal(0, 1e-3, (slots, 3)) for s in scens])
        cov = {"shared": _spd(rng, 1).reshape(9), "each": _spd(rng, N_F * slots).reshape(N_F * slots, 9)}.get(form)
        Zs = [s["Z"][:N_Z] + rng.normal(0, 2e-3, (N_Z, 2)) for s in scens]
        Zs[EMPTY[1]] = Zs[EMPTY[1]][:0] if k == EMPTY[0] else Zs[EMPTY[1]]
        out.append((x, cov, Zs))
    return out


def _cov_of(cov, b, slots, n):
    """Filter b's share of the batch's covariance argument, for a handle of n particles."""
    return cov if cov is None or cov.ndim == 1 else cov[b * slots:b * slots + n]


def _compare(batch, handles, slots, what):
    xb, cb, wb = batch.get_poses(), batch.get_pose_covs(), batch.get_weights()
    for b, h in enumerate(handles):
        n = h.n
        blk = slice(b * slots, b * slots + n)
        w = h.get_weights()
        print("%s filter %d: %d particles, weights differ by at most %.3g (relative)" % (what, b, n, float(np.max(np.abs(wb[blk] / w - 1)))))
        _same(xb[blk], h.get_poses(), "%s filter %d: poses" % (what, b))
        _same(cb[blk], h.get_pose_covs(), "%s filter %d: pose covariances" % (what, b))
        _same(wb[blk], w, "%s filter %d: weights" % (what, b))
        for i in range(n):
            for x, y in zip(batch.export_gm(b * slots + i), h.export_gm(i)):
                _same(x, y, "%s filter %d particle %d: mixture" % (what, b, i))


def _rbphd(pkg, sc, scens):
    from test_filter_batch import _configure_from_scenario
    batch = pkg.FilterBatch(N_F, N_PER, gm_capacity=CAP)
    handles = [pkg.RBPHDFilter(N_PER, gm_capacity=CAP) for _ in scens]
    batch.set_poses(np.vstack([s["poses"] for s in scens]), scens[0]["pose_cov"])
    batch.set_weights(np.concatenate([s["particle_w"] for s in scens]))
    for b, (s, h) in enumerate(zip(scens, handles)):
        _configure_from_scenario(pkg.capi, batch, b, s["params"])
        sc.load_scenario(h, s)
        for i in range(N_PER):
            batch.import_gm(b * N_PER + i, s["w"][i], s["mean"][i], s["cov"][i])

    def cycle(x, cov, Zs):
        batch.cycle_async(True, Zs, poses=None if x is None else x.reshape(-1, 3), pose_cov=cov, normalize=False)
        for b, h in enumerate(handles):
            h.cycle_async(True, Zs[b], poses=None if x is None else x[b], pose_cov=_cov_of(cov, b, N_PER, N_PER), normalize=False)
    return batch, handles, N_PER, cycle


def _fastslam(pkg, sc, scens):
    from test_filter_batch import _configure_from_scenario
    batch = pkg.FastSLAMBatch(N_F, N_PER, gm_capacity=CAP)
    handles = [pkg.FastSLAM(N_PER, gm_capacity=CAP) for _ in scens]
    batch.set_poses(np.vstack([s["poses"] for s in scens]), scens[0]["pose_cov"])
    batch.set_weights(np.concatenate([s["particle_w"] for s in scens]))
    for b, (s, h) in enumerate(zip(scens, handles)):
        _configure_from_scenario(pkg.capi, batch, b, s["params"])
        batch.configure_fastslam(b, batch.default_fastslam_config())
        sc.load_scenario(h, s)
        h.set_fastslam_config(h.default_fastslam_config())
        for i in range(N_PER):
            logodds = np.log(s["w"][i] / (1 - s["w"][i] * 0.5))
            batch.import_gm(b * N_PER + i, logodds, s["mean"][i], s["cov"][i])
            h.import_gm(i, logodds, s["mean"][i], s["cov"][i])

    def cycle(x, cov, Zs):
        batch.cycle_async(True, Zs, poses=None if x is None else x.reshape(-1, 3), pose_cov=cov, normalize=False)
        for b, h in enumerate(handles):      # (FastSLAM::predict's map part, then FastSLAM::update, as Sim2dBatchRun steps a handle)
            if x is not None:
                h.set_poses(x[b], _cov_of(cov, b, N_PER, N_PER))
            h.predict_map(False)
            if len(Zs[b]):
                h.fastslam_update(Zs[b])
    return batch, handles, N_PER, cycle


def _mh(pkg, sc, scens):
    rig = mb.Rig(pkg, sc, scens, [1] * N_F, [3.0] * N_F, N_PER, MH_STRIDE, gm_capacity=CAP)
    u01 = np.array([0.37, 0.81])

    def cycle(x, cov, Zs):
        rig.batch.cycle_async(True, Zs, u01, poses=None if x is None else x.reshape(-1, 3), pose_cov=cov)
        for b, h in enumerate(rig.handles):
            if x is not None:
                h.set_poses(x[b, :h.n], _cov_of(cov, b, MH_STRIDE, h.n))
            h.cycle_async(Zs[b], u01[b], predict=True)
    return rig.batch, rig.handles, MH_STRIDE, cycle


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rbphd", "fastslam", "mh"])
def test_every_covariance_form_in_turn_equals_plain_handles(pkg, sc, kind):
    scens = [sc.make_scenario(N_PER, 6, N_Z, seed=881 + b) for b in range(N_F)]
    assert all(np.array_equal(s["pose_cov"], scens[0]["pose_cov"]) for s in scens)
    batch, handles, slots, cycle = {"rbphd": _rbphd, "fastslam": _fastslam, "mh": _mh}[kind](pkg, sc, scens)
    _compare(batch, handles, slots, "%s, as loaded:" % kind)
    for k, (x, cov, Zs) in enumerate(_inputs(scens, slots)):
        assert [len(Z) for Z in Zs] == [0 if (k, b) == EMPTY else N_Z for b in range(N_F)]
        cycle(x, cov, Zs)
        _compare(batch, handles, slots, "%s, cycle %d (%s):" % (kind, k, FORMS[k]))
    batch.close()
    for h in handles:
        h.close()
