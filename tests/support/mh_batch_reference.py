"""Helpers of tests/test_mh_fastslam_batch.py: a batch of multi-hypothesis FastSLAM filters (pkg.MHFastSLAMBatch) next to its
yardstick -- one FastSLAM handle per filter on rfsgpu_fastslam_cycle_async, created with max_particles = max_per_filter and given the
same state, measurements, poses and draws -- and the comparison of a filter's block with its handle."""
import numpy as np

from tests.support import mh_device_cycle_reference as ref

NEVER = 1000          # minUpdatesBeforeResample that no test reaches


def copy_struct(c):
    return type(c).from_buffer_copy(c)


def handle(pkg, n, stride, gm_capacity=64):
    """pkg.FastSLAM on the device cycle whose handle has exactly `stride` particle slots."""
    return pkg.FastSLAM(n, gm_capacity=gm_capacity, device_cycle=True, max_particles=stride)


class Rig:
    """The batch and its handles.  scens[b], hyps[b], diffs[b]: filter b's scene (ref.crowded / sparse / windowed / mixed), its
    maxNDataAssocHypotheses and its likelihood window."""

    def __init__(self, pkg, sc, scens, hyps, diffs, n_per, stride, gm_capacity=64):
        self.pkg, self.sc, self.nF, self.n_per, self.stride = pkg, sc, len(scens), n_per, stride
        self.batch = pkg.MHFastSLAMBatch(self.nF, n_per, stride, gm_capacity=gm_capacity)
        self.handles = [handle(pkg, n_per, stride, gm_capacity) for _ in scens]
        self.scens = scens
        x = np.zeros((self.nF * stride, 3))
        for b, (scen, h) in enumerate(zip(scens, self.handles)):
            assert scen["n"] == n_per
            ref.load(h, sc, scen, hyps[b], diffs[b])
            P = scen["params"]
            self.batch.configure(b, None, R=P["R"], Pd=P["Pd"], clutter=P["clutter"], rmax=P["rmax"], rmin=P["rmin"], rbuf=P["rbuf"],
                                 kf=(P["kf_range"], P["kf_bearing"]), Q=P["Q_lm"])
            x[b * stride:b * stride + n_per] = scen["poses"]
            for i in range(n_per):
                self.batch.import_gm(b * stride + i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
        assert all(np.array_equal(s["pose_cov"], scens[0]["pose_cov"]) for s in scens)
        self.batch.set_poses(x, scens[0]["pose_cov"])
        self.batch.set_weights(np.ones(self.nF * stride))
        self.push_configs()

    @classmethod
    def of(cls, pkg, sc, batch, handles, n_per, stride, scens=None):
        """A rig around a batch and handles that the caller has configured and loaded."""
        r = cls.__new__(cls)
        r.pkg, r.sc, r.nF, r.n_per, r.stride, r.batch, r.handles, r.scens = pkg, sc, len(handles), n_per, stride, batch, list(handles), scens
        return r

    def each_config(self, fn):
        """fn(b, fs_config) on every handle's FastSlamConfig, then the batch gets copies."""
        for b, h in enumerate(self.handles):
            fn(b, h.fs_config)
        self.push_configs()

    def push_configs(self):
        for b, h in enumerate(self.handles):
            h.set_fastslam_config(h.fs_config)
            self.batch.configure_fastslam(b, copy_struct(h.fs_config))

    def set_resampling(self, b, eff_n, eff_n_percent):
        self.handles[b].effNParticles_t, self.handles[b].effNParticles_t_percent = eff_n, eff_n_percent
        self.batch.set_resampling(b, eff_n, eff_n_percent)

    def cycle(self, Zs, u01, predict=True, handles=True):
        self.batch.cycle_async(predict, Zs, u01)
        if handles:
            for h, Z, u in zip(self.handles, Zs, u01):
                h.cycle_async(Z, u, predict=predict)

    def block_state(self, b, n=None):
        """ref.state of filter b's live slots."""
        B, s = self.batch, self.stride
        n = int(B.live_counts()[b]) if n is None else n
        blk = B.block(b, n)
        return dict(n=n, w=B.get_weights()[blk].copy(), poses=B.get_poses()[blk].copy(), sizes=np.asarray(B.gm_sizes())[blk].copy(),
                    fov=np.array([B.landmarks_in_fov(b * s + i) for i in range(n)]), unused=np.asarray(B.get_unused_masks())[blk].copy(),
                    maps=[tuple(np.array(x) for x in B.export_gm(b * s + i)) for i in range(n)])

    def compare(self, lc=None, maps=True, only=None):
        """Every filter against its handle: counts, decisions, parents, plans, ids and N_eff; the state bit for bit (normalised
        weights to 1e-12 relative).  Returns the batch's last_cycle."""
        B = self.batch
        lc = B.last_cycle() if lc is None else lc
        counts = B.live_counts()
        ids, pids = B.get_particle_ids()
        occ = B.batch_resample_occured()
        for b, h in enumerate(self.handles):
            if only is not None and b not in only:
                continue
            hl = h.fastslam_last_cycle()
            what = "filter %d" % b
            assert counts[b] == h.n == lc["n_after_resample"][b] == hl["n_after_resample"], what
            assert lc["n_after_update"][b] == hl["n_after_update"], what
            assert bool(lc["fired"][b]) == hl["fired"] and not lc["overflowed"][b], what
            assert np.array_equal(lc["parent"][b, :hl["n_after_update"]], hl["parent"]) and (lc["parent"][b, hl["n_after_update"]:] == -1).all(), what
            assert np.array_equal(lc["plan"][b, :h.n], hl["plan"]) and (lc["plan"][b, h.n:] == -1).all(), what
            if hl["n_eff"] == 0.0:
                assert lc["n_eff"][b] == 0.0, what
            else:
                assert abs(lc["n_eff"][b] / hl["n_eff"] - 1) <= 1e-12, what
            hi, hp = h.get_particle_ids()
            assert np.array_equal(ids[B.block(b, h.n)], hi) and np.array_equal(pids[B.block(b, h.n)], hp), what
            # (resampleOccured_ of the handle's device route is what its last cycle with measurements left)
            if maps:
                a, c = ref.state(h), self.block_state(b, h.n)
                np.testing.assert_allclose(c["w"], a["w"], rtol=1e-12, atol=0, err_msg=what)
                ref.assert_same_state(a, c, weights=1e-12)
        return lc, occ

    def snapshot(self):
        """What a probe needs of every handle before a cycle: poses, weights and ordered maps."""
        return [dict(n=h.n, poses=h.get_poses().copy(), w=h.get_weights().copy(), maps=[h.export_gm(i) for i in range(h.n)],
                     pose_cov=(self.scens[b]["pose_cov"] if self.scens else np.zeros((3, 3)))) for b, h in enumerate(self.handles)]

    def assert_margins(self, snap, Zs, u01, configure, predict=True):
        """After a cycle, on the handles alone: N_eff is at least 1e-6 (relative) from both thresholds wherever the test ran, and where
        a resampling fired every sample point is at least 1e-9 from every cumulative sum of the normalised weights it was taken on --
        those of a probe handle that starts from the snapshot and runs the same update with its gates shut (the same kernels on the
        same inputs).  configure(b, probe): the model of filter b.  -> (decisions checked, plans checked)"""
        nd = npl = 0
        for b, h in enumerate(self.handles):
            hl = h.fastslam_last_cycle()
            if hl["n_eff"] != 0.0:
                nd += 1
                for t, v in ((h.effNParticles_t, hl["n_eff"]), (h.effNParticles_t_percent, hl["n_eff"] / hl["n_after_update"])):
                    assert t == 0.0 or abs(v / t - 1) >= 1e-6, "filter %d: N_eff %r at its threshold %r" % (b, v, t)
            if not hl["fired"]:
                continue
            s = snap[b]
            p = handle(self.pkg, s["n"], self.stride)
            configure(b, p)
            p.config = p.get_filter_config()
            p.fs_config = copy_struct(h.fs_config)
            p.fs_config.minUpdatesBeforeResample = NEVER
            p.fs_config.nParticlesMax = self.stride
            p.set_poses(s["poses"], s["pose_cov"])
            p.set_weights(s["w"])
            for i, m in enumerate(s["maps"]):
                if m[0].size:
                    p.import_gm(i, m[0], m[2], m[3])
            p.cycle_async(Zs[b], 0.5, predict=predict)
            w = p.get_weights().copy()
            p.close()
            assert w.size == hl["n_after_update"], "filter %d: the probe grew to %d, the handle to %d" % (b, w.size, hl["n_after_update"])
            near, _ = ref.resample_margins(w, u01[b], hl["n_after_resample"])
            assert near >= 1e-9, "filter %d: a sample point %.3g from a cumulative sum" % (b, near)
            npl += 1
        return nd, npl

    def close(self):
        self.batch.close()
        for h in self.handles:
            h.close()


def probe_weights(pkg, sc, scen, hyp, diff, stride, Z, predict=True):
    """The normalised weights a handle holds after this update when nothing resamples -- what its resampling decision is taken on --
    and the grown state (ref.state) a resampling copies from."""
    h = handle(pkg, scen["n"], stride)
    ref.load(h, sc, scen, hyp, diff)
    h.fs_config.minUpdatesBeforeResample = NEVER
    h.fs_config.nParticlesMax = stride
    h.cycle_async(Z, 0.5, predict=predict)
    w = h.get_weights().copy()
    st = ref.state(h)
    h.close()
    return w, st
