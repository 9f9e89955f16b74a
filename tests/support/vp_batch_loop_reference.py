"""The host-stop twin of a Victoria Park filter batch on the device route (include/rfsgpu.h [batch], csrc/vp_batch_loop.h): a second
VPFilterBatch, created and configured identically, that stays on the unchanged host-stop route.  Its resampling is decided here by the
rule the device states -- the squares added in slot order without a fused multiply-add, the draw restated by
device_loop_reference.resample_draw, engine.systematic_resample_plan -- and applied through rfsgpu_batch_resample_apply."""
import numpy as np

from tests.support import device_loop_reference as dl

CAP = 256


def make_batches(pkg, nF, nPer, params_of, count=2, n_landmarks=12, seed0=900):
    """count identical VPFilterBatch handles on the seeded scenes tests/test_vp_filter_batch.py uses (scenarios.make_vp_scenario,
    seed 900 + b), filter b under params_of(b).  Returns (scens, batches)."""
    sc = pkg.scenarios
    scens = [sc.make_vp_scenario(nPer, n_landmarks, 6, seed=seed0 + b, params=params_of(b)) for b in range(nF)]
    poses = np.concatenate([s["poses"] for s in scens], 0)
    out = []
    for _ in range(count):
        batch = pkg.VPFilterBatch(nF, nPer, gm_capacity=CAP)
        for b, scen in enumerate(scens):
            sc.apply_vp_batch_params(batch, b, scen["params"])
            for i in range(nPer):
                batch.import_gm(b * nPer + i, scen["w"][i], scen["mean"][i], scen["cov"][i])
        batch.set_laser_scan(scens[0]["scan"])
        batch.set_poses(poses, np.zeros((3, 3)))
        batch.set_weights(np.ones(nF * nPer))
        out.append(batch)
    return scens, out


class TwinTail:
    """RBPHDFilter::update's tail for every filter of the twin, by the restated rule.  gates: [(minUpdates, minMeasurements)] per filter;
    eff: [(eff_n, eff_n_percent)]; seeds: the filters' Philox keys."""

    def __init__(self, pkg, twin, gates, eff, seeds):
        self.pkg, self.twin, self.gates, self.eff, self.seeds = pkg, twin, gates, eff, seeds
        self.upd = np.zeros(twin.n_filters, dtype=np.int64)
        self.meas = np.zeros(twin.n_filters, dtype=np.int64)
        self.held = np.zeros(twin.n_filters, dtype=bool)      # the last call: a filter with measurements that a gate stopped

    def __call__(self, n_z, call):
        """Returns (fired [nF] bool, plan [N] global slots, n_eff [nF]: 0 where a filter stopped before the test)."""
        twin, nF, nP = self.twin, self.twin.n_filters, self.twin.n_per_filter
        w = twin.get_weights()
        fired = np.zeros(nF, dtype=bool)
        plan = np.arange(twin.n, dtype=np.int32)
        neff = np.zeros(nF)
        self.held[:] = False
        for b in range(nF):
            self.upd[b] += 1
            if n_z[b] == 0:
                continue
            self.meas[b] += int(n_z[b])
            if self.upd[b] < self.gates[b][0] or self.meas[b] < self.gates[b][1]:
                self.held[b] = True
                continue
            wb = w[b * nP:(b + 1) * nP]
            ss = 0.0
            for v in wb.tolist():      # sequential, each square rounded before it is added
                ss = ss + v * v
            neff[b] = 1.0 / ss
            if neff[b] > self.eff[b][0] and neff[b] / nP > self.eff[b][1]:
                continue
            plan[b * nP:(b + 1) * nP] = b * nP + self.pkg.engine.systematic_resample_plan(wb, dl.resample_draw(self.seeds[b], call))
            fired[b] = True
            self.upd[b] = self.meas[b] = 0
        if fired.any():
            twin.batch_resample_apply(plan, fired)
        return fired, plan, neff


def state(batch, lists=True, mixtures=True):
    """Everything the tests compare, read back (synchronising)."""
    batch.synchronize()
    ids, par = batch.get_particle_ids()
    s = dict(w=batch.get_weights(), sizes=batch.gm_sizes(), masks=batch.get_unused_masks(), ids=ids, par=par, occured=batch.batch_resample_occured(),
             poses=batch.get_poses())
    if mixtures:
        s["gm"] = [batch.export_gm(i) for i in range(batch.n)]
    if lists:
        s["cands"] = [batch.export_birth_candidates(i) for i in range(batch.n)]
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_state(a, b, what):
    for k in ("sizes", "masks", "ids", "par", "occured"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    for k in ("w", "poses"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}")
    for k in ("gm", "cands"):
        if k in a and k in b:
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                for p, q in zip(x, y):
                    np.testing.assert_array_equal(p, q, err_msg=f"{what}: {k} of slot {i}")
