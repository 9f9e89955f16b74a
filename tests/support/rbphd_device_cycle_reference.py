"""Helpers of tests/test_rbphd_device_cycle.py: the host-stop route of one RBPHDFilter::update (the yardstick of
rfsgpu_rbphd_cycle_async), the inheritance-level rule of predict_launch restated in numpy, pairs of handles with the same state,
and the state that is compared between them."""
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def walk_levels_constant():
    """RFSGPU_RBPHD_WALK_LEVELS as include/rfsgpu.h defines it."""
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    return int(re.search(r"#define\s+RFSGPU_RBPHD_WALK_LEVELS\s+(\d+)", txt).group(1))


def declared_args(name):
    """The argument list of `name` in include/rfsgpu.h, white space squeezed."""
    txt = open(os.path.join(ROOT, "include", "rfsgpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    return None if m is None else re.sub(r"\s+", " ", m.group(1)).strip()


# ---- the levels rule -----------------------------------------------------------------------------------------------------------
def levels_loop(ppid, n=None):
    """predict_launch's loop: parent[i] = ppid[i] (i itself where that is no slot), level[i] = 0 where parent >= i, else
    level[parent] + 1.  Returns (parent, level, any, max_level)."""
    n = len(ppid) if n is None else n
    parent, level = [0] * n, [0] * n
    any_, mx = False, 0
    for i in range(n):
        p = int(ppid[i])
        if p < 0 or p >= n:
            p = i
        parent[i] = p
        level[i] = 0 if p >= i else level[p] + 1
        any_ |= p != i
        mx = max(mx, level[i])
    return np.array(parent), np.array(level), any_, mx


def levels_chase(ppid, n=None):
    """The same by the rule the device follows: every slot chases its own chain of lower-slot parents and counts the links; all
    slots at once, one link per round (numpy)."""
    ppid = np.asarray(ppid, dtype=np.int64)
    n = len(ppid) if n is None else n
    idx = np.arange(n)
    parent = np.where((ppid[:n] < 0) | (ppid[:n] >= n), idx, ppid[:n])
    level = np.zeros(n, dtype=np.int64)
    cur = idx.copy()
    while True:
        nxt = parent[cur]
        go = nxt < cur
        if not go.any():
            break
        level += go
        cur = np.where(go, nxt, cur)
    return parent, level, bool(np.any(parent != idx)), int(level.max()) if n else 0


# ---- the host-stop route --------------------------------------------------------------------------------------------------------
def n_eff_slot_order(w):
    """1 / sum w_i^2 in the arithmetic of resample_plan_kernel's lane 0: the sum starts at 0 and takes one particle after the other in
    slot order, each step ONE rounding of s + w_i * w_i (the compiler contracts the kernel's product and sum into a fused
    multiply-add: v_fmac_f64 in its code object), then one correctly rounded division.  Exact rational arithmetic rounded to the
    nearest double once per step is that fused step."""
    s = 0.0
    for v in np.asarray(w, dtype=np.float64):
        v = Fraction(float(v))
        s = float(Fraction(s) + v * v)
    return 1.0 / s


class HostRoute:
    """RBPHDFilter::update (:444-541) around a handle, every decision on the host: cycle_async without predict, the two gates, then
    weight_sums / normalize_weights / get_weights / N_eff / systematic_resample_plan / resample_apply, or the second normalisation.
    N_eff is added as the device adds it (n_eff_slot_order)."""

    def __init__(self, pkg, f, eff_n, eff_pct):
        self.plan_fn = pkg.engine.systematic_resample_plan
        self.f, self.eff_n, self.eff_pct = f, float(eff_n), float(eff_pct)
        self.n_upd = self.n_meas = 0
        self.n_cycles = self.n_gate = self.n_fired = 0

    def update(self, Z, u01, scan=None):
        f = self.f
        cfg = f.get_filter_config()
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, f.dz)
        self.n_upd += 1
        self.n_cycles += 1
        out = dict(gate_open=False, fired=False, n_eff=0.0, plan=np.arange(f.n, dtype=np.int32))
        if Z.shape[0] == 0:
            return out
        self.n_meas += Z.shape[0]
        if scan is not None:
            f.set_laser_scan(scan)
        f.cycle_async(None, Z, normalize=False)
        gate = self.n_upd >= cfg.minUpdatesBeforeResample and self.n_meas >= cfg.minMeasurementsBeforeResample
        out["gate_open"] = bool(gate)
        f.normalize_weights(f.weight_sums()[0])
        if not gate:
            return out
        self.n_gate += 1
        w = f.get_weights()
        neff = n_eff_slot_order(w)
        out["n_eff"] = neff
        if neff > self.eff_n and neff / f.n > self.eff_pct:
            f.normalize_weights(f.weight_sums()[0])
            return out
        plan = np.asarray(self.plan_fn(w, float(u01)), dtype=np.int32)
        f.resample_apply(plan)
        self.n_upd = self.n_meas = 0
        self.n_fired += 1
        out["fired"], out["plan"] = True, plan
        return out


def device_update(f, Z, u01, scan=None):
    """The same update as one rfsgpu_rbphd_cycle_async; nothing is read."""
    f.rbphd_cycle_async(np.asarray(Z, dtype=np.float64).reshape(-1, f.dz), u01, scan=scan)


def same_outcome(h, lc):
    assert lc["gate_open"] == h["gate_open"] and lc["fired"] == h["fired"], (h, lc)
    assert lc["n_eff"] == h["n_eff"], (lc["n_eff"], h["n_eff"])
    assert np.array_equal(lc["plan"], h["plan"])


# ---- states -----------------------------------------------------------------------------------------------------------------------
def state(f):
    n = f.n
    ids = f.get_particle_ids()
    return dict(n=n, w=f.get_weights().copy(), poses=f.get_poses().copy(), sizes=np.asarray(f.gm_sizes()).copy(),
                fov=np.array([f.landmarks_in_fov(i) for i in range(n)]), unused=np.asarray(f.get_unused_masks()).copy(),
                maps=[tuple(np.array(x) for x in f.export_gm(i)) for i in range(n)],
                cands=[tuple(np.array(x) for x in f.export_birth_candidates(i)) for i in range(n)],
                ids=np.array(ids[0]), parents=np.array(ids[1]), resampled=bool(f.resample_occured()))


def assert_same_state(a, b):
    assert a["n"] == b["n"]
    for k in ("w", "poses", "sizes", "fov", "unused", "ids", "parents"):
        assert np.array_equal(a[k], b[k]), k
    assert a["resampled"] == b["resampled"]
    for i in range(a["n"]):
        for x, y in zip(a["maps"][i], b["maps"][i]):
            assert x.shape == y.shape and np.array_equal(x, y), "mixture of particle %d" % i
        for x, y, what in zip(a["cands"][i], b["cands"][i], ("mean", "cov", "support", "check")):
            assert x.shape == y.shape and np.array_equal(x, y), "candidate %s of particle %d" % (what, i)


# ---- handles ------------------------------------------------------------------------------------------------------------------------
def candidate_config(f, thr, min_updates, min_measurements=1, check_thr=2, cur_thr=0):
    cfg = f.get_filter_config()
    cfg.birthGaussianMeasurementCountThreshold = thr
    if thr != 1:
        cfg.birthGaussianMeasurementCheckThreshold = check_thr
        cfg.birthGaussianMeasurementSupportDist = 2.0
        cfg.birthGaussianCurrentMeasurementCountThreshold = cur_thr
    cfg.minUpdatesBeforeResample = min_updates
    cfg.minMeasurementsBeforeResample = min_measurements
    f.set_filter_config(cfg)
    if hasattr(f, "config"):
        f.config = cfg


def make_pair(pkg, sc, scen, thr, min_updates, eff_n, eff_pct, cap=96, min_measurements=1, check_thr=2, same_particles=False):
    """(host route, device route): two handles of the scenario's model in the same state.  same_particles: every particle gets
    particle 0's pose and map, so that every update leaves equal weights."""
    model = pkg.capi.MODEL_VICTORIAPARK_3D if scen.get("model") == "vp" else pkg.capi.MODEL_RNGBRG_2D
    out = []
    for _ in range(2):
        f = pkg.RBPHDFilter(scen["n"], gm_capacity=cap, model=model)
        sc.load_scenario(f, scen, maps=not same_particles)
        if same_particles:
            f.set_poses(np.tile(scen["poses"][0], (scen["n"], 1)), scen["pose_cov"])
            for i in range(scen["n"]):
                f.import_gm(i, scen["w"][0], scen["mean"][0], scen["cov"][0])
        candidate_config(f, thr, min_updates, min_measurements, check_thr)
        f.rbphd_set_resampling(eff_n, eff_pct)
        out.append(f)
    return HostRoute(pkg, out[0], eff_n, eff_pct), out[1]


def far_candidates(k, dm, x0=1000.0):
    """k candidates no measurement supports, one supporting measurement each, no checks yet."""
    mean = np.zeros((k, dm))
    mean[:, 0] = x0 + 10.0 * np.arange(k)
    mean[:, 1] = 1000.0
    if dm == 3:
        mean[:, 2] = 0.5
    return mean, np.tile(np.eye(dm) * 0.01, (k, 1, 1)), np.ones(k, np.int32), np.zeros(k, np.int32)
