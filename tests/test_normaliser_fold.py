"""The map update's normaliser fold in the workgroup form (csrc/update_map.h, phd_update_map_block) against the one-wave form.

The workgroup form finds the survivors of measurement z through a bit table over the list positions and adds them once, behind the
passes; the one-wave form (phd_update_map_particle) walks the whole list after every pass.  Both add clutter first and then the
landmarks in ascending order, so a handle created under RFSGPU_UPDMAP_WPP = 2, 3 or 4 must leave what one created under
RFSGPU_UPDMAP_WPP = 1 leaves, bit for bit: weights, previous weights, means, covariances, mixture sizes, unused-measurement lists and
landmarks in the field of view.  Form 2 is also held against the oracle, ordered, at test_gpu_parity's mixture tolerances.

Planted inputs: measurements on a grid of 4 ranges x 16 bearings, 0.4 m and 0.39 rad apart (more than 4.5 standard deviations of the
innovation, whose gate is at 3), and k landmarks within a centimetre or two of the first `groups` of them, dealt round robin -- every
landmark survives for exactly one measurement, so list position == landmark index and measurement z owns positions z, z + groups, ...
Their weights are log-uniform over 1e-12 .. 1: a sum taken in another order differs in its low bits.  Every case has 4 to 16 particles."""
import functools

import numpy as np
import pytest

from tests.test_gate_index import GM_ATOL, GM_RTOL, polar_scenario, set_env, snapshot

pytestmark = pytest.mark.gpu

FORMS = ("2", "3", "4")
K_BOUNDARIES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129]     # word (32), wave (64) and pass (128 at two waves) boundaries of the list
GRID = [(r, b) for b in -2.9 + 0.39 * np.arange(16) for r in (0.8, 1.2, 1.6, 2.0)]


@functools.lru_cache(maxsize=None)
def _planted(k, groups, n_z, n=4, twin=False, seed=0):
    from __graft_entry__ import load_package
    sc = load_package().scenarios
    rng = np.random.default_rng(1000 * k + 10 * groups + n_z + seed)
    Z = np.array(GRID[:n_z])
    if twin:                                                   # measurement 1 two centimetres from measurement 0: two survivors per landmark
        Z[1] = Z[0] + np.array([0.02, 0.004])
    poses = rng.normal(0, 1, (n, 3)) * np.array([0.02, 0.02, 0.3])
    scen = polar_scenario(sc, poses, [GRID[m % groups] for m in range(k)], Z)
    scen["mean"] = scen["mean"] + rng.normal(0, 0.01, scen["mean"].shape)
    scen["w"] = 10.0 ** rng.uniform(-12, 0, (n, k))
    return scen


def planted(k, groups, n_z, **kw):
    s = _planted(k, groups, n_z, **kw)
    return dict(s, params=dict(s["params"]))


def run_form(pkg, sc, monkeypatch, scen, wpp, cap, call="update_map", env=None, capacity_error=False):
    set_env(monkeypatch, dict(env or {}, **({"RFSGPU_UPDMAP_WPP": wpp} if wpp else {})))
    f = pkg.RBPHDFilter(scen["n"], device_id=0, gm_capacity=cap)
    set_env(monkeypatch, {})
    sc.load_scenario(f, scen)
    if capacity_error:
        with pytest.raises(pkg.capi.EngineError) as e:
            getattr(f, call)(scen["Z"])
        assert e.value.status == pkg.capi.ERR_CAPACITY
    else:
        getattr(f, call)(scen["Z"])
        if call == "update_async":
            f.synchronize()
    return f


def check_forms(pkg, ob, sc, monkeypatch, scen, cap=512, oracle=True, capacity_error=False, label=""):
    """Forms 2, 3, 4 against form 1 bit for bit; form 2 against the oracle.  Returns (form 1's handle, the oracle)."""
    ref = run_form(pkg, sc, monkeypatch, scen, "1", cap, capacity_error=capacity_error)
    want = snapshot(ref, scen["n"])
    first = None
    for wpp in FORMS:
        f = run_form(pkg, sc, monkeypatch, scen, wpp, cap, capacity_error=capacity_error)
        got = snapshot(f, scen["n"])
        assert got.keys() == want.keys()
        for key in want:
            assert np.array_equal(got[key], want[key]), f"{label}: {key} differs between {wpp} waves per particle and the one-wave form"
        first = first or f
    orc = None
    if oracle:
        orc = ob.OracleFilter(scen["n"])
        sc.load_scenario(orc, scen)
        orc.update_map(scen["Z"])
        assert np.array_equal(first.gm_sizes(), orc.gm_sizes()), label
        for i in range(scen["n"]):
            sc.assert_gm_close(first.export_gm(i), orc.export_gm(i), GM_RTOL, GM_ATOL, ordered=True)
            assert np.array_equal(first.get_unused(i), orc.get_unused(i)), label
            assert first.landmarks_in_fov(i) == orc.landmarks_in_fov(i), label
    return ref, orc


@pytest.mark.parametrize("groups", [1, 2, 30])
@pytest.mark.parametrize("k", K_BOUNDARIES)
def test_planted_survivors(pkg, ob, sc, monkeypatch, k, groups):
    """k survivors of one measurement, of two and of thirty; nothing is clamped (capacity 512)."""
    scen = planted(k, groups, 30)
    ref, _ = check_forms(pkg, ob, sc, monkeypatch, scen, label=f"k={k} groups={groups}")
    assert np.array_equal(ref.gm_sizes(), np.full(scen["n"], 2 * k))            # every landmark survived once
    for i in range(scen["n"]):
        assert np.array_equal(np.sort(ref.get_unused(i)), np.arange(min(groups, k), 30))


@pytest.mark.parametrize("n_z", [1, 63, 64])
def test_measurement_counts(pkg, ob, sc, monkeypatch, n_z):
    """One measurement, 63, and RFSGPU_MAX_Z = 64, where every lane of wave 0 folds: 130 landmarks dealt over all of them."""
    scen = planted(130, n_z, n_z)
    ref, _ = check_forms(pkg, ob, sc, monkeypatch, scen, label=f"n_z={n_z}")
    assert np.array_equal(ref.gm_sizes(), np.full(scen["n"], 260))
    for i in range(scen["n"]):
        assert ref.get_unused(i).size == 0


def test_two_survivors_per_landmark(pkg, ob, sc, monkeypatch):
    """Two measurements inside the gates of every landmark: the list alternates between them, a lane keeps two values per pass."""
    scen = planted(65, 1, 30, twin=True)
    ref, _ = check_forms(pkg, ob, sc, monkeypatch, scen, label="twin")
    assert np.array_equal(ref.gm_sizes(), np.full(scen["n"], 65 + 130))


@pytest.mark.parametrize("kw", [dict(n_particles=16, n_landmarks=1, n_z=3, seed=6), dict(n_particles=16, n_landmarks=70, n_z=19, seed=2)])
def test_ragged_shapes(pkg, ob, sc, monkeypatch, kw):
    check_forms(pkg, ob, sc, monkeypatch, sc.make_scenario(**kw), label=str(kw))


@pytest.mark.parametrize("use_cluster", [0, 1])
def test_no_survivors(pkg, ob, sc, monkeypatch, use_cluster):
    """Every landmark at least 0.8 m from every measurement: nothing is appended, no measurement is used, and the normalisers are the
    clutter intensity -- which the SC-PHD particle weight (use_cluster) shows: exp(sum of weights) * clutter ** n_z, the same bits in
    every form."""
    n, n_z = 4, 30
    rng = np.random.default_rng(5)
    inner = [p for p in GRID if p[0] < 1.5]
    outer = [(r + 0.4, b) for r, b in GRID if r > 1.5]          # ranges 2.0 and 2.4
    scen = polar_scenario(sc, rng.normal(0, 1, (n, 3)) * np.array([0.02, 0.02, 0.3]), inner[:32] * 3, outer[:n_z], params=dict(use_cluster=use_cluster))
    ref, _ = check_forms(pkg, ob, sc, monkeypatch, scen, label="no survivors")
    assert np.array_equal(ref.gm_sizes(), np.full(n, 96))
    for i in range(n):
        assert np.array_equal(np.sort(ref.get_unused(i)), np.arange(n_z))
    if use_cluster:
        w = ref.get_weights()
        np.testing.assert_allclose(w, np.exp(scen["w"].sum(axis=1)) * scen["params"]["clutter"] ** n_z, rtol=1e-12)


def test_cluster_weight_reads_the_folded_normalisers(pkg, ob, sc, monkeypatch):
    """SC-PHD: the particle weight is the product of the normalisers wave 0's lanes hold after the fold."""
    scen = planted(65, 30, 30)
    scen["params"]["use_cluster"] = 1
    ref, orc = check_forms(pkg, ob, sc, monkeypatch, scen, label="use_cluster")
    wd, wo = ref.get_weights(), orc.get_weights()
    np.testing.assert_allclose(wd / wd.sum(), wo / wo.sum(), rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("groups", [1, 30])
def test_capacity_reached(pkg, sc, monkeypatch, groups):
    """129 landmarks and 129 survivors at capacity 192: room for 63.  Every form raises the capacity error and keeps the same prefix of
    the appended Gaussians -- normalised by sums over the kept survivors only: a bit set or read at a position >= room would show in
    the weights (a missing or an extra term) or in the sizes."""
    scen = planted(129, groups, 30)
    ref, _ = check_forms(pkg, None, sc, monkeypatch, scen, cap=192, oracle=False, capacity_error=True, label=f"capacity groups={groups}")
    assert np.array_equal(ref.gm_sizes(), np.full(scen["n"], 192))
    # the kept prefix is what an update with room for everything appends first -- means and covariances bit for bit; the weights differ
    # (their normalisers there include the survivors that did not fit here)
    full = run_form(pkg, sc, monkeypatch, scen, "2", 512)
    for i in range(scen["n"]):
        a, b = ref.export_gm(i), full.export_gm(i)
        assert np.array_equal(a[2][129:], b[2][129:192]) and np.array_equal(a[3][129:], b[3][129:192])


def test_underflowing_normalised_weights(pkg, ob, sc, monkeypatch):
    """test_new_gaussians_whose_normalised_weight_underflows_are_dropped_in_order's input (clutter 1e10, weights 1e-322) through every
    form: the compaction reads the survivor values behind the fold."""
    scen = sc.make_scenario(16, 90, 20, seed=77, params=dict(clutter=1e10), weights=(0.5, 1.0))
    rng = np.random.default_rng(4)
    scen["w"][rng.random(scen["w"].shape) < 0.4] = 1e-322
    ref, _ = check_forms(pkg, ob, sc, monkeypatch, scen, label="underflow")
    scen2 = dict(scen, params=dict(scen["params"], clutter=1e-4))
    more = run_form(pkg, sc, monkeypatch, scen2, "2", 512)
    assert (ref.gm_sizes() > 90).any() and (more.gm_sizes() > ref.gm_sizes()).any()    # some appended, some dropped


@pytest.mark.parametrize("step_wpp", ["2", "3"])
def test_fused_step(pkg, sc, monkeypatch, step_wpp):
    """The fused step (update_async) with two and three waves per particle against the phase-by-phase update, on the k = 65 input."""
    scen = planted(65, 30, 30)
    fused = run_form(pkg, sc, monkeypatch, scen, None, 512, call="update_async", env={"RFSGPU_STEP_WPP": step_wpp})
    phases = run_form(pkg, sc, monkeypatch, scen, "1", 512, call="update", env={"RFSGPU_FUSED_STEP": "0"})
    a, b = snapshot(fused, scen["n"]), snapshot(phases, scen["n"])
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{key} differs between the fused step with {step_wpp} waves and the separate phases"
