#!/usr/bin/env python3
"""Randomised differential run of the FastSLAM / MH-FastSLAM update, device vs oracle (GPU box): random shapes, hypothesis
counts 1..5, likelihood-difference windows, candidate thresholds; four cycles with particle growth, forced and conditional
resample(nParticles_init), candidate inheritance.   python tools/fuzz_fastslam.py [n_cases] [seed]"""
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package
import importlib
pkg = load_package()
sc = pkg.scenarios
ob = importlib.import_module("oracle.binding")
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
rng_crowded = np.random.default_rng([int(sys.argv[2]) if len(sys.argv) > 2 else 1, 64])   # its own stream: the other draws of a seed stay as they were


def compare(dev, orc):
    assert dev.n == orc.n, (dev.n, orc.n)
    wd, wo = dev.get_weights(), orc.get_weights()
    # (a zero / non-finite weight sum: raw weights, agreement on non-finiteness, counted -- never NaN against NaN)
    global n_degenerate
    sd, so = float(np.sum(wd)), float(np.sum(wo))
    if np.isfinite(sd) and np.isfinite(so) and sd > 0.0 and so > 0.0:
        np.testing.assert_allclose(wd / sd, wo / so, rtol=1e-9, atol=1e-300)
    else:
        n_degenerate += 1
        fd, fo = np.isfinite(wd), np.isfinite(wo)
        assert np.array_equal(fd, fo) and np.array_equal(np.isnan(wd), np.isnan(wo)), "device and oracle disagree on which weights are finite"
        np.testing.assert_allclose(wd[fd], wo[fo], rtol=1e-9, atol=1e-300)
    assert np.array_equal(dev.gm_sizes(), orc.gm_sizes())
    for i in range(dev.n):
        sc.assert_gm_close(dev.export_gm(i), orc.export_gm(i), 1e-10, 1e-12, ordered=True)
        md, cd, sd, kd = dev.export_birth_candidates(i)
        mo, co, so, ko = orc.export_birth_candidates(i)
        assert list(sd) == list(so) and list(kd) == list(ko), i
        np.testing.assert_allclose(md, mo, rtol=1e-9, atol=1e-11)


def table_dim(orc, P, poses, n_z):
    """The largest nMZ = max(landmarks in range, measurements) over the particles, range-bearing model: a landmark is in range when
    its Pd is not 0 or it is close to the sensing limit, i.e. its distance lies in [rmin - rbuf, rmax + rbuf]."""
    n_in = 0
    for i in range(orc.n):
        mu = orc.export_gm(i)[2]
        r = np.hypot(mu[:, 0] - poses[i, 0], mu[:, 1] - poses[i, 1]) if len(mu) else np.zeros(0)
        n_in = max(n_in, int(np.sum((r >= P["rmin"] - P["rbuf"]) & (r <= P["rmax"] + P["rbuf"]))))
    return max(n_in, n_z)


bad = grown = n_refused = n_crowded = 0
n_degenerate = 0
for case in range(n_cases):
    hyp = int(rng.choice([1, 1, 2, 3, 5]))
    crowded = False
    n0 = int(rng.integers(3, 10))
    kw = dict(n_particles=n0, n_landmarks=int(rng.choice([2, 6, 12, 25, 40])), n_z=int(rng.integers(1, 14)), seed=int(rng.integers(1 << 30)),
              rmax=float(rng.choice([4.0, 5.0, 8.0])))
    if hyp == 1 and rng.random() < 0.4:
        kw.update(n_landmarks=int(rng.choice([70, 130, 200])), n_z=int(rng.integers(10, 40)), rmax=float(rng.choice([12.0, 25.0])))
    elif hyp > 1 and rng_crowded.random() < 0.4:
        # crowded tables for Murty: the default 2.5 m range, every landmark in range, nMZ = max(landmarks, measurements) up to 64 (the
        # LDS tile's limit of 32, the second queue register and the largest table all lie in here).  Later cycles add landmarks: a
        # table that outgrows 64 must be refused by the device (checked below against table_dim of the oracle's maps) and ends the case.
        crowded = True
        kw.pop("rmax")
        kw.update(n_landmarks=int(rng_crowded.integers(8, 65)), n_z=int(rng_crowded.integers(4, 65)))
        n_crowded += 1
    vp = rng.random() < 0.3          # Victoria Park model (3-D landmarks, scan-based Pd)
    if vp:
        n_crowded -= int(crowded)
        crowded = False
        kw = dict(n_particles=n0, n_landmarks=int(rng.choice([3, 10, 30, 60])), n_z=int(rng.integers(1, 14)), seed=int(rng.integers(1 << 30)),
                  scan=str(rng.choice(["const", "ragged"])))
        scen = sc.make_vp_scenario(**kw)
        if rng.random() < 0.5:
            scen["mean"][:, ::3, 2] = rng.uniform(0.04, 0.2)
            scen["cov"][:, ::3, 0, 0] *= rng.uniform(10, 200)
            scen["cov"][:, ::3, 1, 1] *= rng.uniform(10, 200)
    else:
        scen = sc.make_scenario(**kw)
    diff = float(rng.choice([2.0, 5.0, 50.0]))
    model = pkg.capi.MODEL_VICTORIAPARK_3D if vp else pkg.capi.MODEL_RNGBRG_2D
    dev = pkg.RBPHDFilter(n0, gm_capacity=320, max_particles=n0 * hyp * 4, model=model)
    orc = ob.OracleFilter(n0, model=model)
    try:
        for f in (dev, orc):
            sc.load_scenario(f, scen)
            for i in range(n0):
                f.import_gm(i, np.zeros(scen["w"][i].shape), scen["mean"][i], scen["cov"][i])
            cfg = f.default_fastslam_config()
            cfg.maxNDataAssocHypotheses = hyp
            cfg.maxDataAssocLogLikelihoodDiff = diff
            cfg.landmarkCandidateMeasurementCountThreshold = int(kw["seed"] % 3) + 1
            cfg.landmarkCandidateCurrentMeasurementCountThreshold = int(kw["seed"] % 2)
            cfg.landmarkCandidateMeasurementCheckThreshold = 3
            f.set_fastslam_config(cfg)
        poses = scen["poses"].copy()
        rz, ru = np.random.default_rng(kw["seed"]), np.random.default_rng(kw["seed"] + 1)
        for step in range(4):
            Z = scen["Z"] + rz.normal(0, 3e-3, scen["Z"].shape)
            orc.predict_map(False)
            dev.predict_map(False)
            if crowded and table_dim(orc, scen["params"], poses, len(Z)) > 64:      # a table beyond Murty's 64: the device must refuse, untouched
                n_before = dev.n
                try:
                    dev.fastslam_update(Z)
                except pkg.capi.EngineError as e:
                    assert e.status == pkg.capi.ERR_UNSUPPORTED and dev.n == n_before, (e.status, dev.n, n_before)
                else:
                    raise AssertionError("a table of more than 64 rows was accepted")
                n_refused += 1
                break
            for f in (dev, orc):
                f.fastslam_update(Z)
            par = dev.particle_parents()
            assert np.array_equal(par, orc.particle_parents())
            grown += int(dev.n > len(poses))
            poses = poses[par]
            compare(dev, orc)
            for f in (dev, orc):
                s = f.weight_sums()
                f.normalize_weights(s[0])
            resampled = dev.n > 2 * n0 or step == 2
            if resampled:
                plan = pkg.engine.systematic_resample_plan(orc.get_weights(), float(ru.random()), n_out=n0)
                for f in (dev, orc):
                    f.resample_apply(plan, n_out=n0)
                poses = poses[plan]
                compare(dev, orc)
            for f in (dev, orc):
                f.fastslam_set_resample_occured(resampled)
                f.set_poses(poses, scen["pose_cov"])
    except Exception as e:  # noqa: BLE001
        bad += 1
        print("VP CASE" if vp else "CASE", case, kw, "hyp", hyp, "diff", diff, "->", type(e).__name__, str(e)[:300], flush=True)
    dev.close()
print("fastslam fuzz: %d cases, %d failures (updates that multiplied particles: %d); %d weight comparisons had a zero / non-finite sum "
      "and were made on the raw weights; %d crowded cases, %d of them ended in a correct refusal of a table beyond 64" % (n_cases, bad, grown, n_degenerate, n_crowded, n_refused))
sys.exit(1 if bad else 0)
