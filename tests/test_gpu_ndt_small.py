"""The small cycle of an NDT context (mcl_set_ndt_small_cycle): the wave-per-particle reweight (k_reweight_ndt_wave) against the
lane-per-particle kernel, bit for bit; whole cycles - propagation, that reweight, the one-launch tail, and the host's end of a cycle the
tail hands back - against the CPU oracle's stages with the comparisons and tolerances of test_gpu_ndt.py (resampling counts and the KLD
cut exact, ancestors except at CDF-step ties, estimates 1e-9, the random state probability 1e-12); a refused generator in a handed-back
cycle; determinism; and the cases the switch refuses."""
import math

import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import Amcl, AmclParams, LikelihoodFieldModelParam, NDTMap2d, NDTModelParam2d, se2_from_xytheta
from oracle import binding as orc

import ndt_reference as ref
from test_gpu_ndt import HASH, MOTION, MOTION_T, NODE, _tie_flips, ref_map, ring_scan, turtlebot_grid, turtlebot_ndt

pytestmark = pytest.mark.gpu

RES = 0.5


def patchwork_ndt(seed=5):
    """Keys -8 .. 7 on both axes at 0.5 m: a solid block on the left (every look-up of the 3 x 3 kernel finds 9 cells inside it), a
    checkerboard in the middle (4 or 5 of 9), single cells on the right, nothing in the top rows - 0 to 9 present per look-up."""
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = []
    for x in range(-8, 8):
        for y in range(-8, 5):
            if x < -2 or (x < 3 and (x + y) % 2 == 0) or (x >= 3 and x % 3 == 0 and y % 3 == 0):
                keys.append((x, y))
    keys = np.array(keys, dtype=np.int32)
    means = (keys + 0.5) * RES + rng.uniform(-0.2, 0.2, keys.shape)
    a = rng.uniform(0.01, 0.08, len(keys))
    d = rng.uniform(0.01, 0.08, len(keys))
    b = rng.uniform(-0.9, 0.9, len(keys)) * np.sqrt(a * d)
    covs = np.stack([np.stack([a, b], 1), np.stack([b, d], 1)], 1)
    return NDTMap2d(keys, means, covs, RES)


def present_per_lookup(m, states, means):
    """How many of the 3 x 3 kernel's cells are present around cell_near(state * mean), for every (state, measurement cell)."""
    have = {(int(x), int(y)) for x, y in m.cells}
    c, s, x, y = states[:, 0:1], states[:, 1:2], states[:, 2:3], states[:, 3:4]
    ux = c * means[None, :, 0] - s * means[None, :, 1] + x
    uy = s * means[None, :, 0] + c * means[None, :, 1] + y
    kx, ky = np.floor(ux / m.resolution).astype(int), np.floor(uy / m.resolution).astype(int)
    count = np.zeros(kx.shape, dtype=int)
    for i in range(kx.shape[0]):
        for j in range(kx.shape[1]):
            count[i, j] = sum((kx[i, j] + dx, ky[i, j] + dy) in have for dx in (-1, 0, 1) for dy in (-1, 0, 1))
    return count


def edge_states(n, seed):
    """The first states are the edges: a heading with a negative cosine (the reflection of the measurement cells), poses inside the
    keys' box, on its border (the box is [-4, 4) x [-4, 2.5) m; with the kernel's reach of one cell the centre box ends half a metre
    farther out), and farther than the reach outside it; the rest is a cloud that covers the map and its surroundings."""
    special = [se2_from_xytheta(-2.0, -1.0, 2.5), se2_from_xytheta(-4.0, 0.3, 0.4), se2_from_xytheta(60.0, -45.0, 1.0),
               se2_from_xytheta(0.2, 0.1, 0.0), se2_from_xytheta(3.9999, 2.4999, -2.0), se2_from_xytheta(-4.5, -4.5, 3.1),
               se2_from_xytheta(4.5, 3.0, -0.3), se2_from_xytheta(-6.1, 0.0, 0.0)]
    cloud = synth.normal_particles(max(n, 1), (0.0, -0.5, 0.0), (3.5, 3.5, 3.0), seed=seed)
    return np.concatenate([np.array(special), cloud])[:n]


def measurement_cells(k, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.uniform(-math.pi, math.pi, k)
    r = rng.uniform(0.3, 3.5, k)
    means = np.stack([r * np.cos(a), r * np.sin(a)], 1)
    sa, sd = rng.uniform(1e-5, 0.05, k), rng.uniform(1e-5, 0.05, k)
    sb = rng.uniform(-0.9, 0.9, k) * np.sqrt(sa * sd)
    return means, np.stack([sa, sb, sb, sd], 1)


KS = [0, 1, 3, 4, 5, 63, 64, 65, 67, 128, 131]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_wave_kernel_weights_are_the_lane_kernels_bits(n):
    """Quad, pass and remainder edges of the measurement cells (K) against the four-particle block and its tail (n)."""
    m = patchwork_ndt()
    states = edge_states(n, seed=n)
    w0 = np.random.Generator(np.random.PCG64(n)).uniform(0.5, 2.0, n)
    params = AmclParams(min_particles=n, max_particles=n)
    lanes = Amcl(m, MOTION, NODE, params, seed=3)
    waves = Amcl(m, MOTION, NODE, params, seed=3, ndt_small_cycle=True)
    assert waves.ndt_small_cycle() and not lanes.ndt_small_cycle()
    for k in KS:
        means, covs = measurement_cells(k, seed=100 + k)
        out = []
        for f in (lanes, waves):
            f.set_particles(states, w0)
            f.reweight_ndt_cells(means, covs)
            out.append(f.particles()[1])
        assert np.array_equal(out[0], out[1]), f"K = {k}: {np.flatnonzero(out[0] != out[1])[:5]}"
        if k == 0:
            assert np.array_equal(out[1], w0)
        else:
            assert np.all(out[1] >= w0 * (1.0 + k * NODE.minimum_likelihood) * (1 - 1e-12))
    if n == 257:  # the inputs cover what they claim: 0 .. 9 of 9 cells present, and likelihoods above the floor
        means, _ = measurement_cells(131, seed=231)
        present = present_per_lookup(m, states, means)
        assert present.min() == 0 and present.max() == 9 and set(range(10)) <= set(np.unique(present))
        assert np.mean(out[1] > w0 * (1.0 + 131 * NODE.minimum_likelihood) * (1 + 1e-9)) > 0.3
    lanes.close()
    waves.close()


def test_stage_level_reweight_takes_the_wave_kernel_up_to_4096():
    """mcl_reweight (the scan fitted on the host) through both kernels at the size rule's edge, and one beyond it."""
    m = turtlebot_ndt()
    pts = ring_scan((0.0, 0.0), 720, seed=2)
    for n in (4096, 4097):
        states = synth.normal_particles(n, (0.0, 0.0, 0.0), (1.2, 1.2, 3.0), seed=n)
        out = []
        for on in (False, True):
            f = Amcl(m, MOTION, NODE, AmclParams(min_particles=n, max_particles=n), seed=3, ndt_small_cycle=on)
            f.set_particles(states, np.ones(n))
            f.reweight(pts)
            out.append(f.particles()[1])
            f.close()
        assert np.array_equal(out[0], out[1]), n
        means, covs = ref.to_cells(pts, m.resolution)
        want = ref.weights_vectorized(ref_map(m), states, means, covs, NODE.minimum_likelihood, NODE.d1, NODE.d2)
        np.testing.assert_allclose(out[1], want, rtol=1e-12)


def thrun(slow, fast, a_slow, a_fast, average):
    slow = average if slow == 0.0 else slow + a_slow * (average - slow)
    fast = average if fast == 0.0 else fast + a_fast * (average - fast)
    p = min(max(1.0 - fast / slow, 0.0), 1.0) if slow != 0.0 else 0.0
    return slow, fast, p


def _cycles_against_oracle(a_slow, a_fast, start_dispersed, cycles=30, min_p=500, max_p=2000, seed=21):
    """test_gpu_ndt._cycle_against_oracle with the switch on, the recovery estimator restated beside it, and the counters of the two
    kinds of small cycle.  Returns per cycle (handed back, random state probability, particles)."""
    m = turtlebot_ndt()
    rm = ref_map(m)
    params = AmclParams(min_particles=min_p, max_particles=max_p, alpha_slow=a_slow, alpha_fast=a_fast)
    gpu = Amcl(m, MOTION, NODE, params, seed=seed, ndt_small_cycle=True)
    truth = (-0.5, 0.3, 0.2)
    if start_dispersed:  # min_p states all over the map: the first resampling finds many bins and grows the set to max_p
        states = synth.normal_particles(min_p, (truth[0], truth[1], 0.0), (1.5, 1.5, 3.0), seed=seed)
        gpu.set_particles(states, np.ones(min_p))
        w = np.ones(min_p)
    else:
        cov = np.diag([0.09, 0.09, 0.04])
        gpu.initialize(truth, cov)
        states, w = orc.init_normal(max_p, truth, cov, seed)
        g0, _ = gpu.particles()
        np.testing.assert_allclose(g0, states, rtol=1e-12, atol=1e-12)
        states = g0.copy()
    slow = fast = 0.0
    odom, prev = (0.0, 0.0, 0.0), None
    rows = []
    for c in range(cycles):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        pts = ring_scan((0.0, 0.0), 360, seed=c)
        gpu.force_update()
        before = gpu.ndt_small_cycle_counts()
        tails = gpu.counter("small_tail_launches")
        est = gpu.update(ctrl, pts)
        assert est is not None
        done, back = (a - b for a, b in zip(gpu.ndt_small_cycle_counts(), before))
        assert done + back == 1 and gpu.counter("small_tail_launches") == tails + 1, f"cycle {c}: not a small cycle"
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        means, covs = ref.to_cells(pts, m.resolution)
        w = orc.normalize(w * ref.weights_vectorized(rm, states, means, covs, NODE.minimum_likelihood, NODE.d1, NODE.d2))[0]
        slow, fast, p = thrun(slow, fast, a_slow, a_fast, w.sum() / len(w))
        info = gpu.last_info
        assert info["resampled"] and info["random_state_probability"] == pytest.approx(p, abs=1e-12), f"cycle {c}"
        p = info["random_state_probability"]  # (the library's own bits for the Bernoulli comparisons)
        assert back == (1 if p > 0.0 else 0), f"cycle {c}: p = {p}"
        got, gw = gpu.particles()
        assert np.all(gw == 1.0) and info["num_particles"] == len(got)
        if p > 0.0:
            # Random states: the oracle's stand-in states are not N(estimate), so the KLD cut (which hashes them) is the library's own;
            # the candidate stream is compared over the set's length: the injected slots are the oracle's (random_intersperse), the
            # other slots hold the oracle's ancestors.
            slow = fast = 0.0
            want, anc = orc.resample(states, w, max_p, max_p, 0.05, 3.0, HASH, p, seed, c + 1, free_xy=np.zeros((1, 2)))
            assert min_p <= len(got) <= max_p
            inj = anc[:len(got)] == -1
            assert _tie_flips(got, want, w, seed, c + 1, np.flatnonzero(~inj)) <= 3, f"cycle {c}"
            if inj.sum() > 20:  # the injected slots hold states of no ancestor: N(estimate of the normalised set)
                mean, ecov = orc.estimate(states, w)
                assert abs(got[inj, 2].mean() - mean[2]) < 5 * math.sqrt(ecov[0, 0] / inj.sum())
        else:
            want, anc = orc.resample(states, w, min_p, max_p, 0.05, 3.0, HASH, 0.0, seed, c + 1)
            assert len(got) == len(want), f"cycle {c}: particle counts differ"
            flips = int(np.any(np.abs(got - want) > 1e-9, axis=1).sum())
            assert flips <= 3, f"cycle {c}: {flips} ancestors differ"
        om, oc = orc.estimate(got, np.ones(len(got)))
        np.testing.assert_allclose(est[0], om, atol=1e-9)
        np.testing.assert_allclose(est[1], oc, rtol=1e-8, atol=1e-9)
        rows.append((back == 1, p, len(got)))
        states, w = got, np.ones(len(got))
    gpu.close()
    return rows


def test_cycles_without_random_states_all_end_in_the_tail():
    """alpha_slow == alpha_fast: the two filters never move apart, p is exactly 0 in every cycle."""
    rows = _cycles_against_oracle(0.05, 0.05, start_dispersed=False)
    assert len(rows) == 30 and not any(back for back, _, _ in rows) and all(p == 0.0 for _, p, _ in rows)
    assert min(n for _, _, n in rows) < 2000  # (the KLD cut is at work)


def test_cycles_with_the_reference_defaults_hand_back_when_the_set_grows():
    """alpha 0.001 / 0.1 and a set that starts at min_particles, dispersed: the first resampling grows it, the average weight drops to
    a quarter, the fast filter follows it down ahead of the slow one, and the next cycle injects random states - handed back.  The
    filters' reset behind it puts the following cycle back into the tail."""
    rows = _cycles_against_oracle(0.001, 0.1, start_dispersed=True)
    handed = [c for c, (back, _, _) in enumerate(rows) if back]
    assert handed, rows
    assert rows[0][2] > 500, "the first resampling did not grow the set"
    assert any(not rows[c + 1][0] for c in handed if c + 1 < len(rows)), rows


def collapsed(n):
    states = np.tile(se2_from_xytheta(0.1, 0.2, 0.3), (n, 1))
    states[:, :2] = [[1.0, 0.0] if i % 2 else [-1.0, 0.0] for i in range(n)]  # headings cancel: infinite circular variance
    return states


def test_refused_generator_in_a_handed_back_cycle():
    """The set collapsed to one point with cancelling headings, a scan without a measurement cell and the filters put apart: the tail
    hands back, the generator is refused (an infinite circular variance).
    As DESIGN describes the failure: set propagated (a first update: by no motion), reweighted and normalised, estimator and policy
    advanced, no particle replaced, estimator not reset; the step taken.  The general path (switch off) leaves the same state.  The next update on a sane set works."""
    m = turtlebot_ndt()
    n = 64
    left = {}
    for on in (True, False):
        f = Amcl(m, MOTION, NODE, AmclParams(min_particles=n, max_particles=n), seed=9, ndt_small_cycle=on)
        f.set_particles(collapsed(n), np.ones(n))
        f.debug_set_recovery_filters(2.0 / n, 0.5 / n)
        pts = ring_scan((0.0, 0.0), 360, seed=1)
        with pytest.raises(capi.MclError) as e:  # (four points: no measurement cell, the weights stay equal and the headings cancel)
            f.update(se2_from_xytheta(0.0, 0.0, 0.0), pts[::90])
        assert e.value.status == capi.MCL_ERR_BAD_COVARIANCE
        states, w = f.particles()
        assert len(states) == n and np.array_equal(states[:, :2], collapsed(n)[:, :2])  # none replaced by a draw (a first update: no motion)
        assert abs(w.sum() - 1.0) < 1e-12 and not np.all(w == 1.0)  # reweighted and normalised
        if on:
            assert f.ndt_small_cycle_counts() == (0, 1)
        left[on] = (states, w)
        # a sane set: the update succeeds; the step has advanced by one (the same noise as a twin that made two updates would not be
        # drawn twice), the filters were advanced and not reset: p > 0 again, and this time the generator stands
        sane = synth.normal_particles(n, (-0.5, 0.3, 0.2), (0.3, 0.3, 0.2), seed=4)
        f.set_particles(sane, np.ones(n))
        f.force_update()
        est = f.update(se2_from_xytheta(0.3, 0.0, 0.05), pts)
        assert est is not None and np.all(np.isfinite(est[0])) and f.last_info["random_state_probability"] > 0.0
        left[on] += (f.particles()[0], f.last_info["random_state_probability"])
        if on:
            assert f.ndt_small_cycle_counts() == (0, 2)
        f.close()
    assert np.array_equal(left[True][0], left[False][0])  # the propagation is the same kernel on the same step
    np.testing.assert_allclose(left[True][1], left[False][1], rtol=1e-12)
    assert left[True][3] == pytest.approx(left[False][3], abs=1e-12)  # the filters went the same way


def test_two_contexts_return_the_same_bits():
    m = turtlebot_ndt()
    runs = []
    for _ in range(2):
        f = Amcl(m, MOTION, NODE, AmclParams(min_particles=500, max_particles=2000), seed=77, ndt_small_cycle=True)
        states = synth.normal_particles(500, (-0.5, 0.3, 0.0), (1.5, 1.5, 3.0), seed=2)
        f.set_particles(states, np.ones(500))
        odom, out = (0.0, 0.0, 0.0), []
        for c in range(10):
            odom = synth.odometry_step(odom, 0.3, 0.05)
            f.force_update()
            est = f.update(se2_from_xytheta(*odom), ring_scan((0.0, 0.0), 360, seed=c))
            s, w = f.particles()
            out.append((est[0], est[1], s, w, tuple(sorted(f.last_info.items()))))
        out.append(f.ndt_small_cycle_counts())
        runs.append(out)
        f.close()
    assert runs[0][-1] == runs[1][-1] and sum(runs[0][-1]) == 10 and runs[0][-1][1] >= 1  # (a handed-back cycle among them)
    for a, b in zip(runs[0][:-1], runs[1][:-1]):
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def test_refusals():
    lib = capi.load()
    g = Amcl(turtlebot_grid(), MOTION, LikelihoodFieldModelParam(), AmclParams(min_particles=10, max_particles=10))
    with pytest.raises(capi.MclError) as e:
        g.set_ndt_small_cycle(True)
    assert e.value.status == capi.MCL_ERR_UNSUPPORTED
    g.close()
    m = turtlebot_ndt()
    f = Amcl(m, MOTION, NODE, AmclParams(min_particles=10, max_particles=10))
    assert not f.ndt_small_cycle()  # the default
    for bad in (2, -1):
        assert lib.mcl_set_ndt_small_cycle(f._ctx, bad) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_set_ndt_small_cycle(None, 1) == capi.MCL_ERR_INVALID_ARGUMENT
    f.set_ndt_small_cycle(True)
    assert f.ndt_small_cycle()
    f.set_ndt_small_cycle(False)
    assert not f.ndt_small_cycle()
    f.close()


def test_4097_particles_take_the_general_path():
    m = turtlebot_ndt()
    n = 4097
    out = []
    for on in (True, False):
        f = Amcl(m, MOTION, NODE, AmclParams(min_particles=n, max_particles=n), seed=5, ndt_small_cycle=on)
        f.initialize((-0.5, 0.3, 0.2), np.diag([0.09, 0.09, 0.04]))
        odom, rows = (0.0, 0.0, 0.0), []
        for c in range(3):
            odom = synth.odometry_step(odom, 0.3, 0.05)
            f.force_update()
            est = f.update(se2_from_xytheta(*odom), ring_scan((0.0, 0.0), 360, seed=c))
            s, w = f.particles()
            rows.append((est[0], est[1], s, w, tuple(sorted(f.last_info.items()))))
        assert f.ndt_small_cycle_counts() == (0, 0) and f.counter("small_tail_launches") == 0
        out.append(rows)
        f.close()
    for a, b in zip(*out):
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
