"""The inputs of the estimate tests, shared by test_estimate_reference_cpu.py (oracle and host finish against the exact reference, and
what each family must reach) and test_gpu_estimate_edges.py (device against reference).  Plain numpy and the oracle; nothing of the
code under test.  Everything is seeded; a reference is computed once per case and never modified."""
import math
import zlib

import numpy as np

import estimate_reference as ref
from oracle import binding as orc

CHUNK = 2048       # kChunk: k_estimate_partials' workgroup
SMALL_MAX = 4096   # kSmallMax: the one-workgroup kernels
N_STRIDED = CHUNK * 256 + 1  # 257 chunks: row_total of k_final_rows strides past its 256 lanes
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 65_537, N_STRIDED)
POSE_SIZES = (65, 4097, 65_537)

CENTRES = {"origin": (0.0, 0.0), "near": (57.3, -41.2), "km": (5e3, -3.5e3), "utm": (5e5, 4e6), "utm_west": (-4e6, 5e5)}
FAR = ("utm", "utm_west")
SPREADS = {"s0.5": 0.5, "s0.05": 0.05, "s0.01": 0.01, "wide": None}  # wide: uniform over 200 m x 150 m
WEIGHTS = ("unit", "gamma", "seventh_zero", "one_heavy", "dynamic")
HEADINGS = ("tight", "uniform", "pair")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


_clouds = {}


def cloud(n, centre, spread, weights="gamma", headings="tight"):
    """-> (states (n, 4) as (cos, sin, x, y), weights (n,)), read-only."""
    key = (n, centre, spread, weights, headings)
    if key in _clouds:
        return _clouds[key]
    rng = np.random.Generator(np.random.PCG64(_seed(*key)))
    cx, cy = CENTRES[centre]
    sigma = SPREADS[spread]
    if sigma is None:
        x, y = cx + rng.uniform(-100.0, 100.0, n), cy + rng.uniform(-75.0, 75.0, n)
    else:
        x, y = cx + rng.normal(0.0, sigma, n), cy + rng.normal(0.0, sigma, n)
    if headings == "tight":
        h = rng.normal(0.7, 0.01, n)
    elif headings == "uniform":
        h = rng.uniform(-math.pi, math.pi, n)
    else:  # the pair +-pi/2 of test_estimation.cpp's CancellingOrientations, alternating: with equal weights on both the mean sine is 0
        h = np.where(np.arange(n) % 2 == 0, math.pi / 2, -math.pi / 2)
    if weights == "unit" or headings == "pair":
        w = np.ones(n)
    elif weights == "gamma":
        w = rng.gamma(1.5, 1.0, n)
    elif weights == "seventh_zero":
        w = rng.gamma(1.5, 1.0, n)
        w[::7] = 0.0
        if n < 7:
            w[-1] = 1.0
    elif weights == "one_heavy":  # one particle holds 1 - 1e-12 of the mass
        w = rng.gamma(1.5, 1.0, n)
        if n > 1:
            k = n // 2
            rest = w.sum() - w[k]
            w[k] = rest * (1.0 / 1e-12 - 1.0)
    else:  # 1e-280 .. 1
        w = 10.0 ** rng.uniform(-280.0, 0.0, n)
        w[0] = 1.0
    s = np.stack([np.cos(h), np.sin(h), x, y], axis=1)
    s.setflags(write=False)
    w.setflags(write=False)
    _clouds[key] = (s, w)
    return _clouds[key]


def pose_cases():
    """Every centre x spread at POSE_SIZES; the weights and headings kinds rotate through the cases so that each meets far and near
    centres.  -> [(label, n, centre, spread, weights, headings)]"""
    out = []
    k = 0
    for n in POSE_SIZES:
        for centre in CENTRES:
            for spread in SPREADS:
                weights, headings = WEIGHTS[k % len(WEIGHTS)], HEADINGS[(k // 2) % len(HEADINGS)]
                if n % 2 and headings == "pair":
                    headings = "uniform"  # (an odd count leaves one of the pair uncancelled: not the degenerate branch)
                out.append((f"{n}-{centre}-{spread}-{weights}-{headings}", n, centre, spread, weights, headings))
                k += 1
    # the degenerate branch on its own: an even count, equal weights
    out.append(("64-utm-s0.05-unit-pair", 64, "utm", "s0.05", "unit", "pair"))
    return out


def sums_cases():
    """Every size, on the far centre with a tight cloud; the weight kinds at the two sizes beside kSmallMax.
    -> [(label, n, centre, spread, weights, headings)]"""
    out = [(f"{n}-utm-s0.05-gamma", n, "utm", "s0.05", "gamma", "tight") for n in SIZES]
    out += [(f"{n}-near-wide-{wk}", n, "near", "wide", wk, "uniform") for n in (4096, 4097) for wk in WEIGHTS if wk != "gamma"]
    return out


def sums_pivots(centre):
    cx, cy = CENTRES[centre]
    return {"origin": (0.0, 0.0), "centre": (cx, cy), "1e6 away": (cx + 1e6, cy - 1e6)}


# ---- what a family must reach -------------------------------------------------------------------------------------------
def pivot_distance_over_sigma(states, w, pivot):
    """Distance from the pivot to the weighted mean over the set's weighted spread (doubles: a figure, not a reference)."""
    live = w > 0
    v = w[live] / w[live].sum()
    x, y = states[live, 2], states[live, 3]
    mx, my = float(v @ (x - x[0])) + x[0], float(v @ (y - y[0])) + y[0]
    spread = math.sqrt(float(v @ ((x - mx) ** 2 + (y - my) ** 2)))
    return math.hypot(mx - pivot[0], my - pivot[1]) / spread if spread > 0 else math.inf


TARGETS = {  # (centre, spread) -> pivot-to-mean distance over sigma that the family reaches with the pivot at the origin, at least
    ("utm", "s0.5"): 5e6, ("utm", "s0.05"): 5e7, ("utm", "s0.01"): 2.5e8, ("utm", "wide"): 4e4,
    ("utm_west", "s0.5"): 5e6, ("utm_west", "s0.05"): 5e7, ("utm_west", "s0.01"): 2.5e8, ("utm_west", "wide"): 4e4,
    ("km", "s0.5"): 8e3, ("km", "s0.05"): 8e4, ("km", "s0.01"): 4e5,
}


# ---- references and yardsticks ----------------------------------------------------------------------------------------------
_references = {}
_yardsticks = {}


def reference(case):
    label = case[0]
    if label not in _references:
        _references[label] = ref.estimate(*cloud(*case[1:]))
    return _references[label]


def yardstick(case):
    """-> (the exact estimate of the case, the double-precision oracle's Errors against it)."""
    label = case[0]
    if label not in _yardsticks:
        s, w = cloud(*case[1:])
        r = reference(case)
        _yardsticks[label] = (r, ref.errors(r, *orc.estimate(s, w)))
    return _yardsticks[label]


# The oracle's worst error (pos, rot, cov, tt; units) per centre and size, over that family's cases, as recorded when the families were
# written: test_estimate_reference_cpu.py holds the oracle to 1.5 times these (other libm builds round a sine differently), so an oracle
# that got worse cannot quietly widen the device's limit.  The device's limit takes the oracle's error of the CASE, which is at most
# its family's worst.
ORACLE_WORST = {
    ('km', 65): (4.72, 0.366, 0.224, 4.1), ('km', 4097): (40.2, 8.85, 1.76, 33.2), ('km', 65537): (93, 7.29, 70, 22.8),
    ('near', 65): (1.36, 0.613, 0.28, 4.78), ('near', 4097): (39.1, 3.82, 2.27, 11.4), ('near', 65537): (201, 0.502, 4.84, 0.821),
    ('origin', 65): (0.908, 1.31, 0.127, 1.65), ('origin', 4097): (10.2, 0.637, 2.87, 12.4), ('origin', 65537): (1.49e+03, 21.9, 849, 21.8),
    ('utm', 64): (2.34, 0, 0.0777, 0), ('utm', 65): (9.44, 0.626, 1.46, 8.29), ('utm', 4097): (17.8, 1.4, 12.1, 42.1),
    ('utm', 65537): (242, 12.7, 850, 4.4e+03),
    ('utm_west', 65): (3.14, 1.08, 0.486, 2.07), ('utm_west', 4097): (15.5, 3.17, 39.9, 34.1), ('utm_west', 65537): (323, 1.59, 2.55e+04, 4.42e+03),
}


def limit(n, oracle_error, world=1):
    """What a device figure is held to, in its unit: the tree's bound, or four times the oracle's own error on the same inputs if that
    is more (the rule of propagate_families.hold)."""
    bound = ref.estimate_error_bound(n) + (world if world > 1 else 0)
    return max(float(bound), 4.0 * float(oracle_error)) if math.isfinite(oracle_error) else math.inf


def hold(label, n, got, oracle_errors, world=1):
    """got, oracle_errors: ref.Errors.  Prints the figures, then asserts each within its limit.  -> got."""
    parts = []
    for name in ref.Errors._fields:
        parts.append(f"{name} {getattr(got, name):.3g} (oracle {getattr(oracle_errors, name):.3g}, "
                     f"limit {limit(n, getattr(oracle_errors, name), world):.3g})")
    print(f"{label}: " + ", ".join(parts) + " units")
    for name in ref.Errors._fields:
        o = getattr(oracle_errors, name)
        assert math.isfinite(o), f"{label}: the oracle's {name} is not finite"
        assert getattr(got, name) <= limit(n, o, world), f"{label}: {name} {getattr(got, name)} units > {limit(n, o, world)}"
    return got


# ---- cluster sets ---------------------------------------------------------------------------------------------------------------
BLOB_OFFSETS = ((0.0, 0.0), (100.0, 0.0), (50.0, 110.0))  # 100 m, 120.8 m and 120.8 m apart
BLOB_SHARES = {2: (0.6, 0.4), 3: (0.5, 0.3, 0.2)}
BLOB_SIGMA = 0.05
BLOB_SIZES = (4096, 20_001)  # k_small_cluster_sums up to kSmallMax; k_estimate_partials_cluster(s) above
BLOB_CENTRES = ("near", "utm")


def blob_cases():
    return [(f"{n}-{centre}-{k}blobs", n, centre, k) for n in BLOB_SIZES for centre in BLOB_CENTRES for k in (2, 3)]


def blobs(n, centre, k):
    """k blobs of sigma 0.05 m, 100 .. 121 m apart, the first at the centre; gamma weights, the blobs' particles interleaved at random
    (every workgroup sees every blob).  -> (states, weights, blob of every particle), read-only."""
    key = ("blobs", n, centre, k)
    if key not in _clouds:
        rng = np.random.Generator(np.random.PCG64(_seed(*key)))
        which = rng.choice(k, size=n, p=BLOB_SHARES[k])
        which[:k] = np.arange(k)
        cx, cy = CENTRES[centre]
        off = np.array(BLOB_OFFSETS)[which]
        x, y = cx + off[:, 0] + rng.normal(0.0, BLOB_SIGMA, n), cy + off[:, 1] + rng.normal(0.0, BLOB_SIGMA, n)
        h = 0.7 + 0.3 * which + rng.normal(0.0, 0.01, n)
        s = np.stack([np.cos(h), np.sin(h), x, y], axis=1)
        w = rng.gamma(1.5, 1.0, n)
        for a in (s, w, which):
            a.setflags(write=False)
        _clouds[key] = (s, w, which)
    return _clouds[key]


def hold_clusters(label, states, w, labels, entries, overall_n):
    """entries: [(id, pose, cov)] as the code under test reports its clusters; labels: the cluster of every particle.  Each entry
    against the exact reference over the particles that carry its id, in that cluster's own units; the limit from the oracle's
    orc.estimate over the same particles.  -> the worst Errors."""
    worst = ref.Errors(0.0, 0.0, 0.0, 0.0)
    for cid, pose, cov in entries:
        members = labels == cid
        assert members.sum() > 1, (label, cid)
        s, ww = states[members], w[members]
        r = ref.estimate(s, ww)
        oracle = ref.errors(r, *orc.estimate(s, ww))
        got = hold(f"{label} cluster {cid} ({int(members.sum())} particles)", overall_n, ref.errors(r, pose, cov), oracle)
        worst = ref.Errors(*(max(a, b) for a, b in zip(worst, got)))
    return worst
