"""The CDF, its tree search and the shard routing, each against an independent reference, at the edges.

test_gpu_parity.py holds resampling to the oracle "within flips".  Here the CDF itself is read back (mcl_device_view.cdf)
and held to a high-precision prefix sum and to its contract, the searches are asked for targets chosen on and next to the
CDF's own entries, and the sharded stage entry points are held to the numpy restatements of tests/shard_oracle_engine.py.

The CDF's contract ("The CDF's contract"):
  * cdf[i] >= cdf[i-1]; cdf[i] == cdf[i-1] wherever w[i] == 0; cdf[0] == w[0]; total == cdf[n-1], bit for bit;
  * |cdf[i] - exact prefix sum| <= cdf_error_bound(n) * 2^-53 * total.

Definition D (include/beluga_mcl.h, mcl_serve_requests): the served index is the first i with cdf[i] >= t, or n - 1 if
there is none.  It is evaluated on the CDF as read back, without assuming that it is sorted.

Every particle's state names it: x = its index (exact in f64 below 2^53), so a reply identifies its ancestor.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from beluga_amd.amcl import Amcl, AmclParams
from oracle import binding as orc
from shard_oracle_engine import OracleShardEngine
from test_gpu_parity import LF, MOTION, MOTION_T, rooms_grid

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEED = 11
CHUNK, BLOCK = 2048, 256  # kChunk, kBlock (kernels.h)
CAPACITY = 4_200_000

# ---- reading device memory ---------------------------------------------------------------------------
_hip = None


def _hip_runtime():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def read_cdf(f):
    """The n entries of mcl_device_view.cdf, copied from the raw pointer by the HIP runtime after mcl_sync."""
    f.sync()
    v = f.device_view()
    out = np.empty(int(v.n), dtype=np.float64)
    if v.n:
        st = _hip_runtime().hipMemcpy(out.ctypes.data, v.cdf, out.nbytes, 2)  # hipMemcpyDeviceToHost
        assert st == 0, f"hipMemcpy: {st}"
    return out


def named_states(n):
    s = np.zeros((n, 4))
    s[:, 0] = 1.0
    s[:, 2] = np.arange(n, dtype=np.float64)
    return s


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u53(r):
    return float(((int(r[0]) << 32) | int(r[1])) >> 11) * 2.0 ** -53


def first_at_least(cdf, targets):
    """Definition D on an array that need not be sorted: the first i with max(cdf[0..i]) >= t is the first i with cdf[i] >= t."""
    idx = np.searchsorted(np.maximum.accumulate(cdf), targets, side="left")
    return np.minimum(idx, len(cdf) - 1)


# ---- the cases of part A -------------------------------------------------------------------------------
SIZES = {
    1: "one", 2: "two", 15: "group-1", 16: "group", 17: "group+1", 255: "level2-1", 256: "level2", 257: "level2+1",
    2047: "chunk-1", 2048: "chunk", 2049: "chunk+1", 4096: "level3=2chunks", 4097: "level3+1", 65_535: "level4-1",
    65_536: "level4", 65_537: "level4+1", 1_048_577: "level5+1", 2_097_152: "last-replayed-offsets",
    2_097_153: "first-scan-chunks", 4_200_000: "scan-chunks-9-tiles",
}
BIG = [n for n in SIZES if n > 65_537]
ZERO_RUNS = {"zrun16": 16, "zrun256": 256, "zrun2048": 2048, "zrun5000": 5000}


def zero_runs_of(family, n):
    """[(first, last)] of the zero runs a family plants (clipped to n)."""
    name = family.split("-")[0]
    if name in ZERO_RUNS:
        L = ZERO_RUNS[name]
        shift = 0 if family.endswith("-aligned") else 5
        return [(s, min(s + L, n) - 1) for s in range(shift, n, 2 * L)]
    if family == "head3000":
        return [(0, min(3000, n - 1) - 1)]
    if family == "tail3000":
        return [(max(n - 3000, 1), n - 1)]
    return []


def make_weights(family, n):
    rng = np.random.Generator(np.random.MT19937(1000 + n % 9973))
    w = rng.gamma(0.5, 1.0, n)
    if family == "gamma":
        pass
    elif family == "halfzero":
        w[rng.random(n) < 0.5] = 0.0
        if not w.any():
            w[n // 2] = 1.0
    elif family in ("one-first", "one-last", "one-middle"):
        w[:] = 0.0
        w[{"one-first": 0, "one-last": n - 1, "one-middle": n // 2}[family]] = 0.75
    elif family == "decades":
        w = 10.0 ** rng.uniform(-12.0, 0.0, n)
    elif family == "equal":
        w[:] = 1.0 / 3.0
    else:
        for a, b in zero_runs_of(family, n):
            w[a:b + 1] = 0.0
    assert w.any()
    return w


def _cases():
    out = []
    for n in SIZES:
        fams = ["gamma", "halfzero"]
        if n not in BIG:
            fams += ["one-first", "one-last", "one-middle", "decades", "equal"]
            for name, L in ZERO_RUNS.items():
                if n > L:
                    fams += [name + "-aligned", name + "-misaligned"]
            if n > 3000:
                fams += ["head3000", "tail3000"]
        out += [(f, n) for f in fams]
    return out


CASES = _cases()
SEARCH_CASES = [c for c in CASES if c[1] <= 65_537 or c[1] == 2_097_153]


def case_id(c):
    return f"{c[0]}-n{c[1]}-{SIZES[c[1]]}"


def cdf_error_bound(n):
    """In units of 2^-53 * total; derived in test_cdf_error_within_derived_bound's docstring."""
    chunks = -(-n // CHUNK)
    tiles = -(-chunks // BLOCK)
    offset = 0 if chunks == 1 else 16 + 17 * (tiles - 1) + 18
    return 46 + offset + 3


def reference_cdf(w):
    """np.cumsum in np.longdouble of the same f64 weights, rounded once at the end.  Run in blocks of 2048 with a cumsum of
    the blocks' totals, so that no entry is more than 2048 + n / 2048 longdouble additions deep: below 2^-52 of the total
    for every size here (a single run of 4.2M additions could be 2^-42 off in the worst case)."""
    n = len(w)
    pad = (-n) % CHUNK
    x = np.concatenate([w, np.zeros(pad)]).astype(np.longdouble).reshape(-1, CHUNK)
    inner = np.cumsum(x, axis=1)
    before = np.concatenate([[np.longdouble(0)], np.cumsum(inner[:, -1])[:-1]])
    return (inner + before[:, None]).reshape(-1)[:n].astype(np.float64)


@pytest.fixture(scope="module")
def big_filter():
    grid = rooms_grid(64, 1)
    f = Amcl(grid, MOTION, LF, AmclParams(min_particles=CAPACITY, max_particles=CAPACITY), seed=SEED)
    yield f
    f.close()


_last = {}


def _build(f, case):
    if _last.get("case") != case:
        family, n = case
        w = make_weights(family, n)
        f.set_particles(named_states(n), w)
        total = f.build_cdf()
        _last.clear()
        _last.update(case=case, family=family, n=n, w=w, total=total, cdf=read_cdf(f), f=f)
    return dict(_last)


@pytest.fixture(scope="module", params=CASES, ids=case_id)
def built(request, big_filter):
    return _build(big_filter, request.param)


@pytest.fixture(scope="module", params=SEARCH_CASES, ids=case_id)
def searched(request, big_filter):
    return _build(big_filter, request.param)


# ---- A. the CDF against a high-precision prefix sum -------------------------------------------------------
def test_cdf_error_within_derived_bound(built):
    """|cdf[i] - reference| <= cdf_error_bound(n) * 2^-53 * total.

    The bound counts f64 roundings on the way to an element, each worth at most 2^-53 of the total (all terms are
    non-negative partial sums of the weights, so every intermediate is <= total).  The order-enforcing max / min of
    chunk_cdf_ordered and chunk_bounds_tile are exact and pick values that are themselves scan results: they add nothing.
      in the chunk (chunk_cdf_ordered, shared by k_cdf and k_normalize_cdf): a thread's run of 8 items, 7 additions; the
      wave's shuffle scan of the thread totals, 6 more (13 for an inclusive total, which is also a wave sum's depth); the
      exclusive prefix of a thread, formed from the inclusive total and the thread's own, 13 + 7 + 1 = 21; the sums of up
      to three earlier waves onto the chunk's lower bound, 3 additions of values 13 deep; the thread's prefix onto that,
      1; the item onto the prefix, 1 of a value 7 deep: 3 + 13 + 21 + 1 + 7 + 1 = 46;
      the chunk's bounds (chunk_bounds_tile: replayed up to 4 * kBlock chunks, k_scan_chunk_bounds beyond; exact for one
      chunk): a chunk sum (k_chunk_sum's block reduction: 7 in the thread, 6 shuffles, 3 waves) 16; every tile of 256
      chunks before the element's own adds to the carry 2 additions of a wave prefix (6 + 3) and an inclusive total (6):
      17 a tile; in the element's tile the wave prefix 9, the inclusive value 6 and 2 additions, 17, counted as 18;
      the reference: 2 for its own additions (reference_cdf) and 1 for its final rounding.
    bound(n) = 46 + [16 + 17 * (tiles - 1) + 18 if more than one chunk] + 3: 49 for one chunk, 83 up to 524 288 particles
    (one tile), 117 at 1 048 577, 134 at 2 097 152 (4 tiles), 151 at 2 097 153, 219 at 4 200 000 (9 tiles).

    Measured on an MI355X, the largest error over the families of a size, same units (bound): n = 1, 2: 0 (49); 15: 1.6;
    16: 2.4; 17: 1.9; 255 .. 257: 2.1; 2047: 2.0; 2048: 1.9 (49); 2049: 2.0; 4096: 4.0; 4097: 2.0; 65 535: 5.1 (twelve decades);
    65 536: 3.4; 65 537: 3.5 (83); 1 048 577: 3.0 (117); 2 097 152: 3.0 (134); 2 097 153: 4.0 (151); 4 200 000: 6.0 (half
    zeros; 219).  Before the order was enforced the same errors were measured within 0.01 of these, with 76 006 decreasing steps in 59
    of the 190 cases and 152 460 zero-weight steps in 61 (test_cdf_is_non_decreasing, test_cdf_is_flat_over_zero_weight).
    """
    cdf, w, total, n = built["cdf"], built["w"], built["total"], built["n"]
    ref = reference_cdf(w)
    err = float(np.max(np.abs(cdf - ref))) / (U * total)
    print(f"CDFERR {case_id(built['case'])} err={err:.3f} bound={cdf_error_bound(n)}")
    assert err <= cdf_error_bound(n)


def test_total_is_the_last_entry(built):
    cdf, total = built["cdf"], built["total"]
    assert np.float64(total).view(np.uint64) == cdf[-1:].view(np.uint64)[0]


def test_cdf_is_non_decreasing(built):
    cdf = built["cdf"]
    down = np.flatnonzero(cdf[1:] < cdf[:-1]) + 1
    print(f"CDFDOWN {case_id(built['case'])} decreasing_steps={len(down)}")
    assert len(down) == 0, f"{len(down)} decreasing steps, first at {down[:5]}"


def test_cdf_is_flat_over_zero_weight(built):
    cdf, w = built["cdf"], built["w"]
    z = np.flatnonzero(w[1:] == 0.0) + 1
    bad = z[cdf[z] != cdf[z - 1]]
    print(f"CDFZERO {case_id(built['case'])} zero_weight_steps={len(bad)} of {len(z)}")
    assert len(bad) == 0, f"{len(bad)} zero-weight particles own an interval, first at {bad[:5]}"


def test_cdf_starts_at_the_first_weight(built):
    assert built["cdf"][0] == built["w"][0]


# ---- C. the search with chosen targets --------------------------------------------------------------------
def chosen_targets(case):
    family, n, cdf, total = case["family"], case["n"], case["cdf"], case["total"]
    idx = [0, 1, 14, 15, 16, 17, 255, 256, 2047, 2048, n - 2, n - 1]
    last_chunk = (n - 1) // CHUNK * CHUNK
    for base in {0, last_chunk}:  # every thread boundary of the first and of the last chunk
        for k in range(1, BLOCK + 1):
            idx += [base + 8 * k - 1, base + 8 * k]
    for a, b in zero_runs_of(family, n):
        idx += [a - 1, a, b, b + 1]
    rng = np.random.Generator(np.random.MT19937(77 + n))
    idx = np.unique(np.concatenate([np.array(idx, dtype=np.int64), rng.integers(0, n, 4096)]))
    idx = idx[(idx >= 0) & (idx < n)]
    v = cdf[idx]
    special = np.array([0.0, total, np.nextafter(total, np.inf), 2.0 * total, 5e-324])
    return np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), special])


def serve(f, targets):
    t = dev(targets)
    replies = torch.zeros((len(targets), 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.serve_requests(t.data_ptr(), len(targets), replies.data_ptr())
    f.sync()
    return replies.cpu().numpy()


def test_serve_requests_is_the_first_entry_at_least_the_target(searched):
    """The per-lane tree search (cdf_tree_lower_bound, k_gather_by_cdf_aos) against definition D, and no particle of weight
    zero for a target in (0, total].  A NaN target is "no request": a reply of zeros (k_gather_by_cdf_aos)."""
    f, cdf, w, total, n = searched["f"], searched["cdf"], searched["w"], searched["total"], searched["n"]
    targets = chosen_targets(searched)
    replies = serve(f, np.concatenate([targets, [np.nan]]))
    assert np.array_equal(replies[-1], np.zeros(4))
    replies = replies[:-1]
    assert np.all(replies[:, 2] == 1.0) and np.all(replies[:, 3] == 0.0) and np.all(replies[:, 1] == 0.0)
    got = replies[:, 0].astype(np.int64)
    want = first_at_least(cdf, targets)
    wrong = np.flatnonzero(got != want)
    print(f"SERVE {case_id(searched['case'])} targets={len(targets)} differ_from_D={len(wrong)}")
    assert len(wrong) == 0, f"{len(wrong)} of {len(targets)} targets, first: " + ", ".join(
        f"t={targets[k]!r} got {got[k]} want {want[k]}" for k in wrong[:4])
    inside = (targets > 0.0) & (targets <= total)
    zero_served = np.flatnonzero(inside & (w[got] == 0.0))
    print(f"SERVEZERO {case_id(searched['case'])} zero_weight_served={len(zero_served)}")
    assert len(zero_served) == 0, f"{len(zero_served)} targets in (0, total] served a particle of weight zero, first: " + ", ".join(
        f"t={targets[k]!r} -> {got[k]}" for k in zero_served[:4])


def oracle_uniforms(seed, step, count, first=0):
    return np.array([u53(orc.draw(seed, step, 2, first + j)) for j in range(count)])


STAGED_CASES = [(fam, n) for fam, n in CASES
                if n in (17, 257, 4097, 65_537) and (fam.startswith("zrun") or fam in ("head3000", "tail3000"))]


@pytest.mark.parametrize("case", STAGED_CASES + [("halfzero", 17), ("halfzero", 257)], ids=case_id)
def test_staged_search_agrees_with_definition_on_zero_runs(case):
    """k_resample_draw's search (LDS levels, wave_group_lower_bound's ballot count) cannot be handed targets: its targets
    are the oracle's uniforms times the device's own total, its CDF the device's own, and every output slot has to be the
    particle definition D names - through sample_particle_cloud and through resample.  Equality, no allowance."""
    family, n = case
    grid = rooms_grid(64, 1)
    f = Amcl(grid, MOTION, LF, AmclParams(min_particles=n, max_particles=n), seed=SEED)
    w = make_weights(family, n)
    f.set_particles(named_states(n), w)
    total = f.build_cdf()
    cdf = read_cdf(f)
    size, draw_id = 3001, 6
    cloud = f.sample_particle_cloud(size, draw_id)
    want = first_at_least(cdf, oracle_uniforms(SEED, 0x80000000 | draw_id, size) * total)
    assert np.array_equal(cloud[:, 2].astype(np.int64), want)
    assert f.resample(0.0, 4) == n
    got, gw = f.particles()
    u = oracle_uniforms(SEED, 4, n)
    anc = got[:, 2].astype(np.int64)
    assert np.array_equal(anc, first_at_least(cdf, u * total))
    assert np.all(w[anc[u > 0.0]] > 0.0)
    assert np.all(gw == 1.0)
    f.close()


# ---- B. zero weight at a size that takes the full launch shape ----------------------------------------------
def test_resample_full_launch_shape_with_half_the_weights_zero():
    """mcl_resample at n = 300 000 (1024-wide workgroups, the last one partial, upper levels in LDS) with a random half of the
    weights zero: every slot's ancestor is the one definition D names for u * total on the device's own CDF and total."""
    n, step = 300_000, 5
    grid = rooms_grid(64, 1)
    f = Amcl(grid, MOTION, LF, AmclParams(min_particles=n, max_particles=n), seed=SEED)
    rng = np.random.Generator(np.random.MT19937(9))
    w = rng.gamma(0.5, 1.0, n)
    w[rng.permutation(n)[: n // 2]] = 0.0
    f.set_particles(named_states(n), w)
    total = f.build_cdf()
    cdf = read_cdf(f)
    assert f.resample(0.0, step) == n
    assert np.array_equal(read_cdf(f), cdf)  # mcl_resample builds the same CDF from the weights as they are
    got, gw = f.particles()
    u = oracle_uniforms(SEED, step, n)
    want = first_at_least(cdf, u * total)
    anc = got[:, 2].astype(np.int64)
    wrong = np.flatnonzero(anc != want)
    print(f"RESAMPLE300K differ_from_D={len(wrong)} zero_weight_ancestors={int(np.sum(w[anc] == 0.0))}")
    assert len(wrong) == 0, f"{len(wrong)} slots, first {wrong[:5]}: got {anc[wrong[:5]]} want {want[wrong[:5]]}"
    assert np.all(w[anc[u > 0.0]] > 0.0)
    assert np.all(gw == 1.0)
    f.close()


# ---- D. targets, routing, commit and the KLD feed against numpy -------------------------------------------
KLD_MIN, KLD_MAX = 100, 120_000


@pytest.fixture(scope="module")
def shard():
    """One context and the oracle engine that restates its stage kernels (tests/shard_oracle_engine.py)."""
    grid = rooms_grid(64, 1)
    params = AmclParams(min_particles=KLD_MIN, max_particles=KLD_MAX)
    f = Amcl(grid, MOTION, LF, params, seed=SEED, shard_capacity=400_000)
    eng = OracleShardEngine(grid, MOTION, LF, params, SEED, 0, 400_000)
    yield f, eng
    f.close()


@pytest.mark.parametrize("p", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("first_slot", [0, 1, 2 ** 32 + 5])
@pytest.mark.parametrize("count", [1, 255, 256, 257, 2049, 100_003])
def test_resample_targets_are_the_oracles_uniforms_times_total(shard, count, first_slot, p):
    f, eng = shard
    total, step = 0.8125 * math.pi, 7
    if count > 3000 and first_slot == 1:
        count = 3000 + count % 7  # (the reference is a Python loop over the oracle's generator: the large count runs at slots 0 and 2^32 + 5)
    got = torch.zeros(count, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.resample_targets(step, p, total, first_slot, count, got.data_ptr())
    f.sync()
    want = torch.zeros(count, dtype=torch.float64)
    eng.resample_targets(step, p, total, first_slot, count, want)
    got, want = got.cpu().numpy(), want.numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))  # (NaN: the same quiet NaN on both sides, else bit for bit)
    if first_slot == 0:
        assert not np.isnan(got[0])  # random_intersperse.hpp:90-100: never the first element
    if p == 0.0:
        assert not np.isnan(got).any()
    if p == 1.0:
        assert np.isnan(got[1 if first_slot == 0 else 0:]).all()


def _route_case(world, count, rng):
    """Interval ends with an empty shard where the world allows it, and targets on an end, one ulp above it, above the last
    end, and NaN."""
    widths = rng.uniform(0.5, 2.0, world)
    if world >= 3:
        widths[1] = 0.0  # an empty shard: two equal ends
    if world >= 7:
        widths[world - 2] = 0.0
    ends = np.cumsum(widths)
    offsets = np.concatenate([[0.0], ends[:-1]])
    t = rng.uniform(0.0, ends[-1], count)
    special = np.concatenate([ends, np.nextafter(ends, np.inf), np.nextafter(ends, -np.inf), [0.0, 2.0 * ends[-1], np.nan, np.nan]])
    k = min(len(special), count)
    t[rng.permutation(count)[:k]] = special[:k]
    if count > 64:
        t[rng.permutation(count)[: count // 16]] = np.nan
    return t, ends, offsets


@pytest.mark.parametrize("world", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("count", [1, 2047, 2048, 2049, 300_001])
def test_route_targets_is_a_counting_sort_by_owner(shard, world, count):
    f, eng = shard
    rng = np.random.Generator(np.random.MT19937(world * 1000 + count % 1000))
    self_rank = world // 2
    t, ends, offsets = _route_case(world, count, rng)
    d_t, d_ends, d_off = dev(t), dev(ends), dev(offsets)
    send = torch.full((count,), -1.0, dtype=torch.float64, device="cuda")
    order = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((world,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    f.route_targets(d_t.data_ptr(), count, d_ends.data_ptr(), d_off.data_ptr(), world, self_rank, send.data_ptr(), order.data_ptr(),
                    counts.data_ptr())
    f.sync()
    send, order, counts = send.cpu().numpy(), order.cpu().numpy().astype(np.int64), counts.cpu().numpy()
    w_send, w_order, w_counts = eng.route_targets(torch.from_numpy(t), torch.from_numpy(ends), torch.from_numpy(offsets), self_rank)
    w_send, w_order, w_counts = w_send.numpy(), w_order.numpy().astype(np.int64), w_counts.numpy()
    # the reference itself, at the edges it has to get right: on an end -> the lower rank; one ulp above -> the next with room
    dest = np.empty(count, dtype=np.int64)
    dest[w_order] = np.repeat(np.arange(world), w_counts)
    for r in range(world):
        on = np.flatnonzero(t == ends[r])
        assert np.all(dest[on] <= r)
    assert np.array_equal(counts, w_counts)
    assert np.array_equal(np.sort(order), np.arange(count))
    begin = 0
    for r in range(world):
        seg = slice(begin, begin + int(w_counts[r]))
        by_slot, w_by_slot = np.argsort(order[seg]), np.argsort(w_order[seg])
        assert np.array_equal(order[seg][by_slot], w_order[seg][w_by_slot]), f"rank {r}: other slots"
        assert np.array_equal(send[seg][by_slot].view(np.uint64), w_send[seg][w_by_slot].view(np.uint64)), f"rank {r}: other local targets"
        begin += int(w_counts[r])
    assert np.all(send[np.isnan(t[order])] == 0.0)


def _serve_and_route(f, eng, n, count, first_slot, step, p):
    """A set of n named particles with zeros among the weights, `count` targets from the device, routed (world 1) and served."""
    rng = np.random.Generator(np.random.MT19937(n + count))
    w = rng.gamma(0.5, 1.0, n)
    w[rng.random(n) < 0.3] = 0.0
    states = named_states(n)
    states[:, 3] = rng.uniform(-1.0, 1.0, n)
    f.set_particles(states, w)
    total = f.build_cdf()
    cdf = read_cdf(f)
    eng.set_particles(states, w)
    eng.cdf = cdf  # (the search is held to the device's own CDF: part C; here the commit is the subject)
    targets = torch.zeros(count, dtype=torch.float64, device="cuda")
    send = torch.zeros(count, dtype=torch.float64, device="cuda")
    order = torch.zeros(count, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    replies = torch.zeros((count, 4), dtype=torch.float64, device="cuda")
    ends, offs = dev(np.array([total])), dev(np.array([0.0]))
    torch.cuda.synchronize()
    f.resample_targets(step, p, total, first_slot, count, targets.data_ptr())
    f.route_targets(targets.data_ptr(), count, ends.data_ptr(), offs.data_ptr(), 1, 0, send.data_ptr(), order.data_ptr(), counts.data_ptr())
    f.serve_requests(send.data_ptr(), count, replies.data_ptr())
    f.sync()
    assert int(counts.cpu()[0]) == count
    w_replies = eng.serve_requests(send.cpu())
    assert np.array_equal(replies.cpu().numpy(), w_replies.numpy())
    return targets, order, replies


@pytest.mark.parametrize("count,first_slot,p", [(1, 0, 0.0), (2049, 0, 0.25), (5000, 2 ** 32 + 5, 0.25), (777, 3, 1.0)])
def test_commit_routed_and_finish_candidates_place_every_reply(shard, count, first_slot, p):
    f, eng = shard
    step = 12
    targets, order, replies = _serve_and_route(f, eng, 6000, count, first_slot, step, p)
    t_h, o_h, r_h = targets.cpu(), order.cpu(), replies.cpu()
    want = eng._materialise(step, first_slot, count, r_h, o_h, t_h)
    hashes = np.array([orc.spatial_hash(s, eng.hash_res) for s in want], dtype=np.uint64)
    d_states = torch.zeros((count, 4), dtype=torch.float64, device="cuda")
    d_hashes = torch.zeros(count, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    f.finish_candidates(step, first_slot, count, replies.data_ptr(), order.data_ptr(), targets.data_ptr(), d_states.data_ptr(),
                        d_hashes.data_ptr())
    f.sync()
    assert f.num_particles() == 6000  # the live set is untouched
    injected = np.isnan(t_h.numpy())
    got = d_states.cpu().numpy()
    assert np.array_equal(got[~injected], want[~injected])
    np.testing.assert_allclose(got[injected], want[injected], rtol=1e-12, atol=1e-12)  # (libm's sincos of the random heading)
    assert np.array_equal(d_hashes.cpu().numpy().view(np.uint64), hashes)
    f.commit_routed(step, first_slot, count, replies.data_ptr(), order.data_ptr(), targets.data_ptr())
    f.sync()
    assert f.num_particles() == count
    s, w = f.particles()
    assert np.array_equal(s[~injected], want[~injected])
    np.testing.assert_allclose(s[injected], want[injected], rtol=1e-12, atol=1e-12)
    assert np.all(w == 1.0)


def _kld_stream(k, order, length):
    """`length` hashes over k distinct values: order "cycle" walks them round, "late" shows the last bins only at the end."""
    values = (np.arange(1, k + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    if order == "cycle":
        return values[np.arange(length) % k]
    seen = np.maximum(1, (np.arange(length) * k) // length + 1)  # bins open up one by one along the stream
    return values[np.arange(length) % seen]


@pytest.mark.parametrize("k,order", [(3, "cycle"), (40, "cycle"), (40, "late"), (4000, "cycle")])
@pytest.mark.parametrize("blocks", [(1, 2048, 2049, 50_000), (50_000, 1, 2049, 2048), (2049, 2049, 2049)])
def test_kld_feed_cuts_where_take_while_kld_does(shard, k, order, blocks):
    f, eng = shard
    stream = _kld_stream(k, order, sum(blocks))
    cut = orc.kld_take_while(stream, KLD_MIN, f.params.kld_epsilon, f.params.kld_z)
    f.kld_begin()
    at, got = 0, None
    for b in blocks:
        d = dev(stream[at:at + b].view(np.int64))
        torch.cuda.synchronize()
        got = f.kld_feed(d.data_ptr(), b)
        at += b
        if got is not None:
            break
    assert got == (None if cut >= len(stream) else int(cut))
    print(f"KLD k={k} {order} blocks={blocks} cut={cut} of {len(stream)}")


@pytest.mark.parametrize("where", ["first-of-block", "last-of-block", "never"])
def test_kld_feed_cut_on_a_block_edge(shard, where):
    """The same stream (k = 400 bins in a cycle) cut into blocks so that the first failing candidate is the first / the last of
    the second block; and a pass that never fails (every candidate in a bin of its own: the target grows with the stream)."""
    f, eng = shard
    if where == "never":
        stream = np.arange(1, 5001, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        assert orc.kld_take_while(stream, KLD_MIN, f.params.kld_epsilon, f.params.kld_z) >= len(stream)
        blocks = [2048, 2049, 903]
        want = None
    else:
        stream = _kld_stream(400, "cycle", 20_000)
        cut = int(orc.kld_take_while(stream, KLD_MIN, f.params.kld_epsilon, f.params.kld_z))
        assert 2100 < cut < len(stream) - 2100
        blocks = [cut, 2048] if where == "first-of-block" else [cut - 2047, 2048]
        want = cut
    f.kld_begin()
    at, got = 0, None
    for b in blocks:
        d = dev(stream[at:at + b].view(np.int64))
        torch.cuda.synchronize()
        got = f.kld_feed(d.data_ptr(), b)
        if got is not None:
            assert at <= got < at + b
            break
        at += b
    assert got == want


def test_load_shard_with_an_offset_then_propagate(shard):
    f, eng = shard
    n, offset, step = 5001, 2 ** 32 + 12_345, 3
    rng = np.random.Generator(np.random.MT19937(8))
    th = rng.uniform(-np.pi, np.pi, n)
    states = np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1)
    d = dev(states)
    torch.cuda.synchronize()
    f.load_shard(d.data_ptr(), n, offset)
    f.sync()
    s, w = f.particles()
    assert np.array_equal(s, states) and np.all(w == 1.0)
    pose, prev = orc.se2(0.4, 0.1, 0.2), orc.se2(0.1, 0.0, 0.05)
    f.propagate(pose, prev, step)
    got, _ = f.particles()
    want = orc.propagate(states, orc.diffdrive_sampler(pose, prev, MOTION_T), SEED, step, index_offset=offset)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13)  # (test_propagate_matches_oracle's)
    assert not np.allclose(got, orc.propagate(states, orc.diffdrive_sampler(pose, prev, MOTION_T), SEED, step, index_offset=0))
    f.load_shard(d.data_ptr(), n, 0)  # (the shared context goes back to offset 0)
    f.sync()
