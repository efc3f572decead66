"""The written rule of the device-built likelihood field (option field_build = 1), in numpy.  No device, nothing
compiled, no oracle.

The rule, per cell c = (x, y) of a W x H grid of int8 values with traits (free, unknown, occupied):

    seeds        the occupied cells; with only_obstacle_boundaries only those occupied cells that have a FREE 4-neighbour inside the grid
                 (a neighbour that is unknown, or holds any other value, does not make an edge; the grid's border is no neighbour)
    n(c)         min over the seeds s of the integer (sx - x)^2 + (sy - y)^2                 - the exact squared distance, in cells
    A(c)         { metric(c, s) : s a seed with (sx - x)^2 + (sy - y)^2 == n(c) }            - the ADMISSIBLE set
    metric(c, s) ax = (x + 0.5) * resolution, bx = (sx + 0.5) * resolution, likewise ay, by, every operation one IEEE double rounding;
                 float32((ax - bx)^2 + (ay - by)^2)                                          - how the reference measures two cell centres
    cap          a member that is not < float32(max_obstacle_distance^2) becomes that value; a cell without a seed in reach holds it alone
    overlay      with model_unknown_space the set of an unknown cell - and, with only_obstacle_boundaries as well, of an occupied cell that
                 is no edge - is { min(cap value, float32(-2 sigma^2 log((1 / max_laser - z_random / max_laser) / amplitude))) }
    likelihood   float32(amplitude * exp(-float64(sq) / (2 sigma^2)) + z_random / max_laser), amplitude = z_hit / (sigma sqrt(2 pi))

Seeds that tie in n(c) - offsets (0, 5), (3, 4), (5, 0) - have the same distance on paper, and at a resolution that is no power of two
their float32 metric values can differ in the last bit: any of them is a right answer, which is why a cell has a set.

How n(c) is found here: a WINDOW MINIMUM over shifted copies of the seed mask.  The offsets (dx, dy) are visited in the order of
dx^2 + dy^2; a cell takes the first level at which a shifted seed covers it, and collects the metric value of every offset of that
level that does.  (The kernels split the transform into a column pass and a row pass; nothing of that is used here.)  Offsets farther
than max_obstacle_distance + one cell are not visited: whatever they reach is capped.
"""
import math
from collections import namedtuple

import numpy as np

ROS_TRAITS = (0, -1, 100)  # free, unknown, occupied

# what LikelihoodFieldModelParam's first five fields are
Params = namedtuple("Params", "max_obstacle_distance max_laser_distance z_hit z_random sigma_hit")
Admissible = namedtuple("Admissible", "squared likelihood cells2 seeds")
# squared, likelihood: (K, H, W) float32, NaN where a cell has fewer than K members; cells2: (H, W) int64 n(c), -1 without a seed in reach


def edge_mask(cells, traits=ROS_TRAITS):
    cells = np.asarray(cells)
    free, occupied = cells == traits[0], cells == traits[2]
    near = np.zeros(cells.shape, dtype=bool)
    near[:, :-1] |= free[:, 1:]
    near[:, 1:] |= free[:, :-1]
    near[:-1, :] |= free[1:, :]
    near[1:, :] |= free[:-1, :]
    return occupied & near


def seed_mask(cells, only_obstacle_boundaries=False, traits=ROS_TRAITS):
    return edge_mask(cells, traits) if only_obstacle_boundaries else np.asarray(cells) == traits[2]


def metric(x, y, sx, sy, resolution):
    """float32 squared distance between the centres of cells (x, y) and (sx, sy); numpy float64 arithmetic rounds once per operation."""
    res = np.float64(resolution)
    ax, ay = (np.asarray(x, dtype=np.float64) + 0.5) * res, (np.asarray(y, dtype=np.float64) + 0.5) * res
    bx, by = (np.asarray(sx, dtype=np.float64) + 0.5) * res, (np.asarray(sy, dtype=np.float64) + 0.5) * res
    dx, dy = ax - bx, ay - by
    return (dx * dx + dy * dy).astype(np.float32)


def cap_value(p):
    return np.float32(p.max_obstacle_distance * p.max_obstacle_distance)


def overlay_value(p):
    two_squared_sigma = 2 * p.sigma_hit * p.sigma_hit
    amplitude = p.z_hit / (p.sigma_hit * math.sqrt(2 * math.pi))
    offset = p.z_random / p.max_laser_distance
    background = np.float32(-two_squared_sigma * math.log((1 / p.max_laser_distance - offset) / amplitude))
    return min(cap_value(p), background)


def likelihood(squared, p):
    two_squared_sigma = 2 * p.sigma_hit * p.sigma_hit
    amplitude = p.z_hit / (p.sigma_hit * math.sqrt(2 * math.pi))
    offset = p.z_random / p.max_laser_distance
    with np.errstate(invalid="ignore"):
        return (amplitude * np.exp(-np.asarray(squared, dtype=np.float32).astype(np.float64) / two_squared_sigma) + offset).astype(np.float32)


def reach2(resolution, p):
    """Offsets with dx^2 + dy^2 above this are farther than max_obstacle_distance + one cell: capped, whatever the rounding."""
    return int(math.floor((p.max_obstacle_distance / resolution + 1.0) ** 2)) + 1


def nearest_seed_sets(seeds, resolution, limit2):
    """(cells2, members): n(c) (-1 where no seed lies within limit2) and the list of (H, W) float32 planes of the distinct metric values of
    the seeds that attain it (NaN where a cell has fewer)."""
    seeds = np.asarray(seeds, dtype=bool)
    H, W = seeds.shape
    cells2 = np.full((H, W), -1, dtype=np.int64)
    members = [np.full((H, W), np.nan, dtype=np.float32)]
    count = np.zeros((H, W), dtype=np.int64)
    if not seeds.any():
        return cells2, members
    r = math.isqrt(limit2)
    levels = {}
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
            if dx * dx + dy * dy <= limit2:
                levels.setdefault(dx * dx + dy * dy, []).append((dx, dy))
    for d2 in sorted(levels):
        undecided = cells2 < 0
        if not undecided.any():
            break
        for dx, dy in levels[d2]:
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            hit = seeds[y0 + dy:y1 + dy, x0 + dx:x1 + dx] & undecided[y0:y1, x0:x1]
            if not hit.any():
                continue
            ys, xs = np.nonzero(hit)
            ys += y0
            xs += x0
            cells2[ys, xs] = d2
            values = metric(xs, ys, xs + dx, ys + dy, resolution)
            fresh = np.ones(len(values), dtype=bool)
            for plane in members:
                fresh &= plane[ys, xs] != values
            ys, xs, values = ys[fresh], xs[fresh], values[fresh]
            slot = count[ys, xs]
            for k in np.unique(slot):
                while len(members) <= k:
                    members.append(np.full((H, W), np.nan, dtype=np.float32))
                at = slot == k
                members[k][ys[at], xs[at]] = values[at]
            count[ys, xs] += 1
    return cells2, members


def admissible(cells, resolution, p, model_unknown_space=False, only_obstacle_boundaries=False, traits=ROS_TRAITS):
    """The admissible squared distances and likelihoods of every cell (the module's docstring)."""
    cells = np.asarray(cells, dtype=np.int8)
    p = Params(*p)
    seeds = seed_mask(cells, only_obstacle_boundaries, traits)
    cells2, members = nearest_seed_sets(seeds, resolution, reach2(resolution, p))
    squared = np.stack(members)
    cap = cap_value(p)
    with np.errstate(invalid="ignore"):
        squared[~(squared < cap) & ~np.isnan(squared)] = cap
    squared[0][cells2 < 0] = cap
    if model_unknown_space:
        masked = cells == traits[1]
        if only_obstacle_boundaries:
            masked |= (cells == traits[2]) & ~edge_mask(cells, traits)
        squared[1:, masked] = np.nan
        squared[0, masked] = overlay_value(p)
    return Admissible(squared, likelihood(squared, p), cells2, seeds)


def ulps_between(a, b):
    """|a - b| in float32 steps, for positive finite float32 values (their bit patterns are ordered like the values)."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def ulps_off(field, adm):
    """(H, W) int64: how many float32 steps the field's value is away from the nearest admissible likelihood of its cell."""
    field = np.ascontiguousarray(field, dtype=np.float32)
    assert field.shape == adm.likelihood.shape[1:] and np.all(np.isfinite(field)) and np.all(field > 0)
    best = np.full(field.shape, np.iinfo(np.int64).max, dtype=np.int64)
    for plane in adm.likelihood:
        have = ~np.isnan(plane)
        d = ulps_between(field, np.where(have, plane, np.float32(1.0)))
        best = np.where(have, np.minimum(best, d), best)
    return best


def brute_force_cells2(seeds):
    """n(c) by comparing every cell with every seed (small maps only): the check of the window minimum."""
    seeds = np.asarray(seeds, dtype=bool)
    H, W = seeds.shape
    sy, sx = np.nonzero(seeds)
    out = np.full((H, W), -1, dtype=np.int64)
    if len(sx) == 0:
        return out
    for y in range(H):
        for x in range(W):
            out[y, x] = int(np.min((sx - x) ** 2 + (sy - y) ** 2))
    return out


def separation_ulps(p, resolution, W, H, model_unknown_space=False):
    """What a test with these parameters on a W x H grid can SEE: the least number of float32 steps between the likelihoods of two different
    squared cell distances below the cap (the cap's own likelihood among them), and - with the overlay - between the overlay's and the
    cap's.  Distances are taken at their nominal value float32(n * resolution^2)."""
    p = Params(*p)
    r = math.isqrt(reach2(resolution, p))
    a = np.arange(0, min(W - 1, r) + 1, dtype=np.int64)
    b = np.arange(0, min(H - 1, r) + 1, dtype=np.int64)
    n = np.unique((a[:, None] ** 2 + b[None, :] ** 2).ravel())
    sq = (n.astype(np.float64) * np.float64(resolution) * np.float64(resolution)).astype(np.float32)
    sq = np.unique(np.append(sq[sq < cap_value(p)], cap_value(p)))
    lik = np.sort(likelihood(sq, p))
    gaps = [int(np.min(ulps_between(lik[1:], lik[:-1])))] if len(lik) > 1 else []
    if model_unknown_space:
        gaps.append(int(ulps_between(likelihood(overlay_value(p), p), likelihood(cap_value(p), p)).ravel()[0]))
    return min(gaps) if gaps else None
