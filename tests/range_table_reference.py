"""The written rule of the beam model's range table (include/beluga_mcl.h "Range table for the beam model"), from the pieces of
tests/beam_reference.py.  Python ints for the walk, IEEE doubles (one rounding per operation) for what the library computes in doubles,
extended precision for the mixture.  No device, nothing compiled, no oracle.

The table, all in the GRID frame: entry (x, y, k) of table[(y * W + x) * A + k] is the exact rule's cast
    source cell  = (x, y)
    far end      = ((x + 0.5) * resolution + c_k * max_range, (y + 0.5) * resolution + s_k * max_range), each product and sum rounded on
                   its own; its cell floor(v * (1 / resolution))                                       (beam_reference.cell_near)
    trace        = the standard Bresenham line between the two cells; it stops at the first cell outside the grid (no hit), not free
                   (hit) or past the end (no hit)                                                      (beam_reference.cast)
    entry        = (hx - x)^2 + (hy - y)^2, saturating at 0xFFFFFFFE; 0xFFFFFFFF without a hit
The bearings (c_k, s_k) are an INPUT: tests feed the ones the library used, so no libm difference enters the table.

The reweight over it.  Per pose: T = origin^-1 * pose (beam_reference.source_poses), its cell (sx, sy), theta = atan2(T.sin, T.cos).  Per
scan point: z = sqrt(px^2 + py^2), beta = atan2(py, px).  u = (theta + beta) * (A / (2 pi)), k = floor(u + 0.5) mod A.  The entry is the
table's at (sy * W + sx) * A + k for a source cell inside the grid, "no hit" outside.  expected = fmin(sqrt(r2) * resolution, max_range)
(beam_reference.table_distance), max_range without a hit; `z < expected` decided on that double - no tie re-derivation, the table knows
no hit cell -; the mixture is beam_reference.mixture.

MUTANTS restates the rule wrongly, one way at a time.
"""
import math

import numpy as np

import beam_reference as ref
from propagate_reference import to_f64

NO_HIT = 0xFFFFFFFF
FARTHEST = 0xFFFFFFFE

RULE = dict(bin_floor=False, row_stride=False, layout_bin_major=False, tie=False, world_cell=False, no_hit_zero=False)
MUTANTS = {
    "bin_floor": dict(bin_floor=True),                # the bin by floor(u) instead of floor(u + 0.5)
    "row_stride": dict(row_stride=True),              # the row of a cell A - 1 entries long
    "layout_bin_major": dict(layout_bin_major=True),  # the table read as [k * W * H + cell]
    "tie": dict(tie=True),                            # the exact path's tie re-derivation applied (it needs a hit cell: the table's own cast's)
    "world_cell": dict(world_cell=True),              # the source cell from the world-frame pose instead of the grid-frame one
    "no_hit_zero": dict(no_hit_zero=True),            # "no hit" read as r2 = 0
}


def rule_of(mutant=None):
    return dict(RULE, **(MUTANTS[mutant] if isinstance(mutant, str) else (mutant or {})))


def bearings_of(A):
    """cos, sin of k * (2 pi / A) by numpy: what the library's host-side table is compared with (within 1e-15), never fed into table()."""
    a = np.arange(A, dtype=np.float64) * (2.0 * math.pi / A)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def row(mask, W, H, x, y, resolution, max_range, bearings, hits=None):
    """The A entries of cell (x, y); hits (optional list) receives the hit cells or None."""
    out = np.empty(len(bearings), dtype=np.int64)
    for k, (c, s) in enumerate(bearings):
        ex = (float(x) + 0.5) * resolution + float(c) * max_range
        ey = (float(y) + 0.5) * resolution + float(s) * max_range
        fx, fy = ref.cell_near(ex, resolution), ref.cell_near(ey, resolution)
        got, _ = ref.cast(mask, W, H, x, y, fx, fy)
        out[k] = NO_HIT if got is None else min((got[0] - x) ** 2 + (got[1] - y) ** 2, FARTHEST)
        if hits is not None:
            hits.append(got)
    return out


def table(cells, resolution, max_range, bearings, only_cells=None):
    """The r2 array, int64 (H, W, A) - or, with only_cells (linear indices y * W + x), (len(only_cells), A)."""
    cells = np.asarray(cells, dtype=np.int8)
    H, W = cells.shape
    mask = ref.nonfree_mask(cells)
    bearings = np.asarray(bearings, dtype=np.float64).reshape(-1, 2)
    res, max_range = float(resolution), float(max_range)
    which = range(W * H) if only_cells is None else [int(c) for c in only_cells]
    out = np.array([row(mask, W, H, c % W, c // W, res, max_range, bearings) for c in which], dtype=np.int64).reshape(len(which), len(bearings))
    return out.reshape(H, W, len(bearings)) if only_cells is None else out


def bins(case, A, mutant=None, states=None):
    """Per pose the source cell [m, 2] and whether it is inside the grid; per (pose, beam) u, the bin k and `margin`: the distance of u
    from the nearest bin edge, in bins."""
    rule = rule_of(mutant)
    cells = np.asarray(case["cells"])
    H, W = cells.shape
    res = float(case["resolution"])
    world = np.asarray(case["states"] if states is None else states, dtype=np.float64).reshape(-1, 4)
    T = ref.source_poses(case["origin"], world)
    points = np.asarray(case["points"], dtype=np.float64).reshape(-1, 2)
    at = world if rule["world_cell"] else T
    source = np.array([[ref.cell_near(float(p[2]), res), ref.cell_near(float(p[3]), res)] for p in at], dtype=np.int64).reshape(-1, 2)
    inside = (source[:, 0] >= 0) & (source[:, 0] < W) & (source[:, 1] >= 0) & (source[:, 1] < H)
    theta = np.array([math.atan2(float(t[1]), float(t[0])) for t in T])
    beta = np.array([math.atan2(float(py), float(px)) for px, py in points])
    u = (theta[:, None] + beta[None, :]) * (A / (2.0 * math.pi))
    shifted = u if rule["bin_floor"] else u + 0.5
    k = np.floor(shifted).astype(np.int64) % A
    frac = (u + 0.5) - np.floor(u + 0.5)
    return dict(source=source, inside=inside, u=u, k=k, margin=np.minimum(frac, 1.0 - frac))


def weights(case, table_r2, A, mutant=None, states=None):
    """Per pose sum pz^3 over the case's points with the expected ranges read from table_r2 ((H, W, A) or flat, as the library lays it
    out), for a prior of 1, rounded once; with the bins, the entries and the margin of every (pose, beam) from the nearest bin edge."""
    rule = rule_of(mutant)
    cells = np.asarray(case["cells"])
    H, W = cells.shape
    res, params = float(case["resolution"]), tuple(float(v) for v in case["params"])
    max_range = params[6]
    flat = np.asarray(table_r2, dtype=np.int64).reshape(-1)
    assert flat.size == W * H * A
    b = bins(case, A, mutant, states)
    points = np.asarray(case["points"], dtype=np.float64).reshape(-1, 2)
    z = np.array([ref.bearing_of(float(px), float(py))[0] for px, py in points])
    m, B = b["k"].shape
    cell = b["source"][:, 1] * W + b["source"][:, 0]
    if rule["layout_bin_major"]:
        index = b["k"] * (W * H) + cell[:, None]
    else:
        index = cell[:, None] * ((A - 1) if rule["row_stride"] else A) + b["k"]
    index = np.where(b["inside"][:, None], index, 0)
    r2 = np.where(b["inside"][:, None], flat[np.clip(index, 0, flat.size - 1)], NO_HIT)
    hit = r2 != NO_HIT
    if rule["no_hit_zero"]:
        r2, hit = np.where(hit, r2, 0), np.ones_like(hit)
    expected = np.where(hit, np.minimum(np.sqrt(r2.astype(np.float64)) * res, max_range), max_range)
    decide = expected.copy()
    if rule["tie"]:  # the hit cell of the table's own cast, its centre distance where the measured range is within 1e-9 of the table's value
        mask = ref.nonfree_mask(cells)
        bearings_used = case["table_bearings"]
        for i, j in zip(*np.nonzero(hit & (np.abs(z[None, :] - expected) < 1e-9))):
            sx, sy = int(b["source"][i, 0]), int(b["source"][i, 1])
            hits = []
            row(mask, W, H, sx, sy, res, max_range, bearings_used[b["k"][i, j]:b["k"][i, j] + 1], hits)
            if hits[0] is not None:
                expected[i, j] = decide[i, j] = ref.cell_distance(sx, sy, hits[0][0], hits[0][1], res, max_range)
    short = z[None, :] < decide
    terms = ref.mixture(params, z, expected, short)
    w = to_f64(terms.sum(axis=1)) if B else np.zeros(m)
    return dict(b, r2=r2, expected=expected, short=short, weights=w)
