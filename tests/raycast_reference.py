"""The written rule of mcl_cast_rays (include/beluga_mcl.h "Ray casting as a function"), from the pieces of tests/beam_reference.py - the
beam model's own walk, opened to caller-given poses and bearings.  Python ints for the walk, Python floats for what the reference computes
in doubles.  No device, nothing compiled, no oracle.

    T = grid_origin^-1 * pose                                                              (beam_reference.source_poses)
    source cell  = floor(T.x * (1 / resolution)), floor(T.y * (1 / resolution))            (beam_reference.cell_near)
    far end      = T * (c * max_range, s * max_range), each product and sum rounded on its own; its cell as above   (beam_reference.far_end)
    trace        = the standard Bresenham line from the source cell to the far-end cell; it stops at the first cell outside the grid (no hit),
                   not free (hit: unknown cells are not free) or past the end (no hit)     (beam_reference.cast)
    ranges       = fmin(distance of the two cells' centres, max_range), or max_range without a hit    (beam_reference.cell_distance)
    hit_cells    = y * W + x of the hit cell, or -1
    visited      = the cells looked at: those of the trace inside the grid up to and including the hit
    out of reach = a source cell at or beyond 2^30 in magnitude along an axis, or a line that spans 2^27 cells or more along an axis (only a
                   bearing or a rotation that is no unit vector gets there): no hit, no cell visited

The bearings are used as given: (c, s), never normalised.  bearings_of_points forms them from scan points as the beam model does, so that
ranges == beam_reference.reference(case)["expected"] for a case's own points and max_range.
"""
import math

import numpy as np

import beam_reference as ref

SOURCE_CELLS = 1 << 30
SPAN_CELLS = 1 << 27
MAX_REACH_CELLS = float((1 << 27) - 2)  # max_range / resolution at or above this is refused (kBeamMaxReachCells)

WALK_MUTANTS = ("trip_ge", "truncate", "divide", "past_the_end", "stop_early", "unknown_free", "outside_hit", "modified", "corners")


def bearings_of_points(points):
    """(px / z, py / z) per scan point, z = sqrt(px^2 + py^2): beam_reference.bearing_of."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return np.array([ref.bearing_of(float(px), float(py))[1:] for px, py in points], dtype=np.float64).reshape(-1, 2)


def bearings_of_angles(angles):
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def cast_rays(cells, resolution, origin, poses, bearings, max_range, mutant=None):
    """ranges [n, B], hit_cells [n, B] (int64, -1: no hit), visited [n, B], cells_visited (their sum)."""
    rule = ref.rule_of(mutant)
    cells = np.asarray(cells, dtype=np.int8)
    H, W = cells.shape
    res, max_range = float(resolution), float(max_range)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4)
    bearings = np.asarray(bearings, dtype=np.float64).reshape(-1, 2)
    n, B = len(poses), len(bearings)
    T = ref.source_poses(origin, poses) if n else np.zeros((0, 4))
    mask = ref.nonfree_mask(cells, rule)
    ranges = np.full((n, B), max_range)
    hit_cells = np.full((n, B), -1, dtype=np.int64)
    visited = np.zeros((n, B), dtype=np.int64)
    for i in range(n):
        Ti = [float(v) for v in T[i]]
        sx, sy = ref.cell_near(Ti[2], res, rule), ref.cell_near(Ti[3], res, rule)
        if abs(sx) >= SOURCE_CELLS or abs(sy) >= SOURCE_CELLS:
            continue
        for b in range(B):
            ex, ey = ref.far_end(Ti, float(bearings[b, 0]), float(bearings[b, 1]), max_range)
            fx, fy = ref.cell_near(ex, res, rule), ref.cell_near(ey, res, rule)
            if abs(fx - sx) >= SPAN_CELLS or abs(fy - sy) >= SPAN_CELLS:
                continue
            got, visited[i, b] = ref.cast(mask, W, H, sx, sy, fx, fy, rule)
            if got is not None:
                ranges[i, b] = ref.cell_distance(sx, sy, got[0], got[1], res, max_range, rule)
                hit_cells[i, b] = got[1] * W + got[0]
    return dict(ranges=ranges, hit_cells=hit_cells, visited=visited, cells_visited=int(visited.sum()))


def of_case(case, mutant=None, states=None, points=None):
    """cast_rays for a case of tests/beam_families.py: its grid, its states, the bearings of its points, its params' max_range."""
    return cast_rays(case["cells"], case["resolution"], case["origin"], case["states"] if states is None else states,
                     bearings_of_points(case["points"] if points is None else points), float(case["params"][6]), mutant)


def chunk_plan(n, B, chunk_rays):
    """[(first ray, rays, first pose, first bearing, poses touched, workgroups of 256)] of the flattened order i * B + b."""
    rays = n * B
    chunk_rays = min(max(chunk_rays, 64), 1 << 38)
    out = []
    for first in range(0, rays, chunk_rays):
        count = min(chunk_rays, rays - first)
        out.append((first, count, first // B, first % B, (first + count - 1) // B - first // B + 1, -(-count // 256)))
    return out
