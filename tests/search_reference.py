"""The global pose search's rule (include/beluga_mcl.h, "Global pose search"), restated in numpy and plain Python.

Candidate cells: the map's free cells (value == free_value, in ascending linear index: collect_free_cells) whose
  x % cell_stride == 0 and y % cell_stride == 0.
Headings: theta_h = -pi + h * (2 pi / headings), h < headings; one rotation per heading for every cell.
Position: the centre of the cell in the world, random_free_state's expressions operation by operation:
  lx = (x + 0.5) * resolution, ly = (y + 0.5) * resolution; gx = c * lx - s * ly, gy = s * lx + c * ly; + origin.
Candidate id: linear_cell_index * headings + h.
Pool: the first `pool` candidates by (score descending, id ascending); NaN is the lowest score.
Suppression: greedy in pool order; a candidate is dropped if a kept one lies within separation_cells of it (dx^2 + dy^2 <=
  separation_cells^2, integer cells) AND within separation_headings of it (min(|dh|, headings - |dh|)); stop after max_results kept.
Chunk plan: a chunk is a range of max(1, search_chunk // headings) cells of the free list, before the stride test.
"""
import math

import numpy as np


def candidate_cells(cells, free_value, cell_stride):
    """Linear indices (y * W + x) of the candidate cells, ascending."""
    grid = np.asarray(cells)
    H, W = grid.shape
    free = np.flatnonzero(grid.reshape(-1) == free_value)
    x, y = free % W, free // W
    return free[(x % cell_stride == 0) & (y % cell_stride == 0)].astype(np.uint64)


def candidate_ids(cell_indices, headings):
    """Ids of every candidate, in id order: cell-major, heading-minor."""
    return (np.asarray(cell_indices, dtype=np.uint64)[:, None] * np.uint64(headings) + np.arange(headings, dtype=np.uint64)[None, :]).reshape(-1)


def heading_angles(headings):
    return np.array([-math.pi + h * (2.0 * math.pi / headings) for h in range(headings)])


def cell_positions(cell_indices, width, resolution, origin):
    """World positions of the cells' centres; origin = (cos, sin, x, y)."""
    idx = np.asarray(cell_indices, dtype=np.int64)
    c, s, ox, oy = (np.float64(v) for v in origin)
    lx = ((idx % width).astype(np.float64) + 0.5) * np.float64(resolution)
    ly = ((idx // width).astype(np.float64) + 0.5) * np.float64(resolution)
    gx = c * lx - s * ly
    gy = s * lx + c * ly
    return gx + ox, gy + oy


def pool_order(ids, scores, pool):
    """Indices of the first `pool` candidates by (score descending, id ascending); NaN lowest."""
    scores = np.asarray(scores, dtype=np.float64)
    key = np.where(np.isnan(scores), -np.inf, scores)
    nan_last = np.isnan(scores).astype(np.int8)  # (-inf itself ranks above NaN)
    order = np.lexsort((np.asarray(ids, dtype=np.uint64), -key, nan_last))
    return order[:pool]


def suppress(pool_cells, pool_headings, width, headings, separation_cells, separation_headings, max_results):
    """Indices into the pool of the kept candidates."""
    kept = []
    for i, (cell, h) in enumerate(zip(pool_cells, pool_headings)):
        if len(kept) >= max_results:
            break
        x, y, h = int(cell) % width, int(cell) // width, int(h)
        near = False
        for k in kept:
            kx, ky, kh = int(pool_cells[k]) % width, int(pool_cells[k]) // width, int(pool_headings[k])
            dh = abs(h - kh)
            if (x - kx) ** 2 + (y - ky) ** 2 <= separation_cells ** 2 and min(dh, headings - dh) <= separation_headings:
                near = True
                break
        if not near:
            kept.append(i)
    return kept


def chunk_plan(free_cells, headings, search_chunk):
    """(cells per chunk, chunks) for a free list of `free_cells` entries."""
    per = max(1, min(max(search_chunk, 64), 1 << 22) // headings)
    return per, (free_cells + per - 1) // per
