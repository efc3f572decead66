"""The NDT map build, the parts that need no GPU: the declarations of the new entries (include/beluga_mcl.h, capi.py, the C++ facade) and
NDTMap2d.from_points - the host route through mcl_ndt_measurement_cells - against the numpy restatement of detail::to_cells
(tests/ndt_reference.py) on hand-made clouds.  Keys and cell counts exactly; means and covariances within test_ndt_cpu.py's bounds for
the restatement (1e-12 / 1e-10 relative: numpy adds a cell's points in another order than the library's loop)."""
import os
import re

import numpy as np
import pytest

from beluga_amd import capi
from beluga_amd.amcl import Amcl, NDTMap2d, OccupancyGrid, occupied_cell_centres, se2_from_xytheta

import ndt_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mcl_build_ndt_map_from_points", "mcl_build_ndt_map_from_grid", "mcl_get_ndt_map")


def _spread(key, n, seed, resolution=1.0):
    """n points strictly inside the cell `key` of the truncation rule, on the side of the cell away from zero."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.uniform(0.1, 0.9, (n, 2))
    k = np.asarray(key, dtype=np.float64)
    return (np.where(k < 0, k - u, k + u)) * resolution


def hand_cases():
    """name -> (points, resolution, expected keys)."""
    cases = {}
    # a cell with exactly 4 points (dropped) between two with exactly 5 and 6
    cases["four_and_five"] = (np.concatenate([_spread((0, 0), 4, 1), _spread((2, 1), 5, 2), _spread((3, 3), 6, 3)]), 1.0, [(2, 1), (3, 3)])
    # negative coordinates: truncation toward zero puts (-1, 0) and (0, 1) into cell 0; key -1 covers (-2, -1]
    neg = np.array([[-0.9, 0.2], [-0.5, 0.3], [-0.1, 0.4], [0.3, -0.6], [0.7, -0.2], [-1.9, -1.2], [-1.7, -1.4], [-1.5, -1.6], [-1.3, -1.8],
                    [-1.1, -1.1], [-1.2, -1.5]])
    cases["negative"] = (neg, 1.0, [(-1, -1), (0, 0)])
    # points exactly on a cell's edge: x = 1.0 belongs to key 1, x = -1.0 to key -1, and at 0.5 m cells 1.5 / 0.5 = 3 exactly
    edge = np.array([[1.0, 0.1], [1.0, 0.3], [1.0, 0.5], [1.2, 0.7], [1.4, 0.9], [-1.0, 0.1], [-1.0, 0.3], [-1.3, 0.5], [-1.6, 0.7],
                     [-1.0, 0.9], [0.99, 0.5]])
    cases["edge"] = (edge, 1.0, [(-1, 0), (1, 0)])
    cases["edge_half"] = (np.array([[1.5, 0.0], [1.5, 0.1], [1.6, 0.2], [1.7, 0.3], [1.99, 0.4], [1.49, 0.2]]), 0.5, [(3, 0)])
    # collinear points: the variance across the line is 0 and is clamped to 1e-5; a slanted line keeps a singular covariance
    t = np.linspace(0.1, 0.9, 7)
    col = np.concatenate([np.stack([4.0 + t, np.full(7, 0.5)], 1), np.stack([np.full(7, 6.5), 2.0 + t], 1), np.stack([8.0 + t, 8.0 + t], 1)])
    cases["collinear"] = (col, 1.0, [(4, 0), (6, 2), (8, 8)])
    return cases


def combined_cloud():
    """All hand-made clouds at 1 m in one, shuffled (seeded), so that a cell's points are scattered through the input."""
    parts = [p + np.array([20.0 * i, 0.0]) * np.sign(p[:, :1] + 1e-300) for i, (p, r, _) in enumerate(hand_cases().values()) if r == 1.0]
    pts = np.concatenate(parts)
    return pts[np.random.Generator(np.random.PCG64(5)).permutation(len(pts))]


def test_new_entries_are_declared_consistently():
    header = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    facade = open(os.path.join(ROOT, "include", "beluga_amd", "amcl.hpp")).read()
    lib = capi.load()
    for name in NEW_ENTRIES:
        assert re.search(r"mcl_status\s+" + name + r"\(mcl_ctx\* ctx,", header), name
        assert name in capi.exported_names() and hasattr(lib, name), name
        assert name + "(" in facade, name
    assert capi._SIGNATURES["mcl_build_ndt_map_from_points"][1] == [capi._ctx, capi.c_double_p, capi.C.c_uint64, capi.C.c_double]
    assert len(capi._SIGNATURES["mcl_build_ndt_map_from_grid"][1]) == 7 and len(capi._SIGNATURES["mcl_get_ndt_map"][1]) == 6
    for method in ("build_ndt_map", "ndt_map"):
        assert callable(getattr(Amcl, method))


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_from_points_equals_the_restatement(name):
    pts, res, keys = hand_cases()[name]
    m = NDTMap2d.from_points(pts, res)
    wm, wc = ref.to_cells(pts, res)
    assert m.cells.dtype == np.int32 and [tuple(k) for k in m.cells] == keys
    assert len(m.means) == len(wm) == len(keys) and m.resolution == res
    np.testing.assert_allclose(m.means, wm, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(m.covariances, wc, rtol=1e-10, atol=1e-15)


def test_from_points_clamps_collinear_cells_and_keeps_input_order_out_of_it():
    pts, res, _ = hand_cases()["collinear"]
    m = NDTMap2d.from_points(pts, res)
    assert m.covariances[0][1, 1] == 1e-5 and m.covariances[1][0, 0] == 1e-5  # the clamp, exactly
    assert m.covariances[0][0, 0] > 1e-3 and m.covariances[2][0, 1] > 1e-3    # and nothing else is touched
    # the combined, shuffled cloud: every case's cells, in ascending key order
    c = NDTMap2d.from_points(combined_cloud(), 1.0)
    wm, wc = ref.to_cells(combined_cloud(), 1.0)
    assert len(c.cells) == len(wm) >= 8
    assert [tuple(k) for k in c.cells] == sorted(tuple(k) for k in c.cells)
    np.testing.assert_allclose(c.means, wm, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(c.covariances, wc, rtol=1e-10, atol=1e-15)


def test_from_occupancy_grid_fits_the_occupied_cells_centres():
    cells = np.zeros((40, 60), dtype=np.int8)
    cells[5, 3:50] = 100
    cells[5:35, 20] = 100
    cells[30, 10] = -1
    grid = OccupancyGrid(cells=cells, resolution=0.05, origin=se2_from_xytheta(-1.0, -0.7, 0.3))
    pts = occupied_cell_centres(grid)
    assert len(pts) == 47 + 30 - 1
    # row-major order, through the origin
    c, s = np.cos(0.3), np.sin(0.3)
    first = np.array([c * 3.5 * 0.05 - s * 5.5 * 0.05 - 1.0, s * 3.5 * 0.05 + c * 5.5 * 0.05 - 0.7])
    np.testing.assert_allclose(pts[0], first, rtol=1e-15)
    m = NDTMap2d.from_occupancy_grid(grid, 0.5)
    w = NDTMap2d.from_points(pts, 0.5)
    assert len(m.cells) > 3 and np.array_equal(m.cells, w.cells) and np.array_equal(m.means, w.means)
    assert np.array_equal(m.covariances, w.covariances)
