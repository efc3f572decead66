"""The cases of the device field build's edge suite (tests/test_gpu_field_build_edges.py), and what tests/test_field_build_reference_cpu.py
checks about them without a device: every case's parameters make every squared distance the case can hold VISIBLE in the float field
(field_build_reference.separation_ulps >= 64).  No case uses sigma_hit = 0.2: at that width the field cannot tell the larger distances apart.

kBlock = 256 columns per block of k_edt_field; R = ceil(max_obstacle_distance / resolution) + 1 is its halo and the column pass's cap.
"""
import math
from collections import namedtuple

import numpy as np

import field_build_reference as ref
from field_build_reference import Params, ROS_TRAITS

F, U, T = 0, -1, 100
K_BLOCK = 256
SEPARATION = 64  # float32 steps between any two values a case can hold

# max_obstacle_distance, max_laser_distance, z_hit, z_random, sigma_hit
WIDE = Params(2.0, 10.0, 0.5, 0.5, 1.0)       # the issue's set: 504 distinct distances on turtlebot3, the closest pair 4612 steps apart
NEAR = Params(1.0, 10.0, 0.5, 0.5, 1.0)       # R = 21 at 5 cm: the block-border sweep
OFF_GRID = Params(2.02, 10.0, 0.5, 0.5, 1.0)  # max / resolution no integer at 0.05 and 0.0625
OFF_HALF = Params(2.2, 10.0, 0.5, 0.5, 1.0)   # the same at 0.5
# 2 mm cells: neighbouring distances differ by 4e-6 m^2 all the way to the cap.  Without the z_random floor the likelihood is a pure
# exponential, whose RELATIVE step is d(sq) / (2 sigma^2) = 1.25e-5 everywhere: at least 105 float32 steps (a step is at most 1.19e-7).
FINE = Params(2.0, 10.0, 0.5, 0.0, 0.4)
# 1 mm cells and a cap of 1031 of them: the same reasoning, 1e-6 / (2 sigma^2) = 1.03e-5, at least 86 steps
TINY = Params(1.03, 10.0, 0.5, 0.0, 0.22)
PARAMETER_SETS = {"WIDE": WIDE, "NEAR": NEAR, "OFF_GRID": OFF_GRID, "OFF_HALF": OFF_HALF, "FINE": FINE, "TINY": TINY}

Case = namedtuple("Case", "name cells resolution params unknown edges traits on_device")


def case(name, cells, resolution, params, unknown=False, edges=False, traits=ROS_TRAITS, on_device=True):
    return Case(name, np.ascontiguousarray(cells, dtype=np.int8), float(resolution), params, bool(unknown), bool(edges), tuple(traits), on_device)


def reach(resolution, params):
    return int(math.ceil(params.max_obstacle_distance / resolution)) + 1


def grid_with(W, H, seeds, fill=F):
    cells = np.full((H, W), fill, dtype=np.int8)
    for x, y in seeds:
        cells[y, x] = T
    return cells


FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (model_unknown_space, only_obstacle_boundaries)


def flag_name(unknown, edges):
    return ("unknown" if unknown else "plain") + ("_edges" if edges else "")


# ---- widths and heights at the block edges -------------------------------------------------------------------------------------------------
BLOCK_WIDTHS = (1, 2, 255, 256, 257, 511, 513)
BLOCK_HEIGHTS = (1, 2, 3, 40)


def block_edge_cases(W, H):
    """Seeds in the corners; on the rim (first and last row and column); alone in column 255 and alone in column 256, so that the cells of
    the neighbouring block have nothing nearer than the seed across the border."""
    out = [case(f"block_{W}x{H}_corners", grid_with(W, H, [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]), 0.05, NEAR),
           case(f"block_{W}x{H}_rim", grid_with(W, H, [(W // 2, 0), (W // 3, H - 1), (0, H // 2), (W - 1, H // 3)]), 0.05, NEAR)]
    if W > K_BLOCK - 1:
        out.append(case(f"block_{W}x{H}_column255", grid_with(W, H, [(K_BLOCK - 1, H - 1)]), 0.05, NEAR))
    if W > K_BLOCK:
        out.append(case(f"block_{W}x{H}_column256", grid_with(W, H, [(K_BLOCK, 0)]), 0.05, NEAR))
    if W > 2 * K_BLOCK:
        out.append(case(f"block_{W}x{H}_column512", grid_with(W, H, [(2 * K_BLOCK, H // 2)]), 0.05, NEAR))
    return out


# ---- the cap -------------------------------------------------------------------------------------------------------------------------------
CAP_SETTINGS = [(0.05, WIDE), (0.05, OFF_GRID), (0.5, WIDE), (0.5, OFF_HALF), (0.0625, WIDE), (0.0625, OFF_GRID)]


def cap_cases(resolution, params):
    """One seed; cells at axis distance R - 2 ... R + 1 (and two more) along its row, its column and its diagonals, in the middle of a map and
    from a corner.  max / resolution an integer (WIDE: 40, 4, 32 cells - the strict `d < max^2` edge sits on a cell) and none."""
    R = reach(resolution, params)
    n = 2 * (R + 3) + 1
    name = f"cap_res{resolution}_max{params.max_obstacle_distance}"
    return [case(name + "_middle", grid_with(n, n, [(R + 3, R + 3)]), resolution, params),
            case(name + "_corner", grid_with(R + 4, R + 4, [(0, 0)]), resolution, params),
            case(name + "_far_corner", grid_with(R + 4, R + 4, [(R + 3, R + 3)]), resolution, params)]


# ---- a halo wider than a block -------------------------------------------------------------------------------------------------------------
def halo_cases():
    """2 mm cells, 2 m: R = 1001, four blocks of halo on either side."""
    one = grid_with(2100, 3, [(1050, 1)])
    two = grid_with(2100, 3, [(0, 0), (2099, 2)])  # the middle of the map is farther than the cap from both
    two[1, 40:60] = U
    two[2, 1040:1060] = U
    return [case("halo_one_seed", one, 0.002, FINE), case("halo_two_seeds", two, 0.002, FINE, unknown=True)]


# ---- ties ----------------------------------------------------------------------------------------------------------------------------------
# 25 * TIE_RES^2 lies half-way between two neighbouring float32 values (0.0625 and the next, to the last bit of the double): which of
# the two a tied seed's distance rounds to is decided by the rounding of its cell centres, and differs from seed to seed.
TIE_RES = 0.0500000014901161
TIE_CENTRES = [(290, 41), (30, 8), (150, 25), (254, 12), (260, 30)]  # (two of them next to the block border at column 256)
THREE_CENTRE = (250, 10)  # (a cell at which the three offsets (0, 5), (3, 4), (5, 0) alone round to two different values)
CIRCLE_25 = [(0, 5), (3, 4), (4, 3), (5, 0), (4, -3), (3, -4), (0, -5), (-3, -4), (-4, -3), (-5, 0), (-4, 3), (-3, 4)]


def tie_cases():
    """Twelve seeds on the circle dx^2 + dy^2 = 25 about a cell, far from the origin (where the rounding of the cell centres depends on the
    cell); the cells about the centre have two to twelve nearest seeds.  At TIE_RES the tied seeds' float32 distances differ in the last bit;
    0.0625 and 0.25 are dyadic - the tied values are equal there."""
    cx, cy = TIE_CENTRES[0]
    cells = grid_with(320, 50, [(x + dx, y + dy) for x, y in TIE_CENTRES for dx, dy in CIRCLE_25])
    out = [case(f"ties_res{res}", cells, res, WIDE) for res in (TIE_RES, 0.05, 0.3, 0.0625, 0.25)]
    cx, cy = THREE_CENTRE
    three = grid_with(320, 50, [(cx, cy + 5), (cx + 3, cy + 4), (cx + 5, cy)])  # the issue's three offsets alone
    return out + [case(f"ties_three_res{TIE_RES}", three, TIE_RES, WIDE), case("ties_three_res0.0625", three, 0.0625, WIDE)]


# ---- no seeds, all seeds -------------------------------------------------------------------------------------------------------------------
def no_seed_cases():
    free = np.full((5, 300), F, dtype=np.int8)
    unknown = free.copy()
    unknown[1:4, 100:280] = U
    out = []
    for u, e in FLAGS:
        out.append(case("no_seeds_all_free_" + flag_name(u, e), free, 0.05, WIDE, u, e))
        out.append(case("no_seeds_only_unknown_" + flag_name(u, e), unknown, 0.05, WIDE, u, e))
    return out


def all_occupied_cases():
    """With only_obstacle_boundaries no cell has a free neighbour: no edge, no seed - the cap everywhere, the overlay everywhere with
    model_unknown_space."""
    full = np.full((30, 270), T, dtype=np.int8)
    return [case("all_occupied_" + flag_name(u, e), full, 0.05, WIDE, u, e) for u, e in FLAGS]


# ---- the edge mask -------------------------------------------------------------------------------------------------------------------------
def edge_mask_map(free=F, unknown=U, occupied=T, other=50):
    c = np.full((48, 300), free, dtype=np.int8)
    c[0:7, 0:9] = occupied                    # thick, in the corner: its cells on the border have no neighbour outside
    c[20:29, 291:300] = occupied              # hollow, on the right border
    c[23:26, 294:297] = free
    c[41:48, 120:131] = occupied              # thick, on the bottom border
    c[10:18, 40:50] = unknown                 # occupied cells that see unknown space only: no edges
    c[12:16, 42:48] = occupied
    c[10:18, 70:80] = other                   # occupied cells that see a fourth value only: no edges
    c[12:16, 72:78] = occupied
    c[30:36, 250:258] = occupied              # a block whose only free neighbours lie to the LEFT (x - 1) ...
    c[29, 249:259] = unknown
    c[36, 249:259] = other
    c[29:37, 258] = unknown
    c[30:36, 200:208] = occupied              # ... to the RIGHT (x + 1) ...
    c[29, 199:209] = other
    c[36, 199:209] = unknown
    c[29:37, 199] = other
    c[30:36, 150:158] = occupied              # ... ABOVE (y - 1) ...
    c[29:37, 149] = unknown
    c[29:37, 158] = other
    c[36, 149:159] = unknown
    c[38:44, 20:28] = occupied                # ... and BELOW (y + 1)
    c[37:45, 19] = other
    c[37:45, 28] = unknown
    c[37, 19:29] = other
    c[20, 254:258] = occupied                 # across the block border at column 256, one cell thick
    c[3, 100] = other
    c[5, 101] = unknown
    return c


OTHER_TRAITS = (10, -7, 77)  # free, unknown, occupied - and the usual 0, -1, 100 then are "some other value"


def edge_mask_cases():
    out = []
    for u, e in FLAGS:
        out.append(case("edge_mask_" + flag_name(u, e), edge_mask_map(), 0.05, WIDE, u, e))
        c = edge_mask_map(*OTHER_TRAITS, other=T)
        c[46, 5:9] = F   # what the default traits call free, unknown and occupied: all of them "other" here
        c[46, 10:14] = U
        out.append(case("edge_mask_traits_" + flag_name(u, e), c, 0.05, WIDE, u, e, traits=OTHER_TRAITS))
    return out


# ---- random maps ---------------------------------------------------------------------------------------------------------------------------
def random_map(W, H, seed, occupied=0.03, unknown=0.10, other=0.01):
    rng = np.random.default_rng(seed)
    r = rng.random((H, W))
    c = np.full((H, W), F, dtype=np.int8)
    c[r < occupied] = T
    c[(r >= occupied) & (r < occupied + unknown)] = U
    c[(r >= occupied + unknown) & (r < occupied + unknown + other)] = 50
    return c


def random_cases():
    return [case("random_300x70_" + flag_name(u, e), random_map(300, 70, 1234 + k), 0.05, WIDE, u, e) for k, (u, e) in enumerate(FLAGS)]


# ---- the fallbacks -------------------------------------------------------------------------------------------------------------------------
def tall_map(H, seed=77):
    rng = np.random.default_rng(seed)
    c = np.full((H, 1), F, dtype=np.int8)
    c[rng.random(H) < 0.02, 0] = T
    c[rng.random(H) < 0.02, 0] = U
    c[0, 0] = c[H - 1, 0] = T
    c[1:40, 0] = F  # one stretch longer than the cap
    return c


def fallback_cases():
    """R = 1031 > 1024 cells, and a height the column offsets (16 bits) cannot hold: both build on the host, like option field_build = 0."""
    small = grid_with(8, 8, [(2, 5), (7, 0)])
    small[6, 6] = U
    return [case("fallback_cap_1031_cells", small, 0.001, TINY, unknown=True, on_device=False),
            case("fallback_height_32768", tall_map(32768), 0.5, WIDE, unknown=True, on_device=False)]


def tallest_case():
    return case("height_32767", tall_map(32767), 0.5, WIDE, unknown=True)


# ---- every way in --------------------------------------------------------------------------------------------------------------------------
def every_way_in_cases():
    """A larger map, a smaller one, the larger one again: what the first build left in the scratch planes lies under the second."""
    return [case("ways_in_large", random_map(300, 70, 99), 0.05, WIDE, True, False),
            case("ways_in_small", random_map(37, 11, 98, occupied=0.01), 0.05, WIDE, True, False)]


def families():
    """name -> list of cases, every case of the GPU suite."""
    out = {"block_edges": [c for W in BLOCK_WIDTHS for H in BLOCK_HEIGHTS for c in block_edge_cases(W, H)],
           "cap": [c for res, p in CAP_SETTINGS for c in cap_cases(res, p)],
           "halo": halo_cases(),
           "ties": tie_cases(),
           "no_seeds": no_seed_cases(),
           "all_occupied": all_occupied_cases(),
           "edge_mask": edge_mask_cases(),
           "random": random_cases(),
           "fallbacks": fallback_cases() + [tallest_case()],
           "every_way_in": every_way_in_cases()}
    names = [c.name for cs in out.values() for c in cs]
    assert len(names) == len(set(names))
    return out


_ADMISSIBLE = {}


def admissible_of(c):
    """The case's reference, computed once per process."""
    if c.name not in _ADMISSIBLE:
        _ADMISSIBLE[c.name] = ref.admissible(c.cells, c.resolution, c.params, c.unknown, c.edges, c.traits)
    return _ADMISSIBLE[c.name]


def check_field(field, adm, what):
    """THE check: every cell of the field within one float32 step of the likelihood of a member of its admissible set.  Returns the number of
    cells checked.  One step, derived: the device's double exp (and the multiply-add around it) differs from numpy's by a few double ulps,
    which can move the float32 rounding of the result by its last bit and no further."""
    off = ref.ulps_off(field, adm)
    bad = np.argwhere(off > 1)
    if len(bad):
        lines = [f"  cell (x={x}, y={y}): got {field[y, x]!r}, admissible {[float(v) for v in adm.likelihood[:, y, x] if not np.isnan(v)]} "
                 f"(squared {[float(v) for v in adm.squared[:, y, x] if not np.isnan(v)]}, n = {int(adm.cells2[y, x])}), {int(off[y, x])} steps off"
                 for y, x in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {field.size} cells are no admissible value\n" + "\n".join(lines))
    return int(field.size)
