"""Inputs shared by tests/test_beam_reference_cpu.py and tests/test_gpu_beam_edges.py: maps, poses and scans ENGINEERED to sit where the beam
kernels' closed forms (csrc/beam_kernels.hip: walk_room / floor_div, walk_blocks' three phases, the LDS window and its sectors, the free-ahead
certificate, the range table and its tie rule) can go wrong.  Deterministic; no device.

A family is a function returning a list of cases; a case is a dict
    cells (H, W) int8, resolution, origin (cos, sin, x, y), states [m, 4] (world frame), points [B, 2], params (z_hit, z_short, z_max,
    z_rand, sigma_hit, lambda_short, max_range), targets: what the case is for,
    majority (optional): the first `majority` states share one cell and are what a set is filled with - the others appear once each, so
    that the ordered kernel's middle particle, and with it its window, is known (see `assignment`),
    plus whatever the family's own claims need (tests/test_beam_reference_cpu.py asserts them).
Every case has a few to a few thousand rays and at most ~2e6 cells of reference work, so that its count of visited cells localises a fault.
Rays are engineered by placing poses in the grid frame (the origin's inverse is applied by the reference in its own arithmetic, so what a
case claims is always asserted on what beam_reference computes, never assumed from the construction).
"""
import functools
import math

import numpy as np

import beam_reference as ref
import lf_reference as lfref

RES = 0.05
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])
ROTATED = np.array([np.cos(0.7), np.sin(0.7), 3.0, -2.0])  # lf_families.GRID_A's origin


def local_pose(origin, cx, cy, theta, resolution=RES):
    """The world pose whose grid-frame position is (cx, cy) cells and whose grid-frame heading is theta."""
    return lfref.pose_mul(origin, np.array([[np.cos(theta), np.sin(theta), cx * resolution, cy * resolution]]))[0]


def scan(angles, ranges):
    a, r = np.asarray(angles, dtype=np.float64), np.asarray(ranges, dtype=np.float64)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def spread_ranges(count, max_range, lo=0.12, hi=0.9):
    """Measured ranges over (lo, hi) * max_range: many below the expected range of their ray (the short-return term then feels it)."""
    return max_range * (lo + (hi - lo) * ((np.arange(count) * 0.6180339887498949) % 1.0))


def salt(H, W, k=101):
    yy, xx = np.mgrid[0:H, 0:W]
    cells = np.zeros((H, W), dtype=np.int8)
    cells[(7 * xx + 13 * yy) % k == 0] = ref.OCCUPIED
    cells[(5 * xx + 3 * yy) % (2 * k + 1) == 0] = ref.UNKNOWN
    return cells


def _case(cells, states, points, max_range, targets, origin=IDENTITY, resolution=RES, params=None, **more):
    return dict(cells=np.ascontiguousarray(cells, dtype=np.int8), resolution=resolution, origin=np.asarray(origin, dtype=np.float64),
                states=np.asarray(states, dtype=np.float64).reshape(-1, 4), points=np.asarray(points, dtype=np.float64).reshape(-1, 2),
                params=params or ref.revealing_params(resolution, max_range), targets=targets, **more)


def assignment(case, n, offset=0):
    """Which state each of n particles gets: the states in turn from `offset` on - or, with `majority`, the majority states in turn and
    every other state once (at positions 1, 3, 5, ...), so that a workgroup's middle particle of the spatial order is a majority state."""
    m = len(case["states"])
    k = case.get("majority", m)
    idx = (np.arange(n) + offset) % k
    for j in range(m - k):
        if 2 * j + 1 < n:
            idx[2 * j + 1] = k + j
    return idx


# ---- slopes ---------------------------------------------------------------------------------------------------------------------------
SLOPE_REACHES = (0.4, 1.5, 3.0, 5.0, 8.0, 12.0, 14.0, 17.0, 23.0, 25.0, 63.0, 65.0)  # cells: major spans 0, 1, .. 17, 23 .. 25, 63 .. 65 between them


@functools.lru_cache(maxsize=None)
def slopes():
    """Every octant, axis-aligned and exactly diagonal rays, far end = source, major span = minor span + 1, lengths 1 .. 17 and 8 m - 1,
    8 m, 8 m + 1, from sources at every (sx & 7, sy & 7): walk_blocks' phase 1 / 2 / 3 seams, for both step signs."""
    out = []
    cells = salt(157, 203)
    for reach in SLOPE_REACHES:
        states = [local_pose(IDENTITY, 40.5 + i, 48.5 + j, 0.0) for j in range(8) for i in range(8)]
        d = max(1, int(round(reach / math.sqrt(2.0))))
        base = [(1.0, 0.0), (1.0, 1.0), (d + 1.0, float(d)), (float(d), d - 1.0)] + [(math.cos(t), math.sin(t)) for t in (0.13, 0.31, 0.52, 0.71)]
        dirs = []
        for a, b in base:
            for u, v in ((a, b), (b, a)):
                for su in (1.0, -1.0):
                    for sv in (1.0, -1.0):
                        if (su * u, sv * v) not in dirs:
                            dirs.append((su * u, sv * v))
        r = spread_ranges(len(dirs), reach * RES)
        points = [(rb * u / math.hypot(u, v), rb * v / math.hypot(u, v)) for rb, (u, v) in zip(r, dirs)]
        out.append(_case(cells, states, points, reach * RES, "slopes, reach %.1f cells" % reach))
    # The cell one past the end NEARER than max_range (from a source at its cell's centre it never is, and fmin hides it): sources in the low
    # corner of their cell, far ends just below the next cell on both axes - (16.97, 5.97) cells away, far-end cell (+16, +5), the line's next
    # cell (+17, +5) at 17.72 cells < 17.99 - and a non-free cell exactly there.
    cells = np.zeros((157, 203), dtype=np.int8)
    states = [local_pose(IDENTITY, 40.01 + 3 * i, 48.01 + 9 * i, 0.0) for i in range(4)]
    for i in range(4):
        cells[48 + 9 * i + 5, 40 + 3 * i + 17] = ref.OCCUPIED
    reach = math.hypot(16.97, 5.97)
    points = [(0.9 * 16.97 * RES, 0.9 * 5.97 * RES), (0.5 * reach * RES, 0.0)]
    out.append(_case(cells, states, points, reach * RES, "a non-free cell one past the end, nearer than max_range", past_end=True))
    return out


# ---- obstacle_at_k --------------------------------------------------------------------------------------------------------------------
TILE = 64  # a multiple of 32: every tile repeats the line at the same phase of the 8-cell blocks and the 32-cell words
OBSTACLE_LINES = ((17, 17, 0.0), (17, 17, math.pi / 4), (17, 19, 0.32), (19, 17, 1.2), (47, 17, 2.5), (47, 47, math.pi + 0.41),
                  (17, 47, -1.1), (20, 46, -0.2))


@functools.lru_cache(maxsize=None)
def obstacle_at_k():
    """Per line (one per octant, 30 cells long) one map of tiles: tile k holds a single non-free cell at index k of the line's trace, for
    every k from 0 (the source cell: range 0) to the last; then tiles with the cell one past the end (no hit), with cells beside the trace
    only, and with two cells touching at a corner the ray passes between.  Beam 0 is the line; four more beams fan around it."""
    out = []
    reach = 30.0
    for sx, sy, theta in OBSTACLE_LINES:
        fx, fy = math.floor(sx + 0.5 + reach * math.cos(theta)), math.floor(sy + 0.5 + reach * math.sin(theta))
        trace = list(ref.line(sx, sy, fx, fy, extra_cells=1))
        on, past = trace[:-1], trace[-1]
        beside = [(x + dx, y + dy) for (x, y) in on[2::5] for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0)) if (x + dx, y + dy) not in on]
        corner = None
        for (x0, y0), (x1, y1) in zip(on[3:], on[4:]):
            if x1 != x0 and y1 != y0:
                corner = [(x1, y0), (x0, y1)]
                break
        tiles = [[c] for c in on] + [[past], beside] + ([corner] if corner else [])
        per_row = 6
        rows = -(-len(tiles) // per_row)
        cells = np.zeros((rows * TILE, per_row * TILE), dtype=np.int8)
        states, kinds = [], []
        for t, obstacles in enumerate(tiles):
            ox, oy = (t % per_row) * TILE, (t // per_row) * TILE
            for k, (x, y) in enumerate(obstacles):
                cells[oy + y, ox + x] = ref.UNKNOWN if (t + k) % 3 == 2 else ref.OCCUPIED
            states.append(local_pose(IDENTITY, ox + sx + 0.5, oy + sy + 0.5, 0.0))
            kinds.append(t if t < len(on) else ("past", "beside", "corner")[t - len(on)])
        angles = [theta, theta + 0.05, theta - 0.05, theta + 0.4, theta - 0.4]
        points = scan(angles, spread_ranges(5, reach * RES, 0.5, 0.95))
        out.append(_case(cells, states, points, reach * RES, "one non-free cell at every index of a line towards %.2f rad" % theta,
                         kinds=kinds, trace=on, tile=(per_row, TILE)))
    return out


# ---- borders_and_tiny_grids ------------------------------------------------------------------------------------------------------------
TINY_GRIDS = ((1, 1), (1, 7), (7, 1), (8, 8), (9, 33), (31, 33), (157, 203))  # W x H


def _fan(count, max_range, phase=0.0):
    return scan(phase + 2 * np.pi * np.arange(count) / count, spread_ranges(count, max_range))


@functools.lru_cache(maxsize=None)
def borders_and_tiny_grids():
    """Grids below, at and astride one 8 x 8 block and one 32-cell word; sources in corner and border cells, one cell outside (-1 and W)
    and far outside (empty traces); exits through every side and exactly through a corner; far ends far outside; negative coordinates;
    an unknown frame around free space; a rotated origin."""
    out = []
    for W, H in TINY_GRIDS:
        for variant in ("free", "frame"):
            if variant == "frame" and min(W, H) < 7:
                continue
            origin = ROTATED if (W, H) == (157, 203) else IDENTITY
            cells = np.zeros((H, W), dtype=np.int8)
            if variant == "frame":
                cells[:] = ref.UNKNOWN
                cells[2:-2, 2:-2] = ref.FREE
                cells[H // 2, W // 2] = ref.OCCUPIED
            elif W * H > 64:
                cells[salt(H, W, 53) == ref.OCCUPIED] = ref.OCCUPIED
            reach = 3.0 * max(W, H) + 3.0 if variant == "free" else max(W, H) + 3.0
            spots = [(0.5, 0.5), (W - 0.5, 0.5), (0.5, H - 0.5), (W - 0.5, H - 0.5), (W / 2.0, 0.3), (0.3, H / 2.0), (W - 0.3, H / 2.0),
                     (W / 2.0, H - 0.3), (-0.5, 0.5), (W + 0.5, H - 0.5), (0.5, -0.5), (W - 0.5, H + 0.5), (-0.5, -0.5), (-50.5, H / 2.0),
                     (W / 2.0, H + 70.5), (W / 2.0 + 0.1, H / 2.0 + 0.2)]
            states = [local_pose(origin, x, y, 0.0) for x, y in spots]
            points = np.concatenate([_fan(24, reach * RES, 0.02), scan([math.pi / 4, 3 * math.pi / 4, -3 * math.pi / 4, -math.pi / 4, 0.0,
                                                                         math.pi / 2, math.pi, -math.pi / 2], spread_ranges(8, reach * RES))])
            out.append(_case(cells, states, points, reach * RES, "a %d x %d grid, %s" % (W, H, variant), origin=origin, size=(W, H)))
    return out


# ---- cell_boundaries -------------------------------------------------------------------------------------------------------------------
def _ulp_steps(x, k):
    return (np.array([x], dtype=np.float64).view(np.int64)[0] + np.asarray(k, dtype=np.int64)).view(np.float64)


def _straddle(value_of, x0, k, span=96):
    """Doubles next to x0 whose value_of(x) (cells) is the largest below k, equal to k where there is one, and the smallest above k."""
    xs = _ulp_steps(x0, np.arange(-span, span + 1)) if x0 != 0.0 else np.array([-(2.0 ** -60), -5e-324, 0.0, 5e-324, 2.0 ** -60])
    vs = np.array([value_of(float(x)) for x in xs])
    picks = []
    if (vs < k).any():
        picks.append(("below", float(xs[vs < k][np.argmax(vs[vs < k])])))
    if (vs == k).any():
        picks.append(("at", float(xs[vs == k][0])))
    if (vs > k).any():
        picks.append(("above", float(xs[vs > k][np.argmin(vs[vs > k])])))
    return picks


@functools.lru_cache(maxsize=None)
def cell_boundaries():
    """Source positions, and far ends, on a cell boundary and the nearest doubles either side - boundaries 0 (where floor and truncation
    part), 8, 32, 33 and W - on x and on y, behind an identity and a rotated origin (lf_families.engineer's approach: solve, then search
    the neighbouring doubles by the reference's own arithmetic)."""
    out = []
    W, H = 203, 157
    cells = salt(H, W, 67)
    reach = 20.5  # cells: with the far end on a boundary the source sits mid-cell, and the other way round
    for origin in (IDENTITY, ROTATED):
        inv_origin = lfref.pose_inverse(origin)

        def grid_x(wx, wy, axis):
            T = lfref.pose_mul(inv_origin, np.array([[1.0, 0.0, wx, wy]]))[0]
            return float(T[2 + axis]) * (1.0 / RES)

        states, marks = [], []
        for axis in (0, 1):
            side = (W, H)[axis]
            for k in (0, 8, 32, 33, side):
                for what, shift in (("source", 0.0), ("far", -reach)):
                    c = [60.4, 70.6]
                    c[axis] = k + shift
                    if not -1.0 < c[axis] < side + 1.0:
                        continue
                    w0 = local_pose(origin, c[0], c[1], 0.0)
                    # move the world coordinate that moves this grid axis most
                    coord = 2 + (axis if abs(origin[0]) >= abs(origin[1]) else 1 - axis)

                    def value_of(x, w0=w0, coord=coord, axis=axis, shift=shift):
                        w = w0.copy()
                        w[coord] = x
                        if shift == 0.0:
                            return grid_x(w[2], w[3], axis)
                        T = lfref.pose_mul(inv_origin, w[None, :])[0]
                        ex, ey = ref.far_end([float(v) for v in T], *((1.0, 0.0) if axis == 0 else (0.0, 1.0)), reach * RES)
                        return (ex, ey)[axis] * (1.0 / RES)

                    for side_name, x in _straddle(value_of, float(w0[coord]), k):
                        w = w0.copy()
                        w[coord] = x
                        marks.append((len(states), axis, k, what, side_name))
                        states.append(w)
        # the far ends above are those of the beams along +x and +y of a pose with the grid's heading
        points = np.concatenate([np.array([[0.7 * reach * RES, 0.0], [0.0, 0.6 * reach * RES]]), _fan(14, reach * RES, 0.11)])
        out.append(_case(cells, states, points, reach * RES, "sources and far ends on cell boundaries", origin=origin, marks=marks, reach=reach))
    return out


# ---- closed_form_thresholds ------------------------------------------------------------------------------------------------------------
POW = 0.0625  # a resolution whose reciprocal is exact: spans of millions of cells are engineered exactly


def floor_div_range(num):
    return 0 if num < (1 << 22) else 1 if num < (1 << 32) else 2


def exit_numerator(sx, sy, fx, fy, W, H):
    """walk_room_in_grid's floor_div numerator for the ray (None: dminor = 0 or the source is outside): (room_minor + 1) dmajor - span."""
    xs, ys = abs(fx - sx), abs(fy - sy)
    steep = xs < ys
    span, minor = (ys, xs) if steep else (xs, ys)
    if minor == 0 or not (0 <= sx < W and 0 <= sy < H):
        return None
    pos, size, step = (sx, W, fx - sx) if steep else (sy, H, fy - sy)
    room = size - 1 - pos if step > 0 else pos
    return (room + 1) * 2 * span - span


def trips_numerator(sx, sy, fx, fy, k):
    """walk_trips_at's floor_div numerator at cell k of the ray (walk_seek: every hit, every window exit): span + k dminor + dmajor - 1."""
    xs, ys = abs(fx - sx), abs(fy - sy)
    span, minor = max(xs, ys), min(xs, ys)
    return span + k * 2 * minor + 2 * span - 1


# (span of the rays, cells from the minor-side border they head for, what is reached)
THRESHOLD_SPANS = (((1 << 22) - 1, 0, "2^22 - 1"), (1 << 22, 0, "2^22"), ((1 << 22) + 1, 0, "2^22 + 1"),
                   (130150524, 16, "2^32 - 4"), (130150525, 16, "2^32 + 29"), (32767, 2, "closed forms on"), (32768, 2, "closed forms off"))
THRESHOLD_STARTS = (39000, 39700, 20000, 100)


@functools.lru_cache(maxsize=None)
def closed_form_thresholds():
    """floor_div's three ranges: walk_room's numerators 2^22 - 1, 2^22, 2^22 + 1 and 2^32 - 4, 2^32 + 29 ((2 room + 1) * span = 33 span: 2^32
    itself is no multiple of an odd number, and spans stay below the library's 2^27 - 2 cells) on thin long grids, along x and along y;
    a third beam 0.3 rad off the line climbs into a strip of non-free cells in the far border row, so that walk_trips_at's numerator
    span + k dminor + dmajor - 1 of its hit lands in each range as well; major spans 32 767 / 32 768; a single non-free cell in an empty
    map passed at block distances 0, 1, 2, 3, 16, 17 by rays of every remaining length (skips cut short by `room`)."""
    out = []
    for steep in (False, True):
        L, T_ = 40000, 24
        W, H = (T_, L) if steep else (L, T_)
        cells = np.zeros((H, W), dtype=np.int8)
        along = np.arange(L)
        for row in range(T_):
            hits = (along % 7919 == 13 * row + 5) | ((along % 9973 == 40 * row + 1) & (row % 2 == 0))
            if steep:
                cells[hits, row] = ref.OCCUPIED
            else:
                cells[row, hits] = ref.OCCUPIED
        for start in THRESHOLD_STARTS[2:]:  # the strips the third beam of the last two poses climbs into (cell 1 of a ray from that row)
            if steep:
                cells[start + 1:start + 70, T_ - 1] = ref.OCCUPIED
            else:
                cells[T_ - 1, start + 1:start + 70] = ref.OCCUPIED
        for span, room, what in THRESHOLD_SPANS:
            reach = float(span + 2)  # cells: cos = span / reach puts the far end `span` cells along and thousands of cells across
            states = []
            for start in (s_ + 0.5 for s_ in THRESHOLD_STARTS):
                row = T_ - 1 - room + 0.5
                theta = math.acos(span / reach)
                if steep:
                    states.append(local_pose(IDENTITY, row, start, math.pi / 2 - theta, POW))
                else:
                    states.append(local_pose(IDENTITY, start, row, theta, POW))
            off = -0.3 if steep else 0.3  # (towards the far border row either way)
            points = [(0.4 * reach * POW, 0.0), (0.9 * reach * POW * math.cos(0.01), -0.9 * reach * POW * math.sin(0.01)),
                      (0.7 * reach * POW * math.cos(off), 0.7 * reach * POW * math.sin(off))]
            out.append(_case(cells, states, points, reach * POW, "floor_div / closed forms: " + what, resolution=POW, span=span, room=room,
                             what=what, steep=steep))
    # one non-free cell, passed at exact block distances
    W, H = 600, 400
    cells = np.zeros((H, W), dtype=np.int8)
    cells[203, 299] = ref.OCCUPIED  # block (37, 25)
    states, distances = [], []
    for d in (0, 1, 2, 3, 16, 17):
        for sign in (1, -1):
            if d == 0 and sign < 0:
                continue
            for start in range(5, 13):
                states.append(local_pose(IDENTITY, start + 0.5, 8 * (25 + sign * d) + 3.5, 0.0))
                distances.append(d)
    points = [(0.5 * 600 * RES, 0.0), (20.0, 0.004), (3.0, 3.0), (-1.0, 0.3)]  # (every ray leaves the grid: 588 .. 595 cells)
    out.append(_case(cells, states, points, 600 * RES, "one non-free cell at block distances 0, 1, 2, 3, 16, 17", distances=distances,
                     block=(37, 25)))
    return out


# ---- window_and_sectors (ordered kernel) -----------------------------------------------------------------------------------------------
WINDOW_REACHES = (447, 449, 600, 895, 897)
WIN = 1024


def sectors_of(max_range, resolution):
    """k_reweight_beam_sorted's own test, in its float arithmetic: four sector windows for a reach in (448, 896) cells."""
    reach = np.float32(max_range) * np.float32(1.0 / resolution)
    return 4 if (reach > np.float32(WIN // 2 - 64) and reach < np.float32(WIN - 128)) else 1


def sector_window_x0(cx, reach):
    """The corner column of the +x sectors' window (k_reweight_beam_sorted: room = (kWin - reach) / 2, x0 = cx - room on a multiple of 32)."""
    return ((cx - (WIN - int(reach)) // 2) >> 5) << 5


def window_of(cx, cy):
    """The single window's corner for a middle particle in cell (cx, cy)."""
    return ((cx - WIN // 2) >> 5) << 5, ((cy - WIN // 2) >> 3) << 3


@functools.lru_cache(maxsize=None)
def window_and_sectors():
    """A 1300 x 1100 grid, larger than the 1024 x 1024 window; the set sits in cell (650, 550) with the grid's heading (so the middle ray
    of the beams along the axes has ex = 0 or ey = 0: the sector seams), one pose 300 cells away and two outside the window altogether
    (at most one of them can be alone in a last workgroup of one lane); walls in the single window's last cells and in the first cells
    outside it, on all four sides; for each reach that engages the four sector windows, a pose 14 cells inside the low-x edge of the
    +x +y sector's window, turned so that its rays of that sector's beams run back across the edge, and walls in the window's first
    column and in the column outside it: the hand-over from the LDS sector window to the whole-grid maps.  Reaches either side of 448 and
    896 cells."""
    W, H = 1300, 1100
    cx, cy = 650, 550
    x0, y0 = window_of(cx, cy)
    cells = np.zeros((H, W), dtype=np.int8)
    cells[555:566, x0 + WIN - 1] = ref.OCCUPIED   # last column inside
    cells[566:580, x0 + WIN] = ref.OCCUPIED       # first column outside
    cells[520:532, x0] = ref.OCCUPIED
    cells[532:545, x0 - 1] = ref.UNKNOWN
    cells[y0 + WIN - 1, 655:668] = ref.OCCUPIED
    cells[y0 + WIN, 668:682] = ref.OCCUPIED
    cells[y0, 620:633] = ref.UNKNOWN
    cells[y0 - 1, 633:646] = ref.OCCUPIED
    for reach in WINDOW_REACHES:
        if sectors_of(reach * RES, RES) == 4:
            sx0 = sector_window_x0(cx, reach)
            cells[566:640, sx0] = ref.OCCUPIED       # the sector window's first column
            cells[640:800, sx0 - 1] = ref.OCCUPIED   # the column outside it
    cells[salt(H, W, 4099) == ref.OCCUPIED] = ref.OCCUPIED
    cells[545:556, 645:656] = ref.FREE
    out = []
    for reach in WINDOW_REACHES:
        states = [local_pose(IDENTITY, cx + fx, cy + fy, 0.0) for fx, fy in ((0.5, 0.5), (0.2, 0.7), (0.8, 0.3), (0.35, 0.15), (0.6, 0.9), (0.9, 0.6))]
        states.append(local_pose(IDENTITY, 350.5, 380.5, 0.9))    # inside the window, its long rays leave it
        states.append(local_pose(IDENTITY, 60.5, 1030.5, -0.7))   # outside the window altogether
        states.append(local_pose(IDENTITY, 1240.5, 20.5, 2.5))    # and another, elsewhere in the order
        edge = [r_ for r_ in WINDOW_REACHES if sectors_of(r_ * RES, RES) == 4]
        states += [local_pose(IDENTITY, sector_window_x0(cx, r_) + 14.5, 560.5, 1.2) for r_ in edge]
        aims = [math.atan2(dy, dx) for dx, dy in ((501.0, 9.0), (502.0, 22.0), (-522.0, -25.0), (-523.0, -12.0), (10.0, 505.0), (24.0, 506.0),
                                                   (-24.0, -518.0), (-11.0, -519.0))]
        angles = [0.0, math.pi / 2, math.pi, -math.pi / 2] + aims + list(0.05 + 2 * np.pi * np.arange(28) / 28)
        points = scan(angles, spread_ranges(len(angles), reach * RES))
        points[1], points[3] = (0.0, points[1][1]), (0.0, points[3][1])   # exactly along +y and -y: ex = 0
        points[2] = (points[2][0], 0.0)                                    # exactly along -x: ey = 0
        out.append(_case(cells, states, points, reach * RES, "reach %d cells: %d window(s)" % (reach, sectors_of(reach * RES, RES)), majority=6,
                         reach=reach, window=(x0, y0), middle=(cx, cy), outside=(7, 8),
                         edge_pose=(9 + edge.index(reach)) if reach in edge else None))
    return out


# ---- free_ahead (ordered kernel) -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def free_ahead():
    """A tight cloud (a cell wide, headings within 4 mrad) in a room whose walls stand 20 .. 140 cells away, with one-cell pillars next to
    the middle rays - off some lanes' rays, on others' -; and a wide cloud over the same room, for which no certificate applies."""
    W, H = 420, 330
    cells = np.zeros((H, W), dtype=np.int8)
    cx, cy = 200, 160
    cells[cy - 137, :] = cells[cy + 30, :] = ref.OCCUPIED
    cells[:, cx - 100] = cells[:, cx + 50] = ref.OCCUPIED
    cells[cy + 20, cx - 30:cx + 10] = ref.UNKNOWN
    for k, t in enumerate(np.linspace(-3.0, 3.0, 23)):
        r = 18 + (11 * k) % 70
        px, py = cx + int(round(r * math.cos(t))), cy + int(round(r * math.sin(t)))
        if 0 < px < W - 1 and 0 < py < H - 1 and cells[py, px] == ref.FREE:
            cells[py, px] = ref.OCCUPIED
    angles = 0.01 + 2 * np.pi * np.arange(64) / 64
    reach = 300
    points = scan(angles, spread_ranges(64, reach * RES))
    tight = [local_pose(IDENTITY, cx + fx, cy + fy, dth) for fx, fy, dth in ((0.5, 0.5, 0.0), (0.1, 0.8, 0.002), (0.9, 0.2, -0.002), (0.3, 0.3, 0.001),
                                                                            (0.7, 0.6, -0.001), (0.05, 0.05, 0.0015), (0.95, 0.95, -0.0015), (0.5, 0.1, 0.0005))]
    rng = np.random.Generator(np.random.MT19937(5))
    wide = [local_pose(IDENTITY, x, y, th) for x, y, th in zip(rng.uniform(cx - 95, cx + 45, 12), rng.uniform(cy - 130, cy + 25, 12), rng.uniform(-np.pi, np.pi, 12))]
    return [_case(cells, tight, points, reach * RES, "a tight cloud: the certificate fires", tight=True),
            _case(cells, wide, points, reach * RES, "a wide cloud: no certificate", tight=False)]


# ---- range_terms -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_terms():
    """Around a pose: a ring of cells 8.8 .. 10.2 cells away over the first quadrant (expected ranges either side of 6.5 .. 6.6 sqrt(2)
    sigma_hit = 9.19 .. 9.33 cells from 0), one 190 .. 191.6 cells away over the second (the same from max_range = 200 cells), one at
    199.5 .. 201.2 over the third (hits at and beyond max_range: fmin, and squared distances at the table's end), nothing over the fourth.
    Measured ranges EQUAL to a pose's expected range along its own +x, +y, -x, -y and one ulp either side (the tie rule), at, above and
    far above max_range (the z_max tail), and a pose inside a non-free cell (expected range 0).  The second case has the same rays with
    max_range / resolution = 2100 cells > 2046: no table."""
    W = H = 440
    cx = cy = 220
    yy, xx = np.mgrid[0:H, 0:W]
    rr, aa = np.hypot(xx - cx, yy - cy), np.arctan2(yy - cy, xx - cx)
    cells = np.zeros((H, W), dtype=np.int8)
    cells[(rr >= 8.8) & (rr <= 10.2) & (aa >= -0.1) & (aa < 1.5)] = ref.OCCUPIED
    cells[(rr >= 190.0) & (rr <= 191.6) & (aa >= 1.65) & (aa < 3.0)] = ref.OCCUPIED
    cells[(rr >= 199.5) & (rr <= 201.2) & (aa >= -3.0) & (aa < -1.65)] = ref.UNKNOWN
    cells[cy - 40, cx + 3] = ref.OCCUPIED
    out = []
    for reach, name in ((200.0, "table"), (2100.0, "no table")):
        max_range = reach * RES
        heads = (0.0, 0.0, 0.0, 0.3, 0.7, 1.1, 2.0, 2.9, -2.2, -0.8)
        offs = ((0.5, 0.5), (0.9, 0.9), (0.1, 0.3), (0.5, 0.5), (0.2, 0.8), (0.7, 0.4), (0.5, 0.5), (0.6, 0.1), (0.4, 0.6), (0.8, 0.2))
        states = [local_pose(IDENTITY, cx + fx, cy + fy, th) for (fx, fy), th in zip(offs, heads)]
        states.append(local_pose(IDENTITY, cx + 3.5, cy - 39.5, 0.4))  # inside the non-free cell
        generic = scan(0.02 + 2 * np.pi * np.arange(48) / 48, spread_ranges(48, max_range))
        probe = dict(cells=cells, resolution=RES, origin=IDENTITY, states=np.array(states), points=np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]),
                     params=ref.revealing_params(RES, max_range))
        r = ref.reference(probe)
        ties, points = [], [tuple(p) for p in generic]
        axes = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
        for i in range(len(states) - 1):
            for b, (ux, uy) in enumerate(axes):
                if not r["has_hit"][i, b] or r["expected"][i, b] <= 0.0:
                    continue
                e = float(r["expected"][i, b])
                for j, z in ((-1, np.nextafter(e, 0.0)), (0, e), (1, np.nextafter(e, np.inf))):
                    ties.append((i, len(points), j))
                    points.append((ux * float(z), uy * float(z)))
        tails = []
        for z in (np.nextafter(max_range, 0.0), max_range, np.nextafter(max_range, np.inf), 2.5 * max_range):
            tails.append(len(points))
            points.append((float(z), 0.0))
        out.append(_case(cells, states, points, max_range, "range terms, " + name, ties=ties, tails=tails, reach=reach))
    return out


# ---- beam_counts -----------------------------------------------------------------------------------------------------------------------
BEAM_COUNTS = (1, 7, 8, 9, 63, 64, 65, 129)
# The ordered kernel splits the scan of a set of n < 262 144 particles into min(16, B / 8) segments (launch_reweight_beam): none below 16
# beams, partial sums and k_lf_combine from 16 on.  A segment of more than kBeamCertified = 2048 beams (no per-beam entries: no certificate,
# no sectors) takes 16 * 2048 + 1 = 32 769 beams or more at these set sizes: CERTIFIED_OVERFLOW has 32 784 = 16 segments of 2049.
CERTIFIED_OVERFLOW = 32784


@functools.lru_cache(maxsize=None)
def beam_counts():
    """One scan of 129 points over a salted 157 x 203 grid behind a rotated origin (the tests take its first B points for every B of
    BEAM_COUNTS), and one of 32 784 short beams whose segments exceed the certificate's 2048 entries."""
    cells = salt(157, 203)
    rng = np.random.Generator(np.random.MT19937(80))
    states = [local_pose(ROTATED, x, y, th) for x, y, th in zip(rng.uniform(20, 180, 8), rng.uniform(20, 140, 8), rng.uniform(-np.pi, np.pi, 8))]
    reach = 120.0
    points = scan(rng.uniform(-np.pi, np.pi, 129), spread_ranges(129, reach * RES))
    many = scan(2 * np.pi * np.arange(CERTIFIED_OVERFLOW) / CERTIFIED_OVERFLOW, spread_ranges(CERTIFIED_OVERFLOW, 12 * RES))
    return [_case(cells, states, points, reach * RES, "every beam count", origin=ROTATED),
            _case(cells, states[:2], many, 12 * RES, "segments of 2049 beams: beyond kBeamCertified", origin=ROTATED)]


def prefix(case, B):
    return dict(case, points=case["points"][:B])


FAMILIES = {"slopes": slopes, "obstacle_at_k": obstacle_at_k, "borders_and_tiny_grids": borders_and_tiny_grids, "cell_boundaries": cell_boundaries,
            "closed_form_thresholds": closed_form_thresholds, "window_and_sectors": window_and_sectors, "free_ahead": free_ahead,
            "range_terms": range_terms, "beam_counts": beam_counts}
