"""The written rule of the beam sensor model (sensor/beam_model.hpp, algorithm/raycasting.hpp, algorithm/raycasting/bresenham.hpp), as
plain as it can be made: Python ints for the walk, one cell at a time; Python floats (IEEE doubles, one rounding per operation, no
contraction) for what the reference computes in doubles; extended precision for the mixture.  No device, nothing compiled, no oracle.

    T = grid_origin^-1 * state                                  (Ray2d ctor, raycasting.hpp:62-70; Sophus' order: lf_reference.transforms)
    source cell  = floor(T.x * (1 / resolution)), floor(T.y * (1 / resolution))                     (regular_grid.hpp:75-78)
    z = sqrt(px^2 + py^2), bearing = (px / z, py / z)                                              (beam_model.hpp:112-114)
    far end      = T * (bearing * max_range), each product and sum rounded on its own; its cell as above         (raycasting.hpp:78-88)
    trace        = the STANDARD Bresenham line from the source cell to the far-end cell (bresenham.hpp:84-160), cell by cell; it stops at
                   the first cell outside the grid (no hit), not free (hit: unknown cells are not free) or past the end (no hit)
    visited      = the cells looked at: those of the trace inside the grid up to and including the hit
    expected     = fmin(distance of the two cells' CENTRES (xi + 0.5) * resolution, max_range), or max_range without a hit
    pz           = z_hit eta_hit N(z; expected, sigma_hit) + [z < expected] z_short lambda_short eta_short exp(-lambda_short z)
                   + (z < max_range ? z_rand / max_range : z_max);   the weight is prior * sum pz^3            (beam_model.hpp:104-150)

`z < expected` is decided on the doubles (it is the one place where the last bit of the expected range decides something); the mixture
itself is then evaluated in extended precision - numpy.longdouble where that is the x87 format, mpmath at 80 bits where not, as in
propagate_reference.py - and rounded once.

In contract: |cell coordinates| below 2^31 and line spans below 2^29 cells (the reference's own int error term holds up to 4 * span).
Scan points of range 0 are out (the reference divides 0 / 0 there).

MUTANTS restates the rule wrongly, one way at a time - what a subtly wrong kernel would compute.  revealing_params() are beam parameters
under which a wrong hit cell shows in a weight.
"""
import math

import numpy as np

import lf_reference as lfref
from propagate_reference import USE_MPMATH, ext, to_f64, x_sqrt

FREE, UNKNOWN, OCCUPIED = 0, -1, 100  # the ROS traits (beluga_ros/occupancy_grid.hpp:48-64)

# ---- extended precision exp and erf ---------------------------------------------------------------------------------------------------
if USE_MPMATH:
    import mpmath

    x_exp = np.frompyfunc(mpmath.exp, 1, 1)
    x_erf = np.frompyfunc(mpmath.erf, 1, 1)
else:
    x_exp = np.exp
    _PI_LD = np.longdouble("3.14159265358979323846264338327950288")

    def x_erf(x):
        """erf in long double: 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 .. (2n+1)) - every term positive, no cancellation;
        1 beyond |x| = 7 (erfc(7) = 4e-23, below half an ulp)."""
        x = np.asarray(x, dtype=np.longdouble)
        a = np.abs(x)
        big = a >= 7
        a = np.where(big, np.longdouble(0), a)
        term = a.copy()
        total = a.copy()
        for n in range(1, 240):
            term = term * (2 * a * a) / (2 * n + 1)
            total = total + term
        r = 2 / np.sqrt(_PI_LD) * np.exp(-a * a) * total
        return np.copysign(np.where(big, np.longdouble(1), r), x)


# ---- the rule and its wrong restatements -----------------------------------------------------------------------------------------------
RULE = dict(trip_ge=False, truncate=False, divide=False, extra_cells=0, unknown_free=False, outside_hit=False, modified=False,
            corners=False, short_le=False, tie_sqrt=False)
MUTANTS = {
    "trip_ge": dict(trip_ge=True),            # the error term trips on error >= dmajor
    "truncate": dict(truncate=True),          # static_cast<int>(v) without the floor
    "divide": dict(divide=True),              # v / resolution instead of v * (1 / resolution)
    "past_the_end": dict(extra_cells=1),      # one cell past the far-end cell is examined
    "stop_early": dict(extra_cells=-1),       # the far-end cell itself is not examined
    "unknown_free": dict(unknown_free=True),  # unknown cells let the ray through
    "outside_hit": dict(outside_hit=True),    # the first cell outside the grid is a hit
    "modified": dict(modified=True),          # the modified Bresenham variant (bresenham.hpp:122-160, Variant::kModified)
    "corners": dict(corners=True),            # range between the cells' corners xi * resolution
    "short_le": dict(short_le=True),          # measured <= expected for the short-return term
    "tie_sqrt": dict(tie_sqrt=True),          # expected range sqrt(r2) * resolution (the table's value) where it decides measured < expected
}


def rule_of(mutant=None):
    return dict(RULE, **(MUTANTS[mutant] if isinstance(mutant, str) else (mutant or {})))


def source_poses(origin, states):
    """grid_origin^-1 * state, [m, 4] as (cos, sin, x, y)."""
    return lfref.transforms(origin, states)


def cell_near(v, resolution, rule=RULE):
    q = v / resolution if rule["divide"] else v * (1.0 / resolution)
    return int(q) if rule["truncate"] else math.floor(q)


def bearing_of(px, py):
    z = math.sqrt(px * px + py * py)
    return z, px / z, py / z


def far_end(T, c, s, max_range):
    tx, ty = c * max_range, s * max_range
    ex = T[0] * tx - T[1] * ty
    ey = T[1] * tx + T[0] * ty
    return ex + T[2], ey + T[3]


def line(x0, y0, x1, y1, modified=False, trip_ge=False, extra_cells=0):
    """The cells of Bresenham2i's iterator from (x0, y0) to (x1, y1), in order."""
    xspan, xstep = x1 - x0, 1
    if xspan < 0:
        xspan, xstep = -xspan, -1
    yspan, ystep = y1 - y0, 1
    if yspan < 0:
        yspan, ystep = -yspan, -1
    x, y = x0, y0
    steep = xspan < yspan
    if steep:
        x, y, xspan, yspan, xstep, ystep = y, x, yspan, xspan, ystep, xstep
    dxspan, dyspan = 2 * xspan, 2 * yspan
    error = prev = xspan
    yield (x0, y0)
    for _ in range(xspan + extra_cells):
        x += xstep
        error += dyspan
        if (error >= dxspan) if trip_ge else (error > dxspan):
            y += ystep
            error -= dxspan
            if modified:
                if error + prev <= dxspan:
                    yield (y - ystep, x) if steep else (x, y - ystep)
                if error + prev >= dxspan:
                    yield (y, x - xstep) if steep else (x - xstep, y)
        yield (y, x) if steep else (x, y)
        prev = error


def nonfree_mask(cells, rule=RULE):
    """bytes, row-major: 1 where a cell stops a ray."""
    cells = np.asarray(cells, dtype=np.int8)
    return (((cells != FREE) & (cells != UNKNOWN)) if rule["unknown_free"] else (cells != FREE)).astype(np.uint8).tobytes()


def cast(mask, W, H, sx, sy, fx, fy, rule=RULE):
    """(hit cell or None, cells visited)."""
    visited = 0
    for x, y in line(sx, sy, fx, fy, rule["modified"], rule["trip_ge"], rule["extra_cells"]):
        if not (0 <= x < W and 0 <= y < H):
            return ((x, y) if rule["outside_hit"] else None), visited
        visited += 1
        if mask[y * W + x]:
            return (x, y), visited
    return None, visited


def cell_distance(sx, sy, hx, hy, resolution, max_range, rule=RULE):
    off = 0.0 if rule["corners"] else 0.5
    ax, ay = (float(sx) + off) * resolution, (float(sy) + off) * resolution
    bx, by = (float(hx) + off) * resolution, (float(hy) + off) * resolution
    dx, dy = bx - ax, by - ay
    return min(math.sqrt(dx * dx + dy * dy), max_range)


def table_distance(sx, sy, hx, hy, resolution, max_range):
    """What the ordered kernel's table holds for the hit's squared cell distance."""
    return min(math.sqrt(float((hx - sx) ** 2 + (hy - sy) ** 2)) * resolution, max_range)


def mixture(params, z, expected, short):
    """pz^3 per ray in extended precision; z [B] and expected [m, B] doubles, short [m, B] the decided `z < expected`."""
    z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short, max_range = (ext(float(v)) for v in params)
    Z, M = ext(z)[None, :], ext(expected)
    scale = x_sqrt(ext(2.0)) * sigma_hit
    with np.errstate(all="ignore"):
        eta_hit = 2 / (x_erf((max_range - M) / scale) - x_erf(-M / scale))
        norm = 1 / (x_sqrt(ext(2.0) * ext(math.pi)) * sigma_hit)  # (M_PI, the double, as written)
        d = (Z - M) / sigma_hit
        pz = z_hit * eta_hit * norm * x_exp(-(d * d) / 2)
        M_short = np.where(short, M, ext(1.0))  # (eta_short only where it is used: an expected range of 0 never has z < 0)
        eta_short = 1 / (1 - x_exp(-lambda_short * M_short))
        pz = pz + np.where(short, z_short * lambda_short * eta_short * x_exp(-lambda_short * Z), ext(0.0))
        tail = np.where(np.asarray(z)[None, :] < float(params[6]), z_rand / max_range, z_max)
        pz = pz + tail
    return pz * pz * pz


def reference(case, mutant=None, states=None):
    """Everything the rule says about a case (tests/beam_families.py): per pose the source cell, per ray the far-end cell, the hit cell
    (has_hit), the cells visited and the expected range; per pose sum pz^3 (`weights`, for a prior of 1) rounded once; the total count."""
    rule = rule_of(mutant)
    cells = np.asarray(case["cells"], dtype=np.int8)
    H, W = cells.shape
    res, params = float(case["resolution"]), tuple(float(v) for v in case["params"])
    max_range = params[6]
    T = source_poses(case["origin"], case["states"] if states is None else states)
    points = np.asarray(case["points"], dtype=np.float64).reshape(-1, 2)
    m, B = len(T), len(points)
    mask = nonfree_mask(cells, rule)
    bearings = [bearing_of(float(px), float(py)) for px, py in points]
    z = np.array([b[0] for b in bearings])
    source = np.zeros((m, 2), dtype=np.int64)
    far = np.zeros((m, B, 2), dtype=np.int64)
    hit = np.zeros((m, B, 2), dtype=np.int64)
    has_hit = np.zeros((m, B), dtype=bool)
    visited = np.zeros((m, B), dtype=np.int64)
    expected = np.full((m, B), max_range)
    short = np.zeros((m, B), dtype=bool)
    for i in range(m):
        Ti = [float(v) for v in T[i]]
        sx, sy = cell_near(Ti[2], res, rule), cell_near(Ti[3], res, rule)
        source[i] = sx, sy
        for b, (zb, c, s) in enumerate(bearings):
            ex, ey = far_end(Ti, c, s, max_range)
            fx, fy = cell_near(ex, res, rule), cell_near(ey, res, rule)
            far[i, b] = fx, fy
            got, visited[i, b] = cast(mask, W, H, sx, sy, fx, fy, rule)
            decide = max_range
            if got is not None:
                has_hit[i, b] = True
                hit[i, b] = got
                expected[i, b] = decide = cell_distance(sx, sy, got[0], got[1], res, max_range, rule)
                if rule["tie_sqrt"]:
                    decide = table_distance(sx, sy, got[0], got[1], res, max_range)
            short[i, b] = (zb <= decide) if rule["short_le"] else (zb < decide)
    terms = mixture(params, z, expected, short)
    weights = to_f64(terms.sum(axis=1)) if B else np.zeros(m)
    return dict(source=source, far=far, hit=hit, has_hit=has_hit, visited=visited, expected=expected, short=short, z=z, weights=weights,
                steps=int(visited.sum()))


def revealing_params(resolution, max_range):
    """(z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short, max_range): a hit distribution one cell wide and next to no random floor, so
    that a hit cell that is wrong by one cell moves its beam's term - and through it the particle's weight - by far more than 1e-6 relative
    wherever the measured range is below or within a few cells of the expected one (tests/test_beam_reference_cpu.py asserts it per kill)."""
    return (0.5, 0.5, 0.05, 0.001, float(resolution), 0.1, float(max_range))
