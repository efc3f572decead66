"""The reference's 2D NDT sensor model (beluga/include/beluga/sensor/ndt_sensor_model.hpp, sensor/data/ndt_cell.hpp), twice: a numpy
f64 restatement that follows the reference's (Eigen's, Sophus') arithmetic step by step, and an extended-precision form of everything
behind the cell choice.  The yardstick of tests/test_ndt_cpu.py, test_ndt_reference_cpu.py, test_gpu_ndt.py and test_gpu_ndt_edges.py.

  to_cells(points, resolution)      detail::to_cells (:88-110) + fit_points (:66-80): groups by (p / resolution) truncated toward
                                    zero, groups of < 5 points dropped, mean + sample covariance with the diagonal clamped to 1e-5
  likelihood_at(map, params, m, c)  NDTSensorModel::likelihood_at (:229-239) of a measurement cell already in the map frame
  weights(map, params, states, cells)  operator() (:216-226): 1 + sum over the cells of likelihood_at(state * cell)
  weights_exact(...)                the same weight with the centre key from the reference's own f64 sequence and everything after it
                                    in 60-digit arithmetic (mpmath), rounded to f64 once; MUTANTS: plausible slips of a kernel's cell choice
  revealing_map(keys, resolution)   map cells on which one wrong cell shows in the weight

Two things the reference leaves open.  to_cells iterates an unordered_map, so the ORDER of a scan's measurement cells is whatever the
standard library's hash gives: the project's ascending key order (to_cells here, ndt_fit_cells in the library) is a choice, not the
reference's, and only the rounding of the weight's sum depends on it.  The edges suite (ndt_families.py) therefore hands its
measurement cells to the library directly, in a fixed order (reweight_ndt_cells): the engineered cell means reach the kernel as the
doubles they were made, not through a fit, and the order of the sum is the one weights_exact's error bound was measured for.
The f64 loop form inverts S' + S_map as Eigen does a 2 x 2 matrix - adjugate times 1 / det - and forms the exponent in Eigen's product
order ((-d2 / 2 e)^T S^-1) e; the covariance is rotated as (R S) R^T with every product and sum rounded.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

DEFAULT_KERNEL = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1))


def fit_points(pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    mean = pts.mean(axis=0)
    d = pts - mean
    cov = d.T @ d / (len(pts) - 1)
    cov[0, 0] = max(cov[0, 0], 1e-5)
    cov[1, 1] = max(cov[1, 1], 1e-5)
    return mean, cov


def to_cells(points, resolution):
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    groups = {}
    for p in pts:
        key = (int(p[0] / resolution), int(p[1] / resolution))  # Eigen cast<int>: truncation toward zero
        groups.setdefault(key, []).append(p)
    means, covs = [], []
    for key in sorted(groups):
        g = groups[key]
        if len(g) < 5:
            continue
        m, c = fit_points(g)
        means.append(m)
        covs.append(c)
    return np.asarray(means).reshape(-1, 2), np.asarray(covs).reshape(-1, 2, 2)


class NdtMap:
    def __init__(self, cells, means, covariances, resolution):
        self.resolution = float(resolution)
        self.data = {(int(k[0]), int(k[1])): (np.asarray(m, dtype=np.float64), np.asarray(c, dtype=np.float64).reshape(2, 2))
                     for k, m, c in zip(np.asarray(cells).reshape(-1, 2), np.asarray(means).reshape(-1, 2),
                                        np.asarray(covariances).reshape(-1, 2, 2))}

    def cell_near(self, p):  # regular_grid.hpp:75-78; None for a component that is not finite (the reference's cast is undefined there)
        inv = 1.0 / self.resolution
        return tuple(int(math.floor(v * inv)) if math.isfinite(v * inv) else None for v in (float(p[0]), float(p[1])))


def inverse_2x2(S):
    """Eigen's inverse of a 2 x 2 matrix (compute_inverse_size2_helper): the adjugate times inv_det = 1 / det, det = s00 s11 - s10 s01.
    Elementwise over leading axes; a zero det gives infinities and NaNs as IEEE arithmetic does, without a warning."""
    S = np.asarray(S, dtype=np.float64)
    s00, s01, s10, s11 = S[..., 0, 0], S[..., 0, 1], S[..., 1, 0], S[..., 1, 1]
    with np.errstate(all="ignore"):
        inv_det = np.float64(1.0) / (s00 * s11 - s10 * s01)
        return np.stack([np.stack([s11 * inv_det, -s01 * inv_det], -1), np.stack([-s10 * inv_det, s00 * inv_det], -1)], -2)


def cell_likelihood(map_mean, map_cov, mean, cov, d1=1.0, d2=1.0):  # ndt_cell.hpp:49-54
    e0, e1 = np.float64(mean[0]) - np.float64(map_mean[0]), np.float64(mean[1]) - np.float64(map_mean[1])
    inv = inverse_2x2(np.asarray(cov, dtype=np.float64) + np.asarray(map_cov, dtype=np.float64))
    with np.errstate(all="ignore"):
        v0, v1 = np.float64(-d2 / 2.0) * e0, np.float64(-d2 / 2.0) * e1
        r0, r1 = v0 * inv[0, 0] + v1 * inv[1, 0], v0 * inv[0, 1] + v1 * inv[1, 1]
        q = float(r0 * e0 + r1 * e1)
    if math.isnan(q):
        return math.nan
    return d1 * (math.inf if q > 709.782712893384 else math.exp(q))


def likelihood_at(ndt_map, mean, cov, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL):
    cx, cy = ndt_map.cell_near(mean)
    total = 0.0
    for dx, dy in kernel if cx is not None and cy is not None else ():
        hit = ndt_map.data.get((cx + dx, cy + dy))
        if hit is not None:
            total += cell_likelihood(hit[0], hit[1], mean, cov, d1, d2)
    return max(total, minimum_likelihood)


def transform_cell(state, mean, cov):  # operator*(SE2, NDTCell), ndt_cell.hpp:61-66; state = (cos, sin, x, y)
    c, s, x, y = (np.float64(v) for v in state)
    mx, my = np.float64(mean[0]), np.float64(mean[1])
    cov = np.asarray(cov, dtype=np.float64)
    sa, sb, sc, sd = cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1]
    with np.errstate(all="ignore"):
        t00, t01, t10, t11 = c * sa - s * sc, c * sb - s * sd, s * sa + c * sc, s * sb + c * sd  # R S
        tc = np.array([[t00 * c - t01 * s, t00 * s + t01 * c], [t10 * c - t11 * s, t10 * s + t11 * c]])  # (R S) R^T
        return np.array([(c * mx - s * my) + x, (s * mx + c * my) + y]), tc


def weights(ndt_map, states, means, covs, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL):
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    out = np.empty(len(states))
    for i, st in enumerate(states):
        acc = 1.0
        for m, c in zip(means, covs):
            tm, tc = transform_cell(st, m, c)
            acc += likelihood_at(ndt_map, tm, tc, minimum_likelihood, d1, d2, kernel)
        out[i] = acc
    return out


def weights_vectorized(ndt_map, states, means, covs, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL):
    """weights() over many states at once (numpy over the states; the same arithmetic, the cells and offsets in the same order)."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    c, s, x, y = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    keys = sorted(ndt_map.data)
    codes = np.array([(kx << 32) + (ky & 0xFFFFFFFF) for kx, ky in keys], dtype=np.int64)
    order = np.argsort(codes)
    codes = codes[order]
    mm = np.array([ndt_map.data[keys[i]][0] for i in order]).reshape(-1, 2)
    mc = np.array([ndt_map.data[keys[i]][1] for i in order]).reshape(-1, 2, 2)
    inv = 1.0 / ndt_map.resolution
    acc = np.ones(len(st))
    for m, cv in zip(means, covs):
        ux = c * m[0] - s * m[1] + x
        uy = s * m[0] + c * m[1] + y
        sa, sb, sc, sd = (np.float64(v) for v in np.asarray(cv, dtype=np.float64).reshape(4))
        t00, t01, t10, t11 = c * sa - s * sc, c * sb - s * sd, s * sa + c * sc, s * sb + c * sd  # R S, then (R S) R^T
        tc = np.stack([np.stack([t00 * c - t01 * s, t00 * s + t01 * c], -1), np.stack([t10 * c - t11 * s, t10 * s + t11 * c], -1)], -2)
        cx = np.floor(ux * inv).astype(np.int64)
        cy = np.floor(uy * inv).astype(np.int64)
        total = np.zeros(len(st))
        for dx, dy in kernel:
            code = ((cx + dx) << 32) + ((cy + dy) & 0xFFFFFFFF)
            pos = np.clip(np.searchsorted(codes, code), 0, len(codes) - 1) if len(codes) else np.zeros(len(st), dtype=np.int64)
            hit = (codes[pos] == code) if len(codes) else np.zeros(len(st), dtype=bool)
            if not np.any(hit):
                continue
            e = np.stack([ux - mm[pos, 0], uy - mm[pos, 1]], -1)[hit]
            S = tc[hit] + mc[pos[hit]]
            si = inverse_2x2(S)
            with np.errstate(all="ignore"):
                v0, v1 = (-d2 / 2.0) * e[:, 0], (-d2 / 2.0) * e[:, 1]
                r0, r1 = v0 * si[:, 0, 0] + v1 * si[:, 1, 0], v0 * si[:, 0, 1] + v1 * si[:, 1, 1]
                total[hit] += d1 * np.exp(r0 * e[:, 0] + r1 * e[:, 1])
        acc += np.maximum(total, minimum_likelihood)
    return acc


# ---- the exact form ----------------------------------------------------------------------------------------------------------------------
mpmath.mp.dps = 60
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def _fl(q):
    """A rational rounded to the nearest double (ties to even): CPython's int / int is correctly rounded."""
    return np.float64(q.numerator / q.denominator)


def moved_mean(state, mean, fused=None):
    """Sophus so2 * p + t as the reference's compiler evaluates it without contraction: the two products and their difference (sum) each
    rounded, then + t.  fused = "ux_a" / "ux_b" / "uy_a" / "uy_b": ONE product of that component kept exact into the difference (a fused
    multiply-add), the first or the second - exact rational arithmetic, rounded once."""
    c, s, x, y = (np.float64(v) for v in state)
    mx, my = np.float64(mean[0]), np.float64(mean[1])
    F = Fraction
    with np.errstate(all="ignore"):
        if fused == "ux_a":
            ax = _fl(F(float(c)) * F(float(mx)) - F(float(s * my)))
        elif fused == "ux_b":
            ax = _fl(F(float(c * mx)) - F(float(s)) * F(float(my)))
        else:
            ax = c * mx - s * my
        if fused == "uy_a":
            ay = _fl(F(float(s)) * F(float(mx)) + F(float(c * my)))
        elif fused == "uy_b":
            ay = _fl(F(float(s * mx)) + F(float(c)) * F(float(my)))
        else:
            ay = s * mx + c * my
        return ax + x, ay + y


def cell_key(u, resolution):
    """regular_grid.hpp:75-78 on one component: floor(u * (1. / resolution)) cast to int, every step a float64 operation.  Beyond the
    int32 range the reference's cast is undefined; the Python int of the floor is returned there (no map has such a key)."""
    with np.errstate(all="ignore"):
        t = np.float64(u) * (np.float64(1.0) / np.float64(resolution))
    return int(np.floor(t)) if np.isfinite(t) else None


def _key_divide(u, resolution, box):
    with np.errstate(all="ignore"):
        t = np.float64(u) / np.float64(resolution)
    return int(np.floor(t)) if np.isfinite(t) else None


def _key_truncate(u, resolution, box):
    with np.errstate(all="ignore"):
        t = np.float64(u) * (np.float64(1.0) / np.float64(resolution))
    return int(np.trunc(t)) if np.isfinite(t) else None


def _key_from_corner(axis):
    def key(u, resolution, box):
        """floor((u - origin) * inv) + the box's first key: the box corner subtracted in metres before the scaling."""
        first = box[axis]
        with np.errstate(all="ignore"):
            t = (np.float64(u) - np.float64(first) * np.float64(resolution)) * (np.float64(1.0) / np.float64(resolution))
        return int(np.floor(t)) + first if np.isfinite(t) else None
    return key


class Variant:
    """A way to choose and look up cells.  The default is the reference's; MUTANTS override one piece each.
      fused      moved_mean's argument
      key        (u, resolution, box) -> key of one component, or None; box = (first centre key x, first centre key y)
      box_shrink (x_lo, x_hi, y_lo, y_hi): cells taken off that end of the centre box [first key - reach, last key + reach]
      border     the index grid's border in units of reach as the HOST lays it out, the kernel counting on 2 (2: the library's).  A border
                 of reach on both sides would be harmless: with the centre box a neighbour at most reach past the grid's edge lands in
                 the next row's border columns, which are empty
      swap       kernel offsets visited as (dy, dx)
      wrap32     centre and neighbour keys wrapped to int32 before the box test and the look-up
      transposed the covariance rotated as R^T S R"""

    def __init__(self, fused=None, key=None, box_shrink=(0, 0, 0, 0), border=2, swap=False, wrap32=False, transposed=False):
        self.fused, self.key, self.box_shrink, self.border = fused, key, box_shrink, border
        self.swap, self.wrap32, self.transposed = swap, wrap32, transposed


REFERENCE = Variant()
MUTANTS = {
    "fused_ux_a": Variant(fused="ux_a"), "fused_ux_b": Variant(fused="ux_b"),
    "fused_uy_a": Variant(fused="uy_a"), "fused_uy_b": Variant(fused="uy_b"),
    "divide_by_resolution": Variant(key=_key_divide),
    "truncate": Variant(key=_key_truncate),
    "corner_first": Variant(key="corner"),
    "box_x_lo": Variant(box_shrink=(1, 0, 0, 0)), "box_x_hi": Variant(box_shrink=(0, 1, 0, 0)),
    "box_y_lo": Variant(box_shrink=(0, 0, 1, 0)), "box_y_hi": Variant(box_shrink=(0, 0, 0, 1)),
    "border_reach": Variant(border=1),
    "offsets_dy_dx": Variant(swap=True),
    "wrap_int32": Variant(wrap32=True),
    "rotation_transposed": Variant(transposed=True),
}
FUSED_MUTANTS = ("fused_ux_a", "fused_ux_b", "fused_uy_a", "fused_uy_b")
BOX_MUTANTS = ("box_x_lo", "box_x_hi", "box_y_lo", "box_y_hi", "border_reach")


def _wrap32(v):
    return (v + 2**31) % 2**32 - 2**31


def neighbours(ndt_map, kernel, centre, variant=REFERENCE):
    """The map cells a centre key finds, as keys, in kernel order (None where there is none).  The reference's look-up is a dictionary's;
    the variants model a device layout: the centre box, and for border != 2 an index grid with too narrow a border, whose flat index wraps."""
    keys = list(ndt_map.data)
    if not keys or centre[0] is None or centre[1] is None:
        return [None] * len(kernel)
    reach = max(1, max(max(abs(dx), abs(dy)) for dx, dy in kernel))
    x0, x1 = min(k[0] for k in keys), max(k[0] for k in keys)
    y0, y1 = min(k[1] for k in keys), max(k[1] for k in keys)
    lo_x, hi_x, lo_y, hi_y = variant.box_shrink
    if variant.wrap32:  # (the centre key held in an int32 as well: the box test sees the wrapped key)
        centre = (_wrap32(centre[0]), _wrap32(centre[1]))
    inside = x0 - reach + lo_x <= centre[0] <= x1 + reach - hi_x and y0 - reach + lo_y <= centre[1] <= y1 + reach - hi_y
    out = []
    for dx, dy in kernel:
        if variant.swap:
            dx, dy = dy, dx
        k = (centre[0] + dx, centre[1] + dy)
        if not inside:
            k = None
        elif variant.wrap32:
            k = (_wrap32(k[0]), _wrap32(k[1]))
        elif variant.border != 2:
            # the index grid laid out with a border of `border` x reach while the kernel's index arithmetic counts on 2 x reach: the flat
            # index lands in another column and, past a row's end, on the next row
            b = variant.border * reach
            gw, gh = (x1 - x0 + 1) + 2 * b, (y1 - y0 + 1) + 2 * b
            flat = (k[1] - (y0 - 2 * reach)) * gw + (k[0] - (x0 - 2 * reach))
            k = (x0 - b + flat % gw, y0 - b + flat // gw) if 0 <= flat < gw * gh else None
        out.append(k if k in ndt_map.data else None)
    return out


def centre_key(ndt_map, state, mean, variant=REFERENCE):
    """(ux, uy, (cx, cy)) of a measurement cell's mean under a pose: the f64 sequence the reference runs."""
    ux, uy = moved_mean(state, mean, variant.fused)
    keys = list(ndt_map.data)
    box = (min(k[0] for k in keys), min(k[1] for k in keys)) if keys else (0, 0)
    if variant.key is None:
        return ux, uy, (cell_key(ux, ndt_map.resolution), cell_key(uy, ndt_map.resolution))
    kx = _key_from_corner(0) if variant.key == "corner" else variant.key
    ky = _key_from_corner(1) if variant.key == "corner" else variant.key
    return ux, uy, (kx(ux, ndt_map.resolution, box), ky(uy, ndt_map.resolution, box))


def _mp(v):
    return mpmath.mpf(float(v))


def likelihood_exact(ux, uy, state, cov, map_mean, map_cov, d1, d2, transposed=False):
    """d1 exp(-d2 / 2 e^T (R S R^T + S_map)^-1 e) in 60 digits from the doubles given; also det(S) / (s00 s11)."""
    c, s = _mp(state[0]), _mp(state[1])
    if transposed:
        s = -s
    sa, sb, sc, sd = (_mp(v) for v in np.asarray(cov, dtype=np.float64).reshape(4))
    t00, t01, t10, t11 = c * sa - s * sc, c * sb - s * sd, s * sa + c * sc, s * sb + c * sd
    mc = np.asarray(map_cov, dtype=np.float64).reshape(4)
    s00, s01 = t00 * c - t01 * s + _mp(mc[0]), t00 * s + t01 * c + _mp(mc[1])
    s10, s11 = t10 * c - t11 * s + _mp(mc[2]), t10 * s + t11 * c + _mp(mc[3])
    det = s00 * s11 - s10 * s01
    e0, e1 = _mp(ux) - _mp(map_mean[0]), _mp(uy) - _mp(map_mean[1])
    q = (e0 * (s11 * e0 - s01 * e1) + e1 * (s00 * e1 - s10 * e0)) / det
    return _mp(d1) * mpmath.exp(-_mp(d2) / 2 * q), det / (s00 * s11)


def weights_exact(ndt_map, states, means, covs, w0=None, minimum_likelihood=0.0, d1=1.0, d2=1.0, kernel=DEFAULT_KERNEL, variant=REFERENCE):
    """The weight w0 (1 + sum over the measurement cells of max(sum over the kernel's offsets of the likelihood, minimum)).

    The transformed mean (ux, uy) and the centre key come from the reference's own f64 sequence (moved_mean, cell_key): they are what
    the reference, and any correct kernel, computes bit for bit, and they are INPUTS of what follows - the error e = (ux, uy) - map mean
    uses the rounded ux.  Everything behind them is 60-digit arithmetic from the input doubles: the rotated covariance, its sum with the
    map cell's, the inverse, the quadratic form, exp, the sums, the max, 1 + sum and the product with the prior weight; the result is
    rounded to f64 once.  Returns (weights[n], keys[n][K] of (cx, cy), nearest: the smallest |ux inv - round(ux inv)| over both
    components that occurred, as a double, thinnest: the smallest det(S) / (s00 s11) over the cells that were hit, 1.0 if none)."""
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    means = np.asarray(means, dtype=np.float64).reshape(-1, 2)
    covs = np.asarray(covs, dtype=np.float64).reshape(-1, 2, 2)
    w0 = np.ones(len(states)) if w0 is None else np.asarray(w0, dtype=np.float64)
    inv = np.float64(1.0) / np.float64(ndt_map.resolution)
    out, all_keys = np.empty(len(states)), []
    nearest, thinnest = math.inf, mpmath.mpf(1)
    floor_term = _mp(minimum_likelihood)
    for i, st in enumerate(states):
        acc, row = mpmath.mpf(1), []
        for m, cv in zip(means, covs):
            ux, uy, centre = centre_key(ndt_map, st, m, variant)
            row.append(centre)
            with np.errstate(all="ignore"):
                for t in (ux * inv, uy * inv):
                    if np.isfinite(t):
                        nearest = min(nearest, float(abs(t - np.rint(t))))
            total = mpmath.mpf(0)
            for k in neighbours(ndt_map, kernel, centre, variant):
                if k is None:
                    continue
                value, thin = likelihood_exact(ux, uy, st, cv, ndt_map.data[k][0], ndt_map.data[k][1], d1, d2, variant.transposed)
                total += value
                thinnest = min(thinnest, thin)
            acc += max(total, floor_term)
        out[i] = float(acc * _mp(w0[i]))
        all_keys.append(row)
    return out, all_keys, nearest, float(thinnest)


def centre_keys_f64(ndt_map, states, means):
    """The loop form's centre keys (NdtMap.cell_near of transform_cell's mean), [n][K]."""
    return [[ndt_map.cell_near(transform_cell(st, m, np.eye(2))[0]) for m in np.asarray(means).reshape(-1, 2)]
            for st in np.asarray(states, dtype=np.float64).reshape(-1, 4)]


def revealing_map(keys, resolution, spread=1.5, seed=0):
    """Map cells for `keys` on which ONE wrong cell shows: every cell's mean at a place of its own inside its cell (0.2 .. 0.8 of it), its
    covariance with eigenvalues between 1 and 4 times (spread resolution)^2 along a direction of its own - condition number at most 4 -
    so that with spread cells of reach every cell within a kernel's reach contributes a visible share of a measurement cell's
    likelihood and no two cells contribute alike: a centre one cell off drops and adds cells, and the sum moves by far more than 1e-3
    of it (test_ndt_reference_cpu.py measures that on the engineered points).  A cell's values depend on its key alone."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    means, covs = np.empty((len(keys), 2)), np.empty((len(keys), 2, 2))
    for i, (kx, ky) in enumerate(keys):
        rng = np.random.Generator(np.random.PCG64([int(kx) & 0xFFFFFFFF, int(ky) & 0xFFFFFFFF, seed]))
        means[i] = (np.array([kx, ky], dtype=np.float64) + rng.uniform(0.2, 0.8, 2)) * resolution
        l1, l2 = rng.uniform(1.0, 4.0, 2) * (spread * resolution) ** 2
        a = rng.uniform(0.0, math.pi)
        ca, sa = math.cos(a), math.sin(a)
        b = (l1 - l2) * ca * sa
        covs[i] = [[l1 * ca * ca + l2 * sa * sa, b], [b, l1 * sa * sa + l2 * ca * ca]]
    return means, covs
