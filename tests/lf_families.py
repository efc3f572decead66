"""Inputs shared by tests/test_lf_reference_cpu.py and tests/test_gpu_lf_edges.py: scans whose end-points are ENGINEERED to sit where the
likelihood-field kernels' cell decisions can go wrong.  Deterministic; no device.

A family is a function returning a list of cases; a case is a dict
    shape (H, W), resolution, origin (cos, sin, x, y), states [m, 4], points [B, 2],
    pairs: [(particle, point, axis, tag)] - the engineered end-points (a scan point is special for ONE pose; for the others it is an
           ordinary point), axis "x" / "y" / "xy",
    targets: what the case is for.
End-points are engineered by solving for the scan point that puts pose i's end-point on the wanted value and then searching the
neighbouring doubles (steps of one ulp of px and py) for one whose end-point - by lf_reference's own separately rounded arithmetic, or
by a long-double stand-in for the fast kernels' FMA evaluation that the CPU test then checks exactly - satisfies the family's condition.
"""
import functools

import numpy as np

import lf_reference as ref


def se2(x, y, theta):
    return np.array([np.cos(theta), np.sin(theta), x, y])


GRID_A = dict(shape=(157, 203), resolution=0.05, origin=se2(3.0, -2.0, 0.7))    # inexact reciprocal, rotated, sides no multiples of 8
GRID_B = dict(shape=(90, 120), resolution=0.1, origin=se2(-4.0, 1.0, -0.3))


def poses_in(grid, m, seed, lo=0.15, hi=0.85):
    """m poses with general headings at random places inside the grid: states [m, 4] in the world frame."""
    rng = np.random.Generator(np.random.MT19937(seed))
    H, W = grid["shape"]
    fx, fy = rng.uniform(lo * W, hi * W, m) * grid["resolution"], rng.uniform(lo * H, hi * H, m) * grid["resolution"]
    oc, os_, ox, oy = grid["origin"]
    th = rng.uniform(-np.pi, np.pi, m)
    return np.stack([np.cos(th), np.sin(th), ox + oc * fx - os_ * fy, oy + os_ * fx + oc * fy], axis=1)


def _ulp_steps(x, k):
    return (np.array([x], dtype=np.float64).view(np.int64)[0] + k).view(np.float64)


def _fast_standin(T, inv, px, py):
    """The fast kernels' v~ with every fma evaluated in long double and rounded to double (exact but for rare double roundings)."""
    L = np.longdouble
    ict, ist, ixt, iyt = (np.float64(T[k] * inv) for k in range(4))
    ix = (L(-py) * L(ist) + L(ixt)).astype(np.float64)
    iy = (L(py) * L(ict) + L(iyt)).astype(np.float64)
    return (L(px) * L(ict) + L(ix)).astype(np.float64), (L(px) * L(ist) + L(iy)).astype(np.float64)


def engineer(T, resolution, target, pred, rx=48, ry=48, prefer=None):
    """The scan point (px, py) next to the solution of `end-point of pose T = target cells` whose end-point satisfies pred(vx, vy, tx, ty)
    (arrays; tx, ty the FMA stand-in); among several, one that also satisfies `prefer` if any, else the nearest.  None if there is none."""
    ct, st, xt, yt = (np.float64(v) for v in T)
    inv = np.float64(1.0) / np.float64(resolution)
    dx, dy = target[0] * resolution - xt, target[1] * resolution - yt
    px0, py0 = ct * dx + st * dy, -st * dx + ct * dy
    PX = _ulp_steps(px0, np.arange(-rx, rx + 1, dtype=np.int64))[:, None]
    PY = _ulp_steps(py0, np.arange(-ry, ry + 1, dtype=np.int64))[None, :]
    vx = (PX * ct - PY * st + xt) * inv
    vy = (PX * st + PY * ct + yt) * inv
    tx, ty = _fast_standin(T, inv, PX, PY)
    ok = pred(vx, vy, tx, ty)
    if not ok.any():
        return None
    cost = np.abs(np.arange(-rx, rx + 1))[:, None] + np.abs(np.arange(-ry, ry + 1))[None, :] + 0.0
    if prefer is not None:
        cost = cost + np.where(prefer(vx, vy, tx, ty), 0.0, 1e9)
    cost = np.where(ok, cost, np.inf)
    a, b = np.unravel_index(np.argmin(cost), cost.shape)
    return float(PX[a, 0]), float(PY[0, b]), bool(cost[a, b] < 1e9)


def stepped(k, j):
    """The double j ulps above (j > 0) or below the integer k."""
    v = np.float64(k)
    for _ in range(abs(j)):
        v = np.nextafter(v, np.inf if j > 0 else -np.inf)
    return v


def _mid(v):  # comfortably inside a cell
    f = v - np.floor(v)
    return (f > 0.2) & (f < 0.8)


def _case(grid, states, points, pairs, targets):
    return dict(shape=grid["shape"], resolution=grid["resolution"], origin=np.asarray(grid["origin"], dtype=np.float64),
                states=np.asarray(states, dtype=np.float64), points=np.asarray(points, dtype=np.float64).reshape(-1, 2), pairs=pairs,
                targets=targets)


def _fma_differs(vx, vy, tx, ty):
    return (np.floor(vx) != np.floor(tx)) | (np.floor(vy) != np.floor(ty))


def _build(grid, states, requests, targets, filler_seed=1, filler=5):
    """requests: (particle, target cells, pred, axis, tag, kwargs).  A few ordinary points go in front, so that engineered points sit at
    all positions of the kernels' groups."""
    T = ref.transforms(grid["origin"], states)
    rng = np.random.Generator(np.random.MT19937(filler_seed))
    points = [(r * np.cos(a), r * np.sin(a)) for r, a in zip(rng.uniform(0.3, 3.0, filler), rng.uniform(-np.pi, np.pi, filler))]
    pairs = []
    for i, target, pred, axis, tag, kw in requests:
        # (several alternative (target, pred) for one request: the first whose point also has the preferred property, else the last found)
        got = None
        for t, p in (zip(target, pred) if isinstance(pred, list) else ((target, pred),)):
            found = engineer(T[i], grid["resolution"], t, p, **kw)
            got = found or got
            if found and found[2]:
                break
        if got is None:
            continue
        pairs.append((i, len(points), axis, tag))
        points.append(got[:2])
    return _case(grid, states, points, pairs, targets)


@functools.lru_cache(maxsize=None)
def ulp_straddle():
    """End-points -4 .. +4 ulps of a cell boundary on x, on y and on both, general headings, resolutions with inexact reciprocals, rotated
    origins; where the search finds one, an end-point on which the FMA evaluation falls on the other side of the boundary."""
    out = []
    for g, grid in enumerate((GRID_A, GRID_B)):
        H, W = grid["shape"]
        states = poses_in(grid, 6, seed=10 + g)
        rng = np.random.Generator(np.random.MT19937(20 + g))
        req = []
        for i in range(len(states)):
            for axis in ("x", "y", "xy"):
                for j in range(-4, 5):
                    preds, targets = [], []
                    for _ in range(6):  # boundaries to try for one on which the FMA evaluation errs
                        kx, ky = int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))
                        wx, wy = stepped(kx, j), stepped(ky, j)
                        if axis == "x":
                            pred, target = (lambda vx, vy, tx, ty, wx=wx: (vx == wx) & _mid(vy)), (kx, ky + 0.5)
                        elif axis == "y":
                            pred, target = (lambda vx, vy, tx, ty, wy=wy: (vy == wy) & _mid(vx)), (kx + 0.5, ky)
                        else:
                            pred, target = (lambda vx, vy, tx, ty, wx=wx, wy=wy: (vx == wx) & (vy == wy)), (kx, ky)
                        preds.append(pred)
                        targets.append(target)
                    req.append((i, targets, preds, axis, j, dict(prefer=_fma_differs)))
        out.append(_build(grid, states, req, "v at -4 .. +4 ulps of a cell boundary; the FMA evaluation on the other side where found"))
    return out


RING = tuple(s * f * t for t in (ref.TRIGGER, 2 * ref.TRIGGER) for f in (1 - 2.0 ** -6, 1 + 2.0 ** -6) for s in (-1.0, 1.0))


def _ring_requests(i, kx, ky, tol):
    req = []
    for axis in ("x", "y"):
        for d in RING:
            if axis == "x":
                pred = lambda vx, vy, tx, ty, d=d, k=kx: (np.abs((tx - k) - d) <= tol) & _mid(vy)
                target, kw = (kx + d, ky + 0.5), dict(rx=40000, ry=1)
            else:
                pred = lambda vx, vy, tx, ty, d=d, k=ky: (np.abs((ty - k) - d) <= tol) & _mid(vx)
                target, kw = (kx + 0.5, ky + d), dict(rx=1, ry=40000)
            req.append((i, target, pred, axis, d, kw))
    return req


@functools.lru_cache(maxsize=None)
def trigger_ring():
    """v~ at (1 -+ 2^-6) 2^-33 and (1 -+ 2^-6) 2^-32 either side of an integer: just inside and just outside the zero-low-word fallback
    (and the patch kernel's `low word < 4`).  Poses with |cos| and |sin| both large, so that either coordinate of the point moves either
    axis finely."""
    out = []
    for g, grid in enumerate((GRID_A, GRID_B)):
        H, W = grid["shape"]
        states = poses_in(grid, 10, seed=30 + g)
        T = ref.transforms(grid["origin"], states)
        rng = np.random.Generator(np.random.MT19937(40 + g))
        req = []
        for i in range(len(states)):
            # vary the coordinate with the larger coefficient on the axis: swap the search's long side if needed
            kx, ky = int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))
            for r in _ring_requests(i, kx, ky, 2.0 ** -41):
                if abs(T[i][0]) < abs(T[i][1]):  # px moves y more than x
                    r[5]["rx"], r[5]["ry"] = r[5]["ry"], r[5]["rx"]
                req.append(r)
        out.append(_build(grid, states, req, "v~ just inside / outside the fallback's trigger, both sides of a cell boundary"))
    return out


@functools.lru_cache(maxsize=None)
def borders():
    """v within ulps of -1, W-1, W, H-1, H and either side of 0, and inside [-1, 0), under rotation; the negative-zero product."""
    out = []
    for g, grid in enumerate((GRID_A, GRID_B)):
        H, W = grid["shape"]
        states = poses_in(grid, 6, seed=50 + g, lo=0.05, hi=0.95)
        rng = np.random.Generator(np.random.MT19937(60 + g))
        req = []
        for i in range(len(states)):
            for axis, side, other in (("x", W, H), ("y", H, W)):
                for k in (-1, 0, side - 1, side):
                    for j in (-2, -1, 0, 1, 2):
                        o = float(rng.integers(2, other - 2)) + 0.5
                        if k <= 0:  # the sum that ends near 0 or -1 cancels a translation of ~100 cells: its values lie ~2^-46 apart, an
                            # ulp of the result says nothing - the value itself and the nearest ones the arithmetic produces either side
                            near = lambda v, k=k, j=j: (v == k) if j == 0 else ((v < k) & (v > k - 2.0 ** -40)) if j < 0 else ((v > k) & (v < k + 2.0 ** -40))
                        else:
                            near = lambda v, w=stepped(k, j): v == w
                        kw = dict(rx=300, ry=300) if (k <= 0 and j == 0) else {}  # an exact hit is one candidate in ~50
                        if axis == "x":
                            req.append((i, (k, o), (lambda vx, vy, tx, ty, near=near: near(vx) & _mid(vy)), axis, (k, j), kw))
                        else:
                            req.append((i, (o, k), (lambda vx, vy, tx, ty, near=near: near(vy) & _mid(vx)), axis, (k, j), kw))
                for f in (0.03, 0.5, 0.97):  # inside [-1, 0)
                    o = float(rng.integers(2, other - 2)) + 0.5
                    inside = lambda v: (v > -1) & (v < 0)
                    if axis == "x":
                        req.append((i, (-1 + f, o), (lambda vx, vy, tx, ty: inside(vx) & _mid(vy)), axis, (-1, "in"), {}))
                    else:
                        req.append((i, (o, -1 + f), (lambda vx, vy, tx, ty: inside(vy) & _mid(vx)), axis, (-1, "in"), {}))
        out.append(_build(grid, states, req, "cells -1 / 0 and W-1 / W, H-1 / H under rotation"))
    # the negative-zero product: an unrotated grid at the world's origin, poses on its origin, points with zero coordinates of either sign
    grid = dict(shape=(9, 9), resolution=0.05, origin=se2(0.0, 0.0, 0.0))
    states = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.05, 0.1]])
    points = [(-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, 0.07), (0.07, -0.0), (-0.05, -0.1)]
    pairs = [(i, b, "xy", "zero") for i in range(len(states)) for b in range(len(points))]
    out.append(_case(grid, states, points, pairs, "end-points that are +0 or -0: cell 0, inside"))
    return out


@functools.lru_cache(maxsize=None)
def small_grids():
    """Grids below and astride one 8x8 palette tile and the 64-cell patch: W x H = 1x1, 1x9, 9x1, 7x9, 65x63."""
    out = []
    for g, (W, H) in enumerate(((1, 1), (1, 9), (9, 1), (7, 9), (65, 63))):
        grid = dict(shape=(H, W), resolution=0.05, origin=se2(0.4, -0.3, 0.5 + 0.3 * g))
        rng = np.random.Generator(np.random.MT19937(70 + g))
        m, B = 8, 48
        # poses and end-points over the grid and two cells around it
        fx, fy = rng.uniform(-2, W + 2, m) * 0.05, rng.uniform(-2, H + 2, m) * 0.05
        oc, os_, ox, oy = grid["origin"]
        th = rng.uniform(-np.pi, np.pi, m)
        states = np.stack([np.cos(th), np.sin(th), ox + oc * fx - os_ * fy, oy + os_ * fx + oc * fy], axis=1)
        r, a = rng.uniform(0.0, 0.05 * (max(W, H) + 2), B), rng.uniform(-np.pi, np.pi, B)
        points = np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
        pairs = [(i, b, "xy", "any") for i in range(m) for b in range(B)]
        out.append(_case(grid, states, points, pairs, "a %d x %d grid" % (W, H)))
    return out


GROUP_OF_8_COUNTS = tuple(range(0, 42))                                            # 0 .. 5 groups x tails 0 .. 7
LANE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 319, 320, 511, 512, 513)            # lanes over beams: rounds of 64, blocks of 256
# Segmented launches (launch_reweight_lf in csrc/kernels.hip): 16 411 particles are 257 waves, so the scan is split into
# s = min(ceil(4096 / 257) = 16, B / 64) segments of per = ceil(B / s) beams, the last one taking what is left: B - (s - 1) * per.
#   129 -> 2 segments: 65 + 64          193 -> 3: 65 + 65 + 63           1009 -> 15 segments of 68, the last of 57
#   1025 -> 16 of 65, the last of 50    1041 -> 16 of 66, the last of 51 (6 groups of 8 and a tail of 3)
# The last segment is never shorter than B - (s - 1) * ceil(B / s) >= B / s - (s - 1) > 48 beams here: one with a SINGLE beam cannot be
# reached through the library (s <= B / 64), so the shortest reachable ones stand in for it.
SEGMENT_COUNTS = (129, 193, 1009, 1025, 1041)


@functools.lru_cache(maxsize=None)
def beam_counts():
    """One scan of 1041 points over GRID_A; the tests take its first B points for every B of the count lists above."""
    grid = GRID_A
    states = poses_in(grid, 8, seed=80)
    rng = np.random.Generator(np.random.MT19937(81))
    r, a = rng.uniform(0.2, 9.0, 1041), rng.uniform(-np.pi, np.pi, 1041)
    points = np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
    return [_case(grid, states, points, [], "every prologue, loop and epilogue shape of the pipelined loops")]


NO_CELL_POINTS = ((np.nan, np.nan), (np.inf, np.inf), (-np.inf, -np.inf), (np.nan, 0.7), (0.7, np.inf), (-np.inf, 0.3))


def _huge_points(resolution):  # finite, but |v| >= 2^31 for the poses of the case: OUT OF CONTRACT on the device
    return ((1e300, 1e300), ((2.0 ** 31 + 1) * resolution * 2, 0.0), (-(2.0 ** 31 + 1) * resolution * 2, 0.0),
            (0.0, (2.0 ** 31 - 1) * resolution * 2), (0.0, -(2.0 ** 31 - 1) * resolution * 2))


@functools.lru_cache(maxsize=None)
def no_cell(include_finite=False):
    """Scan points without a cell mixed into an ordinary scan of 41 points: first, last, inside a group of 8, inside the tail.  With
    include_finite (the CPU reference only): finite points so large that |v| >= 2^31 as well."""
    grid = GRID_A
    states = poses_in(grid, 8, seed=90)
    rng = np.random.Generator(np.random.MT19937(91))
    r, a = rng.uniform(0.2, 4.0, 41), rng.uniform(-np.pi, np.pi, 41)
    base = [tuple(p) for p in np.stack([r * np.cos(a), r * np.sin(a)], axis=1)]
    bad = list(NO_CELL_POINTS) + (list(_huge_points(grid["resolution"])) if include_finite else [])
    out = []
    for places in ((0,), (-1,), (3,), (11, 12), (0, 5, 17, 38, -1), tuple(range(0, 41, 3))):
        points = list(base)
        pairs = []
        for n_, at in enumerate(places):
            points[at] = bad[(n_ + len(places)) % len(bad)]
        for b, p in enumerate(points):
            if p in bad or any(np.isnan(p)):
                pairs += [(i, b, "xy", "no cell") for i in range(len(states))]
        out.append(_case(grid, states, points, pairs, "points without a cell at scan positions %s" % (places,)))
    out.append(_case(grid, states, bad * 3, [(i, b, "xy", "no cell") for i in range(len(states)) for b in range(3 * len(bad))],
                     "a scan of nothing but points without a cell"))
    return out


@functools.lru_cache(maxsize=None)
def long_lever():
    """Particles 16 383.5 and 16 384.5 cells from the grid origin along x and along y - either side of the fast kernels' per-wave guard -
    among particles near the origin, beams of up to 8000 cells (the host sends scans of 8192 cells and more to the exact kernel) that
    end inside a 16 000-cell-long map: |px ict| < 2^13, |ixt| just under / over 2^14, end-points in [2^13, 2^14): one ulp of v is
    2^-39 cells, 2^-33 is 64 of them; end-points on the ring's offsets, which here are whole ulps (63 and 65, 126 and 130).
    (Diagonally the map would need 2^28 cells: left out.)"""
    out = []
    for along in ("x", "y"):
        W, H = (16000, 64) if along == "x" else (64, 16000)
        grid = dict(shape=(H, W), resolution=0.05, origin=se2(0.0, 0.0, 0.0))
        res = 0.05
        far = []
        for d in (16383.5, 16384.5):
            for th in (np.pi - 0.02, np.pi + 0.013) if along == "x" else (-np.pi / 2 + 0.02, -np.pi / 2 - 0.013):
                far.append(se2(d * res, 31.7 * res, th) if along == "x" else se2(31.7 * res, d * res, th))
        near = [se2(*(((100.0 + 7 * k) * res, 30.3 * res) if along == "x" else (30.3 * res, (100.0 + 7 * k) * res)), 0.3 + k) for k in range(4)]
        states = np.array(far + near)
        rng = np.random.Generator(np.random.MT19937(95))
        req = []
        for i in range(len(far)):
            for k_long in rng.integers(8500, 15900, 2):
                k_short = int(rng.integers(4, 60))
                kx, ky = (int(k_long), k_short) if along == "x" else (k_short, int(k_long))
                for r in _ring_requests(i, kx, ky, 0.0):
                    r[5]["rx"], r[5]["ry"] = 3000, 3  # the long axis moves with px (the beams point back along it)
                    req.append(r)
        out.append(_build(grid, states, req, "terms up to 2^15 cells, particles either side of the 2^14-cell guard, along " + along))
    return out


FAMILIES = {"ulp_straddle": ulp_straddle, "trigger_ring": trigger_ring, "long_lever": long_lever, "borders": borders,
            "small_grids": small_grids, "beam_counts": beam_counts, "no_cell": no_cell}
