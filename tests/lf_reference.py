"""The exact reference of the likelihood-field cell decision and weight (plain numpy and Python, no device, nothing compiled).

The cell rule (the contract every kernel form is held to, tests/test_gpu_lf_edges.py):

    T = world_to_field * state                      (likelihood_field_model.hpp:70, Sophus' operation order: csrc/se2.h)
    x = px * cos - py * sin + tx,  y = px * sin + py * cos + ty        each product and sum rounded on its own
    v = x * (1 / resolution)                                           (regular_grid.hpp:75-78)
    cell = floor(v) on each axis; the end-point is IN the grid iff 0 <= xi < W and 0 <= yi < H   (dense_grid.hpp:92-96)
    an end-point whose v is NaN or +-inf, or whose |floor(v)| >= 2^31, has NO cell: it is not in the grid
    a beam's term is pz^3 of pz = double(float field value), or of double(float(1 / max_laser_distance)) outside the grid

The last-but-one line is written out because the reference leaves it to static_cast<int>, which is undefined there; as compiled for the
oracle it gives INT_MIN, "not contained" (recorded by tests/test_lf_reference_cpu.py).  numpy's float64 arithmetic does not contract, so
`cells` is bit-identical to oracle/beluga_oracle.cpp's lf_cell.

Also here: the fast kernels' FMA evaluation v~ in exact rational arithmetic with one rounding per fma, in the order of issue_fast
(csrc/kernels.hip); the margins of an end-point from the nearest cell boundary; the cell rules a wrong kernel would implement (MUTANTS);
and fields on which one wrong cell moves a weight visibly (revealing_field).
"""
import math
from fractions import Fraction

import numpy as np

FAST_MAGIC = 1572864.0      # 1.5 * 2^20 (kFastMagic): v~ + FAST_MAGIC has 32 fraction bits in its low word
FAST_BIAS = 0x41380000      # its high word (kFastBias)
TRIGGER = 2.0 ** -33        # the low word is zero iff v~ lies within this of an integer (round to nearest, ties to even)
GUARD_CELLS = 16384.0       # a wave holding a particle at or beyond this many cells from the grid origin takes the exact path
INT_LIMIT = 2.0 ** 31


# ---- SE(2) as csrc/se2.h does it (vectorised over the second operand) -------------------------------------------------------------
def _rot_from_complex(re, im):
    length = np.hypot(re, im)
    return re / length, im / length


def _rot_mul(ac, as_, bc, bs):
    re = ac * bc - as_ * bs
    im = ac * bs + as_ * bc
    n2 = re * re + im * im
    with np.errstate(all="ignore"):
        scale = 2.0 / (1.0 + n2)
    fix = n2 != 1.0
    re = np.where(fix, re * scale, re)
    im = np.where(fix, im * scale, im)
    return _rot_from_complex(re, im)


def pose_inverse(a):
    c, s = _rot_from_complex(np.float64(a[0]), -np.float64(a[1]))
    px, py = np.float64(a[2]) * -1.0, np.float64(a[3]) * -1.0
    return np.array([c, s, c * px - s * py, s * px + c * py])


def pose_mul(a, b):
    """a: one pose (cos, sin, x, y); b: [n, 4].  pose_mul of se2.h, row by row."""
    b = np.asarray(b, dtype=np.float64).reshape(-1, 4)
    ac, as_, ax, ay = (np.float64(v) for v in a)
    c, s = _rot_mul(ac, as_, b[:, 0], b[:, 1])
    x = ax + (ac * b[:, 2] - as_ * b[:, 3])
    y = ay + (as_ * b[:, 2] + ac * b[:, 3])
    return np.stack([c, s, x, y], axis=1)


def transforms(origin, states):
    """world_to_field * state for every state: [n, 4] (likelihood_field_model.hpp:70, likelihood_field_model_base.hpp:99)."""
    return pose_mul(pose_inverse(np.asarray(origin, dtype=np.float64)), states)


def end_points(resolution, origin, states, points):
    """(vx, vy), each [n, B]: the end-points in cells, separately rounded (likelihood_field_model.hpp:82-83, regular_grid.hpp:76)."""
    T = transforms(origin, states)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    ct, st, xt, yt = (T[:, k][:, None] for k in range(4))
    px, py = p[:, 0][None, :], p[:, 1][None, :]
    inv = np.float64(1.0) / np.float64(resolution)
    with np.errstate(all="ignore"):
        x = px * ct - py * st + xt
        y = px * st + py * ct + yt
        return x * inv, y * inv


def cell_of(v):
    """(cell as int64, has_cell): floor, and the written rule for values without an int32 cell."""
    with np.errstate(all="ignore"):
        f = np.floor(v)
        ok = np.isfinite(f) & (np.abs(f) < INT_LIMIT)
    return np.where(ok, f, 0.0).astype(np.int64), ok


def cells(field_shape, resolution, origin, states, points):
    """(xi, yi, inside), each [n, B].  xi, yi are meaningful where the end-point has a cell (0 elsewhere; such a point is not inside)."""
    H, W = field_shape
    vx, vy = end_points(resolution, origin, states, points)
    xi, okx = cell_of(vx)
    yi, oky = cell_of(vy)
    inside = okx & oky & (xi >= 0) & (yi >= 0) & (xi < W) & (yi < H)
    return xi, yi, inside


def unknown_value(max_laser_distance):
    return np.float32(1.0 / max_laser_distance)  # likelihood_field_model.hpp:75


def beam_values(field, max_laser_distance, xi, yi, inside):
    """pz per end-point as float64 widened from float32 (the kernels' tables hold exactly these)."""
    field = np.asarray(field, dtype=np.float32)
    H, W = field.shape
    flat = np.clip(yi, 0, H - 1) * W + np.clip(xi, 0, W - 1)
    got = field.reshape(-1)[flat]
    return np.where(inside, got, unknown_value(max_laser_distance)).astype(np.float64)


def weights(field, resolution, origin, max_laser_distance, states, points, rule=None):
    """1 + sum pz^3 per particle (likelihood_field_model.hpp:76-88), the sum exact (math.fsum) and rounded once.  rule: a mutant."""
    xi, yi, inside = (rule or cells)(np.shape(field), resolution, origin, states, points)
    pz = beam_values(field, max_laser_distance, xi, yi, inside)
    t = pz * pz * pz
    return np.array([math.fsum([1.0] + row.tolist()) for row in t])


def weights_prob(field, resolution, origin, max_laser_distance, states, points, rule=None):
    """exp(sum log pz) (likelihood_field_prob_model.hpp:77-90), the sum exact."""
    xi, yi, inside = (rule or cells)(np.shape(field), resolution, origin, states, points)
    pz = beam_values(field, max_laser_distance, xi, yi, inside)
    return np.array([math.exp(math.fsum(math.log(z) for z in row)) for row in pz])


# ---- the fast kernels' evaluation, exactly -------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding (to nearest even)


def fast_end_points(resolution, origin, states, points, pairs=None):
    """v~ of issue_fast: fma(px, ict, fma(-py, ist, ixt)), fma(px, ist, fma(py, ict, iyt)) with the pose pre-multiplied by 1 / res.
    pairs: iterable of (particle, point) to evaluate (others NaN); None = all.  Returns (vx~, vy~) [n, B]."""
    T = transforms(origin, states)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    inv = np.float64(1.0) / np.float64(resolution)
    n, B = len(T), len(p)
    ox, oy = np.full((n, B), np.nan), np.full((n, B), np.nan)
    it = pairs if pairs is not None else ((i, b) for i in range(n) for b in range(B))
    for i, b in it:
        ict, ist, ixt, iyt = (float(T[i, k] * inv) for k in range(4))
        px, py = float(p[b, 0]), float(p[b, 1])
        if not all(map(math.isfinite, (px, py, ict, ist, ixt, iyt))):
            continue
        ox[i, b] = _fma(px, ict, _fma(-py, ist, ixt))
        oy[i, b] = _fma(px, ist, _fma(py, ict, iyt))
    return ox, oy


def fast_cell(vt):
    """What the fast kernels read from v~ + 1.5 * 2^20: (cell by the high word, low word).  Valid for |v~| < 2^19."""
    s = np.asarray(vt, dtype=np.float64) + FAST_MAGIC
    bits = s.view(np.uint64) if s.ndim else np.array([s]).view(np.uint64)
    lo = (bits & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hi = (bits >> np.uint64(32)).astype(np.int64) - FAST_BIAS
    return hi.reshape(np.shape(vt)), lo.reshape(np.shape(vt))


def distance_to_integer(v):
    """|v - nearest integer| in cells (exact: the subtraction of two close doubles), and in ulps of v (inf next to 0)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.rint(v)
        d = np.abs(v - r)
        same = (r != 0) & np.isfinite(v)
        a = np.where(same, np.abs(v), 1.0).view(np.int64)
        b = np.where(same, np.abs(r), 1.0).view(np.int64)
    return d, np.where(same, np.abs(a - b).astype(np.float64), np.where(d == 0, 0.0, np.inf))


def margins(resolution, origin, states, points, pairs=None):
    """Per end-point and axis: the distance of v from the nearest integer in cells and in ulps of v, and the same for the fast kernels'
    v~ (exact rational evaluation; only for `pairs` if given).  dict of [n, B] arrays."""
    vx, vy = end_points(resolution, origin, states, points)
    tx, ty = fast_end_points(resolution, origin, states, points, pairs)
    out = {"vx": vx, "vy": vy, "vx_fast": tx, "vy_fast": ty}
    for name, v in (("x", vx), ("y", vy), ("x_fast", tx), ("y_fast", ty)):
        out["cells_" + name], out["ulps_" + name] = distance_to_integer(v)
    return out


# ---- cell rules a wrong kernel would implement ---------------------------------------------------------------------------------------
def _rule_from(fx, contains=None):
    def rule(field_shape, resolution, origin, states, points):
        H, W = field_shape
        vx, vy = end_points(resolution, origin, states, points)
        xi, okx = fx(vx)
        yi, oky = fx(vy)
        inside = okx & oky & ((xi >= 0) & (yi >= 0) & (xi < W) & (yi < H) if contains is None else contains(xi, yi, W, H))
        return xi, yi, inside
    return rule


def _floor_like(op):
    def fx(v):
        with np.errstate(all="ignore"):
            f = op(v)
            ok = np.isfinite(f) & (np.abs(f) < INT_LIMIT)
        return np.where(ok, f, 0.0).astype(np.int64), ok
    return fx


def _cell0_for_non_finite(v):  # the low mantissa word of NaN + 1.5 * 2^52 or of an infinity: 0
    xi, ok = cell_of(v)
    return xi, ok | ~np.isfinite(v)


def _wrap(v):  # the low mantissa word of v + 1.5 * 2^52 for any finite v: floor(v) modulo 2^32 as int32; 0 for NaN and infinities
    with np.errstate(all="ignore"):
        f = np.floor(v)
    fin = np.isfinite(f) & (np.abs(f) < 2.0 ** 62)
    w = np.where(fin, f, 0.0).astype(np.int64)
    w = ((w + 2 ** 31) % 2 ** 32) - 2 ** 31
    return w, np.ones(np.shape(v), dtype=bool)


def _fast_rule(fallback_within, guard):
    """Cells from v~ by the high word; the exact cell instead where v~ lies within `fallback_within` of an integer (None: never) and, with
    `guard`, for every end-point of a particle at or beyond GUARD_CELLS.  (The kernels redo a whole group or wave: no other cells.)"""
    def rule(field_shape, resolution, origin, states, points):
        H, W = field_shape
        xi, yi, inside = cells(field_shape, resolution, origin, states, points)
        tx, ty = fast_end_points(resolution, origin, states, points)
        T = transforms(origin, states)
        inv = 1.0 / np.float64(resolution)
        far = ~((np.abs(T[:, 2] * inv) < GUARD_CELLS) & (np.abs(T[:, 3] * inv) < GUARD_CELLS))
        out = []
        for v, exact in ((tx, xi), (ty, yi)):
            ok = np.isfinite(v) & (np.abs(v) < 2.0 ** 19)
            hi, _ = fast_cell(np.where(ok, v, 0.0))
            take = ok.copy()
            if fallback_within is not None:
                take &= distance_to_integer(np.where(ok, v, 0.5))[0] > fallback_within
            if guard:
                take &= ~far[:, None]
            out.append(np.where(take, hi, exact))
        fx, fy = out
        vx, vy = end_points(resolution, origin, states, points)
        has = cell_of(vx)[1] & cell_of(vy)[1]  # (a point without a cell never reaches a kernel, or is out of contract)
        return fx, fy, has & (fx >= 0) & (fy >= 0) & (fx < W) & (fy < H)
    return rule


MUTANTS = {
    "truncate": _rule_from(_floor_like(np.trunc)),                       # toward zero: cell -1 becomes 0
    "nearest": _rule_from(_floor_like(np.rint)),
    "bounds_le": _rule_from(cell_of, lambda xi, yi, W, H: (xi >= 0) & (yi >= 0) & (xi <= W) & (yi <= H)),
    "fma_no_fallback": _fast_rule(None, True),
    "fma_trigger_halved": _fast_rule(TRIGGER / 2, True),
    "fma_no_guard": _fast_rule(TRIGGER, False),
    "non_finite_is_cell_0": _rule_from(_cell0_for_non_finite),
    "wrap_mod_2_32": _rule_from(_wrap),
}
# The fast rule as the kernels implement it: held to `cells` like everything else (test_lf_reference_cpu.py).
FAST_RULE = _fast_rule(TRIGGER, True)


# ---- fields on which a wrong cell shows ------------------------------------------------------------------------------------------------
PALETTE_VALUES = (np.float32(0.2) + np.float32(0.0625) * np.arange(17, dtype=np.float32)).astype(np.float32)  # 0.2 .. 1.2, exact


def revealing_field(H, W, kind):
    """kind="palette": value[(3x + 5y) mod 17] of 17 float32 values 0.0625 apart in [0.2, 1.2] - all eight neighbours of a cell differ
    from it (3dx + 5dy is no multiple of 17 for |dx|, |dy| <= 1) and none is the unknown value; few values: the palette table engages.
    kind="cube": every cell another value in [0.2, 1.2), seeded (more than a palette holds once the grid has over 2048 cells)."""
    if kind == "palette":
        y, x = np.mgrid[0:H, 0:W]
        return PALETTE_VALUES[(3 * x + 5 * y) % 17].astype(np.float32)
    assert kind == "cube" and H * W < 2 ** 22
    order = np.random.Generator(np.random.MT19937(1234)).permutation(H * W)
    return (0.2 + order.astype(np.float64) / (H * W)).astype(np.float32).reshape(H, W)
