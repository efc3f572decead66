"""beluga::estimate (algorithm/estimation.hpp:436-475) and the nine sums the kernels take it from, evaluated exactly, and the units
their errors are quoted in.

Plain Python and numpy; nothing here imports the code under test.  Two forms:
  * exact: every double is an integer times a power of two, so the sums are integer sums and the estimate is a ratio of integers
    (fractions.Fraction).  Used up to EXACT_MAX particles.
  * extended: numpy.longdouble where that is the x87 format (mpmath at 80 bits where it is not, as propagate_reference.py does), pairwise
    sums, the covariance in two passes about a mean that is itself taken about a particle of the set.  Used above EXACT_MAX; its own
    error is a few 2^-64 of a term, a hundredth of a unit below.
tests/test_estimate_reference_cpu.py holds the two to each other.

The nine sums about a pivot (px, py), as k_estimate_partials and its siblings define them, dx = x - px, dy = y - py:
    Sw, Sw^2, Sw c, Sw s, Sw dx, Sw dy, Sw dx^2, Sw dx dy, Sw dy^2
each with S|term|, the sum of the absolute values of its terms: the error of a sum is quoted in units of 2^-53 S|term|, the rounding of
one addition at the size of the whole sum.

The estimate (estimation.hpp:436-475, statistics at :262-281): with W = Sw and the normalised weights v = w / W,
    mean = S v x,    (mc, ms) = S v (cos, sin),    R = |(mc, ms)|
    cov_xy = S v (x - mean_x)(y - mean_y) / (1 - S v^2)                  (position block, :270)
    R < epsilon: heading = 0, cov_tt = infinity;  otherwise heading = (mc, ms) / R, cov_tt = -2 log R

The conditioned units, u = 2^-53.  D is the diagonal of the bounding box of the particles with w > 0.
  position    u max(|mean|, D): the rounding of the mean itself, or - for a set about the origin - of one offset within the set.
  covariance  u (D^2 + q T) / (1 - q), q = S v^2, T = cov_xx + cov_yy.  The biased second moment is a sum of terms of size up to D^2 for
              any pivot inside the box (|dx| <= D): one rounding of one term is u D^2.  The division by 1 - q carries that rounding, and the
              rounding of q itself (u q, relative to 1 - q: u q / (1 - q), times the covariance).  For a set of many comparable weights
              q is about 1 / n and the unit is u D^2; for a set whose mass sits on one particle 1 - q is small and no double-precision
              evaluation - the reference's own included - can do better than this.
  heading     u (1 + 1 / R): mc and ms are sums of terms of size up to 1, so one rounding moves them by u; the direction of a vector of
              length R moves by u / R, and normalising rounds once more.  Quoted as the distance between the (cos, sin) pairs.
  cov_tt      u (2 / R + |2 log R|): d(-2 log R) = -2 dR / R with dR = u, and the rounding of the logarithm itself.
A figure that is not finite where the reference's is (or the other way round) counts as infinitely wrong; where 1 - q is exactly zero
(one particle carries all the weight) the position covariance is 0 / 0 in the reference and must be NaN; where R < epsilon the heading
must be exactly (1, 0) and cov_tt exactly infinity.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import propagate_reference as xp

U = 2.0 ** -53
EPSILON = 2.0 ** -52  # std::numeric_limits<double>::epsilon()
EXACT_MAX = 4097
SUM_NAMES = ("w", "w2", "wc", "ws", "wdx", "wdy", "wdxdx", "wdxdy", "wdydy")

Sums = namedtuple("Sums", "value abs")  # nine exact (Fraction) or extended values; nine doubles S|term|
Estimate = namedtuple("Estimate", "x y cos sin cov_xx cov_xy cov_yy cov_tt degenerate singular R q D "
                                  "pos_unit cov_unit rot_unit tt_unit")
# x .. cov_tt: Fraction or extended scalars (cos, sin, cov_tt, R: extended); degenerate: R < epsilon; singular: 1 - q == 0


# ---- doubles as integers ---------------------------------------------------------------------------------------
def _ints(*arrays):
    """The doubles of every array on one scale: -> ([list of Python ints per array], e) with value = int * 2^e."""
    flat = [np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]
    parts = [np.frexp(a) for a in flat]
    exps = np.concatenate([e[m != 0] for m, e in parts]) if any((m != 0).any() for m, _ in parts) else np.array([53])
    e_min = int(exps.min()) - 53
    out = []
    for m, e in parts:
        mi = np.ldexp(m, 53).astype(np.int64)
        shift = np.where(m != 0, e - 53 - e_min, 0)
        out.append([int(a) << int(s) for a, s in zip(mi.tolist(), shift.tolist())])
    return out, e_min


def _scaled(value, e):
    return Fraction(value) * (Fraction(2) ** e)


def _split(states, w):
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    assert len(states) == len(w) and len(w) > 0
    return states, w


# ---- the nine sums -----------------------------------------------------------------------------------------------
def sums_exact(states, w, pivot):
    states, w = _split(states, w)
    (wi,), ew = _ints(w)
    (ci, si), er = _ints(states[:, 0], states[:, 1])
    (xi, yi, pi), ex = _ints(states[:, 2], states[:, 3], np.asarray(pivot, dtype=np.float64))
    dx = [v - pi[0] for v in xi]
    dy = [v - pi[1] for v in yi]
    terms = (
        (wi, ew), ([a * a for a in wi], 2 * ew), ([a * b for a, b in zip(wi, ci)], ew + er), ([a * b for a, b in zip(wi, si)], ew + er),
        ([a * b for a, b in zip(wi, dx)], ew + ex), ([a * b for a, b in zip(wi, dy)], ew + ex),
        ([a * b * b for a, b in zip(wi, dx)], ew + 2 * ex), ([a * b * c for a, b, c in zip(wi, dx, dy)], ew + 2 * ex),
        ([a * b * b for a, b in zip(wi, dy)], ew + 2 * ex),
    )
    value = [_scaled(sum(t), e) for t, e in terms]
    absolute = np.array([float(_scaled(sum(abs(v) for v in t), e)) for t, e in terms])
    return Sums(value, absolute)


def _ext_sum(a):
    """Pairwise: numpy's own for longdouble; for mpmath objects a tree of halves."""
    if a.dtype != object:
        return np.sum(a)
    while len(a) > 1:
        if len(a) % 2:
            a = np.concatenate([a, np.array([xp.ext(np.array([0.0]))[0]], dtype=object)])
        a = a[0::2] + a[1::2]
    return a[0]


def sums_extended(states, w, pivot):
    states, w = _split(states, w)
    we, c, s = xp.ext(w), xp.ext(states[:, 0]), xp.ext(states[:, 1])
    dx, dy = xp.ext(states[:, 2]) - xp.ext(np.array([pivot[0]]))[0], xp.ext(states[:, 3]) - xp.ext(np.array([pivot[1]]))[0]
    terms = (we, we * we, we * c, we * s, we * dx, we * dy, we * dx * dx, we * dx * dy, we * dy * dy)
    value = [_ext_sum(t) for t in terms]
    absolute = np.array([float(xp.to_f64(np.array([_ext_sum(xp.x_abs(t))]))[0]) for t in terms])
    return Sums(value, absolute)


def sums(states, w, pivot):
    return sums_exact(states, w, pivot) if len(w) <= EXACT_MAX else sums_extended(states, w, pivot)


def _to_ext(v):
    """A Fraction, or an extended scalar, as an extended scalar (a Fraction through its two leading doubles)."""
    if isinstance(v, Fraction):
        hi = float(v)
        lo = float(v - Fraction(hi)) if math.isfinite(hi) else 0.0
        return xp.ext(np.array([hi]))[0] + xp.ext(np.array([lo]))[0]
    return v


def _f(v):
    return float(xp.to_f64(np.array([_to_ext(v)]))[0])


def sum_errors(reference, got):
    """got: the nine doubles of mcl_estimate_sums -> their errors in units of 2^-53 S|term| (a sum of no terms at all must be 0)."""
    out = np.empty(9)
    for k in range(9):
        g = float(got[k])
        if not math.isfinite(g):
            out[k] = math.inf
            continue
        v = reference.value[k]
        diff = abs(float(Fraction(g) - v)) if isinstance(v, Fraction) else abs(_f(xp.ext(np.array([g]))[0] - v))
        unit = U * reference.abs[k]
        out[k] = diff / unit if unit > 0 else (0.0 if diff == 0 else math.inf)
    return out


def rounded_sums(reference, pivot):
    """The reference's sums rounded to double, as the twelve of mcl_estimate_from_sums."""
    return np.array([_f(v) for v in reference.value] + [float(pivot[0]), float(pivot[1]), 0.0])


# ---- the estimate --------------------------------------------------------------------------------------------------
def _box_diagonal(states, w):
    live = w > 0
    if not live.any():
        return 0.0
    x, y = states[live, 2], states[live, 3]
    return math.hypot(float(x.max()) - float(x.min()), float(y.max()) - float(y.min()))


def _finish(x, y, mc, ms, bxx, bxy, byy, q, D):
    """From exact or extended moments (b: the biased second moments about the mean) to the Estimate and its units."""
    one = Fraction(1) if isinstance(q, Fraction) else 1
    corr = one - q
    singular = corr == 0
    if singular:
        cxx = cxy = cyy = math.nan
    else:
        cxx, cxy, cyy = bxx / corr, bxy / corr, byy / corr
    mce, mse = _to_ext(mc), _to_ext(ms)
    R = xp.x_sqrt(np.array([mce * mce + mse * mse]))[0]
    Rf = _f(R)
    degenerate = Rf < EPSILON
    if degenerate:
        cos, sin, ctt = 1.0, 0.0, math.inf
        rot_unit = tt_unit = 0.0
    else:
        cos, sin = mce / R, mse / R
        ctt = -2 * xp.x_log(np.array([R]))[0]
        rot_unit = U * (1.0 + 1.0 / Rf)
        tt_unit = U * (2.0 / Rf + abs(_f(ctt)))
    pos_unit = U * max(math.hypot(_f(x), _f(y)), D)
    qf = _f(q)
    cov_unit = math.nan if singular else U * (D * D + qf * (_f(cxx) + _f(cyy))) / _f(corr)
    return Estimate(x, y, cos, sin, cxx, cxy, cyy, ctt, degenerate, singular, Rf, qf, D, pos_unit, cov_unit, rot_unit, tt_unit)


def estimate_exact(states, w):
    states, w = _split(states, w)
    s = sums_exact(states, w, (0.0, 0.0)).value
    W = s[0]
    x, y = s[4] / W, s[5] / W
    return _finish(x, y, s[2] / W, s[3] / W, s[6] / W - x * x, s[7] / W - x * y, s[8] / W - y * y, s[1] / (W * W), _box_diagonal(states, w))


def estimate_extended(states, w):
    states, w = _split(states, w)
    first = int(np.argmax(w > 0))
    p0 = (float(states[first, 2]), float(states[first, 3]))
    a = sums_extended(states, w, p0).value
    W = a[0]
    # the mean to double-double: what is left of it after the double nearest to it is taken out
    px, py = _f(xp.ext(np.array([p0[0]]))[0] + a[4] / W), _f(xp.ext(np.array([p0[1]]))[0] + a[5] / W)
    b = sums_extended(states, w, (px, py)).value
    rx, ry = b[4] / W, b[5] / W  # (the residual of the rounded mean: below 2^-53 of it)
    x, y = xp.ext(np.array([px]))[0] + rx, xp.ext(np.array([py]))[0] + ry
    return _finish(x, y, b[2] / W, b[3] / W, b[6] / W - rx * rx, b[7] / W - rx * ry, b[8] / W - ry * ry, b[1] / (W * W),
                   _box_diagonal(states, w))


def estimate(states, w):
    return estimate_exact(states, w) if len(w) <= EXACT_MAX else estimate_extended(states, w)


Errors = namedtuple("Errors", "pos rot cov tt")


def _diff(got, want):
    """|got - want| as a double; want exact or extended, got a double."""
    if isinstance(want, Fraction):
        return abs(float(Fraction(got) - want))
    return abs(_f(xp.ext(np.array([got]))[0] - want))


def _in_units(diff, unit):
    if diff == 0:
        return 0.0
    return diff / unit if unit > 0 else math.inf


def errors(reference, pose, cov):
    """pose: (cos, sin, x, y); cov: 3 x 3 -> Errors in the reference's units."""
    pose = np.asarray(pose, dtype=np.float64).reshape(4)
    cov = np.asarray(cov, dtype=np.float64).reshape(3, 3)
    r = reference
    if not (math.isfinite(pose[2]) and math.isfinite(pose[3])):
        pos = math.inf
    else:
        pos = _in_units(math.hypot(_diff(pose[2], r.x), _diff(pose[3], r.y)), r.pos_unit)
    block = (cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1])
    if r.singular:
        c = 0.0 if all(math.isnan(v) for v in block) else math.inf
    elif not all(math.isfinite(v) for v in block):
        c = math.inf
    else:
        c = max(_in_units(_diff(g, want), r.cov_unit) for g, want in zip(block, (r.cov_xx, r.cov_xy, r.cov_xy, r.cov_yy)))
    if any(cov[i, j] != 0.0 for i, j in ((0, 2), (1, 2), (2, 0), (2, 1))):
        c = math.inf
    if r.degenerate:
        rot = 0.0 if (pose[0] == 1.0 and pose[1] == 0.0) else math.inf
        tt = 0.0 if cov[2, 2] == math.inf else math.inf
    elif not all(math.isfinite(v) for v in (pose[0], pose[1], cov[2, 2])):
        rot = tt = math.inf
    else:
        rot = _in_units(math.hypot(_diff(pose[0], r.cos), _diff(pose[1], r.sin)), r.rot_unit)
        tt = _in_units(_diff(cov[2, 2], r.cov_tt), r.tt_unit)
    return Errors(pos, rot, c, tt)


def as_doubles(reference):
    """(pose, cov) of the reference rounded to double (for printing and for the pinned vectors)."""
    r = reference
    pose = np.array([_f(r.cos), _f(r.sin), _f(r.x), _f(r.y)])
    cov = np.zeros((3, 3))
    if r.singular:
        cov[:2, :2] = math.nan
    else:
        cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1] = _f(r.cov_xx), _f(r.cov_xy), _f(r.cov_xy), _f(r.cov_yy)
    cov[2, 2] = _f(r.cov_tt)
    return pose, cov


# ---- the limit -----------------------------------------------------------------------------------------------------
def estimate_error_bound(n):
    """How many roundings one of the nine sums can carry, from the fixed tree every estimate kernel adds it in (kernels.hip; kChunk = 2048
    particles per workgroup of 256 lanes, 64 lanes per wave):
       4  a term: dx = x - pivot rounds once and enters w dx dx twice, the two products round once each
       8  the lane's serial additions (k_estimate_partials: 8 items per lane; the one-workgroup kernels of up to 4096 particles: 4 per
          lane of 1024)
       6  wave_sum_f64: quads, octets, rows, half-waves, and the four rows as (r0 + r1) + (r2 + r3)
       3  block_reduce: the four waves of a workgroup in order          (small_block_sum: its 16 waves in order, 15 - with 4 items
                                                                         per lane 4 + 4 + 6 + 15 = 29, below the 30 of this line and
                                                                         the next)
       9  k_final_rows over the chunks' partial sums (and the same tree folded into the draw kernel's last workgroup): a lane adds
          ceil(chunks / 256) of them in order, then the wave (6) and the block (3) as above - counted whether or not n reaches a
          second chunk, so that one figure covers every kernel
    = 30 + ceil(chunks / 256) units of u S|term| for a sum.  The same figure is the limit of the estimate in its conditioned units: with
    the pivot inside the bounding box every term of a second moment is at most D^2 (of a first moment D, of the heading's sums 1), so a
    sum's bound in units of its S|term| / W is a bound in the estimate's units; the host finish (mcl_estimate_from_sums) rounds a
    handful of times more and W's own error enters once more, which the distance between this worst case - every rounding of the tree
    in one direction - and any real sum leaves ample room for (test_estimate_reference_cpu.py shows the finish on correctly rounded
    sums within it).  Sharded: a rank's sum goes through its own tree, then launch_sum_rows adds the ranks in order: + world."""
    chunks = max(1, -(-int(n) // 2048))
    return 30 + -(-chunks // 256)
