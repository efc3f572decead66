"""The rule of the local pose search (mcl_local_search*, include/beluga_mcl.h), restated in numpy and exact rationals.

Parameters (Kx = half_steps_xy <= 32, Kt = half_steps_theta <= 64, finite steps, step_theta > 0, step_xy >= 0, Kt * step_theta < pi), the
lattice of L = (2 Kx + 1)^2 (2 Kt + 1) candidates (i, j, k) with id ((k + Kt)(2 Kx + 1) + (j + Kx))(2 Kx + 1) + (i + Kx), their poses
(x = seed.x + double(i) * step_xy, likewise y; the rotation rot_mul(seed.r, rot_exp(double(k) * step_theta)), the seed's own for k == 0),
the best candidate by (score descending, i*i + j*j ascending, |k| ascending, id ascending), the plateau, the ten sums and their finish.
Nothing here reads the library: the tests hold the library to this file, and this file to brute force (tests/test_local_search_reference_cpu.py).
"""
import math
from fractions import Fraction

import numpy as np

MAX_HALF_XY, MAX_HALF_THETA = 32, 64
DEFAULTS = (4, 5, 0.0, math.pi / 360)
SECOND = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # sums[4 .. 9]: ii ij ik jj jk kk


def check_params(Kx, Kt, step_xy, step_theta):
    """True where the library takes the parameters."""
    if not (0 <= Kx <= MAX_HALF_XY and 0 <= Kt <= MAX_HALF_THETA):
        return False
    if not (math.isfinite(step_xy) and math.isfinite(step_theta)):
        return False
    return step_xy >= 0.0 and step_theta > 0.0 and float(Kt) * step_theta < math.pi


def side(K):
    return 2 * K + 1


def candidates(Kx, Kt):
    return side(Kx) ** 2 * side(Kt)


def local_id(Kx, Kt, i, j, k):
    return ((k + Kt) * side(Kx) + (j + Kx)) * side(Kx) + (i + Kx)


def offsets_of(Kx, Kt, ids):
    """(i, j, k) of ids (an int or an integer array)."""
    nx = side(Kx)
    return ids % nx - Kx, ids // nx % nx - Kx, ids // (nx * nx) - Kt


# -- se2.h, operation by operation (np.hypot is the C library's hypot, as std::hypot on the host) ----------------------------------
def rot_from_complex(re, im):
    length = float(np.hypot(re, im))
    return re / length, im / length


def rot_exp(theta):
    return rot_from_complex(math.cos(theta), math.sin(theta))


def rot_mul(a, b):
    re = a[0] * b[0] - a[1] * b[1]
    im = a[0] * b[1] + a[1] * b[0]
    n2 = re * re + im * im
    if n2 != 1.0:
        scale = 2.0 / (1.0 + n2)
        re, im = re * scale, im * scale
    return rot_from_complex(re, im)


def offset_table(Kx, step_xy):
    return np.array([float(i) * step_xy for i in range(-Kx, Kx + 1)], dtype=np.float64)


def rotation_table(seed, Kt, step_theta):
    """(2 Kt + 1, 2): (cos, sin) per step; the seed's rotation as given at k == 0."""
    r = (float(seed[0]), float(seed[1]))
    return np.array([r if k == 0 else rot_mul(r, rot_exp(float(k) * step_theta)) for k in range(-Kt, Kt + 1)], dtype=np.float64)


def lattice_poses(seed, Kx, Kt, step_xy, step_theta):
    """The L poses of a seed in id order, float64 (L, 4)."""
    off, rot = offset_table(Kx, step_xy), rotation_table(seed, Kt, step_theta)
    i, j, k = offsets_of(Kx, Kt, np.arange(candidates(Kx, Kt)))
    return np.column_stack([rot[k + Kt, 0], rot[k + Kt, 1], float(seed[2]) + off[i + Kx], float(seed[3]) + off[j + Kx]])


def pass_plan(n, L, search_chunk):
    """(seeds per pass, candidates a pass's buffers hold, passes)."""
    chunk = min(max(int(search_chunk), 64), 1 << 22)
    per_pass = max(1, chunk // L)
    return per_pass, per_pass * L, (n + per_pass - 1) // per_pass


# -- the order ------------------------------------------------------------------------------------------------------------------------
def score_key(score):
    """The uint64 whose unsigned order is the scores' order; NaN is the lowest (0)."""
    if score != score:
        return 0
    bits = int(np.float64(score).view(np.uint64))
    return (~bits & 0xFFFFFFFFFFFFFFFF) if bits >> 63 else bits | (1 << 63)


def tie_key(Kx, Kt, ident):
    i, j, k = offsets_of(Kx, Kt, int(ident))
    return ((i * i + j * j) << 27) | (abs(k) << 20) | int(ident)


def best_of(scores, Kx, Kt):
    """(id of the first candidate by the order, plateau) of one seed's L scores in id order."""
    scores = np.asarray(scores, dtype=np.float64)
    keys = np.array([score_key(s) for s in scores], dtype=np.uint64)
    top = keys.max()
    tied = np.flatnonzero(keys == top)
    i, j, k = offsets_of(Kx, Kt, tied)
    order = np.lexsort((tied, np.abs(k), i * i + j * j))
    return int(tied[order[0]]), len(tied)


# -- the moments ------------------------------------------------------------------------------------------------------------------------
def exact_sums(scores, Kx, Kt):
    """The ten sums as exact rationals over the scores' exact binary values, and the sums of the terms' magnitudes."""
    ids = np.arange(len(scores))
    c = offsets_of(Kx, Kt, ids)
    factors = [np.ones(len(scores), dtype=np.int64), c[0], c[1], c[2]] + [c[a] * c[b] for a, b in SECOND]
    w = [Fraction(float(s)) for s in scores]
    sums, magnitudes = [], []
    for f in factors:
        terms = [wi * int(fi) for wi, fi in zip(w, f)]
        sums.append(sum(terms, Fraction(0)))
        magnitudes.append(sum((abs(t) for t in terms), Fraction(0)))
    return sums, magnitudes


def finish_exact(sums, step_xy, step_theta):
    """(mean offsets (dx, dy, dtheta), covariance 3 x 3) as exact rationals of sums (any numbers with exact values) and the steps."""
    S = [Fraction(s) for s in sums]
    step = [Fraction(step_xy), Fraction(step_xy), Fraction(step_theta)]
    m = [S[1 + a] / S[0] for a in range(3)]
    second = {pair: S[4 + n] for n, pair in enumerate(SECOND)}
    cov = [[(second[(min(a, b), max(a, b))] / S[0] - m[a] * m[b]) * step[a] * step[b] for b in range(3)] for a in range(3)]
    return [m[a] * step[a] for a in range(3)], cov


def finish_bound(sums, step_xy, step_theta):
    """What the library's finish may be off by, from its operations alone (u = 2^-53 per rounding).
    A mean offset is two roundings (a division, a product): 3 u |mean| covers them with their second order.
    A covariance entry ((S_ab / S0 - m_a m_b) step_a) step_b: the quotient carries 1 rounding, the product m_a m_b 3 (two quotients and
    itself), the difference 1 and the two products by the steps 2 more, all relative to magnitudes no larger than
    (|S_ab / S0| + |m_a m_b|) step_a step_b: 1 + 3 + 1 + 2 = 7 roundings, and 8 u of that magnitude covers their second order."""
    u = Fraction(1, 2 ** 53)
    S = [Fraction(s) for s in sums]
    step = [Fraction(step_xy), Fraction(step_xy), Fraction(step_theta)]
    m = [S[1 + a] / S[0] for a in range(3)]
    second = {pair: S[4 + n] for n, pair in enumerate(SECOND)}
    mean = [3 * u * abs(m[a] * step[a]) for a in range(3)]
    cov = [[8 * u * (abs(second[(min(a, b), max(a, b))] / S[0]) + abs(m[a] * m[b])) * step[a] * step[b] for b in range(3)] for a in range(3)]
    return mean, cov


def uniform_covariance(K, step):
    """The variance of a uniform weight over the offsets -K .. K of `step`: K (K + 1) / 3 * step^2."""
    return Fraction(K * (K + 1), 3) * Fraction(step) ** 2
