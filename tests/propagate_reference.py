"""The propagation (actions::propagate with the three motion models) restated in extended precision, and the unit its error is quoted in.

Plain numpy; nothing here imports the code under test.  The integer part - the Philox4x32-10 words of (seed, step, purpose 0 / 1,
index) and the 53-bit uniforms made of them - is exact; tests/test_propagate_reference_cpu.py holds it to orc.draw word for word.
Everything after that is numpy.longdouble where that is the x87 format (64-bit significand) and mpmath at 80 bits where it is not.

What is restated (beluga_amd/csrc/rng.h and kernels.hip, propagate_with_normals; the reference project's lines beside each):
  * Box-Muller as rng.h writes it: r = sqrt(-2 log(1 - u1)), a = (2.0 * kPi) * u2 with 2.0 * kPi THE DOUBLE CONSTANT, z = r (cos a, sin a);
  * differential (differential_drive_model.hpp:156-163): r1 = z0 s1 + m1, t = z1 st + mt, r2 = z2 s2 + m2,
    state * (exp r1, 0, 0) * (exp r2, t, 0);
  * omnidirectional (omnidirectional_drive_model.hpp:133-144): r = z0 s1 + m1, t = z1 st + mt, strafe = z2 s2,
    state * (first, 0, 0) * (exp r * first^-1, t, -strafe);
  * stationary (stationary_model.hpp:55-61): state * (exp 0.02 z0, 0.02 z1, 0.02 z2).
Composition is on ANGLES: the heading is atan2 of the input rotation (which normalises it) plus the drawn rotations, the output
rotation is (cos, sin) of the heading; a translation is turned by the heading of the rotation left of it.  (The stationary model's one
product turns its translation by the input rotation AS STORED, se2.h pose_mul - for a rotation that is not unit that includes its
length -, and so does the restatement.)

The conditioned unit, u = 2^-53.  A result cannot be better than its inputs allow: each term below is the effect on the result of one
rounding (half a unit in the last place, relative) of a quantity every double-precision evaluation has to round.
  zu = r (2 + a) for a Box-Muller pair: a normal's absolute error (r, the angle a = 2 pi u2 and the sine each rounded);
  differential:    d1 = u (s1 zu0 + |r1| + 1)        - the heading left of the translation (r1's product and sum, the input heading)
                   rot_unit = d1 + u (s2 zu2 + |r2|)
                   pos_unit = u (|x_in| + |y_in| + |x_out| + |y_out| + st zu1 + |t|) + |t| d1
  omnidirectional: d1 = u (|phi| + 1), phi = atan2(first_s, first_c)
                   rot_unit = d1 + u (s1 zu0 + |r| + |phi|)
                   pos_unit = u (|x_in| + |y_in| + |x_out| + |y_out| + st zu1 + |t| + s2 zu2 + |strafe|) + (|t| + |strafe|) d1
  stationary:      d1 = u
                   rot_unit = d1 + u (0.02 zu0 + |r|)
                   pos_unit = u (|x_in| + |y_in| + |x_out| + |y_out| + 0.02 (zu1 + zu2) + |dx| + |dy|) + (|dx| + |dy|) d1
An error is quoted in these units: for the rotation the distance between the stored (cos, sin) and the reference's point on the unit
circle (so a rotation of the wrong length counts like one of the wrong angle), for the position the Euclidean distance.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -53
TWO_PI = 2.0 * 3.14159265358979323846  # rng.h: 2.0 * kPi, the double
KIND_DIFFERENTIAL, KIND_OMNIDIRECTIONAL, KIND_STATIONARY = 0, 1, 2
FALLBACK = 1.0e6  # sincos_fast hands |theta| >= 1e6 to the library

USE_MPMATH = np.finfo(np.longdouble).eps > 2.0 ** -63

if USE_MPMATH:
    import mpmath

    mpmath.mp.prec = 80
    _mpf = mpmath.mpf

    def ext(a):
        a = np.asarray(a, dtype=np.float64)
        out = np.empty(a.shape, dtype=object)
        flat = out.reshape(-1)
        for i, v in enumerate(a.reshape(-1)):
            flat[i] = _mpf(float(v))
        return out

    _f1 = {name: np.frompyfunc(getattr(mpmath, name), 1, 1) for name in ("sin", "cos", "log", "sqrt")}
    x_sin, x_cos, x_log, x_sqrt = _f1["sin"], _f1["cos"], _f1["log"], _f1["sqrt"]
    x_atan2 = np.frompyfunc(mpmath.atan2, 2, 1)
    x_abs = np.frompyfunc(abs, 1, 1)

    def to_f64(a):
        return np.array([float(v) for v in np.asarray(a, dtype=object).reshape(-1)], dtype=np.float64).reshape(np.shape(a))
else:
    def ext(a):
        return np.asarray(a, dtype=np.float64).astype(np.longdouble)

    x_sin, x_cos, x_log, x_sqrt, x_atan2, x_abs = np.sin, np.cos, np.log, np.sqrt, np.arctan2, np.abs

    def to_f64(a):
        return np.asarray(a).astype(np.float64)


# ---- the integer part ----------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: (n, 4) uint32, key: (2,) -> (n, 4) uint32 (rng.h philox4x32_10)."""
    c = [np.asarray(counter[:, j], dtype=np.uint64) for j in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    mask = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & mask, p1 >> s32, p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def draw(seed, step, purpose, index):
    """rng_draw: counter = (index_lo, index_hi, step, purpose), key = (seed_lo, seed_hi); index: (n,) -> (n, 4) uint32."""
    index = np.asarray(index, dtype=np.uint64)
    ctr = np.empty((len(index), 4), dtype=np.uint64)
    ctr[:, 0] = index & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = index >> np.uint64(32)
    ctr[:, 2] = int(step) & 0xFFFFFFFF
    ctr[:, 3] = int(purpose)
    return philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def uniform53(hi, lo):
    """rng_uniform53: the top 53 bits of (hi : lo) * 2^-53, exact in double."""
    v = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return (v >> np.uint64(11)).astype(np.float64) * U


# ---- Box-Muller ----------------------------------------------------------------------------------------
def box_muller(u1, u2):
    """-> z0, z1 (extended), zu (double): r (2 + a)."""
    r = x_sqrt(-2 * x_log(ext(1.0 - u1)))  # (1 - u1 is exact: both are multiples of 2^-53 in (0, 1])
    a = ext(TWO_PI) * ext(u2)
    return r * x_cos(a), r * x_sin(a), to_f64(r * (2 + a))


def normals(seed, step, index):
    """The three standard normals of every index in extended precision, and their units: (z0, z1, z2), (zu0, zu1, zu2)."""
    a, b = draw(seed, step, 0, index), draw(seed, step, 1, index)
    z0, z1, zu01 = box_muller(uniform53(a[:, 0], a[:, 1]), uniform53(a[:, 2], a[:, 3]))
    z2, _, zu2 = box_muller(uniform53(b[:, 0], b[:, 1]), uniform53(b[:, 2], b[:, 3]))
    return (z0, z1, z2), (zu01, zu01, zu2)


# ---- the motion models -----------------------------------------------------------------------------------
Reference = namedtuple("Reference", "cos sin x y rot_unit pos_unit angles")
# cos, sin, x, y: the propagated states in extended precision; rot_unit, pos_unit: float64; angles: (n, k) float64, the arguments the
# model hands to rot_exp (differential: r1, r2; the others: one), rounded - what the kernel's sine / cosine reduction sees, to rounding.


def propagate(states, sampler, seed, step, index=None, index_offset=0):
    """states: (n, 4) as (cos, sin, x, y); sampler: (m1, s1, mt, st, m2, s2, kind, first_c, first_s) - for the differential model the
    first six suffice; index: the rows' particle indices (default 0 .. n - 1), to which index_offset is added for the random stream."""
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    n = len(states)
    sampler = np.asarray(sampler, dtype=np.float64)
    kind = int(sampler[6]) if len(sampler) > 6 else KIND_DIFFERENTIAL
    index = np.arange(n, dtype=np.uint64) if index is None else np.asarray(index, dtype=np.uint64)
    assert len(index) == n
    (z0, z1, z2), (zu0, zu1, zu2) = normals(seed, step, index + np.uint64(index_offset))
    m1, s1, mt, st, m2, s2 = (ext(v) for v in sampler[:6])
    f1, ft, f2 = abs(float(sampler[1])), abs(float(sampler[3])), abs(float(sampler[5]))
    c_in, s_in, x_in, y_in = (ext(states[:, j]) for j in range(4))
    h_in = x_atan2(s_in, c_in)
    ax_in = np.abs(states[:, 2]) + np.abs(states[:, 3])
    if kind == KIND_DIFFERENTIAL:
        r1, t, r2 = z0 * s1 + m1, z1 * st + mt, z2 * s2 + m2
        h1 = h_in + r1
        h = h1 + r2
        x, y = x_in + t * x_cos(h1), y_in + t * x_sin(h1)
        at = to_f64(x_abs(t))
        d1 = U * (f1 * zu0 + to_f64(x_abs(r1)) + 1.0)
        rot_unit = d1 + U * (f2 * zu2 + to_f64(x_abs(r2)))
        pos_unit = U * (ax_in + to_f64(x_abs(x) + x_abs(y)) + ft * zu1 + at) + at * d1
        angles = np.stack([to_f64(r1), to_f64(r2)], axis=1)
    elif kind == KIND_OMNIDIRECTIONAL:
        phi = x_atan2(ext(sampler[8]), ext(sampler[7]))
        r, t, strafe = z0 * s1 + m1, z1 * st + mt, z2 * s2
        h1 = h_in + phi
        h = h1 + (r - phi)
        c1, sn1 = x_cos(h1), x_sin(h1)
        x, y = x_in + (c1 * t - sn1 * (-strafe)), y_in + (sn1 * t + c1 * (-strafe))
        aphi = abs(float(to_f64(x_abs(phi))))
        at, astrafe = to_f64(x_abs(t)), to_f64(x_abs(strafe))
        d1 = U * (aphi + 1.0)
        rot_unit = d1 + U * (f1 * zu0 + to_f64(x_abs(r)) + aphi)
        pos_unit = U * (ax_in + to_f64(x_abs(x) + x_abs(y)) + ft * zu1 + at + f2 * zu2 + astrafe) + (at + astrafe) * d1
        angles = to_f64(r).reshape(-1, 1)
    elif kind == KIND_STATIONARY:
        k = ext(0.02)
        r, dx, dy = z0 * k, z1 * k, z2 * k
        h = h_in + r
        x, y = x_in + (c_in * dx - s_in * dy), y_in + (s_in * dx + c_in * dy)
        adx, ady = to_f64(x_abs(dx)), to_f64(x_abs(dy))
        d1 = U
        rot_unit = d1 + U * (0.02 * zu0 + to_f64(x_abs(r)))
        pos_unit = U * (ax_in + to_f64(x_abs(x) + x_abs(y)) + 0.02 * (zu1 + zu2) + adx + ady) + (adx + ady) * d1
        angles = to_f64(r).reshape(-1, 1)
    else:
        raise ValueError(f"unknown motion kind {kind}")
    return Reference(x_cos(h), x_sin(h), x, y, rot_unit, pos_unit, angles)


def errors(ref, got):
    """got: (n, 4) doubles as (cos, sin, x, y) -> (rotation error, position error) per row, in the row's units."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    dc, ds, dx, dy = ext(got[:, 0]) - ref.cos, ext(got[:, 1]) - ref.sin, ext(got[:, 2]) - ref.x, ext(got[:, 3]) - ref.y
    rot = to_f64(x_sqrt(dc * dc + ds * ds)) / ref.rot_unit
    pos = to_f64(x_sqrt(dx * dx + dy * dy)) / ref.pos_unit
    return rot, pos


def worst(ref, got):
    """-> (worst rotation error, worst position error) in units; a value that is not finite counts as infinitely wrong."""
    rot, pos = errors(ref, got)
    if not (np.all(np.isfinite(rot)) and np.all(np.isfinite(pos))):
        return float("inf"), float("inf")
    return (float(rot.max()), float(pos.max())) if len(rot) else (0.0, 0.0)


def limit(oracle_worst):
    """What the device is held to: 4 units for its four substituted helpers at the 2 ulp each documents ("The
    propagation's own forms"), or four times the double-precision oracle's own worst error on the same inputs if that is more."""
    return max(4.0, 4.0 * float(oracle_worst))


def quadrant(theta):
    """k of sincos_fast's reduction theta = r + k pi/2: rint(theta * 2 / pi), as integers."""
    return np.rint(np.asarray(theta, dtype=np.float64) * float.fromhex("0x1.45f306dc9c883p-1")).astype(np.int64)
