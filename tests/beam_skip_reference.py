"""The exact restatement of beam skipping (include/beluga_mcl.h "Beam skipping"; plain numpy and Python, no device, nothing compiled):
the level, the per-beam agreement counts over lf_reference.cells, and the decision.  The device and the host rule are held to these."""
import numpy as np

import lf_reference as ref

DEFAULTS = dict(enabled=0, distance=0.5, threshold=0.3, error_threshold=0.9)  # Nav2's


def level(z_hit, z_random, sigma_hit, max_laser_distance, distance):
    """float(amplitude * exp(-double(float(distance^2)) / (2 sigma^2)) + z_random / max_laser_distance): the field builder's last
    expression (likelihood_field_model_base.hpp:136-146,181-182) at the squared distance float(distance * distance)."""
    two_squared_sigma = np.float64(2.0) * np.float64(sigma_hit) * np.float64(sigma_hit)
    amplitude = np.float64(z_hit) / (np.float64(sigma_hit) * np.sqrt(np.float64(2.0) * np.float64(np.pi)))
    offset = np.float64(z_random) / np.float64(max_laser_distance)
    squared = np.float32(np.float64(distance) * np.float64(distance))
    return np.float32(amplitude * np.exp(-np.float64(squared) / two_squared_sigma) + offset)


def agreement_counts(field, level_value, resolution, origin, states, points):
    """count[b]: the states whose end-point of points[b] has a cell inside the grid with field[cell] > level, strictly (float32
    compare).  A point with a NaN or infinite coordinate agrees with no state; an end-point off the grid does not agree."""
    field = np.asarray(field, dtype=np.float32)
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    counts = np.zeros(len(points), dtype=np.int64)
    if len(points) == 0 or len(states) == 0:
        return counts
    finite = np.isfinite(points).all(axis=1)
    H, W = field.shape
    lvl = np.float32(level_value)
    flat = field.reshape(-1)
    for lo in range(0, len(states), 4096):  # (chunks: [n, B] arrays of a large set do not fit comfortably)
        xi, yi, inside = ref.cells(field.shape, resolution, origin, states[lo:lo + 4096], points)
        value = flat[np.clip(yi, 0, H - 1) * W + np.clip(xi, 0, W - 1)]
        agree = inside & (value > lvl) & finite[None, :]
        counts += agree.sum(axis=0)
    return counts


def decide(counts, n, B, params):
    """(kept [B] bool, skipped, used_all): kept[b] = double(count[b]) / double(n) > threshold; skipped = B - sum kept;
    used_all = B > 0 and double(skipped) / double(B) >= error_threshold."""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)[:B]
    with np.errstate(all="ignore"):
        kept = counts / np.float64(n) > np.float64(params["threshold"])
    skipped = int(B - int(kept.sum()))
    used_all = bool(B > 0 and np.float64(skipped) / np.float64(B) >= np.float64(params["error_threshold"]))
    return kept, skipped, used_all
