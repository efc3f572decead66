"""Shared by test_ndt_sparse_host_cpu.py and test_gpu_ndt_sparse.py: the hash of the NDT map's hashed layout restated from the words of
beluga_amd/csrc/ndt_hash.h (not from its code), and the maps both files use - one with holes, one whose keys all share a home slot,
one at the ends of the int32 range."""
import numpy as np

MULTIPLIER = 0x9E3779B97F4A7C15  # 2^64 / golden ratio
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def pack(x, y):
    return ((int(x) & 0xFFFFFFFF) << 32) | (int(y) & 0xFFFFFFFF)


def log2_capacity(n):
    """The smallest c >= 1 with 2^c >= 2 n: a power of two of slots, the load at most 1/2."""
    c = 1
    while (1 << c) < 2 * n:
        c += 1
    return c


def home(x, y, c):
    """The Fibonacci multiply of the packed key, the top c bits kept."""
    return ((pack(x, y) * MULTIPLIER) & (2**64 - 1)) >> (64 - c)


def holes_keys(seed=7, span=24, keep=0.55):
    """A few hundred keys on both sides of zero with holes between them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xs, ys = np.meshgrid(np.arange(-span // 2, span // 2), np.arange(-span // 3, span // 3), indexing="ij")
    keys = np.stack([xs.ravel(), ys.ravel()], 1)
    keys = keys[rng.random(len(keys)) < keep]
    rng.shuffle(keys)  # (records in the caller's order, not in key order)
    return keys.astype(np.int32)


def colliding_keys(count=12, near=(40, -17), width=4096):
    """`count` keys, found by search, that all have ONE home slot in the table of `count` cells: a row of the map, x from near[0] on."""
    c = log2_capacity(count)
    by_home = {}
    for x in range(near[0], near[0] + width):
        bucket = by_home.setdefault(home(x, near[1], c), [])
        bucket.append((x, near[1]))
        if len(bucket) == count:
            return np.array(bucket, dtype=np.int32)
    raise AssertionError("no home slot with that many keys in the searched row")


def cells_for(keys, resolution, seed=1):
    """Means inside their cells and covariances of a sensible size for `keys`: (means[n, 2], covariances[n, 2, 2])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    means = (keys + rng.uniform(0.25, 0.75, keys.shape)) * resolution
    a = rng.uniform(0.02, 0.08, len(keys)) * resolution**2
    d = rng.uniform(0.02, 0.08, len(keys)) * resolution**2
    b = rng.uniform(-0.5, 0.5, len(keys)) * np.sqrt(a * d)
    covs = np.stack([np.stack([a, b], 1), np.stack([b, d], 1)], 1)
    return means, covs
