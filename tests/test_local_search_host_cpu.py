"""The local pose search's host rule (beluga_amd/csrc/local_search_host.cpp) on the CPU: a plain g++ builds the file, with a few
extern "C" doors to its C++ functions, into a small shared object, and the parameter checks, the tables, the ids, the pass plan, the
order key and the finish are held to tests/local_search_reference.py - the finish to exact rationals within the bound its operation
count gives (ref.finish_bound)."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import local_search_reference as ref
from beluga_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beluga_amd", "csrc")

DOORS = r"""
#include "local_search_host.h"
using namespace mcl;
extern "C" {
int t_check(uint32_t kx, uint32_t kt, double sx, double st) { return local_check_params(mcl_local_search_params{kx, kt, sx, st}) == nullptr; }
uint64_t t_candidates(uint32_t kx, uint32_t kt) { return local_candidates(mcl_local_search_params{kx, kt, 0.0, 1.0}); }
uint32_t t_id(uint32_t kx, uint32_t kt, int32_t i, int32_t j, int32_t k) { return local_id(kx, kt, i, j, k); }
void t_offsets_of(uint32_t kx, uint32_t kt, uint32_t id, int32_t* out) { local_offsets_of(kx, kt, id, out[0], out[1], out[2]); }
void t_offsets(uint32_t kx, double step, double* out) {
  std::vector<double> off;
  local_offsets(kx, step, off);
  for (size_t i = 0; i < off.size(); ++i) out[i] = off[i];
}
void t_rotations(const double* seeds, uint64_t n, uint32_t kt, double step, double* out) {
  std::vector<double> rot;
  local_rotations(seeds, n, kt, step, rot);
  for (size_t i = 0; i < rot.size(); ++i) out[i] = rot[i];
}
void t_pose(const double* seed, uint32_t kx, uint32_t kt, double sx, double st, uint32_t id, double* out) {
  std::vector<double> off, rot;
  local_offsets(kx, sx, off);
  local_rotations(seed, 1, kt, st, rot);
  local_pose(seed, off.data(), rot.data(), kx, kt, id, out);
}
void t_plan(uint64_t n, uint64_t L, int64_t chunk, uint64_t* out) {
  const LocalPlan plan = local_plan(n, L, chunk);
  out[0] = plan.seeds_per_pass, out[1] = plan.pass_candidates, out[2] = plan.passes;
}
uint64_t t_tie(uint32_t kx, uint32_t kt, uint32_t id) { return local_tie_key(kx, kt, id); }
uint64_t t_score_key(double score) { return local_score_key(score); }
int t_before(uint64_t ka, uint64_t ta, uint64_t kb, uint64_t tb) { return local_before(ka, ta, kb, tb) ? 1 : 0; }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("local_search_host")
    doors = d / "doors.cpp"
    doors.write_text(DOORS)
    out = d / "liblocal_search_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(CSRC, "local_search_host.cpp"), str(doors), "-o", str(out)])
    so = C.CDLL(str(out))
    u32, u64, i32, f64 = C.c_uint32, C.c_uint64, C.c_int32, C.c_double
    for name, res, args in (("t_check", C.c_int, [u32, u32, f64, f64]), ("t_candidates", u64, [u32, u32]), ("t_id", u32, [u32, u32, i32, i32, i32]),
                            ("t_offsets_of", None, [u32, u32, u32, C.POINTER(i32)]), ("t_offsets", None, [u32, f64, capi.c_double_p]),
                            ("t_rotations", None, [capi.c_double_p, u64, u32, f64, capi.c_double_p]),
                            ("t_pose", None, [capi.c_double_p, u32, u32, f64, f64, u32, capi.c_double_p]),
                            ("t_plan", None, [u64, u64, C.c_int64, capi.c_u64_p]), ("t_tie", u64, [u32, u32, u32]), ("t_score_key", u64, [f64]),
                            ("t_before", C.c_int, [u64, u64, u64, u64]),
                            ("mcl_default_local_search_params", None, [C.POINTER(capi.LocalSearchParams)]),
                            ("mcl_local_search_finish", C.c_int32, capi._SIGNATURES["mcl_local_search_finish"][1])):
        getattr(so, name).restype = res
        getattr(so, name).argtypes = args
    return so


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dp(a):
    return a.ctypes.data_as(capi.c_double_p)


def test_defaults(lib):
    p = capi.LocalSearchParams()
    lib.mcl_default_local_search_params(C.byref(p))
    assert (p.half_steps_xy, p.half_steps_theta, p.step_xy) == ref.DEFAULTS[:3] and p.step_theta == ref.DEFAULTS[3] == math.pi / 360
    lib.mcl_default_local_search_params(None)
    assert ref.check_params(*ref.DEFAULTS) and lib.t_check(*ref.DEFAULTS)


def test_parameter_limits_at_their_edges(lib):
    below_pi = math.nextafter(math.pi / 64, 0.0)
    cases = [(32, 64, 0.0, 0.01, True), (33, 64, 0.1, 0.01, False), (32, 65, 0.1, 0.01, False), (0, 0, 0.0, 1e300, True),
             (4, 5, -0.0, 0.01, True), (4, 5, -1e-300, 0.01, False), (4, 5, 0.1, 0.0, False), (4, 5, 0.1, -0.1, False),
             (4, 5, math.inf, 0.01, False), (4, 5, 0.1, math.inf, False), (4, 5, math.nan, 0.01, False), (4, 5, 0.1, math.nan, False),
             (4, 64, 0.1, below_pi, 64.0 * below_pi < math.pi), (4, 64, 0.1, math.pi / 64, False), (4, 1, 0.1, math.pi, False),
             (4, 1, 0.1, math.nextafter(math.pi, 0.0), True), (4, 0, 0.1, 100.0, True), (4, 5, 5e-324, 5e-324, True)]
    for Kx, Kt, sx, st, want in cases:
        assert ref.check_params(Kx, Kt, sx, st) == want, (Kx, Kt, sx, st)
        assert bool(lib.t_check(Kx, Kt, sx, st)) == want, (Kx, Kt, sx, st)


SHAPES = [(0, 0), (1, 1), (2, 3), (6, 8), (32, 64), (0, 64), (32, 0)]


def test_ids_and_their_inverse(lib):
    assert ref.candidates(32, 64) == 545025 < (1 << 20)
    for Kx, Kt in SHAPES:
        L = ref.candidates(Kx, Kt)
        assert lib.t_candidates(Kx, Kt) == L
        ids = np.unique(np.concatenate([np.arange(min(L, 300)), np.arange(max(L - 300, 0), L), np.random.default_rng(Kx + Kt).integers(0, L, 200)]))
        out = (C.c_int32 * 3)()
        for ident in ids:
            i, j, k = (int(v) for v in ref.offsets_of(Kx, Kt, int(ident)))
            assert abs(i) <= Kx and abs(j) <= Kx and abs(k) <= Kt
            lib.t_offsets_of(Kx, Kt, int(ident), out)
            assert tuple(out) == (i, j, k)
            assert lib.t_id(Kx, Kt, i, j, k) == ident == ref.local_id(Kx, Kt, i, j, k)
        assert ref.local_id(Kx, Kt, -Kx, -Kx, -Kt) == 0 and ref.local_id(Kx, Kt, Kx, Kx, Kt) == L - 1


def test_tables_equal_the_restatement_bit_for_bit(lib):
    rng = np.random.default_rng(5)
    seeds = np.column_stack([np.cos(t := rng.uniform(-math.pi, math.pi, 7)), np.sin(t), rng.normal(0, 50, 7), rng.normal(0, 50, 7)])
    seeds[1, :2] *= 1.0 + 2.0 ** -51  # not normalised to the last bit
    seeds[2, :2] = (1.0, 0.0)
    seeds[3, :2] = (-1.0, 1.2246467991473532e-16)
    for Kx, Kt, sx, st in ((0, 0, 0.0125, 0.01), (4, 5, 0.0125, math.pi / 360), (32, 64, 0.1 / 3, math.nextafter(math.pi / 64, 0.0)), (6, 8, 0.0, 0.3)):
        off = np.zeros(ref.side(Kx))
        lib.t_offsets(Kx, sx, dp(off))
        assert np.array_equal(bits(off), bits(ref.offset_table(Kx, sx))) and off[Kx] == 0.0
        rot = np.zeros((len(seeds), ref.side(Kt), 2))
        lib.t_rotations(dp(np.ascontiguousarray(seeds)), len(seeds), Kt, st, dp(rot))
        for s, seed in enumerate(seeds):
            assert np.array_equal(bits(rot[s]), bits(ref.rotation_table(seed, Kt, st))), (Kx, Kt, s)
            assert np.array_equal(bits(rot[s, Kt]), bits(seed[:2]))  # the seed's rotation as given
            poses = ref.lattice_poses(seed, Kx, Kt, sx, st)
            L = len(poses)
            assert np.array_equal(bits(poses[ref.local_id(Kx, Kt, 0, 0, 0)]), bits(seed))  # the centre is the seed bit for bit
            got = np.zeros(4)
            for ident in {0, L // 3, L // 2, L - 1}:
                lib.t_pose(dp(np.ascontiguousarray(seed)), Kx, Kt, sx, st, ident, dp(got))
                assert np.array_equal(bits(got), bits(poses[ident])), (Kx, Kt, s, ident)


def test_pass_plan(lib):
    out = (C.c_uint64 * 3)()
    want = {1: (64, 64), 27: (2, 54), 175: (1, 175), 545025: (1, 545025)}
    for L, (per_pass, held) in want.items():
        for n in (0, 1, 5, 64, 65, 129):
            lib.t_plan(n, L, 64, out)
            assert tuple(out) == ref.pass_plan(n, L, 64) == (per_pass, held, -(-n // per_pass)), (L, n)
            assert held <= max(64, L)
    for chunk, L, n in ((1 << 20, 2873, 16), (0, 27, 3), (1 << 40, 1, 1 << 23), (4096, 545025, 2), (1 << 22, 545025, 9)):
        lib.t_plan(n, L, chunk, out)
        assert tuple(out) == ref.pass_plan(n, L, chunk)
    assert ref.pass_plan(16, 2873, 1 << 20) == (364, 364 * 2873, 1) and ref.pass_plan(9, 545025, 1 << 22) == (7, 7 * 545025, 2)


def test_order_key_on_ties_at_each_level(lib):
    Kx, Kt = 2, 3
    key, tie = lambda s: lib.t_score_key(s), lambda i, j, k: lib.t_tie(Kx, Kt, ref.local_id(Kx, Kt, i, j, k))
    for ident in range(ref.candidates(Kx, Kt)):
        assert lib.t_tie(Kx, Kt, ident) == ref.tie_key(Kx, Kt, ident)
    for s in (-math.inf, -1.0, -0.0, 0.0, 5e-324, 0.5, 1.0, math.nextafter(1.0, 2.0), math.inf, math.nan):
        assert lib.t_score_key(s) == ref.score_key(s)

    def first(a, b):  # a = (score, i, j, k)
        return bool(lib.t_before(key(a[0]), tie(*a[1:]), key(b[0]), tie(*b[1:])))

    # 1. the score decides, whatever the offsets: a far corner with the higher score comes first, by one ulp too
    assert first((0.7, 2, 2, 3), (0.6, 0, 0, 0)) and not first((0.6, 0, 0, 0), (0.7, 2, 2, 3))
    assert first((math.nextafter(0.7, 1.0), 2, 2, -3), (0.7, 0, 0, 0))
    # 2. equal scores: i*i + j*j ascending, whatever |k| and the id
    assert first((0.7, 1, 0, 3), (0.7, 1, 1, 0)) and first((0.7, 0, -1, 3), (0.7, -1, -1, 0)) and first((0.7, 0, 0, -3), (0.7, 0, 1, 0))
    assert first((0.7, 2, 0, 0), (0.7, 2, 1, 0)) and first((0.7, 1, 1, 0), (0.7, 2, 0, 0))  # 2 < 4 < 5
    # 3. equal scores and radius: |k| ascending, whatever the id (k = -1 has the lower id, k = 0 wins; |-1| ties with |1|: level 4)
    assert first((0.7, 1, 0, 0), (0.7, 1, 0, -1)) and first((0.7, 0, 1, 1), (0.7, 1, 0, -2)) and first((0.7, -1, 0, -1), (0.7, 1, 0, 2))
    # 4. all equal: the id ascending
    assert first((0.7, 1, 0, -1), (0.7, 1, 0, 1)) and first((0.7, -1, 0, 1), (0.7, 1, 0, 1)) and first((0.7, 0, -1, 1), (0.7, -1, 0, 1))
    assert not first((0.7, 1, 0, 1), (0.7, 1, 0, 1))
    # NaN is behind everything, -inf included
    assert first((-math.inf, 2, 2, 3), (math.nan, 0, 0, 0))
    # and the reference's best_of agrees with a scan by t_before
    rng = np.random.default_rng(2)
    for _ in range(20):
        scores = rng.choice([0.25, 0.5, 0.5000000000000001, 0.75], ref.candidates(Kx, Kt))
        best = 0
        for ident in range(1, len(scores)):
            if lib.t_before(key(scores[ident]), lib.t_tie(Kx, Kt, ident), key(scores[best]), lib.t_tie(Kx, Kt, best)):
                best = ident
        assert (best, int(np.count_nonzero(scores == scores[best]))) == ref.best_of(scores, Kx, Kt)


def finish(lib, sums, Kx, Kt, sx, st, seed):
    p = capi.LocalSearchParams(Kx, Kt, sx, st)
    mean, cov, valid = np.full(4, 99.0), np.full(9, 99.0), C.c_int32(7)
    status = lib.mcl_local_search_finish(dp(np.ascontiguousarray(sums, dtype=np.float64)), C.byref(p), dp(np.ascontiguousarray(seed, dtype=np.float64)),
                                         dp(mean), dp(cov), C.byref(valid))
    return status, mean, cov.reshape(3, 3), valid.value


def check_finish(lib, sums, Kx, Kt, sx, st, seed):
    status, mean, cov, valid = finish(lib, sums, Kx, Kt, sx, st, seed)
    assert status == capi.MCL_OK and valid == 1
    want_mean, want_cov = ref.finish_exact(sums, sx, st)
    bound_mean, bound_cov = ref.finish_bound(sums, sx, st)
    u = Fraction(1, 2 ** 53)
    for a, coordinate in ((0, 2), (1, 3)):  # seed + offset: the offset's own error, and one rounding of the sum
        exact = Fraction(float(seed[coordinate])) + want_mean[a]
        assert abs(Fraction(float(mean[coordinate])) - exact) <= bound_mean[a] + u * (abs(exact) + bound_mean[a]), (a, sums)
    # the rotation: rot_mul(seed.r, rot_exp(dtheta)) as the reference forms it from the library's own dtheta = step_theta * (S_k / S0)
    dtheta = st * (float(sums[3]) / float(sums[0]))
    assert abs(Fraction(dtheta) - want_mean[2]) <= bound_mean[2]
    assert np.array_equal(bits(mean[:2]), bits(ref.rot_mul((float(seed[0]), float(seed[1])), ref.rot_exp(dtheta))))
    for a in range(3):
        for b in range(3):
            assert abs(Fraction(float(cov[a, b])) - want_cov[a][b]) <= bound_cov[a][b], (a, b, sums)
            assert cov[a, b] == cov[b, a]
    return mean, cov


def sums_of(scores, Kx, Kt):
    exact, _ = ref.exact_sums(scores, Kx, Kt)
    return np.array([float(s) for s in exact])


def test_finish_within_the_bound_of_its_operation_count(lib):
    rng = np.random.default_rng(9)
    seed = np.array([math.cos(0.7), math.sin(0.7), -12.25, 3.375])
    for Kx, Kt, sx, st in ((1, 1, 0.0125, math.pi / 360), (2, 3, 0.05, 0.01), (4, 5, 0.0125, math.pi / 360), (0, 2, 0.0, 0.1), (3, 0, 0.02, 0.1)):
        L = ref.candidates(Kx, Kt)
        for scores in (rng.uniform(0.0, 1.0, L), rng.uniform(0.0, 1.0, L) ** 40, np.where(np.arange(L) == L - 1, 1.0, 1e-30)):
            check_finish(lib, sums_of(scores, Kx, Kt), Kx, Kt, sx, st, seed)
    # sums that no lattice gave: the finish is arithmetic on ten numbers
    check_finish(lib, np.array([3.0, 1.0, -2.0, 0.5, 7.0, 0.25, -1.0, 9.0, 0.125, 2.0]), 4, 5, 0.1, 0.02, seed)


def test_finish_of_a_uniform_response(lib):
    seed = np.array([1.0, 0.0, 2.0, -3.0])
    for Kx, Kt, sx, st in ((4, 5, 0.0125, math.pi / 360), (1, 1, 0.5, 0.25), (8, 16, 0.0125, 0.001), (0, 0, 0.0125, 0.001), (2, 0, 0.25, 0.5)):
        sums = sums_of(np.ones(ref.candidates(Kx, Kt)), Kx, Kt)
        assert all(float(s).is_integer() for s in sums) and np.all(sums[[1, 2, 3, 5, 6, 8]] == 0.0)
        mean, cov = check_finish(lib, sums, Kx, Kt, sx, st, seed)
        assert np.array_equal(mean[2:], seed[2:])  # the mean offsets are exactly 0
        want = [ref.uniform_covariance(Kx, sx), ref.uniform_covariance(Kx, sx), ref.uniform_covariance(Kt, st)]
        exact = ref.finish_exact(sums, sx, st)[1]
        for a in range(3):
            assert exact[a][a] == want[a] and all(exact[a][b] == 0 and cov[a, b] == 0.0 for b in range(3) if b != a)
            assert abs(Fraction(float(cov[a, a])) - want[a]) <= 8 * Fraction(1, 2 ** 53) * want[a]


def test_finish_without_weight_and_refusals(lib):
    seed = np.array([0.6, 0.8000000000000002, 5.0, -7.0])
    for S0 in (0.0, -0.0, math.inf, -math.inf, math.nan):
        status, mean, cov, valid = finish(lib, [S0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0], 4, 5, 0.1, 0.01, seed)
        assert status == capi.MCL_OK and valid == 0 and np.array_equal(bits(mean), bits(seed)) and np.all(cov == 0.0)
    sums = np.arange(1.0, 11.0)
    for Kx, Kt, sx, st in ((33, 5, 0.1, 0.01), (4, 65, 0.1, 0.01), (4, 5, -0.1, 0.01), (4, 5, 0.1, 0.0), (4, 5, math.nan, 0.01), (4, 64, 0.1, 0.05)):
        status, mean, cov, valid = finish(lib, sums, Kx, Kt, sx, st, seed)
        assert status == capi.MCL_ERR_INVALID_ARGUMENT and valid == 7 and np.all(mean == 99.0) and np.all(cov == 99.0)
    for c in range(4):
        bad = seed.copy()
        bad[c] = math.inf
        status, mean, cov, valid = finish(lib, sums, 4, 5, 0.1, 0.01, bad)
        assert status == capi.MCL_ERR_INVALID_ARGUMENT and valid == 7 and np.all(mean == 99.0)
    p = capi.LocalSearchParams(4, 5, 0.1, 0.01)
    mean, cov, valid = np.zeros(4), np.zeros(9), C.c_int32(0)
    args = [dp(sums), C.byref(p), dp(seed), dp(mean), dp(cov), C.byref(valid)]
    for null in (0, 2, 3, 4, 5):
        assert lib.mcl_local_search_finish(*[None if k == null else a for k, a in enumerate(args)]) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_local_search_finish(dp(sums), None, dp(seed), dp(mean), dp(cov), C.byref(valid)) == capi.MCL_OK and valid.value == 1  # NULL: the defaults


def test_the_symbols_are_declared():
    for name in ("mcl_default_local_search_params", "mcl_local_search", "mcl_local_search_landmarks", "mcl_local_search_bearings",
                 "mcl_local_search_candidates", "mcl_local_search_finish"):
        assert name in capi.exported_names()
    header = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    assert "mcl_local_search(" in header and "typedef struct mcl_local_hit" in header
    assert C.sizeof(capi.LocalHit) == 256 and C.sizeof(capi.LocalSearchParams) == 24 and C.sizeof(capi.LocalSearchInfo) == 32


def test_search_host_still_builds_alone(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(CSRC, "search_host.cpp"), "-o", str(tmp_path / "libsearch_host.so")])


def test_the_stand_alone_check_passes_under_the_sanitizers(tmp_path):
    """tests/cpp/local_search_host_check.cpp with local_search_host.cpp, as a program of its own under the address and
    undefined-behaviour sanitizers: nothing of it is loaded into this process."""
    exe = tmp_path / "local_search_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "local_search_host_check.cpp"),
                           os.path.join(CSRC, "local_search_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "local_search_host_check OK", out.stdout + out.stderr
