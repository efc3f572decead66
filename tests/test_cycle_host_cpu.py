"""The update cycle's host decisions (beluga_amd/csrc/cycle_host.cpp) on the CPU: a plain g++ compiles the file with a short driver that
takes one command and its numbers as arguments (reals as C99 hex floats, so nothing is rounded on the way) and prints what the
function returned.  The motion sampler, the covariance transform, the planner of the likelihood-field kernels, the key frame, the
policies and the shard arithmetic are checked against restatements written here and against the oracle, without a GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import binding as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
// driver <command> <numbers ...>; every real is printed as a hex float.
//   sampler  kind alpha5 a1 a2 a3 a4 threshold  pose(c s x y) prev(c s x y)      -> kind m1 s1 mt st m2 s2 first_c first_s
//   close    sampler[9] sampler[9]                                               -> 0 / 1
//   cov      cov[9]                                                              -> ok T[9]
//   keyframe valid mean[3] sigma[3]  have_motion sampler[9]  moves layout  patch_useful resolution scan_extent key_warp key_bits_xy
//                                                                                -> ok cx cy c0 s0 inv_x inv_y inv_t t_off layout bits_xy
//   policy   alpha_slow alpha_fast slow fast selective fires norm_sum norm_sumsq n -> p ess resample slow fast
//   filter   alpha inputs ...                                                    -> the outputs
//   moved    latest(c s x y) pose(c s x y) min_d min_a                           -> 0 / 1
//   everyn   current interval                                                    -> the counter
//   bounds   n world                                                             -> first count, per rank
//   capacity n world permille                                                    -> the capacity
//   block    pos cnt n_out world                                                 -> per rank: out0 send[world] recv[world]
//   planner  events ...   (below)                                                -> a line per event
//   family   sensor_kind                                                         -> 0 .. 3 (SensorFamily, in its declared order)
//   gridsmall small_fused n max_particles                                        -> 0 / 1 (grid_cycle_is_small)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cycle_host.h"

using namespace mcl;

static char** g_arg;
static double real() { return std::strtod(*g_arg++, nullptr); }
static long long word() { return std::strtoll(*g_arg++, nullptr, 0); }
static unsigned long long uword() { return std::strtoull(*g_arg++, nullptr, 0); }
static Pose2 pose() {
  const double c = real(), s = real(), x = real(), y = real();
  return Pose2{Rot2{c, s}, x, y};
}
static DiffDriveSampler sampler() {
  DiffDriveSampler s{};
  s.kind = static_cast<int>(word());
  s.m1 = real(), s.s1 = real(), s.mt = real(), s.st = real(), s.m2 = real(), s.s2 = real(), s.first_c = real(), s.first_s = real();
  return s;
}
static CloudEstimate cloud() {
  CloudEstimate c;
  const bool valid = word() != 0;
  double mean[3], sigma[3];
  for (double& v : mean) v = real();
  for (double& v : sigma) v = real();
  if (valid) c.set(mean, sigma);
  return c;
}
static bool set_option(Tuning& t, const std::string& name, int value) {
  if (name == "lf_variant") t.lf_variant = value;
  else if (name == "lf_table") t.lf_table = value;
  else if (name == "lf_patch") t.lf_patch = value;
  else if (name == "lf_dispersed") t.lf_dispersed = value;
  else if (name == "lf_far_tiles") t.lf_far_tiles = value;
  else if (name == "key_layout") t.key_layout = value;
  else if (name == "key_curve") t.key_curve = value;
  else if (name == "sort_min_particles") t.sort_min_particles = value;
  else if (name == "beam_sort_min_particles") t.beam_sort_min_particles = value;
  else if (name == "lf_small_particles") t.lf_small_particles = value;
  else return false;
  return true;
}

// planner events, each "name" or "name:a,b,c":
//   kind:k  n:particles  palette:0/1  far:0/1  res:resolution  opt:name,value  cloud:sx,sy,st  nocloud
//   begin  decide:planned,through  consume  install:how,planned,through  look
// A line per event: decided patches beams useful ordering layout dispersed sparse (patches / beams: what the last decide returned).
static int planner(int argc, char** argv) {
  Tuning tuning;
  int kind = MCL_SENSOR_LIKELIHOOD_FIELD;
  unsigned long long n = 100000;
  bool palette = true, far = true;
  double resolution = 0.05;
  CloudEstimate where;
  LfPlanner p;
  LfPlanner::Mode mode{false, false};
  for (int k = 0; k < argc; ++k) {
    std::string name(argv[k]);
    std::vector<std::string> a;
    if (const size_t colon = name.find(':'); colon != std::string::npos) {
      std::string rest = name.substr(colon + 1);
      name.resize(colon);
      size_t from = 0;
      while (true) {
        const size_t comma = rest.find(',', from);
        a.push_back(rest.substr(from, comma == std::string::npos ? comma : comma - from));
        if (comma == std::string::npos) break;
        from = comma + 1;
      }
    }
    auto u = [&](size_t i) { return std::strtoull(a.at(i).c_str(), nullptr, 0); };
    auto r = [&](size_t i) { return std::strtod(a.at(i).c_str(), nullptr); };
    const LfSite site{kind, n, palette, far, resolution, tuning};
    if (name == "kind") kind = static_cast<int>(u(0));
    else if (name == "n") n = u(0);
    else if (name == "palette") palette = u(0) != 0;
    else if (name == "far") far = u(0) != 0;
    else if (name == "res") resolution = r(0);
    else if (name == "opt") { if (!set_option(tuning, a.at(0), std::atoi(a.at(1).c_str()))) return 2; }
    else if (name == "cloud") { const double mean[3] = {0, 0, 0}, sigma[3] = {r(0), r(1), r(2)}; where.set(mean, sigma); }
    else if (name == "nocloud") where.forget();
    else if (name == "begin") p.cycle_begins();
    else if (name == "decide") mode = p.decide(site, where, u(0), u(1));
    else if (name == "consume") p.mode_consumed();
    else if (name == "install") p.set_installed(static_cast<LfPlanner::Installed>(u(0)), u(1), u(2));
    else if (name != "look") return 2;
    const LfSite now{kind, n, palette, far, resolution, tuning};
    std::printf("%d %d %d %d %d %u %d %d\n", p.decided() ? 1 : 0, mode.patches ? 1 : 0, mode.beams ? 1 : 0, p.patch_useful() ? 1 : 0,
                p.wants_ordering(now) ? 1 : 0, p.key_layout(now), p.gathers_dispersed(tuning) ? 1 : 0,
                LfPlanner::hopelessly_sparse(now, where) ? 1 : 0);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string what = argv[1];
  g_arg = argv + 2;
  if (what == "planner") return planner(argc - 2, argv + 2);
  if (what == "sampler") {
    const int kind = static_cast<int>(word());
    const double alpha5 = real();
    mcl_diffdrive_params a{};
    a.rotation_noise_from_rotation = real(), a.rotation_noise_from_translation = real();
    a.translation_noise_from_translation = real(), a.translation_noise_from_rotation = real(), a.distance_threshold = real();
    const Pose2 now = pose(), prev = pose();
    const DiffDriveSampler s = make_sampler(now, prev, a, kind, alpha5);
    std::printf("%d %a %a %a %a %a %a %a %a\n", s.kind, s.m1, s.s1, s.mt, s.st, s.m2, s.s2, s.first_c, s.first_s);
  } else if (what == "close") {
    const DiffDriveSampler a = sampler(), b = sampler();
    std::printf("%d\n", samplers_close(a, b) ? 1 : 0);
  } else if (what == "cov") {
    double cov[9], T[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (double& v : cov) v = real();
    std::printf("%d", covariance_to_transform(cov, T) ? 1 : 0);
    for (const double v : T) std::printf(" %a", v);
    std::printf("\n");
  } else if (what == "keyframe") {
    const CloudEstimate c = cloud();
    const bool have_motion = word() != 0;
    const DiffDriveSampler s = sampler();
    const int moves = static_cast<int>(word());
    const uint32_t layout = static_cast<uint32_t>(word());
    KeyFrameInputs in{};
    in.patch_useful = word() != 0, in.resolution = real(), in.scan_extent = real();
    in.key_warp = static_cast<int>(word()), in.key_bits_xy = static_cast<int>(word());
    KeyFrame f{};
    const bool ok = predict_key_frame(c, have_motion ? &s : nullptr, moves, layout, in, &f);
    std::printf("%d %a %a %a %a %a %a %a %a %u %u\n", ok ? 1 : 0, f.cx, f.cy, f.c0, f.s0, static_cast<double>(f.inv_x), static_cast<double>(f.inv_y),
                static_cast<double>(f.inv_t), static_cast<double>(f.t_off), f.layout, f.bits_xy);
  } else if (what == "policy") {
    ExponentialFilter slow, fast;
    slow.alpha = real(), fast.alpha = real(), slow.output = real(), fast.output = real();
    const bool selective = word() != 0, fires = word() != 0;
    const double norm_sum = real(), norm_sumsq = real();
    const HostPolicy r = host_policy(slow, fast, selective, fires, norm_sum, norm_sumsq, uword());
    std::printf("%a %a %d %a %a\n", r.random_state_probability, r.ess, r.resample ? 1 : 0, slow.output, fast.output);
  } else if (what == "filter") {
    ExponentialFilter f;
    f.alpha = real();
    while (*g_arg) std::printf("%a ", f(real()));
    std::printf("\n");
  } else if (what == "moved") {
    const Pose2 latest = pose(), now = pose();
    const double min_d = real(), min_a = real();
    std::printf("%d\n", moved_enough(latest, now, min_d, min_a) ? 1 : 0);
  } else if (what == "everyn") {
    const uint64_t current = uword(), interval = uword();
    std::printf("%llu\n", static_cast<unsigned long long>(next_every_n(current, interval)));
  } else if (what == "bounds") {
    const uint64_t n = uword();
    const uint32_t world = static_cast<uint32_t>(uword());
    for (uint32_t r = 0; r < world; ++r) {
      uint64_t first = 0, count = 0;
      shard_bounds(n, world, r, &first, &count);
      std::printf("%llu %llu\n", static_cast<unsigned long long>(first), static_cast<unsigned long long>(count));
    }
  } else if (what == "capacity") {
    const uint64_t n = uword();
    const uint32_t world = static_cast<uint32_t>(uword()), permille = static_cast<uint32_t>(uword());
    std::printf("%llu\n", static_cast<unsigned long long>(padded_capacity(n, world, permille)));
  } else if (what == "family") {
    std::printf("%d\n", static_cast<int>(sensor_family(static_cast<int>(word()))));
  } else if (what == "gridsmall") {
    GridCycleFacts f{};
    f.small_fused = word() != 0, f.n = uword(), f.max_particles = uword();
    std::printf("%d\n", grid_cycle_is_small(f) ? 1 : 0);
  } else if (what == "block") {
    const uint64_t pos = uword(), cnt = uword(), n_out = uword();
    const uint32_t world = static_cast<uint32_t>(uword());
    std::vector<uint64_t> send(world), recv(world);
    for (uint32_t r = 0; r < world; ++r) {
      const uint64_t out0 = rebalance_block(pos, cnt, n_out, world, r, send.data(), recv.data());
      std::printf("%llu", static_cast<unsigned long long>(out0));
      for (const uint64_t v : send) std::printf(" %llu", static_cast<unsigned long long>(v));
      for (const uint64_t v : recv) std::printf(" %llu", static_cast<unsigned long long>(v));
      std::printf("\n");
    }
  } else {
    return 2;
  }
  return *g_arg ? 3 : 0;
}
"""


def _compile(d, name, extra):
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / name
    csrc = os.path.join(ROOT, "beluga_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                          ["-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "cycle_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("cycle_host"), "driver", [])


def _arg(v):
    if isinstance(v, (bool, np.bool_)):
        return str(int(v))
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    v = float(v)
    return float.hex(v) if math.isfinite(v) else repr(v)  # (strtod reads "inf" and "nan")


def _value(word):
    return float.fromhex(word) if "x" in word else float(word)


def call(driver, what, *args):
    """The rows of numbers the driver printed."""
    flat = []
    for a in args:  # (integers stay integers: a list is not taken through an array)
        flat.extend(a.reshape(-1).tolist() if isinstance(a, np.ndarray) else a if isinstance(a, (list, tuple)) else [a])
    out = subprocess.check_output([driver, what] + [_arg(v) for v in flat], text=True)
    return [[_value(w) for w in line.split()] for line in out.splitlines()]


# ---- the motion sampler -------------------------------------------------------------------------------------------------------------
# The restatement keeps rotations as Sophus::SO2d does, as unit complex numbers (so2.hpp: the constructors normalise, a product
# renormalises to first order where its squared norm is not 1, log() is atan2): the reference's own operations in the reference's order.

DIFFERENTIAL, OMNIDIRECTIONAL, STATIONARY = 0, 1, 2


class SO2:
    def __init__(self, re, im):
        length = math.hypot(re, im)
        self.c, self.s = re / length, im / length

    @classmethod
    def exp(cls, theta):
        return cls(math.cos(theta), math.sin(theta))

    def log(self):
        return math.atan2(self.s, self.c)

    def inverse(self):
        return SO2(self.c, -self.s)

    def __mul__(self, o):
        re, im = self.c * o.c - self.s * o.s, self.c * o.s + self.s * o.c
        n2 = re * re + im * im
        if n2 != 1.0:
            scale = 2.0 / (1.0 + n2)
            re, im = re * scale, im * scale
        return SO2(re, im)


def rotation_variance(r):  # differential_drive_model.hpp:167-173
    delta = min(abs(r.log()), abs((r * SO2.exp(math.pi)).log()))
    return delta * delta


def reference_sampler(kind, pose, prev, alphas, threshold, alpha5):
    """(m1, s1, mt, st, m2, s2, first_c, first_s); pose = (x, y, theta).  differential_drive_model.hpp:129-154,
    omnidirectional_drive_model.hpp:102-131; the stationary model (stationary_model.hpp:53-61) ignores the control action."""
    a1, a2, a3, a4 = alphas
    tx, ty = pose[0] - prev[0], pose[1] - prev[1]
    distance = math.sqrt(tx * tx + ty * ty)
    dv = distance * distance
    previous, current = SO2.exp(prev[2]), SO2.exp(pose[2])
    heading = SO2.exp(math.atan2(ty, tx))
    first = heading * previous.inverse() if distance > threshold else SO2(1.0, 0.0)
    if kind == STATIONARY:
        return (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, first.c, first.s)
    if kind == OMNIDIRECTIONAL:
        rotation = current * previous.inverse()
        rv = rotation_variance(rotation)
        return (rotation.log(), math.sqrt(a1 * rv + a2 * dv), distance, math.sqrt(a3 * dv + a4 * rv), 0.0, math.sqrt(alpha5 * dv + a4 * rv),
                first.c, first.s)
    second = current * previous.inverse() * first.inverse()
    v1, v2 = rotation_variance(first), rotation_variance(second)
    return (first.log(), math.sqrt(a1 * v1 + a2 * dv), distance, math.sqrt(a3 * dv + a4 * (v1 + v2)), second.log(), math.sqrt(a1 * v2 + a2 * dv),
            first.c, first.s)


ALPHAS, THRESHOLD, ALPHA5 = (0.1, 0.05, 0.1, 0.05), 0.01, 0.07
PREV = (1.0, 2.0, 0.4)
MOVES = {
    "pure rotation": (1.0 + 0.004 * math.cos(0.4), 2.0 + 0.004 * math.sin(0.4), 0.9),  # 4 mm: below distance_threshold, `first` is the identity
    "straight": (1.0 + 0.3 * math.cos(0.4), 2.0 + 0.3 * math.sin(0.4), 0.4),
    "backwards": (1.0 - 0.3 * math.cos(0.4), 2.0 - 0.3 * math.sin(0.4), 0.45),  # `first` is near pi: rotation_variance takes the flipped branch
    "arc": (1.25, 2.2, 0.7),
    "zero": PREV,
}


def _pose_args(p):
    r = SO2.exp(p[2])
    return [r.c, r.s, p[0], p[1]]


@pytest.mark.parametrize("kind", [DIFFERENTIAL, OMNIDIRECTIONAL, STATIONARY])
@pytest.mark.parametrize("move", sorted(MOVES))
def test_sampler_matches_the_reference_models(driver, kind, move):
    pose = MOVES[move]
    got = call(driver, "sampler", kind, ALPHA5, *ALPHAS, THRESHOLD, _pose_args(pose), _pose_args(PREV))[0]
    want = reference_sampler(kind, pose, PREV, ALPHAS, THRESHOLD, ALPHA5)
    assert got[0] == kind
    np.testing.assert_allclose(got[1:], want, rtol=1e-15, atol=0)
    if move == "pure rotation":
        assert got[7:] == [1.0, 0.0]
        if kind == DIFFERENTIAL:
            assert got[1] == 0.0 and got[5] == pytest.approx(0.5, abs=1e-15)  # the whole turn is the second rotation
    if move == "backwards" and kind == DIFFERENTIAL:
        assert abs(got[1]) > 3.0 and got[2] < 0.1  # |first| is near pi, its variance is the flipped rotation's
    if move == "zero" and kind != STATIONARY:
        assert got[1:7] == [0.0] * 6
    if kind == STATIONARY:
        assert got[1:7] == [0.0] * 6


# ---- covariance_to_transform --------------------------------------------------------------------------------------------------------

def _rotation(a, b, c):
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    rz = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rx = np.array([[1, 0, 0], [0, cc, -sc], [0, sc, cc]])
    return rz @ ry @ rx


def _symmetric(eigenvalues):
    q = _rotation(0.3, -0.7, 1.1)
    m = q @ np.diag(eigenvalues) @ q.T
    return (m + m.T) / 2


COVARIANCES = {
    "diagonal": np.diag([0.25, 0.09, 0.04]),
    "full": _symmetric([0.5, 0.2, 0.03]),
    "rank deficient": _symmetric([0.4, 0.1, 0.0]),
}


@pytest.mark.parametrize("name", sorted(COVARIANCES))
def test_covariance_transform_reproduces_the_matrix_and_agrees_with_the_oracle(driver, name):
    cov = COVARIANCES[name]
    row = call(driver, "cov", cov)[0]
    assert row[0] == 1
    T = np.asarray(row[1:]).reshape(3, 3)
    np.testing.assert_allclose(T @ T.T, cov, rtol=0, atol=1e-12)
    want = orc.covariance_transform(cov)
    assert want is not None
    # up to the sign of columns: an eigenvector's sign is the solver's choice (eigenvalues apart by 0.05 or more, in ascending order in both)
    for j in range(3):
        assert min(np.max(np.abs(T[:, j] - want[:, j])), np.max(np.abs(T[:, j] + want[:, j]))) <= 1e-12, (j, T, want)


@pytest.mark.parametrize("cov", [
    np.array([[1.0, 2.0, 0], [0.0, 1.0, 0], [0, 0, 1.0]]),  # not symmetric
    np.diag([1.0, -1.0, 1.0]),                              # negative eigenvalue
    np.array([[1.0, float("nan"), 0], [float("nan"), 1.0, 0], [0, 0, 1.0]]),
    np.diag([1.0, float("nan"), 1.0]),
    np.array([[1.0, float("inf"), 0], [float("inf"), 1.0, 0], [0, 0, 1.0]]),
], ids=["asymmetric", "negative", "nan off the diagonal", "nan on the diagonal", "infinite"])
def test_covariance_transform_rejects_what_initialize_rejects(driver, cov):
    assert call(driver, "cov", cov)[0][0] == 0
    if np.all(np.isfinite(cov)):
        assert orc.covariance_transform(cov) is None


# ---- samplers_close -----------------------------------------------------------------------------------------------------------------

def _sampler(kind=DIFFERENTIAL, m1=0.02, s1=0.04, mt=0.3, st=0.03, m2=0.03, s2=0.05, first=0.02):
    return [kind, m1, s1, mt, st, m2, s2, math.cos(first), math.sin(first)]


@pytest.mark.parametrize("kind", [DIFFERENTIAL, OMNIDIRECTIONAL, STATIONARY])
def test_samplers_close_is_reflexive_and_false_across_kinds(driver, kind):
    s = _sampler(kind)
    assert call(driver, "close", s, s) == [[1]]
    zero = [kind] + [0.0] * 8
    assert call(driver, "close", zero, zero) == [[1]]  # (what make_sampler gives the stationary model)
    for other in {DIFFERENTIAL, OMNIDIRECTIONAL, STATIONARY} - {kind}:
        assert call(driver, "close", s, _sampler(other)) == [[0]]


@pytest.mark.parametrize("field", ["s1", "st", "s2"])
def test_samplers_close_noise_ratio_bound(driver, field):
    """a <= 1.5 b + 1e-3, both ways."""
    base = _sampler()
    b = dict(s1=0.04, st=0.03, s2=0.05)[field]
    edge = 1.5 * b + 1e-3
    for value, want in ((edge * (1 - 1e-9), 1), (edge * (1 + 1e-9), 0)):
        other = _sampler(**{field: value})
        assert call(driver, "close", other, base) == [[want]]
        assert call(driver, "close", base, other) == [[want]]  # (the ratio is tested both ways)


def test_samplers_close_translation_bound(driver):
    """|mt - predicted| <= 0.3 max(|predicted|, 0.02)"""
    base = _sampler(mt=0.3)
    for mt, want in ((0.3 + 0.09 * (1 - 1e-9), 1), (0.3 + 0.09 * (1 + 1e-9), 0), (0.3 - 0.09 * (1 - 1e-9), 1), (0.3 - 0.09 * (1 + 1e-9), 0)):
        assert call(driver, "close", _sampler(mt=mt, m1=0.0, first=0.0), _sampler(mt=0.3, m1=0.0, first=0.0)) == [[want]]
    # a prediction that stands still: 30 % of 2 cm
    still = _sampler(mt=0.0, m1=0.0)
    assert call(driver, "close", _sampler(mt=0.006 * (1 - 1e-9), m1=0.0), still) == [[1]]
    assert call(driver, "close", _sampler(mt=0.006 * (1 + 1e-9), m1=0.0), still) == [[0]]
    assert base is not None


@pytest.mark.parametrize("kind", [DIFFERENTIAL, OMNIDIRECTIONAL])
def test_samplers_close_turn_bound(driver, kind):
    """The whole turn (m1 + m2 of the differential model, m1 of the omnidirectional one) within 0.15 rad."""
    base = _sampler(kind, m1=0.0, m2=0.0, mt=0.0)  # (no translation: the lateral bound is out of the way)
    for turn, want in ((0.15 * (1 - 1e-9), 1), (0.15 * (1 + 1e-9), 0)):
        other = _sampler(kind, m1=0.0, m2=turn, mt=0.0) if kind == DIFFERENTIAL else _sampler(kind, m1=turn, m2=0.0, mt=0.0)
        assert call(driver, "close", other, base) == [[want]]


@pytest.mark.parametrize("kind", [DIFFERENTIAL, OMNIDIRECTIONAL])
def test_samplers_close_lateral_bound(driver, kind):
    """The directions of the two translations apart by an angle that makes 5 cm over the longer of them."""
    mt = 0.5
    angle = 0.05 / mt
    for a, want in ((angle * (1 - 1e-6), 1), (angle * (1 + 1e-6), 0)):
        if kind == DIFFERENTIAL:  # the direction is the first rotation; the second takes the turn back
            now, predicted = _sampler(kind, m1=a, m2=-a, mt=mt), _sampler(kind, m1=0.0, m2=0.0, mt=mt)
        else:  # the direction is `first`
            now, predicted = _sampler(kind, m1=0.0, mt=mt, first=a), _sampler(kind, m1=0.0, mt=mt, first=0.0)
        assert call(driver, "close", now, predicted) == [[want]]


# ---- LfPlanner ----------------------------------------------------------------------------------------------------------------------

FIELDS = ("decided", "patches", "beams", "useful", "ordering", "layout", "dispersed", "sparse")
KEPT, FRESH, DISPERSED = 0, 1, 2


def plan(driver, *events):
    out = subprocess.check_output([driver, "planner"] + list(events), text=True).splitlines()
    assert len(out) == len(events)
    return [dict(zip(FIELDS, map(int, line.split()))) for line in out]


def cycle(planned, through):
    """One cycle's three events; the decision is what the second one printed."""
    return ["begin", "decide:%d,%d" % (planned, through), "consume"]


def decisions(driver, setup, totals):
    steps = plan(driver, *setup, *[e for t in totals for e in cycle(*t)])
    return steps[len(setup) + 1::3]


def test_a_fresh_planner_takes_patches_and_a_good_report_keeps_them(driver):
    got = decisions(driver, [], [(0, 0), (1000, 250), (1000, 250), (2000, 500)])  # 4 x through >= planned, at the bound
    assert [d["patches"] for d in got] == [1, 1, 1, 1]
    assert all(d["useful"] == 1 and d["beams"] == 0 and d["dispersed"] == 0 and d["layout"] == 0 and d["ordering"] == 1 for d in got)


@pytest.mark.parametrize("lf_dispersed, beams", [(2, 0), (0, 0), (1, 1)])
def test_a_poor_report_switches_to_the_dispersed_kernel_and_probes_on_the_16th_decision(driver, lf_dispersed, beams):
    """The launch that reports is followed by 15 decisions for the dispersed kernel and a probe on the 16th; and again."""
    totals = [(0, 0)] + [(1000, 249)] * 40  # one below the bound; nothing reports after it
    got = decisions(driver, ["opt:lf_dispersed,%d" % lf_dispersed], totals)
    patches = [d["patches"] for d in got[1:]]
    assert patches == ([0] * 15 + [1]) * 2 + [0] * 8
    for d in got[1:]:
        assert d["useful"] == 0 and d["layout"] == 1  # position-major keys while the set is reported as dispersed
        assert d["dispersed"] == 1 - d["patches"]
        assert d["beams"] == (beams if not d["patches"] else 0)
        assert d["ordering"] == (0 if d["beams"] else 1)  # (the wave-per-particle kernel needs no order)


def test_a_probe_that_reports_well_returns_to_patches(driver):
    totals = [(0, 0)] + [(1000, 249)] * 16 + [(2000, 1249)] * 3
    got = decisions(driver, [], totals)
    assert [d["patches"] for d in got[1:]] == [0] * 15 + [1] + [1, 1, 1]
    assert [d["useful"] for d in got[-3:]] == [1, 1, 1] and got[-1]["layout"] == 0


def _sparse_bound(sx, sy, st, resolution):
    """Particles below which hopelessly_sparse holds: 56 poses in a patch-sized volume of a set taken as uniform."""
    side = 40.0 * resolution
    volume = max(12.0 * sx * sy, side * side) * max(min(2.0 * math.pi, math.sqrt(12.0) * st), 0.05)
    return 56.0 * volume / (side * side * 0.05)


@pytest.mark.parametrize("sigma", [(0.01, 0.01, 0.001), (5.0, 7.0, 0.02), (20.0, 20.0, 3.0)], ids=["tight", "wide", "everywhere"])
def test_a_probe_is_suppressed_while_the_set_is_hopelessly_sparse(driver, sigma):
    bound = _sparse_bound(*sigma, 0.05)
    assert abs(bound - round(bound)) > 1e-6 or sigma[0] == 0.01  # (the tight set's bound is 56 exactly: 55 below, 56 not)
    below, above = math.ceil(bound) - 1, math.ceil(bound)
    totals = [(0, 0)] + [(1000, 0)] * 16
    for n, probe in ((below, 0), (above, 1)):
        setup = ["n:%d" % n, "cloud:%r,%r,%r" % sigma, "opt:sort_min_particles,0", "opt:lf_small_particles,0"]
        got = decisions(driver, setup, totals)
        assert [d["patches"] for d in got[1:]] == [0] * 15 + [probe]
        assert got[-1]["sparse"] == 1 - probe
    # without an estimate of the set nothing is known about its spread: the probe goes ahead
    got = decisions(driver, ["n:%d" % below, "nocloud"], totals)
    assert got[-1]["patches"] == 1 and got[-1]["sparse"] == 0


def test_the_tight_sets_bound_is_56_poses(driver):
    assert _sparse_bound(0.01, 0.01, 0.001, 0.05) == 56.0


def test_totals_that_wrap_past_2_32_give_no_false_verdict(driver):
    # `planned` wraps, `through` does not: 512 planned, 512 through (without the modulus: 2^64 - ... planned, a false "dispersed")
    got = decisions(driver, ["install:%d,%d,%d" % (FRESH, 0xFFFFFF00, 0x10)], [(0x100, 0x210)])
    assert got[0]["patches"] == 1 and got[0]["useful"] == 1
    # `through` wraps: 1024 planned, 32 through (without the modulus: 2^64 - ... through, a false "useful")
    got = decisions(driver, ["install:%d,%d,%d" % (FRESH, 0x100, 0xFFFFFFF0)], [(0x500, 0x10)])
    assert got[0]["patches"] == 0 and got[0]["useful"] == 0
    # both wrap, at the bound and one below it
    for through, useful in ((0xFFFFFFF0 + 256 - (1 << 32), 1), (0xFFFFFFF0 + 255 - (1 << 32), 0)):
        got = decisions(driver, ["install:%d,%d,%d" % (FRESH, 0xFFFFFC00, 0xFFFFFFF0)], [(0, through)])
        assert got[0]["useful"] == useful


@pytest.mark.parametrize("lf_patch, patches", [(0, 0), (2, 1)])
def test_lf_patch_0_and_2_bypass_the_statistics(driver, lf_patch, patches):
    totals = [(0, 0), (1000, 0), (1000, 0), (2000, 1000), (2000, 1000)]
    got = decisions(driver, ["opt:lf_patch,%d" % lf_patch], totals)
    assert [d["patches"] for d in got] == [patches] * 5
    assert all(d["useful"] == 1 and d["beams"] == 0 and d["layout"] == 0 for d in got)  # no report is looked at
    # ... and a planner that has learnt "dispersed" forgets nothing while the option is forced
    got = decisions(driver, ["install:%d,0,0" % DISPERSED, "opt:lf_patch,%d" % lf_patch], totals)
    assert [d["patches"] for d in got] == [patches] * 5 and all(d["useful"] == 0 for d in got)


def test_the_three_install_set_transitions(driver):
    poor = [e for t in [(0, 0), (1000, 0), (1000, 0)] for e in cycle(*t)]  # leaves: not useful, probe in 14
    # kept: nothing changes - the probe comes where it would have
    kept = plan(driver, *poor, "install:%d,5000,5000" % KEPT, *[e for _ in range(14) for e in cycle(1000, 0)])
    assert kept[len(poor)]["useful"] == 0
    assert [d["patches"] for d in kept[len(poor) + 2::3]] == [0] * 13 + [1]
    # fresh: useful again, and the totals of the moment are history - the same totals are no report
    fresh = plan(driver, *poor, "install:%d,1000,0" % FRESH, *cycle(1000, 0), *cycle(1000, 0))
    assert fresh[len(poor)]["useful"] == 1 and fresh[len(poor)]["layout"] == 0
    assert [d["patches"] for d in fresh[len(poor) + 2::3]] == [1, 1]
    # ... and a report behind it counts from them: 100 planned, 24 through
    fresh = plan(driver, *poor, "install:%d,1000,0" % FRESH, *cycle(1100, 24))
    assert fresh[-2]["patches"] == 0 and fresh[-2]["useful"] == 0
    # dispersed: the first cycle already takes the kernel for dispersed sets, the probe comes on the 16th decision
    for before in ([], poor):
        steps = plan(driver, *before, "install:%d,1000,1000" % DISPERSED, *[e for _ in range(17) for e in cycle(1000, 1000)])
        at = len(before)
        assert steps[at]["useful"] == 0 and steps[at]["layout"] == 1
        assert [d["patches"] for d in steps[at + 2::3]] == [0] * 15 + [1, 0]
        assert all(d["dispersed"] == 1 - d["patches"] for d in steps[at + 2::3])


@pytest.mark.parametrize("kind", [1, 3, 4, 5], ids=["beam", "ndt", "landmark", "bearing"])
@pytest.mark.parametrize("lf_patch", [1, 2])
def test_other_sensor_kinds_never_ask_for_patches(driver, kind, lf_patch):
    got = decisions(driver, ["kind:%d" % kind, "opt:lf_patch,%d" % lf_patch], [(0, 0), (1000, 1000), (2000, 1000)])
    assert all(d["patches"] == 0 and d["beams"] == 0 and d["useful"] == 1 for d in got)
    # (the beam model orders its sets from beam_sort_min_particles on; the models with a map of their own never do)
    assert all(d["ordering"] == (1 if kind == 1 else 0) and d["layout"] == 0 for d in got)


def test_lf_variants_other_than_the_sorted_lanes_look_at_no_statistics(driver):
    for variant, beams in ((0, 0), (1, 0), (3, 1)):
        got = decisions(driver, ["opt:lf_variant,%d" % variant], [(0, 0), (1000, 0), (2000, 0)])
        assert all(d["patches"] == 0 and d["beams"] == beams and d["useful"] == 1 and d["ordering"] == 0 for d in got)
    got = decisions(driver, ["opt:lf_variant,3", "palette:0"], [(0, 0)])  # the lanes-over-beams kernel reads the palette table
    assert got[0]["beams"] == 0
    got = decisions(driver, ["opt:lf_variant,3", "opt:lf_table,1"], [(0, 0)])
    assert got[0]["beams"] == 0


@pytest.mark.parametrize("n", [1000, 16383, 16384, 65535, 65536, 100000, (1 << 32) - 1, 1 << 32])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("state", ["fresh", "dispersed", "dispersed beams", "no palette"])
def test_wants_ordering_does_not_depend_on_the_mode_being_decided_unless_it_is_beams(driver, n, kind, state):
    setup = ["kind:%d" % kind, "n:%d" % n]
    if state.startswith("dispersed"):
        setup.append("install:%d,0,0" % DISPERSED)
    if state == "dispersed beams":
        setup.append("opt:lf_dispersed,1")
    if state == "no palette":
        setup.append("palette:0")
    steps = plan(driver, *setup, "look", *cycle(0, 0))
    before, decided, after = steps[-4], steps[-2], steps[-1]
    assert (before["decided"], decided["decided"], after["decided"]) == (0, 1, 0)
    assert before["ordering"] == after["ordering"]
    if not decided["beams"]:
        assert decided["ordering"] == before["ordering"]
    else:
        assert decided["ordering"] == 0 and kind in (0, 2) and state == "dispersed beams" and n >= 65536
    # the answer itself, where no mode is decided
    if kind in (3, 4, 5) or n >= (1 << 32):
        want = 0
    elif kind == 1:
        want = int(n >= 16384)
    else:
        want = int(n >= 16384 and not (n < 65536 and state != "no palette"))
    assert before["ordering"] == want


def test_key_layout_follows_the_forced_option_and_the_curve(driver):
    assert plan(driver, "look")[0]["layout"] == 0
    assert plan(driver, "opt:key_curve,0", "look")[-1]["layout"] == 2
    assert plan(driver, "opt:key_layout,1", "look")[-1]["layout"] == 1
    assert plan(driver, "opt:key_layout,0", "install:%d,0,0" % DISPERSED)[-1]["layout"] == 0
    assert plan(driver, "install:%d,0,0" % DISPERSED)[-1]["layout"] == 1
    assert plan(driver, "opt:key_curve,0", "install:%d,0,0" % DISPERSED)[-1]["layout"] == 3
    for off in ("far:0", "opt:lf_far_tiles,0", "opt:lf_patch,2", "kind:1", "kind:3"):  # position-major keys serve the far-tile gather kernel alone
        assert plan(driver, off, "install:%d,0,0" % DISPERSED)[-1]["layout"] == 0


def test_gathering_with_the_far_tile_bitmap(driver):
    """LfReweightArgs::dispersed: a launch that gathers, of a set reported as dispersed or with lf_far_tiles = 2."""
    assert decisions(driver, ["opt:lf_patch,0"], [(0, 0)])[0]["dispersed"] == 0
    assert decisions(driver, ["opt:lf_patch,0", "opt:lf_far_tiles,2"], [(0, 0)])[0]["dispersed"] == 1
    assert decisions(driver, ["opt:lf_far_tiles,2"], [(0, 0)])[0]["dispersed"] == 0  # (the patch kernel)
    assert decisions(driver, ["install:%d,0,0" % DISPERSED, "opt:lf_patch,0"], [(0, 0)])[0]["dispersed"] == 0  # (lf_patch = 0: no reports, no verdict)


def test_a_second_decide_in_a_cycle_returns_the_first_ones_answer(driver):
    steps = plan(driver, "begin", "decide:0,0", "decide:1000,0", "consume", "begin", "decide:1000,0")
    assert steps[1]["patches"] == 1 and steps[2]["patches"] == 1 and steps[2]["useful"] == 1  # (the report waits for the next cycle)
    assert steps[5]["patches"] == 0 and steps[5]["useful"] == 0
    # a cycle that failed between decide and the reweight: the next one decides again
    steps = plan(driver, "begin", "decide:0,0", "begin")
    assert [s["decided"] for s in steps] == [0, 1, 0]


# ---- predict_key_frame --------------------------------------------------------------------------------------------------------------

KEY_FIELDS = ("ok", "cx", "cy", "c0", "s0", "inv_x", "inv_y", "inv_t", "t_off", "layout", "bits_xy")
NO_MOTION = [0] + [0.0] * 8


def key_frame(driver, cloud, motion=None, moves=1, layout=0, useful=1, resolution=0.05, extent=20.0, key_warp=1, key_bits_xy=0):
    valid, mean, sigma = (0, [0.0] * 3, [0.0] * 3) if cloud is None else (1, cloud[0], cloud[1])
    row = call(driver, "keyframe", valid, mean, sigma, 0 if motion is None else 1, NO_MOTION if motion is None else motion, moves, layout,
               useful, resolution, extent, key_warp, key_bits_xy)[0]
    return dict(zip(KEY_FIELDS, row))


def f32(x):
    return float(np.float32(x))


CLOUD = ((3.0, -2.0, 0.6), (0.3, 0.4, 0.1))


def test_key_frame_without_an_estimate_is_false_with_the_layout_set(driver):
    for layout in (0, 1, 2, 3):
        f = key_frame(driver, None, layout=layout)
        assert f["ok"] == 0 and f["layout"] == layout


def test_key_frame_of_the_set_as_it_stands(driver):
    f = key_frame(driver, CLOUD)
    assert f["ok"] == 1 and (f["cx"], f["cy"]) == (3.0, -2.0)
    assert (f["c0"], f["s0"]) == (math.cos(0.6), math.sin(0.6))
    assert (f["inv_x"], f["inv_y"], f["inv_t"], f["t_off"]) == (f32(1 / (8 * 0.3)), f32(1 / (8 * 0.4)), f32(1 / (8 * 0.1)), 0.0)
    assert f["layout"] == 4  # bins of equal mass (key_warp) over the +- 4 sigma of a heading-major key
    assert key_frame(driver, CLOUD, key_warp=0)["layout"] == 0
    assert key_frame(driver, CLOUD, layout=1)["layout"] == 1  # (not for position-major keys)
    # a set reported as dispersed: +- 2 sigma, bins of equal width; the heading bins stay at 8 sigma
    d = key_frame(driver, CLOUD, useful=0, layout=1)
    assert (d["inv_x"], d["inv_y"], d["inv_t"], d["layout"]) == (f32(1 / (4 * 0.3)), f32(1 / (4 * 0.4)), f32(1 / (8 * 0.1)), 1)
    assert key_frame(driver, CLOUD, useful=0, layout=0)["layout"] == 0
    # the heading bins never span more than the circle; a sigma of zero gives no span at all
    assert key_frame(driver, ((0, 0, 0), (0.3, 0.4, 2.0)))["inv_t"] == f32(1 / (8 * (math.pi / 4)))
    z = key_frame(driver, ((0, 0, 0), (0.0, 0.4, 0.0)))
    assert (z["ok"], z["inv_x"], z["inv_t"]) == (1, 0.0, 0.0)


def test_key_frame_a_stationary_sampler_widens_by_two_hundredths(driver):
    f = key_frame(driver, CLOUD, motion=[STATIONARY] + [0.0] * 6 + [1.0, 0.0])
    assert (f["cx"], f["cy"], f["c0"], f["s0"]) == (3.0, -2.0, math.cos(0.6), math.sin(0.6))
    want = [f32(1 / (8 * math.sqrt(s * s + 0.02 * 0.02))) for s in CLOUD[1]]
    np.testing.assert_allclose([f["inv_x"], f["inv_y"], f["inv_t"]], want, rtol=2 ** -23)  # (a float's rounding)


def _moved(cloud, m, moves):
    """The restatement: the centre moved `moves` times along its heading by the translation times the headings' mean resultant length,
    the spread widened once."""
    kind, m1, s1, mt, st_, m2, s2, fc, fs = m
    (x, y, t), (sx, sy, st) = cloud
    toward = m1 if kind == DIFFERENTIAL else math.atan2(fs, fc)
    turn = m1 + m2 if kind == DIFFERENTIAL else m1
    for _ in range(moves):
        x += mt * math.exp(-0.5 * st * st) * math.cos(t + toward)
        y += mt * math.exp(-0.5 * st * st) * math.sin(t + toward)
        t += turn
    lateral = mt * min(st, math.sqrt(0.5))
    noise2 = st_ * st_ + lateral * lateral + (s2 * s2 if kind == OMNIDIRECTIONAL else 0.0)
    return (x, y, t), (math.sqrt(sx * sx + noise2), math.sqrt(sy * sy + noise2),
                       math.sqrt(st * st + s1 * s1 + (s2 * s2 if kind == DIFFERENTIAL else 0.0)))


@pytest.mark.parametrize("kind", [DIFFERENTIAL, OMNIDIRECTIONAL])
def test_key_frame_two_moves_shift_the_centre_twice_and_widen_once(driver, kind):
    m = _sampler(kind, m1=0.1, s1=0.04, mt=0.5, st=0.03, m2=-0.05, s2=0.05, first=0.2)
    one, two = key_frame(driver, CLOUD, motion=m, moves=1), key_frame(driver, CLOUD, motion=m, moves=2)
    for f, moves in ((one, 1), (two, 2)):
        (x, y, t), (sx, sy, st) = _moved(CLOUD, m, moves)
        np.testing.assert_allclose([f["cx"], f["cy"], f["c0"], f["s0"]], [x, y, math.cos(t), math.sin(t)], rtol=1e-14)
        np.testing.assert_allclose([f["inv_x"], f["inv_y"], f["inv_t"]], [1 / (8 * sx), 1 / (8 * sy), 1 / (8 * st)], rtol=2 ** -23)
    assert (one["inv_x"], one["inv_y"], one["inv_t"]) == (two["inv_x"], two["inv_y"], two["inv_t"])
    step = (one["cx"] - 3.0, one["cy"] + 2.0)
    assert math.hypot(two["cx"] - one["cx"], two["cy"] - one["cy"]) == pytest.approx(math.hypot(*step), rel=1e-12)
    assert math.hypot(*step) == pytest.approx(0.5 * math.exp(-0.005), rel=1e-12)


@pytest.mark.parametrize("sigma", [(float("inf"), 0.4, 0.1), (0.3, float("nan"), 0.1), (0.3, 0.4, float("inf"))])
def test_key_frame_a_sigma_that_is_not_finite_gives_false(driver, sigma):
    assert key_frame(driver, ((3.0, -2.0, 0.6), sigma), layout=1)["ok"] == 0
    assert key_frame(driver, ((3.0, -2.0, 0.6), sigma), motion=_sampler())["ok"] == 0
    assert key_frame(driver, ((float("nan"), -2.0, 0.6), (0.3, 0.4, 0.1)))["ok"] == 0


def _best_bits(sx, sy, st, resolution, extent, spans=8.0):
    """The documented cost: 8 sigma_xy / res / 2^b + 8 sigma_theta reach / 2^(20 - 2 b) in cells, b = 4 .. 6, the first minimum."""
    reach = 0.5 * extent / resolution
    span_xy, span_t = spans * max(sx, sy) / resolution, 8.0 * min(st, math.pi / 4) * reach
    costs = {b: span_xy / 2 ** b + span_t / 2 ** (20 - 2 * b) for b in (4, 5, 6)}
    return min((4, 5, 6), key=lambda b: (costs[b], b)), costs


def test_key_frame_bits_follow_the_forced_option_and_otherwise_the_cost_minimum(driver):
    narrow, wide = ((0, 0, 0), (0.02, 0.02, 0.3)), ((0, 0, 0), (3.0, 2.0, 0.01))
    for cloud in (narrow, wide):
        for forced in (4, 5, 6):
            assert key_frame(driver, cloud, key_bits_xy=forced)["bits_xy"] == forced
        for other in (1, 3, 7):  # (neither a width nor "choose": the default)
            assert key_frame(driver, cloud, key_bits_xy=other)["bits_xy"] == 6
    wants = []
    for cloud in (narrow, wide):
        want, costs = _best_bits(*cloud[1], 0.05, 20.0)
        assert sorted(costs.values())[1] - sorted(costs.values())[0] > 1e-6 * max(costs.values())  # (no tie for rounding to break)
        assert key_frame(driver, cloud)["bits_xy"] == want
        wants.append(want)
    assert wants == [4, 6]  # heading bits for the narrow set with a long reach, position bits for the wide one
    # a dispersed set's +- 2 sigma enter the cost
    want, _ = _best_bits(0.6, 0.6, 0.05, 0.05, 20.0, spans=4.0)
    assert key_frame(driver, ((0, 0, 0), (0.6, 0.6, 0.05)), useful=0)["bits_xy"] == want
    # no map or a scan with a NaN: nothing to weigh
    assert key_frame(driver, narrow, resolution=0.0)["bits_xy"] == 6
    assert key_frame(driver, narrow, extent=float("nan"))["bits_xy"] == 6


# ---- policies -----------------------------------------------------------------------------------------------------------------------

def test_exponential_filter_takes_its_first_input(driver):
    """exponential_filter.hpp:32-44: an output of zero takes the input as it is."""
    assert call(driver, "filter", 0.1, 2.0, 3.0, 3.0)[0] == [2.0, 2.0 + 0.1 * (3.0 - 2.0), 2.1 + 0.1 * (3.0 - 2.1)]
    assert call(driver, "filter", 0.5, 0.0, 4.0, 0.0, 0.0, 7.0)[0] == [0.0, 4.0, 2.0, 1.0, 4.0]
    assert call(driver, "filter", 0.001, 5.0)[0] == [5.0]


def test_host_policy_reproduces_the_ess_and_the_recovery_probability(driver):
    n = 50_001
    w = np.random.Generator(np.random.MT19937(12)).gamma(0.7, 1.0, n)  # (the weights of test_normalize_and_policy_statistics)
    w, _ = orc.normalize(w)
    norm_sum, norm_sumsq = float(np.sum(w)), float(np.sum(w * w))
    alpha_slow, alpha_fast = 0.001, 0.1
    # fresh filters: both take the average, the probability is 0; not selective: every_n's verdict stands and no ESS is evaluated
    p, ess, resample, slow, fast = call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 0, 1, norm_sum, norm_sumsq, n)[0]
    assert (p, ess, resample) == (0.0, -1.0, 1) and slow == fast == norm_sum / n
    assert call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 0, 0, norm_sum, norm_sumsq, n)[0][2] == 0
    # selective: the ESS of the normalised weights against n / 2
    p, ess, resample, _, _ = call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 1, 1, norm_sum, norm_sumsq, n)[0]
    assert ess == norm_sum ** 2 / norm_sumsq
    assert ess == pytest.approx(orc.effective_sample_size(w), rel=1e-11)
    assert resample == int(ess < n / 2) == 1  # (gamma(0.7) weights: ESS = n / (1 + 1 / 0.7))
    half = call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 1, 1, 1.0, 2.0 / 10, 10)[0]
    assert half[1:3] == [5.0, 0]  # ESS = n / 2 exactly: no drop
    assert call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 1, 1, 0.0, 0.0, 10)[0][1:3] == [0.0, 1]
    assert call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 1, 0, 1.0, 0.9, 10)[0][1:3] == [-1.0, 0]  # every_n did not fire
    # the recovery estimator: 1 - fast / slow of the filtered averages, clamped (thrun_recovery_probability_estimator.hpp:69-89)
    slow0, fast0, average = 2.0e-5, 4.0e-5, norm_sum / n
    p, _, _, slow, fast = call(driver, "policy", alpha_slow, alpha_fast, slow0, fast0, 0, 1, norm_sum, norm_sumsq, n)[0]
    want_slow, want_fast = slow0 + alpha_slow * (average - slow0), fast0 + alpha_fast * (average - fast0)
    assert (slow, fast) == (want_slow, want_fast)
    assert p == max(0.0, min(1.0, 1.0 - want_fast / want_slow)) == 0.0  # the fast average is above the slow one: clamped
    p, _, _, slow, fast = call(driver, "policy", alpha_slow, alpha_fast, 4.0e-5, 3.0e-5, 0, 1, norm_sum, norm_sumsq, n)[0]
    assert p == 1.0 - fast / slow and 0.2 < p < 0.3
    assert call(driver, "policy", alpha_slow, alpha_fast, 0.0, 0.0, 0, 1, 0.0, 0.0, n)[0][0] == 0.0  # a slow average of zero: no division


def test_moved_enough_and_every_n(driver):
    latest = _pose_args((1.0, 2.0, 0.4))
    for dx, dtheta, want in ((0.2499, 0.0, 0), (0.2501, 0.0, 1), (0.0, 0.1999, 0), (0.0, 0.2001, 1), (0.0, -0.2001, 1), (0.0, 0.0, 0)):
        pose = _pose_args((1.0 + dx * math.cos(1.0), 2.0 + dx * math.sin(1.0), 0.4 + dtheta))
        assert call(driver, "moved", latest, pose, 0.25, 0.2) == [[want]]
    assert [call(driver, "everyn", c, 3)[0][0] for c in (0, 1, 2)] == [1, 2, 0]
    assert call(driver, "everyn", 0, 1) == [[0]]


# ---- shards -------------------------------------------------------------------------------------------------------------------------

WORLDS = [1, 2, 3, 4, 8]


def _sizes(world):
    return sorted({0, 1, world - 1, world, 10_007})


def bounds(driver, n, world):
    rows = call(driver, "bounds", n, world)
    return [(int(a), int(b)) for a, b in rows]


@pytest.mark.parametrize("world", WORLDS)
def test_shard_bounds_tile_the_range_in_rank_order(driver, world):
    for n in _sizes(world):
        at = 0
        counts = []
        for first, count in bounds(driver, n, world):
            assert first == at
            at += count
            counts.append(count)
        assert at == n and max(counts) - min(counts) <= 1 and counts == sorted(counts, reverse=True)


@pytest.mark.parametrize("world", WORLDS)
def test_padded_capacity_is_a_multiple_of_64_above_the_mean_share(driver, world):
    for n in _sizes(world):
        for permille in (1000, 1063, 1500):
            cap = int(call(driver, "capacity", n, world, permille)[0][0])
            assert cap % 64 == 0
            share = -(-n // world)  # the largest shard's output slots ...
            assert cap >= share / world  # ... ask one other shard for a world-th of them on average
            assert cap >= share / world * permille / 1000 + 8 * math.sqrt(share / world)
    # (every rank calls it with the same arguments: one value for all)


def _overlap(a0, a1, b0, b1):
    return max(0, min(a1, b1) - max(a0, b0))


def _blocks(n_total, world):
    """The candidate blocks of sharded_resample_kld for a set of up to n_total: doubling, from 8192 per rank (small here)."""
    pos, block, out = 0, max(3, world), []
    while pos < n_total:
        cnt = min(block, n_total - pos)
        out.append((pos, cnt))
        pos += cnt
        block *= 2
    return out


@pytest.mark.parametrize("world", WORLDS)
def test_rebalance_blocks_agree_between_every_pair_of_ranks(driver, world):
    for n in _sizes(world):
        blocks = _blocks(n, world)
        cuts = {n}
        if blocks:
            pos, cnt = blocks[-1]
            cuts |= {pos, pos + cnt // 2, max(pos + cnt - 1, 0)}  # on a block boundary, in the middle of a block, one short of its end
            if len(blocks) > 1:
                cuts |= {blocks[1][0], blocks[1][0] + 1}
        for n_out in sorted(cuts):
            new = bounds(driver, n_out, world)
            received = [0] * world
            for pos, cnt in blocks:
                if pos >= n_out:
                    break
                rows = call(driver, "block", pos, cnt, n_out, world)
                send = [[int(v) for v in row[1:1 + world]] for row in rows]
                recv = [[int(v) for v in row[1 + world:]] for row in rows]
                for r in range(world):
                    for q in range(world):
                        assert send[r][q] == recv[q][r], (world, n, n_out, pos, cnt, r, q)
                    first, count = new[r]
                    assert sum(recv[r]) == 32 * _overlap(first, first + count, pos, min(pos + cnt, n_out))
                    # what a rank receives from a block is one run of its new shard, from out0 on, behind what the blocks before it brought
                    assert int(rows[r][0]) == min(max(pos, first) - first, count)
                    if sum(recv[r]):
                        assert 32 * int(rows[r][0]) == received[r]
                    received[r] += sum(recv[r])
                    # ... and nothing is sent that the sender does not hold: its slice of the block, cut at n_out
                    slices = bounds(driver, cnt, world)
                    assert sum(send[r]) == 32 * _overlap(pos + slices[r][0], pos + slices[r][0] + slices[r][1], 0, n_out)
            assert received == [32 * count for _, count in new]


# ---- which family a sensor kind belongs to, and the grid models' small cycle ----------------------------------------------------------------
LIKELIHOOD_FIELD, BEAM, NDT, LANDMARK = 0, 1, 2, 3  # SensorFamily, in its declared order (cycle_types.h)
# MCL_SENSOR_* (include/beluga_mcl.h) -> its one family
FAMILY_OF = {0: LIKELIHOOD_FIELD, 1: BEAM, 2: LIKELIHOOD_FIELD, 3: NDT, 4: LANDMARK, 5: LANDMARK}


def test_the_sensor_kinds_of_the_header_are_the_six_of_the_table():
    """A kind added to the header is a kind to add to FAMILY_OF (and to sensor_family)."""
    header = open(os.path.join(ROOT, "include", "beluga_mcl.h")).read()
    declared = re.findall(r"\bMCL_SENSOR_(\w+) = (\d+)", header)
    assert declared == [("LIKELIHOOD_FIELD", "0"), ("BEAM", "1"), ("LIKELIHOOD_FIELD_PROB", "2"), ("NDT", "3"), ("LANDMARK", "4"), ("BEARING", "5")]
    assert sorted(FAMILY_OF) == [int(value) for _, value in declared]


@pytest.mark.parametrize("kind", sorted(FAMILY_OF))
def test_every_sensor_kind_has_its_one_family(driver, kind):
    assert call(driver, "family", kind) == [[FAMILY_OF[kind]]]


@pytest.mark.parametrize("kind", [-1, 6, 1 << 20])
def test_a_kind_outside_the_six_answers_the_likelihood_field_family(driver, kind):
    """mcl_create refuses such a kind; the function still answers, with the arm those kinds have always fallen to."""
    assert call(driver, "family", kind) == [[LIKELIHOOD_FIELD]]


@pytest.mark.parametrize("small_fused", [0, 1])
@pytest.mark.parametrize("max_live", [4096, 4097])
@pytest.mark.parametrize("n", [0, 1, 4096, 4097])
def test_grid_cycle_is_small_at_the_edges(driver, n, max_live, small_fused):
    """Restated: the option is on, and the set and the most particles a resampling may leave both fit one workgroup of k_small_tail."""
    want = int(small_fused != 0 and n <= 4096 and max_live <= 4096)
    assert call(driver, "gridsmall", small_fused, n, max_live) == [[want]]


def test_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _compile(tmp_path, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for args in ([["family", k] for k in (-1, 0, 1, 2, 3, 4, 5, 6)] + [["gridsmall", 1, 4096, 4096], ["gridsmall", 1, 4097, 4096], ["gridsmall", 0, 0, 4097]] +
                 [["bounds", 1000, 3], ["capacity", 1000000, 8, 1063], ["everyn", 3, 4]]):
        done = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert done.returncode == 0 and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr, (args, done.stderr)
