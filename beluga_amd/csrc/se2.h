// se2.h — SO(2)/SE(2) arithmetic shared by host and device code.
//
// The reference stores particle states as Sophus::SE2d (unit complex + translation); the filter's
// results depend on Sophus 1.22.10's exact operation order (products renormalise, constructors
// normalise with hypot).  These functions reproduce that order so that host-side policy code and
// the device kernels agree with the reference to rounding.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (a host-only source that hipcc compiles as HIP includes nothing else of it)
#define MCL_HD __host__ __device__ __forceinline__
#else
#define MCL_HD inline
#endif

namespace mcl {

constexpr double kPi = 3.14159265358979323846264338327950288;

struct Rot2 {
  double c, s;
};
struct Pose2 {
  Rot2 r;
  double x, y;
};

// hypot for the device (pose_mul_ieee below), bit for bit the host library's on normal-range arguments: a square root corrected by its own rounding error
// (C. F. Borges, "An Improved Algorithm for hypot(a, b)", 2019, the variant without fused operations - the one the reference's host
// library evaluates), in IEEE operations alone, each rounded on its own.  The device library's hypot is accurate to an ulp but not the
// same function: one pose in a few had a world -> field rotation one ulp off the reference's, which moves every end-point of that pose by
// an ulp and with it the cell of any end-point that close to a cell boundary (tests/test_gpu_lf_edges.py, family ulp_straddle).
// Held to std::hypot by tests/test_lf_reference_cpu.py.  "The host library" is the C library the oracle and numpy run on (glibc 2.35 and
// later evaluate exactly this sequence); on a host whose hypot is another function that test fails and says so - the kernels then
// agree with THIS sequence, and the oracle and tests/lf_reference.py would have to normalise with it too to stay the yardstick.
MCL_HD double hypot_ieee(double x, double y) {
  double ax = fabs(x), ay = fabs(y);
  if (ax < ay) {
    const double t = ax;
    ax = ay;
    ay = t;
  }
  if (!(ax < 0x1p+500 && ay > 0x1p-500)) return hypot(x, y);  // zeros, infinities, NaN, scales a rotation never has
  if (ay <= ax * 0x1p-54) return ax + ay;
  const double h = sqrt(ax * ax + ay * ay);
  double t1, t2;
  if (h <= 2.0 * ay) {
    const double d = h - ay;
    t1 = ax * (2.0 * d - ax);
    t2 = (d - 2.0 * (ax - ay)) * d;
  } else {
    const double d = h - ax;
    t1 = 2.0 * d * (ax - 2.0 * ay);
    t2 = (4.0 * d - ay) * ay + d * d;
  }
  return h - (t1 + t2) / (2.0 * h);
}

// SO2(real, imag): store then normalize() (hypot).
MCL_HD Rot2 rot_from_complex(double re, double im) {
  const double len = hypot(re, im);
  return Rot2{re / len, im / len};
}
MCL_HD Rot2 rot_exp(double theta) { return rot_from_complex(cos(theta), sin(theta)); }
MCL_HD double rot_log(const Rot2& r) { return atan2(r.s, r.c); }
MCL_HD Rot2 rot_inverse(const Rot2& r) { return rot_from_complex(r.c, -r.s); }
// SO2 * SO2: complex product, first-order renormalisation if |z|^2 != 1, then the ctor's normalize().
MCL_HD Rot2 rot_mul(const Rot2& a, const Rot2& b) {
  double re = a.c * b.c - a.s * b.s;
  double im = a.c * b.s + a.s * b.c;
  const double n2 = re * re + im * im;
  if (n2 != 1.0) {
    const double scale = 2.0 / (1.0 + n2);
    re = re * scale;
    im = im * scale;
  }
  return rot_from_complex(re, im);
}
MCL_HD void rot_apply(const Rot2& r, double px, double py, double& ox, double& oy) {
  ox = r.c * px - r.s * py;
  oy = r.s * px + r.c * py;
}
MCL_HD Pose2 pose_mul(const Pose2& a, const Pose2& b) {
  Pose2 o;
  o.r = rot_mul(a.r, b.r);
  double tx, ty;
  rot_apply(a.r, b.x, b.y, tx, ty);
  o.x = a.x + tx;
  o.y = a.y + ty;
  return o;
}
// pose_mul with the rotation normalised by hypot_ieee: on the device the same bits as the host's pose_mul.  For the ONE product whose last
// bit decides a map cell - world -> field times the particle's pose, which the likelihood-field kernels start from.  Formed once per
// set of poses, where a pose is written (the propagation kernels, or k_field_pose for a set that something else wrote) and kept in a
// buffer the LF kernels load (option lf_pose_ahead; with 0 each LF kernel forms it, once per particle and launch): a complex product, a
// renormalisation, a square root and a division behind two branches and two more divisions are too much for the prologue of a kernel at
// its register cap.  Every other rotation on the device keeps the device library's hypot (an ulp is within every other stage's
// tolerance).
MCL_HD Pose2 pose_mul_ieee(const Pose2& a, const Pose2& b) {
  double re = a.r.c * b.r.c - a.r.s * b.r.s;
  double im = a.r.c * b.r.s + a.r.s * b.r.c;
  const double n2 = re * re + im * im;
  if (n2 != 1.0) {
    const double scale = 2.0 / (1.0 + n2);
    re = re * scale;
    im = im * scale;
  }
  const double len = hypot_ieee(re, im);
  Pose2 o;
  o.r = Rot2{re / len, im / len};
  double tx, ty;
  rot_apply(a.r, b.x, b.y, tx, ty);
  o.x = a.x + tx;
  o.y = a.y + ty;
  return o;
}
MCL_HD Pose2 pose_inverse(const Pose2& a) {
  Pose2 o;
  o.r = rot_inverse(a.r);
  rot_apply(o.r, a.x * -1.0, a.y * -1.0, o.x, o.y);
  return o;
}
MCL_HD Pose2 pose_identity() { return Pose2{Rot2{1.0, 0.0}, 0.0, 0.0}; }

}  // namespace mcl
