// scan_host_check.cpp — the rule about which points of a scan are staged (mcl::scan_finite_points, beluga_amd/csrc/scan_host.cpp) as a
// stand-alone program, for a CPU build under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeluga_amd/csrc
//       tests/cpp/scan_host_check.cpp beluga_amd/csrc/scan_host.cpp -o scan_host_check && ./scan_host_check
// Every buffer is a heap vector of exactly the size the function may touch, so that a read or a write past it is seen; exits 0 and
// prints "scan_host_check OK" if every expectation holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "scan_host.h"

#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

using mcl::scan_finite_points;

// The function on `points`, with and without the index list, against the rule written out here.
static void check(const std::vector<double>& points) {
  const uint64_t n = points.size() / 2;
  std::vector<double> want;
  std::vector<uint32_t> want_slots;
  for (uint64_t i = 0; i < n; ++i) {
    if (!std::isfinite(points[2 * i]) || !std::isfinite(points[2 * i + 1])) continue;
    want.push_back(points[2 * i]);
    want.push_back(points[2 * i + 1]);
    want_slots.push_back(static_cast<uint32_t>(i));
  }
  for (const bool with_slots : {true, false}) {
    std::vector<double> kept(2 * n, -7.0);
    std::vector<uint32_t> slots(with_slots ? n : 0, 0xFFFFFFFFu);
    const uint64_t count = scan_finite_points(n ? points.data() : nullptr, n, kept.data(), with_slots ? slots.data() : nullptr);
    EXPECT(count == want_slots.size());
    EXPECT(count == 0 || std::memcmp(kept.data(), want.data(), 2 * count * sizeof(double)) == 0);  // bit for bit
    for (uint64_t i = 2 * count; i < 2 * n; ++i) EXPECT(kept[i] == -7.0);                            // nothing behind the kept points
    for (uint64_t k = 0; k < slots.size(); ++k) EXPECT(slots[k] == (k < count ? want_slots[k] : 0xFFFFFFFFu));
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (const uint64_t n : {0ull, 1ull, 2ull, 7ull, 64ull}) {
    std::vector<double> clean(2 * n);
    for (uint64_t i = 0; i < 2 * n; ++i) clean[i] = 0.25 * static_cast<double>(i) - 3.0;
    if (n) clean[0] = -0.0, clean[1] = std::numeric_limits<double>::denorm_min();
    check(clean);  // nothing to take out
    if (n == 0) continue;
    for (const double bad : {nan, inf, -inf})
      for (const int column : {0, 1}) {
        for (const uint64_t row : {uint64_t{0}, n / 2, n - 1}) {  // the first point, one in the middle, the last
          std::vector<double> p = clean;
          p[2 * row + column] = bad;
          check(p);
        }
        std::vector<double> every = clean, alternate = clean;
        for (uint64_t i = 0; i < n; ++i) every[2 * i + column] = bad;
        for (uint64_t i = 0; i < n; i += 2) alternate[2 * i + column] = bad;
        check(every);
        check(alternate);
      }
    std::vector<double> big = clean;  // finite, the sum |x| + |y| overflows: the point stays
    big[2 * (n / 2)] = big[2 * (n / 2) + 1] = 1e308;
    check(big);
    std::vector<double> kept(2 * n);
    EXPECT(scan_finite_points(big.data(), n, kept.data()) == n);
    EXPECT(std::memcmp(kept.data(), big.data(), 2 * n * sizeof(double)) == 0);
    EXPECT(std::isinf(std::abs(kept[2 * (n / 2)]) + std::abs(kept[2 * (n / 2) + 1])));
  }
  std::puts("scan_host_check OK");
  return 0;
}
