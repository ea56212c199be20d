// lm_rules_test.cpp — csrc/lm_rules.h against the rule as oracle/lm_dense.py states it: every function on a fixed table of inputs,
// results compared bit for bit with values computed from that statement in Python (never by calling the header).  No GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../3dbodyanimation_amd/csrc/lm_rules.h"

using namespace bodyfit;

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)
static uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(kLmInitialRadius == 1e4 && kLmInitialDecrease == 2.0 && kLmMaxRadius == 1e16 && kLmMinRadius == 1e-32);
  // accept test: finite cost, positive model change, rho above 1e-3 (strictly)
  CHECK(lm_step_accepted(1.0, 1.0, 0.0010000000000000002));      // just above 1e-3
  CHECK(!lm_step_accepted(1.0, 1.0, 1e-3));
  CHECK(!lm_step_accepted(1.0, 1.0, 0.0009999999999999998));     // just below
  CHECK(lm_step_accepted(0.0, 1e-300, 0.5));
  CHECK(!lm_step_accepted(nan, 1.0, 0.5));
  CHECK(!lm_step_accepted(1e300, 1.0, 0.5));
  CHECK(lm_step_accepted(9.999999999999999e+299, 1.0, 0.5));        // the largest cost below 1e300
  CHECK(!lm_step_accepted(inf, 1.0, 0.5));
  CHECK(!lm_step_accepted(1.0, 0.0, 0.5));
  CHECK(!lm_step_accepted(1.0, -1.0, 0.5));
  CHECK(!lm_step_accepted(1.0, 1.0, nan));
  // the finite-cost predicate (initial cost and candidates alike): not NaN and strictly below 1e300
  CHECK(!lm_cost_finite(nan) && !lm_cost_finite(inf) && !lm_cost_finite(1e300));
  CHECK(lm_cost_finite(9.999999999999999e+299) && !lm_cost_finite(1.0000000000000002e+300));   // the neighbours of 1e300
  CHECK(std::nextafter(1e300, 0.0) == 9.999999999999999e+299 && std::nextafter(1e300, inf) == 1.0000000000000002e+300);
  CHECK(lm_cost_finite(0.0) && lm_cost_finite(1.0) && !lm_cost_finite(std::numeric_limits<double>::max()));
  // radius after an accepted step: rho = 0.5 leaves it, rho = 1 triples it, the cap at 1e16 holds
  struct { double radius, rho; uint64_t want; } const acc[] = {
    {10000.0, 0.5, 0x40c3880000000000ull},
    {10000.0, 1.0, 0x40dd4c0000000000ull},
    {10000.0, 0.75, 0x40c6524924924925ull},
    {10000.0, 0.0011, 0x40b39884a349a064ull},
    {1e+16, 1.0, 0x4341c37937e08000ull},
    {5000000000000000.0, 1.0, 0x4341c37937e08000ull},
    {1e+16, 0.5, 0x4341c37937e08000ull},
    {123.456, 0.9, 0x406f9f79b475821cull},
    {10000.0, 0.25, 0x40c15c71c71c71c7ull},
    {10000.0, 1.7, 0x40dd4c0000000000ull}};
  for (const auto& c : acc) CHECK(bits(lm_radius_after_accept(c.radius, c.rho)) == c.want);
  CHECK(lm_radius_after_accept(1e4, 0.5) == 1e4);
  CHECK(lm_radius_after_accept(1e4, 1.0) == 1e4 / (1.0 / 3.0));
  CHECK(lm_radius_after_accept(1e16, 1.0) == 1e16 && lm_radius_after_accept(5e15, 1.0) == 1e16);
  // repeated rejection from the start radius: divide, then double.  After k rejections the radius is 1e4 / 2^(k (k + 1) / 2):
  // 2.5e-28 at k = 14 (2^105), 7.5e-33 at k = 15 (2^120) — below 1e-32 first at the 15th
  const uint64_t rej[] = {
    0x40b3880000000000ull,
    0x4093880000000000ull,
    0x4063880000000000ull,
    0x4023880000000000ull,
    0x3fd3880000000000ull,
    0x3f73880000000000ull,
    0x3f03880000000000ull,
    0x3e83880000000000ull,
    0x3df3880000000000ull,
    0x3d53880000000000ull,
    0x3ca3880000000000ull,
    0x3be3880000000000ull,
    0x3b13880000000000ull,
    0x3a33880000000000ull,
    0x3943880000000000ull,
    0x3843880000000000ull,
    0x3733880000000000ull,
    0x3613880000000000ull};
  double radius = kLmInitialRadius, dec = kLmInitialDecrease;
  int first = 0;
  for (int k = 1; k <= 18; ++k) {
    lm_reject(radius, dec);
    CHECK(bits(radius) == rej[k - 1]);
    CHECK(dec == std::ldexp(1.0, k + 1));
    if (!first && lm_radius_collapsed(radius)) first = k;
  }
  CHECK(first == 15);
  CHECK(!lm_radius_collapsed(1e-32) && lm_radius_collapsed(9.999999999999999e-33) && !lm_radius_collapsed(1.0000000000000002e-32));
  // tolerances at their boundaries: function < (strict), gradient <=, parameter <=
  CHECK(!lm_function_tolerance(1e-6 * 8.0, 8.0) && lm_function_tolerance(7.999999999999998e-06, 8.0) && lm_function_tolerance(-7.999999999999998e-06, 8.0));
  CHECK(!lm_function_tolerance(0.0, 0.0));
  CHECK(lm_gradient_tolerance(1e-10) && lm_gradient_tolerance(0.0) && !lm_gradient_tolerance(1.0000000000000002e-10));
  CHECK(lm_parameter_tolerance(2.00000001e-08, 2.0) && !lm_parameter_tolerance(2.0000000100000002e-08, 2.0));
  CHECK(lm_parameter_tolerance(0.0, 0.0) && lm_parameter_tolerance(1e-16, 0.0) && !lm_parameter_tolerance(1.0000000000000002e-16, 0.0));
  if (g_bad) return 1;
  std::printf("lm_rules_test ok\n");
  return 0;
}
