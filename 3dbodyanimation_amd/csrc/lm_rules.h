// lm_rules.h — the trust-region rule of Ceres' Levenberg-Marquardt loop (1.14 defaults), stated ONCE for the host loop
// (host_solver.cpp) and the device solvers (k_lm_batched.hip, window_lm_inl.h): they are tested to agree iterate by iterate,
// which holds only while every one of them evaluates these expressions, in this association.  Plain C++17, host and device.
// (oracle/lm_dense.py states the same rule independently; tests/cpp/lm_rules_test.cpp checks this header against it.)
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define LM_RULE_FN __host__ __device__ inline
#else
#define LM_RULE_FN inline
#endif

namespace bodyfit {

constexpr double kLmInitialRadius = 1e4;        // initial_trust_region_radius
constexpr double kLmMaxRadius = 1e16;           // max_trust_region_radius
constexpr double kLmMinRadius = 1e-32;          // min_trust_region_radius
constexpr double kLmInitialDecrease = 2.0;      // the radius is divided by this after a rejected step, and it doubles
constexpr double kLmMinRelativeDecrease = 1e-3; // min_relative_decrease: a step is taken when rho exceeds it
constexpr double kLmMaxShrink = 1.0 / 3.0;      // an accepted step grows the radius by at most 3
constexpr double kLmFunctionTolerance = 1e-6;
constexpr double kLmGradientTolerance = 1e-10;
constexpr double kLmParameterTolerance = 1e-8;
constexpr double kLmCostLimit = 1e300;          // a cost at or above it counts as not finite

// The one finite-cost predicate: the initial cost of a solve (not finite: failure before the first iteration) and the cost at
// every candidate (not finite: rejected).  (A cost is a sum of squares and Huber terms, never negative, so `finite` is written
// as "not NaN and below the limit": -inf, the one input std::isfinite would treat differently, cannot occur.)
LM_RULE_FN bool lm_cost_finite(double cost) { return (cost == cost) && cost < kLmCostLimit; }
// rho = (cost - new_cost) / model_change
LM_RULE_FN bool lm_step_accepted(double new_cost, double model_change, double rho) {
  return lm_cost_finite(new_cost) && model_change > 0.0 && rho > kLmMinRelativeDecrease;
}
LM_RULE_FN double lm_radius_after_accept(double radius, double rho) {
  const double t = 2.0 * rho - 1.0;
  return fmin(kLmMaxRadius, radius / fmax(kLmMaxShrink, 1.0 - t * t * t));
}
// a rejected step or a failed factorisation: shrink the radius, then double the factor of the next shrink
LM_RULE_FN void lm_reject(double& radius, double& decrease) {
  radius = radius / decrease;
  decrease = decrease * 2.0;
}
LM_RULE_FN bool lm_radius_collapsed(double radius) { return radius < kLmMinRadius; }
LM_RULE_FN bool lm_function_tolerance(double change, double old_cost) { return fabs(change) < kLmFunctionTolerance * old_cost; }
LM_RULE_FN bool lm_gradient_tolerance(double gmax) { return gmax <= kLmGradientTolerance; }
// norms, not squares: |step| and |x|
LM_RULE_FN bool lm_parameter_tolerance(double dnorm, double xnorm) {
  return dnorm <= kLmParameterTolerance * (xnorm + kLmParameterTolerance);
}

}  // namespace bodyfit
