// window_lm_inl.h — what the three units of the device window LM share (k_window_lm.hip, k_window_cr.hip,
// k_window_shard.hip; private to them): the block geometry, the batched copy, and the two decisions of an iteration, which the
// single-GPU kernels (k_win_finish, k_win_tail, k_win_accept) and the sharded solve's k_win_decide both run.
#pragma once
#include "bodyfit_device.h"
#include "device_util_inl.h"
#include "lm_rules.h"

namespace bodyfit {
namespace {

constexpr int NP = kFrameParams;     // 76
constexpr int NBETA = kMaxShape;     // 10
constexpr int WB = kWinBlock;        // 80
constexpr int WR = kWinRhs;          // 16
constexpr int LD = WB + 1;           // LDS leading dimension

// dst[i] = src[i], i in [0, n): eight loads in flight per thread and pass (a load-store loop is one dependent round trip per trip)
__device__ __forceinline__ void copy_batched(double* __restrict__ dst, const double* __restrict__ src, int n, int tid, int nthreads) {
  int i = tid;
  for (; i + 7 * nthreads < n; i += 8 * nthreads) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[i + u * nthreads];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[i + u * nthreads] = v[u];
  }
  for (; i < n; i += nthreads) dst[i] = src[i];
}

// ---- decide: gradient tolerance, failed factorisation, parameter tolerance, or a candidate --------------------------------
// mode 0: all; 1: this shard's sums -> W.fin[0..3] = {model, |d|^2, |x|^2, max |g_frames|}, W.fin[4] = fail flag, only;
// 2: decide from W.fin (the first three summed, the last two maximised over the shards)
// the decision of an iteration from the sums over the frames (256 threads): gradient tolerance, failed factorisation,
// parameter tolerance, or a candidate
__device__ __forceinline__ void finish_core(const WinProblem& P, const WinBuf& W, const double* __restrict__ x,
                                            const double* __restrict__ beta, double* __restrict__ x_new,
                                            double* __restrict__ beta_new, double pm, double dn, double xn, double gm, int tid) {
  const int F = P.F;
  if (tid == 0) gm = fmax(gm, W.gmaxp[F]);
  // the beta block's operands into LDS first (one round trip; thread 0 walking global memory made this an 11 us kernel)
  __shared__ double sCr[NBETA * NBETA], sdb2[NBETA], sgb[NBETA], sbt[NBETA];
  if (tid < NBETA * NBETA) sCr[tid] = W.Craw[tid];
  if (tid >= 128 && tid < 128 + NBETA) {
    const int a = tid - 128;
    sdb2[a] = (a < P.nb) ? W.d[(size_t)F * NP + a] : 0.0;
    sgb[a] = W.gbraw[a];
    sbt[a] = (a < P.nb) ? beta[a] : 0.0;
  }
  __syncthreads();
  __shared__ int no_cand;
  if (tid == 0) {
    double* st = W.status;
    for (int a = 0; a < P.nb; ++a) {
      const double da = sdb2[a];
      pm -= da * sgb[a];
      double h = 0.0;
      for (int c = 0; c < P.nb; ++c) h += sCr[a * NBETA + c] * sdb2[c];
      pm -= 0.5 * da * h;
      dn += da * da;
      xn += sbt[a] * sbt[a];
    }
    st[kWsGmax] = gm;
    st[kWsHasCand] = 0.0;
    no_cand = 1;
    if (st[kWsActive] != 0.0) {
      if (lm_gradient_tolerance(gm)) {
        st[kWsActive] = 0.0; st[kWsTermination] = 0.0;
      } else if (*W.fail) {                                // the damped system was not positive definite
        double rad = st[kWsRadius], dec = st[kWsDec];
        lm_reject(rad, dec);
        st[kWsRadius] = rad; st[kWsDec] = dec; st[kWsBad] += 1.0; st[kWsIters] += 1.0;
        st[kWsAccepted] = 0.0;
        if (lm_radius_collapsed(rad)) { st[kWsActive] = 0.0; st[kWsTermination] = 2.0; }
      } else if (lm_parameter_tolerance(sqrt(dn), sqrt(xn))) {
        st[kWsActive] = 0.0; st[kWsTermination] = 0.0;
      } else {
        st[kWsModel] = pm; st[kWsHasCand] = 1.0;
        no_cand = 0;
      }
    }
  }
  __syncthreads();
  if (no_cand) {   // the residual sweep that follows still reads a well-defined point
    copy_batched(x_new, x, F * NP, tid, 256);
    if (tid < P.nb) beta_new[tid] = beta[tid];
  }
}

// ---- accept / reject the candidate (Ceres' step quality and radius rules, host_solver.cpp) ------------------------------
// the decision itself, for a candidate that exists (status HasCand), given the candidate's cost; thread 0 decides, every
// thread then copies the accepted point.  Returns (to every thread) whether the candidate was accepted.
__device__ __forceinline__ bool accept_core(const WinProblem& P, const WinBuf& W, double* __restrict__ x, double* __restrict__ beta,
                                            const double* __restrict__ x_new, const double* __restrict__ beta_new, double new_cost,
                                            int tid, int nthreads) {
  __shared__ int acc_flag;
  double* st = W.status;
  if (tid == 0) {
    const double cost = st[kWsCost], model = st[kWsModel];
    const double change = cost - new_cost, rho = change / model;
    const bool accept = lm_step_accepted(new_cost, model, rho);
    st[kWsIters] += 1.0;
    st[kWsNewCost] = new_cost;
    if (accept) {
      st[kWsCost] = new_cost;
      st[kWsRadius] = lm_radius_after_accept(st[kWsRadius], rho);
      st[kWsDec] = kLmInitialDecrease;
      st[kWsOk] += 1.0;
      if (lm_function_tolerance(change, cost)) { st[kWsActive] = 0.0; st[kWsTermination] = 0.0; }
    } else {
      double rad = st[kWsRadius], dec = st[kWsDec];
      lm_reject(rad, dec);
      st[kWsRadius] = rad; st[kWsDec] = dec; st[kWsBad] += 1.0;
      if (lm_radius_collapsed(rad)) { st[kWsActive] = 0.0; st[kWsTermination] = 2.0; }
    }
    st[kWsAccepted] = accept ? 1.0 : 0.0;
    st[kWsJsel] = accept ? 1.0 : 2.0;     // (single-GPU loop: the candidate sweep also left the candidate's Jacobian)
    st[kWsHasCand] = 0.0;
    acc_flag = accept ? 1 : 0;
  }
  __syncthreads();
  if (acc_flag) {
    copy_batched(x, x_new, P.F * NP, tid, nthreads);
    if (tid < P.nb) beta[tid] = beta_new[tid];
  }
  return acc_flag != 0;
}

}  // namespace
}  // namespace bodyfit
