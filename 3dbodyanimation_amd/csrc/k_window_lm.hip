// k_window_lm.hip — device-resident Levenberg-Marquardt for ONE problem over all frames of a window with a shared shape
// block: what OptimizeMultiFrame hands to ceres::Solve with DENSE_QR (include/MultiFrameBA.h:144-151).
//
// The normal equations of such a window are block tridiagonal in the frames (76 x 76 blocks, coupled by the temporal
// term: diagonal off-diagonal blocks) with a 10-wide border (beta).  host_solver.cpp factors the chain frame after frame
// on the host; here it is solved on the device, parallel in the frames, by BLOCK CYCLIC REDUCTION with the border carried
// as 11 right-hand sides [B | rhs]:
//   level l: every second remaining frame j (neighbours a < j < b) is eliminated (the larger independent set when the count
//   is odd: api_solve.hip build_cr_schedule):
//       D_j = L L^T,  P = L^-1 U_a^T,  Q = L^-1 U_j,  Y = L^-1 R_j                         (k_cr_factor, two workgroups per j)
//       D_a -= P^T P,  D_b -= Q^T Q,  U_a := -P^T Q,  R_a -= P^T Y,  R_b -= Q^T Y          (k_cr_update, f64 MFMA)
//   after ceil(log2 F) levels one frame is left: x = D^-1 R; then down again: x_j = L^-T (Y - P x_a - Q x_b)  (k_cr_back)
//   beta:  S = C - B^T X_B,  d_beta = S^-1 (rhs_b - B^T x),  d_f = x_f - X_B,f d_beta     (k_win_schur*, k_win_beta_solve)
// (U_j: coupling block (j, next remaining frame); at level 0 it is the diagonal temporal block, afterwards dense.)
// Around it, all of Ceres' trust-region logic as restated in host_solver.cpp (Jacobi scaling fixed at the first iterate,
// LM damping, projected scale bounds, step quality, radius update, the three termination tests) runs in small kernels on
// the device: per LM iteration the host launches a fixed sequence and reads back one 16-double status record (every fourth
// iteration on one GPU).  Single-GPU windows of up to 256 frames end an iteration with ONE launch for step, model change and
// decision (k_win_tail: the last workgroup, found by a ticket, decides).
// Every block that moves between global memory and LDS does so with all its loads issued before the first is used
// (BlockRegs): written as load-store loops these kernels spent a third of their time in dependent L2 round trips.
// Blocks are padded to 80 x 80 (identity on the padding), right-hand sides to 16 rows, all stored row-major; "t" buffers
// hold transposes (Pt[i][k] = P[k][i]) so that every product is  C[i][i'] = sum_k X[i][k] Y[i'][k]  with k contiguous.
// This unit: the cost functions and the kernels around the linear solve.  The cyclic reduction itself is k_window_cr.hip, the
// exchange steps of sharded solves k_window_shard.hip; window_lm_inl.h holds what the three share.
#include "dense_inl.h"
#include "window_lm_inl.h"

namespace bodyfit {
namespace {

constexpr int kHLd = kNormalLd, kHRows = kNormalRows;   // k_frame_normal panels: 87 x 88, n = 86

// ---- cost of a residual vector: 1/2 sum rho(|r_kp|^2) over the keypoints + 1/2 |other rows|^2 -----------------------
__device__ double window_cost(const WinProblem& P, const double* __restrict__ r, double* red, int tid, int nthreads) {
  // independent partial sums per thread, sixteen loads in flight per pass (a 1024-frame window has 170 rows per thread: one
  // dependent load per pass made this the second longest kernel of an iteration, four in flight still left it at 39 us)
  auto rho = [&](double s) { double rho1; return huber_rho(P.huber, s, &rho1); };   // (the derivative is not needed here)
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int k = tid;
  for (; k + 7 * nthreads < P.K; k += 8 * nthreads) {
    double xx[8], yy[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { xx[u] = r[2 * (size_t)(k + u * nthreads)]; yy[u] = r[2 * (size_t)(k + u * nthreads) + 1]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; u += 4) {
      a0 += 0.5 * rho(xx[u] * xx[u] + yy[u] * yy[u]);
      a1 += 0.5 * rho(xx[u + 1] * xx[u + 1] + yy[u + 1] * yy[u + 1]);
      a2 += 0.5 * rho(xx[u + 2] * xx[u + 2] + yy[u + 2] * yy[u + 2]);
      a3 += 0.5 * rho(xx[u + 3] * xx[u + 3] + yy[u + 3] * yy[u + 3]);
    }
  }
  for (; k < P.K; k += nthreads) {
    const double r0 = r[2 * (size_t)k], r1 = r[2 * (size_t)k + 1];
    a0 += 0.5 * rho(r0 * r0 + r1 * r1);
  }
  int i = 2 * P.K + tid;
  for (; i + 15 * nthreads < P.total_rows; i += 16 * nthreads) {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = r[i + u * nthreads];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 16; u += 4) { a0 += 0.5 * v[u] * v[u]; a1 += 0.5 * v[u + 1] * v[u + 1]; a2 += 0.5 * v[u + 2] * v[u + 2]; a3 += 0.5 * v[u + 3] * v[u + 3]; }
  }
  for (; i < P.total_rows; i += nthreads) a0 += 0.5 * r[i] * r[i];
  const double acc = (a0 + a1) + (a2 + a3);
  return block_sum_n(acc, red, tid, nthreads / 64);
}

// The same cost from the partials the Jacobian sweep at that point left (P.cost_partials): F + tiles values instead of every
// residual row — at 1,024 frames the walk over the residual vector was 45 us of a 0.9 ms iteration, one workgroup reading 1.6 MB.
__device__ double window_cost_any(const WinProblem& P, const double* __restrict__ r, double* red, int tid, int nthreads) {
  if (!P.cost_partials) return window_cost(P, r, red, tid, nthreads);
  double a = 0.0;
  const int n = P.F + P.cost_tiles;
  for (int i = tid; i < n; i += nthreads) a += P.cost_partials[(size_t)i * kReducePartial + (i < P.F ? fold_slot_cost(0) : fold_slot_cost(1))];
  return block_sum_n(a, red, tid, nthreads / 64);
}

// mode 0: all; 1: this shard's cost -> W.fin[0] only; 2: initialise the status from W.fin[0] (summed over the shards)
__global__ __launch_bounds__(1024) void k_win_init(WinProblem P, WinBuf W, const double* __restrict__ r, int mode) {
  __shared__ double red[16];
  double c = 0.0;
  if (mode != 2) c = window_cost_any(P, r, red, threadIdx.x, 1024);
  if (mode == 1) { if (threadIdx.x == 0) W.fin[0] = c; return; }
  if (mode == 2) c = W.fin[0];
  if (threadIdx.x == 0) {
    double* st = W.status;
    st[kWsCost] = c; st[kWsInitialCost] = c; st[kWsRadius] = kLmInitialRadius; st[kWsDec] = kLmInitialDecrease; st[kWsModel] = 0.0;
    st[kWsHasCand] = 0.0; st[kWsIters] = 0.0; st[kWsOk] = 0.0; st[kWsBad] = 0.0;
    const bool finite = lm_cost_finite(c);
    st[kWsActive] = finite ? 1.0 : 0.0;
    st[kWsTermination] = finite ? 1.0 : 2.0;
    st[kWsAccepted] = 1.0; st[kWsGmax] = 0.0; st[kWsNewCost] = c; st[kWsJsel] = 0.0;
    st[kWsPoison] = 0.0;   // (the record lives in the problem's pool: a poisoned solve must not poison the next one)
    *W.fail = 0;
  }
}

// ---- beta block: C = sum_f C_f (+ shape prior), g_beta; scaling; damped scaled copy ------------------------------------
// mode 0: all; 1: this shard's sums -> W.Craw, W.gbraw only; 2: scaling and the damped copy from W.Craw, W.gbraw (summed
// over the shards by the caller)
__global__ __launch_bounds__(1024) void k_win_beta(WinProblem P, WinBuf W, const double* __restrict__ Hpan,
                                                   const double* __restrict__ r, int first, int mode) {
  __shared__ double sC[NBETA * NBETA], sg[NBETA], ssc[NBETA];
  __shared__ double part[8][128];
  const int tid = threadIdx.x, F = P.F;
  if (tid == 0 && mode != 2) *W.fail = 0;
  if (P.nb == 0) return;
  if (mode == 2) {
    if (tid < NBETA * NBETA) sC[tid] = W.Craw[tid];
    if (tid < NBETA) sg[tid] = W.gbraw[tid];
  } else {
    // C = sum_f H_f[beta, beta], g_beta = sum_f H_f[rhs row, beta]: 110 words, eight frame lanes of 128 threads, four
    // independent loads per pass
    const int w = tid & 127, g = tid >> 7;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (w < NBETA * NBETA + NBETA) {
      size_t off;
      if (w < NBETA * NBETA) {
        const int a = w / NBETA, b = w % NBETA, lo = a > b ? a : b, hi = a > b ? b : a;
        off = (size_t)(NP + lo) * kHLd + NP + hi;
      } else {
        off = (size_t)(NP + NBETA) * kHLd + NP + (w - NBETA * NBETA);
      }
      const size_t fs = (size_t)kHRows * kHLd;
      int f = g;
      for (; f + 120 < F; f += 128) {        // sixteen loads in flight
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = Hpan[(size_t)(f + 8 * u) * fs + off];
        __builtin_amdgcn_sched_barrier(0);     // (without it the scheduler pairs every load with its add again)
#pragma unroll
        for (int u = 0; u < 16; u += 4) { a0 += v[u]; a1 += v[u + 1]; a2 += v[u + 2]; a3 += v[u + 3]; }
      }
      for (; f < F; f += 8) a0 += Hpan[(size_t)f * fs + off];
    }
    part[g][w] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (tid < NBETA * NBETA + NBETA) {
      const double v = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) +
                       ((part[4][tid] + part[5][tid]) + (part[6][tid] + part[7][tid]));
      if (tid < NBETA * NBETA) sC[tid] = v; else sg[tid - NBETA * NBETA] = v;
    }
  }
  __syncthreads();
  if (mode != 2 && tid < NBETA && P.shape_rows > 0) {   // ShapePriorL2Analytic: r = beta_s w, J = beta_s I (include/Sim3BA.h:336-340)
    sC[tid * NBETA + tid] += P.beta_shape * P.beta_shape;
    sg[tid] += P.beta_shape * r[P.row_shape + tid];
  }
  __syncthreads();
  if (mode == 1) {
    if (tid < NBETA * NBETA) W.Craw[tid] = sC[tid];
    if (tid < NBETA) W.gbraw[tid] = sg[tid];
    return;
  }
  if (tid < NBETA) {
    const double s = first ? 1.0 / (1.0 + sqrt(sC[tid * NBETA + tid])) : W.scale[(size_t)F * NP + tid];
    if (first) W.scale[(size_t)F * NP + tid] = s;
    ssc[tid] = s;
    W.gbraw[tid] = sg[tid];
    W.rhsb[tid] = -sg[tid] * s;
    W.gmaxp[F] = 0.0;
  }
  __syncthreads();
  if (tid < NBETA * NBETA) {
    const int a = tid / NBETA, b = tid % NBETA;
    W.Craw[tid] = sC[tid];
    double v = sC[tid] * ssc[a] * ssc[b];
    if (a == b) v += fmin(fmax(v, 1e-6), 1e32) / W.status[kWsRadius];
    W.Cs[tid] = v;
  }
  if (tid == 0) {
    double gm = 0.0;
    for (int b = 0; b < NBETA; ++b) gm = fmax(gm, fabs(sg[b]));
    W.gmaxp[F] = gm;
  }
}

// ---- per frame: complete the normal-equation block (priors, temporal), scale, damp, write the CR operands ---------------
// Shards of a window (bodyfit_solve_sharded): x_left = parameters of the frame in front of the shard's first one (null: none),
// P.halo: a temporal pair leaves the shard behind its last frame (its residual rows are this shard's), scale_halo = Jacobi
// scaling of that next frame (null on the first pass of the first iteration, which only produces this shard's scaling).
constexpr int kAsmThreads = 1024;
__global__ __launch_bounds__(kAsmThreads) void k_win_assemble(WinProblem P, WinBuf W, const double* __restrict__ Hpan,
                                                      const double* __restrict__ r, const double* __restrict__ x,
                                                      const unsigned char* __restrict__ constant, int first,
                                                      const double* __restrict__ x_left, const double* __restrict__ scale_halo) {
  __shared__ double sA[NP * (NP + 1)];
  __shared__ double sB[NBETA * NP];           // H[beta rows][pose columns]: the frame's B block
  __shared__ double sg[NP], ss[NP], ssn[NP], scf[WB], sbs[NBETA], red[kAsmThreads / 64];
  const int f = blockIdx.x, tid = threadIdx.x, F = P.F;
  const double* H = Hpan + (size_t)f * kHRows * kHLd;
  const double lam2 = P.lambda_t * P.lambda_t, bp2 = P.beta_pose * P.beta_pose;
  const bool pair_right = f + 1 < F || P.halo, pair_left = f > 0 || x_left != nullptr;
  const int npairs = (P.lambda_t > 0.0) ? ((int)pair_right + (int)pair_left) : 0;
  // Every global operand of the frame is requested before the first is used (a load-store loop compiles to one dependent
  // L2 round trip per trip: 23 of them for the 76 x 76 block alone)
  constexpr int kAPasses = (NP * NP + kAsmThreads - 1) / kAsmThreads, kBPasses = (NBETA * NP + kAsmThreads - 1) / kAsmThreads;
  double av[kAPasses], bv[kBPasses];
#pragma unroll
  for (int u = 0; u < kAPasses; ++u) {
    const int e = min(tid + u * kAsmThreads, NP * NP - 1);
    const int i = e / NP, j = e % NP, lo = i > j ? i : j, hi = i > j ? j : i;
    av[u] = H[(size_t)lo * kHLd + hi];
  }
#pragma unroll
  for (int u = 0; u < kBPasses; ++u) {
    const int e = min(tid + u * kAsmThreads, NBETA * NP - 1);
    bv[u] = H[(size_t)(NP + e / NP) * kHLd + e % NP];
  }
  const int tc = min(tid, NP - 1);
  double g_in = H[(size_t)(NP + NBETA) * kHLd + tc];
  const double rp_in = (P.prior_rows > 0) ? r[P.row_prior + (size_t)f * P.prior_rows + max(tc - 7, 0)] : 0.0;
  const int ti_c = temporal_row(max(tc, 1));
  const double rt_r = (P.lambda_t > 0.0 && pair_right) ? r[P.row_temporal + (size_t)f * 75 + ti_c] : 0.0;
  const double rt_l = (P.lambda_t > 0.0 && f > 0) ? r[P.row_temporal + (size_t)(f - 1) * 75 + ti_c] : 0.0;
  const double xl_in = (f == 0 && x_left) ? x_left[tc] - x[tc] : 0.0;
  const double cf_in = (constant && constant[tc]) ? 1.0 : 0.0;
  const double sc_in = first ? 0.0 : W.scale[(size_t)f * NP + tc];
  const double scn_in = (!first && f + 1 < F) ? W.scale[(size_t)(f + 1) * NP + tc] : 0.0;
  double dn_in = (first && f + 1 < F) ? Hpan[(size_t)(f + 1) * kHRows * kHLd + (size_t)tc * kHLd + tc] : 0.0;
  const double sh_in = (f + 1 == F && P.halo && scale_halo) ? scale_halo[tc] : 0.0;
  const double sbeta_in = W.scale[(size_t)F * NP + min(tid, NBETA - 1)];
  const double inv_radius = 1.0 / W.status[kWsRadius];
#pragma unroll
  for (int u = 0; u < kAPasses; ++u) {
    const int e = tid + u * kAsmThreads;
    if (e < NP * NP) {
      const int i = e / NP, j = e % NP;
      double v = av[u];
      if (i == j) {
        if (i >= 7 && P.prior_rows > 0) v += bp2;       // PosePriorAAAnalytic, L2 branch (include/Sim3BA.h:304-310)
        if (i >= 1) v += lam2 * npairs;                 // Vec3DiffCost on rootT, rootAA, joints (include/MultiFrameBA.h:121-142)
      }
      sA[i * (NP + 1) + j] = v;
    }
  }
#pragma unroll
  for (int u = 0; u < kBPasses; ++u)
    if (tid + u * kAsmThreads < NBETA * NP) sB[tid + u * kAsmThreads] = bv[u];
  if (tid < WB) scf[tid] = (tid < NP) ? cf_in : 0.0;
  if (tid < NBETA) sbs[tid] = sbeta_in;
  if (tid < NP) {
    double g = g_in;
    if (tid >= 7 && P.prior_rows > 0) g += P.beta_pose * rp_in;
    if (tid >= 1 && P.lambda_t > 0.0) {
      if (pair_right) g += P.lambda_t * rt_r;
      if (f > 0) g -= P.lambda_t * rt_l;
      else if (x_left) g -= P.lambda_t * (P.lambda_t * xl_in);   // the previous shard's last pair
    }
    sg[tid] = g;
  }
  __syncthreads();
  if (tid < NP) {
    double s, sn = 0.0;
    if (first) {
      s = 1.0 / (1.0 + sqrt(sA[tid * (NP + 1) + tid]));
      W.scale[(size_t)f * NP + tid] = s;
      if (f + 1 < F) {   // the next frame's scale, from its diagonal entry alone (its workgroup may not have run yet)
        double dn = dn_in;
        if (tid >= 7 && P.prior_rows > 0) dn += bp2;
        if (tid >= 1 && P.lambda_t > 0.0) dn += lam2 * (1 + (int)(f + 2 < F || P.halo));
        sn = 1.0 / (1.0 + sqrt(dn));
      }
    } else {
      s = sc_in;
      if (f + 1 < F) sn = scn_in;
    }
    if (f + 1 == F && P.halo && scale_halo) sn = sh_in;
    ss[tid] = s; ssn[tid] = sn;
    W.graw[(size_t)f * NP + tid] = sg[tid];
    W.Eraw[(size_t)f * NP + tid] = (tid >= 1 && pair_right && P.lambda_t > 0.0) ? -lam2 : 0.0;
  }
  __syncthreads();
  double* D = W.D + (size_t)f * WB * WB;
  double* U = W.U + (size_t)f * WB * WB;
  for (int e = tid; e < WB * WB; e += kAsmThreads) {
    const int i = e / WB, j = e % WB;
    double v = (i == j) ? 1.0 : 0.0, u = 0.0;
    if (i < NP && j < NP) {
      if (scf[i] == 0.0 && scf[j] == 0.0) {
        v = sA[i * (NP + 1) + j] * ss[i] * ss[j];
        if (i == j) {
          v += fmin(fmax(v, 1e-6), 1e32) * inv_radius;
          if (i >= 1 && pair_right && P.lambda_t > 0.0) u = -lam2 * ss[i] * ssn[i];
        }
      }
    }
    D[e] = v;
    U[e] = u;
  }
  for (int e = tid; e < NP * NP; e += kAsmThreads) W.Araw[(size_t)f * NP * NP + e] = sA[(e / NP) * (NP + 1) + e % NP];
  double* Rt = W.Rt + (size_t)f * WR * WB;
  double* Rt0 = W.Rt0 + (size_t)f * WR * WB;
  for (int e = tid; e < WR * WB; e += kAsmThreads) {
    const int c = e / WB, i = e % WB;
    double v = 0.0;
    if (i < NP && scf[i] == 0.0) {
      if (c < P.nb) v = sB[c * NP + i] * ss[i] * sbs[c];
      else if (c == NBETA) v = -sg[i] * ss[i];
    }
    Rt[e] = v;
    Rt0[e] = v;
  }
  for (int e = tid; e < NP * NBETA; e += kAsmThreads) {
    const int i = e / NBETA, c = e % NBETA;
    W.Braw[(size_t)f * NP * NBETA + e] = (c < P.nb) ? sB[c * NP + i] : 0.0;
  }
  // gradient tolerance test: max |g_i| over the free parameters, the bounded scale projected (Ceres gradient_tolerance)
  double gm = 0.0;
  if (tid < NP && scf[tid] == 0.0) {
    double gi = sg[tid];
    if (tid == 0) {
      const double s0 = x[(size_t)f * NP];
      gi = s0 - fmin(fmax(s0 - gi, P.scale_lo), P.scale_hi);
    }
    gm = fabs(gi);
  }
  gm = block_max_n(gm, red, tid, kAsmThreads / 64);
  if (tid == 0) W.gmaxp[f] = gm;
}

// ---- beta Schur complement: per-frame partials, then the 10 x 10 solve ---------------------------------------------------
__global__ __launch_bounds__(128) void k_win_schur_part(WinProblem P, WinBuf W) {
  __shared__ double sBt[(NBETA + 1) * WB], sXt[(NBETA + 1) * WB];
  const int f = blockIdx.x, tid = threadIdx.x;
  const double* B = W.Rt0 + (size_t)f * WR * WB;     // scaled [B | rhs]^T as assembled
  const double* X = W.Xt + (size_t)f * WR * WB;
  {
    // both 11 x 80 operands into LDS, every load issued before the first is used
    constexpr int kN = (NBETA + 1) * WB, kPasses = (kN + 127) / 128;
    double bv[kPasses], xv[kPasses];
#pragma unroll
    for (int u = 0; u < kPasses; ++u) { const int e = min(tid + u * 128, kN - 1); bv[u] = B[e]; xv[u] = X[e]; }
#pragma unroll
    for (int u = 0; u < kPasses; ++u) { const int e = tid + u * 128; if (e < kN) { sBt[e] = bv[u]; sXt[e] = xv[u]; } }
  }
  __syncthreads();
  if (tid < NBETA * NBETA + NBETA) {
    const int a = (tid < NBETA * NBETA) ? tid / NBETA : tid - NBETA * NBETA;
    const int c = (tid < NBETA * NBETA) ? tid % NBETA : NBETA;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int i = 0; i + 1 < NP; i += 2) { s0 += sBt[a * WB + i] * sXt[c * WB + i]; s1 += sBt[a * WB + i + 1] * sXt[c * WB + i + 1]; }
    W.part[(size_t)f * kWinPart + tid] = s0 + s1;
  }
}

// mode 0: all; 1: this shard's sums of the Schur partials -> W.sred[110] only; 2: solve from W.sred (summed over the shards)
__global__ __launch_bounds__(1024) void k_win_beta_solve(WinProblem P, WinBuf W, const double* __restrict__ beta,
                                                         double* __restrict__ beta_new, int mode) {
  __shared__ double red[8][128];
  __shared__ double S[NBETA * NBETA], rb[NBETA];
  const int tid = threadIdx.x, F = P.F;
  if (P.nb == 0) return;
  // sums over the frames: 110 words, eight frame lanes of 128 threads, four independent loads per pass
  const int w = tid & 127, g = tid >> 7;
  if (mode != 2) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (w < NBETA * NBETA + NBETA) {
      int f = g;
      for (; f + 120 < F; f += 128) {        // sixteen loads in flight
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = W.part[(size_t)(f + 8 * u) * kWinPart + w];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; u += 4) { s0 += v[u]; s1 += v[u + 1]; s2 += v[u + 2]; s3 += v[u + 3]; }
      }
      for (; f < F; f += 8) s0 += W.part[(size_t)f * kWinPart + w];
    }
    red[g][w] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();
  if (tid < NBETA * NBETA + NBETA) {
    double s;
    if (mode == 2) s = W.sred[tid];
    else s = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid]));
    if (mode == 1) W.sred[tid] = s;
    if (tid < NBETA * NBETA) S[tid] = W.Cs[tid] - s; else rb[tid - NBETA * NBETA] = W.rhsb[tid - NBETA * NBETA] - s;
  }
  if (mode == 1) return;
  __syncthreads();
  if (tid < 64) {
    // 10 x 10 Cholesky + both substitutions in the registers of one wave (dense_inl.h): lanes 0-15 the rows of S padded with
    // the identity, lane 16 the right-hand side as one more row (comes out as y^T = rb^T L^-T), lanes 32-47 the identity
    // (comes out as L^-T);  x = L^-T y
    const int rr = tid & 15, grp = tid >> 4;
    double av[16], iv[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      double v = 0.0;
      if (grp == 0) v = (rr < NBETA && k < NBETA) ? ((k <= rr) ? S[rr * NBETA + k] : 0.0) : (rr == k ? 1.0 : 0.0);
      else if (grp == 1) v = (rr == 0 && k < NBETA) ? rb[k] : 0.0;
      else if (grp == 2) v = (rr == k) ? 1.0 : 0.0;
      av[k] = v;
    }
    const bool ok = diag_factor16(av, rr, grp == 0, iv, NBETA);
    double x = 0.0;
#pragma unroll
    for (int k = 0; k < NBETA; ++k) x += av[k] * readlane_f64(av[k], 16);     // lanes 32 + r: sum_k (L^-T)[r][k] y[k]
    if (grp == 2 && rr < NBETA) {
      const double dsb = ok ? x : 0.0;
      W.dsb[rr] = dsb;
      const double di = dsb * W.scale[(size_t)F * NP + rr];
      W.d[(size_t)F * NP + rr] = di;
      beta_new[rr] = beta[rr] + di;
    }
    if (tid == 0 && !ok) *W.fail = 1;
  }
}

// ---- step of one frame: d_f = S_f (x_f - X_B,f d_beta), candidate projected on the scale bounds --------------------------
__global__ __launch_bounds__(128) void k_win_step(WinProblem P, WinBuf W, const double* __restrict__ x,
                                                  double* __restrict__ x_new) {
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid >= NP) return;
  const double* X = W.Xt + (size_t)f * WR * WB;
  double xc[NBETA], dc[NBETA];
#pragma unroll
  for (int c = 0; c < NBETA; ++c) { xc[c] = X[c * WB + tid]; dc[c] = W.dsb[c]; }   // (dsb is zero past nb)
  double ds = X[NBETA * WB + tid];
  const double sc = W.scale[(size_t)f * NP + tid];
  const double xi = x[(size_t)f * NP + tid];
#pragma unroll
  for (int c = 0; c < NBETA; ++c) ds -= (c < P.nb) ? xc[c] * dc[c] : 0.0;
  double di = ds * sc;
  if (tid == 0) {
    const double s_new = fmin(fmax(xi + di, P.scale_lo), P.scale_hi);
    di = s_new - xi;
  }
  W.d[(size_t)f * NP + tid] = di;
  x_new[(size_t)f * NP + tid] = xi + di;
}
__global__ __launch_bounds__(128) void k_win_model(WinProblem P, WinBuf W, const double* __restrict__ x,
                                                   const double* __restrict__ d_halo) {
  __shared__ double sd[NP], sdn[NP], sdb[NBETA], red[2];
  const int f = blockIdx.x, tid = threadIdx.x, F = P.F;
  if (tid < NP) {
    sd[tid] = W.d[(size_t)f * NP + tid];
    sdn[tid] = (f + 1 < F) ? W.d[(size_t)(f + 1) * NP + tid] : ((P.halo && d_halo) ? d_halo[tid] : 0.0);
  }
  if (tid < NBETA) sdb[tid] = (tid < P.nb) ? W.d[(size_t)F * NP + tid] : 0.0;
  __syncthreads();
  double pm = 0.0, dn = 0.0, xn = 0.0;
  if (tid < NP) {
    // A is symmetric: thread i walks COLUMN i (consecutive threads read consecutive words), 19 loads in flight per batch
    const double* Ac = W.Araw + (size_t)f * NP * NP + tid;
    double hd = 0.0, h1 = 0.0;
#pragma unroll 1
    for (int jb = 0; jb < NP; jb += 19) {
      double aw[19];
#pragma unroll
      for (int u = 0; u < 19; ++u) aw[u] = Ac[(size_t)(jb + u) * NP];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u + 1 < 19; u += 2) { hd += aw[u] * sd[jb + u]; h1 += aw[u + 1] * sd[jb + u + 1]; }
      hd += aw[18] * sd[jb + 18];
    }
    hd += h1;
    double bw[NBETA];
#pragma unroll
    for (int c = 0; c < NBETA; ++c) bw[c] = W.Braw[((size_t)f * NP + tid) * NBETA + c];
#pragma unroll
    for (int c = 0; c < NBETA; ++c) hd += 2.0 * bw[c] * sdb[c];
    hd += 2.0 * W.Eraw[(size_t)f * NP + tid] * sdn[tid];
    pm = -sd[tid] * W.graw[(size_t)f * NP + tid] - 0.5 * sd[tid] * hd;
    dn = sd[tid] * sd[tid];
    const double xv = x[(size_t)f * NP + tid];
    xn = xv * xv;
  }
  pm = block_sum_n(pm, red, tid, 2);
  dn = block_sum_n(dn, red, tid, 2);
  xn = block_sum_n(xn, red, tid, 2);
  if (tid == 0) {
    double* o = W.part + (size_t)f * kWinPart + 112;
    o[0] = pm; o[1] = dn; o[2] = xn;
  }
}

__global__ __launch_bounds__(256) void k_win_finish(WinProblem P, WinBuf W, const double* __restrict__ x,
                                                    const double* __restrict__ beta, double* __restrict__ x_new,
                                                    double* __restrict__ beta_new, int mode) {
  __shared__ double red[4];
  const int tid = threadIdx.x, F = P.F;
  double pm = 0.0, dn = 0.0, xn = 0.0, gm = 0.0;
  if (mode != 2) {
    for (int f = tid; f < F; f += 256) {
      const double* o = W.part + (size_t)f * kWinPart + 112;
      pm += o[0]; dn += o[1]; xn += o[2];
      gm = fmax(gm, W.gmaxp[f]);
    }
    pm = block_sum_n(pm, red, tid, 4);
    dn = block_sum_n(dn, red, tid, 4);
    xn = block_sum_n(xn, red, tid, 4);
    gm = block_max_n(gm, red, tid, 4);
    if (mode == 1) {
      if (tid == 0) { W.fin[0] = pm; W.fin[1] = dn; W.fin[2] = xn; W.fin[3] = gm; W.fin[4] = *W.fail ? 1.0 : 0.0; }
      return;
    }
  } else {
    pm = W.fin[0]; dn = W.fin[1]; xn = W.fin[2]; gm = W.fin[3];
    if (tid == 0 && W.fin[4] != 0.0) *W.fail = 1;
  }
  finish_core(P, W, x, beta, x_new, beta_new, pm, dn, xn, gm, tid);
}

// ---- single-GPU tail of an iteration in ONE launch: the step of every frame (k_win_step), its share of the model cost
//      change (k_win_model; the next frame's step, which the temporal term needs, is recomputed here instead of read), and —
//      by the LAST workgroup to finish, found by a ticket — the decision (k_win_finish).  Two launch floors (~5 us each) and
//      their boundaries less per iteration.  Sharded solves exchange boundary rows between these steps and keep the three
//      kernels. ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_win_tail(WinProblem P, WinBuf W, const double* __restrict__ x,
                                                  const double* __restrict__ beta, double* __restrict__ x_new,
                                                  double* __restrict__ beta_new) {
  __shared__ double sd[2][NP], sdb[NBETA], red[4];
  __shared__ int s_last;
  const int f = blockIdx.x, tid = threadIdx.x, F = P.F;
  {
    // d of frame f (threads 0..75, stored) and of frame f + 1 (threads 128..203, kept here)
    const int h = tid >> 7, i = tid & 127, ff = f + h;
    if (i < NP) {
      double di = 0.0;
      if (ff < F) {
        const double* X = W.Xt + (size_t)ff * WR * WB;
        double xc[NBETA], dc[NBETA];
#pragma unroll
        for (int c = 0; c < NBETA; ++c) { xc[c] = X[c * WB + i]; dc[c] = W.dsb[c]; }
        double ds = X[NBETA * WB + i];
        const double sc = W.scale[(size_t)ff * NP + i];
        const double xi = x[(size_t)ff * NP + i];
#pragma unroll
        for (int c = 0; c < NBETA; ++c) ds -= (c < P.nb) ? xc[c] * dc[c] : 0.0;
        di = ds * sc;
        if (i == 0) {
          const double s_new = fmin(fmax(xi + di, P.scale_lo), P.scale_hi);
          di = s_new - xi;
        }
        if (h == 0) {
          W.d[(size_t)f * NP + i] = di;
          x_new[(size_t)f * NP + i] = xi + di;
        }
      }
      sd[h][i] = di;
    }
    if (tid >= 224 && tid < 224 + NBETA) sdb[tid - 224] = (tid - 224 < P.nb) ? W.d[(size_t)F * NP + tid - 224] : 0.0;
  }
  __syncthreads();
  double pm = 0.0, dn = 0.0, xn = 0.0;
  if (tid < NP) {
    const double* Ac = W.Araw + (size_t)f * NP * NP + tid;
    double hd = 0.0, h1 = 0.0;
#pragma unroll 1
    for (int jb = 0; jb < NP; jb += 19) {
      double aw[19];
#pragma unroll
      for (int u = 0; u < 19; ++u) aw[u] = Ac[(size_t)(jb + u) * NP];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u + 1 < 19; u += 2) { hd += aw[u] * sd[0][jb + u]; h1 += aw[u + 1] * sd[0][jb + u + 1]; }
      hd += aw[18] * sd[0][jb + 18];
    }
    hd += h1;
    double bw[NBETA];
#pragma unroll
    for (int c = 0; c < NBETA; ++c) bw[c] = W.Braw[((size_t)f * NP + tid) * NBETA + c];
#pragma unroll
    for (int c = 0; c < NBETA; ++c) hd += 2.0 * bw[c] * sdb[c];
    hd += 2.0 * W.Eraw[(size_t)f * NP + tid] * sd[1][tid];
    pm = -sd[0][tid] * W.graw[(size_t)f * NP + tid] - 0.5 * sd[0][tid] * hd;
    dn = sd[0][tid] * sd[0][tid];
    const double xv = x[(size_t)f * NP + tid];
    xn = xv * xv;
  }
  pm = block_sum_n(pm, red, tid, 4);
  dn = block_sum_n(dn, red, tid, 4);
  xn = block_sum_n(xn, red, tid, 4);
  if (tid == 0) {
    // the partial is at the memory side before the ticket is taken: write-through stores and this wave's vmcnt(0) (cdna guide,
    // Guideline 16 R1), not an agent-scope release fence (buffer_wbl2 writes back every dirty line of the XCD's L2)
    double* o = W.part + (size_t)f * kWinPart + 112;
    store_f64_through(o, pm); store_f64_through(o + 1, dn); store_f64_through(o + 2, xn);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // two-level ticket: groups of 32 frames, then the groups (atomics on ONE word serialise at ~40 ns each: 1024 of them
    // were two thirds of this kernel at 1024 frames)
    const int grp = f >> 5, ngrp = (F + 31) >> 5, gsize = min(32, F - 32 * grp);
    int last = 0;
    if (atomicAdd(W.ticket + 1 + grp, 1) == gsize - 1) {
      __hip_atomic_store(W.ticket + 1 + grp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (for the next launch)
      last = (atomicAdd(W.ticket, 1) == ngrp - 1) ? 1 : 0;
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  // ---- the last workgroup: every frame's partial is at the memory side (sc1 loads: past this XCD's L2), decide ----
  if (tid == 0) __hip_atomic_store(W.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  pm = 0.0; dn = 0.0; xn = 0.0;
  double gm = 0.0;
  for (int g = tid; g < F; g += 256) {
    const double* o = W.part + (size_t)g * kWinPart + 112;
    pm += __hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    dn += __hip_atomic_load(o + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    xn += __hip_atomic_load(o + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gm = fmax(gm, W.gmaxp[g]);
  }
  pm = block_sum_n(pm, red, tid, 4);
  dn = block_sum_n(dn, red, tid, 4);
  xn = block_sum_n(xn, red, tid, 4);
  gm = block_max_n(gm, red, tid, 4);
  finish_core(P, W, x, beta, x_new, beta_new, pm, dn, xn, gm, tid);
}

// mode 0: all; 1: this shard's cost at the candidate -> W.fin[0] only; 2: decide with W.fin[0] (summed over the shards);
// 3: this shard's cost at the candidate -> W.fin[5] only (sharded solves: the decision is k_win_decide's)
__global__ __launch_bounds__(1024) void k_win_accept(WinProblem P, WinBuf W, const double* __restrict__ r_new,
                                                     double* __restrict__ x, double* __restrict__ beta,
                                                     const double* __restrict__ x_new, const double* __restrict__ beta_new,
                                                     int mode) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  double* st = W.status;
  if (mode == 1 || mode == 3) {
    const double c = window_cost_any(P, r_new, red, tid, 1024);
    if (tid == 0) W.fin[mode == 1 ? 0 : 5] = c;
    return;
  }
  if (st[kWsHasCand] == 0.0) {
    if (tid == 0) st[kWsJsel] = 2.0;     // no candidate was produced (inactive solve, failed factorisation): nothing moved
    return;
  }
  const double new_cost = (mode == 2) ? W.fin[0] : window_cost_any(P, r_new, red, tid, 1024);
  (void)accept_core(P, W, x, beta, x_new, beta_new, new_cost, tid, 1024);
}

}  // namespace

void launch_win_init(const WinProblem& P, const WinBuf& W, const double* d_r, int mode, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_init, dim3(1), dim3(1024), 0, s, P, W, d_r, mode);
}
void launch_win_beta(const WinProblem& P, const WinBuf& W, const double* d_Hpan, const double* d_r, int first, int mode,
                     hipStream_t s) {
  BODYFIT_LAUNCH(k_win_beta, dim3(1), dim3(1024), 0, s, P, W, d_Hpan, d_r, first, mode);
}
void launch_win_assemble(const WinProblem& P, const WinBuf& W, const double* d_Hpan, const double* d_r, const double* d_x,
                         const unsigned char* d_constant, int first, const double* d_x_left, const double* d_scale_halo,
                         hipStream_t s) {
  BODYFIT_LAUNCH(k_win_assemble, dim3(P.F), dim3(kAsmThreads), 0, s, P, W, d_Hpan, d_r, d_x, d_constant, first, d_x_left,
                     d_scale_halo);
}
void launch_win_schur_part(const WinProblem& P, const WinBuf& W, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_schur_part, dim3(P.F), dim3(128), 0, s, P, W);
}
void launch_win_beta_solve(const WinProblem& P, const WinBuf& W, const double* d_beta, double* d_beta_new, int mode, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_beta_solve, dim3(1), dim3(1024), 0, s, P, W, d_beta, d_beta_new, mode);
}
void launch_win_tail(const WinProblem& P, const WinBuf& W, const double* d_x, const double* d_beta, double* d_x_new, double* d_beta_new,
                     hipStream_t s) {
  BODYFIT_LAUNCH(k_win_tail, dim3(P.F), dim3(256), 0, s, P, W, d_x, d_beta, d_x_new, d_beta_new);
}
void launch_win_step(const WinProblem& P, const WinBuf& W, const double* d_x, double* d_x_new, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_step, dim3(P.F), dim3(128), 0, s, P, W, d_x, d_x_new);
}
void launch_win_model(const WinProblem& P, const WinBuf& W, const double* d_x, const double* d_halo_step, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_model, dim3(P.F), dim3(128), 0, s, P, W, d_x, d_halo_step);
}
void launch_win_finish(const WinProblem& P, const WinBuf& W, const double* d_x, const double* d_beta, double* d_x_new,
                       double* d_beta_new, int mode, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_finish, dim3(1), dim3(256), 0, s, P, W, d_x, d_beta, d_x_new, d_beta_new, mode);
}
void launch_win_accept(const WinProblem& P, const WinBuf& W, const double* d_r_new, double* d_x, double* d_beta,
                       const double* d_x_new, const double* d_beta_new, int mode, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_accept, dim3(1), dim3(1024), 0, s, P, W, d_r_new, d_x, d_beta, d_x_new, d_beta_new, mode);
}

}  // namespace bodyfit
