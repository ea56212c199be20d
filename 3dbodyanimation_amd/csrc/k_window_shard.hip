// k_window_shard.hip — the device window LM (k_window_lm.hip) sharded over several GPUs (bodyfit_solve_sharded*): what the
// exchanges between the shards need, and the decision of an iteration from every shard's partials.
#include <algorithm>

#include "window_lm_inl.h"

namespace bodyfit {
namespace {

// sum of the shards' partials in rank order: out[i] = sum_r gathered[r][i] (every rank computes bit-identical totals)
__global__ __launch_bounds__(256) void k_sum_ranks(const double* __restrict__ g, int N, int stride, int n, double* __restrict__ out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    double s = 0.0;
    for (int r = 0; r < N; ++r) s += g[(size_t)r * stride + i];
    out[i] = s;
  }
}
// shard proxy (bodyfit_set_shard_proxy, a measurement aid): the one-rank all-gather has filled slot 0; the other N - 1 slots
// get copies, as if N identical shards had contributed
__global__ __launch_bounds__(256) void k_replicate_ranks(double* __restrict__ g, int n, int N) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double v = g[i];
    for (int r = 1; r < N; ++r) g[(size_t)r * n + i] = v;
  }
}
// this shard's contribution to the interface system: [D_first, D_last, U_first, U_last | Rt_first, Rt_last | extra], one
// contiguous buffer for ONE all-gather
__global__ __launch_bounds__(256) void k_iface_pack(WinBuf W, int F, const double* __restrict__ extra, int n_extra,
                                                    double* __restrict__ send) {
  constexpr int blk = WB * WB, rhs = WR * WB;
  const int fl = F - 1, total = 4 * blk + 2 * rhs + n_extra;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    double v;
    if (i < blk) v = W.D[i];
    else if (i < 2 * blk) v = W.D[(size_t)fl * blk + (i - blk)];
    else if (i < 3 * blk) v = W.U[i - 2 * blk];
    else if (i < 4 * blk) v = W.U[(size_t)fl * blk + (i - 3 * blk)];
    else if (i < 4 * blk + rhs) v = W.Rt[i - 4 * blk];
    else if (i < 4 * blk + 2 * rhs) v = W.Rt[(size_t)fl * rhs + (i - 4 * blk - rhs)];
    else v = extra[i - 4 * blk - 2 * rhs];
    send[i] = v;
  }
}
// the gathered contributions -> the interface chain of 2 N frames (every rank builds the same), the extras summed in rank order
__global__ __launch_bounds__(256) void k_iface_unpack(WinBuf Wi, const double* __restrict__ g, int N, int n_extra,
                                                      double* __restrict__ extra_sum) {
  constexpr int blk = WB * WB, rhs = WR * WB;
  const int per = 4 * blk + 2 * rhs + n_extra;
  const int total = N * (4 * blk + 2 * rhs) + n_extra;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    if (i < N * (4 * blk + 2 * rhs)) {
      const int r = i / (4 * blk + 2 * rhs), j = i - r * (4 * blk + 2 * rhs);
      const double v = g[(size_t)r * per + j];
      if (j < 2 * blk) Wi.D[(size_t)(2 * r) * blk + j] = v;
      else if (j < 4 * blk) Wi.U[(size_t)(2 * r) * blk + (j - 2 * blk)] = v;
      else Wi.Rt[(size_t)(2 * r) * rhs + (j - 4 * blk)] = v;
    } else {
      const int e = i - N * (4 * blk + 2 * rhs);
      double s = 0.0;
      for (int r = 0; r < N; ++r) s += g[(size_t)r * per + 4 * blk + 2 * rhs + e];
      extra_sum[e] = s;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *Wi.fail = 0;
}
// The steps of the neighbouring shards' boundary frames, computed HERE from the interface solution every rank holds (node
// 2 r = first frame of shard r, 2 r + 1 = its last): the same arithmetic as k_win_step on the same numbers, so the row this
// rank keeps of its neighbour's frame is bit-identical to the neighbour's own.  block 0: the next shard's first frame (the
// halo row of the temporal pair this shard owns), block 1: the previous shard's last frame.
__global__ __launch_bounds__(128) void k_win_halo_step(WinProblem P, const double* __restrict__ Xi, const double* __restrict__ dsb,
                                                       int node_right, const double* __restrict__ scale_right,
                                                       const double* __restrict__ x_right, double* __restrict__ d_right,
                                                       double* __restrict__ xn_right, int node_left,
                                                       const double* __restrict__ scale_left, const double* __restrict__ x_left,
                                                       double* __restrict__ xn_left) {
  const int tid = threadIdx.x;
  if (tid >= NP) return;
  const bool right = blockIdx.x == 0;
  const int node = right ? node_right : node_left;
  if (node < 0) return;
  const double* X = Xi + (size_t)node * WR * WB;
  double ds = X[NBETA * WB + tid];
#pragma unroll
  for (int c = 0; c < NBETA; ++c) ds -= (c < P.nb) ? X[c * WB + tid] * dsb[c] : 0.0;
  const double sc = (right ? scale_right : scale_left)[tid];
  const double xi = (right ? x_right : x_left)[tid];
  double di = ds * sc;
  if (tid == 0) {
    const double s_new = fmin(fmax(xi + di, P.scale_lo), P.scale_hi);
    di = s_new - xi;
  }
  if (right) { d_right[tid] = di; xn_right[tid] = xi + di; }
  else xn_left[tid] = xi + di;
}
// a failed interface factorisation (every rank factors the same chain) is this shard's failure too
__global__ void k_win_fold_fail(WinBuf W, WinBuf Wi) {
  if (threadIdx.x == 0 && *Wi.fail) *W.fail = 1;
}
// The whole decision of a sharded iteration in one launch, from every shard's partials [model, |d|^2, |x|^2, max |g|, fail,
// cost at the candidate] (gathered, [N][8]): k_win_finish's tests, then — if there is a candidate — k_win_accept's.  Every
// rank runs it on the same numbers.  On acceptance the rows this rank keeps of its neighbours' boundary frames move too.
__global__ __launch_bounds__(256) void k_win_decide(WinProblem P, WinBuf W, double* __restrict__ x, double* __restrict__ beta,
                                                    double* __restrict__ x_new, double* __restrict__ beta_new,
                                                    const double* __restrict__ g, int N, double* __restrict__ x_halo,
                                                    const double* __restrict__ xn_halo, double* __restrict__ x_left,
                                                    const double* __restrict__ xn_left) {
  const int tid = threadIdx.x;
  double pm = 0.0, dn = 0.0, xn = 0.0, gm = 0.0, fl = 0.0, cost = 0.0, poison = 0.0;
  for (int r = 0; r < N; ++r) {
    const double* o = g + (size_t)r * 8;
    pm += o[0]; dn += o[1]; xn += o[2];
    gm = fmax(gm, o[3]); fl = fmax(fl, o[4]);
    cost += o[5];
    poison = fmax(poison, o[6]);
  }
  if (poison != 0.0) {
    // A rank could not produce its part of this iteration (a failed launch / HIP call: api_solve.hip puts a 1 in slot 6 of its
    // scalars and keeps taking part in the exchanges).  Every rank reads the same gathered scalars, so every rank ends the solve
    // HERE, in the same iteration: nothing moves, the host loops find the solve inactive at their next status read and return.
    if (tid == 0) {
      W.status[kWsActive] = 0.0; W.status[kWsTermination] = 2.0; W.status[kWsHasCand] = 0.0; W.status[kWsJsel] = 2.0;
      W.status[kWsPoison] = poison;
    }
    return;
  }
  if (tid == 0 && fl != 0.0) *W.fail = 1;
  __syncthreads();
  finish_core(P, W, x, beta, x_new, beta_new, pm, dn, xn, gm, tid);
  __syncthreads();
  if (W.status[kWsHasCand] == 0.0) {
    if (tid == 0) W.status[kWsJsel] = 2.0;   // nothing moved
    return;
  }
  const bool accepted = accept_core(P, W, x, beta, x_new, beta_new, cost, tid, 256);
  if (accepted && tid < NP) {
    if (x_halo) x_halo[tid] = xn_halo[tid];
    if (x_left) x_left[tid] = xn_left[tid];
  }
}


}  // namespace

void launch_sum_ranks(const double* d_g, int N, int stride, int n, double* d_out, hipStream_t s) {
  BODYFIT_LAUNCH(k_sum_ranks, dim3((n + 255) / 256), dim3(256), 0, s, d_g, N, stride, n, d_out);
}
void launch_replicate_ranks(double* d_g, int n, int N, hipStream_t s) {
  BODYFIT_LAUNCH(k_replicate_ranks, dim3(std::min(64, (n + 255) / 256)), dim3(256), 0, s, d_g, n, N);
}
int iface_doubles(int n_extra) { return 4 * WB * WB + 2 * WR * WB + n_extra; }
void launch_iface_pack(const WinBuf& W, int F, const double* d_extra, int n_extra, double* d_send, hipStream_t s) {
  BODYFIT_LAUNCH(k_iface_pack, dim3(64), dim3(256), 0, s, W, F, d_extra, n_extra, d_send);
}
void launch_iface_unpack(const WinBuf& Wi, const double* d_g, int N, int n_extra, double* d_extra_sum, hipStream_t s) {
  BODYFIT_LAUNCH(k_iface_unpack, dim3(64), dim3(256), 0, s, Wi, d_g, N, n_extra, d_extra_sum);
}
void launch_win_halo_step(const WinProblem& P, const double* d_Xi, const double* d_dsb, int node_right, const double* d_scale_right,
                          const double* d_x_right, double* d_d_right, double* d_xn_right, int node_left,
                          const double* d_scale_left, const double* d_x_left, double* d_xn_left, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_halo_step, dim3(2), dim3(128), 0, s, P, d_Xi, d_dsb, node_right, d_scale_right, d_x_right, d_d_right,
                     d_xn_right, node_left, d_scale_left, d_x_left, d_xn_left);
}
void launch_win_fold_fail(const WinBuf& W, const WinBuf& Wi, hipStream_t s) { BODYFIT_LAUNCH(k_win_fold_fail, dim3(1), dim3(64), 0, s, W, Wi); }
void launch_win_decide(const WinProblem& P, const WinBuf& W, double* d_x, double* d_beta, double* d_x_new, double* d_beta_new,
                       const double* d_g, int N, double* d_x_halo, const double* d_xn_halo, double* d_x_left,
                       const double* d_xn_left, hipStream_t s) {
  BODYFIT_LAUNCH(k_win_decide, dim3(1), dim3(256), 0, s, P, W, d_x, d_beta, d_x_new, d_beta_new, d_g, N, d_x_halo, d_xn_halo,
                     d_x_left, d_xn_left);
}
}  // namespace bodyfit
