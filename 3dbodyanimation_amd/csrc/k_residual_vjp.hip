// k_residual_vjp.hip — vector-Jacobian product of the WHOLE residual vector of a problem (bodyfit_residual_vjp_device):
// given g = dL/dr over the rows of bodyfit_problem_layout, dL/dframe_params = (dr/dx)^T g and dL/dbeta = (dr/dbeta)^T g.
// Host side: api_vjp.hip.
//
// Row kinds and their Jacobians (as the sweep writes the rows: k_sweep.hip, priors_inl.h):
//   reprojection  the dense [2K][n_cols] panel of the sweep (d_J); frame f owns rows 2 kp_offset[f] .. 2 kp_offset[f+1] - 1
//   pose prior    L2: r = beta_p x[7:], J = beta_p I.  GMM: r = beta_p s (x[7:] - mu_k) L_k (k = the sweep's component of
//                 the frame), J = beta_p s L_k^T, so the gradient is beta_p s L_k g; the last row beta_p sqrt(-log w_k) is
//                 constant.  The host builds [K][D][npose] rows G_k[c][7 + d] = beta_p s L_k[d][c] once per problem, laid out
//                 like a row of the panel, so the product is the same column loop as the reprojection rows
//   shape prior   beta_s I on beta (per frame when beta_per_frame)
//   temporal      pair f: lambda (a_f - a_{f+1}) on rootT, rootAA, joints 1..nJ-1: frame f gets +lambda g, frame f+1 -lambda g
//                 (with temporal_halo the last pair's -lambda g goes to the halo row F, which gets nothing else)
//
// One wave per frame (4 frames per 256-thread workgroup).  Lane l owns columns 2l and 2l + 1 of the frame's row (a row of 86
// doubles is 43 lanes x 16 bytes: one coalesced load per row), accumulates them over the frame's rows in ascending order with
// kRows rows in flight, then adds the prior / temporal terms and stores its columns once.  g of a row is the same for the whole
// wave.  No atomics and no LDS: a frame's gradient row (and its beta row) depends on that frame's rows of J and g only, so it is
// bit-identical whatever the frame count and wherever the frame sits.  Shared beta: each frame writes a [nS] partial, summed
// in a fixed order by k_vjp_beta_sum (k_forward_vjp.hip); the shared shape-prior term rides on frame 0's partial.
#include <hip/hip_runtime.h>

#include "bodyfit_device.h"

namespace bodyfit {

namespace {

constexpr int kRows = 16;           // panel rows in flight per wave
constexpr int kWavesPerBlock = 4;   // frames per workgroup (16 rows in flight take 144 VGPRs: three waves per SIMD)

// lane's two columns of row `row` of a row-major panel of `ncols` columns; kPair: 16-byte aligned rows (even ncols)
template <bool kPair>
__device__ __forceinline__ double2 load_pair(const double* __restrict__ base, int ncols, int row, int c0) {
  const double* p = base + (size_t)row * ncols + c0;
  if (kPair) {
    if (c0 < ncols) return *reinterpret_cast<const double2*>(p);
    return double2{0.0, 0.0};
  }
  double2 v{0.0, 0.0};
  if (c0 < ncols) v.x = p[0];
  if (c0 + 1 < ncols) v.y = p[1];
  return v;
}

// a0, a1 += sum over rows [r0, r1) of g[grow0 + (r - r0)] * panel[r][c0 .. c0 + 1], rows in ascending order
template <bool kPair>
__device__ __forceinline__ void accumulate_rows(const double* __restrict__ panel, int ncols, int r0, int r1,
                                                const double* __restrict__ g, int grow0, int c0, double& a0, double& a1) {
  for (int rb = r0; rb < r1; rb += kRows) {
    double2 v[kRows];
    double gr[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int r = rb + u;
      const bool ok = r < r1;
      v[u] = ok ? load_pair<kPair>(panel, ncols, r, c0) : double2{0.0, 0.0};
      gr[u] = ok ? g[grow0 + (r - r0)] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      a0 = fma(gr[u], v[u].x, a0);
      a1 = fma(gr[u], v[u].y, a1);
    }
  }
}

// temporal row of frame parameter column s (temporal_rows, priors_inl.h): rootT -> 0..2, rootAA -> 3..5, joints -> 6..; -1: scale
__device__ __forceinline__ int temporal_slot(int s) { return s == 0 ? -1 : (s < 4 ? s + 2 : (s < 7 ? s - 4 : s - 1)); }

template <bool kPair>
__global__ __launch_bounds__(256) void k_residual_vjp(const ResVjpArgs a) {
  const int f = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= a.n_param_rows) return;
  const int c0 = 2 * lane, npose = a.npose, D = npose - 7;
  double a0 = 0.0, a1 = 0.0;   // reprojection rows
  double p0 = 0.0, p1 = 0.0;   // pose prior rows
  if (f < a.F) {
    const int r0 = 2 * a.kp_offset[f], r1 = 2 * a.kp_offset[f + 1];
    accumulate_rows<kPair>(a.J, a.ncols, r0, r1, a.g, r0, c0, a0, a1);
    if (a.prior_rows > 0) {
      const int grow = a.row_prior + f * a.prior_rows;
      if (a.gmm_rows) {
        const double* Gk = a.gmm_rows + (size_t)a.comp[f] * D * npose;
        accumulate_rows<true>(Gk, npose, 0, D, a.g, grow, c0, p0, p1);   // (npose = 76 here: even)
      } else {
        if (c0 >= 7 && c0 < npose) p0 = a.beta_pose * a.g[grow + c0 - 7];
        if (c0 + 1 >= 7 && c0 + 1 < npose) p1 = a.beta_pose * a.g[grow + c0 + 1 - 7];
      }
    }
  }
  const int T = npose - 1;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = c0 + h;
    if (c >= a.ncols) break;
    const double acc = (h == 0 ? a0 : a1) + (h == 0 ? p0 : p1);
    if (c < npose) {
      double v = acc;
      const int slot = temporal_slot(c);
      if (a.n_pairs > 0 && slot >= 0) {
        if (f < a.n_pairs) v += a.lambda_t * a.g[a.row_temporal + (size_t)f * T + slot];
        if (f >= 1 && f - 1 < a.n_pairs) v -= a.lambda_t * a.g[a.row_temporal + (size_t)(f - 1) * T + slot];
      }
      a.gx[(size_t)f * npose + c] = v;
    } else if (a.gb && f < a.F) {
      const int j = c - npose;
      double v = acc;
      if (a.shape_rows > 0) {
        if (a.shape_per_frame) v += a.beta_shape * a.g[a.row_shape + f * a.nS + j];
        else if (f == 0) v += a.beta_shape * a.g[a.row_shape + j];
      }
      a.gb[(size_t)f * a.nS + j] = v;
    }
  }
}

}  // namespace

void launch_residual_vjp(const ResVjpArgs& a, hipStream_t s) {
  if (a.n_param_rows <= 0) return;
  const dim3 grid((a.n_param_rows + kWavesPerBlock - 1) / kWavesPerBlock), block(64 * kWavesPerBlock);
  if (a.ncols % 2 == 0) BODYFIT_LAUNCH(k_residual_vjp<true>, grid, block, 0, s, a);
  else BODYFIT_LAUNCH(k_residual_vjp<false>, grid, block, 0, s, a);
}

}  // namespace bodyfit
