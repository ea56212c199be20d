// k_surface_gram.hip — the Gauss-Newton normal equations of the scan terms at a fixed correspondence (bodyfit_surface_gram_device,
// declared in include/bodyfit.h; host side: api_gram.hip): per frame H = sum_i w_i A_i^T D_i A_i over the scan rows i, with
// A_i = sum_a b_ia J[.][faces[t_i][a]][0..2] the 3 x P Jacobian of the row's surface point and D_i = I (point-to-point) or d_i d_i^T
// (point-to-plane), WITHOUT forming any A_i:
//
//   sum_i w_i A_i^T D_i A_i = J^T W J,    W[(v, x), (v', y)] = sum over the faces t with v = faces[t][a], v' = faces[t][c] of M_t[a][c][x][y],
//   M_t[a][c][x][y] = sum over the rows i that chose t of w_i b_ia b_ic D_i[x][y]                     (the per-face MOMENTS)
//
// W is 3 V x 3 V, non-zero on the mesh's vertices and edges only, and does not grow with the number of scan rows.  Stages, for
// kGramFrames frames at a time (the handle holds the moments, the mixed rows and the partial panels of ONE such group):
//   a  k_gram_moments   one thread per (frame, face): the moments, f64 sums over the rows that chose the face in ascending row
//                       order — the grouping and the summation rule of k_cs_vjp_faces (a face that more than 64 rows chose: the
//                       wave, 64 interleaved ascending partial sums and a fixed butterfly) — rounded once to f32.  M is symmetric
//                       in (a, c) and in (x, y): 6 numbers per face (isotropic), 36 with directions.
//   b  k_gram_mix       Y = W J, one thread per (frame, vertex, 16 tangents): over the vertex's incident (face, corner) entries in
//                       the ascending order of the handle's vertex -> corner CSR, the three corners of the face in turn; f64
//                       sums, rounded once to f32, stored [frame][P][3 V]
//   c  k_gram_contract  H = J . Y^T on the matrix pipe.  One wave per (frame, pair of 32-tangent tiles pt >= qt, slice of 256
//                       floats of the contracted index): both operands are contiguous along that index, so a lane reads its 8
//                       consecutive floats of its row straight into the MFMA layout (V_MFMA_F32_32X32X16_BF16: lane l holds row
//                       l & 31, k = 8 (l >> 5) .. + 7), splits them into bf16 hi + lo and issues hi.hi + hi.lo + lo.hi with f32
//                       accumulation, 16 k-steps.  Rows past P and floats past 3 V are ZEROS IN REGISTERS: nothing is read past a
//                       row's 3 V floats (the padding of a row may hold anything), nothing past tangent P - 1.
//   d  k_gram_fold      one thread per (frame, p >= q): the slices' partial panels summed in f64 in ascending slice order, stored to
//                       H[p][q] and H[q][p]: exactly symmetric.
// k_gram_rhs: g[p] = sum_k J[p][k] rhs[k], the products of two f32 exact in f64, 256 interleaved ascending f64 sums and a fixed tree.
// No float atomics anywhere; every order above is a function of the frame's own data, so a frame's panel is bit-identical
// whatever the frame count, the grouping's origin (kept or rebuilt) and the frame's place in its group.  The error bound is
// derived beside the contract in include/bodyfit.h.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bodyfit_device.h"
#include "surface_gram.h"

namespace bodyfit {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 gram_bf16x8;
typedef __attribute__((ext_vector_type(16))) float gram_f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int gram_u32x4;

constexpr int kGramHeavy = 64;       // rows per face above which the wave sums the face together (kHeavy of closest_group_inl.h)
constexpr int kGramMixQ = 16;        // tangents per thread of k_gram_mix

// index of the symmetric pair (a, c), a, c in 0..2: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
__device__ __forceinline__ int sym3(int a, int c) {
  const int lo = a < c ? a : c, hi = a < c ? c : a;
  return 3 * lo - (lo * (lo - 1)) / 2 + (hi - lo);
}

// ---- stage a --------------------------------------------------------------------------------------------------------------
template <bool kPlane>
__device__ __forceinline__ void add_moment(const GramArgs& a, int i, double* m) {
  const double w = a.weight ? (double)a.weight[i] : 1.0;
  if (w == 0.0) return;                                    // (a row of weight 0 contributes nothing, whatever else it holds)
  const double b[3] = {(double)a.bary[3 * (size_t)i], (double)a.bary[3 * (size_t)i + 1], (double)a.bary[3 * (size_t)i + 2]};
  if constexpr (kPlane) {
    const double dx = a.dir[3 * (size_t)i], dy = a.dir[3 * (size_t)i + 1], dz = a.dir[3 * (size_t)i + 2];
    const double dd[6] = {dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int c = p; c < 3; ++c) {
        const double wb = w * b[p] * b[c];
        const int o = 6 * (3 * p - (p * (p - 1)) / 2 + (c - p));
#pragma unroll
        for (int e = 0; e < 6; ++e) m[o + e] = fma(wb, dd[e], m[o + e]);
      }
  } else {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int c = p; c < 3; ++c) m[3 * p - (p * (p - 1)) / 2 + (c - p)] += w * b[p] * b[c];
  }
}

template <bool kPlane>
__global__ __launch_bounds__(256) void k_gram_moments(const GramArgs a) {
  constexpr int NM = kPlane ? 36 : 6;
  const long long lrow = (long long)blockIdx.x * 256 + threadIdx.x;     // (frame of the group, face)
  const int lane = threadIdx.x & 63;
  const bool live = lrow < (long long)a.nf * a.n_faces;
  int n = 0, s = 0;
  if (live) {
    const long long grow = (long long)a.f0 * a.n_faces + lrow;          // its row in the call's grouping
    n = a.cnt[grow]; s = a.start[grow];
  }
  double m[NM];
#pragma unroll
  for (int e = 0; e < NM; ++e) m[e] = 0.0;
  if (live && n <= kGramHeavy)
    for (int k = 0; k < n; ++k) add_moment<kPlane>(a, a.sorted[s + k], m);
  // faces that many rows chose: the wave sums them together, lane l entries l, l + 64, ... then a butterfly
  unsigned long long heavy = __ballot(live && n > kGramHeavy);
  while (heavy) {
    const int src = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const int hn = __shfl(n, src, 64), hs = __shfl(s, src, 64);
    double part[NM];
#pragma unroll
    for (int e = 0; e < NM; ++e) part[e] = 0.0;
    for (int k = lane; k < hn; k += 64) add_moment<kPlane>(a, a.sorted[hs + k], part);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int e = 0; e < NM; ++e) part[e] += __shfl_xor(part[e], d, 64);
    }
    if (lane == src) {
#pragma unroll
      for (int e = 0; e < NM; ++e) m[e] = part[e];
    }
  }
  if (live) {
    float* out = a.mom + (size_t)lrow * NM;
#pragma unroll
    for (int e = 0; e < NM; ++e) out[e] = (float)m[e];
  }
}

// ---- stage b --------------------------------------------------------------------------------------------------------------
template <bool kPlane>
__global__ __launch_bounds__(256) void k_gram_mix(const GramArgs a) {
  constexpr int NM = kPlane ? 36 : 6;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.n_verts) return;
  const int q0 = blockIdx.y * kGramMixQ, lf = blockIdx.z, f = a.f0 + lf;
  const float* jf = a.jac + (size_t)f * (size_t)a.jac_stride;
  const float* mf = a.mom + (size_t)lf * (size_t)a.n_faces * NM;
  const int* cnt = a.cnt + (size_t)f * (size_t)a.n_faces;
  double acc[kGramMixQ][3];
#pragma unroll
  for (int q = 0; q < kGramMixQ; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.0;
  for (int k = a.csr_off[v]; k < a.csr_off[v + 1]; ++k) {
    const int fc = a.csr_fc[k], t = fc / 3, ca = fc - 3 * t;
    if (cnt[t] == 0) continue;                              // (no row chose the face: its moments are zeros)
    for (int c = 0; c < 3; ++c) {
      const size_t col = 3 * (size_t)a.faces[3 * t + c];
      const float* mm = mf + (size_t)t * NM + (kPlane ? 6 : 1) * sym3(ca, c);
      if constexpr (kPlane) {
        const double xx = mm[0], xy = mm[1], xz = mm[2], yy = mm[3], yz = mm[4], zz = mm[5];
#pragma unroll
        for (int q = 0; q < kGramMixQ; ++q)
          if (q0 + q < a.P) {
            const float* r = jf + (size_t)(q0 + q) * (size_t)a.row_floats + col;
            const double jx = r[0], jy = r[1], jz = r[2];
            acc[q][0] += xx * jx + xy * jy + xz * jz;
            acc[q][1] += xy * jx + yy * jy + yz * jz;
            acc[q][2] += xz * jx + yz * jy + zz * jz;
          }
      } else {
        const double w = mm[0];
#pragma unroll
        for (int q = 0; q < kGramMixQ; ++q)
          if (q0 + q < a.P) {
            const float* r = jf + (size_t)(q0 + q) * (size_t)a.row_floats + col;
            acc[q][0] += w * (double)r[0]; acc[q][1] += w * (double)r[1]; acc[q][2] += w * (double)r[2];
          }
      }
    }
  }
  const size_t K3 = 3 * (size_t)a.n_verts;
#pragma unroll
  for (int q = 0; q < kGramMixQ; ++q)
    if (q0 + q < a.P) {
      float* o = a.mixed + ((size_t)lf * a.P + (q0 + q)) * K3 + 3 * (size_t)v;
      o[0] = (float)acc[q][0]; o[1] = (float)acc[q][1]; o[2] = (float)acc[q][2];
    }
}

// ---- stage c --------------------------------------------------------------------------------------------------------------
// the lane's 8 floats row[k .. k + 7] as bf16 hi and lo fragments; ZERO where the row does not exist or k + j >= K3
__device__ __forceinline__ void load8_split(const float* row, bool row_ok, int k, int K3, gram_bf16x8* hi, gram_bf16x8* lo) {
  gram_u32x4 h, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint16_t bh[2], bl[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kk = k + 2 * j + t;
      const float x = (row_ok && kk < K3) ? row[kk] : 0.0f;
      bh[t] = f32_to_bf16(x);
      bl[t] = f32_to_bf16(x - bf16_to_f32(bh[t]));
    }
    h[j] = (uint32_t)bh[0] | ((uint32_t)bh[1] << 16);
    l[j] = (uint32_t)bl[0] | ((uint32_t)bl[1] << 16);
  }
  *hi = __builtin_bit_cast(gram_bf16x8, h);
  *lo = __builtin_bit_cast(gram_bf16x8, l);
}

__global__ __launch_bounds__(64) void k_gram_contract(const GramArgs a, int n_pairs, int n_slices) {
  const int lane = threadIdx.x, r32 = lane & 31, half = lane >> 5;
  const int pair = blockIdx.x % n_pairs, slice = blockIdx.x / n_pairs, lf = blockIdx.y, f = a.f0 + lf;
  int pt = 0;
  while ((pt + 1) * (pt + 2) / 2 <= pair) ++pt;            // pair = pt (pt + 1) / 2 + qt, qt <= pt
  const int qt = pair - pt * (pt + 1) / 2;
  const int K3 = 3 * a.n_verts;
  const int p = pt * kGramTile + r32, q = qt * kGramTile + r32;
  const bool p_ok = p < a.P, q_ok = q < a.P;
  const float* ja = a.jac + (size_t)f * (size_t)a.jac_stride + (size_t)(p_ok ? p : 0) * (size_t)a.row_floats;
  const float* yb = a.mixed + ((size_t)lf * a.P + (q_ok ? q : 0)) * (size_t)K3;
  gram_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int k_begin = slice * kGramSlice;
#pragma unroll 2
  for (int ks = 0; ks < kGramSlice / 16; ++ks) {
    const int k = k_begin + ks * 16 + 8 * half;
    gram_bf16x8 a_hi, a_lo, b_hi, b_lo;
    load8_split(ja, p_ok, k, K3, &a_hi, &a_lo);
    load8_split(yb, q_ok, k, K3, &b_hi, &b_lo);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc, 0, 0, 0);
  }
  float* out = a.part + (((size_t)lf * n_slices + slice) * n_pairs + pair) * (kGramTile * kGramTile);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 8 * (r >> 2) + 4 * half + (r & 3);     // accumulator register r of half-wave `half`: tangent pt 32 + row
    out[row * kGramTile + r32] = acc[r];
  }
}

// ---- stage d --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gram_fold(const GramArgs a, int n_pairs, int n_slices) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.P * a.P) return;
  const int p = e / a.P, q = e - p * a.P;
  if (q > p) return;
  const int lf = blockIdx.y, f = a.f0 + lf;
  const int pt = p / kGramTile, qt = q / kGramTile, pair = pt * (pt + 1) / 2 + qt;
  const float* src = a.part + ((size_t)lf * n_slices * n_pairs + pair) * (kGramTile * kGramTile) + (p - pt * kGramTile) * kGramTile +
                     (q - qt * kGramTile);
  double h = 0.0;
  for (int s = 0; s < n_slices; ++s) h += (double)src[(size_t)s * n_pairs * (kGramTile * kGramTile)];
  double* H = a.H + (size_t)f * a.P * a.P;
  H[(size_t)p * a.P + q] = h;
  H[(size_t)q * a.P + p] = h;
}

// ---- the right-hand side ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gram_rhs(const float* jac, long long row_floats, long long jac_stride, const float* rhs,
                                                  long long rhs_stride, int P, int K3, double* g) {
  __shared__ double sh[256];
  const int f = blockIdx.x / P, p = blockIdx.x - f * P, tid = threadIdx.x;
  const float* j = jac + (size_t)f * (size_t)jac_stride + (size_t)p * (size_t)row_floats;
  const float* r = rhs + (size_t)f * (size_t)rhs_stride;
  double acc = 0.0;
  for (int k = tid; k < K3; k += 256) acc += (double)j[k] * (double)r[k];   // (24 + 24 bits: the product is exact)
  sh[tid] = acc;
  for (int d = 128; d >= 1; d >>= 1) {
    __syncthreads();
    if (tid < d) sh[tid] += sh[tid + d];
  }
  if (tid == 0) g[(size_t)f * P + p] = sh[0];
}

}  // namespace

void launch_gram_frames(const GramArgs& a, hipStream_t st) {
  const long long rows = (long long)a.nf * a.n_faces;
  const int n_pairs = gram_pairs(a.P), n_slices = gram_slices(a.n_verts);
  const dim3 mix_grid((unsigned)((a.n_verts + 255) / 256), (unsigned)((a.P + kGramMixQ - 1) / kGramMixQ), (unsigned)a.nf);
  if (a.plane) {
    BODYFIT_LAUNCH(k_gram_moments<true>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a);
    BODYFIT_LAUNCH(k_gram_mix<true>, mix_grid, dim3(256), 0, st, a);
  } else {
    BODYFIT_LAUNCH(k_gram_moments<false>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a);
    BODYFIT_LAUNCH(k_gram_mix<false>, mix_grid, dim3(256), 0, st, a);
  }
  BODYFIT_LAUNCH(k_gram_contract, dim3((unsigned)(n_pairs * n_slices), (unsigned)a.nf), dim3(64), 0, st, a, n_pairs, n_slices);
  BODYFIT_LAUNCH(k_gram_fold, dim3((unsigned)((a.P * a.P + 255) / 256), (unsigned)a.nf), dim3(256), 0, st, a, n_pairs, n_slices);
}

void launch_gram_rhs(const float* jac, long long row_floats, long long jac_stride, const float* rhs, long long rhs_stride, int F,
                     int P, int n_verts, double* g, hipStream_t st) {
  BODYFIT_LAUNCH(k_gram_rhs, dim3((unsigned)((long long)F * P)), dim3(256), 0, st, jac, row_floats, jac_stride, rhs, rhs_stride, P,
                 3 * n_verts, g);
}

}  // namespace bodyfit
