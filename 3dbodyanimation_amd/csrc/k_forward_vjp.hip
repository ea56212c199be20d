// k_forward_vjp.hip — reverse-mode gradient (vector-Jacobian product) of the SMPL forward that bodyfit_forward computes:
// given G = dL/dcloud ([F][V][3] f32) and H = dL/djoints ([F][24][3] f64), either optional, dL/dframe_params ([F][76] f64)
// and dL/dbeta.  Host side: bodyfit_forward_vjp_device (api_vjp.hip).
//
// For frame f (frame_part_inl.h, mesh_part_inl.h):
//   T_j     = s Rr0 [A_j | P_j - A_j Jc_j] + [0 | t],  Rr0 = R(rootAA) R0,  A_j = A_par R_j,  P_j = A_par o_j + P_par
//   cloud_v = sum_j W_vj T_j [b_v; 1],  b_v = [feat | beta | 1 1 0..] . [posedirs_v | shapedirs_v - S_root | template_v]
//   joint_j = s Rr0 P_j + t
//
// Stages (all deterministic: no atomics, every sum in a fixed order, every frame's numbers independent of the frame count):
//   0  k_frame_resjac (k_sweep.hip, the two-launch sweep's first kernel) into the VJP's own operand buffers: the frame's
//      blend-coefficient fragments and skinning transforms, exactly what k_mesh_blend_lbs reads
//   a  k_vjp_mesh       one wave per (32-frame tile, 32-vertex tile): the blend recomputed with the forward's own MFMA
//                       sequence on the forward's operand block (so b_v is the forward's, bit for bit), stored for (c);
//      k_vjp_vertex_grad  per (frame, vertex): gb_v = (sum_j W_vj T_j[:, :3])^T G_v, f32, coordinate-major rows.  (Computed
//                       in k_vjp_mesh's waves behind the blend, gb came out different from run to run in a few frames of
//                       the upper half-wave; as a kernel of its own it is bit-stable.)
//   b  k_vjp_blend_t    [dL/dfeat | dL/dbeta_blend] = sum_v [posedirs_v | shapedirs_v - S_root]^T gb_v on the matrix pipe
//                       (bf16 hi/lo, three products, f32 accumulation), one wave per (frame tile, chunk of 9 vertex tiles);
//                       the chunk partials are summed in chunk order by stage d
//   c  k_vjp_skin_t     dL/dT_j = sum_v W_vj G_v [b_v; 1]^T per frame, f64 accumulation over each joint's vertex list
//                       (ascending vertex order)
//   d  k_vjp_chain      one thread per frame, f64: rotations, chain, joint regression recomputed, then the transposed chain,
//                       Rodrigues (both theta^2 branches) and the shape tables; 76 frame gradients and the frame's beta gradient
//   e  k_vjp_beta_sum   shared beta: the per-frame beta gradients summed in a fixed order (64 strided lane sums, butterfly)
// Joints only (no G): stages d and e.
#include <hip/hip_runtime.h>

#include "bodyfit_device.h"
#include "frame_part_inl.h"
#include "mesh_part_inl.h"

namespace bodyfit {

namespace {

constexpr int kVjpKSteps = 6;   // k-steps of stage b per vertex tile: 3 coordinates x 32 vertices = 96 = 6 x 16
constexpr int kVjpNTiles = 7;   // 224 blend columns = 7 MFMA column tiles
constexpr int kVjpCols = kVjpNTiles * 32;
constexpr int kVjpChunkTiles = 9;   // vertex tiles per stage-b wave (216 SMPL tiles: 24 chunks); fixed, so a frame's sum order is too

__device__ __forceinline__ uint4 split_hi_lo8(const float (&x)[8], int hl) {
  uint32_t pk[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint16_t b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const uint16_t hi = f32_to_bf16(x[2 * q + t]);
      b[t] = hl == 0 ? hi : f32_to_bf16(x[2 * q + t] - bf16_to_f32(hi));
    }
    pk[q] = (uint32_t)b[0] | ((uint32_t)b[1] << 16);
  }
  return make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// 32 wait states between the last product and the first read of its accumulators (a margin over the hazard recognizer's own
// padding, which put 12 instructions there; a few hundred cycles per wave).
__device__ __forceinline__ void mfma_drain() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// ---- stage b's B operand: the forward's operand block transposed --------------------------------------------------------
// dirsT[vtile][s][n][hi/lo][64 lanes][8]: lane l holds blend column n * 32 + (l & 31) and the eight contraction entries
// (coordinate s >> 1, vertices 16 (s & 1) + 8 (l >> 5) + e) — the same bf16 hi / lo values as dirsB, re-ordered.
__global__ void k_vjp_build_dirs_t(const uint16_t* __restrict__ dirsB, uint16_t* __restrict__ dirsT, int nVT) {
  const size_t n_out = (size_t)nVT * kVjpKSteps * kVjpNTiles * 2 * 64 * 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
    size_t r = i;
    const int e = (int)(r % 8); r /= 8;
    const int l = (int)(r % 64); r /= 64;
    const int hl = (int)(r % 2); r /= 2;
    const int n = (int)(r % kVjpNTiles); r /= kVjpNTiles;
    const int s = (int)(r % kVjpKSteps); r /= kVjpKSteps;
    const int vt = (int)r;
    const int kk = n * 32 + (l & 31);                     // blend column
    const int c = s >> 1, vcol = 16 * (s & 1) + 8 * (l >> 5) + e;
    // dirsB: [vt][ks = kk >> 4][c][hl][lane = 32 ((kk >> 3) & 1) + vcol][kk & 7]
    const size_t src = (((((size_t)vt * kBlendKSteps + (kk >> 4)) * 3 + c) * 2 + hl) * 64 + 32 * ((kk >> 3) & 1) + vcol) * 8 + (kk & 7);
    dirsT[i] = dirsB[src];
  }
}

// ---- stage a --------------------------------------------------------------------------------------------------------------
struct VjpMeshArgs {
  const uint16_t* dirsB;
  const uint16_t* featA;    // the VJP's own fragments (k_frame_resjac, natural row order)
  const float* skinT;       // [F][24][12]
  const uint32_t* wIdx;
  const float* wVal;
  const float* G;           // caller's [F][row_floats]
  long long row_floats;
  int F, V, nVT;
  float* gbuf;              // [Fp][3][Vp] gb
  float* bbuf;              // [F][Vp][3] blended rest vertices
};

__global__ __launch_bounds__(64) void k_vjp_mesh(VjpMeshArgs a) {
  const int vtile = blockIdx.x, ftile = blockIdx.y;
  const int lane = threadIdx.x, col = lane & 31, h = lane >> 5;
  const int v = vtile * kVTile + col;
  // ---- the blend, as mesh_part_inl.h blend_step issues it: per k-step and coordinate hi.hi, hi.lo, lo.hi ----------------
  const unsigned char* fa = reinterpret_cast<const unsigned char*>(a.featA) + (size_t)ftile * kBlendKSteps * 2048;
  const unsigned char* bb = reinterpret_cast<const unsigned char*>(a.dirsB) + (size_t)vtile * kBBytes;
  f32x16 acc[3];
#pragma unroll
  for (int ks = 0; ks < kBlendKSteps; ++ks) {
    const bf16x8 a_hi = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fa + ks * 2048 + feat_frag_off(lane, 0)));
    const bf16x8 a_lo = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fa + ks * 2048 + feat_frag_off(lane, 1)));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint4* bp = reinterpret_cast<const uint4*>(bb + (size_t)((ks * 3 + c) * 2) * 1024) + lane;
      const bf16x8 bhi = __builtin_bit_cast(bf16x8, bp[0]);
      const bf16x8 blo = __builtin_bit_cast(bf16x8, bp[64]);
      if (ks == 0) {
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.0f;
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, bhi, z, 0, 0, 0);
      } else {
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, bhi, acc[c], 0, 0, 0);
      }
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, blo, acc[c], 0, 0, 0);
      acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, bhi, acc[c], 0, 0, 0);
    }
  }
  // ---- the blended rest vertices of the tile's valid (frame, vertex) pairs, for stage c ---------------------------------
  mfma_drain();
  const size_t Vp = (size_t)a.nVT * kVTile;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int f = ftile * kFTile + 8 * (r >> 2) + 4 * h + (r & 3);   // accumulator register r of half-wave h
    if (f < a.F && v < a.V) {
      float* bo = a.bbuf + ((size_t)f * Vp + v) * 3;
      bo[0] = acc[0][r]; bo[1] = acc[1][r]; bo[2] = acc[2][r];
    }
  }
}

// gb_v = (sum_j W_vj T_j[:, :3])^T G_v per (frame, vertex), f32, [Fp][3][Vp] (zeros on the padding)
__global__ __launch_bounds__(256) void k_vjp_vertex_grad(VjpMeshArgs a) {
  const size_t Vp = (size_t)a.nVT * kVTile;
  const int v = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (v >= (int)Vp) return;
  float gb0 = 0.0f, gb1 = 0.0f, gb2 = 0.0f;
  if (f < a.F && v < a.V) {
    const uint32_t widx = a.wIdx[v];
    const float4 wv = reinterpret_cast<const float4*>(a.wVal)[v];
    const float wgt[4] = {wv.x, wv.y, wv.z, wv.w};
    float Mx[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Mx[e] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4* T = reinterpret_cast<const float4*>(a.skinT + ((size_t)f * kMaxJoints + ((widx >> (8 * i)) & 0xffu)) * 12);
      const float4 t0 = T[0], t1 = T[1], t2 = T[2];
      const float tv[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
#pragma unroll
      for (int e = 0; e < 12; ++e) Mx[e] += wgt[i] * tv[e];
    }
    const float* g = a.G + (size_t)f * a.row_floats + (size_t)v * 3;
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    gb0 = Mx[0] * g0 + Mx[4] * g1 + Mx[8] * g2;
    gb1 = Mx[1] * g0 + Mx[5] * g1 + Mx[9] * g2;
    gb2 = Mx[2] * g0 + Mx[6] * g1 + Mx[10] * g2;
  }
  float* go = a.gbuf + ((size_t)f * 3) * Vp + v;
  go[0] = gb0; go[Vp] = gb1; go[2 * Vp] = gb2;
}

// ---- stage b --------------------------------------------------------------------------------------------------------------
// One wave per (frame tile, chunk of kVjpChunkTiles vertex tiles): out[chunk][f][224].
__global__ __launch_bounds__(64) void k_vjp_blend_t(const float* __restrict__ gbuf, const uint16_t* __restrict__ dirsT,
                                                    float* __restrict__ part, int nVT, int Fp) {
  const int ftile = blockIdx.x, chunk = blockIdx.y;
  const int lane = threadIdx.x;
  const int vt0 = chunk * kVjpChunkTiles, vt1 = min(vt0 + kVjpChunkTiles, nVT);
  const size_t Vp = (size_t)nVT * kVTile;
  f32x16 acc[kVjpNTiles];
#pragma unroll
  for (int n = 0; n < kVjpNTiles; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.0f;
  // A fragment of k-step s: frame row lane & 31, gb[coordinate s >> 1] of vertices 16 (s & 1) + 8 (lane >> 5) + 0..7
  const float* ga = gbuf + ((size_t)(ftile * kFTile + (lane & 31)) * 3) * Vp + 8 * (lane >> 5);
  const unsigned char* bb = reinterpret_cast<const unsigned char*>(dirsT);
  for (int vt = vt0; vt < vt1; ++vt) {
#pragma unroll 2
    for (int s = 0; s < kVjpKSteps; ++s) {
      const size_t ks = (size_t)vt * kVjpKSteps + s;
      const float4* gp = reinterpret_cast<const float4*>(ga + (size_t)(s >> 1) * Vp + (size_t)vt * kVTile + 16 * (s & 1));
      const float4 g0 = gp[0], g1 = gp[1];
      const float x[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const bf16x8 a_hi = __builtin_bit_cast(bf16x8, split_hi_lo8(x, 0));
      const bf16x8 a_lo = __builtin_bit_cast(bf16x8, split_hi_lo8(x, 1));
#pragma unroll
      for (int n = 0; n < kVjpNTiles; ++n) {
        const uint4* bp = reinterpret_cast<const uint4*>(bb + (ks * kVjpNTiles + n) * 2048) + lane;
        const bf16x8 bhi = __builtin_bit_cast(bf16x8, bp[0]);
        const bf16x8 blo = __builtin_bit_cast(bf16x8, bp[64]);
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, bhi, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, blo, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, bhi, acc[n], 0, 0, 0);
      }
    }
  }
  mfma_drain();
  const int col = lane & 31, h = lane >> 5;
  float* o = part + ((size_t)chunk * Fp + (size_t)ftile * kFTile) * kVjpCols;
#pragma unroll
  for (int n = 0; n < kVjpNTiles; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(size_t)(8 * (r >> 2) + 4 * h + (r & 3)) * kVjpCols + n * 32 + col] = acc[n][r];
}

// ---- stage c --------------------------------------------------------------------------------------------------------------
// One workgroup per frame; thread (joint j, row a): dT_j[a][0..3] = sum over j's vertices (ascending) of w G_v[a] [b_v; 1].
__global__ __launch_bounds__(128) void k_vjp_skin_t(const int* __restrict__ csr_off, const int* __restrict__ csr_v,
                                                    const float* __restrict__ csr_w, const float* __restrict__ G,
                                                    long long row_floats, const float* __restrict__ bbuf, int Vp,
                                                    double* __restrict__ dT) {
  const int f = blockIdx.x, t = threadIdx.x;
  if (t >= 3 * kMaxJoints) return;
  const int j = t / 3, ar = t % 3;
  const float* g = G + (size_t)f * row_floats;
  const float* b = bbuf + (size_t)f * Vp * 3;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int i = csr_off[j]; i < csr_off[j + 1]; ++i) {
    const int v = csr_v[i];
    const double wg = (double)csr_w[i] * (double)g[(size_t)v * 3 + ar];
    s0 += wg * (double)b[(size_t)v * 3];
    s1 += wg * (double)b[(size_t)v * 3 + 1];
    s2 += wg * (double)b[(size_t)v * 3 + 2];
    s3 += wg;
  }
  double* o = dT + ((size_t)f * kMaxJoints + j) * 12 + ar * 4;
  o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
}

// ---- stage d --------------------------------------------------------------------------------------------------------------
struct VjpChainArgs {
  DevModel M;
  int F, use_shape, beta_stride, pose_blend;
  const double* params;     // [F(+1)][npose], npose = 7 + 3 (nJ - 1)
  const double* beta;       // may be null (zeros)
  const double* R0;         // [F][9]
  const double* dT;         // [F][24][12] or null
  const float* part;        // [n_chunks][Fp][224] or null
  int n_chunks, Fp;
  const double* H;          // [F][nJ][3] or null
  double* gx;               // [F][npose]
  double* gbeta;            // [F][nS] (per frame, or the shared sum's inputs); may be null
};

__device__ inline void rot_grad(const double* a, const double* gR, double* out) {   // out_k = <gR, dR/da_k>
  for (int k = 0; k < 3; ++k) {
    double R[9], dR[9];
    rodrigues_grad_k(a[0], a[1], a[2], k, R, dR);
    double s = 0.0;
    for (int e = 0; e < 9; ++e) s += gR[e] * dR[e];
    out[k] = s;
  }
}

__global__ __launch_bounds__(64) void k_vjp_chain(VjpChainArgs a) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.F) return;
  const DevModel& M = a.M;
  const int nJ = M.nJ, nS = M.nS, npose = 7 + 3 * (nJ - 1);
  const double* x = a.params + (size_t)f * npose;
  const bool shp = a.use_shape && nS > 0;                  // (no beta given: the forward's beta = 0)
  double beta[kMaxShape];
  for (int k = 0; k < kMaxShape; ++k) beta[k] = (shp && a.beta && k < nS) ? a.beta[(size_t)f * a.beta_stride + k] : 0.0;
  const double s = x[0];
  double R[kMaxJoints][9], A[kMaxJoints][9], P[kMaxJoints][3], o[kMaxJoints][3], Jc[kMaxJoints][3];
  double Rroot[9], dummy[9], Rr0[9];
  rodrigues_grad_k(x[1], x[2], x[3], 0, Rroot, dummy);
  mul33(Rroot, a.R0 + (size_t)f * 9, Rr0);
  for (int j = 0; j < nJ; ++j) {
    if (j > 0) rodrigues_grad_k(x[7 + 3 * (j - 1)], x[8 + 3 * (j - 1)], x[9 + 3 * (j - 1)], 0, R[j], dummy);
    for (int c = 0; c < 3; ++c) {
      double ov = M.offset[j * 3 + c], jc = M.Jc0[j * 3 + c];
      for (int k = 0; k < nS; ++k) {
        ov += M.dS[(j * 3 + c) * nS + k] * beta[k];
        jc += M.Sc[(j * 3 + c) * nS + k] * beta[k];
      }
      o[j][c] = j == 0 ? 0.0 : ov;
      Jc[j][c] = jc;
    }
  }
  for (int e = 0; e < 9; ++e) A[0][e] = (e % 4 == 0) ? 1.0 : 0.0;
  P[0][0] = P[0][1] = P[0][2] = 0.0;
  for (int i = 0; i < M.level_off[M.nLevels]; ++i) {       // parents before children
    const int j = M.level_joint[i], p = M.parent[j];
    mul33(A[p], R[j], A[j]);
    double q[3];
    mv3(A[p], o[j][0], o[j][1], o[j][2], q);
    for (int c = 0; c < 3; ++c) P[j][c] = q[c] + P[p][c];
  }
  // ---- gradients of the outputs w.r.t. s, t, Rr0, A_j, P_j, Jc_j ----------------------------------------------------
  double gs = 0.0, gt[3] = {0, 0, 0}, gRr0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double gA[kMaxJoints][9], gP[kMaxJoints][3], gR[kMaxJoints][9];
  double gb[kMaxShape];
  for (int k = 0; k < kMaxShape; ++k) gb[k] = 0.0;
  for (int j = 0; j < nJ; ++j) {
    for (int e = 0; e < 9; ++e) { gA[j][e] = 0.0; gR[j][e] = 0.0; }
    gP[j][0] = gP[j][1] = gP[j][2] = 0.0;
  }
  if (a.H) {
    const double* Hf = a.H + (size_t)f * nJ * 3;
    for (int j = 0; j < nJ; ++j) {
      const double h0 = Hf[j * 3], h1 = Hf[j * 3 + 1], h2 = Hf[j * 3 + 2];
      double q[3];
      mv3(Rr0, P[j][0], P[j][1], P[j][2], q);
      gs += h0 * q[0] + h1 * q[1] + h2 * q[2];
      gt[0] += h0; gt[1] += h1; gt[2] += h2;
      const double hv[3] = {h0, h1, h2};
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) gRr0[r * 3 + c] += s * hv[r] * P[j][c];
      for (int c = 0; c < 3; ++c) gP[j][c] += s * (Rr0[c] * h0 + Rr0[3 + c] * h1 + Rr0[6 + c] * h2);
    }
  }
  if (a.dT) {
    const double* D = a.dT + (size_t)f * kMaxJoints * 12;
    for (int j = 0; j < nJ; ++j) {
      const double* Dj = D + j * 12;                       // row r: [dT[r][0..2] | dT[r][3]]
      double aj[3];
      mv3(A[j], Jc[j][0], Jc[j][1], Jc[j][2], aj);
      const double u[3] = {P[j][0] - aj[0], P[j][1] - aj[1], P[j][2] - aj[2]};   // P_j - A_j Jc_j
      double MA[9], mu[3];
      mul33(Rr0, A[j], MA);
      mv3(Rr0, u[0], u[1], u[2], mu);
      const double d[3] = {Dj[3], Dj[7], Dj[11]};
      for (int r = 0; r < 3; ++r) {
        gt[r] += d[r];
        gs += Dj[r * 4] * MA[r * 3] + Dj[r * 4 + 1] * MA[r * 3 + 1] + Dj[r * 4 + 2] * MA[r * 3 + 2] + d[r] * mu[r];
        for (int c = 0; c < 3; ++c)
          gRr0[r * 3 + c] += s * (Dj[r * 4] * A[j][c * 3] + Dj[r * 4 + 1] * A[j][c * 3 + 1] + Dj[r * 4 + 2] * A[j][c * 3 + 2] +
                                  d[r] * u[c]);
      }
      double rt[3];                                        // Rr0^T d
      for (int c = 0; c < 3; ++c) rt[c] = Rr0[c] * d[0] + Rr0[3 + c] * d[1] + Rr0[6 + c] * d[2];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          const double rd = Rr0[r] * Dj[c] + Rr0[3 + r] * Dj[4 + c] + Rr0[6 + r] * Dj[8 + c];   // (Rr0^T DA)[r][c]
          gA[j][r * 3 + c] += s * (rd - rt[r] * Jc[j][c]);
        }
      for (int c = 0; c < 3; ++c) gP[j][c] += s * rt[c];
      if (shp) {
        double gJc[3];                                     // -s A_j^T Rr0^T d
        for (int c = 0; c < 3; ++c) gJc[c] = -s * (A[j][c] * rt[0] + A[j][3 + c] * rt[1] + A[j][6 + c] * rt[2]);
        for (int k = 0; k < nS; ++k)
          gb[k] += M.Sc[(j * 3) * nS + k] * gJc[0] + M.Sc[(j * 3 + 1) * nS + k] * gJc[1] + M.Sc[(j * 3 + 2) * nS + k] * gJc[2];
      }
    }
  }
  if (a.part) {   // blend gradients: the chunk partials in chunk order
    const int nfeat = 9 * (nJ - 1);
    for (int k = 0; k < kPoseFeat + kMaxShape; ++k) {
      const bool pose = k < kPoseFeat;
      if (pose ? !(a.pose_blend && k < nfeat) : !(shp && k - kPoseFeat < nS)) continue;
      double g = 0.0;
      for (int ch = 0; ch < a.n_chunks; ++ch) g += (double)a.part[((size_t)ch * a.Fp + f) * kVjpCols + k];
      if (pose) gR[1 + k / 9][k % 9] += g;
      else gb[k - kPoseFeat] += g;
    }
  }
  // ---- back through the chain, children before parents ----------------------------------------------------------------
  for (int i = M.level_off[M.nLevels] - 1; i >= 0; --i) {
    const int j = M.level_joint[i], p = M.parent[j];
    // A_j = A_p R_j: gR_j += A_p^T gA_j, gA_p += gA_j R_j^T;  P_j = A_p o_j + P_p: go_j = A_p^T gP_j, gA_p += gP_j o_j^T
    double go[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        gR[j][r * 3 + c] += A[p][r] * gA[j][c] + A[p][3 + r] * gA[j][3 + c] + A[p][6 + r] * gA[j][6 + c];
      go[r] = A[p][r] * gP[j][0] + A[p][3 + r] * gP[j][1] + A[p][6 + r] * gP[j][2];
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        gA[p][r * 3 + c] += gA[j][r * 3] * R[j][c * 3] + gA[j][r * 3 + 1] * R[j][c * 3 + 1] + gA[j][r * 3 + 2] * R[j][c * 3 + 2] +
                            gP[j][r] * o[j][c];
    for (int c = 0; c < 3; ++c) gP[p][c] += gP[j][c];
    if (shp)
      for (int k = 0; k < nS; ++k)
        gb[k] += M.dS[(j * 3) * nS + k] * go[0] + M.dS[(j * 3 + 1) * nS + k] * go[1] + M.dS[(j * 3 + 2) * nS + k] * go[2];
  }
  // ---- out --------------------------------------------------------------------------------------------------------------
  double* g = a.gx + (size_t)f * npose;
  g[0] = gs;
  double gRroot[9];                                        // Rr0 = Rroot R0: gRroot = gRr0 R0^T
  mul33_bt(gRr0, a.R0 + (size_t)f * 9, gRroot);
  rot_grad(x + 1, gRroot, g + 1);
  g[4] = gt[0]; g[5] = gt[1]; g[6] = gt[2];
  for (int j = 1; j < nJ; ++j) rot_grad(x + 7 + 3 * (j - 1), gR[j], g + 7 + 3 * (j - 1));
  if (a.gbeta)
    for (int k = 0; k < nS; ++k) a.gbeta[(size_t)f * nS + k] = gb[k];
}

// ---- stage e ----------------------------------------------------------------------------------------------------------------
// One wave per shape coefficient: lane l sums frames l, l + 64, ... in order, then a fixed butterfly over the lanes.
__global__ __launch_bounds__(64) void k_vjp_beta_sum(const double* __restrict__ gbf, int F, int nS, double* __restrict__ out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int f = lane; f < F; f += 64) s += gbf[(size_t)f * nS + k];
  s = wave_sum(s);
  if (lane == 0) out[k] = s;
}

}  // namespace

size_t vjp_dirs_t_elems(int nVT) { return (size_t)nVT * kVjpKSteps * kVjpNTiles * 2 * 64 * 8; }
size_t vjp_gb_elems(int nFT, int nVT) { return (size_t)nFT * kFTile * 3 * nVT * kVTile; }
int vjp_n_chunks(int nVT) { return (nVT + kVjpChunkTiles - 1) / kVjpChunkTiles; }
size_t vjp_part_elems(int nFT, int nVT) { return (size_t)vjp_n_chunks(nVT) * nFT * kFTile * kVjpCols; }

void launch_vjp_build_dirs_t(const DevModel& M, uint16_t* d_dirsT, hipStream_t s) {
  BODYFIT_LAUNCH(k_vjp_build_dirs_t, dim3(1024), dim3(256), 0, s, M.dirsB, d_dirsT, M.nVTiles);
}

void launch_vjp_mesh(const DevModel& M, const DevProblem& P, const MeshCoef& mc, const float* d_G, long long row_floats,
                     float* d_gb, float* d_bbuf, hipStream_t s) {
  VjpMeshArgs a;
  a.dirsB = M.dirsB; a.featA = mc.featA; a.skinT = mc.skinT; a.wIdx = M.wIdx; a.wVal = M.wVal;
  a.G = d_G; a.row_floats = row_floats; a.F = P.F; a.V = M.V; a.nVT = M.nVTiles; a.gbuf = d_gb; a.bbuf = d_bbuf;
  BODYFIT_LAUNCH(k_vjp_mesh, dim3(M.nVTiles, P.nFTiles), dim3(64), 0, s, a);
  BODYFIT_LAUNCH(k_vjp_vertex_grad, dim3((M.nVTiles * kVTile + 255) / 256, P.nFTiles * kFTile), dim3(256), 0, s, a);
}

void launch_vjp_blend_t(const DevModel& M, const DevProblem& P, const float* d_gb, const uint16_t* d_dirsT, float* d_part,
                        hipStream_t s) {
  BODYFIT_LAUNCH(k_vjp_blend_t, dim3(P.nFTiles, vjp_n_chunks(M.nVTiles)), dim3(64), 0, s, d_gb, d_dirsT, d_part, M.nVTiles,
                 P.nFTiles * kFTile);
}

void launch_vjp_skin_t(const DevModel& M, const DevProblem& P, const int* d_csr_off, const int* d_csr_v, const float* d_csr_w,
                       const float* d_G, long long row_floats, const float* d_bbuf, double* d_dT, hipStream_t s) {
  BODYFIT_LAUNCH(k_vjp_skin_t, dim3(P.F), dim3(128), 0, s, d_csr_off, d_csr_v, d_csr_w, d_G, row_floats, d_bbuf,
                 M.nVTiles * kVTile, d_dT);
}

void launch_vjp_chain(const DevModel& M, const DevProblem& P, const double* d_params, const double* d_beta, const double* d_dT,
                      const float* d_part, const double* d_H, double* d_gx, double* d_gbeta_frames, hipStream_t s) {
  VjpChainArgs a;
  a.M = M; a.F = P.F; a.use_shape = P.use_shape; a.beta_stride = P.beta_stride; a.pose_blend = P.pose_blend;
  a.params = d_params; a.beta = d_beta; a.R0 = P.R0; a.dT = d_dT; a.part = d_part;
  a.n_chunks = vjp_n_chunks(M.nVTiles); a.Fp = P.nFTiles * kFTile; a.H = d_H; a.gx = d_gx; a.gbeta = d_gbeta_frames;
  BODYFIT_LAUNCH(k_vjp_chain, dim3((P.F + 63) / 64), dim3(64), 0, s, a);
}

void launch_vjp_beta_sum(const double* d_gbeta_frames, int F, int nS, double* d_out, hipStream_t s) {
  if (nS > 0) BODYFIT_LAUNCH(k_vjp_beta_sum, dim3(nS), dim3(64), 0, s, d_gbeta_frames, F, nS, d_out);
}

}  // namespace bodyfit
