// k_forward_jvp.hip — forward-mode tangents (Jacobian-vector products) of the SMPL forward that bodyfit_forward_device computes,
// for K tangents per frame at once: given (xdot_fk, betadot_k) the directional derivatives jointsdot [F][K][nJ][3] (f64) and
// clouddot [F][K][row_floats] (f32).  Host side: bodyfit_forward_jvp_device (api_jvp.hip).  Notation: k_forward_vjp.hip.
//
//   T_j     = s Rr0 [A_j | u_j] + [0 | t],  u_j = P_j - A_j Jc_j,  Rr0 = R(rootAA) R0,  A_j = A_par R_j,  P_j = A_par o_j + P_par
//   Tdot_j  = M [A_j | u_j] + N [Adot_j | udot_j] + [0 | tdot],  M = sdot Rr0 + s Rr0dot,  N = s Rr0
//   cloud_v = sum_j W_vj T_j [b_v; 1]   ->   clouddot_v = sum_j W_vj (Tdot_j [b_v; 1] + T_j[:, :3] bdot_v)
//   bdot_v  = [featdot | betadot | 0 0 ..] . [posedirs_v | shapedirs_v - S_root | template_v],  featdot = vec(Rdot_j), j >= 1
//
// Stages (deterministic: no atomics, every sum in a fixed order; the numbers of a (frame, tangent) pair depend on that pair only):
//   0  k_frame_resjac (k_sweep.hip) into the JVP's own operand buffers: the frame's blend-coefficient fragments and f32
//      skinning transforms, exactly what k_mesh_blend_lbs reads                                          (once per call)
//   a  k_jvp_blend      one wave per (32-frame tile, 32-vertex tile): the primal b_v recomputed with the forward's MFMA
//                       sequence on the forward's operand block, stored [F][Vp][3]                        (once per call)
//   then per tile of 32 tangents (host loop: the scratch holds ONE tangent tile per frame):
//   b  k_jvp_chain      one wave per (frame, tangent tile), f64.  The primal chain once per workgroup with the joints on the
//                       lanes (Rodrigues and its three partial derivatives per joint, both theta^2 branches; shape tables;
//                       the walk), then one lane per tangent: Rdot_j = sum_c dR_j/da_c adot_c, Adot_j, Pdot_j, the beta
//                       dependence of o_j and Jc_j, root and scale.  Out: jointsdot, Tdot (f32, [F][32][24][12]) and the tangent's
//                       blend coefficients as MFMA A fragments (bf16 hi / lo, the forward's fragment layout with the tangents
//                       where the forward has frames)
//   c  k_jvp_blend      again, on those fragments: one wave per (frame, vertex tile), bdot by the forward's sequence (hi.hi +
//                       hi.lo + lo.hi per k-step, f32 accumulation) on the model's operand block as it is, 32 wait states, the
//                       accumulators stored [F][32][Vp][3]
//   d  k_jvp_skin       one thread per (frame, vertex), the frame's Tdot tile in LDS: the skinning tangent of the tile's tangents
//                       in turn, f32, one 12-byte store per (frame, tangent, vertex), coalesced along the vertices
// (c and d fused into one wave, the skinning tangent applied to the accumulators in registers, was not bit-stable: the rows of
// the upper half-wave changed from run to run, as DESIGN section 5 records for the VJP; the split form is.)
// Joints only (no clouddot): stage b alone, all tangent tiles in one grid, nothing written to scratch.
#include <hip/hip_runtime.h>

#include "bodyfit_device.h"
#include "frame_part_inl.h"
#include "mesh_part_inl.h"

namespace bodyfit {

namespace {

constexpr int kJvpTile = 32;                           // tangents per tile: the MFMA rows
constexpr int kJvpCoef = kBlendKSteps * 16;            // 224 blend coefficients
constexpr int kJvpCoefLd = kJvpCoef + 1;               // LDS row stride (floats) of a tangent's coefficients
constexpr int kJvpTdotFloats = kJvpTile * kMaxJoints * 12;   // one frame's Tdot tile: 9,216 floats

// 32 wait states between the last product and the first read of its accumulators (as k_forward_vjp.hip)
__device__ __forceinline__ void jvp_mfma_drain() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// The forward's blend of one (row tile, vertex tile): fa = the row tile's 14 A-fragment blocks (28 KiB), bb = the vertex tile's
// operands (kBBytes), both wave-uniform.  Raw buffer loads: the lane offset is ONE register and every fragment's offset a scalar,
// so no vector instruction sits between the products (plain pointers cost a 64-bit vector add per load, and hipcc put the sums
// into registers a product issued just before had read).
__device__ __forceinline__ void jvp_blend(const void* fa, const void* bb, int lane, f32x16 (&acc)[3]) {
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(fa), 0, kBlendKSteps * 2048, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(bb), 0, kBBytes, 0x00020000);
  const unsigned lo = (unsigned)lane * 16u;
#pragma unroll
  for (int ks = 0; ks < kBlendKSteps; ++ks) {
    const bf16x8 a_hi = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, lo, ks * 2048, 0));
    const bf16x8 a_lo = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, lo, ks * 2048 + 1024, 0));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int so = ((ks * 3 + c) * 2) * 1024;
      const bf16x8 bhi = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rb, lo, so, 0));
      const bf16x8 blo = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rb, lo, so + 1024, 0));
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
}

// ---- stages a and c: the blend of one (row tile, vertex tile), rows stored [row][Vp][3] -------------------------------------
// One wave per tile, nothing in it but the products and the stores of their accumulators.  Row tile t holds rows 32 t .. 32 t + 31
// (primal: frames; tangents: the 32 tangents of frame t), of which the first n_act are stored, and none past n_rows.
__global__ __launch_bounds__(64) void k_jvp_blend(const uint16_t* __restrict__ dirsB, const uint16_t* __restrict__ feat,
                                                  int n_rows, int n_act, int V, int nVT, float* __restrict__ out) {
  const int vtile = blockIdx.x, tile = blockIdx.y;
  const int lane = threadIdx.x, col = lane & 31, h = lane >> 5;
  const int v = vtile * kVTile + col;
  f32x16 acc[3];
  __builtin_amdgcn_sched_barrier(0);
  jvp_blend(reinterpret_cast<const unsigned char*>(feat) + (size_t)tile * kBlendKSteps * 2048,
            reinterpret_cast<const unsigned char*>(dirsB) + (size_t)vtile * kBBytes, lane, acc);
  jvp_mfma_drain();
  const size_t Vp = (size_t)nVT * kVTile;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 8 * (r >> 2) + 4 * h + (r & 3);        // accumulator register r of half-wave h
    if (row < n_act && tile * kJvpTile + row < n_rows && v < V) {
      float* bo = out + ((size_t)(tile * kJvpTile + row) * Vp + v) * 3;
      bo[0] = acc[0][r]; bo[1] = acc[1][r]; bo[2] = acc[2][r];
    }
  }
}

// ---- stage b --------------------------------------------------------------------------------------------------------------
struct JvpChainArgs {
  DevModel M;
  int F, K, k0;             // tangents k0 + 32 blockIdx.x + (0..31) of frame blockIdx.y
  int use_shape, beta_stride, pose_blend, tan_beta_per_frame;
  const double* params;     // [F(+1)][npose]
  const double* beta;       // may be null (zeros)
  const double* R0;         // [F][9]
  const double* tan_params; // [F][K][npose] or null (zeros)
  const double* tan_beta;   // [K][nS] or [F][K][nS], or null (zeros)
  double* tan_joints;       // [F][K][nJ][3] or null
  float* tdot;              // [F][32][24][12] or null (joints only)
  uint16_t* featD;          // [F][kBlendKSteps][2 hi/lo][64][8] or null (joints only)
};

__global__ __launch_bounds__(64) void k_jvp_chain(JvpChainArgs a) {
  __shared__ double sR[kMaxJoints * 9], sdR[kMaxJoints * 27], sO[kMaxJoints * 3], sJc[kMaxJoints * 3];
  __shared__ double sA[kMaxJoints * 9], sP[kMaxJoints * 3], sRr0[9];
  __shared__ float sCf[kJvpTile * kJvpCoefLd];
  const DevModel& M = a.M;
  const int f = blockIdx.y, lane = threadIdx.x;
  const int nJ = M.nJ, nS = M.nS, npose = 7 + 3 * (nJ - 1);
  const double* x = a.params + (size_t)f * npose;
  const bool shp = a.use_shape && nS > 0;
  const bool mesh = a.featD != nullptr;
  // ---- the primal chain, once per workgroup: (joint, axis) and (joint, coordinate) items on the lanes --------------------
  for (int it = lane; it < 3 * nJ; it += 64) {
    const int jj = it / 3, c = it - 3 * jj;
    const double* aa = (jj == 0) ? (x + 1) : (x + 7 + 3 * (jj - 1));
    double R[9], dRc[9];
    rodrigues_grad_k(aa[0], aa[1], aa[2], c, R, dRc);
    if (c == 0)
      for (int e = 0; e < 9; ++e) sR[jj * 9 + e] = R[e];
    for (int e = 0; e < 9; ++e) sdR[jj * 27 + c * 9 + e] = dRc[e];
    double ov = M.offset[it], jc = M.Jc0[it];
    if (shp && a.beta)
      for (int k = 0; k < nS; ++k) {
        const double bk = a.beta[(size_t)f * a.beta_stride + k];
        ov += M.dS[it * nS + k] * bk;
        jc += M.Sc[it * nS + k] * bk;
      }
    sO[it] = jj == 0 ? 0.0 : ov;
    sJc[it] = jc;
  }
  if (mesh)
    for (int i = lane; i < kJvpTile * kJvpCoefLd; i += 64) sCf[i] = 0.0f;
  __syncthreads();
  if (lane == 0) {
    mul33(sR, a.R0 + (size_t)f * 9, sRr0);               // (sR[0..8]: the root rotation)
    for (int e = 0; e < 9; ++e) sA[e] = (e % 4 == 0) ? 1.0 : 0.0;
    sP[0] = sP[1] = sP[2] = 0.0;
    for (int i = 0; i < M.level_off[M.nLevels]; ++i) {   // parents before children
      const int j = M.level_joint[i], p = M.parent[j];
      mul33(sA + p * 9, sR + j * 9, sA + j * 9);
      double q[3];
      mv3(sA + p * 9, sO[j * 3], sO[j * 3 + 1], sO[j * 3 + 2], q);
      for (int c = 0; c < 3; ++c) sP[j * 3 + c] = q[c] + sP[p * 3 + c];
    }
  }
  __syncthreads();
  // ---- one lane per tangent -------------------------------------------------------------------------------------------
  const int k = a.k0 + blockIdx.x * kJvpTile + lane;
  if (lane < kJvpTile && k < a.K) {
    const double* tx = a.tan_params ? a.tan_params + ((size_t)f * a.K + k) * npose : nullptr;
    const double* tb = (shp && a.tan_beta) ? a.tan_beta + (a.tan_beta_per_frame ? ((size_t)f * a.K + k) : (size_t)k) * nS : nullptr;
    double bd[kMaxShape];
    for (int i = 0; i < kMaxShape; ++i) bd[i] = (tb && i < nS) ? tb[i] : 0.0;
    const double s = x[0], sd = tx ? tx[0] : 0.0;
    const double td[3] = {tx ? tx[4] : 0.0, tx ? tx[5] : 0.0, tx ? tx[6] : 0.0};
    // M = sdot Rr0 + s Rr0dot, N = s Rr0;  Rr0dot = (sum_c dRroot/da_c adot_c) R0
    double Mm[9], Nm[9];
    {
      double Rd[9], Rr0d[9];
      for (int e = 0; e < 9; ++e)
        Rd[e] = tx ? sdR[e] * tx[1] + sdR[9 + e] * tx[2] + sdR[18 + e] * tx[3] : 0.0;
      mul33(Rd, a.R0 + (size_t)f * 9, Rr0d);
      for (int e = 0; e < 9; ++e) {
        Mm[e] = sd * sRr0[e] + s * Rr0d[e];
        Nm[e] = s * sRr0[e];
      }
    }
    double Ad[kMaxJoints][9], Pd[kMaxJoints][3];
    for (int e = 0; e < 9; ++e) Ad[0][e] = 0.0;
    Pd[0][0] = Pd[0][1] = Pd[0][2] = 0.0;
    float* cf = sCf + lane * kJvpCoefLd;
    const int n_walk = M.level_off[M.nLevels];
    for (int i = -1; i < n_walk; ++i) {                   // the root first, then parents before children
      const int j = i < 0 ? 0 : M.level_joint[i];
      if (i >= 0) {
        const int p = M.parent[j];
        double Rd[9], od[3] = {0.0, 0.0, 0.0};
        const double* dRj = sdR + j * 27;
        const double* ad = tx ? tx + 7 + 3 * (j - 1) : nullptr;
        for (int e = 0; e < 9; ++e) Rd[e] = ad ? dRj[e] * ad[0] + dRj[9 + e] * ad[1] + dRj[18 + e] * ad[2] : 0.0;
        if (mesh && a.pose_blend)
          for (int e = 0; e < 9; ++e) cf[9 * (j - 1) + e] = (float)Rd[e];
        if (tb)
          for (int c = 0; c < 3; ++c)
            for (int q = 0; q < nS; ++q) od[c] += M.dS[(j * 3 + c) * nS + q] * bd[q];
        // Adot_j = Adot_p R_j + A_p Rdot_j;  Pdot_j = Adot_p o_j + A_p odot_j + Pdot_p
        double t0[9], t1[9], q0[3], q1[3];
        mul33(Ad[p], sR + j * 9, t0);
        mul33(sA + p * 9, Rd, t1);
        for (int e = 0; e < 9; ++e) Ad[j][e] = t0[e] + t1[e];
        mv3(Ad[p], sO[j * 3], sO[j * 3 + 1], sO[j * 3 + 2], q0);
        mv3(sA + p * 9, od[0], od[1], od[2], q1);
        for (int c = 0; c < 3; ++c) Pd[j][c] = q0[c] + q1[c] + Pd[p][c];
      }
      const double* Aj = sA + j * 9;
      const double* Pj = sP + j * 3;
      if (a.tan_joints) {
        double q0[3], q1[3];
        mv3(Mm, Pj[0], Pj[1], Pj[2], q0);
        mv3(Nm, Pd[j][0], Pd[j][1], Pd[j][2], q1);
        double* o = a.tan_joints + (((size_t)f * a.K + k) * nJ + j) * 3;
        for (int c = 0; c < 3; ++c) o[c] = q0[c] + q1[c] + td[c];
      }
      if (mesh) {
        double jcd[3] = {0.0, 0.0, 0.0};
        if (tb)
          for (int c = 0; c < 3; ++c)
            for (int q = 0; q < nS; ++q) jcd[c] += M.Sc[(j * 3 + c) * nS + q] * bd[q];
        double aj[3], adj[3], ajd[3];
        mv3(Aj, sJc[j * 3], sJc[j * 3 + 1], sJc[j * 3 + 2], aj);
        mv3(Ad[j], sJc[j * 3], sJc[j * 3 + 1], sJc[j * 3 + 2], adj);
        mv3(Aj, jcd[0], jcd[1], jcd[2], ajd);
        const double u[3] = {Pj[0] - aj[0], Pj[1] - aj[1], Pj[2] - aj[2]};
        const double ud[3] = {Pd[j][0] - adj[0] - ajd[0], Pd[j][1] - adj[1] - ajd[1], Pd[j][2] - adj[2] - ajd[2]};
        double MA[9], NA[9], mu[3], nu[3];
        mul33(Mm, Aj, MA);
        mul33(Nm, Ad[j], NA);
        mv3(Mm, u[0], u[1], u[2], mu);
        mv3(Nm, ud[0], ud[1], ud[2], nu);
        float4* T = reinterpret_cast<float4*>(a.tdot + (((size_t)f * kJvpTile + lane) * kMaxJoints + j) * 12);
        for (int r = 0; r < 3; ++r)
          T[r] = make_float4((float)(MA[r * 3] + NA[r * 3]), (float)(MA[r * 3 + 1] + NA[r * 3 + 1]),
                             (float)(MA[r * 3 + 2] + NA[r * 3 + 2]), (float)(mu[r] + nu[r] + td[r]));
      }
    }
    if (mesh)
      for (int q = 0; q < nS; ++q) cf[kPoseFeat + q] = (float)bd[q];
  }
  if (!mesh) return;
  __syncthreads();
  // ---- the tile's coefficients as A fragments: row = tangent, the forward's [ks][hi | lo][k-half][row][8] ----------------
  unsigned char* fd = reinterpret_cast<unsigned char*>(a.featD) + (size_t)f * kBlendKSteps * 2048;
  for (int i = lane; i < kJvpTile * kBlendKSteps * 4; i += 64) {
    const int row = i & 31, h = (i >> 5) & 1, hl = (i >> 6) & 1, ks = i >> 7;
    const float* c = sCf + row * kJvpCoefLd + ks * 16 + 8 * h;
    uint32_t pk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint16_t b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float xv = c[2 * q + t];
        const uint16_t hi = f32_to_bf16(xv);
        b[t] = hl == 0 ? hi : f32_to_bf16(xv - bf16_to_f32(hi));
      }
      pk[q] = (uint32_t)b[0] | ((uint32_t)b[1] << 16);
    }
    *reinterpret_cast<uint4*>(fd + ks * 2048 + feat_frag_off(h * 32 + row, hl)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
  }
}

// ---- stage d --------------------------------------------------------------------------------------------------------------
struct JvpSkinArgs {
  const float* tdot;        // [F][32][24][12]
  const float* skinT;       // [F][24][12] primal transforms (k_frame_resjac)
  const float* bbuf;        // [F][Vp][3] primal blended rest vertices
  const float* dbuf;        // [F][32][Vp][3] their tangents
  const uint32_t* wIdx;
  const float* wVal;
  int F, K, k0, V, nVT;
  float* out;               // caller's [F][K][row_floats]
  long long row_floats;
};

struct __attribute__((packed, aligned(4))) JvpF3 { float x, y, z; };

// One workgroup per (frame, 256 vertices): the frame's Tdot tile in LDS, one thread per vertex, the tile's tangents in turn.
__global__ __launch_bounds__(256) void k_jvp_skin(JvpSkinArgs a) {
  __shared__ float4 sT[kJvpTdotFloats / 4];
  const int f = blockIdx.x;
  {
    const float4* src = reinterpret_cast<const float4*>(a.tdot + (size_t)f * kJvpTdotFloats);
    for (int i = threadIdx.x; i < kJvpTdotFloats / 4; i += 256) sT[i] = src[i];
  }
  __syncthreads();
  const int v = blockIdx.y * 256 + threadIdx.x;
  if (v >= a.V) return;
  const uint32_t widx = a.wIdx[v];
  const float4 wv = reinterpret_cast<const float4*>(a.wVal)[v];
  const float wgt[4] = {wv.x, wv.y, wv.z, wv.w};
  int jn[4];
  float Mx[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) Mx[e] = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    jn[i] = (int)((widx >> (8 * i)) & 0xffu);
    jn[i] = jn[i] < kMaxJoints ? jn[i] : 0;                // (padding entries carry weight 0)
    const float4* T = reinterpret_cast<const float4*>(a.skinT + ((size_t)f * kMaxJoints + jn[i]) * 12);
    const float4 t0 = T[0], t1 = T[1], t2 = T[2];
    Mx[0] += wgt[i] * t0.x; Mx[1] += wgt[i] * t0.y; Mx[2] += wgt[i] * t0.z;
    Mx[3] += wgt[i] * t1.x; Mx[4] += wgt[i] * t1.y; Mx[5] += wgt[i] * t1.z;
    Mx[6] += wgt[i] * t2.x; Mx[7] += wgt[i] * t2.y; Mx[8] += wgt[i] * t2.z;
  }
  const size_t Vp = (size_t)a.nVT * kVTile;
  const float* bp = a.bbuf + ((size_t)f * Vp + v) * 3;
  const float b0 = bp[0], b1 = bp[1], b2 = bp[2];
  const int n_act = min(kJvpTile, a.K - a.k0);
  for (int row = 0; row < n_act; ++row) {
    float D[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) D[e] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4* T = sT + (row * kMaxJoints + jn[i]) * 3;
      const float4 t0 = T[0], t1 = T[1], t2 = T[2];
      const float tv[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
#pragma unroll
      for (int e = 0; e < 12; ++e) D[e] += wgt[i] * tv[e];
    }
    const float* dp = a.dbuf + (((size_t)f * kJvpTile + row) * Vp + v) * 3;
    const float d0 = dp[0], d1 = dp[1], d2 = dp[2];
    JvpF3 o;
    o.x = D[0] * b0 + D[1] * b1 + D[2] * b2 + D[3] + (Mx[0] * d0 + Mx[1] * d1 + Mx[2] * d2);
    o.y = D[4] * b0 + D[5] * b1 + D[6] * b2 + D[7] + (Mx[3] * d0 + Mx[4] * d1 + Mx[5] * d2);
    o.z = D[8] * b0 + D[9] * b1 + D[10] * b2 + D[11] + (Mx[6] * d0 + Mx[7] * d1 + Mx[8] * d2);
    *reinterpret_cast<JvpF3*>(a.out + ((size_t)f * a.K + a.k0 + row) * (size_t)a.row_floats + (size_t)v * 3) = o;
  }
}

}  // namespace

size_t jvp_feat_elems(int F) { return (size_t)F * kBlendKSteps * 2 * 64 * 8; }
size_t jvp_tdot_elems(int F) { return (size_t)F * kJvpTdotFloats; }
size_t jvp_bbuf_elems(int F, int nVT) { return (size_t)F * nVT * kVTile * 3; }

size_t jvp_dbuf_elems(int F, int nVT) { return (size_t)F * kJvpTile * nVT * kVTile * 3; }

void launch_jvp_blend(const DevModel& M, const DevProblem& P, const MeshCoef& mc, float* d_bbuf, hipStream_t s) {
  BODYFIT_LAUNCH(k_jvp_blend, dim3(M.nVTiles, P.nFTiles), dim3(64), 0, s, M.dirsB, mc.featA, P.F, kJvpTile, M.V, M.nVTiles, d_bbuf);
}

void launch_jvp_chain(const DevModel& M, const DevProblem& P, const double* d_params, const double* d_beta, int K, int k0,
                      int n_tiles, const double* d_tan_params, const double* d_tan_beta, int tan_beta_per_frame,
                      double* d_tan_joints, float* d_tdot, uint16_t* d_featD, hipStream_t s) {
  JvpChainArgs a;
  a.M = M; a.F = P.F; a.K = K; a.k0 = k0;
  a.use_shape = P.use_shape; a.beta_stride = P.beta_stride; a.pose_blend = P.pose_blend;
  a.tan_beta_per_frame = tan_beta_per_frame;
  a.params = d_params; a.beta = d_beta; a.R0 = P.R0; a.tan_params = d_tan_params; a.tan_beta = d_tan_beta;
  a.tan_joints = d_tan_joints; a.tdot = d_tdot; a.featD = d_featD;
  BODYFIT_LAUNCH(k_jvp_chain, dim3(n_tiles, P.F), dim3(64), 0, s, a);
}

void launch_jvp_mesh(const DevModel& M, const DevProblem& P, const MeshCoef& mc, const uint16_t* d_featD, const float* d_tdot,
                     const float* d_bbuf, float* d_dbuf, int K, int k0, float* d_out, long long row_floats, hipStream_t s) {
  const int n_act = K - k0 < kJvpTile ? K - k0 : kJvpTile;
  BODYFIT_LAUNCH(k_jvp_blend, dim3(M.nVTiles, P.F), dim3(64), 0, s, M.dirsB, d_featD, P.F * kJvpTile, n_act, M.V, M.nVTiles, d_dbuf);
  JvpSkinArgs a;
  a.tdot = d_tdot; a.skinT = mc.skinT; a.bbuf = d_bbuf; a.dbuf = d_dbuf; a.wIdx = M.wIdx; a.wVal = M.wVal;
  a.F = P.F; a.K = K; a.k0 = k0; a.V = M.V; a.nVT = M.nVTiles; a.out = d_out; a.row_floats = row_floats;
  BODYFIT_LAUNCH(k_jvp_skin, dim3(P.F, (M.V + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace bodyfit
