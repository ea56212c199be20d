// k_window_cr.hip — the block cyclic reduction of the device window LM (k_window_lm.hip has the method): factor an
// eliminated frame's block (k_cr_factor), update the remaining frames (k_cr_update), and the way down (k_cr_back).
#include "dense_inl.h"
#include "window_lm_inl.h"

namespace bodyfit {
namespace {

typedef __attribute__((ext_vector_type(4))) double d4;

// Staging of 80 x 80 (or 16 x 80) blocks between HBM/L2 and LDS.  A plain `for (idx = tid; idx < n; idx += threads) lds[..] =
// g[idx]` compiles to load -> s_waitcnt vmcnt(0) -> ds_write per trip: thirteen DEPENDENT L2 round trips per block (k_cr_factor
// spent 9 of its 27 us in them).  Here every load of a block is issued before the first is used (fixed trip count, clamped
// index, predicated use).
constexpr int kCrThreads = 512, kCrWaves = 8;
template <int ROWS>
struct BlockRegs { static constexpr int kPasses = (ROWS * WB + kCrThreads - 1) / kCrThreads; double v[kPasses]; };
template <int ROWS>
__device__ __forceinline__ void block_load(BlockRegs<ROWS>& r, const double* __restrict__ src, int tid) {
#pragma unroll
  for (int u = 0; u < BlockRegs<ROWS>::kPasses; ++u) r.v[u] = src[min(tid + u * kCrThreads, ROWS * WB - 1)];
}
// dst[row][col] (leading dimension LD); transposed: the element (i, k) of the source lands at row k, column i
template <int ROWS, bool kTransposed = false, bool kLowerOnly = false>
__device__ __forceinline__ void block_to_lds(const BlockRegs<ROWS>& r, double* dst, int tid) {
#pragma unroll
  for (int u = 0; u < BlockRegs<ROWS>::kPasses; ++u) {
    const int idx = tid + u * kCrThreads;
    if (idx < ROWS * WB) {
      const int i = idx / WB, k = idx % WB;
      const double v = (kLowerOnly && k > i) ? 0.0 : r.v[u];
      dst[kTransposed ? k * LD + i : i * LD + k] = v;
    }
  }
}
// LDS [ROWS][LD] -> global [ROWS][WB]: the LDS reads of the block first, then its stores
template <int ROWS, bool kLowerOnly = false>
__device__ __forceinline__ void block_from_lds(double* __restrict__ dst, const double* src, int tid) {
  BlockRegs<ROWS> r;
#pragma unroll
  for (int u = 0; u < BlockRegs<ROWS>::kPasses; ++u) {
    const int idx = min(tid + u * kCrThreads, ROWS * WB - 1);
    r.v[u] = src[(idx / WB) * LD + idx % WB];
  }
#pragma unroll
  for (int u = 0; u < BlockRegs<ROWS>::kPasses; ++u) {
    const int idx = tid + u * kCrThreads;
    if (idx < ROWS * WB) dst[idx] = (kLowerOnly && idx % WB > idx / WB) ? 0.0 : r.v[u];
  }
}

// ---- cyclic reduction: factor one eliminated block, solve its appended rows -------------------------------------------
// Two workgroups per eliminated frame j (side = blockIdx.x & 1): both factor D_j = L L^T (right-looking, 16-column
// panels, the k_lm_step scheme: diagonal block in the registers of wave 0, panel solve one row per thread, trailing update
// on the f64 matrix cores) with rows appended below that receive L^-T from the right:
//   side 0:  rows of U_a (-> Pt_j)  and the 16 rows of Rt_j (-> Yt_j);  writes L_j
//   side 1:  rows of U_j^T (-> Qt_j)
constexpr int kCrRowsMax = WB + WB + WR;   // 176
#ifdef BODYFIT_CR_STAMPS   // diagnostic build only (tools/ubench/cr_factor_phases.hip): s_memtime of wave 0 per phase
__device__ unsigned long long g_cr_stamps[64];
#define CR_STAMP(i)                                                                   \
  do {                                                                                \
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                        \
      unsigned long long t_;                                                          \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
      g_cr_stamps[i] = t_;                                                            \
    }                                                                                 \
  } while (0)
#else
#define CR_STAMP(i)
#endif
// (the pointers of the kernel's first loads come as leading scalar arguments: with -mllvm -amdgpu-kernarg-preload-count they are
//  in SGPRs when the wave starts, one scalar round trip earlier than fields of the by-value struct)
__global__ __launch_bounds__(kCrThreads) void k_cr_factor(const int* __restrict__ elim, const double* __restrict__ Dp,
                                                          const double* __restrict__ Up, const double* __restrict__ Rtp,
                                                          int n_elim, WinBuf W) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* M = sm;                          // [kCrRowsMax][LD]
  double* invd = sm + kCrRowsMax * LD;     // [WB]
  double* stat = invd + WB;                // [1]
  const int e = blockIdx.x >> 1, side = blockIdx.x & 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = elim[3 * e], a = elim[3 * e + 1], b = elim[3 * e + 2];
  if (side == 1 && b < 0) return;
  CR_STAMP(0);
  const int nU = (side == 0) ? (a >= 0 ? WB : 0) : WB;       // appended coupling rows
  const int nApp = nU + (side == 0 ? WR : 0);
  const int nRows = WB + nApp;
  {
    // the node's blocks: all three requested before any lands in LDS (one round trip)
    BlockRegs<WB> rD, rU;
    BlockRegs<WR> rR;
    block_load<WB>(rD, Dp + (size_t)j * WB * WB, tid);
    if (nU) block_load<WB>(rU, Up + (size_t)(side == 0 ? a : j) * WB * WB, tid);
    if (side == 0) block_load<WR>(rR, Rtp + (size_t)j * WR * WB, tid);
    block_to_lds<WB, false, true>(rD, M, tid);
    if (nU) {
      if (side == 0) block_to_lds<WB>(rU, M + WB * LD, tid);              // row i of U_a
      else block_to_lds<WB, true>(rU, M + WB * LD, tid);                  // row i of U_j^T = column i of U_j
    }
    if (side == 0) block_to_lds<WR>(rR, M + (WB + nU) * LD, tid);
  }
  if (tid == 0) stat[0] = 1.0;
  __syncthreads();
  CR_STAMP(1);
  constexpr int NPAN = WB / 16;   // 5
  double* Linv = stat + 8;        // [16][17]: L_pp^-T of the current panel
  // (a) diagonal block p + identity below it, in the registers of wave 0, spread over all 64 lanes in the layout of an f64
  //     16 x 16 accumulator (dense_inl.h diag_factor16_acc): lane (m, kk), register q <-> row kk + 4 q, column m
  auto diag_block = [&](int p) {
    const int c0 = 16 * p;
    const int m = lane & 15, kk = lane >> 4;
    double av[4], bv[4], invc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // (the FULL symmetric block: only its lower triangle is kept up to date in LDS, mirror it)
      const int r = kk + 4 * q, lo = max(r, m), hi = min(r, m);
      av[q] = M[(c0 + lo) * LD + c0 + hi];
      bv[q] = (r == m) ? 1.0 : 0.0;
    }
    const bool okp = diag_factor16_acc(av, bv, lane, invc, min(16, NP - c0));
    double* Lg = W.Li + ((size_t)j * (WB / 16) + p) * 256;   // kept for the way down (k_cr_back)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = kk + 4 * q;
      if (r >= m) M[(c0 + r) * LD + c0 + m] = av[q];           // L (lower triangle)
      Linv[r * 17 + m] = bv[q];                                // row r of L_pp^-T (zero left of the diagonal)
      if (side == 0) Lg[r * 16 + m] = bv[q];
    }
    if (lane == 0 && !okp) stat[0] = 0.0;
  };
  if (wave == 0) diag_block(0);
  __syncthreads();
  CR_STAMP(2);
  const int nRowTiles = nRows / 16;
  for (int p = 0; p < NPAN; ++p) {
    const int c0 = 16 * p;
    // (b) panel solve on the matrix cores: every 16-row tile below the diagonal block  X = A L_pp^-T
    {
      const int m = lane & 15, kk = lane >> 4;
      for (int I = p + 1 + wave; I < nRowTiles; I += kCrWaves) {
        double a4[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) a4[s4] = M[(16 * I + m) * LD + c0 + 4 * s4 + kk];
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a4[s4], Linv[(4 * s4 + kk) * 17 + m], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) M[(16 * I + kk + 4 * q) * LD + c0 + m] = acc[q];
      }
    }
    __syncthreads();
    CR_STAMP(3 + 4 * p);
    // (c) trailing update on the matrix cores: rows of tile I, columns of panel Kc > p:  M[I][Kc] -= X_I X_Kc^T.
    //     Look-ahead: wave 0 updates the next diagonal tile first and factors it at once (the serial part of a panel)
    //     while the other seven waves update the rest.
    if (p + 1 < NPAN) {
      const int m = lane & 15, kk = lane >> 4;
      auto tile_update = [&](int I, int Kc) {
        d4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = M[(16 * I + kk + 4 * q) * LD + 16 * Kc + m];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const double av = -M[(16 * I + m) * LD + c0 + 4 * s4 + kk];
          const double bv = M[(16 * Kc + m) * LD + c0 + 4 * s4 + kk];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) M[(16 * I + kk + 4 * q) * LD + 16 * Kc + m] = acc[q];
      };
      // a whole row of tiles per wave: the row tile's own panel entries (A operand) are read once, every LDS read of the row
      // is issued before the first product, and the <= 4 column tiles are four independent accumulator chains (tile by tile,
      // each product waited for its two LDS reads and the previous product: ~790 cycles per tile against 256 of matrix work)
      auto row_update = [&](int I) {
        const int kc1 = (I < NPAN) ? I : NPAN - 1;                 // last column tile of this row
        double a4[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) a4[s4] = -M[(16 * I + m) * LD + c0 + 4 * s4 + kk];
        d4 acc[4];
        double b4[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int Kc = min(p + 1 + j, NPAN - 1);                 // (clamped: loads of unused tiles stay inside the block)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[j][q] = M[(16 * I + kk + 4 * q) * LD + 16 * Kc + m];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) b4[j][s4] = M[(16 * Kc + m) * LD + c0 + 4 * s4 + kk];
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (p + 1 + j <= kc1) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a4[s4], b4[j][s4], acc[j], 0, 0, 0);   // (uniform)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (p + 1 + j <= kc1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) M[(16 * I + kk + 4 * q) * LD + 16 * (p + 1 + j) + m] = acc[j][q];
          }
        }
      };
      if (wave == 0) {
        tile_update(p + 1, p + 1);
        CR_STAMP(4 + 4 * p);
        diag_block(p + 1);
        CR_STAMP(5 + 4 * p);
      } else {
        for (int I = p + 2 + (wave - 1); I < nRowTiles; I += kCrWaves - 1) row_update(I);
      }
    }
    __syncthreads();
    CR_STAMP(6 + 4 * p);
  }
  if (tid == 0 && stat[0] == 0.0) *W.fail = 1;
  if (side == 0) {
    block_from_lds<WB, true>(W.L + (size_t)j * WB * WB, M, tid);
    if (nU) block_from_lds<WB>(W.Pt + (size_t)j * WB * WB, M + WB * LD, tid);
    block_from_lds<WR>(W.Yt + (size_t)j * WR * WB, M + (WB + nU) * LD, tid);
  } else {
    block_from_lds<WB>(W.Qt + (size_t)j * WB * WB, M + WB * LD, tid);
  }
  CR_STAMP(24);
}

// C[ti][tj] (16 x 16 tile, accumulator layout: row = (lane >> 4) + 4 q, column = lane & 15) += sign * sum_k X[i][k] Y[i'][k]
// with X, Y staged in LDS (leading dimension LD), K = WB
__device__ __forceinline__ d4 tile_xyT(const double* X, const double* Y, int ti, int tj, int lane, d4 acc, double sign) {
  const int m = lane & 15, kk = lane >> 4;
#pragma unroll 4
  for (int s = 0; s < WB / 4; ++s) {
    const double av = sign * X[(16 * ti + m) * LD + 4 * s + kk];
    const double bv = Y[(16 * tj + m) * LD + 4 * s + kk];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

// ---- cyclic reduction: Schur updates of one remaining frame a (left eliminated neighbour jl, right one jr, next
//      remaining frame b).  Four workgroups per frame: diagonal block (two halves of its tiles), coupling block, rhs. -----
__global__ __launch_bounds__(kCrThreads) void k_cr_update(const int* __restrict__ surv, int n_surv, int split,
                                                          double* __restrict__ Dp, const double* __restrict__ Qtp,
                                                          const double* __restrict__ Ptp, WinBuf W) {   // (leading scalars: k_cr_factor)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* X0 = sm;                 // [WB][LD]
  double* X1 = sm + WB * LD;       // [WB][LD]
  double* Ys = X1 + WB * LD;       // [2][WR][LD]
  // four workgroups per remaining frame: the diagonal block's 15 lower tiles in two halves (its 600 f64 matrix
  // instructions were the longest part by 2x: one tile per wave now), the coupling block, the right-hand sides
  // (split = 1, levels that do not fill the chip; on the throughput-bound levels of a long window one workgroup takes both
  //  halves: three workgroups per frame)
  const int sidx = split ? (int)(blockIdx.x >> 2) : (int)(blockIdx.x / 3), part4 = split ? (int)(blockIdx.x & 3) : -1;
  const int part = split ? (part4 < 2 ? 0 : part4 - 1) : (int)(blockIdx.x % 3);
  const int h0 = split ? (part4 & 1) : 0, h1 = split ? h0 + 1 : 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int a = surv[4 * sidx], jl = surv[4 * sidx + 1], jr = surv[4 * sidx + 2], b = surv[4 * sidx + 3];
  const int m = lane & 15, kk = lane >> 4;
  // Every operand of the part is requested before the first is used: the source blocks (13 loads per thread each) and the
  // accumulator tiles of the wave (read-modify-write of global memory), one round trip instead of one per trip / per tile.
  if (part == 0) {
    // D_a -= Qt_jl Qt_jl^T + Pt_jr Pt_jr^T  (15 lower tiles over 8 waves: tiles wave and wave + 8)
    double* D = Dp + (size_t)a * WB * WB;
    BlockRegs<WB> r0, r1;
    if (jl >= 0) block_load<WB>(r0, Qtp + (size_t)jl * WB * WB, tid);
    if (jr >= 0) block_load<WB>(r1, Ptp + (size_t)jr * WB * WB, tid);
    int tis[2], tjs[2];
    d4 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {                         // this wave's tile of each half it carries
      const int t = min(wave + 8 * u, 14);
      int ti = 0, tj = t;
      while (tj > ti) { tj -= ti + 1; ++ti; }             // t -> (ti, tj) of the lower triangle, row-major
      tis[u] = ti; tjs[u] = tj;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[u][q] = (u >= h0 && u < h1) ? D[(size_t)(16 * ti + kk + 4 * q) * WB + 16 * tj + m] : 0.0;
    }
    if (jl >= 0) block_to_lds<WB>(r0, X0, tid);
    if (jr >= 0) block_to_lds<WB>(r1, X1, tid);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u < h0 || u >= h1 || wave + 8 * u > 14) continue;
      // the two sources as two independent accumulator chains
      d4 acc2 = {0.0, 0.0, 0.0, 0.0};
      if (jl >= 0) acc[u] = tile_xyT(X0, X0, tis[u], tjs[u], lane, acc[u], -1.0);
      if (jr >= 0) acc2 = tile_xyT(X1, X1, tis[u], tjs[u], lane, acc2, -1.0);
#pragma unroll
      for (int q = 0; q < 4; ++q) D[(size_t)(16 * tis[u] + kk + 4 * q) * WB + 16 * tjs[u] + m] = acc[u][q] + acc2[q];
    }
  } else if (part == 1) {
    // U_a := -Pt_jr Qt_jr^T  (coupling of a with the next remaining frame b)
    if (jr < 0 || b < 0) return;
    BlockRegs<WB> r0, r1;
    block_load<WB>(r0, W.Pt + (size_t)jr * WB * WB, tid);
    block_load<WB>(r1, W.Qt + (size_t)jr * WB * WB, tid);
    block_to_lds<WB>(r0, X0, tid);
    block_to_lds<WB>(r1, X1, tid);
    __syncthreads();
    double* U = W.U + (size_t)a * WB * WB;
    for (int t = wave; t < 25; t += kCrWaves) {
      const int ti = t / 5, tj = t % 5;
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      acc = tile_xyT(X0, X1, ti, tj, lane, acc, -1.0);
#pragma unroll
      for (int q = 0; q < 4; ++q) U[(size_t)(16 * ti + kk + 4 * q) * WB + 16 * tj + m] = acc[q];
    }
  } else {
    // Rt_a -= Yt_jl Qt_jl^T + Yt_jr Pt_jr^T   ([16 x 80]: one column tile per wave, waves 0-4)
    double* Rt = W.Rt + (size_t)a * WR * WB;
    BlockRegs<WB> r0, r1;
    BlockRegs<WR> y0, y1;
    if (jl >= 0) { block_load<WB>(r0, W.Qt + (size_t)jl * WB * WB, tid); block_load<WR>(y0, W.Yt + (size_t)jl * WR * WB, tid); }
    if (jr >= 0) { block_load<WB>(r1, W.Pt + (size_t)jr * WB * WB, tid); block_load<WR>(y1, W.Yt + (size_t)jr * WR * WB, tid); }
    const int tj = min(wave, 4);
    d4 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = Rt[(size_t)(kk + 4 * q) * WB + 16 * tj + m];
    if (jl >= 0) { block_to_lds<WB>(r0, X0, tid); block_to_lds<WR>(y0, Ys, tid); }
    if (jr >= 0) { block_to_lds<WB>(r1, X1, tid); block_to_lds<WR>(y1, Ys + WR * LD, tid); }
    __syncthreads();
    if (wave < 5) {
      if (jl >= 0) acc = tile_xyT(Ys, X0, 0, tj, lane, acc, -1.0);
      if (jr >= 0) acc = tile_xyT(Ys + WR * LD, X1, 0, tj, lane, acc, -1.0);
#pragma unroll
      for (int q = 0; q < 4; ++q) Rt[(size_t)(kk + 4 * q) * WB + 16 * tj + m] = acc[q];
    }
  }
}

// ---- cyclic reduction, way down: x_j = L_j^-T (Y_j - P_j x_a - Q_j x_b), 11 right-hand sides ---------------------------
// In the transposed storage:  Zt = Yt - Xt_a Pt - Xt_b Qt  ([16 x 80] = [16 x 80][80 x 80], f64 MFMA, B operands straight from
// L2: 16 consecutive doubles per lane group), then  Xt L = Zt  solved panel by panel from the last one: the products with
// the already known panels on the matrix cores, the 16 x 16 diagonal blocks through their explicit inverses (computed
// here, one block per wave, while the other waves form Zt).
__global__ __launch_bounds__(kCrThreads) void k_cr_back(const int* __restrict__ elim, const double* __restrict__ Lp,
                                                        const double* __restrict__ Xtp, int n_elim, WinBuf W) {   // (leading scalars: k_cr_factor)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Ls = sm;                     // [WB][LD]
  double* Zt = sm + WB * LD;           // [WR][LD]   right-hand sides, overwritten by the solution panel by panel
  double* Xa = Zt + WR * LD;           // [WR][LD]
  double* Xb = Xa + WR * LD;           // [WR][LD]
  double* Li = Xb + WR * LD;           // [5][16][17]  inverses of the diagonal blocks of L
  const int e = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = lane & 15, kk = lane >> 4;
  const int j = elim[3 * e], a = elim[3 * e + 1], b = elim[3 * e + 2];
  {
    BlockRegs<WB> rL;
    BlockRegs<WR> rA, rB;
    block_load<WB>(rL, Lp + (size_t)j * WB * WB, tid);
    if (a >= 0) block_load<WR>(rA, Xtp + (size_t)a * WR * WB, tid);
    if (b >= 0) block_load<WR>(rB, Xtp + (size_t)b * WR * WB, tid);
    block_to_lds<WB>(rL, Ls, tid);
    if (a >= 0) block_to_lds<WR>(rA, Xa, tid);
    if (b >= 0) block_to_lds<WR>(rB, Xb, tid);
  }
  __syncthreads();
  if (wave < 5) {
    // Zt tile (all 16 rows, columns 16 wave ..): accumulate -X P and -X Q on top of Yt
    const int tj = wave;
    const double* Yt = W.Yt + (size_t)j * WR * WB;
    d4 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = Yt[(size_t)(kk + 4 * q) * WB + 16 * tj + m];
    for (int src = 0; src < 2; ++src) {
      const int nb_ = src == 0 ? a : b;
      if (nb_ < 0) continue;
      const double* G = (src == 0 ? W.Pt : W.Qt) + (size_t)j * WB * WB;
      const double* Xs = src == 0 ? Xa : Xb;
      double bv[WB / 4];
#pragma unroll
      for (int s4 = 0; s4 < WB / 4; ++s4) bv[s4] = G[(size_t)(4 * s4 + kk) * WB + 16 * tj + m];
#pragma unroll
      for (int s4 = 0; s4 < WB / 4; ++s4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Xs[m * LD + 4 * s4 + kk], bv[s4], acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Zt[(kk + 4 * q) * LD + 16 * tj + m] = acc[q];
  } else if (wave == 5 || wave == 6) {
    // inverses of the five 16 x 16 diagonal blocks of L, as k_cr_factor left them: (L_pp^-T)[c][r] = (L_pp^-1)[r][c]
    const double* Lg = W.Li + (size_t)j * (WB / 16) * 256;
    for (int it = tid - 320; it < 5 * 256; it += 128) {
      const int blk = it >> 8, c = (it >> 4) & 15, r = it & 15;
      Li[(blk * 16 + r) * 17 + c] = Lg[it];
    }
  }
  __syncthreads();
  // Xt[:, p] = (Zt[:, p] - sum_{q > p} Xt[:, q] L[q, p]) Linv_pp, panels from the last to the first; wave 0 only (each step
  // depends on the previous one; 4 + 4 (5 - p - 1) MFMAs per step)
  if (wave == 0) {
    for (int p = 4; p >= 0; --p) {
      d4 acc;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = Zt[(kk + 4 * q) * LD + 16 * p + m];
      for (int qp = p + 1; qp < 5; ++qp) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Zt[m * LD + 16 * qp + 4 * s4 + kk], Ls[(16 * qp + 4 * s4 + kk) * LD + 16 * p + m],
                                                     acc, 0, 0, 0);
      }
      // through LDS: the accumulator tile becomes the A operand of the product with the inverse
#pragma unroll
      for (int q = 0; q < 4; ++q) Zt[(kk + 4 * q) * LD + 16 * p + m] = acc[q];
      d4 xo = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
        xo = __builtin_amdgcn_mfma_f64_16x16x4f64(Zt[m * LD + 16 * p + 4 * s4 + kk], Li[(p * 16 + 4 * s4 + kk) * 17 + m], xo, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) Zt[(kk + 4 * q) * LD + 16 * p + m] = xo[q];
    }
  }
  __syncthreads();
  double* Xt = W.Xt + (size_t)j * WR * WB;
  for (int idx = tid; idx < WR * WB; idx += kCrThreads) {
    const int c = idx / WB, k = idx % WB;
    Xt[idx] = (c <= NBETA) ? Zt[c * LD + k] : 0.0;
  }
}

}  // namespace

size_t win_factor_lds_bytes() { return (size_t)(kCrRowsMax * LD + WB + 8 + 16 * 17) * sizeof(double); }
size_t win_update_lds_bytes() { return (size_t)(2 * WB * LD + 2 * WR * LD) * sizeof(double); }
size_t win_back_lds_bytes() { return (size_t)(WB * LD + 3 * WR * LD + 5 * 16 * 17) * sizeof(double); }

void launch_cr_factor(const WinBuf& W, const int* d_elim, int n_elim, hipStream_t s) {
  static DeviceOnce attr;
  attr.run(current_device(), [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_cr_factor), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)win_factor_lds_bytes());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_cr_update), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)win_update_lds_bytes());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_cr_back), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)win_back_lds_bytes());
  });
  if (n_elim > 0)
    BODYFIT_LAUNCH(k_cr_factor, dim3(2 * n_elim), dim3(kCrThreads), win_factor_lds_bytes(), s, d_elim, W.D, W.U, W.Rt, n_elim, W);
}
void launch_cr_update(const WinBuf& W, const int* d_surv, int n_surv, hipStream_t s) {
  if (n_surv > 0) {
    const int split = 4 * n_surv <= 256 ? 1 : 0;        // (the diagonal block in two workgroups where CUs are idle anyway)
    BODYFIT_LAUNCH(k_cr_update, dim3((split ? 4 : 3) * n_surv), dim3(kCrThreads), win_update_lds_bytes(), s, d_surv, n_surv, split,
                   W.D, W.Qt, W.Pt, W);
  }
}
void launch_cr_back(const WinBuf& W, const int* d_elim, int n_elim, hipStream_t s) {
  if (n_elim > 0) BODYFIT_LAUNCH(k_cr_back, dim3(n_elim), dim3(kCrThreads), win_back_lds_bytes(), s, d_elim, W.L, W.Xt, n_elim, W);
}

}  // namespace bodyfit
