// Surface extraction: marching cubes of a distance volume as a stream compaction (bodyfit_volume_surface_count_device /
// _emit_device; include/bodyfit.h: the definition, the table's rule, the contract and its derivation; the host entries:
// api_volume.hip; the table: mc_table_inl.h, written by tools/gen_mc_table.py).
//
//   k_mc_classify  one lane per voxel, x fastest: the eight voxels (and weights) of the cell whose corner 0 the voxel is -> one byte,
//                  the cell's CODE: its case when the cell is live, 0 when it is dead or does not exist (the last index of an axis).
//                  A dead cell and case 0 need not be told apart: neither emits a triangle nor crosses an edge.
//   k_mc_count     one lane per voxel: the codes of the seven cells around the voxel's three owned edges say which of them carry a
//                  vertex (an edge is crossed in a live cell around it iff the two case bits of its ends differ: a live cell has
//                  usable corners, so "both ends usable" needs no second look at the volume), the own code how many triangles.
//                  Exclusive scan inside the workgroup (wave64 shuffles, then the four wave sums through LDS); per voxel a u16 word
//                  = the three edge flags over the vertex offset inside the workgroup (at most 3 x 255), per workgroup two sums.
//   k_mc_scan      one workgroup of 1024 lanes per volume: the exclusive scan of the workgroup sums in place, four sums per lane and
//                  4096 per round, the carry going from round to round (a 256^3 volume: 65,536 sums, 16 rounds); the volume's totals.
//   k_mc_offsets   one workgroup: the exclusive scan of the volumes' totals into the caller's i64 offsets.
//   k_mc_emit      one lane per voxel: its vertices (unfused f64, one store each) at offsets[vol] + workgroup offset + word; its
//                  cell's triangles at the same of the triangle counts, scanned again here; a triangle corner is the owner's
//                  workgroup offset + word + the rank of the axis among the owner's flags: plain loads of what k_mc_count kept.
// Everything is a function of the volume alone, integers are summed in a fixed order, no atomics: bit-identical from run to run
// and whatever the batch.  Every store of k_mc_emit is guarded by the capacities.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bodyfit_device.h"
#include "volume.h"

#pragma clang fp contract(off)

namespace bodyfit {

namespace {

#define MC_TABLE_STORAGE __constant__
#include "mc_table_inl.h"                            // MC_N_TRI[256], MC_TRI[256][16]: a case's 16 bytes are one uint4

constexpr unsigned WORD_BITS = 13;                   // the vertex offset inside a workgroup: <= 765 < 2^13; the flags above it
constexpr unsigned WORD_MASK = (1u << WORD_BITS) - 1;

struct Voxel { unsigned vol, chunk, n, i, j, k; };

__device__ __forceinline__ Voxel voxel_of(const SurfaceArgs& A) {
  Voxel v;
  v.vol = blockIdx.x / A.chunks;
  v.chunk = blockIdx.x - v.vol * A.chunks;
  v.n = v.chunk * 256 + threadIdx.x;
  v.i = v.n % (unsigned)A.nx;
  const unsigned row = v.n / (unsigned)A.nx;
  v.j = row % (unsigned)A.ny;
  v.k = row / (unsigned)A.ny;
  return v;
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned wave_scan(unsigned x) {
  const unsigned lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d, 64);
    if (lane >= (unsigned)d) x += y;
  }
  return x;
}

// exclusive scan over the W waves of a workgroup (every lane calls it); `total`: the workgroup's sum.  `part`: W + 1 words of LDS.
template <int W>
__device__ __forceinline__ unsigned block_scan(unsigned x, unsigned* part, unsigned& total) {
  const unsigned incl = wave_scan(x);
  const unsigned wave = threadIdx.x >> 6;
  __syncthreads();                                   // (the previous use of `part` is over)
  if ((threadIdx.x & 63) == 63) part[wave] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const unsigned s = part[w];
    if ((unsigned)w < wave) before += s;
    all += s;
  }
  total = all;
  return before + incl - x;
}

__global__ __launch_bounds__(256) void k_mc_classify(const SurfaceArgs A) {
  const Voxel v = voxel_of(A);
  if (v.n >= A.n_voxels) return;
  unsigned code = 0;
  if ((int)v.i < A.nx - 1 && (int)v.j < A.ny - 1 && (int)v.k < A.nz - 1) {
    const size_t base = (size_t)v.vol * (size_t)A.volume_stride + (size_t)v.n;
    const size_t sy = (size_t)A.nx, sz = (size_t)A.nx * (size_t)A.ny;
    float val[8], wt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const size_t at = base + (c & 1) + (c >> 1 & 1) * sy + (c >> 2 & 1) * sz;
      val[c] = A.volume[at];
      wt[c] = A.weight ? A.weight[at] : 0.0f;
    }
    bool live = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      // (x - x == 0: finite; every comparison is false on a NaN, a NaN weight's too)
      live = live & (val[c] - val[c] == 0.0f) & (A.weight == nullptr || wt[c] >= A.min_weight);
      code |= (val[c] < A.iso ? 1u : 0u) << c;
    }
    if (!live) code = 0;
  }
  A.code[(size_t)v.vol * A.n_voxels + v.n] = (unsigned char)code;
}

// does a cell of code `cc` cross its edge between the corners p and q
__device__ __forceinline__ unsigned crosses(unsigned cc, int p, int q) { return ((cc >> p) ^ (cc >> q)) & 1u; }

__global__ __launch_bounds__(256) void k_mc_count(const SurfaceArgs A) {
  __shared__ unsigned part[5];
  __shared__ unsigned char n_tri[256];
  n_tri[threadIdx.x] = MC_N_TRI[threadIdx.x];
  __syncthreads();
  const Voxel v = voxel_of(A);
  const bool in = v.n < A.n_voxels;
  unsigned flags = 0, tris = 0;
  if (in) {
    const unsigned char* code = A.code + (size_t)v.vol * A.n_voxels + v.n;
    const ptrdiff_t sy = A.nx, sz = (ptrdiff_t)A.nx * A.ny;
    const bool bi = v.i > 0, bj = v.j > 0, bk = v.k > 0;
    // the cells (k - dk, j - dj, i - di) around the owned edges; a cell that does not exist reads as 0
    const unsigned c000 = code[0];
    const unsigned c001 = bi ? code[-1] : 0u, c010 = bj ? code[-sy] : 0u, c100 = bk ? code[-sz] : 0u;
    const unsigned c011 = bi && bj ? code[-sy - 1] : 0u, c101 = bi && bk ? code[-sz - 1] : 0u, c110 = bj && bk ? code[-sz - sy] : 0u;
    const unsigned fx = crosses(c000, 0, 1) | crosses(c010, 2, 3) | crosses(c100, 4, 5) | crosses(c110, 6, 7);
    const unsigned fy = crosses(c000, 0, 2) | crosses(c001, 1, 3) | crosses(c100, 4, 6) | crosses(c101, 5, 7);
    const unsigned fz = crosses(c000, 0, 4) | crosses(c001, 1, 5) | crosses(c010, 2, 6) | crosses(c011, 3, 7);
    flags = fx | fy << 1 | fz << 2;
    tris = n_tri[c000];
  }
  const unsigned verts = __popc(flags);
  // one scan for both: the triangles (<= 5 x 256) above bit 16, the vertices (<= 3 x 256) below
  unsigned total;
  const unsigned excl = block_scan<4>(verts | tris << 16, part, total);
  if (in) A.word[(size_t)v.vol * A.n_voxels + v.n] = (unsigned short)(flags << WORD_BITS | (excl & 0xffffu));
  if (threadIdx.x == 0) {
    A.block_verts[blockIdx.x] = total & 0xffffu;
    A.block_tris[blockIdx.x] = total >> 16;
  }
}

__global__ __launch_bounds__(1024) void k_mc_scan(const SurfaceArgs A) {
  __shared__ unsigned part[17];
  const unsigned vol = blockIdx.x;
  unsigned* bv = A.block_verts + (size_t)vol * A.chunks;
  unsigned* bt = A.block_tris + (size_t)vol * A.chunks;
  unsigned carry_v = 0, carry_t = 0;                 // (a volume's totals are below 2^31: the host's check)
  for (unsigned start = 0; start < A.chunks; start += 4096) {
    const unsigned at = start + 4 * threadIdx.x;
    unsigned v[4], t[4], sum_v = 0, sum_t = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = at + q < A.chunks;
      v[q] = in ? bv[at + q] : 0u;
      t[q] = in ? bt[at + q] : 0u;
      sum_v += v[q];
      sum_t += t[q];
    }
    unsigned all_v, all_t;
    unsigned run_v = carry_v + block_scan<16>(sum_v, part, all_v);
    unsigned run_t = carry_t + block_scan<16>(sum_t, part, all_t);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (at + q < A.chunks) { bv[at + q] = run_v; bt[at + q] = run_t; }
      run_v += v[q];
      run_t += t[q];
    }
    carry_v += all_v;
    carry_t += all_t;
  }
  if (threadIdx.x == 0) { A.totals[2 * vol] = carry_v; A.totals[2 * vol + 1] = carry_t; }
}

__global__ __launch_bounds__(256) void k_mc_offsets(const SurfaceArgs A) {
  // the totals are below 2^31 each and there are fewer than 2^31 volumes: the sums fit i64.  Lane t sums the volumes
  // [t m, (t + 1) m), adds up the lanes' sums before its own, and walks its volumes again with the running offset
  __shared__ long long sums[2][256];
  const long long F = A.F, m = (F + 255) / 256;
  const long long lo = (long long)threadIdx.x * m < F ? (long long)threadIdx.x * m : F, hi = lo + m < F ? lo + m : F;
  long long sv = 0, st = 0;
  for (long long f = lo; f < hi; ++f) { sv += A.totals[2 * f]; st += A.totals[2 * f + 1]; }
  sums[0][threadIdx.x] = sv;
  sums[1][threadIdx.x] = st;
  __syncthreads();
  long long run_v = 0, run_t = 0;
  for (unsigned w = 0; w < threadIdx.x; ++w) { run_v += sums[0][w]; run_t += sums[1][w]; }
  for (long long f = lo; f < hi; ++f) {
    A.offsets[f] = run_v;
    A.offsets[F + 1 + f] = run_t;
    run_v += A.totals[2 * f];
    run_t += A.totals[2 * f + 1];
  }
  if (threadIdx.x == 255) { A.offsets[F] = run_v; A.offsets[2 * F + 1] = run_t; }      // (lane 255's range ends at F: the totals)
}

__global__ __launch_bounds__(256) void k_mc_emit(const SurfaceArgs A) {
  __shared__ unsigned part[5];
  __shared__ uint4 tri_rows[256];
  tri_rows[threadIdx.x] = *reinterpret_cast<const uint4*>(&MC_TRI[threadIdx.x][0]);
  const Voxel v = voxel_of(A);
  const bool in = v.n < A.n_voxels;
  const size_t ws = (size_t)v.vol * A.n_voxels;
  const unsigned* block_verts = A.block_verts + (size_t)v.vol * A.chunks;
  unsigned code = 0, word = 0;
  if (in) { code = A.code[ws + v.n]; word = A.word[ws + v.n]; }
  const unsigned n_tri = (unsigned)MC_N_TRI[code];
  unsigned all;
  const unsigned tri_at = block_scan<4>(n_tri, part, all);        // (its barriers publish tri_rows too)
  if (!in) return;
  const unsigned flags = word >> WORD_BITS;
  if (flags) {
    const size_t at = (size_t)v.vol * (size_t)A.volume_stride + (size_t)v.n;
    const size_t step[3] = {1, (size_t)A.nx, (size_t)A.nx * (size_t)A.ny};
    const unsigned index[3] = {v.i, v.j, v.k};
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = A.origin[a] + (double)index[a] * A.spacing[a];
    const double iso = (double)A.iso, va = (double)A.volume[at];
    long long id = A.offsets[v.vol] + (long long)(block_verts[v.chunk] + (word & WORD_MASK));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(flags >> a & 1u)) continue;
      const double vb = (double)A.volume[at + step[a]];
      const double t = (iso - va) / (vb - va);
      const double along = A.origin[a] + ((double)index[a] + t) * A.spacing[a];
      if (id < A.vert_capacity) {
        float* out = A.verts + 3 * (size_t)id;
        out[0] = (float)(a == 0 ? along : p[0]);
        out[1] = (float)(a == 1 ? along : p[1]);
        out[2] = (float)(a == 2 ? along : p[2]);
      }
      ++id;
    }
  }
  if (n_tri) {
    const unsigned short* words = A.word + ws;
    const unsigned char* row = reinterpret_cast<const unsigned char*>(&tri_rows[code]);
    const unsigned sy = (unsigned)A.nx, sz = (unsigned)A.nx * (unsigned)A.ny;
    long long face = A.offsets[A.F + 1 + v.vol] + (long long)(A.block_tris[(size_t)v.vol * A.chunks + v.chunk] + tri_at);
    for (unsigned t = 0; t < n_tri; ++t, ++face) {
      int corner[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned e = row[3 * t + c], axis = e >> 2, r = e & 3u;
        // the end of edge e whose axis bit is clear, as offsets (di, dj, dk): it owns the edge
        const unsigned di = axis == 0 ? 0u : r & 1u;
        const unsigned dj = axis == 0 ? r & 1u : (axis == 1 ? 0u : r >> 1);
        const unsigned dk = axis == 2 ? 0u : r >> 1;
        const unsigned owner = v.n + di + dj * sy + dk * sz;      // (a live cell: i + 1, j + 1, k + 1 exist)
        const unsigned ow = words[owner];
        corner[c] = (int)(block_verts[owner >> 8] + (ow & WORD_MASK) + __popc((ow >> WORD_BITS) & ((1u << axis) - 1u)));
      }
      if (face < A.face_capacity) {
        int* out = A.faces + 3 * (size_t)face;
        out[0] = corner[0]; out[1] = corner[1]; out[2] = corner[2];
      }
    }
  }
}

}  // namespace

void launch_surface_count(const SurfaceArgs& a, hipStream_t st) {
  const dim3 grid(a.chunks * (unsigned)a.F);
  BODYFIT_LAUNCH(k_mc_classify, grid, dim3(256), 0, st, a);
  BODYFIT_LAUNCH(k_mc_count, grid, dim3(256), 0, st, a);
  BODYFIT_LAUNCH(k_mc_scan, dim3((unsigned)a.F), dim3(1024), 0, st, a);
  BODYFIT_LAUNCH(k_mc_offsets, dim3(1), dim3(256), 0, st, a);
}

void launch_surface_emit(const SurfaceArgs& a, hipStream_t st) {
  BODYFIT_LAUNCH(k_mc_emit, dim3(a.chunks * (unsigned)a.F), dim3(256), 0, st, a);
}

}  // namespace bodyfit
