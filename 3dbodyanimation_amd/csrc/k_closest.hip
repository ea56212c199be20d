// k_closest.hip — closest-point search between two per-frame point sets and its reverse-mode gradient
// (bodyfit_closest_points_device, bodyfit_closest_points_vjp_device; declared in include/bodyfit.h).  The 3-D data term of a
// fit: every point of a depth map / scan / marker set against the posed vertices of its frame, or the other way round.
//
// Point sets are f32 xyz rows, per frame either uniform (n rows, a frame stride in floats: the library's padded cloud) or
// ragged (an int32 CSR offset[F + 1] over one packed array).  Per-query values (dist2, index, dL/ddist2) are packed in frame
// order: row offset[f] + i of a ragged query set, f n + i of a uniform one.  Gradients have the layout of their point set.
//
// Forward (k_closest): a workgroup of four waves owns 256 queries of one frame; every lane keeps four of them and their running
// (min, argmin) in registers, all four waves hold the SAME queries.  The frame's reference points go through LDS 1024 at a
// time as padded float4; the waves take the groups of four points of a tile in turn and read each point back at a wave-uniform
// address (one broadcast LDS read, compiled to ds_read_b96, feeds 256 distance evaluations).  A distance is the difference form
// (px - cx)^2 + (py - cy)^2 + (pz - cz)^2 in f32 — the expansion form loses the digits at camera-frame magnitudes — and a
// candidate replaces the running minimum on `<` only, in ascending index order, so equal distances keep the lowest index and a
// NaN never wins.  The four waves' results meet in LDS, reduced by (value, then index).  With few query tiles (one frame, or a
// few markers per frame) the reference range is also split over blockIdx.y; the splits leave partial (min, argmin) rows that
// k_closest_reduce folds in the same (value, index) order.  The minimum of a set and its lowest index do not depend on how the
// set was partitioned, so the outputs are bit-identical whatever the split, the frame count and the other frames hold.
// Ragged sets: offset[0] = 0 and offset[F] = the set's row count (the tile numbering and the packed rows rely on it).
//
// Backward (k_cp_vjp, one launch): dL/dquery_i = -2 g_i (c_index_i - p_i) is one thread per query.  dL/dref_v sums over the
// queries that chose v, in f32, without float atomics and in a fixed order: one thread per reference row in ascending query
// order, or, for a row more than 64 queries chose, the whole wave with lane l taking entries l, l + 64, ... in ascending order
// followed by a fixed butterfly.  Either order is a function of the frame's own data only.
//
// That needs the queries grouped by reference row, each group in ascending query order: a stable counting sort of the index,
// which depends on the index alone.  It is built once per correspondence, by the forward call when asked (prepare_vjp), and
// kept in the handle; a backward whose index no forward prepared builds it first.  INTEGER atomics give a count per row and an
// arrival slot per query (k_cp_group_count); a scan hands every row a segment (k_cp_group_alloc); rows of at most 64 queries
// are placed by slot and then ordered by rank = smaller query ids in the segment, at most 64 reads per query (k_cp_group_place,
// k_cp_group_rank); a row that more queries chose is filled by one wave that walks the frame's index array in order, 64 queries
// at a time, ballot + prefix count (k_cp_group_heavy): linear in the frame's queries.  Where a segment sits differs from run
// to run (the cursor's atomics); its contents and order do not, and no sum depends on anything else.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "host_state.h"
#include "solver_view.h"

namespace bodyfit {

namespace {

constexpr int kQ = 4;                 // queries per lane
constexpr int kWaves = 4;             // waves per workgroup; they share the queries and split every reference tile
constexpr int kTileQ = 64 * kQ;       // queries per workgroup
constexpr int kTileR = 1024;          // reference points per LDS tile (16 KB as float4)
constexpr int kGroup = 4;             // reference points a wave takes at a time
constexpr int kMaxSplit = 32;         // splits of the reference range over blockIdx.y
constexpr int kMinPerSplit = 256;     // reference points a split should at least have
constexpr int kHeavy = 64;            // queries per reference row above which the wave sums the row together

struct PointSet {
  const float* xyz;
  const int* offset;   // [F + 1] or nullptr: uniform
  int n;               // uniform: rows per frame
  long long stride;    // uniform: floats between frames
};

struct FrameRange {
  size_t first;   // float offset of the frame's first row in xyz (and in a gradient of the same layout)
  long long row0; // packed row number of the frame's first row
  int count;
};

__device__ __forceinline__ FrameRange frame_range(const PointSet& s, int f) {
  FrameRange r;
  if (s.offset) {
    const int o0 = s.offset[f], o1 = s.offset[f + 1];
    r.first = 3 * (size_t)o0; r.row0 = o0; r.count = o1 > o0 ? o1 - o0 : 0;
  } else {
    r.first = (size_t)f * (size_t)s.stride; r.row0 = (long long)f * s.n; r.count = s.n;
  }
  return r;
}

// frame of packed row `row` (0 <= row < total rows): the largest f with offset[f] <= row
__device__ __forceinline__ int frame_of(const PointSet& s, int F, long long row) {
  if (!s.offset) return (int)(row / s.n);
  int lo = 0, hi = F;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s.offset[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// (d, i) replaces (bd, bi): smaller value, then lower index (-1, "none", is the largest as unsigned)
__device__ __forceinline__ bool better(float d, int i, float bd, int bi) {
  return d < bd || (d == bd && (unsigned)i < (unsigned)bi);
}

struct ClosestArgs {
  PointSet q, r;
  int F, n_split;
  long long nq_total;
  float* dist2; int* index;      // [nq_total]
  float* part_d; int* part_i;    // [n_split][nq_total] when n_split > 1
};

__global__ __launch_bounds__(64 * kWaves) void k_closest(const ClosestArgs a) {
  __shared__ float4 s_ref[kTileR];
  __shared__ float s_d[kWaves][kTileQ];
  __shared__ int s_i[kWaves][kTileQ];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // this workgroup's frame and query tile.  Ragged: frame f owns the tile numbers offset[f] / kTileQ + f up to those of f + 1
  // (at least as many as it has tiles; the grid is nq_total / kTileQ + F wide, the spare ones leave at once).
  int f, tile;
  if (a.q.offset) {
    const int b = blockIdx.x;
    int lo = 0, hi = a.F;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.q.offset[mid] / kTileQ + mid <= b) lo = mid; else hi = mid;
    }
    f = lo; tile = b - (a.q.offset[lo] / kTileQ + lo);
  } else {
    const int tpf = (a.q.n + kTileQ - 1) / kTileQ;
    f = blockIdx.x / tpf; tile = blockIdx.x - f * tpf;
  }
  const FrameRange fq = frame_range(a.q, f), fr = frame_range(a.r, f);
  const int q0 = tile * kTileQ;
  if (q0 >= fq.count) return;
  float px[kQ], py[kQ], pz[kQ], best[kQ];
  int bi[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int qi = q0 + k * 64 + lane;
    const bool ok = qi < fq.count;
    const float* p = a.q.xyz + fq.first + 3 * (size_t)(ok ? qi : q0);
    px[k] = p[0]; py[k] = p[1]; pz[k] = p[2];
    best[k] = std::numeric_limits<float>::infinity(); bi[k] = -1;
  }
  // this split's share of the frame's reference points: whole groups, the same for every query of the frame
  int c0 = 0, c1 = fr.count;
  if (a.n_split > 1) {
    const int chunk = (((fr.count + a.n_split - 1) / a.n_split + kGroup - 1) / kGroup) * kGroup;
    c0 = min((int)blockIdx.y * chunk, fr.count);
    c1 = min(c0 + chunk, fr.count);
  }
  const float* rbase = a.r.xyz + fr.first;
  for (int t0 = c0; t0 < c1; t0 += kTileR) {
    const int cnt = min(kTileR, c1 - t0), groups = (cnt + kGroup - 1) / kGroup;
    __syncthreads();   // the previous tile has been read by every wave
    const float* src = rbase + 3 * (size_t)t0;
    for (int j = tid; j < 3 * cnt; j += 64 * kWaves) {
      const int pt = j / 3;
      reinterpret_cast<float*>(s_ref)[4 * pt + (j - 3 * pt)] = src[j];
    }
    // the last group's missing points sit infinitely far away: their distance is +inf (or NaN), which never wins a `<`
    for (int j = cnt + tid; j < kGroup * groups; j += 64 * kWaves) {
      const float inf = std::numeric_limits<float>::infinity();
      s_ref[j] = make_float4(inf, inf, inf, 0.f);
    }
    __syncthreads();
    for (int g = wave; g < groups; g += kWaves) {
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        const float4 c = s_ref[kGroup * g + u];
        const int ci = t0 + kGroup * g + u;
#pragma unroll
        for (int k = 0; k < kQ; ++k) {
          const float dx = px[k] - c.x, dy = py[k] - c.y, dz = pz[k] - c.z;
          const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          const bool lt = d < best[k];
          best[k] = lt ? d : best[k];
          bi[k] = lt ? ci : bi[k];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    s_d[wave][k * 64 + lane] = best[k];
    s_i[wave][k * 64 + lane] = bi[k];
  }
  __syncthreads();
  const int qi = q0 + tid;
  if (qi >= fq.count) return;
  float bd = s_d[0][tid];
  int bx = s_i[0][tid];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const float d = s_d[w][tid];
    const int i = s_i[w][tid];
    if (better(d, i, bd, bx)) { bd = d; bx = i; }
  }
  const size_t row = (size_t)(fq.row0 + qi);
  if (a.n_split > 1) {
    a.part_d[(size_t)blockIdx.y * (size_t)a.nq_total + row] = bd;
    a.part_i[(size_t)blockIdx.y * (size_t)a.nq_total + row] = bx;
  } else {
    a.dist2[row] = bd;
    a.index[row] = bx;
  }
}

__global__ __launch_bounds__(256) void k_closest_reduce(const ClosestArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.nq_total) return;
  float bd = a.part_d[row];
  int bx = a.part_i[row];
  for (int s = 1; s < a.n_split; ++s) {
    const float d = a.part_d[(size_t)s * (size_t)a.nq_total + row];
    const int i = a.part_i[(size_t)s * (size_t)a.nq_total + row];
    if (better(d, i, bd, bx)) { bd = d; bx = i; }
  }
  a.dist2[row] = bd;
  a.index[row] = bx;
}

// ---- grouping of the queries by reference row (a function of the index alone: built once per correspondence) ------------
struct GroupArgs {
  PointSet q, r;
  int F;
  long long nq_total, nr_total;
  const int* index;    // [nq_total] frame-local reference row or -1
  int* cnt;            // kept  [nr_total] queries per reference row (zeroed before k_cp_group_count)
  int* start;          // kept  [nr_total] first entry of the row's segment in `sorted`
  int* sorted;         // kept  [nq_total] the segments, each in ascending query row
  int* slot;           // scratch [nq_total] arrival number of the query in its row
  int* rowid;          // scratch [nq_total] packed reference row of the query, -1: none
  int* perm;           // scratch [nq_total] the segments, arbitrary order inside
  int* cursor;         // scratch [1] entries handed out so far (zeroed before k_cp_group_alloc)
};

__global__ __launch_bounds__(256) void k_cp_group_count(const GroupArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.nq_total) return;
  const int f = frame_of(a.q, a.F, row);
  const FrameRange fr = frame_range(a.r, f);
  const int v = a.index[row];
  const bool ok = v >= 0 && v < fr.count;   // (an index out of the frame's range counts as "none")
  const long long rr = fr.row0 + v;
  a.rowid[row] = ok ? (int)rr : -1;
  a.slot[row] = ok ? atomicAdd(&a.cnt[rr], 1) : 0;
}

// a segment of cnt[row] entries for every reference row: every thread takes kAllocRows consecutive rows, an exclusive scan of the
// threads' sums inside the workgroup, ONE atomic on the cursor per workgroup of 4096 rows (one per 256 rows was measured to
// dominate the whole grouping: thousands of atomics on one address)
constexpr int kAllocRows = 16;

__global__ __launch_bounds__(256) void k_cp_group_alloc(const GroupArgs a) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const long long row0 = ((long long)blockIdx.x * 256 + threadIdx.x) * kAllocRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c[kAllocRows];
  int n = 0;
#pragma unroll
  for (int k = 0; k < kAllocRows; ++k) {
    c[k] = row0 + k < a.nr_total ? a.cnt[row0 + k] : 0;
    n += c[k];
  }
  int incl = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = total > 0 ? atomicAdd(a.cursor, total) : 0;
  }
  __syncthreads();
  int at = s_base + incl - n;
  for (int w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
  for (int k = 0; k < kAllocRows; ++k) {
    if (row0 + k < a.nr_total) a.start[row0 + k] = at;
    at += c[k];
  }
}

__global__ __launch_bounds__(256) void k_cp_group_place(const GroupArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.nq_total) return;
  const int rr = a.rowid[row];
  if (rr >= 0 && a.cnt[rr] <= kHeavy) a.perm[a.start[rr] + a.slot[row]] = (int)row;
}

// rows of at most kHeavy queries: a query's place in its segment is the number of smaller query rows in it (<= 64 reads)
__global__ __launch_bounds__(256) void k_cp_group_rank(const GroupArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.nq_total) return;
  const int rr = a.rowid[row];
  if (rr < 0) return;
  const int s = a.start[rr], n = a.cnt[rr];
  if (n > kHeavy) return;
  int rank = 0;
  for (int k = 0; k < n; ++k) rank += a.perm[s + k] < (int)row ? 1 : 0;
  a.sorted[s + rank] = (int)row;
}

// rows that more than kHeavy queries chose: the wave that holds the row walks the frame's index array in order, 64 queries at a
// time, and appends the ones that chose the row (ballot + prefix count): linear in the frame's queries, ascending by construction
__global__ __launch_bounds__(256) void k_cp_group_heavy(const GroupArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = row < a.nr_total;
  const int n = live ? a.cnt[row] : 0;
  unsigned long long heavy = __ballot(n > kHeavy);
  if (!heavy) return;
  const int s = live ? a.start[row] : 0;
  while (heavy) {
    const int src = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const long long hrow = row - lane + src;
    const int hs = __shfl(s, src, 64);
    const int f = frame_of(a.r, a.F, hrow);
    const FrameRange fr = frame_range(a.r, f), fq = frame_range(a.q, f);
    const int v = (int)(hrow - fr.row0);
    int base = 0;
    for (int k0 = 0; k0 < fq.count; k0 += 64) {
      const int i = k0 + lane;
      const bool m = i < fq.count && a.index[fq.row0 + i] == v;
      const unsigned long long mask = __ballot(m);
      if (m) a.sorted[hs + base + __popcll(mask & ((1ull << lane) - 1ull))] = (int)(fq.row0 + i);
      base += __popcll(mask);
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct VjpArgs {
  PointSet q, r;
  int F;
  long long nq_total, nr_total;
  const int* index;    // [nq_total] frame-local reference row or -1
  const float* g;      // [nq_total] dL/ddist2
  float* gq;           // layout of q, or nullptr
  float* gr;           // layout of r, or nullptr
  const int* cnt;      // the grouping (gr only)
  const int* start;
  const int* sorted;
  unsigned qblocks;    // workgroups [0, qblocks): dL/dquery, 256 query rows each; the rest: dL/dref, 256 reference rows each
};

__device__ __forceinline__ void vjp_query_rows(const VjpArgs& a, long long row) {
  if (row >= a.nq_total) return;
  const int f = frame_of(a.q, a.F, row);
  const FrameRange fq = frame_range(a.q, f), fr = frame_range(a.r, f);
  const size_t qoff = fq.first + 3 * (size_t)(row - fq.row0);
  const int v = a.index[row];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (v >= 0 && v < fr.count) {
    const float* p = a.q.xyz + qoff;
    const float* c = a.r.xyz + fr.first + 3 * (size_t)v;
    const float m = -2.f * a.g[row];
    gx = m * (c[0] - p[0]); gy = m * (c[1] - p[1]); gz = m * (c[2] - p[2]);
  }
  a.gq[qoff] = gx; a.gq[qoff + 1] = gy; a.gq[qoff + 2] = gz;
}

__device__ __forceinline__ void vjp_ref_rows(const VjpArgs& a, long long row) {
  const int lane = threadIdx.x & 63;
  const bool live = row < a.nr_total;
  int f = 0, n = 0, s = 0;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  size_t roff = 0;
  if (live) {
    f = frame_of(a.r, a.F, row);
    const FrameRange fr = frame_range(a.r, f);
    roff = fr.first + 3 * (size_t)(row - fr.row0);
    cx = a.r.xyz[roff]; cy = a.r.xyz[roff + 1]; cz = a.r.xyz[roff + 2];
    n = a.cnt[row]; s = a.start[row];
  }
  float ax = 0.f, ay = 0.f, az = 0.f;
  // the query rows of frame f: packed row i sits at float q_first + 3 (i - q_row0)
  if (live && n <= kHeavy && n > 0) {
    const FrameRange fq = frame_range(a.q, f);
    for (int k = 0; k < n; ++k) {
      const int i = a.sorted[s + k];
      const float* p = a.q.xyz + fq.first + 3 * (size_t)(i - fq.row0);
      const float m = 2.f * a.g[i];
      ax = fmaf(m, cx - p[0], ax); ay = fmaf(m, cy - p[1], ay); az = fmaf(m, cz - p[2], az);
    }
  }
  // rows that many queries chose: the wave sums them together, lane l entries l, l + 64, ... then a butterfly
  unsigned long long heavy = __ballot(live && n > kHeavy);
  while (heavy) {
    const int src = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const int hf = __shfl(f, src, 64), hn = __shfl(n, src, 64), hs = __shfl(s, src, 64);
    const float hx = __shfl(cx, src, 64), hy = __shfl(cy, src, 64), hz = __shfl(cz, src, 64);
    const FrameRange fq = frame_range(a.q, hf);
    float tx = 0.f, ty = 0.f, tz = 0.f;
    for (int k = lane; k < hn; k += 64) {
      const int i = a.sorted[hs + k];
      const float* p = a.q.xyz + fq.first + 3 * (size_t)(i - fq.row0);
      const float m = 2.f * a.g[i];
      tx = fmaf(m, hx - p[0], tx); ty = fmaf(m, hy - p[1], ty); tz = fmaf(m, hz - p[2], tz);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      tx += __shfl_xor(tx, d, 64); ty += __shfl_xor(ty, d, 64); tz += __shfl_xor(tz, d, 64);
    }
    if (lane == src) { ax = tx; ay = ty; az = tz; }
  }
  if (live) { a.gr[roff] = ax; a.gr[roff + 1] = ay; a.gr[roff + 2] = az; }
}

// one launch for both gradients (the branch is uniform over a workgroup)
__global__ __launch_bounds__(256) void k_cp_vjp(const VjpArgs a) {
  if (blockIdx.x < a.qblocks) vjp_query_rows(a, (long long)blockIdx.x * 256 + threadIdx.x);
  else vjp_ref_rows(a, (long long)(blockIdx.x - a.qblocks) * 256 + threadIdx.x);
}

int invalid(const char* fn, const char* what) {
  return bodyfit_internal_fail(BODYFIT_ERR_INVALID, (std::string(fn) + ": " + what).c_str());
}

// 0, or the failure.  `total`: the caller's row count of a ragged set; a uniform set's is n_frames n_per_frame.
int check_set(const char* fn, const char* name, const bodyfit_pointset* s, int n_frames, long long* total) {
  const std::string nm(name);
  if (!s) return invalid(fn, (nm + " is NULL").c_str());
  if (s->d_offset) {
    if (*total < 0) return invalid(fn, (nm + ": negative row count").c_str());
  } else {
    if (s->n_per_frame < 0) return invalid(fn, (nm + ": negative n_per_frame").c_str());
    if (s->frame_stride < 3LL * s->n_per_frame) return invalid(fn, (nm + ": frame_stride < 3 n_per_frame").c_str());
    *total = (long long)n_frames * s->n_per_frame;
  }
  if (*total > 0 && !s->d_xyz) return invalid(fn, (nm + ": d_xyz is NULL").c_str());
  if (*total >= (1LL << 31) - 4096) return invalid(fn, (nm + ": more than 2^31 rows").c_str());
  return 0;
}

PointSet device_set(const bodyfit_pointset* s) { return PointSet{s->d_xyz, s->d_offset, s->n_per_frame, s->frame_stride}; }

constexpr int kGroupings = 4;   // correspondences a handle keeps (a bidirectional term runs two forwards before its backwards)

// the grouping of one correspondence, and what it was built from
struct Grouping {
  bool valid = false;
  const void* index = nullptr;
  const void* q_offset = nullptr;
  const void* r_offset = nullptr;
  int F = 0, q_n = 0, r_n = 0;
  long long nq = 0, nr = 0;
  unsigned long long used = 0;
  char* buf = nullptr;
  size_t bytes = 0;
  int *cnt = nullptr, *start = nullptr, *sorted = nullptr;
  bool matches(const void* ix, const bodyfit_pointset* q, const bodyfit_pointset* r, int F_, long long nq_, long long nr_) const {
    return valid && index == ix && q_offset == q->d_offset && r_offset == r->d_offset && F == F_ && nq == nq_ && nr == nr_ &&
           (q->d_offset || q_n == q->n_per_frame) && (r->d_offset || r_n == r->n_per_frame);
  }
};

}  // namespace

}  // namespace bodyfit

struct bodyfit_closest {
  int device = 0;
  int n_cu = 256;
  char* ws = nullptr;      // scratch of one call: the splits' partial minima, then the grouping's scratch
  size_t ws_bytes = 0;
  bodyfit::Grouping groupings[bodyfit::kGroupings];
  unsigned long long tick = 0;
};

namespace {

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// `*p` holds at least `bytes` (growing frees the old block, which waits for the device: calls on a handle are ordered)
int reserve(char** p, size_t* have, size_t bytes) {
  if (bytes <= *have) return 0;
  if (*p) { HIP_TRY(hipFree(*p)); *p = nullptr; *have = 0; }
  bytes += bytes / 4;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), bytes));
  *have = bytes;
  return 0;
}

size_t group_scratch_bytes(long long nq) { return 3 * align256((size_t)nq * 4 + 4) + 256; }

// Builds the grouping of d_index on `st` into the slot that held this index before, else the least recently used one.  The
// handle's scratch must already hold group_scratch_bytes(nq).  keep: later VJP calls with this d_index may use it.
int build_grouping(bodyfit_closest* h, const bodyfit_pointset* query, const bodyfit_pointset* ref, int F, long long nq,
                   long long nr, const int32_t* d_index, bool keep, hipStream_t st, bodyfit::Grouping** out) {
  using namespace bodyfit;
  Grouping* g = nullptr;
  for (Grouping& c : h->groupings)
    if (c.index == d_index) { g = &c; break; }
  if (!g) {
    g = &h->groupings[0];
    for (Grouping& c : h->groupings)
      if (!c.valid && g->valid) g = &c;
      else if (c.valid == g->valid && c.used < g->used) g = &c;
  }
  g->valid = false;
  const size_t a_nr = align256(((size_t)nr + 1) * 4), a_nq = align256((size_t)nq * 4 + 4);
  if (int rc = reserve(&g->buf, &g->bytes, 2 * a_nr + a_nq)) return rc;
  g->cnt = reinterpret_cast<int*>(g->buf);
  g->start = reinterpret_cast<int*>(g->buf + a_nr);
  g->sorted = reinterpret_cast<int*>(g->buf + 2 * a_nr);
  GroupArgs a{};
  a.q = device_set(query); a.r = device_set(ref);
  a.F = F; a.nq_total = nq; a.nr_total = nr; a.index = d_index;
  a.cnt = g->cnt; a.start = g->start; a.sorted = g->sorted;
  a.slot = reinterpret_cast<int*>(h->ws);
  a.rowid = reinterpret_cast<int*>(h->ws + a_nq);
  a.perm = reinterpret_cast<int*>(h->ws + 2 * a_nq);
  a.cursor = reinterpret_cast<int*>(h->ws + 3 * a_nq);
  HIP_TRY(hipMemsetAsync(a.cnt, 0, (size_t)nr * 4, st));
  HIP_TRY(hipMemsetAsync(a.cursor, 0, 4, st));
  const unsigned qblocks = (unsigned)((nq + 255) / 256), rblocks = (unsigned)((nr + 255) / 256);
  if (qblocks) {
    BODYFIT_LAUNCH(k_cp_group_count, dim3(qblocks), dim3(256), 0, st, a);
    BODYFIT_LAUNCH(k_cp_group_alloc, dim3((unsigned)((nr + 256 * kAllocRows - 1) / (256 * kAllocRows))), dim3(256), 0, st, a);
    BODYFIT_LAUNCH(k_cp_group_place, dim3(qblocks), dim3(256), 0, st, a);
    BODYFIT_LAUNCH(k_cp_group_rank, dim3(qblocks), dim3(256), 0, st, a);
    BODYFIT_LAUNCH(k_cp_group_heavy, dim3(rblocks), dim3(256), 0, st, a);
  }
  HIP_TRY(hipGetLastError());
  g->index = d_index; g->q_offset = query->d_offset; g->r_offset = ref->d_offset;
  g->q_n = query->n_per_frame; g->r_n = ref->n_per_frame;
  g->F = F; g->nq = nq; g->nr = nr;
  g->used = ++h->tick;
  g->valid = keep;
  *out = g;
  return 0;
}

}  // namespace

extern "C" {

int bodyfit_closest_create(int device, bodyfit_closest** out) {
  if (!out) return bodyfit::invalid("bodyfit_closest_create", "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return bodyfit_internal_fail(BODYFIT_ERR_HIP, "bodyfit_closest_create: no such HIP device (there is no CPU path)");
  HIP_TRY(hipSetDevice(device));
  int n_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  bodyfit_closest* h = new bodyfit_closest;
  h->device = device;
  h->n_cu = n_cu > 0 ? n_cu : 256;
  *out = h;
  return BODYFIT_OK;
}

void bodyfit_closest_destroy(bodyfit_closest* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->ws) (void)hipFree(h->ws);
  for (bodyfit::Grouping& g : h->groupings)
    if (g.buf) (void)hipFree(g.buf);
  delete h;
}

int bodyfit_closest_points_device(bodyfit_closest* h, const bodyfit_pointset* query, const bodyfit_pointset* ref, int n_frames,
                                  long long n_query_total, long long n_ref_total, float* d_dist2, int32_t* d_index,
                                  int prepare_vjp, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_closest_points_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (int rc = check_set(fn, "query", query, n_frames, &n_query_total)) return rc;
  if (int rc = check_set(fn, "ref", ref, n_frames, &n_ref_total)) return rc;
  if (!d_dist2 || !d_index) return invalid(fn, "d_dist2 / d_index is NULL");
  if (!h) return invalid(fn, "null handle");
  if (n_frames == 0 || n_query_total == 0) return BODYFIT_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // d_index is about to change: a grouping kept for this pointer is void
  for (Grouping& g : h->groupings)
    if (g.index == d_index) g.valid = false;
  ClosestArgs a{};
  a.q = device_set(query); a.r = device_set(ref);
  a.F = n_frames; a.nq_total = n_query_total;
  a.dist2 = d_dist2; a.index = d_index;
  const long long tiles = query->d_offset ? n_query_total / kTileQ + n_frames
                                          : (long long)n_frames * ((query->n_per_frame + kTileQ - 1) / kTileQ);
  if (tiles >= (1LL << 31)) return invalid(fn, "too many query tiles");
  // few query tiles: split the reference range until the device has about four workgroups per compute unit
  const long long ref_per_frame = ref->d_offset ? (n_ref_total + n_frames - 1) / n_frames : ref->n_per_frame;
  long long split = (4LL * h->n_cu + tiles - 1) / tiles;
  if (split > ref_per_frame / kMinPerSplit) split = ref_per_frame / kMinPerSplit;
  if (split > kMaxSplit) split = kMaxSplit;
  if (split < 1) split = 1;
  a.n_split = (int)split;
  const bool group = prepare_vjp && n_ref_total > 0;
  const size_t part = a.n_split > 1 ? align256((size_t)a.n_split * (size_t)n_query_total * 4) : 0;
  size_t need = 2 * part;
  if (group && group_scratch_bytes(n_query_total) > need) need = group_scratch_bytes(n_query_total);
  if (int rc = reserve(&h->ws, &h->ws_bytes, need)) return rc;
  if (a.n_split > 1) {
    a.part_d = reinterpret_cast<float*>(h->ws);
    a.part_i = reinterpret_cast<int*>(h->ws + part);
  }
  BODYFIT_LAUNCH(k_closest, dim3((unsigned)tiles, (unsigned)a.n_split), dim3(64 * kWaves), 0, st, a);
  if (a.n_split > 1)
    BODYFIT_LAUNCH(k_closest_reduce, dim3((unsigned)((n_query_total + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  if (group) {   // (behind the reduction on the stream: the scratch may lie over the partial minima)
    Grouping* g = nullptr;
    if (int rc = build_grouping(h, query, ref, n_frames, n_query_total, n_ref_total, d_index, true, st, &g)) return rc;
  }
  return BODYFIT_OK;
}

int bodyfit_closest_points_vjp_device(bodyfit_closest* h, const bodyfit_pointset* query, const bodyfit_pointset* ref,
                                      int n_frames, long long n_query_total, long long n_ref_total, const int32_t* d_index,
                                      const float* d_grad_dist2, float* d_grad_query, float* d_grad_ref, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_closest_points_vjp_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (int rc = check_set(fn, "query", query, n_frames, &n_query_total)) return rc;
  if (int rc = check_set(fn, "ref", ref, n_frames, &n_ref_total)) return rc;
  if (n_query_total > 0 && (!d_index || !d_grad_dist2)) return invalid(fn, "d_index / d_grad_dist2 is NULL");
  if (!h) return invalid(fn, "null handle");
  if (n_frames == 0 || (!d_grad_query && !d_grad_ref)) return BODYFIT_OK;
  if (n_query_total == 0 && (!d_grad_ref || n_ref_total == 0)) return BODYFIT_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  VjpArgs a{};
  a.q = device_set(query); a.r = device_set(ref);
  a.F = n_frames; a.nq_total = n_query_total; a.nr_total = n_ref_total;
  a.index = d_index; a.g = d_grad_dist2; a.gq = d_grad_query; a.gr = n_ref_total > 0 ? d_grad_ref : nullptr;
  a.qblocks = a.gq ? (unsigned)((n_query_total + 255) / 256) : 0u;
  const unsigned rblocks = a.gr ? (unsigned)((n_ref_total + 255) / 256) : 0u;
  if (a.gr) {
    Grouping* g = nullptr;
    for (Grouping& c : h->groupings)
      if (c.matches(d_index, query, ref, n_frames, n_query_total, n_ref_total)) g = &c;
    if (g) {
      g->used = ++h->tick;
    } else {   // no forward prepared this correspondence: group now, for this call only
      if (int rc = reserve(&h->ws, &h->ws_bytes, group_scratch_bytes(n_query_total))) return rc;
      if (int rc = build_grouping(h, query, ref, n_frames, n_query_total, n_ref_total, d_index, false, st, &g)) return rc;
    }
    a.cnt = g->cnt; a.start = g->start; a.sorted = g->sorted;
  }
  if (a.qblocks + rblocks) BODYFIT_LAUNCH(k_cp_vjp, dim3(a.qblocks + rblocks), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
