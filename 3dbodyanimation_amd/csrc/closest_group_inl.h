// closest_group_inl.h — the skeleton the closest-point search (k_closest.hip) and the closest-surface search
// (k_closest_surface.hip) share; either file keeps what is specific to its search.  Included once per translation unit;
// everything has internal linkage.  Device: the per-frame point-set convention; the numbering of the query tiles
// (BODYFIT_QUERY_TILE); the (value, index) order of every minimum fold (better) and the folds over the waves of a workgroup and
// over the blockIdx.y splits (fold_waves, fold_splits); the grouping of the queries by the reference row they chose (rows =
// reference points there, faces here), which the scatter-free backward of either needs.  Host: check_set, reserve, and
// ClosestWorkspace, the part of either handle that the helpers for the device, the tile count, the split, the scratch and the
// kept groupings work on.
// What rests on these pieces alone: index is the LOWEST index of the minimum whatever the split, the wave a candidate fell to
// and the other frames hold (a minimum by `better` does not depend on how the set was partitioned), and every summation order
// of a backward is a function of the frame's own data.
//
// Grouping: the queries grouped by reference row, each group in ascending query order: a stable counting sort of the index,
// which depends on the index alone.  INTEGER atomics give a count per row and an arrival slot per query (k_cp_group_count); a
// scan hands every row a segment (k_cp_group_alloc); rows of at most 64 queries are placed by slot and then ordered by rank =
// smaller query ids in the segment, at most 64 reads per query (k_cp_group_place, k_cp_group_rank); a row that more queries
// chose is filled by one wave that walks the frame's index array in order, 64 queries at a time, ballot + prefix count
// (k_cp_group_heavy): linear in the frame's queries.  Where a segment sits differs from run to run (the cursor's atomics); its
// contents and order do not.  The kernels read only the row COUNT of the reference set's frames, never its coordinates.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "host_state.h"

namespace bodyfit {

namespace {

constexpr int kQ = 4;                 // queries per lane
constexpr int kWaves = 4;             // waves per workgroup; they share the queries and split every reference tile
constexpr int kTileQ = 64 * kQ;       // queries per workgroup (BODYFIT_QUERY_TILE on the device, query_tiles on the host)
constexpr int kMaxSplit = 32;         // splits of the reference range over blockIdx.y
constexpr int kMinPerSplit = 256;     // reference rows a split should at least have
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

// ---- the search skeleton: a workgroup of kWaves waves owns the kTileQ queries of one tile of one frame --------------------
// This workgroup's frame and query tile, into the caller's `int f, tile`.  Ragged: frame f owns the tile numbers offset[f] / kTileQ
// + f up to those of f + 1 (at least as many as it has tiles; the grid is nq_total / kTileQ + F wide, the spare ones leave at
// once: q0 >= the frame's count).  A macro on purpose: as a function the numbering is simplified on its own before it is inlined,
// and both search kernels then come out with another scalar prologue than with the text in place.
#define BODYFIT_QUERY_TILE(q, F, f, tile)                                    \
  if ((q).offset) {                                                          \
    const int b = blockIdx.x;                                                \
    int lo = 0, hi = (F);                                                    \
    while (hi - lo > 1) {                                                    \
      const int mid = (lo + hi) >> 1;                                        \
      if ((q).offset[mid] / kTileQ + mid <= b) lo = mid; else hi = mid;      \
    }                                                                        \
    f = lo; tile = b - ((q).offset[lo] / kTileQ + lo);                       \
  } else {                                                                   \
    const int tpf = ((q).n + kTileQ - 1) / kTileQ;                           \
    f = blockIdx.x / tpf; tile = blockIdx.x - f * tpf;                       \
  }

// The waves hold the same queries (lane l of every wave: q0 + l, q0 + 64 + l, ...) and each its own share of the candidates:
// they meet in LDS and thread tid folds query q0 + tid by (value, index).  False: the frame has no such query.
__device__ __forceinline__ bool fold_waves(float (&s_d)[kWaves][kTileQ], int (&s_i)[kWaves][kTileQ], const float (&best)[kQ],
                                           const int (&bi)[kQ], int wave, int lane, int tid, int q0, int count, float* out_d,
                                           int* out_i) {
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    s_d[wave][k * 64 + lane] = best[k];
    s_i[wave][k * 64 + lane] = bi[k];
  }
  __syncthreads();
  if (q0 + tid >= count) return false;
  float bd = s_d[0][tid];
  int bx = s_i[0][tid];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const float d = s_d[w][tid];
    const int i = s_i[w][tid];
    if (better(d, i, bd, bx)) { bd = d; bx = i; }
  }
  *out_d = bd; *out_i = bx;
  return true;
}

// the partial minima of the blockIdx.y splits, [n_split][nq_total], and their fold in the same (value, index) order
__device__ __forceinline__ void fold_splits(const float* part_d, const int* part_i, int n_split, long long nq_total, long long row,
                                            float* out_d, int* out_i) {
  float bd = part_d[row];
  int bx = part_i[row];
  for (int s = 1; s < n_split; ++s) {
    const float d = part_d[(size_t)s * (size_t)nq_total + row];
    const int i = part_i[(size_t)s * (size_t)nq_total + row];
    if (better(d, i, bd, bx)) { bd = d; bx = i; }
  }
  *out_d = bd; *out_i = bx;
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

// what bodyfit_closest and bodyfit_surface both hold, and all the host helpers below work on
struct ClosestWorkspace {
  int device = 0;
  int n_cu = 256;
  char* ws = nullptr;      // scratch of one call: the splits' partial minima, then the grouping's scratch
  size_t ws_bytes = 0;
  Grouping groupings[kGroupings];
  unsigned long long tick = 0;   // the least-recently-used clock of the slots
};

// makes `device` current and reads its compute-unit count into a fresh workspace
int open_workspace(const char* fn, int device, ClosestWorkspace* w) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return bodyfit_internal_fail(BODYFIT_ERR_HIP, (std::string(fn) + ": no such HIP device (there is no CPU path)").c_str());
  HIP_TRY(hipSetDevice(device));
  int n_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  w->device = device;
  w->n_cu = n_cu > 0 ? n_cu : 256;
  return 0;
}

void release_workspace(ClosestWorkspace* w) {
  if (w->ws) (void)hipFree(w->ws);
  for (Grouping& g : w->groupings)
    if (g.buf) (void)hipFree(g.buf);
}

// the width of the search grid (the numbering of BODYFIT_QUERY_TILE), or the failure
int query_tiles(const char* fn, const bodyfit_pointset* query, long long nq, int F, long long* tiles) {
  *tiles = query->d_offset ? nq / kTileQ + F : (long long)F * ((query->n_per_frame + kTileQ - 1) / kTileQ);
  if (*tiles >= (1LL << 31)) return invalid(fn, "too many query tiles");
  return 0;
}

// few query tiles: split the frame's reference rows until the device has about four workgroups per compute unit
int choose_split(int n_cu, long long tiles, long long rows_per_frame) {
  long long split = (4LL * n_cu + tiles - 1) / tiles;
  if (split > rows_per_frame / kMinPerSplit) split = rows_per_frame / kMinPerSplit;
  if (split > kMaxSplit) split = kMaxSplit;
  return split < 1 ? 1 : (int)split;
}

// The scratch of one search: the partial minima of n_split > 1 splits, part_d and part_i (else left as they are), and, with
// `group`, room for the grouping's scratch, which may lie over them: the grouping runs behind the fold on the stream.
int reserve_search_scratch(ClosestWorkspace* w, int n_split, long long nq, bool group, float** part_d, int** part_i) {
  const size_t part = n_split > 1 ? align256((size_t)n_split * (size_t)nq * 4) : 0;
  size_t need = 2 * part;
  if (group && group_scratch_bytes(nq) > need) need = group_scratch_bytes(nq);
  if (int rc = reserve(&w->ws, &w->ws_bytes, need)) return rc;
  if (n_split > 1) {
    *part_d = reinterpret_cast<float*>(w->ws);
    *part_i = reinterpret_cast<int*>(w->ws + part);
  }
  return 0;
}

// d_index is about to change: a grouping kept for this pointer is void
void invalidate(ClosestWorkspace* w, const void* d_index) {
  for (Grouping& g : w->groupings)
    if (g.index == d_index) g.valid = false;
}

// Builds the grouping of d_index on `st` into the slot that held this index before, else the least recently used one.  The
// workspace's scratch must already hold group_scratch_bytes(nq).  keep: later VJP calls with this d_index may use it.
int build_grouping(ClosestWorkspace* h, const bodyfit_pointset* query, const bodyfit_pointset* ref, int F, long long nq,
                   long long nr, const int32_t* d_index, bool keep, hipStream_t st, Grouping** out) {
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

// the grouping a search kept for this correspondence, or, where none prepared it, one built now for this call only
int kept_or_built_grouping(ClosestWorkspace* w, const bodyfit_pointset* query, const bodyfit_pointset* ref, int F, long long nq,
                           long long nr, const int32_t* d_index, hipStream_t st, Grouping** out) {
  *out = nullptr;
  for (Grouping& c : w->groupings)
    if (c.matches(d_index, query, ref, F, nq, nr)) *out = &c;
  if (*out) {
    (*out)->used = ++w->tick;
    return 0;
  }
  if (int rc = reserve(&w->ws, &w->ws_bytes, group_scratch_bytes(nq))) return rc;
  return build_grouping(w, query, ref, F, nq, nr, d_index, false, st, out);
}

}  // namespace

}  // namespace bodyfit
