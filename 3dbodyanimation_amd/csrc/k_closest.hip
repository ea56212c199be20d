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
// NaN never wins.  The four waves' results meet in LDS; with few query tiles (one frame, or a few markers per frame) the
// reference range is also split over blockIdx.y and k_closest_reduce folds the splits' partial rows: every fold is by (value,
// then index), so the outputs are bit-identical whatever the split, the frame count and the other frames hold.
// Ragged sets: offset[0] = 0 and offset[F] = the set's row count (the tile numbering and the packed rows rely on it).
//
// Backward (k_cp_vjp, one launch): dL/dquery_i = -2 g_i (c_index_i - p_i) is one thread per query.  dL/dref_v sums over the
// queries that chose v, in f32, without float atomics and in a fixed order: one thread per reference row in ascending query
// order, or the whole wave for a row more than 64 queries chose.  Either order is a function of the frame's own data only.
//
// The point-set convention, the tile numbering, the folds, the grouping and the host side of the workspace live in
// closest_group_inl.h: the closest-surface search shares them.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "host_state.h"
#include "solver_view.h"

#include "closest_group_inl.h"

namespace bodyfit {

namespace {

constexpr int kTileR = 1024;          // reference points per LDS tile (16 KB as float4)
constexpr int kGroup = 4;             // reference points a wave takes at a time

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
  int f, tile;
  BODYFIT_QUERY_TILE(a.q, a.F, f, tile)
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
  float bd;
  int bx;
  if (!fold_waves(s_d, s_i, best, bi, wave, lane, tid, q0, fq.count, &bd, &bx)) return;
  const size_t row = (size_t)(fq.row0 + (q0 + tid));
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
  float bd;
  int bx;
  fold_splits(a.part_d, a.part_i, a.n_split, a.nq_total, row, &bd, &bx);
  a.dist2[row] = bd;
  a.index[row] = bx;
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

}  // namespace

}  // namespace bodyfit

struct bodyfit_closest { bodyfit::ClosestWorkspace w; };

extern "C" {

int bodyfit_closest_create(int device, bodyfit_closest** out) {
  if (!out) return bodyfit::invalid("bodyfit_closest_create", "null argument");
  bodyfit::ClosestWorkspace w;
  if (int rc = bodyfit::open_workspace("bodyfit_closest_create", device, &w)) return rc;
  *out = new bodyfit_closest{w};
  return BODYFIT_OK;
}

void bodyfit_closest_destroy(bodyfit_closest* h) {
  if (!h) return;
  (void)hipSetDevice(h->w.device);
  bodyfit::release_workspace(&h->w);
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
  HIP_TRY(hipSetDevice(h->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  invalidate(&h->w, d_index);
  ClosestArgs a{};
  a.q = device_set(query); a.r = device_set(ref);
  a.F = n_frames; a.nq_total = n_query_total;
  a.dist2 = d_dist2; a.index = d_index;
  long long tiles;
  if (int rc = query_tiles(fn, query, n_query_total, n_frames, &tiles)) return rc;
  a.n_split = choose_split(h->w.n_cu, tiles, ref->d_offset ? (n_ref_total + n_frames - 1) / n_frames : ref->n_per_frame);
  const bool group = prepare_vjp && n_ref_total > 0;
  if (int rc = reserve_search_scratch(&h->w, a.n_split, n_query_total, group, &a.part_d, &a.part_i)) return rc;
  BODYFIT_LAUNCH(k_closest, dim3((unsigned)tiles, (unsigned)a.n_split), dim3(64 * kWaves), 0, st, a);
  if (a.n_split > 1)
    BODYFIT_LAUNCH(k_closest_reduce, dim3((unsigned)((n_query_total + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  Grouping* g = nullptr;   // (behind the reduction on the stream: the scratch may lie over the partial minima)
  if (group) return build_grouping(&h->w, query, ref, n_frames, n_query_total, n_ref_total, d_index, true, st, &g);
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
  HIP_TRY(hipSetDevice(h->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  VjpArgs a{};
  a.q = device_set(query); a.r = device_set(ref);
  a.F = n_frames; a.nq_total = n_query_total; a.nr_total = n_ref_total;
  a.index = d_index; a.g = d_grad_dist2; a.gq = d_grad_query; a.gr = n_ref_total > 0 ? d_grad_ref : nullptr;
  a.qblocks = a.gq ? (unsigned)((n_query_total + 255) / 256) : 0u;
  const unsigned rblocks = a.gr ? (unsigned)((n_ref_total + 255) / 256) : 0u;
  if (a.gr) {
    Grouping* g = nullptr;
    if (int rc = kept_or_built_grouping(&h->w, query, ref, n_frames, n_query_total, n_ref_total, d_index, st, &g)) return rc;
    a.cnt = g->cnt; a.start = g->start; a.sorted = g->sorted;
  }
  if (a.qblocks + rblocks) BODYFIT_LAUNCH(k_cp_vjp, dim3(a.qblocks + rblocks), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
