// raster_handle.h — the bodyfit_raster handle, shared by the translation units that work on it: k_raster.hip (create, destroy, the
// render and the visibility), k_raster_rows.hip (depth and interpolation rows), k_raster_shade.hip (attribute shading and image
// samples), k_raster_edges.hip (silhouette-edge antialiasing), k_edt.hip (the distance transform), k_texture.hip and k_light.hip;
// and what their entries check alike, each rule with its one message.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/bodyfit.h"
#include "host_state.h"

struct RsFace;   // a face's 96-byte record of one render (k_raster.hip)

struct bodyfit_raster {
  int device = 0, nV = 0, nF = 0, W = 0, H = 0, tilesX = 0, tilesY = 0;
  int* d_faces = nullptr;
  int* d_adj = nullptr;                         // [n_faces][3]: the lowest-id other face on edge (corner e, corner e + 1), or -1
  unsigned* d_totals = nullptr;                 // [0] entries, [1] the longest list, [2] scratch_word(), [3] unused
  RsFace* d_recs = nullptr;      size_t recsCap = 0;      // records
  unsigned* d_tiles = nullptr;   size_t tilesCap = 0;     // tiles: count | cursor | offset
  int* d_entries = nullptr;      size_t entriesCap = 0;   // face ids
  int32_t* d_edt = nullptr;      size_t edtCap = 0;       // distance transform: seed columns and envelope stacks (k_edt.hip)
  unsigned lastTotals[2] = {0, 0};
  // one u32 on the device that a call may use between its own kernels (calls on one handle are ordered; the render uses
  // d_totals[0] and [1] only)
  unsigned* scratch_word() const { return d_totals + 2; }
  ~bodyfit_raster() {
    for (void* q : {(void*)d_faces, (void*)d_adj, (void*)d_totals, (void*)d_recs, (void*)d_tiles, (void*)d_entries, (void*)d_edt})
      if (q) (void)hipFree(q);
  }
};

namespace bodyfit {

template <typename T>
int rs_grow(T** p, size_t* have, size_t want) {
  if (want <= *have) return BODYFIT_OK;
  if (*p) { HIP_TRY(hipFree(*p)); *p = nullptr; *have = 0; }   // (synchronises the device: nothing of ours is in flight on it)
  want += want / 4;
  void* q = nullptr;
  HIP_TRY(hipMalloc(&q, want * sizeof(T)));
  *p = static_cast<T*>(q);
  *have = want;
  return BODYFIT_OK;
}

// (device) frame of packed row `row` of a ragged row set: the largest f with offset[f] <= row (closest_group_inl.h's frame_of)
__device__ __forceinline__ int rs_frame_of(const int* __restrict__ offset, int F, long long row) {
  int lo = 0, hi = F;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offset[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- what the entries check alike.  Each returns BODYFIT_OK or the rejection, and an entry calls them in its OWN order between its
// own checks: the first rule an argument list breaks decides the status and the message, and that order is part of each entry.
inline int rs_check_handle(const char* fn, const bodyfit_raster* r, int n_frames) {
  if (!r) return invalid_arg(fn, "handle is NULL");
  if (n_frames < 0) return invalid_arg(fn, "negative n_frames");
  return BODYFIT_OK;
}

inline bool rs_intrinsics_ok(double fx, double fy, double cx, double cy) {
  return fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy);
}

inline int rs_check_intrinsics(const char* fn, double fx, double fy, double cx, double cy) {
  if (!rs_intrinsics_ok(fx, fy, cx, cy)) return invalid_arg(fn, "fx and fy must be positive, and the intrinsics finite");
  return BODYFIT_OK;
}

inline int rs_check_channels(const char* fn, int n_channels) {
  if (n_channels < 1 || n_channels > 4) return invalid_arg(fn, "n_channels outside 1 .. 4");
  return BODYFIT_OK;
}

inline int rs_check_verts_stride(const char* fn, const bodyfit_raster* r, long long verts_frame_stride) {
  if (verts_frame_stride < 3ll * r->nV) return invalid_arg(fn, "verts_frame_stride below 3 n_verts");
  return BODYFIT_OK;
}

inline int rs_check_pixels(const char* fn, const bodyfit_raster* r, int n_frames) {
  if ((long long)r->W * r->H * n_frames >= (1ll << 39)) return invalid_arg(fn, "2^39 pixels or more in one call");
  return BODYFIT_OK;
}

// a row set of the depth and interpolation rows: the whole image (no d_pixel), n_rows / n_frames listed pixels per frame, or a
// ragged list (d_offset)
inline int rs_check_row_set(const char* fn, const bodyfit_raster* r, int n_frames, const int32_t* d_pixel, const int32_t* d_offset,
                            long long n_rows) {
  if (d_offset && !d_pixel) return invalid_arg(fn, "d_offset without d_pixel");
  if (!d_pixel && n_rows != (long long)r->W * r->H * n_frames) return invalid_arg(fn, "without d_pixel n_rows must be n_frames H W");
  if (n_rows >= (1ll << 31) - 4096) return invalid_arg(fn, "2^31 rows or more in one call");
  if (n_rows > 0 && n_frames == 0) return invalid_arg(fn, "rows without frames");
  if (d_pixel && !d_offset && n_frames > 0 && n_rows % n_frames != 0)
    return invalid_arg(fn, "a uniform row set needs n_rows divisible by n_frames");
  return BODYFIT_OK;
}

// launch(std::integral_constant<int, C>) for the kernels instantiated per channel count: the entries have checked the range, and
// any value other than 1, 2 or 3 takes the 4 instantiation
template <typename Launch>
void rs_dispatch_channels(int n_channels, Launch&& launch) {
  switch (n_channels) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
}

}  // namespace bodyfit
