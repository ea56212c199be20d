// Depth and face-id render of the posed mesh, and the visibility of faces and vertices from a face-id image
// (bodyfit_raster_create, bodyfit_raster_render_device, bodyfit_raster_visibility_device, bodyfit_raster_last_bins;
// include/bodyfit.h: the definition, the contract and the derivation of its constants).  The handle and what the entries of
// every unit on it check alike: raster_handle.h.  The rest of the handle's entries: k_raster_rows.hip (depth and interpolation
// rows), k_raster_shade.hip (attributes, image samples), k_raster_edges.hip (antialiasing), k_edt.hip (distance transform),
// k_texture.hip, k_light.hip.
//
//   k_rs_faces   one thread per (frame, face): the f64 projection of the three corners, the signed area, 1 / Z per corner, the
//                pixel bounding box and the validity, as one 96-byte record (prepared once per call, read by every tile the
//                face touches)
//   k_rs_bin<0>  32 x 8-pixel tiles: how many bounding boxes touch which tile (integer atomics)
//   k_rs_alloc   a block-wide scan of 256 tile counts and ONE integer atomic per block: where each tile's list starts.  The
//                order of the lists in memory is immaterial: nothing below depends on it
//   k_rs_bin<1>  the face ids into the lists (in any order: a pixel's answer is a minimum over a total order)
//   k_rs_tiles   one workgroup per (frame, tile), one thread per pixel: the tile's records are staged through LDS 128 at a
//                time; a pixel inside a record's bounding box evaluates the three edge functions RELATIVE TO ITSELF in f64 and
//                keeps (1 / z, face) in registers; the three images are written with plain stores, empty tiles included, so the
//                outputs never depend on what they held
//   k_rs_visible one thread per pixel of a face-id image: the constant 1 into the face's and its corners' bytes, after a clear
//
// Arithmetic.  The decision "does face t cover pixel s" and the depth order are taken in f64 from differences (corner - pixel),
// never from coefficients of the whole image, so the cancellation is that of the face at the pixel; products are formed
// separately and subtracted (no contraction), so a pixel exactly on an edge gives an exact 0 and the two faces of a shared edge
// see E and -E: no crack, no double miss.  The integer bounding-box test in front only removes pairs whose exact answer is
// "outside".  Only the three outputs are rounded to f32.  No MFMA, no float atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "raster_handle.h"

#pragma clang fp contract(off)

using namespace bodyfit;

struct alignas(16) RsFace {   // 96 bytes, moved in 16-byte pieces (the handle holds a pointer to them: raster_handle.h)
  double u[3], v[3];   // projected corners, pixels
  double inv_area;     // 1 / ((p1 - p0) x (p2 - p0))
  double iz[3];        // 1 / Z per corner
  int bx0, by0, bx1, by1;   // pixels whose centre can lie inside, clipped to the image; bx0 > bx1: not drawn
};
static_assert(sizeof(RsFace) == 96, "RsFace layout");

namespace {

constexpr int kTileW = 32, kTileH = 8;   // one thread per pixel; a wave's store is two full 128-byte rows of depth
constexpr int kTileThreads = kTileW * kTileH;
constexpr int kBatch = 128;              // records staged per pass: 12 KiB of LDS

__global__ __launch_bounds__(256) void k_rs_faces(const float* __restrict__ verts, long long frame_stride,
                                                  const int* __restrict__ faces, int nF, long long total, double fx,
                                                  double fy, double cx, double cy, float z_near, int cull, int W, int H,
                                                  RsFace* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long frame = i / nF;
  const int f = (int)(i - frame * nF);
  const float* c = verts + frame * frame_stride;
  RsFace r;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const size_t id = (size_t)faces[3 * f + k];
    const float X = c[3 * id], Y = c[3 * id + 1], Z = c[3 * id + 2];
    // (a NaN fails every comparison; X - X is NaN for an infinity)
    if (!(X - X == 0.0f) || !(Y - Y == 0.0f) || !(Z - Z == 0.0f) || !(Z >= z_near)) ok = false;
    const double zd = ok ? (double)Z : 1.0;
    r.u[k] = fx * ((double)X / zd) + cx;
    r.v[k] = fy * ((double)Y / zd) + cy;
    r.iz[k] = 1.0 / zd;
  }
  const double area = (r.u[1] - r.u[0]) * (r.v[2] - r.v[0]) - (r.u[2] - r.u[0]) * (r.v[1] - r.v[0]);
  if (!(area != 0.0) || !(area - area == 0.0)) ok = false;
  if (cull && !(area < 0.0)) ok = false;    // front: the normal (v1 - v0) x (v2 - v0) points to the camera
  r.inv_area = ok ? 1.0 / area : 0.0;
  r.bx0 = r.by0 = 1; r.bx1 = r.by1 = 0;
  if (ok) {
    const double x0 = ceil(fmin(r.u[0], fmin(r.u[1], r.u[2]))), x1 = floor(fmax(r.u[0], fmax(r.u[1], r.u[2])));
    const double y0 = ceil(fmin(r.v[0], fmin(r.v[1], r.v[2]))), y1 = floor(fmax(r.v[0], fmax(r.v[1], r.v[2])));
    if (x1 >= 0.0 && y1 >= 0.0 && x0 <= (double)(W - 1) && y0 <= (double)(H - 1) && x0 <= x1 && y0 <= y1) {
      r.bx0 = (int)fmax(x0, 0.0); r.bx1 = (int)fmin(x1, (double)(W - 1));
      r.by0 = (int)fmax(y0, 0.0); r.by1 = (int)fmin(y1, (double)(H - 1));
    }
  }
  out[i] = r;
}

template <bool kFillPass>
__global__ __launch_bounds__(256) void k_rs_bin(const RsFace* __restrict__ recs, int nF, long long total, int tilesX,
                                                int tilesPerFrame, unsigned* __restrict__ count,
                                                const unsigned* __restrict__ offset, unsigned* __restrict__ cursor,
                                                int* __restrict__ entries) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int4 b = *reinterpret_cast<const int4*>(&recs[i].bx0);
  if (b.x > b.z) return;
  const long long frame = i / nF;
  const int f = (int)(i - frame * nF);
  const size_t tb = (size_t)frame * tilesPerFrame;
  for (int ty = b.y / kTileH; ty <= b.w / kTileH; ++ty)
    for (int tx = b.x / kTileW; tx <= b.z / kTileW; ++tx) {
      const size_t t = tb + (size_t)ty * tilesX + tx;
      if (kFillPass) entries[offset[t] + atomicAdd(&cursor[t], 1u)] = f;
      else atomicAdd(&count[t], 1u);
    }
}

__global__ __launch_bounds__(256) void k_rs_alloc(const unsigned* __restrict__ count, long long nT,
                                                  unsigned* __restrict__ offset, unsigned* __restrict__ totals) {
  __shared__ unsigned part[256];
  __shared__ unsigned base, longest;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned c = t < nT ? count[t] : 0u;
  part[threadIdx.x] = c;
  if (threadIdx.x == 0) longest = 0u;
  __syncthreads();
  if (c) atomicMax(&longest, c);
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  if (threadIdx.x == 255) {
    base = part[255] ? atomicAdd(&totals[0], part[255]) : 0u;
    if (longest) atomicMax(&totals[1], longest);   // (the longest list: a statistic, bodyfit_raster_last_bins)
  }
  __syncthreads();
  if (t < nT) offset[t] = base + part[threadIdx.x] - c;
}

__global__ __launch_bounds__(kTileThreads) void k_rs_tiles(const RsFace* __restrict__ recs, int nF, int W, int H,
                                                           int tilesX, int tilesPerFrame,
                                                           const unsigned* __restrict__ count,
                                                           const unsigned* __restrict__ offset,
                                                           const int* __restrict__ entries, float* __restrict__ depth,
                                                           int* __restrict__ face, float* __restrict__ bary) {
  __shared__ RsFace rec[kBatch];
  __shared__ int ids[kBatch];
  const unsigned t = blockIdx.x;
  const unsigned frame = t / (unsigned)tilesPerFrame;
  const int tt = (int)(t - frame * (unsigned)tilesPerFrame);
  const int px = (tt % tilesX) * kTileW + (int)(threadIdx.x % kTileW);
  const int py = (tt / tilesX) * kTileH + (int)(threadIdx.x / kTileW);
  const unsigned n = count[t];
  const unsigned e0 = n ? offset[t] : 0u;
  const RsFace* fr = recs + (size_t)frame * nF;
  const double su = (double)px, sv = (double)py;
  double bw = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0;   // the best 1 / z so far and its weights
  int bf = -1;
  for (unsigned base = 0; base < n; base += kBatch) {
    const unsigned m = min((unsigned)kBatch, n - base);
    __syncthreads();
    // a record is six 16-byte pieces: two threads' worth of a wave read one record's 96 contiguous bytes
    for (unsigned k = threadIdx.x; k < m * 6; k += kTileThreads) {
      const unsigned j = k / 6, q = k - j * 6;
      const int id = entries[e0 + base + j];
      reinterpret_cast<double2*>(&rec[j])[q] = reinterpret_cast<const double2*>(&fr[id])[q];
      if (q == 0) ids[j] = id;
    }
    __syncthreads();
    for (unsigned j = 0; j < m; ++j) {
      const RsFace& r = rec[j];
      if (px < r.bx0 || px > r.bx1 || py < r.by0 || py > r.by1) continue;
      const double d0u = r.u[0] - su, d1u = r.u[1] - su, d2u = r.u[2] - su;
      const double d0v = r.v[0] - sv, d1v = r.v[1] - sv, d2v = r.v[2] - sv;
      const double a0 = (d1u * d2v - d2u * d1v) * r.inv_area;   // (p1 - s) x (p2 - s) / area
      const double a1 = (d2u * d0v - d0u * d2v) * r.inv_area;
      const double a2 = (d0u * d1v - d1u * d0v) * r.inv_area;
      if (!(a0 >= 0.0 && a1 >= 0.0 && a2 >= 0.0)) continue;
      const double w = a0 * r.iz[0] + a1 * r.iz[1] + a2 * r.iz[2];
      const int id = ids[j];
      if (w > bw || (w == bw && id < bf)) { bw = w; bf = id; l0 = a0; l1 = a1; l2 = a2; }
    }
  }
  if (px < W && py < H) {
    const size_t o = ((size_t)frame * H + py) * W + px;
    depth[o] = bf >= 0 ? (float)(1.0 / bw) : std::numeric_limits<float>::infinity();
    face[o] = bf;
    if (bary) { bary[3 * o] = (float)l0; bary[3 * o + 1] = (float)l1; bary[3 * o + 2] = (float)l2; }
  }
}

__global__ __launch_bounds__(256) void k_rs_visible(const int* __restrict__ face_img, long long total,
                                                    long long pixels_per_frame, const int* __restrict__ faces, int nF,
                                                    int nV, unsigned char* __restrict__ face_vis,
                                                    unsigned char* __restrict__ vert_vis) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int f = face_img[i];
  if ((unsigned)f >= (unsigned)nF) return;     // empty (-1), or not a face of this topology
  const long long frame = i / pixels_per_frame;
  if (face_vis) face_vis[frame * nF + f] = 1;
  if (vert_vis)
    for (int k = 0; k < 3; ++k) vert_vis[frame * nV + faces[3 * f + k]] = 1;
}

// (face, edge) -> the lowest-id OTHER face that holds both vertex ids of the edge (corner e, corner (e + 1) % 3), -1 if none or if
// the two ids are equal: the (key, face) pairs sorted, each group scanned once
std::vector<int> rs_adjacency(int nF, const int32_t* faces) {
  struct Item { uint64_t key; int face, edge; };
  std::vector<Item> items;
  items.reserve((size_t)nF * 3);
  for (int f = 0; f < nF; ++f)
    for (int e = 0; e < 3; ++e) {
      const uint32_t a = (uint32_t)faces[3 * f + e], b = (uint32_t)faces[3 * f + (e + 1) % 3];
      if (a != b) items.push_back({((uint64_t)std::min(a, b) << 32) | std::max(a, b), f, e});
    }
  std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.key != y.key ? x.key < y.key : x.face < y.face; });
  std::vector<int> adj((size_t)nF * 3, -1);
  for (size_t g0 = 0; g0 < items.size();) {
    size_t g1 = g0;
    while (g1 < items.size() && items[g1].key == items[g0].key) ++g1;
    for (size_t k = g0; k < g1; ++k)
      for (size_t m = g0; m < g1; ++m)
        if (items[m].face != items[k].face) { adj[3 * (size_t)items[k].face + items[k].edge] = items[m].face; break; }
    g0 = g1;
  }
  return adj;
}

}  // namespace

extern "C" {

int bodyfit_raster_create(int device, int n_verts, int n_faces, const int32_t* faces, int width, int height,
                          bodyfit_raster** out) {
  const char* fn = "bodyfit_raster_create";
  if (!out) return invalid_arg(fn, "out is NULL");
  if (n_verts < 0 || n_faces < 0 || (n_faces > 0 && !faces)) return invalid_arg(fn, "negative count or NULL faces");
  if (width < 1 || height < 1 || width > 16384 || height > 16384) return invalid_arg(fn, "image size outside 1 .. 16384");
  for (long long i = 0; i < 3ll * n_faces; ++i)
    if (faces[i] < 0 || faces[i] >= n_verts) return invalid_arg(fn, "face refers to a vertex out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return bodyfit_internal_fail(BODYFIT_ERR_HIP, "bodyfit_raster_create: no such HIP device (there is no CPU path)");
  HIP_TRY(hipSetDevice(device));
  auto* r = new bodyfit_raster;
  r->device = device; r->nV = n_verts; r->nF = n_faces; r->W = width; r->H = height;
  r->tilesX = (width + kTileW - 1) / kTileW; r->tilesY = (height + kTileH - 1) / kTileH;
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, std::max<size_t>((size_t)n_faces * 3, 1) * sizeof(int));
  if (e == hipSuccess) {
    r->d_faces = static_cast<int*>(q);
    if (n_faces) e = hipMemcpy(r->d_faces, faces, (size_t)n_faces * 3 * sizeof(int), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc(&q, std::max<size_t>((size_t)n_faces * 3, 1) * sizeof(int));
  if (e == hipSuccess) {
    r->d_adj = static_cast<int*>(q);
    if (n_faces) {
      const std::vector<int> adj = rs_adjacency(n_faces, faces);
      e = hipMemcpy(r->d_adj, adj.data(), adj.size() * sizeof(int), hipMemcpyHostToDevice);
    }
  }
  if (e == hipSuccess) { e = hipMalloc(&q, 4 * sizeof(unsigned)); if (e == hipSuccess) r->d_totals = static_cast<unsigned*>(q); }
  if (e != hipSuccess) {
    delete r;
    return bodyfit_internal_fail(BODYFIT_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  }
  *out = r;
  return BODYFIT_OK;
}

void bodyfit_raster_destroy(bodyfit_raster* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  delete r;
}

int bodyfit_raster_render_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                 double fx, double fy, double cx, double cy, float z_near, int cull_backfaces,
                                 float* d_depth, int32_t* d_face, float* d_bary, void* stream) {
  const char* fn = "bodyfit_raster_render_device";
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (!(z_near > 0.0f)) return invalid_arg(fn, "z_near must be positive");
  if (int rc = rs_check_intrinsics(fn, fx, fy, cx, cy)) return rc;
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_depth || !d_face) return invalid_arg(fn, "d_depth or d_face is NULL");
  if (r->nF > 0 && !d_verts) return invalid_arg(fn, "d_verts is NULL");
  if (int rc = rs_check_verts_stride(fn, r, verts_frame_stride)) return rc;
  const int tilesPerFrame = r->tilesX * r->tilesY;
  const long long nT = (long long)n_frames * tilesPerFrame, nR = (long long)n_frames * r->nF;
  if (nT >= (1ll << 31) || nR >= (1ll << 31)) return invalid_arg(fn, "2^31 tiles or records or more in one call");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = rs_grow(&r->d_tiles, &r->tilesCap, (size_t)nT * 3)) return rc;
  unsigned *count = r->d_tiles, *cursor = count + nT, *offset = cursor + nT;
  HIP_TRY(hipMemsetAsync(count, 0, (size_t)nT * 2 * sizeof(unsigned), st));
  r->lastTotals[0] = r->lastTotals[1] = 0;
  if (r->nF > 0) {
    if (int rc = rs_grow(&r->d_recs, &r->recsCap, (size_t)nR)) return rc;
    const unsigned fblocks = (unsigned)((nR + 255) / 256), tblocks = (unsigned)((nT + 255) / 256);
    HIP_TRY(hipMemsetAsync(r->d_totals, 0, 4 * sizeof(unsigned), st));
    BODYFIT_LAUNCH(k_rs_faces, dim3(fblocks), dim3(256), 0, st, d_verts, verts_frame_stride, r->d_faces, r->nF, nR, fx, fy,
                   cx, cy, z_near, cull_backfaces, r->W, r->H, r->d_recs);
    BODYFIT_LAUNCH(k_rs_bin<false>, dim3(fblocks), dim3(256), 0, st, r->d_recs, r->nF, nR, r->tilesX, tilesPerFrame, count,
                   offset, cursor, r->d_entries);
    BODYFIT_LAUNCH(k_rs_alloc, dim3(tblocks), dim3(256), 0, st, count, nT, offset, r->d_totals);
    // the one host synchronisation of a render: two integers that size the tile lists
    HIP_TRY(hipMemcpyAsync(r->lastTotals, r->d_totals, sizeof(r->lastTotals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = rs_grow(&r->d_entries, &r->entriesCap, (size_t)r->lastTotals[0])) return rc;
    if (r->lastTotals[0])
      BODYFIT_LAUNCH(k_rs_bin<true>, dim3(fblocks), dim3(256), 0, st, r->d_recs, r->nF, nR, r->tilesX, tilesPerFrame, count,
                     offset, cursor, r->d_entries);
  }
  BODYFIT_LAUNCH(k_rs_tiles, dim3((unsigned)nT), dim3(kTileThreads), 0, st, r->d_recs, r->nF, r->W, r->H, r->tilesX,
                 tilesPerFrame, count, offset, r->d_entries, d_depth, d_face, d_bary);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_visibility_device(bodyfit_raster* r, const int32_t* d_face, int n_frames, uint8_t* d_face_visible,
                                     uint8_t* d_vert_visible, void* stream) {
  const char* fn = "bodyfit_raster_visibility_device";
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (n_frames == 0 || (!d_face_visible && !d_vert_visible)) return BODYFIT_OK;
  if (!d_face) return invalid_arg(fn, "d_face is NULL");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = rs_check_pixels(fn, r, n_frames)) return rc;
  const long long ppf = (long long)r->W * r->H, total = ppf * n_frames;
  if (d_face_visible && r->nF) HIP_TRY(hipMemsetAsync(d_face_visible, 0, (size_t)n_frames * r->nF, st));
  if (d_vert_visible && r->nV) HIP_TRY(hipMemsetAsync(d_vert_visible, 0, (size_t)n_frames * r->nV, st));
  if (r->nF > 0)
    BODYFIT_LAUNCH(k_rs_visible, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_face, total, ppf, r->d_faces,
                   r->nF, r->nV, d_face_visible, d_vert_visible);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_last_bins(bodyfit_raster* r, long long* n_entries, int* longest) {
  if (!r || !n_entries || !longest) return invalid_arg("bodyfit_raster_last_bins", "null argument");
  *n_entries = r->lastTotals[0];
  *longest = (int)r->lastTotals[1];
  return BODYFIT_OK;
}

}  // extern "C"
