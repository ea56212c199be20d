// Depth and face-id render of the posed mesh, the visibility of faces and vertices from a face-id image, and the depth rows
// (bodyfit_raster_*, include/bodyfit.h: the definition, the contract and the derivation of its constants).
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
//   k_rs_depth_rows one thread per depth row (a pixel of a frame): the ray through the pixel against the plane of the face the
//                face-id image holds there: z, the object-space barycentrics and the direction m with dz/dcorner_a = beta_a m
//                (bodyfit_raster_depth_rows_device), f64 throughout, plain stores
//   k_rs_interp_rows<C, kIndexed> one thread per interpolation row: the depth row's face, ray and beta, and the one direction dir
//                with dL/dcorner_c = beta_c dir for upstream gradients in the interpolated attributes and in z
//                (bodyfit_raster_interp_rows_device; kIndexed: the attribute rows of a face from a table of their own, a uv atlas:
//                bodyfit_raster_interp_rows_indexed_device), f64 throughout, plain stores
//   k_rs_shade<C>  one thread per pixel of a render: per-vertex attributes interpolated with the perspective-correct weights
//                (lambda_a / Z_a) / sum, the background where the pixel is void (bodyfit_raster_shade_device)
//   k_rs_sample<C, T>  one thread per (frame, point): the point's projection, the bilinear value of a u8 or f32 image there and
//                the derivative of the cell's patch (bodyfit_raster_sample_device; the patch is bilinear_inl.h's, shared with
//                k_texture.hip)
//   k_rs_edges   one thread per pixel: its right and lower neighbour pairs; where the two face ids differ, the bounded walk from
//                the nearer pixel's face to the silhouette edge that crosses the segment between the two centres, and the blend
//                weight (bodyfit_raster_edges_device)
//   k_rs_edge_blend<C>  one thread per pixel: the blend of an image by the weight image, or its adjoint
//   k_rs_edge_rows<C>   one thread per listed pair: the walk again, and the two "barycentric x direction" rows of the crossing's
//                derivative in the edge's two corners (bodyfit_raster_edge_rows_device)
// bodyfit_raster_distance_device, the distance transform of masks and face-id images, has its host entry here, on the handle's
// size and workspace; its kernels are k_edt.hip's (edt.h).
//
// Arithmetic.  The decision "does face t cover pixel s" and the depth order are taken in f64 from differences (corner - pixel),
// never from coefficients of the whole image, so the cancellation is that of the face at the pixel; products are formed
// separately and subtracted (no contraction), so a pixel exactly on an edge gives an exact 0 and the two faces of a shared edge
// see E and -E: no crack, no double miss.  The integer bounding-box test in front only removes pairs whose exact answer is
// "outside".  Only the three outputs are rounded to f32.  No MFMA, no float atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../include/bodyfit.h"
#include "bilinear_inl.h"
#include "bodyfit_device.h"
#include "edt.h"
#include "host_state.h"
#include "raster_view.h"
#include "solver_view.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTileW = 32, kTileH = 8;   // one thread per pixel; a wave's store is two full 128-byte rows of depth
constexpr int kTileThreads = kTileW * kTileH;
constexpr int kBatch = 128;              // records staged per pass: 12 KiB of LDS

struct alignas(16) RsFace {   // 96 bytes, moved in 16-byte pieces
  double u[3], v[3];   // projected corners, pixels
  double inv_area;     // 1 / ((p1 - p0) x (p2 - p0))
  double iz[3];        // 1 / Z per corner
  int bx0, by0, bx1, by1;   // pixels whose centre can lie inside, clipped to the image; bx0 > bx1: not drawn
};
static_assert(sizeof(RsFace) == 96, "RsFace layout");

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

// frame of packed row `row` of a ragged row set: the largest f with offset[f] <= row (closest_group_inl.h's frame_of)
__device__ __forceinline__ int rs_frame_of(const int* __restrict__ offset, int F, long long row) {
  int lo = 0, hi = F;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offset[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// One thread per depth row: the pixel's ray against the plane of the face the face-id image holds there.  A gather of 36
// bytes of corners per row; every operation that decides is f64 and unfused (this file's contract(off)), in the order that
// include/bodyfit.h counts and tests/depth_rows_ref.py restates: e1, e2, n = e1 x e2, d, D = n . d, N0 = n . v0, z = N0 / D,
// x = z d, beta_a = (n . ((v_b - x) x (v_c - x))) / (n . n), m = n / D.  Only the stores round to f32.
__global__ __launch_bounds__(256) void k_rs_depth_rows(const float* __restrict__ verts, long long frame_stride,
                                                       const int* __restrict__ faces, int nF, int F, int W, int H, double fx,
                                                       double fy, double cx, double cy, const int* __restrict__ face_img,
                                                       const int* __restrict__ pixel, const int* __restrict__ offset,
                                                       long long per_frame, long long n_rows, int* __restrict__ index,
                                                       float* __restrict__ z_out, float* __restrict__ bary,
                                                       float* __restrict__ dir) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const long long ppf = (long long)W * H;
  long long frame, pix;
  if (pixel) {
    frame = offset ? rs_frame_of(offset, F, row) : row / per_frame;
    pix = pixel[row];
  } else {
    frame = row / ppf;
    pix = row - frame * ppf;
  }
  int f = -1;
  if (pix >= 0 && pix < ppf) f = face_img[(size_t)frame * (size_t)ppf + (size_t)pix];
  bool ok = (unsigned)f < (unsigned)nF;     // empty (-1), not a face of this topology, or a pixel outside the image
  double zz = 0.0, b[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
  if (ok) {
    const float* c = verts + (size_t)frame * (size_t)frame_stride;
    double v[3][3];
    for (int k = 0; k < 3; ++k) {
      const size_t id = (size_t)faces[3 * f + k];
      for (int a = 0; a < 3; ++a) {
        const float X = c[3 * id + a];
        if (!(X - X == 0.0f)) ok = false;   // (a NaN fails every comparison; X - X is NaN for an infinity)
        v[k][a] = (double)X;
      }
    }
    const double e1x = v[1][0] - v[0][0], e1y = v[1][1] - v[0][1], e1z = v[1][2] - v[0][2];
    const double e2x = v[2][0] - v[0][0], e2y = v[2][1] - v[0][1], e2z = v[2][2] - v[0][2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const long long i = pix / W, j = pix - i * W;
    const double dx = ((double)j - cx) / fx, dy = ((double)i - cy) / fy;
    const double D = (nx * dx + ny * dy) + nz;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    if (!(nn > 0.0) || !(D != 0.0)) ok = false;
    if (ok) {
      const double N0 = (nx * v[0][0] + ny * v[0][1]) + nz * v[0][2];
      zz = N0 / D;
      const double x[3] = {zz * dx, zz * dy, zz};
      const double inv_nn = 1.0 / nn;
      for (int a = 0; a < 3; ++a) {
        const double* vb = v[(a + 1) % 3];
        const double* vc = v[(a + 2) % 3];
        const double px = vb[0] - x[0], py = vb[1] - x[1], pz = vb[2] - x[2];
        const double qx = vc[0] - x[0], qy = vc[1] - x[1], qz = vc[2] - x[2];
        const double wx = py * qz - pz * qy, wy = pz * qx - px * qz, wz = px * qy - py * qx;
        b[a] = ((nx * wx + ny * wy) + nz * wz) * inv_nn;
      }
      m[0] = nx / D; m[1] = ny / D; m[2] = nz / D;
    }
  }
  index[row] = ok ? f : -1;
  if (z_out) z_out[row] = ok ? (float)zz : std::numeric_limits<float>::infinity();
  if (bary)
    for (int a = 0; a < 3; ++a) bary[3 * (size_t)row + a] = ok ? (float)b[a] : 0.0f;
  if (dir)
    for (int a = 0; a < 3; ++a) dir[3 * (size_t)row + a] = ok ? (float)m[a] : 0.0f;
}

// One thread per interpolation row: the depth row's evaluation, operation for operation (so index and beta are the depth rows'
// bits), then the ONE direction that carries dL/dz and dL/dimage to the three corners, dL/dv_c = beta_c dir (include/bodyfit.h,
// INTERPOLATION ROWS).  f64 and unfused, in the order the header counts and tests/interp_ref.py restates:
//   s_a = ((G_0 A_a0 + G_1 A_a1) + G_2 A_a2) + G_3 A_a3 (the products of two f32 are exact in f64), p = s_1 - s_0, q = s_2 - s_0,
//   E = q e1 - p e2 (= sum_a s_a (v_c - v_b): the DIFFERENCES against s_0, so three equal s_a give an exact 0),
//   w = (n x E) (1 / (n . n)) (= sum_a s_a g_a),  k = (w_x d_x + w_y d_y) + w_z,  a = w - k m (= sum_a s_a h_a),
//   dir = g_z m - a,  value_c = (beta_0 A_0c + beta_1 A_1c) + beta_2 A_2c from the unrounded beta.
// C = 0: no attributes, dir = g_z m.  The row reads the upstream gradients at its own (frame, pixel): nothing is gathered before
// the call.  Only the stores round to f32.
template <int C, bool kIndexed>
__global__ __launch_bounds__(256) void k_rs_interp_rows(const float* __restrict__ verts, long long frame_stride,
                                                        const int* __restrict__ faces, int nF, int F, int W, int H, double fx,
                                                        double fy, double cx, double cy, const int* __restrict__ face_img,
                                                        const int* __restrict__ pixel, const int* __restrict__ offset,
                                                        long long per_frame, long long n_rows, const float* __restrict__ attr,
                                                        long long attr_stride, const float* __restrict__ grad_image,
                                                        const float* __restrict__ grad_z, int* __restrict__ index,
                                                        float* __restrict__ bary, float* __restrict__ dir,
                                                        float* __restrict__ value, const int* __restrict__ attr_faces,
                                                        int n_attr_rows) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const long long ppf = (long long)W * H;
  long long frame, pix;
  if (pixel) {
    frame = offset ? rs_frame_of(offset, F, row) : row / per_frame;
    pix = pixel[row];
  } else {
    frame = row / ppf;
    pix = row - frame * ppf;
  }
  int f = -1;
  if (pix >= 0 && pix < ppf) f = face_img[(size_t)frame * (size_t)ppf + (size_t)pix];
  bool ok = (unsigned)f < (unsigned)nF;     // empty (-1), not a face of this topology, or a pixel outside the image
  double b[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
  double val[C > 0 ? C : 1] = {};
  size_t aid[3] = {0, 0, 0};     // the rows of attr: the corners' vertex ids, or (kIndexed) the face's own three entries
  if (kIndexed && C > 0 && ok)
    for (int k = 0; k < 3; ++k) {
      const int e = attr_faces[3 * f + k];
      if ((unsigned)e >= (unsigned)n_attr_rows) ok = false;     // an entry out of range voids the rows of that face
      aid[k] = (size_t)e;
    }
  if (ok) {
    const float* c = verts + (size_t)frame * (size_t)frame_stride;
    size_t id[3];
    double v[3][3];
    for (int k = 0; k < 3; ++k) {
      id[k] = (size_t)faces[3 * f + k];
      if (!kIndexed) aid[k] = id[k];
      for (int a = 0; a < 3; ++a) {
        const float X = c[3 * id[k] + a];
        if (!(X - X == 0.0f)) ok = false;   // (a NaN fails every comparison; X - X is NaN for an infinity)
        v[k][a] = (double)X;
      }
    }
    const double e1x = v[1][0] - v[0][0], e1y = v[1][1] - v[0][1], e1z = v[1][2] - v[0][2];
    const double e2x = v[2][0] - v[0][0], e2y = v[2][1] - v[0][1], e2z = v[2][2] - v[0][2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const long long i = pix / W, j = pix - i * W;
    const double dx = ((double)j - cx) / fx, dy = ((double)i - cy) / fy;
    const double D = (nx * dx + ny * dy) + nz;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    if (!(nn > 0.0) || !(D != 0.0)) ok = false;
    if (ok) {
      const double N0 = (nx * v[0][0] + ny * v[0][1]) + nz * v[0][2];
      const double zz = N0 / D;
      const double x[3] = {zz * dx, zz * dy, zz};
      const double inv_nn = 1.0 / nn;
      for (int a = 0; a < 3; ++a) {
        const double* vb = v[(a + 1) % 3];
        const double* vc = v[(a + 2) % 3];
        const double px = vb[0] - x[0], py = vb[1] - x[1], pz = vb[2] - x[2];
        const double qx = vc[0] - x[0], qy = vc[1] - x[1], qz = vc[2] - x[2];
        const double wx = py * qz - pz * qy, wy = pz * qx - px * qz, wz = px * qy - py * qx;
        b[a] = ((nx * wx + ny * wy) + nz * wz) * inv_nn;
      }
      const double m[3] = {nx / D, ny / D, nz / D};
      const size_t at = (size_t)frame * (size_t)ppf + (size_t)pix;
      if (grad_z) {
        const double gz = (double)grad_z[at];
        for (int a = 0; a < 3; ++a) r[a] = gz * m[a];
      }
      if (C > 0) {
        const float* A = attr + (size_t)frame * (size_t)attr_stride;
        double s[3];
        for (int k = 0; k < 3; ++k) {
          double acc = 0.0;
          for (int ch = 0; ch < C; ++ch) {
            const double Ak = (double)A[C * aid[k] + ch];
            const double t = (double)grad_image[C * at + ch] * Ak;
            acc = ch == 0 ? t : acc + t;
            const double bt = b[k] * Ak;
            val[ch] = k == 0 ? bt : val[ch] + bt;
          }
          s[k] = acc;
        }
        const double p = s[1] - s[0], q = s[2] - s[0];
        const double Ex = q * e1x - p * e2x, Ey = q * e1y - p * e2y, Ez = q * e1z - p * e2z;
        const double wx = (ny * Ez - nz * Ey) * inv_nn, wy = (nz * Ex - nx * Ez) * inv_nn, wz = (nx * Ey - ny * Ex) * inv_nn;
        const double kk = (wx * dx + wy * dy) + wz;
        const double a3[3] = {wx - kk * m[0], wy - kk * m[1], wz - kk * m[2]};
        for (int a = 0; a < 3; ++a) r[a] = grad_z ? r[a] - a3[a] : -a3[a];
      }
    }
  }
  index[row] = ok ? f : -1;
  if (bary)
    for (int a = 0; a < 3; ++a) bary[3 * (size_t)row + a] = ok ? (float)b[a] : 0.0f;
  if (dir)
    for (int a = 0; a < 3; ++a) dir[3 * (size_t)row + a] = ok ? (float)r[a] : 0.0f;
  if (C > 0 && value)
    for (int ch = 0; ch < C; ++ch) value[C * (size_t)row + ch] = ok ? (float)val[ch] : 0.0f;
}

// One thread per pixel, neighbouring lanes on neighbouring columns: the face's three ids, the three Z and the 3 C attributes are
// gathered (neighbouring pixels mostly share a face: the gathers hit cache), the image streams.  f64 and unfused, in the order
// include/bodyfit.h counts: q_a = lambda_a / Z_a, S = (q_0 + q_1) + q_2, w_a = q_a / S, image_c = (w_0 a_0c + w_1 a_1c) + w_2 a_2c;
// only the stores round.  bg: the background, by value.
template <int C>
__global__ __launch_bounds__(256) void k_rs_shade(const int* __restrict__ face_img, const float* __restrict__ bary,
                                                  const float* __restrict__ verts, long long verts_stride,
                                                  const float* __restrict__ attr, long long attr_stride,
                                                  const int* __restrict__ faces, int nF, long long ppf, long long total,
                                                  float4 bg, float* __restrict__ image, float* __restrict__ weight) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int t = face_img[o];
  const float l0 = bary[3 * (size_t)o], l1 = bary[3 * (size_t)o + 1], l2 = bary[3 * (size_t)o + 2];
  const float bgc[4] = {bg.x, bg.y, bg.z, bg.w};
  float out[C], w[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < C; ++c) out[c] = bgc[c];
  // (a NaN fails every comparison; x - x is NaN for an infinity)
  bool ok = (unsigned)t < (unsigned)nF && l0 - l0 == 0.0f && l1 - l1 == 0.0f && l2 - l2 == 0.0f && l0 >= 0.0f && l1 >= 0.0f &&
            l2 >= 0.0f;
  if (ok) {
    const size_t frame = (size_t)(o / ppf);
    const float* v = verts + frame * (size_t)verts_stride;
    const float* a = attr + frame * (size_t)attr_stride;
    const size_t i0 = (size_t)faces[3 * t], i1 = (size_t)faces[3 * t + 1], i2 = (size_t)faces[3 * t + 2];
    const float Z0 = v[3 * i0 + 2], Z1 = v[3 * i1 + 2], Z2 = v[3 * i2 + 2];
    float a0[C], a1[C], a2[C];
    for (int c = 0; c < C; ++c) { a0[c] = a[C * i0 + c]; a1[c] = a[C * i1 + c]; a2[c] = a[C * i2 + c]; }
    ok = Z0 - Z0 == 0.0f && Z1 - Z1 == 0.0f && Z2 - Z2 == 0.0f && Z0 > 0.0f && Z1 > 0.0f && Z2 > 0.0f;
    if (ok) {
      const double q0 = (double)l0 / (double)Z0, q1 = (double)l1 / (double)Z1, q2 = (double)l2 / (double)Z2;
      const double S = (q0 + q1) + q2;
      ok = S != 0.0;
      if (ok) {
        const double w0 = q0 / S, w1 = q1 / S, w2 = q2 / S;
        for (int c = 0; c < C; ++c) out[c] = (float)((w0 * (double)a0[c] + w1 * (double)a1[c]) + w2 * (double)a2[c]);
        w[0] = (float)w0; w[1] = (float)w1; w[2] = (float)w2;
      }
    }
  }
  for (int c = 0; c < C; ++c) image[C * (size_t)o + c] = out[c];
  if (weight)
    for (int k = 0; k < 3; ++k) weight[3 * (size_t)o + k] = w[k];
}

// One thread per (frame, point): the f64 projection in the render's order, the cell of the bilinear patch, its 4 C texels
// (loaded before anything is combined: the gathers are what this kernel waits for), the value and the patch's exact derivative.
// T: uint8_t or float texels, used as they are.  Unfused f64; only the stores round.
template <int C, typename T>
__global__ __launch_bounds__(256) void k_rs_sample(const float* __restrict__ points, long long points_stride, long long N,
                                                   long long total, double fx, double fy, double cx, double cy, float z_near,
                                                   const T* __restrict__ image, long long image_stride, int W, int H,
                                                   const unsigned char* __restrict__ gate, float* __restrict__ value,
                                                   unsigned char* __restrict__ valid, float* __restrict__ grad) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const size_t frame = (size_t)(p / N);
  const size_t n = (size_t)p - frame * (size_t)N;
  const float* x = points + frame * (size_t)points_stride + 3 * n;
  const float X = x[0], Y = x[1], Z = x[2];
  bool ok = X - X == 0.0f && Y - Y == 0.0f && Z - Z == 0.0f && Z >= z_near && (!gate || gate[p] != 0);
  double val[C], gu[C], gv[C];
  for (int c = 0; c < C; ++c) val[c] = gu[c] = gv[c] = 0.0;
  if (ok) {
    const double u = fx * ((double)X / (double)Z) + cx, v = fy * ((double)Y / (double)Z) + cy;
    ok = u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1);
    if (ok) {
      const bodyfit::BilinearCell cell = bodyfit::bilinear_cell(u, v, W, H);
      bodyfit::bilinear_patch<C, T>(image + frame * (size_t)image_stride, W, cell, val, gu, gv);
    }
  }
  valid[p] = ok ? 1 : 0;
  for (int c = 0; c < C; ++c) value[C * (size_t)p + c] = (float)val[c];
  if (grad)
    for (int c = 0; c < C; ++c) {
      grad[2 * (C * (size_t)p + c)] = (float)gu[c];
      grad[2 * (C * (size_t)p + c) + 1] = (float)gv[c];
    }
}

// ---- silhouette-edge antialiasing (bodyfit_raster_edges_device, include/bodyfit.h: the definition and its bands) -------------
// One face of the walk: the projection of k_rs_faces (the same operations in the same order), the corner ids and "drawn".
struct AaFace {
  double u[3], v[3];
  int id[3];
  bool drawn;
};

__device__ __forceinline__ void aa_project(const float* __restrict__ c, const int* __restrict__ faces, int f, double fx, double fy,
                                           double cx, double cy, float z_near, int cull, AaFace& r) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const int id = faces[3 * f + k];
    r.id[k] = id;
    const float X = c[3 * (size_t)id], Y = c[3 * (size_t)id + 1], Z = c[3 * (size_t)id + 2];
    if (!(X - X == 0.0f) || !(Y - Y == 0.0f) || !(Z - Z == 0.0f) || !(Z >= z_near)) ok = false;
    const double zd = ok ? (double)Z : 1.0;
    r.u[k] = fx * ((double)X / zd) + cx;
    r.v[k] = fy * ((double)Y / zd) + cy;
  }
  const double area = (r.u[1] - r.u[0]) * (r.v[2] - r.v[0]) - (r.u[2] - r.u[0]) * (r.v[1] - r.v[0]);
  if (!(area != 0.0) || !(area - area == 0.0)) ok = false;
  if (cull && !(area < 0.0)) ok = false;
  r.drawn = ok;
}

struct AaHit {
  int face, edge, steps;   // the face that holds the silhouette edge, the edge (corners edge, (edge + 1) % 3), faces visited
  int ida, idb;            // the vertex ids of the edge's two corners
  double s, num, den, d;   // the crossing's parameter on the edge, the edge's slope num / den = d along / d across, |x* - x_n|
};

// The walk of the definition: from face t, at most BODYFIT_AA_WALK faces.  axis 0: along = u, across = v; axis 1: exchanged.
// c0: the scanline, lo: the lower end of the unit segment, xn: the near pixel's centre on it.  `cur` is left on the final face.
__device__ bool aa_walk(const float* __restrict__ c, const int* __restrict__ faces, const int* __restrict__ adj, double fx, double fy,
                        double cx, double cy, float z_near, int cull, int t, int axis, double c0, double lo, double xn,
                        AaFace& cur, AaHit& h) {
  aa_project(c, faces, t, fx, fy, cx, cy, z_near, cull, cur);
  if (!cur.drawn) return false;
  int ea = -1, eb = -1;
  const double hi = lo + 1.0;
  for (int step = 1; step <= BODYFIT_AA_WALK; ++step) {
    // (everything the chosen edge is asked for below is kept by value: no register array is indexed by a run-time edge)
    int best = -1, bia = -1, bib = -1;
    double bd = 0.0, bs = 0.0, bnum = 0.0, bden = 0.0, bua = 0.0, bva = 0.0, bub = 0.0, bvb = 0.0, buo = 0.0, bvo = 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int a = e, b = e == 2 ? 0 : e + 1, o = e == 0 ? 2 : e - 1;
      if (ea >= 0 && ((cur.id[a] == ea && cur.id[b] == eb) || (cur.id[a] == eb && cur.id[b] == ea))) continue;
      const double la = axis ? cur.v[a] : cur.u[a], lb = axis ? cur.v[b] : cur.u[b];
      const double ca = axis ? cur.u[a] : cur.v[a], cb = axis ? cur.u[b] : cur.v[b];
      const double da = ca - c0, db = cb - c0;
      const bool up = da <= 0.0 && 0.0 < db, dn = db <= 0.0 && 0.0 < da;
      if (up == dn) continue;
      const double den = cb - ca;
      const double s = (c0 - ca) / den;
      const double xs = la + (lb - la) * s;
      if (!(xs >= lo && xs <= hi)) continue;
      const double d = fabs(xs - xn);
      if (best < 0 || d < bd) {
        best = e; bd = d; bs = s; bnum = lb - la; bden = den; bia = cur.id[a]; bib = cur.id[b];
        bua = cur.u[a]; bva = cur.v[a]; bub = cur.u[b]; bvb = cur.v[b]; buo = cur.u[o]; bvo = cur.v[o];
      }
    }
    if (best < 0) return false;
    const int t2 = adj[3 * t + best];
    bool sil = t2 < 0;
    AaFace nx;
    if (!sil) {
      aa_project(c, faces, t2, fx, fy, cx, cy, z_near, cull, nx);
      sil = !nx.drawn;
      if (!sil) {
        int o2 = -1;
        double u2 = 0.0, v2 = 0.0;
#pragma unroll
        for (int q = 2; q >= 0; --q)
          if (nx.id[q] != bia && nx.id[q] != bib) { o2 = q; u2 = nx.u[q]; v2 = nx.v[q]; }
        if (o2 < 0) sil = true;
        else {
          const double eu = bub - bua, ev = bvb - bva;
          const double s1 = eu * (bvo - bva) - ev * (buo - bua);
          const double s2 = eu * (v2 - bva) - ev * (u2 - bua);
          sil = !((s1 > 0.0 && s2 < 0.0) || (s1 < 0.0 && s2 > 0.0));   // side(c) side(c') >= 0: folded
        }
      }
    }
    if (sil) {
      h.face = t; h.edge = best; h.steps = step; h.ida = bia; h.idb = bib; h.s = bs; h.num = bnum; h.den = bden; h.d = bd;
      return true;
    }
    ea = bia; eb = bib;
    cur = nx; t = t2;
  }
  return false;
}

// The pair (p, q = p's neighbour on `axis`) of one frame: false when it does not blend, else the hit, the near pixel (0: p, 1: q)
// and the signed weight of the definition in f64.
__device__ __forceinline__ bool aa_pair(const float* __restrict__ c, const int* __restrict__ faces, const int* __restrict__ adj, int nF,
                                        double fx, double fy, double cx, double cy, float z_near, int cull, int fp, int fq, float dp,
                                        float dq, int i, int j, int axis, AaFace& cur, AaHit& h, int& near_q, double& w) {
  if ((unsigned)fp >= (unsigned)nF) { fp = -1; dp = std::numeric_limits<float>::infinity(); }
  if ((unsigned)fq >= (unsigned)nF) { fq = -1; dq = std::numeric_limits<float>::infinity(); }
  if (fp == fq) return false;
  near_q = dp <= dq ? 0 : 1;
  const int t = near_q ? fq : fp;
  if (t < 0) return false;
  const double c0 = axis ? (double)j : (double)i, lo = axis ? (double)i : (double)j;
  if (!aa_walk(c, faces, adj, fx, fy, cx, cy, z_near, cull, t, axis, c0, lo, near_q ? lo + 1.0 : lo, cur, h)) return false;
  // d >= 1/2: the other pixel receives d - 1/2; else the near one receives 1/2 - d.  w > 0: q receives; w < 0: p receives
  const bool to_other = h.d >= 0.5;
  const double alpha = to_other ? h.d - 0.5 : 0.5 - h.d;
  const bool to_q = to_other ? near_q == 0 : near_q == 1;
  w = to_q ? alpha : -alpha;
  return alpha != 0.0;
}

// One thread per pixel, neighbouring lanes on neighbouring columns.  Equal ids: two compares and one 8-byte store.  The candidate
// pairs of the block's 256 pixels (inside a body nearly one per pixel, on one axis or the other) are listed in LDS and walked one
// per lane, so a lane with two candidates does not hold 63 lanes with none; a pair's weight lands in the slot of its (pixel, axis)
// whichever lane walked it and in whatever order the list was filled (an integer atomic on its length): the output is the same.
__global__ __launch_bounds__(256) void k_rs_edges(const float* __restrict__ verts, long long frame_stride,
                                                  const int* __restrict__ faces, const int* __restrict__ adj, int nF, int W, int H,
                                                  long long total, double fx, double fy, double cx, double cy, float z_near,
                                                  int cull, const int* __restrict__ face_img, const float* __restrict__ depth,
                                                  float2* __restrict__ weight) {
  __shared__ int items[512];      // 2 lane + axis
  __shared__ float result[512];
  __shared__ int n_items;
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * 256, o = base + tid;
  const long long ppf = (long long)W * H;
  if (tid == 0) n_items = 0;
  result[2 * tid] = 0.0f; result[2 * tid + 1] = 0.0f;
  __syncthreads();
  if (o < total) {
    const long long pix = o % ppf;
    const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
    const int fp = face_img[o];
    if (j + 1 < W && face_img[o + 1] != fp) items[atomicAdd(&n_items, 1)] = 2 * tid;
    if (i + 1 < H && face_img[o + W] != fp) items[atomicAdd(&n_items, 1)] = 2 * tid + 1;
  }
  __syncthreads();
  const int n = n_items;
  for (int k = tid; k < n; k += 256) {
    const int item = items[k], axis = item & 1;
    const long long op = base + (item >> 1), oq = op + (axis ? W : 1);
    const long long frame = op / ppf, pix = op - frame * ppf;
    const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
    AaFace cur; AaHit h; int nq; double w;
    if (aa_pair(verts + (size_t)frame * (size_t)frame_stride, faces, adj, nF, fx, fy, cx, cy, z_near, cull, face_img[op], face_img[oq],
                depth[op], depth[oq], i, j, axis, cur, h, nq, w))
      result[item] = (float)w;
  }
  __syncthreads();
  if (o < total) weight[o] = make_float2(result[2 * tid], result[2 * tid + 1]);
}

// One thread per pixel: out = image + what the pixel receives from its four pairs, in the order left, right, up, down; with
// `transpose` the adjoint of that linear map.  f64, unfused; only the stores round.
template <int C>
__global__ __launch_bounds__(256) void k_rs_edge_blend(const float* __restrict__ weight, const float* __restrict__ image, int W, int H,
                                                       long long total, int transpose, float* __restrict__ out) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const long long ppf = (long long)W * H;
  const long long pix = o % ppf;
  const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
  // the signed amount with which THIS pixel receives from the neighbour (> 0), or the neighbour from this pixel (< 0)
  // (8-byte loads, neighbouring lanes on neighbouring entries; the entries of pairs that leave the image hold 0)
  const float2* w2 = reinterpret_cast<const float2*>(weight);
  const float2 wc = w2[o];
  const float w4[4] = {j > 0 ? w2[o - 1].x : 0.0f, j + 1 < W ? -wc.x : 0.0f, i > 0 ? w2[o - W].y : 0.0f, i + 1 < H ? -wc.y : 0.0f};
  const long long nb[4] = {o - 1, o + 1, o - W, o + W};
  double x[C], acc[C];
  for (int c = 0; c < C; ++c) acc[c] = x[c] = (double)image[C * (size_t)o + c];
  for (int k = 0; k < 4; ++k) {
    const float w = w4[k];
    if (!(w > 0.0f) && !(w < 0.0f)) continue;
    const bool receives = w > 0.0f;
    if (!receives && !transpose) continue;
    const double alpha = receives ? (double)w : -(double)w;
    for (int c = 0; c < C; ++c) {
      if (!transpose) acc[c] = acc[c] + alpha * ((double)image[C * (size_t)nb[k] + c] - x[c]);
      else if (receives) acc[c] = acc[c] - alpha * x[c];
      else acc[c] = acc[c] + alpha * (double)image[C * (size_t)nb[k] + c];
    }
  }
  for (int c = 0; c < C; ++c) out[C * (size_t)o + c] = (float)acc[c];
}

// One thread per listed pair (code = 2 pixel + axis): the walk again, then the rows of corner a and corner b of the silhouette
// edge.  G = sigma sum_c grad[r][c] (image[n][c] - image[o][c]); coef = G (1 - s), G s; dir = grad(along) - k grad(across).
template <int C>
__global__ __launch_bounds__(256) void k_rs_edge_rows(const float* __restrict__ verts, long long frame_stride,
                                                      const int* __restrict__ faces, const int* __restrict__ adj, int nF, int F, int W,
                                                      int H, double fx, double fy, double cx, double cy, float z_near, int cull,
                                                      const int* __restrict__ face_img, const float* __restrict__ depth,
                                                      const float* __restrict__ image, const float* __restrict__ grad,
                                                      const int* __restrict__ pair, const int* __restrict__ offset,
                                                      long long per_frame, long long n_pairs, int* __restrict__ index,
                                                      float* __restrict__ bary, float* __restrict__ coef, float* __restrict__ dir) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_pairs) return;
  const long long ppf = (long long)W * H;
  const long long frame = offset ? rs_frame_of(offset, F, row) : row / per_frame;
  const int code = pair[row];
  const int axis = code & 1;
  const long long pix = code >> 1;
  bool ok = code >= 0 && pix < ppf;
  int i = 0, j = 0;
  if (ok) {
    i = (int)(pix / W); j = (int)(pix - (long long)i * W);
    ok = axis ? i + 1 < H : j + 1 < W;
  }
  AaFace cur; AaHit h; int nq = 0; double w = 0.0;
  size_t op = 0, oq = 0;
  const float* c = verts + (size_t)frame * (size_t)frame_stride;
  if (ok) {
    op = (size_t)frame * (size_t)ppf + (size_t)pix;
    oq = op + (axis ? (size_t)W : 1);
    ok = aa_pair(c, faces, adj, nF, fx, fy, cx, cy, z_near, cull, face_img[op], face_img[oq], depth[op], depth[oq], i, j, axis, cur,
                 h, nq, w);
  }
  int idx = -1;
  double co[2] = {0.0, 0.0}, m[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  int corner[2] = {0, 0};
  if (ok) {
    const size_t on = nq ? oq : op, oo = nq ? op : oq, orc = w > 0.0 ? oq : op;
    double G = 0.0;
    for (int ch = 0; ch < C; ++ch)
      G = G + (double)grad[C * orc + ch] * ((double)image[C * on + ch] - (double)image[C * oo + ch]);
    if (nq) G = -G;
    idx = h.face;
    corner[0] = h.edge; corner[1] = h.edge == 2 ? 0 : h.edge + 1;
    co[0] = G * (1.0 - h.s); co[1] = G * h.s;
    const double k = h.num / h.den;
    for (int q = 0; q < 2; ++q) {
      const size_t id = (size_t)(q ? h.idb : h.ida);
      const double X = (double)c[3 * id], Y = (double)c[3 * id + 1], Z = (double)c[3 * id + 2];
      const double iz = 1.0 / Z, ax = fx * iz, ay = fy * iz;
      const double zu = (ax * X) * iz, zv = (ay * Y) * iz;      // grad u = (ax, 0, -zu), grad v = (0, ay, -zv)
      if (axis == 0) { m[q][0] = ax; m[q][1] = -(k * ay); m[q][2] = k * zv - zu; }
      else { m[q][0] = -(k * ax); m[q][1] = ay; m[q][2] = k * zu - zv; }
    }
  }
  for (int q = 0; q < 2; ++q) {
    const size_t r = 2 * (size_t)row + q;
    index[r] = idx;
    for (int a = 0; a < 3; ++a) bary[3 * r + a] = idx >= 0 && a == corner[q] ? 1.0f : 0.0f;
    coef[r] = (float)co[q];
    for (int a = 0; a < 3; ++a) dir[3 * r + a] = (float)m[q][a];
  }
}

int rs_invalid(const char* fn, const char* what) {
  return bodyfit_internal_fail(BODYFIT_ERR_INVALID, (std::string(fn) + ": " + what).c_str());
}

}  // namespace

struct bodyfit_raster {
  int device = 0, nV = 0, nF = 0, W = 0, H = 0, tilesX = 0, tilesY = 0;
  int* d_faces = nullptr;
  int* d_adj = nullptr;                         // [n_faces][3]: the lowest-id other face on edge (corner e, corner e + 1), or -1
  unsigned* d_totals = nullptr;                 // [0] entries, [1] the longest list
  RsFace* d_recs = nullptr;      size_t recsCap = 0;      // records
  unsigned* d_tiles = nullptr;   size_t tilesCap = 0;     // tiles: count | cursor | offset
  int* d_entries = nullptr;      size_t entriesCap = 0;   // face ids
  int32_t* d_edt = nullptr;      size_t edtCap = 0;       // distance transform: seed columns and envelope stacks (edt.h)
  unsigned lastTotals[2] = {0, 0};
  ~bodyfit_raster() {
    for (void* q : {(void*)d_faces, (void*)d_adj, (void*)d_totals, (void*)d_recs, (void*)d_tiles, (void*)d_entries, (void*)d_edt})
      if (q) (void)hipFree(q);
  }
};

namespace bodyfit {
RasterView raster_view(const bodyfit_raster* r) {      // (d_totals[2]: the render uses [0] and [1] only)
  return RasterView{r->device, r->nV, r->nF, r->W, r->H, r->d_faces, r->d_totals + 2};
}
}  // namespace bodyfit

namespace {
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
}  // namespace

namespace {
template <typename T>
void rs_launch_sample(int C, dim3 grid, hipStream_t st, const float* d_points, long long points_frame_stride, long long N,
                      long long total, double fx, double fy, double cx, double cy, float z_near, const void* d_image,
                      long long image_frame_stride, int W, int H, const uint8_t* d_gate, float* d_value, uint8_t* d_valid,
                      float* d_grad) {
  auto launch = [&](auto kernel) {
    BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_points, points_frame_stride, N, total, fx, fy, cx, cy, z_near,
                   static_cast<const T*>(d_image), image_frame_stride, W, H, d_gate, d_value, d_valid, d_grad);
  };
  switch (C) {
    case 1: launch(k_rs_sample<1, T>); break;
    case 2: launch(k_rs_sample<2, T>); break;
    case 3: launch(k_rs_sample<3, T>); break;
    default: launch(k_rs_sample<4, T>); break;
  }
}
}  // namespace

namespace {
// the two interpolation-row entries: one validation, one launch (indexed: attr rows by d_attr_faces, else by the corners' ids)
int rs_interp_rows(const char* fn, bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                   double fy, double cx, double cy, const int32_t* d_face_image, const int32_t* d_pixel, const int32_t* d_offset,
                   long long n_rows, const float* d_attr, long long attr_frame_stride, int n_channels, bool indexed,
                   const int32_t* d_attr_faces, int n_attr_rows, const float* d_grad_image, const float* d_grad_z, int32_t* d_index,
                   float* d_bary, float* d_dir, float* d_value, void* stream) {
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0 || n_rows < 0) return rs_invalid(fn, "negative n_frames or n_rows");
  if (!(fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
    return rs_invalid(fn, "fx and fy must be positive, and the intrinsics finite");
  if (n_channels < 0 || n_channels > 4) return rs_invalid(fn, "n_channels outside 0 .. 4");
  if (indexed && n_attr_rows < 0) return rs_invalid(fn, "negative n_attr_rows");
  if (d_offset && !d_pixel) return rs_invalid(fn, "d_offset without d_pixel");
  const long long ppf = (long long)r->W * r->H;
  if (!d_pixel && n_rows != ppf * n_frames) return rs_invalid(fn, "without d_pixel n_rows must be n_frames H W");
  if (n_rows >= (1ll << 31) - 4096) return rs_invalid(fn, "2^31 rows or more in one call");
  if (n_rows > 0 && n_frames == 0) return rs_invalid(fn, "rows without frames");
  if (d_pixel && !d_offset && n_frames > 0 && n_rows % n_frames != 0)
    return rs_invalid(fn, "a uniform row set needs n_rows divisible by n_frames");
  if (n_frames == 0 || n_rows == 0) return BODYFIT_OK;
  if (!d_face_image || !d_index) return rs_invalid(fn, "d_face_image or d_index is NULL");
  if (r->nF > 0 && !d_verts) return rs_invalid(fn, "d_verts is NULL");
  if (verts_frame_stride < 3ll * r->nV) return rs_invalid(fn, "verts_frame_stride below 3 n_verts");
  if (n_channels > 0 && (!d_attr || !d_grad_image)) return rs_invalid(fn, "d_attr or d_grad_image is NULL with n_channels > 0");
  if (n_channels > 0 && attr_frame_stride != 0 && attr_frame_stride < (long long)n_channels * n_attr_rows)
    return rs_invalid(fn, indexed ? "a non-zero attr_frame_stride below n_channels n_attr_rows"
                                  : "a non-zero attr_frame_stride below n_channels n_verts");
  if (indexed && n_channels > 0 && r->nF > 0 && !d_attr_faces) return rs_invalid(fn, "d_attr_faces is NULL");
  if (n_channels == 0 && !d_grad_z) return rs_invalid(fn, "n_channels == 0 needs d_grad_z");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n_rows + 255) / 256));
  auto launch = [&](auto kernel) {
    BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_verts, verts_frame_stride, r->d_faces, r->nF, n_frames, r->W, r->H, fx, fy,
                   cx, cy, d_face_image, d_pixel, d_offset, n_rows / n_frames, n_rows, d_attr, attr_frame_stride, d_grad_image,
                   d_grad_z, d_index, d_bary, d_dir, d_value, d_attr_faces, n_attr_rows);
  };
  // (the un-indexed entry launches what it always has; C = 0 reads no attributes: one instantiation serves both)
  if (indexed && n_channels > 0)
    switch (n_channels) {
      case 1: launch(k_rs_interp_rows<1, true>); break;
      case 2: launch(k_rs_interp_rows<2, true>); break;
      case 3: launch(k_rs_interp_rows<3, true>); break;
      default: launch(k_rs_interp_rows<4, true>); break;
    }
  else
    switch (n_channels) {
      case 0: launch(k_rs_interp_rows<0, false>); break;
      case 1: launch(k_rs_interp_rows<1, false>); break;
      case 2: launch(k_rs_interp_rows<2, false>); break;
      case 3: launch(k_rs_interp_rows<3, false>); break;
      default: launch(k_rs_interp_rows<4, false>); break;
    }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}
}  // namespace

extern "C" {

int bodyfit_raster_create(int device, int n_verts, int n_faces, const int32_t* faces, int width, int height,
                          bodyfit_raster** out) {
  const char* fn = "bodyfit_raster_create";
  if (!out) return rs_invalid(fn, "out is NULL");
  if (n_verts < 0 || n_faces < 0 || (n_faces > 0 && !faces)) return rs_invalid(fn, "negative count or NULL faces");
  if (width < 1 || height < 1 || width > 16384 || height > 16384) return rs_invalid(fn, "image size outside 1 .. 16384");
  for (long long i = 0; i < 3ll * n_faces; ++i)
    if (faces[i] < 0 || faces[i] >= n_verts) return rs_invalid(fn, "face refers to a vertex out of range");
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
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0) return rs_invalid(fn, "negative n_frames");
  if (!(z_near > 0.0f)) return rs_invalid(fn, "z_near must be positive");
  if (!(fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
    return rs_invalid(fn, "fx and fy must be positive, and the intrinsics finite");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_depth || !d_face) return rs_invalid(fn, "d_depth or d_face is NULL");
  if (r->nF > 0 && !d_verts) return rs_invalid(fn, "d_verts is NULL");
  if (verts_frame_stride < 3ll * r->nV) return rs_invalid(fn, "verts_frame_stride below 3 n_verts");
  const int tilesPerFrame = r->tilesX * r->tilesY;
  const long long nT = (long long)n_frames * tilesPerFrame, nR = (long long)n_frames * r->nF;
  if (nT >= (1ll << 31) || nR >= (1ll << 31)) return rs_invalid(fn, "2^31 tiles or records or more in one call");
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
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0) return rs_invalid(fn, "negative n_frames");
  if (n_frames == 0 || (!d_face_visible && !d_vert_visible)) return BODYFIT_OK;
  if (!d_face) return rs_invalid(fn, "d_face is NULL");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long ppf = (long long)r->W * r->H, total = ppf * n_frames;
  if (total >= (1ll << 39)) return rs_invalid(fn, "2^39 pixels or more in one call");
  if (d_face_visible && r->nF) HIP_TRY(hipMemsetAsync(d_face_visible, 0, (size_t)n_frames * r->nF, st));
  if (d_vert_visible && r->nV) HIP_TRY(hipMemsetAsync(d_vert_visible, 0, (size_t)n_frames * r->nV, st));
  if (r->nF > 0)
    BODYFIT_LAUNCH(k_rs_visible, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_face, total, ppf, r->d_faces,
                   r->nF, r->nV, d_face_visible, d_vert_visible);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_depth_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                     double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                     const int32_t* d_pixel, const int32_t* d_offset, long long n_rows, int32_t* d_index,
                                     float* d_z, float* d_bary, float* d_dir, void* stream) {
  const char* fn = "bodyfit_raster_depth_rows_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0 || n_rows < 0) return rs_invalid(fn, "negative n_frames or n_rows");
  if (!(fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
    return rs_invalid(fn, "fx and fy must be positive, and the intrinsics finite");
  if (d_offset && !d_pixel) return rs_invalid(fn, "d_offset without d_pixel");
  const long long ppf = (long long)r->W * r->H;
  if (!d_pixel && n_rows != ppf * n_frames) return rs_invalid(fn, "without d_pixel n_rows must be n_frames H W");
  if (n_rows >= (1ll << 31) - 4096) return rs_invalid(fn, "2^31 rows or more in one call");
  if (n_rows > 0 && n_frames == 0) return rs_invalid(fn, "rows without frames");
  if (d_pixel && !d_offset && n_frames > 0 && n_rows % n_frames != 0)
    return rs_invalid(fn, "a uniform row set needs n_rows divisible by n_frames");
  if (n_frames == 0 || n_rows == 0) return BODYFIT_OK;
  if (!d_face_image || !d_index) return rs_invalid(fn, "d_face_image or d_index is NULL");
  if (r->nF > 0 && !d_verts) return rs_invalid(fn, "d_verts is NULL");
  if (verts_frame_stride < 3ll * r->nV) return rs_invalid(fn, "verts_frame_stride below 3 n_verts");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  BODYFIT_LAUNCH(k_rs_depth_rows, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, d_verts, verts_frame_stride,
                 r->d_faces, r->nF, n_frames, r->W, r->H, fx, fy, cx, cy, d_face_image, d_pixel, d_offset, n_rows / n_frames,
                 n_rows, d_index, d_z, d_bary, d_dir);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_interp_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                      double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                      const int32_t* d_pixel, const int32_t* d_offset, long long n_rows, const float* d_attr,
                                      long long attr_frame_stride, int n_channels, const float* d_grad_image,
                                      const float* d_grad_z, int32_t* d_index, float* d_bary, float* d_dir, float* d_value,
                                      void* stream) {
  return rs_interp_rows("bodyfit_raster_interp_rows_device", r, d_verts, verts_frame_stride, n_frames, fx, fy, cx, cy, d_face_image,
                        d_pixel, d_offset, n_rows, d_attr, attr_frame_stride, n_channels, false, nullptr, r ? r->nV : 0,
                        d_grad_image, d_grad_z, d_index, d_bary, d_dir, d_value, stream);
}

int bodyfit_raster_interp_rows_indexed_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                              double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                              const int32_t* d_pixel, const int32_t* d_offset, long long n_rows,
                                              const float* d_attr, long long attr_frame_stride, int n_channels,
                                              const int32_t* d_attr_faces, int n_attr_rows, const float* d_grad_image,
                                              const float* d_grad_z, int32_t* d_index, float* d_bary, float* d_dir,
                                              float* d_value, void* stream) {
  return rs_interp_rows("bodyfit_raster_interp_rows_indexed_device", r, d_verts, verts_frame_stride, n_frames, fx, fy, cx, cy,
                        d_face_image, d_pixel, d_offset, n_rows, d_attr, attr_frame_stride, n_channels, true, d_attr_faces,
                        n_attr_rows, d_grad_image, d_grad_z, d_index, d_bary, d_dir, d_value, stream);
}

int bodyfit_raster_shade_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                long long verts_frame_stride, const float* d_attr, long long attr_frame_stride, int n_channels,
                                int n_frames, const float* background, float* d_image, float* d_weight, void* stream) {
  const char* fn = "bodyfit_raster_shade_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0) return rs_invalid(fn, "negative n_frames");
  if (n_channels < 1 || n_channels > 4) return rs_invalid(fn, "n_channels outside 1 .. 4");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_face || !d_bary || !d_image) return rs_invalid(fn, "d_face, d_bary or d_image is NULL");
  if (r->nF > 0 && (!d_verts || !d_attr)) return rs_invalid(fn, "d_verts or d_attr is NULL");
  if (verts_frame_stride < 3ll * r->nV) return rs_invalid(fn, "verts_frame_stride below 3 n_verts");
  if (attr_frame_stride != 0 && attr_frame_stride < (long long)n_channels * r->nV)
    return rs_invalid(fn, "a non-zero attr_frame_stride below n_channels n_verts");
  const long long ppf = (long long)r->W * r->H, total = ppf * n_frames;
  if (total >= (1ll << 39)) return rs_invalid(fn, "2^39 pixels or more in one call");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float4 bg = background ? make_float4(background[0], background[1], background[2], background[3])
                               : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const dim3 grid((unsigned)((total + 255) / 256));
  auto launch = [&](auto kernel) {
    BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_face, d_bary, d_verts, verts_frame_stride, d_attr, attr_frame_stride,
                   r->d_faces, r->nF, ppf, total, bg, d_image, d_weight);
  };
  switch (n_channels) {
    case 1: launch(k_rs_shade<1>); break;
    case 2: launch(k_rs_shade<2>); break;
    case 3: launch(k_rs_shade<3>); break;
    default: launch(k_rs_shade<4>); break;
  }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_sample_device(bodyfit_raster* r, const float* d_points, long long points_frame_stride,
                                 long long n_points, int n_frames, double fx, double fy, double cx, double cy, float z_near,
                                 const void* d_image, int image_kind, int n_channels, long long image_frame_stride,
                                 const uint8_t* d_gate, float* d_value, uint8_t* d_valid, float* d_grad, void* stream) {
  const char* fn = "bodyfit_raster_sample_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0 || n_points < 0) return rs_invalid(fn, "negative n_frames or n_points");
  if (n_channels < 1 || n_channels > 4) return rs_invalid(fn, "n_channels outside 1 .. 4");
  if (image_kind != 0 && image_kind != 1) return rs_invalid(fn, "image_kind must be 0 (u8) or 1 (f32)");
  if (!(z_near > 0.0f)) return rs_invalid(fn, "z_near must be positive");
  if (!(fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
    return rs_invalid(fn, "fx and fy must be positive, and the intrinsics finite");
  if (n_frames == 0 || n_points == 0) return BODYFIT_OK;
  if (!d_points || !d_image || !d_value || !d_valid) return rs_invalid(fn, "d_points, d_image, d_value or d_valid is NULL");
  if (points_frame_stride < 3 * n_points) return rs_invalid(fn, "points_frame_stride below 3 n_points");
  if (image_frame_stride < (long long)r->W * r->H * n_channels) return rs_invalid(fn, "image_frame_stride below H W n_channels");
  if (n_points >= (1ll << 39) / n_frames) return rs_invalid(fn, "2^39 points or more in one call");
  const long long total = n_points * n_frames;
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (image_kind == 0)
    rs_launch_sample<uint8_t>(n_channels, grid, st, d_points, points_frame_stride, n_points, total, fx, fy, cx, cy, z_near,
                              d_image, image_frame_stride, r->W, r->H, d_gate, d_value, d_valid, d_grad);
  else
    rs_launch_sample<float>(n_channels, grid, st, d_points, points_frame_stride, n_points, total, fx, fy, cx, cy, z_near,
                            d_image, image_frame_stride, r->W, r->H, d_gate, d_value, d_valid, d_grad);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_distance_device(bodyfit_raster* r, const void* d_seed, int seed_kind, long long seed_frame_stride,
                                   int n_frames, int invert, int32_t* d_dist2, int32_t* d_nearest, void* stream) {
  const char* fn = "bodyfit_raster_distance_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0) return rs_invalid(fn, "negative n_frames");
  if (seed_kind != 0 && seed_kind != 1) return rs_invalid(fn, "seed_kind must be 0 (u8) or 1 (int32)");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_seed || !d_dist2) return rs_invalid(fn, "d_seed or d_dist2 is NULL");
  const long long ppf = (long long)r->W * r->H;
  if (seed_frame_stride < ppf) return rs_invalid(fn, "seed_frame_stride below H W");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // groups of frames that share the workspace one after the other on the stream: its size follows from (F, H, W) alone
  const int group = (int)std::max(1ll, std::min<long long>(n_frames, bodyfit::kEdtGroupPixels / ppf));
  if (int rc = rs_grow(&r->d_edt, &r->edtCap, (size_t)group * ppf * bodyfit::kEdtWorkspaceInts)) return rc;
  const size_t elem = seed_kind == 0 ? 1 : 4;
  for (int f0 = 0; f0 < n_frames; f0 += group)
    bodyfit::edt_launch(static_cast<const char*>(d_seed) + (size_t)f0 * seed_frame_stride * elem, seed_kind, seed_frame_stride,
                        std::min(group, n_frames - f0), invert, r->W, r->H, r->d_edt, d_dist2 + (size_t)f0 * ppf,
                        d_nearest ? d_nearest + (size_t)f0 * ppf : nullptr, st);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_edges_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                                double fy, double cx, double cy, float z_near, int cull_backfaces, const int32_t* d_face,
                                const float* d_depth, float* d_weight, void* stream) {
  const char* fn = "bodyfit_raster_edges_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0) return rs_invalid(fn, "negative n_frames");
  if (!(z_near > 0.0f)) return rs_invalid(fn, "z_near must be positive");
  if (!(fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
    return rs_invalid(fn, "fx and fy must be positive, and the intrinsics finite");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_weight) return rs_invalid(fn, "d_weight is NULL");
  const long long ppf = (long long)r->W * r->H, total = ppf * n_frames;
  if (total >= (1ll << 39)) return rs_invalid(fn, "2^39 pixels or more in one call");
  if (r->nF > 0 && (!d_verts || !d_face || !d_depth)) return rs_invalid(fn, "d_verts, d_face or d_depth is NULL");
  if (verts_frame_stride < 3ll * r->nV) return rs_invalid(fn, "verts_frame_stride below 3 n_verts");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r->nF == 0) {
    HIP_TRY(hipMemsetAsync(d_weight, 0, (size_t)total * 2 * sizeof(float), st));
    return BODYFIT_OK;
  }
  BODYFIT_LAUNCH(k_rs_edges, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_verts, verts_frame_stride, r->d_faces,
                 r->d_adj, r->nF, r->W, r->H, total, fx, fy, cx, cy, z_near, cull_backfaces, d_face, d_depth,
                 reinterpret_cast<float2*>(d_weight));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_edge_blend_device(bodyfit_raster* r, const float* d_weight, const float* d_image, int n_channels, int n_frames,
                                     int transpose, float* d_out, void* stream) {
  const char* fn = "bodyfit_raster_edge_blend_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0) return rs_invalid(fn, "negative n_frames");
  if (n_channels < 1 || n_channels > 4) return rs_invalid(fn, "n_channels outside 1 .. 4");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_weight || !d_image || !d_out) return rs_invalid(fn, "d_weight, d_image or d_out is NULL");
  if (d_out == d_image) return rs_invalid(fn, "d_out must not be d_image");
  const long long ppf = (long long)r->W * r->H, total = ppf * n_frames;
  if (total >= (1ll << 39)) return rs_invalid(fn, "2^39 pixels or more in one call");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((total + 255) / 256));
  auto launch = [&](auto kernel) {
    BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_weight, d_image, r->W, r->H, total, transpose ? 1 : 0, d_out);
  };
  switch (n_channels) {
    case 1: launch(k_rs_edge_blend<1>); break;
    case 2: launch(k_rs_edge_blend<2>); break;
    case 3: launch(k_rs_edge_blend<3>); break;
    default: launch(k_rs_edge_blend<4>); break;
  }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_edge_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                                    double fy, double cx, double cy, float z_near, int cull_backfaces, const int32_t* d_face,
                                    const float* d_depth, const float* d_image, const float* d_grad, int n_channels,
                                    const int32_t* d_pair, const int32_t* d_offset, long long n_pairs, int32_t* d_index,
                                    float* d_bary, float* d_coef, float* d_dir, void* stream) {
  const char* fn = "bodyfit_raster_edge_rows_device";
  if (!r) return rs_invalid(fn, "handle is NULL");
  if (n_frames < 0 || n_pairs < 0) return rs_invalid(fn, "negative n_frames or n_pairs");
  if (n_channels < 1 || n_channels > 4) return rs_invalid(fn, "n_channels outside 1 .. 4");
  if (!(z_near > 0.0f)) return rs_invalid(fn, "z_near must be positive");
  if (!(fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
    return rs_invalid(fn, "fx and fy must be positive, and the intrinsics finite");
  if (n_pairs >= (1ll << 30) - 2048) return rs_invalid(fn, "2^30 pairs or more in one call");
  if (n_pairs > 0 && n_frames == 0) return rs_invalid(fn, "pairs without frames");
  if (!d_offset && n_frames > 0 && n_pairs % n_frames != 0)
    return rs_invalid(fn, "a uniform pair list needs n_pairs divisible by n_frames");
  if (n_frames == 0 || n_pairs == 0) return BODYFIT_OK;
  if (!d_pair || !d_index || !d_bary || !d_coef || !d_dir) return rs_invalid(fn, "d_pair or an output is NULL");
  if (r->nF > 0 && (!d_verts || !d_face || !d_depth || !d_image || !d_grad))
    return rs_invalid(fn, "d_verts, d_face, d_depth, d_image or d_grad is NULL");
  if (verts_frame_stride < 3ll * r->nV) return rs_invalid(fn, "verts_frame_stride below 3 n_verts");
  if ((long long)r->W * r->H >= (1ll << 30)) return rs_invalid(fn, "2^30 pixels or more in a frame");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (r->nF == 0) {      // nothing blends: every row void
    HIP_TRY(hipMemsetAsync(d_index, 0xff, (size_t)n_pairs * 2 * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(d_bary, 0, (size_t)n_pairs * 6 * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_coef, 0, (size_t)n_pairs * 2 * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_dir, 0, (size_t)n_pairs * 6 * sizeof(float), st));
    return BODYFIT_OK;
  }
  const dim3 grid((unsigned)((n_pairs + 255) / 256));
  auto launch = [&](auto kernel) {
    BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_verts, verts_frame_stride, r->d_faces, r->d_adj, r->nF, n_frames, r->W, r->H,
                   fx, fy, cx, cy, z_near, cull_backfaces, d_face, d_depth, d_image, d_grad, d_pair, d_offset, n_pairs / n_frames,
                   n_pairs, d_index, d_bary, d_coef, d_dir);
  };
  switch (n_channels) {
    case 1: launch(k_rs_edge_rows<1>); break;
    case 2: launch(k_rs_edge_rows<2>); break;
    case 3: launch(k_rs_edge_rows<3>); break;
    default: launch(k_rs_edge_rows<4>); break;
  }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_last_bins(bodyfit_raster* r, long long* n_entries, int* longest) {
  if (!r || !n_entries || !longest) return rs_invalid("bodyfit_raster_last_bins", "null argument");
  *n_entries = r->lastTotals[0];
  *longest = (int)r->lastTotals[1];
  return BODYFIT_OK;
}

}  // extern "C"
