// Silhouette-edge antialiasing of a render (bodyfit_raster_edges_device, bodyfit_raster_edge_blend_device,
// bodyfit_raster_edge_rows_device; include/bodyfit.h: the definition and its bands).
//
//   k_rs_edges   one thread per pixel: its right and lower neighbour pairs; where the two face ids differ, the bounded walk from
//                the nearer pixel's face to the silhouette edge that crosses the segment between the two centres, and the blend
//                weight (bodyfit_raster_edges_device)
//   k_rs_edge_blend<C>  one thread per pixel: the blend of an image by the weight image, or its adjoint
//   k_rs_edge_rows<C>   one thread per listed pair: the walk again, and the two "barycentric x direction" rows of the crossing's
//                derivative in the edge's two corners (bodyfit_raster_edge_rows_device)
//
// Arithmetic.  A face of the walk is projected by the operations of the render's k_rs_faces (k_raster.hip) in the same order, in
// f64; products are formed separately and subtracted (no contraction), so the walk sees the edges the render drew.  Only the
// stores round to f32.  No MFMA, no float atomics.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <limits>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "raster_handle.h"

#pragma clang fp contract(off)

using namespace bodyfit;

namespace {

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

}  // namespace

extern "C" {

int bodyfit_raster_edges_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                                double fy, double cx, double cy, float z_near, int cull_backfaces, const int32_t* d_face,
                                const float* d_depth, float* d_weight, void* stream) {
  const char* fn = "bodyfit_raster_edges_device";
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (!(z_near > 0.0f)) return invalid_arg(fn, "z_near must be positive");
  if (int rc = rs_check_intrinsics(fn, fx, fy, cx, cy)) return rc;
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_weight) return invalid_arg(fn, "d_weight is NULL");
  if (int rc = rs_check_pixels(fn, r, n_frames)) return rc;
  const long long total = (long long)r->W * r->H * n_frames;
  if (r->nF > 0 && (!d_verts || !d_face || !d_depth)) return invalid_arg(fn, "d_verts, d_face or d_depth is NULL");
  if (int rc = rs_check_verts_stride(fn, r, verts_frame_stride)) return rc;
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
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_weight || !d_image || !d_out) return invalid_arg(fn, "d_weight, d_image or d_out is NULL");
  if (d_out == d_image) return invalid_arg(fn, "d_out must not be d_image");
  if (int rc = rs_check_pixels(fn, r, n_frames)) return rc;
  const long long total = (long long)r->W * r->H * n_frames;
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((total + 255) / 256));
  rs_dispatch_channels(n_channels, [&](auto c) {
    BODYFIT_LAUNCH(k_rs_edge_blend<decltype(c)::value>, grid, dim3(256), 0, st, d_weight, d_image, r->W, r->H, total,
                   transpose ? 1 : 0, d_out);
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_edge_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                                    double fy, double cx, double cy, float z_near, int cull_backfaces, const int32_t* d_face,
                                    const float* d_depth, const float* d_image, const float* d_grad, int n_channels,
                                    const int32_t* d_pair, const int32_t* d_offset, long long n_pairs, int32_t* d_index,
                                    float* d_bary, float* d_coef, float* d_dir, void* stream) {
  const char* fn = "bodyfit_raster_edge_rows_device";
  if (!r) return invalid_arg(fn, "handle is NULL");
  if (n_frames < 0 || n_pairs < 0) return invalid_arg(fn, "negative n_frames or n_pairs");
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (!(z_near > 0.0f)) return invalid_arg(fn, "z_near must be positive");
  if (int rc = rs_check_intrinsics(fn, fx, fy, cx, cy)) return rc;
  if (n_pairs >= (1ll << 30) - 2048) return invalid_arg(fn, "2^30 pairs or more in one call");
  if (n_pairs > 0 && n_frames == 0) return invalid_arg(fn, "pairs without frames");
  if (!d_offset && n_frames > 0 && n_pairs % n_frames != 0)
    return invalid_arg(fn, "a uniform pair list needs n_pairs divisible by n_frames");
  if (n_frames == 0 || n_pairs == 0) return BODYFIT_OK;
  if (!d_pair || !d_index || !d_bary || !d_coef || !d_dir) return invalid_arg(fn, "d_pair or an output is NULL");
  if (r->nF > 0 && (!d_verts || !d_face || !d_depth || !d_image || !d_grad))
    return invalid_arg(fn, "d_verts, d_face, d_depth, d_image or d_grad is NULL");
  if (int rc = rs_check_verts_stride(fn, r, verts_frame_stride)) return rc;
  if ((long long)r->W * r->H >= (1ll << 30)) return invalid_arg(fn, "2^30 pixels or more in a frame");
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
  rs_dispatch_channels(n_channels, [&](auto c) {
    BODYFIT_LAUNCH(k_rs_edge_rows<decltype(c)::value>, grid, dim3(256), 0, st, d_verts, verts_frame_stride, r->d_faces, r->d_adj,
                   r->nF, n_frames, r->W, r->H, fx, fy, cx, cy, z_near, cull_backfaces, d_face, d_depth, d_image, d_grad, d_pair,
                   d_offset, n_pairs / n_frames, n_pairs, d_index, d_bary, d_coef, d_dir);
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
