// UV textures over a render: the texture lookup and its gradients in the uv coordinates and in the texels
// (bodyfit_raster_texture_device, bodyfit_raster_texture_grad_device; include/bodyfit.h: the definitions, the contracts and the
// derivation of their constants).
//
//   k_tx_forward<C, T>  one thread per pixel of a render, neighbouring lanes on neighbouring columns: the shade's weights (the
//                same operations in the same order as k_rs_shade), the pixel's (u, v) from the face's three uv rows, the clamp in
//                f64, the cell and the bilinear patch (bilinear_inl.h, the image sampler's).  Plain stores.
//   k_tx_gmax    the largest |G| of the call as the u32 bit pattern of |G| (for non-negative floats the order of the patterns is the
//                order of the values, and every NaN or infinity is >= 0x7f800000): a wave reduction, then ONE integer atomicMax per
//                workgroup
//   k_tx_grad<C, T>  one thread per pixel: the forward's pixel again, (a) the patch's derivative times (Wt, Ht), stored; (b) the
//                4 C contributions G_c omega_k of the cell, each formed in f64 (one rounding), scaled by 2^s (exact), rounded to
//                the nearest integer; the lanes of a wave that share a cell add their integers up first (runs of equal cells),
//                and the run's first lane adds with no-return 64-bit INTEGER atomics.  Integer addition is associative: the sums
//                do not depend on the order of the lanes, of the workgroups or of the frames, nor on the combining
//   k_tx_fold    one thread per texel element: (float)((double)sum 2^-s)
// The scale exponent s = 60 - B - E, B the bit length of the pixel count (host) and E the smallest integer with max|G| < 2^E
// (device): no host synchronisation.  No float atomics anywhere.
// The lookup with mipmaps (bodyfit_raster_texture_mip_*: k_txm_build, k_txm_forward, k_txm_grad, k_txm_fold) stands below the
// plain kernels, which it leaves as they are, and shares tx_pixel, k_tx_gmax and the scale exponent with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/bodyfit.h"
#include "bilinear_inl.h"
#include "bodyfit_device.h"
#include "raster_handle.h"

#pragma clang fp contract(off)

using namespace bodyfit;

namespace {

struct TxArgs {
  const int* face_img;       // [F][H][W]
  const float* bary;         // [F][H][W][3]
  const float* verts;        // [F] stride verts_stride, [n_verts][3]
  long long verts_stride;
  const int* faces;          // [nF][3]
  const float* uv;           // [T][2]
  const int* uv_faces;       // [nF][3]
  int nF, T;
  int Wt, Ht;
  long long tex_stride;      // elements between the frames' textures; 0: shared
  long long ppf, total;      // pixels per frame, pixels
};

// One pixel of the lookup: the shade's weights, (u, v) and the clamped texel coordinates.  Everything f64 and unfused.
struct TxPixel {
  bool ok;
  bool free_x, free_y;       // the clamp is NOT active in x / y: the derivative passes
  double w[3], u, v, x, y;
};

__device__ __forceinline__ TxPixel tx_pixel(const TxArgs& A, long long o) {
  TxPixel p;
  p.ok = false; p.free_x = p.free_y = false;
  p.w[0] = p.w[1] = p.w[2] = 0.0; p.u = p.v = p.x = p.y = 0.0;
  const int t = A.face_img[o];
  const float l0 = A.bary[3 * (size_t)o], l1 = A.bary[3 * (size_t)o + 1], l2 = A.bary[3 * (size_t)o + 2];
  // (a NaN fails every comparison; x - x is NaN for an infinity)
  bool ok = (unsigned)t < (unsigned)A.nF && l0 - l0 == 0.0f && l1 - l1 == 0.0f && l2 - l2 == 0.0f && l0 >= 0.0f && l1 >= 0.0f &&
            l2 >= 0.0f;
  if (!ok) return p;
  const int k0 = A.uv_faces[3 * t], k1 = A.uv_faces[3 * t + 1], k2 = A.uv_faces[3 * t + 2];
  if ((unsigned)k0 >= (unsigned)A.T || (unsigned)k1 >= (unsigned)A.T || (unsigned)k2 >= (unsigned)A.T) return p;
  const size_t frame = (size_t)(o / A.ppf);
  const float* v = A.verts + frame * (size_t)A.verts_stride;
  const size_t i0 = (size_t)A.faces[3 * t], i1 = (size_t)A.faces[3 * t + 1], i2 = (size_t)A.faces[3 * t + 2];
  const float Z0 = v[3 * i0 + 2], Z1 = v[3 * i1 + 2], Z2 = v[3 * i2 + 2];
  const float u0 = A.uv[2 * (size_t)k0], v0 = A.uv[2 * (size_t)k0 + 1];
  const float u1 = A.uv[2 * (size_t)k1], v1 = A.uv[2 * (size_t)k1 + 1];
  const float u2 = A.uv[2 * (size_t)k2], v2 = A.uv[2 * (size_t)k2 + 1];
  ok = Z0 - Z0 == 0.0f && Z1 - Z1 == 0.0f && Z2 - Z2 == 0.0f && Z0 > 0.0f && Z1 > 0.0f && Z2 > 0.0f;
  if (!ok) return p;
  const double q0 = (double)l0 / (double)Z0, q1 = (double)l1 / (double)Z1, q2 = (double)l2 / (double)Z2;
  const double S = (q0 + q1) + q2;
  if (!(S != 0.0)) return p;
  const double w0 = q0 / S, w1 = q1 / S, w2 = q2 / S;
  const double uu = (w0 * (double)u0 + w1 * (double)u1) + w2 * (double)u2;
  const double vv = (w0 * (double)v0 + w1 * (double)v1) + w2 * (double)v2;
  if (!(uu - uu == 0.0) || !(vv - vv == 0.0)) return p;     // a non-finite uv voids the pixel
  // the clamp, in f64, BEFORE anything becomes an integer: x and y leave here inside [0, Wt - 1] x [0, Ht - 1]
  const double xr = uu * (double)A.Wt - 0.5, yr = vv * (double)A.Ht - 0.5;
  const double xmax = (double)(A.Wt - 1), ymax = (double)(A.Ht - 1);
  p.free_x = xr >= 0.0 && xr <= xmax;
  p.free_y = yr >= 0.0 && yr <= ymax;
  p.x = xr < 0.0 ? 0.0 : (xr > xmax ? xmax : xr);
  p.y = yr < 0.0 ? 0.0 : (yr > ymax ? ymax : yr);
  p.w[0] = w0; p.w[1] = w1; p.w[2] = w2;
  p.u = uu; p.v = vv;
  p.ok = true;
  return p;
}

template <int C, typename T>
__global__ __launch_bounds__(256) void k_tx_forward(TxArgs A, const T* __restrict__ tex, float4 bg, float* __restrict__ image,
                                                    float* __restrict__ weight, float* __restrict__ uv_out) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= A.total) return;
  const TxPixel p = tx_pixel(A, o);
  const float bgc[4] = {bg.x, bg.y, bg.z, bg.w};
  float out[C];
  for (int c = 0; c < C; ++c) out[c] = bgc[c];
  if (p.ok) {
    const size_t frame = (size_t)(o / A.ppf);
    const bodyfit::BilinearCell cell = bodyfit::bilinear_cell(p.x, p.y, A.Wt, A.Ht);
    double val[C];
    bodyfit::bilinear_patch<C, T>(tex + frame * (size_t)A.tex_stride, A.Wt, cell, val, nullptr, nullptr);
    for (int c = 0; c < C; ++c) out[c] = (float)val[c];
  }
  for (int c = 0; c < C; ++c) image[C * (size_t)o + c] = out[c];
  if (weight)
    for (int k = 0; k < 3; ++k) weight[3 * (size_t)o + k] = (float)p.w[k];
  if (uv_out) { uv_out[2 * (size_t)o] = (float)p.u; uv_out[2 * (size_t)o + 1] = (float)p.v; }
}

// max over n floats of the bit pattern of |g|
__global__ __launch_bounds__(256) void k_tx_gmax(const float* __restrict__ g, long long n, unsigned* __restrict__ out) {
  unsigned m = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
  __shared__ unsigned part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(part[0], part[1]), max(part[2], part[3]));
    if (m) atomicMax(out, m);
  }
}

// s = 60 - B - E with E = (bits >> 23) - 126: max|G| < 2^E (a subnormal maximum has bits >> 23 = 0 and lies below 2^-126)
__device__ __forceinline__ int tx_scale_exponent(unsigned gbits, int B) { return 60 - B - ((int)(gbits >> 23) - 126); }

// BODYFIT_TX_COMBINE = 1: lanes of a wave whose pixels share a cell (neighbouring pixels do, under magnification) add their
// integers up inside the wave first, and the first lane of each RUN of equal cells issues the run's atomics.  Integers: the
// texel sums are the same bits either way.  Both forms were measured ("Textures"); the default is the faster.
#ifndef BODYFIT_TX_COMBINE
#define BODYFIT_TX_COMBINE 1
#endif

template <int C, typename T>
__global__ __launch_bounds__(256) void k_tx_grad(TxArgs A, const T* __restrict__ tex, const float* __restrict__ grad_image,
                                                 const unsigned* __restrict__ gmax, int B, float* __restrict__ grad_uv,
                                                 unsigned long long* __restrict__ sums) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = o < A.total;       // (no early return: with BODYFIT_TX_COMBINE every lane of the wave reaches the shuffles)
  const unsigned gbits = *gmax;
  double gu = 0.0, gv = 0.0;
  long long q[4][C];
  for (int k = 0; k < 4; ++k)
    for (int c = 0; c < C; ++c) q[k][c] = 0;
  long long key = -1;                // the lane's cell (with its frame, for per-frame textures); -1: nothing to add
  size_t at[4] = {0, 0, 0, 0};
  if (in && gbits != 0u && gbits < 0x7f800000u) {       // (all G zero: nothing to add; a NaN or an infinity: the fold writes NaN)
    const TxPixel p = tx_pixel(A, o);
    if (p.ok) {
      const size_t frame = (size_t)(o / A.ppf);
      const bodyfit::BilinearCell cell = bodyfit::bilinear_cell(p.x, p.y, A.Wt, A.Ht);
      double G[C];
      for (int c = 0; c < C; ++c) G[c] = (double)grad_image[C * (size_t)o + c];
      if (grad_uv) {
        double val[C], du[C], dv[C];
        bodyfit::bilinear_patch<C, T>(tex + frame * (size_t)A.tex_stride, A.Wt, cell, val, du, dv);
        double su = 0.0, sv = 0.0;
        for (int c = 0; c < C; ++c) {
          const double tu = G[c] * du[c], tv = G[c] * dv[c];
          su = c == 0 ? tu : su + tu;
          sv = c == 0 ? tv : sv + tv;
        }
        gu = p.free_x ? su * (double)A.Wt : 0.0;
        gv = p.free_y ? sv * (double)A.Ht : 0.0;
      }
      if (sums) {
        const double scale = ldexp(1.0, tx_scale_exponent(gbits, B));     // |s| <= 186: a normal f64, the products below exact
        double w[4];
        bodyfit::bilinear_weights(cell, w);
        const size_t f0 = A.tex_stride ? frame * ((size_t)A.Ht * A.Wt * C) : 0;
        at[0] = f0 + ((size_t)cell.i0 * A.Wt + cell.j0) * C; at[1] = f0 + ((size_t)cell.i0 * A.Wt + cell.j1) * C;
        at[2] = f0 + ((size_t)cell.i1 * A.Wt + cell.j0) * C; at[3] = f0 + ((size_t)cell.i1 * A.Wt + cell.j1) * C;
        key = (long long)at[0];
        for (int k = 0; k < 4; ++k)
          for (int c = 0; c < C; ++c) {
            const double t = G[c] * w[k];          // rounds once
            q[k][c] = llrint(t * scale);           // exact scaling, round to nearest
          }
      }
    }
  }
  bool issue = key >= 0;
#if BODYFIT_TX_COMBINE
  if (sums && __ballot(key >= 0) != 0ull) {        // (wave-uniform: most waves of an image hold no covered pixel)
    const int lane = threadIdx.x & 63;
    const long long prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);      // (by ALL lanes, before anything lane-dependent: a ballot only sees active lanes)
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run_end = later ? lane + 1 + __ffsll((long long)later) - 1 : 64;     // the first lane of the next run
    for (int d = 1; d < 64; d <<= 1) {             // a suffix sum inside the run: after the step q covers [lane, lane + 2 d)
      const bool take = lane + d < run_end;
      for (int k = 0; k < 4; ++k)
        for (int c = 0; c < C; ++c) {
          const long long other = __shfl_down(q[k][c], d, 64);
          if (take) q[k][c] += other;
        }
    }
    issue = head && key >= 0;
  }
#endif
  if (issue)
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < C; ++c)
        if (q[k][c] != 0) atomicAdd(sums + at[k] + c, (unsigned long long)q[k][c]);     // (the result is not used: a no-return add)
  if (in && grad_uv) { grad_uv[2 * (size_t)o] = (float)gu; grad_uv[2 * (size_t)o + 1] = (float)gv; }
}

__global__ __launch_bounds__(256) void k_tx_fold(const unsigned long long* __restrict__ sums, long long n,
                                                 const unsigned* __restrict__ gmax, int B, float* __restrict__ grad_tex) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned gbits = *gmax;
  float r;
  if (gbits >= 0x7f800000u) r = __uint_as_float(0x7fc00000u);
  else r = (float)((double)(long long)sums[i] * ldexp(1.0, -tx_scale_exponent(gbits, B)));
  grad_tex[i] = r;
}

// what the two entries check alike; *work: there are pixels to write
int tx_check(const char* fn, const bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
             long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces, int tex_kind, int n_channels,
             int tex_height, int tex_width, long long tex_frame_stride, int n_frames, bool* work) {
  *work = false;
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (tex_kind != 0 && tex_kind != 1) return invalid_arg(fn, "tex_kind must be 0 (u8) or 1 (f32)");
  if (tex_height < 1 || tex_width < 1 || tex_height > 16384 || tex_width > 16384)
    return invalid_arg(fn, "texture size outside 1 .. 16384");
  if (n_uv < 0) return invalid_arg(fn, "negative n_uv");
  if (tex_frame_stride != 0 && tex_frame_stride < (long long)tex_height * tex_width * n_channels)
    return invalid_arg(fn, "a non-zero tex_frame_stride below Ht Wt n_channels");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_face || !d_bary) return invalid_arg(fn, "d_face or d_bary is NULL");
  if (r->nF > 0 && (!d_verts || !d_uv_faces)) return invalid_arg(fn, "d_verts or d_uv_faces is NULL");
  if (r->nF > 0 && n_uv > 0 && !d_uv) return invalid_arg(fn, "d_uv is NULL");
  if (int rc = rs_check_verts_stride(fn, r, verts_frame_stride)) return rc;
  if (int rc = rs_check_pixels(fn, r, n_frames)) return rc;
  *work = true;
  return BODYFIT_OK;
}

TxArgs tx_args(const bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
               long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces, int tex_height, int tex_width,
               long long tex_frame_stride, int n_frames) {
  TxArgs A;
  A.face_img = d_face; A.bary = d_bary; A.verts = d_verts; A.verts_stride = verts_frame_stride; A.faces = r->d_faces;
  A.uv = d_uv; A.uv_faces = d_uv_faces; A.nF = r->nF; A.T = n_uv; A.Wt = tex_width; A.Ht = tex_height;
  A.tex_stride = tex_frame_stride; A.ppf = (long long)r->W * r->H; A.total = A.ppf * n_frames;
  return A;
}

// launch(channel count, a null pointer of the texel type): u8 or f32 texels by tex_kind
template <typename Launch>
void tx_dispatch(int tex_kind, int C, Launch&& launch) {
  rs_dispatch_channels(C, [&](auto c) {
    if (tex_kind == 0) launch(c, (const uint8_t*)nullptr);
    else launch(c, (const float*)nullptr);
  });
}

// ---- mipmaps: the pyramid, the lookup with a level of detail, its gradients (include/bodyfit.h, MIPMAPS OF THE TEXTURE LOOKUP) -------
//   k_txm_build<T>   one thread per element of level l + 1: the average of its 4 (or 2) children of the STORED level l in f64,
//                rounded once to f32.  One launch per level, plain stores.
//   k_txm_forward<C, T>  tx_pixel's pixel, then the footprint from the face's projected corners (txm_lod), then one or two
//                bilinear patches, each level with its own clamp and cell; where f = 0 only level l0 is read.
//   k_txm_grad<C, T>  the same pixel and level again; (a) the levels' patch derivatives blended; (b) 4 C contributions to level l0
//                and, where f != 0, 4 C to level l0 + 1, as integers into the packed int64 pyramid (level 0 first).
//   k_txm_fold   one thread per level-0 texel element: the fixed-order gather over the levels.
struct TxMip {
  double fx, fy, cx, cy;
  const float* mip;          // levels 1 .. n - 1, packed; per frame mip_stride elements apart (shared: 0)
  long long mip_stride;
  long long off[BODYFIT_TX_MAX_LEVELS];     // TEXEL offset of level l in the packed buffer (off[0] unused)
  int Hl[BODYFIT_TX_MAX_LEVELS], Wl[BODYFIT_TX_MAX_LEVELS];
  int n_levels;
  float lod_bias;
};

// the layout (host): level l + 1 exists iff l < max_level, (H_l, W_l) != (1, 1) and each of H_l, W_l is even or 1
int txm_layout(int Ht, int Wt, int max_level, int* Hl, int* Wl, long long* off, long long* total) {
  int n = 1;
  Hl[0] = Ht; Wl[0] = Wt; off[0] = 0;
  long long at = 0;
  while (n < BODYFIT_TX_MAX_LEVELS && (max_level < 0 || n <= max_level)) {
    const int h = Hl[n - 1], w = Wl[n - 1];
    if ((h == 1 && w == 1) || (h > 1 && (h & 1)) || (w > 1 && (w & 1))) break;
    Hl[n] = h > 1 ? h / 2 : 1; Wl[n] = w > 1 ? w / 2 : 1;
    off[n] = at;
    at += (long long)Hl[n] * Wl[n];
    ++n;
  }
  *total = at;
  return n;
}

template <typename T>
__global__ __launch_bounds__(256) void k_txm_build(const T* __restrict__ src, long long src_stride, int Hs, int Ws, int C,
                                                   float* __restrict__ dst, long long dst_stride, int Hd, int Wd, long long per_tex,
                                                   long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long tex = e / per_tex, r = e - tex * per_tex;       // r = (i Wd + j) C + c
  const int c = (int)(r % C);
  const long long ij = r / C;
  const int i = (int)(ij / Wd), j = (int)(ij - (long long)i * Wd);
  const T* s = src + tex * src_stride;
  const int di = Hs > 1 ? 1 : 0, dj = Ws > 1 ? 1 : 0;             // a dimension of 1 stays 1
  const size_t i0 = (size_t)(Hs > 1 ? 2 * i : 0), j0 = (size_t)(Ws > 1 ? 2 * j : 0);
  double v;
  if (di && dj) {
    const double t00 = (double)s[(i0 * Ws + j0) * C + c], t01 = (double)s[(i0 * Ws + j0 + 1) * C + c];
    const double t10 = (double)s[((i0 + 1) * Ws + j0) * C + c], t11 = (double)s[((i0 + 1) * Ws + j0 + 1) * C + c];
    v = ((t00 + t01) + (t10 + t11)) * 0.25;
  } else {
    const double t0 = (double)s[(i0 * Ws + j0) * C + c], t1 = (double)s[((i0 + di) * Ws + j0 + dj) * C + c];
    v = (t0 + t1) * 0.5;
  }
  dst[tex * dst_stride + r] = (float)v;
}

// The level of detail of a live pixel: L = clamp(log2(rho^2) / 2 + lod_bias, 0, n_levels - 1), rho^2 the largest eigenvalue of J J^T,
// J = diag(Wt, Ht) d(uv)/d(sample) from the face's projected corners.  0 where rho^2, the area or a corner is not finite or A = 0.
__device__ __forceinline__ double txm_lod(const TxArgs& A, const TxMip& M, long long o, const TxPixel& p) {
  if (M.n_levels <= 1) return 0.0;
  const int t = A.face_img[o];
  const size_t frame = (size_t)(o / A.ppf);
  const float* v = A.verts + frame * (size_t)A.verts_stride;
  double px[3], py[3], Z[3], du[3], dv[3];
  bool fin = true;
  for (int a = 0; a < 3; ++a) {
    const size_t id = (size_t)A.faces[3 * t + a];
    const float X = v[3 * id], Y = v[3 * id + 1], Zf = v[3 * id + 2];
    if (!(X - X == 0.0f) || !(Y - Y == 0.0f)) fin = false;
    Z[a] = (double)Zf;                                       // (finite and > 0: tx_pixel's rule)
    px[a] = M.fx * ((double)X / Z[a]) + M.cx;
    py[a] = M.fy * ((double)Y / Z[a]) + M.cy;
    const int k = A.uv_faces[3 * t + a];
    du[a] = (double)A.uv[2 * (size_t)k] - p.u;
    dv[a] = (double)A.uv[2 * (size_t)k + 1] - p.v;
  }
  if (!fin) return 0.0;
  const double area = (px[1] - px[0]) * (py[2] - py[0]) - (px[2] - px[0]) * (py[1] - py[0]);
  if (!(area != 0.0) || !(area - area == 0.0)) return 0.0;
  const float l0 = A.bary[3 * (size_t)o], l1 = A.bary[3 * (size_t)o + 1], l2 = A.bary[3 * (size_t)o + 2];
  const double S = ((double)l0 / Z[0] + (double)l1 / Z[1]) + (double)l2 / Z[2];      // tx_pixel's S, the same bits
  double hx[3], hy[3];
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    hx[a] = ((py[b] - py[c]) / area) / Z[a];
    hy[a] = ((px[c] - px[b]) / area) / Z[a];
  }
  const double ux = ((hx[0] * du[0] + hx[1] * du[1]) + hx[2] * du[2]) / S, uy = ((hy[0] * du[0] + hy[1] * du[1]) + hy[2] * du[2]) / S;
  const double vx = ((hx[0] * dv[0] + hx[1] * dv[1]) + hx[2] * dv[2]) / S, vy = ((hy[0] * dv[0] + hy[1] * dv[1]) + hy[2] * dv[2]) / S;
  const double j00 = (double)A.Wt * ux, j01 = (double)A.Wt * uy, j10 = (double)A.Ht * vx, j11 = (double)A.Ht * vy;
  const double ca = j00 * j00 + j10 * j10, cb = j01 * j01 + j11 * j11, cc = j00 * j01 + j10 * j11;
  const double hs = 0.5 * (ca + cb), hd = 0.5 * (ca - cb);
  const double rho2 = hs + sqrt(hd * hd + cc * cc);
  if (!(rho2 - rho2 == 0.0)) return 0.0;
  const double Lr = 0.5 * log2(rho2) + (double)M.lod_bias;
  const double top = (double)(M.n_levels - 1);
  const double Lc = !(Lr > 0.0) ? 0.0 : (Lr > top ? top : Lr);      // (a NaN, from -inf + inf, is 0 as well)
  return (double)(float)Lc;          // d_lod's f32 IS the L that is used: the gradients' contracts are stated at the returned L
}

// one level's clamp (tx_pixel's, with the level's size) and cell
struct TxmLevel {
  bool free_x, free_y;
  bodyfit::BilinearCell cell;
};

__device__ __forceinline__ TxmLevel txm_level(const TxPixel& p, int Wl, int Hl) {
  TxmLevel r;
  const double xr = p.u * (double)Wl - 0.5, yr = p.v * (double)Hl - 0.5;
  const double xmax = (double)(Wl - 1), ymax = (double)(Hl - 1);
  r.free_x = xr >= 0.0 && xr <= xmax;
  r.free_y = yr >= 0.0 && yr <= ymax;
  const double x = xr < 0.0 ? 0.0 : (xr > xmax ? xmax : xr);
  const double y = yr < 0.0 ? 0.0 : (yr > ymax ? ymax : yr);
  r.cell = bodyfit::bilinear_cell(x, y, Wl, Hl);
  return r;
}

// value and derivatives of level l's patch at the pixel (level 0: the texture in its own type; l > 0: the f32 pyramid)
template <int C, typename T>
__device__ __forceinline__ void txm_patch(const TxArgs& A, const TxMip& M, const T* tex, size_t frame, int l, const TxmLevel& lv,
                                          double* val, double* du, double* dv) {
  if (l == 0) bodyfit::bilinear_patch<C, T>(tex + frame * (size_t)A.tex_stride, A.Wt, lv.cell, val, du, dv);
  else bodyfit::bilinear_patch<C, float>(M.mip + frame * (size_t)M.mip_stride + (size_t)M.off[l] * C, M.Wl[l], lv.cell, val, du, dv);
}

template <int C, typename T>
__global__ __launch_bounds__(256) void k_txm_forward(TxArgs A, TxMip M, const T* __restrict__ tex, float4 bg,
                                                     float* __restrict__ image, float* __restrict__ weight,
                                                     float* __restrict__ uv_out, float* __restrict__ lod) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= A.total) return;
  const TxPixel p = tx_pixel(A, o);
  const float bgc[4] = {bg.x, bg.y, bg.z, bg.w};
  float out[C];
  for (int c = 0; c < C; ++c) out[c] = bgc[c];
  double L = 0.0;
  if (p.ok) {
    const size_t frame = (size_t)(o / A.ppf);
    L = txm_lod(A, M, o, p);
    const int l0 = (int)floor(L);
    const double f = L - (double)l0;
    double val[C];
    txm_patch<C, T>(A, M, tex, frame, l0, txm_level(p, M.Wl[l0], M.Hl[l0]), val, nullptr, nullptr);
    if (f != 0.0) {
      double val1[C];
      txm_patch<C, T>(A, M, tex, frame, l0 + 1, txm_level(p, M.Wl[l0 + 1], M.Hl[l0 + 1]), val1, nullptr, nullptr);
      const double nf = 1.0 - f;
      for (int c = 0; c < C; ++c) val[c] = nf * val[c] + f * val1[c];
    }
    for (int c = 0; c < C; ++c) out[c] = (float)val[c];
  }
  for (int c = 0; c < C; ++c) image[C * (size_t)o + c] = out[c];
  if (weight)
    for (int k = 0; k < 3; ++k) weight[3 * (size_t)o + k] = (float)p.w[k];
  if (uv_out) { uv_out[2 * (size_t)o] = (float)p.u; uv_out[2 * (size_t)o + 1] = (float)p.v; }
  if (lod) lod[o] = (float)L;
}

// BODYFIT_TXM_COMBINE = 1: k_tx_grad's run combining with the key (level, cell) of BOTH levels of the lane.  The same bits either
// way (integers); measured both ways, magnified and minified ("Mipmaps"): combining is the faster in both, and the default.
#ifndef BODYFIT_TXM_COMBINE
#define BODYFIT_TXM_COMBINE 1
#endif

template <int C, typename T>
__global__ __launch_bounds__(256) void k_txm_grad(TxArgs A, TxMip M, const T* __restrict__ tex, const float* __restrict__ grad_image,
                                                  const unsigned* __restrict__ gmax, int B, long long pyramid,
                                                  float* __restrict__ grad_uv, unsigned long long* __restrict__ sums) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = o < A.total;       // (no early return: with BODYFIT_TXM_COMBINE every lane of the wave reaches the shuffles)
  const unsigned gbits = *gmax;
  double gu = 0.0, gv = 0.0;
  long long q[8][C];                 // 0 .. 3: level l0's texels, 4 .. 7: level l0 + 1's
  for (int k = 0; k < 8; ++k)
    for (int c = 0; c < C; ++c) q[k][c] = 0;
  long long key0 = -1, key1 = -1;    // the lane's cells in the packed pyramid (with its frame, for per-frame textures); -1: none
  size_t at[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (in && gbits != 0u && gbits < 0x7f800000u) {
    const TxPixel p = tx_pixel(A, o);
    if (p.ok) {
      const size_t frame = (size_t)(o / A.ppf);
      const double L = txm_lod(A, M, o, p);
      const int l0 = (int)floor(L);
      const double f = L - (double)l0, nf = 1.0 - f;
      const int n_lv = f != 0.0 ? 2 : 1;
      double G[C];
      for (int c = 0; c < C; ++c) G[c] = (double)grad_image[C * (size_t)o + c];
      const double scale = ldexp(1.0, tx_scale_exponent(gbits, B));
      const size_t f0 = A.tex_stride ? frame * (size_t)pyramid * C : 0;
      // (a constant trip count, unrolled: q and at are indexed with compile-time constants and stay in registers)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (n >= n_lv) break;
        const int l = l0 + n, Wl = M.Wl[l], Hl = M.Hl[l];
        const TxmLevel lv = txm_level(p, Wl, Hl);
        if (grad_uv) {
          double val[C], du[C], dv[C];
          txm_patch<C, T>(A, M, tex, frame, l, lv, val, du, dv);
          double su = 0.0, sv = 0.0;
          for (int c = 0; c < C; ++c) {
            const double tu = G[c] * du[c], tv = G[c] * dv[c];
            su = c == 0 ? tu : su + tu;
            sv = c == 0 ? tv : sv + tv;
          }
          const double lu = lv.free_x ? su * (double)Wl : 0.0, lw = lv.free_y ? sv * (double)Hl : 0.0;
          if (n_lv == 1) { gu = lu; gv = lw; }
          else if (n == 0) { gu = nf * lu; gv = nf * lw; }
          else { gu = gu + f * lu; gv = gv + f * lw; }
        }
        if (sums) {
          double w[4];
          bodyfit::bilinear_weights(lv.cell, w);
          const size_t base = f0 + (l == 0 ? (size_t)0 : ((size_t)A.Ht * A.Wt + (size_t)M.off[l]) * C);
          const bodyfit::BilinearCell& k = lv.cell;
          at[4 * n + 0] = base + ((size_t)k.i0 * Wl + k.j0) * C; at[4 * n + 1] = base + ((size_t)k.i0 * Wl + k.j1) * C;
          at[4 * n + 2] = base + ((size_t)k.i1 * Wl + k.j0) * C; at[4 * n + 3] = base + ((size_t)k.i1 * Wl + k.j1) * C;
          (n == 0 ? key0 : key1) = (long long)at[4 * n];
          const double share = n == 0 ? nf : f;
          for (int kk = 0; kk < 4; ++kk) {
            const double wk = n_lv == 1 ? w[kk] : share * w[kk];     // (f = 0: the plain entry's contribution, operation for operation)
            for (int c = 0; c < C; ++c) {
              const double tt = G[c] * wk;           // rounds once
              q[4 * n + kk][c] = llrint(tt * scale); // exact scaling, round to nearest
            }
          }
        }
      }
    }
  }
  bool issue = key0 >= 0;
#if BODYFIT_TXM_COMBINE
  if (sums && __ballot(key0 >= 0) != 0ull) {
    const int lane = threadIdx.x & 63;
    const long long prev0 = __shfl_up(key0, 1, 64), prev1 = __shfl_up(key1, 1, 64);
    const bool head = lane == 0 || prev0 != key0 || prev1 != key1;
    const unsigned long long heads = __ballot(head);
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run_end = later ? lane + 1 + __ffsll((long long)later) - 1 : 64;
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = lane + d < run_end;
      for (int k = 0; k < 8; ++k)
        for (int c = 0; c < C; ++c) {
          const long long other = __shfl_down(q[k][c], d, 64);
          if (take) q[k][c] += other;
        }
    }
    issue = head && key0 >= 0;
  }
#endif
  if (issue)
    for (int k = 0; k < 8; ++k)
      for (int c = 0; c < C; ++c)
        if (q[k][c] != 0) atomicAdd(sums + at[k] + c, (unsigned long long)q[k][c]);     // (no-return)
  if (in && grad_uv) { grad_uv[2 * (size_t)o] = (float)gu; grad_uv[2 * (size_t)o + 1] = (float)gv; }
}

// One thread per level-0 texel element: sum_l (double)S_l[i_l][j_l][c] 2^-s a_l in the order l = 0, 1, ..., a_l the exact product of
// the 1/4 (both dimensions halved) and 1/2 (one of them) factors; (i_l, j_l) the ancestor of (i, j) on level l.
__global__ __launch_bounds__(256) void k_txm_fold(const unsigned long long* __restrict__ sums, TxMip M, int C, long long pyramid,
                                                  long long n, const unsigned* __restrict__ gmax, int B,
                                                  float* __restrict__ grad_tex) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const unsigned gbits = *gmax;
  if (gbits >= 0x7f800000u) { grad_tex[e] = __uint_as_float(0x7fc00000u); return; }
  const long long per = (long long)M.Hl[0] * M.Wl[0] * C;
  const long long tex = e / per, r = e - tex * per;
  const int c = (int)(r % C);
  const long long ij = r / C;
  int i = (int)(ij / M.Wl[0]), j = (int)(ij - (long long)i * M.Wl[0]);
  const double unit = ldexp(1.0, -tx_scale_exponent(gbits, B));
  const unsigned long long* s = sums + tex * pyramid * C;
  double acc = (double)(long long)s[r] * unit;
  double al = 1.0;
  for (int l = 1; l < M.n_levels; ++l) {
    const bool hi = M.Hl[l - 1] > 1, hj = M.Wl[l - 1] > 1;
    if (hi) i >>= 1;
    if (hj) j >>= 1;
    al = al * (hi && hj ? 0.25 : 0.5);
    const size_t idx = (((size_t)M.Hl[0] * M.Wl[0] + (size_t)M.off[l]) + ((size_t)i * M.Wl[l] + j)) * C + c;
    acc = acc + ((double)(long long)s[idx] * unit) * al;
  }
  grad_tex[e] = (float)acc;
}

// the arguments the mip entries add to tx_check's; n_levels > 1 needs the pyramid
int txm_check(const char* fn, double fx, double fy, double cx, double cy, float lod_bias, int n_levels, long long total,
              int n_channels, const float* d_mip, long long tex_frame_stride, long long mip_frame_stride) {
  if (!rs_intrinsics_ok(fx, fy, cx, cy)) return invalid_arg(fn, "fx or fy <= 0 or a non-finite intrinsic");      // (this entry's wording)
  if (lod_bias != lod_bias) return invalid_arg(fn, "lod_bias is NaN");
  if (n_levels > 1 && !d_mip) return invalid_arg(fn, "d_mip is NULL with more than one level");
  if (n_levels > 1 && tex_frame_stride != 0 && mip_frame_stride < total * n_channels)
    return invalid_arg(fn, "mip_frame_stride below the layout's total");
  return BODYFIT_OK;
}

TxMip txm_args(double fx, double fy, double cx, double cy, const float* d_mip, long long tex_frame_stride, long long mip_frame_stride,
               int tex_height, int tex_width, int max_level, float lod_bias, long long* total) {
  TxMip M;
  M.fx = fx; M.fy = fy; M.cx = cx; M.cy = cy; M.mip = d_mip; M.mip_stride = tex_frame_stride ? mip_frame_stride : 0;
  for (int l = 0; l < BODYFIT_TX_MAX_LEVELS; ++l) { M.Hl[l] = M.Wl[l] = 1; M.off[l] = 0; }
  M.n_levels = txm_layout(tex_height, tex_width, max_level, M.Hl, M.Wl, M.off, total);
  M.lod_bias = lod_bias;
  return M;
}

}  // namespace

extern "C" {

int bodyfit_raster_texture_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                  long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                  const void* d_tex, int tex_kind, int n_channels, int tex_height, int tex_width,
                                  long long tex_frame_stride, int n_frames, const float* background, float* d_image,
                                  float* d_weight, float* d_uv_out, void* stream) {
  const char* fn = "bodyfit_raster_texture_device";
  bool work = false;
  if (int rc = tx_check(fn, r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_kind, n_channels,
                        tex_height, tex_width, tex_frame_stride, n_frames, &work))
    return rc;
  if (!work) return BODYFIT_OK;
  if (!d_image) return invalid_arg(fn, "d_image is NULL");
  if (r->nF > 0 && !d_tex) return invalid_arg(fn, "d_tex is NULL");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TxArgs A = tx_args(r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_height, tex_width,
                           tex_frame_stride, n_frames);
  const float4 bg = background ? make_float4(background[0], background[1], background[2], background[3])
                               : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const dim3 grid((unsigned)((A.total + 255) / 256));
  tx_dispatch(tex_kind, n_channels, [&](auto c, auto* type) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(type)>>;
    BODYFIT_LAUNCH((k_tx_forward<decltype(c)::value, T>), grid, dim3(256), 0, st, A, static_cast<const T*>(d_tex), bg, d_image,
                   d_weight, d_uv_out);
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_texture_grad_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                       long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                       const void* d_tex, int tex_kind, int n_channels, int tex_height, int tex_width,
                                       long long tex_frame_stride, int n_frames, const float* d_grad_image, float* d_grad_uv,
                                       float* d_grad_tex, long long* d_workspace, void* stream) {
  const char* fn = "bodyfit_raster_texture_grad_device";
  bool work = false;
  if (int rc = tx_check(fn, r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_kind, n_channels,
                        tex_height, tex_width, tex_frame_stride, n_frames, &work))
    return rc;
  if (!work || (!d_grad_uv && !d_grad_tex)) return BODYFIT_OK;
  if (!d_grad_image) return invalid_arg(fn, "d_grad_image is NULL");
  if (d_grad_tex && !d_workspace) return invalid_arg(fn, "d_grad_tex without d_workspace");
  if (r->nF > 0 && d_grad_uv && !d_tex) return invalid_arg(fn, "d_grad_uv without d_tex");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TxArgs A = tx_args(r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_height, tex_width,
                           tex_frame_stride, n_frames);
  int B = 0;      // the bit length of the pixel count: total < 2^B
  while ((A.total >> B) != 0) ++B;
  const long long n_tex = (long long)tex_height * tex_width * n_channels * (tex_frame_stride ? n_frames : 1);
  const long long n_grad = A.total * n_channels;
  if (d_grad_tex && n_tex >= (1ll << 39)) return invalid_arg(fn, "2^39 texel elements or more in one call");
  HIP_TRY(hipMemsetAsync(r->scratch_word(), 0, sizeof(unsigned), st));
  if (d_grad_tex) HIP_TRY(hipMemsetAsync(d_workspace, 0, (size_t)n_tex * sizeof(long long), st));
  const unsigned mblocks = (unsigned)std::min<long long>((n_grad + 255) / 256, 4096);
  BODYFIT_LAUNCH(k_tx_gmax, dim3(mblocks), dim3(256), 0, st, d_grad_image, n_grad, r->scratch_word());
  const dim3 grid((unsigned)((A.total + 255) / 256));
  unsigned long long* sums = d_grad_tex ? reinterpret_cast<unsigned long long*>(d_workspace) : nullptr;
  tx_dispatch(tex_kind, n_channels, [&](auto c, auto* type) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(type)>>;
    BODYFIT_LAUNCH((k_tx_grad<decltype(c)::value, T>), grid, dim3(256), 0, st, A, static_cast<const T*>(d_tex), d_grad_image,
                   r->scratch_word(), B, d_grad_uv, sums);
  });
  if (d_grad_tex)
    BODYFIT_LAUNCH(k_tx_fold, dim3((unsigned)((n_tex + 255) / 256)), dim3(256), 0, st, sums, n_tex, r->scratch_word(), B, d_grad_tex);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_texture_mip_layout(int tex_height, int tex_width, int max_level, int* n_levels, int* heights, int* widths,
                               long long* offsets, long long* total) {
  const char* fn = "bodyfit_texture_mip_layout";
  if (tex_height < 1 || tex_width < 1 || tex_height > 16384 || tex_width > 16384)
    return invalid_arg(fn, "texture size outside 1 .. 16384");
  if (!n_levels) return invalid_arg(fn, "n_levels is NULL");
  int Hl[BODYFIT_TX_MAX_LEVELS], Wl[BODYFIT_TX_MAX_LEVELS];
  long long off[BODYFIT_TX_MAX_LEVELS], tot = 0;
  const int n = txm_layout(tex_height, tex_width, max_level, Hl, Wl, off, &tot);
  *n_levels = n;
  for (int l = 0; l < n; ++l) {
    if (heights) heights[l] = Hl[l];
    if (widths) widths[l] = Wl[l];
    if (offsets) offsets[l] = off[l];
  }
  if (total) *total = tot;
  return BODYFIT_OK;
}

int bodyfit_raster_texture_mip_build_device(bodyfit_raster* r, const void* d_tex, int tex_kind, int n_channels, int tex_height,
                                            int tex_width, long long tex_frame_stride, int n_textures, int max_level, float* d_mip,
                                            long long mip_frame_stride, void* stream) {
  const char* fn = "bodyfit_raster_texture_mip_build_device";
  if (!r) return invalid_arg(fn, "handle is NULL");
  if (n_textures < 0) return invalid_arg(fn, "negative n_textures");
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (tex_kind != 0 && tex_kind != 1) return invalid_arg(fn, "tex_kind must be 0 (u8) or 1 (f32)");
  if (tex_height < 1 || tex_width < 1 || tex_height > 16384 || tex_width > 16384)
    return invalid_arg(fn, "texture size outside 1 .. 16384");
  TxMip M;
  long long total = 0;
  M.n_levels = txm_layout(tex_height, tex_width, max_level, M.Hl, M.Wl, M.off, &total);
  if (n_textures > 1 && tex_frame_stride < (long long)tex_height * tex_width * n_channels)
    return invalid_arg(fn, "tex_frame_stride below Ht Wt n_channels");
  if (n_textures > 1 && M.n_levels > 1 && mip_frame_stride < total * n_channels)
    return invalid_arg(fn, "mip_frame_stride below the layout's total");
  if (n_textures == 0 || M.n_levels == 1) return BODYFIT_OK;
  if (!d_tex || !d_mip) return invalid_arg(fn, "d_tex or d_mip is NULL");
  if (total * n_channels * n_textures >= (1ll << 39)) return invalid_arg(fn, "2^39 pyramid elements or more in one call");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = n_channels;
  for (int l = 1; l < M.n_levels; ++l) {
    const long long per = (long long)M.Hl[l] * M.Wl[l] * C, n = per * n_textures;
    const dim3 grid((unsigned)((n + 255) / 256));
    float* dst = d_mip + M.off[l] * C;
    if (l == 1 && tex_kind == 0)
      BODYFIT_LAUNCH(k_txm_build<uint8_t>, grid, dim3(256), 0, st, static_cast<const uint8_t*>(d_tex), tex_frame_stride, M.Hl[0],
                     M.Wl[0], C, dst, mip_frame_stride, M.Hl[1], M.Wl[1], per, n);
    else if (l == 1)
      BODYFIT_LAUNCH(k_txm_build<float>, grid, dim3(256), 0, st, static_cast<const float*>(d_tex), tex_frame_stride, M.Hl[0], M.Wl[0],
                     C, dst, mip_frame_stride, M.Hl[1], M.Wl[1], per, n);
    else
      BODYFIT_LAUNCH(k_txm_build<float>, grid, dim3(256), 0, st, static_cast<const float*>(d_mip + M.off[l - 1] * C), mip_frame_stride,
                     M.Hl[l - 1], M.Wl[l - 1], C, dst, mip_frame_stride, M.Hl[l], M.Wl[l], per, n);
  }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_texture_mip_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                      long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                      const void* d_tex, int tex_kind, int n_channels, int tex_height, int tex_width,
                                      long long tex_frame_stride, int n_frames, double fx, double fy, double cx, double cy,
                                      const float* d_mip, long long mip_frame_stride, int max_level, float lod_bias,
                                      const float* background, float* d_image, float* d_weight, float* d_uv_out, float* d_lod,
                                      void* stream) {
  const char* fn = "bodyfit_raster_texture_mip_device";
  bool work = false;
  if (int rc = tx_check(fn, r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_kind, n_channels,
                        tex_height, tex_width, tex_frame_stride, n_frames, &work))
    return rc;
  long long total = 0;
  const TxMip M = txm_args(fx, fy, cx, cy, d_mip, tex_frame_stride, mip_frame_stride, tex_height, tex_width, max_level, lod_bias,
                           &total);
  if (int rc = txm_check(fn, fx, fy, cx, cy, lod_bias, M.n_levels, total, n_channels, d_mip, tex_frame_stride, mip_frame_stride))
    return rc;
  if (!work) return BODYFIT_OK;
  if (!d_image) return invalid_arg(fn, "d_image is NULL");
  if (r->nF > 0 && !d_tex) return invalid_arg(fn, "d_tex is NULL");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TxArgs A = tx_args(r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_height, tex_width,
                           tex_frame_stride, n_frames);
  const float4 bg = background ? make_float4(background[0], background[1], background[2], background[3])
                               : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const dim3 grid((unsigned)((A.total + 255) / 256));
  tx_dispatch(tex_kind, n_channels, [&](auto c, auto* type) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(type)>>;
    BODYFIT_LAUNCH((k_txm_forward<decltype(c)::value, T>), grid, dim3(256), 0, st, A, M, static_cast<const T*>(d_tex), bg, d_image,
                   d_weight, d_uv_out, d_lod);
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_texture_mip_grad_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                           long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                           const void* d_tex, int tex_kind, int n_channels, int tex_height, int tex_width,
                                           long long tex_frame_stride, int n_frames, double fx, double fy, double cx, double cy,
                                           const float* d_mip, long long mip_frame_stride, int max_level, float lod_bias,
                                           const float* d_grad_image, float* d_grad_uv, float* d_grad_tex, long long* d_workspace,
                                           void* stream) {
  const char* fn = "bodyfit_raster_texture_mip_grad_device";
  bool work = false;
  if (int rc = tx_check(fn, r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_kind, n_channels,
                        tex_height, tex_width, tex_frame_stride, n_frames, &work))
    return rc;
  long long total = 0;
  // (the pyramid is read for d_grad_uv only: without it d_mip may be NULL, as d_tex)
  const TxMip M = txm_args(fx, fy, cx, cy, d_mip, tex_frame_stride, mip_frame_stride, tex_height, tex_width, max_level, lod_bias,
                           &total);
  if (int rc = txm_check(fn, fx, fy, cx, cy, lod_bias, d_grad_uv ? M.n_levels : 1, total, n_channels, d_mip, tex_frame_stride,
                         mip_frame_stride))
    return rc;
  if (!work || (!d_grad_uv && !d_grad_tex)) return BODYFIT_OK;
  if (!d_grad_image) return invalid_arg(fn, "d_grad_image is NULL");
  if (d_grad_tex && !d_workspace) return invalid_arg(fn, "d_grad_tex without d_workspace");
  if (r->nF > 0 && d_grad_uv && !d_tex) return invalid_arg(fn, "d_grad_uv without d_tex");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TxArgs A = tx_args(r, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_height, tex_width,
                           tex_frame_stride, n_frames);
  int B = 0;      // the bit length of the pixel count: total < 2^B
  while ((A.total >> B) != 0) ++B;
  const long long n_textures = tex_frame_stride ? n_frames : 1;
  const long long pyramid = (long long)tex_height * tex_width + total;       // texels of one pyramid, level 0 first
  const long long n_tex = (long long)tex_height * tex_width * n_channels * n_textures;
  const long long n_work = pyramid * n_channels * n_textures;
  const long long n_grad = A.total * n_channels;
  if (d_grad_tex && n_work >= (1ll << 39)) return invalid_arg(fn, "2^39 pyramid elements or more in one call");
  HIP_TRY(hipMemsetAsync(r->scratch_word(), 0, sizeof(unsigned), st));
  if (d_grad_tex) HIP_TRY(hipMemsetAsync(d_workspace, 0, (size_t)n_work * sizeof(long long), st));
  const unsigned mblocks = (unsigned)std::min<long long>((n_grad + 255) / 256, 4096);
  BODYFIT_LAUNCH(k_tx_gmax, dim3(mblocks), dim3(256), 0, st, d_grad_image, n_grad, r->scratch_word());
  const dim3 grid((unsigned)((A.total + 255) / 256));
  unsigned long long* sums = d_grad_tex ? reinterpret_cast<unsigned long long*>(d_workspace) : nullptr;
  tx_dispatch(tex_kind, n_channels, [&](auto c, auto* type) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(type)>>;
    BODYFIT_LAUNCH((k_txm_grad<decltype(c)::value, T>), grid, dim3(256), 0, st, A, M, static_cast<const T*>(d_tex), d_grad_image,
                   r->scratch_word(), B, pyramid, d_grad_uv, sums);
  });
  if (d_grad_tex)
    BODYFIT_LAUNCH(k_txm_fold, dim3((unsigned)((n_tex + 255) / 256)), dim3(256), 0, st, sums, M, n_channels, pyramid, n_tex,
                   r->scratch_word(), B, d_grad_tex);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
