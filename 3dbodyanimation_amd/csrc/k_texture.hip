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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/bodyfit.h"
#include "bilinear_inl.h"
#include "bodyfit_device.h"
#include "host_state.h"
#include "raster_view.h"
#include "solver_view.h"

#pragma clang fp contract(off)

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

int tx_invalid(const char* fn, const char* what) {
  return bodyfit_internal_fail(BODYFIT_ERR_INVALID, (std::string(fn) + ": " + what).c_str());
}

// what the two entries check alike; *work: there are pixels to write
int tx_check(const char* fn, const bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
             long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces, int tex_kind, int n_channels,
             int tex_height, int tex_width, long long tex_frame_stride, int n_frames, bool* work) {
  *work = false;
  if (!r) return tx_invalid(fn, "handle is NULL");
  if (n_frames < 0) return tx_invalid(fn, "negative n_frames");
  if (n_channels < 1 || n_channels > 4) return tx_invalid(fn, "n_channels outside 1 .. 4");
  if (tex_kind != 0 && tex_kind != 1) return tx_invalid(fn, "tex_kind must be 0 (u8) or 1 (f32)");
  if (tex_height < 1 || tex_width < 1 || tex_height > 16384 || tex_width > 16384)
    return tx_invalid(fn, "texture size outside 1 .. 16384");
  if (n_uv < 0) return tx_invalid(fn, "negative n_uv");
  if (tex_frame_stride != 0 && tex_frame_stride < (long long)tex_height * tex_width * n_channels)
    return tx_invalid(fn, "a non-zero tex_frame_stride below Ht Wt n_channels");
  if (n_frames == 0) return BODYFIT_OK;
  const bodyfit::RasterView V = bodyfit::raster_view(r);
  if (!d_face || !d_bary) return tx_invalid(fn, "d_face or d_bary is NULL");
  if (V.nF > 0 && (!d_verts || !d_uv_faces)) return tx_invalid(fn, "d_verts or d_uv_faces is NULL");
  if (V.nF > 0 && n_uv > 0 && !d_uv) return tx_invalid(fn, "d_uv is NULL");
  if (verts_frame_stride < 3ll * V.nV) return tx_invalid(fn, "verts_frame_stride below 3 n_verts");
  if ((long long)V.W * V.H * n_frames >= (1ll << 39)) return tx_invalid(fn, "2^39 pixels or more in one call");
  *work = true;
  return BODYFIT_OK;
}

TxArgs tx_args(const bodyfit::RasterView& V, const int32_t* d_face, const float* d_bary, const float* d_verts,
               long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces, int tex_height, int tex_width,
               long long tex_frame_stride, int n_frames) {
  TxArgs A;
  A.face_img = d_face; A.bary = d_bary; A.verts = d_verts; A.verts_stride = verts_frame_stride; A.faces = V.d_faces;
  A.uv = d_uv; A.uv_faces = d_uv_faces; A.nF = V.nF; A.T = n_uv; A.Wt = tex_width; A.Ht = tex_height;
  A.tex_stride = tex_frame_stride; A.ppf = (long long)V.W * V.H; A.total = A.ppf * n_frames;
  return A;
}

template <typename Launch>
void tx_dispatch(int tex_kind, int C, Launch&& launch) {
#define TX_CASE(c)                                        \
  case c:                                                 \
    if (tex_kind == 0) launch(std::integral_constant<int, c>{}, (const uint8_t*)nullptr); \
    else launch(std::integral_constant<int, c>{}, (const float*)nullptr);                 \
    break;
  switch (C) {
    TX_CASE(1)
    TX_CASE(2)
    TX_CASE(3)
    default:
    TX_CASE(4)
  }
#undef TX_CASE
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
  if (!d_image) return tx_invalid(fn, "d_image is NULL");
  const bodyfit::RasterView V = bodyfit::raster_view(r);
  if (V.nF > 0 && !d_tex) return tx_invalid(fn, "d_tex is NULL");
  HIP_TRY(hipSetDevice(V.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TxArgs A = tx_args(V, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_height, tex_width,
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
  if (!d_grad_image) return tx_invalid(fn, "d_grad_image is NULL");
  if (d_grad_tex && !d_workspace) return tx_invalid(fn, "d_grad_tex without d_workspace");
  const bodyfit::RasterView V = bodyfit::raster_view(r);
  if (V.nF > 0 && d_grad_uv && !d_tex) return tx_invalid(fn, "d_grad_uv without d_tex");
  HIP_TRY(hipSetDevice(V.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TxArgs A = tx_args(V, d_face, d_bary, d_verts, verts_frame_stride, d_uv, n_uv, d_uv_faces, tex_height, tex_width,
                           tex_frame_stride, n_frames);
  int B = 0;      // the bit length of the pixel count: total < 2^B
  while ((A.total >> B) != 0) ++B;
  const long long n_tex = (long long)tex_height * tex_width * n_channels * (tex_frame_stride ? n_frames : 1);
  const long long n_grad = A.total * n_channels;
  if (d_grad_tex && n_tex >= (1ll << 39)) return tx_invalid(fn, "2^39 texel elements or more in one call");
  HIP_TRY(hipMemsetAsync(V.d_scratch, 0, sizeof(unsigned), st));
  if (d_grad_tex) HIP_TRY(hipMemsetAsync(d_workspace, 0, (size_t)n_tex * sizeof(long long), st));
  const unsigned mblocks = (unsigned)std::min<long long>((n_grad + 255) / 256, 4096);
  BODYFIT_LAUNCH(k_tx_gmax, dim3(mblocks), dim3(256), 0, st, d_grad_image, n_grad, V.d_scratch);
  const dim3 grid((unsigned)((A.total + 255) / 256));
  unsigned long long* sums = d_grad_tex ? reinterpret_cast<unsigned long long*>(d_workspace) : nullptr;
  tx_dispatch(tex_kind, n_channels, [&](auto c, auto* type) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(type)>>;
    BODYFIT_LAUNCH((k_tx_grad<decltype(c)::value, T>), grid, dim3(256), 0, st, A, static_cast<const T*>(d_tex), d_grad_image,
                   V.d_scratch, B, d_grad_uv, sums);
  });
  if (d_grad_tex)
    BODYFIT_LAUNCH(k_tx_fold, dim3((unsigned)((n_tex + 255) / 256)), dim3(256), 0, st, sums, n_tex, V.d_scratch, B, d_grad_tex);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
