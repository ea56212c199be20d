// Vertex attributes over a render, and images read where the points of a cloud project (bodyfit_raster_shade_device,
// bodyfit_raster_sample_device; include/bodyfit.h: the definitions, the contracts and the derivation of their constants).
//
//   k_rs_shade<C>  one thread per pixel of a render: per-vertex attributes interpolated with the perspective-correct weights
//                (lambda_a / Z_a) / sum, the background where the pixel is void (bodyfit_raster_shade_device)
//   k_rs_sample<C, T>  one thread per (frame, point): the point's projection, the bilinear value of a u8 or f32 image there and
//                the derivative of the cell's patch (bodyfit_raster_sample_device; the patch is bilinear_inl.h's, shared with
//                k_texture.hip)
//
// Arithmetic.  f64 and unfused (no contraction), in the order include/bodyfit.h counts; only the stores round to f32.  No MFMA,
// no atomics.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/bodyfit.h"
#include "bilinear_inl.h"
#include "bodyfit_device.h"
#include "raster_handle.h"

#pragma clang fp contract(off)

using namespace bodyfit;

namespace {

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

}  // namespace

extern "C" {

int bodyfit_raster_shade_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                long long verts_frame_stride, const float* d_attr, long long attr_frame_stride, int n_channels,
                                int n_frames, const float* background, float* d_image, float* d_weight, void* stream) {
  const char* fn = "bodyfit_raster_shade_device";
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_face || !d_bary || !d_image) return invalid_arg(fn, "d_face, d_bary or d_image is NULL");
  if (r->nF > 0 && (!d_verts || !d_attr)) return invalid_arg(fn, "d_verts or d_attr is NULL");
  if (int rc = rs_check_verts_stride(fn, r, verts_frame_stride)) return rc;
  if (attr_frame_stride != 0 && attr_frame_stride < (long long)n_channels * r->nV)
    return invalid_arg(fn, "a non-zero attr_frame_stride below n_channels n_verts");
  if (int rc = rs_check_pixels(fn, r, n_frames)) return rc;
  const long long ppf = (long long)r->W * r->H, total = ppf * n_frames;
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float4 bg = background ? make_float4(background[0], background[1], background[2], background[3])
                               : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const dim3 grid((unsigned)((total + 255) / 256));
  rs_dispatch_channels(n_channels, [&](auto c) {
    BODYFIT_LAUNCH(k_rs_shade<decltype(c)::value>, grid, dim3(256), 0, st, d_face, d_bary, d_verts, verts_frame_stride, d_attr,
                   attr_frame_stride, r->d_faces, r->nF, ppf, total, bg, d_image, d_weight);
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_raster_sample_device(bodyfit_raster* r, const float* d_points, long long points_frame_stride,
                                 long long n_points, int n_frames, double fx, double fy, double cx, double cy, float z_near,
                                 const void* d_image, int image_kind, int n_channels, long long image_frame_stride,
                                 const uint8_t* d_gate, float* d_value, uint8_t* d_valid, float* d_grad, void* stream) {
  const char* fn = "bodyfit_raster_sample_device";
  if (!r) return invalid_arg(fn, "handle is NULL");
  if (n_frames < 0 || n_points < 0) return invalid_arg(fn, "negative n_frames or n_points");
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (image_kind != 0 && image_kind != 1) return invalid_arg(fn, "image_kind must be 0 (u8) or 1 (f32)");
  if (!(z_near > 0.0f)) return invalid_arg(fn, "z_near must be positive");
  if (int rc = rs_check_intrinsics(fn, fx, fy, cx, cy)) return rc;
  if (n_frames == 0 || n_points == 0) return BODYFIT_OK;
  if (!d_points || !d_image || !d_value || !d_valid) return invalid_arg(fn, "d_points, d_image, d_value or d_valid is NULL");
  if (points_frame_stride < 3 * n_points) return invalid_arg(fn, "points_frame_stride below 3 n_points");
  if (image_frame_stride < (long long)r->W * r->H * n_channels) return invalid_arg(fn, "image_frame_stride below H W n_channels");
  if (n_points >= (1ll << 39) / n_frames) return invalid_arg(fn, "2^39 points or more in one call");
  const long long total = n_points * n_frames;
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((total + 255) / 256));
  rs_dispatch_channels(n_channels, [&](auto c) {
    auto launch = [&](auto kernel, auto* image) {
      BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_points, points_frame_stride, n_points, total, fx, fy, cx, cy, z_near, image,
                     image_frame_stride, r->W, r->H, d_gate, d_value, d_valid, d_grad);
    };
    if (image_kind == 0) launch(k_rs_sample<decltype(c)::value, uint8_t>, static_cast<const uint8_t*>(d_image));
    else launch(k_rs_sample<decltype(c)::value, float>, static_cast<const float*>(d_image));
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
