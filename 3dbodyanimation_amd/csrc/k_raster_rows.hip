// The depth rows and the interpolation rows of a render (bodyfit_raster_depth_rows_device, bodyfit_raster_interp_rows_device,
// bodyfit_raster_interp_rows_indexed_device; include/bodyfit.h: the definitions, the contracts and the derivation of their
// constants).
//
//   k_rs_depth_rows one thread per depth row (a pixel of a frame): the ray through the pixel against the plane of the face the
//                face-id image holds there: z, the object-space barycentrics and the direction m with dz/dcorner_a = beta_a m
//                (bodyfit_raster_depth_rows_device), f64 throughout, plain stores
//   k_rs_interp_rows<C, kIndexed> one thread per interpolation row: the depth row's face, ray and beta, and the one direction dir
//                with dL/dcorner_c = beta_c dir for upstream gradients in the interpolated attributes and in z
//                (bodyfit_raster_interp_rows_device; kIndexed: the attribute rows of a face from a table of their own, a uv atlas:
//                bodyfit_raster_interp_rows_indexed_device), f64 throughout, plain stores
//
// Arithmetic.  Everything that decides is f64, from the corners' differences; products are formed separately and added or
// subtracted (no contraction), in the order include/bodyfit.h counts.  Only the stores round to f32.  No MFMA, no atomics.
//
// The two kernels share their first 70 lines (the row's frame and pixel, the corner gather with its finiteness test, n, d, D, z,
// beta and m) as TEXT, not as a function.  Three forms of one __forceinline__ ray-face function were compiled against this text
// (two straight-line helpers around the callers' `ok`; one function that runs the rest of the row as a continuation; either with the
// row locator inside or outside): each kept every kernel's length within two instructions, and none gave the same instruction
// stream in any of the ten kernels (other registers, commuted operands, another schedule), because a helper is simplified on its own
// before it is inlined.  Without that identity the fold needs timings that say nothing at this size, so the text stays in both places:
// a change to one kernel's first half is a change to the other's.
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

// One thread per depth row: the pixel's ray against the plane of the face the face-id image holds there.  A gather of 36
// bytes of corners per row; every operation that decides is f64 and unfused (this file's contract(off)), in the order that
// include/bodyfit.h counts and tests/depth_rows_ref.py restates: e1, e2, n = e1 x e2, d, D = n . d, N0 = n . v0, z = N0 / D,
// x = z d, beta_a = (n . ((v_b - x) x (v_c - x))) / (n . n), m = n / D.  Only the stores round to f32.
// (Down to m the text is k_rs_interp_rows': see the heading.)
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
// bits; the same text down to m: see the heading), then the ONE direction that carries dL/dz and dL/dimage to the three corners,
// dL/dv_c = beta_c dir (include/bodyfit.h, INTERPOLATION ROWS).  f64 and unfused, in the order the header counts and
// tests/interp_ref.py restates:
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

// what the three entries check alike: before their own arguments, and (rows_check_buffers) once there are rows to write
int rows_check_args(const char* fn, const bodyfit_raster* r, int n_frames, long long n_rows, double fx, double fy, double cx,
                    double cy) {
  if (!r) return invalid_arg(fn, "handle is NULL");
  if (n_frames < 0 || n_rows < 0) return invalid_arg(fn, "negative n_frames or n_rows");
  return rs_check_intrinsics(fn, fx, fy, cx, cy);
}

int rows_check_buffers(const char* fn, const bodyfit_raster* r, const int32_t* d_face_image, const int32_t* d_index,
                       const float* d_verts, long long verts_frame_stride) {
  if (!d_face_image || !d_index) return invalid_arg(fn, "d_face_image or d_index is NULL");
  if (r->nF > 0 && !d_verts) return invalid_arg(fn, "d_verts is NULL");
  return rs_check_verts_stride(fn, r, verts_frame_stride);
}

// the two interpolation-row entries: one validation, one launch (indexed: attr rows by d_attr_faces, else by the corners' ids)
int rs_interp_rows(const char* fn, bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                   double fy, double cx, double cy, const int32_t* d_face_image, const int32_t* d_pixel, const int32_t* d_offset,
                   long long n_rows, const float* d_attr, long long attr_frame_stride, int n_channels, bool indexed,
                   const int32_t* d_attr_faces, int n_attr_rows, const float* d_grad_image, const float* d_grad_z, int32_t* d_index,
                   float* d_bary, float* d_dir, float* d_value, void* stream) {
  if (int rc = rows_check_args(fn, r, n_frames, n_rows, fx, fy, cx, cy)) return rc;
  if (n_channels < 0 || n_channels > 4) return invalid_arg(fn, "n_channels outside 0 .. 4");
  if (indexed && n_attr_rows < 0) return invalid_arg(fn, "negative n_attr_rows");
  if (int rc = rs_check_row_set(fn, r, n_frames, d_pixel, d_offset, n_rows)) return rc;
  if (n_frames == 0 || n_rows == 0) return BODYFIT_OK;
  if (int rc = rows_check_buffers(fn, r, d_face_image, d_index, d_verts, verts_frame_stride)) return rc;
  if (n_channels > 0 && (!d_attr || !d_grad_image)) return invalid_arg(fn, "d_attr or d_grad_image is NULL with n_channels > 0");
  if (n_channels > 0 && attr_frame_stride != 0 && attr_frame_stride < (long long)n_channels * n_attr_rows)
    return invalid_arg(fn, indexed ? "a non-zero attr_frame_stride below n_channels n_attr_rows"
                                   : "a non-zero attr_frame_stride below n_channels n_verts");
  if (indexed && n_channels > 0 && r->nF > 0 && !d_attr_faces) return invalid_arg(fn, "d_attr_faces is NULL");
  if (n_channels == 0 && !d_grad_z) return invalid_arg(fn, "n_channels == 0 needs d_grad_z");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n_rows + 255) / 256));
  auto launch = [&](auto kernel) {
    BODYFIT_LAUNCH(kernel, grid, dim3(256), 0, st, d_verts, verts_frame_stride, r->d_faces, r->nF, n_frames, r->W, r->H, fx, fy,
                   cx, cy, d_face_image, d_pixel, d_offset, n_rows / n_frames, n_rows, d_attr, attr_frame_stride, d_grad_image,
                   d_grad_z, d_index, d_bary, d_dir, d_value, d_attr_faces, n_attr_rows);
  };
  // (the un-indexed entry launches what it always has; C = 0 reads no attributes: one instantiation serves both)
  if (n_channels == 0) launch(k_rs_interp_rows<0, false>);
  else
    rs_dispatch_channels(n_channels, [&](auto c) {
      if (indexed) launch(k_rs_interp_rows<decltype(c)::value, true>);
      else launch(k_rs_interp_rows<decltype(c)::value, false>);
    });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // namespace

extern "C" {

int bodyfit_raster_depth_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                     double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                     const int32_t* d_pixel, const int32_t* d_offset, long long n_rows, int32_t* d_index,
                                     float* d_z, float* d_bary, float* d_dir, void* stream) {
  const char* fn = "bodyfit_raster_depth_rows_device";
  if (int rc = rows_check_args(fn, r, n_frames, n_rows, fx, fy, cx, cy)) return rc;
  if (int rc = rs_check_row_set(fn, r, n_frames, d_pixel, d_offset, n_rows)) return rc;
  if (n_frames == 0 || n_rows == 0) return BODYFIT_OK;
  if (int rc = rows_check_buffers(fn, r, d_face_image, d_index, d_verts, verts_frame_stride)) return rc;
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

}  // extern "C"
