// Lighting: second-order spherical-harmonic shading of a render, its gradients, and the adjoint of the vertex normals
// (bodyfit_raster_light_device, bodyfit_raster_light_grad_device, bodyfit_light_grad_layout,
// bodyfit_surface_vertex_normals_vjp_device; include/bodyfit.h: the definitions, the contracts and the derivation of their
// constants).
//
//   k_lt_forward<C>  one thread per pixel, neighbouring lanes on neighbouring columns: the shade's weights (the same operations in
//                the same order as k_rs_shade), the interpolated normal m of the face's three vertex normals, n = m / |m|, the nine
//                polynomials b_k(n), s_c = sum_k light[k][c] b_k, image_c = albedo_c s_c.  An unlit pixel passes its albedo through.
//                A workgroup never straddles two frames, so the frame's 9 C light coefficients sit at wave-uniform addresses: the
//                compiler reads them through scalar loads into SGPRs, no lane gathers them.  Plain stores.
//   k_lt_grad<C>  a workgroup owns one CHUNK of one frame, 256 P consecutive pixels (P a power of two that depends on H W only:
//                lt_layout), thread j the pixels chunk + i 256 + j, i ascending.  Per pixel the forward's pixel again, then
//                G_c s_c, the gradient in m, and (when asked) the 9 C products G_c albedo_c b_k added to a per-lane f64
//                accumulator whose indices are all compile-time (registers, no scratch).  The lanes meet in a butterfly of
//                shuffles (the same tree for every lane), the four waves in LDS in ascending order, and the chunk's [9][C] f64
//                partial is STORED.  No atomics of any kind.
//   k_lt_light_sum  one thread per (frame, k, c): the frame's partials added in ascending chunk order in f64, rounded once.
//   k_vn_h       one thread per (frame, vertex): the forward's sum s_i by the forward's arithmetic, h_i = (g_i - n_i (n_i . g_i)) /
//                |s_i| in f64 into the handle's workspace
//   k_vn_vjp     one thread per (frame, vertex): over the vertex's entries of the vertex -> corner table in ascending order,
//                (v_{a+1} - v_{a+2}) x (h_i0 + h_i1 + h_i2) in f64, rounded once.  A gather: no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "raster_handle.h"
#include "surface_handle.h"

#pragma clang fp contract(off)

namespace bodyfit {

namespace {

struct LtArgs {
  const int* face_img;       // [F][H][W]
  const float* bary;         // [F][H][W][3]
  const float* verts;        // [F] stride verts_stride, [n_verts][3]
  long long verts_stride;
  const float* normals;      // [F] stride normals_stride, [n_verts][3]
  long long normals_stride;
  const int* faces;          // [nF][3]
  int nF;
  const float* albedo;       // [F][H][W][C]
  const float* light;        // [9][C], light_stride floats between frames (0: shared)
  long long light_stride;
  long long ppf;             // pixels per frame
  int P;                     // pixels per thread of a chunk (the forward: 1)
  long long chunks;          // chunks per frame
};

// One pixel: lit or not, the unit normal and the length of the interpolated one.  Everything f64 and unfused.
struct LtPixel {
  bool lit;
  double n[3], l;
};

__device__ __forceinline__ LtPixel lt_pixel(const LtArgs& A, size_t frame, long long o) {
  LtPixel p;
  p.lit = false;
  p.n[0] = p.n[1] = p.n[2] = 0.0; p.l = 0.0;
  const int t = A.face_img[o];
  const float l0 = A.bary[3 * (size_t)o], l1 = A.bary[3 * (size_t)o + 1], l2 = A.bary[3 * (size_t)o + 2];
  // (a NaN fails every comparison; x - x is NaN for an infinity)
  bool ok = (unsigned)t < (unsigned)A.nF && l0 - l0 == 0.0f && l1 - l1 == 0.0f && l2 - l2 == 0.0f && l0 >= 0.0f && l1 >= 0.0f &&
            l2 >= 0.0f;
  if (!ok) return p;
  const float* v = A.verts + frame * (size_t)A.verts_stride;
  const float* nr = A.normals + frame * (size_t)A.normals_stride;
  const size_t i0 = (size_t)A.faces[3 * t], i1 = (size_t)A.faces[3 * t + 1], i2 = (size_t)A.faces[3 * t + 2];
  const float Z0 = v[3 * i0 + 2], Z1 = v[3 * i1 + 2], Z2 = v[3 * i2 + 2];
  float a0[3], a1[3], a2[3];
  for (int k = 0; k < 3; ++k) { a0[k] = nr[3 * i0 + k]; a1[k] = nr[3 * i1 + k]; a2[k] = nr[3 * i2 + k]; }
  ok = Z0 - Z0 == 0.0f && Z1 - Z1 == 0.0f && Z2 - Z2 == 0.0f && Z0 > 0.0f && Z1 > 0.0f && Z2 > 0.0f;
  if (!ok) return p;
  const double q0 = (double)l0 / (double)Z0, q1 = (double)l1 / (double)Z1, q2 = (double)l2 / (double)Z2;
  const double S = (q0 + q1) + q2;
  if (!(S != 0.0)) return p;
  for (int k = 0; k < 3; ++k)
    if (!(a0[k] - a0[k] == 0.0f) || !(a1[k] - a1[k] == 0.0f) || !(a2[k] - a2[k] == 0.0f)) return p;
  const double w0 = q0 / S, w1 = q1 / S, w2 = q2 / S;
  double m[3];
  for (int k = 0; k < 3; ++k) m[k] = (w0 * (double)a0[k] + w1 * (double)a1[k]) + w2 * (double)a2[k];
  const double l = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  if (!(l - l == 0.0) || !(l != 0.0)) return p;      // the three normals cancel, or their squares overflow
  for (int k = 0; k < 3; ++k) p.n[k] = m[k] / l;
  p.l = l;
  p.lit = true;
  return p;
}

// b(n) = (1, x, y, z, xy, xz, yz, x^2 - y^2, 3 z^2 - 1)
__device__ __forceinline__ void lt_basis(const double n[3], double b[9]) {
  const double x = n[0], y = n[1], z = n[2];
  b[0] = 1.0; b[1] = x; b[2] = y; b[3] = z;
  b[4] = x * y; b[5] = x * z; b[6] = y * z;
  b[7] = x * x - y * y;
  b[8] = 3.0 * (z * z) - 1.0;
}

// the frame's light at wave-uniform addresses
template <int C>
__device__ __forceinline__ void lt_light(const LtArgs& A, size_t frame, double L[9][C]) {
  const float* __restrict__ src = A.light + frame * (size_t)A.light_stride;
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int c = 0; c < C; ++c) L[k][c] = (double)src[k * C + c];
}

template <int C>
__device__ __forceinline__ void lt_shading(const double L[9][C], const double b[9], double s[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double acc = L[0][c] * b[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) acc = acc + L[k][c] * b[k];
    s[c] = acc;
  }
}

template <int C>
__global__ __launch_bounds__(256) void k_lt_forward(const LtArgs A, float* __restrict__ image, float* __restrict__ normal,
                                                    float* __restrict__ shading) {
  const size_t frame = (size_t)(blockIdx.x / A.chunks);             // (wave-uniform)
  const long long in_frame = (long long)(blockIdx.x - frame * A.chunks) * 256 + threadIdx.x;
  if (in_frame >= A.ppf) return;
  const long long o = (long long)frame * A.ppf + in_frame;
  double L[9][C];
  lt_light<C>(A, frame, L);
  const LtPixel p = lt_pixel(A, frame, o);
  float out[C], sh[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { out[c] = A.albedo[C * (size_t)o + c]; sh[c] = 0.0f; }
  if (p.lit) {
    double b[9], s[C];
    lt_basis(p.n, b);
    lt_shading<C>(L, b, s);
#pragma unroll
    for (int c = 0; c < C; ++c) { out[c] = (float)((double)out[c] * s[c]); sh[c] = (float)s[c]; }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) image[C * (size_t)o + c] = out[c];
  if (normal)
    for (int k = 0; k < 3; ++k) normal[3 * (size_t)o + k] = (float)p.n[k];
  if (shading)
#pragma unroll
    for (int c = 0; c < C; ++c) shading[C * (size_t)o + c] = sh[c];
}

template <int C>
__global__ __launch_bounds__(256) void k_lt_grad(const LtArgs A, const float* __restrict__ grad_image, float* __restrict__ grad_albedo,
                                                 float* __restrict__ grad_m, double* __restrict__ partial) {
  __shared__ double s_part[4][9 * C];
  const size_t frame = (size_t)(blockIdx.x / A.chunks);             // (wave-uniform)
  const long long chunk = (long long)(blockIdx.x - frame * A.chunks);
  const long long first = chunk * 256 * A.P + threadIdx.x;
  double L[9][C];
  lt_light<C>(A, frame, L);
  double acc[9][C];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[k][c] = 0.0;
  for (int i = 0; i < A.P; ++i) {
    const long long in_frame = first + (long long)i * 256;
    if (in_frame >= A.ppf) break;
    const long long o = (long long)frame * A.ppf + in_frame;
    const LtPixel p = lt_pixel(A, frame, o);
    double G[C], ga[C], gm[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < C; ++c) { G[c] = (double)grad_image[C * (size_t)o + c]; ga[c] = G[c]; }
    if (p.lit) {
      double b[9], s[C], t[C];
      lt_basis(p.n, b);
      lt_shading<C>(L, b, s);
#pragma unroll
      for (int c = 0; c < C; ++c) { ga[c] = G[c] * s[c]; t[c] = G[c] * (double)A.albedo[C * (size_t)o + c]; }
      if (partial) {
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
          for (int c = 0; c < C; ++c) acc[k][c] += t[c] * b[k];
      }
      if (grad_m) {
        double q[9];      // q_k = sum_c t_c light[k][c], ascending c (q_0 is not needed: b_0 is constant)
#pragma unroll
        for (int k = 1; k < 9; ++k) {
          double a = t[0] * L[k][0];
#pragma unroll
          for (int c = 1; c < C; ++c) a = a + t[c] * L[k][c];
          q[k] = a;
        }
        const double x = p.n[0], y = p.n[1], z = p.n[2];
        const double gx = ((q[1] + y * q[4]) + z * q[5]) + (2.0 * x) * q[7];
        const double gy = ((q[2] + x * q[4]) + z * q[6]) - (2.0 * y) * q[7];
        const double gz = ((q[3] + x * q[5]) + y * q[6]) + (6.0 * z) * q[8];
        const double d = (x * gx + y * gy) + z * gz;
        gm[0] = (gx - x * d) / p.l; gm[1] = (gy - y * d) / p.l; gm[2] = (gz - z * d) / p.l;
      }
    }
    if (grad_albedo)
#pragma unroll
      for (int c = 0; c < C; ++c) grad_albedo[C * (size_t)o + c] = (float)ga[c];
    if (grad_m)
      for (int k = 0; k < 3; ++k) grad_m[3 * (size_t)o + k] = (float)gm[k];
  }
  if (!partial) return;                                             // (uniform over the grid)
  // the lanes of a wave: a butterfly, every lane adds the same tree; then the waves in ascending order
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double a = acc[k][c];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) a = a + __shfl_xor(a, d, 64);
      acc[k][c] = a;
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int c = 0; c < C; ++c) s_part[wave][k * C + c] = acc[k][c];
  }
  __syncthreads();
  if (threadIdx.x < 9 * C) {
    const int j = threadIdx.x;
    partial[((size_t)frame * (size_t)A.chunks + (size_t)chunk) * (9 * C) + j] =
        ((s_part[0][j] + s_part[1][j]) + s_part[2][j]) + s_part[3][j];
  }
}

// the frames' partials [F][chunks][n] f64 -> [F][n] f32, n = 9 C
__global__ __launch_bounds__(64) void k_lt_light_sum(const double* __restrict__ partial, long long chunks, int n,
                                                     float* __restrict__ grad_light) {
  const int j = threadIdx.x;
  const size_t frame = blockIdx.x;
  if (j >= n) return;
  const double* p = partial + frame * (size_t)chunks * n + j;
  double a = p[0];
#pragma unroll 8
  for (long long ch = 1; ch < chunks; ++ch) a = a + p[(size_t)ch * n];     // (unrolled: eight loads in flight, the additions in order)
  grad_light[frame * (size_t)n + j] = (float)a;
}

// the chunks of a frame of ppf pixels: 256 P pixels each, P the smallest power of two that leaves at most 256 chunks, at most 64
void lt_layout(long long ppf, long long* P, long long* chunks) {
  long long p = 1;
  while (p < 64 && (ppf + 256 * p - 1) / (256 * p) > 256) p *= 2;
  *P = p;
  *chunks = ppf > 0 ? (ppf + 256 * p - 1) / (256 * p) : 0;
}

// what the two entries check alike; *work: there are pixels to write
int lt_check(const char* fn, const bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
             long long verts_frame_stride, const float* d_normals, long long normals_frame_stride, const float* d_albedo,
             int n_channels, const float* d_light, long long light_frame_stride, int n_frames, bool* work) {
  *work = false;
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  if (light_frame_stride != 0 && light_frame_stride < 9ll * n_channels)
    return invalid_arg(fn, "a non-zero light_frame_stride below 9 n_channels");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_face || !d_bary || !d_albedo || !d_light) return invalid_arg(fn, "d_face, d_bary, d_albedo or d_light is NULL");
  if (r->nF > 0 && (!d_verts || !d_normals)) return invalid_arg(fn, "d_verts or d_normals is NULL");
  if (int rc = rs_check_verts_stride(fn, r, verts_frame_stride)) return rc;
  if (normals_frame_stride < 3ll * r->nV) return invalid_arg(fn, "normals_frame_stride below 3 n_verts");
  if (int rc = rs_check_pixels(fn, r, n_frames)) return rc;
  *work = true;
  return BODYFIT_OK;
}

LtArgs lt_args(const bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts, long long verts_frame_stride,
               const float* d_normals, long long normals_frame_stride, const float* d_albedo, const float* d_light,
               long long light_frame_stride) {
  LtArgs A;
  A.face_img = d_face; A.bary = d_bary; A.verts = d_verts; A.verts_stride = verts_frame_stride;
  A.normals = d_normals; A.normals_stride = normals_frame_stride; A.faces = r->d_faces; A.nF = r->nF;
  A.albedo = d_albedo; A.light = d_light; A.light_stride = light_frame_stride;
  A.ppf = (long long)r->W * r->H; A.P = 1; A.chunks = (A.ppf + 255) / 256;
  return A;
}

struct NormalVjpArgs {
  const float* verts;
  long long vstride;
  const int* faces;
  const int *csr_off, *csr_fc;
  int n_verts, F;
  const float* grad_normals;   // [F][n_verts][3]
  double* h;                   // [F][n_verts][3]
  float* grad_verts;
  long long gstride;
};

// h_i from the forward's sum (k_winding.hip's k_vertex_normals: the same faces in the same order by the same operations)
__global__ __launch_bounds__(256) void k_vn_h(const NormalVjpArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.F * a.n_verts) return;
  const int f = (int)(row / a.n_verts), v = (int)(row - (long long)f * a.n_verts);
  const float* vb = a.verts + (size_t)f * (size_t)a.vstride;
  double sx = 0., sy = 0., sz = 0.;
  for (int k = a.csr_off[v]; k < a.csr_off[v + 1]; ++k) {
    const int fc = a.csr_fc[k], t = fc / 3, corner = fc - 3 * t;
    const int* id = a.faces + 3 * (size_t)t;
    const int i0 = id[0], i1 = id[1], i2 = id[2];
    if ((corner == 1 && i0 == v) || (corner == 2 && (i0 == v || i1 == v))) continue;   // the face was taken at an earlier corner
    const float* v0 = vb + 3 * (size_t)i0;
    const float* v1 = vb + 3 * (size_t)i1;
    const float* v2 = vb + 3 * (size_t)i2;
    const double e1x = (double)v1[0] - (double)v0[0], e1y = (double)v1[1] - (double)v0[1], e1z = (double)v1[2] - (double)v0[2];
    const double e2x = (double)v2[0] - (double)v0[0], e2y = (double)v2[1] - (double)v0[1], e2z = (double)v2[2] - (double)v0[2];
    sx += e1y * e2z - e1z * e2y;
    sy += e1z * e2x - e1x * e2z;
    sz += e1x * e2y - e1y * e2x;
  }
  const double l = sqrt(sx * sx + sy * sy + sz * sz);
  const bool ok = isfinite(l) && l > 0.;
  double hx = 0., hy = 0., hz = 0.;
  if (ok) {
    const double nx = sx / l, ny = sy / l, nz = sz / l;
    const float* g = a.grad_normals + 3 * (size_t)row;
    const double gx = (double)g[0], gy = (double)g[1], gz = (double)g[2];
    const double d = (nx * gx + ny * gy) + nz * gz;
    hx = (gx - nx * d) / l; hy = (gy - ny * d) / l; hz = (gz - nz * d) / l;
  }
  double* h = a.h + 3 * (size_t)row;
  h[0] = hx; h[1] = hy; h[2] = hz;
}

__global__ __launch_bounds__(256) void k_vn_vjp(const NormalVjpArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.F * a.n_verts) return;
  const int f = (int)(row / a.n_verts), v = (int)(row - (long long)f * a.n_verts);
  const float* vb = a.verts + (size_t)f * (size_t)a.vstride;
  const double* hb = a.h + 3 * (size_t)f * (size_t)a.n_verts;
  double gx = 0., gy = 0., gz = 0.;
  for (int k = a.csr_off[v]; k < a.csr_off[v + 1]; ++k) {
    const int fc = a.csr_fc[k], t = fc / 3, corner = fc - 3 * t;
    const int* id = a.faces + 3 * (size_t)t;
    const int i0 = id[0], i1 = id[1], i2 = id[2];
    if (i0 == i1 || i1 == i2 || i0 == i2) continue;                 // N_t is identically 0
    const double* h0 = hb + 3 * (size_t)i0;
    const double* h1 = hb + 3 * (size_t)i1;
    const double* h2 = hb + 3 * (size_t)i2;
    const double ax = (h0[0] + h1[0]) + h2[0], ay = (h0[1] + h1[1]) + h2[1], az = (h0[2] + h1[2]) + h2[2];
    if (ax == 0. && ay == 0. && az == 0.) continue;                 // (nothing to carry: a non-finite corner stays out of it)
    const int ip = corner == 0 ? i1 : (corner == 1 ? i2 : i0), iq = corner == 0 ? i2 : (corner == 1 ? i0 : i1);
    const float* vp = vb + 3 * (size_t)ip;
    const float* vq = vb + 3 * (size_t)iq;
    const double ex = (double)vp[0] - (double)vq[0], ey = (double)vp[1] - (double)vq[1], ez = (double)vp[2] - (double)vq[2];
    gx += ey * az - ez * ay;
    gy += ez * ax - ex * az;
    gz += ex * ay - ey * ax;
  }
  float* out = a.grad_verts + (size_t)f * (size_t)a.gstride + 3 * (size_t)v;
  out[0] = (float)gx; out[1] = (float)gy; out[2] = (float)gz;
}

}  // namespace

}  // namespace bodyfit

extern "C" {

int bodyfit_raster_light_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                long long verts_frame_stride, const float* d_normals, long long normals_frame_stride,
                                const float* d_albedo, int n_channels, const float* d_light, long long light_frame_stride,
                                int n_frames, float* d_image, float* d_normal, float* d_shading, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_raster_light_device";
  bool work = false;
  if (int rc = lt_check(fn, r, d_face, d_bary, d_verts, verts_frame_stride, d_normals, normals_frame_stride, d_albedo, n_channels,
                        d_light, light_frame_stride, n_frames, &work))
    return rc;
  if (!work) return BODYFIT_OK;
  if (!d_image) return invalid_arg(fn, "d_image is NULL");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LtArgs A = lt_args(r, d_face, d_bary, d_verts, verts_frame_stride, d_normals, normals_frame_stride, d_albedo, d_light,
                           light_frame_stride);
  const dim3 grid((unsigned)(A.chunks * n_frames));
  rs_dispatch_channels(n_channels, [&](auto c) {
    BODYFIT_LAUNCH((k_lt_forward<decltype(c)::value>), grid, dim3(256), 0, st, A, d_image, d_normal, d_shading);
  });
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_light_grad_layout(long long pixels_per_frame, int n_channels, int n_frames, long long* chunk_pixels,
                              long long* n_chunks, long long* workspace_doubles) {
  using namespace bodyfit;
  const char* fn = "bodyfit_light_grad_layout";
  if (pixels_per_frame < 0 || n_frames < 0) return invalid_arg(fn, "a negative count");
  if (int rc = rs_check_channels(fn, n_channels)) return rc;
  long long P = 1, chunks = 0;
  lt_layout(pixels_per_frame, &P, &chunks);
  if (chunk_pixels) *chunk_pixels = 256 * P;
  if (n_chunks) *n_chunks = chunks;
  if (workspace_doubles) *workspace_doubles = chunks * 9 * n_channels * n_frames;
  return BODYFIT_OK;
}

int bodyfit_raster_light_grad_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                     long long verts_frame_stride, const float* d_normals, long long normals_frame_stride,
                                     const float* d_albedo, int n_channels, const float* d_light, long long light_frame_stride,
                                     int n_frames, const float* d_grad_image, float* d_grad_albedo, float* d_grad_m,
                                     float* d_grad_light, double* d_workspace, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_raster_light_grad_device";
  bool work = false;
  if (int rc = lt_check(fn, r, d_face, d_bary, d_verts, verts_frame_stride, d_normals, normals_frame_stride, d_albedo, n_channels,
                        d_light, light_frame_stride, n_frames, &work))
    return rc;
  if (!work || (!d_grad_albedo && !d_grad_m && !d_grad_light)) return BODYFIT_OK;
  if (!d_grad_image) return invalid_arg(fn, "d_grad_image is NULL");
  if (d_grad_light && !d_workspace) return invalid_arg(fn, "d_grad_light without d_workspace");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  LtArgs A = lt_args(r, d_face, d_bary, d_verts, verts_frame_stride, d_normals, normals_frame_stride, d_albedo, d_light,
                     light_frame_stride);
  long long P = 1;
  lt_layout(A.ppf, &P, &A.chunks);
  A.P = (int)P;
  double* partial = d_grad_light ? d_workspace : nullptr;
  const dim3 grid((unsigned)(A.chunks * n_frames));
  rs_dispatch_channels(n_channels, [&](auto c) {
    BODYFIT_LAUNCH((k_lt_grad<decltype(c)::value>), grid, dim3(256), 0, st, A, d_grad_image, d_grad_albedo, d_grad_m, partial);
  });
  if (d_grad_light)
    BODYFIT_LAUNCH(k_lt_light_sum, dim3((unsigned)n_frames), dim3(64), 0, st, partial, A.chunks, 9 * n_channels, d_grad_light);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_surface_vertex_normals_vjp_device(bodyfit_surface* s, const float* d_verts, long long verts_frame_stride, int n_frames,
                                              const float* d_grad_normals, float* d_grad_verts, long long grad_frame_stride,
                                              void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_vertex_normals_vjp_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (!s) return invalid(fn, "null handle");
  if (verts_frame_stride < 3LL * s->n_verts) return invalid(fn, "verts_frame_stride < 3 n_verts");
  if (grad_frame_stride < 3LL * s->n_verts) return invalid(fn, "grad_frame_stride < 3 n_verts");
  if ((long long)n_frames * s->n_verts >= (1LL << 31) - 4096) return invalid(fn, "more than 2^31 vertices over the frames");
  if (n_frames == 0 || s->n_verts == 0) return BODYFIT_OK;
  if (!d_verts || !d_grad_normals || !d_grad_verts) return invalid(fn, "d_verts / d_grad_normals / d_grad_verts is NULL");
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long rows = (long long)n_frames * s->n_verts;
  if (int rc = reserve(&s->acc, &s->acc_bytes, (size_t)rows * 24)) return rc;
  NormalVjpArgs a{};
  a.verts = d_verts; a.vstride = verts_frame_stride; a.faces = s->d_faces;
  a.csr_off = s->d_csr_off; a.csr_fc = s->d_csr_fc;
  a.n_verts = s->n_verts; a.F = n_frames;
  a.grad_normals = d_grad_normals; a.h = reinterpret_cast<double*>(s->acc);
  a.grad_verts = d_grad_verts; a.gstride = grad_frame_stride;
  const dim3 grid((unsigned)((rows + 255) / 256));
  BODYFIT_LAUNCH(k_vn_h, grid, dim3(256), 0, st, a);
  BODYFIT_LAUNCH(k_vn_vjp, grid, dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
