// k_offsets.hip — per-vertex offsets d (SMPL+D: a displacement added to the blended rest vertex before skinning) carried through
// the forward, its VJP and its JVP, and the mesh Laplacian their regulariser needs.  Host side: bodyfit_forward_offsets*_device
// (api_problem.hip, api_vjp.hip, api_jvp.hip) and bodyfit_surface_laplacian_device (below).  Notation: k_forward_vjp.hip.
//
//   cloud_v = sum_j W_vj T_j [b_v + d_v; 1] = cloud0_v + L_fv d_v,   L_fv = sum_j W_vj T_j[:, :3]
//
//   k_offsets_apply     behind the two-launch forward: one thread per (frame, vertex), the frame's 24 x 12 transform floats (the
//                       ones the forward left in mc.skinT) staged once per workgroup, the four transforms blended as in
//                       k_vjp_vertex_grad, cloud_v += L_fv d_v in the caller's rows: 12 B of d and 12 B of cloud read, 12 B
//                       written.  A vertex whose d_v is exactly 0 is left untouched (so zero offsets give the forward's bits),
//                       the padding vertices of the last 32-vertex tile have no row in the caller's buffer and are skipped.
//   k_offsets_displace  bbuf[f][v] += d_v on the [F][Vp][3] blended rest vertices: between the VJP's stage a and stage c (so
//                       dL/dT_j sees b_v + d_v, while stage b's input gb_v = L_fv^T G_v does not depend on d), and between the
//                       JVP's primal blend and k_jvp_skin (the offsets are constant there and carry no tangent)
//   k_offsets_grad      dL/dd from the VJP's gb ([Fp][3][Vp] f32, gb_fv = L_fv^T G_fv IS frame f's dL/dd_v): per-frame offsets a
//                       transposed copy; shared offsets one thread per (vertex, component) adding the frames in ascending order
//                       in f64, rounded once.  No atomics.
//   k_mesh_laplacian    the uniform ("umbrella") Laplacian of a per-vertex field and its transpose, a gather over the vertex's
//                       faces through the surface handle's vertex -> corner table
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "host_state.h"

#include "surface_handle.h"

namespace bodyfit {

namespace {

constexpr int kSkinFloats = kMaxJoints * 12;

struct OffsetsApplyArgs {
  const float* skinT;       // [F][24][12]
  const uint32_t* wIdx;
  const float* wVal;
  const float* off;         // frame f at off + f off_stride
  long long off_stride;
  float* cloud;             // caller's [F][row_floats]
  long long row_floats;
  int V;
};

__global__ __launch_bounds__(256) void k_offsets_apply(OffsetsApplyArgs a) {
  __shared__ float T[kSkinFloats];
  const int f = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
  const float* Tf = a.skinT + (size_t)f * kSkinFloats;
  for (int e = threadIdx.x; e < kSkinFloats; e += 256) T[e] = Tf[e];
  __syncthreads();
  if (v >= a.V) return;
  const float* d = a.off + (size_t)f * (size_t)a.off_stride + (size_t)v * 3;
  const float d0 = d[0], d1 = d[1], d2 = d[2];
  if (d0 == 0.0f && d1 == 0.0f && d2 == 0.0f) return;
  const uint32_t widx = a.wIdx[v];
  const float4 wv = reinterpret_cast<const float4*>(a.wVal)[v];
  const float wgt[4] = {wv.x, wv.y, wv.z, wv.w};
  float Mx[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) Mx[e] = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* tv = T + ((widx >> (8 * i)) & 0xffu) * 12;   // (an unused slot: a valid joint with weight 0)
#pragma unroll
    for (int e = 0; e < 12; ++e) Mx[e] += wgt[i] * tv[e];
  }
  float* c = a.cloud + (size_t)f * (size_t)a.row_floats + (size_t)v * 3;
  c[0] += Mx[0] * d0 + Mx[1] * d1 + Mx[2] * d2;
  c[1] += Mx[4] * d0 + Mx[5] * d1 + Mx[6] * d2;
  c[2] += Mx[8] * d0 + Mx[9] * d1 + Mx[10] * d2;
}

// one thread per (frame, vertex); v < V only (the padding of bbuf stays as it is)
__global__ __launch_bounds__(256) void k_offsets_displace(const float* __restrict__ off, long long off_stride,
                                                          float* __restrict__ bbuf, int V, int Vp) {
  const int f = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const float* d = off + (size_t)f * (size_t)off_stride + (size_t)v * 3;
  float* b = bbuf + ((size_t)f * Vp + v) * 3;
  b[0] += d[0]; b[1] += d[1]; b[2] += d[2];
}

// per-frame offsets: grad[f][v][c] = gb[f][c][v]
__global__ __launch_bounds__(256) void k_offsets_grad_frames(const float* __restrict__ gbuf, float* __restrict__ grad,
                                                             long long off_stride, int V, int Vp) {
  const int f = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const float* g = gbuf + ((size_t)f * 3) * Vp + v;
  float* o = grad + (size_t)f * (size_t)off_stride + (size_t)v * 3;
  o[0] = g[0]; o[1] = g[(size_t)Vp]; o[2] = g[2 * (size_t)Vp];
}

// shared offsets: thread (component c, vertex v), the frames in ascending order
__global__ __launch_bounds__(256) void k_offsets_grad_shared(const float* __restrict__ gbuf, float* __restrict__ grad, int F, int V,
                                                             int Vp) {
  const int v = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (v >= V) return;
  const float* g = gbuf + (size_t)c * Vp + v;
  const size_t fs = (size_t)3 * Vp;
  double s = 0.0;
  int f = 0;
  // sixteen loads in flight per thread, added in the frames' order: V x 3 threads are a third of the chip's wave slots, so the
  // memory parallelism has to come from inside the thread
  for (; f + 16 <= F; f += 16) {
    float t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = g[(size_t)(f + i) * fs];
#pragma unroll
    for (int i = 0; i < 16; ++i) s += (double)t[i];
  }
  for (; f < F; ++f) s += (double)g[(size_t)f * fs];
  grad[(size_t)v * 3 + c] = (float)s;
}

// ---- the mesh Laplacian ---------------------------------------------------------------------------------------------------
struct LaplaceArgs {
  const float* x;           // field k at x + k stride, [n_verts][3]
  long long stride;
  const int* faces;
  const int *csr_off, *csr_fc;
  int n_verts, n_fields, transpose;
  float* out;               // [n_fields][n_verts][3]
};

// is position q the first one at which face `id` holds id[q]?
__device__ __forceinline__ bool first_position(const int* id, int q) {
  return q == 0 || (q == 1 && id[0] != id[1]) || (q == 2 && id[0] != id[2] && id[1] != id[2]);
}

// the faces that hold vertex v, each once
__device__ inline int face_count(const LaplaceArgs& a, int v) {
  int n = 0;
  for (int k = a.csr_off[v]; k < a.csr_off[v + 1]; ++k) {
    const int fc = a.csr_fc[k], t = fc / 3;
    n += first_position(a.faces + 3 * (size_t)t, fc - 3 * t) ? 1 : 0;
  }
  return n;
}

__global__ __launch_bounds__(256) void k_mesh_laplacian(const LaplaceArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.n_fields * a.n_verts) return;
  const int k = (int)(row / a.n_verts), v = (int)(row - (long long)k * a.n_verts);
  const float* x = a.x + (size_t)k * (size_t)a.stride;
  double s0 = 0., s1 = 0., s2 = 0.;
  int n = 0;
  for (int e = a.csr_off[v]; e < a.csr_off[v + 1]; ++e) {
    const int fc = a.csr_fc[e], t = fc / 3, c = fc - 3 * t;
    const int* id = a.faces + 3 * (size_t)t;
    const bool first = first_position(id, c);
    n += first ? 1 : 0;
    if (!a.transpose) {
      // row v of L: the face once, at v's first position; the other two positions
      if (!first) continue;
      const float* xa = x + 3 * (size_t)id[(c + 1) % 3];
      const float* xb = x + 3 * (size_t)id[(c + 2) % 3];
      s0 += (double)xa[0] + (double)xb[0];
      s1 += (double)xa[1] + (double)xb[1];
      s2 += (double)xa[2] + (double)xb[2];
    } else {
      // column v of L: position c is read by the row of every vertex w of the face whose first position is another one
      for (int q = 0; q < 3; ++q) {
        if (q == c || !first_position(id, q)) continue;
        const int w = id[q];
        const double cw = 1.0 / (2.0 * (double)face_count(a, w));   // (w holds this face: the count is >= 1)
        const float* xw = x + 3 * (size_t)w;
        s0 += cw * (double)xw[0]; s1 += cw * (double)xw[1]; s2 += cw * (double)xw[2];
      }
    }
  }
  float* o = a.out + 3 * (size_t)row;
  if (n == 0) { o[0] = o[1] = o[2] = 0.f; return; }        // no face: a zero row of L, and a zero column
  const double div = a.transpose ? 1.0 : 2.0 * (double)n;   // (a division, not a reciprocal: a constant field gives exactly 0)
  const float* xv = x + 3 * (size_t)v;
  o[0] = (float)((double)xv[0] - s0 / div);
  o[1] = (float)((double)xv[1] - s1 / div);
  o[2] = (float)((double)xv[2] - s2 / div);
}

}  // namespace

void launch_offsets_apply(const DevModel& M, const DevProblem& P, const MeshCoef& mc, const float* d_off, long long off_stride,
                          float* d_cloud, long long row_floats, hipStream_t s) {
  OffsetsApplyArgs a;
  a.skinT = mc.skinT; a.wIdx = M.wIdx; a.wVal = M.wVal; a.off = d_off; a.off_stride = off_stride;
  a.cloud = d_cloud; a.row_floats = row_floats; a.V = M.V;
  BODYFIT_LAUNCH(k_offsets_apply, dim3((M.V + 255) / 256, P.F), dim3(256), 0, s, a);
}

void launch_offsets_displace(const DevModel& M, const DevProblem& P, const float* d_off, long long off_stride, float* d_bbuf,
                             hipStream_t s) {
  BODYFIT_LAUNCH(k_offsets_displace, dim3((M.V + 255) / 256, P.F), dim3(256), 0, s, d_off, off_stride, d_bbuf, M.V,
                 M.nVTiles * kVTile);
}

void launch_offsets_grad(const DevModel& M, const DevProblem& P, const float* d_gb, float* d_grad_off, long long off_stride,
                         hipStream_t s) {
  const int Vp = M.nVTiles * kVTile;
  if (off_stride > 0)
    BODYFIT_LAUNCH(k_offsets_grad_frames, dim3((M.V + 255) / 256, P.F), dim3(256), 0, s, d_gb, d_grad_off, off_stride, M.V, Vp);
  else
    BODYFIT_LAUNCH(k_offsets_grad_shared, dim3((M.V + 255) / 256, 3), dim3(256), 0, s, d_gb, d_grad_off, P.F, M.V, Vp);
}

}  // namespace bodyfit

extern "C" {

int bodyfit_surface_laplacian_device(bodyfit_surface* s, const float* d_field, long long field_stride, int n_fields,
                                     int transpose, float* d_out, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_laplacian_device";
  if (n_fields < 0) return invalid(fn, "negative n_fields");
  if (!s) return invalid(fn, "null handle");
  if (field_stride < 3LL * s->n_verts) return invalid(fn, "field_stride < 3 n_verts");
  if ((long long)n_fields * s->n_verts >= (1LL << 31) - 4096) return invalid(fn, "more than 2^31 vertices over the fields");
  if (n_fields == 0 || s->n_verts == 0) return BODYFIT_OK;
  if (!d_field || !d_out) return invalid(fn, "d_field / d_out is NULL");
  if (d_field == d_out) return invalid(fn, "in place: d_out is d_field");
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  LaplaceArgs a{};
  a.x = d_field; a.stride = field_stride; a.faces = s->d_faces;
  a.csr_off = s->d_csr_off; a.csr_fc = s->d_csr_fc;
  a.n_verts = s->n_verts; a.n_fields = n_fields; a.transpose = transpose ? 1 : 0; a.out = d_out;
  BODYFIT_LAUNCH(k_mesh_laplacian, dim3((unsigned)(((long long)n_fields * s->n_verts + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
