// k_winding.hip — the winding number of a frame's posed mesh about every query point (bodyfit_surface_winding_device) and the
// area-weighted vertex normals (bodyfit_surface_vertex_normals_device; declared in include/bodyfit.h).  The inside / outside
// question of the self-penetration term and of a signed distance: an all-pairs (query x triangle) sum per frame, no tree.
//
// Winding (k_wn_sum, k_wn_finish): the skeleton of closest_group_inl.h, as in k_cs_search — a workgroup of four waves owns 256
// queries of one frame, every lane four of them; the frame's triangles go through LDS 256 at a time and are read back at
// wave-uniform addresses (a broadcast), the waves take a tile's triangles in turn.  There is no prepared record in memory: thread j
// of the workgroup gathers triangle j of the tile from `faces` and the frame's vertices (nine f32 and three ids, 48 bytes in LDS),
// 2,304 dwords per 65,536 pairs.  A triangle with a non-finite corner is stored as zeros (it then contributes an exact 0) and
// raises the workgroup's flag: every query of the frame gets NaN.  Per pair, in f32, with a = v0 - p, b = v1 - p, c = v2 - p:
//   la = sqrt(a . a), lb, lc;  n = b x c, each component fma(x, y, -(z w));  num = a . n;
//   den = fma(a . b, lc, fma(b . c, la, fma(c . a, lb, la lb lc)));          (every dot a three-term fma chain)
//   theta = atan2(num, den), half the solid angle: with mx, mn the larger and the smaller of |num|, |den|,
//     t = mn / mx, or (mn - mx) / (mn + mx) behind pi / 4 where mn > tan(pi / 8) mx (ONE correctly rounded division),
//     r = t + t z (((c0 z + c1) z + c2) z + c3), z = t^2 (Cephes' atanf coefficients: within 0.14 u of atan on the reduced range),
//     then pi / 2 - r where |num| > |den|, pi - r where den < 0, the sign of num; mx = 0 gives 0 (atan2(0, 0) = 0: a corner at p).
// The sum is EXACT: theta is rounded to a multiple of 2^-32 (2^-33, 0.002 u, beside the 10 u of the atan2) and added as a 64-bit
// integer — fma((double)theta, 2^32, 1.5 2^52) holds round(theta 2^32) in its low mantissa bits, the bits are added modulo 2^64
// and the constant's are taken off once at the end.  |theta| <= pi and n_faces < 2^30 / 3 keep the sum below 2^63.  Integer
// addition is associative, so the result does not depend on the wave a triangle fell to, on the split of the face range over
// blockIdx.y, or on anything outside the frame: w = (float)(sum 2^-32 / 2 pi), rounded once.  No atomics at all.
// kSkip: row i leaves out the triangles that have skip[i] >= 0 among their three ids (their theta is replaced by 0, so every
// lane adds the same number of terms); the other instantiation never reads the ids.
// The error bound of all this is derived beside the declaration in include/bodyfit.h (k = 64, k_s = 16).  It holds for distances
// between 2^-40 and 2^40; beyond, la lb lc overflows, theta becomes a NaN whose BITS enter the integer sum, and the row's result
// is undefined and possibly finite (only non-finite inputs are flagged: a per-pair test of theta was not worth its issue slots).
//
// Vertex normals (k_vertex_normals): one thread per (frame, vertex) walks the handle's vertex -> corner table in ascending order
// and adds (v1 - v0) x (v2 - v0) of every incident face ONCE (a face that repeats the id is taken at its first corner), in f64 with
// contraction off (a repeated corner then gives an exact zero), normalises in f64 and rounds once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "host_state.h"

#include "surface_handle.h"

namespace bodyfit {

namespace {

constexpr int kWTileT = 256;          // triangles per LDS tile (12 KB): one per thread of the workgroup
constexpr double kFixScale = 4294967296.0;            // 2^32: the grid of the exact sum
constexpr double kFixMagic = 6755399441055744.0;      // 1.5 2^52: its low mantissa bits hold the integer
constexpr long long kNanPartial = std::numeric_limits<long long>::min();   // a split's partial sum: "the frame holds a non-finite face"

struct WindArgs {
  PointSet q;
  const int* skip;          // [nq_total] packed like the output, or nullptr
  const float* verts;       // [F][vstride]
  long long vstride;
  const int* faces;         // [n_faces][3]
  int n_faces, F, n_split;
  long long nq_total;
  float* winding;           // [nq_total]
  long long* part;          // [n_split][nq_total] (n_split > 1)
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// atan2(y, x) as the header derives its error: one division, a degree-9 odd polynomial, three reflections
__device__ __forceinline__ float atan2_reduced(float y, float x) {
  const float ay = fabsf(y), ax = fabsf(x);
  const bool swap = ay > ax;
  const float mx = swap ? ay : ax, mn = swap ? ax : ay;     // (selects, not fmaxf: a NaN stays a NaN)
  const bool hi = mn > 0.41421357f * mx;
  const float n = hi ? mn - mx : mn, d = hi ? mn + mx : mx;
  const float t = d == 0.f ? 0.f : n / d;
  const float z = t * t;
  float p = 8.05374449538e-2f;
  p = fmaf(p, z, -1.38776856032e-1f);
  p = fmaf(p, z, 1.99777106478e-1f);
  p = fmaf(p, z, -3.33329491539e-1f);
  float r = fmaf(p * z, t, t);
  r = hi ? r + 0.78539816339744830962f : r;
  r = swap ? 1.57079632679489661923f - r : r;
  r = x < 0.f ? 3.14159265358979323846f - r : r;
  return copysignf(r, y);
}

// w of packed row `row` from the exact sum of its half angles (in units of 2^-32 rad); a non-finite query or face: NaN
__device__ __forceinline__ float winding_of(long long sum, bool bad) {
  return bad ? std::numeric_limits<float>::quiet_NaN() : (float)((double)sum * (1.0 / kFixScale) * 0.15915494309189533577);
}

template <bool kSkip>
__global__ __launch_bounds__(64 * kWaves) void k_wn_sum(const WindArgs a) {
  __shared__ float4 s_tri[3 * kWTileT];
  __shared__ unsigned long long s_acc[kWaves][kTileQ];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int f, tile;
  BODYFIT_QUERY_TILE(a.q, a.F, f, tile)
  const FrameRange fq = frame_range(a.q, f);
  const int q0 = tile * kTileQ;
  if (q0 >= fq.count) return;
  if (tid == 0) s_bad = 0;
  float px[kQ], py[kQ], pz[kQ];
  [[maybe_unused]] int sk[kQ];
  unsigned long long acc[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int qi = q0 + k * 64 + lane;
    const bool ok = qi < fq.count;
    const float* p = a.q.xyz + fq.first + 3 * (size_t)(ok ? qi : q0);
    const float x = p[0], y = p[1], z = p[2];
    const bool fin = isfinite(x) && isfinite(y) && isfinite(z);   // (a non-finite query is summed as the origin; k_wn_finish and
    px[k] = fin ? x : 0.f; py[k] = fin ? y : 0.f; pz[k] = fin ? z : 0.f;   //  the fold below write its NaN)
    if constexpr (kSkip) sk[k] = a.skip[fq.row0 + (ok ? qi : q0)];
    acc[k] = 0ull;
  }
  int c0 = 0, c1 = a.n_faces;
  if (a.n_split > 1) {
    const int chunk = (a.n_faces + a.n_split - 1) / a.n_split;
    c0 = min((int)blockIdx.y * chunk, a.n_faces);
    c1 = min(c0 + chunk, a.n_faces);
  }
  const float* vb = a.verts + (size_t)f * (size_t)a.vstride;
  unsigned n_terms = 0;
  for (int t0 = c0; t0 < c1; t0 += kWTileT) {
    const int cnt = min(kWTileT, c1 - t0);
    __syncthreads();   // the previous tile has been read by every wave (and s_bad = 0 has landed)
    if (tid < cnt) {
      const int* id = a.faces + 3 * (size_t)(t0 + tid);
      const int i0 = id[0], i1 = id[1], i2 = id[2];
      const float* v0 = vb + 3 * (size_t)i0;
      const float* v1 = vb + 3 * (size_t)i1;
      const float* v2 = vb + 3 * (size_t)i2;
      float4 r0 = make_float4(v0[0], v0[1], v0[2], __int_as_float(i0));
      float4 r1 = make_float4(v1[0], v1[1], v1[2], __int_as_float(i1));
      float4 r2 = make_float4(v2[0], v2[1], v2[2], __int_as_float(i2));
      const bool fin = isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z) &&
                       isfinite(r2.x) && isfinite(r2.y) && isfinite(r2.z);
      if (!fin) {
        r0.x = r0.y = r0.z = 0.f; r1.x = r1.y = r1.z = 0.f; r2.x = r2.y = r2.z = 0.f;
        s_bad = 1;   // (every writer stores the same value)
      }
      s_tri[3 * tid] = r0; s_tri[3 * tid + 1] = r1; s_tri[3 * tid + 2] = r2;
    }
    __syncthreads();
    for (int j = wave; j < cnt; j += kWaves) {
      const float4 r0 = s_tri[3 * j], r1 = s_tri[3 * j + 1], r2 = s_tri[3 * j + 2];
      [[maybe_unused]] int i0, i1, i2;
      if constexpr (kSkip) { i0 = __float_as_int(r0.w); i1 = __float_as_int(r1.w); i2 = __float_as_int(r2.w); }
      ++n_terms;
#pragma unroll
      for (int k = 0; k < kQ; ++k) {
        const float ax = r0.x - px[k], ay = r0.y - py[k], az = r0.z - pz[k];
        const float bx = r1.x - px[k], by = r1.y - py[k], bz = r1.z - pz[k];
        const float cx = r2.x - px[k], cy = r2.y - py[k], cz = r2.z - pz[k];
        const float la = sqrtf(dot3(ax, ay, az, ax, ay, az));
        const float lb = sqrtf(dot3(bx, by, bz, bx, by, bz));
        const float lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
        const float nx = fmaf(by, cz, -(bz * cy));
        const float ny = fmaf(bz, cx, -(bx * cz));
        const float nz = fmaf(bx, cy, -(by * cx));
        const float num = dot3(ax, ay, az, nx, ny, nz);
        const float den = fmaf(dot3(ax, ay, az, bx, by, bz), lc,
                               fmaf(dot3(bx, by, bz, cx, cy, cz), la, fmaf(dot3(cx, cy, cz, ax, ay, az), lb, la * lb * lc)));
        float th = atan2_reduced(num, den);
        if constexpr (kSkip) th = (sk[k] >= 0 && (sk[k] == i0 || sk[k] == i1 || sk[k] == i2)) ? 0.f : th;
        acc[k] += (unsigned long long)__double_as_longlong(fma((double)th, kFixScale, kFixMagic));
      }
    }
  }
  // the waves meet in LDS; thread tid owns query q0 + tid.  Every wave added n_terms numbers that carry the magic constant's bits.
  const unsigned long long magic = (unsigned long long)__double_as_longlong(kFixMagic);
#pragma unroll
  for (int k = 0; k < kQ; ++k) s_acc[wave][k * 64 + lane] = acc[k] - (unsigned long long)n_terms * magic;
  __syncthreads();
  if (q0 + tid >= fq.count) return;
  unsigned long long sum = s_acc[0][tid];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) sum += s_acc[w][tid];
  const size_t row = (size_t)(fq.row0 + (q0 + tid));
  if (a.n_split > 1) {
    a.part[(size_t)blockIdx.y * (size_t)a.nq_total + row] = s_bad ? kNanPartial : (long long)sum;
  } else {
    const float* p = a.q.xyz + fq.first + 3 * (size_t)(q0 + tid);
    const bool fin = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    a.winding[row] = winding_of((long long)sum, s_bad || !fin);
  }
}

// adds the splits' partial sums (exact: any order gives these bits)
__global__ __launch_bounds__(256) void k_wn_finish(const WindArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.nq_total) return;
  const int f = frame_of(a.q, a.F, row);
  const FrameRange fq = frame_range(a.q, f);
  const float* p = a.q.xyz + fq.first + 3 * (size_t)(row - fq.row0);
  bool bad = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
  unsigned long long sum = 0ull;
  for (int s = 0; s < a.n_split; ++s) {
    const long long v = a.part[(size_t)s * (size_t)a.nq_total + row];
    bad = bad || v == kNanPartial;
    sum += (unsigned long long)v;
  }
  a.winding[row] = winding_of((long long)sum, bad);
}

struct NormalArgs {
  const float* verts;
  long long vstride;
  const int* faces;
  const int *csr_off, *csr_fc;
  int n_verts, F;
  float* out;               // [F][n_verts][3]
};

__global__ __launch_bounds__(256) void k_vertex_normals(const NormalArgs a) {
#pragma clang fp contract(off)
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
  const bool ok = isfinite(l) && l > 0.;   // (a non-finite corner makes l NaN or inf)
  float* out = a.out + 3 * (size_t)row;
  out[0] = ok ? (float)(sx / l) : 0.f;
  out[1] = ok ? (float)(sy / l) : 0.f;
  out[2] = ok ? (float)(sz / l) : 0.f;
}

}  // namespace

}  // namespace bodyfit

extern "C" {

int bodyfit_surface_winding_device(bodyfit_surface* s, const bodyfit_pointset* query, const int32_t* d_skip_vertex,
                                   const float* d_verts, long long verts_frame_stride, int n_frames, long long n_query_total,
                                   float* d_winding, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_winding_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (int rc = check_set(fn, "query", query, n_frames, &n_query_total)) return rc;
  if (!s) return invalid(fn, "null handle");
  if (verts_frame_stride < 3LL * s->n_verts) return invalid(fn, "verts_frame_stride < 3 n_verts");
  if (n_frames > 0 && s->n_verts > 0 && !d_verts) return invalid(fn, "d_verts is NULL");
  if ((long long)n_frames * s->n_faces >= (1LL << 31) - 4096 || (long long)n_frames * s->n_verts >= (1LL << 31) - 4096)
    return invalid(fn, "more than 2^31 faces or vertices over the frames");
  if (!d_winding) return invalid(fn, "d_winding is NULL");
  if (n_frames == 0 || n_query_total == 0) return BODYFIT_OK;
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  WindArgs a{};
  a.q = device_set(query);
  a.skip = d_skip_vertex;
  a.verts = d_verts; a.vstride = verts_frame_stride; a.faces = s->d_faces; a.n_faces = s->n_faces;
  a.F = n_frames; a.nq_total = n_query_total;
  a.winding = d_winding;
  long long tiles;
  if (int rc = query_tiles(fn, query, n_query_total, n_frames, &tiles)) return rc;
  a.n_split = choose_split(s->w.n_cu, tiles, s->n_faces);
  if (a.n_split > 1) {
    if (int rc = reserve(&s->w.ws, &s->w.ws_bytes, (size_t)a.n_split * (size_t)n_query_total * 8)) return rc;
    a.part = reinterpret_cast<long long*>(s->w.ws);
  }
  const dim3 grid((unsigned)tiles, (unsigned)a.n_split);
  if (d_skip_vertex) BODYFIT_LAUNCH(k_wn_sum<true>, grid, dim3(64 * kWaves), 0, st, a);
  else BODYFIT_LAUNCH(k_wn_sum<false>, grid, dim3(64 * kWaves), 0, st, a);
  if (a.n_split > 1) BODYFIT_LAUNCH(k_wn_finish, dim3((unsigned)((n_query_total + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_surface_vertex_normals_device(bodyfit_surface* s, const float* d_verts, long long verts_frame_stride, int n_frames,
                                          float* d_normals, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_vertex_normals_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (!s) return invalid(fn, "null handle");
  if (verts_frame_stride < 3LL * s->n_verts) return invalid(fn, "verts_frame_stride < 3 n_verts");
  if ((long long)n_frames * s->n_verts >= (1LL << 31) - 4096) return invalid(fn, "more than 2^31 vertices over the frames");
  if (n_frames == 0 || s->n_verts == 0) return BODYFIT_OK;
  if (!d_verts || !d_normals) return invalid(fn, "d_verts / d_normals is NULL");
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  NormalArgs a{};
  a.verts = d_verts; a.vstride = verts_frame_stride; a.faces = s->d_faces;
  a.csr_off = s->d_csr_off; a.csr_fc = s->d_csr_fc;
  a.n_verts = s->n_verts; a.F = n_frames; a.out = d_normals;
  BODYFIT_LAUNCH(k_vertex_normals, dim3((unsigned)(((long long)n_frames * s->n_verts + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
