// k_closest_surface.hip — closest point on a frame's TRIANGLES for every query point, and its reverse-mode gradient
// (bodyfit_surface_*, bodyfit_closest_surface_device, bodyfit_closest_surface_vjp_device; declared in include/bodyfit.h).  The
// point-to-surface scan term: a scan point that lies on the posed surface costs nothing, wherever it falls between the vertices.
// bodyfit_closest_surface_oriented_device is the same search over the triangles whose face normal agrees with a direction the
// query carries (k_cs_search<true>: the gate is described at the kernel).
//
// Prepared record (k_cs_prepare, once per call, one thread per (frame, face), in f64 from the f32 corners, rounded once to
// f32; 16 floats):  the corners are rotated so that A -> B is the LONGEST edge (the lowest rotation among equals), C the third;
//   [0] A.xyz, L          L = |B - A|
//   [1] u.xyz, cx         u = (B - A) / L,  cx = (C - A) . u  (clamped to [0, L])
//   [2] w.xyz, t          w = the unit vector of (C - A) - cx u,  t = its length (the height over the longest edge)
//   [3] R, invBC, invCA, rot    R: radius of the culling sphere about the midpoint of AB, inflated by 2^-12;
//                               inv*: 1 / squared length of the 2-D edge (0 for a zero edge); rot: the rotation, as int bits
// In the frame (u, w) the triangle is (0, 0), (L, 0), (cx, t): well conditioned however thin the face is, because the thin
// direction has a unit vector of its own that was formed in f64.  A degenerate face needs no special path: collinear corners
// give t = 0, w = 0 (the face is the segment AB, which contains C since AB is the longest edge), a point gives L = 0, u = 0.
// A face with a non-finite corner gets R = NaN and is never looked at.
//
// Search (k_cs_search): the skeleton of closest_group_inl.h, as in k_closest — a workgroup of four waves owns 256 queries of one
// frame, every lane four of them with their running (min, argmin) in registers, records go through LDS 256 at a time and are read
// back at wave-uniform addresses, the waves take a tile's records in turn and meet in LDS by (value, index).  Per pair, in f32:
//   ap = p - A;  X = ap . u;  cull: |ap - (L/2) u|^2 > (sqrt(best) (1 + 2^-12) + R)^2 -> next triangle;
//   Y = ap . w;  the closest point (qx, qy) of the 2-D triangle to (X, Y): (X, Y) itself when the three edge functions say
//   inside (Ericson's interior region), else the nearest of the projections onto the three edges, each clamped to its segment
//   (the edge and vertex regions; a zero edge projects onto its start);  dist2 = |ap - qx u - qy w|^2.
// The cull cannot change the answer.  Its margin, 2^-12 of sqrt(best) + R with R >= L / 2, is at least 2048 u L; the errors of
// the cull test and of the pair's evaluation together stay below 342 u L (derived beside the contract in include/bodyfit.h).
// So a culled triangle's COMPUTED distance is above the running best and could neither win nor tie.  Hence index is the
// lowest index of the minimum computed distance over the frame's faces, whatever the split over blockIdx.y, the wave a record
// fell to and the other frames hold.  k_cs_finish evaluates the winner once more for the barycentrics: w_C = qy / t,
// w_B = (qx - w_C cx) / L, both rounded to multiples of 2^-23 and clamped so that w_A = 1 - w_B - w_C is exact and >= 0: the
// three f32 weights sum to 1 EXACTLY (one ulp of the sum would move the point by 2^-24 |v|, 0.2 um at 3 m, ten times the bound).
//
// Backward (k_cs_vjp_faces, k_cs_vjp_verts): with d_i = p_i - c_i = (p - v0) - b1 (v1 - v0) - b2 (v2 - v0) in f32,
// dL/dquery_i = 2 g_i d_i is one thread per query; dL/dverts is scatter-free in two stages: per (frame, face) the nine sums
// S[a][:] = sum_i b_ia (-2 g_i d_i) over the queries that chose the face, in ascending query order (a face more than 64 queries
// chose: the wave, 64 interleaved ascending partial sums and a fixed butterfly) — the grouping of closest_group_inl.h with
// rows = faces — then one thread per (frame, vertex) adds its incident (face, corner) entries in ascending (face, corner) order
// through the vertex -> corner CSR the handle built from the topology.  No float atomics; every order depends on the frame alone.
// Rows VJP (k_cs_rows_vjp_faces, k_cs_rows_vjp_verts; bodyfit_surface_rows_vjp_device): the same two stages for rows that arrive with
// their weights, coefficient and direction (the depth rows of k_raster_rows.hip, any point-to-plane row), summed in f64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "host_state.h"

#include "surface_handle.h"

namespace bodyfit {

namespace {

constexpr int kSTileT = 256;          // triangle records per LDS tile (16 KB)
constexpr float kCullInflate = 1.0f + 1.0f / 4096.0f;

struct SurfArgs {
  PointSet q;
  const float* verts;       // [F][vstride]
  long long vstride;
  const int* faces;         // [n_faces][3]
  int n_faces, F, n_split;
  long long nq_total;
  float4* rec;              // [F][n_faces][4]
  float* dist2; int* index; float* bary;
  float* part_d; int* part_i;
  const float* qn;          // oriented search: the queries' directions, packed [nq_total][3] in the row order of dist2
  float min_cos;            // oriented search: a triangle is a candidate iff (u x w) . m >= min_cos
};

__global__ __launch_bounds__(256) void k_cs_prepare(const SurfArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.F * a.n_faces) return;
  const int f = (int)(row / a.n_faces), t = (int)(row - (long long)f * a.n_faces);
  const float* vb = a.verts + (size_t)f * (size_t)a.vstride;
  double v[3][3];
  bool finite = true;
  for (int i = 0; i < 3; ++i) {
    const int id = a.faces[3 * t + i];
    for (int c = 0; c < 3; ++c) {
      const float x = vb[3 * (size_t)id + c];
      finite = finite && isfinite(x);
      v[i][c] = (double)x;
    }
  }
  float4* out = a.rec + 4 * (size_t)row;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  if (!finite) {
    out[0] = make_float4(0.f, 0.f, 0.f, 0.f); out[1] = out[0]; out[2] = out[0];
    out[3] = make_float4(nan, 0.f, 0.f, __int_as_float(0));
    return;
  }
  double l2[3];
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3;
    const double dx = v[j][0] - v[i][0], dy = v[j][1] - v[i][1], dz = v[j][2] - v[i][2];
    l2[i] = dx * dx + dy * dy + dz * dz;
  }
  int r = 0;
  if (l2[1] > l2[r]) r = 1;
  if (l2[2] > l2[r]) r = 2;
  const double* A = v[r];
  const double* B = v[(r + 1) % 3];
  const double* C = v[(r + 2) % 3];
  double L = sqrt(l2[r]);
  double u[3] = {0, 0, 0}, w[3] = {0, 0, 0}, cx = 0, th = 0;
  if ((float)L >= 1e-30f) {
    for (int c = 0; c < 3; ++c) u[c] = (B[c] - A[c]) / L;
    double e2[3];
    for (int c = 0; c < 3; ++c) e2[c] = C[c] - A[c];
    cx = e2[0] * u[0] + e2[1] * u[1] + e2[2] * u[2];
    double pr[3];
    for (int c = 0; c < 3; ++c) pr[c] = e2[c] - cx * u[c];
    th = sqrt(pr[0] * pr[0] + pr[1] * pr[1] + pr[2] * pr[2]);
    // (below 2^-40 L the direction of pr is the rounding of the f64 projection, and the height is far below an f32 ulp of L)
    if (th > L * 0x1p-40 && (float)th >= 1e-30f) {
      for (int c = 0; c < 3; ++c) w[c] = pr[c] / th;
    } else {
      th = 0;
    }
    cx = cx < 0 ? 0 : (cx > L ? L : cx);
  } else {
    L = 0;
  }
  const float Lf = (float)L, tf = (float)th;
  float cxf = (float)cx;
  cxf = cxf > Lf ? Lf : cxf;
  // the 2-D edges as the search sees them (from the rounded numbers)
  const double dbx = (double)cxf - (double)Lf;
  const double bc2 = dbx * dbx + (double)tf * tf, ca2 = (double)cxf * cxf + (double)tf * tf;
  const float invBC = bc2 >= 1e-36 ? (float)(1.0 / bc2) : 0.f, invCA = ca2 >= 1e-36 ? (float)(1.0 / ca2) : 0.f;
  const double mx = cx - 0.5 * L;
  const double Rm = fmax(0.5 * L, sqrt(mx * mx + th * th));
  const float R = (float)(Rm * (1.0 + 1.0 / 4096.0));
  out[0] = make_float4((float)A[0], (float)A[1], (float)A[2], Lf);
  out[1] = make_float4((float)u[0], (float)u[1], (float)u[2], cxf);
  out[2] = make_float4((float)w[0], (float)w[1], (float)w[2], tf);
  out[3] = make_float4(R, invBC, invCA, __int_as_float(r));
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// closest point (qx, qy) of the 2-D triangle (0,0), (L,0), (cx,t) to (X, Y) and the squared 3-D distance of ap to it
__device__ __forceinline__ float eval_tri(float ax, float ay, float az, float X, const float4 r1, const float4 r2, const float4 r3,
                                          float L, float* oqx, float* oqy) {
  const float cx = r1.w, t = r2.w, invBC = r3.y, invCA = r3.z;
  const float Y = fmaf(az, r2.z, fmaf(ay, r2.y, ax * r2.x));
  // edge AB
  float qx = fminf(fmaxf(X, 0.f), L), qy = 0.f;
  float ex = X - qx;
  float best = fmaf(Y, Y, ex * ex);
  // edge CA: from (0,0) along (cx, t)
  {
    const float tau = clamp01(fmaf(Y, t, X * cx) * invCA);
    const float sx = tau * cx, sy = tau * t;
    const float dx = X - sx, dy = Y - sy;
    const float r = fmaf(dy, dy, dx * dx);
    const bool lt = r < best;
    best = lt ? r : best; qx = lt ? sx : qx; qy = lt ? sy : qy;
  }
  // edge BC: from (L,0) along (cx - L, t)
  const float Dx = cx - L, XL = X - L;
  {
    const float tau = clamp01(fmaf(Y, t, XL * Dx) * invBC);
    const float sx = fmaf(tau, Dx, L), sy = tau * t;
    const float dx = X - sx, dy = Y - sy;
    const float r = fmaf(dy, dy, dx * dx);
    const bool lt = r < best;
    qx = lt ? sx : qx; qy = lt ? sy : qy;
  }
  // interior: on the inner side of all three edges
  const bool in = t > 0.f && Y >= 0.f && fmaf(Dx, Y, -(t * XL)) >= 0.f && fmaf(t, X, -(cx * Y)) >= 0.f;
  qx = in ? X : qx; qy = in ? Y : qy;
  const float rx = fmaf(-qy, r2.x, fmaf(-qx, r1.x, ax));
  const float ry = fmaf(-qy, r2.y, fmaf(-qx, r1.y, ay));
  const float rz = fmaf(-qy, r2.z, fmaf(-qx, r1.z, az));
  *oqx = qx; *oqy = qy;
  return fmaf(rz, rz, fmaf(ry, ry, rx * rx));
}

// kOriented: the normal-compatible search (bodyfit_closest_surface_oriented_device).  The face normal is n = u x w of the record
// (the corner rotation of k_cs_prepare is cyclic, so (B - A) x (C - A) = L t (u x w) keeps the orientation of `faces`); a record
// without a height (t = 0) has no normal and is never a candidate.  The gate sits between the cull and the evaluation and only
// removes candidates, so the cull argument stands; everything written with `if constexpr` is absent from the other instantiation.
template <bool kOriented>
__global__ __launch_bounds__(64 * kWaves) void k_cs_search(const SurfArgs a) {
  __shared__ float4 s_rec[4 * kSTileT];
  __shared__ float s_d[kWaves][kTileQ];
  __shared__ int s_i[kWaves][kTileQ];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int f, tile;
  BODYFIT_QUERY_TILE(a.q, a.F, f, tile)
  const FrameRange fq = frame_range(a.q, f);
  const int q0 = tile * kTileQ;
  if (q0 >= fq.count) return;
  float px[kQ], py[kQ], pz[kQ], best[kQ], bs[kQ];
  [[maybe_unused]] float mx[kQ], my[kQ], mz[kQ];
  int bi[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int qi = q0 + k * 64 + lane;
    const bool ok = qi < fq.count;
    const float* p = a.q.xyz + fq.first + 3 * (size_t)(ok ? qi : q0);
    px[k] = p[0]; py[k] = p[1]; pz[k] = p[2];
    if constexpr (kOriented) {
      const float* m = a.qn + 3 * (size_t)(fq.row0 + (ok ? qi : q0));
      mx[k] = m[0]; my[k] = m[1]; mz[k] = m[2];
    }
    best[k] = std::numeric_limits<float>::infinity(); bs[k] = best[k]; bi[k] = -1;
  }
  int c0 = 0, c1 = a.n_faces;
  if (a.n_split > 1) {
    const int chunk = (a.n_faces + a.n_split - 1) / a.n_split;
    c0 = min((int)blockIdx.y * chunk, a.n_faces);
    c1 = min(c0 + chunk, a.n_faces);
  }
  const float4* rbase = a.rec + 4 * (size_t)f * (size_t)a.n_faces;
  for (int t0 = c0; t0 < c1; t0 += kSTileT) {
    const int cnt = min(kSTileT, c1 - t0);
    __syncthreads();   // the previous tile has been read by every wave
    const float4* src = rbase + 4 * (size_t)t0;
    for (int j = tid; j < 4 * cnt; j += 64 * kWaves) s_rec[j] = src[j];
    __syncthreads();
    for (int j = wave; j < cnt; j += kWaves) {
      const float4 r0 = s_rec[4 * j], r1 = s_rec[4 * j + 1], r2 = s_rec[4 * j + 2], r3 = s_rec[4 * j + 3];
      const int ci = t0 + j;
      const float L = r0.w, R = r3.x;
      const float Lq = 0.25f * L * L;
      [[maybe_unused]] float nx, ny, nz;
      if constexpr (kOriented) {   // (the record is the same in every lane: so is this branch)
        if (!(r2.w > 0.f)) continue;
        nx = fmaf(r1.y, r2.z, -(r1.z * r2.y));
        ny = fmaf(r1.z, r2.x, -(r1.x * r2.z));
        nz = fmaf(r1.x, r2.y, -(r1.y * r2.x));
      }
#pragma unroll
      for (int k = 0; k < kQ; ++k) {
        const float ax = px[k] - r0.x, ay = py[k] - r0.y, az = pz[k] - r0.z;
        const float ap2 = fmaf(az, az, fmaf(ay, ay, ax * ax));
        const float X = fmaf(az, r1.z, fmaf(ay, r1.y, ax * r1.x));
        const float dc2 = fmaf(-L, X, ap2 + Lq);
        const float reach = bs[k] + R;
        if (dc2 <= reach * reach) {   // (false for a NaN on either side: a non-finite query or face is never evaluated)
          if constexpr (kOriented) {   // (false for a NaN in m or min_cos: that query has no candidate)
            if (!(fmaf(nz, mz[k], fmaf(ny, my[k], nx * mx[k])) >= a.min_cos)) continue;
          }
          float qx, qy;
          const float d = eval_tri(ax, ay, az, X, r1, r2, r3, L, &qx, &qy);
          if (d < best[k]) {
            best[k] = d; bi[k] = ci;
            bs[k] = sqrtf(d) * kCullInflate;
          }
        }
      }
    }
  }
  float bd;
  int bx;
  if (!fold_waves(s_d, s_i, best, bi, wave, lane, tid, q0, fq.count, &bd, &bx)) return;
  const size_t row = (size_t)(fq.row0 + (q0 + tid));
  if (a.n_split > 1) {
    a.part_d[(size_t)blockIdx.y * (size_t)a.nq_total + row] = bd;
    a.part_i[(size_t)blockIdx.y * (size_t)a.nq_total + row] = bx;
  } else {
    a.index[row] = bx;
  }
}

// folds the splits' partial minima by (value, index), then evaluates the winner once more: barycentrics and dist2
__global__ __launch_bounds__(256) void k_cs_finish(const SurfArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.nq_total) return;
  int bx;
  if (a.n_split > 1) {
    float bd;
    fold_splits(a.part_d, a.part_i, a.n_split, a.nq_total, row, &bd, &bx);
    a.index[row] = bx;
  } else {
    bx = a.index[row];
  }
  float b[3] = {0.f, 0.f, 0.f};
  float d2 = std::numeric_limits<float>::infinity();
  if (bx >= 0) {
    const int f = frame_of(a.q, a.F, row);
    const FrameRange fq = frame_range(a.q, f);
    const float* p = a.q.xyz + fq.first + 3 * (size_t)(row - fq.row0);
    const float4* rc = a.rec + 4 * ((size_t)f * (size_t)a.n_faces + (size_t)bx);
    const float4 r0 = rc[0], r1 = rc[1], r2 = rc[2], r3 = rc[3];
    const float ax = p[0] - r0.x, ay = p[1] - r0.y, az = p[2] - r0.z;
    const float X = fmaf(az, r1.z, fmaf(ay, r1.y, ax * r1.x));
    const float L = r0.w, cx = r1.w, t = r2.w;
    float qx, qy;
    d2 = eval_tri(ax, ay, az, X, r1, r2, r3, L, &qx, &qy);
    // weights as multiples of 2^-23 (x + 1 rounds there, - 1 is exact), so that 1 - wB - wC is exact
    float wC = t > 0.f ? clamp01(qy / t) : 0.f;
    wC = __fsub_rn(__fadd_rn(wC, 1.f), 1.f);
    float wB = L > 0.f ? clamp01(fmaf(-wC, cx, qx) / L) : 0.f;
    wB = __fsub_rn(__fadd_rn(wB, 1.f), 1.f);
    const float rest = 1.f - wC;
    wB = fminf(wB, rest);
    const float wA = rest - wB;
    const int rot = __float_as_int(r3.w);
    b[rot] = wA; b[(rot + 1) % 3] = wB; b[(rot + 2) % 3] = wC;
  }
  a.dist2[row] = d2;
  a.bary[3 * (size_t)row] = b[0]; a.bary[3 * (size_t)row + 1] = b[1]; a.bary[3 * (size_t)row + 2] = b[2];
}

// ---- backward ----------------------------------------------------------------------------------------------------------
struct SurfVjpArgs {
  PointSet q;
  const float* verts;
  long long vstride;
  const int* faces;
  int n_faces, n_verts, F;
  long long nq_total, nr_total;   // nr_total = F n_faces
  const int* index; const float* bary; const float* g;
  float* gq;               // layout of q, or nullptr
  float* gv;               // [F][vstride], or nullptr
  float* acc;              // [nr_total][9] per-face corner sums (gv only)
  const int *cnt, *start, *sorted;
  const int *csr_off, *csr_fc;    // vertex -> 3 face + corner, ascending
  unsigned qblocks;
};

// d = p - c of packed query row i (frame f, its face t): (p - v0) - b1 (v1 - v0) - b2 (v2 - v0)
__device__ __forceinline__ void residual_of(const SurfVjpArgs& a, const float* vb, const FrameRange& fq, long long i, int t, float* d,
                                            float* b) {
  const float* p = a.q.xyz + fq.first + 3 * (size_t)(i - fq.row0);
  const int i0 = a.faces[3 * t], i1 = a.faces[3 * t + 1], i2 = a.faces[3 * t + 2];
  const float* v0 = vb + 3 * (size_t)i0;
  const float* v1 = vb + 3 * (size_t)i1;
  const float* v2 = vb + 3 * (size_t)i2;
  b[0] = a.bary[3 * (size_t)i]; b[1] = a.bary[3 * (size_t)i + 1]; b[2] = a.bary[3 * (size_t)i + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = fmaf(-b[2], v2[c] - v0[c], fmaf(-b[1], v1[c] - v0[c], p[c] - v0[c]));
}

__device__ __forceinline__ void vjp_query_rows(const SurfVjpArgs& a, long long row) {
  if (row >= a.nq_total) return;
  const int f = frame_of(a.q, a.F, row);
  const FrameRange fq = frame_range(a.q, f);
  const size_t qoff = fq.first + 3 * (size_t)(row - fq.row0);
  const int t = a.index[row];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (t >= 0 && t < a.n_faces) {
    float d[3], b[3];
    residual_of(a, a.verts + (size_t)f * (size_t)a.vstride, fq, row, t, d, b);
    const float m = 2.f * a.g[row];
    gx = m * d[0]; gy = m * d[1]; gz = m * d[2];
  }
  a.gq[qoff] = gx; a.gq[qoff + 1] = gy; a.gq[qoff + 2] = gz;
}

__device__ __forceinline__ void add_term(const SurfVjpArgs& a, const float* vb, const FrameRange& fq, int i, int t, float* s) {
  float d[3], b[3];
  residual_of(a, vb, fq, i, t, d, b);
  const float m = -2.f * a.g[i];
  const float wx = m * d[0], wy = m * d[1], wz = m * d[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    s[3 * c] = fmaf(b[c], wx, s[3 * c]); s[3 * c + 1] = fmaf(b[c], wy, s[3 * c + 1]); s[3 * c + 2] = fmaf(b[c], wz, s[3 * c + 2]);
  }
}

__device__ __forceinline__ void vjp_face_rows(const SurfVjpArgs& a, long long row) {
  const int lane = threadIdx.x & 63;
  const bool live = row < a.nr_total;
  int f = 0, t = 0, n = 0, s = 0;
  if (live) {
    f = (int)(row / a.n_faces); t = (int)(row - (long long)f * a.n_faces);
    n = a.cnt[row]; s = a.start[row];
  }
  float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live && n <= kHeavy && n > 0) {
    const FrameRange fq = frame_range(a.q, f);
    const float* vb = a.verts + (size_t)f * (size_t)a.vstride;
    for (int k = 0; k < n; ++k) add_term(a, vb, fq, a.sorted[s + k], t, acc);
  }
  // faces that many queries chose: the wave sums them together, lane l entries l, l + 64, ... then a butterfly
  unsigned long long heavy = __ballot(live && n > kHeavy);
  while (heavy) {
    const int src = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const int hf = __shfl(f, src, 64), ht = __shfl(t, src, 64), hn = __shfl(n, src, 64), hs = __shfl(s, src, 64);
    const FrameRange fq = frame_range(a.q, hf);
    const float* vb = a.verts + (size_t)hf * (size_t)a.vstride;
    float part[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < hn; k += 64) add_term(a, vb, fq, a.sorted[hs + k], ht, part);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int e = 0; e < 9; ++e) part[e] += __shfl_xor(part[e], d, 64);
    }
    if (lane == src) {
#pragma unroll
      for (int e = 0; e < 9; ++e) acc[e] = part[e];
    }
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.acc[9 * (size_t)row + e] = acc[e];
  }
}

// dL/dquery and the per-face sums in one launch (the branch is uniform over a workgroup)
__global__ __launch_bounds__(256) void k_cs_vjp_faces(const SurfVjpArgs a) {
  if (blockIdx.x < a.qblocks) vjp_query_rows(a, (long long)blockIdx.x * 256 + threadIdx.x);
  else vjp_face_rows(a, (long long)(blockIdx.x - a.qblocks) * 256 + threadIdx.x);
}

// one thread per (frame, vertex): its incident (face, corner) sums in ascending order; zeros where nothing is incident
__global__ __launch_bounds__(256) void k_cs_vjp_verts(const SurfVjpArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.F * a.n_verts) return;
  const int f = (int)(row / a.n_verts), v = (int)(row - (long long)f * a.n_verts);
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const float* acc = a.acc + 9 * (size_t)f * (size_t)a.n_faces;
  for (int k = a.csr_off[v]; k < a.csr_off[v + 1]; ++k) {
    const float* e = acc + 3 * (size_t)a.csr_fc[k];
    gx += e[0]; gy += e[1]; gz += e[2];
  }
  float* out = a.gv + (size_t)f * (size_t)a.vstride + 3 * (size_t)v;
  out[0] = gx; out[1] = gy; out[2] = gz;
}

// ---- rows VJP: gverts = sum over rows of coef_i bary_ia dir_i at corner a of face index_i ----------------------------------------
// The surface backward's two stages with the rows given instead of derived from a residual: per (frame, face) the nine f64 sums
// S[a][c] = sum_i coef_i b_ia m_ic over the rows that chose the face, in ascending row order (more than kHeavy: 64 interleaved
// ascending partial sums and the same butterfly), then per (frame, vertex) the incident (face, corner) entries in ascending
// order, rounded ONCE to f32.  The vertices are never read.
struct RowsVjpArgs {
  int n_faces, n_verts, F;
  long long nr_total;               // F n_faces
  const float* bary; const float* coef; const float* dir;
  float* gv;                        // [F][vstride]
  long long vstride;
  double* acc;                      // [nr_total][9]
  const int *cnt, *start, *sorted;
  const int *csr_off, *csr_fc;
};

__device__ __forceinline__ void rows_add_term(const RowsVjpArgs& a, int i, double* s) {
  const double g = (double)a.coef[i];
  const float* b = a.bary + 3 * (size_t)i;
  const float* m = a.dir + 3 * (size_t)i;
  const double mx = (double)m[0], my = (double)m[1], mz = (double)m[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double w = g * (double)b[c];   // (exact: 48 significant bits)
    s[3 * c] += w * mx; s[3 * c + 1] += w * my; s[3 * c + 2] += w * mz;
  }
}

__global__ __launch_bounds__(256) void k_cs_rows_vjp_faces(const RowsVjpArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = row < a.nr_total;
  int n = 0, s = 0;
  if (live) { n = a.cnt[row]; s = a.start[row]; }
  double acc[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
  if (live && n <= kHeavy)
    for (int k = 0; k < n; ++k) rows_add_term(a, a.sorted[s + k], acc);
  unsigned long long heavy = __ballot(live && n > kHeavy);
  while (heavy) {
    const int src = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const int hn = __shfl(n, src, 64), hs = __shfl(s, src, 64);
    double part[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    for (int k = lane; k < hn; k += 64) rows_add_term(a, a.sorted[hs + k], part);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int e = 0; e < 9; ++e) part[e] += __shfl_xor(part[e], d, 64);
    }
    if (lane == src) {
#pragma unroll
      for (int e = 0; e < 9; ++e) acc[e] = part[e];
    }
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.acc[9 * (size_t)row + e] = acc[e];
  }
}

__global__ __launch_bounds__(256) void k_cs_rows_vjp_verts(const RowsVjpArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= (long long)a.F * a.n_verts) return;
  const int f = (int)(row / a.n_verts), v = (int)(row - (long long)f * a.n_verts);
  double gx = 0., gy = 0., gz = 0.;
  const double* acc = a.acc + 9 * (size_t)f * (size_t)a.n_faces;
  for (int k = a.csr_off[v]; k < a.csr_off[v + 1]; ++k) {
    const double* e = acc + 3 * (size_t)a.csr_fc[k];
    gx += e[0]; gy += e[1]; gz += e[2];
  }
  float* out = a.gv + (size_t)f * (size_t)a.vstride + 3 * (size_t)v;
  out[0] = (float)gx; out[1] = (float)gy; out[2] = (float)gz;
}

}  // namespace

}  // namespace bodyfit

namespace {

int check_surface_call(const char* fn, const bodyfit_surface* s, const bodyfit_pointset* query, const float* d_verts,
                       long long stride, int n_frames, long long* nq) {
  using namespace bodyfit;
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (int rc = check_set(fn, "query", query, n_frames, nq)) return rc;
  if (!s) return invalid(fn, "null handle");
  if (stride < 3LL * s->n_verts) return invalid(fn, "verts_frame_stride < 3 n_verts");
  if (n_frames > 0 && s->n_verts > 0 && !d_verts) return invalid(fn, "d_verts is NULL");
  if ((long long)n_frames * s->n_faces >= (1LL << 31) - 4096 || (long long)n_frames * s->n_verts >= (1LL << 31) - 4096)
    return invalid(fn, "more than 2^31 faces or vertices over the frames");
  return 0;
}

}  // namespace

extern "C" {

int bodyfit_surface_create(int device, int n_verts, int n_faces, const int32_t* faces, bodyfit_surface** out) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_create";
  if (!out) return invalid(fn, "null argument");
  if (n_verts < 0 || n_faces < 0) return invalid(fn, "negative count");
  if (n_faces > 0 && !faces) return invalid(fn, "faces is NULL");
  if (n_faces >= (1 << 30) / 3) return invalid(fn, "too many faces");
  std::vector<int> off((size_t)n_verts + 1, 0), fc(3 * (size_t)n_faces);
  for (size_t k = 0; k < 3 * (size_t)n_faces; ++k) {
    if (faces[k] < 0 || faces[k] >= n_verts) return invalid(fn, "a face id outside [0, n_verts)");
    ++off[(size_t)faces[k] + 1];
  }
  for (int v = 0; v < n_verts; ++v) off[v + 1] += off[v];
  {
    std::vector<int> at(off.begin(), off.end() - 1);
    for (size_t k = 0; k < 3 * (size_t)n_faces; ++k) fc[at[faces[k]]++] = (int)k;   // ascending 3 face + corner
  }
  ClosestWorkspace w;
  if (int rc = open_workspace(fn, device, &w)) return rc;
  bodyfit_surface* s = new bodyfit_surface;
  s->w = w;
  s->n_verts = n_verts; s->n_faces = n_faces;
  const size_t fb = 3 * (size_t)n_faces * 4, ob = ((size_t)n_verts + 1) * 4;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_faces), fb + 4);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->d_csr_off), ob);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->d_csr_fc), fb + 4);
  if (e == hipSuccess && fb) e = hipMemcpy(s->d_faces, faces, fb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->d_csr_off, off.data(), ob, hipMemcpyHostToDevice);
  if (e == hipSuccess && fb) e = hipMemcpy(s->d_csr_fc, fc.data(), fb, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    bodyfit_surface_destroy(s);
    return fail(BODYFIT_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  }
  *out = s;
  return BODYFIT_OK;
}

void bodyfit_surface_destroy(bodyfit_surface* s) {
  if (!s) return;
  (void)hipSetDevice(s->w.device);
  for (void* p : {(void*)s->d_faces, (void*)s->d_csr_off, (void*)s->d_csr_fc, (void*)s->rec, (void*)s->acc, (void*)s->gram})
    if (p) (void)hipFree(p);
  bodyfit::release_workspace(&s->w);
  delete s;
}

}  // extern "C"

namespace {

// both searches: `oriented` selects the instantiation of k_cs_search, nothing else differs
int closest_surface_call(const char* fn, bool oriented, bodyfit_surface* s, const bodyfit_pointset* query,
                         const float* d_query_normals, float min_cos, const float* d_verts, long long verts_frame_stride,
                         int n_frames, long long n_query_total, float* d_dist2, int32_t* d_index, float* d_bary, int prepare_vjp,
                         void* stream) {
  using namespace bodyfit;
  if (int rc = check_surface_call(fn, s, query, d_verts, verts_frame_stride, n_frames, &n_query_total)) return rc;
  if (!d_dist2 || !d_index || !d_bary) return invalid(fn, "d_dist2 / d_index / d_bary is NULL");
  if (oriented && n_frames > 0 && n_query_total > 0 && !d_query_normals) return invalid(fn, "d_query_normals is NULL");
  if (n_frames == 0 || n_query_total == 0) return BODYFIT_OK;
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  invalidate(&s->w, d_index);
  SurfArgs a{};
  a.q = device_set(query);
  a.verts = d_verts; a.vstride = verts_frame_stride; a.faces = s->d_faces; a.n_faces = s->n_faces;
  a.F = n_frames; a.nq_total = n_query_total;
  a.dist2 = d_dist2; a.index = d_index; a.bary = d_bary;
  a.qn = d_query_normals; a.min_cos = min_cos;
  long long tiles;
  if (int rc = query_tiles(fn, query, n_query_total, n_frames, &tiles)) return rc;
  a.n_split = choose_split(s->w.n_cu, tiles, s->n_faces);
  const long long n_rows = (long long)n_frames * s->n_faces;
  const bool group = prepare_vjp && n_rows > 0;
  if (int rc = reserve_search_scratch(&s->w, a.n_split, n_query_total, group, &a.part_d, &a.part_i)) return rc;
  if (int rc = reserve(&s->rec, &s->rec_bytes, (size_t)n_rows * 64)) return rc;
  a.rec = reinterpret_cast<float4*>(s->rec);
  if (n_rows > 0) BODYFIT_LAUNCH(k_cs_prepare, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, a);
  if (oriented) BODYFIT_LAUNCH(k_cs_search<true>, dim3((unsigned)tiles, (unsigned)a.n_split), dim3(64 * kWaves), 0, st, a);
  else BODYFIT_LAUNCH(k_cs_search<false>, dim3((unsigned)tiles, (unsigned)a.n_split), dim3(64 * kWaves), 0, st, a);
  BODYFIT_LAUNCH(k_cs_finish, dim3((unsigned)((n_query_total + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  if (group) {   // (behind the fold on the stream: the scratch may lie over the partial minima)
    const bodyfit_pointset fr = face_rows(s);
    Grouping* g = nullptr;
    return build_grouping(&s->w, query, &fr, n_frames, n_query_total, n_rows, d_index, true, st, &g);
  }
  return BODYFIT_OK;
}

}  // namespace

extern "C" {

int bodyfit_closest_surface_device(bodyfit_surface* s, const bodyfit_pointset* query, const float* d_verts,
                                   long long verts_frame_stride, int n_frames, long long n_query_total, float* d_dist2,
                                   int32_t* d_index, float* d_bary, int prepare_vjp, void* stream) {
  return closest_surface_call("bodyfit_closest_surface_device", false, s, query, nullptr, 0.f, d_verts, verts_frame_stride, n_frames,
                              n_query_total, d_dist2, d_index, d_bary, prepare_vjp, stream);
}

int bodyfit_closest_surface_oriented_device(bodyfit_surface* s, const bodyfit_pointset* query, const float* d_query_normals,
                                            float min_cos, const float* d_verts, long long verts_frame_stride, int n_frames,
                                            long long n_query_total, float* d_dist2, int32_t* d_index, float* d_bary,
                                            int prepare_vjp, void* stream) {
  return closest_surface_call("bodyfit_closest_surface_oriented_device", true, s, query, d_query_normals, min_cos, d_verts,
                              verts_frame_stride, n_frames, n_query_total, d_dist2, d_index, d_bary, prepare_vjp, stream);
}

int bodyfit_closest_surface_vjp_device(bodyfit_surface* s, const bodyfit_pointset* query, const float* d_verts,
                                       long long verts_frame_stride, int n_frames, long long n_query_total, const int32_t* d_index,
                                       const float* d_bary, const float* d_grad_dist2, float* d_grad_query, float* d_grad_verts,
                                       void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_closest_surface_vjp_device";
  if (int rc = check_surface_call(fn, s, query, d_verts, verts_frame_stride, n_frames, &n_query_total)) return rc;
  if (n_query_total > 0 && (!d_index || !d_bary || !d_grad_dist2)) return invalid(fn, "d_index / d_bary / d_grad_dist2 is NULL");
  if (n_frames == 0 || (!d_grad_query && !d_grad_verts)) return BODYFIT_OK;
  if (n_query_total == 0 && (!d_grad_verts || s->n_verts == 0)) return BODYFIT_OK;
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long n_rows = (long long)n_frames * s->n_faces;
  const bodyfit_pointset fr = face_rows(s);
  SurfVjpArgs a{};
  a.q = device_set(query);
  a.verts = d_verts; a.vstride = verts_frame_stride; a.faces = s->d_faces;
  a.n_faces = s->n_faces; a.n_verts = s->n_verts; a.F = n_frames;
  a.nq_total = n_query_total; a.nr_total = n_rows;
  a.index = d_index; a.bary = d_bary; a.g = d_grad_dist2;
  a.gq = n_query_total > 0 ? d_grad_query : nullptr;
  a.gv = s->n_verts > 0 ? d_grad_verts : nullptr;
  a.csr_off = s->d_csr_off; a.csr_fc = s->d_csr_fc;
  a.qblocks = a.gq ? (unsigned)((n_query_total + 255) / 256) : 0u;
  unsigned fblocks = 0;
  if (a.gv && n_rows > 0) {
    Grouping* g = nullptr;
    if (int rc = kept_or_built_grouping(&s->w, query, &fr, n_frames, n_query_total, n_rows, d_index, st, &g)) return rc;
    a.cnt = g->cnt; a.start = g->start; a.sorted = g->sorted;
    if (int rc = reserve(&s->acc, &s->acc_bytes, (size_t)n_rows * 36)) return rc;
    a.acc = reinterpret_cast<float*>(s->acc);
    fblocks = (unsigned)((n_rows + 255) / 256);
  }
  if (a.qblocks + fblocks) BODYFIT_LAUNCH(k_cs_vjp_faces, dim3(a.qblocks + fblocks), dim3(256), 0, st, a);
  if (a.gv)
    BODYFIT_LAUNCH(k_cs_vjp_verts, dim3((unsigned)(((long long)n_frames * s->n_verts + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_surface_rows_vjp_device(bodyfit_surface* s, const bodyfit_pointset* rows, int n_frames, long long n_rows_total,
                                    const int32_t* d_index, const float* d_bary, const float* d_coef, const float* d_dir,
                                    float* d_gverts, long long gverts_frame_stride, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_rows_vjp_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (int rc = check_set(fn, "rows", rows, n_frames, &n_rows_total)) return rc;
  if (!s) return invalid(fn, "null handle");
  if (gverts_frame_stride < 3LL * s->n_verts) return invalid(fn, "gverts_frame_stride < 3 n_verts");
  if (n_rows_total > 0 && (!d_index || !d_bary || !d_coef || !d_dir)) return invalid(fn, "d_index / d_bary / d_coef / d_dir is NULL");
  const long long n_face_rows = (long long)n_frames * s->n_faces;
  if (n_face_rows >= (1LL << 31) - 4096 || (long long)n_frames * s->n_verts >= (1LL << 31) - 4096)
    return invalid(fn, "more than 2^31 faces or vertices over the frames");
  if (n_frames == 0 || s->n_verts == 0) return BODYFIT_OK;
  if (!d_gverts) return invalid(fn, "d_gverts is NULL");
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bodyfit_pointset fr = face_rows(s);
  RowsVjpArgs a{};
  a.n_faces = s->n_faces; a.n_verts = s->n_verts; a.F = n_frames; a.nr_total = n_face_rows;
  a.bary = d_bary; a.coef = d_coef; a.dir = d_dir;
  a.gv = d_gverts; a.vstride = gverts_frame_stride;
  a.csr_off = s->d_csr_off; a.csr_fc = s->d_csr_fc;
  if (n_face_rows > 0) {
    Grouping* g = nullptr;
    if (int rc = kept_or_built_grouping(&s->w, rows, &fr, n_frames, n_rows_total, n_face_rows, d_index, st, &g)) return rc;
    a.cnt = g->cnt; a.start = g->start; a.sorted = g->sorted;
    if (int rc = reserve(&s->acc, &s->acc_bytes, (size_t)n_face_rows * 72)) return rc;
    a.acc = reinterpret_cast<double*>(s->acc);
    BODYFIT_LAUNCH(k_cs_rows_vjp_faces, dim3((unsigned)((n_face_rows + 255) / 256)), dim3(256), 0, st, a);
  }
  BODYFIT_LAUNCH(k_cs_rows_vjp_verts, dim3((unsigned)(((long long)n_frames * s->n_verts + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
