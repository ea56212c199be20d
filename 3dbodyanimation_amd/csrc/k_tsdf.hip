// TSDF fusion: depth maps integrated into a truncated signed-distance volume, the running average of the projective distance along
// the optical axis (bodyfit_volume_integrate_device; include/bodyfit.h: the definition, the contract and the derivation of its
// constants; the host entry: api_volume.hip).
//
//   k_tsdf_integrate<POSE>  one lane per voxel, x fastest (neighbouring lanes project to neighbouring pixels of a row), a workgroup
//                inside one volume.  The state (D, W) is read once (not at all under reset), lives in two registers across the
//                frame loop and is written once.  A frame's camera is wave-uniform: its 12 pose values and the intrinsics are read
//                at a uniform address (scalar loads, scalar registers).  The frames are taken TSDF_AHEAD at a time, the rest one
//                by one: the projections and the depth gathers of a group are issued before the first of its updates (the only
//                chain from frame to frame is the two-register state); a lane that misses the image gathers pixel 0 of the
//                frame and discards it, so a group is straight-line code.  The state is rounded to f32 after every frame: a
//                call with F frames is the chain of F calls, bit for bit.  Unfused f64; plain stores.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "bodyfit_device.h"
#include "volume.h"

#pragma clang fp contract(off)

#ifndef TSDF_AHEAD
#define TSDF_AHEAD 2      // (measured beside 1, 4 and 8: tools/tsdf_bench.py --variant, profiles/tsdf_bench.txt)
#endif

namespace bodyfit {

namespace {

// N consecutive frames from frame f: the N projections and depth gathers first, then the N updates of (D, W) in ascending order
template <bool POSE, int N>
__device__ __forceinline__ void tsdf_frames(const TsdfArgs& A, int f, double px, double py, double pz, float& D, float& W) {
  const double w_last = (double)(A.W - 1), h_last = (double)(A.H - 1);
  double qz[N];
  float d[N];
  bool hit[N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
    double qx = px, qy = py;
    qz[a] = pz;
    if (POSE) {
      const double* P = A.pose + 12 * (size_t)(f + a);
      qx = P[0] * px + P[1] * py + P[2] * pz + P[3];
      qy = P[4] * px + P[5] * py + P[6] * pz + P[7];
      qz[a] = P[8] * px + P[9] * py + P[10] * pz + P[11];
    }
    // (one reciprocal and two products where the definition has two quotients: a rounding more each, inside the pixel band)
    const double inv = 1.0 / qz[a];
    const double cj = __builtin_floor(A.fx * qx * inv + A.cx + 0.5), ci = __builtin_floor(A.fy * qy * inv + A.cy + 0.5);
    // (& and not &&: one test of the lanes; every comparison is false on a NaN; the range is tested before anything is an index)
    hit[a] = (qz[a] > A.z_near) & (cj >= 0.0) & (cj <= w_last) & (ci >= 0.0) & (ci <= h_last);
    const int pixel = hit[a] ? (int)ci * A.W + (int)cj : 0;
    d[a] = A.depth[(size_t)(f + a) * (size_t)A.depth_stride + (size_t)pixel];
  }
#pragma unroll
  for (int a = 0; a < N; ++a) {
    const double s = (double)d[a] - qz[a];
    if (hit[a] & (d[a] - d[a] == 0.0f) & (d[a] > 0.0f) & (s >= -A.trunc)) {
      const bool seen = (W > 0.0f) & (D - D == 0.0f);
      const double w0 = seen ? (double)W : 0.0, wd = seen ? (double)W * (double)D : 0.0;
      const double w1 = w0 + 1.0;
      D = (float)((wd + (s < A.trunc ? s : A.trunc)) / w1);
      W = (float)(w1 < A.max_weight ? w1 : A.max_weight);
    }
  }
}

template <bool POSE>
__global__ __launch_bounds__(256) void k_tsdf_integrate(const TsdfArgs A) {
  // a workgroup never straddles two volumes: the volume, and with it the frame range, is wave-uniform
  const unsigned vol = blockIdx.x / A.chunks;
  const unsigned n = (blockIdx.x - vol * A.chunks) * 256 + threadIdx.x;
  if (n >= A.n_voxels) return;
  const bool shared = A.volume_stride == 0;
  const int f_end = shared ? A.F : (int)vol + 1;
  const size_t at = (size_t)vol * (size_t)A.volume_stride + (size_t)n;
  float D = __builtin_nanf(""), W = 0.0f;
  if (!A.reset) { D = A.tsdf[at]; W = A.weight[at]; }
  const unsigned i = n % (unsigned)A.nx, row = n / (unsigned)A.nx;
  const unsigned j = row % (unsigned)A.ny, k = row / (unsigned)A.ny;
  const double px = A.origin[0] + (double)i * A.spacing[0];
  const double py = A.origin[1] + (double)j * A.spacing[1];
  const double pz = A.origin[2] + (double)k * A.spacing[2];
  int f = shared ? 0 : (int)vol;
  for (; f_end - f >= TSDF_AHEAD; f += TSDF_AHEAD) tsdf_frames<POSE, TSDF_AHEAD>(A, f, px, py, pz, D, W);
  for (; f < f_end; ++f) tsdf_frames<POSE, 1>(A, f, px, py, pz, D, W);       // (the rest, and a per-frame volume's one frame)
  const bool seen = (W > 0.0f) & (D - D == 0.0f);
  A.tsdf[at] = seen ? D : __builtin_nanf("");
  A.weight[at] = seen ? W : 0.0f;
}

}  // namespace

void launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st) {
  const dim3 grid(a.chunks * (a.volume_stride == 0 ? 1u : (unsigned)a.F));
  if (a.pose) BODYFIT_LAUNCH(k_tsdf_integrate<true>, grid, dim3(256), 0, st, a);
  else BODYFIT_LAUNCH(k_tsdf_integrate<false>, grid, dim3(256), 0, st, a);
}

}  // namespace bodyfit
