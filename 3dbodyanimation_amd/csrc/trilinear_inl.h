// The trilinear patch of a scalar f32 volume [nz][ny][nx] (x fastest) and its exact derivative: the 3-D counterpart of
// bilinear_inl.h, used by the volume sampler (k_vol_sample, k_volume.hip).  f64 and unfused: every function switches contraction
// off for its own body.  The definitions and their error bounds: include/bodyfit.h (bodyfit_volume_sample_device).
#pragma once
#include <hip/hip_runtime.h>

namespace bodyfit {

// The cell of the grid coordinates (gx, gy, gz), 0 <= g_a <= n_a - 1 on every axis (the CALLER has tested that in f64: the
// conversions below are then defined): i0 = min(floor(gx), max(nx - 2, 0)), i1 = min(i0 + 1, nx - 1), a = gx - i0 (exact), and
// (j0, j1, b) in y, (k0, k1, c) in z alike: bilinear_cell's rule on three axes.
struct TrilinearCell {
  int i0, i1, j0, j1, k0, k1;
  double a, b, c;
};

__device__ __forceinline__ TrilinearCell trilinear_cell(double gx, double gy, double gz, int nx, int ny, int nz) {
#pragma clang fp contract(off)
  TrilinearCell q;
  q.i0 = min((int)floor(gx), max(nx - 2, 0)); q.i1 = min(q.i0 + 1, nx - 1);
  q.j0 = min((int)floor(gy), max(ny - 2, 0)); q.j1 = min(q.j0 + 1, ny - 1);
  q.k0 = min((int)floor(gz), max(nz - 2, 0)); q.k1 = min(q.k0 + 1, nz - 1);
  q.a = gx - (double)q.i0; q.b = gy - (double)q.j0; q.c = gz - (double)q.k0;
  return q;
}

// The cell's eight voxels, t[4 dk + 2 dj + di] = vol[k_dk][j_dj][i_di]: eight independent loads and nothing else, so that all of
// them are in flight before the first is used.  The voxel count is below 2^31 (bodyfit_volume_create): 32-bit indices.
__device__ __forceinline__ void trilinear_gather(const float* __restrict__ vol, int nx, int ny, const TrilinearCell& q, float t[8]) {
  const int r00 = (q.k0 * ny + q.j0) * nx, r01 = (q.k0 * ny + q.j1) * nx;
  const int r10 = (q.k1 * ny + q.j0) * nx, r11 = (q.k1 * ny + q.j1) * nx;
  t[0] = vol[r00 + q.i0]; t[1] = vol[r00 + q.i1];
  t[2] = vol[r01 + q.i0]; t[3] = vol[r01 + q.i1];
  t[4] = vol[r10 + q.i0]; t[5] = vol[r10 + q.i1];
  t[6] = vol[r11 + q.i0]; t[7] = vol[r11 + q.i1];
}

// every one of the eight is finite (x - x is NaN for an infinity, and a NaN fails the comparison)
__device__ __forceinline__ bool trilinear_finite(const float t[8]) {
  bool ok = true;
#pragma unroll
  for (int n = 0; n < 8; ++n) ok = ok && (t[n] - t[n] == 0.0f);
  return ok;
}

// value and, when GRAD, (d/dgx, d/dgy, d/dgz) of the cell's patch, in GRID units (the caller divides by the spacing)
template <bool GRAD>
__device__ __forceinline__ void trilinear_patch(const float t[8], const TrilinearCell& q, double* __restrict__ val,
                                                double* __restrict__ g) {
#pragma clang fp contract(off)
  double V[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) V[n] = (double)t[n];
  const double a = q.a, b = q.b, c = q.c;
  const double na = 1.0 - a, nb = 1.0 - b, nc = 1.0 - c;
  const double w00 = nb * nc, w01 = b * nc, w10 = nb * c, w11 = b * c;      // (the y z weights: w[dk][dj])
  *val = (((na * w00) * V[0] + (a * w00) * V[1]) + ((na * w01) * V[2] + (a * w01) * V[3])) +
         (((na * w10) * V[4] + (a * w10) * V[5]) + ((na * w11) * V[6] + (a * w11) * V[7]));
  if (GRAD) {
    g[0] = (w00 * (V[1] - V[0]) + w01 * (V[3] - V[2])) + (w10 * (V[5] - V[4]) + w11 * (V[7] - V[6]));
    g[1] = ((na * nc) * (V[2] - V[0]) + (a * nc) * (V[3] - V[1])) + ((na * c) * (V[6] - V[4]) + (a * c) * (V[7] - V[5]));
    g[2] = ((na * nb) * (V[4] - V[0]) + (a * nb) * (V[5] - V[1])) + ((na * b) * (V[6] - V[2]) + (a * b) * (V[7] - V[3]));
  }
}

}  // namespace bodyfit
