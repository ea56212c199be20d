// Signed-distance volumes: a batch of scalar f32 volumes read trilinearly at the points of a cloud, with the exact spatial gradient
// of the cell's patch in world units (bodyfit_volume_sample_device; include/bodyfit.h: the definition, the contract and the
// derivation of its constants; the host entry: api_volume.hip).
//
//   k_vol_sample<GRAD>  one thread per (frame, point), a workgroup inside one frame: the grid coordinates in f64, the cell
//                (trilinear_inl.h), its eight voxels (gathered before anything is combined: the gathers are what this kernel waits
//                for), the finiteness of the eight, the value and the patch's derivative over the spacing.  Unfused f64; only the
//                stores round.  Plain stores.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "bodyfit_device.h"
#include "trilinear_inl.h"
#include "volume.h"

#pragma clang fp contract(off)

namespace bodyfit {

namespace {

template <bool GRAD>
__global__ __launch_bounds__(256) void k_vol_sample(const VolumeArgs A) {
  // a workgroup never straddles two frames: the frame, and with it the bases of its points and of its volume, is wave-uniform
  // (one 32-bit scalar division per wave, none per lane)
  const unsigned frame = blockIdx.x / A.chunks;
  const long long n = (long long)(blockIdx.x - frame * A.chunks) * 256 + threadIdx.x;
  if (n >= A.N) return;
  const size_t p = (size_t)frame * (size_t)A.N + (size_t)n;
  const float* x = A.points + (size_t)frame * (size_t)A.points_stride + 3 * (size_t)n;
  const float X = x[0], Y = x[1], Z = x[2];
  const unsigned char gate = A.gate ? A.gate[p] : 1;       // (with the point's load in flight, not behind it)
  // (& and not &&: one test of the lanes, not a branch per comparison)
  bool ok = (X - X == 0.0f) & (Y - Y == 0.0f) & (Z - Z == 0.0f) & (gate != 0);
  double val = 0.0, g[3] = {0.0, 0.0, 0.0};
  if (ok) {
    // (the product with the handle's 1 / spacing, not a quotient: one rounding more, inside the contract's delta, and no f64
    //  division per lane)
    const double gx = ((double)X - A.origin[0]) * A.inv_spacing[0];
    const double gy = ((double)Y - A.origin[1]) * A.inv_spacing[1];
    const double gz = ((double)Z - A.origin[2]) * A.inv_spacing[2];
    ok = (gx >= 0.0) & (gx <= (double)(A.nx - 1)) & (gy >= 0.0) & (gy <= (double)(A.ny - 1)) & (gz >= 0.0) &
         (gz <= (double)(A.nz - 1));
    if (ok) {
      const TrilinearCell cell = trilinear_cell(gx, gy, gz, A.nx, A.ny, A.nz);
      float t[8];
      trilinear_gather(A.volume + (size_t)frame * (size_t)A.volume_stride, A.nx, A.ny, cell, t);
      ok = trilinear_finite(t);
      if (ok) {
        trilinear_patch<GRAD>(t, cell, &val, g);
        if (GRAD) { g[0] = g[0] * A.inv_spacing[0]; g[1] = g[1] * A.inv_spacing[1]; g[2] = g[2] * A.inv_spacing[2]; }
      }
    }
  }
  A.valid[p] = ok ? 1 : 0;
  A.value[p] = (float)val;
  if (GRAD) {
    float* out = A.grad + 3 * p;
    out[0] = (float)g[0]; out[1] = (float)g[1]; out[2] = (float)g[2];
  }
}

}  // namespace

void launch_volume_sample(const VolumeArgs& a, hipStream_t st) {
  const dim3 grid(a.chunks * (unsigned)a.F);
  if (a.grad) BODYFIT_LAUNCH(k_vol_sample<true>, grid, dim3(256), 0, st, a);
  else BODYFIT_LAUNCH(k_vol_sample<false>, grid, dim3(256), 0, st, a);
}

}  // namespace bodyfit
