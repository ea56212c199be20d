// volume.h — what api_volume.hip (the host side of bodyfit_volume_sample_device and bodyfit_volume_integrate_device) launches from
// k_volume.hip and k_tsdf.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace bodyfit {

struct VolumeArgs {
  int nx, ny, nz;
  double origin[3], inv_spacing[3];    // inv_spacing: 1 / spacing, rounded once on the host
  const float* points;            // [F] stride points_stride, [N][3]
  long long points_stride, N;
  int F;
  unsigned chunks;                // workgroups per frame: ceil(N / 256); chunks F < 2^32
  const float* volume;            // [nz][ny][nx], volume_stride elements between frames (0: shared)
  long long volume_stride;
  const unsigned char* gate;      // [F][N] or null
  float* value;                   // [F][N]
  unsigned char* valid;           // [F][N]
  float* grad;                    // [F][N][3] or null
};

// one launch of k_vol_sample over the a.F a.N points (a.F, a.N > 0), on `st`
void launch_volume_sample(const VolumeArgs& a, hipStream_t st);

struct TsdfArgs {
  int nx, ny, nz;
  unsigned n_voxels, chunks;      // nx ny nz < 2^31; workgroups per volume: ceil(n_voxels / 256); chunks n_volumes < 2^31
  double origin[3], spacing[3];
  const float* depth;             // [F] stride depth_stride, [H][W]
  long long depth_stride;
  int H, W, F;
  double fx, fy, cx, cy;
  const double* pose;             // [F][12] row-major [A | t], or null: the identity
  double trunc, z_near, max_weight;
  int reset;                      // non-zero: the start state is (NaN, 0) and the buffers are not read
  float* tsdf;                    // [nz][ny][nx], volume_stride elements between the frames' volumes (0: one volume, every frame)
  float* weight;
  long long volume_stride;
};

// one launch of k_tsdf_integrate over the voxels of the one volume (a.volume_stride == 0, a.F >= 0) or of the a.F > 0 volumes, on `st`
void launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st);

}  // namespace bodyfit
