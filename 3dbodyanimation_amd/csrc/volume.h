// volume.h — what api_volume.hip (the host side of bodyfit_volume_sample_device) launches from k_volume.hip.
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

}  // namespace bodyfit
