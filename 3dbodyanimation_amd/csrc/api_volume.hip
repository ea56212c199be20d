// The C ABI of the signed-distance volumes (include/bodyfit.h: bodyfit_volume_create / _destroy / _sample_device): the handle, the
// argument checks and the one launch (k_volume.hip through volume.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/bodyfit.h"
#include "host_state.h"
#include "volume.h"

struct bodyfit_volume {
  int device = 0;
  int nx = 0, ny = 0, nz = 0;
  double origin[3] = {0.0, 0.0, 0.0}, spacing[3] = {1.0, 1.0, 1.0};
};

namespace {
int vol_invalid(const char* fn, const char* what) {
  return bodyfit_internal_fail(BODYFIT_ERR_INVALID, (std::string(fn) + ": " + what).c_str());
}
}  // namespace

extern "C" {

int bodyfit_volume_create(int device, int nx, int ny, int nz, const double origin[3], const double spacing[3],
                          bodyfit_volume** out) {
  const char* fn = "bodyfit_volume_create";
  if (!out) return vol_invalid(fn, "out is NULL");
  if (!origin || !spacing) return vol_invalid(fn, "origin or spacing is NULL");
  if (nx < 1 || ny < 1 || nz < 1) return vol_invalid(fn, "a dimension below 1");
  if ((long long)nx * ny >= (1ll << 31) || (long long)nx * ny * nz >= (1ll << 31)) return vol_invalid(fn, "2^31 voxels or more");
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(origin[a])) return vol_invalid(fn, "the origin must be finite");
    if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a])) return vol_invalid(fn, "the spacings must be finite and positive");
    if (!std::isnormal(1.0 / spacing[a])) return vol_invalid(fn, "a spacing whose reciprocal is not a normal f64 number");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return bodyfit_internal_fail(BODYFIT_ERR_HIP, "bodyfit_volume_create: no such HIP device (there is no CPU path)");
  auto* h = new bodyfit_volume;
  h->device = device; h->nx = nx; h->ny = ny; h->nz = nz;
  for (int a = 0; a < 3; ++a) { h->origin[a] = origin[a]; h->spacing[a] = spacing[a]; }
  *out = h;
  return BODYFIT_OK;
}

void bodyfit_volume_destroy(bodyfit_volume* h) { delete h; }

int bodyfit_volume_sample_device(bodyfit_volume* h, const float* d_points, long long points_frame_stride, long long n_points,
                                 int n_frames, const float* d_volume, long long volume_frame_stride, const uint8_t* d_gate,
                                 float* d_value, uint8_t* d_valid, float* d_grad, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_volume_sample_device";
  if (!h) return vol_invalid(fn, "handle is NULL");
  if (n_frames < 0 || n_points < 0) return vol_invalid(fn, "negative n_frames or n_points");
  if (n_frames == 0 || n_points == 0) return BODYFIT_OK;
  if (!d_points || !d_volume || !d_value || !d_valid) return vol_invalid(fn, "d_points, d_volume, d_value or d_valid is NULL");
  if (points_frame_stride < 3 * n_points) return vol_invalid(fn, "points_frame_stride below 3 n_points");
  if (volume_frame_stride != 0 && volume_frame_stride < (long long)h->nx * h->ny * h->nz)
    return vol_invalid(fn, "volume_frame_stride is neither 0 (shared) nor >= nx ny nz");
  if (n_points >= (1ll << 39) / n_frames) return vol_invalid(fn, "2^39 points or more in one call");
  HIP_TRY(hipSetDevice(h->device));
  VolumeArgs a;
  a.nx = h->nx; a.ny = h->ny; a.nz = h->nz;
  for (int k = 0; k < 3; ++k) { a.origin[k] = h->origin[k]; a.inv_spacing[k] = 1.0 / h->spacing[k]; }
  a.points = d_points; a.points_stride = points_frame_stride; a.N = n_points; a.F = n_frames;
  a.chunks = (unsigned)((n_points + 255) / 256);      // (n_points n_frames < 2^39: chunks n_frames < 2^31 + n_frames < 2^32)
  a.volume = d_volume; a.volume_stride = volume_frame_stride;
  a.gate = d_gate; a.value = d_value; a.valid = d_valid; a.grad = d_grad;
  launch_volume_sample(a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
