// The C ABI of the signed-distance volumes (include/bodyfit.h: bodyfit_volume_create / _destroy / _sample_device /
// _integrate_device / _surface_layout / _surface_count_device / _surface_emit_device / _distance_layout / _distance_device): the
// handle, the argument checks and the launches of each call (k_volume.hip, k_tsdf.hip, k_surface_extract.hip, k_edt3.hip through
// volume.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/bodyfit.h"
#include "host_state.h"
#include "volume.h"

struct bodyfit_volume {
  int device = 0;
  int nx = 0, ny = 0, nz = 0;
  double origin[3] = {0.0, 0.0, 0.0}, spacing[3] = {1.0, 1.0, 1.0};
};

using bodyfit::invalid_arg;

namespace {

// The checks that the two surface entries share, and the kernels' arguments but for the outputs.  *work: 1 when there is something
// to launch, 0 for the no-ops (no volumes, or an axis of length 1: no cells).
int surface_args(const char* fn, bodyfit_volume* h, const float* d_volume, const float* d_weight, long long volume_frame_stride,
                 int n_volumes, float iso, float min_weight, void* d_workspace, long long* d_offsets, bodyfit::SurfaceArgs* a,
                 int* work) {
  *work = 0;
  if (!h) return invalid_arg(fn, "handle is NULL");
  if (n_volumes < 0) return invalid_arg(fn, "negative n_volumes");
  const long long n_voxels = (long long)h->nx * h->ny * h->nz;
  if (volume_frame_stride != 0 && volume_frame_stride < n_voxels)
    return invalid_arg(fn, "volume_frame_stride is neither 0 nor >= nx ny nz");
  if (!std::isfinite(iso)) return invalid_arg(fn, "iso must be finite");
  if (std::isnan(min_weight)) return invalid_arg(fn, "min_weight is NaN");
  // at most three vertices per voxel and five triangles per cell: below 2^31 of either in one volume
  const long long n_cells = (long long)(h->nx - 1) * (h->ny - 1) * (h->nz - 1);
  if (3 * n_voxels >= (1ll << 31) || 5 * n_cells >= (1ll << 31))
    return invalid_arg(fn, "a volume that could hold 2^31 vertices or faces or more (3 nx ny nz, 5 cells)");
  if (n_volumes == 0) return BODYFIT_OK;
  if (!d_offsets) return invalid_arg(fn, "d_offsets is NULL");
  if (n_cells == 0) return BODYFIT_OK;
  if (!d_volume || !d_workspace) return invalid_arg(fn, "d_volume or d_workspace is NULL");
  const long long chunks = (n_voxels + 255) / 256;
  if (chunks * n_volumes >= (1ll << 31)) return invalid_arg(fn, "2^31 workgroups or more in one call");
  a->nx = h->nx; a->ny = h->ny; a->nz = h->nz;
  a->n_voxels = (unsigned)n_voxels; a->chunks = (unsigned)chunks; a->F = n_volumes;
  a->iso = iso; a->min_weight = min_weight;
  a->volume = d_volume; a->weight = d_weight; a->volume_stride = volume_frame_stride;
  for (int k = 0; k < 3; ++k) { a->origin[k] = h->origin[k]; a->spacing[k] = h->spacing[k]; }
  const bodyfit::SurfaceWorkspace w = bodyfit::surface_workspace(n_voxels, n_volumes);
  char* base = static_cast<char*>(d_workspace);
  a->code = reinterpret_cast<unsigned char*>(base + w.code);
  a->word = reinterpret_cast<unsigned short*>(base + w.word);
  a->block_verts = reinterpret_cast<unsigned*>(base + w.block_verts);
  a->block_tris = reinterpret_cast<unsigned*>(base + w.block_tris);
  a->totals = reinterpret_cast<unsigned*>(base + w.totals);
  a->offsets = d_offsets;
  a->vert_capacity = a->face_capacity = 0; a->verts = nullptr; a->faces = nullptr;
  *work = 1;
  return BODYFIT_OK;
}

// the checks that the two distance entries share
int distance_handle(const char* fn, bodyfit_volume* h, int n_volumes) {
  if (!h) return invalid_arg(fn, "handle is NULL");
  if (n_volumes < 0) return invalid_arg(fn, "negative n_volumes");
  if (std::max(h->nx, std::max(h->ny, h->nz)) > bodyfit::kDistanceMaxDim)
    return invalid_arg(fn, "a dimension above 16384 (the int32 range of the transform)");
  return BODYFIT_OK;
}

}  // namespace

extern "C" {

int bodyfit_volume_create(int device, int nx, int ny, int nz, const double origin[3], const double spacing[3],
                          bodyfit_volume** out) {
  const char* fn = "bodyfit_volume_create";
  if (!out) return invalid_arg(fn, "out is NULL");
  if (!origin || !spacing) return invalid_arg(fn, "origin or spacing is NULL");
  if (nx < 1 || ny < 1 || nz < 1) return invalid_arg(fn, "a dimension below 1");
  if ((long long)nx * ny >= (1ll << 31) || (long long)nx * ny * nz >= (1ll << 31)) return invalid_arg(fn, "2^31 voxels or more");
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(origin[a])) return invalid_arg(fn, "the origin must be finite");
    if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a])) return invalid_arg(fn, "the spacings must be finite and positive");
    if (!std::isnormal(1.0 / spacing[a])) return invalid_arg(fn, "a spacing whose reciprocal is not a normal f64 number");
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
  if (!h) return invalid_arg(fn, "handle is NULL");
  if (n_frames < 0 || n_points < 0) return invalid_arg(fn, "negative n_frames or n_points");
  if (n_frames == 0 || n_points == 0) return BODYFIT_OK;
  if (!d_points || !d_volume || !d_value || !d_valid) return invalid_arg(fn, "d_points, d_volume, d_value or d_valid is NULL");
  if (points_frame_stride < 3 * n_points) return invalid_arg(fn, "points_frame_stride below 3 n_points");
  if (volume_frame_stride != 0 && volume_frame_stride < (long long)h->nx * h->ny * h->nz)
    return invalid_arg(fn, "volume_frame_stride is neither 0 (shared) nor >= nx ny nz");
  if (n_points >= (1ll << 39) / n_frames) return invalid_arg(fn, "2^39 points or more in one call");
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

int bodyfit_volume_integrate_device(bodyfit_volume* h, const float* d_depth, long long depth_frame_stride, int height, int width,
                                    int n_frames, const double intr[4], const double* d_pose, double trunc, double z_near,
                                    double max_weight, int reset, float* d_tsdf, float* d_weight, long long volume_frame_stride,
                                    void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_volume_integrate_device";
  if (!h) return invalid_arg(fn, "handle is NULL");
  if (n_frames < 0) return invalid_arg(fn, "negative n_frames");
  if (height < 1 || width < 1) return invalid_arg(fn, "height or width below 1");
  if ((long long)height * width >= (1ll << 31)) return invalid_arg(fn, "2^31 pixels or more");
  if (depth_frame_stride < (long long)height * width) return invalid_arg(fn, "depth_frame_stride below height width");
  const long long n_voxels = (long long)h->nx * h->ny * h->nz;
  if (volume_frame_stride != 0 && volume_frame_stride < n_voxels)
    return invalid_arg(fn, "volume_frame_stride is neither 0 (one volume) nor >= nx ny nz");
  if (!std::isfinite(trunc) || !(trunc > 0.0)) return invalid_arg(fn, "trunc must be finite and positive");
  if (!std::isfinite(z_near) || z_near < 0.0) return invalid_arg(fn, "z_near must be finite and not negative");
  if (!(max_weight > 0.0)) return invalid_arg(fn, "max_weight must be positive (+inf: no cap)");
  if (!intr) return invalid_arg(fn, "intr is NULL");
  for (int a = 0; a < 4; ++a)
    if (!std::isfinite(intr[a])) return invalid_arg(fn, "the intrinsics must be finite");
  if (intr[0] == 0.0 || intr[1] == 0.0) return invalid_arg(fn, "fx or fy is zero");
  // what there is to do: every frame's volume, or the one volume when there is a frame to fuse or the empty state to write
  const long long n_volumes = volume_frame_stride != 0 ? n_frames : (n_frames > 0 || reset ? 1 : 0);
  if (n_volumes == 0) return BODYFIT_OK;
  if (!d_tsdf || !d_weight || (n_frames > 0 && !d_depth)) return invalid_arg(fn, "d_depth, d_tsdf or d_weight is NULL");
  const long long chunks = (n_voxels + 255) / 256;
  if (chunks * n_volumes >= (1ll << 31)) return invalid_arg(fn, "2^31 workgroups or more in one call");
  HIP_TRY(hipSetDevice(h->device));
  TsdfArgs a;
  a.nx = h->nx; a.ny = h->ny; a.nz = h->nz;
  a.n_voxels = (unsigned)n_voxels; a.chunks = (unsigned)chunks;
  for (int k = 0; k < 3; ++k) { a.origin[k] = h->origin[k]; a.spacing[k] = h->spacing[k]; }
  a.depth = d_depth; a.depth_stride = depth_frame_stride; a.H = height; a.W = width; a.F = n_frames;
  a.fx = intr[0]; a.fy = intr[1]; a.cx = intr[2]; a.cy = intr[3];
  a.pose = d_pose;
  a.trunc = trunc; a.z_near = z_near; a.max_weight = max_weight; a.reset = reset;
  a.tsdf = d_tsdf; a.weight = d_weight; a.volume_stride = volume_frame_stride;
  launch_tsdf_integrate(a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_volume_surface_layout(bodyfit_volume* h, int n_volumes, long long* workspace_bytes) {
  const char* fn = "bodyfit_volume_surface_layout";
  if (!h) return invalid_arg(fn, "handle is NULL");
  if (!workspace_bytes) return invalid_arg(fn, "workspace_bytes is NULL");
  if (n_volumes < 0) return invalid_arg(fn, "negative n_volumes");
  *workspace_bytes = bodyfit::surface_workspace((long long)h->nx * h->ny * h->nz, n_volumes).bytes;
  return BODYFIT_OK;
}

int bodyfit_volume_surface_count_device(bodyfit_volume* h, const float* d_volume, const float* d_weight, long long volume_frame_stride,
                                        int n_volumes, float iso, float min_weight, void* d_workspace, long long* d_offsets,
                                        void* stream) {
  using namespace bodyfit;
  SurfaceArgs a;
  int work = 0;
  const int rc = surface_args("bodyfit_volume_surface_count_device", h, d_volume, d_weight, volume_frame_stride, n_volumes, iso,
                              min_weight, d_workspace, d_offsets, &a, &work);
  if (rc != BODYFIT_OK) return rc;
  if (!work) {
    // no volumes, or no cells: the offsets are all zero (with no volumes and no d_offsets there is nothing to write)
    if (d_offsets) {
      HIP_TRY(hipSetDevice(h->device));
      HIP_TRY(hipMemsetAsync(d_offsets, 0, 2 * ((size_t)n_volumes + 1) * sizeof(long long), static_cast<hipStream_t>(stream)));
    }
    return BODYFIT_OK;
  }
  HIP_TRY(hipSetDevice(h->device));
  launch_surface_count(a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_volume_surface_emit_device(bodyfit_volume* h, const float* d_volume, const float* d_weight, long long volume_frame_stride,
                                       int n_volumes, float iso, float min_weight, void* d_workspace, const long long* d_offsets,
                                       long long vert_capacity, long long face_capacity, float* d_verts, int32_t* d_faces,
                                       void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_volume_surface_emit_device";
  SurfaceArgs a;
  int work = 0;
  const int rc = surface_args(fn, h, d_volume, d_weight, volume_frame_stride, n_volumes, iso, min_weight, d_workspace,
                              const_cast<long long*>(d_offsets), &a, &work);
  if (rc != BODYFIT_OK) return rc;
  if (vert_capacity < 0 || face_capacity < 0) return invalid_arg(fn, "negative vert_capacity or face_capacity");
  if (!work) return BODYFIT_OK;
  if ((vert_capacity > 0 && !d_verts) || (face_capacity > 0 && !d_faces))
    return invalid_arg(fn, "d_verts or d_faces is NULL with a capacity above 0");
  if (vert_capacity == 0 && face_capacity == 0) return BODYFIT_OK;
  a.vert_capacity = vert_capacity; a.face_capacity = face_capacity; a.verts = d_verts; a.faces = d_faces;
  HIP_TRY(hipSetDevice(h->device));
  launch_surface_emit(a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_volume_distance_layout(bodyfit_volume* h, int n_volumes, long long* workspace_bytes) {
  const char* fn = "bodyfit_volume_distance_layout";
  if (int rc = distance_handle(fn, h, n_volumes)) return rc;
  if (!workspace_bytes) return invalid_arg(fn, "workspace_bytes is NULL");
  *workspace_bytes = bodyfit::distance_workspace((long long)h->nx * h->ny * h->nz, n_volumes).bytes;
  return BODYFIT_OK;
}

int bodyfit_volume_distance_device(bodyfit_volume* h, const void* d_seed, int seed_kind, long long seed_volume_stride, int n_volumes,
                                   int invert, void* d_workspace, int32_t* d_dist2, int32_t* d_nearest, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_volume_distance_device";
  if (int rc = distance_handle(fn, h, n_volumes)) return rc;
  if (seed_kind != 0 && seed_kind != 1) return invalid_arg(fn, "seed_kind must be 0 (u8) or 1 (int32)");
  if (n_volumes == 0) return BODYFIT_OK;
  if (!d_seed || !d_dist2 || !d_workspace) return invalid_arg(fn, "d_seed, d_dist2 or d_workspace is NULL");
  if (reinterpret_cast<uintptr_t>(d_workspace) % 8 != 0) return invalid_arg(fn, "d_workspace is not 8-byte aligned");
  if (seed_volume_stride < (long long)h->nx * h->ny * h->nz) return invalid_arg(fn, "seed_volume_stride below nx ny nz");
  HIP_TRY(hipSetDevice(h->device));
  DistanceArgs a;
  a.nx = h->nx; a.ny = h->ny; a.nz = h->nz; a.F = n_volumes;
  a.seed = d_seed; a.kind = seed_kind; a.invert = invert; a.seed_stride = seed_volume_stride;
  a.workspace = d_workspace; a.dist2 = d_dist2; a.nearest = d_nearest;
  launch_volume_distance(a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
