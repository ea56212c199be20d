// volume.h — what api_volume.hip (the host side of bodyfit_volume_sample_device, bodyfit_volume_integrate_device,
// bodyfit_volume_surface_* and bodyfit_volume_distance_*) launches from k_volume.hip, k_tsdf.hip, k_surface_extract.hip and
// k_edt3.hip.
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


struct SurfaceArgs {
  int nx, ny, nz;
  unsigned n_voxels, chunks;      // nx ny nz < 2^31 / 3; workgroups per volume: ceil(n_voxels / 256); chunks F < 2^31
  int F;                          // volumes
  float iso, min_weight;
  const float* volume;            // [nz][ny][nx], volume_stride elements between the volumes
  const float* weight;            // the same shape, or null
  long long volume_stride;
  double origin[3], spacing[3];
  // the workspace (surface_workspace: bodyfit_volume_surface_layout)
  unsigned char* code;            // [F][n_voxels]: the cell whose corner 0 the voxel is: its case, 0 when dead or not a cell
  unsigned short* word;           // [F][n_voxels]: edge flags x, y, z << 13 | the exclusive vertex offset inside the workgroup
  unsigned* block_verts;          // [F][chunks]: a workgroup's vertices; after k_mc_scan: exclusive inside the volume
  unsigned* block_tris;           // [F][chunks]: a workgroup's triangles, alike
  unsigned* totals;               // [F][2]: a volume's vertices and triangles
  long long* offsets;             // the caller's [2][F + 1]
  // k_mc_emit only
  long long vert_capacity, face_capacity;
  float* verts;                   // [.][3]
  int* faces;                     // [.][3]
};

// the byte offsets of the workspace's arrays for F volumes of n_voxels voxels, and its size
struct SurfaceWorkspace { long long code, word, block_verts, block_tris, totals, bytes; };
inline SurfaceWorkspace surface_workspace(long long n_voxels, long long F) {
  const long long chunks = (n_voxels + 255) / 256;
  auto up = [](long long b) { return (b + 255) / 256 * 256; };
  SurfaceWorkspace w;
  w.code = 0;
  w.word = w.code + up(F * n_voxels);
  w.block_verts = w.word + up(2 * F * n_voxels);
  w.block_tris = w.block_verts + up(4 * F * chunks);
  w.totals = w.block_tris + up(4 * F * chunks);
  w.bytes = w.totals + up(8 * F);
  return w;
}

// bodyfit_volume_surface_count_device: k_mc_classify, k_mc_count, k_mc_scan and k_mc_offsets over the a.F > 0 volumes, on `st`
void launch_surface_count(const SurfaceArgs& a, hipStream_t st);
// bodyfit_volume_surface_emit_device: k_mc_emit
void launch_surface_emit(const SurfaceArgs& a, hipStream_t st);


struct DistanceArgs {
  int nx, ny, nz;                 // each <= kDistanceMaxDim
  int F;                          // volumes
  const void* seed;               // u8 (kind 0, seed iff != 0) or int32 (kind 1, seed iff >= 0), seed_stride elements between volumes
  int kind, invert;
  long long seed_stride;
  void* workspace;                // distance_workspace(nx ny nz, F).bytes, 8-byte aligned
  int* dist2;                     // [F][nz][ny][nx]
  int* nearest;                   // the same shape, or null
};

constexpr int kDistanceMaxDim = 16384;
// voxels of the largest group of volumes transformed by one round of launches: 16 bytes each, 4 GiB of workspace (a single
// larger volume is a group of its own)
constexpr long long kDistanceGroupVoxels = 1ll << 28;

// the byte offsets of the workspace's arrays for F volumes of n_voxels voxels, its size, and the volumes per group: the envelope
// stack that the xy and the z stage share (8 bytes per voxel), then the slices' 2-D results d2 and n2 (4 each)
struct DistanceWorkspace { long long stack, d2, n2, bytes; int group; };
inline DistanceWorkspace distance_workspace(long long n_voxels, long long F) {
  DistanceWorkspace w;
  long long group = kDistanceGroupVoxels / n_voxels;
  group = group < 1 ? 1 : group;
  group = group > F ? F : group;
  w.group = (int)group;
  w.stack = 0;
  w.d2 = 8 * group * n_voxels;
  w.n2 = w.d2 + 4 * group * n_voxels;
  w.bytes = w.n2 + 4 * group * n_voxels;
  return w;
}

// bodyfit_volume_distance_device: k_edt_rows, k_edt_cols over the slices and k_edt_depth over the columns of the a.F > 0 volumes,
// group after group on `st`
void launch_volume_distance(const DistanceArgs& a, hipStream_t st);

}  // namespace bodyfit
