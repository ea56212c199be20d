// edt.h — the exact distance transform's kernels (k_edt.hip) as the raster handle's host entry (k_raster.hip) launches them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace bodyfit {

// ints of workspace per pixel of a group of frames: the column pass's envelope stack (the row pass's seed columns pass
// through the dist2 image)
constexpr int kEdtWorkspaceInts = 2;
// pixels of the largest group of frames transformed by one pair of launches: 4 GiB of workspace (the serial chains of the
// column pass want as many columns in flight as there are; one frame is at most 16384 x 16384 = 2^28)
constexpr long long kEdtGroupPixels = 1ll << 29;

// The two passes over n_frames frames of H x W (n_frames H W <= kEdtGroupPixels), on `stream`: no allocation, no
// synchronisation, no atomics.  seed: u8 (kind 0, seed iff != 0) or int32 (kind 1, seed iff >= 0), seed_stride elements between
// frames; workspace: kEdtWorkspaceInts ints per pixel, 8-byte aligned; dist2, nearest (may be NULL): dense [n_frames][H][W].
void edt_launch(const void* seed, int kind, long long seed_stride, int n_frames, int invert, int W, int H, int32_t* workspace,
                int32_t* dist2, int32_t* nearest, hipStream_t stream);

}  // namespace bodyfit
