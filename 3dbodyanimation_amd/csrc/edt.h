// edt.h — what k_edt3.hip (the volume distance transform's slices) shares with k_edt.hip (the 2-D distance transform).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bodyfit {

// ints of workspace per pixel of a group of frames: the column pass's envelope stack (the row pass's seed columns pass
// through the dist2 image)
constexpr int kEdtWorkspaceInts = 2;

// floor(n / d) for d > 0
__device__ __forceinline__ int edt_floor_div(int n, int d) {
  int q = n / d;
  if (n - q * d < 0) --q;
  return q;
}

// k_edt_rows and k_edt_cols over n_frames frames of H x W, on `stream`: no allocation, no synchronisation, no atomics.
// seed: u8 (kind 0, seed iff != 0) or int32 (kind 1, seed iff >= 0), seed_stride elements between frames; workspace:
// kEdtWorkspaceInts ints per pixel, 8-byte aligned; dist2, nearest (may be NULL): dense [n_frames][H][W].
void edt_launch(const void* seed, int kind, long long seed_stride, int n_frames, int invert, int W, int H, int32_t* workspace,
                int32_t* dist2, int32_t* nearest, hipStream_t stream);

}  // namespace bodyfit
