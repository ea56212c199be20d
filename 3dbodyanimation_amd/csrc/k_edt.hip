// Exact Euclidean distance transform WITH THE NEAREST SEED (a feature transform) of a batch of masks and face-id images, on the
// raster handle's size and workspace (bodyfit_raster_distance_device, include/bodyfit.h: the definition, the tie rule and why the
// integer division is exact).
// Separable, linear in the pixels, integers only, no atomics, plain stores:
//
//   k_edt_rows   one wave per (frame, row).  The row's seeds become one 64-bit ballot per 64 columns, kept in LDS (a row of 16384
//                pixels is 256 words); a pixel's nearest seed column to the left and to the right is a count of leading / trailing
//                zeros in its own word, or the carry of the nearest non-empty word on that side.  The seed image is read once,
//                coalesced; the nearer column (ties: the left one), or -1 for a row without a seed, goes INTO THE dist2 IMAGE,
//                which the column pass reads before it overwrites it.
//   k_edt_cols   one lane per (frame, column), neighbouring lanes on neighbouring columns, so every load and store of a wave is
//                one coalesced row segment.  Meijster's two scans: down the column the lower envelope of the parabolas
//                x -> (x - i)^2 + g_i (g_i the squared horizontal distance of row i, rows without a seed skipped) is kept as a
//                stack of (row i, first row t where it is the minimum, seed column) in the workspace, entry q of column j at
//                [q][j]; up the column the envelope is read back and (dist2, nearest) written.  The top TWO entries live in
//                registers on the way down (a push is a store; only a second pop in a row loads), and the way up reads the
//                stack four entries at a time.
//
// The chain of a column is serial and its memory latency is the cost: rows are loaded eight at a time ahead of it, and a frame
// group is as large as the workspace allows so that other waves fill the waits ("Silhouette").
// The column-strip form (a strip of columns transposed through LDS, stack and all) was not built: a 1080-row column needs 12
// bytes per row of g and stack, so 160 KiB of LDS hold 12 columns, a fifth of one wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/bodyfit.h"
#include "bodyfit_device.h"
#include "edt.h"
#include "raster_handle.h"

using namespace bodyfit;

namespace {

// pixels of the largest group of frames transformed by one pair of launches: 4 GiB of workspace (the serial chains of the
// column pass want as many columns in flight as there are; one frame is at most 16384 x 16384 = 2^28)
constexpr long long kEdtGroupPixels = 1ll << 29;

constexpr int kRowWaves = 4;        // rows per workgroup of k_edt_rows
constexpr int kMaxWords = 256;      // 64-column words of the widest row (16384)
constexpr int kColThreads = 64;     // one wave per workgroup: a group of frames has few columns, spread them over the CUs

template <int KIND>
__device__ __forceinline__ bool edt_is_seed(const void* __restrict__ p, size_t at) {
  if (KIND == 0) return static_cast<const uint8_t*>(p)[at] != 0;
  return static_cast<const int32_t*>(p)[at] >= 0;
}

template <int KIND>
__global__ __launch_bounds__(64 * kRowWaves) void k_edt_rows(const void* __restrict__ seed, long long seed_stride, int W, int H,
                                                             long long n_rows, int invert, int32_t* __restrict__ col) {
  __shared__ unsigned long long s_mask[kRowWaves][kMaxWords];
  __shared__ int s_right[kRowWaves][kMaxWords];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRowWaves + wave;
  if (row >= n_rows) return;          // (a whole wave: nothing below synchronises across waves)
  const long long f = row / H;
  const int i = (int)(row - f * H);
  const size_t in = (size_t)f * (size_t)seed_stride + (size_t)i * W;
  const int n_words = (W + 63) >> 6;
  unsigned long long* mask = s_mask[wave];
  int* right = s_right[wave];
  // every lane stores the same ballot to the same word, so each lane later reads what it wrote itself
  for (int c = 0; c < n_words; ++c) {
    const int j = c * 64 + lane;
    const bool is = j < W && (edt_is_seed<KIND>(seed, in + j) != (invert != 0));
    mask[c] = __ballot(is);
  }
  int carry = -1;                     // the first seed column in the words to the right of word c
  for (int c = n_words - 1; c >= 0; --c) {
    right[c] = carry;
    const unsigned long long m = mask[c];
    if (m) carry = c * 64 + __builtin_ctzll(m);
  }
  carry = -1;                         // the last seed column in the words to the left of word c
  int32_t* out = col + (size_t)row * W;
  for (int c = 0; c < n_words; ++c) {
    const unsigned long long m = mask[c];
    const int j = c * 64 + lane;
    const unsigned long long below = m & ((2ull << lane) - 1ull);   // columns <= j (lane 63: 2 << 63 wraps to 0, all ones)
    const unsigned long long above = m >> lane;                       // columns >= j
    const int l = below ? c * 64 + 63 - __builtin_clzll(below) : carry;
    const int r = above ? j + __builtin_ctzll(above) : right[c];
    int pick;
    if (l < 0) pick = r;
    else if (r < 0) pick = l;
    else pick = (j - l <= r - j) ? l : r;
    if (j < W) out[j] = pick;
    if (m) carry = c * 64 + 63 - __builtin_clzll(m);
  }
}

// `image` holds the row pass's seed columns on entry and dist2 on exit: a column is read whole (down) before any of it is
// written (up), and no other thread touches it.
__global__ __launch_bounds__(kColThreads) void k_edt_cols(int32_t* image, uint2* __restrict__ stack, int W, int H,
                                                          long long n_cols, int32_t* __restrict__ nearest) {
  const long long t = (long long)blockIdx.x * kColThreads + threadIdx.x;
  if (t >= n_cols) return;
  const long long f = t / W;
  const int j = (int)(t - f * W);
  const size_t base = (size_t)f * (size_t)H * W + j;
  int32_t* cp = image + base;
  uint2* sp = stack + base;
  // The top of the stack lives in registers as row ts, first row tt of its reign, seed column tc and tg = (j - tc)^2, and the
  // entry below it packed as it lies in memory, while `have_below`.  The common alternation on the way down, "the new row
  // pops the top and takes its place", then touches memory with its store only; a second pop in a row loads, and waits.
  int q = -1, ts = 0, tt = 0, tc = 0, tg = 0;
  uint2 below = make_uint2(0u, 0u);
  bool have_below = false;
  auto set_top = [&](uint2 e) {
    ts = (int)(e.x & 0xffffu); tt = (int)(e.x >> 16); tc = (int)e.y;
    tg = (j - tc) * (j - tc);
  };
  auto pop = [&]() {
    if (--q < 0) return;
    if (!have_below) below = sp[(size_t)q * W];
    set_top(below);
    have_below = false;
  };
  auto step = [&](int u, int c) {
    if (c < 0) return;                                   // a row without a seed has no parabola
    const int g = (j - c) * (j - c);
    while (q >= 0) {
      const int a = tt - ts, b = tt - u;
      if (a * a + tg <= b * b + g) break;                // the top still holds the first row of its reign (ties: the older)
      pop();
    }
    int w = 0;
    if (q >= 0) {
      // the largest x with (x - ts)^2 + tg <= (x - u)^2 + g, plus one; > tt by the loop above
      w = 1 + edt_floor_div(u * u - ts * ts + g - tg, 2 * (u - ts));
      if (w >= H) return;
      below = make_uint2((unsigned)ts | ((unsigned)tt << 16), (unsigned)tc);
      have_below = true;
    }
    ++q;
    ts = u; tt = w; tc = c; tg = g;
    sp[(size_t)q * W] = make_uint2((unsigned)u | ((unsigned)w << 16), (unsigned)c);
  };
  int u = 0;
  for (; u + 8 <= H; u += 8) {                           // eight independent loads in flight ahead of the dependent chain
    int c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = cp[(size_t)(u + k) * W];
#pragma unroll
    for (int k = 0; k < 8; ++k) step(u + k, c[k]);
  }
  for (; u < H; ++u) step(u, cp[(size_t)u * W]);
  int32_t* nr = nearest ? nearest + base : nullptr;
  if (q < 0) {                                           // no seed in the frame (every column sees every seed, or none)
    for (u = 0; u < H; ++u) {
      cp[(size_t)u * W] = INT_MAX;
      if (nr) nr[(size_t)u * W] = -1;
    }
    return;
  }
  // up the column nothing is pushed: the next tops are fetched four at a time, so that a run of one-row reigns (a column
  // inside the seeds) waits for memory once in four rows
  uint2 e0 = below, e1 = below, e2 = below, e3 = below;
  int cached = have_below ? 1 : 0;
  for (u = H - 1; u >= 0; --u) {
    const int a = u - ts;
    cp[(size_t)u * W] = a * a + tg;
    if (nr) nr[(size_t)u * W] = ts * W + tc;
    if (u == tt && --q >= 0) {
      if (cached == 0) {
        e0 = sp[(size_t)q * W];
        if (q >= 1) e1 = sp[(size_t)(q - 1) * W];
        if (q >= 2) e2 = sp[(size_t)(q - 2) * W];
        if (q >= 3) e3 = sp[(size_t)(q - 3) * W];
        cached = q >= 3 ? 4 : q + 1;
      }
      set_top(e0);
      e0 = e1; e1 = e2; e2 = e3;
      --cached;
    }
  }
}

}  // namespace

// The two passes over n_frames frames of H x W (edt.h: the volume distance transform runs them over its slices too).
void bodyfit::edt_launch(const void* seed, int kind, long long seed_stride, int n_frames, int invert, int W, int H,
                         int32_t* workspace, int32_t* dist2, int32_t* nearest, hipStream_t stream) {
  const long long n_rows = (long long)n_frames * H, n_cols = (long long)n_frames * W;
  uint2* stack = reinterpret_cast<uint2*>(workspace);              // [n_frames][H][W] entries
  int32_t* col = dist2;                                            // the seed columns pass through the output image
  const dim3 rgrid((unsigned)((n_rows + kRowWaves - 1) / kRowWaves)), cgrid((unsigned)((n_cols + kColThreads - 1) / kColThreads));
  if (kind == 0)
    BODYFIT_LAUNCH(k_edt_rows<0>, rgrid, dim3(64 * kRowWaves), 0, stream, seed, seed_stride, W, H, n_rows, invert, col);
  else
    BODYFIT_LAUNCH(k_edt_rows<1>, rgrid, dim3(64 * kRowWaves), 0, stream, seed, seed_stride, W, H, n_rows, invert, col);
  BODYFIT_LAUNCH(k_edt_cols, cgrid, dim3(kColThreads), 0, stream, dist2, stack, W, H, n_cols, nearest);
}

extern "C" {

int bodyfit_raster_distance_device(bodyfit_raster* r, const void* d_seed, int seed_kind, long long seed_frame_stride,
                                   int n_frames, int invert, int32_t* d_dist2, int32_t* d_nearest, void* stream) {
  const char* fn = "bodyfit_raster_distance_device";
  if (int rc = rs_check_handle(fn, r, n_frames)) return rc;
  if (seed_kind != 0 && seed_kind != 1) return invalid_arg(fn, "seed_kind must be 0 (u8) or 1 (int32)");
  if (n_frames == 0) return BODYFIT_OK;
  if (!d_seed || !d_dist2) return invalid_arg(fn, "d_seed or d_dist2 is NULL");
  const long long ppf = (long long)r->W * r->H;
  if (seed_frame_stride < ppf) return invalid_arg(fn, "seed_frame_stride below H W");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // groups of frames that share the workspace one after the other on the stream: its size follows from (F, H, W) alone
  const int group = (int)std::max(1ll, std::min<long long>(n_frames, kEdtGroupPixels / ppf));
  if (int rc = rs_grow(&r->d_edt, &r->edtCap, (size_t)group * ppf * kEdtWorkspaceInts)) return rc;
  const size_t elem = seed_kind == 0 ? 1 : 4;
  for (int f0 = 0; f0 < n_frames; f0 += group)
    edt_launch(static_cast<const char*>(d_seed) + (size_t)f0 * seed_frame_stride * elem, seed_kind, seed_frame_stride,
               std::min(group, n_frames - f0), invert, r->W, r->H, r->d_edt, d_dist2 + (size_t)f0 * ppf,
               d_nearest ? d_nearest + (size_t)f0 * ppf : nullptr, st);
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
