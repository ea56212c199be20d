// Exact Euclidean distance transform WITH THE NEAREST SEED (a feature transform) of a batch of volumes
// (bodyfit_volume_distance_device, include/bodyfit.h: the definition, the range, the tie rule and the derivation).  Separable,
// linear in the voxels, integers only, no atomics, plain stores:
//
//   stage xy     k_edt_rows + k_edt_cols of k_edt.hip as they are, over the slices: a slice is a frame, W = nx, H = ny.  The 2-D
//                results go into the workspace: d2[v][k][j][i] (INT32_MAX in a slice without a seed) and n2 = j' nx + i'.
//   k_edt_depth  one lane per (volume, j, i) column, neighbouring lanes on neighbouring i, so every load and store of a wave is one
//                coalesced x segment.  Meijster's two scans along k with g_k = d2[k], slices without a seed skipped: the stack of
//                k_edt_cols, an entry (slice s, first slice t of its reign, g_s), entry q of a column at [q][column].
//
// What differs from k_edt_cols: there g is recomputed from the seed column; here g_s is arbitrary and is needed AFTER slice s has
// been passed on the way up (the reigning slice may lie above the one being written), so g travels in the stack entry, d2 and n2
// are read-only and the outputs are separate arrays.  The payload n2[s] is not part of the chain: it is fetched on the way up,
// for the four entries read back at a time.  As there, the top two entries live in registers on the way down and slices are
// loaded eight ahead of the dependent chain.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#include "bodyfit_device.h"
#include "edt.h"
#include "volume.h"

using namespace bodyfit;

namespace {

constexpr int kDepthThreads = 64;   // one wave per workgroup: a volume has few columns, spread them over the CUs

// plane = ny nx, the distance between the slices of a column and between the entries of its stack
__global__ __launch_bounds__(kDepthThreads) void k_edt_depth(const int32_t* __restrict__ d2, const int32_t* __restrict__ n2,
                                                             uint2* __restrict__ stack, int plane, int nz, long long n_cols,
                                                             int32_t* __restrict__ dist2, int32_t* __restrict__ nearest) {
  const long long t = (long long)blockIdx.x * kDepthThreads + threadIdx.x;
  if (t >= n_cols) return;
  const long long v = t / plane;
  const size_t base = (size_t)v * (size_t)plane * nz + (size_t)(t - v * plane);
  const int32_t* gp = d2 + base;
  uint2* sp = stack + base;
  // the top of the stack in registers as slice ts, first slice tt of its reign and tg = d2[ts], and the entry below it packed
  // as it lies in memory, while `have_below` (k_edt_cols)
  int q = -1, ts = 0, tt = 0, tg = 0;
  uint2 below = make_uint2(0u, 0u);
  bool have_below = false;
  auto set_top = [&](uint2 e) { ts = (int)(e.x & 0xffffu); tt = (int)(e.x >> 16); tg = (int)e.y; };
  auto pop = [&]() {
    if (--q < 0) return;
    if (!have_below) below = sp[(size_t)q * plane];
    set_top(below);
    have_below = false;
  };
  auto step = [&](int u, int g) {
    if (g == INT_MAX) return;                            // a slice without a seed has no parabola
    while (q >= 0) {
      const int a = tt - ts, b = tt - u;
      if (a * a + tg <= b * b + g) break;                // the top still holds the first slice of its reign (ties: the older)
      pop();
    }
    int w = 0;
    if (q >= 0) {
      // the largest x with (x - ts)^2 + tg <= (x - u)^2 + g, plus one; > tt by the loop above
      w = 1 + edt_floor_div(u * u - ts * ts + g - tg, 2 * (u - ts));
      if (w >= nz) return;
      below = make_uint2((unsigned)ts | ((unsigned)tt << 16), (unsigned)tg);
      have_below = true;
    }
    ++q;
    ts = u; tt = w; tg = g;
    sp[(size_t)q * plane] = make_uint2((unsigned)u | ((unsigned)w << 16), (unsigned)g);
  };
  int u = 0;
  for (; u + 8 <= nz; u += 8) {                          // eight independent loads in flight ahead of the dependent chain
    int g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = gp[(size_t)(u + k) * plane];
#pragma unroll
    for (int k = 0; k < 8; ++k) step(u + k, g[k]);
  }
  for (; u < nz; ++u) step(u, gp[(size_t)u * plane]);
  int32_t* dp = dist2 + base;
  int32_t* nr = nearest ? nearest + base : nullptr;
  if (q < 0) {                                           // no seed in the volume (every column sees every seed, or none)
    for (u = 0; u < nz; ++u) {
      dp[(size_t)u * plane] = INT_MAX;
      if (nr) nr[(size_t)u * plane] = -1;
    }
    return;
  }
  // up the column nothing is pushed: the next tops are fetched four at a time and their payloads right behind them, so that a
  // run of one-slice reigns (a column inside the seeds) waits for memory twice in four slices
  const int32_t* np = nr ? n2 + base : nullptr;
  auto payload = [&](uint2 e) { return np ? np[(size_t)(e.x & 0xffffu) * plane] : 0; };
  int tn = np ? np[(size_t)ts * plane] : 0;
  uint2 e0 = below, e1 = below, e2 = below, e3 = below;
  int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  int cached = 0;
  for (u = nz - 1; u >= 0; --u) {
    const int a = u - ts;
    dp[(size_t)u * plane] = a * a + tg;
    if (nr) nr[(size_t)u * plane] = ts * plane + tn;     // (s ny + j') nx + i' < nx ny nz < 2^31
    if (u == tt && --q >= 0) {
      if (cached == 0) {
        e0 = sp[(size_t)q * plane];
        if (q >= 1) e1 = sp[(size_t)(q - 1) * plane];
        if (q >= 2) e2 = sp[(size_t)(q - 2) * plane];
        if (q >= 3) e3 = sp[(size_t)(q - 3) * plane];
        p0 = payload(e0);
        if (q >= 1) p1 = payload(e1);
        if (q >= 2) p2 = payload(e2);
        if (q >= 3) p3 = payload(e3);
        cached = q >= 3 ? 4 : q + 1;
      }
      set_top(e0);
      tn = p0;
      e0 = e1; e1 = e2; e2 = e3;
      p0 = p1; p1 = p2; p2 = p3;
      --cached;
    }
  }
}

}  // namespace

void bodyfit::launch_volume_distance(const DistanceArgs& a, hipStream_t st) {
  const int plane = a.nx * a.ny;                                   // <= 2^28
  const long long n = (long long)plane * a.nz;
  const DistanceWorkspace w = distance_workspace(n, a.F);
  char* ws = static_cast<char*>(a.workspace);
  int32_t* stack = reinterpret_cast<int32_t*>(ws + w.stack);
  int32_t* d2 = reinterpret_cast<int32_t*>(ws + w.d2);
  int32_t* n2 = a.nearest ? reinterpret_cast<int32_t*>(ws + w.n2) : nullptr;
  const size_t elem = a.kind == 0 ? 1 : 4;
  for (int v0 = 0; v0 < a.F; v0 += w.group) {
    const int g = std::min(w.group, a.F - v0);
    const char* seed = static_cast<const char*>(a.seed) + (size_t)v0 * (size_t)a.seed_stride * elem;
    if (a.seed_stride == n || g == 1) {
      // dense volumes: their slices are g nz frames plane elements apart
      edt_launch(seed, a.kind, plane, g * a.nz, a.invert, a.nx, a.ny, stack, d2, n2, st);
    } else {
      for (int v = 0; v < g; ++v)
        edt_launch(seed + (size_t)v * (size_t)a.seed_stride * elem, a.kind, plane, a.nz, a.invert, a.nx, a.ny,
                   stack + (size_t)v * n * kEdtWorkspaceInts, d2 + (size_t)v * n, n2 ? n2 + (size_t)v * n : nullptr, st);
    }
    const long long n_cols = (long long)g * plane;
    BODYFIT_LAUNCH(k_edt_depth, dim3((unsigned)((n_cols + kDepthThreads - 1) / kDepthThreads)), dim3(kDepthThreads), 0, st, d2, n2,
                   reinterpret_cast<uint2*>(stack), plane, a.nz, n_cols, a.dist2 + (size_t)v0 * n,
                   a.nearest ? a.nearest + (size_t)v0 * n : nullptr);
  }
}
