// The bilinear patch of an interleaved image and its exact derivative: the ONE statement of it, used by the image sampler
// (k_rs_sample, k_raster_shade.hip) and by the texture lookup and its gradient (k_texture.hip).  f64 and unfused: every function
// switches contraction off for its own body, so it does not matter where an includer puts its own pragma.  The definitions and
// their error bounds: include/bodyfit.h (bodyfit_raster_sample_device).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bodyfit {

// The cell of (u, v), 0 <= u <= W - 1 and 0 <= v <= H - 1 (the CALLER has clamped or tested in f64: the conversions below are
// then defined): j0 = min(floor(u), max(W - 2, 0)), j1 = min(j0 + 1, W - 1), a = u - j0 (exact), and i0, i1, b alike.
struct BilinearCell {
  int i0, i1, j0, j1;
  double a, b;
};

__device__ __forceinline__ BilinearCell bilinear_cell(double u, double v, int W, int H) {
#pragma clang fp contract(off)
  BilinearCell k;
  k.j0 = min((int)floor(u), max(W - 2, 0)); k.j1 = min(k.j0 + 1, W - 1);
  k.i0 = min((int)floor(v), max(H - 2, 0)); k.i1 = min(k.i0 + 1, H - 1);
  k.a = u - (double)k.j0; k.b = v - (double)k.i0;
  return k;
}

// The four weights of the cell's texels (i0, j0), (i0, j1), (i1, j0), (i1, j1): one product each.
__device__ __forceinline__ void bilinear_weights(const BilinearCell& k, double w[4]) {
#pragma clang fp contract(off)
  const double na = 1.0 - k.a, nb = 1.0 - k.b;
  w[0] = na * nb; w[1] = k.a * nb; w[2] = na * k.b; w[3] = k.a * k.b;
}

// value, d/du and d/dv of the patch for C interleaved channels of T texels (used as they are).  All 4 C texels are loaded before
// anything is combined: the gathers are what the callers wait for.  gu / gv may be nullptr (a compile-time fact at the call).
template <int C, typename T>
__device__ __forceinline__ void bilinear_patch(const T* __restrict__ img, int W, const BilinearCell& k, double* __restrict__ val,
                                               double* __restrict__ gu, double* __restrict__ gv) {
#pragma clang fp contract(off)
  const T* r0 = img + ((size_t)k.i0 * W) * C;
  const T* r1 = img + ((size_t)k.i1 * W) * C;
  T t00[C], t01[C], t10[C], t11[C];
  for (int c = 0; c < C; ++c) {
    t00[c] = r0[(size_t)k.j0 * C + c]; t01[c] = r0[(size_t)k.j1 * C + c];
    t10[c] = r1[(size_t)k.j0 * C + c]; t11[c] = r1[(size_t)k.j1 * C + c];
  }
  const double a = k.a, b = k.b;
  const double na = 1.0 - a, nb = 1.0 - b;
  for (int c = 0; c < C; ++c) {
    const double I00 = (double)t00[c], I01 = (double)t01[c], I10 = (double)t10[c], I11 = (double)t11[c];
    val[c] = ((na * nb) * I00 + (a * nb) * I01) + ((na * b) * I10 + (a * b) * I11);
    if (gu) gu[c] = nb * (I01 - I00) + b * (I11 - I10);
    if (gv) gv[c] = na * (I10 - I00) + a * (I11 - I01);
  }
}

}  // namespace bodyfit
