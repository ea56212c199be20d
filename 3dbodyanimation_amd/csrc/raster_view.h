// What another translation unit may know of a bodyfit_raster (k_raster.hip keeps the handle itself): its device, its topology
// and its size.  k_texture.hip's entries take the handle and read it through this.
#pragma once
#include "../../include/bodyfit.h"

namespace bodyfit {

struct RasterView {
  int device, nV, nF, W, H;
  const int* d_faces;      // [n_faces][3], device
  unsigned* d_scratch;     // one u32 on the device that a call may use between its own kernels (calls on one handle are ordered)
};

RasterView raster_view(const bodyfit_raster* r);

}  // namespace bodyfit
