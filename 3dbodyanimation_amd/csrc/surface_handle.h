// surface_handle.h — the bodyfit_surface handle, shared by the translation units that work on it: k_closest_surface.hip (create,
// destroy, the searches and their VJP), api_gram.hip (the Gauss-Newton normal equations at a fixed correspondence) and
// k_winding.hip (winding numbers and vertex normals).
#pragma once
#include "closest_group_inl.h"

struct bodyfit_surface {
  bodyfit::ClosestWorkspace w;
  int n_verts = 0, n_faces = 0;
  int* d_faces = nullptr;      // [n_faces][3]
  int* d_csr_off = nullptr;    // [n_verts + 1]
  int* d_csr_fc = nullptr;     // [3 n_faces]
  char* rec = nullptr;         // the prepared records of the last search
  size_t rec_bytes = 0;
  char* acc = nullptr;         // per-face corner sums of a backward
  size_t acc_bytes = 0;
  char* gram = nullptr;        // bodyfit_surface_gram_device: moments, mixed rows and partial panels of one group of frames
  size_t gram_bytes = 0;
};

namespace {

// the faces as a uniform "reference set" of n_faces rows per frame: what the grouping counts rows of
inline bodyfit_pointset face_rows(const bodyfit_surface* s) { return bodyfit_pointset{nullptr, nullptr, s->n_faces, 3LL * s->n_faces}; }

}  // namespace
