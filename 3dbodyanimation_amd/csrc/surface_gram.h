// surface_gram.h — what api_gram.hip (the host side of bodyfit_surface_gram_device) launches from k_surface_gram.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bodyfit {

constexpr int kGramTile = 32;        // tangents per panel tile: the MFMA rows and columns
constexpr int kGramSlice = 256;      // floats of the contracted index (3 V) per partial panel: 16 MFMA k-steps
constexpr int kGramFrames = 16;      // frames that share the handle's moments, mixed rows and partial panels at a time
constexpr int kGramMaxTangents = 4096;

struct GramArgs {
  int f0, nf;                  // frames f0 .. f0 + nf - 1 of the call, nf <= kGramFrames
  int n_faces, n_verts, P;
  int plane;                   // 0: isotropic (point-to-point), 1: a unit direction per row
  const int* faces;            // [n_faces][3]
  const int *csr_off, *csr_fc; // vertex -> 3 face + corner, ascending
  const int *cnt, *start, *sorted;   // the grouping of the rows by face, over all frames of the call
  const float *bary, *weight, *dir;  // packed rows; weight / dir may be null
  const float* jac;            // [F][P][row_floats]
  long long row_floats, jac_stride;
  float* mom;                  // [nf][n_faces][6 or 36]
  float* mixed;                // [nf][P][3 V]
  float* part;                 // [nf][n_slices][n_pairs][32][32]
  double* H;                   // [F][P][P]
};

inline int gram_moment_floats(int plane) { return plane ? 36 : 6; }
inline int gram_tiles(int P) { return (P + kGramTile - 1) / kGramTile; }
inline int gram_pairs(int P) { return gram_tiles(P) * (gram_tiles(P) + 1) / 2; }
inline int gram_slices(int n_verts) { return (3 * n_verts + kGramSlice - 1) / kGramSlice; }

// moments, the mix Y = W J, the contraction and the f64 fold of the partial panels, for the frames of `a`, in that order on `st`
void launch_gram_frames(const GramArgs& a, hipStream_t st);
// g[f][p] = sum_k J[f][p][k] rhs[f][k], k < 3 V, for every frame
void launch_gram_rhs(const float* jac, long long row_floats, long long jac_stride, const float* rhs, long long rhs_stride, int F,
                     int P, int n_verts, double* g, hipStream_t st);

}  // namespace bodyfit
