// api_gram.hip — bodyfit_surface_gram_device of the C ABI in include/bodyfit.h: the checks, the grouping of the rows by face (the
// handle's, as bodyfit_closest_surface_vjp_device takes it), the handle's workspace and the loop over groups of kGramFrames frames.
// The kernels are in k_surface_gram.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "surface_gram.h"
#include "surface_handle.h"

extern "C" {

int bodyfit_surface_gram_device(bodyfit_surface* s, const bodyfit_pointset* query, int n_frames, long long n_query_total,
                                const int32_t* d_index, const float* d_bary, const float* d_weight, const float* d_direction,
                                const float* d_jac, int n_tangents, long long row_floats, long long jac_frame_stride,
                                const float* d_rhs, long long rhs_frame_stride, double* d_H, double* d_g, void* stream) {
  using namespace bodyfit;
  const char* fn = "bodyfit_surface_gram_device";
  if (n_frames < 0) return invalid(fn, "negative n_frames");
  if (int rc = check_set(fn, "query", query, n_frames, &n_query_total)) return rc;
  if (!s) return invalid(fn, "null handle");
  if (!d_index || !d_bary) return invalid(fn, "d_index / d_bary is NULL");
  if (!d_jac || !d_H) return invalid(fn, "d_jac / d_H is NULL");
  if (n_tangents < 1) return invalid(fn, "n_tangents < 1");
  if (n_tangents > kGramMaxTangents) return invalid(fn, "more than 4096 tangents");
  if (row_floats < 3LL * s->n_verts) return invalid(fn, "row_floats < 3 V");
  if (jac_frame_stride < (long long)n_tangents * row_floats) return invalid(fn, "jac_frame_stride < n_tangents row_floats");
  if (d_g && !d_rhs) return invalid(fn, "d_g needs d_rhs");
  if (d_rhs && rhs_frame_stride < 3LL * s->n_verts) return invalid(fn, "rhs_frame_stride < 3 V");
  const long long n_rows = (long long)n_frames * s->n_faces;
  if (n_rows >= (1LL << 31) - 4096 || (long long)n_frames * n_tangents >= (1LL << 31) || 3LL * s->n_verts >= (1LL << 31) - 4096)
    return invalid(fn, "more than 2^31 faces, tangents or coordinates over the frames");
  // the contraction's grid and the partial panels of one group of frames: n_pairs n_slices tiles of 4 KiB per frame
  if ((long long)gram_pairs(n_tangents) * gram_slices(s->n_verts) >= (1LL << 31) / (kGramTile * kGramTile * 4))
    return invalid(fn, "n_tangents^2 x n_verts too large: more than 2^31 bytes of partial panels per frame");
  if (n_frames == 0) return BODYFIT_OK;
  HIP_TRY(hipSetDevice(s->w.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int P = n_tangents, V = s->n_verts;
  if (d_g) {
    if (V > 0) launch_gram_rhs(d_jac, row_floats, jac_frame_stride, d_rhs, rhs_frame_stride, n_frames, P, V, d_g, st);
    else HIP_TRY(hipMemsetAsync(d_g, 0, (size_t)n_frames * P * sizeof(double), st));
  }
  if (n_query_total == 0 || n_rows == 0 || V == 0) {       // no row can contribute: exact zeros
    HIP_TRY(hipMemsetAsync(d_H, 0, (size_t)n_frames * P * P * sizeof(double), st));
    HIP_TRY(hipGetLastError());
    return BODYFIT_OK;
  }
  const bodyfit_pointset fr = face_rows(s);
  Grouping* g = nullptr;
  if (int rc = kept_or_built_grouping(&s->w, query, &fr, n_frames, n_query_total, n_rows, d_index, st, &g)) return rc;
  GramArgs a{};
  a.n_faces = s->n_faces; a.n_verts = V; a.P = P;
  a.plane = d_direction ? 1 : 0;
  a.faces = s->d_faces; a.csr_off = s->d_csr_off; a.csr_fc = s->d_csr_fc;
  a.cnt = g->cnt; a.start = g->start; a.sorted = g->sorted;
  a.bary = d_bary; a.weight = d_weight; a.dir = d_direction;
  a.jac = d_jac; a.row_floats = row_floats; a.jac_stride = jac_frame_stride;
  a.H = d_H;
  // one group of frames in the handle: [moments | mixed rows | partial panels]
  const int nfb = std::min(n_frames, kGramFrames);
  const size_t b_mom = align256((size_t)nfb * s->n_faces * gram_moment_floats(a.plane) * 4);
  const size_t b_mix = align256((size_t)nfb * P * 3 * (size_t)V * 4);
  const size_t b_part = align256((size_t)nfb * gram_slices(V) * gram_pairs(P) * (kGramTile * kGramTile) * 4);
  if (int rc = reserve(&s->gram, &s->gram_bytes, b_mom + b_mix + b_part)) return rc;
  a.mom = reinterpret_cast<float*>(s->gram);
  a.mixed = reinterpret_cast<float*>(s->gram + b_mom);
  a.part = reinterpret_cast<float*>(s->gram + b_mom + b_mix);
  for (int f0 = 0; f0 < n_frames; f0 += kGramFrames) {     // (the groups follow one another on the stream: they share the buffers)
    a.f0 = f0; a.nf = std::min(kGramFrames, n_frames - f0);
    launch_gram_frames(a, st);
  }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

}  // extern "C"
