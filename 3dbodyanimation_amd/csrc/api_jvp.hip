// api_jvp.hip — forward mode of the C ABI in include/bodyfit.h: the forward's multi-tangent JVP (k_forward_jvp.hip) as a device
// entry point and a host wrapper.
#include "host_state.h"

#include <algorithm>
#include <string>

using namespace bodyfit;

extern "C" {

namespace {

// the problem's JVP buffers, once (first JVP with a cloud tangent): its own mesh operands (so an evaluation's and the VJP's are
// left alone), the primal blended vertices, and ONE 32-tangent tile per frame of transform tangents and coefficient fragments.
// The clears are enqueued on the caller's stream `st`, in front of the launches that follow them there: a clear on the NULL
// stream is not ordered against a non-blocking stream, and need not have completed when hipMemset returns.
int jvp_problem_ready(bodyfit_problem* p, hipStream_t st) {
  if (p->jvp_alloc) return BODYFIT_OK;
  const bodyfit_model* m = p->m;
  const int F = p->d.F, nFT = p->d.nFTiles, nVT = m->d.nVTiles;
  const size_t nfa = (size_t)nFT * kBlendKSteps * 2 * 64 * 8, nsk = (size_t)nFT * kFTile * m->nJ * 12;
  HIP_TRY(p->mem.alloc(&p->jvp_mc.featA, nfa));
  HIP_TRY(p->mem.alloc(&p->jvp_mc.skinT, nsk));
  HIP_TRY(hipMemsetAsync(p->jvp_mc.featA, 0, nfa * sizeof(uint16_t), st));
  HIP_TRY(hipMemsetAsync(p->jvp_mc.skinT, 0, nsk * sizeof(float), st));
  HIP_TRY(p->mem.alloc(&p->jvp_r, (size_t)std::max(1, p->lay.reproj_rows)));
  HIP_TRY(p->mem.alloc(&p->jvp_joints, (size_t)F * m->nJ * 3));
  HIP_TRY(p->mem.alloc(&p->jvp_bbuf, jvp_bbuf_elems(F, nVT)));
  HIP_TRY(p->mem.alloc(&p->jvp_tdot, jvp_tdot_elems(F)));
  HIP_TRY(p->mem.alloc(&p->jvp_featD, jvp_feat_elems(F)));
  HIP_TRY(p->mem.alloc(&p->jvp_dbuf, jvp_dbuf_elems(F, nVT)));
  HIP_TRY(hipMemsetAsync(p->jvp_bbuf, 0, jvp_bbuf_elems(F, nVT) * sizeof(float), st));
  HIP_TRY(hipMemsetAsync(p->jvp_tdot, 0, jvp_tdot_elems(F) * sizeof(float), st));
  HIP_TRY(hipMemsetAsync(p->jvp_featD, 0, jvp_feat_elems(F) * sizeof(uint16_t), st));
  p->jvp_alloc = true;
  return BODYFIT_OK;
}

}  // namespace

int bodyfit_forward_jvp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, int n_tangents,
                               const double* d_tan_params, const double* d_tan_beta, double* d_tan_joints, float* d_tan_cloud,
                               long long row_floats, void* stream) {
  return bodyfit_forward_offsets_jvp_device(p, d_frame_params, d_beta, nullptr, 0, n_tangents, d_tan_params, d_tan_beta,
                                            d_tan_joints, d_tan_cloud, row_floats, stream);
}

int bodyfit_forward_offsets_jvp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                                       const float* d_offsets, long long offsets_frame_stride, int n_tangents,
                                       const double* d_tan_params, const double* d_tan_beta, double* d_tan_joints,
                                       float* d_tan_cloud, long long row_floats, void* stream) {
  if (!p || !d_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  if (d_offsets)
    if (int rc = check_offsets(p, offsets_frame_stride)) return rc;
  if (n_tangents < 1) return fail(BODYFIT_ERR_INVALID, "n_tangents < 1");
  if (!d_tan_joints && !d_tan_cloud) return fail(BODYFIT_ERR_INVALID, "both outputs are NULL");
  const bodyfit_model* m = p->m;
  if (d_tan_cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "tan_cloud needs a problem created with want_mesh");
  if (d_tan_cloud && row_floats < 3LL * m->V) return fail(BODYFIT_ERR_INVALID, "row_floats < 3 V");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool has_beta = dims(p).has_beta;
  const double* d_b = has_beta ? d_beta : nullptr;
  const double* d_tb = has_beta ? d_tan_beta : nullptr;
  const int per_frame = p->desc.beta_per_frame != 0, K = n_tangents;
  const bool mesh = d_tan_cloud != nullptr;
  if (mesh)
    if (int rc = jvp_problem_ready(p, st)) return rc;
  p->async_stream = st;
  p->async_pending = true;
  const int n_tiles = (K + 31) / 32;
  if (!mesh) {
    launch_jvp_chain(m->d, p->d, d_frame_params, d_b, K, 0, n_tiles, d_tan_params, d_tb, per_frame, d_tan_joints, nullptr,
                     nullptr, st);
  } else {
    const PriorArgs none{};
    launch_frame_resjac(m->d, p->d, d_frame_params, d_b, p->jvp_r, nullptr, p->jvp_joints, p->jvp_mc, 0, none, st);
    launch_jvp_blend(m->d, p->d, p->jvp_mc, p->jvp_bbuf, st);
    if (d_offsets) launch_offsets_displace(m->d, p->d, d_offsets, offsets_frame_stride, p->jvp_bbuf, st);
    for (int t = 0; t < n_tiles; ++t) {   // one tangent tile of scratch per frame: chain and mesh alternate on the stream
      launch_jvp_chain(m->d, p->d, d_frame_params, d_b, K, t * 32, 1, d_tan_params, d_tb, per_frame, d_tan_joints, p->jvp_tdot,
                       p->jvp_featD, st);
      launch_jvp_mesh(m->d, p->d, p->jvp_mc, p->jvp_featD, p->jvp_tdot, p->jvp_bbuf, p->jvp_dbuf, K, t * 32, d_tan_cloud, row_floats, st);
    }
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BODYFIT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return BODYFIT_OK;
}

int bodyfit_forward_jvp(bodyfit_problem* p, const double* frame_params, const double* beta, int n_tangents,
                        const double* tan_params, const double* tan_beta, double* tan_joints, float* tan_cloud) {
  if (!p || !frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  if (n_tangents < 1) return fail(BODYFIT_ERR_INVALID, "n_tangents < 1");
  if (!tan_joints && !tan_cloud) return fail(BODYFIT_ERR_INVALID, "both outputs are NULL");
  const bodyfit_model* m = p->m;
  const int F = p->d.F, nS = m->nS, K = n_tangents;
  const auto [npose, has_beta, npar, nbeta_all] = dims(p);
  if (tan_cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "tan_cloud needs a problem created with want_mesh");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  if (int ro = order_after_async(p, nullptr)) return ro;
  const size_t nbeta = (has_beta && beta) ? nbeta_all : 0;
  const size_t ntx = tan_params ? (size_t)F * K * npose : 0;
  const size_t ntb = (has_beta && tan_beta) ? (size_t)(p->desc.beta_per_frame ? F : 1) * K * nS : 0;
  const size_t njt = tan_joints ? (size_t)F * K * m->nJ * 3 : 0, ncl = tan_cloud ? (size_t)F * K * m->V * 3 : 0;
  Allocs tmp;
  double *d_x = nullptr, *d_b = nullptr, *d_tx = nullptr, *d_tb = nullptr, *d_tj = nullptr;
  float* d_tc = nullptr;
  HIP_TRY(tmp.alloc(&d_x, npar));
  if (nbeta) HIP_TRY(tmp.alloc(&d_b, nbeta));
  if (ntx) HIP_TRY(tmp.alloc(&d_tx, ntx));
  if (ntb) HIP_TRY(tmp.alloc(&d_tb, ntb));
  if (njt) HIP_TRY(tmp.alloc(&d_tj, njt));
  if (ncl) HIP_TRY(tmp.alloc(&d_tc, ncl));
  HIP_TRY(hipMemcpy(d_x, frame_params, npar * sizeof(double), hipMemcpyHostToDevice));
  if (nbeta) HIP_TRY(hipMemcpy(d_b, beta, nbeta * sizeof(double), hipMemcpyHostToDevice));
  if (ntx) HIP_TRY(hipMemcpy(d_tx, tan_params, ntx * sizeof(double), hipMemcpyHostToDevice));
  if (ntb) HIP_TRY(hipMemcpy(d_tb, tan_beta, ntb * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = bodyfit_forward_jvp_device(p, d_x, d_b, K, d_tx, d_tb, d_tj, d_tc, 3LL * m->V, nullptr)) return rc;
  p->async_pending = false;   // (NULL stream, waited for below)
  if (njt) HIP_TRY(hipMemcpy(tan_joints, d_tj, njt * sizeof(double), hipMemcpyDeviceToHost));
  if (ncl) HIP_TRY(hipMemcpy(tan_cloud, d_tc, ncl * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return BODYFIT_OK;
}

}  // extern "C"
