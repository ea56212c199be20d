// api_vjp.hip — reverse mode of the C ABI in include/bodyfit.h: the forward's VJP (k_forward_vjp.hip) and the residual vector's
// (k_residual_vjp.hip), each as a device entry point and a host wrapper.
#include "host_state.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

using namespace bodyfit;

extern "C" {

namespace {

// the model's VJP operands, once (first VJP of the model): transposed operand block, per-joint skinning lists
int vjp_model_ready(const bodyfit_model* m, hipStream_t st) {
  std::lock_guard<std::mutex> lock(m->vjp_mu);
  if (m->vjp_ready) return BODYFIT_OK;
  const int nVT = m->d.nVTiles, nJ = m->nJ;
  std::vector<std::vector<std::pair<int, float>>> lists(nJ);
  for (int vt = 0; vt < nVT; ++vt)
    for (int col = 0; col < kVTile; ++col) {
      const int v = vt * kVTile + col;
      if (v >= m->V) continue;
      for (int i = 0; i < kMeshNnz; ++i) {
        const float w = m->h_wVal[((size_t)vt * kVTile + col) * kMeshNnz + i];
        const int j = (int)((m->h_wIdx[(size_t)vt * kVTile + col] >> (8 * i)) & 0xffu);
        if (w != 0.0f && j < nJ) lists[j].push_back({v, w});
      }
    }
  std::vector<int> off(kMaxJoints + 1, 0), vid;
  std::vector<float> wv;
  for (int j = 0; j < kMaxJoints; ++j) {
    if (j < nJ) {
      std::sort(lists[j].begin(), lists[j].end(), [](const std::pair<int, float>& a, const std::pair<int, float>& b) {
        return a.first < b.first;
      });
      for (const auto& e : lists[j]) { vid.push_back(e.first); wv.push_back(e.second); }
    }
    off[j + 1] = (int)vid.size();
  }
  HIP_TRY(m->vjp_mem.alloc(&m->d_dirsT, vjp_dirs_t_elems(nVT)));
  const int* d_off = nullptr;
  const int* d_v = nullptr;
  const float* d_w = nullptr;
  HIP_TRY(m->vjp_mem.upload(&d_off, off));
  HIP_TRY(m->vjp_mem.upload(&d_v, vid));
  HIP_TRY(m->vjp_mem.upload(&d_w, wv));
  m->d_csr_off = const_cast<int*>(d_off);
  m->d_csr_v = const_cast<int*>(d_v);
  m->d_csr_w = const_cast<float*>(d_w);
  launch_vjp_build_dirs_t(m->d, m->d_dirsT, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));   // (once per model: VJPs on other streams read the block too)
  m->vjp_ready = true;
  return BODYFIT_OK;
}

// the problem's VJP buffers, once; the clears of its mesh operands are enqueued on the caller's stream `st`, in front of the
// launches that follow them there (a clear on the NULL stream is not ordered against a non-blocking stream)
int vjp_problem_ready(bodyfit_problem* p, bool mesh, hipStream_t st) {
  const bodyfit_model* m = p->m;
  const int F = p->d.F, nFT = p->d.nFTiles, nVT = m->d.nVTiles;
  if (!p->vjp_alloc) {
    HIP_TRY(p->mem.alloc(&p->vjp_gbf, (size_t)F * std::max(m->nS, 1)));
    p->vjp_alloc = true;
  }
  if (mesh && !p->vjp_mesh_alloc) {
    const size_t nfa = (size_t)nFT * kBlendKSteps * 2 * 64 * 8, nsk = (size_t)nFT * kFTile * m->nJ * 12;
    HIP_TRY(p->mem.alloc(&p->vjp_mc.featA, nfa));
    HIP_TRY(p->mem.alloc(&p->vjp_mc.skinT, nsk));
    HIP_TRY(hipMemsetAsync(p->vjp_mc.featA, 0, nfa * sizeof(uint16_t), st));
    HIP_TRY(hipMemsetAsync(p->vjp_mc.skinT, 0, nsk * sizeof(float), st));
    HIP_TRY(p->mem.alloc(&p->vjp_r, (size_t)std::max(1, p->lay.reproj_rows)));
    HIP_TRY(p->mem.alloc(&p->vjp_joints, (size_t)F * m->nJ * 3));
    HIP_TRY(p->mem.alloc(&p->vjp_gb, vjp_gb_elems(nFT, nVT)));
    HIP_TRY(p->mem.alloc(&p->vjp_bbuf, (size_t)F * nVT * kVTile * 3));
    HIP_TRY(p->mem.alloc(&p->vjp_part, vjp_part_elems(nFT, nVT)));
    HIP_TRY(p->mem.alloc(&p->vjp_dT, (size_t)F * kMaxJoints * 12));
    p->vjp_mesh_alloc = true;
  }
  return BODYFIT_OK;
}

}  // namespace

int bodyfit_forward_vjp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                               const float* d_grad_cloud, long long grad_cloud_row_floats, const double* d_grad_joints,
                               double* d_grad_frame_params, double* d_grad_beta, void* stream) {
  return bodyfit_forward_offsets_vjp_device(p, d_frame_params, d_beta, nullptr, 0, d_grad_cloud, grad_cloud_row_floats,
                                            d_grad_joints, d_grad_frame_params, d_grad_beta, nullptr, stream);
}

int bodyfit_forward_offsets_vjp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                                       const float* d_offsets, long long offsets_frame_stride, const float* d_grad_cloud,
                                       long long grad_cloud_row_floats, const double* d_grad_joints, double* d_grad_frame_params,
                                       double* d_grad_beta, float* d_grad_offsets, void* stream) {
  if (!p || !d_frame_params || !d_grad_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  if (d_grad_offsets && !d_offsets) return fail(BODYFIT_ERR_INVALID, "grad_offsets without offsets");
  if (d_grad_offsets && !d_grad_cloud) return fail(BODYFIT_ERR_INVALID, "grad_offsets needs grad_cloud");
  if (d_offsets)
    if (int rc = check_offsets(p, offsets_frame_stride)) return rc;
  const bodyfit_model* m = p->m;
  const int npose = dims(p).npose, F = p->d.F, nS = m->nS;
  const bool has_beta = dims(p).has_beta;
  if (d_grad_cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "grad_cloud needs a problem created with want_mesh");
  if (d_grad_cloud && grad_cloud_row_floats < 3LL * m->V) return fail(BODYFIT_ERR_INVALID, "grad_cloud_row_floats < 3 V");
  if (has_beta && !d_grad_beta) return fail(BODYFIT_ERR_INVALID, "grad_beta is required when n_cols = 76 + n_shape");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double* d_b = has_beta ? d_beta : nullptr;
  const bool mesh = d_grad_cloud != nullptr;
  if (mesh)
    if (int rc = vjp_model_ready(m, st)) return rc;
  if (int rc = vjp_problem_ready(p, mesh, st)) return rc;
  p->async_stream = st;
  p->async_pending = true;
  if (mesh) {
    const PriorArgs none{};
    launch_frame_resjac(m->d, p->d, d_frame_params, d_b, p->vjp_r, nullptr, p->vjp_joints, p->vjp_mc, 0, none, st);
    launch_vjp_mesh(m->d, p->d, p->vjp_mc, d_grad_cloud, grad_cloud_row_floats, p->vjp_gb, p->vjp_bbuf, st);
    if (d_offsets) launch_offsets_displace(m->d, p->d, d_offsets, offsets_frame_stride, p->vjp_bbuf, st);
    if (d_grad_offsets) launch_offsets_grad(m->d, p->d, p->vjp_gb, d_grad_offsets, offsets_frame_stride, st);
    launch_vjp_blend_t(m->d, p->d, p->vjp_gb, m->d_dirsT, p->vjp_part, st);
    launch_vjp_skin_t(m->d, p->d, m->d_csr_off, m->d_csr_v, m->d_csr_w, d_grad_cloud, grad_cloud_row_floats, p->vjp_bbuf,
                      p->vjp_dT, st);
  }
  const bool per_frame = p->desc.beta_per_frame != 0;
  double* gbf = (d_grad_beta && per_frame) ? d_grad_beta : p->vjp_gbf;
  launch_vjp_chain(m->d, p->d, d_frame_params, d_b, mesh ? p->vjp_dT : nullptr, mesh ? p->vjp_part : nullptr, d_grad_joints,
                   d_grad_frame_params, gbf, st);
  if (d_grad_beta && !per_frame) launch_vjp_beta_sum(gbf, F, nS, d_grad_beta, st);
  if (p->n_param_rows > F)   // the halo row
    HIP_TRY(hipMemsetAsync(d_grad_frame_params + (size_t)F * npose, 0, (size_t)(p->n_param_rows - F) * npose * sizeof(double), st));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BODYFIT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return BODYFIT_OK;
}

int bodyfit_forward_vjp(bodyfit_problem* p, const double* frame_params, const double* beta, const float* grad_cloud,
                        const double* grad_joints, double* grad_frame_params, double* grad_beta) {
  return bodyfit_forward_offsets_vjp(p, frame_params, beta, nullptr, 0, grad_cloud, grad_joints, grad_frame_params, grad_beta,
                                     nullptr);
}

int bodyfit_forward_offsets_vjp(bodyfit_problem* p, const double* frame_params, const double* beta, const float* offsets,
                                long long offsets_frame_stride, const float* grad_cloud, const double* grad_joints,
                                double* grad_frame_params, double* grad_beta, float* grad_offsets) {
  if (!p || !frame_params || !grad_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  if (grad_offsets && !offsets) return fail(BODYFIT_ERR_INVALID, "grad_offsets without offsets");
  if (grad_offsets && !grad_cloud) return fail(BODYFIT_ERR_INVALID, "grad_offsets needs grad_cloud");
  if (offsets)
    if (int rc = check_offsets(p, offsets_frame_stride)) return rc;
  const bodyfit_model* m = p->m;
  const int F = p->d.F, nS = m->nS;
  const auto [npose, has_beta, npar, nbeta_all] = dims(p);
  if (grad_cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "grad_cloud needs a problem created with want_mesh");
  if (has_beta && !grad_beta) return fail(BODYFIT_ERR_INVALID, "grad_beta is required when n_cols = 76 + n_shape");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  if (int ro = order_after_async(p, nullptr)) return ro;
  const size_t nbeta = (has_beta && beta) ? nbeta_all : 0;
  const size_t ngb = grad_beta ? (size_t)std::max(1, p->desc.beta_per_frame ? F * nS : nS) : 0;
  const size_t ncl = grad_cloud ? (size_t)F * m->V * 3 : 0, njt = grad_joints ? (size_t)F * m->nJ * 3 : 0;
  // one temporary block: parameters, beta, upstream gradients, outputs
  Allocs tmp;
  double *d_x = nullptr, *d_b = nullptr, *d_gx = nullptr, *d_gb = nullptr, *d_H = nullptr;
  float *d_G = nullptr, *d_o = nullptr, *d_go = nullptr;
  const size_t nof = !offsets ? 0 : (offsets_frame_stride ? (size_t)(F - 1) * (size_t)offsets_frame_stride : 0) + 3 * (size_t)m->V;
  if (nof) HIP_TRY(tmp.alloc(&d_o, nof));
  if (nof && grad_offsets) HIP_TRY(tmp.alloc(&d_go, nof));
  if (nof) HIP_TRY(hipMemcpy(d_o, offsets, nof * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(tmp.alloc(&d_x, npar));
  HIP_TRY(tmp.alloc(&d_gx, npar));
  if (nbeta) HIP_TRY(tmp.alloc(&d_b, nbeta));
  if (ngb) HIP_TRY(tmp.alloc(&d_gb, ngb));
  if (ncl) HIP_TRY(tmp.alloc(&d_G, ncl));
  if (njt) HIP_TRY(tmp.alloc(&d_H, njt));
  HIP_TRY(hipMemcpy(d_x, frame_params, npar * sizeof(double), hipMemcpyHostToDevice));
  if (nbeta) HIP_TRY(hipMemcpy(d_b, beta, nbeta * sizeof(double), hipMemcpyHostToDevice));
  if (ncl) HIP_TRY(hipMemcpy(d_G, grad_cloud, ncl * sizeof(float), hipMemcpyHostToDevice));
  if (njt) HIP_TRY(hipMemcpy(d_H, grad_joints, njt * sizeof(double), hipMemcpyHostToDevice));
  if (ngb) HIP_TRY(hipMemset(d_gb, 0, ngb * sizeof(double)));
  if (int rc = bodyfit_forward_offsets_vjp_device(p, d_x, d_b, d_o, offsets_frame_stride, d_G, 3LL * m->V, d_H, d_gx, d_gb, d_go,
                                                  nullptr))
    return rc;
  p->async_pending = false;   // (NULL stream, waited for below)
  if (d_go) {   // the rows alone: what lies between rows longer than 3 V stays the caller's
    const size_t row = 3 * (size_t)m->V * sizeof(float), pitch = offsets_frame_stride ? (size_t)offsets_frame_stride * sizeof(float) : row;
    HIP_TRY(hipMemcpy2D(grad_offsets, pitch, d_go, pitch, row, offsets_frame_stride ? (size_t)F : 1, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipMemcpy(grad_frame_params, d_gx, npar * sizeof(double), hipMemcpyDeviceToHost));
  if (ngb) HIP_TRY(hipMemcpy(grad_beta, d_gb, ngb * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return BODYFIT_OK;
}

int bodyfit_residuals_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, double* d_residuals,
                             int* d_gmm_comp, int keep_jacobian, void* stream) {
  if (!p || !d_frame_params || !d_residuals) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const bool has_beta = dims(p).has_beta;
  if (has_beta && !d_beta) return fail(BODYFIT_ERR_INVALID, "beta required when the shape block is present");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  p->async_stream = st;
  p->async_pending = true;
  // the sweep without the mesh (k_frame_resjac and its prior workgroups): residuals, Jacobian and components are those of the
  // one-launch sweep
  SweepRequest rq{d_frame_params, has_beta ? d_beta : nullptr};
  rq.want_jac = keep_jacobian ? 1 : 0; rq.stream = st;
  if (int rc = sweep(p, rq)) return rc;
  if (p->lay.total_rows > 0)
    HIP_TRY(hipMemcpyAsync(d_residuals, p->d_r, (size_t)p->lay.total_rows * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (d_gmm_comp) HIP_TRY(hipMemcpyAsync(d_gmm_comp, p->d_comp, (size_t)p->d.F * sizeof(int), hipMemcpyDeviceToDevice, st));
  return BODYFIT_OK;
}

int bodyfit_residual_vjp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                                const double* d_grad_residuals, double* d_grad_frame_params, double* d_grad_beta,
                                int reuse_jacobian, void* stream) {
  if (!p || !d_frame_params || !d_grad_residuals || !d_grad_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const int npose = dims(p).npose, F = p->d.F, nS = m->nS;
  const bool has_beta = dims(p).has_beta, per_frame = p->desc.beta_per_frame != 0;
  if (has_beta && !d_grad_beta) return fail(BODYFIT_ERR_INVALID, "grad_beta is required when n_cols = 76 + n_shape");
  if (has_beta && !reuse_jacobian && !d_beta) return fail(BODYFIT_ERR_INVALID, "beta required when the shape block is present");
  if (reuse_jacobian && !p->jac_current)
    return fail(BODYFIT_ERR_INVALID, "reuse_jacobian: the problem's buffers hold no current Jacobian (none since creation, or "
                                     "a later sweep or solve overwrote it)");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (has_beta && !per_frame && !p->rvjp_gbf) HIP_TRY(p->mem.alloc(&p->rvjp_gbf, (size_t)F * nS));
  if (p->has_gmm && p->lay.prior_rows_per_frame > 0 && !p->rvjp_gmm) {
    // G_k[c][7 + d] = beta_p s L_k[d][c]: row c of the GMM block's transposed Jacobian, in the frame's column layout
    const int D = npose - 7, K = p->gmm.K;
    const std::vector<double>& L = p->desc.gmm->prec_cho;
    const double sc = p->desc.beta_pose * p->gmm.resid_scale;
    std::vector<double> G((size_t)K * D * npose, 0.0);
    for (int k = 0; k < K; ++k)
      for (int c = 0; c < D; ++c)
        for (int d = 0; d < D; ++d) G[((size_t)k * D + c) * npose + 7 + d] = sc * L[((size_t)k * D + d) * D + c];
    const double* up = nullptr;
    HIP_TRY(p->mem.upload(&up, G));
    p->rvjp_gmm = const_cast<double*>(up);
  }
  p->async_stream = st;
  p->async_pending = true;
  if (!reuse_jacobian) {
    SweepRequest rq{d_frame_params, has_beta ? d_beta : nullptr};
    rq.want_jac = 1; rq.stream = st;
    if (int rc = sweep(p, rq)) return rc;
  }
  ResVjpArgs a{};
  a.F = F; a.n_param_rows = p->n_param_rows; a.ncols = p->lay.n_cols; a.npose = npose; a.nS = nS;
  a.kp_offset = p->d.kp_offset;
  a.J = p->d_J;
  a.g = d_grad_residuals;
  a.row_prior = p->row_prior; a.prior_rows = p->lay.prior_rows_per_frame;
  a.row_shape = p->row_shape; a.shape_rows = p->lay.shape_rows; a.shape_per_frame = per_frame ? 1 : 0;
  a.row_temporal = p->row_temporal; a.n_pairs = p->n_pairs;
  a.beta_pose = p->desc.beta_pose; a.beta_shape = p->desc.beta_shape; a.lambda_t = p->desc.lambda_temporal;
  a.gmm_rows = p->has_gmm ? p->rvjp_gmm : nullptr;
  a.comp = p->d_comp;
  a.gx = d_grad_frame_params;
  a.gb = has_beta ? (per_frame ? d_grad_beta : p->rvjp_gbf) : nullptr;
  launch_residual_vjp(a, st);
  if (has_beta && !per_frame) launch_vjp_beta_sum(p->rvjp_gbf, F, nS, d_grad_beta, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BODYFIT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return BODYFIT_OK;
}

int bodyfit_residual_vjp(bodyfit_problem* p, const double* frame_params, const double* beta, const double* grad_residuals,
                         double* grad_frame_params, double* grad_beta) {
  if (!p || !frame_params || !grad_residuals || !grad_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const auto [npose, has_beta, npar, nbeta] = dims(p);
  if (has_beta && !grad_beta) return fail(BODYFIT_ERR_INVALID, "grad_beta is required when n_cols = 76 + n_shape");
  if (has_beta && !beta) return fail(BODYFIT_ERR_INVALID, "beta required when the shape block is present");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  if (int ro = order_after_async(p, nullptr)) return ro;
  const size_t nr = (size_t)p->lay.total_rows;
  Allocs tmp;
  double *d_x = nullptr, *d_b = nullptr, *d_g = nullptr, *d_gx = nullptr, *d_gb = nullptr;
  HIP_TRY(tmp.alloc(&d_x, npar));
  HIP_TRY(tmp.alloc(&d_gx, npar));
  HIP_TRY(tmp.alloc(&d_g, nr));
  if (nbeta) HIP_TRY(tmp.alloc(&d_b, nbeta));
  if (nbeta) HIP_TRY(tmp.alloc(&d_gb, nbeta));
  HIP_TRY(hipMemcpy(d_x, frame_params, npar * sizeof(double), hipMemcpyHostToDevice));
  if (nr) HIP_TRY(hipMemcpy(d_g, grad_residuals, nr * sizeof(double), hipMemcpyHostToDevice));
  if (nbeta) HIP_TRY(hipMemcpy(d_b, beta, nbeta * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = bodyfit_residual_vjp_device(p, d_x, d_b, d_g, d_gx, d_gb, 0, nullptr)) return rc;
  p->async_pending = false;   // (NULL stream, waited for below)
  HIP_TRY(hipMemcpy(grad_frame_params, d_gx, npar * sizeof(double), hipMemcpyDeviceToHost));
  if (nbeta) HIP_TRY(hipMemcpy(grad_beta, d_gb, nbeta * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return BODYFIT_OK;
}

}  // extern "C"
