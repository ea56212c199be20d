// api_problem.hip — a problem's buffers and every evaluation entry point of the C ABI in include/bodyfit.h: asynchronous and
// batched sweeps (with the packed Jacobian of the Ceres-kept path), frame normals, the shared reduction, profiling, status and
// test hooks, write-back and the forward.
#include "host_state.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace bodyfit;

extern "C" {

// ------------------------------------------------------------------------------------------------
// problem
// ------------------------------------------------------------------------------------------------
int bodyfit_problem_create(const bodyfit_model* m, const bodyfit_problem_desc* desc, bodyfit_problem** out) {
  if (!m || !desc || !out) return fail(BODYFIT_ERR_INVALID, "null argument");
  *out = nullptr;
  const int F = desc->n_frames, nJ = m->nJ, nS = m->nS;
  const int npose = 7 + 3 * (nJ - 1);
  if (F <= 0 || !desc->kp_offset || !desc->R0) return fail(BODYFIT_ERR_INVALID, "bad frame arrays");
  if (desc->n_cols != npose && desc->n_cols != npose + nS) return fail(BODYFIT_ERR_INVALID, "n_cols must be 76 or 76 + n_shape");
  if (desc->use_shape && desc->n_cols == npose) return fail(BODYFIT_ERR_INVALID, "use_shape needs the shape block (n_cols = 86)");
  if (desc->kp_offset[0] != 0) return fail(BODYFIT_ERR_INVALID, "kp_offset[0] must be 0");
  for (int f = 0; f < F; ++f)
    if (desc->kp_offset[f + 1] < desc->kp_offset[f]) return fail(BODYFIT_ERR_INVALID, "kp_offset must be non-decreasing");
  const int K = desc->kp_offset[F];
  if (K > 0 && (!desc->kp_id || !desc->kp_uv)) return fail(BODYFIT_ERR_INVALID, "missing keypoints");
  for (int k = 0; k < K; ++k)
    if (desc->kp_id[k] < 0 || desc->kp_id[k] >= nJ + m->nL + m->nReg) return fail(BODYFIT_ERR_INVALID, "keypoint id out of range");
  if (desc->gmm && desc->gmm->d.D != 3 * (nJ - 1)) return fail(BODYFIT_ERR_INVALID, "GMM dimension must be 3 (n_joints - 1)");
  if (desc->beta_pose > 0.0 && nJ != kMaxJoints)
    return fail(BODYFIT_ERR_INVALID, "the pose prior (beta_pose > 0) is built for 24 joints (69 pose dimensions)");
  if (desc->want_mesh && (size_t)((F + kFTile - 1) / kFTile) * kFTile * m->d.nVTiles * kVTile * 12 >= ((size_t)1 << 32))
    return fail(BODYFIT_ERR_INVALID, "mesh path: the cloud of one problem must stay below 4 GiB (split the frames)");
  if (desc->want_mesh && !m->mesh_ok)
    return fail(BODYFIT_ERR_INVALID, "mesh path needs <= 4 skinning weights per vertex");
  if (desc->want_mesh && (nJ != 24 || (m->P != 0 && m->P != 207) || nS > 10))
    return fail(BODYFIT_ERR_INVALID, "mesh path is built for the SMPL shape (24 joints, 207 pose features)");

  HIP_TRY(hipSetDevice(m->device));
  std::unique_ptr<bodyfit_problem> p(new bodyfit_problem());
  // a creation that fails half way returns its blocks to the pool, like bodyfit_problem_destroy: behind a device synchronisation
  // (memsets and uploads may still be in flight on them; later takers use non-blocking streams).  Declared after p: runs first.
  struct SyncOnFailure { std::unique_ptr<bodyfit_problem>& q; ~SyncOnFailure() { if (q) (void)hipDeviceSynchronize(); } } sync_on_failure{p};
  p->mem.pooled = true;
  p->m = m;
  p->desc = *desc;
  p->desc.kp_offset = nullptr; p->desc.kp_id = nullptr; p->desc.kp_uv = nullptr; p->desc.R0 = nullptr;
  p->kp_offset.assign(desc->kp_offset, desc->kp_offset + F + 1);
  p->kp_id.assign(desc->kp_id, desc->kp_id + K);
  p->kp_uv.assign(desc->kp_uv, desc->kp_uv + (size_t)2 * K);
  p->kp_frame.resize(K);
  for (int f = 0; f < F; ++f)
    for (int k = p->kp_offset[f]; k < p->kp_offset[f + 1]; ++k) p->kp_frame[k] = f;
  p->has_gmm = desc->gmm != nullptr && desc->beta_pose > 0.0;
  if (p->has_gmm) p->gmm = desc->gmm->d;

  bodyfit_layout& L = p->lay;
  L.n_keypoints = K;
  L.n_cols = desc->n_cols;
  L.reproj_rows = 2 * K;
  L.prior_rows_per_frame = desc->beta_pose > 0.0 ? (p->has_gmm ? 3 * (nJ - 1) + 1 : 3 * (nJ - 1)) : 0;
  const bool has_beta = desc->n_cols > npose;
  L.shape_rows = (desc->beta_shape > 0.0 && has_beta && nS > 0) ? (desc->beta_per_frame ? F * nS : nS) : 0;
  p->n_pairs = desc->lambda_temporal > 0.0 ? (F - 1 + (desc->temporal_halo ? 1 : 0)) : 0;
  L.temporal_rows = p->n_pairs * (6 + 3 * (nJ - 1));
  if (p->has_gmm) {
    // the GMM prior block's Jacobian per mixture component and joint block, in Ceres' layout (include/Sim3BA.h:293-299)
    const int D = 3 * (nJ - 1), nRes = L.prior_rows_per_frame;
    const size_t Kc = desc->gmm->prec_cho.size() / ((size_t)D * D);
    p->gmm_jt.assign(Kc * (nJ - 1) * nRes * 3, 0.0);
    for (size_t k = 0; k < Kc; ++k) {
      const double* Lk = desc->gmm->prec_cho.data() + k * D * D;
      for (int j = 0; j < nJ - 1; ++j) {
        double* Jb = p->gmm_jt.data() + (k * (nJ - 1) + j) * nRes * 3;
        for (int row = 0; row < D; ++row)
          for (int c = 0; c < 3; ++c) Jb[(size_t)row * 3 + c] = Lk[(size_t)(3 * j + c) * D + row] * desc->beta_pose;
      }
    }
  }
  p->row_prior = L.reproj_rows;
  p->row_shape = p->row_prior + F * L.prior_rows_per_frame;
  p->row_temporal = p->row_shape + L.shape_rows;
  L.total_rows = p->row_temporal + L.temporal_rows;
  p->n_param_rows = F + (desc->temporal_halo ? 1 : 0);

  DevProblem& d = p->d;
  d.F = F; d.K = K; d.ncols = desc->n_cols; d.use_shape = desc->use_shape ? 1 : 0;
  d.beta_stride = desc->beta_per_frame ? nS : 0;
  d.pose_blend = (desc->pose_blend && m->P > 0) ? 1 : 0;
  d.nFTiles = (F + kFTile - 1) / kFTile;
  d.fx = desc->fx; d.fy = desc->fy; d.cx = desc->cx; d.cy = desc->cy;
  {
    // the device copies carry one keypoint chunk (32 entries) of zero padding: k_frame_resjac prefetches a frame's first
    // chunk with unconditional loads.  One block for the three tables (bodyfit_device.h ptab_*_off).
    std::vector<int> ids(p->kp_id);
    for (int& id : ids)        // a regressor row is addressed by the first of its landmark slots on the device
      if (id >= nJ + m->nL) id = nJ + m->reg_slot[id - nJ - m->nL];
    std::vector<double> uv(p->kp_uv);
    ids.resize(ids.size() + 32, 0);
    uv.resize(uv.size() + 64, 0.0);
    const int id_off = ptab_id_off(F), uv_off = ptab_uv_off(F, K);
    std::vector<unsigned char> ptab((size_t)uv_off + uv.size() * sizeof(double), 0);
    std::memcpy(ptab.data(), p->kp_offset.data(), p->kp_offset.size() * sizeof(int));
    std::memcpy(ptab.data() + id_off, ids.data(), ids.size() * sizeof(int));
    std::memcpy(ptab.data() + uv_off, uv.data(), uv.size() * sizeof(double));
    const unsigned char* dev = nullptr;
    HIP_TRY(p->mem.upload(&dev, ptab));
    d.ptab = dev;
    d.kp_offset = reinterpret_cast<const int*>(dev);
    d.kp_id = reinterpret_cast<const int*>(dev + id_off);
    d.kp_uv = reinterpret_cast<const double*>(dev + uv_off);
  }
  std::vector<double> R0(desc->R0, desc->R0 + (size_t)F * 9);
  HIP_TRY(p->mem.upload(&d.R0, R0));

  HIP_TRY(p->mem.alloc(&p->d_params, (size_t)p->n_param_rows * npose));
  HIP_TRY(p->mem.alloc(&p->d_beta, (size_t)std::max(1, desc->beta_per_frame ? F * nS : nS)));
  HIP_TRY(p->mem.alloc(&p->d_r, (size_t)L.total_rows));
  HIP_TRY(p->mem.alloc(&p->d_J, (size_t)L.reproj_rows * L.n_cols));
  HIP_TRY(p->mem.alloc(&p->d_joints, (size_t)F * nJ * 3));
  HIP_TRY(p->mem.alloc(&p->d_comp, (size_t)F));
  HIP_TRY(p->mem.alloc(&p->d_partials, (size_t)reduce_partials_doubles()));
  if (L.n_cols > npose && !desc->beta_per_frame && nS == kMaxShape) {
    const size_t nfp = (size_t)(F + (F + 15) / 16) * kReducePartial;   // one row per frame + one per prior tile
    HIP_TRY(p->mem.alloc(&p->d_frame_partials, nfp));
    HIP_TRY(hipMemset(p->d_frame_partials, 0, nfp * sizeof(double)));
  }
  HIP_TRY(p->mem.alloc(&p->d_normal, (size_t)66));
  HIP_TRY(hipMemset(p->d_r, 0, (size_t)std::max(1, L.total_rows) * sizeof(double)));
  HIP_TRY(hipMemset(p->d_comp, 0, (size_t)F * sizeof(int)));
  HIP_TRY(hipMemset(p->d_beta, 0, (size_t)std::max(1, desc->beta_per_frame ? F * nS : nS) * sizeof(double)));
  if (desc->want_mesh) {
    const size_t nfa = (size_t)d.nFTiles * kBlendKSteps * 2 * 64 * 8;
    HIP_TRY(p->mem.alloc(&p->mc.featA, nfa));
    const size_t nsk = (size_t)d.nFTiles * kFTile * nJ * 12;   // whole frame tiles, zero beyond F
    HIP_TRY(p->mem.alloc(&p->mc.skinT, nsk));
    HIP_TRY(hipMemset(p->mc.skinT, 0, nsk * sizeof(float)));
    // frames padded to whole 32-frame tiles, each frame to whole 32-vertex tiles: k_mesh_blend_lbs stores
    // unconditionally, whole 128-byte lines per half-wave
    HIP_TRY(p->mem.alloc(&p->d_cloud, (size_t)d.nFTiles * kFTile * m->d.nVTiles * kVTile * 3));
    HIP_TRY(hipMemset(p->mc.featA, 0, nfa * sizeof(uint16_t)));
    const size_t nfu = kFusedSyncHeader + (size_t)((F + 255) / 256) * 8 * kUnitCounterStride * 4;
    HIP_TRY(p->mem.alloc(&p->d_fused, nfu));
    HIP_TRY(hipMemset(p->d_fused, 0, nfu));
    p->fused_bytes = nfu;
    // BODYFIT_ONE_LAUNCH=0 keeps the two-launch sweep (k_frame_resjac, then k_mesh_blend_lbs): A/B measurements, fallback
    const char* fe = std::getenv("BODYFIT_ONE_LAUNCH");
    p->fused_enabled = !(fe && fe[0] == '0');
  }
  // the clears above run on the NULL stream and need not have completed when hipMemset returns; the problem's first caller may
  // be a non-blocking stream, which is not ordered against the NULL stream: wait for them here, once per problem
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = p.release();
  return BODYFIT_OK;
}

void bodyfit_problem_destroy(bodyfit_problem* p) {
  if (!p) return;
  (void)hipSetDevice(p->m->device);
  if (p->lm_stream) (void)hipStreamDestroy(p->lm_stream);
  if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
  if (p->async_event) (void)hipEventDestroy(p->async_event);
  // the problem's blocks go to the BlockPool, not to hipFree: what hipFree did implicitly — wait for every kernel that may
  // still touch them — is done here once
  (void)hipDeviceSynchronize();
  delete p;
}

int bodyfit_problem_layout(const bodyfit_problem* p, bodyfit_layout* out) {
  if (!p || !out) return fail(BODYFIT_ERR_INVALID, "null argument");
  *out = p->lay;
  return BODYFIT_OK;
}

int bodyfit_problem_views(bodyfit_problem* p, bodyfit_device_views* out) {
  if (!p || !out) return fail(BODYFIT_ERR_INVALID, "null argument");
  out->residuals = p->d_r;
  out->jacobian = p->d_J;
  out->gmm_comp = p->d_comp;
  out->cloud = p->d_cloud;
  out->cloud_frame_stride = (long long)p->m->d.nVTiles * kVTile * 3;
  out->joints = p->d_joints;
  out->normal_eq = p->d_normal;
  return BODYFIT_OK;
}

int bodyfit_evaluate_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                            int want_jacobian, void* stream) {
  if (!p || !d_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(p->m->device));
  // Eager launches.  A hipGraph capture of this fork/join sweep was measured SLOWER on MI355X / ROCm 7.2
  // (256 frames: 79.8 us per replay vs 59.8 us eager), so no graph is used here.
  p->async_stream = static_cast<hipStream_t>(stream);
  p->async_pending = true;
  SweepRequest rq{d_frame_params, d_beta};
  rq.want_jac = want_jacobian; rq.mesh = p->desc.want_mesh != 0; rq.stream = static_cast<hipStream_t>(stream);
  return sweep(p, rq);
}

// Which column blocks of each reprojection block's Jacobian are STRUCTURALLY non-zero: found once per problem by a probe
// sweep at a generic (pseudo-random) point — a block that is zero there is zero everywhere (the chain walk of
// include/Sim3BA.h:173-207 reaches a keypoint's kinematic ancestors only; landmark / regressor keypoints come out dense).
// No model-specific reasoning on the host: the kernel's own output decides.  Called under the problem's lock.
static int build_pack_tables(bodyfit_problem* p, hipStream_t st) {
  const bodyfit_model* m = p->m;
  const int nJ = m->nJ, n = p->lay.n_cols, K = p->lay.n_keypoints;
  const auto [npose, has_beta, npar, nbeta] = dims(p);
  const size_t nJd = (size_t)p->lay.reproj_rows * n;
  HIP_TRY(p->c_J.ensure(nJd));
  std::vector<double> x(npar), b(nbeta);
  unsigned long long sd = 0x9e3779b97f4a7c15ull;
  auto u = [&]() { sd = sd * 6364136223846793005ull + 1442695040888963407ull; return (double)(sd >> 11) / 9007199254740992.0 - 0.5; };
  for (int f = 0; f < p->n_param_rows; ++f) {
    double* q = x.data() + (size_t)f * npose;
    q[0] = 1.0 + 0.2 * u();
    for (int i = 1; i < 4; ++i) q[i] = 0.6 * u();
    q[4] = 0.2 * u(); q[5] = 0.2 * u(); q[6] = 3.0 + 0.4 * u();
    for (int i = 7; i < npose; ++i) q[i] = 0.6 * u();
  }
  for (auto& v : b) v = u();
  HIP_TRY(hipMemcpyAsync(p->d_params, x.data(), npar * sizeof(double), hipMemcpyHostToDevice, st));
  if (nbeta) HIP_TRY(hipMemcpyAsync(p->d_beta, b.data(), nbeta * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));   // (x, b are pageable: the copies above have left them)
  SweepRequest rq{p->d_params, has_beta ? p->d_beta : nullptr};
  rq.want_jac = 1; rq.stream = st;
  if (int rc = sweep(p, rq)) return rc;
  HIP_TRY(hipMemcpyAsync(p->c_J.data(), p->d_J, nJd * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int nblocks = 3 + (nJ - 1) + (has_beta ? 1 : 0);
  p->pk_mask.assign((size_t)K, 0u);
  p->pk_off.assign((size_t)K + 1, 0u);
  p->pk_src.assign((size_t)K * 32, (short)-1);
  size_t total = 0;
  for (int k = 0; k < K; ++k) {
    const double* J0 = p->c_J.data() + (size_t)(2 * k) * n;
    const double* J1 = J0 + n;
    unsigned mask = 0;
    int ncol = 0;
    for (int blk = 0; blk < nblocks; ++blk) {
      const int off = blk == 0 ? 0 : (blk < 3 + (nJ - 1) ? 1 + 3 * (blk - 1) : npose);
      const int sz = blk == 0 ? 1 : (blk < 3 + (nJ - 1) ? 3 : n - npose);
      bool any = false;
      for (int i = 0; i < sz; ++i) any = any || J0[off + i] != 0.0 || J1[off + i] != 0.0;
      if (any) { mask |= 1u << blk; ncol += sz; }
    }
    p->pk_mask[k] = mask;
    p->pk_off[k] = (unsigned)total;
    {
      // a present block's [2][size] row-major image (what Ceres asks for) starts at src[blk] inside the keypoint's packed span:
      // the span holds the present blocks in block order, each as its two rows back to back (k_pack_jacobian's layout)
      short* src = p->pk_src.data() + (size_t)k * 32;
      int at = 0;
      for (int blk = 0; blk < 32; ++blk) {
        const int sz = blk == 0 ? 1 : (blk < 3 + (nJ - 1) ? 3 : n - npose);
        const bool present = blk < nblocks && ((mask >> blk) & 1u);
        src[blk] = present ? (short)at : (short)-1;
        if (present) at += 2 * sz;
      }
    }
    total += 2 * (size_t)ncol;
  }
  if (total >= ((size_t)1 << 32)) return fail(BODYFIT_ERR_INVALID, "packed Jacobian exceeds 2^32 doubles");
  p->pk_off[K] = (unsigned)total;
  HIP_TRY(p->mem.alloc(&p->d_pk_mask, (size_t)std::max(K, 1)));
  HIP_TRY(p->mem.alloc(&p->d_pk_off, (size_t)K + 1));
  HIP_TRY(p->mem.alloc(&p->d_Jp, std::max<size_t>(total, 1)));
  HIP_TRY(p->c_Jp.ensure(std::max<size_t>(total, 1)));
  HIP_TRY(hipMemcpy(p->d_pk_mask, p->pk_mask.data(), (size_t)K * sizeof(unsigned), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_pk_off, p->pk_off.data(), ((size_t)K + 1) * sizeof(unsigned), hipMemcpyHostToDevice));
  p->pk_ready = true;
  return BODYFIT_OK;
}

int bodyfit_evaluate_batch(bodyfit_problem* p, const double* frame_params, const double* beta, double* residuals,
                           double* jacobian, int* gmm_comp, int want_jacobian) {
  if (!p || !frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const auto [npose, has_beta, npar, nbeta] = dims(p);
  if (has_beta && !beta) return fail(BODYFIT_ERR_INVALID, "beta required when the shape block is present");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  const int wj = (want_jacobian && p->lay.reproj_rows > 0) ? 1 : 0;
  const size_t nr = (size_t)p->lay.total_rows, nJ = (size_t)p->lay.reproj_rows * p->lay.n_cols;
  // everything crosses PCIe from / into page-locked mirrors, on the problem's own stream
  HIP_TRY(p->c_params.ensure(npar)); HIP_TRY(p->c_beta.ensure(nbeta)); HIP_TRY(p->c_r.ensure(nr));
  HIP_TRY(p->c_comp.ensure((size_t)p->d.F));
  if (!p->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
  hipStream_t st = p->copy_stream;
  p->cache_valid = false;
  // No caller's Jacobian buffer: the sweep is cached for bodyfit_evaluate_block (Ceres' EvaluationCallback pattern), and only
  // the structurally non-zero column blocks cross PCIe (BODYFIT_PACKED_J=0: the dense panel, as with a caller's buffer)
  static const bool packed_enabled = [] { const char* e = std::getenv("BODYFIT_PACKED_J"); return !(e && e[0] == '0'); }();
  const bool packed = wj && !jacobian && packed_enabled && p->lay.n_cols <= 128;
  if (int ro = order_after_async(p, st)) return ro;   // behind any asynchronous sweep of this problem still in flight
  if (packed && !p->pk_ready)
    if (int rcp = build_pack_tables(p, st)) return rcp;
  if (wj && !packed) HIP_TRY(p->c_J.ensure(nJ));
  std::memcpy(p->c_params.data(), frame_params, npar * sizeof(double));
  if (nbeta) std::memcpy(p->c_beta.data(), beta, nbeta * sizeof(double));
  p->c_npar = npar; p->c_nbeta = nbeta;
  static const bool pack_direct = [] { const char* e = std::getenv("BODYFIT_PACK_DIRECT"); return !(e && e[0] == '0'); }();
  for (int attempt = 0;; ++attempt) {   // (a one-launch sweep whose in-launch wait ran out is re-issued as two launches)
    // (measured and rejected, round 5: the sweep reading the parameters straight from the page-locked mirrors instead of these two
    //  copies — 180.2 / 181.8 / 182.9 us per cached sweep against 181.1 / 182.6 / 180.0: no difference)
    HIP_TRY(hipMemcpyAsync(p->d_params, p->c_params.data(), npar * sizeof(double), hipMemcpyHostToDevice, st));
    if (nbeta) HIP_TRY(hipMemcpyAsync(p->d_beta, p->c_beta.data(), nbeta * sizeof(double), hipMemcpyHostToDevice, st));
    const double* xs = p->d_params;
    const double* bs = has_beta ? p->d_beta : nullptr;
    SweepRequest rq{xs, bs};
    rq.want_jac = wj; rq.mesh = p->desc.want_mesh != 0; rq.stream = st;
    int rc = sweep(p, rq);
    if (rc) return rc;
    const bool one_kernel_down = wj && packed && pack_direct;   // residuals and components ride on the packing kernel
    if (!one_kernel_down) {
      HIP_TRY(hipMemcpyAsync(p->c_r.data(), p->d_r, nr * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(p->c_comp.data(), p->d_comp, (size_t)p->d.F * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    size_t n_down = 0;
    const double* src_down = nullptr;
    double* dst_down = nullptr;
    // (measured and rejected: the Jacobian's two halves on two streams / copy engines — 234 against 221 us per sweep)
    if (one_kernel_down) {
      // the packing kernel stores straight into the page-locked host cache (it is device-addressable), residuals and GMM
      // components with it: ONE kernel behind the sweep instead of a kernel and three copy commands (219 -> 207 -> see DESIGN 6)
      launch_pack_jacobian(p->lay.n_keypoints, p->lay.n_cols, m->nJ - 1, p->d_J, p->d_pk_mask, p->d_pk_off, p->c_Jp.data(), p->d_r,
                           (int)nr, p->c_r.data(), p->d_comp, p->d.F, p->c_comp.data(), st);
    } else if (wj && packed) {
      launch_pack_jacobian(p->lay.n_keypoints, p->lay.n_cols, m->nJ - 1, p->d_J, p->d_pk_mask, p->d_pk_off, p->d_Jp, nullptr, 0,
                           nullptr, nullptr, 0, nullptr, st);
      n_down = (size_t)p->pk_off[p->lay.n_keypoints]; src_down = p->d_Jp; dst_down = p->c_Jp.data();
    } else if (wj) {
      n_down = nJ; src_down = p->d_J; dst_down = p->c_J.data();
    }
    if (n_down) HIP_TRY(hipMemcpyAsync(dst_down, src_down, n_down * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (attempt == 0 && fused_timed_out(p)) continue;
    break;
  }
  p->cache_valid = true;
  p->cache_has_jac = wj != 0;
  p->cache_packed = packed;
  if (residuals) std::memcpy(residuals, p->c_r.data(), nr * sizeof(double));
  if (jacobian && wj) std::memcpy(jacobian, p->c_J.data(), nJ * sizeof(double));
  if (gmm_comp) std::memcpy(gmm_comp, p->c_comp.data(), (size_t)p->d.F * sizeof(int));
  return BODYFIT_OK;
}

int bodyfit_internal_frame_normals(bodyfit_problem* p, const double* frame_params, const double* beta, double* residuals,
                                   int* gmm_comp, double* H) {
  if (!p || !frame_params || !residuals || !H) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const int F = p->d.F;
  const auto [npose, has_beta, npar, nbeta] = dims(p);
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  const size_t nH = (size_t)F * kNormalRows * kNormalLd;
  if (!p->d_frame_normal) HIP_TRY(p->mem.alloc(&p->d_frame_normal, nH));
  if (int ro = order_after_async(p, nullptr)) return ro;
  HIP_TRY(hipMemcpyAsync(p->d_params, frame_params, npar * sizeof(double), hipMemcpyHostToDevice, nullptr));
  if (nbeta) HIP_TRY(hipMemcpyAsync(p->d_beta, beta, nbeta * sizeof(double), hipMemcpyHostToDevice, nullptr));
  SweepRequest rq{p->d_params, has_beta ? p->d_beta : nullptr};
  rq.want_jac = 1;
  int rc = sweep(p, rq);
  if (rc) return rc;
  launch_frame_normal(F, p->lay.n_cols, p->d.kp_offset, p->desc.huber_delta, p->d_r, p->d_J, p->d_frame_normal, nullptr);
  HIP_TRY(hipMemcpyAsync(residuals, p->d_r, (size_t)p->lay.total_rows * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  if (gmm_comp) HIP_TRY(hipMemcpyAsync(gmm_comp, p->d_comp, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipMemcpyAsync(H, p->d_frame_normal, nH * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

int bodyfit_frame_normals(bodyfit_problem* p, const double* frame_params, const double* beta, double* residuals,
                          int* gmm_comp, double* normals) {
  if (p) {
    int maxk = 0;
    for (int f = 0; f < p->d.F; ++f) maxk = std::max(maxk, p->kp_offset[f + 1] - p->kp_offset[f]);
    if (maxk > 32) return fail(BODYFIT_ERR_INVALID, "bodyfit_frame_normals: at most 32 keypoints per frame");
  }
  return bodyfit_internal_frame_normals(p, frame_params, beta, residuals, gmm_comp, normals);
}

int bodyfit_arm_shared_reduction(bodyfit_problem* p, double* d_out66) {
  if (!p) return fail(BODYFIT_ERR_INVALID, "null argument");
  if (d_out66 && (p->desc.beta_per_frame || p->m->nS != kMaxShape || !dims(p).has_beta))
    return fail(BODYFIT_ERR_INVALID, "bodyfit_arm_shared_reduction: needs a problem with a shared 10-coefficient shape block");
  std::lock_guard<std::mutex> lock(p->mu);
  p->armed_out66 = d_out66;
  p->fold_fresh = false;
  return BODYFIT_OK;
}

int bodyfit_reduce_shared_device(bodyfit_problem* p, double* d_out66, void* stream) {
  if (!p) return fail(BODYFIT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(p->m->device));
  const int npose = dims(p).npose;
  const int shared_shape_rows = (!p->desc.beta_per_frame) ? p->lay.shape_rows : 0;
  if (p->fold_fresh && d_out66 && d_out66 == p->armed_out66) return BODYFIT_OK;   // the sweep's own tail has written it
  p->async_stream = static_cast<hipStream_t>(stream);
  p->async_pending = true;
  if (p->d_frame_partials && p->partials_fresh) {
    // the sweep's k_frame_resjac already reduced every frame's reprojection rows: sum the per-frame partials and the
    // prior / temporal rows, pack
    launch_reduce_frames(p->d.F + p->partials_tiles, p->d_r, p->row_shape, shared_shape_rows,
                         p->desc.beta_shape, p->d_frame_partials, p->d_partials, d_out66 ? d_out66 : p->d_normal,
                         static_cast<hipStream_t>(stream));
  } else {
    launch_reduce_shared_ex(p->lay.n_keypoints, p->lay.n_cols, npose, p->m->nS, p->lay.total_rows, p->d_r, p->d_J,
                            p->desc.huber_delta, p->row_shape, shared_shape_rows, p->desc.beta_shape, p->d_partials,
                            d_out66 ? d_out66 : p->d_normal, static_cast<hipStream_t>(stream));
  }
  HIP_TRY(hipGetLastError());
  return BODYFIT_OK;
}

// Per-kernel timing with HIP events on `stream`: `iters` sweeps, avg_ms[0..4] = {frame_resjac, priors,
// mesh_blend_lbs, reduce_shared, sweep_roles} average launch durations in milliseconds.
int bodyfit_profile_sweep(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                          int want_jacobian, int with_reduce, int iters, void* stream, double* avg_ms) {
  if (!p || !d_frame_params || !avg_ms || iters <= 0) return fail(BODYFIT_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(p->m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // per sweep: [0],[1] begin / end of the k_frame_resjac dispatch, [2],[3] of the mesh dispatch, [4],[5] of the fused
  // dispatch (all taken from the dispatch's own timestamps, so they match rocprofv3's kernel durations; a sweep is
  // either the first two pairs or the third), [6],[7] around the reduction launches
  const bool mesh = p->desc.want_mesh != 0;
  std::vector<hipEvent_t> ev((size_t)iters * 8);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  int rc = BODYFIT_OK;
  const unsigned epoch0 = p->fused_epoch;
  for (int it = 0; it < iters && rc == BODYFIT_OK; ++it) {
    hipEvent_t* e = ev.data() + (size_t)it * 8;
    SweepRequest rq{d_frame_params, d_beta};
    rq.want_jac = want_jacobian; rq.mesh = mesh; rq.stream = st; rq.events = e;
    rc = sweep(p, rq);
    if (rc == BODYFIT_OK && with_reduce) {
      (void)hipEventRecord(e[6], st);
      rc = bodyfit_reduce_shared_device(p, p->armed_out66, stream);   // (armed: the sweep's own tail did it, nothing is launched)
      (void)hipEventRecord(e[7], st);
    }
  }
  const bool fused = p->fused_epoch != epoch0;
  hipError_t se = hipStreamSynchronize(st);
  for (int k = 0; k < 5; ++k) avg_ms[k] = 0.0;
  if (rc == BODYFIT_OK && se == hipSuccess) {
    for (int it = 0; it < iters; ++it) {
      hipEvent_t* e = ev.data() + (size_t)it * 8;
      float ms = 0.f;
      if (fused) {
        (void)hipEventElapsedTime(&ms, e[4], e[5]); avg_ms[4] += ms / iters;
      } else {
        (void)hipEventElapsedTime(&ms, e[0], e[1]); avg_ms[0] += ms / iters;
        if (mesh) { (void)hipEventElapsedTime(&ms, e[2], e[3]); avg_ms[2] += ms / iters; }
      }
      if (with_reduce) { (void)hipEventElapsedTime(&ms, e[6], e[7]); avg_ms[3] += ms / iters; }
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (se != hipSuccess) return fail(BODYFIT_ERR_HIP, std::string("profile sync: ") + hipGetErrorString(se));
  if (rc == BODYFIT_OK) rc = fused_check(p);
  return rc;
}

// Status of the problem's asynchronous sweeps (bodyfit_evaluate_device) enqueued on `stream` so far: waits for the stream,
// then reads the one-launch sweep's error word.
int bodyfit_sweep_status(bodyfit_problem* p, void* stream) {
  if (!p) return fail(BODYFIT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(p->m->device));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  if (p->async_stream == static_cast<hipStream_t>(stream)) p->async_pending = false;
  return fused_check(p);
}

long bodyfit_sweep_timeouts(const bodyfit_problem* p) { return p ? p->fused_timeouts : 0; }
long bodyfit_internal_fused_timeouts(const bodyfit_problem* p) { return bodyfit_sweep_timeouts(p); }   // (the tests' older name)

int bodyfit_set_exchange_timeout(bodyfit_problem* p, double seconds) {
  if (!p || !(seconds >= 0.0)) return fail(BODYFIT_ERR_INVALID, "bodyfit_set_exchange_timeout: bad argument");
  p->exchange_timeout_s = seconds;
  return BODYFIT_OK;
}

int bodyfit_set_shard_proxy(bodyfit_problem* p, int n_ranks, int rank) {
  if (!p || n_ranks < 0 || (n_ranks > 0 && (rank < 0 || rank >= n_ranks)))
    return fail(BODYFIT_ERR_INVALID, "bodyfit_set_shard_proxy: bad argument");
  p->proxy_ranks = n_ranks > 1 ? n_ranks : 0;
  p->proxy_rank = n_ranks > 1 ? rank : 0;
  return BODYFIT_OK;
}

// Test hook (not part of include/bodyfit.h): rank `rank`'s candidate sweep "fails" in LM iteration `iter` of the problem's
// next sharded solves (-1, -1: off).  tests/test_gpu_sharded_solve.py.
int bodyfit_internal_set_test_poison(bodyfit_problem* p, int rank, int iter) {
  if (!p) return fail(BODYFIT_ERR_INVALID, "null argument");
  p->test_poison_rank = rank; p->test_poison_iter = iter;
  return BODYFIT_OK;
}

int bodyfit_internal_solver_view(bodyfit_problem* p, bodyfit_solver_view* out) {
  if (!p || !out) return BODYFIT_ERR_INVALID;
  out->n_frames = p->d.F; out->n_joints = p->m->nJ; out->n_shape = p->m->nS;
  out->beta_per_frame = p->desc.beta_per_frame; out->has_gmm = p->has_gmm ? 1 : 0;
  out->temporal_halo = p->desc.temporal_halo;
  out->beta_pose = p->desc.beta_pose; out->beta_shape = p->desc.beta_shape;
  out->lambda_temporal = p->desc.lambda_temporal; out->huber_delta = p->desc.huber_delta;
  out->kp_offset = p->kp_offset.data();
  out->max_kp_per_frame = 0;
  for (int f = 0; f < p->d.F; ++f)
    out->max_kp_per_frame = std::max(out->max_kp_per_frame, p->kp_offset[f + 1] - p->kp_offset[f]);
  out->prec_cho = p->has_gmm ? p->desc.gmm->prec_cho.data() : nullptr;
  return BODYFIT_OK;
}

// Test hook (not part of include/bodyfit.h): the bound of the one-launch sweep's in-launch waits, in 10 ns ticks.  A bound of
// one tick makes every wait run out, which is how tests/test_gpu_one_launch.py exercises the error word and the fall-back to
// the two-launch sweep.  0 restores the default.
int bodyfit_internal_set_role_timeout(bodyfit_problem* p, unsigned long long ticks) {
  if (!p) return fail(BODYFIT_ERR_INVALID, "null argument");
  p->role_timeout_ticks = ticks ? ticks : kRoleTimeoutDefault;
  return BODYFIT_OK;
}

#ifdef BODYFIT_STAMPS
// diagnostic builds only; not part of include/bodyfit.h
int bodyfit_debug_set_stamp_buffer(bodyfit_problem* p, unsigned long long* d_buf) {
  p->d.dbg = d_buf;
  return BODYFIT_OK;
}
#endif

int bodyfit_writeback_batch(bodyfit_problem* p, const double* frame_params, const double* beta, double* R0_out,
                            double* joints, float* cloud, double* mean_px) {
  if (!p || !frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const int F = p->d.F;
  const auto [npose, has_beta, npar, nbeta_all] = dims(p);
  if (cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "problem was created without want_mesh");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  const size_t nbeta = (has_beta && beta) ? nbeta_all : 0;
  if (!p->d_writeback) HIP_TRY(p->mem.alloc(&p->d_writeback, npar + (size_t)F * 10));
  double* d_upd = p->d_writeback;
  double* d_R0n = d_upd + npar;
  double* d_px = d_R0n + (size_t)F * 9;
  if (int ro = order_after_async(p, nullptr)) return ro;
  HIP_TRY(hipMemcpyAsync(p->d_params, frame_params, npar * sizeof(double), hipMemcpyHostToDevice, nullptr));
  if (nbeta) HIP_TRY(hipMemcpyAsync(p->d_beta, beta, nbeta * sizeof(double), hipMemcpyHostToDevice, nullptr));
  launch_writeback_prepare(F, npose, p->d_params, p->d.R0, d_upd, d_R0n, nullptr);
  for (int attempt = 0;; ++attempt) {   // (a one-launch sweep whose in-launch wait ran out is re-issued as two launches)
    SweepRequest rq{d_upd, nbeta ? p->d_beta : nullptr};
    rq.mesh = p->desc.want_mesh != 0; rq.R0_override = d_R0n;
    int rc = sweep(p, rq);
    if (rc) return rc;
    launch_mean_pixel_error(F, m->nJ, p->d.kp_offset, p->d.kp_id, p->d.kp_uv, p->d_joints, p->d.fx, p->d.fy, p->d.cx,
                            p->d.cy, d_px, nullptr);
    if (R0_out) HIP_TRY(hipMemcpyAsync(R0_out, d_R0n, (size_t)F * 9 * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    if (mean_px) HIP_TRY(hipMemcpyAsync(mean_px, d_px, (size_t)F * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    if (joints)
      HIP_TRY(hipMemcpyAsync(joints, p->d_joints, (size_t)F * m->nJ * 3 * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    if (cloud) {
      const size_t row = (size_t)m->V * 3 * sizeof(float), pitch = (size_t)m->d.nVTiles * kVTile * 3 * sizeof(float);
      HIP_TRY(hipMemcpy2DAsync(cloud, row, p->d_cloud, pitch, row, (size_t)F, hipMemcpyDeviceToHost, nullptr));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipGetLastError());
    if (attempt == 0 && fused_timed_out(p)) continue;
    break;
  }
  return BODYFIT_OK;
}

int bodyfit_forward(bodyfit_problem* p, const double* frame_params, const double* beta, double* joints,
                    float* cloud) {
  if (!p || !frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const auto [npose, has_beta, npar, nbeta_all] = dims(p);
  if (cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "problem was created without want_mesh");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  const size_t nbeta = (has_beta && beta) ? nbeta_all : 0;
  if (int ro = order_after_async(p, nullptr)) return ro;
  HIP_TRY(hipMemcpy(p->d_params, frame_params, npar * sizeof(double), hipMemcpyHostToDevice));
  if (nbeta) HIP_TRY(hipMemcpy(p->d_beta, beta, nbeta * sizeof(double), hipMemcpyHostToDevice));
  for (int attempt = 0;; ++attempt) {   // (a one-launch sweep whose in-launch wait ran out is re-issued as two launches)
    SweepRequest rq{p->d_params, nbeta ? p->d_beta : nullptr};
    rq.mesh = cloud != nullptr;
    int rc = sweep(p, rq);
    if (rc) return rc;
    if (joints)
      HIP_TRY(hipMemcpy(joints, p->d_joints, (size_t)p->d.F * m->nJ * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (cloud) {
      const size_t row = (size_t)m->V * 3 * sizeof(float), pitch = (size_t)m->d.nVTiles * kVTile * 3 * sizeof(float);
      HIP_TRY(hipMemcpy2D(cloud, row, p->d_cloud, pitch, row, (size_t)p->d.F, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipDeviceSynchronize());
    if (attempt == 0 && fused_timed_out(p)) continue;
    break;
  }
  return BODYFIT_OK;
}

int bodyfit_forward_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, double* d_joints,
                           float* d_cloud, long long cloud_row_floats, void* stream) {
  return bodyfit_forward_offsets_device(p, d_frame_params, d_beta, nullptr, 0, d_joints, d_cloud, cloud_row_floats, stream);
}

int bodyfit_forward_offsets_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, const float* d_offsets,
                                   long long offsets_frame_stride, double* d_joints, float* d_cloud, long long cloud_row_floats,
                                   void* stream) {
  if (!p || !d_frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  if (d_cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "problem was created without want_mesh");
  if (d_cloud && cloud_row_floats < 3LL * m->V) return fail(BODYFIT_ERR_INVALID, "cloud_row_floats < 3 V");
  if (d_offsets)
    if (int rc = check_offsets(p, offsets_frame_stride)) return rc;
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  p->async_stream = st;
  p->async_pending = true;
  const double* d_b = dims(p).has_beta ? d_beta : nullptr;
  // the two-launch sweep without Jacobian or priors: joints straight into the caller's buffer, the cloud through the problem's
  // padded one
  const PriorArgs none{};
  p->jac_current = false;   // (its residual rows land in d_r)
  launch_frame_resjac(m->d, p->d, d_frame_params, d_b, p->d_r, nullptr, d_joints ? d_joints : p->d_joints,
                      d_cloud ? p->mc : MeshCoef{}, 0, none, st);
  if (d_cloud) {
    launch_mesh(m->d, p->d, p->mc, p->d_cloud, none, d_frame_params, st);
    const size_t row = (size_t)m->V * 3 * sizeof(float), pitch = (size_t)m->d.nVTiles * kVTile * 3 * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(d_cloud, (size_t)cloud_row_floats * sizeof(float), p->d_cloud, pitch, row, (size_t)p->d.F,
                             hipMemcpyDeviceToDevice, st));
    if (d_offsets) launch_offsets_apply(m->d, p->d, p->mc, d_offsets, offsets_frame_stride, d_cloud, cloud_row_floats, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BODYFIT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return BODYFIT_OK;
}

int bodyfit_forward_offsets(bodyfit_problem* p, const double* frame_params, const double* beta, const float* offsets,
                            long long offsets_frame_stride, double* joints, float* cloud) {
  if (!offsets) return bodyfit_forward(p, frame_params, beta, joints, cloud);
  if (!p || !frame_params) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const auto [npose, has_beta, npar, nbeta_all] = dims(p);
  if (cloud && !p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "problem was created without want_mesh");
  if (int rc = check_offsets(p, offsets_frame_stride)) return rc;
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  if (int ro = order_after_async(p, nullptr)) return ro;
  const int F = p->d.F;
  const size_t nbeta = (has_beta && beta) ? nbeta_all : 0;
  const size_t nof = offsets_frame_stride ? (size_t)(F - 1) * (size_t)offsets_frame_stride + 3 * (size_t)m->V : 3 * (size_t)m->V;
  const size_t njt = joints ? (size_t)F * m->nJ * 3 : 0, ncl = cloud ? (size_t)F * m->V * 3 : 0;
  Allocs tmp;
  double *d_x = nullptr, *d_b = nullptr, *d_j = nullptr;
  float *d_o = nullptr, *d_c = nullptr;
  HIP_TRY(tmp.alloc(&d_x, npar));
  HIP_TRY(tmp.alloc(&d_o, nof));
  if (nbeta) HIP_TRY(tmp.alloc(&d_b, nbeta));
  if (njt) HIP_TRY(tmp.alloc(&d_j, njt));
  if (ncl) HIP_TRY(tmp.alloc(&d_c, ncl));
  HIP_TRY(hipMemcpy(d_x, frame_params, npar * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_o, offsets, nof * sizeof(float), hipMemcpyHostToDevice));
  if (nbeta) HIP_TRY(hipMemcpy(d_b, beta, nbeta * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = bodyfit_forward_offsets_device(p, d_x, d_b, d_o, offsets_frame_stride, d_j, d_c, 3LL * m->V, nullptr)) return rc;
  p->async_pending = false;   // (NULL stream, waited for below)
  if (njt) HIP_TRY(hipMemcpy(joints, d_j, njt * sizeof(double), hipMemcpyDeviceToHost));
  if (ncl) HIP_TRY(hipMemcpy(cloud, d_c, ncl * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return BODYFIT_OK;
}

double bodyfit_mean_pixel_error(int n_kp, const int* jid, const double* uv, const double* joints, double fx,
                                double fy, double cx, double cy) {
  if (n_kp <= 0) return 0.0;  // include/Utils.h:106
  double sum = 0.0;
  for (int k = 0; k < n_kp; ++k) {
    const double* J = joints + 3 * jid[k];
    const double u = fx * J[0] / J[2] + cx, v = fy * J[1] / J[2] + cy;
    sum += std::hypot(u - uv[2 * k], v - uv[2 * k + 1]);
  }
  return sum / n_kp;
}

}  // extern "C"
