// api_blocks.hip — the Ceres block server of the C ABI in include/bodyfit.h (include/bodyfit_ceres.h calls it).
#include "host_state.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

using namespace bodyfit;

extern "C" {

// ------------------------------------------------------------------------------------------------
// ceres::CostFunction::Evaluate for one block, served from the cached sweep when the caller's
// parameters match it; otherwise the affected frame is re-evaluated on the device first.
// ------------------------------------------------------------------------------------------------
// kinds 0 / 1 of bodyfit_evaluate_block from the cached sweep (page-locked mirrors of the last bodyfit_evaluate_batch)
static void serve_block(bodyfit_problem* p, int kind, int index, int frame, double* residuals, double** jacobians) {
  const bodyfit_model* m = p->m;
  const int nJ = m->nJ, nS = m->nS, npose = dims(p).npose, D = 3 * (nJ - 1);
  const bodyfit_layout& L = p->lay;
  const bool has_beta = dims(p).has_beta;
  {
  if (kind == 0) {
    residuals[0] = p->c_r[2 * (size_t)index];
    residuals[1] = p->c_r[2 * (size_t)index + 1];
    if (jacobians && p->cache_packed) {
      // packed cache: the keypoint's present blocks in block order, each ALREADY in Ceres' layout ([2][size] row-major); the
      // others are zero.  Where a block starts comes from a per-keypoint table made with the pack tables: a present 3-column
      // block is one 48-byte copy, an absent one 48 bytes of zeros (at C3 the 6,400 reprojection blocks of an evaluation point
      // are three quarters of the Ceres-side time)
      const double* __restrict__ P = p->c_Jp.data() + p->pk_off[index];
      const short* __restrict__ src = p->pk_src.data() + (size_t)index * 32;
      const int nj3 = 3 + (nJ - 1);
      if (double* J = jacobians[0]) {
        const int a = src[0];
        if (a >= 0) { J[0] = P[a]; J[1] = P[a + 1]; } else { J[0] = 0.0; J[1] = 0.0; }
      }
      for (int blk = 1; blk < nj3; ++blk) {
        double* __restrict__ J = jacobians[blk];
        if (!J) continue;
        const int a = src[blk];
        if (a >= 0) __builtin_memcpy(J, P + a, 48);
        else __builtin_memset(J, 0, 48);
      }
      if (has_beta) {
        if (double* J = jacobians[nj3]) {
          const int a = src[nj3];
          if (a >= 0) std::memcpy(J, P + a, (size_t)2 * nS * sizeof(double));
          else std::memset(J, 0, (size_t)2 * nS * sizeof(double));
        }
      }
    } else if (jacobians) {
      const double* J0 = p->c_J.data() + (size_t)(2 * index) * L.n_cols;
      const double* J1 = J0 + L.n_cols;
      const int nblocks = 3 + (nJ - 1) + (has_beta ? 1 : 0);
      for (int blk = 0; blk < nblocks; ++blk) {
        if (!jacobians[blk]) continue;
        const int off = blk == 0 ? 0 : (blk == 1 ? 1 : (blk == 2 ? 4 : (blk < 3 + (nJ - 1) ? 7 + 3 * (blk - 3) : npose)));
        const int sz = blk == 0 ? 1 : (blk < 3 + (nJ - 1) ? 3 : nS);
        for (int i = 0; i < sz; ++i) {
          jacobians[blk][i] = J0[off + i];
          jacobians[blk][sz + i] = J1[off + i];
        }
      }
    }
  } else {
    const int nRes = L.prior_rows_per_frame;
    const double* r = p->c_r.data() + p->row_prior + (size_t)frame * nRes;
    std::memcpy(residuals, r, (size_t)nRes * sizeof(double));
    if (jacobians) {
      const double bp = p->desc.beta_pose;
      const int comp = p->c_comp[frame];
      for (int j = 0; j < nJ - 1; ++j) {
        if (!jacobians[j]) continue;
        double* Jb = jacobians[j];  // nRes x 3 row-major (include/Sim3BA.h:293,306)
        if (!(p->has_gmm && !p->gmm_jt.empty())) std::fill(Jb, Jb + (size_t)nRes * 3, 0.0);
        if (p->has_gmm && !p->gmm_jt.empty()) {
          // beta_pose L_k^T, one joint's three columns as the contiguous [nRes][3] block Ceres asks for (built once per problem:
          // the transposed walk over L_k was most of a prior block's Evaluate)
          std::memcpy(Jb, p->gmm_jt.data() + ((size_t)comp * (nJ - 1) + j) * nRes * 3, (size_t)nRes * 3 * sizeof(double));
        } else if (p->has_gmm) {
          const double* Lk = p->desc.gmm->prec_cho.data() + (size_t)comp * D * D;
          for (int row = 0; row < D; ++row)
            for (int c = 0; c < 3; ++c) Jb[(size_t)row * 3 + c] = Lk[(size_t)(3 * j + c) * D + row] * bp;  // :298-299
        } else {
          for (int c = 0; c < 3; ++c) Jb[(size_t)(3 * j + c) * 3 + c] = bp;  // :308-309
        }
      }
    }
  }
}
}

int bodyfit_evaluate_block(bodyfit_problem* p, int kind, int index, const double* const* parameters,
                           double* residuals, double** jacobians) {
  if (!p || !parameters || !residuals) return fail(BODYFIT_ERR_INVALID, "null argument");
  const bodyfit_model* m = p->m;
  const int nJ = m->nJ, nS = m->nS;
  const bodyfit_layout& L = p->lay;
  const auto [npose, has_beta, npar, nbeta_all] = dims(p);
  if (kind == 1) {  // pose prior: constant-structure Jacobian, evaluate through the batch of frame `index`
    if (index < 0 || index >= p->d.F || L.prior_rows_per_frame == 0) return fail(BODYFIT_ERR_INVALID, "bad prior block");
  }
  if (kind == 2) {
    if (L.shape_rows == 0) return fail(BODYFIT_ERR_INVALID, "no shape prior in this problem");
    const double bs = p->desc.beta_shape;
    for (int i = 0; i < nS; ++i) residuals[i] = bs * parameters[0][i];          // include/Sim3BA.h:336
    if (jacobians && jacobians[0]) {
      std::fill(jacobians[0], jacobians[0] + (size_t)nS * nS, 0.0);
      for (int i = 0; i < nS; ++i) jacobians[0][(size_t)i * nS + i] = bs;       // :338-340
    }
    return BODYFIT_OK;
  }
  if (kind == 3) {
    const double lam = p->desc.lambda_temporal;
    for (int i = 0; i < 3; ++i) residuals[i] = (parameters[0][i] - parameters[1][i]) * lam;  // MultiFrameBA.h:24
    if (jacobians) {
      for (int b = 0; b < 2; ++b)
        if (jacobians[b]) {
          std::fill(jacobians[b], jacobians[b] + 9, 0.0);
          for (int i = 0; i < 3; ++i) jacobians[b][i * 3 + i] = b == 0 ? lam : -lam;
        }
    }
    return BODYFIT_OK;
  }
  if (kind != 0 && kind != 1) return fail(BODYFIT_ERR_INVALID, "unknown block kind");
  int frame;
  if (kind == 0) {
    if (index < 0 || index >= L.n_keypoints) return fail(BODYFIT_ERR_INVALID, "keypoint index out of range");
    frame = p->kp_frame[index];
  } else {
    frame = index;
  }
  // gather the caller's parameter blocks into the packed frame row (stack arrays: this function runs once per residual
  // block and Ceres thread, nothing on its hit path allocates)
  double x[kFrameParams] = {0.0}, b[kMaxShape] = {0.0};
  if (kind == 0) {
    x[0] = parameters[0][0];
    for (int i = 0; i < 3; ++i) { x[1 + i] = parameters[1][i]; x[4 + i] = parameters[2][i]; }
    for (int j = 1; j < nJ; ++j)
      for (int i = 0; i < 3; ++i) x[7 + 3 * (j - 1) + i] = parameters[3 + (j - 1)][i];
    if (has_beta)
      for (int i = 0; i < nS; ++i) b[i] = parameters[3 + (nJ - 1)][i];
  } else {
    for (int j = 1; j < nJ; ++j)
      for (int i = 0; i < 3; ++i) x[7 + 3 * (j - 1) + i] = parameters[j - 1][i];
  }
  {
    std::unique_lock<std::mutex> lock(p->mu);
    bool hit = p->cache_valid && (p->cache_has_jac || !jacobians);
    if (hit) {
      const double* cx = p->c_params.data() + (size_t)frame * npose;
      const int i0 = (kind == 0) ? 0 : 7;
      hit = p->c_npar == npar && std::memcmp(cx + i0, x + i0, (size_t)(npose - i0) * sizeof(double)) == 0;
      if (hit && kind == 0 && has_beta) {
        const double* cb = p->c_beta.data() + (p->desc.beta_per_frame ? (size_t)frame * nS : 0);
        hit = std::memcmp(cb, b, (size_t)nS * sizeof(double)) == 0;
      }
    }
    if (!hit) {
      // refresh the cached parameter set with this frame's values and sweep again
      std::vector<double> par(p->c_params.data(), p->c_params.data() + p->c_npar), be(p->c_beta.data(), p->c_beta.data() + p->c_nbeta);
      if (par.size() != npar) {
        par.assign(npar, 0.0);
        for (int f = 0; f < p->n_param_rows; ++f) { par[(size_t)f * npose] = 1.0; par[(size_t)f * npose + 6] = 3.0; }
      }
      const size_t nb = nbeta_all;
      if (be.size() != nb) be.assign(nb, 0.0);
      const int i0 = (kind == 0) ? 0 : 7;
      std::memcpy(par.data() + (size_t)frame * npose + i0, x + i0, (size_t)(npose - i0) * sizeof(double));
      if (kind == 0 && has_beta)
        std::memcpy(be.data() + (p->desc.beta_per_frame ? (size_t)frame * nS : 0), b, (size_t)nS * sizeof(double));
      lock.unlock();
      int rc = bodyfit_evaluate_batch(p, par.data(), nb ? be.data() : nullptr, nullptr, nullptr, nullptr, 1);
      if (rc) return rc;
      lock.lock();
    }
    serve_block(p, kind, index, frame, residuals, jacobians);
  }
  return BODYFIT_OK;
}

// The EvaluationCallback form (include/bodyfit_ceres.h: SweepCallback): the caller guarantees that the cached sweep IS the point
// Ceres is evaluating (PrepareForEvaluation ran for it), so kinds 0 / 1 are served without gathering and comparing the block's
// 76 parameters and without the problem's lock (the cache is only written by the callback, between evaluations): ~4x less host
// time per block, and Ceres' evaluation threads do not serialise on it.  Kinds 2 / 3 are functions of their parameters alone.
int bodyfit_evaluate_block_cached(bodyfit_problem* p, int kind, int index, const double* const* parameters,
                                  double* residuals, double** jacobians) {
  if (!p || !residuals) return fail(BODYFIT_ERR_INVALID, "null argument");
  if (kind == 2 || kind == 3) return bodyfit_evaluate_block(p, kind, index, parameters, residuals, jacobians);
  if (kind != 0 && kind != 1) return fail(BODYFIT_ERR_INVALID, "unknown block kind");
  if (!p->cache_valid || (jacobians && !p->cache_has_jac))
    return fail(BODYFIT_ERR_INVALID, "bodyfit_evaluate_block_cached: no sweep cached for this evaluation (EvaluationCallback not run?)");
  int frame;
  if (kind == 0) {
    if (index < 0 || index >= p->lay.n_keypoints) return fail(BODYFIT_ERR_INVALID, "keypoint index out of range");
    frame = p->kp_frame[index];
  } else {
    if (index < 0 || index >= p->d.F || p->lay.prior_rows_per_frame == 0) return fail(BODYFIT_ERR_INVALID, "bad prior block");
    frame = index;
  }
  serve_block(p, kind, index, frame, residuals, jacobians);
  return BODYFIT_OK;
}

}  // extern "C"
