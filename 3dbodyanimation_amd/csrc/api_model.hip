// api_model.hip — model upload (operand packing for the MFMA kernel) and the GMM precompute of the C ABI in include/bodyfit.h.
#include "host_state.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

using namespace bodyfit;

namespace {

bool chol_lower(std::vector<double>& A, int n) {
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    A[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
      A[(size_t)i * n + j] = s / d;
    }
    for (int i = 0; i < j; ++i) A[(size_t)i * n + j] = 0.0;
  }
  return true;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------
int bodyfit_model_create(const bodyfit_model_desc* desc, int device, bodyfit_model** out) {
  if (!desc || !out) return fail(BODYFIT_ERR_INVALID, "null argument");
  *out = nullptr;
  const int V = desc->n_verts, nJ = desc->n_joints, nS = desc->n_shape;
  const int P = desc->posedirs ? desc->n_pose_feat : 0;
  const int nL = desc->n_landmarks;
  if (V <= 0 || nJ <= 0 || nJ > kMaxJoints || nS < 0 || nS > kMaxShape)
    return fail(BODYFIT_ERR_INVALID, "unsupported model size (n_joints <= 24, n_shape <= 10)");
  if (P != 0 && P != 9 * (nJ - 1)) return fail(BODYFIT_ERR_INVALID, "n_pose_feat must be 9 (n_joints - 1)");
  if (nL < 0 || nL > kMaxLandmarks) return fail(BODYFIT_ERR_INVALID, "too many landmarks (<= 32)");
  if (!desc->v_template || !desc->shapedirs || !desc->j_regressor || !desc->weights || !desc->parent)
    return fail(BODYFIT_ERR_INVALID, "missing model tensor");
  if (desc->parent[0] != -1) return fail(BODYFIT_ERR_INVALID, "parent[0] must be -1 (npz_fixer convention)");
  for (int j = 1; j < nJ; ++j)
    if (desc->parent[j] < 0 || desc->parent[j] >= j)
      return fail(BODYFIT_ERR_INVALID, "kintree must be topologically ordered with a single root");
  {
    // the frame role walks a joint's ancestors from a packed list of 12 entries (root excluded): depth <= 13
    std::vector<int> depth(nJ, 0);
    for (int j = 1; j < nJ; ++j)
      if ((depth[j] = depth[desc->parent[j]] + 1) > kMaxDepth)
        return fail(BODYFIT_ERR_INVALID, "kintree deeper than 13 levels below the root (the ancestor walk holds 12 joints)");
  }
  for (int l = 0; l < nL; ++l)
    if (desc->landmark_vid[l] < 0 || desc->landmark_vid[l] >= V) return fail(BODYFIT_ERR_INVALID, "landmark vertex id");
  const int nReg = desc->n_kp_regressors;
  if (nReg < 0 || (nReg > 0 && (!desc->kpreg_offset || !desc->kpreg_vid || !desc->kpreg_weight)))
    return fail(BODYFIT_ERR_INVALID, "keypoint regressors: missing arrays");
  for (int r = 0; r < nReg; ++r) {
    if (desc->kpreg_offset[r + 1] <= desc->kpreg_offset[r] || desc->kpreg_offset[0] != 0)
      return fail(BODYFIT_ERR_INVALID, "keypoint regressors: offsets must start at 0 and every row needs an entry");
    for (int e = desc->kpreg_offset[r]; e < desc->kpreg_offset[r + 1]; ++e)
      if (desc->kpreg_vid[e] < 0 || desc->kpreg_vid[e] >= V) return fail(BODYFIT_ERR_INVALID, "keypoint regressor vertex id");
  }

  HIP_TRY(hipSetDevice(device));
  bodyfit_model* m = new bodyfit_model();
  std::unique_ptr<bodyfit_model> guard(m);
  m->device = device;
  HIP_TRY(hipDeviceGetAttribute(&m->n_cus, hipDeviceAttributeMultiprocessorCount, device));
  m->V = V; m->nJ = nJ; m->nS = nS; m->P = P; m->nL = nL;
  m->parent.assign(desc->parent, desc->parent + nJ);

  // joint regression on the device: J0 = Jreg . v_template, S = Jreg . shapedirs
  m->J0.assign((size_t)nJ * 3, 0.0);
  m->S.assign((size_t)nJ * 3 * std::max(nS, 1), 0.0);
  {
    Allocs tmp;
    double *d_reg, *d_vt, *d_sd, *d_j0, *d_s;
    HIP_TRY(tmp.alloc(&d_reg, (size_t)nJ * V));
    HIP_TRY(tmp.alloc(&d_vt, (size_t)V * 3));
    HIP_TRY(tmp.alloc(&d_sd, (size_t)V * 3 * std::max(nS, 1)));
    HIP_TRY(tmp.alloc(&d_j0, (size_t)nJ * 3));
    HIP_TRY(tmp.alloc(&d_s, (size_t)nJ * 3 * std::max(nS, 1)));
    HIP_TRY(hipMemcpy(d_reg, desc->j_regressor, (size_t)nJ * V * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_vt, desc->v_template, (size_t)V * 3 * sizeof(double), hipMemcpyHostToDevice));
    launch_regress(nJ, V, 3, d_reg, d_vt, d_j0, nullptr);
    if (nS > 0) {
      HIP_TRY(hipMemcpy(d_sd, desc->shapedirs, (size_t)V * 3 * nS * sizeof(double), hipMemcpyHostToDevice));
      launch_regress(nJ, V, 3 * nS, d_reg, d_sd, d_s, nullptr);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(m->J0.data(), d_j0, (size_t)nJ * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (nS > 0)
      HIP_TRY(hipMemcpy(m->S.data(), d_s, (size_t)nJ * 3 * nS * sizeof(double), hipMemcpyDeviceToHost));
  }
  const std::vector<double>& J0 = m->J0;
  const std::vector<double>& S = m->S;

  // rest offsets (include/Sim3BA.h:372-392) and the shape-difference tables
  m->offset.assign((size_t)nJ * 3, 0.0);
  std::vector<double> Jc0((size_t)nJ * 3), dS((size_t)nJ * 3 * std::max(nS, 1), 0.0), Sc(dS.size(), 0.0);
  for (int j = 0; j < nJ; ++j)
    for (int a = 0; a < 3; ++a) Jc0[j * 3 + a] = J0[j * 3 + a] - J0[a];
  for (int j = 1; j < nJ; ++j)
    for (int a = 0; a < 3; ++a) m->offset[j * 3 + a] = Jc0[j * 3 + a] - Jc0[m->parent[j] * 3 + a];
  for (int j = 0; j < nJ; ++j)
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < nS; ++k) {
        const double sj = S[(size_t)(j * 3 + a) * nS + k];
        const int pj = m->parent[j];
        dS[(size_t)(j * 3 + a) * nS + k] = sj - (pj >= 0 ? S[(size_t)(pj * 3 + a) * nS + k] : 0.0);
        Sc[(size_t)(j * 3 + a) * nS + k] = sj - S[(size_t)a * nS + k];
      }
  // depth levels and ancestor masks
  std::vector<int> depth(nJ, 0);
  int maxd = 0;
  for (int j = 1; j < nJ; ++j) { depth[j] = depth[m->parent[j]] + 1; maxd = std::max(maxd, depth[j]); }
  std::vector<int> level_off(maxd + 1, 0), level_joint;
  for (int d = 1; d <= maxd; ++d) {
    level_off[d - 1] = (int)level_joint.size();
    for (int j = 1; j < nJ; ++j)
      if (depth[j] == d) level_joint.push_back(j);
  }
  level_off[maxd] = (int)level_joint.size();
  std::vector<unsigned> anc(nJ, 0u);
  for (int j = 1; j < nJ; ++j)
    for (int k = m->parent[j]; k > 0; k = m->parent[k]) anc[j] |= (1u << k);

  DevModel& d = m->d;
  d.V = V; d.nJ = nJ; d.nS = nS; d.P = P; d.nL = nL; d.nLevels = maxd;
  d.nVTiles = (V + kVTile - 1) / kVTile;
  // (parent, anc_mask, anc_chain, offset, dS, Jc0, Sc and the landmark tables: one block, bodyfit_device.h kTab*)
  std::vector<unsigned char> tabA(kTabBytes, 0);
  auto put = [&](int off, const void* src, size_t bytes) { if (bytes) std::memcpy(tabA.data() + off, src, bytes); };
  if (nJ > kMaxJoints || nS > kMaxShape) return fail(BODYFIT_ERR_INVALID, "model: at most 24 joints and 10 shape coefficients");
  put(kTabParent, m->parent.data(), m->parent.size() * sizeof(int));
  HIP_TRY(m->mem.upload(&d.level_off, level_off));
  HIP_TRY(m->mem.upload(&d.level_joint, level_joint));
  put(kTabAnc, anc.data(), anc.size() * sizeof(unsigned));
  // the same ancestors as a packed walk list: nearest first, 5 bits each, 0-terminated (joint ids 1..23; depth <= kMaxDepth)
  std::vector<unsigned long long> chain(nJ, 0ull);
  for (int j = 1; j < nJ; ++j) {
    int lvl = 0;
    for (int k = m->parent[j]; k > 0; k = m->parent[k], ++lvl) chain[j] |= (unsigned long long)k << (5 * lvl);   // (lvl < 12: kMaxDepth)
  }
  put(kTabChain, chain.data(), chain.size() * sizeof(unsigned long long));
  put(kTabOffset, m->offset.data(), m->offset.size() * sizeof(double));
  put(kTabDS, dS.data(), dS.size() * sizeof(double));
  put(kTabJc0, Jc0.data(), Jc0.size() * sizeof(double));
  put(kTabSc, Sc.data(), Sc.size() * sizeof(double));

  // landmark slots of the frame kernel: the caller's one-hot landmarks, then the pseudo-vertices of the regressor rows.
  // A row  k = sum_i a_i posed(v_i),  posed(v) = sum_j W_vj (A_j (rest_v - Jc_j) + P_j),  collapses per skinning joint j to
  //   s_j (A_j (r_j - Jc_j) + P_j),   s_j = sum_i a_i W_ij,   r_j = sum_i a_i W_ij rest_i / s_j
  // (rest_i = template + shapedirs beta + posedirs feat is linear in the vertex rows, and the coefficients a_i W_ij / s_j
  // sum to one, so r_j is itself a "vertex" with rows combined the same way): one slot per joint with s_j != 0, skinned to
  // that joint alone with weight s_j.  The kernel adds the slots of a row up (position and Jacobian terms) into the first.
  {
    struct Slot { std::vector<std::pair<int, double>> w; std::vector<std::pair<int, double>> src; };   // (joint, weight), (vertex, coefficient)
    std::vector<Slot> slots;
    std::vector<int> gcount;
    for (int l = 0; l < nL; ++l) {
      Slot sl;
      const int vid = desc->landmark_vid[l];
      for (int j = 0; j < nJ; ++j) {
        const double w = desc->weights[(size_t)vid * nJ + j];
        if (w != 0.0) sl.w.emplace_back(j, w);
      }
      if ((int)sl.w.size() > kMaxLmNnz) return fail(BODYFIT_ERR_INVALID, "landmark vertex has more than 8 skinning weights");
      sl.src.emplace_back(vid, 1.0);
      slots.push_back(std::move(sl));
      gcount.push_back(1);
    }
    m->nReg = nReg;
    for (int r = 0; r < nReg; ++r) {
      m->reg_slot.push_back((int)slots.size());
      const int first = (int)slots.size();
      for (int j = 0; j < nJ; ++j) {
        double sj = 0.0;
        for (int e = desc->kpreg_offset[r]; e < desc->kpreg_offset[r + 1]; ++e)
          sj += desc->kpreg_weight[e] * desc->weights[(size_t)desc->kpreg_vid[e] * nJ + j];
        if (sj == 0.0) continue;
        Slot sl;
        sl.w.emplace_back(j, sj);
        for (int e = desc->kpreg_offset[r]; e < desc->kpreg_offset[r + 1]; ++e) {
          const double c = desc->kpreg_weight[e] * desc->weights[(size_t)desc->kpreg_vid[e] * nJ + j];
          if (c != 0.0) sl.src.emplace_back(desc->kpreg_vid[e], c / sj);
        }
        slots.push_back(std::move(sl));
        gcount.push_back(0);
      }
      if ((int)slots.size() == first) return fail(BODYFIT_ERR_INVALID, "keypoint regressor row without skinning weight");
      gcount[first] = (int)slots.size() - first;
    }
    const int nSlots = (int)slots.size();
    if (nSlots > kMaxLandmarks)
      return fail(BODYFIT_ERR_INVALID, "landmarks + regressor pseudo-vertices (one per row and skinning joint) must be <= 32");
    d.nL = nSlots;
    // fixed-stride skinning weights per slot: kMaxLmNnz entries padded with weight 0; woff[l] = count
    std::vector<int> woff(nSlots + 1, 0), wj((size_t)std::max(nSlots, 1) * kMaxLmNnz, 0);
    std::vector<double> ww((size_t)std::max(nSlots, 1) * kMaxLmNnz, 0.0), vt((size_t)nSlots * 3, 0.0),
        sd((size_t)nSlots * 3 * std::max(nS, 1), 0.0), pd((size_t)std::max(nSlots, 1) * 27 * 32, 0.0);
    for (int l = 0; l < nSlots; ++l) {
      const Slot& sl = slots[l];
      for (size_t i = 0; i < sl.w.size(); ++i) {
        wj[(size_t)l * kMaxLmNnz + i] = sl.w[i].first;
        ww[(size_t)l * kMaxLmNnz + i] = sl.w[i].second;
      }
      woff[l] = (int)sl.w.size();
      for (const auto& [vid, c] : sl.src)
        for (int a = 0; a < 3; ++a) {
          vt[l * 3 + a] += c * (desc->v_template[(size_t)vid * 3 + a] - J0[a]);
          for (int k = 0; k < nS; ++k)
            sd[(size_t)(l * 3 + a) * nS + k] += c * (desc->shapedirs[((size_t)vid * 3 + a) * nS + k] - S[(size_t)a * nS + k]);
          // [l][a * 9 + e][k - 1]: the 9 (k - 1) + e pose-feature column of joint k, joint-minor, so that the lanes of a
          // half-wave (one joint each) read 184 contiguous bytes per (a, e)
          for (int k = 0; k < P; ++k)
            pd[((size_t)l * 27 + a * 9 + k % 9) * 32 + k / 9] += c * desc->posedirs[((size_t)vid * 3 + a) * P + k];
        }
    }
    put(kTabLmWoff, woff.data(), woff.size() * sizeof(int));
    put(kTabLmWj, wj.data(), wj.size() * sizeof(int));
    put(kTabLmWw, ww.data(), ww.size() * sizeof(double));
    put(kTabLmVt, vt.data(), vt.size() * sizeof(double));
    put(kTabLmSd, sd.data(), sd.size() * sizeof(double));
    {
      const unsigned char* dev = nullptr;
      HIP_TRY(m->mem.upload(&dev, tabA));
      d.tabA = dev;
      d.parent = reinterpret_cast<const int*>(dev + kTabParent);
      d.anc_mask = reinterpret_cast<const unsigned*>(dev + kTabAnc);
      d.anc_chain = reinterpret_cast<const unsigned long long*>(dev + kTabChain);
      d.offset = reinterpret_cast<const double*>(dev + kTabOffset);
      d.dS = reinterpret_cast<const double*>(dev + kTabDS);
      d.Jc0 = reinterpret_cast<const double*>(dev + kTabJc0);
      d.Sc = reinterpret_cast<const double*>(dev + kTabSc);
      d.lm_woff = reinterpret_cast<const int*>(dev + kTabLmWoff);
      d.lm_wj = reinterpret_cast<const int*>(dev + kTabLmWj);
      d.lm_ww = reinterpret_cast<const double*>(dev + kTabLmWw);
      d.lm_vt = reinterpret_cast<const double*>(dev + kTabLmVt);
      d.lm_sd = reinterpret_cast<const double*>(dev + kTabLmSd);
    }
    HIP_TRY(m->mem.upload(&d.lm_pd, pd));
    d.lm_gcount = nullptr;
    if (nReg > 0) {
      gcount.resize(kMaxLandmarks, 0);
      HIP_TRY(m->mem.upload(&d.lm_gcount, gcount));
    }
  }

  // mesh operands in MFMA fragment order
  {
    const int nVT = d.nVTiles;
    std::vector<uint16_t> dirsB((size_t)nVT * kBlendKSteps * 3 * 2 * 64 * 8, 0);
    std::vector<float> vtB((size_t)nVT * 3 * 32, 0.0f);
    auto put = [&](int vt_i, int c, int col, int k, float x) {   // 32x32x16: B[k = 16 ks + 8 h + j][col]
      const int ks = k >> 4, hh = (k >> 3) & 1, jj = k & 7;
      const uint16_t hi = f32_to_bf16(x);
      const uint16_t lo = f32_to_bf16(x - bf16_to_f32(hi));
      const size_t base = ((((size_t)vt_i * kBlendKSteps + ks) * 3 + c) * 2) * 64 * 8;
      dirsB[base + (size_t)(hh * 32 + col) * 8 + jj] = hi;
      dirsB[base + (size_t)64 * 8 + (size_t)(hh * 32 + col) * 8 + jj] = lo;
    };
    std::vector<uint32_t> wIdx((size_t)nVT * 32, 0u);
    std::vector<float> wVal((size_t)nVT * 32 * 4, 0.0f);
    for (int vt_i = 0; vt_i < nVT; ++vt_i)
      for (int col = 0; col < 32; ++col) {
        const int v = vt_i * 32 + col;
        if (v >= V) continue;
        for (int c = 0; c < 3; ++c) {
          vtB[((size_t)vt_i * 3 + c) * 32 + col] = (float)(desc->v_template[(size_t)v * 3 + c] - J0[c]);
          {
            // the template rides in the contraction on two of its padding slots (coefficient 1 in k_frame_resjac's
            // fragments): slot 217 carries its first 16 bits (bf16 hi + lo), slot 218 what those left over
            const float t0 = vtB[((size_t)vt_i * 3 + c) * 32 + col];
            const uint16_t h0 = f32_to_bf16(t0);
            const uint16_t l0 = f32_to_bf16(t0 - bf16_to_f32(h0));
            put(vt_i, c, col, kPoseFeat + kMaxShape, t0);
            put(vt_i, c, col, kPoseFeat + kMaxShape + 1, t0 - (bf16_to_f32(h0) + bf16_to_f32(l0)));
          }
          for (int k = 0; k < nS && k < kMaxShape; ++k)
            put(vt_i, c, col, kPoseFeat + k, (float)(desc->shapedirs[((size_t)v * 3 + c) * nS + k] - S[(size_t)c * nS + k]));
          for (int k = 0; k < P && k < kPoseFeat; ++k) put(vt_i, c, col, k, (float)desc->posedirs[((size_t)v * 3 + c) * P + k]);
        }
      }
    // Skinning weights: <= 4 (joint, weight) entries per vertex, lane = vertex.  The kernel's i-th ds_read_b128 of a row
    // has each lane fetch 16 B of its i-th joint's transform (48-byte records), served in groups of 16 lanes; two lanes
    // of a group collide on LDS banks exactly when their i-th joints differ by 16.  The order of a vertex's entries is
    // free, so it is chosen (greedily, per tile) to keep "joint mod 16" unique per group and slot; unused slots take
    // weight 0 and a joint that broadcasts or falls on a free residue.
    const int group_of_col[32] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1};
    for (int vt_i = 0; vt_i < nVT; ++vt_i) {
      int used[2][kMeshNnz][16];   // joint + 1 occupying residue r of (group, slot), 0 = free
      std::memset(used, 0, sizeof(used));
      for (int col = 0; col < 32; ++col) {
        const int v = vt_i * 32 + col, g = group_of_col[col];
        int js[kMeshNnz], cnt = 0;
        double ws[kMeshNnz];
        if (v < V)
          for (int j = 0; j < nJ; ++j) {
            const double w = desc->weights[(size_t)v * nJ + j];
            if (w == 0.0) continue;
            if (cnt < kMeshNnz) { js[cnt] = j; ws[cnt] = w; }
            ++cnt;
          }
        if (cnt > kMeshNnz) { m->mesh_ok = false; cnt = kMeshNnz; }
        int perm[kMeshNnz] = {0, 1, 2, 3}, best[kMeshNnz] = {0, 1, 2, 3}, best_cost = 1 << 30;
        do {   // slot perm[e] receives entry e (e < cnt)
          int cost = 0;
          for (int e = 0; e < cnt; ++e) {
            const int u = used[g][perm[e]][js[e] & 15];
            cost += (u != 0 && u != js[e] + 1);
          }
          if (cost < best_cost) { best_cost = cost; std::copy(perm, perm + kMeshNnz, best); }
        } while (best_cost > 0 && std::next_permutation(perm, perm + kMeshNnz));
        int slot_j[kMeshNnz];
        float slot_w[kMeshNnz];
        bool filled[kMeshNnz] = {false, false, false, false};
        for (int e = 0; e < cnt; ++e) { slot_j[best[e]] = js[e]; slot_w[best[e]] = (float)ws[e]; filled[best[e]] = true; }
        for (int sl = 0; sl < kMeshNnz; ++sl) {
          if (!filled[sl]) {
            int pick = -1;
            for (int r = 0; r < 16 && pick < 0; ++r) if (used[g][sl][r]) pick = used[g][sl][r] - 1;   // broadcast
            slot_j[sl] = pick < 0 ? 0 : pick;
            slot_w[sl] = 0.0f;
          }
          if (!used[g][sl][slot_j[sl] & 15]) used[g][sl][slot_j[sl] & 15] = slot_j[sl] + 1;
        }
        uint32_t packed = 0;
        for (int sl = 0; sl < kMeshNnz; ++sl) {
          packed |= ((uint32_t)slot_j[sl]) << (8 * sl);
          wVal[((size_t)vt_i * 32 + col) * 4 + sl] = slot_w[sl];
        }
        wIdx[(size_t)vt_i * 32 + col] = packed;
      }
    }
    HIP_TRY(m->mem.upload(&d.dirsB, dirsB));
    HIP_TRY(m->mem.upload(&d.vtB, vtB));
    HIP_TRY(m->mem.upload(&d.wIdx, wIdx));
    HIP_TRY(m->mem.upload(&d.wVal, wVal));
    m->h_wIdx = std::move(wIdx);
    m->h_wVal = std::move(wVal);
  }
  *out = guard.release();
  return BODYFIT_OK;
}

void bodyfit_model_destroy(bodyfit_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  BlockPool::get().trim(m->device);   // (blocks of this device's destroyed problems)
  delete m;
}

int bodyfit_model_get_derived(const bodyfit_model* m, double* joints0, double* joint_shape_reg, double* offset) {
  if (!m) return fail(BODYFIT_ERR_INVALID, "null model");
  if (joints0) std::memcpy(joints0, m->J0.data(), (size_t)m->nJ * 3 * sizeof(double));
  if (joint_shape_reg) std::memcpy(joint_shape_reg, m->S.data(), (size_t)m->nJ * 3 * m->nS * sizeof(double));
  if (offset) std::memcpy(offset, m->offset.data(), (size_t)m->nJ * 3 * sizeof(double));
  return BODYFIT_OK;
}

// ------------------------------------------------------------------------------------------------
// GMM (ark::GaussianMixture restated: precision Cholesky + SMPLify max-mixture constants)
// ------------------------------------------------------------------------------------------------
int bodyfit_gmm_create(int K, int D, const double* weights, const double* means, const double* covs,
                       double resid_scale, int device, bodyfit_gmm** out) {
  if (!out || !weights || !means || !covs || K <= 0 || K > 8 || D <= 0 || D > 72)
    return fail(BODYFIT_ERR_INVALID, "bad GMM arguments (1..8 components, dimension <= 72)");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<bodyfit_gmm> g(new bodyfit_gmm());
  g->device = device;
  g->prec_cho.assign((size_t)K * D * D, 0.0);
  g->neg_log_w.assign(K, 0.0);
  g->mean.assign(means, means + (size_t)K * D);
  std::vector<double> hld(K);
  for (int k = 0; k < K; ++k) {
    std::vector<double> C(covs + (size_t)k * D * D, covs + (size_t)(k + 1) * D * D);
    if (!chol_lower(C, D)) return fail(BODYFIT_ERR_NUMERIC, "GMM covariance is not SPD");
    double ld = 0;
    for (int i = 0; i < D; ++i) ld += std::log(C[(size_t)i * D + i]);
    hld[k] = ld;
    // Y = C^{-1} by forward substitution on the identity; precision = Y^T Y
    std::vector<double> Y((size_t)D * D, 0.0);
    for (int c = 0; c < D; ++c)
      for (int r = c; r < D; ++r) {
        double s = (r == c) ? 1.0 : 0.0;
        for (int t = c; t < r; ++t) s -= C[(size_t)r * D + t] * Y[(size_t)t * D + c];
        Y[(size_t)r * D + c] = s / C[(size_t)r * D + r];
      }
    std::vector<double> Pm((size_t)D * D, 0.0);
    for (int r = 0; r < D; ++r)
      for (int c = 0; c <= r; ++c) {
        double s = 0;
        for (int t = r; t < D; ++t) s += Y[(size_t)t * D + r] * Y[(size_t)t * D + c];
        Pm[(size_t)r * D + c] = s;
        Pm[(size_t)c * D + r] = s;
      }
    g->prec.insert(g->prec.end(), Pm.begin(), Pm.end());
    if (!chol_lower(Pm, D)) return fail(BODYFIT_ERR_NUMERIC, "GMM precision is not SPD");
    std::memcpy(&g->prec_cho[(size_t)k * D * D], Pm.data(), (size_t)D * D * sizeof(double));
  }
  const double mn = *std::min_element(hld.begin(), hld.end());
  for (int k = 0; k < K; ++k)
    g->neg_log_w[k] = -(std::log(weights[k]) - 0.5 * D * std::log(2.0 * M_PI) - (hld[k] - mn));
  g->d.K = K; g->d.D = D; g->d.resid_scale = resid_scale;
  HIP_TRY(g->mem.upload(&g->d.mean, g->mean));
  HIP_TRY(g->mem.upload(&g->d.prec_cho, g->prec_cho));
  HIP_TRY(g->mem.upload(&g->d.prec, g->prec));
  {
    // B-fragment order of v_mfma_f64_16x16x4_f64 (B[k = lane>>4][j = lane&15]), two column tiles per
    // 16-byte load: frag[k][ks][pair][lane][t] = L[4 ks + (lane>>4)][16 (2 pair + t) + (lane&15)], zero padded
    std::vector<double> frag((size_t)K * 18 * 3 * 64 * 2, 0.0);
    for (int k = 0; k < K; ++k)
      for (int ks = 0; ks < 18; ++ks)
        for (int pr = 0; pr < 3; ++pr)
          for (int lane = 0; lane < 64; ++lane)
            for (int t = 0; t < 2; ++t) {
              const int r = 4 * ks + (lane >> 4), c = 16 * (2 * pr + t) + (lane & 15);
              if (r < D && c < D && 2 * pr + t < 5)
                frag[((((size_t)k * 18 + ks) * 3 + pr) * 64 + lane) * 2 + t] = g->prec_cho[((size_t)k * D + r) * D + c];
            }
    HIP_TRY(g->mem.upload(&g->d.prec_frag, frag));
  }
  HIP_TRY(g->mem.upload(&g->d.neg_log_w, g->neg_log_w));
  *out = g.release();
  return BODYFIT_OK;
}

void bodyfit_gmm_destroy(bodyfit_gmm* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  delete g;
}

int bodyfit_gmm_get(const bodyfit_gmm* g, double* prec_cho, double* neg_log_w) {
  if (!g) return fail(BODYFIT_ERR_INVALID, "null gmm");
  if (prec_cho) std::memcpy(prec_cho, g->prec_cho.data(), g->prec_cho.size() * sizeof(double));
  if (neg_log_w) std::memcpy(neg_log_w, g->neg_log_w.data(), g->neg_log_w.size() * sizeof(double));
  return BODYFIT_OK;
}

}  // extern "C"
