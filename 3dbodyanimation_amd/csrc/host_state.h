// host_state.h — host-only internals shared by the C ABI translation units (api_*.hip) and the host sides of k_closest.hip and
// overlay.hip: error reporting, the owners of device and page-locked memory, the three handle structs, the sweep.
#pragma once
#include "../../include/bodyfit.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "bodyfit_device.h"
#include "solver_view.h"

namespace bodyfit {

// sets what bodyfit_last_error() returns on this thread (the string itself lives in api_core.hip) and hands the code back
inline int fail(int code, const std::string& msg) { return bodyfit_internal_fail(code, msg.c_str()); }
// an entry's rejection of its arguments: BODYFIT_ERR_INVALID with "<entry>: <what>"
inline int invalid_arg(const char* fn, const char* what) { return fail(BODYFIT_ERR_INVALID, std::string(fn) + ": " + what); }

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return ::bodyfit::fail(BODYFIT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Device blocks of destroyed problems, kept for the next problem of the same shape.  The reference's staged drivers
// (src/main_multi_frame.cpp:109-217: anchors, then one solve per sliding window, an update() after each) create and destroy
// two problems per stage; hipFree synchronises the device and unmaps — 0.6 ms per problem, 12 of the 149 ms of a staged
// 128-frame run (tools/probes/run_multi_breakdown.py).  A block is reused only for a request of exactly its size on its device;
// contents are unspecified, as hipMalloc's are (problem creation clears what it needs cleared).  Bounded: beyond kLimit bytes
// per device a block is freed at once; bodyfit_model_destroy empties its device's list.  Nothing is freed at process exit (the
// runtime may be gone by then).
class BlockPool {
 public:
  static BlockPool& get() { static BlockPool* p = new BlockPool; return *p; }
  void* take(int dev, size_t bytes) {
    std::lock_guard<std::mutex> g(mu_);
    auto& f = free_[dev];
    auto it = f.find(bytes);
    if (it == f.end()) return nullptr;
    void* p = it->second;
    f.erase(it);
    held_[dev] -= bytes;
    return p;
  }
  void give(int dev, size_t bytes, void* p) {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (held_[dev] + bytes <= kLimit) {
        free_[dev].emplace(bytes, p);
        held_[dev] += bytes;
        return;
      }
    }
    (void)hipFree(p);
  }
  void trim(int dev) {
    std::multimap<size_t, void*> drop;
    {
      std::lock_guard<std::mutex> g(mu_);
      drop.swap(free_[dev]);
      held_[dev] = 0;
    }
    for (auto& kv : drop) (void)hipFree(kv.second);
  }
 private:
  static constexpr size_t kLimit = (size_t)1 << 30;
  std::mutex mu_;
  std::map<int, std::multimap<size_t, void*>> free_;
  std::map<int, size_t> held_;
};

struct Allocs {
  struct Block { void* p; size_t bytes; int dev; };
  std::vector<Block> blocks;
  bool pooled = false;   // problems: blocks go back to the BlockPool (the owner has synchronised the device first)
  ~Allocs() {
    for (const Block& b : blocks) {
      if (pooled) BlockPool::get().give(b.dev, b.bytes, b.p);
      else (void)hipFree(b.p);
    }
  }
  template <typename T>
  hipError_t alloc(T** out, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    int dev = 0;
    (void)hipGetDevice(&dev);
    void* p = pooled ? BlockPool::get().take(dev, bytes) : nullptr;
    hipError_t e = hipSuccess;
    if (!p) e = hipMalloc(&p, bytes);
    if (!p && e != hipSuccess) {
      // out of memory while the pool sits on up to 1 GiB of blocks of other sizes: give them back and try once more
      (void)hipGetLastError();
      BlockPool::get().trim(dev);
      e = hipMalloc(&p, bytes);
    }
    if (e == hipSuccess) {
      blocks.push_back(Block{p, bytes, dev});
      *out = static_cast<T*>(p);
    }
    return e;
  }
  template <typename T>
  hipError_t upload(const T** out, const std::vector<T>& h) {
    T* p = nullptr;
    hipError_t e = alloc(&p, h.size());
    if (e != hipSuccess) return e;
    if (!h.empty()) e = hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    *out = p;
    return e;
  }
};

// a page-locked host buffer (hipHostMalloc): the host side of every copy of the Ceres-kept path.  From pageable memory the
// runtime stages a copy through its own bounce buffers in chunks, synchronously: 9 MB of Jacobian per 256-frame sweep came
// back at ~17 GB/s and the sweep's parameters went up behind a stall; page-locked, both are single DMA transfers that are
// asynchronous on the problem's copy stream.
template <typename T>
struct Pinned {
  T* p = nullptr;
  size_t n = 0;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  hipError_t ensure(size_t want) {
    if (want <= n) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; n = 0;
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, std::max<size_t>(want, 1) * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) { p = static_cast<T*>(q); n = want; }
    return e;
  }
  T* data() { return p; }
  const T* data() const { return p; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

}  // namespace bodyfit

struct bodyfit_model {
  int device = 0;
  int n_cus = 0;
  int V = 0, nJ = 0, nS = 0, P = 0, nL = 0;   // nL: the caller's one-hot landmarks (the device model's nL counts slots)
  int nReg = 0;                               // sparse keypoint regressors over posed vertices
  std::vector<int> reg_slot;                  // [nReg] first landmark slot of the row's pseudo-vertices
  bool mesh_ok = true;
  bodyfit::DevModel d{};
  std::vector<int> parent;
  std::vector<double> J0, S, offset;
  bodyfit::Allocs mem;
  // forward VJP (k_forward_vjp.hip), built on the model's first VJP and freed with the model: the operand block transposed
  // for the blend gradient, and every joint's skinning list (vertex ascending, f32 weights as the forward skins with them)
  std::vector<uint32_t> h_wIdx;
  std::vector<float> h_wVal;
  mutable std::mutex vjp_mu;
  mutable bool vjp_ready = false;
  mutable uint16_t* d_dirsT = nullptr;
  mutable int* d_csr_off = nullptr;
  mutable int* d_csr_v = nullptr;
  mutable float* d_csr_w = nullptr;
  mutable bodyfit::Allocs vjp_mem;
};

struct bodyfit_gmm {
  int device = 0;
  bodyfit::DevGmm d{};
  std::vector<double> prec_cho, neg_log_w, mean, prec;
  bodyfit::Allocs mem;
};

struct bodyfit_problem {
  const bodyfit_model* m = nullptr;
  bodyfit_problem_desc desc{};
  bodyfit_layout lay{};
  bodyfit::DevProblem d{};
  bodyfit::MeshCoef mc{};
  bodyfit::DevGmm gmm{};
  bool has_gmm = false;
  int n_param_rows = 0, n_pairs = 0;
  int row_prior = 0, row_shape = 0, row_temporal = 0;
  // host copies
  std::vector<int> kp_offset, kp_id, kp_frame;
  std::vector<double> kp_uv;
  std::vector<double> gmm_jt;   // [K][nJ - 1][prior rows][3]: beta_pose L_k^T per joint block, what a GMM prior block's Jacobian is (host path)

  // ---- sweep: the device buffers an evaluation reads and writes, and what the last sweep left in them
  double* d_params = nullptr;
  double* d_beta = nullptr;
  double* d_r = nullptr;
  double* d_J = nullptr;
  double* d_joints = nullptr;
  double* d_partials = nullptr;
  double* d_normal = nullptr;
  int* d_comp = nullptr;
  float* d_cloud = nullptr;
  double* d_frame_normal = nullptr;   // [F][87][88] per-frame normal-equation panels (window solver), on first use
  double* d_writeback = nullptr;      // [F][76] update parameters + [F][9] R0' + [F] mean pixel error, on first use
  double* d_frame_partials = nullptr; // [F][258] per-frame beta partials written by k_frame_resjac (shared-beta problems)
  int partials_tiles = 0;             // prior tiles that added their plain-cost rows behind the frame rows
  bool partials_fresh = false;        // the last sweep produced them (want_jac)
  double* armed_out66 = nullptr;      // bodyfit_arm_shared_reduction: where a folding sweep deposits [cost | g_beta | H_bb]
  unsigned fold_count = 0;            // tickets taken by the folding sweeps since the sync buffer was zeroed
  bool fold_fresh = false;            // the last sweep folded into armed_out66

  // ---- one-launch sync (k_sweep_roles): in-launch synchronisation words [error | pad | one counter per 32-frame unit], launch counter
  unsigned char* d_fused = nullptr;
  size_t fused_bytes = 0;
  unsigned fused_epoch = 0;
  bool fused_enabled = true, fused_unchecked = false;
  long fused_timeouts = 0;             // one-launch sweeps found incomplete (bodyfit_internal_fused_timeouts)
  unsigned long long role_timeout_ticks = bodyfit::kRoleTimeoutDefault;   // bound of the one-launch sweep's in-launch waits

  // ---- async ordering (order_after_async)
  hipStream_t async_stream = nullptr;  // stream of the last bodyfit_evaluate_device / bodyfit_reduce_shared_device
  bool async_pending = false;          // ... and whether anything was enqueued there since the last synchronous entry point
  hipEvent_t async_event = nullptr;

  // ---- solves
  unsigned char* lm_pool = nullptr;    // device LM state of bodyfit_solve, one allocation kept across solves
  unsigned char* win_pool = nullptr;   // device window LM (k_window_lm.hip): state + cyclic-reduction buffers
  size_t win_pool_bytes = 0;
  hipStream_t lm_stream = nullptr;
  long last_exchanges = 0;             // all-gathers issued by the last sharded solve (tests: exchanges per iteration)
  double exchange_timeout_s = 0.0;     // bodyfit_set_exchange_timeout: bound of one exchange / status read of a sharded solve
  int test_poison_rank = -1, test_poison_iter = -1;   // bodyfit_internal_set_test_poison (tests only)
  int proxy_ranks = 0, proxy_rank = 0;                // bodyfit_set_shard_proxy (measurement aid): 0 = off

  // ---- Ceres cache: host cache of the last batched evaluation (serves bodyfit_evaluate_block)
  std::mutex mu;
  bool cache_valid = false, cache_has_jac = false;
  // (page-locked mirrors: the sweep's parameters go up from them, its residuals / Jacobian / components come back into them)
  bodyfit::Pinned<double> c_params, c_beta, c_r, c_J;
  // packed form of the cached Jacobian (bodyfit_evaluate_batch without a caller's Jacobian buffer): only the column blocks a
  // probe sweep found non-zero cross PCIe, k_pack_jacobian's layout
  bodyfit::Pinned<double> c_Jp;
  std::vector<unsigned> pk_mask, pk_off;   // [K] block masks, [K + 1] offsets (doubles) into the packed buffer
  std::vector<short> pk_src;               // [K][32]: where block b of keypoint k starts inside the keypoint's packed row, -1: absent
                                           // (bodyfit_evaluate_block_cached serves a block with one table look-up instead of a walk
                                           // over the mask)
  unsigned* d_pk_mask = nullptr;
  unsigned* d_pk_off = nullptr;
  double* d_Jp = nullptr;
  bool pk_ready = false, cache_packed = false;
  bodyfit::Pinned<int> c_comp;
  size_t c_npar = 0, c_nbeta = 0;       // valid entries of c_params / c_beta
  hipStream_t copy_stream = nullptr;   // the Ceres-kept path's own stream (H2D, sweep, D2H)

  // ---- forward VJP: buffers allocated on the problem's first VJP (bodyfit_forward_vjp_device): its own mesh operands (so an
  // evaluation's views are left alone), the vertex gradients gb, blended vertices, blend partials, transform gradients
  bool vjp_alloc = false, vjp_mesh_alloc = false;
  bodyfit::MeshCoef vjp_mc{};
  double* vjp_r = nullptr;
  double* vjp_joints = nullptr;
  double* vjp_gbf = nullptr;           // [F][nS] per-frame beta gradients
  float* vjp_gb = nullptr;
  float* vjp_bbuf = nullptr;
  float* vjp_part = nullptr;
  double* vjp_dT = nullptr;

  // ---- forward JVP (k_forward_jvp.hip): buffers allocated on the problem's first JVP with a cloud tangent
  // (bodyfit_forward_jvp_device): its own mesh operands, the primal blended vertices [F][Vp][3], and one 32-tangent tile per
  // frame of transform tangents [F][32][24][12] f32, blend-coefficient fragments [F][14][2][64][8] bf16 and blended-vertex
  // tangents [F][32][Vp][3] f32
  bool jvp_alloc = false;
  bodyfit::MeshCoef jvp_mc{};
  double* jvp_r = nullptr;
  double* jvp_joints = nullptr;
  float* jvp_bbuf = nullptr;
  float* jvp_tdot = nullptr;
  float* jvp_dbuf = nullptr;
  uint16_t* jvp_featD = nullptr;

  // ---- residual VJP (k_residual_vjp.hip): whether d_J / d_comp hold the dense Jacobian of the last sweep (a Jacobian sweep into the
  // problem's own buffers sets it; residual-only sweeps, the solves and every other writer of d_r / d_J clear it), the per-frame
  // beta partials of a shared beta and the GMM prior's transposed factor rows, both allocated on the first residual VJP
  bool jac_current = false;
  double* rvjp_gbf = nullptr;
  double* rvjp_gmm = nullptr;

  bodyfit::Allocs mem;
};

namespace bodyfit {

// A problem's sizes, in one place.  nbeta_all: the shape coefficients the problem holds when its shape block is present (0
// without one); what an entry point does about a NULL beta stays its own rule.
struct ProblemDims {
  int npose;          // parameters of one frame row: 7 + 3 (n_joints - 1)
  bool has_beta;      // n_cols = npose + n_shape
  size_t npar;        // doubles of the parameter rows (the halo row included)
  size_t nbeta_all;
};
inline ProblemDims dims(const bodyfit_problem* p) {
  const int npose = 7 + 3 * (p->m->nJ - 1);
  const bool has_beta = p->lay.n_cols > npose;
  return ProblemDims{npose, has_beta, (size_t)p->n_param_rows * npose,
                     has_beta ? (size_t)(p->desc.beta_per_frame ? p->d.F * p->m->nS : p->m->nS) : 0};
}

// The preconditions of per-vertex offsets, shared by bodyfit_forward_offsets*: a want_mesh problem, SMPL's 24 joints (the
// skinning transforms' stride in k_offsets.hip), and a frame stride of 0 (shared) or at least one dense row.  (A call without
// its cloud argument ignores valid offsets: the joints do not depend on them.)
inline int check_offsets(const bodyfit_problem* p, long long offsets_frame_stride) {
  if (p->m->nJ != kMaxJoints) return fail(BODYFIT_ERR_INVALID, "offsets need a model with 24 joints");
  if (!p->desc.want_mesh) return fail(BODYFIT_ERR_INVALID, "offsets need a problem created with want_mesh");
  if (offsets_frame_stride != 0 && offsets_frame_stride < 3LL * p->m->V)
    return fail(BODYFIT_ERR_INVALID, "offsets_frame_stride is neither 0 (shared) nor >= 3 V");
  return BODYFIT_OK;
}

// What one sweep() evaluates, where, and where its results go.
struct SweepRequest {
  const double* params;           // device
  const double* beta;             // device, nullptr without a shape block
  int want_jac = 0;               // (handed to the kernels as the caller gave it)
  bool mesh = false;
  hipStream_t stream = nullptr;
  hipEvent_t* events = nullptr;   // optional: the dispatches' own begin / end timestamps (sweep())
  // Redirections: a sweep with any of these set does not leave the problem's own r / J / comp describing `params`.  One added
  // later goes HERE and into fills_problem_buffers(): bodyfit_residual_vjp_device(reuse_jacobian = 1) trusts d_J / d_comp on
  // that predicate alone.
  double* r_out = nullptr;
  double* J_out = nullptr;
  int* comp_out = nullptr;
  const int* frame_flags = nullptr;
  int frame_mask = 0;
  const double* R0_override = nullptr;
  bool skip_priors = false;
  bool fills_problem_buffers() const {
    return !r_out && !J_out && !comp_out && !frame_flags && !skip_priors && !R0_override;
  }
};

// api_core.hip
int sweep(bodyfit_problem* p, const SweepRequest& rq);
bool fused_timed_out(bodyfit_problem* p);
int fused_check(bodyfit_problem* p);
int order_after_async(bodyfit_problem* p, hipStream_t own);

// The solves reuse d_r / d_J / d_comp as their working state: whatever they leave there is no Jacobian a caller may reuse
struct DropJacobianOnExit {
  bodyfit_problem* p;
  ~DropJacobianOnExit() { p->jac_current = false; }
};

}  // namespace bodyfit
