// api_core.hip — what every other unit of the C ABI (include/bodyfit.h) goes through: the thread's error string, the launch
// counter, the evaluation sweep and the checks and ordering around it (host_state.h declares them).
#include "host_state.h"

#include <cstdlib>
#include <string>

namespace bodyfit {
std::atomic<long> g_launch_count{0};
}

namespace {

thread_local std::string g_err;

int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return (e && *e) ? std::atoi(e) : dflt;
}

}  // namespace

namespace bodyfit {

// The bounded waits of the one-launch sweep's mesh role set an error word instead of hanging (the tile's part of the cloud is
// then missing; r, J, joints and the folded reduction never depend on a wait).  fused_timed_out reads and clears the word
// (the caller has synchronised the stream the sweep ran on) and switches the problem to the two-launch sweep for the rest of
// its life.  The synchronous entry points re-issue their sweep at once, so their callers never see the event; asynchronous
// callers ask bodyfit_sweep_status.
bool fused_timed_out(bodyfit_problem* p) {
  if (!p->fused_unchecked || !p->d_fused) return false;
  p->fused_unchecked = false;
  unsigned err = 0;
  if (hipMemcpy(&err, p->d_fused, sizeof(err), hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (!err) return false;
  (void)hipMemset(p->d_fused, 0, 4);
  p->fused_enabled = false;
  ++p->fused_timeouts;
  return true;
}
int fused_check(bodyfit_problem* p) {
  if (fused_timed_out(p))
    return fail(BODYFIT_ERR_HIP, "one-launch sweep: an in-launch wait timed out (the cloud of that sweep is incomplete); "
                                 "the problem now uses the two-launch sweep");
  return BODYFIT_OK;
}

// bodyfit_evaluate_batch (and the other entry points that own a stream) may run while asynchronous sweeps of the same problem
// are still in flight on a caller's stream: both write the problem's r / J / partials and the one-launch sweep's counters, so
// they must not overlap.  The asynchronous entry points only note their stream (no event per sweep: that would cost the
// resident path a microsecond per step); the synchronous ones record ONE event behind everything enqueued there so far and
// make their own stream wait for it.
// The caller's stream must stay alive until the problem's next synchronous entry point (or bodyfit_sweep_status on it) has
// returned: the event is recorded on it (include/bodyfit.h, bodyfit_evaluate_device).
int order_after_async(bodyfit_problem* p, hipStream_t own) {
  if (!p->async_pending) return BODYFIT_OK;
  if (p->async_stream != own) {                    // (same stream: ordered anyway)
    if (!p->async_event) HIP_TRY(hipEventCreateWithFlags(&p->async_event, hipEventDisableTiming));
    const hipError_t er = hipEventRecord(p->async_event, p->async_stream);
    if (er == hipErrorInvalidHandle || er == hipErrorInvalidResourceHandle || er == hipErrorContextIsDestroyed) {
      // the caller has destroyed that stream: a stream can only be destroyed once its work is done (hipStreamDestroy waits), so
      // there is nothing left to order behind
      (void)hipGetLastError();
    } else {
      HIP_TRY(er);
      HIP_TRY(hipStreamWaitEvent(own, p->async_event, 0));
    }
  }
  p->async_pending = false;                        // only once the ordering is in place
  return BODYFIT_OK;
}

// One evaluation sweep on the caller's stream: ONE launch (k_sweep_roles: frame, mesh and prior workgroups side by side)
// when the mesh is on, otherwise (no mesh, device LM with frame flags, models with more than 12 landmark slots) two.  The prior residuals are produced by extra
// workgroups (priors_inl.h) of the mesh launch when the mesh is on (its vertex tiles leave 40 CUs idle), otherwise
// of the k_frame_resjac launch.  rq.events (optional, 4 events): the dispatches' own begin / end timestamps,
// [0],[1] k_frame_resjac, [2],[3] k_mesh_blend_lbs.
int sweep(bodyfit_problem* p, const SweepRequest& rq) {
  const bodyfit_model* m = p->m;
  DevProblem dp = p->d;
  p->jac_current = false;
  if (rq.R0_override) dp.R0 = rq.R0_override;
  dp.beta_partials = (rq.want_jac && !rq.frame_flags) ? p->d_frame_partials : nullptr;
  dp.huber = p->desc.huber_delta;
  p->partials_fresh = dp.beta_partials != nullptr;
  p->fold_fresh = false;
  dp.frame_flags = rq.frame_flags;
  dp.frame_mask = rq.frame_mask;
  double* d_r = rq.r_out ? rq.r_out : p->d_r;
  double* d_J = rq.J_out ? rq.J_out : p->d_J;
  int* d_comp = rq.comp_out ? rq.comp_out : p->d_comp;
  MeshCoef mc = p->mc;
  if (!rq.mesh) mc = MeshCoef{};
  const bodyfit_problem_desc& D = p->desc;
  PriorArgs pa{};
  pa.F = p->d.F; pa.nS = m->nS; pa.beta_stride = p->d.beta_stride; pa.npose = 7 + 3 * (m->nJ - 1);
  pa.has_gmm = p->has_gmm ? 1 : 0;
  if (p->has_gmm) pa.g = p->gmm;
  pa.beta_pose = D.beta_pose;
  pa.beta_shape = p->lay.shape_rows > 0 ? D.beta_shape : 0.0;
  pa.lambda_t = D.lambda_temporal;
  pa.n_pairs = p->n_pairs;
  pa.beta = rq.beta;
  pa.r_prior = d_r + p->row_prior; pa.r_shape = d_r + p->row_shape; pa.r_temporal = d_r + p->row_temporal;
  pa.comp = d_comp;
  const bool priors = D.beta_pose > 0.0 || pa.beta_shape > 0.0 || D.lambda_temporal > 0.0;
  pa.n_tiles = (priors && !rq.skip_priors) ? (p->d.F + 15) / 16 : 0;
  pa.plain_cost = dp.beta_partials ? dp.beta_partials + (size_t)p->d.F * kReducePartial : nullptr;
  p->partials_tiles = dp.beta_partials ? pa.n_tiles : 0;
  PriorArgs none = pa;
  none.n_tiles = 0;
  if (rq.mesh && !rq.frame_flags && p->fused_enabled && p->d_fused && role_sweep_fits(m->d, dp)) {
    // ONE launch: frame, mesh and prior roles, operands handed over inside the launch (k_sweep.hip)
    FusedSync sy{};
    sy.error = reinterpret_cast<unsigned*>(p->d_fused);
    sy.flag = reinterpret_cast<unsigned*>(p->d_fused + kFusedSyncHeader);
    if (p->fused_epoch >= (1u << 26) || p->fold_count >= (1u << 31)) {
      // epoch x 32 is about to wrap the 32-bit unit counters (or the fold ticket): start over (stream-ordered)
      (void)hipMemsetAsync(p->d_fused, 0, p->fused_bytes, rq.stream);
      p->fused_epoch = 0;
      p->fold_count = 0;
    }
    sy.epoch = ++p->fused_epoch;
    sy.resident_blocks = 2 * m->n_cus;
    sy.timeout_ticks = p->role_timeout_ticks;
#ifdef BODYFIT_TUNE_ENV   // diagnostic builds only (tools/probes/sweep_tune.py): the shipped library reads no tuning word from outside
    static const int tune_prio = env_int("BODYFIT_MESH_PRIO", kTuneMeshPrio), tune_start = env_int("BODYFIT_TRICKLE_START", kTuneTrickleStart),
                     tune_sleep = env_int("BODYFIT_TRICKLE_SLEEP", kTuneTrickleSleep), tune_jscope = env_int("BODYFIT_J_SCOPE", kTuneJScope);
#else
    constexpr int tune_prio = kTuneMeshPrio, tune_start = kTuneTrickleStart, tune_sleep = kTuneTrickleSleep, tune_jscope = kTuneJScope;
#endif
    sy.mesh_prio_early = tune_prio; sy.trickle_start = tune_start; sy.trickle_sleep = tune_sleep; sy.j_scope = tune_jscope;
    p->fused_unchecked = true;
    FoldTail fold{};
    const int n_partials = p->d.F + pa.n_tiles;
    if (p->armed_out66 && dp.beta_partials && !p->desc.beta_per_frame && rq.beta && n_partials <= kFoldMaxPartials) {
      // the shared-shape reduction rides on this launch's tail (bodyfit_arm_shared_reduction)
      fold.ticket = reinterpret_cast<unsigned*>(p->d_fused + kFoldTicketOffset);
      fold.want = (p->fold_count += (unsigned)n_partials);
      fold.n_partials = n_partials;
      fold.partials = dp.beta_partials;
      fold.beta = rq.beta;
      fold.shape_rows = p->lay.shape_rows;
      fold.beta_shape = D.beta_shape;
      fold.out66 = p->armed_out66;
      p->fold_fresh = true;
    }
    launch_sweep_roles(m->d, dp, rq.params, rq.beta, d_r, rq.want_jac ? d_J : nullptr, p->d_joints, mc, rq.want_jac, pa,
                       p->d_cloud, sy, fold, rq.stream, rq.events ? rq.events[4] : nullptr, rq.events ? rq.events[5] : nullptr);
  } else {
    launch_frame_resjac(m->d, dp, rq.params, rq.beta, d_r, rq.want_jac ? d_J : nullptr, p->d_joints, mc, rq.want_jac,
                        rq.mesh ? none : pa, rq.stream, rq.events ? rq.events[0] : nullptr, rq.events ? rq.events[1] : nullptr);
    if (rq.mesh) launch_mesh(m->d, p->d, p->mc, p->d_cloud, pa, rq.params, rq.stream, rq.events ? rq.events[2] : nullptr, rq.events ? rq.events[3] : nullptr);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BODYFIT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  // the dense Jacobian of every frame and the components of this point are now in the problem's own buffers
  p->jac_current = rq.want_jac && rq.fills_problem_buffers();
  return BODYFIT_OK;
}

}  // namespace bodyfit

extern "C" {

const char* bodyfit_last_error(void) { return g_err.c_str(); }

int bodyfit_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

long bodyfit_launch_count(void) { return bodyfit::g_launch_count.load(std::memory_order_relaxed); }

int bodyfit_internal_fail(int code, const char* msg) {
  g_err = msg ? msg : "";
  return code;
}

void bodyfit_internal_drop_jacobian(bodyfit_problem* p) {
  if (p) p->jac_current = false;
}

}  // extern "C"
