// api_solve.hip — the device-resident solves behind bodyfit_solve (host_solver.cpp routes to them) and bodyfit_solve_sharded*:
// the batched LM over independent frames, the window LM with its cyclic-reduction schedule, the host and RCCL transports.
#include "host_state.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "collectives.h"

using namespace bodyfit;

extern "C" {

// Device-resident LM over independent frames (k_lm_batched.hip).  Called by bodyfit_solve.
int bodyfit_internal_solve_batched_device(bodyfit_problem* p, double* frame_params, double* beta,
                                          const unsigned char* param_constant, const bodyfit_fit_options* opt,
                                          bodyfit_fit_summary* summaries, int n_summaries) {
  const bodyfit_model* m = p->m;
  const int F = p->d.F, npose = dims(p).npose, n = p->lay.n_cols, nb = n - npose;
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  DropJacobianOnExit drop_jacobian{p};
  LmState S{};
  LmProblem P{};
  P.F = F; P.ncols = n; P.kp_offset = p->d.kp_offset;
  P.huber = p->desc.huber_delta; P.beta_pose = p->desc.beta_pose; P.beta_shape = p->desc.beta_shape;
  P.scale_lo = opt->scale_lo; P.scale_hi = opt->scale_hi;
  P.prior_rows = p->lay.prior_rows_per_frame; P.row_prior = p->row_prior;
  P.shape_rows_per_frame = (p->lay.shape_rows > 0) ? m->nS : 0; P.row_shape = p->row_shape;
  P.prec = p->has_gmm ? p->gmm.prec : nullptr; P.prec_cho = p->has_gmm ? p->gmm.prec_cho : nullptr;
  P.gmm_mean = p->has_gmm ? p->gmm.mean : nullptr; P.gmm_scale = p->has_gmm ? p->gmm.resid_scale : 0.0;
  double* d_r_new = nullptr;
  double* d_J_new = nullptr;
  int* d_comp_new = nullptr;
  unsigned char* d_const = nullptr;
  {
    // one pooled allocation (sizes depend on the problem only), made on the first solve and reused: seventeen
    // hipMalloc / hipFree pairs per solve were a quarter of a single-frame fit
    const size_t nbb = (size_t)std::max(nb, 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_x = take((size_t)F * npose * 8), o_b = take((size_t)F * nbb * 8), o_xn = take((size_t)F * npose * 8),
                 o_bn = take((size_t)F * nbb * 8), o_rad = take((size_t)F * 8), o_dec = take((size_t)F * 8),
                 o_cost = take((size_t)F * 8), o_ic = take((size_t)F * 8), o_model = take((size_t)F * 8),
                 o_scale = take((size_t)F * 86 * 8), o_flags = take((size_t)F * 4), o_iters = take((size_t)F * 4),
                 o_ok = take((size_t)F * 4), o_bad = take((size_t)F * 4), o_act = take(4),
                 o_rn = take((size_t)std::max(1, p->lay.total_rows) * 8), o_cn = take((size_t)F * 4), o_const = take((size_t)npose),
                 o_Jn = take((size_t)std::max(1, p->lay.reproj_rows) * p->lay.n_cols * 8);
    if (!p->lm_pool) HIP_TRY(p->mem.alloc(&p->lm_pool, off));
    unsigned char* B = p->lm_pool;
    S.x = reinterpret_cast<double*>(B + o_x); S.beta = reinterpret_cast<double*>(B + o_b);
    S.x_new = reinterpret_cast<double*>(B + o_xn); S.beta_new = reinterpret_cast<double*>(B + o_bn);
    S.radius = reinterpret_cast<double*>(B + o_rad); S.dec = reinterpret_cast<double*>(B + o_dec);
    S.cost = reinterpret_cast<double*>(B + o_cost); S.initial_cost = reinterpret_cast<double*>(B + o_ic);
    S.model = reinterpret_cast<double*>(B + o_model); S.scale = reinterpret_cast<double*>(B + o_scale);
    S.flags = reinterpret_cast<int*>(B + o_flags); S.iters = reinterpret_cast<int*>(B + o_iters);
    S.n_ok = reinterpret_cast<int*>(B + o_ok); S.n_bad = reinterpret_cast<int*>(B + o_bad);
    S.active_count = reinterpret_cast<int*>(B + o_act);
    d_r_new = reinterpret_cast<double*>(B + o_rn); d_comp_new = reinterpret_cast<int*>(B + o_cn);
    d_J_new = reinterpret_cast<double*>(B + o_Jn);
    if (param_constant) d_const = B + o_const;
  }
  if (!p->lm_stream) HIP_TRY(hipStreamCreateWithFlags(&p->lm_stream, hipStreamNonBlocking));
  hipStream_t st = p->lm_stream;
  if (int ro = order_after_async(p, st)) return ro;   // (the solve writes the r / J / partials an asynchronous sweep may still be writing)
  HIP_TRY(hipMemsetAsync(S.active_count, 0, sizeof(int), st));
  HIP_TRY(hipMemcpyAsync(S.x, frame_params, (size_t)F * npose * sizeof(double), hipMemcpyHostToDevice, st));
  if (nb) HIP_TRY(hipMemcpyAsync(S.beta, beta, (size_t)F * nb * sizeof(double), hipMemcpyHostToDevice, st));
  if (param_constant) HIP_TRY(hipMemcpyAsync(d_const, param_constant, (size_t)npose, hipMemcpyHostToDevice, st));
  const double* bptr = nb ? S.beta : nullptr;
  SweepRequest at_x{S.x, bptr};
  at_x.want_jac = 1; at_x.stream = st;
  int rc = sweep(p, at_x);
  if (rc) return rc;
  launch_lm_init(P, S, p->d_r, st);
  int n_sweeps = 1;
  // Speculative iteration (default): the sweep at the candidate also produces its Jacobian (into second buffers), and the
  // next k_lm_step judges the candidate before it builds its system from whichever point won: two launches per iteration
  // (step, sweep) instead of four (step, residual sweep, accept, Jacobian sweep).  A rejected candidate's Jacobian is
  // wasted work that costs no time (the sweep is latency-bound).  BODYFIT_LM_PLAIN=1 keeps the four-launch form.
  const bool plain = [] { const char* e = std::getenv("BODYFIT_LM_PLAIN"); return e && e[0] == '1'; }();
  auto iteration = [&](int first) -> int {
    if (!plain) {
      launch_lm_step(P, S, p->d_r, p->d_J, p->d_comp, d_r_new, d_J_new, d_comp_new, d_const, first, st);
      SweepRequest cand{S.x_new, nb ? S.beta_new : nullptr};
      cand.want_jac = 1; cand.stream = st;
      cand.r_out = d_r_new; cand.J_out = d_J_new; cand.comp_out = d_comp_new;
      cand.frame_flags = S.flags; cand.frame_mask = kLmHasCand;
      return sweep(p, cand);
    }
    launch_lm_step(P, S, p->d_r, p->d_J, p->d_comp, nullptr, nullptr, nullptr, d_const, first, st);
    // candidate residuals only for frames that have a candidate; fresh Jacobians only for frames still active
    SweepRequest cand{S.x_new, nb ? S.beta_new : nullptr};
    cand.stream = st;
    cand.r_out = d_r_new; cand.comp_out = d_comp_new;
    cand.frame_flags = S.flags; cand.frame_mask = kLmHasCand;
    int rc2 = sweep(p, cand);
    if (rc2) return rc2;
    launch_lm_accept(P, S, d_r_new, p->d_r, d_comp_new, p->d_comp, st);
    // (prior rows of accepted frames were carried over by k_lm_accept: no prior workgroups on this sweep)
    SweepRequest active{S.x, bptr};
    active.want_jac = 1; active.stream = st;
    active.frame_flags = S.flags; active.frame_mask = kLmActive;
    active.skip_priors = true;
    return sweep(p, active);
  };
  // (a hipGraph replay of this ~20-launch iteration was measured slower than eager launches on ROCm 7.2:
  //  256 frames to convergence 25.6 ms vs 23.0 ms; so the loop stays eager)
  for (int it = 0; it < opt->max_iters; ++it) {
    rc = iteration(it == 0 ? 1 : 0);
    if (rc) return rc;
    n_sweeps += plain ? 2 : 1;
    if ((it & 7) == 7 || it + 1 == opt->max_iters) {   // poll the number of frames still iterating (speculative form:
      int active = 0;                                  // as of the previous iteration's candidates)
      HIP_TRY(hipMemcpyAsync(&active, S.active_count, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (active <= 0) break;
    }
  }
  // the last candidates are still unjudged in the speculative form (no further step: only x, cost and the counters matter)
  if (!plain) launch_lm_accept(P, S, d_r_new, p->d_r, d_comp_new, p->d_comp, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(frame_params, S.x, (size_t)F * npose * sizeof(double), hipMemcpyDeviceToHost));
  if (nb) HIP_TRY(hipMemcpy(beta, S.beta, (size_t)F * nb * sizeof(double), hipMemcpyDeviceToHost));
  if (summaries && n_summaries > 0) {
    std::vector<int> fl(F), itv(F), ok(F), bad(F);
    std::vector<double> c0(F), c1(F);
    HIP_TRY(hipMemcpy(fl.data(), S.flags, F * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(itv.data(), S.iters, F * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ok.data(), S.n_ok, F * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bad.data(), S.n_bad, F * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c0.data(), S.initial_cost, F * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c1.data(), S.cost, F * sizeof(double), hipMemcpyDeviceToHost));
    for (int f = 0; f < F && f < n_summaries; ++f) {
      bodyfit_fit_summary& s2 = summaries[f];
      s2.iterations = itv[f];
      s2.termination = (fl[f] & kLmActive) ? 1 : ((fl[f] & kLmTermMask) >> kLmTermShift);
      s2.usable = s2.termination != 2;
      s2.n_successful = ok[f]; s2.n_unsuccessful = bad[f];
      s2.n_sweeps = n_sweeps; s2.n_sweeps_issued = n_sweeps;
      s2.initial_cost = c0[f]; s2.final_cost = c1[f];
    }
  }
  return BODYFIT_OK;
}

// Cyclic-reduction schedule over `n` chain nodes (ids base .. base + n - 1): per level the eliminated nodes (j, left, right)
// and the remaining ones that receive an update (a, jl, jr, next).  pinned: the two end nodes are never eliminated (a shard's
// interface with its neighbours); otherwise the last level is the root (j, -1, -1).
struct CrLevel { int elim_off, n_elim, surv_off, n_surv; };
static void build_cr_schedule(int n, bool pinned, std::vector<int>& sched, std::vector<CrLevel>& levels) {
  std::vector<int> active(n);
  for (int f = 0; f < n; ++f) active[f] = f;
  for (;;) {
    const int na = (int)active.size();
    std::vector<char> el(na, 0);
    int ne = 0;
    // every other node goes; with an odd number of free-ended nodes the EVEN positions (one more of them) go, so that
    // 20 frames take 20 -> 10 -> 5 -> 2 -> 1 -> root, one level less than always eliminating the odd positions
    const int first = (!pinned && (na & 1) && na > 1) ? 0 : 1;
    for (int pos = first; pos < na; pos += 2)
      if (!(pinned && pos == na - 1)) { el[pos] = 1; ++ne; }
    if (ne == 0) break;
    CrLevel lv{};
    lv.elim_off = (int)sched.size();
    for (int pos = 0; pos < na; ++pos)
      if (el[pos]) {
        sched.push_back(active[pos]); sched.push_back(pos > 0 ? active[pos - 1] : -1); sched.push_back(pos + 1 < na ? active[pos + 1] : -1);
        ++lv.n_elim;
      }
    lv.surv_off = (int)sched.size();
    std::vector<int> next;
    for (int pos = 0; pos < na; ++pos) {
      if (el[pos]) continue;
      next.push_back(active[pos]);
      const int jl = (pos > 0 && el[pos - 1]) ? active[pos - 1] : -1;
      const int jr = (pos + 1 < na && el[pos + 1]) ? active[pos + 1] : -1;
      if (jl < 0 && jr < 0) continue;
      sched.push_back(active[pos]); sched.push_back(jl); sched.push_back(jr);
      sched.push_back((jr >= 0 && pos + 2 < na) ? active[pos + 2] : -1);
      ++lv.n_surv;
    }
    levels.push_back(lv);
    active.swap(next);
  }
  if (!pinned) {
    CrLevel root{};
    root.elim_off = (int)sched.size(); root.n_elim = 1;
    sched.push_back(active[0]); sched.push_back(-1); sched.push_back(-1);
    levels.push_back(root);
  }
}

// carve the cyclic-reduction buffers of `n` nodes out of a pool
static size_t carve_cr(unsigned char* base, size_t off, int n, WinBuf& W, bool dry) {
  const size_t blk = (size_t)kWinBlock * kWinBlock * 8, rhs = (size_t)kWinRhs * kWinBlock * 8;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_D = take(n * blk), o_U = take(n * blk), o_L = take(n * blk), o_P = take(n * blk), o_Q = take(n * blk),
               o_R = take(n * rhs), o_R0 = take(n * rhs), o_Y = take(n * rhs), o_X = take(n * rhs),
               o_Li = take((size_t)n * (kWinBlock / 16) * 256 * 8), o_fail = take(8), o_ticket = take(4 * (size_t)(2 + n / 32 + 1));
  if (!dry) {
    auto dp = [&](size_t o) { return reinterpret_cast<double*>(base + o); };
    W.D = dp(o_D); W.U = dp(o_U); W.L = dp(o_L); W.Pt = dp(o_P); W.Qt = dp(o_Q); W.Rt = dp(o_R); W.Rt0 = dp(o_R0);
    W.Yt = dp(o_Y); W.Xt = dp(o_X); W.Li = dp(o_Li); W.fail = reinterpret_cast<int*>(base + o_fail);
    W.ticket = reinterpret_cast<int*>(base + o_ticket);
  }
  return off;
}

// Device-resident LM for ONE problem over all frames with a shared beta (k_window_lm.hip): the outer loop of
// OptimizeMultiFrame (include/MultiFrameBA.h:144-151) with every piece of linear algebra on the device.  Per LM iteration
// the host launches: [Jacobian sweep + k_frame_normal when the point moved] -> assemble -> cyclic reduction up and down ->
// beta Schur + step + model change -> residual sweep at the candidate -> accept, and reads back one status record.
//
// comm != NULL: this problem is ONE SHARD (contiguous frames) of the window, one process per GPU (bodyfit_solve_sharded).
// Every rank reduces its own chain down to its two end frames (cyclic reduction with the ends pinned), the 2 N interface
// blocks are all-gathered and solved redundantly by every rank, then each rank substitutes back through its own levels.
// What crosses ranks per LM iteration, as THREE all-gathers of device buffers ordered on the solve's stream (RCCL: nothing
// touches the host, no stream synchronisation between the host's status reads):
//   1. the interface blocks of the shard's two end frames (225 KB) with the shard's beta terms [C, g_beta] (110 doubles)
//      riding on the same buffer;
//   2. the shard's beta Schur partials (110 doubles) — they need the interface solution, the step needs them;
//   3. the shard's scalars [model change, |d|^2, |x|^2, max |g|, failure flag, cost at the candidate] (8 doubles): ONE
//      decision kernel then applies Ceres' tests and the accept / reject rules on every rank, on the same numbers.
// Sums are taken by every rank in rank order from the gathered partials (bit-identical totals, identical decisions, no
// broadcast).  The steps of the neighbouring shards' boundary frames — the halo row of the temporal pair this shard owns, the
// frame in front of its first — are not exchanged at all: every rank holds the whole interface solution and computes them
// with the neighbour's own arithmetic (k_win_halo_step).  The first iteration has two more small gathers (the beta terms
// before the first scaling, the boundary frames' Jacobi scaling), the start one (the boundary rows).
static int solve_window_device(bodyfit_problem* p, double* frame_params, double* beta,
                               const unsigned char* param_constant, const bodyfit_fit_options* opt,
                               bodyfit_fit_summary* summary, Transport* comm, bool force_sharded) {
  const bodyfit_model* m = p->m;
  const int F = p->d.F, npose = dims(p).npose, n = p->lay.n_cols, nb = n - npose;
  DropJacobianOnExit drop_jacobian{p};
  // shard proxy (bodyfit_set_shard_proxy): through a ONE-rank communicator this problem runs as rank proxy_rank of proxy_ranks
  // identical shards — every kernel, buffer and exchange of that geometry, the gathered slots filled with copies of its own
  const bool proxy = comm != nullptr && comm->size == 1 && p->proxy_ranks > 1;
  const bool sharded = comm != nullptr && (comm->size > 1 || force_sharded || proxy);
  const int halo = p->desc.temporal_halo ? 1 : 0;
  if (npose != kFrameParams || nb != kMaxShape || p->desc.beta_per_frame || p->has_gmm)
    return fail(BODYFIT_ERR_INVALID, "device window solver: needs 24 joints, a shared 10-coefficient beta and the L2 pose prior");
  if (halo && !sharded) return fail(BODYFIT_ERR_INVALID, "device window solver: a halo row needs bodyfit_solve_sharded");
  if (sharded && F < 2) return fail(BODYFIT_ERR_INVALID, "bodyfit_solve_sharded: every shard needs at least two frames");
  const int R = proxy ? p->proxy_rank : (sharded ? comm->rank : 0), N = proxy ? p->proxy_ranks : (sharded ? comm->size : 1);
  const bool has_left = sharded && R > 0;
  if (sharded && (halo != 0) != (R + 1 < N))
    return fail(BODYFIT_ERR_INVALID, "bodyfit_solve_sharded: every shard but the last needs temporal_halo");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> lock(p->mu);
  p->cache_valid = false;
  // ---- schedules ----
  std::vector<int> sched;
  std::vector<CrLevel> levels, ilevels;
  build_cr_schedule(F, sharded, sched, levels);
  const int NI = 2 * N;   // interface nodes
  if (sharded) build_cr_schedule(NI, false, sched, ilevels);
  // ---- one pooled allocation, kept across solves ----
  WinBuf W{}, Wi{};
  double *d_x, *d_b, *d_xn, *d_bn, *d_rn, *d_xl, *d_sh, *d_dh, *d_xln, *d_sl, *d_cg, *d_send, *d_gath, *d_Jn;
  int *d_compn, *d_sched;
  unsigned char* d_const = nullptr;
  {
    size_t off = carve_cr(nullptr, 0, F, W, true);
    if (sharded) off = carve_cr(nullptr, off, NI, Wi, true);
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_A = take((size_t)F * npose * npose * 8), o_B = take((size_t)F * npose * nb * 8),
                 o_g = take((size_t)F * npose * 8), o_E = take((size_t)F * npose * 8), o_sc = take(((size_t)F * npose + nb) * 8),
                 o_Cs = take(100 * 8), o_rb = take(16 * 8), o_Cr = take(112 * 8), o_dsb = take(16 * 8),
                 o_sred = take(112 * 8), o_fin = take(8 * 8),
                 o_part = take((size_t)F * kWinPart * 8), o_gm = take((size_t)(F + 1) * 8), o_d = take(((size_t)F * npose + nb) * 8),
                 o_st = take(kWsCount * 8), o_x = take((size_t)(F + 1) * npose * 8), o_b = take(nb * 8),
                 o_xn = take((size_t)(F + 1) * npose * 8), o_bn = take(nb * 8), o_rn = take((size_t)std::max(1, p->lay.total_rows) * 8),
                 o_cn = take((size_t)F * 4), o_sched = take(sched.size() * 4), o_const = take((size_t)npose),
                 o_xl = take(npose * 8), o_sh = take(npose * 8), o_dh = take(npose * 8), o_xln = take(npose * 8), o_sl = take(npose * 8),
                 o_Jn = take((size_t)std::max(1, p->lay.reproj_rows) * p->lay.n_cols * 8),
                 o_cg = take(112 * 8), o_send = take(sharded ? (size_t)iface_doubles(112) * 8 : 8),
                 o_gath = take(sharded ? (size_t)N * iface_doubles(112) * 8 : 8);
    if (!p->win_pool || p->win_pool_bytes < off) {
      HIP_TRY(p->mem.alloc(&p->win_pool, off));
      HIP_TRY(hipMemset(p->win_pool, 0, off));
      HIP_TRY(hipStreamSynchronize(nullptr));   // (the clear is on the NULL stream, the solve on a non-blocking one: as in bodyfit_problem_create)
      p->win_pool_bytes = off;
    }
    unsigned char* Bp = p->win_pool;
    size_t o2 = carve_cr(Bp, 0, F, W, false);
    if (sharded) carve_cr(Bp, o2, NI, Wi, false);
    auto dp = [&](size_t o) { return reinterpret_cast<double*>(Bp + o); };
    W.Araw = dp(o_A); W.Braw = dp(o_B); W.graw = dp(o_g); W.Eraw = dp(o_E);
    W.scale = dp(o_sc); W.Cs = dp(o_Cs); W.rhsb = dp(o_rb); W.Craw = dp(o_Cr); W.gbraw = dp(o_Cr) + 100; W.dsb = dp(o_dsb);
    W.sred = dp(o_sred); W.fin = dp(o_fin);
    W.part = dp(o_part); W.gmaxp = dp(o_gm); W.d = dp(o_d); W.status = dp(o_st);
    d_x = dp(o_x); d_b = dp(o_b); d_xn = dp(o_xn); d_bn = dp(o_bn); d_rn = dp(o_rn);
    d_compn = reinterpret_cast<int*>(Bp + o_cn);
    d_sched = reinterpret_cast<int*>(Bp + o_sched);
    if (param_constant) d_const = Bp + o_const;
    d_xl = dp(o_xl); d_sh = dp(o_sh); d_dh = dp(o_dh); d_xln = dp(o_xln); d_sl = dp(o_sl);
    d_cg = dp(o_cg); d_send = dp(o_send); d_gath = dp(o_gath);
    d_Jn = dp(o_Jn);
  }
  if (!p->d_frame_normal) HIP_TRY(p->mem.alloc(&p->d_frame_normal, (size_t)F * kNormalRows * kNormalLd));
  if (!p->lm_stream) HIP_TRY(hipStreamCreateWithFlags(&p->lm_stream, hipStreamNonBlocking));
  hipStream_t st = p->lm_stream;
  if (int ro = order_after_async(p, st)) return ro;
  WinProblem P{};
  P.F = F; P.K = p->lay.n_keypoints; P.total_rows = p->lay.total_rows; P.nb = nb; P.halo = halo;
  P.prior_rows = p->lay.prior_rows_per_frame; P.row_prior = p->row_prior;
  P.shape_rows = p->lay.shape_rows; P.row_shape = p->row_shape; P.row_temporal = p->row_temporal;
  P.huber = p->desc.huber_delta; P.beta_pose = p->desc.beta_pose; P.beta_shape = p->desc.beta_shape;
  P.lambda_t = p->desc.lambda_temporal; P.scale_lo = opt->scale_lo; P.scale_hi = opt->scale_hi;
  {
    // every sweep of this loop is a Jacobian sweep without frame flags: with a shared shape block (the partials exist) it leaves
    // the point's cost as F + tiles partial sums (sweep(): dp.beta_partials, pa.plain_cost)
    const bool priors = p->desc.beta_pose > 0.0 || (p->lay.shape_rows > 0 && p->desc.beta_shape > 0.0) || p->desc.lambda_temporal > 0.0;
    P.cost_partials = (p->d_frame_partials && n > npose && m->nS == kMaxShape) ? p->d_frame_partials : nullptr;
    P.cost_tiles = priors ? (F + 15) / 16 : 0;
  }
  const int rows_x = F + halo;
  HIP_TRY(hipMemcpyAsync(d_x, frame_params, (size_t)rows_x * npose * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_b, beta, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_sched, sched.data(), sched.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (param_constant) HIP_TRY(hipMemcpyAsync(d_const, param_constant, (size_t)npose, hipMemcpyHostToDevice, st));
  // ---- exchanges of a sharded solve: all-gathers of device buffers on the solve's stream (collectives.h) ----
  auto comm_fail = [&](const char* what) {
    return fail(BODYFIT_ERR_INVALID, std::string("bodyfit_solve_sharded: ") + what + " failed: " + (comm ? comm->error : ""));
  };
  // gather n doubles per rank from d_send into d_gath [N][n]
  auto gather = [&](const double* d_send, int cnt, const char* what) -> int {
    if (comm->allgather(d_send, d_gath, cnt, st)) return comm_fail(what);
    if (proxy) launch_replicate_ranks(d_gath, cnt, N, st);
    return BODYFIT_OK;
  };
  // the host's wait for a status record: bounded for sharded solves with bodyfit_set_exchange_timeout (a peer that left after a
  // transport failure never enters the collectives queued on the stream)
  auto wait_status = [&](hipStream_t s2) -> int {
    hipError_t he = hipSuccess;
    const int w = wait_stream(s2, sharded ? p->exchange_timeout_s : 0.0, &he);
    if (w == 1) return fail(BODYFIT_ERR_HIP, "bodyfit_solve_sharded: the solve's stream did not drain within the exchange timeout "
                                             "(a peer has left the collective); the problem's stream is unusable from here on");
    if (w < 0) return fail(BODYFIT_ERR_HIP, std::string("status read: ") + hipGetErrorString(he));
    return BODYFIT_OK;
  };
  if (sharded) {
    // the boundary rows of the starting point: [first row | last row] of every shard -> the frame in front of this shard's
    // first (d_xl) and the halo row behind its last
    HIP_TRY(hipMemcpyAsync(d_send, d_x, npose * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_send + npose, d_x + (size_t)(F - 1) * npose, npose * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (int rcg = gather(d_send, 2 * npose, "allgather (boundary rows)")) return rcg;
    if (has_left)
      HIP_TRY(hipMemcpyAsync(d_xl, d_gath + ((size_t)(R - 1) * 2 + 1) * npose, npose * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (halo)
      HIP_TRY(hipMemcpyAsync(d_x + (size_t)F * npose, d_gath + (size_t)(R + 1) * 2 * npose, npose * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  // The loop never sweeps twice at the same point.  The sweep at a candidate also leaves the candidate's Jacobian (second
  // buffers); the next iteration's k_frame_normal takes the starting point's (r, J), the accepted candidate's, or nothing at
  // all (rejected step: the panels are current), as the device's own record says (W.status[kWsJsel]; sharded solves: every
  // rank's k_win_decide writes the same).
  // Sharded solves: a rank whose own work fails (a kernel launch, a HIP call) must not simply return — its peers would wait for
  // it in the next all-gather for ever.  It marks slot 6 of its scalars (`poison`), keeps taking part in the exchanges of the
  // iteration, and k_win_decide ends the solve on EVERY rank in that same iteration (kWsPoison).  Only a failure of the
  // transport itself returns at once (bodyfit_set_exchange_timeout bounds how long the peers then wait).
  int poison = BODYFIT_OK;
  std::string poison_msg;
  SweepRequest at_x{d_x, d_b};
  at_x.want_jac = 1; at_x.stream = st;
  int rc = sweep(p, at_x);
  if (rc && sharded) { poison = rc; poison_msg = bodyfit_last_error(); rc = BODYFIT_OK; }   // (between two exchanges: stay in step)
  if (rc) return rc;
  if (!sharded) {
    launch_win_init(P, W, p->d_r, 0, st);
  } else {
    launch_win_init(P, W, p->d_r, 1, st);
    if ((rc = gather(W.fin, 1, "allgather (initial cost)"))) return rc;
    launch_sum_ranks(d_gath, N, 1, 1, W.fin, st);
    launch_win_init(P, W, p->d_r, 2, st);
  }
  int n_sweeps = 1;
  double status[kWsCount] = {0};
  bool first = true;
  const size_t rhs = (size_t)kWinRhs * kWinBlock;
  if (sharded) HIP_TRY(hipMemsetAsync(W.fin, 0, 8 * sizeof(double), st));
  // test hook (tests/test_gpu_sharded_solve.py, bodyfit_internal_set_test_poison): that rank's sweep "fails" in that iteration
  const int test_poison_rank = p->test_poison_rank, test_poison_iter = p->test_poison_iter;
  // a HIP call inside the loop: unsharded, its failure returns; sharded, it poisons (this rank stays in the exchanges)
  auto guard = [&](hipError_t e, const char* what) -> int {
    if (e == hipSuccess) return BODYFIT_OK;
    const int rcg = fail(BODYFIT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    if (!sharded) return rcg;
    if (!poison) { poison = rcg; poison_msg = bodyfit_last_error(); }
    return BODYFIT_OK;
  };
  // the sweep at a candidate: residuals, Jacobian and components into the second buffers
  SweepRequest cand{d_xn, d_bn};
  cand.want_jac = 1; cand.stream = st;
  cand.r_out = d_rn; cand.J_out = d_Jn; cand.comp_out = d_compn;
  for (int it = 0; it < opt->max_iters; ++it) {
    launch_frame_normal_sel(F, n, p->d.kp_offset, p->desc.huber_delta, p->d_r, p->d_J, d_rn, d_Jn, W.status + kWsJsel,
                            p->lay.total_rows, p->d_frame_normal, st);
    // ---- beta block and per-frame blocks ----
    if (!sharded) {
      launch_win_beta(P, W, p->d_frame_normal, p->d_r, first ? 1 : 0, 0, st);
      launch_win_assemble(P, W, p->d_frame_normal, p->d_r, d_x, d_const, first ? 1 : 0, nullptr, nullptr, st);
    } else {
      launch_win_beta(P, W, p->d_frame_normal, p->d_r, first ? 1 : 0, 1, st);   // this shard's [C (100) | g_beta (10)] -> W.Craw
      if (first) {
        // first iteration only: the Jacobi scaling needs the complete C before the blocks are assembled, and the boundary
        // frames' scaling rows (this shard's first and last frame) complete the couplings across the shard boundaries
        if ((rc = gather(W.Craw, 112, "allgather (beta terms)"))) return rc;
        launch_sum_ranks(d_gath, N, 112, 110, W.Craw, st);
        launch_win_beta(P, W, p->d_frame_normal, p->d_r, 1, 2, st);
        launch_win_assemble(P, W, p->d_frame_normal, p->d_r, d_x, d_const, 1, has_left ? d_xl : nullptr, nullptr, st);
        if (int g = guard(hipMemcpyAsync(d_send, W.scale, npose * sizeof(double), hipMemcpyDeviceToDevice, st), "scaling rows")) return g;
        if (int g = guard(hipMemcpyAsync(d_send + npose, W.scale + (size_t)(F - 1) * npose, npose * sizeof(double), hipMemcpyDeviceToDevice, st), "scaling rows")) return g;
        if ((rc = gather(d_send, 2 * npose, "allgather (scaling rows)"))) return rc;
        if (halo) if (int g = guard(hipMemcpyAsync(d_sh, d_gath + (size_t)(R + 1) * 2 * npose, npose * sizeof(double), hipMemcpyDeviceToDevice, st), "scaling halo")) return g;
        if (has_left) if (int g = guard(hipMemcpyAsync(d_sl, d_gath + ((size_t)(R - 1) * 2 + 1) * npose, npose * sizeof(double), hipMemcpyDeviceToDevice, st), "scaling halo")) return g;
      }
      launch_win_assemble(P, W, p->d_frame_normal, p->d_r, d_x, d_const, 0, has_left ? d_xl : nullptr, halo ? d_sh : nullptr, st);
    }
    // ---- cyclic reduction over the local chain ----
    for (size_t l = 0; l < levels.size(); ++l) {
      const CrLevel& lv = levels[l];
      launch_cr_factor(W, d_sched + lv.elim_off, lv.n_elim, st);
      launch_cr_update(W, d_sched + lv.surv_off, lv.n_surv, st);
    }
    if (sharded) {
      // ---- interface system of the 2 N end frames: ONE all-gather (the shard's beta terms ride on it from the second
      //      iteration on), then every rank solves the same chain ----
      const int n_extra = 112;
      launch_iface_pack(W, F, W.Craw, n_extra, d_send, st);
      if ((rc = gather(d_send, iface_doubles(n_extra), "allgather (interface blocks)"))) return rc;
      launch_iface_unpack(Wi, d_gath, N, n_extra, d_cg, st);
      if (!first) {
        if (int g = guard(hipMemcpyAsync(W.Craw, d_cg, 110 * sizeof(double), hipMemcpyDeviceToDevice, st), "beta terms")) return g;
        launch_win_beta(P, W, p->d_frame_normal, p->d_r, 0, 2, st);
      }
      for (size_t l = 0; l < ilevels.size(); ++l) {
        const CrLevel& lv = ilevels[l];
        launch_cr_factor(Wi, d_sched + lv.elim_off, lv.n_elim, st);
        launch_cr_update(Wi, d_sched + lv.surv_off, lv.n_surv, st);
      }
      for (size_t l = ilevels.size(); l-- > 0;) launch_cr_back(Wi, d_sched + ilevels[l].elim_off, ilevels[l].n_elim, st);
      if (int g = guard(hipMemcpyAsync(W.Xt, Wi.Xt + (size_t)(2 * R) * rhs, rhs * 8, hipMemcpyDeviceToDevice, st), "interface solution")) return g;
      if (int g = guard(hipMemcpyAsync(W.Xt + (size_t)(F - 1) * rhs, Wi.Xt + (size_t)(2 * R + 1) * rhs, rhs * 8, hipMemcpyDeviceToDevice, st), "interface solution")) return g;
    }
    for (size_t l = levels.size(); l-- > 0;) launch_cr_back(W, d_sched + levels[l].elim_off, levels[l].n_elim, st);
    // ---- beta Schur complement, step, model change, decision ----
    launch_win_schur_part(P, W, st);
    if (!sharded) {
      launch_win_beta_solve(P, W, d_b, d_bn, 0, st);
      if (F <= 256) {
        launch_win_tail(P, W, d_x, d_b, d_xn, d_bn, st);      // step + model change + (last workgroup) decision in one launch
      } else {                                                // (long windows: the three kernels are bandwidth-bound, not
        launch_win_step(P, W, d_x, d_xn, st);                 //  launch-bound, and their separate grids fill the chip better)
        launch_win_model(P, W, d_x, nullptr, st);
        launch_win_finish(P, W, d_x, d_b, d_xn, d_bn, 0, st);
      }
    } else {
      // (a failed interface factorisation is everybody's failure: every rank factors the same chain and sees the same flag,
      //  k_win_finish folds it into the shard's own)
      launch_win_beta_solve(P, W, d_b, d_bn, 1, st);                     // this shard's Schur partials -> W.sred
      if ((rc = gather(W.sred, 112, "allgather (Schur partials)"))) return rc;
      launch_sum_ranks(d_gath, N, 112, 110, W.sred, st);
      launch_win_beta_solve(P, W, d_b, d_bn, 2, st);
      launch_win_step(P, W, d_x, d_xn, st);
      // the neighbours' boundary frames move by the steps their own shards compute (same arithmetic, same numbers)
      launch_win_halo_step(P, Wi.Xt, W.dsb, halo ? 2 * (R + 1) : -1, d_sh, d_x + (size_t)F * npose, d_dh, d_xn + (size_t)F * npose,
                           has_left ? 2 * R - 1 : -1, d_sl, d_xl, d_xln, st);
      launch_win_model(P, W, d_x, halo ? d_dh : nullptr, st);
      launch_win_fold_fail(W, Wi, st);
      launch_win_finish(P, W, d_x, d_b, d_xn, d_bn, 1, st);              // this shard's scalars -> W.fin[0..4]
    }
    if (!sharded) {
      rc = sweep(p, cand);
      if (rc) return rc;
      ++n_sweeps;
      launch_win_accept(P, W, d_rn, d_x, d_b, d_xn, d_bn, 0, st);
    } else {
      // the candidate is evaluated whatever the decision will be (it is taken once, below, from everybody's scalars)
      rc = sweep(p, cand);
      if (R == test_poison_rank && it == test_poison_iter) rc = fail(BODYFIT_ERR_HIP, "test hook: this rank's sweep failed");
      if (rc && !poison) { poison = rc; poison_msg = bodyfit_last_error(); }
      ++n_sweeps;
      launch_win_accept(P, W, d_rn, d_x, d_b, d_xn, d_bn, 3, st);       // this shard's cost at the candidate -> W.fin[5]
      if (poison) {
        static const double one = 1.0;
        (void)hipMemcpyAsync(W.fin + 6, &one, sizeof(double), hipMemcpyHostToDevice, st);
      }
      if ((rc = gather(W.fin, 8, "allgather (scalars)"))) return rc;
      launch_win_decide(P, W, d_x, d_b, d_xn, d_bn, d_gath, N, halo ? d_x + (size_t)F * npose : nullptr, d_xn + (size_t)F * npose,
                        has_left ? d_xl : nullptr, d_xln, st);
    }
    first = false;
    if (!opt->verbose && (it & 3) != 3 && it + 1 < opt->max_iters) {
      // The device takes every decision itself, so the host only looks at the status record every fourth iteration (a
      // read-back drains the launch pipeline: ~30 us of a ~250 us iteration at 20 frames).  Iterations launched after the
      // solve has terminated leave the state untouched (every kernel checks the active / candidate flags).
      continue;
    }
    HIP_TRY(hipMemcpyAsync(status, W.status, sizeof(status), hipMemcpyDeviceToHost, st));
    if (int rw = wait_status(st)) return rw;
    if (opt->verbose && R == 0)
      std::printf("[bodyfit-dev] it %3d cost %.6e radius %.3e accepted %d gmax %.2e\n", (int)status[kWsIters], status[kWsCost],
                  status[kWsRadius], (int)status[kWsAccepted], status[kWsGmax]);
    if (status[kWsActive] == 0.0) break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(status, W.status, sizeof(status), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(frame_params, d_x, (size_t)rows_x * npose * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(beta, d_b, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
  if (int rw = wait_status(st)) return rw;
  if (sharded && (poison || status[kWsPoison] != 0.0)) {
    if (summary) {
      *summary = bodyfit_fit_summary{};
      summary->iterations = (int)status[kWsIters]; summary->termination = 2; summary->usable = 0;
      summary->n_successful = (int)status[kWsOk]; summary->n_unsuccessful = (int)status[kWsBad];
      summary->n_sweeps = 1 + (int)status[kWsIters]; summary->n_sweeps_issued = n_sweeps;
      summary->initial_cost = status[kWsInitialCost]; summary->final_cost = status[kWsCost];
    }
    if (poison) return fail(poison, "sharded solve: this rank failed (" + poison_msg + "); every rank left at the same exchange");
    return fail(BODYFIT_ERR_HIP, "sharded solve: another rank reported a device failure; every rank left at the same exchange");
  }
  if (summary) {
    summary->iterations = (int)status[kWsIters];
    summary->termination = status[kWsActive] != 0.0 ? 1 : (int)status[kWsTermination];
    summary->usable = summary->termination != 2;
    summary->n_successful = (int)status[kWsOk]; summary->n_unsuccessful = (int)status[kWsBad];
    // the evaluations the solve NEEDED, from the device's own record: one at the start and one per iteration at the candidate —
    // that sweep also leaves the candidate's Jacobian (second buffers), so an accepted step costs no sweep of its own.  The loop
    // ISSUES a few more: between two status reads it runs up to three iterations past the termination (those kernels find the
    // solve inactive and leave the state alone); n_sweeps_issued is the host's own count.
    summary->n_sweeps = 1 + (int)status[kWsIters];
    summary->n_sweeps_issued = n_sweeps;
    summary->initial_cost = status[kWsInitialCost]; summary->final_cost = status[kWsCost];
  }
  return BODYFIT_OK;
}

// the unsharded entry (host_solver.cpp's router)
int bodyfit_internal_solve_window_device(bodyfit_problem* p, double* frame_params, double* beta,
                                         const unsigned char* param_constant, const bodyfit_fit_options* opt,
                                         bodyfit_fit_summary* summary, const bodyfit_comm* comm) {
  (void)comm;
  return solve_window_device(p, frame_params, beta, param_constant, opt, summary, nullptr, false);
}

static int sharded_common(bodyfit_problem* p, double* frame_params, double* beta, const unsigned char* param_constant,
                          Transport* tr, const bodyfit_fit_options* opt_in, bodyfit_fit_summary* summary, long* n_exchanges) {
  bodyfit_fit_options opt;
  opt.max_iters = 100; opt.scale_lo = -1e300; opt.scale_hi = 1e300; opt.verbose = 0; opt.solver = 3;
  if (opt_in) opt = *opt_in;
  int maxk = 0;
  for (int f = 0; f < p->d.F; ++f) maxk = std::max(maxk, p->kp_offset[f + 1] - p->kp_offset[f]);
  if (maxk > 32) return fail(BODYFIT_ERR_INVALID, "bodyfit_solve_sharded: at most 32 keypoints per frame");
  // BODYFIT_FORCE_SHARDED=1 (tests): a communicator of ONE rank still takes the sharded code path (interface system of its two
  // end frames, every exchange issued), which is how the RCCL transport is exercised on a box with a single GPU
  const char* fs = std::getenv("BODYFIT_FORCE_SHARDED");
  const long before = tr->n_calls;
  const int rc = solve_window_device(p, frame_params, beta, param_constant, &opt, summary, tr, fs && fs[0] == '1');
  if (n_exchanges) *n_exchanges = tr->n_calls - before;
  return rc;
}

// One window sharded over several processes (one per GPU): this rank's shard of the frames, exchanges through the caller's
// callbacks on host buffers (the transport of tests and of MPI hosts; bodyfit_solve_sharded_rccl keeps them on the device).
int bodyfit_solve_sharded(bodyfit_problem* p, double* frame_params, double* beta, const unsigned char* param_constant,
                          const bodyfit_comm* comm, const bodyfit_fit_options* opt_in, bodyfit_fit_summary* summary) {
  if (!p || !frame_params || !beta || !comm || !comm->allgather || comm->size < 1 || comm->rank < 0 || comm->rank >= comm->size)
    return fail(BODYFIT_ERR_INVALID, "bodyfit_solve_sharded: bad argument");
  HostTransport tr;
  tr.rank = comm->rank; tr.size = comm->size; tr.cb = *comm; tr.timeout_s = p->exchange_timeout_s;
  long n = 0;
  const int rc = sharded_common(p, frame_params, beta, param_constant, &tr, opt_in, summary, &n);
  p->last_exchanges = n;
  return rc;
}

// ---- RCCL transport ---------------------------------------------------------------------------------------------------------
struct bodyfit_rccl {
  RcclTransport tr;
  bool owns = false;
};

int bodyfit_rccl_unique_id(unsigned char* id128) {
  if (!id128) return fail(BODYFIT_ERR_INVALID, "null argument");
  RcclApi& A = RcclApi::get();
  if (!A.ok()) return fail(BODYFIT_ERR_HIP, A.error);
  RcclApi::unique_id id;
  const int rc = A.GetUniqueId(&id);
  if (rc != 0) return fail(BODYFIT_ERR_HIP, std::string("ncclGetUniqueId: ") + A.GetErrorString(rc));
  std::memcpy(id128, id.internal, 128);
  return BODYFIT_OK;
}

int bodyfit_rccl_create(const unsigned char* id128, int rank, int size, int device, bodyfit_rccl** out) {
  if (!id128 || !out || size < 1 || rank < 0 || rank >= size) return fail(BODYFIT_ERR_INVALID, "bodyfit_rccl_create: bad argument");
  *out = nullptr;
  RcclApi& A = RcclApi::get();
  if (!A.ok()) return fail(BODYFIT_ERR_HIP, A.error);
  HIP_TRY(hipSetDevice(device));
  RcclApi::unique_id id;
  std::memcpy(id.internal, id128, 128);
  std::unique_ptr<bodyfit_rccl> c(new bodyfit_rccl());
  const int rc = A.CommInitRank(&c->tr.comm, size, id, rank);
  if (rc != 0) return fail(BODYFIT_ERR_HIP, std::string("ncclCommInitRank: ") + A.GetErrorString(rc));
  c->tr.rank = rank; c->tr.size = size; c->owns = true;
  *out = c.release();
  return BODYFIT_OK;
}

int bodyfit_rccl_wrap(void* nccl_comm, int rank, int size, bodyfit_rccl** out) {
  if (!nccl_comm || !out || size < 1 || rank < 0 || rank >= size) return fail(BODYFIT_ERR_INVALID, "bodyfit_rccl_wrap: bad argument");
  RcclApi& A = RcclApi::get();
  if (!A.ok()) return fail(BODYFIT_ERR_HIP, A.error);
  bodyfit_rccl* c = new bodyfit_rccl();
  c->tr.comm = nccl_comm; c->tr.rank = rank; c->tr.size = size; c->owns = false;
  *out = c;
  return BODYFIT_OK;
}

void bodyfit_rccl_destroy(bodyfit_rccl* c) {
  if (!c) return;
  if (c->owns && c->tr.comm) (void)RcclApi::get().CommDestroy(c->tr.comm);
  delete c;
}

int bodyfit_solve_sharded_rccl(bodyfit_problem* p, double* frame_params, double* beta, const unsigned char* param_constant,
                               bodyfit_rccl* comm, const bodyfit_fit_options* opt_in, bodyfit_fit_summary* summary) {
  if (!p || !frame_params || !beta || !comm || !comm->tr.comm) return fail(BODYFIT_ERR_INVALID, "bodyfit_solve_sharded_rccl: bad argument");
  long n = 0;
  comm->tr.timeout_s = p->exchange_timeout_s;
  const int rc = sharded_common(p, frame_params, beta, param_constant, &comm->tr, opt_in, summary, &n);
  p->last_exchanges = n;
  return rc;
}

// The evaluation path's only collective ("one ncclAllReduce(sum, ncclDouble) per evaluation on [cost, g_beta, H_bb]"),
// in place on the caller's device buffer and stream: behind bodyfit_evaluate_device + bodyfit_reduce_shared_device (or the
// armed sweep's own tail) on the same stream it needs no host synchronisation and no Python hop.
int bodyfit_allreduce_shared_rccl(bodyfit_rccl* comm, double* d_buf66, void* stream) {
  if (!comm || !comm->tr.comm || !d_buf66) return fail(BODYFIT_ERR_INVALID, "bodyfit_allreduce_shared_rccl: bad argument");
  RcclApi& A = RcclApi::get();
  if (!A.ok()) return fail(BODYFIT_ERR_HIP, A.error);
  const int rc = A.AllReduce(d_buf66, d_buf66, 66, RcclApi::kDouble, RcclApi::kSum, comm->tr.comm, static_cast<hipStream_t>(stream));
  if (rc != 0) return fail(BODYFIT_ERR_HIP, std::string("ncclAllReduce: ") + (A.GetErrorString ? A.GetErrorString(rc) : "error"));
  return BODYFIT_OK;
}

// ranks of the communicator as RCCL itself reports them (ncclCommCount), and this process's rank in it (ncclCommUserRank)
int bodyfit_rccl_count(bodyfit_rccl* comm, int* n_ranks, int* rank) {
  if (!comm || !comm->tr.comm) return fail(BODYFIT_ERR_INVALID, "bodyfit_rccl_count: bad argument");
  RcclApi& A = RcclApi::get();
  if (!A.ok() || !A.CommCount || !A.CommUserRank) return fail(BODYFIT_ERR_HIP, A.ok() ? "librccl lacks ncclCommCount" : A.error);
  int n = 0, r = 0;
  int rc = A.CommCount(comm->tr.comm, &n);
  if (rc == 0) rc = A.CommUserRank(comm->tr.comm, &r);
  if (rc != 0) return fail(BODYFIT_ERR_HIP, std::string("ncclCommCount: ") + (A.GetErrorString ? A.GetErrorString(rc) : "error"));
  if (n_ranks) *n_ranks = n;
  if (rank) *rank = r;
  return BODYFIT_OK;
}

long bodyfit_last_exchange_count(const bodyfit_problem* p) { return p ? p->last_exchanges : 0; }

}  // extern "C"
