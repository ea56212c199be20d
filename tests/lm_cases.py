"""A named table of small fitting problems that take the LM solvers OFF the path every other solver test walks (a start from
rest pose on well-posed data: accepted steps only, convergence), each with the answer of the checker's LM (oracle/lm_dense.py).

Imported by the tests as a plain module (like domain_cases.py); numpy and the f64 CPU checker only, deterministic.  The checker's
answers are computed once per process and shared (answer(), pool_answer()): tests/test_lm_cases.py asserts on them alone that
every case is a fair parity case, tests/test_gpu_lm_branches.py compares the three product solvers with them.

THE CASES.  kind "frames": independent frames, one LM state each (host loop, batched device LM in both forms); the checker
solves every frame alone.  kind "window": one problem over all frames with a shared beta (host loop, device window LM).
A start "(sigma, seed)" is init_params (rest pose, s = 1, t = (0, 0, 3)) with the joints, then the root rotation, replaced by
N(0, sigma) draws from default_rng(seed); windows add the root draw to the start's instead.  Decisions: a = accepted step,
r = rejected step.  A "rejection run" case holds three or more consecutive rejections, an acceptance, and a later rejection:
the only trajectory on which the doubling of `decrease` AND its reset after an accepted step change the iterates.

What makes a case a FAIR parity case (asserted by tests/test_lm_cases.py for every case):
  (a) every step quality rho of the trace is at least RHO_MARGIN = 1e-2 away from the acceptance threshold 1e-3;
  (b) every model change of the trace is positive;
  (c) the dense and the sparse form of the checker (two correct restatements of one algorithm) take the same decisions, and
      their results differ by at most 1 / 100 of the tolerance of the GPU comparison: TOL_X / 100 in the parameters (the
      metric of param_diff), TOL_COST / 100 relative in the final cost.
A start that fails one of them is not a parity case -- ill-conditioned starts end a radian apart between the checker's two
forms -- and was replaced by another seed; the tolerances are the ones the iterate-for-iterate tests of the suite already use
(tests/test_gpu_fit.py test_c5_stage1_103_anchors_against_the_checkers_lm: 1e-6, 1e-8 relative).

Stopping reasons not in the table: `radius` (the trust region collapsing below 1e-32 takes fifteen consecutive rejections; no
start of the searches behind this table -- sigma 0.3 to 1.5, eight seeds each, pose-only and shape + GMM; windows at sigma 0.5
and 0.8 -- has more than six) stays covered by tests/cpp/lm_rules_test.cpp only; no input was constructed to force it.
"""
from __future__ import annotations

import re
from types import SimpleNamespace

import numpy as np

import model_variants as mv

synth = mv.synth

TOL_X = 1e-6          # parameters, product against checker (test_c5_stage1_103_anchors_against_the_checkers_lm)
TOL_COST = 1e-8       # final cost, relative (the same test)
TOL_INITIAL = 1e-9    # initial cost, relative (test_one_long_window_against_the_checkers_lm)
RHO_MARGIN = 1e-2     # condition (a)
UNBOUNDED = (-1e300, 1e300)

POSE = dict(n_cols=76, use_shape=False, beta_pose=20.0)
SHAPE = dict(n_cols=86, use_shape=True, beta_per_frame=True, beta_pose=20.0, gmm=True, beta_shape=30.0)
WINDOW = dict(n_cols=86, use_shape=True, beta_pose=5.0, beta_shape=25.0, lambda_temporal=3.0)

_cache: dict = {}


def model():
    if "model" not in _cache:
        _cache["model"] = synth.make_model(0)
    return _cache["model"]


def checker():
    """(oracle module, OracleModel, OracleGmm) of the suite's model and mixture"""
    if "checker" not in _cache:
        from oracle import oracle
        oracle.build()
        w, mu, cov = synth.make_gmm(0)
        _cache["checker"] = (oracle, oracle.OracleModel(model()), oracle.OracleGmm(w, mu, cov))
    return _cache["checker"]


def frames_of(seq, ids, empty=(), uv_edit=None):
    """the observations of frames `ids` of seq as a problem of their own; `empty`: positions left without keypoints;
    uv_edit: (position, keypoint, component, value) written into the copy"""
    offs, kid, uv = [0], [], []
    for pos, f in enumerate(ids):
        k0, k1 = (seq.kp_offset[f], seq.kp_offset[f + 1]) if pos not in empty else (0, 0)
        kid.append(seq.kp_id[k0:k1]); uv.append(seq.kp_uv[k0:k1].copy()); offs.append(offs[-1] + k1 - k0)
        if uv_edit is not None and uv_edit[0] == pos:
            uv[-1][uv_edit[1], uv_edit[2]] = uv_edit[3]
    ids = list(ids)
    return SimpleNamespace(kp_offset=np.array(offs, np.int32), kp_id=np.concatenate(kid).astype(np.int32),
                           kp_uv=np.concatenate(uv, 0).reshape(-1, 2), intr=seq.intr, R0=seq.R0[ids].copy(),
                           init_params=seq.init_params[ids].copy())


def start(init, sigma, seed, add_root=False):
    """init [F, 76] with the joints (first) and the root rotation drawn from N(0, sigma), default_rng(seed)"""
    rng = np.random.default_rng(seed)
    x0 = np.array(init, np.float64)
    F = len(x0)
    x0[:, 7:] = rng.normal(scale=sigma, size=(F, 69))
    root = rng.normal(scale=sigma, size=(F, 3))
    x0[:, 1:4] = x0[:, 1:4] + root if add_root else root
    return x0


def standard_constant():
    """joints 10 / 11 / 22 / 23 held constant (include/Sim3BA.h:608-611)"""
    c = np.zeros(76, np.uint8)
    for j in (10, 11, 22, 23):
        c[7 + 3 * (j - 1):10 + 3 * (j - 1)] = 1
    return c


def _case(name, group, kind, obs, x0, problem, beta0=None, constant=None, bounds=(0.3, 3.0), max_iters=25, why=None,
          run=False):
    """why: the stopping reason the case is in the table for (per frame for kind "frames"); run: a rejection-run case"""
    F = len(x0)
    if problem["n_cols"] > 76 and beta0 is None:
        beta0 = np.zeros((F, 10)) if kind == "frames" else np.zeros(10)
    return SimpleNamespace(name=name, group=group, kind=kind, obs=obs, x0=x0, beta0=beta0, problem=dict(problem),
                           constant=constant, bounds=bounds, max_iters=max_iters, why=why, run=run, n_frames=F)


def cases():
    """the table, in a fixed order"""
    if "cases" in _cache:
        return _cache["cases"]
    m = model()
    seq = synth.make_sequence(m, 4, seed=0, beta_fixed=True)      # pose only: the shape is known
    seqs = synth.make_sequence(m, 4, seed=1)                      # per-frame shape and GMM
    one, ones = frames_of(seq, [0]), frames_of(seqs, [0])
    init = one.init_params
    T = []
    # ---- rejection runs, single frame ----
    for sigma, seed in ((1.0, 7), (1.5, 0), (1.0, 2)):
        T.append(_case(f"pose_run_{sigma}_{seed}", "run_pose", "frames", one, start(init, sigma, seed), POSE, run=True))
    for sigma, seed in ((1.5, 4), (1.5, 3), (1.0, 3)):
        T.append(_case(f"shape_run_{sigma}_{seed}", "run_shape", "frames", ones, start(init, sigma, seed), SHAPE, run=True))
    # ---- windows: rejection run at F = 5 and F = 13 (the smallest window solver 0 gives to the device), a frame without
    #      keypoints in the middle ----
    for F in (5, 13):
        sw = synth.make_sequence(m, F, seed=2)
        T.append(_case(f"window{F}_run", "run_window", "window", frames_of(sw, range(F)), start(sw.init_params, 0.5, 0, True),
                       WINDOW, bounds=UNBOUNDED, max_iters=15, run=True))
    sw = synth.make_sequence(m, 5, seed=2)
    T.append(_case("window5_empty_middle", "window_empty", "window", frames_of(sw, range(5), empty=(2,)),
                   start(sw.init_params, 0.5, 0, True), WINDOW, bounds=UNBOUNDED, max_iters=15))
    # ---- every reason for stopping ----
    # gradient: a frame without keypoints at the L2 prior's minimum has a zero gradient at iteration 0 (beside an ordinary frame)
    two = frames_of(seq, [0, 1], empty=(0,))
    T.append(_case("stop_gradient", "why_gradient", "frames", two, two.init_params.copy(), POSE, why=("gradient", "function")))
    # parameter: the same frame away from the minimum -- an exactly quadratic cost, two full steps, then a step below 1e-8 |x|
    x0 = two.init_params.copy(); x0[0] = start(init, 0.3, 1)[0]
    T.append(_case("stop_parameter", "why_parameter", "frames", two, x0, POSE, why=("parameter", "function")))
    T.append(_case("stop_function", "why_function", "frames", one, start(init, 0.3, 1), POSE, max_iters=30, why=("function",)))
    # iterations: no iteration, one, and the fourth of `arrrrra...` -- a shrunken radius and a raised `decrease` are left behind
    for k in (0, 1, 4):
        T.append(_case(f"stop_iterations_{k}", "why_iterations", "frames", one, start(init, 1.0, 7), POSE, max_iters=k,
                       why=("iterations",)))
    T.append(_case("window5_iterations_0", "why_iterations", "window", frames_of(sw, range(5)), start(sw.init_params, 0.5, 0, True),
                   WINDOW, bounds=UNBOUNDED, max_iters=0, why="iterations"))
    # initial_cost: one observed coordinate NaN, one infinite -- data, like an occluded keypoint a loader did not filter
    T.append(_case("fail_nan", "why_initial_cost", "frames", frames_of(seq, [0], uv_edit=(0, 3, 0, np.nan)), init.copy(), POSE,
                   why=("initial_cost",)))
    T.append(_case("fail_inf", "why_initial_cost", "frames", frames_of(seq, [0], uv_edit=(0, 5, 1, np.inf)), init.copy(), POSE,
                   why=("initial_cost",)))
    T.append(_case("window5_fail_nan", "why_initial_cost", "window", frames_of(sw, range(5), uv_edit=(2, 7, 1, np.nan)),
                   sw.init_params.copy(), WINDOW, bounds=UNBOUNDED, max_iters=15, why="initial_cost"))
    # ---- active scale bounds, independent frames: the scale ends exactly on the upper bound, every step is projected ----
    x0 = start(init, 1.0, 7)
    T.append(_case("bounds_active", "bounds", "frames", one, x0, POSE, bounds=(0.95, 1.0)))
    # ---- almost everything constant: three unknowns in the 16-wide diagonal-block Cholesky ----
    only_t = np.ones(76, np.uint8); only_t[4:7] = 0
    for name, t in (("translation_only_near", (0.4, -0.3, 4.0)), ("translation_only_far", (1.5, -1.0, 8.0))):
        x0 = init.copy(); x0[:, 4:7] = t
        T.append(_case(name, "translation_only", "frames", one, x0, POSE, constant=only_t))
    # ---- the standard constant joints on a rejection-run start ----
    x0 = start(init, 1.0, 7); x0[:, standard_constant().astype(bool)] = 0.0
    T.append(_case("constant_joints_run", "constant_joints", "frames", one, x0, POSE, constant=standard_constant(), run=True))
    assert len({c.name for c in T}) == len(T)
    _cache["cases"] = T
    return T


GROUPS = ("run_pose", "run_shape", "run_window", "window_empty", "why_gradient", "why_function", "why_parameter", "why_iterations",
          "why_initial_cost", "bounds", "translation_only", "constant_joints")


def get(name):
    return next(c for c in cases() if c.name == name)


def pool():
    """Eight independent frames for ONE batched solve, built from the table's observations and starts, that leave the pooled LM
    state at different iterations for different reasons: two rejection-run starts, a gradient stop at iteration 0, the NaN
    and the inf frame, a start that runs into the iteration limit, the bound-active start, a plain start from rest pose.
    One configuration for all (pose only, scale in [0.95, 1], 25 iterations)."""
    if "pool" in _cache:
        return _cache["pool"]
    m = model()
    seq = synth.make_sequence(m, 8, seed=0, beta_fixed=True)
    obs = frames_of(seq, range(8), empty=(2,))
    obs.kp_uv[obs.kp_offset[3] + 3, 0] = np.nan
    obs.kp_uv[obs.kp_offset[4] + 5, 1] = np.inf
    x0 = obs.init_params.copy()
    x0[0] = start(x0[:1], 1.0, 7)[0]
    x0[1] = start(x0[:1], 1.5, 0)[0]
    x0[5] = start(x0[:1], 0.3, 1)[0]       # (converges late, after a rejection run; frames 0, 1 and 6 run into the limit)
    x0[6] = get("bounds_active").x0[0]
    x0[6, 1:4] += 0.05                     # (not a copy of frame 0's start)
    _cache["pool"] = _case("pool", "pool", "frames", obs, x0, POSE, bounds=(0.95, 1.0))
    return _cache["pool"]


def reversed_frames(case):
    """the same independent frames in reverse order"""
    o = case.obs
    F = case.n_frames
    obs = SimpleNamespace(kp_offset=o.kp_offset, kp_id=o.kp_id, kp_uv=o.kp_uv, intr=o.intr, R0=o.R0, init_params=o.init_params)
    rev = frames_of(obs, range(F - 1, -1, -1))
    return _case(case.name + "_reversed", case.group, "frames", rev, case.x0[::-1].copy(), case.problem,
                 beta0=None if case.beta0 is None else case.beta0[::-1].copy(), constant=case.constant, bounds=case.bounds,
                 max_iters=case.max_iters)


def single(case, f):
    """frame f of a case of independent frames as a case of its own"""
    obs = frames_of(case.obs, [f])
    return _case(f"{case.name}[{f}]", case.group, "frames", obs, case.x0[f:f + 1].copy(), case.problem,
                 beta0=None if case.beta0 is None else case.beta0[f:f + 1].copy(), constant=case.constant, bounds=case.bounds,
                 max_iters=case.max_iters)


# ---- the checker's answers ---------------------------------------------------------------------------------------------------
def _solve(case, obs, x0, beta0, sparse):
    from oracle import lm_dense
    _, om, ogmm = checker()
    p = case.problem
    with np.errstate(all="ignore"):      # (the NaN and inf cases)
        return lm_dense.solve(om, obs, x0, beta0, n_cols=p["n_cols"], use_shape=p["use_shape"], beta_pose=p.get("beta_pose", 0.0),
                              ogmm=ogmm if p.get("gmm") else None, beta_shape=p.get("beta_shape", 0.0),
                              lam=p.get("lambda_temporal", 0.0), max_iters=case.max_iters, constant=case.constant,
                              scale_bounds=case.bounds, sparse=sparse)


def _answers(case):
    """per problem of the case (one per frame for kind "frames", one for a window): dense = (x, beta, info), sparse likewise"""
    out = []
    if case.kind == "window":
        out.append(SimpleNamespace(dense=_solve(case, case.obs, case.x0, case.beta0, False),
                                   sparse=_solve(case, case.obs, case.x0, case.beta0, True)))
    else:
        for f in range(case.n_frames):
            one = single(case, f)
            b0 = None if one.beta0 is None else one.beta0[0]
            out.append(SimpleNamespace(dense=_solve(case, one.obs, one.x0, b0, False), sparse=_solve(case, one.obs, one.x0, b0, True)))
    return out


def answer(case):
    key = ("answer", case.name)
    if key not in _cache:
        _cache[key] = _answers(case)
    return _cache[key]


def cost_is_finite(cost):
    from oracle import lm_dense
    return lm_dense.cost_finite(cost)


def decisions(info):
    return "".join("a" if t["accepted"] else "r" for t in info["trace"])


def has_run(dec):
    """three or more consecutive rejections, an acceptance, and a later rejection"""
    m = re.search(r"r{3,}a", dec)
    return bool(m) and "r" in dec[m.end():]


def rho_margin(info):
    return min([abs(t["rho"] - 1e-3) for t in info["trace"] if t["rho"] is not None], default=np.inf)


def min_model(info):
    return min([t["model"] for t in info["trace"] if t["model"] is not None], default=np.inf)


def param_diff(case, x, b, xo, bo):
    """max |difference| of the parameters; with an unbounded scale modulo the gauge (s, t) -> (c s, c t), an exact null
    direction of every reprojection residual: rotations directly, the translation as t / s (tests/test_gpu_fit.py)"""
    x, xo = np.atleast_2d(x), np.atleast_2d(xo)
    if case.bounds == UNBOUNDED:
        d = max(np.abs(np.delete(x, [0, 4, 5, 6], axis=1) - np.delete(xo, [0, 4, 5, 6], axis=1)).max(),
                np.abs(x[:, 4:7] / x[:, :1] - xo[:, 4:7] / xo[:, :1]).max())
    else:
        d = np.abs(x - xo).max()
    if b is not None and bo is not None and np.size(bo):
        d = max(d, np.abs(np.asarray(b) - np.asarray(bo)).max())
    return float(d)


def spread(case, ans):
    """dense against sparse checker: (parameters, relative final cost)"""
    (xd, bd, infd), (xs, bs, infs) = ans.dense, ans.sparse
    with np.errstate(invalid="ignore"):
        dc = abs(infd["final_cost"] - infs["final_cost"])
    if np.isfinite(infd["final_cost"]) and infd["final_cost"] > 0:
        dc /= infd["final_cost"]
    elif not np.isfinite(infd["final_cost"]):
        dc = 0.0 if (np.isnan(infd["final_cost"]) == np.isnan(infs["final_cost"])) else np.inf
    return param_diff(case, xd, bd, xs, bs), float(dc)


def table_rows():
    """(name, frame, decisions, why, rho margin, parameter spread, cost spread) for every problem of the table"""
    rows = []
    for c in cases():
        for f, a in enumerate(answer(c)):
            info = a.dense[2]
            sx, sc = spread(c, a)
            rows.append((c.name, f, decisions(info), info["why"], rho_margin(info), sx, sc))
    return rows
