"""GPU: the three LM loops off the happy path -- rejected steps and runs of them, every reason for stopping, failures, active
bounds, constant blocks -- on the table of tests/lm_cases.py, iterate for iterate against the checker's LM (oracle/lm_dense.py)
and against each other:
  independent frames   host loop (solver 1), batched device LM (solver 2) in its speculative and its four-launch form
  shared-beta windows  host loop (solver 1), device window LM (solver 3), and solver 0 at the 13-frame window it hands to the device
tests/test_lm_cases.py holds, on the checker alone, what makes each case a fair parity case; the tolerances are lm_cases' (the
ones the suite's iterate-for-iterate tests use), with the checker's own dense-against-sparse spread a hundred times below them."""
import os

import numpy as np
import pytest

import lm_cases as lc

pytestmark = pytest.mark.gpu

FRAME_SOLVERS = (("host", 1, False), ("device", 2, False), ("device_plain", 2, True))
_runs: dict = {}


def _solvers(case):
    if case.kind == "frames":
        return FRAME_SOLVERS
    return (("host", 1, False), ("window", 3, False)) + ((("auto", 0, False),) if case.n_frames == 13 else ())


def _solve(api, gpu_model, case, solver, plain):
    """one solve on a problem of its own: (x, beta, summaries); the call returning at all is the ABI's success"""
    kw = dict(case.problem)
    if kw.pop("gmm", False):
        kw["gmm"] = api.Gmm(*lc.synth.make_gmm(0))
    old = os.environ.get("BODYFIT_LM_PLAIN")
    os.environ["BODYFIT_LM_PLAIN"] = "1" if plain else "0"
    try:
        prob = api.Problem.from_sequence(gpu_model, case.obs, **kw)
        return prob.solve(case.x0, case.beta0, constant=case.constant, independent=case.kind == "frames", max_iters=case.max_iters,
                          scale_bounds=case.bounds, solver=solver)
    finally:
        if old is None:
            del os.environ["BODYFIT_LM_PLAIN"]
        else:
            os.environ["BODYFIT_LM_PLAIN"] = old


def _run(api, gpu_model, case, which):
    key = (case.name, which)
    if key not in _runs:
        name, solver, plain = next(s for s in _solvers(case) if s[0] == which)
        _runs[key] = _solve(api, gpu_model, case, solver, plain)
    return _runs[key]


def _ints(s):
    return (s.iterations, s.n_successful, s.n_unsuccessful, s.termination, s.usable)


def _problems(case, x, b, summ):
    """(x, beta, summary) per problem of the case: per frame for independent frames, one for a window"""
    if case.kind == "window":
        return [(x, b, summ[0])]
    return [(x[f:f + 1], None if b is None else b[f], summ[f]) for f in range(case.n_frames)]


def _rel(a, b):
    with np.errstate(invalid="ignore"):      # (inf - inf in the printed line of a failure case)
        return abs(a - b) / abs(b) if b != 0 else abs(a - b)


CASES = [c.name for c in lc.cases()]
PAIRS = [(c.name, s[0]) for c in lc.cases() for s in _solvers(c)]


@pytest.mark.parametrize("name,which", PAIRS)
def test_solver_matches_the_checker_iterate_for_iterate(api, gpu_model, name, which):
    case = lc.get(name)
    x, b, summ = _run(api, gpu_model, case, which)
    for f, ((xf, bf, s), a) in enumerate(zip(_problems(case, x, b, summ), lc.answer(case))):
        xo, bo, info = a.dense
        want = (info["iterations"], info["n_ok"], info["n_bad"], info["termination"], int(info["termination"] != 2))
        d = lc.param_diff(case, xf, bf, xo, bo)
        print(f"{name}[{f}] {which}: {_ints(s)} checker {want} ({info['why']}), cost {s.initial_cost:.6e} -> {s.final_cost:.6e}, "
              f"final cost rel. diff {_rel(s.final_cost, info['final_cost']):.2e}, parameters {d:.2e}")
        assert _ints(s) == want, (name, f, which, lc.decisions(info))
        if info["why"] == "initial_cost":
            # the failure branch: nothing is touched
            assert not lc.cost_is_finite(s.initial_cost)
            assert (s.iterations, s.termination, s.usable) == (0, 2, 0)
        else:
            assert _rel(s.initial_cost, info["initial_cost"]) <= lc.TOL_INITIAL
            assert _rel(s.final_cost, info["final_cost"]) <= lc.TOL_COST
            assert d <= lc.TOL_X
            if case.max_iters == 0:
                assert s.termination == 1 and s.final_cost == s.initial_cost
    if case.group == "why_initial_cost" or case.max_iters == 0:
        assert np.array_equal(x, case.x0)                                   # bit-identical to the input
        assert b is None or np.array_equal(b, case.beta0)
    if case.constant is not None:
        c = case.constant.astype(bool)
        assert np.array_equal(x[:, c], case.x0[:, c])
    if case.group == "bounds":
        assert x[0, 0] == lc.answer(case)[0].dense[0][0, 0] and x[0, 0] in case.bounds     # exactly on the bound


@pytest.mark.parametrize("name", CASES)
def test_solvers_agree_with_each_other(api, gpu_model, name):
    """tolerances of tests/test_gpu_window_lm.py: the same integers, 1e-9 relative on the cost, 1e-7 on the parameters (the scale,
    where it is bounded, 1e-6; unbounded it is the gauge); the two forms of the batched device LM bit for bit"""
    case = lc.get(name)
    names = [s[0] for s in _solvers(case)]
    runs = {w: _run(api, gpu_model, case, w) for w in names}
    xh, bh, sh = runs["host"]
    for w in names[1:]:
        x, b, summ = runs[w]
        for f, (s, s0) in enumerate(zip(summ, sh)):
            assert _ints(s) == _ints(s0), (name, w, f)
            if not lc.cost_is_finite(s0.initial_cost):
                assert not lc.cost_is_finite(s.initial_cost)
            else:
                assert _rel(s.initial_cost, s0.initial_cost) <= 1e-12 and _rel(s.final_cost, s0.final_cost) <= 1e-9, (name, w, f)
        assert np.abs(x[:, 1:] - xh[:, 1:]).max() < 1e-7 and (b is None or np.abs(b - bh).max() < 1e-7), (name, w)
        if case.bounds != lc.UNBOUNDED:
            assert np.abs(x[:, 0] - xh[:, 0]).max() < 1e-6
    if case.kind == "frames":
        (xs, bs, ss), (xp, bp, sp) = runs["device"], runs["device_plain"]
        for a, b in zip(ss, sp):
            assert _ints(a) == _ints(b)
            assert np.array_equal([a.initial_cost, a.final_cost], [b.initial_cost, b.final_cost], equal_nan=True)
        assert np.array_equal(xs, xp) and (bs is None or np.array_equal(bs, bp))
        if case.max_iters > 1:
            assert ss[0].n_sweeps < sp[0].n_sweeps     # (they ARE the two forms: one sweep per iteration against two)


def _same(a, b, what):
    """every frame's result of two solves, bit for bit: a, b = (x, beta, summaries)"""
    for f, (s, t) in enumerate(zip(a[2], b[2])):
        assert _ints(s) == _ints(t), (what, f, _ints(s), _ints(t))
        assert np.array_equal([s.initial_cost, s.final_cost], [t.initial_cost, t.final_cost], equal_nan=True), (what, f)
        assert np.array_equal(a[0][f], b[0][f]), (what, f, np.abs(a[0][f] - b[0][f]).max())


@pytest.mark.parametrize("which,solver,plain", FRAME_SOLVERS)
def test_pool_isolation(api, gpu_model, which, solver, plain):
    """Eight frames that leave one batched solve at different iterations for different reasons (lm_cases.pool: rejection runs, a
    gradient stop at iteration 0, a NaN and an inf frame, the iteration limit, an active bound, a plain fit): every frame's
    summary and parameters are those of the same frame solved alone by the same solver, bit for bit -- one workgroup per frame
    in k_lm_step / k_lm_accept, every reduction per frame, and the evaluator's frames are independent of the batch
    (test_large_batch_equals_small_batches).  The batch twice gives the same bits; the frames in reverse order give every frame
    the same result."""
    pool = lc.pool()
    batch = _solve(api, gpu_model, pool, solver, plain)
    F = pool.n_frames
    outcomes = {(_ints(s)[0], _ints(s)[3]) for s in batch[2]}
    print(f"pool {which}:", [_ints(s) for s in batch[2]])
    assert len(outcomes) >= 4 and {s.termination for s in batch[2]} == {0, 1, 2}
    for f in range(F):
        alone = _solve(api, gpu_model, lc.single(pool, f), solver, plain)
        _same((batch[0][f:f + 1], None, batch[2][f:f + 1]), alone, f"{which}: frame {f} alone")
    _same(batch, _solve(api, gpu_model, pool, solver, plain), f"{which}: the batch again")
    rev = _solve(api, gpu_model, lc.reversed_frames(pool), solver, plain)
    _same(batch, (rev[0][::-1], None, rev[2][::-1]), f"{which}: reverse order")
