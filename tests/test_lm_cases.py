"""CPU: the table of tests/lm_cases.py holds what it promises, on the checker's LM (oracle/lm_dense.py) alone, before any solver
of the product is compared with it (tests/test_gpu_lm_branches.py): every mandatory group has a case, every case stops for the
reason it is in the table for, and every case is a FAIR parity case -- conditions (a), (b), (c) of lm_cases' docstring.
Nothing here touches the library."""
import numpy as np
import pytest

import lm_cases as lc


def _ids():
    return [c.name for c in lc.cases()]


def test_every_mandatory_group_has_a_case():
    groups = {c.group for c in lc.cases()}
    assert groups == set(lc.GROUPS)
    by = {g: [c for c in lc.cases() if c.group == g] for g in lc.GROUPS}
    assert len(by["run_pose"]) >= 2 and len(by["run_shape"]) >= 2
    assert sorted(c.n_frames for c in by["run_window"]) == [5, 13]
    assert sorted(c.max_iters for c in by["why_iterations"] if c.kind == "frames") == [0, 1, 4]
    assert {c.kind for c in by["why_initial_cost"]} == {"frames", "window"}
    # sizes of the issue: at most 8 independent frames, windows of 5 and 13, at most 30 iterations, 25 keypoints per frame
    for c in lc.cases() + [lc.pool()]:
        assert c.max_iters <= 30 and np.diff(c.obs.kp_offset).max() <= 25
        assert c.n_frames <= 8 if c.kind == "frames" else c.n_frames in (5, 13)


def test_print_the_table():
    """the table of DESIGN.md (section "The LM solvers off the happy path")"""
    print("\ncase                     frame  decisions                       why           rho margin  dense-sparse x   cost")
    for name, f, dec, why, margin, sx, sc in lc.table_rows():
        print(f"  {name:24s} {f}  {dec or '-':30s}  {why:12s}  {margin:10.3g}  {sx:10.2e}  {sc:9.2e}")


@pytest.mark.parametrize("name", _ids())
def test_case_is_a_fair_parity_case(name):
    c = lc.get(name)
    for f, a in enumerate(lc.answer(c)):
        (xd, bd, infd), (xs, bs, infs) = a.dense, a.sparse
        # (a) no decision near the acceptance threshold, (b) every model change positive
        assert lc.rho_margin(infd) >= lc.RHO_MARGIN, (name, f, lc.rho_margin(infd))
        assert lc.min_model(infd) > 0.0, (name, f, lc.min_model(infd))
        # (c) the checker's two forms agree: decisions and integers exactly, results to 1 / 100 of the GPU tolerances
        assert lc.decisions(infd) == lc.decisions(infs)
        for k in ("iterations", "n_ok", "n_bad", "termination", "why"):
            assert infd[k] == infs[k], (name, f, k)
        sx, sc = lc.spread(c, a)
        assert sx <= lc.TOL_X / 100 and sc <= lc.TOL_COST / 100, (name, f, sx, sc)
        assert len(infd["trace"]) == infd["iterations"] == infd["n_ok"] + infd["n_bad"] <= c.max_iters


@pytest.mark.parametrize("name", _ids())
def test_case_does_what_it_is_in_the_table_for(name):
    c = lc.get(name)
    ans = lc.answer(c)
    infos = [a.dense[2] for a in ans]
    if c.why is not None:
        want = (c.why,) if isinstance(c.why, str) else c.why
        assert tuple(i["why"] for i in infos) == want
    if c.run:
        assert all(lc.has_run(lc.decisions(i)) for i in infos), [lc.decisions(i) for i in infos]
    for a, info in zip(ans, infos):
        term = {"gradient": 0, "parameter": 0, "function": 0, "iterations": 1, "initial_cost": 2, "radius": 2}[info["why"]]
        assert info["termination"] == term
    if c.group == "why_initial_cost":
        for a in ans:
            x, b, info = a.dense
            assert info["iterations"] == 0 and info["trace"] == [] and not lc.cost_is_finite(info["initial_cost"])
        x = np.concatenate([a.dense[0] for a in ans]) if c.kind == "frames" else ans[0].dense[0]
        assert np.array_equal(x, c.x0)                               # parameters untouched
    if c.group == "why_gradient":
        assert infos[0]["iterations"] == 0 and np.array_equal(ans[0].dense[0], c.x0[:1])
    if c.group == "why_iterations":
        for a, info in zip(ans, infos):
            assert info["iterations"] == c.max_iters
        if c.max_iters == 0:
            assert infos[0]["final_cost"] == infos[0]["initial_cost"]
            assert np.array_equal(ans[0].dense[0], c.x0 if c.kind == "window" else c.x0[:1])
        if c.max_iters == 4:          # stops inside the run: the last decisions are rejections
            assert lc.decisions(infos[0]).endswith("rrr")
    if c.group == "bounds":
        x, _, info = ans[0].dense
        assert x[0, 0] in c.bounds and any(t["projected"] for t in info["trace"])
        assert info["n_bad"] >= 1 and info["n_ok"] >= 5
    if c.group == "window_empty":
        assert np.diff(c.obs.kp_offset)[c.n_frames // 2] == 0 and infos[0]["n_ok"] >= 5
    if c.group == "translation_only":
        x = ans[0].dense[0]
        free = ~c.constant.astype(bool)
        assert free.sum() == 3 and np.array_equal(x[:, ~free], c.x0[:, ~free]) and infos[0]["n_ok"] >= 5
    if c.group == "constant_joints":
        assert np.array_equal(ans[0].dense[0][:, c.constant.astype(bool)], c.x0[:, c.constant.astype(bool)])


def test_rejections_are_in_every_translation_only_and_window_group():
    """the three-unknown Cholesky and both window sizes see rejected steps, not only accepted ones"""
    assert any("r" in lc.decisions(lc.answer(c)[0].dense[2]) for c in lc.cases() if c.group == "translation_only")
    for c in lc.cases():
        if c.group == "run_window":
            assert lc.has_run(lc.decisions(lc.answer(c)[0].dense[2]))


def test_pool_frames_stop_for_different_reasons():
    """the eight frames of the pool-isolation test leave the batch at different iterations for different reasons"""
    p = lc.pool()
    infos = [a.dense[2] for a in lc.answer(p)]
    whys = [i["why"] for i in infos]
    print("\npool:", [(w, i["iterations"], lc.decisions(i)) for w, i in zip(whys, infos)])
    assert whys[2] == "gradient" and infos[2]["iterations"] == 0
    assert whys[3] == whys[4] == "initial_cost"
    assert whys[7] == "function"
    assert "iterations" in whys
    assert sum("rrr" in lc.decisions(i) for i in infos) >= 2
    x6 = lc.answer(p)[6].dense[0]
    assert x6[0, 0] in p.bounds
    assert len({i["iterations"] for i in infos}) >= 4


def test_the_checker_states_the_initial_cost_rule_and_traces_every_decision():
    """oracle/lm_dense.py: a non-finite initial cost is a failure before the first iteration (it used to run max_iters rejected
    iterations and report termination 1); the trace holds the radius before every decision, which follows the rule"""
    info = lc.answer(lc.get("fail_nan"))[0].dense[2]
    assert (info["termination"], info["iterations"], info["n_bad"], info["why"]) == (2, 0, 0, "initial_cost")
    assert np.isnan(info["initial_cost"]) and np.isnan(info["final_cost"])
    assert lc.answer(lc.get("fail_inf"))[0].dense[2]["initial_cost"] == np.inf
    info = lc.answer(lc.get("pose_run_1.0_7"))[0].dense[2]
    radius, dec = 1e4, 2.0
    for t in info["trace"]:
        assert t["radius"] == radius
        if t["accepted"]:
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2 * t["rho"] - 1) ** 3)); dec = 2.0
        else:
            radius /= dec; dec *= 2
    assert set(info["trace"][0]) == {"radius", "accepted", "projected", "rho", "model", "cost"}
