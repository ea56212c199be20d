"""GPU: every kernel on the model shapes the API accepts beyond SMPL's (tests/model_variants.py: 0..10 shape coefficients,
no pose correctives, V from one partial tile to many VJP chunks, trees from a star to depth 13, 1..23 joints), against the
f64 checker; and the shapes bodyfit_model_create / bodyfit_problem_create refuse.

Bounds are those of the SMPL-shape tests: residuals 1e-9 px and the Jacobian 1e-9 of its largest entry
(test_gpu_parity.py), joints 1e-11 m and the f32 cloud 5e-6 m (test_mesh_forward_matches_oracle), one launch against two
at the bounds of test_gpu_one_launch.py, the VJP at 1e-4 of each frame's largest entry (test_gpu_forward_vjp.py) plus two
per-column bounds: against the column's largest entry over the frames (test_vjp_matches_checker_on_every_shape) and, entry by
entry, 2^-14 S_fc + CD_fc (joints only: 1e-9 S_fc; tests/domain_cases.py)."""
import importlib

import numpy as np
import pytest

import domain_cases as dc
import model_variants as mv
from test_gpu_fit import TOL, gauge_free_diff
from test_gpu_one_launch import _Env, _timeouts

pytestmark = pytest.mark.gpu

api = importlib.import_module("3dbodyanimation_amd.api")
synth = mv.synth
_models: dict = {}


def _gm(v):
    if v.id not in _models:
        if api.device_count() < 1:
            pytest.fail("no GPU visible: -m gpu tests need an MI355X (there is no CPU fallback)")
        _models[v.id] = api.Model(v.model, pose_blend_data=v.pose_blend_data)
    return _models[v.id]


@pytest.fixture(scope="module")
def gmm_data():
    return synth.make_gmm(0, n_comp=3)


def _oracle_rows(oracle_mod, om, v, obs, x, beta, n_cols, use_shape, beta_pose, ogmm, beta_shape, lam):
    """the whole residual vector in the ABI's row layout, from the checker (temporal rows: rootT, rootAA, joints)"""
    F = len(obs.kp_offset) - 1
    b = beta if beta is not None else np.zeros(max(v.n_shape, 1))
    r, J = om.evaluate_batch(obs, x, b, n_cols, use_shape, v.pose_blend_data, mode=0)
    parts, comps = [r], np.zeros(F, int)
    if beta_pose > 0:
        for f in range(F):
            rp, _, k = oracle_mod.pose_prior(ogmm, beta_pose, x[f, 7:])
            parts.append(rp); comps[f] = k
    if beta_shape > 0 and n_cols > v.npose and v.n_shape:
        parts.append(beta_shape * np.asarray(beta).reshape(-1))
    if lam > 0:
        for f in range(F - 1):
            a, c = x[f], x[f + 1]
            parts.append(lam * np.concatenate([a[4:7] - c[4:7], a[1:4] - c[1:4], a[7:] - c[7:]]))
    return np.concatenate(parts), J, comps


SETUPS = ["kp_shape", "kp_no_shape", "shared_priors", "per_frame_priors"]


@pytest.mark.parametrize("F", [1, 33])
@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("vid", mv.ACCEPTED)
def test_evaluate_matches_checker(oracle_mod, gmm_data, vid, setup, F):
    """Residuals and Jacobian of FK-joint and landmark keypoints (every one of the model's), with and without the shape
    block in use, shared and per-frame beta, with the shape prior, temporal rows and (24 joints) the L2 or GMM pose prior;
    joints at exactly zero rotation and at theta^2 just below and above DBL_EPSILON (model_variants.random_params)."""
    v = mv.get(vid)
    gm, om = _gm(v), mv.oracle_model(oracle_mod, v)
    obs = mv.observations(v, F, seed=F + 3)
    rng = np.random.default_rng(F)
    x = mv.random_params(rng, v, F)
    nS, n_cols = v.n_shape, v.npose + v.n_shape
    use_shape = setup != "kp_no_shape" and nS > 0
    per_frame = setup in ("kp_shape", "per_frame_priors")
    beta = (rng.normal(size=(F, nS)) if per_frame else rng.normal(size=nS)) if nS else None
    bp = bs = lam = 0.0
    gmm = ogmm = None
    if setup == "shared_priors":
        bs, lam = 25.0, 3.0
        bp = 5.0 if v.n_joints == 24 else 0.0
    elif setup == "per_frame_priors":
        bs = 30.0
        if v.n_joints == 24:
            bp = 20.0
            gmm, ogmm = api.Gmm(*gmm_data), oracle_mod.OracleGmm(*gmm_data)
    prob = api.Problem(gm, obs.kp_offset, obs.kp_id, obs.kp_uv, obs.intr, obs.R0, n_cols=n_cols, use_shape=use_shape,
                       beta_per_frame=per_frame and nS > 0, beta_pose=bp, gmm=gmm, beta_shape=bs, lambda_temporal=lam)
    r, J, comp = prob.evaluate(x, beta, True)
    ro, Jo, co = _oracle_rows(oracle_mod, om, v, obs, x, beta, n_cols, use_shape, bp, ogmm, bs, lam)
    assert r.shape == ro.shape and J.shape == Jo.shape
    assert np.abs(r - ro).max() < 1e-9
    assert np.abs(J - Jo).max() < 1e-9 * max(1.0, np.abs(Jo).max())
    if ogmm is not None:
        assert np.array_equal(comp, co)
    r2, J2, _ = prob.evaluate(x, beta, False)
    assert J2 is None and np.array_equal(r, r2)


@pytest.mark.parametrize("F", [1, 33])
@pytest.mark.parametrize("vid", mv.ACCEPTED)
def test_forward_matches_checker(oracle_mod, vid, F):
    """Joints of every frame at 1e-11; the f32 cloud (mesh-capable shapes) at 5e-6 in every frame."""
    v = mv.get(vid)
    gm, om = _gm(v), mv.oracle_model(oracle_mod, v)
    obs = mv.observations(v, F, seed=F)
    rng = np.random.default_rng(F + 1)
    x = mv.random_params(rng, v, F)
    beta = rng.normal(size=(F, v.n_shape)) if v.n_shape else None
    prob = api.Problem(gm, obs.kp_offset, obs.kp_id, obs.kp_uv, obs.intr, obs.R0, n_cols=v.npose + v.n_shape,
                       use_shape=v.n_shape > 0, beta_per_frame=v.n_shape > 0, want_mesh=v.mesh_capable)
    joints, cloud = prob.forward(x, beta, want_cloud=v.mesh_capable)
    b = beta if beta is not None else np.zeros((F, 1))
    jo, co = om.forward_batch(x, b, obs.R0, v.n_shape > 0, v.pose_blend_data, want_cloud=v.mesh_capable)
    assert np.abs(joints - jo).max() < 1e-11
    if v.mesh_capable:
        assert np.abs(cloud - co).max() < 5e-6


ONE_LAUNCH = ["v31", "v289", "ns0", "ns6", "nopd", "deep13", "star"]


@pytest.mark.parametrize("F", [1, 33, 257])
@pytest.mark.parametrize("vid", ONE_LAUNCH)
def test_one_launch_equals_two_launches(gmm_data, vid, F):
    """The one-launch sweep against the two-launch sweep of the same build, several back-to-back launches with new
    parameters, at the bounds of test_gpu_one_launch.py::test_one_launch_equals_two_launches."""
    v = mv.get(vid)
    gm = _gm(v)
    seq = synth.make_sequence(v.model, F, seed=F)
    nS = v.n_shape
    kw = dict(n_cols=76 + nS, use_shape=nS > 0, beta_per_frame=nS > 0, beta_pose=20.0, gmm=api.Gmm(*gmm_data),
              beta_shape=30.0, want_mesh=True)
    with _Env(BODYFIT_ONE_LAUNCH="1"):
        pf = api.Problem.from_sequence(gm, seq, **kw)
    with _Env(BODYFIT_ONE_LAUNCH="0"):
        pt = api.Problem.from_sequence(gm, seq, **kw)
    rng = np.random.default_rng(F)
    for _ in range(4):
        x = seq.gt_params + 0.05 * rng.standard_normal(seq.gt_params.shape)
        beta = np.tile(seq.gt_beta, (F, 1)) + 0.3 * rng.standard_normal((F, nS)) if nS else None
        rf, Jf, cf = pf.evaluate(x, beta, True)
        rt, Jt, ct = pt.evaluate(x, beta, True)
        jf, clf = pf.forward(x, beta)
        jt, clt = pt.forward(x, beta)
        assert np.array_equal(cf, ct)
        np.testing.assert_allclose(rf, rt, rtol=0, atol=1e-10)
        np.testing.assert_allclose(Jf, Jt, rtol=0, atol=1e-9)
        np.testing.assert_allclose(jf, jt, rtol=0, atol=1e-12)
        np.testing.assert_allclose(clf, clt, rtol=0, atol=2e-6)
    assert _timeouts(pf) == 0


def _kp_free(gm, F, R0, **kw):
    return api.Problem(gm, np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), (1000.0, 1000.0, 960.0, 540.0),
                       R0, **kw)


ROW_TOL = 1e-4        # of each frame's largest entry (test_gpu_forward_vjp.py)
COL_TOL = 5e-4        # of each column's own largest entry over the frames, with a floor; measured worst 1.36e-4 (x3.7)
COL_FLOOR = 1e-3      # of the frame's largest entry


def _check_vjp(g, g_ref, row_floor=None):
    """row bound, then the per-column bound; returns the worst column ratio.  row_floor: the frames' parameter-gradient
    scale, for the beta gradient (with one shape coefficient its row is a single entry, which may be small)"""
    g, g_ref = np.atleast_2d(g), np.atleast_2d(g_ref)
    row = np.abs(g_ref).max(1, keepdims=True)
    if row_floor is not None:
        row = np.maximum(row, np.asarray(row_floor).reshape(row.shape[0], -1).max(1, keepdims=True))
    err = np.abs(g - g_ref)
    assert (err <= ROW_TOL * row).all(), err.max()
    col = np.maximum(np.abs(g_ref).max(0, keepdims=True), max(COL_FLOOR * row.max(), 1e-300))
    worst = (err / col).max()
    assert worst <= COL_TOL, (worst, int((err / col).max(0).argmax()))
    return worst


@pytest.mark.parametrize("F", [1, 33])
@pytest.mark.parametrize("vid", mv.MESH)
def test_vjp_matches_checker_on_every_shape(oracle_mod, vid, F):
    """Cloud-plus-joints gradient against central differences of the checker's forward, per-frame beta (shared beta for
    F = 1); ns0 has no beta block (grad_beta absent).  Each column is also bounded against its own magnitude (floor: 1e-3
    of the largest entry), so that a leaf joint's columns cannot hide under the translation gradient: measured worst column
    error 1.36e-4 of the column's magnitude over these shapes (the f32 / bf16 cloud path), bound 5e-4.  Deterministic, and
    the first frame's gradient does not depend on the frame count."""
    v = mv.get(vid)
    gm, om = _gm(v), mv.oracle_model(oracle_mod, v)
    rng = np.random.default_rng(F + 5)
    x = mv.random_params(rng, v, F, pose_sigma=0.2)
    nS = v.n_shape
    per_frame = F > 1 and nS > 0
    beta = (rng.normal(size=(F, nS)) if per_frame else rng.normal(size=nS)) if nS else None
    R0 = np.tile(synth.R0_DEFAULT.reshape(1, 9), (F, 1))
    G = rng.normal(size=(F, v.model.n_verts, 3)).astype(np.float32)
    H = rng.normal(size=(F, v.n_joints, 3))
    prob = _kp_free(gm, F, R0, n_cols=76 + nS, use_shape=nS > 0, beta_per_frame=per_frame, want_mesh=True)
    gx, gb = prob.forward_vjp(x, beta, G, H)
    b_ref = beta if beta is not None else np.zeros(1)
    ref = dc.ref_grad_scaled(om, x, b_ref, R0, G, H, nS > 0, v.pose_blend_data, per_frame, nS > 0)   # (mv.ref_grad's numbers)
    gx_ref, gb_ref = ref.gx, ref.gb
    _check_vjp(gx, gx_ref)
    dc.check_columns(gx, gx_ref, ref.Sx, ref.CDx, what=f"vjp {vid} F={F} dL/dx")           # 2^-14 S_fc + CD_fc
    if nS == 0:
        assert gb is None
    else:
        _check_vjp(gb, gb_ref, np.abs(gx_ref).max(1).sum() if not per_frame else np.abs(gx_ref).max(1))
        dc.check_columns(gb, gb_ref, ref.Sb, ref.CDb, what=f"vjp {vid} F={F} dL/dbeta")
    gx2, gb2 = prob.forward_vjp(x, beta, G, H)
    assert np.array_equal(gx, gx2) and (gb is None or np.array_equal(gb, gb2))
    if F > 1:
        p1 = _kp_free(gm, 1, R0[:1], n_cols=76 + nS, use_shape=nS > 0, beta_per_frame=per_frame, want_mesh=True)
        g1, b1 = p1.forward_vjp(x[:1], beta[:1] if per_frame else beta, G[:1], H[:1])
        assert np.array_equal(g1[0], gx[0]) and (not per_frame or np.array_equal(b1[0], gb[0]))


@pytest.mark.parametrize("F", [1, 33])
@pytest.mark.parametrize("vid", mv.FEW_JOINTS + ["deep13", "star"])
def test_joints_only_vjp_matches_checker(oracle_mod, vid, F):
    """The joints-only gradient ([F, 7 + 3 (nJ - 1)] parameters) on models with fewer than 24 joints and on the deepest and
    the flattest tree, shared beta (all f64: measured worst column error 7.6e-7, under the same bounds)."""
    v = mv.get(vid)
    gm, om = _gm(v), mv.oracle_model(oracle_mod, v)
    rng = np.random.default_rng(F + 9)
    x = mv.random_params(rng, v, F, pose_sigma=0.2)
    nS = v.n_shape
    beta = rng.normal(size=nS)
    R0 = np.tile(synth.R0_DEFAULT.reshape(1, 9), (F, 1))
    H = rng.normal(size=(F, v.n_joints, 3))
    prob = _kp_free(gm, F, R0, n_cols=v.npose + nS, use_shape=True, want_mesh=False)
    gx, gb = prob.forward_vjp(x, beta, None, H)
    assert gx.shape == (F, v.npose)
    gx_ref, gb_ref = mv.ref_grad(om, x, beta, R0, None, H, True, v.pose_blend_data, False, True)
    _check_vjp(gx, gx_ref)
    _check_vjp(gb, gb_ref, np.abs(gx_ref).max(1).sum())
    # per column, f64: 1e-9 S_fc against fourth-order differences at t = 0 (tests/test_gpu_domain.py, _check_vjp)
    ref4 = dc.ref_grad_scaled(om, x, beta, R0, None, H, True, v.pose_blend_data, False, True, step=1e-3, order=4, zero_t=True)
    f64 = dict(rel=1e-9, add_cd=False, ref_share=0.5)
    # (random_params puts a joint at theta^2 just below DBL_EPSILON: the first-order Rodrigues branch, dR 2 theta off)
    dc.check_columns(gx, ref4.gx, ref4.Sx, ref4.CDx, what=f"joints-only vjp {vid} F={F} dL/dx",
                     slack=dc.first_order_slack(om, x, beta, R0, H, True, v.pose_blend_data), **f64)
    dc.check_columns(gb, ref4.gb, ref4.Sb, ref4.CDb, what=f"joints-only vjp {vid} F={F} dL/dbeta", **f64)
    gx2, gb2 = prob.forward_vjp(x, beta, None, H)
    assert np.array_equal(gx, gx2) and np.array_equal(gb, gb2)


def _frame_obs(seq, f):
    k0, k1 = seq.kp_offset[f], seq.kp_offset[f + 1]
    return mv.SimpleNamespace(kp_offset=np.array([0, k1 - k0], np.int32), kp_id=seq.kp_id[k0:k1], kp_uv=seq.kp_uv[k0:k1],
                              intr=seq.intr, R0=seq.R0[f:f + 1])


def test_fit_independent_frames_per_frame_beta_ns6(oracle_mod):
    """6 shape coefficients, frames fitted independently (device batched LM), against the dense LM frame by frame."""
    from oracle import lm_dense
    v = mv.get("ns6")
    gm, om = _gm(v), mv.oracle_model(oracle_mod, v)
    F = 4
    seq = synth.make_sequence(v.model, F, seed=1)
    kw = dict(n_cols=82, use_shape=True, beta_pose=20.0, beta_shape=30.0)
    prob = api.Problem.from_sequence(gm, seq, beta_per_frame=True, **kw)
    x, b, summ = prob.solve(seq.init_params, np.zeros((F, 6)), independent=True, max_iters=60)
    for f in range(F):
        xo, bo, info = lm_dense.solve(om, _frame_obs(seq, f), seq.init_params[f:f + 1], np.zeros(6), max_iters=60, **kw)
        assert summ[f].termination == 0 and info["termination"] == 0
        assert abs(summ[f].final_cost - info["final_cost"]) < 1e-5 * info["final_cost"]
        d, ok_s = gauge_free_diff(x[f], xo[0])
        assert d < TOL and ok_s and np.abs(b[f] - bo).max() < TOL


@pytest.mark.parametrize("vid", ["ns6", "nopd"])
def test_fit_window_shared_beta(oracle_mod, vid):
    """A short window with a shared beta (ns6: the fallback path, the device window needs 10 coefficients; nopd: no pose
    correctives), against the dense LM over the same rows."""
    from oracle import lm_dense
    v = mv.get(vid)
    gm, om = _gm(v), mv.oracle_model(oracle_mod, v)
    F = 6
    seq = synth.make_sequence(v.model, F, seed=2)
    nS = v.n_shape
    kw = dict(n_cols=76 + nS, use_shape=True, beta_pose=5.0, beta_shape=25.0)
    prob = api.Problem.from_sequence(gm, seq, lambda_temporal=3.0, pose_blend=v.pose_blend_data, **kw)
    x, b, summ = prob.solve(seq.init_params, np.zeros(nS), independent=False, max_iters=40)
    xo, bo, info = lm_dense.solve(om, seq, seq.init_params, np.zeros(nS), lam=3.0, max_iters=40,
                                  pose_blend=v.pose_blend_data, **kw)
    assert abs(summ[0].final_cost - info["final_cost"]) < 1e-5 * info["final_cost"]
    d, _ = gauge_free_diff(x, xo)
    assert d < TOL and np.abs(b - bo).max() < TOL


def _invalid(fn):
    with pytest.raises(api.BodyfitError) as e:
        fn()
    msg = str(e.value)
    assert msg.startswith("bodyfit status 1:"), msg   # BODYFIT_ERR_INVALID
    return msg


@pytest.mark.parametrize("vid", mv.FEW_JOINTS)
def test_fits_and_unsupported_roles_are_refused_below_24_joints(vid):
    """Below 24 joints: the solvers, the pose prior (69-dimensional) and the mesh path are refused, not answered wrongly."""
    v = mv.get(vid)
    gm = _gm(v)
    F = 3
    obs = mv.observations(v, F, seed=1, ragged=False)
    x = mv.random_params(np.random.default_rng(0), v, F)
    mk = lambda **kw: api.Problem(gm, obs.kp_offset, obs.kp_id, obs.kp_uv, obs.intr, obs.R0, **kw)
    prob = mk(n_cols=v.npose + v.n_shape, use_shape=True)
    assert "24-joint" in _invalid(lambda: prob.solve(x, np.zeros((F, v.n_shape)), independent=True))
    assert "24-joint" in _invalid(lambda: prob.solve(x, np.zeros(v.n_shape), independent=False))
    assert "pose prior" in _invalid(lambda: mk(n_cols=v.npose, use_shape=False, beta_pose=5.0))
    assert "mesh path" in _invalid(lambda: mk(n_cols=v.npose, use_shape=False, want_mesh=True))


@pytest.mark.parametrize("vid", ["deep14", "chain23"])
def test_model_create_refuses_deep_trees(vid):
    assert "deeper than 13" in _invalid(lambda: api.Model(mv.get(vid).model))
