"""GPU: every SMPL kernel on the table of tests/domain_cases.py (theta at and past pi and 2 pi, axis-aligned rotations, a flipped
root, a body that is near, far, off-axis or behind the camera, scales 0.05 and 20, |beta| = 5), against the f64 checker, with
bounds that scale with the frame and the column; tests/test_domain_cases.py validates the checker on the same table and shows
that these bounds reject wrong arithmetic.

Bounds, all per frame or per column (a loose frame never loosens another):
  residuals     reprojection rows 1e-9 max(1, P_f); prior / temporal rows 1e-9 max(1, max |r_ref|) of the frame's rows
  Jacobian      1e-9 max(1, max |J_ref|) of the frame's rows; GMM components equal; a residual-only sweep: the same bits
  joints        1e-11 max(1, M_f / 4)          (4 m: the largest coordinate the suite's 1e-11 has been asserted on)
  cloud         B_f = 4 E_f, E_f the error of the arithmetic model (domain_cases.model_cloud) on that frame; min(B_f, 5e-6) on
                control and rest; one launch against two: 2 B_f, 2e-6 on control
  JVP           unit tangents (the dense Jacobian): joints 1e-7, cloud 1e-4 of that (frame, column)'s largest entry (joints:
                + 2 theta D_f on the columns of a rotation in the first-order branch)
  VJP           1e-4 of the frame's largest entry AND |g - g_ref| <= 2^-14 S_fc + CD_fc per column; joints only: 1e-9 S_fc
                (+ 2 theta D_f sum |H| on the columns of a rotation in the first-order branch, domain_cases.first_order_slack)
  residual VJP  1e-9 sum |g| |J_ref| per column
  offsets       the cloud bound plus the header's 2^-24 (16 |s| |d_v|_1 + |cloud_d|); the VJP's two bounds
Models: model_variants v2049 for values, v289 for derivatives.  Every test prints its worst error / bound."""
import importlib

import numpy as np
import pytest

import domain_cases as dc
import model_variants as mv
import offsets_ref
from test_gpu_one_launch import _Env, _timeouts
from test_gpu_parity import _oracle_full
from test_gpu_residual_vjp import _oracle_dense, _split

pytestmark = pytest.mark.gpu

api = importlib.import_module("3dbodyanimation_amd.api")
synth = mv.synth
U = 2.0 ** -24
CONFIGS = ["pose_only_76", "shape_shared", "shape_per_frame_gmm"]
_models: dict = {}


def _gm(v):
    if v.id not in _models:
        if api.device_count() < 1:
            pytest.fail("no GPU visible: -m gpu tests need an MI355X (there is no CPU fallback)")
        _models[v.id] = api.Model(v.model, pose_blend_data=v.pose_blend_data)
    return _models[v.id]


def _report(what, ratio):
    print(f"domain {what}: worst error / bound = {float(ratio):.3e}")


@pytest.fixture(scope="module")
def val(oracle_mod):
    """v2049: the table with per-frame and with shared beta, the checker's forward, E_f and B_f"""
    v = mv.get("v2049")
    om = mv.oracle_model(oracle_mod, v)
    tabs = {}
    for shared in (False, True):
        tab = dc.cases(v, 0, shared_beta=shared, om=om)
        mag = dc.magnitudes(om, v, tab)
        tabs[shared] = (tab, mag, dc.cloud_bounds(tab, dc.model_errors(v, tab, mag.cloud)))
    return v, om, tabs


@pytest.fixture(scope="module")
def der(oracle_mod):
    """v289: the table and its reference Jacobians (central differences of the checker at steps 1e-6 and 2e-6; the joints'
    also to fourth order at 1e-3 and 2e-3), per-frame and shared beta"""
    v = mv.get("v289")
    om = mv.oracle_model(oracle_mod, v)
    out = {}
    for shared in (False, True):
        tab = dc.cases(v, 0, shared_beta=shared, om=om)
        out[shared] = mv.SimpleNamespace(
            tab=tab, J1=dc.dense_jacobian(om, tab.x, tab.beta, tab.R0, step=1e-6), J2=dc.dense_jacobian(om, tab.x, tab.beta, tab.R0, step=2e-6),
            Jj4=dc.joint_jacobian_o4(om, tab.x, tab.beta, tab.R0), Jj4b=dc.joint_jacobian_o4(om, tab.x, tab.beta, tab.R0, step=2e-3))
    return v, om, out


def _kp_free(gm, F, R0, **kw):
    kw.setdefault("want_mesh", True)
    return api.Problem(gm, np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), (1000.0, 1000.0, 960.0, 540.0),
                       R0, **kw)


def _config(cfg, val, oracle_mod):
    """(table, magnitudes, beta for the problem, beta for the checker, problem keywords, bp, ogmm, bs, lam, per_frame)"""
    v, om, tabs = val
    kw = dict(pose_blend=True, huber_delta=3.0, want_mesh=True)
    ogmm = None
    if cfg == "pose_only_76":       # the shape block is absent: the table without its beta
        tab = mv.SimpleNamespace(**vars(tabs[True][0]))
        tab.beta = np.zeros(v.n_shape)
        mag = dc.magnitudes(om, v, tab)
        kw.update(n_cols=76, use_shape=False, beta_pose=20.0)
        return tab, mag, None, kw, 20.0, None, 0.0, 0.0, False
    if cfg == "shape_shared":
        tab, mag, _ = tabs[True]
        kw.update(n_cols=86, use_shape=True, beta_pose=5.0, beta_shape=25.0, lambda_temporal=3.0)
        return tab, mag, tab.beta, kw, 5.0, None, 25.0, 3.0, False
    tab, mag, _ = tabs[False]
    w, mu, cov = synth.make_gmm(0)
    ogmm = oracle_mod.OracleGmm(w, mu, cov)
    kw.update(n_cols=86, use_shape=True, beta_per_frame=True, beta_pose=20.0, gmm=api.Gmm(w, mu, cov), beta_shape=30.0)
    return tab, mag, tab.beta, kw, 20.0, ogmm, 30.0, 0.0, True


# ---- residuals and Jacobian -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["two_launches", "one_launch"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_residuals_and_jacobian(val, oracle_mod, cfg, fused):
    v, om, _ = val
    tab, mag, beta, kw, bp, ogmm, bs, lam, per_frame = _config(cfg, val, oracle_mod)
    F = len(tab.names)
    obs = dc.observations(v, tab)
    with _Env(BODYFIT_ONE_LAUNCH="1" if fused else "0"):
        prob = api.Problem.from_sequence(_gm(v), obs, **kw)
    r, J, comp = prob.evaluate(tab.x, beta, True)
    n_cols, use_shape = kw["n_cols"], kw["use_shape"]
    ro, Jo, co = _oracle_full(oracle_mod, om, obs, tab.x, beta if beta is not None else np.zeros(v.n_shape), n_cols, use_shape,
                              True, bp, ogmm, bs, lam)
    assert r.shape == ro.shape and J.shape == Jo.shape
    worst_r = worst_J = 0.0
    K2 = prob.layout.reproj_rows
    npr = 70 if ogmm is not None else 69
    rows = K2
    for f, name in enumerate(tab.names):
        a, e = 2 * obs.kp_offset[f], 2 * obs.kp_offset[f + 1]
        if e > a:
            br, bJ = 1e-9 * max(1.0, mag.P[f]), 1e-9 * max(1.0, np.abs(Jo[a:e]).max())
            er, eJ = np.abs(r[a:e] - ro[a:e]).max(), np.abs(J[a:e] - Jo[a:e]).max()
            assert er <= br, (name, "reprojection", er, br)
            assert eJ <= bJ, (name, "Jacobian", eJ, bJ)
            worst_r, worst_J = max(worst_r, er / br), max(worst_J, eJ / bJ)
        groups = [slice(K2 + f * npr, K2 + (f + 1) * npr)]                                   # the frame's pose prior rows
        if per_frame:
            groups.append(slice(K2 + F * npr + f * v.n_shape, K2 + F * npr + (f + 1) * v.n_shape))
        if lam > 0 and f < F - 1:
            t0 = K2 + F * npr + v.n_shape + f * 75                                            # (shared beta: nS shape rows)
            groups.append(slice(t0, t0 + 75))
        for g in groups:
            b = 1e-9 * max(1.0, np.abs(ro[g]).max())
            er = np.abs(r[g] - ro[g]).max()
            assert er <= b, (name, "prior / temporal rows", er, b)
            worst_r = max(worst_r, er / b)
            rows += g.stop - g.start
    if bs > 0 and not per_frame:
        g = slice(K2 + F * npr, K2 + F * npr + v.n_shape)
        assert np.abs(r[g] - ro[g]).max() <= 1e-9 * max(1.0, np.abs(ro[g]).max())
        rows += v.n_shape
    assert rows == len(ro)                       # every row was held to a bound
    if ogmm is not None:
        assert np.array_equal(comp, co)
    r2, J2, _ = prob.evaluate(tab.x, beta, False)
    assert J2 is None and np.array_equal(r, r2)
    if fused:
        assert _timeouts(prob) == 0
    _report(f"residuals {cfg} {'one launch' if fused else 'two launches'}", worst_r)
    _report(f"Jacobian {cfg} {'one launch' if fused else 'two launches'}", worst_J)


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _forward_device(prob, x, beta, d=None):
    """bodyfit_forward_device (always the two-launch sweep) through device memory"""
    torch = importlib.import_module("torch")
    F, V = x.shape[0], prob.model.n_verts
    xt, bt = torch.tensor(x, device="cuda"), torch.tensor(beta, device="cuda")
    cloud = torch.full((F, 3 * V), float("nan"), dtype=torch.float32, device="cuda")
    joints = torch.empty((F, 24, 3), dtype=torch.float64, device="cuda")
    kw = {}
    if d is not None:
        dt = torch.tensor(d, device="cuda")
        kw = dict(d_offsets_ptr=dt.data_ptr(), offsets_frame_stride=3 * V)
    prob.forward_device(xt.data_ptr(), bt.data_ptr(), joints.data_ptr(), cloud.data_ptr(), 3 * V,
                        torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return joints.cpu().numpy(), cloud.reshape(F, V, 3).cpu().numpy()


@pytest.mark.parametrize("shared", [False, True], ids=["beta_per_frame", "beta_shared"])
def test_forward(val, shared):
    v, om, tabs = val
    tab, mag, B = tabs[shared]
    F = len(tab.names)
    obs = dc.observations(v, tab)
    kw = dict(n_cols=86, use_shape=True, beta_per_frame=not shared, want_mesh=True)
    with _Env(BODYFIT_ONE_LAUNCH="1"):
        p1 = api.Problem.from_sequence(_gm(v), obs, **kw)
    with _Env(BODYFIT_ONE_LAUNCH="0"):
        p2 = api.Problem.from_sequence(_gm(v), obs, **kw)
    j1, c1 = p1.forward(tab.x, tab.beta)                    # the one-launch cloud
    assert _timeouts(p1) == 0 and p1.sweep_timeouts() == 0
    j2, c2 = _forward_device(p2, tab.x, tab.beta)           # bodyfit_forward_device: two launches
    worst = dict(joints=0.0, one=0.0, two=0.0, between=0.0)
    fails = []
    for f, name in enumerate(tab.names):
        bj = 1e-11 * max(1.0, mag.M[f] / 4.0)
        e1, e2 = np.abs(c1[f] - mag.cloud[f]).max(), np.abs(c2[f] - mag.cloud[f]).max()
        e12 = np.abs(c1[f].astype(np.float64) - c2[f]).max()
        b12 = min(2 * B[f], 2e-6) if name in ("control", "control_empty") else 2 * B[f]
        ej = max(np.abs(j1[f] - mag.joints[f]).max(), np.abs(j2[f] - mag.joints[f]).max())
        print(f"  {name:14s} cloud error one launch {e1:.3e}  two launches {e2:.3e}  between {e12:.3e}  B_f {B[f]:.3e}  joints {ej:.2e}")
        for key, err, bound in (("joints", ej, bj), ("one", e1, B[f]), ("two", e2, B[f]), ("between", e12, b12)):
            worst[key] = max(worst[key], err / bound)
            if err > bound:
                fails.append((name, key, err, bound))
    for key in worst:
        _report(f"forward {key} ({'shared' if shared else 'per-frame'} beta)", worst[key])
    assert not fails, fails


# ---- forward JVP: the dense Jacobian by unit tangents -------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["beta_per_frame", "beta_shared"])
def test_forward_jvp_unit_tangents(der, shared):
    v, om, refs = der
    ref = refs[shared]
    tab = ref.tab
    F, nS = len(tab.names), v.n_shape
    K = 76 + nS
    eye = np.eye(K)
    tx = np.ascontiguousarray(np.broadcast_to(eye[:, :76], (F, K, 76)))
    tb = eye[:, 76:].copy() if shared else np.ascontiguousarray(np.broadcast_to(eye[:, 76:], (F, K, nS)))
    prob = _kp_free(_gm(v), F, tab.R0, n_cols=86, use_shape=True, beta_per_frame=not shared)
    tj, tc = prob.forward_jvp(tab.x, tab.beta, tx, tb)
    fails = []
    # a rotation in the first-order Rodrigues branch (tiny_1e-8) has dR_c = [e_c]x, 2 theta off the exponential's derivative
    # that the differences see: at most 2 theta D_f per entry of its joint tangents (domain_cases.first_order_slack)
    slack = np.zeros((F, K))
    slack[:, :76] = dc.first_order_slack(om, tab.x, tab.beta, tab.R0, None)
    for what, got, want, tol, extra in (("joints", tj, ref.Jj4, 1e-7, slack), ("cloud", tc, ref.J1[1], 1e-4, 0.0)):
        err = np.abs(got.astype(np.float64) - want).reshape(F, K, -1).max(-1)
        scale = np.abs(want).reshape(F, K, -1).max(-1)
        ratio = np.where(err == 0.0, 0.0, err / np.maximum(tol * scale + extra, 1e-300))
        _report(f"JVP {what} ({'shared' if shared else 'per-frame'} beta)", ratio.max())
        fails += [(what, tab.names[f], int(k), float(err[f, k]), float(scale[f, k])) for f, k in np.argwhere(ratio > 1.0)[:6]]
    assert not fails, fails


# ---- forward VJP --------------------------------------------------------------------------------------------------------------
def _contract(G, H, Jj, Jc):
    g = np.einsum("fjc,fkjc->fk", H, Jj)
    S = np.einsum("fjc,fkjc->fk", np.abs(H), np.abs(Jj))
    if G is not None:
        G64 = G.astype(np.float64)
        g += np.einsum("fvc,fkvc->fk", G64, Jc)
        S += np.einsum("fvc,fkvc->fk", np.abs(G64), np.abs(Jc))
    return g, S


def _check_vjp(what, gx, gb, g, S, CD, shared, rel, slack=0.0):
    """the row-maximum bound (cloud path: the suite's 1e-4) and the per-column bound, parameters and beta"""
    # joints only (f64): the bound is 1e-9 S_fc alone.  Its reference is a difference quotient of an f64 forward, good to about
    # 6e-17 m / step per entry: at theta = 2 pi a column's own scale S_fc is 2e-4 and that is a fifth of the bound (the worst
    # column of the table), so the reference is required to leave the kernel half of the bound, not nine tenths
    kw = dict(add_cd=True, ref_share=0.1) if rel == dc.VJP_REL else dict(add_cd=False, ref_share=0.5)
    if rel == dc.VJP_REL:
        assert dc.row_max_ok(gx, g[:, :76]), what
    dc.check_columns(gx, g[:, :76], S[:, :76], CD[:, :76], rel, f"domain {what} dL/dx", slack=slack, **kw)
    gb_ref, Sb, CDb = g[:, 76:], S[:, 76:], CD[:, 76:]
    if shared:
        gb_ref, Sb, CDb = gb_ref.sum(0), Sb.sum(0), np.abs(CDb.sum(0))
    if rel == dc.VJP_REL:
        assert dc.row_max_ok(gb, gb_ref), what
    dc.check_columns(gb, gb_ref, Sb, CDb, rel, f"domain {what} dL/dbeta", **kw)


@pytest.mark.parametrize("shared", [False, True], ids=["beta_per_frame", "beta_shared"])
def test_forward_vjp(der, shared):
    v, om, refs = der
    ref = refs[shared]
    tab = ref.tab
    F = len(tab.names)
    rng = np.random.default_rng(F)
    G = rng.normal(size=(F, v.model.n_verts, 3)).astype(np.float32)
    H = rng.normal(size=(F, 24, 3))
    prob = _kp_free(_gm(v), F, tab.R0, n_cols=86, use_shape=True, beta_per_frame=not shared)
    gx, gb = prob.forward_vjp(tab.x, tab.beta, G, H)
    g, S = _contract(G, H, *ref.J1)
    g2, _ = _contract(G, H, *ref.J2)
    # (a shared beta: the signed difference is summed over the frames before its magnitude is taken)
    CD = np.abs(g - g2)
    if shared:
        CD[:, 76:] = g[:, 76:] - g2[:, 76:]
    _check_vjp("VJP cloud + joints", gx, gb, g, S, CD, shared, dc.VJP_REL)
    # joints only: the f64 chain kernel alone, against the fourth-order differences
    gx, gb = prob.forward_vjp(tab.x, tab.beta, None, H)
    g, S = _contract(None, H, ref.Jj4, None)
    g2, _ = _contract(None, H, ref.Jj4b, None)
    CD = np.abs(g - g2)
    if shared:
        CD[:, 76:] = g[:, 76:] - g2[:, 76:]
    # (tiny_1e-8 is in the first-order Rodrigues branch: its dR is 2 theta off the exponential's, which the differences see)
    _check_vjp("VJP joints only", gx, gb, g, S, CD, shared, 1e-9, dc.first_order_slack(om, tab.x, tab.beta, tab.R0, H))


# ---- residual VJP ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
def test_residual_vjp(val, oracle_mod, cfg):
    v, om, _ = val
    tab, mag, beta, kw, bp, ogmm, bs, lam, per_frame = _config(cfg, val, oracle_mod)
    F, nS = len(tab.names), v.n_shape
    obs = dc.observations(v, tab)
    prob = api.Problem.from_sequence(_gm(v), obs, **kw)
    Jfull = _oracle_dense(oracle_mod, om, obs, tab.x, beta, kw["n_cols"], kw["use_shape"], True, bp, ogmm, bs, lam, per_frame, nS)
    assert Jfull.shape[0] == prob.layout.total_rows
    g = np.random.default_rng(7).normal(size=prob.layout.total_rows)
    gx, gb = prob.residual_vjp(tab.x, beta, g)
    has_beta = kw["n_cols"] > 76
    wx, wb = _split(Jfull.T @ g, F, 76, F, nS, per_frame, has_beta)
    sx, sb = _split(np.abs(Jfull).T @ np.abs(g), F, 76, F, nS, per_frame, has_beta)
    dc.check_columns(gx, wx, sx, np.zeros_like(sx), 1e-9, f"domain residual VJP {cfg} dL/dx", add_cd=False)
    if has_beta:
        dc.check_columns(gb, wb, sb, np.zeros_like(sb), 1e-9, f"domain residual VJP {cfg} dL/dbeta", add_cd=False)
    else:
        assert gb is None


# ---- offsets (SMPL+D) -----------------------------------------------------------------------------------------------------------
OFFSET_CASES = ("pi", "scale_20", "near", "mixed")


def test_offsets_forward_and_vjp(val):
    """the displaced forward and its VJP on four cases, |d| <= 0.05 m, against the checker's cloud + L d (offsets_ref.py)"""
    v, om, tabs = val
    full, mag, B = tabs[False]
    idx = [full.index[n] for n in OFFSET_CASES]
    x, beta, R0 = full.x[idx], full.beta[idx], full.R0[idx]
    F, V, m = len(idx), v.model.n_verts, v.model
    rng = np.random.default_rng(3)
    u = rng.normal(size=(F, V, 3))
    d = (u / np.linalg.norm(u, axis=2, keepdims=True) * rng.uniform(0.0, 0.05, size=(F, V, 1))).astype(np.float32)
    d[:, 5:8] = 0.0
    d[:, V - 1] = [0.03, -0.04, 0.0]                       # the tail tile's one vertex at the full 5 cm
    d64 = d.astype(np.float64)
    prob = _kp_free(_gm(v), F, R0, n_cols=86, use_shape=True, beta_per_frame=True)
    _, cd = _forward_device(prob, x, beta, d)
    L = offsets_ref.blend_matrices(m, x, R0)
    want = mag.cloud[idx] + offsets_ref.delta(L, d64)
    worst = 0.0
    for i, name in enumerate(OFFSET_CASES):
        # the undisplaced cloud's bound and the displacement's own (bodyfit.h, bodyfit_forward_offsets_device)
        bound = B[idx[i]] + U * (16.0 * abs(x[i, 0]) * np.abs(d64[i]).sum(1, keepdims=True) + np.abs(cd[i]))
        err = np.abs(cd[i] - want[i])
        assert (err <= bound).all(), (name, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    _report("offsets forward", worst)
    # the VJP: d (checker cloud + L d) / dx by central differences at t = 0, column by column
    G = rng.normal(size=(F, V, 3)).astype(np.float32)
    H = rng.normal(size=(F, 24, 3))
    gx, gb, go = prob.forward_vjp(x, beta, G, H, offsets=d)

    def jac(step):
        Jj, Jc = dc.dense_jacobian(om, x, beta, R0, step=step)
        for c in list(range(4)) + list(range(7, 76)):      # (neither the translation nor beta enters L)
            xp = x.copy(); xp[:, c] += step
            xm = x.copy(); xm[:, c] -= step
            Jc[:, c] += (offsets_ref.delta(offsets_ref.blend_matrices(m, xp, R0), d64) -
                         offsets_ref.delta(offsets_ref.blend_matrices(m, xm, R0), d64)) / (2 * step)
        return Jj, Jc

    g, S = _contract(G, H, *jac(1e-6))
    g2, _ = _contract(G, H, *jac(2e-6))
    _check_vjp("offsets VJP", gx, gb, g, S, np.abs(g - g2), False, dc.VJP_REL)
    wo = offsets_ref.grad_offsets(L, G, shared=False)
    bo = U * (16.0 * (np.abs(x[:, 0])[:, None] * np.abs(G.astype(np.float64)).sum(2))[..., None] + np.abs(go.astype(np.float64)))
    eo = np.abs(go.astype(np.float64) - wo)
    assert (eo <= bo).all(), float((eo / np.maximum(bo, 1e-300)).max())
    _report("offsets dL/dd", (eo / np.maximum(bo, 1e-300)).max())
