"""CPU: the reference holds on the table of tests/domain_cases.py before any kernel is compared with it, the arithmetic
model's error E_f per case, and proof that the bounds of tests/test_gpu_domain.py reject wrong arithmetic (the mutants).

The checker has only ever been validated on the suite's one distribution; here, on every case: its forward, residuals and
dual-number Jacobian are finite, its forward agrees with an implementation on scipy's rotations, its Jacobian with central
differences of its own residuals.  Nothing here touches the library."""
import re

import numpy as np
import pytest

import domain_cases as dc
import model_variants as mv

synth = mv.synth
INTR = synth.camera_intrinsics()


@pytest.fixture(scope="module")
def dom(oracle_mod):
    """the table on the value model (v2049), per-frame and shared beta, with the checker's forward and magnitudes"""
    v = mv.get("v2049")
    om = mv.oracle_model(oracle_mod, v)
    out = {}
    for shared in (False, True):
        tab = dc.cases(v, 0, shared_beta=shared, om=om)
        out[shared] = (tab, dc.magnitudes(om, v, tab))
    return v, om, out


@pytest.fixture(scope="module")
def dom_small(oracle_mod):
    """the table on the derivative model (v289) with its central-difference Jacobians at steps 1e-6 and 2e-6 and the fourth-order
    one of the joints"""
    v = mv.get("v289")
    om = mv.oracle_model(oracle_mod, v)
    tab = dc.cases(v, 0, om=om)
    J1 = dc.dense_jacobian(om, tab.x, tab.beta, tab.R0, step=1e-6)
    J2 = dc.dense_jacobian(om, tab.x, tab.beta, tab.R0, step=2e-6)
    Jj4 = dc.joint_jacobian_o4(om, tab.x, tab.beta, tab.R0)
    return v, om, tab, J1, J2, Jj4


def _obs_all_joints(tab, f):
    """frame f alone with the FK joints 1..23 as keypoints (the root keypoint follows a rule of its own)"""
    return mv.SimpleNamespace(kp_offset=np.array([0, 23], np.int32), kp_id=np.arange(1, 24, dtype=np.int32),
                              kp_uv=np.zeros((23, 2)), intr=INTR, R0=tab.R0[f:f + 1])


# ---- an independent forward: rotations from a caller's function ------------------------------------------------------------
def _scipy_rot(a):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(a).as_matrix()


def fk(model, Rl, x, beta, R0, Rroot):
    """posed joints [24, 3] from the joints' rotations Rl [24] (Rl[0] unused): multilinear in them"""
    nJ = model.n_joints
    Jb = model.J0 + (model.S @ beta).reshape(nJ, 3)
    A = [np.eye(3)] * nJ
    P = np.zeros((nJ, 3))
    for j in range(1, nJ):
        p = model.parent[j]
        A[j] = A[p] @ Rl[j]
        P[j] = P[p] + A[p] @ (Jb[j] - Jb[p])
    M = x[0] * Rroot @ np.asarray(R0).reshape(3, 3)
    return P @ M.T + x[4:7], A, P, Jb, M


def forward_rot(model, x, beta, R0, rot):
    """joints and cloud of one frame, every rotation from rot(a)"""
    nJ = model.n_joints
    Rl = [np.eye(3)] + [rot(x[7 + 3 * (j - 1):10 + 3 * (j - 1)]) for j in range(1, nJ)]
    joints, A, P, Jb, M = fk(model, Rl, x, beta, R0, rot(x[1:4]))
    feat = np.array([R - np.eye(3) for R in Rl[1:]]).reshape(-1)
    vp = model.v_template - Jb[0] + model.shapedirs @ beta + model.posedirs @ feat
    Jc = Jb - Jb[0]
    out = np.zeros_like(vp)
    for j in range(nJ):
        out += model.weights[:, j:j + 1] * ((vp - Jc[j]) @ A[j].T + P[j])
    return joints, out @ M.T + x[4:7]


def joint_jacobian(model, x, beta, R0, rot_grad):
    """d joints [24, 3] / d joint angles [69] with (R, dR [3]) = rot_grad(a) for every joint: the joints are affine in each
    R_k, so the derivative along a_kc is fk(R_k -> dR_kc) - fk(R_k -> 0), exactly"""
    nJ = model.n_joints
    RdR = [None] + [rot_grad(x[7 + 3 * (j - 1):10 + 3 * (j - 1)]) for j in range(1, nJ)]
    Rl = [np.eye(3)] + [r[0] for r in RdR[1:]]
    Rroot = rot_grad(x[1:4])[0]
    out = np.zeros((nJ, 3, 3 * (nJ - 1)))
    for k in range(1, nJ):
        Rz = list(Rl); Rz[k] = np.zeros((3, 3))
        base = fk(model, Rz, x, beta, R0, Rroot)[0]
        for c in range(3):
            Rd = list(Rl); Rd[k] = RdR[k][1][c]
            out[:, :, 3 * (k - 1) + c] = fk(model, Rd, x, beta, R0, Rroot)[0] - base
    return out


def _project_jacobian(joints, dJ):
    """d (u, v) of joints 1..23 / d the columns of dJ: [46, n]"""
    fx, fy = INTR[0], INTR[1]
    X, Y, Z = joints[1:, 0:1], joints[1:, 1:2], joints[1:, 2:3]
    du = fx * (dJ[1:, 0] / Z - X * dJ[1:, 2] / Z ** 2)
    dv = fy * (dJ[1:, 1] / Z - Y * dJ[1:, 2] / Z ** 2)
    return np.stack([du, dv], axis=1).reshape(46, -1)


# ---- the reference on the table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_checker_is_finite_and_the_depths_are_as_named(dom, shared):
    v, om, tabs = dom
    tab, mag = tabs[shared]
    assert len(tab.names) == (26 if shared else 29) and len(set(tab.names)) == len(tab.names)
    assert np.isfinite(mag.joints).all() and np.isfinite(mag.cloud).all() and np.isfinite(mag.P).all()
    i = tab.index["near"]
    assert abs(mag.zmin[i] - dc.NEAR_Z) < 1e-12
    for f, name in enumerate(tab.names):
        if name == "behind":
            assert mag.joints[f, :, 2].max() < 0 and mag.cloud[f, :, 2].max() < 0
        else:
            assert mag.zmin[f] >= dc.NEAR_Z - 1e-12, (name, mag.zmin[f])
    obs = dc.observations(v, tab)
    assert (np.diff(obs.kp_offset) == 0).sum() == 1
    for mode in (0, 1):     # analytic and dual-number (Jet) Jacobian
        r, J = om.evaluate_batch(obs, tab.x, tab.beta, 86, True, True, mode=mode)
        assert np.isfinite(r).all() and np.isfinite(J).all()
    # what the names promise, bit for bit
    x = tab.x
    assert not x[tab.index["rest"], 7:].any()
    knee = x[tab.index["one_knee_pi_x"], 7:].reshape(23, 3)
    assert knee[dc.KNEE - 1].tolist() == [np.pi, 0.0, 0.0] and np.count_nonzero(knee) == 1
    assert ((x[tab.index["axis_aligned"], 7:].reshape(23, 3) == 0.0).sum(1) == 2).all()
    th = np.linalg.norm(x[:, 7:].reshape(len(x), 23, 3), axis=2)
    for name, want in (("tiny_1e-8", 1e-8), ("tiny_1e-7", 1e-7), ("pi", np.pi), ("pi_plus", np.pi + 1e-6), ("two_pi", 2 * np.pi), ("theta_7.5", 7.5)):
        assert np.abs(th[tab.index[name]] - want).max() < 4e-16 * max(want, 1.0)
    assert np.array_equal(x[tab.index["control_empty"]], x[tab.index["control"]])


@pytest.mark.parametrize("shared", [False, True])
def test_checker_matches_scipy_rotations_on_every_case(dom, shared):
    """test_oracle.py's tolerances (joints 1e-13, cloud 1e-12, reprojection 1e-10), relative to M_f and P_f"""
    v, om, tabs = dom
    tab, mag = tabs[shared]
    F = len(tab.names)
    beta = np.broadcast_to(tab.beta, (F, v.n_shape))
    obs = dc.observations(v, tab)
    r, _ = om.evaluate_batch(obs, tab.x, tab.beta, 86, True, True, mode=0, want_jac=False)
    for f, name in enumerate(tab.names):
        j, c = forward_rot(v.model, tab.x[f], beta[f], tab.R0[f], _scipy_rot)
        m = max(1.0, mag.M[f])
        assert np.abs(j - mag.joints[f]).max() < 1e-13 * m, name
        assert np.abs(c - mag.cloud[f]).max() < 1e-12 * m, name
        pts = np.concatenate([j, c[v.model.landmark_vid]])
        k0, k1 = obs.kp_offset[f], obs.kp_offset[f + 1]
        kid = obs.kp_id[k0:k1]
        keep = kid != 0                     # (the root keypoint carries S_0 beta without a parent term: test_oracle.py)
        uv = synth.project(pts[kid], INTR) - obs.kp_uv[k0:k1]
        err = np.abs(uv - r[2 * k0:2 * k1].reshape(-1, 2))[keep]
        assert err.size == 0 or err.max() < 1e-10 * max(1.0, mag.P[f]), (name, err.max())


def test_jet_jacobian_matches_central_differences_on_every_case(dom):
    """test_oracle.py's 2e-5 of the largest entry, per frame"""
    v, om, tabs = dom
    tab, mag = tabs[False]
    obs = dc.observations(v, tab)
    _, J = om.evaluate_batch(obs, tab.x, tab.beta, 86, True, True, mode=1)
    h = 1e-6
    fd = np.zeros_like(J)
    for c in range(86):
        xp, xm, bp, bm = tab.x.copy(), tab.x.copy(), tab.beta.copy(), tab.beta.copy()
        if c < 76:
            xp[:, c] += h; xm[:, c] -= h
        else:
            bp[:, c - 76] += h; bm[:, c - 76] -= h
        rp, _ = om.evaluate_batch(obs, xp, bp, 86, True, True, mode=0, want_jac=False)
        rm, _ = om.evaluate_batch(obs, xm, bm, 86, True, True, mode=0, want_jac=False)
        fd[:, c] = (rp - rm) / (2 * h)
    for f, name in enumerate(tab.names):
        a, e = 2 * obs.kp_offset[f], 2 * obs.kp_offset[f + 1]
        if e > a:
            assert np.abs(fd[a:e] - J[a:e]).max() < 2e-5 * max(1.0, np.abs(J[a:e]).max()), name


# ---- the arithmetic model --------------------------------------------------------------------------------------------------
def _committed_table():
    rows = re.findall(r"^  (\S+)\s+([0-9.]+e[-+][0-9]+)$", dc.__doc__, flags=re.M)
    return {n: float(e) for n, e in rows}


def test_arithmetic_model_error_table(dom):
    """E_f per case: printed, and the figures in domain_cases' docstring (and DESIGN.md) are these up to the math library"""
    v, om, tabs = dom
    tab, mag = tabs[False]
    E = dc.model_errors(v, tab, mag.cloud)
    B = dc.cloud_bounds(tab, E)
    committed = _committed_table()
    print("\ncase             E_f [m]     B_f [m]     M_f [m]   max T_fv [m]")
    for f, name in enumerate(tab.names):
        print(f"  {name:14s} {E[f]:.3e}  {B[f]:.3e}  {mag.M[f]:8.2f}  {mag.T[f].max():.3f}")
    assert set(committed) == set(tab.names)
    for f, name in enumerate(tab.names):
        assert 0.5 * committed[name] <= E[f] <= 2.0 * committed[name], (name, E[f], committed[name])
        # the model is the stated arithmetic and nothing worse: the split's a-priori 3.02 x 2^-16 of the blend's terms
        # (bodyfit.h, the Gram's derivation) through the scale, and the f32 roundings of a 4 x 4-term transform
        apriori = abs(tab.x[f, 0]) * 3.02 * 2.0 ** -16 * (mag.T[f].max() + 2.0 ** -8) + 16 * 2.0 ** -24 * mag.M[f]
        assert E[f] <= apriori, (name, E[f], apriori)
    assert B[tab.index["control"]] <= 5e-6 and B[tab.index["rest"]] <= 5e-6


# ---- teeth ------------------------------------------------------------------------------------------------------------------
def test_mutant_a_dropped_lo_hi_product_exceeds_the_cloud_bound(dom):
    v, om, tabs = dom
    tab, mag = tabs[False]
    B = dc.cloud_bounds(tab, dc.model_errors(v, tab, mag.cloud))
    Em = dc.model_errors(v, tab, mag.cloud, drop_lo_hi=True)
    caught = [n for f, n in enumerate(tab.names) if Em[f] > B[f]]
    f = tab.index["pi"]
    print(f"\nmutant (a): error {Em[f]:.3e} m against B = {B[f]:.3e} m at pi ({Em[f] / B[f]:.0f} x); rejected in {caught}")
    assert Em[f] > B[f]
    assert {"control", "half_pi", "pi", "sigma_1", "scale_20", "near", "mixed"} <= set(caught)


def _rot_grad(oracle_mod):
    return lambda a: oracle_mod.rodrigues(a)


def _first_order_below(oracle_mod, th2_max):
    def rot_grad(a):
        if a @ a <= th2_max:
            K = lambda w: np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
            return np.eye(3) + K(a), np.array([K(e) for e in np.eye(3)])
        return oracle_mod.rodrigues(a)
    return rot_grad


def _wrapped(oracle_mod):
    """theta wrapped into [0, pi] by negating the axis: the same rotation, dR taken at the wrapped vector"""
    def rot_grad(a):
        th = np.linalg.norm(a)
        if th <= np.pi:
            return oracle_mod.rodrigues(a)
        phi = th % (2 * np.pi)
        w = a / th
        return oracle_mod.rodrigues(phi * w if phi <= np.pi else -(2 * np.pi - phi) * w)
    return rot_grad


def test_mutant_b_wide_first_order_branch_exceeds_the_jacobian_bound(dom, oracle_mod):
    """Rodrigues' first-order branch taken for theta^2 <= 1e-12 instead of DBL_EPSILON, against the f64 bound on J
    (1e-9 max(1, max |J_ref|) per frame) at tiny_1e-7; the true rotation passes it on every case."""
    v, om, tabs = dom
    tab, mag = tabs[False]
    for f, name in enumerate(tab.names):
        _, Jref = om.evaluate_batch(_obs_all_joints(tab, f), tab.x[f:f + 1], tab.beta[f], 86, True, True, mode=0)
        bound = 1e-9 * max(1.0, np.abs(Jref).max())
        good = _project_jacobian(mag.joints[f], joint_jacobian(v.model, tab.x[f], tab.beta[f], tab.R0[f], _rot_grad(oracle_mod)))
        assert np.abs(good - Jref[:, 7:76]).max() <= bound, name
        if name == "tiny_1e-7":
            bad = _project_jacobian(mag.joints[f], joint_jacobian(v.model, tab.x[f], tab.beta[f], tab.R0[f],
                                                                  _first_order_below(oracle_mod, 1e-12)))
            err = np.abs(bad - Jref[:, 7:76]).max()
            print(f"\nmutant (b): J error {err:.3e} against the bound {bound:.3e} at tiny_1e-7 ({err / bound:.0f} x)")
            assert err > bound


def test_mutant_c_wrapped_angle_exceeds_the_jvp_joint_bound(dom_small, oracle_mod):
    """theta wrapped into [0, pi]: against the JVP's joint bound (1e-7 of the column's largest entry, the reference by
    fourth-order differences of the checker) at pi_plus and theta_7.5; the unwrapped derivative passes it on every case."""
    v, om, tab, _, _, Jj = dom_small
    slack = dc.first_order_slack(om, tab.x, tab.beta, tab.R0, None)     # tiny_1e-8: dR_c = [e_c]x is 2 theta off, by design
    assert slack[tab.index["tiny_1e-8"], 7:].min() > 0 and not np.delete(slack, tab.index["tiny_1e-8"], 0).any()
    for f, name in enumerate(tab.names):
        ref = Jj[f, 7:76].transpose(1, 2, 0)                      # [24, 3, 69]
        scale = np.abs(ref).reshape(-1, 69).max(0)
        good = joint_jacobian(v.model, tab.x[f], tab.beta[f], tab.R0[f], _rot_grad(oracle_mod))
        assert (np.abs(good - ref).reshape(-1, 69).max(0) <= 1e-7 * scale + slack[f, 7:]).all(), name
        if name in ("pi_plus", "theta_7.5"):
            bad = joint_jacobian(v.model, tab.x[f], tab.beta[f], tab.R0[f], _wrapped(oracle_mod))
            err = np.abs(bad - ref).reshape(-1, 69).max(0)
            moving = scale > 0
            worst = float((err[moving] / scale[moving]).max())
            print(f"\nmutant (c): worst column error {worst:.3e} of the column's largest entry at {name} (bound 1e-7)")
            assert (err[moving] > 1e-7 * scale[moving]).all()
            assert np.abs(_wrapped(oracle_mod)(tab.x[f, 7:10])[0] - oracle_mod.rodrigues(tab.x[f, 7:10])[0]).max() < 1e-14


def test_mutant_d_wrong_distal_columns_exceed_the_column_bound_and_pass_the_row_bound(dom_small):
    """A VJP reference with distal columns wrong, under the row-maximum check (1e-4 of the frame's largest entry) and under the
    per-column bound 2^-14 S_fc + CD_fc.  Random G (f32) and H as in test_gpu_forward_vjp.py, every frame of the table.
    What the numbers say: the row-maximum check accepts a zero in every column below 1e-4 of its row's maximum and a 10 % error
    in every column below 1e-3 of it (114 of the 2,001 joint columns, two thirds of them the leaves'); the per-column bound rejects both
    wherever the column is not also small against its own scale S_fc (a sum that cancels).  With all THREE columns of a hand
    or foot set to 0 at once the row-maximum check does reject on this table -- the largest of a leaf's three columns is never
    below 1.5e-4 of the row's maximum -- so the gap is a leaf's columns being wrong by a fraction, or one of them being lost;
    the per-column bound rejects the three zeros too, in every frame."""
    v, om, tab, (J1j, J1c), (J2j, J2c), _ = dom_small
    F = len(tab.names)
    rng = np.random.default_rng(F)
    G = rng.normal(size=(F, v.model.n_verts, 3)).astype(np.float32).astype(np.float64)
    H = rng.normal(size=(F, 24, 3))
    g = np.einsum("fvc,fkvc->fk", G, J1c) + np.einsum("fjc,fkjc->fk", H, J1j)
    g2 = np.einsum("fvc,fkvc->fk", G, J2c) + np.einsum("fjc,fkjc->fk", H, J2j)
    S = np.einsum("fvc,fkvc->fk", np.abs(G), np.abs(J1c)) + np.einsum("fjc,fkjc->fk", np.abs(H), np.abs(J1j))
    CD = np.abs(g - g2)
    ratio, ref_ok = dc.column_ratios(g, g, S, CD)
    assert ref_ok and ratio.max() == 0.0 and dc.row_max_ok(g, g)
    g, S, CD = g[:, :76], S[:, :76], CD[:, :76]
    row = np.abs(g).max(1, keepdims=True)
    joint_cols = np.arange(76) >= 7
    # (1) the literal mutant: a leaf's three columns set to 0
    n_leaf_ok, smallest = 0, 1.0
    for f in range(F):
        for j in (22, 23, 10, 11):                              # hands and feet
            cols = slice(7 + 3 * (j - 1), 10 + 3 * (j - 1))
            smallest = min(smallest, np.abs(g[f, cols]).max() / row[f, 0])
            zero = g[f].copy(); zero[cols] = 0.0
            assert (dc.column_ratios(zero, g[f], S[f], CD[f])[0][cols] > 1.0).any(), (tab.names[f], j)
            n_leaf_ok += dc.row_max_ok(zero, g[f])
    # (2) every column below 1e-4 of its row's maximum set to 0, (3) every column below 1e-3 of it 10 % wrong
    lost = joint_cols & (np.abs(g) <= 1e-4 * row)
    tenth = joint_cols & (np.abs(g) <= 1e-3 * row)
    m_lost = np.where(lost, 0.0, g)
    m_tenth = np.where(tenth, 0.9 * g, g)
    assert dc.row_max_ok(m_lost, g) and dc.row_max_ok(m_tenth, g)          # the gap: accepted, in every frame
    r_lost = dc.column_ratios(m_lost, g, S, CD)[0]
    r_tenth = dc.column_ratios(m_tenth, g, S, CD)[0]
    leaves = np.zeros(76, bool)
    for j in (22, 23, 10, 11, 15, 20, 21, 7, 8):                # hands, feet, head, wrists, ankles
        leaves[7 + 3 * (j - 1):10 + 3 * (j - 1)] = True
    print(f"\nmutant (d): the row-maximum check accepts {n_leaf_ok} of {4 * F} leaves with three zeroed columns (smallest leaf / "
          f"row maximum {smallest:.2e}); it accepts {int(lost.sum())} columns set to 0 and {int(tenth.sum())} columns 10 % wrong "
          f"({int((tenth & leaves).sum())} of them of hands, feet, head, wrists, ankles; {int(tenth.any(1).sum())} of {F} frames); the "
          f"per-column bound rejects {int((r_lost > 1).sum())} and {int((r_tenth > 1).sum())} of those, in "
          f"{int((r_tenth > 1).any(1).sum())} frames")
    assert tenth.any(1).sum() >= F // 2 and (r_tenth > 1).sum() >= tenth.sum() // 2
    assert (r_lost > 1).sum() >= 1
