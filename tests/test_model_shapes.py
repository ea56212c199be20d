"""CPU suite: the checker at the model shapes the API accepts beyond SMPL's (tests/model_variants.py), and the shapes
bodyfit_model_create / bodyfit_problem_create reject before touching a device.

Each variant is first checked against the numpy forward (synth.forward_numpy), which shares nothing with the checker, so a
broken variant is not mistaken for a kernel bug by the GPU tests (test_gpu_model_shapes.py); then the checker's analytic
Jacobian against its dual-number autodiff and central differences, and the dense LM at n_cols = 76 + n_shape."""
import numpy as np
import pytest

import model_variants as mv

INTR = np.array([1728.0, 1728.0, 960.0, 540.0])


@pytest.fixture(scope="module")
def variants():
    return {i: mv.get(i) for i in mv.ALL}


def test_variants_have_the_advertised_shapes(variants):
    v = variants
    assert [v[f"ns{k}"].n_shape for k in (0, 1, 6, 9)] == [0, 1, 6, 9]
    assert [v[f"v{n}"].model.n_verts for n in (31, 33, 288, 289, 2049)] == [31, 33, 288, 289, 2049]
    assert [v[i].depth for i in ("deep13", "deep14", "chain23", "star")] == [13, 14, 23, 1]
    assert [v[f"nj{n}"].n_joints for n in (1, 2, 16, 23)] == [1, 2, 16, 23]
    for i, var in v.items():
        m = var.model
        nJ = m.n_joints
        assert m.weights.shape == (m.n_verts, nJ) and np.allclose(m.weights.sum(1), 1.0), i
        assert (np.count_nonzero(m.weights, 1) <= 4).all(), i         # the mesh path's limit
        assert m.posedirs.shape[2] == 9 * (nJ - 1) and m.j_regressor.shape == (nJ, m.n_verts), i
        assert m.S.shape == (3 * nJ, m.n_shape), i
        assert var.accepted == (var.depth <= mv.MAX_DEPTH)
    assert mv.ACCEPTED == mv.ids(lambda x: x.accepted)
    assert mv.MESH == mv.ids(lambda x: x.mesh_capable)


@pytest.mark.parametrize("vid", mv.ALL)
def test_checker_forward_equals_numpy_forward(oracle_mod, vid):
    v = mv.get(vid)
    om = mv.oracle_model(oracle_mod, v)
    rng = np.random.default_rng(7)
    F = 3
    x = mv.random_params(rng, v, F)
    beta = rng.normal(size=v.n_shape)
    R0 = np.tile(np.eye(3).reshape(1, 9), (F, 1))
    for use_shape in (True, False):
        joints, cloud = om.forward_batch(x, beta, R0, use_shape, v.pose_blend_data)
        for f in range(F):
            jn, cn = mv.synth.forward_numpy(v.model, x[f], beta, np.eye(3), v.pose_blend_data, use_shape=use_shape)
            assert np.abs(joints[f] - jn).max() < 1e-12, (vid, f)
            assert np.abs(cloud[f] - cn).max() < 1e-12, (vid, f)


@pytest.mark.parametrize("vid", mv.ALL)
def test_checker_jacobian_equals_autodiff_and_central_differences(oracle_mod, vid):
    v = mv.get(vid)
    om = mv.oracle_model(oracle_mod, v)
    rng = np.random.default_rng(11)
    x = mv.random_params(rng, v, 2)[1]
    xx = np.concatenate([x, rng.normal(size=v.n_shape)])
    R0 = -np.eye(3).reshape(-1)
    nJ, nL = v.n_joints, len(v.model.landmark_vid)
    kids = sorted({0, nJ - 1, nJ // 2, nJ, nJ + nL - 1})
    for use_shape in (True, False):
        for kid in kids:
            uv = rng.uniform(0, 1000, 2)
            ra, Ja = om.kp_block(kid, uv, INTR, R0, xx, use_shape, v.pose_blend_data, mode=0)
            rb, Jb = om.kp_block(kid, uv, INTR, R0, xx, use_shape, v.pose_blend_data, mode=1)
            assert np.abs(ra - rb).max() < 1e-9, (vid, kid)
            assert np.abs(Ja - Jb).max() < 1e-9 * max(1.0, np.abs(Jb).max()), (vid, kid)
            if not use_shape:
                assert np.all(Ja[:, v.npose:] == 0.0)
                continue
            fd = np.zeros_like(Ja)
            for c in range(len(xx)):
                h = 1e-6
                xp, xm = xx.copy(), xx.copy()
                xp[c] += h; xm[c] -= h
                rp, _ = om.kp_block(kid, uv, INTR, R0, xp, True, v.pose_blend_data, 0, want_jac=False)
                rm, _ = om.kp_block(kid, uv, INTR, R0, xm, True, v.pose_blend_data, 0, want_jac=False)
                fd[:, c] = (rp - rm) / (2 * h)
            assert np.abs(fd - Ja).max() < 1e-5 * max(1.0, np.abs(Ja).max()), (vid, kid)


@pytest.mark.parametrize("vid", ["ns0", "ns1", "ns6", "ns9", "nopd"])
def test_dense_lm_at_every_shape_width(oracle_mod, vid):
    """lm_dense.solve at n_cols = 76 + n_shape (and without pose correctives): from a perturbed start it runs, its
    Jacobian has the 76 F + n_shape columns, and the cost it reports is the cost of the rows at its answer (a tenth of the
    start cost or less)."""
    from oracle import lm_dense
    v = mv.get(vid)
    om = mv.oracle_model(oracle_mod, v)
    F = 2
    seq = mv.synth.make_sequence(v.model, F, seed=4, noise_px=0.5)
    rng = np.random.default_rng(2)
    x0 = seq.gt_params + 0.02 * rng.normal(size=seq.gt_params.shape)
    x0[:, 0] = 1.0
    b0 = np.zeros(v.n_shape)
    n_cols = 76 + v.n_shape
    x, b, info = lm_dense.solve(om, seq, x0, b0, n_cols=n_cols, use_shape=True, pose_blend=v.pose_blend_data,
                                beta_pose=1.0, beta_shape=1.0, lam=1.0, max_iters=100)
    assert x.shape == (F, 76) and np.asarray(b).shape == (v.n_shape,)
    cost0, _, _ = lm_dense._rows(om, seq, x0, b0, n_cols, True, v.pose_blend_data, 1.0, None, 1.0, 1.0, 3.0, False)
    cost1, _, J = lm_dense._rows(om, seq, x, np.asarray(b), n_cols, True, v.pose_blend_data, 1.0, None, 1.0, 1.0, 3.0, True)
    assert J.shape[1] == F * 76 + v.n_shape
    assert cost1 == pytest.approx(info["final_cost"], rel=1e-12) and cost1 < 0.1 * cost0, (cost0, cost1)


def _desc_error(api, m):
    with pytest.raises(api.BodyfitError) as e:
        api.Model(m)
    return str(e.value)


@pytest.mark.parametrize("vid", ["deep14", "chain23"])
def test_model_create_rejects_trees_deeper_than_the_ancestor_walk(api, vid):
    """bodyfit_model_create refuses a tree deeper than 13 levels before any device call (no GPU needed): the frame role's
    packed ancestor list holds 12 joints, a deeper chain was cut short without an error."""
    msg = _desc_error(api, mv.get(vid).model)
    assert msg.startswith("bodyfit status 1:"), msg   # BODYFIT_ERR_INVALID
    assert "deeper than 13" in msg, msg
