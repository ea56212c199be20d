"""CPU: the numpy restatement of the per-vertex offsets (offsets_ref.py) against the project's f64 checker by an independent
route, and the dense mesh Laplacian's own properties.

The route: synth.make_model's joint regressor has at most 24 x 64 non-zero columns.  Offsets that are zero on those vertices do
not move the regressed joints, so a checker model whose template is v_template + d has the same joints, transforms and pose /
shape blend, and its cloud is the undisplaced checker cloud + L d exactly (up to f64 rounding): SMPL+D without any offsets code
in the checker."""
import dataclasses

import numpy as np
import pytest

import offsets_ref
from conftest import random_params


def _free_vertices(model):
    return np.flatnonzero(np.abs(model.j_regressor).sum(axis=0) == 0.0)


@pytest.mark.parametrize("per_frame_offsets", [False, True], ids=["shared", "per_frame"])
@pytest.mark.parametrize("pose_blend", [True, False], ids=["blend", "noblend"])
def test_restatement_against_the_checker(oracle_mod, synth, model, omodel, per_frame_offsets, pose_blend):
    V = model.n_verts
    free = _free_vertices(model)
    assert len(free) >= V // 2, (len(free), V)
    rng = np.random.default_rng(3)
    F = 3
    x = random_params(rng, F)
    x[0, 10:13] = 0.0                                   # a joint at zero rotation, one at a tiny one
    x[1, 13:16] = [1e-9, -2e-9, 0.5e-9]
    beta = rng.normal(size=model.n_shape)
    R0 = np.stack([synth.rodrigues(rng.normal(size=3) * 0.3) for _ in range(F)])
    d = np.zeros((F if per_frame_offsets else 1, V, 3))
    d[:, free] = rng.uniform(-0.05, 0.05, size=(d.shape[0], len(free), 3))
    _, cloud0 = omodel.forward_batch(x, beta, R0.reshape(F, 9), True, pose_blend)
    L = offsets_ref.blend_matrices(model, x, R0)
    want = cloud0 + offsets_ref.delta(L, d if per_frame_offsets else d[0])
    for f in range(F):
        moved = dataclasses.replace(model, v_template=model.v_template + d[f if per_frame_offsets else 0]).finalize()
        assert np.array_equal(moved.J0, model.J0)       # the joints did not move
        om = oracle_mod.OracleModel(moved)
        joints, cloud = om.forward(x[f], beta, R0[f].reshape(9), True, pose_blend)
        err = np.abs(cloud - want[f]).max()
        assert err <= 1e-12, (f, err)
    # and the exact gradient is the transpose of delta: <G, L d> = <L^T G, d>
    G = rng.normal(size=(F, V, 3))
    g = offsets_ref.grad_offsets(L, G, shared=not per_frame_offsets)
    lhs = float((G * offsets_ref.delta(L, d if per_frame_offsets else d[0])).sum())
    rhs = float((g * (d if per_frame_offsets else d[0])).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_dense_laplacian_properties():
    V, faces = offsets_ref.mesh_with_boundary()
    L = offsets_ref.laplacian_dense(V, faces)
    held = np.zeros(V, bool)
    held[faces.ravel()] = True
    assert not held[V - 1] and held[:V - 1].all()
    # a constant field: 0 at every vertex with a face (each row sums to 1 - 2 n_i / (2 n_i)); the unreferenced row is zero
    assert np.abs(L @ np.ones(V)).max() <= 1e-15
    assert not L[V - 1].any() and not L[:, V - 1].any()
    # L^T as the header states it, (L^T r)_u = [n_u > 0] r_u - sum_{t holds u} sum_{other corners v} r_v / (2 n_v), gathered
    # per vertex over the faces' corner POSITIONS, is the transpose of the dense matrix
    count = np.zeros(V, np.int64)
    for t in faces:
        for i in set(t.tolist()):
            count[i] += 1
    r = np.random.default_rng(0).normal(size=(V, 3))
    out = np.where(count[:, None] > 0, r, 0.0)
    for t in faces.tolist():
        for c, u in enumerate(t):
            for q, v in enumerate(t):
                if q != c and t.index(v) == q:              # v's row reads position c (not its own first position)
                    out[u] -= r[v] / (2.0 * count[v])
    assert np.abs(out - L.T @ r).max() <= 1e-14
    # an interior vertex of the regular sheet: itself minus the mean over its faces' other corners
    i = 3 * 7 + 3
    x = np.random.default_rng(1).normal(size=(V, 3))
    acc = np.zeros(3); n = 0
    for t in faces.tolist():
        if i in t:
            acc += sum(x[v] for v in t if v != i); n += 1
    assert np.abs((L @ x)[i] - (x[i] - acc / (2 * n))).max() <= 1e-14
