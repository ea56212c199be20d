"""CPU: the references of the closest-surface search (tests/surface_ref.py) checked on their own, before any GPU test relies on
them: the f64 brute force by the KKT condition of the projection and a dense barycentric sampling, all seven Voronoi regions and
the degenerate faces by construction, the f32 restatement of the kernel's arithmetic inside the derived bound on every input
set the GPU tests use, and the envelope property (the analytic VJP at a frozen (index, bary) equals central differences of the
f64 squared distance)."""
import numpy as np
import pytest

import surface_ref as sr


def _kkt(q, verts, faces, index, bary, tol_scale=1e-9):
    """(p - c) . (v_i - c) <= tol for every corner v_i of the returned triangle: c is the projection of p onto that triangle"""
    c = sr.point_at(verts, faces, index, bary)
    P = q.astype(np.float64)
    tri = verts.astype(np.float64)[faces[index]]
    h = sr.longest_edge(verts, faces, index)
    d = np.sqrt(((P - c) ** 2).sum(axis=1))
    for i in range(3):
        s = ((P - c) * (tri[:, i] - c)).sum(axis=1)
        assert np.all(s <= tol_scale * (d + h) * (h + 1e-30) + 1e-300), (i, float(s.max()))


def test_reference_satisfies_kkt_and_beats_a_dense_sampling(synth):
    q, verts, faces = sr.mesh_scene(synth, 1, V=200, n_faces=60, n_query=80)
    d2, ix, b = sr.brute_force(q, verts, faces)
    assert np.all(b >= 0) and np.allclose(b.sum(axis=1), 1.0, atol=1e-12)
    _kkt(q, verts, faces, ix, b)
    # global optimality: no point of a dense barycentric lattice of ANY face is closer
    n = 24
    ij = np.array([(i, j) for i in range(n + 1) for j in range(n + 1 - i)], np.float64) / n
    lat = np.stack([1 - ij.sum(axis=1), ij[:, 0], ij[:, 1]], axis=1)                  # [m, 3]
    pts = np.einsum("ma,fac->fmc", lat, verts.astype(np.float64)[faces]).reshape(-1, 3)
    for i in range(len(q)):
        dd = ((pts - q[i].astype(np.float64)) ** 2).sum(axis=1).min()
        assert d2[i] <= dd * (1 + 1e-12) + 1e-30, (i, d2[i], dd)


def test_all_seven_regions_by_construction():
    q, verts, faces, want = sr.region_scene()
    assert set(want.tolist()) == set(range(7))
    d2, ix, b = sr.brute_force(q, verts, faces)
    _kkt(q, verts, faces, ix, b)
    eps = 1e-9
    zero = b <= eps
    got = np.full(len(q), -1)
    got[(~zero).all(axis=1)] = 0
    for i in range(3):
        edge = ~zero[:, i] & ~zero[:, (i + 1) % 3] & zero[:, (i + 2) % 3]
        got[edge] = 1 + i
        got[~zero[:, i] & zero[:, (i + 1) % 3] & zero[:, (i + 2) % 3]] = 4 + i
    on_vertex_or_edge = d2 < 1e-16              # (exactly on a corner or an edge: the region is the construction's by definition)
    assert np.array_equal(got[~on_vertex_or_edge], want[~on_vertex_or_edge]), (got, want)
    assert on_vertex_or_edge.sum() >= 4
    # the f32 form reaches the same regions and stays inside the bound
    f2, fi, fb = sr.kernel_form_f32(q, verts, faces)
    sr.check_bounds(q, verts, faces, f2, fi, fb, ref=(d2, ix, b))
    # (a query exactly on a corner: zero up to the bound, which check_bounds has asserted; the corner's weight is 1 to 2^-22)
    assert np.all(fb[-4:-1].max(axis=1) >= 1 - 2.0 ** -22)


def test_degenerate_faces_point_segment_collinear():
    q, verts, faces = sr.degenerate_scene()
    d2, ix, b = sr.brute_force(q, verts, faces)
    assert np.all(np.isfinite(d2)) and np.all(np.isfinite(b))
    _kkt(q, verts, faces, ix, b, tol_scale=1e-7)
    # each degenerate face alone: the distance is that of the segment / point it collapses to
    V = verts.astype(np.float64); P = q.astype(np.float64)
    d_pt, _, _ = sr.brute_force(q, verts, faces[0:1])
    np.testing.assert_allclose(d_pt, ((P - V[5]) ** 2).sum(axis=1), rtol=1e-12)
    d_seg, _, _ = sr.brute_force(q, verts, faces[2:3])
    _, want = sr._segment(V[5], V[6] - V[5], P)
    np.testing.assert_allclose(d_seg, want, rtol=1e-12, atol=1e-30)
    d_col, _, _ = sr.brute_force(q, verts, faces[3:4])
    _, want = sr._segment(V[0], V[2] - V[0], P)
    np.testing.assert_allclose(d_col, want, rtol=1e-12, atol=1e-30)
    for sub in (faces, faces[0:1], faces[1:2], faces[2:3], faces[3:5], faces[5:6], faces[6:7], faces[9:10]):
        f2, fi, fb = sr.kernel_form_f32(q, verts, sub)
        assert np.all(np.isfinite(f2)) and np.all(np.isfinite(fb))
        sr.check_bounds(q, verts, sub, f2, fi, fb)


@pytest.mark.parametrize("seed,V,nf,nq", [(0, 1000, 2000, 600), (1, 1000, 257, 300), (2, 1000, 33, 300), (3, 1000, 1, 100)])
def test_f32_form_meets_the_derived_bound_on_the_gpu_tests_inputs(synth, seed, V, nf, nq):
    q, verts, faces = sr.mesh_scene(synth, seed, V=V, n_faces=nf, n_query=nq)
    f2, fi, fb = sr.kernel_form_f32(q, verts, faces)
    opt, con = sr.check_bounds(q, verts, faces, f2, fi, fb)
    print(f"surface f32 form nf={nf}: optimality excess {opt:.1f} u (d + h), consistency {con:.1f} u (d + h); bound {sr.K}")
    assert sr.K <= 64


def test_f32_form_far_from_the_origin_keeps_its_digits(synth):
    """the same scene moved from 3 m to 30 m: local coordinates, so the bound in local scale still holds"""
    q, verts, faces = sr.mesh_scene(synth, 4, V=300, n_faces=500, n_query=200)
    shift = np.array([10.0, -20.0, 27.0], np.float32)
    q2, v2 = (q + shift).astype(np.float32), (verts + shift).astype(np.float32)
    sr.check_bounds(q2, v2, faces, *sr.kernel_form_f32(q2, v2, faces))


def test_nonfinite_rule_of_the_f32_form(synth):
    q, verts, faces = sr.mesh_scene(synth, 5, V=200, n_faces=100, n_query=50)
    q = q.copy(); verts = verts.copy()
    q[3] = np.nan; q[5, 1] = np.inf
    verts[faces[17, 0]] = np.nan
    f2, fi, fb = sr.kernel_form_f32(q, verts, faces)
    assert fi[3] == -1 and fi[5] == -1 and np.isposinf(f2[3]) and np.all(fb[[3, 5]] == 0)
    hit = np.isin(faces, faces[17, 0]).any(axis=1)
    assert not np.isin(fi, np.flatnonzero(hit)).any()
    f2, fi, fb = sr.kernel_form_f32(q, verts, faces[:0])
    assert np.all(fi == -1) and np.all(np.isposinf(f2)) and np.all(fb == 0)


def test_envelope_property_vjp_equals_finite_differences(synth):
    """d/dp and d/dcorner of the f64 reference's d^2 (the minimisation re-run at every step) against the analytic VJP at the
    frozen (index, bary), over all regions; queries whose region is stable under the step"""
    rng = np.random.default_rng(7)
    q, verts, faces, want = sr.region_scene()
    keep = np.flatnonzero(sr.brute_force(q, verts, faces)[0] > 1e-6)           # off the surface: d^2 is smooth there
    q = q[keep]
    d2, ix, b = sr.brute_force(q, verts, faces)
    g = rng.normal(size=len(q))
    gq, gv, _, _, _, _ = sr.vjp(q, verts, faces, ix, b, g)
    h = 1e-6
    P, V = q.astype(np.float64), verts.astype(np.float64)

    def cost(P_, V_):
        return sr.tri_closest64(P_, V_[0], V_[1], V_[2])[0]

    for c in range(3):
        dP = np.zeros(3); dP[c] = h
        fd = (cost(P + dP, V) - cost(P - dP, V)) / (2 * h)
        np.testing.assert_allclose(g * fd, gq[:, c], rtol=2e-5, atol=1e-9)
        for v in range(3):
            Vp, Vm = V.copy(), V.copy()
            Vp[v, c] += h; Vm[v, c] -= h
            fd = (g * (cost(P, Vp) - cost(P, Vm)) / (2 * h)).sum()
            np.testing.assert_allclose(fd, gv[v, c], rtol=2e-5, atol=1e-8)
