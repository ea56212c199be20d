"""CPU: the definition of the mesh winding number and of the contract of bodyfit_surface_winding_device (include/bodyfit.h), on the
numpy references of tests/winding_ref.py: the closed-mesh integer property, the k + cone identity of the vertex query and the
threshold-free classification w > 1, the f32 restatement of the kernel's arithmetic inside the bound B_i at every query, and the
CONDITION bound64 < 0.05 at every query of every named scene (the classification keeps 0.41 from the threshold, so no vertex may
go unclassified by rounding).  The figure of the kernel's arctangent polynomial that the derivation of k_s uses is checked here."""
import re

import numpy as np
import pytest

import winding_ref as wr


@pytest.fixture(scope="module", autouse=True)
def header_contract(api):
    """the constants every test here uses are the ones include/bodyfit.h states beside bodyfit_surface_winding_device"""
    assert "bodyfit_surface_winding_device" in api.declared_symbols() and "bodyfit_surface_vertex_normals_device" in api.declared_symbols()
    text = open(api.HEADER_PATH).read()
    doc = text[text.index("The WINDING NUMBER"):text.index("int bodyfit_surface_winding_device")]
    k, k_s = re.search(r"k = (\d+), k_s = (\d+)\.", doc).groups()
    assert (int(k), int(k_s)) == (wr.K, wr.K_S)
    assert f"within {wr.P_TRUNC} of atan" in doc


@pytest.fixture(scope="module", params=[2, 3], ids=["324v", "1284v"])
def scene(request):
    """the two-sphere scene with its f64 vertex winding, bound and f32 restatement (computed once, never written)"""
    verts, faces, nA = wr.two_spheres(request.param)
    ids = np.arange(len(verts))
    return dict(verts=verts, faces=faces, nA=nA, truth=wr.two_spheres_truth(verts, nA), w=wr.winding64(verts, verts, faces, ids),
                B=wr.bound64(verts, verts, faces, ids), w32=wr.kernel_form_f32(verts, verts, faces, ids))


def test_the_polynomial_is_within_its_stated_share_of_k_s():
    x = np.linspace(-wr.ATAN_REDUCED, wr.ATAN_REDUCED, 400001)
    err = np.abs(wr.atan_poly(x) - np.arctan(x)).max() / wr.U
    print(f"atan polynomial on |x| <= {wr.ATAN_REDUCED}: {err:.4f} u (stated {wr.P_TRUNC})")
    assert err <= wr.P_TRUNC
    assert np.float32(wr.ATAN_SPLIT) >= np.tan(np.pi / 8) and wr.ATAN_REDUCED >= float(np.float32(wr.ATAN_SPLIT)) * (1 + 4 * wr.U)


def test_atan2_restatement_against_numpy():
    rng = np.random.default_rng(0)
    y, x = (rng.normal(size=20000) * 10.0 ** rng.uniform(-6, 6, 20000)).astype(np.float32), rng.normal(size=20000).astype(np.float32)
    y[:8] = [0, 0, 1, -1, 0, -0.0, 1, -1]; x[:8] = [0, 1, 0, 0, -1, -1, 1, -1]
    got = wr.atan2_f32(y, x)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    want[0] = 0.0
    assert np.abs(got - want).max() <= 10.1 * wr.U      # the derivation's count for the arctangent alone
    assert got[0] == 0 and got[1] == 0


@pytest.mark.parametrize("mesh", ["icosphere", "uv_sphere", "two_spheres"])
def test_closed_mesh_winding_is_an_integer(mesh):
    rng = np.random.default_rng(1)
    q = np.concatenate([rng.normal(size=(150, 3)) * 0.5, rng.normal(size=(150, 3)) * 1.5 + [0.6, 0, 0]]).astype(np.float32)
    if mesh == "icosphere":
        verts, faces = wr.icosphere(2)
        want = (np.linalg.norm(q, axis=1) < 0.9).astype(int)
        sure = np.abs(np.linalg.norm(q, axis=1) - 0.95) > 0.06
    elif mesh == "uv_sphere":
        verts, faces = wr.uv_sphere(12, 9)
        want = (np.linalg.norm(q, axis=1) < 0.8).astype(int)
        sure = np.abs(np.linalg.norm(q, axis=1) - 0.9) > 0.11
    else:
        verts, faces, _ = wr.two_spheres(2)
        ra, rb = np.linalg.norm(q, axis=1), np.linalg.norm(q - np.asarray(wr.B_CENTER, np.float32), axis=1)
        want = (ra < 0.95).astype(int) + (rb < 0.66).astype(int)
        sure = (np.abs(ra - 0.975) > 0.03) & (np.abs(rb - 0.68) > 0.025)
    w = wr.winding64(q, verts, faces)
    assert np.abs(w - np.round(w)).max() < 1e-12
    assert sure.sum() > 200 and np.array_equal(np.round(w[sure]).astype(int), want[sure])
    assert set(np.round(w).astype(int)) >= ({0, 1, 2} if mesh == "two_spheres" else {0, 1})
    B = wr.bound64(q, verts, faces)
    assert B.max() < 0.05
    assert np.all(np.abs(wr.kernel_form_f32(q, verts, faces) - w) <= B)
    # flipped faces: the sign flips
    assert np.abs(wr.winding64(q, verts, faces[:, ::-1]) + w).max() < 1e-12


def test_vertex_query_is_k_plus_cone_and_classifies_without_a_threshold(scene):
    w, truth = scene["w"], scene["truth"]
    assert truth.sum() == {324: 50, 1284: 202}[len(w)]
    assert np.array_equal(w > 1.0, truth)
    # the cone's share: strictly inside (0, 1), the same whether or not another sheet encloses the vertex
    cone = w - truth
    assert cone.min() > 0.41 and cone.max() < 0.47 and np.abs(w - 1.0).min() > 0.41
    # against each sphere alone: k_i is the other sphere's winding at the vertex, the cone the vertex's own sphere's
    verts, faces, nA = scene["verts"], scene["faces"], scene["nA"]
    fa = faces[faces[:, 0] < nA]
    fb = faces[faces[:, 0] >= nA]
    k = np.concatenate([wr.winding64(verts[:nA], verts, fb), wr.winding64(verts[nA:], verts, fa)])
    assert np.array_equal(np.round(k).astype(int), truth.astype(int)) and np.abs(k - np.round(k)).max() < 1e-12
    own = np.concatenate([wr.winding64(verts[:nA], verts, fa, np.arange(nA)), wr.winding64(verts[nA:], verts, fb, np.arange(nA, len(w)))])
    assert np.abs(w - (k + own)).max() < 1e-12


def test_f32_restatement_is_within_the_bound_at_every_query(scene):
    err, B = np.abs(scene["w32"].astype(np.float64) - scene["w"]), scene["B"]
    print(f"{len(B)} vertices: B_i <= {B.max():.2e}, f32 restatement off by <= {err.max():.2e}, {100 * (err / B).max():.3f} % of B_i")
    assert np.all(np.isfinite(B)) and B.max() < 0.05
    assert np.all(err <= B)
    assert np.array_equal(scene["w32"] > 1.0, scene["truth"])


@pytest.mark.parametrize("name", ["fan", "hemisphere", "free_points"])
def test_open_meshes_and_free_points_are_within_the_bound(name):
    rng = np.random.default_rng(2)
    if name == "fan":
        verts, faces = wr.fan(40)
        q, skip = verts, np.arange(len(verts))
    elif name == "hemisphere":
        verts, faces = wr.hemisphere(2)
        q, skip = (rng.normal(size=(300, 3)) * 0.8).astype(np.float32), None
    else:
        verts, faces, _ = wr.two_spheres(2)
        q, skip = (rng.normal(size=(300, 3)) * 0.9 + [0.6, 0, 0]).astype(np.float32), None
    w, B = wr.winding64(q, verts, faces, skip), wr.bound64(q, verts, faces, skip)
    assert B.max() < 0.05
    assert np.all(np.abs(wr.kernel_form_f32(q, verts, faces, skip) - w) <= B)
    if name == "fan":
        # the apex skips every face; a rim vertex sees the 38 faces it is no corner of
        assert w[0] == 0.0 and np.all(np.abs(w[1:]) < 0.5) and np.ptp(w[1:]) < 1e-6
    if name == "hemisphere":
        frac = np.abs(w - np.round(w))
        assert (frac > 0.05).sum() > 200            # fractional: the generalised winding number of an open mesh


def test_conventions():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [np.nan, 0, 0]], np.float32)
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    q = np.array([[0.1, 0.1, 0.1], [1, 1, 1], [0, 0, 0]], np.float32)
    w = wr.winding64(q, verts, tet)
    assert abs(w[0] - 1) < 1e-12 and abs(w[1]) < 1e-12
    assert abs(w[2] - 0.125) < 1e-12                 # on a corner: the three faces that hold it give 0, the fourth an octant
    assert np.array_equal(wr.kernel_form_f32(q, verts, tet)[2:], np.float32([0.125]))
    # zero-area faces and repeated ids add nothing
    junk = np.array([[0, 0, 1], [2, 2, 2], [1, 3, 1]], np.int32)
    assert np.array_equal(wr.winding64(q, verts, np.concatenate([tet, junk])), w)
    # a non-finite corner of a counted face, a NaN query
    assert np.isnan(wr.winding64(q, verts, np.concatenate([tet, [[0, 1, 4]]]))).all()
    assert np.isnan(wr.winding64(np.array([[np.nan, 0, 0]], np.float32), verts, tet)).all()
    # on an edge: |z| = 0, the bound is infinite
    assert np.isinf(wr.bound64(np.array([[0.5, 0, 0]], np.float32), verts, tet)[0])


def test_vertex_normals_reference():
    verts, faces = wr.icosphere(2)
    n, cond = wr.vertex_normals64(verts, faces)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12 and (n * verts).sum(axis=1).min() > 0.999 and cond.max() < 1.1
    v2 = np.concatenate([verts, [[5, 5, 5]]]).astype(np.float32)
    n2, _ = wr.vertex_normals64(v2, np.concatenate([faces, [[0, 0, 1]]]))
    assert np.array_equal(n2[:-1], n) and np.all(n2[-1] == 0)


def test_the_term_reference_pushes_the_spheres_apart():
    """the figures the GPU tests of the term are held to: 50 enclosed vertices, all matched on the OTHER sphere, 3.206, -17.7, and
    eight gradient steps of 0.02 on B's shift bring the term below 1/100 of its start"""
    verts, faces, nA = wr.two_spheres(2)
    e = wr.self_penetration64(verts, faces)
    assert len(e["rows"]) == 50 and np.all(e["index"] >= 0)
    nfa = int((faces[:, 0] < nA).sum())
    assert np.all(np.where(e["rows"] < nA, e["index"] >= nfa, e["index"] < nfa))
    assert abs(e["value"] - 3.206) < 1e-3 and abs(e["grad"][nA:, 0].sum() + 17.7) < 0.05
    shift, start = np.zeros(3), e["value"]
    for _ in range(8):
        shift = shift - 0.02 * e["grad"][nA:].sum(axis=0)
        verts, faces, nA = wr.two_spheres(2, shift)
        e = wr.self_penetration64(verts, faces)
    print(f"term {start:.4f} -> {e['value']:.5f} after eight steps")
    assert e["value"] < start / 100
