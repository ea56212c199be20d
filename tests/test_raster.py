"""CPU: the reference of the depth render (tests/raster_ref.py) on hand-made scenes whose answers are known, the share of
ambiguous pixels of the scene the GPU test asserts face identity on, and the presence of the new names (the header's symbols,
the Python surface).  The kernel itself is tested in tests/test_gpu_raster.py."""
import importlib
import os

import numpy as np
import pytest

import raster_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scenes():
    return rr.hand_scenes()


def _ref(scene):
    verts, faces, intr, size, z_near, cull = scene
    return rr.Reference(verts, faces, intr, size, z_near, cull)


def test_new_names_exist(api):
    syms = api.declared_symbols()
    for s in ("bodyfit_raster_create", "bodyfit_raster_destroy", "bodyfit_raster_render_device",
              "bodyfit_raster_visibility_device"):
        assert s in syms, s
    assert hasattr(api.Raster, "render_device") and hasattr(api.Raster, "visibility_device")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    assert callable(tl.render_depth) and callable(tl.visible_vertices) and issubclass(tl.DepthMapTerm, tl.torch.nn.Module)
    assert "NOT differentiable" in tl.render_depth.__doc__


def test_the_mirrored_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "bodyfit.h")).read()
    k_e, k_z, tau_shift, c_shift, area_shift = rr.header_constants(text)
    assert (k_e, k_z) == (rr.K_E, rr.K_Z)
    assert (2.0 ** -tau_shift, 2.0 ** -c_shift, 2.0 ** -area_shift) == (rr.Q_SHIFT, rr.C_SHIFT, rr.AREA_TOL)


def test_layer_checks_inputs_without_a_device():
    torch = importlib.import_module("torch")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    faces = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(TypeError):
        tl.render_depth(torch.zeros((1, 3, 3)), faces, (1.0, 1.0, 0.0, 0.0), (4, 4))          # not on the GPU
    with pytest.raises(TypeError):
        tl.DepthMapTerm(torch.zeros((1, 4, 4)), (1.0, 1.0, 0.0, 0.0), faces)


def test_sample_on_a_shared_edge_and_on_a_shared_vertex(scenes):
    ref = _ref(scenes["shared_edge"])
    for i in range(2, 11):                       # the diagonal u = v is the shared edge: both faces cover, the lowest id wins
        lmin = [ref.F.evaluate(t, np.array([i]), np.array([i]))[1][0] for t in (0, 1)]
        assert lmin[0] == 0.0 and lmin[1] == 0.0
        assert ref.face[i, i] == 0 and ref.n_admissible[i, i] == 2 and not ref.unambiguous[i, i]
    assert ref.face[4, 7] == 0 and ref.face[7, 4] == 1 and ref.unambiguous[4, 7] and ref.unambiguous[7, 4]
    assert ref.face[2, 10] == 0 and ref.face[10, 2] == 1          # corners: edges are inclusive
    assert ref.covered.sum() == 81 and np.all(ref.depth[ref.covered] == 2.0)
    ref = _ref(scenes["shared_vertex"])
    assert all(ref.F.evaluate(t, np.array([6]), np.array([6]))[1][0] == 0.0 for t in range(4))
    assert ref.face[6, 6] == 0 and ref.n_admissible[6, 6] == 4
    assert ref.face[3, 6] == 0 and ref.face[6, 9] == 1 and ref.face[9, 6] == 2 and ref.face[6, 3] == 3


def test_identical_faces_tie_to_the_lowest_id(scenes):
    ref = _ref(scenes["identical_faces"])
    assert ref.covered.sum() > 30
    assert np.all(ref.face[ref.covered] == 0) and np.all(ref.n_admissible[ref.covered] == 2)
    assert not ref.unambiguous[ref.covered].any()
    assert ref.may[0] and ref.may[1] and not ref.must.any()


def test_a_corner_in_front_of_z_near_drops_the_face_whole(scenes):
    ref = _ref(scenes["behind_z_near"])
    assert not ref.F.drawn[0] and ref.F.drawn[1]
    assert ref.covered.sum() > 50 and np.all(ref.face[ref.covered] == 1)
    np.testing.assert_allclose(ref.depth[ref.covered], 4.0, rtol=1e-15)


def test_faces_without_an_area_are_not_drawn(scenes):
    ref = _ref(scenes["zero_area"])
    assert list(ref.F.drawn) == [False, False, True]
    assert np.all(ref.face[ref.covered] == 2) and ref.face[6, 6] == 2


def test_backface_culling_of_both_orientations(scenes):
    culled, plain = _ref(scenes["cull"]), _ref(scenes["no_cull"])
    assert list(culled.F.drawn) == [False, True] and list(plain.F.drawn) == [True, True]
    assert np.array_equal(culled.covered, plain.covered) and culled.covered.sum() > 30
    assert np.all(culled.face[culled.covered] == 1) and np.all(culled.depth[culled.covered] == 2.0)
    assert np.all(plain.face[plain.covered] == 0) and np.all(plain.depth[plain.covered] == 1.0)


def test_front_is_the_normal_towards_the_camera_as_the_overlay_culls():
    """A < 0 iff n . v0 < 0 (n the normal in the orientation of faces); the overlay keeps n_z < 0, the same sign wherever the face
    is not seen nearly edge-on.  On a closed surface with outward normals culling changes nothing that is visible."""
    verts, faces, intr, size = rr.two_spheres()
    F = rr.Faces(verts, faces, intr, size)
    v = verts.astype(np.float64)[faces]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    toward = (n * v[:, 0]).sum(axis=1)
    assert np.array_equal(F.A < 0, toward < 0)
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    clear = np.abs(unit[:, 2]) > 0.3               # not edge-on: the overlay's rule and this one agree
    assert clear.sum() > 300 and np.array_equal((n[:, 2] < 0)[clear], (F.A < 0)[clear])
    plain, culled = rr.Reference(verts, faces, intr, size), rr.Reference(verts, faces, intr, size, cull=True)
    assert np.array_equal(plain.face, culled.face) and np.array_equal(plain.depth, culled.depth)


def test_depth_is_the_ray_plane_intersection(scenes):
    verts, faces, intr, size, z_near, cull = scenes["slanted"]
    ref = _ref(scenes["slanted"])
    fx, fy, cx, cy = intr
    v = verts.astype(np.float64)
    n = np.cross(v[2] - v[0], v[1] - v[0])
    ys, xs = np.nonzero(ref.covered)
    assert len(ys) > 40
    d = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones(len(ys))], axis=1)
    z = (n @ v[0]) / (d @ n)
    np.testing.assert_allclose(ref.depth[ys, xs], z, rtol=1e-13)
    assert ref.depth[ys, xs].min() < 1.5 and ref.depth[ys, xs].max() > 2.5
    lam = ref.exact_bary()[ys, xs]
    np.testing.assert_allclose(lam @ ref.F.u[0].astype(np.float64), xs, atol=1e-11)     # the weights reproduce the sample
    np.testing.assert_allclose(lam @ ref.F.v[0].astype(np.float64), ys, atol=1e-11)


def test_two_spheres_keep_their_ambiguous_share_under_the_cap():
    """The GPU test asserts face identity on the unambiguous pixels only; this cap (2 % of the covered pixels) keeps that
    assertion from hiding failures."""
    verts, faces, intr, size = rr.two_spheres()
    assert verts.shape == (264, 3) and faces.shape == (520, 3)
    ref = rr.Reference(verts, faces, intr, size)
    share = ref.ambiguous_share()
    print(f"two spheres: {int(ref.covered.sum())} covered pixels, {int((ref.covered & ~ref.unambiguous).sum())} ambiguous "
          f"({share:.2%}); faces must / may be visible {int(ref.must.sum())} / {int(ref.may.sum())}, vertices "
          f"{int(ref.must_vertices.sum())} / {int(ref.may_vertices.sum())}; largest tau {ref.F.tau.max() / rr.U:.2f} u")
    assert ref.covered.sum() > 2000
    assert share <= 0.02
    assert ref.must.sum() > 150 and np.all(ref.may[ref.must])
    # the exact answer satisfies its own contract
    rr.check_contract(ref, ref.depth.astype(np.float32), ref.face.astype(np.int32), ref.exact_bary().astype(np.float32))


def test_the_contract_check_rejects_wrong_answers():
    verts, faces, intr, size = rr.two_spheres()
    ref = rr.Reference(verts, faces, intr, size)
    depth, face = ref.depth.astype(np.float32), ref.face.astype(np.int32)
    ys, xs = np.nonzero(ref.unambiguous & ref.covered)
    y, x = ys[len(ys) // 2], xs[len(xs) // 2]
    bad = depth.copy(); bad[y, x] *= np.float32(1 + 1e-5)
    with pytest.raises(AssertionError):
        rr.check_contract(ref, bad, face)
    bad = face.copy(); bad[y, x] = -1
    d2 = depth.copy(); d2[y, x] = np.inf
    with pytest.raises(AssertionError):
        rr.check_contract(ref, d2, bad)
    hidden = int(np.nonzero(~ref.may & ref.F.drawn)[0][0])          # a face on the far side
    bad = face.copy(); bad[y, x] = hidden
    with pytest.raises(AssertionError):
        rr.check_contract(ref, depth, bad)


def test_visibility_statement():
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]], np.int32)
    img = np.array([[-1, 2, 2], [0, -1, 7]], np.int32)              # 7: not a face of this topology
    fv, vv = rr.visibility_of(img, faces, 8)
    assert list(fv) == [1, 0, 1] and list(vv) == [1, 1, 1, 0, 1, 1, 1, 0]


def test_the_kernels_arithmetic_meets_the_contract_on_every_scene(synth):
    """k_raster.hip's arithmetic restated in numpy f64 (raster_ref.kernel_form_f64), on the scenes of the GPU test: the bound of
    include/bodyfit.h is attainable, and the check accepts an honest answer."""
    for name, (verts, faces, intr, size, z_near, cull) in rr.contract_scenes(synth).items():
        ref = rr.Reference(verts, faces, intr, size, z_near, cull)
        depth, face, bary = rr.kernel_form_f64(verts, faces, intr, size, z_near, cull)
        worst = rr.check_contract(ref, depth, face, bary)
        print(f"{name}: {int(ref.covered.sum())} covered, ambiguous {ref.ambiguous_share():.2%}, worst -min lambda / tau "
              f"{worst[0]:.2e}, depth {worst[1]:.2f} of its bound, weights {worst[2]:.2f} of tau; "
              f"differs from the exact face on {int((face != ref.face).sum())} pixels")
        assert (ref.F.valid3d.sum() < len(faces)) == name.startswith(("soup_at_0.9m", "hand_behind"))
