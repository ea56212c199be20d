"""GPU: the mesh winding number (bodyfit_surface_winding_device, k_wn_sum / k_wn_finish of k_winding.hip) and the vertex normals
(bodyfit_surface_vertex_normals_device), through api.Surface.

Reference: tests/winding_ref.py; check() asserts the contract of include/bodyfit.h, |w^ - w*| <= B_i (k = 64, k_s = 16), for EVERY
query, and tests/test_winding.py has shown on the same scenes that B_i < 0.05 and that the f32 restatement of the kernel's
arithmetic meets it.  Shapes: 640 faces are 2 1/2 LDS tiles and two splits, 324 vertices one full and one partial query tile;
2,560 faces are ten splits at 1 and 3 frames and eight at 24; the fan, the hemisphere and the tetrahedron run unsplit.  The device helpers (Queries, Verts) are
those of tests/test_gpu_closest_surface.py."""
import importlib

import numpy as np
import pytest

import winding_ref as wr
from test_gpu_closest_surface import Queries, Verts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def posed(verts, F, seed=0):
    """[F, V, 3] f32: frame 0 as given, every later frame rotated, scaled and moved on its own"""
    rng = np.random.default_rng(seed)
    out = [verts.astype(np.float32)]
    for _ in range(F - 1):
        R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        R = R * np.sign(np.linalg.det(R))
        out.append((rng.uniform(0.6, 1.5) * verts.astype(np.float64) @ R.T + rng.normal(size=3)).astype(np.float32))
    return np.stack(out)


def run(torch, surf, q, v, skip=None):
    """w [N] on the device; skip: the packed [N] ids, a numpy array, or None"""
    w = torch.full((max(q.total, 1),), -7.0, dtype=torch.float32, device="cuda")
    sk = None if skip is None else torch.tensor(np.ascontiguousarray(skip, np.int32).reshape(-1), device="cuda")
    surf.winding_device(q.ps, sk.data_ptr() if sk is not None else None, v.ptr, v.stride, q.F, q.total, w.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return w[:q.total]


def vertex_query(torch, api, v):
    """the vertex query of the posed mesh v: the uniform set over the vertex buffer itself, and its skip ids"""
    q = Queries.__new__(Queries)
    q.frames, q.F, q.total, q.stride, q.buf = v.frames, v.F, v.F * v.V, v.stride, v.buf
    q.off = np.arange(v.F + 1) * v.V
    q.ps = api.PointSet.uniform(v.ptr, v.V, v.stride)
    return q, np.tile(np.arange(v.V, dtype=np.int32), v.F)


def check(q, vframes, faces, w, skip=None, label="", frames=None):
    """|w^ - w*| <= B_i at every query of the frames (all, or the listed ones); returns the f64 values per frame"""
    wh = w.cpu().numpy()
    worst, ref = 0.0, {}
    for f in (range(q.F) if frames is None else frames):
        qf, got = q.frames[f], q.split(wh)[f]
        sk = None if skip is None else q.split(np.asarray(skip))[f]
        want, B = wr.winding64(qf, vframes[f], faces, sk), wr.bound64(qf, vframes[f], faces, sk)
        assert np.all(np.isfinite(B)) and (B.max(initial=0.0) < 0.05), (label, f, "the scene is not one the bound classifies")
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= B), (label, f, int((err > B).sum()), float((err / np.maximum(B, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(B, 1e-300)).max(initial=0.0)))
        ref[f] = want
    print(f"winding {label}: device error at most {100 * worst:.3f} % of B_i")
    return ref


# ---- 1. the vertex query on the two-sphere scene -----------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [2, 3], ids=["640f", "2560f"])
def test_two_spheres_vertex_query_frames_and_determinism(torch, api, subdiv):
    verts, faces, nA = wr.two_spheres(subdiv)
    surf = api.Surface(0, len(verts), faces)
    P = posed(verts, 3, seed=subdiv)
    v3 = Verts(torch, P, stride=3 * len(verts) + 5)
    q3, skip3 = vertex_query(torch, api, v3)
    w3 = run(torch, surf, q3, v3, skip3)
    ref = check(q3, v3.frames, faces, w3, skip3, f"two spheres {len(faces)} faces F=3")
    truth = wr.two_spheres_truth(verts, nA)
    assert int(truth.sum()) == {2: 50, 3: 202}[subdiv]
    assert np.array_equal(ref[0] > 1.0, truth)
    inside = (w3 > 1.0).cpu().numpy().reshape(3, -1)
    assert all(np.array_equal(inside[f], truth) for f in range(3))       # a similarity transform keeps what is enclosed
    assert torch.equal(w3, run(torch, surf, q3, v3, skip3))                # two runs: the same bits
    for f in range(3):                                                     # frame f of the batch == the single-frame call
        v1 = Verts(torch, P[f:f + 1])
        q1, skip1 = vertex_query(torch, api, v1)
        assert torch.equal(run(torch, surf, q1, v1, skip1), w3[f * len(verts):(f + 1) * len(verts)]), f
    # another split of the face range: the split follows the number of query tiles (about four workgroups per compute unit), so a
    # batch of 24 frames runs with fewer splits than one of 3 or 1 whenever the face count, not the device, capped those
    # (n_faces / 256 = 10 at 2,560 faces: 24 x 6 tiles leave 8 on 256 compute units).  The sum is exact, so the bits are the same.
    P24 = np.concatenate([P] * 8)
    v24 = Verts(torch, P24)
    q24, skip24 = vertex_query(torch, api, v24)
    w24 = run(torch, surf, q24, v24, skip24).view(8, -1)
    assert all(torch.equal(w24[k], w3) for k in range(8))
    # skip off: every vertex lies on the surface, on the corners of its own faces, which then count 0 all the same
    w_off = run(torch, surf, q3, v3, None)
    v1 = Verts(torch, P[:1]); q1, skip1 = vertex_query(torch, api, v1)
    w1_off = run(torch, surf, q1, v1, None)
    assert torch.equal(w1_off, w_off[:len(verts)])
    check(q1, v1.frames, faces, w1_off, None, "skip off")
    assert torch.equal(w1_off, w3[:len(verts)])      # the faces a vertex is a corner of give an exact 0 either way


def test_ragged_free_points_with_an_empty_frame(torch, api):
    verts, faces, _ = wr.two_spheres(2)
    surf = api.Surface(0, len(verts), faces)
    P = posed(verts, 3, seed=5)
    rng = np.random.default_rng(3)
    frames = [(rng.normal(size=(n, 3)) * 0.9 + [0.6, 0, 0]).astype(np.float32) for n in (300, 0, 77)]
    frames[2] = (frames[2].astype(np.float64) * 1.2 + P[2].mean(axis=0)).astype(np.float32)
    q, v = Queries(torch, api, frames), Verts(torch, P)
    w = run(torch, surf, q, v)
    ref = check(q, v.frames, faces, w, None, "ragged 300 / 0 / 77")
    assert set(np.round(ref[0]).astype(int)) == {0, 1, 2}
    assert torch.equal(w, run(torch, surf, q, v))
    for f in (0, 2):
        q1, v1 = Queries(torch, api, [frames[f]]), Verts(torch, P[f:f + 1])
        assert torch.equal(run(torch, surf, q1, v1), w[int(q.off[f]):int(q.off[f + 1])])
    # skip ids on free points: -1 skips none, an id leaves its faces out
    skip = np.full(q.total, -1, np.int32)
    assert torch.equal(run(torch, surf, q, v, skip), w)
    skip[::3] = 7
    check(q, v.frames, faces, run(torch, surf, q, v, skip), skip, "ragged with skip ids")
    # a uniform set inside padded rows
    qu = Queries(torch, api, [frames[0][:70], frames[0][70:140], frames[0][140:210]], uniform_stride=3 * 70 + 2)
    check(qu, v.frames, faces, run(torch, surf, qu, v), None, "uniform 3 x 70")


# ---- 2. open meshes, orientation, degenerate faces -----------------------------------------------------------------------------------
def test_fan_apex_of_valence_40(torch, api):
    verts, faces = wr.fan(40)
    surf = api.Surface(0, len(verts), faces)
    v = Verts(torch, verts[None])
    q, skip = vertex_query(torch, api, v)
    w = run(torch, surf, q, v, skip)
    check(q, v.frames, faces, w, skip, "fan, skip on")
    assert float(w[0]) == 0.0                                           # the apex leaves out all 40 faces
    above = Queries(torch, api, [np.array([[0, 0, 0.31], [0, 0, 0.29], [0, 0, 5.0]], np.float32)])
    wa = run(torch, surf, above, v)
    ref = check(above, v.frames, faces, wa, None, "fan, free points")
    assert ref[0][0] < -0.3 and ref[0][1] > 0.3                           # the jump of 1 across an open sheet


def test_open_hemisphere_is_fractional_and_flipped_faces_flip_the_sign(torch, api):
    verts, faces = wr.hemisphere(2)
    rng = np.random.default_rng(4)
    q = Queries(torch, api, [(rng.normal(size=(300, 3)) * 0.8).astype(np.float32)])
    v = Verts(torch, verts[None])
    w = run(torch, api.Surface(0, len(verts), faces), q, v)
    ref = check(q, v.frames, faces, w, None, "hemisphere")
    assert (np.abs(ref[0] - np.round(ref[0])) > 0.05).sum() > 200
    flipped = np.ascontiguousarray(faces[:, ::-1])
    wf = run(torch, api.Surface(0, len(verts), flipped), q, v)
    refl = check(q, v.frames, flipped, wf, None, "hemisphere, flipped")
    assert np.abs(refl[0] + ref[0]).max() < 1e-12


def test_degenerate_faces_corner_and_edge_queries(torch, api):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, 0.5, 0.125]], np.float32)
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    junk = np.array([[0, 0, 1], [2, 2, 2], [1, 3, 1], [4, 4, 0]], np.int32)
    pts = np.array([[0.1, 0.1, 0.1], [1, 1, 1], [0, 0, 0], [0, 0, 1], [-0.2, 0.3, 0.4]], np.float32)
    q, v = Queries(torch, api, [pts]), Verts(torch, verts[None])
    w = run(torch, api.Surface(0, 5, tet), q, v)
    ref = check(q, v.frames, tet, w, None, "tetrahedron")
    assert abs(ref[0][0] - 1) < 1e-12 and abs(ref[0][2] - 0.125) < 1e-12   # inside; on a corner: an octant from the far face
    # a query exactly on a corner of ONE face: num = den = 0, an exact 0
    one = api.Surface(0, 5, tet[:1])
    assert run(torch, one, Queries(torch, api, [verts[:3]]), v).cpu().tolist() == [0.0, 0.0, 0.0]
    # zero-area faces and repeated ids: within the bound of the mesh with them (they count k_s each, nothing else)
    both = np.concatenate([tet[:2], junk, tet[2:]])
    wj = run(torch, api.Surface(0, 5, both), q, v)
    refj = check(q, v.frames, both, wj, None, "tetrahedron with degenerate faces")
    assert np.abs(refj[0] - ref[0]).max() < 1e-12
    # on an edge midpoint |z| = 0: finite, and nothing else
    edge = Queries(torch, api, [np.array([[0.5, 0, 0], [0, 0.5, 0.5], [0.5, 0.5, 0]], np.float32)])
    we = run(torch, api.Surface(0, 5, tet), edge, v)
    assert bool(torch.isfinite(we).all())


# ---- 3. non-finite inputs, no-ops, errors -------------------------------------------------------------------------------------------------
def test_a_nan_vertex_spoils_its_frame_only(torch, api):
    verts, faces, _ = wr.two_spheres(2)
    surf = api.Surface(0, len(verts), faces)
    P = posed(verts, 3, seed=9)
    clean = Verts(torch, P)
    q, skip = vertex_query(torch, api, clean)
    w = run(torch, surf, q, clean, skip)
    for bad in (np.nan, np.inf):
        Pb = P.copy(); Pb[1, 200, 1] = bad
        vb = Verts(torch, Pb)
        qb, _ = vertex_query(torch, api, vb)
        wb = run(torch, surf, qb, vb, skip).view(3, -1)
        assert bool(torch.isnan(wb[1]).all())
        assert torch.equal(wb[0], w.view(3, -1)[0]) and torch.equal(wb[2], w.view(3, -1)[2])
    # a vertex no face holds may be anything
    loose = np.concatenate([verts, [[np.nan, 0, 0]]]).astype(np.float32)
    s2, v2 = api.Surface(0, len(loose), faces), Verts(torch, loose[None])
    pts = Queries(torch, api, [np.array([[0.1, 0, 0], [np.nan, 0, 0], [3, 3, 3], [0, np.inf, 0], [0.9, 0, 0]], np.float32)])
    wp = run(torch, s2, pts, v2).cpu().numpy()
    assert np.isnan(wp[[1, 3]]).all() and np.array_equal(np.round(wp[[0, 2, 4]]), [1, 0, 2])


def test_no_ops_and_errors(torch, api):
    verts, faces = wr.fan(5)
    surf = api.Surface(0, len(verts), faces)
    v = Verts(torch, verts[None])
    q = Queries(torch, api, [np.zeros((2, 3), np.float32)])
    w = torch.full((2,), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    surf.winding_device(q.ps, None, v.ptr, v.stride, 0, 0, w.data_ptr(), st)                          # no frames
    surf.winding_device(Queries(torch, api, [np.zeros((0, 3))]).ps, None, v.ptr, v.stride, 1, 0, w.data_ptr(), st)   # no rows
    torch.cuda.synchronize()
    assert w.cpu().tolist() == [-7.0, -7.0]
    empty = api.Surface(0, len(verts), np.zeros((0, 3), np.int32))                                     # no faces: 0
    assert run(torch, empty, q, v).cpu().tolist() == [0.0, 0.0]
    with pytest.raises(api.BodyfitError):
        surf.winding_device(q.ps, None, v.ptr, v.stride, 1, 2, None, st)
    with pytest.raises(api.BodyfitError):
        surf.winding_device(q.ps, None, v.ptr, 3 * len(verts) - 1, 1, 2, w.data_ptr(), st)
    with pytest.raises(api.BodyfitError):
        surf.vertex_normals_device(v.ptr, v.stride, 1, None, st)


# ---- 4. vertex normals ------------------------------------------------------------------------------------------------------------------------
def test_vertex_normals(torch, api):
    """|n^ - n*| <= u + 2^-50 c_i per component (include/bodyfit.h): one rounding of a number <= 1 and the f64 sums' own rounding
    amplified by the cancellation c_i = sum |N_t| / |sum N_t|; isolated vertices and vertices of degenerate faces only get 0"""
    verts, faces, _ = wr.two_spheres(2)
    extra = np.array([[5, 5, 5], [6, 5, 5], [7, 5, 5], [np.nan, 1, 1], [8, 8, 8]], np.float32)   # isolated, collinear, NaN, its neighbour
    V0 = len(verts)
    verts = np.concatenate([verts, extra])
    faces = np.concatenate([faces, [[V0, V0, V0 + 1], [V0 + 1, V0 + 2, V0 + 1], [V0 + 3, V0 + 4, 0]]]).astype(np.int32)
    surf = api.Surface(0, len(verts), faces)
    P = posed(verts, 2, seed=11)
    v = Verts(torch, P, stride=3 * len(verts) + 4)
    n = torch.full((2, len(verts), 3), -9.0, dtype=torch.float32, device="cuda")
    surf.vertex_normals_device(v.ptr, v.stride, 2, n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    again = torch.full_like(n, -9.0)
    surf.vertex_normals_device(v.ptr, v.stride, 2, again.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(n, again)
    nh = n.cpu().numpy()
    for f in range(2):
        want, cond = wr.vertex_normals64(P[f], faces)
        err = np.abs(nh[f].astype(np.float64) - want).max(axis=1)
        assert np.all(err <= wr.U + 2.0 ** -50 * cond), (f, float(err.max()))
        assert np.all(nh[f][V0:] == 0) and np.all(nh[f][0] == 0)         # no area, a NaN corner (vertex 0 shares that face)
        assert np.abs(np.linalg.norm(nh[f][1:V0], axis=1) - 1).max() < 1e-6
    one = torch.empty((1, len(verts), 3), dtype=torch.float32, device="cuda")
    v1 = Verts(torch, P[1:2])
    surf.vertex_normals_device(v1.ptr, v1.stride, 1, one.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(one[0], n[1])
