"""GPU: the torch layer over the winding number: vertex_winding, vertex_normals, winding_number, signed_distance and
SelfPenetrationTerm (torch_layer/solid.py), on the two-sphere scene of tests/winding_ref.py — the unit icosphere A and the icosphere B of
radius 0.7 about (1.2, 0, 0) as one mesh, 50 of 324 (202 of 1,284) vertices inside the other sphere.

Reference: wr.self_penetration64 (f64: winding with the own faces left out, the oriented brute force with minus the vertex normal,
the analytic gradient at the correspondence); tests/test_winding.py holds that reference to the figures 50 / 202, 3.206, -17.7.
Values are compared within the search's contract (k = 32 of include/bodyfit.h, on distances), gradients at the RETURNED
correspondence within the f32 bound of the surface backward."""
import importlib

import numpy as np
import pytest

import surface_ref as sr
import winding_ref as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def tl():
    return importlib.import_module("3dbodyanimation_amd.torch_layer")


@pytest.fixture(scope="module", params=[2, 3], ids=["324v", "1284v"])
def scene(request):
    verts, faces, nA = wr.two_spheres(request.param)
    return dict(verts=verts, faces=faces, nA=nA, truth=wr.two_spheres_truth(verts, nA), ref=wr.self_penetration64(verts, faces))


def shifted(torch, scene, shift):
    """verts [1, V, 3] on the device as a function of B's shift [3] (a leaf that requires grad)"""
    base = torch.tensor(scene["verts"], device="cuda")
    mask = torch.zeros((len(scene["verts"]), 1), device="cuda")
    mask[scene["nA"]:] = 1.0
    return (base + mask * shift.to(torch.float32)[None, :])[None]


def test_enclosed_set_matches_and_value(torch, tl, scene):
    verts, faces, nA, ref = scene["verts"], scene["faces"], scene["nA"], scene["ref"]
    term = tl.SelfPenetrationTerm(faces)
    vt = torch.tensor(verts[None], device="cuda", requires_grad=True)
    e = term.evaluate(vt)
    inside = e["inside"][0].cpu().numpy()
    assert inside.sum() == {324: 50, 1284: 202}[len(verts)] and np.array_equal(inside, scene["truth"])
    rows, index = e["rows"].cpu().numpy(), e["index"].cpu().numpy()
    assert np.array_equal(rows, ref["rows"]) and e["offset"].cpu().tolist() == [0, len(rows)]
    nfa = int((faces[:, 0] < nA).sum())
    assert np.all(index >= 0) and np.all(np.where(rows < nA, index >= nfa, index < nfa))      # every one on the OTHER sphere
    # distances: the search's contract against the oriented f64 brute force (optimality and consistency, k u (d + h) each)
    d, dstar = np.sqrt(e["dist2"].detach().cpu().numpy().astype(np.float64)), np.sqrt(ref["dist2"])
    h = sr.longest_edge(verts, faces, index)
    assert np.all(np.abs(d - dstar) <= 2 * sr.K * sr.U * (dstar + h))
    value = term(vt)
    assert value.dtype == torch.float64
    tol = float((2 * dstar * 2 * sr.K * sr.U * (dstar + h)).sum()) + len(rows) * sr.U * float(ref["dist2"].max())
    print(f"term {float(value.detach()):.6f} against {ref['value']:.6f} (tolerance {tol:.2e})")
    assert abs(float(value.detach()) - ref["value"]) <= tol
    # the gradient at the RETURNED correspondence, every vertex component
    value.backward()
    q = np.ascontiguousarray(verts[rows])
    gq, gv, av, lv, n_v, lq = sr.vjp(q, verts, faces, index, e["bary"].cpu().numpy(), np.ones(len(rows)))
    want = gv.copy()
    np.add.at(want, rows, gq)
    # the bounds of the surface backward (tests/test_gpu_closest_surface.py, check_vjp): a vertex sum 3 u loc + (2 n + 4) u abs, a
    # query row 3 u loc + 2 u |value|; autograd adds the two with one more rounding
    allow = 3 * sr.U * lv + (2 * n_v[:, None] + 4) * sr.U * av + sr.U * np.abs(gv)
    np.add.at(allow, rows, 3 * sr.U * lq + 3 * sr.U * np.abs(gq))
    got = vt.grad[0].double().cpu().numpy()
    assert np.all(np.abs(got - want) <= allow), float((np.abs(got - want) / allow).max())
    # (the reference's own correspondence may differ where the symmetry of the scene ties two faces at different points; what
    #  both agree on is the derivative along the axis of symmetry, checked in the next test)
    # backward twice: identical bits
    vt2 = torch.tensor(verts[None], device="cuda", requires_grad=True)
    term(vt2).backward()
    assert torch.equal(vt.grad, vt2.grad)


def test_the_gradient_moves_b_away_and_descent_separates_the_spheres(torch, tl, scene):
    term = tl.SelfPenetrationTerm(scene["faces"])
    shift = torch.zeros(3, dtype=torch.float64, device="cuda", requires_grad=True)
    start = term(shifted(torch, scene, shift))
    start.backward()
    want = scene["ref"]["grad"][scene["nA"]:].sum(axis=0)
    print(f"d term / d shift = {shift.grad.cpu().numpy()} against {want}; term {float(start.detach()):.4f}")
    assert float(shift.grad[0]) < 0 and abs(float(shift.grad[0]) - want[0]) < 1e-3 * abs(want[0])
    if len(scene["verts"]) == 324:
        assert abs(float(shift.grad[0]) + 17.7) < 0.05 and abs(float(start.detach()) - 3.206) < 1e-3
    value = start
    for _ in range(8):
        with torch.no_grad():
            shift -= 0.02 * shift.grad
        shift.grad = None
        value = term(shifted(torch, scene, shift))
        value.backward()
    print(f"after eight steps of 0.02: shift {shift.detach().cpu().numpy()}, term {float(value.detach()):.5f}")
    assert float(value.detach()) < float(start.detach()) / 100


def test_separated_spheres_cost_exactly_nothing(torch, tl, scene):
    term = tl.SelfPenetrationTerm(scene["faces"], trunc=0.05)
    shift = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device="cuda", requires_grad=True)
    vt = shifted(torch, scene, shift)
    e = term.evaluate(vt)
    assert not bool(e["inside"].any()) and e["rows"].numel() == 0 and e["index"].numel() == 0
    value = term(vt)
    assert float(value.detach()) == 0.0 and value.dtype == torch.float64
    value.backward()
    assert shift.grad is not None and bool((shift.grad == 0).all())


def test_subset_truncation_and_batches(torch, tl, scene):
    verts, faces, nA, ref = scene["verts"], scene["faces"], scene["nA"], scene["ref"]
    far = np.array([3.0, 0.0, 0.0], np.float32)
    batch = np.stack([verts, np.concatenate([verts[:nA], verts[nA:] + far]), verts[::1] * np.float32(1.0)])
    vt = torch.tensor(batch, device="cuda", requires_grad=True)
    term = tl.SelfPenetrationTerm(faces)
    e = term.evaluate(vt)
    n = len(ref["rows"])
    assert e["offset"].cpu().tolist() == [0, n, n, 2 * n]                         # the middle frame has no enclosed vertex
    single = term.evaluate(torch.tensor(verts[None], device="cuda"))
    assert torch.equal(e["dist2"][:n], single["dist2"]) and torch.equal(e["dist2"][n:], single["dist2"])
    assert torch.equal(e["winding"][0], single["winding"][0]) and torch.equal(e["winding"][2], single["winding"][0])
    # only B's vertices are tested
    ids = np.arange(nA, len(verts))
    sub = tl.SelfPenetrationTerm(faces, vertex_ids=ids).evaluate(torch.tensor(verts[None], device="cuda"))
    assert sub["winding"].shape == (1, len(ids)) and torch.equal(sub["winding"][0], single["winding"][0][nA:])
    assert np.array_equal(sub["rows"].cpu().numpy(), ref["rows"][ref["rows"] >= nA])
    # truncation: rho = min(s, tau^2)
    tau = float(np.sqrt(np.median(ref["dist2"])))
    cut = tl.SelfPenetrationTerm(faces, trunc=tau)(torch.tensor(verts[None], device="cuda"))
    want = np.minimum(single["dist2"].double().cpu().numpy(), tau * tau).sum()
    assert abs(float(cut) - want) <= 2 * sr.U * want          # (the clamp is taken at tau^2 rounded to f32)


def test_winding_number_vertex_normals_and_signed_distance(torch, tl, scene):
    verts, faces, nA = scene["verts"], scene["faces"], scene["nA"]
    rng = np.random.default_rng(6)
    ball = lambda n, r: (lambda d: d / np.linalg.norm(d, axis=1, keepdims=True) * r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))(rng.normal(size=(n, 3)))
    pts = np.concatenate([ball(120, 0.45),                                # inside A alone
                          ball(120, 0.15) + [0.75, 0, 0],                 # in the overlap
                          ball(120, 0.8) + [0.5, 2.5, 0]]).astype(np.float32)   # outside both
    w64 = wr.winding64(pts, verts, faces)
    keep = np.abs(w64 - np.round(w64)) < 1e-9
    vt = torch.tensor(verts[None], device="cuda", requires_grad=True)
    pt = torch.tensor(pts[None], device="cuda", requires_grad=True)
    w = tl.winding_number(pt, vt, faces)
    assert w.shape == (len(pts),) and not w.requires_grad
    assert np.all(np.abs(w.cpu().numpy() - w64) <= wr.bound64(pts, verts, faces))
    assert set(np.round(w64).astype(int)) == {0, 1, 2}
    # the vertex query through the layer equals the reference's classification, with and without a subset
    vw = tl.vertex_winding(vt, faces)
    assert vw.shape == (1, len(verts)) and np.array_equal((vw[0] > 1).cpu().numpy(), scene["truth"])
    n = tl.vertex_normals(vt, faces)
    n64, cond = wr.vertex_normals64(verts, faces)
    assert n.shape == (1, len(verts), 3) and not n.requires_grad
    assert np.all(np.abs(n[0].double().cpu().numpy() - n64).max(axis=1) <= wr.U + 2.0 ** -50 * cond)
    # the signed distance: sign(1/2 - w) sqrt(dist2), negative inside, closest_surface's gradient times sign / (2 sqrt(dist2))
    sdf, index, bary = tl.signed_distance(pt, vt, faces)
    d2, idx, _ = sr.brute_force(pts, verts, faces)
    want = np.sign(0.5 - w64) * np.sqrt(d2)
    h = sr.longest_edge(verts, faces, index.cpu().numpy())
    assert keep.all() and np.all(np.abs(sdf.detach().cpu().numpy() - want) <= 2 * sr.K * sr.U * (np.sqrt(d2) + h))
    assert (want[:240] < 0).all() and (want[240:] > 0).sum() > 100
    g = torch.tensor(rng.normal(size=len(pts)), device="cuda", dtype=torch.float32)
    (sdf * g).sum().backward()
    sign = torch.tensor(np.sign(0.5 - w64), device="cuda", dtype=torch.float32)
    pt2 = pt.detach().clone().requires_grad_()
    d2b, _, _ = tl.closest_surface(pt2, vt.detach(), faces)
    (d2b * (g * sign / (2 * torch.sqrt(d2b.detach())))).sum().backward()
    assert torch.allclose(pt.grad, pt2.grad, rtol=1e-5, atol=1e-7)
    # the gradient of the signed distance to a point is the unit direction away from the surface, times the sign
    unit = (pt.grad[0] / g[:, None]).norm(dim=1)
    assert bool(((unit - 1).abs() < 1e-3).all())
    # a point ON the surface: |sdf| within the search's consistency bound; where dist2 = 0 the gradient is 0, not inf; a NaN vertex: NaN
    on = torch.tensor(verts[None, :5].copy(), device="cuda")
    s0, i0, _ = tl.signed_distance(on, vt.detach(), faces)
    assert np.all(np.abs(s0.cpu().numpy()) <= sr.K * sr.U * sr.longest_edge(verts, faces, i0.cpu().numpy()))
    z = torch.tensor([0.0, 4.0, 9.0], device="cuda", requires_grad=True)
    tl._SignedRoot.apply(z, torch.tensor([-1.0, -1.0, 1.0], device="cuda")).sum().backward()
    assert z.grad.cpu().tolist() == [0.0, -0.25, 1.0 / 6.0] or torch.allclose(z.grad.cpu(), torch.tensor([0.0, -0.25, 1.0 / 6.0]))
    bad = verts.copy(); bad[3, 0] = np.nan
    sb, _, _ = tl.signed_distance(torch.tensor(pts[None, :4], device="cuda"), torch.tensor(bad[None], device="cuda"), faces)
    assert bool(torch.isnan(sb).all())
