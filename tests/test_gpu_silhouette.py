"""GPU: torch_layer.SilhouetteTerm, both halves, against tests/silhouette_ref.py, which takes the render, the visibility and the two
`nearest` images of the evaluation AS GIVEN and restates the composition and the sums in float64.

Scene: the 1000-vertex synthetic model with the 2000-face soup of tests/test_gpu_raster.py's `small` fixture, 3 frames at 96 x
128; the mask S is rendered from the same frames scaled by 1.08 about their centroid and shifted by (6, -3, 0) cm, so that both
S \\ M (rows of the data -> model half) and M \\ S (pulled vertices of the model -> data half) are non-empty.

Tolerances, u = 2^-24, eps = 2^-53, per vertex component, T the sum of the absolute values of the data -> model terms
(silhouette_ref's abs_dm), g_md the model -> data gradient:
  data -> model VALUE: equality of the integer sum and of the count of truncated rows, then of the float64 built from them.
  data -> model GRADIENT: 4.5 u T.  The rows VJP states |g - G*| <= 2 u T' for the sums G*, T' of the f32 rows it is given; the term
      rounds beta and m to f32 once each, so T' <= (1 + u)^2 T and |G*' - G*| <= (2 u + u^2) T: together below 4.5 u T.
  model -> data VALUE: C_VALUE eps scale_value_md; GRADIENT: C_GRAD eps scale_md + u |g_md| (autograd rounds the float64 gradient
      to the f32 of verts).  C_VALUE and C_GRAD are the roundings of the elementwise float64 operations: silhouette_ref
      measures them as float64 against extended precision over this test's scenes, in units of eps x the magnitudes that enter
      (silhouette_ref.evaluate: scale_md, scale_rho), and the constants here are 4 x the measured worst case.
      Measured on MI355X over the configurations below: gradient 0.191, value 0.170; C_GRAD = 0.764, C_VALUE = 0.68.
  both halves: the sum of the two, plus u (|g_md| + T) for the one f32 addition of the two gradients."""
import importlib

import numpy as np
import pytest

import silhouette_ref as sr

pytestmark = pytest.mark.gpu

V_SMALL, NF_SMALL = 1000, 2000
SIZE, INTR = (96, 128), (150.0, 150.0, 64.0, 48.0)
C_GRAD, C_VALUE = 0.764, 0.68
U, EPS = sr.U32, sr.EPS


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def tl():
    return importlib.import_module("3dbodyanimation_amd.torch_layer")


@pytest.fixture(scope="module")
def scene(torch, tl, api, synth):
    """(verts f32 [3, V, 3] numpy, faces, mask bool [3, H, W] on the GPU)"""
    m = synth.make_model(0, n_verts=V_SMALL)
    seq = synth.make_sequence(m, 6, seed=5)
    prob = api.Problem.from_sequence(api.Model(m), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"]
    faces = synth.make_faces(m, n_faces=NF_SMALL)
    verts = np.ascontiguousarray(cloud[:3]).astype(np.float32)
    target = torch.tensor(sr.shifted(verts, 1.08, (0.06, -0.03, 0.0)), device="cuda")
    mask = tl.render_depth(target, faces, INTR, SIZE)[1] >= 0
    return verts, faces, mask


def given(ev, term):
    """the evaluation's correspondences, as numpy, for silhouette_ref"""
    n = lambda t: t.detach().cpu().numpy()
    return dict(mask=n(term.mask), nearest_s=n(term.nearest_S), face=n(ev["face"]), bary=n(ev["bary"]), depth=n(ev["depth"]),
                visible=n(ev["visible"]) if "visible" in ev else np.zeros(ev["face"].shape[:1] + (V_SMALL,), bool),
                nearest_m=n(ev["nearest_model"]) if "nearest_model" in ev else np.full(ev["face"].shape, -1, np.int32))


def val(t):
    return float(t.detach())


def run(torch, term, verts):
    v = torch.tensor(verts, device="cuda", requires_grad=True)
    ev = term.evaluate(v)
    ev["cost"].backward()
    torch.cuda.synchronize()
    return ev, v.grad.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("trunc", (None, 6.0))
def test_value_and_gradient_of_both_halves(torch, tl, scene, trunc):
    verts, faces, mask = scene
    worst = {}
    for md, dm in ((False, True), (True, False), (True, True)):
        term = tl.SilhouetteTerm(mask, INTR, faces, trunc=trunc, model_to_data=md, data_to_model=dm)
        ev, g = run(torch, term, verts)
        assert ev["cost"].dtype == torch.float64
        gv = given(ev, term)
        ref = sr.evaluate(verts, faces, INTR, trunc=trunc, **gv)
        tol = np.zeros_like(g)
        want_g = np.zeros_like(g)
        if dm:
            S, M = gv["mask"], gv["face"] >= 0
            assert all((S[f] & ~M[f]).sum() > 50 and (M[f] & ~S[f]).sum() > 50 for f in range(3))     # both differences, every frame
            assert ref["n_rows"] == (S & ~M).sum() == ev["row_index"].shape[0]
            assert int(ev["sum_dist2"]) == ref["sum_dist2"] and int(ev["n_truncated"]) == ref["n_truncated"]
            assert val(ev["cost_data_to_model"]) == float(ref["cost_dm"])
            assert (ref["n_truncated"] > 0) == (trunc is not None) and ref["sum_dist2"] > 0
            tol += 4.5 * U * ref["abs_dm"]
            want_g += ref["grad_dm"]
        else:
            assert val(ev["cost_data_to_model"]) == 0.0
        if md:
            c_grad, c_value = sr.measure_constants(verts, faces, INTR, trunc=trunc, **gv)
            err_v = abs(val(ev["cost_model_to_data"]) - float(ref["cost_md"]))
            print(f"silhouette trunc {trunc}, model -> data: {ref['n_pulled']} of {int(gv['visible'].sum())} visible vertices pulled, "
                  f"cost {float(ref['cost_md']):.6e}, error {err_v:.2e} (bound {C_VALUE * EPS * float(ref['scale_value_md']):.2e}); "
                  f"float64 against extended precision: gradient {c_grad:.3f}, value {c_value:.3f} (x 4: the constants)")
            assert ref["n_pulled"] > 20
            assert err_v <= C_VALUE * EPS * float(ref["scale_value_md"])
            tol += C_GRAD * EPS * ref["scale_md"] + U * np.abs(ref["grad_md"])
            want_g += ref["grad_md"]
        else:
            assert val(ev["cost_model_to_data"]) == 0.0
        if md and dm:
            tol += U * (np.abs(ref["grad_md"]) + ref["abs_dm"])
        assert val(ev["cost"]) == val(ev["cost_model_to_data"]) + val(ev["cost_data_to_model"])
        err = np.abs(g - want_g)
        on = tol > 0
        ratio = float((err[on] / tol[on]).max())
        worst[(md, dm)] = ratio
        assert not g[~on].any() and not want_g[~on].any()            # a component nothing lands on is exactly 0
        assert np.abs(want_g).max() > 1.0
        print(f"silhouette trunc {trunc}, halves (model -> data {md}, data -> model {dm}): cost {val(ev['cost']):.6e}, "
              f"{int(on.sum())} live gradient components, largest {np.abs(want_g).max():.3e}, worst error {ratio:.3f} of its bound")
        assert ratio <= 1.0, worst


def test_gradient_is_bit_identical_and_flags_switch_halves_off(torch, tl, scene):
    verts, faces, mask = scene
    term = tl.SilhouetteTerm(mask, INTR, faces, trunc=6.0)
    ev1, g1 = run(torch, term, verts)
    ev2, g2 = run(torch, term, verts)
    assert np.array_equal(g1, g2) and val(ev1["cost"]) == val(ev2["cost"])
    only_dm = tl.SilhouetteTerm(mask, INTR, faces, trunc=6.0, model_to_data=False)
    only_md = tl.SilhouetteTerm(mask, INTR, faces, trunc=6.0, data_to_model=False)
    v = torch.tensor(verts, device="cuda")
    with torch.no_grad():
        a, b, c = float(only_dm(v)), float(only_md(v)), float(term(v))
    assert a == val(ev1["cost_data_to_model"]) > 0 and b == val(ev1["cost_model_to_data"]) > 0 and c == a + b
    neither = tl.SilhouetteTerm(mask, INTR, faces, model_to_data=False, data_to_model=False)
    assert float(neither(v)) == 0.0


def test_truncation_is_respected(torch, tl, scene):
    verts, faces, mask = scene
    v = torch.tensor(verts, device="cuda")
    trunc = 4.0
    with torch.no_grad():
        full = tl.SilhouetteTerm(mask, INTR, faces).evaluate(v)
        cut = tl.SilhouetteTerm(mask, INTR, faces, trunc=trunc).evaluate(v)
    rows = (mask & (full["face"] < 0)).cpu().numpy()
    d2 = full["dist2_model"].cpu().numpy()[rows].astype(np.int64)
    assert (d2 > trunc * trunc).any() and (d2 < trunc * trunc).any()
    assert float(full["cost_data_to_model"]) == float(d2.sum())
    assert float(cut["cost_data_to_model"]) == float(np.minimum(d2, trunc * trunc).sum())
    assert int(cut["n_truncated"]) == (d2 >= trunc * trunc).sum()
    assert float(cut["cost_model_to_data"]) <= float(full["cost_model_to_data"])
    direction = cut["row_direction"].cpu().numpy()
    assert not direction[d2 >= trunc * trunc].any() and direction[d2 < trunc * trunc].any(axis=1).all()


def test_an_empty_mask_and_a_mesh_behind_z_near_contribute_exactly_nothing(torch, tl, scene):
    verts, faces, mask = scene
    moved = verts.copy()
    moved[2, :, 2] -= 4.0                                             # frame 2: behind the camera, every face dropped
    assert moved[2, :, 2].max() < 0.1
    m = mask.clone()
    m[1] = False                                                      # frame 1: nothing observed
    term = tl.SilhouetteTerm(m, INTR, faces, trunc=6.0)
    ev, g = run(torch, term, moved)
    assert val(ev["cost"]) > 0 and np.abs(g[0]).max() > 1.0
    assert not g[1].any() and not g[2].any()
    assert not bool(ev["visible"][2].any()) and bool(ev["visible"][1].any()) and bool((ev["face"][2] < 0).all())
    frames = ev["row_frame"].cpu().numpy()
    assert len(frames) > 50 and (frames == 0).all()
    tail = tl.SilhouetteTerm(m[1:], INTR, faces, trunc=6.0)
    ev_tail, g_tail = run(torch, tail, moved[1:])
    assert val(ev_tail["cost"]) == 0.0 and not g_tail.any()
    alone = tl.SilhouetteTerm(m[:1], INTR, faces, trunc=6.0)
    ev0, g0 = run(torch, alone, moved[:1])
    assert np.array_equal(g0[0], g[0]) and val(ev0["cost_data_to_model"]) == val(ev["cost_data_to_model"])


def test_wrong_inputs_raise(torch, tl, scene):
    verts, faces, mask = scene
    v = torch.tensor(verts, device="cuda")
    with pytest.raises(TypeError):
        tl.SilhouetteTerm(mask.float(), INTR, faces)
    with pytest.raises(TypeError):
        tl.SilhouetteTerm(mask.to(torch.int32), INTR, faces)
    with pytest.raises(TypeError):
        tl.SilhouetteTerm(mask.cpu(), INTR, faces)
    with pytest.raises(ValueError):
        tl.SilhouetteTerm(mask[0], INTR, faces)
    with pytest.raises(ValueError):
        tl.SilhouetteTerm(mask, INTR[:3], faces)
    with pytest.raises(ValueError):
        tl.SilhouetteTerm(mask, INTR, faces, trunc=0.0)
    with pytest.raises(ValueError):
        tl.SilhouetteTerm(mask, INTR, faces, z_near=0.0)
    term = tl.SilhouetteTerm(mask.to(torch.uint8) * 7, INTR, faces)
    assert torch.equal(term.mask, mask)
    with pytest.raises(ValueError):
        term(v[:2])
    with pytest.raises(TypeError):
        term(v.double())
    with pytest.raises(TypeError):
        term(v.cpu())
    with pytest.raises(ValueError):
        term(v[:, :, :2])


def test_fit_beside_the_keypoints(torch, tl, api, synth):
    """30 steps of Adam on the keypoint + prior objective, with and without w SilhouetteTerm, from a start that is scaled and
    shifted against the ground truth whose render is the mask.  Asserted: the silhouette cost ends below its start.  Printed,
    not asserted: the mask IoU before and after, and the mean vertex distance to the ground truth with and without the term
    (recorded in DESIGN.md section 5, "Silhouette")."""
    F, steps, w = 3, 30, 0.5
    m = synth.make_model(0, n_verts=V_SMALL)
    faces = synth.make_faces(m, n_faces=NF_SMALL)
    gm = api.Model(m)
    seq = synth.make_sequence(m, F, seed=77)
    x0 = seq.gt_params.copy()
    x0[:, 0] *= 1.08
    x0[:, 4:7] += [0.06, -0.03, 0.0]
    layer = tl.SMPLLayer(gm, R0=seq.R0.reshape(F, 3, 3))
    prob = api.Problem.from_sequence(gm, seq, n_cols=86, use_shape=True, beta_pose=5.0, beta_shape=25.0, lambda_temporal=3.0)
    obj = tl.FitObjective(prob)
    beta = torch.tensor(seq.gt_beta, device="cuda")
    with torch.no_grad():
        v_gt, _ = layer(torch.tensor(seq.gt_params, device="cuda"), beta)
    mask = tl.render_depth(v_gt, faces, INTR, SIZE)[1] >= 0
    assert int(mask.sum(dim=(1, 2)).min()) > 300
    term = tl.SilhouetteTerm(mask, INTR, faces, trunc=20.0)

    def iou(verts):
        model = tl.render_depth(verts, faces, INTR, SIZE)[1] >= 0
        return float((model & mask).sum()) / float((model | mask).sum())

    def fit(weight):
        xt = torch.tensor(x0, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([xt], lr=0.01)
        for _ in range(steps):
            opt.zero_grad()
            loss = obj.cost(obj(xt, beta))
            if weight:
                loss = loss + weight * term(layer(xt, beta)[0])
            loss.backward()
            opt.step()
        with torch.no_grad():
            v, _ = layer(xt, beta)
            return float(term(v)), iou(v), float((v.double() - v_gt.double()).norm(dim=2).mean())

    with torch.no_grad():
        v0, _ = layer(torch.tensor(x0, device="cuda"), beta)
        c0, iou0 = float(term(v0)), iou(v0)
        d0 = float((v0.double() - v_gt.double()).norm(dim=2).mean())
    c1, iou1, d1 = fit(w)
    c_plain, iou_plain, d_plain = fit(0.0)
    print(f"silhouette fit, {steps} Adam steps: silhouette cost {c0:.1f} -> {c1:.1f} px^2 (keypoints alone: {c_plain:.1f}); mask IoU "
          f"{iou0:.3f} -> {iou1:.3f} (keypoints alone: {iou_plain:.3f}); mean vertex distance to the ground truth {d0 * 1e3:.2f} -> "
          f"{d1 * 1e3:.2f} mm (keypoints alone: {d_plain * 1e3:.2f} mm)")
    assert c0 > 0 and c1 < c0
