"""GPU: lighting.  bodyfit_raster_light_device and bodyfit_raster_light_grad_device against the extended-precision reference
of their contracts (lighting_ref.py) on EVERY pixel and coefficient; the reduction's edges, frame independence and bit identity;
bodyfit_surface_vertex_normals_vjp_device on every vertex; torch_layer.lighting against torch f64 autograd through the same
definition at the same face image; the fit of a light with LitPhotometricTerm against its restatement."""
import importlib

import numpy as np
import pytest

import depth_rows_ref as dr
import interp_ref as ir
import lighting_ref as lr
import raster_ref as rr
import winding_ref as wr
from test_gpu_appearance import host, junk_lambda, padded, ptr, render, run_shade, stream, three_poses
from test_gpu_depth_rows import SCENES, three_frames
from test_gpu_interp_rows import beta_f64
from test_lighting import FIT_FRACTION, FIT_STORE_DIFF, inputs

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -24
CHANNELS = (1, 3, 4)


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def lighting():
    return importlib.import_module("3dbodyanimation_amd.torch_layer.lighting")


@pytest.fixture(scope="module")
def tl():
    return importlib.import_module("3dbodyanimation_amd.torch_layer")


@pytest.fixture(scope="module")
def scenes(synth):
    return dr.row_scenes(synth)


def dev(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def bits(t):
    return host(t.detach()).view(np.int32)


def gpu_normals(torch, api, faces, vbuf, vstride, V, F):
    """the kernel's own vertex normals [F, V, 3] f32 of the padded vertex buffer"""
    s = api.Surface(0, V, faces)
    n = torch.full((F, V, 3), float("nan"), dtype=torch.float32, device="cuda")
    s.vertex_normals_device(ptr(vbuf), vstride, F, ptr(n), stream(torch))
    torch.cuda.synchronize()
    s.close()
    return host(n)


def run_light(torch, h, face, bary, vbuf, vstride, nbuf, nstride, albedo, C, lbuf, lstride, F, outputs=(True, True)):
    """(image, normal, shading) of the kernel, the outputs pre-filled with junk"""
    H, W = h.height, h.width
    image = torch.full((F, H, W, C), float("nan"), dtype=torch.float32, device="cuda")
    normal = torch.full((F, H, W, 3), -3.0, dtype=torch.float32, device="cuda") if outputs[0] else None
    shading = torch.full((F, H, W, C), float("nan"), dtype=torch.float32, device="cuda") if outputs[1] else None
    h.light_device(ptr(face), ptr(bary), ptr(vbuf), vstride, ptr(nbuf), nstride, ptr(albedo), C, ptr(lbuf), lstride, F, ptr(image),
                   ptr(normal), ptr(shading), stream(torch))
    torch.cuda.synchronize()
    return image, normal, shading


def run_light_grad(torch, api, h, face, bary, vbuf, vstride, nbuf, nstride, albedo, C, lbuf, lstride, F, G, outputs=(True, True, True)):
    """(grad_albedo, grad_m, grad_light) of the kernels, the outputs and the workspace pre-filled with junk"""
    H, W = h.height, h.width
    ga = torch.full((F, H, W, C), float("nan"), dtype=torch.float32, device="cuda") if outputs[0] else None
    gm = torch.full((F, H, W, 3), float("nan"), dtype=torch.float32, device="cuda") if outputs[1] else None
    gl = torch.full((F, 9, C), float("nan"), dtype=torch.float32, device="cuda") if outputs[2] else None
    work = torch.full((api.light_grad_layout(H * W, C, F)[2],), float("nan"), dtype=torch.float64, device="cuda") if outputs[2] else None
    h.light_grad_device(ptr(face), ptr(bary), ptr(vbuf), vstride, ptr(nbuf), nstride, ptr(albedo), C, ptr(lbuf), lstride, F, ptr(G),
                        ptr(ga), ptr(gm), ptr(gl), ptr(work), stream(torch))
    torch.cuda.synchronize()
    return ga, gm, gl


def light_buffers(torch, lights, shared, C, pad=5):
    """(device buffer, stride in floats) of one shared light or of per-frame lights inside poisoned rows"""
    if shared:
        return dev(torch, lights[0]), 0
    return padded(torch, lights, 9 * C, 9 * C + pad, np.nan), 9 * C + pad


def check_all(frames, faces, face_h, bary_h, normals, albedo, lights, shared, G, out_f, out_g, label):
    """the contracts on every pixel of every frame and every coefficient; returns the references"""
    worst = np.zeros(4)
    refs = []
    for f in range(len(frames)):
        with np.errstate(all="ignore"):
            ex = lr.light_exact(face_h[f], bary_h[f], frames[f], faces, normals[f], albedo[f], lights[0 if shared else f])
        refs.append(ex)
        image, normal, shading = (None if o is None else o[f] for o in out_f)
        w = lr.check_light(ex, image, normal, shading)
        ga, gm, gl = (None if o is None else o[f] for o in out_g)
        worst = np.maximum(worst, (w,) + lr.check_grad(ex, G[f], ga, gm, gl))
    lit = sum(int(ex["lit"].sum()) for ex in refs)
    print(f"lighting {label}: {lit} lit pixels; worst image {worst[0]:.3f}, grad_albedo {worst[1]:.3f}, grad_m {worst[2]:.3f}, "
          f"grad_light {worst[3]:.3f} of their bounds")
    return refs


# ---- 1. the contracts, every pixel and every coefficient ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_contracts_on_every_pixel_and_coefficient(torch, api, scenes, name):
    """F = 3 (the second frame holds a NaN and an infinite corner, so zero vertex normals; the third lies behind the camera), a
    padded and poisoned vertex stride and normal stride, a NaN in one corner normal, junk-filled outputs and workspace; C and
    (shared / per-frame light with a padded and poisoned stride) rotating over the scenes; each optional output NULL in turn leaves
    the others bit-identical; then a hand-made round-robin face image with junk barycentrics"""
    verts, faces, intr, size, z_near, cull = scenes[name]
    H, W = size
    V, F = len(verts), 3
    frames = three_poses(verts, faces[[0, len(faces) - 1]])
    h = api.Raster(0, V, faces, W, H)
    vstride, nstride = 3 * V + 13, 3 * V + 7
    vbuf = padded(torch, frames, 3 * V, vstride, -777.0)
    _, face, bary = render(torch, h, vbuf, vstride, F, intr, z_near, cull)
    torch.cuda.synchronize()
    face_h, bary_h = host(face), host(bary)
    normals = gpu_normals(torch, api, faces, vbuf, vstride, V, F)
    seen = np.unique(face_h[0][face_h[0] >= 0])
    if len(seen):
        normals[0, faces[seen[len(seen) // 2], 1], 2] = np.nan        # a corner normal with a NaN, in a face that owns pixels
    nbuf = padded(torch, list(normals), 3 * V, nstride, np.nan)
    rot = SCENES.index(name)
    C, shared = CHANNELS[rot % 3], (rot // 3) % 2 == 0
    rng = np.random.default_rng(rot)
    albedo = rng.uniform(0.05, 1.0, (F, H, W, C)).astype(np.float32)
    G = rng.standard_normal((F, H, W, C)).astype(np.float32)
    lights = [inputs(np.random.default_rng(50 + f), size, C)[1] for f in range(1 if shared else F)]
    lbuf, lstride = light_buffers(torch, lights, shared, C)
    a_t, G_t = dev(torch, albedo), dev(torch, G)
    args = (vbuf, vstride, nbuf, nstride, a_t, C, lbuf, lstride, F)
    out_f = run_light(torch, h, face, bary, *args)
    out_g = run_light_grad(torch, api, h, face, bary, *args, G_t)
    refs = check_all(frames, faces, face_h, bary_h, normals, albedo, lights, shared, G, [host(o) for o in out_f],
                     [host(o) for o in out_g], f"{name} C={C} {'shared' if shared else 'per-frame'}")
    if len(seen):
        assert ((face_h[0] >= 0) & ~refs[0]["lit"]).any(), "the NaN normal unlights pixels of its faces"
    for k in range(2):
        sel = tuple(j != k for j in range(2))
        alt = run_light(torch, h, face, bary, *args, outputs=sel)
        assert alt[1 + k] is None
        for a, b in zip(out_f, alt):
            assert b is None or np.array_equal(bits(a), bits(b))
    for k in range(3):
        sel = tuple(j != k for j in range(3))
        alt = run_light_grad(torch, api, h, face, bary, *args, G_t, outputs=sel)
        assert alt[k] is None
        for a, b in zip(out_g, alt):
            assert b is None or np.array_equal(bits(a), bits(b))
    robin = np.stack([dr.round_robin_image(len(faces), size)] * F)
    lam = junk_lambda(np.random.default_rng(3), (F, H, W))
    rf, rl = dev(torch, robin), dev(torch, lam)
    out_f = [host(o) for o in run_light(torch, h, rf, rl, *args)]
    out_g = [host(o) for o in run_light_grad(torch, api, h, rf, rl, *args, G_t)]
    check_all(frames, faces, robin, lam, normals, albedo, lights, shared, G, out_f, out_g, f"{name} hand-made images")
    h.close()


def test_cancelling_and_zero_normals(torch, api):
    """the flat scene: on a hand-made column of pixels lambda_0 = lambda_1 and the corner normals cancel EXACTLY (l = 0), face 1
    has zero normals: unlit, the albedo passes bit for bit, the gradients are G, 0 and nothing; beside the median c is large and
    the bound with it"""
    v, f, normals, intr, size = lr.flat_scene()
    H, W = size
    h = api.Raster(0, len(v), f, W, H)
    vbuf = dev(torch, v.reshape(1, -1))
    _, face, bary = render(torch, h, vbuf, 3 * len(v), 1, intr)
    torch.cuda.synchronize()
    face_h, bary_h = host(face), host(bary)
    rows = np.argwhere(face_h[0] == 0)[:6]
    assert len(rows) == 6 and (face_h[0] == 1).sum() > 5
    for (i, j) in rows:
        bary_h[0, i, j] = (0.375, 0.375, 0.25)
    albedo, light, G = inputs(np.random.default_rng(5), size, 3)
    args = (vbuf, 3 * len(v), dev(torch, normals.reshape(1, -1)), 3 * len(v), dev(torch, albedo[None]), 3, dev(torch, light), 0, 1)
    bt = dev(torch, bary_h)
    out_f = [host(o) for o in run_light(torch, h, face, bt, *args)]
    out_g = [host(o) for o in run_light_grad(torch, api, h, face, bt, *args, dev(torch, G[None]))]
    ex = check_all([v], f, face_h, bary_h, normals[None], albedo[None], [light], True, G[None], out_f, out_g, "flat scene")[0]
    for (i, j) in rows:
        assert not ex["lit"][i, j]
    assert not ex["lit"][face_h[0] == 1].any() and ex["lit"][face_h[0] == 0].sum() > 10 and ex["c"][ex["lit"]].max() > 5
    h.close()


# ---- 2. the reduction's edges ---------------------------------------------------------------------------------------------------------
def test_reduction_edges_frame_independence_and_bit_identity(torch, api):
    """One triangle over the whole image, so every chunk holds lit pixels.  The chunk is 256 P pixels with P = 1 for these sizes
    (k_light.hip's lt_layout, read through api.light_grad_layout): 67 x 45 = 3,015 pixels are 12 chunks with a ragged last one
    (199 pixels), 5 x 7 = 35 pixels are less than one wave.  A frame's grad_light and image are bit-equal between the F = 3 call
    and the F = 1 call of that frame; two identical calls are bit-equal; a NaN in G makes the coefficients of ITS frame
    non-finite and leaves the other frames' bits"""
    v0 = np.array([[-5, -5, 2], [5, -5, 2.5], [0, 8, 3]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    normals0 = np.array([[0.6, 0.0, -0.8], [0.0, 0.6, -0.8], [0.0, 0.0, -1.0]], np.float32)
    F, C = 3, 4
    for (H, W) in ((45, 67), (5, 7)):
        assert api.light_grad_layout(H * W, C, F)[:2] == (256, 12 if H == 45 else 1)
        intr = (60.0 * W / 32, 60.0 * H / 24, (W - 1) / 2, (H - 1) / 2)
        frames = [v0, (v0 * np.float32(1.1)).astype(np.float32), (v0 + np.float32([0.2, -0.1, 0.3])).astype(np.float32)]
        normals = np.stack([normals0, normals0[[1, 2, 0]], normals0[[2, 0, 1]]])
        h = api.Raster(0, 3, f, W, H)
        vbuf, nbuf = dev(torch, np.stack(frames).reshape(F, -1)), dev(torch, normals.reshape(F, -1))
        _, face, bary = render(torch, h, vbuf, 9, F, intr)
        torch.cuda.synchronize()
        rng = np.random.default_rng(H)
        albedo = rng.uniform(0.05, 1.0, (F, H, W, C)).astype(np.float32)
        G = rng.standard_normal((F, H, W, C)).astype(np.float32)
        lights = [inputs(np.random.default_rng(60 + k), (H, W), C)[1] for k in range(F)]
        lbuf = dev(torch, np.stack(lights))
        a_t, G_t = dev(torch, albedo), dev(torch, G)
        args = (vbuf, 9, nbuf, 9, a_t, C, lbuf, 9 * C, F)
        out_f = run_light(torch, h, face, bary, *args)
        out_g = run_light_grad(torch, api, h, face, bary, *args, G_t)
        refs = check_all(frames, f, host(face), host(bary), normals, albedo, lights, False, G, [host(o) for o in out_f],
                         [host(o) for o in out_g], f"{H}x{W}")
        assert all(ex["lit"].all() for ex in refs)
        again = run_light_grad(torch, api, h, face, bary, *args, G_t)
        for a, b in zip(out_g, again):
            assert np.array_equal(bits(a), bits(b)), "two identical calls are bit-equal"
        for k in range(F):
            one = (vbuf[k:k + 1].contiguous(), 9, nbuf[k:k + 1].contiguous(), 9, a_t[k:k + 1].contiguous(), C, lbuf[k:k + 1].contiguous(),
                   9 * C, 1)
            fk, bk = face[k:k + 1].contiguous(), bary[k:k + 1].contiguous()
            img1 = run_light(torch, h, fk, bk, *one)[0]
            g1 = run_light_grad(torch, api, h, fk, bk, *one, G_t[k:k + 1].contiguous())
            assert np.array_equal(bits(img1[0]), bits(out_f[0][k]))
            for a, b in zip(out_g, g1):
                assert np.array_equal(bits(a[k]), bits(b[0])), "a frame's results do not depend on the batch around it"
        Gn = G.copy()
        Gn[1, H // 2, W // 2, 2] = np.nan
        gl = host(run_light_grad(torch, api, h, face, bary, *args, dev(torch, Gn))[2])
        assert not np.isfinite(gl[1, :, 2]).any() and np.isfinite(gl[1][:, [0, 1, 3]]).all()
        assert np.array_equal(gl[[0, 2]].view(np.int32), host(out_g[2])[[0, 2]].view(np.int32))
        h.close()


# ---- 3. the vertex normals' adjoint ---------------------------------------------------------------------------------------------------
def run_normals_vjp(torch, s, vbuf, vstride, F, V, g, gstride):
    out = torch.full((F, gstride), -777.0, dtype=torch.float32, device="cuda")
    s.vertex_normals_vjp_device(ptr(vbuf), vstride, F, ptr(g), ptr(out), gstride, stream(torch))
    torch.cuda.synchronize()
    return out


def test_normals_vjp_on_every_vertex(torch, api):
    """two_spheres (subdivided twice, three poses) with padded vertex and gradient strides, and the hand mesh (a repeated-corner
    face, an isolated vertex, a vertex between two opposite faces, a NaN vertex): every vertex inside the contract; the padding
    is not written; a frame alone gives the same bits; two calls give the same bits"""
    rng = np.random.default_rng(4)
    verts, faces, _ = wr.two_spheres(2)
    base = (verts * 0.3 + [0.1, 0.0, 2.5])
    frames = [base.astype(np.float32), (base * 1.07 + [0.03, -0.02, 0.1]).astype(np.float32), (base * [-1, 1, 1]).astype(np.float32)]
    hv, hf = lr.hand_mesh()
    for label, fr, fc in (("two_spheres", frames, faces), ("hand mesh", [hv, (hv * np.float32(1.5)).astype(np.float32)], hf)):
        F, V = len(fr), len(fr[0])
        vstride, gstride = 3 * V + 13, 3 * V + 5
        vbuf = padded(torch, fr, 3 * V, vstride, -777.0)
        g = rng.standard_normal((F, V, 3)).astype(np.float32)
        s = api.Surface(0, V, fc)
        out = run_normals_vjp(torch, s, vbuf, vstride, F, V, dev(torch, g), gstride)
        got = host(out)
        assert np.all(got[:, 3 * V:] == -777.0), "the padding of the gradient's rows is not written"
        worst = 0.0
        with np.errstate(all="ignore"):
            for k in range(F):
                worst = max(worst, lr.check_normals_vjp(fr[k], fc, g[k], got[k, :3 * V].reshape(V, 3)))
        print(f"normals VJP {label}: worst {worst:.3f} of the bound")
        assert np.array_equal(bits(out), bits(run_normals_vjp(torch, s, vbuf, vstride, F, V, dev(torch, g), gstride)))
        one = run_normals_vjp(torch, s, vbuf[1:2].contiguous(), vstride, 1, V, dev(torch, g[1:2]), gstride)
        assert np.array_equal(bits(one[0]), bits(out[1]))
        if label == "hand mesh":
            gv = got[0, :3 * V].reshape(V, 3)
            assert np.isfinite(got[:, :3 * V]).all() and not gv[[4, 5, 6, 7]].any() and gv[[0, 1, 2, 3]].any(axis=1).all()
        s.close()


def test_invalid_arguments_launch_nothing_and_the_no_ops_succeed(torch, api):
    v, f, normals, intr, size = lr.flat_scene()
    H, W = size
    V = len(v)
    h = api.Raster(0, V, f, W, H)
    face = torch.full((1, H, W), -1, dtype=torch.int32, device="cuda")
    bary = torch.zeros((1, H, W, 3), device="cuda")
    vb, nb = dev(torch, v.reshape(1, -1)), dev(torch, normals.reshape(1, -1))
    al, G = torch.ones((1, H, W, 3), device="cuda"), torch.ones((1, H, W, 3), device="cuda")
    light, image = torch.ones((9, 3), device="cuda"), torch.zeros((1, H, W, 3), device="cuda")
    ok = [ptr(face), ptr(bary), ptr(vb), 3 * V, ptr(nb), 3 * V, ptr(al), 3, ptr(light), 0, 1, ptr(image), None, None]
    before = api.launch_count()
    for pos, bad in ((0, None), (1, None), (2, None), (3, 3 * V - 1), (4, None), (5, 3 * V - 1), (6, None), (7, 0), (7, 5), (8, None),
                     (9, 26), (10, -1), (11, None)):
        a = list(ok)
        a[pos] = bad
        with pytest.raises(api.BodyfitError):
            h.light_device(*a, stream(torch))
    gl, work = torch.zeros((1, 9, 3), device="cuda"), torch.zeros(api.light_grad_layout(H * W, 3, 1)[2], dtype=torch.float64, device="cuda")
    okg = ok[:11] + [ptr(G), None, None, ptr(gl), ptr(work)]
    for pos, bad in ((0, None), (7, 5), (9, 26), (10, -1), (11, None), (15, None)):
        a = list(okg)
        a[pos] = bad
        with pytest.raises(api.BodyfitError):
            h.light_grad_device(*a, stream(torch))
    s = api.Surface(0, V, f)
    gn, gv = torch.zeros((1, V, 3), device="cuda"), torch.zeros((1, V, 3), device="cuda")
    oks = [ptr(vb), 3 * V, 1, ptr(gn), ptr(gv), 3 * V]
    for pos, bad in ((0, None), (1, 3 * V - 1), (2, -1), (3, None), (4, None), (5, 3 * V - 1)):
        a = list(oks)
        a[pos] = bad
        with pytest.raises(api.BodyfitError):
            s.vertex_normals_vjp_device(*a, stream(torch))
    assert api.launch_count() == before, "an invalid call launches nothing"
    a = list(ok); a[10] = 0
    h.light_device(*a, stream(torch))
    a = list(okg); a[10] = 0
    h.light_grad_device(*a, stream(torch))
    a = list(okg); a[14] = None; a[15] = None
    h.light_grad_device(*a, stream(torch))
    a = list(oks); a[2] = 0
    s.vertex_normals_vjp_device(*a, stream(torch))
    assert api.launch_count() == before, "the no-ops launch nothing"
    s.close()
    h.close()


# ---- 4. the layer -----------------------------------------------------------------------------------------------------------------------
def lit_f64(torch, lighting, albedo64, light64, normals64, v32, faces_t, face, bary, lit):
    """[F, H, W, C] f64 of the definition at the fixed render (face, bary) on the pixels `lit` [F, H, W], albedo64 elsewhere: the
    weights in f64, the interpolated normal, sh_basis, the light [9, C] or [F, 9, C]; differentiable in albedo64, light64, normals64"""
    F, H, W = face.shape
    C = albedo64.shape[-1]
    fr, pix = torch.nonzero(lit.reshape(F, -1), as_tuple=True)
    t = face.reshape(F, -1)[fr, pix].long()
    q = bary.reshape(F, -1, 3)[fr, pix].double() / v32[fr[:, None], faces_t[t], 2].double()
    w = q / ((q[:, 0] + q[:, 1]) + q[:, 2])[:, None]
    m = (w[:, :, None] * normals64[fr[:, None], faces_t[t]]).sum(dim=1)
    b = lighting.sh_basis(m / m.norm(dim=1, keepdim=True))
    s = (b[:, :, None] * (light64[None] if light64.ndim == 2 else light64[fr])).sum(dim=1)
    flat = albedo64.reshape(F * H * W, C)
    return flat.index_put((fr * H * W + pix,), flat[fr * H * W + pix] * s).reshape(F, H, W, C)


@pytest.mark.parametrize("shared", [True, False])
def test_shade_gradients(torch, api, tl, lighting, shared):
    """lighting.shade on three_frames (a padded verts leaf): vertex_normals equals solid.vertex_normals in bits; the image and the
    gradients in albedo, light and normals against the reference's contracts and against torch f64 autograd through the same
    definition at the same face image; verts through vertex_normals within the adjoint's contract on the layer's own upstream;
    verts with interior=True (normals given: the interior part alone) within the interpolation rows' and the rows VJP's contracts
    composed on the face soup; a shared light is the f64 sum of the per-frame gradients"""
    frames, faces, intr, size = three_frames()
    H, W = size
    F, V, C = 3, len(frames[0]), 3
    rng = np.random.default_rng(90)
    albedo = rng.uniform(0.05, 1.0, (F, H, W, C)).astype(np.float32)
    up = rng.standard_normal((F, H, W, C)).astype(np.float32)
    lights = np.stack([inputs(np.random.default_rng(70 + f), size, C)[1] for f in range(F)])
    light_np = lights[0] if shared else lights
    upt = dev(torch, up)

    def leaf_verts():
        pv = torch.zeros((F, 3 * V + 5), device="cuda")[:, :3 * V].view(F, V, 3)
        pv.copy_(dev(torch, np.stack(frames)))
        return pv.requires_grad_()

    # 1. normals=None: albedo, light, and verts through the vertex normals
    leaf, a_l, l_l = leaf_verts(), dev(torch, albedo).requires_grad_(), dev(torch, light_np).requires_grad_()
    n_layer = lighting.vertex_normals(leaf, faces)
    assert np.array_equal(bits(n_layer), bits(tl.vertex_normals(leaf.detach(), faces))), "solid.vertex_normals, bit for bit"
    image = lighting.shade(a_l, leaf, faces, intr, l_l)
    (image * upt).sum().backward()
    g_verts_n = leaf.grad.clone()
    # the kernels' own outputs for the same inputs
    h = api.Raster(0, V, faces, W, H)
    vbuf = padded(torch, frames, 3 * V, 3 * V, 0.0)
    _, face, bary = render(torch, h, vbuf, 3 * V, F, intr)
    normals_t = n_layer.detach().contiguous()
    lbuf = dev(torch, light_np)
    args = (vbuf, 3 * V, normals_t.reshape(F, -1), 3 * V, dev(torch, albedo), C, lbuf, 0 if shared else 9 * C, F)
    k_image = run_light(torch, h, face, bary, *args)[0]
    k_ga, k_gm, k_gl = run_light_grad(torch, api, h, face, bary, *args, upt)
    weight = run_shade(torch, h, face, bary, vbuf, 3 * V, normals_t.reshape(F, -1), 3 * V, 3, F, [0.0])[1]
    assert np.array_equal(bits(image), bits(k_image)) and np.array_equal(bits(a_l.grad), bits(k_ga))
    want_l = k_gl.double().sum(dim=0).to(torch.float32) if shared else k_gl
    assert np.array_equal(bits(l_l.grad), bits(want_l)), "a shared light: the f64 sum of the per-frame gradients, rounded once"
    face_h, bary_h, normals_h, weight_h, gm_h = host(face), host(bary), host(normals_t), host(weight), host(k_gm)
    refs = check_all(frames, faces, face_h, bary_h, normals_h, albedo, [light_np] if shared else list(lights), shared, up,
                     [host(k_image), None, None], [host(k_ga), gm_h, host(k_gl)], f"layer shared={shared}")
    lit = dev(torch, np.stack([ex["lit"] for ex in refs]))
    # torch f64 autograd through the same definition
    a64 = torch.tensor(albedo, device="cuda", dtype=torch.float64, requires_grad=True)
    l64 = torch.tensor(light_np, device="cuda", dtype=torch.float64, requires_grad=True)
    n64 = normals_t.double().requires_grad_()
    faces_t = dev(torch, faces.astype(np.int64))
    ref_img = lit_f64(torch, lighting, a64, l64, n64, vbuf.view(F, V, 3), faces_t, face, bary, lit)
    (ref_img * upt.double()).sum().backward()
    lim_i = np.stack([lr.light_bound(ex)[0] for ex in refs]).astype(np.float64)
    assert np.all(np.abs(host(ref_img.detach()) - host(image.detach()).astype(np.float64)) <= lim_i + 1e-13)
    for f in range(F):
        ga, gm, gl, lim_a, lim_m, sum_tb, sum_tc = lr.grad_exact(refs[f], up[f])
        assert np.all(np.abs(host(a64.grad)[f] - ga.astype(np.float64)) <= 1e-12 * (1 + np.abs(ga.astype(np.float64))))
        if not shared:
            assert np.all(np.abs(host(l64.grad)[f] - gl.astype(np.float64)) <= 1e-11 * (1 + sum_tb.astype(np.float64)))
    if shared:
        err = np.abs(host(l_l.grad).astype(np.float64) - host(l64.grad))
        tot = sum(lr.grad_exact(refs[f], up[f])[5] for f in range(F)).astype(np.float64)
        assert np.all(err <= 2 * U * tot), "the shared light's gradient against autograd: the stores' u on sum |t b|"
    # 2. normals given: the gradient in the normals, and verts through the interior alone
    leaf2, n_l = leaf_verts(), normals_t.clone().requires_grad_()
    img2 = lighting.shade(dev(torch, albedo), leaf2, faces, intr, dev(torch, light_np), normals=n_l, interior=True)
    assert np.array_equal(bits(img2), bits(k_image))
    (img2 * upt).sum().backward()
    leaf3, n_l3 = leaf_verts(), normals_t.clone().requires_grad_()
    img3 = lighting.shade(dev(torch, albedo), leaf3, faces, intr, dev(torch, light_np), normals=n_l3,
                          render=tl.render_depth(leaf3, faces, intr, size))
    (img3 * upt).sum().backward()
    assert leaf3.grad is None and np.array_equal(bits(n_l3.grad), bits(n_l.grad)) and np.array_equal(bits(img3), bits(k_image))
    got_n = host(n_l.grad)
    worst_n = 0.0
    for f in range(F):
        Gf, Tf = dr.vjp_exact(faces, V, face_h[f].reshape(-1), weight_h[f].reshape(-1, 3), np.ones(H * W, np.float32),
                              gm_h[f].reshape(-1, 3))
        bound = (dr.K_VJP + 1) * U * Tf + 2.0 ** -140
        assert np.all(np.abs(got_n[f].astype(LD) - Gf) <= bound), "the normals' gradient is the exact sum of its rows within the rows VJP's contract"
        lim_m = lr.grad_exact(refs[f], up[f])[4].reshape(-1, 3)
        Bs = np.zeros((V, 3), LD)
        keep = face_h[f].reshape(-1) >= 0
        for a in range(3):
            np.add.at(Bs, faces[face_h[f].reshape(-1)[keep], a], weight_h[f].reshape(-1, 3)[keep, a:a + 1].astype(LD) * lim_m[keep])
        err = np.abs(got_n[f].astype(LD) - host(n64.grad)[f].astype(LD))
        lim = bound + Bs + 64 * lr.EPS * Tf + 2 * U * Tf       # (the stored weights are within 2 u of the f64 ones autograd uses)
        assert np.all(err <= lim), (f, float((err[Tf > 0] / lim[Tf > 0]).max()))
        if (Tf > 0).any():
            worst_n = max(worst_n, float((err[Tf > 0] / lim[Tf > 0]).max()))
        assert np.all(got_n[f][Tf == 0] == 0)
    # verts through the vertex normals: the adjoint's contract on the layer's own upstream (the gradient in the normals)
    worst_v = 0.0
    for f in range(F):
        worst_v = max(worst_v, lr.check_normals_vjp(frames[f], faces, got_n[f], host(g_verts_n)[f]))
    # verts through the interior: autograd through sum_a beta_a(verts) n_a with the kernel's pixel gradients upstream
    v64 = torch.tensor(np.stack(frames), device="cuda", dtype=torch.float64, requires_grad=True)
    live = (weight != 0).any(dim=-1)
    fr, pix = torch.nonzero(live.reshape(F, -1), as_tuple=True)
    t = face.reshape(F, -1)[fr, pix].long()
    beta = beta_f64(torch, v64, faces_t, intr, W, fr, pix, t)
    m_pix = (beta[:, :, None] * normals_t.double()[fr[:, None], faces_t[t]]).sum(dim=1)
    (m_pix * k_gm.reshape(F, -1, 3)[fr, pix].double()).sum().backward()
    soup_f = np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)
    want, gv = host(v64.grad), host(leaf2.grad)
    worst_i = 0.0
    for f in range(F):
        pixf = np.nonzero((weight_h[f] != 0).any(axis=-1).reshape(-1))[0]
        with np.errstate(all="ignore"):
            ref = ir.InterpRows(frames[f][faces].reshape(-1, 3), soup_f, intr, size, face_h[f], pixf, normals_h[f][faces].reshape(-1, 3),
                                gm_h[f], None)
        assert not ref.void.any()
        Gx, bnd, Tx = (np.zeros((V, 3)) for _ in range(3))
        for src, dst in zip(ir.composed_gradient(ref, soup_f, 3 * len(faces)), (Gx, bnd, Tx)):
            np.add.at(dst, faces.reshape(-1), src)
        tol64 = 16 * (ref.kappa_d.max() + ref.rows.kappa_b.max() + 64 * 2.0 ** -29) * U * Tx
        err = np.abs(gv[f].astype(np.float64) - want[f])
        lim_v = bnd + tol64
        assert np.all(err <= lim_v), (f, float((err[Tx > 0] / lim_v[Tx > 0]).max()))
        if f < 2:
            worst_i = max(worst_i, float((err[Tx > 0] / lim_v[Tx > 0]).max()))
        assert np.all(gv[f][Tx == 0] == 0)
    assert float(g_verts_n.abs().max()) > 0 and float(leaf2.grad.abs().max()) > 0
    print(f"lighting.shade shared={shared}: normals worst {worst_n:.3f}, verts (normals) {worst_v:.3f}, verts (interior) {worst_i:.3f} "
          f"of their bounds")
    h.close()


def test_argument_errors(torch, lighting):
    frames, faces, intr, size = three_frames()
    H, W = size
    v = dev(torch, np.stack(frames))
    F, V = v.shape[:2]
    albedo, light = torch.ones((F, H, W, 3), device="cuda"), torch.ones((9, 3), device="cuda")
    with pytest.raises(TypeError):
        lighting.shade(albedo.double(), v, faces, intr, light)
    with pytest.raises(TypeError):
        lighting.shade(albedo, v, faces, intr, light.cpu())
    with pytest.raises(ValueError):
        lighting.shade(albedo[:2], v, faces, intr, light)
    with pytest.raises(ValueError):
        lighting.shade(albedo, v, faces, intr, torch.ones((8, 3), device="cuda"))
    with pytest.raises(ValueError):
        lighting.shade(albedo, v, faces, intr, torch.ones((2, 9, 3), device="cuda"))
    with pytest.raises(ValueError):
        lighting.shade(albedo, v, faces, intr, light, normals=torch.ones((F, V + 1, 3), device="cuda"))
    with pytest.raises(ValueError):
        lighting.shade(albedo, v, faces, intr, light, render=(None, None))
    with pytest.raises(ValueError):
        lighting.shade(albedo, v, faces, intr[:3], light)
    with pytest.raises(ValueError):
        lighting.LitPhotometricTerm(albedo, intr, faces, uv=torch.zeros((4, 2), device="cuda"))
    term = lighting.LitPhotometricTerm(albedo, intr, faces)
    with pytest.raises(ValueError):
        term.mipmaps()
    with pytest.raises(ValueError):
        term(v, torch.ones((V, 4), device="cuda"), light)
    with pytest.raises(ValueError):
        term(v, torch.ones((V, 3), device="cuda"), torch.ones((9, 4), device="cuda"))


# ---- 5. the fit ---------------------------------------------------------------------------------------------------------------------------
def test_a_light_is_fitted_and_the_unlit_term_cannot_move(torch, tl, lighting):
    """lighting_ref.fit_scene: two_spheres in three poses, vertex colours, a target rendered with a light that has a strong
    directional part.  From the ambient-only start, FIT_STEPS plain gradient steps in the light with LitPhotometricTerm
    (antialias off: the restatement is per pixel), at the rate 1 / trace of the Hessian.  The same steps in torch f64 (the
    definition through sh_basis at the same render, from the same f32 albedo image and normals) end below FIT_FRACTION of the
    starting cost, and the layer's final light is within 4 x FIT_STORE_DIFF of theirs: FIT_STORE_DIFF is the largest difference
    between the f32-store restatement and the f64 one measured on the CPU (tests/test_lighting.py: 5.65e-8), the factor 4 the
    margin for the GPU's different summation chunks.  RenderedPhotometricTerm on the same target has no light to move: its cost
    is the same at every step while the lit term's falls: the reason for the feature"""
    verts, faces, intr, size, colours = lr.fit_scene()
    H, W = size
    F, V, C = 3, verts.shape[1], 3
    v, col = dev(torch, verts), dev(torch, colours)
    true_l, start = dev(torch, lr.FIT_LIGHT), dev(torch, lr.FIT_START)
    with torch.no_grad():
        A, face = tl.render_attributes(v, faces, intr, size, col)
        target = lighting.shade(A, v, faces, intr, true_l)
    term = lighting.LitPhotometricTerm(target, intr, faces, antialias=False)
    ev = term.evaluate(v, col, true_l)
    assert float(ev["cost"]) == 0.0 and ev["shading"].shape == (F, H, W, C)
    lit = (ev["shading"] != 0).any(dim=-1)
    # the restatement's ingredients, from the layer's own render: the f32 albedo image, the normals, the weights in f64
    normals = lighting.vertex_normals(v, faces)
    _, face2, bary = tl.render_depth(v, faces, intr, size)
    faces_t = dev(torch, faces.astype(np.int64))

    def image64(light64):
        return lit_f64(torch, lighting, A.double(), light64, normals.double(), v, faces_t, face2, bary, lit)

    # the rate, as lighting_ref.fit_rate states it
    with torch.no_grad():
        fr, pix = torch.nonzero(lit.reshape(F, -1), as_tuple=True)
        t = face2.reshape(F, -1)[fr, pix].long()
        q = bary.reshape(F, -1, 3)[fr, pix].double() / v[fr[:, None], faces_t[t], 2].double()
        w = q / ((q[:, 0] + q[:, 1]) + q[:, 2])[:, None]
        m = (w[:, :, None] * normals.double()[fr[:, None], faces_t[t]]).sum(dim=1)
        b = lighting.sh_basis(m / m.norm(dim=1, keepdim=True))
        a2 = (A.double().reshape(-1, C)[fr * H * W + pix] ** 2).max(dim=-1).values
        rate = float(1.0 / (2.0 * (a2 * (b * b).sum(dim=-1)).sum()))
    light = start.clone().requires_grad_()
    l64 = start.double().clone().requires_grad_()
    unlit = tl.RenderedPhotometricTerm(target, intr, faces, antialias=False)
    costs, costs64, flat = [], [], []
    for _ in range(lr.FIT_STEPS):
        cost = term(v, col, light)
        cost.backward()
        costs.append(float(cost.detach()))
        c64 = (image64(l64) - target.double()).square().sum()
        c64.backward()
        costs64.append(float(c64.detach()))
        flat.append(float(unlit(v, col)))
        with torch.no_grad():
            light -= rate * light.grad
            l64 -= rate * l64.grad
        light.grad = None
        l64.grad = None
    final64 = float((image64(l64.detach()) - target.double()).square().sum())
    diff = float((light.detach().double() - l64.detach()).abs().max())
    print(f"fit: cost {costs[0]:.4f} -> {float(term(v, col, light.detach())):.4f}; restated {costs64[0]:.4f} -> {final64:.4f} "
          f"({final64 / costs64[0]:.4f} of the start); |layer - f64| of the final light {diff:.2e} (allowed {4 * FIT_STORE_DIFF:.2e}); "
          f"the unlit term stays at {flat[0]:.4f}")
    assert final64 < FIT_FRACTION * costs64[0]
    assert diff <= 4 * FIT_STORE_DIFF
    assert costs[-1] < FIT_FRACTION * costs[0], "the lit term's cost falls with the restatement's"
    assert flat[0] > 0 and all(c == flat[0] for c in flat), "without a light to move, the unlit term's cost stays where it is"
    # with antialias and the vertices: the term reaches verts through the albedo, the shading and coverage
    term_aa = lighting.LitPhotometricTerm(target, intr, faces)
    vl = v.clone().requires_grad_()
    term_aa(vl, col, start).backward()
    assert vl.grad is not None and bool(torch.isfinite(vl.grad).all()) and float(vl.grad.abs().max()) > 0
