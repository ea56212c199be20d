"""GPU: the interpolation rows (bodyfit_raster_interp_rows_device, k_raster_rows.hip), their sum through the rows VJP,
torch_layer.render_attributes(interior=True) and RenderedPhotometricTerm.

The kernel is checked against the extended-precision reference of its contract (interp_ref.py) on EVERY row; the layer against torch
f64 autograd through sum_a beta_a(verts) A_a at the same fixed face image, within the contracts composed by the reference."""
import importlib

import numpy as np
import pytest

import antialias_ref as aa
import appearance_ref as ar
import depth_rows_ref as dr
import interp_ref as ir
import raster_ref as rr
from test_gpu_antialias import restatement
from test_gpu_appearance import host, padded, ptr, render, run_shade, stream, three_poses
from test_gpu_depth_rows import SCENES, run_rows, three_frames

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def tl():
    return importlib.import_module("3dbodyanimation_amd.torch_layer")


@pytest.fixture(scope="module")
def scenes(synth):
    return dr.row_scenes(synth)


def run_interp(torch, h, vbuf, vstride, F, intr, face_img, pixel=None, offset=None, abuf=None, astride=0, C=0, G=None, gz=None,
               outputs=(True, True, True), n_rows=None):
    """(index, bary, direction, value) of the kernel, the outputs pre-filled with junk; every argument a torch tensor or None"""
    N = F * h.height * h.width if pixel is None else (pixel.numel() if n_rows is None else n_rows)
    index = torch.full((N,), -9, dtype=torch.int32, device="cuda")
    bary = torch.full((N, 3), -3.0, dtype=torch.float32, device="cuda") if outputs[0] else None
    direction = torch.full((N, 3), float("nan"), dtype=torch.float32, device="cuda") if outputs[1] else None
    value = torch.full((N, max(C, 1)), float("nan"), dtype=torch.float32, device="cuda")[:, :C].contiguous() if outputs[2] and C else None
    h.interp_rows_device(ptr(vbuf), vstride, F, intr, ptr(face_img), ptr(pixel), ptr(offset), N, ptr(abuf), astride, C, ptr(G), ptr(gz),
                         ptr(index), ptr(bary), ptr(direction), ptr(value), stream(torch))
    torch.cuda.synchronize()
    return index, bary, direction, value


def check_frame(verts, faces, intr, size, image, pixel, attr, G, gz, out, sl, label):
    with np.errstate(all="ignore"):
        ref = ir.InterpRows(verts, faces, intr, size, image, pixel, attr, G, gz)
    w = ir.check_rows(ref, *[None if o is None else o[sl] for o in out])
    keep = ~ref.void
    print(f"interp rows {label}: {int(keep.sum())} of {len(ref.pix)} rows live; worst beta {w[0]:.2f}, dir {w[1]:.2f}, value {w[2]:.2f} "
          f"of their bounds (largest kappa_d {np.max(ref.kappa_d[keep], initial=0):.2e})")
    return ref


# ---- 1. the contract, every row ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [0, 1, 3, 4])
@pytest.mark.parametrize("name", SCENES)
def test_rows_contract_on_every_row(torch, api, scenes, name, C):
    """F = 3 (the second frame holds a NaN and an infinite corner, the third lies behind the camera), a padded and poisoned vertex
    stride, junk-filled outputs; attributes shared (C = 1, 4) or per frame with a padded stride (C = 3), one of them NaN (C = 3):
    all-pixel rows of the scene's own render and of a hand-made round-robin image, and a ragged list over the render"""
    verts, faces, intr, size, z_near, cull = scenes[name]
    H, W = size
    V, F = len(verts), 3
    robin = np.stack([dr.round_robin_image(len(faces), size)] * F)
    addressed = np.unique(robin[(robin >= 0) & (robin < len(faces))])
    frames = three_poses(verts, faces[[addressed.min(), addressed.max()]])
    h = api.Raster(0, V, faces, W, H)
    vstride = 3 * V + 13
    vbuf = padded(torch, frames, 3 * V, vstride, -777.0)
    shared = C != 3
    attr = G = abuf = Gt = None
    astride = 0
    gzs = np.stack([ir.inputs(V, size, 0, seed=f)[2] for f in range(F)])
    if C:
        attr = np.stack([ir.inputs(V, size, C, seed=10 + f)[0] for f in range(1 if shared else F)])
        if C == 3:
            attr[1, faces[addressed[len(addressed) // 2]][0], 1] = np.nan
        G = np.stack([ir.inputs(V, size, C, seed=f)[1] for f in range(F)])
        astride = 0 if shared else V * C + 11
        abuf = padded(torch, list(attr), V * C, V * C + 11, np.nan)
        Gt = torch.tensor(G, device="cuda")
    gzt = torch.tensor(gzs, device="cuda")
    _, face, _ = render(torch, h, vbuf, vstride, F, intr, z_near, cull)
    fh = host(face)
    lists = [np.concatenate([np.arange(0, H * W, 3), [-1, H * W, H * W + 5, 2 ** 31 - 1, -2 ** 31]]), np.zeros(0, np.int64),
             np.random.default_rng(4).integers(0, H * W, size=min(3000, 4 * H * W))]
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
    pixel = torch.tensor(np.concatenate(lists).astype(np.int32), device="cuda")
    offset = torch.tensor(off, device="cuda")
    n_nan = 0
    for label, img_t, img_h, px, of, with_z in (("render", face, fh, None, None, True), ("hand-made", torch.tensor(robin, device="cuda"), robin, None, None, C in (0, 3)),
                                                ("ragged", face, fh, pixel, offset, C == 0)):
        out = [host(o) for o in run_interp(torch, h, vbuf, vstride, F, intr, img_t, px, of, abuf, astride, C, Gt, gzt if with_z else None)]
        for f in range(F):
            if px is not None and off[f] == off[f + 1]:
                continue
            sl = slice(H * W * f, H * W * (f + 1)) if px is None else slice(off[f], off[f + 1])
            a_f = None if not C else attr[0 if shared else f]
            ref = check_frame(frames[f], faces, intr, size, img_h[f], None if px is None else lists[f], a_f, None if not C else G[f],
                              gzs[f] if with_z else None, out, sl, f"{name} C={C} {label} frame {f}")
            if label == "render":
                assert np.array_equal(out[0][sl] >= 0, ~ref.void)
            with np.errstate(invalid="ignore"):
                n_nan += int((~np.isfinite(out[2][sl]).all(axis=1) & (out[0][sl] >= 0)).sum())
        if label == "hand-made":
            # index and beta are the depth rows', bit for bit
            di, _, db, _ = run_rows(torch, h, vbuf, vstride, F, intr, img_t)
            assert np.array_equal(out[0], host(di)) and np.array_equal(out[1].view(np.int32), host(db).view(np.int32))
    # (check_rows asserts it row by row: a NaN attribute keeps its rows and makes their directions NaN, nothing else is NaN)
    assert n_nan > 0 if (C == 3 and name == "two_spheres") else (n_nan == 0 or C == 3)
    h.close()


@pytest.mark.parametrize("name", ["two_spheres", "big_and_small", "soup_at_0.9m", "hand_slanted", "grazing", "sliver"])
def test_value_against_the_shade(torch, api, scenes, name):
    """d_value against bodyfit_raster_shade_device's image at every pixel the shade does not void, within the header's composed
    bound: the rows' own, the shade's k_s u T_ch (T_ch <= V_ch + 5 tau_t R_t A_ch) and the render's 5 tau_t R_t A_ch"""
    verts, faces, intr, size, z_near, cull = scenes[name]
    H, W = size
    V, C = len(verts), 3
    h = api.Raster(0, V, faces, W, H)
    vbuf = padded(torch, [verts], 3 * V, 3 * V, 0.0)
    attr, G, _ = ir.inputs(V, size, C, seed=2)
    abuf = torch.tensor(attr, device="cuda")
    _, face, bary = render(torch, h, vbuf, 3 * V, 1, intr, z_near, cull)
    image, weight = run_shade(torch, h, face, bary, vbuf, 3 * V, abuf, 0, C, 1, [0.0] * C)
    out = [host(o) for o in run_interp(torch, h, vbuf, 3 * V, 1, intr, face, None, None, abuf, 0, C, torch.tensor(G[None], device="cuda"))]
    fh = host(face)[0]
    with np.errstate(all="ignore"):
        ref = ir.InterpRows(verts, faces, intr, size, fh, None, attr, G, None)
        Fc = rr.Faces(verts, faces, intr, size, z_near, cull)
    shaded = (host(weight)[0] != 0).any(axis=-1).reshape(-1)
    assert shaded.sum() > 50 and np.array_equal(shaded, fh.reshape(-1) >= 0) and np.all(out[0][shaded] >= 0)
    t = fh.reshape(-1)[shaded]
    tr = (Fc.tau[t] * Fc.R[t])[:, None]
    assert np.all(tr <= 1.0 / 16)
    lim = ref.value_tol[shaded] + ar.K_S * U * (ref.V[shaded] + ir.SHADE_TAU * tr * ref.A[shaded]) + ir.SHADE_TAU * tr * ref.A[shaded]
    err = np.abs(out[3][shaded].astype(np.float64) - host(image)[0].reshape(-1, C)[shaded].astype(np.float64))
    print(f"interp value against the shade, {name}: {int(shaded.sum())} shaded pixels, worst {float((err / lim).max()):.2f} of the summed "
          f"contracts, {float((err / np.maximum(ref.V[shaded], 1e-30)).max() / U):.2f} u of V")
    assert np.all(err <= lim), float((err / lim).max())
    h.close()


# ---- 2. addressing, determinism ------------------------------------------------------------------------------------------------------
def test_uniform_lists_null_outputs_two_runs_and_a_frame_alone(torch, api):
    """F = 3 with a padded stride and per-frame attributes: a uniform list of 500 pixels per frame within the contract; two runs are
    bit-identical; NULL outputs leave the others bit-identical; frame 2 of the F = 3 call is the frame run alone"""
    frames, faces, intr, size = three_frames()
    H, W = size
    V, F, C = len(frames[0]), 3, 3
    h = api.Raster(0, V, faces, W, H)
    vstride = 3 * V + 13
    vbuf = padded(torch, frames, 3 * V, vstride, -777.0)
    _, face, _ = render(torch, h, vbuf, vstride, F, intr)
    fh = host(face)
    attr = np.stack([ir.inputs(V, size, C, seed=20 + f)[0] for f in range(F)])
    G = np.stack([ir.inputs(V, size, C, seed=f)[1] for f in range(F)])
    gzs = np.stack([ir.inputs(V, size, 0, seed=f)[2] for f in range(F)])
    abuf = padded(torch, list(attr), V * C, V * C + 7, np.nan)
    Gt, gzt = torch.tensor(G, device="cuda"), torch.tensor(gzs, device="cuda")
    rng = np.random.default_rng(6)
    uni = rng.integers(0, H * W, size=(F, 500)).astype(np.int32)
    ut = torch.tensor(uni, device="cuda")
    full = run_interp(torch, h, vbuf, vstride, F, intr, face, ut, None, abuf, V * C + 7, C, Gt, gzt)
    out = [host(o) for o in full]
    for f in range(F):
        ref = check_frame(frames[f], faces, intr, size, fh[f], uni[f], attr[f], G[f], gzs[f], out, slice(500 * f, 500 * f + 500), f"uniform, frame {f}")
        assert (~ref.void).sum() > 20
    again = run_interp(torch, h, vbuf, vstride, F, intr, face, ut, None, abuf, V * C + 7, C, Gt, gzt)
    for a, b in zip(full, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # (bits: a NaN would not equal itself)
    for outputs in ((False, False, False), (True, False, True), (False, True, False)):
        part = run_interp(torch, h, vbuf, vstride, F, intr, face, ut, None, abuf, V * C + 7, C, Gt, gzt, outputs=outputs)
        for a, b in zip(full, part):
            assert b is None or torch.equal(a.view(torch.int32), b.view(torch.int32))
    v2 = padded(torch, [frames[2]], 3 * V, 3 * V, 0.0)
    alone = run_interp(torch, h, v2, 3 * V, 1, intr, face[2:3].contiguous(), ut[2:3].contiguous(), None, torch.tensor(attr[2], device="cuda"),
                       V * C, C, Gt[2:3].contiguous(), gzt[2:3].contiguous())
    for a, b in zip(full, alone):
        assert torch.equal(a[1000:1500].view(torch.int32), b.view(torch.int32))
    allpix = run_interp(torch, h, vbuf, vstride, F, intr, face, None, None, abuf, V * C + 7, C, Gt, gzt)
    for a, b in zip(full, allpix):
        for f in range(F):
            pick = torch.tensor(uni[f].astype(np.int64) + f * H * W, device="cuda")
            assert torch.equal(a[500 * f:500 * f + 500].view(torch.int32), b[pick].view(torch.int32))
    h.close()


def test_invalid_arguments_launch_nothing_and_the_no_ops_succeed(torch, api):
    verts, faces, intr, size = rr.two_spheres()
    H, W = size
    V, C, N = len(verts), 3, 6
    h = api.Raster(0, V, faces, W, H)
    vbuf = padded(torch, [verts], 3 * V, 3 * V, 0.0)
    _, face, _ = render(torch, h, vbuf, 3 * V, 1, intr)
    attr = torch.zeros((V, C), device="cuda")
    G = torch.zeros((1, H, W, C), device="cuda")
    gz = torch.zeros((1, H, W), device="cuda")
    pixel = torch.zeros(N, dtype=torch.int32, device="cuda")
    off = torch.tensor([0, N], dtype=torch.int32, device="cuda")
    index = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    bary, direction, value = (torch.full((N, 3), -3.0, device="cuda") for _ in range(3))
    good = dict(d_verts_ptr=ptr(vbuf), verts_frame_stride=3 * V, n_frames=1, intr=intr, d_face_image_ptr=ptr(face), d_pixel_ptr=ptr(pixel),
                d_offset_ptr=ptr(off), n_rows=N, d_attr_ptr=ptr(attr), attr_frame_stride=0, n_channels=C, d_grad_image_ptr=ptr(G),
                d_grad_z_ptr=ptr(gz), d_index_ptr=ptr(index), d_bary_ptr=ptr(bary), d_dir_ptr=ptr(direction), d_value_ptr=ptr(value),
                stream=stream(torch))
    before = api.launch_count()
    for change in [dict(n_frames=-1), dict(n_rows=-1), dict(intr=(0.0, 300.0, 64.0, 64.0)), dict(intr=(300.0, -1.0, 64.0, 64.0)),
                   dict(intr=(300.0, 300.0, float("inf"), 64.0)), dict(intr=(300.0, 300.0, 64.0, float("nan"))),
                   dict(d_pixel_ptr=None), dict(d_pixel_ptr=None, d_offset_ptr=None), dict(n_frames=4, d_offset_ptr=None),
                   dict(n_rows=2 ** 31 - 4096), dict(n_frames=0), dict(d_face_image_ptr=None), dict(d_index_ptr=None),
                   dict(d_verts_ptr=None), dict(verts_frame_stride=3 * V - 1), dict(n_channels=-1), dict(n_channels=5),
                   dict(d_attr_ptr=None), dict(d_grad_image_ptr=None), dict(attr_frame_stride=C * V - 1),
                   dict(n_channels=0, d_grad_z_ptr=None), dict(n_channels=0, d_attr_ptr=None, d_grad_image_ptr=None, d_grad_z_ptr=None)]:
        with pytest.raises(api.BodyfitError, match="status 1"):
            h.interp_rows_device(**{**good, **change})
    lib = api.load_library()
    assert lib.bodyfit_raster_interp_rows_device(None, ptr(vbuf), 3 * V, 1, 300.0, 300.0, 64.0, 64.0, ptr(face), ptr(pixel), ptr(off), N,
                                                 ptr(attr), 0, C, ptr(G), ptr(gz), ptr(index), ptr(bary), ptr(direction), ptr(value), None) == 1
    assert api.launch_count() == before
    torch.cuda.synchronize()
    assert bool((index == -7).all()) and bool((bary == -3.0).all()) and bool((direction == -3.0).all()) and bool((value == -3.0).all())
    # the no-ops, the optional inputs and outputs, a topology without faces
    h.interp_rows_device(**{**good, "n_frames": 0, "n_rows": 0, "d_index_ptr": None})
    h.interp_rows_device(**{**good, "n_rows": 0, "d_index_ptr": None, "d_pixel_ptr": ptr(pixel), "d_offset_ptr": None})
    assert api.launch_count() == before
    h.interp_rows_device(**{**good, "d_grad_z_ptr": None, "d_bary_ptr": None, "d_value_ptr": None})
    h.interp_rows_device(**{**good, "n_channels": 0, "d_attr_ptr": None, "d_grad_image_ptr": None, "d_value_ptr": None})
    assert api.launch_count() == before + 2
    none = api.Raster(0, V, np.zeros((0, 3), np.int32), W, H)
    none.interp_rows_device(**{**good, "d_verts_ptr": None})
    torch.cuda.synchronize()
    assert bool((index == -1).all()) and bool((bary == 0).all()) and bool((direction == 0).all()) and bool((value == 0).all())
    h.close()
    none.close()


# ---- 3. through the rows VJP ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_spheres", "grazing", "sliver"])
def test_rows_through_the_rows_vjp(torch, api, scenes, name):
    """every row of the render through bodyfit_surface_rows_vjp_device with coef = 1: the VJP's own contract for THESE f32 rows, and
    the exact vertex gradient of sum G . I + g_z z within the two contracts composed, every component"""
    verts, faces, intr, size, z_near, cull = scenes[name]
    H, W = size
    V, C = len(verts), 3
    h = api.Raster(0, V, faces, W, H)
    s = api.Surface(0, V, faces)
    vbuf = padded(torch, [verts], 3 * V, 3 * V, 0.0)
    attr, G, gz = ir.inputs(V, size, C, seed=3)
    _, face, _ = render(torch, h, vbuf, 3 * V, 1, intr, z_near, cull)
    index, bary, direction, _ = run_interp(torch, h, vbuf, 3 * V, 1, intr, face, None, None, torch.tensor(attr, device="cuda"), 0, C,
                                           torch.tensor(G[None], device="cuda"), torch.tensor(gz[None], device="cuda"))
    coef = torch.ones(H * W, device="cuda")
    g = torch.full((1, 3 * V + 7), -777.0, device="cuda")
    rows = api.PointSet.uniform(index.data_ptr(), H * W, 3 * H * W)
    s.rows_vjp_device(rows, 1, H * W, ptr(index), ptr(bary), ptr(coef), ptr(direction), ptr(g), 3 * V + 7, stream(torch))
    torch.cuda.synchronize()
    assert bool((g[:, 3 * V:] == -777.0).all())
    got = host(g)[0, :3 * V].reshape(V, 3)
    w = dr.check_vjp(faces, V, host(index), host(bary), host(coef), host(direction), got)
    with np.errstate(all="ignore"):
        ref = ir.InterpRows(verts, faces, intr, size, host(face)[0], None, attr, G, gz)
    Gx, bound, T = ir.composed_gradient(ref, faces, V)
    err = np.abs(got.astype(np.float64) - Gx)
    assert (T > 0).sum() >= 9 and np.all(got[T == 0] == 0)
    print(f"interp rows through the rows VJP, {name}: {int((~ref.void).sum())} rows, {int((T > 0).any(axis=1).sum())} vertices; the VJP "
          f"{w:.3f} of 2 u T, the composition {float((err[T > 0] / bound[T > 0]).max()):.3f} of its bound (bound / T up to "
          f"{float((bound[T > 0] / T[T > 0]).max()):.2e})")
    assert np.all(err <= bound), float((err[T > 0] / bound[T > 0]).max())
    h.close()


# ---- 4. the layer ---------------------------------------------------------------------------------------------------------------------
def beta_f64(torch, v64, faces_t, intr, W, frame, pix, index):
    """the object-space barycentrics [N, 3] of the pixels' rays in their faces, torch f64, differentiable in v64 [F, V, 3]"""
    fx, fy, cx, cy = intr
    c = v64[frame[:, None], faces_t[index]]
    n = torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    d = torch.stack((((pix % W).double() - cx) / fx, ((pix // W).double() - cy) / fy, torch.ones_like(pix, dtype=torch.float64)), dim=1)
    z = (n * c[:, 0]).sum(dim=1) / (n * d).sum(dim=1)
    x = z[:, None] * d
    nn = (n * n).sum(dim=1)
    return torch.stack([(n * torch.linalg.cross(c[:, (a + 1) % 3] - x, c[:, (a + 2) % 3] - x)).sum(dim=1) / nn for a in range(3)], dim=1)


def shaded_f64(torch, v64, a64, faces_t, intr, face, background):
    """[F, H, W, C] f64: sum_a beta_a(v64) a64[corner a] where face >= 0, the background elsewhere; a64 [V, C] or [F, V, C]"""
    F, H, W = face.shape
    fr, pix = torch.nonzero(face.reshape(F, -1) >= 0, as_tuple=True)
    t = face.reshape(F, -1)[fr, pix].long()
    beta = beta_f64(torch, v64, faces_t, intr, W, fr, pix, t)
    ids = faces_t[t]
    A = a64[ids] if a64.ndim == 2 else a64[fr[:, None], ids]
    val = (beta[:, :, None] * A).sum(dim=1)
    C = a64.shape[-1]
    out = torch.as_tensor(background, dtype=torch.float64, device=v64.device).expand(C).repeat(F * H * W, 1)
    return out.index_put((fr * H * W + pix,), val).reshape(F, H, W, C)


@pytest.mark.parametrize("C,shared", [(3, False), (4, True)])
def test_render_attributes_interior(torch, api, tl, C, shared):
    """interior=True: the image and the attribute gradient are bit-identical to interior=False; the gradient in verts (a padded
    leaf) against torch f64 autograd through sum beta(verts) A at the same face image, every component, within the rows' and the
    rows VJP's contracts composed; interior=False leaves verts.grad None"""
    frames, faces, intr, size = three_frames()
    H, W = size
    F, V = 3, len(frames[0])
    rng = np.random.default_rng(70 + C)
    attr = rng.uniform(-1.0, 2.0, size=(V, C) if shared else (F, V, C)).astype(np.float32)
    up = rng.standard_normal((F, H, W, C)).astype(np.float32)
    upt = torch.tensor(up, device="cuda")
    grads, images = [], []
    for interior in (False, True):
        pv = torch.zeros((F, 3 * V + 5), device="cuda")[:, :3 * V].view(F, V, 3)
        pv.copy_(torch.tensor(np.stack(frames), device="cuda"))
        leaf = pv.requires_grad_()                                        # a leaf whose frames are 3 V + 5 floats apart
        a = torch.tensor(attr, device="cuda").requires_grad_()
        image, face = tl.render_attributes(leaf, faces, intr, size, a, background=0.5, interior=interior)
        (image * upt).sum().backward()
        grads.append((leaf.grad, a.grad))
        images.append((image.detach(), face))
    assert grads[0][0] is None and grads[1][0] is not None and grads[1][0].shape == (F, V, 3)
    assert torch.equal(images[0][0].view(torch.int32), images[1][0].view(torch.int32)) and torch.equal(images[0][1], images[1][1])
    assert torch.equal(grads[0][1].view(torch.int32), grads[1][1].view(torch.int32))
    gv, face = host(grads[1][0]), images[1][1]
    fh = host(face)
    faces_t = torch.tensor(faces.astype(np.int64), device="cuda")
    v64 = torch.tensor(np.stack(frames), device="cuda", dtype=torch.float64, requires_grad=True)
    a64 = torch.tensor(attr, device="cuda", dtype=torch.float64)
    (shaded_f64(torch, v64, a64, faces_t, intr, face, 0.5) * upt.double()).sum().backward()
    want = host(v64.grad)
    for f in range(F):
        pix = np.nonzero(fh[f].reshape(-1) >= 0)[0]
        with np.errstate(all="ignore"):
            ref = ir.InterpRows(frames[f], faces, intr, size, fh[f], pix, attr if shared else attr[f], up[f], None)
        assert not ref.void.any()                    # (a rendered face has an area and meets the ray: the shade's list is the rows')
        Gx, bound, T = ir.composed_gradient(ref, faces, V)
        # the f64 restatement against the reference: f64 is 2^-29 u, and kappa_d, kappa_b are what an f64 evaluation loses, in u
        tol64 = 16 * (ref.kappa_d.max() + ref.rows.kappa_b.max() + 64 * 2.0 ** -29) * U * T
        assert np.all(np.abs(want[f] - Gx) <= tol64)
        err = np.abs(gv[f].astype(np.float64) - want[f])
        print(f"render_attributes(interior=True) C={C} frame {f}: {len(pix)} rows, {int((T > 0).any(axis=1).sum())} vertices with a gradient, "
              f"worst {float((err[T > 0] / bound[T > 0]).max()):.3f} of the composed bound (gradient up to {float(np.abs(Gx).max()):.2e})")
        assert np.all(err <= bound + tol64) and np.all(gv[f][T == 0] == 0) and (T > 0).sum() > 300


def test_wall_interior_gradients_lower_a_dense_image_loss(torch, tl):
    """A wall that overhangs the image on all sides, colours a smooth function of the rest position, moved by 0.4 pixel: no
    silhouette is in sight, so interior=False leaves verts.grad None; with interior=True the gradient is non-zero and 20 plain
    gradient steps of one fixed length (0.05 pixel for the largest first gradient) lower the cost"""
    rest, moved, faces, intr, size, colours = ir.wall_scene(0.4)
    cols = torch.tensor(colours, device="cuda")
    with torch.no_grad():
        target, face = tl.render_attributes(torch.tensor(rest[None], device="cuda"), faces, intr, size, cols)
    assert bool((face >= 0).all())

    def cost_of(x, interior):
        image, _ = tl.render_attributes(x, faces, intr, size, cols, interior=interior)
        return (image.double() - target.double()).square().sum()

    leaf = torch.tensor(moved[None], device="cuda").requires_grad_()
    cols.requires_grad_()
    c0 = cost_of(leaf, False)
    c0.backward()
    assert leaf.grad is None and cols.grad is not None
    cols.requires_grad_(False)
    c0 = c0.detach()
    cost_of(leaf, True).backward()
    g0 = leaf.grad.clone()
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    px = lambda x: float(((x - torch.tensor(rest[None], device="cuda"))[..., :2].norm(dim=-1) * intr[0] / 2.0).mean())
    step = 0.05 * 2.0 / intr[0] / float(g0.abs().max())
    x = torch.tensor(moved[None], device="cuda")
    cost_0, err_0 = float(c0), px(x)
    for _ in range(20):
        xl = x.clone().requires_grad_()
        cost_of(xl, True).backward()
        x = (x - step * xl.grad).contiguous()
    cost_20 = float(cost_of(x, False))
    print(f"wall, 20 plain gradient steps: cost {cost_0:.6f} -> {cost_20:.6f}; mean vertex error {err_0:.4f} -> {px(x):.4f} pixel")
    assert cost_20 < cost_0


def neighbours_sum(e):
    """[H, W, C]: per pixel the sum of e over its four neighbours"""
    out = np.zeros_like(e)
    out[:, 1:] += e[:, :-1]; out[:, :-1] += e[:, 1:]
    out[1:] += e[:-1]; out[:-1] += e[1:]
    return out


def test_rendered_photometric_term(torch, api, tl):
    """RenderedPhotometricTerm on two_spheres moved by 0.4 pixel against its own unmoved antialiased render as the video.  The torch
    f64 restatement at the same correspondence (the face image, the reference's blended pairs): sum_a beta_a(verts) colour_a inside
    the faces, the definition's blend on top.  The cost within what the shade's, the render's and the blend's contracts let the
    image move; both gradients, every component, against the restatement linearised at the layer's own upstream, within the
    contracts of the edge rows, the interpolation rows, the transposed blend and the rows VJP composed."""
    verts, faces, intr, size = rr.two_spheres()
    H, W = size
    V, C = len(verts), 3
    bg = [0.25, -0.5, 0.75]
    rng = np.random.default_rng(8)
    colours = rng.uniform(0.0, 2.0, size=(V, C)).astype(np.float32)
    cols = torch.tensor(colours, device="cuda")
    moved = verts.astype(np.float64).copy()
    moved[:, 0] += 0.4 * moved[:, 2] / intr[0]
    moved = moved.astype(np.float32)
    with torch.no_grad():
        v0 = torch.tensor(verts[None], device="cuda")
        video = tl.antialias(tl.render_attributes(v0, faces, intr, size, cols, background=bg)[0], v0, faces, intr)
    term = tl.RenderedPhotometricTerm(video, intr, faces, background=bg)
    leaf = torch.tensor(moved[None], device="cuda").requires_grad_()
    cl = cols.clone().requires_grad_()
    e = term.evaluate(leaf, cl)
    assert e["cost"].dtype == torch.float64 and e["image"].shape == (1, H, W, C)
    e["cost"].backward()
    cost = float(e["cost"].detach())
    with torch.no_grad():
        shaded, face2 = tl.render_attributes(leaf.detach(), faces, intr, size, cols, background=bg)
        w_gpu = tl.edge_weights(leaf.detach(), faces, intr, size)
    assert torch.equal(face2, e["face"])
    fh, dh, Sg, Rg, wh, I = host(e["face"])[0], host(e["depth"])[0], host(shaded)[0], host(e["image"].detach())[0], host(w_gpu)[0], host(video)[0]
    E = aa.Edges(moved, faces, intr, size, fh, dh)
    assert E.census()[3] == 0
    aa.check_weights(E, wh)
    aa.check_blend(wh, Sg, Rg)                                                   # the term's image IS the blend of the shaded image
    pix = np.nonzero(fh.reshape(-1) >= 0)[0]
    with np.errstate(all="ignore"):
        Fc = rr.Faces(moved, faces, intr, size)
    tr = np.zeros((H * W, 1))
    tr[pix] = (Fc.tau[fh.reshape(-1)[pix]] * Fc.R[fh.reshape(-1)[pix]])[:, None]
    # ---- the cost, against the restatement
    faces_t = torch.tensor(faces.astype(np.int64), device="cuda")
    v64 = torch.tensor(moved[None], device="cuda", dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(colours, device="cuda", dtype=torch.float64, requires_grad=True)
    S64 = shaded_f64(torch, v64, c64, faces_t, intr, e["face"], bg)
    R64 = restatement(torch, v64, S64, faces, intr, [E], W)
    cost64 = float((R64 - video.double()).square().sum().detach())
    with np.errstate(all="ignore"):
        unit = ir.InterpRows(moved, faces, intr, size, fh, pix, colours, np.ones((H, W, C), np.float32), None)
    Vc, Ac = np.zeros((H * W, C)), np.zeros((H * W, C))
    Vc[pix], Ac[pix] = unit.V, unit.A
    e_S = (ar.K_S * U * (Vc + ir.SHADE_TAU * tr * Ac) + ir.SHADE_TAU * tr * Ac + unit.rows.kappa_b.max() * U * Ac).reshape(H, W, C)
    _, Tb = aa.blend_exact(E.w_ref, Sg)
    e_R = 3 * e_S + 0.5 * neighbours_sum(e_S) + aa.K_B * U * Tb.astype(np.float64) * (1 + 2.0 ** -20) + aa.blend_slack(E.tau_w, Sg)
    d = np.abs(Rg.astype(np.float64) - I.astype(np.float64))
    cost_tol = float((2 * d * e_R + e_R ** 2).sum()) + 1e-12 * cost64
    print(f"RenderedPhotometricTerm: cost {cost:.9e} against {cost64:.9e} in f64 (bound {cost_tol:.2e}); {len(pix)} covered pixels, "
          f"{len(E.hits)} blended pairs")
    assert abs(cost - cost64) <= cost_tol and cost > 1.0
    # ---- the gradients: the restatement linearised at the upstream and the shaded image the layer's backward saw
    up = (2.0 * (Rg.astype(np.float64) - I.astype(np.float64))).astype(np.float32)
    upt = torch.tensor(up[None], device="cuda").double()
    S_at = shaded.double() + (S64 - S64.detach())
    (restatement(torch, v64, S_at, faces, intr, [E], W) * upt).sum().backward()
    want_v, want_c = host(v64.grad)[0], host(c64.grad)
    # coverage: the edge rows of the blended pairs
    codes = aa.pair_codes(wh)
    ref_aa = aa.exact_rows(E, codes, Sg, up)
    G_aa, B_aa = aa.vertex_gradient(faces, V, ref_aa)
    T_aa = np.zeros((V, 3))
    live = ref_aa[0] >= 0
    np.add.at(T_aa, np.asarray(faces, np.int64)[ref_aa[0][live], ref_aa[1][live]], np.abs((ref_aa[2][live, None] * ref_aa[3][live]).astype(np.float64)))
    # interior: the upstream of the shaded image is the transposed blend of up by the layer's f32 weights, within the blend's contract
    adj, T_adj = aa.blend_exact(wh, up, transpose=True)
    G32 = adj.astype(np.float32)
    dG = (aa.K_B * U * T_adj.astype(np.float64) + U * np.abs(adj).astype(np.float64)).astype(np.float32) * np.float32(1 + 2.0 ** -20)
    with np.errstate(all="ignore"):
        ref_in = ir.InterpRows(moved, faces, intr, size, fh, pix, colours, G32, None)
        ref_dG = ir.InterpRows(moved, faces, intr, size, fh, pix, colours, dG, None)
    G_in, B_in, T_in = ir.composed_gradient(ref_in, faces, V)
    B_up = np.zeros((V, 3))
    ids = np.asarray(faces, np.int64)[ref_in.face]
    babs = np.abs(ref_in.beta).astype(np.float64) + ref_in.rows.b_tol[:, None]
    for a in range(3):
        np.add.at(B_up, ids[:, a], (babs[:, a] * ref_dG.T1)[:, None] * np.ones(3))
    exact_v = (G_aa + G_in.astype(LD)).astype(np.float64)
    tol64 = 16 * (ref_in.kappa_d.max() + ref_in.rows.kappa_b.max() + 64 * 2.0 ** -29) * U * (T_in + T_aa) + B_up
    # the restatement blends by the reference's weights, the layer by its f32 ones (within tau_w): that moves the interior upstream
    slack_w = aa.blend_slack(E.tau_w, up)
    with np.errstate(all="ignore"):
        ref_sw = ir.InterpRows(moved, faces, intr, size, fh, pix, colours, (slack_w * (1 + 2.0 ** -20)).astype(np.float32), None)
    B_w = np.zeros((V, 3))
    for a in range(3):
        np.add.at(B_w, ids[:, a], (babs[:, a] * ref_sw.T1)[:, None] * np.ones(3))
    assert np.all(np.abs(want_v - exact_v) <= tol64 + B_w + 1e-11 * T_aa)
    got_v = host(leaf.grad)[0]
    # the two f32 gradients are added in f32
    lim = (1 + dr.K_VJP * U) * B_aa + dr.K_VJP * U * T_aa + B_in + B_up + 2 * U * (np.abs(G_aa).astype(np.float64) + np.abs(G_in) + B_aa + B_in + B_up)
    err = np.abs(got_v.astype(np.float64) - want_v)
    touched = (T_in + T_aa) > 0
    print(f"RenderedPhotometricTerm, vertex gradient: {int(touched.any(axis=1).sum())} vertices, worst "
          f"{float((err[touched] / (lim + B_w + tol64)[touched]).max()):.3f} of the composed bound (bound / T up to "
          f"{float(((lim + B_w)[touched] / (T_in + T_aa)[touched]).max()):.2e}); interior share of |gradient| "
          f"{float(np.abs(G_in).sum() / (np.abs(G_in).sum() + np.abs(G_aa).astype(np.float64).sum())):.2f}")
    assert np.all(err <= lim + B_w + tol64) and np.all(got_v[~touched] == 0) and touched.sum() > 300
    # colours: sum over the shaded pixels of w_a G_int, w the shade's stored weights (within 5 tau_t R_t + k_s u of beta), by the rows VJP
    T_c, lim_c = np.zeros((V, C)), np.zeros((V, C))
    g_abs = np.abs(G32.reshape(-1, C)[pix]).astype(np.float64)
    dg = dG.reshape(-1, C)[pix].astype(np.float64) + slack_w.reshape(-1, C)[pix]
    dw = (ir.SHADE_TAU * tr[pix] + ar.K_S * U) * np.ones((1, 3)) + ref_in.rows.b_tol[:, None]
    b = np.abs(ref_in.beta).astype(np.float64)
    for a in range(3):
        np.add.at(T_c, ids[:, a], b[:, a:a + 1] * g_abs)
        np.add.at(lim_c, ids[:, a], dw[:, a:a + 1] * (g_abs + dg) + b[:, a:a + 1] * dg)
    lim_c = lim_c + (dr.K_VJP + 2) * U * (T_c + lim_c)
    got_c = host(cl.grad)
    err_c = np.abs(got_c.astype(np.float64) - want_c)
    print(f"RenderedPhotometricTerm, colour gradient: {int((T_c > 0).any(axis=1).sum())} vertices, worst "
          f"{float((err_c[T_c > 0] / lim_c[T_c > 0]).max()):.3f} of the composed bound (bound / T up to {float((lim_c[T_c > 0] / T_c[T_c > 0]).max()):.2e})")
    assert np.all(err_c <= lim_c + 1e-11 * T_c) and np.all(got_c[T_c == 0] == 0)
    # ---- trunc, a mask, u8 images, no antialiasing
    mask = torch.zeros((1, H, W), dtype=torch.bool, device="cuda")
    mask[:, : H // 2] = True
    sq = host(e["sq"].detach())[0]
    trunc = float(np.sqrt(np.median(sq[sq > 0])))
    et = tl.RenderedPhotometricTerm(video, intr, faces, trunc=trunc, background=bg, mask=mask).evaluate(leaf.detach(), cols)
    keep = sq[: H // 2]
    assert int(et["n_truncated"]) == int((keep > trunc * trunc).sum()) > 0
    assert abs(float(et["cost"]) - float(np.minimum(keep, trunc * trunc).sum())) <= 1e-12 * float(keep.sum())
    v8 = (video * 100).clamp(0, 255).to(torch.uint8)
    a8 = tl.RenderedPhotometricTerm(v8, intr, faces, background=bg, antialias=False)
    b8 = tl.RenderedPhotometricTerm(v8.float(), intr, faces, background=bg, antialias=False)
    assert float(a8(leaf.detach(), cols)) == float(b8(leaf.detach(), cols))
    assert torch.equal(a8.evaluate(leaf.detach(), cols)["image"].view(torch.int32), shaded.view(torch.int32))
    # ---- printed, not asserted: 20 plain gradient steps from the 0.4-pixel shift, beside antialias alone
    def descend(interior):
        def cost_of(x):
            if interior:
                return term(x, cols)
            img = tl.antialias(tl.render_attributes(x, faces, intr, size, cols, background=bg)[0], x, faces, intr)
            return (img.double() - video.double()).square().sum()
        x = torch.tensor(moved[None], device="cuda")
        xl = x.clone().requires_grad_()
        cost_of(xl).backward()
        step = 0.05 * float(moved[:, 2].mean()) / intr[0] / float(xl.grad.abs().max())
        for _ in range(20):
            xl = x.clone().requires_grad_()
            cost_of(xl).backward()
            x = (x - step * xl.grad).contiguous()
        return float(cost_of(x))
    print(f"20 plain gradient steps from the 0.4-pixel shift: cost {cost:.6f} -> {descend(True):.6f} with the interior gradients, "
          f"-> {descend(False):.6f} with antialias alone")
