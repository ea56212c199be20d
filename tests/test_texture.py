"""UV textures without a GPU: the ABI is declared, exported and bound; the mirrored constants are the header's; the kernels'
operation order, restated in f64, meets the contracts of include/bodyfit.h against the definition in longdouble on every pixel and
every texel of every scene; hand-made uv tables (outside [0, 1], huge, NaN, on texel centres and cell borders, faces of one uv); the
adjoint identity; the integer sums do not depend on the order; the scale's worst case; the uv gradient against central differences."""
import importlib
import inspect
import os

import numpy as np
import pytest

import depth_rows_ref as dr
import interp_ref as ir
import raster_ref as rr
import texture_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 5), (64, 64))       # (Ht, Wt)
CHANNELS = (1, 3, 4)
ATLASES = ("charts", "cylinder")
FD_SIZES = ((7, 5), (64, 64))      # the atlas inset 0.13 keeps every uv out of their clamped border, 1 / (2 x 5) wide at most
FD_BORDER = 1e-6
FD_CAP = 0.01


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module("3dbodyanimation_amd.synth")


@pytest.fixture(scope="module")
def scenes(synth):
    """name -> (scene, the kernel-form render (face, bary), {atlas kind: (uv, uv_faces, Pixels, pixels_f64)}): computed once"""
    out = {}
    with np.errstate(all="ignore"):
        for name, sc in dr.row_scenes(synth).items():
            v, f, intr, size, z_near, cull = sc
            _, face, bary = rr.kernel_form_f64(v, f, intr, size, z_near, cull)
            atl = {}
            for kind in ATLASES:
                uv, uvf = synth.make_uv_atlas(f, kind, verts=v)
                atl[kind] = (uv, uvf, tr.Pixels(face, bary, v, f, uv, uvf), tr.pixels_f64(face, bary, v, f, uv, uvf))
            out[name] = (sc, face, bary, atl)
    return out


def test_the_functions_are_declared_exported_and_bound(api):
    lib = api.load_library()
    for name, n_args in (("bodyfit_raster_texture_device", 20), ("bodyfit_raster_texture_grad_device", 20),
                         ("bodyfit_raster_interp_rows_indexed_device", 24)):
        assert name in api.declared_symbols()
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args
    for m in ("texture_device", "texture_grad_device", "interp_rows_indexed_device"):
        assert hasattr(api.Raster, m)
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    assert inspect.signature(tl.render_texture).parameters["interior"].default is False
    assert issubclass(tl.TexturedPhotometricTerm, tl.torch.nn.Module) and callable(tl.bake_texture)
    assert "k_texture.hip" in open(os.path.join(ROOT, "3dbodyanimation_amd", "csrc", "Makefile")).read()


def test_the_mirrored_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "bodyfit.h")).read()
    ks, kt, unit, delta, kg = tr.header_constants(text)
    assert (ks, kt, 2.0 ** -unit, 2.0 ** -delta, kg) == (tr.K_S, tr.K_T, tr.KAPPA_UNIT, tr.DELTA_SHIFT, tr.K_G)


def test_the_atlases(synth):
    v, f, _, _ = rr.two_spheres()
    for kind in ATLASES:
        uv, uvf = synth.make_uv_atlas(f, kind, verts=v)
        assert uv.dtype == np.float32 and uvf.dtype == np.int32 and uvf.shape == f.shape
        assert uvf.min() >= 0 and uvf.max() < len(uv) and uv.min() >= 0.13 and uv.max() <= 0.87
        span = uv[uvf].max(axis=1) - uv[uvf].min(axis=1)
        assert span.max() < 0.5, "no face wraps around the atlas"
    uv, uvf = synth.make_uv_atlas(f, "charts")
    assert len(uv) == 3 * len(f)
    uv, uvf = synth.make_uv_atlas(f, "cylinder", verts=v)
    assert len(v) < len(uv) < 2 * len(v), "the seam's vertices are duplicated, the others are not"
    with pytest.raises(ValueError):
        synth.make_uv_atlas(f, "cylinder")


def test_the_kernel_form_meets_the_contract_on_every_pixel(scenes):
    """every scene, both atlases, C = 1, 3, 4, u8 and f32, every texture size: the image, the weights and uv; the weights are the
    shade's bit for bit; on 7 x 5 also the gradients in uv and in the texels"""
    import appearance_ref as ar
    worst = {"image": 0.0, "grad_uv": 0.0, "grad_tex": 0.0}
    for name, (sc, face, bary, atl) in scenes.items():
        v, f, _, size, _, _ = sc
        shade_w = ar.shade_kernel_form_f64(face, bary, v, f, np.zeros((len(v), 1), np.float32), 0.0)[1]
        for kind, (uv, uvf, px, pf) in atl.items():
            assert np.array_equal(pf["w"].astype(np.float32), shade_w), "the weights are the shade's, bit for bit"
            for (Ht, Wt) in SIZES:
                for C in CHANNELS:
                    for tk in (0, 1):
                        tex = tr.make_texture(Ht, Wt, C, tk)
                        bg = np.arange(1, C + 1, dtype=np.float32) * 0.25
                        with np.errstate(all="ignore"):
                            lk, form = tr.Lookup(px, tex), tr.lookup_f64(pf, tex, bg)
                        worst["image"] = max(worst["image"], tr.check_forward(lk, form, bg, form["image"], form["weight"], form["uv"]))
                        if (Ht, Wt) == (7, 5):
                            G = np.random.default_rng(C).standard_normal(size + (C,)).astype(np.float32)
                            gu = np.stack(((G * form["du"]).sum(-1) * Wt * form["free_x"], (G * form["dv"]).sum(-1) * Ht * form["free_y"]), -1)
                            worst["grad_uv"] = max(worst["grad_uv"], tr.check_grad_uv(lk, form, G, gu.astype(np.float32)))
                            gt, _, _ = tr.accumulate_f64([form], G[None], tex.shape, True)
                            worst["grad_tex"] = max(worst["grad_tex"], tr.check_grad_tex([form], G[None], tex.shape, True, gt))
    print(f"worst errors of the f64 restatement in units of their bounds: {worst}")
    assert all(w <= 1.0 for w in worst.values())


def _hand_scene():
    """one frontal quad of two faces over a 16 x 16 image, rendered by the kernel form: every pixel of columns 2 .. 10 is covered"""
    sc = rr.hand_scenes()["shared_edge"]
    v, f, intr, size, z_near, cull = sc
    _, face, bary = rr.kernel_form_f64(v, f, intr, size, z_near, cull)
    return v, f, size, face, bary


def test_hand_made_uv_tables():
    """uv outside [0, 1] and +-1e30 clamp to the border texels and never index outside; a NaN voids the pixels of its faces; an
    out-of-range uv_faces entry voids its face; x and y exactly on texel centres and cell borders"""
    v, f, size, face, bary = _hand_scene()
    tex = tr.make_texture(4, 8, 3, 1)
    bg = np.float32(-7.0)
    tables = {
        "outside": np.array([[-0.5, -0.25], [1.5, -0.25], [1.5, 1.75], [-0.5, 1.75]], np.float32),
        "huge": np.array([[-1e30, -1e30], [1e30, -1e30], [1e30, 1e30], [-1e30, 1e30]], np.float32),
        # the quad spans pixels 2 .. 10: 8 pixels; 8 texels wide -> x = j - 2 - 1/2 + ..., on texel centres with this offset
        "centres": np.array([[0.5 / 8, 0.5 / 4], [8.5 / 8, 0.5 / 4], [8.5 / 8, 4.5 / 4], [0.5 / 8, 4.5 / 4]], np.float32),
    }
    for name, uv in tables.items():
        px, pf = tr.Pixels(face, bary, v, f, uv, f), tr.pixels_f64(face, bary, v, f, uv, f)
        with np.errstate(all="ignore"):
            lk, form = tr.Lookup(px, tex), tr.lookup_f64(pf, tex, bg)
        tr.check_forward(lk, form, bg, form["image"], form["weight"], form["uv"])
        live = form["ok"]
        assert live.sum() > 40
        for k, n in (("i0", 4), ("i1", 4), ("j0", 8), ("j1", 8)):
            assert form[k].min() >= 0 and form[k].max() < n
        if name == "huge":
            # every pixel off the diagonal's exact cancellation lands on a border texel, and the clamp is active both ways
            corner = np.isin(form["x"][live], (0.0, 7.0)) & np.isin(form["y"][live], (0.0, 3.0))
            assert corner.mean() > 0.9 and not (form["free_x"] & form["free_y"])[live][corner].any()
        if name == "centres":
            # integer texel coordinates: the value is the texel itself, from the cell to its left or its own
            xi = form["x"][live]
            assert (xi == np.round(xi)).mean() > 0.9
            on = live & (form["x"] == np.round(form["x"])) & (form["y"] == np.round(form["y"]))
            want = tex[form["y"][on].astype(int), form["x"][on].astype(int)]
            assert on.sum() > 20 and np.array_equal(form["image"][on], want)
    # NaN in one uv row: the faces that use it are void, the others are not
    uv = tables["centres"].copy()
    uv[1, 0] = np.nan                                   # vertex 1 belongs to face 0 = (0, 2, 1) only
    pf = tr.pixels_f64(face, bary, v, f, uv, f)
    px = tr.Pixels(face, bary, v, f, uv, f)
    assert np.array_equal(pf["ok"], ~px.void) and not pf["ok"][face == 0].any() and pf["ok"][face == 1].all()
    # an out-of-range entry voids its face
    uvf = f.copy()
    uvf[1, 2] = 4
    pf = tr.pixels_f64(face, bary, v, f, tables["centres"], uvf)
    assert pf["ok"][face == 0].all() and not pf["ok"][face == 1].any()
    uvf[1, 2] = -1
    assert not tr.pixels_f64(face, bary, v, f, tables["centres"], uvf)["ok"][face == 1].any()


def test_faces_of_one_uv_have_rows_whose_attribute_part_is_exactly_zero(scenes):
    """interp rows with per-corner attributes are the plain rows of the face soup (corner k of face t -> vertex 3 t + k, attr row
    uv[uv_faces[t][k]]); where a face's three uv rows are equal, s_0 = s_1 = s_2 and dir is EXACTLY 0"""
    sc, face, bary, atl = scenes["two_spheres"]
    v, f, intr, size, _, _ = sc
    uv, uvf = (a.copy() for a in atl["charts"][:2])
    flat = np.arange(0, len(f), 3)
    uvf[flat] = uvf[flat, :1]                                 # every third face: one uv row for its three corners
    soup_v, soup_f = v[f].reshape(-1, 3), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)
    G = np.random.default_rng(0).standard_normal(size + (2,)).astype(np.float32)
    index, beta, direction, _ = ir.kernel_form_f64(soup_v, soup_f, intr, size, face, None, uv[uvf].reshape(-1, 2), G, None)
    one = np.isin(index, flat)
    assert one.sum() > 500 and np.all(direction[one] == 0.0)
    assert np.abs(direction[(index >= 0) & ~one]).max() > 0
    # the soup's rows are the mesh's, bit for bit: index and beta do not depend on the attributes
    i2, b2, _, _ = ir.kernel_form_f64(v, f, intr, size, face, None, np.zeros((len(v), 2), np.float32), G, None)
    assert np.array_equal(index, i2) and np.array_equal(beta, b2)


def _frames(scenes, name, kind, tex, n_frames=3):
    """n_frames copies of a scene's restated lookup with per-frame upstream gradients"""
    sc, face, bary, atl = scenes[name]
    pf = atl[kind][3]
    form = tr.lookup_f64(pf, tex, 0.0)
    G = np.random.default_rng(5).standard_normal((n_frames,) + sc[3] + (tex.shape[2],)).astype(np.float32)
    return [form] * n_frames, G


def test_the_adjoint_identity(scenes):
    """sum G . image(tex) = sum g_tex . tex within the two contracts, for a texture-linear image (background 0)"""
    for (Ht, Wt) in ((1, 1), (7, 5), (64, 64)):
        tex = tr.make_texture(Ht, Wt, 3, 1)
        forms, G = _frames(scenes, "two_spheres", "cylinder", tex)
        gt, _, _ = tr.accumulate_f64(forms, G, tex.shape, True)
        g_star, m, A = tr.grad_tex_exact(forms, G, tex.shape, True)
        s, _ = tr.scale_exponent(G, G.size // 3)
        live = forms[0]["ok"]
        lhs = sum((G[k].astype(LD) * forms[k]["image"].astype(LD))[live].sum() for k in range(len(forms)))
        rhs = (gt.astype(LD) * tex.astype(LD)).sum()
        # image^ is within u |B| + 8 eps M of sum omega tex at the returned point; g^ within (b) of g*
        M = np.abs(tex).max()
        tol = sum((np.abs(G[k]).astype(LD) * (tr.U * np.abs(forms[k]["image"]) + 8 * tr.EPS * M))[live].sum() for k in range(len(forms)))
        tol += ((tr.U * np.abs(g_star) + m * np.ldexp(LD(1), -(s + 1)) + tr.K_G * tr.EPS * A) * np.abs(tex)).sum()
        assert abs(lhs - rhs) <= tol, (Ht, Wt, float(abs(lhs - rhs)), float(tol))
        assert abs(lhs) > 1e3 * tol or Ht == 1


def test_the_integer_sums_do_not_depend_on_the_order(scenes):
    tex = tr.make_texture(7, 5, 3, 1)
    forms, G = _frames(scenes, "two_spheres", "charts", tex)
    g0, s0, _ = tr.accumulate_f64(forms, G, tex.shape, True)
    n = G.size // 3 * 12
    g1, s1, _ = tr.accumulate_f64(forms, G, tex.shape, True, order=np.random.default_rng(1).permutation(n))
    assert np.array_equal(s0, s1) and np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    # the frames reversed, and per-frame textures permute with their frames
    g2, s2, _ = tr.accumulate_f64(forms[::-1], G[::-1], tex.shape, True)
    assert np.array_equal(s0, s2)
    g3, _, _ = tr.accumulate_f64(forms, G, tex.shape, False)
    g4, _, _ = tr.accumulate_f64(forms[::-1], G[::-1], tex.shape, False)
    assert np.array_equal(g3, g4[::-1])
    assert np.array_equal(tr.accumulate_f64(forms, 0 * G, tex.shape, True)[0], np.zeros(tex.shape, np.float32))
    Gn = G.copy(); Gn[1, 3, 4, 0] = np.nan
    assert np.isnan(tr.accumulate_f64(forms, Gn, tex.shape, True)[0]).all()


def test_the_scale_keeps_the_worst_case_below_2_to_the_62():
    """every pixel on ONE texel (a 1 x 1 texture: the four texels of the cell coincide) at |G| = Gmax: the integer sum stays below
    2^62 with s, and the a-priori bound 4 N 2^(E + s) that guarantees it would not with the next larger scale s + 1 (the next
    SMALLER one only loses bits)"""
    for N in (1, 2, 3, 255, 256, 12345, 2 ** 21, 2 ** 31 - 1, 2 ** 38 + 17):
        for gmax in (np.float32(1.0), np.float32(0.99999994), np.float32(3.4e38), np.float32(1e-45), np.float32(2.0 ** -126), np.float32(5.5)):
            s, gbits = tr.scale_exponent(np.array([gmax, -gmax / 2], np.float32), N)
            E = (gbits >> 23) - 126
            assert float(gmax) < 2.0 ** E and (gbits >> 23 == 0 or float(gmax) >= 2.0 ** (E - 1))
            assert abs(s) <= 186
            # omega = (1, 0, 0, 0) at every pixel: N contributions of rint(Gmax 2^s) into one element
            q = int(np.rint(np.ldexp(np.float64(gmax), s)))
            assert E + s == 60 - N.bit_length() >= 21
            assert N * q < 2 ** 62 and 4 * N * 2 ** (E + s) < 2 ** 62
            assert 4 * N * 2 ** (E + s + 1) >= 2 ** 62
            # a NORMAL maximum is at least 2^(E - 1): it keeps 59 - B >= 20 bits (a subnormal one, below 2^-126, may round away)
            assert gbits >> 23 == 0 or q >= 2 ** (59 - N.bit_length())


def _bilinear_ld(tex, x, y):
    """B at texel coordinates (x, y) (clamped here), longdouble"""
    import appearance_ref as ar
    Ht, Wt, _ = tex.shape
    x, y = np.clip(x, 0, Wt - 1), np.clip(y, 0, Ht - 1)
    j0, _ = ar._cell(np.floor(x), Wt)
    i0, _ = ar._cell(np.floor(y), Ht)
    return ar._patch(tex, i0, j0, x, y)[0]


def test_the_uv_gradient_is_the_central_difference_of_the_definition(scenes):
    """sum_c G_c dimage_c/d(u, v) of the f64 restatement against central differences of the longdouble lookup.  Pixels within 1e-6
    texels of a cell border or on an active clamp are left out of THIS comparison; their share stays under 1 % (the atlas inset keeps
    uv out of the clamped border of these textures)"""
    h = LD(2.5e-7)
    for (Ht, Wt) in FD_SIZES:
        tex = tr.make_texture(Ht, Wt, 3, 1)
        for kind in ATLASES:
            n_live = n_out = 0
            for name, (sc, face, bary, atl) in scenes.items():
                uv, uvf, px, pf = atl[kind]
                with np.errstate(all="ignore"):
                    lk, form = tr.Lookup(px, tex), tr.lookup_f64(pf, tex, 0.0)
                live = ~px.void
                G = np.random.default_rng(2).standard_normal(sc[3] + (3,)).astype(np.float32)
                frac = lambda c: c - np.floor(c)
                near = lambda c: (frac(c) < FD_BORDER) | (frac(c) > 1 - FD_BORDER)
                out = live & (near(lk.xr) | near(lk.yr) | ~lk.free_x | ~lk.free_y)
                n_live, n_out = n_live + int(live.sum()), n_out + int(out.sum())
                use = (live & ~out).reshape(-1)
                x, y, Gf = lk.xr.reshape(-1)[use], lk.yr.reshape(-1)[use], G.reshape(-1, 3)[use].astype(LD)
                fd_u = (Gf * (_bilinear_ld(tex, x + h, y) - _bilinear_ld(tex, x - h, y))).sum(-1) / (2 * h) * Wt
                fd_v = (Gf * (_bilinear_ld(tex, x, y + h) - _bilinear_ld(tex, x, y - h))).sum(-1) / (2 * h) * Ht
                got_u = ((G * form["du"]).sum(-1) * Wt).reshape(-1)[use]
                got_v = ((G * form["dv"]).sum(-1) * Ht).reshape(-1)[use]
                scale = max(Wt, Ht) * 2.0 * np.abs(Gf).sum(-1)            # |texel| <= 2
                # (the difference quotient of a function that is LINEAR in x between the two points: only longdouble rounding, 2^-63 / h)
                assert np.all(np.abs(got_u - fd_u) <= 1e-9 * scale) and np.all(np.abs(got_v - fd_v) <= 1e-9 * scale), (name, kind, Ht, Wt)
            print(f"{kind} {Ht}x{Wt}: {n_out} of {n_live} live pixels left out of the comparison")
            assert n_live > 20000 and n_out < FD_CAP * n_live
