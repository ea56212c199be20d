"""Depth rows and the rows VJP without a GPU: the ABI is declared, exported and bound; the closed form beta_a m of the header IS
the derivative of the exact ray-plane depth; the kernel's operation order, restated in f64, meets the rows contract on every row of
every scene; the thresholds of the DepthResidualTerm scene keep their distance from every row."""
import importlib
import os
import re

import numpy as np
import pytest

import depth_rows_ref as dr
import raster_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.fixture(scope="module")
def scenes():
    """name -> (scene, the kernel-form render's face image): computed once"""
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    out = {}
    with np.errstate(all="ignore"):
        for name, sc in dr.row_scenes(synth).items():
            v, f, intr, size, z_near, cull = sc
            out[name] = (sc, rr.kernel_form_f64(v, f, intr, size, z_near, cull)[1])
    return out


def test_both_functions_are_declared_exported_and_bound(api):
    syms = api.declared_symbols()
    lib = api.load_library()
    for name, n_args in (("bodyfit_raster_depth_rows_device", 17), ("bodyfit_surface_rows_vjp_device", 11)):
        assert name in syms, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert hasattr(api.Raster, "depth_rows_device") and hasattr(api.Surface, "rows_vjp_device")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    assert callable(tl.depth_at_pixels) and issubclass(tl.DepthResidualTerm, tl.torch.nn.Module)
    assert "NOT differentiable" in tl.render_depth.__doc__ and "depth_at_pixels" in tl.render_depth.__doc__


def test_the_mirrored_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "bodyfit.h")).read()
    k, a, b, v = dr.header_constants(text)
    assert (k, 2.0 ** -a, 2.0 ** -b, v) == (dr.K, dr.KAPPA_SHIFT, dr.KAPPA_B_SHIFT, dr.K_VJP)
    assert re.search(r"kappa >= 2\^24", text) and dr.KAPPA_VOID == 2.0 ** 24


def test_beta_m_is_the_derivative_of_the_exact_depth(scenes):
    """A central difference, in longdouble, of the exact ray-plane depth at the fixed face against beta_a m_c.  Moving ONE corner
    coordinate by t makes n . v0 and n . d linear in t, so z(t) = (N0 + a t) / (D + b t): with cd the central difference, s2 the
    second difference and q = h s2 / (2 cd) = -b h / D, cd (1 - q^2) = z'(0) exactly.  The step's truncation is therefore
    |cd| q^2 = (h |s2| / 2) |q|, taken as (h |s2| / 2) min(1, |q|); the rounding is that of three longdouble evaluations of z, each
    within 2^-11 of the f64 bound kappa u |z| of the contract, over 2 h.  No constant."""
    checked = 0
    for name, (sc, img) in scenes.items():
        v, f, intr, size, _, _ = sc
        with np.errstate(all="ignore"):
            rows = dr.Rows(v, f, intr, size, img)
        live = np.nonzero(~rows.void)[0]
        # a spread of rows, the worst-conditioned one among them
        pick = list(live[:: max(1, len(live) // 12)][:12])
        if len(live):
            pick.append(live[np.argmax(rows.kappa[live])])
        vL = np.asarray(v, np.float32).astype(LD)
        for row in pick:
            t, pix = int(rows.face[row]), int(rows.pix[row])
            ids = np.asarray(f).reshape(-1, 3)[t]
            ext = float(np.abs(vL[ids] - vL[ids][[1, 2, 0]]).max())
            area2 = float(np.linalg.norm(np.cross((vL[ids[1]] - vL[ids[0]]).astype(np.float64), (vL[ids[2]] - vL[ids[0]]).astype(np.float64))))
            h = LD(2.0 ** (np.floor(np.log2(area2 / ext)) - 14))        # 2^-14 of the face's height: the pole of z(t) is a height away
            z0 = dr.exact_depth_at(vL, f, intr, size, t, pix)
            assert abs(z0 - rows.z[row]) <= 2.0 ** -60 * abs(z0)
            round_err = LD(rows.kappa[row] * dr.U * 2.0 ** -11) * abs(z0) * (1 + 2.0 ** -10)
            for a in range(3):
                for c in range(3):
                    vp, vm = vL.copy(), vL.copy()
                    vp[ids[a], c] += h
                    vm[ids[a], c] -= h
                    zp, zm = dr.exact_depth_at(vp, f, intr, size, t, pix), dr.exact_depth_at(vm, f, intr, size, t, pix)
                    cd, s2 = (zp - zm) / (2 * h), (zp - 2 * z0 + zm) / (h * h)
                    q = abs(h * s2 / (2 * cd)) if cd != 0 else LD(1)
                    tol = h * abs(s2) / 2 * min(LD(1), q) + 4 * round_err / (2 * h) + 3 * round_err / h * min(LD(1), q)
                    want = rows.beta[row, a] * rows.m[row, c]
                    assert abs(cd - want) <= tol, (name, row, a, c, float(cd), float(want), float(tol))
                    # the test has teeth: away from the two hard scenes the tolerance is far below the derivative's scale
                    if name not in ("sliver", "grazing"):
                        assert tol <= 2.0 ** -16 * rows.abs_m[row], (name, float(tol), float(rows.abs_m[row]))
                    checked += 1
    assert checked > 1000


def test_the_kernel_form_meets_the_contract_on_every_row(scenes):
    """every pixel of the rendered face image, of a hand-made image that addresses every face from pixels far from it, and a
    pixel list with indices outside the image"""
    worst = [0.0, 0.0, 0.0]
    for name, (sc, img) in scenes.items():
        v, f, intr, size, _, _ = sc
        H, W = size
        ragged = np.concatenate([np.arange(0, H * W, 3), [-1, H * W, H * W + 5, 2 ** 31 - 1, -2 ** 31]])
        for image, pixel in ((img, None), (dr.round_robin_image(len(f), size), None), (img, ragged)):
            with np.errstate(all="ignore"):
                rows = dr.Rows(v, f, intr, size, image, pixel)
                out = dr.kernel_form_f64(v, f, intr, size, image, pixel)
            w = dr.check_rows(rows, *out)
            worst = [max(a, b) for a, b in zip(worst, w)]
            assert np.array_equal(out[0] < 0, rows.void), name          # (no scene loses a row to the f64 evaluation)
    print(f"worst z, beta, m errors of the f64 restatement in units of their bounds: {worst}")
    assert max(worst) <= 1.0 and min(worst) > 0.25       # the f32 store alone is half of k = 2


def test_a_nan_corner_and_a_degenerate_face_are_void():
    v, f, intr, size = rr.two_spheres()
    v = v.copy()
    v[5] = np.nan
    v[40, 1] = np.inf
    with np.errstate(all="ignore"):
        img = dr.round_robin_image(len(f), size)
        rows = dr.Rows(v, f, intr, size, img)
        out = dr.kernel_form_f64(v, f, intr, size, img)
    touched = np.isin(np.asarray(f), (5, 40)).any(axis=1)
    assert rows.void[(rows.t_image >= 0) & touched[np.clip(rows.t_image, 0, None)]].all()
    dr.check_rows(rows, *out)
    assert np.isfinite(out[1][out[0] >= 0]).all()


def test_the_vjp_reference_checks_itself():
    rng = np.random.default_rng(0)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    index = rng.integers(-1, 3, 200).astype(np.int32)         # 2 is out of range: contributes nothing
    bary, coef, direction = (rng.standard_normal(s).astype(np.float32) for s in ((200, 3), (200,), (200, 3)))
    coef[index < 0] = np.nan
    G, T = dr.vjp_exact(faces, 5, index, bary, coef, direction)
    assert np.all(T[4] == 0) and np.all(T[:4] > 0) and np.all(np.abs(G) <= T)
    g = G.astype(np.float32)
    dr.check_vjp(faces, 5, index, bary, coef, direction, g)
    # the check has teeth: with positive terms T = |G*|, and three ulps (more than 3 u |g|, less half an ulp of the rounding) pass 2 u T
    bary, coef, direction = np.abs(bary), np.abs(np.nan_to_num(coef)) + np.float32(0.5), np.abs(direction)
    G, T = dr.vjp_exact(faces, 5, index, bary, coef, direction)
    assert np.array_equal(G, T)
    g = G.astype(np.float32)
    dr.check_vjp(faces, 5, index, bary, coef, direction, g)
    for _ in range(3):
        g[1, 1] = np.nextafter(g[1, 1], np.float32(np.inf))
    with pytest.raises(AssertionError):
        dr.check_vjp(faces, 5, index, bary, coef, direction, g)
    g[1, 1] = G[1, 1]
    g[4, 0] = np.float32(1e-30)                                # a vertex nothing lands on holds an exact 0
    with pytest.raises(AssertionError):
        dr.check_vjp(faces, 5, index, bary, coef, direction, g)


def test_the_term_scene_keeps_its_distance_from_both_thresholds():
    """the DepthResidualTerm test counts decisions that differ between the f32 rows and an f64 restatement and wants 0: on its
    scene every row's |r| and cosine are farther from trunc and min_cos than the rows contract lets the f32 rows move"""
    verts, faces, intr, size, sensor = dr.term_scene()
    assert not (np.isfinite(sensor[2]) & (sensor[2] > 0)).any()
    n_cut = n_gated = n_rows = 0
    for k in range(2):
        valid = np.isfinite(sensor[k]) & (sensor[k] > 0)
        assert valid.any() and not valid.all()
        pix = np.nonzero(valid.reshape(-1))[0]
        with np.errstate(all="ignore"):
            img = rr.kernel_form_f64(verts[k], faces, intr, size)[1]
            rows = dr.Rows(verts[k], faces, intr, size, img, pix)
        m_trunc, m_cos = dr.decision_margins(rows, sensor[k].reshape(-1)[pix], dr.TERM_TRUNC, dr.TERM_MIN_COS)
        assert m_trunc > 1e-5 and m_cos > 1e-3, (m_trunc, m_cos)
        keep = ~rows.void
        r = np.abs(rows.z[keep] - sensor[k].reshape(-1)[pix][keep].astype(LD)).astype(np.float64)
        n_rows += int(keep.sum())
        n_cut += int((r >= dr.TERM_TRUNC).sum())
        n_gated += int((rows.cos[keep] < dr.TERM_MIN_COS).sum())
    assert n_cut > 100 and n_gated > 100 and n_rows - n_cut > 1000          # both thresholds are active
