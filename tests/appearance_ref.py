"""Test infrastructure (numpy): the reference statement of the attribute shading (bodyfit_raster_shade_device) and of the image
sampling (bodyfit_raster_sample_device), of their contracts in include/bodyfit.h, and what the layer tests compose from them.

The definitions are evaluated in extended precision (np.longdouble, as raster_ref and depth_rows_ref do: 2^-11 of the f64 the
kernels work in) from the f32 inputs and the f64 intrinsics.  Everything here works on ONE frame: a face-id image [H, W] int, its
weights [H, W, 3] f32, verts [V, 3] f32, faces [nf, 3] int, attr [V, C] f32; points [N, 3] f32, an image [H, W, C] u8 or f32."""
import numpy as np

import raster_ref as rr

LD = np.longdouble
U = 2.0 ** -24
K_S = 2                       # the constants of include/bodyfit.h: |image^ - image| <= k_s u T_c, |w^ - w| <= k_s u w ...
DELTA_SHIFT = 2.0 ** -50      # ... delta = 2^-50 P
SAMPLE_SHIFT = 2.0 ** -46     # ... |value^ - B| <= u |B| + 2^-46 P M
TINY = 2.0 ** -150            # ... half the least f32 subnormal: the underflow term of a result below f32's normal range


def header_constants(text):
    """(k_s, the shift of delta, the shift of the sample's absolute term) as include/bodyfit.h states them"""
    import re
    s = text[text.index("VERTEX ATTRIBUTES OVER A RENDER"):]
    k = re.search(r"u = 2\^-24, k_s = (\d+) and per pixel", s)
    k2 = re.search(r"\|image\^_c - image_c\| <= k_s u T_c,\s+\|w\^_a - w_a\| <= k_s u w_a", s)
    s = s[s.index("IMAGE SAMPLES AT PROJECTED POINTS"):]
    d = re.search(r"delta = 2\^-(\d+) P", s)
    b = re.search(r"\|value\^ - B\(u, v\)\| <= u \|B\| \+ 2\^-(\d+) P M", s)
    c = re.search(r"u \|g_K\| \+ 2\^-(\d+) P M", s)
    assert k2 is not None and b.group(1) == c.group(1)
    return int(k.group(1)), int(d.group(1)), int(b.group(1))


# ---- shading -------------------------------------------------------------------------------------------------------------------
def shade_exact(face_img, bary, verts, faces, attr):
    """(void [H, W] bool, w [H, W, 3] longdouble, image [H, W, C] longdouble, T [H, W, C] longdouble) of the definition; image and T
    hold 0 on a void pixel.  A NaN attribute gives NaN."""
    assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an extended-precision long double"
    face_img = np.asarray(face_img, np.int64)
    H, W = face_img.shape
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lam = np.asarray(bary).reshape(H, W, 3)               # (f32 from the kernels; the identities of test_appearance.py pass f64)
    attr = np.asarray(attr)
    C = attr.shape[1]
    inside = (face_img >= 0) & (face_img < len(faces))
    if len(faces) == 0:
        return np.ones((H, W), bool), np.zeros((H, W, 3), LD), np.zeros((H, W, C), LD), np.zeros((H, W, C), LD)
    ids = faces[np.where(inside, face_img, 0)]                                    # [H, W, 3]
    Z = np.asarray(verts)[ids, 2]
    with np.errstate(all="ignore"):
        ok = inside & np.isfinite(lam).all(axis=-1) & np.isfinite(Z).all(axis=-1) & (Z > 0).all(axis=-1) & (lam >= 0).all(axis=-1)
        q = np.where(ok[..., None], lam, 0).astype(LD) / np.where(ok[..., None], Z, 1).astype(LD)
        S = q.sum(axis=-1)
        ok &= S != 0
        w = np.where(ok[..., None], q / np.where(ok, S, 1)[..., None], 0)
        a = attr[ids].astype(LD)                                                  # [H, W, 3, C]
        image = np.where(ok[..., None], (w[..., None] * a).sum(axis=2), 0)
        T = np.where(ok[..., None], (w[..., None] * np.abs(a)).sum(axis=2), 0)
    return ~ok, w, image, T


def check_shade(face_img, bary, verts, faces, attr, background, image, weight=None):
    """Asserts the shading contract at EVERY pixel of one frame's outputs (image f32 [H, W, C]; weight f32 [H, W, 3] or None).
    Returns the worst (image, weight) errors in units of their bounds."""
    void, w, exact, T = shade_exact(face_img, bary, verts, faces, attr)
    H, W = void.shape
    C = exact.shape[2]
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.shape == (H, W, C)
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    assert np.array_equal(image[void], np.broadcast_to(bg, image[void].shape)), "a void pixel holds the background"
    live = ~void
    worst = [0.0, 0.0]
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(exact)
        assert np.array_equal(np.isnan(image), nan & live[..., None]), "NaN exactly where a NaN attribute is used"
        fin = live[..., None] & ~nan
        err = np.abs(image.astype(LD) - exact)
        lim = K_S * U * T + TINY
        assert np.all(err[fin] <= lim[fin]), ("shade: image", int((err[fin] > lim[fin]).sum()), float((err[fin] / lim[fin]).max()))
        worst[0] = float((err[fin] / lim[fin]).max()) if fin.any() else 0.0
        if weight is not None:
            weight = np.asarray(weight)
            assert weight.dtype == np.float32 and weight.shape == (H, W, 3)
            assert np.all(weight[void] == 0), "a void pixel holds zero weights"
            assert np.all(weight[live] >= 0)
            err = np.abs(weight.astype(LD) - w)[live]
            lim = (K_S * U * w + TINY)[live]
            assert np.all(err <= lim), ("shade: weights", int((err > lim).sum()), float((err / lim).max()))
            worst[1] = float((err / lim).max()) if live.any() else 0.0
    return tuple(worst)


def shade_kernel_form_f64(face_img, bary, verts, faces, attr, background):
    """(image f32 [H, W, C], weight f32 [H, W, 3]) by the arithmetic of k_rs_shade, operation for operation in f64 (numpy never
    fuses): shows on the CPU that the contract is attainable."""
    face_img = np.asarray(face_img, np.int64)
    H, W = face_img.shape
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lam = np.asarray(bary, np.float32).reshape(H, W, 3)
    attr = np.asarray(attr, np.float32)
    C = attr.shape[1]
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    image = np.broadcast_to(bg, (H, W, C)).copy()
    weight = np.zeros((H, W, 3), np.float32)
    if len(faces) == 0:
        return image, weight
    inside = (face_img >= 0) & (face_img < len(faces))
    ids = faces[np.where(inside, face_img, 0)]
    Z = np.asarray(verts, np.float32)[ids, 2]
    with np.errstate(all="ignore"):
        ok = inside & np.isfinite(lam).all(axis=-1) & np.isfinite(Z).all(axis=-1) & (Z > 0).all(axis=-1) & (lam >= 0).all(axis=-1)
        q = np.where(ok[..., None], lam, 0).astype(np.float64) / np.where(ok[..., None], Z, 1).astype(np.float64)
        S = (q[..., 0] + q[..., 1]) + q[..., 2]
        ok &= S != 0
        w = q / np.where(ok, S, 1)[..., None]
        a = attr[ids].astype(np.float64)
        val = (w[..., 0, None] * a[..., 0, :] + w[..., 1, None] * a[..., 1, :]) + w[..., 2, None] * a[..., 2, :]
        image = np.where(ok[..., None], val.astype(np.float32), image)
        weight = np.where(ok[..., None], w.astype(np.float32), weight)
    return image, weight


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def _cell(c, n):
    """the cell index of coordinate c (an integer-valued array) in an axis of n texels: min(c, max(n - 2, 0)), and its partner"""
    c0 = np.clip(c, 0, max(n - 2, 0)).astype(np.int64)
    return c0, np.minimum(c0 + 1, n - 1)


def _patch(img, i0, j0, u, v):
    """(value [N, C], d/du [N, C], d/dv [N, C], M [N]) of the bilinear patch of the cells (i0, j0) at (u, v), longdouble"""
    H, W = img.shape[:2]
    i1, j1 = np.minimum(i0 + 1, H - 1), np.minimum(j0 + 1, W - 1)
    I00, I01, I10, I11 = (img[i, j].astype(LD) for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
    a, b = (u - j0.astype(LD))[:, None], (v - i0.astype(LD))[:, None]
    val = (1 - a) * (1 - b) * I00 + a * (1 - b) * I01 + (1 - a) * b * I10 + a * b * I11
    du = (1 - b) * (I01 - I00) + b * (I11 - I10)
    dv = (1 - a) * (I10 - I00) + a * (I11 - I01)
    M = np.max(np.abs(np.stack((I00, I01, I10, I11))), axis=(0, 2))
    return val, du, dv, M


class Samples:
    """the exact samples of one frame, and what the contract allows around them"""

    def __init__(self, points, intr, img, gate=None, z_near=0.1):
        assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an extended-precision long double"
        img = np.asarray(img)
        self.img = img = img[..., None] if img.ndim == 2 else img
        H, W, C = img.shape
        fx, fy, cx, cy = (LD(float(a)) for a in intr)
        p = np.asarray(points, np.float32)
        N = len(p)
        self.P = float(max(W, H) + max(abs(cx), abs(cy)))
        self.delta = DELTA_SHIFT * self.P
        with np.errstate(all="ignore"):
            self.base = np.isfinite(p).all(axis=1) & (p[:, 2] >= np.float32(z_near))
            if gate is not None:
                self.base &= np.asarray(gate).reshape(N) != 0
            q = np.where(self.base[:, None], p, np.float32(1)).astype(LD)
            self.u, self.v = fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy
        u, v, d = self.u, self.v, LD(self.delta)
        self.live = self.base & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        self.must = self.base & (u >= d) & (u <= W - 1 - d) & (v >= d) & (v <= H - 1 - d)
        self.may = self.base & (u >= -d) & (u <= W - 1 + d) & (v >= -d) & (v <= H - 1 + d)
        uc, vc = np.clip(u, 0, W - 1), np.clip(v, 0, H - 1)
        self.j0, _ = _cell(np.floor(uc), W)
        self.i0, _ = _cell(np.floor(vc), H)
        self.B, self.du, self.dv, self.M = _patch(img, self.i0, self.j0, uc, vc)     # B at the point moved into the rectangle
        # every cell whose closed support is within delta of (u, v)
        self.candidates = []
        for jj in (np.floor(u - d), np.floor(u + d)):
            for ii in (np.floor(v - d), np.floor(v + d)):
                j0, _ = _cell(np.clip(jj, 0, W - 1), W)
                i0, _ = _cell(np.clip(ii, 0, H - 1), H)
                self.candidates.append((i0, j0) + _patch(img, i0, j0, u, v)[1:])
        self.n_border = int((self.may & ((self.candidates[0][0] != self.candidates[3][0]) |
                                         (self.candidates[0][1] != self.candidates[3][1]))).sum())


def check_sample(points, intr, img, gate, z_near, value, valid, grad=None):
    """Asserts the sampling contract at EVERY point of one frame's outputs (value f32 [N, C], valid u8 / bool [N], grad f32
    [N, C, 2] or None).  For a point within delta of a cell border the gradient is held against every candidate cell.  Returns
    (the worst value error, the worst gradient error) in units of their bounds, and the Samples."""
    s = Samples(points, intr, img, gate, z_near)
    N, C = len(s.u), s.img.shape[2]
    value, valid = np.asarray(value), np.asarray(valid).astype(bool)
    assert value.dtype == np.float32 and value.shape == (N, C) and valid.shape == (N,)
    assert np.all(valid[s.must]), ("(a) a live point well inside came back invalid", np.nonzero(s.must & ~valid)[0][:8])
    assert not np.any(valid[~s.may]), ("(a) a point outside came back live", np.nonzero(~s.may & valid)[0][:8])
    assert np.all(value[~valid] == 0), "an invalid point holds 0"
    worst = [0.0, 0.0]
    with np.errstate(invalid="ignore", over="ignore"):
        Mall = s.M.copy()
        for c in s.candidates:
            Mall = np.maximum(Mall, c[4])
        lim = U * np.abs(s.B) + (SAMPLE_SHIFT * s.P * Mall)[:, None] + TINY
        err = np.abs(value.astype(LD) - s.B)
        bad = valid[:, None] & ~(err <= lim)
        assert not bad.any(), ("(b) value", int(bad.sum()), float((err / lim)[valid].max()))
        worst[0] = float((err / lim)[valid].max()) if valid.any() else 0.0
        if grad is not None:
            grad = np.asarray(grad)
            assert grad.dtype == np.float32 and grad.shape == (N, C, 2)
            assert np.all(grad[~valid] == 0), "an invalid point holds a zero gradient"
            best = np.full(N, np.inf)
            for _, _, du, dv, M in s.candidates:
                M = np.maximum(M, s.M)
                ru = np.abs(grad[:, :, 0].astype(LD) - du) / (U * np.abs(du) + (SAMPLE_SHIFT * s.P * M)[:, None] + TINY)
                rv = np.abs(grad[:, :, 1].astype(LD) - dv) / (U * np.abs(dv) + (SAMPLE_SHIFT * s.P * M)[:, None] + TINY)
                best = np.minimum(best, np.maximum(ru, rv).max(axis=1).astype(np.float64))
            bad = valid & ~(best <= 1.0)
            assert not bad.any(), ("(c) gradient", int(bad.sum()), float(best[valid].max()))
            worst[1] = float(best[valid].max()) if valid.any() else 0.0
    return worst[0], worst[1], s


def sample_kernel_form_f64(points, intr, img, gate=None, z_near=0.1):
    """(value f32 [N, C], valid bool [N], grad f32 [N, C, 2]) by the arithmetic of k_rs_sample, operation for operation in f64"""
    img = np.asarray(img)
    img = img[..., None] if img.ndim == 2 else img
    H, W, C = img.shape
    fx, fy, cx, cy = (np.float64(a) for a in intr)
    p = np.asarray(points, np.float32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(p).all(axis=1) & (p[:, 2] >= np.float32(z_near))
        if gate is not None:
            ok &= np.asarray(gate).reshape(-1) != 0
        q = np.where(ok[:, None], p, np.float32(1)).astype(np.float64)
        u, v = fx * (q[:, 0] / q[:, 2]) + cx, fy * (q[:, 1] / q[:, 2]) + cy
        ok &= (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        j0, j1 = _cell(np.floor(u), W)
        i0, i1 = _cell(np.floor(v), H)
        a, b = (u - j0)[:, None], (v - i0)[:, None]
        I00, I01, I10, I11 = (img[i, j].astype(np.float64) for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
        na, nb = 1.0 - a, 1.0 - b
        val = ((na * nb) * I00 + (a * nb) * I01) + ((na * b) * I10 + (a * b) * I11)
        gu = nb * (I01 - I00) + b * (I11 - I10)
        gv = na * (I10 - I00) + a * (I11 - I01)
        z = np.zeros_like(val)
        return (np.where(ok[:, None], val, z).astype(np.float32), ok,
                np.where(ok[:, None, None], np.stack((gu, gv), axis=-1), 0.0).astype(np.float32))


# ---- what the layer tests compose from the contracts ----------------------------------------------------------------------------
def shaded_depth_bound(Fc, face, lmin, zr):
    """[n] f64: what shading attr = the vertices' own z over a render may differ from that render's depth zr by, at covered pixels
    with rendered faces `face` (Fc = raster_ref.Faces of the scene, lmin the exact least lambda there).  The render's contract
    (e) puts each stored weight within tau of the exact lambda (m = 2 tau in the coverage band, where (b) speaks of the clamped
    lambda) and their sum within 2 tau of 1, so sum lambda^ / sum (lambda^_a / Z_a) is within (2 + 3 R) m tau / (1 - 3 m tau R) of
    z(t, s) relatively; (b) puts zr within (k_z + c_t) u of z(t, s); the shading adds k_s u T with T the shaded depth itself."""
    tau, R, c = Fc.tau[face], Fc.R[face], Fc.c[face]
    m = np.where(lmin < 0, 2.0, 1.0) * tau
    with np.errstate(all="ignore"):
        rel = np.where(3 * m * R < 0.5, (2 + 3 * R) * m / (1 - 3 * m * R), np.inf)
        return (rel + (rr.K_Z + c) * U + K_S * U * (1 + rel)) * zr * (1 + 2.0 ** -20)


def sample_vjp_bound(points, intr, g, samples, valid, dg=None):
    """[N, 3] f64: what dL/dpoints formed from the kernel's f32 gradient output (each derivative within u |g_K| + 2^-46 P M of the
    cell's) with the upstream g [N, C] (known to dg [N, C] or exactly), in f64 and rounded once, may differ by from the exact
    chain rule through (u, v) = (fx X / Z + cx, fy Y / Z + cy) at the same cell"""
    fx, fy = float(intr[0]), float(intr[1])
    p = np.asarray(points, np.float64)
    g = np.abs(np.asarray(g, np.float64))
    dg = np.zeros_like(g) if dg is None else np.asarray(dg, np.float64)
    absu = np.max([np.abs(c[2]).astype(np.float64) for c in samples.candidates], axis=0)     # [N, C]
    absv = np.max([np.abs(c[3]).astype(np.float64) for c in samples.candidates], axis=0)
    tol = (SAMPLE_SHIFT * samples.P * np.max([c[4] for c in samples.candidates], axis=0).astype(np.float64))[:, None]
    eu = (g * (U * absu + tol) + dg * (absu + U * absu + tol)).sum(axis=1)
    ev = (g * (U * absv + tol) + dg * (absv + U * absv + tol)).sum(axis=1)
    Gu, Gv = ((g + dg) * (absu + tol)).sum(axis=1), ((g + dg) * (absv + tol)).sum(axis=1)
    with np.errstate(all="ignore"):
        Z = np.where(valid, p[:, 2], 1.0)
        bx, by = fx * eu / Z, fy * ev / Z
        bz = (bx * np.abs(p[:, 0]) + by * np.abs(p[:, 1])) / Z
        mag = np.stack((fx * Gu / Z, fy * Gv / Z, (fx * Gu * np.abs(p[:, 0]) + fy * Gv * np.abs(p[:, 1])) / Z ** 2), axis=1)
        out = np.stack((bx, by, bz), axis=1) + 2 * U * mag
    return np.where(valid[:, None], out, 0.0)


def pixel_colour_ranges(verts, faces, intr, size, colour, background=0.0, z_near=0.1):
    """(lo, hi) [H, W, C] f64: per pixel the range of what a shaded render of the frame may hold, from the reference's own render:
    over every face the render's contract admits at the pixel, the exactly interpolated colour at the lambda clamped to the face,
    widened by the colour's spread over the face times the (2 + 3 R) 2 tau the stored weights may move the object-space weights
    by; the background where the contract lets the pixel be empty"""
    ref = rr.Reference(verts, faces, intr, size, z_near)
    Fc = ref.F
    H, W = size
    col = np.asarray(colour, np.float64)
    C = col.shape[1]
    lo, hi = np.full((H, W, C), np.inf), np.full((H, W, C), -np.inf)
    fa = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for t in np.nonzero(Fc.loose)[0]:
            y0, y1, x0, x1 = Fc.region(t)
            if y0 >= y1 or x0 >= x1:
                continue
            ys, xs = np.mgrid[y0:y1, x0:x1]
            lam, lmin, z = Fc.evaluate(t, ys, xs)
            sl = (slice(y0, y1), slice(x0, x1))
            adm = (lmin >= -Fc.tau[t]) & (z / (1 + (rr.K_Z + Fc.c[t]) * U) <= ref.zcap[sl])
            if not adm.any():
                continue
            pos = np.maximum(lam, 0)
            pos /= pos.sum(axis=-1, keepdims=True)
            q = pos / Fc.Z[t].astype(np.float64)
            w = q / q.sum(axis=-1, keepdims=True)
            c = w @ col[fa[t]]                                                            # [h, w, C]
            spread = np.abs(col[fa[t]][:, None, :] - col[fa[t]][None, :, :]).max(axis=(0, 1))
            slack = min((2 + 3 * Fc.R[t]) * 2 * Fc.tau[t] * 3, 1.0) * spread + K_S * U * np.abs(col[fa[t]]).max(axis=0)
            lo[sl] = np.where(adm[..., None], np.minimum(lo[sl], c - slack), lo[sl])
            hi[sl] = np.where(adm[..., None], np.maximum(hi[sl], c + slack), hi[sl])
    empty_ok = ~np.isfinite(ref.zcap)
    bg = np.broadcast_to(np.asarray(background, np.float64), (C,))
    lo = np.where(empty_ok[..., None], np.minimum(lo, bg), lo)
    hi = np.where(empty_ok[..., None], np.maximum(hi, bg), hi)
    return lo, hi, ref


def linear_image(size, alpha, beta, gamma, dtype=np.float32):
    """I[i][j] = alpha j + beta i + gamma"""
    H, W = size
    i, j = np.mgrid[0:H, 0:W]
    return (alpha * j + beta * i + gamma).astype(dtype)
