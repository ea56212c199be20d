"""Test infrastructure (numpy): the reference statement of the texture lookup (bodyfit_raster_texture_device) and of its gradients
(bodyfit_raster_texture_grad_device), in np.longdouble from the f32 inputs; the kernels' operation order restated in f64, the
accumulation in int64 with the same scale exponent; and the checks of include/bodyfit.h's bounds per pixel and per texel.
Everything works on ONE frame (face_img [H, W], bary [H, W, 3], verts [V, 3]) unless it says frames."""
import re

import numpy as np

import appearance_ref as ar

LD = np.longdouble
U = 2.0 ** -24
EPS = 2.0 ** -53
K_S = 2                     # the constants of include/bodyfit.h (UV TEXTURES OVER A RENDER) ... the uv's k_s, the shade's
K_T = 16                    # ... kappa = k_t 2^-50 P_x U
KAPPA_UNIT = 2.0 ** -50
DELTA_SHIFT = 2.0 ** -49    # ... delta = 2^-49 P_x U
K_G = 6                     # ... |g^ - g*| <= u |g*| + m 2^-(s + 1) + k_g eps A
TINY = 2.0 ** -149


def header_constants(text):
    """(k_s, k_t, the shift of kappa's unit, the shift of delta, k_g) as include/bodyfit.h states them"""
    s = text[text.index("UV TEXTURES OVER A RENDER"):]
    d = re.search(r"delta = 2\^-(\d+) P_x U", s)
    k = re.search(r"kappa = k_t 2\^-(\d+) P_x U with k_t = (\d+)", s)
    ks = re.search(r"per component \(k_s = (\d+), the shade's\)", s)
    g = re.search(r"k_g = (\d+)", s)
    assert re.search(r"\|image\^_c - B_c\(x, y\)\| <= u \|B_c\| \+ kappa M", s)
    assert re.search(r"\|g\^ - g\*\| <= u \|g\*\| \+ m 2\^-\(s \+ 1\) \+ k_g eps A", s)
    assert re.search(r"s = 60 - B - E", s)
    return int(ks.group(1)), int(k.group(2)), int(k.group(1)), int(d.group(1)), int(g.group(1))


def make_texture(Ht, Wt, C, kind, seed=0):
    """a random texture: kind 0 u8 (the full range), 1 f32 in (-1, 2)"""
    rng = np.random.default_rng(1000 * seed + 31 * Ht + 7 * Wt + C)
    if kind == 0:
        return rng.integers(0, 256, size=(Ht, Wt, C), dtype=np.uint8)
    return rng.uniform(-1.0, 2.0, size=(Ht, Wt, C)).astype(np.float32)


# ---- the pixel: void rule, weights, uv -----------------------------------------------------------------------------------------
class Pixels:
    """the exact per-pixel stage of one frame: void [H, W], w [H, W, 3], uv [H, W, 2], T_uv [H, W, 2] = sum_a w_a |uv_a| and Umax
    [H, W] = max(1, max_a |u_a|, |v_a|), longdouble"""

    def __init__(self, face_img, bary, verts, faces, uv, uv_faces):
        assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an extended-precision long double"
        face_img = np.asarray(face_img, np.int64)
        H, W = face_img.shape
        faces = np.asarray(faces, np.int64).reshape(-1, 3)
        uvf = np.asarray(uv_faces, np.int64).reshape(-1, 3)
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        T = len(uv)
        lam = np.asarray(bary).reshape(H, W, 3)
        self.shape = (H, W)
        if len(faces) == 0:
            self.void = np.ones((H, W), bool)
            self.w, self.uv, self.T_uv, self.Umax = np.zeros((H, W, 3), LD), np.zeros((H, W, 2), LD), np.zeros((H, W, 2), LD), np.ones((H, W), LD)
            return
        inside = (face_img >= 0) & (face_img < len(faces))
        t = np.where(inside, face_img, 0)
        ids, k = faces[t], uvf[t]
        inside &= ((k >= 0) & (k < T)).all(axis=-1)
        k = np.where(inside[..., None], k, 0)
        Z = np.asarray(verts)[ids, 2]
        with np.errstate(all="ignore"):
            ok = inside & np.isfinite(lam).all(axis=-1) & np.isfinite(Z).all(axis=-1) & (Z > 0).all(axis=-1) & (lam >= 0).all(axis=-1)
            q = np.where(ok[..., None], lam, 0).astype(LD) / np.where(ok[..., None], Z, 1).astype(LD)
            S = q.sum(axis=-1)
            ok &= S != 0
            w = np.where(ok[..., None], q / np.where(ok, S, 1)[..., None], 0)
            a = (uv[k] if T else np.zeros((H, W, 3, 2), np.float32)).astype(LD)       # [H, W, 3, 2]
            val = (w[..., None] * a).sum(axis=2)
            ok &= np.isfinite(val).all(axis=-1)
            a = np.where(ok[..., None, None], a, 0)
            self.uv = np.where(ok[..., None], val, 0)
            self.T_uv = np.where(ok[..., None], (w[..., None] * np.abs(a)).sum(axis=2), 0)
            self.Umax = np.maximum(1, np.abs(a).max(axis=(2, 3)))
        self.void, self.w = ~ok, np.where(ok[..., None], w, 0)


def pixels_f64(face_img, bary, verts, faces, uv, uv_faces):
    """the same stage by the arithmetic of k_texture.hip's tx_pixel, operation for operation in f64 (numpy never fuses):
    dict(ok [H, W], w [H, W, 3] f64, u, v [H, W] f64)"""
    face_img = np.asarray(face_img, np.int64)
    H, W = face_img.shape
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    uvf = np.asarray(uv_faces, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    T = len(uv)
    lam = np.asarray(bary, np.float32).reshape(H, W, 3)
    if len(faces) == 0:
        return {"ok": np.zeros((H, W), bool), "w": np.zeros((H, W, 3)), "u": np.zeros((H, W)), "v": np.zeros((H, W))}
    inside = (face_img >= 0) & (face_img < len(faces))
    t = np.where(inside, face_img, 0)
    ids, k = faces[t], uvf[t]
    inside &= ((k >= 0) & (k < T)).all(axis=-1)
    k = np.where(inside[..., None], k, 0)
    Z = np.asarray(verts, np.float32)[ids, 2]
    with np.errstate(all="ignore"):
        ok = inside & np.isfinite(lam).all(axis=-1) & np.isfinite(Z).all(axis=-1) & (Z > 0).all(axis=-1) & (lam >= 0).all(axis=-1)
        q = np.where(ok[..., None], lam, 0).astype(np.float64) / np.where(ok[..., None], Z, 1).astype(np.float64)
        S = (q[..., 0] + q[..., 1]) + q[..., 2]
        ok &= S != 0
        w = q / np.where(ok, S, 1)[..., None]
        a = (uv[k] if T else np.zeros((H, W, 3, 2), np.float32)).astype(np.float64)
        val = (w[..., 0, None] * a[..., 0, :] + w[..., 1, None] * a[..., 1, :]) + w[..., 2, None] * a[..., 2, :]
        ok &= np.isfinite(val).all(axis=-1)
    z = ok[..., None]
    return {"ok": ok, "w": np.where(z, w, 0.0), "u": np.where(ok, val[..., 0], 0.0), "v": np.where(ok, val[..., 1], 0.0)}


# ---- the lookup ----------------------------------------------------------------------------------------------------------------
def _clamped(u, n, one):
    """(the unclamped texel coordinate u n - 1/2, its clamp to [0, n - 1], "the clamp is not active") in the type of `one`"""
    xr = u * one * n - one / 2
    return xr, np.minimum(np.maximum(xr, 0), n - 1), (xr >= 0) & (xr <= n - 1)


class Lookup:
    """the exact lookup of one frame's Pixels in tex [Ht, Wt, C]: x, y (clamped), xr, yr, free_x, free_y, the cell (i0, j0), B
    [H, W, C], the patch's d/dx and d/dy [H, W, C] and M [H, W] (the cell's largest |texel|), longdouble; 0 on void pixels"""

    def __init__(self, px, tex):
        tex = np.asarray(tex)
        self.tex = tex
        Ht, Wt, C = tex.shape
        H, W = px.shape
        self.px = px
        self.xr, self.x, self.free_x = _clamped(px.uv[..., 0], Wt, LD(1))
        self.yr, self.y, self.free_y = _clamped(px.uv[..., 1], Ht, LD(1))
        self.j0, _ = ar._cell(np.floor(self.x), Wt)
        self.i0, _ = ar._cell(np.floor(self.y), Ht)
        self.delta = DELTA_SHIFT * max(Wt, Ht) * px.Umax
        self.kappa = K_T * KAPPA_UNIT * max(Wt, Ht) * px.Umax
        B, du, dv, M = self.patch(self.i0, self.j0)
        live = ~px.void
        self.B, self.M = np.where(live[..., None], B, 0), np.where(live, M, 0)
        self.du, self.dv = du, dv

    def patch(self, i0, j0):
        """(value, d/dx, d/dy [H, W, C], M [H, W]) of the patch of the cells (i0, j0) at the exact (x, y)"""
        H, W = self.px.shape
        val, du, dv, M = ar._patch(self.tex, i0.reshape(-1), j0.reshape(-1), self.x.reshape(-1), self.y.reshape(-1))
        return val.reshape(H, W, -1), du.reshape(H, W, -1), dv.reshape(H, W, -1), M.reshape(H, W)


def lookup_f64(pf, tex, background):
    """the lookup by the arithmetic of k_tx_forward: dict(image f32 [H, W, C], weight f32 [H, W, 3], uv f32 [H, W, 2], x, y f64,
    i0, i1, j0, j1, free_x, free_y, omega f64 [H, W, 4] (the weights of texels 00, 01, 10, 11), du, dv f64 [H, W, C])"""
    tex = np.asarray(tex)
    Ht, Wt, C = tex.shape
    ok = pf["ok"]
    H, W = ok.shape
    _, x, free_x = _clamped(pf["u"], Wt, np.float64(1))
    _, y, free_y = _clamped(pf["v"], Ht, np.float64(1))
    j0 = np.minimum(np.floor(x).astype(np.int64), max(Wt - 2, 0)); j1 = np.minimum(j0 + 1, Wt - 1)
    i0 = np.minimum(np.floor(y).astype(np.int64), max(Ht - 2, 0)); i1 = np.minimum(i0 + 1, Ht - 1)
    a, b = (x - j0.astype(np.float64)), (y - i0.astype(np.float64))
    na, nb = 1.0 - a, 1.0 - b
    omega = np.stack((na * nb, a * nb, na * b, a * b), axis=-1)
    I00, I01, I10, I11 = (tex[i, j].astype(np.float64) for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
    o = omega[..., None, :]
    val = (o[..., 0] * I00 + o[..., 1] * I01) + (o[..., 2] * I10 + o[..., 3] * I11)
    du = nb[..., None] * (I01 - I00) + b[..., None] * (I11 - I10)
    dv = na[..., None] * (I10 - I00) + a[..., None] * (I11 - I01)
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    image = np.where(ok[..., None], val.astype(np.float32), np.broadcast_to(bg, (H, W, C)))
    return {"ok": ok, "image": image, "weight": pf["w"].astype(np.float32),
            "uv": np.stack((pf["u"], pf["v"]), axis=-1).astype(np.float32), "x": x, "y": y, "i0": i0, "i1": i1, "j0": j0, "j1": j1,
            "free_x": free_x & ok, "free_y": free_y & ok, "omega": omega, "du": du, "dv": dv}


def check_forward(lk, form, background, image, weight=None, uv_out=None):
    """Asserts the lookup's contract at EVERY pixel of one frame's outputs against Lookup lk; form: lookup_f64's dict, whose cell
    stands for "the returned cell" in M.  Returns the worst image error in units of its bound."""
    px = lk.px
    H, W = px.shape
    C = lk.tex.shape[2]
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.shape == (H, W, C)
    void, live = px.void, ~px.void
    assert np.array_equal(form["ok"], live), "the f64 restatement voids the pixels the definition voids"
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    assert np.array_equal(image[void], np.broadcast_to(bg, image[void].shape)), "a void pixel holds the background"
    with np.errstate(invalid="ignore", over="ignore"):
        # the returned cell lies within delta of the exact clamped point, and M covers both cells
        assert np.all(np.abs(form["x"].astype(LD) - lk.x)[live] <= lk.delta[live]) and np.all(np.abs(form["y"].astype(LD) - lk.y)[live] <= lk.delta[live])
        M = np.maximum(lk.M, lk.patch(form["i0"], form["j0"])[3])
        err = np.abs(image.astype(LD) - lk.B)
        lim = U * np.abs(lk.B) + (lk.kappa * M)[..., None] + TINY
        fin = live[..., None] & np.isfinite(lk.B)
        assert np.all(err[fin] <= lim[fin]), ("texture: image", int((err[fin] > lim[fin]).sum()), float((err[fin] / lim[fin]).max()))
        worst = float((err[fin] / lim[fin]).max()) if fin.any() else 0.0
        if weight is not None:
            weight = np.asarray(weight)
            assert weight.dtype == np.float32 and weight.shape == (H, W, 3)
            assert np.all(weight[void] == 0), "a void pixel holds zero weights"
            err, lim = np.abs(weight.astype(LD) - px.w)[live], (K_S * U * px.w + TINY)[live]
            assert np.all(err <= lim), ("texture: weights", float((err / lim).max()))
        if uv_out is not None:
            uv_out = np.asarray(uv_out)
            assert uv_out.dtype == np.float32 and uv_out.shape == (H, W, 2)
            assert np.all(uv_out[void] == 0), "a void pixel holds uv 0"
            err, lim = np.abs(uv_out.astype(LD) - px.uv)[live], (K_S * U * px.T_uv + TINY)[live]
            assert np.all(err <= lim), ("texture: uv", float((err / lim).max()))
    return worst


# ---- (a) the gradient in uv ---------------------------------------------------------------------------------------------------
def grad_uv_exact(lk, form, G):
    """(g [H, W, 2], bound [H, W, 2], undecided [H, W, 2] bool) of the contract's (a): the derivative of the RETURNED cell's patch at
    the exact (x, y) times (Wt, Ht), 0 where the exact clamp is active or the pixel void; undecided: the unclamped coordinate is
    within delta of 0 or of n - 1, where 0 and g are both allowed"""
    Ht, Wt, C = lk.tex.shape
    G = np.asarray(G, np.float32).astype(LD)
    _, du, dv, Mk = lk.patch(form["i0"], form["j0"])
    live = ~lk.px.void
    M = np.maximum(lk.M, Mk)
    g = np.stack(((G * du).sum(axis=-1) * Wt, (G * dv).sum(axis=-1) * Ht), axis=-1)
    g = np.where(live[..., None], g, 0)
    slack = (lk.kappa * M * np.abs(G).sum(axis=-1))[..., None] * np.array([Wt, Ht], LD)
    free = np.stack((lk.free_x, lk.free_y), axis=-1) & live[..., None]
    d = lk.delta[..., None]
    r, n = np.stack((lk.xr, lk.yr), axis=-1), np.array([Wt - 1, Ht - 1], LD)
    undecided = live[..., None] & ((np.abs(r) <= d) | (np.abs(r - n) <= d))
    return g, U * np.abs(g) + slack + TINY, free, undecided


def check_grad_uv(lk, form, G, grad_uv):
    """Asserts (a) at EVERY pixel; returns the worst error in units of its bound"""
    g, lim, free, undecided = grad_uv_exact(lk, form, G)
    got = np.asarray(grad_uv)
    assert got.dtype == np.float32 and got.shape == g.shape
    assert np.all(got[lk.px.void] == 0), "a void pixel holds a zero uv gradient"
    with np.errstate(invalid="ignore", over="ignore"):
        e_free, e_zero = np.abs(got.astype(LD) - g) <= lim, got == 0
        good = np.where(undecided, e_free | e_zero, np.where(free, e_free, e_zero))
        assert np.all(good), ("texture: grad_uv", int((~good).sum()))
        sel = free & ~undecided
        return float((np.abs(got.astype(LD) - g)[sel] / lim[sel]).max()) if sel.any() else 0.0


# ---- (b) the gradient in the texels --------------------------------------------------------------------------------------------
def scale_exponent(G, n_pixels):
    """(s, gbits) of the kernels: gbits the largest bit pattern of |G| over the whole array, E = (gbits >> 23) - 126, B the bit
    length of n_pixels, s = 60 - B - E"""
    bits = np.ascontiguousarray(G, np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    gbits = int(bits.max()) if bits.size else 0
    return 60 - int(n_pixels).bit_length() - ((gbits >> 23) - 126), gbits


def _destinations(form, Ht, Wt, C):
    """[H, W, 4, C] int64: the linear texel element of contribution (k, c) of every pixel"""
    i, j = (form["i0"], form["i0"], form["i1"], form["i1"]), (form["j0"], form["j1"], form["j0"], form["j1"])
    at = np.stack([(ii * Wt + jj) * C for ii, jj in zip(i, j)], axis=-1)
    return at[..., None] + np.arange(C)


def accumulate_f64(forms, G, tex_shape, shared, order=None):
    """the accumulation of k_tx_grad and k_tx_fold over the frames' lookup_f64 dicts: (grad_tex f32 in the texture's layout, the
    int64 sums, s).  order: a permutation of the frames' pixels (of all contributions), to show that the sums do not depend on it"""
    Ht, Wt, C = tex_shape
    G = np.asarray(G, np.float32)
    F = len(forms)
    n_tex = Ht * Wt * C
    s, gbits = scale_exponent(G, G.size // C)
    sums = np.zeros((1 if shared else F) * n_tex, np.int64)
    if gbits >= 0x7f800000:
        return np.full(sums.shape, np.nan, np.float32).reshape((Ht, Wt, C) if shared else (F, Ht, Wt, C)), sums, s
    if gbits:
        scale = np.ldexp(1.0, s)
        dest, q = [], []
        for f, form in enumerate(forms):
            t = G[f].astype(np.float64)[..., None, :] * form["omega"][..., :, None]            # [H, W, 4, C]: rounds once
            qf = np.where(form["ok"][..., None, None], np.rint(t * scale), 0.0).astype(np.int64)
            dest.append((_destinations(form, Ht, Wt, C) + (0 if shared else f * n_tex)).reshape(-1))
            q.append(qf.reshape(-1))
        dest, q = np.concatenate(dest), np.concatenate(q)
        if order is not None:
            dest, q = dest[order], q[order]
        np.add.at(sums, dest, q)
    g = (sums.astype(np.float64) * np.ldexp(1.0, -s)).astype(np.float32)
    return g.reshape((Ht, Wt, C) if shared else (F, Ht, Wt, C)), sums, s


def grad_tex_exact(forms, G, tex_shape, shared):
    """(g* longdouble, m int64, A longdouble) per texel element in the texture's layout: the adjoint at the returned (x^, y^) with
    exact weights, the count of non-zero contributions and the sum of their magnitudes"""
    Ht, Wt, C = tex_shape
    G = np.asarray(G, np.float32)
    F = len(forms)
    n_tex = Ht * Wt * C
    n = (1 if shared else F) * n_tex
    g, m, A = np.zeros(n, LD), np.zeros(n, np.int64), np.zeros(n, LD)
    for f, form in enumerate(forms):
        a, b = form["x"].astype(LD) - form["j0"], form["y"].astype(LD) - form["i0"]
        omega = np.stack(((1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b), axis=-1)
        t = np.where(form["ok"][..., None, None], G[f].astype(LD)[..., None, :] * omega[..., :, None], 0).reshape(-1)
        dest = (_destinations(form, Ht, Wt, C) + (0 if shared else f * n_tex)).reshape(-1)
        np.add.at(g, dest, t)
        np.add.at(A, dest, np.abs(t))
        np.add.at(m, dest, (t != 0).astype(np.int64))
    shape = (Ht, Wt, C) if shared else (F, Ht, Wt, C)
    return g.reshape(shape), m.reshape(shape), A.reshape(shape)


def check_grad_tex(forms, G, tex_shape, shared, grad_tex):
    """Asserts (b) at EVERY texel element; returns the worst error in units of its bound"""
    got = np.asarray(grad_tex)
    s, gbits = scale_exponent(G, np.asarray(G).size // tex_shape[2])
    assert got.dtype == np.float32
    if gbits >= 0x7f800000:
        assert np.isnan(got).all(), "a non-finite upstream gradient gives an all-NaN texel gradient"
        return 0.0
    g, m, A = grad_tex_exact(forms, G, tex_shape, shared)
    assert got.shape == g.shape
    err = np.abs(got.astype(LD) - g)
    lim = U * np.abs(g) + m * np.ldexp(LD(1), -(s + 1)) + K_G * EPS * A + TINY
    assert np.all(err <= lim), ("texture: grad_tex", int((err > lim).sum()), float((err / lim).max()))
    return float((err / lim).max())
