"""Test infrastructure (numpy): the reference statement of the texture lookup with mipmaps (bodyfit_texture_mip_layout,
bodyfit_raster_texture_mip_build_device, bodyfit_raster_texture_mip_device, bodyfit_raster_texture_mip_grad_device): the layout, the
pyramid, the footprint and its level of detail, the trilinear image and the gradients (a) and (b) in np.longdouble from the f32
inputs; the kernels' operation order restated in f64 with the int64 accumulation and the fixed-order fold; and the checks of
include/bodyfit.h's bounds per pixel and per texel.  Everything works on ONE frame unless it says frames; texture_ref.py holds the
single-level pieces."""
import re

import numpy as np

import texture_ref as tr

LD = np.longdouble
U, EPS, TINY = tr.U, tr.EPS, tr.TINY
MAX_LEVELS = 15            # the constants of include/bodyfit.h (MIPMAPS OF THE TEXTURE LOOKUP) ... BODYFIT_TX_MAX_LEVELS
K_D = 12                   # ... D = 12 U R_t Q_t / (P_t Lambda)
K_J = 64                   # ... E_J = k_J eps P_x D (1 + 4 Q_t)
K_L = 24                   # ... d_log = k_L eps (1 + |log2(rho^2) / 2| + |lod_bias|)
K_M = 24                   # ... |g^ - g*| <= u |g*| + sum_l a_l m_l 2^-(s + 1) + k_m eps sum_l a_l A_l
Q_CAP = 0.5 / (80 * EPS)   # ... the footprint's contract holds for 80 eps Q_t <= 1/2


def header_constants(text):
    """(BODYFIT_TX_MAX_LEVELS, the 12 of D, k_J, k_L, k_m) as include/bodyfit.h states them"""
    s = text[text.index("MIPMAPS OF THE TEXTURE LOOKUP"):]
    n = re.search(r"#define BODYFIT_TX_MAX_LEVELS (\d+)", s)
    d = re.search(r"D = (\d+) U R_t Q_t / \(P_t Lambda\)", s)
    j = re.search(r"E_J = k_J eps P_x D \(1 \+ 4 Q_t\), k_J = (\d+)", s)
    k = re.search(r"d_log = k_L eps \(1 \+ \|log2\(rho\^2\) / 2\| \+ \|lod_bias\|\), k_L = (\d+)", s)
    m = re.search(r"k_m = (\d+)", s)
    assert re.search(r"\|image\^_c - I_c\(L\)\| <= u \|I_c\| \+ kappa M \+ 2 M delta_L", s)
    assert re.search(r"\|g\^ - g\*\| <= u \|g\*\| \+ sum_l a_l m_l 2\^-\(s \+ 1\) \+ k_m eps sum_l a_l A_l", s)
    assert re.search(r"80 eps Q_t <= 1/2", s)
    return int(n.group(1)), int(d.group(1)), int(j.group(1)), int(k.group(1)), int(m.group(1))


# ---- the pyramid ---------------------------------------------------------------------------------------------------------------
def layout(Ht, Wt, max_level=-1):
    """(n_levels, [(H_l, W_l)], [texel offset of level l in the packed buffer of levels 1 .. n - 1; entry 0 is 0], its texels)"""
    sizes, off, at = [(Ht, Wt)], [0], 0
    while max_level < 0 or len(sizes) <= max_level:
        h, w = sizes[-1]
        if (h, w) == (1, 1) or (h > 1 and h % 2) or (w > 1 and w % 2):
            break
        sizes.append((max(h // 2, 1), max(w // 2, 1)))
        off.append(at)
        at += sizes[-1][0] * sizes[-1][1]
    return len(sizes), sizes, off, at


def _children(t):
    """the 4 (or 2) children arrays of every texel of the next level of t [H, W, C]"""
    H, W = t.shape[:2]
    if H > 1 and W > 1:
        return [t[0::2, 0::2], t[0::2, 1::2], t[1::2, 0::2], t[1::2, 1::2]]
    return [t[:, 0::2], t[:, 1::2]] if H == 1 else [t[0::2], t[1::2]]


def pyramid_f64(tex, max_level=-1):
    """the kernels' pyramid: [tex, level 1 f32, ...], level l + 1 from the STORED level l, ((t00 + t01) + (t10 + t11)) * 0.25 (or
    (t0 + t1) * 0.5) in f64, rounded once to f32"""
    levels = [np.asarray(tex)]
    for _ in range(layout(tex.shape[0], tex.shape[1], max_level)[0] - 1):
        c = [a.astype(np.float64) for a in _children(levels[-1])]
        with np.errstate(all="ignore"):
            v = ((c[0] + c[1]) + (c[2] + c[3])) * 0.25 if len(c) == 4 else (c[0] + c[1]) * 0.5
            levels.append(v.astype(np.float32))
    return levels


def pack(levels):
    """the packed f32 buffer of the levels 1 .. n - 1"""
    return np.concatenate([l.reshape(-1) for l in levels[1:]]).astype(np.float32) if len(levels) > 1 else np.zeros(0, np.float32)


def average_exact(tex, max_level=-1):
    """the UNROUNDED pyramid of tex in longdouble (what the texel gradient is the adjoint of)"""
    levels = [np.asarray(tex).astype(LD)]
    for _ in range(layout(tex.shape[0], tex.shape[1], max_level)[0] - 1):
        c = _children(levels[-1])
        levels.append(sum(c) / len(c))
    return levels


def fold_factors(sizes):
    """a_l, the exact product of the build's 1/4 and 1/2 factors, and per level the (row, column) shifts of a level-0 index"""
    a, sh, out = 1.0, (0, 0), [(1.0, (0, 0))]
    for (h, w) in sizes[:-1]:
        a *= 0.25 if (h > 1 and w > 1) else 0.5
        sh = (sh[0] + (h > 1), sh[1] + (w > 1))
        out.append((a, sh))
    return out


# ---- the footprint and the level of detail ----------------------------------------------------------------------------------------
def _corners(face_img, verts, faces, uv, uv_faces, live):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    uvf = np.asarray(uv_faces, np.int64).reshape(-1, 3)
    t = np.where(live, np.asarray(face_img, np.int64), 0)
    return np.asarray(verts, np.float32)[faces[t]], np.asarray(uv, np.float32).reshape(-1, 2)[uvf[t]]     # [H, W, 3, 3], [H, W, 3, 2]


class Footprint:
    """the exact footprint of one frame's live pixels: rho [H, W] (longdouble; 0 where `flat`: L = 0 by rule) and what the contract
    allows: E_J [H, W] (inf where Q_t is past the cap)"""

    def __init__(self, px, face_img, bary, verts, faces, uv, uv_faces, intr, size, tex_hw):
        H, W = px.shape
        live = ~px.void
        fx, fy, cx, cy = (LD(float(a)) for a in intr)
        Ht, Wt = tex_hw
        self.live = live
        if not live.any():
            self.rho, self.flat, self.E_J = np.zeros((H, W), LD), np.ones((H, W), bool), np.zeros((H, W), LD)
            return
        P3, A3 = _corners(face_img, verts, faces, uv, uv_faces, live)
        with np.errstate(all="ignore"):
            fin = np.isfinite(P3).all(axis=(-1, -2))
            P = np.where((live & fin)[..., None, None], P3, 1).astype(LD)
            X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
            pu, pv = fx * X / Z + cx, fy * Y / Z + cy                                          # [H, W, 3]
            A = (pu[..., 1] - pu[..., 0]) * (pv[..., 2] - pv[..., 0]) - (pu[..., 2] - pu[..., 0]) * (pv[..., 1] - pv[..., 0])
            flat = ~live | ~fin | (A == 0) | ~np.isfinite(A)
            A1 = np.where(flat, 1, A)
            b, c = [1, 2, 0], [2, 0, 1]
            gx, gy = (pv[..., b] - pv[..., c]) / A1[..., None], (pu[..., c] - pu[..., b]) / A1[..., None]
            lam = np.where(live[..., None], np.asarray(bary, np.float32).reshape(H, W, 3), 1).astype(LD)
            S = (lam / Z).sum(axis=-1)
            d = np.where(live[..., None, None], A3, 0).astype(LD) - px.uv[..., None, :]        # [H, W, 3, 2]
            hx, hy = gx / Z, gy / Z
            J = np.stack(((hx[..., None] * d).sum(axis=2), (hy[..., None] * d).sum(axis=2)), axis=-1) / S[..., None, None]   # [H, W, (u, v), (x, y)]
            J = J * np.array([Wt, Ht], LD)[:, None]
            a, bb, cc = (J[..., 0] ** 2).sum(-1), (J[..., 1] ** 2).sum(-1), (J[..., 0] * J[..., 1]).sum(-1)
            rho2 = (a + bb) / 2 + np.sqrt(((a - bb) / 2) ** 2 + cc ** 2)
            flat |= ~np.isfinite(rho2)
            self.rho = np.where(flat, 0, np.sqrt(np.where(flat, 0, rho2)))
            # the contract's terms: P_t, Q_t, R_t of the render, Lambda, U
            Pt = np.maximum(np.abs(pu), np.abs(pv)).max(axis=-1) + max(size) + max(abs(float(intr[2])), abs(float(intr[3])))
            Qt = Pt * Pt / np.abs(A1)
            Rt = Z.max(axis=-1) / Z.min(axis=-1)
            D = K_D * px.Umax * Rt * Qt / (Pt * lam.sum(axis=-1))
            E = K_J * EPS * max(Ht, Wt) * D * (1 + 4 * Qt)
            self.E_J = np.where(flat, 0, np.where(Qt <= Q_CAP, E, np.inf))
        self.flat = flat

    def lod(self, n_levels, lod_bias):
        """(L, lo, hi) [H, W] longdouble: the exact level of detail and the interval the contract allows the returned one (before
        its f32 rounding); all 0 on void and flat pixels"""
        top, bias = n_levels - 1, LD(float(lod_bias))

        def level(r, shift):
            with np.errstate(all="ignore"):
                Lr = np.log2(r) + bias
                dlog = K_L * EPS * (1 + np.abs(np.where(np.isfinite(Lr), Lr - bias, 0)) + (abs(bias) if np.isfinite(bias) else 0))
                Lr = Lr + shift * dlog
                return np.where(self.flat | ~(Lr > 0), 0, np.minimum(Lr, top))               # (a NaN, -inf + inf, is 0)
        with np.errstate(all="ignore"):
            lo = level(np.maximum(self.rho - self.E_J, 0), -1)
            hi = level(self.rho + self.E_J, +1)
        if n_levels == 1:
            z = np.zeros(self.rho.shape, LD)
            return z, z, z
        return level(self.rho, 0), lo, hi


def lod_f64(pf, face_img, bary, verts, faces, uv, uv_faces, intr, tex_hw, n_levels, lod_bias):
    """L f32 [H, W] by the arithmetic of k_texture.hip's txm_lod, operation for operation in f64; 0 on void pixels"""
    ok = pf["ok"]
    H, W = ok.shape
    if n_levels <= 1 or not ok.any():
        return np.zeros((H, W), np.float32)
    fx, fy, cx, cy = (np.float64(a) for a in intr)
    Ht, Wt = tex_hw
    P3, A3 = _corners(face_img, verts, faces, uv, uv_faces, ok)
    with np.errstate(all="ignore"):
        fin = np.isfinite(P3[..., :2]).all(axis=(-1, -2))
        P = np.where(ok[..., None, None], P3, 1).astype(np.float64)
        X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
        pu, pv = fx * (X / Z) + cx, fy * (Y / Z) + cy
        A = (pu[..., 1] - pu[..., 0]) * (pv[..., 2] - pv[..., 0]) - (pu[..., 2] - pu[..., 0]) * (pv[..., 1] - pv[..., 0])
        flat = ~ok | ~fin | ~(A != 0) | ~np.isfinite(A)
        lam = np.where(ok[..., None], np.asarray(bary, np.float32).reshape(H, W, 3), 1).astype(np.float64)
        q = lam / Z
        S = (q[..., 0] + q[..., 1]) + q[..., 2]
        b, c = [1, 2, 0], [2, 0, 1]
        hx, hy = ((pv[..., b] - pv[..., c]) / A[..., None]) / Z, ((pu[..., c] - pu[..., b]) / A[..., None]) / Z
        a3 = A3.astype(np.float64)
        du, dv = a3[..., 0] - pf["u"][..., None], a3[..., 1] - pf["v"][..., None]
        dot = lambda h, d: ((h[..., 0] * d[..., 0] + h[..., 1] * d[..., 1]) + h[..., 2] * d[..., 2]) / S
        j00, j01, j10, j11 = np.float64(Wt) * dot(hx, du), np.float64(Wt) * dot(hy, du), np.float64(Ht) * dot(hx, dv), np.float64(Ht) * dot(hy, dv)
        ca, cb, cc = j00 * j00 + j10 * j10, j01 * j01 + j11 * j11, j00 * j01 + j10 * j11
        hs, hd = 0.5 * (ca + cb), 0.5 * (ca - cb)
        rho2 = hs + np.sqrt(hd * hd + cc * cc)
        flat |= ~np.isfinite(rho2)
        Lr = 0.5 * np.log2(np.where(flat, 1.0, rho2)) + np.float64(np.float32(lod_bias))
        L = np.where(flat | ~(Lr > 0), 0.0, np.minimum(Lr, n_levels - 1.0))
    return L.astype(np.float32)


def check_lod(fp, n_levels, lod_bias, lod):
    """Asserts that the returned L (f32 [H, W]) lies in the contract's interval at EVERY pixel; returns (the exact L, delta_L)"""
    L, lo, hi = fp.lod(n_levels, np.float32(lod_bias))
    got = np.asarray(lod)
    assert got.dtype == np.float32 and got.shape == L.shape
    assert np.all(got[~fp.live] == 0), "a void pixel holds L = 0"
    g = got.astype(LD)
    ok = (g >= lo * (1 - U) - TINY) & (g <= hi * (1 + U) + TINY)
    assert np.all(ok), ("texture mip: L", int((~ok).sum()), float(np.abs(g - L)[~ok].max()))
    return L, np.maximum(np.maximum(hi - L, L - lo), np.abs(g - L))


# ---- the trilinear lookup ------------------------------------------------------------------------------------------------------
def _split(L):
    l0 = np.floor(L).astype(np.int64)
    return l0, L - l0


def lookup_f64(pf, levels, L, background):
    """the lookup by the arithmetic of k_txm_forward at the level of detail L (f32 [H, W]: the kernel rounds L to f32 before it is
    used): dict(ok, image f32, l0, f f64, weight, uv, forms: {level: texture_ref.lookup_f64's dict with "val" f64 [H, W, C] and
    "size" = (H_l, W_l) added})"""
    ok = pf["ok"]
    H, W = ok.shape
    C = levels[0].shape[2]
    l0, f = _split(np.asarray(L, np.float32).astype(np.float64))
    forms = {}
    for l in sorted(set(np.unique(l0[ok])) | set(np.unique((l0 + 1)[ok & (f != 0)]))):
        with np.errstate(all="ignore"):
            fm = tr.lookup_f64(pf, levels[l], 0.0)
            I = [levels[l][i, j].astype(np.float64) for i, j in ((fm["i0"], fm["j0"]), (fm["i0"], fm["j1"]), (fm["i1"], fm["j0"]), (fm["i1"], fm["j1"]))]
            o = fm["omega"][..., None, :]
            fm["val"] = (o[..., 0] * I[0] + o[..., 1] * I[1]) + (o[..., 2] * I[2] + o[..., 3] * I[3])
            fm["size"] = levels[l].shape[:2]
        forms[int(l)] = fm
    val = np.zeros((H, W, C))
    with np.errstate(all="ignore"):
        for l, fm in forms.items():
            one = ok & (l0 == l) & (f == 0)
            val[one] = fm["val"][one]
            two = ok & (l0 == l) & (f != 0)
            if two.any():
                ff = f[two][:, None]
                val[two] = (1.0 - ff) * fm["val"][two] + ff * forms[l + 1]["val"][two]
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    image = np.where(ok[..., None], val.astype(np.float32), np.broadcast_to(bg, (H, W, C)))
    return {"ok": ok, "image": image, "l0": np.where(ok, l0, 0), "f": np.where(ok, f, 0.0), "forms": forms,
            "weight": pf["w"].astype(np.float32), "uv": np.stack((pf["u"], pf["v"]), axis=-1).astype(np.float32)}


class Lookups:
    """texture_ref.Lookup of one frame's Pixels on every level the frame can touch (built on demand)"""

    def __init__(self, px, levels):
        self.px, self.levels, self._lk = px, levels, {}

    def __getitem__(self, l):
        if l not in self._lk:
            with np.errstate(all="ignore"):
                self._lk[l] = tr.Lookup(self.px, self.levels[l])
        return self._lk[l]

    def M(self, l, form=None):
        """the largest |texel| of level l's exact cell and, with the restated form, of its returned cell; [H, W]"""
        lk = self[l]
        return lk.M if form is None else np.maximum(lk.M, np.where(self.px.void, 0, lk.patch(form["i0"], form["j0"])[3]))


def image_exact(lks, L):
    """I(L) [H, W, C] longdouble over the stored pyramid: (1 - f) B_l0 + f B_(l0+1)"""
    px = lks.px
    l0, f = _split(L)
    out = np.zeros(px.shape + (lks.levels[0].shape[2],), LD)
    for l in np.unique(l0[~px.void]):
        sel = ~px.void & (l0 == l)
        ff = f[sel][:, None]
        hi = lks[int(l) + 1].B[sel] if (ff != 0).any() else 0
        out[sel] = np.where(ff != 0, (1 - ff) * lks[int(l)].B[sel] + ff * hi, lks[int(l)].B[sel])
    return out


def _level_range(lks, form, lo, hi):
    """M [H, W]: the largest |texel| among the exact and the returned cells of every level from floor(lo) to ceil(hi)"""
    n = len(lks.levels)
    a, b = np.floor(lo).astype(np.int64), np.minimum(np.ceil(hi).astype(np.int64), n - 1)
    M = np.zeros(lks.px.shape, LD)
    for l in range(int(a.min()), int(b.max()) + 1):
        use = (a <= l) & (l <= b) & ~lks.px.void
        if use.any():
            M = np.where(use, np.maximum(M, lks.M(l, form["forms"].get(l))), M)
    return M


def check_forward(lks, form, lod, background, image, weight=None, uv_out=None):
    """Asserts the mip lookup's image contract at EVERY pixel AT THE RETURNED L (lod f32 [H, W], itself checked by check_lod):
    |image - I(L^)| <= u |I| + kappa M, M over the levels L^ touches.  Returns the worst error in units of its bound."""
    px = lks.px
    H, W = px.shape
    C = lks.levels[0].shape[2]
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.shape == (H, W, C)
    void, live = px.void, ~px.void
    assert np.array_equal(form["ok"], live)
    bg = np.broadcast_to(np.asarray(background, np.float32), (C,))
    assert np.array_equal(image[void], np.broadcast_to(bg, image[void].shape)), "a void pixel holds the background"
    L = np.asarray(lod, np.float32).astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        I = image_exact(lks, L)
        M = _level_range(lks, form, L, L)
        err = np.abs(image.astype(LD) - I)
        lim = U * np.abs(I) + (lks[0].kappa * M)[..., None] + TINY
        fin = live[..., None] & np.isfinite(I)
        assert np.all(err[fin] <= lim[fin]), ("texture mip: image", int((err[fin] > lim[fin]).sum()), float((err[fin] / lim[fin]).max()))
        worst = float((err[fin] / lim[fin]).max()) if fin.any() else 0.0
    for got, n, want in ((weight, 3, form["weight"]), (uv_out, 2, form["uv"])):
        if got is not None:
            # (the plain lookup's outputs, by the same device function: its contract is checked where the plain lookup is)
            assert np.asarray(got).shape == (H, W, n) and np.all(np.asarray(got)[void] == 0)
    return worst


def check_forward_exact(lks, form, L_exact, delta_L, image):
    """Asserts the contract against the EXACT level of detail at EVERY pixel: |image - I(L)| <= u |I| + kappa M + 2 M delta_L, M over
    every level from floor(L - delta_L) to ceil(L + delta_L) (L_exact, delta_L: check_lod's).  Returns the worst error in units of
    its bound."""
    px = lks.px
    live = ~px.void
    with np.errstate(invalid="ignore", over="ignore"):
        I = image_exact(lks, L_exact)
        M = _level_range(lks, form, np.maximum(L_exact - delta_L, 0), L_exact + delta_L)
        err = np.abs(np.asarray(image).astype(LD) - I)
        lim = U * np.abs(I) + ((lks[0].kappa + 2 * delta_L * (1 + U)) * M)[..., None] + TINY
        fin = live[..., None] & np.isfinite(I)
        assert np.all(err[fin] <= lim[fin]), ("texture mip: image against the exact L", int((err[fin] > lim[fin]).sum()), float((err[fin] / lim[fin]).max()))
        return float((err[fin] / lim[fin]).max()) if fin.any() else 0.0


DECIDED = 2.0 ** -10       # a pixel's level of detail is DECIDED when E_J <= 2^-10 rho: delta_L is then below 2^-10 / ln 2 + d_log + u L


def decided(fp):
    """[H, W] bool: the live pixels whose footprint the contract pins down (E_J <= DECIDED rho).  A face of a body mesh in an image
    has Q_t between 2^10 and 2^18 and E_J / rho around 64 eps P_x 12 U R_t Q_t (1 + 4 Q_t) / (P_t rho) < 2^-15; only slivers in
    the image or in the atlas miss it."""
    with np.errstate(invalid="ignore", over="ignore"):
        return fp.live & ~fp.flat & (fp.E_J <= DECIDED * fp.rho)


# ---- (a) the gradient in uv ------------------------------------------------------------------------------------------------------
def grad_uv_f64(form, G):
    """d_grad_uv [H, W, 2] f32 by the arithmetic of k_txm_grad"""
    G = np.asarray(G, np.float32).astype(np.float64)
    ok, l0, f = form["ok"], form["l0"], form["f"]
    out = np.zeros(ok.shape + (2,))

    def level(l, sel):
        fm = form["forms"][l]
        su, sv = G[sel][:, 0] * fm["du"][sel][:, 0], G[sel][:, 0] * fm["dv"][sel][:, 0]
        for c in range(1, G.shape[-1]):
            su, sv = su + G[sel][:, c] * fm["du"][sel][:, c], sv + G[sel][:, c] * fm["dv"][sel][:, c]
        return np.stack((np.where(fm["free_x"][sel], su * fm["size"][1], 0.0), np.where(fm["free_y"][sel], sv * fm["size"][0], 0.0)), axis=-1)
    with np.errstate(all="ignore"):
        for l in form["forms"]:
            one = ok & (l0 == l) & (f == 0)
            if one.any():
                out[one] = level(l, one)
            two = ok & (l0 == l) & (f != 0)
            if two.any():
                ff = f[two][:, None]
                out[two] = (1.0 - ff) * level(l, two) + ff * level(l + 1, two)
    return out.astype(np.float32)


def check_grad_uv(lks, form, lod, G, grad_uv):
    """Asserts (a) at EVERY pixel at the returned L: the plain contract per level, blended.  A component that is undecided (its
    unclamped coordinate within delta of a clamp border) on a level the pixel uses may be either blend.  Returns the worst error"""
    px = lks.px
    got = np.asarray(grad_uv)
    assert got.dtype == np.float32 and got.shape == px.shape + (2,)
    assert np.all(got[px.void] == 0), "a void pixel holds a zero uv gradient"
    l0, f = _split(np.asarray(lod, np.float32).astype(LD))
    g, lim = np.zeros(got.shape, LD), np.zeros(got.shape, LD)
    loose = np.zeros(got.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for l, fm in form["forms"].items():
            gl, liml, free, und = tr.grad_uv_exact(lks[l], fm, G)
            gl = np.where(free, gl, 0)
            share = np.where(~px.void & (l0 == l), 1 - f, np.where(~px.void & (l0 + 1 == l) & (f != 0), f, 0))[..., None]
            g, lim = g + share * gl, lim + share * liml
            loose |= (share != 0) & und
        lim = lim + U * np.abs(g) + TINY
        err = np.abs(got.astype(LD) - g)
        good = loose | (err <= lim)
        assert np.all(good), ("texture mip: grad_uv", int((~good).sum()), float((err / lim)[~good].max()))
        sel = ~loose & ~px.void[..., None]
        return float((err[sel] / lim[sel]).max()) if sel.any() else 0.0


# ---- (b) the gradient in the texels ------------------------------------------------------------------------------------------------
def _scatter(forms, G, sizes, off, C, shared, one, exact):
    """the per-level sums over the frames' forms into the packed pyramid (level 0 first): exact=False the kernels' int64 sums (one:
    2^s), exact=True (g, m, A) longdouble / int64 / longdouble with exact weights at the returned cells and L"""
    F = len(forms)
    Ht, Wt = sizes[0]
    P = (Ht * Wt + sum(h * w for h, w in sizes[1:])) * C
    n = (1 if shared else F) * P
    base = [0] + [(Ht * Wt + o) * C for o in off[1:]]
    ty = LD if exact else np.float64
    acc = (np.zeros(n, LD), np.zeros(n, np.int64), np.zeros(n, LD)) if exact else np.zeros(n, np.int64)
    dest_all, q_all = [], []
    for k, form in enumerate(forms):
        Gk = np.asarray(G[k], np.float32).astype(ty)
        ok, l0, f = form["ok"], form["l0"], form["f"].astype(ty)
        for l, fm in form["forms"].items():
            Hl, Wl = sizes[l]
            for share, sel in ((None, ok & (l0 == l) & (f == 0)), (1 - f, ok & (l0 == l) & (f != 0)), (f, ok & (l0 + 1 == l) & (f != 0))):
                if not sel.any():
                    continue
                if exact:
                    a, b = fm["x"][sel].astype(LD) - fm["j0"][sel], fm["y"][sel].astype(LD) - fm["i0"][sel]
                    om = np.stack(((1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b), axis=-1)
                else:
                    om = fm["omega"][sel]
                wk = om if share is None else share[sel][:, None] * om                         # [N, 4]
                t = Gk[sel][:, None, :] * wk[:, :, None]                                        # [N, 4, C]
                i, j = (fm["i0"], fm["i0"], fm["i1"], fm["i1"]), (fm["j0"], fm["j1"], fm["j0"], fm["j1"])
                at = np.stack([(ii[sel] * Wl + jj[sel]) * C for ii, jj in zip(i, j)], axis=-1)[..., None] + np.arange(C)
                dest = (at + base[l] + (0 if shared else k * P)).reshape(-1)
                if exact:
                    t = t.reshape(-1)
                    np.add.at(acc[0], dest, t); np.add.at(acc[2], dest, np.abs(t)); np.add.at(acc[1], dest, (t != 0).astype(np.int64))
                else:
                    dest_all.append(dest); q_all.append(np.rint(t * one).astype(np.int64).reshape(-1))
    if exact:
        return acc, P, base
    return (np.concatenate(dest_all) if dest_all else np.zeros(0, np.int64)), (np.concatenate(q_all) if q_all else np.zeros(0, np.int64)), acc, P, base


def _gather(arr, sizes, C, base, P, n_tex, weight_by_a=True):
    """sum_l a_l arr_l[ancestor] in the level-0 layout [n_tex, Ht, Wt, C], in the order l = 0, 1, ... (the type of arr)"""
    Ht, Wt = sizes[0]
    i, j = np.mgrid[0:Ht, 0:Wt]
    out = None
    for l, ((a, (si, sj)), (Hl, Wl)) in enumerate(zip(fold_factors(sizes), sizes)):
        idx = ((i >> si) * Wl + (j >> sj))[..., None] * C + np.arange(C) + base[l]             # [Ht, Wt, C]
        term = np.stack([arr[k * P + idx] for k in range(n_tex)])
        term = term * a if weight_by_a else term
        out = term if out is None else out + term
    return out


def accumulate_f64(forms, G, sizes, off, C, shared, order=None):
    """k_txm_grad's integer sums and k_txm_fold over the frames' forms: (grad_tex f32 in the level-0 layout, the int64 workspace, s)"""
    G = np.asarray(G, np.float32)
    F = len(forms)
    s, gbits = tr.scale_exponent(G, G.size // C)
    dest, q, sums, P, base = _scatter(forms, G, sizes, off, C, shared, np.ldexp(1.0, s) if 0 < gbits < 0x7f800000 else 0.0, False)
    n_tex = 1 if shared else F
    shape = sizes[0] + (C,) if shared else (F,) + sizes[0] + (C,)
    if gbits >= 0x7f800000:
        return np.full(shape, np.nan, np.float32), sums, s
    if gbits:
        if order is not None:
            dest, q = dest[order], q[order]
        np.add.at(sums, dest, q)
    g = _gather(sums.astype(np.float64) * np.ldexp(1.0, -s), sizes, C, base, P, n_tex)
    return g.astype(np.float32).reshape(shape), sums, s


def grad_tex_exact(forms, G, sizes, off, C, shared):
    """(g*, the bound's sum_l a_l m_l, sum_l a_l A_l) per level-0 texel element, longdouble"""
    (g, m, A), P, base = _scatter(forms, G, sizes, off, C, shared, None, True)
    n_tex = 1 if shared else len(forms)
    shape = sizes[0] + (C,) if shared else (len(forms),) + sizes[0] + (C,)
    return tuple(_gather(a.astype(LD), sizes, C, base, P, n_tex).reshape(shape) for a in (g, m, A))


def check_grad_tex(forms, G, sizes, off, C, shared, grad_tex):
    """Asserts (b) at EVERY level-0 texel element (forms at the RETURNED L); returns the worst error in units of its bound"""
    got = np.asarray(grad_tex)
    s, gbits = tr.scale_exponent(G, np.asarray(G).size // C)
    assert got.dtype == np.float32
    if gbits >= 0x7f800000:
        assert np.isnan(got).all(), "a non-finite upstream gradient gives an all-NaN texel gradient"
        return 0.0
    g, m, A = grad_tex_exact(forms, G, sizes, off, C, shared)
    assert got.shape == g.shape
    err = np.abs(got.astype(LD) - g)
    lim = U * np.abs(g) + m * np.ldexp(LD(1), -(s + 1)) + K_M * EPS * A + TINY
    assert np.all(err <= lim), ("texture mip: grad_tex", int((err > lim).sum()), float((err / lim).max()))
    return float((err / lim).max())
