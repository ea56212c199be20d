"""Test infrastructure (numpy): the reference statement of the interpolation rows (bodyfit_raster_interp_rows_device) and of
their contract in include/bodyfit.h, on the scenes and with the machinery of depth_rows_ref.py and raster_ref.py.

ONE routine, evaluate(), states both the definition (np.longdouble, every h_a formed on its own: 2^-11 of the f64 the kernel
works in) and the kernel's own operation order (np.float64: numpy never fuses).  Everything works on ONE frame: verts [V, 3] f32,
faces [nf, 3] int, intr = (fx, fy, cx, cy), size = (H, W), a face-id image [H, W] int, optionally a list of linear pixel
indices, attr [V, C] f32 (C = 0: None), the upstream gradients G [H, W, C] f32 and gz [H, W] f32 or None."""
import re

import numpy as np

import depth_rows_ref as dr

LD = np.longdouble
U = 2.0 ** -24
K_I = 2                     # the constants of include/bodyfit.h (bodyfit_raster_interp_rows_device) ...
KAPPA_D_SHIFT = 2.0 ** -19  # ... kappa_d = 2^-19 rho Q / c
SHADE_TAU = 5               # ... AGAINST THE SHADE: 5 tau_t R_t A_ch


def header_constants(text):
    """(k_i, the shift of kappa_d, the factor of tau_t R_t against the shade) as include/bodyfit.h states them"""
    s = text[text.index("INTERPOLATION ROWS"):]
    k = re.search(r"u = 2\^-24, k_i = (\d+), P, L, Q, rho, c and kappa_b of the depth rows", s)
    d = re.search(r"kappa_d = 2\^-(\d+) rho Q / c", s)
    t = re.search(r"k_s u T_ch \+ (\d+) tau_t R_t A_ch", s)
    return int(k.group(1)), int(d.group(1)), int(t.group(1))


def inputs(n_verts, size, n_channels, seed=0):
    """(attr [V, C] f32 or None, G [H, W, C] f32 or None, gz [H, W] f32): the same random numbers whatever C, so the channels of a
    smaller C are the first ones of a larger"""
    rng = np.random.default_rng(seed)
    H, W = size
    attr = rng.uniform(-1.0, 2.0, size=(n_verts, 4)).astype(np.float32)
    G = rng.standard_normal((H, W, 4)).astype(np.float32)
    gz = rng.standard_normal((H, W)).astype(np.float32)
    if n_channels == 0:
        return None, None, gz
    return np.ascontiguousarray(attr[:, :n_channels]), np.ascontiguousarray(G[:, :, :n_channels]), gz


def evaluate(dtype, verts, faces, intr, size, face_img, pixel=None, attr=None, G=None, gz=None):
    """The rows in `dtype`.  np.float64: k_rs_interp_rows operation for operation (the depth rows' order up to beta and m, then s_a,
    the differences against s_0, E, w, k, a, dir; value from the unrounded beta).  np.longdouble: the DEFINITION, dir = g_z m -
    sum_a s_a h_a with every h_a formed on its own, and the quantities the contract's bounds are made of.  Returns a dict:
    ok [N] (the evaluation keeps the row), t [N], beta [N, 3], dir [N, 3], value [N, C], and in longdouble also m, z, s, sigma
    [N, 3], abs_h [N, 3], A [N, 3, C]."""
    H, W = size
    definition = dtype is LD
    fx, fy, cx, cy = (dtype(float(a)) for a in intr)
    pix, t, corners, live = dr._gather(verts, faces, size, face_img, pixel)
    N = len(pix)
    C = 0 if attr is None else attr.shape[1]
    v = corners.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        n = dr._cross(e1, e2)
        i, j = pix // W, pix - (pix // W) * W
        dx, dy = (j.astype(dtype) - cx) / fx, (i.astype(dtype) - cy) / fy
        d = np.stack((dx, dy, np.ones(N, dtype)), axis=-1)
        D = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2]
        nn = dr._dot(n, n)
        ok = live & (nn > 0) & (D != 0)
        Ds, nns = np.where(ok, D, 1), np.where(ok, nn, 1)
        z = dr._dot(n, v[:, 0]) / Ds
        x = np.stack((z * dx, z * dy, z), axis=-1)
        inv = 1 / nns
        beta = np.stack([dr._dot(n, dr._cross(v[:, (a + 1) % 3] - x, v[:, (a + 2) % 3] - x)) * inv for a in range(3)], axis=-1)
        m = n / Ds[:, None]
        at = np.clip(pix, 0, H * W - 1)
        out = dict(ok=ok, t=t, pix=pix, beta=beta)
        r = np.zeros((N, 3), dtype)
        if gz is not None:
            g = np.asarray(gz, np.float32).reshape(-1)[at].astype(dtype)
            r = g[:, None] * m
        value = np.zeros((N, C), dtype)
        if C > 0:
            ids = np.asarray(faces, np.int64).reshape(-1, 3)[np.clip(t, 0, None)] if len(np.asarray(faces)) else np.zeros((N, 3), np.int64)
            A = np.asarray(attr, np.float32)[ids].astype(dtype)                          # [N, corner, C]
            Gp = np.asarray(G, np.float32).reshape(-1, C)[at].astype(dtype)             # [N, C]
            s, sigma = [], []
            for k in range(3):
                acc, ab = Gp[:, 0] * A[:, k, 0], np.abs(Gp[:, 0] * A[:, k, 0])
                for ch in range(1, C):
                    acc = acc + Gp[:, ch] * A[:, k, ch]
                    ab = ab + np.abs(Gp[:, ch] * A[:, k, ch])
                s.append(acc)
                sigma.append(ab)
            value = (beta[:, 0:1] * A[:, 0] + beta[:, 1:2] * A[:, 1]) + beta[:, 2:3] * A[:, 2]
            if definition:
                a3 = np.zeros((N, 3), dtype)
                abs_h = []
                for a in range(3):
                    g_a = dr._cross(n, v[:, (a + 2) % 3] - v[:, (a + 1) % 3]) * inv[:, None]
                    h_a = g_a - dr._dot(g_a, d)[:, None] * m
                    a3 = a3 + s[a][:, None] * h_a
                    abs_h.append(np.sqrt(dr._dot(h_a, h_a)))
                out.update(s=np.stack(s, axis=-1), sigma=np.stack(sigma, axis=-1), abs_h=np.stack(abs_h, axis=-1), A=A)
            else:
                p, q = s[1] - s[0], s[2] - s[0]
                E = q[:, None] * e1 - p[:, None] * e2
                w = dr._cross(n, E) * inv[:, None]
                kk = (w[:, 0] * dx + w[:, 1] * dy) + w[:, 2]
                a3 = w - kk[:, None] * m
            r = r - a3 if gz is not None else -a3
        out.update(dir=r, value=value, m=m, z=z, d=d)
    return out


class InterpRows:
    """the exact rows of one frame and what the contract allows around them; .rows is the depth_rows_ref.Rows of the same rows
    (index, beta, the void rules, kappa, kappa_b)"""

    def __init__(self, verts, faces, intr, size, face_img, pixel=None, attr=None, G=None, gz=None):
        self.rows = rows = dr.Rows(verts, faces, intr, size, face_img, pixel)
        e = evaluate(LD, verts, faces, intr, size, face_img, pixel, attr, G, gz)
        ok = ~rows.void
        assert np.array_equal(e["ok"], ok)
        N, C = len(rows.pix), 0 if attr is None else attr.shape[1]
        self.C, self.void, self.pix, self.face = C, rows.void, rows.pix, rows.face
        self.beta = rows.beta
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.all(np.abs(np.where(ok[:, None], e["beta"], 0) - rows.beta) <= 2.0 ** -50 * np.maximum(1, np.abs(rows.beta)) * (1 + rows.kappa_b[:, None]))
            self.dir = np.where(ok[:, None], e["dir"], 0)
            self.value = np.where(ok[:, None], e["value"], 0)
            abs_m = rows.abs_m
            gzp = np.zeros(N, LD) if gz is None else np.abs(np.asarray(gz, np.float32).reshape(-1)[np.clip(rows.pix, 0, size[0] * size[1] - 1)].astype(LD))
            T = gzp * abs_m
            T1 = T.copy()
            if C > 0:
                T = T + (np.abs(e["s"]) * e["abs_h"]).sum(axis=1)
                T1 = T1 + (e["sigma"] * e["abs_h"]).sum(axis=1)
                self.V = (np.abs(rows.beta)[:, :, None] * np.abs(e["A"])).sum(axis=1).astype(np.float64)        # [N, C]
                self.A = np.abs(e["A"]).sum(axis=1).astype(np.float64)
            else:
                self.V = self.A = np.zeros((N, 0))
            self.T, self.T1 = np.where(ok, T, 0).astype(np.float64), np.where(ok, T1, 0).astype(np.float64)
            self.kappa_d = np.where(ok, KAPPA_D_SHIFT * rows.rho * rows.Q / np.where(ok, rows.cos, 1), np.inf)
            self.dir_tol = np.where(ok, K_I * U * self.T + self.kappa_d * U * self.T1, np.inf)
            bmax = np.maximum(1.0, np.abs(rows.beta).max(axis=1).astype(np.float64))
            self.value_tol = np.where(ok[:, None], K_I * U * self.V + (rows.kappa_b * U * bmax)[:, None] * self.A, np.inf)
        self.gz_abs = gzp.astype(np.float64)


def check_rows(ref, index, bary=None, direction=None, value=None):
    """Asserts the contract for EVERY row of one frame's outputs: index and bary by depth_rows_ref.check_rows (they ARE the depth
    rows'), direction within k_i u T + kappa_d u T_1 and value within its bound on every row both keep, zeros on every void row;
    a row whose attributes or upstream gradients are not finite is kept and holds a non-finite direction.  Returns the worst
    (bary, direction, value) errors in units of their bounds."""
    index = np.asarray(index)
    worst_b = dr.check_rows(ref.rows, index, None, bary, None)[1]
    out_void = index < 0
    both = ~out_void & ~ref.void
    worst = [worst_b, 0.0, 0.0]
    N = len(ref.pix)
    with np.errstate(invalid="ignore", over="ignore"):
        if direction is not None:
            direction = np.asarray(direction)
            assert direction.dtype == np.float32 and direction.shape == (N, 3)
            assert np.all(direction[out_void] == 0), "a void row holds a zero direction"
            finite = both & np.isfinite(ref.dir.astype(np.float64)).all(axis=1) & np.isfinite(ref.dir_tol)
            wild = both & ~finite
            assert not np.isfinite(direction[wild]).all(axis=1).any(), "a NaN attribute or gradient gives a non-finite direction"
            err = np.abs(direction[finite].astype(LD) - ref.dir[finite]).max(axis=1).astype(np.float64)
            lim = ref.dir_tol[finite]
            assert np.all(err <= lim), ("dir", float((err[lim > 0] / lim[lim > 0]).max()), int((err > lim).sum()))
            worst[1] = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
        if value is not None:
            value = np.asarray(value)
            assert value.dtype == np.float32 and value.shape == (N, ref.C)
            assert np.all(value[out_void] == 0), "a void row holds a zero value"
            finite = both[:, None] & np.isfinite(ref.value_tol) & np.isfinite(ref.value.astype(np.float64))
            err = np.abs(value.astype(LD) - ref.value).astype(np.float64)
            assert np.all(err[finite] <= ref.value_tol[finite]), ("value", float((err[finite] / ref.value_tol[finite]).max()))
            pos = finite & (ref.value_tol > 0)
            worst[2] = float((err[pos] / ref.value_tol[pos]).max()) if pos.any() else 0.0
    return tuple(worst)


def kernel_form_f64(verts, faces, intr, size, face_img, pixel=None, attr=None, G=None, gz=None):
    """(index int32 [N], bary f32 [N, 3], direction f32 [N, 3], value f32 [N, C]) by the arithmetic of k_rs_interp_rows in f64"""
    e = evaluate(np.float64, verts, faces, intr, size, face_img, pixel, attr, G, gz)
    ok = e["ok"]
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.where(ok, e["t"], -1).astype(np.int32), np.where(ok[:, None], e["beta"], 0).astype(np.float32),
                np.where(ok[:, None], e["dir"], 0).astype(np.float32), np.where(ok[:, None], e["value"], 0).astype(np.float32))


def exact_loss_at(verts, faces, intr, size, t, pix, attr_rows, G_row, gz):
    """L = sum_ch G_ch I_ch + g_z z in longdouble at the FIXED face t and linear pixel pix, for the vertices `verts` (any float
    dtype, used as given); attr_rows [3, C] the face's attribute rows (or None), G_row [C], gz a number (0: no depth part)"""
    H, W = size
    fx, fy, cx, cy = (LD(float(a)) for a in intr)
    v = np.asarray(verts).astype(LD)[np.asarray(faces, np.int64).reshape(-1, 3)[t]]
    n = dr._cross(v[1] - v[0], v[2] - v[0])
    i, j = pix // W, pix % W
    d = np.array([(LD(j) - cx) / fx, (LD(i) - cy) / fy, LD(1)])
    z = dr._dot(n, v[0]) / dr._dot(n, d)
    x = z * d
    L = LD(float(gz)) * z
    if attr_rows is not None:
        beta = np.array([dr._dot(n, dr._cross(v[(a + 1) % 3] - x, v[(a + 2) % 3] - x)) for a in range(3)]) / dr._dot(n, n)
        L = L + (np.asarray(G_row).astype(LD) * (beta[:, None] * np.asarray(attr_rows).astype(LD)).sum(axis=0)).sum()
    return L


def composed_gradient(ref, faces, n_verts):
    """The two contracts composed, for one frame: (G, bound, T) [V, 3] f64.  G: the exact vertex gradient sum_i beta_ia dir_i at
    faces[index_i][a] (coef = 1); T: the same sum of absolute values; bound: what the f32 rows (each beta within the depth rows'
    b_tol, each dir_c within dir_tol) followed by the rows VJP (depth_rows_ref.K_VJP u T of the perturbed rows) may differ from G
    by.  Void rows contribute nothing; rows with a non-finite direction make their vertices' entries non-finite."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = ~ref.void
    b, m = ref.beta[keep], ref.dir[keep]
    db, dm = ref.rows.b_tol[keep].astype(LD)[:, None], ref.dir_tol[keep].astype(LD)[:, None]
    ids = faces[ref.face[keep]]
    G, B, T = np.zeros((n_verts, 3), LD), np.zeros((n_verts, 3), LD), np.zeros((n_verts, 3), LD)
    for a in range(3):
        ba = b[:, a:a + 1]
        np.add.at(G, ids[:, a], ba * m)
        np.add.at(T, ids[:, a], np.abs(ba * m))
        first = np.abs(ba) * dm + np.abs(m) * db + db * dm
        vjp = dr.K_VJP * U * (np.abs(ba) + db) * (np.abs(m) + dm)
        np.add.at(B, ids[:, a], first + vjp)
    return G.astype(np.float64), B.astype(np.float64), T.astype(np.float64)


def exact_gradient_of_rows(faces, n_verts, index, bary, direction):
    """(G*, T) of depth_rows_ref.vjp_exact for f32 rows with coef = 1: what the rows VJP must return for THESE rows"""
    return dr.vjp_exact(faces, n_verts, index, bary, np.ones(len(np.asarray(index)), np.float32), direction)


def wall_scene(shift_px=0.4):
    """A 9 x 9-vertex grid at z = 2 that overhangs a 32 x 32 image on all sides, colours a smooth function of the rest position:
    (verts_rest [81, 3] f32, verts_shifted (the grid moved by shift_px pixels along x and 0.6 of that along y), faces [128, 3], intr,
    size, colours [81, 3] f32).  No silhouette falls into the image: only interior gradients can see the shift."""
    intr, size = (40.0, 40.0, 15.5, 15.5), (32, 32)
    g = np.linspace(-1.2, 1.2, 9)
    X, Y = np.meshgrid(g, g)
    rest = np.stack((X.reshape(-1), Y.reshape(-1), np.full(81, 2.0)), axis=1).astype(np.float32)
    faces = []
    for r in range(8):
        for c in range(8):
            a = 9 * r + c
            faces += [[a, a + 1, a + 10], [a, a + 10, a + 9]]
    colours = np.stack((np.sin(2.1 * rest[:, 0]) + 0.5 * rest[:, 1], np.cos(1.7 * rest[:, 1]) - 0.3 * rest[:, 0],
                        0.6 * rest[:, 0] * rest[:, 1] + np.sin(1.3 * (rest[:, 0] + rest[:, 1]))), axis=1).astype(np.float32)
    dz = 2.0 / intr[0] * shift_px
    moved = (rest.astype(np.float64) + [dz, 0.6 * dz, 0.0]).astype(np.float32)
    return rest, moved, np.array(faces, np.int32), intr, size, colours
