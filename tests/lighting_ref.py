"""Test infrastructure (numpy): the reference statement of the lighting (bodyfit_raster_light_device, its gradients
bodyfit_raster_light_grad_device) and of the vertex normals' adjoint (bodyfit_surface_vertex_normals_vjp_device), of their
contracts in include/bodyfit.h, and the restatement of each kernel's arithmetic in f64 with f32 stores.

The definitions are evaluated in extended precision (np.longdouble, as appearance_ref does) from the f32 inputs.  The lighting
functions work on ONE frame: a face-id image [H, W] int, its weights [H, W, 3] f32, verts [V, 3] f32, faces [nf, 3] int, normals
[V, 3] f32, albedo [H, W, C] f32, light [9, C] f32."""
import re

import numpy as np

import appearance_ref as ar

LD = np.longdouble
U = 2.0 ** -24
EPS = 2.0 ** -53
TINY = 2.0 ** -150
K_L, K_C, K_M, K_R0, K_V, K_N = 16, 256, 4096, 80, 128, 32       # the constants of include/bodyfit.h (header_constants reads them)


def header_constants(text):
    """(k_l, k_c, k_m, k_r0, k_v, the constant of the normal's bound) as include/bodyfit.h states them"""
    s = text[text.index("LIGHTING OF A RENDER"):]
    a = re.search(r"eps = 2\^-53, k_l = (\d+), k_c = (\d+) and per lit pixel", s)
    n = re.search(r"\|normal\^ - n\| <= u \+ (\d+) eps c per component", s)
    g = re.search(r"k_m = (\d+), k_r0 = (\d+), Q = ", s)
    assert re.search(r"\(k_r0 \+ n_chunks\) \|b_k\| \+ k_c c\)", s)
    v = text[text.index("THE VERTEX NORMALS' ADJOINT"):]
    k = re.search(r"eps = 2\^-53, k_v = (\d+), c_i of the forward", v)
    return int(a.group(1)), int(a.group(2)), int(g.group(1)), int(g.group(2)), int(k.group(1)), int(n.group(1))


def layout(ppf):
    """(P, the chunks per frame) of the gradient's reduction: chunks of 256 P pixels, P the smallest power of two with at most 256
    chunks, at most 64 (k_light.hip's lt_layout; api.light_grad_layout returns 256 P and the chunks)"""
    P = 1
    while P < 64 and (ppf + 256 * P - 1) // (256 * P) > 256:
        P *= 2
    return P, (ppf + 256 * P - 1) // (256 * P) if ppf > 0 else 0


def basis(n):
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return np.stack((np.ones_like(x), x, y, z, x * y, x * z, y * z, x * x - y * y, 3 * (z * z) - 1), axis=-1)


def basis_pull(n, q):
    """sum_k q_k grad b_k(n), in the kernel's order of operations"""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    gx = ((q[..., 1] + y * q[..., 4]) + z * q[..., 5]) + (2 * x) * q[..., 7]
    gy = ((q[..., 2] + x * q[..., 4]) + z * q[..., 6]) - (2 * y) * q[..., 7]
    gz = ((q[..., 3] + x * q[..., 5]) + y * q[..., 6]) + (6 * z) * q[..., 8]
    return np.stack((gx, gy, gz), axis=-1)


def _corner_normals(face_img, faces, normals):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    face_img = np.asarray(face_img, np.int64)
    inside = (face_img >= 0) & (face_img < len(faces))
    if len(faces) == 0:
        return np.zeros(face_img.shape + (3, 3), np.float32)
    return np.asarray(normals, np.float32)[faces[np.where(inside, face_img, 0)]]         # [H, W, 3 corners, 3]


# ---- the lighting ------------------------------------------------------------------------------------------------------------------
def light_exact(face_img, bary, verts, faces, normals, albedo, light):
    """the definition in long double: dict(lit [H, W], n, l, c, b [H, W, 9], s [H, W, C], image [H, W, C])"""
    albedo, light = np.asarray(albedo, np.float32), np.asarray(light, np.float32)
    void, w, _, _ = ar.shade_exact(face_img, bary, verts, faces, np.zeros((len(verts), 1), np.float32))
    na = _corner_normals(face_img, faces, normals)
    with np.errstate(all="ignore"):
        fin = np.isfinite(na).all(axis=(-1, -2))
        nl = np.where(fin[..., None, None], na, 0).astype(LD)
        m = (w[..., None] * nl).sum(axis=2)
        l = np.sqrt((m * m).sum(axis=-1))
        lit = ~void & fin & np.isfinite(l) & (l != 0)
        l1 = np.where(lit, l, 1)
        n = np.where(lit[..., None], m / l1[..., None], 0)
        c = np.where(lit, (w * np.sqrt((nl * nl).sum(axis=-1))).sum(axis=-1) / l1, 0)
        b = basis(n)
        s = np.where(lit[..., None], b @ light.astype(LD), 0)
        image = np.where(lit[..., None], albedo.astype(LD) * s, albedo.astype(LD))
    return dict(lit=lit, n=n, l=l1, c=c, b=b, s=s, image=image, albedo=albedo, light=light)


def light_f64(face_img, bary, verts, faces, normals, albedo, light):
    """the arithmetic of k_lt_forward, operation for operation in f64 (numpy never fuses), the stores rounded to f32:
    dict(image, normal, shading f32; lit, n, l, b, s f64)"""
    albedo, light = np.asarray(albedo, np.float32), np.asarray(light, np.float32)
    H, W, C = albedo.shape
    faces_ = np.asarray(faces, np.int64).reshape(-1, 3)
    fi = np.asarray(face_img, np.int64)
    inside = (fi >= 0) & (fi < len(faces_))
    lam = np.asarray(bary, np.float32).reshape(H, W, 3)
    with np.errstate(all="ignore"):
        if len(faces_):
            Z = np.asarray(verts, np.float32)[faces_[np.where(inside, fi, 0)], 2]
            ok = inside & np.isfinite(lam).all(axis=-1) & np.isfinite(Z).all(axis=-1) & (Z > 0).all(axis=-1) & (lam >= 0).all(axis=-1)
            q = np.where(ok[..., None], lam, 0).astype(np.float64) / np.where(ok[..., None], Z, 1).astype(np.float64)
            S = (q[..., 0] + q[..., 1]) + q[..., 2]
            ok &= S != 0
            w = q / np.where(ok, S, 1)[..., None]
        else:
            ok, w = np.zeros((H, W), bool), np.zeros((H, W, 3))
        na = _corner_normals(face_img, faces, normals)
        fin = np.isfinite(na).all(axis=(-1, -2))
        nd = np.where(fin[..., None, None], na, 0).astype(np.float64)
        m = (w[..., 0, None] * nd[..., 0, :] + w[..., 1, None] * nd[..., 1, :]) + w[..., 2, None] * nd[..., 2, :]
        l = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        lit = ok & fin & np.isfinite(l) & (l != 0)
        l1 = np.where(lit, l, 1.0)
        n = np.where(lit[..., None], m / l1[..., None], 0.0)
        b = basis(n)
        L = light.astype(np.float64)
        s = L[0][None, None, :] * b[..., 0, None]
        for k in range(1, 9):
            s = s + L[k][None, None, :] * b[..., k, None]
        s = np.where(lit[..., None], s, 0.0)
        image = np.where(lit[..., None], (albedo.astype(np.float64) * s).astype(np.float32), albedo)
    return dict(image=image.astype(np.float32), normal=n.astype(np.float32), shading=s.astype(np.float32), lit=lit, n=n, l=l1, b=b, s=s,
                albedo=albedo, light=light)


def light_bound(ex):
    """the contract's bound on |image^ - image| [H, W, C] (and on the shading: the same without albedo) of light_exact's pixels"""
    absL = np.abs(ex["light"]).astype(LD)
    t2 = np.abs(ex["b"]) @ absL
    t3 = ex["c"][..., None] * absL[1:].sum(axis=0)[None, None, :]
    shading = U * np.abs(ex["s"]) + K_L * EPS * t2 + K_C * EPS * t3 + TINY
    image = U * np.abs(ex["image"]) + np.abs(ex["albedo"]).astype(LD) * (K_L * EPS * t2 + K_C * EPS * t3) + TINY
    return image, shading


def _worst(err, lim, mask, what):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bad = mask & ~(err <= lim)
        assert not bad.any(), (what, int(bad.sum()), float(np.where(mask & (lim > 0), err / np.where(lim > 0, lim, 1), 0).max()))
        return float(np.where(mask & (lim > 0), err / np.where(lim > 0, lim, 1), 0).max()) if mask.any() else 0.0


def check_light(ex, image, normal=None, shading=None):
    """Asserts the lighting contract at EVERY pixel of one frame's outputs.  Returns the worst error in units of its bound."""
    lit = ex["lit"]
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.shape == ex["albedo"].shape
    assert np.array_equal(image[~lit].view(np.int32), ex["albedo"][~lit].view(np.int32)), "an unlit pixel keeps its albedo, bit for bit"
    lim_i, lim_s = light_bound(ex)
    m3 = np.broadcast_to(lit[..., None], image.shape)
    worst = _worst(np.abs(image.astype(LD) - ex["image"]), lim_i, m3, "light: image")
    if shading is not None:
        shading = np.asarray(shading)
        assert shading.dtype == np.float32 and np.all(shading[~lit] == 0), "an unlit pixel has shading 0"
        worst = max(worst, _worst(np.abs(shading.astype(LD) - ex["s"]), lim_s, m3, "light: shading"))
    if normal is not None:
        normal = np.asarray(normal)
        assert normal.dtype == np.float32 and np.all(normal[~lit] == 0), "an unlit pixel has normal 0"
        lim = np.broadcast_to((U + K_N * EPS * ex["c"])[..., None], normal.shape)
        worst = max(worst, _worst(np.abs(normal.astype(LD) - ex["n"]), lim, np.broadcast_to(lit[..., None], normal.shape), "light: normal"))
    return worst


# ---- its gradients -----------------------------------------------------------------------------------------------------------------
def grad_exact(ex, G):
    """(grad_albedo [H, W, C], grad_m [H, W, 3], grad_light [9, C]) of the definition in long double, with their bounds but for
    the reduction's n_chunks term: (ga, gm, gl, lim_a, lim_m, sum |t| |b_k| [9, C], sum |t| c [C])"""
    G = np.asarray(G, np.float32).astype(LD)
    lit, n, l, c, b, s = (ex[k] for k in ("lit", "n", "l", "c", "b", "s"))
    L = ex["light"].astype(LD)
    with np.errstate(all="ignore"):
        ga = np.where(lit[..., None], G * s, G)
        t = np.where(lit[..., None], G * ex["albedo"].astype(LD), 0)                 # [H, W, C]
        q = t @ L.T                                                                # [H, W, 9]
        gn = basis_pull(n, q)
        gm = np.where(lit[..., None], (gn - n * (n * gn).sum(axis=-1, keepdims=True)) / l[..., None], 0)
        gl = np.einsum("hwc,hwk->kc", t, np.where(lit[..., None], b, 0))
        absL = np.abs(L)
        t2 = np.abs(b) @ absL
        t3 = c[..., None] * absL[1:].sum(axis=0)[None, None, :]
        lim_a = np.where(lit[..., None], U * np.abs(ga) + np.abs(G) * (K_L * EPS * t2 + K_C * EPS * t3), 0) + TINY
        Q = (np.abs(t) @ absL[1:].T).sum(axis=-1)
        lim_m = U * np.abs(gm) + (K_M * EPS * c * Q / l)[..., None] + TINY
        sum_tb = np.einsum("hwc,hwk->kc", np.abs(t), np.where(lit[..., None], np.abs(b), 0))
        sum_tc = (np.abs(t) * c[..., None]).sum(axis=(0, 1))
    return ga, gm, gl, lim_a, lim_m, sum_tb, sum_tc


def grad_f64(form, G):
    """the arithmetic of k_lt_grad and k_lt_light_sum in f64 with f32 stores: (grad_albedo, grad_m, grad_light [9, C]) f32; the
    reduction in the kernels' order (a thread's pixels in ascending order, the butterfly, the waves, the chunks)"""
    G = np.asarray(G, np.float32).astype(np.float64)
    lit, n, l, b, s = (form[k] for k in ("lit", "n", "l", "b", "s"))
    L = form["light"].astype(np.float64)
    H, W, C = G.shape
    with np.errstate(all="ignore"):
        ga = np.where(lit[..., None], G * s, G)
        t = G * form["albedo"].astype(np.float64)
        q = np.zeros((H, W, 9))
        for k in range(1, 9):
            a = t[..., 0] * L[k, 0]
            for c in range(1, C):
                a = a + t[..., c] * L[k, c]
            q[..., k] = a
        gn = basis_pull(n, q)
        d = (n[..., 0] * gn[..., 0] + n[..., 1] * gn[..., 1]) + n[..., 2] * gn[..., 2]
        gm = np.where(lit[..., None], (gn - n * d[..., None]) / l[..., None], 0.0)
        terms = np.where(lit[..., None, None], t[..., None, :] * b[..., :, None], 0.0).reshape(H * W, 9 * C)
    P, chunks = layout(H * W)
    x = np.zeros((chunks * P * 256, 9 * C))
    x[:H * W] = terms
    x = x.reshape(chunks, P, 4, 64, 9 * C)
    with np.errstate(all="ignore"):
        acc = np.zeros((chunks, 4, 64, 9 * C))
        for i in range(P):
            acc = acc + x[:, i]
        lane = np.arange(64)
        for dd in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lane ^ dd]
        part = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]           # [chunks, 9 C]
        tot = part[0]
        for ch in range(1, chunks):
            tot = tot + part[ch]
    return ga.astype(np.float32), gm.astype(np.float32), tot.reshape(9, C).astype(np.float32)


def check_grad(ex, G, grad_albedo=None, grad_m=None, grad_light=None):
    """Asserts the gradient contracts on every pixel and every coefficient of one frame.  Returns the worst errors in units of
    their bounds (albedo, m, light)."""
    ga, gm, gl, lim_a, lim_m, sum_tb, sum_tc = grad_exact(ex, G)
    H, W, C = ga.shape
    worst = [0.0, 0.0, 0.0]
    if grad_albedo is not None:
        got = np.asarray(grad_albedo)
        assert got.dtype == np.float32 and got.shape == ga.shape
        unlit = ~ex["lit"]
        assert np.array_equal(got[unlit].view(np.int32), np.asarray(G, np.float32)[unlit].view(np.int32)), "an unlit pixel passes G through"
        worst[0] = _worst(np.abs(got.astype(LD) - ga), lim_a, np.ones(ga.shape, bool), "light grad: albedo")
    if grad_m is not None:
        got = np.asarray(grad_m)
        assert got.dtype == np.float32 and got.shape == gm.shape and np.all(got[~ex["lit"]] == 0)
        worst[1] = _worst(np.abs(got.astype(LD) - gm), lim_m, np.ones(gm.shape, bool), "light grad: m")
    if grad_light is not None:
        got = np.asarray(grad_light)
        assert got.dtype == np.float32 and got.shape == (9, C)
        _, chunks = layout(H * W)
        lim = U * np.abs(gl) + EPS * ((K_R0 + chunks) * sum_tb + K_C * sum_tc[None, :]) + TINY
        worst[2] = _worst(np.abs(got.astype(LD) - gl), lim, np.ones(gl.shape, bool), "light grad: light")
    return tuple(worst)


# ---- the vertex normals' adjoint -----------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def _normal_sums(v, faces, dtype):
    """(s [V, 3], sum |N_t| [V], has a face [V]) of one frame, every face once per vertex in ascending (face, corner) order"""
    V = len(v)
    s, sa, has = np.zeros((V, 3), dtype), np.zeros(V, dtype), np.zeros(V, bool)
    x = v.astype(dtype)
    with np.errstate(all="ignore"):
        N = _cross(x[faces[:, 1]] - x[faces[:, 0]], x[faces[:, 2]] - x[faces[:, 0]])
        Nn = np.sqrt((N * N).sum(axis=-1))
    for t, ids in enumerate(faces):
        for a in range(3):
            if ids[a] in ids[:a]:
                continue
            with np.errstate(all="ignore"):
                s[ids[a]] += N[t]
                sa[ids[a]] += Nn[t]
            has[ids[a]] = True
    return s, sa, has


def _normals_vjp(verts, faces, g, dtype):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    v = np.asarray(verts, np.float32)
    V = len(v)
    s, sa, has = _normal_sums(v, faces, dtype)
    x = v.astype(dtype)
    gg = np.asarray(g, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        l = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        ok = has & np.isfinite(l) & (l > 0)
        l1 = np.where(ok, l, 1)
        n = np.where(ok[:, None], s / l1[:, None], 0)
        d = (n[:, 0] * gg[:, 0] + n[:, 1] * gg[:, 1]) + n[:, 2] * gg[:, 2]
        h = np.where(ok[:, None], (gg - n * d[:, None]) / l1[:, None], 0)
        ci = np.where(ok, sa / l1, 0)
        hb = np.where(ok, ci * np.sqrt((gg * gg).sum(axis=-1)) / l1, 0)               # c_i |g_i| / |s_i|
    out, lim = np.zeros((V, 3), dtype), np.zeros(V, dtype)
    for t, ids in enumerate(faces):
        if ids[0] == ids[1] or ids[1] == ids[2] or ids[0] == ids[2]:
            continue
        a_t = (h[ids[0]] + h[ids[1]]) + h[ids[2]]
        if not a_t.any():
            continue
        A_t = hb[ids].sum()
        for a in range(3):
            e = x[ids[(a + 1) % 3]] - x[ids[(a + 2) % 3]]
            with np.errstate(all="ignore"):
                out[ids[a]] += _cross(e, a_t)
                lim[ids[a]] += np.sqrt((e * e).sum()) * A_t
    return out, lim, ok


def normals_vjp_exact(verts, faces, g):
    """(dL/dverts [V, 3] long double, the contract's absolute term per vertex but for its factor, the vertices with a normal)"""
    return _normals_vjp(verts, faces, g, LD)


def normals_vjp_f64(verts, faces, g):
    """the arithmetic of k_vn_h and k_vn_vjp in f64, the store rounded to f32"""
    return _normals_vjp(verts, faces, g, np.float64)[0].astype(np.float32)


def check_normals_vjp(verts, faces, g, grad_verts):
    """Asserts the adjoint's contract on every vertex and component of one frame.  Returns the worst error in units of its bound."""
    exact, lim, _ = normals_vjp_exact(verts, faces, g)
    got = np.asarray(grad_verts)
    assert got.dtype == np.float32 and got.shape == exact.shape
    bound = U * np.abs(exact) + (K_V * EPS * lim)[:, None] + TINY
    return _worst(np.abs(got.astype(LD) - exact), bound, np.ones(exact.shape, bool), "normals vjp")


def normals_f64(verts, faces):
    """the unit vertex normals in f64 (0 where the forward writes 0), for finite differences"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    s, _, has = _normal_sums(np.asarray(verts, np.float64), faces, np.float64)
    with np.errstate(all="ignore"):
        l = np.sqrt((s * s).sum(axis=-1))
        ok = has & np.isfinite(l) & (l > 0)
        return np.where(ok[:, None], s / np.where(ok, l, 1)[:, None], 0)


def hand_mesh():
    """(verts [8, 3] f32, faces): a tiny mesh with a repeated-corner face, an isolated vertex (5), a vertex between two opposite
    faces (4: its sum is exactly zero) and a NaN vertex (6)"""
    verts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2.5], [1, 1, 2.25], [0.5, -1, 2], [3, 3, 3], [np.nan, 0.5, 2], [2, 1, 2]],
                     np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2], [0, 0, 1], [4, 0, 1], [4, 1, 0], [3, 7, 6]], np.int32)
    return verts, faces


def flat_scene():
    """(verts, faces, normals, intr, size): one frontal triangle at z = 2 whose corners 0 and 1 carry OPPOSITE normals and corner 2
    a zero one (on the median lambda_0 = lambda_1 the three cancel exactly: l = 0), and a second triangle with all-zero normals"""
    intr, size = (60.0, 60.0, 16.0, 12.0), (24, 32)
    verts = np.array([[-0.4, -0.3, 2], [0.4, -0.3, 2], [0, 0.3, 2], [-0.5, 0.1, 3], [0.5, 0.1, 3], [0, 0.4, 3]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    normals = np.array([[0.6, 0, -0.8], [-0.6, 0, 0.8], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    return verts, faces, normals, intr, size


# ---- the fit of the light ----------------------------------------------------------------------------------------------------------
FIT_STEPS = 40
FIT_LIGHT = np.array([[0.7, 0.7, 0.65], [0.45, 0.4, 0.35], [-0.3, -0.3, -0.25], [-0.5, -0.45, -0.4], [0, 0, 0], [0, 0, 0], [0, 0, 0],
                      [0, 0, 0], [0.05, 0.05, 0.05]], np.float32)          # ambient, a strong directional part, a little z^2
FIT_START = np.array([[0.7, 0.7, 0.65]] + [[0, 0, 0]] * 8, np.float32)    # ambient only


def fit_scene():
    """(verts [3, V, 3] f32, faces, intr, size, colours [V, 3] f32): raster_ref's two_spheres in three poses (the body turns a little
    about the vertical axis between them), with smooth vertex colours"""
    import raster_ref as rr
    v, faces, intr, size = rr.two_spheres()
    c0 = np.array([0.02, -0.01, 3.0])
    poses = []
    for ang, shift in ((0.0, (0, 0, 0)), (0.35, (0.01, -0.02, 0.05)), (-0.3, (-0.02, 0.01, -0.04))):
        ca, sa = np.cos(ang), np.sin(ang)
        R = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
        poses.append(((v.astype(np.float64) - c0) @ R.T + c0 + np.asarray(shift)).astype(np.float32))
    x = v.astype(np.float64)
    colours = 0.55 + 0.35 * np.stack((np.sin(7 * x[:, 0]), np.cos(5 * x[:, 1]), np.sin(3 * x[:, 2] + x[:, 0])), axis=1)
    return np.stack(poses), faces, intr, size, colours.astype(np.float32)


def fit_rate(A, b, lit):
    """the step of the plain gradient descent: 1 / trace of the cost's Hessian in the light, 2 sum over the lit pixels of
    max_c A_c^2 |b|^2, from the f32 albedo images A [F, H, W, C] and the bases b [F, H, W, 9]"""
    a2 = (A.astype(np.float64) ** 2).max(axis=-1)
    return float(1.0 / (2.0 * (np.where(lit, a2 * (b.astype(np.float64) ** 2).sum(axis=-1), 0.0)).sum()))


def fit_restated(A, b, lit, target, rate, steps=FIT_STEPS, store32=True, start=FIT_START):
    """`steps` plain gradient steps in the light on sum |A s(light) - target|^2 over all pixels (an unlit pixel holds A): the final
    light and the costs before every step and after the last.  store32: the image, the upstream gradient, the light's gradient
    and the light are rounded to f32 where the layer stores them; otherwise everything f64."""
    A64, b64, T = A.astype(np.float64), b.astype(np.float64), target.astype(np.float64)
    r = (lambda x: x.astype(np.float32).astype(np.float64)) if store32 else (lambda x: x)
    L = start.astype(np.float64)
    costs = []

    def image_of(L):
        return np.where(lit[..., None], r(A64 * (b64 @ L)), A64)

    for _ in range(steps):
        d = image_of(L) - T
        costs.append(float((d * d).sum()))
        G = r(2.0 * d)
        g = np.zeros((9, A.shape[-1]))
        for f in range(A.shape[0]):         # per frame (rounded once each), then the frames in f64: a shared light
            g += r(np.einsum("hwc,hwk->kc", np.where(lit[f][..., None], G[f] * A64[f], 0.0), b64[f]))
        L = r(L - rate * r(g))
    d = image_of(L) - T
    costs.append(float((d * d).sum()))
    return L, costs
