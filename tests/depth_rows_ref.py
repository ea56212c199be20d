"""Test infrastructure (numpy): the reference statement of the depth rows (bodyfit_raster_depth_rows_device) and of the rows VJP
(bodyfit_surface_rows_vjp_device), of their contracts in include/bodyfit.h, and the scenes the CPU and the GPU tests share.

The definitions are evaluated in extended precision (np.longdouble, as raster_ref does: 2^-11 of the f64 the kernel works in),
from the f32 vertices and the f64 intrinsics.  Rows works on ONE frame: (verts [V, 3] f32, faces [nf, 3] int, intr = (fx, fy,
cx, cy), size = (H, W), a face-id image [H, W] int and optionally a list of linear pixel indices)."""
import numpy as np

import raster_ref as rr

LD = np.longdouble
U = 2.0 ** -24
K = 2                     # the constants of include/bodyfit.h (bodyfit_raster_depth_rows_device) ...
KAPPA_SHIFT = 2.0 ** -21  # ... kappa = 2^-21 rho Q / c
KAPPA_B_SHIFT = 2.0 ** -18  # ... kappa_b = 2^-18 rho Q^2 / c
KAPPA_VOID = 2.0 ** 24    # ... a row voided although n, D != 0 has kappa above this
K_VJP = 2                 # ... |g - G*| <= 2 u T (bodyfit_surface_rows_vjp_device)


def header_constants(text):
    """(k, the shift of kappa, the shift of kappa_b, k of the VJP) as include/bodyfit.h states them"""
    import re
    s = text[text.index("DEPTH ROWS"):]
    k = re.search(r"u = 2\^-24, k = (\d+) and per non-void row", s)
    a = re.search(r"kappa = 2\^-(\d+) rho Q / c", s)
    b = re.search(r"kappa_b = 2\^-(\d+) rho Q\^2 / c", s)
    v = re.search(r"\|d_gverts - G\*\| <= (\d+) u T", text)
    return int(k.group(1)), int(a.group(1)), int(b.group(1)), int(v.group(1))


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _gather(verts, faces, size, face_img, pixel):
    """(pix [N] int64, t [N] int64 the face or -1, corners [N, 3, 3] f32 (a unit triangle where there is none), live [N])"""
    H, W = size
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    img = np.asarray(face_img, np.int64).reshape(-1)
    assert img.shape[0] == H * W
    pix = np.arange(H * W, dtype=np.int64) if pixel is None else np.asarray(pixel, np.int64).reshape(-1)
    inside = (pix >= 0) & (pix < H * W)
    t = np.where(inside, img[np.clip(pix, 0, H * W - 1)], -1)
    t = np.where((t >= 0) & (t < len(faces)), t, -1)
    unit = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)
    corners = np.asarray(verts, np.float32)[faces[np.clip(t, 0, None)]] if len(faces) else np.tile(unit, (len(pix), 1, 1))
    live = (t >= 0) & np.isfinite(corners).all(axis=(1, 2))
    corners = np.where(live[:, None, None], corners, unit)
    return pix, t, corners, live


class Rows:
    """the exact rows of one frame, and what the contract allows around them"""

    def __init__(self, verts, faces, intr, size, face_img, pixel=None):
        assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an extended-precision long double"
        H, W = size
        fx, fy, cx, cy = (LD(float(a)) for a in intr)
        pix, t, corners, live = _gather(verts, faces, size, face_img, pixel)
        v = corners.astype(LD)
        n = _cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        i, j = pix // W, pix - (pix // W) * W
        d = np.stack(((j.astype(LD) - cx) / fx, (i.astype(LD) - cy) / fy, np.ones(len(pix), LD)), axis=-1)
        D, nn = _dot(n, d), _dot(n, n)
        self.n_zero = live & (nn == 0)
        self.d_zero = live & (nn != 0) & (D == 0)
        self.void = ~live | self.n_zero | self.d_zero
        ok = ~self.void
        Ds, nns = np.where(ok, D, 1), np.where(ok, nn, 1)
        z = _dot(n, v[:, 0]) / Ds
        x = z[:, None] * d
        beta = np.stack([_dot(n, _cross(v[:, (a + 1) % 3] - x, v[:, (a + 2) % 3] - x)) / nns for a in range(3)], axis=-1)
        m = n / Ds[:, None]
        P = np.maximum(np.abs(v).max(axis=(1, 2)), np.abs(x).max(axis=1))
        L = np.abs(v - x[:, None, :]).max(axis=(1, 2))
        for a in range(3):
            L = np.maximum(L, np.abs(v[:, a] - v[:, (a + 1) % 3]).max(axis=1))
        absn, absx, absd = np.sqrt(nns), np.sqrt(_dot(x, x)), np.sqrt(_dot(d, d))
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            Q = (P * L / absn).astype(np.float64)
            rho = np.maximum(1.0, (P / np.where(absx > 0, absx, 1)).astype(np.float64))
            rho = np.where(absx > 0, rho, np.inf)
            c = (np.abs(Ds) / (absn * absd)).astype(np.float64)
            self.kappa = np.where(ok, KAPPA_SHIFT * rho * Q / c, np.inf)
            self.kappa_b = np.where(ok, KAPPA_B_SHIFT * rho * Q * Q / c, np.inf)
        self.pix, self.face, self.live, self.d = pix, np.where(self.void, -1, t), live, d.astype(np.float64)
        self.t_image = t
        self.z = np.where(ok, z, np.inf)                                   # extended precision
        self.beta = np.where(ok[:, None], beta, 0)
        self.m = np.where(ok[:, None], m, 0)
        self.abs_m = np.sqrt(_dot(self.m, self.m))
        self.cos = np.where(ok, c, 0.0)
        self.Q, self.rho = Q, rho
        # the bounds of the contract, f64
        with np.errstate(over="ignore", invalid="ignore"):
            self.z_tol = np.where(ok, (K + self.kappa) * U * np.abs(self.z).astype(np.float64), np.inf)
            self.m_tol = np.where(ok, (K + self.kappa) * U * self.abs_m.astype(np.float64), np.inf)
            self.b_tol = np.where(ok, (K + self.kappa_b) * U * np.maximum(1.0, np.abs(self.beta).max(axis=1).astype(np.float64)), np.inf)


def check_rows(rows, index, z=None, bary=None, direction=None):
    """Asserts the rows contract for EVERY row of one frame's outputs (index int32 [N]; z f32 [N], bary f32 [N, 3], direction f32
    [N, 3] or None).  Returns the worst (z, bary, direction) errors in units of their bounds."""
    index = np.asarray(index)
    N = len(rows.pix)
    assert index.dtype == np.int32 and index.shape == (N,)
    out_void = index < 0
    assert np.all(index[out_void] == -1)
    # void by definition (empty, outside, non-finite, an exact n = 0): void in the output.  An exact D = 0 may come out either way.
    must_void = rows.void & ~rows.d_zero
    assert np.all(out_void[must_void]), ("a void row came back with a face", np.nonzero(must_void & ~out_void)[0][:8])
    # a row the definition keeps is voided only where the f64 evaluation cannot tell n or D from 0
    lost = out_void & ~rows.void
    assert np.all(rows.kappa[lost] >= KAPPA_VOID), ("a row was voided", np.nonzero(lost)[0][:8], rows.kappa[lost][:8])
    both = ~out_void & ~rows.void
    assert np.all(index[both] == rows.face[both]), "a row holds another face than the image"
    worst = [0.0, 0.0, 0.0]
    with np.errstate(invalid="ignore", over="ignore"):
        if z is not None:
            z = np.asarray(z)
            assert z.dtype == np.float32 and z.shape == (N,)
            assert np.all(np.isposinf(z[out_void])), "a void row holds z = +inf"
            err = np.abs(z[both].astype(LD) - rows.z[both]).astype(np.float64)
            assert np.all(err <= rows.z_tol[both]), ("z", float((err / rows.z_tol[both]).max()))
            worst[0] = float((err / rows.z_tol[both]).max()) if both.any() else 0.0
        if bary is not None:
            bary = np.asarray(bary)
            assert bary.dtype == np.float32 and bary.shape == (N, 3)
            assert np.all(bary[out_void] == 0), "a void row holds zero weights"
            err = np.abs(bary[both].astype(LD) - rows.beta[both]).max(axis=1).astype(np.float64)
            assert np.all(err <= rows.b_tol[both]), ("beta", float((err / rows.b_tol[both]).max()))
            worst[1] = float((err / rows.b_tol[both]).max()) if both.any() else 0.0
        if direction is not None:
            direction = np.asarray(direction)
            assert direction.dtype == np.float32 and direction.shape == (N, 3)
            assert np.all(direction[out_void] == 0), "a void row holds a zero direction"
            err = np.abs(direction[both].astype(LD) - rows.m[both]).max(axis=1).astype(np.float64)
            assert np.all(err <= rows.m_tol[both]), ("m", float((err / rows.m_tol[both]).max()))
            worst[2] = float((err / rows.m_tol[both]).max()) if both.any() else 0.0
    return tuple(worst)


def kernel_form_f64(verts, faces, intr, size, face_img, pixel=None):
    """(index int32 [N], z f32 [N], bary f32 [N, 3], direction f32 [N, 3]) by the arithmetic of k_rs_depth_rows, operation for
    operation in f64 (numpy never fuses): shows on the CPU that the contract is attainable."""
    H, W = size
    fx, fy, cx, cy = (np.float64(a) for a in intr)
    pix, t, corners, live = _gather(verts, faces, size, face_img, pixel)
    v = corners.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = _cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        i, j = pix // W, pix - (pix // W) * W
        dx, dy = (j.astype(np.float64) - cx) / fx, (i.astype(np.float64) - cy) / fy
        D = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2]
        nn = _dot(n, n)
        ok = live & (nn > 0) & (D != 0)
        z = _dot(n, v[:, 0]) / D
        x = np.stack((z * dx, z * dy, z), axis=-1)
        inv = 1.0 / nn
        beta = np.stack([_dot(n, _cross(v[:, (a + 1) % 3] - x, v[:, (a + 2) % 3] - x)) * inv for a in range(3)], axis=-1)
        m = n / D[:, None]
        return (np.where(ok, t, -1).astype(np.int32), np.where(ok, z, np.inf).astype(np.float32),
                np.where(ok[:, None], beta, 0).astype(np.float32), np.where(ok[:, None], m, 0).astype(np.float32))


def exact_depth_at(verts, faces, intr, size, t, pix):
    """the exact ray-plane depth (longdouble) of face t at linear pixel pix for the vertices verts (any float dtype, used as given)"""
    H, W = size
    fx, fy, cx, cy = (LD(float(a)) for a in intr)
    v = np.asarray(verts).astype(LD)[np.asarray(faces, np.int64).reshape(-1, 3)[t]]
    n = _cross(v[1] - v[0], v[2] - v[0])
    i, j = pix // W, pix % W
    d = np.array([(LD(j) - cx) / fx, (LD(i) - cy) / fy, LD(1)])
    return _dot(n, v[0]) / _dot(n, d)


# ---- the rows VJP ------------------------------------------------------------------------------------------------------------
def vjp_exact(faces, n_verts, index, bary, coef, direction):
    """(G* [V, 3], T [V, 3]) in extended precision from the f32 rows of one frame: the sum of coef_i bary_ia dir_i at
    faces[index_i][a] and the same sum of absolute values; rows with index outside [0, n_faces) contribute nothing"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    index = np.asarray(index, np.int64)
    keep = (index >= 0) & (index < len(faces))
    G, T = np.zeros((n_verts, 3), LD), np.zeros((n_verts, 3), LD)
    if keep.any():
        b = np.asarray(bary, np.float32)[keep].astype(LD)
        g = np.asarray(coef, np.float32)[keep].astype(LD)
        m = np.asarray(direction, np.float32)[keep].astype(LD)
        terms = g[:, None, None] * b[:, :, None] * m[:, None, :]               # [n, corner, xyz]
        ids = faces[index[keep]]
        for a in range(3):
            np.add.at(G, ids[:, a], terms[:, a])
            np.add.at(T, ids[:, a], np.abs(terms[:, a]))
    return G, T


def check_vjp(faces, n_verts, index, bary, coef, direction, gverts):
    """Asserts |gverts - G*| <= 2 u T for EVERY vertex component of one frame (gverts f32 [V, 3]); an untouched vertex holds an
    exact 0.  Returns the worst error in units of the bound."""
    gverts = np.asarray(gverts)
    assert gverts.dtype == np.float32 and gverts.shape == (n_verts, 3)
    G, T = vjp_exact(faces, n_verts, index, bary, coef, direction)
    assert np.all(np.isfinite(gverts)), "a non-finite gradient"
    err = np.abs(gverts.astype(LD) - G)
    lim = K_VJP * U * T
    assert np.all(gverts[T == 0] == 0), "a vertex nothing lands on holds 0"
    assert np.all(err <= lim), ("rows VJP", int((err > lim).sum()), float((err[T > 0] / lim[T > 0]).max()))
    return float((err[T > 0] / lim[T > 0]).max()) if (T > 0).any() else 0.0


def composed_gradient(rows, faces, n_verts, coef):
    """The two contracts composed, for one frame: (G, bound, T) [V, 3] f64 with G the gradient of sum_i coef_i z_i by the exact
    rows, T the same sum of absolute values, and bound what the f32 rows (each beta within b_tol, each m_c within m_tol) followed
    by the rows VJP (2 u T of the perturbed rows) may differ from G by.  coef f32 [N]; void rows contribute nothing."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = ~rows.void
    g = np.asarray(coef, np.float32).astype(np.float64)[keep].astype(LD)
    b, m = rows.beta[keep], rows.m[keep]
    db, dm = rows.b_tol[keep].astype(LD)[:, None], rows.m_tol[keep].astype(LD)[:, None]
    ids = faces[rows.face[keep]]
    G, B, T = np.zeros((n_verts, 3), LD), np.zeros((n_verts, 3), LD), np.zeros((n_verts, 3), LD)
    for a in range(3):
        ba = b[:, a:a + 1]
        np.add.at(G, ids[:, a], g[:, None] * ba * m)
        np.add.at(T, ids[:, a], np.abs(g[:, None] * ba * m))
        first = np.abs(ba) * dm + np.abs(m) * db + db * dm
        vjp = K_VJP * U * (np.abs(ba) + db) * (np.abs(m) + dm)
        np.add.at(B, ids[:, a], np.abs(g)[:, None] * (first + vjp))
    return G.astype(np.float64), B.astype(np.float64), T.astype(np.float64)


def residual_gradient_bound(rows, faces, n_verts, r, used):
    """[V, 3] f64: what the gradient of sum over the `used` rows of r_i^2, formed from the f32 rows with coef_i = f32(2 r_i), r_i =
    z^_i - sensor_i [N] f64, may differ by from the exact gradient at the same rows: composed_gradient's bound, and the
    coefficient's own error 2 z_tol + u |coef| (r moves with z^; the conversion to f32) through |beta| |m|"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    used = np.asarray(used, bool) & ~rows.void
    coef = np.where(used, (2 * np.asarray(r, np.float64)).astype(np.float32), np.float32(0))
    _, bound, _ = composed_gradient(rows, faces, n_verts, coef)
    dcoef = np.where(used, 2 * rows.z_tol + U * np.abs(coef.astype(np.float64)), 0.0)[used]
    b = np.abs(rows.beta[used]).astype(np.float64) + rows.b_tol[used][:, None]
    m = np.abs(rows.m[used]).astype(np.float64) + rows.m_tol[used][:, None]
    ids = faces[rows.face[used]]
    for a in range(3):
        np.add.at(bound, ids[:, a], dcoef[:, None] * b[:, a:a + 1] * m)
    return bound


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def grazing_scene():
    """one face seen about 2 degrees from edge-on (its plane passes 0.1 m from the camera), 1.5 m to 3.4 m deep, over a frontal
    backdrop"""
    intr, size = (300.0, 300.0, 32.0, 24.0), (48, 64)
    un = lambda u, v, z: [(u - intr[2]) / intr[0] * z, (v - intr[3]) / intr[1] * z, z]
    A, B = np.array(un(4, 4, 1.5)), np.array(un(9, 44, 1.6))
    up = np.cross(A, B)
    C = 1.1 * (A + B) - 0.15 * np.sign(up[0]) * up / np.linalg.norm(up)     # in span(A, B) the face would be exactly edge-on
    verts = np.array([A, B, C, un(-64, -48, 5.0), un(192, -48, 5.0), un(0, 144, 5.0)], np.float32)
    return verts, np.array([[0, 1, 2], [3, 5, 4]], np.int32), intr, size, 0.1, False


def sliver_scene():
    """a sliver 40 pixels long and a third of a pixel wide (|n| / L^2 about 1 / 250), 2.5 m away, over a frontal backdrop, and a
    second one 2^-12 of a pixel wide that owns no pixel centre but is addressed by hand-made face images"""
    intr, size = (300.0, 300.0, 32.0, 24.0), (48, 64)
    un = lambda u, v, z: [(u - intr[2]) / intr[0] * z, (v - intr[3]) / intr[1] * z, z]
    verts = np.array([un(10, 20, 2.5), un(50, 20.2, 2.6), un(50, 19.87, 2.6), un(-64, -48, 5.0), un(192, -48, 5.0), un(0, 144, 5.0),
                      un(10, 30, 2.5), un(50, 30.0, 2.6), un(50, 30.0 + 2.0 ** -12, 2.6)], np.float32)
    return verts, np.array([[0, 1, 2], [3, 5, 4], [6, 7, 8]], np.int32), intr, size, 0.1, False


def row_scenes(synth):
    """name -> (verts, faces, intr, size, z_near, cull): raster_ref's contract scenes, a grazing face and a sliver"""
    S = dict(rr.contract_scenes(synth))
    S["grazing"] = grazing_scene()
    S["sliver"] = sliver_scene()
    return S


def round_robin_image(n_faces, size):
    """a hand-made face-id image that addresses every face from many pixels, whether or not the face covers them (-1 and an
    id past the topology among them): rows whose pixel is far from the face, whose face is degenerate or behind z_near"""
    H, W = size
    img = (np.arange(H * W, dtype=np.int64) * 7) % (n_faces + 2) - 1
    return img.reshape(H, W).astype(np.int32)


# ---- the scene of the DepthResidualTerm test -----------------------------------------------------------------------------------
# (both thresholds sit in gaps of the scene's own |r| and cosine values, 1e-4 m and 0.02 wide, against a rows contract of 4e-7 m:
#  test_depth_rows.py asserts the margins)
TERM_TRUNC = 0.0118
TERM_MIN_COS = 0.38


def term_scene():
    """(verts [3, V, 3] f32, faces, intr, size, sensor [3, H, W] f32): two_spheres in three poses; the sensor maps are the
    kernel-form render of the poses moved by a few millimetres, with pixels knocked out (0, NaN, -1), and frame 2 holds none"""
    v, faces, intr, size = rr.two_spheres()
    verts = np.stack([v, v + np.float32([0.01, -0.02, 0.05]), v + np.float32([-0.02, 0.01, -0.04])]).astype(np.float32)
    moved = verts + np.float32([0.004, -0.003, 0.009])
    sensor = np.stack([rr.kernel_form_f64(m, faces, intr, size)[0] for m in moved[:2]] + [np.zeros(size, np.float32)])
    flat = sensor.reshape(3, -1)
    flat[:, ::5] = 0.0
    flat[:, 3::11] = np.nan
    flat[:, 7::13] = -1.0
    return verts, faces, intr, size, sensor


def decision_margins(rows, sensor_row, trunc, min_cos):
    """(margin of |r| to trunc, margin of the cosine to min_cos) over the non-void rows of one frame, each reduced by what the
    rows contract lets the f32 rows differ from the exact ones: positive means no f32 row can decide otherwise than the exact
    one.  sensor_row f32 [N]: the sensor depth of every row."""
    keep = ~rows.void
    r = np.abs(rows.z[keep] - np.asarray(sensor_row, np.float32)[keep].astype(LD)).astype(np.float64)
    m_trunc = np.abs(r - trunc) - rows.z_tol[keep]
    absd = np.sqrt((rows.d[keep] ** 2).sum(axis=1))
    cos = 1.0 / (rows.abs_m[keep].astype(np.float64) * absd)
    m_cos = np.abs(cos - min_cos) - 2.0 * cos * rows.m_tol[keep] / rows.abs_m[keep].astype(np.float64)
    return (float(m_trunc.min()) if keep.any() else np.inf), (float(m_cos.min()) if keep.any() else np.inf)
