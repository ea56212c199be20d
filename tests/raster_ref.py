"""Test infrastructure (numpy): the reference statement of the depth render's DEFINITION (bodyfit_raster_render_device,
include/bodyfit.h) and of its contract, the visibility that follows from it, and the scenes the CPU and the GPU tests share.

The definition is evaluated in extended precision (np.longdouble: 64 significant bits on x86-64) from the f32 vertices and the
f64 intrinsics, 2^-11 of the f64 the kernel decides in, so the reference's own error is nothing beside the bands it draws.
Per pixel it gives the exact minimiser (ties to the lowest face id), the set of answers the contract admits, and a flag
"unambiguous": exactly one admissible face and no face inside a band (|min lambda| < tau, or an area the kernel's f64 may see
as zero or of the other sign).  check_contract asserts (a) .. (e) for EVERY pixel of a frame.

A frame is (verts [V, 3] f32, faces [nf, 3] int); an image size is (H, W); intr is (fx, fy, cx, cy)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -24       # unit roundoff of f32
K_E = 2              # the derived constants of include/bodyfit.h (bodyfit_raster_render_device) ...
K_Z = 2
Q_SHIFT = 2.0 ** -22     # ... tau_t = K_E U (1 + 2^-22 Q_t)
C_SHIFT = 2.0 ** -19     # ... c_t = 2^-19 Q_t R_t
AREA_TOL = 2.0 ** -46    # ... a cull decision is sure beyond 2^-46 P_t^2


def header_constants(text):
    """(k_e, k_z, the shifts of Q in tau and c, the shift of the area tolerance) as include/bodyfit.h states them"""
    import re
    s = text[text.index("depth render and visibility"):]
    k = re.search(r"k_e = (\d+), k_z = (\d+)", s)
    t = re.search(r"tau_t = k_e u \(1 \+ 2\^-(\d+) Q_t\)", s)
    c = re.search(r"c_t = 2\^-(\d+) Q_t R_t", s)
    a = re.search(r"A <= 2\^-(\d+) P_t\^2", s)
    return int(k.group(1)), int(k.group(2)), int(t.group(1)), int(c.group(1)), int(a.group(1))


class Faces:
    """per-face quantities of one frame, exact to extended precision"""

    def __init__(self, verts, faces, intr, size, z_near=0.1, cull=False):
        assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an extended-precision long double"
        H, W = size
        fx, fy, cx, cy = (LD(float(a)) for a in intr)
        v = np.asarray(verts, np.float32)[np.asarray(faces, np.int64).reshape(-1, 3)]          # [nf, 3, 3] f32
        self.n = v.shape[0]
        self.valid3d = np.isfinite(v).all(axis=(1, 2)) & (v[:, :, 2] >= np.float32(z_near)).all(axis=1)
        vv = np.where(self.valid3d[:, None, None], v, np.float32(1)).astype(LD)
        self.Z = vv[:, :, 2]
        self.u = fx * vv[:, :, 0] / self.Z + cx
        self.v = fy * vv[:, :, 1] / self.Z + cy
        u, w = self.u, self.v
        self.A = (u[:, 1] - u[:, 0]) * (w[:, 2] - w[:, 0]) - (u[:, 2] - u[:, 0]) * (w[:, 1] - w[:, 0])
        P = np.maximum(np.abs(u), np.abs(w)).max(axis=1) + LD(max(W, H)) + max(abs(cx), abs(cy))
        absA = np.abs(self.A)
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            Q = np.where(absA > 0, P * P / np.where(absA > 0, absA, 1), np.inf).astype(np.float64)
            R = (self.Z.max(axis=1) / self.Z.min(axis=1)).astype(np.float64)
            self.tau = K_E * U * (1.0 + Q_SHIFT * Q)
            self.c = np.where(np.isfinite(Q), C_SHIFT * Q * R, np.inf)
        tol = (AREA_TOL * P * P)
        self.drawn = self.valid3d & (self.A != 0) & ((self.A < 0) if cull else True)             # the definition
        self.sure = self.valid3d & (absA > tol) & ((self.A < -tol) if cull else True)            # ... whatever the f64 rounding
        self.loose = self.valid3d & (self.A != 0) & ((self.A <= tol) if cull else True)
        self.Q, self.R, self.P = Q, R, P.astype(np.float64)
        self.size = (H, W)

    def region(self, t):
        """the pixel rectangle (y0, y1, x0, x1), half open, outside which face t is surely missing"""
        H, W = self.size
        u, v = self.u[t].astype(np.float64), self.v[t].astype(np.float64)
        diag = float(np.hypot(u.max() - u.min(), v.max() - v.min()))
        m = self.tau[t] * diag
        m = 2.0 + (m if np.isfinite(m) and m < 1e6 else 1e6)
        x0, x1 = int(max(np.floor(u.min() - m), 0)), int(min(np.ceil(u.max() + m), W - 1))
        y0, y1 = int(max(np.floor(v.min() - m), 0)), int(min(np.ceil(v.max() + m), H - 1))
        return y0, y1 + 1, x0, x1 + 1

    def evaluate(self, t, ys, xs):
        """(lambda [.., 3], min lambda, z at the clamped lambda), f64, of face t (scalar or array) at the samples (xs, ys)"""
        su, sv = np.asarray(xs).astype(LD), np.asarray(ys).astype(LD)
        u, v, A, Z = self.u[t], self.v[t], self.A[t], self.Z[t]
        lam = []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            lam.append(((u[..., b] - su) * (v[..., c] - sv) - (u[..., c] - su) * (v[..., b] - sv)) / A)
        lam = np.stack(lam, axis=-1)
        pos = np.maximum(lam, 0)
        s = pos.sum(axis=-1, keepdims=True)
        pos = pos / np.where(s > 0, s, 1)
        w = (pos / Z).sum(axis=-1)
        z = 1 / np.where(w > 0, w, 1)
        return lam.astype(np.float64), lam.min(axis=-1).astype(np.float64), np.where(w > 0, z, np.inf).astype(np.float64)


class Reference:
    """what the definition and the contract say about every pixel of one frame"""

    def __init__(self, verts, faces, intr, size, z_near=0.1, cull=False):
        H, W = size
        self.verts, self.faces_arr, self.size = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3), (H, W)
        self.F = F = Faces(verts, faces, intr, size, z_near, cull)
        self.depth = np.full((H, W), np.inf)          # the exact answer
        self.face = np.full((H, W), -1, np.int64)
        self.zcap = np.full((H, W), np.inf)           # (c): min over the surely covering faces of (1 + (k_z + c_t) u) z
        self.band = np.zeros((H, W), bool)
        kept = []
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for t in np.nonzero(F.loose)[0]:
                y0, y1, x0, x1 = F.region(t)
                if y0 >= y1 or x0 >= x1:
                    continue
                ys, xs = np.mgrid[y0:y1, x0:x1]
                _, lmin, z = F.evaluate(t, ys, xs)
                sl = (slice(y0, y1), slice(x0, x1))
                tau = F.tau[t]
                near = lmin >= -tau
                if not near.any():
                    continue
                kept.append((t, sl, near, z))
                if F.drawn[t]:
                    win = (lmin >= 0) & (z < self.depth[sl])          # ascending t: the lowest id keeps a tie
                    self.depth[sl] = np.where(win, z, self.depth[sl])
                    self.face[sl] = np.where(win, t, self.face[sl])
                if F.sure[t]:
                    surely = lmin >= tau
                    self.zcap[sl] = np.minimum(self.zcap[sl], np.where(surely, z * (1 + (K_Z + F.c[t]) * U), np.inf))
                    self.band[sl] |= near & ~surely
                else:
                    self.band[sl] |= near
            self.n_admissible = np.zeros((H, W), np.int64)
            self.admissible_face = np.full((H, W), -1, np.int64)
            self.may = np.zeros(F.n, bool)
            for t, sl, near, z in kept:
                adm = near & (z / (1 + (K_Z + F.c[t]) * U) <= self.zcap[sl])
                self.n_admissible[sl] += adm
                self.admissible_face[sl] = np.where(adm, t, self.admissible_face[sl])
                self.may[t] = adm.any()
        self.covered = self.face >= 0
        self.unambiguous = (self.n_admissible == 1) & ~self.band
        self.must = np.zeros(F.n, bool)
        self.must[self.admissible_face[self.unambiguous]] = True
        self.must_vertices = np.zeros(len(self.verts), bool)
        self.must_vertices[self.faces_arr[self.must].reshape(-1)] = True
        self.may_vertices = np.zeros(len(self.verts), bool)
        self.may_vertices[self.faces_arr[self.may].reshape(-1)] = True

    def ambiguous_share(self):
        """the share of the covered pixels that are not unambiguous"""
        n = int(self.covered.sum())
        return float((self.covered & ~self.unambiguous).sum()) / max(n, 1)

    def exact_bary(self):
        """[H, W, 3] f64: the lambda of the exact answer (0 where empty)"""
        out = np.zeros(self.size + (3,))
        ys, xs = np.nonzero(self.covered)
        if len(ys):
            out[ys, xs] = self.F.evaluate(self.face[ys, xs], ys, xs)[0]
        return out


def check_contract(ref, depth, face, bary=None):
    """Asserts (a) .. (e) of include/bodyfit.h for EVERY pixel of one frame's outputs (depth f32 [H, W], face int32 [H, W], bary
    f32 [H, W, 3] or None), and that every unambiguous pixel holds the reference's face.  Returns the worst figures: (min lambda
    of a returned face in units of its tau, depth error in units of (k_z + c) u z^, weight error in units of tau)."""
    F = ref.F
    H, W = ref.size
    depth, face = np.asarray(depth), np.asarray(face).astype(np.int64)
    assert depth.dtype == np.float32 and depth.shape == (H, W) and face.shape == (H, W)
    empty = face < 0
    assert np.all(face[empty] == -1) and np.all(np.isposinf(depth[empty])), "an empty pixel holds -1 and +inf"
    assert not (empty & np.isfinite(ref.zcap)).any(), ("(d) empty where a face surely covers", int((empty & np.isfinite(ref.zcap)).sum()))
    if bary is not None:
        bary = np.asarray(bary)
        assert bary.dtype == np.float32 and bary.shape == (H, W, 3)
        assert np.all(bary[empty] == 0), "an empty pixel holds zero weights"
    worst = [0.0, 0.0, 0.0]
    ys, xs = np.nonzero(~empty)
    if len(ys):
        t = face[ys, xs]
        assert np.all(t < F.n), "face id out of range"
        assert np.all(F.loose[t]), ("(a) a face that is not drawn was returned", np.unique(t[~F.loose[t]])[:8])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            lam, lmin, z = F.evaluate(t, ys, xs)
            tau, c = F.tau[t], F.c[t]
            zh = depth[ys, xs].astype(np.float64)
            bad = lmin < -tau
            assert not bad.any(), ("(a) surely missing", int(bad.sum()), list(zip(ys[bad][:4], xs[bad][:4], t[bad][:4])))
            assert np.all(np.isfinite(zh) & (zh > 0)), "a covered pixel holds a finite positive depth"
            lim = np.where(np.isfinite(c), (K_Z + c) * U * zh, np.inf)
            bad = np.abs(zh - z) > lim
            assert not bad.any(), ("(b) depth", int(bad.sum()), float((np.abs(zh - z) / lim).max()))
            bad = zh > ref.zcap[ys, xs]
            assert not bad.any(), ("(c) a surely covering face is nearer", int(bad.sum()), list(zip(ys[bad][:4], xs[bad][:4])))
            worst[0] = float((-lmin / tau).max())
            worst[1] = float((np.abs(zh - z) / lim).max())
            if bary is not None:
                b = bary[ys, xs].astype(np.float64)
                assert np.all(b >= 0), "(e) negative weight"
                bad = np.abs(b.sum(axis=1) - 1) > 2 * tau
                assert not bad.any(), ("(e) the weights' sum", int(bad.sum()))
                err = np.abs(b - lam).max(axis=1)
                bad = err > tau
                assert not bad.any(), ("(e) weights against the exact lambda", int(bad.sum()), float((err / tau).max()))
                worst[2] = float((err / tau).max())
    una = ref.unambiguous
    wrong = una & (face != ref.admissible_face)
    assert not wrong.any(), ("face identity on unambiguous pixels", int(wrong.sum()), list(zip(*np.nonzero(wrong)))[:4])
    assert np.array_equal(ref.admissible_face[una], ref.face[una])
    return tuple(worst)


def kernel_form_f64(verts, faces, intr, size, z_near=0.1, cull=False):
    """(depth f32 [H, W], face int32, bary f32 [H, W, 3]) by the arithmetic of k_raster.hip, operation for operation in f64
    (numpy never fuses), every (face, pixel) pair of a face's bounding box: shows on the CPU that the contract is attainable."""
    H, W = size
    fx, fy, cx, cy = (np.float64(a) for a in intr)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    best_w = np.zeros((H, W)); best_f = np.full((H, W), -1, np.int64); best_l = np.zeros((H, W, 3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t, ids in enumerate(faces):
            c = np.asarray(verts, np.float32)[ids]
            if not (np.isfinite(c).all() and (c[:, 2] >= np.float32(z_near)).all()):
                continue
            c = c.astype(np.float64)
            u = fx * (c[:, 0] / c[:, 2]) + cx
            v = fy * (c[:, 1] / c[:, 2]) + cy
            iz = 1.0 / c[:, 2]
            area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0])
            if not (area != 0.0 and np.isfinite(area)) or (cull and not area < 0.0):
                continue
            inv = 1.0 / area
            x0, x1, y0, y1 = np.ceil(u.min()), np.floor(u.max()), np.ceil(v.min()), np.floor(v.max())
            if not (x1 >= 0 and y1 >= 0 and x0 <= W - 1 and y0 <= H - 1 and x0 <= x1 and y0 <= y1):
                continue
            x0, x1, y0, y1 = int(max(x0, 0)), int(min(x1, W - 1)), int(max(y0, 0)), int(min(y1, H - 1))
            ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            du, dv = u[:, None, None] - xs.astype(np.float64), v[:, None, None] - ys.astype(np.float64)
            a = [(du[(k + 1) % 3] * dv[(k + 2) % 3] - du[(k + 2) % 3] * dv[(k + 1) % 3]) * inv for k in range(3)]
            cover = (a[0] >= 0) & (a[1] >= 0) & (a[2] >= 0)
            w = a[0] * iz[0] + a[1] * iz[1] + a[2] * iz[2]
            sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            win = cover & (w > best_w[sl])              # ascending t: an equal 1 / z keeps the lower id
            best_w[sl] = np.where(win, w, best_w[sl])
            best_f[sl] = np.where(win, t, best_f[sl])
            best_l[sl] = np.where(win[..., None], np.stack(a, axis=-1), best_l[sl])
        depth = np.where(best_f >= 0, 1.0 / np.where(best_f >= 0, best_w, 1.0), np.inf).astype(np.float32)
    return depth, best_f.astype(np.int32), best_l.astype(np.float32)


def visibility_of(face_img, faces, n_verts):
    """numpy's statement of bodyfit_raster_visibility_device for one frame: (u8 [n_faces], u8 [n_verts])"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = np.zeros(len(faces), np.uint8)
    ids = np.asarray(face_img).reshape(-1)
    ids = ids[(ids >= 0) & (ids < len(faces))]
    fv[ids] = 1
    vv = np.zeros(n_verts, np.uint8)
    vv[faces[fv.astype(bool)].reshape(-1)] = 1
    return fv, vv


# ---- scenes shared by the CPU and the GPU tests ----------------------------------------------------------------------------
def uv_sphere(centre, radius, n_lat, n_lon, tilt):
    """a closed UV sphere with pole fans, outward normals in the orientation of its faces, tilted about the x axis:
    (n_lat - 1) n_lon + 2 vertices, 2 (n_lat - 1) n_lon faces"""
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    v.append([0.0, 0.0, -1.0])
    v = np.asarray(v)
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = []
    for j in range(n_lon):
        f.append([0, ring(1, j), ring(1, j + 1)])
        f.append([len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    c, s = np.cos(tilt), np.sin(tilt)
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return radius * v @ Rx.T + np.asarray(centre), np.asarray(f, np.int32)


SPHERES_INTR = (300.0, 300.0, 64.0, 64.0)
SPHERES_SIZE = (128, 128)


def two_spheres():
    """Two tilted UV spheres, the small one in front of the large one's edge: closed, self-occluding, 264 vertices, 520 faces.
    Returns (verts f32, faces, intr, size)."""
    v1, f1 = uv_sphere((0.02, -0.01, 3.0), 0.30, 12, 16, 0.4)
    v2, f2 = uv_sphere((0.11, 0.06, 2.5), 0.12, 8, 12, -0.7)
    verts = np.concatenate([v1, v2]).astype(np.float32)
    faces = np.concatenate([f1, f2 + len(v1)]).astype(np.int32)
    return verts, faces, SPHERES_INTR, SPHERES_SIZE


HAND_INTR = (256.0, 256.0, 8.0, 8.0)      # powers of two: the hand-made projections below are exact integers
HAND_SIZE = (16, 16)


def _unproject(u, v, z):
    fx, fy, cx, cy = HAND_INTR
    return [(u - cx) / fx * z, (v - cy) / fy * z, z]


def hand_scenes():
    """name -> (verts f32, faces, intr, size, z_near, cull): small scenes with exact projections (every corner below projects
    to the integers given, at a depth that is a power of two)"""
    P = _unproject
    S = {}
    # a square split along its diagonal: pixel centres lie exactly on the shared edge (u = v) and on the shared vertices
    quad = np.array([P(2, 2, 2.0), P(10, 2, 2.0), P(10, 10, 2.0), P(2, 10, 2.0)], np.float32)
    S["shared_edge"] = (quad, np.array([[0, 2, 1], [0, 3, 2]], np.int32), HAND_INTR, HAND_SIZE, 0.1, False)
    # a fan of four faces about a vertex that is a pixel centre
    fan = np.array([P(6, 6, 2.0), P(2, 2, 2.0), P(10, 2, 2.0), P(10, 10, 2.0), P(2, 10, 2.0)], np.float32)
    S["shared_vertex"] = (fan, np.array([[0, 2, 1], [0, 3, 2], [0, 4, 3], [0, 1, 4]], np.int32), HAND_INTR, HAND_SIZE, 0.1, False)
    tri = np.array([P(2, 2, 2.0), P(12, 3, 2.0), P(5, 12, 2.0)], np.float32)
    S["identical_faces"] = (tri, np.array([[0, 2, 1], [0, 2, 1]], np.int32), HAND_INTR, HAND_SIZE, 0.1, False)
    # face 0 has a corner in front of z_near = 0.5 and is dropped whole; face 1, behind it, shows
    near = np.array([P(2, 2, 1.0), P(12, 3, 0.25), P(5, 12, 1.0), P(1, 1, 4.0), P(14, 1, 4.0), P(7, 14, 4.0)], np.float32)
    S["behind_z_near"] = (near, np.array([[0, 2, 1], [3, 5, 4]], np.int32), HAND_INTR, HAND_SIZE, 0.5, False)
    # collinear corners, a repeated id, and one ordinary face behind them
    flat = np.array([P(2, 2, 1.0), P(6, 6, 1.0), P(10, 10, 1.0), P(1, 1, 4.0), P(14, 1, 4.0), P(7, 14, 4.0)], np.float32)
    S["zero_area"] = (flat, np.array([[0, 1, 2], [0, 1, 1], [3, 5, 4]], np.int32), HAND_INTR, HAND_SIZE, 0.1, False)
    # the same triangle in both orientations at two depths: culling keeps the front one (face 1, the farther)
    both = np.array([P(2, 2, 1.0), P(12, 3, 1.0), P(5, 12, 1.0), P(2, 2, 2.0), P(12, 3, 2.0), P(5, 12, 2.0)], np.float32)
    S["cull"] = (both, np.array([[0, 1, 2], [3, 5, 4]], np.int32), HAND_INTR, HAND_SIZE, 0.1, True)
    S["no_cull"] = (both, np.array([[0, 1, 2], [3, 5, 4]], np.int32), HAND_INTR, HAND_SIZE, 0.1, False)
    # a slanted triangle: depth 1 to 4 across twelve pixels
    slant = np.array([P(1, 2, 1.0), P(14, 3, 4.0), P(4, 13, 2.0)], np.float32)
    S["slanted"] = (slant, np.array([[0, 2, 1]], np.int32), HAND_INTR, HAND_SIZE, 0.1, False)
    return S


def big_and_small(size=(128, 128), n_small=500, seed=3):
    """One face that covers the whole image, at depth 4, beside n_small faces about a pixel across at depth 2 to 3, some of
    them stacked on one pixel: (verts, faces, intr, size)."""
    H, W = size
    intr = (200.0, 200.0, W / 2.0, H / 2.0)
    fx, fy, cx, cy = intr
    rng = np.random.default_rng(seed)
    un = lambda u, v, z: [(u - cx) / fx * z, (v - cy) / fy * z, z]
    verts = [un(-W, -H, 4.0), un(3 * W, -H, 4.0), un(-W, 3 * H, 4.0)]
    faces = [[0, 2, 1]]
    for k in range(n_small):
        c = rng.uniform([0, 0], [W, H]) if k >= 40 else np.array([17.3, 23.6])
        z = rng.uniform(2.0, 3.0)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0, 2.1, 4.2])
        for a in ang:
            verts.append(un(c[0] + 0.9 * np.cos(a), c[1] + 0.9 * np.sin(a), z))
        faces.append([3 * k + 3, 3 * k + 4, 3 * k + 5])
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32), intr, size


def soup_scene(synth, depth, seed=1):
    """surface_ref.mesh_scene's face soup (V = 1000, 2,000 faces of synth.make_faces) moved to `depth` metres: (verts, faces)"""
    import surface_ref
    _, verts, faces = surface_ref.mesh_scene(synth, seed, n_query=0)
    verts = verts.astype(np.float64) + np.array([0.0, 0.0, depth - 3.0])
    return verts.astype(np.float32), faces


def contract_scenes(synth):
    """name -> (verts, faces, intr, size, z_near, cull): every scene the contract is asserted on, pixel by pixel"""
    S = {"two_spheres": two_spheres() + (0.1, False), "two_spheres_culled": two_spheres() + (0.1, True),
         "big_and_small": big_and_small() + (0.1, False)}
    v, f = soup_scene(synth, 3.0)
    S["soup_at_3m"] = (v, f, SPHERES_INTR, SPHERES_SIZE, 0.1, False)
    v, f = soup_scene(synth, 0.9)
    S["soup_at_0.9m"] = (v, f, SPHERES_INTR, SPHERES_SIZE, 0.85, False)       # faces leave the image and cross z_near
    S["soup_at_0.9m_67x45"] = (v, f, (150.0, 150.0, 33.0, 22.0), (45, 67), 0.85, True)
    for name, scene in hand_scenes().items():
        S["hand_" + name] = scene
    return S
