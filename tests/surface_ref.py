"""Test infrastructure (numpy): the f64 brute-force reference of the closest-surface search and of its gradient
(bodyfit_closest_surface_device / bodyfit_closest_surface_vjp_device), chunked so that it stays in memory; an f32 restatement of
the arithmetic of k_closest_surface.hip (every operation rounded to f32, no fused steps, no cull) that shows the bound of
include/bodyfit.h is attainable; check_bounds, which asserts that contract for every query of a frame; and the input sets the
CPU and the GPU tests share.

A frame is (q [nq, 3] f32, verts [V, 3] f32, faces [nf, 3] int)."""
import numpy as np

CHUNK = 128
U = 2.0 ** -24      # unit roundoff of f32
K = 32              # the derived constant of include/bodyfit.h (bodyfit_closest_surface_device)


# ---- f64 reference -----------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _segment(S, D, P):
    """parameter in [0, 1] and squared distance of the closest point of the segment S + t D (D = 0: the point S)"""
    dd = _dot(D, D)
    pos = dd > 0
    t = np.clip(np.where(pos, _dot(P - S, D) / np.where(pos, dd, 1.0), 0.0), 0.0, 1.0)
    r = P - (S + t[..., None] * D)
    return t, _dot(r, r)


def tri_closest64(p, v0, v1, v2):
    """closest point of triangle (v0, v1, v2) to p, broadcasting, f64: (dist2, bary [..., 3]).  The minimum over the three
    edges (each clamped to its segment) and, where the face has an area and the plane projection falls inside, that projection;
    a degenerate face is covered by its edges."""
    p, v0, v1, v2 = (np.asarray(x, np.float64) for x in (p, v0, v1, v2))
    e1, e2, ap = v1 - v0, v2 - v0, p - v0
    tAB, dAB = _segment(v0, e1, p)
    tBC, dBC = _segment(v1, v2 - v1, p)
    tCA, dCA = _segment(v2, v0 - v2, p)
    a, b, c, d1, d2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(ap, e1), _dot(ap, e2)
    det = a * c - b * b
    ok = det > 1e-18 * a * c
    sdet = np.where(ok, det, 1.0)
    v = (c * d1 - b * d2) / sdet
    w = (a * d2 - b * d1) / sdet
    inside = ok & (v >= 0) & (w >= 0) & (v + w <= 1)
    r = ap - v[..., None] * e1 - w[..., None] * e2
    din = np.where(inside, _dot(r, r), np.inf)
    z, o = np.zeros_like(tAB), np.ones_like(tAB)
    cands = [(dAB, (o - tAB, tAB, z)), (dBC, (z, o - tBC, tBC)), (dCA, (tCA, z, o - tCA)), (din, (o - v - w, v, w))]
    best = cands[0][0].copy()
    bary = np.stack(cands[0][1], axis=-1)
    for d, bb in cands[1:]:
        lt = d < best
        best = np.where(lt, d, best)
        bary = np.where(lt[..., None], np.stack(bb, axis=-1), bary)
    return best, bary


def brute_force(q, verts, faces):
    """(d*^2 [nq] f64, argmin [nq], bary [nq, 3] f64) of one frame; (+inf, -1, 0) without faces"""
    nq, nf = q.shape[0], faces.shape[0]
    if nf == 0:
        return np.full(nq, np.inf), np.full(nq, -1, np.int64), np.zeros((nq, 3))
    V = verts.astype(np.float64)
    v0, v1, v2 = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    dmin = np.empty(nq); amin = np.empty(nq, np.int64); bary = np.empty((nq, 3))
    for s in range(0, nq, CHUNK):
        P = q[s:s + CHUNK].astype(np.float64)
        D, _ = tri_closest64(P[:, None, :], v0[None], v1[None], v2[None])
        a = D.argmin(axis=1)
        d, b = tri_closest64(P, v0[a], v1[a], v2[a])
        amin[s:s + CHUNK] = a; dmin[s:s + CHUNK] = d; bary[s:s + CHUNK] = b
    return dmin, amin, bary


def point_at(verts, faces, index, bary):
    """c^ = sum_i b_i v_faces[index][i] in f64 (products of two f32 are exact in f64)"""
    V = verts.astype(np.float64)
    tri = V[faces[index]]                                 # [n, 3 corners, 3]
    return (np.asarray(bary, np.float64)[:, :, None] * tri).sum(axis=1)


def longest_edge(verts, faces, index):
    tri = verts.astype(np.float64)[faces[index]]
    e = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], axis=1)
    return np.sqrt((e * e).sum(axis=2)).max(axis=1)


def vjp(q, verts, faces, index, bary, g):
    """Analytic f64 gradient of sum_i g_i dist2_i of one frame at the fixed (index, bary):
    grad_q [nq, 3] = 2 g_i (p_i - c^_i), grad_v [V, 3] = sum over (i, a) with faces[index_i][a] = v of -2 g_i b_ia (p_i - c^_i),
    and the terms of the f32 error bound: abs_v = sum |term|, loc_v = sum 2 |g_i| b_ia M_i with M_i = |p - v0| + b1 |v1 - v0| +
    b2 |v2 - v0| per component (what the f32 form of p - c^ rounds against), n_v = terms per vertex; loc_q = 2 |g_i| M_i.
    index -1 (or out of range): the query contributes nothing."""
    nq, nv, nf = q.shape[0], verts.shape[0], faces.shape[0]
    index = np.asarray(index).astype(np.int64)
    ok = (index >= 0) & (index < nf)
    gq = np.zeros((nq, 3)); lq = np.zeros((nq, 3))
    gv = np.zeros((nv, 3)); av = np.zeros((nv, 3)); lv = np.zeros((nv, 3)); n_v = np.zeros(nv, np.int64)
    if ok.any():
        ix = index[ok]
        b = np.asarray(bary, np.float64)[ok]
        P = q[ok].astype(np.float64)
        tri = verts.astype(np.float64)[faces[ix]]
        d = P - (b[:, :, None] * tri).sum(axis=1)
        M = np.abs(P - tri[:, 0]) + b[:, 1:2] * np.abs(tri[:, 1] - tri[:, 0]) + b[:, 2:3] * np.abs(tri[:, 2] - tri[:, 0])
        g2 = 2.0 * g[ok].astype(np.float64)[:, None]
        gq[ok] = g2 * d
        lq[ok] = np.abs(g2) * M
        for a in range(3):
            t = -g2 * b[:, a:a + 1] * d
            np.add.at(gv, faces[ix, a], t)
            np.add.at(av, faces[ix, a], np.abs(t))
            np.add.at(lv, faces[ix, a], np.abs(g2) * b[:, a:a + 1] * M)
            np.add.at(n_v, faces[ix, a], 1)
    return gq, gv, av, lv, n_v, lq


# ---- the kernel's arithmetic, in f32 -------------------------------------------------------------------------------------
def prepare_records(verts, faces):
    """the prepared triangle record of k_cs_prepare: f64 from the f32 corners, rounded once to f32.  Returns a dict of [nf]
    (or [nf, 3]) f32 arrays A, u, w, L, cx, t, invBC, invCA and the rotation rot."""
    V = verts.astype(np.float64)
    v = V[faces]                                                    # [nf, 3, 3]
    l2 = np.stack([((v[:, (i + 1) % 3] - v[:, i]) ** 2).sum(axis=1) for i in range(3)], axis=1)
    rot = np.zeros(len(faces), np.int64)
    rot = np.where(l2[:, 1] > l2[np.arange(len(faces)), rot], 1, rot)
    rot = np.where(l2[:, 2] > l2[np.arange(len(faces)), rot], 2, rot)
    ar = np.arange(len(faces))
    A, B, C = v[ar, rot], v[ar, (rot + 1) % 3], v[ar, (rot + 2) % 3]
    L = np.sqrt(l2[ar, rot])
    live = L.astype(np.float32) >= np.float32(1e-30)
    sL = np.where(live, L, 1.0)
    u = np.where(live[:, None], (B - A) / sL[:, None], 0.0)
    e2 = C - A
    cx = _dot(e2, u)
    pr = e2 - cx[:, None] * u
    th = np.sqrt(_dot(pr, pr))
    tall = live & (th > L * 2.0 ** -40) & (th.astype(np.float32) >= np.float32(1e-30))
    w = np.where(tall[:, None], pr / np.where(tall, th, 1.0)[:, None], 0.0)
    th = np.where(tall, th, 0.0)
    cx = np.where(live, np.clip(cx, 0.0, L), 0.0)
    L = np.where(live, L, 0.0)
    Lf, tf = L.astype(np.float32), th.astype(np.float32)
    cxf = np.minimum(cx.astype(np.float32), Lf)
    dbx = cxf.astype(np.float64) - Lf.astype(np.float64)
    bc2 = dbx * dbx + tf.astype(np.float64) ** 2
    ca2 = cxf.astype(np.float64) ** 2 + tf.astype(np.float64) ** 2
    inv = lambda x: np.where(x >= 1e-36, 1.0 / np.where(x >= 1e-36, x, 1.0), 0.0).astype(np.float32)
    return dict(A=A.astype(np.float32), u=u.astype(np.float32), w=w.astype(np.float32), L=Lf, cx=cxf, t=tf, invBC=inv(bc2),
                invCA=inv(ca2), rot=rot, finite=np.isfinite(v).all(axis=(1, 2)))


def _eval_f32(ap, R):
    """closest point (qx, qy) of the record's 2-D triangle and the squared distance, f32 throughout, broadcasting; ap [..., 3]"""
    f = np.float32
    u, w, L, cx, t = R["u"], R["w"], R["L"], R["cx"], R["t"]
    X = ap[..., 0] * u[..., 0] + ap[..., 1] * u[..., 1] + ap[..., 2] * u[..., 2]
    Y = ap[..., 0] * w[..., 0] + ap[..., 1] * w[..., 1] + ap[..., 2] * w[..., 2]
    qx = np.minimum(np.maximum(X, f(0)), L); qy = np.zeros_like(qx)
    ex = X - qx
    best = ex * ex + Y * Y
    tau = np.clip((X * cx + Y * t) * R["invCA"], f(0), f(1))
    sx, sy = tau * cx, tau * t
    r = (X - sx) * (X - sx) + (Y - sy) * (Y - sy)
    lt = r < best
    best = np.where(lt, r, best); qx = np.where(lt, sx, qx); qy = np.where(lt, sy, qy)
    Dx, XL = cx - L, X - L
    tau = np.clip((XL * Dx + Y * t) * R["invBC"], f(0), f(1))
    sx, sy = tau * Dx + L, tau * t
    r = (X - sx) * (X - sx) + (Y - sy) * (Y - sy)
    lt = r < best
    qx = np.where(lt, sx, qx); qy = np.where(lt, sy, qy)
    inside = (t > 0) & (Y >= 0) & (Dx * Y - t * XL >= 0) & (t * X - cx * Y >= 0)
    qx = np.where(inside, X, qx); qy = np.where(inside, Y, qy)
    rr = ap - qx[..., None] * u - qy[..., None] * w
    d2 = rr[..., 0] * rr[..., 0] + rr[..., 1] * rr[..., 1] + rr[..., 2] * rr[..., 2]
    assert d2.dtype == np.float32
    return d2, qx, qy


def kernel_form_f32(q, verts, faces):
    """(dist2 [nq] f32, index [nq], bary [nq, 3] f32) of the kernel's form, every operation rounded to f32, every pair evaluated
    (no cull), lowest index among equal computed distances"""
    nq, nf = q.shape[0], faces.shape[0]
    if nf == 0:
        return np.full(nq, np.inf, np.float32), np.full(nq, -1, np.int64), np.zeros((nq, 3), np.float32)
    R = prepare_records(verts, faces)
    q = q.astype(np.float32)
    d2 = np.empty(nq, np.float32); idx = np.empty(nq, np.int64); bary = np.zeros((nq, 3), np.float32)
    one = np.float32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, nq, CHUNK):
            P = q[s:s + CHUNK]
            ap = P[:, None, :] - R["A"][None]
            D, _, _ = _eval_f32(ap, {k: (v[None] if k != "rot" else v) for k, v in R.items()})
            D = np.where(R["finite"][None] & np.isfinite(D), D, np.inf)
            a = D.argmin(axis=1)
            Rw = {k: v[a] for k, v in R.items()}
            dw, qx, qy = _eval_f32(P - Rw["A"], Rw)
            t, L, cx = Rw["t"], Rw["L"], Rw["cx"]
            wC = np.where(t > 0, np.clip(qy / np.where(t > 0, t, one), 0, 1), 0).astype(np.float32)
            wC = (wC + one) - one
            wB = np.where(L > 0, np.clip((qx - wC * cx) / np.where(L > 0, L, one), 0, 1), 0).astype(np.float32)
            wB = (wB + one) - one
            rest = one - wC
            wB = np.minimum(wB, rest)
            wA = rest - wB
            b = np.zeros((len(a), 3), np.float32)
            ar = np.arange(len(a))
            b[ar, Rw["rot"]] = wA; b[ar, (Rw["rot"] + 1) % 3] = wB; b[ar, (Rw["rot"] + 2) % 3] = wC
            none = ~np.isfinite(D[ar, a])
            d2[s:s + CHUNK] = np.where(none, np.inf, dw); idx[s:s + CHUNK] = np.where(none, -1, a)
            b[none] = 0
            bary[s:s + CHUNK] = b
    return d2, idx, bary


# ---- the contract --------------------------------------------------------------------------------------------------------
def check_bounds(q, verts, faces, dist2, index, bary, ref=None):
    """Asserts the contract of include/bodyfit.h for EVERY query of one frame (finite inputs).  ref: brute_force(q, verts, faces)
    if the caller has it.  Returns (worst optimality excess, worst consistency error), both in units of U (d + h)."""
    nq, nf = q.shape[0], faces.shape[0]
    index = np.asarray(index).astype(np.int64)
    dist2 = np.asarray(dist2); bary = np.asarray(bary)
    if nf == 0:
        assert np.all(index == -1) and np.all(np.isposinf(dist2)) and np.all(bary == 0), "a frame without faces: -1, +inf, 0"
        return 0.0, 0.0
    if nq == 0:
        return 0.0, 0.0
    assert np.all((index >= 0) & (index < nf)), "index out of the frame's range"
    assert bary.dtype == np.float32 and np.all(bary >= 0), "negative weight"
    assert np.all(bary.astype(np.float64).sum(axis=1) == 1.0), "the weights must sum to 1 exactly"
    dstar = np.sqrt((brute_force(q, verts, faces) if ref is None else ref)[0])
    c = point_at(verts, faces, index, bary)
    dhat = np.sqrt(((q.astype(np.float64) - c) ** 2).sum(axis=1))
    h = longest_edge(verts, faces, index)
    opt = (dhat - dstar) / (U * (dstar + h) + 1e-300)
    con = np.abs(np.sqrt(dist2.astype(np.float64)) - dhat) / (U * (dhat + h) + 1e-300)
    bad = opt > K
    assert not bad.any(), ("optimality", int(bad.sum()), float(opt.max()))
    bad = con > K
    assert not bad.any(), ("consistency", int(bad.sum()), float(con.max()))
    return float(opt.max()), float(con.max())


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------
def region_scene():
    """One well-shaped triangle in camera coordinates and queries in each of the seven regions by construction: over the
    interior, beyond each edge, beyond each vertex (at 1 mm, 1 cm and 30 cm off the plane), exactly on every vertex, exactly on
    an edge midpoint (where representable) and on the centroid.  Returns (q, verts, faces, want_region [nq]) with regions
    0 interior, 1..3 edge i -> i+1, 4..6 vertex i."""
    v = np.array([[0.10, 0.20, 3.00], [0.13, 0.21, 3.01], [0.11, 0.24, 2.99]], np.float32)
    V = v.astype(np.float64)
    n = np.cross(V[1] - V[0], V[2] - V[0]); n /= np.linalg.norm(n)
    cen = V.mean(axis=0)
    pts, reg = [], []
    for off in (0.0, 1e-3, -1e-2, 0.3):
        for bw in ([1 / 3, 1 / 3, 1 / 3], [0.6, 0.3, 0.1], [0.05, 0.05, 0.9]):
            pts.append(np.asarray(bw) @ V + off * n); reg.append(0)
        for i in range(3):
            a, b = V[i], V[(i + 1) % 3]
            out = np.cross(b - a, n); out /= np.linalg.norm(out)
            if out @ (cen - a) > 0:
                out = -out
            for s in (0.25, 0.5, 0.8):
                pts.append(a + s * (b - a) + 0.02 * out + off * n); reg.append(1 + i)
            away = V[i] - cen
            pts.append(V[i] + 0.5 * away + off * n); reg.append(4 + i)
    for i in range(3):
        pts.append(V[i]); reg.append(4 + i)
    pts.append(0.5 * (V[0] + V[1])); reg.append(1)
    q = np.asarray(pts).astype(np.float32)
    return q, v, np.array([[0, 1, 2]], np.int32), np.asarray(reg)


def degenerate_scene(seed=0):
    """faces that collapse: a point (three times the same id), a point (three coincident vertices), a segment (a repeated id),
    collinear corners (exactly, on a grid of representable numbers, and to f32 rounding at camera magnitude), a sliver of
    relative height 1e-5, beside two ordinary faces.  Queries: around every face and exactly on corners."""
    rng = np.random.default_rng(seed)
    base = np.array([0.25, -0.5, 3.0])
    v = [base + [0, 0, 0], base + [0.03125, 0, 0], base + [0.0625, 0, 0],             # 0 1 2: exactly collinear
         base + [0.01, 0.02, 0.01], base + [0.01, 0.02, 0.01],                         # 3 4: coincident
         base + [0.02, 0.05, -0.01], base + [0.05, 0.04, 0.02],                        # 5 6
         base + [0.1, 0.1, 0.0], base + [0.1 + 0.02 * 0.3, 0.1 + 0.03 * 0.3, 0.01 * 0.3], base + [0.12, 0.13, 0.01],  # 7 8 9
         base + [0.2, 0.0, 0.0], base + [0.22, 0.0, 0.0], base + [0.21, 2e-7, 0.0]]    # 10 11 12: a sliver
    v = np.asarray(v).astype(np.float32)
    faces = np.array([[5, 5, 5], [3, 4, 3], [5, 6, 5], [0, 1, 2], [2, 0, 1], [7, 8, 9], [10, 11, 12], [0, 5, 6], [3, 6, 9],
                      [4, 3, 4]], np.int32)
    q = [v[rng.integers(0, len(v), 300)] + rng.normal(scale=10.0 ** rng.uniform(-4, -1, (300, 1)), size=(300, 3)), v,
         0.5 * (v[10] + v[11])[None], (v[0] * 0.5 + v[2] * 0.5)[None]]
    return np.concatenate(q).astype(np.float32), v, faces


def mesh_scene(synth, seed, V=1000, n_faces=2000, n_query=600, on_surface=0.3):
    """A synthetic body in camera coordinates (the template of synth.make_model rotated and moved to z = 3 m, f32) with
    synth.make_faces' connectivity (a face soup with ties and degenerate faces), and queries: points on random faces at random
    barycentric positions, displaced along a random direction by 0 (the share `on_surface`), or by 0.1 mm to 10 cm, plus a few
    metres away.  Returns (q, verts, faces)."""
    rng = np.random.default_rng(seed)
    model = synth.make_model(0, n_verts=V)
    faces = synth.make_faces(model, n_faces=n_faces, seed=seed)
    th = 0.3 + 0.1 * seed
    Rm = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    verts = (model.v_template @ Rm.T + np.array([0.1, -0.2, 3.0])).astype(np.float32)
    return surface_queries(rng, verts, faces, n_query, on_surface), verts, faces


def surface_queries(rng, verts, faces, n, on_surface=0.3, outliers=0.02):
    if n == 0 or len(faces) == 0:
        return (np.array([0.0, 0.0, 3.0]) + rng.normal(size=(n, 3))).astype(np.float32)
    t = rng.integers(0, len(faces), n)
    b = rng.dirichlet([1.0, 1.0, 1.0], n)
    c = (b[:, :, None] * verts.astype(np.float64)[faces[t]]).sum(axis=1)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    mag = 10.0 ** rng.uniform(-4, -1, size=(n, 1))
    mag[rng.random(n) < on_surface] = 0.0
    far = rng.random(n) < outliers
    mag[far] = rng.uniform(0.5, 3.0, size=(int(far.sum()), 1))
    return (c + d * mag).astype(np.float32)
