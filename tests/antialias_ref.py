"""Test infrastructure (numpy): the reference statement of the silhouette-edge antialiasing (bodyfit_raster_edges_device,
bodyfit_raster_edge_blend_device, bodyfit_raster_edge_rows_device; include/bodyfit.h) and of its contract, and the scenes the CPU
and the GPU tests share.

The definition is evaluated twice per candidate pair by ONE routine: in extended precision (np.longdouble, 64 significant bits:
the reference) and in f64, operation for operation in the kernel's stated order (numpy never fuses: the kernel form).  Every
discrete decision of the reference's walk is recorded with its margin and its band tau; a decision is SURE when the margin clears
the band, or when the f64 evaluation of its quantity reproduces the extended value exactly (dyadic scenes: the tie rules hold to
the bit).  A pair all of whose decisions are sure is DECIDED; the bound checkers compare values on decided pairs only and check
everything else (written, finite, |w| <= 1/2) everywhere.

A frame is (verts [V, 3] f32, faces [nf, 3] int); the render's images face int32 [H, W] and depth f32 [H, W] are INPUTS."""
import re

import numpy as np

import raster_ref as rr

LD = np.longdouble
U = 2.0 ** -24
EPS = 2.0 ** -53
WALK = 8              # BODYFIT_AA_WALK
K_C = 8               # the derived constants of include/bodyfit.h (bodyfit_raster_edges_device) ...
K_X = 32
SIDE_TOL = 2.0 ** -46
K_B = 2
K_R = 2
G_SHIFT = 2.0 ** -48


def header_constants(text):
    """(walk, k_c, k_x, the shift of the fold band, k_b, k_r, the shift of T_G) as include/bodyfit.h states them"""
    s = text[text.index("SILHOUETTE-EDGE ANTIALIASING"):]
    walk = re.search(r"#define BODYFIT_AA_WALK (\d+)", s)
    k = re.search(r"k_c = (\d+), k_x = (\d+)", s)
    f = re.search(r"\|side\(c\)\|, \|side\(c'\)\| >= 2\^-(\d+) P\^2", s)
    b = re.search(r"k_b = (\d+)", s)
    r = re.search(r"k_r = (\d+)", s)
    g = re.search(r"2\^-(\d+) T_G", s)
    return int(walk.group(1)), int(k.group(1)), int(k.group(2)), int(f.group(1)), int(b.group(1)), int(r.group(1)), int(g.group(1))


def adjacency(faces):
    """[nf, 3] int: per (face, edge e = corners e, (e + 1) % 3) the lowest-id other face that holds both vertex ids, -1 if none or
    if the two ids are equal"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    groups = {}
    for f, ids in enumerate(faces):
        for e in range(3):
            a, b = int(ids[e]), int(ids[(e + 1) % 3])
            if a != b:
                groups.setdefault((min(a, b), max(a, b)), []).append(f)
    adj = np.full(faces.shape, -1, np.int64)
    for f, ids in enumerate(faces):
        for e in range(3):
            a, b = int(ids[e]), int(ids[(e + 1) % 3])
            for g in groups.get((min(a, b), max(a, b)), []):          # ascending by construction
                if g != f:
                    adj[f, e] = g
                    break
    return adj


class Projection:
    """per-face projected corners, areas and "drawn" of one frame in the arithmetic `dtype` (LD: the reference; f64: k_rs_faces')"""

    def __init__(self, verts, faces, intr, size, z_near, cull, dtype):
        H, W = size
        fx, fy, cx, cy = (dtype(float(a)) for a in intr)
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3)
        verts = np.asarray(verts)
        v = verts[self.faces] if len(self.faces) else np.zeros((0, 3, 3), verts.dtype)
        zn = verts.dtype.type(z_near) if verts.dtype == np.float32 else z_near
        with np.errstate(all="ignore"):
            self.valid3d = np.isfinite(v).all(axis=(1, 2)) & (v[:, :, 2] >= zn).all(axis=1)
            vv = np.where(self.valid3d[:, None, None], v, 1).astype(dtype)
            self.X, self.Y, self.Z = vv[:, :, 0], vv[:, :, 1], vv[:, :, 2]
            self.u = fx * (self.X / self.Z) + cx
            self.v = fy * (self.Y / self.Z) + cy
            u, w = self.u, self.v
            self.A = (u[:, 1] - u[:, 0]) * (w[:, 2] - w[:, 0]) - (u[:, 2] - u[:, 0]) * (w[:, 1] - w[:, 0])
            self.drawn = self.valid3d & (self.A != 0) & np.isfinite(self.A) & ((self.A < 0) if cull else True)
            P = np.maximum(np.abs(u), np.abs(w)).max(axis=1) + dtype(max(W, H)) + max(abs(cx), abs(cy)) if len(self.faces) else np.zeros(0)
        self.P = np.asarray(P, np.float64)
        self.intr = (fx, fy, cx, cy)
        self.dtype = dtype


def _walk(pr, adj, t, axis, c0, lo, xn, dec):
    """the walk of the definition in pr's arithmetic; appends (margin, tau, quantities) per decision to dec.  Returns None or the
    hit: dict(face, edge, s, x, d, k, steps, tau_x, den, visited)"""
    D = pr.dtype
    F = pr.faces
    if not pr.valid3d[t]:
        return None
    dec.append((abs(pr.A[t]), rr.AREA_TOL * pr.P[t] ** 2, (pr.A[t],)))
    if not pr.drawn[t]:
        return None
    al, ac = (pr.v, pr.u) if axis else (pr.u, pr.v)
    entry = None
    hi = lo + D(1)
    visited = []
    for step in range(1, WALK + 1):
        visited.append(t)
        P = pr.P[t]
        tau_c = K_C * EPS * P
        cands = []
        for e in range(3):
            a, b = e, (e + 1) % 3
            if entry is not None and {int(F[t, a]), int(F[t, b])} == entry:
                continue
            da, db = ac[t, a] - c0, ac[t, b] - c0
            dec.append((abs(da), tau_c, (da,)))
            dec.append((abs(db), tau_c, (db,)))
            up, dn = bool(da <= 0 < db), bool(db <= 0 < da)
            if up == dn:
                continue
            den = ac[t, b] - ac[t, a]
            s = (c0 - ac[t, a]) / den
            x = al[t, a] + (al[t, b] - al[t, a]) * s
            K = float(abs(al[t, b] - al[t, a]) / abs(den))
            tau_x = K_X * EPS * P * (1.0 + K)
            dec.append((abs(x - lo), tau_x, (x,)))
            dec.append((abs(hi - x), tau_x, (x,)))
            if not (x >= lo and x <= hi):
                continue
            cands.append(dict(edge=e, d=abs(x - xn), s=s, x=x, k=(al[t, b] - al[t, a]) / den, tau_x=tau_x, den=den))
        if not cands:
            return None
        best = cands[0]
        for c in cands[1:]:
            dec.append((abs(c["d"] - best["d"]), c["tau_x"] + best["tau_x"], (c["d"], best["d"])))
            if c["d"] < best["d"]:
                best = c
        e = best["edge"]
        a, b, o = e, (e + 1) % 3, (e + 2) % 3
        t2 = int(adj[t, e])
        sil = t2 < 0
        if not sil:
            if not pr.valid3d[t2]:
                sil = True
            else:
                dec.append((abs(pr.A[t2]), rr.AREA_TOL * pr.P[t2] ** 2, (pr.A[t2],)))
                if not pr.drawn[t2]:
                    sil = True
                else:
                    o2 = [q for q in range(3) if F[t2, q] != F[t, a] and F[t2, q] != F[t, b]]
                    if not o2:
                        sil = True
                    else:
                        o2 = o2[0]
                        eu, ev = pr.u[t, b] - pr.u[t, a], pr.v[t, b] - pr.v[t, a]
                        s1 = eu * (pr.v[t, o] - pr.v[t, a]) - ev * (pr.u[t, o] - pr.u[t, a])
                        s2 = eu * (pr.v[t2, o2] - pr.v[t, a]) - ev * (pr.u[t2, o2] - pr.u[t, a])
                        tau = SIDE_TOL * max(P, pr.P[t2]) ** 2
                        dec.append((abs(s1), tau, (s1,)))
                        dec.append((abs(s2), tau, (s2,)))
                        sil = not ((s1 > 0 and s2 < 0) or (s1 < 0 and s2 > 0))
        if sil:
            return dict(best, face=t, steps=step, visited=visited)
        entry = {int(F[t, a]), int(F[t, b])}
        t = t2
    return None


def pair_eval(pr, adj, face_img, depth_img, i, j, axis, dec):
    """one pair (pixel (i, j), axis) in pr's arithmetic: (w in pr's dtype, hit or None, near_is_q).  The pair must lie in the image."""
    D = pr.dtype
    nF = len(pr.faces)
    qi, qj = (i + 1, j) if axis else (i, j + 1)
    fp, fq = int(face_img[i, j]), int(face_img[qi, qj])
    dp, dq = np.float32(depth_img[i, j]), np.float32(depth_img[qi, qj])
    if not 0 <= fp < nF:
        fp, dp = -1, np.float32(np.inf)
    if not 0 <= fq < nF:
        fq, dq = -1, np.float32(np.inf)
    if fp == fq:
        return D(0), None, 0
    near_q = 0 if dp <= dq else 1
    t = fq if near_q else fp
    if t < 0:
        return D(0), None, near_q
    c0, lo = (D(j), D(i)) if axis else (D(i), D(j))
    xn = lo + D(1) if near_q else lo
    hit = _walk(pr, adj, t, axis, c0, lo, xn, dec)
    if hit is None:
        return D(0), None, near_q
    d = hit["d"]
    dec.append((abs(d - D(0.5)), hit["tau_x"], (d,)))
    to_other = bool(d >= D(0.5))
    alpha = d - D(0.5) if to_other else D(0.5) - d
    to_q = (near_q == 0) if to_other else (near_q == 1)
    return (alpha if to_q else -alpha), hit, near_q


class Edges:
    """what the definition and the contract say about every pair of one frame, from the frame's vertices and the render's images"""

    def __init__(self, verts, faces, intr, size, face_img, depth_img, z_near=0.1, cull=False, reference=True):
        assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an extended-precision long double"
        H, W = size
        self.size, self.intr = (H, W), intr
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3)
        self.verts = np.asarray(verts)
        self.adj = adjacency(self.faces)
        nF = len(self.faces)
        face_img = np.asarray(face_img).astype(np.int64)
        depth_img = np.asarray(depth_img, np.float32)
        self.face_img, self.depth_img = face_img, depth_img
        self.p64 = Projection(verts, faces, intr, size, z_near, cull, np.float64)
        self.pld = Projection(verts, faces, intr, size, z_near, cull, LD) if reference else None
        norm = np.where((face_img >= 0) & (face_img < nF), face_img, -1)
        self.candidate = np.zeros((H, W, 2), bool)
        self.candidate[:, :-1, 0] = norm[:, :-1] != norm[:, 1:]
        self.candidate[:-1, :, 1] = norm[:-1, :] != norm[1:, :]
        self.w64 = np.zeros((H, W, 2))                   # the kernel form, before the store
        self.w_ref = np.zeros((H, W, 2), LD)             # the reference
        self.decided = np.ones((H, W, 2), bool)
        self.tau_w = np.zeros((H, W, 2))
        self.hits, self.hits64 = {}, {}
        self.min_margin, self.n_decisions, self.n_exact_ties = np.inf, 0, 0
        with np.errstate(all="ignore"):
            for i, j, axis in zip(*np.nonzero(self.candidate)):
                key = (int(i), int(j), int(axis))
                d64 = []
                w, hit, nq = pair_eval(self.p64, self.adj, face_img, depth_img, key[0], key[1], key[2], d64)
                self.w64[key] = w
                if hit is not None and w != 0:
                    self.hits64[key] = dict(hit, near_q=nq)
                if not reference:
                    continue
                dld = []
                w, hit, nq = pair_eval(self.pld, self.adj, face_img, depth_img, key[0], key[1], key[2], dld)
                self.w_ref[key] = w
                if hit is not None:
                    self.tau_w[key] = U * float(abs(w)) + 2 * hit["tau_x"]
                    if w != 0:
                        self.hits[key] = dict(hit, near_q=nq)
                for k, (margin, tau, q) in enumerate(dld):
                    self.n_decisions += 1
                    if margin >= tau:
                        self.min_margin = min(self.min_margin, float(margin))
                        continue
                    exact = k < len(d64) and len(d64[k][2]) == len(q) and all(LD(a) == b for a, b in zip(d64[k][2], q))
                    if exact:
                        self.n_exact_ties += 1
                        continue
                    self.decided[key] = False
                    break
        self.w_kernel = self.w64.astype(np.float32)

    def census(self):
        """(candidate pairs, blended pairs, pairs whose walk visited more than one face, undecided candidate pairs)"""
        hits = self.hits if self.pld is not None else self.hits64
        return (int(self.candidate.sum()), len(hits), sum(1 for h in hits.values() if h["steps"] > 1),
                int((self.candidate & ~self.decided).sum()))

    def undecided_share(self):
        n = int(self.candidate.sum())
        return float((self.candidate & ~self.decided).sum()) / max(n, 1)

    def undecided_pixels(self):
        """bool [H, W]: the two pixels of every undecided pair"""
        H, W = self.size
        bad = np.zeros((H, W), bool)
        und = self.candidate & ~self.decided
        bad |= und[:, :, 0] | und[:, :, 1]
        bad[:, 1:] |= und[:, :-1, 0]
        bad[1:, :] |= und[:-1, :, 1]
        return bad


def check_weights(E, w):
    """Asserts the weight image of one frame (f32 [H, W, 2]): every entry finite and |w| <= 1/2, 0 on every pair that is not a
    candidate or would leave the image, and |w - w*| <= u |w*| + 2 tau_x on every decided pair.  Returns the worst error in units
    of the bound."""
    H, W = E.size
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.shape == (H, W, 2)
    assert np.all(np.isfinite(w)) and np.all(np.abs(w) <= 0.5), "a weight is not finite or exceeds 1/2"
    assert np.all(w[~E.candidate] == 0), "a pair of equal ids, or one that leaves the image, holds a weight"
    ok = E.candidate & E.decided
    err = np.abs(w.astype(LD) - E.w_ref)[ok]
    lim = E.tau_w[ok]
    zero = ok & (E.w_ref == 0)
    assert np.all(w[zero & (E.tau_w == 0)] == 0), "a decided pair that does not blend holds a weight"
    bad = err > lim
    assert not bad.any(), ("weights", int(bad.sum()), [k for k in zip(*np.nonzero(ok))][int(np.argmax(bad))])
    pos = lim > 0
    return float((err[pos] / lim[pos]).max()) if pos.any() else 0.0


def blend_exact(w, img, transpose=False):
    """(out [H, W, C] LD, T [H, W, C] LD): the blend of img by the weight image w (f32 as the kernels return it, or the reference's own
    extended weights), or its adjoint, exact to extended precision, with the sum of the absolute values of its terms"""
    w = np.asarray(w)
    w = (w if w.dtype == LD else w.astype(np.float32)).astype(LD)
    x = np.asarray(img).astype(LD)
    if x.ndim == 2:
        x = x[:, :, None]
    H, W, _ = x.shape
    out, T = x.copy(), np.abs(x)
    # per axis: p = the pixel, q = its neighbour; w > 0: q receives w (x[p] - x[q]); w < 0: p receives |w| (x[q] - x[p])
    for axis in (0, 1):
        wa = (w[:, :-1, 0] if axis == 0 else w[:-1, :, 1])[:, :, None]
        p = (slice(None), slice(0, W - 1)) if axis == 0 else (slice(0, H - 1), slice(None))
        q = (slice(None), slice(1, W)) if axis == 0 else (slice(1, H), slice(None))
        pos, neg = np.maximum(wa, 0), np.maximum(-wa, 0)
        if not transpose:
            out[q] += pos * (x[p] - x[q]); T[q] += pos * np.abs(x[p] - x[q])
            out[p] += neg * (x[q] - x[p]); T[p] += neg * np.abs(x[q] - x[p])
        else:
            out[q] -= pos * x[q]; T[q] += pos * np.abs(x[q])
            out[p] += pos * x[q]; T[p] += pos * np.abs(x[q])
            out[p] -= neg * x[p]; T[p] += neg * np.abs(x[p])
            out[q] += neg * x[p]; T[q] += neg * np.abs(x[p])
    return out, T


def blend_slack(tau_w, img):
    """f64 [H, W, C]: by how much a pixel of the blend can move when every pair's weight moves by its bound tau_w (whichever of
    the two pixels receives)"""
    x = np.asarray(img, np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    out = np.zeros(x.shape)
    dx, dy = np.abs(x[:, 1:] - x[:, :-1]) * tau_w[:, :-1, 0, None], np.abs(x[1:] - x[:-1]) * tau_w[:-1, :, 1, None]
    out[:, 1:] += dx; out[:, :-1] += dx
    out[1:] += dy; out[:-1] += dy
    return out


def blend_kernel_form(w, img, transpose=False):
    """f32 [H, W, C]: k_rs_edge_blend's arithmetic, f64 in the order left, right, up, down"""
    w = np.asarray(w, np.float32)
    x = np.asarray(img, np.float32).astype(np.float64)
    H, W, C = x.shape
    out = x.copy()
    for i in range(H):
        for j in range(W):
            w4 = [(w[i, j - 1, 0] if j > 0 else 0.0, (i, j - 1)), (-w[i, j, 0] if j + 1 < W else 0.0, (i, j + 1)),
                  (w[i - 1, j, 1] if i > 0 else 0.0, (i - 1, j)), (-w[i, j, 1] if i + 1 < H else 0.0, (i + 1, j))]
            acc = x[i, j].copy()
            for a, nb in w4:
                a = np.float64(a)
                if a == 0 or (a < 0 and not transpose):
                    continue
                if not transpose:
                    acc = acc + a * (x[nb] - x[i, j])
                elif a > 0:
                    acc = acc - a * x[i, j]
                else:
                    acc = acc + (-a) * x[nb]
            out[i, j] = acc
    return out.astype(np.float32)


def check_blend(w, img, out, transpose=False):
    """Asserts |out - out*| <= k_b u T at EVERY pixel and channel of one frame, out* the exact blend by the given f32 weights.
    Returns the worst error in units of the bound."""
    out = np.asarray(out)
    assert out.dtype == np.float32 and np.all(np.isfinite(out))
    want, T = blend_exact(w, img, transpose)
    assert out.shape == want.shape
    err = np.abs(out.astype(LD) - want)
    lim = K_B * U * T
    assert np.all(out[T == 0] == 0)
    assert np.all(err <= lim), ("blend", int((err > lim).sum()), float((err[T > 0] / lim[T > 0]).max()))
    return float((err[T > 0] / lim[T > 0]).max()) if (T > 0).any() else 0.0


def pair_codes(w):
    """int32 [N]: 2 (i W + j) + axis of the non-zero entries of one frame's weight image, ascending"""
    return np.nonzero(np.asarray(w).reshape(-1))[0].astype(np.int32)


def exact_rows(E, codes, img, grad):
    """the reference's rows of the listed pairs of one frame: (index [2 N], corner [2 N], coef [2 N] LD, dir [2 N, 3] LD, dcoef [2 N],
    ddir [2 N, 3], decided [N]); dcoef / ddir are the contract's bounds.  index -1: the reference does not blend the pair."""
    H, W = E.size
    img = np.asarray(img, np.float32).astype(LD).reshape(H, W, -1)
    grad = np.asarray(grad, np.float32).astype(LD).reshape(H, W, -1)
    N = len(codes)
    index, corner = np.full(2 * N, -1, np.int64), np.zeros(2 * N, np.int64)
    coef, direction = np.zeros(2 * N, LD), np.zeros((2 * N, 3), LD)
    dcoef, ddir = np.zeros(2 * N), np.zeros((2 * N, 3))
    decided = np.ones(N, bool)
    pr = E.pld
    fx, fy, _, _ = pr.intr
    for n, code in enumerate(codes):
        axis, pix = int(code) & 1, int(code) >> 1
        i, j = divmod(pix, W)
        key = (i, j, axis)
        if not (0 <= pix < H * W and (i + 1 < H if axis else j + 1 < W)):
            continue
        decided[n] = bool(E.decided[key]) or not E.candidate[key]
        hit = E.hits.get(key)
        if hit is None:
            continue
        p, q = (i, j), ((i + 1, j) if axis else (i, j + 1))
        near, other = (q, p) if hit["near_q"] else (p, q)
        r = q if E.w_ref[key] > 0 else p
        terms = grad[r] * (img[near] - img[other])
        G = terms.sum() * (-1 if hit["near_q"] else 1)
        TG = float(np.abs(terms).sum())
        t, e, s, k = hit["face"], hit["edge"], hit["s"], hit["k"]
        tau_s = K_X * EPS * pr.P[t] / float(abs(hit["den"]))
        tau_k = tau_s * (1.0 + float(abs(k)))
        for c, (a, cf) in enumerate(((e, G * (1 - s)), ((e + 1) % 3, G * s))):
            X, Y, Z = pr.X[t, a], pr.Y[t, a], pr.Z[t, a]
            gu = np.array([fx / Z, LD(0), -fx * X / (Z * Z)], LD)
            gv = np.array([LD(0), fy / Z, -fy * Y / (Z * Z)], LD)
            along, across = (gv, gu) if axis else (gu, gv)
            row = 2 * n + c
            index[row], corner[row] = t, a
            coef[row], direction[row] = cf, along - k * across
            dcoef[row] = K_R * U * float(abs(cf)) + float(abs(G)) * tau_s + G_SHIFT * TG
            ddir[row] = K_R * U * (np.abs(along) + abs(k) * np.abs(across)).astype(np.float64) + tau_k * np.abs(across).astype(np.float64)
    return index, corner, coef, direction, dcoef, ddir, decided


def rows_kernel_form(E, codes, img, grad):
    """(index int32 [2 N], bary f32 [2 N, 3], coef f32 [2 N], dir f32 [2 N, 3]) by k_rs_edge_rows' arithmetic, f64 in its order"""
    H, W = E.size
    img = np.asarray(img, np.float32).astype(np.float64).reshape(H, W, -1)
    grad = np.asarray(grad, np.float32).astype(np.float64).reshape(H, W, -1)
    N = len(codes)
    index = np.full(2 * N, -1, np.int32)
    bary, coef, direction = np.zeros((2 * N, 3), np.float32), np.zeros(2 * N, np.float32), np.zeros((2 * N, 3), np.float32)
    pr = E.p64
    fx, fy, _, _ = pr.intr
    for n, code in enumerate(codes):
        axis, pix = int(code) & 1, int(code) >> 1
        i, j = divmod(pix, W)
        hit = E.hits64.get((i, j, axis)) if 0 <= pix < H * W else None
        if hit is None:
            continue
        p, q = (i, j), ((i + 1, j) if axis else (i, j + 1))
        near, other = (q, p) if hit["near_q"] else (p, q)
        r = q if E.w64[i, j, axis] > 0 else p
        G = np.float64(0)
        for c in range(img.shape[2]):
            G = G + grad[r][c] * (img[near][c] - img[other][c])
        if hit["near_q"]:
            G = -G
        t, e, s, k = hit["face"], hit["edge"], hit["s"], hit["k"]
        for c, (a, cf) in enumerate(((e, G * (1.0 - s)), ((e + 1) % 3, G * s))):
            X, Y, Z = pr.X[t, a], pr.Y[t, a], pr.Z[t, a]
            iz = 1.0 / Z
            ax, ay = fx * iz, fy * iz
            zu, zv = (ax * X) * iz, (ay * Y) * iz
            m = (-(k * ax), ay, k * zu - zv) if axis else (ax, -(k * ay), k * zv - zu)
            row = 2 * n + c
            index[row], bary[row, a], coef[row], direction[row] = t, 1.0, cf, m
    return index, bary, coef, direction


def check_rows(E, codes, img, grad, index, bary, coef, direction):
    """Asserts the rows kernel's outputs for the listed pairs of one frame: every entry finite; on decided pairs the reference's
    face (or -1, with zero rows), a one-hot bary at the reference's corner, and coef / dir within the contract.  Returns (worst coef,
    worst dir) in units of their bounds, and the reference's rows."""
    N = len(codes)
    index, bary, coef, direction = (np.asarray(a) for a in (index, bary, coef, direction))
    assert index.shape == (2 * N,) and bary.shape == (2 * N, 3) and coef.shape == (2 * N,) and direction.shape == (2 * N, 3)
    assert bary.dtype == coef.dtype == direction.dtype == np.float32
    assert np.all(np.isfinite(bary)) and np.all(np.isfinite(coef)) and np.all(np.isfinite(direction))
    assert np.all((index >= -1) & (index < len(E.faces)))
    void = index < 0
    assert np.all(bary[void] == 0) and np.all(coef[void] == 0) and np.all(direction[void] == 0), "a void row holds zeros"
    ref = exact_rows(E, codes, img, grad)
    ri, rc, rcoef, rdir, dcoef, ddir, decided = ref
    ok = np.repeat(decided, 2)
    assert np.array_equal(index[ok], ri[ok]), ("rows: face", int((index[ok] != ri[ok]).sum()))
    live = ok & (ri >= 0)
    onehot = np.zeros((2 * N, 3), np.float32)
    onehot[np.arange(2 * N), rc] = 1
    assert np.array_equal(bary[live], onehot[live]), "rows: the corner"
    e1 = np.abs(coef.astype(LD) - rcoef)[live]
    e2 = np.abs(direction.astype(LD) - rdir)[live]
    assert np.all(e1 <= dcoef[live]), ("rows: coef", float((e1 / dcoef[live]).max()))
    assert np.all(e2 <= ddir[live] + 1e-300), ("rows: dir", float((e2 / (ddir[live] + 1e-300)).max()))
    worst = (float((e1 / np.maximum(dcoef[live], 1e-300)).max()) if live.any() else 0.0,
             float((e2 / np.maximum(ddir[live], 1e-300)).max()) if live.any() else 0.0)
    return worst, ref


def vertex_gradient(faces, n_verts, ref):
    """(G* [V, 3] LD, B [V, 3] f64) from exact_rows' output: the exact vertex gradient of the listed pairs and the bound on what the
    rows' own errors (dcoef, ddir) can move it by"""
    ri, rc, rcoef, rdir, dcoef, ddir, _ = ref
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    G, B = np.zeros((n_verts, 3), LD), np.zeros((n_verts, 3))
    live = ri >= 0
    ids = faces[ri[live], rc[live]]
    np.add.at(G, ids, rcoef[live, None] * rdir[live])
    np.add.at(B, ids, dcoef[live, None] * (np.abs(rdir[live]).astype(np.float64) + ddir[live]) + np.abs(rcoef[live]).astype(np.float64)[:, None] * ddir[live])
    return G, B


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def _hand(points, faces, edit=None, cull=False):
    v = np.array([rr._unproject(u, w, z) for u, w, z in points], np.float32)
    return dict(verts=v, faces=np.asarray(faces, np.int32), intr=rr.HAND_INTR, size=rr.HAND_SIZE, z_near=0.1, cull=cull, edit=edit)


def _clear_column(col):
    def edit(face, depth):
        face, depth = face.copy(), depth.copy()
        face[:, col], depth[:, col] = -1, np.inf
        return face, depth
    return edit


def _flat_depth(z):
    def edit(face, depth):
        return face, np.where(face >= 0, np.float32(z), np.float32(np.inf)).astype(np.float32)
    return edit


def aa_hand_scenes():
    """name -> scene: exact (dyadic) projections at power-of-two depths for the tie rules; every f64 operation of the kernel form is
    exact on them, so the weights are the reference's to the bit"""
    S = {}
    # the left rim at x = 4: the crossing is the near pixel's centre, d = 0, alpha = 1/2
    S["aa_centre"] = _hand([(4, 2, 2.0), (12, 2, 2.0), (4, 10, 2.0)], [[0, 2, 1]])
    # the left rim at x = 4.5: d = 1/2, alpha = 0
    S["aa_half"] = _hand([(4.5, 2, 2.0), (12.5, 2, 2.0), (4.5, 10, 2.0)], [[0, 2, 1]])
    # the left rim at x = 4 with column 4 emptied in the images: near pixel 5, d = 1, the other pixel receives 1/2
    S["aa_one"] = _hand([(4, 2, 2.0), (12, 2, 2.0), (4, 10, 2.0)], [[0, 2, 1]], edit=_clear_column(4))
    # a rim vertex (4.25, 6) exactly on scanline 6 between pixels 4 and 5: of the two rim edges that meet there one crosses
    S["aa_vertex_on_scanline"] = _hand([(5, 2, 2.0), (4.25, 6, 2.0), (5, 10, 2.0), (12, 7, 2.0)], [[0, 1, 3], [1, 2, 3]])
    # a single open triangle: every edge is a boundary edge
    S["aa_open_triangle"] = _hand([(2.25, 2.5, 2.0), (12.5, 3.25, 2.0), (5.75, 12.5, 4.0)], [[0, 2, 1]])
    # a flat quad split along its diagonal: no blend across the unfolded edge, blends on the rim
    S["aa_flat_quad"] = _hand([(2.25, 2.25, 2.0), (10.25, 2.25, 2.0), (10.25, 10.25, 2.0), (2.25, 10.25, 2.0)], [[0, 2, 1], [0, 3, 2]])
    # a strip 5/16 of a pixel wide (the dyadic number next to one third) along the left rim of a quad: a walk of three faces
    S["aa_strip"] = _hand([(4.25, 2, 2.0), (4.25, 10, 2.0), (4.5625, 2, 2.0), (4.5625, 10, 2.0), (12, 2, 2.0), (12, 10, 2.0)],
                          [[0, 1, 3], [0, 3, 2], [2, 3, 5], [2, 5, 4]])
    # two identical faces: each is the other's neighbour on every edge, and folded over it
    S["aa_twins"] = _hand([(2.25, 2, 2.0), (10.25, 2, 2.0), (2.25, 10, 2.0)], [[0, 2, 1], [0, 2, 1]])
    # two faces with a gap between x = 6.25 and x = 6.75 and EQUAL depths in the image: the near pixel is p
    S["aa_equal_depth"] = _hand([(2, 2, 2.0), (6.25, 2, 2.0), (6.25, 12, 2.0), (6.75, 2, 2.0), (12, 2, 2.0), (6.75, 12, 2.0)],
                                [[0, 2, 1], [3, 5, 4]], edit=_flat_depth(2.0))
    return S


EXACT = tuple(aa_hand_scenes())


def scenes(synth):
    """name -> dict(verts, faces, intr, size, z_near, cull, edit): every scene the contract is asserted on"""
    C = rr.contract_scenes(synth)
    S = {}
    for name in ["two_spheres", "two_spheres_culled", "soup_at_0.9m_67x45"] + [n for n in C if n.startswith("hand_")]:
        v, f, intr, size, z_near, cull = C[name]
        S[name] = dict(verts=v, faces=f, intr=intr, size=size, z_near=z_near, cull=cull, edit=None)
    S.update(aa_hand_scenes())
    return S


def images_of(scene, verts=None, render=None):
    """(face int32 [H, W], depth f32 [H, W]) of a scene: the render (by default raster_ref.kernel_form_f64) with the scene's edit"""
    v = scene["verts"] if verts is None else verts
    if render is None:
        depth, face, _ = rr.kernel_form_f64(v, scene["faces"], scene["intr"], scene["size"], scene["z_near"], scene["cull"])
    else:
        face, depth = render
    if scene["edit"] is not None:
        face, depth = scene["edit"](np.asarray(face), np.asarray(depth))
    return np.ascontiguousarray(face, np.int32), np.ascontiguousarray(depth, np.float32)


def edges_of(scene, verts=None, render=None, reference=True):
    face, depth = images_of(scene, verts, render)
    v = scene["verts"] if verts is None else verts
    return Edges(v, scene["faces"], scene["intr"], scene["size"], face, depth, scene["z_near"], scene["cull"], reference)
