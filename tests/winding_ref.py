"""Test infrastructure (numpy): the references of the mesh winding number (bodyfit_surface_winding_device, k_winding.hip), of the
vertex normals (bodyfit_surface_vertex_normals_device) and of the self-penetration term over them (torch_layer.SelfPenetrationTerm),
on top of tests/surface_ref.py and tests/oriented_ref.py: winding64, the f64 value of the definition; bound64, the B_i of the contract
in include/bodyfit.h; kernel_form_f32, an all-f32 restatement of the kernel's pair arithmetic (the fused steps rounded twice, as
oriented_ref._fma32 does); atan_poly, the kernel's arctangent polynomial, whose truncation error is a figure of the contract;
vertex_normals64; self_penetration64, the term with its gradient; and the scenes the CPU and the GPU tests share.

A frame is (q [nq, 3] f32, verts [V, 3] f32, faces [nf, 3] int); skip [nq] int or None: the faces that have skip[i] >= 0 among their
corner IDS are left out for row i."""
import numpy as np

import oriented_ref as orf
import surface_ref as sr

U = sr.U
K = 64              # rounding of num and den, in units of u l_t / |z_t|   (derived in include/bodyfit.h)
K_S = 16            # the arctangent's own error, the fixed-point step and the final rounding, in units of u per counted face
P_TRUNC = 0.14      # |atan_poly(x) - atan(x)| <= P_TRUNC u on |x| <= ATAN_REDUCED, part of K_S (asserted in tests/test_winding.py)
ATAN_SPLIT = 0.41421357     # tan(pi / 8) as the kernel's f32 constant
ATAN_REDUCED = 0.4142137    # the reduced argument stays below this (the split constant and the quotient's roundings)
ATAN_C = (8.05374449538e-2, -1.38776856032e-1, 1.99777106478e-1, -3.33329491539e-1)   # Cephes atanf, highest power first
CHUNK = 64


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def icosphere(subdiv, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts [V, 3] f32, faces [nf, 3] int32), outward oriented: an icosahedron subdivided `subdiv` times, every vertex pushed
    to the sphere in f64 and rounded once (subdiv 2: 162 vertices, 320 faces; 3: 642, 1,280)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        g = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    verts = (np.array(v) * radius + np.asarray(center, np.float64)).astype(np.float32)
    faces = np.array(f, np.int32)
    # outward: the face normal agrees with the centroid's direction from the centre
    tri = verts.astype(np.float64)[faces] - np.asarray(center, np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.all((n * tri.mean(axis=1)).sum(axis=1) > 0)
    return verts, faces


def uv_sphere(segments, rings, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts, faces) of a closed, outward oriented UV sphere: two poles and rings - 1 latitude circles of `segments` vertices:
    segments (rings - 1) + 2 vertices and 2 segments (rings - 1) faces (84 x 83: 6,890 and 13,776, SMPL's counts)"""
    lat = np.pi * np.arange(1, rings) / rings
    lon = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None], np.sin(lat)[:, None] * np.sin(lon)[None],
                     np.broadcast_to(np.cos(lat)[:, None], (rings - 1, segments))], axis=2).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * radius + np.asarray(center, np.float64)
    idx = lambda r, s: 1 + r * segments + (s % segments)
    south = 1 + (rings - 1) * segments
    f = []
    for s in range(segments):
        f.append((0, idx(0, s), idx(0, s + 1)))
        for r in range(rings - 2):
            f.append((idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)))
            f.append((idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)))
        f.append((south, idx(rings - 2, s + 1), idx(rings - 2, s)))
    return verts.astype(np.float32), np.array(f, np.int32)


B_RADIUS, B_CENTER = 0.7, (1.2, 0.0, 0.0)


def two_spheres(subdiv, shift=(0.0, 0.0, 0.0)):
    """The two-sphere scene: the unit icosphere A at the origin and the icosphere B of radius 0.7 about (1.2, 0, 0) + shift, both
    subdivided `subdiv` times, as ONE mesh (B's ids behind A's).  subdiv 2: 324 vertices, 640 faces; 3: 1,284 and 2,560.
    Returns (verts, faces, nA): nA the number of A's vertices."""
    va, fa = icosphere(subdiv)
    vb, fb = icosphere(subdiv, B_RADIUS, np.asarray(B_CENTER) + np.asarray(shift))
    return np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)]).astype(np.int32), len(va)


def two_spheres_truth(verts, nA, shift=(0.0, 0.0, 0.0)):
    """[V] bool, analytic: a vertex of A inside the ball of B, a vertex of B inside the ball of A"""
    v = verts.astype(np.float64)
    inside = np.zeros(len(v), bool)
    inside[:nA] = np.linalg.norm(v[:nA] - (np.asarray(B_CENTER) + np.asarray(shift)), axis=1) < B_RADIUS
    inside[nA:] = np.linalg.norm(v[nA:], axis=1) < 1.0
    return inside


def fan(valence=40, height=0.3):
    """an open fan: apex 0 at (0, 0, height) over a rim of `valence` vertices on the unit circle, normals upward"""
    a = 2.0 * np.pi * np.arange(valence) / valence
    verts = np.concatenate([[[0.0, 0.0, height]], np.stack([np.cos(a), np.sin(a), np.zeros(valence)], axis=1)]).astype(np.float32)
    faces = np.array([(0, 1 + k, 1 + (k + 1) % valence) for k in range(valence)], np.int32)
    return verts, faces


def hemisphere(subdiv=2):
    """the faces of the unit icosphere whose centroid has z > 0: an open mesh"""
    v, f = icosphere(subdiv)
    return v, np.ascontiguousarray(f[v.astype(np.float64)[f].mean(axis=1)[:, 2] > 0])


# ---- f64 reference -----------------------------------------------------------------------------------------------------------
def _pairs64(q, verts, faces):
    """(num, den, l) [nq, nf] f64 of van Oosterom-Strackee, from the f32 inputs"""
    V = verts.astype(np.float64)
    P = q.astype(np.float64)[:, None, :]
    a, b, c = V[faces[:, 0]][None] - P, V[faces[:, 1]][None] - P, V[faces[:, 2]][None] - P
    la, lb, lc = (np.sqrt((x * x).sum(axis=-1)) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(axis=-1)
    den = la * lb * lc + (a * b).sum(axis=-1) * lc + (b * c).sum(axis=-1) * la + (c * a).sum(axis=-1) * lb
    return num, den, la * lb * lc


def _counted(faces, skip, s, e):
    if skip is None:
        return np.ones((e - s, len(faces)), bool)
    sk = np.asarray(skip)[s:e, None, None]
    return ~((faces[None] == sk) & (sk >= 0)).any(axis=2)


def winding64(q, verts, faces, skip=None):
    """w [nq] f64 = (1 / 4 pi) sum_t 2 atan2(num, den) over the counted faces; atan2(0, 0) = 0; NaN propagates (a non-finite
    corner of a counted face, a NaN query)"""
    nq = len(q)
    w = np.zeros(nq)
    if len(faces) == 0:
        return w
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, nq, CHUNK):
            num, den, _ = _pairs64(q[s:s + CHUNK], verts, faces)
            th = np.where(_counted(faces, skip, s, min(s + CHUNK, nq)), np.arctan2(num, den), 0.0)
            w[s:s + CHUNK] = th.sum(axis=1) / (2.0 * np.pi)
    return w


def bound64(q, verts, faces, skip=None):
    """B_i [nq] f64 = (u / 2 pi) sum over the counted faces of (K l_t / |z_t| + K_S); +inf where a counted |z_t| = 0 with l_t > 0
    (the query on an edge); a counted face with l_t = 0 (the query on a corner) contributes K_S alone: its num and den are exact
    zeros"""
    nq = len(q)
    B = np.zeros(nq)
    if len(faces) == 0:
        return B
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(0, nq, CHUNK):
            num, den, l = _pairs64(q[s:s + CHUNK], verts, faces)
            z = np.hypot(num, den)
            r = np.where(l > 0, l / z, 0.0)
            t = np.where(_counted(faces, skip, s, min(s + CHUNK, nq)), K * r + K_S, 0.0)
            B[s:s + CHUNK] = U / (2.0 * np.pi) * t.sum(axis=1)
    return B


# ---- the kernel's arithmetic, in f32 -------------------------------------------------------------------------------------------
_f = np.float32
_fma = orf._fma32


def atan_poly(x):
    """the kernel's polynomial for atan on the reduced range, in the precision of x: x + x z (((c0 z + c1) z + c2) z + c3), z = x^2"""
    z = x * x
    p = x.dtype.type(ATAN_C[0])
    for c in ATAN_C[1:]:
        p = p * z + x.dtype.type(c)
    return p * z * x + x


def atan2_f32(y, x):
    """k_winding.hip's atan2 on f32 arrays: the smaller over the larger magnitude, or (mn - mx) / (mn + mx) behind pi / 4 above
    tan(pi / 8); the polynomial; the octant by pi / 2 - r and pi - r; the sign of y.  (0, 0) gives 0."""
    ay, ax = np.abs(y), np.abs(x)
    swap = ay > ax
    mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
    hi = mn > _f(ATAN_SPLIT) * mx
    n = np.where(hi, mn - mx, mn)
    d = np.where(hi, mn + mx, mx)
    t = np.where(d == 0, _f(0), n / np.where(d == 0, _f(1), d)).astype(np.float32)
    z = t * t
    p = _f(ATAN_C[0])
    for c in ATAN_C[1:]:
        p = _fma(p, z, np.full_like(z, _f(c)))
    r = _fma(p * z, t, t)
    r = np.where(hi, r + _f(np.pi / 4), r)
    r = np.where(swap, _f(np.pi / 2) - r, r)
    r = np.where(x < 0, _f(np.pi) - r, r)
    assert r.dtype == np.float32
    return np.copysign(r, y)


def _dot_f32(a, b):
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def kernel_form_f32(q, verts, faces, skip=None):
    """w [nq] f32 of the kernel's form: per pair in f32 from the differences to the query (the dots and the cross product with the
    kernel's fused steps), atan2_f32, the half angles rounded to multiples of 2^-32 and summed exactly, one rounding of sum / 2 pi"""
    nq = len(q)
    w = np.zeros(nq, np.float32)
    if len(faces) == 0:
        return w
    V = verts.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, nq, CHUNK):
            P = q[s:s + CHUNK].astype(np.float32)[:, None, :]
            a, b, c = V[faces[:, 0]][None] - P, V[faces[:, 1]][None] - P, V[faces[:, 2]][None] - P
            assert a.dtype == np.float32
            la, lb, lc = np.sqrt(_dot_f32(a, a)), np.sqrt(_dot_f32(b, b)), np.sqrt(_dot_f32(c, c))
            n = np.stack([_fma(b[..., 1], c[..., 2], -(b[..., 2] * c[..., 1])), _fma(b[..., 2], c[..., 0], -(b[..., 0] * c[..., 2])),
                          _fma(b[..., 0], c[..., 1], -(b[..., 1] * c[..., 0]))], axis=-1)
            num = _dot_f32(a, n)
            den = _fma(_dot_f32(a, b), lc, _fma(_dot_f32(b, c), la, _fma(_dot_f32(c, a), lb, la * lb * lc)))
            assert num.dtype == np.float32 and den.dtype == np.float32
            th = np.where(_counted(faces, skip, s, min(s + CHUNK, nq)), atan2_f32(num, den), _f(0))
            fixed = np.rint(th.astype(np.float64) * 2.0 ** 32)
            w[s:s + CHUNK] = (fixed.sum(axis=1) * 2.0 ** -32 / (2.0 * np.pi)).astype(np.float32)
    return w


# ---- vertex normals ------------------------------------------------------------------------------------------------------------
def vertex_normals64(verts, faces):
    """(n [V, 3] f64, cond [V]): the area-weighted vertex normals, normalise(sum over the faces that hold the vertex of (v1 - v0) x
    (v2 - v0)), every face once; 0 for a vertex without a face, a zero sum or a non-finite corner.  cond = sum |N_t| / |sum N_t|
    (1 where the normal is 0): what the f64 summation's own rounding is amplified by."""
    V = verts.astype(np.float64)
    nv = len(V)
    with np.errstate(invalid="ignore", over="ignore"):
        N = np.cross(V[faces[:, 1]] - V[faces[:, 0]], V[faces[:, 2]] - V[faces[:, 0]]) if len(faces) else np.zeros((0, 3))
        s = np.zeros((nv, 3)); a = np.zeros(nv)
        for t, f in enumerate(faces):
            for i in set(int(x) for x in f):
                s[i] += N[t]; a[i] += np.linalg.norm(N[t])
        l = np.linalg.norm(s, axis=1)
        ok = np.isfinite(l) & (l > 0)
        n = np.where(ok[:, None], s / np.where(ok, l, 1.0)[:, None], 0.0)
        cond = np.where(ok, a / np.where(ok, l, 1.0), 1.0)
    return n, cond


# ---- the self-penetration term ---------------------------------------------------------------------------------------------------
def self_penetration64(verts, faces, trunc=None, min_cos=0.0):
    """The term of one frame in f64: the vertices with w_i > 1 (their own faces left out), each matched by the oriented brute force
    with direction -n_i, the cost sum rho(dist2), and its gradient [V, 3] at the returned correspondence (on the gathered rows and
    on the matched faces' corners, both `verts`).  Returns a dict: winding, inside, rows (the vertex ids), dist2, index, bary,
    value, grad."""
    nv = len(verts)
    ids = np.arange(nv)
    w = winding64(verts, verts, faces, skip=ids)
    inside = w > 1.0
    rows = np.flatnonzero(inside)
    n, _ = vertex_normals64(verts, faces)
    q = np.ascontiguousarray(verts[rows])
    m = (-n[rows]).astype(np.float32)
    d2, idx, bary = orf.brute_force_oriented(q, m, verts, faces, min_cos)
    hit = idx >= 0
    live = hit if trunc is None else hit & (d2 < trunc * trunc)
    cost = np.where(hit, d2 if trunc is None else np.minimum(d2, trunc * trunc), 0.0)
    gq, gv = sr.vjp(q, verts, faces, np.where(live, idx, -1), bary, np.ones(len(rows)))[:2]
    grad = gv.copy()
    np.add.at(grad, rows, gq)
    return dict(winding=w, inside=inside, rows=rows, dist2=d2, index=idx, bary=bary, value=float(cost.sum()), grad=grad)
