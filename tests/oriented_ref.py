"""Test infrastructure (numpy): the references of the ORIENTED closest-surface search (bodyfit_closest_surface_oriented_device), on top
of tests/surface_ref.py: the f64 face normals and the has-area rule of the prepared record; the f64 brute force over the
normal-compatible faces; check_oriented, which asserts the sandwich contract of include/bodyfit.h for EVERY query of a frame;
an f32 restatement of the kernel's gate (the cross product and the dot with the kernel's fused steps) in front of surface_ref's
f32 evaluation; and the scenes the CPU and the GPU tests share.

A frame is (q [nq, 3] f32, m [nq, 3] f32 directions, verts [V, 3] f32, faces [nf, 3] int).  min_cos is an f32 value (what the C
function receives): every function here rounds it to f32 first."""
import numpy as np

import surface_ref as sr

U, K = sr.U, sr.K
K_N = 16            # the derived constant of the gate, include/bodyfit.h (bodyfit_closest_surface_oriented_device)


# ---- f64 reference -----------------------------------------------------------------------------------------------------
def face_normals64(verts, faces):
    """(n [nf, 3] f64, area [nf] bool): the unit normal of every face in the orientation of `faces`, (v1 - v0) x (v2 - v0)
    normalised, and whether the face has an area by the rule of k_cs_prepare: longest edge L >= 1e-30 as f32, height over it above
    2^-40 L and >= 1e-30 as f32, finite corners.  Formed as the record is, u x w with u along the longest edge and w the unit
    vector of the third corner's offset from it (the corner rotation is cyclic, so the orientation is kept): for a sliver this
    keeps the digits that normalising the raw cross product would lose.  Zeros where there is no area."""
    v = verts.astype(np.float64)[faces]                              # [nf, 3, 3]
    nf = len(faces)
    if nf == 0:
        return np.zeros((0, 3)), np.zeros(0, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = np.stack([((v[:, (i + 1) % 3] - v[:, i]) ** 2).sum(axis=1) for i in range(3)], axis=1)
        ar = np.arange(nf)
        rot = np.zeros(nf, np.int64)
        rot = np.where(l2[:, 1] > l2[ar, rot], 1, rot)
        rot = np.where(l2[:, 2] > l2[ar, rot], 2, rot)
        A, B, C = v[ar, rot], v[ar, (rot + 1) % 3], v[ar, (rot + 2) % 3]
        L = np.sqrt(l2[ar, rot])
        finite = np.isfinite(v).all(axis=(1, 2))
        live = finite & (L.astype(np.float32) >= np.float32(1e-30))
        u = (B - A) / np.where(live, L, 1.0)[:, None]
        e2 = C - A
        pr = e2 - sr._dot(e2, u)[:, None] * u
        th = np.sqrt(sr._dot(pr, pr))
        area = live & (th > L * 2.0 ** -40) & (th.astype(np.float32) >= np.float32(1e-30))
        w = pr / np.where(area, th, 1.0)[:, None]
        n = np.where(area[:, None], np.cross(u, w), 0.0)
    return n, area


def pair_distances64(q, verts, faces):
    """D [nq, nf] f64: the exact squared distance of every query to every face (surface_ref.tri_closest64, chunked)"""
    nq, nf = q.shape[0], faces.shape[0]
    D = np.empty((nq, nf))
    if nq == 0 or nf == 0:
        return D
    V = verts.astype(np.float64)
    v0, v1, v2 = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    for s in range(0, nq, sr.CHUNK):
        P = q[s:s + sr.CHUNK].astype(np.float64)
        D[s:s + sr.CHUNK], _ = sr.tri_closest64(P[:, None, :], v0[None], v1[None], v2[None])
    return D


def compatible64(m, verts, faces, min_cos, slack):
    """[nq, nf] bool: face t has an area and n_t . m_i >= min_cos + slack_i, in f64 (false wherever a NaN is involved)"""
    n, area = face_normals64(verts, faces)
    mc = float(np.float32(min_cos))
    with np.errstate(invalid="ignore"):
        s = m.astype(np.float64) @ n.T
        return area[None] & (s >= mc + np.broadcast_to(np.asarray(slack, np.float64), (len(m),))[:, None])


def brute_force_oriented(q, m, verts, faces, min_cos, slack=0.0, D=None):
    """surface_ref.brute_force over the faces with an area and n . m >= min_cos + slack (slack: a number or [nq]):
    (d*^2 [nq] f64, argmin [nq], bary [nq, 3] f64); (+inf, -1, 0) for a query no face qualifies for.  D: pair_distances64 of
    the frame if the caller has it."""
    nq, nf = q.shape[0], faces.shape[0]
    dmin, amin, bary = np.full(nq, np.inf), np.full(nq, -1, np.int64), np.zeros((nq, 3))
    if nq == 0 or nf == 0:
        return dmin, amin, bary
    ok = compatible64(m, verts, faces, min_cos, slack)
    D = np.where(ok, pair_distances64(q, verts, faces) if D is None else D, np.inf)
    a = D.argmin(axis=1)
    has = ok.any(axis=1)
    V = verts.astype(np.float64)
    d, b = sr.tri_closest64(q.astype(np.float64), V[faces[a, 0]], V[faces[a, 1]], V[faces[a, 2]])
    dmin[has] = d[has]; amin[has] = a[has]; bary[has] = b[has]
    return dmin, amin, bary


def tau_of(m):
    """tau_i = k_n u |m_i|"""
    with np.errstate(invalid="ignore", over="ignore"):
        return K_N * U * np.sqrt((m.astype(np.float64) ** 2).sum(axis=1))


# ---- the contract --------------------------------------------------------------------------------------------------------
def check_oriented(q, m, verts, faces, min_cos, dist2, index, bary, D=None):
    """Asserts the sandwich contract of include/bodyfit.h (bodyfit_closest_surface_oriented_device) for EVERY query of one
    frame (finite q and verts; m may hold NaN, then the query must get nothing).  With tau_i = k_n u |m_i|:
      (1) the returned face is in the loose set (an area and n . m >= min_cos - tau), or index = -1 with dist2 = +inf, bary = 0;
      (2) a non-empty strict set (n . m >= min_cos + tau): index != -1 and d^ <= d*_strict + k u (d*_strict + h);
      (3) an empty loose set: index = -1;
      (4) b >= 0, sum b = 1 exactly, |sqrt(dist2) - d^| <= k u (d^ + h)      (surface_ref.check_bounds' forms).
    Returns (worst optimality excess, worst consistency error) in units of u (d + h), and the number of hits."""
    nq, nf = q.shape[0], faces.shape[0]
    index = np.asarray(index).astype(np.int64)
    dist2, bary = np.asarray(dist2), np.asarray(bary)
    assert index.shape == (nq,) and dist2.shape == (nq,) and bary.shape == (nq, 3)
    if nq == 0:
        return 0.0, 0.0, 0
    hit = index >= 0
    assert np.all(index[~hit] == -1) and np.all(index < max(nf, 1)), "index out of the frame's range"
    assert np.all(np.isposinf(dist2[~hit])) and np.all(bary[~hit] == 0), "a query without a candidate: -1, +inf, 0"
    if nf == 0:
        assert not hit.any()
        return 0.0, 0.0, 0
    tau = tau_of(m)
    loose = compatible64(m, verts, faces, min_cos, -tau)
    strict = compatible64(m, verts, faces, min_cos, tau)
    rows = np.flatnonzero(hit)
    bad = ~loose[rows, index[rows]]
    assert not bad.any(), ("(1) a returned face outside the loose set", int(bad.sum()), rows[bad][:5].tolist())
    bad = hit & ~loose.any(axis=1)
    assert not bad.any(), ("(3) a hit with an empty loose set", int(bad.sum()))
    must = strict.any(axis=1)
    bad = must & ~hit
    assert not bad.any(), ("(2) no hit with a non-empty strict set", int(bad.sum()), np.flatnonzero(bad)[:5].tolist())
    if not hit.any():
        return 0.0, 0.0, 0
    qh, ih, bh = q[hit], index[hit], bary[hit]
    assert bary.dtype == np.float32 and np.all(bh >= 0), "negative weight"
    assert np.all(bh.astype(np.float64).sum(axis=1) == 1.0), "the weights must sum to 1 exactly"
    c = sr.point_at(verts, faces, ih, bh)
    dhat = np.sqrt(((qh.astype(np.float64) - c) ** 2).sum(axis=1))
    h = sr.longest_edge(verts, faces, ih)
    con = np.abs(np.sqrt(dist2[hit].astype(np.float64)) - dhat) / (U * (dhat + h) + 1e-300)
    bad = con > K
    assert not bad.any(), ("(4) consistency", int(bad.sum()), float(con.max()))
    dstar = np.sqrt(brute_force_oriented(q, m, verts, faces, min_cos, tau, D=D)[0])[hit]      # +inf where strict is empty
    with np.errstate(invalid="ignore"):
        opt = np.where(must[hit], (dhat - dstar) / (U * (dstar + h) + 1e-300), -np.inf)
    bad = opt > K
    assert not bad.any(), ("(2) optimality against the strict set", int(bad.sum()), float(opt.max()))
    return float(opt.max()), float(con.max()), int(hit.sum())


# ---- the kernel's gate, in f32 ---------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fma(a, b, c) of f32 arrays: the product of two f32 is exact in f64, the sum is rounded to f64 and then to f32 (a double
    rounding, which differs from the fused result by at most 2^-29 of an f32 ulp's worth of cases: the error bound is the same)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gate_f32(m, R, min_cos):
    """[nq, nf] bool, the gate of k_cs_search<true> on the prepared records R (surface_ref.prepare_records): n = u x w per
    component as fma(a, b, -(c d)), s = fma(nz, mz, fma(ny, my, nx mx)), candidate iff t > 0 and s >= min_cos"""
    u, w = R["u"], R["w"]
    nx = _fma32(u[:, 1], w[:, 2], -(u[:, 2] * w[:, 1]))
    ny = _fma32(u[:, 2], w[:, 0], -(u[:, 0] * w[:, 2]))
    nz = _fma32(u[:, 0], w[:, 1], -(u[:, 1] * w[:, 0]))
    assert nx.dtype == np.float32
    m = m.astype(np.float32)
    mx, my, mz = m[:, 0:1], m[:, 1:2], m[:, 2:3]
    with np.errstate(invalid="ignore", over="ignore"):
        s = _fma32(nz[None], mz, _fma32(ny[None], my, nx[None] * mx))
        return (R["t"] > 0)[None] & R["finite"][None] & (s >= np.float32(min_cos))


def kernel_form_oriented_f32(q, m, verts, faces, min_cos):
    """(dist2 [nq] f32, index [nq], bary [nq, 3] f32) of the oriented kernel's form: the f32 gate, then surface_ref's f32
    evaluation of every admitted pair (no cull), the lowest index among equal computed distances, and the winner's weights by
    surface_ref.kernel_form_f32 on that face alone"""
    nq, nf = q.shape[0], faces.shape[0]
    d2 = np.full(nq, np.inf, np.float32); idx = np.full(nq, -1, np.int64); bary = np.zeros((nq, 3), np.float32)
    if nq == 0 or nf == 0:
        return d2, idx, bary
    R = sr.prepare_records(verts, faces)
    ok = gate_f32(m, R, min_cos)
    q = q.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, nq, sr.CHUNK):
            P = q[s:s + sr.CHUNK]
            D, _, _ = sr._eval_f32(P[:, None, :] - R["A"][None], {k: (v[None] if k != "rot" else v) for k, v in R.items()})
            D = np.where(ok[s:s + sr.CHUNK] & np.isfinite(D), D, np.inf)
            a = D.argmin(axis=1)
            idx[s:s + sr.CHUNK] = np.where(np.isfinite(D[np.arange(len(a)), a]), a, -1)
    for t in np.unique(idx[idx >= 0]):
        sel = np.flatnonzero(idx == t)
        d2[sel], one, bary[sel] = sr.kernel_form_f32(q[sel], verts, faces[t:t + 1])
        assert np.all(one == 0)
    return d2, idx, bary


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def directions(rng, verts, faces, source, max_deg=30.0):
    """[n, 3] f32 unit directions: the first half of the rows get the normal of their source face rotated by up to max_deg about
    a random axis in the face's plane, the other half (and any row whose source face has no area) a uniformly random unit vector"""
    n = len(source)
    m = _unit(rng.normal(size=(n, 3)))
    if len(faces):
        nrm, area = face_normals64(verts, faces)
        k = n // 2
        src = np.asarray(source[:k])
        side = np.cross(nrm[src], _unit(rng.normal(size=(k, 3))))
        good = area[src] & (np.linalg.norm(side, axis=1) > 1e-3)
        ang = np.deg2rad(rng.uniform(0.0, max_deg, k))[:, None]
        rot = np.cos(ang) * nrm[src] + np.sin(ang) * _unit(np.where(good[:, None], side, 1.0))
        m[:k] = np.where(good[:, None], rot, m[:k])
    return m.astype(np.float32)


def oriented_scene(synth, seed, V=1000, n_faces=2000, n_query=600, on_surface=0.3):
    """surface_ref.mesh_scene with a direction per query: (q, m, verts, faces).  The source face of a query is the face
    mesh_scene sampled it on, recovered by replaying its generator (and checked: the replay reproduces the queries)."""
    q, verts, faces = sr.mesh_scene(synth, seed, V=V, n_faces=n_faces, n_query=n_query, on_surface=on_surface)
    assert np.array_equal(sr.surface_queries(np.random.default_rng(seed), verts, faces, n_query, on_surface), q)
    source = np.random.default_rng(seed).integers(0, len(faces), n_query)
    m = directions(np.random.default_rng(1000 + seed), verts, faces, source)
    return q, m, verts, faces


# (seed, V, n_faces, n_query) of the scenes the GPU tests run: the 2000-face scene and the face counts off the 256-record tile
MAIN = (0, 1000, 2000, 600)
OFF_TILE = {1: (3, 1000, 1, 300), 33: (2, 1000, 33, 300), 257: (1, 1000, 257, 300)}
MIN_COS = (-2.0, 0.0, 0.5, 2.0)


def threshold_case():
    """One triangle whose record is exact in f32: corners (0,0,3), (2,0,3), (1,1,3), the longest edge along x, so u = (1,0,0),
    w = (0,1,0) and n = u x w = (0,0,1) without any rounding; m = (0.6, 0, 0.8) as f32.  Then every step of the gate is exact and
    s = m_z = float32(0.8) bit for bit.  Returns (q, m, verts, faces, [below, on, above]): min_cos = float32(0.8) and its two
    f32 neighbours.  On the threshold the contract accepts either outcome; one neighbour below the exact comparison admits the
    face, one above it rejects it (both lie inside tau, so the contract alone would not fix them: the construction does)."""
    verts = np.array([[0, 0, 3], [2, 0, 3], [1, 1, 3]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    q = np.array([[1.0, 0.25, 2.5]], np.float32)
    m = np.array([[0.6, 0.0, 0.8]], np.float32)
    on = np.float32(0.8)
    return q, m, verts, faces, [np.nextafter(on, np.float32(-1)), on, np.nextafter(on, np.float32(2))]


def two_sheets(n=64, seed=0):
    """Two parallel square sheets of 0.2 m, two triangles each: the front one at z = 3.000 with normal -z (vertices 0..3), the
    back one at z = 3.010 with normal +z (vertices 4..7); n points at z = 3.004 over the sheets' interior with direction +z.
    By distance alone a point matches the front sheet (4 mm); with its direction only the back sheet (6 mm) is compatible."""
    xy = np.array([[0.0, 0.0], [0.2, 0.0], [0.2, 0.2], [0.0, 0.2]])
    verts = np.concatenate([np.c_[xy, np.full(4, 3.000)], np.c_[xy, np.full(4, 3.010)]]).astype(np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7]], np.int32)
    rng = np.random.default_rng(seed)
    q = np.c_[rng.uniform(0.02, 0.18, (n, 2)), np.full(n, 3.004)].astype(np.float32)
    m = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (n, 1))
    return q, m, verts, faces
