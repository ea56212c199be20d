"""The definition of bodyfit_volume_surface_* (include/bodyfit.h, SURFACE EXTRACTION) restated in numpy: usability, cells, welded
vertices in numpy.longdouble, faces from the table of tools/gen_mc_table.py; the position bound of the contract; the census of
directed edges that says whether a mesh is a closed oriented manifold; and the volumes that test_extract.py (CPU) and
test_gpu_extract.py share."""
import importlib.util
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

N_TRI, TRI = gen.table()
N_TRI = N_TRI.astype(np.int64)
LOW = np.array([gen.edge_corners(e)[0] for e in range(12)], np.int64)          # the corner of a cell that owns its edge e
# SHARED[e1][e2]: the cube face 2 axis + value that holds both edges, -1: none (e1 == e2: -1)
SHARED = np.full((12, 12), -1, np.int64)
for _a in range(12):
    for _b in range(12):
        _both = gen.edge_faces(_a) & gen.edge_faces(_b)
        if _a != _b and _both:
            (_axis, _value), = _both
            SHARED[_a, _b] = 2 * _axis + _value

U = 2.0 ** -24
LD = np.longdouble


def _next(a, axis, fill):
    """a's neighbour towards + on `axis` (0: x) of an array [nz, ny, nx]; `fill` behind the last index"""
    out = np.full_like(a, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[2 - axis] = slice(1, None)
    dst[2 - axis] = slice(0, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def extract(vol, origin, spacing, iso=0.0, weight=None, min_weight=0.0):
    """One volume [nz, ny, nx].  A namespace with verts (longdouble [Nv, 3], the definition's exact positions up to longdouble's own
    rounding), vert_axis [Nv], vert_index [Nv, 3] (i, j, k of the owner), faces (int32 [Nf, 3]), face_cell [Nf] (the linear index of
    the cell's corner 0), face_edges [Nf, 3] (the cube edges of the corners), live [nz - 1, ny - 1, nx - 1] and case (alike)."""
    vol = np.ascontiguousarray(vol, np.float32)
    nz, ny, nx = vol.shape
    iso = np.float32(iso)
    usable = np.isfinite(vol)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            usable &= np.asarray(weight, np.float32) >= np.float32(min_weight)
    with np.errstate(invalid="ignore"):
        inside = vol < iso
    out = types.SimpleNamespace(verts=np.zeros((0, 3), LD), vert_axis=np.zeros(0, np.int64), vert_index=np.zeros((0, 3), np.int64),
                                faces=np.zeros((0, 3), np.int32), face_cell=np.zeros(0, np.int64),
                                face_edges=np.zeros((0, 3), np.int64), live=np.zeros((max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)), bool))
    out.case = np.zeros(out.live.shape, np.int64)
    if min(nx, ny, nz) < 2:
        return out
    live = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros(live.shape, np.int64)
    for c in range(8):
        sl = (slice(c >> 2 & 1, nz - 1 + (c >> 2 & 1)), slice(c >> 1 & 1, ny - 1 + (c >> 1 & 1)), slice(c & 1, nx - 1 + (c & 1)))
        live &= usable[sl]
        case |= inside[sl].astype(np.int64) << c
    out.live, out.case = live, case
    # the cells around an edge: L[1 - dk:, 1 - dj:, 1 - di:] is the liveness of cell (k - dk, j - dj, i - di) at every voxel
    L = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    L[1:nz, 1:ny, 1:nx] = live

    def cell(dk, dj, di):
        return L[1 - dk:1 - dk + nz, 1 - dj:1 - dj + ny, 1 - di:1 - di + nx]

    around = [cell(0, 0, 0) | cell(0, 1, 0) | cell(1, 0, 0) | cell(1, 1, 0),
              cell(0, 0, 0) | cell(0, 0, 1) | cell(1, 0, 0) | cell(1, 0, 1),
              cell(0, 0, 0) | cell(0, 0, 1) | cell(0, 1, 0) | cell(0, 1, 1)]
    flag = np.zeros((nz, ny, nx, 3), bool)
    for axis in range(3):
        flag[..., axis] = usable & _next(usable, axis, False) & (inside ^ _next(inside, axis, False)) & around[axis]
    flat = flag.reshape(-1)
    vid = np.cumsum(flat) - 1                                                    # of a flagged (voxel, axis)
    at = np.nonzero(flat)[0]
    owner, axis = at // 3, at % 3
    idx = np.stack([owner % nx, owner // nx % ny, owner // (nx * ny)], axis=-1)
    o, s = np.asarray(origin, np.float64).astype(LD), np.broadcast_to(np.asarray(spacing, np.float64), (3,)).astype(LD)
    verts = o[None, :] + idx.astype(LD) * s[None, :]
    va = vol.reshape(-1)[owner].astype(LD)
    vb = vol.reshape(-1)[owner + np.array([1, nx, nx * ny])[axis]].astype(LD)
    t = (LD(iso) - va) / (vb - va)
    assert bool(((t >= 0) & (t <= 1)).all())
    rows = np.arange(at.shape[0])
    verts[rows, axis] = o[axis] + (idx[rows, axis].astype(LD) + t) * s[axis]
    out.verts, out.vert_axis, out.vert_index = verts, axis, idx
    # faces
    code = np.zeros((nz, ny, nx), np.int64)
    code[:nz - 1, :ny - 1, :nx - 1] = np.where(live, case, 0)
    code = code.reshape(-1)
    cells = np.nonzero(N_TRI[code])[0]
    nt = N_TRI[code[cells]]
    start = np.cumsum(nt) - nt
    n_faces = int(nt.sum())
    faces = np.zeros((n_faces, 3), np.int64)
    face_edges = np.zeros((n_faces, 3), np.int64)
    face_cell = np.zeros(n_faces, np.int64)
    for k in range(gen.MAX_TRI):
        m = nt > k
        cs = cells[m]
        face_cell[start[m] + k] = cs
        for c in range(3):
            e = TRI[code[cs], 3 * k + c].astype(np.int64)
            low = LOW[e]
            own = cs + (low & 1) + (low >> 1 & 1) * nx + (low >> 2 & 1) * nx * ny
            assert bool(flat[3 * own + e // 4].all())                            # every corner is a vertex that exists
            faces[start[m] + k, c] = vid[3 * own + e // 4]
            face_edges[start[m] + k, c] = e
    assert n_faces == 0 or np.unique(faces).shape[0] == at.shape[0]              # no vertex is unreferenced
    out.faces, out.face_cell, out.face_edges = faces.astype(np.int32), face_cell, face_edges
    return out


def position_bound(ref, origin, spacing):
    """the contract's bound on |x^ - x*| at every coordinate of every vertex of `ref`: [Nv, 3] longdouble"""
    o, s = np.abs(np.asarray(origin, np.float64)).astype(LD), np.broadcast_to(np.asarray(spacing, np.float64), (3,)).astype(LD)
    idx = ref.vert_index.astype(LD)
    bound = LD(U) * np.abs(ref.verts) + LD(2.0 ** -51) * (o[None, :] + idx * s[None, :])
    rows = np.arange(ref.verts.shape[0])
    a = ref.vert_axis
    bound[rows, a] = (LD(U) * np.abs(ref.verts[rows, a]) + LD(2.0 ** -50) * (o[a] + (idx[rows, a] + 1) * s[a]) + LD(2.0 ** -149))
    return bound


def edge_census(faces, n_verts):
    """(unmatched [Nf, 3] bool: the directed edge corner c -> c + 1 has no reverse; n_repeated: directed edges used more than once)"""
    f = np.asarray(faces, np.int64)
    key = f * max(n_verts, 1) + np.roll(f, -1, axis=1)
    rev = np.roll(f, -1, axis=1) * max(n_verts, 1) + f
    _, counts = np.unique(key, return_counts=True)
    return ~np.isin(rev, key), int((counts > 1).sum())


def open_edges_are_explained(ref, dims):
    """every directed edge of ref's mesh occurs once, and one without its reverse lies in a face of its cell beyond which there is no
    live cell (the volume's border or a dead cell): (ok, the number of such open edges)"""
    nx, ny, nz = dims
    unmatched, repeated = edge_census(ref.faces, ref.verts.shape[0])
    if repeated:
        return False, 0
    f, c = np.nonzero(unmatched)
    side = SHARED[ref.face_edges[f, c], ref.face_edges[f, (c + 1) % 3]]
    if (side < 0).any():
        return False, 0                                                          # an open edge inside a cell
    cell = ref.face_cell[f]
    ijk = np.stack([cell % nx, cell // nx % ny, cell // (nx * ny)], axis=-1)
    axis, value = side // 2, side % 2
    ijk[np.arange(f.shape[0]), axis] += 2 * value - 1
    lim = np.array([nx - 1, ny - 1, nz - 1])
    exists = ((ijk >= 0) & (ijk < lim)).all(axis=1)
    i, j, k = (ijk[exists, a] for a in range(3))
    return not bool(ref.live[k, j, i].any()), int(f.shape[0])


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ni,ni->", v[:, 0], np.cross(v[:, 1], v[:, 2])) / 6.0)


# ---- the shared volumes ----------------------------------------------------------------------------------------------------------------
DIMS = [(2, 2, 2), (5, 4, 3), (33, 17, 9), (48, 48, 33), (7, 1, 5), (1, 1, 1)]           # (nx, ny, nz)
KINDS = ["normal", "sphere", "dyadic", "iso", "holes", "weights", "far"]
ORIGIN, SPACING = (-0.4, 0.1, 0.25), (0.02, 0.025, 0.03)


def make_volume(kind, dims, seed=0):
    """a namespace: vol [nz, ny, nx] f32, origin, spacing, iso, weight (or None), min_weight"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed + 7919 * KINDS.index(kind) + nx + 100 * ny + 10000 * nz)
    v = types.SimpleNamespace(dims=dims, origin=ORIGIN, spacing=SPACING, iso=0.0, weight=None, min_weight=0.0)
    v.vol = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if kind == "sphere":
        # (a radius that lets the sphere through the border of the flatter grids and keeps it inside 48 x 48 x 33)
        centre = np.array([(nx - 1) / 2 + 0.13, (ny - 1) / 2 - 0.21, (nz - 1) / 2 + 0.37])
        v.vol = (np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - 0.31 * max(min(nx, 48), 2)).astype(np.float32)
    elif kind == "dyadic":
        # multiples of 1/4 in [-1, 1]: many values equal iso = 0, some of them -0.0
        v.vol = (rng.integers(-4, 5, (nz, ny, nx)) / 4.0).astype(np.float32)
        v.vol[(v.vol == 0) & (rng.random((nz, ny, nx)) < 0.5)] = -0.0
        v.origin, v.spacing = (-1.0, 0.5, 2.0), (0.25, 0.5, 0.125)
    elif kind == "iso":
        v.iso = 0.3
        v.vol[rng.random((nz, ny, nx)) < 0.1] = np.float32(0.3)
    elif kind == "holes":
        bad = rng.random((nz, ny, nx)) < 0.04
        v.vol[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        v.vol[0, 0, 0] = np.nan
        v.vol[-1, -1, -1] = -np.inf
        v.vol[nz // 2, 0, nx // 2] = np.inf
    elif kind == "weights":
        v.weight = rng.integers(0, 6, (nz, ny, nx)).astype(np.float32)
        v.weight[rng.random((nz, ny, nx)) < 0.03] = np.nan
        v.weight[0, 0, -1] = np.nan
        v.min_weight = 1.0
    elif kind == "far":
        # a large origin that the grid cancels near the middle index in x: there the f64 term of the bound is what is left
        v.origin, v.spacing = (-77.16049 * (nx // 2), 987.654321, -3.0e5), (77.16049, 1.7, 1.0 / 3.0)
    return v


def padded_random(dims, seed):
    """a standard-normal volume with a layer of outside (positive) voxels around it: its surface is closed"""
    nx, ny, nz = dims
    vol = np.random.default_rng(seed).standard_normal((nz, ny, nx)).astype(np.float32)
    for a in range(3):
        sl = [slice(None)] * 3
        for end in (0, -1):
            sl[a] = end
            vol[tuple(sl)] = 1.0
    return vol
