"""Test infrastructure (numpy): the reference statement of the volume distance transform with the nearest seed
(bodyfit_volume_distance_device, include/bodyfit.h; csrc/k_edt3.hip), the named masks the CPU and the GPU tests share, a
plain-Python restatement of the z pass the kernel runs, and numpy restatements of torch_layer.volume.esdf / occupancy_sdf.

brute(mask) is the DEFINITION: the minimum over all (voxel, seed) pairs in int64.  separable(mask) is the exact per-axis minimum
in int64, for shapes where all pairs are too many: min over i', then j', then k' of the squared offsets, which is the same
minimum because the three squares add.  kernel_form(mask) follows the kernels step by step: edt_ref.kernel_form on every slice,
then Meijster's two scans along z with g = the slice's 2-D dist2, g carried in the stack entry and the 2-D results read-only."""
import numpy as np

import edt_ref

INT32_MAX = 2 ** 31 - 1


def brute(mask):
    """dist2 int64 [nz, ny, nx] of a bool mask (True: a seed) by all pairs, chunked over the voxels; INT32_MAX without a seed"""
    mask = np.asarray(mask, bool)
    shape = mask.shape
    seeds = np.stack(np.nonzero(mask), axis=1).astype(np.int64)
    if len(seeds) == 0:
        return np.full(shape, INT32_MAX, np.int64)
    # |p - s|^2 = |p|^2 + (|s|^2 - 2 p . s) for every pair, the products as one matrix product in f64: every term is an integer
    # below 2^53, so f64 holds it exactly and the result is the int64 one
    vox = np.stack(np.unravel_index(np.arange(mask.size, dtype=np.int64), shape), axis=1).astype(np.float64)
    s = seeds.astype(np.float64)
    s_norm = (s * s).sum(axis=1)[None, :]
    s_twice = np.ascontiguousarray(-2.0 * s.T)
    out = np.empty(mask.size, np.float64)
    chunk = max(1, (1 << 22) // len(seeds))
    for a in range(0, mask.size, chunk):
        d = vox[a:a + chunk] @ s_twice
        d += s_norm
        out[a:a + chunk] = d.min(axis=1)
    out += (vox * vox).sum(axis=1)
    return out.astype(np.int64).reshape(shape)


def separable(mask):
    """dist2 int64 [nz, ny, nx]: the exact minimum axis after axis, each by all offsets of that axis"""
    mask = np.asarray(mask, bool)
    if not mask.any():
        return np.full(mask.shape, INT32_MAX, np.int64)
    big = np.int64(1) << 40
    d = np.where(mask, np.int64(0), big)
    for axis in (2, 1, 0):
        n = mask.shape[axis]
        at = np.arange(n, dtype=np.int64).reshape([n if a == axis else 1 for a in range(3)])
        out = np.full(mask.shape, big, np.int64)
        for s in range(n):
            np.minimum(out, np.take(d, [s], axis=axis) + (at - s) ** 2, out=out)
        d = out
    assert d.max() < big
    return d


def depth_pass(d2, n2):
    """k_edt_depth: (dist2, nearest) int64 [nz, ny, nx] from the slices' 2-D results (d2 INT32_MAX in a slice without a seed)"""
    nz, ny, nx = d2.shape
    plane = ny * nx
    dist2 = np.full(d2.shape, INT32_MAX, np.int64)
    nearest = np.full(d2.shape, -1, np.int64)
    g_all = d2.reshape(nz, plane)
    n_all = n2.reshape(nz, plane)
    dist2_flat, nearest_flat = dist2.reshape(nz, plane), nearest.reshape(nz, plane)
    for c in range(plane):
        col = g_all[:, c].tolist()
        stack = []                                        # (slice s, first slice t of its reign, g_s)
        for u in range(nz):
            g = col[u]
            if g == INT32_MAX:
                continue
            while stack:
                s, t, tg = stack[-1]
                if (t - s) * (t - s) + tg <= (t - u) * (t - u) + g:
                    break
                stack.pop()
            w = 0
            if stack:
                s, _, tg = stack[-1]
                w = 1 + (u * u - s * s + g - tg) // (2 * (u - s))          # Python's // is the floor
                if w >= nz:
                    continue
            stack.append((u, w, g))
        if not stack:
            continue
        for u in range(nz - 1, -1, -1):
            s, t, g = stack[-1]
            dist2_flat[u, c] = (u - s) * (u - s) + g
            nearest_flat[u, c] = s * plane + n_all[s, c]
            if u == t:
                stack.pop()
    return dist2, nearest


def kernel_form(mask):
    """(dist2, nearest) int64 [nz, ny, nx] as k_edt.hip over the slices and k_edt3.hip along z compute them"""
    mask = np.asarray(mask, bool)
    d2 = np.empty(mask.shape, np.int64)
    n2 = np.empty(mask.shape, np.int64)
    for k in range(mask.shape[0]):
        d2[k], n2[k] = edt_ref.kernel_form(mask[k])
    return depth_pass(d2, n2)


def check(mask, dist2, nearest, want=None):
    """asserts the contract for one volume: dist2 is the definition at every voxel (want: brute(mask), computed here when None),
    nearest (None: not checked) an in-volume seed at exactly that squared distance, or INT32_MAX / -1 without a seed"""
    mask = np.asarray(mask, bool)
    dist2 = np.asarray(dist2).astype(np.int64)
    assert dist2.shape == mask.shape
    if want is None:
        want = brute(mask)
    assert np.array_equal(dist2, want), f"{int((dist2 != want).sum())} of {mask.size} voxels differ from the definition"
    if nearest is None:
        return
    nearest = np.asarray(nearest).astype(np.int64)
    assert nearest.shape == mask.shape
    if not mask.any():
        assert np.all(nearest == -1) and np.all(dist2 == INT32_MAX)
        return
    assert nearest.min() >= 0 and nearest.max() < mask.size
    nk, nj, ni = np.unravel_index(nearest, mask.shape)
    assert np.all(mask[nk, nj, ni]), "nearest names a voxel that is not a seed"
    pk, pj, pi = np.indices(mask.shape)
    assert np.array_equal((pk - nk) ** 2 + (pj - nj) ** 2 + (pi - ni) ** 2, dist2), "nearest is not at the squared distance dist2"
    own = np.arange(mask.size).reshape(mask.shape)
    assert np.array_equal(nearest[mask], own[mask]), "a seed's nearest is not itself"


# (nz, ny, nx): the smallest shapes that cross a 64-column ballot word, the eight-ahead unroll and its tail, and a stack deep enough
# for repeated pops and the four-at-a-time read-back
SHAPES = [(1, 1, 1), (1, 1, 67), (1, 67, 1), (67, 1, 1), (9, 13, 67), (70, 3, 5), (3, 70, 130), (64, 64, 130)]
LARGE = (64, 64, 130)                       # all pairs are too many here: separable() is the reference
KINDS = ["empty", "full", "corners", "tie", "checkerboard", "random_0.5", "random_0.002", "shell"]


def make_mask(kind, shape, seed=0):
    nz, ny, nx = shape
    m = np.zeros(shape, bool)
    k, j, i = np.indices(shape)
    if kind == "empty":
        pass
    elif kind == "full":
        m[:] = True
    elif kind == "corners":
        m[0, 0, 0] = m[nz - 1, ny - 1, nx - 1] = True
    elif kind == "tie":
        # two seeds equidistant along z from a whole plane of voxels (along x or y where z is too short)
        if nz >= 3:
            m[0, ny // 2, nx // 2] = m[2 * ((nz - 1) // 2), ny // 2, nx // 2] = True
        elif nx >= 3:
            m[nz // 2, ny // 2, 0] = m[nz // 2, ny // 2, 2 * ((nx - 1) // 2)] = True
        elif ny >= 3:
            m[nz // 2, 0, nx // 2] = m[nz // 2, 2 * ((ny - 1) // 2), nx // 2] = True
        else:
            m[0, 0, 0] = True
    elif kind == "checkerboard":
        m = (k + j + i) % 2 == 0
    elif kind.startswith("random_"):
        rng = np.random.default_rng([seed, nz, ny, nx, int(float(kind[7:]) * 1000)])
        m = rng.random(shape) < float(kind[7:])
        if not m.any():                                   # (the sparse one: at least one seed, so most slices are empty)
            m.reshape(-1)[rng.integers(m.size)] = True
    elif kind == "shell":
        r2 = (k - (nz - 1) / 2.0) ** 2 + (j - (ny - 1) / 2.0) ** 2 + (i - (nx - 1) / 2.0) ** 2
        R = min(shape) / 2.0 * 0.8
        m = (r2 <= R * R) & (r2 > (0.7 * R) ** 2)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(m)


_want = {}


def want(kind, shape, invert=False):
    """the definition's answer for a named mask, computed once: brute, or separable at LARGE"""
    key = (kind, tuple(shape), bool(invert))
    if key not in _want:
        mask = make_mask(kind, shape) != invert
        _want[key] = separable(mask) if tuple(shape) == LARGE else brute(mask)
    return _want[key]


# ---- the fields built on the transform ------------------------------------------------------------------------------------------
def crossings(phi, iso, usable):
    """esdf's crossing voxels: usable and phi == iso, or a usable 6-neighbour on the other side of iso (inside: phi < iso)"""
    with np.errstate(invalid="ignore"):
        inside = usable & (phi < iso)
        cross = usable & (phi == iso)
    for axis in range(3):
        n = phi.shape[axis]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        flip = usable[lo] & usable[hi] & (inside[lo] != inside[hi])
        cross[lo] |= flip
        cross[hi] |= flip
    return cross


def esdf(tsdf, spacing, trunc, transform, iso=0.0, weight=None, min_weight=0.0):
    """torch_layer.volume.esdf of one volume [nz, ny, nx] in numpy (f64, rounded once to f32); transform(mask) -> (dist2, nearest)
    is the distance transform to build on: kernel_form, or the device's own"""
    phi = np.asarray(tsdf, np.float32)
    usable = np.isfinite(phi)
    if weight is not None:
        usable &= np.asarray(weight, np.float32) >= np.float32(min_weight)
    D, n = transform(crossings(phi, np.float32(iso), usable))
    _, m = transform(usable)
    if (np.asarray(n) < 0).any():
        return np.full(phi.shape, np.nan, np.float32)
    rel = phi.astype(np.float64).reshape(-1) - float(iso)
    a = float(spacing) * np.sqrt(np.asarray(D, np.float64)) + np.abs(rel[np.asarray(n)])
    with np.errstate(invalid="ignore"):
        out = np.where(rel[np.asarray(m)] < 0.0, -a, a)
        band = usable & (np.abs(rel.reshape(phi.shape)) < float(np.float32(trunc)))
    return np.where(band, rel.reshape(phi.shape), out).astype(np.float32)


def occupancy_sdf(inside, spacing, transform):
    """torch_layer.volume.occupancy_sdf of one volume in numpy"""
    inside = np.asarray(inside, bool)
    to_in, _ = transform(inside)
    to_out, _ = transform(~inside)
    if not inside.any() or inside.all():
        return np.full(inside.shape, np.nan, np.float32)
    d = np.sqrt(np.where(inside, to_out, to_in).astype(np.float64))
    return np.where(inside, -float(spacing) * (d - 0.5), float(spacing) * (d - 0.5)).astype(np.float32)


def plane_tsdf(shape, spacing, normal, offset, trunc, hole=None):
    """A TSDF of the half space normal . p < offset seen from the other side, in closed form, at the voxel centres p = spacing (i,
    j, k): (tsdf f32 [nz, ny, nx], the true signed distance f64).  Positive in front, capped at trunc; NaN where the surface hides
    the voxel (distance < -trunc) and inside `hole` = (k0, k1, j0, j1, i0, i1), a block that no frame has seen."""
    k, j, i = np.indices(shape)
    nrm = np.asarray(normal, np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    true = (nrm[0] * i + nrm[1] * j + nrm[2] * k) * float(spacing) - float(offset)
    tsdf = np.minimum(true, float(trunc))
    tsdf[true < -float(trunc)] = np.nan
    if hole is not None:
        tsdf[hole[0]:hole[1], hole[2]:hole[3], hole[4]:hole[5]] = np.nan
    return tsdf.astype(np.float32), true


def trilinear(vol, origin, spacing, p):
    """(value [N], valid [N], grad [N, 3]) f64 of the volume [nz, ny, nx] at the points p [N, 3]: sample_volume's patch and its
    derivative in world units, dead outside the voxel centres' box or next to a voxel that is not finite"""
    vol = np.asarray(vol, np.float64)
    nz, ny, nx = vol.shape
    g = (np.asarray(p, np.float64) - np.asarray(origin, np.float64)) / float(spacing)
    hi = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    valid = np.all(np.isfinite(g), axis=1) & np.all((g >= 0.0) & (g <= hi), axis=1)
    gs = np.where(valid[:, None], g, 0.0)
    c = np.minimum(np.floor(gs), np.maximum(hi - 1, 0)).astype(np.int64)
    t = gs - c
    V = np.empty((2, 2, 2, len(g)))                        # [dz][dy][dx]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                v = vol[np.minimum(c[:, 2] + dz, nz - 1), np.minimum(c[:, 1] + dy, ny - 1), np.minimum(c[:, 0] + dx, nx - 1)]
                valid &= np.isfinite(v)
                V[dz, dy, dx] = np.where(np.isfinite(v), v, 0.0)
    # (trilinear_inl.h's form: the derivative from the DIFFERENCES of the voxels, exactly 0 in a constant cell)
    w = [[1.0 - t[:, axis], t[:, axis]] for axis in range(3)]
    value = sum(w[2][dz] * w[1][dy] * w[0][dx] * V[dz, dy, dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    grad = np.stack([sum(w[2][dz] * w[1][dy] * (V[dz, dy, 1] - V[dz, dy, 0]) for dz in (0, 1) for dy in (0, 1)),
                     sum(w[2][dz] * w[0][dx] * (V[dz, 1, dx] - V[dz, 0, dx]) for dz in (0, 1) for dx in (0, 1)),
                     sum(w[1][dy] * w[0][dx] * (V[1, dy, dx] - V[0, dy, dx]) for dy in (0, 1) for dx in (0, 1))], axis=1)
    value[~valid] = 0.0
    grad[~valid] = 0.0
    return value, valid, grad / float(spacing)


def sole_descent(value_and_grad, soles, steps, damping=0.5):
    """The fit loop of the tests: the soles [K, 3] under a translation t, cost sum r^2 with r = phi(sole + t); `steps` plain
    gradient steps of length damping / (2 K) (the cost's curvature along a unit gradient of phi is 2 K).  value_and_grad(points)
    -> (phi [K], grad [K, 3]).  The translations visited, [steps + 1, 3], and the first gradient."""
    t = np.zeros(3)
    path, first = [t.copy()], None
    for _ in range(steps):
        r, g = value_and_grad(soles + t)
        grad = 2.0 * (r[:, None] * g).sum(axis=0)
        first = grad if first is None else first
        t = t - damping / (2.0 * len(soles)) * grad
        path.append(t.copy())
    return np.array(path), first
