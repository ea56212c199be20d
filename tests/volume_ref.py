"""The definition of bodyfit_volume_sample_device (include/bodyfit.h) in numpy longdouble, and the check of a result against its
contract (a) liveness, (b) value, (c) gradient: per point, against every candidate cell whose closed support is within delta of
the exact grid coordinates.  Nothing here mirrors the kernel's order of operations: the bounds of the header carry the
difference."""
import itertools
import math

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -24


def bounds(dims):
    """(delta in voxels, c1 = c2 as a multiple of M) of a grid (nx, ny, nz): 2^-50 E and 2^-46 E, E the largest dimension"""
    E = LD(max(dims))
    return LD(2.0) ** -50 * E, LD(2.0) ** -46 * E


def grid_coords(p, origin, spacing):
    """g = (p - origin) / spacing of one f32 point, per axis, in longdouble (origin, spacing: the handle's f64 values)"""
    return (np.asarray(p, np.float32).astype(LD) - np.asarray(origin, np.float64).astype(LD)) / np.asarray(spacing, np.float64).astype(LD)


def exact_cell(g, n):
    """i0 of the header's cell choice on one axis, 0 <= g <= n - 1"""
    return min(int(math.floor(g)), max(n - 2, 0))


def axis_cells(g, n, delta):
    """every i0 whose closed support [i0, min(i0 + 1, n - 1)] is within delta of g"""
    hi = max(n - 2, 0)
    w = 1 if n >= 2 else 0
    f = int(math.floor(g)) if abs(g) < 2.0 ** 40 else 0
    return [i0 for i0 in range(max(0, f - 1), min(hi, f + 1) + 1) if i0 - delta <= g <= i0 + w + delta]


def patch(vol, cell, g):
    """(value, world-unit-free derivative [3] in GRID units, the eight voxels) of the patch of cell = (i0, j0, k0) of vol
    [nz, ny, nx] (longdouble) at g = (gx, gy, gz), which need not lie inside the cell (the patch is a polynomial)"""
    nz, ny, nx = vol.shape
    i0, j0, k0 = cell
    i1, j1, k1 = min(i0 + 1, nx - 1), min(j0 + 1, ny - 1), min(k0 + 1, nz - 1)
    a, b, c = g[0] - i0, g[1] - j0, g[2] - k0
    V = np.array([[[vol[k, j, i] for i in (i0, i1)] for j in (j0, j1)] for k in (k0, k1)], dtype=LD)   # [dk][dj][di]
    wa, wb, wc = (LD(1) - a, a), (LD(1) - b, b), (LD(1) - c, c)
    val = LD(0)
    d = [LD(0), LD(0), LD(0)]
    with np.errstate(invalid="ignore"):                  # (a cell with a voxel that is not finite: the caller looks at V)
        for dk, dj, di in itertools.product((0, 1), repeat=3):
            val += wa[di] * wb[dj] * wc[dk] * V[dk, dj, di]
        for dk, dj in itertools.product((0, 1), repeat=2):
            d[0] += wb[dj] * wc[dk] * (V[dk, dj, 1] - V[dk, dj, 0])
        for dk, di in itertools.product((0, 1), repeat=2):
            d[1] += wa[di] * wc[dk] * (V[dk, 1, di] - V[dk, 0, di])
        for dj, di in itertools.product((0, 1), repeat=2):
            d[2] += wa[di] * wb[dj] * (V[1, dj, di] - V[0, dj, di])
    return val, d, V.reshape(-1)


def sample(vol, origin, spacing, p, gate=1):
    """The DEFINITION at one point: (live, value, grad [3] in world units), exact cell, no band."""
    vol = np.asarray(vol)
    nz, ny, nx = vol.shape
    dead = (False, LD(0), [LD(0)] * 3)
    if not np.all(np.isfinite(np.asarray(p, np.float32))) or not gate:
        return dead
    g = grid_coords(p, origin, spacing)
    if not all(0 <= g[a] <= n - 1 for a, n in enumerate((nx, ny, nz))):
        return dead
    cell = tuple(exact_cell(g[a], n) for a, n in enumerate((nx, ny, nz)))
    val, d, V = patch(vol.astype(LD), cell, g)
    if not np.all(np.isfinite(V)):
        return dead
    s = np.asarray(spacing, np.float64).astype(LD)
    return True, val, [d[a] / s[a] for a in range(3)]


def check_point(vol, origin, spacing, p, gate, got_value, got_valid, got_grad):
    """None if (got_value f32, got_valid, got_grad f32 [3] or None) at point p obeys the contract, else what it breaks."""
    vol = np.asarray(vol)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    delta, c = bounds(dims)
    s = np.asarray(spacing, np.float64).astype(LD)
    got_live = bool(got_valid)
    grad = [0.0, 0.0, 0.0] if got_grad is None else [float(x) for x in got_grad]

    def dead_outputs():
        if float(got_value) != 0.0 or any(x != 0.0 for x in grad):
            return "a dead point with a non-zero output"
        return None

    if not np.all(np.isfinite(np.asarray(p, np.float32))) or not gate:
        return "live, but not finite or gated off" if got_live else dead_outputs()
    g = grid_coords(p, origin, spacing)
    if any(g[a] < -delta or g[a] > n - 1 + delta for a, n in enumerate(dims)):
        return "live more than delta outside the box" if got_live else dead_outputs()
    # (an axis of length 1 has no interior: the one coordinate that is inside, g = 0, is computed exactly)
    deep = all(g[a] == 0 or (n > 1 and delta <= g[a] <= n - 1 - delta) for a, n in enumerate(dims))
    cands = list(itertools.product(*(axis_cells(g[a], n, delta) for a, n in enumerate(dims))))
    volL = vol.astype(LD)
    evals = [(K,) + patch(volL, K, g) for K in cands]
    finite = [bool(np.all(np.isfinite(e[3]))) for e in evals]
    if not got_live:
        if deep and cands and all(finite):
            return "dead, but inside by delta with every candidate cell finite"
        return dead_outputs()
    if not any(finite):
        return "live without a finite candidate cell"
    inside = all(0 <= g[a] <= n - 1 for a, n in enumerate(dims))
    T, M_exact = None, LD(0)
    if inside:
        Tv, _, TV = patch(volL, tuple(exact_cell(g[a], n) for a, n in enumerate(dims)), g)
        if np.all(np.isfinite(TV)):
            T, M_exact = Tv, np.abs(TV).max()
    worst = None
    for (K, val, d, V), fin in zip(evals, finite):
        if not fin:
            continue
        M = max(np.abs(V).max(), M_exact)
        ref = val if T is None else T
        if abs(LD(float(got_value)) - ref) > U * abs(ref) + c * M:
            worst = f"value {float(got_value)!r} against {float(ref)!r} (cell {K})"
            continue
        if got_grad is not None:
            bad = [a for a in range(3) if abs(LD(grad[a]) - d[a] / s[a]) > U * abs(d[a] / s[a]) + c * M / s[a]]
            if bad:
                worst = f"derivative {bad[0]}: {grad[bad[0]]!r} against {float(d[bad[0]] / s[bad[0]])!r} (cell {K})"
                continue
        return None
    return worst
