"""CPU: the reference of the volume sampler (volume_ref.py) checked against facts that do not depend on it: an affine field is
reproduced with its gradient, the derivative is that of the value, the cell choice at the upper face and on short axes, the
rule of the cell with a voxel that is not finite; and the checker accepts the definition and rejects what breaks it."""
import numpy as np
import pytest

import volume_ref as vr

LD = np.longdouble
ORIGIN = (0.25, -0.5, 1.0)
SPACING = (0.03, 0.05, 0.02)


def affine_volume(dims, normal, d, origin=ORIGIN, spacing=SPACING):
    """phi = n . p - d at the voxel centres, [nz, ny, nx] f64 (not rounded to f32: the reference takes any array)"""
    nx, ny, nz = dims
    x = origin[0] + spacing[0] * np.arange(nx)
    y = origin[1] + spacing[1] * np.arange(ny)
    z = origin[2] + spacing[2] * np.arange(nz)
    return normal[0] * x[None, None, :] + normal[1] * y[None, :, None] + normal[2] * z[:, None, None] - d


def inside_points(rng, dims, n, origin=ORIGIN, spacing=SPACING):
    g = rng.uniform(0.0, 1.0, size=(n, 3)) * (np.array(dims) - 1)
    return (np.array(origin) + g * np.array(spacing)).astype(np.float32)


@pytest.mark.parametrize("dims", [(5, 4, 3), (17, 9, 6), (2, 1, 3)])
def test_an_affine_field_is_reproduced_with_its_gradient(dims):
    rng = np.random.default_rng(1)
    n, d = np.array([0.3, -0.8, 0.52]), 0.7
    vol = affine_volume(dims, n, d)
    pts = inside_points(rng, dims, 40)
    if dims[1] == 1:
        pts[:, 1] = ORIGIN[1]
    for p in pts:
        live, val, grad = vr.sample(vol, ORIGIN, SPACING, p)
        assert live
        want = float(np.dot(n, p.astype(np.float64)) - d)
        assert abs(float(val) - want) <= 1e-13
        for a in range(3):
            assert abs(float(grad[a]) - (0.0 if dims[a] == 1 else n[a])) <= 1e-11


def test_the_derivative_is_that_of_the_value():
    rng = np.random.default_rng(2)
    dims = (5, 4, 3)
    vol = rng.normal(size=dims[::-1])
    volL = vol.astype(LD)
    for _ in range(30):
        cell = tuple(int(rng.integers(0, n - 1)) for n in dims)
        g = np.array([c + rng.uniform(0.2, 0.8) for c in cell], dtype=LD)
        _, d, _ = vr.patch(volL, cell, g)
        for a in range(3):
            h = LD(1e-6)
            e = np.zeros(3, LD)
            e[a] = h
            fd = (vr.patch(volL, cell, g + e)[0] - vr.patch(volL, cell, g - e)[0]) / (2 * h)
            assert abs(float(fd - d[a])) <= 1e-9        # (the patch is linear in each coordinate: central differences are exact)


def test_cell_choice_at_the_upper_face_and_on_short_axes():
    assert vr.exact_cell(LD(4.0), 5) == 3 and vr.exact_cell(LD(3.999), 5) == 3 and vr.exact_cell(LD(0.0), 5) == 0
    assert vr.exact_cell(LD(1.0), 2) == 0 and vr.exact_cell(LD(0.5), 2) == 0
    assert vr.exact_cell(LD(0.0), 1) == 0
    delta = LD(2.0) ** -50 * 5
    assert vr.axis_cells(LD(2.0), 5, delta) == [1, 2] and vr.axis_cells(LD(2.5), 5, delta) == [2]
    assert vr.axis_cells(LD(4.0), 5, delta) == [3] and vr.axis_cells(LD(0.0), 1, delta) == [0]
    # at g = n - 1 the value is the last voxel's and the derivative the last cell's, from inside; an axis of length 1: 0
    vol = np.arange(2 * 1 * 5, dtype=np.float64).reshape(2, 1, 5) ** 2
    p = np.array([ORIGIN[0] + 4 * 0.5, ORIGIN[1], ORIGIN[2] + 0.25], np.float32)
    live, val, grad = vr.sample(vol, ORIGIN, (0.5, 0.5, 0.25), p)
    assert live and float(val) == float(vol[1, 0, 4])
    assert float(grad[0]) == float(vol[1, 0, 4] - vol[1, 0, 3]) / 0.5 and float(grad[1]) == 0.0
    assert float(grad[2]) == float(vol[1, 0, 4] - vol[0, 0, 4]) / 0.25


def test_a_cell_with_a_voxel_that_is_not_finite_is_dead():
    dims = (5, 4, 3)
    vol = np.ones(dims[::-1])
    vol[1, 2, 3] = np.nan
    vol[0, 0, 0] = np.inf
    s = (1.0, 1.0, 1.0)
    o = (0.0, 0.0, 0.0)
    assert not vr.sample(vol, o, s, np.array([2.5, 1.5, 0.5], np.float32))[0]      # the cell (2, 1, 0) holds [1, 2, 3]
    assert not vr.sample(vol, o, s, np.array([3.0, 2.0, 1.0], np.float32))[0]      # the voxel itself, as the cell (3, 2, 1)'s corner
    assert not vr.sample(vol, o, s, np.array([0.5, 0.5, 0.5], np.float32))[0]      # inf
    live, val, grad = vr.sample(vol, o, s, np.array([1.5, 0.5, 1.5], np.float32))  # the cell (1, 0, 1): all finite
    assert live and float(val) == 1.0 and [float(x) for x in grad] == [0.0, 0.0, 0.0]
    assert not vr.sample(vol, o, s, np.array([1.5, 0.5, 1.5], np.float32), gate=0)[0]
    assert not vr.sample(vol, o, s, np.array([1.5, np.nan, 1.5], np.float32))[0]
    assert not vr.sample(vol, o, s, np.array([4.0001, 0.5, 1.5], np.float32))[0]


def test_the_checker_accepts_the_definition_and_rejects_what_breaks_it():
    rng = np.random.default_rng(3)
    dims = (5, 4, 3)
    vol = rng.normal(size=dims[::-1]).astype(np.float32)
    vol[1, 1, 1] = np.nan
    pts = np.concatenate([inside_points(rng, dims, 40), np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0]], np.float32)])
    n_live = 0
    for p in pts:
        live, val, grad = vr.sample(vol, ORIGIN, SPACING, p)
        v32, g32 = np.float32(val), np.array([float(x) for x in grad], np.float32)
        assert vr.check_point(vol, ORIGIN, SPACING, p, 1, v32, live, g32) is None
        assert vr.check_point(vol, ORIGIN, SPACING, p, 1, v32, live, None) is None
        if live:
            n_live += 1
            assert vr.check_point(vol, ORIGIN, SPACING, p, 1, np.float32(v32 + 1e-4), live, g32) is not None
            assert vr.check_point(vol, ORIGIN, SPACING, p, 1, v32, live, g32[[1, 2, 0]] + np.float32(1e-3)) is not None
            assert vr.check_point(vol, ORIGIN, SPACING, p, 1, np.float32(0), False, np.zeros(3, np.float32)) is not None
            assert vr.check_point(vol, ORIGIN, SPACING, p, 0, v32, live, g32) is not None
        else:
            assert vr.check_point(vol, ORIGIN, SPACING, p, 1, np.float32(1.0), True, g32) is not None
    assert 10 < n_live < 40
    # a transposed volume (the index-order mistake) does not pass
    bad = 0
    volT = np.ascontiguousarray(vol.reshape(-1).reshape(dims))      # read as [nx][ny][nz]
    for p in inside_points(rng, dims, 20):
        g = vr.grid_coords(p, ORIGIN, SPACING)
        cell = tuple(vr.exact_cell(g[a], n) for a, n in enumerate(dims))
        wrong = volT[cell[0], cell[1], cell[2]]
        if np.isfinite(wrong) and vr.check_point(vol, ORIGIN, SPACING, p, 1, np.float32(wrong), True, None) is not None:
            bad += 1
    assert bad >= 10
