"""CPU: the volume distance transform's algorithm (tests/edt3_ref.py kernel_form: k_edt.hip over the slices, then the z pass of
k_edt3.hip step by step) against the definition, and numpy restatements of torch_layer.volume.esdf / occupancy_sdf on planes.

No tolerance in the transform: dist2 equals the definition at every voxel (all pairs on the small shapes, the exact per-axis
minimum on the large one) and nearest is a seed at exactly that squared distance."""
import numpy as np
import pytest

import edt3_ref as e3


# ---- 1. the transform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", e3.KINDS)
@pytest.mark.parametrize("shape", e3.SHAPES, ids=lambda s: "x".join(str(n) for n in s))
def test_kernel_form_is_the_definition(shape, kind):
    mask = e3.make_mask(kind, shape)
    dist2, nearest = e3.kernel_form(mask)
    e3.check(mask, dist2, nearest, e3.want(kind, shape))


def test_separable_is_the_definition_where_both_can_run():
    for kind in e3.KINDS:
        mask = e3.make_mask(kind, (9, 13, 67))
        assert np.array_equal(e3.separable(mask), e3.brute(mask))
        assert np.array_equal(e3.separable(~mask), e3.brute(~mask))


def test_the_reigning_slice_can_lie_above_the_voxel_being_written():
    """why the z pass cannot run in place over d2 without carrying g: on the way back up, g of the reigning slice is read after
    that slice itself has been written"""
    n_above = 0
    for kind in e3.KINDS:
        mask = e3.make_mask(kind, (9, 13, 67))
        _, nearest = e3.kernel_form(mask)
        if mask.any():
            k = np.indices(mask.shape)[0]
            n_above += int((nearest // (13 * 67) > k).sum())
    assert n_above > 0


def test_the_named_masks_are_what_they_say():
    shape = (9, 13, 67)
    assert not e3.make_mask("empty", shape).any() and e3.make_mask("full", shape).all()
    assert e3.make_mask("corners", shape).sum() == 2
    tie = e3.make_mask("tie", shape)
    ks = np.nonzero(tie)[0]
    assert tie.sum() == 2 and (ks[0] + ks[1]) % 2 == 0                    # a whole plane half-way between the two
    sparse = e3.make_mask("random_0.002", (70, 3, 5))
    assert 0 < sparse.sum() and (~sparse.any(axis=(1, 2))).sum() > 35        # most slices are empty
    assert e3.make_mask("random_0.002", (1, 1, 1)).sum() == 1             # at least one seed
    shell = e3.make_mask("shell", (24, 24, 24))
    assert shell.any() and not shell[12, 12, 12] and not shell[0, 0, 0]


# ---- 2. the fields on planes -----------------------------------------------------------------------------------------------------
SPACING, TRUNC = 0.05, 0.12
PLANES = {
    # (shape, normal, offset, unobserved block)
    "axis": ((20, 24, 22), (0.0, 1.0, 0.0), 0.53, None),
    "tilted": ((40, 40, 40), (0.35, 0.85, -0.4), 0.61, (8, 20, 14, 30, 10, 24)),
}


@pytest.mark.parametrize("name", PLANES)
def test_esdf_on_a_plane(name):
    shape, normal, offset, hole = PLANES[name]
    tsdf, true = e3.plane_tsdf(shape, SPACING, normal, offset, TRUNC, hole)
    out = e3.esdf(tsdf, SPACING, TRUNC, e3.kernel_form)
    seen = np.isfinite(tsdf)
    assert np.isfinite(out).all() and out.dtype == np.float32
    # the sign is exact where the voxel was observed
    assert np.array_equal(out[seen] < 0, tsdf[seen] < 0)
    # inside the band it is the TSDF, bit for bit
    band = seen & (np.abs(tsdf) < TRUNC)
    assert band.sum() > 0 and np.array_equal(out[band], tsdf[band])
    # outside the band it is an upper estimate: spacing sqrt(D) + |phi(n)| >= |p - p_n| + dist(p_n, plane) >= dist(p, plane) by the
    # triangle inequality, up to phi(n)'s own rounding to f32 (2^-24 relative, of at most trunc) and the result's (2^-24 relative)
    rest = ~band
    slack = 2.0 ** -23 * (np.abs(true) + TRUNC)
    assert rest.sum() > 0 and np.all(np.abs(out[rest].astype(np.float64)) >= np.abs(true[rest]) - slack[rest])
    wrong = (out < 0) != (true < 0)
    print(f"esdf on the {name} plane: {int(wrong.sum())} of {out.size} voxels with the wrong sign, "
          f"{int((wrong & seen).sum())} of them observed; worst overestimate outside the band "
          f"{float((np.abs(out[rest]) - np.abs(true[rest])).max()):.4f} m")
    assert not (wrong & seen).any()
    if hole is None:
        assert not wrong.any()
    else:
        inside_hole = np.zeros(shape, bool)
        inside_hole[hole[0]:hole[1], hole[2]:hole[3], hole[4]:hole[5]] = True
        hidden = true < -TRUNC
        assert not (wrong & ~inside_hole & ~hidden).any()


def test_esdf_without_a_crossing_is_nan_and_weights_gate():
    tsdf = np.full((5, 6, 7), 0.1, np.float32)
    assert np.isnan(e3.esdf(tsdf, SPACING, TRUNC, e3.kernel_form)).all()
    tsdf[2:] = -0.02
    weight = np.ones_like(tsdf)
    plain = e3.esdf(tsdf, SPACING, TRUNC, e3.kernel_form)
    assert np.isfinite(plain).all() and np.array_equal(plain[2], tsdf[2])
    weight[1:3] = 0.0                                                     # both layers of the crossing unusable: none left
    assert np.isnan(e3.esdf(tsdf, SPACING, TRUNC, e3.kernel_form, weight=weight, min_weight=1.0)).all()
    iso = e3.esdf(tsdf, SPACING, TRUNC, e3.kernel_form, iso=0.04)
    assert np.array_equal(iso[0], np.full((6, 7), np.float32(np.float64(np.float32(0.1)) - 0.04)))


@pytest.mark.parametrize("name", PLANES)
def test_occupancy_sdf_on_a_plane(name):
    shape, normal, offset, _ = PLANES[name]
    _, true = e3.plane_tsdf(shape, SPACING, normal, offset, TRUNC)
    inside = true < 0
    out = e3.occupancy_sdf(inside, SPACING, e3.kernel_form)
    assert np.isfinite(out).all() and np.array_equal(out < 0, inside)
    # the nearest voxel of the other side lies beyond the plane: spacing sqrt(dist2) >= the true distance, so |out| >= |true| -
    # spacing / 2 (f32 rounding: 2^-24 relative)
    assert np.all(np.abs(out.astype(np.float64)) >= (np.abs(true) - 0.5 * SPACING) * (1 - 2.0 ** -23) - 2.0 ** -23 * SPACING)
    if name == "axis":
        # layers straight across: the distance to the other side's first layer less half a voxel, exactly
        j = np.arange(shape[1])
        first_in = int(np.nonzero(inside[0, :, 0])[0].max())             # inside is normal . p < offset: the low layers
        want = np.where(j <= first_in, -(first_in + 1 - j - 0.5), j - first_in - 0.5) * SPACING
        assert np.array_equal(out, np.broadcast_to(want.astype(np.float32)[None, :, None], shape))
    assert np.isnan(e3.occupancy_sdf(np.zeros((3, 4, 5), bool), SPACING, e3.kernel_form)).all()
    assert np.isnan(e3.occupancy_sdf(np.ones((3, 4, 5), bool), SPACING, e3.kernel_form)).all()


# ---- 3. the fit's loop --------------------------------------------------------------------------------------------------------------
def test_soles_above_the_band_come_down_on_the_esdf_and_not_on_the_tsdf():
    """The GPU fit (tests/test_gpu_edt3.py) in numpy: a floor's TSDF in closed form, the soles 0.4 m above it.  On the TSDF the
    cell is the constant trunc and the gradient is exactly zero; on esdf the same damped steps bring the soles down to well below
    a quarter of the start: the bound of the GPU test has room."""
    shape, spacing, trunc, level = (30, 20, 30), 0.05, 0.12, 0.13        # the floor at y = level, the world below it; y is up here
    tsdf, _ = e3.plane_tsdf(shape, spacing, (0.0, 1.0, 0.0), level, trunc)
    rng = np.random.default_rng(5)
    soles = np.stack([0.4 + 0.5 * rng.random(12), level + 0.4 + 0.02 * rng.random(12), 0.5 + 0.4 * rng.random(12)], axis=1)
    origin = (0.0, 0.0, 0.0)

    def on(vol):
        def f(p):
            value, valid, grad = e3.trilinear(vol, origin, spacing, p)
            assert valid.all()
            return value, grad
        return f

    path, first = e3.sole_descent(on(tsdf), soles, 6)
    assert np.all(first == 0.0) and np.all(path == 0.0)
    field = e3.esdf(tsdf, spacing, trunc, e3.kernel_form)
    path, first = e3.sole_descent(on(field), soles, 6)
    height = (soles[:, 1] - level).mean() + path[:, 1]
    print(f"numpy soles: height {' -> '.join(f'{h:.4f}' for h in height)} m")
    assert first[1] > 0 and abs(first[0]) < 1e-9 * first[1] and abs(first[2]) < 1e-9 * first[1]
    assert abs(height[-1]) < height[0] / 16                               # (1/64 for an exact distance; the GPU test asks 1/4)
