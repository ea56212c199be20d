"""CPU: the reference of the TSDF fusion (tsdf_ref.py, the definition of bodyfit_volume_integrate_device in longdouble) against
facts that do not use it, a census of the shared case generator, and the checker against the definition and against each way of
getting it wrong.  The kernel itself is tested in test_gpu_tsdf.py."""
import collections
import fractions
import functools

import numpy as np
import pytest

import tsdf_ref as tr


@pytest.mark.parametrize("translation", [None, (0.125, -0.0625, 0.5)], ids=["identity", "translated"])
def test_a_constant_depth_gives_the_clamped_distance_exactly(translation):
    z0 = 1.25 if translation is None else 1.75
    case = tr.dyadic_case(1, [z0], translation)
    D, W = tr.fuse(case, [0])
    s = z0 - (tr.grid_z(case) + (0.0 if translation is None else translation[2]))
    want = np.where(s >= -case.trunc, np.minimum(s, case.trunc), np.nan).astype(np.float32)
    assert np.isnan(want).any() and (want == case.trunc).any() and (np.abs(want) < case.trunc).any()
    assert np.array_equal(D, want, equal_nan=True)
    assert np.array_equal(W, np.where(np.isnan(want), 0, 1).astype(np.float32))


def plane_case():
    """the plane m . x = c seen from three oblique poses; depth maps in closed form: z = (c + (A m) . t) / ((A m) . r) along the ray
    r = ((j - cx) / fx, (i - cy) / fy, 1) of pixel (i, j)"""
    rng = np.random.default_rng(12)
    dims, spacing = (6, 5, 4), (0.02, 0.02, 0.02)
    origin = (-0.05, -0.04, 1.97)
    m = np.array([0.2, -0.25, -1.0])
    m /= np.linalg.norm(m)
    c = float(m @ np.array([0.0, 0.0, 2.0]))                    # through the volume's middle; the cameras are on the side m . x > c
    H, W, fx = 48, 64, 600.0
    intr = (fx, fx, 31.5, 23.5)
    mid = np.array([origin[a] + 0.5 * (dims[a] - 1) * spacing[a] for a in range(3)])
    poses, depth = [], np.empty((3, H, W), np.float32)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for f in range(3):
        P = tr.rigid(rng, 0.06 * (f + 1), (0, 0, 0)).reshape(3, 4)
        A = P[:, :3]
        t = mid - A @ mid + rng.uniform(-0.003, 0.003, size=3)
        poses.append(np.concatenate([A, t.reshape(3, 1)], axis=1).reshape(12))
        Am = A @ m
        r = np.stack([(j - intr[2]) / fx, (i - intr[3]) / fx, np.ones_like(i, dtype=np.float64)], axis=-1)
        depth[f] = (c + Am @ t) / (r @ Am)
    return tr.make_case(dims, origin, spacing, intr, poses, depth, 0.05, 0.1), m, c


def test_an_oblique_plane_keeps_the_sign_of_its_distance():
    case, m, c = plane_case()
    spacing = min(case.spacing)
    # the half-pixel slop of a depth read at the nearest pixel, from the maps themselves, against the spacing
    slop = max(0.5 * (np.abs(np.diff(d, axis=0)).max() + np.abs(np.diff(d, axis=1)).max()) for d in case.depth.astype(np.float64))
    assert 10 * slop <= spacing, (slop, spacing)
    D, W = tr.fuse(case, [0, 1, 2])
    nx, ny, nz = case.dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([case.origin[0] + i * case.spacing[0], case.origin[1] + j * case.spacing[1], case.origin[2] + k * case.spacing[2]], -1)
    dist = p @ m - c                                            # positive on the cameras' side
    # along the optical axis a distance delta shows as at least delta q_z / |q|: the rays are within a few degrees of the axis
    cos = min(float((q[..., 2] / np.linalg.norm(q, axis=-1)).min())
              for q in (p @ P.reshape(3, 4)[:, :3].T + P.reshape(3, 4)[:, 3] for P in case.poses))
    assert cos * spacing > 5 * slop
    far = np.isfinite(D) & (W > 0) & (np.abs(dist) > spacing)
    assert far.sum() >= 20 and (dist[far] > 0).sum() >= 5 and (dist[far] < 0).sum() >= 5
    assert np.array_equal(np.sign(D[far]), np.sign(dist[far]))
    assert W.max() == 3


def test_split_invariance_and_the_cap():
    case = tr.dyadic_case(5, [1.5, 1.25, 1.75, 1.375, 1.5])
    steps = [tr.all_steps(case, f) for f in range(5)]
    whole = tr.fuse(case, range(5), max_weight=2.0, steps=steps)
    part = tr.fuse(case, [0, 1], max_weight=2.0, steps=steps)
    split = tr.fuse(case, [2, 3, 4], max_weight=2.0, state=part, steps=steps)
    chain = None
    for f in range(5):
        chain = tr.fuse(case, [f], max_weight=2.0, state=chain, steps=steps)
    for other in (split, chain):
        assert np.array_equal(whole[0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(whole[1], other[1])
    D, W = whole
    assert W.max() == 2.0 and (W == 2.0).sum() >= 20
    # the first layer, z = 1: s = 0.5, 0.25, 0.75, 0.375, 0.5, clamped at 0.25: D = 0.25 whatever the cap
    assert np.all(D[0] == 0.25) and np.all(W[0] == 2.0)
    # the layer z = 1.375: s = 0.125, -0.125, 0.375 (clamped: 0.25), 0, 0.125: the capped average by hand, in fractions, rounded
    # to f32 after every frame; the weight is 1, then 2, and stays 2
    d = fractions.Fraction(0)                                   # after two frames: (0.125 - 0.125) / 2
    for s in (fractions.Fraction(1, 4), fractions.Fraction(0), fractions.Fraction(1, 8)):
        d = fractions.Fraction(float(np.float32(float((2 * d + s) / 3))))
    assert np.all(D[3] == np.float32(float(d))) and 0.078 < float(d) < 0.079
    free = tr.fuse(case, range(5), steps=steps)
    assert free[1].max() == 5.0 and not np.array_equal(free[0], D, equal_nan=True)


@functools.lru_cache(maxsize=None)
def census(dims):
    """(classes over every voxel-step of the generator's images and frames, the most admissible vectors of any of them)"""
    count, most = collections.Counter(), 0
    for image in tr.IMAGES:
        case = tr.random_case(dims, image, seed=1000 * dims[0] + image[0])
        for f in range(tr.N_FRAMES):
            for step in tr.all_steps(case, f):
                count[step.cls] += 1
                most = max(most, len(step.admissible))
    return count, most


@pytest.mark.parametrize("dims", [(5, 4, 3), (17, 9, 6)], ids=lambda d: "x".join(map(str, d)))
def test_census_of_the_generator(dims):
    count, most = census(dims)
    print(f"{dims}: " + ", ".join(f"{c} {count[c]}" for c in tr.CLASSES) + f"; at most {most} admissible vector(s) per voxel-step")
    assert all(count[c] >= 5 for c in tr.CLASSES), count
    assert most == 1                                            # a condition on the inputs: the seeds are chosen to meet it


def test_the_boundary_cases_are_on_their_boundaries():
    case = tr.boundary_case()
    nx, ny, nz = case.dims
    steps = tr.all_steps(case, 0)
    at = lambda i, j, k: steps[(k * ny + j) * nx + i]
    keys = lambda step: {v[0][0] for v in step.admissible}
    assert at(2, 0, 0).cls == "behind" and keys(at(2, 0, 0)) == {"behind", "update"}           # q_z = z_near exactly
    assert at(2, 0, 2).cls == "band" and keys(at(2, 0, 2)) == {"update", "hidden"}             # s = -trunc exactly
    assert at(2, 0, 1).cls == "band" and len(at(2, 0, 1).admissible) == 1                      # u = 2, v = 1: inside pixel (1, 2)
    edge = at(3, 1, 1)                                                                          # u = 2.5, v = 1.5: a corner of four pixels
    assert edge.cls == "hole" and {v[0][1:] for v in edge.admissible} == {(1, 2), (1, 3), (2, 2), (2, 3)}


def accepted(case, f, prior, got, max_weight, steps):
    bad, worst = [], 0.0
    for n, step in enumerate(steps):
        why, ratio = tr.check_voxel(prior[0].reshape(-1)[n], prior[1].reshape(-1)[n], got[0].reshape(-1)[n], got[1].reshape(-1)[n],
                                    step, max_weight)
        if why is not None:
            bad.append((n, why))
        else:
            worst = max(worst, ratio)
    return bad, worst


def test_checker_accepts_the_definition_and_rejects_each_mistake():
    dims = (5, 4, 3)
    rejected = collections.Counter()
    for image in tr.IMAGES[1:]:
        case = tr.random_case(dims, image, seed=1000 * dims[0] + image[0])
        for f in range(tr.N_FRAMES):
            steps = tr.all_steps(case, f)
            for kind in tr.PRIORS:
                prior = tr.prior_state(kind, dims, seed=f)
                bad, worst = accepted(case, f, prior, tr.simulate(case, f, *prior, tr.MAX_WEIGHT), tr.MAX_WEIGHT, steps)
                assert not bad and worst < 1.0, (image, f, kind, bad[:3])
                # the reference's own stepping is the definition, rounded: accepted too
                bad, _ = accepted(case, f, prior, tr.fuse(case, [f], tr.MAX_WEIGHT, state=prior, steps={f: steps}), tr.MAX_WEIGHT, steps)
                assert not bad, (image, f, kind, bad[:3])
                for how in tr.MUTATIONS:
                    bad, _ = accepted(case, f, prior, tr.simulate(case, f, *prior, tr.MAX_WEIGHT, mutate=how), tr.MAX_WEIGHT, steps)
                    rejected[how] += bool(bad)
    print("cases that reject: " + ", ".join(f"{how} {rejected[how]}" for how in tr.MUTATIONS))
    assert all(rejected[how] >= 1 for how in tr.MUTATIONS), rejected
    # the boundary cases: the definition is accepted on them, whichever side it takes
    case = tr.boundary_case()
    steps = tr.all_steps(case, 0)
    prior = tr.prior_state("observed", case.dims, seed=0)
    bad, _ = accepted(case, 0, prior, tr.simulate(case, 0, *prior, tr.MAX_WEIGHT), tr.MAX_WEIGHT, steps)
    assert not bad, bad[:3]
