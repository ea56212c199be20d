"""GPU: the TSDF fusion (bodyfit_volume_integrate_device, k_tsdf.hip) against the extended-precision reference of its contract
(tsdf_ref.py) at EVERY voxel, its bit-identity whatever the batch and the split, a dyadic oracle that does not use the reference,
its error codes, the layer on top of it (torch_layer.volume.integrate_tsdf) and a fit against a fused floor."""
import collections
import ctypes
import importlib

import numpy as np
import pytest

import tsdf_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def tl():
    return importlib.import_module("3dbodyanimation_amd.torch_layer")


@pytest.fixture(scope="module")
def volume():
    return importlib.import_module("3dbodyanimation_amd.torch_layer.volume")


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def subcase(case, frames):
    """the case with the frames `frames` (any order, repeats allowed) as its frames"""
    return tr.make_case(case.dims, case.origin, case.spacing, case.intr, [case.poses[f] for f in frames], case.depth[list(frames)],
                        case.trunc, case.z_near)


def run(torch, api, case, max_weight=np.inf, state=None, per_frame=False, pad=0, with_pose=True):
    """One call over every frame of `case`: (D, W) on the host, [nz, ny, nx] or with per_frame [F, nz, ny, nx].  state None: reset,
    the outputs pre-filled with junk; else (D, W) of the output's shape, continued.  The depth maps lie `pad` floats farther apart
    than H W, the padding poisoned with a plausible depth."""
    nx, ny, nz = case.dims
    F, H, W = case.depth.shape
    handle = api.Volume(0, case.dims, case.origin, case.spacing)
    host = np.full((max(F, 1), H * W + pad), 0.5, np.float32)
    host[:F, :H * W] = case.depth.reshape(F, -1)
    depth = torch.tensor(host, device="cuda")
    pose = torch.tensor(tr.pose_array(case), device="cuda") if with_pose and F > 0 else None
    shape = (F, nz, ny, nx) if per_frame else (nz, ny, nx)
    if state is None:
        D, Wt = torch.full(shape, -5.0, device="cuda"), torch.full(shape, 7.0, device="cuda")
    else:
        D = torch.tensor(np.ascontiguousarray(state[0], np.float32).reshape(shape), device="cuda")
        Wt = torch.tensor(np.ascontiguousarray(state[1], np.float32).reshape(shape), device="cuda")
    handle.integrate_device(depth.data_ptr(), H * W + pad, H, W, F, case.intr, pose.data_ptr() if pose is not None else None,
                            case.trunc, case.z_near, max_weight, state is None, D.data_ptr(), Wt.data_ptr(),
                            nx * ny * nz if per_frame else 0, stream(torch))
    torch.cuda.synchronize()
    return D.cpu().numpy(), Wt.cpu().numpy()


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def check_all(prior, got, steps, max_weight):
    """every voxel of one one-frame step against the contract: the worst error / bound"""
    bad, worst = [], 0.0
    pD, pW, gD, gW = (np.asarray(a).reshape(-1) for a in (*prior, *got))
    for n, step in enumerate(steps):
        why, ratio = tr.check_voxel(pD[n], pW[n], gD[n], gW[n], step, max_weight)
        if why is not None:
            bad.append((n, step.cls, why))
        else:
            worst = max(worst, ratio)
    assert not bad, bad[:5]
    return worst


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", tr.IMAGES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dims", tr.GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_integration_against_the_reference_at_every_voxel(torch, api, dims, image):
    case = tr.random_case(dims, image, seed=1000 * dims[0] + image[0])
    F = tr.N_FRAMES
    steps = [tr.all_steps(case, f) for f in range(F)]
    census = collections.Counter(step.cls for st in steps for step in st)
    empty = (np.full(dims[::-1], np.nan, np.float32), np.zeros(dims[::-1], np.float32))
    worst = 0.0
    # under reset, on junk: frame f into volume f is the one-frame step from the empty state
    got = run(torch, api, case, tr.MAX_WEIGHT, per_frame=True, pad=5)
    for f in range(F):
        worst = max(worst, check_all(empty, (got[0][f], got[1][f]), steps[f], tr.MAX_WEIGHT))
    # from each prior state
    for kind in tr.PRIORS:
        prior = tr.prior_state(kind, dims, seed=dims[0] + image[0])
        tiled = tuple(np.broadcast_to(a, (F,) + a.shape).copy() for a in prior)
        got = run(torch, api, case, tr.MAX_WEIGHT, state=tiled, per_frame=True, pad=5)
        for f in range(F):
            worst = max(worst, check_all(prior, (got[0][f], got[1][f]), steps[f], tr.MAX_WEIGHT))
    # the identity as a NULL pose (the kernel without the pose's arithmetic), one volume, one frame
    prior = tr.prior_state("observed", dims, seed=3)
    got = run(torch, api, subcase(case, [0]), tr.MAX_WEIGHT, state=prior, with_pose=False)
    worst = max(worst, check_all(prior, got, steps[0], tr.MAX_WEIGHT))
    print(f"{dims} {image}: worst error / bound {worst:.3f}; " + ", ".join(f"{c} {census[c]}" for c in tr.CLASSES))
    assert worst <= 1.0


def test_boundary_cases_against_the_reference(torch, api):
    case = tr.boundary_case()
    steps = tr.all_steps(case, 0)
    several = sum(len(step.admissible) > 1 for step in steps)
    worst = 0.0
    for kind in tr.PRIORS:
        prior = tr.prior_state(kind, case.dims, seed=1)
        for with_pose in (False, True):
            worst = max(worst, check_all(prior, run(torch, api, case, tr.MAX_WEIGHT, state=prior, with_pose=with_pose), steps,
                                         tr.MAX_WEIGHT))
    print(f"boundary cases: {several} voxels with more than one admissible vector, worst error / bound {worst:.3f}")
    assert several >= 20


# ---- 2. bit-identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 5])
def test_bit_identity_whatever_the_batch_and_the_split(torch, api, F):
    dims = (17, 9, 6)
    base = tr.random_case(dims, (33, 17), seed=77)
    case = subcase(base, [0, 1, 2, 1, 0][:F])
    for cap in (np.inf, 2.0):
        whole = run(torch, api, case, cap, pad=3)
        assert same_bits(whole, run(torch, api, case, cap, pad=3))                       # from run to run
        chain = None
        for f in range(F):
            chain = run(torch, api, subcase(case, [f]), cap, state=chain)
        assert same_bits(whole, chain)
        part = run(torch, api, subcase(case, [0, 1]), cap)
        assert same_bits(whole, run(torch, api, subcase(case, range(2, F)), cap, state=part))
        seen = np.isfinite(whole[0])
        assert np.array_equal(seen, whole[1] > 0) and seen.sum() > 100 and (~seen).sum() > 100
        assert bool(np.isnan(whole[0][~seen]).all()) and bool((whole[1][~seen] == 0).all())
        if cap == 2.0:
            assert whole[1].max() == 2.0 and (whole[1] == 2.0).sum() > 20                # the cap is reached, and held
        elif F == 5:
            assert whole[1].max() > 2.0                                                  # (what the cap holds down)
    # reset on junk is reset = 0 on the empty state
    nx, ny, nz = dims
    empty = (np.full((nz, ny, nx), np.nan, np.float32), np.zeros((nz, ny, nx), np.float32))
    assert same_bits(run(torch, api, case, 2.0), run(torch, api, case, 2.0, state=empty))
    # per frame: volume f is the one-frame call of frame f alone
    per = run(torch, api, case, per_frame=True)
    for f in range(F):
        assert same_bits((per[0][f], per[1][f]), run(torch, api, subcase(case, [f])))


# ---- 3. the dyadic oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("translation", [None, (0.125, -0.0625, 0.5)], ids=["identity", "translated"])
def test_a_constant_dyadic_depth_is_fused_exactly(torch, api, translation):
    """An identity (or purely translated) camera and a constant dyadic depth z0 over a dyadic grid: every quantity is exact in
    f64, so D = min(z0 - q_z, trunc) exactly where z0 - q_z >= -trunc, and the voxel stays unobserved elsewhere."""
    z0 = 1.25 if translation is None else 1.75
    case = tr.dyadic_case(1, [z0], translation)
    D, W = run(torch, api, case, with_pose=translation is not None)
    s = z0 - (tr.grid_z(case) + (0.0 if translation is None else translation[2]))
    want = np.where(s >= -case.trunc, np.minimum(s, case.trunc), np.nan).astype(np.float32)
    assert np.isnan(want).any() and (want == case.trunc).any() and (np.abs(want) < case.trunc).any()
    assert np.array_equal(D, want, equal_nan=True)
    assert np.array_equal(W, np.where(np.isnan(want), 0, 1).astype(np.float32))
    # five frames under a cap of 2: the first layer is clamped in every frame
    case = tr.dyadic_case(5, [1.5, 1.25, 1.75, 1.375, 1.5], translation=None)
    D, W = run(torch, api, case, 2.0, with_pose=translation is not None)
    assert bool((D[0] == 0.25).all()) and bool((W[0] == 2.0).all()) and W.max() == 2.0


# ---- 4. error codes -----------------------------------------------------------------------------------------------------------------
def test_error_codes_launch_nothing(torch, api):
    lib = api.load_library()
    dims, H, W, F = (5, 4, 3), 7, 9, 2
    h = api.Volume(0, dims, tr.ORIGIN, tr.SPACING)
    depth = torch.full((F, H * W), 0.52, device="cuda")
    pose = torch.tensor(np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (F, 1)), device="cuda")
    D = torch.full((F, 3, 4, 5), -5.0, device="cuda")
    Wt = torch.full((F, 3, 4, 5), 7.0, device="cuda")
    intr = (9.0, 9.0, 4.0, 3.0)
    good = dict(d_depth_ptr=depth.data_ptr(), depth_frame_stride=H * W, height=H, width=W, n_frames=F, intr=intr,
                d_pose_ptr=pose.data_ptr(), trunc=0.015, z_near=0.1, max_weight=np.inf, reset=True, d_tsdf_ptr=D.data_ptr(),
                d_weight_ptr=Wt.data_ptr(), volume_frame_stride=60, stream=stream(torch))
    before = api.launch_count()
    for change in [dict(d_depth_ptr=None), dict(d_tsdf_ptr=None), dict(d_weight_ptr=None), dict(height=0), dict(width=0),
                   dict(height=-1), dict(height=1 << 16, width=1 << 15, depth_frame_stride=1 << 31),
                   dict(depth_frame_stride=H * W - 1), dict(volume_frame_stride=59), dict(volume_frame_stride=-60),
                   dict(volume_frame_stride=1), dict(n_frames=-1), dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=np.inf),
                   dict(trunc=np.nan), dict(z_near=-0.1), dict(z_near=np.inf), dict(z_near=np.nan), dict(max_weight=0.0),
                   dict(max_weight=-1.0), dict(max_weight=np.nan), dict(intr=(np.nan, 9.0, 4.0, 3.0)),
                   dict(intr=(9.0, 9.0, np.inf, 3.0)), dict(intr=(0.0, 9.0, 4.0, 3.0)), dict(intr=(9.0, 0.0, 4.0, 3.0))]:
        with pytest.raises(api.BodyfitError, match="status 1"):
            h.integrate_device(**{**good, **change})
    k = (ctypes.c_double * 4)(*intr)
    assert lib.bodyfit_volume_integrate_device(None, depth.data_ptr(), H * W, H, W, F, k, None, 0.015, 0.1, np.inf, 1, D.data_ptr(),
                                               Wt.data_ptr(), 60, None) == 1
    with pytest.raises(api.BodyfitError, match="status 1"):                              # NULL intr
        h.integrate_device(**{**good, "intr": None})
    # the no-ops: no frames without reset; no frames, per frame
    h.integrate_device(**{**good, "n_frames": 0, "reset": False, "volume_frame_stride": 0, "d_depth_ptr": None})
    h.integrate_device(**{**good, "n_frames": 0, "d_depth_ptr": None, "d_tsdf_ptr": None})
    assert api.launch_count() == before
    torch.cuda.synchronize()
    assert bool((D == -5.0).all()) and bool((Wt == 7.0).all())
    # no frames under reset, one volume: the empty state is written, and nothing beyond the volume
    h.integrate_device(**{**good, "n_frames": 0, "volume_frame_stride": 0, "d_depth_ptr": None})
    assert api.launch_count() == before + 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(D[0]).all()) and bool((Wt[0] == 0).all()) and bool((D[1] == -5.0).all()) and bool((Wt[1] == 7.0).all())
    h.integrate_device(**good)
    assert api.launch_count() == before + 2
    torch.cuda.synchronize()
    assert bool((Wt <= 1).all()) and bool((Wt == 1).any())


# ---- 5. the layer -----------------------------------------------------------------------------------------------------------------
def test_integrate_tsdf_is_the_kernel_and_feeds_the_sampler(torch, api, volume):
    dims = (17, 9, 6)
    case = tr.random_case(dims, (33, 17), seed=77)
    F, H, W = case.depth.shape
    # depth as a view with a frame stride of its own; the pose as [F, 3, 4]
    buf = torch.full((F, H * W + 7), 0.5, device="cuda")
    buf[:, :H * W] = torch.tensor(case.depth.reshape(F, -1), device="cuda")
    depth = buf[:, :H * W].view(F, H, W)
    pose = torch.tensor(tr.pose_array(case).reshape(F, 3, 4), device="cuda")
    args = (case.intr, case.origin, case.spacing, dims, case.trunc)
    D, Wt = volume.integrate_tsdf(depth, *args, pose=pose, z_near=case.z_near, max_weight=2.0)
    assert D.shape == (6, 9, 17) and D.dtype == torch.float32 and Wt.shape == D.shape and not D.requires_grad
    assert same_bits((D.cpu().numpy(), Wt.cpu().numpy()), run(torch, api, case, 2.0))
    # state=: continued, the arguments untouched; [F, 12]; per frame
    first = volume.integrate_tsdf(depth[:2], *args, pose=pose[:2].reshape(2, 12), z_near=case.z_near, max_weight=2.0)
    kept = tuple(t.clone() for t in first)
    D2, W2 = volume.integrate_tsdf(depth[2:], *args, pose=pose[2:], z_near=case.z_near, max_weight=2.0, state=first)
    assert same_bits((D2.cpu().numpy(), W2.cpu().numpy()), (D.cpu().numpy(), Wt.cpu().numpy()))
    assert same_bits(tuple(t.cpu().numpy() for t in first), tuple(t.cpu().numpy() for t in kept))
    Dp, Wp = volume.integrate_tsdf(depth, *args, pose=pose, z_near=case.z_near, per_frame=True)
    assert Dp.shape == (F, 6, 9, 17) and same_bits((Dp.cpu().numpy(), Wp.cpu().numpy()), run(torch, api, case, per_frame=True))
    # without a pose and with the defaults: frame 0 is the identity
    D0, W0 = volume.integrate_tsdf(depth[:1], *args)
    assert same_bits((D0.cpu().numpy(), W0.cpu().numpy()), run(torch, api, subcase(case, [0]), with_pose=False))
    for bad, error in [(dict(depth=depth.double()), TypeError), (dict(depth=depth.cpu()), TypeError), (dict(depth=depth[0]), ValueError),
                       (dict(pose=pose.float()), TypeError), (dict(pose=pose.cpu()), ValueError), (dict(pose=pose[:2]), ValueError),
                       (dict(state=(D, Wt.double())), TypeError), (dict(state=(D[:2], Wt)), ValueError), (dict(state=(D,)), TypeError),
                       (dict(state=(D.cpu(), Wt)), TypeError), (dict(dims=(17, 9, 0)), ValueError), (dict(intr=(1.0, 1.0, 1.0)), ValueError),
                       (dict(state=(D, Wt), per_frame=True), ValueError)]:
        kw = {**dict(depth=depth, intr=case.intr, origin=case.origin, spacing=case.spacing, dims=dims, trunc=case.trunc, pose=pose), **bad}
        with pytest.raises(error):
            volume.integrate_tsdf(**kw)
    # straight into the sampler: a point at a voxel centre of an observed cell is valid, one in an unobserved cell is not
    seen = np.isfinite(D.cpu().numpy())
    nx, ny, nz = dims
    cell_seen = np.ones((nz - 1, ny - 1, nx - 1), bool)
    cell_any = np.zeros_like(cell_seen)
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                part = seen[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]
                cell_seen &= part
                cell_any |= part
    k, j, i = np.nonzero(cell_seen | ~cell_any)
    assert cell_seen.sum() >= 10 and (~cell_any).sum() >= 10
    centre = np.stack([case.origin[0] + (i + 0.5) * case.spacing[0], case.origin[1] + (j + 0.5) * case.spacing[1],
                       case.origin[2] + (k + 0.5) * case.spacing[2]], axis=-1).astype(np.float32)
    value, valid = volume.sample_volume(D, case.origin, case.spacing, torch.tensor(centre[None], device="cuda"))
    assert np.array_equal(valid[0].cpu().numpy(), cell_seen[k, j, i])
    assert bool((value[0][valid[0]].abs() <= case.trunc * (1 + 1e-6)).all())


# ---- 6. a fit ----------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, down):
    """world -> camera [A | t] as 12 f64: the optical axis from `eye` to `target`, the image's v axis along `down`"""
    z = (target - eye) / np.linalg.norm(target - eye)
    y = down - (down @ z) * z
    y /= np.linalg.norm(y)
    A = np.stack([np.cross(y, z), y, z])
    return np.concatenate([A, (-A @ eye).reshape(3, 1)], axis=1).reshape(12)


def test_gradient_steps_lift_the_body_off_a_fused_floor(torch, tl, api, synth, volume):
    """test_gpu_volume's floor fit with a FUSED floor: the depth maps of the plane the body stands on, in closed form from three
    oblique poses, fused, and VolumeTerm(mode="inside") on the result."""
    F, V = 1, 1000
    m = synth.make_model(0, n_verts=V)
    seq = synth.make_sequence(m, F, seed=4)
    layer = tl.SMPLLayer(api.Model(m), R0=seq.R0.reshape(F, 3, 3))
    x, b = torch.tensor(seq.gt_params, device="cuda"), torch.tensor(seq.gt_beta, device="cuda")
    with torch.no_grad():
        verts = layer(x, b)[0]
    lo, hi = verts[0].min(dim=0).values.cpu().numpy().astype(np.float64), verts[0].max(dim=0).values.cpu().numpy().astype(np.float64)
    level = hi[1]                                               # the floor: y = the body's largest y, the inside beyond it
    x = x.clone()
    x[:, 5] += 0.03                                             # 3 cm into it
    dims = (24, 32, 24)
    origin = tuple(lo - 0.2)
    spacing = tuple((hi - lo + 0.4) / (np.array(dims) - 1))
    # the plane m . p = c with the cameras on the side m . p > c (y < level); depth along the optical axis in closed form
    H, W, fx = 240, 320, 250.0
    intr = (fx, fx, 159.5, 119.5)
    normal, c = np.array([0.0, -1.0, 0.0]), -level
    ground = np.array([0.5 * (lo[0] + hi[0]), level, 0.5 * (lo[2] + hi[2])])
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(j - intr[2]) / fx, (i - intr[3]) / fx, np.ones((H, W))], axis=-1)
    poses, depth = [], np.zeros((3, H, W), np.float32)
    for f, off in enumerate([(-1.2, -1.6, -2.4), (0.2, -2.2, -2.2), (1.3, -1.5, 2.3)]):
        P = look_at(ground + np.array(off), ground, np.array([0.0, 1.0, 0.0]))
        A, t = P.reshape(3, 4)[:, :3], P.reshape(3, 4)[:, 3]
        with np.errstate(divide="ignore"):
            z = (c + (A @ normal) @ t) / (ray @ (A @ normal))
        depth[f] = np.where(np.isfinite(z) & (z > 0) & (z < 20.0), z, 0.0)
        poses.append(P)
    trunc = 0.03 + 3 * max(spacing)                             # the body's 3 cm and the cells around them stay observed
    D, Wt = volume.integrate_tsdf(torch.tensor(depth, device="cuda"), intr, origin, spacing, dims, trunc,
                                  pose=torch.tensor(np.stack(poses), device="cuda"))
    y = origin[1] + spacing[1] * np.arange(dims[1])
    Dh = D.cpu().numpy()
    seen = np.isfinite(Dh)
    plane = np.broadcast_to((level - y)[None, :, None], Dh.shape)
    print(f"fused floor: {int(seen.sum())} of {seen.size} voxels observed, weights up to {float(Wt.max()):.0f}; fused distance against "
          f"level - y inside the band: worst {1e3 * float(np.abs(Dh - plane)[seen & (np.abs(plane) < 0.5 * trunc)].max(initial=0.0)):.1f} mm")
    assert seen.sum() > seen.size // 4 and float(Wt.max()) == 3.0
    term = volume.VolumeTerm(D, origin, spacing, mode="inside")

    def state(xc):
        xc = xc.clone().requires_grad_()
        v = layer(xc, b)[0]
        parts = term.evaluate(v)
        parts["cost"].backward()
        return (float(parts["cost"].detach()), float(v.detach()[0, :, 1].max()) - level, int((parts["r"].detach() < 0).sum()),
                xc.grad[:, 4:7].clone())

    cost, depth0, rows0, g = state(x)
    assert rows0 > 0
    lr = 0.1 / rows0                     # (the cost's curvature along the floor's normal is 2 rows |grad phi|^2, |grad phi| near 1)
    costs, deep = [cost], depth0
    xc = x.clone()
    for _ in range(5):
        xc[:, 4:7] -= lr * g
        cost, deep, rows, g = state(xc)
        costs.append(cost)
    print(f"fused floor fit: {rows0} vertices inside at the start, cost {' -> '.join(f'{c:.3e}' for c in costs)}, deepest penetration "
          f"{1e3 * depth0:.2f} mm -> {1e3 * deep:.2f} mm")
    assert all(b_ < a_ for a_, b_ in zip(costs, costs[1:]))
    assert deep < depth0
