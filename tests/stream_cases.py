"""The stream table: one row per asynchronous entry point of the public surface, for tests/test_gpu_streams.py (which runs the rows)
and tests/test_stream_cases.py (which checks, without a GPU, that no entry point is missing from the table).

A row holds
    name       its id
    build      build(fresh=False) -> Scene, on the default stream: a SMALL scene (F = 3 frames, a 1000-vertex body or the two
               spheres of raster_ref, 32 x 48 images, 9 x 13 x 17 volumes, 16 x 16 textures) from the builders of tests/*_ref.py.
               fresh=True (rows with `lazy`): the OWNER of the row's lazily created state is new and already created (the layer's
               problem, the kept handle), so that creating it is not part of the row's first call; what the first call itself
               makes (the problem's VJP / JVP / residual-VJP buffers, the handle's workspace) does not exist yet
    reaches    the bodyfit_*_device exports (include/bodyfit.h) and the torch-layer names the row runs
    host_sync  False where the entry point's docstring or header text promises "no host synchronisation" (or plain "asynchronous
               on `stream`"); otherwise the documented synchronisation, in words
    lazy       None, or the kind of lazily created state the row's first call makes (check (c) of test_gpu_streams.py)

A Scene holds the device tensors the operation READS ON THE STREAM, twice: `real`, and `stale`, other VALID data of the same
shapes (another pose, another mask, other in-range indices: never poison), and run(tensors) -> the operation's device outputs,
through the public surface, on torch.cuda.current_stream().  Importing this module needs neither torch nor a GPU; building a
scene needs both."""
import functools
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F = 3                                    # frames: a partial frame tile
INTR, SIZE = (80.0, 80.0, 24.0, 16.0), (32, 48)          # the two spheres of raster_ref in a 32 x 48 image
DIMS = (9, 13, 17)                       # (nx, ny, nz) of the volumes
RENDER = "the render's 8-byte read-back"
NONZERO = RENDER + ", and the backward's nonzero that lists its rows"


class Scene:
    def __init__(self, real, stale, run, status=None, close=None):
        self.real, self.stale, self.run, self.status, self.close = real, stale, run, status, close


class Row:
    def __init__(self, name, build, reaches, host_sync=False, lazy=None):
        self.name, self.build, self.reaches, self.host_sync, self.lazy = name, build, tuple(reaches), host_sync, lazy

    def __repr__(self):
        return f"Row({self.name})"


# ---- what the scenes share -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def env():
    import torch
    e = types.SimpleNamespace(torch=torch, kept={})
    e.api = importlib.import_module("3dbodyanimation_amd.api")
    e.synth = importlib.import_module("3dbodyanimation_amd.synth")
    e.tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    for name in ("_common", "lighting", "volume", "texture", "silhouette"):
        setattr(e, name.lstrip("_"), importlib.import_module("3dbodyanimation_amd.torch_layer." + name))
    if e.api.device_count() < 1:
        raise RuntimeError("no GPU visible: the stream rows need an MI355X (there is no CPU fallback)")
    e.model = e.synth.make_model(0, n_verts=1000)
    e.gm = e.api.Model(e.model, device=0)
    e.layer = e.tl.SMPLLayer(e.gm)
    e.dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return e


def _stream():
    return env().torch.cuda.current_stream().cuda_stream


def _scene(pairs, run, **kw):
    """pairs: {name: (real, stale)}, host arrays or device tensors"""
    e = env()
    return Scene({k: e.dev(a) for k, (a, _) in pairs.items()}, {k: e.dev(b) for k, (_, b) in pairs.items()}, run, **kw)


def _leaf(t):
    """t's storage as a leaf that requires grad (no copy: the operation reads the tensor the test filled on the stream)"""
    return t.detach().requires_grad_()


def _f32(rng, shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def _unit(rng, shape):
    d = rng.standard_normal(shape)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _body():
    """the SMPL rows' host data: a 3-frame sequence of the 1000-vertex body, and every tensor a row reads, real and stale"""
    e = env()
    V, nJ, nS = e.model.n_verts, e.model.n_joints, e.model.n_shape
    rng = np.random.default_rng(11)
    b = types.SimpleNamespace(seq=e.synth.make_sequence(e.model, F, seed=0), V=V)
    x, beta = b.seq.gt_params + 0.01, np.asarray(b.seq.gt_beta, np.float64) + 0.05
    K = 3
    b.pairs = dict(
        x=(x, x + 0.05 * rng.standard_normal(x.shape)), beta=(beta, beta + 0.1 * rng.standard_normal(beta.shape)),
        offsets_shared=(_f32(rng, (V, 3), 0.01), _f32(rng, (V, 3), 0.01)),
        offsets_frames=(_f32(rng, (F, V, 3), 0.01), _f32(rng, (F, V, 3), 0.01)),
        g_verts=(_f32(rng, (F, V, 3)), _f32(rng, (F, V, 3))),
        g_joints=(rng.standard_normal((F, nJ, 3)), rng.standard_normal((F, nJ, 3))),
        tan_x=(rng.standard_normal((F, K, 76)), rng.standard_normal((F, K, 76))),
        tan_beta=(rng.standard_normal((K, nS)), rng.standard_normal((K, nS))))
    return b


@functools.lru_cache(maxsize=None)
def _mesh():
    """the mesh rows' host data: the two spheres of raster_ref, shifted per frame, seen through INTR in a SIZE image"""
    import raster_ref as rr
    v0, faces, _, _ = rr.two_spheres()
    rng = np.random.default_rng(12)
    m = types.SimpleNamespace(faces=faces, V=len(v0))
    shifts = np.array([[0.0, 0.0, 0.0], [0.03, -0.02, 0.05], [-0.04, 0.03, -0.06]], np.float32)
    verts = (v0[None] + shifts[:, None]).astype(np.float32)
    stale = (verts + np.array([0.05, 0.04, 0.1], np.float32) + _f32(rng, verts.shape, 0.003)).astype(np.float32)
    n = verts[:, ::7].shape[1]
    H, W = SIZE
    m.pairs = dict(
        verts=(verts, stale),
        points=(verts[:, ::7] + _f32(rng, (F, n, 3), 0.03), stale[:, ::7] + _f32(rng, (F, n, 3), 0.03)),
        point_normals=(_unit(rng, (F, n, 3)), _unit(rng, (F, n, 3))),
        skip_vertex=(rng.integers(0, m.V, (F, n)).astype(np.int32), rng.integers(0, m.V, (F, n)).astype(np.int32)),
        g_rows=(_f32(rng, (F * n,)), _f32(rng, (F * n,))),
        field=(_f32(rng, (F, m.V, 3)), _f32(rng, (F, m.V, 3))), g_field=(_f32(rng, (F, m.V, 3)), _f32(rng, (F, m.V, 3))),
        g_pixels=(_f32(rng, (F, H, W)), _f32(rng, (F, H, W))),
        image=(_f32(rng, (F, H, W, 3)), _f32(rng, (F, H, W, 3))), g_image=(_f32(rng, (F, H, W, 3)), _f32(rng, (F, H, W, 3))),
        attr=(_f32(rng, (m.V, 3)), _f32(rng, (m.V, 3))),
        light=(_f32(rng, (9, 3), 0.3), _f32(rng, (9, 3), 0.3)))
    return m


def _pick(data, names, rename=None):
    return {(rename or {}).get(k, k): data.pairs[k] for k in names}


def _fresh_cache(name, make=None):
    """forget the layer's kept handles of one kind and (make) create the row's anew, unused: its first call through the layer is
    the handle's first use.  The rows look their handles up in these caches on every call and hold none themselves, so the kept
    scenes of other rows just get a new handle; a row that held a handle would depend on the order of the tests."""
    getattr(env().common, name).clear()
    if make is not None:
        make()


# ---- smpl ----------------------------------------------------------------------------------------------------------------------
def _smpl(kind, offsets=None):
    def build(fresh=False):
        e, b = env(), _body()
        torch = e.torch
        layer = e.tl.SMPLLayer(e.gm) if fresh else e.layer
        if fresh:
            layer.problem(F)               # (created here: the row's first call makes only the problem's VJP / JVP buffers)
        names = ["x", "beta"] + {"backward": ["g_verts", "g_joints"], "jvp": ["tan_x", "tan_beta"]}.get(kind, [])
        pairs = _pick(b, names)
        if offsets:
            pairs["offsets"] = b.pairs["offsets_" + offsets]

        def run(t):
            off = t.get("offsets")
            if kind == "forward":
                return layer(t["x"], t["beta"], off)
            if kind == "backward":
                wrt = [_leaf(t["x"]), _leaf(t["beta"])] + ([_leaf(off)] if off is not None else [])
                verts, joints = layer(*wrt)
                return torch.autograd.grad((verts, joints), wrt, (t["g_verts"], t["g_joints"]))
            if kind == "jvp":
                return layer.jvp(t["x"], t["beta"], t["tan_x"], t["tan_beta"], offsets=off)
            return layer.jacobian(t["x"], t["beta"], offsets=off)

        def close():
            for p in layer._problems.values():
                p.close()
            layer._problems.clear()

        return _scene(pairs, run, close=close if fresh else None)
    return build


def _problem(want_mesh):
    e, b = env(), _body()
    return e.api.Problem.from_sequence(e.gm, b.seq, n_cols=86, use_shape=True, beta_pose=5.0, beta_shape=25.0, lambda_temporal=3.0,
                                       want_mesh=want_mesh)


def _kept_problem(want_mesh):
    e = env()
    key = ("problem", want_mesh)
    if key not in e.kept:
        e.kept[key] = _problem(want_mesh)
    return e.kept[key]


def _objective(kind):
    def build(fresh=False):
        e, b = env(), _body()
        torch = e.torch
        prob = _problem(False) if fresh else _kept_problem(False)
        obj = e.tl.FitObjective(prob)
        rng = np.random.default_rng(13)
        n = prob.layout.total_rows
        pairs = _pick(b, ["x", "beta"])
        if kind == "backward":
            pairs["g_rows"] = (rng.standard_normal(n), rng.standard_normal(n))

        def run(t):
            if kind == "forward":
                return (obj(t["x"], t["beta"]),)
            wrt = (_leaf(t["x"]), _leaf(t["beta"]))
            r = obj(*wrt)
            return (r.detach(),) + torch.autograd.grad(r, wrt, t["g_rows"])

        return _scene(pairs, run, close=prob.close if fresh else None)
    return build


# ---- the api level ---------------------------------------------------------------------------------------------------------------
def _api_evaluate(fresh=False):
    e, b = env(), _body()
    torch = e.torch
    prob = _kept_problem(True)

    def run(t):
        out = torch.empty(66, dtype=torch.float64, device="cuda")
        prob.evaluate_device(t["x"].data_ptr(), t["beta"].data_ptr(), True, _stream())
        prob.reduce_shared_device(out.data_ptr(), _stream())
        return (out,)

    return _scene(_pick(b, ["x", "beta"]), run, status=lambda: prob.sweep_status(_stream()))


def _api_residuals(fresh=False):
    e, b = env(), _body()
    torch = e.torch
    prob = _kept_problem(False)

    def run(t):
        r = torch.empty(prob.layout.total_rows, dtype=torch.float64, device="cuda")
        comp = torch.zeros(F, dtype=torch.int32, device="cuda")
        prob.residuals_device(t["x"].data_ptr(), t["beta"].data_ptr(), r.data_ptr(), comp.data_ptr(), False, _stream())
        return r, comp

    return _scene(_pick(b, ["x", "beta"]), run)


def _api_overlay(fresh=False):
    e, b = env(), _body()
    torch = e.torch
    H, W = SIZE
    key = "overlay"
    if key not in e.kept:
        e.kept[key] = e.api.Overlay(e.synth.make_faces(e.model), b.V, W, H, max_frames=F)
    ov = e.kept[key]
    intr = e.synth.camera_intrinsics(W, H)
    rng = np.random.default_rng(14)
    with torch.no_grad():
        clouds = [e.layer(e.dev(x), e.dev(be))[0].contiguous() for x, be in zip(b.pairs["x"], b.pairs["beta"])]
    frames = [rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8) for _ in range(2)]

    def run(t):
        images = t["frames"].clone()                 # (drawn in place)
        ov.render_device(t["cloud"].data_ptr(), False, 3 * b.V, F, images.data_ptr(), intr, stream=_stream())
        return (images,)

    return _scene(dict(cloud=tuple(clouds), frames=tuple(frames)), run)


# ---- scan ------------------------------------------------------------------------------------------------------------------------
def _closest_points(backward):
    def build(fresh=False):
        e, m = env(), _mesh()
        if fresh:
            _fresh_cache("_closest_handles", lambda: e.common._closest_handle(0))

        def run(t):
            if not backward:
                return e.tl.closest_points(t["points"], t["verts"])
            wrt = (_leaf(t["points"]), _leaf(t["verts"]))
            dist2, _ = e.tl.closest_points(*wrt)
            return e.torch.autograd.grad(dist2, wrt, t["g_rows"])

        return _scene(_pick(m, ["points", "verts"] + (["g_rows"] if backward else [])), run,
                      close=(lambda: _fresh_cache("_closest_handles")) if fresh else None)
    return build


def _closest_surface(oriented, backward):
    def build(fresh=False):
        e, m = env(), _mesh()
        if fresh:
            _fresh_cache("_surface_handles", lambda: e.common._surface_handle(0, m.V, m.faces))
        names = ["points", "verts"] + (["point_normals"] if oriented else []) + (["g_rows"] if backward else [])

        def run(t):
            kw = dict(point_normals=t["point_normals"], min_cos=0.2) if oriented else {}
            if not backward:
                return e.tl.closest_surface(t["points"], t["verts"], m.faces, **kw)
            wrt = (_leaf(t["points"]), _leaf(t["verts"]))
            dist2, _, _ = e.tl.closest_surface(wrt[0], wrt[1], m.faces, **kw)
            return e.torch.autograd.grad(dist2, wrt, t["g_rows"])

        return _scene(_pick(m, names), run, close=(lambda: _fresh_cache("_surface_handles")) if fresh else None)
    return build


def _surface_gram(fresh=False):
    e, m = env(), _mesh()
    rng = np.random.default_rng(15)
    P = 7
    found = []
    with e.torch.no_grad():
        for k in (0, 1):           # the correspondences of the real and of the stale pose: both in range
            _, index, bary = e.tl.closest_surface(e.dev(m.pairs["points"][k]), e.dev(m.pairs["verts"][k]), m.faces)
            found.append((index, bary))
    N = found[0][0].shape[0]
    pairs = dict(points=m.pairs["points"], index=(found[0][0], found[1][0]), bary=(found[0][1], found[1][1]),
                 jac=(_f32(rng, (F, P, m.V, 3)), _f32(rng, (F, P, m.V, 3))),
                 weight=(rng.uniform(0.5, 1.5, N).astype(np.float32), rng.uniform(0.5, 1.5, N).astype(np.float32)),
                 direction=(_unit(rng, (N, 3)), _unit(rng, (N, 3))), rhs=(_f32(rng, (F, m.V, 3)), _f32(rng, (F, m.V, 3))))

    # a handle of the row's own, which no search has used: a search whose verts required grad keeps the grouping of ITS index
    # tensor in the handle by address, and torch's allocator may hand that address to one of this row's index tensors
    if "gram_surface" not in e.kept:
        e.kept["gram_surface"] = e.api.Surface(0, m.V, m.faces)
    surface = e.kept["gram_surface"]

    def run(t):
        return e.tl.surface_gram(t["jac"], t["points"], t["index"], t["bary"], surface, weight=t["weight"], direction=t["direction"],
                                 rhs=t["rhs"])

    return _scene(pairs, run)


# ---- one builder for the rows that are a function call (and a backward) on the mesh scene -----------------------------------------
def _mesh_row(names, call, wrt=(), grad=None, out=0, fresh_cache=None, make=None):
    """call(e, m, t) -> the outputs, t the row's tensors with those named in `wrt` as leaves; with grad (the name of the upstream
    gradient of output `out`): (that output, the gradients in `wrt`)"""
    def build(fresh=False):
        e, m = env(), _mesh()
        if fresh:
            _fresh_cache(fresh_cache, lambda: make(e, m))

        def run(t):
            if grad is None:
                res = call(e, m, t)
                return res if isinstance(res, (tuple, list)) else (res,)
            t = dict(t)
            for k in wrt:
                t[k] = _leaf(t[k])
            res = call(e, m, t)
            y = res[out] if isinstance(res, (tuple, list)) else res
            return (y.detach(),) + e.torch.autograd.grad(y, [t[k] for k in wrt], t[grad])

        return _scene(_pick(m, list(names)), run, close=(lambda: _fresh_cache(fresh_cache)) if fresh else None)
    return build


@functools.lru_cache(maxsize=None)
def _atlas():
    """the texture rows' host data: the "charts" atlas of the two spheres' faces and 16 x 16 textures"""
    import texture_ref as tr
    e, m = env(), _mesh()
    uv, uv_faces = e.synth.make_uv_atlas(m.faces, "charts")
    rng = np.random.default_rng(16)
    stale_uv = np.clip(uv + _f32(rng, uv.shape, 0.01), 0.0, 1.0).astype(np.float32)
    return types.SimpleNamespace(uv_faces=uv_faces, pairs=dict(uv=(uv, stale_uv), tex=(tr.make_texture(16, 16, 3, 1, 0),
                                                                                        tr.make_texture(16, 16, 3, 1, 1))))


def _texture(mip, backward):
    def build(fresh=False):
        e, m, a = env(), _mesh(), _atlas()
        render = e.texture.render_texture_mip if mip else e.tl.render_texture
        pairs = dict(_pick(m, ["verts"] + (["g_image"] if backward else [])), **a.pairs)

        def run(t):
            if not backward:
                return render(t["verts"], m.faces, INTR, SIZE, t["uv"], a.uv_faces, t["tex"], interior=True)
            wrt = (_leaf(t["tex"]), _leaf(t["uv"]), _leaf(t["verts"]))
            image, _ = render(wrt[2], m.faces, INTR, SIZE, wrt[1], a.uv_faces, wrt[0], interior=True)
            return (image.detach(),) + e.torch.autograd.grad(image, wrt, t["g_image"])

        return _scene(pairs, run)
    return build


# ---- volume ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _volumes():
    import edt3_ref
    import extract_ref
    import tsdf_ref
    rng = np.random.default_rng(17)
    nx, ny, nz = DIMS
    v = types.SimpleNamespace()
    v.sphere = extract_ref.make_volume("sphere", DIMS)
    other = extract_ref.make_volume("iso", DIMS).vol            # standard normal: another valid volume
    lo = np.asarray(v.sphere.origin)
    ext = np.asarray(v.sphere.spacing) * (np.array(DIMS) - 1)
    inside = lambda: (lo + ext * rng.uniform(0.02, 0.98, (F, 41, 3))).astype(np.float32)
    v.cases = [tsdf_ref.random_case(DIMS, SIZE, seed) for seed in (0, 1)]
    v.pairs = dict(volume=(v.sphere.vol, other), points=(inside(), inside()), g_value=(_f32(rng, (F, 41)), _f32(rng, (F, 41))),
                   depth=tuple(c.depth for c in v.cases), pose=tuple(tsdf_ref.pose_array(c) for c in v.cases),
                   seed=tuple(edt3_ref.make_mask("random_0.05", (nz, ny, nx), seed=s) for s in (0, 1)))
    return v


def _volume_row(names, call, wrt=(), grad=None, lazy_cache=None):
    def build(fresh=False):
        e, v = env(), _volumes()
        if fresh:
            _fresh_cache(lazy_cache, lambda: e.common._volume_handle(0, DIMS, v.sphere.origin, v.sphere.spacing))

        def run(t):
            if grad is None:
                return call(e, v, t)
            t = dict(t)
            for k in wrt:
                t[k] = _leaf(t[k])
            value, valid = call(e, v, t)
            return (value.detach(), valid) + e.torch.autograd.grad(value, [t[k] for k in wrt], t[grad])

        return _scene(_pick(v, list(names)), run, close=(lambda: _fresh_cache(lazy_cache)) if fresh else None)
    return build


def _sample_volume(e, v, t):
    return e.volume.sample_volume(t["volume"], v.sphere.origin, v.sphere.spacing, t["points"])


def _integrate(e, v, t):
    c = v.cases[0]
    return e.volume.integrate_tsdf(t["depth"], c.intr, c.origin, c.spacing, c.dims, c.trunc, pose=t["pose"], z_near=c.z_near)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _distance_transform(fresh=False):
    import edt_ref
    e = env()
    masks = tuple(np.stack([edt_ref.make_mask("random_0.05", SIZE, seed=s + f) for f in range(F)]) for s in (0, 10))
    return _scene(dict(mask=masks), lambda t: e.tl.distance_transform(t["mask"]))


TABLE = [
    # smpl
    Row("smpl_forward", _smpl("forward"), ["bodyfit_forward_device", "SMPLLayer"]),
    Row("smpl_forward_offsets", _smpl("forward", "shared"), ["bodyfit_forward_offsets_device", "SMPLLayer"]),
    Row("smpl_backward", _smpl("backward"), ["bodyfit_forward_vjp_device", "SMPLLayer"], lazy="problem"),
    Row("smpl_backward_offsets", _smpl("backward", "frames"), ["bodyfit_forward_offsets_vjp_device", "SMPLLayer"], lazy="problem"),
    Row("smpl_jvp", _smpl("jvp"), ["bodyfit_forward_jvp_device", "SMPLLayer"], lazy="problem"),
    Row("smpl_jvp_offsets", _smpl("jvp", "shared"), ["bodyfit_forward_offsets_jvp_device", "SMPLLayer"], lazy="problem"),
    Row("smpl_jacobian", _smpl("jacobian"), ["bodyfit_forward_jvp_device", "SMPLLayer"]),
    Row("fit_objective_forward", _objective("forward"), ["bodyfit_residuals_device", "FitObjective"], lazy="problem"),
    Row("fit_objective_backward", _objective("backward"), ["bodyfit_residuals_device", "bodyfit_residual_vjp_device", "FitObjective"],
        lazy="problem"),
    # scan
    Row("closest_points", _closest_points(False), ["bodyfit_closest_points_device", "closest_points"], lazy="closest"),
    Row("closest_points_backward", _closest_points(True), ["bodyfit_closest_points_vjp_device", "closest_points"]),
    Row("closest_surface", _closest_surface(False, False), ["bodyfit_closest_surface_device", "closest_surface"], lazy="surface"),
    Row("closest_surface_oriented", _closest_surface(True, False), ["bodyfit_closest_surface_oriented_device", "closest_surface"]),
    Row("closest_surface_backward", _closest_surface(False, True), ["bodyfit_closest_surface_vjp_device", "closest_surface"]),
    Row("closest_surface_oriented_backward", _closest_surface(True, True),
        ["bodyfit_closest_surface_oriented_device", "bodyfit_closest_surface_vjp_device", "closest_surface"]),
    Row("surface_gram", _surface_gram, ["bodyfit_surface_gram_device", "surface_gram"]),
    # solid
    Row("winding_number", _mesh_row(["points", "verts", "skip_vertex"], lambda e, m, t: e.tl.winding_number(
        t["points"], t["verts"], m.faces, skip_vertex=t["skip_vertex"])), ["bodyfit_surface_winding_device", "winding_number"]),
    Row("vertex_winding", _mesh_row(["verts"], lambda e, m, t: e.tl.vertex_winding(t["verts"], m.faces)),
        ["bodyfit_surface_winding_device", "vertex_winding"]),
    Row("vertex_normals", _mesh_row(["verts"], lambda e, m, t: e.tl.vertex_normals(t["verts"], m.faces)),
        ["bodyfit_surface_vertex_normals_device", "vertex_normals"]),
    Row("signed_distance", _mesh_row(["points", "verts"], lambda e, m, t: e.tl.signed_distance(t["points"], t["verts"], m.faces)),
        ["bodyfit_closest_surface_device", "bodyfit_surface_winding_device", "signed_distance"]),
    Row("mesh_laplacian", _mesh_row(["field"], lambda e, m, t: e.tl.mesh_laplacian(t["field"], m.faces)),
        ["bodyfit_surface_laplacian_device", "mesh_laplacian"]),
    Row("mesh_laplacian_transpose", _mesh_row(["field", "g_field"], lambda e, m, t: e.tl.mesh_laplacian(t["field"], m.faces),
                                              wrt=["field"], grad="g_field"), ["bodyfit_surface_laplacian_device", "mesh_laplacian"]),
    # depth
    Row("render_depth", _mesh_row(["verts"], lambda e, m, t: e.tl.render_depth(t["verts"], m.faces, INTR, SIZE),
                                  fresh_cache="_raster_handles", make=lambda e, m: e.common._raster_handle(0, m.V, m.faces, SIZE)),
        ["bodyfit_raster_render_device", "render_depth"], RENDER, lazy="raster"),
    Row("visible_vertices", _mesh_row(["verts"], lambda e, m, t: e.tl.visible_vertices(t["verts"], m.faces, INTR, SIZE)),
        ["bodyfit_raster_render_device", "bodyfit_raster_visibility_device", "visible_vertices"], RENDER),
    Row("depth_at_pixels", _mesh_row(["verts"], lambda e, m, t: e.tl.depth_at_pixels(t["verts"], m.faces, INTR, SIZE)),
        ["bodyfit_raster_depth_rows_device", "depth_at_pixels"], RENDER),
    Row("depth_at_pixels_backward", _mesh_row(["verts", "g_pixels"], lambda e, m, t: e.tl.depth_at_pixels(t["verts"], m.faces, INTR, SIZE),
                                              wrt=["verts"], grad="g_pixels"),
        ["bodyfit_raster_depth_rows_device", "bodyfit_surface_rows_vjp_device", "depth_at_pixels"], RENDER),
    # silhouette
    Row("distance_transform", _distance_transform, ["bodyfit_raster_distance_device", "distance_transform"]),
    Row("edge_weights", _mesh_row(["verts"], lambda e, m, t: e.tl.edge_weights(t["verts"], m.faces, INTR, SIZE)),
        ["bodyfit_raster_edges_device", "edge_weights"], RENDER),
    Row("antialias", _mesh_row(["image", "verts"], lambda e, m, t: e.tl.antialias(t["image"], t["verts"], m.faces, INTR)),
        ["bodyfit_raster_edges_device", "bodyfit_raster_edge_blend_device", "antialias"], RENDER),
    Row("antialias_backward", _mesh_row(["image", "verts", "g_image"], lambda e, m, t: e.tl.antialias(t["image"], t["verts"], m.faces, INTR),
                                        wrt=["image", "verts"], grad="g_image"),
        ["bodyfit_raster_edge_blend_device", "bodyfit_raster_edge_rows_device", "bodyfit_surface_rows_vjp_device", "antialias"], NONZERO),
    # appearance
    Row("render_attributes", _mesh_row(["verts", "attr"], lambda e, m, t: e.tl.render_attributes(
        t["verts"], m.faces, INTR, SIZE, t["attr"], interior=True)), ["bodyfit_raster_shade_device", "render_attributes"], RENDER),
    Row("render_attributes_backward", _mesh_row(["verts", "attr", "g_image"], lambda e, m, t: e.tl.render_attributes(
        t["verts"], m.faces, INTR, SIZE, t["attr"], interior=True), wrt=["attr", "verts"], grad="g_image"),
        ["bodyfit_raster_interp_rows_device", "bodyfit_surface_rows_vjp_device", "render_attributes"], NONZERO),
    Row("sample_images", _mesh_row(["image", "verts"], lambda e, m, t: e.tl.sample_images(t["image"], t["verts"], INTR)),
        ["bodyfit_raster_sample_device", "sample_images"]),
    Row("sample_images_backward", _mesh_row(["image", "verts", "g_field"], lambda e, m, t: e.tl.sample_images(t["image"], t["verts"], INTR),
                                            wrt=["verts"], grad="g_field"), ["bodyfit_raster_sample_device", "sample_images"]),
    # texture
    Row("render_texture", _texture(False, False), ["bodyfit_raster_texture_device", "render_texture"], RENDER),
    Row("render_texture_backward", _texture(False, True),
        ["bodyfit_raster_texture_grad_device", "bodyfit_raster_interp_rows_indexed_device", "render_texture"], NONZERO),
    Row("render_texture_mip", _texture(True, False),
        ["bodyfit_raster_texture_mip_build_device", "bodyfit_raster_texture_mip_device", "texture.render_texture_mip"], RENDER),
    Row("render_texture_mip_backward", _texture(True, True), ["bodyfit_raster_texture_mip_grad_device", "texture.render_texture_mip"],
        NONZERO),
    # lighting
    Row("lighting_vertex_normals", _mesh_row(["verts"], lambda e, m, t: e.lighting.vertex_normals(t["verts"], m.faces)),
        ["bodyfit_surface_vertex_normals_device", "lighting.vertex_normals"]),
    Row("lighting_vertex_normals_backward", _mesh_row(["verts", "g_field"], lambda e, m, t: e.lighting.vertex_normals(t["verts"], m.faces),
                                                      wrt=["verts"], grad="g_field"),
        ["bodyfit_surface_vertex_normals_vjp_device", "lighting.vertex_normals"]),
    Row("lighting_shade", _mesh_row(["image", "verts", "light"], lambda e, m, t: e.lighting.shade(
        t["image"], t["verts"], m.faces, INTR, t["light"], interior=True)), ["bodyfit_raster_light_device", "lighting.shade"], RENDER),
    Row("lighting_shade_backward", _mesh_row(["image", "verts", "light", "g_image"], lambda e, m, t: e.lighting.shade(
        t["image"], t["verts"], m.faces, INTR, t["light"], interior=True), wrt=["image", "light", "verts"], grad="g_image"),
        ["bodyfit_raster_light_grad_device", "bodyfit_raster_shade_device", "lighting.shade"], NONZERO),
    # volume
    # (the volume handle owns nothing on the device, so its first use makes no device state: the row is in check (c) as the
    # one row of its handle kind, and shows that the first call on a new handle is on the caller's stream like every other)
    Row("sample_volume", _volume_row(["volume", "points"], _sample_volume, lazy_cache="_volume_handles"),
        ["bodyfit_volume_sample_device", "volume.sample_volume"], lazy="volume"),
    Row("sample_volume_backward", _volume_row(["volume", "points", "g_value"], _sample_volume, wrt=["points"], grad="g_value"),
        ["bodyfit_volume_sample_device", "volume.sample_volume"]),
    Row("integrate_tsdf", _volume_row(["depth", "pose"], _integrate), ["bodyfit_volume_integrate_device", "volume.integrate_tsdf"]),
    Row("extract_surface", _volume_row(["volume"], lambda e, v, t: e.volume.extract_surface(t["volume"], v.sphere.origin, v.sphere.spacing)),
        ["bodyfit_volume_surface_count_device", "bodyfit_volume_surface_emit_device", "volume.extract_surface"],
        "the read of the totals that size the outputs, between the counting and the emitting launches"),
    Row("volume_distance_transform", _volume_row(["seed"], lambda e, v, t: e.volume.distance_transform(t["seed"])),
        ["bodyfit_volume_distance_device", "volume.distance_transform"]),
    # the api level
    Row("api_evaluate_reduce", _api_evaluate, ["bodyfit_evaluate_device", "bodyfit_reduce_shared_device"]),
    Row("api_residuals", _api_residuals, ["bodyfit_residuals_device"]),
    Row("api_overlay_render", _api_overlay, ["bodyfit_overlay_render_device"],
        "one 8-byte read-back that sizes the tile lists"),
]


BY_NAME = {r.name: r for r in TABLE}

# every other bodyfit_*_device export, and every other public callable of the torch layer's recorded surface that launches device
# work, with the reason it has no row
EXCLUDED = {
    "huber_rho": "plain torch arithmetic on the caller's tensors: it launches nothing of the library's",
    "fuse_vertex_colours": "a composition of the visible_vertices, vertex_normals and sample_images rows, with torch in between",
    "bake_texture": "a composition of the render_depth and render_texture_backward rows (one texture_grad launch), with torch in between",
    "OffsetRegulariser": "a sum over the mesh_laplacian row",
}
for _name in ("CoverageTerm", "DepthMapTerm", "DepthResidualTerm", "PhotometricTerm", "PointCloudTerm", "RenderedPhotometricTerm",
              "SelfPenetrationTerm", "SilhouetteTerm", "SurfaceTerm", "TexturedPhotometricTerm"):
    EXCLUDED[_name] = "a composed term: a sum over the primitives that have rows"
del _name
