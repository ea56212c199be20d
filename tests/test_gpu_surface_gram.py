"""GPU: the Gauss-Newton normal equations of the scan terms (bodyfit_surface_gram_device, k_surface_gram.hip),
torch_layer.surface_gram and SurfaceTerm / PointCloudTerm.normal_equations.

The raw kernel is checked against the numpy f64 reference of its contract (gram_ref.py) with the bounds the header derives,
|H - H*| <= 2^-12 H^ and |g - g*| <= 2^-32 g^, elementwise.  The layer is checked against the dense path (layer.jacobian, a
gather and an einsum in f64) within the same bound, and g against the reverse-mode gradient of the same cost within the bound
of test_gpu_forward_jvp.test_adjoint_identity_with_the_vjp (1e-4 of the largest entry times the absolute sum, on either side)."""
import importlib

import numpy as np
import pytest

import gram_ref
import model_variants as mv
from test_gpu_forward_jvp import gn_start

pytestmark = pytest.mark.gpu

ADJOINT_TOL = 1e-4       # test_adjoint_identity_with_the_vjp: the cloud tangent's and the VJP's relative bound


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def tl():
    return importlib.import_module("3dbodyanimation_amd.torch_layer")


_models: dict = {}


def _gmv(api, v):
    if v.id not in _models:
        _models[v.id] = api.Model(v.model, pose_blend_data=v.pose_blend_data)
    return _models[v.id]


# ---- the raw kernel -------------------------------------------------------------------------------------------------------
def _soup(V, rng):
    """a face soup with a shared edge, a degenerate face and an unreferenced vertex (the last one)"""
    if V == 3:
        return np.array([[0, 1, 1], [1, 0, 0], [0, 0, 1]], np.int32)
    f = rng.integers(0, V - 1, size=(2 * V, 3)).astype(np.int32)
    f[0] = [0, 1, 2]; f[1] = [2, 1, 3]; f[2] = [4, 4, 5]
    return f


def _case(V, P, F, ragged, plane, seed=0):
    rng = np.random.default_rng(1000 * V + 10 * P + F + (5 if ragged else 0) + seed)
    faces = _soup(V, np.random.default_rng(V))             # one topology per V: the tests keep one handle for it
    nf = len(faces)
    if ragged:
        counts = [150 + 37 * f for f in range(F)]
        if F > 1:
            counts[1] = 0                                  # an empty frame
        offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        n, N = 0, int(offset[-1])
    else:
        offset, n = None, 171
        N = F * n
    rows = gram_ref.frame_rows(F, n, offset)
    index = rng.integers(0, nf, size=N).astype(np.int32)
    for r0, r1 in rows:
        if r1 - r0 >= 150:
            index[r0:r0 + 64] = 0                          # exactly 64 rows on face 0: the last count without the partial-sum rule
            index[r0 + 64:r0 + 64 + 70] = 1                # 70 on face 1: the wave's 64 partial sums
            index[r0 + 134:r0 + 140] = -1                  # rows without a counterpart
            index[r0 + 140] = nf                           # out of range
    bary = rng.dirichlet(np.ones(3), size=N).astype(np.float32)
    bary[::7] = [1.0, 0.0, 0.0]
    weight = rng.uniform(0.1, 2.0, size=N).astype(np.float32)
    weight[rng.random(N) < 0.15] = 0.0
    d = rng.normal(size=(N, 3))
    direction = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32) if plane else None
    jac = (rng.normal(size=(F, P, V, 3)) * rng.uniform(0.01, 2.0, size=(F, P, 1, 1))).astype(np.float32)
    rhs = rng.normal(scale=0.01, size=(F, V, 3)).astype(np.float32)
    return dict(V=V, P=P, F=F, faces=faces, offset=offset, n=n, N=N, rows=rows, index=index, bary=bary, weight=weight,
                direction=direction, jac=jac, rhs=rhs)


def _frame_of(c, f):
    """frame f of case c as a one-frame case"""
    r0, r1 = c["rows"][f]
    o = dict(c, F=1, N=r1 - r0, rows=[(0, r1 - r0)], index=c["index"][r0:r1], bary=c["bary"][r0:r1],
             weight=c["weight"][r0:r1], direction=None if c["direction"] is None else c["direction"][r0:r1],
             jac=c["jac"][f:f + 1], rhs=c["rhs"][f:f + 1])
    if c["offset"] is not None:
        o["offset"] = np.array([0, r1 - r0], np.int32)
    return o


def _run(api, torch, handle, c, use_weight=True, pad=True, index_dev=None):
    """bodyfit_surface_gram_device on case c through the ctypes binding: the Jacobian rows with NaN behind their 3 V floats and
    frames farther apart than P rows (pad), the right-hand side with a frame stride of its own.  -> (H, g) numpy"""
    F, P, V, N = c["F"], c["P"], c["V"], c["N"]
    dev = "cuda"
    row = 3 * V + (5 if pad else 0)
    frame = (P + (1 if pad else 0)) * row + (3 if pad else 0)
    jbuf = torch.full((F * frame + 8,), float("nan"), dtype=torch.float32, device=dev)
    jview = torch.as_strided(jbuf, (F, P, 3 * V), (frame, row, 1))
    jview.copy_(torch.tensor(c["jac"].reshape(F, P, 3 * V), device=dev))
    rstride = 3 * V + (7 if pad else 0)
    rbuf = torch.full((F * rstride + 8,), float("nan"), dtype=torch.float32, device=dev)
    torch.as_strided(rbuf, (F, 3 * V), (rstride, 1)).copy_(torch.tensor(c["rhs"].reshape(F, 3 * V), device=dev))
    pts = torch.zeros((max(N, 1), 3), dtype=torch.float32, device=dev)
    keep = [pts]
    if c["offset"] is not None:
        off = torch.tensor(c["offset"], device=dev)
        keep.append(off)
        ps = api.PointSet.ragged(pts.data_ptr(), off.data_ptr())
    else:
        ps = api.PointSet.uniform(pts.data_ptr(), c["n"])
    index = index_dev if index_dev is not None else torch.tensor(c["index"], device=dev)
    bary = torch.tensor(c["bary"], device=dev)
    weight = torch.tensor(c["weight"], device=dev) if use_weight else None
    direction = torch.tensor(c["direction"], device=dev) if c["direction"] is not None else None
    H = torch.full((F, P, P), float("nan"), dtype=torch.float64, device=dev)
    g = torch.full((F, P), float("nan"), dtype=torch.float64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else (None if t is None else pts.data_ptr())
    handle.gram_device(ps, F, N, ptr(index), ptr(bary), ptr(weight), ptr(direction), jbuf.data_ptr(), P, row, frame,
                       rbuf.data_ptr(), rstride, H.data_ptr(), g.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return H.cpu().numpy(), g.cpu().numpy()


def _assert_contract(c, H, g, use_weight, what):
    Hr, Hh, gr, gh = gram_ref.gram_reference(c["jac"], c["faces"], c["rows"], c["index"], c["bary"],
                                             c["weight"] if use_weight else None, c["direction"], c["rhs"])
    assert np.isfinite(H).all() and np.isfinite(g).all(), what
    ratio_h = float((np.abs(H - Hr) / np.maximum(Hh, 1e-300)).max())
    ratio_g = float((np.abs(g - gr) / np.maximum(gh, 1e-300)).max())
    print(f"gram {what}: max |H - H*| / H^ = {ratio_h:.3e} (eps {gram_ref.EPS_H:.3e}), max |g - g*| / g^ = {ratio_g:.3e} "
          f"(eps {gram_ref.EPS_G:.3e})")
    assert np.all(np.abs(H - Hr) <= gram_ref.EPS_H * Hh), (what, ratio_h)
    assert np.all(np.abs(g - gr) <= gram_ref.EPS_G * gh), (what, ratio_g)
    assert np.array_equal(H, H.transpose(0, 2, 1)), what                                   # exactly symmetric
    for f, (r0, r1) in enumerate(c["rows"]):
        if r1 == r0:
            assert not H[f].any(), what                                                    # an empty frame: exact zeros


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("V", [3, 50, 257])
def test_kernel_against_the_reference(api, torch, V, plane):
    handle = None
    for P in (1, 31, 32, 33, 86, 96):
        for F in (1, 3):
            for ragged in (False, True):
                c = _case(V, P, F, ragged, plane)
                if handle is None:
                    handle = api.Surface(0, V, c["faces"])
                H, g = _run(api, torch, handle, c)
                _assert_contract(c, H, g, True, f"V={V} P={P} F={F} ragged={ragged} plane={plane}")
    c = _case(V, 33, 3, True, plane)                       # no weights: w = 1
    H, g = _run(api, torch, handle, c, use_weight=False, pad=False)
    _assert_contract(c, H, g, False, f"V={V} unweighted")


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_bit_level_properties(api, torch, tl, plane):
    V, P, F = 257, 86, 3
    c = _case(V, P, F, True, plane, seed=1)
    handle = api.Surface(0, V, c["faces"])
    H1, g1 = _run(api, torch, handle, c)
    H2, g2 = _run(api, torch, handle, c)
    assert np.array_equal(H1, H2) and np.array_equal(g1, g2)                               # two runs
    Hn, gn = _run(api, torch, handle, c, pad=False)
    assert np.array_equal(H1, Hn) and np.array_equal(g1, gn)                               # whatever the strides
    for f in range(F):                                                                     # a frame alone
        Hf, gf = _run(api, torch, handle, _frame_of(c, f))
        assert np.array_equal(Hf[0], H1[f]) and np.array_equal(gf[0], g1[f]), f
    cu = _case(V, P, F, False, plane, seed=2)
    Hu, _ = _run(api, torch, handle, cu)
    for f in range(F):
        Hf, _ = _run(api, torch, handle, _frame_of(cu, f))
        assert np.array_equal(Hf[0], Hu[f]), f
    # a frame in the second group of sixteen (the kernel's workspace holds one group) equals the frame alone
    c18 = _case(50, 33, 18, False, plane, seed=3)
    h50 = api.Surface(0, 50, c18["faces"])
    H18, _ = _run(api, torch, h50, c18)
    H17, _ = _run(api, torch, h50, _frame_of(c18, 17))
    assert np.array_equal(H17[0], H18[17])
    # the grouping a search kept in the handle against the one rebuilt inside the call
    rng = np.random.default_rng(9)
    verts = torch.tensor(rng.normal(size=(F, V, 3)).astype(np.float32), device="cuda")
    pts = torch.tensor(rng.normal(size=(c["N"], 3)).astype(np.float32), device="cuda")
    off = torch.tensor(c["offset"], device="cuda")
    ps = api.PointSet.ragged(pts.data_ptr(), off.data_ptr())
    dist2 = torch.empty(c["N"], dtype=torch.float32, device="cuda")
    index = torch.empty(c["N"], dtype=torch.int32, device="cuda")
    bary = torch.empty((c["N"], 3), dtype=torch.float32, device="cuda")
    handle.closest_device(ps, verts.data_ptr(), 3 * V, F, c["N"], dist2.data_ptr(), index.data_ptr(), bary.data_ptr(),
                          torch.cuda.current_stream().cuda_stream, prepare_vjp=True)
    torch.cuda.synchronize()
    cs = dict(c, index=index.cpu().numpy(), bary=bary.cpu().numpy())
    jac = torch.tensor(c["jac"], device="cuda")
    w = torch.tensor(c["weight"], device="cuda")
    d = torch.tensor(c["direction"], device="cuda") if plane else None
    Hk, _ = tl.surface_gram(jac, pts, index, bary, handle, query_offset=off, weight=w, direction=d)          # kept
    Hb, _ = tl.surface_gram(jac, pts, index.clone(), bary, handle, query_offset=off, weight=w, direction=d)  # rebuilt
    assert torch.equal(Hk, Hb)
    Hraw, _ = _run(api, torch, handle, cs)                                                 # the layer call = the raw call
    assert np.array_equal(Hk.cpu().numpy(), Hraw)
    # surface_gram on views: rows and frames farther apart than 3 V and P rows, with NaN between them, are used in place;
    # a view whose [V, 3] blocks are not dense, or whose rows overlap, is copied: the same bits either way
    kw = dict(query_offset=off, weight=w, direction=d)
    wide = torch.full((F, P + 2, V + 3, 3), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :P, :V] = jac
    view = torch.as_strided(wide, (F, P, V, 3), wide.stride())
    assert view.stride(1) > 3 * V and view.stride(0) > P * view.stride(1) and not view.is_contiguous()
    assert torch.equal(tl.surface_gram(view, pts, index, bary, handle, **kw)[0], Hk)
    assert torch.equal(tl.surface_gram(view[:1], pts[:c["offset"][1]], index[:c["offset"][1]], bary[:c["offset"][1]], handle,
                                       query_offset=off[:2], weight=w[:c["offset"][1]],
                                       direction=d[:c["offset"][1]] if plane else None)[0], Hk[:1])   # F = 1: any frame stride
    swapped = jac.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)                     # [V, 3] blocks not dense
    assert swapped.stride(3) != 1
    assert torch.equal(tl.surface_gram(swapped, pts, index, bary, handle, **kw)[0], Hk)
    one = jac[:, :1].expand(F, P, V, 3)                                                    # tangent rows on top of each other
    H1 = tl.surface_gram(one, pts, index, bary, handle, **kw)[0]
    assert torch.equal(H1, tl.surface_gram(one.contiguous(), pts, index, bary, handle, **kw)[0])


def test_error_codes(api, torch):
    lib = api.load_library()
    V, P, F, n = 5, 3, 2, 4
    handle = api.Surface(0, V, np.array([[0, 1, 2], [2, 3, 4]], np.int32))
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    ps = api.PointSet.uniform(p, n)
    import ctypes as C
    call = lib.bodyfit_surface_gram_device
    row, frame = 3 * V, P * 3 * V

    def gram(h=handle.h, s=C.byref(ps), nF=F, idx=p, bary=p, w=None, d=None, jac=p, nP=P, row_=row, frame_=frame, rhs=p,
             rstride=3 * V, H=p, g=p):
        return call(h, s, nF, F * n, idx, bary, w, d, jac, nP, row_, frame_, rhs, rstride, H, g, None)

    assert gram() == 0
    torch.cuda.synchronize()
    assert gram(h=None) == 1                       # NULL handle
    assert gram(s=None) == 1                       # NULL set
    assert gram(idx=None) == 1                     # NULL index
    assert gram(bary=None) == 1                    # NULL bary
    assert gram(jac=None) == 1                     # NULL jac
    assert gram(H=None) == 1                       # NULL H
    assert gram(nP=0) == 1                         # n_tangents < 1
    assert gram(row_=3 * V - 1) == 1               # row_floats < 3 V
    assert gram(frame_=frame - 1) == 1             # frames closer than P rows
    assert gram(rstride=3 * V - 1) == 1            # rhs frames closer than 3 V
    assert gram(rhs=None) == 1                     # d_g without d_rhs
    assert gram(nF=-1) == 1
    big = api.Surface(0, 6000, np.zeros((0, 3), np.int32))
    assert gram(h=big.h, nP=4096, row_=18000, frame_=4096 * 18000, rstride=18000) == 1   # 2^31 bytes of partial panels a frame
    assert gram(rhs=None, g=None) == 0             # H alone
    assert gram(nF=0) == 0                         # zero frames: a no-op
    torch.cuda.synchronize()
    assert b"bodyfit_surface_gram_device" in lib.bodyfit_last_error()


# ---- the layer against the dense path ---------------------------------------------------------------------------------------
def _rotations(synth, F):
    """a distinct root orientation per frame"""
    return np.stack([synth.rodrigues(np.array([0.11 * f, -0.07 * f, 0.2 + 0.05 * f])) for f in range(F)])


def _scene(api, torch, tl, synth, vid, F, per_frame, n_per_frame, seed, noise=0.002, outliers=8, R0=None, step=20):
    """a layer on variant vid, parameters, and scan points sampled on the posed surface (+ noise, + a few far outliers)"""
    v = mv.get(vid)
    layer = tl.SMPLLayer(_gmv(api, v), R0=R0, beta_per_frame=per_frame)
    rng = np.random.default_rng(seed)
    x = mv.random_params(rng, v, F, pose_sigma=0.2)
    beta = rng.normal(size=(F, v.n_shape)) if per_frame else rng.normal(size=v.n_shape)
    V = v.model.n_verts
    faces = synth.make_faces(v.model, n_faces=2 * V - 4)
    xt, bt = torch.tensor(x, device="cuda"), torch.tensor(beta, device="cuda")
    with torch.no_grad():
        verts = layer(xt, bt)[0].cpu().numpy().astype(np.float64)
    pts, counts = [], []
    for f in range(F):
        n = n_per_frame - step * f
        t = rng.integers(0, len(faces), size=n)
        b = rng.dirichlet(np.ones(3), size=n)
        p = np.einsum("na,nax->nx", b, verts[f][faces[t]]) + rng.normal(scale=noise, size=(n, 3))
        p[:outliers] += 0.3
        pts.append(p); counts.append(n)
    points = torch.tensor(np.concatenate(pts).astype(np.float32), device="cuda")
    offset = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device="cuda")
    return v, layer, xt, bt, points, offset, faces


def _frames(torch, offset, N):
    off = offset.long()
    return torch.repeat_interleave(torch.arange(off.shape[0] - 1, device=offset.device), off[1:] - off[:-1], output_size=N)


def _plane_geometry(torch, verts, faces_t, frame, index, bary, points):
    """(d [N, 3] f64 from the f32 direction, flat [N], c [N, 3]) as SurfaceTerm's plane mode forms them"""
    ids = faces_t[index.clamp(min=0).long()]
    corners = verts[frame[:, None], ids].double()
    nrm = torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    length = nrm.norm(dim=1)
    flat = ~(length > 1e-30)
    d = torch.where(flat[:, None], torch.zeros_like(nrm), nrm / length.clamp(min=1e-30)[:, None])
    c = (bary.double()[:, :, None] * corners).sum(dim=1)
    return d, flat, c, ids


def _dense_surface(torch, tl, layer, x, b, points, offset, faces, trunc, mode):
    """the dense path: layer.jacobian, a gather of the corner rows and einsums in f64 -> cost, g, H, H^"""
    with torch.no_grad():
        verts = layer(x, b)[0]
        dist2, index, bary = tl.closest_surface(points, verts, faces, query_offset=offset)
        Jv = layer.jacobian(x, b)[0].double()                                  # [F, P, V, 3]
        F, P = Jv.shape[0], Jv.shape[1]
        N = points.shape[0]
        frame = _frames(torch, offset, N)
        faces_t = torch.tensor(faces, device=x.device).long()
        d, flat, c, ids = _plane_geometry(torch, verts, faces_t, frame, index, bary, points)
        keep = index >= 0
        if trunc is not None:
            cut = keep & ~(dist2 < trunc * trunc)
            keep = keep & (dist2 < trunc * trunc)
        else:
            cut = torch.zeros_like(keep)
        if mode == "plane":
            keep, cut = keep & ~flat, cut & ~flat
        w = keep.double()
        e = points.double() - c
        H = torch.zeros((F, P, P), dtype=torch.float64, device=x.device)
        Hh = torch.zeros_like(H)
        g = torch.zeros((F, P), dtype=torch.float64, device=x.device)
        d32 = d.float().double()
        for f in range(F):
            m = frame == f
            A = torch.einsum("na,panx->npx", bary[m].double(), Jv[f][:, ids[m].T, :])      # [n, P, 3]
            Aa = torch.einsum("na,panx->npx", bary[m].double().abs(), Jv[f][:, ids[m].T, :].abs())
            if mode == "point":
                H[f] = torch.einsum("n,npx,nqx->pq", w[m], A, A)
                Hh[f] = torch.einsum("n,npx,nqx->pq", w[m], Aa, Aa)
                g[f] = -torch.einsum("n,npx,nx->p", w[m], A, e[m])
            else:
                s = torch.einsum("npx,nx->np", A, d32[m])
                sa = torch.einsum("npx,nx->np", Aa, d32[m].abs())
                r = (d[m] * e[m]).sum(dim=1)
                H[f] = torch.einsum("n,np,nq->pq", w[m], s, s)
                Hh[f] = torch.einsum("n,np,nq->pq", w[m], sa, sa)
                g[f] = -torch.einsum("n,np,n->p", w[m], s, r)
        r2 = (e * e).sum(dim=1) if mode == "point" else ((d * e).sum(dim=1)) ** 2
        cost = 0.5 * (w * r2).sum()
        if trunc is not None:
            cost = cost + 0.5 * trunc * trunc * cut.double().sum()
    return cost, g, H, Hh


def _assert_gradient(torch, layer, x, b, cost_fn, g, per_frame, what):
    """g [F, P] against the reverse-mode gradient of cost_fn(verts) through the layer, within the adjoint test's bound"""
    xg, bg = x.clone().requires_grad_(), b.clone().requires_grad_()
    verts = layer(xg, bg)[0]
    verts.retain_grad()
    cost = cost_fn(verts)
    cost.backward()
    with torch.no_grad():
        Jv = layer.jacobian(x, b)[0]
    G = verts.grad.double()
    F = x.shape[0]
    jmax = Jv.abs().reshape(F, Jv.shape[1], -1).max(dim=2).values.double()                 # [F, P]
    gsum = G.abs().reshape(F, -1).sum(dim=1)                                              # [F]
    want_x = xg.grad
    want_b = bg.grad if per_frame else None
    gmax = torch.maximum(want_x.abs().max(dim=1).values, (bg.grad.abs().max(dim=-1).values if per_frame else bg.grad.abs().max()))
    bound = ADJOINT_TOL * jmax * gsum[:, None] + ADJOINT_TOL * gmax.reshape(-1, 1)         # [F, P]
    err_x = (g[:, :76] - want_x).abs()
    worst = float((err_x / bound[:, :76]).max())
    assert bool((err_x <= bound[:, :76]).all()), (what, worst)
    if per_frame:
        err_b = (g[:, 76:] - want_b).abs()
        worst = max(worst, float((err_b / bound[:, 76:]).max()))
        assert bool((err_b <= bound[:, 76:]).all()), (what, worst)
    else:
        err_b = (g[:, 76:].sum(dim=0) - bg.grad).abs()
        bb = bound[:, 76:].sum(dim=0)
        worst = max(worst, float((err_b / bb).max()))
        assert bool((err_b <= bb).all()), (what, worst)
    print(f"gram {what}: worst |g - autograd| / bound = {worst:.3e}")
    return cost.detach()


@pytest.mark.parametrize("per_frame", [False, True], ids=["shared_beta", "per_frame_beta"])
@pytest.mark.parametrize("mode", ["point", "plane"])
def test_surface_term_against_the_dense_path(api, torch, tl, synth, mode, per_frame):
    F, trunc = 2, 0.05
    v, layer, x, b, points, offset, faces = _scene(api, torch, tl, synth, "v289", F, per_frame, 300, seed=31)
    term = tl.SurfaceTerm(points, offset, faces, trunc=trunc)
    cost, g, H = term.normal_equations(layer, x, b, mode=mode, frame_chunk=1)
    P = 76 + v.n_shape
    assert H.shape == (F, P, P) and g.shape == (F, P) and H.dtype == torch.float64 and g.dtype == torch.float64
    cost_d, g_d, H_d, Hh = _dense_surface(torch, tl, layer, x, b, points, offset, faces, trunc, mode)
    ratio = float(((H - H_d).abs() / Hh.clamp(min=1e-300)).max())
    print(f"gram dense path {mode}: max |H - H_dense| / H^ = {ratio:.3e} (eps {gram_ref.EPS_H:.3e})")
    assert bool(((H - H_d).abs() <= gram_ref.EPS_H * Hh).all()), ratio
    assert torch.equal(H, H.transpose(1, 2))
    assert abs(float(cost) - float(cost_d)) <= 1e-4 * float(cost_d)        # (the search's f32 dist2 against the f64 residual)
    if mode == "point":
        cost_fn = lambda verts: 0.5 * term(verts)
    else:
        with torch.no_grad():
            verts0 = layer(x, b)[0]
            dist2, index, bary = tl.closest_surface(points, verts0, faces, query_offset=offset)
            frame = _frames(torch, offset, points.shape[0])
            faces_t = torch.tensor(faces, device="cuda").long()
            d, flat, _, ids = _plane_geometry(torch, verts0, faces_t, frame, index, bary, points)
            keep = (index >= 0) & ~flat
            w = (keep & (dist2 < trunc * trunc)).double()
            n_cut = (keep & ~(dist2 < trunc * trunc)).double().sum()

        def cost_fn(verts):       # 1/2 sum w (d . (p - c))^2 with (index, bary, d) held fixed, written in torch
            c = (bary.double()[:, :, None] * verts[frame[:, None], ids].double()).sum(dim=1)
            r = (d * (points.double() - c)).sum(dim=1)
            return 0.5 * (w * r * r).sum() + 0.5 * trunc * trunc * n_cut

    cost_t = _assert_gradient(torch, layer, x, b, cost_fn, g, per_frame, f"surface {mode}")
    assert abs(float(cost) - float(cost_t)) <= 1e-6 * float(cost_t)
    # the dense g is the same contraction in f64
    assert bool(((g - g_d).abs() <= 1e-4 * g_d.abs().max()).all())


@pytest.mark.parametrize("bidirectional", [False, True], ids=["one_way", "bidirectional"])
def test_point_cloud_term_against_the_dense_path(api, torch, tl, synth, bidirectional):
    F, trunc, per_frame = 2, 0.05, bidirectional            # (one way with a shared beta, both ways with a per-frame beta)
    v, layer, x, b, points, offset, _ = _scene(api, torch, tl, synth, "v289", F, per_frame, 300, seed=32)
    term = tl.PointCloudTerm(points, offset, bidirectional=bidirectional, trunc=trunc)
    cost, g, H = term.normal_equations(layer, x, b, frame_chunk=2)
    with torch.no_grad():
        verts = layer(x, b)[0]
        Jv = layer.jacobian(x, b)[0].double()
        P = Jv.shape[1]
        frame = _frames(torch, offset, points.shape[0])
        dist2, index = tl.closest_points(points, verts, query_offset=offset)
        w = ((index >= 0) & (dist2 < trunc * trunc)).double()
        H_d = torch.zeros((F, P, P), dtype=torch.float64, device="cuda")
        Hh = torch.zeros_like(H_d)
        for f in range(F):
            m = frame == f
            A = Jv[f][:, index[m].long(), :]                                   # [P, n, 3]
            H_d[f] = torch.einsum("n,pnx,qnx->pq", w[m], A, A)
            Hh[f] = torch.einsum("n,pnx,qnx->pq", w[m], A.abs(), A.abs())
        if bidirectional:
            dist2_v, index_v = tl.closest_points(verts, points, ref_offset=offset)
            wv = ((index_v >= 0) & (dist2_v < trunc * trunc)).double().view(F, -1)
            H_d += torch.einsum("fv,fpvx,fqvx->fpq", wv, Jv, Jv)
            Hh += torch.einsum("fv,fpvx,fqvx->fpq", wv, Jv.abs(), Jv.abs())
    ratio = float(((H - H_d).abs() / Hh.clamp(min=1e-300)).max())
    print(f"gram point cloud (bidirectional={bidirectional}): max |H - H_dense| / H^ = {ratio:.3e}")
    assert bool(((H - H_d).abs() <= gram_ref.EPS_H * Hh).all()), ratio
    assert torch.equal(H, H.transpose(1, 2))
    cost_t = _assert_gradient(torch, layer, x, b, lambda vv: 0.5 * term(vv), g, per_frame, "point cloud")
    assert abs(float(cost) - float(cost_t)) <= 1e-9 * float(cost_t)


def test_chunks_are_bit_identical_and_bound_the_memory(api, torch, tl, synth):
    F = 8
    R0 = _rotations(synth, F)                              # a per-frame R0, every frame its own: the chunks slice it
    v, layer, x, b, points, offset, faces = _scene(api, torch, tl, synth, "v289", F, True, 300, seed=33, R0=R0)
    term = tl.SurfaceTerm(points, offset, faces, trunc=0.05)
    P, V = 76 + v.n_shape, v.model.n_verts
    peak, out = {}, {}
    for chunk in (2, 8, 2, 8):                             # (the first round creates the problems and the handles)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out[chunk] = term.normal_equations(layer, x, b, mode="plane", frame_chunk=chunk)
        torch.cuda.synchronize()
        peak[chunk] = torch.cuda.max_memory_allocated()
    for a, c in zip(out[2], out[8]):
        assert torch.equal(a, c)
    c3 = term.normal_equations(layer, x, b, mode="plane", frame_chunk=3)      # a last chunk of two frames
    assert torch.equal(c3[2], out[8][2]) and torch.equal(c3[1], out[8][1])
    assert len(layer._chunk_problems) <= 1                 # one chunk problem at a time
    # the sliced R0 against the dense path, which runs all frames on problem(F)
    _, _, H_d, Hh = _dense_surface(torch, tl, layer, x, b, points, offset, faces, 0.05, "plane")
    assert bool(((out[2][2] - H_d).abs() <= gram_ref.EPS_H * Hh).all())
    saved = peak[8] - peak[2]
    print(f"gram memory: peak {peak[2]} bytes (chunk 2), {peak[8]} (chunk 8), saved {saved}; one Jacobian chunk of 2 frames "
          f"is {2 * P * V * 12}")
    assert saved >= 5 * P * V * 3 * 4


def test_library_memory_is_one_chunk_with_a_per_frame_R0(api, torch, tl, synth):
    """With a per-frame R0 every chunk runs on a problem of its own, and a problem's JVP scratch is its own (api_jvp.hip: per
    frame a 32-tangent tile of blend tangents [32][Vp][3] f32, the primal blend [Vp][3], the transform tangents and the
    coefficient fragments).  What the library holds on the device (everything in use there that is not torch's) may therefore
    grow, over a normal_equations call, by ONE chunk's problem and the Gram workspace of one chunk, whatever the number of
    chunks: 48 frames in chunks of 2 may take at most half of 48 frames' scratch more than 8 frames in chunks of 2 do (problems
    kept per chunk would take 40 frames' scratch more), and a second call nothing but rounding."""
    chunk = 2
    v = mv.get("v2049")
    Vp = 32 * ((v.model.n_verts + 31) // 32)
    scratch = 32 * Vp * 12 + Vp * 12 + 32 * 24 * 12 * 4 + 14 * 2 * 64 * 8 * 2          # bytes per frame

    def library_bytes():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free - torch.cuda.memory_reserved()

    def growth(F):
        _, layer, x, b, points, offset, faces = _scene(api, torch, tl, synth, "v2049", F, True, 60, seed=34, outliers=0,
                                                       R0=_rotations(synth, F), step=0)
        term = tl.SurfaceTerm(points, offset, faces)
        with torch.no_grad():
            term(layer(x, b)[0])                           # the forward's problem, the handle and the search's workspace
        before = library_bytes()
        first = term.normal_equations(layer, x, b, mode="point", frame_chunk=chunk)
        after = library_bytes()
        again = term.normal_equations(layer, x, b, mode="point", frame_chunk=chunk)
        steady = library_bytes()
        assert len(layer._chunk_problems) <= 1
        assert torch.equal(first[2], again[2])
        return after - before, steady - after

    g8, s8 = growth(8)
    g48, s48 = growth(48)
    print(f"gram library memory: +{g8} bytes over the first call at 8 frames (+{s8} over the second), +{g48} at 48 frames "
          f"(+{s48}); the JVP scratch of 48 frames is {48 * scratch}")
    assert g48 - g8 <= 48 * scratch // 2
    assert s8 <= 2 * scratch and s48 <= 2 * scratch


# ---- a fit ------------------------------------------------------------------------------------------------------------------
def test_keypoint_and_scan_fit_matches_the_dense_gauss_newton(api, torch, tl, synth):
    """The setting of test_gauss_newton_fit_on_the_jacobian (two frames of the 2,049-vertex model, per-frame beta, gn_start's
    perturbed start), with scan points sampled on the mesh at (x*, beta*) and keypoints observed there.  Damped Gauss-Newton on
    the FitObjective's keypoint normals plus w x the scan normals, plane mode, once with SurfaceTerm.normal_equations and once
    with the dense Jacobian, each until an accepted step gains less than 1 % of the cost.  The samples carry 1 mm of noise so that the optimum's scan cost sits far above the f32 floor:
    "within 1 %" then compares the fits, not their roundings."""
    v = mv.get("v2049")
    F, w_scan, cap = 2, 1e6, 15
    gm = _gmv(api, v)
    layer = tl.SMPLLayer(gm, beta_per_frame=True)
    xs, bs, x0, b0 = gn_start(v)
    dev = lambda a: torch.tensor(a, device="cuda")
    V = v.model.n_verts
    faces = synth.make_faces(v.model, n_faces=2 * V - 4)
    rng = np.random.default_rng(41)
    with torch.no_grad():
        target = layer(dev(xs), dev(bs))[0].cpu().numpy().astype(np.float64)
    n = 3000
    t = rng.integers(0, len(faces), size=(F, n))
    bw = rng.dirichlet(np.ones(3), size=(F, n))
    pts = np.stack([np.einsum("na,nax->nx", bw[f], target[f][faces[t[f]]]) for f in range(F)]) + rng.normal(scale=1e-3, size=(F, n, 3))
    points = dev(pts.astype(np.float32))
    term = tl.SurfaceTerm(points, None, faces)
    # keypoints observed at (x*, beta*): the residual with uv = 0 is the projection, up to its sign
    ids = mv.kp_ids(v)
    kp_off = np.arange(F + 1, dtype=np.int32) * len(ids)
    kp_id = np.tile(ids, F)
    intr, R0 = synth.camera_intrinsics(), np.tile(np.eye(3).reshape(1, 9), (F, 1))
    mk = lambda uv: api.Problem(gm, kp_off, kp_id, uv, intr, R0, n_cols=86, use_shape=True, beta_per_frame=True, huber_delta=0.0)
    K2 = 2 * len(kp_id)
    assert mk(np.zeros((len(kp_id), 2))).layout.reproj_rows == K2
    r0 = mk(np.zeros((len(kp_id), 2))).evaluate(xs, bs, False)[0][:K2].reshape(-1, 2)
    prob = mk(r0)
    if np.abs(prob.evaluate(xs, bs, False)[0][:K2]).max() > 1e-6:
        prob = mk(-r0)
    assert np.abs(prob.evaluate(xs, bs, False)[0][:K2]).max() <= 1e-6
    obj = tl.FitObjective(prob)

    def keypoint_normals(x, b):
        r, J, _ = prob.evaluate(x.cpu().numpy(), b.cpu().numpy(), True)
        r, J = dev(r[:K2]).view(F, -1), dev(J).view(F, -1, 86)
        with torch.no_grad():
            cost = obj.cost(obj(x, b))
        return cost, torch.einsum("frp,fr->fp", J, r), torch.einsum("frp,frq->fpq", J, J)

    def fused(x, b):
        return term.normal_equations(layer, x, b, mode="plane")

    def dense(x, b):
        return _dense_surface(torch, tl, layer, x, b, points.view(-1, 3), dev(np.arange(F + 1, dtype=np.int32) * n), faces, None,
                              "plane")[:3]

    def fit(scan, max_iters):
        x, b, lam = dev(x0), dev(b0), 1e-3

        def total(xx, bb):
            ck, gk, Hk = keypoint_normals(xx, bb)
            cs, gs, Hs = scan(xx, bb)
            return float(ck + w_scan * cs), float(cs), gk + w_scan * gs, Hk + w_scan * Hs

        c, cs, g, H = total(x, b)
        it = 0
        while it < max_iters:
            it += 1
            D = torch.diagonal(H, dim1=1, dim2=2)
            D = torch.maximum(D, 1e-9 * D.max(dim=1, keepdim=True).values)
            step = torch.linalg.solve(H + lam * torch.diag_embed(D), -g[:, :, None])[:, :, 0]
            xn, bn = x + step[:, :76], b + step[:, 76:]
            cn, csn, gn, Hn = total(xn, bn)
            print(f"gram fit   iteration {it}: total {c:.6e} -> {cn:.6e}, scan {csn:.6e}, lambda {lam:.1e}")
            if cn < c:
                done = c - cn < 1e-2 * c                   # converged: an accepted step that gains less than 1 %
                x, b, c, cs, g, H, lam = xn, bn, cn, csn, gn, Hn, lam * 0.5
                if done:
                    break
            else:
                lam *= 2.0
        return cs, c, it

    scan_dense, total_dense, it_dense = fit(dense, cap)
    scan_fused, total_fused, it_fused = fit(fused, it_dense)
    print(f"gram fit: dense scan cost {scan_dense:.6e} (total {total_dense:.6e}) after {it_dense} iterations; fused "
          f"{scan_fused:.6e} (total {total_fused:.6e}) after {it_fused}")
    assert it_dense < cap
    assert it_fused <= it_dense
    assert scan_fused <= 1.01 * scan_dense
    assert scan_dense <= 4 * 0.5 * F * n * 1e-6          # the baseline did fit: the noise's own cost is 1/2 F n sigma^2
