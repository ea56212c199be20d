"""The body as a solid: winding numbers, vertex normals, the mesh Laplacian, the signed distance and the self-penetration term.

    w = winding_number(points, verts, faces, offset)                     # 0 outside, 1 inside a closed mesh (no gradient)
    sdf, index, bary = signed_distance(points, verts, faces, offset)     # negative inside; closest_surface's gradient
    term = SelfPenetrationTerm(faces, trunc=0.05)                        # m^2: the vertices inside another part of the body

None of the data terms knows that the body is a solid.  winding_number is bodyfit_surface_winding_device (k_winding.hip: all
pairs of query and triangle, the half solid angles summed exactly as integers); vertex_winding asks it about the mesh's own
vertices with their own faces left out, where w > 1 means "inside another part of the body" without a threshold.
SelfPenetrationTerm matches those vertices, through the oriented search with minus their normal (vertex_normals,
bodyfit_surface_vertex_normals_device), to the sheet they have passed through, and pulls them back out.

    reg = OffsetRegulariser(faces, w_smooth=1e3, w_norm=1.0)             # w_smooth sum |L d|^2 + w_norm sum |d|^2
    (term(verts) + reg(d)).backward()

The regulariser of SMPLLayer's per-vertex offsets.  mesh_laplacian is bodyfit_surface_laplacian_device, a deterministic gather
whose backward is the transposed gather.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._common import (_SURFACE_CACHE, _TermHandles, _host_faces, _point_set, _ragged_rows, _rho_sum, _stream,
                      _surface_handle)
from .scan import closest_surface


def _posed_mesh(verts, faces):
    """(the [F, V, 3] f32 tensor to keep alive, its api.PointSet, F, the api.Surface) of a posed mesh; verts is used detached"""
    if not isinstance(verts, torch.Tensor):
        raise TypeError("verts must be a torch tensor")
    if verts.dtype != torch.float32:
        raise TypeError("verts must be float32")
    if not verts.is_cuda:
        raise ValueError("verts must be on the GPU")
    if verts.ndim != 3 or verts.shape[2] != 3:
        raise ValueError(f"verts must be [F, V, 3], got {tuple(verts.shape)}")
    v, vs, F, _ = _point_set("verts", verts.detach(), None)
    return v, vs, F, _surface_handle(v.device.index, v.shape[1], faces)


def _winding(q, qs, nq, skip, v, vs, F, handle) -> torch.Tensor:
    w = torch.empty(nq, dtype=torch.float32, device=v.device)
    if nq > 0 and F > 0:
        with torch.cuda.device(v.device):
            handle.winding_device(qs, skip.data_ptr() if skip is not None else None, v.data_ptr(), vs.frame_stride, F, nq,
                                  w.data_ptr(), _stream())
    return w


def winding_number(points: torch.Tensor, verts: torch.Tensor, faces, offset: torch.Tensor | None = None,
                   skip_vertex: torch.Tensor | None = None) -> torch.Tensor:
    """The winding number w [N] f32 of every point about the posed mesh of its frame (bodyfit_surface_winding_device,
    k_winding.hip): for a closed, outward oriented mesh the number of times the surface encloses the point, 0 outside and 1 inside;
    for an open mesh the generalised winding number.  points, verts, faces and offset as in closest_surface.  skip_vertex: None,
    or int32 on the same GPU with one id per point ([N], or the leading shape of points): row i leaves out the faces that have
    that vertex id among their corners (-1: none).  A frame with a non-finite vertex in a face gives NaN for its points, a NaN
    point gives NaN.  No gradient: w is piecewise constant.  Runs on torch.cuda.current_stream()."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch tensor")
    q, qs, F, nq = _point_set("points", points.detach(), offset)
    v, vs, Fv, handle = _posed_mesh(verts, faces)
    if F != Fv:
        raise ValueError(f"points has {F} frames, verts has {Fv}")
    if v.device != q.device:
        raise ValueError("points and verts must be on the same GPU")
    skip = None
    if skip_vertex is not None:
        if not isinstance(skip_vertex, torch.Tensor) or skip_vertex.dtype != torch.int32:
            raise TypeError("skip_vertex must be an int32 tensor")
        if skip_vertex.device != q.device:
            raise ValueError("skip_vertex must be on the GPU of points")
        if skip_vertex.numel() != nq or skip_vertex.shape != points.shape[:-1]:
            raise ValueError(f"skip_vertex must have one id per point, {tuple(points.shape[:-1])}, got {tuple(skip_vertex.shape)}")
        skip = skip_vertex.contiguous()
    return _winding(q, qs, nq, skip, v, vs, F, handle)


def _vertex_ids(vertex_ids, n_verts: int):
    """the checked host int32 [K] array of a vertex subset (None stays None)"""
    if vertex_ids is None:
        return None
    ids = vertex_ids.detach().cpu().numpy() if isinstance(vertex_ids, torch.Tensor) else np.asarray(vertex_ids)
    if ids.dtype.kind not in "iu" or ids.ndim != 1:
        raise TypeError("vertex_ids must be a one-dimensional integer array")
    if ids.size and (int(ids.min()) < 0 or (n_verts is not None and int(ids.max()) >= n_verts)):
        raise ValueError(f"vertex_ids holds an id outside [0, {n_verts})")
    return np.ascontiguousarray(ids, dtype=np.int32)


def vertex_winding(verts: torch.Tensor, faces, vertex_ids=None) -> torch.Tensor:
    """w [F, V] f32 (or [F, len(vertex_ids)]): the winding number of the posed mesh about its OWN vertices, each with the faces
    it is a corner of left out: w_i = k_i + (the interior solid angle of the cone of faces about vertex i) / 4 pi, k_i the number of
    other sheets of the surface that enclose it.  The cone's share lies strictly between 0 and 1, so vertex i lies inside another
    part of the body iff w_i > 1: no threshold to tune.  No gradient."""
    v, vs, F, handle = _posed_mesh(verts, faces)
    V = v.shape[1]
    ids = _vertex_ids(vertex_ids, V)
    gather, skip = _skip_ids(v.device, F, V, ids)
    if gather is None:
        return _winding(v, vs, F * V, skip, v, vs, F, handle).view(F, V)
    q, qs, _, nq = _point_set("verts", v[:, gather].contiguous(), None)
    return _winding(q, qs, nq, skip, v, vs, F, handle).view(F, len(ids))


_skip_cache: dict[tuple, tuple] = {}   # (device, F, V, the subset's bytes) -> (int64 ids or None, int32 skip [F K]); the last _SURFACE_CACHE


def _skip_ids(device, F: int, V: int, ids):
    """(the subset as an int64 device tensor, or None for every vertex; the packed skip ids of the vertex query, int32 [F K]),
    kept between calls: a term asks for the same ones at every evaluation"""
    key = (device.index, F, V, None if ids is None else ids.tobytes())
    hit = _skip_cache.pop(key, None)
    if hit is None:
        one = torch.arange(V, dtype=torch.int32, device=device) if ids is None else torch.from_numpy(ids).to(device)
        hit = (None if ids is None else one.long(), one.repeat(F))
    _skip_cache[key] = hit                           # (most recently used last)
    while len(_skip_cache) > _SURFACE_CACHE:
        _skip_cache.pop(next(iter(_skip_cache)))
    return hit


def vertex_normals(verts: torch.Tensor, faces) -> torch.Tensor:
    """n [F, V, 3] f32: the area-weighted unit vertex normals of the posed mesh, normalise(sum of (v1 - v0) x (v2 - v0) over the
    faces that hold the vertex), oriented as faces; 0 for a vertex without a face, with a zero sum or a non-finite corner
    (bodyfit_surface_vertex_normals_device: summed in f64 in a fixed order, bit-identical from run to run).  No gradient."""
    v, vs, F, handle = _posed_mesh(verts, faces)
    n = torch.empty((F, v.shape[1], 3), dtype=torch.float32, device=v.device)
    if n.numel() > 0:
        with torch.cuda.device(v.device):
            handle.vertex_normals_device(v.data_ptr(), vs.frame_stride, F, n.data_ptr(), _stream())
    return n


class _MeshLaplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, handle):
        ctx.handle = handle
        return _laplacian(field, handle, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _laplacian(g.to(torch.float32).contiguous(), ctx.handle, True), None


def _laplacian(field: torch.Tensor, handle, transpose: bool) -> torch.Tensor:
    n = field.numel() // (3 * handle.n_verts) if handle.n_verts > 0 else 0
    out = torch.empty_like(field)
    if out.numel() > 0:
        with torch.cuda.device(field.device):
            handle.laplacian_device(field.data_ptr(), 3 * handle.n_verts, n, out.data_ptr(), transpose, _stream())
    return out


def mesh_laplacian(field: torch.Tensor, faces) -> torch.Tensor:
    """The uniform Laplacian of a per-vertex field [V, 3] or [K, V, 3] f32 on the GPU over the topology `faces` (int32
    [n_faces, 3] on the host, or an api.Surface): l_i = x_i - (1 / 2 n_i) sum over the n_i faces that hold i of their other two
    corners, an interior vertex minus the mean of its ring; 0 for a vertex without a face (bodyfit_surface_laplacian_device:
    a gather in f64 in a fixed order).  Differentiable: the backward is the transposed gather, as deterministic as the forward
    (torch's index_add_ is not)."""
    if not isinstance(field, torch.Tensor):
        raise TypeError("field must be a torch tensor")
    if field.dtype != torch.float32:
        raise TypeError("field must be float32")
    if not field.is_cuda:
        raise ValueError("field must be on the GPU")
    if field.ndim not in (2, 3) or field.shape[-1] != 3:
        raise ValueError(f"field must be [V, 3] or [K, V, 3], got {tuple(field.shape)}")
    handle = _surface_handle(field.device.index, field.shape[-2], faces)
    return _MeshLaplacian.apply(field.contiguous(), handle)


class OffsetRegulariser(_TermHandles, torch.nn.Module):
    """w_smooth sum |L d|^2 + w_norm sum |d|^2 (f64) of per-vertex offsets d [V, 3] or [F, V, 3] f32, L the uniform mesh Laplacian
    of `faces` (mesh_laplacian): what keeps an offset field a garment and not noise.  The keypoint landmarks and the joints do
    not see the offsets, so without this term the vertices no data term reaches are free."""

    def __init__(self, faces, w_smooth: float = 1.0, w_norm: float = 0.0):
        super().__init__()
        if w_smooth < 0.0 or w_norm < 0.0:
            raise ValueError("the weights must be non-negative")
        self.faces = _host_faces(faces).copy()
        self.w_smooth = float(w_smooth)
        self.w_norm = float(w_norm)

    def forward(self, offsets: torch.Tensor) -> torch.Tensor:
        handle = self.faces
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.ndim in (2, 3):
            handle = self._handle_for(offsets)
        lap = mesh_laplacian(offsets, handle).double()
        d = offsets.double()
        return self.w_smooth * (lap * lap).sum() + self.w_norm * (d * d).sum()


class _SignedRoot(torch.autograd.Function):
    """sign sqrt(dist2), with the gradient sign / (2 sqrt(dist2)) and 0 where dist2 = 0 (the point is on the surface)"""

    @staticmethod
    def forward(ctx, dist2, sign):
        root = torch.sqrt(dist2)
        ctx.save_for_backward(root, sign)
        return sign * root

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        root, sign = ctx.saved_tensors
        return torch.where(root > 0, g * sign / (2.0 * root), torch.zeros_like(root)), None


def signed_distance(points: torch.Tensor, verts: torch.Tensor, faces, offset: torch.Tensor | None = None):
    """(sdf [N] f32, index [N] int32, bary [N, 3] f32): sdf = sign(1/2 - w) sqrt(dist2) with (dist2, index, bary) of
    closest_surface and w of winding_number: NEGATIVE inside a closed, outward oriented mesh.  The gradient is closest_surface's
    at the fixed correspondence times sign / (2 sqrt(dist2)), 0 where dist2 = 0; the sign carries none.  A NaN w gives a NaN sdf.
    sign(0) = 0: a point whose w is exactly 1/2 gets sdf = 0 however far it is from the surface.  About a closed mesh w is an integer
    off the surface and this does not occur; about an OPEN mesh w passes 1/2 smoothly and "inside" has no meaning there anyway."""
    dist2, index, bary = closest_surface(points, verts, faces, query_offset=offset)
    w = winding_number(points, verts, faces, offset)
    sign = torch.where(torch.isnan(w), w, torch.sign(0.5 - w))      # (torch.sign(nan) is 0)
    return _SignedRoot.apply(dist2, sign), index, bary


class SelfPenetrationTerm(_TermHandles, torch.nn.Module):
    """The interpenetration term of a posed mesh: sum over the vertices that lie INSIDE another part of the body of rho(squared
    distance to the sheet they have passed through), m^2.

    faces: int32 [n_faces, 3], closed and outward oriented.  trunc = tau: rho(s) = min(s, tau^2); None: rho(s) = s.  vertex_ids:
    None (every vertex), or the subset to test (hands and forearms, say).  term(verts), verts [F, V, 3] f32, returns the f64 cost:
      enclosed:  vertex_winding(verts.detach()) > 1, NaN counting as not enclosed: a ragged set with a CSR offset;
      matched:   closest_surface(P, verts, faces, offset, point_normals=-n_i, min_cos) with n_i = vertex_normals: the direction
                 gate removes the vertex's own neighbourhood, whose normals agree with n_i, and leaves the sheet the vertex has
                 passed through, whose normals oppose it; a vertex without such a face (index -1) costs nothing;
      gradient:  closest_surface's (bodyfit_closest_surface_vjp_device) at the fixed correspondence, on the gathered rows and on
                 the corners of the matched faces, both of which are verts.  Which vertices are enclosed is piecewise constant.
    With no enclosed vertex the result is 0 with a zero gradient and nothing is searched.  The gather sizes its result on the host:
    one synchronisation per evaluation."""

    def __init__(self, faces, trunc: float | None = None, min_cos: float = 0.0, vertex_ids=None):
        super().__init__()
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        self.faces = _host_faces(faces).copy()
        self.trunc = None if trunc is None else float(trunc)
        self.min_cos = float(min_cos)
        self.vertex_ids = _vertex_ids(vertex_ids, None)

    def evaluate(self, verts: torch.Tensor) -> dict:
        """The term's parts: winding [F, K] f32, inside [F, K] bool, offset int32 [F + 1] (the CSR of the enclosed vertices), rows
        [n] int64 (their vertex ids), and dist2 [n] (with the term's gradient), index [n], bary [n, 3] of their matches; K = V or
        len(vertex_ids).  Without an enclosed vertex the last four are empty."""
        # (not _check_verts: one TypeError for all of it, with a message of its own)
        if (not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32 or not verts.is_cuda or verts.ndim != 3
                or verts.shape[2] != 3):
            raise TypeError("verts must be a float32 tensor [F, V, 3] on the GPU")
        handle = self._handle_for(verts)
        vd = verts.detach()
        _vertex_ids(self.vertex_ids, vd.shape[1])
        winding = vertex_winding(vd, handle, self.vertex_ids)
        inside = winding > 1.0
        frame, col, offset, _ = _ragged_rows(inside)               # frame-major: the packed order of a ragged set
        col = col.long()                                           # (the helper packs columns as the kernels read them, int32; an index is int64)
        rows = col if self.vertex_ids is None else torch.from_numpy(self.vertex_ids).to(vd.device).long()[col]
        out = dict(winding=winding, inside=inside, offset=offset, rows=rows)
        if rows.numel() == 0:
            out.update(dist2=verts[:0, :0, 0].reshape(0), index=torch.zeros(0, dtype=torch.int32, device=vd.device),
                       bary=torch.zeros((0, 3), dtype=torch.float32, device=vd.device))
            return out
        P = verts[frame, rows]                                     # [n, 3], frame after frame; differentiable
        m = -vertex_normals(vd, handle)[frame, rows]
        out["dist2"], out["index"], out["bary"] = closest_surface(P, verts, handle, query_offset=offset,
                                                                  point_normals=m.contiguous(), min_cos=self.min_cos)
        return out

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        e = self.evaluate(verts)
        if e["rows"].numel() == 0:
            return e["dist2"].sum().double()                     # 0, with a zero gradient
        return _rho_sum(e["dist2"], e["index"], self.trunc)
