"""The 3-D scan terms: closest points, closest surface, and their Gauss-Newton normal equations.

    dist2, index = closest_points(points, verts, query_offset=offset)   # every scan point against its frame's vertices
    term = PointCloudTerm(points, offset)                               # sum of (truncated) squared distances
    (obj.cost(obj(x, beta)) + w * term(layer(x, beta)[0])).backward()   # keypoints + priors + scan

closest_points is bodyfit_closest_points_device (k_closest.hip: brute force from LDS, no [F, N, V] intermediate); its backward is
bodyfit_closest_points_vjp_device, with the correspondence held fixed, deterministic like the other gradients here.

    dist2, index, bary = closest_surface(points, verts, faces, query_offset=offset)   # ... against its frame's TRIANGLES
    term = SurfaceTerm(points, offset, faces)                                         # the scan -> surface cost
    (obj.cost(obj(x, beta)) + w * term(layer(x, beta)[0])).backward()

closest_surface is bodyfit_closest_surface_device (k_closest_surface.hip: prepared triangle records streamed through LDS, a
conservative sphere cull, no [F, N, n_faces] intermediate): a point on the posed surface costs nothing wherever it falls between
the vertices, which the point-to-point term cannot offer.  Its backward is bodyfit_closest_surface_vjp_device at the fixed
(index, bary), which by the envelope theorem is the true gradient of the squared distance almost everywhere.

    dist2, index, bary = closest_surface(points, verts, faces, query_offset=offset, point_normals=normals, min_cos=0.5)
    term = SurfaceTerm(points, offset, faces, normals=normals, min_cos=0.5)          # normal-compatible correspondences

With point_normals (the scan's normals, or for a depth map the directions towards the sensor) a point may only match a triangle
whose face normal n, in the orientation of faces, has n . m >= min_cos (bodyfit_closest_surface_oriented_device): the inside
of the arm no longer matches the torso because the torso is nearer.  The gate is piecewise constant, so the backward is the same.

    cost, g, H = term.normal_equations(layer, x, beta, mode="plane")    # g [F, P] f64, H [F, P, P] f64, P = 76 + nS
    H, g = surface_gram(jac, points, index, bary, faces, weight=w, direction=d, rhs=rhs)   # the kernel behind it

The second-order side of the scan terms: per frame the Gauss-Newton normal equations H = J^T W J, g = J^T rhs of
1/2 sum w r^2 at the current correspondence, in the column order of SMPLLayer.jacobian (bodyfit_surface_gram_device,
k_surface_gram.hip: per-face moments, a sparse mix and one dense contraction on the matrix pipe; no per-point Jacobian row, and
the dense vertex Jacobian only frame_chunk frames at a time).  A keypoint + prior + scan Levenberg-Marquardt step adds these
panels to its own and solves with torch.linalg.solve.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import _TermHandles, _closest_handle, _grads_for, _host_faces, _point_set, _rho_sum, _stream, _surface_handle
from .smpl import SMPLLayer


class _ClosestPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, ref, query_offset, ref_offset):
        q, qs, F, nq = _point_set("query", query, query_offset)
        r, rs, Fr, nr = _point_set("ref", ref, ref_offset)
        if F != Fr:
            raise ValueError(f"query has {F} frames, ref has {Fr}")
        if r.device != q.device:
            raise ValueError("query and ref must be on the same GPU")
        handle = _closest_handle(q.device.index)
        dist2 = torch.empty(nq, dtype=torch.float32, device=q.device)
        index = torch.empty(nq, dtype=torch.int32, device=q.device)
        if nq > 0:
            # (the reference set's gradient needs the queries grouped by reference row: built with the search, once)
            handle.points_device(qs, rs, F, nq, nr, dist2.data_ptr(), index.data_ptr(), _stream(),
                                 prepare_vjp=ctx.needs_input_grad[1])
        ctx.sets = (qs, rs, F, nq, nr, handle)
        ctx.save_for_backward(q, r, index)
        ctx.mark_non_differentiable(index)
        return dist2, index

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dist2, _g_index):
        q, r, index = ctx.saved_tensors
        qs, rs, F, nq, nr, handle = ctx.sets
        live = g_dist2 is not None and nq > 0
        gq, gr = _grads_for(ctx, ((q, qs), (r, rs)), live)
        if live:
            g = g_dist2.to(torch.float32).contiguous()
            handle.points_vjp_device(qs, rs, F, nq, nr, index.data_ptr(), g.data_ptr(),
                                     gq.data_ptr() if gq is not None else None,
                                     gr.data_ptr() if gr is not None else None, _stream())
        return gq, gr, None, None


def closest_points(query: torch.Tensor, ref: torch.Tensor, query_offset: torch.Tensor | None = None,
                   ref_offset: torch.Tensor | None = None):
    """For every query point the closest reference point of the same frame: (dist2 [N] f32, index [N] int32, frame-local, -1
    and +inf where the frame has no reference point), packed in frame order.

    A point set is f32 on the GPU, either uniform, [F, n, 3] (a view whose frames are farther apart than 3 n floats, such as
    the library's padded cloud, is used without a copy), or ragged, [N, 3] with an int32 offset [F + 1] on the same GPU
    (offset[0] = 0, offset[F] = N, non-decreasing: not checked, that would synchronise).
    dist2 is differentiable with respect to both point tensors with the correspondence held fixed (the ICP / Chamfer gradient);
    index carries no gradient.  Runs on torch.cuda.current_stream() without a host synchronisation (bodyfit_closest_points_device
    and bodyfit_closest_points_vjp_device, k_closest.hip).  Calls on one GPU share a workspace: interleaving them on several
    streams at once needs the caller's own ordering."""
    return _ClosestPoints.apply(query, ref, query_offset, ref_offset)


class PointCloudTerm(torch.nn.Module):
    """The 3-D data term of a sequence: sum over the target points of rho(squared distance to the closest vertex of the frame),
    plus, when bidirectional, the same from every vertex to the closest target point of its frame.

    points: [N, 3] f32 on the GPU with offset, int32 [F + 1] (a depth map, scan or marker set per frame; frames may be empty),
    or [F, n, 3] with offset None.  trunc = tau: rho(s) = min(s, tau^2), so points farther than tau from the body (background)
    stop pulling; None: rho(s) = s.  term(verts), verts [F, V, 3] f32 (SMPLLayer's first output), returns the f64 cost."""

    def __init__(self, points: torch.Tensor, offset: torch.Tensor | None = None, bidirectional: bool = False,
                 trunc: float | None = None):
        super().__init__()
        _point_set("points", points, offset)   # the checks
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        self.register_buffer("points", points.detach())
        self.register_buffer("offset", offset.detach() if offset is not None else None)
        self.bidirectional = bool(bidirectional)
        self.trunc = None if trunc is None else float(trunc)
        self._pseudo: dict[tuple, object] = {}   # (device, V) -> the api.Surface of the one-corner faces (v, v, v) (normal_equations)
        self._offset_host = None

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        cost = _rho_sum(*closest_points(self.points, verts, query_offset=self.offset), self.trunc)
        if self.bidirectional:
            cost = cost + _rho_sum(*closest_points(verts, self.points, ref_offset=self.offset), self.trunc)
        return cost

    def normal_equations(self, layer: "SMPLLayer", x: torch.Tensor, beta: torch.Tensor, frame_chunk: int = 32, offsets=None):
        """(cost, g [F, P], H [F, P, P]), f64: the Gauss-Newton normal equations of 1/2 term(verts) at the current closest
        vertices, as SurfaceTerm.normal_equations gives them for the surface term (conventions there).  A scan point's
        counterpart is a vertex, so the kernel sees a list of one-corner pseudo-faces (v, v, v) with the weights (1, 0, 0); the
        bidirectional half (every vertex against its closest scan point) is the same call with a diagonal W."""
        return _normal_equations(self, layer, x, beta, frame_chunk, lambda verts: self._jobs(verts), offsets)

    def _jobs(self, verts):
        F, V = verts.shape[0], verts.shape[1]
        dev = verts.device
        handle = self._pseudo.get((dev.index, V))
        if handle is None:
            pseudo = np.repeat(np.arange(V, dtype=np.int32)[:, None], 3, axis=1)
            handle = self._pseudo[(dev.index, V)] = api.Surface(dev.index, V, pseudo)
        _, qs, _, nq = _point_set("points", self.points, self.offset)
        v, vs, _, nv = _point_set("verts", verts, None)
        closest = _closest_handle(dev.index)

        def half(query_ps, ref_ps, n_query, n_ref):
            dist2 = torch.empty(n_query, dtype=torch.float32, device=dev)
            index = torch.empty(n_query, dtype=torch.int32, device=dev)
            if n_query > 0:
                closest.points_device(query_ps, ref_ps, F, n_query, n_ref, dist2.data_ptr(), index.data_ptr(), _stream())
            keep = index >= 0
            if self.trunc is not None:
                keep = keep & (dist2 < self.trunc * self.trunc)
            return index, keep.to(torch.float32), 0.5 * _rho_sum(dist2, index, self.trunc)

        def corner_zero(n):
            bary = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            bary[:, 0] = 1.0
            return bary

        index, weight, cost = half(qs, vs, nq, nv)
        rhs = torch.zeros((F, V, 3), dtype=torch.float32, device=dev)
        if nq > 0 and nv > 0:
            half_w = 0.5 * weight
            closest.points_vjp_device(qs, vs, F, nq, nv, index.data_ptr(), half_w.data_ptr(), None, rhs.data_ptr(), _stream())
        jobs = [_GramJob(handle, self.points, self.offset, _host_offset(self), index, corner_zero(nq), weight, None)]
        if self.bidirectional:
            index_v, weight_v, cost_v = half(vs, qs, nv, nq)
            cost = cost + cost_v
            if nq > 0 and nv > 0:
                back = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
                half_w = 0.5 * weight_v
                closest.points_vjp_device(vs, qs, F, nv, nq, index_v.data_ptr(), half_w.data_ptr(), back.data_ptr(), None, _stream())
                rhs = rhs + back
            own = torch.arange(V, dtype=torch.int32, device=dev).repeat(F)
            jobs.append(_GramJob(handle, v, None, None, own, corner_zero(nv), weight_v, None))
        return cost, rhs, jobs


class _ClosestSurface(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, verts, faces, query_offset, point_normals, min_cos):
        q, qs, F, nq = _point_set("points", points, query_offset)
        if not isinstance(verts, torch.Tensor):
            raise TypeError("verts must be a torch tensor")
        if verts.dtype != torch.float32:
            raise TypeError("verts must be float32")
        if not verts.is_cuda:
            raise ValueError("verts must be on the GPU")
        if verts.ndim != 3 or verts.shape[2] != 3:
            raise ValueError(f"verts must be [F, V, 3], got {tuple(verts.shape)}")
        v, vs, Fv, _ = _point_set("verts", verts, None)
        if F != Fv:
            raise ValueError(f"points has {F} frames, verts has {Fv}")
        if v.device != q.device:
            raise ValueError("points and verts must be on the same GPU")
        handle = _surface_handle(q.device.index, v.shape[1], faces)
        dist2 = torch.empty(nq, dtype=torch.float32, device=q.device)
        index = torch.empty(nq, dtype=torch.int32, device=q.device)
        bary = torch.empty((nq, 3), dtype=torch.float32, device=q.device)
        if point_normals is not None:
            m = _packed_normals(point_normals, points)
            if nq > 0:
                handle.closest_oriented_device(qs, m.data_ptr(), min_cos, v.data_ptr(), vs.frame_stride, F, nq, dist2.data_ptr(),
                                               index.data_ptr(), bary.data_ptr(), _stream(), prepare_vjp=ctx.needs_input_grad[1])
        elif nq > 0:
            handle.closest_device(qs, v.data_ptr(), vs.frame_stride, F, nq, dist2.data_ptr(), index.data_ptr(), bary.data_ptr(),
                                  _stream(), prepare_vjp=ctx.needs_input_grad[1])
        ctx.sets = (qs, vs, F, nq, handle)
        ctx.save_for_backward(q, v, index, bary)
        ctx.mark_non_differentiable(index, bary)
        return dist2, index, bary

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dist2, _g_index, _g_bary):
        q, v, index, bary = ctx.saved_tensors
        qs, vs, F, nq, handle = ctx.sets
        live = g_dist2 is not None and nq > 0
        gq, gv = _grads_for(ctx, ((q, qs), (v, vs)), live)
        if live:
            g = g_dist2.to(torch.float32).contiguous()
            handle.vjp_device(qs, v.data_ptr(), vs.frame_stride, F, nq, index.data_ptr(), bary.data_ptr(), g.data_ptr(),
                              gq.data_ptr() if gq is not None else None, gv.data_ptr() if gv is not None else None, _stream())
        return gq, gv, None, None, None, None


def _packed_normals(normals, points) -> torch.Tensor:
    """the checked directions of `points` as one packed [N, 3] f32 array in the row order of dist2"""
    if not isinstance(normals, torch.Tensor):
        raise TypeError("point_normals must be a torch tensor")
    if normals.dtype != torch.float32:
        raise TypeError("point_normals must be float32")
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch tensor")
    if normals.device != points.device:
        raise ValueError("point_normals must be on the GPU of points")
    if normals.shape != points.shape:
        raise ValueError(f"point_normals must have the shape of points, {tuple(points.shape)}, got {tuple(normals.shape)}")
    if normals.requires_grad:
        raise ValueError("point_normals carries no gradient (the gate is piecewise constant): pass point_normals.detach()")
    return normals.contiguous()


def closest_surface(points: torch.Tensor, verts: torch.Tensor, faces, query_offset: torch.Tensor | None = None,
                    point_normals: torch.Tensor | None = None, min_cos: float = 0.0):
    """For every point the closest point on the triangles (verts[f][faces[t]]) of its frame: (dist2 [N] f32, index [N] int32,
    the frame-local triangle, bary [N, 3] f32, the barycentric weights of the closest point), packed in frame order; -1, +inf
    and zeros where no finite candidate exists (no faces, a NaN point).

    points: f32 on the GPU, [F, n, 3], or [N, 3] with an int32 query_offset [F + 1] (the conventions of closest_points).  verts:
    [F, V, 3] f32 on the same GPU (a view whose frames are farther apart than 3 V floats is used without a copy).  faces: int32
    [n_faces, 3] with ids in [0, V): a HOST array or CPU tensor (its content is hashed on every call to find the kept handle of
    the (device, topology); a CUDA tensor is accepted but copied to the host first, which synchronises), or an api.Surface, which
    skips both (SurfaceTerm does that).  dist2 is differentiable with respect to points and verts at the fixed (index, bary);
    index and bary carry no gradient.  Runs on torch.cuda.current_stream(); with host faces or an api.Surface there is no host
    synchronisation (bodyfit_closest_surface_device and its _vjp_device, k_closest_surface.hip).  Calls on one topology share a workspace: interleaving them on several streams at once needs the
    caller's own ordering.

    point_normals: None (the search by distance alone), or a direction per point, f32 on the same GPU in the shape of points
    ([N, 3] with an offset, [F, n, 3] without; made contiguous).  A point may then only match a triangle with an area whose face
    normal n, in the orientation of faces, has n . m >= min_cos (a Python float); a point without such a triangle gets -1, +inf
    and zeros (bodyfit_closest_surface_oriented_device).  The directions are used as given (pass unit vectors) and carry no
    gradient: a point_normals that requires grad is a ValueError."""
    if point_normals is not None:
        _packed_normals(point_normals, points)   # (the checks, before autograd sees the tensor)
        min_cos = float(min_cos)
    return _ClosestSurface.apply(points, verts, faces, query_offset, point_normals, min_cos)


class SurfaceTerm(_TermHandles, torch.nn.Module):
    """The scan -> surface data term of a sequence: sum over the target points of rho(squared distance to the closest point on
    the frame's triangles).

    points: [N, 3] f32 on the GPU with offset, int32 [F + 1], or [F, n, 3] with offset None.  faces: int32 [n_faces, 3].
    trunc = tau: rho(s) = min(s, tau^2); None: rho(s) = s.  normals: None, or a direction per point in the shape of points, with
    min_cos the point_normals / min_cos of closest_surface: only normal-compatible triangles are matched.  term(verts), verts
    [F, V, 3] f32 (SMPLLayer's first output), returns the f64 cost; a point without a counterpart (index -1: no faces, or no
    compatible triangle) costs nothing."""

    def __init__(self, points: torch.Tensor, offset: torch.Tensor | None, faces, trunc: float | None = None,
                 normals: torch.Tensor | None = None, min_cos: float = 0.0):
        super().__init__()
        _point_set("points", points, offset)   # the checks
        if normals is not None:
            _packed_normals(normals, points)
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        f = _host_faces(faces)
        self.register_buffer("points", points.detach())
        self.register_buffer("offset", offset.detach() if offset is not None else None)
        self.faces = f.copy()                    # the term's own topology: later changes to the caller's array do not reach it
        self.register_buffer("normals", normals.detach().contiguous() if normals is not None else None)
        self.min_cos = float(min_cos)
        self.trunc = None if trunc is None else float(trunc)
        self._offset_host = None

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        faces = self.faces
        if isinstance(verts, torch.Tensor) and verts.is_cuda and verts.ndim == 3:
            faces = self._handle_for(verts)
        dist2, index, _ = closest_surface(self.points, verts, faces, query_offset=self.offset, point_normals=self.normals,
                                          min_cos=self.min_cos)
        return _rho_sum(dist2, index, self.trunc)

    def normal_equations(self, layer: "SMPLLayer", x: torch.Tensor, beta: torch.Tensor, mode: str = "point",
                         frame_chunk: int = 32, offsets=None):
        """The Gauss-Newton normal equations of the term at (x, beta): (cost, g [F, P], H [F, P, P]), f64, P = 76 + nS in the
        column order of SMPLLayer.jacobian, per frame.  With a shared beta the caller sums the beta rows and columns (76 ..) of g
        and H over the frames, the convention of bodyfit_frame_normals.

        mode "point": the residual of a scan point is r_i = p_i - c_i, c_i its closest surface point, the cost 1/2 sum w_i |r_i|^2
        = 1/2 term(verts), truncation as the weight w_i = [dist2_i < tau^2] (a truncated point costs its constant 1/2 tau^2).
        mode "plane": r_i = d_i . (p_i - c_i) with d_i the unit normal of the matched face at the current vertices, held fixed
        (point-to-plane ICP); a face without an area gets weight 0.  g and H are those of 1/2 |r|^2, as Ceres and
        FitObjective.cost count: g = J^T dcost/dverts equals the reverse-mode gradient of the same cost through the layer, and
        H = sum_i w_i (dr_i/dtheta)^T (dr_i/dtheta) at the fixed correspondence.

        Order: the forward and the term's search (oriented when the term has normals), then frame_chunk frames at a time the dense
        vertex Jacobian (layer's forward_jvp_device with the unit tangents, into ONE workspace [frame_chunk, P, V, 3] f32 that is
        reused) and surface_gram on it: nothing here grows with F P V (torch's temporaries of the rows grow with the number of
        scan points, the library's buffers with frame_chunk).  A layer with a per-frame R0 gives every chunk a problem of its
        own, one at a time (SMPLLayer.chunk_problem): a create and a destroy, with a device synchronisation, per chunk.  No
        autograd; on torch.cuda.current_stream().  offsets (as SMPLLayer.forward's): the equations of pose and shape at the
        displaced body, the offsets held constant (they have no columns)."""
        if mode not in ("point", "plane"):
            raise ValueError('mode must be "point" or "plane"')
        return _normal_equations(self, layer, x, beta, frame_chunk, lambda verts: self._jobs(verts, mode), offsets)

    def _jobs(self, verts, mode):
        F, V = verts.shape[0], verts.shape[1]
        dev = verts.device
        handle = self._handle_for(verts)
        dist2, index, bary = closest_surface(self.points, verts, handle, query_offset=self.offset, point_normals=self.normals,
                                             min_cos=self.min_cos)
        _, qs, _, nq = _point_set("points", self.points, self.offset)
        v, vs, _, _ = _point_set("verts", verts, None)
        keep = index >= 0
        cut = None
        if self.trunc is not None:
            cut = keep & ~(dist2 < self.trunc * self.trunc)
            keep = keep & (dist2 < self.trunc * self.trunc)
        if mode == "point":
            weight = keep.to(torch.float32)
            cost = 0.5 * _rho_sum(dist2, index, self.trunc)
            rhs = torch.zeros((F, V, 3), dtype=torch.float32, device=dev)
            if nq > 0 and V > 0:
                handle.vjp_device(qs, v.data_ptr(), vs.frame_stride, F, nq, index.data_ptr(), bary.data_ptr(),
                                  (0.5 * weight).data_ptr(), None, rhs.data_ptr(), _stream())
            return cost, rhs, [_GramJob(handle, self.points, self.offset, _host_offset(self), index, bary, weight, None)]
        # point-to-plane: the matched face's unit normal at the current vertices, in f64
        faces = torch.from_numpy(self.faces).to(dev).long()
        if self.offset is None:
            frame = torch.arange(F, device=dev).repeat_interleave(self.points.shape[1])
        else:
            off = self.offset.long()
            frame = torch.repeat_interleave(torch.arange(F, device=dev), off[1:] - off[:-1], output_size=nq)
        ids = faces[index.clamp(min=0).long()] if faces.shape[0] > 0 else torch.zeros((nq, 3), dtype=torch.long, device=dev)
        corners = verts[frame[:, None], ids].double()                     # [N, 3 corners, 3]
        n = torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
        length = n.norm(dim=1)
        flat = ~(length > 1e-30)
        d = torch.where(flat[:, None], torch.zeros_like(n), n / length.clamp(min=1e-30)[:, None])
        keep = keep & ~flat
        w = keep.double()
        c = (bary.double()[:, :, None] * corners).sum(dim=1)
        r = (d * (self.points.reshape(-1, 3).double() - c)).sum(dim=1)
        r = torch.where(keep, r, torch.zeros_like(r))
        cost = 0.5 * (w * r * r).sum()
        if cut is not None:
            cost = cost + 0.5 * self.trunc * self.trunc * (cut & ~flat).double().sum()
        # dcost/dverts = -sum_i w_i r_i b_ia d_i at corner a: index_put_ with accumulate adds duplicates in a fixed order
        vals = -(w * r)[:, None, None] * bary.double()[:, :, None] * d[:, None, :]
        rhs = torch.zeros((F * V, 3), dtype=torch.float64, device=dev)
        if nq > 0:
            rhs.index_put_(((frame[:, None] * V + ids).reshape(-1),), vals.reshape(-1, 3), accumulate=True)
        rhs = rhs.to(torch.float32).view(F, V, 3)
        job = _GramJob(handle, self.points, self.offset, _host_offset(self), index, bary, keep.to(torch.float32),
                       d.to(torch.float32).contiguous())
        return cost, rhs, [job]


def _host_offset(term):
    """the term's ragged offset on the host (None: uniform), copied once: a synchronisation"""
    if term.offset is None:
        return None
    if term._offset_host is None:
        term._offset_host = term.offset.detach().cpu().numpy().astype(np.int64)
    return term._offset_host


class _GramJob:
    """one surface_gram call per frame chunk: a topology handle, the rows' point set and their (index, bary, weight, direction)"""

    def __init__(self, handle, points, offset, host_offset, index, bary, weight, direction):
        self.handle, self.points, self.offset, self.host_offset = handle, points, offset, host_offset
        self.index, self.bary, self.weight, self.direction = index, bary, weight, direction

    def chunk(self, f0: int, f1: int):
        """(points, offset, rows) of frames f0 .. f1 - 1"""
        if self.offset is None:
            n = self.points.shape[1]
            return self.points[f0:f1], None, slice(f0 * n, f1 * n)
        r0, r1 = int(self.host_offset[f0]), int(self.host_offset[f1])
        return self.points[r0:r1], (self.offset[f0:f1 + 1] - r0).to(torch.int32), slice(r0, r1)


def surface_gram(jac: torch.Tensor, points: torch.Tensor, index: torch.Tensor, bary: torch.Tensor, faces,
                 query_offset: torch.Tensor | None = None, weight: torch.Tensor | None = None,
                 direction: torch.Tensor | None = None, rhs: torch.Tensor | None = None):
    """Per frame the normal equations of the scan rows at the fixed correspondence (index, bary) (closest_surface's outputs):
    (H [F, P, P] f64, g [F, P] f64 or None).  With A_i[:, p] = sum_a bary[i, a] jac[f, p, faces[index[i], a]],
    H[f, p, q] = sum_i weight_i A_i[:, p] . A_i[:, q], or sum_i weight_i (d_i . A_i[:, p]) (d_i . A_i[:, q]) with direction;
    g[f, p] = sum_v jac[f, p, v] . rhs[f, v] (None without rhs).  Rows with index -1 or weight 0 contribute nothing.

    jac: [F, P, V, 3] f32 on the GPU, SMPLLayer.jacobian's first output; a view whose tangent rows are farther apart than 3 V
    floats is used in place.  points / query_offset: the rows' point set (conventions of closest_surface; only its frame
    structure is used).  index [N] int32, bary [N, 3] f32, weight [N] f32 (None: 1), direction [N, 3] f32 unit vectors (None:
    point-to-point), rhs [F, V, 3] f32, all on jac's GPU.  faces: as for closest_surface (an api.Surface skips the hashing).
    |H - H*| <= 2^-12 H^ (include/bodyfit.h derives it); H is exactly symmetric and bit-identical from run to run and whatever F.
    index must not have been written since the search that produced it: a closest_surface call whose verts required grad keeps
    the grouping of its rows by face in the handle, and a later call with the same index tensor (same address, frames and row
    counts) uses that grouping as it is.  To drop rows, pass weight 0, or give a NEW tensor (index.clone() with -1 written).
    No autograd; on torch.cuda.current_stream() (bodyfit_surface_gram_device, k_surface_gram.hip)."""
    named = (("jac", jac, torch.float32), ("index", index, torch.int32), ("bary", bary, torch.float32),
             ("weight", weight, torch.float32), ("direction", direction, torch.float32), ("rhs", rhs, torch.float32))
    for name, t, dtype in named:
        if t is None and name in ("weight", "direction", "rhs"):
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {str(dtype).replace('torch.', '')}")
    if jac.ndim != 4 or jac.shape[3] != 3 or jac.shape[1] < 1:
        raise ValueError(f"jac must be [F, P, V, 3], got {tuple(jac.shape)}")
    q, qs, F, nq = _point_set("points", points, query_offset)
    Fj, P, V = jac.shape[0], jac.shape[1], jac.shape[2]
    if Fj != F:
        raise ValueError(f"points has {F} frames, jac has {Fj}")
    for name, t, shape in (("index", index, (nq,)), ("bary", bary, (nq, 3)), ("weight", weight, (nq,)),
                           ("direction", direction, (nq, 3)), ("rhs", rhs, (F, V, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    for name, t, _ in named:
        if t is not None and (not t.is_cuda or t.device != q.device):
            raise ValueError(f"{name} must be on the GPU of points")
    handle = _surface_handle(q.device.index, V, faces)
    # the Jacobian in place when its [V, 3] blocks are dense and the rows and frames are far enough apart
    dense = jac.stride(3) == 1 and jac.stride(2) == 3 and (P == 1 or jac.stride(1) >= 3 * V)
    row = jac.stride(1) if P > 1 else 3 * V
    if not dense or V == 0 or (F > 1 and jac.stride(0) < P * row):
        jac = jac.contiguous()
        row = 3 * V
    frame = jac.stride(0) if F > 1 and jac.stride(0) >= P * row else P * row
    index, bary = index.contiguous(), bary.contiguous()
    weight = weight.contiguous() if weight is not None else None
    direction = direction.contiguous() if direction is not None else None
    rhs = rhs.contiguous() if rhs is not None else None
    H = torch.empty((F, P, P), dtype=torch.float64, device=q.device)
    g = torch.empty((F, P), dtype=torch.float64, device=q.device) if rhs is not None else None
    if F > 0:
        handle.gram_device(qs, F, nq, index.data_ptr(), bary.data_ptr(), weight.data_ptr() if weight is not None else None,
                           direction.data_ptr() if direction is not None else None, jac.data_ptr(), P, row, frame,
                           rhs.data_ptr() if rhs is not None else None, 3 * V, H.data_ptr(),
                           g.data_ptr() if g is not None else None, _stream())
    return H, g


def _chunk_offsets(offsets, f0: int, V: int) -> dict:
    """a chunk problem's offset arguments for the frames from f0 on (nothing without offsets: today's call)"""
    if offsets is None:
        return {}
    if offsets.ndim == 2:
        return {"d_offsets_ptr": offsets.data_ptr(), "offsets_frame_stride": 0}
    return {"d_offsets_ptr": offsets[f0:].data_ptr(), "offsets_frame_stride": 3 * V}


def _normal_equations(term, layer, x, beta, frame_chunk, jobs_of, offsets=None):
    """the shared body of the terms' normal_equations: forward, the term's jobs, then the Jacobian and the Gram chunk by chunk
    (offsets: constant per-vertex displacements of the forward and of the Jacobian's point, sliced with the frames)"""
    if not isinstance(layer, SMPLLayer):
        raise TypeError("layer must be an SMPLLayer")
    if not isinstance(frame_chunk, int) or isinstance(frame_chunk, bool) or frame_chunk < 1:
        raise ValueError("frame_chunk must be a positive int")
    F = layer._check(x, beta)
    _, _, Ft, _ = _point_set("points", term.points, term.offset)
    if Ft != F:
        raise ValueError(f"the term has {Ft} frames, x has {F}")
    nP, nS, V = api.N_FRAME_PARAMS, layer.model.n_shape, layer.model.n_verts
    P = nP + nS
    with torch.no_grad():
        x, beta = x.detach().contiguous(), beta.detach().contiguous()
        if offsets is not None:
            offsets = layer._check_offsets(offsets, x, F).detach()
        verts, _ = layer(x, beta, offsets)
        cost, rhs, jobs = jobs_of(verts)
        dev = x.device
        chunk = min(frame_chunk, F)
        work = torch.empty((chunk, P, V, 3), dtype=torch.float32, device=dev)
        eye = torch.eye(P, dtype=torch.float64, device=dev)
        tan_x = eye[:, :nP].expand(chunk, P, nP).contiguous()
        tan_beta = None
        if nS > 0:
            tan_beta = eye[:, nP:].expand(chunk, P, nS).contiguous() if layer.beta_per_frame else eye[:, nP:].contiguous()
        H = torch.empty((F, P, P), dtype=torch.float64, device=dev)
        g = torch.empty((F, P), dtype=torch.float64, device=dev)
        for f0 in range(0, F, chunk):
            f1 = min(f0 + chunk, F)
            n = f1 - f0
            b = beta[f0:f1] if layer.beta_per_frame else beta
            # (tan_x and a per-frame tan_beta are [chunk, P, .]: their first n frames are the unit tangents of n frames)
            layer.chunk_problem(f0, n).forward_jvp_device(x[f0:f1].data_ptr(), b.data_ptr(), P, tan_x.data_ptr(),
                                                          tan_beta.data_ptr() if tan_beta is not None else None, None,
                                                          work.data_ptr(), 3 * V, _stream(), **_chunk_offsets(offsets, f0, V))
            for k, job in enumerate(jobs):
                pts, off, rows = job.chunk(f0, f1)
                Hc, gc = surface_gram(work[:n], pts, job.index[rows], job.bary[rows], job.handle, query_offset=off,
                                      weight=job.weight[rows],
                                      direction=job.direction[rows] if job.direction is not None else None,
                                      rhs=rhs[f0:f1] if k == 0 else None)
                if k == 0:
                    H[f0:f1] = Hc
                    g[f0:f1] = gc
                else:
                    H[f0:f1] += Hc
    return cost, g, H
