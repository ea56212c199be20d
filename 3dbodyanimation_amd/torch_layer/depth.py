"""The depth camera: the render, mesh visibility, the depth-map term and the projective depth residual.

    depth, face, bary = render_depth(verts, faces, intr, (H, W))        # what the camera sees of the posed mesh (no gradient)
    vis = visible_vertices(verts, faces, intr, (H, W))                  # bool [F, V]
    term = DepthMapTerm(depth_map, intr, faces, trunc=0.1, min_cos=0.2) # an RGB-D frame: both directions, the second one gated

render_depth is bodyfit_raster_render_device (k_raster.hip: a z-buffer over faces binned to screen tiles, decided in f64),
visible_vertices adds bodyfit_raster_visibility_device.  DepthMapTerm back-projects a depth map once, matches its points to
sensor-facing triangles (SurfaceTerm with the directions towards the sensor) and pulls only the VISIBLE vertices to the points.

    z, index, bary, direction = depth_at_pixels(verts, faces, intr, (H, W))   # the rendered face's ray-plane depth, with a gradient
    term = DepthResidualTerm(depth_map, intr, faces, trunc=0.05, min_cos=0.2)   # projective: model depth - sensor depth per pixel
    cost, g, H = term.normal_equations(layer, x, beta)

The projective term of a calibrated depth camera needs no search: its correspondence is the z-buffer.  depth_at_pixels renders the
face image from verts.detach() and evaluates, per pixel, the intersection of the ray with the plane of the face under it
(bodyfit_raster_depth_rows_device); at the fixed (face, ray) dz/dcorner_a = bary_a direction, summed into the vertices without
float atomics by bodyfit_surface_rows_vjp_device.  A depth row has the shape of a point-to-plane row, so the normal equations are
surface_gram's.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import _TermHandles, _grad_like, _host_faces, _point_set, _raster_handle, _rho_sum, _stream, _surface_handle
from .scan import SurfaceTerm, _GramJob, _host_offset, _normal_equations, closest_points


def _render(verts, faces, intr, size, z_near, cull_backfaces, want_bary):
    # (not _check_verts: a tensor that is not on the GPU gets the first message here, and before its shape is looked at)
    if not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32 or not verts.is_cuda:
        raise TypeError("verts must be a float32 tensor on the GPU")
    if verts.ndim != 3 or verts.shape[2] != 3:
        raise ValueError(f"verts must be [F, V, 3], got {tuple(verts.shape)}")
    if len(intr) != 4 or len(size) != 2:
        raise ValueError("intr is (fx, fy, cx, cy), size is (height, width)")
    v, vs, F, _ = _point_set("verts", verts.detach(), None)
    H, W = int(size[0]), int(size[1])
    handle = _raster_handle(v.device.index, v.shape[1], faces, (H, W))
    depth = torch.empty((F, H, W), dtype=torch.float32, device=v.device)
    face = torch.empty((F, H, W), dtype=torch.int32, device=v.device)
    bary = torch.empty((F, H, W, 3), dtype=torch.float32, device=v.device) if want_bary else None
    with torch.cuda.device(v.device):
        handle.render_device(v.data_ptr(), vs.frame_stride, F, [float(a) for a in intr], depth.data_ptr(), face.data_ptr(),
                             bary.data_ptr() if want_bary else None, z_near=float(z_near), cull_backfaces=cull_backfaces,
                             stream=_stream())
    return handle, depth, face, bary


def render_depth(verts: torch.Tensor, faces, intr, size, z_near: float = 0.1, cull_backfaces: bool = False):
    """What the camera intr = (fx, fy, cx, cy) sees of the posed meshes verts [F, V, 3] f32 (GPU; a view with a frame stride of its
    own is used in place) with the triangles faces (int32 [n_faces, 3], host array or tensor), in an image of size = (height,
    width): (depth [F, H, W] f32, +inf where empty; face [F, H, W] int32, -1 where empty; bary [F, H, W, 3] f32, the
    screen-space barycentric weights of the pixel in that face, 0 where empty).  Pixel (i, j) is the ray through (u, v) = (j, i)
    in the convention of synth.project; a face with a corner in front of z_near is dropped whole; cull_backfaces keeps only
    faces whose normal, in the orientation of faces, points to the camera.  The z-buffer, its tie rule and its error bounds are
    those of bodyfit_raster_render_device (include/bodyfit.h, k_raster.hip).

    NOT differentiable: the outputs carry no gradient, whatever verts requires (depth_at_pixels gives the ray-plane depth of the
    rendered face under a pixel with its gradient at the fixed (face, ray)).  Runs on torch.cuda.current_stream(), with one 8-byte read-back per call;
    the handle of (device, V, faces, size) is kept between calls, and calls that share one share its workspace."""
    _, depth, face, bary = _render(verts, faces, intr, size, z_near, cull_backfaces, True)
    return depth, face, bary


def visible_vertices(verts: torch.Tensor, faces, intr, size, z_near: float = 0.1, cull_backfaces: bool = False):
    """bool [F, V]: the vertices that are a corner of a face that owns at least one pixel of render_depth(verts, faces, intr,
    size, ...) (bodyfit_raster_visibility_device on the rendered face ids).  No gradient."""
    handle, _, face, _ = _render(verts, faces, intr, size, z_near, cull_backfaces, False)
    F, V = verts.shape[0], verts.shape[1]
    vis = torch.empty((F, V), dtype=torch.uint8, device=face.device)
    with torch.cuda.device(face.device):
        handle.visibility_device(face.data_ptr(), F, None, vis.data_ptr(), _stream())
    return vis.bool()


class DepthMapTerm(torch.nn.Module):
    """The data term of a single-view depth map, both directions, from terms that are already differentiable.

    depth: [F, H, W] f32 on the GPU, metres along the optical axis; a pixel that is not finite or not > 0 holds nothing.  The
    constructor back-projects the valid pixels through intr = (fx, fy, cx, cy) (pixel (i, j) at (u, v) = (j, i)) into a ragged
    point set and forms their unit directions towards the sensor, once.  term(verts), verts [F, V, 3] f32, returns the f64 cost
      data -> model: SurfaceTerm(points, offset, faces, trunc, normals=directions, min_cos)(verts): a depth pixel is matched to the
                     closest point of a triangle that faces the sensor (n . direction >= min_cos);
      model -> data (model_to_data): sum over the VISIBLE vertices of rho(squared distance to the closest back-projected point of
                     the frame), rho(s) = min(s, trunc^2).  Visibility is rendered from verts.detach() at the depth map's size
                     (visible_vertices, z_near): the back of the body and what a limb hides are not pulled to a scan that cannot
                     contain them, which PointCloudTerm(bidirectional=True) does.
    A frame without a valid pixel, or without a visible vertex, contributes 0 to the direction that lacks it.  Gradients are
    those of closest_surface and closest_points at the fixed correspondence; visibility is piecewise constant and carries none.
    The mask gather sizes its result on the host: one synchronisation per evaluation, beside the render's own read-back."""

    def __init__(self, depth: torch.Tensor, intr, faces, trunc: float | None = None, min_cos: float = 0.0,
                 z_near: float = 0.1, model_to_data: bool = True):
        super().__init__()
        if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or not depth.is_cuda or depth.ndim != 3:
            raise TypeError("depth must be a float32 tensor [F, H, W] on the GPU")
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        depth = depth.detach()
        F, H, W = depth.shape
        fx, fy, cx, cy = (float(a) for a in intr)
        valid = torch.isfinite(depth) & (depth > 0)
        f, i, j = torch.nonzero(valid, as_tuple=True)          # frame-major, then row-major: the packed order of a ragged set
        z = depth[f, i, j].double()
        p = torch.stack(((j.double() - cx) / fx * z, (i.double() - cy) / fy * z, z), dim=1)
        toward = -p / p.norm(dim=1, keepdim=True)
        offset = torch.zeros(F + 1, dtype=torch.int32, device=depth.device)
        offset[1:] = valid.reshape(F, -1).sum(dim=1).cumsum(0).to(torch.int32)
        self.intr, self.size, self.z_near = (fx, fy, cx, cy), (int(H), int(W)), float(z_near)
        self.model_to_data = bool(model_to_data)
        self.surface = SurfaceTerm(p.to(torch.float32).contiguous(), offset, faces, trunc=trunc,
                                   normals=toward.to(torch.float32).contiguous(), min_cos=min_cos)

    @property
    def points(self):
        return self.surface.points

    @property
    def offset(self):
        return self.surface.offset

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        cost = self.surface(verts)
        if self.model_to_data:
            vis = visible_vertices(verts, self.surface.faces, self.intr, self.size, z_near=self.z_near)
            query = verts[vis]                                   # [n_visible, 3], frame after frame
            q_offset = torch.zeros(vis.shape[0] + 1, dtype=torch.int32, device=verts.device)
            q_offset[1:] = vis.sum(dim=1).cumsum(0).to(torch.int32)
            cost = cost + _rho_sum(*closest_points(query, self.points, query_offset=q_offset, ref_offset=self.offset),
                                   self.surface.trunc)
        return cost


def _pixel_rows(pixel, offset, F: int, H: int, W: int, device):
    """(pixel or None, offset or None, rows, rows per frame or None) of depth_at_pixels' pixel arguments, checked"""
    if pixel is None:
        if offset is not None:
            raise ValueError("offset needs pixel")
        return None, None, F * H * W, H * W
    if not isinstance(pixel, torch.Tensor) or pixel.dtype != torch.int32 or pixel.device != device:
        raise TypeError("pixel must be an int32 tensor on the GPU of verts")
    if offset is None:
        if pixel.ndim != 2 or pixel.shape[0] != F:
            raise ValueError(f"pixel without an offset must be [F, n] with F = {F}, got {tuple(pixel.shape)}")
        return pixel.contiguous(), None, pixel.numel(), pixel.shape[1]
    if not isinstance(offset, torch.Tensor) or offset.dtype != torch.int32 or offset.device != device:
        raise TypeError("offset must be an int32 tensor on the GPU of verts")
    if pixel.ndim != 1 or offset.ndim != 1 or offset.shape[0] != F + 1:
        raise ValueError(f"pixel with an offset must be [N] and offset [F + 1] with F = {F}")
    return pixel.contiguous(), offset.contiguous(), pixel.shape[0], None


class _DepthAtPixels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, intr, size, pixel, offset, z_near, cull_backfaces, surface):
        raster, _, face_img, _ = _render(verts, faces, intr, size, z_near, cull_backfaces, False)
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        H, W = int(size[0]), int(size[1])
        dev = v.device
        pixel, offset, N, per_frame = _pixel_rows(pixel, offset, F, H, W, dev)
        shape = (F, H, W) if pixel is None else (N,)
        index = torch.empty(shape, dtype=torch.int32, device=dev)
        z = torch.empty(shape, dtype=torch.float32, device=dev)
        bary = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
        direction = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
        if N > 0:
            with torch.cuda.device(dev):
                raster.depth_rows_device(v.data_ptr(), vs.frame_stride, F, [float(a) for a in intr], face_img.data_ptr(),
                                         pixel.data_ptr() if pixel is not None else None,
                                         offset.data_ptr() if offset is not None else None, N, index.data_ptr(), z.data_ptr(),
                                         bary.data_ptr(), direction.data_ptr(), _stream())
        if ctx.needs_input_grad[0]:
            if surface is None:
                surface = _surface_handle(dev.index, v.shape[1], faces)
            # (the rows' frame structure as a point set; its xyz pointer is never read)
            if offset is not None:
                rows = api.PointSet.ragged(index.data_ptr(), offset.data_ptr())
                rows._keep = offset
            else:
                rows = api.PointSet.uniform(index.data_ptr(), per_frame, 3 * per_frame)
            ctx.rows = (rows, vs, F, N, surface)
            ctx.save_for_backward(v, index, bary, direction)
        ctx.mark_non_differentiable(index, bary, direction)
        return z, index, bary, direction

    @staticmethod
    @once_differentiable
    def backward(ctx, g_z, _g_index, _g_bary, _g_dir):
        v, index, bary, direction = ctx.saved_tensors
        rows, vs, F, N, surface = ctx.rows
        gv = _grad_like(v, vs)
        if g_z is None or N == 0 or v.shape[1] == 0:
            gv.zero_()
        else:
            # a void row (z = +inf) takes no gradient: its upstream is masked, so that an inf x 0 upstream cannot make a NaN
            coef = torch.where(index >= 0, g_z.to(torch.float32), torch.zeros((), dtype=torch.float32, device=v.device))
            coef = coef.contiguous()
            with torch.cuda.device(v.device):
                surface.rows_vjp_device(rows, F, N, index.data_ptr(), bary.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                        gv.data_ptr(), vs.frame_stride, _stream())
        return gv, None, None, None, None, None, None, None, None


def depth_at_pixels(verts: torch.Tensor, faces, intr, size, pixel: torch.Tensor | None = None,
                    offset: torch.Tensor | None = None, z_near: float = 0.1, cull_backfaces: bool = False, _surface=None):
    """The model's depth along the rays of given pixels, differentiable at the rendered correspondence: (z, index, bary,
    direction).  The face image is rendered from verts.detach() exactly as render_depth does (same arguments, same handle, one
    8-byte read-back); then for every row, a pixel (i, j) of a frame, with the face t that image holds there:
      z          f32: the z of the intersection of the ray d = ((j - cx) / fx, (i - cy) / fy, 1) with the plane of face t, +inf
                 for a void row (empty pixel, a pixel index outside the image, a non-finite corner, a face without an area or
                 edge-on to the ray); inside the face this is the rendered depth, to the sum of the two contracts;
      index      int32: t, or -1;
      bary       f32 [.., 3]: the OBJECT-space barycentrics of the intersection (not render_depth's screen-space ones; not
                 clamped: slightly negative on the silhouette's coverage band), 0 for a void row;
      direction  f32 [.., 3]: m = n / (n . d), with dz/dverts[faces[t][a]] = bary_a m; 1 / (|m| |d|) is the cosine between the face
                 normal and the ray.
    pixel None: every pixel, the outputs are [F, H, W] (and [F, H, W, 3]).  pixel int32 [F, n] (GPU): n linear indices i W + j
    per frame; pixel int32 [N] with offset int32 [F + 1]: ragged, frame after frame; outputs packed like pixel.
    z carries a gradient to verts at the fixed (face, ray) (bodyfit_surface_rows_vjp_device with coef = the upstream gradient:
    deterministic, no float atomics); void rows receive none.  index, bary and direction carry no gradient.  faces: a host int32
    [n_faces, 3] array or tensor (hashed on every call, as render_depth).  The definitions, their error bounds and the
    derivation: bodyfit_raster_depth_rows_device, include/bodyfit.h.  Runs on torch.cuda.current_stream()."""
    return _DepthAtPixels.apply(verts, faces, intr, size, pixel, offset, float(z_near), bool(cull_backfaces), _surface)


class DepthResidualTerm(_TermHandles, torch.nn.Module):
    """The PROJECTIVE data term of a calibrated depth camera: model depth minus sensor depth along the pixel's ray, at the
    correspondence the z-buffer already holds (no closest-point search).

    depth: [F, H, W] f32 on the GPU, metres along the optical axis; a pixel that is not finite or not > 0 holds nothing.  The
    constructor compacts the valid pixels once into (pixel, offset, sensor), frame-major then row-major (the order of
    DepthMapTerm's points; `points` are the same back-projections, kept for the rows' frame structure).  term(verts), verts
    [F, V, 3] f32, returns the f64 cost  sum_i rho(r_i^2),  r_i = z_i - sensor_i  with z_i = depth_at_pixels(verts, ...) at the
    pixel, rho(s) = min(s, trunc^2) (trunc None: rho(s) = s), over the rows that have a model face under them (index >= 0)
    and pass the grazing gate 1 / (|m_i| |d_i|) >= min_cos, the cosine between the face normal and the ray: piecewise constant,
    no gradient.  A sensor pixel with no model face under it contributes 0, and so does a model pixel without a sensor value:
    pulling the outline of the model onto the outline of the data is the business of a silhouette term, not of this one.  A
    frame without a valid pixel contributes 0.  The gradient is that of depth_at_pixels: at the fixed (face, ray)."""

    def __init__(self, depth: torch.Tensor, intr, faces, trunc: float | None = None, min_cos: float = 0.0,
                 z_near: float = 0.1):
        super().__init__()
        if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or not depth.is_cuda or depth.ndim != 3:
            raise TypeError("depth must be a float32 tensor [F, H, W] on the GPU")
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        depth = depth.detach()
        F, H, W = depth.shape
        fx, fy, cx, cy = (float(a) for a in intr)
        valid = torch.isfinite(depth) & (depth > 0)
        f, i, j = torch.nonzero(valid, as_tuple=True)          # frame-major, then row-major
        sensor = depth[f, i, j]
        dx, dy = (j.double() - cx) / fx, (i.double() - cy) / fy
        z = sensor.double()
        offset = torch.zeros(F + 1, dtype=torch.int32, device=depth.device)
        offset[1:] = valid.reshape(F, -1).sum(dim=1).cumsum(0).to(torch.int32)
        self.intr, self.size, self.z_near = (fx, fy, cx, cy), (int(H), int(W)), float(z_near)
        self.trunc = None if trunc is None else float(trunc)
        self.min_cos = float(min_cos)
        self.faces = _host_faces(faces).copy()
        self.register_buffer("pixel", (i * W + j).to(torch.int32).contiguous())
        self.register_buffer("offset", offset)
        self.register_buffer("sensor", sensor.contiguous())
        self.register_buffer("ray_length", torch.sqrt(dx * dx + dy * dy + 1.0))
        self.register_buffer("points", torch.stack((dx * z, dy * z, z), dim=1).to(torch.float32).contiguous())
        self._offset_host = None

    def rows(self, verts: torch.Tensor):
        """depth_at_pixels at the term's pixels: (z, index, bary, direction), packed like `sensor`"""
        surface = None
        if isinstance(verts, torch.Tensor) and verts.is_cuda and verts.ndim == 3:
            surface = self._handle_for(verts)
        return depth_at_pixels(verts, self.faces, self.intr, self.size, pixel=self.pixel, offset=self.offset,
                               z_near=self.z_near, _surface=surface)

    def residuals(self, z, index, direction):
        """(keep [N] bool: a model face under the pixel that passes the gate; r [N] f64: z - sensor there, 0 elsewhere;
        |m| [N] f64)"""
        length = direction.double().norm(dim=1)
        keep = index >= 0
        cos = 1.0 / torch.where(keep, length * self.ray_length, torch.ones_like(length))
        keep = keep & (cos >= self.min_cos)
        r = torch.where(keep, z.double() - self.sensor.double(), torch.zeros_like(length))
        return keep, r, length

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        z, index, _, direction = self.rows(verts)
        _, r, _ = self.residuals(z, index, direction)
        s = r * r
        if self.trunc is not None:                               # (not _truncated_cost: nothing is counted here)
            s = torch.clamp(s, max=self.trunc * self.trunc)
        return s.sum()

    def normal_equations(self, layer: "SMPLLayer", x: torch.Tensor, beta: torch.Tensor, frame_chunk: int = 32, offsets=None):
        """The Gauss-Newton normal equations of the term at (x, beta): (cost, g [F, P], H [F, P, P]), f64, in the conventions of
        SurfaceTerm.normal_equations.  cost = 1/2 sum_i w_i r_i^2 + 1/2 trunc^2 (the truncated rows) = 1/2 term(verts), w_i the gate
        and the truncation indicator [r_i^2 < trunc^2]; a depth row is a point-to-plane row with the weights bary_i on its face's
        corners, the unit direction m_i / |m_i| and the weight w_i |m_i|^2 (dr_i/dverts = bary_ia m_i), so H = sum_i w_i
        (dr_i/dtheta)^T (dr_i/dtheta) comes from surface_gram as it is, and g = J^T rhs with rhs = sum_i w_i r_i bary_ia m_i from
        the rows VJP: the reverse-mode gradient of the same cost through the layer."""
        return _normal_equations(self, layer, x, beta, frame_chunk, self._jobs, offsets)

    def _jobs(self, verts):
        F, V = verts.shape[0], verts.shape[1]
        handle = self._handle_for(verts)
        z, index, bary, direction = self.rows(verts)
        keep, r, length = self.residuals(z, index, direction)
        w = keep
        cost = torch.zeros((), dtype=torch.float64, device=verts.device)
        if self.trunc is not None:
            w = keep & (r * r < self.trunc * self.trunc)
            cost = 0.5 * self.trunc * self.trunc * (keep & ~w).double().sum()
        wd = w.double()
        cost = cost + 0.5 * (wd * r * r).sum()
        N = index.shape[0]
        rhs = torch.zeros((F, V, 3), dtype=torch.float32, device=verts.device)
        if V > 0 and F > 0:
            coef = (wd * r).to(torch.float32).contiguous()
            rows = api.PointSet.ragged(index.data_ptr(), self.offset.data_ptr())
            with torch.cuda.device(verts.device):
                handle.rows_vjp_device(rows, F, N, index.data_ptr(), bary.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                       rhs.data_ptr(), 3 * V, _stream())
        safe = torch.where(w, length, torch.ones_like(length))
        unit = torch.where(w[:, None], direction.double() / safe[:, None], torch.zeros((), dtype=torch.float64, device=verts.device))
        weight = torch.where(w, length * length, torch.zeros_like(length))
        job = _GramJob(handle, self.points, self.offset, _host_offset(self), index, bary, weight.to(torch.float32).contiguous(),
                       unit.to(torch.float32).contiguous())
        return cost, rhs, [job]
