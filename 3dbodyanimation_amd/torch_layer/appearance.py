"""Vertex colours: the attribute render with its gradients, image sampling, colour fusion and the photometric terms.

    image, face = render_attributes(verts, faces, intr, (H, W), colours)   # the coloured avatar; a gradient to colours only
    value, valid = sample_images(video, verts, intr)                     # the frames read at the vertices, differentiable in verts
    colours, weight = fuse_vertex_colours(video, verts, faces, intr, owner=True)   # [V, C]: the person's colours on the mesh
    term = PhotometricTerm(video, intr, faces, trunc=30.0, owner=True)   # sum rho(|I(pi(v)) - colour_v|^2) over the visible vertices

The dense signal between the keypoints and the outline is the image itself.  render_attributes is render_depth followed by
bodyfit_raster_shade_device (k_raster_shade.hip: per-vertex attributes interpolated with the perspective-correct weights), its
backward bodyfit_surface_rows_vjp_device over the pixels.  sample_images is bodyfit_raster_sample_device (one bilinear read per
vertex and frame, u8 or f32 images, with the image gradient of the cell).  fuse_vertex_colours averages the samples of the frames
that see a vertex, weighted by the cosine to the camera; PhotometricTerm holds such colours against the frames and is
differentiable in the vertices and in the colours.

    image, face = render_attributes(verts, faces, intr, (H, W), colours, interior=True)   # ALSO differentiable in verts, inside the faces
    term = RenderedPhotometricTerm(video, intr, faces, trunc=30.0)       # sum rho(|antialias(render) - I|^2) over the pixels

interior=True adds the middle of rasterize -> interpolate -> antialias: the same image, and in the backward one row per shaded
pixel from bodyfit_raster_interp_rows_device (k_raster_rows.hip: the object-space barycentrics of the pixel's ray in its face and the
one direction that carries dL/dimage to the three corners) into bodyfit_surface_rows_vjp_device.  RenderedPhotometricTerm is
PhotometricTerm at the pixels instead of the vertices: interior and coverage gradients of one render.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import (_NO_FACES, _check_background, _check_intr_size, _check_per_vertex, _check_verts, _grad_like,
                      _host_faces, _pixel_rows_vjp, _point_set, _ragged_rows, _raster_handle, _stream, _surface_handle,
                      _truncated_cost)
from .depth import _render
from .silhouette import antialias
from .solid import vertex_normals


class _RenderAttributes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, verts, faces, intr, size, background, z_near, cull_backfaces, interior):
        raster, depth, face, bary = _render(verts, faces, intr, size, z_near, cull_backfaces, True)
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        H, W = int(size[0]), int(size[1])
        V, C = v.shape[1], attr.shape[-1]
        a = attr.detach().contiguous()
        shared = a.ndim == 2
        image = torch.empty((F, H, W, C), dtype=torch.float32, device=v.device)
        weight = torch.empty((F, H, W, 3), dtype=torch.float32, device=v.device)
        if F > 0:
            with torch.cuda.device(v.device):
                raster.shade_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, a.data_ptr(),
                                    0 if shared else V * C, C, F, background, image.data_ptr(), weight.data_ptr(), _stream())
        ctx.interior = bool(interior) and ctx.needs_input_grad[1]
        if ctx.needs_input_grad[0] or ctx.interior:
            ctx.rows = (_surface_handle(v.device.index, V, faces), F, V, C, H * W, shared)
            if ctx.interior:
                ctx.raster = (raster, vs, tuple(float(x) for x in intr))
                ctx.save_for_backward(face, weight, v, a)
            else:
                ctx.save_for_backward(face, weight)
        ctx.mark_non_differentiable(face, depth)
        return image, face, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g_image, _g_face, _g_depth):
        if not (ctx.needs_input_grad[0] or ctx.interior):       # (verts alone asks, without interior: there is nothing to give)
            return (None,) * 9
        face, weight = ctx.saved_tensors[:2]
        surface, F, V, C, ppf, shared = ctx.rows
        g = None
        if ctx.needs_input_grad[0]:
            g = torch.zeros((F, V, C), dtype=torch.float32, device=face.device)
            if g_image is not None and F * V * ppf > 0:
                gi = g_image.to(torch.float32).reshape(F * ppf, C)
                # (a row's direction has three components: C = 4 takes two calls, each with a coef and a padded direction of its own)
                for c0 in range(0, C, 3):
                    n = min(3, C - c0)
                    g[:, :, c0:c0 + n] = _pixel_rows_vjp(surface, face, weight, gi[:, c0:c0 + n], F, V)[:, :, :n]
            if shared:
                g = g.double().sum(dim=0).to(torch.float32)
        g_verts = _interior_backward(ctx, g_image) if ctx.interior else None
        return g, g_verts, None, None, None, None, None, None, None


def _interior_backward(ctx, g_image):
    """dL/dverts of _RenderAttributes through the interpolation inside the faces, at the fixed face image: the pixels the shade did
    not void as rows of bodyfit_raster_interp_rows_device, summed by ONE bodyfit_surface_rows_vjp_device call"""
    face, weight, v, a = ctx.saved_tensors
    surface, F, V, C, ppf, shared = ctx.rows
    raster, vs, intr = ctx.raster
    return _interior_rows(raster, surface, v, vs, intr, face, weight, a, 0 if shared else V * C, C, g_image)


def _interior_rows(raster, surface, v, vs, intr, face, weight, a, attr_stride, C, g_image, attr_faces=None, n_attr_rows=0):
    """the gradient in the layout of v of the interpolation rows of the pixels whose weight is not all zero: attributes a (C per
    row) by the corners' vertex ids, or (attr_faces: int32 [n_faces, 3] on the device, rows in [0, n_attr_rows)) per corner"""
    F, V, ppf = face.shape[0], v.shape[1], face.shape[1] * face.shape[2]
    dev = face.device
    gv = _grad_like(v, vs)
    N = 0
    if g_image is not None and F * V * ppf > 0:
        # the shaded pixels (their weights are >= 0 and sum to 1: not all zero), frame after frame and ascending inside a frame
        _, pixel, offset, N = _ragged_rows((weight != 0).any(dim=-1).reshape(F, ppf))
    if N == 0:
        gv.zero_()
        return gv
    gi = g_image.to(torch.float32).contiguous()
    index = torch.empty(N, dtype=torch.int32, device=dev)
    bary = torch.empty((N, 3), dtype=torch.float32, device=dev)
    direction = torch.empty((N, 3), dtype=torch.float32, device=dev)
    coef = torch.ones(N, dtype=torch.float32, device=dev)
    rows = api.PointSet.ragged(index.data_ptr(), offset.data_ptr())      # (the rows' frame structure; its xyz is never read)
    with torch.cuda.device(dev):
        if attr_faces is None:
            raster.interp_rows_device(v.data_ptr(), vs.frame_stride, F, intr, face.data_ptr(), pixel.data_ptr(), offset.data_ptr(), N,
                                      a.data_ptr(), attr_stride, C, gi.data_ptr(), None, index.data_ptr(), bary.data_ptr(),
                                      direction.data_ptr(), None, _stream())
        else:
            raster.interp_rows_indexed_device(v.data_ptr(), vs.frame_stride, F, intr, face.data_ptr(), pixel.data_ptr(),
                                              offset.data_ptr(), N, a.data_ptr(), attr_stride, C, attr_faces.data_ptr(), n_attr_rows,
                                              gi.data_ptr(), None, index.data_ptr(), bary.data_ptr(), direction.data_ptr(), None,
                                              _stream())
        surface.rows_vjp_device(rows, F, N, index.data_ptr(), bary.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                gv.data_ptr(), vs.frame_stride, _stream())
    return gv


def render_attributes(verts: torch.Tensor, faces, intr, size, attr: torch.Tensor, background=0.0, z_near: float = 0.1,
                      cull_backfaces: bool = False, interior: bool = False):
    """The per-vertex attributes attr ([V, C] shared by the frames, or [F, V, C]; f32, C in 1 .. 4: colours) of the posed meshes
    verts [F, V, 3] f32 as the camera intr sees them in an image of size = (height, width): (image [F, H, W, C] f32, face
    [F, H, W] int32).  render_depth's render (same arguments, same handle, one 8-byte read-back) followed by
    bodyfit_raster_shade_device: in a covered pixel the attributes of the face's corners with the perspective-correct weights
    w_a = (lambda_a / Z_a) / sum, elsewhere background (a float, or C floats).  The definition and its error bound:
    include/bodyfit.h.

    Differentiable in attr at the fixed render, and by default in attr ONLY: NOT differentiable in verts (neither through the
    weights nor through visibility or coverage; antialias(image, verts, ...) adds the gradient through coverage).  The backward is
    bodyfit_surface_rows_vjp_device with the pixels as rows (index = the face image,
    bary = the stored weights, coef = 1, direction = the upstream gradient, three channels per call: C = 4 takes two); shared
    attributes get the frames' gradients summed in f64.  No float atomics, no index_add_: bit-identical from run to run.

    interior=True: the same forward, launch for launch and bit for bit, is ALSO differentiable in verts through the interpolation
    INSIDE the faces, at the fixed face image and the fixed pixel rays: how a pixel's value changes as its face's corners move
    under it (a print sliding over the chest), which neither the default nor antialias carries.  The backward lists the pixels
    the shade did not void (one nonzero of its weights: one host synchronisation, as antialias), writes one "barycentric x
    direction" row per pixel whatever C (bodyfit_raster_interp_rows_device: the object-space barycentrics of the pixel's ray in
    its face and dir = -sum_a (sum_c G_c attr_a,c) h_a) and sums them into the layout of verts with one
    bodyfit_surface_rows_vjp_device call.  Not part of it: visibility and coverage (antialias), z_near and culling.  The
    gradient in attr is the same with and without it."""
    _check_verts(verts)
    _check_intr_size(intr, size)
    _check_per_vertex(attr, "attr", verts.shape[0], verts.shape[1], verts.device)
    bg = _check_background(background, attr.shape[-1])
    image, face, _ = _RenderAttributes.apply(attr, verts, faces, intr, size, bg, float(z_near), bool(cull_backfaces), bool(interior))
    return image, face


def _check_images(images):
    """images as [F, H, W, C] (a [F, H, W] tensor gets C = 1), contiguous, with its kind (0: u8, 1: f32)"""
    if not isinstance(images, torch.Tensor) or images.dtype not in (torch.uint8, torch.float32):
        raise TypeError("images must be a uint8 or float32 tensor on the GPU")
    if images.ndim not in (3, 4) or images.shape[1] < 1 or images.shape[2] < 1 or (images.ndim == 4 and not 1 <= images.shape[3] <= 4):
        raise ValueError(f"images must be [F, H, W, C] with C in 1 .. 4, or [F, H, W], got {tuple(images.shape)}")
    if not images.is_cuda:
        raise TypeError("images must be on the GPU")
    img = images.detach()
    img = img.unsqueeze(-1) if img.ndim == 3 else img
    return img.contiguous(), 0 if images.dtype == torch.uint8 else 1


class _SampleImages(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, img, kind, intr, gate, z_near):
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        N = v.shape[1]
        _, H, W, C = img.shape
        dev = v.device
        handle = _raster_handle(dev.index, 0, _NO_FACES, (H, W))
        value = torch.empty((F, N, C), dtype=torch.float32, device=dev)
        valid = torch.empty((F, N), dtype=torch.uint8, device=dev)
        grad = torch.empty((F, N, C, 2), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        if F * N > 0:
            with torch.cuda.device(dev):
                handle.sample_device(v.data_ptr(), vs.frame_stride, N, F, intr, img.data_ptr(), kind, C, H * W * C,
                                     gate.data_ptr() if gate is not None else None, value.data_ptr(), valid.data_ptr(),
                                     grad.data_ptr() if grad is not None else None, z_near=z_near, stream=_stream())
        valid = valid.bool()
        if grad is not None:
            ctx.intr = intr
            ctx.save_for_backward(v, valid, grad)
        ctx.mark_non_differentiable(valid)
        return value, valid

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_valid):
        v, valid, grad = ctx.saved_tensors
        fx, fy, _, _ = ctx.intr
        if g_value is None:
            return torch.zeros_like(v), None, None, None, None, None
        # per point, f64, rounded once: dL/du = sum_c g_c dI_c/du, then the projection's Jacobian
        g = g_value.double().unsqueeze(-1) * grad.double()
        gu, gv = g[..., 0].sum(dim=-1), g[..., 1].sum(dim=-1)
        p = v.double()
        Z = torch.where(valid, p[..., 2], torch.ones((), dtype=torch.float64, device=v.device))
        gx, gy = fx * gu / Z, fy * gv / Z
        gz = -(gx * p[..., 0] + gy * p[..., 1]) / Z
        zero = torch.zeros((), dtype=torch.float64, device=v.device)
        out = torch.where(valid.unsqueeze(-1), torch.stack((gx, gy, gz), dim=-1), zero)
        return out.to(torch.float32), None, None, None, None, None


def sample_images(images: torch.Tensor, verts: torch.Tensor, intr, gate: torch.Tensor | None = None, z_near: float = 0.1):
    """The images ([F, H, W, C] or [F, H, W]; uint8, used as the raw 0 .. 255, or float32; GPU) read bilinearly where the points
    verts [F, N, 3] f32 project through intr = (fx, fy, cx, cy), pixel centres at integers: (value [F, N, C] f32, valid [F, N]
    bool).  A point is valid iff it is finite, at or behind z_near, its gate ([F, N] bool / uint8, or None) is set and it projects
    into [0, W - 1] x [0, H - 1]; an invalid point's value is 0 (bodyfit_raster_sample_device, include/bodyfit.h).

    Differentiable in verts: dL/dverts = sum_c g_c (dI_c/du du/dverts + dI_c/dv dv/dverts) from the kernel's gradient output, the
    exact derivative of the bilinear patch of the point's cell; formed per point in f64 and rounded once, no scatter.  NOT
    differentiable in the images."""
    img, kind = _check_images(images)
    _check_verts(verts)
    if len(intr) != 4:
        raise ValueError("intr is (fx, fy, cx, cy)")
    if not z_near > 0.0:
        raise ValueError("z_near must be positive")
    if img.shape[0] != verts.shape[0] or img.device != verts.device:
        raise ValueError(f"images has {img.shape[0]} frames on {img.device}, verts has {verts.shape[0]} on {verts.device}")
    if gate is not None:
        if not isinstance(gate, torch.Tensor) or gate.dtype not in (torch.bool, torch.uint8) or gate.device != verts.device:
            raise TypeError("gate must be a bool or uint8 tensor on the GPU of verts")
        if gate.shape != verts.shape[:2]:
            raise ValueError(f"gate must be [F, N] = {tuple(verts.shape[:2])}, got {tuple(gate.shape)}")
        gate = gate.detach().to(torch.uint8).contiguous()
    return _SampleImages.apply(verts, img, kind, tuple(float(a) for a in intr), gate, float(z_near))


def _colour_gate(verts, faces, faces_device, intr, size, min_cos, owner: bool, z_near: float):
    """(gate bool [F, V], cos f64 [F, V]) from verts.detach(): visible in the frame's render at `size`; cos = n . (-x / |x|) >=
    min_cos (None: no test) with n of vertex_normals; owner: the face image at the vertex's nearest pixel holds a face that has
    the vertex as a corner"""
    v = verts.detach()
    F, V = v.shape[0], v.shape[1]
    H, W = size
    fx, fy, cx, cy = intr
    raster, _, face, _ = _render(v, faces, intr, size, z_near, False, False)
    vis = torch.empty((F, V), dtype=torch.uint8, device=v.device)
    with torch.cuda.device(v.device):
        raster.visibility_device(face.data_ptr(), F, None, vis.data_ptr(), _stream())
    gate = vis.bool()
    x = v.double()
    cos = -(vertex_normals(v, faces).double() * x).sum(dim=-1) / x.norm(dim=-1).clamp(min=1e-300)
    if min_cos is not None:
        gate = gate & (cos >= min_cos)
    if owner:
        Z = torch.where(x[..., 2] > 0, x[..., 2], torch.ones((), dtype=torch.float64, device=v.device))
        j, i = torch.floor(fx * x[..., 0] / Z + cx + 0.5), torch.floor(fy * x[..., 1] / Z + cy + 0.5)
        inside = (x[..., 2] > 0) & (i >= 0) & (i < H) & (j >= 0) & (j < W)
        i, j = torch.nan_to_num(i).clamp(0, H - 1).long(), torch.nan_to_num(j).clamp(0, W - 1).long()
        t = face[torch.arange(F, device=v.device)[:, None], i, j].long()
        ids = faces_device[t.clamp(min=0)]                                          # [F, V, 3]
        own = (ids == torch.arange(V, device=v.device)[None, :, None]).any(dim=-1)
        gate = gate & inside & (t >= 0) & own
    return gate, cos


def fuse_vertex_colours(images: torch.Tensor, verts: torch.Tensor, faces, intr, min_cos: float = 0.0, owner: bool = False,
                        z_near: float = 0.1):
    """Per-vertex colours from a sequence: (colour [V, C] f32, weight [V] f64).  (f, v) counts iff the vertex is visible in frame
    f's render at the images' size (visible_vertices), its sample (sample_images) is valid and cos = n . (-x / |x|) >= min_cos, n
    the vertex normal (vertex_normals) and x the vertex: the cosine between the normal and the direction to the camera.  With
    owner=True also: the face image at the vertex's nearest pixel holds a face that has v as a corner, an integer test that keeps a
    vertex behind an occluding edge from taking the occluder's colour.  colour_v = sum_f cos c / sum_f cos in f64, weight_v =
    sum_f cos; a vertex that was never seen gets colour 0 and weight 0.  No gradient."""
    img, _ = _check_images(images)
    _check_verts(verts)
    if len(intr) != 4:
        raise ValueError("intr is (fx, fy, cx, cy)")
    f = _host_faces(faces)
    with torch.no_grad():
        intr = tuple(float(a) for a in intr)
        size = (int(img.shape[1]), int(img.shape[2]))
        faces_device = torch.from_numpy(f).to(verts.device).long().reshape(-1, 3)
        gate, cos = _colour_gate(verts, f, faces_device, intr, size, min_cos, owner, z_near) if f.shape[0] else (
            torch.zeros(verts.shape[:2], dtype=torch.bool, device=verts.device), torch.zeros(verts.shape[:2], dtype=torch.float64, device=verts.device))
        value, valid = sample_images(images, verts.detach(), intr, gate=gate, z_near=z_near)
        w = torch.where(valid, cos, torch.zeros_like(cos))
        weight = w.sum(dim=0)
        num = (w.unsqueeze(-1) * value.double()).sum(dim=0)
        seen = weight > 0
        colour = torch.where(seen.unsqueeze(-1), num / torch.where(seen, weight, torch.ones_like(weight)).unsqueeze(-1),
                             torch.zeros_like(num))
        return colour.to(torch.float32), torch.where(seen, weight, torch.zeros_like(weight))


def _video_term(term, images, intr, trunc, z_near):
    """The constructor checks every photometric term makes; sets term.intr, .size (the video's), .z_near and .trunc and returns the
    video as [F, H, W, C]."""
    img, _ = _check_images(images)
    if len(intr) != 4:
        raise ValueError("intr is (fx, fy, cx, cy)")
    if not z_near > 0.0:
        raise ValueError("z_near must be positive")
    if trunc is not None and not trunc > 0.0:
        raise ValueError("trunc must be positive")
    term.intr = tuple(float(a) for a in intr)
    term.size, term.z_near = (int(img.shape[1]), int(img.shape[2])), float(z_near)
    term.trunc = None if trunc is None else float(trunc)
    return img


def _check_frames(images, verts, named="the images have"):
    if images.device != verts.device or images.shape[0] != verts.shape[0]:
        raise ValueError(f"{named} {images.shape[0]} frames on {images.device}, verts has {verts.shape[0]} on {verts.device}")


def _check_verts_colours(term, verts, colours):
    _check_verts(verts)
    _check_per_vertex(colours, "colours", verts.shape[0], verts.shape[1], verts.device)
    _check_frames(term.images, verts)
    if colours.shape[-1] != term.images.shape[3]:
        raise ValueError(f"colours has {colours.shape[-1]} channels, the images {term.images.shape[3]}")


class PhotometricTerm(torch.nn.Module):
    """The PHOTOMETRIC term: the images of the video against the colours the vertices carry.

    images: [F, H, W, C] or [F, H, W], uint8 (raw 0 .. 255) or float32, on the GPU; intr = (fx, fy, cx, cy).  term(verts, colours),
    verts [F, V, 3] f32 and colours [V, C] or [F, V, C] f32 in the images' units, returns the f64 cost
      sum over the live (f, v) of rho(sum_c (I_c(pi(v)) - colour_c)^2),    rho(s) = min(s, trunc^2) (trunc None: rho(s) = s),
    I(pi(v)) the bilinear sample of frame f at the vertex's projection (sample_images).  The live set is fuse_vertex_colours',
    taken from verts.detach() at every evaluation: visible in the frame's render at the images' size, a valid sample, with min_cos
    (None: no test) n . (-x / |x|) >= min_cos, with owner the integer test on the face image.  It is piecewise constant and
    carries no gradient.  Differentiable in verts (through the image gradient of the sample's cell and the projection) and in
    colours (plain torch).  evaluate(verts, colours) returns the cost with its parts."""

    def __init__(self, images: torch.Tensor, intr, faces, trunc: float | None = None, min_cos: float | None = None,
                 owner: bool = False, z_near: float = 0.1):
        super().__init__()
        img = _video_term(self, images, intr, trunc, z_near)
        self.min_cos = None if min_cos is None else float(min_cos)
        self.owner = bool(owner)
        self.faces = _host_faces(faces).copy()
        self.register_buffer("images", img)
        self.register_buffer("faces_device", torch.from_numpy(self.faces).to(img.device).long().reshape(-1, 3))

    def evaluate(self, verts: torch.Tensor, colours: torch.Tensor) -> dict:
        """term(verts, colours) with what it was built from: cost (f64, with the gradient), gate bool [F, V] (the live set before
        the sample's own validity), valid bool [F, V] (the rows that count), value f32 [F, V, C] (the samples, 0 where not valid),
        sq f64 [F, V] (the squared colour distance of a valid row, else 0) and n_truncated"""
        _check_verts_colours(self, verts, colours)
        with torch.no_grad():
            if self.faces.shape[0]:
                gate, _ = _colour_gate(verts, self.faces, self.faces_device, self.intr, self.size, self.min_cos, self.owner,
                                       self.z_near)
            else:
                gate = torch.zeros(verts.shape[:2], dtype=torch.bool, device=verts.device)
        value, valid = sample_images(self.images, verts, self.intr, gate=gate, z_near=self.z_near)
        diff = value.double() - (colours if colours.ndim == 3 else colours.unsqueeze(0)).double()
        sq = torch.where(valid, diff.square().sum(dim=-1), torch.zeros((), dtype=torch.float64, device=verts.device))
        cost, n_cut = _truncated_cost(sq, self.trunc)
        return {"cost": cost, "gate": gate, "valid": valid, "value": value, "sq": sq, "n_truncated": n_cut}

    def forward(self, verts: torch.Tensor, colours: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts, colours)["cost"]


class _PixelPhotometricTerm(torch.nn.Module):
    """What the photometric terms at the PIXELS share (RenderedPhotometricTerm, TexturedPhotometricTerm): the constructor's checks
    and buffers (images, mask), and the tail of evaluate, antialias -> compare with the video -> mask -> truncate.  A subclass
    keeps its render call and the checks of its own arguments."""

    _VIDEO_NAME, _VIDEO_FRAMES = "the images", "the images have"      # how the subclass's messages speak of the video

    def __init__(self, images, intr, faces, trunc, background, mask, antialias, z_near, cull_backfaces):
        super().__init__()
        img = _video_term(self, images, intr, trunc, z_near)
        bg = _check_background(background, int(img.shape[3]))
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != img.device:
                raise TypeError(f"mask must be a bool or uint8 tensor [F, H, W] on the GPU of {self._VIDEO_NAME}")
            if tuple(mask.shape) != tuple(img.shape[:3]):
                raise ValueError(f"mask must be {tuple(img.shape[:3])}, got {tuple(mask.shape)}")
        self.cull_backfaces = bool(cull_backfaces)
        self.background, self.antialias = bg, bool(antialias)
        self.faces = _host_faces(faces).copy()
        self.register_buffer("images", img)
        self.register_buffer("mask", None if mask is None else (mask != 0).contiguous())

    def _against_video(self, verts, image, face, depth) -> dict:
        """the result of evaluate from a render (image with its gradients, face, depth) of verts"""
        if self.antialias:
            image = antialias(image, verts, self.faces, self.intr, render=(depth, face), z_near=self.z_near,
                              cull_backfaces=self.cull_backfaces)
        sq = (image.double() - self.images.double()).square().sum(dim=-1)
        if self.mask is not None:
            sq = torch.where(self.mask, sq, torch.zeros((), dtype=torch.float64, device=verts.device))
        cost, n_cut = _truncated_cost(sq, self.trunc)
        return {"cost": cost, "image": image, "depth": depth, "face": face, "sq": sq, "n_truncated": n_cut}


class RenderedPhotometricTerm(_PixelPhotometricTerm):
    """The DENSE photometric term, PhotometricTerm's counterpart at the pixels: the rendered vertex colours against the video.

    images: [F, H, W, C] or [F, H, W], uint8 (raw 0 .. 255) or float32, on the GPU; intr = (fx, fy, cx, cy).  term(verts, colours),
    verts [F, V, 3] f32 and colours [V, C] or [F, V, C] f32 in the images' units, returns the f64 cost
      sum over the pixels p of mask of rho(sum_c (R_c(p) - I_c(p))^2),    rho(s) = min(s, trunc^2) (trunc None: rho(s) = s),
    R = antialias(render_attributes(verts, colours, background, interior=True)) (antialias=False: the render itself) and I the
    images; mask: bool or uint8 [F, H, W] on the GPU (None: every pixel).  PhotometricTerm samples the video at the 6,890
    vertices; this term compares every pixel the mesh covers, and the uncovered ones against background.  Differentiable in
    verts through the interpolation inside the faces (render_attributes' interior) and, with antialias, through coverage
    at the silhouettes; in colours through both.  One render per evaluation, shared by the two.  No normal equations are built
    for it.  evaluate(verts, colours) returns the cost with its parts."""

    def __init__(self, images: torch.Tensor, intr, faces, trunc: float | None = None, background=0.0, mask: torch.Tensor | None = None,
                 antialias: bool = True, z_near: float = 0.1, cull_backfaces: bool = False):
        super().__init__(images, intr, faces, trunc, background, mask, antialias, z_near, cull_backfaces)

    def evaluate(self, verts: torch.Tensor, colours: torch.Tensor) -> dict:
        """term(verts, colours) with what it was built from: cost (f64, with the gradient), image f32 [F, H, W, C] (what was
        compared with the video: antialiased or not), the render (depth, face), sq f64 [F, H, W] (the squared colour distance of a
        pixel of the mask, else 0) and n_truncated"""
        _check_verts_colours(self, verts, colours)
        image, face, depth = _RenderAttributes.apply(colours, verts, self.faces, self.intr, self.size, self.background, self.z_near,
                                                     self.cull_backfaces, True)
        return self._against_video(verts, image, face, depth)

    def forward(self, verts: torch.Tensor, colours: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts, colours)["cost"]
