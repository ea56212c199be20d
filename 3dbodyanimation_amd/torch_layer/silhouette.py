"""The outline: the exact distance transform of masks, the silhouette term, silhouette-edge antialiasing and the coverage term.

    dist2, nearest = distance_transform(mask)                            # exact, int32: squared distance and a nearest seed per pixel
    term = SilhouetteTerm(person_mask, intr, faces, trunc=40.0)          # pixels^2: the model inside the mask, the mask covered

What a monocular user has beside the keypoints is a person mask.  distance_transform is bodyfit_raster_distance_device
(k_edt.hip: a separable exact Euclidean feature transform in integers, no atomics).  SilhouetteTerm transforms the mask once;
per evaluation it renders the face image from verts.detach(), transforms that, and pulls the visible vertices that project
outside the mask to their nearest mask pixel, and the nearest rendered surface point to every mask pixel the model leaves
uncovered; the second half's gradient is summed by bodyfit_surface_rows_vjp_device at the fixed (face, weights).

    soft = antialias(image, verts, faces, intr)                          # silhouette edges blended: a gradient to image AND verts
    w = edge_weights(verts, faces, intr, (H, W))                         # [F, H, W, 2]: the blend's weights, no gradient
    term = CoverageTerm(mask, intr, faces)                               # sum (antialias(covered) - mask)^2, pixel^2

Every render is piecewise constant in the vertices.  antialias is bodyfit_raster_edges_device (k_raster_edges.hip: per pair of
neighbouring pixels owned by different faces, a bounded walk to the nearer face's silhouette edge and the fraction of the segment
between the two centres it cuts off) followed by bodyfit_raster_edge_blend_device; its backward is that blend transposed for the
image and, for the vertices, bodyfit_raster_edge_rows_device into bodyfit_surface_rows_vjp_device.  Of antialias only coverage
carries a gradient: the interpolation inside a face does not.  CoverageTerm is the exact-outline counterpart of SilhouetteTerm.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import (_NO_FACES, _TermHandles, _check_intr_size, _check_verts, _grad_like, _host_faces, _point_set,
                      _ragged_rows, _raster_handle, _stream, _surface_handle)
from .depth import _render


def distance_transform(mask: torch.Tensor, invert: bool = False, size_handle=None):
    """The exact Euclidean distance transform WITH the nearest seed of a batch of images: (dist2 int32 [F, H, W], nearest int32
    [F, H, W]).  mask: a GPU tensor [F, H, W]; torch.bool / torch.uint8: a pixel is a seed iff it is != 0; torch.int32: a seed iff
    it is >= 0, so render_depth's face image goes in as it is.  invert swaps seeds and non-seeds.  dist2[f, i, j] is the least
    (i - i')^2 + (j - j')^2 over the seeds (i', j') of frame f, in integers, with no tolerance; nearest[f, i, j] = i' W + j' of a
    seed that attains it (among ties always the same one); a frame without a seed holds INT32_MAX and -1.  A view whose frames
    are farther apart than H W elements is used in place.  size_handle: an api.Raster of this device and image size (None: a kept
    handle without a topology).  No gradient; runs on torch.cuda.current_stream() without a host synchronisation
    (bodyfit_raster_distance_device, include/bodyfit.h; k_edt.hip)."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8, torch.int32) or not mask.is_cuda:
        raise TypeError("mask must be a bool, uint8 or int32 tensor on the GPU")
    if mask.ndim != 3 or mask.shape[1] < 1 or mask.shape[2] < 1:
        raise ValueError(f"mask must be [F, H, W] with H, W >= 1, got {tuple(mask.shape)}")
    m = mask.detach()
    F, H, W = m.shape
    if not (m.stride(2) == 1 and m.stride(1) == W and (F <= 1 or m.stride(0) >= H * W)):
        m = m.contiguous()
    stride = m.stride(0) if F > 1 else H * W
    if size_handle is None:
        size_handle = _raster_handle(m.device.index, 0, _NO_FACES, (H, W))
    elif not isinstance(size_handle, api.Raster):
        raise TypeError("size_handle must be an api.Raster")
    elif (size_handle.device, size_handle.height, size_handle.width) != (m.device.index, H, W):
        raise ValueError(f"size_handle is for cuda:{size_handle.device} and {size_handle.height} x {size_handle.width}, the mask is "
                         f"on cuda:{m.device.index} and {H} x {W}")
    dist2 = torch.empty((F, H, W), dtype=torch.int32, device=m.device)
    nearest = torch.empty((F, H, W), dtype=torch.int32, device=m.device)
    if F > 0:
        with torch.cuda.device(m.device):
            size_handle.distance_device(m.data_ptr(), 1 if m.dtype == torch.int32 else 0, stride, F, invert, dist2.data_ptr(),
                                        nearest.data_ptr(), _stream())
    return dist2, nearest


class _SilhouetteRows(torch.autograd.Function):
    """value (a constant of the evaluation) with the data -> model rows' gradient: gverts = upstream x sum_i beta_ia m_i at corner
    a of face index_i, by the rows VJP"""

    @staticmethod
    def forward(ctx, verts, value, index, beta, direction, offset, surface):
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        ctx.rows = (vs, F, surface)
        ctx.save_for_backward(v, index, beta, direction, offset)
        return value.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        v, index, beta, direction, offset = ctx.saved_tensors
        vs, F, surface = ctx.rows
        gv = _grad_like(v, vs)
        N = index.shape[0]
        if g is None or N == 0 or v.shape[1] == 0:
            gv.zero_()
        else:
            coef = g.to(torch.float32).expand(N).contiguous()
            rows = api.PointSet.ragged(index.data_ptr(), offset.data_ptr())   # (the frame structure; its xyz is never read)
            with torch.cuda.device(v.device):
                surface.rows_vjp_device(rows, F, N, index.data_ptr(), beta.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                        gv.data_ptr(), vs.frame_stride, _stream())
        return gv, None, None, None, None, None, None


class SilhouetteTerm(_TermHandles, torch.nn.Module):
    """The OUTLINE term of a person mask S beside the keypoints: the model stays inside S, and S is covered by the model.

    mask: [F, H, W] bool / uint8 on the GPU (a pixel of S iff != 0); intr = (fx, fy, cx, cy); pixel (i, j) is the sample (u, v) =
    (j, i), render_depth's convention.  The constructor transforms S once (distance_transform) and keeps nearest_S.
    term(verts), verts [F, V, 3] f32, returns the f64 cost in pixel^2, rho(s) = min(s, trunc^2) (trunc in pixels; None: rho(s) =
    s).  Per evaluation, from verts.detach(): ONE render at the mask's size gives (depth z^, face, lambda); M = {face >= 0}; ONE
    distance_transform(face) gives (d2_M, nearest_M); the visibility kernel on the same face image gives the visible vertices.

      model -> data (model_to_data): for every VISIBLE vertex with projection p = (u, v) = (fx X / Z + cx, fy Y / Z + cy), let
        (i, j) = (floor(v + 1/2), floor(u + 1/2)).  A vertex whose pixel lies outside the image, or inside S, costs 0; else with
        s = nearest_S[f, i, j] = (i_s, j_s) it costs rho(|e|^2), e = (u - j_s, v - i_s).  A frame whose S is empty costs 0.  The
        gradient is plain torch through the projection of verts[visible] at the fixed s (a boolean-mask gather: its backward is
        deterministic).
      data -> model (data_to_model): for every pixel q = (i, j) of S \\ M in a frame whose M is not empty, t = nearest_M[f, i, j] =
        (i_t, j_t), k = face[f, t], lambda = bary[f, t], z^ = depth[f, t], Z_a the depths of face k's corners.  The matched surface
        point is x = sum_a beta_a v_a with beta_a = lambda_a z^ / Z_a: the perspective-correct object-space weights, >= 0 and
        summing to 1 by the render's definition of z^, and well conditioned on slivers (which the ray-plane beta of the depth
        rows are not).  The row's residual e = pi(x) - (j, i) is (j_t - j, i_t - i) at the current vertices, so its value is
        rho(d2_M[q]), an exact integer from the transform: the half's value is the int64 sum of the rows with d2_M < trunc^2
        plus trunc^2 per truncated row.  Its gradient at the fixed (k, beta): d/dv_a = beta_a m,
          m = 2 rho' (fx e_u / z^, fy e_v / z^, -(e_u (j_t - cx) + e_v (i_t - cy)) / z^),   rho' = 0 on a truncated row,
        summed into the vertices by bodyfit_surface_rows_vjp_device (index k, bary beta, direction m, coef the upstream gradient):
        scatter-free f64 sums, bit-identical from run to run.

    The render and the two transforms carry NO gradient: the correspondences are piecewise constant.  A frame whose mesh is
    behind z_near has no M and no visible vertex and contributes exactly 0 with a zero gradient.  The host synchronises at the
    render's 8-byte read-back and at the nonzero calls that size the visible vertices and the rows.  evaluate(verts) returns the
    cost with what it was built from."""

    def __init__(self, mask: torch.Tensor, intr, faces, trunc: float | None = None, z_near: float = 0.1,
                 model_to_data: bool = True, data_to_model: bool = True):
        super().__init__()
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or not mask.is_cuda:
            raise TypeError("mask must be a bool or uint8 tensor [F, H, W] on the GPU")
        if mask.ndim != 3 or mask.shape[1] < 1 or mask.shape[2] < 1:
            raise ValueError(f"mask must be [F, H, W] with H, W >= 1, got {tuple(mask.shape)}")
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        self.intr = tuple(float(a) for a in intr)
        self.size, self.z_near = (int(mask.shape[1]), int(mask.shape[2])), float(z_near)
        self.trunc = None if trunc is None else float(trunc)
        self.model_to_data, self.data_to_model = bool(model_to_data), bool(data_to_model)
        self.faces = _host_faces(faces).copy()
        inside = (mask.detach() != 0).contiguous()
        self.register_buffer("mask", inside)
        self.register_buffer("nearest_S", distance_transform(inside)[1])
        self.register_buffer("faces_device", torch.from_numpy(self.faces).to(mask.device).long())

    def _rho(self, s: torch.Tensor) -> torch.Tensor:
        # (not _truncated_cost: rho per row under a mask, summed by the caller; the other half counts in integers)
        return s if self.trunc is None else torch.clamp(s, max=self.trunc * self.trunc)

    def evaluate(self, verts: torch.Tensor) -> dict:
        """term(verts) with what it was built from: cost, cost_model_to_data, cost_data_to_model (f64, the first with the
        gradient), the render (depth, face, bary), visible bool [F, V], (dist2_model, nearest_model), the rows (row_frame, row_i,
        row_j int64 [N]; row_index int32 [N], row_beta f32 [N, 3], row_direction f32 [N, 3]), and the data -> model value's
        integer parts sum_dist2 (int64, over the rows that are not truncated) and n_truncated"""
        raster, depth, face, bary = _render(verts, self.faces, self.intr, self.size, self.z_near, False, True)
        F, V = verts.shape[0], verts.shape[1]
        H, W = self.size
        dev = verts.device
        if self.mask.device != dev or self.mask.shape[0] != F:
            raise ValueError(f"the mask has {self.mask.shape[0]} frames on {self.mask.device}, verts has {F} on {dev}")
        fx, fy, cx, cy = self.intr
        out = {"depth": depth, "face": face, "bary": bary}
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        cost_md, cost_dm = zero, zero
        if self.model_to_data:
            vis = torch.empty((F, V), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                raster.visibility_device(face.data_ptr(), F, None, vis.data_ptr(), _stream())
            vis = vis.bool()
            out["visible"] = vis
            frame = torch.nonzero(vis, as_tuple=True)[0]                # (the order of the boolean-mask gather below)
            p = verts[vis].double()                                     # [n, 3], with the gradient
            u = fx * p[:, 0] / p[:, 2] + cx
            v = fy * p[:, 1] / p[:, 2] + cy
            with torch.no_grad():
                i, j = torch.floor(v + 0.5), torch.floor(u + 0.5)
                inside = (i >= 0) & (i < H) & (j >= 0) & (j < W)
                i, j = i.clamp(0, H - 1).long(), j.clamp(0, W - 1).long()
                s = self.nearest_S[frame, i, j].long()
                pull = inside & ~self.mask[frame, i, j] & (s >= 0)
                i_s = torch.div(s.clamp(min=0), W, rounding_mode="floor")
                j_s = s.clamp(min=0) - i_s * W
            e2 = (u - j_s.double()).square() + (v - i_s.double()).square()
            cost_md = torch.where(pull, self._rho(e2), zero).sum()
        if self.data_to_model:
            with torch.no_grad(), torch.cuda.device(dev):
                d2_m = torch.empty((F, H, W), dtype=torch.int32, device=dev)
                near_m = torch.empty((F, H, W), dtype=torch.int32, device=dev)
                if F > 0:
                    raster.distance_device(face.data_ptr(), 1, H * W, F, False, d2_m.data_ptr(), near_m.data_ptr(), _stream())
                rows = self.mask & (face < 0) & (near_m >= 0)
                f, i, j = torch.nonzero(rows, as_tuple=True)            # frame-major, then row-major: a ragged set of rows
                offset = torch.zeros(F + 1, dtype=torch.int32, device=dev)
                offset[1:] = rows.reshape(F, -1).sum(dim=1).cumsum(0).to(torch.int32)
                t = near_m[f, i, j].long()
                i_t = torch.div(t, W, rounding_mode="floor")
                j_t = t - i_t * W
                k = face[f, i_t, j_t].contiguous()
                z = depth[f, i_t, j_t].double()
                ids = self.faces_device[k.long()] if self.faces_device.shape[0] > 0 else torch.zeros((0, 3), dtype=torch.long,
                                                                                                    device=dev)
                Z = verts.detach()[f[:, None], ids, 2].double()
                beta = bary[f, i_t, j_t].double() * z[:, None] / Z
                d2 = d2_m[f, i, j].long()
                keep = d2.double() < self.trunc * self.trunc if self.trunc is not None else torch.ones_like(d2, dtype=torch.bool)
                sum_d2 = torch.where(keep, d2, torch.zeros_like(d2)).sum()
                n_cut = (~keep).sum()
                value = sum_d2.double()
                if self.trunc is not None:
                    value = value + self.trunc * self.trunc * n_cut.double()
                e_u, e_v = (j_t - j).double(), (i_t - i).double()
                w = 2.0 * keep.double() / z
                m = torch.stack((fx * e_u * w, fy * e_v * w, -(e_u * (j_t.double() - cx) + e_v * (i_t.double() - cy)) * w), dim=1)
                beta32, m32 = beta.to(torch.float32).contiguous(), m.to(torch.float32).contiguous()
            cost_dm = _SilhouetteRows.apply(verts, value, k, beta32, m32, offset, self._handle_for(verts))
            out.update(dist2_model=d2_m, nearest_model=near_m, row_frame=f, row_i=i, row_j=j, row_index=k, row_beta=beta32,
                       row_direction=m32, row_offset=offset, sum_dist2=sum_d2, n_truncated=n_cut)
        out.update(cost=cost_md + cost_dm, cost_model_to_data=cost_md, cost_data_to_model=cost_dm)
        return out

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts)["cost"]


def _render_or(render, verts, faces, intr, size, z_near, cull_backfaces):
    """(raster handle, depth [F, H, W] f32, face [F, H, W] int32) of verts: `render` (what render_depth returned, or (depth,
    face)) checked and used as it is, or a fresh render"""
    H, W = int(size[0]), int(size[1])
    if render is None:
        raster, depth, face, _ = _render(verts, faces, intr, (H, W), z_near, cull_backfaces, False)
        return raster, depth, face
    if len(render) < 2:
        raise ValueError("render is (depth, face) or (depth, face, bary), as render_depth returns them")
    depth, face = render[0], render[1]
    F = verts.shape[0]
    for t, dt, name in ((depth, torch.float32, "depth"), (face, torch.int32, "face")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != verts.device or tuple(t.shape) != (F, H, W):
            raise ValueError(f"render's {name} must be a {dt} tensor [{F}, {H}, {W}] on the GPU of verts")
    raster = _raster_handle(verts.device.index, verts.shape[1], faces, (H, W))
    return raster, depth.detach().contiguous(), face.contiguous()


def _edge_weights(raster, verts, intr, depth, face, z_near, cull_backfaces):
    v, vs, F, _ = _point_set("verts", verts.detach(), None)
    H, W = face.shape[1], face.shape[2]
    w = torch.empty((F, H, W, 2), dtype=torch.float32, device=v.device)
    if F > 0:
        with torch.cuda.device(v.device):
            raster.edges_device(v.data_ptr(), vs.frame_stride, F, [float(a) for a in intr], face.data_ptr(), depth.data_ptr(),
                                w.data_ptr(), z_near=float(z_near), cull_backfaces=cull_backfaces, stream=_stream())
    return w


def edge_weights(verts: torch.Tensor, faces, intr, size, render=None, z_near: float = 0.1, cull_backfaces: bool = False):
    """The silhouette-edge antialiasing weights of the posed meshes verts [F, V, 3] f32 in an image of size = (height, width):
    f32 [F, H, W, 2], per pixel p its pair with the right (axis 0) and the lower (axis 1) neighbour q.  w > 0: q receives
    w (img[p] - img[q]); w < 0: p receives |w| (img[q] - img[p]); 0: no blend; |w| <= 1/2.  render: what render_depth(verts, faces,
    intr, size, z_near, cull_backfaces) returned, reused; None: rendered here.  The definition (pairs of neighbouring pixels owned
    by different faces, the bounded walk from the nearer pixel's face to the silhouette edge that crosses the segment between the
    two centres, the blend by the covered fraction), its tie rules and its error bounds: bodyfit_raster_edges_device,
    include/bodyfit.h.  NOT differentiable (antialias is).  Runs on torch.cuda.current_stream()."""
    _check_verts(verts)
    _check_intr_size(intr, size)
    raster, depth, face = _render_or(render, verts, faces, intr, size, z_near, cull_backfaces)
    return _edge_weights(raster, verts, intr, depth, face, float(z_near), bool(cull_backfaces))


def _edge_blend(raster, w, image, transpose: bool):
    F, H, W, C = image.shape
    out = torch.empty((F, H, W, C), dtype=torch.float32, device=image.device)
    if F > 0:
        with torch.cuda.device(image.device):
            raster.edge_blend_device(w.data_ptr(), image.data_ptr(), C, F, transpose, out.data_ptr(), _stream())
    return out


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, verts, faces, intr, render, z_near, cull_backfaces):
        F, H, W, C = image.shape
        raster, depth, face = _render_or(render, verts, faces, intr, (H, W), z_near, cull_backfaces)
        w = _edge_weights(raster, verts, intr, depth, face, z_near, cull_backfaces)
        img = image.detach().contiguous()
        out = _edge_blend(raster, w, img, False)
        ctx.args = (raster, faces, tuple(float(a) for a in intr), z_near, cull_backfaces)
        if ctx.needs_input_grad[1]:
            v, _, _, _ = _point_set("verts", verts.detach(), None)
            ctx.save_for_backward(w, img, v, depth, face)
        else:
            ctx.save_for_backward(w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        w = ctx.saved_tensors[0]
        raster, faces, intr, z_near, cull = ctx.args
        g = g.to(torch.float32).contiguous()
        g_image = _edge_blend(raster, w, g, True) if ctx.needs_input_grad[0] else None
        gv = None
        if ctx.needs_input_grad[1]:
            _, img, v, depth, face = ctx.saved_tensors
            v, vs, F, _ = _point_set("verts", v, None)
            gv = _grad_like(v, vs)
            dev = v.device
            C = g.shape[-1]
            # the blended pairs, frame after frame and ascending inside a frame: code = 2 pixel + axis
            _, pair, offset, N = _ragged_rows(w.reshape(F, -1))
            if N == 0 or v.shape[1] == 0:
                gv.zero_()
            else:
                index = torch.empty(2 * N, dtype=torch.int32, device=dev)
                bary = torch.empty((2 * N, 3), dtype=torch.float32, device=dev)
                coef = torch.empty(2 * N, dtype=torch.float32, device=dev)
                direction = torch.empty((2 * N, 3), dtype=torch.float32, device=dev)
                offset2 = (2 * offset).contiguous()
                surface = _surface_handle(dev.index, v.shape[1], faces)
                rows = api.PointSet.ragged(index.data_ptr(), offset2.data_ptr())     # (the frame structure; its xyz is never read)
                with torch.cuda.device(dev):
                    raster.edge_rows_device(v.data_ptr(), vs.frame_stride, F, intr, face.data_ptr(), depth.data_ptr(), img.data_ptr(),
                                            g.data_ptr(), C, pair.data_ptr(), offset.data_ptr(), N, index.data_ptr(), bary.data_ptr(),
                                            coef.data_ptr(), direction.data_ptr(), z_near=z_near, cull_backfaces=cull, stream=_stream())
                    surface.rows_vjp_device(rows, F, 2 * N, index.data_ptr(), bary.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                            gv.data_ptr(), vs.frame_stride, _stream())
        return g_image, gv, None, None, None, None, None


def antialias(image: torch.Tensor, verts: torch.Tensor, faces, intr, render=None, z_near: float = 0.1,
              cull_backfaces: bool = False) -> torch.Tensor:
    """image ([F, H, W, C] or [F, H, W] f32 on the GPU, C in 1 .. 4: a render_attributes image, a coverage mask as 0 / 1) with the
    silhouette edges of the posed meshes verts [F, V, 3] f32 antialiased (Laine et al. 2020): an image of the same shape in which a
    pixel next to an occlusion boundary is blended with its neighbour across the boundary by the fraction of the segment between
    the two centres that the nearer face's silhouette edge cuts off.  render: what render_depth(verts, faces, intr, (H, W), z_near,
    cull_backfaces) returned, reused; None: rendered here (one 8-byte read-back).

    Differentiable in image (the blend's exact adjoint, bodyfit_raster_edge_blend_device with transpose) and in verts THROUGH
    COVERAGE at the fixed face image: the blend weight is a smooth function of the two vertices of the silhouette edge, and
    loss(antialias(render(verts))).backward() reaches verts.  Gradients of the interpolation inside a face (how image itself changes
    as its face's corners move) are NOT part of it: pass an image that already carries those if it has them.  The backward: nonzero
    of the weights lists the blended pairs in ascending order (one host synchronisation), bodyfit_raster_edge_rows_device writes two
    rows per pair, bodyfit_surface_rows_vjp_device sums them into the vertices: no float atomics, bit-identical from run to run.
    The definition, its tie rules and error bounds: include/bodyfit.h.  Runs on torch.cuda.current_stream()."""
    _check_verts(verts)
    if len(intr) != 4:
        raise ValueError("intr is (fx, fy, cx, cy)")
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or not image.is_cuda:
        raise TypeError("image must be a float32 tensor on the GPU")
    if image.device != verts.device:
        raise ValueError("image and verts must be on the same GPU")
    flat = image.ndim == 3
    img = image.unsqueeze(-1) if flat else image
    if img.ndim != 4 or img.shape[0] != verts.shape[0] or not 1 <= img.shape[3] <= 4 or img.shape[1] < 1 or img.shape[2] < 1:
        raise ValueError(f"image must be [F, H, W] or [F, H, W, C] with F = {verts.shape[0]} and C in 1 .. 4, got {tuple(image.shape)}")
    if not z_near > 0.0:
        raise ValueError("z_near must be positive")
    out = _Antialias.apply(img, verts, faces, intr, render, float(z_near), bool(cull_backfaces))
    return out.squeeze(-1) if flat else out


class CoverageTerm(torch.nn.Module):
    """The EXACT-outline counterpart of SilhouetteTerm: sum over the pixels of (antialias(covered) - mask)^2, in pixel^2.

    mask: [F, H, W] bool / uint8 / float32 on the GPU (a person mask, as 0 / 1; a float mask may hold fractions); intr = (fx, fy, cx,
    cy).  term(verts), verts [F, V, 3] f32, renders the mesh at the mask's size, takes its coverage {face >= 0} as a 0 / 1 f32 image,
    antialiases it (antialias, with that render) and returns the f64 sum of squared differences to the mask.  Its gradient reaches
    verts through the antialiased outline only, so it is non-zero only where the model's outline is within a pixel of a
    disagreement with the mask: SilhouetteTerm (distance transforms: a pull from any distance) brings the fit there, this term
    finishes it.  No normal equations are built for it."""

    def __init__(self, mask: torch.Tensor, intr, faces, z_near: float = 0.1, cull_backfaces: bool = False):
        super().__init__()
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8, torch.float32) or not mask.is_cuda:
            raise TypeError("mask must be a bool, uint8 or float32 tensor [F, H, W] on the GPU")
        if mask.ndim != 3 or mask.shape[1] < 1 or mask.shape[2] < 1:
            raise ValueError(f"mask must be [F, H, W] with H, W >= 1, got {tuple(mask.shape)}")
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        self.intr = tuple(float(a) for a in intr)
        self.size, self.z_near, self.cull_backfaces = (int(mask.shape[1]), int(mask.shape[2])), float(z_near), bool(cull_backfaces)
        self.faces = _host_faces(faces).copy()
        m = mask.detach()
        self.register_buffer("mask", (m if m.dtype == torch.float32 else (m != 0).to(torch.float32)).contiguous())

    def evaluate(self, verts: torch.Tensor) -> dict:
        """term(verts) with what it was built from: cost (f64, with the gradient), the render (depth, face) and the antialiased
        coverage [F, H, W] f32"""
        _check_verts(verts)
        if self.mask.device != verts.device or self.mask.shape[0] != verts.shape[0]:
            raise ValueError(f"the mask has {self.mask.shape[0]} frames on {self.mask.device}, verts has {verts.shape[0]} on {verts.device}")
        _, depth, face, _ = _render(verts, self.faces, self.intr, self.size, self.z_near, self.cull_backfaces, False)
        covered = (face >= 0).to(torch.float32)
        soft = antialias(covered, verts, self.faces, self.intr, render=(depth, face), z_near=self.z_near,
                         cull_backfaces=self.cull_backfaces)
        cost = (soft.double() - self.mask.double()).square().sum()
        return {"cost": cost, "depth": depth, "face": face, "coverage": soft}

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts)["cost"]
