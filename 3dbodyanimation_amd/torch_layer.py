"""PyTorch autograd layers over the library's SMPL forward and fitting objective, with their reverse-mode gradients.

    layer = SMPLLayer(api.Model(model))
    verts, joints = layer(x, beta)          # x [F, 76] f64 cuda, beta [nS] (or [F, nS]) f64 cuda
    loss(verts, joints).backward()

forward is bodyfit_forward_device (the two-launch sweep: verts [F, V, 3] f32, joints [F, 24, 3] f64), backward is
bodyfit_forward_vjp_device (HIP kernels, k_forward_vjp.hip); forward-mode AD (torch.autograd.forward_ad) and layer.jvp /
layer.jacobian are bodyfit_forward_jvp_device (k_forward_jvp.hip: K tangents per frame at once, the dense Jacobian with the unit
tangents).  Both run on torch.cuda.current_stream() without a host
synchronisation.  The layer keeps one keypoint-free problem (want_mesh) per frame count.  Calls that share a frame count share
that problem's device buffers, so interleaving them on several streams at once needs the caller's own ordering (events).

    obj = FitObjective(problem)             # an api.Problem: keypoints, camera, priors, temporal terms
    r = obj(x, beta)                        # [total_rows] f64 residual vector (bodyfit_residuals_device)
    (obj.cost(r) + my_term).backward()      # backward: bodyfit_residual_vjp_device (k_residual_vjp.hip)

obj.cost(r) is the Ceres cost of the problem (HuberLoss on the keypoint blocks, squares elsewhere), written in torch.

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

    dist2, nearest = distance_transform(mask)                            # exact, int32: squared distance and a nearest seed per pixel
    term = SilhouetteTerm(person_mask, intr, faces, trunc=40.0)          # pixels^2: the model inside the mask, the mask covered

What a monocular user has beside the keypoints is a person mask.  distance_transform is bodyfit_raster_distance_device
(k_edt.hip: a separable exact Euclidean feature transform in integers, no atomics).  SilhouetteTerm transforms the mask once;
per evaluation it renders the face image from verts.detach(), transforms that, and pulls the visible vertices that project
outside the mask to their nearest mask pixel, and the nearest rendered surface point to every mask pixel the model leaves
uncovered; the second half's gradient is summed by bodyfit_surface_rows_vjp_device at the fixed (face, weights).

    w = winding_number(points, verts, faces, offset)                     # 0 outside, 1 inside a closed mesh (no gradient)
    sdf, index, bary = signed_distance(points, verts, faces, offset)     # negative inside; closest_surface's gradient
    term = SelfPenetrationTerm(faces, trunc=0.05)                        # m^2: the vertices inside another part of the body

None of the data terms knows that the body is a solid.  winding_number is bodyfit_surface_winding_device (k_winding.hip: all
pairs of query and triangle, the half solid angles summed exactly as integers); vertex_winding asks it about the mesh's own
vertices with their own faces left out, where w > 1 means "inside another part of the body" without a threshold.
SelfPenetrationTerm matches those vertices, through the oriented search with minus their normal (vertex_normals,
bodyfit_surface_vertex_normals_device), to the sheet they have passed through, and pulls them back out.

    verts, joints = layer(x, beta, offsets=d)                            # SMPL+D: d [V, 3] or [F, V, 3] f32, differentiable
    reg = OffsetRegulariser(faces, w_smooth=1e3, w_norm=1.0)             # w_smooth sum |L d|^2 + w_norm sum |d|^2
    (term(verts) + reg(d)).backward()

Every data term above measures a naked body against a clothed person.  offsets displaces the blended rest vertex before
skinning (bodyfit_forward_offsets*_device, k_offsets.hip); the joints, and with them FitObjective's keypoint landmarks, stay those
of the undisplaced shape.  layer.jvp / layer.jacobian / forward_ad and every normal_equations take offsets= as a constant, so a
Gauss-Newton step on pose and shape alternates with gradient steps on the offsets.  mesh_laplacian is
bodyfit_surface_laplacian_device, a deterministic gather whose backward is the transposed gather.

    image, face = render_attributes(verts, faces, intr, (H, W), colours)   # the coloured avatar; a gradient to colours only
    value, valid = sample_images(video, verts, intr)                     # the frames read at the vertices, differentiable in verts
    colours, weight = fuse_vertex_colours(video, verts, faces, intr, owner=True)   # [V, C]: the person's colours on the mesh
    term = PhotometricTerm(video, intr, faces, trunc=30.0, owner=True)   # sum rho(|I(pi(v)) - colour_v|^2) over the visible vertices

The dense signal between the keypoints and the outline is the image itself.  render_attributes is render_depth followed by
bodyfit_raster_shade_device (k_raster.hip: per-vertex attributes interpolated with the perspective-correct weights), its
backward bodyfit_surface_rows_vjp_device over the pixels.  sample_images is bodyfit_raster_sample_device (one bilinear read per
vertex and frame, u8 or f32 images, with the image gradient of the cell).  fuse_vertex_colours averages the samples of the frames
that see a vertex, weighted by the cosine to the camera; PhotometricTerm holds such colours against the frames and is
differentiable in the vertices and in the colours.

    soft = antialias(image, verts, faces, intr)                          # silhouette edges blended: a gradient to image AND verts
    w = edge_weights(verts, faces, intr, (H, W))                         # [F, H, W, 2]: the blend's weights, no gradient
    term = CoverageTerm(mask, intr, faces)                               # sum (antialias(covered) - mask)^2, pixel^2

Every render above is piecewise constant in the vertices.  antialias is bodyfit_raster_edges_device (k_raster.hip: per pair of
neighbouring pixels owned by different faces, a bounded walk to the nearer face's silhouette edge and the fraction of the segment
between the two centres it cuts off) followed by bodyfit_raster_edge_blend_device; its backward is that blend transposed for the
image and, for the vertices, bodyfit_raster_edge_rows_device into bodyfit_surface_rows_vjp_device.  Of antialias only coverage
carries a gradient: the interpolation inside a face does not.  CoverageTerm is the exact-outline counterpart of SilhouetteTerm.

    image, face = render_attributes(verts, faces, intr, (H, W), colours, interior=True)   # ALSO differentiable in verts, inside the faces
    term = RenderedPhotometricTerm(video, intr, faces, trunc=30.0)       # sum rho(|antialias(render) - I|^2) over the pixels

interior=True adds the middle of rasterize -> interpolate -> antialias: the same image, and in the backward one row per shaded
pixel from bodyfit_raster_interp_rows_device (k_raster.hip: the object-space barycentrics of the pixel's ray in its face and the
one direction that carries dL/dimage to the three corners) into bodyfit_surface_rows_vjp_device.  RenderedPhotometricTerm is
PhotometricTerm at the pixels instead of the vertices: interior and coverage gradients of one render.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import api


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _SMPLForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, beta, prob, n_verts, n_joints):
        F = x.shape[0]
        verts = torch.empty((F, n_verts, 3), dtype=torch.float32, device=x.device)
        joints = torch.empty((F, n_joints, 3), dtype=torch.float64, device=x.device)
        prob.forward_device(x.data_ptr(), beta.data_ptr(), joints.data_ptr(), verts.data_ptr(), 3 * n_verts, _stream())
        ctx.prob = prob
        ctx.n_verts = n_verts
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, beta)
        ctx.save_for_forward(x, beta)
        return verts, joints

    @staticmethod
    def jvp(ctx, x_t, beta_t, *_):
        # forward-mode AD (torch.autograd.forward_ad): one tangent, bodyfit_forward_jvp_device; a missing tangent is zero
        x, beta = ctx.saved_tensors
        F = x.shape[0]
        n_joints = (x.shape[1] - 7) // 3 + 1
        verts_t = torch.empty((F, ctx.n_verts, 3), dtype=torch.float32, device=x.device)
        joints_t = torch.empty((F, n_joints, 3), dtype=torch.float64, device=x.device)
        if x_t is not None:
            x_t = x_t.to(torch.float64).contiguous()
        if beta_t is not None:
            beta_t = beta_t.to(torch.float64).contiguous()
        ctx.prob.forward_jvp_device(x.data_ptr(), beta.data_ptr(), 1, x_t.data_ptr() if x_t is not None else None,
                                    beta_t.data_ptr() if beta_t is not None else None, joints_t.data_ptr(),
                                    verts_t.data_ptr(), 3 * ctx.n_verts, _stream())
        return verts_t, joints_t

    @staticmethod
    @once_differentiable
    def backward(ctx, g_verts, g_joints):
        x, beta = ctx.saved_tensors
        want_x, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_verts is not None:
            g_verts = g_verts.to(torch.float32).contiguous()
        if g_joints is not None:
            g_joints = g_joints.to(torch.float64).contiguous()
        gx = torch.empty_like(x)
        gb = torch.empty_like(beta)
        if g_verts is None and g_joints is None:
            gx.zero_(); gb.zero_()
        else:
            ctx.prob.forward_vjp_device(x.data_ptr(), beta.data_ptr(),
                                        g_verts.data_ptr() if g_verts is not None else None,
                                        g_joints.data_ptr() if g_joints is not None else None,
                                        gx.data_ptr(), gb.data_ptr(), 3 * ctx.n_verts, _stream())
        return (gx if want_x else None), (gb if want_b else None), None, None, None


class _SMPLForwardOffsets(torch.autograd.Function):
    """_SMPLForward with per-vertex offsets [V, 3] or [F, V, 3] f32 as a third differentiable input (bodyfit_forward_offsets*)."""

    @staticmethod
    def forward(ctx, x, beta, offsets, prob, n_verts, n_joints):
        F = x.shape[0]
        verts = torch.empty((F, n_verts, 3), dtype=torch.float32, device=x.device)
        joints = torch.empty((F, n_joints, 3), dtype=torch.float64, device=x.device)
        stride = 3 * n_verts if offsets.ndim == 3 else 0
        prob.forward_device(x.data_ptr(), beta.data_ptr(), joints.data_ptr(), verts.data_ptr(), 3 * n_verts, _stream(),
                            d_offsets_ptr=offsets.data_ptr(), offsets_frame_stride=stride)
        ctx.prob = prob
        ctx.n_verts = n_verts
        ctx.stride = stride
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, beta, offsets)
        ctx.save_for_forward(x, beta, offsets)
        return verts, joints

    @staticmethod
    def jvp(ctx, x_t, beta_t, offsets_t, *_):
        if offsets_t is not None:
            raise NotImplementedError("the offsets carry no tangent: forward-mode AD treats them as constants")
        x, beta, offsets = ctx.saved_tensors
        F = x.shape[0]
        n_joints = (x.shape[1] - 7) // 3 + 1
        verts_t = torch.empty((F, ctx.n_verts, 3), dtype=torch.float32, device=x.device)
        joints_t = torch.empty((F, n_joints, 3), dtype=torch.float64, device=x.device)
        if x_t is not None:
            x_t = x_t.to(torch.float64).contiguous()
        if beta_t is not None:
            beta_t = beta_t.to(torch.float64).contiguous()
        ctx.prob.forward_jvp_device(x.data_ptr(), beta.data_ptr(), 1, x_t.data_ptr() if x_t is not None else None,
                                    beta_t.data_ptr() if beta_t is not None else None, joints_t.data_ptr(),
                                    verts_t.data_ptr(), 3 * ctx.n_verts, _stream(), d_offsets_ptr=offsets.data_ptr(),
                                    offsets_frame_stride=ctx.stride)
        return verts_t, joints_t

    @staticmethod
    @once_differentiable
    def backward(ctx, g_verts, g_joints):
        x, beta, offsets = ctx.saved_tensors
        want_x, want_b, want_o = ctx.needs_input_grad[:3]
        if g_verts is not None:
            g_verts = g_verts.to(torch.float32).contiguous()
        if g_joints is not None:
            g_joints = g_joints.to(torch.float64).contiguous()
        gx = torch.empty_like(x)
        gb = torch.empty_like(beta)
        # (without a gradient on the vertices the offsets get zeros: the joints do not depend on them)
        go = (torch.empty_like(offsets) if g_verts is not None else torch.zeros_like(offsets)) if want_o else None
        if g_verts is None and g_joints is None:
            gx.zero_(); gb.zero_()
        else:
            ctx.prob.forward_vjp_device(x.data_ptr(), beta.data_ptr(),
                                        g_verts.data_ptr() if g_verts is not None else None,
                                        g_joints.data_ptr() if g_joints is not None else None,
                                        gx.data_ptr(), gb.data_ptr(), 3 * ctx.n_verts, _stream(),
                                        d_offsets_ptr=offsets.data_ptr(), offsets_frame_stride=ctx.stride,
                                        d_grad_offsets_ptr=go.data_ptr() if (go is not None and g_verts is not None) else None)
        return (gx if want_x else None), (gb if want_b else None), go, None, None, None


class SMPLLayer(torch.nn.Module):
    """SMPL forward with gradients w.r.t. the frame parameters [s, rootAA, rootT, jointAA[1..23]] and beta.

    model: an api.Model.  R0: [3, 3] for every frame (default: identity) or [F, 3, 3] (then only F frames are accepted).
    beta_per_frame: beta is [F, nS] instead of [nS].  use_shape / pose_blend: as for api.Problem.
    """

    def __init__(self, model, R0=None, beta_per_frame: bool = False, use_shape: bool = True, pose_blend: bool = True):
        super().__init__()
        self.model = model
        R0 = np.eye(3) if R0 is None else np.asarray(R0.detach().cpu() if isinstance(R0, torch.Tensor) else R0, dtype=np.float64)
        if R0.shape != (3, 3) and (R0.ndim != 3 or R0.shape[1:] != (3, 3)):
            raise ValueError("R0 must be [3, 3] or [F, 3, 3]")
        self.R0 = R0
        self.beta_per_frame = bool(beta_per_frame)
        self.use_shape = bool(use_shape)
        self.pose_blend = bool(pose_blend)
        self._problems: dict[int, object] = {}
        self._chunk_problems: dict[tuple, object] = {}

    def problem(self, F: int):
        """The keypoint-free problem the layer runs F frames on (created on first use)."""
        p = self._problems.get(F)
        if p is None:
            if self.R0.ndim == 3 and self.R0.shape[0] != F:
                raise ValueError(f"this layer's R0 is for {self.R0.shape[0]} frames, got {F}")
            R0 = self.R0 if self.R0.ndim == 3 else np.broadcast_to(self.R0, (F, 3, 3))
            p = api.Problem(self.model, np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)),
                            (1.0, 1.0, 0.0, 0.0), np.ascontiguousarray(R0), n_cols=api.N_FRAME_PARAMS + self.model.n_shape,
                            use_shape=self.use_shape, beta_per_frame=self.beta_per_frame, pose_blend=self.pose_blend,
                            want_mesh=True)
            self._problems[F] = p
        return p

    def chunk_problem(self, first: int, count: int):
        """The keypoint-free problem for frames first .. first + count - 1 of a longer sequence: problem(count) when every frame
        shares one R0, else a problem of its own on that slice of the per-frame R0.  A problem's R0 is fixed and its JVP scratch
        is its own, so the layer keeps ONE such problem: asking for another slice destroys the previous one (which waits for the
        device) before the new one is created, and the library's memory stays that of one chunk however many chunks a sequence
        has."""
        if self.R0.ndim == 2:
            return self.problem(count)
        key = (first, count)
        p = self._chunk_problems.get(key)
        if p is None:
            if first < 0 or first + count > self.R0.shape[0]:
                raise ValueError(f"this layer's R0 is for {self.R0.shape[0]} frames, got frames {first} .. {first + count - 1}")
            for old in self._chunk_problems.values():
                old.close()
            self._chunk_problems.clear()
            p = api.Problem(self.model, np.zeros(count + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)),
                            (1.0, 1.0, 0.0, 0.0), np.ascontiguousarray(self.R0[first:first + count]),
                            n_cols=api.N_FRAME_PARAMS + self.model.n_shape, use_shape=self.use_shape,
                            beta_per_frame=self.beta_per_frame, pose_blend=self.pose_blend, want_mesh=True)
            self._chunk_problems[key] = p
        return p

    def _check(self, x, beta):
        if not isinstance(x, torch.Tensor) or not isinstance(beta, torch.Tensor):
            raise TypeError("x and beta must be torch tensors")
        if not (x.is_cuda and beta.is_cuda):
            raise ValueError("x and beta must be on the GPU")
        if x.dtype != torch.float64 or beta.dtype != torch.float64:
            raise TypeError("x and beta must be float64")
        if x.ndim != 2 or x.shape[1] != api.N_FRAME_PARAMS or x.shape[0] < 1:
            raise ValueError(f"x must be [F, {api.N_FRAME_PARAMS}], got {tuple(x.shape)}")
        F, nS = x.shape[0], self.model.n_shape
        want_b = (F, nS) if self.beta_per_frame else (nS,)
        if tuple(beta.shape) != want_b:
            raise ValueError(f"beta must be {list(want_b)}, got {list(beta.shape)}")
        if x.device.index != self.model.device or beta.device != x.device:
            raise ValueError(f"x and beta must be on cuda:{self.model.device}")
        return F

    def _check_offsets(self, offsets, x, F):
        """the checked offsets, contiguous: f32 on x's GPU, [V, 3] (shared by the frames) or [F, V, 3]"""
        V = self.model.n_verts
        if not isinstance(offsets, torch.Tensor):
            raise TypeError("offsets must be a torch tensor")
        if offsets.dtype != torch.float32:
            raise TypeError("offsets must be float32")
        if not offsets.is_cuda or offsets.device != x.device:
            raise ValueError(f"offsets must be on cuda:{self.model.device}")
        if tuple(offsets.shape) not in ((V, 3), (F, V, 3)):
            raise ValueError(f"offsets must be [{V}, 3] or [{F}, {V}, 3], got {list(offsets.shape)}")
        if self.model.n_joints != 24:
            raise ValueError("offsets need a model with 24 joints")
        return offsets.contiguous()

    def forward(self, x: torch.Tensor, beta: torch.Tensor, offsets: torch.Tensor | None = None):
        """(verts [F, V, 3] f32, joints [F, nJ, 3] f64).  offsets: None, or per-vertex displacements f32 on the same GPU, [V, 3]
        shared by the frames or [F, V, 3], added to the blended rest vertex before skinning (SMPL+D); differentiable like x and
        beta, with an f32 gradient of its own shape.  The joints are those of the undisplaced shape."""
        F = self._check(x, beta)
        if offsets is None:
            return _SMPLForward.apply(x.contiguous(), beta.contiguous(), self.problem(F), self.model.n_verts, self.model.n_joints)
        offsets = self._check_offsets(offsets, x, F)
        return _SMPLForwardOffsets.apply(x.contiguous(), beta.contiguous(), offsets, self.problem(F), self.model.n_verts,
                                         self.model.n_joints)

    def jvp(self, x: torch.Tensor, beta: torch.Tensor, tan_x: torch.Tensor | None, tan_beta: torch.Tensor | None = None,
            offsets: torch.Tensor | None = None):
        """Forward-mode tangents of forward(x, beta) along K tangents at once (bodyfit_forward_jvp_device, HIP kernels in
        k_forward_jvp.hip; nothing is recorded for autograd): tan_x [F, K, 76] f64 (None: zero) and tan_beta [K, nS], or
        [F, K, nS] with beta_per_frame (None: zero), give (tan_verts [F, K, V, 3] f32, tan_joints [F, K, nJ, 3] f64).  The result
        for a (frame, tangent) pair does not depend on F, K or the tangent's position, bit for bit.  offsets (as forward's): the
        tangents are those of forward(x, beta, offsets) with the offsets held constant."""
        F = self._check(x, beta)
        if offsets is not None:
            offsets = self._check_offsets(offsets, x, F).detach()
        nS = self.model.n_shape
        if tan_x is None and tan_beta is None:
            raise ValueError("give tan_x or tan_beta")
        for name, t in (("tan_x", tan_x), ("tan_beta", tan_beta)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch tensor")
            if not t.is_cuda or t.device != x.device:
                raise ValueError(f"{name} must be on cuda:{self.model.device}")
            if t.dtype != torch.float64:
                raise TypeError(f"{name} must be float64")
        if tan_x is not None:
            if tan_x.ndim != 3 or tan_x.shape[0] != F or tan_x.shape[2] != api.N_FRAME_PARAMS or tan_x.shape[1] < 1:
                raise ValueError(f"tan_x must be [{F}, K, {api.N_FRAME_PARAMS}], got {tuple(tan_x.shape)}")
            K = tan_x.shape[1]
        else:
            if tan_beta.ndim < 2 or tan_beta.shape[-2] < 1:
                raise ValueError(f"tan_beta must be [K, {nS}] or [F, K, {nS}], got {tuple(tan_beta.shape)}")
            K = tan_beta.shape[-2]
        if tan_beta is not None:
            want_tb = (F, K, nS) if self.beta_per_frame else (K, nS)
            if tuple(tan_beta.shape) != want_tb:
                raise ValueError(f"tan_beta must be {list(want_tb)}, got {list(tan_beta.shape)}")
        x, beta = x.detach().contiguous(), beta.detach().contiguous()
        tan_x = tan_x.detach().contiguous() if tan_x is not None else None
        tan_beta = tan_beta.detach().contiguous() if tan_beta is not None else None
        V, nJ = self.model.n_verts, self.model.n_joints
        tan_verts = torch.empty((F, K, V, 3), dtype=torch.float32, device=x.device)
        tan_joints = torch.empty((F, K, nJ, 3), dtype=torch.float64, device=x.device)
        self.problem(F).forward_jvp_device(x.data_ptr(), beta.data_ptr(), K, tan_x.data_ptr() if tan_x is not None else None,
                                           tan_beta.data_ptr() if tan_beta is not None else None, tan_joints.data_ptr(),
                                           tan_verts.data_ptr(), 3 * V, _stream(),
                                           d_offsets_ptr=offsets.data_ptr() if offsets is not None else None,
                                           offsets_frame_stride=3 * V if (offsets is not None and offsets.ndim == 3) else 0)
        return tan_verts, tan_joints

    def jacobian(self, x: torch.Tensor, beta: torch.Tensor, offsets: torch.Tensor | None = None):
        """The dense Jacobian of forward(x, beta): jvp with the P = 76 + nS unit tangents.  (Jv [F, P, V, 3] f32,
        Jj [F, P, nJ, 3] f64); slice p < 76 is the derivative w.r.t. frame parameter p of that frame, slice 76 + i the
        derivative w.r.t. beta_i (of that frame's beta with beta_per_frame, of the shared beta otherwise).  offsets: as jvp's."""
        F = self._check(x, beta)
        nP, nS = api.N_FRAME_PARAMS, self.model.n_shape
        P = nP + nS
        eye = torch.eye(P, dtype=torch.float64, device=x.device)
        tan_x = eye[:, :nP].expand(F, P, nP).contiguous()
        tan_beta = None
        if nS > 0:
            tan_beta = eye[:, nP:].expand(F, P, nS).contiguous() if self.beta_per_frame else eye[:, nP:].contiguous()
        return self.jvp(x, beta, tan_x, tan_beta, offsets=offsets)


def huber_rho(delta: float, s: torch.Tensor) -> torch.Tensor:
    """ceres::HuberLoss(delta).rho of squared norms s: s inside delta^2, 2 delta sqrt(s) - delta^2 beyond (delta <= 0: s)."""
    if delta <= 0.0:
        return s
    d2 = delta * delta
    # (the clamp keeps sqrt's derivative finite in the branch torch.where discards)
    return torch.where(s > d2, 2.0 * delta * torch.sqrt(torch.clamp(s, min=d2)) - d2, s)


class _Objective(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, beta, obj):
        prob = obj.problem
        r = torch.empty(prob.layout.total_rows, dtype=torch.float64, device=x.device)
        prob.residuals_device(x.data_ptr(), beta.data_ptr() if beta is not None else None, r.data_ptr(), None, True, _stream())
        ctx.obj = obj
        ctx.generation = prob.generation
        ctx.has_beta = beta is not None
        ctx.save_for_backward(x, beta if beta is not None else x)
        return r

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, beta = ctx.saved_tensors
        if not ctx.has_beta:
            beta = None
        prob = ctx.obj.problem
        g = g.to(torch.float64).contiguous()
        gx = torch.empty_like(x)
        gb = torch.empty_like(beta) if beta is not None else None
        # nothing else swept on the problem since this forward: its Jacobian is still in the problem's buffers
        reuse = prob.generation == ctx.generation
        prob.residual_vjp_device(x.data_ptr(), beta.data_ptr() if beta is not None else None, g.data_ptr(), gx.data_ptr(),
                                 gb.data_ptr() if gb is not None else None, reuse, _stream())
        return (gx if ctx.needs_input_grad[0] else None), (gb if ctx.needs_input_grad[1] else None), None


class FitObjective(torch.nn.Module):
    """The residual vector of an api.Problem (keypoint reprojection, pose / shape priors, temporal terms) as a differentiable
    function of the frame parameters x [F(+1), 7 + 3 (nJ - 1)] and beta ([nS] shared, [F, nS] per frame; None without the shape
    block), f64 on the problem's GPU, on torch.cuda.current_stream().

    forward sweeps with the Jacobian when x or beta requires grad (the residual-only sweep otherwise); backward is
    bodyfit_residual_vjp_device, which reuses that Jacobian unless another sweep ran on the problem in between (then it sweeps
    again at the saved point).  An optimiser closure thus costs one sweep per evaluation.  The problem's buffers are shared by
    every call on it: calls on several streams at once need the caller's own ordering.
    """

    def __init__(self, problem):
        super().__init__()
        self.problem = problem

    def _check(self, x, beta):
        p = self.problem
        if not isinstance(x, torch.Tensor) or (beta is not None and not isinstance(beta, torch.Tensor)):
            raise TypeError("x and beta must be torch tensors")
        if x.dtype != torch.float64 or (beta is not None and beta.dtype != torch.float64):
            raise TypeError("x and beta must be float64")
        if not x.is_cuda or x.device.index != p.model.device or (beta is not None and beta.device != x.device):
            raise ValueError(f"x and beta must be on cuda:{p.model.device}")
        if tuple(x.shape) != (p.n_param_rows, p.n_frame_params):
            raise ValueError(f"x must be [{p.n_param_rows}, {p.n_frame_params}], got {tuple(x.shape)}")
        if p.n_cols > p.n_frame_params:
            nS = p.model.n_shape
            want_b = (p.n_frames, nS) if p.beta_per_frame else (nS,)
            if beta is None or tuple(beta.shape) != want_b:
                raise ValueError(f"beta must be {list(want_b)}, got {None if beta is None else list(beta.shape)}")
        elif beta is not None:
            raise ValueError("this problem has no shape block: beta must be None")

    def forward(self, x: torch.Tensor, beta: torch.Tensor | None = None) -> torch.Tensor:
        self._check(x, beta)
        x = x.contiguous()
        beta = beta.contiguous() if beta is not None else None
        if torch.is_grad_enabled() and (x.requires_grad or (beta is not None and beta.requires_grad)):
            return _Objective.apply(x, beta, self)
        p = self.problem
        r = torch.empty(p.layout.total_rows, dtype=torch.float64, device=x.device)
        p.residuals_device(x.data_ptr(), beta.data_ptr() if beta is not None else None, r.data_ptr(), None, False, _stream())
        return r

    def cost(self, r: torch.Tensor) -> torch.Tensor:
        """The Ceres cost of residuals r: 1/2 rho(r_u^2 + r_v^2) per keypoint block (HuberLoss(huber_delta) of the problem) plus
        1/2 |r|^2 of the prior and temporal rows; differentiable through r."""
        K2 = self.problem.layout.reproj_rows
        kp = r[:K2].view(-1, 2)
        rest = r[K2:]
        return 0.5 * huber_rho(self.problem.huber_delta, (kp * kp).sum(dim=1)).sum() + 0.5 * (rest * rest).sum()


# ---- 3-D point-cloud term -----------------------------------------------------------------------------------------------
_closest_handles: dict[int, object] = {}


def _closest_handle(device_index: int):
    h = _closest_handles.get(device_index)
    if h is None:
        h = _closest_handles[device_index] = api.ClosestPoints(device_index)
    return h


def _point_set(name: str, t, offset):
    """(tensor to keep alive, api.PointSet, frames, rows) of a uniform [F, n, 3] or ragged [N, 3] + offset [F + 1] point tensor."""
    if not isinstance(t, torch.Tensor) or (offset is not None and not isinstance(offset, torch.Tensor)):
        raise TypeError(f"{name} and its offset must be torch tensors")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU")
    if offset is None:
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError(f"{name} must be [F, n, 3] (or [N, 3] with an offset), got {tuple(t.shape)}")
        F, n = t.shape[0], t.shape[1]
        # a view with a frame stride of its own (the library's padded cloud) is used in place when its [n, 3] blocks are dense
        dense = t.stride(2) == 1 and t.stride(1) == 3 and (F == 1 or t.stride(0) >= 3 * n)
        if not dense or F * n == 0:
            t = t.contiguous()
        stride = t.stride(0) if F > 1 and F * n > 0 else 3 * n
        return t, api.PointSet.uniform(t.data_ptr(), n, stride), F, F * n
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} with an offset must be [N, 3], got {tuple(t.shape)}")
    if offset.dtype != torch.int32 or offset.ndim != 1 or offset.shape[0] < 1:
        raise TypeError(f"{name}'s offset must be an int32 tensor [F + 1]")
    if offset.device != t.device:
        raise ValueError(f"{name} and its offset must be on the same GPU")
    t = t.contiguous()
    offset = offset.contiguous()
    ps = api.PointSet.ragged(t.data_ptr(), offset.data_ptr())
    ps._keep = offset
    return t, ps, offset.shape[0] - 1, t.shape[0]


def _grad_like(t: torch.Tensor, ps) -> torch.Tensor:
    """an uninitialised gradient in the layout of point set ps (whose tensor is t)"""
    if ps.d_offset is None and t.ndim == 3 and t.shape[0] > 1 and t.stride(0) != 3 * t.shape[1]:
        F, n = t.shape[0], t.shape[1]
        return torch.empty((F, t.stride(0)), dtype=torch.float32, device=t.device)[:, :3 * n].view(F, n, 3)
    return torch.empty(t.shape, dtype=torch.float32, device=t.device)


def _grads_for(ctx, sets, live: bool):
    """the gradients of a backward's two point tensors, ((tensor, ps), (tensor, ps)): uninitialised where the VJP kernel will
    write them (live), zero otherwise, None where ctx needs none"""
    grads = [_grad_like(t, ps) if want else None for (t, ps), want in zip(sets, ctx.needs_input_grad)]
    if not live:
        for g in grads:
            if g is not None:
                g.zero_()
    return grads


def _rho_sum(dist2: torch.Tensor, index: torch.Tensor, trunc: float | None) -> torch.Tensor:
    """the f64 sum of rho(dist2) over the rows with a counterpart (a row without one: index -1, dist2 +inf, costs nothing)"""
    s = torch.where(index >= 0, dist2, torch.zeros_like(dist2))
    if trunc is not None:
        s = torch.clamp(s, max=trunc * trunc)
    return s.double().sum()


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



# ---- scan -> surface term -------------------------------------------------------------------------------------------------
_surface_handles: dict[tuple, tuple] = {}   # (device, V, n_faces, content hash) -> (the faces' bytes, api.Surface); the last _SURFACE_CACHE in use
_SURFACE_CACHE = 8


def _host_faces(faces) -> np.ndarray:
    """the checked int32 [n_faces, 3] host array of `faces` (a CUDA tensor is copied to the host: a synchronisation)"""
    if isinstance(faces, torch.Tensor):
        if faces.dtype != torch.int32:
            raise TypeError("faces must be int32")
        f = faces.detach().cpu().numpy()
    else:
        f = np.asarray(faces)
        if f.dtype != np.int32:
            raise TypeError("faces must be int32")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be [n_faces, 3], got {tuple(f.shape)}")
    return np.ascontiguousarray(f)


def _surface_handle(device_index: int, n_verts: int, faces):
    """The api.Surface of (device, topology).  An api.Surface is used as it is.  Anything else is keyed on its CONTENT (hashed on
    every call and compared byte for byte on a hit, so an array changed in place is a new topology); the cache keeps the handles of the last _SURFACE_CACHE
    topologies, an evicted handle is released when the last backward that holds it has run."""
    if isinstance(faces, api.Surface):
        if faces.device != device_index or faces.n_verts != n_verts:
            raise ValueError(f"this Surface is for cuda:{faces.device} and {faces.n_verts} vertices, got cuda:{device_index} and {n_verts}")
        return faces
    return _topology_handle(_surface_handles, device_index, n_verts, faces, (),
                            lambda f: api.Surface(device_index, n_verts, f))


def _topology_handle(cache: dict, device_index: int, n_verts: int, faces, extra: tuple, make):
    """the handle make(faces) of (device, topology, extra) in `cache`, keyed on the faces' content as _surface_handle describes"""
    f = _host_faces(faces)
    raw = f.tobytes()
    key = (device_index, int(n_verts), f.shape[0], hash(raw)) + extra
    hit = cache.pop(key, None)
    if hit is not None and hit[0] != raw:        # (two topologies under one hash: the kept one makes way)
        hit = None
    if hit is None:
        if f.size and (int(f.min()) < 0 or int(f.max()) >= n_verts):
            raise ValueError(f"faces holds an id outside [0, {n_verts})")
        hit = (raw, make(f))
    cache[key] = hit                                # (most recently used last)
    while len(cache) > _SURFACE_CACHE:
        cache.pop(next(iter(cache)))
    return hit[1]


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


class SurfaceTerm(torch.nn.Module):
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
        self._handles: dict[tuple, object] = {}  # (device, V) -> api.Surface, owned by the term
        self._offset_host = None

    def forward(self, verts: torch.Tensor) -> torch.Tensor:
        faces = self.faces
        if isinstance(verts, torch.Tensor) and verts.is_cuda and verts.ndim == 3:
            faces = self._handle_for(verts)
        dist2, index, _ = closest_surface(self.points, verts, faces, query_offset=self.offset, point_normals=self.normals,
                                          min_cos=self.min_cos)
        return _rho_sum(dist2, index, self.trunc)

    def _handle_for(self, verts: torch.Tensor):
        key = (verts.device.index, verts.shape[1])
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = _surface_handle(key[0], key[1], self.faces)
        return h


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


# ---- inside / outside: winding numbers, vertex normals, the signed distance and the self-penetration term ----------------------
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


class OffsetRegulariser(torch.nn.Module):
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
        self._handles: dict[tuple, object] = {}

    def forward(self, offsets: torch.Tensor) -> torch.Tensor:
        handle = self.faces
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.ndim in (2, 3):
            key = (offsets.device.index, offsets.shape[-2])
            handle = self._handles.get(key)
            if handle is None:
                handle = self._handles[key] = _surface_handle(key[0], key[1], self.faces)
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


class SelfPenetrationTerm(torch.nn.Module):
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
        self._handles: dict[tuple, object] = {}  # (device, V) -> api.Surface, owned by the term

    def _handle_for(self, verts: torch.Tensor):
        key = (verts.device.index, verts.shape[1])
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = _surface_handle(key[0], key[1], self.faces)
        return h

    def evaluate(self, verts: torch.Tensor) -> dict:
        """The term's parts: winding [F, K] f32, inside [F, K] bool, offset int32 [F + 1] (the CSR of the enclosed vertices), rows
        [n] int64 (their vertex ids), and dist2 [n] (with the term's gradient), index [n], bary [n, 3] of their matches; K = V or
        len(vertex_ids).  Without an enclosed vertex the last four are empty."""
        if (not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32 or not verts.is_cuda or verts.ndim != 3
                or verts.shape[2] != 3):
            raise TypeError("verts must be a float32 tensor [F, V, 3] on the GPU")
        handle = self._handle_for(verts)
        vd = verts.detach()
        _vertex_ids(self.vertex_ids, vd.shape[1])
        winding = vertex_winding(vd, handle, self.vertex_ids)
        inside = winding > 1.0
        offset = torch.zeros(inside.shape[0] + 1, dtype=torch.int32, device=vd.device)
        offset[1:] = inside.sum(dim=1).cumsum(0).to(torch.int32)
        frame, col = torch.nonzero(inside, as_tuple=True)        # frame-major: the packed order of a ragged set (a synchronisation)
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


# ---- depth render, visibility and the depth-map term ------------------------------------------------------------------------------
_raster_handles: dict[tuple, tuple] = {}   # (device, V, n_faces, content hash, H, W) -> (the faces' bytes, api.Raster)


def _raster_handle(device_index: int, n_verts: int, faces, size):
    """The api.Raster of (device, topology, image size), kept like _surface_handle's: keyed on the faces' content, the last
    _SURFACE_CACHE in use."""
    H, W = int(size[0]), int(size[1])
    return _topology_handle(_raster_handles, device_index, n_verts, faces, (H, W),
                            lambda f: api.Raster(device_index, n_verts, f, W, H))


def _render(verts, faces, intr, size, z_near, cull_backfaces, want_bary):
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


# ---- depth residual: the ray-plane depth of the rendered face under a pixel, and its gradient --------------------------------
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


class DepthResidualTerm(torch.nn.Module):
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
        self._handles: dict[tuple, object] = {}
        self._offset_host = None

    def _handle_for(self, verts: torch.Tensor):
        key = (verts.device.index, verts.shape[1])
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = _surface_handle(key[0], key[1], self.faces)
        return h

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
        if self.trunc is not None:
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


# ---- silhouette: the exact distance transform of masks, and the outline term -------------------------------------------------
_NO_FACES = np.zeros((0, 3), np.int32)


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


class SilhouetteTerm(torch.nn.Module):
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
        self._handles: dict[tuple, object] = {}

    def _handle_for(self, verts: torch.Tensor):
        key = (verts.device.index, verts.shape[1])
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = _surface_handle(key[0], key[1], self.faces)
        return h

    def _rho(self, s: torch.Tensor) -> torch.Tensor:
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


# ---- vertex colours: attribute render, image sampling, colour fusion and the photometric term -----------------------------------
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
        dev = face.device
        g = None
        if ctx.needs_input_grad[0]:
            g = torch.zeros((F, V, C), dtype=torch.float32, device=dev)
            if g_image is not None and F * V * ppf > 0:
                N = F * ppf
                gi = g_image.to(torch.float32).reshape(N, C)
                coef = torch.ones(N, dtype=torch.float32, device=dev)
                rows = api.PointSet.uniform(face.data_ptr(), ppf, 3 * ppf)      # (the rows' frame structure; its xyz is never read)
                for c0 in range(0, C, 3):
                    n = min(3, C - c0)
                    direction = torch.zeros((N, 3), dtype=torch.float32, device=dev)
                    direction[:, :n] = gi[:, c0:c0 + n]
                    gv = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
                    with torch.cuda.device(dev):
                        surface.rows_vjp_device(rows, F, N, face.data_ptr(), weight.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                                gv.data_ptr(), 3 * V, _stream())
                    g[:, :, c0:c0 + n] = gv[:, :, :n]
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
        frame, pix = torch.nonzero((weight != 0).any(dim=-1).reshape(F, ppf), as_tuple=True)
        N = int(pix.shape[0])
    if N == 0:
        gv.zero_()
        return gv
    pixel = pix.to(torch.int32).contiguous()
    offset = torch.zeros(F + 1, dtype=torch.int32, device=dev)
    offset[1:] = torch.bincount(frame, minlength=F).cumsum(0).to(torch.int32)
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


def _check_intr_size(intr, size):
    if len(intr) != 4 or len(size) != 2:
        raise ValueError("intr is (fx, fy, cx, cy), size is (height, width)")


def _check_verts(verts, name="verts"):
    if not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor on the GPU")
    if verts.ndim != 3 or verts.shape[2] != 3:
        raise ValueError(f"{name} must be [F, V, 3], got {tuple(verts.shape)}")
    if not verts.is_cuda:
        raise TypeError(f"{name} must be on the GPU")


def _check_per_vertex(t, name, F: int, V: int, device):
    """a per-vertex f32 tensor [V, C] or [F, V, C], C in 1 .. 4, on `device`"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor on the GPU")
    if t.ndim not in (2, 3) or t.shape[-2] != V or not 1 <= t.shape[-1] <= 4 or (t.ndim == 3 and t.shape[0] != F):
        raise ValueError(f"{name} must be [V, C] or [F, V, C] with V = {V}, F = {F} and C in 1 .. 4, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise TypeError(f"{name} must be on the GPU")
    if t.device != device:
        raise ValueError(f"{name} and verts must be on the same GPU")


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
    C = attr.shape[-1]
    bg = np.atleast_1d(np.asarray(background, np.float32))
    if bg.ndim != 1 or bg.shape[0] not in (1, C):
        raise ValueError(f"background must be a float or {C} floats")
    image, face, _ = _RenderAttributes.apply(attr, verts, faces, intr, size, bg, float(z_near), bool(cull_backfaces), bool(interior))
    return image, face


# ---- silhouette-edge antialiasing: the render's coverage as a smooth function of the vertices -----------------------------------
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
            frame, code = torch.nonzero(w.reshape(F, -1), as_tuple=True)
            N = int(code.shape[0])
            if N == 0 or v.shape[1] == 0:
                gv.zero_()
            else:
                pair = code.to(torch.int32).contiguous()
                offset = torch.zeros(F + 1, dtype=torch.int32, device=dev)
                offset[1:] = torch.bincount(frame, minlength=F).cumsum(0).to(torch.int32)
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


_NO_FACES = np.zeros((0, 3), np.int32)


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
        img, kind = _check_images(images)
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        self.intr = tuple(float(a) for a in intr)
        self.size, self.z_near = (int(img.shape[1]), int(img.shape[2])), float(z_near)
        self.trunc = None if trunc is None else float(trunc)
        self.min_cos = None if min_cos is None else float(min_cos)
        self.owner = bool(owner)
        self.faces = _host_faces(faces).copy()
        self.register_buffer("images", img)
        self.register_buffer("faces_device", torch.from_numpy(self.faces).to(img.device).long().reshape(-1, 3))

    def evaluate(self, verts: torch.Tensor, colours: torch.Tensor) -> dict:
        """term(verts, colours) with what it was built from: cost (f64, with the gradient), gate bool [F, V] (the live set before
        the sample's own validity), valid bool [F, V] (the rows that count), value f32 [F, V, C] (the samples, 0 where not valid),
        sq f64 [F, V] (the squared colour distance of a valid row, else 0) and n_truncated"""
        _check_verts(verts)
        F, V = verts.shape[0], verts.shape[1]
        _check_per_vertex(colours, "colours", F, V, verts.device)
        if self.images.device != verts.device or self.images.shape[0] != F:
            raise ValueError(f"the images have {self.images.shape[0]} frames on {self.images.device}, verts has {F} on {verts.device}")
        if colours.shape[-1] != self.images.shape[3]:
            raise ValueError(f"colours has {colours.shape[-1]} channels, the images {self.images.shape[3]}")
        with torch.no_grad():
            if self.faces.shape[0]:
                gate, _ = _colour_gate(verts, self.faces, self.faces_device, self.intr, self.size, self.min_cos, self.owner,
                                       self.z_near)
            else:
                gate = torch.zeros((F, V), dtype=torch.bool, device=verts.device)
        value, valid = sample_images(self.images, verts, self.intr, gate=gate, z_near=self.z_near)
        diff = value.double() - (colours if colours.ndim == 3 else colours.unsqueeze(0)).double()
        sq = torch.where(valid, diff.square().sum(dim=-1), torch.zeros((), dtype=torch.float64, device=verts.device))
        n_cut = torch.zeros((), dtype=torch.long, device=verts.device)
        rho = sq
        if self.trunc is not None:
            n_cut = (sq.detach() > self.trunc * self.trunc).sum()
            rho = torch.clamp(sq, max=self.trunc * self.trunc)
        return {"cost": rho.sum(), "gate": gate, "valid": valid, "value": value, "sq": sq, "n_truncated": n_cut}

    def forward(self, verts: torch.Tensor, colours: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts, colours)["cost"]


class RenderedPhotometricTerm(torch.nn.Module):
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
        super().__init__()
        img, _ = _check_images(images)
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        C = int(img.shape[3])
        bg = np.atleast_1d(np.asarray(background, np.float32))
        if bg.ndim != 1 or bg.shape[0] not in (1, C):
            raise ValueError(f"background must be a float or {C} floats")
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != img.device:
                raise TypeError("mask must be a bool or uint8 tensor [F, H, W] on the GPU of the images")
            if tuple(mask.shape) != tuple(img.shape[:3]):
                raise ValueError(f"mask must be {tuple(img.shape[:3])}, got {tuple(mask.shape)}")
        self.intr = tuple(float(a) for a in intr)
        self.size, self.z_near, self.cull_backfaces = (int(img.shape[1]), int(img.shape[2])), float(z_near), bool(cull_backfaces)
        self.trunc = None if trunc is None else float(trunc)
        self.background, self.antialias = bg, bool(antialias)
        self.faces = _host_faces(faces).copy()
        self.register_buffer("images", img)
        self.register_buffer("mask", None if mask is None else (mask != 0).contiguous())

    def evaluate(self, verts: torch.Tensor, colours: torch.Tensor) -> dict:
        """term(verts, colours) with what it was built from: cost (f64, with the gradient), image f32 [F, H, W, C] (what was
        compared with the video: antialiased or not), the render (depth, face), sq f64 [F, H, W] (the squared colour distance of a
        pixel of the mask, else 0) and n_truncated"""
        _check_verts(verts)
        F, V = verts.shape[0], verts.shape[1]
        _check_per_vertex(colours, "colours", F, V, verts.device)
        if self.images.device != verts.device or self.images.shape[0] != F:
            raise ValueError(f"the images have {self.images.shape[0]} frames on {self.images.device}, verts has {F} on {verts.device}")
        if colours.shape[-1] != self.images.shape[3]:
            raise ValueError(f"colours has {colours.shape[-1]} channels, the images {self.images.shape[3]}")
        image, face, depth = _RenderAttributes.apply(colours, verts, self.faces, self.intr, self.size, self.background, self.z_near,
                                                     self.cull_backfaces, True)
        if self.antialias:
            image = antialias(image, verts, self.faces, self.intr, render=(depth, face), z_near=self.z_near,
                              cull_backfaces=self.cull_backfaces)
        sq = (image.double() - self.images.double()).square().sum(dim=-1)
        if self.mask is not None:
            sq = torch.where(self.mask, sq, torch.zeros((), dtype=torch.float64, device=verts.device))
        n_cut = torch.zeros((), dtype=torch.long, device=verts.device)
        rho = sq
        if self.trunc is not None:
            n_cut = (sq.detach() > self.trunc * self.trunc).sum()
            rho = torch.clamp(sq, max=self.trunc * self.trunc)
        return {"cost": rho.sum(), "image": image, "depth": depth, "face": face, "sq": sq, "n_truncated": n_cut}

    def forward(self, verts: torch.Tensor, colours: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts, colours)["cost"]


# ---- uv textures: the texture lookup over a render, its gradients in the texels, in uv and in the vertices ----------------------
def _check_atlas(uv, uv_faces, n_faces: int, device):
    """(uv f32 [T, 2] contiguous on `device`, the host int32 [n_faces, 3] table, the same table on the device)"""
    if not isinstance(uv, torch.Tensor) or uv.dtype != torch.float32 or not uv.is_cuda:
        raise TypeError("uv must be a float32 tensor on the GPU")
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise ValueError(f"uv must be [T, 2], got {tuple(uv.shape)}")
    if uv.device != device:
        raise ValueError("uv and verts must be on the same GPU")
    f = _host_faces(uv_faces)
    if f.shape[0] != n_faces:
        raise ValueError(f"uv_faces must be [{n_faces}, 3], one row per face, got {f.shape}")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= uv.shape[0]):
        raise ValueError(f"uv_faces holds a row outside [0, {uv.shape[0]})")
    fd = uv_faces if isinstance(uv_faces, torch.Tensor) and uv_faces.device == device else torch.from_numpy(f).to(device)
    return f, fd.contiguous()


def _check_texture(tex, F: int, device):
    """(kind, shared) of a texture [Ht, Wt, C] or [F, Ht, Wt, C], uint8 (raw 0 .. 255) or float32, C in 1 .. 4, on `device`"""
    if not isinstance(tex, torch.Tensor) or tex.dtype not in (torch.uint8, torch.float32) or not tex.is_cuda:
        raise TypeError("tex must be a uint8 or float32 tensor on the GPU")
    if tex.ndim not in (3, 4) or not 1 <= tex.shape[-1] <= 4 or tex.shape[-2] < 1 or tex.shape[-3] < 1 or (tex.ndim == 4 and tex.shape[0] != F):
        raise ValueError(f"tex must be [Ht, Wt, C] or [F, Ht, Wt, C] with F = {F} and C in 1 .. 4, got {tuple(tex.shape)}")
    if tex.device != device:
        raise ValueError("tex and verts must be on the same GPU")
    return (0 if tex.dtype == torch.uint8 else 1), tex.ndim == 3


class _RenderTexture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, verts, faces, intr, size, uv_faces, uv_faces_device, background, z_near, cull_backfaces, interior):
        raster, depth, face, bary = _render(verts, faces, intr, size, z_near, cull_backfaces, True)
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        H, W = int(size[0]), int(size[1])
        kind, shared = _check_texture(tex, F, v.device)
        t, u = tex.detach().contiguous(), uv.detach().contiguous()
        Ht, Wt, C = (int(n) for n in t.shape[-3:])
        image = torch.empty((F, H, W, C), dtype=torch.float32, device=v.device)
        weight = torch.empty((F, H, W, 3), dtype=torch.float32, device=v.device)
        look = (u.shape[0], kind, C, Ht, Wt, 0 if shared else Ht * Wt * C, F)
        if F > 0:
            with torch.cuda.device(v.device):
                raster.texture_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), look[0],
                                      uv_faces_device.data_ptr(), t.data_ptr(), kind, C, Ht, Wt, look[5], F, background,
                                      image.data_ptr(), weight.data_ptr(), None, _stream())
        want_tex = ctx.needs_input_grad[0] and kind == 1
        ctx.interior = bool(interior) and ctx.needs_input_grad[2]
        if want_tex or ctx.needs_input_grad[1] or ctx.interior:
            ctx.look = (raster, vs, tuple(float(x) for x in intr), look, uv_faces, want_tex, faces)
            ctx.save_for_backward(face, bary, weight, v, u, t, uv_faces_device)
        ctx.mark_non_differentiable(face, depth)
        return image, face, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g_image, _g_face, _g_depth):
        if not hasattr(ctx, "look"):
            return (None,) * 12
        face, bary, weight, v, u, t, uv_faces_device = ctx.saved_tensors
        raster, vs, intr, (T, kind, C, Ht, Wt, tex_stride, F), uv_faces, want_tex, faces = ctx.look
        dev, (H, W) = face.device, face.shape[1:]
        want_uv = ctx.needs_input_grad[1] or ctx.interior
        g_tex = torch.zeros(t.shape, dtype=torch.float32, device=dev) if want_tex else None
        g_uvpix = torch.zeros((F, H, W, 2), dtype=torch.float32, device=dev) if want_uv else None
        if g_image is not None and F * H * W > 0:
            gi = g_image.to(torch.float32).contiguous()
            work = torch.empty(t.shape, dtype=torch.int64, device=dev) if want_tex else None
            with torch.cuda.device(dev):
                raster.texture_grad_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), T,
                                           uv_faces_device.data_ptr(), t.data_ptr(), kind, C, Ht, Wt, tex_stride, F, gi.data_ptr(),
                                           g_uvpix.data_ptr() if want_uv else None, g_tex.data_ptr() if want_tex else None,
                                           work.data_ptr() if want_tex else None, _stream())
        g_uv = None
        if ctx.needs_input_grad[1]:
            # the pixels as rows of the ATLAS's own surface handle (T rows, uv_faces): g_uv[uv_faces[t][a]] += w_a (g_u, g_v, 0)
            g_uv = torch.zeros((T, 2), dtype=torch.float32, device=dev)
            N = F * H * W
            if g_image is not None and N * T > 0:
                atlas = _surface_handle(dev.index, T, uv_faces)
                direction = torch.zeros((N, 3), dtype=torch.float32, device=dev)
                direction[:, :2] = g_uvpix.reshape(N, 2)
                coef = torch.ones(N, dtype=torch.float32, device=dev)
                rows = api.PointSet.uniform(face.data_ptr(), H * W, 3 * H * W)      # (the rows' frame structure; its xyz is never read)
                gt = torch.empty((F, T, 3), dtype=torch.float32, device=dev)
                with torch.cuda.device(dev):
                    atlas.rows_vjp_device(rows, F, N, face.data_ptr(), weight.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                          gt.data_ptr(), 3 * T, _stream())
                g_uv = gt[:, :, :2].double().sum(dim=0).to(torch.float32)
        g_verts = None
        if ctx.interior:
            surface = _surface_handle(dev.index, v.shape[1], faces)
            g_verts = _interior_rows(raster, surface, v, vs, intr, face, weight, u, 0, 2, g_uvpix if g_image is not None else None,
                                     attr_faces=uv_faces_device, n_attr_rows=T)
        return (g_tex, g_uv, g_verts) + (None,) * 9


def render_texture(verts: torch.Tensor, faces, intr, size, uv: torch.Tensor, uv_faces, tex: torch.Tensor, background=0.0,
                   z_near: float = 0.1, cull_backfaces: bool = False, interior: bool = False):
    """The texture tex ([Ht, Wt, C] shared by the frames, or [F, Ht, Wt, C]; float32, or uint8 with raw values 0 .. 255; C in
    1 .. 4) on the posed meshes verts [F, V, 3] f32 as the camera intr sees them in an image of size = (height, width): (image
    [F, H, W, C] f32, face [F, H, W] int32).  The atlas: uv [T, 2] f32 (GPU) and uv_faces int32 [n_faces, 3] (host array or
    tensor), the rows of uv per face CORNER (an atlas has seams: T and V are unrelated).  render_depth's render (same arguments,
    same handle, one 8-byte read-back) followed by bodyfit_raster_texture_device: in a covered pixel the face's three uv rows
    with the shade's perspective-correct weights, then the bilinear texel lookup with texel (i, j) centred at (u, v) = ((j + 1/2)
    / Wt, (i + 1/2) / Ht), row 0 at the top, clamp-to-edge; elsewhere background (a float, or C floats).  The definition and its
    error bound: include/bodyfit.h.

    Differentiable at the FIXED face image and the fixed pixel rays in
      tex (float32 only), by bodyfit_raster_texture_grad_device: the exact adjoint of the lookup, summed in 64-bit integers (no
          float atomics: bit-identical from run to run and under any permutation of the frames; a shared texture gets all frames);
      uv, by the rows VJP on a second surface handle built from (T, uv_faces) with the pixels as rows (index = the face image, bary
          = the stored weights, direction = (g_u, g_v, 0)), the frames summed in f64;
      verts, with interior=True ONLY: how a pixel's uv changes as its face's corners move under it, the rows of
          bodyfit_raster_interp_rows_indexed_device with attr = uv and the upstream gradient (g_u, g_v), summed by one
          bodyfit_surface_rows_vjp_device call (one host synchronisation lists the shaded pixels, as render_attributes').
    NOT part of it: visibility and coverage (antialias(image, verts, ...) adds the gradient through coverage), z_near and
    culling.  NOT built: mipmaps or any minification filter: a body smaller on the screen than its atlas aliases, and the texels
    no pixel's cell touches get no gradient."""
    _check_verts(verts)
    _check_intr_size(intr, size)
    n_faces = _host_faces(faces).shape[0]
    uvf, uvf_device = _check_atlas(uv, uv_faces, n_faces, verts.device)
    _check_texture(tex, verts.shape[0], verts.device)
    C = tex.shape[-1]
    bg = np.atleast_1d(np.asarray(background, np.float32))
    if bg.ndim != 1 or bg.shape[0] not in (1, C):
        raise ValueError(f"background must be a float or {C} floats")
    image, face, _ = _RenderTexture.apply(tex, uv, verts, faces, intr, size, uvf, uvf_device, bg, float(z_near), bool(cull_backfaces),
                                          bool(interior))
    return image, face


class TexturedPhotometricTerm(torch.nn.Module):
    """RenderedPhotometricTerm with a uv texture in place of the vertex colours: antialias(render_texture(verts, tex,
    interior=True)) against the video.

    video: [F, H, W, C] or [F, H, W], uint8 (raw 0 .. 255) or float32, on the GPU; intr = (fx, fy, cx, cy); the atlas uv [T, 2] f32
    (GPU) and uv_faces int32 [n_faces, 3].  term(verts, tex), verts [F, V, 3] f32 and tex [Ht, Wt, C] or [F, Ht, Wt, C] f32 in
    the video's units, returns the f64 cost
      sum over the pixels p of mask of rho(sum_c (R_c(p) - I_c(p))^2),    rho(s) = min(s, trunc^2) (trunc None: rho(s) = s).
    Differentiable in tex (every covered pixel writes into the four texels of its cell) and in verts: through the uv
    interpolation inside the faces and, with antialias, through coverage at the silhouettes.  One render per evaluation.  No
    normal equations are built for it.  evaluate(verts, tex) returns the cost with its parts."""

    def __init__(self, video: torch.Tensor, intr, faces, uv: torch.Tensor, uv_faces, trunc: float | None = None, background=0.0,
                 mask: torch.Tensor | None = None, antialias: bool = True, z_near: float = 0.1, cull_backfaces: bool = False):
        super().__init__()
        img, _ = _check_images(video)
        if len(intr) != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        if not z_near > 0.0:
            raise ValueError("z_near must be positive")
        if trunc is not None and not trunc > 0.0:
            raise ValueError("trunc must be positive")
        C = int(img.shape[3])
        bg = np.atleast_1d(np.asarray(background, np.float32))
        if bg.ndim != 1 or bg.shape[0] not in (1, C):
            raise ValueError(f"background must be a float or {C} floats")
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != img.device:
                raise TypeError("mask must be a bool or uint8 tensor [F, H, W] on the GPU of the video")
            if tuple(mask.shape) != tuple(img.shape[:3]):
                raise ValueError(f"mask must be {tuple(img.shape[:3])}, got {tuple(mask.shape)}")
        self.intr = tuple(float(a) for a in intr)
        self.size, self.z_near, self.cull_backfaces = (int(img.shape[1]), int(img.shape[2])), float(z_near), bool(cull_backfaces)
        self.trunc = None if trunc is None else float(trunc)
        self.background, self.antialias = bg, bool(antialias)
        self.faces = _host_faces(faces).copy()
        self.uv_faces, uvf_device = _check_atlas(uv, uv_faces, self.faces.shape[0], img.device)
        self.register_buffer("images", img)
        self.register_buffer("mask", None if mask is None else (mask != 0).contiguous())
        self.register_buffer("uv", uv.detach().contiguous())
        self.register_buffer("uv_faces_device", uvf_device)

    def evaluate(self, verts: torch.Tensor, tex: torch.Tensor) -> dict:
        """term(verts, tex) with what it was built from: cost (f64, with the gradient), image f32 [F, H, W, C] (what was compared
        with the video: antialiased or not), the render (depth, face), sq f64 [F, H, W] and n_truncated"""
        _check_verts(verts)
        F = verts.shape[0]
        if self.images.device != verts.device or self.images.shape[0] != F:
            raise ValueError(f"the video has {self.images.shape[0]} frames on {self.images.device}, verts has {F} on {verts.device}")
        _check_texture(tex, F, verts.device)
        if tex.shape[-1] != self.images.shape[3]:
            raise ValueError(f"tex has {tex.shape[-1]} channels, the video {self.images.shape[3]}")
        image, face, depth = _RenderTexture.apply(tex, self.uv, verts, self.faces, self.intr, self.size, self.uv_faces,
                                                  self.uv_faces_device, self.background, self.z_near, self.cull_backfaces, True)
        if self.antialias:
            image = antialias(image, verts, self.faces, self.intr, render=(depth, face), z_near=self.z_near,
                              cull_backfaces=self.cull_backfaces)
        sq = (image.double() - self.images.double()).square().sum(dim=-1)
        if self.mask is not None:
            sq = torch.where(self.mask, sq, torch.zeros((), dtype=torch.float64, device=verts.device))
        n_cut = torch.zeros((), dtype=torch.long, device=verts.device)
        rho = sq
        if self.trunc is not None:
            n_cut = (sq.detach() > self.trunc * self.trunc).sum()
            rho = torch.clamp(sq, max=self.trunc * self.trunc)
        return {"cost": rho.sum(), "image": image, "depth": depth, "face": face, "sq": sq, "n_truncated": n_cut}

    def forward(self, verts: torch.Tensor, tex: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts, tex)["cost"]


def bake_texture(video: torch.Tensor, verts: torch.Tensor, faces, intr, uv: torch.Tensor, uv_faces, tex_size, weight=None,
                 z_near: float = 0.1, cull_backfaces: bool = False):
    """A texture from a sequence, the texture counterpart of fuse_vertex_colours: (tex [Ht, Wt, C] f32, hits [Ht, Wt] f32) with
    tex_size = (Ht, Wt).  video [F, H, W, C] or [F, H, W], uint8 or float32, C <= 3; weight f32 [F, H, W] (None: 1) a per-pixel
    confidence.  Every covered pixel SPLATS weight x (I, 1) into the four texels of its cell with its bilinear weights: ONE call of
    bodyfit_raster_texture_grad_device with the upstream gradient weight x [I, 1] (C + 1 channels), so the sums are exact integer
    sums and the result is bit-identical from run to run.  hits is the summed weight a texel received, tex = the summed colour /
    hits where hits > 0 and 0 elsewhere (a texel no pixel's cell touched stays empty: nothing is filled in).  No gradient."""
    img, _ = _check_images(video)
    _check_verts(verts)
    if len(intr) != 4 or len(tex_size) != 2:
        raise ValueError("intr is (fx, fy, cx, cy), tex_size is (height, width)")
    F, H, W, C = (int(n) for n in img.shape)
    if C > 3:
        raise ValueError("bake_texture takes at most 3 channels (the fourth carries the weight)")
    if verts.shape[0] != F or verts.device != img.device:
        raise ValueError(f"the video has {F} frames on {img.device}, verts has {verts.shape[0]} on {verts.device}")
    Ht, Wt = int(tex_size[0]), int(tex_size[1])
    f = _host_faces(faces)
    _, uvf_device = _check_atlas(uv, uv_faces, f.shape[0], verts.device)
    with torch.no_grad():
        raster, _, face, bary = _render(verts, f, intr, (H, W), z_near, cull_backfaces, True)
        v, vs, _, _ = _point_set("verts", verts.detach(), None)
        u = uv.detach().contiguous()
        G = torch.ones((F, H, W, C + 1), dtype=torch.float32, device=v.device)
        G[..., :C] = img.to(torch.float32)
        if weight is not None:
            if not isinstance(weight, torch.Tensor) or tuple(weight.shape) != (F, H, W) or weight.device != v.device:
                raise ValueError(f"weight must be a tensor [{F}, {H}, {W}] on the GPU of the video")
            G = G * weight.to(torch.float32).unsqueeze(-1)
        acc = torch.zeros((Ht, Wt, C + 1), dtype=torch.float32, device=v.device)
        work = torch.empty((Ht, Wt, C + 1), dtype=torch.int64, device=v.device)
        if F * H * W > 0:
            with torch.cuda.device(v.device):
                raster.texture_grad_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), u.shape[0],
                                           uvf_device.data_ptr(), None, 1, C + 1, Ht, Wt, 0, F, G.data_ptr(), None, acc.data_ptr(),
                                           work.data_ptr(), _stream())
        hits = acc[..., C]
        seen = hits > 0
        tex = torch.where(seen.unsqueeze(-1), acc[..., :C] / torch.where(seen, hits, torch.ones_like(hits)).unsqueeze(-1),
                          torch.zeros_like(acc[..., :C]))
        return tex, torch.where(seen, hits, torch.zeros_like(hits))


# ---- Gauss-Newton normal equations of the scan terms ----------------------------------------------------------------------------
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
