"""Lighting: second-order spherical-harmonic shading of a render, its gradients, and differentiable vertex normals.

    n = lighting.vertex_normals(verts, faces)                            # solid.vertex_normals' bits, WITH a gradient to verts
    image = lighting.shade(albedo, verts, faces, intr, light)            # albedo x sum_k light[k] b_k(normal), per pixel
    term = lighting.LitPhotometricTerm(video, intr, faces, trunc=30.0)   # sum rho(|antialias(shade(render)) - I|^2)

A video of a person is albedo x shading; the photometric terms of appearance and texture compare the albedo itself with the
video and so bake the shadows into the colours.  shade is bodyfit_raster_light_device (k_light.hip: the per-vertex normals
interpolated with the shade's perspective-correct weights, normalised, the nine polynomials of Ramamoorthi and Hanrahan's
irradiance, one [9, C] light per frame or for all); its backward is bodyfit_raster_light_grad_device (albedo, the light reduced in
f64 in a fixed order, and the gradient in the interpolated normal), the rows VJP into the vertex normals, and
bodyfit_surface_vertex_normals_vjp_device from there into the vertices.  The names live in this module (the package re-exports
only the names its recorded surface holds).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import (_check_per_vertex, _check_verts, _grad_like, _pixel_rows_vjp, _point_set, _raster_handle, _stream,
                      _surface_handle)
from .appearance import _PixelPhotometricTerm, _RenderAttributes, _check_frames, _interior_rows
from .depth import _render
from .solid import _posed_mesh
from .texture import _RenderTexture, _check_atlas, _check_mip, _check_texture


class _VertexNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces):
        v, vs, F, handle = _posed_mesh(verts, faces)
        n = torch.empty((F, v.shape[1], 3), dtype=torch.float32, device=v.device)
        if n.numel() > 0:
            with torch.cuda.device(v.device):
                handle.vertex_normals_device(v.data_ptr(), vs.frame_stride, F, n.data_ptr(), _stream())
        ctx.look = (vs, F, handle)
        ctx.save_for_backward(v)
        return n

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        vs, F, handle = ctx.look
        gv = _grad_like(v, vs)
        if g is None or gv.numel() == 0:
            gv.zero_()
            return gv, None
        gn = g.to(torch.float32).contiguous()
        V = v.shape[1]
        with torch.cuda.device(v.device):
            handle.vertex_normals_vjp_device(v.data_ptr(), vs.frame_stride, F, gn.data_ptr(), gv.data_ptr(),
                                             gv.stride(0) if F > 1 else 3 * V, _stream())
        return gv, None


def vertex_normals(verts: torch.Tensor, faces) -> torch.Tensor:
    """solid.vertex_normals(verts, faces) bit for bit (the same entry, bodyfit_surface_vertex_normals_device: the area-weighted
    unit normals n [F, V, 3] f32, 0 for a vertex without a face, with a zero sum or a non-finite corner), and DIFFERENTIABLE in
    verts: the backward is bodyfit_surface_vertex_normals_vjp_device, the exact adjoint at the f32 vertices, h_i = (g_i - n_i (n_i .
    g_i)) / |s_i| gathered over the faces of every vertex in f64 in a fixed order: no atomics, no index_add_, bit-identical from run
    to run.  A vertex whose normal is 0 passes no gradient.  The definition and the error bound: include/bodyfit.h."""
    return _VertexNormals.apply(verts, faces)


def sh_basis(n: torch.Tensor) -> torch.Tensor:
    """The nine polynomials b(n) = (1, x, y, z, xy, xz, yz, x^2 - y^2, 3 z^2 - 1) of unit vectors n [..., 3], as [..., 9] in n's
    dtype, plain torch (differentiable): the UNNORMALISED basis of shade, s = sum_k light[k] b_k(n).  A light from real-SH
    coefficients L_lm (Ramamoorthi and Hanrahan 2001): light = (c4 L_00, 2 c2 L_11, 2 c2 L_1-1, 2 c2 L_10, 2 c1 L_2-2, 2 c1 L_21,
    2 c1 L_2-1, c1 L_22, c5 L_20) with c1 = 0.429043, c2 = 0.511664, c4 = 0.886227, c5 = 0.247708."""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return torch.stack((torch.ones_like(x), x, y, z, x * y, x * z, y * z, x * x - y * y, 3.0 * (z * z) - 1.0), dim=-1)


def _check_light(light, F: int, C: int, device):
    """(the light f32 contiguous, its frame stride: 0 when shared)"""
    if not isinstance(light, torch.Tensor) or light.dtype != torch.float32 or not light.is_cuda:
        raise TypeError("light must be a float32 tensor on the GPU")
    if light.ndim not in (2, 3) or tuple(light.shape[-2:]) != (9, C) or (light.ndim == 3 and light.shape[0] != F):
        raise ValueError(f"light must be [9, C] or [F, 9, C] with F = {F} and C = {C}, got {tuple(light.shape)}")
    if light.device != device:
        raise ValueError("light and verts must be on the same GPU")
    return 0 if light.ndim == 2 else 9 * C


class _Shade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, albedo, light, normals, verts, faces, intr, raster, face, bary, interior, want_shading):
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        n, ns, _, _ = _point_set("normals", normals.detach(), None)
        a, lt = albedo.detach().contiguous(), light.detach().contiguous()
        _, H, W, C = a.shape
        light_stride = 0 if lt.ndim == 2 else 9 * C
        image = torch.empty((F, H, W, C), dtype=torch.float32, device=v.device)
        shading = torch.empty((F, H, W, C), dtype=torch.float32, device=v.device) if want_shading else None
        if image.numel() > 0:
            with torch.cuda.device(v.device):
                raster.light_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, n.data_ptr(), ns.frame_stride,
                                    a.data_ptr(), C, lt.data_ptr(), light_stride, F, image.data_ptr(), None,
                                    shading.data_ptr() if want_shading else None, _stream())
        ctx.interior = bool(interior) and ctx.needs_input_grad[3]
        if any(ctx.needs_input_grad[:3]) or ctx.interior:
            ctx.look = (raster, vs, ns, tuple(float(x) for x in intr), faces, light_stride)
            ctx.save_for_backward(face, bary, v, n, a, lt)
        if want_shading:
            ctx.mark_non_differentiable(shading)
        return image, shading

    @staticmethod
    @once_differentiable
    def backward(ctx, g_image, _g_shading):
        if not hasattr(ctx, "look"):
            return (None,) * 11
        face, bary, v, n, a, lt = ctx.saved_tensors
        raster, vs, ns, intr, faces, light_stride = ctx.look
        dev = face.device
        F, H, W, C = a.shape
        V = v.shape[1]
        want_a, want_l, want_n = ctx.needs_input_grad[:3]
        want_m = want_n or ctx.interior
        live = g_image is not None and F * H * W > 0
        g_a = torch.zeros((F, H, W, C), dtype=torch.float32, device=dev) if want_a else None
        g_lf = torch.zeros((F, 9, C), dtype=torch.float32, device=dev) if want_l else None
        g_m = torch.zeros((F, H, W, 3), dtype=torch.float32, device=dev) if want_m else None
        if live:
            gi = g_image.to(torch.float32).contiguous()
            work = torch.empty(api.light_grad_layout(H * W, C, F)[2], dtype=torch.float64, device=dev) if want_l else None
            with torch.cuda.device(dev):
                raster.light_grad_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, n.data_ptr(),
                                         ns.frame_stride, a.data_ptr(), C, lt.data_ptr(), light_stride, F, gi.data_ptr(),
                                         g_a.data_ptr() if want_a else None, g_m.data_ptr() if want_m else None,
                                         g_lf.data_ptr() if want_l else None, work.data_ptr() if want_l else None, _stream())
        g_l = None
        if want_l:
            g_l = g_lf if light_stride else g_lf.double().sum(dim=0).to(torch.float32)
        g_n = g_v = None
        if want_m:
            surface = _surface_handle(dev.index, V, faces)
            weight = torch.zeros((F, H, W, 3), dtype=torch.float32, device=dev)
            if live and V > 0:
                # the shade's stored weights of this face image: one k_rs_shade pass over the normals (its image is not used)
                unused = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
                with torch.cuda.device(dev):
                    raster.shade_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, n.data_ptr(), ns.frame_stride,
                                        3, F, 0.0, unused.data_ptr(), weight.data_ptr(), _stream())
            if want_n:
                g_n = torch.zeros((F, V, 3), dtype=torch.float32, device=dev)
                if live and V > 0:
                    g_n = _pixel_rows_vjp(surface, face, weight, g_m.reshape(F * H * W, 3), F, V)
            if ctx.interior:
                g_v = _interior_rows(raster, surface, v, vs, intr, face, weight, n, ns.frame_stride, 3, g_m if live else None)
        return (g_a, g_l, g_n, g_v) + (None,) * 7


def _shade(albedo, verts, faces, intr, light, normals, render, z_near, cull_backfaces, interior, want_shading=False):
    _check_verts(verts)
    if len(intr) != 4:
        raise ValueError("intr is (fx, fy, cx, cy)")
    if not isinstance(albedo, torch.Tensor) or albedo.dtype != torch.float32 or not albedo.is_cuda:
        raise TypeError("albedo must be a float32 tensor on the GPU")
    F, V = verts.shape[0], verts.shape[1]
    if albedo.ndim != 4 or albedo.shape[0] != F or not 1 <= albedo.shape[3] <= 4 or albedo.shape[1] < 1 or albedo.shape[2] < 1:
        raise ValueError(f"albedo must be [F, H, W, C] with F = {F} and C in 1 .. 4, got {tuple(albedo.shape)}")
    if albedo.device != verts.device:
        raise ValueError("albedo and verts must be on the same GPU")
    if not z_near > 0.0:
        raise ValueError("z_near must be positive")
    H, W, C = (int(x) for x in albedo.shape[1:])
    _check_light(light, F, C, verts.device)
    if normals is None:
        normals = vertex_normals(verts, faces)
    else:
        if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or not normals.is_cuda:
            raise TypeError("normals must be a float32 tensor on the GPU")
        if tuple(normals.shape) != (F, V, 3):
            raise ValueError(f"normals must be [F, V, 3] = {(F, V, 3)}, got {tuple(normals.shape)}")
        if normals.device != verts.device:
            raise ValueError("normals and verts must be on the same GPU")
    if render is None:
        raster, _, face, bary = _render(verts, faces, intr, (H, W), z_near, cull_backfaces, True)
    else:
        if len(render) != 3:
            raise ValueError("render is (depth, face, bary), as render_depth returns them")
        face, bary = render[1], render[2]
        for t, dt, shape, name in ((face, torch.int32, (F, H, W), "face"), (bary, torch.float32, (F, H, W, 3), "bary")):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != verts.device or tuple(t.shape) != shape:
                raise ValueError(f"render's {name} must be a {dt} tensor {list(shape)} on the GPU of verts")
        raster = _raster_handle(verts.device.index, V, faces, (H, W))
        face, bary = face.contiguous(), bary.detach().contiguous()
    return _Shade.apply(albedo, light, normals, verts, faces, tuple(float(x) for x in intr), raster, face, bary, bool(interior),
                        bool(want_shading))


def shade(albedo: torch.Tensor, verts: torch.Tensor, faces, intr, light: torch.Tensor, normals: torch.Tensor | None = None,
          render=None, z_near: float = 0.1, cull_backfaces: bool = False, interior: bool = False) -> torch.Tensor:
    """The image albedo ([F, H, W, C] f32 on the GPU, C in 1 .. 4: what render_attributes, render_texture or render_texture_mip
    made of the posed meshes verts [F, V, 3] f32 through the camera intr) LIT: image [F, H, W, C] f32 with, in every lit pixel,
      image_c = albedo_c s_c,   s_c = sum_k light[k, c] b_k(n),   b = sh_basis,   n = normalise(sum_a w_a normals[corner a]),
    w_a the shade's perspective-correct weights of the pixel in its face.  light: [9, C] (one light for all frames) or [F, 9, C],
    f32.  normals: None: vertex_normals(verts, faces) (this module's, differentiable); or a tensor [F, V, 3] f32, used as given.
    render: what render_depth(verts, faces, intr, (H, W), z_near, cull_backfaces) returned, (depth, face, bary), reused; None:
    rendered here (one 8-byte read-back), as antialias does.  A pixel is UNLIT, and keeps its albedo bit for bit (the background
    passes through), where the render is empty or void, where a corner normal is not finite, and where the three corner normals
    cancel.  There is no clamp on s.  bodyfit_raster_light_device; the definition and its error bound: include/bodyfit.h.

    Differentiable at the FIXED face image and the fixed pixel rays in
      albedo and light, straight from bodyfit_raster_light_grad_device: G_c s_c (G_c on an unlit pixel), and per frame sum over
          the lit pixels of G_c albedo_c b_k(n), reduced in f64 in a fixed order without atomics: bit-identical from run to run,
          and a frame's numbers do not depend on the batch around it; a shared light gets the frames summed in f64;
      normals, by the rows VJP with the pixels as rows (index = the face image, bary = the shade's stored weights, direction =
          the gradient in the unnormalised interpolated normal, (g_n - n (n . g_n)) / |m|).  Through vertex_normals this reaches
          verts: the shading gradient that turns the body under the light;
      verts, with interior=True ONLY, ALSO through the weights: how a pixel's normal changes as its face's corners move under
          it, the rows of bodyfit_raster_interp_rows_device with attr = the normals, three channels and that upstream gradient,
          summed by one bodyfit_surface_rows_vjp_device call (one host synchronisation lists the shaded pixels).
    NOT part of it: visibility and coverage (antialias(image, verts, ...) adds the gradient through coverage), z_near and
    culling.  The backward takes the shade's weights from one bodyfit_raster_shade_device pass over the normals."""
    return _shade(albedo, verts, faces, intr, light, normals, render, z_near, cull_backfaces, interior)[0]


class LitPhotometricTerm(_PixelPhotometricTerm):
    """RenderedPhotometricTerm / TexturedPhotometricTerm UNDER A LIGHT: antialias(shade(A, light)) against the video, A the
    rendered albedo.

    video: [F, H, W, C] or [F, H, W], uint8 (raw 0 .. 255) or float32, on the GPU; intr = (fx, fy, cx, cy).  Without an atlas
    term(verts, albedo, light) takes albedo [V, C] or [F, V, C] f32, vertex colours, and A = render_attributes(verts, albedo,
    interior=True); with uv [T, 2] f32 (GPU) and uv_faces int32 [n_faces, 3] given to the constructor, albedo is a texture [Ht, Wt,
    C] or [F, Ht, Wt, C] f32 and A = render_texture(..., interior=True) (term.mipmaps(...): render_texture_mip, as on
    TexturedPhotometricTerm).  light: [9, C] or [F, 9, C] f32.  The f64 cost is
      sum over the pixels p of mask of rho(sum_c (R_c(p) - I_c(p))^2),    rho(s) = min(s, trunc^2) (trunc None: rho(s) = s),
    R = antialias(shade(A, verts, light, interior=True)).  Differentiable in albedo, in light and in verts: through the albedo's
    interpolation, through the shading (the normals of vertex_normals and their interpolation) and, with antialias, through
    coverage.  The albedo render and shade each render ONCE: two renders per evaluation (the second is a few milliseconds at
    256 frames, against a backward of hundreds); the render entries stay as they are.  No normal equations are built for it.
    evaluate(verts, albedo, light) returns the cost with its parts."""

    _VIDEO_NAME, _VIDEO_FRAMES = "the video", "the video has"

    def __init__(self, video: torch.Tensor, intr, faces, uv: torch.Tensor | None = None, uv_faces=None, trunc: float | None = None,
                 background=0.0, mask: torch.Tensor | None = None, antialias: bool = True, z_near: float = 0.1,
                 cull_backfaces: bool = False):
        super().__init__(video, intr, faces, trunc, background, mask, antialias, z_near, cull_backfaces)
        self.mip = None
        if (uv is None) != (uv_faces is None):
            raise ValueError("uv and uv_faces come together")
        self.textured = uv is not None
        if self.textured:
            self.uv_faces, uvf_device = _check_atlas(uv, uv_faces, self.faces.shape[0], self.images.device)
            self.register_buffer("uv", uv.detach().contiguous())
            self.register_buffer("uv_faces_device", uvf_device)

    def mipmaps(self, enable: bool = True, max_mip_level: int | None = None, lod_bias: float = 0.0):
        """Render a textured albedo through the texture's pyramid from now on (TexturedPhotometricTerm.mipmaps).  Returns the
        term."""
        if not self.textured:
            raise ValueError("mipmaps need the atlas (uv, uv_faces) in the constructor")
        self.mip = _check_mip(max_mip_level, lod_bias) if enable else None
        return self

    def evaluate(self, verts: torch.Tensor, albedo: torch.Tensor, light: torch.Tensor) -> dict:
        """term(verts, albedo, light) with what it was built from: cost (f64, with the gradient), image f32 [F, H, W, C] (what
        was compared with the video: antialiased or not), the render (depth, face), sq f64 [F, H, W], n_truncated and shading
        f32 [F, H, W, C] (s of shade: 0 on an unlit pixel; no gradient)"""
        _check_verts(verts)
        _check_frames(self.images, verts, self._VIDEO_FRAMES)
        C = int(self.images.shape[3])
        if self.textured:
            _check_texture(albedo, verts.shape[0], verts.device)
        else:
            _check_per_vertex(albedo, "albedo", verts.shape[0], verts.shape[1], verts.device)
        if albedo.shape[-1] != C:
            raise ValueError(f"albedo has {albedo.shape[-1]} channels, the video {C}")
        _check_light(light, verts.shape[0], C, verts.device)
        if self.textured:
            A, face, depth = _RenderTexture.apply(albedo, self.uv, verts, self.faces, self.intr, self.size, self.uv_faces,
                                                  self.uv_faces_device, self.background, self.z_near, self.cull_backfaces, True,
                                                  self.mip)
        else:
            A, face, depth = _RenderAttributes.apply(albedo, verts, self.faces, self.intr, self.size, self.background, self.z_near,
                                                     self.cull_backfaces, True)
        image, shading = _shade(A, verts, self.faces, self.intr, light, None, None, self.z_near, self.cull_backfaces, True,
                                want_shading=True)
        out = self._against_video(verts, image, face, depth)
        out["shading"] = shading
        return out

    def forward(self, verts: torch.Tensor, albedo: torch.Tensor, light: torch.Tensor) -> torch.Tensor:
        return self.evaluate(verts, albedo, light)["cost"]
