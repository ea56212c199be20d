"""UV textures: the texture lookup over a render, its gradients in the texels, in uv and in the vertices.

    image, face = render_texture(verts, faces, intr, (H, W), uv, uv_faces, tex, interior=True)
    term = TexturedPhotometricTerm(video, intr, faces, uv, uv_faces, trunc=30.0)     # sum rho(|antialias(render) - I|^2)
    tex, hits = bake_texture(video, verts, faces, intr, uv, uv_faces, (Ht, Wt))      # a texture from a sequence

render_texture is render_depth followed by bodyfit_raster_texture_device (k_texture.hip: the face's three uv rows with the shade's
perspective-correct weights, then a bilinear texel lookup); its backward is bodyfit_raster_texture_grad_device (the exact adjoint
in the texels, summed in 64-bit integers), the rows VJP on the atlas's own surface handle for uv, and for the vertices the rows of
bodyfit_raster_interp_rows_indexed_device.  TexturedPhotometricTerm is appearance.RenderedPhotometricTerm with a texture in place
of the vertex colours; bake_texture is the texture counterpart of fuse_vertex_colours.

    image, face = render_texture_mip(verts, faces, intr, (H, W), uv, uv_faces, tex, interior=True, lod_bias=0.0)
    term = TexturedPhotometricTerm(video, intr, faces, uv, uv_faces).mipmaps()

are the same with MIPMAPS: the texture's pyramid (bodyfit_raster_texture_mip_build_device), then
bodyfit_raster_texture_mip_device and bodyfit_raster_texture_mip_grad_device: a trilinear lookup at each pixel's level of detail,
differentiated at that fixed level.  render_texture_mip is reached through this module (the package re-exports the names its
recorded surface holds; render_texture and the term's constructor keep their signatures).  bake_texture stays level 0.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import (_check_background, _check_intr_size, _check_verts, _host_faces, _pixel_rows_vjp, _point_set, _stream,
                      _surface_handle)
from .appearance import _PixelPhotometricTerm, _check_frames, _check_images, _interior_rows
from .depth import _render


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


def _check_mip(max_mip_level, lod_bias):
    """(max_level for the ABI: -1 = as many as exist, lod_bias)"""
    if max_mip_level is not None and int(max_mip_level) < 0:
        raise ValueError("max_mip_level is None or >= 0")
    if lod_bias != lod_bias:
        raise ValueError("lod_bias is NaN")
    return (-1 if max_mip_level is None else int(max_mip_level), float(lod_bias))


class _RenderTexture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, verts, faces, intr, size, uv_faces, uv_faces_device, background, z_near, cull_backfaces, interior,
                mip=None):
        raster, depth, face, bary = _render(verts, faces, intr, size, z_near, cull_backfaces, True)
        v, vs, F, _ = _point_set("verts", verts.detach(), None)
        H, W = int(size[0]), int(size[1])
        kind, shared = _check_texture(tex, F, v.device)
        t, u = tex.detach().contiguous(), uv.detach().contiguous()
        Ht, Wt, C = (int(n) for n in t.shape[-3:])
        image = torch.empty((F, H, W, C), dtype=torch.float32, device=v.device)
        weight = torch.empty((F, H, W, 3), dtype=torch.float32, device=v.device)
        look = (u.shape[0], kind, C, Ht, Wt, 0 if shared else Ht * Wt * C, F)
        pyramid = None          # mip: (max_level, lod_bias, the pyramid f32 [1 or F, total C], its stride), built once per call
        if mip is not None:
            total = api.texture_mip_layout(Ht, Wt, mip[0])[3]
            pyramid = torch.empty((1 if shared else F, total * C), dtype=torch.float32, device=v.device)
            mip = (mip[0], mip[1], pyramid, pyramid.shape[1])
        if F > 0 and mip is None:
            with torch.cuda.device(v.device):
                raster.texture_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), look[0],
                                      uv_faces_device.data_ptr(), t.data_ptr(), kind, C, Ht, Wt, look[5], F, background,
                                      image.data_ptr(), weight.data_ptr(), None, _stream())
        elif F > 0:
            with torch.cuda.device(v.device):
                raster.texture_mip_build_device(t.data_ptr(), kind, C, Ht, Wt, look[5], pyramid.shape[0], mip[0], pyramid.data_ptr(),
                                                mip[3], _stream())
                raster.texture_mip_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), look[0],
                                          uv_faces_device.data_ptr(), t.data_ptr(), kind, C, Ht, Wt, look[5], F, intr,
                                          pyramid.data_ptr(), mip[3], mip[0], mip[1], background, image.data_ptr(),
                                          weight.data_ptr(), None, None, _stream())
        want_tex = ctx.needs_input_grad[0] and kind == 1
        ctx.interior = bool(interior) and ctx.needs_input_grad[2]
        if want_tex or ctx.needs_input_grad[1] or ctx.interior:
            ctx.look = (raster, vs, tuple(float(x) for x in intr), look, uv_faces, want_tex, faces, mip)
            ctx.save_for_backward(face, bary, weight, v, u, t, uv_faces_device)
        ctx.mark_non_differentiable(face, depth)
        return image, face, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g_image, _g_face, _g_depth):
        if not hasattr(ctx, "look"):
            return (None,) * 13
        face, bary, weight, v, u, t, uv_faces_device = ctx.saved_tensors
        raster, vs, intr, (T, kind, C, Ht, Wt, tex_stride, F), uv_faces, want_tex, faces, mip = ctx.look
        dev, (H, W) = face.device, face.shape[1:]
        want_uv = ctx.needs_input_grad[1] or ctx.interior
        g_tex = torch.zeros(t.shape, dtype=torch.float32, device=dev) if want_tex else None
        g_uvpix = torch.zeros((F, H, W, 2), dtype=torch.float32, device=dev) if want_uv else None
        if g_image is not None and F * H * W > 0:
            gi = g_image.to(torch.float32).contiguous()
            outs = (g_uvpix.data_ptr() if want_uv else None, g_tex.data_ptr() if want_tex else None)
            if mip is None:
                work = torch.empty(t.shape, dtype=torch.int64, device=dev) if want_tex else None
                with torch.cuda.device(dev):
                    raster.texture_grad_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), T,
                                               uv_faces_device.data_ptr(), t.data_ptr(), kind, C, Ht, Wt, tex_stride, F,
                                               gi.data_ptr(), *outs, work.data_ptr() if want_tex else None, _stream())
            else:
                max_level, lod_bias, pyramid, mip_stride = mip
                # the int64 pyramid, level 0 first: Ht Wt C + the packed levels, per texture
                work = (torch.empty((pyramid.shape[0], Ht * Wt * C + mip_stride), dtype=torch.int64, device=dev) if want_tex
                        else None)
                with torch.cuda.device(dev):
                    raster.texture_mip_grad_device(face.data_ptr(), bary.data_ptr(), v.data_ptr(), vs.frame_stride, u.data_ptr(), T,
                                                   uv_faces_device.data_ptr(), t.data_ptr(), kind, C, Ht, Wt, tex_stride, F, intr,
                                                   pyramid.data_ptr(), mip_stride, max_level, lod_bias, gi.data_ptr(), *outs,
                                                   work.data_ptr() if want_tex else None, _stream())
        g_uv = None
        if ctx.needs_input_grad[1]:
            # the pixels as rows of the ATLAS's own surface handle (T rows, uv_faces): g_uv[uv_faces[t][a]] += w_a (g_u, g_v, 0)
            g_uv = torch.zeros((T, 2), dtype=torch.float32, device=dev)
            N = F * H * W
            if g_image is not None and N * T > 0:
                atlas = _surface_handle(dev.index, T, uv_faces)
                gt = _pixel_rows_vjp(atlas, face, weight, g_uvpix.reshape(N, 2), F, T)
                g_uv = gt[:, :, :2].double().sum(dim=0).to(torch.float32)
        g_verts = None
        if ctx.interior:
            surface = _surface_handle(dev.index, v.shape[1], faces)
            g_verts = _interior_rows(raster, surface, v, vs, intr, face, weight, u, 0, 2, g_uvpix if g_image is not None else None,
                                     attr_faces=uv_faces_device, n_attr_rows=T)
        return (g_tex, g_uv, g_verts) + (None,) * 10


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
    culling.  This lookup has NO minification filter: a body smaller on the screen than its atlas ALIASES, and the texels no
    pixel's cell touches get no gradient; render_texture_mip (this module) is the lookup with mipmaps."""
    return _render_texture(verts, faces, intr, size, uv, uv_faces, tex, background, z_near, cull_backfaces, interior, None)


def _render_texture(verts, faces, intr, size, uv, uv_faces, tex, background, z_near, cull_backfaces, interior, mip):
    _check_verts(verts)
    _check_intr_size(intr, size)
    n_faces = _host_faces(faces).shape[0]
    uvf, uvf_device = _check_atlas(uv, uv_faces, n_faces, verts.device)
    _check_texture(tex, verts.shape[0], verts.device)
    bg = _check_background(background, tex.shape[-1])
    image, face, _ = _RenderTexture.apply(tex, uv, verts, faces, intr, size, uvf, uvf_device, bg, float(z_near), bool(cull_backfaces),
                                          bool(interior), mip)
    return image, face


def render_texture_mip(verts: torch.Tensor, faces, intr, size, uv: torch.Tensor, uv_faces, tex: torch.Tensor, background=0.0,
                       z_near: float = 0.1, cull_backfaces: bool = False, interior: bool = False,
                       max_mip_level: int | None = None, lod_bias: float = 0.0):
    """render_texture with MIPMAPS: the same arguments, the same outputs and the same three gradients, through the texture's
    pyramid.  (A function of its own in this module, torch_layer.texture.render_texture_mip: render_texture keeps the signature
    the package's recorded surface holds, and is the plain lookup bit for bit.)

    The pyramid is built once per call (bodyfit_raster_texture_mip_build_device: levels by exact halving while the sizes stay
    even, at most max_mip_level above level 0; None: as many as exist) and looked up trilinearly
    (bodyfit_raster_texture_mip_device) at the level of detail of each pixel's footprint, L = log2(rho) + lod_bias clamped to the
    pyramid, rho the larger singular value of the face's screen-to-texel map at the pixel.  The gradients
    (bodyfit_raster_texture_mip_grad_device) are taken at the FIXED face image, pixel rays AND LEVEL OF DETAIL: tex (float32 only)
    gets every texel under a pixel's footprint, in the level-0 layout, the exact adjoint of "average without rounding, then filter",
    summed in 64-bit integers and bit-identical from run to run and under any permutation of the frames; uv and (interior=True)
    verts go through render_texture's rows with the blended pixel gradients.  Where L = 0 (a one-level texture, lod_bias = -inf)
    everything equals render_texture's bit for bit.
    NOT built: the gradient through the level of detail, anisotropic filtering, wrap and mirror addressing, caller-supplied
    pyramids, a mip-aware bake_texture."""
    return _render_texture(verts, faces, intr, size, uv, uv_faces, tex, background, z_near, cull_backfaces, interior,
                           _check_mip(max_mip_level, lod_bias))


class TexturedPhotometricTerm(_PixelPhotometricTerm):
    """RenderedPhotometricTerm with a uv texture in place of the vertex colours: antialias(render_texture(verts, tex,
    interior=True)) against the video.

    video: [F, H, W, C] or [F, H, W], uint8 (raw 0 .. 255) or float32, on the GPU; intr = (fx, fy, cx, cy); the atlas uv [T, 2] f32
    (GPU) and uv_faces int32 [n_faces, 3].  term(verts, tex), verts [F, V, 3] f32 and tex [Ht, Wt, C] or [F, Ht, Wt, C] f32 in
    the video's units, returns the f64 cost
      sum over the pixels p of mask of rho(sum_c (R_c(p) - I_c(p))^2),    rho(s) = min(s, trunc^2) (trunc None: rho(s) = s).
    Differentiable in tex (every covered pixel writes into the four texels of its cell) and in verts: through the uv
    interpolation inside the faces and, with antialias, through coverage at the silhouettes.  One render per evaluation.  No
    normal equations are built for it.  evaluate(verts, tex) returns the cost with its parts.  term.mipmaps(...) switches the
    render to render_texture_mip's: a body smaller on the screen than its atlas is then minified through the texture's pyramid,
    and every texel under a pixel's footprint gets a gradient."""

    _VIDEO_NAME, _VIDEO_FRAMES = "the video", "the video has"

    def __init__(self, video: torch.Tensor, intr, faces, uv: torch.Tensor, uv_faces, trunc: float | None = None, background=0.0,
                 mask: torch.Tensor | None = None, antialias: bool = True, z_near: float = 0.1, cull_backfaces: bool = False):
        super().__init__(video, intr, faces, trunc, background, mask, antialias, z_near, cull_backfaces)
        self.mip = None
        self.uv_faces, uvf_device = _check_atlas(uv, uv_faces, self.faces.shape[0], self.images.device)
        self.register_buffer("uv", uv.detach().contiguous())
        self.register_buffer("uv_faces_device", uvf_device)

    def mipmaps(self, enable: bool = True, max_mip_level: int | None = None, lod_bias: float = 0.0):
        """Render through the texture's pyramid from now on (render_texture_mip's max_mip_level and lod_bias), or with
        enable=False through the plain lookup again, which is what a new term does.  Returns the term:
        term = TexturedPhotometricTerm(...).mipmaps()."""
        self.mip = _check_mip(max_mip_level, lod_bias) if enable else None
        return self

    def evaluate(self, verts: torch.Tensor, tex: torch.Tensor) -> dict:
        """term(verts, tex) with what it was built from: cost (f64, with the gradient), image f32 [F, H, W, C] (what was compared
        with the video: antialiased or not), the render (depth, face), sq f64 [F, H, W] and n_truncated"""
        _check_verts(verts)
        _check_frames(self.images, verts, self._VIDEO_FRAMES)
        _check_texture(tex, verts.shape[0], verts.device)
        if tex.shape[-1] != self.images.shape[3]:
            raise ValueError(f"tex has {tex.shape[-1]} channels, the video {self.images.shape[3]}")
        image, face, depth = _RenderTexture.apply(tex, self.uv, verts, self.faces, self.intr, self.size, self.uv_faces,
                                                  self.uv_faces_device, self.background, self.z_near, self.cull_backfaces, True,
                                                  self.mip)
        return self._against_video(verts, image, face, depth)

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
