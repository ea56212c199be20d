"""What the modules of the layer share: the stream, point sets and gradients in their layout, the kept library handles (one
cache each, for the whole layer), the argument checks, and the helpers that more than one term is built from."""
from __future__ import annotations

import numpy as np
import torch

from .. import api


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


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
    """the f64 sum of rho(dist2) over the rows with a counterpart (a row without one: index -1, dist2 +inf, costs nothing).
    (Not _truncated_cost: the rows are masked by index first, the sum is widened from f32, and nothing is counted.)"""
    s = torch.where(index >= 0, dist2, torch.zeros_like(dist2))
    if trunc is not None:
        s = torch.clamp(s, max=trunc * trunc)
    return s.double().sum()


def _truncated_cost(sq: torch.Tensor, trunc: float | None):
    """(the sum of rho(sq), rho(s) = min(s, trunc^2), trunc None: rho(s) = s; the number of truncated entries, int64, which
    carries no gradient)"""
    if trunc is None:
        return sq.sum(), torch.zeros((), dtype=torch.long, device=sq.device)
    n_cut = (sq.detach() > trunc * trunc).sum()
    return torch.clamp(sq, max=trunc * trunc).sum(), n_cut


def _ragged_rows(mask_or_weights: torch.Tensor):
    """The nonzeros of a [F, n] mask (or weights) as a ragged set of rows: (frame int64 [N], column int32 [N], offset int32
    [F + 1], N), frame after frame and ascending inside a frame, the packed order of a ragged point set.  nonzero sizes its result
    on the host: the ONE host synchronisation of a caller (bincount's own read-back follows it on a drained stream; without a
    nonzero nothing is counted and the offset stays zero)."""
    F = mask_or_weights.shape[0]
    frame, col = torch.nonzero(mask_or_weights, as_tuple=True)
    N = int(col.shape[0])
    offset = torch.zeros(F + 1, dtype=torch.int32, device=mask_or_weights.device)
    if N > 0:
        offset[1:] = torch.bincount(frame, minlength=F).cumsum(0).to(torch.int32)
    return frame, col.to(torch.int32).contiguous(), offset, N


def _pixel_rows_vjp(surface, face: torch.Tensor, weight: torch.Tensor, direction: torch.Tensor, F: int, n_rows_out: int):
    """The pixels of a face image [F, H, W] as uniform rows of `surface` (an api.Surface over n_rows_out vertices), summed by
    bodyfit_surface_rows_vjp_device: out[f, corner a of face[f, p]] += weight[f, p, a] direction[p], f32 [F, n_rows_out, 3], with
    coef = 1 and direction [F H W, <= 3] padded with zeros to three."""
    dev, ppf = face.device, face.shape[1] * face.shape[2]
    N = F * ppf
    padded = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    padded[:, :direction.shape[1]] = direction
    coef = torch.ones(N, dtype=torch.float32, device=dev)
    rows = api.PointSet.uniform(face.data_ptr(), ppf, 3 * ppf)      # (the rows' frame structure; its xyz is never read)
    out = torch.empty((F, n_rows_out, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        surface.rows_vjp_device(rows, F, N, face.data_ptr(), weight.data_ptr(), coef.data_ptr(), padded.data_ptr(), out.data_ptr(),
                                3 * n_rows_out, _stream())
    return out


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


class _TermHandles:
    """For a term that keeps its own topology in self.faces: its api.Surface per (device, V), owned by the term and built on
    first use, so that an evaluation neither hashes the faces nor depends on what the layer's cache has evicted."""

    def _handle_for(self, verts: torch.Tensor):
        handles = self.__dict__.setdefault("_handles", {})
        key = (verts.device.index, verts.shape[-2])
        h = handles.get(key)
        if h is None:
            h = handles[key] = _surface_handle(key[0], key[1], self.faces)
        return h


_raster_handles: dict[tuple, tuple] = {}   # (device, V, n_faces, content hash, H, W) -> (the faces' bytes, api.Raster)


def _raster_handle(device_index: int, n_verts: int, faces, size):
    """The api.Raster of (device, topology, image size), kept like _surface_handle's: keyed on the faces' content, the last
    _SURFACE_CACHE in use."""
    H, W = int(size[0]), int(size[1])
    return _topology_handle(_raster_handles, device_index, n_verts, faces, (H, W),
                            lambda f: api.Raster(device_index, n_verts, f, W, H))


_volume_handles: dict[tuple, object] = {}   # (device, (nx, ny, nz), origin, spacing) -> api.Volume; the last _SURFACE_CACHE in use


def _volume_handle(device_index: int, dims, origin, spacing):
    """The api.Volume of (device, geometry): dims = (nx, ny, nz), origin and spacing three floats each.  The handle owns nothing
    on the device; it is kept so that an evaluation does not create one."""
    key = (device_index, tuple(int(n) for n in dims), tuple(float(a) for a in origin), tuple(float(a) for a in spacing))
    h = _volume_handles.pop(key, None)
    if h is None:
        h = api.Volume(device_index, key[1], key[2], key[3])
    _volume_handles[key] = h                        # (most recently used last)
    while len(_volume_handles) > _SURFACE_CACHE:
        _volume_handles.pop(next(iter(_volume_handles)))
    return h


_NO_FACES = np.zeros((0, 3), np.int32)


def _check_intr_size(intr, size):
    if len(intr) != 4 or len(size) != 2:
        raise ValueError("intr is (fx, fy, cx, cy), size is (height, width)")


def _check_background(background, C: int) -> np.ndarray:
    """a render's background as a float32 array of 1 or C values"""
    bg = np.atleast_1d(np.asarray(background, np.float32))
    if bg.ndim != 1 or bg.shape[0] not in (1, C):
        raise ValueError(f"background must be a float or {C} floats")
    return bg


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
