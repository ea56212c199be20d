"""PyTorch autograd layers over the library's SMPL forward, fitting objective and data terms, with their reverse-mode gradients.
Everything runs on torch.cuda.current_stream(); every gradient is deterministic (no float atomics).  Each module's docstring
describes what it holds:

    smpl         SMPLLayer (forward, VJP, JVP, Jacobian, per-vertex offsets), FitObjective, huber_rho
    scan         closest_points / PointCloudTerm, closest_surface / SurfaceTerm, surface_gram and the terms' normal_equations
    solid        winding_number, vertex_winding, vertex_normals, signed_distance, SelfPenetrationTerm, mesh_laplacian,
                 OffsetRegulariser
    depth        render_depth, visible_vertices, DepthMapTerm, depth_at_pixels, DepthResidualTerm
    silhouette   distance_transform, SilhouetteTerm, edge_weights, antialias, CoverageTerm
    appearance   render_attributes, sample_images, fuse_vertex_colours, PhotometricTerm, RenderedPhotometricTerm
    texture      render_texture, TexturedPhotometricTerm, bake_texture; with mipmaps (a trilinear lookup at the pixel's level of
                 detail and its gradients): texture.render_texture_mip and TexturedPhotometricTerm.mipmaps()
    lighting     lighting.vertex_normals (differentiable), sh_basis, shade, LitPhotometricTerm (names reached through the module)
    volume       volume.sample_volume, voxelize_sdf, grid_points, VolumeTerm: signed-distance volumes (names reached through the module)
    _common      what they share: point sets, the kept handles (one cache each), the argument checks, the row helpers

Every public name of the recorded surface (tests/golden/torch_layer_surface.json) is importable from here, and so are the private
ones the tests and tools reach; texture.render_texture_mip, added after that record, is imported from its module.
"""
import torch  # noqa: F401  (callers reach torch through the layer)

from ._common import _raster_handle, _surface_handle  # noqa: F401
from .appearance import (PhotometricTerm, RenderedPhotometricTerm, fuse_vertex_colours, render_attributes,  # noqa: F401
                         sample_images)
from .depth import DepthMapTerm, DepthResidualTerm, _render, depth_at_pixels, render_depth, visible_vertices  # noqa: F401
from .scan import PointCloudTerm, SurfaceTerm, closest_points, closest_surface, surface_gram  # noqa: F401
from .silhouette import CoverageTerm, SilhouetteTerm, antialias, distance_transform, edge_weights  # noqa: F401
from .smpl import FitObjective, SMPLLayer, huber_rho  # noqa: F401
from .solid import (OffsetRegulariser, SelfPenetrationTerm, _SignedRoot, mesh_laplacian, signed_distance,  # noqa: F401
                    vertex_normals, vertex_winding, winding_number)
from .texture import TexturedPhotometricTerm, bake_texture, render_texture  # noqa: F401
