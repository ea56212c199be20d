"""The statuses and messages of the entries that take a bodyfit_raster (k_raster*.hip, k_texture.hip, k_light.hip, k_edt.hip),
as one table: (entry, the arguments that differ from the entry's valid call, expected status, expected message).  The messages
are the library's own words, written out; bodyfit_last_error() is "<entry>: <message>".

The handle of the table: 4 vertices, 2 faces, an 8 x 8 image; a valid call has 2 frames.  ARGS gives every entry's valid call in
the order of its C signature.  Pointers are the tokens IN / OUT / OUT2, which the GPU test replaces by device buffers far larger
than any valid call of this size needs (the CPU test, which runs the NULL-handle rows only, by None), or None.  Every row is
decided by a host check before any HIP call: nothing is read, written or launched.

Per entry: every rejection it can return at this size, at least one call that breaks two rules at once (the earlier rule's
message wins: the order of the checks is part of the entry), and the early BODYFIT_OK of n_frames == 0 / n_rows == 0 / nothing
asked for.  Not reachable with an 8 x 8 image and an int n_frames, so not in the table: "2^39 pixels or more in one call",
"2^30 pixels or more in a frame"; decided only after hipSetDevice: the 2^39 bounds of the two texel-gradient entries."""

OK, INVALID = 0, 1
HANDLE, IN, OUT, OUT2, LL, INT = "HANDLE", "IN", "OUT", "OUT2", "LL", "INT"
NAN, INF = float("nan"), float("inf")

N_VERTS, FACES, WIDTH, HEIGHT = 4, [[0, 1, 2], [0, 2, 3]], 8, 8

_CAMERA = dict(fx=10.0, fy=10.0, cx=4.0, cy=4.0)
_VERTS = dict(r=HANDLE, d_verts=IN, verts_frame_stride=12, n_frames=2)
_ROWS = dict(_VERTS, **_CAMERA, d_face_image=IN, d_pixel=None, d_offset=None, n_rows=128)
_TEX = dict(r=HANDLE, d_face=IN, d_bary=IN, d_verts=IN, verts_frame_stride=12, d_uv=IN, n_uv=6, d_uv_faces=IN, d_tex=IN,
            tex_kind=1, n_channels=3, tex_height=4, tex_width=4, tex_frame_stride=0, n_frames=2)
_MIP = dict(_TEX, **_CAMERA, d_mip=IN, mip_frame_stride=0, max_level=-1, lod_bias=0.0)
_LIGHT = dict(r=HANDLE, d_face=IN, d_bary=IN, d_verts=IN, verts_frame_stride=12, d_normals=IN, normals_frame_stride=12,
              d_albedo=IN, n_channels=3, d_light=IN, light_frame_stride=0, n_frames=2)

ARGS = {
    "bodyfit_raster_render_device": dict(_VERTS, **_CAMERA, z_near=0.1, cull_backfaces=0, d_depth=OUT, d_face=OUT, d_bary=OUT,
                                         stream=None),
    "bodyfit_raster_visibility_device": dict(r=HANDLE, d_face=IN, n_frames=2, d_face_visible=OUT, d_vert_visible=OUT, stream=None),
    "bodyfit_raster_depth_rows_device": dict(_ROWS, d_index=OUT, d_z=OUT, d_bary=OUT, d_dir=OUT, stream=None),
    "bodyfit_raster_interp_rows_device": dict(_ROWS, d_attr=IN, attr_frame_stride=12, n_channels=3, d_grad_image=IN, d_grad_z=IN,
                                              d_index=OUT, d_bary=OUT, d_dir=OUT, d_value=OUT, stream=None),
    "bodyfit_raster_interp_rows_indexed_device": dict(_ROWS, d_attr=IN, attr_frame_stride=18, n_channels=3, d_attr_faces=IN,
                                                      n_attr_rows=6, d_grad_image=IN, d_grad_z=IN, d_index=OUT, d_bary=OUT,
                                                      d_dir=OUT, d_value=OUT, stream=None),
    "bodyfit_raster_shade_device": dict(r=HANDLE, d_face=IN, d_bary=IN, d_verts=IN, verts_frame_stride=12, d_attr=IN,
                                        attr_frame_stride=12, n_channels=3, n_frames=2, background=None, d_image=OUT, d_weight=OUT,
                                        stream=None),
    "bodyfit_raster_sample_device": dict(r=HANDLE, d_points=IN, points_frame_stride=15, n_points=5, n_frames=2, **_CAMERA,
                                         z_near=0.1, d_image=IN, image_kind=1, n_channels=3, image_frame_stride=192, d_gate=None,
                                         d_value=OUT, d_valid=OUT, d_grad=OUT, stream=None),
    "bodyfit_raster_distance_device": dict(r=HANDLE, d_seed=IN, seed_kind=1, seed_frame_stride=64, n_frames=2, invert=0,
                                           d_dist2=OUT, d_nearest=OUT, stream=None),
    "bodyfit_raster_edges_device": dict(_VERTS, **_CAMERA, z_near=0.1, cull_backfaces=0, d_face=IN, d_depth=IN, d_weight=OUT,
                                        stream=None),
    "bodyfit_raster_edge_blend_device": dict(r=HANDLE, d_weight=IN, d_image=IN, n_channels=3, n_frames=2, transpose=0, d_out=OUT,
                                             stream=None),
    "bodyfit_raster_edge_rows_device": dict(_VERTS, **_CAMERA, z_near=0.1, cull_backfaces=0, d_face=IN, d_depth=IN, d_image=IN,
                                            d_grad=IN, n_channels=3, d_pair=IN, d_offset=None, n_pairs=4, d_index=OUT, d_bary=OUT,
                                            d_coef=OUT, d_dir=OUT, stream=None),
    "bodyfit_raster_last_bins": dict(r=HANDLE, n_entries=LL, longest=INT),
    "bodyfit_raster_texture_device": dict(_TEX, background=None, d_image=OUT, d_weight=OUT, d_uv_out=OUT, stream=None),
    "bodyfit_raster_texture_grad_device": dict(_TEX, d_grad_image=IN, d_grad_uv=OUT, d_grad_tex=OUT, d_workspace=OUT2, stream=None),
    "bodyfit_raster_texture_mip_build_device": dict(r=HANDLE, d_tex=IN, tex_kind=1, n_channels=3, tex_height=4, tex_width=4,
                                                    tex_frame_stride=0, n_textures=1, max_level=-1, d_mip=OUT, mip_frame_stride=0,
                                                    stream=None),
    "bodyfit_raster_texture_mip_device": dict(_MIP, background=None, d_image=OUT, d_weight=OUT, d_uv_out=OUT, d_lod=OUT, stream=None),
    "bodyfit_raster_texture_mip_grad_device": dict(_MIP, d_grad_image=IN, d_grad_uv=OUT, d_grad_tex=OUT, d_workspace=OUT2,
                                                   stream=None),
    "bodyfit_raster_light_device": dict(_LIGHT, d_image=OUT, d_normal=OUT, d_shading=OUT, stream=None),
    "bodyfit_raster_light_grad_device": dict(_LIGHT, d_grad_image=IN, d_grad_albedo=OUT, d_grad_m=OUT, d_grad_light=OUT,
                                             d_workspace=OUT2, stream=None),
}

_NULL = "handle is NULL"
_FRAMES = "negative n_frames"
_INTR = "fx and fy must be positive, and the intrinsics finite"
_ZNEAR = "z_near must be positive"
_STRIDE = "verts_frame_stride below 3 n_verts"
_CH = "n_channels outside 1 .. 4"
_TEXSIZE = "texture size outside 1 .. 16384"
_TEXKIND = "tex_kind must be 0 (u8) or 1 (f32)"
_MIPINTR = "fx or fy <= 0 or a non-finite intrinsic"
_MIPTOTAL = "mip_frame_stride below the layout's total"


def _rows_cases(e, neg):
    """the rules the depth rows and the two interpolation rows state alike"""
    return [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_frames=-1), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, neg),
        (e, dict(n_rows=-1), INVALID, neg),
        (e, dict(n_rows=-1, fx=0.0), INVALID, neg),
        (e, dict(fx=0.0), INVALID, _INTR),
        (e, dict(fy=-1.0), INVALID, _INTR),
        (e, dict(fx=INF), INVALID, _INTR),
        (e, dict(cx=NAN), INVALID, _INTR),
        (e, dict(cy=-INF), INVALID, _INTR),
        (e, dict(fx=0.0, d_offset=IN), INVALID, _INTR),
        (e, dict(d_offset=IN), INVALID, "d_offset without d_pixel"),
        (e, dict(d_offset=IN, n_rows=100), INVALID, "d_offset without d_pixel"),
        (e, dict(n_rows=100), INVALID, "without d_pixel n_rows must be n_frames H W"),
        (e, dict(n_frames=0), INVALID, "without d_pixel n_rows must be n_frames H W"),
        (e, dict(d_pixel=IN, n_rows=(1 << 31) - 4096), INVALID, "2^31 rows or more in one call"),
        (e, dict(d_pixel=IN, n_rows=1 << 31, n_frames=0), INVALID, "2^31 rows or more in one call"),
        (e, dict(n_frames=1 << 25, n_rows=1 << 31), INVALID, "2^31 rows or more in one call"),
        (e, dict(d_pixel=IN, n_rows=5, n_frames=0), INVALID, "rows without frames"),
        (e, dict(d_pixel=IN, n_rows=5), INVALID, "a uniform row set needs n_rows divisible by n_frames"),
        (e, dict(d_pixel=IN, n_rows=5, d_face_image=None), INVALID, "a uniform row set needs n_rows divisible by n_frames"),
        (e, dict(n_frames=0, n_rows=0, d_face_image=None, d_index=None, d_verts=None), OK, None),
        (e, dict(d_pixel=IN, n_rows=0, d_face_image=None, verts_frame_stride=0), OK, None),
        (e, dict(d_pixel=IN, d_offset=IN, n_rows=0, d_index=None), OK, None),
        (e, dict(d_face_image=None), INVALID, "d_face_image or d_index is NULL"),
        (e, dict(d_index=None), INVALID, "d_face_image or d_index is NULL"),
        (e, dict(d_index=None, d_verts=None, verts_frame_stride=11), INVALID, "d_face_image or d_index is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts is NULL"),
        (e, dict(d_verts=None, verts_frame_stride=11), INVALID, "d_verts is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
    ]


def _interp_cases(e, table_words):
    """what the two interpolation-row entries add to the row rules; table_words: the attribute table's name in the stride message"""
    return [
        (e, dict(n_channels=-1), INVALID, "n_channels outside 0 .. 4"),
        (e, dict(n_channels=5), INVALID, "n_channels outside 0 .. 4"),
        (e, dict(n_channels=5, fx=0.0), INVALID, _INTR),
        (e, dict(n_channels=5, d_offset=IN), INVALID, "n_channels outside 0 .. 4"),
        (e, dict(n_channels=5, n_frames=0, n_rows=0), INVALID, "n_channels outside 0 .. 4"),
        (e, dict(verts_frame_stride=11, d_attr=None), INVALID, _STRIDE),
        (e, dict(d_attr=None), INVALID, "d_attr or d_grad_image is NULL with n_channels > 0"),
        (e, dict(d_grad_image=None), INVALID, "d_attr or d_grad_image is NULL with n_channels > 0"),
        (e, dict(d_attr=None, attr_frame_stride=1), INVALID, "d_attr or d_grad_image is NULL with n_channels > 0"),
        (e, dict(attr_frame_stride=1), INVALID, "a non-zero attr_frame_stride below n_channels " + table_words),
        (e, dict(n_channels=0, d_grad_z=None), INVALID, "n_channels == 0 needs d_grad_z"),
        (e, dict(n_channels=0, d_grad_z=None, d_attr=None, d_grad_image=None, attr_frame_stride=1), INVALID,
         "n_channels == 0 needs d_grad_z"),
    ]


def _tx_cases(e):
    """tx_check: what the four texture lookups and gradients state alike"""
    return [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_channels=0), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, n_channels=0), INVALID, _FRAMES),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, tex_kind=2), INVALID, _CH),
        (e, dict(tex_kind=2), INVALID, _TEXKIND),
        (e, dict(tex_kind=-1, tex_height=0), INVALID, _TEXKIND),
        (e, dict(tex_height=0), INVALID, _TEXSIZE),
        (e, dict(tex_width=16385), INVALID, _TEXSIZE),
        (e, dict(tex_width=0, n_uv=-1), INVALID, _TEXSIZE),
        (e, dict(n_uv=-1), INVALID, "negative n_uv"),
        (e, dict(n_uv=-1, tex_frame_stride=47), INVALID, "negative n_uv"),
        (e, dict(tex_frame_stride=47), INVALID, "a non-zero tex_frame_stride below Ht Wt n_channels"),
        (e, dict(tex_frame_stride=47, n_frames=0), INVALID, "a non-zero tex_frame_stride below Ht Wt n_channels"),
        (e, dict(d_face=None), INVALID, "d_face or d_bary is NULL"),
        (e, dict(d_bary=None, d_verts=None), INVALID, "d_face or d_bary is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts or d_uv_faces is NULL"),
        (e, dict(d_uv_faces=None, d_uv=None), INVALID, "d_verts or d_uv_faces is NULL"),
        (e, dict(d_uv=None), INVALID, "d_uv is NULL"),
        (e, dict(d_uv=None, verts_frame_stride=11), INVALID, "d_uv is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
    ]


def _lt_cases(e):
    """lt_check: what the lighting and its gradient state alike"""
    return [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_frames=-1), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, n_channels=5), INVALID, _FRAMES),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, light_frame_stride=1), INVALID, _CH),
        (e, dict(light_frame_stride=26), INVALID, "a non-zero light_frame_stride below 9 n_channels"),
        (e, dict(light_frame_stride=26, n_frames=0), INVALID, "a non-zero light_frame_stride below 9 n_channels"),
        (e, dict(n_frames=0, d_face=None, d_light=None), OK, None),
        (e, dict(d_face=None), INVALID, "d_face, d_bary, d_albedo or d_light is NULL"),
        (e, dict(d_bary=None), INVALID, "d_face, d_bary, d_albedo or d_light is NULL"),
        (e, dict(d_albedo=None), INVALID, "d_face, d_bary, d_albedo or d_light is NULL"),
        (e, dict(d_light=None, d_verts=None), INVALID, "d_face, d_bary, d_albedo or d_light is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts or d_normals is NULL"),
        (e, dict(d_normals=None, verts_frame_stride=11), INVALID, "d_verts or d_normals is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
        (e, dict(verts_frame_stride=11, normals_frame_stride=11), INVALID, _STRIDE),
        (e, dict(normals_frame_stride=11), INVALID, "normals_frame_stride below 3 n_verts"),
    ]


def _table():
    t = []
    e = "bodyfit_raster_render_device"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_frames=-1, z_near=0.0), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, z_near=0.0), INVALID, _FRAMES),
        (e, dict(z_near=0.0), INVALID, _ZNEAR),
        (e, dict(z_near=NAN), INVALID, _ZNEAR),
        (e, dict(z_near=-1.0, fx=0.0), INVALID, _ZNEAR),
        (e, dict(fx=0.0), INVALID, _INTR),
        (e, dict(fy=NAN), INVALID, _INTR),
        (e, dict(cx=INF), INVALID, _INTR),
        (e, dict(cy=NAN, n_frames=0), INVALID, _INTR),
        (e, dict(n_frames=0, d_depth=None, d_face=None, d_verts=None, verts_frame_stride=0), OK, None),
        (e, dict(d_depth=None), INVALID, "d_depth or d_face is NULL"),
        (e, dict(d_face=None, d_verts=None), INVALID, "d_depth or d_face is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts is NULL"),
        (e, dict(d_verts=None, verts_frame_stride=11), INVALID, "d_verts is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
        (e, dict(verts_frame_stride=11, n_frames=1 << 30), INVALID, _STRIDE),
        (e, dict(n_frames=1 << 30), INVALID, "2^31 tiles or records or more in one call"),
    ]
    e = "bodyfit_raster_visibility_device"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_frames=-1), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, d_face=None), INVALID, _FRAMES),
        (e, dict(n_frames=0, d_face=None), OK, None),
        (e, dict(d_face_visible=None, d_vert_visible=None, d_face=None), OK, None),
        (e, dict(d_face=None), INVALID, "d_face is NULL"),
        (e, dict(d_face=None, d_vert_visible=None), INVALID, "d_face is NULL"),
    ]
    e = "bodyfit_raster_depth_rows_device"
    t += _rows_cases(e, "negative n_frames or n_rows")
    for e, words in (("bodyfit_raster_interp_rows_device", "n_verts"), ("bodyfit_raster_interp_rows_indexed_device", "n_attr_rows")):
        t += _rows_cases(e, "negative n_frames or n_rows") + _interp_cases(e, words)
    e = "bodyfit_raster_interp_rows_indexed_device"
    t += [
        (e, dict(n_attr_rows=-1), INVALID, "negative n_attr_rows"),
        (e, dict(n_attr_rows=-1, n_channels=5), INVALID, "n_channels outside 0 .. 4"),
        (e, dict(n_attr_rows=-1, d_offset=IN), INVALID, "negative n_attr_rows"),
        (e, dict(attr_frame_stride=17), INVALID, "a non-zero attr_frame_stride below n_channels n_attr_rows"),
        (e, dict(attr_frame_stride=17, d_attr_faces=None), INVALID, "a non-zero attr_frame_stride below n_channels n_attr_rows"),
        (e, dict(d_attr_faces=None), INVALID, "d_attr_faces is NULL"),
        (e, dict(d_attr_faces=None, n_channels=0, d_grad_z=None), INVALID, "n_channels == 0 needs d_grad_z"),
    ]
    e = "bodyfit_raster_interp_rows_device"
    t += [(e, dict(attr_frame_stride=11), INVALID, "a non-zero attr_frame_stride below n_channels n_verts")]
    e = "bodyfit_raster_shade_device"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_channels=0), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, n_channels=5), INVALID, _FRAMES),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, n_frames=0), INVALID, _CH),
        (e, dict(n_frames=0, d_face=None, d_image=None, verts_frame_stride=0), OK, None),
        (e, dict(d_face=None), INVALID, "d_face, d_bary or d_image is NULL"),
        (e, dict(d_bary=None), INVALID, "d_face, d_bary or d_image is NULL"),
        (e, dict(d_image=None, d_verts=None), INVALID, "d_face, d_bary or d_image is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts or d_attr is NULL"),
        (e, dict(d_attr=None, verts_frame_stride=11), INVALID, "d_verts or d_attr is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
        (e, dict(verts_frame_stride=11, attr_frame_stride=11), INVALID, _STRIDE),
        (e, dict(attr_frame_stride=11), INVALID, "a non-zero attr_frame_stride below n_channels n_verts"),
    ]
    e = "bodyfit_raster_sample_device"
    neg = "negative n_frames or n_points"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_points=-1), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, neg),
        (e, dict(n_points=-1), INVALID, neg),
        (e, dict(n_points=-1, n_channels=0), INVALID, neg),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, image_kind=2), INVALID, _CH),
        (e, dict(image_kind=2), INVALID, "image_kind must be 0 (u8) or 1 (f32)"),
        (e, dict(image_kind=-1, z_near=0.0), INVALID, "image_kind must be 0 (u8) or 1 (f32)"),
        (e, dict(z_near=0.0), INVALID, _ZNEAR),
        (e, dict(z_near=NAN, fx=0.0), INVALID, _ZNEAR),
        (e, dict(fx=0.0), INVALID, _INTR),
        (e, dict(cy=INF, n_frames=0), INVALID, _INTR),
        (e, dict(n_frames=0, d_points=None, d_image=None), OK, None),
        (e, dict(n_points=0, d_value=None, d_valid=None, points_frame_stride=0), OK, None),
        (e, dict(d_points=None), INVALID, "d_points, d_image, d_value or d_valid is NULL"),
        (e, dict(d_image=None), INVALID, "d_points, d_image, d_value or d_valid is NULL"),
        (e, dict(d_value=None), INVALID, "d_points, d_image, d_value or d_valid is NULL"),
        (e, dict(d_valid=None, points_frame_stride=14), INVALID, "d_points, d_image, d_value or d_valid is NULL"),
        (e, dict(points_frame_stride=14), INVALID, "points_frame_stride below 3 n_points"),
        (e, dict(points_frame_stride=14, image_frame_stride=191), INVALID, "points_frame_stride below 3 n_points"),
        (e, dict(image_frame_stride=191), INVALID, "image_frame_stride below H W n_channels"),
        (e, dict(image_frame_stride=191, n_points=1 << 38, points_frame_stride=3 << 38), INVALID,
         "image_frame_stride below H W n_channels"),
        (e, dict(n_points=1 << 38, points_frame_stride=3 << 38), INVALID, "2^39 points or more in one call"),
    ]
    e = "bodyfit_raster_distance_device"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, seed_kind=2), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, seed_kind=2), INVALID, _FRAMES),
        (e, dict(seed_kind=2), INVALID, "seed_kind must be 0 (u8) or 1 (int32)"),
        (e, dict(seed_kind=-1, n_frames=0), INVALID, "seed_kind must be 0 (u8) or 1 (int32)"),
        (e, dict(n_frames=0, d_seed=None, d_dist2=None, seed_frame_stride=0), OK, None),
        (e, dict(d_seed=None), INVALID, "d_seed or d_dist2 is NULL"),
        (e, dict(d_dist2=None, seed_frame_stride=63), INVALID, "d_seed or d_dist2 is NULL"),
        (e, dict(seed_frame_stride=63), INVALID, "seed_frame_stride below H W"),
    ]
    e = "bodyfit_raster_edges_device"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, z_near=0.0), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, z_near=0.0), INVALID, _FRAMES),
        (e, dict(z_near=0.0), INVALID, _ZNEAR),
        (e, dict(z_near=NAN, fy=0.0), INVALID, _ZNEAR),
        (e, dict(fy=0.0), INVALID, _INTR),
        (e, dict(cx=NAN, n_frames=0), INVALID, _INTR),
        (e, dict(n_frames=0, d_weight=None, d_verts=None), OK, None),
        (e, dict(d_weight=None), INVALID, "d_weight is NULL"),
        (e, dict(d_weight=None, d_verts=None), INVALID, "d_weight is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts, d_face or d_depth is NULL"),
        (e, dict(d_face=None), INVALID, "d_verts, d_face or d_depth is NULL"),
        (e, dict(d_depth=None, verts_frame_stride=11), INVALID, "d_verts, d_face or d_depth is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
    ]
    e = "bodyfit_raster_edge_blend_device"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_frames=-1), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, _FRAMES),
        (e, dict(n_frames=-1, n_channels=0), INVALID, _FRAMES),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, n_frames=0), INVALID, _CH),
        (e, dict(n_frames=0, d_weight=None, d_image=None, d_out=None), OK, None),
        (e, dict(d_weight=None), INVALID, "d_weight, d_image or d_out is NULL"),
        (e, dict(d_image=None, d_out=None), INVALID, "d_weight, d_image or d_out is NULL"),
        (e, dict(d_out=None), INVALID, "d_weight, d_image or d_out is NULL"),
        (e, dict(d_out=IN), INVALID, "d_out must not be d_image"),
    ]
    e = "bodyfit_raster_edge_rows_device"
    neg = "negative n_frames or n_pairs"
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_pairs=-1), INVALID, _NULL),
        (e, dict(n_frames=-1), INVALID, neg),
        (e, dict(n_pairs=-1), INVALID, neg),
        (e, dict(n_pairs=-1, n_channels=0), INVALID, neg),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, z_near=0.0), INVALID, _CH),
        (e, dict(z_near=0.0), INVALID, _ZNEAR),
        (e, dict(z_near=NAN, fx=0.0), INVALID, _ZNEAR),
        (e, dict(fx=0.0), INVALID, _INTR),
        (e, dict(cx=INF, n_pairs=1 << 30), INVALID, _INTR),
        (e, dict(n_pairs=(1 << 30) - 2048), INVALID, "2^30 pairs or more in one call"),
        (e, dict(n_pairs=1 << 30, n_frames=0), INVALID, "2^30 pairs or more in one call"),
        (e, dict(n_pairs=3, n_frames=0), INVALID, "pairs without frames"),
        (e, dict(n_pairs=3), INVALID, "a uniform pair list needs n_pairs divisible by n_frames"),
        (e, dict(n_pairs=3, d_pair=None), INVALID, "a uniform pair list needs n_pairs divisible by n_frames"),
        (e, dict(n_frames=0, n_pairs=0, d_pair=None, d_index=None), OK, None),
        (e, dict(n_pairs=0, d_pair=None, d_verts=None, verts_frame_stride=0), OK, None),
        (e, dict(d_pair=None), INVALID, "d_pair or an output is NULL"),
        (e, dict(d_index=None), INVALID, "d_pair or an output is NULL"),
        (e, dict(d_bary=None), INVALID, "d_pair or an output is NULL"),
        (e, dict(d_coef=None), INVALID, "d_pair or an output is NULL"),
        (e, dict(d_dir=None, d_verts=None), INVALID, "d_pair or an output is NULL"),
        (e, dict(d_verts=None), INVALID, "d_verts, d_face, d_depth, d_image or d_grad is NULL"),
        (e, dict(d_face=None), INVALID, "d_verts, d_face, d_depth, d_image or d_grad is NULL"),
        (e, dict(d_depth=None), INVALID, "d_verts, d_face, d_depth, d_image or d_grad is NULL"),
        (e, dict(d_image=None), INVALID, "d_verts, d_face, d_depth, d_image or d_grad is NULL"),
        (e, dict(d_grad=None, verts_frame_stride=11), INVALID, "d_verts, d_face, d_depth, d_image or d_grad is NULL"),
        (e, dict(verts_frame_stride=11), INVALID, _STRIDE),
    ]
    e = "bodyfit_raster_last_bins"
    t += [
        (e, dict(r=None), INVALID, "null argument"),
        (e, dict(r=None, longest=None), INVALID, "null argument"),      # (its one rule)
        (e, dict(n_entries=None), INVALID, "null argument"),
        (e, dict(longest=None), INVALID, "null argument"),
    ]
    e = "bodyfit_raster_texture_device"
    t += _tx_cases(e) + [
        (e, dict(n_frames=0, d_face=None, d_image=None, d_tex=None), OK, None),
        (e, dict(verts_frame_stride=11, d_image=None), INVALID, _STRIDE),
        (e, dict(d_image=None), INVALID, "d_image is NULL"),
        (e, dict(d_image=None, d_tex=None), INVALID, "d_image is NULL"),
        (e, dict(d_tex=None), INVALID, "d_tex is NULL"),
    ]
    e = "bodyfit_raster_texture_grad_device"
    t += _tx_cases(e) + [
        (e, dict(n_frames=0, d_face=None, d_grad_image=None), OK, None),
        (e, dict(d_grad_uv=None, d_grad_tex=None, d_grad_image=None, d_tex=None), OK, None),
        (e, dict(verts_frame_stride=11, d_grad_image=None), INVALID, _STRIDE),
        (e, dict(d_grad_image=None), INVALID, "d_grad_image is NULL"),
        (e, dict(d_grad_image=None, d_workspace=None), INVALID, "d_grad_image is NULL"),
        (e, dict(d_workspace=None), INVALID, "d_grad_tex without d_workspace"),
        (e, dict(d_workspace=None, d_tex=None), INVALID, "d_grad_tex without d_workspace"),
        (e, dict(d_tex=None), INVALID, "d_grad_uv without d_tex"),
    ]
    e = "bodyfit_raster_texture_mip_build_device"
    big = dict(tex_height=16384, tex_width=16384, n_channels=4, n_textures=4096, tex_frame_stride=1 << 30,
               mip_frame_stride=4 * ((4 ** 14 - 1) // 3))
    t += [
        (e, dict(r=None), INVALID, _NULL),
        (e, dict(r=None, n_textures=-1), INVALID, _NULL),
        (e, dict(n_textures=-1), INVALID, "negative n_textures"),
        (e, dict(n_textures=-1, n_channels=0), INVALID, "negative n_textures"),
        (e, dict(n_channels=0), INVALID, _CH),
        (e, dict(n_channels=5, tex_kind=2), INVALID, _CH),
        (e, dict(tex_kind=2), INVALID, _TEXKIND),
        (e, dict(tex_kind=2, tex_width=0), INVALID, _TEXKIND),
        (e, dict(tex_height=16385), INVALID, _TEXSIZE),
        (e, dict(tex_width=0, n_textures=2), INVALID, _TEXSIZE),
        (e, dict(n_textures=2, tex_frame_stride=47, mip_frame_stride=15), INVALID, "tex_frame_stride below Ht Wt n_channels"),
        (e, dict(n_textures=2, tex_frame_stride=47, mip_frame_stride=14), INVALID, "tex_frame_stride below Ht Wt n_channels"),
        (e, dict(n_textures=2, tex_frame_stride=48, mip_frame_stride=14), INVALID, _MIPTOTAL),
        (e, dict(n_textures=2, tex_frame_stride=48, mip_frame_stride=14, d_tex=None), INVALID, _MIPTOTAL),
        (e, dict(n_textures=0, d_tex=None, d_mip=None), OK, None),
        (e, dict(tex_height=1, tex_width=1, d_tex=None, d_mip=None), OK, None),
        (e, dict(max_level=0, d_mip=None), OK, None),
        (e, dict(d_tex=None), INVALID, "d_tex or d_mip is NULL"),
        (e, dict(d_mip=None), INVALID, "d_tex or d_mip is NULL"),
        (e, dict(big, d_mip=None), INVALID, "d_tex or d_mip is NULL"),
        (e, big, INVALID, "2^39 pyramid elements or more in one call"),
    ]
    for e in ("bodyfit_raster_texture_mip_device", "bodyfit_raster_texture_mip_grad_device"):
        t += _tx_cases(e) + [
            (e, dict(verts_frame_stride=11, fx=0.0), INVALID, _STRIDE),
            (e, dict(fx=0.0), INVALID, _MIPINTR),
            (e, dict(fy=-1.0), INVALID, _MIPINTR),
            (e, dict(fx=NAN), INVALID, _MIPINTR),
            (e, dict(cx=INF), INVALID, _MIPINTR),
            (e, dict(cy=NAN, lod_bias=NAN), INVALID, _MIPINTR),
            (e, dict(fx=0.0, n_frames=0), INVALID, _MIPINTR),             # (the mip arguments are checked without frames too)
            (e, dict(lod_bias=NAN), INVALID, "lod_bias is NaN"),
            (e, dict(lod_bias=NAN, d_mip=None), INVALID, "lod_bias is NaN"),
            (e, dict(d_mip=None), INVALID, "d_mip is NULL with more than one level"),
            (e, dict(d_mip=None, n_frames=0), INVALID, "d_mip is NULL with more than one level"),
            (e, dict(d_mip=None, tex_frame_stride=48, mip_frame_stride=14), INVALID, "d_mip is NULL with more than one level"),
            (e, dict(tex_frame_stride=48, mip_frame_stride=14), INVALID, _MIPTOTAL),
            (e, dict(n_frames=0, d_face=None), OK, None),
            (e, dict(n_frames=0, max_level=0, d_mip=None), OK, None),
        ]
    e = "bodyfit_raster_texture_mip_device"
    t += [
        (e, dict(tex_frame_stride=48, mip_frame_stride=14, d_image=None), INVALID, _MIPTOTAL),
        (e, dict(d_image=None), INVALID, "d_image is NULL"),
        (e, dict(d_image=None, d_tex=None), INVALID, "d_image is NULL"),
        (e, dict(d_tex=None), INVALID, "d_tex is NULL"),
    ]
    e = "bodyfit_raster_texture_mip_grad_device"
    t += [
        (e, dict(d_grad_uv=None, d_grad_tex=None, d_grad_image=None, d_mip=None), OK, None),
        (e, dict(tex_frame_stride=48, mip_frame_stride=14, d_grad_image=None), INVALID, _MIPTOTAL),
        (e, dict(d_grad_image=None), INVALID, "d_grad_image is NULL"),
        (e, dict(d_grad_image=None, d_workspace=None), INVALID, "d_grad_image is NULL"),
        (e, dict(d_workspace=None), INVALID, "d_grad_tex without d_workspace"),
        (e, dict(d_workspace=None, d_tex=None), INVALID, "d_grad_tex without d_workspace"),
        (e, dict(d_tex=None), INVALID, "d_grad_uv without d_tex"),
    ]
    e = "bodyfit_raster_light_device"
    t += _lt_cases(e) + [
        (e, dict(normals_frame_stride=11, d_image=None), INVALID, "normals_frame_stride below 3 n_verts"),
        (e, dict(d_image=None), INVALID, "d_image is NULL"),
    ]
    e = "bodyfit_raster_light_grad_device"
    t += _lt_cases(e) + [
        (e, dict(d_grad_albedo=None, d_grad_m=None, d_grad_light=None, d_grad_image=None), OK, None),
        (e, dict(normals_frame_stride=11, d_grad_image=None), INVALID, "normals_frame_stride below 3 n_verts"),
        (e, dict(d_grad_image=None), INVALID, "d_grad_image is NULL"),
        (e, dict(d_grad_image=None, d_workspace=None), INVALID, "d_grad_image is NULL"),
        (e, dict(d_workspace=None), INVALID, "d_grad_light without d_workspace"),
    ]
    return t


TABLE = _table()


def call(lib, entry, overrides, resolve):
    """(status, bodyfit_last_error()) of `entry` with its valid arguments but for `overrides`; resolve: token -> argument"""
    args = dict(ARGS[entry])
    unknown = set(overrides) - set(args)
    assert not unknown, (entry, unknown)
    args.update(overrides)
    fn = getattr(lib, entry)
    assert len(args) == len(fn.argtypes), (entry, len(args), len(fn.argtypes))
    rc = fn(*[resolve(v) if isinstance(v, str) else v for v in args.values()])
    return rc, lib.bodyfit_last_error().decode()


def mismatches(lib, rows, resolve):
    """the rows whose status or message is not the table's, as printable lines"""
    bad = []
    for entry, overrides, status, what in rows:
        rc, msg = call(lib, entry, overrides, resolve)
        if rc != status or (status != OK and msg != f"{entry}: {what}"):
            bad.append(f"{entry} {overrides}: status {rc} {msg!r}, expected {status} {what!r}")
    return bad
