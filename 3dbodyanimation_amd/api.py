"""ctypes binding of libbodyfit.so (include/bodyfit.h) and a thin host-side mirror of the reference types.

There is no CPU fallback: if the HIP library is missing, or no GPU is visible when a model is
created, the calls raise BodyfitError.  Names follow the reference: PixelKP (include/Sim3BA.h:9),
Sim3Params (:11-19), FramePoseParams (include/MultiFrameBA.h:9-14).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BODYFIT_LIB", os.path.join(_HERE, "libbodyfit.so"))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bodyfit.h")
N_FRAME_PARAMS = 76

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)


class BodyfitError(RuntimeError):
    pass


class _ModelDesc(C.Structure):
    _fields_ = [("n_verts", C.c_int), ("n_joints", C.c_int), ("n_shape", C.c_int), ("n_pose_feat", C.c_int),
                ("v_template", _dp), ("shapedirs", _dp), ("posedirs", _dp), ("j_regressor", _dp),
                ("weights", _dp), ("parent", _ip), ("n_landmarks", C.c_int), ("landmark_vid", _ip),
                ("n_kp_regressors", C.c_int), ("kpreg_offset", _ip), ("kpreg_vid", _ip), ("kpreg_weight", _dp)]


class _ProblemDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("kp_offset", _ip), ("kp_id", _ip), ("kp_uv", _dp),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("R0", _dp), ("n_cols", C.c_int), ("use_shape", C.c_int), ("beta_per_frame", C.c_int),
                ("pose_blend", C.c_int), ("beta_pose", C.c_double), ("gmm", C.c_void_p),
                ("beta_shape", C.c_double), ("lambda_temporal", C.c_double), ("temporal_halo", C.c_int),
                ("huber_delta", C.c_double), ("want_mesh", C.c_int)]


class Layout(C.Structure):
    _fields_ = [("n_keypoints", C.c_int), ("n_cols", C.c_int), ("reproj_rows", C.c_int),
                ("prior_rows_per_frame", C.c_int), ("shape_rows", C.c_int), ("temporal_rows", C.c_int),
                ("total_rows", C.c_int)]


class FitOptions(C.Structure):
    _fields_ = [("max_iters", C.c_int), ("scale_lo", C.c_double), ("scale_hi", C.c_double), ("verbose", C.c_int),
                ("solver", C.c_int)]


class FitSummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("termination", C.c_int), ("usable", C.c_int), ("n_successful", C.c_int),
                ("n_unsuccessful", C.c_int), ("n_sweeps", C.c_int), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("n_sweeps_issued", C.c_int)]


class _OverlayDesc(C.Structure):
    _fields_ = [("device", C.c_int), ("n_vertices", C.c_int), ("n_faces", C.c_int), ("faces", C.POINTER(C.c_int32)),
                ("width", C.c_int), ("height", C.c_int), ("max_frames", C.c_int)]


_ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.c_int, C.c_int)
_ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, _dp, C.c_int)


class Comm(C.Structure):   # bodyfit_comm (include/bodyfit.h)
    _fields_ = [("rank", C.c_int), ("size", C.c_int), ("ctx", C.c_void_p), ("allreduce", _ALLREDUCE_CB),
                ("allgather", _ALLGATHER_CB)]


class Rccl:
    """RCCL communicator of a sharded solve (bodyfit_rccl_*): created by the library from a 128-byte id that rank 0 obtains
    and the application ships to the other ranks (any host channel: here whatever the caller uses, e.g. torch.distributed
    broadcast_object_list), or wrapped around an ncclComm_t the application already has."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        _check(load_library().bodyfit_rccl_unique_id(buf))
        return bytes(buf)

    @classmethod
    def create(cls, uid: bytes, rank: int, size: int, device: int = 0) -> "Rccl":
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        h = C.c_void_p()
        _check(load_library().bodyfit_rccl_create(buf, rank, size, device, C.byref(h)))
        return cls(h)

    @classmethod
    def wrap(cls, nccl_comm_ptr: int, rank: int, size: int) -> "Rccl":
        h = C.c_void_p()
        _check(load_library().bodyfit_rccl_wrap(C.c_void_p(nccl_comm_ptr), rank, size, C.byref(h)))
        return cls(h)

    def count(self) -> tuple[int, int]:
        """(ranks, this rank) as RCCL itself reports them (ncclCommCount, ncclCommUserRank)."""
        n, r = C.c_int(), C.c_int()
        _check(load_library().bodyfit_rccl_count(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def allreduce_shared(self, d_buf66_ptr: int, stream: int | None = None):
        """The evaluation path's one collective: ncclAllReduce(sum, f64) of the 66 doubles, in place, on `stream`."""
        _check(load_library().bodyfit_allreduce_shared_rccl(self.h, d_buf66_ptr, stream))

    def close(self):
        if self.h:
            load_library().bodyfit_rccl_destroy(self.h)
            self.h = None


class DeviceViews(C.Structure):
    _fields_ = [("residuals", C.c_void_p), ("jacobian", C.c_void_p), ("gmm_comp", C.c_void_p),
                ("cloud", C.c_void_p), ("joints", C.c_void_p), ("normal_eq", C.c_void_p),
                ("cloud_frame_stride", C.c_longlong)]


class PointSet(C.Structure):   # bodyfit_pointset (include/bodyfit.h): device pointers
    """f32 xyz rows on the device, per frame: uniform (n_per_frame rows, frame_stride floats between frames) or ragged (d_offset:
    a device int32 CSR [F + 1] over one packed [N][3] array)."""
    _fields_ = [("d_xyz", C.c_void_p), ("d_offset", C.c_void_p), ("n_per_frame", C.c_int), ("frame_stride", C.c_longlong)]

    @classmethod
    def uniform(cls, d_xyz_ptr: int, n_per_frame: int, frame_stride: int | None = None) -> "PointSet":
        return cls(d_xyz_ptr, None, int(n_per_frame), 3 * int(n_per_frame) if frame_stride is None else int(frame_stride))

    @classmethod
    def ragged(cls, d_xyz_ptr: int, d_offset_ptr: int) -> "PointSet":
        return cls(d_xyz_ptr, d_offset_ptr, 0, 0)


_lib = None


def launch_count() -> int:
    """kernels launched through the library by this process so far (bodyfit_launch_count)"""
    return int(load_library().bodyfit_launch_count())


def declared_symbols() -> list[str]:
    """Every function include/bodyfit.h declares (used by the ABI test)."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(bodyfit_[a-z0-9_]+)\s*\(", txt)))


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BodyfitError(f"{LIB_PATH} is missing: build it with `make -C 3dbodyanimation_amd/csrc` "
                           "(__graft_entry__.build()). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; loading the system one first
    # makes torch.cuda see no GPU.  Importing torch first lets libbodyfit.so bind to the runtime torch
    # already mapped (same soname), so streams / tensors / RCCL and our kernels share one context.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.bodyfit_last_error.restype = C.c_char_p
    lib.bodyfit_mean_pixel_error.restype = C.c_double
    lib.bodyfit_mean_pixel_error.argtypes = [C.c_int, _ip, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.bodyfit_model_create.argtypes = [C.POINTER(_ModelDesc), C.c_int, C.POINTER(C.c_void_p)]
    lib.bodyfit_model_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_model_get_derived.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.bodyfit_gmm_create.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.bodyfit_gmm_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_gmm_get.argtypes = [C.c_void_p, _dp, _dp]
    lib.bodyfit_problem_create.argtypes = [C.c_void_p, C.POINTER(_ProblemDesc), C.POINTER(C.c_void_p)]
    lib.bodyfit_problem_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_problem_layout.argtypes = [C.c_void_p, C.POINTER(Layout)]
    lib.bodyfit_problem_views.argtypes = [C.c_void_p, C.POINTER(DeviceViews)]
    lib.bodyfit_evaluate_batch.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _ip, C.c_int]
    lib.bodyfit_evaluate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.bodyfit_reduce_shared_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_arm_shared_reduction.argtypes = [C.c_void_p, C.c_void_p]
    lib.bodyfit_profile_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, _dp]
    lib.bodyfit_solve.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_ubyte), C.c_int, C.POINTER(FitOptions),
                                  C.POINTER(FitSummary), C.c_int]
    lib.bodyfit_solve_sharded.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_ubyte), C.POINTER(Comm), C.POINTER(FitOptions),
                                          C.POINTER(FitSummary)]
    lib.bodyfit_solve_sharded_rccl.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_ubyte), C.c_void_p, C.POINTER(FitOptions),
                                               C.POINTER(FitSummary)]
    lib.bodyfit_rccl_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
    lib.bodyfit_rccl_create.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.bodyfit_rccl_wrap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.bodyfit_rccl_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_rccl_destroy.restype = None
    lib.bodyfit_allreduce_shared_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_rccl_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.bodyfit_sweep_status.argtypes = [C.c_void_p, C.c_void_p]
    lib.bodyfit_sweep_timeouts.argtypes = [C.c_void_p]
    lib.bodyfit_sweep_timeouts.restype = C.c_long
    lib.bodyfit_set_exchange_timeout.argtypes = [C.c_void_p, C.c_double]
    lib.bodyfit_set_shard_proxy.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.bodyfit_launch_count.argtypes = []
    lib.bodyfit_launch_count.restype = C.c_long
    lib.bodyfit_last_exchange_count.argtypes = [C.c_void_p]
    lib.bodyfit_last_exchange_count.restype = C.c_long
    lib.bodyfit_forward.argtypes = [C.c_void_p, _dp, _dp, _dp, _fp]
    lib.bodyfit_forward_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_forward_vjp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_forward_vjp.argtypes = [C.c_void_p, _dp, _dp, _fp, _dp, _dp, _dp]
    lib.bodyfit_forward_jvp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_forward_jvp.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp, _fp]
    lib.bodyfit_forward_offsets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                   C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_forward_offsets_vjp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                       C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_forward_offsets_jvp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_forward_offsets.argtypes = [C.c_void_p, _dp, _dp, _fp, C.c_longlong, _dp, _fp]
    lib.bodyfit_forward_offsets_vjp.argtypes = [C.c_void_p, _dp, _dp, _fp, C.c_longlong, _fp, _dp, _dp, _dp, _fp]
    lib.bodyfit_surface_laplacian_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_void_p]
    lib.bodyfit_residuals_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.bodyfit_residual_vjp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p]
    lib.bodyfit_residual_vjp.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
    lib.bodyfit_closest_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.bodyfit_closest_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_closest_destroy.restype = None
    lib.bodyfit_closest_points_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.POINTER(PointSet), C.c_int, C.c_longlong,
                                                  C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.bodyfit_closest_points_vjp_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.POINTER(PointSet), C.c_int, C.c_longlong,
                                                      C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_surface_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]
    lib.bodyfit_surface_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_surface_destroy.restype = None
    lib.bodyfit_closest_surface_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.c_void_p, C.c_longlong, C.c_int, C.c_longlong,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.bodyfit_closest_surface_oriented_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.c_void_p, C.c_float, C.c_void_p,
                                                            C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_int, C.c_void_p]
    lib.bodyfit_closest_surface_vjp_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.c_void_p, C.c_longlong, C.c_int,
                                                       C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
    lib.bodyfit_surface_rows_vjp_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_surface_winding_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.c_void_p, C.c_void_p, C.c_longlong, C.c_int,
                                                   C.c_longlong, C.c_void_p, C.c_void_p]
    lib.bodyfit_surface_vertex_normals_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    lib.bodyfit_surface_gram_device.argtypes = [C.c_void_p, C.POINTER(PointSet), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong,
                                                C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_writeback_batch.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _fp, _dp]
    lib.bodyfit_evaluate_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_dp), _dp, C.POINTER(_dp)]
    _u8p = C.POINTER(C.c_uint8)
    _i32p = C.POINTER(C.c_int32)
    lib.bodyfit_overlay_create.argtypes = [C.POINTER(_OverlayDesc), C.POINTER(C.c_void_p)]
    lib.bodyfit_overlay_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_overlay_destroy.restype = None
    lib.bodyfit_overlay_render_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p,
                                                  C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.c_double,
                                                  C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.bodyfit_overlay_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, _u8p, C.c_size_t,
                                           C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                           C.c_int]
    lib.bodyfit_overlay_drawlist.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), _i32p, _i32p, _i32p]
    lib.bodyfit_overlay_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.bodyfit_raster_create.argtypes = [C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.bodyfit_raster_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_raster_destroy.restype = None
    lib.bodyfit_raster_render_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double,
                                                 C.c_double, C.c_double, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_visibility_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_depth_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double,
                                                     C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_interp_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double,
                                                      C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                                      C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_distance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_shade_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                                                C.c_void_p]
    lib.bodyfit_raster_sample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_double,
                                                 C.c_double, C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_last_bins.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.bodyfit_raster_edges_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_double,
                                                C.c_double, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_edge_blend_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_void_p]
    lib.bodyfit_raster_edge_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double,
                                                    C.c_double, C.c_double, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_interp_rows_indexed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double,
                                                              C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                                              C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int,
                                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                              C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_texture_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int,
                                                  C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_texture_grad_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
    lib.bodyfit_texture_mip_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.bodyfit_raster_texture_mip_build_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                            C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_raster_texture_mip_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                                      C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.POINTER(C.c_float),
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_texture_mip_grad_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                           C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                           C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                                           C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_raster_light_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_light_grad_layout.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                              C.POINTER(C.c_longlong)]
    lib.bodyfit_raster_light_grad_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                                     C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_surface_vertex_normals_vjp_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p,
                                                              C.c_longlong, C.c_void_p]
    lib.bodyfit_volume_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_void_p)]
    lib.bodyfit_volume_destroy.argtypes = [C.c_void_p]
    lib.bodyfit_volume_destroy.restype = None
    lib.bodyfit_volume_sample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p,
                                                 C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_volume_integrate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(C.c_double), C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.bodyfit_volume_surface_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    lib.bodyfit_volume_surface_count_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float,
                                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bodyfit_volume_surface_emit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float,
                                                       C.c_float, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
    lib.bodyfit_volume_distance_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    lib.bodyfit_volume_distance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise BodyfitError(f"bodyfit status {rc}: {load_library().bodyfit_last_error().decode()}")


def _background4(background):
    """a float (every channel) or up to four floats as the host float[4] the lookups take"""
    bg = np.zeros(4, np.float32)
    b = np.atleast_1d(np.asarray(background, np.float32))
    if b.ndim != 1 or b.shape[0] > 4:
        raise ValueError("background is a float or up to four floats")
    bg[:4 if b.shape[0] == 1 else b.shape[0]] = b
    return bg


TX_MAX_LEVELS = 15          # BODYFIT_TX_MAX_LEVELS


def texture_mip_layout(tex_height: int, tex_width: int, max_level: int = -1):
    """bodyfit_texture_mip_layout (host only): (n_levels, [(H_l, W_l)], [the texel offset of level l in the packed buffer of the
    levels 1 .. n_levels - 1; entry 0 is 0 and not used], that buffer's texels)"""
    n, total = C.c_int(0), C.c_longlong(0)
    hs, ws, off = (C.c_int * TX_MAX_LEVELS)(), (C.c_int * TX_MAX_LEVELS)(), (C.c_longlong * TX_MAX_LEVELS)()
    _check(load_library().bodyfit_texture_mip_layout(int(tex_height), int(tex_width), int(max_level), C.byref(n), hs, ws, off,
                                                     C.byref(total)))
    k = n.value
    return k, [(hs[l], ws[l]) for l in range(k)], [off[l] for l in range(k)], total.value


def light_grad_layout(pixels_per_frame: int, n_channels: int, n_frames: int):
    """bodyfit_light_grad_layout (host only): (the pixels of a chunk of light_grad_device's reduction, the chunks per frame, the
    f64 elements of its workspace)"""
    chunk, n, work = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
    _check(load_library().bodyfit_light_grad_layout(int(pixels_per_frame), int(n_channels), int(n_frames), C.byref(chunk),
                                                    C.byref(n), C.byref(work)))
    return chunk.value, n.value, work.value


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _c32i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def device_count() -> int:
    return load_library().bodyfit_device_count()


# ------------------------------------------------------------------------------------------------
# reference-side value types
# ------------------------------------------------------------------------------------------------
@dataclass
class PixelKP:  # include/Sim3BA.h:9
    jid: int
    u: float
    v: float


@dataclass
class Sim3Params:  # include/Sim3BA.h:11-19   data = [s, aa(3), t(3)]
    data: np.ndarray = field(default_factory=lambda: np.array([1.0, 0, 0, 0, 0, 0, 3.0]))

    @property
    def scale(self):
        return self.data[0]

    @property
    def aa_root(self):
        return self.data[1:4]

    @property
    def trans(self):
        return self.data[4:7]


@dataclass
class FramePoseParams:  # include/MultiFrameBA.h:9-14
    scale: float = 1.0
    rootAA: np.ndarray = field(default_factory=lambda: np.zeros(3))
    rootT: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, 3.0]))
    jointAA: np.ndarray = field(default_factory=lambda: np.zeros((24, 3)))  # index 0 unused

    def pack(self) -> np.ndarray:
        return np.concatenate([[self.scale], self.rootAA, self.rootT, self.jointAA[1:].reshape(-1)])

    @staticmethod
    def unpack(x) -> "FramePoseParams":
        j = np.zeros((24, 3))
        j[1:] = np.asarray(x[7:]).reshape(-1, 3)
        return FramePoseParams(float(x[0]), np.array(x[1:4]), np.array(x[4:7]), j)


class Model:
    """Device-resident SMPL model (ark::AvatarModel stand-in)."""

    def __init__(self, m, device: int = 0, pose_blend_data: bool = True):
        lib = load_library()
        self._keep = [_c64(m.v_template), _c64(m.shapedirs), _c64(m.posedirs) if pose_blend_data else None,
                      _c64(m.j_regressor), _c64(m.weights), _c32i(m.parent), _c32i(m.landmark_vid)]
        k = self._keep
        self.n_verts, self.n_joints, self.n_shape = m.v_template.shape[0], len(m.parent), m.shapedirs.shape[2]
        self.n_landmarks = len(m.landmark_vid)
        self.n_kp_regressors = getattr(m, "n_kp_regressors", 0)
        if self.n_kp_regressors:
            self._keep += [_c32i(m.kpreg_offset), _c32i(m.kpreg_vid), _c64(m.kpreg_weight)]
            reg = (self.n_kp_regressors, _i(self._keep[-3]), _i(self._keep[-2]), _d(self._keep[-1]))
        else:
            reg = (0, None, None, None)
        desc = _ModelDesc(self.n_verts, self.n_joints, self.n_shape, m.posedirs.shape[2] if pose_blend_data else 0,
                          _d(k[0]), _d(k[1]), _d(k[2]), _d(k[3]), _d(k[4]), _i(k[5]), self.n_landmarks, _i(k[6]), *reg)
        h = C.c_void_p()
        _check(lib.bodyfit_model_create(C.byref(desc), device, C.byref(h)))
        self.h = h
        self.device = device

    def derived(self):
        J0 = np.empty((self.n_joints, 3)); S = np.empty((3 * self.n_joints, self.n_shape))
        off = np.empty((self.n_joints, 3))
        _check(load_library().bodyfit_model_get_derived(self.h, _d(J0), _d(S), _d(off)))
        return J0, S, off

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Gmm:
    """Device-resident max-mixture pose prior (ark::GaussianMixture stand-in)."""

    def __init__(self, weights, means, covs, resid_scale=np.sqrt(0.5), device: int = 0):
        self.K, self.D = means.shape
        w, mu, cv = _c64(weights), _c64(means), _c64(covs)
        h = C.c_void_p()
        _check(load_library().bodyfit_gmm_create(self.K, self.D, _d(w), _d(mu), _d(cv), resid_scale, device, C.byref(h)))
        self.h = h

    def get(self):
        L = np.empty((self.K, self.D, self.D)); nlw = np.empty(self.K)
        _check(load_library().bodyfit_gmm_get(self.h, _d(L), _d(nlw)))
        return L, nlw

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_gmm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Problem:
    """The residual blocks of one solve (what the reference adds to its ceres::Problem)."""

    def __init__(self, model: Model, kp_offset, kp_id, kp_uv, intr, R0, n_cols=86, use_shape=True,
                 beta_per_frame=False, pose_blend=True, beta_pose=0.0, gmm: Gmm | None = None, beta_shape=0.0,
                 lambda_temporal=0.0, temporal_halo=False, huber_delta=3.0, want_mesh=False):
        lib = load_library()
        self.model = model
        self.gmm = gmm
        ko, ki, ku, r0 = _c32i(kp_offset), _c32i(kp_id), _c64(kp_uv), _c64(R0)
        self.n_frames = len(ko) - 1
        desc = _ProblemDesc(self.n_frames, _i(ko), _i(ki), _d(ku), float(intr[0]), float(intr[1]), float(intr[2]),
                            float(intr[3]), _d(r0), int(n_cols), int(use_shape), int(beta_per_frame),
                            int(pose_blend), float(beta_pose), gmm.h if gmm is not None else None,
                            float(beta_shape), float(lambda_temporal), int(temporal_halo), float(huber_delta),
                            int(want_mesh))
        h = C.c_void_p()
        _check(lib.bodyfit_problem_create(model.h, C.byref(desc), C.byref(h)))
        self.h = h
        self.layout = Layout()
        _check(lib.bodyfit_problem_layout(self.h, C.byref(self.layout)))
        self.n_cols = n_cols
        self.want_mesh = want_mesh
        self.beta_per_frame = bool(beta_per_frame)
        self.n_param_rows = self.n_frames + (1 if temporal_halo else 0)
        self.n_frame_params = 7 + 3 * (model.n_joints - 1)   # 76 for SMPL's 24 joints
        self.huber_delta = float(huber_delta)
        # bumped by every call that sweeps or solves into the problem's buffers: torch_layer.FitObjective reuses the Jacobian of
        # its forward in its backward only if nothing else ran on the problem in between
        self.generation = 0

    @classmethod
    def from_sequence(cls, model: Model, seq, **kw):
        return cls(model, seq.kp_offset, seq.kp_id, seq.kp_uv, seq.intr, seq.R0, **kw)

    def evaluate(self, frame_params, beta=None, want_jacobian=True):
        self.generation += 1
        L = self.layout
        x = _c64(frame_params); b = _c64(beta) if beta is not None else None
        assert x.size == self.n_param_rows * self.n_frame_params, "frame_params must be [F(+1), 7 + 3 (n_joints - 1)]"
        r = np.empty(L.total_rows); comp = np.zeros(self.n_frames, np.int32)
        J = np.empty((L.reproj_rows, L.n_cols)) if want_jacobian else None
        _check(load_library().bodyfit_evaluate_batch(self.h, _d(x), _d(b), _d(r), _d(J), _i(comp), int(want_jacobian)))
        return r, J, comp

    def evaluate_device(self, d_params_ptr: int, d_beta_ptr: int | None, want_jacobian=True, stream: int | None = None):
        self.generation += 1
        _check(load_library().bodyfit_evaluate_device(self.h, d_params_ptr, d_beta_ptr, int(want_jacobian), stream))

    def reduce_shared_device(self, d_out_ptr: int | None = None, stream: int | None = None):
        _check(load_library().bodyfit_reduce_shared_device(self.h, d_out_ptr, stream))

    def sweep_status(self, stream: int | None = None):
        """Waits for `stream`; raises if an asynchronous one-launch sweep since the last check left its cloud incomplete
        (bodyfit_sweep_status: the problem then uses the two-launch sweep, so evaluating again gives the whole result)."""
        _check(load_library().bodyfit_sweep_status(self.h, stream))

    def sweep_timeouts(self) -> int:
        """one-launch sweeps of this problem found incomplete since it was created (bodyfit_sweep_timeouts); 0 in a healthy run"""
        return int(load_library().bodyfit_sweep_timeouts(self.h))

    def set_exchange_timeout(self, seconds: float):
        """bound on every exchange / status read of this problem's sharded solves (bodyfit_set_exchange_timeout; 0: none)"""
        _check(load_library().bodyfit_set_exchange_timeout(self.h, float(seconds)))

    def set_shard_proxy(self, n_ranks: int, rank: int = 0):
        """measurement aid (bodyfit_set_shard_proxy): sharded solves through a one-rank communicator run as `rank` of `n_ranks`
        identical shards; n_ranks <= 1 switches it off"""
        _check(load_library().bodyfit_set_shard_proxy(self.h, int(n_ranks), int(rank)))

    def arm_shared_reduction(self, d_out_ptr: int | None):
        """Following Jacobian sweeps deposit [cost | g_beta | H_bb] in d_out_ptr at their own tail when they can (one-launch
        sweep, shared beta, <= 256 frames + prior tiles); reduce_shared_device(d_out_ptr) then launches nothing.  None disarms."""
        _check(load_library().bodyfit_arm_shared_reduction(self.h, d_out_ptr))

    def profile_sweep(self, d_params_ptr, d_beta_ptr, want_jacobian=True, with_reduce=False, iters=50, stream=None):
        self.generation += 1
        ms = np.zeros(5)
        _check(load_library().bodyfit_profile_sweep(self.h, d_params_ptr, d_beta_ptr, int(want_jacobian),
                                                    int(with_reduce), int(iters), stream, _d(ms)))
        # (the prior workgroups ride on one of the launches; sweep_roles != 0: the sweep was ONE launch)
        return dict(frame_resjac=ms[0], mesh_blend_lbs=ms[2], reduce_shared=ms[3], sweep_roles=ms[4])

    def views(self) -> DeviceViews:
        v = DeviceViews()
        _check(load_library().bodyfit_problem_views(self.h, C.byref(v)))
        return v

    def _offsets(self, offsets):
        """Host offsets [V, 3] (shared by the frames) or [F, V, 3] as (contiguous f32 array, frame stride in floats)."""
        o = np.ascontiguousarray(offsets, dtype=np.float32)
        V = self.model.n_verts
        if o.shape == (V, 3):
            return o, 0
        if o.shape == (self.n_frames, V, 3):
            return o, 3 * V
        raise ValueError(f"offsets must be [V, 3] or [F, V, 3], got {o.shape}")

    def forward(self, frame_params, beta=None, want_cloud=True, offsets=None):
        """Joints [F, nJ, 3] f64 and cloud [F, V, 3] f32 (bodyfit_forward).  offsets: per-vertex displacements [V, 3] or
        [F, V, 3] f32 added to the blended rest vertices before skinning (bodyfit_forward_offsets; the joints do not move)."""
        self.generation += 1
        x = _c64(frame_params); b = _c64(beta) if beta is not None else None
        assert x.size >= self.n_param_rows * self.n_frame_params, "frame_params must be [F(+1), 7 + 3 (n_joints - 1)]"
        joints = np.empty((self.n_frames, self.model.n_joints, 3))
        cloud = np.empty((self.n_frames, self.model.n_verts, 3), np.float32) if want_cloud else None
        cp = cloud.ctypes.data_as(_fp) if cloud is not None else None
        if offsets is None:
            _check(load_library().bodyfit_forward(self.h, _d(x), _d(b), _d(joints), cp))
        else:
            o, stride = self._offsets(offsets)
            _check(load_library().bodyfit_forward_offsets(self.h, _d(x), _d(b), o.ctypes.data_as(_fp), stride, _d(joints), cp))
        return joints, cloud

    def forward_device(self, d_params_ptr: int, d_beta_ptr: int | None, d_joints_ptr: int | None, d_cloud_ptr: int | None,
                       cloud_row_floats: int | None = None, stream: int | None = None, d_offsets_ptr: int | None = None,
                       offsets_frame_stride: int = 0):
        """bodyfit_forward_device: the two-launch forward into device memory, asynchronous on `stream`.  d_offsets_ptr: f32
        per-vertex offsets, [V, 3] (offsets_frame_stride 0) or rows of offsets_frame_stride floats per frame
        (bodyfit_forward_offsets_device)."""
        self.generation += 1
        rf = 3 * self.model.n_verts if cloud_row_floats is None else int(cloud_row_floats)
        if d_offsets_ptr is None:
            _check(load_library().bodyfit_forward_device(self.h, d_params_ptr, d_beta_ptr, d_joints_ptr, d_cloud_ptr, rf, stream))
        else:
            _check(load_library().bodyfit_forward_offsets_device(self.h, d_params_ptr, d_beta_ptr, d_offsets_ptr,
                                                                 int(offsets_frame_stride), d_joints_ptr, d_cloud_ptr, rf, stream))

    def forward_vjp(self, frame_params, beta=None, grad_cloud=None, grad_joints=None, offsets=None):
        """dL/dframe_params [F(+1), 7 + 3 (nJ - 1)] (76 for 24 joints) and dL/dbeta ([nS] shared, [F, nS] per frame; None
        without the shape block) of the forward, given dL/dcloud [F, V, 3] and / or dL/djoints [F, nJ, 3] (bodyfit_forward_vjp).
        With offsets ([V, 3] or [F, V, 3]) the forward is the displaced one and a third result is dL/doffsets, f32 in the shape
        of offsets (zeros without grad_cloud: the joints do not depend on the offsets; bodyfit_forward_offsets_vjp)."""
        x = _c64(frame_params); b = _c64(beta) if beta is not None else None
        assert x.size == self.n_param_rows * self.n_frame_params, "frame_params must be [F(+1), 7 + 3 (n_joints - 1)]"
        G = None if grad_cloud is None else np.ascontiguousarray(grad_cloud, dtype=np.float32)
        H = None if grad_joints is None else _c64(grad_joints)
        if G is not None:
            assert G.size == self.n_frames * self.model.n_verts * 3, "grad_cloud must be [F, V, 3]"
        if H is not None:
            assert H.size == self.n_frames * self.model.n_joints * 3, "grad_joints must be [F, nJ, 3]"
        gx = np.empty((self.n_param_rows, self.n_frame_params))
        has_beta = self.n_cols > self.n_frame_params
        gb = None
        if has_beta:
            gb = np.empty((self.n_frames, self.model.n_shape)) if self.beta_per_frame else np.empty(self.model.n_shape)
        Gp = G.ctypes.data_as(_fp) if G is not None else None
        if offsets is None:
            _check(load_library().bodyfit_forward_vjp(self.h, _d(x), _d(b), Gp, _d(H), _d(gx), _d(gb)))
            return gx, gb
        o, stride = self._offsets(offsets)
        go = np.zeros_like(o)
        _check(load_library().bodyfit_forward_offsets_vjp(self.h, _d(x), _d(b), o.ctypes.data_as(_fp), stride, Gp, _d(H), _d(gx),
                                                          _d(gb), go.ctypes.data_as(_fp) if G is not None else None))
        return gx, gb, go

    def forward_vjp_device(self, d_params_ptr: int, d_beta_ptr: int | None, d_grad_cloud_ptr: int | None,
                           d_grad_joints_ptr: int | None, d_grad_params_ptr: int, d_grad_beta_ptr: int | None,
                           grad_cloud_row_floats: int | None = None, stream: int | None = None,
                           d_offsets_ptr: int | None = None, offsets_frame_stride: int = 0, d_grad_offsets_ptr: int | None = None):
        """bodyfit_forward_vjp_device: asynchronous on `stream`, device pointers throughout.  d_offsets_ptr /
        offsets_frame_stride as forward_device; d_grad_offsets_ptr: f32 dL/doffsets in the layout of the offsets, or None
        (bodyfit_forward_offsets_vjp_device)."""
        rf = 3 * self.model.n_verts if grad_cloud_row_floats is None else int(grad_cloud_row_floats)
        if d_offsets_ptr is None and d_grad_offsets_ptr is None:
            _check(load_library().bodyfit_forward_vjp_device(self.h, d_params_ptr, d_beta_ptr, d_grad_cloud_ptr, rf,
                                                             d_grad_joints_ptr, d_grad_params_ptr, d_grad_beta_ptr, stream))
        else:
            _check(load_library().bodyfit_forward_offsets_vjp_device(self.h, d_params_ptr, d_beta_ptr, d_offsets_ptr,
                                                                     int(offsets_frame_stride), d_grad_cloud_ptr, rf,
                                                                     d_grad_joints_ptr, d_grad_params_ptr, d_grad_beta_ptr,
                                                                     d_grad_offsets_ptr, stream))

    def forward_jvp(self, frame_params, beta, tan_x, tan_beta=None, want_cloud=True):
        """Forward-mode tangents of the forward (bodyfit_forward_jvp): tan_x [F, K, 7 + 3 (nJ - 1)] (or None = 0) and tan_beta
        ([K, nS] for a shared beta, [F, K, nS] per frame; None = 0) give (tan_joints [F, K, nJ, 3] f64, tan_cloud [F, K, V, 3]
        f32 or None), the directional derivatives of forward()'s joints and cloud along each of the K tangents."""
        x = _c64(frame_params); b = _c64(beta) if beta is not None else None
        assert x.size >= self.n_param_rows * self.n_frame_params, "frame_params must be [F(+1), 7 + 3 (n_joints - 1)]"
        F, nS = self.n_frames, self.model.n_shape
        tx = _c64(tan_x) if tan_x is not None else None
        tb = _c64(tan_beta) if tan_beta is not None else None
        assert tx is not None or tb is not None, "give tan_x or tan_beta"
        if tx is not None:
            assert tx.ndim == 3 and tx.shape[0] == F and tx.shape[2] == self.n_frame_params, "tan_x must be [F, K, n_frame_params]"
            K = tx.shape[1]
        else:
            K = tb.shape[-2]
        if tb is not None:
            want = (F, K, nS) if self.beta_per_frame else (K, nS)
            assert tb.shape == want, f"tan_beta must be {list(want)}"
        joints = np.empty((F, K, self.model.n_joints, 3))
        cloud = np.empty((F, K, self.model.n_verts, 3), np.float32) if want_cloud else None
        _check(load_library().bodyfit_forward_jvp(self.h, _d(x), _d(b), K, _d(tx), _d(tb), _d(joints),
                                                  cloud.ctypes.data_as(_fp) if cloud is not None else None))
        return joints, cloud

    def forward_jvp_device(self, d_params_ptr: int, d_beta_ptr: int | None, n_tangents: int, d_tan_params_ptr: int | None,
                           d_tan_beta_ptr: int | None, d_tan_joints_ptr: int | None, d_tan_cloud_ptr: int | None,
                           row_floats: int | None = None, stream: int | None = None, d_offsets_ptr: int | None = None,
                           offsets_frame_stride: int = 0):
        """bodyfit_forward_jvp_device: asynchronous on `stream`, device pointers throughout.  d_offsets_ptr /
        offsets_frame_stride as forward_device: the tangents are taken at the displaced point, the offsets themselves are
        constants (bodyfit_forward_offsets_jvp_device)."""
        rf = 3 * self.model.n_verts if row_floats is None else int(row_floats)
        if d_offsets_ptr is None:
            _check(load_library().bodyfit_forward_jvp_device(self.h, d_params_ptr, d_beta_ptr, int(n_tangents), d_tan_params_ptr,
                                                             d_tan_beta_ptr, d_tan_joints_ptr, d_tan_cloud_ptr, rf, stream))
        else:
            _check(load_library().bodyfit_forward_offsets_jvp_device(self.h, d_params_ptr, d_beta_ptr, d_offsets_ptr,
                                                                     int(offsets_frame_stride), int(n_tangents), d_tan_params_ptr,
                                                                     d_tan_beta_ptr, d_tan_joints_ptr, d_tan_cloud_ptr, rf, stream))

    def residuals_device(self, d_params_ptr: int, d_beta_ptr: int | None, d_residuals_ptr: int, d_comp_ptr: int | None = None,
                         keep_jacobian=False, stream: int | None = None):
        """bodyfit_residuals_device: the residual vector [total_rows] f64 (and the GMM components [F] int32) into device memory,
        asynchronous on `stream`; keep_jacobian also leaves the Jacobian for residual_vjp_device(..., reuse_jacobian=True)."""
        self.generation += 1
        _check(load_library().bodyfit_residuals_device(self.h, d_params_ptr, d_beta_ptr, d_residuals_ptr, d_comp_ptr,
                                                       int(keep_jacobian), stream))

    def residual_vjp_device(self, d_params_ptr: int, d_beta_ptr: int | None, d_grad_r_ptr: int, d_grad_params_ptr: int,
                            d_grad_beta_ptr: int | None, reuse_jacobian=False, stream: int | None = None):
        """bodyfit_residual_vjp_device: (dr/dx)^T g and (dr/dbeta)^T g of the whole residual vector, asynchronous on `stream`.
        reuse_jacobian: use the Jacobian of the problem's last sweep (residuals_device with keep_jacobian at this point)."""
        if not reuse_jacobian:
            self.generation += 1
        _check(load_library().bodyfit_residual_vjp_device(self.h, d_params_ptr, d_beta_ptr, d_grad_r_ptr, d_grad_params_ptr,
                                                          d_grad_beta_ptr, int(bool(reuse_jacobian)), stream))

    def residual_vjp(self, frame_params, beta, grad_r):
        """(dr/dframe_params)^T g [F(+1), 7 + 3 (nJ - 1)] and (dr/dbeta)^T g ([nS] shared, [F, nS] per frame; None without the
        shape block) of the whole residual vector r [total_rows] at (frame_params, beta), g = grad_r (bodyfit_residual_vjp)."""
        self.generation += 1
        x = _c64(frame_params); b = _c64(beta) if beta is not None else None
        g = _c64(grad_r)
        assert x.size == self.n_param_rows * self.n_frame_params, "frame_params must be [F(+1), 7 + 3 (n_joints - 1)]"
        assert g.size == self.layout.total_rows, "grad_r must be [total_rows]"
        gx = np.empty((self.n_param_rows, self.n_frame_params))
        gb = None
        if self.n_cols > self.n_frame_params:
            gb = np.empty((self.n_frames, self.model.n_shape)) if self.beta_per_frame else np.empty(self.model.n_shape)
        _check(load_library().bodyfit_residual_vjp(self.h, _d(x), _d(b), _d(g), _d(gx), _d(gb)))
        return gx, gb

    def writeback(self, frame_params, beta=None, want_cloud=False):
        """The reference's post-solve write-back for every frame, on the device (bodyfit_writeback_batch):
        R0' = R(rootAA) R0, update() without the Sim3 scale, mean pixel error of the FK keypoints."""
        self.generation += 1
        x = _c64(frame_params); b = _c64(beta) if beta is not None else None
        F = self.n_frames
        r0 = np.empty((F, 3, 3)); joints = np.empty((F, self.model.n_joints, 3)); px = np.empty(F)
        cloud = np.empty((F, self.model.n_verts, 3), np.float32) if want_cloud else None
        _check(load_library().bodyfit_writeback_batch(self.h, _d(x), _d(b), _d(r0), _d(joints),
                                                      cloud.ctypes.data_as(_fp) if cloud is not None else None, _d(px)))
        return dict(R0=r0, joints=joints, cloud=cloud, mean_px=px)

    def solve(self, frame_params, beta=None, constant=None, independent=False, max_iters=100, scale_bounds=(0.3, 3.0),
              verbose=False, solver=0):
        """Ceres-like LM over this problem (bodyfit_solve).  Returns fitted params, beta, [FitSummary]."""
        self.generation += 1
        x = _c64(frame_params).copy()
        b = _c64(beta).copy() if beta is not None else None
        cst = None
        if constant is not None:
            cst = np.ascontiguousarray(constant, dtype=np.uint8)
        n_sum = self.n_frames if independent else 1
        sums = (FitSummary * n_sum)()
        opt = FitOptions(int(max_iters), float(scale_bounds[0]), float(scale_bounds[1]), int(verbose), int(solver))
        _check(load_library().bodyfit_solve(self.h, _d(x), _d(b), cst.ctypes.data_as(C.POINTER(C.c_ubyte)) if cst is not None else None,
                                            int(independent), C.byref(opt), sums, n_sum))
        return x, b, list(sums)

    def _solve_shard(self, call, frame_params, beta, constant, max_iters, scale_bounds, verbose):
        """Marshalling of the two sharded solves: call(x, beta, constant, options, summary) is the ABI function with its
        communicator bound."""
        self.generation += 1
        x = _c64(frame_params).copy()
        b = _c64(beta).copy()
        npf = self.n_frame_params
        assert x.size == self.n_param_rows * npf
        cst = np.ascontiguousarray(constant, dtype=np.uint8) if constant is not None else None
        summ = FitSummary()
        opt = FitOptions(int(max_iters), float(scale_bounds[0]), float(scale_bounds[1]), int(verbose), 3)
        _check(call(_d(x), _d(b), cst.ctypes.data_as(C.POINTER(C.c_ubyte)) if cst is not None else None, C.byref(opt),
                    C.byref(summ)))
        return x.reshape(-1)[:self.n_frames * npf].reshape(self.n_frames, npf).copy(), b, summ

    def solve_sharded(self, frame_params, beta, comm: "Comm", constant=None, max_iters=100, scale_bounds=(-1e300, 1e300),
                      verbose=False):
        """This rank's shard of one window (bodyfit_solve_sharded).  frame_params: the shard's rows (+ the halo row when the
        problem has one).  Returns the shard's fitted rows, beta (the same on every rank) and the FitSummary."""
        lib = load_library()
        return self._solve_shard(lambda x, b, c, o, s: lib.bodyfit_solve_sharded(self.h, x, b, c, C.byref(comm), o, s),
                                 frame_params, beta, constant, max_iters, scale_bounds, verbose)

    def solve_sharded_rccl(self, frame_params, beta, comm: "Rccl", constant=None, max_iters=100,
                           scale_bounds=(-1e300, 1e300), verbose=False):
        """This rank's shard of one window with the exchanges as RCCL all-gathers on the solve's device buffers and stream
        (bodyfit_solve_sharded_rccl)."""
        lib = load_library()
        return self._solve_shard(lambda x, b, c, o, s: lib.bodyfit_solve_sharded_rccl(self.h, x, b, c, comm.h, o, s),
                                 frame_params, beta, constant, max_iters, scale_bounds, verbose)

    def last_exchange_count(self) -> int:
        """all-gathers issued by the last sharded solve of this problem"""
        return int(load_library().bodyfit_last_exchange_count(self.h))

    def cache_sweep(self, params, beta=None):
        """One sweep kept in the problem's host cache for evaluate_block (what bodyfit_ceres::SweepCallback does): no caller
        buffers, so only the structurally non-zero Jacobian column blocks cross PCIe."""
        self.generation += 1
        x = _c64(params)
        b = _c64(beta) if beta is not None else None
        _check(load_library().bodyfit_evaluate_batch(self.h, _d(x), _d(b) if b is not None else None, None, None, None, 1))

    def evaluate_block(self, kind: int, index: int, blocks: list[np.ndarray], n_res: int, want=None):
        """ceres::CostFunction::Evaluate on one block.  `want[b]` False -> jacobians[b] = NULL."""
        self.generation += 1
        blocks = [_c64(b) for b in blocks]
        nb = len(blocks)
        params = (_dp * nb)(*[_d(b) for b in blocks])
        r = np.empty(n_res)
        jacs = [np.full((n_res, len(b)), np.nan) for b in blocks]
        if want is None:
            want = [True] * nb
        jp = (_dp * nb)(*[(_d(j) if w else None) for j, w in zip(jacs, want)])
        _check(load_library().bodyfit_evaluate_block(self.h, kind, index, params, _d(r), jp))
        return r, jacs

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClosestPoints:
    """Closest points between two per-frame point sets on the device, and the gradient of the squared distances with the
    correspondence held fixed (bodyfit_closest_*, csrc/k_closest.hip).  The handle owns the workspace of both calls; calls on
    one handle must be ordered (one stream, or events)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(load_library().bodyfit_closest_create(int(device), C.byref(h)))
        self.h = h
        self.device = device

    def points_device(self, query: PointSet, ref: PointSet, n_frames: int, n_query_total: int, n_ref_total: int,
                      d_dist2_ptr: int, d_index_ptr: int, stream: int | None = None, prepare_vjp: bool = False):
        """bodyfit_closest_points_device: dist2 [N] f32 and frame-local index [N] int32 (-1: none) of every query row,
        asynchronous on `stream`.  n_query_total / n_ref_total: row counts of ragged sets (ignored for uniform ones).
        prepare_vjp: also group the queries by reference row for a points_vjp_device call with this index (kept in the handle)."""
        _check(load_library().bodyfit_closest_points_device(self.h, C.byref(query), C.byref(ref), int(n_frames),
                                                            int(n_query_total), int(n_ref_total), d_dist2_ptr, d_index_ptr,
                                                            int(bool(prepare_vjp)), stream))

    def points_vjp_device(self, query: PointSet, ref: PointSet, n_frames: int, n_query_total: int, n_ref_total: int,
                          d_index_ptr: int, d_grad_dist2_ptr: int, d_grad_query_ptr: int | None, d_grad_ref_ptr: int | None,
                          stream: int | None = None):
        """bodyfit_closest_points_vjp_device: dL/dquery and dL/dref (each in the layout of its set; either may be None) given
        dL/ddist2 [N] and the index of points_device, asynchronous on `stream`."""
        _check(load_library().bodyfit_closest_points_vjp_device(self.h, C.byref(query), C.byref(ref), int(n_frames),
                                                                int(n_query_total), int(n_ref_total), d_index_ptr,
                                                                d_grad_dist2_ptr, d_grad_query_ptr, d_grad_ref_ptr, stream))

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_closest_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Surface:
    """Closest point on the triangles of a posed mesh for every query point, and the gradient of the squared distances at the
    fixed correspondence (bodyfit_surface_*, bodyfit_closest_surface_*, csrc/k_closest_surface.hip); the winding number of the
    mesh about a point and its vertex normals (csrc/k_winding.hip).  The handle holds one
    topology (faces: int32 [n_faces, 3] with ids in [0, n_verts)) and the workspace of both calls; calls on one handle must be
    ordered (one stream, or events)."""

    def __init__(self, device: int, n_verts: int, faces):
        f = np.asarray(faces)
        if f.dtype.kind not in "iu":
            raise TypeError("faces must be an integer array")
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"faces must be [n_faces, 3], got {f.shape}")
        f = np.ascontiguousarray(f, dtype=np.int32)
        h = C.c_void_p()
        _check(load_library().bodyfit_surface_create(int(device), int(n_verts), int(f.shape[0]),
                                                     f.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)))
        self.h = h
        self.device = device
        self.n_verts = int(n_verts)
        self.n_faces = int(f.shape[0])

    def closest_device(self, query: PointSet, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, n_query_total: int,
                       d_dist2_ptr: int, d_index_ptr: int, d_bary_ptr: int, stream: int | None = None,
                       prepare_vjp: bool = False):
        """bodyfit_closest_surface_device: dist2 [N] f32, frame-local triangle index [N] int32 (-1: none) and barycentric
        weights [N, 3] f32 of every query row, asynchronous on `stream`.  prepare_vjp: also group the queries by face for a
        vjp_device call with this index (kept in the handle)."""
        _check(load_library().bodyfit_closest_surface_device(self.h, C.byref(query), d_verts_ptr, int(verts_frame_stride),
                                                             int(n_frames), int(n_query_total), d_dist2_ptr, d_index_ptr,
                                                             d_bary_ptr, int(bool(prepare_vjp)), stream))

    def closest_oriented_device(self, query: PointSet, d_normals_ptr: int, min_cos: float, d_verts_ptr: int,
                                verts_frame_stride: int, n_frames: int, n_query_total: int, d_dist2_ptr: int, d_index_ptr: int,
                                d_bary_ptr: int, stream: int | None = None, prepare_vjp: bool = False):
        """bodyfit_closest_surface_oriented_device: closest_device over the triangles whose face normal n (orientation of
        `faces`) has n . m >= min_cos, m the direction of the query row (d_normals_ptr: [N, 3] f32, packed like dist2 whatever
        the layout of `query`).  A row without a compatible triangle gets -1, +inf, 0.  vjp_device takes the result as it takes
        closest_device's."""
        _check(load_library().bodyfit_closest_surface_oriented_device(self.h, C.byref(query), d_normals_ptr, float(min_cos),
                                                                      d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                                      int(n_query_total), d_dist2_ptr, d_index_ptr, d_bary_ptr,
                                                                      int(bool(prepare_vjp)), stream))

    def vjp_device(self, query: PointSet, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, n_query_total: int,
                   d_index_ptr: int, d_bary_ptr: int, d_grad_dist2_ptr: int, d_grad_query_ptr: int | None,
                   d_grad_verts_ptr: int | None, stream: int | None = None):
        """bodyfit_closest_surface_vjp_device: dL/dquery (layout of the query set) and dL/dverts (layout of the vertices; either
        may be None) given dL/ddist2 [N] and the index and weights of closest_device, asynchronous on `stream`."""
        _check(load_library().bodyfit_closest_surface_vjp_device(self.h, C.byref(query), d_verts_ptr, int(verts_frame_stride),
                                                                 int(n_frames), int(n_query_total), d_index_ptr, d_bary_ptr,
                                                                 d_grad_dist2_ptr, d_grad_query_ptr, d_grad_verts_ptr, stream))

    def rows_vjp_device(self, rows: PointSet, n_frames: int, n_rows_total: int, d_index_ptr: int, d_bary_ptr: int,
                        d_coef_ptr: int, d_dir_ptr: int, d_gverts_ptr: int, gverts_frame_stride: int,
                        stream: int | None = None):
        """bodyfit_surface_rows_vjp_device: gverts [F, n_verts, 3] f32 (gverts_frame_stride floats between frames) = sum over the
        rows of coef_i bary_ia dir_i at corner a of face index_i; index [N] int32 (-1: nothing), bary [N, 3], coef [N], dir
        [N, 3] f32, the rows' frame structure from `rows` (its d_xyz is not read).  Deterministic, asynchronous on `stream`."""
        _check(load_library().bodyfit_surface_rows_vjp_device(self.h, C.byref(rows), int(n_frames), int(n_rows_total), d_index_ptr,
                                                              d_bary_ptr, d_coef_ptr, d_dir_ptr, d_gverts_ptr,
                                                              int(gverts_frame_stride), stream))

    def winding_device(self, query: PointSet, d_skip_vertex_ptr: int | None, d_verts_ptr: int, verts_frame_stride: int,
                       n_frames: int, n_query_total: int, d_winding_ptr: int, stream: int | None = None):
        """bodyfit_surface_winding_device: the winding number w [N] f32 of every query row about its frame's posed mesh (0
        outside a closed, outward oriented mesh, 1 inside), asynchronous on `stream`.  d_skip_vertex_ptr: None, or int32 [N]
        packed like w: row i leaves out the faces that have that vertex id among their corners (-1: none)."""
        _check(load_library().bodyfit_surface_winding_device(self.h, C.byref(query), d_skip_vertex_ptr, d_verts_ptr,
                                                             int(verts_frame_stride), int(n_frames), int(n_query_total),
                                                             d_winding_ptr, stream))

    def vertex_normals_device(self, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, d_normals_ptr: int,
                              stream: int | None = None):
        """bodyfit_surface_vertex_normals_device: the area-weighted unit vertex normals [F, n_verts, 3] f32 (dense) of the posed
        mesh, 0 for a vertex without a face or with a zero sum; deterministic, asynchronous on `stream`."""
        _check(load_library().bodyfit_surface_vertex_normals_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                                    d_normals_ptr, stream))

    def vertex_normals_vjp_device(self, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, d_grad_normals_ptr: int,
                                  d_grad_verts_ptr: int, grad_frame_stride: int, stream: int | None = None):
        """bodyfit_surface_vertex_normals_vjp_device: for grad_normals [F, n_verts, 3] f32 (dense) the gradient in the vertices
        through vertex_normals_device, [n_verts, 3] f32 per frame and grad_frame_stride floats apart: the exact adjoint at the
        f32 vertices, gathered in f64 in a fixed order (no atomics), 0 through a vertex whose normal the forward wrote as 0."""
        _check(load_library().bodyfit_surface_vertex_normals_vjp_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                                        d_grad_normals_ptr, d_grad_verts_ptr,
                                                                        int(grad_frame_stride), stream))

    def laplacian_device(self, d_field_ptr: int, field_stride: int, n_fields: int, d_out_ptr: int, transpose: bool = False,
                         stream: int | None = None):
        """bodyfit_surface_laplacian_device: the uniform mesh Laplacian l_i = x_i - mean over i's faces of the other two corners
        (0 for a vertex without a face) of n_fields per-vertex fields [n_verts, 3] f32, field_stride floats apart, into the dense
        [n_fields, n_verts, 3] f32 at d_out_ptr; transpose: the exact transpose.  Deterministic, asynchronous on `stream`."""
        _check(load_library().bodyfit_surface_laplacian_device(self.h, d_field_ptr, int(field_stride), int(n_fields),
                                                               int(bool(transpose)), d_out_ptr, stream))

    def gram_device(self, query: PointSet, n_frames: int, n_query_total: int, d_index_ptr: int, d_bary_ptr: int,
                    d_weight_ptr: int | None, d_direction_ptr: int | None, d_jac_ptr: int, n_tangents: int, row_floats: int,
                    jac_frame_stride: int, d_rhs_ptr: int | None, rhs_frame_stride: int, d_H_ptr: int, d_g_ptr: int | None,
                    stream: int | None = None):
        """bodyfit_surface_gram_device: the per-frame normal equations H [F, P, P] f64 = J^T W J (and g [F, P] f64 = J^T rhs) of
        the scan rows at the fixed (index, bary), from the dense vertex Jacobian [F, P, row_floats] f32; weight [N] f32 and
        direction [N, 3] f32 (point-to-plane) are optional, asynchronous on `stream`."""
        _check(load_library().bodyfit_surface_gram_device(self.h, C.byref(query), int(n_frames), int(n_query_total), d_index_ptr,
                                                          d_bary_ptr, d_weight_ptr, d_direction_ptr, d_jac_ptr, int(n_tangents),
                                                          int(row_floats), int(jac_frame_stride), d_rhs_ptr,
                                                          int(rhs_frame_stride), d_H_ptr, d_g_ptr, stream))

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_surface_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Overlay:
    """Mesh overlay on the device: smpl::render::renderSMPLMesh (include/RenderSMPLMesh.h:16-110) for a batch of
    frames.  `faces` are the model's triangles (AvatarModel::mesh, src/main_single_frame.cpp:185-188)."""

    def __init__(self, faces, n_vertices: int, width: int, height: int, max_frames: int = 1, device: int = 0):
        self.faces = _c32i(faces).reshape(-1, 3)
        self.n_vertices, self.width, self.height, self.max_frames = int(n_vertices), int(width), int(height), int(max_frames)
        d = _OverlayDesc(device, self.n_vertices, self.faces.shape[0], self.faces.ctypes.data_as(C.POINTER(C.c_int32)),
                         self.width, self.height, self.max_frames)
        h = C.c_void_p()
        _check(load_library().bodyfit_overlay_create(C.byref(d), C.byref(h)))
        self.h = h

    def render(self, cloud, images, intr, fill=True, backface_cull=True, wireframe=False):
        """cloud [F][V][3] float32 or float64 (camera coordinates), images [F][H][W][3] uint8, modified in place."""
        cloud = np.asarray(cloud)
        if cloud.dtype != np.float32:
            cloud = np.ascontiguousarray(cloud, dtype=np.float64)
        cloud = np.ascontiguousarray(cloud).reshape(-1, self.n_vertices, 3)
        F = cloud.shape[0]
        if not (isinstance(images, np.ndarray) and images.dtype == np.uint8 and images.flags.c_contiguous
                and images.size == F * self.height * self.width * 3):
            raise BodyfitError("Overlay.render: images must be a C-contiguous uint8 array [F][H][W][3]")
        _check(load_library().bodyfit_overlay_render(
            self.h, cloud.ctypes.data_as(C.c_void_p), int(cloud.dtype == np.float64), self.n_vertices * 3, F,
            images.ctypes.data_as(C.POINTER(C.c_uint8)), self.width * 3, self.width * 3 * self.height,
            float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]), int(fill), int(backface_cull), int(wireframe)))
        return images

    def render_device(self, d_cloud_ptr: int, cloud_is_f64: bool, cloud_frame_stride: int, n_frames: int, d_images_ptr: int,
                      intr, row_stride=None, frame_stride=None, fill=True, backface_cull=True, stream=None):
        rs = self.width * 3 if row_stride is None else int(row_stride)
        fs = rs * self.height if frame_stride is None else int(frame_stride)
        _check(load_library().bodyfit_overlay_render_device(
            self.h, d_cloud_ptr, int(cloud_is_f64), int(cloud_frame_stride), int(n_frames), d_images_ptr, rs, fs,
            float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]), int(fill), int(backface_cull), 0, stream))

    def drawlist(self, frame: int = 0):
        nf = self.faces.shape[0]
        face = np.zeros(nf, np.int32); pts = np.zeros((nf, 6), np.int32); gray = np.zeros(nf, np.int32)
        n = C.c_int(0)
        p32 = C.POINTER(C.c_int32)
        _check(load_library().bodyfit_overlay_drawlist(self.h, int(frame), C.byref(n), face.ctypes.data_as(p32),
                                                       pts.ctypes.data_as(p32), gray.ctypes.data_as(p32)))
        return face[:n.value], pts[:n.value], gray[:n.value]

    def last_timing(self):
        ms = (C.c_float * 4)()
        _check(load_library().bodyfit_overlay_last_timing(self.h, ms))
        return dict(faces=ms[0], order=ms[1], binning=ms[2], tiles=ms[3])

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_overlay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Raster:
    """Depth and face-id render of the posed mesh on the device, face / vertex visibility from a face-id image, per-vertex
    attributes shaded over a render and images sampled at projected points
    (bodyfit_raster_*, csrc/k_raster*.hip; the definition and its contract: include/bodyfit.h).  The handle holds one topology
    (faces: int32 [n_faces, 3] with ids in [0, n_verts)), one image size and the workspace; calls on one handle must be
    ordered (one stream, or events)."""

    def __init__(self, device: int, n_verts: int, faces, width: int, height: int):
        f = np.asarray(faces)
        if f.dtype.kind not in "iu":
            raise TypeError("faces must be an integer array")
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"faces must be [n_faces, 3], got {f.shape}")
        f = np.ascontiguousarray(f, dtype=np.int32)
        h = C.c_void_p()
        _check(load_library().bodyfit_raster_create(int(device), int(n_verts), int(f.shape[0]),
                                                    f.ctypes.data_as(C.POINTER(C.c_int32)), int(width), int(height),
                                                    C.byref(h)))
        self.h = h
        self.device = device
        self.n_verts, self.n_faces = int(n_verts), int(f.shape[0])
        self.width, self.height = int(width), int(height)

    def render_device(self, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, intr, d_depth_ptr: int, d_face_ptr: int,
                      d_bary_ptr: int | None = None, z_near: float = 0.1, cull_backfaces: bool = False,
                      stream: int | None = None):
        """bodyfit_raster_render_device: depth [F, H, W] f32 (+inf where empty), face [F, H, W] int32 (-1 where empty) and,
        unless None, bary [F, H, W, 3] f32 of the vertices [F, n_verts, 3] f32 at verts_frame_stride floats between frames,
        intr = (fx, fy, cx, cy); asynchronous on `stream` but for one 8-byte read-back that sizes the tile lists."""
        _check(load_library().bodyfit_raster_render_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                           float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]),
                                                           float(z_near), int(bool(cull_backfaces)), d_depth_ptr, d_face_ptr,
                                                           d_bary_ptr, stream))

    def visibility_device(self, d_face_ptr: int, n_frames: int, d_face_visible_ptr: int | None,
                          d_vert_visible_ptr: int | None, stream: int | None = None):
        """bodyfit_raster_visibility_device: u8 [F, n_faces] (the face owns a pixel) and u8 [F, n_verts] (a corner of such a
        face) from a face-id image [F, H, W] int32; either output may be None; asynchronous on `stream`."""
        _check(load_library().bodyfit_raster_visibility_device(self.h, d_face_ptr, int(n_frames), d_face_visible_ptr,
                                                               d_vert_visible_ptr, stream))

    def depth_rows_device(self, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, intr, d_face_image_ptr: int,
                          d_pixel_ptr: int | None, d_offset_ptr: int | None, n_rows: int, d_index_ptr: int,
                          d_z_ptr: int | None = None, d_bary_ptr: int | None = None, d_dir_ptr: int | None = None,
                          stream: int | None = None):
        """bodyfit_raster_depth_rows_device: per row (a pixel of a frame: pixel [N] int32 linear indices with offset [F + 1]
        int32 or None for N / F per frame; both None: every pixel, N = F H W) the face of the face-id image [F, H, W] int32
        under it (index [N] int32, -1: void), the ray-plane depth z [N] f32 (+inf: void), the object-space barycentrics bary
        [N, 3] f32 and the direction dir [N, 3] f32 with dz/dcorner_a = bary_a dir; the last three may be None.  Asynchronous
        on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_depth_rows_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                               float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]),
                                                               d_face_image_ptr, d_pixel_ptr, d_offset_ptr, int(n_rows),
                                                               d_index_ptr, d_z_ptr, d_bary_ptr, d_dir_ptr, stream))

    def interp_rows_device(self, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, intr, d_face_image_ptr: int,
                           d_pixel_ptr: int | None, d_offset_ptr: int | None, n_rows: int, d_attr_ptr: int | None,
                           attr_frame_stride: int, n_channels: int, d_grad_image_ptr: int | None, d_grad_z_ptr: int | None,
                           d_index_ptr: int, d_bary_ptr: int | None = None, d_dir_ptr: int | None = None,
                           d_value_ptr: int | None = None, stream: int | None = None):
        """bodyfit_raster_interp_rows_device: per row (addressed as in depth_rows_device) the face (index [N] int32, -1: void), the
        object-space barycentrics bary [N, 3] f32 and the ONE direction dir [N, 3] f32 with dL/dcorner_a = bary_a dir, for the
        upstream gradients grad_image [F, H, W, n_channels] f32 in the attributes (rows of n_channels f32 per vertex, 0 .. 4;
        attr_frame_stride floats between frames, 0: shared) interpolated over the face and grad_z [F, H, W] f32 (or None) in the
        ray-plane depth, both read at the row's pixel; value [N, n_channels] f32 or None: the interpolated attributes.
        n_channels = 0 (attr and grad_image None) is the depth-only case.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_interp_rows_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                                float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]),
                                                                d_face_image_ptr, d_pixel_ptr, d_offset_ptr, int(n_rows),
                                                                d_attr_ptr, int(attr_frame_stride), int(n_channels),
                                                                d_grad_image_ptr, d_grad_z_ptr, d_index_ptr, d_bary_ptr,
                                                                d_dir_ptr, d_value_ptr, stream))

    def interp_rows_indexed_device(self, d_verts_ptr: int, verts_frame_stride: int, n_frames: int, intr, d_face_image_ptr: int,
                                   d_pixel_ptr: int | None, d_offset_ptr: int | None, n_rows: int, d_attr_ptr: int | None,
                                   attr_frame_stride: int, n_channels: int, d_attr_faces_ptr: int | None, n_attr_rows: int,
                                   d_grad_image_ptr: int | None, d_grad_z_ptr: int | None, d_index_ptr: int,
                                   d_bary_ptr: int | None = None, d_dir_ptr: int | None = None, d_value_ptr: int | None = None,
                                   stream: int | None = None):
        """bodyfit_raster_interp_rows_indexed_device: interp_rows_device with the attribute rows of a face taken from
        attr_faces int32 [n_faces, 3] (device; entries in [0, n_attr_rows), anything else voids the face's rows) instead of the
        corners' vertex ids: per-corner attributes such as the rows of a uv atlas.  Asynchronous on `stream`."""
        _check(load_library().bodyfit_raster_interp_rows_indexed_device(
            self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames), float(intr[0]), float(intr[1]), float(intr[2]),
            float(intr[3]), d_face_image_ptr, d_pixel_ptr, d_offset_ptr, int(n_rows), d_attr_ptr, int(attr_frame_stride),
            int(n_channels), d_attr_faces_ptr, int(n_attr_rows), d_grad_image_ptr, d_grad_z_ptr, d_index_ptr, d_bary_ptr, d_dir_ptr,
            d_value_ptr, stream))

    def texture_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                       d_uv_ptr: int | None, n_uv: int, d_uv_faces_ptr: int | None, d_tex_ptr: int | None, tex_kind: int,
                       n_channels: int, tex_height: int, tex_width: int, tex_frame_stride: int, n_frames: int, background,
                       d_image_ptr: int, d_weight_ptr: int | None = None, d_uv_out_ptr: int | None = None,
                       stream: int | None = None):
        """bodyfit_raster_texture_device: the texture [Ht, Wt, n_channels] (tex_kind 0: u8, raw 0 .. 255; 1: f32;
        tex_frame_stride elements between the frames' textures, 0: shared) looked up bilinearly, clamp-to-edge, at the uv of
        every pixel of a render (face [F, H, W] int32, bary [F, H, W, 3] f32): uv f32 [n_uv, 2] and uv_faces int32 [n_faces, 3]
        on the device, interpolated with the shade's perspective-correct weights.  image [F, H, W, n_channels] f32 and, unless
        None, weight [F, H, W, 3] f32 (the shade's) and uv_out [F, H, W, 2] f32.  background: a float or up to four floats.
        Asynchronous on `stream`, no host synchronisation."""
        bg = np.zeros(4, np.float32)
        b = np.atleast_1d(np.asarray(background, np.float32))
        if b.ndim != 1 or b.shape[0] > 4:
            raise ValueError("background is a float or up to four floats")
        bg[:4 if b.shape[0] == 1 else b.shape[0]] = b          # (one float: every channel)
        _check(load_library().bodyfit_raster_texture_device(
            self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride), d_uv_ptr, int(n_uv), d_uv_faces_ptr, d_tex_ptr,
            int(tex_kind), int(n_channels), int(tex_height), int(tex_width), int(tex_frame_stride), int(n_frames),
            bg.ctypes.data_as(C.POINTER(C.c_float)), d_image_ptr, d_weight_ptr, d_uv_out_ptr, stream))

    def texture_grad_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                            d_uv_ptr: int | None, n_uv: int, d_uv_faces_ptr: int | None, d_tex_ptr: int | None, tex_kind: int,
                            n_channels: int, tex_height: int, tex_width: int, tex_frame_stride: int, n_frames: int,
                            d_grad_image_ptr: int, d_grad_uv_ptr: int | None, d_grad_tex_ptr: int | None,
                            d_workspace_ptr: int | None, stream: int | None = None):
        """bodyfit_raster_texture_grad_device: for grad_image [F, H, W, n_channels] f32 the gradient of texture_device's image
        in the pixels' uv, grad_uv [F, H, W, 2] f32 (or None), and in the texels, grad_tex f32 [Ht, Wt, n_channels] (a shared
        texture: summed over the frames) or [F, Ht, Wt, n_channels] (or None; tex may then be None), summed exactly in the int64
        workspace of grad_tex's shape: no float atomics, bit-identical whatever the order.  Asynchronous on `stream`, no host
        synchronisation."""
        _check(load_library().bodyfit_raster_texture_grad_device(
            self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride), d_uv_ptr, int(n_uv), d_uv_faces_ptr, d_tex_ptr,
            int(tex_kind), int(n_channels), int(tex_height), int(tex_width), int(tex_frame_stride), int(n_frames), d_grad_image_ptr,
            d_grad_uv_ptr, d_grad_tex_ptr, d_workspace_ptr, stream))

    def texture_mip_build_device(self, d_tex_ptr: int | None, tex_kind: int, n_channels: int, tex_height: int, tex_width: int,
                                 tex_frame_stride: int, n_textures: int, max_level: int, d_mip_ptr: int | None,
                                 mip_frame_stride: int, stream: int | None = None):
        """bodyfit_raster_texture_mip_build_device: the levels 1 .. n - 1 of n_textures textures into mip (f32, the packed
        layout of texture_mip_layout, mip_frame_stride elements between the textures' pyramids), each level the f64 average
        of the stored level below it.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_texture_mip_build_device(
            self.h, d_tex_ptr, int(tex_kind), int(n_channels), int(tex_height), int(tex_width), int(tex_frame_stride),
            int(n_textures), int(max_level), d_mip_ptr, int(mip_frame_stride), stream))

    def texture_mip_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                           d_uv_ptr: int | None, n_uv: int, d_uv_faces_ptr: int | None, d_tex_ptr: int | None, tex_kind: int,
                           n_channels: int, tex_height: int, tex_width: int, tex_frame_stride: int, n_frames: int, intr,
                           d_mip_ptr: int | None, mip_frame_stride: int, max_level: int, lod_bias: float, background,
                           d_image_ptr: int, d_weight_ptr: int | None = None, d_uv_out_ptr: int | None = None,
                           d_lod_ptr: int | None = None, stream: int | None = None):
        """bodyfit_raster_texture_mip_device: texture_device with mipmaps: the level of detail L of every pixel from its
        face's footprint under intr = (fx, fy, cx, cy) plus lod_bias, clamped to the pyramid's levels (mip: what
        texture_mip_build_device wrote for the same max_level), and the trilinear blend of the levels floor(L) and
        floor(L) + 1; lod [F, H, W] f32 (or None) receives L.  Where L = 0 the image is texture_device's bit for bit."""
        bg = _background4(background)
        _check(load_library().bodyfit_raster_texture_mip_device(
            self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride), d_uv_ptr, int(n_uv), d_uv_faces_ptr, d_tex_ptr,
            int(tex_kind), int(n_channels), int(tex_height), int(tex_width), int(tex_frame_stride), int(n_frames), float(intr[0]),
            float(intr[1]), float(intr[2]), float(intr[3]), d_mip_ptr, int(mip_frame_stride), int(max_level), float(lod_bias),
            bg.ctypes.data_as(C.POINTER(C.c_float)), d_image_ptr, d_weight_ptr, d_uv_out_ptr, d_lod_ptr, stream))

    def texture_mip_grad_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                                d_uv_ptr: int | None, n_uv: int, d_uv_faces_ptr: int | None, d_tex_ptr: int | None, tex_kind: int,
                                n_channels: int, tex_height: int, tex_width: int, tex_frame_stride: int, n_frames: int, intr,
                                d_mip_ptr: int | None, mip_frame_stride: int, max_level: int, lod_bias: float,
                                d_grad_image_ptr: int, d_grad_uv_ptr: int | None, d_grad_tex_ptr: int | None,
                                d_workspace_ptr: int | None, stream: int | None = None):
        """bodyfit_raster_texture_mip_grad_device: the gradients of texture_mip_device's image at the fixed level of detail:
        grad_uv [F, H, W, 2] (or None) and grad_tex in the LEVEL-0 texture's layout (or None), the exact adjoint of "average
        the pyramid, then filter", summed in the int64 workspace of (Ht Wt + total) n_channels elements per texture (level 0
        first) and folded in a fixed order: bit-identical whatever the order of the pixels and of the frames."""
        _check(load_library().bodyfit_raster_texture_mip_grad_device(
            self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride), d_uv_ptr, int(n_uv), d_uv_faces_ptr, d_tex_ptr,
            int(tex_kind), int(n_channels), int(tex_height), int(tex_width), int(tex_frame_stride), int(n_frames), float(intr[0]),
            float(intr[1]), float(intr[2]), float(intr[3]), d_mip_ptr, int(mip_frame_stride), int(max_level), float(lod_bias),
            d_grad_image_ptr, d_grad_uv_ptr, d_grad_tex_ptr, d_workspace_ptr, stream))

    def light_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                     d_normals_ptr: int | None, normals_frame_stride: int, d_albedo_ptr: int, n_channels: int, d_light_ptr: int,
                     light_frame_stride: int, n_frames: int, d_image_ptr: int, d_normal_ptr: int | None = None,
                     d_shading_ptr: int | None = None, stream: int | None = None):
        """bodyfit_raster_light_device: image [F, H, W, n_channels] f32 = albedo x s(n), s_c = sum_k light[k][c] b_k(n) with
        the nine second-order polynomials b of the unit normal n interpolated from the per-vertex normals [F, n_verts, 3] f32
        with the shade's weights; light f32 [9, n_channels], light_frame_stride floats between frames (0: shared).  An unlit
        pixel (void, a non-finite or cancelling normal) passes its albedo through.  Unless None, normal [F, H, W, 3] f32 and
        shading [F, H, W, n_channels] f32.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_light_device(
            self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride), d_normals_ptr, int(normals_frame_stride),
            d_albedo_ptr, int(n_channels), d_light_ptr, int(light_frame_stride), int(n_frames), d_image_ptr, d_normal_ptr,
            d_shading_ptr, stream))

    def light_grad_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                          d_normals_ptr: int | None, normals_frame_stride: int, d_albedo_ptr: int, n_channels: int,
                          d_light_ptr: int, light_frame_stride: int, n_frames: int, d_grad_image_ptr: int,
                          d_grad_albedo_ptr: int | None, d_grad_m_ptr: int | None, d_grad_light_ptr: int | None,
                          d_workspace_ptr: int | None, stream: int | None = None):
        """bodyfit_raster_light_grad_device: for grad_image [F, H, W, n_channels] f32 the gradients of light_device's image
        in the albedo [F, H, W, n_channels], in the unnormalised interpolated normal [F, H, W, 3] (what the rows VJP takes) and
        in the light, ALWAYS per frame [F, 9, n_channels]; each may be None.  The light's is reduced in f64 in a fixed order
        through the f64 workspace of light_grad_layout(...)[2] elements: no atomics, bit-identical from run to run and
        whatever the batch around a frame.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_light_grad_device(
            self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride), d_normals_ptr, int(normals_frame_stride),
            d_albedo_ptr, int(n_channels), d_light_ptr, int(light_frame_stride), int(n_frames), d_grad_image_ptr,
            d_grad_albedo_ptr, d_grad_m_ptr, d_grad_light_ptr, d_workspace_ptr, stream))

    def distance_device(self, d_seed_ptr: int, seed_kind: int, seed_frame_stride: int, n_frames: int, invert: bool,
                        d_dist2_ptr: int, d_nearest_ptr: int | None = None, stream: int | None = None):
        """bodyfit_raster_distance_device: the exact squared Euclidean distance dist2 [F, H, W] int32 of every pixel to the
        nearest seed of its frame and, unless None, nearest [F, H, W] int32, the linear index i W + j of a seed that attains it
        (INT32_MAX and -1 in a frame without a seed).  seed_kind 0: u8 [F, H, W], a seed iff != 0; 1: int32 [F, H, W], a seed iff
        >= 0 (a rendered face-id image); seed_frame_stride elements between frames; invert swaps seeds and non-seeds.
        Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_distance_device(self.h, d_seed_ptr, int(seed_kind), int(seed_frame_stride),
                                                             int(n_frames), int(bool(invert)), d_dist2_ptr, d_nearest_ptr,
                                                             stream))

    def shade_device(self, d_face_ptr: int, d_bary_ptr: int, d_verts_ptr: int | None, verts_frame_stride: int,
                     d_attr_ptr: int | None, attr_frame_stride: int, n_channels: int, n_frames: int, background,
                     d_image_ptr: int, d_weight_ptr: int | None = None, stream: int | None = None):
        """bodyfit_raster_shade_device: per-vertex attributes (rows of n_channels f32, 1 .. 4; attr_frame_stride floats between
        frames, 0: shared by the frames) interpolated perspective-correct over a face-id image [F, H, W] int32 with weights
        bary [F, H, W, 3] f32: image [F, H, W, n_channels] f32 and, unless None, the object-space weights [F, H, W, 3] f32.
        background: a float or up to four floats (a void pixel's value).  Asynchronous on `stream`, no host synchronisation."""
        bg = np.zeros(4, np.float32)
        b = np.atleast_1d(np.asarray(background, np.float32))
        if b.ndim != 1 or b.shape[0] > 4:
            raise ValueError("background is a float or up to four floats")
        bg[:4 if b.shape[0] == 1 else b.shape[0]] = b          # (one float: every channel)
        _check(load_library().bodyfit_raster_shade_device(self.h, d_face_ptr, d_bary_ptr, d_verts_ptr, int(verts_frame_stride),
                                                          d_attr_ptr, int(attr_frame_stride), int(n_channels), int(n_frames),
                                                          bg.ctypes.data_as(C.POINTER(C.c_float)), d_image_ptr, d_weight_ptr,
                                                          stream))

    def sample_device(self, d_points_ptr: int, points_frame_stride: int, n_points: int, n_frames: int, intr, d_image_ptr: int,
                      image_kind: int, n_channels: int, image_frame_stride: int, d_gate_ptr: int | None, d_value_ptr: int,
                      d_valid_ptr: int, d_grad_ptr: int | None = None, z_near: float = 0.1, stream: int | None = None):
        """bodyfit_raster_sample_device: the images [F, H, W, n_channels] (image_kind 0: u8, raw 0 .. 255; 1: f32;
        image_frame_stride elements between frames) read bilinearly at the projections of points [F, n_points, 3] f32: value
        [F, n_points, n_channels] f32, valid [F, n_points] u8 and, unless None, grad [F, n_points, n_channels, 2] f32 = (d/du,
        d/dv); gate u8 [F, n_points] or None.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_sample_device(self.h, d_points_ptr, int(points_frame_stride), int(n_points),
                                                           int(n_frames), float(intr[0]), float(intr[1]), float(intr[2]),
                                                           float(intr[3]), float(z_near), d_image_ptr, int(image_kind),
                                                           int(n_channels), int(image_frame_stride), d_gate_ptr, d_value_ptr,
                                                           d_valid_ptr, d_grad_ptr, stream))

    def edges_device(self, d_verts_ptr: int | None, verts_frame_stride: int, n_frames: int, intr, d_face_ptr: int | None,
                     d_depth_ptr: int | None, d_weight_ptr: int, z_near: float = 0.1, cull_backfaces: bool = False,
                     stream: int | None = None):
        """bodyfit_raster_edges_device: the silhouette-edge antialiasing weights [F, H, W, 2] f32 (per pixel its right and lower
        pair: > 0 the neighbour receives, < 0 the pixel receives, 0 no blend) of a render (face [F, H, W] int32, depth [F, H, W]
        f32) of the vertices [F, n_verts, 3] f32.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_raster_edges_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                          float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]),
                                                          float(z_near), int(bool(cull_backfaces)), d_face_ptr, d_depth_ptr,
                                                          d_weight_ptr, stream))

    def edge_blend_device(self, d_weight_ptr: int, d_image_ptr: int, n_channels: int, n_frames: int, transpose: bool,
                          d_out_ptr: int, stream: int | None = None):
        """bodyfit_raster_edge_blend_device: out [F, H, W, n_channels] f32 = the image blended by the weights of edges_device, or
        with transpose the adjoint of that map applied to the image.  Asynchronous on `stream`."""
        _check(load_library().bodyfit_raster_edge_blend_device(self.h, d_weight_ptr, d_image_ptr, int(n_channels), int(n_frames),
                                                               int(bool(transpose)), d_out_ptr, stream))

    def edge_rows_device(self, d_verts_ptr: int | None, verts_frame_stride: int, n_frames: int, intr, d_face_ptr: int | None,
                         d_depth_ptr: int | None, d_image_ptr: int | None, d_grad_ptr: int | None, n_channels: int,
                         d_pair_ptr: int, d_offset_ptr: int | None, n_pairs: int, d_index_ptr: int, d_bary_ptr: int,
                         d_coef_ptr: int, d_dir_ptr: int, z_near: float = 0.1, cull_backfaces: bool = False,
                         stream: int | None = None):
        """bodyfit_raster_edge_rows_device: for the listed pairs (pair [N] int32 = 2 pixel + axis, offset [F + 1] int32 or None)
        the two rows (index [2 N] int32, bary [2 N, 3], coef [2 N], dir [2 N, 3] f32) of the blend's gradient in the two corners
        of the pair's silhouette edge, from the image and the upstream gradient [F, H, W, n_channels] f32; index -1: the pair does
        not blend.  Asynchronous on `stream`."""
        _check(load_library().bodyfit_raster_edge_rows_device(self.h, d_verts_ptr, int(verts_frame_stride), int(n_frames),
                                                              float(intr[0]), float(intr[1]), float(intr[2]), float(intr[3]),
                                                              float(z_near), int(bool(cull_backfaces)), d_face_ptr, d_depth_ptr,
                                                              d_image_ptr, d_grad_ptr, int(n_channels), d_pair_ptr, d_offset_ptr,
                                                              int(n_pairs), d_index_ptr, d_bary_ptr, d_coef_ptr, d_dir_ptr, stream))

    def last_bins(self):
        """(face, tile) pairs binned by the latest render, and its longest tile list"""
        n, longest = C.c_longlong(0), C.c_int(0)
        _check(load_library().bodyfit_raster_last_bins(self.h, C.byref(n), C.byref(longest)))
        return int(n.value), int(longest.value)

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_raster_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Volume:
    """The geometry of a scalar volume [nz, ny, nx] f32 (x fastest), voxel (k, j, i) at origin + (i sx, j sy, k sz), and its
    trilinear sampler (bodyfit_volume_*, csrc/k_volume.hip; the definition and its contract: include/bodyfit.h).  The handle holds
    no device memory: the voxels are an argument of every call."""

    def __init__(self, device: int, dims, origin, spacing):
        nx, ny, nz = (int(n) for n in dims)
        o, s = _c64(origin).reshape(-1), _c64(spacing).reshape(-1)
        if o.shape[0] != 3 or s.shape[0] != 3:
            raise ValueError("dims is (nx, ny, nz), origin and spacing are 3 floats")
        h = C.c_void_p()
        _check(load_library().bodyfit_volume_create(int(device), nx, ny, nz, _d(o), _d(s), C.byref(h)))
        self.h = h
        self.device = device
        self.nx, self.ny, self.nz = nx, ny, nz
        self.origin, self.spacing = tuple(float(a) for a in o), tuple(float(a) for a in s)

    def sample_device(self, d_points_ptr: int, points_frame_stride: int, n_points: int, n_frames: int, d_volume_ptr: int,
                      volume_frame_stride: int, d_gate_ptr: int | None, d_value_ptr: int, d_valid_ptr: int,
                      d_grad_ptr: int | None = None, stream: int | None = None):
        """bodyfit_volume_sample_device: the volumes [nz, ny, nx] f32 (volume_frame_stride elements between frames, 0: one for all)
        read trilinearly at points [F, n_points, 3] f32: value [F, n_points] f32, valid [F, n_points] u8 and, unless None, grad
        [F, n_points, 3] f32 = (d/dx, d/dy, d/dz) in world units; gate u8 [F, n_points] or None.  Asynchronous on `stream`, no host
        synchronisation."""
        _check(load_library().bodyfit_volume_sample_device(self.h, d_points_ptr, int(points_frame_stride), int(n_points),
                                                           int(n_frames), d_volume_ptr, int(volume_frame_stride), d_gate_ptr,
                                                           d_value_ptr, d_valid_ptr, d_grad_ptr, stream))

    def integrate_device(self, d_depth_ptr: int | None, depth_frame_stride: int, height: int, width: int, n_frames: int, intr,
                         d_pose_ptr: int | None, trunc: float, z_near: float, max_weight: float, reset: bool, d_tsdf_ptr: int,
                         d_weight_ptr: int, volume_frame_stride: int = 0, stream: int | None = None):
        """bodyfit_volume_integrate_device: the depth maps [n_frames, height, width] f32 (metres along the optical axis,
        depth_frame_stride floats between frames), seen through intr = (fx, fy, cx, cy) from the world -> camera maps d_pose
        [n_frames, 12] f64 (None: the identity), fused in ascending order into the state (tsdf, weight) [nz, ny, nx] f32 of this
        geometry: volume_frame_stride 0 into one volume, >= nx ny nz frame f into volume f.  reset: start from the empty state
        (NaN, 0) without reading the buffers.  max_weight inf: no cap.  Asynchronous on `stream`, no host synchronisation."""
        k = None if intr is None else _c64(intr).reshape(-1)
        if k is not None and k.shape[0] != 4:
            raise ValueError("intr is (fx, fy, cx, cy)")
        _check(load_library().bodyfit_volume_integrate_device(self.h, d_depth_ptr, int(depth_frame_stride), int(height), int(width),
                                                              int(n_frames), None if k is None else _d(k), d_pose_ptr, float(trunc),
                                                              float(z_near), float(max_weight), 1 if reset else 0, d_tsdf_ptr,
                                                              d_weight_ptr, int(volume_frame_stride), stream))

    def surface_layout(self, n_volumes: int) -> int:
        """bodyfit_volume_surface_layout: the bytes of the workspace that surface_count_device and surface_emit_device share"""
        n = C.c_longlong()
        _check(load_library().bodyfit_volume_surface_layout(self.h, int(n_volumes), C.byref(n)))
        return int(n.value)

    def surface_count_device(self, d_volume_ptr: int, d_weight_ptr: int | None, volume_frame_stride: int, n_volumes: int,
                             iso: float, min_weight: float, d_workspace_ptr: int, d_offsets_ptr: int, stream: int | None = None):
        """bodyfit_volume_surface_count_device: marching cubes of the n_volumes volumes [nz, ny, nx] f32 at the level iso (weight:
        the same shape or None; a voxel below min_weight is unusable), first half: offsets i64 [2, n_volumes + 1], the exclusive
        vertex offsets of the volumes, then their face offsets, the last of each the total.  Asynchronous on `stream`."""
        _check(load_library().bodyfit_volume_surface_count_device(self.h, d_volume_ptr, d_weight_ptr, int(volume_frame_stride),
                                                                  int(n_volumes), float(iso), float(min_weight), d_workspace_ptr,
                                                                  d_offsets_ptr, stream))

    def surface_emit_device(self, d_volume_ptr: int, d_weight_ptr: int | None, volume_frame_stride: int, n_volumes: int,
                            iso: float, min_weight: float, d_workspace_ptr: int, d_offsets_ptr: int, vert_capacity: int,
                            face_capacity: int, d_verts_ptr: int | None, d_faces_ptr: int | None, stream: int | None = None):
        """bodyfit_volume_surface_emit_device: second half, with the inputs, the workspace and the offsets of the count: verts f32
        [vert_capacity, 3] and faces int32 [face_capacity, 3] (indices local to a volume); nothing is stored past a capacity."""
        _check(load_library().bodyfit_volume_surface_emit_device(self.h, d_volume_ptr, d_weight_ptr, int(volume_frame_stride),
                                                                 int(n_volumes), float(iso), float(min_weight), d_workspace_ptr,
                                                                 d_offsets_ptr, int(vert_capacity), int(face_capacity), d_verts_ptr,
                                                                 d_faces_ptr, stream))

    def distance_layout(self, n_volumes: int) -> int:
        """bodyfit_volume_distance_layout: the bytes of distance_device's workspace for n_volumes volumes"""
        n = C.c_longlong()
        _check(load_library().bodyfit_volume_distance_layout(self.h, int(n_volumes), C.byref(n)))
        return int(n.value)

    def distance_device(self, d_seed_ptr: int, seed_kind: int, seed_volume_stride: int, n_volumes: int, invert: bool,
                        d_workspace_ptr: int, d_dist2_ptr: int, d_nearest_ptr: int | None = None, stream: int | None = None):
        """bodyfit_volume_distance_device: the exact squared Euclidean distance dist2 [n_volumes, nz, ny, nx] int32, in index
        units, of every voxel to the nearest seed of its volume and, unless None, nearest = (k' ny + j') nx + i' of a seed that
        attains it (INT32_MAX / -1 in a volume without a seed).  seed_kind 0: u8, a seed iff != 0; 1: int32, a seed iff >= 0;
        invert swaps seeds and non-seeds.  Asynchronous on `stream`, no host synchronisation."""
        _check(load_library().bodyfit_volume_distance_device(self.h, d_seed_ptr, int(seed_kind), int(seed_volume_stride),
                                                             int(n_volumes), 1 if invert else 0, d_workspace_ptr, d_dist2_ptr,
                                                             d_nearest_ptr, stream))

    def close(self):
        if getattr(self, "h", None):
            load_library().bodyfit_volume_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def renderSMPLMesh(cloud, faces, img, fx, fy, cx, cy, fill=True, backface_cull=True, wireframe=False, device=0):
    """include/RenderSMPLMesh.h:16-24, one frame: cloud [V][3] (or the reference's 3xV, column-major), img HxWx3 uint8
    drawn in place."""
    cloud = np.asarray(cloud)
    if cloud.ndim == 2 and cloud.shape[0] == 3 and cloud.shape[1] != 3:
        cloud = cloud.T
    ov = Overlay(faces, cloud.shape[0], img.shape[1], img.shape[0], 1, device)
    try:
        ov.render(cloud[None], img.reshape(1, *img.shape), (fx, fy, cx, cy), fill, backface_cull, wireframe)
    finally:
        ov.close()
    return img


def mean_pixel_error(jid, uv, joints, intr) -> float:
    jid = _c32i(jid); uv = _c64(uv); joints = _c64(joints)
    return load_library().bodyfit_mean_pixel_error(len(jid), _i(jid), _d(uv), _d(joints), float(intr[0]), float(intr[1]),
                                                   float(intr[2]), float(intr[3]))
