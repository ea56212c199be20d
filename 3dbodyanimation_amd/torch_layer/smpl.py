"""The SMPL forward and the fitting objective as autograd layers.

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

    verts, joints = layer(x, beta, offsets=d)                            # SMPL+D: d [V, 3] or [F, V, 3] f32, differentiable

Every data term measures a naked body against a clothed person.  offsets displaces the blended rest vertex before
skinning (bodyfit_forward_offsets*_device, k_offsets.hip); the joints, and with them FitObjective's keypoint landmarks, stay those
of the undisplaced shape.  layer.jvp / layer.jacobian / forward_ad and every normal_equations take offsets= as a constant, so a
Gauss-Newton step on pose and shape alternates with gradient steps on the offsets (solid.OffsetRegulariser keeps them smooth).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import api
from ._common import _stream


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
