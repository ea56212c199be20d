"""PyTorch autograd layers over the library's SMPL forward and fitting objective, with their reverse-mode gradients.

    layer = SMPLLayer(api.Model(model))
    verts, joints = layer(x, beta)          # x [F, 76] f64 cuda, beta [nS] (or [F, nS]) f64 cuda
    loss(verts, joints).backward()

forward is bodyfit_forward_device (the two-launch sweep: verts [F, V, 3] f32, joints [F, 24, 3] f64), backward is
bodyfit_forward_vjp_device (HIP kernels, k_forward_vjp.hip).  Both run on torch.cuda.current_stream() without a host
synchronisation.  The layer keeps one keypoint-free problem (want_mesh) per frame count.  Calls that share a frame count share
that problem's device buffers, so interleaving them on several streams at once needs the caller's own ordering (events).

    obj = FitObjective(problem)             # an api.Problem: keypoints, camera, priors, temporal terms
    r = obj(x, beta)                        # [total_rows] f64 residual vector (bodyfit_residuals_device)
    (obj.cost(r) + my_term).backward()      # backward: bodyfit_residual_vjp_device (k_residual_vjp.hip)

obj.cost(r) is the Ceres cost of the problem (HuberLoss on the keypoint blocks, squares elsewhere), written in torch.
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
        return verts, joints

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

    def forward(self, x: torch.Tensor, beta: torch.Tensor):
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
        return _SMPLForward.apply(x.contiguous(), beta.contiguous(), self.problem(F), self.model.n_verts, self.model.n_joints)


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
