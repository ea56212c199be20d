"""A named table of frames across the parameter domain of the SMPL pipeline, the per-frame magnitudes that the bounds of
tests/test_gpu_domain.py scale with, a numpy model of the mesh path's arithmetic, and the scaled reference gradients.

Imported by the tests as a plain module (like model_variants.py); numpy and the f64 CPU checker only, deterministic.

THE TABLE (cases): one frame per case, so that one launch covers all of it.  What a case does not set is joints N(0, 0.3 rad)
(root included), s = 1, t = (0, 0, 3), beta = 0 -- the distribution every other test of the suite draws from ("control").
For shared-beta problems the table carries one beta = 3 x (+-1 alternating) and the three beta cases are dropped.
"tiny_1e-8" is inside Rodrigues' first-order branch (theta^2 <= DBL_EPSILON) without being zero: there dR_c = [e_c]x, which
is off the exponential's derivative by up to 2 theta (first_order_slack).
"control_empty" repeats control's parameters: it is the frame that the observations leave without keypoints.

THE ARITHMETIC MODEL (model_cloud): the mesh path as include/bodyfit.h states it -- f32 Rodrigues features (first-order branch
at theta^2 <= 1e-20f, frame_part_inl.h), operands split in bf16 hi + lo by round-to-nearest-even, hi.hi + hi.lo + lo.hi
accumulated in f32, the skinning transforms computed in f64 with s and + t inside and rounded to f32, the four-joint blend of
the transforms and the final 3 x 4 product in f32.  E_f = max_v |model - checker| is the cost of that arithmetic on frame f;
the cloud bound of the GPU tests is B_f = 4 E_f (min(B_f, 5e-6) on control and rest).  E_f on model_variants.get("v2049"),
seed 0, in metres (tests/test_domain_cases.py prints this table and holds the committed figures to a factor 2):

  control        5.72e-07
  rest           5.71e-07
  tiny_1e-8      5.96e-07
  tiny_1e-7      4.65e-07
  tiny_1e-5      4.90e-07
  tiny_1e-3      5.37e-07
  half_pi        5.25e-07
  pi_minus       6.61e-07
  pi             5.93e-07
  pi_plus        6.20e-07
  two_pi_minus   5.50e-07
  two_pi         4.34e-07
  theta_7.5      6.37e-07
  one_knee_pi_x  4.57e-07
  axis_aligned   5.72e-07
  sigma_1        6.85e-07
  root_pi        5.55e-07
  root_two_pi    5.45e-07
  scale_0.05     5.44e-07
  scale_20       1.17e-05
  near           1.81e-07
  far            1.88e-05
  off_axis       1.01e-05
  behind         5.43e-07
  beta_plus5     3.30e-06
  beta_alt5      3.64e-06
  beta_zero      5.91e-07
  mixed          7.48e-05
  control_empty  5.72e-07
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import model_variants as mv

synth = mv.synth
NEAR_Z = 0.25                 # m: the smallest depth of the case "near"
KNEE = 4                      # l_knee: the joint of "one_knee_pi_x"
F32_BRANCH = np.float32(1e-20)   # frame_part_inl.h: theta^2 at or below it takes R - I = [a]x in the f32 features


def _axes(rng, n):
    a = rng.normal(size=(n, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _alt(n, a):
    return a * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)


def _oracle_model(v):
    from oracle import oracle
    oracle.build()
    return mv.oracle_model(oracle, v)


def cases(v, seed=0, shared_beta=False, om=None):
    """names [F], x [F, 76], beta ([F, nS]; [nS] with shared_beta), R0 [F, 9] for a 24-joint Variant.  om: the checker's model
    of v (built when absent; it places the case "near")."""
    assert v.n_joints == 24, "the table is written for the 24-joint tree"
    rng = np.random.default_rng(seed)
    nS = v.n_shape
    names, X, B = [], [], []

    def add(name, joints=None, root=None, s=1.0, t=(0.0, 0.0, 3.0), beta=None):
        gen = rng.normal(scale=0.3, size=72)          # always drawn: a case's numbers do not depend on what another sets
        x = np.zeros(76)
        x[0] = s
        x[1:4] = gen[:3] if root is None else root
        x[4:7] = t
        x[7:] = gen[3:] if joints is None else np.asarray(joints, np.float64).reshape(-1)
        names.append(name); X.append(x); B.append(np.zeros(nS) if beta is None else np.asarray(beta, np.float64))

    def every(theta):
        return theta * _axes(rng, 23)

    add("control")
    add("rest", joints=np.zeros(69))
    for name, th in (("tiny_1e-8", 1e-8), ("tiny_1e-7", 1e-7), ("tiny_1e-5", 1e-5), ("tiny_1e-3", 1e-3), ("half_pi", np.pi / 2),
                     ("pi_minus", np.pi - 1e-6), ("pi", np.pi), ("pi_plus", np.pi + 1e-6), ("two_pi_minus", 2 * np.pi - 1e-5),
                     ("two_pi", 2 * np.pi), ("theta_7.5", 7.5)):
        add(name, joints=every(th))
    knee = np.zeros((23, 3)); knee[KNEE - 1] = [np.pi, 0.0, 0.0]
    add("one_knee_pi_x", joints=knee)
    aligned = np.zeros((23, 3))
    aligned[np.arange(23), rng.integers(0, 3, 23)] = rng.uniform(-np.pi, np.pi, 23)
    add("axis_aligned", joints=aligned)
    add("sigma_1", joints=rng.normal(scale=1.0, size=69))
    add("root_pi", root=np.pi * _axes(rng, 1)[0])
    add("root_two_pi", root=(2 * np.pi - 1e-5) * _axes(rng, 1)[0])
    add("scale_0.05", s=0.05)
    add("scale_20", s=20.0, t=(0.0, 0.0, 60.0))
    add("near", t=(0.0, 0.0, 0.0))
    add("far", t=(0.0, 0.0, 100.0))
    add("off_axis", t=(40.0, -25.0, 50.0))
    add("behind", t=(0.0, 0.0, -3.0))
    if not shared_beta:
        add("beta_plus5", beta=np.full(nS, 5.0))
        add("beta_alt5", beta=_alt(nS, 5.0))
        add("beta_zero", beta=np.zeros(nS))
    add("mixed", joints=every(np.pi), s=20.0, t=(0.0, 0.0, 60.0), beta=_alt(nS, 5.0))
    add("control_empty")
    X[-1][:] = X[0]
    x = np.array(X)
    beta = _alt(nS, 3.0) if shared_beta else np.array(B)
    R0 = np.tile(synth.R0_DEFAULT.reshape(1, 9), (len(names), 1))
    i = names.index("near")     # t_z from the checker's forward: the smallest Z over joints and vertices (landmarks are vertices)
    om = _oracle_model(v) if om is None else om
    j, c = om.forward(x[i], beta if shared_beta else beta[i], R0[i], True, v.pose_blend_data)
    x[i, 6] = NEAR_Z - min(j[:, 2].min(), c[:, 2].min())
    return SimpleNamespace(names=names, x=x, beta=beta, R0=R0, shared_beta=shared_beta, index={n: k for k, n in enumerate(names)})


def observations(v, tab, seed=0):
    """every joint and landmark of v as keypoints, ragged, the frame "control_empty" empty"""
    return mv.observations(v, len(tab.names), seed=seed, empty=(tab.index["control_empty"],))


def _features(x):
    """vec(R_j - I), j = 1..23, in f64: [F, 207]"""
    return np.array([[synth.rodrigues(xf[7 + 3 * j:10 + 3 * j]) - np.eye(3) for j in range(23)] for xf in x]).reshape(len(x), -1)


def magnitudes(om, v, tab):
    """From the checker's forward: P [F] the largest |projected pixel coordinate| over the frame's keypoints (every joint and
    landmark), M [F] the largest |coordinate| of a joint or vertex, zmin [F] the smallest depth, T [F, V] = sum_k |feat_k|
    |posedirs_vk| + sum_k |beta_k| |shapedirs_vk| (the larger of the three coordinates), and the forward itself."""
    m = v.model
    F = len(tab.names)
    joints, cloud = om.forward_batch(tab.x, tab.beta, tab.R0, True, v.pose_blend_data)
    pts = np.concatenate([joints, cloud[:, m.landmark_vid]], axis=1)
    fx, fy, cx, cy = synth.camera_intrinsics()
    uv = np.stack([fx * pts[..., 0] / pts[..., 2] + cx, fy * pts[..., 1] / pts[..., 2] + cy], axis=-1)
    beta = np.broadcast_to(tab.beta, (F, v.n_shape))
    T = np.einsum("fk,vck->fvc", np.abs(_features(tab.x)), np.abs(m.posedirs)) + \
        np.einsum("fk,vck->fvc", np.abs(beta), np.abs(m.shapedirs))
    return SimpleNamespace(P=np.abs(uv).reshape(F, -1).max(1), M=np.maximum(np.abs(joints).reshape(F, -1).max(1),
                                                                           np.abs(cloud).reshape(F, -1).max(1)),
                           zmin=np.minimum(joints[..., 2].min(1), cloud[..., 2].min(1)), T=T.max(2), joints=joints, cloud=cloud)


# ---- the arithmetic model of the mesh path -------------------------------------------------------------------------------
def bf16_round(x):
    """f32 -> the nearest bf16 (ties to even), as f32: bodyfit_device.h f32_to_bf16"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_split(x):
    hi = bf16_round(x)
    return hi, bf16_round(np.asarray(x, np.float32) - hi)


def features_f32(aa, branch=F32_BRANCH):
    """vec(R - I) [n, 9] in f32 from the angle-axis rows aa [n, 3] rounded to f32: sin and 1 - cos from the half angle"""
    a = np.asarray(aa, np.float64).astype(np.float32)
    th2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
    gen = th2 > branch
    safe = np.where(gen, th2, np.float32(1.0))
    ith = np.float32(1.0) / np.sqrt(safe)
    th = safe * ith
    sh, ch = np.sin(np.float32(0.5) * th), np.cos(np.float32(0.5) * th)
    st = np.where(gen, np.float32(2.0) * sh * ch, np.float32(1.0))
    omc = np.where(gen, np.float32(2.0) * sh * sh, np.float32(0.0))
    w = np.where(gen[:, None], a * ith[:, None], a)
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    one = np.float32(1.0)
    out = np.stack([omc * (w0 * w0 - one), omc * w0 * w1 - st * w2, omc * w0 * w2 + st * w1,
                    omc * w1 * w0 + st * w2, omc * (w1 * w1 - one), omc * w1 * w2 - st * w0,
                    omc * w2 * w0 - st * w1, omc * w2 * w1 + st * w0, omc * (w2 * w2 - one)], axis=1)
    assert out.dtype == np.float32
    return out


_operands: dict = {}


def _model_operands(v):
    """the model's side of the contraction, as api_model.hip lays it out: [posedirs | shapedirs - S_root | template, what the
    template's hi + lo leave over] in f32, split; the skinning weights in f32"""
    if v.id not in _operands:
        m = v.model
        J0 = m.j_regressor @ m.v_template
        S_root = np.einsum("v,vck->ck", m.j_regressor[0], m.shapedirs)
        t0 = (m.v_template - J0[0]).astype(np.float32)
        h0, l0 = bf16_split(t0)
        B = np.concatenate([m.posedirs.astype(np.float32), (m.shapedirs - S_root).astype(np.float32), t0[:, :, None],
                            (t0 - (h0 + l0))[:, :, None]], axis=2)
        _operands[v.id] = (bf16_split(B), m.weights.astype(np.float32))
    return _operands[v.id]


def skinning_transforms(model, x, beta, R0):
    """[nJ, 3, 4] f64: s Rr0 [A_j | P_j - A_j Jc_j] + [0 | t] (frame_part_inl.h), one frame"""
    nJ = model.n_joints
    Jb = model.J0 + (model.S @ beta).reshape(nJ, 3)
    Jc = Jb - Jb[0]
    A = np.empty((nJ, 3, 3)); P = np.zeros((nJ, 3))
    A[0] = np.eye(3)
    for j in range(1, nJ):
        p = model.parent[j]
        A[j] = A[p] @ synth.rodrigues(x[7 + 3 * (j - 1):10 + 3 * (j - 1)])
        P[j] = P[p] + A[p] @ (Jc[j] - Jc[p])
    Rr0 = synth.rodrigues(x[1:4]) @ np.asarray(R0).reshape(3, 3)
    T = np.empty((nJ, 3, 4))
    T[:, :, :3] = x[0] * (Rr0 @ A)
    T[:, :, 3] = x[0] * ((P - np.einsum("jab,jb->ja", A, Jc)) @ Rr0.T) + x[4:7]
    return T


def model_cloud(v, x, beta, R0, drop_lo_hi=False, branch=F32_BRANCH):
    """The cloud [V, 3] f32 of one frame by the kernel's stated arithmetic.  drop_lo_hi: without the product of the
    coefficients' lo with the directions' hi (a mutant for the teeth test)."""
    (Bhi, Blo), W = _model_operands(v)
    a = np.zeros(Bhi.shape[2], np.float32)
    a[:207] = features_f32(x[7:].reshape(23, 3), branch).reshape(-1)
    a[207:207 + v.n_shape] = np.asarray(beta, np.float64).astype(np.float32)
    a[-2:] = 1.0
    ahi, alo = bf16_split(a)
    p = Bhi @ ahi + Blo @ ahi                                  # [V, 3] f32, f32 accumulation
    if not drop_lo_hi:
        p = p + Bhi @ alo
    T = skinning_transforms(v.model, x, np.asarray(beta, np.float64), R0).astype(np.float32)
    b = np.einsum("vj,jrc->vrc", W, T)                         # the blended 3 x 4 transform of every vertex, f32
    out = np.einsum("vrc,vc->vr", b[:, :, :3], p) + b[:, :, 3]
    assert out.dtype == np.float32
    return out


def model_errors(v, tab, cloud_ref, **kw):
    """E [F]: max_v |model - checker| per frame of the table"""
    beta = np.broadcast_to(tab.beta, (len(tab.names), v.n_shape))
    return np.array([np.abs(model_cloud(v, tab.x[f], beta[f], tab.R0[f], **kw).astype(np.float64) - cloud_ref[f]).max()
                     for f in range(len(tab.names))])


def cloud_bounds(tab, E):
    """B_f = 4 E_f: the factor covers the order of the f32 sums and fused against unfused products, numpy against the matrix
    pipe and the packed-f32 skinning; min(B_f, 5e-6) where the suite's absolute tolerance has always held"""
    B = 4.0 * np.asarray(E)
    for name in ("control", "rest", "control_empty"):
        B[tab.index[name]] = min(B[tab.index[name]], 5e-6)
    return B


# ---- reference derivatives by differences of the checker's forward, with their own error ------------------------------------
_cloud_extra = None      # set by ref_grad_scaled for its own calls: x -> [F, V, 3] added to the checker's cloud


def _fwd(om, x, beta, R0, use_shape, pose_blend, want_cloud):
    j, c = om.forward_batch(x, beta, R0, use_shape, pose_blend, want_cloud=want_cloud)
    if want_cloud and _cloud_extra is not None:
        c = c + _cloud_extra(x)
    return j, c


def _column(om, x, beta, R0, use_shape, pose_blend, want_cloud, kind, col, step, per_frame):
    """second-order central difference of column col (kind "x" or "b") in every frame at once: frames are independent"""
    xp, xm, bp, bm = x, x, beta, beta
    if kind == "x":
        xp = x.copy(); xp[:, col] += step
        xm = x.copy(); xm[:, col] -= step
    else:
        bp = beta.copy(); bm = beta.copy()
        if per_frame:
            bp[:, col] += step; bm[:, col] -= step
        else:
            bp[col] += step; bm[col] -= step
    jp, cp = _fwd(om, xp, bp, R0, use_shape, pose_blend, want_cloud)
    jm, cm = _fwd(om, xm, bm, R0, use_shape, pose_blend, want_cloud)
    return (jp - jm) / (2 * step), ((cp - cm) / (2 * step) if want_cloud else None)


def _column_o(om, x, beta, R0, use_shape, pose_blend, want_cloud, kind, col, step, per_frame, order):
    d = _column(om, x, beta, R0, use_shape, pose_blend, want_cloud, kind, col, step, per_frame)
    if order == 2:
        return d
    d2 = _column(om, x, beta, R0, use_shape, pose_blend, want_cloud, kind, col, 2 * step, per_frame)   # Richardson: O(h^4)
    return (4 * d[0] - d2[0]) / 3, ((4 * d[1] - d2[1]) / 3 if want_cloud else None)


def _columns(npose, nS, want_beta):
    return [("x", c) for c in range(npose)] + ([("b", k) for k in range(nS)] if want_beta else [])


def dense_jacobian(om, x, beta, R0, use_shape=True, pose_blend=True, want_cloud=True, step=1e-6, order=2, zero_t=True):
    """(Jj [F, K, nJ, 3], Jc [F, K, V, 3] or None), K = npose + nS, every frame's own columns (a shared beta [nS] too: the
    derivative of frame f in beta).  zero_t: differentiate at t = 0 -- no derivative of the forward depends on t, and the
    difference of two coordinates of 100 m loses what one of 1 m keeps."""
    F, npose = x.shape
    R0 = np.asarray(R0).reshape(F, 9)
    x0 = x.copy()
    if zero_t:
        x0[:, 4:7] = 0.0
    nS = beta.shape[-1] if use_shape else 0
    Jj, Jc = [], []
    for kind, col in _columns(npose, nS, True):
        dj, dc = _column_o(om, x0, beta, R0, use_shape, pose_blend, want_cloud, kind, col, step, beta.ndim == 2, order)
        Jj.append(dj); Jc.append(dc)
    return np.stack(Jj, 1), (np.stack(Jc, 1) if want_cloud else None)


def joint_jacobian_o4(om, x, beta, R0, use_shape=True, pose_blend=True, step=1e-3):
    """Jj [F, K, nJ, 3] by fourth-order differences (Richardson on steps 1e-3 and 2e-3, at t = 0): truncation ~1e-13 of the fifth
    derivative, rounding ~5e-13 m -- what an f64 bound of 1e-7 of a column needs where the column itself is 1e-3 (theta = 2 pi:
    dR/da vanishes across the axis); second-order differences at 1e-6 carry 2e-10"""
    return dense_jacobian(om, x, beta, R0, use_shape, pose_blend, want_cloud=False, step=step, order=4)[0]


def ref_grad_scaled(om, x, beta, R0, G, H, use_shape, pose_blend, per_frame, want_beta, step=1e-6, order=2, zero_t=False,
                    cloud_extra=None):
    global _cloud_extra
    _cloud_extra = cloud_extra
    try:
        return _ref_grad_scaled(om, x, beta, R0, G, H, use_shape, pose_blend, per_frame, want_beta, step, order, zero_t)
    finally:
        _cloud_extra = None


def _ref_grad_scaled(om, x, beta, R0, G, H, use_shape, pose_blend, per_frame, want_beta, step, order, zero_t):
    """J^T [G; H] by central differences of the checker's forward (model_variants.ref_grad's numbers), and with every entry
    its scale and the differences' own error:
      g   gx [F, npose], gb ([F, nS] per frame, [nS] shared, None without want_beta)
      S   S_fc = sum_i |G_fi| |dcloud_fi / dx_c| + sum |H| |djoints / dx_c| (a shared beta: summed over the frames)
      CD  |g(step) - g(2 step)|: an estimate of g's own error (three times its truncation term, its rounding term)
    (ref_grad_scaled; cloud_extra: x -> [F, V, 3] added to the checker's cloud at every point, for a forward that is the
    checker's plus a term of the test's own)"""
    F, npose = x.shape
    R0 = np.asarray(R0).reshape(F, 9)
    x0 = x.copy()
    if zero_t:
        x0[:, 4:7] = 0.0
    want_cloud = G is not None
    G64 = G.astype(np.float64) if want_cloud else None

    def contract(dj, dc):
        g, S = np.zeros(F), np.zeros(F)
        if want_cloud:
            g += np.einsum("fvc,fvc->f", G64, dc)
            S += np.einsum("fvc,fvc->f", np.abs(G64), np.abs(dc))
        if H is not None:
            g += np.einsum("fjc,fjc->f", H, dj)
            S += np.einsum("fjc,fjc->f", np.abs(H), np.abs(dj))
        return g, S

    def col(kind, c):
        g1, S = contract(*_column_o(om, x0, beta, R0, use_shape, pose_blend, want_cloud, kind, c, step, per_frame, order))
        g2, _ = contract(*_column_o(om, x0, beta, R0, use_shape, pose_blend, want_cloud, kind, c, 2 * step, per_frame, order))
        return g1, S, g2

    gx, Sx, CDx = np.zeros((F, npose)), np.zeros((F, npose)), np.zeros((F, npose))
    for c in range(npose):
        g1, S, g2 = col("x", c)
        gx[:, c], Sx[:, c], CDx[:, c] = g1, S, np.abs(g1 - g2)
    gb = Sb = CDb = None
    if want_beta:
        nS = beta.shape[-1]
        shape = (F, nS) if per_frame else (nS,)
        gb, Sb, CDb = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        for k in range(nS):
            g1, S, g2 = col("b", k)
            if per_frame:
                gb[:, k], Sb[:, k], CDb[:, k] = g1, S, np.abs(g1 - g2)
            else:
                gb[k], Sb[k], CDb[k] = g1.sum(), S.sum(), abs(g1.sum() - g2.sum())
    return SimpleNamespace(gx=gx, gb=gb, Sx=Sx, Sb=Sb, CDx=CDx, CDb=CDb)


def first_order_slack(om, x, beta, R0, H, use_shape=True, pose_blend=True):
    """[F, npose]: what the first-order Rodrigues branch adds to the error of a JOINTS gradient, per column.  A rotation with
    0 < theta^2 <= DBL_EPSILON is taken as R = I + [a]x with dR_c = [e_c]x (frame_part_inl.h, the checker and the reference's
    Ceres alike); the exponential's derivative is [e_c]x + (e_c a^T + a e_c^T) / 2 - a_c I + O(theta^2), at most 2 theta away
    in norm.  A joint i below the rotation moves by s Rr0 A_p dR_c u with |u| its distance to the rotating joint over s, so
    the column is off by at most 2 theta D_f sum_i |H_fi|_1, D_f the diameter of the posed skeleton (root: about the camera-
    frame origin of the body, the same bound).  Zero elsewhere."""
    F, npose = x.shape
    j, _ = om.forward_batch(x, beta, np.asarray(R0).reshape(F, 9), use_shape, pose_blend, want_cloud=False)
    D = np.sqrt(((j[:, :, None, :] - j[:, None, :, :]) ** 2).sum(-1)).reshape(F, -1).max(1)
    h1 = np.abs(H).reshape(F, -1).sum(1) if H is not None else np.ones(F)     # (H = None: per entry of a joint tangent)
    out = np.zeros((F, npose))
    for c0 in [1] + list(range(7, npose, 3)):
        th2 = (x[:, c0:c0 + 3] ** 2).sum(1)
        branch = (th2 > 0.0) & (th2 <= np.finfo(np.float64).eps)
        out[:, c0:c0 + 3] = (branch * 2.0 * np.sqrt(th2) * D * h1)[:, None]
    return out


VJP_REL = 2.0 ** -14    # each operand of the bf16 hi + lo split carries 16 significant bits, so a product term is off by at
                        # most 2^-15 relative; a factor 2 for the f32 accumulation and the f32 skinning adjoint


def row_max_ok(g, g_ref, tol=1e-4):
    """the suite's first VJP bound: every entry within tol of its frame's largest entry"""
    g, g_ref = np.atleast_2d(g), np.atleast_2d(g_ref)
    return bool((np.abs(g - g_ref) <= tol * np.abs(g_ref).max(1, keepdims=True)).all())


def column_ratios(g, g_ref, S, CD, rel=VJP_REL, add_cd=True, ref_share=0.1, slack=0.0):
    """|g - g_ref| / (rel S + CD) per entry (0 where both are 0), and whether the reference is good enough for the bound:
    its own error CD at most ref_share of it.  add_cd = False: the bound is rel S alone.  slack: added to the bound
    (first_order_slack)."""
    err = np.abs(np.asarray(g, np.float64) - g_ref)
    bound = rel * np.asarray(S) + (np.asarray(CD) if add_cd else 0.0) + slack
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
    return ratio, bool((np.asarray(CD) <= ref_share * bound).all())


def check_columns(g, g_ref, S, CD, rel=VJP_REL, what="vjp", add_cd=True, ref_share=0.1, slack=0.0):
    """asserts the per-column bound |g - g_ref| <= rel S + CD (+ slack) entry by entry; returns the worst error / bound"""
    ratio, ref_ok = column_ratios(g, g_ref, S, CD, rel, add_cd, ref_share, slack)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: worst column error / bound = {worst:.3e} (bound {rel:.2e} S{' + CD' if add_cd else ''})")
    assert ref_ok, (what, f"the differences' own error exceeds {ref_share} of the bound")
    assert worst <= 1.0, (what, worst, np.argwhere(ratio > 1.0)[:4].tolist())
    return worst
