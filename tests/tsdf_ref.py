"""The definition of bodyfit_volume_integrate_device (include/bodyfit.h) in numpy longdouble: one frame's step at one voxel with its
exact decisions and, for the checker, every decision vector that the header's bands admit; check_voxel, which accepts a result
iff it is the outcome of one admissible vector within the header's bound; the reference's own f32 stepping (fuse); the shared
case generator; and simulate, a plain f64 restatement with switches that break it one way at a time (what the checker must
reject).  Nothing here mirrors the kernel's order of operations: the bands and the bound of the header carry the difference."""
import math
import types

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -24
GRIDS = [(1, 1, 1), (2, 1, 3), (5, 4, 3), (17, 9, 6)]          # the sampler's; the last spans several workgroups
IMAGES = [(1, 1), (7, 9), (33, 17)]                            # (H, W)
CLASSES = ("behind", "outside", "hole", "hidden", "band", "free")
HOLES = (0.0, -1.0, np.nan, np.inf, -np.inf)


def make_case(dims, origin, spacing, intr, poses, depth, trunc, z_near):
    """poses: a list with one entry per frame, each 12 f64 ([A | t] row-major) or None"""
    depth = np.ascontiguousarray(depth, np.float32)
    assert depth.ndim == 3 and len(poses) == depth.shape[0]
    return types.SimpleNamespace(dims=tuple(int(n) for n in dims), origin=tuple(float(a) for a in origin),
                                 spacing=tuple(float(a) for a in spacing), intr=tuple(float(a) for a in intr),
                                 poses=[None if p is None else np.asarray(p, np.float64).reshape(12) for p in poses], depth=depth,
                                 trunc=float(trunc), z_near=float(z_near))


def pose_array(case):
    """[F, 12] f64 with the identity written out where a frame has no pose"""
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
    return np.stack([eye if p is None else p for p in case.poses])


# ---- the definition at one voxel --------------------------------------------------------------------------------------------------
def _pixel_candidates(x, band, n):
    """the indices floor(x + 1/2 + e), |e| <= band, each inside [0, n - 1] or None (outside the image)"""
    if not np.isfinite(x):
        return [None]
    out = []
    for e in (-band, LD(0), band):
        c = np.floor(x + LD(0.5) + e)
        c = int(c) if 0 <= c <= n - 1 else None
        if c not in out:
            out.append(c)
    return out


def voxel_step(case, f, index):
    """Frame f at voxel index = (i, j, k): .cls, the class of the EXACT decisions (one of CLASSES); .update / .sbar, the exact
    outcome; .admissible, a list of (key, update, sbar, delta_4) over every decision vector within the header's bands (a), (b)."""
    o, sp = [LD(a) for a in case.origin], [LD(a) for a in case.spacing]
    p = [o[a] + LD(index[a]) * sp[a] for a in range(3)]
    P = [abs(o[a]) + LD(index[a]) * sp[a] for a in range(3)]
    pose = case.poses[f]
    if pose is None:
        q, S = p, P
    else:
        A = [LD(x) for x in pose]
        q = [A[4 * r] * p[0] + A[4 * r + 1] * p[1] + A[4 * r + 2] * p[2] + A[4 * r + 3] for r in range(3)]
        S = [abs(A[4 * r]) * P[0] + abs(A[4 * r + 1]) * P[1] + abs(A[4 * r + 2]) * P[2] + abs(A[4 * r + 3]) for r in range(3)]
    fx, fy, cx, cy = [LD(a) for a in case.intr]
    H, W = case.depth.shape[1:]
    trunc, z_near = LD(case.trunc), LD(case.z_near)
    front = bool(q[2] > z_near)
    fronts = [front]
    if abs(q[2] - z_near) <= LD(2.0) ** -50 * S[2]:
        fronts.append(not front)

    def after_pixel(pi, pj, exact):
        """the vectors behind decision 2 at pixel (pi, pj); exact: the definition's decisions only"""
        if pi is None or pj is None:
            return [(("outside",), False, None, LD(0))]
        d = case.depth[f, pi, pj]
        if not (np.isfinite(d) and d > 0):
            return [(("hole", pi, pj), False, None, LD(0))]
        s = LD(d) - q[2]
        d4 = LD(2.0) ** -50 * (S[2] + min(LD(d), 2 * (S[2] + trunc)))
        shown = bool(s >= -trunc)
        both = [shown] if exact or abs(s + trunc) > d4 else [shown, not shown]
        return [(("update", pi, pj), True, min(s, trunc), d4) if b else (("hidden", pi, pj), False, None, LD(0)) for b in both]

    out = types.SimpleNamespace()
    # the exact decisions
    if not front:
        out.cls, out.update, out.sbar = "behind", False, None
    else:
        with np.errstate(all="ignore"):
            u, v = fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy
        cj = np.floor(u + LD(0.5)) if np.isfinite(u) else LD(-1)
        ci = np.floor(v + LD(0.5)) if np.isfinite(v) else LD(-1)
        inside = 0 <= ci <= H - 1 and 0 <= cj <= W - 1
        key, out.update, out.sbar, _ = after_pixel(int(ci) if inside else None, int(cj) if inside else None, True)[0]
        out.cls = key[0] if key[0] != "update" else ("free" if LD(case.depth[f, int(ci), int(cj)]) - q[2] >= trunc else "band")
    # every admissible vector
    vectors = {}
    for fr in fronts:
        if not fr:
            vectors[("behind",)] = (("behind",), False, None, LD(0))
            continue
        if not q[2] >= LD(2.0) ** -40 * S[2]:                  # (b): the pixel is not constrained
            ic, jc = list(range(H)) + [None], list(range(W)) + [None]
        else:
            u, v = fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy
            bu = LD(2.0) ** -49 * (abs(fx) * (S[0] + abs(q[0] / q[2]) * S[2]) / q[2] + abs(u) + abs(cx) + 1)
            bv = LD(2.0) ** -49 * (abs(fy) * (S[1] + abs(q[1] / q[2]) * S[2]) / q[2] + abs(v) + abs(cy) + 1)
            ic, jc = _pixel_candidates(v, bv, H), _pixel_candidates(u, bu, W)
        for pi in ic:
            for pj in jc:
                for vec in after_pixel(pi, pj, False):
                    vectors[vec[0]] = vec
    out.admissible = list(vectors.values())
    return out


def all_steps(case, f):
    """voxel_step of frame f at every voxel, x fastest: the order of the volume's memory"""
    nx, ny, nz = case.dims
    return [voxel_step(case, f, (i, j, k)) for k in range(nz) for j in range(ny) for i in range(nx)]


def observed(D, W):
    return bool(W > 0) and bool(np.isfinite(D))


def outcome(D, W, update, sbar, max_weight):
    """The definition's next state of a voxel (D, W f32): (D' longdouble BEFORE its rounding or None: unobserved, W' f32), and
    `kept`: the state is the prior one, bit for bit."""
    seen = observed(D, W)
    if not update:
        return (LD(D), np.float32(W), True) if seen else (None, np.float32(0), False)
    W0, D0 = (LD(W), LD(D)) if seen else (LD(0), LD(0))
    return (W0 * D0 + sbar) / (W0 + 1), np.float32(min(W0 + 1, LD(max_weight))), False


def check_voxel(D, W, got_D, got_W, step, max_weight):
    """(None, error / bound) if (got_D, got_W) is the one-frame step from (D, W) for one admissible vector of `step` within the
    header's bound (c), else (what it breaks, None)."""
    D, W, got_D, got_W = np.float32(D), np.float32(W), np.float32(got_D), np.float32(got_W)
    seen = observed(D, W)
    why = "no admissible vector"
    for key, update, sbar, d4 in step.admissible:
        want_D, want_W, kept = outcome(D, W, update, sbar, max_weight)
        if want_D is None:
            if np.isnan(got_D) and got_W == 0:
                return None, 0.0
            why = f"{key}: unobserved, but got ({got_D!r}, {got_W!r})"
        elif kept:
            if got_D.view(np.uint32) == D.view(np.uint32) and got_W.view(np.uint32) == W.view(np.uint32):
                return None, 0.0
            why = f"{key}: the state ({D!r}, {W!r}) was to stay, got ({got_D!r}, {got_W!r})"
        else:
            W0, D0 = (LD(W), LD(D)) if seen else (LD(0), LD(0))
            bound = U * abs(want_D) + d4 / (W0 + 1) + LD(2.0) ** -50 * (abs(D0) + abs(sbar)) + LD(2.0) ** -149
            if got_W.view(np.uint32) != want_W.view(np.uint32):
                why = f"{key}: weight {got_W!r} against {want_W!r}"
            elif not np.isfinite(got_D) or abs(LD(got_D) - want_D) > bound:
                why = f"{key}: distance {got_D!r} against {float(want_D)!r}"
            else:
                return None, float(abs(LD(got_D) - want_D) / bound)
    return why, None


def fuse(case, frames, max_weight=np.inf, state=None, steps=None):
    """The reference's own stepping: the EXACT decisions of `frames` (ascending) applied to state = (D, W) f32 [nz, ny, nx] (None:
    empty), both rounded to f32 after every frame.  Returns new (D, W)."""
    nx, ny, nz = case.dims
    if state is None:
        D, W = np.full(nx * ny * nz, np.nan, np.float32), np.zeros(nx * ny * nz, np.float32)
    else:
        D, W = (np.array(a, np.float32).reshape(-1) for a in state)
    for f in frames:
        st = steps[f] if steps is not None else all_steps(case, f)
        for n, step in enumerate(st):
            d, w, _ = outcome(D[n], W[n], step.update, step.sbar, max_weight)
            D[n], W[n] = (np.float32(np.nan), np.float32(0)) if d is None else (np.float32(d), w)
    return D.reshape(nz, ny, nx), W.reshape(nz, ny, nx)


# ---- a plain f64 restatement, and the ways to break it -------------------------------------------------------------------------------
MUTATIONS = ("transposed", "floor", "swapped", "sign", "cap", "zeros", "hidden")


def simulate(case, f, D, W, max_weight, mutate=None):
    """One frame in vectorised f64 numpy from (D, W) f32 [nz, ny, nx]: new (D, W).  mutate: None or one of MUTATIONS: transposed
    volume axes, floor(u) in place of floor(u + 1/2), u and v swapped, a flipped sign, the cap ignored, unobserved voxels written
    as 0, hidden voxels updated."""
    nx, ny, nz = case.dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if mutate == "transposed":
        i, k = k, i
    p = [case.origin[0] + i * case.spacing[0], case.origin[1] + j * case.spacing[1], case.origin[2] + k * case.spacing[2]]
    A = pose_array(case)[f]
    q = [A[4 * r] * p[0] + A[4 * r + 1] * p[1] + A[4 * r + 2] * p[2] + A[4 * r + 3] for r in range(3)]
    fx, fy, cx, cy = case.intr
    H, Wd = case.depth.shape[1:]
    with np.errstate(all="ignore"):
        u, v = fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy
        if mutate == "swapped":
            u, v = v, u
        half = 0.0 if mutate == "floor" else 0.5
        cj, ci = np.floor(u + half), np.floor(v + half)
        hit = (q[2] > case.z_near) & (cj >= 0) & (cj <= Wd - 1) & (ci >= 0) & (ci <= H - 1)
        d = case.depth[f][np.where(hit, ci, 0).astype(np.int64), np.where(hit, cj, 0).astype(np.int64)].astype(np.float64)
        s = d - q[2]
        upd = hit & np.isfinite(d) & (d > 0) & ((s >= -case.trunc) | (mutate == "hidden"))
        sb = np.clip(s, -np.inf if mutate != "hidden" else -case.trunc, case.trunc)
        if mutate == "sign":
            sb = -sb
        D, W = np.asarray(D, np.float32), np.asarray(W, np.float32)
        seen = (W > 0) & np.isfinite(D)
        W0 = np.where(seen, W, 0).astype(np.float64)
        WD = np.where(seen, W.astype(np.float64) * np.where(seen, D, 0).astype(np.float64), 0.0)
        Dn = ((WD + sb) / (W0 + 1)).astype(np.float32)
        Wn = (W0 + 1 if mutate == "cap" else np.minimum(W0 + 1, max_weight)).astype(np.float32)
    empty = (np.float32(0), np.float32(0)) if mutate == "zeros" else (np.float32(np.nan), np.float32(0))
    return (np.where(upd, Dn, np.where(seen, D, empty[0])).astype(np.float32),
            np.where(upd, Wn, np.where(seen, W, empty[1])).astype(np.float32))


# ---- the shared cases -------------------------------------------------------------------------------------------------------------
ORIGIN = (-0.07, -0.11, 0.5)
SPACING = (0.03, 0.05, 0.02)
TRUNC, Z_NEAR, MAX_WEIGHT = 0.015, 0.1, 4.0
N_FRAMES = 3                                                   # one per pose


def rigid(rng, angle, shift):
    """a rigid motion [A | t] as 12 f64: a rotation by `angle` about a random axis, about the origin, then a shift"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    return np.concatenate([R, np.asarray(shift, np.float64).reshape(3, 1)], axis=1).reshape(12)


def random_case(dims, image, seed):
    """Three frames of a H x W camera in front of a dims volume: the identity, a small rigid motion, and one that puts part of the
    volume behind z_near.  The depth maps are smooth surfaces through the middle of the volume (so that voxels fall in front of
    the band, inside it and behind it) with holes of every kind; the image is a little smaller than the volume's projection."""
    rng = np.random.default_rng(seed)
    H, W = image
    ext = [max((n - 1) * s, s) for n, s in zip(dims, SPACING)]
    mid = [o + 0.5 * (n - 1) * s for o, n, s in zip(ORIGIN, dims, SPACING)]
    fx, fy = 0.75 * W * mid[2] / ext[0], 0.75 * H * mid[2] / ext[1]
    intr = (fx, fy, 0.5 * (W - 1) + 0.13 - fx * mid[0] / mid[2], 0.5 * (H - 1) - 0.21 - fy * mid[1] / mid[2])
    # the second pose turns about the volume's middle: R (p - mid) + mid + shift
    small = rigid(rng, 0.08, (0, 0, 0))
    R = small.reshape(3, 4)[:, :3]
    small = np.concatenate([R, (np.array(mid) - R @ np.array(mid) + rng.uniform(-0.01, 0.01, size=3)).reshape(3, 1)], axis=1).reshape(12)
    back = rigid(rng, 0.05, (0, 0, 0))
    R = back.reshape(3, 4)[:, :3]
    zc = Z_NEAR + 0.1 * ext[2]                                  # the plane q_z = z_near cuts the volume; its middle stays on its pixel
    shift = np.array([mid[0] * (zc / mid[2] - 1), mid[1] * (zc / mid[2] - 1), zc - mid[2]])
    back = np.concatenate([R, (np.array(mid) - R @ np.array(mid) + shift).reshape(3, 1)], axis=1).reshape(12)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.empty((N_FRAMES, H, W), np.float32)
    for f in range(N_FRAMES):
        a, b = rng.uniform(-0.4, 0.4, size=2) * ext[2]
        depth[f] = (mid[2] + a * np.sin(1.3 * i / max(H - 1, 1) + f) + b * np.cos(2.1 * j / max(W - 1, 1)) + 0.1 * ext[2] * (f - 1))
        holes = rng.uniform(size=(H, W)) < 0.2
        depth[f][holes] = rng.choice(np.array(HOLES, np.float32), size=int(holes.sum()))
    if H * W == 1:                                              # one pixel: a surface, a hole, a surface
        depth[:, 0, 0] = [mid[2], np.nan, mid[2] + 0.3 * ext[2]]
    return make_case(dims, ORIGIN, SPACING, intr, [None, small, back], depth, TRUNC, Z_NEAR)


def boundary_case():
    """Dyadic numbers, the identity: every quantity of the definition is exact in f64, and so is the kernel's.  Voxel centres x =
    i / 8 at z = 1 project to u = 4 x + 1 = i / 2 + 1: on a pixel boundary for odd i; the layers z = 7/8, 1, 9/8 under a constant
    depth 1 with trunc 1/8 and z_near 7/8 hold q_z = z_near exactly and s = -trunc exactly."""
    depth = np.ones((1, 4, 8), np.float32)
    depth[0, 2, 3] = 0.0                                        # beside a boundary: the two admissible pixels differ
    return make_case((9, 3, 3), (0.0, 0.0, 0.875), (0.125, 0.125, 0.125), (4.0, 4.0, 1.0, 1.0), [None], depth, 0.125, 0.875)


def dyadic_case(n_frames, depths, translation=None, trunc=0.25):
    """an identity (or purely translated) camera over a dyadic grid under constant dyadic depths: every voxel projects inside"""
    dims, origin, spacing = (5, 4, 6), (-0.25, -0.25, 1.0), (0.125, 0.125, 0.125)
    depth = np.stack([np.full((33, 33), z, np.float32) for z in depths])
    pose = None if translation is None else np.array([1, 0, 0, translation[0], 0, 1, 0, translation[1], 0, 0, 1, translation[2]], np.float64)
    return make_case(dims, origin, spacing, (16.0, 16.0, 16.0, 16.0), [pose] * n_frames, depth, trunc, 0.5)


def grid_z(case):
    nx, ny, nz = case.dims
    z = case.origin[2] + case.spacing[2] * np.arange(nz)
    return np.broadcast_to(z[:, None, None], (nz, ny, nx))


PRIORS = ("unobserved", "observed", "weight without a distance", "at the cap")


def prior_state(kind, dims, seed):
    """(D, W) f32 [nz, ny, nx] of one of PRIORS, with junk where the definition does not look"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    D = rng.uniform(-TRUNC, TRUNC, size=shape).astype(np.float32)
    if kind == "unobserved":                                    # W = 0, -1 or NaN with any D
        W = rng.choice(np.array([0.0, -1.0, np.nan], np.float32), size=shape)
    elif kind == "observed":
        W = rng.integers(1, int(MAX_WEIGHT), size=shape).astype(np.float32)
    elif kind == "weight without a distance":
        W = np.full(shape, 2.0, np.float32)
        D = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=shape)
    elif kind == "at the cap":
        W = np.full(shape, MAX_WEIGHT, np.float32)
    else:
        raise ValueError(kind)
    return D, W
