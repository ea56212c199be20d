"""Test infrastructure (numpy): the reference statement of torch_layer.SilhouetteTerm, both halves, with the gradient per vertex
component.  It takes the render's (face, lambda, z^), the visibility and the two `nearest` images AS GIVEN: it states the term's
composition and summation, not the z-buffer's tie rules or the distance transform a second time (tests/raster_ref.py and
tests/edt_ref.py do that).

evaluate(..., dtype=np.longdouble) runs the same statement in extended precision: the difference to the float64 run is the
rounding of the elementwise operations, which is what measure_constants() reports in units of eps = 2^-53 times the scales
below, and what the GPU test's tolerance for the torch side of the term is taken from."""
import numpy as np

U32 = 2.0 ** -24
EPS = 2.0 ** -53


def evaluate(verts, faces, intr, mask, nearest_s, face, bary, depth, visible, nearest_m, trunc=None, dtype=np.float64):
    """verts f32 [F, V, 3]; faces int [n_faces, 3]; mask bool [F, H, W]; nearest_s, nearest_m int [F, H, W]; face int, bary
    [F, H, W, 3], depth [F, H, W]: one render; visible bool [F, V].  Returns a dict:
      cost_md, grad_md [F, V, 3], scale_md [F, V, 3], rho_md [F, V], scale_rho [F, V], scale_value_md = sum scale_rho
                                                                       the model -> data half, per vertex and summed, and the
                                                                       magnitudes its elementwise roundings are relative to
      sum_dist2 (int), n_truncated (int), cost_dm, grad_dm, abs_dm [F, V, 3]   the data -> model half from rows in full
                                                                       precision, abs_dm the sum of the terms' absolute values
      n_pulled, n_rows"""
    T = dtype
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = verts.shape[:2]
    H, W = mask.shape[1:]
    fx, fy, cx, cy = (T(a) for a in intr)
    cap = None if trunc is None else T(trunc) * T(trunc)
    out = {}
    # ---- model -> data
    grad_md, scale_md = np.zeros((F, V, 3), T), np.zeros((F, V, 3), T)
    rho_md, scale_rho = np.zeros((F, V), T), np.zeros((F, V), T)
    cost_md, scale_value, n_pulled = T(0), T(0), 0
    for f in range(F):
        ids = np.nonzero(visible[f])[0]
        if len(ids) == 0:
            continue
        p = verts[f, ids].astype(T)
        X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
        u = fx * X / Z + cx
        v = fy * Y / Z + cy
        i, j = np.floor(v + T(0.5)), np.floor(u + T(0.5))
        inside = (i >= 0) & (i < H) & (j >= 0) & (j < W)
        ic, jc = np.clip(i, 0, H - 1).astype(np.int64), np.clip(j, 0, W - 1).astype(np.int64)
        s = nearest_s[f, ic, jc].astype(np.int64)
        pull = inside & ~mask[f, ic, jc] & (s >= 0)
        i_s, j_s = np.divmod(np.maximum(s, 0), W)
        e_u, e_v = u - j_s.astype(T), v - i_s.astype(T)
        e2 = e_u * e_u + e_v * e_v
        live = pull & (e2 <= cap) if cap is not None else pull      # (torch.clamp passes the gradient at the cap itself)
        rho_md[f, ids] = np.where(pull, e2 if cap is None else np.minimum(e2, cap), T(0))
        cost_md += rho_md[f, ids].sum()
        w = np.where(live, T(2), T(0))
        g = np.stack((w * e_u * fx / Z, w * e_v * fy / Z, -w * (e_u * fx * X + e_v * fy * Y) / (Z * Z)), axis=1)
        grad_md[f, ids] = g
        P = np.abs(u) + np.abs(v) + abs(cx) + abs(cy) + T(W + H)
        pl = pull.astype(T)
        scale_md[f, ids] = np.stack((2 * pl * P * fx / Z, 2 * pl * P * fy / Z,
                                     2 * pl * P * (fx * np.abs(X) + fy * np.abs(Y)) / (Z * Z)), axis=1)
        scale_rho[f, ids] = pl * (2 * P * (np.abs(e_u) + np.abs(e_v)) + e2)
        scale_value += scale_rho[f, ids].sum()
        n_pulled += int(pull.sum())
    out.update(cost_md=cost_md, grad_md=grad_md, scale_md=scale_md, rho_md=rho_md, scale_rho=scale_rho,
               scale_value_md=scale_value, n_pulled=n_pulled)
    # ---- data -> model
    grad_dm, abs_dm = np.zeros((F, V, 3), T), np.zeros((F, V, 3), T)
    sum_d2, n_cut, n_rows = 0, 0, 0
    for f in range(F):
        rows = mask[f] & (face[f] < 0) & (nearest_m[f] >= 0)
        i, j = np.nonzero(rows)
        if len(i) == 0:
            continue
        i_t, j_t = np.divmod(nearest_m[f, i, j].astype(np.int64), W)
        k = face[f, i_t, j_t].astype(np.int64)
        assert (k >= 0).all(), "nearest_M names an empty pixel"
        z = depth[f, i_t, j_t].astype(T)
        corners = faces[k]                                           # [N, 3]
        Z = verts[f][corners, 2].astype(T)
        beta = bary[f, i_t, j_t].astype(T) * z[:, None] / Z
        d2 = (i_t - i) ** 2 + (j_t - j) ** 2                        # the row's value: an integer
        keep = d2.astype(T) < cap if cap is not None else np.ones(len(i), bool)
        sum_d2 += int(d2[keep].sum())
        n_cut += int((~keep).sum())
        n_rows += len(i)
        e_u, e_v = (j_t - j).astype(T), (i_t - i).astype(T)
        w = T(2) * keep.astype(T) / z
        m = np.stack((fx * e_u * w, fy * e_v * w, -(e_u * (j_t.astype(T) - cx) + e_v * (i_t.astype(T) - cy)) * w), axis=1)
        terms = beta[:, :, None] * m[:, None, :]                    # [N, corner, 3]
        np.add.at(grad_dm[f], corners.reshape(-1), terms.reshape(-1, 3))
        np.add.at(abs_dm[f], corners.reshape(-1), np.abs(terms).reshape(-1, 3))
    cost_dm = T(sum_d2) + (cap * n_cut if cap is not None else T(0))
    out.update(sum_dist2=sum_d2, n_truncated=n_cut, cost_dm=cost_dm, grad_dm=grad_dm, abs_dm=abs_dm, n_rows=n_rows)
    return out


def measure_constants(*args, **kwargs):
    """(c_grad, c_value): the float64 statement against the extended-precision one, model -> data half: the largest
    |grad64 - grad| / (eps scale_md) over the components, and the largest |rho64 - rho| / (eps scale_rho) over the vertices (per
    vertex, not of the sum, in which the roundings cancel)"""
    a = evaluate(*args, dtype=np.float64, **kwargs)
    b = evaluate(*args, dtype=np.longdouble, **kwargs)
    on = b["scale_md"] > 0
    c_grad = float((np.abs(a["grad_md"].astype(np.longdouble) - b["grad_md"])[on] / (EPS * b["scale_md"][on])).max()) if on.any() else 0.0
    on = b["scale_rho"] > 0
    c_value = float((np.abs(a["rho_md"].astype(np.longdouble) - b["rho_md"])[on] / (EPS * b["scale_rho"][on])).max()) if on.any() else 0.0
    return c_grad, c_value


def shifted(verts, scale, shift):
    """the pose the mask is rendered from: verts scaled about their centroid and shifted, f32"""
    v = np.asarray(verts, np.float64)
    c = v.mean(axis=-2, keepdims=True)
    return ((v - c) * scale + c + np.asarray(shift, np.float64)).astype(np.float32)
