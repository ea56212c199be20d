"""Plain numpy f64 reference of bodyfit_surface_gram_device's contract (include/bodyfit.h): per frame, row by row, the 3 x P
Jacobian A_i of the row's surface point, then H = sum w A^T D A, its bound term H^ (every factor by absolute value, the dot
products expanded) and g = J^T rhs with g^.  gram_w_form computes the same H through the per-face moments and W (the form the
kernel relies on); the CPU test pins the two against each other."""
import numpy as np

EPS_H = 2.0 ** -12      # the header's derived bounds
EPS_G = 2.0 ** -32


def frame_rows(F, n_rows, offset=None):
    """[(first row, one past the last)] per frame of a uniform (n_rows per frame) or ragged (offset [F + 1]) set"""
    if offset is None:
        return [(f * n_rows, (f + 1) * n_rows) for f in range(F)]
    return [(int(offset[f]), int(offset[f + 1])) for f in range(F)]


def gram_reference(jac, faces, rows, index, bary, weight=None, direction=None, rhs=None):
    """jac [F, P, V, 3], faces [n_faces, 3], rows: frame_rows(...), index [N], bary [N, 3], weight [N] or None, direction [N, 3] or
    None, rhs [F, V, 3] or None  ->  H, H^ [F, P, P], g, g^ [F, P] (None without rhs), all f64"""
    J = np.asarray(jac, np.float64)
    F, P, V, _ = J.shape
    faces = np.asarray(faces).reshape(-1, 3)
    Ja = np.abs(J)
    H = np.zeros((F, P, P)); Hh = np.zeros((F, P, P))
    for f, (r0, r1) in enumerate(rows):
        for i in range(r0, r1):
            t = int(index[i])
            if t < 0 or t >= len(faces):
                continue
            w = 1.0 if weight is None else float(weight[i])
            if w == 0.0:
                continue
            b = np.asarray(bary[i], np.float64)
            ids = faces[t]
            A = np.einsum("a,pax->px", b, J[f][:, ids, :])                    # [P, 3]
            Aa = np.einsum("a,pax->px", np.abs(b), Ja[f][:, ids, :])
            if direction is None:
                H[f] += w * (A @ A.T)
                Hh[f] += abs(w) * (Aa @ Aa.T)
            else:
                d = np.asarray(direction[i], np.float64)
                s, sa = A @ d, Aa @ np.abs(d)
                H[f] += w * np.outer(s, s)
                Hh[f] += abs(w) * np.outer(sa, sa)
    g = gh = None
    if rhs is not None:
        R = np.asarray(rhs, np.float64)
        g = np.einsum("fpvx,fvx->fp", J, R)
        gh = np.einsum("fpvx,fvx->fp", Ja, np.abs(R))
    return H, Hh, g, gh


def gram_w_form(jac, faces, rows, index, bary, weight=None, direction=None):
    """H through the moments: M_t[a][c] = sum_{i -> t} w_i b_ia b_ic D_i, W (3 V x 3 V) assembled from them, J^T W J"""
    J = np.asarray(jac, np.float64)
    F, P, V, _ = J.shape
    faces = np.asarray(faces).reshape(-1, 3)
    H = np.zeros((F, P, P))
    for f, (r0, r1) in enumerate(rows):
        M = np.zeros((len(faces), 3, 3, 3, 3))
        for i in range(r0, r1):
            t = int(index[i])
            if t < 0 or t >= len(faces):
                continue
            w = 1.0 if weight is None else float(weight[i])
            b = np.asarray(bary[i], np.float64)
            d = None if direction is None else np.asarray(direction[i], np.float64)
            D = np.eye(3) if d is None else np.outer(d, d)
            M[t] += w * np.einsum("a,c,xy->acxy", b, b, D)
        W = np.zeros((V, 3, V, 3))
        for t, ids in enumerate(faces):
            for a in range(3):
                for c in range(3):
                    W[ids[a], :, ids[c], :] += M[t, a, c]
        Jf = J[f].reshape(P, 3 * V)
        H[f] = Jf @ W.reshape(3 * V, 3 * V) @ Jf.T
    return H
