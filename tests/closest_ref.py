"""Test infrastructure (numpy): the f64 brute-force reference of the closest-point search and of its gradient
(bodyfit_closest_points_device / bodyfit_closest_points_vjp_device), chunked so that it stays in memory, and the f32
difference-form evaluation that shows the bounds of include/bodyfit.h are attainable.

A point set is a list of per-frame arrays [n_f, 3] float32 (frames may be empty)."""
import numpy as np

CHUNK = 512

# bounds of include/bodyfit.h (bodyfit_closest_points_device)
ARGMIN_SLACK = 2.0 ** -19     # D(index) <= (1 + 2^-19) min_v D(v)
DIST2_REL = 2.0 ** -20        # |dist2 - D(index)| <= 2^-20 D(index)


def split_frames(xyz, offset):
    """per-frame views of a packed [N, 3] array with a CSR offset [F + 1]"""
    return [xyz[offset[f]:offset[f + 1]] for f in range(len(offset) - 1)]


def exact_dist2(q, r):
    """D: exact squared distances [nq, nr] of f32 points, in f64 (the differences of f32 numbers are exact in f64)"""
    d = q.astype(np.float64)[:, None, :] - r.astype(np.float64)[None, :, :]
    return np.einsum("qrc,qrc->qr", d, d)


def brute_force(q, r):
    """(min_v D(v) [nq] f64, argmin [nq], lowest index among exact ties) of one frame; (+inf, -1) without reference points"""
    nq = q.shape[0]
    if r.shape[0] == 0:
        return np.full(nq, np.inf), np.full(nq, -1, np.int64)
    dmin = np.empty(nq)
    amin = np.empty(nq, np.int64)
    for s in range(0, nq, CHUNK):
        D = exact_dist2(q[s:s + CHUNK], r)
        a = D.argmin(axis=1)
        amin[s:s + CHUNK] = a
        dmin[s:s + CHUNK] = D[np.arange(D.shape[0]), a]
    return dmin, amin


def dist2_at(q, r, index):
    """D(index) [nq] f64; +inf where index is -1"""
    out = np.full(q.shape[0], np.inf)
    ok = index >= 0
    d = q[ok].astype(np.float64) - r[index[ok]].astype(np.float64)
    out[ok] = (d * d).sum(axis=1)
    return out


def diff_form_f32(q, r):
    """(dist2 [nq] f32, index [nq]) of the f32 difference form (px-cx)^2 + (py-cy)^2 + (pz-cz)^2, every operation rounded to
    f32 (no FMA: five roundings after the subtractions), lowest index among equal computed distances"""
    nq = q.shape[0]
    if r.shape[0] == 0:
        return np.full(nq, np.inf, np.float32), np.full(nq, -1, np.int64)
    d2 = np.empty(nq, np.float32)
    idx = np.empty(nq, np.int64)
    q = q.astype(np.float32); r = r.astype(np.float32)
    for s in range(0, nq, CHUNK):
        qq = q[s:s + CHUNK]
        dx = qq[:, None, 0] - r[None, :, 0]
        dy = qq[:, None, 1] - r[None, :, 1]
        dz = qq[:, None, 2] - r[None, :, 2]
        D = dx * dx + dy * dy + dz * dz
        assert D.dtype == np.float32
        a = D.argmin(axis=1)
        idx[s:s + CHUNK] = a
        d2[s:s + CHUNK] = D[np.arange(D.shape[0]), a]
    return d2, idx


def check_bounds(q, r, dist2, index):
    """Asserts the bounds of include/bodyfit.h for EVERY query of one frame; returns (worst argmin excess, worst dist2 error),
    both relative.  dist2 f32 [nq], index [nq] as the implementation under test returned them."""
    nq, nr = q.shape[0], r.shape[0]
    index = np.asarray(index).astype(np.int64)
    dist2 = np.asarray(dist2)
    if nr == 0:
        assert np.all(index == -1) and np.all(np.isposinf(dist2)), "a frame without reference points: -1, +inf"
        return 0.0, 0.0
    assert np.all((index >= 0) & (index < nr)), "index out of the frame's range"
    dmin, _ = brute_force(q, r)
    dsel = dist2_at(q, r, index)
    bad = dsel > (1.0 + ARGMIN_SLACK) * dmin
    assert not bad.any(), (int(bad.sum()), float((dsel[bad] / dmin[bad]).max()))
    err = np.abs(dist2.astype(np.float64) - dsel)
    bad = err > DIST2_REL * dsel
    assert not bad.any(), (int(bad.sum()), float((err[bad] / dsel[bad]).max()))
    pos = dmin > 0
    worst_a = float((dsel[pos] / dmin[pos]).max() - 1.0) if pos.any() else 0.0
    pos = dsel > 0
    worst_d = float((err[pos] / dsel[pos]).max()) if pos.any() else 0.0
    return worst_a, worst_d


def vjp(q, r, index, g):
    """Analytic f64 gradient of sum_i g_i dist2_i of one frame at a fixed correspondence:
    grad_q [nq, 3] = -2 g_i (c_index_i - p_i), grad_r [nr, 3] = sum_{i: index_i = v} 2 g_i (c_v - p_i),
    plus abs_r [nr, 3] = sum |2 g_i (c_v - p_i)| and n_r [nr] = queries per reference point (the error bound's terms).
    index -1 (or out of range): the query contributes nothing."""
    nq, nr = q.shape[0], r.shape[0]
    index = np.asarray(index).astype(np.int64)
    ok = (index >= 0) & (index < nr)
    gq = np.zeros((nq, 3)); gr = np.zeros((nr, 3)); ar = np.zeros((nr, 3)); n_r = np.zeros(nr, np.int64)
    if ok.any():
        t = 2.0 * g[ok].astype(np.float64)[:, None] * (r[index[ok]].astype(np.float64) - q[ok].astype(np.float64))
        gq[ok] = -t
        np.add.at(gr, index[ok], t)
        np.add.at(ar, index[ok], np.abs(t))
        np.add.at(n_r, index[ok], 1)
    return gq, gr, ar, n_r
