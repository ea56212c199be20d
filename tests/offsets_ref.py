"""numpy f64 restatement of the per-vertex offsets (SMPL+D) of include/bodyfit.h: with offsets d the cloud is

    cloud_v = cloud0_v + L_fv d_v,   L_fv = sum_j W_vj T_j[:, :3] = s R(rootAA) R0 sum_j W_vj A_j,   A_j = A_parent R_j, A_0 = I,

so delta = L d, dL/dd_v = sum_f L_fv^T G_fv (shared offsets) or L_fv^T G_fv (per frame); and the uniform mesh Laplacian of
bodyfit_surface_laplacian_device as a dense matrix.  Nothing here touches the library or the checker."""
import numpy as np


def rodrigues(aa):
    """exp of the skew matrix of aa (both branches agree to O(theta^2) at the switch)"""
    aa = np.asarray(aa, np.float64)
    th2 = float(aa @ aa)
    K = np.array([[0.0, -aa[2], aa[1]], [aa[2], 0.0, -aa[0]], [-aa[1], aa[0], 0.0]])
    if th2 > 1e-16:
        th = np.sqrt(th2)
        return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / th2) * (K @ K)
    return np.eye(3) + K + 0.5 * (K @ K)


def chain_rotations(parent, x):
    """A [nJ, 3, 3] of one frame's parameters x [7 + 3 (nJ - 1)]: A_0 = I, A_j = A_parent(j) R(aa_j), parents first"""
    nJ = len(parent)
    A = np.empty((nJ, 3, 3))
    A[0] = np.eye(3)
    done = {0}
    todo = list(range(1, nJ))
    while todo:                                  # (joint ids need not be topologically sorted)
        rest = []
        for j in todo:
            p = int(parent[j])
            if p in done:
                A[j] = A[p] @ rodrigues(x[7 + 3 * (j - 1): 10 + 3 * (j - 1)])
                done.add(j)
            else:
                rest.append(j)
        assert len(rest) < len(todo), "parent is not a tree"
        todo = rest
    return A


def blend_matrices(model, x, R0):
    """L [F, V, 3, 3]: the linear part of every vertex's blended skinning transform (x [F, 76], R0 [F, 3, 3] or [F, 9])"""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    R0 = np.asarray(R0, np.float64).reshape(F, 3, 3)
    W = np.asarray(model.weights, np.float64)
    L = np.empty((F, W.shape[0], 3, 3))
    for f in range(F):
        A = chain_rotations(model.parent, x[f])
        M = x[f, 0] * rodrigues(x[f, 1:4]) @ R0[f]
        L[f] = np.einsum("ab,vbc->vac", M, np.einsum("vj,jbc->vbc", W, A))
    return L


def _per_frame(d, F):
    d = np.asarray(d, np.float64)
    return np.broadcast_to(d, (F,) + d.shape[-2:]) if d.ndim == 2 else d


def delta(L, d):
    """delta [F, V, 3] = L_fv d_v for offsets d [V, 3] (shared) or [F, V, 3]"""
    return np.einsum("fvab,fvb->fva", L, _per_frame(d, L.shape[0]))


def grad_offsets(L, G, shared):
    """the exact dL/dd for dL/dcloud = G [F, V, 3]: [V, 3] summed over the frames (shared) or [F, V, 3]"""
    g = np.einsum("fvab,fva->fvb", L, np.asarray(G, np.float64))
    return g.sum(axis=0) if shared else g


def laplacian_dense(n_verts, faces):
    """L [V, V]: l_i = x_i - (1 / 2 n_i) sum over the n_i faces that hold i (each once, taken at i's first position in it) of
    the entries at the other two POSITIONS; a vertex without a face has a zero row"""
    faces = np.asarray(faces)
    L = np.zeros((n_verts, n_verts))
    count = np.zeros(n_verts, np.int64)
    for t in faces:
        for i in set(int(v) for v in t):
            count[i] += 1
    for t in faces:
        t = [int(v) for v in t]
        for i in set(t):
            c = t.index(i)
            for q in (1, 2):
                L[i, t[(c + q) % 3]] -= 1.0 / (2.0 * count[i])
    for i in range(n_verts):
        if count[i] > 0:
            L[i, i] += 1.0
    return L


def mesh_with_boundary(n=7):
    """(n_verts, faces): an n x n grid of vertices triangulated as an open sheet (a boundary all round), one face that repeats a
    corner, and one unreferenced vertex at the end"""
    ids = np.arange(n * n).reshape(n, n)
    a, b, c, d = ids[:-1, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, :-1].ravel(), ids[1:, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1), [[0, 0, 1]]]).astype(np.int32)
    return n * n + 1, faces
