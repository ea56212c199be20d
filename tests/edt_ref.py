"""Test infrastructure (numpy): the reference statement of the distance transform with the nearest seed
(bodyfit_raster_distance_device, include/bodyfit.h; csrc/k_edt.hip), the named masks the CPU and the GPU tests share, and a
plain-Python restatement of the separable integer algorithm the kernels run.

brute(mask) is the DEFINITION: the minimum over all (pixel, seed) pairs in int64.  kernel_form(mask) follows k_edt.hip step by
step (the row pass on 64-column words, Meijster's column pass with the floor division), so that the algorithm, its tie rule
and its boundary arithmetic are checked against the definition without a GPU."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def brute(mask):
    """dist2 int64 [H, W] of a bool [H, W] mask (True: a seed) by all pairs, chunked over the pixels; INT32_MAX without a seed"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    si, sj = np.nonzero(mask)
    if len(si) == 0:
        return np.full((H, W), INT32_MAX, np.int64)
    si, sj = si.astype(np.int64), sj.astype(np.int64)
    pi, pj = np.divmod(np.arange(H * W, dtype=np.int64), W)
    out = np.empty(H * W, np.int64)
    chunk = max(1, (1 << 20) // len(si))
    for a in range(0, H * W, chunk):
        di = pi[a:a + chunk, None] - si[None, :]
        dj = pj[a:a + chunk, None] - sj[None, :]
        out[a:a + chunk] = (di * di + dj * dj).min(axis=1)
    return out.reshape(H, W)


def _clz64(m):
    return 64 - m.bit_length()


def _ctz64(m):
    return (m & -m).bit_length() - 1


def row_pass(mask):
    """k_edt_rows: int [H, W], per pixel the seed column of its row nearest to it (ties: the left one), -1 in a row without"""
    H, W = mask.shape
    n_words = (W + 63) >> 6
    col = np.full((H, W), -1, np.int64)
    for i in range(H):
        words = [0] * n_words
        for j in np.nonzero(mask[i])[0]:
            words[j >> 6] |= 1 << (int(j) & 63)
        right, carry = [0] * n_words, -1
        for c in range(n_words - 1, -1, -1):
            right[c] = carry
            if words[c]:
                carry = c * 64 + _ctz64(words[c])
        carry = -1
        for c in range(n_words):
            m = words[c]
            for lane in range(min(64, W - c * 64)):
                j = c * 64 + lane
                below = m & (((2 << lane) - 1) & (2 ** 64 - 1))
                above = m >> lane
                l = c * 64 + 63 - _clz64(below) if below else carry
                r = j + _ctz64(above) if above else right[c]
                if l < 0:
                    pick = r
                elif r < 0:
                    pick = l
                else:
                    pick = l if j - l <= r - j else r
                col[i, j] = pick
            if m:
                carry = c * 64 + 63 - _clz64(m)
    return col


def column_pass(col):
    """k_edt_cols: (dist2, nearest) int64 [H, W] from the row pass's columns"""
    H, W = col.shape
    dist2 = np.full((H, W), INT32_MAX, np.int64)
    nearest = np.full((H, W), -1, np.int64)
    for j in range(W):
        stack = []                                        # (row s, first row t of its reign, seed column, g)
        for u in range(H):
            c = int(col[u, j])
            if c < 0:
                continue
            g = (j - c) * (j - c)
            while stack:
                s, t, _, tg = stack[-1]
                if (t - s) * (t - s) + tg <= (t - u) * (t - u) + g:
                    break
                stack.pop()
            w = 0
            if stack:
                s, _, _, tg = stack[-1]
                w = 1 + (u * u - s * s + g - tg) // (2 * (u - s))          # Python's // is the floor
                if w >= H:
                    continue
            stack.append((u, w, c, g))
        if not stack:
            continue
        for u in range(H - 1, -1, -1):
            s, t, c, g = stack[-1]
            dist2[u, j] = (u - s) * (u - s) + g
            nearest[u, j] = s * W + c
            if u == t:
                stack.pop()
    return dist2, nearest


def kernel_form(mask):
    """(dist2, nearest) int64 [H, W] as k_edt.hip computes them"""
    return column_pass(row_pass(np.asarray(mask, bool)))


def check(mask, dist2, nearest, want=None):
    """asserts the contract for one frame: dist2 is the definition at every pixel (want: brute(mask), computed here when None),
    nearest (None: not checked) an in-frame seed at exactly that squared distance, or INT32_MAX / -1 without a seed"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    dist2 = np.asarray(dist2).astype(np.int64)
    assert dist2.shape == (H, W)
    if want is None:
        want = brute(mask)
    assert np.array_equal(dist2, want), f"{int((dist2 != want).sum())} of {H * W} pixels differ from the definition"
    if nearest is None:
        return
    nearest = np.asarray(nearest).astype(np.int64)
    assert nearest.shape == (H, W)
    if not mask.any():
        assert np.all(nearest == -1) and np.all(dist2 == INT32_MAX)
        return
    assert nearest.min() >= 0 and nearest.max() < H * W
    ni, nj = np.divmod(nearest, W)
    assert np.all(mask[ni, nj]), "nearest names a pixel that is not a seed"
    pi, pj = np.mgrid[0:H, 0:W]
    assert np.array_equal((pi - ni) ** 2 + (pj - nj) ** 2, dist2), "nearest is not at the squared distance dist2"
    assert np.array_equal(nearest[mask], (pi * W + pj)[mask]), "a seed's nearest is not itself"


SIZES = [(1, 1), (1, 67), (67, 1), (45, 67), (5, 300), (300, 5), (128, 128)]
KINDS = ["empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "tie", "checkerboard", "random_0.5", "random_0.002",
         "disc_with_hole"]


def make_mask(kind, size, seed=0):
    H, W = size
    m = np.zeros((H, W), bool)
    i, j = np.mgrid[0:H, 0:W]
    if kind == "empty":
        pass
    elif kind == "full":
        m[:] = True
    elif kind.startswith("corner_"):
        m[0 if kind[7] == "t" else H - 1, 0 if kind[8] == "l" else W - 1] = True
    elif kind == "tie":
        # two seeds equidistant from a whole line of pixels: the middle column (or row) between them, and every pixel of it
        if W >= 3:
            m[H // 2, 0] = m[H // 2, 2 * ((W - 1) // 2)] = True
        elif H >= 3:
            m[0, W // 2] = m[2 * ((H - 1) // 2), W // 2] = True
        else:
            m[0, 0] = True
    elif kind == "checkerboard":
        m = (i + j) % 2 == 0
    elif kind.startswith("random_"):
        rng = np.random.default_rng([seed, H, W, int(float(kind[7:]) * 1000)])
        m = rng.random((H, W)) < float(kind[7:])
    elif kind == "disc_with_hole":
        r2 = (i - (H - 1) / 2.0) ** 2 + (j - (W - 1) / 2.0) ** 2
        R = min(H, W) / 2.0 * 0.8
        m = (r2 <= R * R) & (r2 > (0.4 * R) ** 2)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(m)


def masks():
    """{"kind@HxW": bool [H, W]}: every named mask at every size"""
    return {f"{k}@{s[0]}x{s[1]}": make_mask(k, s) for s in SIZES for k in KINDS}
