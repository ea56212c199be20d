"""CPU: the silhouette-edge antialiasing's reference (antialias_ref.py) against itself.  The f64 kernel form satisfies the contract
of include/bodyfit.h against the extended-precision definition on every scene; the analytic rows are the derivative of the blend
(central differences, bounded by the step's own second-order term and the evaluation's rounding); the transposed blend is the
adjoint; every scene's undecided share is within the cap."""
import os

import numpy as np
import pytest

import antialias_ref as aa
import depth_rows_ref as dr
import raster_ref as rr

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDECIDED_CAP = 0.01


@pytest.fixture(scope="module")
def scenes(synth):
    return aa.scenes(synth)


@pytest.fixture(scope="module")
def edges(scenes):
    return {name: aa.edges_of(sc) for name, sc in scenes.items()}


def test_header_states_the_constants_the_reference_uses():
    got = aa.header_constants(open(os.path.join(ROOT, "include", "bodyfit.h")).read())
    assert got == (aa.WALK, aa.K_C, aa.K_X, 46, aa.K_B, aa.K_R, 48)
    assert (2.0 ** -got[3], 2.0 ** -got[6]) == (aa.SIDE_TOL, aa.G_SHIFT) and aa.SIDE_TOL == rr.AREA_TOL


def test_adjacency_follows_the_lowest_id_rule():
    faces = np.array([[0, 1, 2], [2, 1, 3], [1, 0, 2], [4, 4, 5], [1, 2, 6]])
    adj = aa.adjacency(faces)
    assert adj[0].tolist() == [2, 1, 2]          # (0, 1): face 2; (1, 2): faces 1, 2, 4 -> 1; (2, 0): face 2
    assert adj[1].tolist() == [0, -1, -1]
    assert adj[2].tolist() == [0, 0, 0]
    assert adj[3].tolist() == [-1, -1, -1]       # a repeated id, and edges no other face holds
    assert adj[4].tolist() == [0, -1, -1]


@pytest.mark.parametrize("name", ["two_spheres", "two_spheres_culled", "soup_at_0.9m_67x45", "hand_shared_edge", "hand_shared_vertex",
                                  "hand_identical_faces", "hand_behind_z_near", "hand_zero_area", "hand_cull", "hand_no_cull",
                                  "hand_slanted"] + list(aa.EXACT))
def test_kernel_form_meets_the_contract_and_the_scene_is_decided(scenes, edges, name):
    """weights, blend (C = 1 and 3, forward and adjoint) and rows of the f64 kernel form against the extended reference at every pixel
    and pair; the undecided share of the reference alone is within the cap"""
    sc, E = scenes[name], edges[name]
    H, W = sc["size"]
    n_cand, n_blend, n_walked, n_und = E.census()
    assert E.undecided_share() <= UNDECIDED_CAP, (name, n_und, n_cand)
    worst_w = aa.check_weights(E, E.w_kernel)
    rng = np.random.default_rng(len(name))
    worst_b = 0.0
    for C in (1, 3):
        img = rng.uniform(-2.0, 3.0, size=(H, W, C)).astype(np.float32)
        for tr in (False, True):
            worst_b = max(worst_b, aa.check_blend(E.w_kernel, img, aa.blend_kernel_form(E.w_kernel, img, tr), tr))
    img, up = (rng.uniform(-2.0, 3.0, size=(H, W, 3)).astype(np.float32) for _ in range(2))
    codes = np.concatenate([aa.pair_codes(E.w_kernel), np.int32([0, 2 * H * W - 1, 2 * H * W + 6, -3])])   # and pairs that do not blend
    rows = aa.rows_kernel_form(E, codes, img, up)
    worst_r, ref = aa.check_rows(E, codes, img, up, *rows)
    # ... and the rows' exact sum against the exact vertex gradient, within the rows' bounds
    V = len(sc["verts"])
    G, B = aa.vertex_gradient(sc["faces"], V, ref)
    got, _ = dr.vjp_exact(sc["faces"], V, rows[0], rows[1], rows[2], rows[3])
    assert np.all(np.abs(got - G) <= B + 1e-300), float((np.abs(got - G) / (B + 1e-300)).max())
    print(f"{name}: {n_cand} candidate pairs, {n_blend} blended, {n_walked} walked more than one face, {n_und} undecided; smallest "
          f"margin {E.min_margin:.3g}, {E.n_exact_ties} exact ties; worst weight {worst_w:.3f}, blend {worst_b:.3f}, row coef "
          f"{worst_r[0]:.3f}, row dir {worst_r[1]:.3f} of their bounds")
    assert n_blend > 0
    if name in aa.EXACT:
        assert n_und == 0
        assert np.array_equal(E.w_kernel, E.w_ref.astype(np.float64).astype(np.float32)), "an exact scene: the weights to the bit"
        assert all(h["face"] == E.hits64[k]["face"] and h["edge"] == E.hits64[k]["edge"] for k, h in E.hits.items())


def test_hand_scenes_hit_their_tie_rules(edges):
    w = {name: edges[name].w_kernel for name in aa.EXACT}
    assert np.all(w["aa_centre"][3:10, 3, 0] == 0.5)                     # d = 0: the near pixel (q) receives 1/2
    assert np.all(w["aa_half"][3:10, 4, 0] == 0.0)                       # d = 1/2: alpha = 0
    assert np.all(w["aa_one"][3:9, 4, 0] == -0.5)                        # d = 1: the other pixel (p) receives 1/2
    E = edges["aa_vertex_on_scanline"]
    assert E.w_kernel[6, 4, 0] == -0.25 and E.hits[(6, 4, 0)]["steps"] == 2 and E.hits[(6, 4, 0)]["s"] == 0
    E = edges["aa_flat_quad"]
    inner = [(k, h) for k, h in E.hits.items() if 3 <= k[0] <= 8 and 3 <= k[1] <= 8]
    assert not inner and E.census()[1] > 0                                # nothing blends across the diagonal, the rim does
    E = edges["aa_strip"]
    assert all(E.hits[(i, 4, 0)]["steps"] == 3 and E.w_kernel[i, 4, 0] == -0.25 for i in range(3, 10))
    E = edges["aa_twins"]
    assert E.census()[1] > 0 and all(h["face"] == 0 for h in E.hits.values())
    E = edges["aa_equal_depth"]
    assert all(E.hits[(i, 6, 0)]["near_q"] == 0 and E.w_kernel[i, 6, 0] == -0.25 for i in range(3, 11))
    E = edges["aa_open_triangle"]
    assert all(E.adj[h["face"], h["edge"]] == -1 for h in E.hits.values())


def test_two_spheres_census_is_the_one_the_definition_was_designed_on(edges):
    E = edges["two_spheres"]
    assert E.census() == (2270, 358, 177, 0)
    assert E.min_margin > 1e-9


def test_adjoint_identity(edges):
    rng = np.random.default_rng(5)
    for name in ("two_spheres", "aa_strip", "soup_at_0.9m_67x45"):
        E = edges[name]
        H, W = E.size
        x = rng.standard_normal((H, W, 3)).astype(np.float32)
        y = rng.standard_normal((H, W, 3)).astype(np.float32)
        bx, Tx = aa.blend_exact(E.w_kernel, x)
        bty, Ty = aa.blend_exact(E.w_kernel, y, transpose=True)
        lhs, rhs = (bx * y.astype(LD)).sum(), (x.astype(LD) * bty).sum()
        scale = (Tx * np.abs(y)).sum() + (np.abs(x) * Ty).sum()
        assert abs(lhs - rhs) <= 2.0 ** -55 * scale, (name, float(abs(lhs - rhs) / scale))


def test_rows_are_the_derivative_of_the_blend():
    """f64 on two_spheres: L(verts) = sum up . blend(img, w(verts)) over the pairs whose smallest decision margin exceeds what the
    step can move; its central differences at h and 2 h against the analytic rows.  The bound is Richardson's estimate of the
    step's second-order term, |CD(2h) - CD(h)|, plus what the f64 evaluation's own error can add to a difference quotient: the
    contract bounds the unrounded f64 weight of a decided pair by 2 tau_x, so two evaluations 2 h apart by sum 2 tau_x |up . diff| / h."""
    verts, faces, intr, size = rr.two_spheres()
    sc = dict(verts=verts, faces=faces, intr=intr, size=size, z_near=0.1, cull=False, edit=None)
    face, depth = aa.images_of(sc)
    E = aa.edges_of(sc)
    H, W = size
    rng = np.random.default_rng(11)
    img = rng.uniform(-2.0, 3.0, size=(H, W, 3)).astype(np.float32)
    up = rng.standard_normal((H, W, 3)).astype(np.float32)
    h = 1e-7
    px_per_m = max(intr[0], intr[1]) / float(verts[:, 2].min())
    # the pairs whose every decision clears 100 steps' worth of pixels (the margins of sides and areas are in pixel^2: more)
    keys = []
    for key in E.hits:
        dec = []
        aa.pair_eval(E.pld, E.adj, face, depth, key[0], key[1], key[2], dec)
        if min(float(m) for m, _, _ in dec) > 100 * 2 * h * px_per_m:
            keys.append(key)
    assert len(keys) > 300
    codes = np.array(sorted(2 * (i * W + j) + a for i, j, a in keys), np.int32)
    ref = aa.exact_rows(E, codes, img, up)
    G, _ = aa.vertex_gradient(faces, len(verts), ref)
    touched = np.nonzero(np.abs(G).sum(axis=1) > 0)[0]
    x64, u64 = img.astype(np.float64), up.astype(np.float64)

    fa = np.asarray(faces, np.int64)

    def loss(v64, some):
        """(the loss over the pairs `some`, sum 2 tau_x |up . diff| over them)"""
        pr = aa.Projection(v64, faces, intr, size, 0.1, False, np.float64)
        total, slack = 0.0, 0.0
        for (i, j, a) in some:
            w, hit, _ = aa.pair_eval(pr, E.adj, face, depth, i, j, a, [])
            p, q = (i, j), ((i + 1, j) if a else (i, j + 1))
            r, s = (q, p) if w > 0 else (p, q)
            total += abs(w) * (u64[r] * (x64[s] - x64[r])).sum()
            slack += 2 * hit["tau_x"] * abs((u64[r] * (x64[s] - x64[r])).sum())
        return total, slack

    v0 = verts.astype(np.float64)
    comps = [(int(v), c) for v in touched[:: max(1, len(touched) // 11)] for c in range(3)][:33]
    worst, scale = 0.0, float(np.abs(G).max())
    for v, c in comps:
        some = [k for k in keys if v in fa[E.hits[k]["visited"]]]          # the only pairs whose weight can depend on vertex v
        cd = []
        for step in (h, 2 * h):
            vp, vm = v0.copy(), v0.copy()
            vp[v, c] += step
            vm[v, c] -= step
            (lp, slack), (lm, _) = loss(vp, some), loss(vm, some)
            cd.append((lp - lm) / (2 * step))
        bound = abs(cd[1] - cd[0]) + slack / h
        err = abs(cd[0] - float(G[v, c]))
        assert err <= bound, (v, c, err, bound)
        worst = max(worst, err / scale)
    print(f"rows against central differences (h = {h:g} m, f64): {len(comps)} components of {len(touched)} vertices with a gradient, "
          f"{len(keys)} of {len(E.hits)} pairs; worst disagreement {worst:.2e} of the largest component")
