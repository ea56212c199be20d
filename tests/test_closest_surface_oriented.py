"""CPU: the references of the oriented closest-surface search (tests/oriented_ref.py) checked on their own, before any GPU test
relies on them: the f64 normals against the plain cross product and the orientation of `faces`; the f32 restatement of the
kernel's gate inside the sandwich contract of include/bodyfit.h on every scene the GPU tests use; the conditions on those
scenes that make the GPU tests mean something (the gate changes many answers, leaves some queries without a face, and the
sandwich is tight), asserted from the f64 reference alone; and the constructed threshold case."""
import numpy as np
import pytest

import oriented_ref as orf
import surface_ref as sr

SCENES = [orf.MAIN] + [orf.OFF_TILE[k] for k in sorted(orf.OFF_TILE)]


@pytest.fixture(scope="module")
def scenes(synth):
    """every scene once, with its pair distances: {(seed, V, nf, nq): (q, m, verts, faces, D)}"""
    out = {}
    for key in SCENES:
        q, m, verts, faces = orf.oriented_scene(synth, key[0], V=key[1], n_faces=key[2], n_query=key[3])
        out[key] = (q, m, verts, faces, orf.pair_distances64(q, verts, faces))
    return out


def test_normals_are_the_oriented_unit_cross_product_and_follow_the_area_rule(scenes):
    q, m, verts, faces, _ = scenes[orf.MAIN]
    n, area = orf.face_normals64(verts, faces)
    V = verts.astype(np.float64)
    raw = np.cross(V[faces[:, 1]] - V[faces[:, 0]], V[faces[:, 2]] - V[faces[:, 0]])
    ln = np.linalg.norm(raw, axis=1)
    assert area.sum() > 0.9 * len(faces)
    np.testing.assert_allclose(n[area], raw[area] / ln[area, None], atol=1e-9)       # the orientation of `faces`, unit length
    assert np.all(n[~area] == 0)
    # reversing a face reverses its normal; a cyclic shift does not
    n_rev, _ = orf.face_normals64(verts, faces[:, ::-1])
    n_cyc, _ = orf.face_normals64(verts, np.roll(faces, 1, axis=1))
    np.testing.assert_allclose(n_rev, -n, atol=1e-12)
    np.testing.assert_allclose(n_cyc, n, atol=1e-12)
    # the degenerate faces of surface_ref.degenerate_scene: points, segments and collinear corners have no area, the sliver has
    _, dv, df = sr.degenerate_scene()
    _, darea = orf.face_normals64(dv, df)
    assert darea.tolist() == [False, False, False, False, False, True, True, True, True, False]
    # and the mask is the record's t > 0
    assert np.array_equal(sr.prepare_records(dv, df)["t"] > 0, darea)
    assert np.array_equal(sr.prepare_records(verts, faces)["t"] > 0, area)


def test_directions_of_the_scenes(scenes):
    q, m, verts, faces, _ = scenes[orf.MAIN]
    assert m.dtype == np.float32 and np.allclose(np.linalg.norm(m.astype(np.float64), axis=1), 1.0, atol=1e-6)
    n, area = orf.face_normals64(verts, faces)
    src = np.random.default_rng(orf.MAIN[0]).integers(0, len(faces), len(q))[:len(q) // 2]
    cos = (n[src] * m[:len(q) // 2]).sum(axis=1)
    assert np.all(cos[area[src]] >= np.cos(np.deg2rad(30.0)) - 1e-6), "the first half: within 30 degrees of the source face's normal"
    rest = (m[len(q) // 2:].astype(np.float64)).mean(axis=0)
    assert np.linalg.norm(rest) < 0.2, "the second half: no preferred direction"


@pytest.mark.parametrize("key", SCENES, ids=lambda k: f"nf{k[2]}")
@pytest.mark.parametrize("min_cos", orf.MIN_COS)
def test_f32_form_meets_the_sandwich_contract_on_the_gpu_tests_inputs(scenes, key, min_cos):
    q, m, verts, faces, D = scenes[key]
    got = orf.kernel_form_oriented_f32(q, m, verts, faces, min_cos)
    opt, con, hits = orf.check_oriented(q, m, verts, faces, min_cos, *got, D=D)
    print(f"oriented f32 form nf={key[2]} min_cos={min_cos}: {hits} of {len(q)} hit, optimality excess {opt:.1f}, "
          f"consistency {con:.1f} (units of u (d + h); bound {orf.K}; k_n = {orf.K_N})")
    assert orf.K_N <= 32
    if min_cos == 2.0:
        assert hits == 0
    if min_cos == -2.0:
        # every face with an area is a candidate: the unoriented f32 form over those faces, bit for bit
        _, area = orf.face_normals64(verts, faces)
        keep = np.flatnonzero(area)
        d2, ix, b = sr.kernel_form_f32(q, verts, faces[keep])
        assert np.array_equal(got[0], d2) and np.array_equal(got[1], keep[ix]) and np.array_equal(got[2], b)


def test_some_queries_have_no_compatible_face(scenes):
    """at min_cos = 0.5, from the f64 reference: the one-face scene leaves many queries without a face"""
    q, m, verts, faces, D = scenes[orf.OFF_TILE[1]]
    none = orf.brute_force_oriented(q, m, verts, faces, 0.5, 0.0, D=D)[1] < 0
    assert 1 <= none.sum() < len(q)


@pytest.mark.parametrize("key", [k for k in SCENES if k[2] > 1], ids=lambda k: f"nf{k[2]}")
def test_the_scenes_exercise_the_gate_and_the_sandwich_is_tight(scenes, key):
    """Conditions on the INPUTS at min_cos = 0.5, from the f64 reference alone: in every multi-face scene the oriented answer
    differs from the unoriented one for at least a fifth of the queries (another face, or none), and the strict and the loose
    reference disagree for at most 1 % of the queries.  (Queries without any compatible face are the one-face scene's, asserted
    above: a soup of tens of randomly oriented faces already offers a compatible face to every direction, so in these scenes the
    no-candidate path is reached by min_cos = 2 and by NaN directions.)"""
    q, m, verts, faces, D = scenes[key]
    tau = orf.tau_of(m)
    d_un, i_un, _ = sr.brute_force(q, verts, faces)
    d_or, i_or, _ = orf.brute_force_oriented(q, m, verts, faces, 0.5, 0.0, D=D)
    differs = (i_or < 0) | (d_or > d_un * (1 + 1e-9) + 1e-30)            # (by distance: equal distances on shared edges are no change)
    d_st, i_st, _ = orf.brute_force_oriented(q, m, verts, faces, 0.5, tau, D=D)
    d_lo, i_lo, _ = orf.brute_force_oriented(q, m, verts, faces, 0.5, -tau, D=D)
    disagree = (d_st != d_lo)
    print(f"nf={key[2]}: gate changes {differs.mean():.1%} of the answers, {int((i_or < 0).sum())} queries without a compatible "
          f"face, strict and loose disagree for {disagree.mean():.2%}")
    assert differs.mean() >= 0.2
    assert disagree.mean() <= 0.01


def test_reference_on_two_sheets_and_without_faces():
    q, m, verts, faces = orf.two_sheets()
    d_un, i_un, _ = sr.brute_force(q, verts, faces)
    d_or, i_or, b_or = orf.brute_force_oriented(q, m, verts, faces, 0.5)
    z = verts.astype(np.float64)[:, 2]
    pz = q.astype(np.float64)[:, 2]
    assert np.all(i_un < 2) and np.allclose(d_un, (pz - z[0]) ** 2, rtol=1e-12)
    assert np.all(i_or >= 2) and np.allclose(d_or, (z[4] - pz) ** 2, rtol=1e-12)
    assert np.all(orf.brute_force_oriented(q, -m, verts, faces, 0.5)[1] < 2)
    d, i, b = orf.brute_force_oriented(q, m, verts, faces[:0], 0.5)
    assert np.all(i == -1) and np.all(np.isposinf(d)) and np.all(b == 0)
    got = orf.kernel_form_oriented_f32(q, m, verts, faces[:0], 0.5)
    orf.check_oriented(q, m, verts, faces[:0], 0.5, *got)
    # a NaN direction: nothing qualifies, in the reference and in the f32 form
    mn = m.copy(); mn[3, 1] = np.nan
    assert orf.brute_force_oriented(q, mn, verts, faces, 0.5)[1][3] == -1
    got = orf.kernel_form_oriented_f32(q, mn, verts, faces, 0.5)
    assert got[1][3] == -1 and np.all(np.delete(got[1], 3) >= 2)
    orf.check_oriented(q, mn, verts, faces, 0.5, *got)
    got = orf.kernel_form_oriented_f32(q, m, verts, faces, np.nan)
    assert np.all(got[1] == -1)


def test_check_oriented_rejects_what_the_contract_forbids():
    """the checker itself: an incompatible face, a miss beside a compatible face, and a far face are each refused"""
    q, m, verts, faces = orf.two_sheets(n=8)
    good = orf.kernel_form_oriented_f32(q, m, verts, faces, 0.5)
    orf.check_oriented(q, m, verts, faces, 0.5, *good)
    front = sr.kernel_form_f32(q, verts, faces)                          # the unoriented answer: the front sheet, normal -z
    with pytest.raises(AssertionError, match="loose"):
        orf.check_oriented(q, m, verts, faces, 0.5, *front)
    miss = (np.full(8, np.inf, np.float32), np.full(8, -1), np.zeros((8, 3), np.float32))
    with pytest.raises(AssertionError, match="strict"):
        orf.check_oriented(q, m, verts, faces, 0.5, *miss)
    # a compatible face, but not the closest: a third sheet 5 cm behind the back one
    far = np.concatenate([verts, verts[4:] + np.float32([0, 0, 0.05])]).astype(np.float32)
    faces3 = np.concatenate([faces, faces[2:] + 4]).astype(np.int32)
    wrong = orf.kernel_form_oriented_f32(q, m, far, faces3[4:], 0.5)
    with pytest.raises(AssertionError, match="optimality"):
        orf.check_oriented(q, m, far, faces3, 0.5, wrong[0], wrong[1] + 4, wrong[2])


def test_constructed_threshold_case():
    q, m, verts, faces, (below, on, above) = orf.threshold_case()
    R = sr.prepare_records(verts, faces)
    assert R["u"].tolist() == [[1.0, 0.0, 0.0]] and R["w"].tolist() == [[0.0, 1.0, 0.0]], "the record is exact"
    assert below < on < above and np.float32(m[0, 2]) == on
    n, area = orf.face_normals64(verts, faces)
    assert area.all() and n.tolist() == [[0.0, 0.0, 1.0]]
    for mc, want in ((below, 0), (on, None), (above, -1)):
        got = orf.kernel_form_oriented_f32(q, m, verts, faces, mc)
        orf.check_oriented(q, m, verts, faces, mc, *got)
        assert want is None or got[1][0] == want, (float(mc), got[1])
        assert got[1][0] in (0, -1)
