"""CPU: the marching-cubes table of bodyfit_volume_surface_* is the generator's (tools/gen_mc_table.py), has the properties that
include/bodyfit.h derives, and the numpy restatement of the definition (extract_ref.py), on the volumes of the GPU test, produces
closed oriented manifolds wherever no dead cell and no border of the volume touches the surface."""
import collections

import numpy as np
import pytest

import extract_ref as er

gen = er.gen


def test_the_committed_header_holds_the_generators_numbers():
    text = open(gen.HEADER).read()
    assert text == gen.header_text()
    n_tri, tri = gen.parse_header(text)
    want_n, want = gen.table()
    assert np.array_equal(n_tri, want_n) and np.array_equal(tri, want)


def test_edge_numbering():
    assert [gen.edge_corners(e) for e in range(12)] == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7),
                                                        (0, 4), (1, 5), (2, 6), (3, 7)]


def test_table_properties():
    rows = [gen.case_triangles(case) for case in range(256)]                    # (every case finds an apex, or this raises)
    counts = [len(r) for r in rows]
    assert max(counts) == 5 and sum(counts) == 820
    assert [collections.Counter(counts)[n] for n in range(6)] == [2, 16, 50, 80, 76, 32]
    assert rows[0] == [] and rows[255] == []
    assert rows[1] == [(0, 4, 8)] and rows[254] == [(0, 8, 4)]
    assert rows[0x69] == [(0, 4, 8), (1, 5, 11), (2, 7, 9), (3, 6, 10)]
    for case, tris in enumerate(rows):
        crossed = {e for e in range(12) if (case >> gen.edge_corners(e)[0] ^ case >> gen.edge_corners(e)[1]) & 1}
        assert {e for t in tris for e in t} == crossed                          # every crossed edge is used, and no other
        assert all(len(set(t)) == 3 for t in tris)
        # no triangle edge lies in a cube face unless it is one of that face's segments
        seg = {frozenset(s) for s in gen.segments(case)}
        for t in tris:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                assert not (gen.edge_faces(a) & gen.edge_faces(b)) or frozenset((a, b)) in seg, (case, t)


@pytest.mark.parametrize("dims", [(9, 8, 7), (13, 12, 11)], ids=lambda d: "x".join(map(str, d)))
def test_random_signs_inside_an_outside_layer_give_a_closed_oriented_manifold(dims):
    for seed in range(3):
        ref = er.extract(er.padded_random(dims, seed), er.ORIGIN, er.SPACING)
        unmatched, repeated = er.edge_census(ref.faces, ref.verts.shape[0])
        assert ref.faces.shape[0] > 100 and repeated == 0 and not unmatched.any()
        # closed and oriented with the normals towards the outside: the enclosed (signed) volume is positive
        assert er.signed_volume(ref.verts, ref.faces) > 0.0


def test_a_sphere_has_positive_signed_volume():
    n, radius = 21, 7.3
    k, j, i = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    vol = (np.sqrt((i - 10.2) ** 2 + (j - 9.9) ** 2 + (k - 10.1) ** 2) - radius).astype(np.float32)
    ref = er.extract(vol, (0.0, 0.0, 0.0), 1.0)
    unmatched, repeated = er.edge_census(ref.faces, ref.verts.shape[0])
    assert repeated == 0 and not unmatched.any()
    got, want = er.signed_volume(ref.verts, ref.faces), 4.0 / 3.0 * np.pi * radius ** 3
    print(f"sphere: signed volume {got:.2f} against {want:.2f}")
    assert 0.95 * want < got < want
    assert ref.verts.shape[0] - 3 * ref.faces.shape[0] // 2 + ref.faces.shape[0] == 2          # Euler: one sphere
    radial = np.linalg.norm(ref.verts.astype(np.float64) - np.array([10.2, 9.9, 10.1]), axis=1)
    assert float(np.abs(radial - radius).max()) < 0.1


@pytest.mark.parametrize("dims", er.DIMS, ids=lambda d: "x".join(map(str, d)))
def test_the_reference_on_the_gpu_tests_volumes(dims):
    for kind in er.KINDS:
        v = er.make_volume(kind, dims)
        ref = er.extract(v.vol, v.origin, v.spacing, v.iso, v.weight, v.min_weight)
        ok, n_open = er.open_edges_are_explained(ref, dims)
        assert ok, (kind, dims)
        if min(dims) < 2:
            assert ref.verts.shape[0] == 0 and ref.faces.shape[0] == 0
        elif kind in ("holes", "weights") and dims[0] >= 5:
            assert (~ref.live).any() and n_open > 0
        if kind == "sphere" and dims == (48, 48, 33):
            assert n_open == 0 and ref.faces.shape[0] > 1000                     # inside the volume: closed
        assert ref.faces.shape[0] == 0 or (ref.faces.min() == 0 and ref.faces.max() == ref.verts.shape[0] - 1)


def test_the_volumes_hit_all_256_cases():
    seen = set()
    for dims in er.DIMS:
        v = er.make_volume("normal", dims)
        ref = er.extract(v.vol, v.origin, v.spacing)
        seen |= set(np.unique(ref.case[ref.live]).tolist())
        if dims == (33, 17, 9):
            assert len(set(np.unique(ref.case).tolist())) == 256                 # this one alone holds them all
    assert len(seen) == 256
    # equality with iso and -0.0 are outside: the dyadic volume has both, and zero-area faces from them
    v = er.make_volume("dyadic", (33, 17, 9))
    assert (v.vol == 0).sum() > 100 and np.signbit(v.vol[v.vol == 0]).any()
    ref = er.extract(v.vol, v.origin, v.spacing)
    tri = ref.verts[ref.faces.astype(np.int64)].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).sum() > 10
