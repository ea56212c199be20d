"""CPU: the closest-point primitive's declarations, exports, Python surface and argument checks (no device is touched), and the
numpy reference of tests/closest_ref.py on a hand-made case.  The search and its gradient themselves:
tests/test_gpu_closest_points.py."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

import closest_ref as cr

SYMBOLS = ["bodyfit_closest_create", "bodyfit_closest_destroy", "bodyfit_closest_points_device",
           "bodyfit_closest_points_vjp_device"]


def test_header_declares_and_library_exports(api):
    hdr = open(api.HEADER_PATH).read()
    assert re.search(r"typedef struct bodyfit_pointset\s*\{", hdr) and "typedef struct bodyfit_closest bodyfit_closest;" in hdr
    declared = api.declared_symbols()
    lib = api.load_library()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s


def test_python_surface(api):
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    assert callable(tl.closest_points) and issubclass(tl.PointCloudTerm, tl.torch.nn.Module)
    assert hasattr(api.ClosestPoints, "points_device") and hasattr(api.ClosestPoints, "points_vjp_device")
    u = api.PointSet.uniform(0x1000, 6890, 20672)
    assert (u.n_per_frame, u.frame_stride, u.d_offset) == (6890, 20672, None)
    assert api.PointSet.uniform(0x1000, 5).frame_stride == 15
    r = api.PointSet.ragged(0x1000, 0x2000)
    assert r.d_offset == 0x2000
    # bodyfit_pointset's layout: pointer, pointer, int, long long
    assert C.sizeof(api.PointSet) == 32 and api.PointSet.frame_stride.offset == 24


def test_argument_errors_before_any_device(api):
    """Every argument check comes before the handle is looked at, so it is observable without a GPU (with a NULL handle): the
    status is BODYFIT_ERR_INVALID and the message names the argument."""
    lib = api.load_library()
    INVALID = 1
    ok = api.PointSet.uniform(0x1000, 10, 30)
    rag = api.PointSet.ragged(0x1000, 0x2000)

    def fwd(q, r, F=2, nq=0, nr=0, d=0x3000, i=0x4000):
        return lib.bodyfit_closest_points_device(None, C.byref(q) if q else None, C.byref(r) if r else None, F, nq, nr, d, i, 0, None)

    def bwd(q, r, F=2, nq=0, nr=0, idx=0x3000, g=0x4000, gq=0x5000, gr=0x6000):
        return lib.bodyfit_closest_points_vjp_device(None, C.byref(q) if q else None, C.byref(r) if r else None, F, nq, nr, idx, g,
                                                     gq, gr, None)

    def msg():
        return lib.bodyfit_last_error().decode()

    short = api.PointSet.uniform(0x1000, 10, 29)
    for call in (fwd, bwd):
        assert call(short, ok) == INVALID and "query: frame_stride < 3 n_per_frame" in msg()
        assert call(ok, short) == INVALID and "ref: frame_stride < 3 n_per_frame" in msg()
        assert call(None, ok) == INVALID and "query is NULL" in msg()
        assert call(ok, None) == INVALID and "ref is NULL" in msg()
        assert call(ok, ok, F=-1) == INVALID and "negative n_frames" in msg()
        assert call(rag, ok, nq=-5) == INVALID and "negative row count" in msg()
        assert call(api.PointSet.uniform(0x1000, -1, 30), ok) == INVALID and "negative n_per_frame" in msg()
        assert call(api.PointSet.uniform(None, 10, 30), ok) == INVALID and "d_xyz is NULL" in msg()
        assert call(ok, ok) == INVALID and "null handle" in msg()          # everything else in order: only the handle is missing
    assert fwd(ok, ok, d=None) == INVALID and "d_dist2 / d_index is NULL" in msg()
    assert fwd(ok, ok, i=None) == INVALID and "d_dist2 / d_index is NULL" in msg()
    assert bwd(ok, ok, idx=None) == INVALID and "d_index / d_grad_dist2 is NULL" in msg()
    assert bwd(ok, ok, g=None) == INVALID and "d_index / d_grad_dist2 is NULL" in msg()
    assert lib.bodyfit_closest_create(0, None) == INVALID
    lib.bodyfit_closest_destroy(None)                                     # a no-op


def test_create_needs_a_device(api):
    if api.device_count() > 0:
        pytest.skip("GPU present: covered by the -m gpu tests")
    with pytest.raises(api.BodyfitError):
        api.ClosestPoints(0)                                              # BODYFIT_ERR_HIP, never a CPU path


def test_layer_checks_inputs_without_a_device():
    torch = importlib.import_module("torch")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    p = torch.zeros((2, 5, 3), dtype=torch.float32)
    with pytest.raises(ValueError):
        tl.closest_points(p, p)                                           # not on the GPU
    with pytest.raises(TypeError):
        tl.closest_points(p.double(), p)
    with pytest.raises(TypeError):
        tl.closest_points(np.zeros((2, 5, 3), np.float32), p)
    with pytest.raises(ValueError):
        tl.PointCloudTerm(torch.zeros((4, 3)), torch.zeros(3, dtype=torch.int32), trunc=-1.0)


def test_reference_on_a_hand_made_case():
    """Three reference points, one of them a duplicate of another; known answers.  (A test of the test infrastructure,
    tests/closest_ref.py, which the GPU tests rely on: it says nothing about the library.)"""
    r = np.array([[0, 0, 3], [1, 0, 3], [1, 0, 3]], np.float32)
    q = np.array([[0.9, 0, 3], [0.25, 0, 3], [0, 0, 3], [0.5, 0, 3]], np.float32)
    dmin, amin = cr.brute_force(q, r)
    assert list(amin) == [1, 0, 0, 0]                                     # the duplicate: lowest index; the exact tie at 0.5 too
    np.testing.assert_allclose(dmin, [(np.float64(np.float32(0.9)) - 1.0) ** 2, 0.0625, 0.0, 0.25], rtol=0, atol=0)
    d2, idx = cr.diff_form_f32(q, r)
    assert list(idx) == [1, 0, 0, 0] and d2.dtype == np.float32
    assert max(cr.check_bounds(q, r, d2, idx)) < 2.0 ** -22
    # a wrong answer is caught: index 2 -> 0 for query 0 is 81 times farther
    with pytest.raises(AssertionError):
        cr.check_bounds(q, r, d2, np.array([0, 0, 0, 0]))
    with pytest.raises(AssertionError):
        cr.check_bounds(q, r, d2 * np.float32(1.00001), idx)
    # no reference points
    d2e, idxe = cr.diff_form_f32(q, r[:0])
    assert np.all(idxe == -1) and np.all(np.isposinf(d2e))
    cr.check_bounds(q, r[:0], d2e, idxe)
    # gradient: sum_i g_i dist2_i
    g = np.array([1.0, 2.0, -1.0, 0.5], np.float32)
    gq, gr, ar, n_r = cr.vjp(q, r, idx, g)
    assert list(n_r) == [3, 1, 0]
    np.testing.assert_allclose(gq[1], [-2 * 2.0 * (0 - 0.25), 0, 0])
    np.testing.assert_allclose(gr[0], [2 * 2.0 * (0 - 0.25) + 2 * 0.5 * (0 - 0.5), 0, 0])
    np.testing.assert_allclose(gr.sum(0), -gq.sum(0), atol=1e-15)        # a translation of both sets changes nothing
    assert np.all(gr[2] == 0)
    eps = 1e-6                                                            # against central differences of the frozen-index cost
    cost = lambda qq, rr: float((g * ((qq - rr[idx]) ** 2).sum(1)).sum())
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    for (arr, grad) in ((q64, gq), (r64, gr)):
        for i in range(arr.shape[0]):
            for c in range(3):
                a = arr.copy(); b = arr.copy(); a[i, c] += eps; b[i, c] -= eps
                fd = (cost(a, r64) - cost(b, r64)) / (2 * eps) if arr is q64 else (cost(q64, a) - cost(q64, b)) / (2 * eps)
                assert abs(fd - grad[i, c]) < 1e-8
    # -1 rows contribute nothing
    gq2, gr2, _, n2 = cr.vjp(q, r, np.array([1, -1, 0, -1]), g)
    assert np.all(gq2[[1, 3]] == 0) and list(n2) == [1, 1, 0]
