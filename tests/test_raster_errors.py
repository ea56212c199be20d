"""CPU: what the raster entries reject before they need a device: the NULL-handle rows of tests/raster_errors_table.py (the whole
table runs in tests/test_gpu_raster_errors.py) and bodyfit_raster_create's argument checks, on the loaded library with or
without a GPU."""
import ctypes as C

import numpy as np

import raster_errors_table as ret


def test_null_handle_rows(api):
    lib = api.load_library()
    rows = [row for row in ret.TABLE if "r" in row[1] and row[1]["r"] is None]
    assert {row[0] for row in rows} == set(ret.ARGS) and all(row[2] == ret.INVALID for row in rows)
    n_entries, longest = C.c_longlong(), C.c_int()
    tokens = {ret.LL: C.byref(n_entries), ret.INT: C.byref(longest)}      # every other pointer: NULL, never looked at
    bad = ret.mismatches(lib, rows, lambda token: tokens.get(token))
    assert not bad, "\n".join(bad)


def test_create_rejects_its_arguments_before_it_looks_for_a_device(api):
    lib = api.load_library()
    faces = np.asarray(ret.FACES, np.int32)
    fp = faces.ctypes.data_as(C.POINTER(C.c_int32))
    out = C.c_void_p()
    cases = [
        ((0, 4, 2, fp, 8, 8, None), "out is NULL"),
        ((0, -1, 2, fp, 8, 8, C.byref(out)), "negative count or NULL faces"),
        ((0, 4, -1, fp, 8, 8, C.byref(out)), "negative count or NULL faces"),
        ((0, 4, 2, None, 8, 8, C.byref(out)), "negative count or NULL faces"),
        ((0, 4, 2, None, 0, 8, C.byref(out)), "negative count or NULL faces"),
        ((0, 4, 2, fp, 0, 8, C.byref(out)), "image size outside 1 .. 16384"),
        ((0, 4, 2, fp, 8, 16385, C.byref(out)), "image size outside 1 .. 16384"),
        ((0, 3, 2, fp, 0, 8, C.byref(out)), "image size outside 1 .. 16384"),
        ((0, 3, 2, fp, 8, 8, C.byref(out)), "face refers to a vertex out of range"),
    ]
    for args, what in cases:
        assert lib.bodyfit_raster_create(*args) == ret.INVALID, args
        assert lib.bodyfit_last_error().decode() == "bodyfit_raster_create: " + what, args
        assert out.value is None
    lib.bodyfit_raster_destroy(None)      # (a NULL handle is nothing to destroy)
