"""GPU: the statuses and messages of every entry that takes a bodyfit_raster (k_raster.hip, k_raster_rows.hip, k_raster_shade.hip,
k_raster_edges.hip, k_texture.hip, k_light.hip, k_edt.hip) against tests/raster_errors_table.py: every rejection, the order of the
checks where a call breaks two rules, and the early BODYFIT_OK returns.  No row of the table reaches a HIP call; the one launch of
this file is the valid render at its end, which shows the handle of the table to be a working one."""
import ctypes as C
import importlib

import numpy as np
import pytest

import raster_errors_table as ret

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def handle(api):
    return api.Raster(0, ret.N_VERTS, np.asarray(ret.FACES, np.int32), ret.WIDTH, ret.HEIGHT)


def test_table_covers_every_entry_on_the_handle(api):
    declared = {s for s in api.declared_symbols() if s.startswith("bodyfit_raster_")}
    assert declared - {"bodyfit_raster_create", "bodyfit_raster_destroy"} == set(ret.ARGS) == {row[0] for row in ret.TABLE}
    for entry in ret.ARGS:
        rows = [row for row in ret.TABLE if row[0] == entry]
        assert any(row[2] == ret.INVALID and len(row[1]) >= 2 for row in rows), f"{entry}: no call that breaks two rules"
        assert entry == "bodyfit_raster_last_bins" or any(row[2] == ret.OK for row in rows), f"{entry}: no early BODYFIT_OK"


def test_statuses_and_messages(api, torch, handle):
    lib = api.load_library()
    # 1 MiB each, zeroed: far more than a valid call on 2 frames of 8 x 8 pixels reads or writes
    bufs = {name: torch.zeros(1 << 18, dtype=torch.int32, device="cuda") for name in (ret.IN, ret.OUT, ret.OUT2)}
    n_entries, longest = C.c_longlong(), C.c_int()
    tokens = {ret.HANDLE: handle.h, ret.LL: C.byref(n_entries), ret.INT: C.byref(longest),
              **{name: b.data_ptr() for name, b in bufs.items()}}
    bad = ret.mismatches(lib, ret.TABLE, tokens.__getitem__)
    print(f"raster entries: {len(ret.TABLE)} calls on {len(ret.ARGS)} entries, {len(bad)} not as the table states")
    assert not bad, "\n".join(bad)
    torch.cuda.synchronize()
    assert all(int(b.abs().max()) == 0 for b in bufs.values())      # nothing was written


def test_the_tables_handle_renders(api, torch, handle):
    verts = torch.tensor([[[-1.0, -1.0, 4.0], [1.0, -1.0, 4.0], [1.0, 1.0, 4.0], [-1.0, 1.0, 4.0]]] * 2, dtype=torch.float32,
                         device="cuda")
    depth = torch.full((2, ret.HEIGHT, ret.WIDTH), -5.0, dtype=torch.float32, device="cuda")
    face = torch.full((2, ret.HEIGHT, ret.WIDTH), -9, dtype=torch.int32, device="cuda")
    handle.render_device(verts.data_ptr(), 12, 2, (10.0, 10.0, 4.0, 4.0), depth.data_ptr(), face.data_ptr(), None,
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f = face.cpu().numpy()
    # the square spans u, v in [1.5, 6.5]: pixels 2 .. 6 of both axes, split along its diagonal between the two faces
    inside = np.zeros((ret.HEIGHT, ret.WIDTH), bool)
    inside[2:7, 2:7] = True
    for k in range(2):
        assert ((f[k] >= 0) == inside).all() and set(np.unique(f[k][inside])) == {0, 1}
        d = depth[k].cpu().numpy()
        assert np.allclose(d[inside], 4.0, rtol=1e-6) and np.isinf(d[~inside]).all()
