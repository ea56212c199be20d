"""Times of the volume distance transform (bodyfit_volume_distance_device: k_edt_rows + k_edt_cols of k_edt.hip over the slices, then
k_edt_depth of k_edt3.hip) on one 128^3 volume, one 256^3 volume and 64 volumes of 128^3, with two seed contents each: a sphere's
surface one voxel thick (what esdf transforms) and random 0.5 (deep stacks).
Timed with the protocol of tools/tsdf_bench.py (a warm-up, then --brackets brackets of back-to-back calls, host clock around work
that ends in a device synchronise; median [min .. max]; the alternatives ALTERNATE bracket by bracket):
  full       the entry: both stages, with the nearest seed,
  xy         the stage xy alone: the SAME two kernels on the same slices through bodyfit_raster_distance_device (a slice is a frame),
  z          full - xy, by subtraction: the launches follow one another on one stream,
  copy       a plain copy of the seed volume into the two int32 outputs by torch: the floor,
  2-D        the 2-D transform of the same pixel count in square frames.
Then, at each size, esdf and occupancy_sdf end to end on a sphere's TSDF, and at 128^3 volume.voxelize_sdf of an SMPL-sized mesh, the
path they replace for a scene that is a mesh.  With --parent-lib the 2-D transform of tools/silhouette_bench.py's 1920 x 1080 frames
from this build and from a library built from the parent commit, alternated: the same bits and the same time are what is to be seen.
Nothing is asserted; every comparison is printed whichever way it falls.
Usage: python3 tools/edt3_bench.py [--brackets 5] [--parent-lib PATH] [--quick] [--out profiles/edt3_bench.txt]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tsdf_bench import STREAM_TBPS, alternate  # noqa: E402


def sphere(torch, n, F):
    """the distance to a sphere's surface at the voxel centres of F volumes n^3, in voxels: [F, n, n, n] f32 (the radius varies)"""
    ax = torch.arange(n, dtype=torch.float32, device="cuda") - 0.5 * (n - 1)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    radii = torch.linspace(0.30, 0.42, F, device="cuda") * n
    return r[None] - radii[:, None, None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt3_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    volume = importlib.import_module("3dbodyanimation_amd.torch_layer.volume")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    if api.device_count() < 1:
        raise SystemExit("edt3_bench needs a GPU: nothing here can be timed on the CPU")
    stream = torch.cuda.current_stream().cuda_stream
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# edt3_bench: brackets={args.brackets}; times in ms per call: median [min .. max] x calls per bracket; alternatives "
             f"alternate bracket by bracket" + ("; QUICK sizes: a rehearsal, not a measurement" if args.quick else "")]
    rows = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    no_faces = np.zeros((0, 3), np.int32)
    sizes = [(32, 1, 64), (64, 1, 128), (32, 4, 64)] if args.quick else [(128, 1, 1024), (256, 1, 4096), (128, 64, 2048)]
    for n, F, side in sizes:
        voxels = F * n ** 3
        frames2d = voxels // (side * side)                                   # square frames of the same pixel count
        assert frames2d * side * side == voxels
        dist = sphere(torch, n, F)
        handle = api.Volume(0, (n, n, n), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        slices = api.Raster(0, 0, no_faces, n, n)
        flat = api.Raster(0, 0, no_faces, side, side)
        work = torch.empty(handle.distance_layout(F), dtype=torch.uint8, device="cuda")
        dist2 = torch.empty((F, n, n, n), dtype=torch.int32, device="cuda")
        nearest = torch.empty_like(dist2)
        gen = torch.Generator(device="cuda").manual_seed(3)
        seeds = {"surface": (dist.abs() <= 0.5).to(torch.uint8),
                 "random 0.5": (torch.rand(dist.shape, device="cuda", generator=gen) < 0.5).to(torch.uint8)}
        for content, seed in seeds.items():
            full = lambda: handle.distance_device(seed.data_ptr(), 0, n ** 3, F, False, work.data_ptr(), dist2.data_ptr(),
                                                  nearest.data_ptr(), stream)
            xy = lambda: slices.distance_device(seed.data_ptr(), 0, n * n, F * n, False, dist2.data_ptr(), nearest.data_ptr(), stream)
            two_d = lambda: flat.distance_device(seed.data_ptr(), 0, side * side, frames2d, False, dist2.data_ptr(), nearest.data_ptr(),
                                                 stream)

            def copy():
                dist2.view(-1).copy_(seed.view(-1))
                nearest.view(-1).copy_(seed.view(-1))

            t = alternate(torch, {"full": full, "xy": xy, "copy": copy, "2-D": two_d}, args.brackets)
            z = t["full"][0] - t["xy"][0]
            floor = voxels * 9 / (STREAM_TBPS * 1e12)                       # the seed read, two int32 outputs written
            say(f"{F} x {n}^3, {content} ({int(seed.sum())} seeds of {voxels}): full {fmt(t['full'])}  xy {fmt(t['xy'])}  "
                f"copy {fmt(t['copy'])}  2-D {frames2d} x {side}^2 {fmt(t['2-D'])}")
            say(f"{'':>6s} z = full - xy = {z * 1e3:.3f} ms = {z / t['xy'][0]:.2f} x xy; full / copy = {t['full'][0] / t['copy'][0]:.1f}"
                f"; full / 2-D = {t['full'][0] / t['2-D'][0]:.2f}" + (" (SLOWER THAN THE 2-D TRANSFORM)" if t['full'][0] > t['2-D'][0] else "")
                + f"; xy / 2-D = {t['xy'][0] / t['2-D'][0]:.2f}; 9 bytes per voxel at {STREAM_TBPS} TB/s: {floor * 1e3:.4f} ms, full = "
                f"{t['full'][0] / floor:.0f} x that; {voxels / t['full'][0] / 1e9:.2f} G voxels/s")
            rows.append(dict(n=n, F=F, content=content, full_ms=t["full"][0] * 1e3, xy_ms=t["xy"][0] * 1e3, z_ms=z * 1e3,
                             copy_ms=t["copy"][0] * 1e3, two_d_ms=t["2-D"][0] * 1e3))
        # ---- the fields, end to end
        del seeds, seed, work, dist2, nearest
        torch.cuda.empty_cache()
        spacing, trunc = 2.0 / n, 6.0 / n
        tsdf = torch.clamp(dist * spacing, max=trunc)
        tsdf[dist * spacing < -trunc] = float("nan")
        inside = dist < 0
        fns = {"esdf": lambda: volume.esdf(tsdf, spacing, trunc), "occupancy_sdf": lambda: volume.occupancy_sdf(inside, spacing)}
        if (n, F) == sizes[0][:2]:
            m = synth.make_model(0)
            seq = synth.make_sequence(m, 1, seed=4)
            layer = tl.SMPLLayer(api.Model(m), R0=seq.R0.reshape(1, 3, 3))
            with torch.no_grad():
                verts = layer(torch.tensor(seq.gt_params, device="cuda"), torch.tensor(seq.gt_beta, device="cuda"))[0]
            lo, hi = (a.cpu().numpy().astype(np.float64) for a in (verts[0].min(dim=0).values, verts[0].max(dim=0).values))
            faces = synth.make_faces(m)
            fns["voxelize_sdf"] = lambda: volume.voxelize_sdf(verts, faces, tuple(lo - 0.1), tuple((hi - lo + 0.2) / (n - 1)), (n, n, n))
        t = alternate(torch, fns, args.brackets)
        text = f"{F} x {n}^3 fields of a sphere's TSDF: " + "  ".join(f"{k} {fmt(v)}" for k, v in t.items())
        if "voxelize_sdf" in t:
            text += (f"; voxelize_sdf of a body ({verts.shape[1]} vertices, {len(faces)} faces) / esdf = "
                     f"{t['voxelize_sdf'][0] / t['esdf'][0]:.1f}, / occupancy_sdf = {t['voxelize_sdf'][0] / t['occupancy_sdf'][0]:.1f}")
        say(text)
        rows.append(dict(n=n, F=F, **{k + "_ms": v[0] * 1e3 for k, v in t.items()}))
        del tsdf, inside, dist, fns
        torch.cuda.empty_cache()

    # ---- the 2-D transform, untouched: this build against the parent's, side by side
    if args.parent_lib:
        W, H, F = (96, 54, 4) if args.quick else (1920, 1080, 32)
        gen = torch.Generator(device="cuda").manual_seed(5)
        seed = (torch.rand((F, H, W), device="cuda", generator=gen) < 0.3).to(torch.uint8)
        libs = {"this build": api.load_library(), "parent": ctypes.CDLL(os.path.abspath(args.parent_lib))}
        outs, fns = {}, {}
        for name, lib in libs.items():
            lib.bodyfit_raster_create.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.POINTER(ctypes.c_void_p)]
            lib.bodyfit_raster_distance_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            h = ctypes.c_void_p()
            assert lib.bodyfit_raster_create(0, 0, 0, None, W, H, ctypes.byref(h)) == 0
            d = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
            nr = torch.empty_like(d)
            outs[name] = (d, nr)

            def run(lib=lib, h=h, d=d, nr=nr):
                assert lib.bodyfit_raster_distance_device(h, seed.data_ptr(), 0, H * W, F, 0, d.data_ptr(), nr.data_ptr(), stream) == 0
            fns[name] = run
        t = alternate(torch, fns, args.brackets)
        same = all(torch.equal(a, b) for a, b in zip(outs["this build"], outs["parent"]))
        spread = max((v[2] - v[1]) / v[0] for v in t.values())
        say(f"k_edt_rows + k_edt_cols, {F} x {W} x {H}: " + "  ".join(f"{k} {fmt(v)}" for k, v in t.items())
            + f"; this build / parent = {t['this build'][0] / t['parent'][0]:.3f} (the brackets of one build spread over "
            f"{100 * spread:.1f} % of its median); outputs {'bit-identical' if same else 'DIFFER'}")
        rows.append({"2-D transform": {k: v[0] * 1e3 for k, v in t.items()}})
    lines.append("# json: " + json.dumps(rows))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
