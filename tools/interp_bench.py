"""Times of the interpolation rows (bodyfit_raster_interp_rows_device, k_rs_interp_rows) and of the layer on top of them
(torch_layer.render_attributes(interior=True), RenderedPhotometricTerm) at SMPL's size, 6890 vertices / 13,776 faces of
synth.make_faces, for 1920 x 1080 images of 32 and 256 frames of one posed synthetic sequence.
Timed with the protocol of tools/appearance_bench.py and tools/antialias_bench.py (a warm-up, then --brackets brackets of at least
0.15 s of back-to-back calls, host clock around work that ends in a device synchronise; median [min .. max] of the brackets); the
alternatives of one comparison are ALTERNATED bracket by bracket inside one call, so a drift of the machine falls on both:
  rows       k_rs_interp_rows at C = 3 (upstream in the image) and C = 0 (upstream in z), over the list of the covered pixels and
             over all pixels, against
             depth   k_rs_depth_rows on the SAME rows with its four outputs (the yardstick: the same gathers, the same
                     beta and m, no attributes),
             floor   the bytes a row streams over 6.3 TB/s: list: pixel 4 + face 4 + index 4 + bary 12 + dir 12 = 36, + 12 of G
                     at C = 3 (48) or 4 of g_z at C = 0 (40); depth rows 36 + 4 of z = 40; over all pixels no pixel list (- 4)
                     and an empty pixel reads 4 and writes 28 (32 for the depth rows).  The gathers (12 bytes of ids, 36 of corners, 36 of attributes,
                     shared by the neighbouring rows of a face) are NOT counted;
  layer      render_attributes forward + backward with an upstream in the image: attr only; attr and verts with interior=True;
             and its parts: the nonzero that lists the shaded pixels, the rows VJP over them;
  terms      RenderedPhotometricTerm forward + backward beside PhotometricTerm and CoverageTerm;
  parent     with --parent-lib (the parent commit's libbodyfit.so): render, shade and edges of this build against the other's,
             alternating, the images compared bit for bit: those kernels are untouched, their times must be too.
Nothing is asserted; every comparison is printed whichever way it falls.  No hardware counters are read here.
Usage: python3 tools/interp_bench.py [--size 1920x1080] [--frames 32 256] [--brackets 5] [--parent-lib PATH]
                                     [--out profiles/interp_bench.txt]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBPS = 6.3          # what a float4 copy sustains on the MI355X: the floor's rate


def alternate(torch, fns, n_brackets, min_seconds=0.15, max_reps=2000):
    """{name: (median, min, max, reps)} seconds per call; after a warm-up of each, the brackets of the alternatives take turns"""
    reps = {}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        reps[name] = int(min(max(min_seconds / max(time.perf_counter() - t0, 1e-6), 1), max_reps))
    out = {name: [] for name in fns}
    for _ in range(n_brackets):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / reps[name])
    return {name: (float(np.median(t)), float(min(t)), float(max(t)), reps[name]) for name, t in out.items()}


class RawRaster:
    """create / render / shade / edges / destroy of one loaded library, by ctypes alone: the same calls for both builds"""

    def __init__(self, lib, n_verts, faces, W, H):
        self.lib = lib
        vp, ll, i, d, fl = C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_float
        lib.bodyfit_raster_create.argtypes = [i, i, i, C.POINTER(C.c_int32), i, i, C.POINTER(vp)]
        lib.bodyfit_raster_destroy.argtypes = [vp]
        lib.bodyfit_raster_destroy.restype = None
        lib.bodyfit_raster_render_device.argtypes = [vp, vp, ll, i, d, d, d, d, fl, i, vp, vp, vp, vp]
        lib.bodyfit_raster_shade_device.argtypes = [vp, vp, vp, vp, ll, vp, ll, i, i, C.POINTER(fl), vp, vp, vp]
        lib.bodyfit_raster_edges_device.argtypes = [vp, vp, ll, i, d, d, d, d, fl, i, vp, vp, vp, vp]
        f = np.ascontiguousarray(faces, np.int32)
        self.h = vp()
        self.check(lib.bodyfit_raster_create(0, n_verts, len(f), f.ctypes.data_as(C.POINTER(C.c_int32)), W, H, C.byref(self.h)))

    @staticmethod
    def check(rc):
        if rc != 0:
            raise RuntimeError(f"bodyfit status {rc}")

    def render(self, verts, stride, F, intr, depth, face, bary, stream):
        self.check(self.lib.bodyfit_raster_render_device(self.h, verts.data_ptr(), stride, F, *intr, 0.1, 0, depth.data_ptr(),
                                                         face.data_ptr(), bary.data_ptr(), stream))

    def shade(self, face, bary, verts, stride, attr, Cn, F, image, weight, stream):
        self.check(self.lib.bodyfit_raster_shade_device(self.h, face.data_ptr(), bary.data_ptr(), verts.data_ptr(), stride, attr.data_ptr(),
                                                        0, Cn, F, None, image.data_ptr(), weight.data_ptr(), stream))

    def edges(self, verts, stride, F, intr, face, depth, w, stream):
        self.check(self.lib.bodyfit_raster_edges_device(self.h, verts.data_ptr(), stride, F, *intr, 0.1, 0, face.data_ptr(), depth.data_ptr(),
                                                        w.data_ptr(), stream))

    def close(self):
        self.lib.bodyfit_raster_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", nargs="*", type=int, default=[32, 256])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    if api.device_count() < 1:
        raise SystemExit("interp_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    seq = synth.make_sequence(model, max(args.frames), seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    V, Cn = model.n_verts, 3
    W, H = (int(a) for a in args.size.split("x"))
    intr = tuple(float(a) for a in synth.camera_intrinsics(W, H))
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    colours = torch.tensor(rng.uniform(0, 255, size=(V, Cn)).astype(np.float32), device="cuda")
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# interp_bench: V={V} n_faces={len(faces)} size={args.size} C={Cn} brackets={args.brackets}; times in ms per call: "
             f"median [min .. max] x calls per bracket; alternatives alternate bracket by bracket"]
    out_rows = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for F in args.frames:
        verts = torch.tensor(cloud[:F], device="cuda")
        raster = tl._raster_handle(0, V, faces, (H, W))
        surface = tl._surface_handle(0, V, faces)
        depth = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
        face = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
        raster.render_device(verts.data_ptr(), 3 * V, F, intr, depth.data_ptr(), face.data_ptr(), None, stream=stream)
        pixels = F * H * W
        frame, pix = torch.nonzero((face >= 0).reshape(F, -1), as_tuple=True)
        Nc = int(pix.shape[0])
        pixel = pix.to(torch.int32).contiguous()
        offset = torch.zeros(F + 1, dtype=torch.int32, device="cuda")
        offset[1:] = torch.bincount(frame, minlength=F).cumsum(0).to(torch.int32)
        del frame, pix
        G = torch.randn((F, H, W, Cn), device="cuda")
        gz = torch.randn((F, H, W), device="cuda")
        row = dict(frames=F, covered=Nc / pixels, rows_list=Nc, rows_all=pixels)

        for label, N, px, of in (("list", Nc, pixel, offset), ("all", pixels, None, None)):
            index = torch.empty(N, dtype=torch.int32, device="cuda")
            z = torch.empty(N, dtype=torch.float32, device="cuda")
            bary = torch.empty((N, 3), dtype=torch.float32, device="cuda")
            direction = torch.empty((N, 3), dtype=torch.float32, device="cuda")
            ptr = lambda t: None if t is None else t.data_ptr()

            def interp(c):
                raster.interp_rows_device(verts.data_ptr(), 3 * V, F, intr, face.data_ptr(), ptr(px), ptr(of), N,
                                          colours.data_ptr() if c else None, 0, c, G.data_ptr() if c else None,
                                          None if c else gz.data_ptr(), index.data_ptr(), bary.data_ptr(), direction.data_ptr(), None, stream)

            def depth_rows():
                raster.depth_rows_device(verts.data_ptr(), 3 * V, F, intr, face.data_ptr(), ptr(px), ptr(of), N, index.data_ptr(),
                                         z.data_ptr(), bary.data_ptr(), direction.data_ptr(), stream)

            t = alternate(torch, {"c3": lambda: interp(3), "c0": lambda: interp(0), "depth": depth_rows}, args.brackets)
            depth_rows()
            b_depth = bary.clone()
            interp(3)
            same = bool(torch.equal(b_depth.view(torch.int32), bary.view(torch.int32)))
            del b_depth
            if label == "list":
                by = dict(c3=48 * N, c0=40 * N, depth=40 * N)
            else:
                by = dict(c3=44 * Nc + 32 * (N - Nc), c0=36 * Nc + 32 * (N - Nc), depth=36 * N)
            floor = {k: v / (STREAM_TBPS * 1e12) for k, v in by.items()}
            say(f"{args.size:>9s} F={F:<3d} rows over {'the covered pixels' if label == 'list' else 'all pixels'} ({N} rows, {Nc} live): "
                f"interp C=3 {fmt(t['c3'])}  interp C=0 {fmt(t['c0'])}  depth rows {fmt(t['depth'])}")
            say(f"{'':>9s}       interp C=3 / depth rows = {t['c3'][0] / t['depth'][0]:.3f}, C=0 / depth rows = {t['c0'][0] / t['depth'][0]:.3f}; "
                f"floors {floor['c3'] * 1e3:.3f} / {floor['c0'] * 1e3:.3f} / {floor['depth'] * 1e3:.3f} ms ({by['c3'] / N:.1f} / {by['c0'] / N:.1f} / "
                f"{by['depth'] / N:.1f} bytes per row at {STREAM_TBPS} TB/s): C=3 = {t['c3'][0] / floor['c3']:.2f} x floor, C=0 = "
                f"{t['c0'][0] / floor['c0']:.2f} x, depth rows = {t['depth'][0] / floor['depth']:.2f} x; {N / t['c3'][0] / 1e9:.2f} G rows/s at C=3; "
                f"beta bit-identical to the depth rows': {same}")
            row.update({f"{label}_interp_c3_ms": t["c3"][0] * 1e3, f"{label}_interp_c0_ms": t["c0"][0] * 1e3, f"{label}_depth_rows_ms": t["depth"][0] * 1e3,
                        f"{label}_floor_c3_ms": floor["c3"] * 1e3, f"{label}_floor_c0_ms": floor["c0"] * 1e3, f"{label}_floor_depth_ms": floor["depth"] * 1e3,
                        f"{label}_beta_identical": same})
            if label == "list":
                coef = torch.ones(N, dtype=torch.float32, device="cuda")
                gv = torch.empty((F, V, 3), dtype=torch.float32, device="cuda")
                rows = api.PointSet.ragged(index.data_ptr(), offset.data_ptr())
                weight_like = (face >= 0).reshape(F, -1)

                def vjp():
                    surface.rows_vjp_device(rows, F, N, index.data_ptr(), bary.data_ptr(), coef.data_ptr(), direction.data_ptr(),
                                            gv.data_ptr(), 3 * V, stream)

                t = alternate(torch, {"vjp": vjp, "nonzero": lambda: torch.nonzero(weight_like, as_tuple=True)}, args.brackets)
                say(f"{'':>9s}       parts of the interior backward over these rows: the rows VJP {fmt(t['vjp'])}  the nonzero that lists them {fmt(t['nonzero'])}")
                row.update(rows_vjp_ms=t["vjp"][0] * 1e3, nonzero_ms=t["nonzero"][0] * 1e3)
                del coef, gv, weight_like
            del index, z, bary, direction
            torch.cuda.empty_cache()
        del G, gz, pixel, offset

        # ---- the layer: render_attributes forward + backward, without and with the interior gradients
        leaf = verts.clone().requires_grad_()
        cols = colours.clone().requires_grad_()
        up = torch.randn((F, H, W, Cn), device="cuda")

        def layer(interior):
            leaf.grad = None
            cols.grad = None
            image, _ = tl.render_attributes(leaf, faces, intr, (H, W), cols, interior=interior)
            image.backward(up)

        def forward_only():
            with torch.no_grad():
                tl.render_attributes(leaf, faces, intr, (H, W), cols)

        t = alternate(torch, {"plain": lambda: layer(False), "interior": lambda: layer(True), "forward": forward_only}, args.brackets)
        say(f"{args.size:>9s} F={F:<3d} render_attributes forward + backward: attr only {fmt(t['plain'])}  with interior=True {fmt(t['interior'])}  "
            f"forward alone {fmt(t['forward'])}; interior / plain = {t['interior'][0] / t['plain'][0]:.3f}, the interior's share "
            f"{(t['interior'][0] - t['plain'][0]) * 1e3:.3f} ms")
        row.update(layer_plain_ms=t["plain"][0] * 1e3, layer_interior_ms=t["interior"][0] * 1e3, layer_forward_ms=t["forward"][0] * 1e3)
        del up

        # ---- the terms
        with torch.no_grad():
            image, face_r = tl.render_attributes(verts, faces, intr, (H, W), colours)
            video = tl.antialias(image, verts, faces, intr).clamp(0, 255).to(torch.uint8)
            mask = face_r >= 0
            del image, face_r
        shifted = verts.clone()
        shifted[..., 0] += 0.4 * shifted[..., 2] / intr[0]
        leaf = shifted.requires_grad_()
        dense = tl.RenderedPhotometricTerm(video, intr, faces, trunc=60.0)
        sparse = tl.PhotometricTerm(video, intr, faces, trunc=60.0, min_cos=0.2, owner=True)
        cov = tl.CoverageTerm(mask, intr, faces)

        def term(tm, two):
            leaf.grad = None
            cols.grad = None
            (tm(leaf, cols) if two else tm(leaf)).backward()

        t = alternate(torch, {"dense": lambda: term(dense, True), "sparse": lambda: term(sparse, True), "coverage": lambda: term(cov, False)},
                      args.brackets)
        say(f"{args.size:>9s} F={F:<3d} forward + backward: RenderedPhotometricTerm {fmt(t['dense'])}  PhotometricTerm {fmt(t['sparse'])}  "
            f"CoverageTerm {fmt(t['coverage'])}; dense / PhotometricTerm = {t['dense'][0] / t['sparse'][0]:.2f}, dense / CoverageTerm = "
            f"{t['dense'][0] / t['coverage'][0]:.2f}")
        row.update(rendered_term_ms=t["dense"][0] * 1e3, photometric_term_ms=t["sparse"][0] * 1e3, coverage_term_ms=t["coverage"][0] * 1e3)
        del dense, sparse, cov, video, mask, leaf, cols, shifted
        torch.cuda.empty_cache()

        # ---- render, shade and edges of this build against another build's, alternating
        if args.parent_lib:
            new, old = RawRaster(api.load_library(), V, faces, W, H), RawRaster(C.CDLL(os.path.abspath(args.parent_lib)), V, faces, W, H)
            outs = []
            for _ in range(2):
                outs.append(dict(depth=torch.empty((F, H, W), dtype=torch.float32, device="cuda"), face=torch.empty((F, H, W), dtype=torch.int32, device="cuda"),
                                 bary=torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda"), image=torch.empty((F, H, W, Cn), dtype=torch.float32, device="cuda"),
                                 weight=torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda"), w=torch.empty((F, H, W, 2), dtype=torch.float32, device="cuda")))
            fns = {}
            for name, r, o in (("new", new, outs[0]), ("parent", old, outs[1])):
                fns[f"render_{name}"] = lambda r=r, o=o: r.render(verts, 3 * V, F, intr, o["depth"], o["face"], o["bary"], stream)
                fns[f"shade_{name}"] = lambda r=r, o=o: r.shade(o["face"], o["bary"], verts, 3 * V, colours, Cn, F, o["image"], o["weight"], stream)
                fns[f"edges_{name}"] = lambda r=r, o=o: r.edges(verts, 3 * V, F, intr, o["face"], o["depth"], o["w"], stream)
            for k in ("render", "shade", "edges"):
                t = alternate(torch, {"new": fns[f"{k}_new"], "parent": fns[f"{k}_parent"]}, max(args.brackets, 7))
                keys = dict(render=("depth", "face", "bary"), shade=("image", "weight"), edges=("w",))[k]
                same = all(bool(torch.equal(outs[0][q].view(torch.int32), outs[1][q].view(torch.int32))) for q in keys)
                say(f"{args.size:>9s} F={F:<3d} {k}, this build {fmt(t['new'])}  the other build {fmt(t['parent'])}; this / other = "
                    f"{t['new'][0] / t['parent'][0]:.4f}; images bit-identical: {same}")
                row.update({f"{k}_new_ms": t["new"][0] * 1e3, f"{k}_parent_ms": t["parent"][0] * 1e3, f"{k}_identical": same})
            new.close(); old.close()
            del outs, fns
        out_rows.append(row)
        del depth, face, verts
        torch.cuda.empty_cache()
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
