"""Times of the silhouette-edge antialiasing (bodyfit_raster_edges_device, bodyfit_raster_edge_blend_device,
bodyfit_raster_edge_rows_device) and of the layer on top of them (torch_layer.antialias, CoverageTerm) at SMPL's size, 6890
vertices / 13,776 faces of synth.make_faces, for 1920 x 1080 images of 32 and 256 frames of one posed synthetic sequence.
Timed with the protocol of tools/appearance_bench.py (a warm-up, then --brackets brackets of back-to-back calls, host clock around
work that ends in a device synchronise; median [min .. max] of the brackets); the alternatives of one comparison are ALTERNATED
bracket by bracket inside one call, so a drift of the machine falls on both:
  edges      k_rs_edges over the frames' own render, against
             render  the render it follows (bodyfit_raster_render_device without barycentrics),
             fill    a plain fill of its output (8 bytes per pixel),
             floor   the bytes a pixel needs (face 4, depth 4, weights 8) over 6.3 TB/s, the streaming rate the machine sustains;
  blend      k_rs_edge_blend at C = 1 and C = 3, forward and transposed, against a plain copy of the image into the output and the
             floor of (8 + 8 C) bytes per pixel;
  rows       k_rs_edge_rows at C = 3 over the blended pairs (nonzero of the weights), against a fill of its 64 bytes per pair;
  antialias  torch_layer.antialias forward + backward (C = 3, gradients in image and verts) with its parts;
  terms      CoverageTerm forward + backward beside SilhouetteTerm forward + backward on the same mask;
  census     candidate pairs (the two face ids differ), blended pairs (a non-zero weight) and blended pairs whose walk left the near
             pixel's own face (the rows' face is not the near pixel's);
  render     bodyfit_raster_render_device of THIS library against the same call of another build of the library (--parent-lib: the
             parent commit's libbodyfit.so), alternating: the render's kernels are untouched, its time must be too.
Nothing is asserted; every comparison is printed whichever way it falls.
Usage: python3 tools/antialias_bench.py [--size 1920x1080] [--frames 32 256] [--brackets 5] [--parent-lib PATH]
                                        [--out profiles/antialias_bench.txt]"""
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
    """bodyfit_raster_create / _render_device / _destroy of one loaded library, by ctypes alone: the same calls for both builds"""

    def __init__(self, lib, n_verts, faces, W, H):
        self.lib = lib
        lib.bodyfit_raster_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        lib.bodyfit_raster_destroy.argtypes = [C.c_void_p]
        lib.bodyfit_raster_destroy.restype = None
        lib.bodyfit_raster_render_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_double,
                                                     C.c_double, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        f = np.ascontiguousarray(faces, np.int32)
        self.h = C.c_void_p()
        rc = lib.bodyfit_raster_create(0, n_verts, len(f), f.ctypes.data_as(C.POINTER(C.c_int32)), W, H, C.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"bodyfit_raster_create: status {rc}")

    def render(self, verts, stride, F, intr, depth, face, stream):
        rc = self.lib.bodyfit_raster_render_device(self.h, verts.data_ptr(), stride, F, *intr, 0.1, 0, depth.data_ptr(), face.data_ptr(),
                                                   None, stream)
        if rc != 0:
            raise RuntimeError(f"bodyfit_raster_render_device: status {rc}")

    def close(self):
        self.lib.bodyfit_raster_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", nargs="*", type=int, default=[32, 256])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "antialias_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    if api.device_count() < 1:
        raise SystemExit("antialias_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    seq = synth.make_sequence(model, max(args.frames), seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    V = model.n_verts
    W, H = (int(a) for a in args.size.split("x"))
    intr = tuple(float(a) for a in synth.camera_intrinsics(W, H))
    stream = torch.cuda.current_stream().cuda_stream
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# antialias_bench: V={V} n_faces={len(faces)} size={args.size} brackets={args.brackets}; times in ms per call: "
             f"median [min .. max] x calls per bracket; alternatives alternate bracket by bracket"]
    out_rows = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for F in args.frames:
        verts = torch.tensor(cloud[:F], device="cuda")
        raster = tl._raster_handle(0, V, faces, (H, W))
        depth = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
        face = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
        w = torch.empty((F, H, W, 2), dtype=torch.float32, device="cuda")
        pixels = F * H * W

        def render():
            raster.render_device(verts.data_ptr(), 3 * V, F, intr, depth.data_ptr(), face.data_ptr(), None, stream=stream)

        def edges():
            raster.edges_device(verts.data_ptr(), 3 * V, F, intr, face.data_ptr(), depth.data_ptr(), w.data_ptr(), stream=stream)

        render()
        t = alternate(torch, {"render": render, "edges": edges, "fill": lambda: w.fill_(0.5)}, args.brackets)
        edges()
        torch.cuda.synchronize()
        covered = float((face >= 0).float().mean())
        n_cand = int((face[:, :, 1:] != face[:, :, :-1]).sum()) + int((face[:, 1:, :] != face[:, :-1, :]).sum())
        frame, code = torch.nonzero(w.reshape(F, -1), as_tuple=True)
        N = int(code.shape[0])
        floor = pixels * 16 / (STREAM_TBPS * 1e12)
        say(f"{args.size:>9s} F={F:<3d} edges ({covered * 100:.1f}% of the pixels covered): edges {fmt(t['edges'])}  render {fmt(t['render'])}  "
            f"fill of the weights {fmt(t['fill'])}")
        say(f"{'':>9s}       floor {floor * 1e3:.3f} ms (16 bytes per pixel at {STREAM_TBPS} TB/s): edges = {t['edges'][0] / floor:.2f} x floor, "
            f"{pixels * 16 / t['edges'][0] / 1e12:.2f} TB/s; edges / fill = {t['edges'][0] / t['fill'][0]:.2f}; edges / render = "
            f"{t['edges'][0] / t['render'][0]:.3f}")
        row = dict(frames=F, covered=covered, candidates=n_cand, blended=N, edges_ms=t["edges"][0] * 1e3, render_ms=t["render"][0] * 1e3,
                   fill_w_ms=t["fill"][0] * 1e3, edges_floor_ms=floor * 1e3)

        # ---- blend, C = 1 and C = 3
        for Cn in (1, 3):
            img = torch.rand((F, H, W, Cn), dtype=torch.float32, device="cuda")
            out = torch.empty_like(img)

            def blend(tr):
                raster.edge_blend_device(w.data_ptr(), img.data_ptr(), Cn, F, tr, out.data_ptr(), stream)

            t = alternate(torch, {"blend": lambda: blend(False), "blendT": lambda: blend(True), "copy": lambda: out.copy_(img)},
                          args.brackets)
            floor = pixels * (8 + 8 * Cn) / (STREAM_TBPS * 1e12)
            say(f"{args.size:>9s} F={F:<3d} blend C={Cn}: blend {fmt(t['blend'])}  transposed {fmt(t['blendT'])}  copy of the image "
                f"{fmt(t['copy'])}; floor {floor * 1e3:.3f} ms ({8 + 8 * Cn} bytes per pixel): blend = {t['blend'][0] / floor:.2f} x floor, "
                f"{pixels * (8 + 8 * Cn) / t['blend'][0] / 1e12:.2f} TB/s; blend / copy = {t['blend'][0] / t['copy'][0]:.2f}; blend / render = "
                f"{t['blend'][0] / row['render_ms'] * 1e3:.3f}")
            row.update({f"blend{Cn}_ms": t["blend"][0] * 1e3, f"blendT{Cn}_ms": t["blendT"][0] * 1e3, f"copy{Cn}_ms": t["copy"][0] * 1e3,
                        f"blend{Cn}_floor_ms": floor * 1e3})
            del out
            if Cn == 1:
                del img

        # ---- rows, C = 3, over the blended pairs
        grad = torch.rand_like(img)
        pair = code.to(torch.int32).contiguous()
        offset = torch.zeros(F + 1, dtype=torch.int32, device="cuda")
        offset[1:] = torch.bincount(frame, minlength=F).cumsum(0).to(torch.int32)
        index = torch.empty(2 * N, dtype=torch.int32, device="cuda")
        bary = torch.empty((2 * N, 3), dtype=torch.float32, device="cuda")
        coef = torch.empty(2 * N, dtype=torch.float32, device="cuda")
        direction = torch.empty((2 * N, 3), dtype=torch.float32, device="cuda")

        def rows():
            raster.edge_rows_device(verts.data_ptr(), 3 * V, F, intr, face.data_ptr(), depth.data_ptr(), img.data_ptr(), grad.data_ptr(), 3,
                                    pair.data_ptr(), offset.data_ptr(), N, index.data_ptr(), bary.data_ptr(), coef.data_ptr(),
                                    direction.data_ptr(), stream=stream)

        def rows_fill():
            index.fill_(1); bary.fill_(0.5); coef.fill_(0.5); direction.fill_(0.5)

        t = alternate(torch, {"rows": rows, "fill": rows_fill}, args.brackets)
        rows()
        # a walk that left the near pixel's own face: the rows' face is not the near pixel's
        pix = torch.div(code, 2, rounding_mode="floor")
        other = pix + torch.where(code % 2 == 1, W, 1)
        ff, dd = face.reshape(F, -1), depth.reshape(F, -1)
        near_face = torch.where(dd[frame, pix] <= dd[frame, other], ff[frame, pix], ff[frame, other])
        n_walked = int((index[0::2] != near_face).sum())
        n_void = int((index[0::2] < 0).sum())
        say(f"{args.size:>9s} F={F:<3d} rows C=3: {n_cand} candidate pairs ({n_cand / pixels * 100:.2f}% of the pixels), {N} blended, {n_walked} of "
            f"them walked past the near pixel's face, {n_void} listed pairs void; rows {fmt(t['rows'])}  fill of the rows {fmt(t['fill'])}; "
            f"rows / fill = {t['rows'][0] / t['fill'][0]:.2f}; {N / t['rows'][0] / 1e9:.3f} G pairs/s; rows / render = "
            f"{t['rows'][0] / row['render_ms'] * 1e3:.4f}")
        row.update(walked=n_walked, rows_ms=t["rows"][0] * 1e3, rows_fill_ms=t["fill"][0] * 1e3)
        del index, bary, coef, direction, grad, pair

        # ---- the layer: antialias forward + backward, and the two outline terms
        leaf = verts.clone().requires_grad_()
        image = img.clone().requires_grad_()

        def whole():
            leaf.grad = None
            image.grad = None
            tl.antialias(image, leaf, faces, intr).sum().backward()

        def forward_only():
            with torch.no_grad():
                tl.antialias(img, verts, faces, intr)

        t = alternate(torch, {"antialias": whole, "forward": forward_only, "render": render}, args.brackets)
        say(f"{args.size:>9s} F={F:<3d} antialias C=3 forward + backward (image and verts) {fmt(t['antialias'])}  forward alone (with its "
            f"render) {fmt(t['forward'])}  render {fmt(t['render'])}; whole / render = {t['antialias'][0] / t['render'][0]:.2f}")
        row.update(antialias_ms=t["antialias"][0] * 1e3, antialias_forward_ms=t["forward"][0] * 1e3)
        del image, img
        torch.cuda.empty_cache()
        shifted = verts.clone()
        shifted[..., 0] += 0.004
        with torch.no_grad():
            mask = tl.render_depth(shifted, faces, intr, (H, W))[1] >= 0
        cov, sil = tl.CoverageTerm(mask, intr, faces), tl.SilhouetteTerm(mask, intr, faces)

        def term(tm):
            leaf.grad = None
            tm(leaf).backward()

        t = alternate(torch, {"coverage": lambda: term(cov), "silhouette": lambda: term(sil)}, args.brackets)
        say(f"{args.size:>9s} F={F:<3d} CoverageTerm forward + backward {fmt(t['coverage'])}  SilhouetteTerm forward + backward "
            f"{fmt(t['silhouette'])}; coverage / silhouette = {t['coverage'][0] / t['silhouette'][0]:.2f}")
        row.update(coverage_ms=t["coverage"][0] * 1e3, silhouette_ms=t["silhouette"][0] * 1e3)
        del cov, sil, mask, shifted, leaf

        # ---- the render of this build against another build's, alternating
        if args.parent_lib:
            new, old = RawRaster(api.load_library(), V, faces, W, H), RawRaster(C.CDLL(os.path.abspath(args.parent_lib)), V, faces, W, H)
            d2, f2 = torch.empty_like(depth), torch.empty_like(face)
            t = alternate(torch, {"new": lambda: new.render(verts, 3 * V, F, intr, depth, face, stream),
                                  "parent": lambda: old.render(verts, 3 * V, F, intr, d2, f2, stream)}, max(args.brackets, 7))
            same = bool(torch.equal(face, f2)) and bool(torch.equal(depth.view(torch.int32), d2.view(torch.int32)))
            say(f"{args.size:>9s} F={F:<3d} render, this build {fmt(t['new'])}  the other build {fmt(t['parent'])}; this / other = "
                f"{t['new'][0] / t['parent'][0]:.4f}; images bit-identical: {same}")
            row.update(render_new_ms=t["new"][0] * 1e3, render_parent_ms=t["parent"][0] * 1e3, render_new_range_ms=[t["new"][1] * 1e3, t["new"][2] * 1e3],
                       render_parent_range_ms=[t["parent"][1] * 1e3, t["parent"][2] * 1e3], render_identical=same)
            new.close(); old.close()
            del d2, f2
        out_rows.append(row)
        del depth, face, w, verts
        torch.cuda.empty_cache()
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
