"""Times of the texture lookup (bodyfit_raster_texture_device, k_tx_forward), of its gradients (bodyfit_raster_texture_grad_device:
k_tx_gmax, k_tx_grad, k_tx_fold) and of the layer on top of them (torch_layer.render_texture, TexturedPhotometricTerm) at SMPL's
size, 6890 vertices / 13,776 faces of synth.make_faces with the "cylinder" atlas of synth.make_uv_atlas, for 1920 x 1080 images
of 32 and 256 frames of one posed synthetic sequence, C = 3, f32 textures of 256^2 and 1024^2 shared by the frames.
Timed with the protocol of tools/interp_bench.py (its `alternate`: a warm-up, then brackets of at least 0.15 s of back-to-back
calls, host clock around work that ends in a device synchronise; median [min .. max]; the alternatives of one comparison take
turns bracket by bracket, so a drift of the machine falls on all of them):
  forward    k_tx_forward beside k_rs_shade<3> on the same render (vertex colours in place of the texture), with the bytes a
             pixel streams over 6.3 TB/s as the floor: face 4 + bary 12 + image 12 + weight 12 = 40 for both (the gathers of ids,
             z, uv and texels are not counted); and beside the torch composition render_attributes(uv per vertex) + grid_sample
             (bilinear, border, align_corners=False) on the same render;
  gradient   the entry with d_grad_tex alone, split by what it launches: the same call with an all-zero upstream gradient runs
             the max pass, the clears and the fold but adds nothing (the adding pass leaves after one load), so
             accumulate = full - zero; the integer adds per second are the covered pixels x 4 x C over that difference.  Beside it
             grid_sample's backward into the texture (float atomics, then the sum over the frames' copies);
  layer      render_texture forward + backward in tex, and in tex, uv and verts (interior=True); TexturedPhotometricTerm forward
             + backward in tex and verts;
  variant    with --variant-lib (this library built with -DBODYFIT_TX_COMBINE=1, or =0 if 1 is the default): the gradient entry of
             both builds, alternating, the gradients compared bit for bit: equal destinations combined inside the wave, or not;
  parent     with --parent-lib (the parent commit's libbodyfit.so): render, k_rs_shade, k_rs_sample and k_rs_interp_rows of this
             build against the other's, alternating, outputs compared bit for bit; the other build is timed TWICE in the same
             alternation and the ratio of its two medians is printed beside this / other: the margin.
Nothing is asserted; every comparison is printed whichever way it falls.  No hardware counters are read here.
Usage: python3 tools/texture_bench.py [--size 1920x1080] [--frames 32 256] [--textures 256 1024] [--brackets 5]
                                       [--parent-lib PATH] [--variant-lib PATH] [--out profiles/texture_bench.txt]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from interp_bench import STREAM_TBPS, RawRaster, alternate  # noqa: E402


class RawRaster2(RawRaster):
    """RawRaster with the sampler and the interpolation rows"""

    def __init__(self, lib, n_verts, faces, W, H):
        super().__init__(lib, n_verts, faces, W, H)
        vp, ll, i, d, fl = C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_float
        lib.bodyfit_raster_sample_device.argtypes = [vp, vp, ll, ll, i, d, d, d, d, fl, vp, i, i, ll, vp, vp, vp, vp, vp]
        lib.bodyfit_raster_interp_rows_device.argtypes = [vp, vp, ll, i, d, d, d, d, vp, vp, vp, ll, vp, ll, i, vp, vp, vp, vp, vp, vp, vp]

    def sample(self, verts, stride, n, F, intr, images, Cn, value, valid, grad, stream):
        self.check(self.lib.bodyfit_raster_sample_device(self.h, verts.data_ptr(), stride, n, F, *intr, 0.1, images.data_ptr(), 1, Cn,
                                                         images[0].numel(), None, value.data_ptr(), valid.data_ptr(), grad.data_ptr(), stream))

    def texture_grad(self, face, bary, verts, stride, uv, uvf, Cn, S, F, G, grad_tex, work, stream):
        vp, ll, i = C.c_void_p, C.c_longlong, C.c_int
        self.lib.bodyfit_raster_texture_grad_device.argtypes = [vp, vp, vp, vp, ll, vp, i, vp, vp, i, i, i, i, ll, i, vp, vp, vp, vp, vp]
        self.check(self.lib.bodyfit_raster_texture_grad_device(self.h, face.data_ptr(), bary.data_ptr(), verts.data_ptr(), stride, uv.data_ptr(),
                                                               uv.shape[0], uvf.data_ptr(), None, 1, Cn, S, S, 0, F, G.data_ptr(), None,
                                                               grad_tex.data_ptr(), work.data_ptr(), stream))

    def interp(self, verts, stride, F, intr, face, N, attr, Cn, G, index, bary, direction, stream):
        self.check(self.lib.bodyfit_raster_interp_rows_device(self.h, verts.data_ptr(), stride, F, *intr, face.data_ptr(), None, None, N,
                                                              attr.data_ptr(), 0, Cn, G.data_ptr(), None, index.data_ptr(), bary.data_ptr(),
                                                              direction.data_ptr(), None, stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", nargs="*", type=int, default=[32, 256])
    ap.add_argument("--textures", nargs="*", type=int, default=[256, 1024])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    if api.device_count() < 1:
        raise SystemExit("texture_bench needs a GPU: nothing here can be timed on the CPU")
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
    uv_h, uvf_h = synth.make_uv_atlas(faces, "cylinder", verts=model.v_template)
    uv, uvf = torch.tensor(uv_h, device="cuda"), torch.tensor(uvf_h, device="cuda")
    T = len(uv_h)
    uv_vertex = torch.tensor(uv_h[:V], device="cuda")                 # one uv per vertex: what the torch composition can express
    colours = torch.tensor(rng.uniform(0, 1, size=(V, Cn)).astype(np.float32), device="cuda")
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# texture_bench: V={V} n_faces={len(faces)} uv rows={T} size={args.size} C={Cn} brackets={args.brackets}; times in ms per "
             f"call: median [min .. max] x calls per bracket; alternatives alternate bracket by bracket"]
    out_rows = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for F in args.frames:
        verts = torch.tensor(cloud[:F], device="cuda")
        raster = tl._raster_handle(0, V, faces, (H, W))
        depth = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
        face = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
        bary = torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
        raster.render_device(verts.data_ptr(), 3 * V, F, intr, depth.data_ptr(), face.data_ptr(), bary.data_ptr(), stream=stream)
        pixels = F * H * W
        Nc = int((face >= 0).sum())
        image = torch.empty((F, H, W, Cn), dtype=torch.float32, device="cuda")
        weight = torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
        G = torch.randn((F, H, W, Cn), device="cuda")
        G0 = torch.zeros((F, H, W, Cn), device="cuda")
        floor = 40.0 * pixels / (STREAM_TBPS * 1e12)
        for S in args.textures:
            row = dict(frames=F, texture=S, covered=Nc / pixels, pixels=pixels)
            tex = torch.rand((S, S, Cn), device="cuda")
            grad_tex = torch.empty((S, S, Cn), dtype=torch.float32, device="cuda")
            work = torch.empty((S, S, Cn), dtype=torch.int64, device="cuda")

            def lookup():
                raster.texture_device(face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, uv.data_ptr(), T, uvf.data_ptr(),
                                      tex.data_ptr(), 1, Cn, S, S, 0, F, 0.0, image.data_ptr(), weight.data_ptr(), None, stream)

            def shade():
                raster.shade_device(face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, colours.data_ptr(), 0, Cn, F, 0.0,
                                    image.data_ptr(), weight.data_ptr(), stream)

            def composition():
                with torch.no_grad():
                    img, _ = tl.render_attributes(verts, faces, intr, (H, W), uv_vertex)
                    torch.nn.functional.grid_sample(tex.permute(2, 0, 1)[None].expand(F, -1, -1, -1), img * 2 - 1, mode="bilinear",
                                                    padding_mode="border", align_corners=False)

            def render_and_lookup():
                with torch.no_grad():
                    tl.render_texture(verts, faces, intr, (H, W), uv, uvf_h, tex)

            t = alternate(torch, {"lookup": lookup, "shade": shade, "composition": composition, "layer": render_and_lookup}, args.brackets)
            say(f"{args.size:>9s} F={F:<3d} tex {S}^2 forward: k_tx_forward {fmt(t['lookup'])}  k_rs_shade<3> {fmt(t['shade'])}; lookup / shade = "
                f"{t['lookup'][0] / t['shade'][0]:.3f}; floor {floor * 1e3:.3f} ms (40 bytes per pixel at {STREAM_TBPS} TB/s): lookup = "
                f"{t['lookup'][0] / floor:.2f} x floor, shade = {t['shade'][0] / floor:.2f} x")
            say(f"{'':>9s}       with the render: render_texture (no grad) {fmt(t['layer'])}  render_attributes(uv) + grid_sample {fmt(t['composition'])}; "
                f"render_texture / composition = {t['layer'][0] / t['composition'][0]:.3f}")
            row.update(lookup_ms=t["lookup"][0] * 1e3, shade_ms=t["shade"][0] * 1e3, floor_ms=floor * 1e3, layer_forward_ms=t["layer"][0] * 1e3,
                       composition_forward_ms=t["composition"][0] * 1e3)

            def grad(g, want_uv):
                gu = image.data_ptr() if want_uv else None              # (image's first two thirds serve as the [F, H, W, 2] output)
                raster.texture_grad_device(face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, uv.data_ptr(), T, uvf.data_ptr(),
                                           tex.data_ptr(), 1, Cn, S, S, 0, F, g.data_ptr(), gu, grad_tex.data_ptr(), work.data_ptr(), stream)

            texl = tex.clone().requires_grad_()
            with torch.no_grad():
                grid = tl.render_attributes(verts, faces, intr, (H, W), uv_vertex)[0] * 2 - 1
            Gp = G.permute(0, 3, 1, 2)

            def grid_backward():
                texl.grad = None
                out = torch.nn.functional.grid_sample(texl.permute(2, 0, 1)[None].expand(F, -1, -1, -1), grid, mode="bilinear",
                                                      padding_mode="border", align_corners=False)
                out.backward(Gp)

            def grid_forward():
                with torch.no_grad():
                    torch.nn.functional.grid_sample(texl.permute(2, 0, 1)[None].expand(F, -1, -1, -1), grid, mode="bilinear",
                                                    padding_mode="border", align_corners=False)

            t = alternate(torch, {"full": lambda: grad(G, False), "zero": lambda: grad(G0, False), "both": lambda: grad(G, True),
                                  "grid_fb": grid_backward, "grid_f": grid_forward}, args.brackets)
            acc = max(t["full"][0] - t["zero"][0], 1e-9)
            adds = 4.0 * Cn * Nc
            say(f"{args.size:>9s} F={F:<3d} tex {S}^2 gradient in the texels: the entry {fmt(t['full'])}  with G = 0 (max pass, clears, fold, an empty "
                f"adding pass) {fmt(t['zero'])}; accumulate = the difference {acc * 1e3:.3f} ms: {adds / acc / 1e9:.2f} G integer adds/s "
                f"({adds:.3g} adds into {S * S * Cn} elements); with d_grad_uv too {fmt(t['both'])}")
            say(f"{'':>9s}       grid_sample forward + backward into the texture {fmt(t['grid_fb'])}  forward alone {fmt(t['grid_f'])}: its backward "
                f"{(t['grid_fb'][0] - t['grid_f'][0]) * 1e3:.3f} ms; the entry / grid_sample's backward = "
                f"{t['full'][0] / max(t['grid_fb'][0] - t['grid_f'][0], 1e-9):.3f}")
            row.update(grad_full_ms=t["full"][0] * 1e3, grad_zero_ms=t["zero"][0] * 1e3, grad_both_ms=t["both"][0] * 1e3, accumulate_ms=acc * 1e3,
                       integer_adds_per_s=adds / acc, grid_backward_ms=(t["grid_fb"][0] - t["grid_f"][0]) * 1e3)
            del grid, Gp, texl
            if args.variant_lib:
                here, other = RawRaster2(api.load_library(), V, faces, W, H), RawRaster2(C.CDLL(os.path.abspath(args.variant_lib)), V, faces, W, H)
                gt2 = torch.empty_like(grad_tex)
                t = alternate(torch, {"here": lambda: here.texture_grad(face, bary, verts, 3 * V, uv, uvf, Cn, S, F, G, grad_tex, work, stream),
                                      "other": lambda: other.texture_grad(face, bary, verts, 3 * V, uv, uvf, Cn, S, F, G, gt2, work, stream)}, args.brackets)
                same = bool(torch.equal(grad_tex.view(torch.int32), gt2.view(torch.int32)))
                say(f"{'':>9s}       the entry of this build {fmt(t['here'])}  of the variant build {fmt(t['other'])}; this / variant = "
                    f"{t['here'][0] / t['other'][0]:.3f}; gradients bit-identical: {same}")
                row.update(grad_here_ms=t["here"][0] * 1e3, grad_variant_ms=t["other"][0] * 1e3, grad_variant_identical=same)
                here.close(); other.close()
                del gt2

            # ---- the layer and the term
            leaf = verts.clone().requires_grad_()
            uvl = uv.clone().requires_grad_()
            texl = tex.clone().requires_grad_()

            def layer(full):
                leaf.grad = uvl.grad = texl.grad = None
                img, _ = tl.render_texture(leaf if full else verts, faces, intr, (H, W), uvl if full else uv, uvf_h, texl, interior=full)
                img.backward(G)

            with torch.no_grad():
                video = tl.antialias(tl.render_texture(verts, faces, intr, (H, W), uv, uvf_h, tex)[0], verts, faces, intr)
            shifted = verts.clone()
            shifted[..., 0] += 0.4 * shifted[..., 2] / intr[0]
            leaf2 = shifted.requires_grad_()
            term = tl.TexturedPhotometricTerm(video, intr, faces, uv, uvf_h, trunc=0.5)

            def run_term():
                leaf2.grad = texl.grad = None
                term(leaf2, texl).backward()

            t = alternate(torch, {"tex": lambda: layer(False), "all": lambda: layer(True), "term": run_term}, args.brackets)
            say(f"{args.size:>9s} F={F:<3d} tex {S}^2 forward + backward: render_texture in tex {fmt(t['tex'])}  in tex, uv and verts (interior=True) "
                f"{fmt(t['all'])}  TexturedPhotometricTerm in tex and verts {fmt(t['term'])}")
            row.update(layer_tex_ms=t["tex"][0] * 1e3, layer_all_ms=t["all"][0] * 1e3, term_ms=t["term"][0] * 1e3)
            out_rows.append(row)
            del leaf, uvl, texl, video, shifted, leaf2, term, tex, grad_tex, work
            torch.cuda.empty_cache()
        del G0

        # ---- the kernels this change touched the sources of, against another build's, alternating
        if args.parent_lib:
            libs = {"new": RawRaster2(api.load_library(), V, faces, W, H), "parent": RawRaster2(C.CDLL(os.path.abspath(args.parent_lib)), V, faces, W, H)}
            video = torch.rand((F, H, W, Cn), device="cuda")
            N = pixels
            outs = {}
            for name in libs:
                outs[name] = dict(depth=torch.empty_like(depth), face=torch.empty_like(face), bary=torch.empty_like(bary), image=torch.empty_like(image),
                                  weight=torch.empty_like(weight), value=torch.empty((F, V, Cn), device="cuda"),
                                  valid=torch.empty((F, V), dtype=torch.uint8, device="cuda"), grad=torch.empty((F, V, Cn, 2), device="cuda"),
                                  index=torch.empty(N, dtype=torch.int32, device="cuda"), beta=torch.empty((N, 3), device="cuda"),
                                  dir=torch.empty((N, 3), device="cuda"))
            calls = {
                "render": lambda r, o: r.render(verts, 3 * V, F, intr, o["depth"], o["face"], o["bary"], stream),
                "shade": lambda r, o: r.shade(o["face"], o["bary"], verts, 3 * V, colours, Cn, F, o["image"], o["weight"], stream),
                "sample": lambda r, o: r.sample(verts, 3 * V, V, F, intr, video, Cn, o["value"], o["valid"], o["grad"], stream),
                "interp_rows": lambda r, o: r.interp(verts, 3 * V, F, intr, o["face"], N, colours, Cn, G, o["index"], o["beta"], o["dir"], stream),
            }
            keys = dict(render=("depth", "face", "bary"), shade=("image", "weight"), sample=("value", "valid", "grad"), interp_rows=("index", "beta", "dir"))
            row = dict(frames=F, parent=True)
            for k, call in calls.items():
                t = alternate(torch, {"parent": lambda: call(libs["parent"], outs["parent"]), "new": lambda: call(libs["new"], outs["new"]),
                                      "parent_again": lambda: call(libs["parent"], outs["parent"])}, max(args.brackets, 7))
                same = all(bool(torch.equal(outs["new"][q].view(torch.int32) if outs["new"][q].dtype != torch.uint8 else outs["new"][q],
                                            outs["parent"][q].view(torch.int32) if outs["parent"][q].dtype != torch.uint8 else outs["parent"][q]))
                           for q in keys[k])
                say(f"{args.size:>9s} F={F:<3d} {k}: this build {fmt(t['new'])}  the parent's {fmt(t['parent'])}  the parent's again {fmt(t['parent_again'])}; "
                    f"this / parent = {t['new'][0] / t['parent'][0]:.4f}, parent again / parent (the margin) = {t['parent_again'][0] / t['parent'][0]:.4f}; "
                    f"outputs bit-identical: {same}")
                row.update({f"{k}_new_ms": t["new"][0] * 1e3, f"{k}_parent_ms": t["parent"][0] * 1e3, f"{k}_parent_again_ms": t["parent_again"][0] * 1e3,
                            f"{k}_identical": same})
            out_rows.append(row)
            for r in libs.values():
                r.close()
            del outs, video
        del depth, face, bary, image, weight, G, verts
        torch.cuda.empty_cache()
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
