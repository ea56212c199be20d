"""Times of the texture lookup with mipmaps (bodyfit_raster_texture_mip_build_device, bodyfit_raster_texture_mip_device,
bodyfit_raster_texture_mip_grad_device: k_txm_build, k_txm_forward, k_tx_gmax, k_txm_grad, k_txm_fold) beside the plain entries on
the same render, at the shapes of tools/texture_bench.py: SMPL's 6890 vertices / 13,776 faces with the "cylinder" atlas, 1920 x
1080, C = 3, f32 textures of 256^2 and 1024^2 shared by 32 and 256 frames of one posed synthetic sequence.  The protocol is
tools/interp_bench.py's `alternate` (medians of brackets that take turns):
  build      the pyramid of one texture;
  forward    k_txm_forward beside k_tx_forward, with the bytes a pixel streams over 6.3 TB/s as the floor: face 4 + bary 12 + image
             12 + weight 12 = 40 (the shade's) + 24 of uv + 24 of the corners' x, y + 8 C texel bytes = 112 per COVERED pixel for
             the mip lookup, 40 per pixel otherwise;
  gradient   the mip entry (d_grad_tex alone, and with d_grad_uv) beside the plain entry; with --variant-lib (this library built
             with the other value of BODYFIT_TXM_COMBINE) both builds alternate and the gradients are compared bit for bit;
  layer      torch_layer.texture.render_texture_mip forward + backward in tex, and in tex, uv and verts, beside render_texture;
  reach      the share of the level-0 texels of the shared texture that receive a non-zero gradient (G = 1) from ONE frame and
             from all of them, with and without mipmaps;
  parent     with --parent-lib (the parent commit's libbodyfit.so): k_tx_forward, the plain gradient entry, k_rs_shade<3> and
             k_rs_interp_rows<3> of this build against the other's, alternating, outputs compared bit for bit; the other build
             is timed twice in the same alternation: the margin; then the two builds once more with their output and workspace
             buffers SWAPPED, which tells a difference of the builds from a difference of where their buffers lie.
Nothing is asserted; every comparison is printed whichever way it falls.
Usage: python3 tools/texture_mip_bench.py [--size 1920x1080] [--frames 32 256] [--textures 256 1024] [--brackets 5]
                                           [--parent-lib PATH] [--variant-lib PATH] [--out profiles/texture_mip_bench.txt]"""
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

from interp_bench import STREAM_TBPS, alternate  # noqa: E402
from texture_bench import RawRaster2  # noqa: E402


class RawRaster3(RawRaster2):
    """RawRaster2 with the plain lookup and the mip gradient entry, by ctypes alone: the same calls for two builds"""

    def __init__(self, lib, n_verts, faces, W, H):
        super().__init__(lib, n_verts, faces, W, H)
        vp, ll, i, d, fl = C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_float
        lib.bodyfit_raster_texture_device.argtypes = [vp, vp, vp, vp, ll, vp, i, vp, vp, i, i, i, i, ll, i, C.POINTER(fl), vp, vp, vp, vp]
        if hasattr(lib, "bodyfit_raster_texture_mip_grad_device"):
            lib.bodyfit_raster_texture_mip_grad_device.argtypes = [vp, vp, vp, vp, ll, vp, i, vp, vp, i, i, i, i, ll, i, d, d, d, d, vp, ll,
                                                                   i, fl, vp, vp, vp, vp, vp]

    def texture(self, face, bary, verts, stride, uv, uvf, tex, Cn, S, F, image, weight, stream):
        self.check(self.lib.bodyfit_raster_texture_device(self.h, face.data_ptr(), bary.data_ptr(), verts.data_ptr(), stride, uv.data_ptr(),
                                                          uv.shape[0], uvf.data_ptr(), tex.data_ptr(), 1, Cn, S, S, 0, F, None,
                                                          image.data_ptr(), weight.data_ptr(), None, stream))

    def mip_grad(self, face, bary, verts, stride, uv, uvf, Cn, S, F, intr, G, grad_tex, work, stream):
        self.check(self.lib.bodyfit_raster_texture_mip_grad_device(self.h, face.data_ptr(), bary.data_ptr(), verts.data_ptr(), stride,
                                                                   uv.data_ptr(), uv.shape[0], uvf.data_ptr(), None, 1, Cn, S, S, 0, F, *intr,
                                                                   None, 0, -1, 0.0, G.data_ptr(), None, grad_tex.data_ptr(),
                                                                   work.data_ptr(), stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", nargs="*", type=int, default=[32, 256])
    ap.add_argument("--textures", nargs="*", type=int, default=[256, 1024])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_mip_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    if api.device_count() < 1:
        raise SystemExit("texture_mip_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    seq = synth.make_sequence(model, max(args.frames), seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    V, Cn = model.n_verts, 3
    W, H = (int(a) for a in args.size.split("x"))
    intr = tuple(float(a) for a in synth.camera_intrinsics(W, H))
    stream = torch.cuda.current_stream().cuda_stream
    uv_h, uvf_h = synth.make_uv_atlas(faces, "cylinder", verts=model.v_template)
    uv, uvf = torch.tensor(uv_h, device="cuda"), torch.tensor(uvf_h, device="cuda")
    T = len(uv_h)
    colours = torch.rand((V, Cn), device="cuda")
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# texture_mip_bench: V={V} n_faces={len(faces)} uv rows={T} size={args.size} C={Cn} brackets={args.brackets}; times in ms "
             f"per call: median [min .. max] x calls per bracket; alternatives alternate bracket by bracket"]
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
        lod = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
        G = torch.randn((F, H, W, Cn), device="cuda")
        G1 = torch.ones((F, H, W, Cn), device="cuda")
        for S in args.textures:
            row = dict(frames=F, texture=S, covered=Nc / pixels, pixels=pixels)
            tex = torch.rand((S, S, Cn), device="cuda")
            n_levels, _, _, total = api.texture_mip_layout(S, S)
            pyramid = torch.empty((total * Cn,), dtype=torch.float32, device="cuda")
            grad_tex = torch.empty((S, S, Cn), dtype=torch.float32, device="cuda")
            grad_plain = torch.empty((S, S, Cn), dtype=torch.float32, device="cuda")
            work = torch.empty(((S * S + total) * Cn,), dtype=torch.int64, device="cuda")
            common = (face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, uv.data_ptr(), T, uvf.data_ptr())

            def build():
                raster.texture_mip_build_device(tex.data_ptr(), 1, Cn, S, S, 0, 1, -1, pyramid.data_ptr(), 0, stream)

            def plain():
                raster.texture_device(*common, tex.data_ptr(), 1, Cn, S, S, 0, F, 0.0, image.data_ptr(), weight.data_ptr(), None, stream)

            def mip():
                raster.texture_mip_device(*common, tex.data_ptr(), 1, Cn, S, S, 0, F, intr, pyramid.data_ptr(), 0, -1, 0.0, 0.0,
                                          image.data_ptr(), weight.data_ptr(), None, None, stream)

            build()
            raster.texture_mip_device(*common, tex.data_ptr(), 1, Cn, S, S, 0, F, intr, pyramid.data_ptr(), 0, -1, 0.0, 0.0, image.data_ptr(),
                                      weight.data_ptr(), None, lod.data_ptr(), stream)
            live = (weight != 0).any(dim=-1)
            hist = torch.bincount(lod[live].floor().long(), minlength=n_levels).tolist()
            t = alternate(torch, {"build": build, "plain": plain, "mip": mip}, args.brackets)
            floor_plain = 40.0 * pixels / (STREAM_TBPS * 1e12)
            floor_mip = (40.0 * pixels + (48.0 + 8.0 * Cn) * Nc) / (STREAM_TBPS * 1e12)
            say(f"{args.size:>9s} F={F:<3d} tex {S}^2 ({n_levels} levels; covered pixels per l0: {hist}): build {fmt(t['build'])}")
            say(f"{'':>9s}       forward: k_txm_forward {fmt(t['mip'])}  k_tx_forward {fmt(t['plain'])}; mip / plain = {t['mip'][0] / t['plain'][0]:.3f}; "
                f"floors {floor_mip * 1e3:.3f} and {floor_plain * 1e3:.3f} ms: mip = {t['mip'][0] / floor_mip:.2f} x floor, plain = "
                f"{t['plain'][0] / floor_plain:.2f} x")
            row.update(n_levels=n_levels, l0_hist=hist, build_ms=t["build"][0] * 1e3, mip_ms=t["mip"][0] * 1e3, plain_ms=t["plain"][0] * 1e3,
                       floor_mip_ms=floor_mip * 1e3, floor_plain_ms=floor_plain * 1e3)

            def grad_mip(g, want_uv, n=F):
                raster.texture_mip_grad_device(*common, tex.data_ptr(), 1, Cn, S, S, 0, n, intr, pyramid.data_ptr(), 0, -1, 0.0, g.data_ptr(),
                                               image.data_ptr() if want_uv else None, grad_tex.data_ptr(), work.data_ptr(), stream)

            def grad_plain_(g, want_uv, n=F):
                raster.texture_grad_device(*common, tex.data_ptr(), 1, Cn, S, S, 0, n, g.data_ptr(), image.data_ptr() if want_uv else None,
                                           grad_plain.data_ptr(), work.data_ptr(), stream)

            t = alternate(torch, {"mip": lambda: grad_mip(G, False), "plain": lambda: grad_plain_(G, False), "mip_uv": lambda: grad_mip(G, True),
                                  "plain_uv": lambda: grad_plain_(G, True)}, args.brackets)
            say(f"{'':>9s}       gradient in the texels: the mip entry {fmt(t['mip'])}  the plain entry {fmt(t['plain'])}; mip / plain = "
                f"{t['mip'][0] / t['plain'][0]:.3f}; with d_grad_uv too: {fmt(t['mip_uv'])} and {fmt(t['plain_uv'])}")
            row.update(grad_mip_ms=t["mip"][0] * 1e3, grad_plain_ms=t["plain"][0] * 1e3, grad_mip_uv_ms=t["mip_uv"][0] * 1e3,
                       grad_plain_uv_ms=t["plain_uv"][0] * 1e3)
            reach = {}
            for n in (1, F):
                grad_mip(G1, False, n)
                grad_plain_(G1, False, n)
                torch.cuda.synchronize()
                reach[n] = (float((grad_tex != 0).any(dim=-1).float().mean()), float((grad_plain != 0).any(dim=-1).float().mean()))
            say(f"{'':>9s}       level-0 texels with a non-zero gradient (G = 1): one frame: mip {reach[1][0]:.4f}, plain {reach[1][1]:.4f} of the "
                f"texture; {F} frames: mip {reach[F][0]:.4f}, plain {reach[F][1]:.4f}")
            row.update(reach_one_mip=reach[1][0], reach_one_plain=reach[1][1], reach_all_mip=reach[F][0], reach_all_plain=reach[F][1])
            if args.variant_lib:
                here, other = RawRaster3(api.load_library(), V, faces, W, H), RawRaster3(C.CDLL(os.path.abspath(args.variant_lib)), V, faces, W, H)
                gt2 = torch.empty_like(grad_tex)
                t = alternate(torch, {"here": lambda: here.mip_grad(face, bary, verts, 3 * V, uv, uvf, Cn, S, F, intr, G, grad_tex, work, stream),
                                      "other": lambda: other.mip_grad(face, bary, verts, 3 * V, uv, uvf, Cn, S, F, intr, G, gt2, work, stream)},
                              args.brackets)
                same = bool(torch.equal(grad_tex.view(torch.int32), gt2.view(torch.int32)))
                say(f"{'':>9s}       the mip entry of this build {fmt(t['here'])}  of the variant build (the other BODYFIT_TXM_COMBINE) {fmt(t['other'])}; "
                    f"this / variant = {t['here'][0] / t['other'][0]:.3f}; gradients bit-identical: {same}")
                row.update(grad_here_ms=t["here"][0] * 1e3, grad_variant_ms=t["other"][0] * 1e3, grad_variant_identical=same)
                here.close(); other.close()
                del gt2

            leaf = verts.clone().requires_grad_()
            uvl = uv.clone().requires_grad_()
            texl = tex.clone().requires_grad_()

            def layer(full, use_mip):
                leaf.grad = uvl.grad = texl.grad = None
                fn = tl.texture.render_texture_mip if use_mip else tl.render_texture
                img, _ = fn(leaf if full else verts, faces, intr, (H, W), uvl if full else uv, uvf_h, texl, interior=full)
                img.backward(G)

            t = alternate(torch, {"tex_mip": lambda: layer(False, True), "tex": lambda: layer(False, False), "all_mip": lambda: layer(True, True),
                                  "all": lambda: layer(True, False)}, args.brackets)
            say(f"{'':>9s}       forward + backward in tex: render_texture_mip {fmt(t['tex_mip'])}  render_texture {fmt(t['tex'])}; in tex, uv and "
                f"verts (interior=True): render_texture_mip {fmt(t['all_mip'])}  render_texture {fmt(t['all'])}")
            row.update(layer_tex_mip_ms=t["tex_mip"][0] * 1e3, layer_tex_ms=t["tex"][0] * 1e3, layer_all_mip_ms=t["all_mip"][0] * 1e3,
                       layer_all_ms=t["all"][0] * 1e3)
            out_rows.append(row)
            del leaf, uvl, texl, tex, pyramid, grad_tex, grad_plain, work
            torch.cuda.empty_cache()

        if args.parent_lib:
            S = args.textures[0]
            tex = torch.rand((S, S, Cn), device="cuda")
            libs = {"new": RawRaster3(api.load_library(), V, faces, W, H), "parent": RawRaster3(C.CDLL(os.path.abspath(args.parent_lib)), V, faces, W, H)}
            N = pixels
            outs = {name: dict(image=torch.empty_like(image), weight=torch.empty_like(weight), gt=torch.empty((S, S, Cn), device="cuda"),
                               work=torch.empty((S, S, Cn), dtype=torch.int64, device="cuda"), index=torch.empty(N, dtype=torch.int32, device="cuda"),
                               beta=torch.empty((N, 3), device="cuda"), dir=torch.empty((N, 3), device="cuda")) for name in libs}
            calls = {
                "k_tx_forward": lambda r, o: r.texture(face, bary, verts, 3 * V, uv, uvf, tex, Cn, S, F, o["image"], o["weight"], stream),
                "k_tx_grad (the plain entry)": lambda r, o: r.texture_grad(face, bary, verts, 3 * V, uv, uvf, Cn, S, F, G, o["gt"], o["work"], stream),
                "k_rs_shade<3>": lambda r, o: r.shade(face, bary, verts, 3 * V, colours, Cn, F, o["image"], o["weight"], stream),
                "k_rs_interp_rows<3>": lambda r, o: r.interp(verts, 3 * V, F, intr, face, N, colours, Cn, G, o["index"], o["beta"], o["dir"], stream),
            }
            keys = {"k_tx_forward": ("image", "weight"), "k_tx_grad (the plain entry)": ("gt",), "k_rs_shade<3>": ("image", "weight"),
                    "k_rs_interp_rows<3>": ("index", "beta", "dir")}
            row = dict(frames=F, parent=True)
            for k, call in calls.items():
                t = alternate(torch, {"parent": lambda: call(libs["parent"], outs["parent"]), "new": lambda: call(libs["new"], outs["new"]),
                                      "parent_again": lambda: call(libs["parent"], outs["parent"])}, max(args.brackets, 7))
                same = all(bool(torch.equal(outs["new"][q].view(torch.int32), outs["parent"][q].view(torch.int32))) for q in keys[k])
                say(f"{args.size:>9s} F={F:<3d} {k}: this build {fmt(t['new'])}  the parent's {fmt(t['parent'])}  the parent's again {fmt(t['parent_again'])}; "
                    f"this / parent = {t['new'][0] / t['parent'][0]:.4f}, parent again / parent (the margin) = {t['parent_again'][0] / t['parent'][0]:.4f}; "
                    f"outputs bit-identical: {same}")
                row.update({f"{k}_new_ms": t["new"][0] * 1e3, f"{k}_parent_ms": t["parent"][0] * 1e3, f"{k}_parent_again_ms": t["parent_again"][0] * 1e3,
                            f"{k}_identical": same})
                # the same two builds with their output (and workspace) buffers SWAPPED: if the ratio follows the buffers and not the
                # build, it measures where the buffers lie
                t = alternate(torch, {"parent": lambda: call(libs["parent"], outs["new"]), "new": lambda: call(libs["new"], outs["parent"])},
                              max(args.brackets, 7))
                say(f"{'':>9s}       buffers swapped: this build {fmt(t['new'])}  the parent's {fmt(t['parent'])}; this / parent = "
                    f"{t['new'][0] / t['parent'][0]:.4f}")
                row.update({f"{k}_swapped_new_ms": t["new"][0] * 1e3, f"{k}_swapped_parent_ms": t["parent"][0] * 1e3})
            out_rows.append(row)
            for r in libs.values():
                r.close()
            del outs, tex
        del depth, face, bary, image, weight, lod, G, G1, verts
        torch.cuda.empty_cache()
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
