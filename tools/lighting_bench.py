"""Times of the lighting (bodyfit_raster_light_device, bodyfit_raster_light_grad_device: k_lt_forward, k_lt_grad, k_lt_light_sum),
of the vertex normals' adjoint (bodyfit_surface_vertex_normals_vjp_device: k_vn_h, k_vn_vjp) and of torch_layer.lighting.shade, at
the shapes of tools/texture_mip_bench.py: SMPL's 6890 vertices / 13,776 faces, 1920 x 1080, C = 3, 32 and 256 frames of one posed
synthetic sequence.  The protocol is tools/interp_bench.py's `alternate` (medians of brackets that take turns):
  forward    k_lt_forward with the bytes it streams over 6.3 TB/s as the floor: per pixel face 4 + bary 12 + albedo 12 + image 12 =
             40, per COVERED pixel 36 of normals and 12 of z more; beside k_rs_shade<3> on the same render;
  gradient   the gradient entry with each output alone and with all three; d_grad_light alone is the two reduction passes (the
             store pass without the other outputs' stores, and k_lt_light_sum);
  normals    the vertex normals' adjoint beside their forward;
  layer      lighting.shade forward + backward in albedo, light and verts (through the normals; and with interior=True) beside the
             torch composition a user would otherwise write: render_attributes of the normals, torch SH and autograd (--compose-frames,
             32 by default: at 256 frames its intermediates are tens of GB);
  parent     with --parent-lib (the parent commit's libbodyfit.so): the render, k_rs_shade<3>, k_tx_forward<3, float> and
             k_rs_interp_rows<3> of this build against the other's, alternating, outputs compared bit for bit; the other build is
             timed twice in the same alternation: the margin; then the two builds once more with their output buffers SWAPPED.
Nothing is asserted; every comparison is printed whichever way it falls.
Usage: python3 tools/lighting_bench.py [--size 1920x1080] [--frames 32 256] [--brackets 5] [--compose-frames 32]
                                        [--parent-lib PATH] [--out profiles/lighting_bench.txt]"""
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
from texture_mip_bench import RawRaster3  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", nargs="*", type=int, default=[32, 256])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--compose-frames", type=int, default=32)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lighting_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    lighting = importlib.import_module("3dbodyanimation_amd.torch_layer.lighting")
    if api.device_count() < 1:
        raise SystemExit("lighting_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    seq = synth.make_sequence(model, max(args.frames), seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    V, Cn = model.n_verts, 3
    W, H = (int(a) for a in args.size.split("x"))
    intr = tuple(float(a) for a in synth.camera_intrinsics(W, H))
    stream = torch.cuda.current_stream().cuda_stream
    colours = torch.rand((V, Cn), device="cuda")
    light = torch.tensor([[0.8] * Cn, [0.3] * Cn, [-0.2] * Cn, [-0.4] * Cn] + [[0.05] * Cn] * 5, device="cuda")
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# lighting_bench: V={V} n_faces={len(faces)} size={args.size} C={Cn} brackets={args.brackets}; times in ms per call: median "
             f"[min .. max] x calls per bracket; alternatives alternate bracket by bracket"]
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
        bary = torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
        raster.render_device(verts.data_ptr(), 3 * V, F, intr, depth.data_ptr(), face.data_ptr(), bary.data_ptr(), stream=stream)
        pixels = F * H * W
        Nc = int((face >= 0).sum())
        normals = tl.vertex_normals(verts, faces)
        albedo = torch.empty((F, H, W, Cn), dtype=torch.float32, device="cuda")
        weight = torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
        image = torch.empty((F, H, W, Cn), dtype=torch.float32, device="cuda")
        raster.shade_device(face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, colours.data_ptr(), 0, Cn, F, 0.5, albedo.data_ptr(),
                            weight.data_ptr(), stream)
        G = torch.randn((F, H, W, Cn), device="cuda")
        ga, gm = torch.empty_like(albedo), torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
        gl = torch.empty((F, 9, Cn), dtype=torch.float32, device="cuda")
        chunk, n_chunks, n_work = api.light_grad_layout(H * W, Cn, F)
        work = torch.empty(n_work, dtype=torch.float64, device="cuda")
        common = (face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, normals.data_ptr(), 3 * V, albedo.data_ptr(), Cn,
                  light.data_ptr(), 0, F)
        row = dict(frames=F, covered=Nc / pixels, pixels=pixels, chunk_pixels=chunk, n_chunks=n_chunks)

        def forward():
            raster.light_device(*common, image.data_ptr(), None, None, stream)

        def shade():
            raster.shade_device(face.data_ptr(), bary.data_ptr(), verts.data_ptr(), 3 * V, colours.data_ptr(), 0, Cn, F, 0.5, image.data_ptr(),
                                weight.data_ptr(), stream)

        t = alternate(torch, {"light": forward, "shade": shade}, args.brackets)
        floor = (40.0 * pixels + 48.0 * Nc) / (STREAM_TBPS * 1e12)
        say(f"{args.size:>9s} F={F:<3d} covered {Nc / pixels:.4f}: forward k_lt_forward {fmt(t['light'])}  k_rs_shade<3> {fmt(t['shade'])}; light / shade = "
            f"{t['light'][0] / t['shade'][0]:.3f}; floor {floor * 1e3:.3f} ms: light = {t['light'][0] / floor:.2f} x floor")
        row.update(forward_ms=t["light"][0] * 1e3, shade_ms=t["shade"][0] * 1e3, floor_ms=floor * 1e3)

        def grad(a, m, l):
            raster.light_grad_device(*common, G.data_ptr(), ga.data_ptr() if a else None, gm.data_ptr() if m else None,
                                     gl.data_ptr() if l else None, work.data_ptr() if l else None, stream)

        t = alternate(torch, {"albedo": lambda: grad(1, 0, 0), "m": lambda: grad(0, 1, 0), "light": lambda: grad(0, 0, 1),
                              "all": lambda: grad(1, 1, 1)}, args.brackets)
        floor_g = ((4 + 12 + 12 + 12 + 12 + 12) * pixels + 48.0 * Nc) / (STREAM_TBPS * 1e12)
        say(f"{'':>9s}       gradient entry ({n_chunks} chunks of {chunk} pixels per frame): d_grad_albedo alone {fmt(t['albedo'])}  d_grad_m alone "
            f"{fmt(t['m'])}  d_grad_light alone (the two reduction passes) {fmt(t['light'])}  all three {fmt(t['all'])}; floor of all three "
            f"(64 bytes per pixel + 48 per covered) {floor_g * 1e3:.3f} ms: {t['all'][0] / floor_g:.2f} x")
        row.update(grad_albedo_ms=t["albedo"][0] * 1e3, grad_m_ms=t["m"][0] * 1e3, grad_light_ms=t["light"][0] * 1e3, grad_all_ms=t["all"][0] * 1e3,
                   floor_grad_ms=floor_g * 1e3)

        gn, gv = torch.randn((F, V, 3), device="cuda"), torch.empty((F, V, 3), dtype=torch.float32, device="cuda")
        nout = torch.empty((F, V, 3), dtype=torch.float32, device="cuda")
        t = alternate(torch, {"forward": lambda: surface.vertex_normals_device(verts.data_ptr(), 3 * V, F, nout.data_ptr(), stream),
                              "vjp": lambda: surface.vertex_normals_vjp_device(verts.data_ptr(), 3 * V, F, gn.data_ptr(), gv.data_ptr(), 3 * V, stream)},
                      args.brackets)
        say(f"{'':>9s}       vertex normals: forward {fmt(t['forward'])}  adjoint (k_vn_h + k_vn_vjp) {fmt(t['vjp'])}; adjoint / forward = "
            f"{t['vjp'][0] / t['forward'][0]:.2f}")
        row.update(normals_ms=t["forward"][0] * 1e3, normals_vjp_ms=t["vjp"][0] * 1e3)

        leaf, al, ll = verts.clone().requires_grad_(), albedo.clone().requires_grad_(), light.clone().requires_grad_()
        rend = (depth, face, bary)

        def layer(interior):
            leaf.grad = al.grad = ll.grad = None
            lighting.shade(al, leaf, faces, intr, ll, render=rend, interior=interior).backward(G)

        def layer_light_only():
            ll.grad = None
            lighting.shade(albedo, verts, faces, intr, ll, normals=normals, render=rend).backward(G)

        fns = {"light": layer_light_only, "all": lambda: layer(False), "interior": lambda: layer(True)}
        faces_t = torch.tensor(faces.astype(np.int64), device="cuda")
        if F <= args.compose_frames:
            def composition():
                leaf.grad = al.grad = ll.grad = None
                # the user's own composition: normals by index_add_ (not deterministic), rendered as attributes, torch SH, autograd
                c = leaf[:, faces_t]
                N = torch.linalg.cross(c[:, :, 1] - c[:, :, 0], c[:, :, 2] - c[:, :, 0])
                s = torch.zeros_like(leaf).index_add_(1, faces_t.reshape(-1), N.repeat_interleave(3, dim=1))
                n = torch.nn.functional.normalize(s, dim=-1)
                m, fimg = tl.render_attributes(leaf, faces, intr, (H, W), n)
                lit = (fimg >= 0).unsqueeze(-1)
                sh = lighting.sh_basis(torch.nn.functional.normalize(m, dim=-1)) @ ll
                torch.where(lit, al * sh, al).backward(G)

            fns["composition"] = composition
        t = alternate(torch, fns, args.brackets)
        text = (f"{'':>9s}       lighting.shade forward + backward (render reused): in light alone {fmt(t['light'])}  in albedo, light and verts "
                f"{fmt(t['all'])}  with interior=True {fmt(t['interior'])}")
        if "composition" in t:
            text += (f"; the torch composition (index_add_ normals, render_attributes, torch SH, autograd; it renders) {fmt(t['composition'])}: "
                     f"shade / composition = {t['all'][0] / t['composition'][0]:.3f}")
            row.update(composition_ms=t["composition"][0] * 1e3)
        say(text)
        row.update(layer_light_ms=t["light"][0] * 1e3, layer_all_ms=t["all"][0] * 1e3, layer_interior_ms=t["interior"][0] * 1e3)
        out_rows.append(row)
        del leaf, al, ll, ga, gm, work
        torch.cuda.empty_cache()

        if args.parent_lib:
            S = 256
            tex = torch.rand((S, S, Cn), device="cuda")
            uv_h, uvf_h = synth.make_uv_atlas(faces, "cylinder", verts=model.v_template)
            uv, uvf = torch.tensor(uv_h, device="cuda"), torch.tensor(uvf_h, device="cuda")
            libs = {"new": RawRaster3(api.load_library(), V, faces, W, H), "parent": RawRaster3(C.CDLL(os.path.abspath(args.parent_lib)), V, faces, W, H)}
            N = pixels
            outs = {name: dict(image=torch.empty_like(image), weight=torch.empty_like(weight), depth=torch.empty_like(depth),
                               face=torch.empty_like(face), bary=torch.empty_like(bary), index=torch.empty(N, dtype=torch.int32, device="cuda"),
                               beta=torch.empty((N, 3), device="cuda"), dir=torch.empty((N, 3), device="cuda")) for name in libs}
            calls = {
                "the render": lambda r, o: r.render(verts, 3 * V, F, intr, o["depth"], o["face"], o["bary"], stream),
                "k_rs_shade<3>": lambda r, o: r.shade(face, bary, verts, 3 * V, colours, Cn, F, o["image"], o["weight"], stream),
                "k_tx_forward<3, float>": lambda r, o: r.texture(face, bary, verts, 3 * V, uv, uvf, tex, Cn, S, F, o["image"], o["weight"], stream),
                "k_rs_interp_rows<3>": lambda r, o: r.interp(verts, 3 * V, F, intr, face, N, colours, Cn, G, o["index"], o["beta"], o["dir"], stream),
            }
            keys = {"the render": ("depth", "face", "bary"), "k_rs_shade<3>": ("image", "weight"), "k_tx_forward<3, float>": ("image", "weight"),
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
                t = alternate(torch, {"parent": lambda: call(libs["parent"], outs["new"]), "new": lambda: call(libs["new"], outs["parent"])},
                              max(args.brackets, 7))
                say(f"{'':>9s}       buffers swapped: this build {fmt(t['new'])}  the parent's {fmt(t['parent'])}; this / parent = "
                    f"{t['new'][0] / t['parent'][0]:.4f}")
                row.update({f"{k}_swapped_new_ms": t["new"][0] * 1e3, f"{k}_swapped_parent_ms": t["parent"][0] * 1e3})
            out_rows.append(row)
            for r in libs.values():
                r.close()
            del outs, tex
        del depth, face, bary, image, weight, albedo, G, verts, normals
        torch.cuda.empty_cache()
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
