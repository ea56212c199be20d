"""Times of the depth render and of the visibility kernel (bodyfit_raster_render_device, bodyfit_raster_visibility_device;
k_raster.hip) at SMPL's size, 6890 vertices / 13,776 faces of synth.make_faces, for 640 x 480 and 1920 x 1080 images and 1, 32
and 256 frames of one posed synthetic sequence, at the sequence's own depth (about 3 m) and as a close-up (the clouds moved so
that their median depth is 0.9 m: large faces, many leave the image).  Each time is the median of --brackets brackets of
back-to-back calls after a warm-up, on the host clock around work that ends in a device synchronise (a render has one read-back
of its own, so its time includes that round trip); the spread is the brackets' min .. max.  Beside every render: the (face,
tile) pairs binned per 32 x 8 tile (mean over all tiles, and the longest list) and the covered share of the image.
Two yardsticks in the same process, same sizes and frame counts:
  fill     a plain fill of the three output images (depth, face, bary: F H W 20 bytes), the write floor of a render;
  overlay  bodyfit_overlay_render_device, the sibling rasteriser (painter's order into 8-bit images: anti-aliased fills and a
           sort; a comparison, not a bound).
Usage: python3 tools/raster_bench.py [--sizes 640x480 1920x1080] [--frames 1 32 256] [--brackets 5] [--out profiles/raster_bench.txt]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def brackets(torch, fn, n_brackets, min_seconds=0.15, max_reps=50):
    """(median, min, max) seconds per call of fn over n_brackets brackets, after a warm-up"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    once = max(time.perf_counter() - t0, 1e-6)
    reps = int(min(max(min_seconds / once, 1), max_reps))
    out = []
    for _ in range(n_brackets):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return float(np.median(out)), float(min(out)), float(max(out)), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["640x480", "1920x1080"])
    ap.add_argument("--frames", nargs="*", type=int, default=[1, 32, 256])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    if api.device_count() < 1:
        raise SystemExit("raster_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    Fmax = max(args.frames)
    seq = synth.make_sequence(model, Fmax, seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    V = model.n_verts
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# raster_bench: V={V} n_faces={len(faces)} brackets={args.brackets}; times in ms per call: median [min .. max] x calls per bracket"]
    rows = []
    for size in args.sizes:
        W, H = (int(a) for a in size.split("x"))
        intr = synth.camera_intrinsics(W, H)
        handle = api.Raster(0, V, faces, W, H)
        for F in args.frames:
            depth = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
            face = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
            bary = torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
            fvis = torch.empty((F, len(faces)), dtype=torch.uint8, device="cuda")
            vvis = torch.empty((F, V), dtype=torch.uint8, device="cuda")
            images = torch.zeros((F, H, W, 3), dtype=torch.uint8, device="cuda")
            overlay = api.Overlay(faces, V, W, H, max_frames=F)

            def fill():
                depth.fill_(float("inf")); face.fill_(-1); bary.zero_()

            t_fill = brackets(torch, fill, args.brackets)
            for label, z_med in (("3m", None), ("0.9m", 0.9)):
                c = cloud[:F].copy()
                if z_med is not None:
                    c[..., 2] += np.float32(z_med - np.median(c[..., 2]))
                verts = torch.tensor(c, device="cuda")

                def render():
                    handle.render_device(verts.data_ptr(), 3 * V, F, intr, depth.data_ptr(), face.data_ptr(), bary.data_ptr(),
                                         z_near=0.1, stream=stream)

                def visible():
                    handle.visibility_device(face.data_ptr(), F, fvis.data_ptr(), vvis.data_ptr(), stream)

                def draw():
                    overlay.render_device(verts.data_ptr(), False, 3 * V, F, images.data_ptr(), intr, stream=stream)

                t_render = brackets(torch, render, args.brackets)
                entries, longest = handle.last_bins()
                tiles = F * ((W + 31) // 32) * ((H + 7) // 8)
                covered = float((face >= 0).float().mean())
                t_vis = brackets(torch, visible, args.brackets)
                t_overlay = brackets(torch, draw, args.brackets)
                row = dict(size=size, frames=F, depth=label, render_ms=t_render[0] * 1e3, visibility_ms=t_vis[0] * 1e3,
                           fill_ms=t_fill[0] * 1e3, overlay_ms=t_overlay[0] * 1e3, bins_mean=entries / tiles,
                           bins_longest=longest, covered=covered, visible_faces=float(fvis.float().mean()),
                           visible_vertices=float(vvis.float().mean()))
                rows.append(row)
                fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
                lines.append(f"{size:>9s} F={F:<3d} depth {label:>4s}: render {fmt(t_render)}  visibility {fmt(t_vis)}  "
                             f"fill {fmt(t_fill)}  overlay {fmt(t_overlay)}  bins/tile mean {entries / tiles:7.2f} longest {longest:5d}  "
                             f"covered {covered:6.2%}  visible faces {row['visible_faces']:6.2%} vertices {row['visible_vertices']:6.2%}")
                print(lines[-1], flush=True)
            overlay.close()
            del depth, face, bary, images
        handle.close()
    lines.append("# json: " + json.dumps(rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
