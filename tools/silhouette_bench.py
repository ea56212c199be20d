"""Times of the exact distance transform (bodyfit_raster_distance_device, k_edt.hip) and of torch_layer.SilhouetteTerm at SMPL's
size, 6890 vertices / 13,776 faces of synth.make_faces, for 640 x 480 and 1920 x 1080 images and 32 and 256 frames of one posed
synthetic sequence.  The transformed image is the rendered face-id image of the sequence (seed kind 1), which is what the term
transforms once per evaluation; the term's mask is the render of the same frames scaled by 1.05 about their centroid and shifted
by (4, -2, 0) cm.  Protocol of tools/raster_bench.py: each time is the median of --brackets brackets of back-to-back calls
after a warm-up, on the host clock around work that ends in a device synchronise; the spread is the brackets' min .. max.
Beside the transform, from the same process, sizes and frame counts:
  fill       a plain fill of its two outputs (dist2, nearest: F H W 8 bytes), its write floor;
  render     bodyfit_raster_render_device with the weights, which the term runs once per evaluation as well;
  term       SilhouetteTerm forward (evaluate) and backward, timed separately with a synchronise in between; "rows" is the
             forward less the render and the transform timed above (the visibility kernel and the torch operations that build
             the rows); the backward is the rows VJP (bodyfit_surface_rows_vjp_device, its grouping by face included) plus the
             elementwise torch backward of the model -> data half.
--term-only N: nothing is timed; per size and frame count one warm-up and N forward + backward evaluations of the term, for a run
of its own under rocprofv3 --kernel-trace --stats (which kernels the term's time goes to).
Usage: python3 tools/silhouette_bench.py [--sizes 640x480 1920x1080] [--frames 32 256] [--brackets 5] [--term-only N] [--out profiles/silhouette_bench.txt]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.raster_bench import brackets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["640x480", "1920x1080"])
    ap.add_argument("--frames", nargs="*", type=int, default=[32, 256])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--term-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    if api.device_count() < 1:
        raise SystemExit("silhouette_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    Fmax = max(args.frames)
    seq = synth.make_sequence(model, Fmax, seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    centre = cloud.astype(np.float64).mean(axis=1, keepdims=True)
    target = ((cloud - centre) * 1.05 + centre + np.array([0.04, -0.02, 0.0])).astype(np.float32)
    V = model.n_verts
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# silhouette_bench: V={V} n_faces={len(faces)} brackets={args.brackets}; times in ms per call: median [min .. max] x calls per bracket"]
    rows = []
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    for size in args.sizes:
        W, H = (int(a) for a in size.split("x"))
        intr = synth.camera_intrinsics(W, H)
        handle = api.Raster(0, V, faces, W, H)
        for F in args.frames:
            verts = torch.tensor(cloud[:F], device="cuda")
            depth = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
            face = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
            bary = torch.empty((F, H, W, 3), dtype=torch.float32, device="cuda")
            dist2 = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
            nearest = torch.empty((F, H, W), dtype=torch.int32, device="cuda")

            def fill():
                dist2.fill_(0); nearest.fill_(-1)

            def render():
                handle.render_device(verts.data_ptr(), 3 * V, F, intr, depth.data_ptr(), face.data_ptr(), bary.data_ptr(),
                                     z_near=0.1, stream=stream)

            def transform():
                handle.distance_device(face.data_ptr(), 1, H * W, F, False, dist2.data_ptr(), nearest.data_ptr(), stream)

            if args.term_only:
                mask = tl.render_depth(torch.tensor(target[:F], device="cuda"), faces, intr, (H, W))[1] >= 0
                term = tl.SilhouetteTerm(mask, intr, faces, trunc=0.05 * H)
                v = verts.clone().requires_grad_(True)
                for _ in range(1 + args.term_only):
                    v.grad = None
                    term(v).backward()
                torch.cuda.synchronize()
                print(f"{size} F={F}: {args.term_only} evaluations of the term after one warm-up, nothing timed", flush=True)
                continue
            t_fill = brackets(torch, fill, args.brackets)
            t_render = brackets(torch, render, args.brackets)
            t_edt = brackets(torch, transform, args.brackets)
            covered = float((face >= 0).float().mean())
            far = float(dist2.double().sqrt().max())
            del depth, bary, dist2, nearest
            mask = tl.render_depth(torch.tensor(target[:F], device="cuda"), faces, intr, (H, W))[1] >= 0
            del face
            term = tl.SilhouetteTerm(mask, intr, faces, trunc=0.05 * H)
            v = verts.clone().requires_grad_(True)
            fwd, bwd, n_rows = [], [], 0
            for rep in range(2 + args.brackets):
                v.grad = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev = term.evaluate(v)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ev["cost"].backward()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep >= 2:
                    fwd.append(t1 - t0); bwd.append(t2 - t1)
                n_rows = int(ev["row_index"].shape[0])
                n_vis = int(ev["visible"].sum())
                del ev
            t_fwd = (float(np.median(fwd)), min(fwd), max(fwd), 1)
            t_bwd = (float(np.median(bwd)), min(bwd), max(bwd), 1)
            pixels = F * H * W
            row = dict(size=size, frames=F, transform_ms=t_edt[0] * 1e3, fill_ms=t_fill[0] * 1e3, render_ms=t_render[0] * 1e3,
                       term_forward_ms=t_fwd[0] * 1e3, term_backward_ms=t_bwd[0] * 1e3,
                       term_rows_ms=(t_fwd[0] - t_render[0] - t_edt[0]) * 1e3, rows=n_rows, visible_vertices=n_vis,
                       covered=covered, farthest_px=far, transform_ns_per_pixel=t_edt[0] * 1e9 / pixels,
                       transform_gb_per_s=pixels * 12 / t_edt[0] / 1e9)
            rows.append(row)
            lines.append(f"{size:>9s} F={F:<3d}: transform {fmt(t_edt)}  fill {fmt(t_fill)}  render {fmt(t_render)}  "
                         f"term forward {fmt(t_fwd)} (rows {row['term_rows_ms']:9.3f}) backward {fmt(t_bwd)}  "
                         f"rows {n_rows:8d} visible vertices {n_vis:8d}  covered {covered:6.2%}  farthest pixel {far:7.1f} px  "
                         f"transform {row['transform_ns_per_pixel']:6.3f} ns/pixel, {row['transform_gb_per_s']:7.1f} GB/s of its 12 "
                         f"compulsory bytes a pixel")
            print(lines[-1], flush=True)
            del term, mask, v, verts
            torch.cuda.empty_cache()
        handle.close()
    if args.term_only:
        return
    lines.append("# json: " + json.dumps(rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
