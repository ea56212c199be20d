"""Times of the volume sampler (bodyfit_volume_sample_device, k_volume.hip) at SMPL's counts, 6890 vertices of 256 and 1024 posed
frames, on one 256^3 volume shared by the frames and on 128^3 volumes per frame, without and with the gradient output.
Timed with the protocol of tools/appearance_bench.py (a warm-up, then --brackets brackets of back-to-back calls, host clock around
work that ends in a device synchronise; median [min .. max] of the brackets); the alternatives of one comparison are ALTERNATED
bracket by bracket inside one call, so a drift of the machine falls on all of them:
  sample     k_vol_sample without and with the gradient, against
  grid       torch.nn.functional.grid_sample (5-D, trilinear, align_corners=True) forward, and forward + backward in the grid, on the
             same volume at the same (precomputed) normalised coordinates;
  copy       a plain read of the points and write of the outputs by torch (value <- one coordinate plane, valid filled; with the
             gradient: grad <- the points), and
  floor      the bytes a point needs (12 read, 5 written, 12 more with the gradient) over 6.3 TB/s, the streaming rate the machine
             sustains: the gathers of the eight voxels are not in it;
  search     closest_surface of the same vertices against a 13,776-face mesh (a posed body standing in for a scene): the search a
             lookup in a volume replaces.
Once: voxelize_sdf of that mesh at 128^3 (one search and one winding pass per voxel).
Nothing is asserted; every comparison is printed whichever way it falls.
Usage: python3 tools/volume_bench.py [--frames 256 1024] [--brackets 5] [--out profiles/volume_bench.txt]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="*", type=int, default=[256, 1024])
    ap.add_argument("--posed", type=int, default=256, help="distinct posed frames; more frames repeat them, shifted")
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    volume = importlib.import_module("3dbodyanimation_amd.torch_layer.volume")
    if api.device_count() < 1:
        raise SystemExit("volume_bench needs a GPU: nothing here can be timed on the CPU")
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    n_posed = min(args.posed, max(args.frames))
    seq = synth.make_sequence(model, n_posed, seed=3)
    prob = api.Problem.from_sequence(api.Model(model), seq, n_cols=86, use_shape=True, want_mesh=True)
    cloud = prob.writeback(seq.gt_params, seq.gt_beta, want_cloud=True)["cloud"].astype(np.float32)
    V = model.n_verts
    rng = np.random.default_rng(3)
    stream = torch.cuda.current_stream().cuda_stream
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# volume_bench: V={V} n_faces={len(faces)} brackets={args.brackets}; times in ms per call: median [min .. max] x calls "
             f"per bracket; alternatives alternate bracket by bracket"]
    out_rows = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    lo, hi = cloud.reshape(-1, 3).min(axis=0).astype(np.float64) - 0.15, cloud.reshape(-1, 3).max(axis=0).astype(np.float64) + 0.15
    scene = torch.tensor(cloud[0] + np.array([0.25, 0.0, 0.1], np.float32), device="cuda")       # the mesh of the search and of voxelize_sdf

    for F in args.frames:
        reps = -(-F // n_posed)
        host = np.concatenate([cloud + rng.uniform(-0.05, 0.05, size=3).astype(np.float32) for _ in range(reps)])[:F]
        verts = torch.tensor(host, device="cuda")
        value = torch.empty((F, V), dtype=torch.float32, device="cuda")
        valid = torch.empty((F, V), dtype=torch.uint8, device="cuda")
        grad = torch.empty((F, V, 3), dtype=torch.float32, device="cuda")
        points = F * V
        row = dict(frames=F, points=points)

        def copy(g):
            value.copy_(verts[..., 2])
            valid.fill_(1)
            if g:
                grad.copy_(verts)

        scene_f = scene[None].expand(F, V, 3).contiguous()

        def search():
            return tl.closest_surface(verts, scene_f, faces)

        for label, n, per_frame in (("256^3 shared", 256, False), ("128^3 per frame", 128, True)):
            dims = (n, n, n)
            spacing = tuple((hi - lo) / (n - 1))
            origin = tuple(lo)
            handle = api.Volume(0, dims, origin, spacing)
            shape = (F, n, n, n) if per_frame else (n, n, n)
            vol = torch.empty(shape, dtype=torch.float32, device="cuda")
            ax = [torch.linspace(0.0, 1.0, n, device="cuda") for _ in range(3)]
            base = (0.4 * ax[0][None, None, :] - 0.8 * ax[1][None, :, None] + 0.5 * ax[2][:, None, None]
                    + 0.1 * torch.sin(9.0 * ax[0])[None, None, :] * torch.cos(7.0 * ax[1])[None, :, None])
            if per_frame:
                vol.copy_(base[None].expand(shape))
                vol += torch.linspace(0.0, 0.2, F, device="cuda")[:, None, None, None]
            else:
                vol.copy_(base)
            del base

            def sample(g):
                handle.sample_device(verts.data_ptr(), 3 * V, V, F, vol.data_ptr(), n * n * n if per_frame else 0, None,
                                     value.data_ptr(), valid.data_ptr(), grad.data_ptr() if g else None, stream)

            o = torch.tensor(origin, dtype=torch.float64, device="cuda")
            s = torch.tensor(spacing, dtype=torch.float64, device="cuda")
            norm = (2.0 * ((verts.double() - o) / s) / (n - 1) - 1.0).float()
            if per_frame:
                inp, grid = vol.view(F, 1, n, n, n), norm.view(F, 1, 1, V, 3)
            else:
                inp, grid = vol.view(1, 1, n, n, n), norm.view(1, 1, 1, F * V, 3)
            grid_g = grid.clone().requires_grad_()
            up = torch.ones((grid.shape[0], 1, 1, 1, grid.shape[3]), dtype=torch.float32, device="cuda")

            def grid_sample():
                return torch.nn.functional.grid_sample(inp, grid, mode="bilinear", padding_mode="zeros", align_corners=True)

            def grid_sample_fb():
                out = torch.nn.functional.grid_sample(inp, grid_g, mode="bilinear", padding_mode="zeros", align_corners=True)
                return torch.autograd.grad(out, grid_g, up)[0]

            fns = {"sample": lambda: sample(False), "sample+g": lambda: sample(True), "grid": grid_sample, "grid f+b": grid_sample_fb,
                   "copy": lambda: copy(False), "copy+g": lambda: copy(True)}
            if not per_frame:
                fns["search"] = search
            t = alternate(torch, fns, args.brackets)
            sample(True)
            torch.cuda.synchronize()
            ok = valid.bool()
            gs = grid_sample().reshape(F, V)
            d_value = float((gs - value)[ok].abs().max()) if bool(ok.any()) else 0.0
            gg = grid_sample_fb().reshape(F, V, 3).double() * 2.0 / (n - 1) / s          # d/d(normalised) -> world units
            d_grad = float((gg - grad.double())[ok].abs().max()) if bool(ok.any()) else 0.0
            floor = points * 17 / (STREAM_TBPS * 1e12), points * 29 / (STREAM_TBPS * 1e12)
            say(f"F={F:<4d} {label:>15s} ({points} points, {int(ok.sum())} live): sample {fmt(t['sample'])}  with gradient "
                f"{fmt(t['sample+g'])}  grid_sample {fmt(t['grid'])}  grid_sample fwd+bwd {fmt(t['grid f+b'])}  copy {fmt(t['copy'])}  "
                f"copy with gradient {fmt(t['copy+g'])}" + (f"  closest_surface {fmt(t['search'])}" if "search" in t else ""))
            say(f"{'':>6s}{'':>15s} sample / grid_sample = {t['sample'][0] / t['grid'][0]:.3f}; with gradient / grid_sample fwd+bwd = "
                f"{t['sample+g'][0] / t['grid f+b'][0]:.3f}; sample / copy = {t['sample'][0] / t['copy'][0]:.2f}, with gradient "
                f"{t['sample+g'][0] / t['copy+g'][0]:.2f}; floor {floor[0] * 1e3:.4f} / {floor[1] * 1e3:.4f} ms (17 / 29 bytes per point at "
                f"{STREAM_TBPS} TB/s): sample = {t['sample'][0] / floor[0]:.1f} x floor, with gradient {t['sample+g'][0] / floor[1]:.1f} x; "
                f"{points / t['sample+g'][0] / 1e9:.2f} G points/s with gradient"
                + (f"; closest_surface / sample with gradient = {t['search'][0] / t['sample+g'][0]:.0f}" if "search" in t else "")
                + f"; |sample - grid_sample| <= {d_value:.2e}, gradient <= {d_grad:.2e} (f32 coordinates and arithmetic in grid_sample)")
            key = "shared256" if not per_frame else "perframe128"
            row[key] = dict(sample_ms=t["sample"][0] * 1e3, sample_g_ms=t["sample+g"][0] * 1e3, grid_ms=t["grid"][0] * 1e3,
                            grid_fb_ms=t["grid f+b"][0] * 1e3, copy_ms=t["copy"][0] * 1e3, copy_g_ms=t["copy+g"][0] * 1e3,
                            floor_ms=floor[0] * 1e3, floor_g_ms=floor[1] * 1e3, live=int(ok.sum()),
                            search_ms=t["search"][0] * 1e3 if "search" in t else None)
            del vol, inp, grid, grid_g, norm, gs, gg, up
            torch.cuda.empty_cache()
        out_rows.append(row)
        del verts, value, valid, grad, scene_f
        torch.cuda.empty_cache()

    # ---- voxelize_sdf of the 13,776-face mesh at 128^3, once (and a second time: the first call builds the topology's handle)
    n = 128
    spacing = tuple((hi - lo) / (n - 1))
    times = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sdf = volume.voxelize_sdf(scene, faces, tuple(lo), spacing, (n, n, n))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    say(f"voxelize_sdf at 128^3 ({n ** 3} voxels against {len(faces)} faces): first call {times[0] * 1e3:.1f} ms, second {times[1] * 1e3:.1f} ms; "
        f"{int((sdf < 0).sum())} voxels inside (w > 1/2 of an open synthetic mesh)")
    out_rows.append(dict(voxelize_first_ms=times[0] * 1e3, voxelize_second_ms=times[1] * 1e3))
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
