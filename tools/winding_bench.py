"""Times of the mesh winding number (bodyfit_surface_winding_device, k_winding.hip), of the vertex normals and of
torch_layer.SelfPenetrationTerm at SMPL's size: a closed UV sphere of 84 segments x 83 rings, 6,890 vertices / 13,776 faces
(tests/winding_ref.py builds it), every frame scaled and moved on its own.  Protocol of tools/raster_bench.py: each time is the
median of --brackets brackets of back-to-back calls after a warm-up, on the host clock around work that ends in a device
synchronise; the spread is the brackets' min .. max.  Cases:
  vertex winding   torch_layer.vertex_winding of --frames frames (F x 6,890 x 13,776 pairs, skip ids on);
  free points      winding_number of --points points per frame, --point-frames frames, no skip ids;
  normals          vertex_normals of the same frames;
  term             SelfPenetrationTerm forward + backward on two overlapping copies of the sphere (the second scaled by 0.7 and moved
                   by 1.2 radii: 13,780 vertices, 27,552 faces), --term-frames frames.
Beside them, from the same process on the same device:
  torch            a chunked f32 torch evaluation of the same formula (atan2 of torch, [chunk, n_faces] temporaries), at the frame
                   counts up to --torch-frames (it is slow; its pairs per second do not change with more frames);
  search           closest_surface (no gradient) with the same queries against the same mesh: the same pair count through
                   k_cs_search, which culls most pairs where the winding sum must visit every one.
Usage: python3 tools/winding_bench.py [--frames 1 32 256] [--points 20000] [--point-frames 256] [--term-frames 1 32]
       [--torch-frames 32] [--brackets 5] [--out profiles/winding_bench.txt]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.raster_bench import brackets  # noqa: E402


def torch_winding(torch, points, verts, faces, skip=None, chunk=2048):
    """w [F, n] f32 of points [F, n, 3] about verts [F, V, 3]: the formula of include/bodyfit.h in f32 torch operations"""
    F, n = points.shape[0], points.shape[1]
    out = torch.empty((F, n), dtype=torch.float32, device=points.device)
    f0, f1, f2 = faces[:, 0], faces[:, 1], faces[:, 2]
    for f in range(F):
        v0, v1, v2 = verts[f, f0][None], verts[f, f1][None], verts[f, f2][None]
        for s in range(0, n, chunk):
            p = points[f, s:s + chunk, None, :]
            a, b, c = v0 - p, v1 - p, v2 - p
            la, lb, lc = a.norm(dim=2), b.norm(dim=2), c.norm(dim=2)
            num = (a * torch.linalg.cross(b, c)).sum(dim=2)
            den = la * lb * lc + (a * b).sum(dim=2) * lc + (b * c).sum(dim=2) * la + (c * a).sum(dim=2) * lb
            th = torch.atan2(num, den)
            if skip is not None:
                sk = skip[s:s + chunk, None]
                th = torch.where((f0[None] == sk) | (f1[None] == sk) | (f2[None] == sk), torch.zeros_like(th), th)
            out[f, s:s + chunk] = th.sum(dim=1) / (2.0 * np.pi)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="*", type=int, default=[1, 32, 256])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--point-frames", type=int, default=256)
    ap.add_argument("--term-frames", nargs="*", type=int, default=[1, 32])
    ap.add_argument("--torch-frames", type=int, default=32)
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    wr = importlib.import_module("winding_ref")
    if api.device_count() < 1:
        raise SystemExit("winding_bench needs a GPU: nothing here can be timed on the CPU")
    sphere, faces = wr.uv_sphere(84, 83)
    V, nf = len(sphere), len(faces)
    rng = np.random.default_rng(0)
    Fmax = max(args.frames + [args.point_frames] + args.term_frames)
    scale = rng.uniform(0.8, 1.2, (Fmax, 1, 1)).astype(np.float32)
    move = rng.normal(size=(Fmax, 1, 3)).astype(np.float32)
    cloud = sphere[None] * scale + move
    handle = api.Surface(0, V, faces)
    faces_t = torch.tensor(faces.astype(np.int64), device="cuda")
    ids_t = torch.arange(V, device="cuda")
    lines = [f"# winding_bench: V={V} n_faces={nf} brackets={args.brackets}; times in ms per call: median [min .. max] x calls per bracket"]
    rows = []
    fmt = lambda t: f"{t[0] * 1e3:10.3f} [{t[1] * 1e3:10.3f} .. {t[2] * 1e3:10.3f}] x{t[3]:<3d}"

    def report(case, F, pairs, t, **extra):
        rows.append(dict(case=case, frames=F, pairs=pairs, ms=t[0] * 1e3, ms_min=t[1] * 1e3, ms_max=t[2] * 1e3, **extra))
        rate = f"  {pairs / t[0] * 1e-9:8.1f} G pairs/s" if pairs else ""
        lines.append(f"{case:<34s} F={F:<4d} {fmt(t)}{rate}")
        print(lines[-1], flush=True)

    for F in args.frames:
        verts = torch.tensor(cloud[:F], device="cuda")
        pairs = F * V * nf
        w = tl.vertex_winding(verts, handle)
        assert bool(((w > 0.4) & (w < 0.6)).all()), "the vertices of a sphere see half of it"
        report("vertex winding", F, pairs, brackets(torch, lambda: tl.vertex_winding(verts, handle), args.brackets))
        report("closest_surface, same queries", F, pairs,
               brackets(torch, lambda: tl.closest_surface(verts, verts, handle), args.brackets))
        report("vertex normals", F, 0, brackets(torch, lambda: tl.vertex_normals(verts, handle), args.brackets))
        if F <= args.torch_frames:
            wt = torch_winding(torch, verts, verts, faces_t, ids_t)
            worst = float((wt - w).abs().max())
            report("torch f32, same formula", F, pairs,
                   brackets(torch, lambda: torch_winding(torch, verts, verts, faces_t, ids_t), min(args.brackets, 3), max_reps=3),
                   max_abs_difference=worst)
    if args.points > 0 and args.point_frames > 0:
        F, n = args.point_frames, args.points
        verts = torch.tensor(cloud[:F], device="cuda")
        pts = torch.tensor((rng.normal(size=(F, n, 3)) * 0.8).astype(np.float32) * scale[:F] + move[:F], device="cuda")
        w = tl.winding_number(pts, verts, handle)
        inside = float((w > 0.5).float().mean())
        report(f"free points, {n} per frame", F, F * n * nf, brackets(torch, lambda: tl.winding_number(pts, verts, handle), args.brackets),
               share_inside=inside)
        report("closest_surface, same queries", F, F * n * nf,
               brackets(torch, lambda: tl.closest_surface(pts, verts, handle), args.brackets))
    # the whole term on two overlapping copies of the sphere
    two = np.concatenate([sphere, sphere * np.float32(0.7) + np.array([1.2, 0, 0], np.float32)])
    faces2 = np.concatenate([faces, faces + V]).astype(np.int32)
    term = tl.SelfPenetrationTerm(faces2)
    for F in args.term_frames:
        verts = torch.tensor(np.concatenate([two[None] * scale[:F] + move[:F]]), device="cuda", requires_grad=True)

        def step():
            verts.grad = None
            term(verts).backward()

        e = term.evaluate(verts)
        report("term forward + backward, two copies", F, F * len(two) * len(faces2), brackets(torch, step, args.brackets),
               enclosed_per_frame=int(e["rows"].numel()) // F, vertices=len(two), faces=len(faces2))
        report("  of which vertex winding", F, F * len(two) * len(faces2),
               brackets(torch, lambda: tl.vertex_winding(verts, term._handle_for(verts)), args.brackets))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
        f.write("# " + json.dumps(rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
