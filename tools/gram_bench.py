"""Time and memory of the scan normal equations (SurfaceTerm.normal_equations -> bodyfit_surface_gram_device, k_surface_gram.hip)
on F frames x N scan points x the SMPL-sized synthetic model (V = 6890, 13776 faces, P = 86), H alone in the comparison:

  fused   the forward, the search, then frame_chunk frames at a time the JVP with the 86 unit tangents and the Gram kernels
  dense   layer.jacobian for --dense-chunk frames at a time (default: all of them, which fits a 288 GB device), a torch gather
          of the three corner rows per point and one batched matmul, f32

Wall times with a device synchronisation on either side, the median of --reps runs after one warm-up.  Memory: the peak of
torch's allocator during the run, and the device memory in use after it minus before the first run (the library's own buffers
- the JVP's scratch, the handle's moments / mixed rows / partial panels - are not torch's, and they stay allocated).  The parts
of the fused path are timed one by one on the first chunk (forward + search + right-hand side once; JVP and Gram per chunk).
Usage: python3 tools/gram_bench.py [--frames 256] [--points 20000] [--chunk 32] [--mode plane] [--out profiles/gram_bench.txt]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--dense-chunk", type=int, default=0, help="frames per dense chunk (0: all)")
    ap.add_argument("--mode", default="plane", choices=["point", "plane"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    if api.device_count() < 1:
        raise SystemExit("gram_bench needs a GPU")
    F, N, mode = a.frames, a.points, a.mode
    model = synth.make_model(0)
    faces = synth.make_faces(model)
    layer = tl.SMPLLayer(api.Model(model))
    rng = np.random.default_rng(0)
    x = np.zeros((F, 76))
    x[:, 0] = 1.0
    x[:, 1:4] = rng.normal(scale=0.2, size=(F, 3))
    x[:, 4:7] = [0.0, 0.0, 3.0]
    x[:, 7:] = rng.normal(scale=0.15, size=(F, 69))
    x, beta = torch.tensor(x, device="cuda"), torch.tensor(rng.normal(size=model.n_shape), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    faces_t = torch.tensor(faces, device="cuda").long()
    with torch.no_grad():
        verts = layer(x, beta)[0]
        t = torch.randint(0, faces_t.shape[0], (F, N), generator=gen, device="cuda")
        b = torch.rand((F, N, 3), generator=gen, device="cuda") + 1e-3
        b = b / b.sum(dim=2, keepdim=True)
        corners = verts[torch.arange(F, device="cuda")[:, None, None], faces_t[t]]             # [F, N, 3, 3]
        points = ((b[..., None] * corners).sum(dim=2) + 0.002 * torch.randn((F, N, 3), generator=gen, device="cuda")).contiguous()
        del corners, t, b
    term = tl.SurfaceTerm(points, None, faces, trunc=0.05)
    V, P = model.n_verts, 76 + model.n_shape

    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free

    def run(fn):
        torch.cuda.synchronize()
        base = used()
        fn()                                               # warm-up: problems, handles, workspaces
        ts = []
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, float(np.median(ts)) * 1e3, torch.cuda.max_memory_allocated(), used() - base

    lines = []

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)

    (cost, g, H), ms_fused, peak_fused, dev_fused = run(lambda: term.normal_equations(layer, x, beta, mode=mode, frame_chunk=a.chunk))
    emit({"path": "fused", "frames": F, "points_per_frame": N, "V": V, "P": P, "mode": mode, "frame_chunk": a.chunk,
          "ms": round(ms_fused, 1), "torch_peak_MB": round(peak_fused / 2 ** 20, 1), "device_in_use_after_MB": round(dev_fused / 2 ** 20, 1)})

    # the parts, on the first chunk
    n = min(a.chunk, F)
    with torch.no_grad():
        stream = torch.cuda.current_stream().cuda_stream
        _, ms_pre, _, _ = run(lambda: term._jobs(layer(x, beta)[0], mode))
        cost_, rhs, jobs = term._jobs(layer(x, beta)[0], mode)
        job = jobs[0]
        work = torch.empty((n, P, V, 3), dtype=torch.float32, device="cuda")
        eye = torch.eye(P, dtype=torch.float64, device="cuda")
        tan_x, tan_b = eye[:, :76].expand(n, P, 76).contiguous(), eye[:, 76:].contiguous()
        prob = layer.chunk_problem(0, n)
        _, ms_jvp, _, _ = run(lambda: prob.forward_jvp_device(x[:n].data_ptr(), beta.data_ptr(), P, tan_x.data_ptr(), tan_b.data_ptr(),
                                                              None, work.data_ptr(), 3 * V, stream))
        pts, off, rows = job.chunk(0, n)
        gram = lambda: tl.surface_gram(work, pts, job.index[rows], job.bary[rows], job.handle, weight=job.weight[rows],
                                       direction=job.direction[rows] if job.direction is not None else None, rhs=rhs[:n])
        _, ms_gram, _, _ = run(gram)
        one = lambda: tl.surface_gram(work[:, :1], pts, job.index[rows], job.bary[rows], job.handle, weight=job.weight[rows],
                                      direction=job.direction[rows] if job.direction is not None else None)
        _, ms_one, _, _ = run(one)
    chunks = (F + a.chunk - 1) // a.chunk
    emit({"path": "fused parts", "chunks": chunks, "forward_search_rhs_ms": round(ms_pre, 1), "jvp_ms_per_chunk": round(ms_jvp, 2),
          "gram_ms_per_chunk": round(ms_gram, 2), "gram_with_one_tangent_ms_per_chunk": round(ms_one, 2),
          "share_jvp": round(chunks * ms_jvp / ms_fused, 3), "share_gram": round(chunks * ms_gram / ms_fused, 3),
          "share_grouping_and_moments": round(chunks * ms_one / ms_fused, 3),
          "share_mix_and_contraction": round(chunks * (ms_gram - ms_one) / ms_fused, 3),
          "note": "gram_with_one_tangent: the grouping and the moments with a 1-tangent mix and contraction, i.e. what does not "
                  "scale with P; the difference to gram_ms is the P-dependent mix, contraction and fold"})
    del work

    if not a.skip_dense:
        dc = a.dense_chunk if a.dense_chunk > 0 else F

        def dense():
            with torch.no_grad():
                verts = layer(x, beta)[0]
                dist2, index, bary = tl.closest_surface(points, verts, term._handle_for(verts))
                index, bary, dist2 = index.view(F, N), bary.view(F, N, 3), dist2.view(F, N)
                Hd = torch.empty((F, P, P), dtype=torch.float32, device="cuda")
                for f0 in range(0, F, dc):
                    f1 = min(f0 + dc, F)
                    Jv = layer.jacobian(x[f0:f1], beta)[0]                                       # [fc, P, V, 3]
                    ids = faces_t[index[f0:f1].clamp(min=0).long()]                               # [fc, N, 3]
                    w = ((index[f0:f1] >= 0) & (dist2[f0:f1] < 0.05 * 0.05)).float()
                    A = torch.zeros((f1 - f0, P, N, 3), dtype=torch.float32, device="cuda")
                    for c in range(3):
                        gi = ids[:, None, :, c, None].expand(f1 - f0, P, N, 3)
                        A += bary[f0:f1, None, :, c, None] * torch.gather(Jv, 2, gi)
                    if mode == "plane":
                        cr = verts[torch.arange(f0, f1, device="cuda")[:, None, None], ids]
                        nrm = torch.linalg.cross(cr[:, :, 1] - cr[:, :, 0], cr[:, :, 2] - cr[:, :, 0])
                        d = nrm / nrm.norm(dim=2, keepdim=True).clamp(min=1e-30)
                        S = (A * d[:, None]).sum(dim=3) * w.sqrt()[:, None]                       # [fc, P, N]
                    else:
                        S = (A * w.sqrt()[:, None, :, None]).reshape(f1 - f0, P, 3 * N)
                    Hd[f0:f1] = S @ S.transpose(1, 2)
            return Hd

        Hd, ms_dense, peak_dense, dev_dense = run(dense)
        rel = float((H - Hd.double()).abs().max() / H.abs().max())
        emit({"path": "dense", "dense_chunk": dc, "ms": round(ms_dense, 1), "torch_peak_MB": round(peak_dense / 2 ** 20, 1),
              "device_in_use_after_MB": round(dev_dense / 2 ** 20, 1), "speedup_of_fused": round(ms_dense / ms_fused, 2),
              "max_abs_difference_of_H_over_max_H": float(f"{rel:.3e}")})
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write("# tools/gram_bench.py: wall ms, medians of %d runs after a warm-up\n" % a.reps)
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
