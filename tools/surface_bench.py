"""Forward and backward times of the closest-surface search (bodyfit_closest_surface_device, bodyfit_closest_surface_vjp_device;
k_closest_surface.hip) at SMPL's size, 6890 vertices / 13,776 faces, for 1, 32 and 256 frames of 20,000 scan points, each the
median of brackets of back-to-back calls on one stream (HIP events, after warm-up).  Beside them, in the same process:
closest_points at the same sizes (points -> vertices, with prepare_vjp, and its backward), and a chunked plain-torch
point-triangle evaluation (three clamped edge projections and the interior projection per pair, min over the faces), timed on at
most --torch-frames frames and reported per frame.  The fused forward is timed WITH prepare_vjp (what a training step pays) and
without.  Also printed: the ratio to closest_points and triangle tests (pairs) per second.
The ORIENTED search (bodyfit_closest_surface_oriented_device) is timed in the same run on the same points, search only like
surface_search_only_us, with the direction of every point the normal of the face it was generated on and min_cos = 0 and 0.5;
beside each time the share of points that found a compatible triangle and the share whose triangle differs from the
unoriented search's.
The share of pairs the sphere cull removes is NOT read from the kernel (a counter would sit in its inner loop): it is a HOST
REPLAY in numpy of the kernel's order and f32 arithmetic for one workgroup, the first 256 queries of frame 0 without a split
(the f32 form is the one the tests check against the contract, tests/surface_ref.py, which is why this tool imports it): per pair
(lanes that skip) and per wave evaluation (a wave skips a triangle for a query slot only when all 64 lanes do).  The keys say so.
Topology: the faces ("f") of a real SMPL .npz when one is found — --model, else $BODYFIT_SMPL_NPZ, else the first *.npz with
6890 vertices and faces under data/ or models/ of the repository — else --faces (.npy int32 [n, 3]), else synth.make_faces at
13,776 faces.
Usage: python3 tools/surface_bench.py [--sizes 1x20000 32x20000 256x20000] [--brackets 5] [--out profiles/surface_bench.txt]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V, NF = 6890, 13776
SIZES = [(1, 20000), (32, 20000), (256, 20000)]


def find_model_faces(explicit):
    """(faces, name) of the first SMPL .npz with 6890 vertices and an "f" array among: the explicit path, $BODYFIT_SMPL_NPZ,
    data/ and models/ of the repository; None when there is none"""
    import glob
    cands = [explicit, os.environ.get("BODYFIT_SMPL_NPZ")]
    for d in ("data", "models"):
        cands += sorted(glob.glob(os.path.join(ROOT, d, "**", "*.npz"), recursive=True))
    for path in cands:
        if not path or not os.path.exists(path):
            continue
        try:
            z = np.load(path, allow_pickle=True)
            if "f" in z.files and "v_template" in z.files and np.asarray(z["v_template"]).shape[0] == V:
                return np.ascontiguousarray(z["f"], dtype=np.int32), os.path.basename(path)
        except Exception:
            continue
    return None


def cull_share(sr, q256, verts, faces):
    """replays k_cs_search for one workgroup (256 queries, four waves taking the faces t = wave mod 4 in ascending order, no
    split): (share of pairs skipped, share of wave-level evaluations skipped)"""
    R = sr.prepare_records(verts, faces)
    f = np.float32
    mx = R["cx"].astype(np.float64) - 0.5 * R["L"].astype(np.float64)
    rad = (np.maximum(0.5 * R["L"].astype(np.float64), np.sqrt(mx * mx + R["t"].astype(np.float64) ** 2)) * (1 + 1 / 4096)).astype(f)
    infl = f(1 + 1 / 4096)
    pairs = issued = total = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for wave in range(4):
            best = np.full(256, np.inf, f); bs = best.copy()
            for t in range(wave, len(faces), 4):
                ap = q256 - R["A"][t]
                ap2 = ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1] + ap[:, 2] * ap[:, 2]
                X = ap[:, 0] * R["u"][t, 0] + ap[:, 1] * R["u"][t, 1] + ap[:, 2] * R["u"][t, 2]
                dc2 = ap2 + f(0.25) * R["L"][t] * R["L"][t] - R["L"][t] * X
                reach = bs + rad[t]
                need = dc2 <= reach * reach
                total += 256
                pairs += int(need.sum())
                issued += 64 * int(need.reshape(4, 64).any(axis=1).sum())
                if need.any():
                    d, _, _ = sr._eval_f32(ap[need], {k: (v[t] if k != "rot" else v) for k, v in R.items()})
                    idx = np.flatnonzero(need)
                    lt = d < best[idx]
                    best[idx[lt]] = d[lt]
                    bs[idx[lt]] = np.sqrt(d[lt]) * infl
    return 1.0 - pairs / total, 1.0 - issued / total


def torch_surface(torch, P, verts, faces_t, chunk):
    """plain torch, f32: min over the faces of the point-triangle distance, [chunk, n_faces] at a time; (dist2, index) of one frame"""
    v0, v1, v2 = verts[faces_t[:, 0]], verts[faces_t[:, 1]], verts[faces_t[:, 2]]
    e1, e2, e3 = v1 - v0, v2 - v0, v2 - v1
    a, b, c, l3 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (e3 * e3).sum(1)
    det = a * c - b * b
    ok = det > 1e-12 * a * c
    sdet = torch.where(ok, det, torch.ones_like(det))
    out_d, out_i = [], []
    for s in range(0, P.shape[0], chunk):
        ap = P[s:s + chunk, None, :] - v0[None]
        d1, d2 = (ap * e1[None]).sum(2), (ap * e2[None]).sum(2)

        def seg(S_ap, D, dd, dotv):
            t = torch.clamp(dotv / torch.clamp(dd, min=1e-30), 0, 1)
            r = S_ap - t[..., None] * D[None]
            return (r * r).sum(2)

        best = seg(ap, e1, a, d1)
        best = torch.minimum(best, seg(ap, e2, c, d2))
        bp = ap - e1[None]
        best = torch.minimum(best, seg(bp, e3, l3, (bp * e3[None]).sum(2)))
        vv = (c * d1 - b * d2) / sdet
        ww = (a * d2 - b * d1) / sdet
        inside = ok[None] & (vv >= 0) & (ww >= 0) & (vv + ww <= 1)
        r = ap - vv[..., None] * e1[None] - ww[..., None] * e2[None]
        best = torch.where(inside, (r * r).sum(2), best)
        m = best.min(dim=1)
        out_d.append(m.values); out_i.append(m.indices)
    return torch.cat(out_d), torch.cat(out_i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=[f"{f}x{n}" for f, n in SIZES])
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--budget-s", type=float, default=0.5, help="target duration of one bracket")
    ap.add_argument("--torch-frames", type=int, default=1)
    ap.add_argument("--torch-chunk", type=int, default=1024)
    ap.add_argument("--faces", default=None)
    ap.add_argument("--model", default=None, help="an SMPL .npz (drivers.load_smpl_npz) whose faces are used")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import surface_ref as sr
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    if api.device_count() < 1:
        raise SystemExit("surface_bench needs a GPU")
    model = synth.make_model(0)
    assert model.n_verts == V
    real = find_model_faces(a.model)
    if real is not None:
        faces, topo = real
    elif a.faces:
        faces = np.ascontiguousarray(np.load(a.faces), np.int32)
        topo = os.path.basename(a.faces)
    else:
        faces = synth.make_faces(model, n_faces=NF)
        topo = "synth.make_faces"
    nf = len(faces)
    surf = api.Surface(0, V, faces)
    cp = api.ClosestPoints(0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    faces_t = torch.tensor(faces.astype(np.int64), device="cuda")
    lines = []

    def timed(fn):
        fn(); fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        calls = int(max(1, min(50, a.budget_s * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        ms = []
        for _ in range(a.brackets):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / calls)
        return float(np.median(ms)) * 1e3   # us

    base = (model.v_template + np.array([0.0, 0.0, 3.0])).astype(np.float32)
    for size in a.sizes:
        F, N = (int(t) for t in size.split("x"))
        rng = np.random.default_rng(F * 100003 + N)
        gen = torch.Generator(device="cuda").manual_seed(F * 100003 + N)
        verts = torch.tensor(base, device="cuda")[None] + 1e-3 * torch.randn((F, V, 3), generator=gen, device="cuda")
        verts = verts.contiguous()
        t = torch.randint(0, nf, (F, N), generator=gen, device="cuda")
        bw = torch.rand((F, N, 3), generator=gen, device="cuda") + 1e-3
        bw = bw / bw.sum(dim=2, keepdim=True)
        corners = torch.gather(verts, 1, faces_t[t].reshape(F, 3 * N, 1).expand(F, 3 * N, 3)).view(F, N, 3, 3)
        pts = ((bw[..., None] * corners).sum(dim=2) + 5e-3 * torch.randn((F, N, 3), generator=gen, device="cuda")).contiguous()
        qs = api.PointSet.uniform(pts.data_ptr(), N)
        rs = api.PointSet.uniform(verts.data_ptr(), V)
        d2 = torch.empty(F * N, dtype=torch.float32, device="cuda")
        ix = torch.empty(F * N, dtype=torch.int32, device="cuda")
        bary = torch.empty((F * N, 3), dtype=torch.float32, device="cuda")
        g = torch.randn(F * N, generator=gen, device="cuda")
        # directions: the unit normal of the generating face (a face without area: +z)
        e1, e2 = corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 0]
        nrm = torch.linalg.cross(e1, e2)
        ln = nrm.norm(dim=2, keepdim=True)
        nrm = torch.where(ln > 0, nrm / ln.clamp(min=1e-30), torch.tensor([0.0, 0.0, 1.0], device="cuda")).contiguous()
        od2, oix, obary = torch.empty_like(d2), torch.empty_like(ix), torch.empty_like(bary)
        gq, gv = torch.empty_like(pts), torch.empty_like(verts)

        def s_fwd_plain():
            surf.closest_device(qs, verts.data_ptr(), 3 * V, F, F * N, d2.data_ptr(), ix.data_ptr(), bary.data_ptr(), sp)

        def s_fwd():
            surf.closest_device(qs, verts.data_ptr(), 3 * V, F, F * N, d2.data_ptr(), ix.data_ptr(), bary.data_ptr(), sp,
                                prepare_vjp=True)

        def s_oriented(min_cos):
            def fn():
                surf.closest_oriented_device(qs, nrm.data_ptr(), min_cos, verts.data_ptr(), 3 * V, F, F * N, od2.data_ptr(),
                                             oix.data_ptr(), obary.data_ptr(), sp)
            return fn

        def s_bwd():
            surf.vjp_device(qs, verts.data_ptr(), 3 * V, F, F * N, ix.data_ptr(), bary.data_ptr(), g.data_ptr(), gq.data_ptr(),
                            gv.data_ptr(), sp)

        pd2 = torch.empty(F * N, dtype=torch.float32, device="cuda")
        pix = torch.empty(F * N, dtype=torch.int32, device="cuda")

        def p_fwd():
            cp.points_device(qs, rs, F, F * N, F * V, pd2.data_ptr(), pix.data_ptr(), sp, prepare_vjp=True)

        def p_bwd():
            cp.points_vjp_device(qs, rs, F, F * N, F * V, pix.data_ptr(), g.data_ptr(), gq.data_ptr(), gv.data_ptr(), sp)

        Ft = min(F, a.torch_frames)
        t_out = {}

        def t_fwd():
            for f in range(Ft):
                t_out[f] = torch_surface(torch, pts[f], verts[f], faces_t, a.torch_chunk)

        us_sp = timed(s_fwd_plain)
        oriented = {}
        for mc in (0.0, 0.5):
            us_o = timed(s_oriented(mc))
            torch.cuda.synchronize()
            oriented[mc] = (us_o, float((oix >= 0).float().mean()), float((oix != ix).float().mean()))
        us_sp2 = timed(s_fwd_plain)      # the unoriented search once more, after the oriented ones: the spread of this run
        us_sf, us_sb = timed(s_fwd), timed(s_bwd)
        us_pf, us_pb = timed(p_fwd), timed(p_bwd)
        us_t = timed(t_fwd) / Ft
        torch.cuda.synchronize()
        td, _ = t_out[0]
        rel = float(((td.sqrt() - d2[:N].sqrt()).abs() / (d2[:N].sqrt() + 1e-3)).max())
        skip_pair, skip_wave = cull_share(sr, pts[0, :256].cpu().numpy(), verts[0].cpu().numpy(), faces)
        pairs = float(F) * N * nf
        row = {"frames": F, "n_points": N, "n_faces": nf, "topology": topo, "pairs": pairs,
               "surface_search_only_us": round(us_sp, 1), "surface_forward_us": round(us_sf, 1), "surface_backward_us": round(us_sb, 1),
               "points_forward_us": round(us_pf, 1), "points_backward_us": round(us_pb, 1),
               "forward_ratio_to_closest_points": round(us_sf / us_pf, 2), "backward_ratio_to_closest_points": round(us_sb / us_pb, 2),
               "surface_search_only_us_repeated": round(us_sp2, 1),
               "oriented_search_only_us_min_cos_0": round(oriented[0.0][0], 1),
               "oriented_search_only_us_min_cos_0.5": round(oriented[0.5][0], 1),
               "oriented_share_matched_min_cos_0": round(oriented[0.0][1], 4), "oriented_share_matched_min_cos_0.5": round(oriented[0.5][1], 4),
               "oriented_share_other_triangle_min_cos_0": round(oriented[0.0][2], 4),
               "oriented_share_other_triangle_min_cos_0.5": round(oriented[0.5][2], 4),
               "triangle_gpairs_per_s": round(pairs / us_sp * 1e-3, 1),
               "point_gpairs_per_s": round(float(F) * N * V / us_pf * 1e-3, 1),
               "torch_forward_us_per_frame": round(us_t, 1), "torch_frames_timed": Ft,
               "forward_speedup_per_frame_vs_torch": round(us_t / (us_sf / F), 1),
               "host_replay_one_workgroup_share_of_pairs_culled": round(skip_pair, 4),
               "host_replay_one_workgroup_share_of_wave_evaluations_culled": round(skip_wave, 4),
               "max_rel_distance_difference_to_torch_f32": float(f"{rel:.2e}")}
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
        del verts, pts, corners, d2, ix, bary, g, gq, gv, pd2, pix, t_out, nrm, od2, oix, obary, e1, e2, ln
        torch.cuda.empty_cache()
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write("# tools/surface_bench.py: us per call, medians of %d brackets; V = %d, n_faces = %d (%s)\n" % (a.brackets, V, nf, topo))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
