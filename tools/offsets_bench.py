"""What per-vertex offsets (bodyfit_forward_offsets*_device, k_offsets.hip) cost beside the calls they extend, at 256 and 1,024
frames on SMPL's counts.  Every figure is the median over brackets of back-to-back calls on one stream; within a bracket round
the variants run one after the other, so that a drift of the machine hits all of them alike.
  forward            bodyfit_forward_device                      forward_shared / forward_frames   with [V, 3] / [F, V, 3] offsets
  vjp                bodyfit_forward_vjp_device                  vjp_shared / vjp_frames           with offsets and their gradient
  vjp_*_nograd       with offsets, d_grad_offsets NULL (the displace kernel alone is the difference to vjp)
  apply_*_us         forward_* - forward: k_offsets_apply (it cannot be launched alone)
  rmw_us             cloud.add_(other) in torch on the same [F, V, 3] f32 cloud: 24 B read and 12 B written per vertex, the traffic
                     of the apply kernel with per-frame offsets
  grad_*_us          vjp_* - vjp_*_nograd: k_offsets_grad (shared: the ascending f64 sum over the frames)
  apply_floor_us     36 B (frames) per (frame, vertex) over the nominal 8 TB/s
Usage: python3 tools/offsets_bench.py [--frames 256 1024] [--brackets 9] [--calls 10] [--out profiles/offsets_bench.txt]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--brackets", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    if api.device_count() < 1:
        raise SystemExit("offsets_bench needs a GPU")
    model = synth.make_model(0)
    gm = api.Model(model)
    V, nJ, nS = model.n_verts, model.n_joints, model.n_shape
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    lines = ["# tools/offsets_bench.py on one MI355X: median of %d brackets of %d back-to-back calls on one stream (microseconds)" %
             (a.brackets, a.calls),
             "# apply_* = forward_* - forward, grad_* = vjp_* - vjp_*_nograd (differences of medians); rmw_us: torch cloud.add_(other);",
             "# apply_floor_us: 36 B per (frame, vertex) over the nominal 8 TB/s"]
    for F in a.frames:
        seq = synth.make_sequence(model, min(F, 64), seed=0)
        x = np.tile(seq.gt_params, ((F + 63) // 64, 1))[:F]
        prob = api.Problem(gm, np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), seq.intr,
                           np.tile(seq.R0[:1], (F, 1)), n_cols=76 + nS, use_shape=True, want_mesh=True)
        dev = "cuda"
        xt = torch.tensor(x, device=dev)
        bt = torch.tensor(seq.gt_beta, device=dev)
        verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
        other = torch.randn((F, V, 3), dtype=torch.float32, device=dev) * 0.01
        joints = torch.empty((F, nJ, 3), dtype=torch.float64, device=dev)
        G = torch.randn((F, V, 3), dtype=torch.float32, device=dev)
        H = torch.randn((F, nJ, 3), dtype=torch.float64, device=dev)
        gx = torch.empty((F, 76), dtype=torch.float64, device=dev)
        gb = torch.empty((nS,), dtype=torch.float64, device=dev)
        d_s = torch.randn((V, 3), dtype=torch.float32, device=dev) * 0.01
        d_f = torch.randn((F, V, 3), dtype=torch.float32, device=dev) * 0.01
        go_s, go_f = torch.empty_like(d_s), torch.empty_like(d_f)

        def fwd(d=None, stride=0):
            return lambda: prob.forward_device(xt.data_ptr(), bt.data_ptr(), joints.data_ptr(), verts.data_ptr(), 3 * V, sp,
                                               d_offsets_ptr=d.data_ptr() if d is not None else None, offsets_frame_stride=stride)

        def vjp(d=None, stride=0, go=None):
            return lambda: prob.forward_vjp_device(xt.data_ptr(), bt.data_ptr(), G.data_ptr(), H.data_ptr(), gx.data_ptr(),
                                                   gb.data_ptr(), 3 * V, sp, d_offsets_ptr=d.data_ptr() if d is not None else None,
                                                   offsets_frame_stride=stride,
                                                   d_grad_offsets_ptr=go.data_ptr() if go is not None else None)

        variants = {
            "forward": fwd(), "forward_shared": fwd(d_s, 0), "forward_frames": fwd(d_f, 3 * V),
            "rmw": lambda: verts.add_(other),
            "vjp": vjp(), "vjp_shared_nograd": vjp(d_s, 0), "vjp_shared": vjp(d_s, 0, go_s),
            "vjp_frames_nograd": vjp(d_f, 3 * V), "vjp_frames": vjp(d_f, 3 * V, go_f),
        }
        for fn in variants.values():
            fn(); fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.brackets):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    fn()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.calls)
        t = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
        r = lambda v: round(v, 1)
        row = {"frames": F}
        row.update({k + "_us": r(v) for k, v in t.items()})
        row.update({
            "apply_shared_us": r(t["forward_shared"] - t["forward"]), "apply_frames_us": r(t["forward_frames"] - t["forward"]),
            "forward_frames_over_forward": round(t["forward_frames"] / t["forward"], 2),
            "apply_frames_over_rmw": round((t["forward_frames"] - t["forward"]) / t["rmw"], 2),
            "apply_floor_us": r(F * V * 36 / HBM_BPS * 1e6),
            "grad_shared_us": r(t["vjp_shared"] - t["vjp_shared_nograd"]), "grad_frames_us": r(t["vjp_frames"] - t["vjp_frames_nograd"]),
            "displace_shared_us": r(t["vjp_shared_nograd"] - t["vjp"]),
            "vjp_shared_over_vjp": round(t["vjp_shared"] / t["vjp"], 3), "vjp_frames_over_vjp": round(t["vjp_frames"] / t["vjp"], 3),
        })
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        prob.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
