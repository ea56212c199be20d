"""Forward-JVP times of the library's SMPL forward (bodyfit_forward_jvp_device) at 256 and 1,024 frames x K = 1, 32, 86 tangents,
each the median of brackets of back-to-back calls on one stream, beside the same run's bodyfit_forward_device time and two
yardsticks:
  2K forwards    what a central-difference Jacobian through the forward costs today: 2 K x the forward measured in this run
  write floor    the bytes of the output ([F][K][V][3] f32 and [F][K][nJ][3] f64) over the nominal 8 TB/s
Usage: python3 tools/jvp_bench.py [--frames 256 1024] [--tangents 1 32 86] [--brackets 7] [--calls 10]"""
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
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 32, 86])
    ap.add_argument("--brackets", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    import torch
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    model = synth.make_model(0)
    gm = api.Model(model)
    V, nJ, nS = model.n_verts, model.n_joints, model.n_shape
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    dev = "cuda"

    def timed(fn):
        fn(); fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.brackets):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        return float(np.median(ms)) * 1e3

    for F in a.frames:
        seq = synth.make_sequence(model, min(F, 64), seed=0)
        x = np.tile(seq.gt_params, ((F + 63) // 64, 1))[:F]
        prob = api.Problem(gm, np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), seq.intr,
                           np.tile(seq.R0[:1], (F, 1)), n_cols=76 + nS, use_shape=True, want_mesh=True)
        xt = torch.tensor(x, device=dev)
        bt = torch.tensor(seq.gt_beta, device=dev)
        verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
        joints = torch.empty((F, nJ, 3), dtype=torch.float64, device=dev)
        t_fwd = timed(lambda: prob.forward_device(xt.data_ptr(), bt.data_ptr(), joints.data_ptr(), verts.data_ptr(), 3 * V, sp))
        for K in a.tangents:
            tx = torch.randn((F, K, 76), dtype=torch.float64, device=dev)
            tb = torch.randn((K, nS), dtype=torch.float64, device=dev)
            tv = torch.empty((F, K, V, 3), dtype=torch.float32, device=dev)
            tj = torch.empty((F, K, nJ, 3), dtype=torch.float64, device=dev)
            t_jvp = timed(lambda: prob.forward_jvp_device(xt.data_ptr(), bt.data_ptr(), K, tx.data_ptr(), tb.data_ptr(),
                                                          tj.data_ptr(), tv.data_ptr(), 3 * V, sp))
            t_jj = timed(lambda: prob.forward_jvp_device(xt.data_ptr(), bt.data_ptr(), K, tx.data_ptr(), tb.data_ptr(),
                                                         tj.data_ptr(), None, 3 * V, sp))
            out_bytes = F * K * (V * 3 * 4 + nJ * 3 * 8)
            print(json.dumps({"frames": F, "tangents": K, "forward_us": round(t_fwd, 1), "jvp_us": round(t_jvp, 1),
                              "jvp_joints_only_us": round(t_jj, 1), "two_k_forwards_us": round(2 * K * t_fwd, 1),
                              "two_k_forwards_over_jvp": round(2 * K * t_fwd / t_jvp, 2),
                              "write_floor_us": round(out_bytes / HBM_BPS * 1e6, 1),
                              "jvp_over_write_floor": round(t_jvp / (out_bytes / HBM_BPS * 1e6), 1)}), flush=True)
            del tx, tb, tv, tj
        prob.close()


if __name__ == "__main__":
    main()
