"""Times of the fitting objective's reverse mode (bodyfit_residual_vjp_device) at 256, 1,024 and 4,096 frames of a synthetic
25-keypoint sequence (shared beta, GMM pose prior, shape prior, temporal terms), each the median of brackets of back-to-back
calls on one stream:
  sweep_us       the Jacobian sweep alone (bodyfit_evaluate_device, want_jacobian; the problem has no mesh)
  vjp_reuse_us   residual_vjp_device with reuse_jacobian = 1: k_residual_vjp + the beta sum, beside
  hbm_floor_us   its bytes (the J panel and g read, the gradients written) over the nominal 8 TB/s
  vjp_sweep_us   residual_vjp_device with reuse_jacobian = 0 (the sweep, then the product)
--kernel-only: one sweep and `--calls` products per frame count, nothing timed (for a rocprofv3 --kernel-trace --stats run).
Usage: python3 tools/objective_bench.py [--frames 256 1024 4096] [--brackets 7] [--calls 10] [--kernel-only]"""
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
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--brackets", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch
    api = importlib.import_module("3dbodyanimation_amd.api")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    model = synth.make_model(0)
    gm = api.Model(model)
    gmm = api.Gmm(*synth.make_gmm(0))
    nS = model.n_shape
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for F in a.frames:
        seq = synth.make_sequence(model, F, seed=0)
        prob = api.Problem.from_sequence(gm, seq, n_cols=76 + nS, use_shape=True, beta_pose=20.0, gmm=gmm, beta_shape=25.0,
                                         lambda_temporal=3.0)
        L = prob.layout
        dev = "cuda"
        xt = torch.tensor(seq.gt_params + 0.01, device=dev)
        bt = torch.tensor(seq.gt_beta, device=dev)
        g = torch.randn(L.total_rows, dtype=torch.float64, device=dev)
        gx = torch.empty((F, 76), dtype=torch.float64, device=dev)
        gb = torch.empty((nS,), dtype=torch.float64, device=dev)

        def sweep():
            prob.evaluate_device(xt.data_ptr(), bt.data_ptr(), True, sp)

        def vjp(reuse):
            return lambda: prob.residual_vjp_device(xt.data_ptr(), bt.data_ptr(), g.data_ptr(), gx.data_ptr(), gb.data_ptr(),
                                                    reuse, sp)

        if a.kernel_only:
            sweep()
            for _ in range(a.calls):
                vjp(True)()
            torch.cuda.synchronize()
            prob.close()
            continue

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

        t_sweep = timed(sweep)
        sweep()
        t_reuse = timed(vjp(True))
        t_full = timed(vjp(False))
        hbm_bytes = L.reproj_rows * L.n_cols * 8 + L.total_rows * 8 + F * (76 + nS) * 8 + F * 4 + nS * 8
        print(json.dumps({"frames": F, "keypoints": L.n_keypoints, "sweep_us": round(t_sweep, 1),
                          "vjp_reuse_us": round(t_reuse, 1), "hbm_floor_us": round(hbm_bytes / HBM_BPS * 1e6, 1),
                          "hbm_MB": round(hbm_bytes / 1e6, 1), "vjp_sweep_us": round(t_full, 1),
                          "reuse_over_sweep": round(t_reuse / t_sweep, 3)}), flush=True)
        prob.close()


if __name__ == "__main__":
    main()
