"""Times of the TSDF fusion (bodyfit_volume_integrate_device, k_tsdf.hip): a shared 256^3 volume (a 2 m cube, 7.8 mm voxels) fused
from 64 and 256 depth maps of 640 x 480 and from 32 of 1920 x 1080, and 64 per-frame 128^3 volumes from 64 maps of 640 x 480; the
cameras turn about the cube's middle, the depth maps are a rippled surface through it, every call continues a state (reset = 0:
the volume is read and written).  Timed with the protocol of tools/volume_bench.py (a warm-up, then --brackets brackets of
back-to-back calls, host clock around work that ends in a device synchronise; median [min .. max] of the brackets); the
alternatives of one comparison are ALTERNATED bracket by bracket inside one call, so a drift of the machine falls on all of them:
  fuse       k_tsdf_integrate, one launch, against
  torch      the same step composed in torch on the same device, frame by frame: grid_points (once, outside the timing), the pose
             and the projection in f64, the nearest pixel, the gather, the masks, the running average with torch.where;
  copy       a plain copy of the volume's two arrays by torch, and
  floor      the bytes the call needs (the two arrays read and written once, the depth maps read once) over 6.3 TB/s, the
             streaming rate the machine sustains: the pose arithmetic and the gathers' scatter are not in it.
Then sample_volume's kernel (bodyfit_volume_sample_device, untouched by the fusion) from this build and, with --parent-lib, from a
library built from the parent commit, loaded side by side and alternated: the same bits and the same time are what is to be seen.
Nothing is asserted; every comparison is printed whichever way it falls, in capitals where the kernel is the slower one.
--variant NAME=PATH (repeatable) adds the fusion kernel of another build of the library (one built with -DTSDF_AHEAD=1, 2 or 8:
how many frames' gathers are issued ahead of their use) to the alternation, on a state of its own.
Usage: python3 tools/tsdf_bench.py [--brackets 5] [--parent-lib PATH] [--variant NAME=PATH ...] [--quick] [--out profiles/tsdf_bench.txt]"""
import argparse
import ctypes
import importlib
import json
import math
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


def cameras(F, middle, rng):
    """[F, 12] f64 world -> camera: a turn of up to +-0.3 rad about an axis near y through `middle`, and a small shift"""
    out = np.empty((F, 12))
    for f in range(F):
        axis = np.array([0.1 * rng.normal(), 1.0, 0.1 * rng.normal()])
        axis /= np.linalg.norm(axis)
        a = 0.3 * math.sin(2.0 * math.pi * f / max(F, 1))
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K
        t = middle - R @ middle + rng.uniform(-0.02, 0.02, size=3)
        out[f] = np.concatenate([R, t.reshape(3, 1)], axis=1).reshape(12)
    return out


def torch_step(torch, pts, depth_f, pose_f, intr, trunc, z_near, max_weight, D, W):
    """one frame of the definition composed in torch, in place on (D, W); pts [nz, ny, nx, 3] f64"""
    H, Wd = depth_f.shape
    A, t = pose_f.view(3, 4)[:, :3], pose_f.view(3, 4)[:, 3]
    q = pts @ A.T + t
    qz = q[..., 2]
    cj = torch.floor(intr[0] * q[..., 0] / qz + intr[2] + 0.5)
    ci = torch.floor(intr[1] * q[..., 1] / qz + intr[3] + 0.5)
    hit = (qz > z_near) & (cj >= 0) & (cj <= Wd - 1) & (ci >= 0) & (ci <= H - 1)
    pixel = torch.where(hit, ci * Wd + cj, torch.zeros_like(cj)).long()
    d = depth_f.reshape(-1)[pixel.reshape(-1)].view(qz.shape).double()
    s = d - qz
    upd = hit & torch.isfinite(d) & (d > 0) & (s >= -trunc)
    seen = (W > 0) & torch.isfinite(D)
    w0 = torch.where(seen, W, torch.zeros_like(W)).double()
    wd = torch.where(seen, W.double() * D.double(), torch.zeros_like(w0))
    Dn = ((wd + s.clamp(max=trunc)) / (w0 + 1)).float()
    Wn = (w0 + 1).clamp(max=max_weight).float()
    nan = torch.full_like(D, float("nan"))
    D.copy_(torch.where(upd, Dn, torch.where(seen, D, nan)))
    W.copy_(torch.where(upd, Wn, torch.where(seen, W, torch.zeros_like(W))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libbodyfit.so built from the parent commit, for the sampler's comparison")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH",
                    help="a libbodyfit.so built with another setting of the kernel (-DTSDF_AHEAD=...), timed beside this build's")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    volume = importlib.import_module("3dbodyanimation_amd.torch_layer.volume")
    if api.device_count() < 1:
        raise SystemExit("tsdf_bench needs a GPU: nothing here can be timed on the CPU")
    rng = np.random.default_rng(5)
    stream = torch.cuda.current_stream().cuda_stream
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# tsdf_bench: brackets={args.brackets}; times in ms per call: median [min .. max] x calls per bracket; alternatives "
             f"alternate bracket by bracket" + ("; QUICK sizes: a rehearsal, not a measurement" if args.quick else "")]
    out_rows = []
    variants = {}
    for item in args.variant:
        path = item.split("=", 1)[1]
        lib = variants[path] = ctypes.CDLL(os.path.abspath(path))
        lib.bodyfit_volume_create.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_double)] * 2 + [ctypes.POINTER(ctypes.c_void_p)]
        lib.bodyfit_volume_integrate_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_double,
                                                        ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_longlong, ctypes.c_void_p]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    big, small = (64, 32) if args.quick else (256, 128)
    vga, hd = ((48, 64, 52.5), (108, 192, 140.0)) if args.quick else ((480, 640, 525.0), (1080, 1920, 1400.0))
    sizes = [("shared", big, 64, vga, False), ("shared", big, 256, vga, False), ("shared", big, 32, hd, False),
             ("per frame", small, 64, vga, True)]
    if args.quick:
        sizes = [(a, n, max(F // 16, 2), im, pf) for a, n, F, im, pf in sizes]
    trunc, z_near, cap = 0.04, 0.1, 64.0
    for label, n, F, (H, Wd, fx), per_frame in sizes:
        dims, spacing = (n, n, n), (2.0 / n,) * 3
        origin = (-1.0 + 1.0 / n, -1.0 + 1.0 / n, 1.5 + 1.0 / n)
        middle = np.array([0.0, 0.0, 2.5])
        intr = (fx, fx, 0.5 * (Wd - 1), 0.5 * (H - 1))
        handle = api.Volume(0, dims, origin, spacing)
        pose = torch.tensor(cameras(F, middle, rng), device="cuda")
        ii = torch.linspace(0.0, 1.0, H, device="cuda")[:, None]
        jj = torch.linspace(0.0, 1.0, Wd, device="cuda")[None, :]
        depth = torch.stack([2.5 + 0.5 * torch.sin(3.0 * jj + 0.1 * f) * torch.cos(2.0 * ii) for f in range(F)]).float().contiguous()
        depth[:, : H // 16, : Wd // 16] = 0.0                     # a corner that holds nothing
        shape = (F, n, n, n) if per_frame else (n, n, n)
        # the state the timed calls continue: the first frame(s) fused once
        D0, W0 = volume.integrate_tsdf(depth[:F if per_frame else 1], intr, origin, spacing, dims, trunc, pose=pose[:F if per_frame else 1],
                                       z_near=z_near, max_weight=cap, per_frame=per_frame)
        D, W = D0.clone(), W0.clone()
        D2, W2 = torch.empty_like(D), torch.empty_like(W)
        pts = volume.grid_points(origin, spacing, dims, "cuda").double()
        intr_t = [float(a) for a in intr]

        def fuse():
            handle.integrate_device(depth.data_ptr(), H * Wd, H, Wd, F, intr, pose.data_ptr(), trunc, z_near, cap, False,
                                    D.data_ptr(), W.data_ptr(), n ** 3 if per_frame else 0, stream)

        def variant_fuser(path):
            """the same call through another build of the library, on a state of its own: (fn, D, W)"""
            lib = variants[path]
            h = ctypes.c_void_p()
            assert lib.bodyfit_volume_create(0, n, n, n, (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*spacing), ctypes.byref(h)) == 0
            Dv, Wv = D0.clone(), W0.clone()
            k = (ctypes.c_double * 4)(*intr)

            def fn():
                assert lib.bodyfit_volume_integrate_device(h, depth.data_ptr(), H * Wd, H, Wd, F, k, pose.data_ptr(), trunc, z_near, cap, 0,
                                                           Dv.data_ptr(), Wv.data_ptr(), n ** 3 if per_frame else 0, stream) == 0
            return fn, Dv, Wv

        def composed():
            for f in range(F):
                Df, Wf = (D2[f], W2[f]) if per_frame else (D2, W2)
                torch_step(torch, pts, depth[f], pose[f], intr_t, trunc, z_near, cap, Df, Wf)

        def copy():
            D2.copy_(D)
            W2.copy_(W)

        # one step of each from the same state: what the two agree on
        D.copy_(D0); W.copy_(W0); fuse()
        D2.copy_(D0); W2.copy_(W0); composed()
        torch.cuda.synchronize()
        same_seen = bool((torch.isfinite(D) == torch.isfinite(D2)).all())
        both = torch.isfinite(D) & torch.isfinite(D2)
        d_max = float((D - D2)[both].abs().max()) if bool(both.any()) else 0.0
        w_diff = int((W != W2).sum())
        observed = int(torch.isfinite(D).sum())
        fns = {"fuse": fuse, "torch": composed, "copy": copy}
        others = {}
        for item in args.variant:
            name, path = item.split("=", 1)
            fn, Dv, Wv = variant_fuser(path)
            fn()
            torch.cuda.synchronize()
            others[name] = bool((Dv.view(torch.int32) == D.view(torch.int32)).all()) and bool((Wv == W).all())
            fns["fuse " + name] = fn
        t = alternate(torch, fns, args.brackets)
        voxels = n ** 3 * (F if per_frame else 1)
        floor = (voxels * 16 + F * H * Wd * 4) / (STREAM_TBPS * 1e12)
        steps = n ** 3 * F
        ratio = t["fuse"][0] / t["torch"][0]
        say(f"{n}^3 {label:>9s}, F={F:<3d} of {Wd} x {H} ({voxels} voxels, {observed} observed): fuse {fmt(t['fuse'])}  torch {fmt(t['torch'])}  "
            f"copy {fmt(t['copy'])}")
        say(f"{'':>6s} fuse / torch = {ratio:.4f}" + (" (THE KERNEL IS SLOWER)" if ratio > 1 else f" ({1 / ratio:.0f} x)")
            + f"; fuse / copy = {t['fuse'][0] / t['copy'][0]:.2f}" + (" (SLOWER THAN THE COPY)" if t['fuse'][0] > t['copy'][0] else "")
            + f"; floor {floor * 1e3:.4f} ms (16 bytes per voxel and 4 per pixel at {STREAM_TBPS} TB/s): fuse = {t['fuse'][0] / floor:.1f} x floor; "
            f"{steps / t['fuse'][0] / 1e9:.2f} G voxel-frames/s, {t['fuse'][0] / F * 1e3:.3f} ms per frame; against torch after one call from the "
            f"same state: observed sets {'equal' if same_seen else 'DIFFER'}, |D - D_torch| <= {d_max:.2e}, {w_diff} weights differ")
        for name, same in others.items():
            tv = t["fuse " + name]
            say(f"{'':>6s} variant {name}: {fmt(tv)}; / this build = {tv[0] / t['fuse'][0]:.3f}; after one call from the same state its "
                f"bits are {'the same' if same else 'DIFFERENT'}")
        out_rows.append(dict(n=n, per_frame=per_frame, frames=F, height=H, width=Wd, fuse_ms=t["fuse"][0] * 1e3,
                             variants_ms={name: t["fuse " + name][0] * 1e3 for name in others}, torch_ms=t["torch"][0] * 1e3,
                             copy_ms=t["copy"][0] * 1e3, floor_ms=floor * 1e3, observed=observed, same_seen=same_seen, d_max=d_max,
                             w_diff=w_diff))
        del D, W, D2, W2, D0, W0, pts, depth
        torch.cuda.empty_cache()

    # ---- the sampler, untouched: this build against the parent's, side by side
    n, V, F = (64, 689, 16) if args.quick else (256, 6890, 256)
    dims, spacing, origin = (n, n, n), (2.0 / n,) * 3, (-1.0, -1.0, 1.5)
    vol = torch.rand((n, n, n), device="cuda") - 0.5
    points = (torch.rand((F, V, 3), device="cuda") * 1.9 + torch.tensor([-0.95, -0.95, 1.55], device="cuda")).contiguous()
    libs = {"this build": api.load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    outs, fns = {}, {}
    for name, lib in libs.items():
        lib.bodyfit_volume_create.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_double)] * 2 + [ctypes.POINTER(ctypes.c_void_p)]
        lib.bodyfit_volume_sample_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                                     ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_void_p] * 5
        h = ctypes.c_void_p()
        o, s = (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*spacing)
        assert lib.bodyfit_volume_create(0, n, n, n, o, s, ctypes.byref(h)) == 0
        value = torch.empty((F, V), device="cuda")
        valid = torch.empty((F, V), dtype=torch.uint8, device="cuda")
        grad = torch.empty((F, V, 3), device="cuda")
        outs[name] = (value, valid, grad)

        def sample(lib=lib, h=h, value=value, valid=valid, grad=grad):
            assert lib.bodyfit_volume_sample_device(h, points.data_ptr(), 3 * V, V, F, vol.data_ptr(), 0, None, value.data_ptr(),
                                                    valid.data_ptr(), grad.data_ptr(), stream) == 0
        fns[name] = sample
    t = alternate(torch, fns, args.brackets)
    text = f"sample_volume's kernel with the gradient, {n}^3 shared, F={F} x {V} points: " + "  ".join(f"{k} {fmt(v)}" for k, v in t.items())
    if "parent" in t:
        same = all(bool((a.view(torch.int32) == b.view(torch.int32)).all()) if a.dtype == torch.float32 else bool((a == b).all())
                   for a, b in zip(outs["this build"], outs["parent"]))
        text += f"; this build / parent = {t['this build'][0] / t['parent'][0]:.3f}; outputs {'bit-identical' if same else 'DIFFER'}"
    say(text)
    out_rows.append(dict(sampler={k: v[0] * 1e3 for k, v in t.items()}))
    lines.append("# json: " + json.dumps(out_rows))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
