"""Times of the surface extraction (bodyfit_volume_surface_count_device / _emit_device, k_surface_extract.hip) on
  tsdf 256^3      the shared 256^3 TSDF of tools/tsdf_bench.py's scene (64 depth maps of 640 x 480 fused; with its weight volume),
  per frame 128^3 64 per-frame 128^3 TSDFs of the same scene in one call,
  body 128^3      volume.voxelize_sdf of a posed synthetic body at 128^3 (no weight volume, no dead voxels).
Timed with the protocol of tools/tsdf_bench.py (a warm-up, then --brackets brackets of back-to-back calls, host clock around work
that ends in a device synchronise; median [min .. max]; the alternatives ALTERNATE bracket by bracket):
  count      the counting entry: k_mc_classify, k_mc_count, k_mc_scan, k_mc_offsets (four launches),
  emit       the emitting entry: k_mc_emit,
  copy       a plain copy of the volume (and of the weight volume where there is one) by torch: the byte floor of ONE pass that
             reads it; classify reads the volume once and emit reads it only at the crossed edges,
  torch      a torch composition of the COUNT pass only: eight shifted comparisons, the table's triangle counts looked up, the
             crossed owned edges with a live cell around them, and two cumsums: no positions, no faces.
The split of `count` into its kernels needs the device's own clock: --trace-case NAME runs that case's two entries 20 times and
nothing else, to be run under `rocprofv3 --kernel-trace --stats --output-format csv`, and --stats NAME=CSV (repeatable) takes such a run's
kernel_stats.csv into the report.  Then sample_volume's and integrate_tsdf's kernels from this build and, with --parent-lib,
from a library built from the parent commit, alternated: the same bits and the same time are what is to be seen.
Nothing is asserted; every comparison is printed whichever way it falls.
Usage: python3 tools/extract_bench.py [--brackets 5] [--parent-lib PATH] [--stats NAME=CSV ...] [--trace-case NAME] [--quick]
       [--out profiles/extract_bench.txt]"""
import argparse
import csv
import ctypes
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tsdf_bench import STREAM_TBPS, alternate, cameras  # noqa: E402
import gen_mc_table  # noqa: E402

CASES = ["tsdf", "per_frame", "body"]


def make_case(name, quick, torch, api, volume, synth, tl):
    """(label, vol [n, n, n] or [F, n, n, n], weight or None, min_weight, origin, spacing)"""
    rng = np.random.default_rng(5)
    big, small = (64, 32) if quick else (256, 128)
    if name in ("tsdf", "per_frame"):
        n, F = (big, 64) if name == "tsdf" else (small, 64)
        if quick:
            F = 4
        H, Wd, fx = (48, 64, 52.5) if quick else (480, 640, 525.0)
        spacing, origin = (2.0 / n,) * 3, (-1.0 + 1.0 / n, -1.0 + 1.0 / n, 1.5 + 1.0 / n)
        intr = (fx, fx, 0.5 * (Wd - 1), 0.5 * (H - 1))
        pose = torch.tensor(cameras(F, np.array([0.0, 0.0, 2.5]), rng), device="cuda")
        ii = torch.linspace(0.0, 1.0, H, device="cuda")[:, None]
        jj = torch.linspace(0.0, 1.0, Wd, device="cuda")[None, :]
        depth = torch.stack([2.5 + 0.5 * torch.sin(3.0 * jj + 0.1 * f) * torch.cos(2.0 * ii) for f in range(F)]).float().contiguous()
        depth[:, : H // 16, : Wd // 16] = 0.0
        D, W = volume.integrate_tsdf(depth, intr, origin, spacing, (n, n, n), 0.04, pose=pose, z_near=0.1, max_weight=64.0,
                                     per_frame=name == "per_frame")
        label = f"tsdf {n}^3, {F} maps fused" if name == "tsdf" else f"{F} per-frame tsdf {n}^3"
        return label, D, W, 1.0, origin, spacing
    n = small
    m = synth.make_model(0)
    seq = synth.make_sequence(m, 1, seed=4)
    layer = tl.SMPLLayer(api.Model(m), R0=seq.R0.reshape(1, 3, 3))
    with torch.no_grad():
        verts = layer(torch.tensor(seq.gt_params, device="cuda"), torch.tensor(seq.gt_beta, device="cuda"))[0]
    lo, hi = verts[0].min(dim=0).values.cpu().numpy().astype(np.float64), verts[0].max(dim=0).values.cpu().numpy().astype(np.float64)
    origin = tuple(lo - 0.1)
    spacing = tuple((hi - lo + 0.2) / (n - 1))
    sdf = volume.voxelize_sdf(verts, synth.make_faces(m), origin, spacing, (n, n, n))
    return f"voxelize_sdf body {n}^3", sdf, None, 0.0, origin, spacing


def torch_count(torch, vol, weight, min_weight, iso, n_tri):
    """the COUNT pass composed in torch on [F, nz, ny, nx]: (vertex offsets, face offsets) exclusive over voxels and cells"""
    usable = torch.isfinite(vol)
    if weight is not None:
        usable &= weight >= min_weight
    inside = vol < iso
    F, nz, ny, nx = vol.shape
    live = torch.ones((F, nz - 1, ny - 1, nx - 1), dtype=torch.bool, device=vol.device)
    case = torch.zeros(live.shape, dtype=torch.int64, device=vol.device)
    for c in range(8):
        sl = (slice(None), slice(c >> 2 & 1, nz - 1 + (c >> 2 & 1)), slice(c >> 1 & 1, ny - 1 + (c >> 1 & 1)), slice(c & 1, nx - 1 + (c & 1)))
        live &= usable[sl]
        case |= inside[sl].long() << c
    tris = torch.where(live, n_tri[case], torch.zeros_like(case))
    L = torch.nn.functional.pad(live, (1, 1, 1, 1, 1, 1))
    cell = lambda dk, dj, di: L[:, 1 - dk:1 - dk + nz, 1 - dj:1 - dj + ny, 1 - di:1 - di + nx]
    around = [cell(0, 0, 0) | cell(0, 1, 0) | cell(1, 0, 0) | cell(1, 1, 0), cell(0, 0, 0) | cell(0, 0, 1) | cell(1, 0, 0) | cell(1, 0, 1),
              cell(0, 0, 0) | cell(0, 0, 1) | cell(0, 1, 0) | cell(0, 1, 1)]
    verts = torch.zeros(vol.shape, dtype=torch.int32, device=vol.device)
    for axis, dim in enumerate((3, 2, 1)):
        a, b = [slice(None)] * 4, [slice(None)] * 4
        a[dim], b[dim] = slice(0, -1), slice(1, None)
        flag = torch.zeros(vol.shape, dtype=torch.bool, device=vol.device)
        flag[tuple(a)] = usable[tuple(a)] & usable[tuple(b)] & (inside[tuple(a)] ^ inside[tuple(b)])
        verts += (flag & around[axis]).int()
    return torch.cumsum(verts.reshape(F, -1), dim=1), torch.cumsum(tris.reshape(F, -1), dim=1)


def read_stats(path):
    """{kernel: (calls, average ns)} of a rocprofv3 kernel_stats.csv, the k_mc_ kernels only"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            col = {key.lower(): value for key, value in row.items()}
            for k in ("k_mc_classify", "k_mc_count", "k_mc_scan", "k_mc_offsets", "k_mc_emit"):
                if k in col["name"]:
                    out[k] = (int(col["calls"]), float(col["averagens"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--stats", action="append", default=[], metavar="NAME=CSV")
    ap.add_argument("--trace-case", default=None, choices=CASES)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_bench.txt"))
    args = ap.parse_args()
    torch = importlib.import_module("torch")
    api = importlib.import_module("3dbodyanimation_amd.api")
    volume = importlib.import_module("3dbodyanimation_amd.torch_layer.volume")
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    synth = importlib.import_module("3dbodyanimation_amd.synth")
    if api.device_count() < 1:
        raise SystemExit("extract_bench needs a GPU: nothing here can be timed on the CPU")
    stream = torch.cuda.current_stream().cuda_stream
    fmt = lambda t: f"{t[0] * 1e3:9.3f} [{t[1] * 1e3:9.3f} .. {t[2] * 1e3:9.3f}] x{t[3]:<3d}"
    lines = [f"# extract_bench: brackets={args.brackets}; times in ms per call: median [min .. max] x calls per bracket; alternatives "
             f"alternate bracket by bracket" + ("; QUICK sizes: a rehearsal, not a measurement" if args.quick else "")]
    rows = []
    stats = {item.split("=", 1)[0]: read_stats(item.split("=", 1)[1]) for item in args.stats}
    n_tri = torch.tensor(gen_mc_table.table()[0].astype(np.int64), device="cuda")

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for name in CASES if args.trace_case is None else [args.trace_case]:
        label, vol, weight, min_weight, origin, spacing = make_case(name, args.quick, torch, api, volume, synth, tl)
        F = vol.shape[0] if vol.ndim == 4 else 1
        n = vol.shape[-1]
        handle = api.Volume(0, (n, n, n), origin, spacing)
        work = torch.empty(handle.surface_layout(F), dtype=torch.uint8, device="cuda")
        offsets = torch.zeros((2, F + 1), dtype=torch.int64, device="cuda")
        a = (vol.data_ptr(), weight.data_ptr() if weight is not None else None, n ** 3, F, 0.0, min_weight, work.data_ptr(),
             offsets.data_ptr())
        handle.surface_count_device(*a, stream=stream)
        n_verts, n_faces = (int(x) for x in offsets[:, F].tolist())
        verts = torch.empty((n_verts, 3), device="cuda")
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device="cuda")
        count = lambda: handle.surface_count_device(*a, stream=stream)
        emit = lambda: handle.surface_emit_device(*a, n_verts, n_faces, verts.data_ptr(), faces.data_ptr(), stream=stream)
        if args.trace_case is not None:
            for _ in range(20):
                count()
                emit()
            torch.cuda.synchronize()
            print(f"traced {label}: 20 x (count, emit); {n_verts} vertices, {n_faces} faces")
            return
        vol2 = torch.empty_like(vol)
        w2 = torch.empty_like(weight) if weight is not None else None

        def copy():
            vol2.copy_(vol)
            if weight is not None:
                w2.copy_(weight)

        v4, wt4 = vol.view(F, n, n, n), weight.view(F, n, n, n) if weight is not None else None
        chunk = max(1, (1 << 24) // n ** 3)                                      # (the composition's temporaries: 16 M voxels at a time)

        def composed():
            for f0 in range(0, F, chunk):
                torch_count(torch, v4[f0:f0 + chunk], None if wt4 is None else wt4[f0:f0 + chunk], min_weight, 0.0, n_tri)

        cv, cf = torch_count(torch, v4[:1], None if wt4 is None else wt4[:1], min_weight, 0.0, n_tri)
        agree = (int(cv[0, -1]) == int(offsets[0, 1]), int(cf[0, -1]) == int(offsets[1, 1]))
        t = alternate(torch, {"count": count, "emit": emit, "copy": copy, "torch": composed}, args.brackets)
        arrays = 2 if weight is not None else 1
        floor = F * n ** 3 * 4 * arrays / (STREAM_TBPS * 1e12)
        both = t["count"][0] + t["emit"][0]
        say(f"{label} ({F * n ** 3} voxels, {arrays} array(s) read; {n_verts} vertices, {n_faces} faces): count {fmt(t['count'])}  "
            f"emit {fmt(t['emit'])}  copy {fmt(t['copy'])}  torch (count only) {fmt(t['torch'])}")
        say(f"{'':>6s} count + emit = {both * 1e3:.3f} ms = {both / t['copy'][0]:.2f} x the copy"
            + (" (SLOWER THAN ONE COPY)" if both > t['copy'][0] else "")
            + f"; count / copy = {t['count'][0] / t['copy'][0]:.2f}; emit / copy = {t['emit'][0] / t['copy'][0]:.2f}; reading the arrays once at "
            f"{STREAM_TBPS} TB/s: {floor * 1e3:.4f} ms, count = {t['count'][0] / floor:.1f} x that; count / torch's count = "
            f"{t['count'][0] / t['torch'][0]:.4f}" + (" (THE KERNELS ARE SLOWER)" if t['count'][0] > t['torch'][0] else
                                                       f" ({t['torch'][0] / t['count'][0]:.0f} x)")
            + f"; torch's totals of volume 0 {'agree' if all(agree) else 'DIFFER'}; {F * n ** 3 / both / 1e9:.2f} G voxels/s")
        row = dict(case=name, voxels=F * n ** 3, n_verts=n_verts, n_faces=n_faces, count_ms=t["count"][0] * 1e3, emit_ms=t["emit"][0] * 1e3,
                   copy_ms=t["copy"][0] * 1e3, torch_count_ms=t["torch"][0] * 1e3, floor_ms=floor * 1e3, torch_agrees=all(agree))
        if name in stats:
            k = stats[name]
            say(f"{'':>6s} per kernel, the device's clock (rocprofv3 --kernel-trace --stats over --trace-case {name}), us: "
                + ", ".join(f"{key} {k[key][1] / 1e3:.1f}" for key in sorted(k))
                + f"; count = classify + count {sum(k[x][1] for x in ('k_mc_classify', 'k_mc_count') if x in k) / 1e3:.1f}, scan = scan + "
                f"offsets {sum(k[x][1] for x in ('k_mc_scan', 'k_mc_offsets') if x in k) / 1e3:.1f}, emit {k.get('k_mc_emit', (0, 0.0))[1] / 1e3:.1f}")
            row["kernels_us"] = {key: v[1] / 1e3 for key, v in k.items()}
        rows.append(row)
        del vol2, w2, verts, faces, work, vol, weight, v4, wt4
        torch.cuda.empty_cache()

    # ---- the two older volume kernels, untouched: this build against the parent's, side by side
    n, V, F = (64, 689, 16) if args.quick else (256, 6890, 256)
    dims, spacing, origin = (n, n, n), (2.0 / n,) * 3, (-1.0 + 1.0 / n, -1.0 + 1.0 / n, 1.5 + 1.0 / n)
    vol = torch.rand((n, n, n), device="cuda") - 0.5
    points = (torch.rand((F, V, 3), device="cuda") * 1.9 + torch.tensor([-0.95, -0.95, 1.55], device="cuda")).contiguous()
    Fd = 4 if args.quick else 64
    H, Wd, fx = (48, 64, 52.5) if args.quick else (480, 640, 525.0)
    pose = torch.tensor(cameras(Fd, np.array([0.0, 0.0, 2.5]), np.random.default_rng(5)), device="cuda")
    depth = (2.5 + 0.5 * torch.rand((Fd, H, Wd), device="cuda")).contiguous()
    libs = {"this build": api.load_library()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    outs, fs, fi = {}, {}, {}
    for name, lib in libs.items():
        lib.bodyfit_volume_create.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_double)] * 2 + [ctypes.POINTER(ctypes.c_void_p)]
        lib.bodyfit_volume_sample_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                                     ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_void_p] * 5
        lib.bodyfit_volume_integrate_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_double,
                                                        ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_longlong, ctypes.c_void_p]
        h = ctypes.c_void_p()
        assert lib.bodyfit_volume_create(0, n, n, n, (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*spacing), ctypes.byref(h)) == 0
        value = torch.empty((F, V), device="cuda")
        valid = torch.empty((F, V), dtype=torch.uint8, device="cuda")
        grad = torch.empty((F, V, 3), device="cuda")
        D, W = torch.empty((n, n, n), device="cuda"), torch.empty((n, n, n), device="cuda")
        outs[name] = (value, valid, grad, D, W)
        k = (ctypes.c_double * 4)(fx, fx, 0.5 * (Wd - 1), 0.5 * (H - 1))

        def sample(lib=lib, h=h, value=value, valid=valid, grad=grad):
            assert lib.bodyfit_volume_sample_device(h, points.data_ptr(), 3 * V, V, F, vol.data_ptr(), 0, None, value.data_ptr(),
                                                    valid.data_ptr(), grad.data_ptr(), stream) == 0

        def integrate(lib=lib, h=h, D=D, W=W, k=k):
            assert lib.bodyfit_volume_integrate_device(h, depth.data_ptr(), H * Wd, H, Wd, Fd, k, pose.data_ptr(), 0.04, 0.1, 64.0, 1,
                                                       D.data_ptr(), W.data_ptr(), 0, stream) == 0
        fs[name], fi[name] = sample, integrate
    for what, fns, picks in (("k_vol_sample with the gradient", fs, (0, 1, 2)), (f"k_tsdf_integrate, {Fd} maps under reset", fi, (3, 4))):
        t = alternate(torch, fns, args.brackets)
        text = f"{what}, {n}^3: " + "  ".join(f"{k} {fmt(v)}" for k, v in t.items())
        if "parent" in t:
            same = all(outs["this build"][p].view(torch.uint8).reshape(-1).equal(outs["parent"][p].view(torch.uint8).reshape(-1)) for p in picks)
            spread = max((v[2] - v[1]) / v[0] for v in t.values())
            text += (f"; this build / parent = {t['this build'][0] / t['parent'][0]:.3f} (the brackets of one build spread over "
                     f"{100 * spread:.1f} % of its median); outputs {'bit-identical' if same else 'DIFFER'}")
        say(text)
        rows.append({what: {k: v[0] * 1e3 for k, v in t.items()}})
    lines.append("# json: " + json.dumps(rows))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
