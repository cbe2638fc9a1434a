"""Timing of temporal reprojection on S-cornell at 800x800 and 3840x2160; prints one JSON line.

call_ms: device time of a whole mcpt_set_camera_reproject call (mcpt_reproject_info::last_ms: HIP events around its stream work -- the film
copy, the feature render of the new view at spp 4, the counter fill and rp_reproject_kernel), the camera alternating between two views 2
degrees apart, median of 20 after 3 warm-ups.  features_ms: mcpt_render_features alone at spp 4, bracketed by device events on a torch side
stream lent to the context.  kernel_ms: rp_reproject_kernel alone -- the ABI has no asynchronous entry point for it, so it comes from a kernel
trace of this very tool:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/reproject_probe.py --out FILE
    python tools/reproject_probe.py --merge FILE --kernel-trace DIR/.../*_kernel_trace.csv        (no GPU needed)

Bytes are the call's compulsory HBM traffic per pixel: new features written by their kernel and read by this one (32), old features read (32),
old film copied (16 read + 16 written) and read (16), film written (16).  The issue's 96 B per pixel are the kernel's own.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec (MI355X_MICROARCH: 6.29 TB/s measured for a float4 copy)
KERNEL_BYTES_PER_PIXEL = 96
SIZES = [(800, 800), (3840, 2160)]
WARMUP, RUNS = 3, 20


def rotated(pkg, cam, degrees):
    k = [float(x) for x in cam.up]; n = math.sqrt(sum(x * x for x in k)); k = [x / n for x in k]
    v = [cam.eye[i] - cam.lookat[i] for i in range(3)]
    a = math.radians(degrees); ca, sa = math.cos(a), math.sin(a)
    kv = sum(k[i] * v[i] for i in range(3))
    kx = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    eye = tuple(cam.lookat[i] + v[i] * ca + kx[i] * sa + k[i] * kv * (1 - ca) for i in range(3))
    return pkg.scenes.Camera(eye, cam.lookat, cam.up, cam.fovy, cam.width, cam.height)


def measure(pkg, torch, w, h):
    scene = pkg.scenes.cornell_box(w, h)
    r = pkg.Renderer(scene, max_depth=8)
    s = torch.cuda.Stream()
    r.set_torch_stream(s)
    r.render(4, seed=7)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(s); fn(); e1.record(s); e1.synchronize()
        return e0.elapsed_time(e1)

    feat = [timed(lambda: r.render_features(spp=4, seed=7)) for _ in range(4)]
    views = [rotated(pkg, scene.camera, 2.0), scene.camera]
    call, reused = [], []
    for i in range(WARMUP + RUNS):
        r.reproject_camera(views[i % 2], feature_spp=4, feature_seed=7, max_history=32.0)
        info = r.reproject_info()
        call.append(info.last_ms); reused.append(info.pixels_reused)
    call = sorted(call[WARMUP:])
    n = w * h
    ms = statistics.median(call)
    r.sync(); r.close()
    return {
        "size": "%dx%d" % (w, h), "grid": [(w + 63) // 64 * 64, (h + 3) // 4 * 4],
        "features_ms_spp4": round(statistics.median(feat[1:]), 4),
        "call_ms": round(ms, 4), "call_ms_min": round(call[0], 4), "call_ms_max": round(call[-1], 4),
        "pixels_reused_share": round(reused[WARMUP] / n, 4),
        "kernel_bytes": KERNEL_BYTES_PER_PIXEL * n, "kernel_hbm_floor_ms": round(KERNEL_BYTES_PER_PIXEL * n / HBM_PEAK * 1e3, 4),
    }


def merge_kernel_trace(res, path):
    """Per size the median duration of the rp_reproject_kernel dispatches of that grid in a rocprofv3 kernel trace (warm-ups dropped)."""
    by_grid = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "rp_reproject_kernel" not in row.get("Kernel_Name", ""):
                continue
            key = (int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]))
            by_grid.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    for run in res["runs"]:
        d = [ms for _, ms in sorted(by_grid.get(tuple(run["grid"]), []))][WARMUP:]
        if d:
            ms = statistics.median(d)
            run["kernel_ms"] = round(ms, 4); run["kernel_ms_min"] = round(min(d), 4); run["kernel_ms_max"] = round(max(d), 4); run["kernel_dispatches"] = len(d)
            run["kernel_achieved_GBps"] = round(run["kernel_bytes"] / (ms * 1e-3) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None, help="a result file of an earlier run: add kernel_ms from --kernel-trace and print it")
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            res = json.loads(f.readline())
        res = merge_kernel_trace(res, a.kernel_trace)
    else:
        import torch
        import __graft_entry__ as ge
        pkg = ge.load_package()
        if not torch.cuda.is_available():
            raise SystemExit("reproject_probe: no GPU (timings are only measured on the device)")
        res = {"tool": "reproject_probe", "scene": "S-cornell depth 8, 4 spp film, views 2 degrees apart, max_history 32", "device": torch.cuda.get_device_name(0),
               "runs": [measure(pkg, torch, w, h) for w, h in SIZES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
