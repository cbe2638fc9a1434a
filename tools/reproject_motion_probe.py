"""Timing of motion-vector reprojection on S-bath (bench configuration c4's scene, 0.59 M triangles) at 800x800 and 3840x2160;
prints one JSON line.

call_ms: device time of a whole mcpt_update_vertices_reproject call (mcpt_reproject_info::last_ms), the vertices alternating between the rest
pose and refit_probe's 0.02 sin(.) displacement of the fixtures, median of 20 after 3 warm-ups.  refit_ms: mcpt_update_info::last_update_ms of
the same calls (their refit part); plain_update_ms: the same of plain mcpt_update_vertices calls.  The two new kernels alone come from a kernel
trace of this very tool, in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/reproject_motion_probe.py --out FILE
    python tools/reproject_motion_probe.py --merge FILE --kernel-trace DIR/.../*_kernel_trace.csv        (no GPU needed)

Compulsory bytes per pixel: rp_reproject_motion_kernel reads the new features (32), the first-hit record (16), the old features (32, gathered)
and the old film (16, gathered) and writes the film (16): 112, plus per surface pixel one 24-B index record and six 24-B vertex / normal
records that neighbouring pixels share; rp_first_hit_kernel writes 16 and reads what its traversal touches.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12
MOTION_BYTES_PER_PIXEL, FIRST_HIT_BYTES_PER_PIXEL = 112, 16
SIZES = [(800, 800), (3840, 2160)]
WARMUP, RUNS = 3, 20
KERNELS = {"rp_first_hit_kernel": "first_hit", "rp_reproject_motion_kernel": "motion"}


def measure(pkg, np, w, h):
    from refit_probe import displaced
    scene = pkg.scenes.bathroom_stress(w, h, detail=160)
    moved = displaced(pkg, np, scene)
    r = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC)
    r.render(4, seed=7)
    poses = [moved.vertex, scene.vertex]
    plain = []
    for i in range(WARMUP + RUNS):
        r.update_vertices(poses[i % 2])
        plain.append(r.update_info().last_update_ms)
    call, refit, reused = [], [], []
    for i in range(WARMUP + RUNS):
        r.update_vertices_reproject(poses[i % 2], feature_spp=4, feature_seed=7, max_history=32.0)
        info = r.reproject_info()
        call.append(info.last_ms); reused.append(info.pixels_reused); refit.append(r.update_info().last_update_ms)
    n = w * h
    r.sync(); r.close()
    med = lambda a: round(statistics.median(sorted(a[WARMUP:])), 4)
    return {"size": "%dx%d" % (w, h), "pixels": n, "n_tris": int(scene.face.shape[0]),
            "call_ms": med(call), "call_ms_min": round(min(call[WARMUP:]), 4), "call_ms_max": round(max(call[WARMUP:]), 4),
            "refit_ms": med(refit), "plain_update_ms": med(plain), "pixels_reused_share": round(reused[WARMUP] / n, 4),
            "motion_bytes": MOTION_BYTES_PER_PIXEL * n, "motion_hbm_floor_ms": round(MOTION_BYTES_PER_PIXEL * n / HBM_PEAK * 1e3, 4),
            "first_hit_bytes_written": FIRST_HIT_BYTES_PER_PIXEL * n}


def merge_kernel_trace(res, path):
    """Per size the median duration of the two kernels' dispatches in a rocprofv3 kernel trace.  The dispatches come in the order of the runs:
    WARMUP + RUNS per size, warm-ups dropped."""
    rows = {k: [] for k in KERNELS}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row.get("Kernel_Name", ""):
                    rows[k].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    for k, name in KERNELS.items():
        d = [ms for _, ms in sorted(rows[k])]
        for j, run in enumerate(res["runs"]):
            part = d[j * (WARMUP + RUNS):(j + 1) * (WARMUP + RUNS)][WARMUP:]
            if part:
                ms = statistics.median(part)
                run[name + "_kernel_ms"] = round(ms, 4); run[name + "_kernel_ms_min"] = round(min(part), 4); run[name + "_kernel_ms_max"] = round(max(part), 4)
                run[name + "_dispatches"] = len(part)
                if name == "motion":
                    run["motion_achieved_GBps"] = round(run["motion_bytes"] / (ms * 1e-3) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None, help="a result file of an earlier run: add the kernels' durations from --kernel-trace and print it")
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            res = json.loads(f.readline())
        res = merge_kernel_trace(res, a.kernel_trace)
    else:
        import numpy as np
        import torch
        import __graft_entry__ as ge
        pkg = ge.load_package()
        if not torch.cuda.is_available():
            raise SystemExit("reproject_motion_probe: no GPU (timings are only measured on the device)")
        res = {"tool": "reproject_motion_probe", "scene": "S-bath detail 160, depth 6, 4 spp film, fixtures displaced by 0.02 sin(.), max_history 32",
               "device": torch.cuda.get_device_name(0), "runs": [measure(pkg, np, w, h) for w, h in SIZES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
