"""What mcpt_rebuild_trees costs, on S-bath at detail 160 (0.59 M triangles, bench configuration c4) and detail 420 (4.1 M, c5)
with the fixture displacement of tools/refit_probe.py, for both builders.

Per scene and builder, on one live context: update to the displaced / the original positions in turn, rebuild, read mcpt_rebuild_info -- last_ms
(wall, entry to return), last_build_ms (the tree construction), last_device_ms (HIP events: the bounds kernel, the permutation and the light
kernel) -- median of REPS calls after one warm-up.  device_gb_s: the bytes those kernels must move (per triangle: bounds 124 B read and written, 196 B
with the host builder's fp64 records; permutation 276 B read + 4 B of index + 276 B written) over last_device_ms.  create_ms: wall time of
constructing a fresh Renderer of the displaced scene with the same flags in the same process, median of 3; create_build_ms / create_upload_ms:
its mcpt_scene_info.  wide_area_ratio_before: what the refit had left the tree at.

One process per scene and builder (--detail N --builder B measures one and prints its JSON line), each under its own time limit; a failure ends
the run.  Not part of bench.py.

    python tools/rebuild_probe.py [--out profiles/rebuild_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DETAILS = (160, 420)
BUILDERS = ("device", "host")
LIMIT_S = {160: 240, 420: 400}
REPS = 5


def measure(detail, builder):
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from refit_probe import displaced
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("rebuild_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=detail, tex_size=64)
    moved = displaced(pkg, np, scene)
    fl = pkg.FLAG_DYNAMIC | (pkg.FLAG_GPU_BVH_BUILD if builder == "device" else 0)
    R = pkg.Renderer(scene, max_depth=6, flags=fl)
    n = int(R.info().n_tris)
    rows = []
    for i in range(REPS + 1):
        R.update_vertices(moved.vertex if i % 2 == 0 else scene.vertex)
        R.rebuild()
        rows.append(R.rebuild_info().as_dict())
    R.validate_trees()
    R.close()
    rows = rows[1:]
    create = []
    for i in range(3):
        t0 = time.perf_counter()
        F = pkg.Renderer(moved, max_depth=6, flags=fl)
        create.append(1e3 * (time.perf_counter() - t0))
        fi = F.info()
        F.close()
    med = lambda k: statistics.median(r[k] for r in rows)
    dev_ms = med("last_device_ms")
    dev_bytes = n * ((196 if builder == "host" else 124) + 556)
    return {"detail": detail, "builder": builder, "n_tris": n, "last_ms": round(med("last_ms"), 2), "last_ms_min": round(min(r["last_ms"] for r in rows), 2),
            "last_ms_max": round(max(r["last_ms"] for r in rows), 2), "last_build_ms": round(med("last_build_ms"), 2), "last_device_ms": round(dev_ms, 4),
            "device_gb_s": round(dev_bytes / (dev_ms * 1e-3) / 1e9, 1), "wide_area_ratio_before": round(rows[-1]["area_ratio_before"], 5),
            "create_ms": round(statistics.median(create), 2), "create_build_ms": round(fi.bvh_build_ms, 2), "create_upload_ms": round(fi.upload_ms, 2),
            "rebuild_over_create": round(med("last_ms") / statistics.median(create), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--detail", type=int, default=0, help="measure this one scene in this process")
    ap.add_argument("--builder", choices=BUILDERS, default="device")
    a = ap.parse_args()
    if a.detail:
        print(json.dumps(measure(a.detail, a.builder)))
        return
    runs = []
    for d in DETAILS:                                                     # a fresh child process per scene and builder; the first failure ends the run
        for b in BUILDERS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--detail", str(d), "--builder", b], capture_output=True, text=True, timeout=LIMIT_S[d])
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit("rebuild_probe: detail %d, %s builder failed (exit %d)" % (d, b, p.returncode))
            runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
            print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "rebuild_probe", "scene": "S-bath 640x360 depth 6, fixtures displaced by 0.02 sin(.)", "reps": REPS, "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
