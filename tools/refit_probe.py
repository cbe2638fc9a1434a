"""What a scene update costs against the rebuild it replaces, on S-bath at detail 160 (0.59 M triangles, bench configuration c4)
and detail 420 (4.1 M, c5) with a smooth displacement of the fixtures (the tessellated spheres).

update_ms: device time of mcpt_update_vertices (HIP events on the context's stream, mcpt_update_info::last_update_ms), median of 20 after 3
warm-ups, alternating between the displaced and the original positions.  rebuild_ms: bvh_build_ms + upload_ms of a fresh MCPT_FLAG_GPU_BVH_BUILD
context of the displaced scene created in the same process -- the faster builder, and only part of what mcpt_create costs.  mray_s_*: a 64-spp
depth-6 render at 640x360 on the refitted context R and on the fresh one F: what the refitted tree costs in traversal for this deformation.

One process per scene (--detail N measures one and prints its JSON line), each under its own time limit; a failure ends the run.  Not part of
bench.py.

    python tools/refit_probe.py [--out profiles/refit_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DETAILS = (160, 420)
LIMIT_S = {160: 300, 420: 900}


def displaced(pkg, np, scene):
    fixtures = np.isin(scene.face[:, 0, 3], (5, 6))                      # ceramic and chrome
    vi = np.unique(scene.face[fixtures][:, :, 0])
    v = scene.vertex.copy()
    p = v[vi]
    v[vi] = p + 0.02 * np.stack([np.sin(9.0 * p[:, 1]), np.sin(7.0 * p[:, 2]), np.sin(8.0 * p[:, 0])], -1)
    return pkg.scenes.SceneData(scene.name, v, scene.normal, scene.texcoord, scene.face, scene.materials, scene.camera, dict(scene.meta))


def mray_s(r, spp):
    r.clear(); r.reset_counters()
    r.render(spp, seed=3)
    c = r.counters()
    return c.rays / (c.kernel_ms_total * 1e-3) / 1e6


def measure(detail):
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("refit_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=detail, tex_size=64)
    moved = displaced(pkg, np, scene)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    ms = []
    for i in range(23):
        R.update_vertices(moved.vertex if i % 2 == 0 else scene.vertex)
        ms.append(R.update_info().last_update_ms)
    ms = sorted(ms[3:])
    R.update_vertices(moved.vertex)
    R.validate_trees()
    ui = R.update_info()
    F = pkg.Renderer(moved, max_depth=6, flags=pkg.FLAG_GPU_BVH_BUILD)
    fi = F.info()
    mray_s(R, 8); mray_s(F, 8)                                           # warm-up: pools allocated
    mr = [mray_s(R, 64) for _ in range(3)]; mf = [mray_s(F, 64) for _ in range(3)]
    R.close(); F.close()
    upd = statistics.median(ms); rebuild = fi.bvh_build_ms + fi.upload_ms
    return {"detail": detail, "n_tris": int(fi.n_tris), "update_ms": round(upd, 4), "update_ms_min": round(ms[0], 4), "update_ms_max": round(ms[-1], 4),
            "rebuild_ms": round(rebuild, 2), "bvh_build_ms": round(fi.bvh_build_ms, 2), "upload_ms": round(fi.upload_ms, 2),
            "update_over_rebuild": round(upd / rebuild, 6), "wide_area_ratio": round(ui.wide_area_ratio, 5),
            "mray_s_refitted": round(statistics.median(mr), 1), "mray_s_refitted_runs": [round(x, 1) for x in mr],
            "mray_s_fresh": round(statistics.median(mf), 1), "mray_s_fresh_runs": [round(x, 1) for x in mf]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--detail", type=int, default=0, help="measure this one scene in this process")
    a = ap.parse_args()
    if a.detail:
        print(json.dumps(measure(a.detail)))
        return
    runs = []
    for d in DETAILS:                                                     # a fresh child process per scene; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--detail", str(d)], capture_output=True, text=True, timeout=LIMIT_S[d])
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit("refit_probe: detail %d failed (exit %d)" % (d, p.returncode))
        runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "refit_probe", "scene": "S-bath 640x360 depth 6, fixtures displaced by 0.02 sin(.)", "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
