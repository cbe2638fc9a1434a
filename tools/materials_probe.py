"""What a material edit costs against the re-creation it replaces, on S-bath at detail 160 (0.59 M triangles, bench configuration
c4) and detail 420 (4.1 M, c5).

update_ms: device time of mcpt_update_materials (HIP events on the context's stream, mcpt_material_info::last_ms), median of 20 after 3 warm-ups,
alternating between two looks: the scene's own materials, and one in which the ceramic fixtures glow (hundreds of thousands of faces join the
light list, interleaved with the window in face order), the wood turns into a mirror and the window dims.  rebuild_ms: bvh_build_ms + upload_ms
of a fresh MCPT_FLAG_GPU_BVH_BUILD context of the edited scene created in the same process -- the faster builder, and only part of what
mcpt_create costs.

One process per scene (--detail N measures one and prints its JSON line), each under its own time limit; a failure ends the run.  Not part of
bench.py.

    python tools/materials_probe.py [--out profiles/materials_probe.json]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DETAILS = (160, 420)
LIMIT_S = {160: 300, 420: 900}
WOOD, CERAMIC, WINDOW = 2, 5, 7


def measure(detail):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("materials_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=detail, tex_size=64)
    edited = list(scene.materials)
    edited[CERAMIC] = dataclasses.replace(edited[CERAMIC], radiance=(0.6, 0.5, 0.4))
    edited[WOOD] = dataclasses.replace(edited[WOOD], ns=10000.0)
    edited[WINDOW] = dataclasses.replace(edited[WINDOW], radiance=(5.0, 4.6, 4.0))
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_GPU_BVH_BUILD)
    lights0 = int(R.info().n_lights)
    ms = []
    for i in range(23):
        R.update_materials(edited if i % 2 == 0 else scene.materials)
        ms.append(R.material_info().last_ms)
    ms = sorted(ms[3:])
    R.update_materials(edited)
    lights1 = int(R.material_info().n_lights)
    F = pkg.Renderer(pkg.scenes.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, scene.face, edited, scene.camera, dict(scene.meta)),
                     max_depth=6, flags=pkg.FLAG_GPU_BVH_BUILD)
    fi = F.info()
    assert int(fi.n_lights) == lights1
    R.close(); F.close()
    upd = statistics.median(ms); rebuild = fi.bvh_build_ms + fi.upload_ms
    return {"detail": detail, "n_tris": int(fi.n_tris), "n_lights_before": lights0, "n_lights_after": lights1, "update_ms": round(upd, 4),
            "update_ms_min": round(ms[0], 4), "update_ms_max": round(ms[-1], 4), "rebuild_ms": round(rebuild, 2), "bvh_build_ms": round(fi.bvh_build_ms, 2),
            "upload_ms": round(fi.upload_ms, 2), "update_over_rebuild": round(upd / rebuild, 6)}


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
            raise SystemExit("materials_probe: detail %d failed (exit %d)" % (d, p.returncode))
        runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "materials_probe", "scene": "S-bath 640x360, ceramic made emissive, wood made a mirror, window dimmed; and back", "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
