"""What bending a part costs by bones on the device against the route it replaces, on S-bath at detail 160 (0.59 M triangles,
bench configuration c4) and detail 420 (4.1 M, c5): the fixtures (the tessellated spheres) skinned to two bones by their height, the upper bone
turned a little further about z through their centroid every frame; everything else on bone 0.

Per scene, in one process, medians of 20 after 3 warm-ups, the two routes alternating frame by frame:
  skin_wall_ms / skin_device_ms: mcpt_update_skin -- host clock around the call plus a sync / HIP events on the context's stream
      (mcpt_update_info::last_update_ms: the table's copy, the two skinning kernels and the refit); skin_part_ms: the copy and the two kernels
      alone (mcpt_skin_info::last_ms);
  vertices_wall_ms / vertices_device_ms: the same two figures of mcpt_update_vertices fed the identical arrays (its events span the two copies out
      of pinned memory and the refit; the memcpy into pinned memory is host time and shows in the wall figure only);
  host_arrays_ms: what the caller of the old route spends forming those arrays in numpy (the restatement of the kernels, tests/skin_ref.py).
The baseline is mcpt_update_vertices as it is: this feature does not touch it.  The ratios go into the JSON, not into an assertion.

One process per scene (--detail N measures one and prints its JSON line), each under its own time limit; a failure ends the run.  Not part of
bench.py.

    python tools/skin_probe.py [--out profiles/skin_probe.json]
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

DETAILS = (160, 420)
LIMIT_S = {160: 300, 420: 900}
WARM, TIMED = 3, 20


def measure(detail):
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from tests import skin_ref as S, transform_ref as T
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("skin_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=detail, tex_size=64)
    part = np.isin(scene.face[:, 0, 3], (5, 6))                                                  # ceramic and chrome
    vi = np.unique(scene.face[part][:, :, 0])
    y = scene.vertex[vi, 1]; w = (y - y.min()) / (y.max() - y.min())
    vb, vw = S.single(np.zeros(scene.vertex.shape[0], int))
    vb[vi, 0] = 1; vb[vi, 1] = 2; vw[vi, 0] = 1.0 - w; vw[vi, 1] = w
    nb, nw = pkg.skin_normals_from_faces(scene, vb, vw)
    pivot = scene.vertex[vi].mean(0)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_skin(vb, vw, nb, nw, 3)
    R.sync()
    keys = ("skin_wall_ms", "skin_device_ms", "skin_part_ms", "vertices_wall_ms", "vertices_device_ms", "host_arrays_ms")
    runs = {k: [] for k in keys}
    for i in range(WARM + TIMED):
        m = np.stack([T.identity(1)[0], T.identity(1)[0], T.about(T.rotation((0, 0, 1), 0.25 * (i + 1)), pivot)])
        t0 = time.perf_counter()
        v = S.skin_vertices(scene.vertex, vb, vw, m); n = S.skin_normals(scene.normal, nb, nw, m)
        t1 = time.perf_counter()
        R.update_skin(m); R.sync()
        t2 = time.perf_counter()
        sk_dev = R.update_info().last_update_ms; sk_part = R.skin_info().last_ms
        t3 = time.perf_counter()
        R.update_vertices(v, n); R.sync()
        t4 = time.perf_counter()
        up_dev = R.update_info().last_update_ms
        for k, x in zip(keys, ((t2 - t1) * 1e3, sk_dev, sk_part, (t4 - t3) * 1e3, up_dev, (t1 - t0) * 1e3)):
            runs[k].append(x)
    R.validate_trees()
    ratio = R.update_info().wide_area_ratio
    info = R.info()
    R.close()
    out = {"detail": detail, "n_tris": int(info.n_tris), "n_vertex": int(scene.vertex.shape[0]), "n_normal": int(scene.normal.shape[0]),
           "skinned_vertices": int(vi.size), "bytes_old_route": 24 * int(scene.vertex.shape[0] + scene.normal.shape[0]), "bytes_new_route": 96 * 3}
    for k in keys:
        x = sorted(runs[k][WARM:])
        out[k] = round(statistics.median(x), 4); out[k + "_min"] = round(x[0], 4); out[k + "_max"] = round(x[-1], 4)
    out["device_ratio_skin_over_vertices"] = round(out["skin_device_ms"] / out["vertices_device_ms"], 4)
    out["wall_ratio_skin_over_vertices_plus_host"] = round(out["skin_wall_ms"] / (out["vertices_wall_ms"] + out["host_arrays_ms"]), 4)
    out["wide_area_ratio"] = round(ratio, 5)
    return out


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
            raise SystemExit("skin_probe: detail %d failed (exit %d)" % (d, p.returncode))
        runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "skin_probe", "scene": "S-bath 640x360, the fixtures skinned to two bones by height, the upper bone turned 0.25 degrees further per frame; medians of %d after %d" % (TIMED, WARM),
           "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
