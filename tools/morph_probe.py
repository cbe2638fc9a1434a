"""What morphing a part costs by weights on the device against the route it replaces, on S-bath at detail 160 (0.59 M triangles,
bench configuration c4) and detail 420 (4.1 M, c5): the fixtures (the tessellated spheres) under two targets -- a swell about their centroid over
all of their vertices, a lift that grows with the height over every second one -- with normal targets over the same records; and the same with
§18's two-bone height skin on top (morph, then skin).

Per scene, in one process, medians of 20 after 3 warm-ups, the three routes alternating frame by frame:
  morph_wall_ms / morph_device_ms: mcpt_update_morph -- host clock around the call plus a sync / HIP events on the context's stream
      (mcpt_update_info::last_update_ms: the weights' copy, the two morph kernels and the refit); morph_part_ms: the copy and the two kernels
      alone (mcpt_morph_info::last_ms);
  morph_skin_wall_ms / morph_skin_device_ms / morph_skin_part_ms: the same of mcpt_update_morph WITH bones (two more copies' worth: the table of
      matrices; four kernels);
  vertices_wall_ms / vertices_device_ms: the same two figures of mcpt_update_vertices fed the arrays the weights alone give (its events span the
      two copies out of pinned memory and the refit; the memcpy into pinned memory is host time and shows in the wall figure only);
  host_arrays_ms: what the caller of the old route spends forming those arrays in numpy (tests/morph_ref.py).
entries_per_touched_record_median / _max (vertices; the normals' lists have the same lengths): a wave runs as long as its most loaded lane, so
this is the skew the next reader prices a second code path with.  The baseline is mcpt_update_vertices as it is: this feature does not touch
it.  The ratios go into the JSON, not into an assertion.

One process per scene (--detail N measures one and prints its JSON line), each under its own time limit; a failure ends the run.  Not part of
bench.py.

    python tools/morph_probe.py [--out profiles/morph_probe.json]
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
    from tests import morph_ref as M, skin_ref as S, transform_ref as T
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("morph_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=detail, tex_size=64)
    part = np.isin(scene.face[:, 0, 3], (5, 6))                                                  # ceramic and chrome
    vi = np.unique(scene.face[part][:, :, 0]); ni = np.unique(scene.face[part][:, :, 1])
    p = scene.vertex[vi]; pivot = p.mean(0)
    y = (p[:, 1] - p[:, 1].min()) / (p[:, 1].max() - p[:, 1].min())
    lift = np.stack([0.05 * y, 0.1 * y * y, np.zeros_like(y)], 1)
    rng = np.random.default_rng(12)
    vt = [(vi, p - pivot), (vi[::2], lift[::2])]
    nt = [(ni, rng.uniform(-0.05, 0.05, (len(ni), 3))), (ni[::2], rng.uniform(-0.05, 0.05, (len(ni[::2]), 3)))]
    vb, vw = S.single(np.zeros(scene.vertex.shape[0], int))
    vb[vi, 0] = 1; vb[vi, 1] = 2; vw[vi, 0] = 1.0 - y; vw[vi, 1] = y
    nb, nw = pkg.skin_normals_from_faces(scene, vb, vw)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_morph(vt, nt)
    R.set_vertex_skin(vb, vw, nb, nw, 3)
    R.sync()
    keys = ("morph_wall_ms", "morph_device_ms", "morph_part_ms", "morph_skin_wall_ms", "morph_skin_device_ms", "morph_skin_part_ms",
            "vertices_wall_ms", "vertices_device_ms", "host_arrays_ms")
    runs = {k: [] for k in keys}
    for i in range(WARM + TIMED):
        w = np.array([0.004 * (i + 1), 0.03 * (i + 1)])
        m = np.stack([T.identity(1)[0], T.identity(1)[0], T.about(T.rotation((0, 0, 1), 0.25 * (i + 1)), pivot)])
        t0 = time.perf_counter()
        v = M.morph_vertices(scene.vertex, vt, w); n = M.morph_normals(scene.normal, nt, w)
        t1 = time.perf_counter()
        R.update_morph(w); R.sync()
        t2 = time.perf_counter()
        mo_dev = R.update_info().last_update_ms; mo_part = R.morph_info().last_ms
        t3 = time.perf_counter()
        R.update_morph(w, m); R.sync()
        t4 = time.perf_counter()
        ms_dev = R.update_info().last_update_ms; ms_part = R.morph_info().last_ms
        t5 = time.perf_counter()
        R.update_vertices(v, n); R.sync()
        t6 = time.perf_counter()
        up_dev = R.update_info().last_update_ms
        for k, x in zip(keys, ((t2 - t1) * 1e3, mo_dev, mo_part, (t4 - t3) * 1e3, ms_dev, ms_part, (t6 - t5) * 1e3, up_dev, (t1 - t0) * 1e3)):
            runs[k].append(x)
    R.validate_trees()
    ratio = R.update_info().wide_area_ratio
    info = R.info(); mi = R.morph_info()
    R.close()
    per = np.diff(M.per_record(vt, scene.vertex.shape[0])[0].astype(np.int64)); per = per[per > 0]
    out = {"detail": detail, "n_tris": int(info.n_tris), "n_vertex": int(scene.vertex.shape[0]), "n_normal": int(scene.normal.shape[0]),
           "morphed_vertices": int(vi.size), "vertex_entries": int(mi.vertex_entries), "normal_entries": int(mi.normal_entries),
           "entries_per_touched_record_median": float(np.median(per)), "entries_per_touched_record_max": int(per.max()),
           "bytes_old_route": 24 * int(scene.vertex.shape[0] + scene.normal.shape[0]), "bytes_new_route": 8 * 2, "bytes_new_route_with_bones": 8 * 2 + 96 * 3}
    for k in keys:
        x = sorted(runs[k][WARM:])
        out[k] = round(statistics.median(x), 4); out[k + "_min"] = round(x[0], 4); out[k + "_max"] = round(x[-1], 4)
    out["device_ratio_morph_over_vertices"] = round(out["morph_device_ms"] / out["vertices_device_ms"], 4)
    out["device_ratio_morph_skin_over_vertices"] = round(out["morph_skin_device_ms"] / out["vertices_device_ms"], 4)
    out["wall_ratio_morph_over_vertices_plus_host"] = round(out["morph_wall_ms"] / (out["vertices_wall_ms"] + out["host_arrays_ms"]), 4)
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
            raise SystemExit("morph_probe: detail %d failed (exit %d)" % (d, p.returncode))
        runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "morph_probe", "scene": "S-bath 640x360, the fixtures under two targets (a swell over all their vertices, a lift over every second one; normal targets over "
                                           "the same records), alone and in front of the two-bone height skin; medians of %d after %d" % (TIMED, WARM),
           "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
