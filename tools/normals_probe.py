"""What recomputing the smooth normals on the device costs against the route it replaces, on S-bath at detail 160 (0.59 M
triangles, bench configuration c4): the fixtures (the tessellated spheres) swell and lift, every normal record of the scene is recomputed.

In one process, on ONE context, medians of 20 after 3 warm-ups, the two routes alternating frame by frame:
  auto_wall_ms / auto_device_ms: mcpt_update_vertices(normal = NULL) with auto normals on -- host clock around the call plus a sync / HIP events
      on the context's stream (mcpt_update_info::last_update_ms: the vertices' copy, the normals kernel and the refit); auto_pass_ms: the
      kernel alone (mcpt_normals_info::last_ms);
  arrays_wall_ms / arrays_device_ms: the same two figures of mcpt_update_vertices fed the identical vertices plus the restated normals, with
      auto normals off (its events span the two copies out of pinned memory and the refit);
  host_normals_ms: what the caller of the old route spends forming those normals in numpy (tests/normals_ref.py, lists prepared once);
  set_ms: mcpt_set_auto_normals itself (the read-backs, the host's lists, their upload) -- paid once per scene, here once per frame because
      the feature is switched off for the old route's turn.
The baseline is mcpt_update_vertices as it is: this feature does not touch it.  The ratios go into the JSON, not into an assertion.  Not part
of bench.py.

    python tools/normals_probe.py [--out profiles/normals_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DETAIL = 160
WARM, TIMED = 3, 20


def poses(scene, np):
    """Two poses of the fixtures (ceramic and chrome): a swell about their centroid and a lift that grows with the height."""
    part = np.isin(scene.face[:, 0, 3], (5, 6))
    vi = np.unique(scene.face[part][:, :, 0])
    p = scene.vertex[vi]; c = p.mean(0)
    y = (p[:, 1] - p[:, 1].min()) / (p[:, 1].max() - p[:, 1].min())
    out = []
    for swell, lift in ((0.05, 0.5), (-0.04, 1.0)):
        v = scene.vertex.copy()
        v[vi] = p + swell * (p - c) + lift * np.stack([0.05 * y, 0.1 * y * y, np.zeros_like(y)], 1)
        out.append(v)
    return out


def measure():
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from tests import normals_ref as N
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("normals_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=DETAIL, tex_size=64)
    off, entry = N.per_record(scene.face, scene.normal.shape[0], scene.vertex, scene.normal)
    vs = poses(scene, np)
    t0 = time.perf_counter()
    ns = [N.apply(off, entry, v, scene.normal) for v in vs]
    host_ms = (time.perf_counter() - t0) * 1e3 / len(vs)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.sync()
    keys = ("auto_wall_ms", "auto_device_ms", "auto_pass_ms", "arrays_wall_ms", "arrays_device_ms", "set_ms")
    runs = {k: [] for k in keys}
    for i in range(WARM + TIMED):
        v, n = vs[i % 2], ns[i % 2]
        t0 = time.perf_counter()
        R.set_auto_normals()
        t1 = time.perf_counter()
        R.update_vertices(v, None); R.sync()
        t2 = time.perf_counter()
        a_dev = R.update_info().last_update_ms; a_pass = R.normals_info().last_ms
        if i == 0:                                                            # the lists were taken at the rest pose: the restatement's
            assert np.array_equal(R.vertices()[1].view(np.uint64), n.view(np.uint64))
        R.set_auto_normals(mode=pkg.NORMALS_OFF)
        t3 = time.perf_counter()
        R.update_vertices(v, n); R.sync()
        t4 = time.perf_counter()
        b_dev = R.update_info().last_update_ms
        for k, x in zip(keys, ((t2 - t1) * 1e3, a_dev, a_pass, (t4 - t3) * 1e3, b_dev, (t1 - t0) * 1e3)):
            runs[k].append(x)
    R.validate_trees()
    info = R.info()
    R.close()
    count = np.diff(off.astype(np.int64))
    out = {"tool": "normals_probe", "scene": "S-bath 640x360 detail %d, the fixtures swollen and lifted, every normal record recomputed; one context, "
                                             "the two routes alternating, medians of %d after %d" % (DETAIL, TIMED, WARM),
           "n_tris": int(info.n_tris), "n_vertex": int(scene.vertex.shape[0]), "n_normal": int(scene.normal.shape[0]), "records": int((count > 0).sum()),
           "entries": int(entry.shape[0]), "flipped_entries": int(entry[:, 3].sum()), "valence_median": float(np.median(count[count > 0])), "valence_max": int(count.max()),
           "bytes_old_route": 24 * int(scene.vertex.shape[0] + scene.normal.shape[0]), "bytes_new_route": 24 * int(scene.vertex.shape[0]),
           "list_bytes": 4 * (int(scene.normal.shape[0]) + 1) + 16 * int(entry.shape[0]), "host_normals_ms": round(host_ms, 3)}
    for k in keys:
        x = sorted(runs[k][WARM:])
        out[k] = round(statistics.median(x), 4); out[k + "_min"] = round(x[0], 4); out[k + "_max"] = round(x[-1], 4)
    out["device_ratio_auto_over_arrays"] = round(out["auto_device_ms"] / out["arrays_device_ms"], 4)
    out["wall_ratio_auto_over_arrays_plus_host"] = round(out["auto_wall_ms"] / (out["arrays_wall_ms"] + out["host_normals_ms"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
