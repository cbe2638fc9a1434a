"""What skinning with dual quaternions costs on the device against linear blending, on S-bath at detail 160 (0.59 M triangles,
bench configuration c4): the fixtures (the tessellated spheres) twist about y between two bones by their height, a third bone holds the room.

In one process, on ONE context, medians of 20 after 3 warm-ups, the three routes alternating frame by frame with the identical rigid bones:
  dq_device_ms / dq_skin_ms: mcpt_update_skin in MCPT_SKIN_DUAL_QUATERNION mode -- HIP events on the context's stream
      (mcpt_update_info::last_update_ms: the table's copy, the two kernels and the refit) / the skinning part alone (mcpt_skin_info::last_ms);
  linear_device_ms / linear_skin_ms: the same two figures in MCPT_SKIN_LINEAR mode;
  arrays_device_ms: mcpt_update_vertices fed the arrays the dual-quaternion route computes (its events span the two copies out of pinned
      memory and the refit) -- the route both replace;
  mode_ms: mcpt_set_skin_mode itself, host clock (a synchronisation and the table's allocation or release) -- paid once per scene, here
      twice per frame because the mode alternates.
The dual-quaternion kernels gather 64 B per bone where the linear ones gather 96 B, and pay eight divisions and a root per vertex.  The ratios
go into the JSON, not into an assertion.  Not part of bench.py.

    python tools/skin_dq_probe.py [--out profiles/skin_dq_probe.json]
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


def measure():
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from tests import skin_dq_ref as D, skin_ref as S, transform_ref as T
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("skin_dq_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.bathroom_stress(640, 360, detail=DETAIL, tex_size=64)
    part = np.isin(scene.face[:, 0, 3], (5, 6))
    vi = np.unique(scene.face[part][:, :, 0])
    y = scene.vertex[vi, 1]; w = (y - y.min()) / (y.max() - y.min())
    vb, vw = S.single(np.zeros(scene.vertex.shape[0], int))
    vb[vi, 0] = 1; vb[vi, 1] = 2; vw[vi, 0] = 1.0 - w; vw[vi, 1] = w
    nb, nw = pkg.skin_normals_from_faces(scene, vb, vw)
    pivot = scene.vertex[vi].mean(0)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.set_vertex_skin(vb, vw, nb, nw, 3)
    R.sync()
    keys = ("dq_device_ms", "dq_skin_ms", "linear_device_ms", "linear_skin_ms", "arrays_device_ms", "mode_ms")
    runs = {k: [] for k in keys}
    for i in range(WARM + TIMED):
        m = np.stack([T.identity(1)[0], T.identity(1)[0], T.about(T.rotation((0, 1, 0), 7.0 * (i + 1)), pivot)])
        v, n = D.skin_vertices(scene.vertex, vb, vw, m), D.skin_normals(scene.normal, nb, nw, m)
        t0 = time.perf_counter()
        R.set_skin_mode(pkg.SKIN_DUAL_QUATERNION)
        t1 = time.perf_counter()
        R.update_skin(m)
        dq_dev = R.update_info().last_update_ms; dq_skin = R.skin_info().last_ms
        if i == 0:                                                            # the restatement's arrays, bit for bit
            gv, gn = R.vertices()
            assert np.array_equal(gv.view(np.uint64), v.view(np.uint64)) and np.array_equal(gn.view(np.uint64), n.view(np.uint64))
        t2 = time.perf_counter()
        R.set_skin_mode(pkg.SKIN_LINEAR)
        t3 = time.perf_counter()
        R.update_skin(m)
        ln_dev = R.update_info().last_update_ms; ln_skin = R.skin_info().last_ms
        R.update_vertices(v, n)
        ar_dev = R.update_info().last_update_ms
        for k, x in zip(keys, (dq_dev, dq_skin, ln_dev, ln_skin, ar_dev, 0.5e3 * ((t1 - t0) + (t3 - t2)))):
            runs[k].append(x)
    R.validate_trees()
    info = R.info()
    R.close()
    out = {"tool": "skin_dq_probe", "scene": "S-bath 640x360 detail %d, the fixtures twisted about y between two bones by their height; one context, "
                                             "the three routes alternating, medians of %d after %d" % (DETAIL, TIMED, WARM),
           "n_tris": int(info.n_tris), "n_vertex": int(scene.vertex.shape[0]), "n_normal": int(scene.normal.shape[0]), "n_bones": 3,
           "blended_vertices": int(((vw[:, 0] > 0) & (vw[:, 1] > 0)).sum()), "table_bytes_dq": 64 * 3, "table_bytes_linear": 96 * 3,
           "bytes_arrays_route": 24 * int(scene.vertex.shape[0] + scene.normal.shape[0])}
    for k in keys:
        x = sorted(runs[k][WARM:])
        out[k] = round(statistics.median(x), 4); out[k + "_min"] = round(x[0], 4); out[k + "_max"] = round(x[-1], 4)
    out["device_ratio_dq_over_linear"] = round(out["dq_device_ms"] / out["linear_device_ms"], 4)
    out["skin_ratio_dq_over_linear"] = round(out["dq_skin_ms"] / out["linear_skin_ms"], 4)
    out["device_ratio_dq_over_arrays"] = round(out["dq_device_ms"] / out["arrays_device_ms"], 4)
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
