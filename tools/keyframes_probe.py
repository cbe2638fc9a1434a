"""What playing baked vertex animation from device-resident keyframes costs against the route it replaces, on S-cornell (1 249
vertices, the test scene) and on S-bath at detail 420 (2.04 M vertices, bench configuration c5).  The frames are synthetic: four of them, the
scene's vertices plus a per-frame sine, the scene's normals tilted per frame and normalised.

Per scene, in one process, per interpolation the frames uploaded once and then medians of 20 after 3 warm-ups, the new route and the old one
alternating frame by frame, every time between keyframes (u != 0):
  linear_part_ms / catmull_rom_part_ms: mcpt_keyframe_info::last_ms -- HIP events on the context's stream around the two kernels alone;
  linear_device_ms / catmull_rom_device_ms: mcpt_update_info::last_update_ms of the same call -- the kernels and the refit;
  vertices_device_ms: the same figure of mcpt_update_vertices fed the arrays the blend gives, recorded in the linear run (its events span the
      two copies out of pinned memory and the refit; the memcpy into pinned memory is host time and shows in vertices_wall_ms only);
  vertices_upload_ms: vertices_device_ms less the refit, the refit taken as linear_device_ms - linear_part_ms (the same kernels on the same
      arrays): the staged upload that the deforming part replaces;
  *_bytes: what the deforming part moves, 24 B x (taps + 1) per vertex and per normal, and *_gbps: that over the part's time, to set against
      the 8 TB/s HBM peak of an MI355X (6.3 TB/s is what a copy kernel reaches).
The ratios go into the JSON, not into an assertion.  One process per scene (--scene NAME measures one and prints its JSON line), each under its
own time limit; a failure ends the run.  Not part of bench.py.

    python tools/keyframes_probe.py [--out profiles/keyframes_probe.json]
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

SCENES = ("cornell", "c5")
LIMIT_S = {"cornell": 120, "c5": 420}
WARM, TIMED = 3, 20
N_FRAMES = 4
HBM_PEAK_GBPS = 8000.0


def measure(name):
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from tests import keyframes_ref as F
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("keyframes_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.cornell_box(64, 64, sphere_lon=48, sphere_lat=24) if name == "cornell" else pkg.scenes.bathroom_stress(640, 360, detail=420, tex_size=64)
    nv, nn = scene.vertex.shape[0], scene.normal.shape[0]
    p, q = scene.vertex, scene.normal
    vf = np.empty((N_FRAMES, nv, 3)); nf = np.empty((N_FRAMES, nn, 3))
    for k in range(N_FRAMES):
        vf[k] = p + 0.002 * (k + 1) * np.stack([np.sin(9.0 * p[:, 1] + k), np.sin(7.0 * p[:, 2] + 2 * k), np.sin(8.0 * p[:, 0] - k)], 1)
        n = q + 0.1 * np.stack([np.sin(5.0 * q[:, 1] + k), np.cos(6.0 * q[:, 0] - k), np.sin(4.0 * q[:, 2] + 3 * k)], 1)
        nf[k] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    R.sync()
    modes = (("linear", pkg.KEYFRAMES_LINEAR, 2), ("catmull_rom", pkg.KEYFRAMES_CATMULL_ROM, 4))
    keys = [m + s for m, _, _ in modes for s in ("_part_ms", "_device_ms", "_wall_ms")] + ["vertices_device_ms", "vertices_wall_ms"]
    runs = {k: [] for k in keys}
    for m, mode, _ in modes:                                                 # the frames go up once per interpolation
        R.set_vertex_keyframes(vf, nf, 0.0, 1.0, mode, pkg.KEYFRAMES_CLAMP)
        for i in range(WARM + TIMED):
            t = 0.37 + 2.2 * i / (WARM + TIMED)                              # between keyframes every time
            t0 = time.perf_counter()
            R.update_keyframes(t); R.sync()
            t1 = time.perf_counter()
            runs[m + "_wall_ms"].append((t1 - t0) * 1e3); runs[m + "_device_ms"].append(R.update_info().last_update_ms); runs[m + "_part_ms"].append(R.keyframe_info().last_ms)
            v = F.play_vertices(vf, t, 0.0, 1.0, mode, F.CLAMP); n = F.play_normals(nf, t, 0.0, 1.0, mode, F.CLAMP)
            if i == 0:                                                       # the device against the restatement, once per interpolation
                gv, gn = R.vertices()
                if not (np.array_equal(gv.view(np.uint64), v.view(np.uint64)) and np.array_equal(gn.view(np.uint64), n.view(np.uint64))):
                    raise SystemExit("keyframes_probe: the device's arrays differ from tests/keyframes_ref.py")
            t0 = time.perf_counter()
            R.update_vertices(v, n); R.sync()                                # the route this replaces, on the same arrays, alternating
            t1 = time.perf_counter()
            if mode == pkg.KEYFRAMES_LINEAR:
                runs["vertices_wall_ms"].append((t1 - t0) * 1e3); runs["vertices_device_ms"].append(R.update_info().last_update_ms)
    R.validate_trees()
    info = R.info(); ki = R.keyframe_info()
    R.close()
    out = {"scene": name, "n_tris": int(info.n_tris), "n_vertex": nv, "n_normal": nn, "n_frames": N_FRAMES, "keyframe_device_bytes": int(ki.device_bytes),
           "bytes_old_route_per_update": 24 * (nv + nn), "bytes_new_route_per_update": 8}
    for k in keys:
        x = sorted(runs[k][WARM:])
        out[k] = round(statistics.median(x), 4); out[k + "_min"] = round(x[0], 4); out[k + "_max"] = round(x[-1], 4)
    refit = out["linear_device_ms"] - out["linear_part_ms"]
    out["vertices_upload_ms"] = round(out["vertices_device_ms"] - refit, 4)
    for m, _, taps in modes:
        moved = 24 * (taps + 1) * (nv + nn)
        out[m + "_bytes"] = moved
        out[m + "_gbps"] = round(moved / (out[m + "_part_ms"] * 1e-3) / 1e9, 1)
        out[m + "_share_of_hbm_peak"] = round(out[m + "_gbps"] / HBM_PEAK_GBPS, 4)
        out["upload_over_" + m + "_part"] = round(out["vertices_upload_ms"] / out[m + "_part_ms"], 2)
        out["device_ratio_" + m + "_over_vertices"] = round(out[m + "_device_ms"] / out["vertices_device_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="measure this one scene in this process")
    a = ap.parse_args()
    if a.scene:
        print(json.dumps(measure(a.scene)))
        return
    runs = []
    for s in SCENES:                                                      # a fresh child process per scene; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--scene", s], capture_output=True, text=True, timeout=LIMIT_S[s])
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit("keyframes_probe: scene %s failed (exit %d)" % (s, p.returncode))
        runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "keyframes_probe", "scene": "S-cornell (48 x 24 sphere) and S-bath detail 420 at 640x360; %d synthetic frames (vertices plus a per-frame sine, normals tilted and "
                                               "normalised), played between keyframes; medians of %d after %d" % (N_FRAMES, TIMED, WARM),
           "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
