"""What one parts update that runs all four deformers costs against the four single-route calls it replaces, on S-cornell (1 249
records, the test scene) and on S-bath at detail 420 (2.04 M records, bench configuration c5).  The set-ups are synthetic: two groups, three
bones with one influence per record, one dense morph target over every fourth record, two keyframes with normal frames; vertex owner i % 5,
normal owner (7 i + 3) % 5.

Per scene, in one process, medians of 10 after 2 warm-ups, the parts update and the four single-route calls alternating:
  parts_device_ms: mcpt_update_info::last_update_ms of the parts update -- four routes, eight selects, ONE refit;
  parts_part_ms: mcpt_parts_info::last_ms of the same call -- the routes and their selects alone;
  single_device_ms: the SUM of last_update_ms of mcpt_update_transforms, _skin, _morph and _keyframes with the same payloads -- four refits;
  single_part_ms: the sum of their own last_ms -- the deformer kernels without any select;
  select_ms: parts_part_ms - single_part_ms, the price of the scratch round trip; refit_ms: parts_device_ms - parts_part_ms.
The device's arrays after the parts update are checked against parts_ref.combine of what the four single calls left, bit for bit, in the same
run.  The ratios go into the JSON, not into an assertion.  One process per scene (--scene NAME), each under its own time limit; a failure ends
the run.  Not part of bench.py.

    python tools/parts_probe.py [--out profiles/parts_probe.json]
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

SCENES = ("cornell", "c5")
LIMIT_S = {"cornell": 120, "c5": 420}
WARM, TIMED = 2, 10


def measure(name):
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from tests import parts_ref as P, transform_ref as T
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("parts_probe: no GPU (timings are only measured on the device)")
    scene = pkg.scenes.cornell_box(64, 64, sphere_lon=48, sphere_lat=24) if name == "cornell" else pkg.scenes.bathroom_stress(640, 360, detail=420, tex_size=64)
    nv, nn = scene.vertex.shape[0], scene.normal.shape[0]
    p, q = scene.vertex, scene.normal
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    R = pkg.Renderer(scene, max_depth=6, flags=pkg.FLAG_DYNAMIC | pkg.FLAG_GPU_BVH_BUILD)
    iv, inn = np.arange(nv), np.arange(nn)
    R.set_vertex_groups((iv % 2).astype(np.uint32), (inn % 2).astype(np.uint32), 2)
    one = lambda i: (np.stack([i % 3, 0 * i, 0 * i, 0 * i], 1).astype(np.uint32), np.tile((1.0, 0.0, 0.0, 0.0), (i.shape[0], 1)))
    R.set_vertex_skin(*one(iv), *one(inn), 3)
    R.set_vertex_morph([(iv[::4], np.tile((0.001, 0.002, -0.001), (iv[::4].shape[0], 1)))], [(inn[::4], np.tile((0.01, 0.0, 0.02), (inn[::4].shape[0], 1)))])
    vf = np.stack([p, p + 0.002 * np.stack([np.sin(9.0 * p[:, 1]), np.sin(7.0 * p[:, 2]), np.sin(8.0 * p[:, 0])], 1)])
    R.set_vertex_keyframes(vf, np.stack([q, q]), 0.0, 1.0, pkg.KEYFRAMES_LINEAR, pkg.KEYFRAMES_CLAMP)
    vo, no = (iv % 5).astype(np.uint8), ((7 * inn + 3) % 5).astype(np.uint8)
    R.set_vertex_owners(vo, no)
    turn = lambda deg: T.about(T.rotation((0, 1, 0), deg), centre) + 0.0
    groups = np.stack([T.identity(1)[0], turn(2.0)]); bones = np.stack([T.identity(1)[0], turn(-1.5), turn(1.0)]); weights = np.array([0.5]); time = 0.37
    singles = (("groups", lambda: R.update_transforms(groups), R.transform_info), ("skin", lambda: R.update_skin(bones), R.skin_info),
               ("morph", lambda: R.update_morph(weights), R.morph_info), ("keyframes", lambda: R.update_keyframes(time), R.keyframe_info))
    keys = ["parts_device_ms", "parts_part_ms", "single_device_ms", "single_part_ms"] + [k + "_device_ms" for k, _, _ in singles]
    runs = {k: [] for k in keys}
    bits = lambda a: a.view(np.uint64)
    for i in range(WARM + TIMED):
        dev = part = 0.0; outs_v, outs_n = {}, {}
        for owner, (k, call, info) in enumerate(singles, 1):
            call(); R.sync()
            d = R.update_info().last_update_ms
            dev += d; part += info().last_ms; runs[k + "_device_ms"].append(d)
            if i == 0:
                outs_v[owner], outs_n[owner] = R.vertices()
        runs["single_device_ms"].append(dev); runs["single_part_ms"].append(part)
        before = R.vertices() if i == 0 else None
        R.update_parts(groups=groups, bones=bones, weights=weights, time=time); R.sync()
        runs["parts_device_ms"].append(R.update_info().last_update_ms); runs["parts_part_ms"].append(R.parts_info().last_ms)
        if i == 0:                                                           # the select against the restatement, on what the single calls left
            gv, gn = R.vertices()
            if not (np.array_equal(bits(gv), bits(P.combine(before[0], vo, outs_v))) and np.array_equal(bits(gn), bits(P.combine(before[1], no, outs_n)))):
                raise SystemExit("parts_probe: the device's arrays differ from tests/parts_ref.py")
    R.validate_trees()
    info = R.info(); pi = R.parts_info()
    R.close()
    out = {"scene": name, "n_tris": int(info.n_tris), "n_vertex": nv, "n_normal": nn, "parts_device_bytes": int(pi.device_bytes),            "select_bytes_per_update": int((48 * 0.8 + 4) * (nv + nn))}       # 4 of 5 records are owned: 24 B read and 24 B written; 1 owner byte per record and route
    for k in keys:
        x = sorted(runs[k][WARM:])
        out[k] = round(statistics.median(x), 4); out[k + "_min"] = round(x[0], 4); out[k + "_max"] = round(x[-1], 4)
    out["select_ms"] = round(out["parts_part_ms"] - out["single_part_ms"], 4)
    out["refit_ms"] = round(out["parts_device_ms"] - out["parts_part_ms"], 4)
    out["parts_over_single_device"] = round(out["parts_device_ms"] / out["single_device_ms"], 4)
    out["select_share_of_parts_update"] = round(out["select_ms"] / out["parts_device_ms"], 4)
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
            raise SystemExit("parts_probe: scene %s failed (exit %d)" % (s, p.returncode))
        runs.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "parts_probe", "scene": "S-cornell (48 x 24 sphere) and S-bath detail 420 at 640x360; all four deformers set up synthetically, interleaved owners; "
                                           "medians of %d after %d" % (TIMED, WARM), "runs": runs}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
