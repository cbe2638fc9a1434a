"""What a light-probe pass costs, beside a surface-bake pass of the same item count, on S-cornell 800 x 800 at depth 8:
10 000 probes (a 25 x 20 x 20 grid over the scene's bounds: 640 000 items per pass) against 640 000 lightmap points.  Per figure `--passes`
passes in one call after `--warmup`, the call's own HIP-event bracket (mcpt_counters::kernel_ms) and the stage's stopwatch (last_stage_ms);
`--rounds` rounds, the two alternated.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` (a run of its own) the kernels' names
carry the split: sh_rays_kernel, sh_first_hit_kernel, sh_project_kernel, bk_rays_kernel, bk_unlit_kernel and the pipeline's wf_* kernels.

    python tools/shprobe_probe.py [--passes 32] [--warmup 4] [--rounds 3] [--only sh|bake]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=32); ap.add_argument("--warmup", type=int, default=4); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("sh", "bake"), default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    scene = pkg.scenes.cornell_box(800, 800)
    r = pkg.Renderer(scene, max_depth=8)
    used = scene.vertex[np.unique(scene.face[:, :, 0])]
    probes = pkg.sh_grid(used.min(0), used.max(0), 25, 20, 20)
    points, _ = pkg.lightmap_points(scene, 800, 800)
    out = {"probes": len(probes), "sh_items": 64 * len(probes), "bake_points": len(points), "passes": a.passes, "sh_pass_ms": [], "sh_stage_ms": [], "bake_pass_ms": [],
           "bake_stage_ms": []}
    if a.only != "bake":
        r.set_sh_probes(probes); r.bake_sh(a.warmup, 1, 0)
    if a.only != "sh":
        r.set_bake_points(points); r.bake(a.warmup, 1, 0)
    r.sync()
    for k in range(a.rounds):
        if a.only != "sh":
            r.bake(a.passes, 1, a.warmup + k * a.passes); r.sync()
            out["bake_pass_ms"].append(round(r.counters().kernel_ms / a.passes, 4)); out["bake_stage_ms"].append(round(r.bake_info().last_stage_ms / a.passes, 5))
        if a.only != "bake":
            r.bake_sh(a.passes, 1, a.warmup + k * a.passes); r.sync()
            out["sh_pass_ms"].append(round(r.counters().kernel_ms / a.passes, 4)); out["sh_stage_ms"].append(round(r.sh_info().last_stage_ms / a.passes, 5))
    if a.only != "bake":
        acc, counts = r.read_sh_film()
        out["back_share_max"] = float((counts[:, 1] / np.maximum(counts[:, 0], 1)).max()); out["miss_share_mean"] = float((counts[:, 2] / np.maximum(counts[:, 0], 1)).mean())
        out["finite"] = bool(np.isfinite(acc).all())
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
