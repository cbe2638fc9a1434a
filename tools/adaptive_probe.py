"""Measurements of adaptive sampling; writes profiles/adaptive_probe.json (merged into what is there).  Not part of bench.py.

    python tools/adaptive_probe.py quality      S-cornell 800x800 depth 8 and S-veach 1280x720: display RMSE against 4096 spp of uniform
                                                sampling (a spp sweep) and of mcpt_render_adaptive at the defaults over a threshold sweep --
                                                samples, wall time, RMSE; the threshold at which adaptive matches uniform 256 spp on S-cornell;
                                                time-to-quality (the uniform spp and time at adaptive's RMSE, log-log interpolated)
    python tools/adaptive_probe.py kernels      one-pass adaptive calls (min = max = 2) at 800x800 and 3840x2160, to run under
                                                `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/adaptive_probe.py kernels`
    python tools/adaptive_probe.py parse DIR    per-pass time of the error + compaction kernels, and the host round trip between a pass's last
                                                kernel (ad_scatter_kernel) and the next pass's first, from that kernel trace

Display RMSE: over all pixels and channels of sqrt(clamp(mean, 0, 1)), mcpt_tonemap's curve before the x255.99.  Wall time: the call and a
synchronise, median of 3 after a warm-up.
"""
from __future__ import annotations

import csv
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "adaptive_probe.json")
THRESHOLDS = [0.8, 0.6, 0.45, 0.35, 0.25, 0.18, 0.12, 0.08]
UNIFORM = [16, 32, 64, 128, 256, 512, 1024]


def _merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _wall(r, fn, reps=3):
    ts = []
    for _ in range(reps):
        r.clear(); r.sync()
        t0 = time.perf_counter(); out = fn(); r.sync(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, out


def _loglog(xs, ys, y):
    """x at which the piecewise log-log line through (xs, ys) (ys decreasing) reaches y."""
    for (x0, y0), (x1, y1) in zip(zip(xs, ys), zip(xs[1:], ys[1:])):
        if y1 <= y <= y0:
            f = (math.log(y) - math.log(y0)) / (math.log(y1) - math.log(y0))
            return math.exp(math.log(x0) + f * (math.log(x1) - math.log(x0)))
    return None


def quality(pkg, ar):
    res = {}
    for name, scene, depth in (("S-cornell 800x800 depth 8", pkg.scenes.cornell_box(800, 800), 8),
                               ("S-veach 1280x720 unbounded", pkg.scenes.veach_mis(1280, 720), 0)):
        r = pkg.Renderer(scene, max_depth=depth)
        n_px = scene.camera.width * scene.camera.height
        r.render(4096, seed=99)
        ref = r.read_accum()
        r.render_adaptive(seed=1, max_spp=32); r.sync()                   # warm-up: pools and adaptive buffers allocated
        uni = []
        for spp in UNIFORM:
            ms, _ = _wall(r, lambda: r.render(spp, seed=7))
            uni.append({"spp": spp, "wall_ms": round(ms, 2), "rmse": ar.display_rmse(r.read_accum(), ref)})
        ad = []
        for thr in THRESHOLDS:
            ms, st = _wall(r, lambda: r.render_adaptive(seed=7, threshold=thr))
            rmse = ar.display_rmse(r.read_accum(), ref)
            spp_eq = _loglog([u["spp"] for u in uni], [u["rmse"] for u in uni], rmse)
            same = round(st.pixel_samples / n_px)
            ms_same, _ = _wall(r, lambda: r.render(same, seed=7))
            rmse_same = ar.display_rmse(r.read_accum(), ref)
            ad.append({"threshold": thr, "wall_ms": round(ms, 2), "rmse": rmse, "spp_per_pixel": st.pixel_samples / n_px, "passes": st.passes,
                       "tiles_converged": st.tiles_converged, "tiles_capped": st.tiles_capped,
                       "uniform_same_samples": {"spp": same, "wall_ms": round(ms_same, 2), "rmse": rmse_same, "rmse_ratio": rmse / rmse_same},
                       "uniform_same_rmse": {"spp": spp_eq, "wall_ms": None if spp_eq is None else
                                             round(_loglog_time(uni, spp_eq), 2)}})
            print(json.dumps({"scene": name, **ad[-1]}), flush=True)
        r.close()
        res[name] = {"uniform": uni, "adaptive": ad}
    # the default: where adaptive at the defaults matches uniform 256 spp on S-cornell
    c = res["S-cornell 800x800 depth 8"]
    target = next(u["rmse"] for u in c["uniform"] if u["spp"] == 256)
    pts = sorted((a["rmse"], a["threshold"]) for a in c["adaptive"])
    pick = None
    for (r0, t0), (r1, t1) in zip(pts, pts[1:]):
        if r0 <= target <= r1:
            pick = math.exp(math.log(t0) + (math.log(target) - math.log(r0)) / (math.log(r1) - math.log(r0)) * (math.log(t1) - math.log(t0)))
    res["threshold_matching_uniform_256_on_cornell"] = {"target_rmse": target, "threshold": pick}
    print(json.dumps(res["threshold_matching_uniform_256_on_cornell"]))
    _merge("quality", res)


def _loglog_time(uni, spp):
    xs = [u["spp"] for u in uni]; ts = [u["wall_ms"] for u in uni]
    for i in range(len(xs) - 1):
        if xs[i] <= spp <= xs[i + 1]:
            f = (math.log(spp) - math.log(xs[i])) / (math.log(xs[i + 1]) - math.log(xs[i]))
            return math.exp(math.log(ts[i]) + f * (math.log(ts[i + 1]) - math.log(ts[i])))
    return float("nan")


def kernels(pkg):
    for w, h in ((800, 800), (3840, 2160)):
        r = pkg.Renderer(pkg.scenes.cornell_box(w, h), max_depth=8)
        for _ in range(12):
            r.render_adaptive(seed=3, min_spp=2, max_spp=2)
        r.sync()
        # two passes: pass 0 at 2 spp, every tile active (threshold just above 0), pass 1 at 2 more -- the host round trip between them
        for _ in range(6):
            r.render_adaptive(seed=3, min_spp=2, max_spp=4, threshold=1e-30)
        r.sync(); r.close()


def parse(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    per = {}
    for x in rows:
        per.setdefault(x["Kernel_Name"].split("(")[0], []).append((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3)
    out = {}
    names = [n for n in per if n.startswith("ad_")]
    for n in names:
        v = per[n]
        out[n] = {"count": len(v), "median_us": statistics.median(v)}
    # rounds in trace order: an ad_error_kernel of the 800x800 context precedes its 3840x2160 ones; tell the sizes apart by their duration split
    err = [(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x) for x in rows if x["Kernel_Name"].startswith("ad_error_kernel")]
    rounds = []
    for i, x in enumerate(rows):
        if x["Kernel_Name"].startswith("ad_error_kernel") and i + 2 < len(rows) and rows[i + 2]["Kernel_Name"].startswith("ad_scatter_kernel"):
            t0 = int(x["Start_Timestamp"]); t1 = int(rows[i + 2]["End_Timestamp"])
            nxt = rows[i + 3] if i + 3 < len(rows) else None
            gap = (int(nxt["Start_Timestamp"]) - t1) / 1e3 if nxt is not None and not nxt["Kernel_Name"].startswith("ad_merge") else None
            rounds.append({"grid": int(x.get("Grid_Size", x.get("Grid_Size_X", 0)) or 0), "round_us": (t1 - t0) / 1e3, "gap_to_next_render_us": gap})
    by = {}
    for rd in rounds:
        by.setdefault(rd["grid"], []).append(rd)
    summary = {}
    for g, v in by.items():
        gaps = [x["gap_to_next_render_us"] for x in v if x["gap_to_next_render_us"] is not None]
        summary[str(g)] = {"rounds": len(v), "error_scan_scatter_us_median": statistics.median(x["round_us"] for x in v),
                           "host_round_trip_us_median": statistics.median(gaps) if gaps else None}
    out["rounds_by_error_grid"] = summary
    print(json.dumps(out, indent=1))
    _merge("kernels", out)


def main():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    mode = sys.argv[1] if len(sys.argv) > 1 else "quality"
    if mode == "parse":
        return parse(sys.argv[2])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adaptive_ref as ar
    if mode == "kernels":
        return kernels(pkg)
    return quality(pkg, ar)


if __name__ == "__main__":
    main()
