"""Timing of the denoised preview on S-cornell at 800x800 and 3840x2160; prints one JSON line.

features_ms: mcpt_render_features at spp 4.  denoise_ms: mcpt_denoise with the default 5 levels, median of 20 runs after 3 warm-ups.
Both are bracketed by device events on the context's stream (a torch side stream lent to the context) and end in an event synchronise.
Bytes are the filter's compulsory HBM traffic: per level the guide and {irr, var} read and {irr, var} written (48 B / pixel); the whole
call adds the prep pass (film + features read, guide + {irr, var} written) and the last level's albedo and film reads.  Not part of bench.py.
robust_*: the same call with MCPT_DENOISE_SPLIT_EMISSION | MCPT_DENOISE_CLAMP_FIREFLIES (the LDS-staged prep kernel, the emission read in the prep
pass and the last level), each flag alone, and mcpt_render_features once the context owns the emission buffer (features and emission in one pass).

    python tools/denoise_probe.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec (MI355X_MICROARCH: 6.29 TB/s measured for a float4 copy)
LEVELS = 5


def measure(pkg, torch, w, h):
    scene = pkg.scenes.cornell_box(w, h)
    r = pkg.Renderer(scene, max_depth=8)
    s = torch.cuda.Stream()
    r.set_torch_stream(s)
    r.render(4, seed=7)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(s); fn(); e1.record(s); e1.synchronize()
        return e0.elapsed_time(e1)

    feat = [timed(lambda: r.render_features(spp=4, seed=7)) for _ in range(4)]
    call = lambda: r._check(r.lib.mcpt_denoise(r.ctx, None, None))
    for _ in range(3):
        timed(call)
    den = sorted(timed(call) for _ in range(20))

    def flagged(flags):
        o = pkg.DenoiseOpts(); o.struct_size = pkg.C.sizeof(pkg.DenoiseOpts); o.flags = flags
        run = lambda: r._check(r.lib.mcpt_denoise(r.ctx, None, pkg.C.byref(o)))
        for _ in range(3):
            timed(run)
        return round(statistics.median(timed(run) for _ in range(20)), 4)

    clamp_ms = flagged(pkg.DENOISE_CLAMP_FIREFLIES)                      # before the context owns the emission buffer
    split_ms = flagged(pkg.DENOISE_SPLIT_EMISSION)                       # (the first call allocates it and renders the emission: a warm-up)
    both_ms = flagged(pkg.DENOISE_SPLIT_EMISSION | pkg.DENOISE_CLAMP_FIREFLIES)
    feat_emis = [timed(lambda: r.render_features(spp=4, seed=7)) for _ in range(4)]
    n = w * h
    per_level = 48 * n
    total = n * ((16 + 32 + 16 + 16) + per_level // n * (LEVELS - 1) + (16 + 16 + 16 + 16 + 16))
    ms = statistics.median(den)
    r.sync(); r.close()
    return {
        "size": "%dx%d" % (w, h),
        "features_ms_spp4": round(statistics.median(feat[1:]), 4),
        "denoise_ms": round(ms, 4), "denoise_ms_min": round(den[0], 4), "denoise_ms_max": round(den[-1], 4), "levels": LEVELS,
        "denoise_clamp_ms": clamp_ms, "denoise_split_ms": split_ms, "denoise_robust_ms": both_ms,
        "features_with_emission_ms_spp4": round(statistics.median(feat_emis[1:]), 4),
        "bytes_per_level": per_level, "bytes_per_call": total,
        "achieved_GBps": round(total / (ms * 1e-3) / 1e9, 1),
        "hbm_floor_ms": round(total / HBM_PEAK * 1e3, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_probe: no GPU (timings are only measured on the device)")
    res = {"tool": "denoise_probe", "scene": "S-cornell depth 8, 4 spp film", "device": torch.cuda.get_device_name(0),
           "runs": [measure(pkg, torch, 800, 800), measure(pkg, torch, 3840, 2160)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
