#!/usr/bin/env python3
"""How the two wavefront kernels sit beside each other in time, from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --config c2 --spp 256 --steps 1 --warmup 1     (no --pmc in the same run)
    python tools/overlap_windows.py DIR | FILE.csv [--jobs] [--tenths]                                                         (no GPU needed)

Prints, for the wall-clock span from the first to the last launch of wf_trace8_kernel / wf_shade_kernel, the share in which only trace launches
are running, only shade launches, both, or neither -- a launch "runs" from its start to its end timestamp, so a trace launch whose blocks are
still queued for CUs behind another trace launch counts as running -- and the mean period (start to start) of either kernel per queue, a queue
being a sub-pipeline's stream.  A render call ("job") begins with the wf_pool_reset_kernel launches of its sub-pipelines; the shares are
printed over all jobs together (the time between jobs left out) and, with --jobs, for every job.
"""
import argparse
import csv
import glob
import os

TRACE, SHADE, RESET = "wf_trace8_kernel", "wf_shade_kernel", "wf_pool_reset_kernel"


def read_rows(path):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                kind = "T" if TRACE in name else "S" if SHADE in name else "R" if RESET in name else None
                if kind:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, r.get("Queue_Id", "0")))
    rows.sort()
    return rows


def split_jobs(rows):
    """Lists of T / S launches, one per render call: a reset launch that follows a T or S launch opens the next job."""
    jobs, cur = [], []
    for r in rows:
        if r[2] == "R":
            if cur:
                jobs.append(cur); cur = []
        else:
            cur.append(r)
    if cur:
        jobs.append(cur)
    return jobs


def windows(job, lo=None, hi=None):
    """ns of the job's span (or of its part [lo, hi)) with only trace, only shade, both, neither running: a sweep over the start and end timestamps."""
    ev = []
    for s, e, kind, _ in job:
        ev.append((s, 1, kind)); ev.append((e, -1, kind))
    ev.sort(key=lambda x: (x[0], x[1]))                                     # at equal times an end comes before a start
    out = {"trace": 0, "shade": 0, "both": 0, "neither": 0}
    n = {"T": 0, "S": 0}
    prev = ev[0][0]
    for t, d, kind in ev:
        a, b = (prev, t) if lo is None else (max(prev, lo), min(t, hi))
        if b > a:
            out["both" if n["T"] and n["S"] else "trace" if n["T"] else "shade" if n["S"] else "neither"] += b - a
        n[kind] += d; prev = t
    return out


def tenths(job):
    """windows() of each tenth of the job's span: where in a job the one-kernel windows sit (its start, its steady state, its drain)."""
    t0, t1 = min(r[0] for r in job), max(r[1] for r in job)
    return [windows(job, t0 + (t1 - t0) * i // 10, t0 + (t1 - t0) * (i + 1) // 10) for i in range(10)]


def periods(job):
    """{queue: (mean start-to-start distance of its trace launches in ns, number of distances)}."""
    by_q = {}
    for s, _, kind, q in job:
        if kind == "T":
            by_q.setdefault(q, []).append(s)
    return {q: ((v[-1] - v[0]) / (len(v) - 1), len(v) - 1) for q, v in by_q.items() if len(v) > 1}


def report(title, wins, pers):
    span = sum(wins.values())
    print("%s: span %.3f ms" % (title, span / 1e6))
    for k, label in (("trace", "only wf_trace8_kernel"), ("shade", "only wf_shade_kernel"), ("both", "both"), ("neither", "neither")):
        print("  %-22s %9.3f ms  %5.1f %%" % (label, wins[k] / 1e6, 100.0 * wins[k] / span if span else 0.0))
    for q in sorted(pers):
        print("  queue %-4s mean period %8.1f us over %d iterations" % (q, pers[q][0] / 1e3, pers[q][1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace", help="a rocprofv3 kernel-trace CSV, or a directory that holds one")
    ap.add_argument("--jobs", action="store_true", help="also print every render call on its own")
    ap.add_argument("--tenths", action="store_true", help="also print the windows of every tenth of a render call's span, summed over the calls")
    ap.add_argument("--skip", type=int, default=0, help="leave out the first N render calls (warm-up)")
    a = ap.parse_args()
    jobs = split_jobs(read_rows(a.trace))[a.skip:]
    if not jobs:
        raise SystemExit("no %s / %s launches in the trace" % (TRACE, SHADE))
    total = {"trace": 0, "shade": 0, "both": 0, "neither": 0}
    dist = {}
    by_tenth = [dict(total) for _ in range(10)]
    for i, job in enumerate(jobs):
        w, p = windows(job), periods(job)
        for k in total:
            total[k] += w[k]
        for q, (mean, n) in p.items():
            s, m = dist.get(q, (0.0, 0)); dist[q] = (s + mean * n, m + n)
        for i10, w10 in enumerate(tenths(job)):
            for k in total:
                by_tenth[i10][k] += w10[k]
        if a.jobs:
            report("job %d (%d launches)" % (i + a.skip, len(job)), w, p)
    report("%d render calls, %d launches" % (len(jobs), sum(len(j) for j in jobs)), total, {q: (s / n, n) for q, (s, n) in dist.items()})
    if a.tenths:
        print("by tenth of a render call's span (ms, all calls): only trace / only shade / both / neither")
        for i10, w10 in enumerate(by_tenth):
            print("  %3d - %3d %%  %8.3f  %8.3f  %8.3f  %8.3f" % (10 * i10, 10 * i10 + 10, w10["trace"] / 1e6, w10["shade"] / 1e6, w10["both"] / 1e6, w10["neither"] / 1e6))


if __name__ == "__main__":
    main()
