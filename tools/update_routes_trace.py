"""Every live-scene update route once, plain and _reproject, on the fixture of tests/test_update_routes.py with auto normals on: the workload
whose sequence of kernels a change to the host layer (csrc/mcpt_api.cpp) must leave as it is.  One process, one context, one stream: the order of
the kernels in a trace is the order the host enqueued them in.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/update_routes_trace.py      # the workload, under the tracer
    python tools/update_routes_trace.py --names DIR > sequence.txt                                  # the trace's kernel names in start order

MCPT_LIB_PATH chooses the library (A/B); two sequences are compared with diff.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload():
    import __graft_entry__ as ge
    from tests import test_update_routes as U
    pkg = ge.load_package()
    r = U._context(pkg, auto=True)
    k = 0
    for route in U.ROUTES:
        for reproject in ((False,) if route == "normals" else (False, True)):
            U._call(pkg, r, route, k, reproject); k += 1
    r.sync()
    print("update_routes_trace: %d calls, %d updates" % (k, r.update_info().updates))
    r.close()


def names(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [(int(row["Start_Timestamp"]), row["Kernel_Name"]) for row in csv.DictReader(f)]
    if not rows:
        raise SystemExit("update_routes_trace: no kernel trace under %s" % trace_dir)
    for _, name in sorted(rows):
        print(name)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default=None, metavar="DIR")
    a = ap.parse_args()
    names(a.names) if a.names else workload()
