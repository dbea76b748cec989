"""Reduce a `rocprofv3 --kernel-trace` (or `--pmc`) run of a pipelined-schedule process: per kernel the mean duration,
the gap between consecutive gar_backward_wave_half launches (end of one to start of the next), counters per launch.
usage: pipeline_trace_reduce.py DIR   (searched recursively for *kernel_trace.csv / *counter_collection.csv)"""
import csv, glob, os, sys
import numpy as np
root = sys.argv[1]
for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
    rows = list(csv.DictReader(open(path)))
    by = {}
    for r in rows:
        by.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    print(path)
    for k, v in sorted(by.items(), key=lambda kv: -sum(e - s for s, e in kv[1])):
        d = np.array([e - s for s, e in v]) / 1e6
        print(f"  {k[:70]:70s} n {len(v):4d}  mean {d.mean():8.3f} ms  median {np.median(d):8.3f}  min {d.min():8.3f}")
    half = sorted(v for k, vs in by.items() if "gar_backward_wave_half" in k for v in vs)
    if len(half) > 4:
        gaps = np.array([half[i + 1][0] - half[i][1] for i in range(2, len(half) - 1)]) / 1e3
        per = np.array([half[i + 2][0] - half[i][0] for i in range(2, len(half) - 2)]) / 1e6
        print(f"  gap between consecutive backward halves (us): mean {gaps.mean():.1f}  median {np.median(gaps):.1f}  "
              f"min {gaps.min():.1f}  max {gaps.max():.1f}   (n {len(gaps)}; the first two launches left out)")
        print(f"  start to start over two halves = one step (ms): mean {per.mean():.3f}  median {np.median(per):.3f}")
for path in sorted(glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True)):
    rows = list(csv.DictReader(open(path)))
    acc = {}
    for r in rows:
        key = (r["Kernel_Name"].split("(")[0], r["Counter_Name"])
        acc.setdefault(key, {}).setdefault(r["Dispatch_Id"], 0.0)
        acc[key][r["Dispatch_Id"]] += float(r["Counter_Value"])
    print(path)
    for (k, c), d in sorted(acc.items()):
        v = np.array(list(d.values()))
        print(f"  {k[:60]:60s} {c:16s} launches {len(v):4d}  mean per launch {v.mean():.4g}")
