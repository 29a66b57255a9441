#!/usr/bin/env python
"""GPU-box tool: steady-state durations of the convolution kernels of a headline trace (rocprofv3 --kernel-trace), by full kernel
name: mean, median, 5th and 95th percentile in us.  Steady state = dispatches after the last naive_conv_* kernel (MIOpen find).
    python tools/headline_conv_durations.py DIR_WITH_THE_TRACE"""
import csv, glob, hashlib, sys
import numpy as np
csv.field_size_limit(10**9)
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
t0 = max([e for n, s, e in rows if n.startswith("naive_conv")] or [0])
acc = {}
for n, s, e in rows:
    if s >= t0 and ("kernel_grouped_conv" in n or "k_conv3x3" in n or "k_bias_act" in n):
        acc.setdefault(n, []).append((e - s) / 1e3)
print("\n# convolution kernels by full name (steady state: after the last naive_conv_* dispatch)")
for n, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
    v = np.array(v)
    tag = "ours, hand-written (net_conv3x3.hip), " + ("D = bias + skip" if ("ILb1E" in n or "<true>" in n) else "D = bias") if "k_conv3x3" in n else \
          ("k_bias_act" if "k_bias_act" in n else ("ours (BiasResAct functor)" if "BiasResAct" in n else "MIOpen's"))
    print("%-48s [%s, name sha1 %s] calls=%d mean_us=%.1f median_us=%.1f p05_us=%.1f p95_us=%.1f"
          % (n[:46] + "..", tag, hashlib.sha1(n.encode()).hexdigest()[:8], len(v), v.mean(), np.median(v), np.percentile(v, 5), np.percentile(v, 95)))
