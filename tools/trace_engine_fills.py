#!/usr/bin/env python3
"""How the align_many calls of a traced `bench.py` run begin, from a rocprofv3 --kernel-trace CSV (plain or .gz): per call the
prepare-class dispatches (k_prepare, k_prepare_many), the runtime's fill and copy kernels, when each of the three engines is
filled, and the time from the call's first engine prepare to its first kt_filter (profiles/r10_ab.txt items 0 and 1).
An engine's fill is a burst of prepare-class dispatches less than 0.3 ms apart: at least 15 k_prepare, or any k_prepare_many;
a call is three fills in a row (64 pairs per call: three engines).
usage: trace_engine_fills.py <kernel_trace.csv[.gz]>"""
import csv
import gzip
import sys

path = sys.argv[1]
ev = []
for r in csv.DictReader(gzip.open(path, "rt") if path.endswith(".gz") else open(path)):
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("cvo_dev::", "").replace("void ", "")
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
ev.sort()
bursts = []
for e in ev:
    if not e[2].startswith("k_prepare"):
        continue
    if bursts and e[0] - bursts[-1][-1][0] < 0.3e6:
        bursts[-1].append(e)
    else:
        bursts.append([e])
fills = [b for b in bursts if len(b) >= 15 or any(e[2] == "k_prepare_many" for e in b)]
print("%d dispatches, %d engine fills" % (len(ev), len(fills)))
for k in range(0, len(fills) - 2, 3):
    f = fills[k:k + 3]
    a = f[0][0][0]
    end = fills[k + 3][0][0] if k + 3 < len(fills) else ev[-1][1] + 1
    seg = [e for e in ev if a <= e[0] < end]
    filt = [e for e in seg if e[2].startswith("kt_filter")]
    last = max(e[1] for e in seg if e[2].startswith("kt_"))
    print("call %d: engines filled at +0 / +%.2f / +%.2f ms (%d %d %d prepare dispatches, %.3f %.3f %.3f ms each); prepare-class %d, fills %d, "
          "copies %d; first engine prepare -> first kt_filter %.3f ms, -> last loop kernel %.2f ms" % (
              k // 3, (f[1][0][0] - a) / 1e6, (f[2][0][0] - a) / 1e6, len(f[0]), len(f[1]), len(f[2]),
              (f[0][-1][1] - f[0][0][0]) / 1e6, (f[1][-1][1] - f[1][0][0]) / 1e6, (f[2][-1][1] - f[2][0][0]) / 1e6,
              sum(e[2].startswith("k_prepare") for e in seg), sum("fillBuffer" in e[2] for e in seg),
              sum("copyBuffer" in e[2] for e in seg), (filt[0][0] - a) / 1e6 if filt else float("nan"), (last - a) / 1e6))
