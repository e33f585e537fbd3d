#!/usr/bin/env python3
"""The step timeline from a rocprofv3 --kernel-trace CSV (a run of its own, no counters): per path
kernel of the last N steps, when the retrace and the async fold of the same launch start and end
relative to it, and the gap to the next path kernel.
  python tools/timeline.py <kernel_trace.csv> [N=6]
Times in ms; t = 0 is the start of each row's path kernel."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
paths = [e for e in ev if "mrt_path_kernel" in e[2]]
retr = [e for e in ev if "mrt_retrace_kernel" in e[2]]
fold = [e for e in ev if "mrt_fold_async_kernel" in e[2]]


def after(lst, t):  # the first kernel of lst that starts at or after t
    for e in lst:
        if e[0] >= t:
            return e
    return None


ms = lambda a: a / 1e6
print("%4s %9s %22s %22s %9s %9s" % ("step", "path", "retrace start..end", "fold start..end", "gap next", "period"))
sel = paths[-(n + 1):-1]
for i, p in enumerate(sel):
    nxt = paths[paths.index(p) + 1]
    r = after(retr, p[1] - 1000)  # its own retrace and fold are enqueued behind its end
    f = after(fold, p[1] - 1000)
    rs = "%9.3f..%9.3f" % (ms(r[0] - p[0]), ms(r[1] - p[0])) if r else "-"
    fs = "%9.3f..%9.3f" % (ms(f[0] - p[0]), ms(f[1] - p[0])) if f else "-"
    print("%4d %9.3f %22s %22s %9.3f %9.3f" % (i, ms(p[1] - p[0]), rs, fs, ms(nxt[0] - p[1]), ms(nxt[0] - p[0])))
names = {}
for s, e, k in ev:
    a = names.setdefault(k.split("(")[0][:70], [0, 0])
    a[0] += 1
    a[1] += e - s
for k, (c, t) in sorted(names.items(), key=lambda kv: -kv[1][1])[:8]:
    print("%-70s calls %5d avg %9.3f ms" % (k, c, ms(t) / c))
