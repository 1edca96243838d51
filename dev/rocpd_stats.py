"""Kernel stats of a rocprofv3 --kernel-trace database (rocpd .db), in the layout of the profiles/*_kernel_stats.csv
files: python dev/rocpd_stats.py results.db [out.csv] [empty_below_ns]

With empty_below_ns (e.g. 20000) the launches of a kernel shorter than that are listed apart as "<name> [empty]":
a hybrid-eligible sort enqueues both kernel sequences and the launches of the route not taken leave at once."""
import csv
import math
import sqlite3
import sys


def stats(db, empty_below=0):
    c = sqlite3.connect(db)
    rows = {}
    for name, dur in c.execute("select name, duration from kernels"):
        key = name + (" [empty]" if empty_below and dur < empty_below and "rsort::" in name else "")
        rows.setdefault(key, []).append(dur)
    total = sum(sum(v) for v in rows.values())
    out = []
    for name, v in rows.items():
        n, s = len(v), sum(v)
        mean = s / n
        sd = math.sqrt(sum((x - mean) ** 2 for x in v) / (n - 1)) if n > 1 else 0.0
        out.append([name, n, s, round(mean, 6), round(100.0 * s / total, 4), min(v), max(v), round(sd, 6)])
    out.sort(key=lambda r: -r[2])
    return out


if __name__ == "__main__":
    rows = stats(sys.argv[1], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    f = open(sys.argv[2], "w", newline="") if len(sys.argv) > 2 else sys.stdout
    w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
    w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
    w.writerows(rows)
