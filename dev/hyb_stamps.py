"""Per-phase cycles of the hybrid route's bucket kernel on the headline input (2^30 uniform keys, k = 8).

Needs a librsort.so whose rsort_hybrid.hip was compiled with the lab hooks and -DRSORT_HYB_STAMPS
(dev/lab_hooks.hpp), copied over cuda.radixsort_amd/librsort.so. Thread 0 of every workgroup adds the s_memtime
cycles between its phase ends, so a phase's figure includes the wait at the barrier that ends it. Prints one JSON
line: cycles per bucket by phase, and the bucket kernel's share of a sort measured by device events around whole
sorts of the stamped build.

    python dev/hyb_stamps.py [--log2n 30] [--reps 5]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "cuda.radixsort_amd"))
import radixsort as rs  # noqa: E402
import torch  # noqa: E402

PHASES = ["load_issue_and_wait", "pass0", "pass1", "store_issue"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = 1 << a.log2n
    lib = rs._lib()
    read = lib.rsort_lab_hyb_stamps
    read.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    read.restype = ctypes.c_int
    buf = (ctypes.c_uint64 * 8)()
    p = rs.plan(n, 8)
    keys, out = rs.empty_u32(n), rs.empty_u32(n)
    ws = rs.workspace(p.workspace_bytes)
    rs.gen_uniform(keys, 0x5EED)
    with rs.hybrid(rs.HYBRID_FORCE):
        rs.sort_device(keys, out, 8, ws=ws, plan_=p)
        assert rs.hybrid_report(p, ws)["hybrid"] and rs.plan_check(p, ws) == 0
        assert read(buf) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            rs.sort_device(keys, out, 8, ws=ws, plan_=p)
        e1.record()
        torch.cuda.synchronize()
        assert read(buf) == 0
    v = [int(x) for x in buf]
    buckets = v[7]
    res = {"log2n": a.log2n, "reps": a.reps, "buckets_stamped": buckets, "ms_per_sort_stamped_build": e0.elapsed_time(e1) / a.reps,
           "cycles_per_bucket": {PHASES[i]: round(v[i] / buckets, 1) for i in range(4)},
           "cycles_per_bucket_total": round(sum(v[:4]) / buckets, 1),
           "kernels_used": rs.scatter_kernels_used()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
