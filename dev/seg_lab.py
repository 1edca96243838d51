"""Lab: the segmented sort against the two other ways to sort many segments (DESIGN §5a's table).

    python dev/seg_lab.py --shape A [--reps 12] [--warmup 3]      (one JSON line per shape; dev/lab.sh seg)

2^26 uniform keys in one of five segmentations:
    A  2^12 x 2^14      B  2^16 x 2^10      C  2^20 x 64
    D  2^18 segments, log-normal lengths (median 128, fixed seed, total 2^26), at least 8 longer than the lds capacity
    E  8 x 2^23         (all multi-tile: the documented slow case)
and for each shape, HIP-event medians of `reps` timed calls after `warmup`:
    new     rsort_u32_segmented_device (also with values for A and B)
    loop    a host loop of rsort_u32_device, one call per segment, into the same output -- what a caller had
            before. For B, C and D it runs over the first 256 non-empty segments only and is scaled by the segment
            count (the loop's cost is launches, not keys); A and E run every segment.
    vendor  rsort_u32_vendor_segmented_device (rocPRIM) on the same buffers
The new call's output is compared with the vendor's before anything is timed."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "cuda.radixsort_amd"))
import radixsort as rs  # noqa: E402
import torch  # noqa: E402

N = 1 << 26
LOOP_SAMPLE = 256


def lengths_for(shape: str, c_lds: int) -> np.ndarray:
    if shape == "A":
        return np.full(1 << 12, 1 << 14, np.int64)
    if shape == "B":
        return np.full(1 << 16, 1 << 10, np.int64)
    if shape == "C":
        return np.full(1 << 20, 64, np.int64)
    if shape == "E":
        return np.full(8, 1 << 23, np.int64)
    if shape != "D":
        raise SystemExit(f"unknown shape {shape}")
    s = 1 << 18
    rng = np.random.default_rng(20261020)
    # median 128, mean 256: sigma^2 = 2 ln 2
    ln = np.maximum(rng.lognormal(np.log(128.0), np.sqrt(2.0 * np.log(2.0)), s), 1.0)
    big = np.arange(8) * (s // 8) + 17  # eight segments forced past the lds capacity
    fixed = c_lds + 1 + 1000 * np.arange(8)
    ln[big] = 0
    ln = np.floor(ln * ((N - fixed.sum()) / ln.sum())).astype(np.int64)
    ln[big] = fixed
    rest = N - int(ln.sum())
    assert 0 <= rest < s
    small = np.setdiff1d(np.arange(s), big)[:rest]
    ln[small] += 1
    assert int(ln.sum()) == N and int((ln > c_lds).sum()) >= 8
    return ln


def median_ms(fn, warmup: int, reps: int) -> tuple[float, float, float]:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = rs._lib()
    cap = {"keys": rs.segmented_capacity(False), "pairs": rs.segmented_capacity(True)}
    ln = lengths_for(args.shape, cap["keys"][1])
    off_h = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    nseg = ln.size
    keys = rs.empty_u32(N)
    rs.gen_uniform(keys, seed=0x5EED)
    out = rs.empty_u32(N)
    ref = rs.empty_u32(N)
    off = rs._device_offsets(off_h, keys.device)
    stream = rs._stream()
    rec = {"shape": args.shape, "keys": N, "segments": int(nseg), "max_len": int(ln.max()),
           "median_len": float(np.median(ln)), "capacity": cap, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    # --- the new call, checked against the vendor's output first
    ws = rs.workspace(rs.segmented_workspace_size(N, nseg, False))
    vws = rs.workspace(int(lib.rsort_vendor_segmented_workspace_size(N, nseg)))
    rs.segmented_sort_device(keys, out, off, ws=ws)
    flags, cc = rs.segmented_check(N, nseg, False, ws)
    rs.vendor_segmented_sort_device(keys, ref, off, ws=vws)
    torch.cuda.synchronize()
    rec["flags"], rec["classes"] = flags, cc
    rec["equals_vendor"] = bool(torch.equal(out, ref))
    if flags != 0 or not rec["equals_vendor"]:
        print(json.dumps(rec), flush=True)
        raise SystemExit(2)

    def gk(ms):
        return round(N / ms / 1e6, 3)

    def put(name, t):
        rec[name] = {"ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4), "gkeys_s": gk(t[0])}

    put("new", median_ms(lambda: rs.segmented_sort_device(keys, out, off, ws=ws), args.warmup, args.reps))
    put("vendor", median_ms(lambda: rs.vendor_segmented_sort_device(keys, ref, off, ws=vws), args.warmup, args.reps))
    if args.shape in ("A", "B"):
        vals = rs.empty_u32(N)
        rs.gen_iota(vals)
        vout = rs.empty_u32(N)
        pws = rs.workspace(rs.segmented_workspace_size(N, nseg, True))
        put("new_pairs", median_ms(lambda: rs.segmented_sort_device(keys, out, off, vals_in=vals, vals_out=vout, ws=pws),
                                   args.warmup, args.reps))
        f2, _ = rs.segmented_check(N, nseg, True, pws)
        rec["flags_pairs"] = f2
        del vals, vout, pws

    # --- the loop: one rsort_u32_device call per segment (straight through ctypes: no Python wrapper cost)
    nz = np.flatnonzero(ln > 0)
    full = args.shape in ("A", "E")
    take = nz if full else nz[:LOOP_SAMPLE]
    lws = rs.workspace(max(rs.workspace_size(int(m), 8) for m in set(ln[take].tolist())))
    kin, kout = keys.data_ptr(), out.data_ptr()
    calls = [(ctypes.c_void_p(kin + 4 * int(off_h[i])), ctypes.c_void_p(kout + 4 * int(off_h[i])), int(ln[i]))
             for i in take]
    wsp, wsn = ctypes.c_void_p(lws.data_ptr()), lws.numel()

    def loop():
        for a, b, m in calls:
            st = lib.rsort_u32_device(a, b, m, 8, wsp, wsn, stream)
            if st:
                raise rs.RSortError(st, "rsort_u32_device")

    t = median_ms(loop, 1, max(3, args.reps if not full or args.shape == "E" else 5))
    scale = nz.size / take.size
    rec["loop"] = {"ms": round(t[0] * scale, 3), "measured_ms": round(t[0], 4), "segments_timed": int(take.size),
                   "scaled_by": round(scale, 3), "gkeys_s": gk(t[0] * scale)}
    if full:  # the loop sorted every segment: its output must be the new call's
        rs.segmented_sort_device(keys, ref, off, ws=ws)
        torch.cuda.synchronize()
        rec["loop_equals_new"] = bool(torch.equal(out, ref))
    rec["new_over_loop"] = round(rec["loop"]["ms"] / rec["new"]["ms"], 2)
    rec["new_over_vendor"] = round(rec["vendor"]["ms"] / rec["new"]["ms"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
