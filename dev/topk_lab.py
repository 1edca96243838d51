"""Lab: the top-k selection's two routes against each other (DESIGN §5b's table; profiles/topk.json).

    python dev/topk_lab.py [--lg 26 30] [--reps 12] [--warmup 3] [--out profiles/topk.json]

For n = 2^lg keys of three inputs (uniform; Zipf; keys below 2^16, the worst case, where the first digit removes
nothing), k in {1, 2^10, 2^16, 2^20, n/16, n/4, n/2}, keys only / values / indices, smallest first:
    select  rsort_u32_topk_device with RSORT_TOPK_SELECT forced
    sort    the same call with RSORT_TOPK_SORT forced: the whole sort and a slice, what the library could do before
            (for indices it includes the iota array)
    torch   torch.topk on the same buffer viewed as int32, for the keys below 2^16 only (every key < 2^31, so the
            signed order is the unsigned one) and k <= 2^20; keys and indices in one call
HIP-event medians of `reps` timed calls after `warmup`. Before anything is timed the select's output is compared,
every element, with the sort route's. Each n also gets the level-0 floor: two reads of the keys at the library's own
histogram rate (rsort_pass_histogram of the top digit), measured in the same process."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "cuda.radixsort_amd"))
import radixsort as rs  # noqa: E402
import torch  # noqa: E402

INPUTS = ("uniform", "zipf", "low16")
MODES = ("keys", "vals", "indices")


def zipf_cdf_u32(ranks: int = 1 << 20) -> np.ndarray:
    c = np.cumsum(1.0 / np.arange(1, ranks + 1, dtype=np.float64))
    t = np.minimum(np.floor(c / c[-1] * 4294967296.0), 4294967295.0)
    t[-1] = 4294967295.0
    return t.astype(np.uint32)


def fill(keys, name):
    if name == "zipf":
        rs.gen_zipf(keys, rs.from_numpy_u32(zipf_cdf_u32()), seed=0x5EED)
    else:
        rs.gen_uniform(keys, seed=0x5EED)
        if name == "low16":
            keys.bitwise_right_shift_(16).bitwise_and_(0xFFFF)
    torch.cuda.synchronize()


def median_ms(fn, warmup: int, reps: int):
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
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, nargs="+", default=[26, 30])
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/topk.json")
    args = ap.parse_args()
    rows, floors = [], []
    for lg in args.lg:
        n = 1 << lg
        ks = [1, 1 << 10, 1 << 16, 1 << 20, n // 16, n // 4, n // 2]
        keys, vals = rs.empty_u32(n), rs.empty_u32(n)
        rs.gen_iota(vals, base=7)
        kmax = max(ks)
        out = [(rs.empty_u32(kmax), rs.empty_u32(kmax)) for _ in range(2)]
        wsb = max(rs.topk_workspace_size(n, k, True, r) for k in ks for r in (rs.TOPK_SELECT, rs.TOPK_SORT))
        ws = rs.workspace(wsb)
        fill(keys, "uniform")
        p = rs.plan(n, 8)
        table = rs.empty_u32(p.table_entries)
        h = median_ms(lambda: rs.pass_histogram(p, keys, 24, table), args.warmup, args.reps)
        floors.append({"n": n, "histogram": h, "floor_ms": round(2 * h["ms"], 4)})
        print(json.dumps(floors[-1]), flush=True)
        del table
        for name in INPUTS:
            fill(keys, name)
            for mode in MODES:
                pairs = mode != "keys"
                for k in ks:
                    def run(route, o):
                        with rs.topk_route(route):
                            rs.topk_device(keys, k, vals=vals if mode == "vals" else None, indices=mode == "indices",
                                           out=(o[0][:k], o[1][:k] if pairs else None), ws=ws)
                    run(rs.TOPK_SELECT, out[0])
                    rep = rs.topk_report(n, k, pairs, ws)
                    run(rs.TOPK_SORT, out[1])
                    torch.cuda.synchronize()
                    same = bool(torch.equal(out[0][0][:k], out[1][0][:k])) and \
                        (not pairs or bool(torch.equal(out[0][1][:k], out[1][1][:k])))
                    row = {"n": n, "input": name, "mode": mode, "k": k, "verified": same,
                           "candidates": rep["candidates"]}
                    if not same:
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                        continue
                    row["select"] = median_ms(lambda: run(rs.TOPK_SELECT, out[0]), args.warmup, args.reps)
                    row["sort"] = median_ms(lambda: run(rs.TOPK_SORT, out[1]), args.warmup, args.reps)
                    row["sort_over_select"] = round(row["sort"]["ms"] / row["select"]["ms"], 3)
                    if name == "low16" and mode == "keys" and k <= (1 << 20):
                        try:
                            row["torch"] = median_ms(lambda: torch.topk(keys, k, largest=False, sorted=True),
                                                     1, max(3, args.reps // 3))
                        except Exception as e:  # noqa: BLE001 -- a comparator that cannot run is recorded, not fatal
                            row["torch"] = {"error": type(e).__name__}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        del keys, vals, out, ws
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "auto_limit_div": {m: n // max(1, rs.topk_auto_limit(n, m == "pairs")) for m in ("keys", "pairs")
                              for n in (1 << 26,)},
           "floors": floors, "rows": rows}
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    bad = [r for r in rows if not r["verified"]]
    print(f"{len(rows)} rows, {len(bad)} unverified -> {args.out}", flush=True)
    raise SystemExit(2 if bad else 0)


if __name__ == "__main__":
    main()
