"""Lab: the row-wise top-k against what it replaces (DESIGN §5c's table; profiles/topk_rows.json).

    python dev/topk_rows_lab.py [--reps 10] [--warmup 3] [--out profiles/topk_rows.json] [--quick]

For rows x cols = 2^26 keys in the shapes 2^20 x 64 (k = 2, 8: MoE gating), 2^16 x 2^10 (k = 1, 16, 256), 2^12 x 2^14
(k = 16, 1024, cols / 2), 2^8 x 2^18 (k = 64) and 8 x 2^23 (k = 64), keys only / values / indices, smallest first, on
uniform keys and on keys below 2^10 (every level but the last two keeps every candidate):
    rows      rs.topk_rows, sorted output
    unsorted  the same call with sorted=False: the select alone; finish_share = 1 - unsorted / rows is the share
              of the call spent in the finishing sort (offsets + segmented sort of rows x k)
    sort      rs.sort_rows of all rows x cols keys and a slice [:, :k] made contiguous: what a caller had before
              (with indices its values are a column-index matrix built once, outside the timed window)
    loop      rs.topk_device row by row over the first min(rows, 256) rows, scaled to all rows as dev/seg_lab.py
              scales its loop
    torch     torch.topk(dim=1) on the int32 view, for the keys below 2^10 only (below 2^31 the signed order is the
              unsigned one); it returns keys and indices in one call, so it stands in the keys and the indices rows
HIP-event medians of `reps` timed calls after `warmup`; spread = (max - min) / median. Before anything is timed
the new call's output is compared, every element, with the sort-and-slice's. The floor is one read of the 2^26
keys at the library's own histogram rate (rsort_pass_histogram of the top digit), timed in the same process.

(profiles/topk_rows_wave_select.json is the record of the wave class's two selects, LDS counters against a bit-by-bit
select from registers, measured by an earlier form of this lab before the slower one was removed.)"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "cuda.radixsort_amd"))
import radixsort as rs  # noqa: E402
import torch  # noqa: E402

SHAPES = (((1 << 20, 64), (2, 8)), ((1 << 16, 1 << 10), (1, 16, 256)), ((1 << 12, 1 << 14), (16, 1024, 1 << 13)),
          ((1 << 8, 1 << 18), (64,)), ((8, 1 << 23), (64,)))
QUICK = (((1 << 12, 64), (2,)), ((1 << 8, 1 << 10), (16,)), ((16, 1 << 14), (16,)), ((2, 1 << 18), (64,)))
INPUTS = ("uniform", "low10")
MODES = ("keys", "vals", "indices")


def fill(keys, name):
    rs.gen_uniform(keys.view(-1), seed=0x5EED)
    if name == "low10":
        keys.bitwise_right_shift_(22).bitwise_and_(0x3FF)
    torch.cuda.synchronize()


def timed(fn, warmup: int, reps: int):
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
    med = statistics.median(ts)
    return {"ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "spread": round((max(ts) - min(ts)) / med, 4)}


class Bench:
    """Buffers for one shape; every call it times writes into them."""

    def __init__(self, rows, cols, kmax):
        self.rows, self.cols = rows, cols
        n = rows * cols
        new = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")  # noqa: E731
        self.keys, self.vals = new(rows, cols), new(rows, cols)
        rs.gen_iota(self.vals.view(-1), base=7)
        self.colidx = torch.arange(cols, dtype=torch.int32, device="cuda").repeat(rows, 1).contiguous()
        self.sk, self.sv = new(rows, cols), new(rows, cols)
        self.flat_out = (new(rows * kmax), new(rows * kmax))
        self.sort_ws = rs.workspace(rs.segmented_workspace_size(n, rows, True))
        self.sort_off = torch.arange(rows + 1, dtype=torch.int64, device="cuda") * cols
        self.ws = rs.workspace(rs.topk_rows_workspace_size(rows, cols, kmax, True))
        self.loop_rows = min(rows, 256)
        self.loop_ws = rs.workspace(rs.topk_workspace_size(cols, kmax, True, rs.get_topk_route()))
        self.loop_out = (new(kmax), new(kmax))

    def out(self, k, pairs):
        n = self.rows * k
        return self.flat_out[0][:n].view(self.rows, k), self.flat_out[1][:n].view(self.rows, k) if pairs else None

    def new_call(self, k, mode, sorted_=True):
        pairs = mode != "keys"
        return rs.topk_rows(self.keys, k, vals_2d=self.vals if mode == "vals" else None, indices=mode == "indices",
                            sorted=sorted_, out=self.out(k, pairs), ws=self.ws)

    def sort_slice(self, k, mode):
        v = self.vals if mode == "vals" else self.colidx if mode == "indices" else None
        rs.segmented_sort_device(self.keys, self.sk, self.sort_off, v, self.sv if v is not None else None,
                                 ws=self.sort_ws)
        return self.sk[:, :k].contiguous(), self.sv[:, :k].contiguous() if v is not None else None

    def loop(self, k, mode):
        pairs = mode != "keys"
        for r in range(self.loop_rows):
            rs.topk_device(self.keys[r], k, vals=self.vals[r] if mode == "vals" else None, indices=mode == "indices",
                           out=(self.loop_out[0][:k], self.loop_out[1][:k] if pairs else None), ws=self.loop_ws)

    def verified(self, k, mode):
        ko, vo, _ = self.new_call(k, mode)
        sk, sv = self.sort_slice(k, mode)
        torch.cuda.synchronize()
        flags, rep = rs.topk_rows_check(self.rows, self.cols, k, mode != "keys", self.ws)
        same = bool(torch.equal(ko, sk)) and (vo is None or bool(torch.equal(vo, sv))) and flags == 0 and rep[1] == 0
        return same, rep[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/topk_rows.json")
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of every path, not a measurement")
    args = ap.parse_args()
    rows_out, floors = [], []
    for (rows, cols), ks in (QUICK if args.quick else SHAPES):
        n = rows * cols
        b = Bench(rows, cols, max(ks))
        fill(b.keys, "uniform")
        p = rs.plan(n, 8)
        table = rs.empty_u32(p.table_entries)
        h = timed(lambda: rs.pass_histogram(p, b.keys.view(-1), 24, table), args.warmup, args.reps)
        floors.append({"rows": rows, "cols": cols, "histogram": h, "floor_ms": h["ms"]})
        print(json.dumps(floors[-1]), flush=True)
        del table
        for name in INPUTS:
            fill(b.keys, name)
            for mode in MODES:
                for k in ks:
                    ok, cls = b.verified(k, mode)
                    row = {"rows": rows, "cols": cols, "k": k, "input": name, "mode": mode, "kernel": cls,
                           "verified": ok}
                    if ok:
                        row["rows_call"] = timed(lambda: b.new_call(k, mode), args.warmup, args.reps)
                        row["unsorted"] = timed(lambda: b.new_call(k, mode, False), args.warmup, args.reps)
                        row["sort"] = timed(lambda: b.sort_slice(k, mode), args.warmup, args.reps)
                        lp = timed(lambda: b.loop(k, mode), 1, 3)
                        scale = rows / b.loop_rows
                        row["loop"] = {"ms": round(lp["ms"] * scale, 3), "spread": lp["spread"], "rows_run": b.loop_rows}
                        if name == "low10" and mode != "vals":
                            try:
                                row["torch"] = timed(lambda: torch.topk(b.keys, k, dim=1, largest=False, sorted=True),
                                                     1, max(3, args.reps // 3))
                            except Exception as e:  # noqa: BLE001 -- a comparator that cannot run is recorded, not fatal
                                row["torch"] = {"error": type(e).__name__}
                        t = row["rows_call"]["ms"]
                        row["finish_share"] = round(max(0.0, 1 - row["unsorted"]["ms"] / t), 3)
                        row["sort_over_rows"] = round(row["sort"]["ms"] / t, 3)
                        row["loop_over_rows"] = round(row["loop"]["ms"] / t, 1)
                        row["rows_over_floor"] = round(t / h["ms"], 2)
                        # faster than sort-and-slice by more than the two medians' spreads, or named as open
                        row["open"] = not row["sort"]["ms"] > t * (1 + max(row["rows_call"]["spread"], row["sort"]["spread"]))
                    rows_out.append(row)
                    print(json.dumps(row), flush=True)
        del b
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "quick": args.quick,
           "floors": floors, "rows": rows_out}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    bad = [r for r in rows_out if not r["verified"]]
    print(f"{len(rows_out)} rows, {len(bad)} unverified -> {args.out}", flush=True)
    raise SystemExit(2 if bad else 0)


if __name__ == "__main__":
    main()
