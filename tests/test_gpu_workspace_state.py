"""GPU tests of the workspace as a state machine (DESIGN §3 "Workspace state"; include/rsort.h: the workspace's
content on entry is arbitrary, and successive calls of any plans may share one workspace on one stream).

Three families. POISONED: a workspace of exactly the planned size is filled with a pattern (zero bytes, 0xFF, 0xA5,
words equal to their index, seeded random words) before one call. CHAINS: one workspace, never touched between
calls, takes sorts of different routes and plans back to back. GRAPH REPLAY: one captured call is replayed over
inputs that need different routes, so only the device can pick them.

Every output is compared bit for bit with the oracle (Baseline1.cu:15-64 restated), numpy's stable argsort (the
partition) or, at 2^28 keys, the input's device fingerprint; check words must be 0. The only comparison between two
runs of the library is "reports, flags and kernel names equal the zero-filled run's", on top of the oracle's.
Runs on the MI355X box (-m gpu)."""
import functools
import threading
from contextlib import ExitStack, contextmanager

import numpy as np
import pytest

from _rs import rs
from _util import oracle_sort, oracle_sort_pairs, uniform_keys, zipf_cdf_u32, zipf_keys
from test_gpu_hybrid import CAP, LINE_TILE, NS, bucket_sizes, bucketed, fat_input, fat_sizes, group_plan
from test_gpu_segmented import _case1, _classes, _expected, _offsets

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERNS = ("zero", "ff", "a5", "index", "random")
INELIGIBLE = {"eligible": False, "gate": rs.GATE_NONE, "max_bucket": 0, "hybrid": False}
N_SMALL = 100003
N_RAW, N_RAW_MANY, N_TAIL = 4096 * 40 + 3, (1 << 22) + 9, (1 << 23) + 9
N_PAIRS = 512 * 8192


def dev(a):
    return rs.from_numpy_u32(a if a.flags.writeable else a.copy())  # (torch.from_numpy wants a writable array)


def zeros(n):
    return torch.zeros(n, dtype=torch.int32, device="cuda")


def poisoned(nbytes, pattern):
    """A device buffer of exactly nbytes bytes holding `pattern`."""
    assert nbytes % 4 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if pattern == "zero":
        ws.zero_()
    elif pattern == "ff":
        ws.fill_(0xFF)
    elif pattern == "a5":
        ws.fill_(0xA5)
    elif pattern == "index":  # counters that look plausible
        ws.view(torch.int32).copy_(torch.arange(nbytes // 4, dtype=torch.int32, device="cuda"))
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(0xC0FFEE)
        ws.random_(0, 256, generator=g)
    assert ws.numel() == nbytes
    return ws


@contextmanager
def settings(mode=None, groups=None, algo=None, fault=False):
    with ExitStack() as es:
        if mode is not None:
            es.enter_context(rs.hybrid(mode))
        if groups is not None:
            es.enter_context(rs.group_chunks(groups))
        if algo is not None:
            es.enter_context(rs.rank_algo(algo))
        if fault:
            es.enter_context(rs.rank_fault())
        yield


# ------------------------------------------------------------------------------ inputs (built once, never modified)
@functools.lru_cache(maxsize=None)
def overflow_keys():
    """test_capacity_edge's second input: one bucket of capacity + 1 keys."""
    big = 0x5A * 256 + 0xA5
    s = fat_sizes(NS, special=[(big, CAP)])
    donor = int(np.flatnonzero((s > 0) & (np.arange(65536) != big))[0])
    s[donor] -= 1
    s[big] += 1
    x = bucketed(s, seed=3)
    assert bucket_sizes(x).max() == CAP + 1
    return x


@functools.lru_cache(maxsize=None)
def keys(name, n):
    if name == "fat":
        assert n == NS
        x = fat_input()[0]
    elif name == "overflow":
        assert n == NS
        x = overflow_keys()
    elif name == "uniform":
        x = uniform_keys(n, seed=5)
    elif name == "uniform2":
        x = uniform_keys(n, seed=77)
    elif name == "zipf":
        x = zipf_keys(n, seed=7)
    elif name == "equal":
        x = np.full(n, 0x01234567, dtype=np.uint32)
    else:
        assert name == "sorted"
        x = np.sort(uniform_keys(n, seed=9))
    return x


@functools.lru_cache(maxsize=None)
def sorted_keys(name, n, k):
    if name == "fat" and k == 8:
        return fat_input()[1]
    return oracle_sort(keys(name, n), k)


@functools.lru_cache(maxsize=None)
def sorted_pairs(name, n, k):
    ko, vo = oracle_sort_pairs(keys(name, n), np.arange(n, dtype=np.uint32), k)
    return ko, vo


def lsd_flags(x, p):
    """rsort_group_flags of an LSD sort of x on a digit-group plan, from rs_joint_bounds' rule: pass 1 (3) takes
    the digit-0 (digit-2) groups whole (1) when the largest fits one chunk and one tile, else cuts them (2)."""
    out = []
    for d in (0, 2):
        big = int(np.bincount((x >> np.uint32(8 * d)) & np.uint32(255), minlength=256).max())
        out.append(1 if big <= p.chunk_keys + p.tile_keys else 2)
    return out


# ------------------------------------------------------------------------------ one call each
def do_sort(ws, p, k, d_x, d_want, d_v=None, d_wantv=None, inplace=False, mode=None, groups=None, algo=None,
            fault=False, stream=None):
    """One sort in `ws`: output against the oracle's (on the device, bit for bit), the check word, and what the
    sort reports about itself."""
    ptr, size = ws.data_ptr(), ws.numel()
    assert size >= p.workspace_bytes
    n = d_x.numel()
    d_in = d_x.clone() if inplace else d_x
    dv_in = d_v.clone() if (inplace and d_v is not None) else d_v
    d_out = d_in if inplace else zeros(n)
    dv_out = None if d_v is None else (dv_in if inplace else zeros(n))
    rs.scatter_kernels_used(reset=True)
    with settings(mode, groups, algo, fault):
        rs.sort_device(d_in, d_out, k, vals_in=dv_in, vals_out=dv_out, ws=ws, plan_=p, stream=stream)
    res = {"check": rs.plan_check(p, ws, stream), "report": rs.hybrid_report(p, ws, stream),
           "flags": rs.group_flags(p, ws, stream), "stats": rs.cut_plan_stats(p, ws, stream),
           "kernels": rs.scatter_kernels_used()}
    assert ws.data_ptr() == ptr and ws.numel() == size
    if fault:  # (the hook swaps ranks: the output is not the sort; the check word must say so)
        assert res["check"] & rs.CHECK_RANK_ORDER, res
        return res
    assert res["check"] == 0, res
    assert torch.equal(d_out, d_want), res
    if d_v is not None:
        assert torch.equal(dv_out, d_wantv), res
    return res


def partition_input(n, nb, large):
    x = zipf_keys(n, seed=nb + (100 if large else 0))
    if large:
        q = np.unique(x[:: max(1, n // 512)])
        split = np.sort(np.random.default_rng(nb).choice(q, size=nb - 1, replace=False)).astype(np.uint32)
    else:
        split = np.sort(uniform_keys(nb - 1, seed=nb))
    bucket = np.searchsorted(split, x, side="right")
    order = np.argsort(bucket, kind="stable")  # (test_partition_stable's reference)
    starts = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=nb))]).astype(np.uint32)
    return x, split, order, starts


def partition_bytes(n, nb, pairs):
    return int(rs._lib().rsort_partition_workspace_size(n, nb, 1 if pairs else 0))


def do_partition(ws, d_x, d_v, split, d_wantk, d_wantv, want_starts):
    ptr, size = ws.data_ptr(), ws.numel()
    n, nb, pairs = d_x.numel(), len(split) + 1, d_v is not None
    assert size >= partition_bytes(n, nb, pairs)  # (partition_device would allocate its own otherwise)
    ko, vo, starts = zeros(n), (zeros(n) if pairs else None), zeros(nb + 1)
    rs.partition_device(d_x, ko, split.tolist(), starts, vals_in=d_v, vals_out=vo, ws=ws)
    res = {"check": rs.partition_check(n, nb, pairs, ws), "starts": rs.to_numpy_u32(starts).tolist()}
    assert ws.data_ptr() == ptr and ws.numel() == size
    assert res["check"] == 0, res
    assert res["starts"] == want_starts.tolist()
    assert torch.equal(ko, d_wantk)
    if pairs:
        assert torch.equal(vo, d_wantv)
    return res


def do_segmented(ws, d_x, d_v, d_off, n, nseg, d_wantk, d_wantv, stream=None):
    ptr, size = ws.data_ptr(), ws.numel()
    pairs = d_v is not None
    assert size >= rs.segmented_workspace_size(n, nseg, pairs)
    ko, vo = zeros(n), (zeros(n) if pairs else None)
    rs.segmented_sort_device(d_x, ko, d_off, vals_in=d_v, vals_out=vo, ws=ws, stream=stream)
    flags, cc = rs.segmented_check(n, nseg, pairs, ws, stream)
    assert ws.data_ptr() == ptr and ws.numel() == size
    assert flags == 0, (flags, cc)
    assert torch.equal(ko, d_wantk)
    if pairs:
        assert torch.equal(vo, d_wantv)
    return {"flags": flags, "classes": cc}


# ------------------------------------------------------------------------------ 1. poisoned workspace
# A case: () -> (workspace bytes, run(ws) -> what the call reports, what every pattern's report must hold).
def sort_case(name, n, k, plan, pairs=False, expect=None, **kw):
    def make():
        p = plan()
        x = keys(name, n)
        if pairs:
            wk, wv = sorted_pairs(name, n, k)
            args = (dev(x), dev(wk), dev(np.arange(n, dtype=np.uint32)), dev(wv))
        else:
            args = (dev(x), dev(sorted_keys(name, n, k)))
        return p.workspace_bytes, lambda ws: do_sort(ws, p, k, *args, **kw), (expect(x, p) if expect else {})
    return make


def plan_small(k):
    def f():
        p = rs.plan(N_SMALL, k)
        assert p.tile_keys == 4096 and rs.plan_features(p) == 0, p.as_dict()
        return p
    return f


def plan_lines():
    p = rs.plan((1 << 23) + 4099, 8)
    assert p.tile_keys == LINE_TILE and p.num_chunks != 256 and rs.plan_features(p) == 0, p.as_dict()
    return p


def plan_joint():
    p = group_plan(NS)
    assert rs.plan_features(p) & rs.FEAT_GROUPS
    return p


def plan_pairs():
    p = rs.plan(N_PAIRS, 8, True, 2)
    assert p.num_chunks == 256 and p.tile_keys == 8192 and rs.plan_features(p) & rs.FEAT_GROUPS, p.as_dict()
    return p


def plan_next(n, k, tpc, raw):
    def f():
        p = rs.plan(n, k, False, tpc)
        want = rs.FEAT_NEXT_DIGIT | (rs.FEAT_RAW_TABLES if raw else rs.FEAT_TAIL_SCAN)
        assert rs.plan_features(p) == want and (p.num_chunks <= 1280) == raw, (p.as_dict(), rs.plan_features(p))
        return p
    return f


def plan_k5():
    p = rs.plan(N_SMALL, 5)
    assert p.passes == 7  # (odd: an in-place sort stages its input in the workspace)
    return p


NO_CUT_PLAN = [{"key_ranges": 0, "row_tasks": 0, "direct_adds": 0, "negative_ranges": 0}] * 2


def plain(x, p):
    return {"report": INELIGIBLE, "flags": [0, 0], "stats": NO_CUT_PLAN}


def on_groups(x, p):
    return {"report": INELIGIBLE, "flags": lsd_flags(x, p)}


def hybrid_runs(x, p):
    return {"report": {"eligible": True, "gate": rs.GATE_PASS, "max_bucket": int(bucket_sizes(x).max()),
                       "hybrid": True}, "flags": [1, 0], "stats": NO_CUT_PLAN}  # (no cut plan on this route)


def hybrid_overflows(gate):
    def f(x, p):
        big = int(bucket_sizes(x).max())
        assert big > CAP
        return {"report": {"eligible": True, "gate": gate, "max_bucket": big, "hybrid": False},
                "flags": lsd_flags(x, p)}
    return f


def partition_case(n, nb, pairs, large=False):
    def make():
        nn = n() if callable(n) else n
        x, split, order, starts = partition_input(nn, nb, large)
        v = np.arange(nn, dtype=np.uint32)
        args = (dev(x), dev(v) if pairs else None, split, dev(x[order]), dev(v[order]) if pairs else None, starts)
        return partition_bytes(nn, nb, pairs), lambda ws: do_partition(ws, *args), {}
    return make


def segmented_case(pairs):
    def make():
        lengths, off, x, v, ek, ev = _case1(pairs)
        n, nseg = x.size, len(off) - 1
        args = (dev(x), dev(v) if pairs else None, rs._device_offsets(off, "cuda"), n, nseg, dev(ek),
                dev(ev) if pairs else None)
        return (rs.segmented_workspace_size(n, nseg, pairs), lambda ws: do_segmented(ws, *args),
                {"classes": _classes(lengths, pairs)})
    return make


def large_partition_n():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8192 + 4099


FORCE = rs.HYBRID_FORCE
CASES = {
    "k8_small": sort_case("uniform", N_SMALL, 8, plan_small(8), expect=plain),
    "k8_lines_no_groups_plan": sort_case("uniform", (1 << 23) + 4099, 8, plan_lines, expect=plain),
    "joint_uniform": sort_case("uniform", NS, 8, plan_joint, expect=on_groups),
    "joint_zipf_cut": sort_case("zipf", NS, 8, plan_joint, expect=on_groups),
    "joint_groups_off": sort_case("uniform", NS, 8, plan_joint, expect=plain, groups=False),
    "joint_ballot": sort_case("uniform", NS, 8, plan_joint, expect=plain, algo=rs.RANK_BALLOT),
    "joint_pairs": sort_case("uniform", N_PAIRS, 8, plan_pairs, pairs=True, expect=on_groups),
    "hybrid_run": sort_case("fat", NS, 8, plan_joint, expect=hybrid_runs, mode=FORCE),
    "hybrid_overflow": sort_case("overflow", NS, 8, plan_joint, expect=hybrid_overflows(rs.GATE_PASS), mode=FORCE),
    "hybrid_skewed": sort_case("equal", NS, 8, plan_joint, expect=hybrid_overflows(rs.GATE_SKEWED), mode=FORCE),
    "k4_raw": sort_case("uniform", N_RAW, 4, plan_next(N_RAW, 4, 0, True), expect=plain),
    "k3_raw": sort_case("uniform", N_RAW, 3, plan_next(N_RAW, 3, 0, True), expect=plain),
    "k4_raw_1025_chunks": sort_case("uniform", N_RAW_MANY, 4, plan_next(N_RAW_MANY, 4, 1, True), expect=plain),
    "k3_raw_1025_chunks": sort_case("uniform", N_RAW_MANY, 3, plan_next(N_RAW_MANY, 3, 1, True), expect=plain),
    "k4_tail_scan": sort_case("uniform", N_TAIL, 4, plan_next(N_TAIL, 4, 1, False), expect=plain),
    "k3_tail_scan": sort_case("uniform", N_TAIL, 3, plan_next(N_TAIL, 3, 1, False), expect=plain),
    "k5_in_place": sort_case("uniform", N_SMALL, 5, plan_k5, expect=plain, inplace=True),
    "k11": sort_case("uniform", N_SMALL, 11, plan_small(11), expect=plain),
    "k13": sort_case("uniform", N_SMALL, 13, lambda: rs.plan(N_SMALL, 13), expect=plain),
    "partition_17_keys": partition_case(200003, 17, False),
    "partition_17_pairs": partition_case(200003, 17, True),
    "partition_large_keys": partition_case(large_partition_n, 17, False, large=True),
    "segmented_keys": segmented_case(False),
    "segmented_pairs": segmented_case(True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_poisoned_workspace(case):
    """Whatever the workspace held before -- every pattern, in a buffer of exactly the planned size --, the call
    gives the reference's output with a clean check word and reports the zero-filled run's route."""
    nbytes, run, expect = CASES[case]()
    base = None
    for pattern in PATTERNS:
        ws = poisoned(nbytes, pattern)
        got = run(ws)
        for key, want in expect.items():
            assert got[key] == want, (case, pattern, key, got[key], want)
        if base is None:
            base = got
        assert got == base, (case, pattern, got, base)
    if case == "joint_zipf_cut":
        assert base["flags"] == [2, 2]  # (cut plans on both odd passes, as test_zipf_keys_cut_plan)
    if case == "joint_uniform":
        assert base["flags"] == [1, 1]


# ------------------------------------------------------------------------------ 2. chains in one workspace
def stale(nbytes):
    """A chain's workspace: filled once, then never touched by the test again."""
    return poisoned((nbytes + 255) // 256 * 256, "a5")


class DeviceInputs:
    """Device copies of the cached inputs and oracle results, uploaded once per test."""

    def __init__(self):
        self.d = {}

    def get(self, name, n, k, pairs=False):
        key = (name, n, k, pairs)
        if key not in self.d:
            if pairs:
                wk, wv = sorted_pairs(name, n, k)
                self.d[key] = (dev(keys(name, n)), dev(wk), dev(np.arange(n, dtype=np.uint32)), dev(wv))
            else:
                self.d[key] = (dev(keys(name, n)), dev(sorted_keys(name, n, k)))
        return self.d[key]


def test_route_chain():
    """One digit-group plan, one workspace, twelve sorts whose routes differ: each finds what the route before it
    left behind (after a hybrid run: prefix sums in the joint counts and RUN in the mode word)."""
    p = plan_joint()
    ws = stale(p.workspace_bytes)
    ptr = ws.data_ptr()
    di = DeviceInputs()
    OFF = rs.HYBRID_OFF

    def step(name, expect, **kw):
        x = keys(name, NS)
        res = do_sort(ws, p, 8, *di.get(name, NS, 8), **kw)
        assert ws.data_ptr() == ptr
        for key, want in expect(x, p).items():
            assert res[key] == want, (name, kw, key, res[key], want)
        return res

    step("uniform", hybrid_runs, mode=FORCE)                                     # 1
    assert step("uniform", on_groups, mode=OFF)["flags"] == [1, 1]               # 2
    step("overflow", hybrid_overflows(rs.GATE_PASS), mode=FORCE)                 # 3
    step("fat", hybrid_runs, mode=FORCE)                                         # 4
    step("equal", hybrid_overflows(rs.GATE_SKEWED), mode=FORCE)                  # 5
    step("fat", hybrid_runs, mode=FORCE)                                         # 6
    assert step("uniform", on_groups, mode=FORCE, inplace=True)["flags"] == [1, 1]  # 7 (in place: ineligible)
    step("fat", hybrid_runs, mode=FORCE)                                         # 8
    assert step("zipf", on_groups, mode=OFF)["flags"] == [2, 2]                  # 9 (cut plans)
    assert step("uniform", on_groups, mode=OFF)["flags"] == [1, 1]               # 10
    res = do_sort(ws, p, 8, *di.get("fat", NS, 8), mode=FORCE, fault=True)       # 11 (CHECK_RANK_ORDER is set)
    assert res["report"]["hybrid"]
    step("fat", hybrid_runs, mode=FORCE)                                         # 12 (check 0 again)


def test_plan_chain():
    """The same bytes carved by ten plans in turn, then by the same ten in reverse order: one call's keys and
    tables are the next call's control words."""
    di = DeviceInputs()
    pj, pp = plan_joint(), plan_pairs()
    p4r, p4t = plan_next(N_RAW, 4, 0, True)(), plan_next(N_TAIL, 4, 1, False)()
    p3, p8, p5 = plan_next(N_RAW, 3, 0, True)(), plan_small(8)(), plan_k5()
    lengths, off, sx, sv, ek, ev = _case1(True)
    seg = (dev(sx), dev(sv), rs._device_offsets(off, "cuda"), sx.size, len(off) - 1, dev(ek), dev(ev))
    px, split, order, starts = partition_input(200003, 17, False)
    pv = np.arange(px.size, dtype=np.uint32)
    part = (dev(px), dev(pv), split, dev(px[order]), dev(pv[order]), starts)
    nbytes = max([p.workspace_bytes for p in (pj, pp, p4r, p4t, p3, p8, p5)] +
                 [rs.segmented_workspace_size(sx.size, len(off) - 1, True), partition_bytes(px.size, 17, True)])
    ws = stale(nbytes)
    ptr = ws.data_ptr()

    def hybrid_run():
        res = do_sort(ws, pj, 8, *di.get("fat", NS, 8), mode=FORCE)
        assert res["report"] == hybrid_runs(keys("fat", NS), pj)["report"], res

    def ineligible(p, k, name, n, pairs=False, flags=None, **kw):
        def f():
            res = do_sort(ws, p, k, *di.get(name, n, k, pairs), **kw)
            assert res["report"] == INELIGIBLE and res["flags"] == (flags or [0, 0]), res
        return f

    steps = [
        hybrid_run,
        ineligible(pp, 8, "uniform", N_PAIRS, pairs=True, flags=[1, 1]),
        ineligible(p4r, 4, "uniform", N_RAW),
        ineligible(p4t, 4, "uniform", N_TAIL),
        ineligible(p3, 3, "uniform", N_RAW),
        ineligible(p8, 8, "uniform", N_SMALL),
        lambda: do_segmented(ws, *seg),  # (the workspace's leading bytes)
        lambda: do_partition(ws, *part),
        ineligible(p5, 5, "uniform", N_SMALL, inplace=True),
        hybrid_run,
    ]
    for f in steps + steps[::-1]:
        f()
        assert ws.data_ptr() == ptr and ws.numel() >= nbytes


def test_automatic_route_chain():
    """The smallest automatically eligible size, one workspace under AUTO: uniform (hybrid), Zipf (the gate says
    skewed: the LSD passes find the joint counts as the memset left them -- the only way into that state), uniform,
    all-equal, uniform. Generated and verified on the device: sorted, with the input's multiset fingerprint."""
    n = rs.hybrid_range()[0]
    p = rs.plan(n, 8)
    assert p.num_chunks == 256 and rs.plan_features(p) & rs.FEAT_GROUPS, p.as_dict()
    assert rs.get_hybrid() == rs.HYBRID_AUTO
    inp, out = rs.empty_u32(n), rs.empty_u32(n)
    ws = rs.workspace(p.workspace_bytes)
    ptr = ws.data_ptr()
    cdf = rs.from_numpy_u32(zipf_cdf_u32())

    def step(kind, seed=0):
        if kind == "uniform":
            rs.gen_uniform(inp, seed)
        elif kind == "zipf":
            rs.gen_zipf(inp, cdf, seed)
        else:
            inp.fill_(0x01234567)
        fp = rs.fingerprint(inp)[0]
        out.zero_()
        rs.sort_device(inp, out, 8, ws=ws, plan_=p)
        rep = rs.hybrid_report(p, ws)
        assert ws.data_ptr() == ptr
        assert rs.plan_check(p, ws) == 0, (kind, rep)
        assert rs.fingerprint(out) == (fp, 0), (kind, rep)
        if kind == "uniform":
            assert rep["eligible"] and rep["gate"] == rs.GATE_PASS and 0 < rep["max_bucket"] <= CAP and rep["hybrid"], rep
            assert rs.group_flags(p, ws) == [1, 0]
        else:
            assert rep == {"eligible": True, "gate": rs.GATE_SKEWED, "max_bucket": 0, "hybrid": False}, (kind, rep)
            assert rs.group_flags(p, ws) == [2, 2]

    step("uniform", 0x5EED)
    step("zipf", 0x5EED)
    step("uniform", 0xBEEF)
    step("equal")
    step("uniform", 0x5EED)


def topk_want(x, k, largest=False, vals=None, indices=False, sorted=True):
    """numpy's statement of the top-k contract for every row of a 2-D x (include/rsort.h): the first k of the stable
    argsort of key ^ m; unsorted, the same entries in column order (what the row-wise select writes)."""
    m = np.uint32(0xFFFFFFFF if largest else 0)
    idx = np.argsort(x ^ m, axis=1, kind="stable")[:, :k]
    if not sorted:
        idx = np.sort(idx, axis=1)
    wv = idx.astype(np.uint32) if indices else None if vals is None else np.take_along_axis(vals, idx, 1)
    return np.take_along_axis(x, idx, 1), wv


def check_host_topk(x, k, **kw):
    gk, gv = rs.topkByDevice(x, k, **kw)
    wk, wv = topk_want(x[None, :], k, **kw)
    assert np.array_equal(gk, wk[0]) and (gv is None) == (wv is None), (x.size, k, kw)
    assert wv is None or np.array_equal(gv, wv[0]), (x.size, k, kw)


def check_host_topk_rows(x, rows, cols, k, vals=False, **kw):
    mat = np.resize(x, rows * cols).reshape(rows, cols)  # (the keys again from the start where x is shorter)
    v = (np.arange(rows * cols, dtype=np.uint32) * np.uint32(3)).reshape(rows, cols) if vals else None
    gk, gv = rs.topkRowsByDevice(mat, k, vals_2d=v, **kw)
    wk, wv = topk_want(mat, k, vals=v, **kw)
    assert np.array_equal(gk, wk) and (gv is None) == (wv is None), (x.size, rows, cols, k, kw)
    assert wv is None or np.array_equal(gv, wv), (x.size, rows, cols, k, kw)


def test_host_entries_share_the_cached_buffer():
    """The host entries carve one cached device buffer differently for every (n, k, pairs): sizes that shrink and
    grow, each call against the oracle (a non-zero status -- the check word among them -- raises). The top-k entries
    between the sorts put regions of k entries and their own workspaces into the same buffer."""
    for n, k in zip((70001, 1 << 20, 513, 250001), (8, 4, 5, 12)):
        x = uniform_keys(n, seed=n)
        v = np.arange(n, dtype=np.uint32)
        want = oracle_sort(x, k)
        out = np.zeros_like(x)
        rs.sortByDevice(x, n, out, k)
        assert np.array_equal(out, want), (n, k)
        check_host_topk(x, n // 7, largest=True)
        ko, vo = np.zeros_like(x), np.zeros_like(v)
        rs.sortPairsByDevice(x, v, n, ko, vo, k)
        wk, wv = oracle_sort_pairs(x, v, k)
        assert np.array_equal(ko, wk) and np.array_equal(vo, wv), (n, k)
        check_host_topk_rows(x, 37, 300, 17)
        lengths = [n // 5, 0, 1, n // 3, min(300, n // 8), 64 if n > 1000 else 5]
        off = _offsets(lengths + [n - sum(lengths) - 7], start=3)
        ko, vo = np.zeros_like(x), np.zeros_like(v)
        rs.sortSegmentsByDevice(x, off, ko, vals=v, vals_out=vo)
        ek, ev = _expected(x, v, off)
        assert np.array_equal(ko, ek) and np.array_equal(vo, ev), n
        check_host_topk(x, n // 7, indices=True)
        check_host_topk_rows(x, 5, 20000, 17, vals=True, largest=True, sorted=False)
        out = np.zeros_like(x)
        rs.sortByDevice(x, n, out, k)
        assert np.array_equal(out, want), (n, k)


def test_host_entries_hold_the_cache_lock():
    """Two threads, four host calls each on the one cached buffer of the device (ctypes releases the GIL): the sorts
    in one, the top-k entries in the other. An entry that let go of the cache's lock before its last copy had
    landed would have its regions overwritten by the other thread's call."""
    n = 1 << 18
    x = zipf_keys(n, seed=7)
    v = np.arange(n, dtype=np.uint32)
    off = _offsets([n // 3, 0, 5000, n // 2, 77], start=11)
    sort_want, seg_want = oracle_sort(x, 8), _expected(x, v, off)
    errors = []

    def sorts():
        for _ in range(2):
            out = np.zeros_like(x)
            rs.sortByDevice(x, n, out, 8)
            assert np.array_equal(out, sort_want)
            ko, vo = np.zeros_like(x), np.zeros_like(v)
            rs.sortSegmentsByDevice(x, off, ko, vals=v, vals_out=vo)
            assert np.array_equal(ko, seg_want[0]) and np.array_equal(vo, seg_want[1])

    def topks():
        for largest in (False, True):
            check_host_topk(x, n // 7, largest=largest, indices=True)
            check_host_topk_rows(x, 64, 4096, 17, vals=True, largest=largest)

    def guarded(fn):
        def run():
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 -- reported by the test's own thread
                errors.append((fn.__name__, repr(e)))
        return threading.Thread(target=run)

    threads = [guarded(sorts), guarded(topks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ------------------------------------------------------------------------------ 3. graph replay
def captured(call):
    """`call` run once uncaptured (the lane-order probe and the occupancy queries happen there), then captured
    alone, once, on a side stream. Returns (graph, stream); replays and reads go on that stream."""
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        call()
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        call()
    return g, st


def test_graph_replay_hybrid_follows_the_data():
    """One captured FORCE sort holds both kernel sequences; the device picks one per replay from the keys in the
    captured input buffer: hybrid, overflow (LSD), skewed (LSD), hybrid, hybrid."""
    p = plan_joint()
    names = ("fat", "overflow", "equal", "fat", "uniform")
    src = {nm: (dev(keys(nm, NS)), dev(sorted_keys(nm, NS, 8))) for nm in set(names)}
    d_in, d_out = dev(keys("uniform2", NS)), zeros(NS)
    ws = stale(p.workspace_bytes)
    with rs.hybrid(FORCE):
        g, st = captured(lambda: rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p))
    with torch.cuda.stream(st):
        for nm in names:
            x = keys(nm, NS)
            d_in.copy_(src[nm][0])
            d_out.zero_()
            g.replay()
            rep, chk = rs.hybrid_report(p, ws, st), rs.plan_check(p, ws, st)
            big = int(bucket_sizes(x).max())
            gate = rs.GATE_SKEWED if nm == "equal" else rs.GATE_PASS
            assert rep == {"eligible": True, "gate": gate, "max_bucket": big, "hybrid": big <= CAP}, (nm, rep)
            assert chk == 0, (nm, rep)
            assert rs.group_flags(p, ws, st) == ([1, 0] if big <= CAP else lsd_flags(x, p)), nm
            if big <= CAP:
                assert rs.cut_plan_stats(p, ws, st) == NO_CUT_PLAN, nm
            assert torch.equal(d_out, src[nm][1]), (nm, rep)
        st.synchronize()


def test_graph_replay_raw_tables():
    """k = 4 raw tables: the three-table rotation must end every execution in the state in which it started."""
    p = plan_next(N_RAW, 4, 0, True)()
    names = ("uniform", "equal", "sorted")
    src = {nm: (dev(keys(nm, N_RAW)), dev(sorted_keys(nm, N_RAW, 4))) for nm in names}
    d_in, d_out = dev(keys("uniform2", N_RAW)), zeros(N_RAW)
    ws = stale(p.workspace_bytes)
    g, st = captured(lambda: rs.sort_device(d_in, d_out, 4, ws=ws, plan_=p))
    with torch.cuda.stream(st):
        for nm in names:
            d_in.copy_(src[nm][0])
            d_out.zero_()
            g.replay()
            assert rs.plan_check(p, ws, st) == 0, nm
            assert torch.equal(d_out, src[nm][1]), nm
        st.synchronize()


def test_graph_replay_pairs():
    n = 250001
    p = rs.plan(n, 8, True)
    names = ("uniform", "zipf")
    src = {nm: (dev(keys(nm, n)),) + tuple(dev(a) for a in sorted_pairs(nm, n, 8)) for nm in names}
    d_in, d_v = dev(keys("uniform2", n)), dev(np.arange(n, dtype=np.uint32))
    d_out, dv_out = zeros(n), zeros(n)
    ws = stale(p.workspace_bytes)
    g, st = captured(lambda: rs.sort_device(d_in, d_out, 8, vals_in=d_v, vals_out=dv_out, ws=ws, plan_=p))
    with torch.cuda.stream(st):
        for nm in names:
            d_in.copy_(src[nm][0])
            d_out.zero_()
            dv_out.zero_()
            g.replay()
            assert rs.plan_check(p, ws, st) == 0, nm
            assert torch.equal(d_out, src[nm][1]) and torch.equal(dv_out, src[nm][2]), nm  # (stable)
        st.synchronize()


def test_graph_replay_segmented():
    lengths, off, x, v, ek, ev = _case1(True)
    n, nseg = x.size, len(off) - 1
    x2 = zipf_keys(n, seed=4243)
    ek2, ev2 = _expected(x2, v, off)
    src = [(dev(x), dev(ek), dev(ev)), (dev(x2), dev(ek2), dev(ev2))]
    d_in, d_v, d_off = dev(uniform_keys(n, seed=1)), dev(v), rs._device_offsets(off, "cuda")
    d_out, dv_out = zeros(n), zeros(n)
    ws = stale(rs.segmented_workspace_size(n, nseg, True))
    g, st = captured(lambda: rs.segmented_sort_device(d_in, d_out, d_off, vals_in=d_v, vals_out=dv_out, ws=ws))
    with torch.cuda.stream(st):
        for kx, wk, wv in src:
            d_in.copy_(kx)
            d_out.zero_()
            dv_out.zero_()
            g.replay()
            flags, cc = rs.segmented_check(n, nseg, True, ws, st)
            assert flags == 0 and cc == _classes(lengths, True), (flags, cc)
            assert torch.equal(d_out, wk) and torch.equal(dv_out, wv)
        st.synchronize()
