"""GPU: a failed on-device self-check reaches the caller from EVERY entry that runs a checked sort, not only from the
plain sort, the hybrid route, the segmented sort and the partition (tests/test_gpu_check.py and their own files).

The two test hooks make a sort's output wrong and its check word non-zero (rsort_inject_rank_fault: CHECK_RANK_ORDER;
rsort_inject_table_fault: CHECK_TABLE on raw-table sorts); they never make the device fault. Both are process-wide,
so rsort_inject_fault_window (rs.fault_window) narrows them to chosen sort calls of one thread: a loopback rank can
fault exactly one of its sorts and neither its partition nor another rank. Every comparison is bit-exact against the
oracle (tests/_util.py) or np.sort. A fault acts only on a full tile, so every case first asserts its precondition
(a plain sort of that size trips the check / the plan takes raw tables) and FAILS, never skips, without it.

Which test catches which read of a check word (delete the read, the test fails):
  rsort_u32_multi*   the sample sort's word          test_multi_sample_sort_faulted_alone
                     the lower half's slot           test_multi_each_half_faulted_alone[...-lower] (one word shared
                                                     by both halves and read at the end fails it too: the upper
                                                     half's pass 0 clears what the lower half's sort recorded)
                     the upper half's slot           test_multi_each_half_faulted_alone[...-upper], test_multi_table_fault
                     the direct sort's slot          test_multi_direct_and_whole_protocol_at_world_1
  rsort_topk_report  report8[6] / rsort_u32_topk     test_topk_faulted_and_clean
  multi.py           the sample sort's, partition's  test_dist_sort_rank_fault_raises_on_both_ranks here (either one),
                                                     tests/test_multi.py ..._before_the_exchange_...[sample / partition]
                                                     (each alone, no GPU)
                     the final sort's                test_dist_sort_table_fault_raises_on_that_rank_alone here,
                                                     tests/test_multi.py ..._of_the_final_sort_... (no GPU)
  pinned, not new    rsort_topk_rows_check, rsort_u32_topk_rows, rsort_u32_pairs: test_topk_rows_*, test_host_pairs_*
Runs on the MI355X box (-m gpu)."""
import contextlib
import functools
import os
import socket
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

from _rs import rs
from _util import TOPK_ROWS_CLASS_COLS, oracle_sort_pairs, uniform_keys

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = Path(__file__).resolve().parent.parent / "cuda.radixsort_amd"

N = (1 << 22) + 17        # plain sorts, the top-k input (as tests/test_gpu_check.py)
K_TOP = 1 << 18           # the top-k's k: the finishing sort of the SELECT route has full tiles
N_MULTI = (1 << 21) + 17  # keys per rank of the multi-GPU sorts
NOTHING = (0, 0)          # a window that admits no sort call: this rank's sorts run clean under the hooks


# ------------------------------------------------------------------------------ preconditions
@functools.lru_cache(maxsize=None)
def rank_fault_acts(n, k, pairs, inplace, hybrid=False):
    """A plain rs.sort_device of n keys, under the rank hook, sets CHECK_RANK_ORDER (it has a checked full tile)."""
    x = rs.from_numpy_u32(uniform_keys(n, seed=1 + (n & 0xFFFF)))
    v = rs.from_numpy_u32(np.arange(n, dtype=np.uint32)) if pairs else None
    p = rs.plan(n, k, pairs)
    ws = rs.workspace(p.workspace_bytes)
    with rs.rank_fault():
        rs.sort_device(x, x if inplace else rs.empty_u32(n), k, vals_in=v,
                       vals_out=None if not pairs else v if inplace else rs.empty_u32(n), ws=ws, plan_=p, hybrid=hybrid)
        return bool(rs.plan_check(p, ws) & rs.CHECK_RANK_ORDER)


def raw_tables(n, k):
    return bool(rs.plan_features(rs.plan(n, k, False)) & rs.FEAT_RAW_TABLES)


# ------------------------------------------------------------------------------ the window itself, on the device
def test_fault_window_faults_exactly_its_sort_calls():
    """Under the rank hook with rs.fault_window(1, 2): of four plain sorts the second and third report
    CHECK_RANK_ORDER and come out wrong, the first and fourth are clean and exact; a partition inside the window is
    no sort call and sees no hook. Cleared, every sort and the partition see the hook again."""
    n = N
    assert rank_fault_acts(n, 8, False, False)
    x = uniform_keys(n, seed=3)
    want = np.sort(x)
    d = rs.from_numpy_u32(x)
    out = rs.empty_u32(n)
    p = rs.plan(n, 8)
    ws = rs.workspace(p.workspace_bytes)
    spl = [1 << 30, 1 << 31, 3 << 30]
    starts = torch.empty(len(spl) + 2, dtype=torch.int32, device="cuda")
    pws = rs.workspace(int(rs._lib().rsort_partition_workspace_size(n, len(spl) + 1, 0)))
    with rs.rank_fault():
        with rs.fault_window(1, 2):
            seen = []
            for i in range(4):
                rs.sort_device(d, out, 8, ws=ws, plan_=p, hybrid=False)
                seen.append((rs.plan_check(p, ws), bool(np.array_equal(rs.to_numpy_u32(out), want))))
                assert rs.fault_window_calls() == i + 1
            assert seen == [(0, True), (rs.CHECK_RANK_ORDER, False), (rs.CHECK_RANK_ORDER, False), (0, True)]
            rs.partition_device(d, out, spl, starts, ws=pws)
            assert rs.partition_check(n, len(spl) + 1, False, pws) == 0
            assert rs.fault_window_calls() == 4
        rs.sort_device(d, out, 8, ws=ws, plan_=p, hybrid=False)
        assert rs.plan_check(p, ws) == rs.CHECK_RANK_ORDER
        rs.partition_device(d, out, spl, starts, ws=pws)
        assert rs.partition_check(n, len(spl) + 1, False, pws) & rs.CHECK_RANK_ORDER


# ------------------------------------------------------------------------------ multi-GPU sort, C path (loopback)
@functools.lru_cache(maxsize=None)
def multi_inputs(world, pairs):
    keys = [uniform_keys(N_MULTI, seed=700 + r) for r in range(world)]
    vals = [np.arange(N_MULTI, dtype=np.uint32) + np.uint32(r << 24) for r in range(world)] if pairs else [None] * world
    return tuple(zip(keys, vals))


@functools.lru_cache(maxsize=None)
def multi_want(world, pairs):
    """The oracle's order of the union of the ranks' inputs (the same for every k_bits); computed once, never changed."""
    inp = multi_inputs(world, pairs)
    keys = np.concatenate([k for k, _ in inp])
    if not pairs:
        wk, wv = np.sort(keys), None
    else:
        wk, wv = oracle_sort_pairs(keys, np.concatenate([v for _, v in inp]), 8)
        wv.setflags(write=False)
    wk.setflags(write=False)
    return wk, wv


class Ranks:
    """The loopback ranks of one test (the pattern of tests/test_gpu_multi.py's _run_loopback): inputs, outputs and
    workspaces live as long as the object, so every run() sorts in the SAME workspaces."""

    def __init__(self, world, pairs, k):
        torch.cuda.set_device(0)
        self.world, self.pairs, self.k = world, pairs, k
        self.cap = rs.default_capacity(N_MULTI)
        self.inp = [(rs.from_numpy_u32(kx), rs.from_numpy_u32(vx) if pairs else None)
                    for kx, vx in multi_inputs(world, pairs)]
        wsb = int(rs._lib().rsort_multi_workspace_size(N_MULTI, self.cap, k, 1 if pairs else 0, world))
        self.ws = [rs.workspace(wsb) for _ in range(world)]
        self.out = [(rs.empty_u32(self.cap), rs.empty_u32(self.cap) if pairs else None) for _ in range(world)]

    def run(self, opts, windows=None):
        """One multi-GPU sort, a thread per rank. opts: rsort_set_multi_options flags (0: no overlap flag, the
        automatic overlap). windows[r]: rank r's rs.fault_window arguments, or None. Returns (per rank: (keys, vals,
        offset) or the RSortError status; per rank: the sort calls its thread started)."""
        world = self.world
        grp = rs.LoopbackGroup(world)
        old = rs.set_multi_options(opts)
        res, calls = [None] * world, [None] * world

        def run(r):
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            win = windows[r] if windows is not None else None
            try:
                with torch.cuda.stream(st), (rs.fault_window(*win) if win is not None else contextlib.nullcontext()):
                    try:
                        ok, ov, off = rs.multi_sort_device(grp.transport(r), self.inp[r][0], self.k,
                                                           vals=self.inp[r][1], capacity=self.cap, stream=st,
                                                           ws=self.ws[r], out=self.out[r])
                        st.synchronize()
                        res[r] = (rs.to_numpy_u32(ok), rs.to_numpy_u32(ov) if ov is not None else None, off)
                    except rs.RSortError as e:
                        res[r] = e.status
                    calls[r] = rs.fault_window_calls()
                    st.synchronize()
            except Exception as e:  # noqa: BLE001 -- shown by the caller's assert
                res[r] = repr(e)

        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        alive = any(t.is_alive() for t in th)
        rs.set_multi_options(old)
        assert not alive, "loopback ranks did not finish"
        grp.close()
        return res, calls

    def assert_exact(self, res, failed=()):
        """Every rank outside `failed` holds its slice of the oracle's order at its offset; the failed ones returned
        RSORT_ERR_CHECK."""
        wk, wv = multi_want(self.world, self.pairs)
        brief = [x if not isinstance(x, tuple) else ("ok", x[0].size, x[2]) for x in res]
        for r, x in enumerate(res):
            if r in failed:
                assert x == 11, (r, brief)
                continue
            assert isinstance(x, tuple), (r, brief)
            gk, gv, off = x
            assert gk.size > 0 and np.array_equal(gk, wk[off:off + gk.size]), (r, brief)
            if self.pairs:
                assert np.array_equal(gv, wv[off:off + gk.size]), (r, brief)
        if 0 not in failed:
            assert res[0][2] == 0, brief
        if self.world - 1 not in failed:
            assert res[-1][2] + res[-1][0].size == wk.size, brief
        if not failed:
            assert [x[2] for x in res] == list(np.cumsum([0] + [x[0].size for x in res[:-1]])), brief


@pytest.mark.parametrize("half", ["lower", "upper"])
@pytest.mark.parametrize("world,pairs", [(2, False), (2, True), (3, False), (3, True)])
def test_multi_each_half_faulted_alone(world, pairs, half):
    """No overlap flag, so ranks 2 and 3 worlds sort two halves each, one after the other in ONE sort workspace.
    Rank 1 faults only its lower-half sort (its sort call 1; 0 is the sample sort, 2 the upper half) or only its
    upper-half sort: rank 1 returns RSORT_ERR_CHECK (11), every other rank its exact slice. An implementation that
    reads one shared check word when both halves have run fails the lower-half case: the upper half's pass 0 clears
    the word. Then, hooks cleared, one more sort in the same workspaces is exact on every rank."""
    # (a half holds about N_MULTI / 2 keys, the sample's error apart: the precondition at 9 / 10 of that, in place)
    assert rank_fault_acts(N_MULTI // 2 * 9 // 10, 8, pairs, True)
    ranks = Ranks(world, pairs, 8)
    windows = [NOTHING] * world
    windows[1] = (1 if half == "lower" else 2, 1)
    with rs.rank_fault():
        res, calls = ranks.run(0, windows)
    assert calls == [3] * world, calls  # sample sort, lower half, upper half: the numbering the windows assume
    ranks.assert_exact(res, failed=(1,))
    res, _ = ranks.run(0)
    ranks.assert_exact(res)


def test_multi_sample_sort_faulted_alone():
    """Rank 1 faults only its sort of the gathered sample (its sort call 0). Where that sort has a checked full tile
    (the precondition, asserted on a plain sort of the same key count), its quantiles may be unsorted: every rank
    returns 11 together, before any key moves. Where it has none the fault cannot act, and every rank's output is
    exact. The branch that ran is in the assertion message."""
    world = 2
    n_all = [0] * (2 * world)
    n_all[0::2] = [N_MULTI] * world  # (two halves per rank: the sampling plan is made for 2 x world virtual ranks)
    sp = rs.multi_sample_plan(n_all, max(1, (1 << 20) // (2 * world)))
    ns = world * (sp.row_len + 1)    # the gathered rows, each with its status word
    acts = rank_fault_acts(ns, 8, False, True)
    ranks = Ranks(world, False, 8)
    with rs.rank_fault():
        res, calls = ranks.run(0, [NOTHING, (0, 1)])
    branch = f"sample sort of {ns} keys: the fault {'acts' if acts else 'cannot act'}"
    if acts:
        assert res == [11] * world, (branch, [x if not isinstance(x, tuple) else "ok" for x in res])
        assert calls == [1] * world, (branch, calls)  # nobody got past the partition
    else:
        assert calls == [3] * world, (branch, calls)
        ranks.assert_exact(res)
    res, _ = ranks.run(0)
    ranks.assert_exact(res)


@pytest.mark.parametrize("opts", [rs.MULTI_NO_OVERLAP, 0])
def test_multi_table_fault(opts):
    """k_bits = 4, keys only, under rs.table_fault() with no window: the partition and the k = 8 sample sort are no
    raw-table sorts, so only the local sorts fail -- one per rank without the overlap, two with it (each fails: the
    slots keep both) -- and every rank returns 11 on its own. Cleared: exact."""
    world = 2
    assert raw_tables(N_MULTI, 4) and raw_tables(N_MULTI // 2 * 9 // 10, 4)
    ranks = Ranks(world, False, 4)
    with rs.table_fault():
        res, calls = ranks.run(opts)
    assert res == [11] * world, [x if not isinstance(x, tuple) else "ok" for x in res]
    assert calls == [2 if opts else 3] * world, calls
    res, _ = ranks.run(opts)
    ranks.assert_exact(res)


@pytest.mark.parametrize("pairs", [False, True])
def test_multi_direct_and_whole_protocol_at_world_1(pairs):
    """One rank: by default it sorts directly (sort_direct), with MULTI_FULL the whole protocol runs (no sample sort
    at one virtual rank: the local sort is sort call 0, and the window keeps the hook off the partition). Under the
    rank fault both return 11; cleared, both are exact in the same workspace."""
    assert rank_fault_acts(N_MULTI, 8, pairs, False) and rank_fault_acts(N_MULTI, 8, pairs, True)
    ranks = Ranks(1, pairs, 8)
    with rs.rank_fault():
        res, calls = ranks.run(0)
        assert (res, calls) == ([11], [1])
        res, calls = ranks.run(rs.MULTI_FULL, [(0, 1)])
        assert (res, calls) == ([11], [1])
    for opts in (0, rs.MULTI_FULL):
        res, _ = ranks.run(opts)
        ranks.assert_exact(res)


# ------------------------------------------------------------------------------ multi-GPU sort, multi.py (gloo)
def _dist_inputs(rank, k):
    return uniform_keys(N_MULTI, seed=900 + 10 * k + rank)


def _dist_worker(rank, world, port, k, hook, out_dir):
    sys.path.insert(0, str(PKG))
    import multi
    import radixsort as rs_
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dk = rs_.from_numpy_u32(_dist_inputs(rank, k))
        faulty = getattr(rs_, hook)() if rank == 1 else contextlib.nullcontext()  # the hook in rank 1's process only
        with faulty:
            try:
                ok, _, off = multi.dist_sort(dk, k_bits=k)
                torch.cuda.synchronize()
                np.save(f"{out_dir}/k{rank}.npy", rs_.to_numpy_u32(ok))
                np.save(f"{out_dir}/o{rank}.npy", np.array([off], np.int64))
                res = "ok"
            except rs_.RSortError as e:
                res = str(e.status)
        Path(out_dir, f"r{rank}").write_text(res)
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dist_sort_rank_fault_raises_on_both_ranks(tmp_path):
    """multi.dist_sort, two processes on this GPU over gloo, rs.rank_fault() in rank 1's process only: its partition
    (and its sample sort, where that has a full tile) fails the rank check, the status travels in the step-5
    all-gather, and BOTH ranks raise RSORT_ERR_CHECK before any key moves."""
    assert rank_fault_acts(N_MULTI, 8, False, False)  # (the partition runs the sorts' line kernel over the same keys)
    mp.spawn(_dist_worker, args=(2, _free_port(), 8, "rank_fault", str(tmp_path)), nprocs=2, join=True)
    assert [(tmp_path / f"r{r}").read_text() for r in range(2)] == ["11", "11"]


def test_dist_sort_table_fault_raises_on_that_rank_alone(tmp_path):
    """k_bits = 4, keys only, rs.table_fault() in rank 1's process only: nothing before the exchange is a raw-table
    sort, so the exchange runs; rank 1's final sort fails and rank 1 alone raises 11, rank 0 returns its exact slice."""
    assert raw_tables(N_MULTI, 4) and raw_tables(N_MULTI * 9 // 10, 4) and raw_tables(N_MULTI * 11 // 10, 4)
    mp.spawn(_dist_worker, args=(2, _free_port(), 4, "table_fault", str(tmp_path)), nprocs=2, join=True)
    assert [(tmp_path / f"r{r}").read_text() for r in range(2)] == ["ok", "11"]
    want = np.sort(np.concatenate([_dist_inputs(r, 4) for r in range(2)]))
    got, off = np.load(tmp_path / "k0.npy"), int(np.load(tmp_path / "o0.npy")[0])
    assert off == 0 and abs(got.size - N_MULTI) < N_MULTI // 10 and np.array_equal(got, want[:got.size])


# ------------------------------------------------------------------------------ top-k
@functools.lru_cache(maxsize=None)
def topk_input():
    x, v = uniform_keys(N, seed=11), uniform_keys(N, seed=0xBEEF)  # (values that are not the positions)
    x.setflags(write=False)
    v.setflags(write=False)
    return x, v


@functools.lru_cache(maxsize=None)
def topk_order(largest):
    """The first K_TOP positions of the stable ascending order of x ^ m, from the oracle; computed once per direction."""
    x, _ = topk_input()
    m = np.uint32(0xFFFFFFFF if largest else 0)
    idx = oracle_sort_pairs(x ^ m, np.arange(N, dtype=np.uint32), 8)[1][:K_TOP].copy()
    idx.setflags(write=False)
    return idx


def topk_want(largest, mode):
    x, v = topk_input()
    idx = topk_order(largest)
    return x[idx], (None if mode == "keys" else idx if mode == "indices" else v[idx])


def topk_call(d_x, d_v, largest, mode, ws, sorted=True):
    ko, vo, _ = rs.topk_device(d_x, K_TOP, largest=largest, vals=d_v if mode == "vals" else None,
                               indices=mode == "indices", sorted=sorted, ws=ws)
    return rs.to_numpy_u32(ko), (None if vo is None else rs.to_numpy_u32(vo))


@pytest.mark.parametrize("mode", ["keys", "vals", "indices"])
@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("route", [rs.TOPK_SELECT, rs.TOPK_SORT])
def test_topk_faulted_and_clean(route, largest, mode):
    """Both routes end in a sort through the LSD driver (SELECT: the finishing sort of the k entries; SORT: the whole
    sort). Under the rank fault rsort_topk_report's check field (rs.topk_check) shows CHECK_RANK_ORDER, the output
    with values or indices differs from the clean one, and the host entry rs.topkByDevice raises 11. Before, and
    again after in the same workspace, the field is 0 and the output bit-exact."""
    pairs = mode != "keys"
    sorted_n = K_TOP if route == rs.TOPK_SELECT else N
    assert rank_fault_acts(sorted_n, 8, pairs, False, hybrid=True)
    x, v = topk_input()
    d_x, d_v = rs.from_numpy_u32(x), rs.from_numpy_u32(v)
    wk, wv = topk_want(largest, mode)
    with rs.topk_route(route):
        ws = rs.workspace(rs.topk_workspace_size(N, K_TOP, pairs, route))
        for faulted in (False, True, False):
            with (rs.rank_fault() if faulted else contextlib.nullcontext()):
                gk, gv = topk_call(d_x, d_v, largest, mode, ws)
                check = rs.topk_check(N, K_TOP, pairs, ws)
                assert rs.topk_report(N, K_TOP, pairs, ws)["route"] == route
                if faulted:
                    assert check == rs.CHECK_RANK_ORDER
                    if pairs:
                        assert not np.array_equal(gv, wv)
                    with pytest.raises(rs.RSortError) as e:
                        rs.topkByDevice(x, K_TOP, largest=largest, vals=v if mode == "vals" else None,
                                        indices=mode == "indices")
                    assert e.value.status == 11
                else:
                    assert check == 0
                    assert np.array_equal(gk, wk) and (not pairs or np.array_equal(gv, wv))
        hk, hv = rs.topkByDevice(x, K_TOP, largest=largest, vals=v if mode == "vals" else None, indices=mode == "indices")
        assert np.array_equal(hk, wk) and (not pairs or np.array_equal(hv, wv))


@pytest.mark.parametrize("largest,mode", [(False, "indices"), (True, "keys")])
def test_topk_unsorted_select_runs_no_sort_and_reports_a_clean_field(largest, mode):
    """UNSORTED on the SELECT route runs no sort: under the rank fault, in a workspace that held 0xFF everywhere (a
    stale check word and a stale "sorted" mark included), the field is 0 and the k entries are the right multiset."""
    pairs = mode != "keys"
    assert rank_fault_acts(K_TOP, 8, pairs, False, hybrid=True)
    x, v = topk_input()
    d_x = rs.from_numpy_u32(x)
    wk, wv = topk_want(largest, mode)
    with rs.topk_route(rs.TOPK_SELECT), rs.rank_fault():
        ws = rs.workspace(rs.topk_workspace_size(N, K_TOP, pairs, rs.TOPK_SELECT))
        ws.fill_(0xFF)
        gk, gv = topk_call(d_x, None, largest, mode, ws, sorted=False)
        assert rs.topk_check(N, K_TOP, pairs, ws) == 0
    if pairs:
        g, w = np.lexsort((gv, gk)), np.lexsort((wv, wk))
        assert np.array_equal(gk[g], wk[w]) and np.array_equal(gv[g], wv[w])
    else:
        assert np.array_equal(np.sort(gk), np.sort(wk))


# ------------------------------------------------------------------------------ row-wise top-k
# one shape per kernel class of the select (by row length), k >= 64 so the finishing segmented sort's segments hold
# a full wave (its rank check's unit); the ks reach the segmented sort's wave, small, LDS and multi-tile kernels
ROWS_SHAPES = [(0, 1000, 64), (1, 500, 200), (2, 100, 1500), (3, 16, 18000)]  # (class, rows, k)


@pytest.mark.parametrize("cls,rows,k", ROWS_SHAPES)
@pytest.mark.parametrize("largest,mode", [(False, "vals"), (True, "indices")])
def test_topk_rows_faulted_and_clean(cls, rows, k, largest, mode):
    """rsort_topk_rows_check and rsort_u32_topk_rows's RSORT_ERR_CHECK, seen reporting for the first time: under the
    rank fault the finishing segmented sort's check is flagged and rs.topkRowsByDevice raises 11; UNSORTED under the
    fault runs no sort (flags 0, every row the right set); cleared, the same workspace gives the exact rows."""
    cols = TOPK_ROWS_CLASS_COLS[cls]
    assert rows * cols <= 1 << 22 and 64 <= k <= cols
    x = uniform_keys(rows * cols, seed=40 + cls).reshape(rows, cols)
    v = uniform_keys(rows * cols, seed=0xBEEF + cls).reshape(rows, cols)
    m = np.uint32(0xFFFFFFFF if largest else 0)
    idx = np.argsort(x ^ m, axis=1, kind="stable")[:, :k]
    wk = np.take_along_axis(x, idx, 1)
    wv = idx.astype(np.uint32) if mode == "indices" else np.take_along_axis(v, idx, 1)
    d_x, d_v = rs.from_numpy_u32(x), (rs.from_numpy_u32(v) if mode == "vals" else None)
    assert rs.topk_rows_grids(rows, cols, k, True)["kernel"] == cls
    # precondition: the segmented sort of rows segments of k entries, under the hook, reports the rank check
    seg = rs.from_numpy_u32(wk ^ m)
    with rs.rank_fault():
        _, sws = rs.sort_rows(seg, torch.empty_like(seg), torch.empty_like(seg), torch.empty_like(seg))
        assert rs.segmented_check(rows * k, rows, True, sws)[0] & rs.CHECK_RANK_ORDER
    ws = rs.workspace(rs.topk_rows_workspace_size(rows, cols, k, True))

    def call(sorted=True):
        ko, vo, _ = rs.topk_rows(d_x, k, largest=largest, vals_2d=d_v, indices=mode == "indices", sorted=sorted, ws=ws)
        return rs.to_numpy_u32(ko), rs.to_numpy_u32(vo)

    host = dict(largest=largest, vals_2d=v if mode == "vals" else None, indices=mode == "indices")
    with rs.rank_fault():
        call()
        flags, rep = rs.topk_rows_check(rows, cols, k, True, ws)
        assert flags == rs.CHECK_RANK_ORDER and rep[:2] == [cls, 0]
        with pytest.raises(rs.RSortError) as e:
            rs.topkRowsByDevice(x, k, **host)
        assert e.value.status == 11
        gk, gv = call(sorted=False)
        assert rs.topk_rows_check(rows, cols, k, True, ws) == (0, [cls, 0, 0, 0])
        g, w = np.lexsort((gv, gk), axis=1), np.lexsort((wv, wk), axis=1)
        assert np.array_equal(np.take_along_axis(gk, g, 1), np.take_along_axis(wk, w, 1))
        assert np.array_equal(np.take_along_axis(gv, g, 1), np.take_along_axis(wv, w, 1))
    gk, gv = call()
    assert rs.topk_rows_check(rows, cols, k, True, ws) == (0, [cls, 0, 0, 0])
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
    hk, hv = rs.topkRowsByDevice(x, k, **host)
    assert np.array_equal(hk, wk) and np.array_equal(hv, wv)


# ------------------------------------------------------------------------------ host pairs entry
@pytest.mark.parametrize("k", [8, 6])
def test_host_pairs_entry_returns_check_error_on_a_broken_lane_order(k):
    """rs.sortPairsByDevice (rsort_u32_pairs) reads the check word like the keys host entries: 11 under the rank
    fault, the oracle's stable order without it."""
    n = N
    assert rank_fault_acts(n, k, True, False, hybrid=True)
    x = uniform_keys(n, seed=20 + k) >> np.uint32(8)  # (duplicates: the order of equal keys is checked too)
    v = np.arange(n, dtype=np.uint32)
    ko, vo = np.empty_like(x), np.empty_like(v)
    with rs.rank_fault():
        with pytest.raises(rs.RSortError) as e:
            rs.sortPairsByDevice(x, v, n, ko, vo, k)
        assert e.value.status == 11
    rs.sortPairsByDevice(x, v, n, ko, vo, k)
    wk, wv = oracle_sort_pairs(x, v, k)
    assert np.array_equal(ko, wk) and np.array_equal(vo, wv)
