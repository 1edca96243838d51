"""The multi-GPU sort (cuda.radixsort_amd/multi.py) with the real kernels on the MI355X box:
two ranks sharing cuda:0 over gloo (host-side exchange), and one rank over RCCL ("nccl") --
the driver's 8-GPU run uses the same code with one rank per GPU. Parity: the ranks' outputs,
concatenated in rank order, equal Baseline1 (the oracle) on the union of the inputs."""
import os
import socket
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from _util import oracle_sort, oracle_sort_pairs, uniform_keys, zipf_keys  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = Path(__file__).resolve().parent.parent / "cuda.radixsort_amd"


def _inputs(rank, n, dist_name, pairs):
    gen = zipf_keys if dist_name == "zipf" else uniform_keys
    keys = gen(n + 1031 * rank, seed=0x5EED + rank)
    vals = (np.arange(keys.size, dtype=np.uint32) + np.uint32(rank << 24)) if pairs else None
    return keys, vals


def _worker(rank, world, port, n, dist_name, pairs, k, out_dir):
    sys.path.insert(0, str(PKG))
    import multi
    import radixsort as rs
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        keys, vals = _inputs(rank, n, dist_name, pairs)
        dk = rs.from_numpy_u32(keys)
        dv = rs.from_numpy_u32(vals) if pairs else None
        ok, ov, off = multi.dist_sort(dk, k_bits=k, vals=dv)
        torch.cuda.synchronize()
        np.save(f"{out_dir}/k{rank}.npy", rs.to_numpy_u32(ok))
        if pairs:
            np.save(f"{out_dir}/v{rank}.npy", rs.to_numpy_u32(ov))
        np.save(f"{out_dir}/o{rank}.npy", np.array([off], np.int64))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,dist_name,pairs,k", [(2, "uniform", False, 8), (2, "zipf", True, 8),
                                                     (3, "uniform", True, 4)])
def test_dist_sort_ranks_sharing_one_gpu(tmp_path, world, dist_name, pairs, k):
    n = 1 << 20
    mp.spawn(_worker, args=(world, _free_port(), n, dist_name, pairs, k, str(tmp_path)), nprocs=world, join=True)
    all_k, all_v = zip(*[_inputs(r, n, dist_name, pairs) for r in range(world)])
    keys = np.concatenate(all_k)
    got = [np.load(tmp_path / f"k{r}.npy") for r in range(world)]
    offs = [int(np.load(tmp_path / f"o{r}.npy")[0]) for r in range(world)]
    assert offs == list(np.cumsum([0] + [g.size for g in got[:-1]]))
    if pairs:
        rk, rv = oracle_sort_pairs(keys, np.concatenate(all_v), k)
        assert np.array_equal(np.concatenate(got), rk)
        assert np.array_equal(np.concatenate([np.load(tmp_path / f"v{r}.npy") for r in range(world)]), rv)
    else:
        assert np.array_equal(np.concatenate(got), oracle_sort(keys, k))


def test_dist_sort_rccl_single_rank():
    """The RCCL path end to end (all_reduce, all_to_all_single on device tensors) at world 1."""
    sys.path.insert(0, str(PKG))
    import multi
    import radixsort as rs
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as td:
        store = dist.FileStore(os.path.join(td, "store"), 1)
        dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=torch.device("cuda", 0))
        try:
            x = zipf_keys(700001, seed=9)
            vals = np.arange(x.size, dtype=np.uint32)
            ok, ov, off = multi.dist_sort(rs.from_numpy_u32(x), 8, vals=rs.from_numpy_u32(vals))
            torch.cuda.synchronize()
            rk, rv = oracle_sort_pairs(x, vals, 8)
            assert off == 0
            assert np.array_equal(rs.to_numpy_u32(ok), rk) and np.array_equal(rs.to_numpy_u32(ov), rv)
        finally:
            dist.destroy_process_group()


# ------------------------------------------------------------------ C ABI: rsort_u32_multi over RCCL
def test_c_multi_single_rank():
    """rsort_u32_multi with a one-rank RCCL communicator. With RSORT_MULTI_FULL every step (RCCL
    all-gathers, sample sort, partition, self exchange, in-place local sort) runs; by default one
    rank sorts directly. Result = Baseline1 either way."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    torch.cuda.set_device(0)
    comm = rs.RcclComm(1, 0, rs.rccl_unique_id())
    old = rs.set_multi_options(rs.MULTI_FULL)  # the whole protocol, RCCL calls included, at world 1
    try:
        for n, pairs in ((1000003, False), (600001, True), (0, False)):
            x = zipf_keys(n, seed=n) if n else np.zeros(0, np.uint32)
            vals = np.arange(n, dtype=np.uint32) if pairs else None
            ok, ov, off = rs.multi_sort_device(comm, rs.from_numpy_u32(x), 8,
                                               vals=rs.from_numpy_u32(vals) if pairs else None)
            torch.cuda.synchronize()
            assert off == 0 and ok.numel() == n
            if pairs:
                rk, rv = oracle_sort_pairs(x, vals, 8)
                assert np.array_equal(rs.to_numpy_u32(ok), rk) and np.array_equal(rs.to_numpy_u32(ov), rv)
            else:
                assert np.array_equal(rs.to_numpy_u32(ok), oracle_sort(x, 8))
        # capacity too small is reported, not overrun
        x = uniform_keys(5000)
        with pytest.raises(rs.RSortError) as e:
            rs.multi_sort_device(comm, rs.from_numpy_u32(x), 8, capacity=100)
        assert e.value.status == 9
        # default: one rank sorts directly (no partition, no self exchange), same result
        rs.set_multi_options(0)
        x = zipf_keys(777777, seed=3)
        ok, _, off = rs.multi_sort_device(comm, rs.from_numpy_u32(x), 8)
        torch.cuda.synchronize()
        assert off == 0 and np.array_equal(rs.to_numpy_u32(ok), oracle_sort(x, 8))
    finally:
        rs.set_multi_options(old)
        comm.close()


def _c_multi_worker(rank, world, uid_path, out_dir, n, pairs):
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    torch.cuda.set_device(0)
    uid = Path(uid_path).read_bytes()
    try:
        comm = rs.RcclComm(world, rank, uid)
    except rs.RSortError as e:
        # RCCL refuses two ranks on one device ("Duplicate GPU detected"): recorded, not hidden
        Path(out_dir, f"refused{rank}").write_text(str(e))
        return
    try:
        keys, vals = _inputs(rank, n, "zipf", pairs)
        ok, ov, off = rs.multi_sort_device(comm, rs.from_numpy_u32(keys), 8,
                                           vals=rs.from_numpy_u32(vals) if pairs else None)
        torch.cuda.synchronize()
        np.save(f"{out_dir}/k{rank}.npy", rs.to_numpy_u32(ok))
        if pairs:
            np.save(f"{out_dir}/v{rank}.npy", rs.to_numpy_u32(ov))
        np.save(f"{out_dir}/o{rank}.npy", np.array([off], np.int64))
    finally:
        comm.close()


def test_c_multi_two_ranks_one_gpu(tmp_path):
    """Two RCCL ranks on one GPU. This RCCL refuses that at ncclCommInitRank ("Duplicate GPU
    detected : rank 0 and rank 1 both on CUDA device"), the only case that skips; any other
    failure (a crash, an error status, a wrong result) fails. The world > 1 C-ABI path itself is
    covered on this box by the loopback transport tests below."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    uid_path = tmp_path / "uid"
    uid_path.write_bytes(rs.rccl_unique_id())
    n, world, pairs = 1 << 19, 2, True
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_c_multi_worker, args=(r, world, str(uid_path), str(tmp_path), n, pairs))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    for p in procs:
        if p.is_alive():
            p.kill()
    refused = sorted(tmp_path.glob("refused*"))
    if refused:
        pytest.skip(f"RCCL refuses {world} ranks on one GPU: {refused[0].read_text()[:200]}")
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    all_k, all_v = zip(*[_inputs(r, n, "zipf", pairs) for r in range(world)])
    got = [np.load(tmp_path / f"k{r}.npy") for r in range(world)]
    offs = [int(np.load(tmp_path / f"o{r}.npy")[0]) for r in range(world)]
    assert offs == list(np.cumsum([0] + [g.size for g in got[:-1]]))
    rk, rv = oracle_sort_pairs(np.concatenate(all_k), np.concatenate(all_v), 8)
    assert np.array_equal(np.concatenate(got), rk)
    assert np.array_equal(np.concatenate([np.load(tmp_path / f"v{r}.npy") for r in range(world)]), rv)


# ------------------------------------------------------------------ C ABI at world > 1: loopback transport
def _loopback_inputs(rank, n, dist_name, pairs):
    keys, vals = _inputs(rank, n, "zipf" if dist_name == "zipf" else "uniform", pairs)
    if dist_name == "hot":
        keys = keys.copy()
        keys[: keys.size * 3 // 4] = 0xC0FFEE  # one key: 3/4 of every rank's keys
    elif dist_name == "equal":
        keys = np.full(keys.size, 12345, np.uint32)
    elif dist_name == "empty0" and rank == 0:
        keys = keys[:0]
        vals = vals[:0] if vals is not None else None
    return keys, vals


def _run_loopback(world, inputs, k, capacity=None, piece=None, opts=0, stats=None, transports=None, ws_bytes=None,
                  timeout=240):
    """world threads in this process, one stream each, calling rsort_u32_multi_transport with
    the loopback transport (or `transports[r]`) on cuda:0 concurrently. Returns per-rank (keys, vals,
    offset) or the per-rank RSortError statuses. k: one k_bits, or one per rank. stats: a list that receives
    every rank's rsort_multi_last_stats (profiling on for the call). ws_bytes: per rank, the workspace_bytes it
    tells the call (None: what its workspace holds). timeout: seconds the ranks' threads are waited for."""
    import threading
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    torch.cuda.set_device(0)
    if capacity is None:
        capacity = sum(int(i[0].size) for i in inputs) + 1
    grp = rs.LoopbackGroup(world)
    if stats is not None:
        stats.extend([None] * world)
        rs.multi_set_profiling(True)
    old_piece = rs.set_exchange_piece(piece) if piece else None
    # (opts 0: one half per rank, MULTI_NO_OVERLAP -- the automatic overlap has its own test; None: no
    # overlap flag at all, the library's automatic choice)
    old_opts = rs.set_multi_options(0 if opts is None else opts if opts else rs.MULTI_NO_OVERLAP)
    dev_in = [(rs.from_numpy_u32(kx), rs.from_numpy_u32(vx) if vx is not None else None) for kx, vx in inputs]
    res = [None] * world

    def run(r):
        torch.cuda.set_device(0)
        st = torch.cuda.Stream()
        try:
            with torch.cuda.stream(st):
                kk, vv = dev_in[r]
                tr = transports[r] if transports is not None else grp.transport(r)
                ok, ov, off = rs.multi_sort_device(tr, kk, k[r] if isinstance(k, (list, tuple)) else k, vals=vv,
                                                   capacity=capacity, stream=st,
                                                   ws_bytes=ws_bytes[r] if ws_bytes is not None else None)
                st.synchronize()
                res[r] = (rs.to_numpy_u32(ok), rs.to_numpy_u32(ov) if ov is not None else None, off)
                if stats is not None:
                    stats[r] = rs.multi_last_stats()  # (thread-local: this rank's sort)
        except rs.RSortError as e:
            res[r] = e.status

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    alive = any(t.is_alive() for t in th)
    rs.set_multi_options(old_opts)
    if stats is not None:
        rs.multi_set_profiling(False)
    if old_piece:
        rs.set_exchange_piece(old_piece)
    if not alive:
        grp.close()
    assert not alive, "loopback ranks did not finish"
    return res


@pytest.mark.parametrize("world,dist_name,pairs,k,piece", [(2, "uniform", False, 8, None), (2, "zipf", True, 8, None),
                                                           (3, "hot", True, 8, 4096), (4, "equal", False, 8, None),
                                                           (4, "uniform", True, 4, 10000), (8, "zipf", False, 8, None),
                                                           (3, "empty0", True, 8, None), (12, "hot", True, 8, None),
                                                           (16, "zipf", True, 8, None)])
def test_c_multi_loopback(world, dist_name, pairs, k, piece):
    """rsort_u32_multi_transport at world 2..16 with the real kernels (sampling, device sort of the
    gathered sample, partition into equal-key buckets, exchange plan, exchange, in-place local
    sort): the ranks' outputs concatenated in rank order equal Baseline1 on the union of the
    inputs (stable with values), offsets are the exclusive scan of the counts, and every rank
    holds the mean count within 5 % -- also when one key holds 3/4 of the keys, and at world 12 and 16,
    whose hot quantile keys take the partition past 16 buckets. piece: keys per exchange message
    (rsort_set_exchange_piece), small to force many rounds."""
    n = 300_000 if world <= 8 else 100_000
    inputs = [_loopback_inputs(r, n, dist_name, pairs) for r in range(world)]
    res = _run_loopback(world, inputs, k, piece=piece)
    assert all(isinstance(x, tuple) for x in res), res
    got = [x[0] for x in res]
    offs = [x[2] for x in res]
    assert offs == list(np.cumsum([0] + [g.size for g in got[:-1]]))
    keys = np.concatenate([i[0] for i in inputs])
    if pairs:
        rk, rv = oracle_sort_pairs(keys, np.concatenate([i[1] for i in inputs]), k)
        assert np.array_equal(np.concatenate(got), rk)
        assert np.array_equal(np.concatenate([x[1] for x in res]), rv)
    else:
        assert np.array_equal(np.concatenate(got), oracle_sort(keys, k))
    sizes = np.array([g.size for g in got])
    assert np.abs(sizes - keys.size / world).max() <= 0.05 * keys.size / world + 64, sizes


@pytest.mark.parametrize("world,dist_name", [(2, "uniform"), (3, "hot")])
def test_c_multi_loopback_large_per_rank(world, dist_name):
    """the loopback C-ABI path with a per-rank size above the large-partition threshold
    (2 x CUs x 8192 keys: keys-only partitions run 512 x 16 line tiles with splitter digits), so
    the production partition kernel meets multi-bucket input -- equal-key buckets included ("hot":
    3/4 of every rank's keys are one key)."""
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8192 + 1001
    inputs = [_loopback_inputs(r, n, dist_name, False) for r in range(world)]
    res = _run_loopback(world, inputs, 8)
    assert all(isinstance(x, tuple) for x in res), res
    got = [x[0] for x in res]
    keys = np.concatenate([i[0] for i in inputs])
    assert np.array_equal(np.concatenate(got), oracle_sort(keys, 8))


def test_c_multi_loopback_local_error_on_every_rank():
    """a failure local to one rank (here rank 1 passes k_bits = 0) is carried in the
    status word of the first all-gather, so EVERY rank returns it together (RSORT_ERR_BITS)
    instead of the other ranks waiting in a collective that rank never joins."""
    world = 3
    inputs = [_loopback_inputs(r, 50_000, "uniform", False) for r in range(world)]
    res = _run_loopback(world, inputs, [0 if r == 1 else 8 for r in range(world)], capacity=200_000, timeout=60)
    assert res == [2] * world, res


def test_c_multi_loopback_value_flags_disagree():
    """Rank 1 sorts pairs (values and a values output), ranks 0 and 2 keys only: every rank sees the same flags in
    the first all-gather and returns RSORT_ERR_ARG; nobody is left waiting."""
    world = 3
    inputs = [_loopback_inputs(r, 50_000, "uniform", r == 1) for r in range(world)]
    res = _run_loopback(world, inputs, 8, capacity=200_000, timeout=60)
    assert res == [1] * world, res


def test_c_multi_loopback_workspace_too_small_on_every_rank():
    """Rank 2's workspace is 256 B short of rsort_multi_workspace_size (still above the control buffers, so it
    joins the first all-gather): its RSORT_ERR_WORKSPACE is carried there and every rank returns it."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    world, cap = 3, 200_000
    inputs = [_loopback_inputs(r, 50_000, "uniform", False) for r in range(world)]
    full = int(rs._lib().rsort_multi_workspace_size(inputs[2][0].size, cap, 8, 0, world))
    res = _run_loopback(world, inputs, 8, capacity=cap, ws_bytes=[None, None, full - 256], timeout=60)
    assert res == [7] * world, res


def test_c_multi_workspace_below_the_control_buffers():
    """A workspace that cannot even hold the collectives' control buffers is refused at once, before any
    all-gather (world 1 only: at a larger world the peers would wait for this rank until the transport's limit)."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    inputs = [_loopback_inputs(0, 50_000, "uniform", False)]
    res = _run_loopback(1, inputs, 8, opts=rs.MULTI_FULL, ws_bytes=[256], timeout=60)
    assert res == [7], res


@pytest.mark.parametrize("opts", [0, 1])
def test_c_multi_loopback_world_1_whole_protocol(opts):
    """One loopback rank with RSORT_MULTI_FULL runs every step (one half whatever the overlap flag: H = 2 needs
    two ranks) and gives the oracle's output; without the flag the same input is sorted directly."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    inputs = [_loopback_inputs(0, 60_000, "hot", True)]
    rk, rv = oracle_sort_pairs(inputs[0][0], inputs[0][1], 8)
    for full, direct in ((rs.MULTI_FULL, 0), (0, 1)):
        st = []
        res = _run_loopback(1, inputs, 8, opts=full | (rs.MULTI_OVERLAP if opts else rs.MULTI_NO_OVERLAP), stats=st)
        assert isinstance(res[0], tuple), res
        assert np.array_equal(res[0][0], rk) and np.array_equal(res[0][1], rv) and res[0][2] == 0
        assert st[0]["direct"] == direct and st[0]["halves"] == 1, st[0]


@pytest.mark.parametrize("stage,opts", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_c_multi_loopback_failure_after_sample_gather(stage, opts):
    """a rank that fails AFTER the sample all-gather (stage 1: its sample sort; stage 2:
    its partition) still joins the count all-gather with a row of its peers' size and its status in
    it, so every rank returns that status together (no mismatched collective, nobody left waiting)
    -- with one and with two halves per rank (RSORT_MULTI_OVERLAP: 2 x world virtual ranks)."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    world = 3
    inputs = [_loopback_inputs(r, 60_000, "uniform", False) for r in range(world)]
    _check = rs._lib().rsort_multi_inject_failure
    assert _check(1, stage, 6) == 0  # rank 1 fails with RSORT_ERR_HIP at this stage
    try:
        res = _run_loopback(world, inputs, 8, opts=opts)
    finally:
        _check(-1, 0, 0)
    assert res == [6] * world, res
    res = _run_loopback(world, inputs, 8, opts=opts)  # the hook cleared: the same sort succeeds
    assert all(isinstance(x, tuple) for x in res), res
    assert np.array_equal(np.concatenate([x[0] for x in res]), oracle_sort(np.concatenate([i[0] for i in inputs]), 8))


@pytest.mark.parametrize("opts", [0, 1])
def test_c_multi_loopback_stats(opts):
    """rsort_multi_last_stats (bench.py's N-GPU block): per-thread records of each rank's sort --
    world, halves, keys sent/received per peer (a rank's sends summed over ranks are what the ranks
    receive), and the phase times, which add up to the total."""
    world = 3
    inputs = [_loopback_inputs(r, 200_000, "zipf", True) for r in range(world)]
    st = []
    res = _run_loopback(world, inputs, 8, opts=opts, stats=st)
    assert all(isinstance(x, tuple) for x in res), res
    for r, x in enumerate(st):
        assert x["world"] == world and x["rank"] == r and x["halves"] == (2 if opts else 1) and x["direct"] == 0
        assert x["bytes_per_key"] == 8 and x["n_in"] == inputs[r][0].size and x["n_out"] == res[r][0].size
        assert sum(x["send_keys"]) == x["n_in"] and sum(x["recv_keys"]) == x["n_out"]
        parts = x["ms_plan"] + x["ms_partition"] + x["ms_exchange"] + x["ms_local_sort"]
        assert x["ms_total"] > 0 and abs(parts - x["ms_total"]) < 0.05 * x["ms_total"] + 0.05, x
    for p in range(world):
        assert sum(st[r]["send_keys"][p] for r in range(world)) == st[p]["n_out"]
        assert [st[r]["send_keys"][p] for r in range(world)] == st[p]["recv_keys"]


def _run_host_transport(world, inputs, k, trace=None, **kw):
    """_run_loopback over rs.HostTransport: the ranks as threads with a Python rendezvous. trace: per rank a list
    that receives its collectives in call order -- ("ag", bytes sent) for an all-gather, ("ex", bytes sent to each
    rank, bytes expected from each rank) for an exchange."""
    import threading
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    bar = threading.Barrier(world, timeout=120)
    box = {}

    def mk(r):
        def allgather(send):
            if trace is not None:
                trace[r].append(("ag", len(send)))
            box[("ag", r)] = bytes(send)
            bar.wait()
            out = b"".join(box[("ag", q)] for q in range(world))
            bar.wait()
            return out

        def exchange(sends, recv_sizes):
            if trace is not None:
                trace[r].append(("ex", [len(x) for x in sends], list(recv_sizes)))
            for p in range(world):
                box[("ex", r, p)] = bytes(sends[p])
            bar.wait()
            out = [box[("ex", p, r)] for p in range(world)]
            bar.wait()
            return out
        return rs.HostTransport(world, r, allgather, exchange)

    hts = [mk(r) for r in range(world)]
    try:
        res = _run_loopback(world, inputs, k, transports=[h.transport for h in hts], **kw)
    finally:
        for h in hts:
            h.close()
    assert all(isinstance(x, tuple) for x in res), (res, [h.errors for h in hts])
    return res


def test_c_multi_host_transport_threads():
    """rsort_host_transport_wrap: the C protocol over a HOST-memory transport (the one bench.py's
    gloo rehearsal uses), here three ranks as threads with a Python rendezvous; bit-exact as the
    loopback, also with forced exchange rounds."""
    world = 3
    inputs = [_loopback_inputs(r, 150_000, "hot", True) for r in range(world)]
    res = _run_host_transport(world, inputs, 8, piece=20_000)
    rk, rv = oracle_sort_pairs(np.concatenate([i[0] for i in inputs]), np.concatenate([i[1] for i in inputs]), 8)
    assert np.array_equal(np.concatenate([x[0] for x in res]), rk)
    assert np.array_equal(np.concatenate([x[1] for x in res]), rv)


# The collectives of three ranks, recorded from the library as it was BEFORE multi_sort became one function per
# protocol step (this file's own `python tests/test_gpu_multi.py` against that commit's library, never from the
# code under test): per case, per rank, the all-gathers and exchanges in call order with every byte count. Pins
# the number and order of the collectives, the round cutting, the virtual-rank indexing (two halves: opts 1) and
# the keys-then-values order inside a round.
TRACE_WORLD, TRACE_N = 3, 60_000
TRACE_CASES = (("hot", True, 4096, 0), ("hot", True, 4096, 1), ("empty0", False, None, 1))
TRACES = {
    "hot pairs piece 4096 opts 0": [
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [0, 0, 15616], [0, 15616, 224]),
         ('ex', [0, 0, 15616], [0, 15616, 224]), ('ex', [0, 0, 15616], [0, 15616, 0]),
         ('ex', [0, 0, 15616], [0, 15616, 0]), ('ex', [0, 0, 15616], [0, 15616, 0]),
         ('ex', [0, 0, 15616], [0, 15616, 0]), ('ex', [0, 0, 12948], [0, 15616, 0]),
         ('ex', [0, 0, 12948], [0, 15616, 0]), ('ex', [0, 0, 0], [0, 1232, 0]), ('ex', [0, 0, 0], [0, 1232, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0])],
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [15616, 0, 15616], [0, 0, 15616]),
         ('ex', [15616, 0, 15616], [0, 0, 15616]), ('ex', [15616, 0, 15616], [0, 0, 15616]),
         ('ex', [15616, 0, 15616], [0, 0, 15616]), ('ex', [15616, 0, 15616], [0, 0, 15616]),
         ('ex', [15616, 0, 15616], [0, 0, 15616]), ('ex', [15616, 0, 13968], [0, 0, 15616]),
         ('ex', [15616, 0, 13968], [0, 0, 15616]), ('ex', [1232, 0, 0], [0, 0, 15616]),
         ('ex', [1232, 0, 0], [0, 0, 15616]), ('ex', [0, 0, 0], [0, 0, 15616]), ('ex', [0, 0, 0], [0, 0, 15616]),
         ('ex', [0, 0, 0], [0, 0, 15616]), ('ex', [0, 0, 0], [0, 0, 15616]), ('ex', [0, 0, 0], [0, 0, 15200]),
         ('ex', [0, 0, 0], [0, 0, 15200])],
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [224, 15616, 0], [15616, 15616, 0]),
         ('ex', [224, 15616, 0], [15616, 15616, 0]), ('ex', [0, 15616, 0], [15616, 15616, 0]),
         ('ex', [0, 15616, 0], [15616, 15616, 0]), ('ex', [0, 15616, 0], [15616, 15616, 0]),
         ('ex', [0, 15616, 0], [15616, 15616, 0]), ('ex', [0, 15616, 0], [12948, 13968, 0]),
         ('ex', [0, 15616, 0], [12948, 13968, 0]), ('ex', [0, 15616, 0], [0, 0, 0]), ('ex', [0, 15616, 0], [0, 0, 0]),
         ('ex', [0, 15616, 0], [0, 0, 0]), ('ex', [0, 15616, 0], [0, 0, 0]), ('ex', [0, 15616, 0], [0, 0, 0]),
         ('ex', [0, 15616, 0], [0, 0, 0]), ('ex', [0, 15200, 0], [0, 0, 0]), ('ex', [0, 15200, 0], [0, 0, 0])],
    ],
    "hot pairs piece 4096 opts 1": [
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [0, 0, 15360], [0, 216, 224]),
         ('ex', [0, 0, 15360], [0, 216, 224]), ('ex', [0, 0, 4348], [0, 0, 0]), ('ex', [0, 0, 4348], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 15360], [0, 15360, 0]), ('ex', [0, 0, 15360], [0, 15360, 0]),
         ('ex', [0, 0, 15360], [0, 15360, 0]), ('ex', [0, 0, 15360], [0, 15360, 0]),
         ('ex', [0, 0, 9368], [0, 15360, 0]), ('ex', [0, 0, 9368], [0, 15360, 0]), ('ex', [0, 0, 0], [0, 15360, 0]),
         ('ex', [0, 0, 0], [0, 15360, 0]), ('ex', [0, 0, 0], [0, 2040, 0]), ('ex', [0, 0, 0], [0, 2040, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0])],
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [216, 0, 15360], [0, 0, 2448]),
         ('ex', [216, 0, 15360], [0, 0, 2448]), ('ex', [0, 0, 4752], [0, 0, 0]), ('ex', [0, 0, 4752], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [15360, 0, 15360], [0, 0, 15360]), ('ex', [15360, 0, 15360], [0, 0, 15360]),
         ('ex', [15360, 0, 15360], [0, 0, 15360]), ('ex', [15360, 0, 15360], [0, 0, 15360]),
         ('ex', [15360, 0, 9984], [0, 0, 15360]), ('ex', [15360, 0, 9984], [0, 0, 15360]),
         ('ex', [15360, 0, 0], [0, 0, 15360]), ('ex', [15360, 0, 0], [0, 0, 15360]),
         ('ex', [2040, 0, 0], [0, 0, 15360]), ('ex', [2040, 0, 0], [0, 0, 15360]), ('ex', [0, 0, 0], [0, 0, 15360]),
         ('ex', [0, 0, 0], [0, 0, 15360]), ('ex', [0, 0, 0], [0, 0, 15360]), ('ex', [0, 0, 0], [0, 0, 15360]),
         ('ex', [0, 0, 0], [0, 0, 14544]), ('ex', [0, 0, 0], [0, 0, 14544])],
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [224, 2448, 0], [15360, 15360, 0]),
         ('ex', [224, 2448, 0], [15360, 15360, 0]), ('ex', [0, 0, 0], [4348, 4752, 0]),
         ('ex', [0, 0, 0], [4348, 4752, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 0, 0], [0, 0, 0]),
         ('ex', [0, 0, 0], [0, 0, 0]), ('ex', [0, 15360, 0], [15360, 15360, 0]),
         ('ex', [0, 15360, 0], [15360, 15360, 0]), ('ex', [0, 15360, 0], [15360, 15360, 0]),
         ('ex', [0, 15360, 0], [15360, 15360, 0]), ('ex', [0, 15360, 0], [9368, 9984, 0]),
         ('ex', [0, 15360, 0], [9368, 9984, 0]), ('ex', [0, 15360, 0], [0, 0, 0]), ('ex', [0, 15360, 0], [0, 0, 0]),
         ('ex', [0, 15360, 0], [0, 0, 0]), ('ex', [0, 15360, 0], [0, 0, 0]), ('ex', [0, 15360, 0], [0, 0, 0]),
         ('ex', [0, 15360, 0], [0, 0, 0]), ('ex', [0, 15360, 0], [0, 0, 0]), ('ex', [0, 15360, 0], [0, 0, 0]),
         ('ex', [0, 14544, 0], [0, 0, 0]), ('ex', [0, 14544, 0], [0, 0, 0])],
    ],
    "empty0 keys piece None opts 1": [
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [0, 0, 0], [0, 40676, 41380]),
         ('ex', [0, 0, 0], [0, 40684, 41384])],
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [40676, 0, 40656], [0, 0, 41328]),
         ('ex', [40684, 0, 40724], [0, 0, 41408])],
        [('ag', 24), ('ag', 248252), ('ag', 272), ('ex', [41380, 41328, 0], [0, 40656, 0]),
         ('ex', [41384, 41408, 0], [0, 40724, 0])],
    ],
}


def _trace_key(dist_name, pairs, piece, opts):
    return f"{dist_name} {'pairs' if pairs else 'keys'} piece {piece} opts {opts}"


def _traced_sort(dist_name, pairs, piece, opts):
    inputs = [_loopback_inputs(r, TRACE_N, dist_name, pairs) for r in range(TRACE_WORLD)]
    trace = [[] for _ in range(TRACE_WORLD)]
    res = _run_host_transport(TRACE_WORLD, inputs, 8, trace=trace, piece=piece, opts=opts)
    return inputs, res, trace


@pytest.mark.parametrize("dist_name,pairs,piece,opts", TRACE_CASES)
def test_c_multi_collective_trace(dist_name, pairs, piece, opts):
    """Every rank's collectives, in order and byte for byte, are the recorded ones (TRACES); the output is still
    the oracle's."""
    inputs, res, trace = _traced_sort(dist_name, pairs, piece, opts)
    want = TRACES[_trace_key(dist_name, pairs, piece, opts)]
    for r in range(TRACE_WORLD):
        assert trace[r] == want[r], (r, trace[r])
    if piece:  # (the case is there for its several rounds: more exchanges than arrays x halves)
        assert all(sum(c[0] == "ex" for c in t) > (2 if pairs else 1) * (2 if opts else 1) for t in trace)
    keys = np.concatenate([i[0] for i in inputs])
    if pairs:
        rk, rv = oracle_sort_pairs(keys, np.concatenate([i[1] for i in inputs]), 8)
        assert np.array_equal(np.concatenate([x[0] for x in res]), rk)
        assert np.array_equal(np.concatenate([x[1] for x in res]), rv)
    else:
        assert np.array_equal(np.concatenate([x[0] for x in res]), oracle_sort(keys, 8))
    assert [x[2] for x in res] == list(np.cumsum([0] + [x[0].size for x in res[:-1]]))


@pytest.mark.parametrize("world,dist_name,pairs,k,piece", [(2, "uniform", False, 8, None), (3, "hot", True, 8, None),
                                                           (4, "zipf", True, 8, 5000), (4, "equal", False, 8, None),
                                                           (5, "uniform", True, 4, None), (8, "zipf", False, 8, None),
                                                           (3, "empty0", True, 8, None)])
def test_c_multi_loopback_overlap(world, dist_name, pairs, k, piece):
    """RSORT_MULTI_OVERLAP at world 2..8: the planning functions run for 2 x world ranks, each rank
    receives its lower half first and sorts it on a side stream while its upper half is exchanged
    (VERDICT r2 #6). Output, offsets and stability exactly as without the flag; balance within 5 %
    (equal-key buckets at every world: up to 31 partition buckets at 2 x 8 virtual ranks)."""
    n = 200_000
    inputs = [_loopback_inputs(r, n, dist_name, pairs) for r in range(world)]
    res = _run_loopback(world, inputs, k, piece=piece, opts=1)
    assert all(isinstance(x, tuple) for x in res), res
    got = [x[0] for x in res]
    assert [x[2] for x in res] == list(np.cumsum([0] + [g.size for g in got[:-1]]))
    keys = np.concatenate([i[0] for i in inputs])
    if pairs:
        rk, rv = oracle_sort_pairs(keys, np.concatenate([i[1] for i in inputs]), k)
        assert np.array_equal(np.concatenate(got), rk)
        assert np.array_equal(np.concatenate([x[1] for x in res]), rv)
    else:
        assert np.array_equal(np.concatenate(got), oracle_sort(keys, k))
    sizes = np.array([g.size for g in got])
    assert np.abs(sizes - keys.size / world).max() <= 0.05 * keys.size / world + 64, sizes


@pytest.mark.parametrize("world,halves", [(2, 2), (4, 2), (8, 2), (9, 1)])
def test_c_multi_loopback_automatic_overlap(world, halves):
    """Round 6: without an overlap flag the lower-half overlap runs for 2 <= world <= 8
    (2 x world <= 16 virtual ranks) and not above (predicted faster at every world it runs at).
    Zipf pairs: hot quantile keys, so at world 8 the partition has more than 16 buckets. Same output
    either way."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    inputs = [_loopback_inputs(r, 150_000, "zipf", True) for r in range(world)]
    st = []
    res = _run_loopback(world, inputs, 8, stats=st, opts=None)
    assert all(isinstance(x, tuple) for x in res), res
    assert [x["halves"] for x in st] == [halves] * world
    keys = np.concatenate([i[0] for i in inputs])
    rk, rv = oracle_sort_pairs(keys, np.concatenate([i[1] for i in inputs]), 8)
    assert np.array_equal(np.concatenate([x[0] for x in res]), rk)
    assert np.array_equal(np.concatenate([x[1] for x in res]), rv)


def test_c_multi_loopback_capacity_on_every_rank():
    """one rank's output too small -> EVERY rank returns RSORT_ERR_CAPACITY
    before any key moves (no rank is left waiting in the exchange)."""
    world = 3
    inputs = [_loopback_inputs(r, 100_000, "uniform", False) for r in range(world)]
    res = _run_loopback(world, inputs, 8, capacity=50_000)  # each rank would receive ~100 000
    assert res == [9] * world


# ------------------------------------------------------------------ >= 2 GiB exchange messages
def _sorted_ref(d_keys):
    return torch.sort(d_keys.to(torch.int64) & 0xFFFFFFFF)[0]


def test_dist_sort_rccl_2gib_message():
    """multi.py over RCCL at one rank with 2^29 + 3 keys (2 GiB). At world 1 the rank's own range
    moves by a device copy, so NO 2 GiB message goes through RCCL here: this checks the one-rank
    path at that size. The rounds that keep messages below 1 GiB (this RCCL leaves the second half
    of a >= 2 GiB message unwritten, dev/a2a_lab.py) are exercised by the gloo tests with small
    pieces; a multi-round RCCL exchange needs two GPUs and is unverified on the one-GPU box."""
    sys.path.insert(0, str(PKG))
    import multi
    import radixsort as rs
    torch.cuda.set_device(0)
    n = (1 << 29) + 3
    with tempfile.TemporaryDirectory() as td:
        store = dist.FileStore(os.path.join(td, "store"), 1)
        dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=torch.device("cuda", 0))
        try:
            keys = rs.empty_u32(n)
            rs.gen_uniform(keys, 77)
            ok, _, off = multi.dist_sort(keys, 8)
            torch.cuda.synchronize()
            assert off == 0 and ok.numel() == n
            assert torch.equal(ok.to(torch.int64) & 0xFFFFFFFF, _sorted_ref(keys))
        finally:
            dist.destroy_process_group()


def test_c_multi_2gib_message():
    """rsort_u32_multi over RCCL at one rank with 2^29 + 5 keys (2 GiB), the whole protocol
    (RSORT_MULTI_FULL). The own range moves by a device copy, so no RCCL message is sent: this checks
    the one-rank path at that size. Exchange rounds are exercised by the loopback tests with small
    pieces (test_c_multi_loopback); a multi-round RCCL exchange needs two GPUs and is unverified on
    the one-GPU box."""
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    torch.cuda.set_device(0)
    n = (1 << 29) + 5
    comm = rs.RcclComm(1, 0, rs.rccl_unique_id())
    old = rs.set_multi_options(rs.MULTI_FULL)
    try:
        keys = rs.empty_u32(n)
        rs.gen_uniform(keys, 78)
        ok, _, off = rs.multi_sort_device(comm, keys, 8)
        torch.cuda.synchronize()
        assert off == 0 and ok.numel() == n
        assert torch.equal(ok.to(torch.int64) & 0xFFFFFFFF, _sorted_ref(keys))
    finally:
        rs.set_multi_options(old)
        comm.close()


_INIT_SNIPPET = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
import torch
import radixsort as rs
torch.cuda.set_device(0)
uid = rs.rccl_unique_id()
t0 = time.monotonic()
try:
    rs.RcclComm(2, 0, uid, timeout_ms=5000)  # rank 1 never joins
    print("JOINED")
except rs.RSortError as e:
    print(f"STATUS {e.status} {time.monotonic() - t0:.1f}")
# ADVICE r5: a retry in the same process -- a new communicator (possibly at the aborted one's address) sorts
# and is destroyed normally
c = rs.RcclComm(1, 0, rs.rccl_unique_id(), timeout_ms=20000)
keys = torch.randint(-2**31, 2**31 - 1, (300000,), dtype=torch.int32, device="cuda")
with rs.multi_options(rs.MULTI_FULL):
    ok, _, off = rs.multi_sort_device(c, keys, 8)
got = ok.cpu().numpy().view("uint32")
want = keys.cpu().numpy().view("uint32")
import numpy as np
print("RETRY", int(np.array_equal(got, np.sort(want))), off)
c.close()
print("DESTROYED")
"""


def test_rccl_init_deadline_when_a_peer_never_joins():
    """the communicator is set up non-blocking (ncclCommInitRankConfig, blocking = 0)
    and polled; rank 0 of a world-2 communicator whose rank 1 never joins gets RSORT_ERR_COMM after
    its 5-s deadline (the setup is aborted) instead of waiting forever; then, in the same process, a new
    communicator sorts and is destroyed (the aborted one's address may come back). In a
    subprocess, so a hang in RCCL's abort could only fail this test."""
    import subprocess
    r = subprocess.run([sys.executable, "-c", _INIT_SNIPPET, str(PKG)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(("STATUS", "JOINED"))]
    assert line and line[0].startswith("STATUS 10"), r.stdout[-1000:]
    assert 4.0 <= float(line[0].split()[2]) < 60.0, line
    assert "RETRY 1 0" in r.stdout and "DESTROYED" in r.stdout, r.stdout[-1000:]


def test_rccl_comm_timeout_setting():
    sys.path.insert(0, str(PKG))
    import radixsort as rs
    old = rs.set_comm_timeout(1234)
    try:
        assert rs.set_comm_timeout(0) == 1234  # (<= 0 leaves it unchanged)
    finally:
        rs.set_comm_timeout(old)


if __name__ == "__main__":  # the TRACES literal above, from the library as built
    print("TRACES = {")
    for case in TRACE_CASES:
        print(f'    "{_trace_key(*case)}": [')
        for t in _traced_sort(*case)[2]:
            print(f"        {t},")
        print("    ],")
    print("}")
