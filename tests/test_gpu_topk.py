"""GPU tests of the top-k selection (include/rsort.h "top-k selection").

The expected output everywhere is the project's own oracle: with m = 0xFFFFFFFF for the k largest, else 0, and
idx = oracle_sort_pairs(x ^ m, arange(n), 8)[1][:k] -- the stable order, so equal keys keep their input order and the
lowest positions are taken at the threshold -- the result is (x[idx], v[idx]), or idx itself with indices. Every
element is compared bit for bit; UNSORTED results after sorting both sides' (key, value) pairs on the host. The report
(the k-th key, the entries before it, the ties taken and present, the candidates after the first digit) is compared
with the same host order. Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import oracle_sort_pairs, uniform_keys, zipf_keys

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SELECT, SORT, AUTO = rs.TOPK_SELECT, rs.TOPK_SORT, rs.TOPK_AUTO
MODES = ("keys", "vals", "indices")
KNOWN_SCATTER_KERNELS = 144  # len(rs.scatter_kernels_known()) of the parent commit: this feature adds none
SIZES = (1, 2, 63, 64, 65, 257, 4097, 70001, 200003, (1 << 20) + 77)


def dev(a):
    return rs.from_numpy_u32(a if a.flags.writeable else a.copy())


def ks_for(n):
    return sorted({min(max(k, 1), n) for k in (1, 2, 64, 65, n // 3, n - 1, n)})


@functools.lru_cache(maxsize=None)
def keys(name, n):
    if name == "uniform":
        x = uniform_keys(n)
    elif name == "uniform2":
        x = uniform_keys(n, seed=77)
    elif name == "zipf":
        x = zipf_keys(n)
    elif name == "equal":
        x = np.full(n, 0xDEADBEEF, np.uint32)
    elif name == "ends":  # only 0 and 0xFFFFFFFF
        x = np.where(uniform_keys(n, seed=5) & 1, np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32)
    elif name == "low10":  # below 2^10: every level but the last keeps all n candidates
        x = uniform_keys(n, seed=9) >> np.uint32(22)
    elif name == "top8":  # differ only in the top 8 bits
        x = (uniform_keys(n, seed=11) & np.uint32(0xFF000000)) | np.uint32(0x00ABCDEF)
    elif name == "sorted":
        x = np.sort(uniform_keys(n, seed=13))
    elif name == "reverse":
        x = np.sort(uniform_keys(n, seed=13))[::-1]
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, dtype=np.uint32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def values(n):
    v = uniform_keys(n, seed=0xBEEF)  # (not the positions: a result that returned positions for values would differ)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def order(name, n, largest):
    """The stable ascending order of x ^ m, from the oracle: computed once per input and direction, never changed."""
    x = keys(name, n)
    m = np.uint32(0xFFFFFFFF if largest else 0)
    idx = oracle_sort_pairs(x ^ m, np.arange(n, dtype=np.uint32), 8)[1]
    idx.setflags(write=False)
    return idx


def expected(name, n, k, largest, mode):
    idx = order(name, n, largest)[:k]
    x = keys(name, n)
    return x[idx], (None if mode == "keys" else idx if mode == "indices" else values(n)[idx])


def host_report(name, n, k, largest):
    x = keys(name, n)
    m = np.uint32(0xFFFFFFFF if largest else 0)
    kth = x[order(name, n, largest)[k - 1]]
    t = kth ^ m
    before = int(np.count_nonzero((x ^ m) < t))
    return {"route": SELECT, "kth_key": int(kth), "before": before, "equal_taken": k - before,
            "equal_in_input": int(np.count_nonzero(x == kth)),
            "candidates": int(np.count_nonzero(((x ^ m) >> np.uint32(24)) == (t >> np.uint32(24))))}


def call(d_x, n, k, largest, mode, d_v=None, sorted=True, ws=None, out=None, stream=None):
    return rs.topk_device(d_x, k, largest=largest, vals=d_v if mode == "vals" else None, indices=mode == "indices",
                          sorted=sorted, ws=ws, out=out, stream=stream)


def assert_result(ko, vo, want, what, sorted=True):
    wk, wv = want
    gk = rs.to_numpy_u32(ko)
    gv = None if vo is None else rs.to_numpy_u32(vo)
    assert (gv is None) == (wv is None), what
    if not sorted:  # the same entries in any order: compare as sorted (key, value) pairs
        if wv is None:
            gk, wk = np.sort(gk), np.sort(wk)
        else:
            g = np.lexsort((gv, gk))
            w = np.lexsort((wv, wk))
            gk, gv, wk, wv = gk[g], gv[g], wk[w], wv[w]
    assert np.array_equal(gk, wk), what
    if wv is not None:
        assert np.array_equal(gv, wv), what


def check_case(name, n, k, largest, mode, route=SELECT, sorted=True, report=True, d_x=None, d_v=None):
    d_x = dev(keys(name, n)) if d_x is None else d_x
    d_v = dev(values(n)) if (d_v is None and mode == "vals") else d_v
    with rs.topk_route(route):
        ko, vo, ws = call(d_x, n, k, largest, mode, d_v, sorted)
    what = (name, n, k, largest, mode, route, sorted)
    assert_result(ko, vo, expected(name, n, k, largest, mode), what, sorted)
    rep = rs.topk_report(n, k, mode != "keys", ws)
    if report:
        want = host_report(name, n, k, largest)
        if rep["route"] == SORT:
            want = {**{f: -1 for f in want}, "route": SORT, "kth_key": want["kth_key"]}
        assert rep == want, what
    return rep


# ------------------------------------------------------------------------------ sizes and ks
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_ks(n):
    d_x, d_v = dev(keys("uniform", n)), dev(values(n))
    for k in ks_for(n):
        for largest in (False, True):
            for mode in MODES:
                rep = check_case("uniform", n, k, largest, mode, d_x=d_x, d_v=d_v)
                assert rep["route"] == SELECT


@pytest.mark.parametrize("n", (65, 70001))
def test_unsorted(n):
    for k in ks_for(n):
        for largest in (False, True):
            for mode in MODES:
                check_case("zipf", n, k, largest, mode, sorted=False)


# ------------------------------------------------------------------------------ ties at the threshold
def test_ties_zipf():
    """k inside the run of the most frequent key: some of its copies are taken, the lowest positions, in order."""
    n = 200003
    x = keys("zipf", n)
    vals, counts = np.unique(x, return_counts=True)
    hot = vals[np.argmax(counts)]
    for largest in (False, True):
        o = order("zipf", n, largest)
        run = np.flatnonzero(x[o] == hot)  # the run's bounds in the host order
        lo, hi = int(run[0]), int(run[-1]) + 1
        assert hi - lo == counts.max() and hi - lo > 1000
        for k in (lo + 1, lo + 2, (lo + hi) // 2, hi - 1):
            for mode in MODES:
                rep = check_case("zipf", n, k, largest, mode)
                assert rep["kth_key"] == int(hot)
                assert rep["equal_taken"] == k - lo and rep["equal_taken"] < rep["equal_in_input"] == hi - lo


@pytest.mark.parametrize("name", ("equal", "ends"))
def test_ties_degenerate(name):
    n = 70001
    x = keys(name, n)
    zeros = int(np.count_nonzero(x == 0))
    for largest in (False, True):
        for k in sorted(k for k in {1, 2, 4097, n // 3, zeros, zeros + 1, n - zeros, n - zeros + 1, n - 1, n} if 1 <= k <= n):
            for mode in MODES:
                check_case(name, n, k, largest, mode)


# ------------------------------------------------------------------------------ digits that do not separate
def test_low_keys_keep_every_candidate():
    n = 200003
    for largest in (False, True):
        for k in (1, 65, n // 3, n - 1):
            for mode in ("keys", "indices"):
                rep = check_case("low10", n, k, largest, mode)
                assert rep["candidates"] == n  # the top digit (and the second) removed nothing


@pytest.mark.parametrize("name", ("top8", "sorted", "reverse"))
def test_other_inputs(name):
    n = 70001
    for largest in (False, True):
        for k in (1, 64, n // 3, n):
            for mode in MODES:
                check_case(name, n, k, largest, mode)


# ------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("n", (4097, 200003))
def test_routes_agree(n):
    d_x, d_v = dev(keys("zipf", n)), dev(values(n))
    for mode in MODES:
        lim = rs.topk_auto_limit(n, mode != "keys")
        assert 2 <= lim < n - 1
        for k in (lim // 2, lim, lim + 1, n - 1):  # at and below the limit AUTO selects, above it sorts
            for largest in (False, True):
                for sorted_ in (True, False):
                    got = {}
                    for route in (SELECT, SORT, AUTO):
                        with rs.topk_route(route):
                            ko, vo, ws = call(d_x, n, k, largest, mode, d_v, sorted_)
                        rep = rs.topk_report(n, k, mode != "keys", ws)
                        taken = route if route != AUTO else (SELECT if k <= lim else SORT)
                        assert rep["route"] == taken, (n, k, route)
                        assert rep["kth_key"] == host_report("zipf", n, k, largest)["kth_key"]
                        assert (rep["before"] == -1) == (taken == SORT)
                        assert_result(ko, vo, expected("zipf", n, k, largest, mode), (n, k, largest, mode, route), sorted_)
                        got[route] = (rs.to_numpy_u32(ko).tobytes(), b"" if vo is None else rs.to_numpy_u32(vo).tobytes())
                    if sorted_:
                        assert got[SORT] == got[SELECT] == got[AUTO], (n, k, largest, mode)


# ------------------------------------------------------------------------------ grid-stride
@pytest.mark.parametrize("limit", (1, 3))
def test_grid_limit(limit):
    n = 70001  # 18 tiles
    with rs.topk_grid_limit(limit):
        assert set(rs.topk_grids(n, 5, True).values()) == {limit}
        for name in ("uniform", "low10"):
            for k in (1, 4097, n // 3, n):
                for largest in (False, True):
                    check_case(name, n, k, largest, "indices")
                    check_case(name, n, k, largest, "vals", sorted=False)
    assert min(rs.topk_grids(n, 5, True).values()) > 3


def test_every_workgroup_walks_two_tiles():
    n = 1 << 22
    g = rs.topk_grids(n, 1000, True)
    tiles = n // rs.TOPK_TILE_KEYS
    assert tiles // g["count"] >= 2 and tiles // g["compact"] >= 2, g  # without the hook
    for largest, mode, k in ((False, "indices", 1000), (True, "vals", n // 3), (False, "keys", 1)):
        check_case("uniform", n, k, largest, mode)
    check_case("low10", n, 70001, True, "indices")  # the candidate list's kernels walk two tiles each as well


def test_input_smaller_than_the_grid():
    n = 63
    assert min(rs.topk_grids(n, 5, True).values()) > n  # most slices are empty
    for name in ("uniform", "equal", "low10"):
        for k in (1, 5, 62, 63):
            for largest in (False, True):
                check_case(name, n, k, largest, "indices")


# ------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("off", (1, 2, 3))
def test_alignment(off):
    n = 70001
    x, v = keys("uniform", n), values(n)
    bx, bv = torch.zeros(n + 8, dtype=torch.int32, device="cuda"), torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    assert bx.data_ptr() % 16 == 0 and bv.data_ptr() % 16 == 0
    d_x, d_v = bx[off:off + n], bv[off:off + n]
    d_x.copy_(dev(x))
    d_v.copy_(dev(v))
    for route in (SELECT, SORT):
        for k in (65, n // 3):
            for largest in (False, True):
                for mode in MODES:
                    bo, bvo = rs.empty_u32(k + 8), rs.empty_u32(k + 8)
                    out = (bo[off:off + k], None if mode == "keys" else bvo[off:off + k])
                    wsb = rs.topk_workspace_size(n, k, mode != "keys", route)
                    ws = rs.workspace(wsb + 16)[4 * off:4 * off + wsb]
                    assert ws.data_ptr() % 16 == 4 * off and out[0].data_ptr() % 16 == 4 * off
                    with rs.topk_route(route):
                        ko, vo, _ = call(d_x, n, k, largest, mode, d_v, ws=ws, out=out)
                    assert_result(ko, vo, expected("uniform", n, k, largest, mode), (off, route, k, largest, mode))


# ------------------------------------------------------------------------------ workspace state
@pytest.mark.parametrize("route", (SELECT, SORT))
def test_workspace_state(route):
    """The same call gives the same bytes over a workspace of zeros, of 0xFF, one a different top-k call left behind
    and one a sort left behind."""
    n, k = 200003, 5000
    d_x, d_v = dev(keys("zipf", n)), dev(values(n))
    d_y = dev(keys("low10", n))
    with rs.topk_route(route):
        for largest, mode in ((False, "vals"), (True, "indices"), (True, "keys")):
            pairs = mode != "keys"
            wsb = rs.topk_workspace_size(n, k, pairs, route)
            want = expected("zipf", n, k, largest, mode)

            def fresh(kind):
                ws = torch.empty(max(wsb, rs.topk_workspace_size(n, n // 2, True, route), rs.workspace_size(n, 8, True)),
                                 dtype=torch.uint8, device="cuda")
                if kind == "zero":
                    ws.zero_()
                elif kind == "ff":
                    ws.fill_(0xFF)
                elif kind == "topk":  # another input, k, direction and kind
                    call(d_y, n, n // 2, not largest, "indices", ws=ws)
                else:
                    rs.sort_device(d_x, rs.empty_u32(n), 8, vals_in=d_v, vals_out=rs.empty_u32(n), ws=ws)
                return ws

            seen = set()
            for kind in ("zero", "ff", "topk", "sort"):
                ws = fresh(kind)
                ko, vo, _ = call(d_x, n, k, largest, mode, d_v, ws=ws)
                assert_result(ko, vo, want, (route, largest, mode, kind))
                rep = rs.topk_report(n, k, pairs, ws)
                seen.add((rs.to_numpy_u32(ko).tobytes(), b"" if vo is None else rs.to_numpy_u32(vo).tobytes(),
                          tuple(rep.items())))
            assert len(seen) == 1


# ------------------------------------------------------------------------------ graph replay
def captured(call_):
    """As tests/test_gpu_workspace_state.py: run once uncaptured, then captured alone, once, on one side stream."""
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        call_()
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        call_()
    return g, st


@pytest.mark.parametrize("largest,mode", ((False, "indices"), (True, "vals")))
def test_graph_replay(largest, mode):
    n, k = 70001, 3000
    names = ("uniform", "low10", "zipf")  # different thresholds and candidate counts
    src = {nm: dev(keys(nm, n)) for nm in names}
    reps = [host_report(nm, n, k, largest) for nm in names]
    assert len({(r["kth_key"], r["candidates"]) for r in reps}) == 3
    d_x, d_v = dev(keys("uniform2", n)), dev(values(n))
    out = (rs.empty_u32(k), rs.empty_u32(k))
    with rs.topk_route(SELECT):
        ws = rs.workspace(rs.topk_workspace_size(n, k, True, SELECT))
        ws.fill_(0xA5)
        g, st = captured(lambda: call(d_x, n, k, largest, mode, d_v, ws=ws, out=out))
    with torch.cuda.stream(st):
        for nm, want_rep in zip(names, reps):
            d_x.copy_(src[nm])
            out[0].zero_()
            out[1].zero_()
            g.replay()
            assert rs.topk_report(n, k, True, ws, st) == want_rep, nm
            assert_result(out[0], out[1], expected(nm, n, k, largest, mode), nm)
        st.synchronize()


# ------------------------------------------------------------------------------ host entry
def test_host_entry():
    n = 70001
    x, v = keys("zipf", n), values(n)
    for k in (1, 100, n):
        for largest in (False, True):
            ko, vo = rs.topkByDevice(x, k, largest=largest)
            wk, _ = expected("zipf", n, k, largest, "keys")
            assert vo is None and np.array_equal(ko, wk)
            ko, vo = rs.topkByDevice(x, k, largest=largest, vals=v)
            wk, wv = expected("zipf", n, k, largest, "vals")
            assert np.array_equal(ko, wk) and np.array_equal(vo, wv)
            ko, vo = rs.topkByDevice(x, k, largest=largest, indices=True)
            wk, wv = expected("zipf", n, k, largest, "indices")
            assert np.array_equal(ko, wk) and np.array_equal(vo, wv)


# ------------------------------------------------------------------------------ unchanged behaviour
def test_no_new_scatter_kernels():
    known = rs.scatter_kernels_known()
    assert len(known) == KNOWN_SCATTER_KERNELS
    rs.scatter_kernels_used(reset=True)
    n = 200003
    for route in (SELECT, SORT):
        for mode in MODES:
            check_case("uniform", n, n // 3, True, mode, route=route)
            check_case("uniform", n, 64, False, mode, route=route, sorted=False)
    used = rs.scatter_kernels_used()
    assert used and set(used) <= set(known) | {"rs_bucket_sort16"}, used
