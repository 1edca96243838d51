"""The top-k selection (include/rsort.h "top-k selection") at the sizes its contract names: n past 2^31,
n = 2^32 - 20 and the README's 2^30 keys with k = 2^20. Both select files carry every position, count and offset in
32-bit words; below 2^22 keys (tests/test_gpu_topk.py) a signed word, a missing widening or a 32-bit product cannot
show.

The inputs past 2^31 are periodic, x[i] = base[i % 4099], built on the device in pieces. For those the contract's
answer -- the first k entries of the stable ascending order of x ^ m -- and the report's counts have a closed form
in `base` alone (tests/_util.py periodic_topk_expected / periodic_topk_report, pinned to the oracle on the CPU by
tests/test_topk.py). Every key, value, position and report word is compared bit for bit, on the device; the expected
keys and values are also gathered from the inputs at the expected positions. Each case first asserts on the host what
it is for: expected positions at or above 2^31, a candidate list of all n entries, hundreds of tiles per workgroup.
Runs on the MI355X box (-m gpu); the largest case holds about 52 GB."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import (PERIODIC_POSITION_TABLES, periodic_topk_expected, periodic_topk_positions, periodic_topk_report,
                   periodic_topk_tables, uniform_keys)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SELECT, SORT = rs.TOPK_SELECT, rs.TOPK_SORT
M32 = 0xFFFFFFFF
P = 4099
N31 = (1 << 31) + (1 << 17) + 5
PIECE = 1 << 26


def as_u64(t):
    return t.to(torch.int64) & M32


@functools.lru_cache(maxsize=None)
def base_keys(kind):
    if kind == "distinct":  # about n / P = 524k copies of every key, spread over the whole input
        b = uniform_keys(P, seed=0xA11)
        assert np.unique(b).size == P
    else:  # "low10", below 2^10: every level but the last keeps every candidate, A is the whole input
        b = uniform_keys(P, seed=9) >> np.uint32(22)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    b.setflags(write=False)
    return b


def fill_periodic(dst, base):
    """dst[i] = base[i % P] over a device view of n words, in pieces (never an n-element int64 tensor)."""
    b = rs.from_numpy_u32(base.copy())
    for lo in range(0, dst.numel(), PIECE):
        hi = min(dst.numel(), lo + PIECE)
        dst[lo:hi] = b[torch.arange(lo, hi, dtype=torch.int64, device=dst.device) % P]


def call(x, k, largest, mode, vals=None, sorted=True, route=SELECT):
    with rs.topk_route(route):
        return rs.topk_device(x, k, largest=largest, vals=vals if mode == "vals" else None, indices=mode == "indices",
                              sorted=sorted)


def assert_matches(ko, vo, x, vals, want, mode, what, sorted=True):
    """want: the helper's (keys, positions), numpy. Everything bit for bit, on the device."""
    wk, wp = want
    pos = torch.from_numpy(wp).cuda()
    ek = as_u64(rs.from_numpy_u32(wk))
    assert torch.equal(as_u64(x[pos]), ek), what  # (the helper's keys are the input's at its positions)
    gk = as_u64(ko)
    if mode == "keys":
        assert vo is None, what
        assert torch.equal(gk, ek), what
        return
    ev = pos if mode == "indices" else as_u64(vals[pos])
    gv = as_u64(vo)
    if not sorted:  # the same (key, value) pairs in any order: both sides as sorted 64-bit words
        g, e = torch.sort((gk << 32) | gv).values, torch.sort((ek << 32) | ev).values
        assert torch.equal(g, e), what
        return
    assert torch.equal(gk, ek), what
    assert torch.equal(gv, ev), what


def select_report(base, n, k, largest):
    return {"route": SELECT, **periodic_topk_report(base, n, k, largest)}


def positions_past_2_31(base, n, k, largest):
    """The largest expected position among the first k: the last copy of every value taken whole, and rank k - 1."""
    tab = periodic_topk_tables(base, n, largest)
    ranks = np.r_[tab["gend"][(tab["gcount"] > 0) & (tab["gend"] <= k)] - 1, k - 1].astype(np.int64)
    return int(periodic_topk_positions(tab, ranks)[0].max())


# ------------------------------------------------------------------------------ a. past 2^31, a threshold inside a run
@pytest.mark.parametrize("largest", (False, True))
def test_select_past_2_31(largest):
    """n = 2^31 + 2^17 + 5 of 4099 distinct keys, k = 600000: every copy of the first key and part of the next key's
    copies, positions all over the input. Keys, values and indices; indices UNSORTED; and the input one word past a
    256-B boundary (tk_count<0>'s scalar path, a.vec == 0)."""
    n, k = N31, 600000
    base = base_keys("distinct")
    want = periodic_topk_expected(base, n, k, largest)
    assert int(want[1].max()) >= 1 << 31 and positions_past_2_31(base, n, k, largest) == int(want[1].max())
    want_rep = select_report(base, n, k, largest)
    assert 0 < want_rep["equal_taken"] < want_rep["equal_in_input"] and want_rep["before"] > 0
    big = rs.empty_u32(n + 64)
    assert big.data_ptr() % 256 == 0
    x = big[:n]
    fill_periodic(x, base)
    vals = rs.empty_u32(n)
    rs.gen_uniform(vals, 0xBEEF)  # (never the positions)
    for mode in ("keys", "vals", "indices"):
        ko, vo, ws = call(x, k, largest, mode, vals)
        assert rs.topk_report(n, k, mode != "keys", ws) == want_rep, (largest, mode)
        del ws
        assert_matches(ko, vo, x, vals, want, mode, (largest, mode))
    ko, vo, ws = call(x, k, largest, "indices", sorted=False)
    assert rs.topk_report(n, k, True, ws) == want_rep, (largest, "unsorted")
    del ws
    assert_matches(ko, vo, x, vals, want, "indices", (largest, "unsorted"), sorted=False)
    del vals
    x = big[1:n + 1]
    assert x.data_ptr() % 256 == 4
    fill_periodic(x, base)
    ko, vo, ws = call(x, k, largest, "indices")
    assert rs.topk_report(n, k, True, ws) == want_rep, (largest, "one word past 256 B")
    del ws
    assert_matches(ko, vo, x, None, want, "indices", (largest, "one word past 256 B"))


# ------------------------------------------------------------------------------ b. the candidate list is the input
@pytest.mark.parametrize("largest", (False, True))
def test_select_past_2_31_every_candidate_kept(largest):
    """The same n of 4099 keys below 2^10, with indices: every level but the last keeps every candidate, so A holds
    n > 2^31 entries and the compact's offsets, the level-1 and level-2 counts and the emit's bases pass 2^31.
    k = 2^20 (its positions stay below 2^31: a key has 2^21 copies or more), then k = the automatic limit, n / 2,
    whose expected positions pass 2^31 and which the host does not expand: the closed form's own lines
    (periodic_topk_positions, checked on torch tensors by tests/test_topk.py) run on the device, piece by piece."""
    n = N31
    base = base_keys("low10")
    x = rs.empty_u32(n)
    fill_periodic(x, base)
    k = 1 << 20
    want_rep = select_report(base, n, k, largest)
    assert want_rep["candidates"] == n
    ko, vo, ws = call(x, k, largest, "indices")
    assert rs.topk_report(n, k, True, ws) == want_rep, (largest, k)
    del ws
    assert_matches(ko, vo, x, None, periodic_topk_expected(base, n, k, largest), "indices", (largest, k))
    del ko, vo

    k = rs.topk_auto_limit(n, True)
    assert k == n // 2
    want_rep = select_report(base, n, k, largest)
    assert want_rep["candidates"] == n and positions_past_2_31(base, n, k, largest) >= 1 << 31
    ko, vo, ws = call(x, k, largest, "indices")
    assert rs.topk_report(n, k, True, ws) == want_rep, (largest, k)
    del ws
    tab = periodic_topk_tables(base, n, largest)
    dev = {f: torch.from_numpy(tab[f]).cuda() for f in PERIODIC_POSITION_TABLES}
    dev["P"] = P
    gkey = torch.from_numpy(tab["gx"] ^ tab["m"]).cuda()
    top = 0
    for lo in range(0, k, PIECE):
        hi = min(k, lo + PIECE)
        pos, g = periodic_topk_positions(dev, torch.arange(lo, hi, dtype=torch.int64, device="cuda"))
        top = max(top, int(pos.max()))
        assert torch.equal(as_u64(vo[lo:hi]), pos), (largest, k, lo)
        assert torch.equal(as_u64(ko[lo:hi]), gkey[g]), (largest, k, lo)
        assert torch.equal(ko[lo:hi], x[pos]), (largest, k, lo)
    assert top >= 1 << 31


# ------------------------------------------------------------------------------ c. the SORT route past 2^31
def test_sort_route_past_2_31():
    """What AUTO takes above its limit, at n > 2^31 with values and with indices, the k largest: a pairs sort of more
    than 2^31 entries (with indices: an iota payload). Against the closed form, and byte for byte against SELECT."""
    n, k, largest = N31, 600000, True
    base = base_keys("distinct")
    want = periodic_topk_expected(base, n, k, largest)
    assert int(want[1].max()) >= 1 << 31
    kth = periodic_topk_report(base, n, k, largest)["kth_key"]
    x = rs.empty_u32(n)
    fill_periodic(x, base)
    vals = rs.empty_u32(n)
    rs.gen_uniform(vals, 0xBEEF)
    for mode in ("indices", "vals"):
        sk, sv, ws = call(x, k, largest, mode, vals, route=SELECT)
        assert rs.topk_report(n, k, True, ws)["route"] == SELECT
        del ws
        ko, vo, ws = call(x, k, largest, mode, vals, route=SORT)
        assert rs.topk_report(n, k, True, ws) == {"route": SORT, "kth_key": kth, "before": -1, "equal_taken": -1,
                                                  "equal_in_input": -1, "candidates": -1}, mode
        del ws
        assert_matches(ko, vo, x, vals, want, mode, ("sort", mode))
        assert torch.equal(ko, sk) and torch.equal(vo, sv), mode
        del ko, vo, sk, sv


# ------------------------------------------------------------------------------ d. the README's shape
@pytest.mark.parametrize("largest", (False, True))
def test_select_2_30_uniform(largest):
    """2^30 uniform keys, k = 2^20, keys only and with indices. Expected: the first k of the pairs sort of
    (x ^ m, iota), xor-ed back (that sort is pinned to the oracle at this size by tests/test_gpu_fullsize.py); the
    report's counts against torch counts over the input. Every select workgroup walks 64 tiles or more, unhooked."""
    n, k = 1 << 30, 1 << 20
    m = M32 if largest else 0
    grids = rs.topk_grids(n, k, True)
    tiles = n // rs.TOPK_TILE_KEYS
    assert set(grids) == set(rs.TOPK_KERNELS) and all(tiles // g >= 64 for g in grids.values()), grids
    x = rs.empty_u32(n)
    rs.gen_uniform(x, 0x5EED)
    xm = torch.bitwise_not(x) if largest else x
    iota = rs.empty_u32(n)
    rs.gen_iota(iota, 0)
    rk, rv = rs.empty_u32(n), rs.empty_u32(n)
    rs.sort_device(xm, rk, 8, vals_in=iota, vals_out=rv)
    ek = torch.bitwise_not(rk[:k]) if largest else rk[:k].clone()
    ei = rv[:k].clone()
    del rk, rv, iota, xm
    assert torch.equal(x[as_u64(ei)], ek)
    t = int(as_u64(ek[k - 1:k])[0]) ^ m  # the k-th x
    before = equal = cand = 0
    for lo in range(0, n, PIECE):
        u = as_u64(x[lo:lo + PIECE]) ^ m
        before += int((u < t).sum())
        equal += int((u == t).sum())
        cand += int(((u >> 24) == (t >> 24)).sum())
    del u
    assert before < k <= before + equal and k < cand < n
    want_rep = {"route": SELECT, "kth_key": t ^ m, "before": before, "equal_taken": k - before,
                "equal_in_input": equal, "candidates": cand}
    for mode in ("keys", "indices"):
        ko, vo, ws = call(x, k, largest, mode)
        assert rs.topk_report(n, k, mode != "keys", ws) == want_rep, (largest, mode)
        del ws
        assert torch.equal(ko, ek), (largest, mode)
        assert (vo is None) if mode == "keys" else torch.equal(vo, ei), (largest, mode)


# ------------------------------------------------------------------------------ e. the largest n the entry takes
@pytest.mark.parametrize("largest", (False, True))
def test_select_near_2_32_every_candidate_kept(largest):
    """n = 2^32 - 20 of the keys below 2^10, keys only, k = 2^20: the candidate list is the whole input, so the
    counts and offsets of every level run to n itself -- the case aimed at 32-bit wrap rather than sign."""
    n, k = (1 << 32) - 20, 1 << 20
    base = base_keys("low10")
    want_rep = select_report(base, n, k, largest)
    assert want_rep["candidates"] == n and n + 20 == 1 << 32
    x = rs.empty_u32(n)
    fill_periodic(x, base)
    ko, vo, ws = call(x, k, largest, "keys")
    assert rs.topk_report(n, k, False, ws) == want_rep, largest
    del ws
    assert_matches(ko, vo, x, None, periodic_topk_expected(base, n, k, largest), "keys", largest)
