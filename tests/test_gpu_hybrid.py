"""GPU tests of the hybrid route (rsort_set_hybrid; rsort_hybrid.hip and sort_planned in rsort_capi.cpp): a joint
histogram of (digit 3, digit 2), two MSD passes and the in-LDS bucket finish, against the oracle (Baseline1.cu:15-64
restated), with the route the device took read back through rsort_hybrid_report.

The small cases run under HYBRID_FORCE on plans of 512 or 768 line tiles with exactly 256 chunks (a 256-CU device
takes line tiles from 512 tiles on, so these are the smallest plans the route can run on); every constructed input
is checked on the CPU first for the bucket sizes it claims. Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import oracle_sort, uniform_keys, zipf_keys

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LINE_TILE = 16384
CAP = rs.hybrid_capacity()
NS = 768 * LINE_TILE - 5  # (the smallest ragged n with 256 chunks of line tiles: under 512 tiles no line tiles)
N768 = 768 * LINE_TILE - 77


def group_plan(n, k=8, pairs=False):
    tiles = (n + LINE_TILE - 1) // LINE_TILE
    assert tiles % 256 == 0
    p = rs.plan(n, k, pairs, tiles // 256)
    assert p.num_chunks == 256 and p.tile_keys == LINE_TILE, p.as_dict()
    return p


def bucket_sizes(x):
    return np.bincount(x >> np.uint32(16), minlength=65536)


def bucketed(sizes, seed):
    """Keys whose top 16 bits are bucket b for sizes[b] keys each, low 16 bits uniform, in shuffled order."""
    rng = np.random.default_rng(seed)
    top = np.repeat(np.arange(65536, dtype=np.uint32), sizes)
    x = (top << np.uint32(16)) | rng.integers(0, 65536, top.size, dtype=np.uint32)
    rng.shuffle(x)
    assert np.array_equal(bucket_sizes(x), sizes)
    return x


def fat_sizes(n, per=14000, special=()):
    """~n / per buckets of about `per` keys over ~150 digit-3 values (0x00 and 0xFF among them; the rest of the
    256 groups are empty), six digit-2 values each; `special`: (bucket, size) pairs set first."""
    sizes = np.zeros(65536, dtype=np.int64)
    for b, s in special:
        sizes[b] = s
    taken = {b for b, _ in special}
    d3s = [0x00, 0xFF] + [d for d in range(3, 253, 5)] + [d for d in range(4, 254, 5)] + [d for d in range(6, 250, 5)]
    ids = [d3 * 256 + d2 for d3 in d3s for d2 in (0x00, 0x33, 0x5A, 0xA5, 0xCC, 0xFF) if d3 * 256 + d2 not in taken]
    left = n - int(sizes.sum())
    nb = max(1, min(len(ids), left // per))
    ids = ids[:: max(1, len(ids) // nb)][:nb]  # (digit-3 groups 0x00 and 0xFF come first in the list)
    base, extra = divmod(left, len(ids))
    for i, b in enumerate(ids):
        sizes[b] = base + (1 if i < extra else 0)
    assert sizes.sum() == n
    return sizes


def sort_forced(x, p=None, mode=None, out=None):
    """One sort of x (into `out` or a fresh buffer) under `mode` (default FORCE): (output, report, check flags)."""
    p = p if p is not None else group_plan(x.size)
    d_in = rs.from_numpy_u32(x)
    d_out = out if out is not None else rs.empty_u32(x.size)
    ws = rs.workspace(p.workspace_bytes)
    with rs.hybrid(rs.HYBRID_FORCE if mode is None else mode):
        rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p)
    rep = rs.hybrid_report(p, ws)
    chk = rs.plan_check(p, ws)
    assert np.array_equal(rs.to_numpy_u32(d_in), x), "input buffer was modified"
    return rs.to_numpy_u32(d_out), rep, chk


@functools.lru_cache(maxsize=None)
def fat_input():
    sizes = fat_sizes(NS)
    x = bucketed(sizes, seed=1)
    return x, oracle_sort(x, 8)


def test_few_fat_buckets():
    x, want = fat_input()
    sizes = bucket_sizes(x)
    live = sizes[sizes > 0]
    assert 800 <= live.size <= 1000 and live.min() >= 13000 and live.max() <= CAP
    g = sizes.reshape(256, 256).sum(axis=1)
    assert g[0] > 0 and g[255] > 0 and (g == 0).sum() >= 64  # digit-3 groups 0x00 and 0xFF live, many empty
    y, rep, chk = sort_forced(x)
    assert rep["eligible"] and rep["hybrid"] and rep["max_bucket"] == live.max() and chk == 0
    assert np.array_equal(y, want)
    assert any(k.startswith("rs_bucket_sort16") for k in rs.scatter_kernels_used())


def test_capacity_edge():
    big = 0x5A * 256 + 0xA5
    s0 = fat_sizes(NS, special=[(big, CAP)])
    assert s0.max() == CAP and s0[big] == CAP
    x0 = bucketed(s0, seed=2)
    y0, rep0, chk0 = sort_forced(x0)
    assert rep0["hybrid"] and rep0["max_bucket"] == CAP and chk0 == 0
    assert np.array_equal(y0, oracle_sort(x0, 8))
    # one more key in that bucket (taken from another): the exact count says overflow, the LSD passes sort
    s1 = s0.copy()
    donor = int(np.flatnonzero((s1 > 0) & (np.arange(65536) != big))[0])
    s1[donor] -= 1
    s1[big] += 1
    x1 = bucketed(s1, seed=3)
    assert bucket_sizes(x1).max() == CAP + 1
    y1, rep1, chk1 = sort_forced(x1)
    assert rep1["eligible"] and not rep1["hybrid"] and rep1["max_bucket"] == CAP + 1 and chk1 == 0
    assert np.array_equal(y1, oracle_sort(x1, 8))


def test_odd_bucket_sizes():
    """Buckets of 1, 1025, 63, 65, 1023 and capacity - 1 keys come first (their starts 1, 1026, 1089, 1154 and
    2177 are aligned neither to 16 B nor to 128 B), then an empty one and one of exactly 64."""
    odd = [1, 1025, 63, 65, 1023, CAP - 1, 0, 64]
    sizes = fat_sizes(NS, special=list(enumerate(odd)))
    assert list(sizes[:8]) == odd
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert all(int(starts[b]) % 4 != 0 for b in (1, 2, 3, 4, 5))
    x = bucketed(sizes, seed=4)
    y, rep, chk = sort_forced(x)
    assert rep["hybrid"] and rep["max_bucket"] <= CAP and chk == 0
    assert np.array_equal(y, oracle_sort(x, 8))


def test_tiny_buckets():
    """Full-range uniform keys forced at the smallest ragged plan the route runs on: 65536 buckets of ~192 keys.
    (No plan of 2^22 + 5 keys has line tiles: a 256-CU device takes them from 512 tiles on, so the buckets of
    full-range keys cannot average under 128; the second input makes every odd bucket 16 times rarer: ~23 keys,
    shorter than one wave slot.)"""
    x = uniform_keys(NS, seed=5)
    s = bucket_sizes(x)
    assert 64 < s.min() and s.max() < 300
    y, rep, chk = sort_forced(x)
    assert rep["hybrid"] and rep["max_bucket"] == s.max() and chk == 0
    assert np.array_equal(y, oracle_sort(x, 8))
    rng = np.random.default_rng(6)
    w = np.where(np.arange(65536) % 2 == 1, 1.0, 16.0)
    x2 = (rng.choice(65536, size=NS, p=w / w.sum()).astype(np.uint32) << np.uint32(16)) | \
        rng.integers(0, 65536, NS, dtype=np.uint32)
    s2 = bucket_sizes(x2)
    assert np.median(s2[1::2]) < 32 and s2.min() < 16 and s2.max() < 512
    y2, rep2, chk2 = sort_forced(x2)
    assert rep2["hybrid"] and chk2 == 0
    assert np.array_equal(y2, oracle_sort(x2, 8))


def _hot(n, seed):
    x = uniform_keys(n, seed=seed)
    x[::4] = 0x00C0FFEE
    return x


GATE_INPUTS = {
    "equal": lambda n: np.full(n, 0x01234567, dtype=np.uint32),
    "hot": lambda n: _hot(n, 21),
    "zipf": lambda n: zipf_keys(n, seed=22),
    "small": lambda n: uniform_keys(n, seed=23) >> np.uint32(16),
    "sorted": lambda n: np.sort(uniform_keys(n, seed=24)),
    "reversed": lambda n: np.sort(uniform_keys(n, seed=25))[::-1].copy(),
}


@pytest.mark.parametrize("name", list(GATE_INPUTS))
def test_gate_verdicts(name):
    """The smallest automatically eligible sort is 2^29 keys (seconds of oracle time per input), so the gate runs
    here under FORCE, which reports its verdict and ignores it: the skewed inputs' verdict is SKEWED and the exact
    count then sends them to the LSD passes; sorted and reversed uniform keys pass the gate and take the hybrid."""
    x = GATE_INPUTS[name](NS)
    y, rep, chk = sort_forced(x)
    assert rep["eligible"] and chk == 0
    if name in ("sorted", "reversed"):
        assert rep["gate"] == rs.GATE_PASS and rep["hybrid"]
    else:
        assert bucket_sizes(x).max() > CAP
        assert rep["gate"] == rs.GATE_SKEWED and not rep["hybrid"]
    assert np.array_equal(y, oracle_sort(x, 8))


@pytest.mark.parametrize("route", ["inplace", "pairs", "k4", "ballot", "no_groups", "per_call"])
def test_ineligible_routes(route):
    x = uniform_keys(NS, seed=31)
    with rs.hybrid(rs.HYBRID_FORCE):
        if route == "pairs":
            n = 512 * 8192
            x = x[:n].copy()
            v = np.arange(n, dtype=np.uint32)
            p = rs.plan(n, 8, True, 2)
            ws = rs.workspace(p.workspace_bytes)
            ko, vo = rs.empty_u32(n), rs.empty_u32(n)
            rs.sort_device(rs.from_numpy_u32(x), ko, 8, vals_in=rs.from_numpy_u32(v), vals_out=vo, ws=ws, plan_=p)
            y = rs.to_numpy_u32(ko)
        elif route == "k4":
            p = rs.plan(NS, 4)
            ws = rs.workspace(p.workspace_bytes)
            d_out = rs.empty_u32(NS)
            rs.sort_device(rs.from_numpy_u32(x), d_out, 4, ws=ws, plan_=p)
            y = rs.to_numpy_u32(d_out)
        else:
            p = group_plan(NS)
            ws = rs.workspace(p.workspace_bytes)
            d_in = rs.from_numpy_u32(x)
            d_out = d_in if route == "inplace" else rs.empty_u32(NS)
            if route == "ballot":
                with rs.rank_algo(rs.RANK_BALLOT):
                    rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p)
            elif route == "no_groups":
                with rs.group_chunks(False):
                    rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p)
            else:  # in place, or kept off the route for this call (the multi-GPU local sorts' flag)
                rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p, hybrid=route != "per_call")
            y = rs.to_numpy_u32(d_out)
    rep = rs.hybrid_report(p, ws)
    assert rep == {"eligible": False, "gate": rs.GATE_NONE, "max_bucket": 0, "hybrid": False}
    assert rs.plan_check(p, ws) == 0
    assert np.array_equal(y, oracle_sort(x, 4 if route == "k4" else 8))


def test_unaligned_output():
    """A 4-B-aligned output 4 bytes past a 16-B boundary, n no multiple of the tile: the hybrid runs, and the
    words around the output keep their fill."""
    n = N768
    x = uniform_keys(n, seed=41)
    fill = 0x5A5A5A5A
    big = torch.full((n + 64,), fill, dtype=torch.int32, device="cuda")
    out = big[33:33 + n]
    assert out.data_ptr() % 16 == 4
    y, rep, chk = sort_forced(x, out=out)
    assert rep["hybrid"] and chk == 0
    assert np.array_equal(y, oracle_sort(x, 8))
    assert int((big[:33] != fill).sum()) == 0 and int((big[33 + n:] != fill).sum()) == 0


def test_rank_check():
    x, _ = fat_input()
    p = group_plan(x.size)
    ws = rs.workspace(p.workspace_bytes)
    d_in, d_out = rs.from_numpy_u32(x), rs.empty_u32(x.size)
    with rs.hybrid(rs.HYBRID_FORCE):
        with rs.rank_fault():
            rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p)
        assert rs.hybrid_report(p, ws)["hybrid"]
        assert rs.plan_check(p, ws) & rs.CHECK_RANK_ORDER
        rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p)
        assert rs.hybrid_report(p, ws)["hybrid"] and rs.plan_check(p, ws) == 0


def test_headline_shape_auto_and_off():
    """2^30 uniform keys under AUTO: eligible, gate passed, every bucket within the capacity, the hybrid route;
    the output checked on the device (sorted, the input's multiset fingerprint). OFF: today's path, digit groups
    on both odd passes. Zipf keys of the same size under AUTO: the gate's SKEWED verdict, the LSD passes."""
    n = 1 << 30
    lo, hi = rs.hybrid_range()
    assert lo <= n <= hi
    p = rs.plan(n, 8)
    assert p.num_chunks == 256, p.as_dict()
    keys, out = rs.empty_u32(n), rs.empty_u32(n)
    ws = rs.workspace(p.workspace_bytes)
    rs.gen_uniform(keys, 0x5EED)
    fp_in = rs.fingerprint(keys)[0]
    assert rs.get_hybrid() == rs.HYBRID_AUTO
    rs.sort_device(keys, out, 8, ws=ws, plan_=p)
    rep = rs.hybrid_report(p, ws)
    assert rep["eligible"] and rep["gate"] == rs.GATE_PASS and 0 < rep["max_bucket"] <= CAP and rep["hybrid"]
    assert rs.plan_check(p, ws) == 0
    assert rs.fingerprint(out) == (fp_in, 0)
    out.zero_()
    with rs.hybrid(rs.HYBRID_OFF):
        rs.sort_device(keys, out, 8, ws=ws, plan_=p)
    assert rs.group_flags(p, ws) == [1, 1]
    assert not rs.hybrid_report(p, ws)["eligible"]
    assert rs.fingerprint(out) == (fp_in, 0)
    from _util import zipf_cdf_u32
    rs.gen_zipf(keys, rs.from_numpy_u32(zipf_cdf_u32()), 0x5EED)
    fp_z = rs.fingerprint(keys)[0]
    rs.sort_device(keys, out, 8, ws=ws, plan_=p)
    rep = rs.hybrid_report(p, ws)
    assert rep["eligible"] and rep["gate"] == rs.GATE_SKEWED and rep["max_bucket"] == 0 and not rep["hybrid"]
    assert rs.plan_check(p, ws) == 0
    assert rs.fingerprint(out) == (fp_z, 0)
