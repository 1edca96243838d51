"""GPU tests of the hybrid route's bucket kernel with its 16-bit LDS tile (rs_bucket_sort16, rsort_hybrid.hip):
keys and ranks packed two per register, low halves staged as uint16_t and widened with the bucket index on the
way out, two workgroups resident per CU.

Every case runs under HYBRID_FORCE on the smallest plan the route runs on (768 line tiles, n = 768 * 16384 - 5),
is compared bit-exact with the oracle, and requires the hybrid route and a clean check word; every constructed
input is checked on the CPU first for the bucket sizes it claims. Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import oracle_sort
from test_gpu_hybrid import CAP, NS, bucket_sizes, bucketed, fat_sizes, sort_forced

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EXTREMES = np.array([0x0000, 0xFFFF, 0x00FF, 0xFF00, 0x0100, 0xFEFF], dtype=np.uint32)
B_FULL, B_ZERO, B_65 = 0x5A * 256 + 0xA5, 0x03 * 256 + 0x34, 0xFF * 256 + 0xFE


def sorted_hybrid(x, out=None):
    y, rep, chk = sort_forced(x, out=out)
    assert rep["eligible"] and rep["hybrid"] and rep["max_bucket"] <= CAP, rep
    assert chk == 0
    return y


def test_low_half_extremes():
    """Low halves from {0x0000, 0xFFFF, 0x00FF, 0xFF00, 0x0100, 0xFEFF} only, no bucket size a multiple of 64: a
    full bucket of 0xFFFF (every real key looks like a pad; one counter takes each wave's 1152 adds in both passes,
    ranks and positions at their maxima), capacity - 1 zeros, and 65 keys of which 64 are 0xFFFF."""
    sizes = fat_sizes(NS, special=[(B_FULL, CAP), (B_ZERO, CAP - 1), (B_65, 65)])
    live = sizes[sizes > 0]
    assert sizes[B_FULL] == CAP and sizes[B_ZERO] == CAP - 1 and sizes[B_65] == 65 and sizes.max() == CAP
    others = np.delete(sizes, B_FULL)
    assert live.size > 800 and not (others[others > 0] % 64 == 0).any()
    rng = np.random.default_rng(61)
    top = np.repeat(np.arange(65536, dtype=np.uint32), sizes)
    low = EXTREMES[rng.integers(0, EXTREMES.size, top.size)]
    low[top == B_FULL] = 0xFFFF
    low[top == B_ZERO] = 0x0000
    at = np.flatnonzero(top == B_65)
    low[at] = 0xFFFF
    low[at[37]] = 0x00FF
    x = (top << np.uint32(16)) | low
    rng.shuffle(x)
    assert np.array_equal(bucket_sizes(x), sizes)
    assert set(np.unique(x & np.uint32(0xFFFF)).tolist()) == set(EXTREMES.tolist())
    assert int((x == np.uint32((B_FULL << 16) | 0xFFFF)).sum()) == CAP
    assert int((x == np.uint32(B_ZERO << 16)).sum()) == CAP - 1
    assert int((x == np.uint32((B_65 << 16) | 0xFFFF)).sum()) == 64
    assert np.array_equal(sorted_hybrid(x), oracle_sort(x, 8))


ALIGN_SIZES = [1, 2, 3, 5, 7, 9, 11, 13, 4, 8, 6, 10, 12, 14, 15, 17]


@functools.lru_cache(maxsize=None)
def align_input():
    sizes = fat_sizes(NS, special=list(enumerate(ALIGN_SIZES)))
    assert list(sizes[:16]) == ALIGN_SIZES
    x = bucketed(sizes, seed=62)
    return x, oracle_sort(x, 8)


@pytest.mark.parametrize("offset", [0, 4, 8, 12])
def test_every_alignment(offset):
    """Sixteen tiny buckets first, whose starts and ends fall on every 4-word phase of the tile's alignment; the
    output 0, 4, 8 and 12 bytes past a 16-B boundary (over the four, starts and ends take every residue mod 8
    words); the words around the output keep their fill."""
    x, want = align_input()
    starts = np.concatenate([[0], np.cumsum(ALIGN_SIZES)])
    assert {int(v) % 4 for v in starts[:-1]} == {0, 1, 2, 3} and {int(v) % 4 for v in starts[1:]} == {0, 1, 2, 3}
    assert {(int(v) + k) % 8 for v in starts[:-1] for k in range(4)} == set(range(8))
    assert {(int(v) + k) % 8 for v in starts[1:] for k in range(4)} == set(range(8))
    n, fill, lead = x.size, 0x5A5A5A5A, 32 + offset // 4
    big = torch.full((n + 64,), fill, dtype=torch.int32, device="cuda")
    out = big[lead:lead + n]
    assert out.data_ptr() % 16 == offset
    assert np.array_equal(sorted_hybrid(x, out=out), want)
    assert int((big[:lead] != fill).sum()) == 0 and int((big[lead + n:] != fill).sum()) == 0


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_ordered_low_halves(order):
    """Low halves ascending (descending) with position inside every bucket, the buckets interleaved: pass 1 sees
    runs of ~55 keys with one high byte, whole waves of one digit, which rank through rank_add's aggregated
    branch into packed ranks."""
    sizes = fat_sizes(NS)
    rng = np.random.default_rng(63)
    top = np.repeat(np.arange(65536, dtype=np.uint32), sizes)
    rng.shuffle(top)
    by_bucket = np.argsort(top, kind="stable")  # positions of bucket 0's keys in input order, then bucket 1's, ...
    first = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes)
    within = np.arange(top.size, dtype=np.int64) - first
    low = (within * 65536 // np.repeat(sizes, sizes)).astype(np.uint32)
    if order == "descending":
        low = np.uint32(65535) - low
    x = np.empty(top.size, dtype=np.uint32)
    x[by_bucket] = (top[by_bucket] << np.uint32(16)) | low
    assert np.array_equal(bucket_sizes(x), sizes) and sizes.max() <= CAP
    b = int(np.flatnonzero(sizes)[3])
    seq = (x[(x >> np.uint32(16)) == b] & np.uint32(0xFFFF)).astype(np.int64)
    assert np.all(np.diff(seq) >= 0) if order == "ascending" else np.all(np.diff(seq) <= 0)
    assert np.array_equal(sorted_hybrid(x), oracle_sort(x, 8))


def test_kernel_info():
    """The bucket kernel as built: no scratch, an LDS footprint that leaves room for a second workgroup, and two
    workgroups resident per CU (a later change that spills or loses the second workgroup fails here)."""
    info = rs.hybrid_kernel_info()
    assert info["threads"] in (768, 1024) and CAP % info["threads"] == 0, info
    assert info["scratch_bytes"] == 0, info
    assert 0 < info["lds_bytes"] <= 80 * 1024, info
    assert info["resident_per_cu"] == 2, info
