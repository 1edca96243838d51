"""GPU: the segmented sort where a workgroup (or a wave of rs_seg_wave) sorts MORE THAN ONE segment -- the second
and later iterations of the four kernels' list loops -- and the inputs the partial-slot scheme rests on.

A call's grids are min(the most segments of the kind, CUs x resident workgroups x 4) (rs.segmented_grids reports
them); the lists of tests/test_gpu_segmented.py are all shorter than that, so there every workgroup sorts one
segment. Here the lists are longer than their grids: small inputs under the test hook rs.segmented_grid_limit,
and inputs with more segments than the product grid without it. A later iteration depends on what the one before
left behind: the LDS tile of a longer segment under a shorter one, the counter rows and digit bases, the output
alignment (ak / av) changing between segments, the barrier between the store of one segment and the loads of
the next.

Everything is bit-exact, values are arange(n) so any instability shows, flags == 0, and the class counts say
which kernels ran. Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import uniform_keys
from test_gpu_segmented import FILL, _case1, _classes, _expected, _offsets, _run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF  # the key a partial slot's missing lanes hold (rsort_segmented.hip, "Partial slots")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _assert_sorted(got, want_flags_cc, ek, ev, pairs):
    ko, vo, flags, cc, _ = got
    assert flags == 0 and cc == want_flags_cc, (flags, cc, want_flags_cc)
    assert np.array_equal(ko, ek)
    if pairs:
        assert np.array_equal(vo, ev)


# ------------------------------------------------------------------------------ 1. strides under the limit
def _stride_lengths():
    """Seven to nine segments of every kernel kind, the extremes of each kind next to each other."""
    cS, cL = rs.segmented_capacity(True)
    assert rs.segmented_capacity(False) == (cS, cL) and (cS, cL) == (1024, 16384)
    wave = [256, 1, 255, 64, 65, 63, 200, 2, 129]
    small = [cS, 257, cS - 1, 300, 1000, 258, 640]
    lds = [cL, cS + 1, cL - 1, cS + 2, 5000, 12289, 2000]
    tiles = [cL + 1, 3 * 8192, 2 * 8192 + 1, 40000, 24577, 32768 + 5, 16400]
    return wave, small, lds, tiles


@functools.lru_cache(maxsize=None)
def _stride_case(seed):
    """All kinds in one offsets list, shuffled, with empty segments between; the per-segment oracle's result for
    pairs (whose keys are the keys-only result), computed once per seed and never modified."""
    rng = np.random.default_rng(seed)
    lengths = [ln for kind in _stride_lengths() for ln in kind]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    with_empty = []
    for ln in lengths:
        with_empty.append(ln)
        with_empty.extend([0] * int(rng.integers(0, 3)))
    lengths = [0] + with_empty
    off = _offsets(lengths)
    n = int(off[-1])
    x = uniform_keys(n, seed=1000 + seed)
    v = np.arange(n, dtype=np.uint32)
    ek, ev = _expected(x, v, off)
    _frozen(ek, ev, off)
    return lengths, off, x, v, ek, ev


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("algo", ["RANK_MATCH", "RANK_BALLOT"])
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("limit", [1, 3])
def test_stride_under_grid_limit(limit, pairs, algo, seed):
    lengths, off, x, v, ek, ev = _stride_case(seed)
    want = _classes(lengths, pairs)
    assert want == {"small": 16, "lds": 7, "tiles": 7, "rejected": 0}
    assert sorted(set(int(o) % 4 for o, ln in zip(off[:-1], lengths) if ln)) == [0, 1, 2, 3]
    with rs.rank_algo(getattr(rs, algo)), rs.segmented_grid_limit(limit):
        grids = rs.segmented_grids(x.size, len(lengths), pairs)
        assert grids == {"wave": limit, "small": limit, "lds": limit, "tiles": limit}
        _assert_sorted(_run(x, v if pairs else None, off), want, ek, ev, pairs)
    assert rs.segmented_grids(x.size, len(lengths), pairs)["small"] > limit  # the hook is off again


@pytest.mark.parametrize("pairs", [False, True])
def test_stride_in_place_and_misaligned(pairs):
    lengths, off, x, v, ek, ev = _stride_case(1)
    want = _classes(lengths, pairs)
    n = x.size
    with rs.segmented_grid_limit(1):
        assert set(rs.segmented_grids(n, len(lengths), pairs).values()) == {1}
        _assert_sorted(_run(x, v if pairs else None, off, in_place=True), want, ek, ev, pairs)
        # outputs 4 bytes past a 16-B boundary, a guard word on each side
        kb = torch.full((n + 2,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
        vb = torch.full((n + 2,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
        assert kb[1:n + 1].data_ptr() % 16 == 4 and vb[1:n + 1].data_ptr() % 16 == 4
        _assert_sorted(_run(x, v if pairs else None, off, out=kb[1:n + 1], vout=vb[1:n + 1] if pairs else None),
                       want, ek, ev, pairs)
        guards = rs.to_numpy_u32(torch.stack([kb[0], kb[n + 1], vb[0], vb[n + 1]]))
        assert (guards == FILL).all()
        if not pairs:
            assert bool((vb == FILL - (1 << 32)).all())


# ------------------------------------------------------------------------------ 2. more segments than the product grid
def _device_reference(d_keys, seg_ids):
    """Stable sort by (segment, key) from torch on the device: (keys, original positions), as uint32 numpy."""
    k64 = d_keys.to(torch.int64) & 0xFFFFFFFF
    by_key = torch.sort(k64, stable=True).indices
    by_seg = torch.sort(seg_ids[by_key], stable=True).indices
    perm = by_key[by_seg]
    return (k64[perm].cpu().numpy().astype(np.uint32), perm.cpu().numpy().astype(np.uint32))


@pytest.mark.parametrize("pairs", [False, True])
def test_more_segments_than_the_product_grid(pairs):
    """No limit set: the wave, small and lds lists each hold grid x 3/2 + 37 entries (the wave kernel sorts four
    segments per workgroup, so four times as many segments), of short lengths so the input stays ~10^7 keys.
    The multi-tile kernel strides only under the limit (test_stride_under_grid_limit): its product grid is
    CUs x 4 workgroups (one resident per CU: 1024 on 256 CUs) of segments longer than 16384 keys, so a list
    longer than it needs more than 1.6 x 10^7 keys -- more than 3 x 10^7 where two workgroups fit a CU."""
    cS, cL = rs.segmented_capacity(pairs)
    cap = rs.segmented_grids((1 << 32) - 1, (1 << 31) - 1, pairs)  # every kind at its product grid
    assert min(cap.values()) >= 64
    rng = np.random.default_rng(11)
    counts = {"wave": 4 * (cap["wave"] * 3 // 2 + 37), "small": cap["small"] * 3 // 2 + 37,
              "lds": cap["lds"] * 3 // 2 + 37}
    lengths = np.concatenate([rng.integers(1, 257, size=counts["wave"]), rng.integers(257, 321, size=counts["small"]),
                              rng.integers(cS + 1, 1101, size=counts["lds"])])
    lengths = lengths[rng.permutation(lengths.size)]
    off = _offsets(lengths)
    n, nseg = int(off[-1]), lengths.size
    grids = rs.segmented_grids(n, nseg, pairs)
    assert grids["wave"] == cap["wave"] and grids["small"] == cap["small"] and grids["lds"] == cap["lds"]
    assert counts["wave"] > 4 * grids["wave"] and counts["small"] > grids["small"] and counts["lds"] > grids["lds"]
    x = uniform_keys(n, seed=2024)
    d_in = rs.from_numpy_u32(x)
    d_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    dv_in = torch.arange(n, dtype=torch.int32, device="cuda") if pairs else None
    dv_out = torch.zeros(n, dtype=torch.int32, device="cuda") if pairs else None
    _, ws = rs.segmented_sort_device(d_in, d_out, off, vals_in=dv_in, vals_out=dv_out)
    flags, cc = rs.segmented_check(n, nseg, pairs, ws)
    assert flags == 0
    assert cc == {"small": counts["wave"] + counts["small"], "lds": counts["lds"], "tiles": 0, "rejected": 0}
    seg_ids = torch.repeat_interleave(torch.arange(nseg, device="cuda"), torch.from_numpy(lengths).to("cuda"))
    ek, ev = _device_reference(d_in, seg_ids)
    assert np.array_equal(rs.to_numpy_u32(d_out), ek)
    if pairs:
        assert np.array_equal(rs.to_numpy_u32(dv_out), ev)


@pytest.mark.parametrize("pairs", [False, True])
def test_more_equal_rows_than_the_product_grid(pairs):
    rows, cols = 1 << 17, 64
    n = rows * cols
    grids = rs.segmented_grids(n, rows, pairs)
    assert rows > 4 * grids["wave"] > 0
    d_in = rs.from_numpy_u32(uniform_keys(n, seed=64)).view(rows, cols)
    d_out = torch.zeros_like(d_in)
    dv_in = torch.arange(n, dtype=torch.int32, device="cuda").view(rows, cols) if pairs else None
    dv_out = torch.zeros_like(d_in) if pairs else None
    _, ws = rs.sort_rows(d_in, d_out, dv_in, dv_out)
    flags, cc = rs.segmented_check(n, rows, pairs, ws)
    assert flags == 0 and cc == {"small": rows, "lds": 0, "tiles": 0, "rejected": 0}
    k64 = d_in.to(torch.int64) & 0xFFFFFFFF
    s = torch.sort(k64, dim=1, stable=True)
    assert torch.equal(d_out.to(torch.int64) & 0xFFFFFFFF, s.values)
    if pairs:
        assert torch.equal(dv_out.to(torch.int64), s.indices + torch.arange(rows, device="cuda")[:, None] * cols)


# ------------------------------------------------------------------------------ 3. keys that equal the pad
def _pad_lengths(pairs):
    cS, cL = rs.segmented_capacity(pairs)
    return [1, 63, 64, 65, 255, 257, 1000, 1025, cL - 1, cL + 1, 2 * cL + 3]


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("kind", ["all_pad", "mix"])
def test_pad_valued_keys(kind, pairs):
    """Real keys 0xFFFFFFFF (and their neighbours in every digit) beside the pads of the partial slots: a pad
    must still land behind every real key, whose values must keep their input order."""
    lengths = _pad_lengths(pairs)
    off = _offsets(lengths)
    n = int(off[-1])
    if kind == "all_pad":
        x = np.full(n, PAD, np.uint32)
    else:
        r = uniform_keys(n, seed=255)
        pick = (r >> np.uint32(8)) % np.uint32(5)
        x = np.choose(pick, [np.full(n, PAD, np.uint32), np.full(n, 0xFFFFFFFE, np.uint32),
                             np.uint32(0xFFFFFF00) | (r & np.uint32(0xFF)), np.full(n, 0x00FFFFFF, np.uint32),
                             np.full(n, 0xFF, np.uint32)]).astype(np.uint32)
        assert (x == PAD).sum() > n // 8
    v = np.arange(n, dtype=np.uint32) if pairs else None
    ek, ev = _expected(x, v, off)
    _assert_sorted(_run(x, v, off), _classes(lengths, pairs), ek, ev, pairs)
    with rs.segmented_grid_limit(1):  # ... and over the tile a longer segment left behind
        _assert_sorted(_run(x, v, off), _classes(lengths, pairs), ek, ev, pairs)


# ------------------------------------------------------------------------------ 4. keys-only ballot kernels
@pytest.mark.parametrize("algo", ["RANK_BALLOT", "RANK_SPLIT"])
def test_ballot_ranking_keys_only(algo):
    lengths, off, x, v, ek, ev = _case1(False)
    want = _classes(lengths, False)
    with rs.rank_algo(getattr(rs, algo)):
        _assert_sorted(_run(x, None, off), want, ek, None, False)
        kb = torch.zeros(x.size + 1, dtype=torch.int32, device="cuda")
        assert kb[1:].data_ptr() % 16 == 4
        _assert_sorted(_run(x, None, off, out=kb[1:]), want, ek, None, False)
        assert int(kb[0]) == 0


# ------------------------------------------------------------------------------ 5. offsets at and above 2^31
@pytest.mark.parametrize("pairs", [False, True])
def test_offsets_at_and_above_2_31(pairs):
    """n = 2^31 + 2^17 (rsort_u32_segmented_device takes n < 2^32): one segment of every kind, the first from
    2^31 - 100 (it crosses 2^31), the last ending at n. The buffers are allocated and never initialised; only
    the segments' region and a guard band before it are written."""
    cS, cL = rs.segmented_capacity(pairs)
    n = (1 << 31) + (1 << 17)
    lo = (1 << 31) - 100
    lengths = [200, 777, 12345]
    lengths.append(n - lo - sum(lengths))
    assert lengths[3] > cL and cS < lengths[2] <= cL
    off = _offsets(lengths, start=lo)
    assert int(off[-1]) == n and off[1] > (1 << 31)
    m, guard = n - lo, 4096
    x = uniform_keys(m, seed=31)
    v = np.arange(m, dtype=np.uint32) if pairs else None
    ek, ev = _expected(x, v, off - lo)
    bufs = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4 if pairs else 2)]
    d_in, d_out = bufs[0], bufs[1]
    dv_in, dv_out = (bufs[2], bufs[3]) if pairs else (None, None)
    d_in[lo:] = rs.from_numpy_u32(x)
    if pairs:
        dv_in[lo:] = rs.from_numpy_u32(v)
    for b in bufs:
        b[lo - guard:lo] = FILL - (1 << 32)
    for b in bufs[1::2]:
        b[lo:] = 0
    _, ws = rs.segmented_sort_device(d_in, d_out, off, vals_in=dv_in, vals_out=dv_out)
    flags, cc = rs.segmented_check(n, len(lengths), pairs, ws)
    assert flags == 0 and cc == {"small": 2, "lds": 1, "tiles": 1, "rejected": 0}
    assert np.array_equal(rs.to_numpy_u32(d_out[lo:]), ek)
    if pairs:
        assert np.array_equal(rs.to_numpy_u32(dv_out[lo:]), ev)
    for b in bufs:
        assert (rs.to_numpy_u32(b[lo - guard:lo]) == FILL).all()
    assert np.array_equal(rs.to_numpy_u32(d_in[lo:]), x)
