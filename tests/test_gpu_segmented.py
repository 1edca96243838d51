"""GPU: the segmented sort (rsort_u32_segmented_device and its Python wrappers). Every segment of the output is
compared bit-exactly with the oracle applied to that segment alone (oracle_sort / oracle_sort_pairs, one call
per non-empty segment); pair values are arange(n), so any instability shows. The small and lds capacities cS, cL
come from rs.segmented_capacity(pairs), and the class counts rsort_segmented_check returns prove which kernels
ran. Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import oracle_sort, oracle_sort_pairs, uniform_keys, zipf_keys

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF


def _lengths(pairs):
    cS, cL = rs.segmented_capacity(pairs)
    return [1, 2, 3, 0, 63, 64, 65, 127, 128, 129, 255, 256, 257, cS - 1, cS, cS + 1, 0, 0, cL - 1, cL, cL + 1,
            2 * cL + 3, 3 * cL + 17]


def _offsets(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def _classes(lengths, pairs):
    cS, cL = rs.segmented_capacity(pairs)
    ln = np.asarray(lengths)
    return {"small": int(((ln > 0) & (ln <= cS)).sum()), "lds": int(((ln > cS) & (ln <= cL)).sum()),
            "tiles": int((ln > cL).sum()), "rejected": 0}


def _expected(x, v, off, base_k=None, base_v=None):
    """Per-segment oracle result laid over base_k / base_v (what the output held before; default: zeros)."""
    ek = np.zeros_like(x) if base_k is None else base_k.copy()
    ev = None if v is None else (np.zeros_like(v) if base_v is None else base_v.copy())
    for b, e in zip(off[:-1], off[1:]):
        if e <= b:
            continue
        if v is None:
            ek[b:e] = oracle_sort(x[b:e], 8)
        else:
            ek[b:e], ev[b:e] = oracle_sort_pairs(x[b:e], v[b:e], 8)
    return ek, ev


def _run(x, v, off, out=None, vout=None, ws=None, n=None, in_place=False):
    """One device call; returns (keys out, values out, flags, class counts, workspace)."""
    d_in = rs.from_numpy_u32(x)
    dv_in = rs.from_numpy_u32(v) if v is not None else None
    if in_place:
        d_out, dv_out = d_in, dv_in
    else:
        d_out = out if out is not None else torch.zeros(x.size, dtype=torch.int32, device="cuda")
        dv_out = None if v is None else (vout if vout is not None else torch.zeros(x.size, dtype=torch.int32,
                                                                                 device="cuda"))
    _, ws = rs.segmented_sort_device(d_in, d_out, off, vals_in=dv_in, vals_out=dv_out, ws=ws, n=n)
    nn = x.size if n is None else n
    flags, cc = rs.segmented_check(nn, len(off) - 1, v is not None, ws)
    return rs.to_numpy_u32(d_out), (rs.to_numpy_u32(dv_out) if v is not None else None), flags, cc, ws


@functools.lru_cache(maxsize=None)
def _case1(pairs):
    """The boundary lengths over uniform keys, with the oracle's result (computed once, never modified)."""
    lengths = _lengths(pairs)
    off = _offsets(lengths)
    n = int(off[-1])
    x = uniform_keys(n, seed=4242)
    v = np.arange(n, dtype=np.uint32) if pairs else None
    ek, ev = _expected(x, v, off)
    for a in (ek, ev, off):  # (x and v go through torch.from_numpy, which wants writable arrays; nobody writes them)
        if a is not None:
            a.setflags(write=False)
    return lengths, off, x, v, ek, ev


@pytest.mark.parametrize("pairs", [False, True])
def test_boundaries(pairs):
    lengths, off, x, v, ek, ev = _case1(pairs)
    assert sorted(set(int(o) % 4 for o in off[:-1])) == [0, 1, 2, 3]
    want = _classes(lengths, pairs)
    assert min(want["small"], want["lds"], want["tiles"]) > 0
    ko, vo, flags, cc, _ = _run(x, v, off)
    assert flags == 0 and cc == want, (flags, cc, want)
    assert np.array_equal(ko, ek)
    if pairs:
        assert np.array_equal(vo, ev)
    # the same into outputs that are only 4-byte aligned
    kb = torch.zeros(x.size + 1, dtype=torch.int32, device="cuda")
    vb = torch.zeros(x.size + 1, dtype=torch.int32, device="cuda")
    assert kb[1:].data_ptr() % 16 == 4
    ko, vo, flags, cc, _ = _run(x, v, off, out=kb[1:], vout=vb[1:] if pairs else None)
    assert flags == 0 and cc == want
    assert np.array_equal(ko, ek)
    if pairs:
        assert np.array_equal(vo, ev)
    assert int(kb[0]) == 0 and int(vb[0]) == 0


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("kind", ["equal", "low8", "high8", "mod3"])
def test_degenerate_digits(kind, pairs):
    lengths = _lengths(pairs)
    off = _offsets(lengths)
    n = int(off[-1])
    u = uniform_keys(n, seed=99)
    x = {"equal": np.full(n, 0x12345678, np.uint32), "low8": u & np.uint32(0xFF), "high8": u << np.uint32(24),
         "mod3": u % np.uint32(3)}[kind]
    v = np.arange(n, dtype=np.uint32) if pairs else None
    ek, ev = _expected(x, v, off)
    ko, vo, flags, cc, _ = _run(x, v, off)
    assert flags == 0 and cc == _classes(lengths, pairs)
    assert np.array_equal(ko, ek)
    if pairs:
        assert np.array_equal(vo, ev)


@functools.lru_cache(maxsize=None)
def _case3():
    lengths = np.random.default_rng(7).integers(0, 41, size=20000)
    lengths[100:140] = 0  # (runs of empty segments, besides the scattered ones)
    lengths[19990:] = 0
    off = _offsets(lengths)
    n = int(off[-1])
    x = zipf_keys(n, seed=31)
    v = np.arange(n, dtype=np.uint32)
    ek, ev = _expected(x, v, off)
    for a in (ek, ev, off):  # (x and v go through torch.from_numpy, which wants writable arrays; nobody writes them)
        a.setflags(write=False)
    return lengths, off, x, v, ek, ev


@pytest.mark.parametrize("pairs", [False, True])
def test_many_tiny_segments(pairs):
    lengths, off, x, v, ek, ev = _case3()
    ko, vo, flags, cc, _ = _run(x, v if pairs else None, off)
    assert flags == 0
    assert cc == {"small": int((lengths > 0).sum()), "lds": 0, "tiles": 0, "rejected": 0}
    assert np.array_equal(ko, ek)  # (a stable pair sort orders the keys as the key sort does)
    if pairs:
        assert np.array_equal(vo, ev)


@pytest.mark.parametrize("pairs", [False, True])
def test_in_place(pairs):
    cS, cL = rs.segmented_capacity(pairs)
    lengths = [cS, cL, cL + 5, 7]
    off = _offsets(lengths)
    n = int(off[-1])
    x = uniform_keys(n, seed=5)
    v = np.arange(n, dtype=np.uint32) if pairs else None
    ek, ev = _expected(x, v, off)
    ko, vo, flags, cc, _ = _run(x, v, off, in_place=True)
    assert flags == 0 and cc == _classes(lengths, pairs)
    assert np.array_equal(ko, ek)
    if pairs:
        assert np.array_equal(vo, ev)


@pytest.mark.parametrize("pairs", [False, True])
def test_uncovered_elements_are_not_written(pairs):
    cS, cL = rs.segmented_capacity(pairs)
    lengths = [3, cS + 1, 0, cL + 9, 130]
    off = _offsets(lengths, start=5)
    n = int(off[-1]) + 7
    x = uniform_keys(n, seed=6)
    v = np.arange(n, dtype=np.uint32) if pairs else None
    fill = np.full(n, FILL, np.uint32)
    ek, ev = _expected(x, v, off, base_k=fill, base_v=fill)
    ko, vo, flags, cc, _ = _run(x, v, off, out=rs.from_numpy_u32(fill), vout=rs.from_numpy_u32(fill) if pairs else None)
    assert flags == 0 and cc == _classes(lengths, pairs)
    assert np.array_equal(ko, ek)
    assert (ko[:5] == FILL).all() and (ko[n - 7:] == FILL).all()
    if pairs:
        assert np.array_equal(vo, ev)
        assert (vo[:5] == FILL).all() and (vo[n - 7:] == FILL).all()


@pytest.mark.parametrize("pairs", [False, True])
def test_rejected_offsets(pairs):
    # the tensors hold n_alloc keys and the call is told n = n_alloc - 4096: even an access through a rejected
    # pair of offsets would stay inside the allocations
    n_alloc = 12288
    n = n_alloc - 4096
    # nine good segments [1000, 2800), a decreasing pair (2800 -> 5), a good segment [5, 900), a pair beyond n
    off = np.array([1000 + 200 * i for i in range(10)] + [5, 900, n + 10], dtype=np.int64)
    good = [(int(b), int(e)) for b, e in zip(off[:-1], off[1:]) if b <= e <= n]
    assert len(good) == 10 and len(off) - 1 == 12
    x = uniform_keys(n_alloc, seed=8)
    v = np.arange(n_alloc, dtype=np.uint32) if pairs else None
    fill = np.full(n_alloc, FILL, np.uint32)
    goff = np.array(sorted(set(sum(good, ()))), dtype=np.int64)  # 5, 900 | 1000 .. 2800: [900, 1000) stays uncovered
    ek, ev = _expected(x, v, np.array([5, 900]), base_k=fill, base_v=fill)
    ek, ev = _expected(x, v, goff[2:], base_k=ek, base_v=ev)
    ko, vo, flags, cc, ws = _run(x, v, off, out=rs.from_numpy_u32(fill), vout=rs.from_numpy_u32(fill) if pairs else None,
                                 n=n)
    assert flags == rs.CHECK_OFFSETS
    assert cc["rejected"] == 2 and cc["small"] == 10 and cc["lds"] == 0 and cc["tiles"] == 0
    assert np.array_equal(ko, ek)  # the good segments sorted, everything else as prefilled
    assert (ko[:5] == FILL).all() and (ko[900:1000] == FILL).all() and (ko[2800:] == FILL).all()
    if pairs:
        assert np.array_equal(vo, ev)
        assert (vo[2800:] == FILL).all()
    # the next call in the same workspace, with good offsets, is clean
    off2 = np.array([0, 700, 700, n], dtype=np.int64)
    assert rs.segmented_workspace_size(n, 3, pairs) <= ws.numel()
    ek2, ev2 = _expected(x[:n], None if v is None else v[:n], off2)
    ko, vo, flags, cc, _ = _run(x, v, off2, ws=ws, n=n)
    assert flags == 0 and cc["rejected"] == 0
    assert np.array_equal(ko[:n], ek2)
    if pairs:
        assert np.array_equal(vo[:n], ev2)


def test_rank_check():
    cS, cL = rs.segmented_capacity(True)
    lengths = [cS, cL, 2 * cL]
    off = _offsets(lengths)
    n = int(off[-1])
    x = uniform_keys(n, seed=12)
    v = np.arange(n, dtype=np.uint32)
    ek, ev = _expected(x, v, off)
    assert rs.lane_order_probe() == 1 and rs.get_rank_algo() == rs.RANK_MATCH
    ko, vo, flags, cc, ws = _run(x, v, off)
    assert flags == 0 and cc == _classes(lengths, True)
    assert np.array_equal(ko, ek) and np.array_equal(vo, ev)
    with rs.rank_fault():
        ko, vo, flags, _, _ = _run(x, v, off, ws=ws)
        assert flags & rs.CHECK_RANK_ORDER
        assert not np.array_equal(vo, ev)
        # every class on its own catches it
        for b, e in zip(off[:-1], off[1:]):
            _, _, f1, c1, _ = _run(x[b:e], v[b:e], np.array([0, e - b]))
            assert f1 & rs.CHECK_RANK_ORDER, c1
        with pytest.raises(rs.RSortError) as err:
            rs.sortSegmentsByDevice(x, off, np.zeros_like(x), vals=v, vals_out=np.zeros_like(v))
        assert err.value.status == 11
    ko, vo, flags, _, _ = _run(x, v, off, ws=ws)
    assert flags == 0
    assert np.array_equal(ko, ek) and np.array_equal(vo, ev)


@pytest.mark.parametrize("algo", ["RANK_BALLOT", "RANK_SPLIT"])
def test_ballot_ranking(algo):
    lengths, off, x, v, ek, ev = _case1(True)
    with rs.rank_algo(getattr(rs, algo)):
        ko, vo, flags, cc, ws = _run(x, v, off)
        assert flags == 0 and cc == _classes(lengths, True)
        assert np.array_equal(ko, ek) and np.array_equal(vo, ev)
        with rs.rank_fault():  # no lane-ordered adds on this path: the hook has nothing to break
            ko, vo, flags, _, _ = _run(x, v, off, ws=ws)
        assert flags == 0
        assert np.array_equal(ko, ek) and np.array_equal(vo, ev)


@pytest.mark.parametrize("pairs", [False, True])
def test_sort_rows(pairs):
    rows, cols = 257, 1000
    x = uniform_keys(rows * cols, seed=77)
    v = np.arange(rows * cols, dtype=np.uint32) if pairs else None
    off = _offsets([cols] * rows)
    ek, ev = _expected(x, v, off)
    d_in = rs.from_numpy_u32(x).view(rows, cols)
    d_out = torch.zeros_like(d_in)
    dv_in = rs.from_numpy_u32(v).view(rows, cols) if pairs else None
    dv_out = torch.zeros_like(d_in) if pairs else None
    _, ws = rs.sort_rows(d_in, d_out, dv_in, dv_out)
    flags, cc = rs.segmented_check(rows * cols, rows, pairs, ws)
    assert flags == 0 and cc == {"small": rows, "lds": 0, "tiles": 0, "rejected": 0}
    assert np.array_equal(rs.to_numpy_u32(d_out).ravel(), ek)
    if pairs:
        assert np.array_equal(rs.to_numpy_u32(dv_out).ravel(), ev)
    with pytest.raises(ValueError):
        rs.sort_rows(d_in.t(), d_out)


def test_vendor_comparator_agrees():
    lengths, off, x, v, ek, ev = _case1(False)
    d_in = rs.from_numpy_u32(x)
    d_out = torch.zeros(x.size, dtype=torch.int32, device="cuda")
    rs.vendor_segmented_sort_device(d_in, d_out, off)
    torch.cuda.synchronize()
    ko, _, flags, _, _ = _run(x, None, off)
    assert flags == 0
    assert np.array_equal(rs.to_numpy_u32(d_out), ko)


@pytest.mark.parametrize("pairs", [False, True])
def test_host_entry(pairs):
    lengths, off, x, v, ek, ev = _case3()
    out = np.zeros_like(x)
    vout = np.zeros_like(v) if pairs else None
    rs.sortSegmentsByDevice(x, off, out, vals=v if pairs else None, vals_out=vout)
    assert np.array_equal(out, ek)
    if pairs:
        assert np.array_equal(vout, ev)
    # offsets that leave both ends uncovered: the host entry leaves them alone
    off2 = np.array([11, 50, 50, 2000, x.size - 3], dtype=np.int64)
    out = np.full(x.size, FILL, np.uint32)
    rs.sortSegmentsByDevice(x, off2, out)
    want, _ = _expected(x, None, off2, base_k=np.full(x.size, FILL, np.uint32))
    assert np.array_equal(out, want)
