"""GPU tests of the row-wise top-k (include/rsort.h "row-wise top-k").

The expected output everywhere is the project's own oracle, per row: with m = 0xFFFFFFFF for the k largest, else 0,
idx = oracle_sort_pairs(row ^ m, arange(cols), 8)[1][:k] -- the stable order, so equal keys keep their column order
and the lowest columns are taken at the threshold -- and the row's result is (row[idx], vals[idx]), or idx itself with
indices. Every element is compared bit for bit; UNSORTED results after sorting both sides' (key, value) pairs per row
on the host. After every call rs.topk_rows_check must be clean: flags 0, no row with a count other than k, and the
kernel class rs.topk_rows_grids names. Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import (TOPK_ROWS_CLASS_COLS, byte_row, digit_boundaries, oracle_sort_pairs, select_exit_level, uniform_keys,
                   zipf_keys)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = ("keys", "vals", "indices")
WAVE, SMALL, LDS, STREAM = range(4)
CLASS_COLS = TOPK_ROWS_CLASS_COLS  # {WAVE: 100, SMALL: 600, LDS: 5000, STREAM: 20000}: one row length inside each class
KNOWN_SCATTER_KERNELS = 144  # len(rs.scatter_kernels_known()) of the parent commit: this feature adds none
SENTINEL = 0x5A5A5A5A
PAD = 64


def cls_of(cols):
    return WAVE if cols <= 256 else SMALL if cols <= 1024 else LDS if cols <= 16384 else STREAM


def dev(a):
    return rs.from_numpy_u32(a if a.flags.writeable else a.copy())


def ks_for(cols):
    return sorted({min(max(k, 1), cols) for k in (1, 2, 64, 65, cols // 3, cols - 1, cols)})


def _row(name, cols, r):
    if name == "uniform":  # a different seed per row
        return uniform_keys(cols, seed=1000 + 7919 * r)
    if name == "equal":
        return np.full(cols, 0xDEADBEEF, np.uint32)
    if name == "ends":  # only 0 and 0xFFFFFFFF
        return np.where(uniform_keys(cols, seed=5 + r) & 1, np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32)
    if name == "low10":  # below 2^10: every level but the last two keeps every candidate
        return uniform_keys(cols, seed=9 + r) >> np.uint32(22)
    if name == "top8":  # differ only in the top 8 bits
        return (uniform_keys(cols, seed=11 + r) & np.uint32(0xFF000000)) | np.uint32(0x00ABCDEF)
    if name == "sorted":
        return np.sort(uniform_keys(cols, seed=13 + r))
    if name == "reverse":
        return np.sort(uniform_keys(cols, seed=13 + r))[::-1]
    if name == "zipf":  # few ranks: long runs of equal keys in every row
        return zipf_keys(cols, seed=17 + r, ranks=32)
    if name == "stripes":  # rows of all 0 and all 0xFFFFFFFF in turn
        return np.full(cols, 0xFFFFFFFF if r & 1 else 0, np.uint32)
    if name == "steps":  # every row's keys lie in a band of its own, so the rows' k-th keys all differ
        return (uniform_keys(cols, seed=21 + r) >> np.uint32(8)) + np.uint32((r * 37 % 251) << 24)
    if name in ("byte0", "byte1", "byte2", "byte3"):  # only the byte of one select level varies (tests/_util.py)
        return byte_row(cols, int(name[4]), seed=40 + r)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def matrix(name, rows, cols):
    x = np.ascontiguousarray(np.stack([_row(name, cols, r) for r in range(rows)]), dtype=np.uint32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def values(rows, cols):
    v = uniform_keys(rows * cols, seed=0xBEEF).reshape(rows, cols)  # (never the positions)
    v.setflags(write=False)
    return v


def row_order(x, largest):
    """Every row's stable ascending order of x ^ m, from the oracle."""
    m = np.uint32(0xFFFFFFFF if largest else 0)
    cols = x.shape[1]
    pos = np.arange(cols, dtype=np.uint32)
    idx = np.stack([oracle_sort_pairs(row ^ m, pos, 8)[1] for row in x]) if x.shape[0] else np.empty((0, cols), np.uint32)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def order(name, rows, cols, largest):
    """Computed once per input and direction, shared by every test that needs it, never changed."""
    return row_order(matrix(name, rows, cols), largest)


def expected_from(x, v, idx, k, mode):
    idx = idx[:, :k].astype(np.int64)
    wk = np.take_along_axis(x, idx, 1)
    wv = None if mode == "keys" else idx.astype(np.uint32) if mode == "indices" else np.take_along_axis(v, idx, 1)
    return wk, wv


def expected(name, rows, cols, k, largest, mode):
    return expected_from(matrix(name, rows, cols), values(rows, cols), order(name, rows, cols, largest), k, mode)


def assert_result(ko, vo, want, what, sorted=True):
    wk, wv = want
    gk = rs.to_numpy_u32(ko)
    gv = None if vo is None else rs.to_numpy_u32(vo)
    assert (gv is None) == (wv is None), what
    assert gk.shape == wk.shape, what
    if not sorted:  # the same entries of every row in any order: compare as sorted (key, value) pairs per row
        if wv is None:
            gk, wk = np.sort(gk, axis=1), np.sort(wk, axis=1)
        else:
            g = (gk.astype(np.uint64) << np.uint64(32)) | gv
            w = (wk.astype(np.uint64) << np.uint64(32)) | wv
            gk, wk, gv, wv = np.sort(g, axis=1), np.sort(w, axis=1), None, None
    bad = np.flatnonzero((gk != wk).any(axis=1))
    assert bad.size == 0, (what, "rows", bad[:8])
    if wv is not None:
        bad = np.flatnonzero((gv != wv).any(axis=1))
        assert bad.size == 0, (what, "value rows", bad[:8])


def assert_clean(rows, cols, k, pairs, ws, what, stream=None):
    flags, rep = rs.topk_rows_check(rows, cols, k, pairs, ws, stream)
    assert flags == 0 and rep[1] == 0, (what, flags, rep)
    g = rs.topk_rows_grids(rows, cols, k, pairs)
    assert rep[0] == g["kernel"] == cls_of(cols) and rep[2:] == [0, 0], (what, rep, g)


def call(d_x, k, largest, mode, d_v=None, sorted=True, ws=None, out=None, stream=None):
    return rs.topk_rows(d_x, k, largest=largest, vals_2d=d_v if mode == "vals" else None, indices=mode == "indices",
                        sorted=sorted, ws=ws, out=out, stream=stream)


def check_case(name, rows, cols, k, largest, mode, sorted=True, d_x=None, d_v=None, ws=None):
    d_x = dev(matrix(name, rows, cols)) if d_x is None else d_x
    d_v = dev(values(rows, cols)) if (d_v is None and mode == "vals") else d_v
    ko, vo, ws = call(d_x, k, largest, mode, d_v, sorted, ws=ws)
    what = (name, rows, cols, k, largest, mode, sorted)
    assert ko.shape == (rows, k)
    assert_result(ko, vo, expected(name, rows, cols, k, largest, mode), what, sorted)
    assert_clean(rows, cols, k, mode != "keys", ws, what)
    return ko, vo


# ------------------------------------------------------------------------------ class boundaries
BOUNDARY = ((1, 37), (2, 5), (63, 3), (64, 37), (65, 5), (255, 3), (256, 37), (257, 5), (1023, 3), (1024, 37),
            (1025, 5), (4097, 3), (16383, 1), (16384, 5), (16385, 3), (40001, 1))


@pytest.mark.parametrize("cols,rows", BOUNDARY)
def test_class_boundaries(cols, rows):
    d_x, d_v = dev(matrix("uniform", rows, cols)), dev(values(rows, cols))
    for k in ks_for(cols):
        for largest in (False, True):
            for mode in MODES:
                check_case("uniform", rows, cols, k, largest, mode, d_x=d_x, d_v=d_v)


@pytest.mark.parametrize("cols", (65, 257, 4097, 16385))
def test_unsorted(cols):
    rows = 5
    for k in ks_for(cols):
        for largest in (False, True):
            for mode in MODES:
                check_case("zipf", rows, cols, k, largest, mode, sorted=False)


# ------------------------------------------------------------------------------ ties and degenerate rows
@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
@pytest.mark.parametrize("name", ("equal", "ends", "low10", "top8", "sorted", "reverse"))
def test_ties_and_degenerate_rows(name, cls):
    cols, rows = CLASS_COLS[cls] + 1, 3
    x = matrix(name, rows, cols)
    zeros = int(np.count_nonzero(x[0] == 0))
    for largest in (False, True):  # (both: real 0xFFFFFFFF and real 0 meet whatever stands in the empty slots)
        for k in sorted(k for k in {1, 2, 65, cols // 3, zeros, zeros + 1, cols - zeros, cols - 1, cols} if 1 <= k <= cols):
            for mode in ("keys", "indices"):
                check_case(name, rows, cols, k, largest, mode)
        check_case(name, rows, cols, cols // 3, largest, "vals")
        check_case(name, rows, cols, cols // 2, largest, "vals", sorted=False)


@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_ties_zipf(cls):
    """k inside row 0's run of its most frequent key: some copies are taken, the lowest columns, in column order."""
    cols, rows = CLASS_COLS[cls], 3
    x = matrix("zipf", rows, cols)
    vals, counts = np.unique(x[0], return_counts=True)
    hot = vals[np.argmax(counts)]
    for largest in (False, True):
        o = order("zipf", rows, cols, largest)[0]
        run = np.flatnonzero(x[0][o] == hot)
        lo, hi = int(run[0]), int(run[-1]) + 1
        assert hi - lo == counts.max() and hi - lo >= 8
        for k in (lo + 1, lo + 2, (lo + hi) // 2, hi - 1):
            for mode in MODES:
                ko, _ = check_case("zipf", rows, cols, k, largest, mode)
                assert int(rs.to_numpy_u32(ko)[0, k - 1]) == int(hot)


# ------------------------------------------------------------------------------ rows do not leak
@pytest.mark.parametrize("cols", (65, 1027, 16387, 20001))
def test_rows_do_not_leak(cols):
    """Odd cols: every row starts at another 16-byte phase. A read or a write across a row's end changes a row."""
    rows = 7
    for name in ("stripes", "steps"):
        if name == "steps":
            kth = {int(matrix(name, rows, cols)[r][order(name, rows, cols, False)[r][cols // 3 - 1]]) for r in range(rows)}
            assert len(kth) == rows  # the rows' k-th keys all differ
        for largest in (False, True):
            for k in (1, cols // 3, cols - 1, cols):
                check_case(name, rows, cols, k, largest, "indices")
                check_case(name, rows, cols, k, largest, "vals", sorted=False)


# ------------------------------------------------------------------------------ nothing else is written
@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_nothing_else_is_written(cls):
    cols, rows = CLASS_COLS[cls] + 3, 5
    x, v = matrix("uniform", rows, cols), values(rows, cols)
    d_x, d_v = dev(x), dev(v)
    for k in (1, 65, cols):
        for largest, mode, sorted_ in ((False, "vals", True), (True, "indices", True), (True, "vals", False), (False, "keys", True)):
            bk = torch.full((2 * PAD + rows * k,), SENTINEL, dtype=torch.int32, device="cuda")
            bv = torch.full((2 * PAD + rows * k,), SENTINEL, dtype=torch.int32, device="cuda")
            out = (bk[PAD:PAD + rows * k].view(rows, k), None if mode == "keys" else bv[PAD:PAD + rows * k].view(rows, k))
            ko, vo, ws = call(d_x, k, largest, mode, d_v, sorted_, out=out)
            what = (cls, k, largest, mode, sorted_)
            assert_result(ko, vo, expected("uniform", rows, cols, k, largest, mode), what, sorted_)
            assert_clean(rows, cols, k, mode != "keys", ws, what)
            for b in (bk, bv):
                h = b.cpu().numpy()
                assert (h[:PAD] == SENTINEL).all() and (h[PAD + rows * k:] == SENTINEL).all(), what
            if mode == "keys":
                assert (bv.cpu().numpy() == SENTINEL).all(), what
            assert np.array_equal(rs.to_numpy_u32(d_x), x) and np.array_equal(rs.to_numpy_u32(d_v), v), what


# ------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("off", (1, 2, 3))
@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_alignment(cls, off):
    cols, rows = CLASS_COLS[cls] + 1, 3
    n = rows * cols
    x, v = matrix("uniform", rows, cols), values(rows, cols)
    bx = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    bv = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    assert bx.data_ptr() % 256 == 0 and bv.data_ptr() % 256 == 0
    d_x, d_v = bx[off:off + n].view(rows, cols), bv[off:off + n].view(rows, cols)
    d_x.copy_(dev(x))
    d_v.copy_(dev(v))
    for k in (65, cols // 3):
        for largest in (False, True):
            for mode in MODES:
                bo, bvo = rs.empty_u32(rows * k + 8), rs.empty_u32(rows * k + 8)
                assert bo.data_ptr() % 256 == 0 and bvo.data_ptr() % 256 == 0
                out = (bo[off:off + rows * k].view(rows, k), None if mode == "keys" else bvo[off:off + rows * k].view(rows, k))
                wsb = rs.topk_rows_workspace_size(rows, cols, k, mode != "keys")
                ws = rs.workspace(wsb + 16)[4 * off:4 * off + wsb]
                assert ws.data_ptr() % 256 == 4 * off and out[0].data_ptr() % 256 == 4 * off
                ko, vo, _ = call(d_x, k, largest, mode, d_v, ws=ws, out=out)
                what = (cls, off, k, largest, mode)
                assert_result(ko, vo, expected("uniform", rows, cols, k, largest, mode), what)
                assert_clean(rows, cols, k, mode != "keys", ws, what)


# ------------------------------------------------------------------------------ row striding
@pytest.mark.parametrize("limit", (1, 3))
@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_grid_limit(cls, limit):
    cols, rows = CLASS_COLS[cls], 9
    with rs.topk_rows_grid_limit(limit):
        assert rs.topk_rows_grids(rows, cols, 5, True) == {"workgroups": min(limit, 3 if cls == WAVE else 9), "kernel": cls}
        for largest in (False, True):
            for k in (1, 65, cols // 3):
                check_case("uniform", rows, cols, k, largest, "indices")
    assert rs.topk_rows_grids(rows, cols, 5, True)["workgroups"] == (3 if cls == WAVE else 9)


@pytest.mark.parametrize("cls,cols", ((WAVE, 8), (SMALL, 300)))
def test_more_rows_than_the_grid(cls, cols):
    """Without the hook: every workgroup (every wave of the wave class) takes a second row, some a third."""
    full = rs.topk_rows_grids(1 << 22, cols, 2, True)
    assert full["kernel"] == cls
    grid = full["workgroups"]  # CUs x resident workgroups x 4: rows no longer bound it
    rows = 4 * grid * 4 + 5 if cls == WAVE else grid + 5
    assert rs.topk_rows_grids(rows, cols, 2, True)["workgroups"] == grid
    x = np.ascontiguousarray((uniform_keys(rows * cols, seed=31) >> np.uint32(3)).reshape(rows, cols))
    d_x = dev(x)
    for largest, k in ((True, 2), (False, cols // 2)):
        idx = row_order(x, largest)
        ko, vo, ws = call(d_x, k, largest, "indices")
        assert_result(ko, vo, expected_from(x, None, idx, k, "indices"), (cls, rows, k, largest))
        assert_clean(rows, cols, k, True, ws, (cls, rows, k, largest))


# ------------------------------------------------------------------------------ workspace state
@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_workspace_state(cls):
    """The same call gives the same bytes and a clean check over a workspace of zeros, of 0xFF and of random bytes."""
    cols, rows, k = CLASS_COLS[cls], 5, 70
    d_x, d_v = dev(matrix("zipf", rows, cols)), dev(values(rows, cols))
    for largest, mode, sorted_ in ((False, "vals", True), (True, "indices", True), (True, "vals", False), (False, "keys", False)):
        pairs = mode != "keys"
        wsb = rs.topk_rows_workspace_size(rows, cols, k, pairs)
        want = expected("zipf", rows, cols, k, largest, mode)
        seen = set()
        for kind in ("zero", "ff", "random"):
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            if kind == "zero":
                ws.zero_()
            elif kind == "ff":
                ws.fill_(0xFF)
            else:
                ws.copy_(torch.from_numpy(uniform_keys((wsb + 3) // 4, seed=99).view(np.uint8)[:wsb].copy()))
            ko, vo, _ = call(d_x, k, largest, mode, d_v, sorted_, ws=ws)
            assert_result(ko, vo, want, (cls, largest, mode, sorted_, kind), sorted_)
            assert_clean(rows, cols, k, pairs, ws, (cls, kind))
            seen.add((rs.to_numpy_u32(ko).tobytes(), b"" if vo is None else rs.to_numpy_u32(vo).tobytes()))
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


@pytest.mark.parametrize("cls", (WAVE, LDS))
@pytest.mark.parametrize("largest,mode", ((True, "vals"), (False, "indices")))
def test_graph_replay(cls, largest, mode):
    cols, rows, k = CLASS_COLS[cls], 5, 33
    names = ("uniform", "low10", "zipf")
    src = {nm: dev(matrix(nm, rows, cols)) for nm in names}
    d_x, d_v = dev(matrix("steps", rows, cols)), dev(values(rows, cols))
    out = (torch.zeros((rows, k), dtype=torch.int32, device="cuda"), torch.zeros((rows, k), dtype=torch.int32, device="cuda"))
    ws = rs.workspace(rs.topk_rows_workspace_size(rows, cols, k, True))
    ws.fill_(0xA5)
    g, st = captured(lambda: call(d_x, k, largest, mode, d_v, ws=ws, out=out))
    with torch.cuda.stream(st):
        for nm in names:  # three replays, the input changed before each
            d_x.copy_(src[nm])
            out[0].zero_()
            out[1].zero_()
            g.replay()
            assert_clean(rows, cols, k, True, ws, nm, st)
            assert_result(out[0], out[1], expected(nm, rows, cols, k, largest, mode), (cls, nm))
        st.synchronize()


# ------------------------------------------------------------------------------ host entry
def test_host_entry():
    rows, cols = 37, 1000
    x, v = matrix("zipf", rows, cols), values(rows, cols)
    for k in (1, 100, cols):
        for largest in (False, True):
            ko, vo = rs.topkRowsByDevice(x, k, largest=largest)
            wk, _ = expected("zipf", rows, cols, k, largest, "keys")
            assert vo is None and np.array_equal(ko, wk)
            ko, vo = rs.topkRowsByDevice(x, k, largest=largest, indices=True)
            wk, wv = expected("zipf", rows, cols, k, largest, "indices")
            assert np.array_equal(ko, wk) and np.array_equal(vo, wv)
    ko, vo = rs.topkRowsByDevice(x, 100, largest=True, vals_2d=v)
    wk, wv = expected("zipf", rows, cols, 100, True, "vals")
    assert np.array_equal(ko, wk) and np.array_equal(vo, wv)


# ------------------------------------------------------------------------------ the finishing sort
@pytest.mark.parametrize("cols,k,seg_class", ((5000, 300, "small"), (5000, 2000, "lds"), (40001, 20000, "tiles")))
def test_finishing_sort_is_the_segmented_sort(cols, k, seg_class):
    """k in the segmented sort's small, lds and multi-tile classes (its wave class: every small k above)."""
    rows = 3
    small, lds = rs.segmented_capacity(True)
    assert {"small": 256 < k <= small, "lds": small < k <= lds, "tiles": k > lds}[seg_class]
    for largest, mode in ((False, "vals"), (True, "indices"), (True, "keys")):
        check_case("uniform", rows, cols, k, largest, mode)
    # the finishing sort's own workspace, behind the state words and the offsets: its counters name the class
    pairs = True
    ko, vo, ws = call(dev(matrix("uniform", rows, cols)), k, True, "indices")
    base = -ws.data_ptr() % 256 + 256 + (4 * (rows + 1) + 255) // 256 * 256
    flags, counts = rs.segmented_check(rows * k, rows, pairs, ws[base:])
    assert flags == 0 and counts[seg_class] == rows and sum(counts.values()) == rows, counts


# ------------------------------------------------------------------------------ every exit of the select
@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_select_exit_levels(cls):
    """The four-level loop leaves at the first level whose picked digit holds exactly what is wanted, and entries are
    then compared by the chosen upper bits alone. Rows in which only one level's byte varies (byte_row) put the exit
    where the test wants it: k at a digit boundary ends at that level, one more runs through all four, k = cols ends at
    level 0. The host model (select_exit_level) says so for every row and k before anything runs, and that the class
    sees every exit: 0, 1, 2, 3 and the run through (4)."""
    cols, rows = CLASS_COLS[cls], 3
    cases, seen, at_level_2 = [], set(), {}
    for level in range(4):
        name = "byte%d" % level
        x = matrix(name, rows, cols)
        for largest in (False, True):
            m = np.uint32(0xFFFFFFFF if largest else 0)
            bounds = digit_boundaries(x[0] ^ m, level)
            near = int(bounds[np.argmin(np.abs(bounds - cols // 3))])  # the digit boundary nearest cols // 3 of row 0
            for k, want in ((near, level), (near + 1, 4), (cols, 0)):
                exits = {select_exit_level(x[r] ^ m, k) for r in range(rows)}
                assert exits == {want}, (cls, level, largest, k, exits)
                seen |= exits
                cases.append((name, k, largest))
            if level == 2:
                at_level_2[largest] = near
    assert seen == {0, 1, 2, 3, 4}
    for name, k, largest in cases:
        for mode in ("keys", "indices"):
            check_case(name, rows, cols, k, largest, mode)
    for largest, k in at_level_2.items():  # the raw path writes x ^ m of entries compared by 16 bits only
        check_case("byte2", rows, cols, k, largest, "vals", sorted=False)


# ------------------------------------------------------------------------------ past 2^31
BASE_ROWS = 61
PIECE = 1 << 26
PAST_2_31 = (1 << 31) + (1 << 17)
FULLSIZE = {  # class: cols, rows, k, the calls (mode, largest, sorted)
    WAVE: (65, PAST_2_31 // 65 + 1, 3, (("indices", True, True), ("keys", False, False))),
    LDS: (5000, PAST_2_31 // 5000 + 1, 65, (("indices", False, True),)),
    SMALL: (1024, (1 << 21) + 4099, 1023, (("vals", False, True), ("indices", True, True))),
    STREAM: (20001, PAST_2_31 // 20001 + 1, 70, (("vals", False, True),)),
}


def periodic_rows(base, rows):
    """The rows x cols device matrix whose row r is base[r % 61] (base: 61 x cols on the device), built in pieces."""
    cols = base.shape[1]
    out = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
    step = max(1, PIECE // cols)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        out[r0:r1] = base.index_select(0, torch.arange(r0, r1, device="cuda") % BASE_ROWS)
    return out


@pytest.mark.parametrize("cls", (WAVE, SMALL, LDS, STREAM))
def test_rows_past_2_31(cls):
    """One shape per kernel whose last row starts at or above element 2^31 of the input (rows * cols < 2^32 is what
    the entry accepts): row r = base_rows[r % 61], so the oracle's answer for 61 rows is every row's. The small-class
    shape has k = 1023 of 1024 columns: its output, the i * k offsets and the finishing segmented sort pass 2^31
    too. Compared on the device, bit for bit, in pieces of rows; the call's check must be clean."""
    cols, rows, k, calls = FULLSIZE[cls]
    assert cls_of(cols) == cls and (rows - 1) * cols >= 1 << 31 and rows * cols < 1 << 32
    if cls == SMALL:
        assert (rows - 1) * k >= 1 << 31
    xb = np.ascontiguousarray(np.stack([_row(("zipf", "uniform", "steps")[r % 3], cols, r) for r in range(BASE_ROWS)]),
                              dtype=np.uint32)
    vb = uniform_keys(BASE_ROWS * cols, seed=0xBEEF).reshape(BASE_ROWS, cols)  # (never the positions)
    d_x = periodic_rows(dev(xb), rows)
    d_v = periodic_rows(dev(vb), rows) if any(mode == "vals" for mode, _, _ in calls) else None
    step = max(1, PIECE // k)
    for mode, largest, sorted_ in calls:
        what = (cls, mode, largest, sorted_)
        wk, wv = expected_from(xb, vb, row_order(xb, largest), k, mode)
        ko, vo, ws = call(d_x, k, largest, mode, d_v, sorted_)
        assert ko.shape == (rows, k) and (vo is None) == (wv is None), what
        assert_clean(rows, cols, k, mode != "keys", ws, what)
        del ws
        ek, ev = dev(wk), None if wv is None else dev(wv)
        if not sorted_:  # keys only: every row's entries in any order
            assert wv is None
            ek = torch.sort(ek.to(torch.int64) & 0xFFFFFFFF, dim=1).values
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            src = torch.arange(r0, r1, device="cuda") % BASE_ROWS
            got = ko[r0:r1] if sorted_ else torch.sort(ko[r0:r1].to(torch.int64) & 0xFFFFFFFF, dim=1).values
            bad = (got != ek.index_select(0, src)).any(dim=1)
            assert not bool(bad.any()), (what, "rows", (r0 + torch.nonzero(bad)[:8, 0]).tolist())
            if ev is not None:
                bad = (vo[r0:r1] != ev.index_select(0, src)).any(dim=1)
                assert not bool(bad.any()), (what, "value rows", (r0 + torch.nonzero(bad)[:8, 0]).tolist())
        del ko, vo


# ------------------------------------------------------------------------------ unchanged behaviour
def test_no_new_scatter_kernels():
    assert len(rs.scatter_kernels_known()) == KNOWN_SCATTER_KERNELS
