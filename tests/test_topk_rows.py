"""CPU-side checks of the row-wise top-k's C ABI: argument validation before any HIP call, in the documented order,
the no-ops, the workspace formula of include/rsort.h, the grid-limit hook and the Python wrapper's own checks (no
kernel launches)."""
import ctypes

import numpy as np
import pytest
import torch

from _rs import gpu_available, rs
from _util import TOPK_ROWS_CLASS_COLS, byte_row, digit_boundaries, select_exit_level

P = ctypes.c_void_p
BIG = 1 << 40
SIZE, ARG, ALIGN, WORKSPACE, NODEV = 3, 1, 4, 7, 8


def test_device_entry_validates_before_touching_the_gpu():
    f = rs._lib().rsort_u32_topk_rows_device
    kin, vin, kout, vout, ws = P(256), P(512), P(1024), P(2048), P(4096)
    # sizes first: rows, cols, their product (before k, flags and pointers are looked at)
    assert f(None, None, -1, 10, 0, 0, None, None, None, 0, None) == SIZE
    assert f(None, None, 10, -1, 0, 0, None, None, None, 0, None) == SIZE
    assert f(None, None, 1 << 31, 1, 1, 0, None, None, None, 0, None) == SIZE
    assert f(None, None, 1, 1 << 32, 1, 0, None, None, None, 0, None) == SIZE
    assert f(None, None, 1 << 16, 1 << 16, 1, 0, None, None, None, 0, None) == SIZE  # rows * cols = 2^32
    assert f(None, None, 1 << 30, 4, 99, 99, None, None, None, 0, None) == SIZE      # (2^32 again; k, flags bad too)
    assert f(None, None, (1 << 31) - 1, 3, -1, 8, None, None, None, 0, None) == SIZE
    # k out of range (before the flags)
    assert f(kin, None, 4, 10, -1, 8, kout, None, ws, BIG, None) == ARG
    assert f(kin, None, 4, 10, 11, 0, kout, None, ws, BIG, None) == ARG
    assert f(kin, None, 0, 10, 11, 0, kout, None, ws, BIG, None) == ARG  # (also where there is nothing to do)
    assert f(kin, None, 4, 0, 1, 0, kout, None, ws, BIG, None) == ARG
    # unknown flag bits
    assert f(kin, None, 4, 10, 3, 8, kout, None, ws, BIG, None) == ARG
    assert f(kin, None, 4, 10, 3, -1, kout, None, ws, BIG, None) == ARG
    assert f(None, None, 4, 10, 0, 8, None, None, None, 0, None) == ARG
    # exactly one of the two value pointers
    assert f(kin, vin, 4, 10, 3, 0, kout, None, ws, BIG, None) == ARG
    assert f(kin, None, 4, 10, 3, 0, kout, vout, ws, BIG, None) == ARG
    # INDICES with values in, or without a values output
    assert f(kin, vin, 4, 10, 3, rs.TOPK_INDICES, kout, vout, ws, BIG, None) == ARG
    assert f(kin, None, 4, 10, 3, rs.TOPK_INDICES, kout, None, ws, BIG, None) == ARG
    # NULL data with work to do: keys in, keys out, workspace
    assert f(None, None, 4, 10, 3, 0, kout, None, ws, BIG, None) == ARG
    assert f(kin, None, 4, 10, 3, 0, None, None, ws, BIG, None) == ARG
    assert f(kin, None, 4, 10, 3, 0, kout, None, None, BIG, None) == ARG
    # misaligned pointers, each in turn (NULL checks come first, the workspace size last)
    assert f(P(258), None, 4, 10, 3, 0, kout, None, ws, 0, None) == ALIGN
    assert f(kin, None, 4, 10, 3, 0, P(1025), None, ws, 0, None) == ALIGN
    assert f(kin, None, 4, 10, 3, 0, kout, None, P(4099), 0, None) == ALIGN
    assert f(kin, P(514), 4, 10, 3, 0, kout, vout, ws, 0, None) == ALIGN
    assert f(kin, vin, 4, 10, 3, 0, kout, P(2051), ws, 0, None) == ALIGN
    assert f(kin, None, 4, 10, 3, rs.TOPK_INDICES, kout, P(2050), ws, 0, None) == ALIGN
    # workspace one byte short: keys / values / indices, sorted and unsorted, one shape per kernel class
    for rows, cols, k in [(4, 10, 3), (4, 10, 10), (3, 700, 65), (2, 5000, 2000), (2, 40001, 20000), (1000, 64, 8)]:
        for un in (0, rs.TOPK_UNSORTED):
            need = rs.topk_rows_workspace_size(rows, cols, k, False)
            assert need > 0
            assert f(kin, None, rows, cols, k, un, kout, None, ws, need - 1, None) == WORKSPACE
            need = rs.topk_rows_workspace_size(rows, cols, k, True)
            assert f(kin, vin, rows, cols, k, un | 1, kout, vout, ws, need - 1, None) == WORKSPACE
            assert f(kin, None, rows, cols, k, un | rs.TOPK_INDICES, kout, vout, ws, need - 1, None) == WORKSPACE


def test_noops_need_no_buffers():
    lib = rs._lib()
    for flags in range(8):
        for rows, cols, k in [(0, 10, 3), (0, 0, 0), (5, 0, 0), (5, 10, 0), (0, 10, 10), ((1 << 31) - 1, 0, 0)]:
            assert lib.rsort_u32_topk_rows_device(None, None, rows, cols, k, flags, None, None, None, 0, None) == 0
            assert lib.rsort_u32_topk_rows(None, None, rows, cols, k, flags, None, None) == 0


def test_host_entry_validates_and_has_no_cpu_fallback():
    lib = rs._lib()
    host = lib.rsort_u32_topk_rows
    x = np.arange(100, dtype=np.uint32)[::-1].copy().reshape(10, 10)
    y = np.zeros((10, 5), np.uint32)
    v = np.zeros((10, 5), np.uint32)
    xp, yp, vp = x.ctypes.data, y.ctypes.data, v.ctypes.data
    assert host(xp, None, -1, 10, 0, 0, yp, None) == SIZE
    assert host(xp, None, 1 << 31, 1, 0, 0, yp, None) == SIZE
    assert host(xp, None, 1 << 20, 1 << 12, 5, 0, yp, None) == SIZE
    assert host(xp, None, 10, 10, 11, 0, yp, None) == ARG
    assert host(xp, None, 10, 10, -1, 0, yp, None) == ARG
    assert host(xp, None, 10, 10, 5, 16, yp, None) == ARG
    assert host(xp, None, 10, 10, 5, -1, yp, None) == ARG
    assert host(xp, xp, 10, 10, 5, 0, yp, None) == ARG
    assert host(xp, None, 10, 10, 5, 0, yp, vp) == ARG
    assert host(xp, xp, 10, 10, 5, rs.TOPK_INDICES, yp, vp) == ARG
    assert host(xp, None, 10, 10, 5, rs.TOPK_INDICES, yp, None) == ARG
    assert host(None, None, 10, 10, 5, 0, yp, None) == ARG
    assert host(xp, None, 10, 10, 5, 0, None, None) == ARG
    k0, v0 = rs.topkRowsByDevice(x, 0, indices=True)
    assert k0.shape == (10, 0) and v0.shape == (10, 0)
    k0, v0 = rs.topkRowsByDevice(np.zeros((0, 7), np.uint32), 3)
    assert k0.shape == (0, 3) and v0 is None
    if not gpu_available():
        assert host(xp, None, 10, 10, 5, 0, yp, None) == NODEV
        with pytest.raises(rs.RSortError) as e:
            rs.topkRowsByDevice(x, 5, largest=True, indices=True)
        assert e.value.status == NODEV
        assert not y.any()


def _formula(rows, cols, k, pairs):
    """The byte formula of include/rsort.h, term by term."""
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return 256 + r(4 * (rows + 1)) + rs.segmented_workspace_size(rows * k, rows, pairs) + 256


@pytest.mark.parametrize("pairs", [False, True])
def test_workspace_size(pairs):
    size = rs.topk_rows_workspace_size
    shapes = [(0, 0), (1, 1), (1, 63), (3, 64), (37, 257), (1000, 1000), (1 << 20, 64), (1 << 16, 1 << 10),
              (1 << 12, 1 << 14), (8, 1 << 23), (1, (1 << 32) - 1), ((1 << 31) - 1, 2), (65535, 65537)]
    for rows, cols in shapes:
        last = -1
        for k in sorted({0, min(cols, 1), min(cols, 64), cols // 3, max(cols - 1, 0), cols}):
            w = size(rows, cols, k, pairs)
            assert w == _formula(rows, cols, k, pairs), (rows, cols, k)
            assert w >= last, (rows, cols, k)  # monotone in k
            last = w
    for k in (0, 1, 64):
        by_rows = [size(rows, 64, k, pairs) for rows in (0, 1, 3, 1000, 1 << 20, 1 << 25)]
        assert by_rows == sorted(by_rows), k  # monotone in rows
        by_cols = [size(1000, cols, k, pairs) for cols in (64, 65, 1000, 1 << 14, 1 << 22)]
        assert by_cols == sorted(by_cols), k  # monotone in cols (at a fixed k the bytes do not depend on cols)
    assert size(1000, 64, 8, True) >= size(1000, 64, 8, False)
    # 0 for invalid arguments
    assert size(-1, 10, 0, pairs) == 0
    assert size(10, -1, 0, pairs) == 0
    assert size(1 << 31, 1, 0, pairs) == 0
    assert size(1 << 16, 1 << 16, 1, pairs) == 0
    assert size(10, 10, 11, pairs) == 0
    assert size(10, 10, -1, pairs) == 0


def test_grid_entries_validate():
    lib = rs._lib()
    g = (ctypes.c_int * 2)(7, 7)
    assert lib.rsort_topk_rows_grids(10, 10, 2, 0, None) == ARG
    assert lib.rsort_topk_rows_grids(-1, 10, 0, 0, g) == SIZE and list(g) == [0, 0]
    g[:] = [7, 7]
    assert lib.rsort_topk_rows_grids(1 << 31, 1, 0, 0, g) == SIZE and list(g) == [0, 0]
    assert lib.rsort_topk_rows_grids(1 << 16, 1 << 16, 0, 0, g) == SIZE
    assert lib.rsort_topk_rows_grids(10, 10, 11, 0, g) == ARG
    for rows, cols, k in [(0, 10, 3), (5, 0, 0), (5, 10, 0)]:  # nothing to do: no device needed
        g[:] = [7, 7]
        assert lib.rsort_topk_rows_grids(rows, cols, k, 1, g) == 0 and list(g) == [0, 0]
        assert rs.topk_rows_grids(rows, cols, k) == {"workgroups": 0, "kernel": 0}
    if not gpu_available():
        assert lib.rsort_topk_rows_grids(1000, 64, 3, 0, g) == NODEV  # the occupancy is a device's
        with pytest.raises(rs.RSortError) as e:
            rs.topk_rows_grids(1000, 64, 3)
        assert e.value.status == NODEV


def test_grid_limit_hook():
    lib = rs._lib()
    assert lib.rsort_set_topk_rows_grid_limit(-1) == -1
    assert lib.rsort_set_topk_rows_grid_limit(3) == 0
    assert lib.rsort_set_topk_rows_grid_limit(-5) == -1  # rejected: nothing changes
    assert lib.rsort_set_topk_rows_grid_limit(0) == 3
    with rs.topk_rows_grid_limit(2):
        with rs.topk_rows_grid_limit(1):
            assert lib.rsort_set_topk_rows_grid_limit(1) == 1
        assert lib.rsort_set_topk_rows_grid_limit(2) == 2
    assert lib.rsort_set_topk_rows_grid_limit(0) == 0
    with pytest.raises(rs.RSortError):
        with rs.topk_rows_grid_limit(-2):
            pass
    assert lib.rsort_set_topk_rows_grid_limit(0) == 0
    # its own switch: the single-array top-k's hook is another one
    with rs.topk_rows_grid_limit(5):
        assert lib.rsort_set_topk_grid_limit(0) == 0


def test_check_entry_validates():
    lib = rs._lib()
    fl = ctypes.c_int(9)
    r = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    assert lib.rsort_topk_rows_check(10, 10, 3, 0, P(256), None, r, None) == ARG
    assert lib.rsort_topk_rows_check(-1, 10, 0, 0, P(256), ctypes.byref(fl), r, None) == SIZE
    assert fl.value == 0 and list(r) == [0] * 4
    assert lib.rsort_topk_rows_check(1 << 16, 1 << 16, 0, 0, P(256), ctypes.byref(fl), r, None) == SIZE
    assert lib.rsort_topk_rows_check(10, 10, 11, 0, P(256), ctypes.byref(fl), r, None) == ARG
    assert lib.rsort_topk_rows_check(10, 10, 3, 0, None, ctypes.byref(fl), r, None) == ARG
    for rows, cols, k in [(0, 10, 3), (5, 0, 0), (5, 10, 0)]:  # a no-op call: all zero, no workspace, no device
        fl.value = 9
        r[:] = [9] * 4
        assert lib.rsort_topk_rows_check(rows, cols, k, 1, None, ctypes.byref(fl), r, None) == 0
        assert fl.value == 0 and list(r) == [0] * 4
        assert lib.rsort_topk_rows_check(rows, cols, k, 0, None, ctypes.byref(fl), None, None) == 0
        assert rs.topk_rows_check(rows, cols, k, False, None, stream=_NoStream()) == (0, [0, 0, 0, 0])


def test_python_mirror_raises_on_a_check_status(monkeypatch):
    """rs.topkRowsByDevice raises RSortError(11) when rsort_u32_topk_rows returns RSORT_ERR_CHECK (no device: the
    entry is a stub here; tests/test_gpu_check_entries.py has the library return it)."""
    real, calls = rs._lib(), []

    class Fake:
        def __getattr__(self, attr):
            if attr != "rsort_u32_topk_rows":
                return getattr(real, attr)
            return lambda *args: calls.append(args) or rs.RSORT_ERR_CHECK

    monkeypatch.setattr(rs, "_LIB", Fake())
    with pytest.raises(rs.RSortError) as e:
        rs.topkRowsByDevice(np.arange(12, dtype=np.uint32).reshape(3, 4), 2, largest=True)
    assert e.value.status == 11 == rs.RSORT_ERR_CHECK and len(calls) == 1


def test_python_wrapper_rejects_bad_tensors():
    x = torch.zeros((4, 10), dtype=torch.int32)
    with pytest.raises(TypeError):
        rs.topk_rows(x.to(torch.int64), 3)
    with pytest.raises(TypeError):
        rs.topk_rows(np.zeros((4, 10), np.int32), 3)
    with pytest.raises(TypeError):
        rs.topk_rows(x, 3, vals_2d=x.to(torch.float32))
    with pytest.raises(ValueError):
        rs.topk_rows(x.reshape(-1), 3)              # 1-D
    with pytest.raises(ValueError):
        rs.topk_rows(x.t(), 3)                      # not contiguous
    with pytest.raises(ValueError):
        rs.topk_rows(x[:, ::2], 3)
    with pytest.raises(ValueError):
        rs.topk_rows(x, 3, vals_2d=torch.zeros((4, 9), dtype=torch.int32))
    with pytest.raises(ValueError):
        rs.topk_rows(x, 3, vals_2d=x, indices=True)
    with pytest.raises(ValueError):
        rs.topk_rows(x, 3, out=(torch.zeros((4, 4), dtype=torch.int32), None))
    with pytest.raises(ValueError):
        rs.topk_rows(x, 3, indices=True, out=(torch.zeros((4, 3), dtype=torch.int32), torch.zeros((3, 4), dtype=torch.int32)))
    with pytest.raises(ValueError):
        rs.topk_rows(x, 3, out=(torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 3), dtype=torch.int32)))
    with pytest.raises(TypeError):
        rs.topkRowsByDevice(np.zeros((4, 10), np.int64), 3)
    with pytest.raises(TypeError):
        rs.topkRowsByDevice(np.zeros((4, 10), np.uint32)[:, ::2], 3)
    with pytest.raises(ValueError):
        rs.topkRowsByDevice(np.zeros(40, np.uint32), 3)
    with pytest.raises(ValueError):
        rs.topkRowsByDevice(np.zeros((4, 10), np.uint32), 3, vals_2d=np.zeros((4, 9), np.uint32))
    # k out of range is the library's answer (before any HIP call: host tensors never reach a kernel)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    for k in (-1, 11):
        with pytest.raises(rs.RSortError) as e:
            rs.topk_rows(x, k, ws=ws, stream=_NoStream())
        assert e.value.status == ARG


class _NoStream:
    """Stands in for a torch stream where there may be no GPU: the validation paths never use it."""
    cuda_stream = None


def test_python_constants():
    assert rs.TOPK_ROWS_KERNELS == ("wave", "small", "lds", "stream")


# ------------------------------------------------------------------------------ the select's exits, by construction
@pytest.mark.parametrize("cls", sorted(TOPK_ROWS_CLASS_COLS))
def test_byte_rows_reach_every_exit_of_the_select(cls):
    """What keeps tests/test_gpu_topk_rows.py::test_select_exit_levels from being vacuous, with no GPU: for a
    byte_row of level L (tests/_util.py), in both directions, the host model of the four-level loop ends at level L
    for k at every cumulative digit count but the last, runs through all four levels one entry later, and ends at
    level 0 for k = cols; over the levels that is every exit, 0 to 3, and the run through (4)."""
    cols = TOPK_ROWS_CLASS_COLS[cls]
    assert rs.TOPK_ROWS_KERNELS[cls] == ("wave" if cols <= 256 else "small" if cols <= 1024 else
                                         "lds" if cols <= 16384 else "stream")
    for m in (np.uint32(0), np.uint32(0xFFFFFFFF)):
        seen = set()
        for level in range(4):
            for seed in (40, 41, 42):
                x = byte_row(cols, level, seed) ^ m
                varies = [b for b in range(4) if np.unique((x >> np.uint32(24 - 8 * b)) & np.uint32(255)).size > 1]
                assert varies == [level] and np.unique(x).size == 16
                bounds = digit_boundaries(x, level)
                assert bounds.size == 16 and bounds[-1] == cols and int(np.diff(bounds).min()) >= 2
                for b in bounds[:-1]:
                    assert select_exit_level(x, int(b)) == level, (cols, level, seed, int(b))
                    assert select_exit_level(x, int(b) + 1) == 4, (cols, level, seed, int(b))
                assert select_exit_level(x, cols) == 0
                near = int(bounds[np.argmin(np.abs(bounds - cols // 3))])  # the ks of the GPU test
                seen |= {select_exit_level(x, k) for k in (near, near + 1, cols)}
        assert seen == {0, 1, 2, 3, 4}, (cols, int(m), seen)


def test_select_exit_level_on_plain_rows():
    """The model itself on rows whose exits are known by hand."""
    one = np.full(50, 0x01020304, np.uint32)
    assert all(select_exit_level(one, k) == (0 if k == 50 else 4) for k in (1, 7, 49, 50))
    x = np.array([0x10000000, 0x20000000, 0x20000001, 0x30000500, 0x30000600, 0x30000601], np.uint32)
    # k = 1: the top digit 0x10 holds one entry and one is wanted; k = 2: digit 0x20 holds two, one wanted: down to the
    # last byte, where digit 0 holds exactly the one; k = 3: both of 0x20; k = 4: 0x30 -> byte 2 (5 | 6, 6): digit 5
    # holds one; k = 5: digit 6 holds two, one wanted -> the last byte: digit 0 holds one; k = 6: all of 0x30
    assert [select_exit_level(x, k) for k in range(1, 7)] == [0, 3, 0, 2, 3, 0]
