"""CPU-side checks of the segmented sort's C ABI: argument validation before any HIP call, the no-ops, the
host entry's offset check, the workspace formula's bounds and the reported LDS capacities (no kernel launches)."""
import ctypes

import numpy as np
import pytest

from _rs import gpu_available, rs

P = ctypes.c_void_p


def test_device_entry_validates_before_touching_the_gpu():
    lib = rs._lib()
    seg = lib.rsort_u32_segmented_device
    big = 1 << 30
    # bad n
    assert seg(None, None, None, None, -1, None, 1, None, 0, None) == 3
    assert seg(None, None, None, None, 1 << 32, None, 1, None, 0, None) == 3
    # negative (or too many) segments
    assert seg(P(256), None, P(512), None, 10, P(1024), -1, P(2048), big, None) == 1
    assert seg(P(256), None, P(512), None, 10, P(1024), 1 << 31, P(2048), big, None) == 1
    # exactly one of the two value pointers
    assert seg(P(256), P(768), P(512), None, 10, P(1024), 2, P(2048), big, None) == 1
    assert seg(P(256), None, P(512), P(768), 10, P(1024), 2, P(2048), big, None) == 1
    # n == 0 and num_segments == 0 are no-ops that need no buffers
    assert seg(None, None, None, None, 0, None, 5, None, 0, None) == 0
    assert seg(None, None, None, None, 10, None, 0, None, 0, None) == 0
    # NULL data with work to do: keys in, keys out, offsets, workspace
    assert seg(None, None, P(512), None, 10, P(1024), 2, P(2048), big, None) == 1
    assert seg(P(256), None, None, None, 10, P(1024), 2, P(2048), big, None) == 1
    assert seg(P(256), None, P(512), None, 10, None, 2, P(2048), big, None) == 1
    assert seg(P(256), None, P(512), None, 10, P(1024), 2, None, big, None) == 1
    # misaligned pointers, each in turn
    assert seg(P(258), None, P(512), None, 10, P(1024), 2, P(2048), big, None) == 4
    assert seg(P(256), None, P(513), None, 10, P(1024), 2, P(2048), big, None) == 4
    assert seg(P(256), None, P(512), None, 10, P(1026), 2, P(2048), big, None) == 4
    assert seg(P(256), None, P(512), None, 10, P(1024), 2, P(2049), big, None) == 4
    assert seg(P(256), P(770), P(512), P(1280), 10, P(1024), 2, P(2048), big, None) == 4
    assert seg(P(256), P(768), P(512), P(1283), 10, P(1024), 2, P(2048), big, None) == 4
    # workspace too small (one byte short), keys and pairs
    for pairs in (0, 1):
        need = lib.rsort_segmented_workspace_size(10, 2, pairs)
        v = (P(768), P(1280)) if pairs else (None, None)
        assert seg(P(256), v[0], P(512), v[1], 10, P(1024), 2, P(2048), need - 1, None) == 7


def test_check_entry_validates():
    lib = rs._lib()
    f = ctypes.c_int(77)
    cc = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    assert lib.rsort_segmented_check(0, 0, 0, None, ctypes.byref(f), cc, None) == 0
    assert f.value == 0 and list(cc) == [0, 0, 0, 0]
    assert lib.rsort_segmented_check(10, 2, 0, None, None, None, None) == 1
    assert lib.rsort_segmented_check(10, 2, 0, None, ctypes.byref(f), None, None) == 1
    assert lib.rsort_segmented_check(-1, 2, 0, P(256), ctypes.byref(f), None, None) == 3
    assert lib.rsort_segmented_check(10, -2, 0, P(256), ctypes.byref(f), None, None) == 1


def _host(keys, off, out, vals=None, vals_out=None, n=None, nseg=None):
    lib = rs._lib()
    off = np.ascontiguousarray(off, dtype=np.uint32)
    return lib.rsort_u32_segmented(keys.ctypes.data if keys is not None else None,
                                   vals.ctypes.data if vals is not None else None,
                                   out.ctypes.data if out is not None else None,
                                   vals_out.ctypes.data if vals_out is not None else None,
                                   keys.size if n is None else n, off.ctypes.data if off.size else None,
                                   off.size - 1 if nseg is None else nseg)


def test_host_entry_validates():
    x = np.arange(100, dtype=np.uint32)[::-1].copy()
    y = np.zeros_like(x)
    good = [0, 10, 10, 100]
    assert _host(x, good, y, n=-1) == 3
    assert _host(x, good, y, n=1 << 32) == 3
    assert _host(x, good, y, nseg=-1) == 1
    assert _host(x, good, y, vals=x) == 1  # one of the two value pointers
    assert _host(x, good, y, vals_out=y) == 1
    assert _host(x, good, y, n=0) == 0  # no-ops
    assert _host(x, good, y, nseg=0) == 0
    assert rs._lib().rsort_u32_segmented(None, None, None, None, 0, None, 0) == 0
    assert rs._lib().rsort_u32_segmented(None, None, None, None, 10, None, 3) == 1
    # bad offsets: found on the host, before the device is touched (so also without one)
    assert _host(x, [0, 20, 10, 100], y) == 1  # decreasing
    assert _host(x, [0, 10, 101], y) == 1      # beyond n
    assert _host(x, [101, 101], y) == 1
    assert not y.any()
    with pytest.raises(rs.RSortError) as e:
        rs.sortSegmentsByDevice(x, [0, 50, 40], y)
    assert e.value.status == 1
    with pytest.raises(TypeError):
        rs.sortSegmentsByDevice(x.astype(np.int64), good, y)
    with pytest.raises(ValueError):
        rs.sortSegmentsByDevice(x, good, y, vals=x)


def test_host_entry_has_no_cpu_fallback():
    """Without a GPU the host entry must FAIL (RSORT_ERR_NODEV) for valid input and leave the output alone."""
    if gpu_available():
        pytest.skip("GPU present")
    x = np.arange(100, dtype=np.uint32)[::-1].copy()
    y = np.zeros_like(x)
    assert _host(x, [0, 10, 10, 100], y) == 8
    v = np.zeros_like(x)
    assert _host(x, [0, 10, 10, 100], y, vals=x, vals_out=v) == 8
    with pytest.raises(rs.RSortError) as e:
        rs.sortSegmentsByDevice(x, [3, 50, 97], y)
    assert e.value.status == 8
    assert not y.any() and not v.any()


@pytest.mark.parametrize("pairs", [False, True])
def test_workspace_size(pairs):
    sizes = [0, 1, 63, 1000, 1 << 20, (1 << 24) + 3, (1 << 32) - 1]
    segs = [0, 1, 2, 1000, 1 << 20, (1 << 31) - 1]
    tab = [[rs.segmented_workspace_size(n, s, pairs) for s in segs] for n in sizes]
    for i, n in enumerate(sizes):
        for j, s in enumerate(segs):
            assert tab[i][j] >= 4 * n * (2 if pairs else 1) + 4 * s, (n, s)
            if i:
                assert tab[i][j] >= tab[i - 1][j]
            if j:
                assert tab[i][j] >= tab[i][j - 1]
    # the header's formula
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    assert rs.segmented_workspace_size(1000, 7, pairs) == r(4000) * (2 if pairs else 1) + 4 * r(28) + 256
    assert rs.segmented_workspace_size(-1, 7, pairs) == 0
    assert rs.segmented_workspace_size(10, -1, pairs) == 0


def test_capacities():
    ck = rs.segmented_capacity(False)
    cp = rs.segmented_capacity(True)
    for cs, cl in (ck, cp):
        assert cs > 0 and cs % 64 == 0 and cl % 64 == 0
        assert cs <= cl
    assert ck[1] >= 16384
    assert cp[1] >= 8192
    assert rs._lib().rsort_segmented_capacity(0, None, None) == 1


def test_grid_entries_validate():
    lib = rs._lib()
    g = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert lib.rsort_segmented_grids(10, 2, 0, None) == 1
    assert lib.rsort_segmented_grids(-1, 2, 0, g) == 3 and list(g) == [0, 0, 0, 0]
    assert lib.rsort_segmented_grids(1 << 32, 2, 0, g) == 3
    assert lib.rsort_segmented_grids(10, -1, 0, g) == 1
    assert lib.rsort_segmented_grids(10, 1 << 31, 1, g) == 1
    # nothing to sort: no kernel is launched, and no device is needed to say so
    for n, s in ((0, 5), (10, 0)):
        g[:] = [7, 7, 7, 7]
        assert lib.rsort_segmented_grids(n, s, 0, g) == 0 and list(g) == [0, 0, 0, 0]
    if not gpu_available():
        assert lib.rsort_segmented_grids(1000, 3, 0, g) == 8  # the occupancy is a device's
    # the limit: 0 by default, the previous value comes back, a negative one is refused and changes nothing
    assert lib.rsort_set_segmented_grid_limit(-1) == -1
    assert lib.rsort_set_segmented_grid_limit(3) == 0
    assert lib.rsort_set_segmented_grid_limit(-5) == -1
    assert lib.rsort_set_segmented_grid_limit(0) == 3
    with rs.segmented_grid_limit(2):
        with rs.segmented_grid_limit(1):
            assert lib.rsort_set_segmented_grid_limit(1) == 1
        assert lib.rsort_set_segmented_grid_limit(2) == 2
    assert lib.rsort_set_segmented_grid_limit(0) == 0
    with pytest.raises(rs.RSortError):
        with rs.segmented_grid_limit(-2):
            pass
    assert lib.rsort_set_segmented_grid_limit(0) == 0


def test_python_constants():
    assert rs.CHECK_OFFSETS == 4 and rs.CHECK_RANK_ORDER == 2
    assert rs.SEG_CLASSES == ("small", "lds", "tiles", "rejected")
