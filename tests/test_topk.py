"""CPU-side checks of the top-k selection's C ABI: argument validation before any HIP call, the no-ops, the
workspace formula of include/rsort.h, the route and grid-limit switches and the automatic limit (no kernel launches)."""
import ctypes

import numpy as np
import pytest
import torch

from _rs import gpu_available, rs
from _util import (PERIODIC_POSITION_TABLES, oracle_sort_pairs, periodic_topk_expected, periodic_topk_positions,
                   periodic_topk_report, periodic_topk_tables, uniform_keys)

P = ctypes.c_void_p
BIG = 1 << 40


def test_device_entry_validates_before_touching_the_gpu():
    topk = rs._lib().rsort_u32_topk_device
    kin, vin, kout, vout, ws = P(256), P(512), P(1024), P(2048), P(4096)
    # bad n
    assert topk(None, None, -1, 0, 0, None, None, None, 0, None) == 3
    assert topk(None, None, 1 << 32, 1, 0, None, None, None, 0, None) == 3
    # k out of range
    assert topk(kin, None, 10, -1, 0, kout, None, ws, BIG, None) == 1
    assert topk(kin, None, 10, 11, 0, kout, None, ws, BIG, None) == 1
    # unknown flag bits
    assert topk(kin, None, 10, 3, 8, kout, None, ws, BIG, None) == 1
    assert topk(kin, None, 10, 3, -1, kout, None, ws, BIG, None) == 1
    # exactly one of the two value pointers
    assert topk(kin, vin, 10, 3, 0, kout, None, ws, BIG, None) == 1
    assert topk(kin, None, 10, 3, 0, kout, vout, ws, BIG, None) == 1
    # INDICES with values in, or without a values output
    assert topk(kin, vin, 10, 3, rs.TOPK_INDICES, kout, vout, ws, BIG, None) == 1
    assert topk(kin, None, 10, 3, rs.TOPK_INDICES, kout, None, ws, BIG, None) == 1
    # k == 0 (and n == 0) is a no-op that needs no buffers, under every flag
    for flags in range(8):
        assert topk(None, None, 10, 0, flags, None, None, None, 0, None) == 0
        assert topk(None, None, 0, 0, flags, None, None, None, 0, None) == 0
    # NULL data with work to do: keys in, keys out, workspace
    assert topk(None, None, 10, 3, 0, kout, None, ws, BIG, None) == 1
    assert topk(kin, None, 10, 3, 0, None, None, ws, BIG, None) == 1
    assert topk(kin, None, 10, 3, 0, kout, None, None, BIG, None) == 1
    # misaligned pointers, each in turn
    assert topk(P(258), None, 10, 3, 0, kout, None, ws, BIG, None) == 4
    assert topk(kin, None, 10, 3, 0, P(1025), None, ws, BIG, None) == 4
    assert topk(kin, None, 10, 3, 0, kout, None, P(4099), BIG, None) == 4
    assert topk(kin, P(514), 10, 3, 0, kout, vout, ws, BIG, None) == 4
    assert topk(kin, vin, 10, 3, 0, kout, P(2051), ws, BIG, None) == 4
    assert topk(kin, None, 10, 3, rs.TOPK_INDICES, kout, P(2050), ws, BIG, None) == 4
    # workspace too small (one byte short), on each route, keys / values / indices
    for route in (rs.TOPK_AUTO, rs.TOPK_SELECT, rs.TOPK_SORT):
        with rs.topk_route(route):
            for k in (3, 10):
                need = rs.topk_workspace_size(10, k, False, route)
                assert topk(kin, None, 10, k, 0, kout, None, ws, need - 1, None) == 7
                need = rs.topk_workspace_size(10, k, True, route)
                assert topk(kin, vin, 10, k, 1, kout, vout, ws, need - 1, None) == 7
                assert topk(kin, None, 10, k, rs.TOPK_INDICES, kout, vout, ws, need - 1, None) == 7


def test_host_entry_validates_and_has_no_cpu_fallback():
    lib = rs._lib()
    x = np.arange(100, dtype=np.uint32)[::-1].copy()
    y = np.zeros(5, np.uint32)
    v = np.zeros(5, np.uint32)
    xp, yp, vp = x.ctypes.data, y.ctypes.data, v.ctypes.data
    assert lib.rsort_u32_topk(xp, None, -1, 0, 0, yp, None) == 3
    assert lib.rsort_u32_topk(xp, None, 100, 101, 0, yp, None) == 1
    assert lib.rsort_u32_topk(xp, None, 100, 5, 16, yp, None) == 1
    assert lib.rsort_u32_topk(xp, xp, 100, 5, 0, yp, None) == 1
    assert lib.rsort_u32_topk(xp, xp, 100, 5, rs.TOPK_INDICES, yp, vp) == 1
    assert lib.rsort_u32_topk(xp, None, 100, 5, rs.TOPK_INDICES, yp, None) == 1
    assert lib.rsort_u32_topk(None, None, 100, 5, 0, yp, None) == 1
    assert lib.rsort_u32_topk(None, None, 100, 0, 0, None, None) == 0
    assert lib.rsort_u32_topk(None, None, 0, 0, rs.TOPK_INDICES, None, None) == 0
    k, vv = rs.topkByDevice(x, 0, indices=True)
    assert k.size == 0 and vv.size == 0
    with pytest.raises(TypeError):
        rs.topkByDevice(x.astype(np.int64), 3)
    if not gpu_available():
        assert lib.rsort_u32_topk(xp, None, 100, 5, 0, yp, None) == 8
        with pytest.raises(rs.RSortError) as e:
            rs.topkByDevice(x, 5, largest=True, indices=True)
        assert e.value.status == 8
    assert not y.any() or gpu_available()


def _formula(n, k, pairs, route):
    """The byte formula of include/rsort.h, term by term."""
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    p = 2 if pairs else 1
    if route == rs.TOPK_SELECT:
        return (256 + r(4 * 8448) + 2 * 1024 * 256 * 4 + 2 * r(8 * 1024) + p * r(4 * k) + p * r(4 * n) +
                rs.workspace_size(k, 8, pairs) + 256)
    return 256 + p * r(4 * n) + rs.workspace_size(n, 8, pairs) + 256


@pytest.mark.parametrize("pairs", [False, True])
def test_workspace_size(pairs):
    sizes = [0, 1, 63, 1000, 70001, 1 << 20, (1 << 24) + 3, 1 << 30, (1 << 32) - 1]
    for route in (rs.TOPK_SELECT, rs.TOPK_SORT, rs.TOPK_AUTO):
        prev = None
        for n in sizes:
            ks = sorted({0, min(n, 1), min(n, 64), n // 3, max(n - 1, 0), n})
            row = []
            for k in ks:
                w = rs.topk_workspace_size(n, k, pairs, route)
                taken = route if route != rs.TOPK_AUTO else \
                    (rs.TOPK_SELECT if k <= rs.topk_auto_limit(n, pairs) else rs.TOPK_SORT)
                assert w >= _formula(n, k, pairs, taken), (n, k, route)
                assert w == rs.topk_workspace_size(n, k, pairs, taken)  # AUTO: what its route for (n, k) needs
                row.append(w)
            # monotone in n: at k = 0, and at k = n on a forced route (under AUTO k = n changes route with n: n = 0 selects
            # nothing, every larger n sorts; a fixed k is checked below on every route)
            key = (row[0], row[-1] if route != rs.TOPK_AUTO else 0)
            if prev is not None:
                assert key[0] >= prev[0] and key[1] >= prev[1], (n, route)
            prev = key
        for k in (1, 64, 1000):  # monotone in n at a fixed k
            ws = [rs.topk_workspace_size(n, k, pairs, route) for n in sizes if n >= k]
            assert ws == sorted(ws), (k, route)
    assert rs.topk_workspace_size(-1, 0, pairs) == 0
    assert rs.topk_workspace_size(1 << 32, 1, pairs) == 0
    assert rs.topk_workspace_size(10, 11, pairs) == 0
    assert rs.topk_workspace_size(10, -1, pairs) == 0
    assert rs.topk_workspace_size(10, 3, pairs, 3) == 0
    assert rs.topk_workspace_size(10, 3, pairs, -1) == 0


def test_route_switch():
    lib = rs._lib()
    assert lib.rsort_get_topk_route() == rs.TOPK_AUTO
    assert lib.rsort_set_topk_route(rs.TOPK_SORT) == rs.TOPK_AUTO
    assert lib.rsort_set_topk_route(3) == -1 and lib.rsort_set_topk_route(-1) == -1  # unknown: nothing changes
    assert lib.rsort_get_topk_route() == rs.TOPK_SORT
    assert lib.rsort_set_topk_route(rs.TOPK_SELECT) == rs.TOPK_SORT
    assert lib.rsort_set_topk_route(rs.TOPK_AUTO) == rs.TOPK_SELECT
    with rs.topk_route(rs.TOPK_SELECT):
        assert rs.get_topk_route() == rs.TOPK_SELECT
        with rs.topk_route(rs.TOPK_SORT):
            assert rs.get_topk_route() == rs.TOPK_SORT
        assert rs.get_topk_route() == rs.TOPK_SELECT
    assert rs.get_topk_route() == rs.TOPK_AUTO
    with pytest.raises(rs.RSortError):
        with rs.topk_route(7):
            pass
    assert rs.get_topk_route() == rs.TOPK_AUTO


def test_auto_limit():
    lib = rs._lib()
    v = ctypes.c_int64(77)
    assert lib.rsort_topk_auto_limit(10, 0, None) == 1
    assert lib.rsort_topk_auto_limit(-1, 0, ctypes.byref(v)) == 3 and v.value == 0
    assert lib.rsort_topk_auto_limit(1 << 32, 1, ctypes.byref(v)) == 3
    last = {False: 0, True: 0}
    for n in (0, 1, 7, 8, 63, 1000, 1 << 20, 1 << 30, (1 << 32) - 1):
        for pairs in (False, True):
            lim = rs.topk_auto_limit(n, pairs)
            assert 0 <= lim <= n
            assert lim >= last[pairs]
            last[pairs] = lim


def test_grid_entries_validate():
    lib = rs._lib()
    g = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert lib.rsort_topk_grids(10, 2, 0, None) == 1
    assert lib.rsort_topk_grids(-1, 0, 0, g) == 3 and list(g) == [0, 0, 0, 0]
    assert lib.rsort_topk_grids(10, 11, 0, g) == 1
    g[:] = [7, 7, 7, 7]
    assert lib.rsort_topk_grids(10, 0, 1, g) == 0 and list(g) == [0, 0, 0, 0]  # nothing to do: no device needed
    if not gpu_available():
        assert lib.rsort_topk_grids(1000, 3, 0, g) == 8  # the occupancy is a device's
    assert lib.rsort_set_topk_grid_limit(-1) == -1
    assert lib.rsort_set_topk_grid_limit(3) == 0
    assert lib.rsort_set_topk_grid_limit(-5) == -1
    assert lib.rsort_set_topk_grid_limit(0) == 3
    with rs.topk_grid_limit(2):
        with rs.topk_grid_limit(1):
            assert lib.rsort_set_topk_grid_limit(1) == 1
        assert lib.rsort_set_topk_grid_limit(2) == 2
    assert lib.rsort_set_topk_grid_limit(0) == 0
    with pytest.raises(rs.RSortError):
        with rs.topk_grid_limit(-2):
            pass
    assert lib.rsort_set_topk_grid_limit(0) == 0


def test_report_entry_validates():
    lib = rs._lib()
    r = (ctypes.c_int64 * 8)(*([9] * 8))
    assert lib.rsort_topk_report(10, 3, 0, P(256), None, None) == 1
    assert lib.rsort_topk_report(-1, 0, 0, P(256), r, None) == 3 and list(r) == [0] * 8
    assert lib.rsort_topk_report(10, 11, 0, P(256), r, None) == 1
    assert lib.rsort_topk_report(10, 3, 0, None, r, None) == 1
    r[:] = [9] * 8
    assert lib.rsort_topk_report(10, 0, 1, None, r, None) == 0 and list(r) == [0] * 8


class _NoStream:
    """Stands in for a torch stream where there may be no GPU: the validation paths never use it."""
    cuda_stream = None


def test_noop_calls_report_a_clean_check_field():
    """report8[6], the self-checks of the sort a call ran: 0 for a call that had nothing to do (k == 0), with no
    workspace and no device; rs.topk_check is that field."""
    lib = rs._lib()
    for n, k in ((10, 0), (0, 0), ((1 << 32) - 1, 0)):
        for pairs in (0, 1):
            r = (ctypes.c_int64 * 8)(*([9] * 8))
            assert lib.rsort_topk_report(n, k, pairs, None, r, None) == 0 and r[6] == 0 and r[7] == 0
            assert rs.topk_check(n, k, bool(pairs), None, stream=_NoStream()) == 0
    with pytest.raises(rs.RSortError) as e:
        rs.topk_check(10, 11, False, None, stream=_NoStream())
    assert e.value.status == 1


class _Returns:
    """The library with one entry replaced by a stub that returns `status`: what the Python mirror does with it."""

    def __init__(self, lib, name, status):
        self._lib, self._name, self._status, self.calls = lib, name, status, 0

    def __getattr__(self, attr):
        if attr != self._name:
            return getattr(self._lib, attr)

        def stub(*args):
            self.calls += 1
            return self._status
        return stub


def test_python_mirror_raises_on_a_check_status(monkeypatch):
    """rs.topkByDevice raises RSortError(11) when rsort_u32_topk returns RSORT_ERR_CHECK (no device: the entry is a
    stub here; tests/test_gpu_check_entries.py has the library return it)."""
    fake = _Returns(rs._lib(), "rsort_u32_topk", rs.RSORT_ERR_CHECK)
    monkeypatch.setattr(rs, "_LIB", fake)
    with pytest.raises(rs.RSortError) as e:
        rs.topkByDevice(np.arange(8, dtype=np.uint32), 3, indices=True)
    assert e.value.status == 11 == rs.RSORT_ERR_CHECK and fake.calls == 1
    assert "RSORT_ERR_CHECK" in str(e.value)


def test_python_constants():
    assert (rs.TOPK_LARGEST, rs.TOPK_UNSORTED, rs.TOPK_INDICES) == (1, 2, 4)
    assert (rs.TOPK_AUTO, rs.TOPK_SELECT, rs.TOPK_SORT) == (0, 1, 2)


# ------------------------------------------------------------------------------ the periodic input's closed form
def _periodic_bases(period):
    """A base of P distinct keys and one with long runs of duplicates (values below 5, and 0xFFFFFFFF among them)."""
    distinct = uniform_keys(period, seed=0xA11 + period)
    assert np.unique(distinct).size == period
    dup = (uniform_keys(period, seed=0xD0 + period) % np.uint32(5)).astype(np.uint32)
    dup[dup == 4] = 0xFFFFFFFF
    return (("distinct", distinct), ("dup", dup))


@pytest.mark.parametrize("period", (7, 13, 50, 97, 101))
def test_periodic_topk_closed_form_matches_the_oracle(period):
    """tests/_util.py periodic_topk_expected / periodic_topk_report (what the full-size GPU tests expect) against the
    oracle's stable order and host counting on the materialised x: n below, at and far above P, bases with and
    without duplicates, both directions, k in {1, 2, n // 3, n - 1, n}; the torch statement of the positions too."""
    for kind, base in _periodic_bases(period):
        for n in (1, 2, period - 1, period, period + 1, 3 * period, 1000, 4999, 5000):
            x = base[np.arange(n) % period]
            for largest in (False, True):
                m = np.uint32(0xFFFFFFFF if largest else 0)
                ko, idx = oracle_sort_pairs(x ^ m, np.arange(n, dtype=np.uint32), 8)
                tab = periodic_topk_tables(base, n, largest)
                tt = {f: torch.from_numpy(tab[f]) for f in PERIODIC_POSITION_TABLES}
                tt["P"] = period
                for k in sorted({min(max(k, 1), n) for k in (1, 2, n // 3, n - 1, n)}):
                    what = (kind, period, n, largest, k)
                    keys, pos = periodic_topk_expected(base, n, k, largest)
                    assert keys.dtype == np.uint32 and pos.dtype == np.int64, what
                    assert np.array_equal(pos, idx[:k]), what
                    assert np.array_equal(keys, ko[:k] ^ m) and np.array_equal(keys, x[idx[:k]]), what
                    tpos, _ = periodic_topk_positions(tt, torch.arange(k, dtype=torch.int64))
                    assert np.array_equal(tpos.numpy(), pos), what
                    kth = x[idx[k - 1]]  # host_report-style counting (tests/test_gpu_topk.py)
                    t = kth ^ m
                    before = int(np.count_nonzero((x ^ m) < t))
                    want = {"kth_key": int(kth), "before": before, "equal_taken": k - before,
                            "equal_in_input": int(np.count_nonzero(x == kth)),
                            "candidates": int(np.count_nonzero(((x ^ m) >> np.uint32(24)) == (t >> np.uint32(24))))}
                    assert periodic_topk_report(base, n, k, largest) == want, what


def test_periodic_topk_closed_form_never_touches_n_elements():
    """The full-size shape: n past 2^31, P = 4099, k = 2^20 -- well under a second, positions past 2^31 in int64."""
    import time
    n, k = (1 << 31) + (1 << 17) + 5, 1 << 20
    base = uniform_keys(4099, seed=0xA11)  # distinct: two whole keys' copies, spread over the input, are taken
    t0 = time.perf_counter()
    keys, pos = periodic_topk_expected(base, n, k, True)
    rep = periodic_topk_report(base, n, k, True)
    took = time.perf_counter() - t0
    assert took < 1.0, took
    assert keys.size == pos.size == k and int(pos.max()) >= 1 << 31 and int(pos.max()) < n
    assert np.array_equal(keys, base[pos % 4099]) and bool((np.diff(keys.astype(np.int64)) <= 0).all())
    same = keys[1:] == keys[:-1]
    assert bool((np.diff(pos)[same] > 0).all())  # equal keys in input order
    assert rep["before"] + rep["equal_taken"] == k and rep["before"] >= 2 * (n // 4099)
