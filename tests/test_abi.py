"""CPU-side checks of the C ABI: the library builds, loads, and exports every symbol that
include/rsort.h declares; planning and argument validation (no kernel launches here)."""
import ctypes
import re
from pathlib import Path

import pytest

from _rs import PKG, rs

ROOT = Path(__file__).resolve().parent.parent


def _declared_symbols():
    text = (ROOT / "include" / "rsort.h").read_text()
    return sorted(set(re.findall(r"RSORT_API\s+[\w\s\*]+?\b(rsort_\w+)\s*\(", text)))


def test_library_present_and_loads():
    assert rs.lib_path().exists(), "run __graft_entry__.build() first"
    lib = rs._lib()
    assert isinstance(lib, ctypes.CDLL)
    assert rs.version() == "0.1.0"


def test_every_declared_symbol_is_exported_and_bound():
    declared = _declared_symbols()
    assert len(declared) >= 25
    lib = rs._lib()
    for name in declared:
        assert hasattr(lib, name), name
        assert name in rs.SIGNATURES, f"{name} has no ctypes signature in radixsort.py"
    assert set(rs.SIGNATURES) == set(declared)


# Where a failed on-device self-check (rsort_plan_check's bits) of each entry reaches its caller: a closed table, one
# row per RSORT_API function. The kernels that record a check are the scatter kernels (sorts, the partition), the
# raw-table passes, the hybrid bucket kernel and the segmented sort's kernels.
#   NONE       launches no checked kernel (pure, a setting, a reader, or kernels that check nothing)
#   reader: F  stream-ordered: returns before the device has run, F reads the check afterwards
#   ERR_CHECK  waits for the device and returns RSORT_ERR_CHECK itself
#   (NOT, s)   none, documented: s is the sentence of rsort.h that says so
# tests/test_gpu_check_entries.py and tests/test_gpu_check.py drive every reader and ERR_CHECK row on the device.
NONE, ERR_CHECK = "launches no checked kernel", "returns RSORT_ERR_CHECK"
_PASS_SENTENCE = ("rsort_pass_scatter and rsort_pass_local_sort take no workspace and so have no check word: the "
                  "self-checks that rsort_plan_check reports for a whole sort are not recorded for a single pass, and "
                  "no call returns them.")
NOT = ("none, documented", _PASS_SENTENCE)
CHECK_REACHES_CALLER = {
    "rsort_status_string": NONE, "rsort_version": NONE, "rsort_plan_make": NONE, "rsort_workspace_size": NONE,
    "rsort_u32_device": "reader: rsort_plan_check", "rsort_u32_pairs_device": "reader: rsort_plan_check",
    "rsort_sort_planned_ex": "reader: rsort_plan_check", "rsort_sort_planned": "reader: rsort_plan_check",
    "rsort_u32": ERR_CHECK, "rsort_u32_ex": ERR_CHECK, "rsort_u32_pairs": ERR_CHECK,
    "rsort_segmented_capacity": NONE, "rsort_segmented_workspace_size": NONE,
    "rsort_u32_segmented_device": "reader: rsort_segmented_check", "rsort_segmented_check": NONE,
    "rsort_u32_segmented": ERR_CHECK,
    "rsort_topk_workspace_size": NONE, "rsort_u32_topk_device": "reader: rsort_topk_report",
    "rsort_u32_topk": ERR_CHECK, "rsort_topk_report": NONE, "rsort_set_topk_route": NONE,
    "rsort_get_topk_route": NONE, "rsort_topk_auto_limit": NONE, "rsort_topk_grids": NONE,
    "rsort_set_topk_grid_limit": NONE,
    "rsort_topk_rows_workspace_size": NONE, "rsort_u32_topk_rows_device": "reader: rsort_topk_rows_check",
    "rsort_u32_topk_rows": ERR_CHECK, "rsort_topk_rows_check": NONE, "rsort_topk_rows_grids": NONE,
    "rsort_set_topk_rows_grid_limit": NONE,
    "rsort_pass_histogram": NONE, "rsort_pass_scan": NONE, "rsort_pass_scatter": NOT, "rsort_pass_local_sort": NOT,
    "rsort_set_rank_algo": NONE, "rsort_get_rank_algo": NONE, "rsort_set_group_chunks": NONE,
    "rsort_get_group_chunks": NONE, "rsort_set_hybrid": NONE, "rsort_get_hybrid": NONE,
    "rsort_hybrid_capacity": NONE, "rsort_hybrid_kernel_info": NONE, "rsort_hybrid_range": NONE,
    "rsort_hybrid_gate_threshold": NONE, "rsort_hybrid_report": NONE, "rsort_group_flags": NONE,
    "rsort_cut_plan_stats": NONE, "rsort_plan_check": NONE, "rsort_plan_features": NONE,
    "rsort_inject_table_fault": NONE, "rsort_inject_rank_fault": NONE, "rsort_inject_fault_window": NONE,
    "rsort_fault_window_calls": NONE, "rsort_segmented_grids": NONE, "rsort_set_segmented_grid_limit": NONE,
    "rsort_scatter_kernels_used": NONE, "rsort_scatter_kernels_known": NONE, "rsort_lane_order_probe": NONE,
    "rsort_profile_begin": NONE, "rsort_profile_end": NONE,
    "rsort_partition_workspace_size": NONE, "rsort_partition_device": "reader: rsort_partition_check",
    "rsort_partition_check": NONE, "rsort_top_histogram": NONE, "rsort_top_histogram_sampled": NONE,
    "rsort_multi_sample_plan": NONE, "rsort_sample_device": NONE, "rsort_multi_quantile_index": NONE,
    "rsort_multi_splitters_make": NONE, "rsort_multi_splitters_make_hot": NONE, "rsort_multi_exchange_plan": NONE,
    "rsort_multi_exchange_rounds": NONE, "rsort_multi_workspace_size": NONE,
    "rsort_u32_multi": ERR_CHECK, "rsort_u32_multi_transport": ERR_CHECK,
    "rsort_rccl_unique_id": NONE, "rsort_rccl_comm_init": NONE, "rsort_rccl_comm_destroy": NONE,
    "rsort_set_comm_timeout": NONE, "rsort_set_multi_options": NONE, "rsort_multi_set_profiling": NONE,
    "rsort_multi_last_stats": NONE, "rsort_multi_inject_failure": NONE, "rsort_set_exchange_piece": NONE,
    "rsort_host_transport_wrap": NONE, "rsort_host_transport_free": NONE, "rsort_loopback_create": NONE,
    "rsort_loopback_transport": NONE, "rsort_loopback_destroy": NONE,
    "rsort_vendor_workspace_size": NONE, "rsort_u32_vendor_device": NONE, "rsort_u32_vendor": NONE,
    "rsort_vendor_segmented_workspace_size": NONE, "rsort_u32_vendor_segmented_device": NONE,
    "rsort_fingerprint_device": NONE, "rsort_gen_uniform": NONE, "rsort_gen_zipf": NONE, "rsort_gen_iota": NONE,
}


def test_every_entry_says_where_a_failed_self_check_goes():
    """The table is closed: a declared function without a row fails, a row naming no declared function fails, every
    reader named is itself declared and launches nothing checked, and a "none, documented" row quotes rsort.h."""
    declared = set(_declared_symbols())
    assert declared - set(CHECK_REACHES_CALLER) == set(), "declared in rsort.h, no row in the table"
    assert set(CHECK_REACHES_CALLER) - declared == set(), "rows naming no declared function"
    header = " ".join((ROOT / "include" / "rsort.h").read_text().replace("*", " ").split())
    for name, how in CHECK_REACHES_CALLER.items():
        if isinstance(how, tuple):
            assert how[0] == "none, documented" and " ".join(how[1].split()) in header, name
        elif how.startswith("reader: "):
            reader = how[len("reader: "):]
            assert reader in declared and CHECK_REACHES_CALLER[reader] == NONE, name
        else:
            assert how in (NONE, ERR_CHECK), name
    # every host -> host and multi-GPU sorting entry waits for the device: it has no excuse not to return the check
    waits = {n for n in declared if re.fullmatch(r"rsort_u32(_ex|_pairs|_segmented|_topk|_topk_rows|_multi\w*)?", n)}
    assert waits == {n for n, how in CHECK_REACHES_CALLER.items() if how == ERR_CHECK}


def test_status_strings():
    lib = rs._lib()
    for st in range(12):
        assert lib.rsort_status_string(st) != b"unknown status", st
        assert rs.STATUS_NAMES[st].startswith("RSORT_")
    assert lib.rsort_status_string(12) == b"unknown status"
    assert lib.rsort_status_string(2) == b"k_bits outside [1, 13]"


@pytest.mark.parametrize("n,k", [(0, 8), (1, 8), (513, 4), ((1 << 24) + 1, 8), (1 << 26, 4), (1 << 30, 8),
                                 ((1 << 32) - 1, 8), (100003, 12), (5, 1)])
def test_plan_geometry(n, k):
    p = rs.plan(n, k, False, tiles_per_chunk=0)
    assert p.passes == -(-32 // k)
    assert p.bins == 1 << k
    assert (p.threads, p.tile_keys) in {(256, 4096), (512, 16384), (512, 8192), (1024, 16384)}
    if n >= 2 * 256 * 16384 and 5 <= k <= 8:
        assert (p.threads, p.tile_keys) == (1024, 16384)  # whole-line (rs_scatter_lines) tiles
        assert (rs.plan(n, k, True).threads, rs.plan(n, k, True).tile_keys) == (1024, 8192)  # pairs lines
    assert p.chunk_keys == p.tiles_per_chunk * p.tile_keys
    assert p.num_chunks * p.chunk_keys >= n
    assert (p.num_chunks - 1) * p.chunk_keys < max(n, 1)
    assert p.table_entries == p.bins * p.num_chunks
    assert p.workspace_bytes >= 4 * n + 4 * p.table_entries
    assert rs.workspace_size(n, k) == p.workspace_bytes
    pp = rs.plan(n, k, True)
    assert pp.workspace_bytes >= 8 * n + 4 * pp.table_entries


def test_plan_explicit_tiles_per_chunk():
    p = rs.plan(1 << 20, 8, tiles_per_chunk=1)
    assert p.num_chunks == 256 and p.chunk_keys == 4096
    p = rs.plan(1 << 20, 8, tiles_per_chunk=7)
    assert p.num_chunks == -(-256 // 7)


@pytest.mark.parametrize("n,k,status", [(10, 0, 2), (10, 14, 2), (-1, 8, 3), (1 << 32, 8, 3)])
def test_plan_rejects(n, k, status):
    with pytest.raises(rs.RSortError) as e:
        rs.plan(n, k)
    assert e.value.status == status


def _shaped(n, k, pairs, threads, tile_keys):
    """The planner's plan for (n, k, pairs) moved to another tile shape, every derived field kept consistent."""
    p = rs.plan(n, k, pairs)
    p.threads, p.tile_keys = threads, tile_keys
    tiles = max(1, -(-n // tile_keys))
    p.tiles_per_chunk = max(1, -(-tiles // 512))
    p.chunk_keys = p.tiles_per_chunk * tile_keys
    p.num_chunks = -(-tiles // p.tiles_per_chunk)
    p.table_entries = p.bins * p.num_chunks
    return p


def test_plan_shape_without_a_kernel_is_rejected():
    """check_plan (every entry point that takes a plan) answers RSORT_ERR_ARG for a (k, pairs, tile shape) no
    scatter kernel exists for -- the shapes the planner never picks -- instead of failing at the first launch."""
    n = 1 << 24
    feat = lambda p: rs._lib().rsort_plan_features(ctypes.byref(p))  # noqa: E731
    # (an n = 0 plan: rsort_pass_scan returns right after the plan check, RSORT_OK for a valid one)
    scan = lambda k, pairs, th, tile: rs._lib().rsort_pass_scan(  # noqa: E731
        ctypes.byref(_shaped(0, k, pairs, th, tile)), None, None, None)
    no_kernel = [(k, pairs, 512, 16384) for k in (4, 5, 6, 7, 8) for pairs in (False, True)]  # 512 x 32: no kernel at all
    no_kernel += [(6, False, 512, 8192), (1, True, 512, 8192)]   # 512 x 16: keys only, k <= 5
    no_kernel += [(4, True, 1024, 8192)]                         # pair line tiles: k = 5..8
    no_kernel += [(13, False, 256, 4096), (8, False, 128, 4096), (9, False, 1024, 16384), (3, True, 1024, 8192)]
    for k, pairs, th, tile in no_kernel:
        p = _shaped(n, k, pairs, th, tile)
        assert feat(p) == -1, (k, pairs, th, tile)
        assert scan(k, pairs, th, tile) == 1, (k, pairs, th, tile)
    with pytest.raises(rs.RSortError) as e:
        rs.plan_features(_shaped(n, 6, False, 512, 16384))
    assert e.value.status == 1
    # the same moves onto shapes that do have a kernel stay valid plans
    have = [(1, False, 512, 8192), (2, False, 512, 8192), (4, False, 1024, 16384), (8, False, 1024, 16384),
            (5, True, 1024, 8192), (8, True, 1024, 8192), (12, True, 256, 4096), (13, True, 128, 4096),
            (3, False, 512, 8192), (5, False, 512, 8192)]  # (the last two: keys-only partitions' shape and bits)
    for k, pairs, th, tile in have:
        p = _shaped(n, k, pairs, th, tile)
        assert feat(p) >= 0, (k, pairs, th, tile)
        assert scan(k, pairs, th, tile) == 0, (k, pairs, th, tile)
    # every plan the planner makes passes
    for k in range(1, 14):
        for pairs in (False, True):
            for nn in (1, 70001, 1 << 24, 1 << 28, (1 << 32) - 1):
                assert feat(rs.plan(nn, k, pairs)) >= 0, (k, pairs, nn)


def test_scatter_kernels_known_is_host_only_and_closed():
    known = rs.scatter_kernels_known()
    assert len(known) == len(set(known)) and len(known) > 100
    assert all(re.fullmatch(r"rs_scatter(_lines|_pairs)?<[\w, ]+>", k) for k in known), known
    assert not any(k.startswith("rs_scatter<") and ", 512, 32," in k for k in known)  # no 512 x 32 tiles
    lib = rs._lib()
    n = int(lib.rsort_scatter_kernels_known(None, 0))
    buf = ctypes.create_string_buffer(8)
    assert int(lib.rsort_scatter_kernels_known(buf, 8)) == n and buf.value == ";".join(known).encode()[:7]


def test_device_entry_validates_before_touching_the_gpu():
    lib = rs._lib()
    # bad k, bad n: rejected before any HIP call
    assert lib.rsort_u32_device(None, None, 10, 0, None, 0, None) == 2
    assert lib.rsort_u32_device(None, None, -5, 8, None, 0, None) == 3
    # n == 0 is a no-op that needs no buffers
    assert lib.rsort_u32_device(None, None, 0, 8, None, 0, None) == 0
    # NULL buffers with n > 0
    assert lib.rsort_u32_device(None, None, 10, 8, None, 0, None) == 1
    # misaligned pointers
    assert lib.rsort_u32_device(ctypes.c_void_p(2), ctypes.c_void_p(8), 10, 8, ctypes.c_void_p(256), 1 << 20, None) == 4
    # workspace too small
    assert lib.rsort_u32_device(ctypes.c_void_p(256), ctypes.c_void_p(512), 10, 8, ctypes.c_void_p(1024), 16, None) == 7
    assert lib.rsort_set_rank_algo(7) == 1
    assert lib.rsort_set_rank_algo(3) == 1
    assert lib.rsort_partition_device(None, None, None, None, 10, None, 0, None, None, 0, None) == 1
    assert lib.rsort_partition_device(None, None, None, None, 10, None, 17, None, None, 0, None) == 1


def test_python_mirror_error_behaviour():
    import numpy as np
    with pytest.raises(ValueError):
        rs.sort(np.zeros(4, np.uint32), 4, np.zeros(4, np.uint32), rs.SORT_BY_HOST)
    with pytest.raises(TypeError):
        rs.sortByDevice(np.zeros(4, np.int64), 4, np.zeros(4, np.uint32), 8)
    with pytest.raises(rs.RSortError) as e:
        rs.sortByDevice(np.zeros(4, np.uint32), 4, np.zeros(4, np.uint32), 14)
    assert e.value.status == 2


def test_no_cpu_fallback_without_device():
    """On a machine without a GPU the host entry must FAIL (RSORT_ERR_NODEV), not sort on CPU."""
    from _rs import gpu_available
    if gpu_available():
        pytest.skip("GPU present")
    import numpy as np
    x = np.arange(100, dtype=np.uint32)[::-1].copy()
    y = np.zeros_like(x)
    with pytest.raises(rs.RSortError) as e:
        rs.sortByDevice(x, x.size, y, 8)
    assert e.value.status == 8
    assert not y.any()


def test_package_sources_do_not_reference_the_oracle():
    for f in list(PKG.rglob("*.py")) + list(PKG.rglob("*.cpp")) + list(PKG.rglob("*.hip")) + \
            list((ROOT / "include").glob("*")):
        text = f.read_text()
        assert "liboracle" not in text and "oracle_sort" not in text and "_ref/libref" not in text, f


def test_reference_harness_cli_builds_and_links():
    """tools/rsort_cli: the reference main (Parallel7.cu:696-775) on include/radixsort.hpp."""
    import subprocess
    cli = ROOT / "tools" / "rsort_cli"
    assert cli.exists(), "built by __graft_entry__.build()"
    out = subprocess.run(["ldd", str(cli)], capture_output=True, text=True).stdout
    assert "librsort.so" in out and "not found" not in out.split("librsort.so")[1].split("\n")[0]


def test_compat_header_compiles_with_reference_style_main(tmp_path):
    """A Parallel*.cu-style caller (own sortByHost + main, the reference's sort() signature and
    default arguments) compiles and links unchanged against radixsort.hpp + librsort.so."""
    import subprocess
    src = tmp_path / "caller.cpp"
    src.write_text(r'''
#include "radixsort.hpp"
#include <string.h>
void sortByHost(const uint32_t *in, int n, uint32_t *out, int nBits) { memcpy(out, in, n * 4); (void)nBits; }
int main() {
    uint32_t in[4] = {3, 1, 2, 0}, out[4];
    sort(in, 4, out);                       // default SORT_BY_HOST, numBits = 4, blockSize = 1
    sort(in, 4, out, SORT_BY_DEVICE, 8, 512);
    sort(in, 4, out, SORT_BY_THRUST);
    return 0;
}
''')
    exe = tmp_path / "caller"
    cmd = ["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
           f"-L{PKG}", "-lrsort", f"-Wl,-rpath,{PKG}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("n,world", [(1 << 27, 8), (1 << 22, 2), (3 << 24, 4)])
def test_multi_workspace_holds_any_local_sort(n, world):
    """rsort_multi_workspace_size covers the local sort of any received count up to the capacity --
    including counts whose plan is a digit-group plan with its joint-count rows (64 MiB) where the
    capacity's own plan is not one: the partition buffer (4 n B) plus the largest sort workspace."""
    lib = rs._lib()
    cap = rs.default_capacity(n)
    mw = int(lib.rsort_multi_workspace_size(n, cap, 8, 0, world))
    sizes = {cap, cap // 2 + 1, n, 1 << 25, (1 << 24) + 5, 1 << 23, 3 << 22, 1 << 20, 1}
    need = max(rs.workspace_size(m, 8) for m in sizes if m <= cap)
    assert mw >= 4 * n + need, (mw, need)


def _sort_call():
    """One entry into the LSD driver that needs no device: an n = 0 sort (a numbered sort call that then does nothing)."""
    assert rs._lib().rsort_u32_device(None, None, 0, 8, None, 0, None) == 0


def test_fault_window_numbers_the_sort_calls_and_clears():
    """rsort_inject_fault_window, host side: setting it (and clearing it) restarts the calling thread's count of sort
    calls; rsort_fault_window_calls reads it; a negative first with a window is refused and changes nothing; the
    context manager clears on exit, also when its block raises."""
    lib = rs._lib()
    assert lib.rsort_inject_fault_window(0, -1) == 0 and rs.fault_window_calls() == 0
    _sort_call()
    assert rs.fault_window_calls() == 1  # (counted with the window cleared too)
    with rs.fault_window(1, 2):
        assert rs.fault_window_calls() == 0
        for i in range(4):
            _sort_call()
            assert rs.fault_window_calls() == i + 1
        assert lib.rsort_inject_fault_window(-1, 1) == 1 and rs.fault_window_calls() == 4  # refused: nothing changes
        with pytest.raises(rs.RSortError):
            with rs.fault_window(-3, 0):
                pass
    assert rs.fault_window_calls() == 0  # cleared on exit: a new count
    with pytest.raises(KeyError):
        with rs.fault_window(0, 1):
            _sort_call()
            raise KeyError("from the block")
    assert rs.fault_window_calls() == 0
    # the pairs entry and the planned entries are sort calls too; a plan that is refused never enters the driver
    assert lib.rsort_u32_pairs_device(None, None, None, None, 0, 8, None, 0, None) == 0
    p = rs.plan(0, 8)
    assert lib.rsort_sort_planned(ctypes.byref(p), None, None, None, None, None, 0, None) == 0
    assert lib.rsort_sort_planned_ex(ctypes.byref(p), None, None, None, None, None, 0, None, 1) == 0
    assert lib.rsort_u32_device(None, None, 10, 0, None, 0, None) == 2
    assert rs.fault_window_calls() == 3


def test_fault_window_is_thread_local():
    """Two threads: each sets its own window and counts its own sort calls; neither sees the other's, and the main
    thread's count is untouched."""
    import threading
    lib = rs._lib()
    assert lib.rsort_inject_fault_window(0, -1) == 0
    _sort_call()
    seen, step = {}, threading.Barrier(2, timeout=30)

    def run(name, calls):
        with rs.fault_window(0, 1):
            step.wait()  # both windows are set before either thread sorts
            for _ in range(calls):
                _sort_call()
            step.wait()  # both have sorted before either reads
            seen[name] = rs.fault_window_calls()
            step.wait()
        seen[name + " after"] = rs.fault_window_calls()

    th = [threading.Thread(target=run, args=("a", 2)), threading.Thread(target=run, args=("b", 5))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th)
    assert seen == {"a": 2, "b": 5, "a after": 0, "b after": 0}
    assert rs.fault_window_calls() == 1
