"""GPU: every scatter kernel instantiation the dispatch can launch is launched by a test, and the list is closed.

rs.scatter_kernels_known() is the dispatch's own list: its one selection function over its whole argument domain
(host only). Each name is accounted for in exactly one of three places:

  SWEEP              launched here: one row per instance that no other test launches, run at the planner's own
                     thresholds (rs.plan / rs.partition_device pick the tile shape; no hand-made plans), bit-exact
                     against the oracle (partitions: numpy's stable argsort by bucket), and then found in
                     rs.scatter_kernels_used().
  COVERED_ELSEWHERE  launched by the named existing test. The table is a recording, not a reading: running this
                     file as a script (`python tests/test_gpu_kernel_sweep.py --record out.json`) runs the rest of
                     the GPU suite with rs.scatter_kernels_used() collected per test, writes name -> first test,
                     and checks this table against the run.
  NOT_RUN            cannot be launched on this device or at a size a test can hold, for one of two reasons only,
                     and at most 20 names. The sorts' "needs n + shift >= 2^32" kernels run here in local mode
                     (rs.pass_local_sort takes the same kernel); the partitions' three have no local mode.

test_every_known_kernel_is_accounted_for fails when an instantiation is added to the dispatch without a row in one
of the three, and when a row names a kernel the dispatch no longer has. Runs on the MI355X box (-m gpu)."""
import json
import re
import sys

import numpy as np
import pytest

from _rs import rs
from _util import oracle_block_pass, oracle_sort, oracle_sort_pairs, uniform_keys, zipf_keys

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROBE_FAILS = "needs a failed lane-order probe"
BEYOND_2_32 = "needs n + shift >= 2^32"
NOT_RUN_REASONS = (PROBE_FAILS, BEYOND_2_32)
NOT_RUN_MAX = 20


# ------------------------------------------------------------------------------ from a kernel's name to a launch
def parse(name):
    """'rs_scatter<8, 256, 16, true, 4, 0, 0>' -> ('rs_scatter', [8, 256, 16, 1, 4, 0, 0])."""
    m = re.fullmatch(r"(rs_scatter(?:_lines|_pairs)?)<(.*)>", name)
    assert m, name
    return m.group(1), [{"true": 1, "false": 0}.get(a.strip(), a.strip()) for a in m.group(2).split(",")]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _algo(rank):
    return {1: rs.RANK_SPLIT, 3: rs.RANK_BALLOT, 4: rs.RANK_MATCH}[rank]


def scenario(name):
    """What to run so that the planner and the dispatch pick `name`: a dict, or None where nothing this file
    runs can (the closure test then wants the name in COVERED_ELSEWHERE or NOT_RUN)."""
    kind, a = parse(name)
    a = [int(x) for x in a]
    big = {8192: 2 * _cus() * 8192 + 4099, 16384: 2 * _cus() * 16384 + 4099}
    if kind == "rs_scatter_pairs":
        bits, th, kpt, cl = a
        return {"op": "sort", "n": big[th * kpt], "k": bits, "pairs": True, "algo": rs.RANK_MATCH}
    if kind == "rs_scatter_lines":
        bits, th, kpt, g, pairs, dmode, nt, cl = a
        if dmode == 1:
            if th == 512:  # keys-only partitions of large inputs
                return {"op": "partition", "n": big[8192], "nb": 3 if cl == 2 else (1 << bits) - 1, "pairs": False}
            nb = {2: 3, 3: 7, 4: 16, 5: 32}[bits]
            if (cl == 2) != (nb <= 4):
                return None
            return {"op": "partition", "n": 200003, "nb": nb, "pairs": bool(pairs)}
        if cl == 1:
            return None  # the clustered twin of a k = 8 digit-group pass: the digit-group tests' own
        if th == 256:
            n = 70001 if nt == 1 else (1 << 26) + 70001
        else:
            n = (1 << 28) + 77 if bits == 4 else big[th * kpt]
        return {"op": "sort", "n": n, "k": bits, "pairs": bool(pairs), "algo": rs.RANK_MATCH}
    bits, th, kpt, pairs, rank, dmode, minw = a
    if dmode == 1:
        if rank != 4:
            return None
        if th == 256 and pairs and bits >= 2:  # values no multiple of 16 B from the keys: no whole lines
            return {"op": "partition", "n": 200003, "nb": {2: 3, 3: 7, 4: 16, 5: 32}[bits], "pairs": True,
                    "vals_off": 1}
        return None
    tile = th * kpt
    sc = {"op": "sort", "k": bits, "pairs": bool(pairs), "algo": _algo(rank)}
    if tile == 4096:
        sc["n"] = 70001
        if rank == 4 and not pairs and bits in (3, 4):
            sc["op"] = "local"  # (a line-capable output takes rs_scatter_lines)
    elif tile == 8192 and not pairs:
        sc["n"] = big[8192]
    elif tile == 8192:
        sc["n"] = big[8192]
        if rank == 4:
            sc["vals_off"] = 1
    else:
        sc["n"] = (1 << 28) + 12345 if bits == 4 else big[16384]
        if rank == 4:
            sc["op"] = "local"
    return sc


def _dev(a):
    return rs.from_numpy_u32(a)


def _host(t):
    return rs.to_numpy_u32(t)


def run_sort(sc):
    n, k, pairs = sc["n"], sc["k"], sc["pairs"]
    if n > (1 << 26):
        # too many keys for the host oracle: on the device against the vendor sort (a key sort's output is
        # unique) plus the multiset fingerprint, as tests/test_gpu_fullsize.py::test_fullsize_uniform does
        assert not pairs
        keys = rs.empty_u32(n)
        rs.gen_uniform(keys, 0x5EED + k)
        out = rs.empty_u32(n)
        with rs.rank_algo(sc["algo"]):
            rs.sort_device(keys, out, k)
        ref = rs.empty_u32(n)
        rs.vendor_sort_device(keys, ref)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        assert rs.fingerprint(out) == (rs.fingerprint(keys)[0], 0)
        return
    x = zipf_keys(n, seed=k) if pairs else uniform_keys(n, seed=k)
    off = sc.get("vals_off", 0)
    ko = rs.empty_u32(n)
    with rs.rank_algo(sc["algo"]):
        if not pairs:
            rs.sort_device(_dev(x), ko, k)
            torch.cuda.synchronize()
            assert np.array_equal(_host(ko), oracle_sort(x, k))
            return
        v = np.arange(n, dtype=np.uint32)
        vbuf = torch.zeros(n + 2 * off, dtype=torch.int32, device="cuda")
        vo = vbuf[off:off + n]
        assert ((vo.data_ptr() - ko.data_ptr()) % 16 != 0) == bool(off)
        rs.sort_device(_dev(x), ko, k, vals_in=_dev(v), vals_out=vo)
        torch.cuda.synchronize()
    ek, ev = oracle_sort_pairs(x, v, k)
    assert np.array_equal(_host(ko), ek) and np.array_equal(_host(vo), ev)
    if off:
        assert int(vbuf[0]) == 0 and int(vbuf[-1]) == 0


def run_partition(sc):
    n, nb, pairs = sc["n"], sc["nb"], sc["pairs"]
    off = sc.get("vals_off", 0)
    x = zipf_keys(n, seed=nb)
    v = np.arange(n, dtype=np.uint32)
    split = np.sort(uniform_keys(nb - 1, seed=nb))
    bucket = np.searchsorted(split, x, side="right")
    order = np.argsort(bucket, kind="stable")
    ko, starts = rs.empty_u32(n), rs.empty_u32(nb + 1)
    vbuf = torch.zeros(n + 2 * off, dtype=torch.int32, device="cuda")
    vo = vbuf[off:off + n] if pairs else None
    rs.partition_device(_dev(x), ko, split.tolist(), starts, vals_in=_dev(v) if pairs else None, vals_out=vo)
    torch.cuda.synchronize()
    assert np.array_equal(_host(ko), x[order])
    if pairs:
        assert np.array_equal(_host(vo), v[order])
        assert int(vbuf[0]) == 0 and int(vbuf[-1]) == 0
    want = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=nb))]).astype(np.uint32)
    assert np.array_equal(_host(starts), want)


def run_local(sc):
    """Local mode only: every tile stably sorted by one digit, in place of the tile (rs.pass_local_sort).
    Checked whole on the device against torch's stable sort of every tile's digits, and the first tiles and the
    last (partial) one against the oracle's local tiles (oracle_block_pass)."""
    n, k = sc["n"], sc["k"]
    shift = k  # (the second digit: above bit 0, and whole at every k here)
    p = rs.plan(n, k, False)
    tile = p.tile_keys
    keys = rs.empty_u32(n)
    rs.gen_uniform(keys, 0xABC + k)
    out = rs.empty_u32(n)
    with rs.rank_algo(sc["algo"]):
        rs.pass_local_sort(p, keys, out, shift)
    torch.cuda.synchronize()
    full = n // tile * tile
    for lo, hi in ((0, full), (full, n)):
        if hi == lo:
            continue
        kk = (keys[lo:hi].to(torch.int64) & 0xFFFFFFFF).view(-1, hi - lo if lo else tile)
        idx = torch.sort((kk >> shift) & ((1 << k) - 1), dim=1, stable=True).indices
        assert torch.equal(out[lo:hi].to(torch.int64) & 0xFFFFFFFF, torch.gather(kk, 1, idx).view(-1))
    head = min(n, 4 * tile)
    for lo, hi in ((0, head), (full, n)):
        if hi > lo:
            _, _, loc, _ = oracle_block_pass(_host(keys[lo:hi]), k, shift, tile, int(p.chunk_keys))
            assert np.array_equal(_host(out[lo:hi]), loc)


def launch_and_check(name):
    sc = scenario(name)
    assert sc is not None, f"nothing here launches {name}"
    rs.scatter_kernels_used(reset=True)
    {"sort": run_sort, "partition": run_partition, "local": run_local}[sc["op"]](sc)
    used = rs.scatter_kernels_used(reset=True)
    assert name in used, (name, sc, used)


# ------------------------------------------------------------------------------ the three tables
# (the rows' order is the dispatch's: digit bits, keys before pairs)
SWEEP = [
    "rs_scatter<1, 512, 16, false, 3, 0, 4>",
    "rs_scatter<1, 512, 16, false, 4, 0, 4>",
    "rs_scatter<1, 256, 16, true, 1, 0, 0>",
    "rs_scatter<1, 256, 16, true, 3, 0, 0>",
    "rs_scatter<1, 256, 16, true, 4, 0, 0>",
    "rs_scatter<2, 512, 16, false, 3, 0, 4>",
    "rs_scatter<2, 256, 16, true, 1, 0, 0>",
    "rs_scatter<2, 256, 16, true, 3, 0, 0>",
    "rs_scatter<2, 256, 16, true, 4, 0, 0>",
    "rs_scatter<2, 256, 16, true, 4, 1, 0>",
    "rs_scatter<3, 256, 16, true, 1, 0, 0>",
    "rs_scatter<3, 256, 16, true, 3, 0, 0>",
    "rs_scatter<3, 256, 16, true, 4, 0, 0>",
    "rs_scatter<3, 256, 16, true, 4, 1, 0>",
    "rs_scatter<4, 1024, 16, false, 3, 0, 0>",
    "rs_scatter_lines<4, 256, 16, 32, false, 0, 3, 0>",
    "rs_scatter<4, 256, 16, true, 4, 1, 0>",
    "rs_scatter<5, 1024, 16, false, 3, 0, 0>",
    "rs_scatter<5, 1024, 8, true, 3, 0, 0>",
    "rs_scatter<5, 1024, 8, true, 4, 0, 0>",
    "rs_scatter<5, 256, 16, true, 4, 1, 0>",
    "rs_scatter<6, 1024, 16, false, 3, 0, 0>",
    "rs_scatter<6, 256, 16, true, 1, 0, 0>",
    "rs_scatter<6, 256, 16, true, 3, 0, 0>",
    "rs_scatter<6, 1024, 8, true, 3, 0, 0>",
    "rs_scatter<6, 256, 16, true, 4, 0, 0>",
    "rs_scatter<6, 1024, 8, true, 4, 0, 0>",
    "rs_scatter<7, 1024, 16, false, 3, 0, 0>",
    "rs_scatter<7, 256, 16, true, 1, 0, 0>",
    "rs_scatter<7, 256, 16, true, 3, 0, 0>",
    "rs_scatter<7, 1024, 8, true, 3, 0, 0>",
    "rs_scatter<7, 256, 16, true, 4, 0, 0>",
    "rs_scatter<7, 1024, 8, true, 4, 0, 0>",
    "rs_scatter<8, 1024, 8, true, 3, 0, 0>",
    "rs_scatter<9, 256, 16, true, 1, 0, 0>",
    "rs_scatter<9, 256, 16, true, 3, 0, 0>",
    "rs_scatter<9, 256, 16, true, 4, 0, 0>",
    "rs_scatter<10, 256, 16, true, 1, 0, 0>",
    "rs_scatter<10, 256, 16, true, 3, 0, 0>",
    "rs_scatter<10, 256, 16, true, 4, 0, 0>",
    "rs_scatter<11, 256, 16, true, 1, 0, 0>",
    "rs_scatter<11, 256, 16, true, 3, 0, 0>",
    "rs_scatter<11, 256, 16, true, 4, 0, 0>",
    "rs_scatter<13, 128, 32, true, 1, 0, 0>",
    "rs_scatter<13, 128, 32, true, 3, 0, 0>",
]

# name -> the first test of the recording that launched it
COVERED_ELSEWHERE = {
    "rs_scatter<1, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-1]",
    "rs_scatter<1, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-1]",
    "rs_scatter<1, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_all_golden_cases",
    "rs_scatter<2, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-2]",
    "rs_scatter<2, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-2]",
    "rs_scatter<2, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[0-2]",
    "rs_scatter<2, 512, 16, false, 4, 0, 4>": "tests/test_gpu_parity.py::test_large_tile_geometries[2]",
    "rs_scatter_lines<2, 256, 16, 32, false, 1, 3, 2>": "tests/test_gpu_multi.py::test_c_multi_single_rank",
    "rs_scatter_lines<2, 256, 16, 16, true, 1, 2, 2>": "tests/test_gpu_multi.py::test_dist_sort_rccl_single_rank",
    "rs_scatter<3, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-3]",
    "rs_scatter<3, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-3]",
    "rs_scatter<3, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_pass_intermediates_vs_block_oracle[0-20480-3-3-5]",
    "rs_scatter_lines<3, 256, 16, 32, false, 0, 3, 0>": "tests/test_gpu_fullsize.py::test_fullsize_uniform[134217725-3]",
    "rs_scatter_lines<3, 256, 16, 32, false, 0, 1, 0>": "tests/test_gpu_groups.py::test_next_digit_counts[163843-uniform-3]",
    "rs_scatter_lines<3, 256, 16, 32, false, 1, 3, 0>": "tests/test_gpu_multi.py::test_c_multi_loopback_failure_after_sample_gather[1-1]",
    "rs_scatter_lines<3, 512, 16, 32, false, 1, 3, 0>": "tests/test_gpu_check.py::test_partition_check_and_multi_gpu_sort_report_a_broken_lane_order",
    "rs_scatter_lines<3, 512, 16, 32, false, 1, 3, 2>": "tests/test_gpu_check.py::test_partition_check_and_multi_gpu_sort_report_a_broken_lane_order",
    "rs_scatter_lines<3, 256, 16, 16, true, 1, 2, 0>": "tests/test_gpu_multi.py::test_c_multi_loopback[12-hot-True-8-None]",
    "rs_scatter<4, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_reference_debug_vector",
    "rs_scatter<4, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_reference_debug_vector",
    "rs_scatter<4, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_pass_intermediates_vs_block_oracle[0-513-4-0-1]",
    "rs_scatter_lines<4, 256, 16, 32, false, 0, 1, 0>": "tests/test_gpu_check.py::test_rank_check_catches_a_broken_lane_order[4-2097157-False-uniform-rs_scatter_lines]",
    "rs_scatter_lines<4, 1024, 16, 32, false, 0, 3, 0>": "tests/test_gpu_fullsize.py::test_fullsize_uniform[268435533-4]",
    "rs_scatter_lines<4, 256, 16, 32, false, 1, 3, 0>": "tests/test_gpu_multi.py::test_c_multi_loopback[8-zipf-False-8-None]",
    "rs_scatter_lines<4, 512, 16, 32, false, 1, 3, 0>": "tests/test_gpu_c5.py::test_c5_full_size_loopback_world8",
    "rs_scatter<4, 256, 16, true, 1, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[1-4]",
    "rs_scatter<4, 256, 16, true, 3, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[2-4]",
    "rs_scatter<4, 256, 16, true, 4, 0, 0>": "tests/test_gpu_multi.py::test_c_multi_loopback[4-uniform-True-4-10000]",
    "rs_scatter_lines<4, 256, 16, 16, true, 1, 2, 0>": "tests/test_gpu_multi.py::test_c_multi_loopback_overlap[4-zipf-True-8-5000]",
    "rs_scatter<5, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-5]",
    "rs_scatter<5, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-5]",
    "rs_scatter<5, 256, 16, false, 4, 0, 0>": "tests/test_gpu_launch_counts.py::test_launch_counts[k5_in_place]",
    "rs_scatter_lines<5, 1024, 16, 32, false, 0, 3, 0>": "tests/test_gpu_parity.py::test_large_tile_geometries[5]",
    "rs_scatter_lines<5, 256, 16, 32, false, 1, 3, 0>": "tests/test_gpu_launch_counts.py::test_launch_counts[partition_17_keys]",
    "rs_scatter_lines<5, 512, 16, 32, false, 1, 3, 0>": "tests/test_gpu_launch_counts.py::test_launch_counts[partition_large_keys]",
    "rs_scatter<5, 256, 16, true, 1, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[1-5]",
    "rs_scatter<5, 256, 16, true, 3, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[2-5]",
    "rs_scatter<5, 256, 16, true, 4, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[0-5]",
    "rs_scatter_lines<5, 1024, 8, 16, true, 0, 2, 0>": "tests/test_gpu_parity.py::test_large_tile_geometries[5]",
    "rs_scatter_lines<5, 256, 16, 16, true, 1, 2, 0>": "tests/test_gpu_launch_counts.py::test_launch_counts[partition_17_pairs]",
    "rs_scatter<6, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-6]",
    "rs_scatter<6, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-6]",
    "rs_scatter<6, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[0-6]",
    "rs_scatter_lines<6, 1024, 16, 32, false, 0, 3, 0>": "tests/test_gpu_parity.py::test_large_tile_geometries[6]",
    "rs_scatter_lines<6, 1024, 8, 16, true, 0, 2, 0>": "tests/test_gpu_check.py::test_rank_check_catches_a_broken_lane_order[6-8388617-True-uniform-rs_scatter_lines]",
    "rs_scatter<7, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-7]",
    "rs_scatter<7, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-7]",
    "rs_scatter<7, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[0-7]",
    "rs_scatter_lines<7, 1024, 16, 32, false, 0, 3, 0>": "tests/test_gpu_parity.py::test_whole_line_scatter[0-uniform]",
    "rs_scatter_pairs<7, 1024, 8, 1>": "tests/test_gpu_parity.py::test_pairs_line_tiles_vs_oracle[uniform-7]",
    "rs_scatter<8, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_reference_default_vector[8]",
    "rs_scatter<8, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-8]",
    "rs_scatter<8, 1024, 16, false, 3, 0, 0>": "tests/test_gpu_fullsize.py::test_fullsize_ballot_ranking_agrees[uniform]",
    "rs_scatter<8, 256, 16, false, 4, 0, 0>": "tests/test_gpu_c5.py::test_c5_full_size_loopback_world8",
    "rs_scatter<8, 1024, 16, false, 4, 0, 0>": "tests/test_gpu_fullsize.py::test_near_2_32_keys_unaligned_output",
    "rs_scatter_lines<8, 1024, 16, 32, false, 0, 3, 0>": "tests/test_gpu_c5.py::test_c5_full_size_loopback_world8",
    "rs_scatter_lines<8, 1024, 16, 32, false, 0, 3, 1>": "tests/test_gpu_c5.py::test_c5_full_size_loopback_world8",
    "rs_scatter<8, 256, 16, true, 1, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[1-8]",
    "rs_scatter<8, 256, 16, true, 3, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[2-8]",
    "rs_scatter<8, 256, 16, true, 4, 0, 0>": "tests/test_gpu_multi.py::test_dist_sort_rccl_single_rank",
    "rs_scatter<8, 1024, 8, true, 4, 0, 0>": "tests/test_gpu_groups.py::test_pairs_mismatched_alignment_falls_back",
    "rs_scatter_pairs<8, 1024, 8, 1>": "tests/test_gpu_check.py::test_rank_check_catches_a_broken_lane_order[8-4194381-True-zipf-rs_scatter_pairs]",
    "rs_scatter<9, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-9]",
    "rs_scatter<9, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-9]",
    "rs_scatter<9, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[0-9]",
    "rs_scatter<10, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-10]",
    "rs_scatter<10, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-10]",
    "rs_scatter<10, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[0-10]",
    "rs_scatter<11, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-11]",
    "rs_scatter<11, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-11]",
    "rs_scatter<11, 256, 16, false, 4, 0, 0>": "tests/test_gpu_check.py::test_rank_check_catches_a_broken_lane_order[11-1048579-False-uniform-rs_scatter]",
    "rs_scatter<12, 256, 16, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-12]",
    "rs_scatter<12, 256, 16, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-12]",
    "rs_scatter<12, 256, 16, false, 4, 0, 0>": "tests/test_gpu_parity.py::test_all_golden_cases",
    "rs_scatter<12, 256, 16, true, 1, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[1-12]",
    "rs_scatter<12, 256, 16, true, 3, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[2-12]",
    "rs_scatter<12, 256, 16, true, 4, 0, 0>": "tests/test_gpu_parity.py::test_pairs_stable_vs_oracle[0-12]",
    "rs_scatter<13, 128, 32, false, 1, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[1-13]",
    "rs_scatter<13, 128, 32, false, 3, 0, 0>": "tests/test_gpu_parity.py::test_sizes_and_bits_vs_oracle[2-13]",
    "rs_scatter<13, 128, 32, false, 4, 0, 0>": "tests/test_gpu_launch_counts.py::test_launch_counts[k13]",
    "rs_scatter<13, 128, 32, true, 4, 0, 0>": "tests/test_gpu_check.py::test_rank_check_catches_a_broken_lane_order[13-1048587-True-uniform-rs_scatter]",
}

NOT_RUN = {
    # the ballot twins of the partition kernels: a partition ranks with RSORT_RANK_MATCH whatever rsort_set_rank_algo says
    "rs_scatter<2, 256, 16, false, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<2, 256, 16, true, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<3, 256, 16, false, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<3, 512, 16, false, 3, 1, 4>": PROBE_FAILS,
    "rs_scatter<3, 256, 16, true, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<4, 256, 16, false, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<4, 512, 16, false, 3, 1, 4>": PROBE_FAILS,
    "rs_scatter<4, 256, 16, true, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<5, 256, 16, false, 3, 1, 0>": PROBE_FAILS,
    "rs_scatter<5, 512, 16, false, 3, 1, 4>": PROBE_FAILS,
    "rs_scatter<5, 256, 16, true, 3, 1, 0>": PROBE_FAILS,
    # lane-ordered rs_scatter on 16384-key line tiles: a keys-only output is line-capable unless its positions, counted
    # from the 128-B boundary below it, pass 2^32 (k = 8: tests/test_gpu_fullsize.py::test_near_2_32_keys_unaligned_output)
    "rs_scatter<4, 1024, 16, false, 4, 0, 0>": BEYOND_2_32,
    "rs_scatter<5, 1024, 16, false, 4, 0, 0>": BEYOND_2_32,
    "rs_scatter<6, 1024, 16, false, 4, 0, 0>": BEYOND_2_32,
    "rs_scatter<7, 1024, 16, false, 4, 0, 0>": BEYOND_2_32,
    # ... and on the 8192-key tiles of keys-only partitions of large inputs; a partition has no local mode, and one of
    # 2^32 - 20 keys has no reference a test could hold: these three are not run at all
    "rs_scatter<3, 512, 16, false, 4, 1, 4>": BEYOND_2_32,
    "rs_scatter<4, 512, 16, false, 4, 1, 4>": BEYOND_2_32,
    "rs_scatter<5, 512, 16, false, 4, 1, 4>": BEYOND_2_32,
}

# (digit mode 0: the sorts' kernels; rs.pass_local_sort runs them)
LOCAL_MODE_ONLY = [n for n, why in NOT_RUN.items() if why == BEYOND_2_32 and int(parse(n)[1][5]) == 0]


@pytest.mark.parametrize("name", SWEEP)
def test_sweep(name):
    launch_and_check(name)


@pytest.mark.parametrize("name", LOCAL_MODE_ONLY)
def test_local_mode_only(name):
    """Lane-ordered rs_scatter on key line tiles sorts only outputs whose positions, counted from the 128-B
    boundary below them, pass 2^32 -- and local passes, which is how these four run here."""
    assert parse(name)[0] == "rs_scatter"
    launch_and_check(name)


def test_every_known_kernel_is_accounted_for():
    known = rs.scatter_kernels_known()
    assert len(known) == len(set(known)) > 100
    assert all(why in NOT_RUN_REASONS for why in NOT_RUN.values())
    assert len(NOT_RUN) <= NOT_RUN_MAX
    assert len(SWEEP) == len(set(SWEEP))
    places = [set(SWEEP), set(COVERED_ELSEWHERE), set(NOT_RUN)]
    for i, a in enumerate(places):
        for b in places[i + 1:]:
            assert not (a & b), sorted(a & b)
    accounted = places[0] | places[1] | places[2]
    assert sorted(set(known) - accounted) == [], "kernels no test launches"
    assert sorted(accounted - set(known)) == [], "rows for kernels the dispatch does not have"
    for name in NOT_RUN:
        if NOT_RUN[name] == PROBE_FAILS:  # the ballot twins of the partition kernels
            kind, a = parse(name)
            assert kind == "rs_scatter" and int(a[4]) == 3 and int(a[5]) == 1, name
    assert rs.lane_order_probe() == 1


# ------------------------------------------------------------------------------ the recording behind COVERED_ELSEWHERE
class _Recorder:
    """pytest plugin: which tests launched which kernel. Tests that read (and reset) the library's record
    themselves go through the same wrapper, so nothing they launched is lost."""

    def __init__(self):
        self.by, self.current = {}, None
        self.real = rs.scatter_kernels_used
        rs.scatter_kernels_used = self.read

    def read(self, reset=False):
        used = self.real(reset=reset)
        for k in used:
            self.by.setdefault(k, [])
            if self.current not in self.by[k]:
                self.by[k].append(self.current)
        return used

    def pytest_runtest_setup(self, item):
        self.real(reset=True)
        self.current = item.nodeid

    def pytest_runtest_teardown(self, item):
        self.read(reset=True)


def _record(out_path, extra):
    """Runs every other GPU test file under the recorder; writes {kernel: first test that launched it} for the
    known kernels and checks COVERED_ELSEWHERE against the run: every entry's test must have launched its kernel.
    Returns pytest's status, or 1 when the table and the recording disagree."""
    here = __file__.rsplit("/", 1)[0]
    rec = _Recorder()
    rc = int(pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider", here, f"--ignore={__file__}", *extra],
                         plugins=[rec]))
    known = rs.scatter_kernels_known()
    wrong = {k: t for k, t in COVERED_ELSEWHERE.items() if t not in rec.by.get(k, [])}
    doc = {"pytest_rc": rc, "covered": {k: rec.by[k][0] for k in known if k in rec.by},
           "not_launched": [k for k in known if k not in rec.by],
           "launched_but_unknown": sorted(set(rec.by) - set(known)),  # (the hybrid route's rs_bucket_sort16)
           "table_entries_not_confirmed": wrong}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"{len(doc['covered'])} of {len(known)} known kernels launched by other tests; "
          f"{len(wrong)} COVERED_ELSEWHERE entries not confirmed -> {out_path}")
    return rc or (1 if wrong else 0)


if __name__ == "__main__":
    i = sys.argv.index("--record")
    sys.exit(_record(sys.argv[i + 1], sys.argv[i + 2:]))
