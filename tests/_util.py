"""Shared test helpers: oracle loaders, synthetic workloads, digests.

The oracle (``oracle/liboracle.so``) and the reference build (``oracle/_ref/libref.so``) are
TEST INFRASTRUCTURE: only tests/, ``__graft_entry__.smoke()`` and ``bench.py``'s cpu_baseline
leg load them. The product path is ``cuda.radixsort_amd`` (HIP) and never imports this file.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_DIR = ROOT / "oracle"
GOLDEN_DIR = ROOT / "tests" / "golden"

_u32p = ctypes.POINTER(ctypes.c_uint32)


def _ptr(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_u32p)


_ORACLE = None


def oracle() -> ctypes.CDLL:
    """liboracle.so (CPU restatement of Baseline1/Baseline4); built on first use."""
    global _ORACLE
    if _ORACLE is None:
        so = ORACLE_DIR / "liboracle.so"
        src = ORACLE_DIR / "rsort_oracle.c"
        if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
            subprocess.run(["make", "-s", "-C", str(ORACLE_DIR), "liboracle.so"], check=True)
        lib = ctypes.CDLL(str(so))
        i64, c_int = ctypes.c_int64, ctypes.c_int
        lib.oracle_sort_by_host.argtypes = [_u32p, i64, _u32p, c_int]
        lib.oracle_sort_pairs_by_host.argtypes = [_u32p, _u32p, i64, _u32p, _u32p, c_int]
        lib.oracle_block_pass.argtypes = [_u32p, i64, c_int, c_int, i64, i64, _u32p, _u32p, _u32p, _u32p]
        lib.oracle_block_sort.argtypes = [_u32p, i64, _u32p, c_int, i64]
        lib.oracle_fnv1a64.argtypes = [_u32p, i64]
        lib.oracle_fnv1a64.restype = ctypes.c_uint64
        lib.oracle_fill_rand.argtypes = [_u32p, i64, c_int]
        _ORACLE = lib
    return _ORACLE


def ref_lib():
    """oracle/_ref/libref.so: the reference's own sortByHost / Baseline4 sort, or None."""
    so = ORACLE_DIR / "_ref" / "libref.so"
    if not so.exists():
        if Path("/root/reference/SourceCode").is_dir():
            subprocess.run(["bash", str(ORACLE_DIR / "build_ref.sh")], check=True,
                           stdout=subprocess.DEVNULL)
        if not so.exists():
            return None
    lib = ctypes.CDLL(str(so))
    lib.ref_sort_by_host.argtypes = [_u32p, ctypes.c_int, _u32p, ctypes.c_int]
    lib.ref_block_sort.argtypes = [_u32p, ctypes.c_int, _u32p, ctypes.c_int, ctypes.c_int]
    return lib


# ----------------------------------------------------------------------------- oracle calls
def oracle_sort(keys: np.ndarray, nbits: int) -> np.ndarray:
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.empty_like(keys)
    assert oracle().oracle_sort_by_host(_ptr(keys), keys.size, _ptr(out), nbits) == 0
    return out


def oracle_sort_pairs(keys: np.ndarray, vals: np.ndarray, nbits: int):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.uint32)
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    assert oracle().oracle_sort_pairs_by_host(_ptr(keys), _ptr(vals), keys.size, _ptr(ko), _ptr(vo), nbits) == 0
    return ko, vo


def oracle_block_pass(keys: np.ndarray, nbits: int, bit: int, tile: int, chunk: int):
    """Per-pass intermediates of Baseline4: (hist_cm, scan_cm, local, out)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = keys.size
    nchunks = (n - 1) // chunk + 1
    h = np.empty((1 << nbits) * nchunks, np.uint32)
    s = np.empty_like(h)
    loc = np.empty_like(keys)
    out = np.empty_like(keys)
    rc = oracle().oracle_block_pass(_ptr(keys), n, nbits, bit, tile, chunk, _ptr(h), _ptr(s), _ptr(loc), _ptr(out))
    assert rc == 0
    return h, s, loc, out


def fnv1a64(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return "%016x" % oracle().oracle_fnv1a64(_ptr(a), a.size)


def glibc_rand(n: int, debug: bool = False) -> np.ndarray:
    """The reference's own input stream: glibc rand(), default seed (Parallel7.cu:717-723)."""
    a = np.empty(n, np.uint32)
    oracle().oracle_fill_rand(_ptr(a), n, 1 if debug else 0)
    return a


# ----------------------------------------------------------------------------- workloads
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform_keys(n: int, seed: int = 0x5EED) -> np.ndarray:
    """key[i] = high 32 bits of splitmix64(seed + i)  (SURVEY §8d); == rsort_gen_uniform."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    return (splitmix64(i) >> np.uint64(32)).astype(np.uint32)


def fmix32(h: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        h = h.astype(np.uint32)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
        return h


def zipf_cdf_u32(ranks: int = 1 << 20, s: float = 1.0) -> np.ndarray:
    """Inclusive CDF of Zipf(s) over `ranks`, scaled to u32 thresholds (last = 2^32-1)."""
    w = 1.0 / np.arange(1, ranks + 1, dtype=np.float64) ** s
    c = np.cumsum(w)
    c /= c[-1]
    t = np.floor(c * 4294967296.0)
    t = np.minimum(t, 4294967295.0)
    t[-1] = 4294967295.0
    return t.astype(np.uint32)


def zipf_keys(n: int, seed: int = 0x5EED, ranks: int = 1 << 20, s: float = 1.0) -> np.ndarray:
    """key = fmix32(rank), rank ~ Zipf(s) by inverse CDF of u = uniform_keys (== rsort_gen_zipf)."""
    u = uniform_keys(n, seed)
    cdf = zipf_cdf_u32(ranks, s)
    rank = np.searchsorted(cdf, u, side="left")  # first r with u <= cdf[r]
    rank = np.minimum(rank, ranks - 1).astype(np.uint32)
    return fmix32(rank)


# ----------------------------------------------------------------------------- output check
def fmix64(k: np.ndarray) -> np.ndarray:
    """MurmurHash3's 64-bit finalizer over a uint64 array."""
    with np.errstate(over="ignore"):
        k = k.astype(np.uint64)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
        return k


def fingerprint_ref(keys: np.ndarray, vals: np.ndarray | None = None) -> tuple[int, int]:
    """Host statement of include/rsort.h "output check" (rsort_fingerprint_device): (h, descents) with
    h = sum of fmix64(v << 32 | k) mod 2^64 (v = 0 without values) and descents = #{i : k[i] > k[i + 1]},
    the keys compared as unsigned 32-bit numbers."""
    k = np.ascontiguousarray(keys, dtype=np.uint32).astype(np.uint64)
    word = k
    if vals is not None:
        v = np.ascontiguousarray(vals, dtype=np.uint32).astype(np.uint64)
        assert v.size == k.size
        word = (v << np.uint64(32)) | k
    h = int(np.sum(fmix64(word), dtype=np.uint64))  # integer array sums wrap: the sum mod 2^64
    descents = int(np.count_nonzero(k[:-1] > k[1:]))
    return h, descents


# ----------------------------------------------------------------------------- top-k of a periodic input
def periodic_topk_tables(base: np.ndarray, n: int, largest: bool) -> dict:
    """The input x[i] = base[i % P] (P = base.size, i < n) by the distinct values of base ^ m, ascending (m = 0xFFFFFFFF
    for the k largest, else 0) -- int64 arrays, one entry per distinct value ("group") unless said otherwise:
    gx the value, gsize its base positions, goff where they start in ps, gcount its copies in x (a base position p has
    (n - 1 - p) // P + 1 of them, none at p >= n), gstart / gend the copies before it / through it; ps (P entries): the
    base positions by (value, position); copies (P entries): the copies by base position. Never touches n elements."""
    base = np.ascontiguousarray(base, dtype=np.uint32)
    P, n = int(base.size), int(n)
    assert P >= 1 and 0 <= n < (1 << 32)
    m = np.uint32(0xFFFFFFFF if largest else 0)
    xb = base ^ m
    p = np.arange(P, dtype=np.int64)
    copies = np.where(p < n, (n - 1 - p) // P + 1, 0).astype(np.int64)
    ps = np.argsort(xb, kind="stable").astype(np.int64)  # by (value, position)
    xs = xb[ps]
    goff = np.flatnonzero(np.r_[True, xs[1:] != xs[:-1]]).astype(np.int64)
    gcount = np.add.reduceat(copies[ps], goff).astype(np.int64)
    gend = np.cumsum(gcount)
    return {"P": P, "n": n, "m": int(m), "xb": xb, "copies": copies, "ps": ps, "gx": xs[goff].astype(np.int64),
            "goff": goff, "gsize": np.diff(np.r_[goff, P]).astype(np.int64), "gcount": gcount, "gstart": gend - gcount,
            "gend": gend}


PERIODIC_POSITION_TABLES = ("gend", "gstart", "gsize", "goff", "ps")  # what periodic_topk_positions reads, with "P"


def periodic_topk_positions(tab: dict, ranks):
    """(positions, groups) of the entries at `ranks` (int64, each < n) of the stable ascending order of x ^ m. A
    value's base positions ps (ascending) stand in x at ps + P t: ordered by (t, p) and cut at n, its r-th copy is
    ps[r % |ps|] + P (r // |ps|) -- every t below n // P has all of ps, the last one a prefix of it. Written once for
    numpy arrays and for torch tensors (tab's PERIODIC_POSITION_TABLES then tensors on ranks' device): a k too large
    for the host is expanded on the device in pieces by the same lines."""
    if isinstance(ranks, np.ndarray):
        g = np.searchsorted(tab["gend"], ranks, side="right")  # (a value without a copy, n < P, holds no rank)
    else:
        import torch
        g = torch.searchsorted(tab["gend"], ranks, right=True)
    r = ranks - tab["gstart"][g]
    size = tab["gsize"][g]
    return tab["ps"][tab["goff"][g] + r % size] + tab["P"] * (r // size), g


def periodic_topk_expected(base: np.ndarray, n: int, k: int, largest: bool):
    """The top-k contract for x[i] = base[i % P], i < n, in closed form: (keys, positions) of the first k entries of
    the stable ascending order of x ^ m; keys uint32, positions int64 (they pass 2^31)."""
    tab = periodic_topk_tables(base, n, largest)
    assert 0 <= k <= tab["n"]
    pos, g = periodic_topk_positions(tab, np.arange(k, dtype=np.int64))
    return (tab["gx"][g] ^ tab["m"]).astype(np.uint32), pos


def periodic_topk_report(base: np.ndarray, n: int, k: int, largest: bool) -> dict:
    """rs.topk_report's fields on the SELECT route for the same input, from base and the copy counts alone."""
    tab = periodic_topk_tables(base, n, largest)
    assert 1 <= k <= tab["n"]
    g = int(np.searchsorted(tab["gend"], k - 1, side="right"))
    t = int(tab["gx"][g])
    before = int(tab["gstart"][g])
    top = (tab["xb"] >> np.uint32(24)) == np.uint32(t >> 24)
    return {"kth_key": t ^ tab["m"], "before": before, "equal_taken": k - before,
            "equal_in_input": int(tab["gcount"][g]), "candidates": int(tab["copies"][top].sum())}


# ----------------------------------------------------------------------------- row-wise top-k: the select's exits
TOPK_ROWS_CLASS_COLS = {0: 100, 1: 600, 2: 5000, 3: 20000}  # one row length inside each kernel class (wave .. stream)


def select_exit_level(x_row: np.ndarray, k: int) -> int:
    """The control flow of the row-wise select's four-level loop (csrc/rsort_topk_rows.hip) for a row of x = key ^ m:
    per level the candidates' 8-bit digits are counted, the digit holding the krem-th is picked, rem = krem - (the
    entries below it), and the loop stops with that level when the digit holds exactly rem. 0..3, or 4: ran through."""
    cand, krem = np.ascontiguousarray(x_row, dtype=np.uint32), int(k)
    assert 1 <= krem <= cand.size
    for level in range(4):
        digit = (cand >> np.uint32(24 - 8 * level)) & np.uint32(255)
        cnt = np.bincount(digit, minlength=256)
        cum = np.cumsum(cnt)
        d = int(np.searchsorted(cum, krem, side="left"))  # the first digit with cum >= krem
        rem = krem - int(cum[d] - cnt[d])
        if int(cnt[d]) == rem:
            return level
        cand, krem = cand[digit == d], rem
    return 4


def byte_row(cols: int, level: int, seed: int) -> np.ndarray:
    """A row in which only the byte of one select level varies (bits 24 - 8 level and the 7 above), over 16 digit
    values in a seeded order, each held by cols // 16 entries or one more (cols >= 32: at least two); the other three
    bytes are constants. k at a cumulative digit count then ends the select at that level, one more runs through all
    four levels (the next digit holds more than the one entry wanted and no lower byte separates), k = cols ends at
    level 0; the same in x = key ^ 0xFFFFFFFF, where the digits' order turns round."""
    assert cols >= 32 and 0 <= level <= 3
    sh = np.uint32(24 - 8 * level)
    which = np.argsort(uniform_keys(cols, seed=seed), kind="stable") % 16  # a seeded permutation: balanced counts
    digit = (np.uint32(9) + np.uint32(15) * which.astype(np.uint32)) << sh  # 9, 24, .. 234
    return (np.uint32(0x5AC3A53C) & ~(np.uint32(255) << sh)) | digit


def digit_boundaries(x_row: np.ndarray, level: int) -> np.ndarray:
    """The cumulative counts of the level's digits of x_row, ascending: the ks at which a byte_row's select stops."""
    x = np.ascontiguousarray(x_row, dtype=np.uint32)
    cnt = np.bincount((x >> np.uint32(24 - 8 * level)) & np.uint32(255), minlength=256)
    return np.cumsum(cnt[cnt > 0])


def env_flag(name: str) -> bool:
    return os.environ.get(name, "") not in ("", "0", "false", "False")
