"""GPU: the kernels that judge or feed the sorts and that no sort result depends on -- rs_fingerprint (the output
check of bench.py and of every test above the sizes a host reference fits), rs_sample (the multi-GPU splitter
sample) and the generators' grid-stride loops -- each compared exactly with a host computation of its contract
in include/rsort.h.

The fingerprint is compared with tests/_util.py::fingerprint_ref (pinned on the CPU by tests/test_verifiers.py)
at the sizes around its wave, workgroup and grid edges (8192 workgroups of 256 threads: 2^21 threads, so the
stride loop starts at n = 2^21 + 1), is handed wrong outputs shaped like this code's failure modes -- made by
hand and by the kernels themselves under the rank-fault test hook -- and must report each of them exactly.
Runs on the MI355X box (-m gpu)."""
import functools

import numpy as np
import pytest

from _rs import rs
from _util import fingerprint_ref, oracle_sort, uniform_keys, zipf_cdf_u32, zipf_keys
from test_gpu_check import CASES, _inputs
from test_gpu_hybrid import fat_input, sort_forced

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WRAP = 1 << 21          # threads of the fingerprint's capped grid: element WRAP is thread 0's second
N = WRAP + 257          # the smallest ragged n whose stride loop runs for more than one workgroup's threads
POISON = 0x5A5A5A5A
ERR_ARG, ERR_SIZE = 1, 3


def dev(a):
    return rs.from_numpy_u32(a if a.flags.writeable else a.copy())  # (torch warns about read-only arrays)


def device_fp(keys, vals=None):
    return rs.fingerprint(dev(keys), dev(vals) if vals is not None else None)


def swapped(a, i, j):
    m = a.copy()
    m[i], m[j] = a[j], a[i]
    return m


@functools.lru_cache(maxsize=None)
def sorted_keys():
    """x = the sorted uniform keys every constructed case starts from, and its reference (h, 0). Shared: never
    written (read-only flag set)."""
    x = np.sort(uniform_keys(N, seed=7))
    x.setflags(write=False)
    ref = fingerprint_ref(x)
    assert ref[1] == 0
    return x, ref


def pair_values(n):
    """arange(n) ^ 0x80000001: bit 31 set in every value, so v << 32 must be a 64-bit shift."""
    return np.arange(n, dtype=np.uint32) ^ np.uint32(0x80000001)


# ------------------------------------------------------------------ rs_fingerprint against the reference
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, WRAP - 1, WRAP, N])
def test_fingerprint_matches_reference(n):
    x = uniform_keys(n, seed=1234 + n)
    v = pair_values(n)
    h, desc = fingerprint_ref(x)
    if n >= 255:
        assert 0.4 * n < desc < 0.6 * n     # unsorted: the count is a count, neither a flag nor saturated
    dx, dv = dev(x), dev(v)
    assert rs.fingerprint(dx) == (h, desc)
    assert rs.fingerprint(dx, dv) == fingerprint_ref(x, v)
    s = np.sort(x)
    ds = dev(s)
    assert rs.fingerprint(ds) == (h, 0) == fingerprint_ref(s)
    assert rs.fingerprint(ds, dv) == fingerprint_ref(s, v)
    if n >= 255:  # the values enter h, and which key carries which value does
        assert fingerprint_ref(s, v)[0] != fingerprint_ref(x, v)[0] != h


DESCENT_PAIRS = [(0, 1), (63, 64), (255, 256), (WRAP - 1, WRAP), (N - 2, N - 1)]  # (WRAP - 1, WRAP): the stride wrap


@pytest.mark.parametrize("i,j", DESCENT_PAIRS)
def test_one_descent_is_counted_wherever_it_lies(i, j):
    x, (h, _) = sorted_keys()
    assert x[i] < x[j]
    m = swapped(x, i, j)
    assert fingerprint_ref(m) == (h, 1)
    assert device_fp(m) == (h, 1)


def test_five_descents_are_five():
    x, (h, _) = sorted_keys()
    m = x.copy()
    for i, j in DESCENT_PAIRS:
        m[i], m[j] = x[j], x[i]
    assert fingerprint_ref(m) == (h, 5)
    assert device_fp(m) == (h, 5)


def test_descents_compare_unsigned():
    pair = np.array([0x7FFFFFFF, 0x80000000], dtype=np.uint32)
    assert device_fp(pair) == fingerprint_ref(pair) and fingerprint_ref(pair)[1] == 0
    assert device_fp(pair[::-1]) == fingerprint_ref(pair[::-1]) and fingerprint_ref(pair[::-1])[1] == 1
    # the same pair at the stride wrap: the last thread of the grid and the first thread's second element
    a = np.zeros(N, dtype=np.uint32)
    a[WRAP - 1] = 0x7FFFFFFF
    a[WRAP:] = 0x80000000
    assert fingerprint_ref(a)[1] == 0
    assert device_fp(a) == fingerprint_ref(a)
    b = swapped(a, WRAP - 1, WRAP)
    assert fingerprint_ref(b)[1] == 1
    assert device_fp(b) == fingerprint_ref(b)


def test_c_entry_overwrites_and_checks_its_arguments():
    """rsort_fingerprint_device itself: d_out is overwritten (never added to), n = 0 writes (0, 0), and bad
    arguments are refused before any launch."""
    lib = rs._lib()
    x = uniform_keys(N, seed=99)
    want = fingerprint_ref(x)
    dx = dev(x)
    s = torch.cuda.current_stream().cuda_stream
    out = torch.full((2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    for _ in range(2):
        assert lib.rsort_fingerprint_device(dx.data_ptr(), None, N, out.data_ptr(), s) == 0
        h, d = out.cpu().tolist()
        assert (h & 0xFFFFFFFFFFFFFFFF, d) == want
    assert lib.rsort_fingerprint_device(dx.data_ptr(), None, 0, out.data_ptr(), s) == 0
    assert out.cpu().tolist() == [0, 0]
    out.fill_(0x5A5A5A5A5A5A5A5A)
    assert lib.rsort_fingerprint_device(None, None, 0, out.data_ptr(), s) == 0
    assert out.cpu().tolist() == [0, 0]
    out.fill_(7)
    assert lib.rsort_fingerprint_device(dx.data_ptr(), None, -1, out.data_ptr(), s) == ERR_SIZE
    assert lib.rsort_fingerprint_device(dx.data_ptr(), None, 1 << 32, out.data_ptr(), s) == ERR_SIZE
    assert lib.rsort_fingerprint_device(dx.data_ptr(), None, N, None, s) == ERR_ARG
    assert lib.rsort_fingerprint_device(None, None, N, out.data_ptr(), s) == ERR_ARG
    assert out.cpu().tolist() == [7, 7]  # a refused call writes nothing


@functools.lru_cache(maxsize=None)
def _stream_case():
    n = (1 << 23) + 77
    x = uniform_keys(n, seed=31)
    return x, fingerprint_ref(oracle_sort(x, 8))


def test_stream_order_on_the_current_stream():
    """Sort, then fingerprint, on a side stream with no synchronisation in between."""
    x, want = _stream_case()
    assert want[1] == 0
    side = torch.cuda.Stream()
    d_in = dev(x)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d_out = rs.empty_u32(x.size)
        rs.sort_device(d_in, d_out, 8)
        got = rs.fingerprint(d_out)
    assert got == want
    side.synchronize()


def test_stream_order_on_an_explicit_stream():
    """rs.fingerprint(stream=side) while torch's current stream is another one: its result buffer and its read
    of the result belong to `side` too, behind the sort that runs there."""
    x, want = _stream_case()
    side = torch.cuda.Stream()
    assert side != torch.cuda.current_stream()
    d_in, d_out = dev(x), rs.empty_u32(x.size)
    p = rs.plan(x.size, 8)
    ws = rs.workspace(p.workspace_bytes)
    side.wait_stream(torch.cuda.current_stream())
    rs.sort_device(d_in, d_out, 8, ws=ws, plan_=p, stream=side)
    got = rs.fingerprint(d_out, stream=side)
    assert got == want
    side.synchronize()
    assert rs.fingerprint(d_in, stream=side) == fingerprint_ref(x)


# ------------------------------------------------------------------ the fingerprint notices wrong outputs
LINE = 32        # keys of one 128-B line, the unit the line scatter kernels write
L = 4097         # a line inside the array, off every 256-key edge's start
EDGE = 256 * 4097


def _low_bit(x):
    m = x.copy()
    m[1000] ^= 1
    return m


def _top_bit_of_last(x):
    m = x.copy()
    m[-1] ^= 0x80000000
    return m


def _overwritten_by_neighbour(x):
    assert x[5000] != x[5001]
    m = x.copy()
    m[5000] = x[5001]
    return m


def _line_left_zero(x):
    m = x.copy()
    m[LINE * L:LINE * (L + 1)] = 0
    return m


def _line_written_twice(x):
    m = x.copy()
    m[LINE * L:LINE * (L + 1)] = x[LINE * (L - 1):LINE * L]
    return m


def _plus_one_minus_one(x):
    assert x[10] < 0xFFFFFFFF and x[20] > 0
    m = x.copy()
    m[10] += 1
    m[20] -= 1
    assert int(m.sum(dtype=np.uint64)) == int(x.sum(dtype=np.uint64))  # a plain sum cancels
    return m


# name -> (mutation of the sorted keys, the component of the fingerprint it must change)
KEY_FAULTS = {
    "one low bit flipped": (_low_bit, "h"),
    "top bit of the last key flipped": (_top_bit_of_last, "h"),
    "a key overwritten by its neighbour": (_overwritten_by_neighbour, "h"),
    "a 32-key line left zero": (_line_left_zero, "h"),
    "a 32-key line written twice": (_line_written_twice, "h"),
    "two keys exchanged across the stride wrap": (lambda x: swapped(x, WRAP - 1, WRAP), "descents"),
    "two keys exchanged across a 256-key edge": (lambda x: swapped(x, EDGE - 1, EDGE), "descents"),
    "the last two keys exchanged": (lambda x: swapped(x, N - 2, N - 1), "descents"),
    "+1 on one key, -1 on another": (_plus_one_minus_one, "h"),
}


@pytest.mark.parametrize("name", list(KEY_FAULTS))
def test_fingerprint_notices_a_wrong_key_output(name):
    x, good = sorted_keys()
    mutate, component = KEY_FAULTS[name]
    m = mutate(x)
    assert m.shape == x.shape and not np.array_equal(m, x)
    ref = fingerprint_ref(m)
    # the premise, on the CPU: the reference itself tells the mutant from the sorted output
    assert ref != good
    if component == "h":
        assert ref[0] != good[0]
    else:
        assert ref[0] == good[0] and ref[1] != good[1]
    assert device_fp(m) == ref


def test_fingerprint_notices_wrong_values():
    """Pairs: values that moved to another key, or changed, change h. The documented limit: exchanging the
    values of two EQUAL keys changes neither component -- the fingerprint does not check stability. Stability
    is checked by the pairs comparisons with the oracle (tests/test_gpu_parity.py, tests/test_gpu_check.py,
    tests/test_gpu_fullsize.py::test_fullsize_pairs_zipf_vs_oracle) and by the increasing values within runs
    of equal keys in tests/test_gpu_fullsize.py::test_fullsize_pairs_zipf."""
    x, _ = sorted_keys()
    v = pair_values(N)
    good = fingerprint_ref(x, v)
    dx = dev(x)
    assert rs.fingerprint(dx, dev(v)) == good
    i, j = 777, WRAP + 5
    assert x[i] != x[j]
    faults = {"the values of two different keys exchanged": swapped(v, i, j)}
    m = v.copy()
    m[N - 1] ^= 0x80000000
    faults["one value changed"] = m
    for name, m in faults.items():
        ref = fingerprint_ref(x, m)
        assert ref[0] != good[0] and ref[1] == 0, name
        assert rs.fingerprint(dx, dev(m)) == ref, name
    eq = np.flatnonzero(x[:-1] == x[1:])
    assert eq.size > 0  # 2^21 uniform keys: about 500 adjacent equal pairs
    e = int(eq[0])
    m = swapped(v, e, e + 1)
    assert not np.array_equal(m, v)
    assert fingerprint_ref(x, m) == good
    assert rs.fingerprint(dx, dev(m)) == good


# ------------------------------------------------------------------ wrong outputs made by the kernels themselves
KEYS_ONLY_CASES = [c for c in CASES if not c[2]]
assert [(c[0], c[3]) for c in KEYS_ONLY_CASES] == [(8, "uniform"), (8, "zipf"), (4, "uniform"), (11, "uniform")]


@pytest.mark.parametrize("k,n,pairs,dist,family", KEYS_ONLY_CASES)
def test_fingerprint_counts_the_descents_of_a_rank_faulted_sort(k, n, pairs, dist, family):
    """The rank-fault test hook makes the scatter kernels write a permutation of the input that is not the
    sorted one (tests/test_gpu_check.py asserts that it differs): it has a descent, and the fingerprint must
    report the input's h with exactly the descents numpy counts."""
    x, _ = _inputs(n, pairs, dist, k)
    d_in, d_out = dev(x), rs.empty_u32(n)
    fp_in = rs.fingerprint(d_in)[0]
    assert fp_in == fingerprint_ref(x)[0]
    p = rs.plan(n, k)
    ws = rs.workspace(p.workspace_bytes)
    with rs.rank_fault():
        rs.sort_device(d_in, d_out, k, ws=ws, plan_=p)
        assert rs.plan_check(p, ws) & rs.CHECK_RANK_ORDER
    y = rs.to_numpy_u32(d_out)
    desc = int(np.count_nonzero(y[:-1] > y[1:]))
    assert desc >= 1
    assert rs.fingerprint(d_out) == (fp_in, desc)
    rs.sort_device(d_in, d_out, k, ws=ws, plan_=p)
    assert rs.fingerprint(d_out) == (fp_in, 0)


def test_fingerprint_counts_the_descents_of_a_rank_faulted_hybrid_sort():
    x, want = fat_input()
    fp_in = fingerprint_ref(x)[0]
    with rs.rank_fault():
        y, rep, chk = sort_forced(x)
    assert rep["hybrid"] and chk & rs.CHECK_RANK_ORDER
    if np.array_equal(y, want):
        pytest.fail("the rank fault left the hybrid route's output equal to the oracle's: this case proves nothing")
    desc = int(np.count_nonzero(y[:-1] > y[1:]))
    assert desc >= 1
    assert device_fp(y) == (fp_in, desc)
    y, rep, chk = sort_forced(x)
    assert rep["hybrid"] and chk == 0
    assert device_fp(y) == (fp_in, 0)


# ------------------------------------------------------------------ rs_sample against numpy
def sample_ref(keys, stride, count, row_len):
    """include/rsort.h: out[j] = keys[min(n - 1, j * stride + stride // 2)] for j < count, 0xFFFFFFFF up to row_len."""
    out = np.full(row_len, 0xFFFFFFFF, dtype=np.uint32)
    if count and keys.size:
        j = np.arange(count, dtype=np.int64)
        out[:count] = keys[np.minimum(keys.size - 1, j * stride + stride // 2)]
    return out


NS_ = 300001
SAMPLE_CASES = [
    # (n, stride, count, row_len, whether the last samples clamp to n - 1)
    (NS_, 1, NS_, NS_, False),                        # every key, count == row_len
    (NS_, 1, 1000, 1024, False),
    (NS_, 7, NS_ // 7, NS_ // 7, False),              # count == row_len
    (NS_, 7, NS_ // 7, NS_ // 7 + 100, False),        # count < row_len
    (NS_, 7, NS_ // 7 + 9, NS_ // 7 + 300, True),
    (NS_, 7, 0, 300, False),                          # count = 0: all padding
    (NS_, 4096, NS_ // 4096, 256, False),
    (NS_, 4096, NS_ // 4096 + 7, 257, True),          # row_len one past a workgroup
    (NS_, 4096, 1, 1, False),
    (0, 7, 0, 300, False),                            # n = 0: all padding
    (0, 7, 100, 300, False),
    (1 << 21, 2, 1 << 20, (1 << 20) + 300, False),    # row_len above the grid's 4096 x 256 threads: the stride loop
]


@functools.lru_cache(maxsize=None)
def sample_keys(n):
    return uniform_keys(n, seed=4242)


@pytest.mark.parametrize("n,stride,count,row_len,clamps", SAMPLE_CASES)
def test_sample_matches_numpy(n, stride, count, row_len, clamps):
    x = sample_keys(n)
    want = sample_ref(x, stride, count, row_len)
    if count and n:  # the case's own claim about clamping, checked before the GPU is asked
        assert bool((np.arange(count) * stride + stride // 2 > n - 1).any()) == clamps
    guard = 64
    buf = torch.full((row_len + guard,), POISON, dtype=torch.int32, device="cuda")
    rs.sample_device(dev(x) if n else rs.empty_u32(0), stride, count, row_len, out=buf[:row_len])
    got = rs.to_numpy_u32(buf)
    assert np.array_equal(got[:row_len], want)
    assert (got[row_len:] == POISON).all()


def test_sample_argument_errors():
    lib = rs._lib()
    d = dev(sample_keys(NS_))
    out = torch.full((64,), POISON, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lib.rsort_sample_device
    assert call(d.data_ptr(), NS_, 0, 8, 64, out.data_ptr(), s) == ERR_ARG      # stride = 0
    assert call(d.data_ptr(), NS_, 7, 65, 64, out.data_ptr(), s) == ERR_ARG     # row_len < count
    assert call(d.data_ptr(), 1 << 32, 7, 8, 64, out.data_ptr(), s) == ERR_SIZE
    assert call(d.data_ptr(), -1, 7, 8, 64, out.data_ptr(), s) == ERR_SIZE
    assert call(d.data_ptr(), NS_, 7, 8, 64, None, s) == ERR_ARG
    torch.cuda.synchronize()
    assert (rs.to_numpy_u32(out) == POISON).all()  # a refused call writes nothing


# ------------------------------------------------------------------ the generators in their stride loop
GEN_N = (1 << 24) + 259      # the generators' grid is capped at 65536 x 256 = 2^24 threads
GEN_WINDOWS = [(0, 4096), ((1 << 24) - 4096, GEN_N), (GEN_N - 300, GEN_N)]
# a plain seed, and one 2048 below 2^32: seed + i crosses 2^32 inside the first window, and a 32-bit sum wraps
GEN_SEEDS = [0xC0FFEE, (1 << 32) - 2048]


@pytest.mark.parametrize("seed", GEN_SEEDS)
@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_generator_stride_loop_matches_host_slices(dist, seed):
    d = torch.full((GEN_N + 64,), POISON, dtype=torch.int32, device="cuda")
    if dist == "uniform":
        rs.gen_uniform(d[:GEN_N], seed)
        host = uniform_keys
    else:
        rs.gen_zipf(d[:GEN_N], dev(zipf_cdf_u32()), seed)
        host = zipf_keys
    torch.cuda.synchronize()
    for a, b in GEN_WINDOWS:
        assert np.array_equal(rs.to_numpy_u32(d[a:b]), host(b - a, seed + a)), (a, b)
    assert (rs.to_numpy_u32(d[GEN_N:]) == POISON).all()


def test_iota_stride_loop_wraps():
    base = 0xFFFFFF00  # base + i wraps to 0 at i = 256
    d = torch.full((GEN_N + 64,), POISON, dtype=torch.int32, device="cuda")
    rs.gen_iota(d[:GEN_N], base)
    torch.cuda.synchronize()
    for a, b in GEN_WINDOWS:
        want = ((np.arange(a, b, dtype=np.uint64) + np.uint64(base)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        assert np.array_equal(rs.to_numpy_u32(d[a:b]), want), (a, b)
    assert rs.to_numpy_u32(d[255:258]).tolist() == [0xFFFFFFFF, 0, 1]
    assert (rs.to_numpy_u32(d[GEN_N:]) == POISON).all()
