"""CPU: the host reference of the output check (tests/_util.py::fingerprint_ref), which the GPU tests of
rsort_fingerprint_device compare the kernel with (tests/test_gpu_verifiers.py). The vectorised numpy version
is checked here against the formula of include/rsort.h "output check" restated with plain Python integers."""
import numpy as np

from _util import fingerprint_ref, uniform_keys

M64 = (1 << 64) - 1


def fmix64_int(k: int) -> int:
    k ^= k >> 33
    k = k * 0xFF51AFD7ED558CCD & M64
    k ^= k >> 33
    k = k * 0xC4CEB9FE1A85EC53 & M64
    k ^= k >> 33
    return k


def fingerprint_int(keys, vals=None):
    keys = [int(k) for k in keys]
    vals = [0] * len(keys) if vals is None else [int(v) for v in vals]
    h = sum(fmix64_int(v << 32 | k) for k, v in zip(keys, vals)) & M64
    return h, sum(1 for a, b in zip(keys, keys[1:]) if a > b)


def test_fmix64_int_known_values():
    """The plain restatement itself: fmix64 is a bijection with fmix64(0) = 0, and MurmurHash3's published
    finalizer maps 1 to 0xB456BCFC34C2CB2C."""
    assert fmix64_int(0) == 0
    assert fmix64_int(1) == 0xB456BCFC34C2CB2C


def test_fingerprint_ref_matches_plain_integers():
    n = 1000
    edge = np.array([0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x80000001, 1, 0xFFFFFFFE, 0], dtype=np.uint32)
    keys = uniform_keys(n, seed=11)
    vals = uniform_keys(n, seed=12)
    keys[:edge.size] = edge            # 0x7FFFFFFF, 0x80000001: an ascent a signed compare takes for a descent
    vals[:edge.size] = edge[::-1]
    vals[edge.size:2 * edge.size] = edge
    assert (keys >> 31).sum() > n // 4 and (vals >> 31).sum() > n // 4  # bit 31 set in many keys and values
    want = fingerprint_int(keys, vals)
    assert 400 < want[1] < 600         # about n / 2 descents: a count, not a flag
    assert fingerprint_ref(keys, vals) == want
    assert fingerprint_ref(keys) == fingerprint_int(keys)
    assert fingerprint_ref(keys)[0] != want[0] and fingerprint_ref(keys)[1] == want[1]
    s = np.sort(keys)
    assert fingerprint_ref(s) == (fingerprint_int(keys)[0], 0)   # order-independent sum, no descent
    assert fingerprint_ref(s[::-1])[1] == fingerprint_int(s[::-1])[1] == np.unique(s).size - 1


def test_fingerprint_ref_unsigned_order():
    pair = np.array([0x7FFFFFFF, 0x80000000], dtype=np.uint32)
    assert fingerprint_ref(pair)[1] == 0
    assert fingerprint_ref(pair[::-1])[1] == 1


def test_fingerprint_ref_empty_and_single():
    empty = np.zeros(0, dtype=np.uint32)
    assert fingerprint_ref(empty) == (0, 0)
    assert fingerprint_ref(empty, empty) == (0, 0)
    for k in (0, 1, 0x80000000, 0xFFFFFFFF):
        one = np.array([k], dtype=np.uint32)
        assert fingerprint_ref(one) == (fmix64_int(k), 0)
        assert fingerprint_ref(one, np.array([0xFFFFFFFF], dtype=np.uint32)) == (fmix64_int(0xFFFFFFFF << 32 | k), 0)
