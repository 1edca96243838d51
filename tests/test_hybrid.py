"""The hybrid route's host-side contract (rsort_set_hybrid, rsort_hybrid_capacity, rsort_hybrid_range,
rsort_hybrid_gate_threshold): what can be checked without a device."""
import math

import pytest

from _rs import rs


def test_setters_round_trip():
    assert rs.get_hybrid() == rs.HYBRID_AUTO
    for mode in (rs.HYBRID_OFF, rs.HYBRID_FORCE, rs.HYBRID_AUTO):
        rs.set_hybrid(mode)
        assert rs.get_hybrid() == mode
    with rs.hybrid(rs.HYBRID_FORCE):
        assert rs.get_hybrid() == rs.HYBRID_FORCE
    assert rs.get_hybrid() == rs.HYBRID_AUTO
    with pytest.raises(rs.RSortError):
        rs.set_hybrid(3)
    assert rs.get_hybrid() == rs.HYBRID_AUTO


def test_capacity_and_range():
    cap = rs.hybrid_capacity()
    assert cap >= 18 * 1024 and cap >= 16919  # the largest bucket of the uniform 2^30-key input
    lo, hi = rs.hybrid_range()
    # the digit-group tests pin the LSD passes at 2^27 keys; the upper end is a mean bucket at the capacity
    assert (1 << 27) < lo <= (1 << 30) <= hi == cap * 65536


def poisson_tail(lam, t):
    """P(Poisson(lam) >= t), summed from the tail's first term (no cancellation)."""
    lp = -lam + t * math.log(lam) - math.lgamma(t + 1)
    term, s, k = math.exp(lp), 0.0, t
    while term > 1e-300 and (k < 4 * lam + 64):
        s += term
        k += 1
        term *= lam / k
    return s


@pytest.mark.parametrize("n", [1 << 22, 512 * 16384 - 5, 1 << 28, 1 << 29, 1 << 30, 18432 * 65536])
def test_gate_threshold_is_out_of_a_uniform_samples_reach(n):
    """Each of the gate's 64 workgroups counts m = min(n, 65536) / 64 strided keys by their top 16 bits. A bucket
    within the capacity holds at most Poisson(m * capacity / n) of them (uniform keys: Poisson(m / 65536), less):
    over 65536 buckets and 64 workgroups the threshold is reached less than once in 1e9 sorts, and it is the
    smallest such count. It stays far below what Zipf's most common key (7 % of the keys) or a hot key (25 %) puts
    into one bucket."""
    t = rs.hybrid_gate_threshold(n)
    m = min(n, 65536) / 64
    trials = 65536 * 64
    lam = m * max(1 / 65536, rs.hybrid_capacity() / n)
    assert trials * poisson_tail(lam, t) < 1e-9
    assert trials * poisson_tail(lam, t - 2) > 1e-9  # (the library bounds the tail from above: at most one count of slack)
    assert trials * poisson_tail(m / 65536, t) < 1e-9
    assert t < 0.07 * m / 2


def test_no_plan_feature_bit():
    """The route is a per-call decision, not a plan feature (rsort_plan_features pins the plans' bits)."""
    assert rs.hybrid_gate_threshold(1 << 30) in range(5, 10)
    with pytest.raises(rs.RSortError):
        rs.hybrid_gate_threshold(0)
