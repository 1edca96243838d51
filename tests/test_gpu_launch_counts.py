"""Per-route launch counts: what each route of the host driver enqueues, phase by phase (rsort_profile_begin / _end
count one launch per recorded phase scope; of a hybrid-eligible sort, only the scopes of the route that ran).

LAUNCHES was recorded by running this test's body on the commit BEFORE the host driver's pass loop was split by
route (python tests/test_gpu_launch_counts.py on the MI355X box), not on the code under test: a route that lost or
gained an enqueue fails here even when its output is still right. Runs on the MI355X box (-m gpu)."""
import pytest

from _rs import rs
from test_gpu_workspace_state import CASES, poisoned

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = [c for c in CASES if not c.startswith("segmented")]  # the sort and partition cases

# case: launches of (histogram, scan, scatter, copy, partition)
LAUNCHES = {
    "k8_small": (4, 4, 4, 0, 0),
    "k8_lines_no_groups_plan": (4, 4, 4, 0, 0),
    "joint_uniform": (6, 4, 4, 0, 0),  # (histogram: two joint counts, two rs_joint_bounds, two group passes' tables)
    "joint_zipf_cut": (6, 4, 4, 0, 0),
    "joint_groups_off": (4, 4, 4, 0, 0),
    "joint_ballot": (4, 4, 4, 0, 0),
    "joint_pairs": (6, 4, 4, 0, 0),
    "hybrid_run": (3, 1, 3, 0, 0),  # (gate, joint count, rs_hyb_bounds; one scan; passes A, B and the bucket phase)
    "hybrid_overflow": (9, 4, 4, 0, 0),  # (gate, joint count, rs_hyb_bounds, then the six of the LSD passes)
    "hybrid_skewed": (9, 4, 4, 0, 0),
    "k4_raw": (1, 0, 8, 0, 0),
    "k3_raw": (1, 0, 11, 0, 0),
    "k4_raw_1025_chunks": (1, 0, 8, 0, 0),
    "k3_raw_1025_chunks": (1, 0, 11, 0, 0),
    "k4_tail_scan": (1, 1, 8, 0, 0),
    "k3_tail_scan": (1, 1, 11, 0, 0),
    "k5_in_place": (7, 7, 7, 1, 0),
    "k11": (3, 3, 3, 0, 0),
    "k13": (3, 3, 3, 0, 0),
    "partition_17_keys": (1, 1, 0, 0, 1),
    "partition_17_pairs": (1, 1, 0, 0, 1),
    "partition_large_keys": (1, 1, 0, 0, 1),
}


def launches(case):
    nbytes, run, _ = CASES[case]()
    ws = poisoned(nbytes, "a5")
    with rs.Profile() as prof:
        run(ws)  # (checks the output against the oracle too)
    return tuple(prof.times[ph]["launches"] for ph in rs.PHASES)


@pytest.mark.parametrize("case", NAMES)
def test_launch_counts(case):
    got = launches(case)
    print(case, got)
    assert got == LAUNCHES[case], (case, dict(zip(rs.PHASES, got)))


def test_every_case_is_listed():
    assert sorted(LAUNCHES) == sorted(NAMES)


if __name__ == "__main__":
    for c in NAMES:
        print(f'    "{c}": {launches(c)},', flush=True)
