"""The track queue's schedule (include/umx_hip.h, umx_hip_queue_plan) against a restatement of its definition: before
each call every lane without a track takes the next job, in ascending lane order; a job of S segments holds its lane for S
consecutive calls; the run ends when no lane holds a track.  Host arithmetic: no GPU."""
import numpy as np
import pytest


def plan_ref(lanes, counts):
    left, lane_of, first, j, call = [0] * lanes, [], [], 0, 0
    while True:
        for ln in range(lanes):
            if left[ln] == 0 and j < len(counts):
                lane_of.append(ln)
                first.append(call)
                left[ln] = counts[j]
                j += 1
        if not any(left):
            return lane_of, first, call
        left = [max(0, x - 1) for x in left]
        call += 1


COUNTS = [1, 5, 2, 2, 3, 1, 4]


def test_the_example_of_the_header(pkg):
    assert pkg.queue_plan(3, COUNTS) == ([0, 1, 2, 0, 2, 0, 0], [0, 0, 0, 1, 2, 3, 4], 8)
    assert plan_ref(3, COUNTS) == ([0, 1, 2, 0, 2, 0, 0], [0, 0, 0, 1, 2, 3, 4], 8)
    # pass by pass, in groups of three in list order, the same tracks cost 5 + 3 + 4 calls
    assert sum(max(COUNTS[i:i + 3]) for i in range(0, len(COUNTS), 3)) == 12


def test_one_lane_is_the_sum_and_enough_lanes_the_maximum(pkg):
    lane, first, calls = pkg.queue_plan(1, COUNTS)
    assert calls == sum(COUNTS) and lane == [0] * 7 and first == list(np.cumsum([0] + COUNTS[:-1]))
    for lanes in (7, 8, 64):
        lane, first, calls = pkg.queue_plan(lanes, COUNTS)
        assert calls == max(COUNTS) and lane == list(range(7)) and first == [0] * 7, lanes


def test_random_lists_against_the_restatement(pkg):
    rng = np.random.default_rng(18)
    for _ in range(200):
        lanes = int(rng.integers(1, 65))
        counts = [int(c) for c in rng.integers(1, 12, int(rng.integers(1, 200)))]
        assert pkg.queue_plan(lanes, counts) == plan_ref(lanes, counts), (lanes, counts)


def test_refusals(pkg):
    for lanes, counts in ((0, [1]), (65, [1]), (3, []), (3, [2, 0, 1]), (-1, [1]), (3, [-4])):
        with pytest.raises(pkg.UmxError) as e:
            pkg.queue_plan(lanes, counts)
        assert e.value.code == pkg.ERR_ARG, (lanes, counts)


def test_symbols_and_struct_are_declared(pkg):
    for name in ("umx_hip_separate_queue", "umx_hip_queue_plan", "umx_hip_debug_queue_calls"):
        assert name in pkg.HIP_SYMBOLS
    import ctypes as C
    # umx_queue_job: pointer, two ints, four pointers, pointer
    assert C.sizeof(pkg.QueueJob) == 8 + 8 + 4 * 8 + 8
