"""plan_lanes (zonos_vibes_amd/speaker.py): the grouping of clips into ragged launch sequences, no GPU."""
import random

import pytest

from zonos_vibes_amd.speaker import plan_lanes


def _frames(n, seed):
    r = random.Random(seed)
    return [r.randint(2, 3000) for _ in range(n)]


def _check(frames, groups, max_lanes, cap):
    assert sorted(i for g in groups for i in g) == list(range(len(frames)))  # every index exactly once
    for g in groups:
        assert 1 <= len(g) <= max_lanes
        longest = max(frames[i] for i in g)
        assert len(g) == 1 or len(g) * longest <= cap
        if longest > cap:
            assert len(g) == 1


@pytest.mark.parametrize("n", [1, 32, 33, 100])
@pytest.mark.parametrize("max_lanes,cap", [(32, 32768), (2, 32768), (32, 4000), (5, 1)])
def test_every_clip_once_within_both_caps(n, max_lanes, cap):
    frames = _frames(n, n)
    groups = plan_lanes(frames, max_lanes, cap)
    _check(frames, groups, max_lanes, cap)
    assert groups == plan_lanes(list(frames), max_lanes, cap)  # deterministic


def test_longest_first_and_full_groups():
    frames = [10, 50, 30, 50, 20]
    assert plan_lanes(frames) == [[1, 3, 2, 4, 0]]                       # longest first, ties by index
    assert plan_lanes(frames, max_lanes=2) == [[1, 3], [2, 4], [0]]
    assert plan_lanes(frames, max_lane_frames=100) == [[1, 3], [2, 4, 0]]  # 3 x 50 > 100; 3 x 30 <= 100
    assert plan_lanes([1000] * 33) == [list(range(32)), [32]]
    assert len(plan_lanes([1000] * 100)) == 4


def test_oversize_clip_is_alone():
    frames = [100, 40000, 200, 33000]
    groups = plan_lanes(frames)
    assert groups[:2] == [[1], [3]] and sorted(groups[2]) == [0, 2]
    _check(frames, groups, 32, 32768)


def test_empty_and_bad_arguments():
    assert plan_lanes([]) == []
    for kw in (dict(max_lanes=0), dict(max_lanes=33), dict(max_lane_frames=0)):
        with pytest.raises(ValueError):
            plan_lanes([5, 6], **kw)
