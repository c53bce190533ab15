"""CPU: the case generator of the instance-tracking tests (tests/track_util.py) — that it refuses what it must, and that the cases
test_gpu_instance_track.py runs on are not vacuous: large enough problems where the nearest neighbour is not the optimal partner,
both orientations of a rectangular problem, an empty frame between two others, new ids after a match beyond the threshold."""
import numpy as np
import pytest

import track_util as TU

NAMES = sorted(TU.SPECS)
BOTH = (False, True)


def all_pairs():
    return [(name, warped, b, t, gap) for name in NAMES for warped in BOTH for b, t, gap in TU.pair_costs(TU.case(name, warped))]


def test_every_spec_has_an_accepted_case():
    for name in NAMES:
        for warped in BOTH:
            c = TU.case(name, warped)
            TU.check_case(c)
            assert (c.warped is not None) == warped
            assert c.counts.dtype == np.int32 and c.sums.dtype == np.int64 and c.counts.shape == (c.B * c.T, c.K)
            for f, sizes in enumerate(s for sample in TU.SPECS[name][0] for s in sample):
                assert np.array_equal(np.flatnonzero(c.counts[f]), np.arange(1, sizes + 1))      # raw ids 1..n, id 0 unused


def test_margins_of_the_accepted_cases():
    for name, warped, b, t, gap in all_pairs():
        assert TU.uniqueness_margin(gap) >= TU.MARGIN, (name, warped, b, t)
        for thr in TU.THRESHOLDS:
            assert TU.threshold_margin(gap, thr) >= TU.MARGIN, (name, warped, b, t, thr)


def test_greedy_matching_is_not_enough():
    large = [(name, gap) for name, _, _, _, gap in all_pairs() if min(gap.shape) >= 30]
    differ = sum(TU.greedy_pairs(gap) != TU.optimal_pairs(gap) for _, gap in large)
    assert len(large) >= 10 and 3 * differ >= len(large), (differ, len(large))


def test_both_orientations_are_covered():
    shapes = [gap.shape for *_, gap in all_pairs()]
    assert any(r > c for r, c in shapes) and any(r < c for r, c in shapes) and any(r == c for r, c in shapes)
    assert (128, 128) in shapes and TU.case("128x128_K129", True).K == 129


def test_an_empty_frame_between_two_others():
    c = TU.case("T5_empty_middle", True)
    present = (c.counts[:, 1:] > 0).any(axis=1)
    assert present.tolist() == [True, True, False, True, True]
    want = TU.expected("T5_empty_middle", True, 3.0)
    assert np.array_equal(want[2], np.arange(c.K)) and np.array_equal(want[3], np.arange(c.K))      # the host path's quirk: raw ids again
    assert not (TU.case("T5_empty_first", False).counts[0, 1:] > 0).any()


def test_new_ids_after_a_match_beyond_the_threshold():
    hits = 0
    for name, warped, b, t, gap in all_pairs():
        rows, cols = zip(*sorted(TU.optimal_pairs(gap)))
        hits += int((gap[list(rows), list(cols)] >= 3.0).any())
    assert hits >= 5
    c = TU.case("100x100", True)
    assert TU.expected("100x100", True, 3.0).max() > 100 and TU.expected("100x100", True, 10.0).max() == 100
    assert c.B == 1 and c.T == 2


def test_a_second_optimum_is_refused():
    c = TU.two_optima_case()
    gap = TU.pair_costs(c)[0][2]
    assert gap.shape == (4, 4) and TU.uniqueness_margin(gap) == 0.0
    with pytest.raises(TU.CaseRefused):
        TU.check_case(c)


def test_a_distance_at_the_threshold_is_refused():
    counts = np.zeros((2, 2), dtype=np.int32)
    sums = np.zeros((2, 2, 2), dtype=np.int64)
    counts[:, 1] = 2
    sums[0, 1] = (40, 40)
    sums[1, 1] = (40, 46)      # centres (20, 20) and (20, 23): exactly 3 apart
    c = TU.Case(counts, sums, None, 1, 2)
    with pytest.raises(TU.CaseRefused):
        TU.check_case(c)
    TU.check_case(c, thresholds=(10.0,))
    assert TU.expected_tables(c, 3.0).tolist() == [[0, 1], [0, 2]] and TU.expected_tables(c, 10.0).tolist() == [[0, 1], [0, 1]]


def test_a_missing_raw_id_is_refused():
    c = TU.case("5x1", False)
    counts = c.counts.copy()
    counts[1, 1:4] = (3, 0, 5)      # frame 1: ids 1 and 3, no 2
    with pytest.raises(TU.CaseRefused):
        TU.check_case(TU.Case(counts, c.sums, None, 1, 2))
