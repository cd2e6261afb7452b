"""The per-stream budget's definition, on the model alone (tests/streams_budget_model.py; include/mpeg1_hip.h "Streams: a budget
per stream"): streams do not interact, one span is the single-batch rule, two spans are two single results side by side; and a
census of the cases tests/test_gpu_streams_budget.py runs on the device, so that it cannot pass on cases that never take a step."""
import random

import pytest

import rd_rate_model as rm
import streams_budget_cases as cases
import streams_budget_model as bm
import streams_model as sm

RULES = list(bm.RULES)


def _single(S, D, rule, limit, status):
    if rule == bm.LARGEST_THAT_FITS:
        return rm.batch_byte_rule(S, limit)
    return rm.batch_pick(S, D, rm.BEST_IN_BUDGET if rule == bm.LEAST_DISTORTION else rm.SMALLEST_AT_DISTORTION, limit, status)


@pytest.mark.parametrize("rule", RULES)
def test_one_span_is_the_single_batch_rule(rule):
    for seed in range(6):
        spans, S, D, status, limits = cases.case(seed, 1, 3, rule, lengths=[40])
        picks, dist, stream_status, bits = bm.streams_budget(S, D, spans, limits, rule, status)
        want, over = _single(S, D, rule, limits[0], status)
        assert picks == want and dist == [D[k][f] for f, k in enumerate(want)]
        assert stream_status == [bm.OVER_BIT[rule] if over else 0] and bits == stream_status[0]


@pytest.mark.parametrize("rule", RULES)
def test_two_spans_are_the_two_single_results_side_by_side(rule):
    for seed in range(6):
        spans, S, D, status, limits = cases.case(100 + seed, 2, 4, rule, lengths=[17, 9])
        picks, _, stream_status, bits = bm.streams_budget(S, D, spans, limits, rule, status)
        a, over_a = _single([r[:17] for r in S], [r[:17] for r in D], rule, limits[0], status)
        b, over_b = _single([r[17:] for r in S], [r[17:] for r in D], rule, limits[1], status)
        assert picks == a + b
        assert stream_status == [bm.OVER_BIT[rule] if o else 0 for o in (over_a, over_b)]
        assert bits == stream_status[0] | stream_status[1]


@pytest.mark.parametrize("rule", RULES)
def test_a_change_in_one_span_changes_no_pick_in_another(rule):
    rng = random.Random(7)
    changed = 0
    for seed in range(8):
        spans, S, D, status, limits = cases.case(200 + seed, 4, 3, rule, lengths=[9, 0, 33, 8])
        before = bm.streams_budget(S, D, spans, limits, rule, status)
        a = rng.choice([0, 2, 3])
        lo, hi = sm.clamped(spans[a], len(S[0]))
        f = rng.randrange(lo, hi)
        for k in range(3):                                   # this frame's column: larger records, other distortions
            S[k][f] = S[k][f] * 3 + 1000 * k
            D[k][f] = rng.randrange(0, 1 << 40)
        after = bm.streams_budget(S, D, spans, limits, rule, status)
        for b, span in enumerate(spans):
            if b != a:
                blo, bhi = sm.clamped(span, len(S[0]))
                assert after[0][blo:bhi] == before[0][blo:bhi] and after[2][b] == before[2][b]
        changed += after[0][lo:hi] != before[0][lo:hi]
    assert changed > 0                                       # (the change does move span a's own picks in some case)


def test_empty_spans_bad_spans_and_the_scratch_bit():
    spans, S, D, status, _ = cases.case(5, 3, 3, bm.LEAST_DISTORTION, lengths=[4, 0, 6])
    picks, _, stream_status, bits = bm.streams_budget(S, D, spans, [0, 0, cases.U64], bm.LEAST_DISTORTION, status)
    assert stream_status == [sm.STATUS_OVER_BUDGET, 0, 0] and bits == sm.STATUS_OVER_BUDGET     # an empty span is not over
    status[0] |= sm.STATUS_SCRATCH
    assert bm.streams_budget(S, D, spans, [cases.U64] * 3, bm.LEAST_DISTORTION, status)[3] == sm.STATUS_SCRATCH
    gap = [(0, 4, 0), (5, 5, 0)]                             # frame 4 is in no span: candidate 0
    picks, _, _, bits = bm.streams_budget(S, D, gap, [cases.U64] * 2, bm.LARGEST_THAT_FITS)
    assert bits & sm.STATUS_STREAMS and picks[4] == 0 and all(k == 2 for f, k in enumerate(picks) if f != 4)


@pytest.mark.parametrize("rule", RULES)
def test_census_of_the_gpu_cases(rule):
    """Of the non-empty spans of the rule's cases, at least 5 % end over their limit, 5 % with no step taken, 5 % with some and
    5 % with every one: a condition on the INPUTS of the GPU test, counted with the model alone."""
    counts = {"over": 0, "none": 0, "some": 0, "all": 0}
    for name, args in cases.case_ids():
        if args[3] != rule:
            continue
        spans, S, D, status, limits = cases.case(*args)
        picks, _, stream_status, _ = bm.streams_budget(S, D, spans, limits, rule, status)
        for s, span in enumerate(spans):
            lo, hi = sm.clamped(span, len(S[0]))
            if hi > lo:
                cls = cases.census_class([r[lo:hi] for r in S], [r[lo:hi] for r in D], rule, limits[s], status, picks[lo:hi],
                                         bool(stream_status[s]))
                counts[cls] += 1
    total = sum(counts.values())
    print(f"rule {rule}: {counts} of {total} non-empty spans")
    assert total >= 400
    for cls, c in counts.items():
        assert c * 20 >= total, (cls, counts)
