"""The definition of a batch of many streams (tests/streams_model.py, include/mpeg1_hip.h "Streams") checked against itself on
the CPU: one call over spans is the independent per-stream walks of tests/rd_rate_model.py; a span split across two calls chains
through the levels; empty spans pass their level through; streams with different rates do not interact; and the tiling rule
names each kind of violation."""
import random

import pytest

import rd_rate_model as rd
import streams_model as sm


def _table(rng, K, n, unencodable=False):
    """Non-monotone sizes and distortions (a larger candidate may be smaller and may be worse)."""
    S = [[rng.randrange(60, 900) for _ in range(n)] for _ in range(K)]
    D = [[rng.randrange(0, 5000) for _ in range(n)] for _ in range(K)]
    status = [0] * K
    if unencodable and K > 1:
        status[rng.randrange(K)] = rd.UNENCODABLE
    return S, D, status


def _case(seed, K=4):
    rng = random.Random(seed)
    lengths = [rng.choice((0, 1, 3, 8, 9, 17)) for _ in range(6)]
    spans = sm.spans_of([(n, rng.randrange(-5, 1000)) for n in lengths])
    S, D, status = _table(rng, K, sum(lengths), unencodable=True)
    rates = [(rng.randrange(50, 600), rng.randrange(600, 4000)) for _ in lengths]
    levels = [rng.randrange(-2000, 5000) for _ in lengths]
    return spans, S, D, status, rates, levels


@pytest.mark.parametrize("rule", [sm.LARGEST_THAT_FITS, sm.LEAST_DISTORTION])
@pytest.mark.parametrize("seed", range(6))
def test_a_call_over_spans_is_the_independent_walks(seed, rule):
    spans, S, D, status, rates, levels = _case(seed)
    picks, dist, after, bits = sm.streams_bitrate(S, D, spans, rates, levels, rule, status)
    over_any = False
    for s, (first, n, _) in enumerate(spans):
        own_S = [[S[k][first + j] for j in range(n)] for k in range(len(S))]      # the stream's frames as a batch of their own
        own_D = [[D[k][first + j] for j in range(n)] for k in range(len(S))]
        if rule == sm.LARGEST_THAT_FITS:
            want, over, level = rd.bitrate_byte_rule(own_S, *rates[s], levels[s])
        else:
            want, over, level = rd.bitrate_walk(own_S, own_D, *rates[s], levels[s], status)
        assert picks[first:first + n] == want and after[s] == level
        assert dist[first:first + n] == [own_D[k][j] for j, k in enumerate(want)]
        over_any |= bool(over)
    assert bits == (sm.STATUS_OVER_BUDGET if over_any else 0)
    assert sm.frame_indices(spans, len(S[0])) == [i + j for _, n, i in spans for j in range(n)]


@pytest.mark.parametrize("rule", [sm.LARGEST_THAT_FITS, sm.LEAST_DISTORTION])
def test_a_span_split_across_two_calls_chains_through_the_levels(rule):
    spans, S, D, status, rates, levels = _case(11)
    whole = sm.streams_bitrate(S, D, spans, rates, levels, rule, status)
    # every stream's span cut in two: the first call takes the front halves, the second the rest, from the first call's levels
    cuts = [n // 2 for _, n, _ in spans]
    front = [[f for (first, _, _), c in zip(spans, cuts) for f in range(first, first + c)]]
    back = [[f for (first, n, _), c in zip(spans, cuts) for f in range(first + c, first + n)]]
    picks = [None] * len(S[0])
    now = levels
    for frames, pairs in ((front[0], [(c, i) for (_, _, i), c in zip(spans, cuts)]),
                          (back[0], [(n - c, i + c) for (_, n, i), c in zip(spans, cuts)])):
        part_S = [[row[f] for f in frames] for row in S]
        part_D = [[row[f] for f in frames] for row in D]
        got, _, now, _ = sm.streams_bitrate(part_S, part_D, sm.spans_of(pairs), rates, now, rule, status)
        for f, k in zip(frames, got):
            picks[f] = k
    assert picks == whole[0] and now == whole[2]


def test_empty_spans_pass_the_level_through():
    S, D = [[100, 200, 300]], [[5, 6, 7]]
    spans = sm.spans_of([(0, 77), (3, 0), (0, 5)])
    rates = [(10, 50), (100, 1000), (10, 10 ** 6)]
    _, _, after, bits = sm.streams_bitrate(S, D, spans, rates, [40, 500, 12345], sm.LARGEST_THAT_FITS)
    assert after[0] == 40 and after[2] == 12345 and bits == 0
    _, _, after, _ = sm.streams_bitrate(S, D, spans, rates, [90, 500, 10 ** 7], sm.LEAST_DISTORTION)
    assert after[0] == 50 and after[2] == 10 ** 6                       # an empty span writes min(level, C)
    assert sm.stream_bytes(spans, [100, 200, 300]) == [0, 600, 0]


@pytest.mark.parametrize("rule", [sm.LARGEST_THAT_FITS, sm.LEAST_DISTORTION])
def test_streams_with_different_rates_do_not_interact(rule):
    spans, S, D, status, rates, levels = _case(23)
    base = sm.streams_bitrate(S, D, spans, rates, levels, rule, status)
    victim = next(s for s, (_, n, _) in enumerate(spans) if n > 0)
    other_rates = [(r, c) if s == victim else (7 * r, 9 * c) for s, (r, c) in enumerate(rates)]
    other_levels = [lv if s == victim else lv - 1000 for s, lv in enumerate(levels)]
    moved = sm.streams_bitrate(S, D, spans, other_rates, other_levels, rule, status)
    first, n, _ = spans[victim]
    assert moved[0][first:first + n] == base[0][first:first + n] and moved[2][victim] == base[2][victim]
    # a debt that later refills repay: a stream that starts far below zero comes back above it
    _, _, after, bits = sm.streams_bitrate([[100] * 30], None, [(0, 30, 0)], [(200, 5000)], [-1500], sm.LARGEST_THAT_FITS)
    assert after == [1500] and bits == sm.STATUS_OVER_BUDGET


def test_a_bad_rate_entry_sends_its_stream_to_candidate_zero():
    S, D = [[100] * 6, [200] * 6], [[9] * 6, [1] * 6]
    spans = sm.spans_of([(3, 0), (3, 0)])
    for bad in ((0, 100), (200, 100), (1, 2 ** 62)):
        picks, dist, after, bits = sm.streams_bitrate(S, D, spans, [bad, (500, 1000)], [-77, 1000], sm.LEAST_DISTORTION)
        assert picks == [0, 0, 0, 1, 1, 1] and dist[:3] == [9, 9, 9] and after[0] == -77 and bits == sm.STATUS_STREAMS


def test_the_tiling_rule_and_each_kind_of_violation():
    n = 8
    assert sm.violation([(0, 3, 0), (3, 0, 9), (3, 5, 1)], n) is None
    assert sm.violation([(1, 7, 0)], n) == "start"
    assert sm.violation([(0, 3, 0), (4, 4, 0)], n) == "gap"
    assert sm.violation([(0, 5, 0), (3, 5, 0)], n) == "overlap"
    assert sm.violation([(0, 3, 0), (3, 9, 0)], n) == "overrun"
    assert sm.violation([(0, 3, 0), (3, 4, 0)], n) == "short"
    # whatever the spans say, what they address stays inside the batch
    for spans in ([(1, 7, 0)], [(0, 3, 0), (4, 4, 0)], [(0, 5, 0), (3, 5, 0)], [(0, 3, 0), (3, 9, 0)], [(2 ** 32 - 1, 2 ** 32 - 1, 0)]):
        for span in spans:
            lo, hi = sm.clamped(span, n)
            assert 0 <= lo <= n and 0 <= hi <= n
        _, _, _, bits = sm.streams_bitrate([[1] * n], None, spans, [(1, 1)] * len(spans), [0] * len(spans), sm.LARGEST_THAT_FITS)
        assert bits & sm.STATUS_STREAMS
