"""CPU-side checks of tests/frame_axis.py: with the oracle alone, every case of tests/test_gpu_frame_axis.py has the properties that
make it able to fail — values that differ across every block edge and do not fold onto the first block, levels that a chunk edge
must carry, cuts inside ties that straddle the 1024 lanes, steps in the last workgroup, spans beyond the first 256."""
import pytest

import frame_axis as fa
import rd_oracle as rd
import rd_rate_model as M
import streams_model as sm
from rate_rules import batch_rule

CHANNELS = (3, 4)
PER_FRAME_RULES = (fa.LARGEST, rd.BEST_IN_BUDGET, rd.SMALLEST_AT_DISTORTION)
BITRATE_RULES = (fa.BY_SIZE, fa.BY_DISTORTION)


def test_the_geometry_is_the_one_the_cases_are_built_on():
    assert (fa.W, fa.H, fa.Q, fa.N, fa.FIRST) == (32, 32, 12, 1100, 200)
    assert fa.N > 1024 and fa.N == 2 * 512 + 76 and 76 == 9 * 8 + 4
    assert fa.K8 == (1, 2, 4, 6, 8, 10, 11, 12) and max(fa.K8) == fa.Q
    assert len(set(fa.order())) == fa.POOL == 7 and len(fa.order()) == fa.N
    for channels in CHANNELS:
        px = fa.pool(channels)
        assert px.shape == (7, 32, 32, channels) and len({p.tobytes() for p in px}) == 7
        assert fa.batch(channels).shape == (fa.N, 32, 32, channels)
        assert all((fa.batch(channels)[f] == px[p]).all() for f, p in list(enumerate(fa.order()))[::97])


@pytest.mark.parametrize("channels", CHANNELS)
def test_the_pool_gives_distinct_size_and_distortion_columns(orc, channels):
    s, d = fa.pool_table(orc, channels)
    assert len({tuple(row[p] for row in s) for p in range(fa.POOL)}) >= 5
    assert len({tuple(row[p] for row in d) for p in range(fa.POOL)}) >= 5
    assert len({tuple(row) for row in s}) > 4                       # the candidates differ in size too
    S, D = fa.table(orc, channels)
    assert [len(S), len(S[0]), len(D), len(D[0])] == [8, fa.N, 8, fa.N]
    indices = (0, 255, 256, 1299, 7, 511, 77, fa.FIRST)
    for f in (0, 255, 256, 1023, 1024, 1099):                       # the gather, and that a record's size does not depend on its index
        assert [len(fa.records(orc, [i], [q], channels, start=f)[0]) for i, q in zip(indices, fa.K8)] == [row[f] for row in S]


def test_records_are_per_frame_at_their_own_index_and_quality(orc):
    q = fa.qualities()
    got = fa.records(orc, [fa.FIRST + f for f in range(250, 260)], q[250:260], 3, start=250)
    px = fa.batch(3)
    assert got == [orc.encode_frame(px[f], 32, 32, fa.FIRST + f, q[f], orc.MODE_FULL, 3) for f in range(250, 260)]
    assert got[5] != fa.records(orc, [fa.FIRST + 256], [q[255]], 3, start=255)[0]         # the index is in the record


def test_per_frame_qualities_cross_every_block_edge():
    q = fa.qualities()
    assert fa.axis_problem(q) is None and min(q) >= 1 and max(q) <= fa.Q
    assert q[255] != q[256] and q[511] != q[512] and q[1023] != q[1024]
    assert all(len(set(q[b:b + 256])) >= 6 for b in range(0, fa.N, 256))
    assert 2 * sum(q[f] != q[f & 255] for f in range(256, fa.N)) >= fa.N - 256
    # the detector itself refuses what it is there to refuse
    assert fa.axis_problem(q[:256] * 4 + q[:76]) is not None
    assert fa.axis_problem(q[:255] + [q[256]] + q[256:]) is not None
    assert fa.axis_problem([1 + f % 5 for f in range(fa.N)]) is not None


@pytest.mark.parametrize("rule", PER_FRAME_RULES)
@pytest.mark.parametrize("channels", CHANNELS)
def test_per_frame_limits_give_picks_that_cross_every_block_edge(orc, channels, rule):
    S, D = fa.table(orc, channels)
    limits, picks, over = fa.per_frame_limits(orc, rule, channels)
    assert (picks, over) == fa.per_frame_model(S, D, rule, limits)
    assert fa.axis_problem(picks) is None and over == [fa.N - 1] and min(limits) >= 0
    # a prefix of the model's results is its results on the prefix: the GPU cases share one table
    for n in (256, 257):
        assert fa.per_frame_model(fa.prefix(S, n), fa.prefix(D, n), rule, limits[:n]) == (picks[:n], [])


@pytest.mark.parametrize("by", BITRATE_RULES)
@pytest.mark.parametrize("channels", CHANNELS)
def test_the_bitrate_walk_carries_its_level_across_both_chunk_edges(orc, channels, by):
    S, D = fa.table(orc, channels)
    rate, cap, L0 = fa.bitrate_params(orc, by, channels)
    assert 1 <= rate <= cap and fa.bitrate_problem(S, D, by, rate, cap, L0) is None
    picks, over, after = fa.bitrate_walk(S, D, by, rate, cap, L0)
    before, L = [], min(L0, cap)
    for f, k in enumerate(picks):
        before.append(L)
        L = min(cap, L - S[k][f] + rate)
    assert L == after
    assert any(before[f] < 0 for f in over) and over and max(over) < 512 and min(before[max(over) + 1:]) >= 0   # the debt, repaid
    for lo in (0, 512, 1024):
        hi = min(lo + 512, fa.N)
        assert any(before[f] - S[picks[f]][f] + rate > cap for f in range(lo, hi)) and len(set(picks[lo:hi])) > 1
    for cut in (512, 1024):
        assert before[cut] not in (min(L0, cap), cap)
        assert fa.bitrate_walk(S, D, by, rate, cap, L0, cut)[0] != picks[cut:]
    # prefixes and chained calls: the model on a prefix is the prefix of the model
    for n in (512, 513, 519, 520, 1024):
        p, o, lvl = fa.bitrate_walk(S, D, by, rate, cap, L0, 0, n)
        assert (p, o, lvl) == (picks[:n], [f for f in over if f < n], before[n])
    p, o, lvl = fa.bitrate_walk(S, D, by, rate, cap, before[513], 513)
    assert (p, lvl) == (picks[513:], after)
    # the refusal the detector is there for: a capacity equal to the rate holds the level still
    assert fa.bitrate_problem(S, D, by, rate, rate, L0) is not None


@pytest.mark.parametrize("channels", CHANNELS)
def test_no_debt_can_arise_behind_the_first_one(orc, channels):
    """Why the bitrate cases hold their repaid debt in the first chunk alone (frame_axis.bitrate_problem): a debt that arises past
    the start and is repaid needs a rate between the smallest records of two frames, and here they are all equal."""
    S, _ = fa.table(orc, channels)
    assert len({min(row[f] for row in S) for f in range(fa.N)}) == 1 and len(set(S[0])) == 1


@pytest.mark.parametrize("n", [1024, 1025, 1100])
@pytest.mark.parametrize("channels", CHANNELS)
def test_the_batch_budget_cuts_inside_a_tie_across_the_1024_lanes(orc, channels, n):
    s = fa.prefix(fa.table(orc, channels)[0], n)
    budget, picks = fa.batch_budget(orc, n, channels)
    assert fa.batch_budget_problem(s, budget) is None
    assert (picks, False) == batch_rule(s, budget) and len(set(picks)) == 2 and max(picks) - min(picks) == 1
    top = min(picks)
    order = fa.upgrades(s, top)
    taken, refused = [x for x in order if picks[x[1]] == top + 1], [x for x in order if picks[x[1]] == top]
    assert order == taken + refused and taken and refused           # a prefix of the order is taken
    (dl, fl), (dr, fr) = taken[-1], refused[0]
    assert dl == dr and fl < fr
    assert n <= 1024 or fr >= 1024
    assert sum(s[k][f] for f, k in enumerate(picks)) <= budget < sum(s[top + 1])


@pytest.mark.parametrize("n", [32, 33, 1100])
@pytest.mark.parametrize("rule", [M.BEST_IN_BUDGET, M.SMALLEST_AT_DISTORTION])
@pytest.mark.parametrize("channels", CHANNELS)
def test_the_batch_pick_by_distortion_takes_steps_in_the_last_workgroup(orc, channels, rule, n):
    S, D = (fa.prefix(t, n) for t in fa.table(orc, channels))
    limit, picks = fa.rd_batch_limit(orc, rule, n, channels)
    assert fa.rd_batch_problem(S, D, rule, limit) is None and (picks, False) == M.batch_pick(S, D, rule, limit)
    at, length = fa.steps_taken(S, D, picks)
    last = 32 * ((n - 1) // 32)
    assert any(at[f] >= 1 for f in range(last, n)) and max(at) >= 2 and at != length and len(set(picks)) > 1


@pytest.mark.parametrize("which", fa.SPAN_TABLES)
def test_the_spans_reach_beyond_the_first_256_spans_and_frames(which):
    spans = fa.spans(which)
    assert fa.spans_problem(spans) is None
    assert len(spans) == 300 and sm.violation(spans, fa.N) is None and sum(n for _, n, _ in spans) == fa.N
    assert sum(1 for _, n, _ in spans if n == 0) >= 200
    assert spans[256][1] > 0 and spans[299][1] > 0
    assert any(first == 256 and n > 0 for first, n, _ in spans)
    assert any(first < 512 < first + n - 1 and first != 256 for first, n, _ in spans)
    index = sm.frame_indices(spans, fa.N)
    assert all((index[f] & 255) != (f & 255) for f in range(256, fa.N))
    assert fa.span_pairs(which) == [(n, i) for _, n, i in spans] and sm.spans_of(fa.span_pairs(which)) == spans
    # a map that only sees lanes 0..255 drops frames
    assert any(n > 0 for _, n, _ in spans[256:])


def test_the_two_span_tables_share_out_the_lengths():
    """0, 1, 7, 8, 9, 64, 65, 255, 257 and 513 add up to 1179 frames, more than the batch holds: "a" has the span of 513, "b" those
    of 255 and 257, both have all the others."""
    assert sum(fa.SPAN_LENGTHS) > fa.N
    lengths = {which: [n for _, n, _ in fa.spans(which)] for which in fa.SPAN_TABLES}
    assert set(fa.SPAN_LENGTHS) <= set(lengths["a"]) | set(lengths["b"])
    for which in fa.SPAN_TABLES:
        assert {0, 1, 7, 8, 9, 64, 65} <= set(lengths[which])
    assert lengths["a"].count(513) == 1 and {255, 257} <= set(lengths["b"])
    assert lengths["a"][256] == 513                                 # the longest span is one that lane 256 maps


@pytest.mark.parametrize("by", BITRATE_RULES)
def test_the_streams_bitrate_case(orc, by):
    rates, levels = fa.streams_bitrate_params(orc, by)
    spans = sm.spans_of(fa.BITRATE_PAIRS)
    assert [n for _, n, _ in spans] == [513, 0, 587] and sm.violation(spans, fa.N) is None
    assert all(sm.rate_ok(r, c) for r, c in rates) and len(set(rates)) == 3
    S, D = fa.table(orc)
    rule = sm.LARGEST_THAT_FITS if by == fa.BY_SIZE else sm.LEAST_DISTORTION
    picks, _, after, bits = sm.streams_bitrate(S, D, spans, rates, levels, rule)
    assert bits == sm.STATUS_OVER_BUDGET and after[1] == min(levels[1], rates[1][1])
    # one walk per span
    for s, (first, n, _) in enumerate(spans):
        p, _, lvl = fa.bitrate_walk(S, D, by, rates[s][0], rates[s][1], levels[s], first, first + n) if n else ([], [], after[s])
        assert (p, lvl) == (picks[first:first + n], after[s])
