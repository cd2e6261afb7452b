"""CPU checks of the model of the batch and bitrate picks by distortion (tests/rd_rate_model.py, the rules of
include/mpeg1_hip.h): the gradient table's chain and pick, and on seeded random tables with many ties, against exhaustive search,
that the byte form keeps its budget, that the picked set is optimal for the Lagrangian at its last taken step's slope, that the
distortion form's prefix is the shortest, that chains have non-increasing slopes, that candidates out of the running are never
picked and that the bitrate walk chains."""
import itertools
import random
from fractions import Fraction

import rd_oracle
import rd_rate_model as M


def _tables(seed, count=120):
    rng = random.Random(seed)
    for _ in range(count):
        n, K = rng.randint(1, 5), rng.randint(1, 4)
        hi = rng.choice((3, 6, 12))
        yield ([[rng.randint(1, hi) for _ in range(n)] for _ in range(K)],
               [[rng.randint(1, hi) for _ in range(n)] for _ in range(K)], rng)


def _totals(S, D, picks):
    return sum(S[k][f] for f, k in enumerate(picks)), sum(D[k][f] for f, k in enumerate(picks))


def test_gradient_chain_and_pick():
    S, D = [[s] for s in rd_oracle.GRADIENT_BYTES], [[d] for d in rd_oracle.GRADIENT_D]
    assert M.chains(S, D) == [[0, 1, 2, 3, 5, 6]]
    picks, over = M.batch_pick(S, D, M.BEST_IN_BUDGET, 8000)
    assert (picks, over) == ([3], False)
    assert rd_oracle.GRADIENT_QUALITIES[3] == 38 and rd_oracle.GRADIENT_BYTES[3] == 7815
    assert M.batch_byte_rule(S, 8000) == ([7], False) and rd_oracle.GRADIENT_QUALITIES[7] == 92   # the byte rule's pick
    assert M.bitrate_walk(S, D, 8000, 8000, 8000)[0] == [3]
    assert M.batch_pick(S, D, M.BEST_IN_BUDGET, 3148) == ([0], True)
    assert M.batch_pick(S, D, M.SMALLEST_AT_DISTORTION, 1400207) == ([3], False)
    assert M.batch_pick(S, D, M.SMALLEST_AT_DISTORTION, 499605) == ([6], True)


def test_chains_start_smallest_and_have_non_increasing_slopes():
    for S, D, _ in _tables(1):
        K = len(S)
        for f, c in enumerate(M.chains(S, D)):
            assert (S[c[0]][f], D[c[0]][f], c[0]) == min((S[k][f], D[k][f], k) for k in range(K))
            slopes = [Fraction(D[a][f] - D[b][f], S[b][f] - S[a][f]) for a, b in zip(c, c[1:])]
            assert all(s > 0 for s in slopes) and all(x >= y for x, y in zip(slopes, slopes[1:]))
            assert len(set(c)) == len(c) <= K
            # the chain's end is the least D there is at the smallest record that has it
            least = min(D[k][f] for k in range(K))
            assert D[c[-1]][f] == least and S[c[-1]][f] == min(S[k][f] for k in range(K) if D[k][f] == least)


def test_byte_form_keeps_the_budget_and_is_lagrangian_optimal():
    for S, D, rng in _tables(2):
        K, n = len(S), len(S[0])
        ch = M.chains(S, D)
        order = M.steps(S, D, ch)
        start = sum(S[c[0]][f] for f, c in enumerate(ch))
        bounds = [start + sum(t[2] for t in order[:i]) for i in range(len(order) + 1)]
        for limit in sorted({0, start - 1, 10 ** 6} | set(bounds) | {b - 1 for b in bounds} | {rng.randint(0, 40)}):
            if limit < 0:
                continue
            picks, over = M.batch_pick(S, D, M.BEST_IN_BUDGET, limit)
            s_tot, d_tot = _totals(S, D, picks)
            assert over == (start > limit)
            if over:
                assert picks == [c[0] for c in ch]
                continue
            assert s_tot <= limit
            taken = [t for t in order if ch[t[0]].index(picks[t[0]]) >= t[1]]
            assert taken == order[:len(taken)]                       # a prefix of the order
            assert len(taken) == len(order) or s_tot + order[len(taken)][2] > limit   # the longest one
            if taken:   # no assignment has a smaller D + lambda * s at the last taken step's slope
                lam = Fraction(taken[-1][3], taken[-1][2])
                best = min(sum(D[k][f] + lam * S[k][f] for f, k in enumerate(p)) for p in itertools.product(range(K), repeat=n))
                assert d_tot + lam * s_tot == best


def test_distortion_form_takes_the_shortest_prefix():
    for S, D, rng in _tables(3):
        ch = M.chains(S, D)
        order = M.steps(S, D, ch)
        start = sum(D[c[0]][f] for f, c in enumerate(ch))
        after = [start - sum(t[3] for t in order[:i]) for i in range(len(order) + 1)]
        for limit in sorted({0, 10 ** 6} | set(after) | {a - 1 for a in after if a > 0}):
            picks, over = M.batch_pick(S, D, M.SMALLEST_AT_DISTORTION, limit)
            want = next((i for i, a in enumerate(after) if a <= limit), None)
            assert over == (want is None)
            i = len(order) if want is None else want
            at = [0] * len(ch)
            for f, j, _, _ in order[:i]:
                at[f] = j
            assert picks == [c[at[f]] for f, c in enumerate(ch)]
            assert (_totals(S, D, picks)[1] <= limit) == (not over)


def test_candidates_out_of_the_running_are_never_picked():
    for S, D, rng in _tables(4):
        K = len(S)
        status = [rng.choice((0, 1, 4)) for _ in range(K)]
        ks = M.running(K, status)
        assert ks == ([k for k in range(K) if not status[k] & 1] or [0])
        for rule in (M.BEST_IN_BUDGET, M.SMALLEST_AT_DISTORTION):
            for limit in (0, 7, 20, 10 ** 6):
                picks, _ = M.batch_pick(S, D, rule, limit, status)
                assert set(picks) <= set(ks)
                sub = M.batch_pick([S[k] for k in ks], [D[k] for k in ks], rule, limit)   # = the rule on the rows left
                assert picks == [ks[k] for k in sub[0]]
        picks, _, _ = M.bitrate_walk(S, D, 3, 9, 5, status)
        assert set(picks) <= set(ks)


def test_bitrate_walk_chains_and_picks_least_distortion_that_fits():
    for S, D, rng in _tables(5):
        K, n = len(S), len(S[0])
        rate = rng.randint(1, 6)
        cap = rate + rng.randint(0, 8)
        level = rng.randint(-10, 20)
        picks, over, out = M.bitrate_walk(S, D, rate, cap, level)
        L = min(level, cap)
        for f in range(n):
            fit = [k for k in range(K) if S[k][f] <= L]
            assert (f in over) == (not fit)
            if fit:
                assert (D[picks[f]][f], S[picks[f]][f], picks[f]) == min((D[k][f], S[k][f], k) for k in fit)
            else:
                assert (S[picks[f]][f], picks[f]) == min((S[k][f], k) for k in range(K))
            L = min(cap, L - S[picks[f]][f] + rate)
        assert L == out
        cut = rng.randint(0, n)
        a = M.bitrate_walk([r[:cut] for r in S], [r[:cut] for r in D], rate, cap, level) if cut else ([], [], min(level, cap))
        b = M.bitrate_walk([r[cut:] for r in S], [r[cut:] for r in D], rate, cap, a[2]) if cut < n else ([], [], a[2])
        assert (a[0] + b[0], a[1] + [cut + f for f in b[1]], b[2]) == (picks, over, out)
