"""One long batch for the kernels that split the frame or stream axis at a fixed width — TEST INFRASTRUCTURE ONLY (no tests in
this module; tests/test_frame_axis_cpu.py pins, with the oracle alone, that every case below can fail, and
tests/test_gpu_frame_axis.py runs them).

The batch: N = 1100 pictures of 32 x 32 (mode "full", quality factor 12) drawn from a pool of 7 distinct pictures, one pool of 3
channels and one of 4.  1100 is above k_rate_pick<false>'s 1024 lanes and is 2 * 512 + 76, 76 = 9 * 8 + 4: three chunks of the
bitrate walks, the last one ending inside a step of eight.  table() is the oracle's S[k][f], D[k][f] of the batch, computed once
per pool picture and quality and gathered; records() is the oracle's record of every frame at its own index and quality.

Every case parameter is a function that searches seeded draws or a small grid, asserts the conditions that make the case able to
fail and raises when nothing meets them.  All of them take the K = 8 candidates (1, 2, 4, 6, 8, 10, 11, 12); no case needed
fewer.  Expected values come from the models the project has: batch_rule and cbr_rule (tests/test_rate_abi.py), rd_oracle.pick
and largest_that_fits, rd_rate_model.batch_pick and bitrate_walk, streams_model.

The stream spans are TWO tables of 300 spans, each tiling the 1100 frames: the lengths the cases need (0, 1, 7, 8, 9, 64, 65, 255,
257 and one span of 513) add up to 1179 frames, more than the batch holds, so table "a" carries the span of 513 and table "b" the
spans of 255 and 257; every other condition holds for each table on its own."""
import numpy as np

import rd_oracle as rd
import rd_rate_model as M
import streams_model as sm
from gpu_calls import _mixed_frames
from rate_rules import batch_rule, cbr_rule

W = H = 32
Q = 12
N = 1100
FIRST = 200                                  # the frame index passes 255 -> 256 several times inside the batch
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
POOL = 7
# flat, gentle and nearly full noise.  At this geometry and quality factor only noise of an amplitude near 256 leaves anything but
# DC in a record, so that is where the record sizes differ between pictures and between candidates
AMPS = (4, 256, 40, 220, 240, 200, 250)
ORDER_SEED = 1100
EDGES = (256, 512, 1024)
LARGEST = "largest"                          # the rule of m1v_encode_budget_device beside rd.BEST_IN_BUDGET / SMALLEST_AT_DISTORTION
BY_SIZE, BY_DISTORTION = "size", "distortion"

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- the batch ------------------------------------------------------------------------------------------------------------------
def pool(channels=3):
    """The 7 distinct pictures [7, H, W, channels]."""
    return _once(("pool", channels), lambda: _mixed_frames(np.random.default_rng(700 + channels), POOL, W, H, channels, amps=AMPS))


def order():
    """[frame] the pool picture of every frame of the batch."""
    return _once("order", lambda: [int(p) for p in np.random.default_rng(ORDER_SEED).integers(0, POOL, N)])


def batch(channels=3):
    """The batch [N, H, W, channels]."""
    return _once(("batch", channels), lambda: np.ascontiguousarray(pool(channels)[order()]))


def pool_table(orc, channels=3, cands=K8):
    """(s[k][p], d[k][p]) of the pool's pictures: the oracle's record size (which does not depend on the frame index) and
    rd_oracle.frame_distortion."""
    def make():
        px = pool(channels)
        s = [[len(orc.encode_frame(px[p], W, H, 0, q, orc.MODE_FULL, channels)) for p in range(POOL)] for q in cands]
        d = [[rd.frame_distortion(orc, px[p], W, H, q, orc.MODE_FULL, channels) for p in range(POOL)] for q in cands]
        return s, d
    return _once(("pool_table", channels, tuple(cands)), make)


def table(orc, channels=3, cands=K8):
    """(S[k][f], D[k][f]) of the batch.  Shared between the tests: read, never written."""
    def make():
        s, d = pool_table(orc, channels, cands)
        return [[row[p] for p in order()] for row in s], [[row[p] for p in order()] for row in d]
    return _once(("table", channels, tuple(cands)), make)


def records(orc, indices, qualities, channels=3, start=0):
    """The oracle's record of frames start, start + 1, ... of the batch, each at its own index and quality."""
    px = batch(channels)
    return [orc.encode_frame(px[start + j], W, H, int(i), int(q), orc.MODE_FULL, channels) for j, (i, q) in enumerate(zip(indices, qualities))]


def prefix(rows, n, start=0):
    return [row[start:n] for row in rows]


# ---- per-frame values: what makes an index taken "& 255", or from threadIdx.x alone, visible -------------------------------------
def axis_problem(v):
    """None when a per-frame list v [N] differs across every block edge, holds at least 6 distinct values in every block of 256
    frames and differs from v[f & 255] for at least half of the frames f >= 256; else what it lacks."""
    if len(v) != N:
        return "length"
    if any(v[e - 1] == v[e] for e in EDGES):
        return "equal across a block edge"
    if any(len(set(v[b:b + 256])) < 6 for b in range(0, N, 256)):
        return "fewer than 6 distinct values in a block"
    if 2 * sum(v[f] != v[f & 255] for f in range(256, N)) < N - 256:
        return "folds onto the first block"
    return None


def qualities():
    """[N] one quality per frame, 1 .. Q."""
    def make():
        for seed in range(32):
            q = [int(x) for x in np.random.default_rng(900 + seed).integers(1, Q + 1, N)]
            if axis_problem(q) is None:
                return q
        raise AssertionError("no draw of per-frame qualities crosses the block edges as the cases need")
    return _once("qualities", make)


def per_frame_model(S, D, rule, limits):
    """(picks [frame] = candidate index, the frames over their limit) of the three per-frame rules on a table."""
    picks, over = [], []
    for f, limit in enumerate(limits):
        s, d = [row[f] for row in S], [row[f] for row in D]
        if rule == LARGEST:
            k, o = rd.largest_that_fits(s, limit), min(s) > limit
        else:
            k, o = rd.pick(rule, s, d, limit)
        picks.append(k)
        if o:
            over.append(f)
    return picks, over


def per_frame_limits(orc, rule, channels=3):
    """(limits [N], picks, over): a limit per frame, drawn from the frame's own column of the table, under which the model's picks
    pass axis_problem and the only frame over its limit is the last one (so its status bit comes from the last workgroup)."""
    def make():
        S, D = table(orc, channels)
        bound = D if rule == rd.SMALLEST_AT_DISTORTION else S
        under = min(row[N - 1] for row in bound) - 1
        assert under >= 0, "the last frame needs a limit that nothing meets"
        for seed in range(32):
            ks = np.random.default_rng(1000 + seed).integers(0, len(S), N)
            limits = [bound[int(ks[f])][f] for f in range(N - 1)] + [under]
            picks, over = per_frame_model(S, D, rule, limits)
            if over == [N - 1] and axis_problem(picks) is None:
                return limits, picks, over
        raise AssertionError(f"no draw of per-frame limits gives rule {rule} the picks the cases need")
    return _once(("limits", rule, channels), make)


# ---- the bitrate walks: what makes a level that does not survive a chunk edge visible -------------------------------------------
def bitrate_walk(S, D, by, rate, cap, level, start=0, end=None):
    """(picks, frames over their level, the level afterwards) of frames [start, end) under the byte rule or the distortion rule."""
    end = len(S[0]) if end is None else end
    if by == BY_SIZE:
        picks, over, out = cbr_rule(prefix(S, end, start), rate, cap, level)
    else:
        picks, over, out = M.bitrate_walk(prefix(S, end, start), prefix(D, end, start), rate, cap, level)
    return picks, [f + start for f in over], out


def bitrate_problem(S, D, by, rate, cap, L0):
    """None when (rate, cap, L0) gives the walk over the batch what the cases need, else what it lacks: every chunk of 512 frames
    holds a refill clipped at the capacity and more than one pick; the level in front of frames 512 and 1024 is neither the initial
    one nor the capacity; a walk restarted from L0 at either frame picks otherwise than the true walk; and a frame fits nothing at
    a negative level whose debt later refills repay.

    That last condition can hold in the first chunk only, through a negative L0.  Behind a frame that fitted, the level is at
    least the rate.  It falls from there while frames fit nothing only if their smallest record exceeds the rate, and it rises
    again while nothing fits only if the rate exceeds the smallest record: a debt that arises past the start and is repaid needs a
    rate between the smallest records of two frames.  At 32 x 32 and quality factor 12 every picture's smallest record is the same
    78 bytes (tests/test_frame_axis_cpu.py pins it), so behind the first debt no further one can arise."""
    picks, over, _ = bitrate_walk(S, D, by, rate, cap, L0)
    over = set(over)
    before, L = [], min(L0, cap)                 # the level in front of every frame, and behind the last
    for f, k in enumerate(picks):
        before.append(L)
        L = min(cap, L - S[k][f] + rate)
    before.append(L)
    debts = [f for f in range(512) if before[f] < 0 and f in over]
    if not debts or max(before[debts[0] + 1:]) < 0:
        return "no frame that fits nothing at a negative level, or a debt that is never repaid"
    for lo in range(0, N, 512):
        hi = min(lo + 512, N)
        if not any(before[f] - S[picks[f]][f] + rate > cap for f in range(lo, hi)):
            return "a chunk without a clipped refill"
        if len(set(picks[lo:hi])) < 2:
            return "a chunk with one pick"
    for cut in (512, 1024):
        if before[cut] in (min(L0, cap), cap):
            return "the level in front of a chunk is the initial one, or the capacity"
        if bitrate_walk(S, D, by, rate, cap, L0, cut)[0] == picks[cut:]:
            return "a walk restarted at a chunk gives the same picks"
    return None


def bitrate_params(orc, by, channels=3):
    """(rate, capacity, L0) for the walk over the batch at K8; the search of _cbr_params (tests/test_gpu_rate.py) with the
    conditions of bitrate_problem.  L0 is a debt of four refills."""
    def make():
        S, D = table(orc, channels)
        sizes = sorted(x for row in S for x in row)
        lo, hi = sizes[0], sizes[-1]
        for rate in range(lo, hi, max(1, (hi - lo) // 48)):
            for cap in (3 * rate // 2, 2 * rate, 5 * rate // 4, 3 * rate):
                if bitrate_problem(S, D, by, rate, cap, -4 * rate) is None:
                    return rate, cap, -4 * rate
        raise AssertionError(f"no bitrate gives the {by} walk the cases it needs")
    return _once(("bitrate", by, channels), make)


# ---- the batch budgets ------------------------------------------------------------------------------------------------------------
def upgrades(s, top):
    """The upgrades top -> top + 1 that cost bytes, cheapest first: [(d, frame)]."""
    return sorted((s[top + 1][f] - s[top][f], f) for f in range(len(s[0])) if s[top + 1][f] > s[top][f])


def batch_budget_problem(s, budget):
    """None when batch_rule gives a mixed pick (top and top + 1) under which the last upgrade taken and the first one refused tie
    on d, and, beyond 1024 frames, one frame of that pair has an index >= 1024; else what is lacking."""
    n = len(s[0])
    pick, over = batch_rule(s, budget)
    if over or len(set(pick)) != 2:
        return "not a mixed pick"
    top = min(pick)
    order_ = upgrades(s, top)
    taken, refused = [x for x in order_ if pick[x[1]] == top + 1], [x for x in order_ if pick[x[1]] == top]
    if not taken or not refused:
        return "no upgrade taken, or none refused"
    if taken[-1][0] != refused[0][0]:
        return "the cut does not fall inside a tie"
    if n > 1024 and max(taken[-1][1], refused[0][1]) < 1024:
        return "the tie at the cut lies within the first 1024 frames"
    return None


def batch_budget(orc, n, channels=3):
    """(budget, picks) for the first n frames under the byte rule at K8: the cut in the middle of those batch_budget_problem
    accepts."""
    def make():
        s = prefix(table(orc, channels)[0], n)
        K, T = len(s), [sum(row) for row in s]
        for top in range(K - 1):
            order_ = upgrades(s, top)
            free = sum(s[top][f] - s[top + 1][f] for f in range(n) if s[top + 1][f] <= s[top][f])
            cuts, acc = [], 0
            for i in range(1, len(order_)):           # exactly the first i upgrades fit
                acc += order_[i - 1][0]
                budget = T[top] - free + acc
                tie = order_[i - 1][0] == order_[i][0] and (n <= 1024 or max(order_[i - 1][1], order_[i][1]) >= 1024)
                if tie and [k for k in range(K) if T[k] <= budget][-1:] == [top]:
                    cuts.append(budget)
            for budget in cuts[len(cuts) // 2:] + cuts[:len(cuts) // 2]:
                if batch_budget_problem(s, budget) is None:
                    return budget, batch_rule(s, budget)[0]
        raise AssertionError(f"no budget cuts the first {n} frames inside a tie")
    return _once(("batch_budget", n, channels), make)


def steps_taken(S, D, picks):
    """[frame] how many steps of its chain (rd_rate_model.chains) the frame took to reach its pick, and the chains' lengths."""
    ch = M.chains(S, D)
    return [c.index(k) for c, k in zip(ch, picks)], [len(c) - 1 for c in ch]


def rd_batch_problem(S, D, rule, limit):
    """None when rd_rate_model.batch_pick stays within the limit, takes a step of a frame in the last workgroup of 32 frames,
    takes two or more steps of some frame and leaves some step untaken; else what is lacking."""
    n = len(S[0])
    picks, over = M.batch_pick(S, D, rule, limit)
    if over:
        return "over the limit"
    at, length = steps_taken(S, D, picks)
    if not any(at[f] >= 1 for f in range(32 * ((n - 1) // 32), n)):
        return "no step taken in the last workgroup"
    if max(at) < 2:
        return "no frame takes two steps"
    if at == length:
        return "every step is taken"
    return None


def rd_batch_limit(orc, rule, n, channels=3):
    """(limit, picks) for the first n frames under a batch rule that picks by distortion, at K8."""
    def make():
        S, D = (prefix(t, n) for t in table(orc, channels))
        bound = S if rule == M.BEST_IN_BUDGET else D
        lo, hi = (sum(pick(row[f] for row in bound) for f in range(n)) for pick in (min, max))
        for i in (8, 6, 10, 4, 12, 5, 11, 3, 13, 7, 9, 2, 14, 1, 15):
            limit = lo + (hi - lo) * i // 16
            if rd_batch_problem(S, D, rule, limit) is None:
                return limit, M.batch_pick(S, D, rule, limit)[0]
        raise AssertionError(f"no limit gives rule {rule} on {n} frames the steps the cases need")
    return _once(("rd_batch", rule, n, channels), make)


# ---- stream spans -----------------------------------------------------------------------------------------------------------------
N_SPANS = 300
SPAN_LENGTHS = (0, 1, 7, 8, 9, 64, 65, 255, 257, 513)
# the non-empty spans of each table in batch order, and which of the 300 spans they are; every other span is empty
_SPANS = {
    "a": ((102, 1, 7, 8, 9, 64, 65, 100, 513, 64, 65, 9, 8, 7, 1, 77), (2, 3, 10, 11, 12, 63, 64, 255, 256, 257, 258, 270, 280, 290, 298, 299)),
    "b": ((255, 1, 7, 8, 9, 64, 65, 257, 255, 64, 65, 9, 8, 7, 1, 25), (0, 1, 5, 64, 65, 128, 200, 254, 256, 260, 261, 262, 263, 264, 265, 299)),
}
SPAN_TABLES = tuple(sorted(_SPANS))


def spans_problem(spans):
    """None when 300 spans tile the batch as the cases need (the lengths apart, which the two tables share out), else what is
    lacking."""
    if len(spans) != N_SPANS or sm.violation(spans, N) is not None:
        return "the spans do not tile the batch"
    if sum(1 for _, n, _ in spans if n == 0) < 200:
        return "fewer than 200 empty spans"
    if spans[256][1] == 0 or spans[299][1] == 0:
        return "span 256 or span 299 is empty"
    if not any(first == 256 and n > 0 for first, n, _ in spans):
        return "no span starts at frame 256"
    if not any(first < 512 < first + n - 1 and first != 256 for first, n, _ in spans):
        return "no other span straddles frame 512"
    index = sm.frame_indices(spans, N)
    if any((index[f] & 255) == (f & 255) for f in range(256, N)):
        return "a frame's index folds onto its place in the batch"
    return None


def spans(which):
    """[(first_frame, n_frames, first_frame_index)] of span table "a" or "b"."""
    def make():
        lengths, at = _SPANS[which]
        pairs = _pairs(N_SPANS, {s: n for n, s in zip(lengths, at)}, 1200 + ord(which))
        out = sm.spans_of(pairs)
        problem = spans_problem(out)
        assert problem is None, problem
        return out
    return _once(("spans", which), make)


def span_pairs(which):
    return [(n, index) for _, n, index in spans(which)]


# three streams for the bitrate encodes: a span longer than a chunk, an empty one and a span that starts inside a chunk
BITRATE_PAIRS = ((513, 250), (0, 7), (587, 1000))


def streams_bitrate_params(orc, by, channels=3):
    """(rates [(bytes_per_frame, buffer_bytes)] per stream, levels) for BITRATE_PAIRS: the batch's own (rate, capacity) and two
    variations of it, under which every non-empty stream's picks differ between frames and some frame fits nothing."""
    rate, cap, L0 = bitrate_params(orc, by, channels)
    rates = [(rate, cap), (rate // 2 + 1, cap), (rate + rate // 8, 2 * cap)]
    levels = [L0, 123, -rate]
    S, D = table(orc, channels)
    rule = sm.LARGEST_THAT_FITS if by == BY_SIZE else sm.LEAST_DISTORTION
    picks, _, _, bits = sm.streams_bitrate(S, D, sm.spans_of(BITRATE_PAIRS), rates, levels, rule)
    assert bits == sm.STATUS_OVER_BUDGET and len(set(picks[:513])) > 1 and len(set(picks[513:])) > 1
    return rates, levels


def _pairs(n_spans, lengths, seed):
    """(n_frames, first_frame_index) of n_spans spans, empty but for lengths {span: n_frames}; no frame's index folds onto its
    place in the batch modulo 256."""
    rng = np.random.default_rng(seed)
    pairs, first = [], 0
    for s in range(n_spans):
        index = int(rng.integers(0, 5000))
        index += ((index - first) & 255) == 0
        pairs.append((lengths.get(s, 0), index))
        first += lengths.get(s, 0)
    return pairs


def queued_batches():
    """[(first frame of the batch, its frames, its pairs)] of the two batches queued in pipelined mode: 300 frames in 40 spans and
    700 frames (three header workgroups) in 270 spans (two map workgroups), whose spans and indices have nothing in common."""
    out = [(0, 300, _pairs(40, {0: 255, 7: 1, 8: 44}, 1301)), (300, 700, _pairs(270, {3: 257, 100: 65, 256: 300, 269: 78}, 1302))]
    for _, n, pairs in out:
        assert sm.violation(sm.spans_of(pairs), n) is None
    assert out[0][1] + out[1][1] <= N
    return out
