"""The synthetic tables, spans and limits of the per-stream budget pick — TEST INFRASTRUCTURE ONLY (no tests in this module).

Shared by tests/test_streams_budget_cpu.py (which counts, with the model alone, what the cases exercise) and
tests/test_gpu_streams_budget.py (which runs them on the device).  Span lengths sit on and beside the pick kernel's chunk of 32
frames and its stage of 256 slots (= 32 frames) and 256 keys; each span's limit is drawn from the model's own numbers for that span,
so that both sides of every comparison in the kernel are hit."""
import random

import rd_rate_model as rm
import streams_budget_model as bm
import streams_model as sm

LENGTHS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)
MAX_FRAMES = 1100
U64 = 2 ** 64 - 1
STREAM_COUNTS = (1, 3, 64, 65, 200)
KS = (1, 3, 8)


def lengths_for(rng, n_streams):
    """Span lengths from LENGTHS that fit MAX_FRAMES (the longest is shortened until they do); one span takes all 1100 frames."""
    if n_streams == 1:
        return [MAX_FRAMES]
    out = [rng.choice(LENGTHS) for _ in range(n_streams)]
    if n_streams <= 3:
        out[0], out[1] = 513, 257
    while sum(out) > MAX_FRAMES:
        i = out.index(max(out))
        out[i] = LENGTHS[LENGTHS.index(out[i]) - 1]
    return out


def tables(rng, n, K, rule, huge=False):
    """S mostly growing with k, every ninth frame not (non-monotone in k); D falling with k on average, up to 2^40 (huge: just
    below 2^63, so that three frames' sum passes 2^64); ties in D and in (D, s) every fifth frame; under the two rules that pick
    by distortion one candidate cannot be coded."""
    S = [[0] * n for _ in range(K)]
    D = [[0] * n for _ in range(K)]
    for f in range(n):
        base = rng.randrange(40, 400) * (8 if rng.random() < 0.25 else 1)
        for k in range(K):
            S[k][f] = rng.randrange(40, 3200) if f % 9 == 4 else base * (k + 1) + rng.randrange(0, 40)
            D[k][f] = (1 << 63) - 1 - rng.randrange(0, 1 << 40) * (k + 1) if huge else rng.randrange(0, 1 << 40) >> k
    for f in range(0, n, 5):
        for k in range(1, K):
            D[k][f] = D[0][f]
            if f % 10 == 0:
                S[k][f] = S[0][f]
    status = [0] * K
    if rule != bm.LARGEST_THAT_FITS and K > 1:
        status[rng.randrange(K)] = 1
    return S, D, status


def span_numbers(S, D, rule, status):
    """What the model computes on one span's sub-table, for the limits: (start, the first step's cost, everything).  Byte rules:
    bytes at the start, of the first step, with every step taken.  Distortion rule: the distortion at the start, the first step's
    gain, the distortion with every step taken."""
    K, n = len(S), len(S[0])
    if rule == bm.LARGEST_THAT_FITS:
        T = [sum(row) for row in S]
        k = min(range(K), key=lambda q: (T[q], q))
        first = None
        if k + 1 < K:
            d = [S[k + 1][f] - S[k][f] for f in range(n)]
            pos = [x for x in d if x > 0]
            first = min(pos) - sum(-x for x in d if x < 0) if pos else None
        return T[k], first, max(T)
    ch = rm.chains(S, D, status)
    order = rm.steps(S, D, ch)
    if rule == bm.LEAST_DISTORTION:
        start = sum(S[c[0]][f] for f, c in enumerate(ch))
        return start, order[0][2] if order else None, start + sum(t[2] for t in order)
    start = sum(D[c[0]][f] for f, c in enumerate(ch))
    return start, order[0][3] if order else None, start - sum(t[3] for t in order)


def limit_for(rng, S, D, rule, status):
    """One limit for a non-empty span, from the model's numbers for it: 0; start - 1; start; start + the first step's cost - 1 and
    exactly that; everything; 2^64 - 1; random values in between.  For the distortion ceiling the same, mirrored: the start is
    the most distortion and every step lowers it."""
    start, first, everything = span_numbers(S, D, rule, status)
    first = first if first is not None else 0
    lo, hi = min(start, everything), max(start, everything)
    if rule == bm.SMALLEST_AT_DISTORTION_PER_STREAM:
        options = [0, everything - 1, everything, start - first + 1, start - first, start, U64, rng.randint(lo, hi), rng.randint(lo, hi)]
    else:
        options = [0, start - 1, start, start + first - 1, start + first, everything, U64, rng.randint(lo, hi), rng.randint(lo, hi)]
    return min(max(rng.choice(options), 0), U64)


def case(seed, n_streams, K, rule, lengths=None, huge=False):
    """(spans, S, D, status, limits) of one case; spans as (first_frame, n_frames, first_frame_index)."""
    rng = random.Random(seed)
    lengths = lengths if lengths is not None else lengths_for(rng, n_streams)
    n = sum(lengths)
    spans = sm.spans_of([(c, rng.randrange(0, 5000)) for c in lengths])
    S, D, status = tables(rng, n, K, rule, huge)
    limits = []
    for span in spans:
        lo, hi = sm.clamped(span, n)
        limits.append(limit_for(rng, [row[lo:hi] for row in S], [row[lo:hi] for row in D], rule, status) if hi > lo else rng.choice((0, 77, U64)))
    return spans, S, D, status, limits


def sparse_lengths(seed):
    """4096 spans, most of them empty: every 61st holds a few frames."""
    rng = random.Random(seed)
    return [rng.choice((1, 7, 9, 33)) if s % 61 == 7 else 0 for s in range(sm.MAX_STREAMS)]


def case_ids():
    """[(id, arguments of case())] of every case the GPU test runs, per rule."""
    out = []
    for rule in bm.RULES:
        for K in KS:
            for n_streams in STREAM_COUNTS:
                out.append((f"rule{rule}-K{K}-streams{n_streams}", (1000 * n_streams + 10 * K + rule, n_streams, K, rule)))
        out.append((f"rule{rule}-K8-streams4096", (4096 + rule, sm.MAX_STREAMS, 8, rule, sparse_lengths(rule))))
        if rule != bm.LARGEST_THAT_FITS:
            out.append((f"rule{rule}-K3-near-2^63", (63 + rule, 9, 3, rule, [3, 0, 33, 7, 1, 65, 9, 32, 8], True)))
    return out


def census_class(S, D, rule, limit, status, picks, over):
    """Which of "over", "none", "some", "all" a non-empty span's result is: over its limit, no step taken, some, every one.  Byte
    rule: the steps are the upgrades that cost bytes from the level every frame reaches to the next; "all" is every frame at the
    last candidate."""
    K, n = len(S), len(S[0])
    if over:
        return "over"
    if rule == bm.LARGEST_THAT_FITS:
        if all(k == K - 1 for k in picks):
            return "all"
        top = min(picks)
        return "some" if any(k == top + 1 and S[top + 1][f] > S[top][f] for f, k in enumerate(picks)) else "none"
    ch = rm.chains(S, D, status)
    taken = sum(c.index(picks[f]) for f, c in enumerate(ch))
    total = sum(len(c) - 1 for c in ch)
    return "none" if taken == 0 else ("all" if taken == total else "some")
