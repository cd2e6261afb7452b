"""A byte budget or a distortion ceiling per stream as plain Python — TEST INFRASTRUCTURE ONLY (no tests in this module).

The definition is that of include/mpeg1_hip.h ("Streams: a budget per stream"): the picks of the frames of span s are what the
single-batch rule gives on the sub-table of that span's frames alone, with the span's own limit.  So this module states no rule:
it clamps the spans as tests/streams_model.py does and hands each span's columns to tests/rd_rate_model.py (batch_byte_rule,
batch_pick).  Tables are S[k][f], D[k][f] (lists of lists of ints); status, where given, is the table's status words."""
from rd_rate_model import BEST_IN_BUDGET, SMALLEST_AT_DISTORTION, batch_byte_rule, batch_pick
from streams_model import STATUS_OVER_BUDGET, STATUS_SCRATCH, STATUS_STREAMS, clamped, violation

STATUS_OVER_DISTORTION = 32
LARGEST_THAT_FITS, LEAST_DISTORTION, SMALLEST_AT_DISTORTION_PER_STREAM = 0, 1, 2
RULES = (LARGEST_THAT_FITS, LEAST_DISTORTION, SMALLEST_AT_DISTORTION_PER_STREAM)
OVER_BIT = {LARGEST_THAT_FITS: STATUS_OVER_BUDGET, LEAST_DISTORTION: STATUS_OVER_BUDGET,
            SMALLEST_AT_DISTORTION_PER_STREAM: STATUS_OVER_DISTORTION}


def span_pick(S, D, rule, limit, status=None):
    """(picks, over) of the single-batch rule that `rule` names, on one span's sub-table."""
    if rule == LARGEST_THAT_FITS:
        return batch_byte_rule(S, limit)
    return batch_pick(S, D, BEST_IN_BUDGET if rule == LEAST_DISTORTION else SMALLEST_AT_DISTORTION, limit, status)


def streams_budget(S, D, spans, limits, rule, status=None):
    """(picks [frame] = candidate index, the picks' distortion or None without D, [stream] its over bit or 0, the batch's status
    bits).  limits: one per span.  A frame that no clamped span covers is at candidate 0; with spans that overlap, the later span's
    picks stand here (the library leaves them unspecified)."""
    K, n = len(S), (len(S[0]) if S else 0)
    picks, stream_status, bits = [0] * n, [], 0
    if n > 0 and status is not None and any(int(w) & STATUS_SCRATCH for w in status[:K]):
        bits |= STATUS_SCRATCH
    if violation(spans, n) is not None:
        bits |= STATUS_STREAMS
    for span, limit in zip(spans, limits):
        lo, hi = clamped(span, n)
        got, over = span_pick([row[lo:hi] for row in S], [row[lo:hi] for row in D] if D is not None else None, rule, limit, status)
        picks[lo:hi] = got
        stream_status.append(OVER_BIT[rule] if over else 0)
        bits |= stream_status[-1]
    dist = [D[k][f] for f, k in enumerate(picks)] if D is not None else None
    return picks, dist, stream_status, bits
