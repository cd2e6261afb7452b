"""Batches of many streams as plain Python — TEST INFRASTRUCTURE ONLY (no tests in this module).

The definition is that of include/mpeg1_hip.h ("Streams"): a batch of n frames is the concatenation of spans
(first_frame, n_frames, first_frame_index); the bitrate calls keep one leaky bucket per stream, which is the bucket of
tests/rd_rate_model.py (bitrate_byte_rule, bitrate_walk) applied to the span's columns of the table.  Tables are S[k][f], D[k][f]
(lists of lists of ints); status, where given, is the table's status words, one per candidate."""
from rd_rate_model import bitrate_byte_rule, bitrate_walk

STATUS_SCRATCH, STATUS_OVER_BUDGET, STATUS_STREAMS = 4, 16, 64
MAX_STREAMS = 4096
LARGEST_THAT_FITS, LEAST_DISTORTION = 0, 1


def spans_of(pairs):
    """[(first_frame, n_frames, first_frame_index)] of the spans that (n_frames, first_frame_index) pairs make back to back."""
    out, at = [], 0
    for n, index in pairs:
        out.append((at, n, index))
        at += n
    return out


def violation(spans, n_frames):
    """The tiling rule: span 0 starts at 0, span s + 1 where span s ends, the last span ends at n_frames.  None when the spans
    keep it, else what the first span that breaks it does: "start" (span 0 not at 0), "gap", "overlap" (against the span in
    front), "overrun" or "short" (the last span ends behind or in front of n_frames)."""
    at = 0
    for s, (first, n, _) in enumerate(spans):
        if first != at:
            return "start" if s == 0 else ("gap" if first > at else "overlap")
        at = first + n
    return None if at == n_frames else ("overrun" if at > n_frames else "short")


def clamped(span, n_frames):
    """The frames [lo, hi) of the batch a span addresses: every index is clamped into [0, n_frames]."""
    first, n, _ = span
    return min(first, n_frames), min(first + n, n_frames)


def frame_indices(spans, n_frames):
    """[frame] the index of the frame in its stream (spans that keep the tiling rule cover every frame once)."""
    out = [None] * n_frames
    for span in spans:
        lo, hi = clamped(span, n_frames)
        for f in range(lo, hi):
            out[f] = span[2] + (f - span[0])
    return out


def stream_bytes(spans, sizes):
    return [sum(sizes[f] for f in range(*clamped(span, len(sizes)))) for span in spans]


def rate_ok(rate, cap):
    return 1 <= rate <= cap < 2 ** 62


def streams_bitrate(S, D, spans, rates, levels, rule, status=None):
    """One leaky bucket per stream over spans that keep the tiling rule.  rates: [(bytes_per_frame, buffer_bytes)] per stream.
    Returns (picks [frame] = candidate index, the picks' distortion or None without D, the levels after the batch, status bits).
    A stream whose rate entry is outside 1 <= r <= C < 2^62: its frames at candidate 0, its level as it came, STATUS_STREAMS."""
    K, n = len(S), (len(S[0]) if S else 0)
    picks, levels_out, bits = [None] * n, [], 0
    if n > 0 and status is not None and any(int(w) & STATUS_SCRATCH for w in status[:K]):
        bits |= STATUS_SCRATCH
    if violation(spans, n) is not None:
        bits |= STATUS_STREAMS
    for span, (rate, cap), level in zip(spans, rates, levels):
        lo, hi = clamped(span, n)
        if not rate_ok(rate, cap):
            bits |= STATUS_STREAMS
            picks[lo:hi] = [0] * (hi - lo)
            levels_out.append(level)
            continue
        Ss = [row[lo:hi] for row in S]
        if rule == LARGEST_THAT_FITS:
            got, over, after = bitrate_byte_rule(Ss, rate, cap, level)
        else:
            got, over, after = bitrate_walk(Ss, [row[lo:hi] for row in D], rate, cap, level, status)
        picks[lo:hi] = got
        levels_out.append(after)
        if over:
            bits |= STATUS_OVER_BUDGET
    dist = [D[k][f] if k is not None else None for f, k in enumerate(picks)] if D is not None else None
    return picks, dist, levels_out, bits
