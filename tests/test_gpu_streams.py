"""Batches of many streams on the GPU (include/mpeg1_hip.h "Streams"; csrc/m1v_streams.h; the definition in Python:
tests/streams_model.py).  Every record of a streams batch is the CPU oracle's for (the frame, its index in ITS stream, its
quality) and what per-stream encode(..., first_frame_index=...) calls give; the bitrate calls keep one leaky bucket per stream
and equal sequential calls of the existing bitrate encodes on the slices; the pick alone equals the model on synthetic tables.

Sizes are the smallest at which the kernels can go wrong: 64 x 48 pictures (one tile column, three strips), spans of 0 and 1
frames, an index that crosses 255 -> 256 inside a span, span lengths on both sides of the walk's step of eight, of a wave and of
512 frames, stream counts on both sides of a workgroup's four waves and of k_streams_map's 256 lanes per workgroup (not reached:
M1V_MAX_STREAMS spans need as many frames to be told apart, and 200 streams already take 50 workgroups)."""
import random

import numpy as np
import pytest

import input_families as fam
import streams_model as sm

pytestmark = pytest.mark.gpu

W, H, Q = 64, 48, 50
PAIRS = [(5, 0), (0, 77), (1, 1000), (8, 250), (9, 7)]          # 23 frames; 250 + 8 crosses 255 -> 256
FAMILIES = ["rgb", "rgba", "kt-surface-4-bgr-gap", "kp-planes-nv12"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _pixels(seed, n, channels):
    """A gradient under noise of amplitude 48: every frame its own picture, encodable at every quality <= 50."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (2 * x + 3 * y)[None, :, :, None] + 17 * np.arange(n)[:, None, None, None] + 40 * np.arange(channels)[None, None, None, :]
    return ((base + rng.integers(0, 48, (n, H, W, channels))) % 256).astype(np.uint8)


def _records(orc, px, indices, qualities):
    return [orc.encode_frame(px[f], W, H, indices[f], qualities[f], orc.MODE_FULL, px.shape[-1]) for f in range(len(indices))]


def _spans_tensor(torch, rows):
    """A StreamSpans of arbitrary rows (first_frame, n_frames, first_frame_index): what a caller's own kernel might write."""
    from ec504_imageencoder_amd import StreamSpans
    table = torch.tensor([list(r) + [0] for r in rows], dtype=torch.int32).cuda()
    return StreamSpans(table, [(r[1], r[2]) for r in rows])


def _split(data, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(data[at:at + s])
        at += s
    assert at == len(data)
    return out


# ---- 1. records ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_records_are_those_of_each_frame_at_its_own_index(torch_cuda, orc, family):
    from ec504_imageencoder_amd import stream_spans
    torch = torch_cuda
    n = sum(c for c, _ in PAIRS)
    channels = 4 if family in ("rgba", "kt-surface-4-bgr-gap") else 3
    px = _pixels(11, n, channels)
    inp = fam.build(torch, family, W, H, "full", Q, 32, pixels=px, orc=orc)
    enc = inp.enc
    spans = stream_spans(PAIRS)
    indices = sm.frame_indices(sm.spans_of(PAIRS), n)
    assert indices[14:23] == list(range(7, 16)) and 255 in indices and 256 in indices
    for quality in (None, [1 + (7 * f) % Q for f in range(n)]):
        qs = quality or [Q] * n
        want = _records(orc, px, indices, qs)
        data, sizes, stream_bytes = enc.encode_streams(inp.dev, spans, quality=quality)
        assert sizes == [len(r) for r in want]
        assert _split(data, sizes) == want
        assert stream_bytes == sm.stream_bytes(sm.spans_of(PAIRS), sizes) and stream_bytes[1] == 0
        # the concatenation of one plain call per stream on the same encoder
        per_stream = b""
        for first, count, index in sm.spans_of(PAIRS):
            if count:
                per_stream += enc.encode_to_bytes(inp.dev[first:first + count], index, quality=qs[first:first + count] if quality else None)[0]
        assert data == per_stream
    # pairs instead of the holder, and an empty batch
    assert enc.encode_streams(inp.dev, PAIRS)[0] == b"".join(_records(orc, px, indices, [Q] * n))
    data, sizes, stream_bytes = enc.encode_streams(inp.dev[:0], [(0, 5), (0, 9)])
    assert (data, sizes, stream_bytes) == (b"", [], [0, 0])
    enc.close()


# ---- 2. pipelined ----------------------------------------------------------------------------------------------------------------
def test_two_queued_batches_keep_their_own_indices(torch_cuda, orc):
    """Pipelined mode: batch 1 is queued while batch 0's assembly and finish are still in flight, each with its own spans.  The
    per-frame index array is one per counter set, so neither batch's headers come from the other's spans."""
    from ec504_imageencoder_amd import Mpeg1Encoder, stream_spans
    torch = torch_cuda
    pairs = ([(4, 300), (3, 40), (5, 9000)], [(1, 6), (6, 100), (0, 1), (2, 255)])
    px = [_pixels(21 + b, sum(c for c, _ in p), 3) for b, p in enumerate(pairs)]
    dev = [torch.from_numpy(p).cuda() for p in px]
    spans = [stream_spans(p) for p in pairs]
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=16)
    enc.set_pipelined(True)
    for _ in range(2):                                      # (twice: every Batch and both of its counter sets take a turn)
        results = [enc.encode_streams_device(dev[b], spans[b]) for b in range(2)]
        enc.flush()
        torch.cuda.synchronize()
        for b, (out, sizes, meta, stream_bytes) in enumerate(results):
            n = px[b].shape[0]
            want = _records(orc, px[b], sm.frame_indices(sm.spans_of(pairs[b]), n), [Q] * n)
            total, status = (int(x) for x in meta.cpu())
            assert status == 0 and total == sum(len(r) for r in want)
            assert out[:total].cpu().numpy().tobytes() == b"".join(want)
            assert [int(s) for s in sizes[:n].cpu()] == [len(r) for r in want]
            assert [int(s) for s in stream_bytes.cpu()] == sm.stream_bytes(sm.spans_of(pairs[b]), [len(r) for r in want])
    enc.close()


# ---- 3. out_cap one byte short ------------------------------------------------------------------------------------------------------
def test_a_batch_one_byte_too_long_keeps_the_records_that_fitted(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, stream_spans
    torch = torch_cuda
    n = sum(c for c, _ in PAIRS)
    px = _pixels(31, n, 3)
    dev = torch.from_numpy(px).cuda()
    want = _records(orc, px, sm.frame_indices(sm.spans_of(PAIRS), n), [Q] * n)
    total = sum(len(r) for r in want)
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=32)
    out = torch.full((total - 1 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    got, sizes, meta, stream_bytes = enc.encode_streams_device(dev, stream_spans(PAIRS), out=out[:total - 1])
    torch.cuda.synchronize()
    assert int(meta[1]) == _ffi.STATUS_NOSPACE and int(meta[0]) == total
    fitted = total - len(want[-1])
    host = out.cpu().numpy()
    assert host[:fitted].tobytes() == b"".join(want[:-1])                # headers included
    assert (host[total - 1:] == 0xA5).all()                              # nothing behind the capacity
    assert [int(s) for s in sizes[:n].cpu()] == [len(r) for r in want]
    assert [int(s) for s in stream_bytes.cpu()] == sm.stream_bytes(sm.spans_of(PAIRS), [len(r) for r in want])
    enc.close()


# ---- 4. bad spans --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,rows", [("gap", [(0, 3, 0), (4, 4, 0)]), ("overlap", [(0, 5, 0), (3, 5, 0)]), ("overrun", [(0, 12, 0)])])
def test_spans_that_do_not_tile_the_batch_set_the_status_bit(torch_cuda, orc, kind, rows):
    """n_frames = 8 on max_frames = 16; every claimed index stays below max_frames."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    n = 8
    assert sm.violation(rows, n) == kind and all(first + count <= 16 for first, count, _ in rows)
    px = _pixels(41, n, 3)
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=16)
    _, _, meta, _ = enc.encode_streams_device(dev, _spans_tensor(torch, rows))
    torch.cuda.synchronize()
    assert int(meta[1]) & _ffi.STATUS_STREAMS
    with pytest.raises(EncoderError) as ei:                              # the synchronous form reports it as an argument error
        enc.encode_streams(dev, _spans_tensor(torch, [(0, 3, 0), (4, 5, 0)]))
    assert ei.value.code == _ffi.E_ARG
    pairs = [(3, 254), (5, 0)]                                           # the next call on the same encoder is exact
    want = _records(orc, px, sm.frame_indices(sm.spans_of(pairs), n), [Q] * n)
    assert enc.encode_streams(dev, pairs)[0] == b"".join(want)
    enc.close()


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_a_failed_streams_call_leaves_the_encoder_correct(torch_cuda, orc, stage, pipelined):
    """m1v_debug_fail_encode reaches a streams encode at the stages of the plain encode (in front of the map, in front of
    k_assemble, behind k_streams_finish): the call returns E_HIP, and the next streams call and the next plain call are exact."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    pairs, n = [(3, 254), (0, 9), (4, 12)], 7
    px = _pixels(51, n, 3)
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=8)
    enc.set_pipelined(pipelined)
    want = _records(orc, px, sm.frame_indices(sm.spans_of(pairs), n), [Q] * n)
    assert enc.encode_streams(dev, pairs)[0] == b"".join(want)
    _ffi.lib().m1v_debug_fail_encode(stage)
    try:
        with pytest.raises(EncoderError) as ei:
            enc.encode_streams_device(dev, _spans_tensor(torch, sm.spans_of(pairs)))
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    enc.flush()
    torch.cuda.synchronize()
    assert enc.encode_streams(dev, pairs)[0] == b"".join(want)
    assert enc.encode_to_bytes(dev, 40)[0] == b"".join(_records(orc, px, list(range(40, 40 + n)), [Q] * n))
    enc.close()


# ---- 5. the pick on synthetic tables --------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 513)
MAX_FRAMES = 1200


@pytest.fixture(scope="module")
def pick_encoder(torch_cuda):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(16, 16, 12, "full", max_frames=MAX_FRAMES)
    yield enc
    enc.close()


def _lengths(rng, n_streams):
    """Span lengths drawn from LENGTHS, made to fit max_frames by shortening the longest; every case keeps a long span if it can."""
    out = [rng.choice(LENGTHS) for _ in range(n_streams)]
    if n_streams <= 3:
        out[0] = 513
    while sum(out) > MAX_FRAMES:
        i = out.index(max(out))
        out[i] = LENGTHS[LENGTHS.index(out[i]) - 1]
    return out


def _pick_case(seed, n_streams, K, rule):
    rng = random.Random(seed)
    lengths = _lengths(rng, n_streams)
    n = sum(lengths)
    spans = sm.spans_of([(c, rng.randrange(0, 5000)) for c in lengths])
    # non-monotone in k; a quarter of the frames large against every rate (debts that the refills of the small ones repay)
    S = [[rng.randrange(40, 400) * (8 if rng.random() < 0.25 else 1) for _ in range(n)] for _ in range(K)]
    D = [[rng.randrange(0, 1 << 40) for _ in range(n)] for _ in range(K)]
    for f in range(0, n, 5):                                # ties in D and in (D, s): the order falls to s, then to k
        for k in range(1, K):
            D[k][f] = D[0][f]
            if f % 10 == 0:
                S[k][f] = S[0][f]
    status = [0] * K
    if rule == sm.LEAST_DISTORTION and K > 1:
        status[rng.randrange(K)] = 1                        # an unencodable candidate: out of the running
    rates = [(rng.randrange(100, 900), rng.randrange(900, 6000)) for _ in lengths]
    levels = [rng.randrange(-3000, 7000) for _ in lengths]
    return spans, S, D, status, rates, levels


def _run_pick(torch, enc, spans, S, D, status, rates, levels, rule, alias=False):
    by = "size" if rule == sm.LARGEST_THAT_FITS else "distortion"
    n = len(S[0])
    d_S = torch.tensor(S, dtype=torch.int64).cuda().view(len(S), n)
    d_D = torch.tensor(D, dtype=torch.int64).cuda().view(len(S), n)
    d_status = torch.tensor(status, dtype=torch.int32).cuda()
    d_levels = torch.tensor(levels, dtype=torch.int64).cuda()
    r = torch.tensor([list(x) for x in rates], dtype=torch.int64).cuda()
    picks, dist, bits = enc.streams_bitrate_pick(d_S, d_D, _spans_tensor(torch, spans), r, None, d_levels, by=by, status=d_status,
                                                 levels_out=d_levels if alias else None)
    return picks, dist, [int(x) for x in d_levels.cpu()], bits


@pytest.mark.parametrize("rule", [sm.LARGEST_THAT_FITS, sm.LEAST_DISTORTION])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n_streams", [1, 3, 64, 65, 200])
def test_the_pick_equals_the_model(torch_cuda, pick_encoder, n_streams, K, rule):
    torch, enc = torch_cuda, pick_encoder
    spans, S, D, status, rates, levels = _pick_case(1000 * n_streams + 10 * K + rule, n_streams, K, rule)
    want = sm.streams_bitrate(S, D, spans, rates, levels, rule, status)
    got = _run_pick(torch, enc, spans, S, D, status, rates, levels, rule)
    assert got == (want[0], want[1], want[2], want[3])
    # level_out aliasing level_in
    assert _run_pick(torch, enc, spans, S, D, status, rates, levels, rule, alias=True) == got
    # two chained calls equal one: every span cut in two, the second call from the first call's levels
    cuts = [c // 2 for _, c, _ in spans]
    picks, now = [None] * len(S[0]), levels
    for frames, pairs in (([f for (first, _, _), c in zip(spans, cuts) for f in range(first, first + c)],
                           [(c, i) for (_, _, i), c in zip(spans, cuts)]),
                          ([f for (first, count, _), c in zip(spans, cuts) for f in range(first + c, first + count)],
                           [(count - c, i + c) for (_, count, i), c in zip(spans, cuts)])):
        if not frames:
            continue
        part = _run_pick(torch, enc, sm.spans_of(pairs), [[row[f] for f in frames] for row in S], [[row[f] for f in frames] for row in D],
                         status, rates, now, rule)
        for f, k in zip(frames, part[0]):
            picks[f] = k
        now = part[2]
    assert (picks, now) == (got[0], got[2])


@pytest.mark.parametrize("rule", [sm.LARGEST_THAT_FITS, sm.LEAST_DISTORTION])
def test_a_bad_rate_entry_and_bad_spans_in_the_pick(torch_cuda, pick_encoder, rule):
    torch, enc = torch_cuda, pick_encoder
    spans, S, D, status, rates, levels = _pick_case(77, 9, 3, rule)
    for s, bad in ((2, (0, 100)), (5, (500, 499)), (8, (1, 1 << 62))):
        rates[s] = bad
    want = sm.streams_bitrate(S, D, spans, rates, levels, rule, status)
    assert want[3] & sm.STATUS_STREAMS and [want[2][s] for s in (2, 5, 8)] == [levels[s] for s in (2, 5, 8)]
    assert _run_pick(torch, enc, spans, S, D, status, rates, levels, rule) == (want[0], want[1], want[2], want[3])
    # spans that do not tile the table's frames: the bit, and nothing outside the arrays (the guard behind the picks stays)
    n = len(S[0])
    rows = [(0, n // 2, 0), (n // 2 + 1, n, 0)]
    good = [(100, 1000)] * 2
    picks, _, _, bits = _run_pick(torch, enc, rows, S, D, status, good, [0, 0], rule)
    assert bits & sm.STATUS_STREAMS and len(picks) == n


def test_scalar_rates_and_a_size_table_without_distortion(torch_cuda, pick_encoder):
    """One rate for every stream (checked on the host), no distortion table under the byte rule, no table status."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch, enc = torch_cuda, pick_encoder
    spans, S, D, _, _, levels = _pick_case(5, 7, 4, sm.LARGEST_THAT_FITS)
    want = sm.streams_bitrate(S, None, spans, [(300, 2000)] * 7, levels, sm.LARGEST_THAT_FITS)
    d_S = torch.tensor(S, dtype=torch.int64).cuda()
    d_levels = torch.tensor(levels, dtype=torch.int64).cuda()
    picks, dist, bits = enc.streams_bitrate_pick(d_S, None, _spans_tensor(torch, spans), 300, 2000, d_levels)
    assert (picks, dist, [int(x) for x in d_levels.cpu()], bits) == (want[0], None, want[2], want[3])
    with pytest.raises(EncoderError) as ei:
        enc.streams_bitrate_pick(d_S, None, _spans_tensor(torch, spans), 300, 200, d_levels)
    assert ei.value.code == _ffi.E_ARG


# ---- 6. the bitrate encode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["size", "distortion"])
def test_the_bitrate_encode_equals_one_call_per_stream(torch_cuda, orc, by):
    """3 streams of 6, 0 and 9 frames, candidates (5, 25, 50), a rate per stream: bytes, sizes, chosen and levels are those of
    three sequential calls of the existing bitrate encode on the slices, and every record the oracle's at its picked quality."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    pairs, cands = [(6, 253), (0, 4), (9, 70)], (5, 25, 50)
    n = 15
    px = _pixels(61, n, 3)
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=16)
    table = enc.frame_size_table(dev, cands).cpu().numpy()
    mid = int(table[1].mean())
    rates, caps, start = [mid, mid, int(table[0].mean()) + 40], [3 * mid, 5 * mid, 2 * mid], [mid, 123, -mid]
    single = enc.encode_at_bitrate if by == "size" else enc.encode_best_at_bitrate
    want_data, want_sizes, want_chosen, want_levels, want_over = b"", [], [], [], False
    for s, (first, count, index) in enumerate(sm.spans_of(pairs)):
        level = torch.tensor([start[s]], dtype=torch.int64).cuda()
        res = single(dev[first:first + count], rates[s], caps[s], cands, level, first_frame_index=index)
        want_data += res[0]
        want_sizes += res[1]
        want_chosen += res[2]
        want_over |= bool(res[3])
        want_levels.append(int(level.item()))
    assert len(set(want_chosen)) > 1                                    # (the rates do make the picks differ)
    levels = torch.tensor(start, dtype=torch.int64).cuda()
    data, sizes, chosen, stream_bytes, over, dist = enc.encode_streams_at_bitrate(dev, pairs, cands, rates, caps, levels, by=by)
    assert (data, sizes, chosen, over) == (want_data, want_sizes, want_chosen, want_over)
    assert [int(x) for x in levels.cpu()] == want_levels and want_levels[1] == min(start[1], caps[1])
    assert stream_bytes == sm.stream_bytes(sm.spans_of(pairs), sizes)
    assert (dist is None) == (by == "size")
    assert _split(data, sizes) == _records(orc, px, sm.frame_indices(sm.spans_of(pairs), n), chosen)
    enc.close()
