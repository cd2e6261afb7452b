"""A byte budget or a distortion ceiling per stream on the GPU (include/mpeg1_hip.h "Streams: a budget per stream";
csrc/m1v_span_budget.h; the definition in Python: tests/streams_budget_model.py, a composition of the single-batch models).

The pick runs alone on synthetic tables (tests/streams_budget_cases.py; tests/test_streams_budget_cpu.py counts what they
exercise): span lengths on and beside the kernel's chunk of 32 frames and stage of 256 slots, one span of all 1100 frames, 1 to
4096 streams, K of 1, 3 and 8, limits on both sides of every comparison.  The encodes run on 32 x 32 noise pictures, 40 frames
in spans of 0, 1, 9, 17 and 13 frames: every record is the oracle's and encode_streams' at the picked quality."""
import random

import numpy as np
import pytest

import rd_rate_model as rm
import streams_budget_cases as cases
import streams_budget_model as bm
import streams_model as sm

pytestmark = pytest.mark.gpu

CASES = cases.case_ids()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def pick_encoder(torch_cuda):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(16, 16, 12, "full", max_frames=cases.MAX_FRAMES)
    yield enc
    enc.close()


def _spans_tensor(torch, rows):
    """A StreamSpans of arbitrary rows (first_frame, n_frames, first_frame_index): what a caller's own kernel might write."""
    from ec504_imageencoder_amd import StreamSpans
    table = torch.tensor([[x - 2 ** 32 if x >= 2 ** 31 else x for x in r] + [0] for r in rows], dtype=torch.int32).cuda()
    return StreamSpans(table, [(r[1], r[2]) for r in rows])


def _device_table(torch, rows):
    n = len(rows[0])
    return torch.tensor(rows, dtype=torch.int64).cuda().view(len(rows), n)


def _run_pick(torch, enc, spans, S, D, status, limits, rule):
    d_status = torch.tensor(status, dtype=torch.int32).cuda() if status is not None else None
    return enc.streams_budget_pick(_device_table(torch, S), _device_table(torch, D) if D is not None else None,
                                   _spans_tensor(torch, spans), rule, limits, status=d_status)


# ---- 1. the pick equals the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [a for _, a in CASES], ids=[i for i, _ in CASES])
def test_the_pick_equals_the_model(torch_cuda, pick_encoder, args):
    spans, S, D, status, limits = cases.case(*args)
    want = bm.streams_budget(S, D, spans, limits, args[3], status)
    got = _run_pick(torch_cuda, pick_encoder, spans, S, D, status, limits, args[3])
    assert got[3] == want[2]                                 # per stream
    assert got[2] == want[3]                                 # the batch's word
    assert got[0] == want[0] and got[1] == want[1]


# ---- 2. each span against the single-batch pick of the library itself ----------------------------------------------------------
@pytest.mark.parametrize("rule", bm.RULES)
def test_each_span_equals_the_existing_batch_pick_on_its_slice(torch_cuda, pick_encoder, rule):
    """Nine spans: under the two rules that pick by distortion every span's picks are what rd_batch_pick (k_rd_chains and
    k_rd_batch_pick, the code this feature leaves alone) returns for the span's columns and limit; the byte rule has no pick-only
    call, so its spans are compared with rd_rate_model.batch_byte_rule."""
    torch, enc = torch_cuda, pick_encoder
    spans, S, D, status, limits = cases.case(909 + rule, 9, 8, rule, lengths=[33, 0, 257, 9, 1, 64, 255, 32, 8])
    picks, _, _, stream_status = _run_pick(torch, enc, spans, S, D, status, limits, rule)
    d_S, d_D = _device_table(torch, S), _device_table(torch, D)
    d_status = torch.tensor(status, dtype=torch.int32).cuda()
    for s, span in enumerate(spans):
        lo, hi = sm.clamped(span, len(S[0]))
        if hi == lo:
            assert stream_status[s] == 0
        elif rule == bm.LARGEST_THAT_FITS:
            want, over = rm.batch_byte_rule([row[lo:hi] for row in S], limits[s])
            assert (picks[lo:hi], bool(stream_status[s])) == (want, over)
        else:
            want, over = enc.rd_batch_pick(d_S[:, lo:hi].contiguous(), d_D[:, lo:hi].contiguous(),
                                           rm.BEST_IN_BUDGET if rule == bm.LEAST_DISTORTION else rm.SMALLEST_AT_DISTORTION, limits[s], d_status)
            assert (picks[lo:hi], bool(stream_status[s])) == (want, over), s


# ---- 3. bad spans ----------------------------------------------------------------------------------------------------------------
BAD = [("gap", [(0, 40, 0), (45, 55, 0)]), ("overlap", [(0, 70, 0), (40, 60, 0)]), ("overrun", [(0, 33, 0), (33, 200, 0)]),
       ("overrun", [(0, 100, 0), (100, 0xFFFFFFFF, 0)]), ("gap", [(0, 10, 0), (0xFFFFFFF0, 90, 0)])]


@pytest.mark.parametrize("rule", bm.RULES)
@pytest.mark.parametrize("kind,rows", BAD)
def test_bad_spans_set_the_bit_and_touch_nothing_outside(torch_cuda, pick_encoder, kind, rows, rule):
    """100 frames under spans that do not tile them (the defined, clamped case): M1V_STATUS_STREAMS, every pick below K, the frames
    no clamped span covers at candidate 0, and the guards around the picks, their distortions and the streams' words as they were."""
    from ec504_imageencoder_amd.encoder import _call, _ptr, _stream
    torch, enc = torch_cuda, pick_encoder
    n, K, G = 100, 3, 64
    assert sm.violation(rows, n) == kind
    _, S, D, status, _ = cases.case(31 + rule, 2, K, rule, lengths=[60, 40])
    d_S, d_D = _device_table(torch, S), _device_table(torch, D)
    d_status = torch.tensor(status, dtype=torch.int32).cuda()
    limits = torch.tensor([sum(S[1]), 1 << 62], dtype=torch.int64).cuda()
    picks = torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    pick_dist = torch.full((n + 2 * G,), -7, dtype=torch.int64, device="cuda")
    words = torch.full((2 + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    spans = _spans_tensor(torch, rows)
    _call("m1v_streams_budget_pick_device", enc._h, _ptr(d_S), _ptr(d_D), _ptr(d_status), n, K, _ptr(spans), 2, rule, 0, _ptr(limits),
          _ptr(picks[G:]), _ptr(pick_dist[G:]), _ptr(words[G:]), _ptr(word), _stream())
    torch.cuda.synchronize()
    assert int(word.item()) & sm.STATUS_STREAMS
    got = picks.cpu().numpy()
    assert (got[:G] == 0xA5).all() and (got[G + n:] == 0xA5).all() and (got[G:G + n] < K).all()
    covered = set()
    for row in rows:
        covered.update(range(*sm.clamped(row, n)))
    assert all(got[G + f] == 0 for f in range(n) if f not in covered)
    dist = pick_dist.cpu().numpy()
    assert (dist[:G] == -7).all() and (dist[G + n:] == -7).all()
    w = words.cpu().numpy()
    assert (w[:G] == 0x5A5A5A5A).all() and (w[G + 2:] == 0x5A5A5A5A).all()
    assert all(int(x) in (0, bm.OVER_BIT[rule]) for x in w[G:G + 2])
    # the next call on the same encoder, with good spans, is the model's
    spans, S, D, status, limits = cases.case(31 + rule, 2, K, rule, lengths=[60, 40])
    want = bm.streams_budget(S, D, spans, limits, rule, status)
    assert _run_pick(torch, enc, spans, S, D, status, limits, rule) == (want[0], want[1], want[3], want[2])


# ---- 4. the other argument forms ----------------------------------------------------------------------------------------------------
def test_a_scalar_limit_no_distortion_table_and_no_table_status(torch_cuda, pick_encoder):
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch, enc = torch_cuda, pick_encoder
    spans, S, D, _, _ = cases.case(5, 7, 4, bm.LARGEST_THAT_FITS, lengths=[33, 9, 0, 64, 1, 31, 8])
    limit = sum(S[0][:33])
    want = bm.streams_budget(S, None, spans, [limit] * 7, bm.LARGEST_THAT_FITS)
    assert len(set(want[2])) == 2 and len(set(want[0])) > 1          # (some streams are over this limit, some not)
    assert _run_pick(torch, enc, spans, S, None, None, limit, bm.LARGEST_THAT_FITS) == (want[0], None, want[3], want[2])
    # the same limit as a CUDA tensor and as a sequence; and with a distortion table the picks' distortions come too
    as_tensor = torch.tensor([limit] * 7, dtype=torch.int64).cuda()
    assert _run_pick(torch, enc, spans, S, None, None, as_tensor, bm.LARGEST_THAT_FITS)[0] == want[0]
    with_d = bm.streams_budget(S, D, spans, [limit] * 7, bm.LARGEST_THAT_FITS)
    assert _run_pick(torch, enc, spans, S, D, None, [limit] * 7, bm.LARGEST_THAT_FITS) == (with_d[0], with_d[1], with_d[3], with_d[2])
    for rule in (bm.LEAST_DISTORTION, bm.SMALLEST_AT_DISTORTION_PER_STREAM):
        scalar = limit if rule == bm.LEAST_DISTORTION else sum(D[1][:33])
        want = bm.streams_budget(S, D, spans, [scalar] * 7, rule)
        assert _run_pick(torch, enc, spans, S, D, None, scalar, rule) == (want[0], want[1], want[3], want[2])
        with pytest.raises(EncoderError) as ei:                       # these two rules need the distortion table
            _run_pick(torch, enc, spans, S, None, None, scalar, rule)
        assert ei.value.code == _ffi.E_ARG
    with pytest.raises(EncoderError) as ei:
        _run_pick(torch, enc, spans, S, D, None, limit, 3)
    assert ei.value.code == _ffi.E_ARG
    # an empty table: every span is empty, nothing is over
    from ec504_imageencoder_amd.encoder import _call, _ptr, _stream
    table = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    picks = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
    words = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    _call("m1v_streams_budget_pick_device", enc._h, _ptr(table), _ptr(table), None, 0, 4, _ptr(_spans_tensor(torch, [(0, 0, 0)] * 3)), 3,
          bm.LEAST_DISTORTION, 0, None, _ptr(picks), None, _ptr(words[1:]), _ptr(words), _stream())
    torch.cuda.synchronize()
    assert [int(x) for x in words.cpu()] == [0, 0, 0, 0] and (picks.cpu().numpy() == 0xA5).all()


# ---- 5. the encodes ---------------------------------------------------------------------------------------------------------------
W = H = 32
Q = 12
CANDS = (2, 5, 8, 12)
PAIRS = [(0, 40), (1, 255), (9, 7), (17, 1000), (13, 250)]              # 40 frames; 250 + 13 crosses 255 -> 256


def _pixels(seed, n):
    """Noise of an amplitude that grows with the frame around a flat grey: records and distortions differ widely."""
    rng = np.random.default_rng(seed)
    amp = 4 + 6 * np.arange(n)[:, None, None, None]
    return np.clip(128 + rng.integers(-1, 2, (n, H, W, 3)) * rng.integers(0, 1 + amp, (n, H, W, 3)), 0, 255).astype(np.uint8)


def _limits(S, D, spans, rule):
    """Per span, from the model's numbers on the table: [-, over, one step, in between, everything] for the spans of PAIRS."""
    out = []
    for s, span in enumerate(spans):
        lo, hi = sm.clamped(span, len(S[0]))
        if hi == lo:
            out.append(77)
            continue
        start, first, everything = cases.span_numbers([r[lo:hi] for r in S], [r[lo:hi] for r in D], rule, None)
        first = first or 0
        ceiling = rule == bm.SMALLEST_AT_DISTORTION_PER_STREAM
        out.append([None, everything - 1 if ceiling else start - 1, start - first if ceiling else start + first, (start + everything) // 2,
                    everything][s])
    return [max(x, 0) for x in out]


def _records(orc, px, indices, qualities):
    return [orc.encode_frame(px[f], W, H, indices[f], qualities[f], orc.MODE_FULL, 3) for f in range(len(indices))]


def _encode(enc, dev, pairs, rule, limits):
    if rule == bm.SMALLEST_AT_DISTORTION_PER_STREAM:
        return enc.encode_streams_to_distortion(dev, pairs, CANDS, limits)
    return enc.encode_streams_to_budget(dev, pairs, CANDS, limits, by="size" if rule == bm.LARGEST_THAT_FITS else "distortion")


def _check_encode(enc, dev, px, orc, torch, pairs, rule, table_of=None):
    """One encode with a budget per stream against the model on frame_rd_table of the same frames, encode_streams and the oracle."""
    n = px.shape[0]
    spans = sm.spans_of(pairs)
    sizes, dist = (t.cpu().tolist() for t in enc.frame_rd_table(table_of if table_of is not None else dev, CANDS))
    limits = _limits(sizes, dist, spans, rule)
    want_picks, want_dist, want_stream_status, want_bits = bm.streams_budget(sizes, dist, spans, limits, rule)
    assert 0 < sum(1 for w in want_stream_status if w) < len(spans) and len(set(want_picks)) > 1
    data, got_sizes, chosen, stream_bytes, over, got_dist, stream_status = _encode(enc, dev, pairs, rule, limits)
    assert chosen == [CANDS[k] for k in want_picks]
    assert stream_status == want_stream_status and over == bool(want_bits & bm.OVER_BIT[rule])
    assert got_sizes == [sizes[k][f] for f, k in enumerate(want_picks)]
    assert got_dist == (None if rule == bm.LARGEST_THAT_FITS else want_dist)
    assert stream_bytes == sm.stream_bytes(spans, got_sizes)
    if rule != bm.SMALLEST_AT_DISTORTION_PER_STREAM:
        assert all(b <= L for b, L, w in zip(stream_bytes, limits, stream_status) if not w)
    want = _records(orc, px, sm.frame_indices(spans, n), chosen)
    assert data == b"".join(want)
    assert data == enc.encode_streams(dev, pairs, quality=chosen)[0]
    return limits, data


@pytest.mark.parametrize("rule", bm.RULES)
def test_the_encode_on_packed_frames(torch_cuda, orc, rule):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    px = _pixels(71, 40)
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=40)
    assert enc.size_table_fused
    _check_encode(enc, dev, px, orc, torch, PAIRS, rule)
    # limits as one scalar for every stream, and an empty batch
    scalar = _encode(enc, dev, PAIRS, rule, 1 << 40)
    assert scalar[6] == [0] * 5 and not scalar[4]
    empty = _encode(enc, dev[:0], [(0, 5), (0, 9)], rule, [0, 0])
    assert (empty[0], empty[1], empty[2], empty[3], empty[4], empty[6]) == (b"", [], [], [0, 0], False, [0, 0])
    enc.close()


def test_the_encode_through_a_frame_table(torch_cuda, orc):
    """The frames at separate addresses, in another order than they were allocated in: the pick never sees pixels."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    px = _pixels(72, 40)
    pool = [torch.from_numpy(px[f]).cuda() for f in reversed(range(40))]
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=40)
    enc.set_input_layout(W * 3)
    enc.set_frame_table(True)
    table = enc.frames(pool[::-1])
    _check_encode(enc, table, px, orc, torch, PAIRS, bm.LEAST_DISTORTION)
    enc.close()


def test_the_encode_on_another_stream(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    px = _pixels(73, 40)
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=40)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _check_encode(enc, dev, px, orc, torch, PAIRS, bm.SMALLEST_AT_DISTORTION_PER_STREAM)
    torch.cuda.synchronize()
    enc.close()


def test_two_queued_batches_keep_their_own_spans_and_limits(torch_cuda, orc):
    """Pipelined mode: batch 1 is queued behind batch 0 with other frames, spans, limits and another rule, with no host wait
    between them."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, stream_spans
    from ec504_imageencoder_amd.encoder import _call, _meta_ptrs, _ptr, _stream
    torch = torch_cuda
    pairs = (PAIRS, [(20, 3), (0, 9), (11, 254), (9, 77)])
    rules = (bm.LEAST_DISTORTION, bm.LARGEST_THAT_FITS)
    px = [_pixels(74 + b, 40) for b in range(2)]
    dev = [torch.from_numpy(p).cuda() for p in px]
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=40)
    want = []
    for b in range(2):                                      # the tables, the limits and the model first, outside pipelined mode
        sizes, dist = (t.cpu().tolist() for t in enc.frame_rd_table(dev[b], CANDS))
        spans = sm.spans_of(pairs[b])
        limits = [max(x, 0) for x in (cases.limit_for(random.Random(b * 10 + s), [r[lo:hi] for r in sizes], [r[lo:hi] for r in dist],
                                                      rules[b], None) if hi > lo else 5
                                      for s, (lo, hi) in enumerate(sm.clamped(sp, 40) for sp in spans))]
        want.append((limits,) + bm.streams_budget(sizes, dist, spans, limits, rules[b]))
    enc.set_pipelined(True)
    cand_buf = enc._candidates(CANDS, "test")
    for _ in range(2):                                      # (twice: every Batch and both of its counter sets take a turn)
        results = []
        for b in range(2):
            spans = stream_spans(pairs[b])
            d_limits = torch.tensor([x - 2 ** 64 if x >= 2 ** 63 else x for x in want[b][0]], dtype=torch.int64).cuda()   # (uint64 bit patterns)
            out = torch.empty(enc.default_out_capacity(40), dtype=torch.uint8, device="cuda")
            sizes_t = torch.zeros(40, dtype=torch.int64, device="cuda")
            chosen = torch.zeros(40, dtype=torch.uint8, device="cuda")
            dist_t = torch.zeros(40, dtype=torch.int64, device="cuda")
            stream_bytes = torch.zeros(len(spans), dtype=torch.int64, device="cuda")
            stream_status = torch.full((len(spans),), -1, dtype=torch.int32, device="cuda")
            meta = torch.zeros(2, dtype=torch.int64, device="cuda")
            _call("m1v_encode_streams_budget_device", enc._h, _ptr(dev[b]), 40, _ptr(spans), len(spans), cand_buf, len(cand_buf), rules[b],
                  0, _ptr(d_limits), _ptr(chosen), _ptr(out), out.numel(), _ptr(sizes_t), _ptr(dist_t), _ptr(stream_bytes),
                  _ptr(stream_status), *_meta_ptrs(meta), _stream())
            results.append((spans, d_limits, out, sizes_t, chosen, stream_bytes, stream_status, meta))
        enc.flush()
        torch.cuda.synchronize()
        for b, (spans, _, out, sizes_t, chosen, stream_bytes, stream_status, meta) in enumerate(results):
            limits, picks, _, want_stream_status, bits = want[b]
            total, status = (int(x) for x in meta.cpu())
            assert status == bits and [int(x) for x in stream_status.cpu()] == want_stream_status
            assert [int(c) for c in chosen.cpu()] == [CANDS[k] for k in picks]
            records = _records(orc, px[b], sm.frame_indices(sm.spans_of(pairs[b]), 40), [CANDS[k] for k in picks])
            assert total == sum(len(r) for r in records) and out[:total].cpu().numpy().tobytes() == b"".join(records)
            assert [int(x) for x in stream_bytes.cpu()] == sm.stream_bytes(sm.spans_of(pairs[b]), [len(r) for r in records])
    enc.close()


@pytest.mark.parametrize("stage", [1, 2, 3])
def test_a_failed_call_leaves_the_encoder_correct(torch_cuda, orc, stage):
    """m1v_debug_fail_encode reaches the call as it reaches the streams bitrate call (the table pass comes first and takes the
    stage): E_HIP, and the next call is exact."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    px = _pixels(75, 40)
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=40)
    limits, data = _check_encode(enc, dev, px, orc, torch, PAIRS, bm.LEAST_DISTORTION)
    _ffi.lib().m1v_debug_fail_encode(stage)
    try:
        with pytest.raises(EncoderError) as ei:
            _encode(enc, dev, PAIRS, bm.LEAST_DISTORTION, limits)
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    enc.flush()
    torch.cuda.synchronize()
    assert _encode(enc, dev, PAIRS, bm.LEAST_DISTORTION, limits)[0] == data
    _check_encode(enc, dev, px, orc, torch, PAIRS, bm.LARGEST_THAT_FITS)
    enc.close()
