"""The per-frame control kernels past their block and chunk edges (-m gpu): k_frame_quality, k_rd_pick, k_rate_pick in both forms,
k_rd_chains / k_rd_batch_pick / k_rd_cbr_pick, k_size_table_sizes / k_rd_table_sizes, k_streams_map / k_streams_finish /
k_streams_bitrate, each through an encode of up to 1100 pictures of 32 x 32 (tests/frame_axis.py; tests/test_frame_axis_cpu.py pins
that every case can fail).  Every comparison is for equality with the oracle's records or with a model the project has, and every
status word is checked.  One encoder per producer serves the whole module and the batch is uploaded once; the cases run on its
prefixes.

The encodes that pick by distortion need the fused table, which an encoder forced to the run kernels lacks (M1V_E_ARG): where a
case asks for the run producer under such a rule it takes the 4-channel encoder, whose path is the run kernels too."""
import ctypes as C

import pytest

import frame_axis as fa
import rd_oracle as rd
import rd_rate_model as M
import streams_model as sm

pytestmark = pytest.mark.gpu

OVER_BUDGET, OVER_DISTORTION = 16, 32
K8 = fa.K8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def rigs(torch_cuda):
    """{producer: (encoder of max_frames = 1100, the batch on the device, channels)}."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    out = {}
    for producer, channels in (("tiles", 3), ("runs", 3), ("rgba", 4)):
        enc = Mpeg1Encoder(fa.W, fa.H, fa.Q, "full", channels=channels, max_frames=fa.N)
        if producer == "runs":
            enc.debug_set_path("runs")
        assert enc.path == ("tiles" if producer == "tiles" else "runs")
        assert enc.size_table_fused == (0 if producer == "runs" else 1)
        out[producer] = (enc, torch_cuda.from_numpy(fa.batch(channels)).cuda(), channels)
    yield out
    for enc, _, _ in out.values():
        enc.close()


@pytest.fixture(scope="module")
def nv12(torch_cuda, orc):
    """The 3-channel batch as NV12 planes at addresses of their own behind a plane table (kp_*_planes)."""
    import input_families as fam
    inp = fam.build(torch_cuda, "kp-planes-nv12", fa.W, fa.H, "full", fa.Q, fa.N, pixels=fa.batch(3), orc=orc)
    yield inp
    inp.enc.close()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _indices(n, start=0):
    return [fa.FIRST + start + j for j in range(n)]


def _joined(recs):
    return b"".join(recs), [len(r) for r in recs]


def _finished(torch, enc, n, out, sizes, meta):
    """(bytes, sizes, status) of an asynchronous encode."""
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    return out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()], status & 0xFFFFFFFF


def _candidate_call(torch, enc, fn, dev, first, middle, with_dist):
    """One call of an encode that takes candidates, at K8, through its C entry point `fn`, whose arguments between the candidates
    and d_chosen are `middle`: (bytes, sizes, chosen, distortion or None, status)."""
    from ec504_imageencoder_amd import _ffi
    n = dev.shape[0]
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    chosen = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dist = torch.full((n,), -1, dtype=torch.int64, device="cuda") if with_dist else None
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")
    cbuf = (C.c_uint8 * len(K8))(*K8)
    args = [enc._h, _p(dev), n, first, cbuf, len(K8), *middle, _p(chosen), _p(out), out.numel(), _p(sizes)]
    args += [_p(dist)] if with_dist else []
    rc = getattr(_ffi.lib(), fn)(*args, C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _ffi.last_error()
    got, got_sizes, status = _finished(torch, enc, n, out, sizes, meta)
    return got, got_sizes, [int(c) for c in chosen.cpu()], [int(d) for d in dist.cpu()] if with_dist else None, status


def _check_picks(orc, channels, n, picks, result, want_status, with_dist, start=0):
    """A candidate call's result against the oracle at the model's picks (candidate indices) for frames start .. start + n."""
    S, D = fa.table(orc, channels)
    got, sizes, chosen, dist, status = result
    assert status == want_status, status
    assert chosen == [K8[k] for k in picks]
    assert sizes == [S[k][start + f] for f, k in enumerate(picks)]
    if with_dist:
        assert dist == [D[k][start + f] for f, k in enumerate(picks)]
    want, want_sizes = _joined(fa.records(orc, _indices(n, start), chosen, channels, start))
    assert sizes == want_sizes and got == want


# ---- a. per-frame quality: k_frame_quality, plain form ----------------------------------------------------------------------------
def _encode(torch, enc, dev, quality):
    out, sizes, meta = enc.encode(dev, fa.FIRST, quality=quality)
    return _finished(torch, enc, dev.shape[0], out, sizes, meta)


@pytest.mark.parametrize("n", [256, 257, 1100])
@pytest.mark.parametrize("producer", ["tiles", "runs", "rgba"])
def test_per_frame_quality(torch_cuda, orc, rigs, producer, n):
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    enc, dev, channels = rigs[producer]
    dev = dev[:n]
    q = fa.qualities()[:n]
    want, want_sizes = _joined(fa.records(orc, _indices(n), q, channels))
    got, sizes, status = _encode(torch, enc, dev, q)
    assert status == 0 and sizes == want_sizes and got == want
    word = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    probe = enc.frame_sizes(dev, quality=q, status=word)
    enc.flush()
    torch.cuda.synchronize()
    assert [int(s) for s in probe.cpu()] == want_sizes and int(word.item()) == 0
    bad = {1100: (1099, 13), 257: (256, 0)}.get(n)       # an entry out of range in the last workgroup, its only lane at n = 257
    if bad is None:
        return
    wrong = list(q)
    wrong[bad[0]] = bad[1]
    assert _encode(torch, enc, dev, wrong)[2] & _ffi.STATUS_QUALITY
    enc.frame_sizes(dev, quality=wrong, status=word)
    torch.cuda.synchronize()
    assert int(word.item()) & _ffi.STATUS_QUALITY
    out, sizes, meta = enc.encode(dev, fa.FIRST)                  # the next plain call is exact
    assert _finished(torch, enc, n, out, sizes, meta) == (*_joined(fa.records(orc, _indices(n), [fa.Q] * n, channels)), 0)


# ---- b. per-frame limits: k_frame_quality's budget form and both rules of k_rd_pick ----------------------------------------------
PER_FRAME = {
    # rule: (the model's rule, the C entry point, the status bit of a frame over its limit, the method of Mpeg1Encoder)
    "largest": (fa.LARGEST, "m1v_encode_budget_device", OVER_BUDGET, "encode_to_budget"),
    "best": (rd.BEST_IN_BUDGET, "m1v_encode_rd_device", OVER_BUDGET, "encode_best_in_budget"),
    "distortion": (rd.SMALLEST_AT_DISTORTION, "m1v_encode_rd_device", OVER_DISTORTION, "encode_to_distortion"),
}


@pytest.mark.parametrize("n", [256, 257, 1100])
@pytest.mark.parametrize("rule", sorted(PER_FRAME))
@pytest.mark.parametrize("producer", ["tiles", "rgba"])
def test_per_frame_limits(torch_cuda, orc, rigs, producer, rule, n):
    torch = torch_cuda
    enc, dev, channels = rigs[producer]
    model, fn, bit, method = PER_FRAME[rule]
    limits, picks, over = fa.per_frame_limits(orc, model, channels)
    assert over == [fa.N - 1]                                       # the status bit can only come from the last workgroup
    d_limits = torch.tensor(limits[:n], dtype=torch.int64).cuda()
    with_dist = model != fa.LARGEST
    middle = (model, 0, _p(d_limits)) if with_dist else (0, _p(d_limits))
    result = _candidate_call(torch, enc, fn, dev[:n], fa.FIRST, middle, with_dist)
    _check_picks(orc, channels, n, picks[:n], result, bit if n == fa.N else 0, with_dist)
    if n == fa.N:                                                   # the method of Mpeg1Encoder: the same, and the frames over
        res = getattr(enc, method)(dev, d_limits, K8, first_frame_index=fa.FIRST)
        assert res[:4] == (result[0], result[1], result[2], over) and (not with_dist or res[4] == result[3])


# ---- c. bitrate: k_rate_pick<true> and k_rd_cbr_pick ---------------------------------------------------------------------------------
BITRATE = {fa.BY_SIZE: ("m1v_encode_cbr_device", "encode_at_bitrate"), fa.BY_DISTORTION: ("m1v_encode_rd_cbr_device", "encode_best_at_bitrate")}


def _bitrate_rig(rigs, producer, by):
    return rigs["rgba" if (producer, by) == ("runs", fa.BY_DISTORTION) else producer]


@pytest.mark.parametrize("n", [512, 513, 519, 520, 1024, 1100])
@pytest.mark.parametrize("by", sorted(BITRATE))
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_bitrate(torch_cuda, orc, rigs, producer, by, n):
    torch = torch_cuda
    enc, dev, channels = _bitrate_rig(rigs, producer, by)
    rate, cap, L0 = fa.bitrate_params(orc, by, channels)
    S, D = fa.table(orc, channels)
    picks, over, after = fa.bitrate_walk(S, D, by, rate, cap, L0, 0, n)
    assert over                                                     # (the walk starts in debt)
    level_in = torch.tensor([L0], dtype=torch.int64).cuda()
    level_out = torch.full((1,), -777, dtype=torch.int64, device="cuda")
    with_dist = by == fa.BY_DISTORTION
    result = _candidate_call(torch, enc, BITRATE[by][0], dev[:n], fa.FIRST, (rate, cap, _p(level_in), _p(level_out)), with_dist)
    _check_picks(orc, channels, n, picks, result, OVER_BUDGET, with_dist)
    assert int(level_out.item()) == after and int(level_in.item()) == L0


@pytest.mark.parametrize("by", sorted(BITRATE))
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_two_chained_bitrate_calls_equal_one(torch_cuda, orc, rigs, producer, by):
    """513 and 587 frames on one level tensor: the second call starts a frame behind a chunk edge of the single call."""
    torch = torch_cuda
    enc, dev, channels = _bitrate_rig(rigs, producer, by)
    rate, cap, L0 = fa.bitrate_params(orc, by, channels)
    S, D = fa.table(orc, channels)
    picks, over, after = fa.bitrate_walk(S, D, by, rate, cap, L0)
    call = getattr(enc, BITRATE[by][1])
    level = torch.tensor([L0], dtype=torch.int64).cuda()
    one = call(dev, rate, cap, K8, level, first_frame_index=fa.FIRST)
    assert int(level.item()) == after and one[2:4] == ([K8[k] for k in picks], over)
    assert one[:2] == _joined(fa.records(orc, _indices(fa.N), one[2], channels))
    level.fill_(L0)
    a = call(dev[:513], rate, cap, K8, level, first_frame_index=fa.FIRST)
    b = call(dev[513:], rate, cap, K8, level, first_frame_index=fa.FIRST + 513)
    assert int(level.item()) == after
    assert (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + [f + 513 for f in b[3]]) == one[:4]
    if by == fa.BY_DISTORTION:
        assert a[4] + b[4] == one[4] == [D[k][f] for f, k in enumerate(picks)]


# ---- d. batch budgets: k_rate_pick<false>; k_rd_chains and k_rd_batch_pick -------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 1025, 1100])
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_batch_byte_budget(torch_cuda, orc, rigs, producer, n):
    torch = torch_cuda
    enc, dev, channels = rigs[producer]
    budget, picks = fa.batch_budget(orc, n, channels)
    result = _candidate_call(torch, enc, "m1v_encode_batch_budget_device", dev[:n], fa.FIRST, (budget,), False)
    _check_picks(orc, channels, n, picks, result, 0, False)
    assert len(result[0]) <= budget
    if n == fa.N:
        assert enc.encode_to_batch_budget(dev, budget, K8, first_frame_index=fa.FIRST) == (*result[:3], False)


RD_BATCH = {"best": (M.BEST_IN_BUDGET, "encode_best_in_batch_budget"), "distortion": (M.SMALLEST_AT_DISTORTION, "encode_batch_to_distortion")}


@pytest.mark.parametrize("n", [32, 33, 1100])
@pytest.mark.parametrize("rule", sorted(RD_BATCH))
@pytest.mark.parametrize("producer", ["tiles", "rgba"])
def test_batch_pick_by_distortion(torch_cuda, orc, rigs, producer, rule, n):
    torch = torch_cuda
    enc, dev, channels = rigs[producer]
    model, method = RD_BATCH[rule]
    limit, picks = fa.rd_batch_limit(orc, model, n, channels)
    result = _candidate_call(torch, enc, "m1v_encode_rd_batch_device", dev[:n], fa.FIRST, (model, limit), True)
    _check_picks(orc, channels, n, picks, result, 0, True)
    if n == fa.N:
        assert getattr(enc, method)(dev, limit, K8, first_frame_index=fa.FIRST) == (*result[:3], False, result[3])


# ---- e. tables: k_size_table_sizes, k_rd_table_sizes -------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "rgba"])
def test_tables(torch_cuda, orc, rigs, producer):
    """Every row of both tables at K = 8 over the 1100 frames; the second call right behind the first gives the same, so the
    counters were cleared for all 8 x 1100 cells."""
    torch = torch_cuda
    enc, dev, channels = rigs[producer]
    S, D = fa.table(orc, channels)
    for _ in range(2):
        word = torch.full((len(K8),), 0x40, dtype=torch.int32, device="cuda")
        sizes = enc.frame_size_table(dev, K8, status=word)
        enc.flush()
        torch.cuda.synchronize()
        assert sizes.cpu().tolist() == S and [int(w) for w in word.cpu()] == [0] * len(K8)
        word.fill_(0x40)
        sizes, dist = enc.frame_rd_table(dev, K8, status=word)
        enc.flush()
        torch.cuda.synchronize()
        assert sizes.cpu().tolist() == S and dist.cpu().tolist() == D and [int(w) for w in word.cpu()] == [0] * len(K8)


# ---- f. streams: k_streams_map, k_streams_finish, k_streams_bitrate ---------------------------------------------------------------
def _streams_rig(rigs, nv12, family):
    return (nv12.enc, nv12.dev) if family == "kp-planes-nv12" else rigs[family][:2]


@pytest.mark.parametrize("which", fa.SPAN_TABLES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["uniform", "per_frame_quality"])
@pytest.mark.parametrize("family", ["tiles", "kp-planes-nv12"])
def test_streams_records(torch_cuda, orc, rigs, nv12, family, per_frame, which):
    from ec504_imageencoder_amd import stream_spans
    torch = torch_cuda
    enc, dev = _streams_rig(rigs, nv12, family)
    spans, pairs = fa.spans(which), fa.span_pairs(which)
    quality = fa.qualities() if per_frame else None
    qs = quality or [fa.Q] * fa.N
    want, want_sizes = _joined(fa.records(orc, sm.frame_indices(spans, fa.N), qs, 3))
    out, sizes, meta, stream_bytes = enc.encode_streams_device(dev, stream_spans(pairs), quality=quality)
    got, got_sizes, status = _finished(torch, enc, fa.N, out, sizes, meta)
    assert status == 0 and got_sizes == want_sizes and got == want
    assert [int(b) for b in stream_bytes.cpu()] == sm.stream_bytes(spans, want_sizes)
    per_stream = b""                                                # one plain call per non-empty span
    for first, count, index in spans:
        if count:
            per_stream += enc.encode_to_bytes(dev[first:first + count], index, quality=qs[first:first + count] if per_frame else None)[0]
    assert per_stream == got


@pytest.mark.parametrize("cut", ["one_byte_short", "behind_frame_600"])
@pytest.mark.parametrize("which", fa.SPAN_TABLES)
def test_streams_cut_off(torch_cuda, orc, rigs, which, cut):
    """`out` too short: STATUS_NOSPACE and the full total; the records that fitted are exact, headers included (frame 600 lies in
    the third header workgroup, whose `front` sums 512 frames); nothing behind the capacity is touched; sizes and stream_bytes
    are complete."""
    from ec504_imageencoder_amd import _ffi, stream_spans
    torch = torch_cuda
    enc, dev, _ = rigs["tiles"]
    spans = fa.spans(which)
    recs = fa.records(orc, sm.frame_indices(spans, fa.N), [fa.Q] * fa.N, 3)
    sizes = [len(r) for r in recs]
    total = sum(sizes)
    last = fa.N - 2 if cut == "one_byte_short" else 600             # the last frame that fits
    fitted = sum(sizes[:last + 1])
    cap = total - 1 if cut == "one_byte_short" else fitted + sizes[last + 1] // 2
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _, got_sizes, meta, stream_bytes = enc.encode_streams_device(dev, stream_spans(fa.span_pairs(which)), out=out[:cap])
    enc.flush()
    torch.cuda.synchronize()
    assert int(meta[1]) == _ffi.STATUS_NOSPACE and int(meta[0]) == total
    host = out.cpu().numpy()
    assert host[:fitted].tobytes() == b"".join(recs[:last + 1])
    assert (host[cap:] == 0xA5).all()
    assert [int(s) for s in got_sizes[:fa.N].cpu()] == sizes
    assert [int(b) for b in stream_bytes.cpu()] == sm.stream_bytes(spans, sizes)


def test_two_queued_streams_batches_keep_their_own_spans(torch_cuda, orc, rigs):
    """Pipelined mode, 300 and then 700 frames, each batch with its own spans and its own index array, twice so that every
    counter set takes a turn."""
    from ec504_imageencoder_amd import Mpeg1Encoder, stream_spans
    torch = torch_cuda
    dev = rigs["tiles"][1]
    batches = fa.queued_batches()
    enc = Mpeg1Encoder(fa.W, fa.H, fa.Q, "full", max_frames=700)
    enc.set_pipelined(True)
    device_spans = [stream_spans(pairs) for _, _, pairs in batches]
    want = [fa.records(orc, sm.frame_indices(sm.spans_of(pairs), n), [fa.Q] * n, 3, start) for start, n, pairs in batches]
    for _ in range(2):
        results = [enc.encode_streams_device(dev[start:start + n], device_spans[b]) for b, (start, n, _) in enumerate(batches)]
        enc.flush()
        torch.cuda.synchronize()
        for b, (out, sizes, meta, stream_bytes) in enumerate(results):
            n, spans = batches[b][1], sm.spans_of(batches[b][2])
            total, status = (int(x) for x in meta.cpu())
            assert status == 0 and (out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()]) == _joined(want[b])
            assert [int(x) for x in stream_bytes.cpu()] == sm.stream_bytes(spans, [len(r) for r in want[b]])
    enc.close()


@pytest.mark.parametrize("by", sorted(BITRATE))
def test_streams_bitrate(torch_cuda, orc, rigs, by):
    """Spans of 513, 0 and 587 frames with a rate per stream: the model's picks on the oracle's table, and what one bitrate call
    per span gives."""
    torch = torch_cuda
    enc, dev, channels = rigs["tiles"]
    rates, levels = fa.streams_bitrate_params(orc, by, channels)
    pairs = list(fa.BITRATE_PAIRS)
    spans = sm.spans_of(pairs)
    S, D = fa.table(orc, channels)
    rule = sm.LARGEST_THAT_FITS if by == fa.BY_SIZE else sm.LEAST_DISTORTION
    picks, want_dist, after, bits = sm.streams_bitrate(S, D, spans, rates, levels, rule)
    assert bits == sm.STATUS_OVER_BUDGET
    d_levels = torch.tensor(levels, dtype=torch.int64).cuda()
    data, sizes, chosen, stream_bytes, over, dist = enc.encode_streams_at_bitrate(
        dev, pairs, K8, [r for r, _ in rates], [c for _, c in rates], d_levels, by=by)
    assert over is True and chosen == [K8[k] for k in picks] and [int(x) for x in d_levels.cpu()] == after
    assert dist == (want_dist if by == fa.BY_DISTORTION else None)
    assert (data, sizes) == _joined(fa.records(orc, sm.frame_indices(spans, fa.N), chosen, channels))
    assert sizes == [S[k][f] for f, k in enumerate(picks)] and stream_bytes == sm.stream_bytes(spans, sizes)
    single = getattr(enc, BITRATE[by][1])
    per_stream = b""
    for s, (first, count, index) in enumerate(spans):
        if count:
            level = torch.tensor([levels[s]], dtype=torch.int64).cuda()
            res = single(dev[first:first + count], rates[s][0], rates[s][1], K8, level, first_frame_index=index)
            assert (res[2], int(level.item())) == (chosen[first:first + count], after[s])
            per_stream += res[0]
    assert per_stream == data
