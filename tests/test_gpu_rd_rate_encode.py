"""GPU tests of the batch and bitrate encodes that pick by distortion (m1v_encode_rd_batch_device, m1v_encode_rd_cbr_device,
Mpeg1Encoder.encode_best_in_batch_budget / encode_batch_to_distortion / encode_best_at_bitrate; -m gpu): picks, per-frame
distortion, sizes, status, level and bytes against the model of the rules (tests/rd_rate_model.py) on the oracle's own table and
the oracle's records at the picked qualities."""
import ctypes as C

import numpy as np
import pytest

import rd_oracle as rd
import rd_rate_model as M
from gpu_calls import _mixed_frames
from hard_content_cases import FIRST, _Case, _case_dist

pytestmark = pytest.mark.gpu

OVER_BIT = {M.BEST_IN_BUDGET: 16, M.SMALLEST_AT_DISTORTION: 32}
NOISE_CANDS = (2, 4, 8, 12)
HARD_CANDS = (20, 50, 76, 85, 92)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _buffers(torch, enc, n, want_chosen, want_dist):
    out = torch.empty(enc.frame_bound * max(n, 1), dtype=torch.uint8, device="cuda")
    sizes = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    chosen = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") if want_chosen else None
    dist = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda") if want_dist else None
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")
    return out, sizes, chosen, dist, meta


def _result(torch, enc, n, out, sizes, chosen, dist, meta):
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    return (out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()],
            [int(c) for c in chosen[:n].cpu()] if chosen is not None else None,
            [int(d) for d in dist[:n].cpu()] if dist is not None else None, status & 0xFFFFFFFF)


def _batch_device(torch, enc, dev, cands, rule, limit, first, want_chosen=True, want_dist=True):
    """One m1v_encode_rd_batch_device through the C entry point -> (bytes, sizes, chosen, distortion, status)."""
    from ec504_imageencoder_amd import _ffi
    n = dev.shape[0]
    out, sizes, chosen, dist, meta = _buffers(torch, enc, n, want_chosen, want_dist)
    cbuf = (C.c_uint8 * len(cands))(*cands)
    rc = _ffi.lib().m1v_encode_rd_batch_device(enc._h, _p(dev), n, first, cbuf, len(cands), rule, int(limit), _p(chosen), _p(out),
                                               out.numel(), _p(sizes), _p(dist), C.c_void_p(meta.data_ptr()),
                                               C.c_void_p(meta.data_ptr() + 8), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _ffi.last_error()
    return _result(torch, enc, n, out, sizes, chosen, dist, meta)


def _cbr_device(torch, enc, dev, cands, rate, cap, level, first, want_chosen=True, want_dist=True):
    """One m1v_encode_rd_cbr_device -> (bytes, sizes, chosen, distortion, status, level out)."""
    from ec504_imageencoder_amd import _ffi
    n = dev.shape[0]
    out, sizes, chosen, dist, meta = _buffers(torch, enc, n, want_chosen, want_dist)
    lin = torch.tensor([level], dtype=torch.int64).cuda()
    lout = torch.full((1,), -777, dtype=torch.int64, device="cuda")
    cbuf = (C.c_uint8 * len(cands))(*cands)
    rc = _ffi.lib().m1v_encode_rd_cbr_device(enc._h, _p(dev), n, first, cbuf, len(cands), rate, cap, _p(lin), _p(lout), _p(chosen),
                                             _p(out), out.numel(), _p(sizes), _p(dist), C.c_void_p(meta.data_ptr()),
                                             C.c_void_p(meta.data_ptr() + 8), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _ffi.last_error()
    return _result(torch, enc, n, out, sizes, chosen, dist, meta) + (int(lout.item()),)


def _batch_limits(S, D, rule):
    """Limits from the table itself, a quarter, a half and three quarters of the way between the smallest and the largest sum the
    rule bounds, at which (by the model) the frames' picks differ; and whether any of them differs from the byte rule's picks."""
    bound = S if rule == M.BEST_IN_BUDGET else D
    n = len(S[0])
    lo, hi = sum(min(r[f] for r in bound) for f in range(n)), sum(max(r[f] for r in bound) for f in range(n))
    limits = [lo + (hi - lo) * i // 4 for i in (1, 2, 3)]
    mixed = [x for x in limits if len(set(M.batch_pick(S, D, rule, x)[0])) > 1]
    # the byte rule at the bytes this pick uses
    other = any(M.batch_pick(S, D, rule, x)[0] != M.batch_byte_rule(S, sum(S[k][f] for f, k in enumerate(M.batch_pick(S, D, rule, x)[0])))[0]
                for x in mixed)
    return mixed, other


def _bitrate_setup(S, D):
    """(rate, capacity, level) from the table: the median record per frame into a buffer of two of the largest."""
    flat = sorted(x for r in S for x in r)
    return flat[len(flat) // 2], 2 * flat[-1], flat[len(flat) // 2]


def _check_batch_and_bitrate(torch, enc, dev, cands, S, D, first, records, pipelined):
    """Both batch rules at the table's own limits and the bitrate form, twice per encoder: chosen, per-frame D, sizes, status,
    level and bytes are the oracle's at the model's picks.  Returns whether any pick differed from the byte rules'."""
    n = len(S[0])
    differs = False
    if pipelined:
        enc.set_pipelined(True)
    for rule in (M.BEST_IN_BUDGET, M.SMALLEST_AT_DISTORTION):
        limits, other = _batch_limits(S, D, rule)
        assert limits, "the picks must differ between frames"
        differs |= other
        bound = S if rule == M.BEST_IN_BUDGET else D
        under = sum(min(r[f] for r in bound) for f in range(n)) - 1            # nothing reaches it: the status bit
        for limit in limits + [under]:
            picks, over = M.batch_pick(S, D, rule, limit)
            assert over == (limit == under)
            for _ in range(2):
                got, sizes, chosen, dist, status = _batch_device(torch, enc, dev, cands, rule, limit, first)
                assert status == (OVER_BIT[rule] if over else 0)
                assert chosen == [cands[k] for k in picks]
                assert dist == [D[k][f] for f, k in enumerate(picks)]
                assert (got, sizes) == records([cands[k] for k in picks])
            got2, sizes2, _, _, status2 = _batch_device(torch, enc, dev, cands, rule, limit, first, want_chosen=False, want_dist=False)
            assert (got2, sizes2, status2) == (got, sizes, status)              # d_chosen and d_frame_distortion may be NULL
    rate, cap, level = _bitrate_setup(S, D)
    picks, over, level_out = M.bitrate_walk(S, D, rate, cap, level)
    assert len(set(picks)) > 1, "the picks must differ between frames"
    differs |= picks != M.bitrate_byte_rule(S, rate, cap, level)[0]
    for _ in range(2):
        got, sizes, chosen, dist, status, lout = _cbr_device(torch, enc, dev, cands, rate, cap, level, first)
        assert status == (16 if over else 0) and lout == level_out
        assert chosen == [cands[k] for k in picks] and dist == [D[k][f] for f, k in enumerate(picks)]
        assert (got, sizes) == records([cands[k] for k in picks])
    got2, sizes2, _, _, status2, lout2 = _cbr_device(torch, enc, dev, cands, rate, cap, level, first, want_chosen=False, want_dist=False)
    assert (got2, sizes2, status2, lout2) == (got, sizes, status, lout)
    # a starved stream: nothing fits some frame, the smallest record is taken and the debt carried
    picks, over, level_out = M.bitrate_walk(S, D, 1, cap, 0)
    assert over
    got, sizes, chosen, dist, status, lout = _cbr_device(torch, enc, dev, cands, 1, cap, 0, first)
    assert status == 16 and lout == level_out and chosen == [cands[k] for k in picks]
    assert (got, sizes) == records([cands[k] for k in picks])
    return differs


# ---- 1. noise ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise(orc):
    W, H, n, first = 352, 288, 6, 31
    px = _mixed_frames(np.random.default_rng(606), n, W, H, 3)
    recs = {(f, q): orc.encode_frame(px[f], W, H, first + f, q, orc.MODE_FULL) for f in range(n) for q in NOISE_CANDS}
    s = [[len(recs[f, q]) for f in range(n)] for q in NOISE_CANDS]
    d = [[rd.frame_distortion(orc, px[f], W, H, q, orc.MODE_FULL) for f in range(n)] for q in NOISE_CANDS]
    return dict(W=W, H=H, n=n, first=first, px=px, recs=recs, s=s, d=d)


@pytest.mark.parametrize("pipelined", [False, True])
def test_rules_on_noise(torch_cuda, noise, pipelined):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n = noise["n"]
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=n)
    dev = torch.from_numpy(noise["px"]).cuda()

    def records(qs):
        recs = [noise["recs"][f, q] for f, q in enumerate(qs)]
        return b"".join(recs), [len(r) for r in recs]

    _check_batch_and_bitrate(torch, enc, dev, NOISE_CANDS, noise["s"], noise["d"], noise["first"], records, pipelined)
    enc.close()


# ---- 2. hard content: the picks are not the byte rules' ---------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("family", ["rgb", "surface-4-bgr-gap", "planes-nv12"])
def test_rules_on_hard_content(torch_cuda, orc, family, pipelined):
    """Hard and flat frames in turn on an encoder of quality 92, through three kernel families."""
    torch = torch_cuda
    case = _Case(torch, orc, family, 352, 288, (0, 4, 1, 5, 2, 6))
    n = case.n
    S = [case.sizes(q) for q in HARD_CANDS]
    D = [[_case_dist(orc, case, f, q) for f in range(n)] for q in HARD_CANDS]
    differs = _check_batch_and_bitrate(torch, case.enc, case.dev, HARD_CANDS, S, D, FIRST, case.records, pipelined)
    assert differs, "on this content the picks by distortion differ from the byte rules'"
    case.close()


def test_gradient_batch_budget_picks_38_where_the_byte_rule_picks_92(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    W, H = 352, 288
    pic = rd.gradient_frame(W, H)
    enc = Mpeg1Encoder(W, H, 92, "full", max_frames=1)
    dev = torch.from_numpy(pic[None]).cuda()
    got, sizes, chosen, over = enc.encode_to_batch_budget(dev, 8000, rd.GRADIENT_QUALITIES)
    assert (chosen, sizes, over) == ([92], [7507], False)
    got, sizes, chosen, over, dist = enc.encode_best_in_batch_budget(dev, 8000, rd.GRADIENT_QUALITIES)
    assert (chosen, sizes, over, dist) == ([38], [7815], False, [1400207])
    assert got == orc.encode_frame(pic, W, H, 0, 38, orc.MODE_FULL)
    got, sizes, chosen, over, dist = enc.encode_batch_to_distortion(dev, 1_500_000, rd.GRADIENT_QUALITIES)
    assert (chosen, sizes, over, dist) == ([38], [7815], False, [1400207])
    assert enc.encode_batch_to_distortion(dev, 400_000, rd.GRADIENT_QUALITIES)[2:4] == ([76], True)
    level = torch.tensor([8000], dtype=torch.int64).cuda()
    assert enc.encode_at_bitrate(dev, 8000, 8000, rd.GRADIENT_QUALITIES, level)[2] == [92]
    level.fill_(8000)
    got, sizes, chosen, over, dist = enc.encode_best_at_bitrate(dev, 8000, 8000, rd.GRADIENT_QUALITIES, level)
    assert (chosen, sizes, over, dist) == ([38], [7815], [], [1400207]) and int(level.item()) == 8000
    enc.close()


def test_python_calls_on_noise(torch_cuda, noise):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n, first, S, D = noise["n"], noise["first"], noise["s"], noise["d"]
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=n)
    dev = torch.from_numpy(noise["px"]).cuda()
    for rule, call in ((M.BEST_IN_BUDGET, enc.encode_best_in_batch_budget), (M.SMALLEST_AT_DISTORTION, enc.encode_batch_to_distortion)):
        for limit in _batch_limits(S, D, rule)[0] + [0]:
            picks, over = M.batch_pick(S, D, rule, limit)
            got, sizes, chosen, ov, dist = call(dev, limit, NOISE_CANDS, first_frame_index=first)
            assert (chosen, ov) == ([NOISE_CANDS[k] for k in picks], over)
            assert dist == [D[k][f] for f, k in enumerate(picks)] and sizes == [S[k][f] for f, k in enumerate(picks)]
            assert got == b"".join(noise["recs"][f, NOISE_CANDS[k]] for f, k in enumerate(picks))
    rate, cap, start = _bitrate_setup(S, D)
    level = torch.tensor([start], dtype=torch.int64).cuda()
    for _ in range(2):                                   # two calls form one stream
        picks, over, out = M.bitrate_walk(S, D, rate, cap, start)
        got, sizes, chosen, ov, dist = enc.encode_best_at_bitrate(dev, rate, cap, NOISE_CANDS, level, first_frame_index=first)
        assert (chosen, ov, int(level.item())) == ([NOISE_CANDS[k] for k in picks], over, out)
        assert dist == [D[k][f] for f, k in enumerate(picks)]
        assert got == b"".join(noise["recs"][f, NOISE_CANDS[k]] for f, k in enumerate(picks))
        start = out
    enc.close()


# ---- 3. an unencodable candidate, launches, argument errors, the empty batch ------------------------------------------------
def test_unencodable_candidates_are_skipped(torch_cuda, orc):
    """The extreme-pattern frame makes 90 and 92 unencodable: they are out for every frame, whatever the limit allows; with every
    candidate out the frames go to candidates[0] and the encode reports the bit.  The encoder is exact afterwards."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch = torch_cuda
    case = _Case(torch, orc, "rgb", 352, 288, (0, 3, 1, 4))
    n = case.n
    cands, status = (50, 76, 90, 92), [0, 0, 1, 1]
    S = [case.sizes(q) if not status[k] else [1] * n for k, q in enumerate(cands)]          # (rows of the skipped: never read)
    D = [[_case_dist(orc, case, f, q) for f in range(n)] if not status[k] else [0] * n for k, q in enumerate(cands)]

    def check():
        for rule, limit in ((M.BEST_IN_BUDGET, 1 << 40), (M.SMALLEST_AT_DISTORTION, 0), (M.BEST_IN_BUDGET, sum(S[0]) + 1000)):
            picks, over = M.batch_pick(S, D, rule, limit, status)
            assert all(k < 2 for k in picks) and over == (limit == 0)
            got, sizes, chosen, dist, word = _batch_device(torch, case.enc, case.dev, cands, rule, limit, FIRST)
            assert word == (OVER_BIT[rule] if over else 0) and chosen == [cands[k] for k in picks]
            assert dist == [D[k][f] for f, k in enumerate(picks)] and (got, sizes) == case.records([cands[k] for k in picks])
        picks, over, out = M.bitrate_walk(S, D, max(S[1]), 1 << 30, 1 << 30, status)
        got, sizes, chosen, dist, word, lout = _cbr_device(torch, case.enc, case.dev, cands, max(S[1]), 1 << 30, 1 << 30, FIRST)
        assert all(k < 2 for k in picks) and not over and word == 0 and lout == out
        assert chosen == [cands[k] for k in picks] and (got, sizes) == case.records([cands[k] for k in picks])

    check()
    _, _, chosen, _, word = _batch_device(torch, case.enc, case.dev, (90, 92), M.BEST_IN_BUDGET, 1 << 40, FIRST)
    assert chosen == [90] * n and word & _ffi.STATUS_UNENCODABLE
    _, _, chosen, _, word, _ = _cbr_device(torch, case.enc, case.dev, (90, 92), 1 << 20, 1 << 30, 1 << 30, FIRST)
    assert chosen == [90] * n and word & _ffi.STATUS_UNENCODABLE
    with pytest.raises(EncoderError) as ei:
        case.enc.encode_best_in_batch_budget(case.dev, 1 << 40, (90, 92))
    assert ei.value.code == _ffi.E_UNENCODABLE
    check()
    case.close()


def test_a_profiled_call_counts_two_launches(torch_cuda, noise):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=noise["n"])
    dev = torch.from_numpy(noise["px"]).cuda()
    level = torch.tensor([10 ** 6], dtype=torch.int64).cuda()
    for call in (lambda: enc.encode_best_in_batch_budget(dev, 10 ** 7, NOISE_CANDS),
                 lambda: enc.encode_batch_to_distortion(dev, 10 ** 12, NOISE_CANDS),
                 lambda: enc.encode_best_at_bitrate(dev, 10 ** 5, 10 ** 6, NOISE_CANDS, level)):
        enc.profile(True)
        call()
        launches, _ = enc.profile_read()
        enc.profile(False)
        assert launches == 2
    enc.close()


@pytest.mark.parametrize("call", ["rd", "rd_batch", "rd_cbr"])
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_failed_call_leaves_the_encoder_correct(torch_cuda, noise, stage, call):
    """m1v_debug_fail_encode in front of each of the three encodes that pick by distortion: the call returns E_HIP, the bitrate
    form leaves d_level_in alone, and the same call again, a plain encode and every rule after it are the oracle's.
    Limitation: these calls need the fused table, whose pass comes first and has the hook at all three stages, so the failure
    is always the table's.  This pins the table's poison recovery inside these calls, not a failure in the encode behind it."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    from gpu_calls import _model, _rd_device
    torch = torch_cuda
    n, first, K = 5, noise["first"], len(NOISE_CANDS)
    S, D = [row[:n] for row in noise["s"]], [row[:n] for row in noise["d"]]
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=n)
    assert enc.path == "tiles" and enc.size_table_fused == 1
    if stage == 2:
        enc.set_pipelined(True)
    dev = torch.from_numpy(noise["px"][:n]).cuda()

    def records(qs):
        recs = [noise["recs"][f, q] for f, q in enumerate(qs)]
        return b"".join(recs), [len(r) for r in recs]

    per_frame = sorted(x for row in S for x in row)[K * n // 2]
    budget = _batch_limits(S, D, M.BEST_IN_BUDGET)[0][0]
    rate, cap, level = _bitrate_setup(S, D)
    out, sizes, chosen, dist, meta = _buffers(torch, enc, n, True, True)
    lin = torch.tensor([level], dtype=torch.int64).cuda()
    lout = torch.full((1,), -777, dtype=torch.int64, device="cuda")
    L = _ffi.lib()
    cbuf = (C.c_uint8 * K)(*NOISE_CANDS)
    results = (_p(chosen), _p(out), out.numel(), _p(sizes), _p(dist), C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8),
               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.m1v_debug_fail_encode(stage)
    try:
        if call == "rd":
            rc = L.m1v_encode_rd_device(enc._h, _p(dev), n, first, cbuf, K, M.BEST_IN_BUDGET, per_frame, None, *results)
        elif call == "rd_batch":
            rc = L.m1v_encode_rd_batch_device(enc._h, _p(dev), n, first, cbuf, K, M.BEST_IN_BUDGET, budget, *results)
        else:
            rc = L.m1v_encode_rd_cbr_device(enc._h, _p(dev), n, first, cbuf, K, rate, cap, _p(lin), _p(lout), *results)
        assert rc == _ffi.E_HIP
    finally:
        L.m1v_debug_fail_encode(0)
    enc.flush()
    torch.cuda.synchronize()
    assert int(lin.item()) == level
    # the same call again
    if call == "rd":
        picks, over = _model(M.BEST_IN_BUDGET, S, D, [per_frame] * n)
        got, sizes, chosen, dist, status = _rd_device(torch, enc, dev, NOISE_CANDS, M.BEST_IN_BUDGET, per_frame, first)
    elif call == "rd_batch":
        picks, over = M.batch_pick(S, D, M.BEST_IN_BUDGET, budget)
        got, sizes, chosen, dist, status = _batch_device(torch, enc, dev, NOISE_CANDS, M.BEST_IN_BUDGET, budget, first)
    else:
        picks, over, level_out = M.bitrate_walk(S, D, rate, cap, level)
        got, sizes, chosen, dist, status, lout = _cbr_device(torch, enc, dev, NOISE_CANDS, rate, cap, level, first)
        assert lout == level_out
    assert len(set(picks)) > 1 and status == (16 if over else 0)
    assert chosen == [NOISE_CANDS[k] for k in picks] and dist == [D[k][f] for f, k in enumerate(picks)]
    assert (got, sizes) == records([NOISE_CANDS[k] for k in picks])
    # a plain encode, then both batch rules and the bitrate form
    assert enc.encode_to_bytes(dev, first_frame_index=first) == records([12] * n)
    _check_batch_and_bitrate(torch, enc, dev, NOISE_CANDS, S, D, first, records, False)
    enc.close()


def test_argument_errors_and_the_empty_batch(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=2)
    dev = torch.zeros((2, 288, 352, 3), dtype=torch.uint8, device="cuda")
    big = torch.zeros((3, 288, 352, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(enc.frame_bound * 3, dtype=torch.uint8, device="cuda")
    meta = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    chosen = torch.full((2,), 99, dtype=torch.uint8, device="cuda")
    dist = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    lin = torch.tensor([50], dtype=torch.int64).cuda()
    lout = torch.tensor([-9], dtype=torch.int64).cuda()
    L = _ffi.lib()
    good = (C.c_uint8 * 2)(4, 8)

    def batch(rgb=dev, n=2, cands=good, k=2, rule=0, d_out=out):
        return L.m1v_encode_rd_batch_device(enc._h, _p(rgb), n, 0, cands, k, rule, 5000, _p(chosen), _p(d_out), out.numel(), None,
                                            _p(dist), _p(meta), C.c_void_p(meta.data_ptr() + 8), None)

    def cbr(rgb=dev, n=2, cands=good, k=2, rate=100, cap=1000, d_out=out, lin=lin, lout=lout):
        return L.m1v_encode_rd_cbr_device(enc._h, _p(rgb), n, 0, cands, k, rate, cap, _p(lin), _p(lout), _p(chosen), _p(d_out),
                                          out.numel(), None, _p(dist), _p(meta), C.c_void_p(meta.data_ptr() + 8), None)

    assert batch(rule=2) == _ffi.E_ARG and "rule" in _ffi.last_error()
    assert batch(rule=-1) == _ffi.E_ARG
    for call in (batch, cbr):
        for bad in ((4, 4), (8, 4), (0, 4), (4, 13)):
            assert call(cands=(C.c_uint8 * 2)(*bad)) == _ffi.E_ARG, bad
        assert call(k=0) == _ffi.E_ARG and call(k=9) == _ffi.E_ARG and call(cands=None) == _ffi.E_ARG
        assert call(rgb=big, n=3) == _ffi.E_ARG and call(n=-1) == _ffi.E_ARG
        assert call(rgb=None) == _ffi.E_ARG and call(d_out=None) == _ffi.E_ARG
    assert cbr(rate=0) == _ffi.E_ARG and cbr(rate=1001) == _ffi.E_ARG and cbr(cap=1 << 62) == _ffi.E_ARG
    assert cbr(lin=None) == _ffi.E_ARG and cbr(lout=None) == _ffi.E_ARG
    for limit in (-1, 1 << 64):
        with pytest.raises(EncoderError) as ei:
            enc.encode_best_in_batch_budget(dev, limit, (4, 8))
        assert ei.value.code == _ffi.E_ARG
    # an encoder forced to the run kernels has no fused table: M1V_E_ARG, before any launch
    enc.debug_set_path("runs")
    assert enc.size_table_fused == 0
    assert batch() == _ffi.E_ARG and "fused" in _ffi.last_error()
    assert cbr() == _ffi.E_ARG and "fused" in _ffi.last_error()
    torch.cuda.synchronize()

    def untouched():
        return (chosen.cpu().tolist(), dist.cpu().tolist(), int(out.max().cpu())) == ([99, 99], [-9, -9], 0)

    assert [int(x) for x in meta.cpu()] == [-9, -9] and untouched() and int(lout.item()) == -9
    # an empty batch: total and status written as 0 (the bitrate form also the level), nothing else
    enc.debug_set_path("auto")
    assert batch(n=0) == 0
    torch.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in meta.cpu()] == [0, 0] and untouched() and int(lout.item()) == -9
    meta.fill_(-9)
    assert cbr(n=0, rate=10, cap=40) == 0
    torch.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in meta.cpu()] == [0, 0] and untouched()
    assert int(lout.item()) == 40 and int(lin.item()) == 50
    enc.close()
