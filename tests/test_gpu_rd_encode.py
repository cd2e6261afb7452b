"""GPU tests of the rate-distortion encode (m1v_encode_rd_device, Mpeg1Encoder.encode_best_in_budget / encode_to_distortion;
-m gpu): picks, status bits, the per-frame distortion, sizes and bytes against the Python model of the two rules
(tests/rd_oracle.py) on the oracle's own table, and the oracle's records at the picked qualities."""
import ctypes as C

import numpy as np
import pytest

import rd_oracle as rd
from gpu_calls import _mixed_frames, _model, _rd_device
from hard_content_cases import FIRST, _Case, _case_dist

pytestmark = pytest.mark.gpu

OVER_BIT = {rd.BEST_IN_BUDGET: 16, rd.SMALLEST_AT_DISTORTION: 32}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- 1. both rules on noise: scalar and per-frame limits, none fits / none qualifies ----------------------------------------
NOISE_CANDS = (2, 4, 8, 12)


@pytest.fixture(scope="module")
def noise(orc):
    W, H, n, first = 352, 288, 6, 31
    px = _mixed_frames(np.random.default_rng(606), n, W, H, 3)
    recs = {(f, q): orc.encode_frame(px[f], W, H, first + f, q, orc.MODE_FULL) for f in range(n) for q in NOISE_CANDS}
    s = [[len(recs[f, q]) for f in range(n)] for q in NOISE_CANDS]
    d = [[rd.frame_distortion(orc, px[f], W, H, q, orc.MODE_FULL) for f in range(n)] for q in NOISE_CANDS]
    return dict(W=W, H=H, n=n, first=first, px=px, recs=recs, s=s, d=d)


def _noise_limits(noise, rule, form):
    """Limits from the table itself, so that the frames' picks differ; "none": nothing is within the limit."""
    n = noise["n"]
    bound = noise["s"] if rule == rd.BEST_IN_BUDGET else noise["d"]
    if form == "none":
        return [min(row[f] for row in bound) - 1 for f in range(n)]
    if form == "scalar":
        return [sorted(x for row in bound for x in row)[len(bound) * n // 2]] * n
    return [bound[(f * 7 + 1) % len(bound)][f] + (f % 2) for f in range(n)]


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("form", ["scalar", "per_frame", "none"])
@pytest.mark.parametrize("rule", [rd.BEST_IN_BUDGET, rd.SMALLEST_AT_DISTORTION])
def test_both_rules_on_noise(torch_cuda, noise, rule, form, pipelined):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n, first, s, d = noise["n"], noise["first"], noise["s"], noise["d"]
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=n)
    if pipelined:
        enc.set_pipelined(True)
    dev = torch.from_numpy(noise["px"]).cuda()
    limits = _noise_limits(noise, rule, form)
    picks, over = _model(rule, s, d, limits)
    assert {"none": len(over) == n, "per_frame": not over and len(set(picks)) > 1, "scalar": len(set(picks)) > 1}[form], (picks, over)
    scalar = form == "scalar"
    for _ in range(2):                                   # the second call on the encoder is as exact as the first
        got, sizes, chosen, dist, status = _rd_device(torch, enc, dev, NOISE_CANDS, rule, limits[0] if scalar else 0, first,
                                                      None if scalar else limits)
        assert status == (OVER_BIT[rule] if over else 0)
        assert chosen == [NOISE_CANDS[k] for k in picks]
        assert dist == [d[k][f] for f, k in enumerate(picks)]
        assert sizes == [s[k][f] for f, k in enumerate(picks)]
        assert got == b"".join(noise["recs"][f, NOISE_CANDS[k]] for f, k in enumerate(picks))
    # d_chosen and d_frame_distortion may be NULL
    got2, sizes2, _, _, status2 = _rd_device(torch, enc, dev, NOISE_CANDS, rule, limits[0] if scalar else 0, first,
                                             None if scalar else limits, want_chosen=False, want_dist=False)
    assert (got2, sizes2, status2) == (got, sizes, status)
    enc.close()


def test_python_calls_scalar_list_and_tensor_limits(torch_cuda, noise):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n, first, s, d = noise["n"], noise["first"], noise["s"], noise["d"]
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=n)
    dev = torch.from_numpy(noise["px"]).cuda()
    for rule, call in ((rd.BEST_IN_BUDGET, enc.encode_best_in_budget), (rd.SMALLEST_AT_DISTORTION, enc.encode_to_distortion)):
        per_frame = _noise_limits(noise, rule, "per_frame")
        per_frame[2] = 0                                 # one frame over its limit
        for limit in (_noise_limits(noise, rule, "scalar")[0], per_frame, torch.tensor(per_frame, dtype=torch.int64).cuda()):
            limits = [limit] * n if isinstance(limit, int) else per_frame
            picks, over = _model(rule, s, d, limits)
            got, sizes, chosen, ov, dist = call(dev, limit, NOISE_CANDS, first_frame_index=first)
            assert (chosen, ov) == ([NOISE_CANDS[k] for k in picks], over)
            assert dist == [d[k][f] for f, k in enumerate(picks)] and sizes == [s[k][f] for f, k in enumerate(picks)]
            assert got == b"".join(noise["recs"][f, NOISE_CANDS[k]] for f, k in enumerate(picks))
    # a limit in dB: the helpers of the encoder
    ceiling = enc.psnr_to_distortion(30.0)
    assert enc.distortion_to_psnr(ceiling) >= 30.0 - 1e-9
    picks, over = _model(rd.SMALLEST_AT_DISTORTION, s, d, [ceiling] * n)
    assert enc.encode_to_distortion(dev, ceiling, NOISE_CANDS)[2:4] == ([NOISE_CANDS[k] for k in picks], over)
    enc.close()


# ---- 2. hard content: the rules disagree with "the largest that fits", an unencodable candidate is skipped -------------------
HARD_CANDS = (20, 50, 76, 85, 92)


@pytest.mark.parametrize("family", ["rgb", "surface-4-bgr-gap", "planes-nv12"])
def test_both_rules_on_hard_content(torch_cuda, orc, family):
    """Hard and flat frames in turn on an encoder of quality 92, through three kernel families."""
    torch = torch_cuda
    case = _Case(torch, orc, family, 352, 288, (0, 4, 1, 5, 2, 6))
    n = case.n
    s = [case.sizes(q) for q in HARD_CANDS]
    d = [[_case_dist(orc, case, f, q) for f in range(n)] for q in HARD_CANDS]
    for rule, bound in ((rd.BEST_IN_BUDGET, s), (rd.SMALLEST_AT_DISTORTION, d)):
        limits = [sorted(row[f] for row in bound)[2] for f in range(n)]          # the frame's own median
        picks, over = _model(rule, s, d, limits)
        assert not over
        got, sizes, chosen, dist, status = _rd_device(torch, case.enc, case.dev, HARD_CANDS, rule, 0, FIRST, limits)
        assert status == 0 and chosen == [HARD_CANDS[k] for k in picks]
        assert dist == [d[k][f] for f, k in enumerate(picks)]
        assert (got, sizes) == case.records([HARD_CANDS[k] for k in picks])
    case.close()


def test_unencodable_candidates_are_skipped(torch_cuda, orc):
    """The extreme-pattern frame makes 90 and 92 unencodable (tests/test_gpu_rd_table.py asks the oracle): they are out for EVERY frame, whatever the limit allows; with every
    candidate out the frames go to candidates[0] and the encode reports the bit."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch = torch_cuda
    case = _Case(torch, orc, "rgb", 352, 288, (0, 3, 1, 4))
    n = case.n
    cands, out = (50, 76, 90, 92), (2, 3)
    s = [case.sizes(q) if k not in out else [1] * n for k, q in enumerate(cands)]          # (rows of the skipped: never read)
    d = [[_case_dist(orc, case, f, q) for f in range(n)] if k not in out else [0] * n for k, q in enumerate(cands)]
    for rule, limit in ((rd.BEST_IN_BUDGET, 1 << 40), (rd.SMALLEST_AT_DISTORTION, 1 << 60), (rd.SMALLEST_AT_DISTORTION, 0)):
        picks, over = _model(rule, s, d, [limit] * n, out)
        assert all(k < 2 for k in picks)
        got, sizes, chosen, dist, status = _rd_device(torch, case.enc, case.dev, cands, rule, limit, FIRST)
        assert status == (OVER_BIT[rule] if over else 0) and bool(over) == (limit == 0)
        assert chosen == [cands[k] for k in picks] and dist == [d[k][f] for f, k in enumerate(picks)]
        assert (got, sizes) == case.records([cands[k] for k in picks])
    _, _, chosen, _, status = _rd_device(torch, case.enc, case.dev, (90, 92), rd.BEST_IN_BUDGET, 1 << 40, FIRST)
    assert chosen == [90] * n and status & _ffi.STATUS_UNENCODABLE
    with pytest.raises(EncoderError) as ei:
        case.enc.encode_best_in_budget(case.dev, 1 << 40, (90, 92))
    assert ei.value.code == _ffi.E_UNENCODABLE
    # the encoder is exact afterwards
    picks, _ = _model(rd.BEST_IN_BUDGET, s, d, [1 << 40] * n, out)
    assert _rd_device(torch, case.enc, case.dev, cands, rd.BEST_IN_BUDGET, 1 << 40, FIRST)[:2] == case.records([cands[k] for k in picks])
    case.close()


def test_gradient_best_in_budget_picks_38_where_the_byte_rule_picks_92(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    W, H = 352, 288
    pic = rd.gradient_frame(W, H)
    enc = Mpeg1Encoder(W, H, 92, "full", max_frames=1)
    dev = torch.from_numpy(pic[None]).cuda()
    got, sizes, chosen, over = enc.encode_to_budget(dev, 8000, rd.GRADIENT_QUALITIES)
    assert (chosen, sizes, over) == ([92], [7507], [])
    got, sizes, chosen, over, dist = enc.encode_best_in_budget(dev, 8000, rd.GRADIENT_QUALITIES)
    assert (chosen, sizes, over, dist) == ([38], [7815], [], [1400207])
    assert got == orc.encode_frame(pic, W, H, 0, 38, orc.MODE_FULL)
    got, sizes, chosen, over, dist = enc.encode_to_distortion(dev, 1_500_000, rd.GRADIENT_QUALITIES)
    assert (chosen, sizes, over, dist) == ([38], [7815], [], [1400207])
    enc.close()


# ---- 3. launches, argument errors -------------------------------------------------------------------------------------------
def test_a_profiled_call_counts_two_launches(torch_cuda, noise):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(noise["W"], noise["H"], 12, "full", max_frames=noise["n"])
    dev = torch_cuda.from_numpy(noise["px"]).cuda()
    enc.profile(True)
    enc.encode_best_in_budget(dev, _noise_limits(noise, rd.BEST_IN_BUDGET, "scalar")[0], NOISE_CANDS)
    launches, _ = enc.profile_read()
    enc.profile(False)
    assert launches == 2
    enc.close()


def test_argument_errors(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=2)
    dev = torch.zeros((2, 288, 352, 3), dtype=torch.uint8, device="cuda")
    big = torch.zeros((3, 288, 352, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(enc.frame_bound * 3, dtype=torch.uint8, device="cuda")
    meta = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    L = _ffi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    good = (C.c_uint8 * 2)(4, 8)

    def call(rgb=dev, n=2, cands=good, k=2, rule=0, d_out=out):
        return L.m1v_encode_rd_device(enc._h, p(rgb) if rgb is not None else None, n, 0, cands, k, rule, 5000, None, None,
                                      p(d_out) if d_out is not None else None, out.numel(), None, None, p(meta),
                                      C.c_void_p(meta.data_ptr() + 8), None)

    assert call(rule=2) == _ffi.E_ARG and "rule" in _ffi.last_error()
    assert call(rule=-1) == _ffi.E_ARG
    for bad in ((4, 4), (8, 4), (0, 4), (4, 13)):
        assert call(cands=(C.c_uint8 * 2)(*bad)) == _ffi.E_ARG, bad
    assert call(k=0) == _ffi.E_ARG and call(k=9) == _ffi.E_ARG and call(cands=None) == _ffi.E_ARG
    assert call(rgb=big, n=3) == _ffi.E_ARG and call(n=-1) == _ffi.E_ARG
    assert call(rgb=None) == _ffi.E_ARG and call(d_out=None) == _ffi.E_ARG
    for limit in (-1, 1 << 64):
        with pytest.raises(EncoderError) as ei:
            enc.encode_best_in_budget(dev, limit, (4, 8))
        assert ei.value.code == _ffi.E_ARG
    # an encoder forced to the run kernels has no fused table: M1V_E_ARG, before any launch
    enc.debug_set_path("runs")
    assert enc.size_table_fused == 0
    assert call() == _ffi.E_ARG and "fused" in _ffi.last_error()
    torch.cuda.synchronize()
    assert [int(x) for x in meta.cpu()] == [-9, -9] and int(out.max().cpu()) == 0
    # an empty batch: total and status written as 0, nothing else
    enc.debug_set_path("auto")
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in meta.cpu()] == [0, 0]
    enc.close()
