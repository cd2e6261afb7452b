"""GPU tests of the batch byte budget and the constant bitrate (m1v_encode_batch_budget_device, m1v_encode_cbr_device;
Mpeg1Encoder.encode_to_batch_budget, encode_at_bitrate) (-m gpu).  Every expectation is a rule of tests/test_rate_abi.py applied
to the oracle's record sizes, and every byte is compared with the oracle's records at the picked qualities and global frame
indices."""
import ctypes as C

import numpy as np
import pytest

from gpu_calls import _frames, _mixed_frames, _oracle
from rate_rules import batch_rule, cbr_rule
from table_cases import RCANDS, SEQUENCE, RateMixed, _table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(W, H, n, producer, pipelined=False, channels=3, quality=12):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, quality, "full", channels=channels, max_frames=n)
    if producer == "runs" and channels == 3:
        enc.debug_set_path("runs")
    assert enc.path == producer
    if pipelined:
        enc.set_pipelined(True)
    return enc


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. batch budget against the rule -------------------------------------------------------------------------------------
def _batch_budgets(s):
    """Below T[0], T[k] and T[k] +- 1, both sides of an upgrade-prefix boundary, the top and above."""
    K = len(s)
    T = [sum(r) for r in s]
    out = {T[0] - 1, max(T), max(T) + 1000}
    for k in range(K):
        out |= {T[k] - 1, T[k], T[k] + 1}
    k = K // 2 - 1 if K > 1 else 0
    if k + 1 < K and T[k] <= T[k + 1]:
        n = len(s[0])
        d = [s[k + 1][f] - s[k][f] for f in range(n)]
        free = sum(-x for x in d if x <= 0)
        pos = sorted(x for x in d if x > 0)
        for i in range(1, len(pos) + 1):          # exactly i upgrades fit, and one byte short of that
            B = T[k] - free + sum(pos[:i])
            if T[k] <= B < T[k + 1]:
                out |= {B, B - 1}
    return sorted(b for b in out if b >= 0)


@pytest.mark.parametrize("cands", [(2, 5, 9, 12), (1, 2, 4, 6, 8, 10, 11, 12)], ids=["k4", "k8"])
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_batch_budget_matches_the_rule(torch_cuda, orc, producer, cands):
    n, first = 8, 40
    enc = _encoder(352, 288, n, producer)
    rng = np.random.default_rng(61 + len(cands))
    rgb = _mixed_frames(rng, n, 352, 288, 3)
    dev = torch_cuda.from_numpy(rgb).cuda()
    s = _table(orc, rgb, cands)
    budgets = _batch_budgets(s)
    seen = set()
    for B in budgets:
        pick, over = batch_rule(s, B)
        seen.add((over, len(set(pick))))
        chosen = [cands[k] for k in pick]
        got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, cands, first_frame_index=first)
        want, wsizes = _oracle(orc, rgb, first, chosen, orc.MODE_FULL, 3)
        assert (ch, ov, sizes) == (chosen, over, wsizes), B
        assert got == want and (over or len(got) <= B), B
    assert (True, 1) in seen and (False, 2) in seen, seen     # below T[0]; a mixed pick inside the upgrade prefix
    enc.close()


# ---- 2. ties over many frames ---------------------------------------------------------------------------------------------
def test_ties_over_many_frames(torch_cuda, orc):
    """4,500 pictures of 32x32 made of five distinct frames: the upgrades tie on d across hundreds of frames and the kernel
    loops far past its lanes.  Budgets cut inside a tie group."""
    W = H = 32
    n, cands, first = 4500, (2, 5, 8, 12), 3
    rng = np.random.default_rng(71)
    distinct = _mixed_frames(rng, 5, W, H, 3, amps=(4, 256, 40, 120, 10))
    order = rng.integers(0, 5, n)
    rgb = distinct[order]
    enc = _encoder(W, H, n, "tiles")
    dev = torch_cuda.from_numpy(rgb).cuda()
    ds = _table(orc, distinct, cands)
    s = [[row[i] for i in order] for row in ds]
    T = [sum(r) for r in s]
    budgets = []
    for k in (1, 2):                             # (between 5 and 8 every frame ties; between 8 and 12 only some grow)
        d = [s[k + 1][f] - s[k][f] for f in range(n)]
        free = sum(-x for x in d if x <= 0)
        acc = 0
        for g in sorted(set(x for x in d if x > 0)):   # half of a tie group fits, and one byte short of half and one more
            members = sum(1 for x in d if x == g)
            budgets += [(k, T[k] - free + acc + g * (members // 2)), (k, T[k] - free + acc + g * (members // 2) + g - 1)]
            acc += g * members
    budgets = [(k, B) for k, B in budgets if T[k] <= B < T[k + 1]][:4]
    assert len(budgets) >= 2, budgets
    for k, B in budgets:
        pick, over = batch_rule(s, B)
        assert not over and 0 < sum(p == k + 1 for p in pick) < n
        got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, cands, first_frame_index=first)
        chosen = [cands[p] for p in pick]
        assert ch == chosen and ov == over, B
        assert sizes == [s[p][f] for f, p in enumerate(pick)] and len(got) == sum(sizes) <= B
    # the bytes of the last call, frame by frame
    want, _ = _oracle(orc, rgb, first, chosen, orc.MODE_FULL, 3)
    assert got == want
    enc.close()


# ---- 3. bitrate chained across queued calls -------------------------------------------------------------------------------
CHAIN = (7, 1, 12, 5)
# flat frames, cheap at every candidate, and bursts of noise, dearer at every candidate than a refill: the level falls below
# zero during a burst and recovers after it
BURSTS = (4, 10, 4, 256, 256, 256, 256, 4, 10, 4, 10, 4, 4, 40, 4, 10, 4, 4, 256, 4, 10, 4, 40, 4, 10)


def _cbr_params(s):
    """(r, C, L0) under which the stream has a frame that fits nothing at a negative level whose debt later refills repay,
    refills clipped at C, an initial level above C, and more frames that fit than not, at more than one candidate."""
    sizes = [x for row in s for x in row]
    for r in range(min(sizes) // 2, max(sizes), 16):
        for C_ in (r, 5 * r // 4, 3 * r // 2, 2 * r):
            L0 = 3 * C_
            L = min(L0, C_)
            pick, over, _ = cbr_rule(s, r, C_, L0)
            debt = repaid = clip = False
            for f, k in enumerate(pick):
                debt |= L < 0 and f in over
                repaid |= debt and L >= 0
                clip |= L - s[k][f] + r > C_
                L = min(C_, L - s[k][f] + r)
            if debt and repaid and clip and len(set(pick)) > 1 and len(over) < len(pick) // 2:
                return r, C_, L0
    raise AssertionError("no bitrate gives the cases this test needs")


def _cbr_queue(torch, enc, dev_batches, firsts, cands, r, C_, levels, aliased=False):
    """One m1v_encode_cbr_device per batch, back to back on the current stream, call i reading levels[i] and writing
    levels[i + 1] (or levels[0] in place when aliased).  Returns the per-call (out, sizes, meta, chosen)."""
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * len(cands))(*cands)
    res = []
    for i, (dev, first) in enumerate(zip(dev_batches, firsts)):
        n = dev.shape[0]
        out = torch.zeros(enc.frame_bound * max(n, 1), dtype=torch.uint8, device="cuda")
        sizes = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
        meta = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        chosen = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        lin = levels[0] if aliased else levels[i]
        lout = levels[0] if aliased else levels[i + 1]
        rc = L.m1v_encode_cbr_device(enc._h, C.c_void_p(dev.data_ptr()), n, first, q, len(cands), r, C_,
                                     C.c_void_p(lin.data_ptr()), C.c_void_p(lout.data_ptr()), C.c_void_p(chosen.data_ptr()),
                                     C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(sizes.data_ptr()),
                                     C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8), _stream(torch))
        assert rc == 0, _ffi.last_error()
        res.append((out, sizes, meta, chosen))
    enc.flush()
    torch.cuda.synchronize()
    return res


def _check_chain(torch, orc, rgb, batches, firsts, res, s, cands, r, C_, L0, levels, channels, aliased=False):
    from ec504_imageencoder_amd import _ffi
    pick, over, _ = cbr_rule(s, r, C_, L0)
    lvl = L0
    off = 0
    for i, n in enumerate(batches):
        part = [row[off:off + n] for row in s]
        p, o, lvl = cbr_rule(part, r, C_, lvl)
        assert p == pick[off:off + n] and [f + off for f in o] == [f for f in over if off <= f < off + n]
        out, sizes, meta, chosen = res[i]
        total, status = (int(x) for x in meta.cpu())
        status &= 0xFFFFFFFF                     # (a uint32 status word in an int64 slot)
        assert status == (_ffi.STATUS_OVER_BUDGET if o else 0), (i, status)
        qs = [cands[k] for k in p]
        assert [int(c) for c in chosen[:n].cpu()] == qs, i
        want, wsizes = _oracle(orc, rgb[off:off + n], firsts[i], qs, orc.MODE_FULL, channels)
        assert [int(x) for x in sizes[:n].cpu()] == wsizes and total == len(want), i
        assert out[:total].cpu().numpy().tobytes() == want, i
        if not aliased:
            assert int(levels[i + 1].cpu()[0]) == lvl, i
        off += n
    if aliased:
        assert int(levels[0].cpu()[0]) == lvl
    return lvl


@pytest.mark.parametrize("setup", [("tiles", False, 3), ("tiles", True, 3), ("runs", False, 3), ("runs", True, 3),
                                   ("runs", False, 4)], ids=["tiles", "tiles_pipelined", "runs", "runs_pipelined", "rgba"])
def test_bitrate_chained_across_queued_calls(torch_cuda, orc, setup):
    producer, pipelined, channels = setup
    cands = (12, 20, 30, 40)
    total = sum(CHAIN)
    rng = np.random.default_rng(81 + channels)
    rgb = _mixed_frames(rng, total, 352, 288, channels, amps=BURSTS)
    enc = _encoder(352, 288, max(CHAIN), producer, pipelined, channels, quality=40)
    s = _table(orc, rgb, cands, channels)
    r, C_, L0 = _cbr_params(s)
    assert L0 > C_
    dev = torch_cuda.from_numpy(rgb).cuda()
    starts = np.cumsum((0,) + CHAIN)
    batches = [dev[starts[i]:starts[i + 1]] for i in range(len(CHAIN))]
    firsts = [500 + 3 * int(starts[i]) for i in range(len(CHAIN))]
    levels = [torch_cuda.full((1,), L0 if i == 0 else -7, dtype=torch_cuda.int64, device="cuda") for i in range(len(CHAIN) + 1)]
    res = _cbr_queue(torch_cuda, enc, batches, firsts, cands, r, C_, levels)
    _check_chain(torch_cuda, orc, rgb, list(CHAIN), firsts, res, s, cands, r, C_, L0, levels, channels)
    assert int(levels[0].cpu()[0]) == L0                     # separate pointers: the first level is untouched
    enc.close()


# ---- 4. aliased level pointers, empty batches -----------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_aliased_level_and_empty_batch(torch_cuda, orc, producer):
    from ec504_imageencoder_amd import _ffi
    cands = (4, 8, 12)
    rng = np.random.default_rng(91)
    rgb = _mixed_frames(rng, 9, 352, 288, 3)
    enc = _encoder(352, 288, 6, producer)
    s = _table(orc, rgb, cands)
    r = sorted(s[-1])[4]
    C_, L0 = 3 * r, 10 * r
    dev = torch_cuda.from_numpy(rgb).cuda()
    batches, firsts = [dev[:6], dev[6:]], [0, 6]
    separate = [torch_cuda.full((1,), L0, dtype=torch_cuda.int64, device="cuda") for _ in range(3)]
    res = _cbr_queue(torch_cuda, enc, batches, firsts, cands, r, C_, separate)
    want = _check_chain(torch_cuda, orc, rgb, [6, 3], firsts, res, s, cands, r, C_, L0, separate, 3)
    aliased = [torch_cuda.full((1,), L0, dtype=torch_cuda.int64, device="cuda")]
    res = _cbr_queue(torch_cuda, enc, batches, firsts, cands, r, C_, aliased, aliased=True)
    assert _check_chain(torch_cuda, orc, rgb, [6, 3], firsts, res, s, cands, r, C_, L0, aliased, 3, aliased=True) == want
    # n_frames == 0: total 0, status 0, level_out = min(level_in, C)
    L = _ffi.lib()
    q = (C.c_uint8 * len(cands))(*cands)
    for lin_value in (L0, C_ - 5, -12345):
        lin = torch_cuda.full((1,), lin_value, dtype=torch_cuda.int64, device="cuda")
        lout = torch_cuda.full((1,), 77, dtype=torch_cuda.int64, device="cuda")
        meta = torch_cuda.full((2,), -1, dtype=torch_cuda.int64, device="cuda")
        out = torch_cuda.zeros(16, dtype=torch_cuda.uint8, device="cuda")
        assert L.m1v_encode_cbr_device(enc._h, C.c_void_p(dev.data_ptr()), 0, 0, q, len(cands), r, C_, C.c_void_p(lin.data_ptr()),
                                       C.c_void_p(lout.data_ptr()), None, C.c_void_p(out.data_ptr()), 16, None,
                                       C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8), _stream(torch_cuda)) == 0
        enc.flush()
        torch_cuda.cuda.synchronize()
        assert int(lout.cpu()[0]) == min(lin_value, C_) and int(lin.cpu()[0]) == lin_value
        assert [int(x) & 0xFFFFFFFF for x in meta.cpu()] == [0, 0]
        meta.fill_(-1)
        assert L.m1v_encode_batch_budget_device(enc._h, C.c_void_p(dev.data_ptr()), 0, 0, q, len(cands), 10, None,
                                                C.c_void_p(out.data_ptr()), 16, None, C.c_void_p(meta.data_ptr()),
                                                C.c_void_p(meta.data_ptr() + 8), _stream(torch_cuda)) == 0
        enc.flush()
        torch_cuda.cuda.synchronize()
        assert [int(x) & 0xFFFFFFFF for x in meta.cpu()] == [0, 0]
    enc.close()


# ---- 5. launches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_launch_count(torch_cuda, orc, producer):
    cands = (2, 4, 6, 8, 12)
    n = 5
    enc = _encoder(352, 288, n, producer)
    rng = np.random.default_rng(101)
    rgb = _mixed_frames(rng, n, 352, 288, 3)
    dev = torch_cuda.from_numpy(rgb).cuda()
    s = _table(orc, rgb, cands)
    expect = 2 if producer == "tiles" else len(cands) + 1
    level = torch_cuda.full((1,), 10 ** 6, dtype=torch_cuda.int64, device="cuda")
    for call in ("batch", "cbr"):
        enc.profile(True)
        if call == "batch":
            B = (sum(s[1]) + sum(s[2])) // 2
            got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, cands)
            pick, over = batch_rule(s, B)
        else:
            r = sorted(s[2])[2]
            got, sizes, ch, ov = enc.encode_at_bitrate(dev, r, 2 * r, cands, level)
            pick, over, lvl = cbr_rule(s, r, 2 * r, 10 ** 6)
            assert int(level.cpu()[0]) == lvl
        launches, _ = enc.profile_read()
        enc.profile(False)
        assert launches == expect, (call, launches)
        chosen = [cands[k] for k in pick]
        want, wsizes = _oracle(orc, rgb, 0, chosen, orc.MODE_FULL, 3)
        assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), call
    enc.close()


# ---- 6. interleaved with every other kind of call -------------------------------------------------------------------------


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_interleaved_calls_stay_exact(torch_cuda, orc, producer, pipelined):
    enc = _encoder(352, 288, 5, producer, pipelined)
    calls = RateMixed(torch_cuda, orc, enc, seed=300 + pipelined + 2 * len(producer))
    for _ in range(2):
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("sequence", producer, pipelined))
    enc.close()


# ---- 7. injected failures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["batch", "cbr"])
@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_failed_call_leaves_the_encoder_correct(torch_cuda, orc, producer, stage, form):
    from ec504_imageencoder_amd import _ffi
    enc = _encoder(352, 288, 5, producer, pipelined=stage == 2)
    calls = RateMixed(torch_cuda, orc, enc, seed=400 + 10 * stage + len(form))
    calls.call("cbr", 3)
    calls.call("plain", 4)
    calls.check("before")
    dev = torch_cuda.from_numpy(_frames(calls.rng, 5, 352, 288, 3)).cuda()
    L = _ffi.lib()
    q = (C.c_uint8 * len(RCANDS))(*RCANDS)
    out = torch_cuda.zeros(enc.frame_bound * 5, dtype=torch_cuda.uint8, device="cuda")
    meta = torch_cuda.zeros(2, dtype=torch_cuda.int64, device="cuda")
    lin = torch_cuda.full((1,), 99999, dtype=torch_cuda.int64, device="cuda")
    lout = torch_cuda.full((1,), -3, dtype=torch_cuda.int64, device="cuda")
    L.m1v_debug_fail_encode(stage)
    try:
        if form == "batch":
            rc = L.m1v_encode_batch_budget_device(enc._h, C.c_void_p(dev.data_ptr()), 5, 0, q, len(RCANDS), 10 ** 6, None,
                                                  C.c_void_p(out.data_ptr()), out.numel(), None, C.c_void_p(meta.data_ptr()),
                                                  C.c_void_p(meta.data_ptr() + 8), _stream(torch_cuda))
        else:
            rc = L.m1v_encode_cbr_device(enc._h, C.c_void_p(dev.data_ptr()), 5, 0, q, len(RCANDS), 5000, 20000,
                                         C.c_void_p(lin.data_ptr()), C.c_void_p(lout.data_ptr()), None, C.c_void_p(out.data_ptr()),
                                         out.numel(), None, C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8),
                                         _stream(torch_cuda))
        assert rc == _ffi.E_HIP
    finally:
        L.m1v_debug_fail_encode(0)
    enc.flush()
    torch_cuda.cuda.synchronize()
    assert int(lin.cpu()[0]) == 99999
    for kind, n in SEQUENCE:
        calls.call(kind, n)
    calls.check("after the failure")
    enc.close()


# ---- 8. argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, _ffi
    enc = _encoder(352, 288, 2, "tiles")
    dev = torch_cuda.zeros((2, 288, 352, 3), dtype=torch_cuda.uint8, device="cuda")
    big = torch_cuda.zeros((3, 288, 352, 3), dtype=torch_cuda.uint8, device="cuda")
    out = torch_cuda.zeros(enc.frame_bound * 3, dtype=torch_cuda.uint8, device="cuda")
    meta = torch_cuda.full((2,), -9, dtype=torch_cuda.int64, device="cuda")
    chosen = torch_cuda.full((3,), 0xee, dtype=torch_cuda.uint8, device="cuda")
    lin = torch_cuda.full((1,), 1000, dtype=torch_cuda.int64, device="cuda")
    lout = torch_cuda.full((1,), -9, dtype=torch_cuda.int64, device="cuda")
    L = _ffi.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def batch(rgb, n, quals, o=out):
        q = (C.c_uint8 * max(len(quals), 1))(*quals)
        return L.m1v_encode_batch_budget_device(enc._h, p(rgb), n, 0, q, len(quals), 10 ** 6, p(chosen), p(o), out.numel(), None,
                                                p(meta), C.c_void_p(meta.data_ptr() + 8), None)

    def cbr(rgb, n, quals, r=100, cap=1000, li=lin, lo=lout, o=out):
        q = (C.c_uint8 * max(len(quals), 1))(*quals)
        return L.m1v_encode_cbr_device(enc._h, p(rgb), n, 0, q, len(quals), r, cap, p(li), p(lo), p(chosen), p(o), out.numel(),
                                       None, p(meta), C.c_void_p(meta.data_ptr() + 8), None)

    for quals in ((), (4, 4), (8, 4), (0, 4), (4, 13), tuple(range(1, 10))):
        assert batch(dev, 2, quals) == _ffi.E_ARG and cbr(dev, 2, quals) == _ffi.E_ARG, quals
    good = (4, 8)
    assert batch(big, 3, good) == _ffi.E_ARG and cbr(big, 3, good) == _ffi.E_ARG
    assert batch(dev, -1, good) == _ffi.E_ARG and cbr(dev, -1, good) == _ffi.E_ARG
    assert batch(None, 2, good) == _ffi.E_ARG and cbr(None, 2, good) == _ffi.E_ARG
    assert batch(dev, 2, good, o=None) == _ffi.E_ARG and cbr(dev, 2, good, o=None) == _ffi.E_ARG
    assert cbr(dev, 2, good, li=None) == _ffi.E_ARG and cbr(dev, 2, good, lo=None) == _ffi.E_ARG
    for r, cap in ((0, 1000), (1001, 1000), (1, 2 ** 62), (2 ** 62, 2 ** 62), (2 ** 63, 2 ** 64 - 1)):
        assert cbr(dev, 2, good, r=r, cap=cap) == _ffi.E_ARG, (r, cap)
    assert cbr(dev, 0, good, r=1, cap=2 ** 62 - 1) == 0          # the largest capacity and the smallest rate are valid
    torch_cuda.cuda.synchronize()
    assert int(lout.cpu()[0]) == 1000                              # (only that call wrote: min(1000, C))
    assert [int(x) for x in chosen.cpu()] == [0xee] * 3            # nothing was launched by the refused calls
    level = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda")
    for r, cap in ((0, 10), (11, 10), (5, 2 ** 62)):
        with pytest.raises(EncoderError) as ei:
            enc.encode_at_bitrate(dev, r, cap, good, level)
        assert ei.value.code == _ffi.E_ARG
    with pytest.raises(EncoderError) as ei:
        enc.encode_to_batch_budget(dev, 10 ** 6, (8, 4))
    assert ei.value.code == _ffi.E_ARG
    for budget in (-1, 2 ** 64):                                   # a scalar budget that does not fit uint64
        with pytest.raises(EncoderError) as ei:
            enc.encode_to_budget(dev, budget, good)
        assert ei.value.code == _ffi.E_ARG
    enc.close()
