"""GPU tests of per-frame quality factors, the frame-size probe and the budget encode (-m gpu).

m1v_encode_quality_device, m1v_frame_sizes_device and m1v_encode_budget_device (include/mpeg1_hip.h).  A frame record depends
only on the frame's pixels, its global index and its quality factor, so the expected stream of a per-frame call is the
concatenation of the oracle's single-frame records, each at its own quality."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _frames(rng, n, W, H, channels, amp=256):
    """n frames of noise (amp 256) or of gentle noise around mid-grey (small amp: encodable at any quality factor)."""
    shape = (n, H, W, channels)
    if amp >= 256:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (128 - amp // 2 + rng.integers(0, amp, shape)).astype(np.uint8)


def _mixed_frames(rng, n, W, H, channels):
    """Frames whose record sizes differ a lot: flat, gentle and full noise in turn."""
    amps = (4, 40, 256, 120)
    return np.concatenate([_frames(rng, 1, W, H, channels, amps[f % len(amps)]) for f in range(n)])


def _oracle(orc, rgb, first, qs, mode, channels):
    """(bytes, sizes): frame f at quality qs[f] with global index first + f."""
    W, H = rgb.shape[2], rgb.shape[1]
    recs = [orc.encode_frame(rgb[f], W, H, first + f, int(qs[f]), mode, channels=channels) for f in range(rgb.shape[0])]
    return b"".join(recs), [len(r) for r in recs]


def _encode_checked(torch, enc, dev, first, qs):
    """One per-frame call through Mpeg1Encoder.encode (no retry): (bytes, sizes, status)."""
    out, sizes, meta = enc.encode(dev, first, quality=qs)
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    n = dev.shape[0]
    return out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()], status & 0xFFFFFFFF


# ---- 1. uniform quality = the plain call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "full"])
@pytest.mark.parametrize("producer", ["tiles", "runs", "runs4"])
def test_uniform_quality_equals_plain(torch_cuda, producer, mode):
    """A quality array holding the encoder's own quality gives the bytes and sizes of encode_to_bytes (STRICT: the strip
    kernel; FULL: the tile kernel, the run kernel forced, 4-channel input)."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    C_ = 4 if producer == "runs4" else 3
    enc = Mpeg1Encoder(352, 288, 12, mode, channels=C_, max_frames=4)
    if producer == "runs":
        enc.debug_set_path("runs")
    rng = np.random.default_rng(7)
    dev = torch_cuda.from_numpy(_frames(rng, 4, 352, 288, C_)).cuda()
    want = enc.encode_to_bytes(dev, 300)
    assert enc.encode_to_bytes(dev, 300, quality=[12] * 4) == want
    q = torch_cuda.full((4,), 12, dtype=torch_cuda.uint8, device="cuda")
    assert enc.encode_to_bytes(dev, 300, quality=q) == want
    enc.close()


# ---- 2. per-frame qualities against the oracle ---------------------------------------------------------------------------
CASES = {
    # name: (W, H, channels, Q, n, amp, path, lds_words, qualities drawn from)
    "1080p": (1920, 1080, 3, 12, 4, 256, None, 0, None),
    "odd366": (366, 200, 3, 12, 5, 256, None, 0, None),
    "tiny105x49": (105, 49, 3, 12, 5, 256, None, 0, None),
    "cif4ch_runs": (352, 288, 4, 12, 5, 256, None, 0, None),
    "4k": (3840, 2160, 3, 12, 2, 256, None, 0, None),
    "q90_tiles": (352, 288, 3, 90, 6, 40, None, 0, (20, 60, 76, 77, 85, 90)),
    "q90_runs": (352, 288, 3, 90, 6, 40, "runs", 0, (20, 60, 76, 77, 85, 90)),
    "global_fallback_tiles": (352, 288, 3, 12, 4, 256, None, 8, None),
    "global_fallback_runs": (352, 288, 3, 12, 4, 256, "runs", 8, None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_per_frame_quality_matches_oracle(torch_cuda, orc, case):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, C_, Q, n, amp, path, lds_words, pool = CASES[case]
    enc = Mpeg1Encoder(W, H, Q, "full", channels=C_, max_frames=n)
    if path:
        enc.debug_set_path(path)
    if lds_words:
        enc.debug_set_lds_words(lds_words)      # every unit builds its bits in global memory
        enc.reserve_scratch(True)
    rng = np.random.default_rng(sum(map(ord, case)))
    rgb = _frames(rng, n, W, H, C_, amp)
    qs = [int(x) for x in (rng.choice(pool, n) if pool else rng.integers(1, Q + 1, n))]
    qs[0] = Q                                   # the encoder's own quality and the coarsest one are always in the batch
    qs[-1] = 1 if not pool else qs[-1]
    first = 256 - n // 2                        # the hour fields wrap inside the batch
    dev = torch_cuda.from_numpy(rgb).cuda()
    got, sizes, status = _encode_checked(torch_cuda, enc, dev, first, qs)
    want, wsizes = _oracle(orc, rgb, first, qs, orc.MODE_FULL, C_)
    assert status == 0, status
    assert sizes == wsizes, (qs, sizes, wsizes)
    assert got == want, qs
    enc.close()


def test_per_frame_quality_pipelined(torch_cuda, orc):
    """Pipelined mode: batches with their own qualities in flight on both internal Batches, one flush at the end."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=4)
    enc.set_pipelined(True)
    rng = np.random.default_rng(11)
    pending = []
    for k in range(5):
        n = (4, 1, 3, 4, 2)[k]
        rgb = _frames(rng, n, 352, 288, 3)
        qs = [int(x) for x in rng.integers(1, 13, n)]
        out = torch_cuda.empty(enc.default_out_capacity(n), dtype=torch_cuda.uint8, device="cuda")
        dev = torch_cuda.from_numpy(rgb).cuda()
        pending.append((rgb, qs, 250 + 3 * k, dev, enc.encode(dev, 250 + 3 * k, out=out, quality=qs)))
    enc.flush()
    torch_cuda.cuda.synchronize()
    for rgb, qs, first, _, (out, sizes, meta) in pending:
        total, status = (int(x) for x in meta.cpu())
        want, wsizes = _oracle(orc, rgb, first, qs, orc.MODE_FULL, 3)
        assert status == 0 and [int(s) for s in sizes[:len(qs)].cpu()] == wsizes
        assert out[:total].cpu().numpy().tobytes() == want, qs
    enc.close()


# ---- 3. invalid qualities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "runs"])
@pytest.mark.parametrize("bad", [0, 13, 255])
def test_invalid_quality_sets_status_and_next_call_is_exact(torch_cuda, orc, producer, bad):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=3)
    if producer == "runs":
        enc.debug_set_path("runs")
    rng = np.random.default_rng(bad)
    rgb = _frames(rng, 3, 352, 288, 3)
    dev = torch_cuda.from_numpy(rgb).cuda()
    _, _, status = _encode_checked(torch_cuda, enc, dev, 0, [5, bad, 12])
    assert status & _ffi.STATUS_QUALITY, status
    st = torch_cuda.zeros(1, dtype=torch_cuda.int32, device="cuda")
    enc.frame_sizes(dev, quality=[bad, 3, 4], status=st)
    torch_cuda.cuda.synchronize()
    assert int(st.item()) & _ffi.STATUS_QUALITY
    with pytest.raises(EncoderError):
        enc.encode_to_bytes(dev, 0, quality=[bad, 3, 4])
    got, sizes = enc.encode_to_bytes(dev, 7)
    want, wsizes = _oracle(orc, rgb, 7, [12] * 3, orc.MODE_FULL, 3)
    assert got == want and sizes == wsizes
    got, sizes, status = _encode_checked(torch_cuda, enc, dev, 9, [1, 2, 3])
    want, wsizes = _oracle(orc, rgb, 9, [1, 2, 3], orc.MODE_FULL, 3)
    assert status == 0 and got == want and sizes == wsizes
    enc.close()


# ---- 4. the size probe ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "runs", "strips"])
def test_frame_sizes_probe(torch_cuda, orc, producer):
    """frame_sizes equals the oracle's record sizes and the per-frame encode's; it writes n sizes and nothing else (the
    output of the call before it and the entries past n stay as they were)."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    W, H, C_, mode = (352, 144, 4, "full") if producer == "strips" else (352, 288, 3, "full")
    enc = Mpeg1Encoder(W, H, 12, mode, channels=C_, max_frames=5)
    if producer == "runs":
        enc.debug_set_path("runs")
    assert enc.path == ("tiles" if producer == "tiles" else "runs")
    rng = np.random.default_rng(3)
    rgb = _mixed_frames(rng, 5, W, H, C_)
    dev = torch_cuda.from_numpy(rgb).cuda()
    qs = [12, 1, 7, 3, 12]
    out, _, meta = enc.encode(dev, 40, quality=qs)
    torch_cuda.cuda.synchronize()
    before = out.clone()
    sizes = torch_cuda.full((8,), -77, dtype=torch_cuda.int64, device="cuda")
    status = torch_cuda.full((1,), 0x40, dtype=torch_cuda.int32, device="cuda")
    q = torch_cuda.tensor(qs, dtype=torch_cuda.uint8).cuda()
    rc = _ffi.lib().m1v_frame_sizes_device(enc._h, C.c_void_p(dev.data_ptr()), 5, C.c_void_p(q.data_ptr()),
                                           C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()),
                                           C.c_void_p(torch_cuda.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch_cuda.cuda.synchronize()
    _, wsizes = _oracle(orc, rgb, 40, qs, orc.MODE_FULL, C_)
    got = [int(s) for s in sizes.cpu()]
    assert got[:5] == wsizes and got[5:] == [-77] * 3
    assert int(status.item()) == 0
    assert torch_cuda.equal(out, before)
    assert int(meta[1].item()) == 0
    assert [int(s) for s in enc.frame_sizes(dev).cpu()] == _oracle(orc, rgb, 0, [12] * 5, orc.MODE_FULL, C_)[1]
    enc.close()


# ---- 5. the budget encode -------------------------------------------------------------------------------------------------
CANDS = (2, 4, 8, 12)


def _rule(size_table, budgets):
    """The largest candidate whose record fits, else the smallest: (chosen, over-budget frames)."""
    chosen, over = [], []
    for f, cap in enumerate(budgets):
        fits = [c for c in CANDS if size_table[c][f] <= cap]
        chosen.append(fits[-1] if fits else CANDS[0])
        if not fits:
            over.append(f)
    return chosen, over


@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_budget_encode(torch_cuda, orc, producer):
    from ec504_imageencoder_amd import Mpeg1Encoder
    n = 8
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=n)
    if producer == "runs":
        enc.debug_set_path("runs")
    rng = np.random.default_rng(5)
    rgb = _mixed_frames(rng, n, 352, 288, 3)
    dev = torch_cuda.from_numpy(rgb).cuda()
    first = 252
    table = {c: _oracle(orc, rgb, first, [c] * n, orc.MODE_FULL, 3)[1] for c in CANDS}
    # one budget for every frame, between the sizes: the choices vary across frames
    allsizes = sorted(s for c in CANDS for s in table[c])
    budget = allsizes[len(allsizes) // 2]
    chosen, over = _rule(table, [budget] * n)
    assert len(set(chosen)) > 1, chosen
    got, sizes, ch, ov = enc.encode_to_budget(dev, budget, CANDS, first_frame_index=first)
    want, wsizes = _oracle(orc, rgb, first, chosen, orc.MODE_FULL, 3)
    assert ch == chosen and ov == over and sizes == wsizes and got == want
    # a budget per frame, as a device tensor and as a list
    budgets = [table[CANDS[f % len(CANDS)]][f] for f in range(n)]
    chosen, over = _rule(table, budgets)
    want, wsizes = _oracle(orc, rgb, first, chosen, orc.MODE_FULL, 3)
    for b in (torch_cuda.tensor(budgets, dtype=torch_cuda.int64).cuda(), budgets):
        got, sizes, ch, ov = enc.encode_to_budget(dev, b, CANDS, first_frame_index=first)
        assert ch == chosen and ov == over == [] and sizes == wsizes and got == want
    enc.close()


def test_budget_below_every_candidate(torch_cuda, orc):
    """No candidate fits: the smallest candidate everywhere and M1V_STATUS_OVER_BUDGET (the output is valid)."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    n = 3
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=n)
    rng = np.random.default_rng(9)
    rgb = _frames(rng, n, 352, 288, 3)
    dev = torch_cuda.from_numpy(rgb).cuda()
    got, sizes, ch, ov = enc.encode_to_budget(dev, 100, CANDS, first_frame_index=3)
    want, wsizes = _oracle(orc, rgb, 3, [CANDS[0]] * n, orc.MODE_FULL, 3)
    assert ch == [CANDS[0]] * n and ov == list(range(n)) and sizes == wsizes and got == want
    # the status word itself, through the C entry point
    out = torch_cuda.empty(enc.default_out_capacity(n), dtype=torch_cuda.uint8, device="cuda")
    meta = torch_cuda.zeros(2, dtype=torch_cuda.int64, device="cuda")
    cand = (C.c_uint8 * 4)(*CANDS)
    rc = _ffi.lib().m1v_encode_budget_device(enc._h, C.c_void_p(dev.data_ptr()), n, 3, cand, 4, 100, None, None,
                                             C.c_void_p(out.data_ptr()), out.numel(), None, C.c_void_p(meta.data_ptr()),
                                             C.c_void_p(meta.data_ptr() + 8), None)
    assert rc == 0
    torch_cuda.cuda.synchronize()
    assert int(meta[1].item()) == _ffi.STATUS_OVER_BUDGET
    assert out[:int(meta[0].item())].cpu().numpy().tobytes() == want
    enc.close()


def test_budget_argument_errors(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=2)
    dev = torch_cuda.zeros((2, 288, 352, 3), dtype=torch_cuda.uint8, device="cuda")
    for cands in ((), (4, 4), (8, 4), (0, 4), (4, 13), tuple(range(1, 10))):
        with pytest.raises(EncoderError) as ei:
            enc.encode_to_budget(dev, 10000, cands)
        assert ei.value.code == _ffi.E_ARG, cands
    enc.close()


# ---- 6. encoder state across plain, per-frame, probe and budget calls -------------------------------------------------------
class Mixed:
    """Calls of every kind on one encoder; each call's expected output is computed from the oracle at check time."""

    def __init__(self, torch, orc, enc, seed):
        self.torch, self.orc, self.enc = torch, orc, enc
        self.rng = np.random.default_rng(seed)
        self.pending = []
        self.first = 200

    def call(self, kind, n):
        torch, enc = self.torch, self.enc
        rgb = _mixed_frames(self.rng, n, enc.width, enc.height, enc.channels)
        dev = torch.from_numpy(rgb).cuda()
        self.first += 29
        Q = enc.quality_factor
        if kind == "plain":
            res = enc.encode(dev, self.first)
            self.pending.append((kind, rgb, self.first, [Q] * n, dev, res))
        elif kind == "quality":
            qs = [int(x) for x in self.rng.integers(1, Q + 1, n)]
            res = enc.encode(dev, self.first, quality=qs)
            self.pending.append((kind, rgb, self.first, qs, dev, res))
        elif kind == "probe":
            qs = [int(x) for x in self.rng.integers(1, Q + 1, n)]
            self.pending.append((kind, rgb, self.first, qs, dev, enc.frame_sizes(dev, quality=qs)))
        else:                                    # synchronous: checked at once against the rule on the oracle's sizes
            table = {c: _oracle(self.orc, rgb, self.first, [c] * n, self.orc.MODE_FULL, enc.channels)[1] for c in CANDS}
            budget = sorted(table[8])[0]
            chosen, over = _rule(table, [budget] * n)
            got, sizes, ch, ov = enc.encode_to_budget(dev, budget, CANDS, first_frame_index=self.first)
            want, wsizes = _oracle(self.orc, rgb, self.first, chosen, self.orc.MODE_FULL, enc.channels)
            assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), ("budget", n)

    def check(self, what):
        self.enc.flush()
        self.torch.cuda.synchronize()
        for k, (kind, rgb, first, qs, _, res) in enumerate(self.pending):
            want, wsizes = _oracle(self.orc, rgb, first, qs, self.orc.MODE_FULL, self.enc.channels)
            n = rgb.shape[0]
            if kind == "probe":
                assert [int(s) for s in res[:n].cpu()] == wsizes, (what, k, kind)
                continue
            out, sizes, meta = res
            total, status = (int(x) for x in meta.cpu())
            assert status == 0, (what, k, kind, status)
            assert [int(s) for s in sizes[:n].cpu()] == wsizes, (what, k, kind)
            assert out[:total].cpu().numpy().tobytes() == want, (what, k, kind)
        self.pending = []


SEQUENCE = (("plain", 5), ("probe", 3), ("quality", 5), ("budget", 2), ("plain", 5))


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_interleaved_calls_stay_exact(torch_cuda, orc, producer, pipelined):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=5)
    if producer == "runs":
        enc.debug_set_path("runs")
    if pipelined:
        enc.set_pipelined(True)
    calls = Mixed(torch_cuda, orc, enc, seed=pipelined + 2 * len(producer))
    for _ in range(2):
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("sequence", pipelined))
    enc.close()


@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("pipelined", [False, True])
def test_failed_budget_call_leaves_the_encoder_correct(torch_cuda, orc, pipelined, stage):
    """m1v_debug_fail_encode armed during a budget call: the call fails (in its first probe) with M1V_E_HIP; every call of
    every kind after it is exact."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=5)
    if pipelined:
        enc.set_pipelined(True)
    calls = Mixed(torch_cuda, orc, enc, seed=10 * stage + pipelined)
    calls.call("plain", 5)
    calls.call("quality", 4)
    calls.check("before")
    dev = torch_cuda.from_numpy(_frames(calls.rng, 5, 352, 288, 3)).cuda()
    _ffi.lib().m1v_debug_fail_encode(stage)
    try:
        with pytest.raises(EncoderError) as ei:
            enc.encode_to_budget(dev, 20000, CANDS)
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    enc.flush()
    torch_cuda.cuda.synchronize()
    for kind, n in SEQUENCE:
        calls.call(kind, n)
    calls.check("after the failure")
    enc.close()
