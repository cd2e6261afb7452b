"""GPU tests of the state an encoder carries from one m1v_encode_device call to the next (-m gpu).

Each internal Batch holds two counter sets (strip bits, frame bytes, status and arena words): a call adds into one, and its
k_assemble clears the other for the next call; the host clears what a shorter batch does not reach, and a failed call leaves
the Batch to be cleared by the next one.  Every call here is compared with the oracle on its own frames and first index:
bytes, per-frame sizes, total and status word.  Calls go through Mpeg1Encoder.encode (not encode_to_bytes, which retries
and would hide a status bit)."""
import numpy as np
import pytest

from gpu_calls import _unencodable

pytestmark = pytest.mark.gpu

M = 6  # max_frames of the small encoders

# producer of the segment table: how it is selected (W, H, channels, forced path)
PRODUCERS = {
    "tiles": (352, 288, 3, None),       # 3 channels: k_encode_tiles
    "runs": (352, 288, 3, "runs"),      # 108 blocks per strip: k_encode_dense + k_dense_frame_layout
    "strips": (352, 144, 4, None),      # 4 channels, 9 macroblock rows (54 blocks per strip): k_encode_strips
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(producer, qf=12, max_frames=M):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, C, path = PRODUCERS[producer]
    enc = Mpeg1Encoder(W, H, qf, "full", channels=C, max_frames=max_frames)
    if path:
        enc.debug_set_path(path)
    assert enc.path == ("tiles" if producer == "tiles" else "runs")
    return enc


def _frames(rng, enc, n, amp=256):
    """n frames of noise (amp 256) or of gentle noise around mid-grey (small amp: encodable at any quality factor)."""
    shape = (n, enc.height, enc.width, enc.channels)
    if amp >= 256:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (128 - amp // 2 + rng.integers(0, amp, shape)).astype(np.uint8)


class Calls:
    """Encodes batches on one encoder, keeps every call's input and outputs, and checks them against the oracle."""

    def __init__(self, torch, orc, enc, seed):
        self.torch, self.orc, self.enc = torch, orc, enc
        self.rng = np.random.default_rng(seed)
        self.pending = []
        self.first = int(self.rng.integers(0, 100))

    def encode(self, n, rgb=None, amp=256):
        torch, enc = self.torch, self.enc
        if rgb is None:
            rgb = _frames(self.rng, enc, n, amp)
        self.first += 37                                       # a different first index on every call (hour fields)
        dev = torch.from_numpy(rgb).cuda()
        out = torch.empty(enc.default_out_capacity(n), dtype=torch.uint8, device="cuda")
        res = enc.encode(dev, self.first, out=out)
        self.pending.append((rgb, self.first, dev, res))
        return res

    def check(self, what, status_bit=0):
        """Flushes, waits, and compares every call encoded since the last check (status_bit: every one of them must report
        that status bit instead; its bytes are not compared)."""
        self.enc.flush()
        self.torch.cuda.synchronize()
        enc, orc = self.enc, self.orc
        for k, (rgb, first, _, (out, sizes, meta)) in enumerate(self.pending):
            n = rgb.shape[0]
            total, status = (int(x) for x in meta.cpu())
            where = (what, k, n, first)
            if status_bit:
                assert status & status_bit, (where, "status", status)
                continue
            assert status & 0xFFFFFFFF == 0, (where, "status", status)
            if n == 0:
                assert total == 0, where
                continue
            want, wsizes = orc.encode_frames(rgb, n, enc.width, enc.height, first, enc.quality_factor, orc.MODE_FULL,
                                             channels=enc.channels, threads=8)
            assert [int(x) for x in sizes[:n].cpu()] == [int(x) for x in wsizes], (where, "sizes")
            assert total == len(want), (where, "total", total, len(want))
            assert out[:total].cpu().numpy().tobytes() == want, (where, "bytes")
        self.pending = []


# ---- a. batch-size sequences --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", sorted(PRODUCERS))
def test_batch_size_sequences(torch_cuda, orc, producer):
    """Long, short, long batches on the same counter sets.  A call's k_assemble clears the other set only for the frames it
    reaches; when the batch that last used that set was longer, the host clears the rest (hipMemsetAsync).  Non-pipelined
    (one Batch, the sets alternate call by call), pipelined (two Batches, calls alternate between them: each Batch sees
    long -> short -> long, once flushed only at the end and once synchronised after every call), then back to non-pipelined."""
    enc = _encoder(producer)
    calls = Calls(torch_cuda, orc, enc, seed=len(producer))
    for n in (M, 1, M, 2, M, 0, M):
        calls.encode(n)
        calls.check(("plain", n))
    enc.set_pipelined(True)
    seq = (M, M, 1, 2, M, M, 2, 1, M, M)
    for n in seq:
        calls.encode(n)
    calls.check("pipelined, one flush")
    for n in seq:
        calls.encode(n)
        calls.check(("pipelined, synchronised", n))
    enc.set_pipelined(False)
    for n in (2, M):
        calls.encode(n)
        calls.check(("plain again", n))
    enc.close()


# ---- b. a failed call leaves the encoder correct ------------------------------------------------------------------------
def _status_input(enc, producer, calls):
    """A batch whose encode kernel sets a status bit, and how to undo the setting that made it do so: a forced tiny LDS
    image (M1V_STATUS_SCRATCH: every unit overflows, the default arena is exhausted, the arena counter moves) on the tile
    and run kernels; the unencodable picture (M1V_STATUS_UNENCODABLE) on the strip kernel, whose encoder runs at quality 92."""
    if producer == "strips":
        return _unencodable(enc, M), lambda: None
    enc.debug_set_lds_words(8)
    return _frames(calls.rng, enc, M), lambda: enc.debug_set_lds_words(0)


@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("producer", sorted(PRODUCERS))
def test_failed_call_leaves_the_encoder_correct(torch_cuda, orc, producer, pipelined, stage):
    """m1v_debug_fail_encode(stage) makes the next encode return M1V_E_HIP after it took a counter set: before the encode
    kernel (1), after it (2: its counters and status words are written and never assembled or cleared), after k_assemble (3:
    in pipelined mode without the completion event).  The three batches after it equal the oracle with status 0.

    Every Batch has encoded before the failure, so the set the failed call's assembly would have cleared holds counters.  At
    stage 2 those batches and the failed one set a status bit (and, on the tile and run kernels, move the arena counter),
    so that stale status or arena words would show too: on the run kernels, whose layout kernel assigns the strip and frame
    counters instead of adding to them, they are the only words that can go stale."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    amp = 40 if (producer == "strips" and stage == 2) else 256
    enc = _encoder(producer, qf=92 if amp < 256 else 12)
    if pipelined:
        enc.set_pipelined(True)
    batches = 2 if pipelined else 1                       # one call on each Batch
    calls = Calls(torch_cuda, orc, enc, seed=100 * stage + 10 * pipelined + len(producer))
    for _ in range(batches):
        calls.encode(M, amp=amp)
    calls.check("good batch")
    rgb, undo = (_frames(calls.rng, enc, M, amp), lambda: None) if stage != 2 else _status_input(enc, producer, calls)
    if stage == 2:
        bit = _ffi.STATUS_UNENCODABLE if producer == "strips" else _ffi.STATUS_SCRATCH
        for _ in range(batches):
            calls.encode(M, rgb=rgb)
        calls.check("status batch", status_bit=bit)
    if producer == "strips" and stage == 2:
        with pytest.raises(ValueError):                   # the oracle refuses the same input
            orc.encode_frame(rgb[0], enc.width, enc.height, 0, 92, orc.MODE_FULL, channels=4)
    _ffi.lib().m1v_debug_fail_encode(stage)
    try:
        with pytest.raises(EncoderError) as ei:
            calls.encode(M, rgb=rgb)
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    if stage == 2:                                        # let the failed encode kernel finish before the hooks synchronise
        enc.flush()
        torch_cuda.cuda.synchronize()
    undo()
    for n in (M, 1, M):
        calls.encode(n, amp=amp)
    calls.check("after the failure")
    enc.close()


@pytest.mark.parametrize("producer", ["tiles", "runs", "strips"])
def test_oversized_lds_image_is_refused_when_set(torch_cuda, orc, producer):
    """A forced LDS image that cannot launch (41000 words: more than the 160 KiB of a workgroup) is refused by
    m1v_debug_set_lds_words itself (the budget the encode checks before each launch is checked when the image is set), and
    the encoder stays as it was: same path, same scratch, and the next batches equal the oracle."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    enc = _encoder(producer)
    calls = Calls(torch_cuda, orc, enc, seed=7)
    calls.encode(M)
    calls.check("before")
    path, scratch = enc.path, enc.scratch_bytes()
    with pytest.raises(EncoderError) as ei:
        enc.debug_set_lds_words(41000)
    assert ei.value.code == _ffi.E_ARG
    assert enc.path == path and enc.scratch_bytes() == scratch
    for n in (M, 2):
        calls.encode(n)
    calls.check("after")
    enc.close()


def test_failed_step_of_host_delivery(torch_cuda, orc):
    """HostDelivery: a step whose encode fails (stage 2) raises and delivers nothing; the batch queued before it and the
    two batches after it are delivered as the oracle's streams, with their frame sizes."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    enc = _encoder("tiles")
    W, H = enc.width, enc.height
    rng = np.random.default_rng(11)
    batches = [(_frames(rng, enc, M), 50 * k + 3) for k in range(4)]
    hd = HostDelivery(enc, M)
    got = []

    def take():
        hd.delivered[hd.last[0]].synchronize()
        got.append((bytes(hd.result().numpy()), [int(x) for x in hd.frame_sizes(M)]))

    devs = [torch.from_numpy(b).cuda() for b, _ in batches]
    hd.step(devs[0], batches[0][1])
    assert hd.last is None
    _ffi.lib().m1v_debug_fail_encode(2)
    try:
        with pytest.raises(EncoderError) as ei:
            hd.step(devs[1], batches[1][1])
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    hd.step(devs[2], batches[2][1])                       # batch 0 starts travelling
    take()
    hd.step(devs[3], batches[3][1])                       # batch 2
    take()
    hd.fence()                                            # batch 3
    take()
    for (blob, sizes), k in zip(got, (0, 2, 3)):
        want, wsizes = orc.encode_frames(batches[k][0], M, W, H, batches[k][1], 12, orc.MODE_FULL, threads=8)
        assert sizes == [int(x) for x in wsizes], k
        assert blob == want, k
    hd.close()
    enc.close()


# ---- c. the 64-bit scratch variant of k_assemble, at full size ----------------------------------------------------------
@pytest.mark.parametrize("path", ["tiles", "runs"])
def test_scratch_past_4_gib_at_full_size(torch_cuda, orc, path):
    """300 x 3840x2160 at quality 12 with every unit in the overflow arena, reserved for the worst case: the scratch is
    4 GiB or more, so k_assemble<true> (64-bit source addresses) assembles the batch, and its bytes past 2^32 are read.

    Why slots past 4 GiB are really used (configure_path): a forced 8-word LDS image gives a compact slot of 128 bytes, and
    every unit outgrows it, so every unit takes one arena slot.  Tiles: 30 x 34 tiles per frame (240 strips / 8, 135
    macroblock rows / 4, rounded up) = 1020, 306,000 in the batch; the compact slots take 306,000 x 128 B = 39.2 MB, then the
    arena holds one worst-case slot of 21,424 B per tile (192 blocks x 888 bits + 8 slice headers, rounded): 6.59 GB in all.
    Slot k starts at 39.2 MB + k x 21,424 B, which is past 2^32 for k >= 198,646: the last ~107 k slots.  Runs (256 blocks
    each): 760 per frame, 228,000 in the batch, a worst-case slot of 28,480 B: 6.52 GB, and the last ~78 k slots lie past
    2^32.  The arena hands out exactly as many slots as there are units, so all of them are taken.

    Then the same through HostDelivery: its own SCRATCH retry reserves the worst case and lands on the wide kernel."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n = 3840, 2160, 300

    def make():
        enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
        if path == "runs":
            enc.debug_set_path("runs")
        assert enc.path == path
        return enc

    enc = make()
    rgb = enc.synth(n, seed=504)
    out, sizes, meta = enc.encode(rgb, 0)
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status == 0 and enc.scratch_bytes() < 2 ** 32
    blob = out[:total].cpu()
    want_sizes = sizes[:n].cpu()
    del out, sizes, meta
    enc.close()

    enc = make()
    enc.debug_set_lds_words(8)
    out, sizes, meta = enc.encode(rgb, 0)
    torch.cuda.synchronize()
    assert int(meta.cpu()[1]) & _ffi.STATUS_SCRATCH
    enc.reserve_scratch(True)
    assert enc.scratch_bytes() >= 2 ** 32, enc.scratch_bytes()
    assert enc.path == path
    out, sizes, meta = enc.encode(rgb, 0, out=out, sizes=sizes, meta=meta)
    torch.cuda.synchronize()
    total2, status2 = (int(x) for x in meta.cpu())
    assert status2 == 0 and total2 == total
    assert torch.equal(sizes[:n].cpu(), want_sizes)
    assert torch.equal(out[:total].cpu(), blob)
    del out, sizes, meta
    enc.close()
    offs = np.concatenate([[0], np.cumsum(want_sizes.numpy().astype(np.int64))])
    for f in (0, 150, 255, 299):
        want = orc.encode_frame(rgb[f].cpu().numpy(), W, H, f, 12, orc.MODE_FULL)
        assert blob[int(offs[f]):int(offs[f + 1])].numpy().tobytes() == want, f

    enc = make()
    enc.debug_set_lds_words(8)
    hd = HostDelivery(enc, n, capacity=int(1.25 * total))   # (the default pins 2 x 3.7 GB of host memory)
    hd.step(rgb, 0)
    hd.fence()
    assert enc.scratch_bytes() >= 2 ** 32, enc.scratch_bytes()
    assert torch.equal(hd.result(), blob)
    assert torch.equal(torch.from_numpy(hd.frame_sizes(n).astype(np.int64)), want_sizes)
    hd.close()
    enc.close()
    del rgb
    torch.cuda.empty_cache()
