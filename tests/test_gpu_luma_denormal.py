"""GPU tests of the luma colour row of the tile kernels (-m gpu): csrc/m1v_kernels.hip luma_sums_denormal, the colour bytes of
waves 0 and 1 taken in place as fp32 denormals (tools/colour_fast_proof.c denormal proves the arithmetic on the host,
tests/test_luma_denormal_cpu.py runs it).

  against the oracle            frames 128x64, 144x80 and 176x208 at qualities 12 (byte staging) and 92 (wide staging): every luma
                                tie colour at every byte phase, bytes 0 and 255 only, and noise (tests/luma_denormal.py); bytes
                                and sizes equal; coefficients() at 128x64
  against the run kernel        one 4096x4096 frame holding every (r, g, b) once, encoded from a device buffer at four starts, 0-3
                                pixels in: every colour meets every byte phase.  The run kernel (debug_set_path("runs")) keeps
                                v_cvt_f32_ubyte and its unit-scale sums: the streams are byte-equal.  No oracle run.

Content and the oracle's records are built once per module."""
import numpy as np
import pytest

import luma_denormal as ld

pytestmark = pytest.mark.gpu

FIRST = 5
_records = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _want(orc, name, W, H, q):
    key = (name, W, H, q)
    if key not in _records:
        px = ld.content(name, W, H)
        _records[key] = [orc.encode_frame(px[f], W, H, FIRST + f, q, orc.MODE_FULL) for f in range(len(px))]
    return _records[key]


@pytest.mark.parametrize("q", ld.QUALITIES)
@pytest.mark.parametrize("name", ld.CONTENTS)
def test_encode_equals_the_oracle(torch_cuda, orc, name, q):
    from ec504_imageencoder_amd import Mpeg1Encoder
    for W, H in ld.SIZES:
        px = ld.content(name, W, H)
        enc = Mpeg1Encoder(W, H, q, "full", max_frames=len(px))
        assert enc.path == "tiles"
        got, sizes = enc.encode_to_bytes(torch_cuda.from_numpy(np.array(px)).cuda(), FIRST)
        enc.close()
        want = _want(orc, name, W, H, q)
        assert sizes == [len(r) for r in want], (name, W, H, q)
        assert got == b"".join(want), (name, W, H, q)


@pytest.mark.parametrize("q", ld.QUALITIES)
def test_coefficients_equal_the_oracle(torch_cuda, orc, q):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H = ld.SIZES[0]
    for name in ld.CONTENTS:
        px = ld.content(name, W, H)
        enc = Mpeg1Encoder(W, H, q, "full", max_frames=len(px))
        got = enc.coefficients(torch_cuda.from_numpy(np.array(px)).cuda()).cpu().numpy().astype(np.int32)
        enc.close()
        for f in range(len(px)):
            want = orc.frame_coefficients(px[f], W, H, q, orc.MODE_FULL)
            assert got[f].shape == want.shape and np.array_equal(got[f], want), (name, q, f)


@pytest.mark.parametrize("q", ld.QUALITIES)
def test_every_colour_at_every_byte_phase_equals_the_run_kernel(torch_cuda, q):
    torch = torch_cuda
    from ec504_imageencoder_amd import Mpeg1Encoder
    W = H = 4096
    # pixel i of the buffer has the colour i mod 2^24 = (r << 16) | (g << 8) | b; the frame that starts k pixels in holds every
    # colour once, colour c at pixel c - k (mod 2^24): byte phase 3 * (c - k) & 3
    c = torch.arange(W * H + 3, device="cuda", dtype=torch.int32)
    buf = torch.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], 1).to(torch.uint8).reshape(-1)
    tiles, runs = (Mpeg1Encoder(W, H, q, "full", max_frames=1) for _ in range(2))
    runs.debug_set_path("runs")
    assert tiles.path == "tiles" and runs.path == "runs"
    for k in range(4):
        frame = buf[3 * k:3 * k + W * H * 3].view(1, H, W, 3)
        got, sizes = tiles.encode_to_bytes(frame, FIRST)
        want, wsizes = runs.encode_to_bytes(frame, FIRST)
        assert sizes == wsizes and got == want, (q, k)
    tiles.close()
    runs.close()
