"""GPU tests of the tile kernels' bits stage (-m gpu): the non-zero mask from the staging words, the level fetch by one
sign-extending byte (halfword) read and the shift-out code walk of csrc/m1v_tiles.h (tests/test_bits_trip_cpu.py checks their
arithmetic on the host), through the packed tile kernel, one surface family (BGR, pitch W * 3 + 1), one plane family (NV12) and
the fused size table.  Bytes and sizes equal the CPU oracle's, every status word is 0.

  sizes      128x64 (one full tile), 144x80 (a last tile column of one strip, a last tile row of one macroblock row) and
             176x208 (the size of tests/test_gpu_hard_content.py)
  content    two frames per size: the heavy picture of tests/hard_content.py (blocks of more than 64 bits: pass 2 walks them
             again) and a picture of the blocks of tests/code_space.py's wide set, taken at even distances over its
             (run, level, sign) order — runs up to 61, levels up to +-255, 20- and 28-bit escapes; and one 704x400 frame of
             every colour whose Y, Cb or Cr lies on or next to an integer (where the fp32 colour sums hand over to the
             reference's fp64 expression), Cb and Cr ones behind a grey ramp in the quarter of the frame the chroma blocks read
             (r = g = b makes Cb = Cr = 128 exactly: every chroma pixel of the ramp takes that branch)
  qualities  12, 76, 77 (byte staging ends at 76) and 92, each as the quality of an encoder of its own; the size table at
             (12, 76) — the byte-staged kernel — and at (12, 76, 77, 92)

Content and the oracle's records are built once per module."""
import numpy as np
import pytest

import code_space as cs
import hard_content as hc
import input_families as fam
from gpu_calls import _encode, _table

pytestmark = pytest.mark.gpu

SIZES = [(128, 64), (144, 80), (176, 208)]
QUALITIES = [12, 76, 77, 92]
FAMILIES = ["rgb", "surface-3-bgr-odd", "planes-nv12"]
TIE_W, TIE_H = 704, 400
FIRST = 17
_cache = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _code_space_picture(orc, W, H):
    """Grey picture [H, W, 3]: the quality-92 blocks of the wide set at even distances over their (run, level, sign) order, one
    per 8x8 luma block of the picture.  Every block codes at 92 (code_space accepted it there) and so at every lower quality."""
    blocks = [e for e in cs.ac_blocks(orc, "wide", "grey") if e[0] == cs.TOP["wide"]]
    slots = (W // 8) * (H // 8)
    pick = np.linspace(0, len(blocks) - 1, slots).astype(int)
    Y = np.empty((H, W), np.uint8)
    for k, i in enumerate(pick):
        by, bx = divmod(k, W // 8)
        Y[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = np.asarray(blocks[i][3]).reshape(8, 8)
    assert {blocks[i][1] for i in pick} >= set(range(0, 62, 4)) and max(abs(blocks[i][2]) for i in pick) >= 250
    return np.repeat(Y[..., None], 3, 2)


def _tie_colours():
    """(chroma, luma): the colours [k, 3] whose Cb or Cr, and whose Y, lies within 2.6e-4 above or 2.5e-4 below an integer, in
    exact integer arithmetic (the formulas' coefficients are multiples of 1e-6).  The kernel flags a sum whose fraction is below
    10 / 32768 after adding 1.5e-4, with an error below 1e-4 (csrc/m1v_kernels.hip, component_t): a subset of these."""
    r, g, b = (x.reshape(-1).astype(np.int64) for x in np.meshgrid(*[np.arange(256)] * 3, indexing="ij"))
    def near(v):
        f = v % 1000000
        return (f < 260) | (f > 999750)
    rgb = np.stack([r, g, b], 1).astype(np.uint8)
    chroma = near(-168736 * r - 331264 * g + 500000 * b) | near(500000 * r - 418688 * g - 81312 * b)
    luma = near(299000 * r + 587000 * g + 114000 * b)
    return rgb[chroma], rgb[luma]


def _tie_picture():
    """[TIE_H, TIE_W, 3]: four rows of a grey ramp, the chroma tie colours up to the end of the frame's first quarter (the
    pixels the chroma blocks read, encoder.h:347-348), then the luma tie colours and all of them again in turn."""
    chroma, luma = _tie_colours()
    quarter, total = TIE_W * TIE_H // 4, TIE_W * TIE_H
    ramp = np.repeat(((np.arange(4 * TIE_W) * 3) % 256).astype(np.uint8)[:, None], 3, 1)
    assert len(ramp) + len(chroma) <= quarter and len(luma) <= total - quarter, (len(chroma), len(luma))
    top = np.concatenate([ramp, np.resize(chroma, (quarter - len(ramp), 3))])
    rest = np.concatenate([luma, np.resize(np.concatenate([chroma, luma]), (total - quarter - len(luma), 3))])
    return np.ascontiguousarray(np.concatenate([top, rest]).reshape(TIE_H, TIE_W, 3))


def _content(orc, W, H):
    """uint8 [n, H, W, 3], read-only: the two frames of a size, or the tie frame for (TIE_W, TIE_H)."""
    key = ("px", W, H)
    if key not in _cache:
        if (W, H) == (TIE_W, TIE_H):
            px = _tie_picture()[None]
        else:
            px = np.stack([hc.hard_frames(orc, W, H)[1], _code_space_picture(orc, W, H)])
        px.setflags(write=False)
        _cache[key] = px
    return _cache[key]


def _records(orc, W, H, q):
    key = ("rec", W, H, q)
    if key not in _cache:
        px = _content(orc, W, H)
        _cache[key] = [orc.encode_frame(px[f], W, H, FIRST + f, q, orc.MODE_FULL) for f in range(px.shape[0])]
    return _cache[key]


def _check_encode(torch, orc, family, W, H, q):
    px = _content(orc, W, H)
    case = fam.build(torch, family, W, H, "full", q, px.shape[0], pixels=px, orc=orc)
    recs = _records(orc, W, H, q)
    got, sizes = _encode(torch, case.enc, case.dev, FIRST)
    case.enc.close()
    assert sizes == [len(r) for r in recs], (family, W, H, q)
    assert got == b"".join(recs), (family, W, H, q)


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("family", FAMILIES)
def test_encode_equals_the_oracle(torch_cuda, orc, family, q):
    for W, H in SIZES:
        _check_encode(torch_cuda, orc, family, W, H, q)


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("family", FAMILIES)
def test_tie_colours_through_every_encode_family(torch_cuda, orc, family, q):
    _check_encode(torch_cuda, orc, family, TIE_W, TIE_H, q)


@pytest.mark.parametrize("quals", [(12, 76), (12, 76, 77, 92)], ids=["narrow", "wide"])
def test_size_table_equals_the_oracle(torch_cuda, orc, quals):
    for W, H in SIZES + [(TIE_W, TIE_H)]:
        px = _content(orc, W, H)
        case = fam.build(torch_cuda, "rgb", W, H, "full", 92, px.shape[0], pixels=px, orc=orc)
        got, status = _table(torch_cuda, case.enc, case.dev, quals)
        case.enc.close()
        assert status == [0] * len(quals), (W, H, status)
        assert got == [[len(r) for r in _records(orc, W, H, q)] for q in quals], (W, H)
