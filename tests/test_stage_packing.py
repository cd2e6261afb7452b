"""The tile kernel families build the staging words of a block in registers (csrc/m1v_tiles.h, StagePack: every level's
conversion writes one byte, or halfword, of a word) and store whole words.  Host side: the staging layout is a bijection and
fetch_level's index arithmetic inverts it, and the order in which StagePack fills and stores the words is consistent.  GPU
side (-m gpu): content that stresses the packing — ±1 levels in every byte position, sign bytes beside non-zero
neighbours, words that are zero but for one byte — through every kernel family that shares the helper, at both staging
widths and either side of the switch between them (qualities 12, 76 | 77, 100), byte for byte against the CPU oracle.

Shapes: 16x16 (one block row, one partial tile) and 136x72 (a second tile column of one strip, a partial last tile row),
batches of 1 and 3 frames.  A picture the oracle calls unencodable at a quality (a level outside the code table) must be
reported as such by the GPU (STATUS_UNENCODABLE) instead of compared."""
import os
import re

import numpy as np
import pytest

import hard_content as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (12, 76, 77, 100)   # narrow, the largest narrow, the smallest wide, the largest
SHAPES = [(16, 16), (136, 72)]
FIRST = 17
UNENCODABLE = 1


# ---- host: the layout ---------------------------------------------------------------------------------------------------------
def _constexpr_int(src, name):
    """A one-line `constexpr int name(int p) { return <expr>; }` of the kernel source as a Python function."""
    m = re.search(r"constexpr int %s\(int p\) \{ return (.*?); \}" % name, src)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[p0-9\s()+*&>]*", expr), expr      # integer arithmetic on p only
    return lambda p: eval(expr, {"p": p})


def _scan_pos(src):
    m = re.search(r"constexpr int scan_pos\(int k\) \{\s*constexpr int t\[64\] = \{(.*?)\};", src, re.S)
    t = [int(x) for x in m.group(1).replace("\n", " ").split(",")]
    assert sorted(t) == list(range(64))
    return t


def test_stage_layout_is_a_bijection_and_fetch_level_inverts_it():
    src = open(os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_kernels.hip")).read()
    b8, b16 = _constexpr_int(src, "stage_byte8"), _constexpr_int(src, "stage_byte16")
    # narrow: 64 positions onto the 64 bytes of 16 words; wide: onto the 64 halfwords of 32 words
    assert sorted(b8(p) for p in range(64)) == list(range(64))
    assert sorted(b16(p) for p in range(64)) == list(range(0, 128, 2))
    # fetch_level reads word (p & 7) + 8 (p >> 5), byte (p >> 3) & 3 | word (p & 15) + 16 (p >> 5), halfword (p >> 4) & 1
    assert "blk[(p & 7) + 8 * (p >> 5)]" in src and "(w << (24 - 8 * ((p >> 3) & 3))) >> 24" in src
    assert "blk[(p & 15) + 16 * (p >> 5)]" in src and "(p & 16) ? ((int)w >> 16)" in src
    for p in range(64):
        assert b8(p) == 4 * ((p & 7) + 8 * (p >> 5)) + ((p >> 3) & 3)
        assert b16(p) == 4 * ((p & 15) + 16 * (p >> 5)) + 2 * ((p >> 4) & 1)
    # the mask puts the flag of byte k of word j (bit 8 k + 7, shifted right by 7 - j, word j of a half) on position p
    for p in range(1, 64):
        word, byte = divmod(b8(p), 4)
        assert (8 * byte + 7) - (7 - (word & 7)) + 32 * (word >> 3) == p
        word, half = divmod(b16(p) // 2, 2)
        assert (16 * half + 15) - (15 - (word & 15)) + 32 * (word >> 4) == p


def test_stage_pack_plan_fills_every_word_before_it_is_stored():
    """StagePack takes the levels in the order of the column pass (n = 8 i + u), clears a word with its first level and
    stores words in pairs as their last level arrives: replay that plan."""
    src = open(os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_kernels.hip")).read()
    t = _scan_pos(src)
    for byte_of, parts in ((_constexpr_int(src, "stage_byte8"), 4), (_constexpr_int(src, "stage_byte16"), 2)):
        n_words = 64 // parts
        pos = lambda n: t[(n & 7) * 8 + (n >> 3)]
        word = lambda n: byte_of(pos(n)) // 4
        assert pos(0) == 0                                   # level 0 is the DC level: kept in a register, not staged
        filled = {w: 0 for w in range(n_words)}
        for n in range(1, 64):
            filled[word(n)] += 1
        assert filled[0] == parts - 1 and all(filled[w] == parts for w in range(1, n_words))
        done = {w: max(n for n in range(1, 64) if word(n) == w) >> 3 for w in range(n_words)}
        held, stored = None, []
        for col in range(8):
            for w in range(n_words):
                if done[w] != col:
                    continue
                if held is None:
                    held = w
                else:
                    stored += [held, w]
                    held = None
        assert held is None and sorted(stored) == list(range(n_words))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _grey(a):
    return np.repeat(a[..., None], 3, axis=-1).astype(np.uint8)


_pictures = {}


def _content(W, H):
    """[10, H, W, 3]: noise; gentle noise (levels of +-1 everywhere); a 0/255 checkerboard; vertical and horizontal stripes of
    period 2 and 16 (levels down to -70 at quality 76); mid-grey with one bright or dark pixel per block, at a position that
    moves from block to block; the extreme-pattern picture of tests/hard_content.py (the largest levels a byte holds: 115 at
    quality 76, and past a byte from 77 on)."""
    if (W, H) not in _pictures:
        rng = np.random.default_rng(W * 1000 + H)
        y, x = np.mgrid[0:H, 0:W]
        pics = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
                (118 + rng.integers(0, 20, (H, W, 3))).astype(np.uint8),
                _grey(((x + y) & 1) * 255),
                _grey((x & 1) * 255), _grey(((x >> 3) & 1) * 255),
                _grey((y & 1) * 255), _grey(((y >> 3) & 1) * 255)]
        dot = np.full((H, W), 128, dtype=np.uint8)
        for by in range(H // 8):
            for bx in range(W // 8):
                k = (by * (W // 8) + bx) * 5
                dot[by * 8 + (k >> 3) % 8, bx * 8 + k % 8] = 255 if (bx + by) & 1 else 0
        pics += [_grey(dot), _grey(255 - dot), hc.extreme_pattern_picture(rng, W, H)]
        _pictures[(W, H)] = np.ascontiguousarray(np.stack(pics))
    return _pictures[(W, H)]


_records = {}


def _record(orc, W, H, c, q, index):
    """The oracle's record of content picture c at quality q as frame `index`, or None where it is unencodable."""
    key = (W, H, c, q, index)
    if key not in _records:
        try:
            _records[key] = orc.encode_frame(_content(W, H)[c], W, H, index, q, orc.MODE_FULL)
        except ValueError:
            _records[key] = None
    return _records[key]


def _encodable(orc, W, H, q):
    return [c for c in range(len(_content(W, H))) if _record(orc, W, H, c, q, FIRST) is not None]


def _run(torch, enc, dev):
    """One encode -> (bytes, sizes, status bits)."""
    n = dev.shape[0]
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    out, sizes, meta = enc.encode(dev, FIRST, out=out)
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(v) for v in meta.cpu())
    return out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()], status & 0xFFFFFFFF


def _check_batches(torch, orc, W, H, q, n, make):
    """Through encoder + input built by make(pictures) -> (enc, dev): the pictures the oracle encodes at q in batches of n
    (the last one filled up from the first pictures) equal its records; every other picture, n times in a batch, sets
    STATUS_UNENCODABLE.  Returns how many batches were compared."""
    px = _content(W, H)
    good = _encodable(orc, W, H, q)
    compared = 0
    for at in range(0, len(good), n):
        batch = [good[(at + k) % len(good)] for k in range(n)]
        enc, dev = make(px[batch])
        got, sizes, status = _run(torch, enc, dev)
        recs = [_record(orc, W, H, c, q, FIRST + f) for f, c in enumerate(batch)]
        assert status == 0, (q, batch, status)
        assert sizes == [len(r) for r in recs], (q, batch)
        assert got == b"".join(recs), (q, batch)
        compared += 1
        enc.close()
    for c in sorted(set(range(len(px))) - set(good)):
        enc, dev = make(px[[c] * n])
        assert _run(torch, enc, dev)[2] & UNENCODABLE, (q, c)
        enc.close()
    return compared


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_packed_rgb_encode(torch_cuda, orc, W, H, q, n):
    torch = torch_cuda
    from ec504_imageencoder_amd import Mpeg1Encoder

    def make(px):
        enc = Mpeg1Encoder(W, H, q, "full", max_frames=n)
        assert enc.path == "tiles"
        return enc, torch.from_numpy(px).cuda()

    assert _check_batches(torch, orc, W, H, q, n, make) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_pitched_bgra_surface_encode(torch_cuda, orc, q):
    torch = torch_cuda
    from layout_inputs import _surface, _surface_encoder
    W, H, n = 136, 72, 3
    rng = np.random.default_rng(q)

    def make(px):
        rgba = np.concatenate([px, rng.integers(0, 256, px.shape[:3] + (1,), dtype=np.uint8)], -1)
        dev, pitch, stride = _surface(torch, rgba, "gap", "bgr", fill_seed=q)
        return _surface_encoder(W, H, q, "full", 4, n, pitch, stride, "bgr"), dev

    assert _check_batches(torch, orc, W, H, q, n, make) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_nv12_plane_encode(torch_cuda, orc, q):
    torch = torch_cuda
    from layout_inputs import _plane_encoder, _planes_of, _view
    W, H, n = 136, 72, 3

    def make(px):
        buf, lay, base = _planes_of(torch, orc, px, "full", "nv12", fill_seed=q)
        enc = _plane_encoder(W, H, q, "full", n, lay)
        return enc, _view(torch, buf, n, lay, base, enc)

    assert _check_batches(torch, orc, W, H, q, n, make) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_coefficients(torch_cuda, orc, q):
    torch = torch_cuda
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H = 136, 72
    px = _content(W, H)
    enc = Mpeg1Encoder(W, H, q, "full", max_frames=len(px))
    assert enc.path == "tiles"
    got = enc.coefficients(torch.from_numpy(px).cuda()).cpu().numpy().astype(np.int32)
    for f in range(len(px)):
        want = orc.frame_coefficients(px[f], W, H, q, orc.MODE_FULL)
        assert got[f].shape == want.shape and np.array_equal(got[f], want), (q, f)
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quals", [(12, 76, 77), (12, 50, 76)])
def test_size_table_either_side_of_the_switch(torch_cuda, orc, quals):
    """(12, 76, 77) is served by the wide size-table kernel, (12, 50, 76) by the narrow one: the oracle's sizes of every
    picture that it encodes at all three qualities."""
    torch = torch_cuda
    from ec504_imageencoder_amd import Mpeg1Encoder
    from gpu_calls import _table
    W, H = 136, 72
    px = _content(W, H)
    enc = Mpeg1Encoder(W, H, 100, "full", max_frames=len(px))
    assert enc.path == "tiles" and enc.size_table_fused == 1
    good = [c for c in range(len(px)) if all(_record(orc, W, H, c, q, FIRST) is not None for q in quals)]
    assert len(good) >= 5, good
    table, status = _table(torch, enc, torch.from_numpy(px[good]).cuda(), quals)
    assert status == [0] * len(quals), status
    assert table == [[len(_record(orc, W, H, c, q, FIRST)) for c in good] for q in quals]
    enc.close()
