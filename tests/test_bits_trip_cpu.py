"""The integer arithmetic of the tile kernels' bits stage (csrc/m1v_tiles.h), restated in numpy and checked against the forms
it replaced — no GPU, no library:

  * tile_stage_byte8 / tile_stage_byte16: the LDS byte of the staged level at zigzag position p, written as bit moves, against
    the layout's own definition (stage_byte8 / stage_byte16, csrc/m1v_kernels.hip) for every p;
  * tile_walk_emit: the coded positions of an emit set and each one's run - 1, by shifting the set out, against the run
    kernels' walk (lowest set bit, emit &= emit - 1, run from the difference of positions), for both starts (DC level zero or
    not), on every one- and two-bit set and on 10,000 seeded random sets; the shift count stays below 64;
  * StagePack::mask_and_fence: the non-zero mask from the staging words — for the byte staging the flags of a word from
    per-byte (b + 255) >> 1, gathered by a chain of shifts and bit inserts — against the mask read off the levels, on random
    levels with every field's extremes.

tests/test_gpu_bits_trip.py runs the kernels themselves."""
import numpy as np
import pytest

M64 = (1 << 64) - 1


# ---- the layout (csrc/m1v_kernels.hip) and the kernel's form of its addresses (csrc/m1v_tiles.h) ----------------------------
def stage_byte8(p):
    return ((p & 7) + 8 * (p >> 5)) * 4 + ((p >> 3) & 3)


def stage_byte16(p):
    return ((p & 15) + 16 * (p >> 5)) * 4 + 2 * ((p >> 4) & 1)


def tile_stage_byte8(p):
    x = p & 31
    return (p & 32) | ((((x << 5) | x) >> 3) & 31)


def tile_stage_byte16(p):
    return ((p & 15) << 2) | ((p & 32) << 1) | ((p & 16) >> 3)


def test_byte_addresses_equal_the_layout():
    p = np.arange(64)
    assert np.array_equal(tile_stage_byte8(p), stage_byte8(p))
    assert np.array_equal(tile_stage_byte16(p), stage_byte16(p))
    # a block's levels take every byte (halfword) of its 16 (32) words once
    assert sorted(stage_byte8(p)) == list(range(64)) and sorted(stage_byte16(p)) == list(range(0, 128, 2))


# ---- the two walks ----------------------------------------------------------------------------------------------------------
def emit_set(nz):
    """csrc/m1v_kernels.hip: the non-zero AC positions below the first position whose predecessor is non-zero too."""
    stop = nz & (nz << 1) & M64
    below = ((stop & -stop) - 1) if stop else M64
    return nz & ~1 & below


def walk_before(dc_nonzero, emit):
    out, prev = [], 0 if dc_nonzero else -1
    while emit:
        p = (emit & -emit).bit_length() - 1
        emit &= emit - 1
        out.append((p, p - prev - 2))
        prev = p
    return out


def walk_shift_out(dc_nonzero, emit):
    out, rest, pos, lead = [], emit >> 1, 0, -1 if dc_nonzero else 0
    while rest:
        z = (rest & -rest).bit_length() - 1
        assert z + 1 < 64               # the hardware takes a 64-bit shift count modulo 64
        rest >>= z + 1
        pos += z + 1
        out.append((pos, z + lead))
        lead = -1
    return out


def _both_walks(nz_ac):
    """Both starts of one set of non-zero AC positions (bit 0 clear): the DC level's bit joins the mask that emit_set sees."""
    for dc_nonzero in (False, True):
        emit = emit_set(nz_ac | int(dc_nonzero))
        assert emit & 1 == 0
        got = walk_shift_out(dc_nonzero, emit)
        assert got == walk_before(dc_nonzero, emit), (hex(nz_ac), dc_nonzero)
        assert all(0 <= r < 63 for _, r in got), (hex(nz_ac), dc_nonzero)   # what the kernel tells the compiler about r
        yield got


def test_walk_on_every_one_and_two_bit_set():
    seen = set()
    for a in range(1, 64):
        for got in _both_walks(1 << a):
            seen.update(r for _, r in got)
        for b in range(a + 1, 64):
            for got in _both_walks((1 << a) | (1 << b)):
                seen.update(r for _, r in got)
    assert seen == set(range(63))       # every run - 1 from 0 to 62 (position 63 alone behind a zero DC level)


def test_walk_on_random_sets():
    rng = np.random.default_rng(29)
    codes = 0
    for k in range(10000):
        density = (0.02, 0.1, 0.3, 0.6)[k % 4]
        bits = rng.random(63) < density
        nz_ac = sum(1 << (i + 1) for i in np.flatnonzero(bits))
        for got in _both_walks(int(nz_ac)):
            codes += len(got)
    assert codes > 40000


def test_walk_of_the_raw_sets_too():
    """The walk does not rely on emit_set's shape beyond a clear bit 0: positions and runs agree on arbitrary sets (neighbours
    included: run - 1 = -1 there, which the reference never codes and emit_set never passes on)."""
    rng = np.random.default_rng(30)
    for _ in range(2000):
        emit = int(rng.integers(0, 1 << 63, dtype=np.uint64)) << 1 & M64
        for dc_nonzero in (False, True):
            assert walk_shift_out(dc_nonzero, emit) == walk_before(dc_nonzero, emit)


# ---- the non-zero mask from the staging words -------------------------------------------------------------------------------
def _lerp_u8(w):
    """v_lerp_u8(w, 0xffffffff, 0): per byte (b + 255) >> 1."""
    b = (w[..., None] >> (8 * np.arange(4, dtype=np.uint64))) & 0xFF
    return (((b + 255) >> 1) << (8 * np.arange(4, dtype=np.uint64))).sum(-1)


def _words(levels, narrow):
    """levels [n, 64] by zigzag position (position 0, the DC level's, is not staged: zero) -> staging words [n, 16 | 32]."""
    raw = np.zeros((levels.shape[0], 64 if narrow else 128), np.uint8)
    for p in range(1, 64):
        if narrow:
            raw[:, stage_byte8(p)] = levels[:, p].astype(np.int8).view(np.uint8)
        else:
            raw[:, stage_byte16(p):stage_byte16(p) + 2] = levels[:, p].astype("<i2").view(np.uint8).reshape(-1, 2)
    return raw.view("<u4").astype(np.uint64)


def _mask_narrow(w):
    """Words in order: the collected flags move down one bit per word, v_bfi_b32 takes bit 7 of every byte from the new word."""
    halves = []
    for h in range(2):
        acc = _lerp_u8(w[:, h * 8])
        for j in range(1, 8):
            acc = (_lerp_u8(w[:, h * 8 + j]) & np.uint64(0x80808080)) | ((acc >> np.uint64(1)) & np.uint64(0x7F7F7F7F))
        halves.append(acc)
    return halves[0] | (halves[1] << np.uint64(32))


def _mask_wide(w):
    """The int16 staging keeps the run kernels' form: ((w & 0x7fff7fff) + 0x7fff7fff) | w has bit 15 of a non-zero halfword set."""
    halves = []
    for h in range(2):
        acc = np.zeros(w.shape[0], np.uint64)
        for j in range(16):
            f = ((w[:, h * 16 + j] & np.uint64(0x7FFF7FFF)) + np.uint64(0x7FFF7FFF)) | w[:, h * 16 + j]
            acc |= (f >> np.uint64(15 - j)) & np.uint64(0x00010001 << j)
        halves.append(acc)
    return halves[0] | (halves[1] << np.uint64(32))


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_mask_from_the_staging_words(narrow):
    rng = np.random.default_rng(31)
    top = 127 if narrow else 32767          # (the byte staging is chosen only where no level can reach +-128)
    edge = np.array([0, 1, -1, 2, -2, top, -top, 64, -64] + ([] if narrow else [128, -128, 255, -255, 256, -256]))
    levels = np.where(rng.random((4000, 64)) < 0.5, 0, edge[rng.integers(0, len(edge), (4000, 64))])
    levels[0], levels[1], levels[2] = 0, 1, -1          # nothing, everything
    levels[3:3 + 63] = np.eye(64, dtype=np.int64)[1:] * -top            # every position alone
    want = ((levels[:, 1:] != 0).astype(np.uint64) << np.arange(1, 64, dtype=np.uint64)).sum(1)
    got = (_mask_narrow if narrow else _mask_wide)(_words(levels, narrow))
    assert np.array_equal(got, want)
