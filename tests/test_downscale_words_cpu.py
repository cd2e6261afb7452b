"""CPU checks of the downscale word layout's model and inputs (tests/downscale_words.py) and of its Python side (the extent
Mpeg1Encoder._check_input asks for), without a device: the model against a per-sample loop and its rounding, shift and clamp; the
identity on replicated sources in every form and placement; that the placement writes the addressed bytes and nothing else; the
record oracle on the model's frame against the oracle proper where a picture exists; and a census that the noise inputs of the GPU
arithmetic test are sensitive — every plausible mistake of a kernel changes a record on every size used there."""
import numpy as np
import pytest

import downscale_words as dw
import plane_oracle

# the sizes and modes of tests/test_gpu_downscale_words.py's arithmetic test
CASES = ((16, 16, "full"), (48, 32, "full"), (144, 80, "full"), (40, 32, "full"))
# the quality of that test: on noise of the full range the coarser qualities clip most levels, and a sample that moves by one
# seldom moves a code; at 50 every mistake below shows within the nine frames of a size
QUALITIES = (50,)
# every (c_step, shift) pair of the presets
CENSUS = ("p010", "i010", "i012", "i016")


def _loop(frame, lay, W, H):
    word = lambda at: int(frame[at]) | int(frame[at + 1]) << 8
    out = []
    for (h, w), off, pitch, step in (((H, W), lay["y_offset"], lay["y_pitch"], 2), ((H // 2, W // 2), lay["cb_offset"], lay["c_pitch"], lay["c_step"]),
                                     ((H // 2, W // 2), lay["cr_offset"], lay["c_pitch"], lay["c_step"])):
        for y in range(h):
            for x in range(w):
                at = off + 2 * y * pitch + 2 * x * step
                a = (word(at) + word(at + step) + word(at + pitch) + word(at + pitch + step) + 2) >> 2
                out.append(min(a >> lay["shift"], 255))
    return np.array(out, dtype=np.uint8)


@pytest.mark.parametrize("where", (dw.TIGHT, dw.PITCHED, dict(cr_first=True, cpad=3)), ids=("tight", "pitched", "cr-first"))
@pytest.mark.parametrize("preset", dw.PRESETS)
def test_model_against_a_per_sample_loop(preset, where):
    W, H, n = 8, 4, 2
    src = dw.noise_source(3, n, H, W, preset, over=True)
    host, lay, at, span = dw.host_buffer(src, preset, fill_seed=1, **where)
    want = dw.down2_words(src, dw.SHIFT[preset])
    assert want.shape == (n, W * H * 3 // 2) and want.dtype == np.uint8
    for f in range(n):
        frame = host[at + f * lay["frame_stride"]:]
        assert np.array_equal(dw.down2_frame(frame, lay, W, H), want[f])
        assert np.array_equal(_loop(frame, lay, W, H), want[f])


def test_rounding_shift_and_clamp():
    """All four remainders of the sum mod 4 occur on noise; a remainder of 2 (the tie) goes up, 1 down, 3 up, at the word's
    precision; the shift truncates (it never rounds); the clamp holds words above the stated depth at 255; 4 * 65535 + 2 needs 18
    bits and gives 65535."""
    src = dw.noise_source(1, 1, 16, 16, "p016")
    for plane in src:
        s = plane.astype(np.int64)
        sums = s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]
        assert set(np.unique(sums % 4).tolist()) == {0, 1, 2, 3}
        a = np.where(sums % 4 >= 2, sums // 4 + 1, sums // 4)
        for shift in range(9):
            assert np.array_equal(dw.box(plane, shift).astype(np.int64), np.minimum(a >> shift, 255)), shift
    assert (4 * 65535 + 2) >> 2 == 65535 and (4 * 65535 + 2).bit_length() == 18
    value = lambda cell, shift: int(dw.box(np.array(cell, dtype=np.uint16).reshape(2, 2), shift)[0, 0])
    assert value((0xffff,) * 4, 8) == 255 and value((0,) * 4, 8) == 0
    assert value((0x00ff, 0x00ff, 0x00ff, 0x0101), 8) == 1            # sum 1022, + 2 = 1024: the carry of the average reaches the sample
    assert value((0x00ff, 0x00ff, 0x00ff, 0x0100), 8) == 0            # a = 255: the shift truncates what rounding would lift
    assert value((0x01ff,) * 4, 8) == 1                                # 1.996 stays 1: truncation at the shift
    assert value((3, 3, 3, 2), 2) == 0 and value((3, 3, 3, 3), 2) == 0 and value((4, 4, 3, 3), 2) == 1   # a = 3, 3, 4
    assert value((1023,) * 4, 2) == 255 and value((1024,) * 4, 2) == 255 and value((0xffff,) * 4, 2) == 255    # the clamp
    assert value((4095,) * 4, 4) == 255 and value((4096,) * 4, 4) == 255 and value((4080, 4079, 4079, 4079), 4) == 254
    assert value((0xffff,) * 4, 0) == 255 and value((254, 255, 255, 255), 0) == 255 and value((254, 254, 254, 255), 0) == 254


@pytest.mark.parametrize("preset", dw.PRESETS)
def test_replicated_sources_give_the_planes_back(preset):
    from ec504_imageencoder_amd import downscale_word_layout_preset
    rng = np.random.default_rng(5)
    W, H, n = 16, 8, 2
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, H, W), (n, H // 2, W // 2), (n, H // 2, W // 2)))
    want = np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], 1)
    shift = dw.SHIFT[preset]
    src = dw.replicated_planes(y, cb, cr, shift, seed=1)
    assert [p.shape for p in src] == [(n, 2 * H, 2 * W), (n, H, W), (n, H, W)] and all(p.dtype == np.uint16 for p in src)
    assert any((p & ((1 << shift) - 1)).any() for p in src)                 # the bits below the shift are not zero
    assert np.array_equal(dw.down2_words(src, shift), want)
    # the packed frames are the tight preset's ...
    tight = downscale_word_layout_preset(W, H, preset)
    packed = dw.replicated_source(y, cb, cr, preset, seed=1)
    assert packed.shape == (n, 6 * W * H) and packed.dtype == np.uint16 and tight["frame_stride"] == 12 * W * H
    assert dw.geometry(W, H, preset)[0] == tight
    for f in range(n):
        assert np.array_equal(dw.down2_frame(packed[f].view(np.uint8), tight, W, H), want[f])
    # ... and what the placements hold, tight and pitched
    for where in (dw.TIGHT, dw.PITCHED):
        host, lay, at, span = dw.host_buffer(src, preset, fill_seed=2, **where)
        for f in range(n):
            assert np.array_equal(dw.down2_frame(host[at + f * lay["frame_stride"]:], lay, W, H), want[f])
        if not where:
            assert np.array_equal(host[at:at + n * 12 * W * H].view(np.uint16).reshape(n, -1), packed)


@pytest.mark.parametrize("preset", dw.PRESETS)
def test_host_buffer_places_the_source_and_nothing_else(preset):
    W, H, n = 8, 4, 2
    src = dw.noise_source(2, n, H, W, preset)
    for where in (dw.TIGHT, dw.PITCHED, dict(cr_first=True, cpad=1)):
        a, lay, at, span = dw.host_buffer(src, preset, fill_seed=1, **where)
        b, _, _, _ = dw.host_buffer(src, preset, fill_seed=2, **where)
        assert len(a) == at + n * lay["frame_stride"] + dw.GUARD and at >= dw.GUARD and span <= lay["frame_stride"]
        same = dw.addressed(lay, n, W, H, at, len(a))
        assert same.sum() == n * 12 * W * H                    # no two words share a byte
        assert np.array_equal(a[same], b[same])
        if (~same).sum() > 200:
            assert (a[~same] != b[~same]).mean() > 0.9          # everything else is the fill's noise
    lay, span, at = dw.geometry(W, H, preset, **dw.PITCHED)
    assert at == dw.GUARD + 1 and lay["y_pitch"] % 4 and lay["c_pitch"] % 4 and lay["frame_stride"] == span + 5
    assert lay["y_pitch"] == 2 * (6 + 2 * W + 2) + 13 and lay["y_offset"] == 2 * lay["y_pitch"] + 12
    # one chroma plane named by both offsets: every other word of it belongs to nobody
    shared = (src[0], src[1], src[1])
    a, lay, at, _ = dw.host_buffer(shared, preset, fill_seed=1, shared=True, cpad=5, base=3)
    assert lay["c_step"] == 4 and lay["cb_offset"] == lay["cr_offset"]
    assert dw.addressed(lay, n, W, H, at, len(a)).sum() == n * (8 + 2) * W * H
    assert np.array_equal(dw.down2_frame(a[at:], lay, W, H), dw.down2_words(shared, dw.SHIFT[preset])[0])


# ---- the record oracle on the model's frame -----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,mode,qf,preset", [(48, 32, "full", 12, "p010"), (48, 32, "full", 50, "i010"), (112, 160, "strict", 12, "i012")])
def test_the_record_oracle_on_the_models_frame_equals_the_oracle_on_a_converted_picture(orc, W, H, mode, qf, preset):
    """A picture exists for every rendition whose chroma planes are the head of a converted picture's: the reference addresses
    its full-resolution Cb / Cr plane with stride W / 2, so what it codes as chroma is the first (W / 2) * (H / 2) bytes of each
    plane read as an H / 2 x W / 2 plane.  The word source that repeats the picture's luma plane and those two 2 x 2, as
    `byte << shift` with noise below, has them as its rendition, and plane_oracle.encode_layout on the model's I420 frame is
    orc.encode_frame on the picture (as tests/test_planes_abi.py pins the two oracles to each other on reference-style planes)."""
    from ec504_imageencoder_amd import plane_layout_preset
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    rng = np.random.default_rng(W * 1000 + H + qf)
    yy, xx = np.mgrid[0:H, 0:W]                    # gradient + noise: encodable at these qualities, every block different
    base = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * 2 + yy * 5) % 256], axis=-1)
    rgb = ((base + rng.integers(0, 48, (H, W, 3))) % 256).astype(np.uint8)
    Y, Cb, Cr = (np.asarray(p, dtype=np.uint8).reshape(-1) for p in orc.convert(rgb))
    quarter = (W // 2) * (H // 2)
    y, cb, cr = Y.reshape(1, H, W), Cb[:quarter].reshape(1, H // 2, W // 2), Cr[:quarter].reshape(1, H // 2, W // 2)
    assert len(np.unique(cb)) > 20 and len(np.unique(cr)) > 20
    frame = dw.down2_words(dw.replicated_planes(y, cb, cr, dw.SHIFT[preset]), dw.SHIFT[preset])[0]
    assert np.array_equal(frame, np.concatenate([Y, Cb[:quarter], Cr[:quarter]]))
    got = plane_oracle.encode_layout(frame, plane_layout_preset(W, H, "i420"), W, H, 7, qf, m)
    assert got == orc.encode_frame(rgb, W, H, 7, qf, m)


# ---- the census: the noise inputs are sensitive ---------------------------------------------------------------------------------
def _records(orc, frames, W, H, mode, q):
    from ec504_imageencoder_amd import plane_layout_preset
    lay = plane_layout_preset(W, H, "i420")
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    return [plane_oracle.encode_layout(frames[f], lay, W, H, f, q, m) for f in range(frames.shape[0])]


def _frames_of(planes):
    n = planes[0].shape[0]
    return np.concatenate([p.reshape(n, -1) for p in planes], 1)


def _mutants(src, shift, xe, ye):
    """{name: the I420 frames a kernel with that mistake would code}; xe x ye: the coded region in rendition samples."""
    Y, Cb, Cr = (p.astype(np.uint32) for p in src)
    quad = lambda s: (s[:, 0::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 0::2], s[:, 1::2, 1::2])
    u8 = lambda a: np.minimum(a, 255).astype(np.uint8)
    good = [dw.box(p, shift) for p in src]
    each = lambda f: _frames_of([f(s) for s in (Y, Cb, Cr)])
    out = {}
    out["a truncating average"] = each(lambda s: u8((sum(quad(s)) >> 2) >> shift))
    out["the average of the shifted bytes"] = each(lambda s: u8((sum(np.minimum(q >> shift, 255) for q in quad(s)) + 2) >> 2))
    out["the low byte alone"] = each(lambda s: u8((sum(q & 0xff for q in quad(s)) + 2) >> 2))
    out["the high byte alone"] = each(lambda s: u8((sum(q >> 8 for q in quad(s)) + 2) >> 2))
    out["shift + 1"] = each(lambda s: u8(((sum(quad(s)) + 2) >> 2) >> (shift + 1)))
    out["shift - 1"] = each(lambda s: u8(((sum(quad(s)) + 2) >> 2) >> (shift - 1)))
    out["the top-left word"] = each(lambda s: u8(quad(s)[0] >> shift))
    out["Cb and Cr exchanged"] = _frames_of([good[0], good[2], good[1]])
    # the other halfword phase of an interleaved pair: the first component's lanes get the second's words, the second's get the
    # first's one word further
    ahead = np.roll(src[1], -1, axis=2)
    out["the phases of a pair exchanged"] = _frames_of([good[0], good[2], dw.box(ahead, shift)])

    def repeated(s, axis, last):
        t = s.copy()
        if axis == 1:
            t[:, last] = s[:, last - 1]
        else:
            t[:, :, last] = s[:, :, last - 1]
        return t

    out["the last source row of the region repeated"] = _frames_of(
        [dw.box(repeated(src[0], 1, 2 * ye - 1), shift), dw.box(repeated(src[1], 1, ye - 1), shift), dw.box(repeated(src[2], 1, ye - 1), shift)])
    out["the last source column of the region repeated"] = _frames_of(
        [dw.box(repeated(src[0], 2, 2 * xe - 1), shift), dw.box(repeated(src[1], 2, xe - 1), shift), dw.box(repeated(src[2], 2, xe - 1), shift)])

    def skip_a_row(s):                 # rows 2y and 2y + 2 (the last cell: 2y and 2y + 1, there is no row behind it)
        below = np.concatenate([s[:, 2::2], s[:, -1:]], 1)
        return u8(((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + below[:, :, 0::2] + below[:, :, 1::2] + 2) >> 2) >> shift)

    out["rows 2y and 2y + 2"] = each(skip_a_row)
    # ... per plane, so that a mistake in one plane's path alone shows too
    for i, name in enumerate(("luma", "Cb", "Cr")):
        planes = list(good)
        planes[i] = u8((sum(quad((Y, Cb, Cr)[i])) >> 2) >> shift)
        out[f"a truncating average in {name} alone"] = _frames_of(planes)
    return out


@pytest.mark.parametrize("preset", CENSUS)
@pytest.mark.parametrize("W,H,mode", CASES)
def test_census_every_mutant_changes_a_record_on_every_size(orc, W, H, mode, preset):
    xe, ye = orc.region(orc.MODE_FULL if mode == "full" else orc.MODE_STRICT, W, H)
    shift = dw.SHIFT[preset]
    src = dw.noise_for(W, H, preset)                                # the GPU test's nine frames
    good = dw.down2_words(src, shift)
    mutants = _mutants(src, shift, xe, ye)
    assert len(mutants) == 15
    for q in QUALITIES:
        want = _records(orc, good, W, H, mode, q)
        for name, frames in mutants.items():
            assert frames.shape == good.shape
            got = _records(orc, frames, W, H, mode, q)
            assert any(g != w for g, w in zip(got, want)), (name, W, H, mode, q)


@pytest.mark.parametrize("preset", ("i010", "i012"))
@pytest.mark.parametrize("W,H,mode", CASES)
def test_census_a_missing_clamp_changes_a_record(orc, W, H, mode, preset):
    """On the GPU extremes test's source with words just above the stated depth, and on noise in every bit, a kernel without the
    min(.., 255) codes other samples (the low byte of a >> shift, what a conversion to a byte keeps) and another record."""
    shift = dw.SHIFT[preset]
    for src in (dw.noise_source(W + H, 2, H, W, preset, over=True), dw.above_depth_source(preset, 2, H, W)):
        good = dw.down2_words(src, shift)
        wide = [p.astype(np.uint32) for p in src]
        unclamped = _frames_of([((((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2) >> shift) & 0xff).astype(np.uint8)
                                for s in wide])
        assert (good == 255).any() and (unclamped != good).any()
        assert any(g != w for g, w in zip(_records(orc, unclamped, W, H, mode, 12), _records(orc, good, W, H, mode, 12)))


# ---- the extent Mpeg1Encoder._check_input holds a tensor's rows against -------------------------------------------------------------
def test_the_source_extent_of_the_coded_region():
    """downscale_word_layout_extent against the last addressed byte of the coded region's words, counted from the model's own
    addressing, for xe < W and ye < H, in every form and placement.  (The refusals of _check_input itself are held on a real
    encoder by tests/test_gpu_downscale_words.py.)"""
    from ec504_imageencoder_amd import downscale_word_layout_preset
    from ec504_imageencoder_amd.encoder import downscale_word_layout_extent
    W, H, strips, mb_rows = 40, 24, 2, 1                    # xe = 32 < W, ye = 16 < H
    for preset in dw.PRESETS:
        for where in (dw.TIGHT, dw.PITCHED, dict(cr_first=True)):
            lay = dw.geometry(W, H, preset, **where)[0]
            if not where:
                assert lay == downscale_word_layout_preset(W, H, preset)
            last = int(np.flatnonzero(dw.addressed(lay, 1, 16 * strips, 16 * mb_rows, 0, lay["frame_stride"]))[-1])
            assert downscale_word_layout_extent(lay, strips, mb_rows) == last + 1, (preset, where)
    lay = downscale_word_layout_preset(W, H, "p010")
    E = downscale_word_layout_extent(lay, strips, mb_rows)
    assert E == 8 * W * H + 2 + (16 - 1) * 4 * W + (32 - 1) * 4 + 2 and E < 12 * W * H


def test_the_python_preset_and_its_errors():
    from ec504_imageencoder_amd import downscale_word_layout_preset
    from ec504_imageencoder_amd.encoder import DOWNSCALE_WORD_LAYOUT_FIELDS
    W, H = 48, 32
    assert downscale_word_layout_preset(W, H, "p010") == downscale_word_layout_preset(W, H, "p012") == downscale_word_layout_preset(W, H, "p016") == \
        dict(y_offset=0, cb_offset=8 * W * H, cr_offset=8 * W * H + 2, y_pitch=4 * W, c_pitch=4 * W, c_step=4, frame_stride=12 * W * H, factor=2, shift=8)
    for name, shift in (("i010", 2), ("i012", 4), ("i016", 8)):
        got = downscale_word_layout_preset(W, H, name)
        assert tuple(got) == DOWNSCALE_WORD_LAYOUT_FIELDS
        assert got == dict(y_offset=0, cb_offset=8 * W * H, cr_offset=10 * W * H, y_pitch=4 * W, c_pitch=2 * W, c_step=2, frame_stride=12 * W * H,
                           factor=2, shift=shift)
    for args in ((48, 16, "nv12"), (48, 16, "p210"), (47, 16, "p010"), (48, 15, "i010"), (0, 16, "i010"), (48, 16, "p010", 4)):
        with pytest.raises(ValueError):
            downscale_word_layout_preset(*args)
