"""GPU tests of the downscale word layout (m1v_set_downscale_word_layout; k_half_words_encode, k_half_words_size_table,
k_half_words_rd_table, k_half_words_to_i420; -m gpu): [n, L] frames of 2W x 2H 4:2:0 planes of 16-bit little-endian words (P010 /
P012 / P016, yuv420p10le / 12le / 16le) whose 2 x 2 box average per plane, taken on the words and shifted down to a byte, is
encoded at W x H, where they lie.

The definition (include/mpeg1_hip.h, "Downscale word layout") is checked for equality on the samples themselves
(downscale_words_to_i420) against tests/downscale_words.py's model; every expected record is tests/plane_oracle.py's on the
model's I420 frame under plane_layout_preset(W, H, "i420"), and the rate calls are held against the same calls on those bytes
through the I420 plane layout.  A source is written into a device buffer of noise (downscale_words.place); every batch lies 64
bytes inside its allocation, so nothing here can fault.  Every comparison is for equality and every status word is 0."""
import ctypes as C

import numpy as np
import pytest

import downscale_words as dw
import plane_oracle
import rd_oracle as rd
from gpu_calls import _encode, _rd, _table

pytestmark = pytest.mark.gpu

# rendition size, mode: one macroblock (the smallest extent of the overhang limit); 3 strips in the last tile column; a 2 x 2 tile
# grid with a partial last column and row; a width that is no multiple of 16 (xe = 32 < W)
CASES = ((16, 16, "full"), (48, 32, "full"), (144, 80, "full"), (40, 32, "full"))
BATCHES = (1, 9)
K8 = (1, 2, 3, 5, 7, 9, 11, 12)
CANDS = (2, 5, 8, 10, 12)
FIRST = 17


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(W, H, Q, n, lay, mode="full"):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, mode, max_frames=n)
    enc.set_downscale_word_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1
    assert isinstance(lay, str) or enc.downscale_word_layout == lay
    return enc


def _i420_of(torch, enc, x):
    out = enc.downscale_words_to_i420(x)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_record_cache = {}


def _oracle(orc, frames, W, H, mode, first, qs, key=None):
    """plane_oracle's (records back to back, sizes) of the I420 frames [n, W * H * 3 / 2] at one quality per frame (or one for
    all); cached per frame under `key` where several tests share it (the key names the source)."""
    from ec504_imageencoder_amd import plane_layout_preset
    lay = plane_layout_preset(W, H, "i420")
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    qs = [qs] * frames.shape[0] if isinstance(qs, int) else list(qs)
    recs = []
    for f in range(frames.shape[0]):
        k = (key, W, H, mode, f, first + f, qs[f])
        if key is None or k not in _record_cache:
            rec = plane_oracle.encode_layout(frames[f], lay, W, H, first + f, qs[f], m)
            if key is None:
                recs.append(rec)
                continue
            _record_cache[k] = rec
        recs.append(_record_cache[k])
    return b"".join(recs), [len(r) for r in recs]


def _sizes(torch, enc, x, q):
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    s = enc.frame_sizes(x, quality=[q] * x.shape[0], status=st)
    enc.flush()
    torch.cuda.synchronize()
    return [int(v) for v in s.cpu()], int(st.cpu()[0])


# ---- 1. the averaging ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", dw.PRESETS)
@pytest.mark.parametrize("W,H,mode", CASES)
def test_arithmetic_on_noise(torch_cuda, orc, W, H, mode, preset):
    """Noise sources under each of the six names (both chroma forms), tight by name and as a pitched window (Cr in front of Cb
    there), batches of 1 and 9 frames: the samples are the model's; records, sizes, total and status of the encode, frame_sizes,
    the size table and the rd table are the oracle's on them.  (tests/test_downscale_words_cpu.py holds that the nine frames
    of each of these sources tell every plausible mistake apart at this quality.)"""
    torch = torch_cuda
    Q, N = 50, max(BATCHES)                    # (the census's quality)
    src = dw.noise_for(W, H, preset, N)
    want_frames = dw.down2_words(src, dw.SHIFT[preset])
    for k, where in enumerate((dw.TIGHT, dict(dw.PITCHED, cr_first=True))):
        x, lay, _ = dw.place(torch, src, preset, fill_seed=k, **where)
        enc = _encoder(W, H, Q, N, lay if where else preset)
        assert enc.downscale_word_layout == lay
        for n in BATCHES:
            what = f"{W}x{H} {mode} {preset} {where} n{n}"
            want = _oracle(orc, want_frames[:n], W, H, mode, FIRST, Q, key=("noise", preset))
            got = _i420_of(torch, enc, x[:n])
            assert got.shape == (n, W * H * 3 // 2) and got.dtype == np.uint8
            wrong = np.argwhere(got != want_frames[:n])
            assert not len(wrong), (what, len(wrong), [(tuple(w), int(got[tuple(w)]), int(want_frames[tuple(w)])) for w in wrong[:8]])
            blob, sizes = _encode(torch, enc, x[:n], FIRST)
            assert sizes == want[1], (what, [f for f in range(n) if sizes[f] != want[1][f]])
            at = np.concatenate([[0], np.cumsum(want[1])])
            assert not [f for f in range(n) if blob[at[f]:at[f + 1]] != want[0][at[f]:at[f + 1]]] and len(blob) == at[n], what
            assert _sizes(torch, enc, x[:n], Q) == (want[1], 0), what
            assert _table(torch, enc, x[:n], (Q,)) == ([want[1]], [0]), what
            assert _rd(torch, enc, x[:n], (Q,))[0] == [want[1]], what
        enc.close()


def test_arithmetic_at_every_shift(torch_cuda, orc):
    """The shift is a run-time value of both chroma forms: 0 .. 8 on one source of noise in every bit."""
    torch = torch_cuda
    W, H, n = 48, 32, 2
    for preset in ("p016", "i016"):
        src = dw.noise_source(77, n, H, W, preset, over=True)
        x, lay, _ = dw.place(torch, src, preset, fill_seed=5, **dw.PITCHED)
        enc = _encoder(W, H, 12, n, lay)
        for shift in range(9):
            enc.set_downscale_word_layout(dict(lay, shift=shift))
            assert enc.downscale_word_layout["shift"] == shift
            frames = dw.down2_words(src, shift)
            assert np.array_equal(_i420_of(torch, enc, x), frames), (preset, shift)
            assert _encode(torch, enc, x, 0) == _oracle(orc, frames, W, H, "full", 0, 12), (preset, shift)
        enc.close()


@pytest.mark.parametrize("preset", ("p010", "i010", "i012", "i016"))
def test_extremes(torch_cuda, orc, preset):
    """One frame each, at the preset's shift: all-zero words; all-0xffff words (4 * 65535 + 2 needs 18 bits; 255 at shift 8, the
    clamp below it); a checkerboard of 0 and 0xffff words, in both phases (every cell sums to 2 * 65535: a = 32768 rounds half up
    from 32767.5); the last word below the next sample at the top of the depth and the first words above the depth (the clamp at
    shift 2 and 4); cells whose sum leaves each remainder mod 4 just below a sample boundary.  Luma, Cb and Cr of a frame lie on
    three different contents, so that every content passes through every plane's path and an exchange of Cb and Cr shows."""
    torch = torch_cuda
    W, H = 48, 32
    shift = dw.SHIFT[preset]
    top = 256 << shift if shift < 8 else 0x10000                    # the first word above the depth (none at shift 8)
    unit = 1 << shift
    cells = [(0, 0, 0, 0), (0xffff,) * 4, (0, 0xffff, 0xffff, 0), (0xffff, 0, 0, 0xffff), (0xffff, 0xffff, 0, 0),
             (top - 1,) * 4, (top - unit, top - unit - 1, top - unit - 1, top - unit - 1), (top - unit, top - unit, top - unit - 1, top - unit - 1),
             (min(top, 0xffff),) * 4, (min(top + 1, 0xffff), top - 1, top - 1, top - 1), (min(top + unit, 0xffff),) * 4,
             (5 * unit, 5 * unit, 5 * unit - 1, 5 * unit - 1), (5 * unit, 5 * unit, 5 * unit, 5 * unit - 1),
             (5 * unit, 5 * unit - 1, 5 * unit - 1, 5 * unit - 1), (5 * unit - 1,) * 4]
    n = len(cells)
    parts = [dw.cell_source(cells[f], cells[(f + 4) % n], cells[(f + 9) % n], 1, H, W) for f in range(n)]
    src = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    frames = dw.down2_words(src, shift)
    value = lambda cell: min(((sum(cell) + 2) >> 2) >> shift, 255)
    assert [(int(frames[f, 0]), int(frames[f, W * H]), int(frames[f, W * H + W * H // 4])) for f in range(n)] == \
        [(value(cells[f]), value(cells[(f + 4) % n]), value(cells[(f + 9) % n])) for f in range(n)]
    assert [value(c) for c in cells[:5]] == [0, 255, 255 if shift < 8 else 128, 255 if shift < 8 else 128, 255 if shift < 8 else 128]
    assert [value(c) for c in cells[5:8]] == [255, 254, 255] and [value(c) for c in cells[11:]] == [5, 5, 4, 4]
    want = _oracle(orc, frames, W, H, "full", 0, 12)
    for where in (dw.TIGHT, dw.PITCHED):
        x, lay, _ = dw.place(torch, src, preset, fill_seed=3, **where)
        enc = _encoder(W, H, 12, n, lay)
        got = _i420_of(torch, enc, x)
        assert np.array_equal(got, frames), [cells[f] for f in range(n) if not np.array_equal(got[f], frames[f])]
        assert _encode(torch, enc, x, 0) == want
        assert _table(torch, enc, x, (12,)) == ([want[1]], [0])
        enc.close()


# ---- 2. the read contract -----------------------------------------------------------------------------------------------------------
# one macroblock (the smallest extent), 3 strips in the last tile column (48 and 176 wide) and xe < W (40 wide); tight P010, where
# the last chroma unit of the second component would end two bytes behind the frame, and tight I010; pitched windows of both forms;
# and a c_step = 4 plane that is not interleaved with another (one plane named by both offsets, every other word nobody's)
CONTRACT = [(W, preset, where) for W in (16, 48, 176, 40)
            for preset, where in (("p010", dw.TIGHT), ("i010", dw.TIGHT), ("p016", dw.PITCHED), ("i012", dict(dw.PITCHED, cr_first=True)),
                                  ("p010", dict(cr_first=True, cpad=6, base=2)), ("i016", dict(shared=True, cpad=5, base=3)))]


@pytest.mark.parametrize("W,preset,where", CONTRACT, ids=[f"{W}-{p}-{'tight' if not w else 'shared' if 'shared' in w else 'pitched' if 'window' in w else 'crfirst'}"
                                                          for W, p, w in CONTRACT])
def test_read_contract(torch_cuda, orc, W, preset, where):
    """The same sources under two fills of every byte the definition does not address — row padding, the gaps between planes and
    frames, the surface around the window, the guards (which lie right behind the last chroma row of the last tightly packed
    frame), the other words of a c_step = 4 plane that is not interleaved: identical samples, records and tables, the oracle's;
    and the buffer, guards included, is what was uploaded.  Nothing lies against the end of an allocation."""
    torch = torch_cuda
    H, n = 16 if W == 16 else 32, 3
    src = dw.noise_for(W, H, preset, n)
    if where.get("shared"):
        src = (src[0], src[1], src[1])
    frames = dw.down2_words(src, dw.SHIFT[preset])
    want = _oracle(orc, frames, W, H, "full", 0, 12)
    seen = []
    for fill in (1, 2):
        x, lay, buf = dw.place(torch, src, preset, fill_seed=fill, **where)
        before = buf.cpu().numpy()
        seen.append(before)
        enc = _encoder(W, H, 12, n, lay)
        assert enc.strips * 16 == W - W % 16
        assert np.array_equal(_i420_of(torch, enc, x), frames), fill
        assert _encode(torch, enc, x, 0) == want, fill
        assert _table(torch, enc, x, (12,)) == ([want[1]], [0]), fill
        assert _rd(torch, enc, x, (12,))[0] == [want[1]], fill
        assert np.array_equal(buf.cpu().numpy(), before)                   # the source and its guards are untouched
        enc.close()
    # the two allocations differ everywhere but in the addressed bytes (tests/test_downscale_words_cpu.py pins the placement)
    lay, _, at = dw.geometry(W, H, preset, **where)
    same = dw.addressed(lay, n, W, H, at, len(seen[0]))
    assert np.array_equal(seen[0][same], seen[1][same])
    assert (seen[0][~same] != seen[1][~same]).mean() > 0.9 and (~same).sum() >= 2 * dw.GUARD


# ---- 3. the setter ------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_layout_in_force(torch_cuda, orc):
    """Every M1V_E_ARG case of m1v_set_downscale_word_layout, each with its reason; none changes the layout in force, the table
    mode or the records."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi, downscale_word_layout_preset
    from ec504_imageencoder_amd.encoder import downscale_word_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    S = _ffi.DownscaleWordLayout
    W, H, n = 48, 32, 3
    src = dw.noise_for(W, H, "p010", n)
    want = _oracle(orc, dw.down2_words(src, 8), W, H, "full", 0, 12)
    x, good, _ = dw.place(torch, src, "p010", **dw.PITCHED)
    tight = downscale_word_layout_preset(W, H, "p010")
    planar = downscale_word_layout_preset(W, H, "i010")
    assert good["c_step"] == 4 and good["factor"] == 2 and good["shift"] == 8
    enc = _encoder(W, H, 12, n, good)
    big = 2 ** 40
    E = downscale_word_layout_extent(good, enc.strips, enc.mb_rows)
    assert E == good["cr_offset"] + (H - 1) * good["c_pitch"] + (W - 1) * 4 + 2 and E <= good["frame_stride"]
    chroma = (H - 1) * 4 * W + (W - 1) * 4 + 2                             # a tight interleaved plane's bytes from its offset
    bad = [(dict(good, factor=4), b"factor"), (dict(good, factor=0), b"factor"), (dict(good, factor=1), b"factor"),
           (dict(good, shift=9), b"shift"), (dict(good, shift=-1), b"shift"), (dict(good, shift=16), b"shift"),
           (dict(good, c_step=1), b"c_step"), (dict(good, c_step=3), b"c_step"), (dict(good, c_step=8), b"c_step"),
           (dict(good, cr_offset=good["cb_offset"] + 4), b"4-byte group"), (dict(good, cb_offset=good["cr_offset"] + 4), b"4-byte group"),
           (dict(planar, c_step=4, c_pitch=4 * W, frame_stride=big), b"4-byte group"),          # two planes of their own, each with step 4
           (dict(good, frame_stride=0), b"frame stride"),
           (dict(good, y_pitch=4 * W - 1), b"luma pitch below"), (dict(good, y_pitch=2 * W), b"luma pitch below"),   # a byte source's row
           (dict(good, y_pitch=1), b"luma pitch below"),
           (dict(good, c_pitch=4 * W - 1), b"chroma pitch below"), (dict(good, c_pitch=2 * W), b"chroma pitch below"),
           (dict(planar, c_pitch=2 * W - 1), b"chroma pitch below"),
           (dict(tight, y_pitch=(2 ** 32 - 4 * W) // (2 * H - 1) + 1, frame_stride=big), b"4 GiB"),
           (dict(tight, y_pitch=2 ** 32, frame_stride=big), b"4 GiB"), (dict(tight, c_pitch=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(tight, cb_offset=2 ** 32, cr_offset=2 ** 32 + 2, frame_stride=big), b"4 GiB"), (dict(tight, y_offset=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(tight, cb_offset=2 ** 32 - chroma - 2, cr_offset=2 ** 32 - chroma, frame_stride=big), b"4 GiB"),
           (dict(good, frame_stride=E - 1), b"frame stride below"),
           (dict(good, frame_stride=good["y_offset"] + (2 * H - 1) * good["y_pitch"] + 4 * W), b"frame stride below")]  # the luma plane alone
    for lay, reason in bad:
        assert L.m1v_set_downscale_word_layout(enc._h, C.byref(S(**lay))) == _ffi.E_ARG, lay
        assert L.m1v_last_error() and reason in L.m1v_last_error(), (lay, L.m1v_last_error())
        assert enc.downscale_word_layout == good and enc.path == "tiles" and not enc.frame_table and not enc.plane_table
        with pytest.raises(EncoderError):
            enc.set_downscale_word_layout(lay)
    assert _encode(torch, enc, x, 0) == want
    # the largest extent whose offsets are still 32-bit and the smallest stride are accepted (set, not encoded); zeros default
    edge = dict(tight, cb_offset=2 ** 32 - 1 - chroma - 2, cr_offset=2 ** 32 - 1 - chroma, frame_stride=big)
    assert L.m1v_set_downscale_word_layout(enc._h, C.byref(S(**edge))) == 0 and enc.downscale_word_layout == edge
    assert L.m1v_set_downscale_word_layout(enc._h, C.byref(S(**dict(good, frame_stride=E)))) == 0
    assert enc.downscale_word_layout == dict(good, frame_stride=E)
    assert L.m1v_set_downscale_word_layout(enc._h, C.byref(S(**dict(planar, y_pitch=0, c_pitch=0, c_step=0)))) == 0
    assert enc.downscale_word_layout == planar                                                       # the getter fills in: no zeros
    enc.set_downscale_word_layout(dict(tight, c_pitch=0, y_pitch=0))
    assert enc.downscale_word_layout == tight
    for d in (0, 1, 2, 3):                                                                            # inside one 4-byte group: taken
        enc.set_downscale_word_layout(dict(good, cr_offset=good["cb_offset"] + d))
    enc.set_downscale_word_layout(good)
    # a table that another layout turned on is turned off by this setter, and a failed call leaves it on
    enc.set_rgb_plane_layout("rgb")
    enc.set_plane_table(True)
    assert L.m1v_set_downscale_word_layout(enc._h, C.byref(S(**dict(good, factor=3)))) == _ffi.E_ARG
    assert enc.plane_table and enc.rgb_plane_layout is not None and enc.downscale_word_layout is None
    enc.set_downscale_word_layout(good)
    assert not enc.plane_table and not enc.frame_table and _encode(torch, enc, x, 0) == want
    enc.close()
    for size in ((105, 48), (104, 49)):                                                                 # an odd width, an odd height
        odd = Mpeg1Encoder(*size, 12, "full", max_frames=n)
        lay = S(**dict(tight, y_pitch=0, c_pitch=0, frame_stride=big))
        assert L.m1v_set_downscale_word_layout(odd._h, C.byref(lay)) == _ffi.E_ARG and b"even width and height" in L.m1v_last_error()
        assert odd.downscale_word_layout is None and odd.input_layout == (0, 0, "rgb")
        odd.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)                                     # channels != 3
    assert L.m1v_set_downscale_word_layout(rgba._h, C.byref(S(**good))) == _ffi.E_ARG
    assert b"3 channels" in L.m1v_last_error() and rgba.downscale_word_layout is None and rgba.path == "runs"
    rgba.close()
    assert L.m1v_set_downscale_word_layout(None, C.byref(S(**good))) == _ffi.E_ARG                      # a null encoder
    assert L.m1v_last_error()
    forced = Mpeg1Encoder(W, H, 12, "full", max_frames=n)                                               # the run-kernel hooks
    forced.debug_set_path("runs")
    assert L.m1v_set_downscale_word_layout(forced._h, C.byref(S(**good))) == _ffi.E_ARG
    assert b"hook" in L.m1v_last_error() and forced.downscale_word_layout is None and forced.path == "runs"
    forced.debug_set_path("auto")
    forced.set_downscale_word_layout(good)
    for hook in (lambda: forced.debug_set_path("runs"), lambda: forced.debug_set_input_mode(0)):
        with pytest.raises(EncoderError) as ei:
            hook()
        assert ei.value.code == _ffi.E_ARG and "downscale word layout" in str(ei.value)
        assert forced.path == "tiles" and forced.downscale_word_layout == good
    assert _encode(torch, forced, x, 0) == want
    forced.close()


def test_setters_getters_tables_and_packed_only_calls(torch_cuda, orc):
    from ec504_imageencoder_amd import (EncoderError, Mpeg1Encoder, _ffi, downscale_layout_preset, downscale_plane_layout_preset,
                                        float_pixel_layout_preset)
    from ec504_imageencoder_amd.encoder import downscale_word_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 96, 80, 3
    src = dw.noise_for(W, H, "i012", n)
    frames = dw.down2_words(src, 4)
    want = _oracle(orc, frames, W, H, "full", 5, 12)
    x, lay, _ = dw.place(torch, src, "i012", **dict(dw.PITCHED, cr_first=True))
    i420 = torch.from_numpy(frames).cuda()
    packed = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    fresh = (enc.path, enc.size_table_fused, enc.scratch_bytes())
    assert enc.downscale_word_layout is None and L.m1v_downscale_word_layout_in_force(enc._h, None) == 0
    # for the 8-bit sibling: the NV12 source that repeats the rendition's samples 2 x 2, whose records are the same
    hi = tuple(np.ascontiguousarray(np.repeat(np.repeat(p, 2, -2), 2, -1)) for p in
               (frames[:, :W * H].reshape(n, H, W), frames[:, W * H:W * H * 5 // 4].reshape(n, H // 2, W // 2), frames[:, W * H * 5 // 4:].reshape(n, H // 2, W // 2)))
    nv12 = torch.from_numpy(np.concatenate([hi[0].reshape(n, -1), np.stack([hi[1], hi[2]], -1).reshape(n, -1)], 1)).cuda()
    others = ((lambda: enc.set_plane_layout("i420"), i420), (lambda: enc.set_rgb_plane_layout("rgb"), None),
              (lambda: enc.set_input_layout(W * 3, 0, "bgr"), None), (lambda: enc.set_sample_layout("yuy2"), None),
              (lambda: enc.set_sample_layout("p010"), None),
              (lambda: enc.set_downscale_layout(downscale_layout_preset(W, H, 4)), None),
              (lambda: enc.set_downscale_plane_layout(downscale_plane_layout_preset(W, H, "nv12")), nv12),
              (lambda: enc.set_float_plane_layout(dict(r_offset=0, g_offset=2 * W * H, b_offset=4 * W * H, row_pitch=2 * W,
                                                       frame_stride=6 * W * H, sample=_ffi.SAMPLE_F16, range=_ffi.RANGE_UNIT)), None),
              (lambda: enc.set_float_pixel_layout(float_pixel_layout_preset(W, H, 4, "float16", "bgr")), None),
              (lambda: enc.set_downscale_word_layout(None), None))
    for set_other, tensor in others:
        enc.set_downscale_word_layout(lay)                                  # ... -> downscale words
        assert enc.downscale_word_layout == lay and enc.downscale_layout is None and enc.rgb_plane_layout is None
        assert enc.float_plane_layout is None and enc.float_pixel_layout is None and enc.downscale_plane_layout is None
        assert L.m1v_downscale_word_layout_in_force(enc._h, None) == 1
        assert _encode(torch, enc, x, 5) == want
        for query in (lambda: enc.plane_layout, lambda: enc.sample_layout, lambda: enc.input_layout):
            with pytest.raises(EncoderError) as ei:
                query()
            assert ei.value.code == _ffi.E_ARG and "ask m1v_downscale_word_layout_in_force" in str(ei.value)
        set_other()                                                         # downscale words -> each other layout
        assert enc.downscale_word_layout is None and L.m1v_downscale_word_layout_in_force(enc._h, None) == 0
        if tensor is not None:
            assert _encode(torch, enc, tensor, 5) == want
    enc.set_downscale_word_layout(lay)
    # the table modes refuse this kind, with a reason of their own, and stay off
    for setter in ("m1v_set_frame_table", "m1v_set_plane_table"):
        assert getattr(L, setter)(enc._h, 1) == _ffi.E_ARG
        assert b"downscale word layout" in L.m1v_last_error() and b"not covered" in L.m1v_last_error()
        assert getattr(L, setter)(enc._h, 0) == _ffi.OK
    assert not enc.frame_table and not enc.plane_table
    with pytest.raises(AssertionError, match="downscale word layout"):
        enc.frames([x[0]])
    with pytest.raises(AssertionError, match="downscale word layout"):
        enc.plane_frames([(x[0], x[0], x[0])])
    # packed-only entry points refuse, naming the layout
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(packed.cpu().numpy())):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG and "downscale word layout" in str(ei.value)
    # Python holds the tensor against the layout: another dtype, a row below the extent and another frame stride are refused
    E = downscale_word_layout_extent(lay, enc.strips, enc.mb_rows)
    wider = torch.zeros((n, lay["frame_stride"] + 8), dtype=torch.uint8, device="cuda")
    assert _encode(torch, enc, x[:, :E], 5) == want
    for wrong in (x.float(), x.to(torch.int8), x.to(torch.int32), x[:, :E - 1], wider[:, :x.shape[1]], packed, i420, x[0]):
        with pytest.raises(AssertionError):
            enc.encode(wrong)
    enc.set_downscale_word_layout(None)                                     # downscale words -> default: a fresh encoder's plan
    assert enc.downscale_word_layout is None and enc.input_layout == (0, 0, "rgb")
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes()) == fresh
    out = torch.empty((n, W * H * 3 // 2), dtype=torch.uint8, device="cuda")    # the to-i420 call needs the layout
    assert L.m1v_downscale_words_to_i420_device(enc._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == _ffi.E_ARG
    assert b"m1v_set_downscale_word_layout" in L.m1v_last_error()
    enc.close()


def test_python_takes_names_and_tensors_of_words_or_bytes(torch_cuda, orc):
    """Each of the six names on a decoder's tightly packed frames, as uint8 bytes, as int16 words and, where this torch has it,
    as uint16 words: the same records; a row of words is held by its byte extent and its byte stride."""
    from ec504_imageencoder_amd import Mpeg1Encoder, downscale_word_layout_preset
    from ec504_imageencoder_amd.encoder import downscale_word_layout_extent
    torch = torch_cuda
    W, H, n = 48, 32, 2
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    for preset in dw.PRESETS:
        src = dw.noise_for(W, H, preset, n)
        want = _oracle(orc, dw.down2_words(src, dw.SHIFT[preset]), W, H, "full", 0, 12)
        words = dw.pack(src, preset)                                        # [n, 6 W H] uint16
        enc.set_downscale_word_layout(preset)
        assert enc.downscale_word_layout == downscale_word_layout_preset(W, H, preset)
        forms = [torch.from_numpy(words.view(np.uint8)).cuda(), torch.from_numpy(words.view(np.int16)).cuda()]
        if hasattr(torch, "uint16"):
            forms.append(forms[1].view(torch.uint16))
        assert [tuple(t.shape) for t in forms[:2]] == [(n, 12 * W * H), (n, 6 * W * H)]
        for t in forms:
            assert _encode(torch, enc, t, 0) == want, (preset, t.dtype)
            assert _encode(torch, enc, t[:1], 0) == (want[0][:want[1][0]], want[1][:1])
            assert np.array_equal(_i420_of(torch, enc, t), dw.down2_words(src, dw.SHIFT[preset]))
        E = downscale_word_layout_extent(enc.downscale_word_layout, enc.strips, enc.mb_rows)
        assert E == 12 * W * H
        for t in forms[1:]:                                                 # a row of words one word short; rows another stride apart
            with pytest.raises(AssertionError):
                enc.encode(t[:, :E // 2 - 1])
            with pytest.raises(AssertionError):
                enc.encode(torch.zeros((n, E // 2 + 1), dtype=t.dtype, device="cuda")[:, :E // 2])
    for name in ("nv12", "p210", "reference"):
        with pytest.raises(ValueError):
            enc.set_downscale_word_layout(name)
    enc.close()


# ---- 4. every served call once ------------------------------------------------------------------------------------------------------
def _pair(torch, preset, n):
    """(the encoder with the layout in force, its source view, an encoder under the I420 plane layout, the to-i420 bytes, the
    model's frames, the layout) at 48 x 32."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H = 48, 32
    src = dw.noise_for(W, H, preset, n)
    xa, lay, _ = dw.place(torch, src, preset, fill_seed=4, **dw.PITCHED)
    a = _encoder(W, H, 12, n, lay)
    xb = a.downscale_words_to_i420(xa)
    torch.cuda.synchronize()
    frames = dw.down2_words(src, dw.SHIFT[preset])
    assert np.array_equal(xb.cpu().numpy(), frames)
    b = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    b.set_plane_layout("i420")
    return a, xa, b, xb, frames, lay


@pytest.mark.parametrize("preset", ("i010", "p010"))
def test_tables_against_the_oracles(torch_cuda, orc, preset):
    """The size table and the rd table at K = 8 on 5 frames: the oracle's sizes, tests/rd_oracle.py's distortion, the K probes'
    sizes, and the I420 plane layout's tables on the bytes."""
    from ec504_imageencoder_amd import plane_layout_preset
    torch = torch_cuda
    n, W, H = 5, 48, 32
    a, xa, b, xb, frames, _ = _pair(torch, preset, n)
    sizes = [_oracle(orc, frames, W, H, "full", 0, q)[1] for q in K8]
    tight = plane_layout_preset(W, H, "i420")
    dist = [[rd.plane_frame_distortion(orc, frames[f], tight, W, H, q, orc.MODE_FULL) for f in range(n)] for q in K8]
    assert _table(torch, a, xa, K8) == (sizes, [0] * 8) == _table(torch, b, xb, K8)
    assert _rd(torch, a, xa, K8) == (sizes, dist, [0] * 8) == _rd(torch, b, xb, K8)
    for k, q in enumerate(K8):                              # K probes
        assert _sizes(torch, a, xa, q) == (sizes[k], 0), q
    qs = [K8[(2 * f + 3) % 8] for f in range(n)]           # per-frame quality and frame_sizes
    want = [_oracle(orc, frames[f:f + 1], W, H, "full", FIRST + f, qs[f]) for f in range(n)]
    want = (b"".join(w[0] for w in want), [w[1][0] for w in want])
    assert _encode(torch, a, xa, FIRST, quality=qs) == want == _encode(torch, b, xb, FIRST, quality=qs)
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    s = a.frame_sizes(xa, quality=qs, status=st)
    a.flush()
    torch.cuda.synchronize()
    assert ([int(v) for v in s.cpu()], int(st.cpu()[0])) == (want[1], 0)
    a.close()
    b.close()


@pytest.mark.parametrize("preset", ("i012", "p016"))
def test_rate_calls_equal_the_plane_layout_on_the_bytes(torch_cuda, preset):
    """One budget encode, one rd encode, one batch-budget encode, one bitrate encode and the streams calls (two spans; with a
    bucket per stream and a budget per stream), with limits from the rd table so that the picks differ between frames."""
    torch = torch_cuda
    n, first = 5, 40
    a, xa, b, xb, _, _ = _pair(torch, preset, n)

    def both(call):
        ra, rb = call(a, xa), call(b, xb)
        assert ra == rb
        return ra

    sizes, dist, status = both(lambda e, x: _rd(torch, e, x, CANDS))
    assert status == [0] * len(CANDS)
    cap = sorted(sizes[2])[n // 2]
    both(lambda e, x: e.encode_to_budget(x, cap, CANDS, first_frame_index=first))
    both(lambda e, x: e.encode_to_distortion(x, sorted(dist[2])[n // 2], CANDS, first_frame_index=first))
    both(lambda e, x: e.encode_to_batch_budget(x, (sum(sizes[2]) + sum(sizes[3])) // 2, CANDS, first_frame_index=first))

    def cbr(e, x):
        level = torch.full((1,), 2 * cap, dtype=torch.int64, device="cuda")
        parts = [e.encode_at_bitrate(x[i:i + 2], cap, 2 * cap, CANDS, level, first_frame_index=first + i) for i in (0, 2)]
        return parts, int(level.cpu()[0])

    both(cbr)
    spans = [(2, 7), (3, 0)]
    assert len(both(lambda e, x: e.encode_streams(x, spans))[1]) == n

    def streams_cbr(e, x):
        levels = torch.full((2,), 2 * cap, dtype=torch.int64, device="cuda")
        return e.encode_streams_at_bitrate(x, spans, CANDS, cap, 2 * cap, levels), [int(v) for v in levels.cpu()]

    both(streams_cbr)
    both(lambda e, x: e.encode_streams_to_budget(x, spans, CANDS, [cap, 3 * cap]))
    a.close()
    b.close()


@pytest.mark.parametrize("preset", ("i010", "p010"))
def test_pipelined_delivery_stream_and_fallback_equal_the_plane_layout(torch_cuda, preset):
    """Pipelined mode, HostDelivery.step (with its scratch retry: the arena is not reserved and the LDS image is 8 words, so the
    first attempt runs out of scratch), the global-memory fallback with the worst-case arena reserved, a non-default stream, the
    profile counters."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    n, first = 5, 40
    a, xa, b, xb, _, lay = _pair(torch, preset, n)
    qs = [3, 12, 7, 9, 5]

    def both(call):
        ra, rb = call(a, xa), call(b, xb)
        assert ra == rb
        return ra

    def delivered(e, x):
        hd = HostDelivery(e, n)
        hd.step(x, first)
        hd.fence()
        out = (bytes(hd.result().numpy()), [int(v) for v in hd.frame_sizes(n)])
        hd.close()
        return out

    plain = both(lambda e, x: _encode(torch, e, x, first))
    assert both(delivered) == plain
    side = torch.cuda.Stream()                                  # a non-default stream
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert _encode(torch, a, xa, first) == plain
        assert _table(torch, a, xa, K8) == _table(torch, b, xb, K8)
    torch.cuda.synchronize()
    for e in (a, b):
        e.debug_set_lds_words(8)
    assert both(delivered) == plain                             # the scratch retry
    for e in (a, b):
        e.reserve_scratch(True)
    assert both(lambda e, x: _encode(torch, e, x, first)) == plain      # every unit through the arena
    assert both(lambda e, x: _table(torch, e, x, K8))[1] == [0] * 8
    for e in (a, b):
        e.debug_set_lds_words(0)
        e.reserve_scratch(False)
        e.set_pipelined(True)
    assert a.downscale_word_layout == lay
    assert both(lambda e, x: (_encode(torch, e, x, first), _encode(torch, e, x[1:4], first + 1, quality=qs[1:4]),
                              _table(torch, e, x, K8)))[0] == plain
    for e in (a, b):
        e.set_pipelined(False)
        e.profile(True)
    both(lambda e, x: (_encode(torch, e, x, first), e.profile_read()[0]))        # (launches; the milliseconds differ)
    a.close()
    b.close()


def test_to_i420_needs_the_whole_source_inside_the_frame_stride(torch_cuda):
    """The setter holds a layout to the coded region's extent, the to-i420 call reads the whole 2W x 2H source: on a width that is
    no multiple of 16 and in strict mode a frame stride of exactly E serves every encode and is refused by the to-i420 call,
    before anything is launched; with the whole source inside the stride it is served."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    from ec504_imageencoder_amd.encoder import downscale_word_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    for W, H, mode, preset in ((40, 32, "full", "p010"), (112, 160, "strict", "i010")):
        src = dw.noise_for(W, H, preset, 2)
        x, lay, _ = dw.place(torch, src, preset, **dw.PITCHED)
        enc = Mpeg1Encoder(W, H, 12, mode, max_frames=2)
        E = downscale_word_layout_extent(lay, enc.strips, enc.mb_rows)
        assert E < x.shape[1] <= lay["frame_stride"]
        enc.set_downscale_word_layout(dict(lay, frame_stride=E))
        full = _encode(torch, enc, x[:1], 0)
        out = torch.zeros((1, W * H * 3 // 2), dtype=torch.uint8, device="cuda")
        assert L.m1v_downscale_words_to_i420_device(enc._h, C.c_void_p(x.data_ptr()), 1, C.c_void_p(out.data_ptr()), None) == _ffi.E_ARG
        assert b"whole source" in L.m1v_last_error() and b"frame stride below" in L.m1v_last_error()
        torch.cuda.synchronize()
        assert not out.any()
        enc.set_downscale_word_layout(lay)
        assert _encode(torch, enc, x[:1], 0) == full
        assert np.array_equal(_i420_of(torch, enc, x), dw.down2_words(src, dw.SHIFT[preset]))
        with pytest.raises(AssertionError, match="whole source"):
            enc.downscale_words_to_i420(x[:, :E])
        enc.close()
