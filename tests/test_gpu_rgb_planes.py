"""GPU tests of the RGB plane input layout (m1v_set_rgb_plane_layout; k_encode_rgb_planes, k_size_table_rgb_planes,
k_rd_table_rgb_planes; -m gpu): frames whose R, G and B bytes lie in three planes — NCHW uint8 tensors in any plane order, three
planes of a 4-plane tensor, pitched windows, planes interleaved by rows — encoded where they lie.

The checker is the CPU oracle on the interleaved picture: a planar buffer is a device buffer of noise into which the planes of a
packed [n, H, W, 3] array are written through the strided view the encoder is given, so the expected record is the oracle's for
the array the test started from.  Every frame lies at least 64 bytes inside its allocation.  Every comparison is for equality and
every status word is 0 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import hard_content as hc
import rd_oracle
from colour_content import _CH, _COLOURS_PER_FRAME, _CW, _flat_cell_frames, _tie_colours
from gpu_calls import _encode, _frames, _mixed_frames, _table
from layout_inputs import _planar

pytestmark = pytest.mark.gpu

# one macroblock; 3 strips in one partial tile (a chroma unit that overhangs its half row); 9 strips x 5 macroblock rows (a 2 x 2
# tile grid whose last column holds one strip); 11 strips (3, odd, in the last tile column); 17 strips (1 in the third tile
# column); 22 strips (6, even, in the last tile column)
SIZES = ((16, 16), (48, 32), (144, 80), (176, 144), (272, 144), (352, 288))
LAYOUTS = ("rgb", "bgr", "gbr", "pitched", "rgba", "rows")
QUALITIES = (12, 76, 77, 100)       # byte staging up to 76, halfword staging from 77
BATCHES = (1, 3, 9, 17)             # up to 8 frames and more: both branches of the workgroup -> (frame, tile) map


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(W, H, Q, n, lay):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    enc.set_rgb_plane_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1 and enc.rgb_plane_layout == lay
    return enc


# ---- 1. the parity matrix ---------------------------------------------------------------------------------------------------
_expected_cache = {}


def _expected(orc, size, Q):
    """17 frames of noise of that size (amplitude 64 at quality 100, whose AC levels then stay below 256) and the oracle's
    records of them as frames 17.., computed once and shared by the layouts."""
    key = (size, Q)
    if key not in _expected_cache:
        W, H = size
        rng = np.random.default_rng(W * 1000 + H + Q)
        px = _frames(rng, max(BATCHES), W, H, 3, 64 if Q == 100 else 256)
        blob, sizes = orc.encode_frames(px, px.shape[0], W, H, 17, Q, orc.MODE_FULL, threads=16)
        sizes = [int(s) for s in sizes]
        px.setflags(write=False)
        _expected_cache[key] = (px, blob, sizes)
    return _expected_cache[key]


@pytest.mark.parametrize("k,size,layout", [(i * len(LAYOUTS) + j, s, l) for i, s in enumerate(SIZES) for j, l in enumerate(LAYOUTS)])
def test_parity_matrix(torch_cuda, orc, k, size, layout):
    """Records and sizes of encode, and the size-table and rd-table rows, at every quality; the batch size rotates so that every
    size and layout meets batches of 1, 3, 9 and 17 and every quality meets every batch size."""
    torch = torch_cuda
    W, H = size
    for qi, Q in enumerate(QUALITIES):
        n = BATCHES[(k + qi) % 4]
        px, blob, wsizes = _expected(orc, size, Q)
        dev, lay = _planar(torch, px[:n], layout, fill_seed=k)
        enc = _encoder(W, H, Q, n, lay)
        got, sizes = _encode(torch, enc, dev, 17)
        where = f"{layout} {W}x{H} quality {Q} batch {n}"
        assert sizes == wsizes[:n], (where, [f for f in range(n) if sizes[f] != wsizes[f]])
        at = np.concatenate([[0], np.cumsum(wsizes)])
        wrong = [f for f in range(n) if got[at[f]:at[f + 1]] != blob[at[f]:at[f + 1]]]
        assert not wrong and len(got) == at[n], (where, "frames", wrong)
        table, status = _table(torch, enc, dev, (Q,))
        assert status == [0] and table == [sizes], where
        rd_sizes, _ = enc.frame_rd_table(dev, (Q,))
        torch.cuda.synchronize()
        assert rd_sizes.cpu().numpy().tolist() == [sizes], where
        enc.close()


@pytest.mark.parametrize("layout", ["bgr", "pitched"])
def test_hard_content(torch_cuda, orc, layout):
    """tests/hard_content.py (every run length, escapes, blocks of more than 128 bits) at quality 92, the extreme patterns at 77."""
    torch = torch_cuda
    W, H = 176, 144
    px = hc.hard_frames(orc, W, H)
    qs = [hc.ENCODER_Q] * 3 + [hc.EXTREME_Q]
    want = [orc.encode_frame(px[f], W, H, 5 + f, qs[f], orc.MODE_FULL) for f in range(4)]
    dev, lay = _planar(torch, px, layout, fill_seed=7)
    enc = _encoder(W, H, hc.ENCODER_Q, 4, lay)
    got, sizes = _encode(torch, enc, dev, 5, quality=qs)
    assert sizes == [len(r) for r in want] and got == b"".join(want)
    enc.close()


# ---- 2. A/B on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [12, 90])
@pytest.mark.parametrize("W,H", [(176, 144), (352, 288)])
def test_planar_equals_packed_on_the_device(torch_cuda, W, H, Q):
    """The same pictures packed through the default 3-channel encoder and planar through the new layout: identical output
    buffers, sizes and status."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n = 5
    rng = np.random.default_rng(W + Q)
    px = _mixed_frames(rng, n, W, H, 3, (4, 40, 64, 20))
    packed = torch.from_numpy(px).cuda()
    ref = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    for layout in ("gbr", "rows"):
        dev, lay = _planar(torch, px, layout, fill_seed=3)
        enc = _encoder(W, H, Q, n, lay)
        outs = []
        for e, x in ((ref, packed), (enc, dev)):
            out = torch.zeros(e.frame_bound * n, dtype=torch.uint8, device="cuda")
            out, sizes, meta = e.encode(x, 9, out=out)
            e.flush()
            torch.cuda.synchronize()
            outs.append((out.cpu().numpy().tobytes(), sizes[:n].cpu().tolist(), meta.cpu().tolist()))
        assert outs[0] == outs[1] and outs[0][2][1] == 0
        assert _table(torch, enc, dev, (3, Q)) == _table(torch, ref, packed, (3, Q))
        enc.close()
    ref.close()


# ---- 3. colours -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_colour_inside_the_rgb_plane_kernels_ties_and_sample(torch_cuda, orc, order):
    """All tie / near-tie colours (every input that takes the fp64 branch) and 2^20 random colours as flat 8x8 cells at quality 50
    (the DC level is the converted byte), as Y, Cb and Cr each: the input set of
    tests/test_gpu_surface.py::test_colour_inside_the_surface_kernels_ties_and_sample, through the byte staging of the encode
    kernel and through its halfword staging (an encoder of quality 77 coding every frame at 50)."""
    torch = torch_cuda
    chunk = 48
    ties = _tie_colours()
    assert 50000 < len(ties) < 400000
    sample = np.random.default_rng(2024).integers(0, 256, (1 << 20, 3), dtype=np.uint8)
    colours = np.concatenate([ties, sample])
    _, lay = _planar(torch, np.zeros((chunk, _CH, _CW, 3), np.uint8), order)
    narrow, wide = _encoder(_CW, _CH, 50, chunk, lay), _encoder(_CW, _CH, 77, chunk, lay)
    per = _COLOURS_PER_FRAME * chunk
    for lo in range(0, len(colours), per):
        frames = _flat_cell_frames(colours[lo:lo + per], 3)
        n = frames.shape[0]
        want, wsizes = orc.encode_frames(frames, n, _CW, _CH, 0, 50, orc.MODE_FULL, threads=16)
        wsizes = [int(x) for x in wsizes]
        dev, got_lay = _planar(torch, frames, order, fill_seed=lo % 97)
        assert got_lay == lay
        got, sizes = narrow.encode_to_bytes(dev, 0)
        assert sizes == wsizes and got == want, f"colours {lo}..{lo + per}, byte staging"
        got, sizes = wide.encode_to_bytes(dev, 0, quality=[50] * n)
        assert sizes == wsizes and got == want, f"colours {lo}..{lo + per}, halfword staging"
        del dev
    narrow.close()
    wide.close()


# ---- 4. padding is never used -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rgb", "pitched", "rgba", "rows"])
def test_padding_is_never_used(torch_cuda, orc, layout):
    """48 x 32 (three strips in one partial tile: the chroma unit that overhangs its half row; tightly packed, the last plane ends
    with the frame) and 176 x 144.  The same pictures under two fills of every byte the definition does not address — row padding,
    the alpha plane, the 64 bytes in front of the first and behind the last frame, the gap between frames: identical records and
    tables, the oracle's."""
    torch = torch_cuda
    n, Q = 3, 12
    for W, H in ((48, 32), (176, 144)):
        px = _frames(np.random.default_rng(31 + W), n, W, H, 3)
        want = [orc.encode_frame(px[f], W, H, 3 + f, Q, orc.MODE_FULL) for f in range(n)]
        results = []
        for fill in (1, 2):
            dev, lay = _planar(torch, px, layout, fill_seed=40 + fill)
            enc = _encoder(W, H, Q, n, lay)
            rd = enc.frame_rd_table(dev, (5, Q))
            torch.cuda.synchronize()
            results.append((_encode(torch, enc, dev, 3), _table(torch, enc, dev, (5, Q)), [t.cpu().numpy().tolist() for t in rd]))
            enc.close()
        assert results[0] == results[1]
        assert results[0][0] == (b"".join(want), [len(r) for r in want])
        assert results[0][1][1] == [0, 0] and results[0][1][0][1] == [len(r) for r in want]


# ---- 5. every call ----------------------------------------------------------------------------------------------------------
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
CANDS5 = (2, 4, 6, 8, 12)


def test_every_call(torch_cuda, orc):
    """With a pitched R,G,B plane layout in force every call returns what it returns for the packed copy of the same pictures on
    the default encoder (whose own tests hold those against the oracle and the rate rules); the rd table also against
    tests/rd_oracle.py."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n, first = 144, 80, 9, 40
    px = _mixed_frames(np.random.default_rng(5), n, W, H, 3, (256, 64, 16, 128, 32, 8))
    xa, lay = _planar(torch, px, "pitched", fill_seed=5)
    a = _encoder(W, H, 12, n, lay)
    b = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    xb = torch.from_numpy(px).cuda()
    qs = [int(q) for q in np.random.default_rng(3).integers(1, 13, n)]

    def both(call):
        ra, rb = call(a, xa), call(b, xb)
        assert ra == rb
        return ra

    def sizes_of(e, x):
        st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
        s = e.frame_sizes(x, quality=qs, status=st)
        e.flush()
        torch.cuda.synchronize()
        return [int(v) for v in s.cpu()], int(st.cpu()[0])

    def rd_of(e, x):
        st = torch.full((8,), 0x40, dtype=torch.int32, device="cuda")
        s, d = e.frame_rd_table(x, K8, status=st)
        torch.cuda.synchronize()
        return s.cpu().numpy().tolist(), d.cpu().numpy().tolist(), [int(v) for v in st.cpu()]

    plain = both(lambda e, x: _encode(torch, e, x, first))
    both(lambda e, x: _encode(torch, e, x, first, quality=qs))
    assert both(sizes_of)[1] == 0
    table = both(lambda e, x: _table(torch, e, x, K8))
    assert table[1] == [0] * 8 and table[0][-1] == plain[1]
    rd = both(rd_of)
    assert rd[0] == table[0] and rd[2] == [0] * 8
    wsizes, wdist, wstatus = rd_oracle.rd_table(orc, px, K8, orc.MODE_FULL)
    assert (rd[0], rd[1], rd[2]) == (wsizes, wdist, wstatus)
    s = [table[0][K8.index(c)] for c in CANDS5]
    cap = sorted(x for row in s for x in row)[len(s) * n // 2]
    got = both(lambda e, x: e.encode_to_budget(x, cap, CANDS5, first_frame_index=first))
    assert len(set(got[2])) > 1, got[2]
    both(lambda e, x: e.encode_best_in_budget(x, cap, CANDS5, first_frame_index=first))
    B = (sum(s[1]) + sum(s[2])) // 2
    both(lambda e, x: e.encode_to_batch_budget(x, B, CANDS5, first_frame_index=first))
    both(lambda e, x: e.encode_best_in_batch_budget(x, B, CANDS5, first_frame_index=first))
    r = sorted(s[2])[2]

    def cbr(e, x):
        level = torch.full((1,), 10 ** 6, dtype=torch.int64, device="cuda")
        return e.encode_at_bitrate(x, r, 2 * r, CANDS5, level, first_frame_index=first), int(level.cpu()[0])

    both(cbr)

    def delivered(e, x):
        hd = HostDelivery(e, n)
        out = []
        hd.step(x, first)
        hd.step(x[:4], first + 50)
        hd.delivered[hd.last[0]].synchronize()
        out.append((bytes(hd.result().numpy()), [int(v) for v in hd.frame_sizes(n)]))
        hd.fence()
        out.append((bytes(hd.result().numpy()), [int(v) for v in hd.frame_sizes(4)]))
        hd.close()
        return out

    assert both(delivered)[0] == plain

    def small_image(e, x):                      # an 8-word LDS image: every tile builds its bits in global memory
        e.debug_set_lds_words(8)
        _, _, meta = e.encode(x, first)
        torch.cuda.synchronize()
        status = int(meta.cpu()[1]) & 0xFFFFFFFF
        e.reserve_scratch(True)
        reserved = _encode(torch, e, x, first)
        e.debug_set_lds_words(0)
        e.reserve_scratch(False)
        return status, reserved, _encode(torch, e, x, first)

    status, reserved, after = both(small_image)     # (whether the default arena holds every tile is the plan's business)
    assert status in (0, _ffi.STATUS_SCRATCH) and reserved == plain and after == plain
    for e in (a, b):
        e.set_pipelined(True)
    assert a.rgb_plane_layout == lay and a.path == "tiles"
    for _ in range(2):
        assert both(lambda e, x: (_encode(torch, e, x, first), _encode(torch, e, x[1:4], first + 1, quality=qs[1:4]),
                                  _table(torch, e, x, CANDS5)))[0] == plain
    a.close()
    b.close()


# ---- 6. status and reconfiguration ------------------------------------------------------------------------------------------
def test_unencodable_level_is_reported(torch_cuda, orc):
    """Grey of 255 / 0 in bands of four rows: at quality 92 a luma block has an AC level of 256 or more, which the format cannot
    code; at 76 it codes."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch = torch_cuda
    W, H, n = 96, 48, 1
    bands = np.where((np.arange(H)[:, None, None] % 8) < 4, 255, 0).astype(np.uint8).repeat(W, axis=1).repeat(3, axis=2)[None]
    with pytest.raises(ValueError):
        orc.encode_frame(bands[0], W, H, 0, 92, orc.MODE_FULL)
    ok76 = orc.encode_frame(bands[0], W, H, 0, 76, orc.MODE_FULL)
    dev, lay = _planar(torch, bands, "bgr", fill_seed=4)
    enc = _encoder(W, H, 92, n, lay)
    out = torch.empty(enc.frame_bound, dtype=torch.uint8, device="cuda")
    _, _, meta = enc.encode(dev, 0, out=out)
    enc.flush()
    torch.cuda.synchronize()
    assert int(meta.cpu()[1]) & 0xFFFFFFFF == _ffi.STATUS_UNENCODABLE
    with pytest.raises(EncoderError) as ei:
        enc.encode_to_bytes(dev, 0)
    assert ei.value.code == _ffi.E_UNENCODABLE
    table, status = _table(torch, enc, dev, (76, 92))
    assert status == [0, _ffi.STATUS_UNENCODABLE] and table[0] == [len(ok76)]
    assert _encode(torch, enc, dev, 0, quality=[76]) == (ok76, [len(ok76)])
    enc.close()


def test_argument_errors_leave_the_layout_in_force(torch_cuda, orc):
    """Every M1V_E_ARG case of m1v_set_rgb_plane_layout; none of them changes the layout in force or the bytes."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 176, 80, 2
    px = _frames(np.random.default_rng(56), n, W, H, 3)
    want = [orc.encode_frame(px[f], W, H, f, 12, orc.MODE_FULL) for f in range(n)]
    want = (b"".join(want), [len(r) for r in want])
    dev, good = _planar(torch, px, "pitched", fill_seed=1)
    P = good["row_pitch"]
    enc = _encoder(W, H, 12, n, good)
    big = 2 ** 40
    bad = [dict(good, row_pitch=W - 1), dict(good, row_pitch=0), dict(good, row_pitch=1),               # a pitch below W
           dict(good, b_offset=2 ** 32 - (H - 1) * P - W, frame_stride=big),                            # the extent reaches 2^32
           dict(good, r_offset=2 ** 32, frame_stride=big), dict(good, row_pitch=2 ** 32, frame_stride=big),
           dict(good, row_pitch=(2 ** 32 - good["b_offset"] - W) // (H - 1) + 1, frame_stride=big),
           dict(good, g_offset=0), dict(good, g_offset=W - 1), dict(good, g_offset=P + 5),               # planes that share bytes
           dict(good, b_offset=good["g_offset"] + (H - 1) * P + W - 1),
           dict(good, g_offset=good["r_offset"], b_offset=good["r_offset"]),
           dict(good, frame_stride=good["b_offset"] + (H - 1) * P + W - 1), dict(good, frame_stride=0)]   # frames closer than their span
    for lay in bad:
        assert L.m1v_set_rgb_plane_layout(enc._h, C.byref(_ffi.RgbPlaneLayout(**lay))) == _ffi.E_ARG, lay
        assert enc.rgb_plane_layout == good and enc.path == "tiles"
        with pytest.raises(EncoderError):
            enc.set_rgb_plane_layout(lay)
    assert _encode(torch, enc, dev, 0) == want
    # the largest extent whose offsets are still 32-bit (only set here; encoded in tests/test_gpu_address_space.py), the smallest
    # stride, and rows of the three planes interleaved with padding
    assert L.m1v_set_rgb_plane_layout(enc._h, C.byref(_ffi.RgbPlaneLayout(**dict(good, b_offset=2 ** 32 - (H - 1) * P - W - 1, frame_stride=big)))) == 0
    assert L.m1v_set_rgb_plane_layout(enc._h, C.byref(_ffi.RgbPlaneLayout(**dict(good, frame_stride=good["b_offset"] + (H - 1) * P + W)))) == 0
    assert L.m1v_set_rgb_plane_layout(enc._h, C.byref(_ffi.RgbPlaneLayout(0, W + 1, 2 * W + 2, 3 * W + 3, H * (3 * W + 3)))) == 0
    enc.set_rgb_plane_layout(good)
    assert _encode(torch, enc, dev, 0) == want
    enc.close()
    odd = Mpeg1Encoder(105, 49, 12, "full", max_frames=n)                                               # an odd width
    assert L.m1v_set_rgb_plane_layout(odd._h, C.byref(_ffi.RgbPlaneLayout(0, 105 * 49, 2 * 105 * 49, 105, 3 * 105 * 49))) == _ffi.E_ARG
    assert odd.rgb_plane_layout is None and odd.input_layout == (0, 0, "rgb")
    with pytest.raises(EncoderError):
        odd.set_rgb_plane_layout("rgb")
    odd.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)                                     # channels != 3
    assert L.m1v_set_rgb_plane_layout(rgba._h, C.byref(_ffi.RgbPlaneLayout(**good))) == _ffi.E_ARG
    assert rgba.rgb_plane_layout is None and rgba.path == "runs"
    assert L.m1v_set_rgb_plane_layout(rgba._h, None) == 0
    rgba.close()
    hooked = Mpeg1Encoder(352, 288, 12, "full", max_frames=n)                                           # a run-kernel hook
    big_px = _frames(np.random.default_rng(1), n, 352, 288, 3)
    packed = torch.from_numpy(big_px).cuda()
    before = _encode(torch, hooked, packed, 0)
    for force, undo in ((lambda: hooked.debug_set_path("runs"), lambda: hooked.debug_set_path("auto")),
                        (lambda: hooked.debug_set_input_mode(0), lambda: hooked.debug_set_input_mode(-1)),
                        (lambda: hooked.debug_set_dense_threads(64), lambda: hooked.debug_set_dense_threads(0))):
        force()
        with pytest.raises(EncoderError) as ei:
            hooked.set_rgb_plane_layout("rgb")
        assert ei.value.code == _ffi.E_ARG and hooked.rgb_plane_layout is None and hooked.path == "runs"
        assert _encode(torch, hooked, packed, 0) == before
        undo()
        hooked.set_rgb_plane_layout("rgb")
        with pytest.raises(EncoderError) as ei:
            force()                                                                                     # and the other way round
        assert ei.value.code == _ffi.E_ARG and hooked.path == "tiles"
        hooked.set_rgb_plane_layout(None)
    hooked.close()


def test_the_four_setters_replace_each_other(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 176, 80, 3
    px = _frames(np.random.default_rng(55), n, W, H, 3)
    packed = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    fresh = (enc.path, enc.size_table_fused, enc.scratch_bytes())
    assert enc.rgb_plane_layout is None
    rgb = _encode(torch, enc, packed, 5)
    assert rgb[0] == b"".join(orc.encode_frame(px[f], W, H, 5 + f, 12, orc.MODE_FULL) for f in range(n))
    dev, lay = _planar(torch, px, "rgba", fill_seed=2)
    enc.set_rgb_plane_layout(lay)                                       # default -> RGB planes
    assert enc.rgb_plane_layout == lay and enc.path == "tiles" and enc.size_table_fused == 1
    assert _encode(torch, enc, dev, 5) == rgb
    # the other queries refuse and name this one
    for query in (lambda: enc.plane_layout, lambda: enc.sample_layout, lambda: enc.input_layout):
        with pytest.raises(EncoderError) as ei:
            query()
        assert ei.value.code == _ffi.E_ARG and "m1v_rgb_plane_layout_in_force" in str(ei.value)
    got = _ffi.RgbPlaneLayout()
    assert L.m1v_rgb_plane_layout_in_force(enc._h, C.byref(got)) == 1 and got.as_dict() == lay
    assert L.m1v_rgb_plane_layout_in_force(enc._h, None) == 1
    # packed-only entry points refuse
    hostpx = np.zeros((n, H, W, 3), np.uint8)
    planes = np.zeros((n, 3, H * W), np.uint8)
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(hostpx),
                 lambda: enc.encode_host(hostpx, with_planes=True)):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG
    assert L.m1v_convert_host(enc._h, hostpx.ctypes.data, n, planes.ctypes.data) == _ffi.E_ARG
    enc.set_plane_layout("i420")                                        # RGB planes -> planes
    assert enc.rgb_plane_layout is None and enc.plane_layout is not None
    ycc = torch.from_numpy(np.random.default_rng(3).integers(96, 160, (n, W * H * 3 // 2), dtype=np.uint8)).cuda()
    enc_planes = _encode(torch, enc, ycc, 5)
    enc.set_rgb_plane_layout(lay)                                       # planes -> RGB planes
    assert enc.rgb_plane_layout == lay and _encode(torch, enc, dev, 5) == rgb
    enc.set_sample_layout("yuy2")                                       # RGB planes -> samples
    assert enc.rgb_plane_layout is None and enc.sample_layout["y_step"] == 2
    enc.set_rgb_plane_layout(lay)                                       # samples -> RGB planes
    assert _encode(torch, enc, dev, 5) == rgb
    enc.set_input_layout(W * 3 + 64, 0, "rgb")                          # RGB planes -> surface
    assert enc.rgb_plane_layout is None and enc.input_layout == (W * 3 + 64, H * (W * 3 + 64), "rgb")
    surf = torch.zeros((n, H, W * 3 + 64), dtype=torch.uint8, device="cuda")
    view = torch.as_strided(surf, (n, H, W, 3), (H * (W * 3 + 64), W * 3 + 64, 3, 1))
    view.copy_(packed)
    assert _encode(torch, enc, view, 5) == rgb
    enc.set_rgb_plane_layout(lay)                                       # surface -> RGB planes
    assert enc.rgb_plane_layout == lay and _encode(torch, enc, dev, 5) == rgb
    enc.set_plane_layout("i420")
    assert _encode(torch, enc, ycc, 5) == enc_planes
    enc.set_rgb_plane_layout(lay)
    enc.set_rgb_plane_layout(None)                                      # RGB planes -> default: the plan and bytes of a fresh encoder
    assert enc.rgb_plane_layout is None and enc.plane_layout is None and enc.input_layout == (0, 0, "rgb")
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes()) == fresh
    assert _encode(torch, enc, packed, 5) == rgb
    for restore in (lambda: enc.set_plane_layout(None), lambda: enc.set_sample_layout(None), lambda: enc.set_input_layout()):
        enc.set_rgb_plane_layout(lay)
        restore()                                                       # ... and by each of the older calls
        assert enc.rgb_plane_layout is None and _encode(torch, enc, packed, 5) == rgb
    enc.close()


def test_injected_allocation_failure_changes_nothing(torch_cuda, orc):
    """m1v_debug_fail_alloc (EC504_DEBUG_HOOKS=1) under an RGB plane layout: a reconfiguration that fails in an allocation leaves
    layout, plan, scratch and bytes as they were (on a 3-channel encoder the setter itself finds nothing to allocate — the plan
    is the tile plan on both sides — and then succeeds; reserve_scratch and set_pipelined always allocate at this size)."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 4
    px = _frames(np.random.default_rng(57), n, W, H, 3)
    want = [orc.encode_frame(px[f], W, H, 5 + f, 12, orc.MODE_FULL) for f in range(n)]
    want = (b"".join(want), [len(r) for r in want])
    packed = torch.from_numpy(px).cuda()
    dev, lay = _planar(torch, px, "pitched", fill_seed=8)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    assert _encode(torch, enc, packed, 5) == want

    def armed(call):
        before = (enc.rgb_plane_layout, enc.path, enc.scratch_bytes())
        _ffi.lib().m1v_debug_fail_alloc(1)
        try:
            call()
            rc = None
        except EncoderError as e:
            rc = e.code
        finally:
            _ffi.lib().m1v_debug_fail_alloc(0)
        if rc is not None:
            assert rc == _ffi.E_HIP and (enc.rgb_plane_layout, enc.path, enc.scratch_bytes()) == before
        return rc

    if armed(lambda: enc.set_rgb_plane_layout(lay)) is not None:
        assert enc.rgb_plane_layout is None and _encode(torch, enc, packed, 5) == want
        enc.set_rgb_plane_layout(lay)
    assert enc.rgb_plane_layout == lay and _encode(torch, enc, dev, 5) == want
    assert armed(lambda: enc.reserve_scratch(True)) == _ffi.E_HIP
    assert enc.rgb_plane_layout == lay and _encode(torch, enc, dev, 5) == want
    assert armed(lambda: enc.set_pipelined(True)) == _ffi.E_HIP
    assert enc.rgb_plane_layout == lay and _encode(torch, enc, dev, 5) == want
    if armed(lambda: enc.set_rgb_plane_layout(None)) is not None:
        assert enc.rgb_plane_layout == lay and _encode(torch, enc, dev, 5) == want
        enc.set_rgb_plane_layout(None)
    assert enc.rgb_plane_layout is None and _encode(torch, enc, packed, 5) == want
    enc.close()


# ---- 7. the Python checks ---------------------------------------------------------------------------------------------------
def test_python_checks_the_tensor_against_the_layout(torch_cuda, orc):
    """A sliced NCHW view goes in as it is; a tensor whose stride(3) is not 1, or whose strides are not the layout's, is refused."""
    from ec504_imageencoder_amd import Mpeg1Encoder, rgb_plane_strides
    torch = torch_cuda
    W, H, n = 48, 32, 2
    rng = np.random.default_rng(9)
    large = torch.from_numpy(rng.integers(0, 256, (n, 3, 70, 101), dtype=np.uint8)).cuda()
    window = large[:, :, 5:5 + H, 9:9 + W]
    assert not window.is_contiguous()
    px = np.ascontiguousarray(window.permute(0, 2, 3, 1).cpu().numpy())
    want = [orc.encode_frame(px[f], W, H, f, 12, orc.MODE_FULL) for f in range(n)]
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    with pytest.raises(AssertionError):
        enc.encode(window)                                              # the default layout takes packed frames
    enc.set_rgb_plane_layout(rgb_plane_strides(tuple(window.shape), tuple(window.stride())))
    assert _encode(torch, enc, window, 0) == (b"".join(want), [len(r) for r in want])
    assert _encode(torch, enc, window[1:], 1) == (want[1], [len(want[1])])      # one frame: its stride says nothing
    packed = torch.from_numpy(px).cuda()
    nchw = packed.permute(0, 3, 1, 2)                                   # [n, 3, H, W] with stride(3) == 3
    assert tuple(nchw.shape) == (n, 3, H, W) and nchw.stride(3) == 3
    contiguous = window.contiguous()                                    # another pitch and frame stride
    other_window = large[:, :, 5:5 + H, 10:10 + W][:, :, :, ::1][::1]
    for bad in (nchw, contiguous, packed, window[:, :2], window[:, :, :-16], large[:, :, 5:5 + H, 9:9 + W].to(torch.int8),
                torch.zeros((3, 3, 70, 101), dtype=torch.uint8, device="cuda")[::2, :, 5:5 + H, 9:9 + W]):   # another frame stride
        with pytest.raises(AssertionError):
            enc.encode(bad)
        with pytest.raises(AssertionError):
            enc.frame_size_table(bad, (4, 12))
    enc.encode(other_window)                                            # the same strides somewhere else: accepted
    enc.set_rgb_plane_layout("bgr")
    with pytest.raises(AssertionError):
        enc.encode(window)
    enc.encode(contiguous)
    enc.flush()
    torch.cuda.synchronize()
    enc.close()
