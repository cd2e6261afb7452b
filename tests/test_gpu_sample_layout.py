"""GPU tests of the sample input layout (m1v_set_sample_layout with y_step = 2, c_step = 4; k_encode_step2, k_size_table_step2,
k_rd_table_step2; -m gpu): packed 4:2:2 frames (YUY2, UYVY, YVYU) and P010 frames encoded where they lie.

The checker is tests/sample_oracle.py (tests/plane_oracle.py's frame walk with samplers that step through the luma row too;
pinned by tests/test_sample_layout_abi.py).  A frame buffer is noise as a whole: the addressed bytes are the picture, every other
byte is padding.  Frames lie at least 64 bytes inside their allocation on both sides.  Every comparison is for equality and every
status word is 0 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import sample_oracle
from gpu_calls import _encode, _table
from layout_inputs import GUARD, _noise, _scatter
from layout_inputs import _sample_view as _view

pytestmark = pytest.mark.gpu

PRESETS = ("yuy2", "uyvy", "yvyu", "p010")
LAYOUTS = PRESETS + ("yuy2_window", "p010_window")
# one macroblock; three strips; one whole tile (8 strips x 4 macroblock rows); a second tile column of one strip and a last tile
# row of one macroblock row; 11 strips (3 in the last tile column) and 5 macroblock rows; three tile columns and rows
SIZES = ((16, 16), (48, 16), (136, 72), (144, 80), (176, 80), (272, 144))
QUALITIES = (12, 76, 77, 100)       # byte staging up to 76, halfword staging from 77
BATCHES = (1, 3, 9)                 # up to 8 frames and more: both branches of the workgroup -> (frame, tile) map


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _layout(name, W, H):
    """(layout dict with no zeros, byte offset of frame 0 in the buffer)."""
    from ec504_imageencoder_amd import sample_layout_preset
    if name in PRESETS:
        return sample_layout_preset(W, H, name), GUARD
    if name == "yuy2_window":                   # pitch > 2 W, an odd base, a gap between the frames
        yp = 2 * W + 36
        return dict(y_offset=0, cb_offset=1, cr_offset=3, y_pitch=yp, c_pitch=2 * yp, y_step=2, c_step=4, frame_stride=H * yp + 101), GUARD + 3
    assert name == "p010_window"                # a window 3 samples into both planes of a pitched surface, a gap between the planes
    yp = 2 * W + 64
    cb = H * yp + 32 + 8 + 1
    return dict(y_offset=6 + 1, cb_offset=cb, cr_offset=cb + 2, y_pitch=yp, c_pitch=yp, y_step=2, c_step=4,
                frame_stride=cb + (H // 2) * yp + 200), GUARD


def _want(orc, host, n, lay, base, W, H, first, qs):
    return [sample_oracle.encode_layout(host[base + f * lay["frame_stride"]:], lay, W, H, first + f, qs[f], orc.MODE_FULL) for f in range(n)]


def _encoder(W, H, Q, n, lay, channels=3):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, "full", channels=channels, max_frames=n)
    enc.set_sample_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1 and enc.sample_layout == lay
    return enc


def _gather(host, n, lay, base, W, H):
    """The samples the definition addresses: Y [n, H, W], Cb, Cr [n, H / 2, W / 2]."""
    Ys, Cbs, Crs = [], [], []
    for f in range(n):
        fr = host[base + f * lay["frame_stride"]:]
        r, c = np.mgrid[0:H, 0:W]
        Ys.append(fr[lay["y_offset"] + r * lay["y_pitch"] + c * lay["y_step"]])
        r, c = np.mgrid[0:H // 2, 0:W // 2]
        Cbs.append(fr[lay["cb_offset"] + r * lay["c_pitch"] + c * lay["c_step"]])
        Crs.append(fr[lay["cr_offset"] + r * lay["c_pitch"] + c * lay["c_step"]])
    return np.stack(Ys), np.stack(Cbs), np.stack(Crs)


def _i420(torch, Y, Cb, Cr):
    """The tightly packed I420 frames [n, W * H * 3 / 2] of the samples, on the device (set_plane_layout("i420"))."""
    n = Y.shape[0]
    return torch.from_numpy(np.concatenate([Y.reshape(n, -1), Cb.reshape(n, -1), Cr.reshape(n, -1)], axis=1)).cuda()


# ---- 1. the parity matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,size,layout", [(i * len(LAYOUTS) + j, s, l) for i, s in enumerate(SIZES) for j, l in enumerate(LAYOUTS)])
def test_parity_matrix(torch_cuda, orc, k, size, layout):
    """Records, sizes and total of encode, and the size-table and rd-table rows, at every quality; the batch size rotates so that
    every size and layout meets batches of 1, 3 and 9 and every quality meets every batch size."""
    torch = torch_cuda
    W, H = size
    lay, base = _layout(layout, W, H)
    for qi, Q in enumerate(QUALITIES):
        n, first = BATCHES[(k + qi) % 3], 17 + qi
        host = _noise(n, lay, base, seed=1000 * k + qi, amp=64 if Q == 100 else 256)
        want = _want(orc, host, n, lay, base, W, H, first, [Q] * n)
        enc = _encoder(W, H, Q, n, lay)
        dev = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc)
        got, sizes = _encode(torch, enc, dev, first)
        assert sizes == [len(r) for r in want], (Q, n)
        assert len(got) == sum(sizes) and got == b"".join(want), (Q, n)
        table, status = _table(torch, enc, dev, (Q,))
        assert status == [0] and table == [sizes], (Q, n)
        rd_sizes, _ = enc.frame_rd_table(dev, (Q,))
        torch.cuda.synchronize()
        assert rd_sizes.cpu().numpy().tolist() == [sizes], (Q, n)
        enc.close()


# ---- 2. A/B on the device, without the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [12, 90])
@pytest.mark.parametrize("W,H", [(176, 80), (272, 144)])
def test_yuy2_equals_its_samples_as_i420(torch_cuda, W, H, Q):
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n = 3
    lay, base = _layout("yuy2", W, H)
    host = _noise(n, lay, base, seed=W + Q, amp=64)
    rows = host[base:base + n * lay["frame_stride"]].reshape(n, H, 2 * W)
    planes = _i420(torch, rows[:, :, 0::2], rows[:, 0::2, 1::4], rows[:, 0::2, 3::4])      # chroma of the even rows
    enc = _encoder(W, H, Q, n, lay)
    ref = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    ref.set_plane_layout("i420")
    dev = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc)
    assert _encode(torch, enc, dev, 9) == _encode(torch, ref, planes, 9)
    assert _table(torch, enc, dev, (3, Q)) == _table(torch, ref, planes, (3, Q))
    enc.close()
    ref.close()


@pytest.mark.parametrize("Q", [12, 90])
@pytest.mark.parametrize("W,H", [(176, 80), (272, 144)])
def test_p010_equals_nv12_of_the_truncated_samples(torch_cuda, W, H, Q):
    """Random 10-bit values << 6 as a uint16 tensor viewed as bytes; the coded sample is v >> 2."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n = 3
    rng = np.random.default_rng(W * 7 + Q)
    v = (384 + rng.integers(0, 256, (n, H * 3 // 2, W))).astype(np.uint16)     # 10-bit values whose high bytes span 96..159
    words = torch.from_numpy((v << 6).view(np.int16)).cuda()
    assert words.dtype == torch.int16 and words.element_size() == 2
    frames = torch.zeros(n * 3 * W * H + 2 * GUARD, dtype=torch.uint8, device="cuda")
    frames[GUARD:-GUARD] = words.view(torch.uint8).reshape(-1)
    enc = _encoder(W, H, Q, n, _layout("p010", W, H)[0])
    dev = _view(torch, frames, n, enc.sample_layout, GUARD, enc)
    ref = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    ref.set_plane_layout("nv12")
    nv12 = torch.from_numpy((v >> 2).astype(np.uint8).reshape(n, -1)).cuda()
    assert _encode(torch, enc, dev, 2) == _encode(torch, ref, nv12, 2)
    assert _table(torch, enc, dev, (3, Q)) == _table(torch, ref, nv12, (3, Q))
    enc.close()
    ref.close()


# ---- 3. every byte value in every position -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["yuy2", "p010"])
def test_every_byte_value_in_every_position(torch_cuda, orc, layout):
    """Flat 8x8 cells of all 256 values at quality 50 (the DC level is the byte), frame p varying component p."""
    torch = torch_cuda
    W = H = 256
    n, Q = 3, 50
    lay, base = _layout(layout, W, H)
    host = _noise(n, lay, base, seed=9)
    cells = lambda k: (np.arange(k * k).reshape(k, k) % 256).astype(np.uint8).repeat(8, axis=0).repeat(8, axis=1)
    Y = np.full((n, H, W), 128, np.uint8)
    Cb = np.full((n, H // 2, W // 2), 128, np.uint8)
    Cr = np.full((n, H // 2, W // 2), 128, np.uint8)
    Y[0], Cb[1], Cr[2] = cells(32), cells(16), cells(16)
    assert all(len(np.unique(p)) == 256 for p in (Y[0], Cb[1], Cr[2]))
    _scatter(host, lay, base, Y, Cb, Cr)
    want = _want(orc, host, n, lay, base, W, H, 0, [Q] * n)
    enc = _encoder(W, H, Q, n, lay)
    got, sizes = _encode(torch, enc, _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc), 0)
    assert sizes == [len(r) for r in want] and got == b"".join(want)
    enc.close()


# ---- 4. padding is never used -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["yuy2", "uyvy", "p010", "yuy2_window", "p010_window"])
def test_padding_is_never_used(torch_cuda, orc, layout):
    """176 x 80 (three strips in the last tile column, a last tile row of one macroblock row; tightly packed, the last units of
    the frame end at its last byte).  The addressed samples under two fills of every other byte — row padding, the bytes between
    frames, the low byte of every P010 word, the chroma bytes of odd rows, the bytes in front of the first and behind the last
    frame: identical records and tables, the oracle's."""
    torch = torch_cuda
    W, H, n, Q = 176, 80, 3, 12
    lay, base = _layout(layout, W, H)
    picture = _noise(n, lay, base, seed=31)
    mask = np.zeros(picture.size, bool)
    for f in range(n):
        at = base + f * lay["frame_stride"]
        mask[at:at + lay["frame_stride"]] |= sample_oracle.addressed_mask(lay, W, H, lay["frame_stride"])
    assert int(mask.sum()) == n * W * H * 3 // 2 and not mask[:base].any() and not mask[-GUARD:].any()
    results = []
    for fill in (1, 2):
        host = np.where(mask, picture, _noise(n, lay, base, seed=40 + fill))
        enc = _encoder(W, H, Q, n, lay)
        dev = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc)
        rd = enc.frame_rd_table(dev, (5, Q))
        torch.cuda.synchronize()
        results.append((_encode(torch, enc, dev, 3), _table(torch, enc, dev, (5, Q)), [t.cpu().numpy().tolist() for t in rd]))
        enc.close()
    assert results[0] == results[1]
    want = _want(orc, picture, n, lay, base, W, H, 3, [Q] * n)
    assert results[0][0] == (b"".join(want), [len(r) for r in want])
    assert results[0][1][1] == [0, 0] and results[0][1][0][1] == [len(r) for r in want]


# ---- 5. every call ------------------------------------------------------------------------------------------------------------
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
CANDS5 = (2, 4, 6, 8, 12)


def _mixed(n, lay, base, seed):
    """Frames of different activity (so that the rate rules pick different qualities): noise of amplitude 256, 64, 16, ..."""
    host = _noise(n, lay, base, seed)
    for f in range(n):
        at = base + f * lay["frame_stride"]
        amp = (256, 64, 16, 128, 32, 8)[f % 6]
        if amp != 256:
            host[at:at + lay["frame_stride"]] = 100 + (host[at:at + lay["frame_stride"]].astype(np.int32) * amp >> 8)
    return host


def test_every_call(torch_cuda):
    """With one YUY2 window layout in force every call returns what it returns for the same samples as I420 frames on the plane
    kernels (their own tests hold those against the oracle and the rate rules)."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n, first = 176, 80, 6, 40
    lay, base = _layout("yuy2_window", W, H)
    host = _mixed(n, lay, base, seed=5)
    a = _encoder(W, H, 12, n, lay)
    b = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    b.set_plane_layout("i420")
    xa = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, a)
    xb = _i420(torch, *_gather(host, n, lay, base, W, H))
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
    s = [table[0][K8.index(c)] for c in CANDS5]
    cap = sorted(x for row in s for x in row)[len(s) * n // 2]
    got = both(lambda e, x: e.encode_to_budget(x, cap, CANDS5, first_frame_index=first))
    assert len(set(got[2])) > 1, got[2]
    both(lambda e, x: e.encode_best_in_budget(x, cap, CANDS5, first_frame_index=first))
    both(lambda e, x: e.encode_to_batch_budget(x, (sum(s[1]) + sum(s[2])) // 2, CANDS5, first_frame_index=first))
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

    def small_image(e, x):
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
    assert a.sample_layout == lay and a.path == "tiles"
    for _ in range(2):
        assert both(lambda e, x: (_encode(torch, e, x, first), _encode(torch, e, x[1:4], first + 1, quality=qs[1:4]),
                                  _table(torch, e, x, CANDS5)))[0] == plain
    a.close()
    b.close()


# ---- 6. status and errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["yuy2", "p010"])
def test_unencodable_level_is_reported(torch_cuda, orc, layout):
    """Luma of 255 / 0 in bands of four rows: at quality 92 a block has an AC level the VLC cannot code, at 76 it codes."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    W, H, n = 96, 48, 1
    lay, base = _layout(layout, W, H)
    host = _noise(n, lay, base, seed=4)
    bands = np.where((np.arange(H)[:, None] % 8) < 4, 255, 0).astype(np.uint8).repeat(W, axis=1)[None]
    flat = np.full((1, H // 2, W // 2), 128, np.uint8)
    _scatter(host, lay, base, bands, flat, flat)
    with pytest.raises(sample_oracle.Unencodable):
        sample_oracle.encode_layout(host[base:], lay, W, H, 0, 92, orc.MODE_FULL)
    ok76 = sample_oracle.encode_layout(host[base:], lay, W, H, 0, 76, orc.MODE_FULL)
    enc = _encoder(W, H, 92, n, lay)
    dev = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc)
    out = torch.empty(enc.frame_bound, dtype=torch.uint8, device="cuda")
    _, _, meta = enc.encode(dev, 0, out=out)
    enc.flush()
    torch.cuda.synchronize()
    assert int(meta.cpu()[1]) & 0xFFFFFFFF == _ffi.STATUS_UNENCODABLE
    table, status = _table(torch, enc, dev, (76, 92))
    assert status == [0, _ffi.STATUS_UNENCODABLE] and table[0] == [len(ok76)]
    assert _encode(torch, enc, dev, 0, quality=[76]) == (ok76, [len(ok76)])
    enc.close()


def test_argument_errors_leave_the_encoder_usable(torch_cuda, orc):
    """Every M1V_E_ARG case of m1v_set_sample_layout; none of them changes the layout in force or the bytes."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    from ec504_imageencoder_amd.encoder import plane_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 176, 80, 2
    good, base = _layout("yuy2_window", W, H)
    host = _noise(n, good, base, seed=56)
    want = _want(orc, host, n, good, base, W, H, 0, [12] * n)
    want = (b"".join(want), [len(r) for r in want])
    enc = _encoder(W, H, 12, n, good)
    dev = _view(torch, torch.from_numpy(host).cuda(), n, good, base, enc)
    extent = plane_layout_extent(good, enc.strips, enc.mb_rows)
    bad = [dict(good, y_step=2, c_step=1), dict(good, y_step=2, c_step=2), dict(good, y_step=1, c_step=4), dict(good, y_step=3, c_step=4),
           dict(good, y_step=2, c_step=3), dict(good, y_step=1, c_step=3), dict(good, y_step=0, c_step=4), dict(good, y_step=2, c_step=0),
           dict(good, y_step=4, c_step=4), dict(good, y_step=2, c_step=8),
           dict(good, cb_offset=0, cr_offset=4), dict(good, cb_offset=5, cr_offset=1), dict(good, cr_offset=good["c_pitch"] + 1),
           dict(good, y_pitch=2 * W - 1), dict(good, y_pitch=W), dict(good, c_pitch=2 * W - 1), dict(good, c_pitch=W),
           dict(good, frame_stride=extent - 1), dict(good, frame_stride=0),
           dict(good, y_offset=2 ** 32), dict(good, cr_offset=2 ** 32 - 100, cb_offset=2 ** 32 - 102, frame_stride=2 ** 40),
           dict(good, y_pitch=2 ** 32 // (H - 1) + 1, frame_stride=2 ** 40), dict(good, c_pitch=2 ** 33, frame_stride=2 ** 50)]
    for lay in bad:
        assert L.m1v_set_sample_layout(enc._h, C.byref(_ffi.SampleLayout(**lay))) == _ffi.E_ARG, lay
        assert enc.sample_layout == good and enc.path == "tiles"
        with pytest.raises(EncoderError):
            enc.set_sample_layout(lay)
    assert _encode(torch, enc, dev, 0) == want
    assert L.m1v_set_sample_layout(enc._h, C.byref(_ffi.SampleLayout(**dict(good, frame_stride=extent)))) == 0   # the smallest stride
    enc.set_sample_layout(good)
    assert _encode(torch, enc, dev, 0) == want
    enc.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)
    assert L.m1v_set_sample_layout(rgba._h, C.byref(_ffi.SampleLayout(**good))) == _ffi.E_ARG              # channels != 3
    assert rgba.sample_layout is None and rgba.path == "runs"
    assert L.m1v_set_sample_layout(rgba._h, None) == 0
    rgba.close()
    hooked = Mpeg1Encoder(352, 288, 12, "full", max_frames=n)                                              # a run-kernel hook
    px = np.random.default_rng(1).integers(0, 256, (n, 288, 352, 3), dtype=np.uint8)
    packed = torch.from_numpy(px).cuda()
    before = _encode(torch, hooked, packed, 0)
    hooked.debug_set_path("runs")
    with pytest.raises(EncoderError) as ei:
        hooked.set_sample_layout("yuy2")
    assert ei.value.code == _ffi.E_ARG and hooked.sample_layout is None and hooked.path == "runs"
    assert _encode(torch, hooked, packed, 0) == before
    hooked.debug_set_path("auto")
    hooked.set_sample_layout("yuy2")
    with pytest.raises(EncoderError) as ei:
        hooked.debug_set_path("runs")                                                                       # and the other way round
    assert ei.value.code == _ffi.E_ARG and hooked.path == "tiles"
    hooked.close()


def test_injected_allocation_failure_changes_nothing(torch_cuda, orc):
    """m1v_debug_fail_alloc (EC504_DEBUG_HOOKS=1) under a sample layout: a reconfiguration that fails in an allocation leaves
    layout, plan, scratch and bytes as they were (set_sample_layout itself may find nothing to allocate: then it succeeds;
    reserve_scratch and set_pipelined always allocate at this size)."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 4                       # (the geometry of the plane layouts' test: its worst-case arena is an allocation)
    lay, base = _layout("p010_window", W, H)
    host = _noise(n, lay, base, seed=57)
    want = _want(orc, host, n, lay, base, W, H, 5, [12] * n)
    want = (b"".join(want), [len(r) for r in want])
    px = np.random.default_rng(2).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    packed = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    rgb = _encode(torch, enc, packed, 5)

    def armed(call):
        before = (enc.sample_layout, enc.path, enc.scratch_bytes())
        _ffi.lib().m1v_debug_fail_alloc(1)
        try:
            call()
            rc = None
        except EncoderError as e:
            rc = e.code
        finally:
            _ffi.lib().m1v_debug_fail_alloc(0)
        if rc is not None:
            assert rc == _ffi.E_HIP and (enc.sample_layout, enc.path, enc.scratch_bytes()) == before
        return rc

    if armed(lambda: enc.set_sample_layout(lay)) is not None:
        assert enc.sample_layout is None and _encode(torch, enc, packed, 5) == rgb
        enc.set_sample_layout(lay)
    dev = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc)
    assert enc.sample_layout == lay and _encode(torch, enc, dev, 5) == want
    assert armed(lambda: enc.reserve_scratch(True)) == _ffi.E_HIP
    assert enc.sample_layout == lay and _encode(torch, enc, dev, 5) == want
    assert armed(lambda: enc.set_pipelined(True)) == _ffi.E_HIP
    assert enc.sample_layout == lay and _encode(torch, enc, dev, 5) == want
    if armed(lambda: enc.set_sample_layout(None)) is not None:
        assert enc.sample_layout == lay and _encode(torch, enc, dev, 5) == want
        enc.set_sample_layout(None)
    assert enc.sample_layout is None and _encode(torch, enc, packed, 5) == rgb
    enc.close()


def test_sample_plane_surface_and_default_layouts_replace_each_other(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi, plane_layout_preset
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 176, 80, 3
    px = np.random.default_rng(55).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    packed = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    assert enc.sample_layout is None and enc.plane_layout is None
    rgb = _encode(torch, enc, packed, 5)
    assert rgb == (b"".join(orc.encode_frame(px[f], W, H, 5 + f, 12, orc.MODE_FULL) for f in range(n)), rgb[1])
    lay, base = _layout("uyvy", W, H)
    host = _noise(n, lay, base, seed=58)
    want = _want(orc, host, n, lay, base, W, H, 5, [12] * n)
    want = (b"".join(want), [len(r) for r in want])
    enc.set_sample_layout("uyvy")                                       # default -> sample
    assert enc.sample_layout == lay and enc.path == "tiles" and enc.size_table_fused == 1
    dev = _view(torch, torch.from_numpy(host).cuda(), n, lay, base, enc)
    assert _encode(torch, enc, dev, 5) == want
    # the older queries refuse and name the new one; the new one answers
    for query in (lambda: enc.plane_layout, lambda: enc.input_layout):
        with pytest.raises(EncoderError) as ei:
            query()
        assert ei.value.code == _ffi.E_ARG and "m1v_sample_layout_in_force" in str(ei.value)
    assert L.m1v_plane_layout_in_force(enc._h, None) == _ffi.E_ARG and "m1v_sample_layout_in_force" in _ffi.last_error()
    got = _ffi.SampleLayout()
    assert L.m1v_sample_layout_in_force(enc._h, C.byref(got)) == 1 and got.as_dict() == lay
    assert L.m1v_sample_layout_in_force(enc._h, None) == 1
    with pytest.raises(AssertionError):
        enc.encode(packed)                                              # [n, H, W, 3] is not a frame tensor of this layout
    with pytest.raises(AssertionError):
        enc.encode(dev[:, :-1])                                         # a byte short of the extent
    # packed-only entry points refuse, as under a plane layout
    hostpx = np.zeros((n, H, W, 3), np.uint8)
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(hostpx),
                 lambda: enc.encode_host(hostpx, with_planes=True)):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG
    nv12 = plane_layout_preset(W, H, "nv12")
    enc.set_plane_layout("nv12")                                        # sample -> plane, by the older call
    assert enc.plane_layout == nv12 and enc.sample_layout == dict(nv12, y_step=1)
    planes = torch.from_numpy(host[base:base + n * nv12["frame_stride"]].reshape(n, -1).copy()).cuda()
    as_planes = _encode(torch, enc, planes, 5)
    enc.set_sample_layout(dict(nv12, y_step=1))                         # the same layout by the new call: the same kernels
    assert enc.plane_layout == nv12 and enc.sample_layout == dict(nv12, y_step=1)
    assert _encode(torch, enc, planes, 5) == as_planes
    enc.set_sample_layout({k: v for k, v in nv12.items() if k != "c_pitch"})    # steps and pitches default as in the header
    assert enc.plane_layout == dict(nv12) and _encode(torch, enc, planes, 5) == as_planes
    enc.set_sample_layout(lay)                                          # plane -> sample
    assert _encode(torch, enc, dev, 5) == want
    enc.set_input_layout(W * 3 + 64, 0, "rgb")                          # sample -> surface
    assert enc.sample_layout is None and enc.input_layout == (W * 3 + 64, H * (W * 3 + 64), "rgb")
    surf = torch.zeros((n, H, W * 3 + 64), dtype=torch.uint8, device="cuda")
    view = torch.as_strided(surf, (n, H, W, 3), (H * (W * 3 + 64), W * 3 + 64, 3, 1))
    view.copy_(packed)
    assert _encode(torch, enc, view, 5) == rgb
    enc.set_sample_layout(lay)                                          # surface -> sample
    assert enc.sample_layout == lay and _encode(torch, enc, dev, 5) == want
    enc.set_sample_layout(None)                                         # sample -> default
    assert enc.sample_layout is None and enc.plane_layout is None and enc.input_layout == (0, 0, "rgb")
    assert _encode(torch, enc, packed, 5) == rgb                        # the RGB record of before the round trip
    enc.set_sample_layout(lay)
    enc.set_plane_layout(None)                                          # ... and by the older call
    assert enc.sample_layout is None and _encode(torch, enc, packed, 5) == rgb
    enc.close()
