"""GPU tests of the downscale layout (m1v_set_downscale_layout; k_downscale_encode, k_downscale_size_table,
k_downscale_rd_table, k_downscale_to_bytes; -m gpu): [n, 2H, 2W, 3 | 4] uint8 surfaces whose 2 x 2 box average is encoded at
W x H, where they lie.

The definition (include/mpeg1_hip.h, "Downscale layout") is checked for equality on the bytes themselves (downscale_to_bytes)
against tests/downscale.py's down2; every expected record is the CPU oracle's on down2(source), and the rate calls are held against
the same calls on those bytes through the default packed layout.  A source is written into a device buffer of noise through a
strided view (downscale.place); every batch lies 64 bytes inside its allocation, so nothing here can fault.  Every comparison
is for equality and every status word is 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

import downscale as ds
import rd_oracle as rd
from gpu_calls import _encode, _rd, _table

pytestmark = pytest.mark.gpu

SIZES = ((48, 32), (96, 80))       # 3 strips x 2 rows in one partial tile; 6 x 5: two tile rows
K8 = (1, 2, 3, 5, 7, 9, 11, 12)
CANDS = (2, 5, 8, 10, 12)
# where a source lies: tight; rows padded by 1 and by 13 bytes; frames 5 bytes apart; a window at source pixel (3, 1) of a surface
PLACEMENTS = (dict(), dict(pad=1), dict(pad=13), dict(gap=5), dict(pad=13, gap=5, window=(3, 1), margin=(2, 3)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(W, H, Q, n, lay):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    enc.set_downscale_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1 and enc.downscale_layout == lay
    return enc


def _bytes_of(torch, enc, x):
    out = enc.downscale_to_bytes(x)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_oracle_cache = {}


def _oracle(orc, px, first, Q, key=None):
    """The oracle's (records, sizes) of the picture px; cached under `key` where several tests share it."""
    if key is not None and (key, first, Q) in _oracle_cache:
        return _oracle_cache[(key, first, Q)]
    blob, sizes = orc.encode_frames(px, px.shape[0], px.shape[2], px.shape[1], first, Q, orc.MODE_FULL, threads=16)
    got = (blob, [int(s) for s in sizes])
    if key is not None:
        _oracle_cache[(key, first, Q)] = got
    return got


def _noise(size, Cs, n=3):
    W, H = size
    src = ds.noise_source(W * 100 + H + Cs, n, H, W, Cs)
    src.setflags(write=False)
    return src


# ---- 1. the averaging ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", ds.WIDTHS)
@pytest.mark.parametrize("size", SIZES)
def test_averaging(torch_cuda, orc, size, Cs):
    """Noise sources in both orders and every placement: the bytes are down2's, records, sizes and status the oracle's on them, and
    the default packed encode of the bytes call's output gives the same records."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    W, H = size
    src = _noise(size, Cs)
    n = src.shape[0]
    packed = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    for order in ds.ORDERS:
        px = ds.down2(src, order)
        want = _oracle(orc, px, 17, 12, key=("noise", size, Cs, order))
        for k, where in enumerate(PLACEMENTS):
            x, lay, _ = ds.place(torch, src, Cs, order, fill_seed=k, **where)
            enc = _encoder(W, H, 12, n, lay)
            what = f"{W}x{H} x{Cs} {order} {where}"
            got = _bytes_of(torch, enc, x)
            assert got.shape == px.shape and got.dtype == np.uint8
            wrong = np.argwhere(got != px)
            assert not len(wrong), (what, len(wrong), [(tuple(w), int(got[tuple(w)]), int(px[tuple(w)])) for w in wrong[:8]])
            blob, sizes = _encode(torch, enc, x, 17)
            assert sizes == want[1], (what, [f for f in range(n) if sizes[f] != want[1][f]])
            at = np.concatenate([[0], np.cumsum(want[1])])
            assert not [f for f in range(n) if blob[at[f]:at[f + 1]] != want[0][at[f]:at[f + 1]]] and len(blob) == at[n], what
            assert _encode(torch, packed, enc.downscale_to_bytes(x), 17) == want, what
            enc.close()
    packed.close()


CELLS = [(255, 255, 255, 255)] + sorted({p for cell in ((255, 255, 255, 254), (0, 0, 0, 1), (1, 1, 0, 0), (1, 0, 0, 0))
                                         for p in itertools.permutations(cell)})


@pytest.mark.parametrize("Cs", ds.WIDTHS)
def test_extremes(torch_cuda, orc, Cs):
    """All 255 (the carry into bit 8 of every 16-bit half, 1020 + 2), and the four-value cells in every placement within the
    cell: 1019 rounds up to 255, 1 down to 0, the tie 2 up to 1, one frame per cell.  ({1, 0, 0, 0} in every placement is
    {0, 0, 0, 1} in every placement: 1 + 4 + 4 + 6 frames.)"""
    torch = torch_cuda
    W, H = 48, 32
    assert len(CELLS) == 1 + 4 + 4 + 6
    src = np.concatenate([ds.cell_source(cell, 1, H, W, Cs) for cell in CELLS])
    px = ds.down2(src)
    assert [int(px[f, 0, 0, 0]) for f in range(len(CELLS))] == [(sum(cell) + 2) >> 2 for cell in CELLS]
    assert {int(v) for v in np.unique(px)} == {0, 1, 255}
    want = _oracle(orc, px, 0, 12)
    x, lay, _ = ds.place(torch, src, Cs, "bgr", pad=1, gap=5)
    enc = _encoder(W, H, 12, len(CELLS), lay)
    got = _bytes_of(torch, enc, x)
    assert np.array_equal(got, px), [CELLS[f] for f in range(len(CELLS)) if not np.array_equal(got[f], px[f])]
    assert _encode(torch, enc, x, 0) == want
    enc.close()


# ---- 2. the read contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", ds.WIDTHS)
def test_read_contract(torch_cuda, orc, Cs):
    """The same pictures under two fills of everything else — row padding, the gaps between frames, the surface around the window
    (rows below 2H and pixels right of 2W lie inside the allocation), the 4th bytes, the guards: identical bytes, records and
    tables, the oracle's."""
    torch = torch_cuda
    W, H = 48, 32
    src = _noise((W, H), Cs)
    n = src.shape[0]
    px = ds.down2(src, "rgb")
    want = _oracle(orc, px, 0, 12)
    where = dict(pad=13, gap=5, window=(3, 1), margin=(2, 3))
    seen = []
    for fill in (1, 2):
        x, lay, buf = ds.place(torch, src, Cs, "rgb", fill_seed=fill, **where)
        seen.append(buf.cpu().numpy())
        enc = _encoder(W, H, 12, n, lay)
        assert np.array_equal(_bytes_of(torch, enc, x), px), fill
        assert _encode(torch, enc, x, 0) == want, fill
        assert _table(torch, enc, x, (12,)) == ([want[1]], [0]), fill
        assert _rd(torch, enc, x, (12,))[0] == [want[1]], fill
        enc.close()
    # the two allocations differ everywhere but in the colour bytes (tests/test_downscale_cpu.py pins the placement)
    differ = seen[0] != seen[1]
    assert differ.sum() > 0.9 * (len(seen[0]) - src[..., :3].size)
    if Cs == 4:
        x0 = np.lib.stride_tricks.as_strided(differ[ds.geometry(n, 2 * H, 2 * W, 4, **where)[2]:], (n, 2 * H, 2 * W, 4),
                                             ds.geometry(n, 2 * H, 2 * W, 4, **where)[1::-1] + (4, 1))
        assert not x0[..., :3].any() and x0[..., 3].mean() > 0.9


# ---- 3. batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", ds.WIDTHS)
def test_batches(torch_cuda, orc, Cs):
    """9 frames of 48 x 32 (both branches of the workgroup -> (frame, tile) map) at a frame stride with a gap, first_frame_index
    5, at the encoder's quality and at one quality per frame."""
    torch = torch_cuda
    W, H, n, first = 48, 32, 9, 5
    src = _noise((W, H), Cs, n)
    px = ds.down2(src, "bgr")
    x, lay, _ = ds.place(torch, src, Cs, "bgr", gap=5)
    assert lay["frame_stride"] == 2 * H * 2 * W * Cs + 5
    enc = _encoder(W, H, 12, n, lay)
    assert _encode(torch, enc, x, first) == _oracle(orc, px, first, 12)
    qs = [K8[(2 * f + 3) % 8] for f in range(n)]
    want = [_oracle(orc, px[f:f + 1], first + f, qs[f]) for f in range(n)]
    assert _encode(torch, enc, x, first, quality=qs) == (b"".join(w[0] for w in want), [w[1][0] for w in want])
    assert _encode(torch, enc, x[2:7], first + 2) == _oracle(orc, px[2:7], first + 2, 12)
    enc.close()


# ---- 4. the setter ------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_layout_in_force(torch_cuda, orc):
    """Every M1V_E_ARG case of m1v_set_downscale_layout, each with its reason; none changes the layout in force, the table mode
    or the records."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H = 48, 32
    src = _noise((W, H), 4)
    n = src.shape[0]
    want = _oracle(orc, ds.down2(src), 0, 12)
    x, good, _ = ds.place(torch, src, 4, "rgb", pad=13, gap=5)
    P, step = good["row_pitch"], good["pixel_step"]
    assert step == 4 and good["factor"] == 2
    enc = _encoder(W, H, 12, n, good)
    big = 2 ** 40
    extent = (2 * H - 1) * P + 2 * W * step
    bad = [(dict(good, order=2), b"order"), (dict(good, order=-1), b"order"),
           (dict(good, factor=4), b"factor"), (dict(good, factor=0), b"factor"), (dict(good, factor=1), b"factor"),
           (dict(good, pixel_step=2), b"pixel step"), (dict(good, pixel_step=5), b"pixel step"), (dict(good, pixel_step=0), b"pixel step"),
           (dict(good, pixel_step=1), b"pixel step"), (dict(good, pixel_step=8), b"pixel step"),
           (dict(good, row_pitch=2 * W * step - 1), b"row pitch below"), (dict(good, row_pitch=0), b"row pitch below"),
           (dict(good, row_pitch=W * step), b"row pitch below"),                      # the rendition's row, not the source's
           (dict(good, row_pitch=(2 ** 32 - 2 * W * step) // (2 * H - 1) + 1, frame_stride=big), b"4 GiB"),
           (dict(good, row_pitch=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(good, frame_stride=extent - 1), b"frame stride below"), (dict(good, frame_stride=0), b"frame stride below"),
           (dict(good, frame_stride=(H - 1) * P + 2 * W * step), b"frame stride below")]  # the rendition's rows
    for lay, reason in bad:
        assert L.m1v_set_downscale_layout(enc._h, C.byref(_ffi.DownscaleLayout(**lay))) == _ffi.E_ARG, lay
        assert L.m1v_last_error() and reason in L.m1v_last_error(), (lay, L.m1v_last_error())
        assert enc.downscale_layout == good and enc.path == "tiles" and not enc.frame_table and not enc.plane_table
        with pytest.raises(EncoderError):
            enc.set_downscale_layout(lay)
    assert _encode(torch, enc, x, 0) == want
    # the largest extent whose offsets are still 32-bit and the smallest stride are accepted (set, not encoded)
    edge = (2 ** 32 - 1 - 2 * W * step) // (2 * H - 1)
    assert L.m1v_set_downscale_layout(enc._h, C.byref(_ffi.DownscaleLayout(**dict(good, row_pitch=edge, frame_stride=big)))) == 0
    assert L.m1v_set_downscale_layout(enc._h, C.byref(_ffi.DownscaleLayout(**dict(good, frame_stride=extent)))) == 0
    assert enc.downscale_layout == dict(good, frame_stride=extent)
    enc.set_downscale_layout(good)
    # a table that another layout turned on is turned off by this setter, and a failed call leaves it on
    enc.set_rgb_plane_layout("rgb")
    enc.set_plane_table(True)
    assert L.m1v_set_downscale_layout(enc._h, C.byref(_ffi.DownscaleLayout(**dict(good, factor=3)))) == _ffi.E_ARG
    assert enc.plane_table and enc.rgb_plane_layout is not None and enc.downscale_layout is None
    enc.set_downscale_layout(good)
    assert not enc.plane_table and not enc.frame_table and _encode(torch, enc, x, 0) == want
    enc.close()
    odd = Mpeg1Encoder(105, 49, 12, "full", max_frames=n)                                               # an odd width
    lay = _ffi.DownscaleLayout(210 * 3, 98 * 210 * 3, 3, 0, 2)
    assert L.m1v_set_downscale_layout(odd._h, C.byref(lay)) == _ffi.E_ARG and b"even width" in L.m1v_last_error()
    assert odd.downscale_layout is None and odd.input_layout == (0, 0, "rgb")
    odd.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)                                     # channels != 3
    assert L.m1v_set_downscale_layout(rgba._h, C.byref(_ffi.DownscaleLayout(**good))) == _ffi.E_ARG
    assert b"3 channels" in L.m1v_last_error() and rgba.downscale_layout is None and rgba.path == "runs"
    rgba.close()
    assert L.m1v_set_downscale_layout(None, C.byref(_ffi.DownscaleLayout(**good))) == _ffi.E_ARG         # a null encoder
    assert L.m1v_last_error()
    forced = Mpeg1Encoder(W, H, 12, "full", max_frames=n)                                               # the run-kernel hooks
    forced.debug_set_path("runs")
    assert L.m1v_set_downscale_layout(forced._h, C.byref(_ffi.DownscaleLayout(**good))) == _ffi.E_ARG
    assert b"hook" in L.m1v_last_error() and forced.downscale_layout is None and forced.path == "runs"
    forced.debug_set_path("auto")
    forced.set_downscale_layout(good)
    for hook in (lambda: forced.debug_set_path("runs"), lambda: forced.debug_set_input_mode(0)):
        with pytest.raises(EncoderError) as ei:
            hook()
        assert ei.value.code == _ffi.E_ARG and "downscale layout" in str(ei.value)
        assert forced.path == "tiles" and forced.downscale_layout == good
    assert _encode(torch, forced, x, 0) == want
    forced.close()


def test_setters_getters_tables_and_packed_only_calls(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H = 96, 80
    src = _noise((W, H), 4)
    n = src.shape[0]
    px = ds.down2(src, "bgr")
    want = _oracle(orc, px, 5, 12)
    x, lay, _ = ds.place(torch, src, 4, "bgr")
    packed = torch.from_numpy(px).cuda()
    planar = torch.from_numpy(np.ascontiguousarray(px.transpose(0, 3, 1, 2))).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    fresh = (enc.path, enc.size_table_fused, enc.scratch_bytes())
    assert enc.downscale_layout is None and L.m1v_downscale_layout_in_force(enc._h, None) == 0
    others = ((lambda: enc.set_rgb_plane_layout("rgb"), planar), (lambda: enc.set_input_layout(W * 3, 0, "bgr"), None),
              (lambda: enc.set_plane_layout("i420"), None), (lambda: enc.set_sample_layout("yuy2"), None))
    for set_other, tensor in others:
        enc.set_downscale_layout(lay)                                       # ... -> downscale
        assert enc.downscale_layout == lay and enc.rgb_plane_layout is None and enc.float_plane_layout is None
        assert enc.float_pixel_layout is None and L.m1v_downscale_layout_in_force(enc._h, None) == 1
        assert _encode(torch, enc, x, 5) == want
        for query in (lambda: enc.plane_layout, lambda: enc.sample_layout, lambda: enc.input_layout):
            with pytest.raises(EncoderError) as ei:
                query()
            assert ei.value.code == _ffi.E_ARG and "ask m1v_downscale_layout_in_force" in str(ei.value)
        set_other()                                                         # downscale -> each other layout
        assert enc.downscale_layout is None
        if tensor is not None:
            assert _encode(torch, enc, tensor, 5) == want
    enc.set_downscale_layout(lay)
    # the table modes refuse this kind, with a reason of their own, and stay off
    for setter in ("m1v_set_frame_table", "m1v_set_plane_table"):
        assert getattr(L, setter)(enc._h, 1) == _ffi.E_ARG
        assert b"downscale layout" in L.m1v_last_error() and b"not covered" in L.m1v_last_error()
        assert getattr(L, setter)(enc._h, 0) == _ffi.OK
    assert not enc.frame_table and not enc.plane_table
    with pytest.raises(AssertionError, match="downscale layout"):
        enc.frames([x[0]])
    with pytest.raises(AssertionError, match="downscale layout"):
        enc.plane_frames([(x[0], x[0], x[0])])
    # packed-only entry points refuse, naming the layout
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(px)):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG and "downscale layout" in str(ei.value)
    # Python holds the tensor against the layout: the rendition's own size, another pitch and a float tensor are refused
    for wrong in (packed, x[:, :, :2 * W - 2], x.float()):
        with pytest.raises(AssertionError):
            enc.encode(wrong)
    enc.set_downscale_layout(None)                                          # downscale -> default: a fresh encoder's plan
    assert enc.downscale_layout is None and enc.input_layout == (0, 0, "rgb")
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes()) == fresh
    assert _encode(torch, enc, packed, 5) == want
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")       # the bytes call needs the layout
    assert L.m1v_downscale_to_bytes_device(enc._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == _ffi.E_ARG
    assert b"m1v_set_downscale_layout" in L.m1v_last_error()
    enc.close()


# ---- 5. every served call once ------------------------------------------------------------------------------------------------------
def _pair(torch, Cs, n, order="bgr"):
    """(the encoder with the layout in force, its source view, a default packed encoder, the bytes) at 48 x 32."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H = 48, 32
    src = _noise((W, H), Cs, n)
    xa, lay, _ = ds.place(torch, src, Cs, order, pad=13, gap=5, window=(3, 1), margin=(2, 3))
    a = _encoder(W, H, 12, n, lay)
    xb = a.downscale_to_bytes(xa)
    torch.cuda.synchronize()
    px = ds.down2(src, order)
    assert np.array_equal(xb.cpu().numpy(), px)
    return a, xa, Mpeg1Encoder(W, H, 12, "full", max_frames=n), xb, px, lay


@pytest.mark.parametrize("Cs", ds.WIDTHS)
def test_tables_against_the_oracles(torch_cuda, orc, Cs):
    """The size table and the rd table at K = 8 on 4 frames: the oracle's sizes and tests/rd_oracle.py's distortion."""
    torch = torch_cuda
    a, xa, b, xb, px, _ = _pair(torch, Cs, 4)
    sizes = [_oracle(orc, px, 0, q)[1] for q in K8]
    dist = [[rd.frame_distortion(orc, px[f], 48, 32, q, orc.MODE_FULL, 3) for f in range(4)] for q in K8]
    assert _table(torch, a, xa, K8) == (sizes, [0] * 8)
    assert _rd(torch, a, xa, K8) == (sizes, dist, [0] * 8)
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    s = a.frame_sizes(xa, status=st)
    a.flush()
    torch.cuda.synchronize()
    assert ([int(v) for v in s.cpu()], int(st.cpu()[0])) == (sizes[-1], 0)
    a.close()
    b.close()


@pytest.mark.parametrize("Cs", ds.WIDTHS)
def test_rate_calls_equal_the_packed_layout_on_the_bytes(torch_cuda, Cs):
    """One budget encode, one rd encode, one bitrate encode and one streams call (with a bucket per stream and a budget per
    stream), with limits from the rd table so that the picks differ between frames."""
    torch = torch_cuda
    n, first = 4, 40
    a, xa, b, xb, _, _ = _pair(torch, Cs, n)

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
    spans = [(1, 7), (3, 0)]
    assert len(both(lambda e, x: e.encode_streams(x, spans))[1]) == n

    def streams_cbr(e, x):
        levels = torch.full((2,), 2 * cap, dtype=torch.int64, device="cuda")
        return e.encode_streams_at_bitrate(x, spans, CANDS, cap, 2 * cap, levels), [int(v) for v in levels.cpu()]

    both(streams_cbr)
    both(lambda e, x: e.encode_streams_to_budget(x, spans, CANDS, [cap, 3 * cap]))
    a.close()
    b.close()


@pytest.mark.parametrize("Cs", ds.WIDTHS)
def test_pipelined_delivery_and_fallback_equal_the_packed_layout(torch_cuda, Cs):
    """Pipelined mode, HostDelivery.step (with its scratch retry: the arena is not reserved and the LDS image is 8 words, so the
    first attempt runs out of scratch), the global-memory fallback with the worst-case arena reserved, the profile counters."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    n, first = 4, 40
    a, xa, b, xb, _, lay = _pair(torch, Cs, n, order="rgb")
    qs = [3, 12, 7, 9]

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
    assert a.downscale_layout == lay
    assert both(lambda e, x: (_encode(torch, e, x, first), _encode(torch, e, x[1:4], first + 1, quality=qs[1:4]),
                              _table(torch, e, x, K8)))[0] == plain
    for e in (a, b):
        e.set_pipelined(False)
        e.profile(True)
    both(lambda e, x: (_encode(torch, e, x, first), e.profile_read()[0]))        # (launches; the milliseconds differ)
    a.close()
    b.close()


def test_python_takes_contiguous_tensors_windows_and_channels_last_views(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder, downscale_layout_preset, downscale_strides
    torch = torch_cuda
    W, H, n = 48, 32, 2
    src = _noise((W, H), 4, n)
    x = torch.from_numpy(src.copy()).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    enc.set_downscale_layout(downscale_layout_preset(W, H, 4))
    want = _oracle(orc, ds.down2(src), 0, 12)
    assert _encode(torch, enc, x, 0) == want
    assert _encode(torch, enc, x.permute(0, 3, 1, 2), 0) == want            # the channels-last view of the same memory
    assert _encode(torch, enc, x[:1], 0) == _oracle(orc, ds.down2(src[:1]), 0, 12)
    # the quarter of the surface that starts at source pixel (W, H), three of its four bytes, as the source of a 24 x 16 rendition
    win = x[:, H:H + H, W:W + W, :3]
    half = Mpeg1Encoder(W // 2, H // 2, 12, "full", max_frames=n)
    half.set_downscale_layout(downscale_strides(tuple(win.shape), tuple(win.stride()), "nhwc", "bgr"))
    assert _encode(torch, half, win, 0) == _oracle(orc, ds.down2(src[:, H:2 * H, W:2 * W], "bgr"), 0, 12)
    enc.close()
    half.close()
