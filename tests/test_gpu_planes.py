"""GPU tests of the plane input layout (m1v_set_plane_layout; k_encode_planes, k_size_table_planes; -m gpu): frames that are
Y, Cb, Cr planes on the device — the reference's own planes, I420 / YV12, NV12 / NV21, pitched and windowed variants — encoded
without a colour conversion.

Two checkers.  Planes that are the image of an RGB picture (orc.convert) must give the oracle's RGB records of that picture:
the reference cuts its chroma blocks from the full-resolution planes addressed with stride W / 2, and a layout's chroma plane
here holds exactly the samples that addressing reaches (the first (ye / 2) rows of W / 2 samples).  Planes that no RGB picture
maps to are checked against tests/plane_oracle.py (pinned to the oracle by tests/test_planes_abi.py).  A frame buffer is device
noise into which only the samples the definition addresses are written; every comparison is for equality and every status word
is 0 unless a case says otherwise."""
import numpy as np
import pytest

import plane_oracle
from gpu_calls import _encode, _frame_rule, _frames, _mixed_frames, _oracle, _oracle_on_buffer, _oracle_sizes, _table
from layout_inputs import PRESETS, _buffer, _layout, _plane_encoder, _planes_of, _region, _view, _write_planes
from rate_rules import batch_rule, cbr_rule
from table_cases import RGB_CASES, SEQUENCE, RateMixed
from table_cases import MATRIX as SURFACE_MATRIX

pytestmark = pytest.mark.gpu

LAYOUTS = PRESETS + ("pitched", "odd", "window")
# the surface matrix (3-channel side) with the odd-width case kept: a plane layout takes odd widths
MATRIX = dict(SURFACE_MATRIX)
MATRIX["tiny_105x49"] = RGB_CASES["tiny_105x49"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- 1. the parity matrix ---------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _expected(orc, case):
    if case not in _oracle_cache:
        W, H, Q, mode, n, amps, quals = MATRIX[case]
        rng = np.random.default_rng(sum(map(ord, case)) + 3)
        px = _mixed_frames(rng, n, W, H, 3, amps)
        m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
        first = 17
        qs = sorted(set(quals) | {Q})
        recs = {q: [orc.encode_frame(px[f], W, H, first + f, q, m) for f in range(n)] for q in qs}   # (asserts encodable)
        _oracle_cache[case] = (px, first, recs)
    return _oracle_cache[case]


def _matrix_params():
    for case in sorted(MATRIX):
        W, H = MATRIX[case][:2]
        for layout in LAYOUTS:
            if (W % 2 or H % 2) and layout in PRESETS[1:]:
                continue                        # the 4:2:0 presets are defined for even sizes (test_planes_abi.py)
            yield case, layout


@pytest.mark.parametrize("case,layout", list(_matrix_params()))
def test_parity_matrix(torch_cuda, orc, case, layout):
    """encode, encode(quality=per frame), frame_sizes and frame_size_table on planes converted from RGB frames: the oracle's
    RGB records."""
    torch = torch_cuda
    W, H, Q, mode, n, amps, quals = MATRIX[case]
    px, first, recs = _expected(orc, case)
    buf, lay, base = _planes_of(torch, orc, px, mode, layout, fill_seed=len(case))
    enc = _plane_encoder(W, H, Q, mode, n, lay)
    dev = _view(torch, buf, n, lay, base, enc)
    if layout == "odd":
        assert dev.data_ptr() % 2 == 1
    got, sizes = _encode(torch, enc, dev, first)
    assert sizes == [len(r) for r in recs[Q]]
    assert got == b"".join(recs[Q])
    qs = [quals[(f + 1) % len(quals)] for f in range(n)]
    got, sizes = _encode(torch, enc, dev, first, quality=qs)
    assert sizes == [len(recs[q][f]) for f, q in enumerate(qs)]
    assert got == b"".join(recs[q][f] for f, q in enumerate(qs))
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    probe = enc.frame_sizes(dev, quality=qs, status=st)
    enc.flush()
    torch.cuda.synchronize()
    assert [int(s) for s in probe.cpu()] == sizes and int(st.cpu()[0]) == 0
    table, status = _table(torch, enc, dev, quals)
    assert status == [0] * len(quals), status
    assert table == [[len(r) for r in recs[q]] for q in quals]
    enc.close()


# ---- 2. planes that are the image of no RGB picture -------------------------------------------------------------------------
def _independent(W, H, n, seed):
    """Unrelated planes: noise, gradients and a gentle plane in turn, different per plane and frame."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]

    def plane(kind, h, w):
        if kind == 0:
            return rng.integers(0, 256, (h, w), dtype=np.uint8)
        if kind == 1:
            return ((xx[:h, :w] * 5 + yy[:h, :w] * 3 + int(rng.integers(0, 256))) % 256).astype(np.uint8)
        return (100 + rng.integers(0, 30, (h, w))).astype(np.uint8)

    Y = np.stack([plane(f % 3, H, W) for f in range(n)])
    Cb = np.stack([plane((f + 1) % 3, H // 2, W // 2) for f in range(n)])
    Cr = np.stack([plane((f + 2) % 3, H // 2, W // 2) for f in range(n)])
    return Y, Cb, Cr


@pytest.mark.parametrize("layout", PRESETS)
@pytest.mark.parametrize("W,H", [(96, 48), (366, 216)])
def test_independent_planes(torch_cuda, orc, W, H, layout):
    torch = torch_cuda
    n, Q, first = 3, 12, 5
    lay, base = _layout(layout, W, H)
    buf = _buffer(torch, n, lay, base, W)
    xe, ye = _region(W, H, "full")
    Y, Cb, Cr = _independent(W, H, n, seed=W + len(layout))
    _write_planes(torch, buf, lay, base, Y[:, :ye, :xe], Cb[:, :ye // 2, :xe // 2], Cr[:, :ye // 2, :xe // 2])
    want = _oracle_on_buffer(orc, buf, n, lay, base, W, H, first, [Q] * n, orc.MODE_FULL)
    enc = _plane_encoder(W, H, Q, "full", n, lay)
    dev = _view(torch, buf, n, lay, base, enc)
    got, sizes = _encode(torch, enc, dev, first)
    assert sizes == [len(r) for r in want] and got == b"".join(want)
    quals = (3, 12)
    table, status = _table(torch, enc, dev, quals)
    assert status == [0, 0]
    assert table == [[len(r) for r in _oracle_on_buffer(orc, buf, n, lay, base, W, H, 0, [q] * n, orc.MODE_FULL)] for q in quals]
    enc.close()


# ---- 3. every byte value in every plane -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_every_byte_value_in_every_plane(torch_cuda, orc, layout):
    """Flat 8x8 cells of all 256 values at quality 50 (the DC level is the byte), frame p varying plane p."""
    torch = torch_cuda
    W = H = 256
    n, Q = 3, 50
    lay, base = _layout(layout, W, H)
    buf = _buffer(torch, n, lay, base, 9)
    cells = lambda k: (np.arange(k * k).reshape(k, k) % 256).astype(np.uint8).repeat(8, axis=0).repeat(8, axis=1)
    Y = np.full((n, H, W), 128, np.uint8)
    Cb = np.full((n, H // 2, W // 2), 128, np.uint8)
    Cr = np.full((n, H // 2, W // 2), 128, np.uint8)
    Y[0], Cb[1], Cr[2] = cells(32), cells(16), cells(16)
    assert all(len(np.unique(p)) == 256 for p in (Y[0], Cb[1], Cr[2]))
    _write_planes(torch, buf, lay, base, Y, Cb, Cr)
    want = _oracle_on_buffer(orc, buf, n, lay, base, W, H, 0, [Q] * n, orc.MODE_FULL)
    enc = _plane_encoder(W, H, Q, "full", n, lay)
    got, sizes = _encode(torch, enc, _view(torch, buf, n, lay, base, enc), 0)
    assert sizes == [len(r) for r in want] and got == b"".join(want)
    enc.close()


# ---- 4. the device chain: convert, then encode the planes ----------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1920, 1080), (3840, 2160), (366, 216)])
def test_device_chain_ab(torch_cuda, W, H):
    """enc.encode(x) equals planes.encode(enc.convert(x).view(n, -1)): no host data in between."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    n = 2
    rgb_enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    x = rgb_enc.synth(n, seed=77)
    a = _encode(torch, rgb_enc, x, 4)
    planes = rgb_enc.convert(x).view(n, -1)
    enc = _plane_encoder(W, H, 12, "full", n, _layout("reference", W, H)[0])
    b = _encode(torch, enc, planes, 4)
    assert a == b
    assert _table(torch, rgb_enc, x, (2, 7, 12)) == _table(torch, enc, planes, (2, 7, 12))
    enc.close()
    rgb_enc.close()


# ---- 5. every call ------------------------------------------------------------------------------------------------------------
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
CANDS5 = (2, 4, 6, 8, 12)


@pytest.mark.parametrize("layout", ["nv12", "pitched"])
def test_every_call(torch_cuda, orc, layout):
    """Per-frame quality, frame_sizes, a K = 8 table, budget, batch budget and bitrate (one size-table pass + one encode = 2
    profiled launches each; a bitrate stream continued over two calls equals one call): the rules of tests/test_rate_abi.py
    on the oracle's sizes, the oracle's records at the picked qualities."""
    torch = torch_cuda
    n, W, H, first = 6, 352, 288, 40
    rng = np.random.default_rng(101 + len(layout))
    px = _mixed_frames(rng, n, W, H, 3)
    buf, lay, base = _planes_of(torch, orc, px, "full", layout, fill_seed=3)
    enc = _plane_encoder(W, H, 12, "full", n, lay)
    dev = _view(torch, buf, n, lay, base, enc)
    qs = [int(q) for q in rng.integers(1, 13, n)]
    assert _encode(torch, enc, dev, first, quality=qs) == _oracle(orc, px, first, qs, orc.MODE_FULL, 3)
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    probe = enc.frame_sizes(dev, quality=qs, status=st)
    enc.flush()
    torch.cuda.synchronize()
    assert [int(s) for s in probe.cpu()] == _oracle(orc, px, first, qs, orc.MODE_FULL, 3)[1] and int(st.cpu()[0]) == 0
    enc.profile(True)
    table, status = _table(torch, enc, dev, K8)
    launches, _ = enc.profile_read()
    enc.profile(False)
    assert launches == 1 and status == [0] * 8
    assert table == [_oracle_sizes(orc, px, orc.MODE_FULL, q, 3) for q in K8]
    s = [_oracle_sizes(orc, px, orc.MODE_FULL, c, 3) for c in CANDS5]
    level = torch.full((1,), 10 ** 6, dtype=torch.int64, device="cuda")
    r = sorted(s[2])[2]
    for call in ("budget", "batch", "cbr"):
        enc.profile(True)
        if call == "budget":
            cap = sorted(x for row in s for x in row)[len(s) * n // 2]
            got, sizes, ch, ov = enc.encode_to_budget(dev, cap, CANDS5, first_frame_index=first)
            pick, over = _frame_rule(s, cap)
            assert len(set(pick)) > 1, pick
        elif call == "batch":
            B = (sum(s[1]) + sum(s[2])) // 2
            got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, CANDS5, first_frame_index=first)
            pick, over = batch_rule(s, B)
        else:
            got, sizes, ch, ov = enc.encode_at_bitrate(dev, r, 2 * r, CANDS5, level, first_frame_index=first)
            pick, over, lvl = cbr_rule(s, r, 2 * r, 10 ** 6)
            assert int(level.cpu()[0]) == lvl
        launches, _ = enc.profile_read()
        enc.profile(False)
        assert launches == 2, (call, launches)
        chosen = [CANDS5[k] for k in pick]
        want, wsizes = _oracle(orc, px, first, chosen, orc.MODE_FULL, 3)
        assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), call
    one = (got, sizes, ch, ov, int(level.cpu()[0]))
    level.fill_(10 ** 6)
    a = enc.encode_at_bitrate(dev[:4], r, 2 * r, CANDS5, level, first_frame_index=first)
    b = enc.encode_at_bitrate(dev[4:], r, 2 * r, CANDS5, level, first_frame_index=first + 4)
    assert (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + [f + 4 for f in b[3]], int(level.cpu()[0])) == one
    enc.close()


class _PlaneUploads:
    """torch as RateMixed sees it: from_numpy(frames).cuda() converts a batch of the encoder's RGB frames to planes in the
    layout, over fresh noise, and returns the [n, L] view; everything else is torch's.  RateMixed computes its expectations
    from the RGB frames it made."""

    def __init__(self, torch, orc, enc, layout, tail):
        self._torch, self._orc, self._enc, self._layout, self._tail, self._fills = torch, orc, enc, layout, tuple(tail), 0

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def from_numpy(self, arr):
        outer = self

        class _Upload:
            def cuda(self):
                if arr.dtype != np.uint8 or arr.ndim != 4 or tuple(arr.shape[1:]) != outer._tail:
                    return outer._torch.from_numpy(arr).cuda()
                outer._fills += 1
                buf, lay, base = _planes_of(outer._torch, outer._orc, arr, "full", outer._layout, fill_seed=outer._fills)
                return _view(outer._torch, buf, arr.shape[0], lay, base, outer._enc)

        return _Upload()


@pytest.mark.parametrize("layout", ["nv12", "pitched"])
def test_interleaved_calls_in_pipelined_mode(torch_cuda, orc, layout):
    """SEQUENCE of tests/test_gpu_rate.py (plain, per-frame, probe, table, budget, batch-budget and bitrate calls) twice on a
    pipelined plane encoder."""
    W, H = 352, 288
    enc = _plane_encoder(W, H, 12, "full", 5, _layout(layout, W, H)[0], pipelined=True)
    calls = RateMixed(_PlaneUploads(torch_cuda, orc, enc, layout, (H, W, 3)), orc, enc, seed=960 + len(layout))
    for _ in range(2):
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("sequence", layout))
    enc.close()


@pytest.mark.parametrize("layout", ["nv12", "pitched"])
def test_host_delivery_of_plane_batches(torch_cuda, orc, layout):
    """m1v_delivery_* through the Python mirror: three batches of planes arrive as the oracle's streams."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n = 352, 288, 4
    rng = np.random.default_rng(12 + len(layout))
    batches = [(_frames(rng, n, W, H, 3), 50 * k + 3) for k in range(3)]
    lay = _layout(layout, W, H)[0]
    enc = _plane_encoder(W, H, 12, "full", n, lay)
    views = []
    for k, (px, _) in enumerate(batches):
        buf, lay_k, base = _planes_of(torch, orc, px, "full", layout, fill_seed=k)
        views.append(_view(torch, buf, n, lay_k, base, enc))
    hd = HostDelivery(enc, n)
    got = []

    def take():
        hd.delivered[hd.last[0]].synchronize()
        got.append((bytes(hd.result().numpy()), [int(x) for x in hd.frame_sizes(n)]))

    hd.step(views[0], batches[0][1])
    assert hd.last is None
    hd.step(views[1], batches[1][1])
    take()
    hd.step(views[2], batches[2][1])
    take()
    hd.fence()
    take()
    for (blob, sizes), (px, first) in zip(got, batches):
        assert (blob, sizes) == _oracle(orc, px, first, [12] * n, orc.MODE_FULL, 3), first
    hd.close()
    enc.close()


# ---- 6. padding is never used -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,layout", [
    ("odd_last_column_176x208", "i420"),        # tightly packed, 3 strips in the last tile column: the last chroma unit of a row
                                                # would reach past the frame's extent in the last row of the last plane
    ("odd_last_column_176x208", "nv12"), ("odd_last_column_176x208", "odd"), ("partial_tiles_366x216", "reference"),
    ("partial_tiles_366x216", "pitched"), ("partial_tiles_366x216", "window"), ("cif_strict_k1", "nv21"),
    ("cif_strict_k1", "yv12"), ("tiny_105x49", "odd"), ("tiny_105x49", "window")])
def test_padding_is_never_used(torch_cuda, orc, case, layout):
    """The same addressed samples under two different fills of every other byte (row padding, gaps between planes and frames,
    the surroundings of a window, columns and rows outside the region, the rest of an interleaved plane): identical records,
    sizes and tables."""
    torch = torch_cuda
    W, H, Q, mode, n, amps, quals = MATRIX[case]
    px = _mixed_frames(np.random.default_rng(5), n, W, H, 3, amps)
    results = []
    for fill in (1, 2):
        buf, lay, base = _planes_of(torch, orc, px, mode, layout, fill_seed=fill)
        enc = _plane_encoder(W, H, Q, mode, n, lay)
        dev = _view(torch, buf, n, lay, base, enc)
        results.append((_encode(torch, enc, dev, 3), _table(torch, enc, dev, quals)))
        enc.close()
    assert results[0] == results[1]
    assert results[0][1][1] == [0] * len(quals)
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    assert results[0][0] == _oracle(orc, px, 3, [Q] * n, m, 3)


# ---- 7. status --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["luma", "cb"])
@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_unencodable_level_is_reported(torch_cuda, orc, layout, which):
    """A plane of 255 / 0 in bands of four rows: at quality 92 a block has an AC level the VLC cannot code (plane_oracle returns
    the oracle's ORC_E_UNENCODABLE), at 76 it codes.  Luma and chroma blocks take the same path."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    W, H, n = 96, 48, 1
    lay, base = _layout(layout, W, H)
    buf = _buffer(torch, n, lay, base, 4)
    bands = lambda h, w: np.where((np.arange(h)[:, None] % 8) < 4, 255, 0).astype(np.uint8).repeat(w, axis=1)[None]
    flat = lambda h, w: np.full((1, h, w), 128, np.uint8)
    Y = bands(H, W) if which == "luma" else flat(H, W)
    Cb = bands(H // 2, W // 2) if which == "cb" else flat(H // 2, W // 2)
    _write_planes(torch, buf, lay, base, Y, Cb, flat(H // 2, W // 2))
    host = buf.cpu().numpy()[base:]
    with pytest.raises(plane_oracle.Unencodable):
        plane_oracle.encode_layout(host, lay, W, H, 0, 92, orc.MODE_FULL)
    ok76 = plane_oracle.encode_layout(host, lay, W, H, 0, 76, orc.MODE_FULL)
    enc = _plane_encoder(W, H, 92, "full", n, lay)
    dev = _view(torch, buf, n, lay, base, enc)
    out = torch.empty(enc.frame_bound, dtype=torch.uint8, device="cuda")
    _, _, meta = enc.encode(dev, 0, out=out)
    enc.flush()
    torch.cuda.synchronize()
    assert int(meta.cpu()[1]) & 0xFFFFFFFF == _ffi.STATUS_UNENCODABLE
    table, status = _table(torch, enc, dev, (76, 92))
    assert status == [0, _ffi.STATUS_UNENCODABLE]
    assert table[0] == [len(ok76)]
    assert _encode(torch, enc, dev, 0, quality=[76]) == (ok76, [len(ok76)])
    enc.close()


# ---- 8. reconfiguration -----------------------------------------------------------------------------------------------------
def test_plane_surface_and_default_layouts_replace_each_other(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 4
    px = _mixed_frames(np.random.default_rng(55), n, W, H, 3)
    packed = torch.from_numpy(px).cuda()
    want = _oracle(orc, px, 5, [12] * n, orc.MODE_FULL, 3)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    assert enc.plane_layout is None and enc.path == "tiles"
    assert _encode(torch, enc, packed, 5) == want
    buf, lay, base = _planes_of(torch, orc, px, "full", "nv12")
    enc.set_plane_layout("nv12")
    assert enc.plane_layout == lay and enc.path == "tiles" and enc.size_table_fused == 1
    with pytest.raises(EncoderError) as ei:
        enc.input_layout
    assert ei.value.code == _ffi.E_ARG and "m1v_plane_layout_in_force" in str(ei.value)
    dev = _view(torch, buf, n, lay, base, enc)
    assert _encode(torch, enc, dev, 5) == want
    with pytest.raises(AssertionError):
        enc.encode(packed)                                          # [n, H, W, 3] is not a plane tensor
    enc.set_plane_layout(None)                                      # plane -> default
    assert enc.plane_layout is None and enc.input_layout == (0, 0, "rgb") and enc.path == "tiles" and enc.size_table_fused == 1
    assert _encode(torch, enc, packed, 5) == want
    enc.set_plane_layout(lay)
    enc.set_input_layout(W * 3 + 64, 0, "rgb")                      # plane -> surface
    assert enc.plane_layout is None and enc.input_layout == (W * 3 + 64, H * (W * 3 + 64), "rgb")
    surf = torch.zeros((n, H, W * 3 + 64), dtype=torch.uint8, device="cuda")
    view = torch.as_strided(surf, (n, H, W, 3), (H * (W * 3 + 64), W * 3 + 64, 3, 1))
    view.copy_(packed)
    assert _encode(torch, enc, view, 5) == want
    enc.set_plane_layout("nv12")                                    # surface -> plane
    assert enc.plane_layout == lay
    assert _encode(torch, enc, dev, 5) == want
    enc.set_input_layout()                                          # plane -> default, by the other call
    assert enc.plane_layout is None and enc.input_layout == (0, 0, "rgb")
    assert _encode(torch, enc, packed, 5) == want
    enc.close()


def test_argument_errors_leave_the_encoder_usable(torch_cuda, orc):
    """Every M1V_E_ARG case of m1v_set_plane_layout; none of them changes the layout in force or the bytes."""
    import ctypes as C
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 352, 288, 2
    px = _mixed_frames(np.random.default_rng(56), n, W, H, 3)
    want = _oracle(orc, px, 0, [12] * n, orc.MODE_FULL, 3)
    buf, good, base = _planes_of(torch, orc, px, "full", "pitched")
    enc = _plane_encoder(W, H, 12, "full", n, good)
    dev = _view(torch, buf, n, good, base, enc)
    extent = good["cr_offset"] + (H // 2 - 1) * good["c_pitch"] + W // 2
    bad = [dict(good, c_step=3), dict(good, c_step=7), dict(good, frame_stride=0), dict(good, y_pitch=W - 1), dict(good, y_pitch=1),
           dict(good, c_pitch=W // 2 - 1), dict(good, c_step=2, c_pitch=W - 1), dict(good, frame_stride=extent - 1),
           dict(good, y_offset=2 ** 32), dict(good, cr_offset=2 ** 32 - 100, frame_stride=2 ** 40),
           dict(good, y_pitch=2 ** 32 // (H - 1) + 1, frame_stride=2 ** 40), dict(good, c_pitch=2 ** 33, frame_stride=2 ** 50)]
    for lay in bad:
        c = _ffi.PlaneLayout(**lay)
        assert L.m1v_set_plane_layout(enc._h, C.byref(c)) == _ffi.E_ARG, lay
        assert enc.plane_layout == good and enc.path == "tiles"
    assert L.m1v_set_plane_layout(enc._h, C.byref(_ffi.PlaneLayout(**dict(good, frame_stride=extent)))) == 0   # the smallest stride
    enc.set_plane_layout(good)
    assert _encode(torch, enc, dev, 0) == want
    enc.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)
    assert L.m1v_set_plane_layout(rgba._h, C.byref(_ffi.PlaneLayout(**good))) == _ffi.E_ARG             # channels != 3
    assert rgba.plane_layout is None and rgba.path == "runs"
    assert L.m1v_set_plane_layout(rgba._h, None) == 0
    rgba.close()


def test_injected_allocation_failure_changes_nothing(torch_cuda, orc):
    """m1v_debug_fail_alloc reaches m1v_set_plane_layout (configure_path), and a reconfiguration of a plane encoder that fails
    in an allocation leaves layout, plan, scratch and bytes as they were.  A 3-channel encoder's plane plan is its default tile
    plan, so set_plane_layout itself may find nothing to allocate: then it succeeds with the hook armed; if it does allocate
    it fails with M1V_E_HIP and changes nothing.  reserve_scratch and set_pipelined always allocate."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 4
    px = _mixed_frames(np.random.default_rng(57), n, W, H, 3)
    packed = torch.from_numpy(px).cuda()
    want = _oracle(orc, px, 5, [12] * n, orc.MODE_FULL, 3)
    buf, lay, base = _planes_of(torch, orc, px, "full", "i420")
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)

    def armed(call):
        """call() with the next allocation failing -> None, or the error code; state unchanged after an error."""
        before = (enc.plane_layout, enc.path, enc.scratch_bytes())
        _ffi.lib().m1v_debug_fail_alloc(1)
        try:
            call()
            rc = None
        except EncoderError as e:
            rc = e.code
        finally:
            _ffi.lib().m1v_debug_fail_alloc(0)
        if rc is not None:
            assert rc == _ffi.E_HIP and (enc.plane_layout, enc.path, enc.scratch_bytes()) == before
        return rc

    if armed(lambda: enc.set_plane_layout(lay)) is not None:
        assert enc.plane_layout is None and _encode(torch, enc, packed, 5) == want
        enc.set_plane_layout(lay)
    dev = _view(torch, buf, n, lay, base, enc)
    assert enc.plane_layout == lay and _encode(torch, enc, dev, 5) == want
    assert armed(lambda: enc.reserve_scratch(True)) == _ffi.E_HIP
    assert enc.plane_layout == lay and _encode(torch, enc, dev, 5) == want
    assert armed(lambda: enc.set_pipelined(True)) == _ffi.E_HIP
    assert enc.plane_layout == lay and _encode(torch, enc, dev, 5) == want
    enc.reserve_scratch(True)
    assert enc.plane_layout == lay and _encode(torch, enc, dev, 5) == want
    if armed(lambda: enc.set_plane_layout(None)) is not None:
        assert enc.plane_layout == lay and _encode(torch, enc, dev, 5) == want
        enc.set_plane_layout(None)
    assert enc.plane_layout is None and _encode(torch, enc, packed, 5) == want
    enc.close()


def test_hooks_and_plane_layouts_refuse_each_other(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    W, H = 352, 288
    forcing = {"path": lambda e: e.debug_set_path("runs"), "input mode": lambda e: e.debug_set_input_mode(0),
               "funnel": lambda e: e.debug_set_input_mode(2), "run length": lambda e: e.debug_set_dense_threads(64)}
    undo = {"path": lambda e: e.debug_set_path("auto"), "input mode": lambda e: e.debug_set_input_mode(-1),
            "funnel": lambda e: e.debug_set_input_mode(-1), "run length": lambda e: e.debug_set_dense_threads(0)}
    lay = _layout("nv12", W, H)[0]
    for name, force in forcing.items():
        enc = Mpeg1Encoder(W, H, 12, "full", max_frames=2)
        force(enc)
        assert enc.path == "runs"
        with pytest.raises(EncoderError) as ei:
            enc.set_plane_layout("nv12")
        assert ei.value.code == _ffi.E_ARG and enc.plane_layout is None and enc.path == "runs"
        enc.set_plane_layout(None)                                  # the default layout is always accepted
        undo[name](enc)
        enc.set_plane_layout("nv12")
        with pytest.raises(EncoderError) as ei:
            force(enc)
        assert ei.value.code == _ffi.E_ARG, name
        assert enc.path == "tiles" and enc.plane_layout == lay
        undo[name](enc)
        assert enc.path == "tiles" and enc.plane_layout == lay
        enc.close()


def test_packed_only_entry_points_refuse_a_plane_encoder(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 2
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    dev = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    host = np.zeros((n, H, W, 3), np.uint8)
    planes = np.zeros((n, 3, H * W), np.uint8)
    enc.set_plane_layout("reference")
    for call in (lambda: enc.coefficients(dev), lambda: enc.convert(dev), lambda: enc.encode_host(host),
                 lambda: enc.encode_host(host, with_planes=True)):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG
    assert _ffi.lib().m1v_convert_host(enc._h, host.ctypes.data, n, planes.ctypes.data) == _ffi.E_ARG
    enc.set_plane_layout(None)
    assert enc.convert(dev).shape == (n, 3, H * W)
    assert len(enc.encode_host(host)[1]) == n
    enc.close()


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_forced_small_lds_image_and_reserved_scratch(torch_cuda, orc, layout):
    """An 8-word LDS image sends every tile to the overflow arena: M1V_STATUS_SCRATCH with the default arena, the oracle's bytes
    once the worst case is reserved; then the default image again."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 5
    px = _frames(np.random.default_rng(77), n, W, H, 3)
    buf, lay, base = _planes_of(torch, orc, px, "full", layout, fill_seed=4)
    enc = _plane_encoder(W, H, 12, "full", n, lay)
    dev = _view(torch, buf, n, lay, base, enc)
    want = _oracle(orc, px, 21, [12] * n, orc.MODE_FULL, 3)
    enc.debug_set_lds_words(8)
    assert enc.path == "tiles" and enc.plane_layout == lay
    out, sizes, meta = enc.encode(dev, 21)
    torch.cuda.synchronize()
    assert int(meta.cpu()[1]) & 0xFFFFFFFF == _ffi.STATUS_SCRATCH
    enc.reserve_scratch(True)
    assert enc.path == "tiles" and enc.plane_layout == lay
    assert _encode(torch, enc, dev, 21) == want
    enc.debug_set_lds_words(0)
    enc.reserve_scratch(False)
    assert _encode(torch, enc, dev, 21) == want
    enc.close()


def test_python_checks_the_tensor_against_the_layout(torch_cuda):
    from ec504_imageencoder_amd import Mpeg1Encoder
    from ec504_imageencoder_amd.encoder import plane_layout_extent
    torch = torch_cuda
    W, H, n = 352, 288, 2
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    enc.set_plane_layout("nv12")
    lay = enc.plane_layout
    L = plane_layout_extent(lay, enc.strips, enc.mb_rows)
    assert L == W * H * 3 // 2
    buf = torch.full((n * lay["frame_stride"] + 64,), 128, dtype=torch.uint8, device="cuda")
    good = torch.as_strided(buf, (n, L), (lay["frame_stride"], 1))
    for bad in (torch.as_strided(buf, (n, L - 1), (lay["frame_stride"], 1)), torch.as_strided(buf, (n, L), (lay["frame_stride"] + 1, 1)),
                torch.as_strided(buf, (n, L // 2), (lay["frame_stride"], 2)), buf[:n * L].view(n, H * 3 // 2, W)):
        with pytest.raises(AssertionError):
            enc.encode(bad)
    enc.encode(good)
    enc.encode(good[1:])                                            # one frame: its stride says nothing
    enc.flush()
    torch.cuda.synchronize()
    enc.close()


# ---- 9. a full-size batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["reference", "nv12"])
def test_full_size_batch(torch_cuda, orc, layout):
    """300 x 1080p of synthetic bytes read as planes (any bytes are valid planes; the NV12 layout with the frame stride of the
    synthetic frames, 3 * W * H): two runs identical, every record's length field consistent, the sizes sum to the total,
    and frames 0, 255, 256, 299 are plane_oracle's."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    W, H, n, first = 1920, 1080, 300, 0
    lay = dict(_layout(layout, W, H)[0], frame_stride=3 * W * H)
    enc = _plane_encoder(W, H, 12, "full", n, lay)
    src = Mpeg1Encoder(W, H, 12, "full", max_frames=1)
    x = src.synth(n, seed=504).view(n, -1)
    src.close()
    check = (0, 255, 256, 299)
    host = {f: x[f].cpu().numpy() for f in check}
    want = {f: plane_oracle.encode_layout(host[f], lay, W, H, first + f, 12, orc.MODE_FULL) for f in check}   # (encodable)
    runs = []
    for _ in range(2):
        out = torch.empty(enc.frame_bound * 8 + n * (W * H // 2), dtype=torch.uint8, device="cuda")
        out, sizes, meta = enc.encode(x, first, out=out)
        enc.flush()
        torch.cuda.synchronize()
        total, status = (int(v) for v in meta.cpu())
        assert status & 0xFFFFFFFF == 0, status
        runs.append((out[:total].cpu().numpy(), [int(s) for s in sizes[:n].cpu()]))
    (blob, sizes), (blob2, sizes2) = runs
    assert sizes == sizes2 and np.array_equal(blob, blob2)
    assert sum(sizes) == len(blob)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for f in range(n):
        rec = blob[offs[f]:offs[f + 1]]
        assert (int(rec[4]) << 8 | int(rec[5])) == (sizes[f] - 4 - 8) & 0xffff, f
        assert bytes(rec[-4:]) == b"\0\0\0\0", f
    for f in check:
        assert blob[offs[f]:offs[f + 1]].tobytes() == want[f], f
    enc.close()
