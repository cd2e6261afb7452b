"""GPU tests of the surface input layout (m1v_set_input_layout; k_encode_surface, k_size_table_surface; -m gpu): frames that
are windows of pitched device surfaces, in R,G,B(,A) or B,G,R(,A) byte order, encoded where they lie.

The checker is the CPU oracle.  The expected bytes of a surface encode are the oracle's bytes for the packed R,G,B(,A) copy of
the window, np.ascontiguousarray(surface[:, y0:y0+H, x0:x0+W, :]) with bytes 0 and 2 swapped for B,G,R: here a surface is a
device buffer of noise into which exactly that packed copy is written through the strided view the encoder is given, so the
packed copy is the array the test started from.  Every comparison is for equality; every status word is 0 unless a case says
otherwise."""

import numpy as np
import pytest

from colour_content import _CH, _COLOURS_PER_FRAME, _CW, _flat_cell_frames, _tie_colours
from gpu_calls import _encode, _frame_rule, _frames, _mixed_frames, _oracle, _oracle_sizes, _table
from layout_inputs import _surface, _surface_encoder
from layout_inputs import _surface_geometry as _geometry
from rate_rules import batch_rule, cbr_rule
from table_cases import MATRIX, RGB_CASES, SEQUENCE, RateMixed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- surfaces ---------------------------------------------------------------------------------------------------------------


LAYOUTS = ("packed", "odd", "gap", "window")


def _with_alpha(rng, px):
    if px.shape[-1] == 4:                       # noise: a kernel that reads alpha as a colour gets every size wrong
        px[..., 3] = rng.integers(0, 256, px.shape[:3], dtype=np.uint8)
    return px


# ---- 1. the parity matrix ---------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _expected(orc, case, channels):
    """The case's frames (alpha noise) and the oracle's records of every frame at every quality the case uses."""
    key = (case, channels)
    if key not in _oracle_cache:
        W, H, Q, mode, n, amps, quals = MATRIX[case]
        rng = np.random.default_rng(sum(map(ord, case)) + channels)
        px = _with_alpha(rng, _mixed_frames(rng, n, W, H, channels, amps))
        m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
        first = 17
        qs = sorted(set(quals) | {Q})
        recs = {q: [orc.encode_frame(px[f], W, H, first + f, q, m, channels=channels) for f in range(n)] for q in qs}
        _oracle_cache[key] = (px, first, recs)
    return _oracle_cache[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("case", sorted(MATRIX))
def test_parity_matrix(torch_cuda, orc, case, channels, order, layout):
    """encode, encode(quality=per frame), frame_sizes and frame_size_table on a surface against the oracle."""
    torch = torch_cuda
    W, H, Q, mode, n, amps, quals = MATRIX[case]
    px, first, recs = _expected(orc, case, channels)
    dev, pitch, stride = _surface(torch, px, layout, order, fill_seed=len(case))
    enc = _surface_encoder(W, H, Q, mode, channels, n, pitch, stride, order)
    got, sizes = _encode(torch, enc, dev, first)
    assert sizes == [len(r) for r in recs[Q]]
    assert got == b"".join(recs[Q])
    qs = [quals[(f + 1) % len(quals)] for f in range(n)]             # one quality per frame, from the case's list
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


# ---- 2. padding is never used -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["odd", "gap", "window"])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("case", ["cif_full_k8", "partial_tiles_366x216", "odd_last_column_176x208"])
def test_padding_is_never_used(torch_cuda, case, channels, layout):
    """The same window content under two different fills of everything outside the window (row padding, frame gaps, the
    surface around the window; for 4 channels also the 4th byte of every pixel): identical records, sizes and tables."""
    torch = torch_cuda
    W, H, Q, mode, n, amps, quals = MATRIX[case]
    results = []
    for fill in (1, 2):
        rng = np.random.default_rng(5)
        px = _mixed_frames(rng, n, W, H, channels, amps)
        _with_alpha(np.random.default_rng(70 + fill), px)
        dev, pitch, stride = _surface(torch, px, layout, "bgr", fill_seed=fill)
        enc = _surface_encoder(W, H, Q, mode, channels, n, pitch, stride, "bgr")
        results.append((_encode(torch, enc, dev, 3), _table(torch, enc, dev, quals)))
        enc.close()
    assert results[0] == results[1]
    assert results[0][1][1] == [0] * len(quals)


# ---- 3. one packed buffer through both kernel families -------------------------------------------------------------------------
K8 = (1, 2, 4, 6, 8, 10, 11, 12)


@pytest.mark.parametrize("channels", [3, 4])
def test_ab_on_one_buffer(torch_cuda, orc, channels):
    """A packed buffer through the default kernels and, with the pitch W * C set explicitly, through the surface kernels:
    identical records, sizes and K = 8 tables.  The 4-channel surface encoder runs the tile workgroup; back on the default
    layout it runs the run kernels again, with the same bytes."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    W, H, n = 352, 288, 5
    rng = np.random.default_rng(31 + channels)
    px = _with_alpha(rng, _mixed_frames(rng, n, W, H, channels))
    dev = torch.from_numpy(px).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", channels=channels, max_frames=n)
    default_path = "tiles" if channels == 3 else "runs"
    assert enc.path == default_path and enc.input_layout == (0, 0, "rgb")
    a = (_encode(torch, enc, dev, 9), _table(torch, enc, dev, K8))
    enc.set_input_layout(W * channels)
    assert enc.path == "tiles" and enc.size_table_fused == 1
    assert enc.input_layout == (W * channels, H * W * channels, "rgb")
    b = (_encode(torch, enc, dev, 9), _table(torch, enc, dev, K8))
    enc.set_input_layout()
    assert enc.path == default_path and enc.size_table_fused == 1 and enc.input_layout == (0, 0, "rgb")
    c = (_encode(torch, enc, dev, 9), _table(torch, enc, dev, K8))
    assert a == b == c
    want, wsizes = _oracle(orc, px, 9, [12] * n, orc.MODE_FULL, channels)
    assert a[0] == (want, wsizes) and a[1][1] == [0] * len(K8)
    enc.close()


# ---- 4. colours -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("channels", [3, 4])
def test_colour_inside_the_surface_kernels_ties_and_sample(torch_cuda, orc, channels, order):
    """All tie / near-tie colours (every input that takes the fp64 branch) and 2^20 random colours through each of the four
    [bytes per pixel][byte order] encode kernels, on a padded pitch, as Y, Cb and Cr each: the flat-cell pictures of
    tests/test_gpu_parity.py (the loop of its _check_colours_through, which uploads packed R,G,B frames).  The byte
    permutation feeds the fp64 tie path."""
    torch = torch_cuda
    chunk = 48
    ties = _tie_colours()
    assert 50000 < len(ties) < 400000
    sample = np.random.default_rng(2024).integers(0, 256, (1 << 20, 3), dtype=np.uint8)
    colours = np.concatenate([ties, sample])
    pitch, stride, _, _ = _geometry("gap", _CW, _CH, channels)
    enc = _surface_encoder(_CW, _CH, 50, "full", channels, chunk, pitch, stride, order)
    per = _COLOURS_PER_FRAME * chunk
    for lo in range(0, len(colours), per):
        frames = _flat_cell_frames(colours[lo:lo + per], channels)
        n = frames.shape[0]
        want, wsizes = orc.encode_frames(frames, n, _CW, _CH, 0, 50, orc.MODE_FULL, channels=channels, threads=16)
        dev, p, s = _surface(torch, frames, "gap", order, fill_seed=lo % 97)
        assert (p, s) == (pitch, stride)
        got, sizes = enc.encode_to_bytes(dev, 0)
        assert sizes == [int(x) for x in wsizes] and got == want, f"colours {lo}..{lo + per}"
        del dev
    enc.close()


# ---- 5. the rate calls ------------------------------------------------------------------------------------------------------
CANDS5 = (2, 4, 6, 8, 12)


def test_rate_calls_on_a_pitched_bgra_surface(torch_cuda, orc):
    """Budget, batch budget and bitrate: the picks are the Python rules of tests/test_rate_abi.py on the oracle's sizes, the
    records the oracle's at the picked qualities; each is one size-table pass + one encode (2 profiled launches).  A bitrate
    stream chained over two calls equals one call."""
    torch = torch_cuda
    n, W, H, first = 6, 352, 288, 40
    rng = np.random.default_rng(101)
    px = _with_alpha(rng, _mixed_frames(rng, n, W, H, 4))
    dev, pitch, stride = _surface(torch, px, "gap", "bgr", fill_seed=3)
    enc = _surface_encoder(W, H, 12, "full", 4, n, pitch, stride, "bgr")
    s = [_oracle_sizes(orc, px, orc.MODE_FULL, c, 4) for c in CANDS5]
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
        want, wsizes = _oracle(orc, px, first, chosen, orc.MODE_FULL, 4)
        assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), call
    # the same stream in two calls: frames [0, 4) then [4, 6), the level handed from one to the next on the device
    one = (got, sizes, ch, ov, int(level.cpu()[0]))
    level.fill_(10 ** 6)
    a = enc.encode_at_bitrate(dev[:4], r, 2 * r, CANDS5, level, first_frame_index=first)
    b = enc.encode_at_bitrate(dev[4:], r, 2 * r, CANDS5, level, first_frame_index=first + 4)
    assert (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + [f + 4 for f in b[3]], int(level.cpu()[0])) == one
    enc.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------
class _SurfaceUploads:
    """torch as RateMixed sees it: from_numpy(frames).cuda() puts a batch of the encoder's frames into a pitched B,G,R(,A)
    surface and returns the view; everything else is torch's.  Mixed and RateMixed compute their expectations from the numpy
    frames they made, i.e. from the packed R,G,B(,A) copy of the window."""

    def __init__(self, torch, shape_tail, layout, order):
        self._torch, self._tail, self._layout, self._order, self._fills = torch, tuple(shape_tail), layout, order, 0

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def from_numpy(self, arr):
        outer = self

        class _Upload:
            def cuda(self):
                if arr.dtype != np.uint8 or arr.ndim != 4 or tuple(arr.shape[1:]) != outer._tail:
                    return outer._torch.from_numpy(arr).cuda()
                outer._fills += 1
                return _surface(outer._torch, arr, outer._layout, outer._order, fill_seed=outer._fills)[0]

        return _Upload()


def _mixed_on_a_surface(torch, orc, channels, pipelined, seed, layout="gap", order="bgr", max_frames=5):
    W, H = 352, 288
    pitch, stride, _, _ = _geometry(layout, W, H, channels)
    enc = _surface_encoder(W, H, 12, "full", channels, max_frames, pitch, stride, order, pipelined)
    return enc, RateMixed(_SurfaceUploads(torch, (H, W, channels), layout, order), orc, enc, seed=seed)


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("channels", [3, 4])
def test_interleaved_calls_stay_exact(torch_cuda, orc, channels, pipelined):
    """SEQUENCE of tests/test_gpu_rate.py (plain, per-frame, probe, table, budget, batch-budget and bitrate calls) twice on a
    surface encoder, plain and pipelined."""
    enc, calls = _mixed_on_a_surface(torch_cuda, orc, channels, pipelined, seed=900 + channels + pipelined)
    for _ in range(2):
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("sequence", channels, pipelined))
    enc.close()


@pytest.mark.parametrize("channels", [3, 4])
def test_host_delivery_of_surface_batches(torch_cuda, orc, channels):
    """m1v_delivery_* through the Python mirror: three batches of a pitched B,G,R(,A) surface arrive as the oracle's streams."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n = 352, 288, 4
    rng = np.random.default_rng(12 + channels)
    batches = [(_with_alpha(rng, _frames(rng, n, W, H, channels)), 50 * k + 3) for k in range(3)]
    views = [_surface(torch, px, "window", "bgr", fill_seed=k) for k, (px, _) in enumerate(batches)]
    enc = _surface_encoder(W, H, 12, "full", channels, n, views[0][1], views[0][2], "bgr")
    hd = HostDelivery(enc, n)
    got = []

    def take():
        hd.delivered[hd.last[0]].synchronize()
        got.append((bytes(hd.result().numpy()), [int(x) for x in hd.frame_sizes(n)]))

    hd.step(views[0][0], batches[0][1])
    assert hd.last is None
    hd.step(views[1][0], batches[1][1])
    take()
    hd.step(views[2][0], batches[2][1])
    take()
    hd.fence()
    take()
    for (blob, sizes), (px, first) in zip(got, batches):
        want, wsizes = _oracle(orc, px, first, [12] * n, orc.MODE_FULL, channels)
        assert (blob, sizes) == (want, wsizes), first
    hd.close()
    enc.close()


@pytest.mark.parametrize("channels", [3, 4])
def test_forced_small_lds_image_takes_the_arena(torch_cuda, orc, channels):
    """An 8-word LDS image sends every tile to the overflow arena: M1V_STATUS_SCRATCH with the default arena, and the oracle's
    bytes (built by global atomics in worst-case slots) once the worst case is reserved; then the default image again."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 5
    rng = np.random.default_rng(77 + channels)
    px = _with_alpha(rng, _frames(rng, n, W, H, channels))
    dev, pitch, stride = _surface(torch, px, "odd", "bgr", fill_seed=4)
    enc = _surface_encoder(W, H, 12, "full", channels, n, pitch, stride, "bgr")
    want = _oracle(orc, px, 21, [12] * n, orc.MODE_FULL, channels)
    enc.debug_set_lds_words(8)
    assert enc.path == "tiles" and enc.input_layout == (pitch, stride, "bgr")
    out, sizes, meta = enc.encode(dev, 21)
    torch.cuda.synchronize()
    assert int(meta.cpu()[1]) & 0xFFFFFFFF == _ffi.STATUS_SCRATCH
    enc.reserve_scratch(True)
    assert enc.path == "tiles" and enc.input_layout == (pitch, stride, "bgr")
    assert _encode(torch, enc, dev, 21) == want
    enc.debug_set_lds_words(0)
    enc.reserve_scratch(False)
    assert _encode(torch, enc, dev, 21) == want
    enc.close()


@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("pipelined", [False, True])
def test_failed_call_leaves_the_encoder_correct(torch_cuda, orc, pipelined, stage):
    """m1v_debug_fail_encode makes an encode and a size-table call on a surface encoder return M1V_E_HIP on the host (nothing
    faults on the device); every call of every kind after each is exact."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch = torch_cuda
    enc, calls = _mixed_on_a_surface(torch, orc, 4, pipelined, seed=950 + 10 * stage + pipelined)
    calls.call("table", 5)
    calls.call("plain", 4)
    calls.check("before")
    dev = calls.torch.from_numpy(_frames(calls.rng, 5, 352, 288, 4)).cuda()
    for what in ("encode", "table"):
        _ffi.lib().m1v_debug_fail_encode(stage)
        try:
            with pytest.raises(EncoderError) as ei:
                if what == "encode":
                    enc.encode(dev, 0)
                else:
                    enc.frame_size_table(dev, (3, 6, 9, 12))
            assert ei.value.code == _ffi.E_HIP
        finally:
            _ffi.lib().m1v_debug_fail_encode(0)
        enc.flush()
        torch.cuda.synchronize()
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("after the failed", what))
    enc.close()


def test_failed_allocation_in_set_input_layout_changes_nothing(torch_cuda, orc):
    """m1v_debug_fail_alloc inside set_input_layout (a 4-channel encoder: the tile plan needs scratch of another size than the
    run plan, in both directions): M1V_E_HIP, and layout, path, scratch and bytes are what they were."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 4
    rng = np.random.default_rng(55)
    px = _with_alpha(rng, _mixed_frames(rng, n, W, H, 4))
    packed = torch.from_numpy(px).cuda()
    dev, pitch, stride = _surface(torch, px, "gap", "bgr", fill_seed=6)
    want = _oracle(orc, px, 5, [12] * n, orc.MODE_FULL, 4)
    enc = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)
    assert _encode(torch, enc, packed, 5) == want

    def refused(*layout):
        before = (enc.input_layout, enc.path, enc.scratch_bytes())
        _ffi.lib().m1v_debug_fail_alloc(1)
        try:
            with pytest.raises(EncoderError) as ei:
                enc.set_input_layout(*layout)
            assert ei.value.code == _ffi.E_HIP
        finally:
            _ffi.lib().m1v_debug_fail_alloc(0)
        assert (enc.input_layout, enc.path, enc.scratch_bytes()) == before

    refused(pitch, stride, "bgr")
    assert enc.path == "runs" and _encode(torch, enc, packed, 5) == want
    enc.set_input_layout(pitch, stride, "bgr")
    assert _encode(torch, enc, dev, 5) == want
    refused()
    assert enc.path == "tiles" and _encode(torch, enc, dev, 5) == want
    enc.set_input_layout()
    assert enc.path == "runs" and _encode(torch, enc, packed, 5) == want
    enc.close()


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------
def test_argument_errors(torch_cuda):
    """Every M1V_E_ARG case of m1v_set_input_layout; none of them changes the layout in force."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    L = _ffi.lib()
    W, H = 352, 288
    for channels in (3, 4):
        row = W * channels
        enc = Mpeg1Encoder(W, H, 12, "full", channels=channels, max_frames=2)
        good = (row + 64, H * (row + 64) + 5, "bgr")
        enc.set_input_layout(*good)
        for pitch, stride, order in (
                (row - 1, 0, 0), (1, 0, 0),                                   # a pitch below W * C
                (row + 64, (H - 1) * (row + 64) + row - 1, 0),                # a stride below the bytes a frame's window spans
                (0, (H - 1) * row + row - 1, 1), (0, 1, 0),
                ((2 ** 32 - row) // (H - 1) + 1, 0, 0), (2 ** 32, 0, 0), (2 ** 40, 0, 1),   # (H - 1) * pitch + W * C >= 2^32
                (row, 0, 2), (0, 0, -1), (row, H * row, 7)):                  # an unknown order
            assert L.m1v_set_input_layout(enc._h, pitch, stride, order) == _ffi.E_ARG, (pitch, stride, order)
            assert enc.input_layout == good and enc.path == "tiles"
        # the largest window whose offsets are still 32-bit is accepted (only set here: tests/test_gpu_address_space.py encodes
        # through this pitch, in a pool that holds every offset it reaches)
        assert L.m1v_set_input_layout(enc._h, (2 ** 32 - row - 1) // (H - 1), 0, 0) == 0
        enc.set_input_layout()
        assert enc.input_layout == (0, 0, "rgb")
        enc.close()


@pytest.mark.parametrize("channels", [3, 4])
def test_odd_width_keeps_the_default_layout(torch_cuda, orc, channels):
    """tiny_105x49: every surface layout is an argument error (a chroma block row would straddle two picture rows), and the
    default layout encodes it as before."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, Q, mode, n, amps, quals = RGB_CASES["tiny_105x49"]
    rng = np.random.default_rng(15)
    px = _with_alpha(rng, _mixed_frames(rng, n, W, H, channels, amps))
    enc = Mpeg1Encoder(W, H, Q, mode, channels=channels, max_frames=n)
    path = enc.path
    for layout in ((W * channels,), (W * channels + 3,), (0, H * W * channels + 7), (0, 0, "bgr"), (W * channels + 1, 0, "bgr")):
        with pytest.raises(EncoderError) as ei:
            enc.set_input_layout(*layout)
        assert ei.value.code == _ffi.E_ARG
        assert enc.input_layout == (0, 0, "rgb") and enc.path == path
    enc.set_input_layout()
    dev = torch.from_numpy(px).cuda()
    assert _encode(torch, enc, dev, 2) == _oracle(orc, px, 2, [Q] * n, orc.MODE_FULL, channels)
    table, status = _table(torch, enc, dev, quals)
    assert status == [0] * len(quals) and table == [_oracle_sizes(orc, px, orc.MODE_FULL, q, channels) for q in quals]
    enc.close()


def test_packed_only_entry_points_refuse_a_surface_encoder(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 2
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    dev = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    host = np.zeros((n, H, W, 3), np.uint8)
    planes = np.zeros((n, 3, H * W), np.uint8)
    for layout in ((W * 3,), (W * 3 + 4, 0, "bgr")):
        enc.set_input_layout(*layout)
        for call in (lambda: enc.coefficients(dev), lambda: enc.convert(dev), lambda: enc.encode_host(host),
                     lambda: enc.encode_host(host, with_planes=True)):
            with pytest.raises(EncoderError) as ei:
                call()
            assert ei.value.code == _ffi.E_ARG
        assert _ffi.lib().m1v_convert_host(enc._h, host.ctypes.data, n, planes.ctypes.data) == _ffi.E_ARG
    enc.set_input_layout()
    assert enc.coefficients(dev).shape == (n, enc.blocks_per_frame, 64)
    assert enc.convert(dev).shape == (n, 3, H * W)
    assert len(enc.encode_host(host)[1]) == n
    assert _ffi.lib().m1v_convert_host(enc._h, host.ctypes.data, n, planes.ctypes.data) == 0
    enc.close()


def test_hooks_and_surface_layouts_refuse_each_other(torch_cuda):
    """A surface layout on an encoder that a hook has forced to the run kernels, and those hooks on a surface encoder."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    W, H = 352, 288
    forcing = {"path": lambda e: e.debug_set_path("runs"), "input mode": lambda e: e.debug_set_input_mode(0),
               "funnel": lambda e: e.debug_set_input_mode(2), "run length": lambda e: e.debug_set_dense_threads(64)}
    undo = {"path": lambda e: e.debug_set_path("auto"), "input mode": lambda e: e.debug_set_input_mode(-1),
            "funnel": lambda e: e.debug_set_input_mode(-1), "run length": lambda e: e.debug_set_dense_threads(0)}
    for channels in (3, 4):
        for name, force in forcing.items():
            if name == "funnel" and channels == 4:
                continue
            enc = Mpeg1Encoder(W, H, 12, "full", channels=channels, max_frames=2)
            force(enc)
            assert enc.path == "runs"
            for layout in ((W * channels,), (W * channels + 16, 0, "rgb"), (0, 0, "bgr")):
                with pytest.raises(EncoderError) as ei:
                    enc.set_input_layout(*layout)
                assert ei.value.code == _ffi.E_ARG, (name, layout)
                assert enc.input_layout == (0, 0, "rgb") and enc.path == "runs"
            enc.set_input_layout()                                 # the default layout is always accepted
            undo[name](enc)
            enc.set_input_layout(W * channels + 16, 0, "bgr")
            assert enc.path == "tiles"
            with pytest.raises(EncoderError) as ei:
                force(enc)
            assert ei.value.code == _ffi.E_ARG, name
            assert enc.path == "tiles" and enc.input_layout == (W * channels + 16, H * (W * channels + 16), "bgr")
            undo[name](enc)                                        # (releasing a hook that is not set changes nothing)
            assert enc.path == "tiles"
            enc.close()


def test_python_checks_the_strides_against_the_layout(torch_cuda):
    """A contiguous tensor is rejected while a padded pitch is in force, a padded view while the default layout is, and a
    view of another pitch or frame stride than the layout's."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    W, H, n = 352, 288, 2
    px = np.zeros((n, H, W, 4), np.uint8)
    packed = torch.from_numpy(px).cuda()
    gap, pitch, stride = _surface(torch, px, "gap", "rgb")
    window = _surface(torch, px, "window", "rgb")[0]
    enc = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)
    for bad in (gap, window):
        with pytest.raises(AssertionError):
            enc.encode(bad)
        with pytest.raises(AssertionError):
            enc.frame_size_table(bad, (4, 12))
    enc.set_input_layout(pitch, stride)
    for bad in (packed, window, gap[:, :, :, :3], gap[:, ::2]):
        with pytest.raises(AssertionError):
            enc.encode(bad)
        with pytest.raises(AssertionError):
            enc.frame_sizes(bad)
    enc.encode(gap)
    enc.encode(gap[1:])                                            # one frame: its stride says nothing
    enc.set_input_layout(W * 4)
    enc.encode(packed)                                             # the packed pitch, set explicitly: a contiguous tensor fits
    enc.flush()
    torch.cuda.synchronize()
    enc.close()
