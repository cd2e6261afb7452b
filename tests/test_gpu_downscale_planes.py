"""GPU tests of the downscale plane layout (m1v_set_downscale_plane_layout; k_half_planes_encode, k_half_planes_size_table,
k_half_planes_rd_table, k_half_planes_to_i420; -m gpu): [n, L] uint8 frames of 2W x 2H 4:2:0 planes (I420, YV12, NV12, NV21) whose
2 x 2 box average per plane is encoded at W x H, where they lie.

The definition (include/mpeg1_hip.h, "Downscale plane layout") is checked for equality on the samples themselves
(downscale_planes_to_i420) against tests/downscale_planes.py's model; every expected record is tests/plane_oracle.py's on the
model's I420 frame under plane_layout_preset(W, H, "i420"), and the rate calls are held against the same calls on those bytes
through the I420 plane layout.  A source is written into a device buffer of noise (downscale_planes.place); every batch lies 64
bytes inside its allocation, so nothing here can fault.  Every comparison is for equality and every status word is 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

import downscale_planes as dp
import plane_oracle
import rd_oracle as rd
from gpu_calls import _encode, _rd, _table

pytestmark = pytest.mark.gpu

# rendition size, mode: one macroblock; 3 strips; a 2 x 2 tile grid with a 1-strip, 1-row remainder; the 96 x 144 corner
CASES = ((16, 16, "full"), (48, 32, "full"), (144, 80, "full"), (112, 160, "strict"))
QUALITIES = (12, 50)
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
    enc.set_downscale_plane_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1 and enc.downscale_plane_layout == lay
    return enc


def _i420_of(torch, enc, x):
    out = enc.downscale_planes_to_i420(x)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_record_cache = {}


def _oracle(orc, frames, W, H, mode, first, qs, key=None):
    """plane_oracle's (records back to back, sizes) of the I420 frames [n, W * H * 3 / 2] at one quality per frame (or one for
    all); cached per frame under `key` where several tests share it (the key names the source: its seed comes from W and H, its
    samples also depend on the number of frames drawn)."""
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


def _noise(W, H, n=3):
    return dp.noise_source(W * 100 + H, n, H, W)      # (the sources of tests/test_downscale_planes_cpu.py's census)


# ---- 1. the averaging ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", dp.PRESETS)
@pytest.mark.parametrize("W,H,mode", CASES)
def test_arithmetic_on_noise(torch_cuda, orc, W, H, mode, preset):
    """Noise sources in every form, tight and as a pitched window, batches of 1 and 3 frames at qualities 12 and 50: the samples
    are the model's; records, sizes, total and status are the oracle's on them, and the same encoder under the I420 plane layout
    on the to-i420 call's output gives the same records."""
    torch = torch_cuda
    src = _noise(W, H)
    want_frames = dp.model_frames(src)
    for k, where in enumerate((dp.TIGHT, dp.PITCHED)):
        x, lay, _ = dp.place(torch, src, preset, fill_seed=k, **where)
        for Q in QUALITIES:
            enc = _encoder(W, H, Q, 3, lay, mode)
            for n in (1, 3):
                what = f"{W}x{H} {mode} {preset} {where} Q{Q} n{n}"
                want = _oracle(orc, want_frames[:n], W, H, mode, FIRST, Q, key=("noise", 3))
                i420 = enc.downscale_planes_to_i420(x[:n])
                got = _i420_of(torch, enc, x[:n])
                assert got.shape == (n, W * H * 3 // 2) and got.dtype == np.uint8
                wrong = np.argwhere(got != want_frames[:n])
                assert not len(wrong), (what, len(wrong), [(tuple(w), int(got[tuple(w)]), int(want_frames[tuple(w)])) for w in wrong[:8]])
                blob, sizes = _encode(torch, enc, x[:n], FIRST)
                assert sizes == want[1], (what, [f for f in range(n) if sizes[f] != want[1][f]])
                at = np.concatenate([[0], np.cumsum(want[1])])
                assert not [f for f in range(n) if blob[at[f]:at[f + 1]] != want[0][at[f]:at[f + 1]]] and len(blob) == at[n], what
                enc.set_plane_layout("i420")                            # the same encoder on the bytes
                assert _encode(torch, enc, i420, FIRST) == want, what
                enc.set_downscale_plane_layout(lay)
            enc.close()


# every residue of the four-sum mod 4 at the bottom (sums 0, 1, 2, 3) and at the top (1017, 1018, 1019, 1020), each cell in every
# placement of its values
CELLS = sorted({p for cell in ((0, 0, 0, 0), (0, 0, 0, 1), (1, 1, 0, 0), (1, 1, 1, 0),
                               (255, 254, 254, 254), (255, 255, 254, 254), (255, 255, 255, 254), (255, 255, 255, 255))
                for p in itertools.permutations(cell)})


@pytest.mark.parametrize("preset", dp.PRESETS)
def test_extremes(torch_cuda, orc, preset):
    """Every residue of the four-sum mod 4 at both ends: 0 -> 0, 1 rounds down to 0, the tie 2 up to 1, 3 up to 1; 1017 down to 254,
    the tie 1018 up to 255, 1019 up to 255, and all 255 (the carry into bit 8 of every 16-bit half, 1020 + 2), the four-value
    cells in every placement within the cell; one frame per cell, with the luma, Cb and Cr planes of a frame on three different
    cells, so that every cell passes through every plane's path and an exchange of Cb and Cr shows."""
    torch = torch_cuda
    W, H, n = 48, 32, len(CELLS)
    assert n == 1 + 4 + 6 + 4 + 4 + 6 + 4 + 1 and {sum(c) % 4 for c in CELLS if sum(c) < 4} == {sum(c) % 4 for c in CELLS if sum(c) > 4} == {0, 1, 2, 3}
    parts = [dp.cell_source(CELLS[f], CELLS[(f + 10) % n], CELLS[(f + 20) % n], 1, H, W) for f in range(n)]
    src = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    frames = dp.model_frames(src)
    value = lambda cell: (sum(cell) + 2) >> 2
    assert [(int(frames[f, 0]), int(frames[f, W * H]), int(frames[f, W * H + W * H // 4])) for f in range(n)] == \
        [(value(CELLS[f]), value(CELLS[(f + 10) % n]), value(CELLS[(f + 20) % n])) for f in range(n)]
    assert {int(v) for v in np.unique(frames)} == {0, 1, 254, 255}
    assert any(frames[f, W * H] != frames[f, W * H + W * H // 4] for f in range(n))
    want = _oracle(orc, frames, W, H, "full", 0, 12)
    x, lay, _ = dp.place(torch, src, preset, fill_seed=3, **dp.PITCHED)
    enc = _encoder(W, H, 12, n, lay)
    got = _i420_of(torch, enc, x)
    assert np.array_equal(got, frames), [CELLS[f] for f in range(n) if not np.array_equal(got[f], frames[f])]
    assert _encode(torch, enc, x, 0) == want
    enc.close()


# ---- 2. the read contract -----------------------------------------------------------------------------------------------------------
# 3 strips in the last tile column (48 and 176 wide) and xe < W (40 wide); tight I420 and NV12, where the last chroma unit of the
# second component ends with the frame, the pitched window, and planes with c_step 2 that are not interleaved with each other
CONTRACT = [(W, preset, where) for W in (48, 176, 40)
            for preset, where in (("i420", dp.TIGHT), ("nv12", dp.TIGHT), ("nv21", dp.PITCHED), ("yv12", dp.PITCHED),
                                  ("i420", dict(spread=True, cpad=5, shift=3)))]


@pytest.mark.parametrize("W,preset,where", CONTRACT, ids=[f"{W}-{p}-{'tight' if not w else 'spread' if 'spread' in w else 'pitched'}"
                                                          for W, p, w in CONTRACT])
def test_read_contract(torch_cuda, orc, W, preset, where):
    """The same sources under two fills of every byte the definition does not address — row padding, the gaps between planes and
    frames, the surface around the window, the guards, the other bytes of a c_step = 2 plane that is not interleaved: identical
    samples, records and tables, the oracle's.  Nothing lies against the end of an allocation."""
    torch = torch_cuda
    H, n = 32, 3
    src = _noise(W, H, n)
    frames = dp.model_frames(src)
    want = _oracle(orc, frames, W, H, "full", 0, 12, key=("noise", n))
    seen = []
    for fill in (1, 2):
        x, lay, buf = dp.place(torch, src, preset, fill_seed=fill, **where)
        seen.append(buf.cpu().numpy())
        enc = _encoder(W, H, 12, n, lay)
        assert enc.strips * 16 == W - W % 16
        assert np.array_equal(_i420_of(torch, enc, x), frames), fill
        assert _encode(torch, enc, x, 0) == want, fill
        assert _table(torch, enc, x, (12,)) == ([want[1]], [0]), fill
        assert _rd(torch, enc, x, (12,))[0] == [want[1]], fill
        enc.close()
    # the two allocations differ everywhere but in the addressed bytes (tests/test_downscale_planes_cpu.py pins the placement)
    lay, _, at = dp.geometry(W, H, preset, **where)
    same = dp.addressed(lay, n, W, H, at, len(seen[0]))
    assert np.array_equal(seen[0][same], seen[1][same])
    assert (seen[0][~same] != seen[1][~same]).mean() > 0.9 and (~same).sum() >= 2 * dp.GUARD


# ---- 3. the setter ------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_layout_in_force(torch_cuda, orc):
    """Every M1V_E_ARG case of m1v_set_downscale_plane_layout, each with its reason; none changes the layout in force, the table
    mode or the records."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi, downscale_plane_layout_preset
    from ec504_imageencoder_amd.encoder import downscale_plane_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    S = _ffi.DownscalePlaneLayout
    W, H, n = 48, 32, 3
    src = _noise(W, H, n)
    want = _oracle(orc, dp.model_frames(src), W, H, "full", 0, 12, key=("noise", n))
    x, good, _ = dp.place(torch, src, "nv12", **dp.PITCHED)
    tight = downscale_plane_layout_preset(W, H, "nv12")
    assert good["c_step"] == 2 and good["factor"] == 2 and good["reserved"] == 0
    enc = _encoder(W, H, 12, n, good)
    big = 2 ** 40
    E = downscale_plane_layout_extent(good, enc.strips, enc.mb_rows)
    assert E == good["cr_offset"] + (H - 1) * good["c_pitch"] + (W - 1) * 2 + 1 and E <= good["frame_stride"]
    bad = [(dict(good, factor=4), b"factor"), (dict(good, factor=0), b"factor"), (dict(good, factor=1), b"factor"),
           (dict(good, reserved=1), b"reserved"), (dict(good, reserved=-1), b"reserved"),
           (dict(good, c_step=3), b"c_step"), (dict(good, c_step=4), b"c_step"),
           (dict(good, frame_stride=0), b"frame stride"),
           (dict(good, y_pitch=2 * W - 1), b"luma pitch below"), (dict(good, y_pitch=W), b"luma pitch below"),   # the rendition's row
           (dict(good, y_pitch=1), b"luma pitch below"),
           (dict(good, c_pitch=2 * W - 1), b"chroma pitch below"), (dict(good, c_pitch=W), b"chroma pitch below"),
           (dict(good, c_step=1, c_pitch=W - 1), b"chroma pitch below"),
           (dict(tight, y_pitch=(2 ** 32 - 2 * W) // (2 * H - 1) + 1, frame_stride=big), b"4 GiB"),
           (dict(tight, y_pitch=2 ** 32, frame_stride=big), b"4 GiB"), (dict(tight, c_pitch=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(tight, cb_offset=2 ** 32, frame_stride=big), b"4 GiB"), (dict(tight, y_offset=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(tight, cr_offset=2 ** 32 - ((H - 1) * 2 * W + (W - 1) * 2 + 1), frame_stride=big), b"4 GiB"),
           (dict(good, frame_stride=E - 1), b"frame stride below"),
           (dict(good, frame_stride=good["y_offset"] + (2 * H - 1) * good["y_pitch"] + 2 * W), b"frame stride below")]  # the luma plane alone
    for lay, reason in bad:
        assert L.m1v_set_downscale_plane_layout(enc._h, C.byref(S(**lay))) == _ffi.E_ARG, lay
        assert L.m1v_last_error() and reason in L.m1v_last_error(), (lay, L.m1v_last_error())
        assert enc.downscale_plane_layout == good and enc.path == "tiles" and not enc.frame_table and not enc.plane_table
        with pytest.raises(EncoderError):
            enc.set_downscale_plane_layout(lay)
    assert _encode(torch, enc, x, 0) == want
    # the largest extent whose offsets are still 32-bit and the smallest stride are accepted (set, not encoded); zeros default
    edge = dict(tight, cr_offset=2 ** 32 - 1 - ((H - 1) * 2 * W + (W - 1) * 2 + 1), frame_stride=big)
    assert L.m1v_set_downscale_plane_layout(enc._h, C.byref(S(**edge))) == 0 and enc.downscale_plane_layout == edge
    assert L.m1v_set_downscale_plane_layout(enc._h, C.byref(S(**dict(good, frame_stride=E)))) == 0
    assert enc.downscale_plane_layout == dict(good, frame_stride=E)
    planar = downscale_plane_layout_preset(W, H, "i420")
    assert L.m1v_set_downscale_plane_layout(enc._h, C.byref(S(**dict(planar, y_pitch=0, c_pitch=0, c_step=0)))) == 0
    assert enc.downscale_plane_layout == planar                                                      # the getter fills in: no zeros
    enc.set_downscale_plane_layout(dict(tight, c_pitch=0))
    assert enc.downscale_plane_layout == tight
    enc.set_downscale_plane_layout(good)
    # a table that another layout turned on is turned off by this setter, and a failed call leaves it on
    enc.set_rgb_plane_layout("rgb")
    enc.set_plane_table(True)
    assert L.m1v_set_downscale_plane_layout(enc._h, C.byref(S(**dict(good, factor=3)))) == _ffi.E_ARG
    assert enc.plane_table and enc.rgb_plane_layout is not None and enc.downscale_plane_layout is None
    enc.set_downscale_plane_layout(good)
    assert not enc.plane_table and not enc.frame_table and _encode(torch, enc, x, 0) == want
    enc.close()
    for size in ((105, 48), (104, 49)):                                                                 # an odd width, an odd height
        odd = Mpeg1Encoder(*size, 12, "full", max_frames=n)
        lay = S(**dict(tight, y_pitch=0, c_pitch=0, frame_stride=big))
        assert L.m1v_set_downscale_plane_layout(odd._h, C.byref(lay)) == _ffi.E_ARG and b"even width and height" in L.m1v_last_error()
        assert odd.downscale_plane_layout is None and odd.input_layout == (0, 0, "rgb")
        odd.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)                                     # channels != 3
    assert L.m1v_set_downscale_plane_layout(rgba._h, C.byref(S(**good))) == _ffi.E_ARG
    assert b"3 channels" in L.m1v_last_error() and rgba.downscale_plane_layout is None and rgba.path == "runs"
    rgba.close()
    assert L.m1v_set_downscale_plane_layout(None, C.byref(S(**good))) == _ffi.E_ARG                     # a null encoder
    assert L.m1v_last_error()
    forced = Mpeg1Encoder(W, H, 12, "full", max_frames=n)                                               # the run-kernel hooks
    forced.debug_set_path("runs")
    assert L.m1v_set_downscale_plane_layout(forced._h, C.byref(S(**good))) == _ffi.E_ARG
    assert b"hook" in L.m1v_last_error() and forced.downscale_plane_layout is None and forced.path == "runs"
    forced.debug_set_path("auto")
    forced.set_downscale_plane_layout(good)
    for hook in (lambda: forced.debug_set_path("runs"), lambda: forced.debug_set_input_mode(0)):
        with pytest.raises(EncoderError) as ei:
            hook()
        assert ei.value.code == _ffi.E_ARG and "downscale plane layout" in str(ei.value)
        assert forced.path == "tiles" and forced.downscale_plane_layout == good
    assert _encode(torch, forced, x, 0) == want
    forced.close()


def test_setters_getters_tables_and_packed_only_calls(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi, downscale_layout_preset, float_pixel_layout_preset
    from ec504_imageencoder_amd.encoder import downscale_plane_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 96, 80, 3
    src = _noise(W, H, n)
    frames = dp.model_frames(src)
    want = _oracle(orc, frames, W, H, "full", 5, 12)
    x, lay, _ = dp.place(torch, src, "nv21", **dp.PITCHED)
    i420 = torch.from_numpy(frames).cuda()
    packed = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    fresh = (enc.path, enc.size_table_fused, enc.scratch_bytes())
    assert enc.downscale_plane_layout is None and L.m1v_downscale_plane_layout_in_force(enc._h, None) == 0
    others = ((lambda: enc.set_plane_layout("i420"), i420), (lambda: enc.set_rgb_plane_layout("rgb"), None),
              (lambda: enc.set_input_layout(W * 3, 0, "bgr"), None), (lambda: enc.set_sample_layout("yuy2"), None),
              (lambda: enc.set_downscale_layout(downscale_layout_preset(W, H, 4)), None),
              (lambda: enc.set_float_plane_layout(dict(r_offset=0, g_offset=2 * W * H, b_offset=4 * W * H, row_pitch=2 * W,
                                                       frame_stride=6 * W * H, sample=_ffi.SAMPLE_F16, range=_ffi.RANGE_UNIT)), None),
              (lambda: enc.set_float_pixel_layout(float_pixel_layout_preset(W, H, 4, "float16", "bgr")), None))
    for set_other, tensor in others:
        enc.set_downscale_plane_layout(lay)                                 # ... -> downscale planes
        assert enc.downscale_plane_layout == lay and enc.downscale_layout is None and enc.rgb_plane_layout is None
        assert enc.float_plane_layout is None and enc.float_pixel_layout is None
        assert L.m1v_downscale_plane_layout_in_force(enc._h, None) == 1
        assert _encode(torch, enc, x, 5) == want
        for query in (lambda: enc.plane_layout, lambda: enc.sample_layout, lambda: enc.input_layout):
            with pytest.raises(EncoderError) as ei:
                query()
            assert ei.value.code == _ffi.E_ARG and "ask m1v_downscale_plane_layout_in_force" in str(ei.value)
        set_other()                                                         # downscale planes -> each other layout
        assert enc.downscale_plane_layout is None and L.m1v_downscale_plane_layout_in_force(enc._h, None) == 0
        if tensor is not None:
            assert _encode(torch, enc, tensor, 5) == want
    enc.set_downscale_plane_layout(lay)
    # the table modes refuse this kind, with a reason of their own, and stay off
    for setter in ("m1v_set_frame_table", "m1v_set_plane_table"):
        assert getattr(L, setter)(enc._h, 1) == _ffi.E_ARG
        assert b"downscale plane layout" in L.m1v_last_error() and b"not covered" in L.m1v_last_error()
        assert getattr(L, setter)(enc._h, 0) == _ffi.OK
    assert not enc.frame_table and not enc.plane_table
    with pytest.raises(AssertionError, match="downscale plane layout"):
        enc.frames([x[0]])
    with pytest.raises(AssertionError, match="downscale plane layout"):
        enc.plane_frames([(x[0], x[0], x[0])])
    # packed-only entry points refuse, naming the layout
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(packed.cpu().numpy())):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG and "downscale plane layout" in str(ei.value)
    # Python holds the tensor against the layout: another dtype, a row below the extent and another frame stride are refused
    E = downscale_plane_layout_extent(lay, enc.strips, enc.mb_rows)
    wider = torch.zeros((n, lay["frame_stride"] + 8), dtype=torch.uint8, device="cuda")
    assert _encode(torch, enc, x[:, :E], 5) == want
    for wrong in (x.float(), x.to(torch.int8), x[:, :E - 1], wider[:, :x.shape[1]], packed, i420):
        with pytest.raises(AssertionError):
            enc.encode(wrong)
    enc.set_downscale_plane_layout(None)                                    # downscale planes -> default: a fresh encoder's plan
    assert enc.downscale_plane_layout is None and enc.input_layout == (0, 0, "rgb")
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes()) == fresh
    out = torch.empty((n, W * H * 3 // 2), dtype=torch.uint8, device="cuda")    # the to-i420 call needs the layout
    assert L.m1v_downscale_planes_to_i420_device(enc._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == _ffi.E_ARG
    assert b"m1v_set_downscale_plane_layout" in L.m1v_last_error()
    enc.close()


# ---- 4. every served call once ------------------------------------------------------------------------------------------------------
def _pair(torch, preset, n):
    """(the encoder with the layout in force, its source view, an encoder under the I420 plane layout, the to-i420 bytes, the
    model's frames, the layout) at 48 x 32."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H = 48, 32
    src = _noise(W, H, n)
    xa, lay, _ = dp.place(torch, src, preset, fill_seed=4, **dp.PITCHED)
    a = _encoder(W, H, 12, n, lay)
    xb = a.downscale_planes_to_i420(xa)
    torch.cuda.synchronize()
    frames = dp.model_frames(src)
    assert np.array_equal(xb.cpu().numpy(), frames)
    b = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    b.set_plane_layout("i420")
    return a, xa, b, xb, frames, lay


@pytest.mark.parametrize("preset", ("i420", "nv12"))
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
        st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
        s = a.frame_sizes(xa, quality=[q] * n, status=st)
        a.flush()
        torch.cuda.synchronize()
        assert ([int(v) for v in s.cpu()], int(st.cpu()[0])) == (sizes[k], 0), q
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


@pytest.mark.parametrize("preset", ("yv12", "nv21"))
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


@pytest.mark.parametrize("preset", ("i420", "nv12"))
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
    assert a.downscale_plane_layout == lay
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
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    from ec504_imageencoder_amd.encoder import downscale_plane_layout_extent
    torch = torch_cuda
    L = _ffi.lib()
    for W, H, mode in ((40, 32, "full"), (112, 160, "strict")):
        src = _noise(W, H, 2)
        x, lay, _ = dp.place(torch, src, "nv12", **dp.PITCHED)
        enc = Mpeg1Encoder(W, H, 12, mode, max_frames=2)
        E = downscale_plane_layout_extent(lay, enc.strips, enc.mb_rows)
        assert E < x.shape[1] <= lay["frame_stride"]
        enc.set_downscale_plane_layout(dict(lay, frame_stride=E))
        full = _encode(torch, enc, x[:1], 0)
        out = torch.zeros((1, W * H * 3 // 2), dtype=torch.uint8, device="cuda")
        assert L.m1v_downscale_planes_to_i420_device(enc._h, C.c_void_p(x.data_ptr()), 1, C.c_void_p(out.data_ptr()), None) == _ffi.E_ARG
        assert b"whole source" in L.m1v_last_error() and b"frame stride below" in L.m1v_last_error()
        torch.cuda.synchronize()
        assert not out.any()
        enc.set_downscale_plane_layout(lay)
        assert _encode(torch, enc, x[:1], 0) == full
        assert np.array_equal(_i420_of(torch, enc, x), dp.model_frames(src))
        with pytest.raises(AssertionError, match="whole source"):
            enc.downscale_planes_to_i420(x[:, :E])
        enc.close()


def test_python_takes_presets_by_name_and_whole_tensors(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder, downscale_plane_layout_preset
    torch = torch_cuda
    W, H, n = 48, 32, 2
    src = _noise(W, H, n)
    want = _oracle(orc, dp.model_frames(src), W, H, "full", 0, 12, key=("noise", n))
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    for preset in dp.PRESETS:
        x = torch.from_numpy(dp.pack(src, preset)).cuda()       # a decoder's tightly packed surfaces, as they are
        enc.set_downscale_plane_layout(preset)
        assert enc.downscale_plane_layout == downscale_plane_layout_preset(W, H, preset)
        assert _encode(torch, enc, x, 0) == want, preset
        assert _encode(torch, enc, x[:1], 0) == (want[0][:want[1][0]], want[1][:1])
    with pytest.raises(ValueError):
        enc.set_downscale_plane_layout("reference")
    enc.close()
