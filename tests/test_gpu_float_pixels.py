"""GPU tests of the float pixel layout (m1v_set_float_pixel_layout; k_float_pixels_encode, k_float_pixels_size_table,
k_float_pixels_rd_table, k_float_pixels_to_bytes; -m gpu): [n, H, W, 3 | 4] and channels-last tensors of float16, bfloat16 or
float32 samples of R, G and B encoded where they lie.

The rule (include/mpeg1_hip.h, "Float plane layout") is checked for equality on the bytes themselves (float_pixels_to_bytes, the
kernels' own conversion function) against tests/float_planes.py; records are checked against the CPU oracle on the rule's bytes,
and the rate calls against the same calls on those bytes through the default packed layout.  A float tensor is a device buffer
of noise (or of all-NaN patterns) into which the samples are written through a strided view; every batch lies 64 bytes inside its
allocation.  Every comparison is for equality and every status word is 0."""
import ctypes as C

import numpy as np
import pytest

import float_planes as fp
from gpu_calls import _encode, _rd, _table
from layout_inputs import _float_pixels_tensor as _tensor

pytestmark = pytest.mark.gpu

# one macroblock; 3 strips in one partial tile; a 2 x 2 tile grid with one strip in the last column; 17 strips
SIZES = ((16, 16), (48, 32), (144, 80), (272, 144))
FORMS = ("nhwc", "nchw", "window")     # packed [n, H, W, C]; its channels-last view [n, C, H, W]; a window of a larger tensor
WIDTHS = (3, 4)                        # samples per pixel
ORDERS = ("rgb", "bgr")
K8 = (1, 2, 3, 5, 7, 9, 11, 12)
K8_WIDE = (20, 40, 60, 76, 77, 80, 85, 90)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(W, H, Q, n, lay):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    enc.set_float_pixel_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1 and enc.float_pixel_layout == lay
    return enc


def _bytes_of(torch, enc, x):
    out = enc.float_pixels_to_bytes(x)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _oracle(orc, px, first, Q):
    blob, sizes = orc.encode_frames(px, px.shape[0], px.shape[2], px.shape[1], first, Q, orc.MODE_FULL, threads=16)
    return blob, [int(s) for s in sizes]


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


# ---- 1. the rule, on the bytes call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", WIDTHS)
@pytest.mark.parametrize("rng", ["unit", "byte"])
@pytest.mark.parametrize("kind", fp.KINDS)
def test_rule_on_every_pattern(torch_cuda, kind, rng, Cs):
    """256 x 256 frames that hold every pattern of the type in each sample, in another order per sample, in the window layout.
    float32: the set of tests/test_gpu_float_planes.py."""
    torch = torch_cuda
    g = np.random.default_rng(11)
    pats = fp.all_patterns(kind)
    if kind == "float32":
        pats = np.concatenate([pats, fp.boundary_values(), fp.ties_byte_range(kind), fp.special_f32()])
        pats = np.concatenate([pats, g.integers(0, 1 << 32, 3 * 65536 - len(pats), dtype=np.uint64).astype(np.uint32)])
    n = len(pats) // 65536
    planes = np.stack([g.permutation(pats).reshape(n, 256, 256) for _ in range(3)], axis=1)
    bits = _nhwc(planes)
    order = ORDERS[(Cs + fp.KINDS.index(kind)) % 2]
    x, lay = _tensor(torch, bits, kind, "window", Cs, order, rng, seed=1)
    enc = _encoder(256, 256, 12, n, lay)
    got = _bytes_of(torch, enc, x)
    want = _nhwc(fp.rule_bytes(planes, kind, rng))
    assert got.shape == want.shape and got.dtype == np.uint8
    wrong = np.argwhere(got != want)
    assert not len(wrong), (len(wrong), [(hex(int(bits[tuple(w)])), int(got[tuple(w)]), int(want[tuple(w)])) for w in wrong[:8]])
    enc.close()


# ---- 2. parity with the oracle ------------------------------------------------------------------------------------------------
_noise_cache = {}


def _noise(orc, kind, size, Q, rng, n=3):
    """n frames of jitter noise of that type and size (amplitude 20 at quality 90, which every quality up to 90 can code):
    (patterns [n, H, W, 3], the rule's bytes, the oracle's records of those bytes as frames 17.. at quality Q, their sizes)."""
    key = (kind, size, Q, rng, n)
    if key not in _noise_cache:
        W, H = size
        planes, px = fp.jitter_noise(W * 1000 + H + Q, n, H, W, kind, rng, amplitude=256 if Q == 12 else 20)
        blob, sizes = _oracle(orc, px, 17, Q)
        bits = _nhwc(planes)
        bits.setflags(write=False)
        px.setflags(write=False)
        _noise_cache[key] = (bits, px, blob, sizes)
    return _noise_cache[key]


_table_cache = {}


def _oracle_tables(orc, kind, size, Q, rng, quals):
    import rd_oracle as rd
    key = (kind, size, Q, rng, quals)
    if key not in _table_cache:
        W, H = size
        px = _noise(orc, kind, size, Q, rng)[1]
        sizes = [_oracle(orc, px, 17, q)[1] for q in quals]
        dist = [[rd.frame_distortion(orc, px[f], W, H, q, orc.MODE_FULL, 3) for f in range(px.shape[0])] for q in quals]
        _table_cache[key] = (sizes, dist)
    return _table_cache[key]


@pytest.mark.parametrize("Q", [12, 90])             # narrow staging, wide staging
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("Cs", WIDTHS)
@pytest.mark.parametrize("kind", fp.KINDS)
def test_parity_with_the_oracle(torch_cuda, orc, kind, Cs, size, Q):
    """Both orders and the three forms at every type, pixel width and size: records, sizes, frame_sizes, the size table and the
    rd table (sizes and distortion) at K = 8, and per-frame qualities; the range alternates with the form."""
    torch = torch_cuda
    W, H = size
    quals = K8 if Q == 12 else K8_WIDE
    n = 3
    for order in ORDERS:
        for form in FORMS:
            rng = "byte" if (FORMS.index(form) + ORDERS.index(order)) % 2 else "unit"
            bits, px, blob, wsizes = _noise(orc, kind, size, Q, rng)
            tsizes, tdist = _oracle_tables(orc, kind, size, Q, rng, quals)
            x, lay = _tensor(torch, bits, kind, form, Cs, order, rng, seed=SIZES.index(size))
            enc = _encoder(W, H, Q, n, lay)
            where = f"{kind} x{Cs} {order} {form} {W}x{H} quality {Q} range {rng}"
            assert np.array_equal(_bytes_of(torch, enc, x), px), where
            got, sizes = _encode(torch, enc, x, 17)
            assert sizes == wsizes, (where, [f for f in range(n) if sizes[f] != wsizes[f]])
            at = np.concatenate([[0], np.cumsum(wsizes)])
            wrong = [f for f in range(n) if got[at[f]:at[f + 1]] != blob[at[f]:at[f + 1]]]
            assert not wrong and len(got) == at[n], (where, "frames", wrong)
            st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
            s = enc.frame_sizes(x, status=st)
            enc.flush()
            torch.cuda.synchronize()
            assert ([int(v) for v in s.cpu()], int(st.cpu()[0])) == (wsizes, 0), where
            assert _table(torch, enc, x, quals) == (tsizes, [0] * 8), where
            assert _rd(torch, enc, x, quals) == (tsizes, tdist, [0] * 8), where
            qs = [quals[(2 * f + 3) % 8] for f in range(n)]
            want = [_oracle(orc, px[f:f + 1], 17 + f, qs[f]) for f in range(n)]
            assert _encode(torch, enc, x, 17, quality=qs) == (b"".join(w[0] for w in want), [w[1][0] for w in want]), where
            enc.close()


# ---- 3. every served call equals the same call on the bytes through the default packed layout ---------------------------------
def _pair(torch, kind, Cs, W, H, n, Q, form="window", order="bgr", seed=4, amplitude=256):
    from ec504_imageencoder_amd import Mpeg1Encoder
    planes, px = fp.jitter_noise(77 + Cs, n, H, W, kind, "unit", amplitude=amplitude)
    xa, lay = _tensor(torch, _nhwc(planes), kind, form, Cs, order, "unit", seed=seed)
    a = _encoder(W, H, Q, n, lay)
    xb = a.float_pixels_to_bytes(xa)
    torch.cuda.synchronize()
    assert np.array_equal(xb.cpu().numpy(), px)
    b = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    return a, xa, b, xb, lay


CANDS = (2, 5, 8, 10, 12)


@pytest.mark.parametrize("Cs", WIDTHS)
@pytest.mark.parametrize("kind", fp.KINDS)
def test_rate_calls_equal_the_packed_layout_on_the_bytes(torch_cuda, kind, Cs):
    """The budget, rd, batch-budget and bitrate encodes, by size and by distortion, with limits from the size and rd tables so
    that the picks differ between frames."""
    torch = torch_cuda
    W, H, n, first = 144, 80, 6, 40
    a, xa, b, xb, _ = _pair(torch, kind, Cs, W, H, n, 12)

    def both(call):
        ra, rb = call(a, xa), call(b, xb)
        assert ra == rb
        return ra

    sizes, dist, status = both(lambda e, x: _rd(torch, e, x, CANDS))
    assert status == [0] * len(CANDS)
    cap = sorted(sizes[2])[n // 2]
    ceiling = sorted(dist[2])[n // 2]
    r = both(lambda e, x: e.encode_to_budget(x, cap, CANDS, first_frame_index=first))
    assert len(set(r[2])) > 1
    both(lambda e, x: e.encode_best_in_budget(x, cap, CANDS, first_frame_index=first))
    both(lambda e, x: e.encode_to_distortion(x, ceiling, CANDS, first_frame_index=first))
    B = (sum(sizes[2]) + sum(sizes[3])) // 2
    both(lambda e, x: e.encode_to_batch_budget(x, B, CANDS, first_frame_index=first))
    both(lambda e, x: e.encode_best_in_batch_budget(x, B, CANDS, first_frame_index=first))
    both(lambda e, x: e.encode_batch_to_distortion(x, (sum(dist[2]) + sum(dist[3])) // 2, CANDS, first_frame_index=first))

    def cbr(method):
        def call(e, x):
            level = torch.full((1,), 2 * cap, dtype=torch.int64, device="cuda")
            parts = [getattr(e, method)(x[i:i + 2], cap, 2 * cap, CANDS, level, first_frame_index=first + i) for i in (0, 2, 4)]
            return parts, int(level.cpu()[0])
        return call

    both(cbr("encode_at_bitrate"))
    both(cbr("encode_best_at_bitrate"))
    a.close()
    b.close()


@pytest.mark.parametrize("Cs", WIDTHS)
@pytest.mark.parametrize("kind", fp.KINDS)
def test_pipelined_delivery_and_fallback_equal_the_packed_layout(torch_cuda, kind, Cs):
    """Pipelined mode, HostDelivery.step (with its scratch retry: the arena is not reserved and the LDS image is 8 words, so the
    first attempt runs out of scratch), and the global-memory fallback with the worst-case arena reserved."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n, first = 144, 80, 9, 40
    a, xa, b, xb, lay = _pair(torch, kind, Cs, W, H, n, 12, form="nchw", order="rgb")
    qs = [int(q) for q in np.random.default_rng(3).integers(1, 13, n)]

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
    both(lambda e, x: _encode(torch, e, x, first, quality=qs))
    assert both(lambda e, x: _table(torch, e, x, K8))[1] == [0] * 8
    for e in (a, b):
        e.debug_set_lds_words(0)
        e.reserve_scratch(False)
        e.set_pipelined(True)
    assert a.float_pixel_layout == lay
    assert both(lambda e, x: (_encode(torch, e, x, first), _encode(torch, e, x[1:4], first + 1, quality=qs[1:4]),
                              _table(torch, e, x, K8)))[0] == plain
    # the profile counters count this layout's launches as they count the packed layout's
    for e in (a, b):
        e.set_pipelined(False)
        e.profile(True)
    both(lambda e, x: (_encode(torch, e, x, first), e.profile_read()[0]))        # (launches; the milliseconds differ)
    a.close()
    b.close()


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", WIDTHS)
@pytest.mark.parametrize("kind", fp.KINDS)
def test_batches(torch_cuda, orc, kind, Cs):
    """Batches of 7, 8, 9, 16 and 17 frames at 48 x 32 on an encoder of 17: both branches of the workgroup -> (frame, tile)
    map."""
    torch = torch_cuda
    W, H = 48, 32
    bits, px, blob, wsizes = _noise(orc, kind, (W, H), 12, "unit", n=17)
    x, lay = _tensor(torch, bits, kind, "window", Cs, "rgb", "unit", seed=7)
    enc = _encoder(W, H, 12, 17, lay)
    at = np.concatenate([[0], np.cumsum(wsizes)])
    for n in (7, 8, 9, 16, 17):
        assert _encode(torch, enc, x[:n], 17) == (blob[:at[n]], wsizes[:n]), n
        assert _table(torch, enc, x[:n], (12,)) == ([wsizes[:n]], [0]), n
        assert _rd(torch, enc, x[:n], (12,))[0] == [wsizes[:n]], n
    enc.close()


# ---- 5. the read contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", WIDTHS)
@pytest.mark.parametrize("kind", fp.KINDS)
def test_padding_and_fourth_samples_are_never_used(torch_cuda, orc, kind, Cs):
    """The same samples under noise and under all-NaN patterns everywhere else (row padding, 4th samples, the rows between
    frames, 64 guard bytes either side): identical bytes, records and tables, the oracle's."""
    torch = torch_cuda
    W, H, n = 48, 32, 3
    planes, px = fp.jitter_noise(5, n, H, W, kind, "byte")
    want = _oracle(orc, px, 0, 12)
    for fill in ("noise", "nan"):
        x, lay = _tensor(torch, _nhwc(planes), kind, "window", Cs, "bgr", "byte", fill=fill, seed=9)
        enc = _encoder(W, H, 12, n, lay)
        assert np.array_equal(_bytes_of(torch, enc, x), px), fill
        assert _encode(torch, enc, x, 0) == want, fill
        assert _table(torch, enc, x, (12,)) == ([want[1]], [0]), fill
        assert _rd(torch, enc, x, (12,))[0] == [want[1]], fill
        enc.close()


@pytest.mark.parametrize("kind", fp.KINDS)
def test_a_nan_fourth_sample_never_changes_a_byte(torch_cuda, kind):
    """Packed four-sample pixels of special values, the 4th sample noise or NaN: float_pixels_to_bytes gives the rule's bytes."""
    torch = torch_cuda
    W, H, n = 144, 80, 2
    f32 = np.array([np.nan, np.inf, -np.inf, -0.25, -3.0e4, 1.5, 3.0e4, -0.0, 0.0, 0.5, 1.0], dtype=np.float32)
    if kind == "float16":
        specials = f32.astype(np.float16).view(np.uint16)
    elif kind == "bfloat16":
        specials = (f32.view(np.uint32) >> 16).astype(np.uint16)
    else:
        specials = np.concatenate([f32.view(np.uint32), fp.special_f32()])
    planes = np.random.default_rng(8).choice(specials, (n, 3, H, W))
    want = _nhwc(fp.rule_bytes(planes, kind, "unit"))
    assert set(np.unique(want).tolist()) == {0, 128, 255}
    for fourth in (None, "nan"):
        x, lay = _tensor(torch, _nhwc(planes), kind, "nhwc", 4, "rgb", "unit", seed=2, fourth=fourth)
        enc = _encoder(W, H, 12, n, lay)
        assert np.array_equal(_bytes_of(torch, enc, x), want), fourth
        enc.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float16", "float32"])
def test_argument_errors_leave_the_layout_in_force(torch_cuda, orc, kind):
    """Every M1V_E_ARG case of m1v_set_float_pixel_layout, each with its reason; none changes the layout in force, the table
    mode or the records.  A misaligned d_rgb is refused by every call in front of its launch."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 48, 32, 2
    S = fp.BYTES[kind]
    planes, px = fp.jitter_noise(9, n, H, W, kind, "unit")
    want = _oracle(orc, px, 0, 12)
    x, good = _tensor(torch, _nhwc(planes), kind, "window", 4, "rgb", "unit")
    P, step = good["row_pitch"], good["pixel_step"]
    assert step == 4 * S
    enc = _encoder(W, H, 12, n, good)
    big = 2 ** 40
    bad = [(dict(good, order=2), b"order"), (dict(good, order=-1), b"order"),
           (dict(good, sample=3), b"sample type"), (dict(good, sample=-1), b"sample type"),
           (dict(good, range=2), b"range"), (dict(good, range=-1), b"range"),
           (dict(good, pixel_step=2 * S), b"pixel step"), (dict(good, pixel_step=5 * S), b"pixel step"),
           (dict(good, pixel_step=0), b"pixel step"), (dict(good, pixel_step=3 * S + 1), b"pixel step"),
           (dict(good, pixel_step=S), b"m1v_set_float_plane_layout"),
           (dict(good, row_pitch=P + 1), b"multiples of the sample size"),
           (dict(good, frame_stride=good["frame_stride"] + S // 2), b"multiples of the sample size"),
           (dict(good, row_pitch=W * step - S), b"row pitch below"), (dict(good, row_pitch=0), b"row pitch below"),
           (dict(good, row_pitch=(2 ** 32 - W * step) // (H - 1) // S * S + S, frame_stride=big), b"4 GiB"),
           (dict(good, row_pitch=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(good, frame_stride=(H - 1) * P + W * step - S), b"frame stride below"), (dict(good, frame_stride=0), b"frame stride below")]
    for lay, reason in bad:
        assert L.m1v_set_float_pixel_layout(enc._h, C.byref(_ffi.FloatPixelLayout(**lay))) == _ffi.E_ARG, lay
        assert reason in L.m1v_last_error(), (lay, L.m1v_last_error())
        assert enc.float_pixel_layout == good and enc.path == "tiles" and not enc.frame_table and not enc.plane_table
        with pytest.raises(EncoderError):
            enc.set_float_pixel_layout(lay)
    assert _encode(torch, enc, x, 0) == want
    # the largest extent whose offsets are still 32-bit (only set here; encoded in tests/test_gpu_address_space.py), and the
    # smallest stride
    edge = (2 ** 32 - 1 - W * step) // (H - 1) // S * S
    assert L.m1v_set_float_pixel_layout(enc._h, C.byref(_ffi.FloatPixelLayout(**dict(good, row_pitch=edge, frame_stride=big)))) == 0
    least = (H - 1) * P + W * step
    assert L.m1v_set_float_pixel_layout(enc._h, C.byref(_ffi.FloatPixelLayout(**dict(good, frame_stride=least)))) == 0
    assert enc.float_pixel_layout == dict(good, frame_stride=least)
    enc.set_float_pixel_layout(good)
    # a table that another layout turned on is turned off by this setter, and a failed call leaves it on
    enc.set_rgb_plane_layout("rgb")
    enc.set_plane_table(True)
    assert L.m1v_set_float_pixel_layout(enc._h, C.byref(_ffi.FloatPixelLayout(**dict(good, sample=7)))) == _ffi.E_ARG
    assert enc.plane_table and enc.rgb_plane_layout is not None and enc.float_pixel_layout is None
    enc.set_float_pixel_layout(good)
    assert not enc.plane_table and not enc.frame_table and _encode(torch, enc, x, 0) == want
    # a pointer that is no multiple of the sample size: every call that takes d_rgb, in front of its launch
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(8 * n, dtype=torch.int64, device="cuda")
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = C.c_void_p(x.data_ptr() + S // 2)
    o, s, m = (C.c_void_p(t.data_ptr()) for t in (out, sizes, meta))
    assert L.m1v_encode_device(enc._h, off, n, 0, o, out.numel(), s, m, C.c_void_p(meta.data_ptr() + 8), None) == _ffi.E_ARG
    assert b"multiple of the sample size" in L.m1v_last_error() and b"m1v_set_float_pixel_layout" in L.m1v_last_error()
    assert L.m1v_frame_sizes_device(enc._h, off, n, None, s, None, None) == _ffi.E_ARG
    quals = (C.c_uint8 * 2)(3, 12)
    assert L.m1v_frame_size_table_device(enc._h, off, n, quals, 2, s, None, None) == _ffi.E_ARG
    bytes_out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    assert L.m1v_float_pixels_to_bytes_device(enc._h, off, n, C.c_void_p(bytes_out.data_ptr()), None) == _ffi.E_ARG
    torch.cuda.synchronize()
    assert _encode(torch, enc, x, 0) == want
    enc.close()
    odd = Mpeg1Encoder(105, 49, 12, "full", max_frames=n)                                               # an odd width
    lay = _ffi.FloatPixelLayout(105 * 3 * S, 49 * 105 * 3 * S, 3 * S, 0, good["sample"], 0)
    assert L.m1v_set_float_pixel_layout(odd._h, C.byref(lay)) == _ffi.E_ARG and b"even width" in L.m1v_last_error()
    assert odd.float_pixel_layout is None and odd.input_layout == (0, 0, "rgb")
    odd.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)                                     # channels != 3
    assert L.m1v_set_float_pixel_layout(rgba._h, C.byref(_ffi.FloatPixelLayout(**good))) == _ffi.E_ARG
    assert b"3 channels" in L.m1v_last_error() and rgba.float_pixel_layout is None and rgba.path == "runs"
    rgba.close()
    assert L.m1v_set_float_pixel_layout(None, C.byref(_ffi.FloatPixelLayout(**good))) == _ffi.E_ARG     # a null encoder
    forced = Mpeg1Encoder(W, H, 12, "full", max_frames=n)                                               # the run-kernel hooks
    forced.debug_set_path("runs")
    assert L.m1v_set_float_pixel_layout(forced._h, C.byref(_ffi.FloatPixelLayout(**good))) == _ffi.E_ARG
    assert b"hook" in L.m1v_last_error() and forced.float_pixel_layout is None and forced.path == "runs"
    forced.debug_set_path("auto")
    forced.set_float_pixel_layout(good)
    with pytest.raises(EncoderError) as ei:
        forced.debug_set_path("runs")
    assert ei.value.code == _ffi.E_ARG and forced.path == "tiles" and forced.float_pixel_layout == good
    forced.close()


def test_setters_getters_tables_and_packed_only_calls(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 144, 80, 2
    planes, px = fp.jitter_noise(6, n, H, W, "float16", "unit")
    want = _oracle(orc, px, 5, 12)
    x, lay = _tensor(torch, _nhwc(planes), "float16", "nhwc", 4, "bgr", "unit")
    packed = torch.from_numpy(px).cuda()
    planar = torch.from_numpy(np.ascontiguousarray(px.transpose(0, 3, 1, 2))).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    fresh = (enc.path, enc.size_table_fused, enc.scratch_bytes())
    assert enc.float_pixel_layout is None and L.m1v_float_pixel_layout_in_force(enc._h, None) == 0
    others = ((lambda: enc.set_rgb_plane_layout("rgb"), planar), (lambda: enc.set_input_layout(W * 3, 0, "bgr"), None),
              (lambda: enc.set_plane_layout("i420"), None), (lambda: enc.set_sample_layout("yuy2"), None))
    for set_other, tensor in others:
        enc.set_float_pixel_layout(lay)                                     # ... -> float pixels
        assert enc.float_pixel_layout == lay and enc.rgb_plane_layout is None and enc.float_plane_layout is None
        assert L.m1v_float_pixel_layout_in_force(enc._h, None) == 1
        assert _encode(torch, enc, x, 5) == want
        for query in (lambda: enc.plane_layout, lambda: enc.sample_layout, lambda: enc.input_layout):
            with pytest.raises(EncoderError) as ei:
                query()
            assert ei.value.code == _ffi.E_ARG and "m1v_float_pixel_layout_in_force" in str(ei.value)
        set_other()                                                         # float pixels -> each other layout
        assert enc.float_pixel_layout is None
        if tensor is not None:
            assert _encode(torch, enc, tensor, 5) == want
    enc.set_float_pixel_layout(lay)
    # the table modes refuse this kind, with the reason, and stay off
    for setter in ("m1v_set_frame_table", "m1v_set_plane_table"):
        assert getattr(L, setter)(enc._h, 1) == _ffi.E_ARG
        assert b"float pixel layout" in L.m1v_last_error() and b"not covered" in L.m1v_last_error()
        assert getattr(L, setter)(enc._h, 0) == _ffi.OK
    assert not enc.frame_table and not enc.plane_table
    with pytest.raises(AssertionError, match="float pixel layout"):
        enc.frames([x[0]])
    with pytest.raises(AssertionError, match="float pixel layout"):
        enc.plane_frames([(x[0], x[0], x[0])])
    # packed-only entry points refuse, naming the layout
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(px)):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG and "float pixel layout" in str(ei.value)
    enc.set_float_pixel_layout(None)                                        # float pixels -> default: a fresh encoder's plan
    assert enc.float_pixel_layout is None and enc.input_layout == (0, 0, "rgb")
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes()) == fresh
    assert _encode(torch, enc, packed, 5) == want
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")       # the bytes call needs the layout
    assert L.m1v_float_pixels_to_bytes_device(enc._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == _ffi.E_ARG
    assert b"m1v_set_float_pixel_layout" in L.m1v_last_error()
    enc.close()


def test_python_checks_the_tensor_against_the_layout(torch_cuda):
    from ec504_imageencoder_amd import Mpeg1Encoder, float_pixel_layout_preset, float_pixel_strides
    torch = torch_cuda
    W, H, n = 48, 32, 2
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    x16 = torch.rand((n, H, W, 3), device="cuda").half()
    enc.set_float_pixel_layout(float_pixel_layout_preset(W, H, 3, torch.float16))
    enc.encode(x16)
    enc.encode(x16[:1])
    enc.encode(x16.permute(0, 3, 1, 2))                                     # the channels-last view of the same memory
    nchw = torch.rand((n, 3, H, W), device="cuda").half()
    enc.encode(nchw.contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    for wrong in (x16.float(), x16.bfloat16(), (x16 * 255).to(torch.uint8)):
        with pytest.raises(AssertionError, match="takes torch.float16 tensors, not"):
            enc.encode(wrong)
        with pytest.raises(AssertionError, match="takes torch.float16 tensors, not"):
            enc.float_pixels_to_bytes(wrong)
    big = torch.rand((n, H + 2, W + 2, 4), device="cuda").half()
    for view in (nchw, big[:, :H, :W, :3], x16.cpu(), x16[:, :, ::2], x16[..., :2], x16[0]):
        with pytest.raises(AssertionError):
            enc.encode(view)
    with pytest.raises(ValueError):
        enc.set_float_pixel_layout(dict(row_pitch=0))
    # a window of a four-sample tensor goes in as it is under its own layout, unless the storage ends inside its last pixel
    win = big[:, 1:1 + H, 1:1 + W, :3]
    enc.set_float_pixel_layout(float_pixel_strides(tuple(win.shape), tuple(win.stride()), torch.float16, "nhwc", "bgr"))
    enc.encode(win)
    torch.cuda.synchronize()
    flat = torch.rand(n * (H + 2) * (W + 2) * 4 - 1, device="cuda").half()   # one sample short of the last pixel's 4th
    short = torch.as_strided(flat, (n, H + 2, W + 2, 3), ((H + 2) * (W + 2) * 4, (W + 2) * 4, 4, 1))[:, 2:, 2:]
    assert tuple(short.stride()) == tuple(win.stride())
    with pytest.raises(AssertionError, match="storage ends inside the last pixel"):
        enc.encode(short)
    enc.close()


def test_an_injected_allocation_failure_leaves_everything(torch_cuda, orc):
    """m1v_debug_fail_alloc (EC504_DEBUG_HOOKS=1) and the setter.  The tile plan of this layout is the default plan of a 3-channel
    encoder, so the setter finds every allocation in place and has none to fail: the armed failure stays armed and meets the
    next reconfiguration (m1v_reserve_scratch), which returns M1V_E_HIP and leaves the layout, the plan and the records as they
    were."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 144, 80, 2
    planes, px = fp.jitter_noise(6, n, H, W, "float32", "unit")
    want = _oracle(orc, px, 0, 12)
    x, lay = _tensor(torch, _nhwc(planes), "float32", "nhwc", 4, "rgb", "unit")
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=40)     # 160 tiles: the worst-case arena is larger than the default one
    L.m1v_debug_fail_alloc(1)
    try:
        enc.set_float_pixel_layout(lay)                                     # nothing to allocate
        before = (enc.float_pixel_layout, enc.path, enc.scratch_bytes())
        assert before[0] == lay
        with pytest.raises(EncoderError) as ei:
            enc.reserve_scratch(True)                                       # the armed failure
        assert ei.value.code == _ffi.E_HIP
        assert (enc.float_pixel_layout, enc.path, enc.scratch_bytes()) == before
        assert _encode(torch, enc, x, 0) == want
    finally:
        L.m1v_debug_fail_alloc(0)
    enc.reserve_scratch(True)                                               # disarmed: the same call goes through
    assert enc.float_pixel_layout == lay and _encode(torch, enc, x, 0) == want
    enc.set_float_pixel_layout(None)
    assert enc.float_pixel_layout is None
    enc.close()
