"""GPU tests of the float plane layout (m1v_set_float_plane_layout; k_encode_float_planes, k_size_table_float_planes,
k_rd_table_float_planes, k_float_planes_to_bytes; -m gpu): NCHW tensors of float16, bfloat16 or float32 samples of R, G and B
encoded where they lie.

The rule (include/mpeg1_hip.h) is checked for equality on the bytes themselves (float_planes_to_bytes, the kernels' own
conversion function) against tests/float_planes.py, whose numpy rule tests/test_float_planes_cpu.py holds against exact
arithmetic; records are checked against the CPU oracle on the rule's bytes.  A float tensor is a device buffer of noise (or of
all-NaN patterns) into which the samples are written through the strided view the encoder is given; every frame lies 64 bytes
inside its allocation.  Every comparison is for equality and every status word is 0."""
import ctypes as C

import numpy as np
import pytest

import float_planes as fp
from gpu_calls import _encode, _table
from layout_inputs import _float_planes_tensor as _tensor

pytestmark = pytest.mark.gpu

# the sizes of tests/test_gpu_rgb_planes.py that differ in the lane-to-block map: one macroblock; 3 strips in one partial tile;
# a 2 x 2 tile grid with one strip in the last column; 17 strips
SIZES = ((16, 16), (48, 32), (144, 80), (272, 144))
LAYOUTS = ("rgb", "bgr", "window", "rgba")
K8 = (1, 2, 3, 5, 7, 9, 11, 12)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _encoder(W, H, Q, n, lay):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    enc.set_float_plane_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1 and enc.float_plane_layout == lay
    return enc


def _bytes_of(torch, enc, x):
    out = enc.float_planes_to_bytes(x)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _oracle(orc, px, first, Q):
    blob, sizes = orc.encode_frames(px, px.shape[0], px.shape[2], px.shape[1], first, Q, orc.MODE_FULL, threads=16)
    return blob, [int(s) for s in sizes]


# ---- 1. the rule, on the bytes call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["unit", "byte"])
@pytest.mark.parametrize("kind", fp.KINDS)
def test_rule_on_every_pattern(torch_cuda, kind, rng):
    """256 x 256 frames that hold every pattern of the type in each plane, in another order per plane.  float32: the fp32 images
    of all fp16 and all bf16 patterns, the 765 boundary values, every k + 0.5, the special values, and random patterns."""
    torch = torch_cuda
    g = np.random.default_rng(11)
    pats = fp.all_patterns(kind)
    if kind == "float32":
        pats = np.concatenate([pats, fp.boundary_values(), fp.ties_byte_range(kind), fp.special_f32()])
        pats = np.concatenate([pats, g.integers(0, 1 << 32, 3 * 65536 - len(pats), dtype=np.uint64).astype(np.uint32)])
    n = len(pats) // 65536
    bits = np.stack([g.permutation(pats).reshape(n, 256, 256) for _ in range(3)], axis=1)
    x, lay = _tensor(torch, bits, kind, "window", rng, seed=1)
    enc = _encoder(256, 256, 12, n, lay)
    got = _bytes_of(torch, enc, x)
    want = fp.rule_bytes(bits, kind, rng)
    assert got.shape == want.shape and got.dtype == np.uint8
    wrong = np.argwhere(got != want)
    assert not len(wrong), (len(wrong), [(hex(int(bits[tuple(w)])), int(got[tuple(w)]), int(want[tuple(w)])) for w in wrong[:8]])
    enc.close()


# ---- 2. parity with the oracle ------------------------------------------------------------------------------------------------
_noise_cache = {}


def _noise(orc, kind, size, Q, rng):
    """17 frames of jitter noise of that type and size, and the oracle's records of the rule's bytes as frames 17.."""
    key = (kind, size, Q, rng)
    if key not in _noise_cache:
        W, H = size
        bits, px = fp.jitter_noise(W * 1000 + H + Q, 17, H, W, kind, rng)
        blob, sizes = _oracle(orc, px, 17, Q)
        bits.setflags(write=False)
        _noise_cache[key] = (bits, blob, sizes)
    return _noise_cache[key]


def _check_parity(torch, orc, kind, size, layout, Q, n, rng, seed):
    W, H = size
    bits, blob, wsizes = _noise(orc, kind, size, Q, rng)
    x, lay = _tensor(torch, bits[:n], kind, layout, rng, seed=seed)
    enc = _encoder(W, H, Q, n, lay)
    got, sizes = _encode(torch, enc, x, 17)
    where = f"{kind} {layout} {W}x{H} quality {Q} batch {n} range {rng}"
    assert sizes == wsizes[:n], (where, [f for f in range(n) if sizes[f] != wsizes[f]])
    at = np.concatenate([[0], np.cumsum(wsizes)])
    wrong = [f for f in range(n) if got[at[f]:at[f + 1]] != blob[at[f]:at[f + 1]]]
    assert not wrong and len(got) == at[n], (where, "frames", wrong)
    table, status = _table(torch, enc, x, (Q,))
    assert status == [0] and table == [sizes], where
    rd_sizes, _ = enc.frame_rd_table(x, (Q,))
    torch.cuda.synchronize()
    assert rd_sizes.cpu().numpy().tolist() == [sizes], where
    enc.close()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", fp.KINDS)
def test_parity_every_type_and_size(torch_cuda, orc, kind, size):
    """Records, sizes and the size-table and rd-table rows of a window whose rows are only sample-aligned, 3 frames, quality 12."""
    _check_parity(torch_cuda, orc, kind, size, "window", 12, 3, "unit", SIZES.index(size))


@pytest.mark.parametrize("Q", [12, 77])             # byte staging, halfword staging
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["float16", "float32"])
def test_parity_every_layout_quality_and_batch(torch_cuda, orc, kind, layout, Q):
    """144 x 80, batches of 1, 9 and 17 (both branches of the workgroup -> (frame, tile) map); the range alternates."""
    for n in (1, 9, 17):
        rng = "byte" if (LAYOUTS.index(layout) + n) % 2 else "unit"
        _check_parity(torch_cuda, orc, kind, (144, 80), layout, Q, n, rng, n)


# ---- 3. the rule, through the front half --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [12, 100])
@pytest.mark.parametrize("kind", fp.KINDS)
def test_tie_picture_through_encode(torch_cuda, orc, kind, Q):
    """k + 0.5 as flat blocks, range byte: by tests/test_float_planes_cpu.py a front half that rounds ties up or down gives
    another record."""
    torch = torch_cuda
    samples, px = fp.tie_picture_samples(kind)
    x, lay = _tensor(torch, samples[None], kind, "rgb", "byte")
    enc = _encoder(256, 256, Q, 1, lay)
    assert np.array_equal(_bytes_of(torch, enc, x)[0].transpose(1, 2, 0), px)
    want = orc.encode_frame(np.ascontiguousarray(px), 256, 256, 3, Q, orc.MODE_FULL)
    assert _encode(torch, enc, x, 3) == (want, [len(want)])
    table, status = _table(torch, enc, x, (Q,))
    assert status == [0] and table == [[len(want)]]
    enc.close()


def test_boundary_values_through_encode(torch_cuda, orc):
    """The 765 fp32 values around the rounding boundaries of range unit as flat blocks, quality 100: a front half that takes the
    product in double, or floor(x * 255 + 0.5), gives another record (tests/test_float_planes_cpu.py)."""
    torch = torch_cuda
    samples, px = fp.boundary_picture()
    x, lay = _tensor(torch, samples[None], "float32", "bgr", "unit")
    enc = _encoder(256, 256, 100, 1, lay)
    want = orc.encode_frame(np.ascontiguousarray(px), 256, 256, 0, 100, orc.MODE_FULL)
    assert _encode(torch, enc, x, 0) == (want, [len(want)])
    enc.close()


# ---- 4. agreement of the two paths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fp.KINDS)
def test_float_layout_equals_rgb_plane_layout_on_its_bytes(torch_cuda, orc, kind):
    """encode, frame_sizes, the size and rd tables at K = 8, encode_best_in_budget, HostDelivery.step and pipelined mode: the float
    layout on x gives exactly what the RGB plane layout gives on float_planes_to_bytes(x)."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    W, H, n, first = 144, 80, 9, 40
    bits, _ = fp.jitter_noise(77, n, H, W, kind, "unit")
    xa, lay = _tensor(torch, bits, kind, "window", "unit", seed=4)
    a = _encoder(W, H, 12, n, lay)
    xb = a.float_planes_to_bytes(xa)
    torch.cuda.synchronize()
    assert np.array_equal(xb.cpu().numpy(), fp.rule_bytes(bits, kind, "unit"))
    b = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    b.set_rgb_plane_layout("rgb")
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

    def delivered(e, x):
        hd = HostDelivery(e, n)
        hd.step(x, first)
        hd.fence()
        out = (bytes(hd.result().numpy()), [int(v) for v in hd.frame_sizes(n)])
        hd.close()
        return out

    plain = both(lambda e, x: _encode(torch, e, x, first))
    both(lambda e, x: _encode(torch, e, x, first, quality=qs))
    assert both(sizes_of)[1] == 0
    table = both(lambda e, x: _table(torch, e, x, K8))
    assert table[1] == [0] * 8 and table[0][-1] == plain[1]
    rd = both(rd_of)
    assert rd[0] == table[0] and rd[2] == [0] * 8
    cap = sorted(v for row in table[0] for v in row)[4 * n]
    both(lambda e, x: e.encode_best_in_budget(x, cap, K8, first_frame_index=first))
    assert both(delivered) == plain
    for e in (a, b):
        e.set_pipelined(True)
    assert a.float_plane_layout == lay
    assert both(lambda e, x: (_encode(torch, e, x, first), _encode(torch, e, x[1:4], first + 1, quality=qs[1:4]),
                              _table(torch, e, x, K8)))[0] == plain
    a.close()
    b.close()


# ---- 5. nothing but addressed samples is used -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fp.KINDS)
def test_padding_is_never_used(torch_cuda, orc, kind):
    """The same samples under noise and under all-NaN patterns everywhere else (row padding, a fourth plane, the rows between
    frames, 64 guard bytes either side): identical bytes and records, the oracle's."""
    torch = torch_cuda
    W, H, n = 48, 32, 3
    bits, px = fp.jitter_noise(5, n, H, W, kind, "byte")
    want = _oracle(orc, px, 0, 12)
    for fill in ("noise", "nan"):
        x, lay = _tensor(torch, bits, kind, "window", "byte", fill=fill, seed=9)
        enc = _encoder(W, H, 12, n, lay)
        assert np.array_equal(_bytes_of(torch, enc, x), fp.rule_bytes(bits, kind, "byte")), fill
        assert _encode(torch, enc, x, 0) == want, fill
        assert _table(torch, enc, x, (12,)) == ([want[1]], [0]), fill
        enc.close()


@pytest.mark.parametrize("kind", fp.KINDS)
def test_special_values_as_pixels(torch_cuda, orc, kind):
    """NaN, +-inf, negatives, values above the range, -0.0 and denormals as pixels give the bytes the rule names (0, 255, 0, 255,
    0, 0) and a status word of 0 (_encode asserts it)."""
    torch = torch_cuda
    W, H, n = 144, 80, 2
    f32 = np.array([np.nan, np.inf, -np.inf, -0.25, -3.0e4, 1.5, 3.0e4, -0.0, 0.0, 0.5, 1.0], dtype=np.float32)
    if kind == "float16":
        specials = np.concatenate([f32.astype(np.float16).view(np.uint16), np.array([0x0001, 0x03ff, 0x8001, 0xfe01, 0x7d55], np.uint16)])
    elif kind == "bfloat16":
        specials = np.concatenate([(f32.view(np.uint32) >> 16).astype(np.uint16), np.array([0x0001, 0x007f, 0x8001, 0xff81, 0x7fa5], np.uint16)])
    else:
        specials = np.concatenate([f32.view(np.uint32), fp.special_f32()])
    bits = np.random.default_rng(8).choice(specials, (n, 3, H, W))
    want_bytes = fp.rule_bytes(bits, kind, "unit")
    assert set(np.unique(want_bytes).tolist()) == {0, 128, 255}
    x, lay = _tensor(torch, bits, kind, "rgba", "unit", seed=2)
    enc = _encoder(W, H, 12, n, lay)
    assert np.array_equal(_bytes_of(torch, enc, x), want_bytes)
    assert _encode(torch, enc, x, 0) == _oracle(orc, np.ascontiguousarray(want_bytes.transpose(0, 2, 3, 1)), 0, 12)
    enc.close()


# ---- 6. life cycle and refusals -------------------------------------------------------------------------------------------------
def test_setters_replace_each_other_and_tables_are_refused(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 144, 80, 2
    bits, px = fp.jitter_noise(6, n, H, W, "float16", "unit")
    want = _oracle(orc, px, 5, 12)
    x, lay = _tensor(torch, bits, "float16", "rgba", "unit")
    packed = torch.from_numpy(px).cuda()
    planar = torch.from_numpy(np.ascontiguousarray(px.transpose(0, 3, 1, 2))).cuda()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    fresh = (enc.path, enc.size_table_fused, enc.scratch_bytes())
    assert enc.float_plane_layout is None and L.m1v_float_plane_layout_in_force(enc._h, None) == 0
    others = ((lambda: enc.set_rgb_plane_layout("rgb"), planar), (lambda: enc.set_input_layout(W * 3, 0, "bgr"), None),
              (lambda: enc.set_plane_layout("i420"), None), (lambda: enc.set_sample_layout("yuy2"), None))
    for set_other, tensor in others:
        enc.set_float_plane_layout(lay)                                     # ... -> float planes
        assert enc.float_plane_layout == lay and enc.rgb_plane_layout is None
        assert _encode(torch, enc, x, 5) == want
        for query in (lambda: enc.plane_layout, lambda: enc.sample_layout, lambda: enc.input_layout):
            with pytest.raises(EncoderError) as ei:
                query()
            assert ei.value.code == _ffi.E_ARG and "m1v_float_plane_layout_in_force" in str(ei.value)
        set_other()                                                         # float planes -> each other layout
        assert enc.float_plane_layout is None
        if tensor is not None:
            assert _encode(torch, enc, tensor, 5) == want
    enc.set_float_plane_layout(lay)
    # the table modes refuse this kind, with the reason, and stay off
    for setter in ("m1v_set_frame_table", "m1v_set_plane_table"):
        assert getattr(L, setter)(enc._h, 1) == _ffi.E_ARG
        assert b"float plane layout" in L.m1v_last_error() and b"not covered" in L.m1v_last_error()
        assert getattr(L, setter)(enc._h, 0) == _ffi.OK
    assert not enc.frame_table and not enc.plane_table
    with pytest.raises(EncoderError):
        enc.set_frame_table(True)
    with pytest.raises(EncoderError):
        enc.set_plane_table(True)
    # a table that another layout turned on is turned off by the float setter, and a failed float setter leaves it on
    enc.set_rgb_plane_layout("rgb")
    enc.set_plane_table(True)
    assert L.m1v_set_float_plane_layout(enc._h, C.byref(_ffi.FloatPlaneLayout(**dict(lay, sample=7)))) == _ffi.E_ARG
    assert enc.plane_table and enc.rgb_plane_layout is not None
    enc.set_float_plane_layout(lay)
    assert not enc.plane_table and not enc.frame_table and _encode(torch, enc, x, 5) == want
    # packed-only entry points refuse, naming the layout
    for call in (lambda: enc.coefficients(packed), lambda: enc.convert(packed), lambda: enc.encode_host(px)):
        with pytest.raises(EncoderError) as ei:
            call()
        assert ei.value.code == _ffi.E_ARG and "float plane layout" in str(ei.value)
    enc.set_float_plane_layout(None)                                        # float planes -> default: a fresh encoder's plan
    assert enc.float_plane_layout is None and enc.input_layout == (0, 0, "rgb")
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes()) == fresh
    assert _encode(torch, enc, packed, 5) == want
    with pytest.raises(EncoderError):                                       # the bytes call needs the layout
        _call_bytes(enc, x, n)
    enc.close()


def _call_bytes(enc, x, n):
    import torch
    from ec504_imageencoder_amd import EncoderError, _ffi
    out = torch.empty((n, 3, enc.height, enc.width), dtype=torch.uint8, device="cuda")
    rc = _ffi.lib().m1v_float_planes_to_bytes_device(enc._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), None)
    if rc != _ffi.OK:
        raise EncoderError(rc, "m1v_float_planes_to_bytes_device")
    return out


@pytest.mark.parametrize("kind", ["float16", "float32"])
def test_argument_errors_leave_the_layout_in_force(torch_cuda, orc, kind):
    """Every M1V_E_ARG case of m1v_set_float_plane_layout, each with its reason; none changes the layout in force or the bytes.
    A misaligned d_rgb is refused by every call in front of its launch."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    L = _ffi.lib()
    W, H, n = 48, 32, 2
    S = fp.BYTES[kind]
    bits, px = fp.jitter_noise(9, n, H, W, kind, "unit")
    want = _oracle(orc, px, 0, 12)
    x, good = _tensor(torch, bits, kind, "window", "unit")
    P = good["row_pitch"]
    enc = _encoder(W, H, 12, n, good)
    big = 2 ** 40
    bad = [(dict(good, sample=3), b"sample type"), (dict(good, sample=-1), b"sample type"),
           (dict(good, range=2), b"range"), (dict(good, range=-1), b"range"),
           (dict(good, r_offset=good["r_offset"] + 1), b"multiples of the sample size"),
           (dict(good, g_offset=good["g_offset"] + S - 1), b"multiples of the sample size"),
           (dict(good, row_pitch=P + 1), b"multiples of the sample size"),
           (dict(good, frame_stride=good["frame_stride"] + S // 2), b"multiples of the sample size"),
           (dict(good, row_pitch=W * S - S), b"row pitch below"), (dict(good, row_pitch=0), b"row pitch below"),
           (dict(good, b_offset=2 ** 32 - (H - 1) * P - W * S, frame_stride=big), b"4 GiB"),
           (dict(good, r_offset=2 ** 32, frame_stride=big), b"4 GiB"), (dict(good, row_pitch=2 ** 32, frame_stride=big), b"4 GiB"),
           (dict(good, g_offset=good["r_offset"]), b"share bytes"), (dict(good, g_offset=good["r_offset"] + W * S - S), b"share bytes"),
           (dict(good, g_offset=good["r_offset"] + P + S), b"share bytes"),
           (dict(good, frame_stride=good["b_offset"] - good["r_offset"] + (H - 1) * P + W * S - S), b"frame stride below"),
           (dict(good, frame_stride=0), b"frame stride below")]
    for lay, reason in bad:
        assert L.m1v_set_float_plane_layout(enc._h, C.byref(_ffi.FloatPlaneLayout(**lay))) == _ffi.E_ARG, lay
        assert reason in L.m1v_last_error(), (lay, L.m1v_last_error())
        assert enc.float_plane_layout == good and enc.path == "tiles"
        with pytest.raises(EncoderError):
            enc.set_float_plane_layout(lay)
    assert _encode(torch, enc, x, 0) == want
    # the largest extent whose offsets are still 32-bit (only set here; encoded in tests/test_gpu_address_space.py), the smallest
    # stride, and planes interleaved by rows
    edge = 2 ** 32 - (H - 1) * P - W * S - S
    assert L.m1v_set_float_plane_layout(enc._h, C.byref(_ffi.FloatPlaneLayout(**dict(good, b_offset=edge, frame_stride=big)))) == 0
    least = good["b_offset"] - good["r_offset"] + (H - 1) * P + W * S
    assert L.m1v_set_float_plane_layout(enc._h, C.byref(_ffi.FloatPlaneLayout(**dict(good, frame_stride=least)))) == 0
    rows = dict(r_offset=0, g_offset=W * S, b_offset=2 * W * S, row_pitch=3 * W * S, frame_stride=3 * W * S * H, sample=good["sample"], range=1)
    assert L.m1v_set_float_plane_layout(enc._h, C.byref(_ffi.FloatPlaneLayout(**rows))) == 0
    assert enc.float_plane_layout == rows
    enc.set_float_plane_layout(good)
    # a pointer that is no multiple of the sample size: every call that takes d_rgb, in front of its launch
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(8 * n, dtype=torch.int64, device="cuda")
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = C.c_void_p(x.data_ptr() + S // 2)
    o, s, m = (C.c_void_p(t.data_ptr()) for t in (out, sizes, meta))
    assert L.m1v_encode_device(enc._h, off, n, 0, o, out.numel(), s, m, C.c_void_p(meta.data_ptr() + 8), None) == _ffi.E_ARG
    assert b"multiple of the sample size" in L.m1v_last_error()
    assert L.m1v_frame_sizes_device(enc._h, off, n, None, s, None, None) == _ffi.E_ARG
    quals = (C.c_uint8 * 2)(3, 12)
    assert L.m1v_frame_size_table_device(enc._h, off, n, quals, 2, s, None, None) == _ffi.E_ARG
    bytes_out = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
    assert L.m1v_float_planes_to_bytes_device(enc._h, off, n, C.c_void_p(bytes_out.data_ptr()), None) == _ffi.E_ARG
    torch.cuda.synchronize()
    assert _encode(torch, enc, x, 0) == want
    enc.close()
    odd = Mpeg1Encoder(105, 49, 12, "full", max_frames=n)                                               # an odd width
    lay = _ffi.FloatPlaneLayout(0, 105 * 49 * S, 2 * 105 * 49 * S, 105 * S, 3 * 105 * 49 * S, good["sample"], 0)
    assert L.m1v_set_float_plane_layout(odd._h, C.byref(lay)) == _ffi.E_ARG and b"even width" in L.m1v_last_error()
    assert odd.float_plane_layout is None and odd.input_layout == (0, 0, "rgb")
    odd.close()
    rgba = Mpeg1Encoder(W, H, 12, "full", channels=4, max_frames=n)                                     # channels != 3
    assert L.m1v_set_float_plane_layout(rgba._h, C.byref(_ffi.FloatPlaneLayout(**good))) == _ffi.E_ARG
    assert b"3 channels" in L.m1v_last_error() and rgba.float_plane_layout is None and rgba.path == "runs"
    rgba.close()


def test_python_checks_the_tensor_against_the_layout(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder, float_plane_layout_preset
    torch = torch_cuda
    W, H, n = 48, 32, 2
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    x16 = torch.rand((n, 3, H, W), device="cuda").half()
    # a float tensor under the default, surface and RGB plane layouts is refused, and the message names what the layout takes
    packed = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    for setup, shape in ((lambda: None, (n, H, W, 3)), (lambda: enc.set_input_layout(W * 3, 0, "bgr"), (n, H, W, 3)),
                         (lambda: enc.set_rgb_plane_layout("rgb"), (n, 3, H, W))):
        setup()
        with pytest.raises(AssertionError, match="torch.uint8 tensors, not torch.float16"):
            enc.encode(torch.zeros(shape, dtype=torch.float16, device="cuda"))
    enc.set_float_plane_layout(float_plane_layout_preset(W, H, "rgb", torch.float16))
    enc.encode(x16)
    enc.encode(x16[:1])
    torch.cuda.synchronize()
    for wrong in (x16.float(), x16.bfloat16(), (x16 * 255).to(torch.uint8), packed):
        with pytest.raises(AssertionError, match="takes torch.float16 tensors, not"):
            enc.encode(wrong)
        with pytest.raises(AssertionError, match="takes torch.float16 tensors, not"):
            enc.float_planes_to_bytes(wrong)
    big = torch.rand((n, 4, H + 2, W + 2), device="cuda").half()
    for view in (big[:, :3, :H, :W], x16.cpu(), x16[:, :, :, ::2], x16[:, :2], x16[0]):
        with pytest.raises(AssertionError):
            enc.encode(view)
    with pytest.raises(ValueError):
        enc.set_float_plane_layout(dict(r_offset=0))
    # three planes of a 4-plane tensor and a window go in as they are under their own layout
    from ec504_imageencoder_amd import float_plane_strides
    win = big[:, :, 1:1 + H, 1:1 + W]
    enc.set_float_plane_layout(float_plane_strides(tuple(win.shape), tuple(win.stride()), torch.float16, "bgr"))
    enc.encode(win)
    torch.cuda.synchronize()
    enc.close()
