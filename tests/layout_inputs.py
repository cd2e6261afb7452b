"""Per input layout kind — pitched surfaces, Y/Cb/Cr planes, sample layouts, RGB planes, float planes, float pixels, frame
tables and plane tables — the builders of its buffers of noise, the strided views into them, the layout records and the
encoders with the layout in force.  The GPU tests of each kind use their own; tests/input_families.py and
tests/test_stage_packing.py use those of every kind.  Where two kinds had a builder of the same name, it carries the kind in
front: _surface_geometry, _rgb_planes_geometry, _float_planes_geometry, _float_pixels_geometry; _float_planes_tensor,
_float_pixels_tensor; _sample_view beside the planes' _view."""
import numpy as np

import float_planes as fp
import sample_oracle
from gpu_calls import _encode, _frames, _table


def _surface_geometry(layout, W, H, C):
    """(row pitch, frame stride, byte offset of the window's first pixel in frame 0, bytes behind the last frame's stride)."""
    if layout == "packed":                      # pitch exactly W * C
        return W * C, H * W * C, 0, 0
    if layout == "odd":                         # pitch W * C + 1, the base at an odd address
        return W * C + 1, H * (W * C + 1), 1, 8
    if layout == "gap":                         # pitch W * C + 256 and a gap between the frames
        return W * C + 256, H * (W * C + 256) + 4099, 0, 0
    assert layout == "window", layout           # a window at odd (x0, y0) of a surface about twice as large
    SW, SH, x0, y0 = 2 * W + 6, 2 * H + 2, (W // 2) | 1, (H // 2) | 1
    return SW * C, SH * SW * C, (y0 * SW + x0) * C, 0


def _surface(torch, px, layout, order, fill_seed=0):
    """px: uint8 [n, H, W, C] in R,G,B(,A) order -> the strided CUDA view the encoder is given (bytes 0 and 2 swapped for
    "bgr"), over a buffer whose every other byte — row padding, the gaps, the surface around a window — is noise of
    fill_seed.  Returns (view, row pitch, frame stride)."""
    n, H, W, C_ = px.shape
    pitch, stride, off, tail = _surface_geometry(layout, W, H, C_)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 + fill_seed)
    buf = torch.randint(0, 256, (off + n * stride + tail + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    view = torch.as_strided(buf, (n, H, W, C_), (stride, pitch, C_, 1), off)
    packed = px if order == "rgb" else np.ascontiguousarray(px[..., [2, 1, 0] + ([3] if C_ == 4 else [])])
    view.copy_(torch.from_numpy(packed).cuda())
    if layout == "odd":
        assert view.data_ptr() % 2 == 1, view.data_ptr() % 2
    return view, pitch, stride


def _surface_encoder(W, H, Q, mode, channels, n, pitch, stride, order, pipelined=False):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, mode, channels=channels, max_frames=n)
    enc.set_input_layout(pitch, stride, order)
    assert enc.path == "tiles" and enc.size_table_fused == 1, (enc.path, enc.size_table_fused)
    assert enc.input_layout == (pitch, stride, order), (enc.input_layout, (pitch, stride, order))
    if pipelined:
        enc.set_pipelined(True)
        assert enc.path == "tiles" and enc.size_table_fused == 1, (enc.path, enc.size_table_fused)
    return enc


PRESETS = ("reference", "i420", "yv12", "nv12", "nv21")


def _region(W, H, mode):
    return (W & ~15, H & ~15) if mode == "full" else (96, 144)


def _layout(name, W, H):
    """(layout dict with no zeros, byte offset of frame 0 in the buffer)."""
    from ec504_imageencoder_amd import plane_layout_preset
    if name in PRESETS:
        return plane_layout_preset(W, H, name), 0
    hw, hh = W // 2, H // 2
    if name == "pitched":                       # both pitches + 256 and a gap between the frames
        yp, cp = W + 256, hw + 256
        cb = H * yp
        cr = cb + hh * cp
        return dict(y_offset=0, cb_offset=cb, cr_offset=cr, y_pitch=yp, c_pitch=cp, c_step=1, frame_stride=cr + hh * cp + 4099), 0
    if name == "odd":                           # base, offsets, pitches and stride odd
        yp, cp = (W + 1) | 1, (hw + 1) | 1
        cb = (3 + H * yp) | 1
        cr = (cb + hh * cp + 2) | 1
        return dict(y_offset=3, cb_offset=cb, cr_offset=cr, y_pitch=yp, c_pitch=cp, c_step=1, frame_stride=(cr + hh * cp + 8) | 1), 1
    assert name == "window", name               # a window at odd (x0, y0) of planes about twice as large
    SW, SH = 2 * W + 6, 2 * H + 2
    cw, ch = SW // 2, SH // 2
    x0, y0, cx0, cy0 = (W // 2) | 1, (H // 2) | 1, (W // 4) | 1, (H // 4) | 1
    return dict(y_offset=y0 * SW + x0, cb_offset=SW * SH + cy0 * cw + cx0, cr_offset=SW * SH + cw * ch + cy0 * cw + cx0,
                y_pitch=SW, c_pitch=cw, c_step=1, frame_stride=SW * SH + 2 * cw * ch), 0


def _buffer(torch, n, lay, base, fill_seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2000 + fill_seed)
    return torch.randint(0, 256, (base + n * lay["frame_stride"] + 64,), dtype=torch.uint8, device="cuda", generator=gen)


def _view(torch, buf, n, lay, base, enc):
    """The [n, L] tensor the encoder is given: row f = frame f, L = the bytes the frame's planes span."""
    from ec504_imageencoder_amd.encoder import plane_layout_extent
    L = plane_layout_extent(lay, enc.strips, enc.mb_rows)
    assert L <= lay["frame_stride"], (L, lay["frame_stride"])
    return torch.as_strided(buf, (n, L), (lay["frame_stride"], 1), base)


def _write_planes(torch, buf, lay, base, Y, Cb, Cr):
    """Y [n, rows, cols], Cb / Cr [n, rows / 2, cols / 2] (numpy) -> the samples the definition addresses, through the layout;
    every other byte of buf stays what it was."""
    n = Y.shape[0]
    s = lay["frame_stride"]
    torch.as_strided(buf, Y.shape, (s, lay["y_pitch"], 1), base + lay["y_offset"]).copy_(torch.from_numpy(np.ascontiguousarray(Y)).cuda())
    for plane, off in ((Cb, lay["cb_offset"]), (Cr, lay["cr_offset"])):
        torch.as_strided(buf, plane.shape, (s, lay["c_pitch"], lay["c_step"]), base + off).copy_(
            torch.from_numpy(np.ascontiguousarray(plane)).cuda())
    assert n == Cb.shape[0] == Cr.shape[0], (n, Cb.shape[0], Cr.shape[0])


def _addressed(orc, px, mode):
    """RGB frames [n, H, W, 3] -> the samples the encoder's region addresses: Y [n, ye, xe] and Cb, Cr [n, ye / 2, xe / 2] cut
    from the converted full-resolution planes read with stride W / 2 (encoder.h:347-348)."""
    n, H, W, _ = px.shape
    xe, ye = _region(W, H, mode)
    hw = W // 2
    Ys, Cbs, Crs = [], [], []
    for f in range(n):
        Y, Cb, Cr = orc.convert(px[f])
        Ys.append(Y.reshape(H, W)[:ye, :xe])
        Cbs.append(Cb[:(ye // 2) * hw].reshape(ye // 2, hw)[:, :xe // 2])
        Crs.append(Cr[:(ye // 2) * hw].reshape(ye // 2, hw)[:, :xe // 2])
    return np.stack(Ys), np.stack(Cbs), np.stack(Crs)


def _plane_encoder(W, H, Q, mode, n, lay, pipelined=False):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, mode, channels=3, max_frames=n)
    enc.set_plane_layout(lay)
    assert enc.path == "tiles" and enc.size_table_fused == 1, (enc.path, enc.size_table_fused)
    assert enc.plane_layout == lay, (enc.plane_layout, lay)
    if pipelined:
        enc.set_pipelined(True)
        assert enc.path == "tiles" and enc.plane_layout == lay, (enc.path, enc.plane_layout, lay)
    return enc


def _planes_of(torch, orc, px, mode, layout, fill_seed=0):
    """RGB frames -> (encoder input view, layout dict) in `layout`, over a buffer of noise."""
    n, H, W, _ = px.shape
    lay, base = _layout(layout, W, H)
    buf = _buffer(torch, n, lay, base, fill_seed)
    _write_planes(torch, buf, lay, base, *_addressed(orc, px, mode))
    return buf, lay, base


GUARD = 64


# which component (0 = R) each memory plane holds
_PLANES = {"rgb": (0, 1, 2), "bgr": (2, 1, 0), "gbr": (1, 2, 0)}


def _rgb_planes_geometry(layout, n, H, W):
    """(shape, strides, order) of the [n, C, H, W] view of `layout`, strides in bytes."""
    if layout in _PLANES:                       # tightly packed planes in that memory order
        return (n, 3, H, W), (3 * H * W, H * W, W, 1), layout
    if layout == "pitched":                     # pitch W + 13, 64 + 1 bytes between frames
        P = W + 13
        return (n, 3, H, W), (3 * H * P + 65, H * P, P, 1), "rgb"
    if layout == "rgba":                        # the first three planes of a 4-plane tensor
        return (n, 4, H, W), (4 * H * W, H * W, W, 1), "rgb"
    assert layout == "rows", layout             # planes interleaved by rows: row_pitch 3 W, offsets 0, W, 2 W
    return (n, 3, H, W), (3 * H * W, W, 3 * W, 1), "rgb"


def _planar(torch, px, layout, fill_seed=0, base=GUARD):
    """px: uint8 [n, H, W, 3] in R,G,B order -> (the strided CUDA view [n, C, H, W] the encoder is given, its layout dict), over a
    buffer whose every other byte — row padding, a fourth plane, the gaps between frames, GUARD bytes in front of the first and
    behind the last frame — is noise of fill_seed."""
    from ec504_imageencoder_amd import rgb_plane_strides
    n, H, W, _ = px.shape
    shape, strides, order = _rgb_planes_geometry(layout, n, H, W)
    span = sum(s * (d - 1) for s, d in zip(strides[1:], shape[1:])) + 1   # bytes from a frame's first to its last element
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2000 + fill_seed)
    buf = torch.randint(0, 256, (base + (n - 1) * strides[0] + span + GUARD,), dtype=torch.uint8, device="cuda", generator=gen)
    view = torch.as_strided(buf, shape, strides, base)
    comp = _PLANES.get(layout, (0, 1, 2))
    view[:, :3].copy_(torch.from_numpy(np.ascontiguousarray(px.transpose(0, 3, 1, 2)[:, comp])).cuda())
    return view, rgb_plane_strides(shape, strides, order)


_NP = {"float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}


def _float_planes_geometry(layout, n, H, W):
    """(shape, strides in elements, offset of the view in elements, which component each of the first three channels holds)."""
    if layout in ("rgb", "bgr"):                # tightly packed planes in that memory order
        return (n, 3, H, W), (3 * H * W, H * W, W, 1), 0, (0, 1, 2) if layout == "rgb" else (2, 1, 0)
    if layout == "rgba":                        # the first three planes of a 4-plane tensor
        return (n, 4, H, W), (4 * H * W, H * W, W, 1), 0, (0, 1, 2)
    assert layout == "window", layout           # x[:, :, 3:3+H, 5:5+W] of a [n, 4, H + 7, W + 13] tensor: an odd x0, a pitch that
    P, R = W + 13, H + 7                        # is no multiple of 16 bytes (W + 13 is odd), a fourth plane, rows between frames
    return (n, 4, H, W), (4 * R * P, R * P, P, 1), 3 * P + 5, (0, 1, 2)


def _float_planes_tensor(torch, bits, kind, layout, rng="unit", fill="noise", seed=0):
    """bits: patterns [n, 3, H, W] of R, G, B -> (the strided CUDA view [n, C, H, W] the encoder is given, its layout dict).
    Everything else of the buffer — row padding, a fourth plane, the gaps between frames, GUARD bytes either side — is noise of
    `seed`, or all-NaN patterns (every byte 0xff)."""
    from ec504_imageencoder_amd import float_plane_strides
    n, _, H, W = bits.shape
    S = fp.BYTES[kind]
    shape, strides, at, comp = _float_planes_geometry(layout, n, H, W)
    base = GUARD // S + at
    span = sum(s * (d - 1) for s, d in zip(strides, shape)) + 1
    total = base + span + GUARD // S
    if fill == "noise":
        buf = np.random.default_rng(3000 + seed).integers(0, 1 << (8 * S), total, dtype=np.uint64).astype(_NP[kind])
    else:
        buf = np.full(total, (1 << (8 * S)) - 1, dtype=_NP[kind])
    view = np.lib.stride_tricks.as_strided(buf[base:], shape, tuple(s * S for s in strides))
    for c in range(3):
        view[:, c] = bits[:, comp[c]]
    signed = {2: np.int16, 4: np.int32}[S]
    dtype = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[kind]
    dev = torch.from_numpy(buf.view(signed)).cuda().view(dtype)
    order = "bgr" if layout == "bgr" else "rgb"
    return torch.as_strided(dev, shape, strides, base), float_plane_strides(shape, strides, kind, order, rng)


def _float_pixels_geometry(form, n, H, W, Cs):
    """(strides in elements of the pixel array [n, H, W, Cs], offset of pixel (0, 0) of frame 0 in elements)."""
    if form in ("nhwc", "nchw"):
        return (H * W * Cs, W * Cs, Cs, 1), 0
    assert form == "window", form               # x[:, 3:3+H, 5:5+W, :3] of an [n, H + 7, W + 13, Cs] tensor: an odd x0, a pitch that
    P, R = W + 13, H + 7                        # is no multiple of 16 bytes, rows between frames
    return (R * P * Cs, P * Cs, Cs, 1), (3 * P + 5) * Cs


def _float_pixels_tensor(torch, bits, kind, form, Cs=3, order="rgb", rng="unit", fill="noise", seed=0, fourth=None):
    """bits: patterns [n, H, W, 3] of R, G, B -> (the strided CUDA view the encoder is given, its layout dict).  Everything else
    of the buffer — row padding, 4th samples, the gaps between frames, GUARD bytes either side — is noise of `seed`, or all-NaN
    patterns (every byte 0xff); fourth="nan" makes the 4th samples NaN under either fill."""
    from ec504_imageencoder_amd import float_pixel_strides
    n, H, W, _ = bits.shape
    S = fp.BYTES[kind]
    strides, at = _float_pixels_geometry(form, n, H, W, Cs)
    base = GUARD // S + at
    span = sum(s * (d - 1) for s, d in zip(strides, (n, H, W, Cs))) + 1
    total = base + span + GUARD // S
    if fill == "noise":
        buf = np.random.default_rng(3000 + seed).integers(0, 1 << (8 * S), total, dtype=np.uint64).astype(_NP[kind])
    else:
        buf = np.full(total, (1 << (8 * S)) - 1, dtype=_NP[kind])
    pixels = np.lib.stride_tricks.as_strided(buf[base:], (n, H, W, Cs), tuple(s * S for s in strides))
    pixels[..., :3] = bits if order == "rgb" else bits[..., ::-1]
    if Cs == 4 and fourth == "nan":
        pixels[..., 3] = (1 << (8 * S)) - 1
    signed = {2: np.int16, 4: np.int32}[S]
    dtype = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[kind]
    dev = torch.from_numpy(buf.view(signed)).cuda().view(dtype)
    if form == "nchw":
        shape, vstrides, dims = (n, Cs, H, W), (strides[0], 1, strides[1], strides[2]), "nchw"
    elif form == "window":
        shape, vstrides, dims = (n, H, W, 3), strides, "nhwc"
    else:
        shape, vstrides, dims = (n, H, W, Cs), strides, "nhwc"
    return torch.as_strided(dev, shape, vstrides, base), float_pixel_strides(shape, vstrides, kind, dims, order, rng)


def _noise(n, lay, base, seed, amp=256):
    """The host image of a buffer of n frames: noise everywhere (amp 64: 96..159, whose AC levels stay below 256 at any quality:
    a coefficient is at most 32 * (sum of |cos|)^2 / 4 < 32 * 6.6)."""
    rng = np.random.default_rng(seed)
    size = base + n * lay["frame_stride"] + GUARD
    return rng.integers(0, 256, size, dtype=np.uint8) if amp == 256 else (96 + rng.integers(0, amp, size)).astype(np.uint8)


def _sample_view(torch, dev, n, lay, base, enc):
    """The [n, L] tensor the encoder is given: row f = frame f, L = the frame's extent."""
    from ec504_imageencoder_amd.encoder import plane_layout_extent
    L = plane_layout_extent(lay, enc.strips, enc.mb_rows)
    assert L <= lay["frame_stride"] and base >= GUARD and base + (n - 1) * lay["frame_stride"] + L + GUARD <= dev.numel(), (
        L, lay["frame_stride"], base, GUARD, base + (n - 1) * lay["frame_stride"] + L + GUARD, dev.numel())
    return torch.as_strided(dev, (n, L), (lay["frame_stride"], 1), base)


def _scatter(host, lay, base, Y, Cb, Cr):
    """Y [n, H, W], Cb, Cr [n, H / 2, W / 2] into the bytes the definition addresses; every other byte stays."""
    for f in range(Y.shape[0]):
        fr = host[base + f * lay["frame_stride"]:]
        r, c = np.mgrid[0:Y.shape[1], 0:Y.shape[2]]
        fr[lay["y_offset"] + r * lay["y_pitch"] + c * lay["y_step"]] = Y[f]
        r, c = np.mgrid[0:Cb.shape[1], 0:Cb.shape[2]]
        fr[lay["cb_offset"] + r * lay["c_pitch"] + c * lay["c_step"]] = Cb[f]
        fr[lay["cr_offset"] + r * lay["c_pitch"] + c * lay["c_step"]] = Cr[f]


RESIDUES = (1, 6, 11, 0, 7, 13, 4, 15)      # a frame base's address mod 16, slot by slot
FIRST = 17


class _Pixels:
    """A layout whose frames are pictures [H, W, C]: a pitched surface, or pitched planes of R, G and B."""

    def pictures(self, rng, m, W, H, amp=256):
        px = _frames(rng, m, W, H, self.channels, amp)
        if self.channels == 4:              # alpha is noise: a kernel that reads it as a colour gets every size wrong
            px[..., 3] = rng.integers(0, 256, px.shape[:3], dtype=np.uint8)
        return list(px)

    def want(self, orc, pic, W, H, index, Q):
        return orc.encode_frame(pic, W, H, index, Q, orc.MODE_FULL, channels=self.channels)


class _Surface(_Pixels):
    def __init__(self, channels, pad, order):
        self.channels, self.pad, self.order = channels, pad, order

    def pitch(self, W):
        return W * self.channels + self.pad

    def span(self, W, H):
        return (H - 1) * self.pitch(W) + W * self.channels

    def encoder(self, W, H, Q, n, stride=0):
        from ec504_imageencoder_amd import Mpeg1Encoder
        enc = Mpeg1Encoder(W, H, Q, "full", channels=self.channels, max_frames=n)
        enc.set_input_layout(self.pitch(W), stride, self.order)
        return enc

    def view(self, torch, pool, base, W, H, n=None, stride=0):
        """The tensor of the frame at pool[base] (n: of the n frames `stride` apart from there), as the layout's calls take it."""
        one = (H, W, self.channels), (self.pitch(W), self.channels, 1)
        return torch.as_strided(pool, *(one if n is None else ((n,) + one[0], (stride,) + one[1])), base)

    def write(self, torch, pool, base, pic, W, H):
        src = pic if self.order == "rgb" else np.ascontiguousarray(pic[..., [2, 1, 0] + ([3] if self.channels == 4 else [])])
        self.view(torch, pool, base, W, H).copy_(torch.from_numpy(np.array(src)).cuda())


class _RgbPlanes(_Pixels):
    channels = 3

    def pitch(self, W):
        return W + 13

    def span(self, W, H):
        return 2 * H * self.pitch(W) + (H - 1) * self.pitch(W) + W

    def encoder(self, W, H, Q, n, stride=0):
        from ec504_imageencoder_amd import Mpeg1Encoder
        P = self.pitch(W)
        enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
        enc.set_rgb_plane_layout(dict(r_offset=0, g_offset=H * P, b_offset=2 * H * P, row_pitch=P, frame_stride=stride or 3 * H * P))
        return enc

    def view(self, torch, pool, base, W, H, n=None, stride=0):
        P = self.pitch(W)
        one = (3, H, W), (H * P, P, 1)
        return torch.as_strided(pool, *(one if n is None else ((n,) + one[0], (stride,) + one[1])), base)

    def write(self, torch, pool, base, pic, W, H):
        self.view(torch, pool, base, W, H).copy_(torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1))).cuda())


class _Samples:
    """A tightly packed plane or sample preset: a frame is its bytes, every one of which the definition addresses."""
    channels = 3

    def __init__(self, preset):
        self.preset = preset

    def layout(self, W, H):
        from ec504_imageencoder_amd import plane_layout_preset, sample_layout_preset
        if self.preset == "yuy2":
            return sample_layout_preset(W, H, "yuy2")
        return dict(plane_layout_preset(W, H, self.preset), y_step=1)

    def span(self, W, H):
        return self.layout(W, H)["frame_stride"]

    def encoder(self, W, H, Q, n, stride=0):
        from ec504_imageencoder_amd import Mpeg1Encoder
        enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
        enc.set_sample_layout(dict(self.layout(W, H), frame_stride=stride or self.span(W, H)))
        return enc

    def view(self, torch, pool, base, W, H, n=None, stride=0):
        L = self.span(W, H)
        return torch.as_strided(pool, *(((L,), (1,)) if n is None else ((n, L), (stride, 1))), base)

    def pictures(self, rng, m, W, H, amp=256):
        L = self.span(W, H)
        return [rng.integers(0, 256, L, dtype=np.uint8) if amp >= 256 else (128 - amp // 2 + rng.integers(0, amp, L)).astype(np.uint8)
                for _ in range(m)]

    def write(self, torch, pool, base, pic, W, H):
        self.view(torch, pool, base, W, H).copy_(torch.from_numpy(np.array(pic)).cuda())

    def want(self, orc, pic, W, H, index, Q):
        return sample_oracle.encode_layout(pic, self.layout(W, H), W, H, index, Q, orc.MODE_FULL)


def _picture_of(f):
    """Which picture frame f of a batch shows: frame 2 repeats frame 0's, so a batch of three or more names one address twice."""
    return 0 if f == 2 else f


def _addresses(torch, pool, bases):
    """A caller-built table: the int64 CUDA tensor of the frames' addresses."""
    return torch.tensor([pool.data_ptr() + b for b in bases], dtype=torch.int64).cuda()


def _check(torch, enc, table, recs, first=FIRST, Q=None):
    """encode, the size-table row and the rd-table row of the table against the oracle's records."""
    got, sizes = _encode(torch, enc, table, first)
    want = [len(r) for r in recs]
    assert sizes == want, [f for f in range(len(recs)) if sizes[f] != want[f]]
    at = np.concatenate([[0], np.cumsum(want)])
    wrong = [f for f in range(len(recs)) if got[at[f]:at[f + 1]] != recs[f]]
    assert not wrong and len(got) == at[-1], ("frames", wrong)
    Q = enc.quality_factor if Q is None else Q
    rows, status = _table(torch, enc, table, (Q,))
    assert status == [0] and rows == [want], (status, rows, [want])
    rd_sizes, _ = enc.frame_rd_table(table, (Q,))
    torch.cuda.synchronize()
    assert rd_sizes.cpu().numpy().tolist() == [want], (rd_sizes.cpu().numpy().tolist(), [want])


class _Ycc:
    """Y, Cb, Cr planes.  preset: the layout of the virtual contiguous frame, which the oracle reads.  chroma_offsets: None = the
    encoder gets the preset too (a plane's pointer then stands for the virtual frame's byte 0, and the plane's samples lie
    p_offset behind it); or the (cb, cr) offsets the encoder gets, with y_offset 0.  groups: the planes that share an allocation,
    each with the distance of its pointer from the allocation's first byte."""
    rgb = False

    def __init__(self, preset, groups, chroma_offsets=None):
        self.preset, self.groups, self.chroma_offsets = preset, groups, chroma_offsets

    def oracle_layout(self, W, H):
        from ec504_imageencoder_amd import plane_layout_preset
        return dict(plane_layout_preset(W, H, self.preset), y_step=1)

    def encoder_layout(self, W, H):
        lay = {k: v for k, v in self.oracle_layout(W, H).items() if k != "y_step"}
        if self.chroma_offsets is not None:
            lay.update(y_offset=0, cb_offset=self.chroma_offsets[0], cr_offset=self.chroma_offsets[1])
        return lay

    def encoder(self, W, H, Q, n, stride=0):
        from ec504_imageencoder_amd import Mpeg1Encoder
        enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
        enc.set_plane_layout(dict(self.encoder_layout(W, H), **({"frame_stride": stride} if stride else {})))
        return enc

    def pictures(self, rng, m, W, H, amp=256):
        L = self.oracle_layout(W, H)["frame_stride"]
        return [rng.integers(0, 256, L, dtype=np.uint8) if amp >= 256 else (128 - amp // 2 + rng.integers(0, amp, L)).astype(np.uint8)
                for _ in range(m)]

    def virtual(self, pic, W, H):
        return pic

    def want(self, orc, pic, W, H, index, Q):
        return sample_oracle.encode_layout(pic, self.oracle_layout(W, H), W, H, index, Q, orc.MODE_FULL)

    def planes(self, W, H, region=None):
        """Per plane (v, lo, E, A): the virtual frame's index the plane's pointer stands for, the range [lo, E) of the read
        contract relative to the pointer, and the virtual indices of the samples the definition addresses.  region: the coded
        region (xe, ye), by default W & ~15, H & ~15: the header's E_p counts ye rows of xe bytes for Y and ye / 2 rows of
        (xe / 2 - 1) * c_step + 1 bytes for Cb and Cr."""
        xe, ye = (W & ~15, H & ~15) if region is None else region
        o, e = self.oracle_layout(W, H), self.encoder_layout(W, H)
        r, c = np.arange(ye)[:, None], np.arange(xe)[None, :]
        out = [(o["y_offset"] - e["y_offset"], 0, e["y_offset"] + (ye - 1) * e["y_pitch"] + xe,
                (o["y_offset"] + r * o["y_pitch"] + c).reshape(-1))]
        r, c = np.arange(ye // 2)[:, None], np.arange(xe // 2)[None, :]
        for k in ("cb_offset", "cr_offset"):
            out.append((o[k] - e[k], 0, e[k] + (ye // 2 - 1) * e["c_pitch"] + (xe // 2 - 1) * e["c_step"] + 1,
                        (o[k] + r * o["c_pitch"] + c * o["c_step"]).reshape(-1)))
        return out


class _Rgb:
    """Pitched planes of R, G and B, `order` = which third of the virtual frame holds R, G and B.  A plane's range starts at its
    offset, so its pointer may stand c_offset in front of the allocation that holds it."""
    rgb = True
    groups = (((0, 0),), ((1, 0),), ((2, 0),))

    def __init__(self, order):
        self.order = order

    def pitch(self, W):
        return W + 13

    def encoder_layout(self, W, H):
        P = self.pitch(W)
        r, g, b = (self.order.index(ch) * H * P for ch in "rgb")
        return dict(r_offset=r, g_offset=g, b_offset=b, row_pitch=P, frame_stride=3 * H * P)

    def encoder(self, W, H, Q, n, stride=0):
        from ec504_imageencoder_amd import Mpeg1Encoder
        enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
        enc.set_rgb_plane_layout(dict(self.encoder_layout(W, H), **({"frame_stride": stride} if stride else {})))
        return enc

    def pictures(self, rng, m, W, H, amp=256):
        return list(_frames(rng, m, W, H, 3, amp))

    def virtual(self, pic, W, H):
        e = self.encoder_layout(W, H)
        v = np.zeros(e["frame_stride"], np.uint8)
        for ch, (_, _, _, A) in enumerate(self.planes(W, H)):
            v[A] = pic[..., ch].reshape(-1)
        return v

    def want(self, orc, pic, W, H, index, Q):
        return orc.encode_frame(pic, W, H, index, Q, orc.MODE_FULL, channels=3)

    def planes(self, W, H, region=None):
        """(An RGB plane's range is the layout's own, of the whole picture: width bytes of height rows, whatever the region.)"""
        e = self.encoder_layout(W, H)
        r, c = np.arange(H)[:, None], np.arange(W)[None, :]
        return [(0, e[k], e[k] + (H - 1) * e["row_pitch"] + W, (e[k] + r * e["row_pitch"] + c).reshape(-1))
                for k in ("r_offset", "g_offset", "b_offset")]


SEPARATE = (((0, 0),), ((1, 0),), ((2, 0),))


def _blocks(fam, W, H, region=None):
    """Per group (v0, length, [(plane, distance of its pointer from the block's first byte)], virtual indices written): the bytes
    of the virtual frame from v0 on that the block stands for."""
    planes = fam.planes(W, H, region)
    out = []
    for group in fam.groups:
        # (the group's pointers are d apart as the family says: [f][2] = [f][1] + 1 stands for virtual indices one apart)
        assert len({planes[p][0] - d for p, d in group}) == 1, group
        v0 = min(planes[p][0] + planes[p][1] for p, d in group)
        end = max(planes[p][0] + planes[p][2] for p, d in group)
        out.append((v0, end - v0, [(p, planes[p][0] - v0) for p, d in group], np.concatenate([planes[p][3] for p, d in group])))
    return out


def _device_table(torch, table):
    return torch.from_numpy(np.ascontiguousarray(table)).cuda()
