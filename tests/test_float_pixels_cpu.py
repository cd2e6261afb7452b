"""CPU checks of the float pixel layout's Python side (no GPU, no library): float_pixel_strides on the tensors the layout is for
and on what it refuses; a numpy model of the addressing of include/mpeg1_hip.h ("Float pixel layout") that reads a buffer through
a layout and gives back the bits it was built from; and the mask of the bytes the read contract names, under two fills of
everything else.  Content comes from input_families.float_bits and float_planes.rule_bytes."""
import numpy as np
import pytest

import float_planes as fp
import geometry_space as gs
import input_families as fam

N, H, W = 2, 32, 48
_NP = {"float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}


def _contiguous(shape):
    out, s = [], 1
    for d in reversed(shape):
        out.append(s)
        s *= d
    return tuple(reversed(out))


# ---- float_pixel_strides ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fp.KINDS)
def test_strides_of_the_tensors_the_layout_is_for(kind):
    from ec504_imageencoder_amd import _ffi, float_pixel_layout_preset, float_pixel_strides
    S = fp.BYTES[kind]
    codes = dict(sample=_ffi.FLOAT_SAMPLES[kind], range=0, order=0)
    for Cs in (3, 4):                                                       # packed [n, H, W, Cs]
        shape = (N, H, W, Cs)
        lay = float_pixel_strides(shape, _contiguous(shape), kind)
        assert lay == dict(row_pitch=W * Cs * S, frame_stride=H * W * Cs * S, pixel_step=Cs * S, **codes)
        assert lay == float_pixel_layout_preset(W, H, Cs, kind)
    # a channels-last [n, 3, H, W]: strides (H W 3, 1, W 3, 3)
    lay = float_pixel_strides((N, 3, H, W), (H * W * 3, 1, W * 3, 3), kind, dims="nchw", order="bgr", range="byte")
    assert lay == dict(float_pixel_layout_preset(W, H, 3, kind), order=1, range=1)
    assert float_pixel_strides((N, 4, H, W), (H * W * 4, 1, W * 4, 4), kind, dims="nchw") == float_pixel_layout_preset(W, H, 4, kind)
    # the window x[:, 3:3+H, 5:5+W, :3] of an [n, H + 7, W + 13, 4] tensor
    P, R = W + 13, H + 7
    lay = float_pixel_strides((N, H, W, 3), (R * P * 4, P * 4, 4, 1), kind)
    assert lay == dict(row_pitch=P * 4 * S, frame_stride=R * P * 4 * S, pixel_step=4 * S, **codes)
    # one frame: any stride, the layout takes the smallest
    lay = float_pixel_strides((1, H, W, 3), (12345, P * 4, 4, 1), kind)
    assert lay["frame_stride"] == ((H - 1) * P * 4 + W * 4) * S


def test_strides_value_errors():
    from ec504_imageencoder_amd import float_pixel_layout_preset, float_pixel_strides
    ok = ((N, H, W, 3), (H * W * 3, W * 3, 3, 1))
    float_pixel_strides(*ok, "float16")
    bad = [(((N, H, W), (H * W, W, 1)), {}),                                  # not 4-D
           (((N, H, W, 2), (H * W * 2, W * 2, 2, 1)), {}),                    # two channels
           (((N, H, W, 3), (H * W * 6, W * 6, 6, 2)), {}),                    # samples of a pixel not adjacent
           (((N, 3, H, W), (3 * H * W, H * W, W, 1)), dict(dims="nchw")),     # NCHW-contiguous: planes
           (((N, H, W, 3), (H * W * 5, W * 5, 5, 1)), {}),                    # a pixel stride of 5
           (((N, H, W, 3), (H * W * 2, W * 2, 2, 1)), {}),                    # a pixel stride below the channels
           (((N, H, W, 4), (H * W * 3, W * 3, 3, 1)), {}),                    # four channels three apart
           (((N, H, W, 3), (H * W * 3, W * 3 - 1, 3, 1)), {}),                # a row pitch below the row
           (((N, H, W, 3), (-H * W * 3, W * 3, 3, 1)), {}),                   # negative strides
           (ok, dict(dims="nwhc")), (ok, dict(order="gbr")), (ok, dict(order=(0, 1, 2))), (ok, dict(range="half"))]
    for (shape, strides), kw in bad:
        with pytest.raises(ValueError):
            float_pixel_strides(shape, strides, "float16", **kw)
    with pytest.raises(ValueError):
        float_pixel_strides(*ok, "float64")
    with pytest.raises(ValueError):
        float_pixel_strides(*ok, "uint8")
    for args in ((0, 16, 3, "float16"), (16, 0, 3, "float16"), (16, 16, 2, "float16"), (16, 16, 5, "float16"), (16, 16, 3, "int8")):
        with pytest.raises(ValueError):
            float_pixel_layout_preset(*args)


# ---- a numpy model of the addressing ----------------------------------------------------------------------------------------
def read_through(buf, base, lay, n, height, width):
    """The definition of include/mpeg1_hip.h: sample i of pixel (x, y) of frame f is the S bytes at
    base + f * frame_stride + y * row_pitch + x * pixel_step + i * S; samples 0, 1, 2 are R, G, B or B, G, R.  buf: uint8.
    Returns bit patterns [n, 3, height, width] of R, G, B."""
    S = 2 if lay["sample"] < 2 else 4
    f, y, x, i = np.meshgrid(np.arange(n), np.arange(height), np.arange(width), np.arange(3), indexing="ij")
    at = base + f * lay["frame_stride"] + y * lay["row_pitch"] + x * lay["pixel_step"] + i * S
    assert at.max() + S <= buf.size
    word = sum(buf[at + b].astype(np.uint32) << np.uint32(8 * b) for b in range(S))      # (little-endian)
    rgb = word if lay["order"] == 0 else word[..., ::-1]
    return rgb.transpose(0, 3, 1, 2).astype(np.uint16 if S == 2 else np.uint32)


def addressed_mask(length, base, lay, n, height, width):
    """The bytes the read contract names, [F + y * row_pitch, F + y * row_pitch + width * pixel_step) of every row, and of
    those the bytes of samples 0, 1, 2: (bytes that may be read, bytes that influence the output)."""
    S = 2 if lay["sample"] < 2 else 4
    may, used = np.zeros(length, bool), np.zeros(length, bool)
    for f in range(n):
        for y in range(height):
            row = base + f * lay["frame_stride"] + y * lay["row_pitch"]
            may[row:row + width * lay["pixel_step"]] = True
            for x in range(width):
                used[row + x * lay["pixel_step"]:row + x * lay["pixel_step"] + 3 * S] = True
    return may, used


def _buffer(bits, kind, Cs, form, order, fill_seed):
    """tests/test_gpu_float_pixels.py's _tensor on the host: (uint8 image of the buffer, byte offset of the view, layout)."""
    from ec504_imageencoder_amd import float_pixel_strides
    from layout_inputs import GUARD
    from layout_inputs import _float_pixels_geometry as _geometry
    n, h, w, _ = bits.shape
    S = fp.BYTES[kind]
    strides, at = _geometry(form, n, h, w, Cs)
    base = GUARD // S + at
    total = base + sum(s * (d - 1) for s, d in zip(strides, (n, h, w, Cs))) + 1 + GUARD // S
    buf = np.random.default_rng(3000 + fill_seed).integers(0, 1 << (8 * S), total, dtype=np.uint64).astype(_NP[kind])
    pixels = np.lib.stride_tricks.as_strided(buf[base:], (n, h, w, Cs), tuple(s * S for s in strides))
    pixels[..., :3] = bits if order == "rgb" else bits[..., ::-1]
    if form == "nchw":
        lay = float_pixel_strides((n, Cs, h, w), (strides[0], 1, strides[1], strides[2]), kind, "nchw", order)
    else:
        lay = float_pixel_strides((n, h, w, 3 if form == "window" else Cs), strides, kind, "nhwc", order)
    return buf.view(np.uint8), base * S, lay


@pytest.mark.parametrize("form", ["nhwc", "nchw", "window"])
@pytest.mark.parametrize("Cs", [3, 4])
@pytest.mark.parametrize("kind", fp.KINDS)
def test_the_model_gives_back_the_bits_and_the_mask_separates_the_fills(kind, Cs, form):
    t = gs.restricted(gs.batch_member(), kind + "-window")
    px = gs.pixels(t, "q12", 3, 2)
    for order, rng in (("rgb", "unit"), ("bgr", "byte")):
        planes = fam.float_bits(px, kind, rng, seed=Cs)
        bits = np.ascontiguousarray(planes.transpose(0, 2, 3, 1))
        a, base, lay = _buffer(bits, kind, Cs, form, order, fill_seed=1)
        got = read_through(a, base, lay, 2, t.H, t.W)
        assert np.array_equal(got, planes)
        assert np.array_equal(fp.rule_bytes(got, kind, rng).transpose(0, 2, 3, 1), px)
        # another fill changes padding, 4th samples, gaps and guards, and no addressed sample
        b = _buffer(bits, kind, Cs, form, order, fill_seed=2)[0]
        may, used = addressed_mask(a.size, base, lay, 2, t.H, t.W)
        assert np.array_equal(a[used], b[used]) and used.sum() == 2 * t.H * t.W * 3 * fp.BYTES[kind]
        assert not (used & ~may).any()
        if Cs == 4:
            fourth = may & ~used
            assert fourth.sum() == 2 * t.H * t.W * fp.BYTES[kind] and (a[fourth] != b[fourth]).mean() > 0.9
        else:
            assert np.array_equal(may, used)
        assert (a[~may] != b[~may]).mean() > 0.9
        assert (a[:64] != b[:64]).mean() > 0.9 and (a[-64:] != b[-64:]).mean() > 0.9 and not may[:64].any() and not may[-64:].any()
        if form == "window":            # row padding and the rows between frames exist, and none of them is addressed
            row = base + lay["row_pitch"]
            assert not may[base + t.W * lay["pixel_step"]:row].any()
            last = base + (t.H - 1) * lay["row_pitch"] + t.W * lay["pixel_step"]
            assert not may[last:base + lay["frame_stride"]].any() and last < base + lay["frame_stride"]
