"""Host-side mirror of the reference's operator for this path.

The reference has one operator, `mpeg_encode_procedure(images_folder, bitstream_folder, video_path,
quality_factor)` (include/encoder.h:20), whose per-frame body is the hot path.  `Mpeg1Encoder` is
that body as a batched device operator: frames in (HBM-resident uint8 RGB), contiguous frame
records out, both as torch CUDA tensors.  torch is plumbing here (device memory, streams); all
arithmetic happens in libencoder.so's HIP kernels.
"""
import ctypes as C
import numbers
from collections import namedtuple

from . import _ffi


class EncoderError(RuntimeError):
    def __init__(self, code, where):
        super().__init__(f"{where}: rc={code}: {_ffi.last_error()}")
        self.code = code


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    """The C entry point `name`, whose success value is OK; EncoderError otherwise."""
    rc = getattr(_ffi.lib(), name)(*args)
    if rc != _ffi.OK:
        raise EncoderError(rc, name)


def _meta_ptrs(meta):
    """Where the entry points write a batch's total bytes and its status word: the two elements of meta."""
    return C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8)


def surface_strides(shape, strides):
    """(row_pitch, frame_stride) in bytes of a uint8 [n, H, W, C] array with the given strides (in elements = bytes), as
    Mpeg1Encoder.set_input_layout takes them: a packed tensor, rows with padding, a window surface[:, y0:y0+H, x0:x0+W, :] of a
    larger surface, frames with a gap.  Raises ValueError for what no row pitch describes: pixels whose bytes are not adjacent
    or whose stride is not C, a pitch below W * C, a frame stride below the bytes a frame's window spans.  Pure: no torch."""
    if len(shape) != 4 or len(strides) != 4:
        raise ValueError("frames must be [n, H, W, C]")
    n, H, W, C = (int(x) for x in shape)
    frame_stride, row_pitch, pixel, byte = (int(x) for x in strides)
    if byte != 1 or pixel != C:
        raise ValueError(f"the bytes of a pixel must be adjacent and pixels {C} bytes apart (strides {pixel}, {byte})")
    if row_pitch < W * C:
        raise ValueError(f"row pitch {row_pitch} below W * C = {W * C}")
    if n > 1 and frame_stride < (H - 1) * row_pitch + W * C:
        raise ValueError(f"frame stride {frame_stride} below the {(H - 1) * row_pitch + W * C} bytes a frame's window spans")
    if n <= 1:  # (a single frame's stride is arbitrary)
        frame_stride = H * row_pitch
    return row_pitch, frame_stride


RGB_PLANE_LAYOUT_FIELDS = ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")
# which channel of an [n, C, H, W] tensor holds R, G and B, by the planes' order in memory
_RGB_PLANE_CHANNELS = {"rgb": (0, 1, 2), "bgr": (2, 1, 0), "gbr": (2, 0, 1)}


def rgb_plane_layout_preset(width, height, name):
    """The tightly packed RGB plane layout `name` ("rgb", "bgr", "gbr": the planes' order in memory) of a width x height frame
    as a dict of RGB_PLANE_LAYOUT_FIELDS in bytes, as Mpeg1Encoder.set_rgb_plane_layout takes it (include/mpeg1_hip.h,
    m1v_rgb_plane_layout_preset, whose values these are).  Pure: no torch, no library."""
    W, H = int(width), int(height)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if name not in _RGB_PLANE_CHANNELS:
        raise ValueError(f"unknown RGB plane order {name!r}")
    r, g, b = _RGB_PLANE_CHANNELS[name]
    return dict(r_offset=r * W * H, g_offset=g * W * H, b_offset=b * W * H, row_pitch=W, frame_stride=3 * W * H)


def rgb_plane_strides(shape, strides, order="rgb"):
    """The RGB plane layout (a dict of RGB_PLANE_LAYOUT_FIELDS in bytes, as Mpeg1Encoder.set_rgb_plane_layout takes it) of a uint8
    [n, C, H, W] array with the given strides (in elements = bytes): a packed NCHW tensor, a window x[:, :, y0:y0+H, x0:x0+W] of a
    larger one, three planes of a 4-plane tensor, frames with a gap.  order: "rgb", "bgr" or "gbr" = the order of the first three
    channels, or the three channel indices of R, G and B.  Offsets count from the array's first byte.  Raises ValueError for what
    the layout does not describe: fewer than 3 channels, bytes of a row that are not adjacent, a pitch below W.  Pure: no torch."""
    if len(shape) != 4 or len(strides) != 4:
        raise ValueError("frames must be [n, C, H, W]")
    n, C, H, W = (int(x) for x in shape)
    frame_stride, plane, row_pitch, byte = (int(x) for x in strides)
    channels = _RGB_PLANE_CHANNELS.get(order, order) if isinstance(order, str) else tuple(int(c) for c in order)
    if not isinstance(channels, tuple) or len(channels) != 3:
        raise ValueError(f"unknown RGB plane order {order!r}")
    if C < 3 or any(c < 0 or c >= C for c in channels):
        raise ValueError(f"channels {channels} of a tensor with {C}")
    if byte != 1:
        raise ValueError(f"the bytes of a row must be adjacent (stride {byte})")
    if row_pitch < W:
        raise ValueError(f"row pitch {row_pitch} below W = {W}")
    if plane < 0 or frame_stride < 0:
        raise ValueError("negative strides")
    offsets = [c * plane for c in channels]
    if n <= 1:  # (a single frame's stride is arbitrary)
        frame_stride = max(offsets) + (H - 1) * row_pitch + W
    return dict(r_offset=offsets[0], g_offset=offsets[1], b_offset=offsets[2], row_pitch=row_pitch, frame_stride=frame_stride)


FLOAT_PLANE_LAYOUT_FIELDS = RGB_PLANE_LAYOUT_FIELDS + ("sample", "range")


def _float_sample(dtype):
    """The SAMPLE_* code of "float16", "bfloat16", "float32" or the torch dtype of that name (no torch needed)."""
    name = dtype if isinstance(dtype, str) else str(dtype).rsplit(".", 1)[-1]
    if name not in _ffi.FLOAT_SAMPLES:
        raise ValueError(f"a float plane layout takes float16, bfloat16 or float32 samples, not {dtype!r}")
    return _ffi.FLOAT_SAMPLES[name]


def _float_range(range):
    if range not in _ffi.FLOAT_RANGES:
        raise ValueError(f"unknown range {range!r}: \"unit\" (0.0 ... 1.0) or \"byte\" (0 ... 255)")
    return _ffi.FLOAT_RANGES[range]


def float_plane_layout_preset(width, height, order, dtype, range="unit"):
    """The tightly packed float plane layout of a width x height frame as a dict of FLOAT_PLANE_LAYOUT_FIELDS (bytes, and the
    SAMPLE_* / RANGE_* codes), as Mpeg1Encoder.set_float_plane_layout takes it (include/mpeg1_hip.h,
    m1v_float_plane_layout_preset, whose values these are).  order: "rgb", "bgr", "gbr" = the planes' order in memory; dtype:
    "float16", "bfloat16", "float32" or the torch dtype; range: "unit" (samples 0.0 ... 1.0) or "byte" (0 ... 255).  Pure."""
    sample = _float_sample(dtype)
    S = _ffi.FLOAT_SAMPLE_BYTES[sample]
    layout = {k: v * S for k, v in rgb_plane_layout_preset(width, height, order).items()}
    return dict(layout, sample=sample, range=_float_range(range))


def float_plane_strides(shape, strides, dtype, order="rgb", range="unit"):
    """The float plane layout (a dict of FLOAT_PLANE_LAYOUT_FIELDS, as Mpeg1Encoder.set_float_plane_layout takes it) of a float
    [n, C, H, W] array with the given strides in elements, as torch gives them: a packed NCHW tensor, a window
    x[:, :, y0:y0+H, x0:x0+W] of a larger one, three planes of a 4-plane tensor.  dtype, order and range as in
    float_plane_layout_preset; order may also be the three channel indices of R, G and B.  Raises ValueError for what
    rgb_plane_strides refuses.  Pure: no torch."""
    sample = _float_sample(dtype)
    S = _ffi.FLOAT_SAMPLE_BYTES[sample]
    layout = {k: v * S for k, v in rgb_plane_strides(shape, strides, order).items()}
    return dict(layout, sample=sample, range=_float_range(range))


FLOAT_PIXEL_LAYOUT_FIELDS = ("row_pitch", "frame_stride", "pixel_step", "order", "sample", "range")


def _pixel_order(order):
    if order not in _ffi.PIXEL_ORDERS:
        raise ValueError(f"unknown pixel order {order!r}: \"rgb\" or \"bgr\" (samples 0, 1, 2 of a pixel)")
    return _ffi.PIXEL_ORDERS[order]


def float_pixel_layout_preset(width, height, pixel_samples, dtype, order="rgb", range="unit"):
    """The tightly packed float pixel layout of a width x height frame of pixel_samples (3 or 4) float samples per pixel as a dict
    of FLOAT_PIXEL_LAYOUT_FIELDS (bytes, and the ORDER_* / SAMPLE_* / RANGE_* codes), as Mpeg1Encoder.set_float_pixel_layout takes
    it (include/mpeg1_hip.h, m1v_float_pixel_layout_preset, whose values these are).  dtype: "float16", "bfloat16", "float32" or the
    torch dtype; order: "rgb" or "bgr" = samples 0, 1, 2 of a pixel (a 4th is skipped); range: "unit" or "byte".  Pure."""
    W, H, samples = int(width), int(height), int(pixel_samples)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if samples not in (3, 4):
        raise ValueError("a pixel has 3 or 4 samples")
    sample = _float_sample(dtype)
    step = samples * _ffi.FLOAT_SAMPLE_BYTES[sample]
    return dict(row_pitch=W * step, frame_stride=H * W * step, pixel_step=step, order=_pixel_order(order), sample=sample,
                range=_float_range(range))


def float_pixel_strides(shape, strides, dtype, dims="nhwc", order="rgb", range="unit"):
    """The float pixel layout (a dict of FLOAT_PIXEL_LAYOUT_FIELDS, as Mpeg1Encoder.set_float_pixel_layout takes it) of a 4-D float
    array with the given strides in elements, as torch gives them.  dims="nhwc": an [n, H, W, C] array — a packed tensor of 3 or 4
    samples per pixel, a window x[:, y0:y0+H, x0:x0+W, :3] of a larger one; dims="nchw": an [n, C, H, W] array with channels-last
    strides (torch.channels_last).  dtype, order and range as in float_pixel_layout_preset.  Raises ValueError for what the layout
    does not describe: fewer than 3 channels, a channel stride other than 1, a pixel stride other than 3 or 4 elements or below
    C, a row pitch below W pixels, negative strides.  Pure: no torch."""
    if len(shape) != 4 or len(strides) != 4:
        raise ValueError("frames must be 4-D: [n, H, W, C], or [n, C, H, W] with channels-last strides")
    if dims == "nhwc":
        (n, H, W, C), (frame, row, pixel, channel) = (int(x) for x in shape), (int(x) for x in strides)
    elif dims == "nchw":
        (n, C, H, W), (frame, channel, row, pixel) = (int(x) for x in shape), (int(x) for x in strides)
    else:
        raise ValueError(f"unknown dims {dims!r}: \"nhwc\" or \"nchw\"")
    sample = _float_sample(dtype)
    S = _ffi.FLOAT_SAMPLE_BYTES[sample]
    if C < 3:
        raise ValueError(f"a pixel needs 3 colour samples, not {C}")
    if channel != 1:
        raise ValueError(f"the samples of a pixel must be adjacent (channel stride {channel}): planar frames go through float_plane_strides")
    if pixel not in (3, 4) or pixel < C:
        raise ValueError(f"pixels must lie 3 or 4 samples apart and hold their {C} channels (pixel stride {pixel})")
    if row < W * pixel:
        raise ValueError(f"row pitch {row} below W * pixel stride = {W * pixel}")
    if frame < 0:
        raise ValueError("negative strides")
    if n <= 1:  # (a single frame's stride is arbitrary)
        frame = (H - 1) * row + W * pixel
    return dict(row_pitch=row * S, frame_stride=frame * S, pixel_step=pixel * S, order=_pixel_order(order), sample=sample,
                range=_float_range(range))


DOWNSCALE_LAYOUT_FIELDS = ("row_pitch", "frame_stride", "pixel_step", "order", "factor")


def downscale_layout_preset(width, height, pixel_bytes, order="rgb", factor=2):
    """The downscale layout of a tightly packed 2 * width x 2 * height source of pixel_bytes (3 or 4) bytes per pixel, for an
    encoder of the rendition's width x height, as a dict of DOWNSCALE_LAYOUT_FIELDS (bytes, the ORDER_* code and the factor), as
    Mpeg1Encoder.set_downscale_layout takes it (include/mpeg1_hip.h, m1v_downscale_layout_preset, whose values these are).
    order: "rgb" or "bgr" = bytes 0, 1, 2 of a source pixel (a 4th is skipped); factor: 2.  Pure."""
    W, H, step = int(width), int(height), int(pixel_bytes)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if step not in (3, 4):
        raise ValueError("a source pixel has 3 or 4 bytes")
    code = _pixel_order(order)
    if int(factor) != 2:
        raise ValueError("factor must be 2 (other factors are not covered)")
    return dict(row_pitch=2 * W * step, frame_stride=2 * H * 2 * W * step, pixel_step=step, order=code, factor=2)


def downscale_strides(shape, strides, dims="nhwc", order="rgb"):
    """The downscale layout (a dict of DOWNSCALE_LAYOUT_FIELDS, as Mpeg1Encoder.set_downscale_layout takes it) of a 4-D uint8
    SOURCE array with the given strides in elements (= bytes), as torch gives them, for an encoder of half its width and height.
    dims="nhwc": an [n, 2H, 2W, C] array — a packed tensor of 3 or 4 bytes per pixel, a window x[:, y0:y0+2H, x0:x0+2W, :3] of
    a larger one; dims="nchw": an [n, C, 2H, 2W] array with channels-last strides.  Raises ValueError for what the layout does not
    describe: an odd extent, fewer than 3 channels, a channel stride other than 1, a pixel stride other than 3 or 4 or below C, a
    row pitch below 2W pixels, negative strides.  Pure: no torch."""
    if len(shape) != 4 or len(strides) != 4:
        raise ValueError("source frames must be 4-D: [n, 2H, 2W, C], or [n, C, 2H, 2W] with channels-last strides")
    if dims == "nhwc":
        (n, H2, W2, C), (frame, row, pixel, channel) = (int(x) for x in shape), (int(x) for x in strides)
    elif dims == "nchw":
        (n, C, H2, W2), (frame, channel, row, pixel) = (int(x) for x in shape), (int(x) for x in strides)
    else:
        raise ValueError(f"unknown dims {dims!r}: \"nhwc\" or \"nchw\"")
    if H2 <= 0 or W2 <= 0 or H2 % 2 or W2 % 2:
        raise ValueError(f"a source of odd or empty extent ({W2} x {H2}) is not covered")
    if C < 3:
        raise ValueError(f"a pixel needs 3 colour bytes, not {C}")
    if channel != 1:
        raise ValueError(f"the bytes of a pixel must be adjacent (channel stride {channel})")
    if pixel not in (3, 4) or pixel < C:
        raise ValueError(f"source pixels must lie 3 or 4 bytes apart and hold their {C} channels (pixel stride {pixel})")
    if row < W2 * pixel:
        raise ValueError(f"row pitch {row} below 2W * pixel stride = {W2 * pixel}")
    if frame < 0:
        raise ValueError("negative strides")
    if n <= 1:  # (a single frame's stride is arbitrary)
        frame = (H2 - 1) * row + W2 * pixel
    return dict(row_pitch=row, frame_stride=frame, pixel_step=pixel, order=_pixel_order(order), factor=2)


def distortion_to_psnr(d, blocks):
    """The distortion d of a frame of `blocks` blocks (Mpeg1Encoder.blocks_per_frame = strips * mb_rows * 6) as a PSNR in dB:
    10 * log10(255^2 * 64 * blocks / d), the coefficient-domain squared error read as a pixel-domain one (the FDCT is scaled like
    the orthonormal transform).  inf for d == 0.  Pure: no torch, no library."""
    import math
    if d < 0 or blocks <= 0:
        raise ValueError("need d >= 0 and blocks > 0")
    return math.inf if d == 0 else 10.0 * math.log10(255.0 ** 2 * 64 * blocks / d)


def psnr_to_distortion(db, blocks):
    """The largest integer distortion whose distortion_to_psnr is at least db (up to floating-point rounding of the power): the
    ceiling a caller of Mpeg1Encoder.encode_to_distortion states in dB.  Pure."""
    if blocks <= 0:
        raise ValueError("need blocks > 0")
    return int(255.0 ** 2 * 64 * blocks / 10.0 ** (db / 10.0))


PLANE_LAYOUT_FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")


def plane_layout_preset(width, height, name):
    """The tightly packed plane layout `name` ("reference", "i420", "yv12", "nv12", "nv21") of a width x height frame as a dict
    of PLANE_LAYOUT_FIELDS in bytes, as Mpeg1Encoder.set_plane_layout takes it (include/mpeg1_hip.h, m1v_plane_layout_preset,
    whose values these are).  "reference" = the three full-resolution planes Mpeg1Encoder.convert writes.  Pure: no torch, no
    library."""
    W, H = int(width), int(height)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if name not in _ffi.PLANE_PRESETS:
        raise ValueError(f"unknown plane layout preset {name!r}")
    luma = W * H
    if name == "reference":
        return dict(y_offset=0, cb_offset=luma, cr_offset=2 * luma, y_pitch=W, c_pitch=W // 2, c_step=1, frame_stride=3 * luma)
    if W % 2 or H % 2:
        raise ValueError("a 4:2:0 preset needs an even width and height")
    planar, cr_first = name in ("i420", "yv12"), name in ("yv12", "nv21")
    second = (W // 2) * (H // 2) if planar else 1
    return dict(y_offset=0, cb_offset=luma + (second if cr_first else 0), cr_offset=luma + (0 if cr_first else second),
                y_pitch=W, c_pitch=W // 2 if planar else W, c_step=1 if planar else 2, frame_stride=luma * 3 // 2)


SAMPLE_LAYOUT_FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "y_step", "c_step", "frame_stride")


def sample_layout_preset(width, height, name):
    """The tightly packed sample layout `name` ("yuy2", "uyvy", "yvyu", "p010") of a width x height frame as a dict of
    SAMPLE_LAYOUT_FIELDS in bytes, as Mpeg1Encoder.set_sample_layout takes it (include/mpeg1_hip.h, m1v_sample_layout_preset,
    whose values these are).  The packed 4:2:2 presets take chroma from the even picture rows; "p010" also serves P012 and P016
    (the coded sample is the high byte of each 16-bit word).  Pure: no torch, no library."""
    W, H = int(width), int(height)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if name not in _ffi.SAMPLE_PRESETS:
        raise ValueError(f"unknown sample layout preset {name!r}")
    if W % 2 or H % 2:
        raise ValueError("a sample layout preset needs an even width and height")
    if name == "p010":
        return dict(y_offset=1, cb_offset=2 * W * H + 1, cr_offset=2 * W * H + 3, y_pitch=2 * W, c_pitch=2 * W, y_step=2, c_step=4,
                    frame_stride=3 * W * H)
    y, cb, cr = {"yuy2": (0, 1, 3), "uyvy": (1, 0, 2), "yvyu": (0, 3, 1)}[name]
    return dict(y_offset=y, cb_offset=cb, cr_offset=cr, y_pitch=2 * W, c_pitch=4 * W, y_step=2, c_step=4, frame_stride=2 * W * H)


def plane_layout_extent(layout, strips, mb_rows):
    """Bytes of a frame the plane kernels may read (the read contract of include/mpeg1_hip.h): the largest
    offset + (rows - 1) * pitch + row bytes over the three planes of the strips * 16 x mb_rows * 16 region (row bytes: up to a
    row's last addressed byte, (samples - 1) * step + 1).  layout: a dict of PLANE_LAYOUT_FIELDS (y_step = 1) or
    SAMPLE_LAYOUT_FIELDS with no zeros (Mpeg1Encoder.plane_layout, Mpeg1Encoder.sample_layout)."""
    xe, ye = strips * 16, mb_rows * 16
    luma = (ye - 1) * layout["y_pitch"] + (xe - 1) * layout.get("y_step", 1) + 1
    chroma = (ye // 2 - 1) * layout["c_pitch"] + (xe // 2 - 1) * layout["c_step"] + 1
    return max(layout["y_offset"] + luma, max(layout["cb_offset"], layout["cr_offset"]) + chroma)


DOWNSCALE_PLANE_LAYOUT_FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride", "factor", "reserved")


def downscale_plane_layout_preset(width, height, name, factor=2):
    """The downscale plane layout of a tightly packed 2 * width x 2 * height 4:2:0 source `name` ("i420", "yv12", "nv12", "nv21"),
    for an encoder of the rendition's width x height, as a dict of DOWNSCALE_PLANE_LAYOUT_FIELDS (bytes of the SOURCE, the factor
    and a reserved 0), as Mpeg1Encoder.set_downscale_plane_layout takes it (include/mpeg1_hip.h,
    m1v_downscale_plane_layout_preset, whose values these are).  The reference-style planes are not a source.  Pure."""
    W, H = int(width), int(height)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if name == "reference":
        raise ValueError("the reference-style 4:4:4 planes are not a source of a downscale plane layout")
    if name not in _ffi.PLANE_PRESETS:
        raise ValueError(f"unknown plane layout preset {name!r}")
    if W % 2 or H % 2:
        raise ValueError("a downscale plane layout needs an even width and height")
    if int(factor) != 2:
        raise ValueError("factor must be 2 (other factors are not covered)")
    return dict(plane_layout_preset(2 * W, 2 * H, name), factor=2, reserved=0)


def downscale_plane_layout_extent(layout, strips, mb_rows):
    """Bytes of a SOURCE frame the downscaled plane kernels may read (the read contract of include/mpeg1_hip.h): the plane
    layout's extent taken on the source, rows = 2 * ye (luma) and ye (chroma), row bytes = 2 * xe (luma) and
    (xe - 1) * c_step + 1 (chroma) for the strips * 16 x mb_rows * 16 region.  layout: a dict of DOWNSCALE_PLANE_LAYOUT_FIELDS
    with no zeros (Mpeg1Encoder.downscale_plane_layout)."""
    xe, ye = strips * 16, mb_rows * 16
    luma = (2 * ye - 1) * layout["y_pitch"] + 2 * xe
    chroma = (ye - 1) * layout["c_pitch"] + (xe - 1) * layout["c_step"] + 1
    return max(layout["y_offset"] + luma, max(layout["cb_offset"], layout["cr_offset"]) + chroma)


DOWNSCALE_WORD_LAYOUT_FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride", "factor", "shift")


def downscale_word_layout_preset(width, height, name, factor=2):
    """The downscale word layout of a tightly packed 2 * width x 2 * height 4:2:0 source of 16-bit little-endian words, `name` one of
    "p010", "p012", "p016" (a luma plane and a plane of Cb, Cr word pairs, the value in the high bits: shift 8), "i010", "i012"
    (yuv420p10le, yuv420p12le: three planes, the value in the low bits: shift 2, 4) or "i016" (yuv420p16le: shift 8), for an encoder
    of the rendition's width x height, as a dict of DOWNSCALE_WORD_LAYOUT_FIELDS (bytes of the SOURCE, the factor and the shift), as
    Mpeg1Encoder.set_downscale_word_layout takes it (include/mpeg1_hip.h, m1v_downscale_word_layout_preset, whose values these
    are).  Pure."""
    W, H = int(width), int(height)
    if W <= 0 or H <= 0:
        raise ValueError("bad geometry")
    if name not in _ffi.WORD_PRESETS:
        raise ValueError(f"unknown word layout preset {name!r}")
    if W % 2 or H % 2:
        raise ValueError("a downscale word layout needs an even width and height")
    if int(factor) != 2:
        raise ValueError("factor must be 2 (other factors are not covered)")
    paired = _ffi.WORD_PRESETS[name] == _ffi.WORDS_P010
    shift = {_ffi.WORDS_P010: 8, _ffi.WORDS_I010: 2, _ffi.WORDS_I012: 4, _ffi.WORDS_I016: 8}[_ffi.WORD_PRESETS[name]]
    return dict(y_offset=0, cb_offset=8 * W * H, cr_offset=8 * W * H + 2 if paired else 10 * W * H, y_pitch=4 * W,
                c_pitch=4 * W if paired else 2 * W, c_step=4 if paired else 2, frame_stride=12 * W * H, factor=2, shift=shift)


def downscale_word_layout_extent(layout, strips, mb_rows):
    """Bytes of a SOURCE frame the downscaled word kernels may read (the read contract of include/mpeg1_hip.h): the plane layout's
    extent taken on the source, rows = 2 * ye (luma) and ye (chroma), row bytes = 4 * xe (luma) and (xe - 1) * c_step + 2
    (chroma) for the strips * 16 x mb_rows * 16 region.  layout: a dict of DOWNSCALE_WORD_LAYOUT_FIELDS with no zeros but the
    shift (Mpeg1Encoder.downscale_word_layout)."""
    xe, ye = strips * 16, mb_rows * 16
    luma = (2 * ye - 1) * layout["y_pitch"] + 4 * xe
    chroma = (ye - 1) * layout["c_pitch"] + (xe - 1) * layout["c_step"] + 2
    return max(layout["y_offset"] + luma, max(layout["cb_offset"], layout["cr_offset"]) + chroma)


# The layout kinds: the property that describes one, its name in the C API (m1v_set_<c>_layout, m1v_<c>_layout_in_force), its
# ctypes struct, fields, name in messages and preset function, whether a dict must hold every field, why frames() and
# plane_frames() refuse it (None: they serve it).  In the order in which the C getters cannot fail (_refresh_input):
# sample_layout holds a plane layout too (y_step 1); input_layout is never None (all zeros = packed frames).
_Kind = namedtuple("_Kind", "prop c struct fields name preset exact no_frames no_plane_frames")
_NO_PLANES = "a plane table needs a plane layout or an RGB plane layout in force"
_KINDS = (
    _Kind("downscale_word_layout", "downscale_word", _ffi.DownscaleWordLayout, DOWNSCALE_WORD_LAYOUT_FIELDS, "a downscale word layout",
          downscale_word_layout_preset, False,
          "a frame table does not serve a downscale word layout (set_downscale_word_layout)",
          "a plane table does not serve a downscale word layout (set_downscale_word_layout)"),
    _Kind("downscale_plane_layout", "downscale_plane", _ffi.DownscalePlaneLayout, DOWNSCALE_PLANE_LAYOUT_FIELDS, "a downscale plane layout",
          downscale_plane_layout_preset, False,
          "a frame table does not serve a downscale plane layout (set_downscale_plane_layout)",
          "a plane table does not serve a downscale plane layout (set_downscale_plane_layout)"),
    _Kind("downscale_layout", "downscale", _ffi.DownscaleLayout, DOWNSCALE_LAYOUT_FIELDS, "a downscale layout", None, True,
          "a frame table does not serve a downscale layout (set_downscale_layout)",
          "a plane table does not serve a downscale layout (set_downscale_layout)"),
    _Kind("float_pixel_layout", "float_pixel", _ffi.FloatPixelLayout, FLOAT_PIXEL_LAYOUT_FIELDS, "a float pixel layout", None, True,
          "a frame table does not serve a float pixel layout (set_float_pixel_layout)",
          "a plane table does not serve a float pixel layout (set_float_pixel_layout)"),
    # (frames() checks and uploads float planes although m1v_set_frame_table refuses them)
    _Kind("float_plane_layout", "float_plane", _ffi.FloatPlaneLayout, FLOAT_PLANE_LAYOUT_FIELDS, "a float plane layout", None, True, None, _NO_PLANES),
    _Kind("rgb_plane_layout", "rgb_plane", _ffi.RgbPlaneLayout, RGB_PLANE_LAYOUT_FIELDS, "an RGB plane layout", rgb_plane_layout_preset, True, None, None),
    _Kind("sample_layout", "sample", _ffi.SampleLayout, SAMPLE_LAYOUT_FIELDS, "a sample layout", sample_layout_preset, False, None, None),
    _Kind("plane_layout", "plane", _ffi.PlaneLayout, PLANE_LAYOUT_FIELDS, "a plane layout", plane_layout_preset, False, None, None),
    _Kind("input_layout", "input", None, ("row_pitch", "frame_stride", "order"), "a surface layout", None, False, None, _NO_PLANES),
)
_KIND = {k.prop: k for k in _KINDS}


def _frames_apart(rgb, frame_stride, S=None):
    """S: the bytes of an element where strides count elements"""
    assert rgb.shape[0] <= 1 or rgb.stride(0) * (S or 1) == frame_stride, \
        f"frames must lie {frame_stride} bytes apart (stride {rgb.stride(0)}{' elements' if S else ''})"


class FrameTable:
    """A batch whose frames lie at separate device addresses (Mpeg1Encoder.frames, Mpeg1Encoder.set_frame_table): `table` is the
    int64 CUDA tensor [n] of the frames' base addresses, which the kernels read on the stream; `frames` keeps the tensors it
    names alive.  Stands where the methods of Mpeg1Encoder and HostDelivery.step take `rgb`: they read shape[0], device and
    data_ptr() of it."""

    def __init__(self, table, frames=()):
        self.table, self.frames = table, tuple(frames)
        self.shape, self.device = (int(table.shape[0]),), table.device

    def data_ptr(self):
        return self.table.data_ptr()

    def __len__(self):
        return self.shape[0]


class StreamSpans:
    """The spans of a batch of many streams (stream_spans, Mpeg1Encoder.encode_streams): `table` is the int32 CUDA tensor [n_streams, 4]
    of m1v_stream_span records (first_frame, n_frames, first_frame_index, 0), which the kernels read on the stream; `spans` the
    (n_frames, first_frame_index) pairs it was made from."""

    def __init__(self, table, spans):
        self.table, self.spans = table, tuple((int(n), int(i)) for n, i in spans)
        self.n_streams, self.n_frames = len(self.spans), sum(n for n, _ in self.spans)
        self.device = table.device

    def data_ptr(self):
        return self.table.data_ptr()

    def __len__(self):
        return self.n_streams

    def ranges(self):
        """[(first_frame, n_frames, first_frame_index)] of every span, in batch order."""
        out, at = [], 0
        for n, i in self.spans:
            out.append((at, n, i))
            at += n
        return out


def stream_spans(spans, device="cuda"):
    """The device array of spans for a batch that is the concatenation of `spans`: [(n_frames, first_frame_index), ...], one pair
    per stream in batch order (n_frames may be 0).  Returns a StreamSpans holder with .data_ptr()."""
    import torch
    pairs = [(int(n), int(i)) for n, i in spans]
    if not 1 <= len(pairs) <= _ffi.MAX_STREAMS:
        raise EncoderError(_ffi.E_ARG, f"stream_spans: 1 to {_ffi.MAX_STREAMS} streams")
    if any(n < 0 or not -2 ** 31 <= i < 2 ** 31 for n, i in pairs) or sum(n for n, _ in pairs) >= 2 ** 31:
        raise EncoderError(_ffi.E_ARG, "stream_spans: n_frames >= 0 and a first_frame_index that fits int32")
    rows, at = [], 0
    for n, i in pairs:
        rows.append((at, n, i, 0))
        at += n
    return StreamSpans(torch.tensor(rows, dtype=torch.int32).to(device), pairs)


class Mpeg1Encoder:
    """One picture geometry + quality factor on one GPU.

    Input: packed uint8 frames by default; the set_*_layout methods put surfaces, YCbCr planes, planes of R, G and B bytes, or
    planes of float R, G and B samples (set_float_plane_layout: float16, bfloat16, float32), or float R, G, B pixels
    (set_float_pixel_layout: channels-last tensors), or byte surfaces of twice the size, averaged 2 x 2 (set_downscale_layout),
    or YCbCr planes of twice the size, averaged 2 x 2 per plane (set_downscale_plane_layout), or such planes of 16-bit words
    (set_downscale_word_layout), in their place.

    mode: "strict" = the 96x144 region the unmodified reference encodes (encoder.h:238,248),
          "full"   = every macroblock (the reference with its loop bounds restored).
    """

    def __init__(self, width, height, quality_factor=12, mode="full", channels=3, max_frames=300, device=0):
        self._h = C.c_void_p(0)
        self.width, self.height, self.channels = int(width), int(height), int(channels)
        self.quality_factor, self.max_frames, self.device = int(quality_factor), int(max_frames), int(device)
        self.mode = {"strict": _ffi.MODE_STRICT, "full": _ffi.MODE_FULL}[mode] if isinstance(mode, str) else int(mode)
        rc = _ffi.lib().m1v_create(C.byref(self._h), self.device, self.width, self.height, self.channels,
                                   self.quality_factor, self.mode, self.max_frames)
        if rc != _ffi.OK:
            self._h = C.c_void_p(0)
            raise EncoderError(rc, "m1v_create")
        L = _ffi.lib()
        self.strips, self.mb_rows = L.m1v_strips(self._h), L.m1v_mb_rows(self._h)
        self.frame_bound = L.m1v_frame_bound(self._h)
        # the long-batch rule (include/mpeg1_hip.h, m1v_create): min(max_frames, the device's grid extents in y and z); a call
        # with more frames raises EncoderError (E_ARG) before anything is queued
        self.batch_limit = L.m1v_batch_limit(self._h)
        self.frame_bytes_in = L.m1v_frame_bytes_in(self._h)
        self.blocks_per_frame = self.strips * self.mb_rows * 6
        self._refresh_input()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _ffi.lib().m1v_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:        # at interpreter shutdown module globals may already be gone; the process is ending anyway
            self.close()
        except Exception:
            pass

    # ---- the hot path -------------------------------------------------------------------------
    def encode(self, rgb, first_frame_index=0, out=None, sizes=None, meta=None, quality=None):
        """rgb: uint8 CUDA tensor [n, H, W, C], contiguous — or, after set_input_layout, a view with that layout's strides, such
        as surface[:, y0:y0+H, x0:x0+W, :]; or, after set_plane_layout, [n, L] YCbCr planes; or, after set_rgb_plane_layout,
        [n, C, H, W] planes of R, G and B; or, after set_float_plane_layout, a float16, bfloat16 or float32 tensor [n, C, H, W] of
        the layout's dtype (a uint8 tensor is then refused, as a float tensor is under every other layout); or, after set_float_pixel_layout, a float tensor [n, H, W, C] or a
        channels-last [n, C, H, W] of the layout's dtype; or, after set_frame_table, what frames() returns or an int64 CUDA tensor [n] of frame
        addresses; or, after set_plane_table, what plane_frames() returns or an int64 CUDA tensor [n, 3] of plane addresses
        (this holds for every method that takes rgb).  Asynchronous on torch's current stream.
        quality: None (the encoder's quality factor) or one quality per frame, 1 <= q <= quality_factor (a sequence or a
        CUDA uint8 tensor); an entry outside that range sets STATUS_QUALITY in meta[1] and the output is undefined.
        Returns (out, sizes, meta): out uint8[cap] frame records back to back, sizes uint64-as-int64[n],
        meta int64[2] = (total bytes, status bits)."""
        import torch
        n = rgb.shape[0]
        self._check_input(rgb)
        if out is None:
            out = torch.empty(self.default_out_capacity(n), dtype=torch.uint8, device=rgb.device)
        if sizes is None:
            sizes = torch.empty(max(n, 1), dtype=torch.int64, device=rgb.device)
        if meta is None:
            meta = torch.zeros(2, dtype=torch.int64, device=rgb.device)
        results = (_ptr(out), out.numel(), _ptr(sizes), *_meta_ptrs(meta), _stream())
        if quality is None:
            _call("m1v_encode_device", self._h, _ptr(rgb), n, int(first_frame_index), *results)
        else:
            q = self._quality_tensor(quality, n, rgb.device)
            _call("m1v_encode_quality_device", self._h, _ptr(rgb), n, int(first_frame_index), _ptr(q), *results)
        return out, sizes, meta

    def _refresh_input(self):
        """What _check_input holds tensors against: (the property that describes the input layout in force, its value), asked of
        the library in the order of _KINDS."""
        self._input = next((k.prop, v) for k, v in ((k, getattr(self, k.prop)) for k in _KINDS) if v is not None)
        self._table_on = self.frame_table   # (every successful layout setter turns the tables off)
        self._planes_on = self.plane_table

    def _check_input(self, rgb):
        import torch
        if self._planes_on:  # a plane table: what plane_frames() made, or the caller's own int64 addresses [n, 3]
            assert (isinstance(rgb, FrameTable) and tuple(rgb.table.shape[1:]) == (3,)) or \
                (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.int64 and rgb.dim() == 2
                 and rgb.shape[1] == 3 and rgb.is_contiguous()), \
                "a plane table is on: pass plane_frames([...]) or a contiguous CUDA int64 tensor [n, 3] of plane addresses"
            return
        if self._table_on:  # a frame table: what frames() made, or the caller's own int64 addresses [n]
            assert isinstance(rgb, FrameTable) or (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.int64
                                                   and rgb.dim() == 1 and rgb.is_contiguous()), \
                "a frame table is on: pass frames([...]) or a contiguous CUDA int64 tensor [n] of frame addresses"
            return
        assert not isinstance(rgb, FrameTable), "a FrameTable needs set_frame_table()"
        kind, want = self._input
        if "sample" in _KIND[kind].fields:  # a float layout: tensors of its dtype, whose strides count elements of S bytes
            dtype, S = getattr(torch, _ffi.FLOAT_SAMPLE_DTYPES[want["sample"]]), _ffi.FLOAT_SAMPLE_BYTES[want["sample"]]
            assert isinstance(rgb, torch.Tensor) and rgb.dtype == dtype, \
                f"the {_KIND[kind].name[2:]} in force takes {dtype} tensors, not {getattr(rgb, 'dtype', type(rgb))}"
        if kind == "downscale_word_layout":  # the SOURCE: [n, L] words or bytes, held by their byte extent and byte row stride
            words = tuple(getattr(torch, name) for name in ("uint8", "int16", "uint16") if hasattr(torch, name))
            assert isinstance(rgb, torch.Tensor) and rgb.dtype in words, \
                f"the downscale word layout in force takes torch.uint8, torch.int16 or torch.uint16 tensors, not {getattr(rgb, 'dtype', type(rgb))}"
            assert rgb.is_cuda and rgb.dim() == 2, "downscale word sources must be a CUDA tensor [n, L] of words or bytes"
            extent, S = downscale_word_layout_extent(want, self.strips, self.mb_rows), rgb.element_size()
            assert rgb.shape[0] == 0 or (rgb.stride(1) == 1 and rgb.shape[1] * S >= extent), \
                f"a frame's row must be contiguous and hold the {extent} bytes its source planes span"
            _frames_apart(rgb, want["frame_stride"], S if S > 1 else None)
            return
        if kind == "downscale_plane_layout":  # the SOURCE: [n, L] bytes, the plane layout's rule on the source's extent
            assert isinstance(rgb, torch.Tensor) and rgb.dtype == torch.uint8, \
                f"the downscale plane layout in force takes torch.uint8 tensors, not {getattr(rgb, 'dtype', type(rgb))}"
            assert rgb.is_cuda and rgb.dim() == 2, "downscale plane sources must be a CUDA uint8 tensor [n, L]"
            extent = downscale_plane_layout_extent(want, self.strips, self.mb_rows)
            assert rgb.shape[0] == 0 or (rgb.stride(1) == 1 and rgb.shape[1] >= extent), \
                f"a frame's row must be contiguous and hold the {extent} bytes its source planes span"
            _frames_apart(rgb, want["frame_stride"])
            return
        if kind == "downscale_layout":  # the SOURCE: [n, 2H, 2W, C], or [n, C, 2H, 2W] with channels-last strides
            assert isinstance(rgb, torch.Tensor) and rgb.dtype == torch.uint8, \
                f"the downscale layout in force takes torch.uint8 tensors, not {getattr(rgb, 'dtype', type(rgb))}"
            assert rgb.is_cuda and rgb.dim() == 4, "downscale sources must be a CUDA tensor [n, 2H, 2W, C] or a channels-last [n, C, 2H, 2W]"
            size = (2 * self.height, 2 * self.width)
            if tuple(rgb.shape[1:3]) == size and rgb.shape[3] in (3, 4):
                frame, row, pixel, channel = rgb.stride()
                C_ = rgb.shape[3]
            else:
                assert tuple(rgb.shape[2:]) == size and rgb.shape[1] in (3, 4), \
                    f"sources must be [n, 2H, 2W, C] or a channels-last [n, C, 2H, 2W] with C = 3 or 4 and 2H x 2W = {size[0]} x {size[1]}"
                frame, channel, row, pixel = rgb.stride()
                C_ = rgb.shape[1]
            assert channel == 1, f"strides {tuple(rgb.stride())}: the bytes of a pixel must be adjacent"
            assert pixel == want["pixel_step"] and pixel >= C_ and row == want["row_pitch"], \
                f"strides {tuple(rgb.stride())} are not the downscale layout in force (pixel step {want['pixel_step']}, row pitch {want['row_pitch']} bytes)"
            _frames_apart(rgb, want["frame_stride"])
            # every whole pixel of the read contract lies in the storage (a window's last pixel may lack its 4th byte)
            last = rgb.storage_offset() + max(rgb.shape[0] - 1, 0) * frame + (size[0] - 1) * row + size[1] * pixel
            assert rgb.shape[0] == 0 or last <= rgb.untyped_storage().nbytes(), \
                "the tensor's storage ends inside the last pixel the encoder reads (a 4th byte beyond the view)"
            return
        if kind == "float_pixel_layout":  # [n, H, W, C], or [n, C, H, W] with channels-last strides
            assert rgb.is_cuda and rgb.dim() == 4, "float pixel frames must be a CUDA tensor [n, H, W, C] or a channels-last [n, C, H, W]"
            size = (self.height, self.width)
            if tuple(rgb.shape[1:3]) == size and rgb.shape[3] in (3, 4):
                frame, row, pixel, channel = rgb.stride()
                C_ = rgb.shape[3]
            else:
                assert tuple(rgb.shape[2:]) == size and rgb.shape[1] in (3, 4), \
                    "frames must be [n, H, W, C] or a channels-last [n, C, H, W] with C = 3 or 4"
                frame, channel, row, pixel = rgb.stride()
                C_ = rgb.shape[1]
            assert channel == 1, \
                f"strides {tuple(rgb.stride())}: the samples of a pixel must be adjacent (planar NCHW frames: set_float_plane_layout)"
            assert pixel * S == want["pixel_step"] and pixel >= C_ and row * S == want["row_pitch"], \
                f"strides {tuple(rgb.stride())} are not the float pixel layout in force (pixel step {want['pixel_step']}, row pitch {want['row_pitch']} bytes)"
            _frames_apart(rgb, want["frame_stride"], S)
            # every whole pixel of the read contract lies in the storage (a window's last pixel may lack its 4th sample)
            last = rgb.storage_offset() + max(rgb.shape[0] - 1, 0) * frame + (self.height - 1) * row + self.width * pixel
            assert rgb.shape[0] == 0 or last * S <= rgb.untyped_storage().nbytes(), \
                "the tensor's storage ends inside the last pixel the encoder reads (a 4th sample beyond the view)"
            return
        if kind == "float_plane_layout":  # [n, C, H, W]: strides times S = the layout's bytes
            assert rgb.is_cuda and rgb.dim() == 4, "float plane frames must be a CUDA tensor [n, C, H, W]"
            assert rgb.shape[1] >= 3 and tuple(rgb.shape[2:]) == (self.height, self.width), "frames must be [n, C >= 3, H, W]"
            assert rgb.stride(3) == 1 and rgb.stride(2) * S == want["row_pitch"], \
                f"strides {tuple(rgb.stride())} are not the float plane layout in force (row pitch {want['row_pitch']} bytes)"
            _frames_apart(rgb, want["frame_stride"], S)
            plane = rgb.stride(1) * S
            assert all(plane > 0 and want[k] % plane == 0 and want[k] // plane < rgb.shape[1] for k in ("r_offset", "g_offset", "b_offset")), \
                f"the plane offsets in force are not channels of this tensor (plane stride {plane} bytes)"
            return
        assert not (isinstance(rgb, torch.Tensor) and rgb.dtype.is_floating_point), \
            f"the layout in force takes torch.uint8 tensors, not {rgb.dtype} (float planes: set_float_plane_layout; float pixels: set_float_pixel_layout)"
        if kind == "rgb_plane_layout":  # [n, C, H, W]: channel k of the tensor = the plane at offset k * stride(1)
            assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 4, "RGB plane frames must be a CUDA uint8 tensor [n, C, H, W]"
            assert rgb.shape[1] >= 3 and tuple(rgb.shape[2:]) == (self.height, self.width), "frames must be [n, C >= 3, H, W]"
            assert rgb.stride(3) == 1 and rgb.stride(2) == want["row_pitch"], \
                f"strides {tuple(rgb.stride())} are not the RGB plane layout in force (row pitch {want['row_pitch']})"
            _frames_apart(rgb, want["frame_stride"])
            plane = rgb.stride(1)
            assert all(plane > 0 and want[k] % plane == 0 and want[k] // plane < rgb.shape[1] for k in ("r_offset", "g_offset", "b_offset")), \
                f"the plane offsets in force are not channels of this tensor (plane stride {plane})"
            return
        if kind == "sample_layout":     # [n, L] bytes, frame f at row f: L covers the frame's extent, rows frame_stride apart
            assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 2, "plane frames must be a CUDA uint8 tensor [n, L]"
            extent = plane_layout_extent(want, self.strips, self.mb_rows)
            assert rgb.shape[0] == 0 or (rgb.stride(1) == 1 and rgb.shape[1] >= extent), \
                f"a frame's row must be contiguous and hold the {extent} bytes its planes span"
            _frames_apart(rgb, want["frame_stride"])
            return
        row_pitch, frame_stride, _ = want
        if row_pitch == 0:      # the default layout: packed frames
            assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.is_contiguous()
            assert rgb.numel() == rgb.shape[0] * self.frame_bytes_in
            return
        assert rgb.is_cuda and rgb.dtype == torch.uint8
        assert tuple(rgb.shape[1:]) == (self.height, self.width, self.channels), "frames must be [n, H, W, C]"
        pitch, stride = surface_strides(tuple(rgb.shape), tuple(rgb.stride()))
        assert pitch == row_pitch and (rgb.shape[0] <= 1 or stride == frame_stride), \
            f"strides {tuple(rgb.stride())} are not the input layout in force (row pitch {row_pitch}, frame stride {frame_stride})"

    def set_input_layout(self, row_pitch=0, frame_stride=0, order="rgb"):
        """Frames as windows of pitched device surfaces, in "rgb" or "bgr" byte order (a 4th byte is skipped), encoded where they
        lie (include/mpeg1_hip.h, m1v_set_input_layout).  row_pitch / frame_stride in bytes, 0 = W * C / H * row_pitch (see
        surface_strides).  Every call then takes tensors with those strides.  The defaults restore the packed layout and its
        kernels.  A reconfiguration: call it between batches."""
        code = {"rgb": _ffi.ORDER_RGB, "bgr": _ffi.ORDER_BGR}.get(order, order)
        _call("m1v_set_input_layout", self._h, int(row_pitch), int(frame_stride), int(code))
        self._refresh_input()   # one input layout is in force at a time

    def _set_layout(self, prop, layout):
        """The C setter of the kind of `prop` (_KINDS) with `layout`: a preset name, a dict of its fields, or None."""
        k, c = _KIND[prop], None
        if layout is not None:
            if isinstance(layout, str) and k.preset:
                layout = k.preset(self.width, self.height, layout)
            if k.exact and set(layout) != set(k.fields):
                raise ValueError(f"{k.name} has the fields {k.fields}")
            if set(layout) - set(k.fields):
                raise ValueError(f"unknown {k.c} layout fields {sorted(set(layout) - set(k.fields))}")
            c = C.byref(k.struct(**{f: int(v) for f, v in layout.items()}))
        _call(f"m1v_set_{k.c}_layout", self._h, c)
        self._refresh_input()

    def set_plane_layout(self, layout):
        """Frames as Y, Cb, Cr planes on the device, encoded without a colour conversion (include/mpeg1_hip.h,
        m1v_set_plane_layout; 3-channel encoders).  layout: a preset name ("reference", "i420", "yv12", "nv12", "nv21"), a dict
        of PLANE_LAYOUT_FIELDS in bytes (plane_layout_preset gives one to start from; missing pitches and c_step default as in the
        header), or None = back to the default layout and its kernels.  Every call then takes uint8 CUDA tensors [n, L] whose
        rows are the frames: L >= the bytes a frame's planes span, rows frame_stride apart — convert(rgb).view(n, -1) and
        torch.as_strided views go in as they are.  A reconfiguration: call it between batches."""
        self._set_layout("plane_layout", layout)

    def set_sample_layout(self, layout):
        """Frames whose samples lie one or two bytes apart, encoded where they lie (include/mpeg1_hip.h, m1v_set_sample_layout;
        3-channel encoders): packed 4:2:2 and P010 / P012 / P016 beside everything set_plane_layout takes.  layout: a preset name
        ("yuy2", "uyvy", "yvyu", "p010"), a dict of SAMPLE_LAYOUT_FIELDS in bytes (sample_layout_preset gives one to start from;
        missing pitches and steps default as in the header), or None = back to the default layout and its kernels.  Every call
        then takes uint8 CUDA tensors [n, L] as after set_plane_layout.  A uint16 P010 tensor goes in as
        frames.view(torch.uint8) (reshaped to [n, L]): the coded sample is each word's high byte, truncation, not rounding.
        A reconfiguration: call it between batches."""
        self._set_layout("sample_layout", layout)

    def set_rgb_plane_layout(self, layout):
        """Frames as planes of R, G and B bytes on the device — NCHW uint8 tensors — encoded where they lie, without a permute and
        copy to interleaved pixels (include/mpeg1_hip.h, m1v_set_rgb_plane_layout; 3-channel encoders, even widths).  layout: a
        plane order ("rgb", "bgr", "gbr": tightly packed, rgb_plane_layout_preset), a dict of RGB_PLANE_LAYOUT_FIELDS in bytes
        (rgb_plane_strides derives one from a tensor's shape and strides), or None = back to the default layout and its kernels.
        Every call then takes uint8 CUDA tensors [n, C >= 3, H, W] with those strides: a view x[:, :, y0:y0+H, x0:x0+W] of a larger
        tensor goes in as it is.  A reconfiguration: call it between batches."""
        self._set_layout("rgb_plane_layout", layout)

    def set_float_plane_layout(self, layout):
        """Frames as planes of float R, G and B samples on the device — NCHW float16, bfloat16 or float32 tensors, a model's output
        — encoded where they lie, without x.mul(255).round().clamp(0, 255).to(torch.uint8) in front (include/mpeg1_hip.h,
        m1v_set_float_plane_layout, which defines the byte of a sample: one fp32 multiplication by 255 or 1, ties to even, NaN and
        negatives 0, above 255 255; 3-channel encoders, even widths).  layout: a dict of FLOAT_PLANE_LAYOUT_FIELDS
        (float_plane_layout_preset, or float_plane_strides from a tensor's shape and strides), or None = back to the default
        layout and its kernels.  Every call then takes CUDA tensors [n, C >= 3, H, W] of exactly that dtype with those strides: a
        view x[:, :, y0:y0+H, x0:x0+W] and three planes of a 4-plane tensor go in as they are; a uint8 tensor is refused.  Frame
        and plane tables do not serve it.  A reconfiguration: call it between batches."""
        self._set_layout("float_plane_layout", layout)

    def float_planes_to_bytes(self, x, out=None):
        """The bytes the encoder codes for the float tensor x under the float plane layout in force (include/mpeg1_hip.h,
        m1v_float_planes_to_bytes_device: the kernels' own conversion function): a uint8 CUDA tensor [n, 3, H, W] in R, G, B
        order, what set_rgb_plane_layout("rgb") takes.  Asynchronous on torch's current stream."""
        return self._to_bytes("float_plane_layout", x, out, lambda n: (n, 3, self.height, self.width))

    def _to_bytes(self, prop, x, out, shape, call=None):
        """m1v_<c>s_to_bytes_device (or m1v_<call>_device) under the layout that `prop` describes: the bytes of x as a uint8 tensor
        of shape(n)."""
        import torch
        k = _KIND[prop]
        call = call or f"{k.c}s_to_bytes"
        assert self._input[0] == prop, f"{call}() needs {k.name} in force (set_{k.c}_layout)"
        self._check_input(x)
        shape = shape(x.shape[0])
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == shape
        _call(f"m1v_{call}_device", self._h, _ptr(x), shape[0], _ptr(out), _stream())
        return out

    def set_float_pixel_layout(self, layout):
        """Frames as float R, G and B samples interleaved per pixel on the device — [n, H, W, 3] or [n, H, W, 4] tensors of float16,
        bfloat16 or float32, torch.channels_last model outputs, RGBA16F / RGBA32F targets — encoded where they lie, without a
        conversion to uint8 or a permute and copy to planes in front (include/mpeg1_hip.h, m1v_set_float_pixel_layout; the byte of
        a sample is the float plane layout's; 3-channel encoders, even widths).  layout: a dict of FLOAT_PIXEL_LAYOUT_FIELDS
        (float_pixel_layout_preset, or float_pixel_strides from a tensor's shape and strides), or None = back to the default
        layout and its kernels.  Every call then takes CUDA tensors of exactly that dtype with those strides, as [n, H, W, C] or as
        a channels-last-strided [n, C, H, W]; a window x[:, y0:y0+H, x0:x0+W, :3] goes in as it is; uint8 and NCHW-contiguous
        tensors are refused.  Frame and plane tables do not serve it.  A reconfiguration: call it between batches."""
        self._set_layout("float_pixel_layout", layout)

    def float_pixels_to_bytes(self, x, out=None):
        """The bytes the encoder codes for the float tensor x under the float pixel layout in force (include/mpeg1_hip.h,
        m1v_float_pixels_to_bytes_device: the kernels' own conversion function): a uint8 CUDA tensor [n, H, W, 3] in R, G, B
        order, what the default packed layout takes.  Asynchronous on torch's current stream."""
        return self._to_bytes("float_pixel_layout", x, out, lambda n: (n, self.height, self.width, 3))

    def set_downscale_layout(self, layout):
        """Frames as byte surfaces of TWICE the encoder's width and height on the device — [n, 2H, 2W, 3] or [n, 2H, 2W, 4] uint8
        tensors, windows of larger surfaces — whose 2 x 2 box average, (sum of the four source bytes + 2) >> 2 per colour, is the
        picture that is encoded: the half-size rendition without a resampling kernel and a full-size intermediate in front
        (include/mpeg1_hip.h, m1v_set_downscale_layout; 3-channel encoders, even widths).  layout: a dict of
        DOWNSCALE_LAYOUT_FIELDS (downscale_layout_preset, or downscale_strides from the source tensor's shape and strides), or
        None = back to the default layout and its kernels.  Every call then takes uint8 CUDA tensors with those strides, as
        [n, 2H, 2W, C] or as a channels-last-strided [n, C, 2H, 2W]; a window x[:, y0:y0+2H, x0:x0+2W, :3] goes in as it is.
        Frame and plane tables do not serve it.  A reconfiguration: call it between batches."""
        self._set_layout("downscale_layout", layout)

    def downscale_to_bytes(self, x, out=None):
        """The bytes the encoder codes for the source tensor x under the downscale layout in force (include/mpeg1_hip.h,
        m1v_downscale_to_bytes_device): a uint8 CUDA tensor [n, H, W, 3] in R, G, B order, what the default packed layout takes.
        Asynchronous on torch's current stream."""
        return self._to_bytes("downscale_layout", x, out, lambda n: (n, self.height, self.width, 3), call="downscale_to_bytes")

    def set_downscale_plane_layout(self, layout):
        """Frames as Y, Cb, Cr planes of TWICE the encoder's width and height on the device — true 4:2:0 sources: a decoder's NV12
        surfaces, a camera's I420 frames, pitched windows of them — whose 2 x 2 box average per plane, (sum of the four source
        samples + 2) >> 2, is the picture that is encoded: the half-size rendition without a resampling kernel in front and
        without a detour through RGB (include/mpeg1_hip.h, m1v_set_downscale_plane_layout; 3-channel encoders, even widths and
        heights).  layout: a preset name ("i420", "yv12", "nv12", "nv21": the tightly packed source), a dict of
        DOWNSCALE_PLANE_LAYOUT_FIELDS in bytes of the source (downscale_plane_layout_preset gives one to start from; missing
        pitches and c_step default as in the header, factor is 2), or None = back to the default layout and its kernels.  Every
        call then takes uint8 CUDA tensors [n, L] whose rows are the source frames: L >= the bytes a source frame's planes span,
        rows frame_stride apart.  Frame and plane tables do not serve it.  A reconfiguration: call it between batches."""
        if isinstance(layout, dict):
            layout = {"factor": 2, **layout}
        self._set_layout("downscale_plane_layout", layout)

    def downscale_planes_to_i420(self, x, out=None):
        """The samples the encoder codes for the source tensor x under the downscale plane layout in force (include/mpeg1_hip.h,
        m1v_downscale_planes_to_i420_device): a uint8 CUDA tensor [n, W * H * 3 / 2] of tightly packed I420 frames, what
        set_plane_layout("i420") takes.  Reads the whole 2W x 2H source, so a row of x holds every plane in full.  Asynchronous on
        torch's current stream."""
        want = self._input[1] if self._input[0] == "downscale_plane_layout" else None
        if want is not None and x.shape[0]:  # the whole source, not only the coded region
            W, H = self.width, self.height
            full = max(want["y_offset"] + (2 * H - 1) * want["y_pitch"] + 2 * W,
                       max(want["cb_offset"], want["cr_offset"]) + (H - 1) * want["c_pitch"] + (W - 1) * want["c_step"] + 1)
            assert x.dim() == 2 and x.shape[1] >= full, f"a frame's row must hold the {full} bytes of the whole source"
        return self._to_bytes("downscale_plane_layout", x, out, lambda n: (n, self.width * self.height * 3 // 2), call="downscale_planes_to_i420")

    def set_downscale_word_layout(self, layout):
        """Frames as Y, Cb, Cr planes of 16-bit little-endian words of TWICE the encoder's width and height on the device — true
        4:2:0 sources: a hardware decoder's P010 / P012 / P016 surfaces, a software decoder's yuv420p10le / 12le / 16le frames,
        pitched windows of them — whose 2 x 2 box average per plane, taken on the words, (sum of the four source words + 2) >> 2,
        then >> shift and clamped to 255, is the picture that is encoded (include/mpeg1_hip.h, m1v_set_downscale_word_layout;
        3-channel encoders, even widths and heights).  layout: a preset name ("p010", "p012", "p016", "i010", "i012", "i016": the
        tightly packed source), a dict of DOWNSCALE_WORD_LAYOUT_FIELDS in bytes of the source (downscale_word_layout_preset gives
        one to start from; missing pitches and c_step default as in the header, factor is 2, a missing shift is 0), or None = back
        to the default layout and its kernels.  Every call then takes CUDA tensors [n, L] of uint8, int16 or uint16 whose rows are
        the source frames: a row holds at least the bytes a source frame's planes span, rows frame_stride bytes apart.  Frame and
        plane tables do not serve it.  A reconfiguration: call it between batches."""
        if isinstance(layout, dict):
            layout = {"factor": 2, **layout}
        self._set_layout("downscale_word_layout", layout)

    def downscale_words_to_i420(self, x, out=None):
        """The samples the encoder codes for the source tensor x under the downscale word layout in force (include/mpeg1_hip.h,
        m1v_downscale_words_to_i420_device): a uint8 CUDA tensor [n, W * H * 3 / 2] of tightly packed I420 frames, what
        set_plane_layout("i420") takes.  Reads the whole 2W x 2H source, so a row of x holds every plane in full.  Asynchronous on
        torch's current stream."""
        want = self._input[1] if self._input[0] == "downscale_word_layout" else None
        if want is not None and x.shape[0]:  # the whole source, not only the coded region
            W, H = self.width, self.height
            full = max(want["y_offset"] + (2 * H - 1) * want["y_pitch"] + 4 * W,
                       max(want["cb_offset"], want["cr_offset"]) + (H - 1) * want["c_pitch"] + (W - 1) * want["c_step"] + 2)
            assert x.dim() == 2 and x.shape[1] * x.element_size() >= full, f"a frame's row must hold the {full} bytes of the whole source"
        return self._to_bytes("downscale_word_layout", x, out, lambda n: (n, self.width * self.height * 3 // 2), call="downscale_words_to_i420")

    def set_frame_table(self, enable=True):
        """Batches whose frames lie at separate device addresses (include/mpeg1_hip.h, m1v_set_frame_table): while on, every
        method takes, in the place of `rgb`, what frames() returns or a contiguous CUDA int64 tensor [n] of the frames' base
        addresses, which only the kernels read, on the stream.  Needs a surface, plane, sample or RGB plane layout in force (packed
        frames: set_input_layout(width * channels) first); every layout setter turns it off again.  Not a reconfiguration:
        nothing is allocated or waited for."""
        _call("m1v_set_frame_table", self._h, 1 if enable else 0)
        self._table_on, self._planes_on = self.frame_table, self.plane_table   # (each mode replaces the other)

    def set_plane_table(self, enable=True):
        """Batches whose frames' planes lie at separate device addresses (include/mpeg1_hip.h, m1v_set_plane_table): while on,
        every method takes, in the place of `rgb`, what plane_frames() returns or a contiguous CUDA int64 tensor [n, 3] of plane
        addresses (Y, Cb, Cr or R, G, B), which only the kernels read, on the stream.  Needs a plane layout (set_plane_layout) or
        an RGB plane layout in force, which applies to each plane relative to its own pointer; replaces a frame table; every
        layout setter turns it off again.  Not a reconfiguration: nothing is allocated or waited for."""
        _call("m1v_set_plane_table", self._h, 1 if enable else 0)
        self._table_on, self._planes_on = self.frame_table, self.plane_table

    @property
    def plane_table(self):
        """True while a plane table is on (set_plane_table)."""
        return _ffi.lib().m1v_plane_table(self._h) == 1

    def plane_frames(self, planes):
        """A FrameTable of `planes`: per frame one tuple of three CUDA uint8 tensors, (Y, Cb, Cr) under a plane layout — Y
        [rows, >= coded width] or flat, chroma likewise; both chroma members may be the same NV12 UV tensor — or (R, G, B) [H, W]
        under an RGB plane layout.  A Y, Cb or Cr tensor starts at its plane's pointer, so the layout's offset of that plane lies
        inside it (0 for planes that are allocations of their own); an R, G or B tensor is the plane itself, and the table holds
        its address less the layout's offset, as the read contract of RGB planes allows.  Checks that each plane has unit stride along a row, the row pitch of the layout in force and
        room for the bytes the layout addresses from its pointer, and that all lie on one device; uploads the int64 [n, 3] table of
        their addresses (a host-to-device copy on the current stream) and keeps the tensors alive with the result.  For the calls
        made while set_plane_table() is on."""
        import torch
        planes = [tuple(f) for f in planes]
        assert planes and all(len(f) == 3 for f in planes), "plane_frames() needs at least one frame of three planes"
        kind, want = self._input
        refusal = _KIND[kind].no_plane_frames
        assert refusal is None and want.get("y_step", 1) == 1, refusal or _NO_PLANES
        xe, ye = self.strips * 16, self.mb_rows * 16
        back = [0, 0, 0]    # how far in front of the tensor's first byte the plane's pointer stands
        if kind == "rgb_plane_layout":  # a plane's range starts at its offset: the tensor is the plane, its pointer lies c_offset in front
            back = [want[k] for k in ("r_offset", "g_offset", "b_offset")]
            need = [(want["row_pitch"], (self.height - 1) * want["row_pitch"] + self.width)] * 3
        else:
            chroma = (ye // 2 - 1) * want["c_pitch"] + (xe // 2 - 1) * want["c_step"] + 1
            need = [(want["y_pitch"], want["y_offset"] + (ye - 1) * want["y_pitch"] + xe),
                    (want["c_pitch"], want["cb_offset"] + chroma), (want["c_pitch"], want["cr_offset"] + chroma)]
        flat = [t for f in planes for t in f]
        for f in planes:
            for t, (pitch, extent) in zip(f, need):
                assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() in (1, 2), \
                    "a plane must be a CUDA uint8 tensor [rows, row bytes] or [bytes]"
                assert t.stride(-1) == 1 and (t.dim() == 1 or t.shape[0] <= 1 or t.stride(0) == pitch), \
                    f"strides {tuple(t.stride())} are not the row pitch in force ({pitch})"
                span = t.shape[0] if t.dim() == 1 else (t.shape[0] - 1) * pitch + t.shape[1]
                assert span >= extent, f"a plane of {span} bytes cannot hold the {extent} bytes the layout addresses from its pointer"
        assert all(t.device == flat[0].device for t in flat), "the planes of a table lie on one device"
        table = torch.tensor([[t.data_ptr() - b for t, b in zip(f, back)] for f in planes], dtype=torch.int64).to(flat[0].device)
        return FrameTable(table, flat)

    @property
    def frame_table(self):
        """True while a frame table is on (set_frame_table)."""
        return _ffi.lib().m1v_frame_table(self._h) == 1

    def frames(self, tensors):
        """A FrameTable of `tensors`: one CUDA uint8 tensor per frame, each what the layout in force takes as a batch of one
        without its leading dimension ([H, W, C] with the row pitch in force; [L] bytes of planes or samples; [C, H, W] planes of
        R, G and B) — separate allocations, views of a pool, the same tensor more than once, in any order.  Checks each as a batch
        of one, uploads their addresses (a host-to-device copy on the current stream) and keeps the tensors alive with the
        result.  For the calls made while set_frame_table() is on."""
        import torch
        tensors = list(tensors)
        assert tensors, "frames() needs at least one frame"
        refusal = _KIND[self._input[0]].no_frames
        assert refusal is None, refusal
        assert self._input != ("input_layout", (0, 0, "rgb")), "a frame table needs a layout: set_input_layout(width * channels) for packed frames"
        on, self._table_on = self._table_on, False
        try:
            for t in tensors:
                self._check_input(t.unsqueeze(0))
        finally:
            self._table_on = on
        assert all(t.device == tensors[0].device for t in tensors), "the frames of a table lie on one device"
        table = torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(tensors[0].device)
        return FrameTable(table, tensors)

    def _in_force(self, prop):
        """The C getter of the kind of `prop` (_KINDS): the layout in force as a dict, or None where another kind is."""
        c, name = _KIND[prop].struct(), f"m1v_{_KIND[prop].c}_layout_in_force"
        rc = getattr(_ffi.lib(), name)(self._h, C.byref(c))
        if rc < 0:
            raise EncoderError(rc, name)
        return c.as_dict() if rc == 1 else None

    @property
    def downscale_word_layout(self):
        """The downscale word layout in force as a dict of DOWNSCALE_WORD_LAYOUT_FIELDS (bytes of the source, no zeros but the
        shift; factor; shift), or None."""
        return self._in_force("downscale_word_layout")

    @property
    def downscale_plane_layout(self):
        """The downscale plane layout in force as a dict of DOWNSCALE_PLANE_LAYOUT_FIELDS (bytes of the source, no zeros; factor;
        reserved), or None."""
        return self._in_force("downscale_plane_layout")

    @property
    def downscale_layout(self):
        """The downscale layout in force as a dict of DOWNSCALE_LAYOUT_FIELDS (bytes of the source; order code; factor), or None."""
        return self._in_force("downscale_layout")

    @property
    def float_pixel_layout(self):
        """The float pixel layout in force as a dict of FLOAT_PIXEL_LAYOUT_FIELDS (bytes; order, sample and range codes), or None."""
        return self._in_force("float_pixel_layout")

    @property
    def float_plane_layout(self):
        """The float plane layout in force as a dict of FLOAT_PLANE_LAYOUT_FIELDS (bytes; sample and range codes), or None."""
        return self._in_force("float_plane_layout")

    @property
    def rgb_plane_layout(self):
        """The RGB plane layout in force as a dict of RGB_PLANE_LAYOUT_FIELDS in bytes, or None."""
        return self._in_force("rgb_plane_layout")

    @property
    def sample_layout(self):
        """The plane or sample layout in force as a dict of SAMPLE_LAYOUT_FIELDS in bytes, as the kernels use it (no zeros;
        y_step = 1 for a layout set through set_plane_layout), or None."""
        return self._in_force("sample_layout")

    @property
    def plane_layout(self):
        """The plane layout in force as a dict of PLANE_LAYOUT_FIELDS in bytes, as the kernels use it (no zeros), or None."""
        return self._in_force("plane_layout")

    @property
    def input_layout(self):
        """(row_pitch, frame_stride, order) in force: (0, 0, "rgb") = packed frames, else the bytes the kernels step by."""
        pitch, stride, order = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        _call("m1v_input_layout", self._h, C.byref(pitch), C.byref(stride), C.byref(order))
        return pitch.value, stride.value, "bgr" if order.value == _ffi.ORDER_BGR else "rgb"

    @staticmethod
    def _quality_tensor(quality, n, device):
        """One uint8 quality per frame, on the device (the library validates the values)."""
        import torch
        if isinstance(quality, torch.Tensor):
            assert quality.is_cuda and quality.dtype == torch.uint8 and quality.numel() == n, "quality: CUDA uint8, one per frame"
            return quality.contiguous()
        q = [int(x) for x in quality]
        assert len(q) == n, "quality: one entry per frame"
        if any(x < 0 or x > 255 for x in q):
            raise EncoderError(_ffi.E_ARG, "quality: entries must fit uint8")
        return torch.tensor(q if q else [0], dtype=torch.uint8).to(device, non_blocking=False)

    def frame_sizes(self, rgb, quality=None, status=None):
        """The exact record size of every frame at `quality` (as in encode(); None = the encoder's quality factor), without
        assembling or writing any output: int64 CUDA tensor [n].  Asynchronous on torch's current stream (in pipelined mode
        complete behind flush()).  status: optional CUDA int32 tensor [1] that receives the status bits."""
        import torch
        n = rgb.shape[0]
        self._check_input(rgb)
        sizes = torch.zeros(max(n, 1), dtype=torch.int64, device=rgb.device)
        q = self._quality_tensor(quality, n, rgb.device) if quality is not None else None
        _call("m1v_frame_sizes_device", self._h, _ptr(rgb), n, _ptr(q), _ptr(sizes), _ptr(status), _stream())
        return sizes[:n]

    def frame_size_table(self, rgb, qualities, status=None):
        """The exact record size of every frame at each of `qualities` (1..8, strictly increasing, each <= quality_factor):
        int64 CUDA tensor [K, n], row k = frame_sizes(rgb, quality=[qualities[k]] * n).  One fused pass where size_table_fused
        is 1 (3 channels on the tile path, 4 channels always).  Asynchronous on torch's current stream (complete in stream order,
        pipelined mode included).  status: optional CUDA int32 tensor [K] that receives each quality's status bits
        (STATUS_UNENCODABLE: that row is undefined)."""
        return self._table("frame_size_table", rgb, qualities, status, False)[0]

    def _table(self, name, rgb, qualities, status, with_dist):
        """The table call behind the method `name`: its [K, n] rows, (sizes,) or with_dist (sizes, distortion)."""
        import torch
        n = rgb.shape[0]
        self._check_input(rgb)
        qs = [int(q) for q in qualities]
        if not 1 <= len(qs) <= _ffi.MAX_CANDIDATES or any(q < 1 or q > 255 for q in qs):
            raise EncoderError(_ffi.E_ARG, f"{name}: 1 to 8 qualities")
        if status is not None:
            assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= len(qs), "status: CUDA int32, one per quality"
        q_buf = (C.c_uint8 * len(qs))(*qs)
        rows = [torch.zeros(max(len(qs) * n, 1), dtype=torch.int64, device=rgb.device) for _ in range(2 if with_dist else 1)]
        _call("m1v_frame_rd_table_device" if with_dist else "m1v_frame_size_table_device", self._h, _ptr(rgb), n, q_buf, len(qs),
              *(_ptr(r) for r in rows), _ptr(status), _stream())
        return tuple(r[:len(qs) * n].view(len(qs), n) for r in rows)

    def frame_rd_table(self, rgb, qualities, status=None):
        """frame_size_table plus the distortion (include/mpeg1_hip.h, m1v_frame_rd_table_device): (sizes, distortion), two int64
        CUDA tensors [K, n].  sizes is exactly frame_size_table(rgb, qualities); distortion[k, f] is the exact squared error, in the
        reference's coefficient domain, between what the encoder transformed of frame f and what its record at qualities[k]
        carries.  One fused pass; needs size_table_fused.  Asynchronous on torch's current stream.  status: as frame_size_table
        (STATUS_UNENCODABLE at k: both rows k are undefined)."""
        return self._table("frame_rd_table", rgb, qualities, status, True)

    @staticmethod
    def _candidates(candidates, where):
        """1..8 candidate qualities as the HOST array the library reads (it checks order and range)."""
        cands = [int(c) for c in candidates]
        if not 1 <= len(cands) <= _ffi.MAX_CANDIDATES or any(c < 1 or c > 255 for c in cands):
            raise EncoderError(_ffi.E_ARG, f"{where}: 1 to 8 candidate qualities")
        return (C.c_uint8 * len(cands))(*cands)

    def _encode_retrying(self, rgb, name, launch):
        """Synchronous: launch(out, sizes, meta) queues one encode of rgb into those buffers for the method `name`.  On
        STATUS_SCRATCH the worst-case scratch is reserved and on STATUS_NOSPACE `out` grows to the worst case, and the encode is
        queued again, three times at most.  Returns (bytes, sizes, status bits)."""
        import torch
        n = rgb.shape[0]
        out = None
        for attempt in range(3):
            if out is None:
                out = torch.empty(self.default_out_capacity(n), dtype=torch.uint8, device=rgb.device)
            sizes = torch.empty(max(n, 1), dtype=torch.int64, device=rgb.device)
            meta = torch.zeros(2, dtype=torch.int64, device=rgb.device)
            launch(out, sizes, meta)
            self.flush()
            torch.cuda.synchronize(rgb.device)
            total, status = (int(x) for x in meta.cpu())
            status &= 0xFFFFFFFF
            if status & _ffi.STATUS_UNENCODABLE:
                raise EncoderError(_ffi.E_UNENCODABLE, "encode: |level| >= 256 (the reference crashes on this input)")
            if status & _ffi.STATUS_QUALITY:
                raise EncoderError(_ffi.E_ARG, f"{name}: a quality outside 1 .. quality_factor")
            if status & _ffi.STATUS_STREAMS:
                raise EncoderError(_ffi.E_ARG, f"{name}: spans that do not tile the batch, or a stream's rate outside 1 <= r <= C < 2^62")
            if not status & (_ffi.STATUS_NOSPACE | _ffi.STATUS_SCRATCH):
                break
            if status & _ffi.STATUS_SCRATCH:        # more runs overflowed their compact slot than the arena holds
                self.reserve_scratch(True)
            if status & _ffi.STATUS_NOSPACE:
                out = torch.empty(self.frame_bound * max(n, 1), dtype=torch.uint8, device=rgb.device)
        else:
            raise EncoderError(_ffi.E_NOSPACE if status & _ffi.STATUS_NOSPACE else _ffi.E_SCRATCH, name)
        return out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()], status

    def _encode_candidates(self, name, fn, rgb, candidates, first_frame_index, middle, with_dist=False):
        """The encodes that take candidates, for the method `name`: the C function `fn`, whose arguments between the candidates
        and d_chosen (its rule's) are `middle`, through _encode_retrying.  Returns (bytes, sizes, chosen, distortion per frame
        or None, status bits)."""
        import torch
        n = rgb.shape[0]
        self._check_input(rgb)
        cand_buf = self._candidates(candidates, name)
        chosen = torch.zeros(max(n, 1), dtype=torch.uint8, device=rgb.device)
        dist = torch.zeros(max(n, 1), dtype=torch.int64, device=rgb.device) if with_dist else None
        data, sizes_l, status = self._encode_retrying(
            rgb, name,
            lambda out, sizes, meta: _call(
                fn, self._h, _ptr(rgb), n, int(first_frame_index), cand_buf, len(cand_buf), *middle, _ptr(chosen), _ptr(out),
                out.numel(), _ptr(sizes), *((_ptr(dist),) if with_dist else ()), *_meta_ptrs(meta), _stream()))
        return (data, sizes_l, [int(c) for c in chosen[:n].cpu()], [int(d) for d in dist[:n].cpu()] if with_dist else None, status)

    @staticmethod
    def _uint64(value, what):
        if not 0 <= int(value) < 2 ** 64:
            raise EncoderError(_ffi.E_ARG, f"{what} must fit uint64")
        return int(value)

    @staticmethod
    def _per_frame_limit(name, limit, n, device):
        """One limit for every frame, or one per frame (a sequence or a CUDA int64 tensor): (scalar, tensor or None)."""
        import torch
        if isinstance(limit, torch.Tensor):
            assert limit.is_cuda and limit.dtype == torch.int64 and limit.numel() == n, "limit: CUDA int64, one per frame"
            return 0, limit.contiguous()
        if isinstance(limit, numbers.Integral):
            return Mpeg1Encoder._uint64(limit, f"{name}: the limit"), None
        b = [int(x) for x in limit]
        assert len(b) == n, "limit: one entry per frame"
        return 0, torch.tensor(b if b else [0], dtype=torch.int64).to(device)

    def _encode_per_frame(self, name, fn, rule_args, rgb, limit, candidates, first_frame_index, with_dist):
        """The encodes with a limit per frame: _encode_candidates' results and each frame's limit."""
        n = rgb.shape[0]
        scalar, d_limits = self._per_frame_limit(name, limit, n, rgb.device)
        res = self._encode_candidates(name, fn, rgb, candidates, first_frame_index, (*rule_args, scalar, _ptr(d_limits)), with_dist)
        return res, [scalar] * n if d_limits is None else [int(x) for x in d_limits[:n].cpu()]

    def encode_to_budget(self, rgb, max_frame_bytes, candidates, first_frame_index=0):
        """Synchronous: every frame at the largest of `candidates` (1..8 qualities, strictly increasing, each <= quality_factor)
        whose record fits its budget, else at the smallest.  max_frame_bytes: one budget for every frame, or one per frame
        (a sequence or a CUDA int64 tensor).  Returns (bytes, sizes, chosen, over_budget_frames)."""
        (data, sizes_l, chosen_l, _, _), budgets = self._encode_per_frame(
            "encode_to_budget", "m1v_encode_budget_device", (), rgb, max_frame_bytes, candidates, first_frame_index, False)
        over = [f for f, s in enumerate(sizes_l) if s > budgets[f]]   # (STATUS_OVER_BUDGET is set iff there are any)
        return data, sizes_l, chosen_l, over

    def _encode_rd(self, name, rule, rgb, limit, candidates, first_frame_index):
        """The two rate-distortion encodes: (bytes, sizes, chosen, frames over their limit, distortion per frame)."""
        (data, sizes_l, chosen_l, dist_l, _), limits = self._encode_per_frame(
            name, "m1v_encode_rd_device", (rule,), rgb, limit, candidates, first_frame_index, True)
        bounded = sizes_l if rule == _ffi.RD_BEST_IN_BUDGET else dist_l
        over = [f for f, x in enumerate(bounded) if x > limits[f]]  # (the rule's status bit is set iff there are any)
        return data, sizes_l, chosen_l, over, dist_l

    def encode_best_in_budget(self, rgb, max_frame_bytes, candidates, first_frame_index=0):
        """Synchronous: every frame at the candidate of LEAST DISTORTION among those whose record fits its budget (ties: the
        smaller record, then the smaller quality), else at the candidate of smallest record.  encode_to_budget takes the largest
        quality that fits, which in this encoder can be far from the best picture (include/mpeg1_hip.h, m1v_encode_rd_device).
        max_frame_bytes: one budget for every frame, or one per frame (a sequence or a CUDA int64 tensor).  Candidates that cannot
        be coded are skipped.  Returns (bytes, sizes, chosen, over_budget_frames, distortion)."""
        return self._encode_rd("encode_best_in_budget", _ffi.RD_BEST_IN_BUDGET, rgb, max_frame_bytes, candidates, first_frame_index)

    def encode_to_distortion(self, rgb, max_distortion, candidates, first_frame_index=0):
        """Synchronous: every frame at the candidate of SMALLEST RECORD among those whose distortion (frame_rd_table's measure;
        psnr_to_distortion states it in dB) is at most its ceiling (ties: the less distortion, then the smaller quality), else at
        the candidate of least distortion.  max_distortion: one ceiling for every frame, or one per frame.  Returns
        (bytes, sizes, chosen, over_distortion_frames, distortion)."""
        return self._encode_rd("encode_to_distortion", _ffi.RD_SMALLEST_AT_DISTORTION, rgb, max_distortion, candidates, first_frame_index)

    def distortion_to_psnr(self, d):
        """A frame's distortion as a PSNR in dB (the module's distortion_to_psnr with this encoder's blocks_per_frame).  Pure."""
        return distortion_to_psnr(d, self.blocks_per_frame)

    def psnr_to_distortion(self, db):
        """The distortion ceiling of a frame that a PSNR of db dB stands for (encode_to_distortion's max_distortion).  Pure."""
        return psnr_to_distortion(db, self.blocks_per_frame)

    def encode_to_batch_budget(self, rgb, batch_bytes, candidates, first_frame_index=0):
        """Synchronous: the whole batch within batch_bytes (the sum of its records).  Every frame at one of two neighbouring
        `candidates` (1..8 qualities, strictly increasing, each <= quality_factor): the highest level whose every-frame total
        fits, and the leftover bytes spent on the cheapest upgrades to the next (include/mpeg1_hip.h,
        m1v_encode_batch_budget_device).  over_budget: even every frame at the smallest candidate does not fit (all are there).
        Returns (bytes, sizes, chosen, over_budget)."""
        budget = self._uint64(batch_bytes, "encode_to_batch_budget: batch_bytes")
        data, sizes_l, chosen_l, _, status = self._encode_candidates(
            "encode_to_batch_budget", "m1v_encode_batch_budget_device", rgb, candidates, first_frame_index, (budget,))
        return data, sizes_l, chosen_l, bool(status & _ffi.STATUS_OVER_BUDGET)

    def _encode_rd_batch(self, name, rule, rgb, limit, candidates, first_frame_index):
        """The two batch forms that pick by distortion: (bytes, sizes, chosen, over the limit, distortion per frame)."""
        middle = (rule, self._uint64(limit, f"{name}: the limit"))
        data, sizes_l, chosen_l, dist_l, status = self._encode_candidates(
            name, "m1v_encode_rd_batch_device", rgb, candidates, first_frame_index, middle, with_dist=True)
        bit = _ffi.STATUS_OVER_BUDGET if rule == _ffi.RD_BEST_IN_BUDGET else _ffi.STATUS_OVER_DISTORTION
        return data, sizes_l, chosen_l, bool(status & bit), dist_l

    def encode_best_in_batch_budget(self, rgb, batch_bytes, candidates, first_frame_index=0):
        """Synchronous: the whole batch within batch_bytes (the sum of its records) at the least total distortion the greedy
        on each frame's convex hull finds (include/mpeg1_hip.h, m1v_encode_rd_batch_device): every frame starts at its smallest
        record and the steps along the hulls are taken steepest first (distortion saved per byte) while they fit.  Not the
        knapsack optimum.  encode_to_batch_budget takes the largest qualities that fit, which here can be far from the best
        picture.  over_budget: even every frame at its smallest record does not fit (all are there).  Returns
        (bytes, sizes, chosen, over_budget, distortion)."""
        return self._encode_rd_batch("encode_best_in_batch_budget", _ffi.RD_BEST_IN_BUDGET, rgb, batch_bytes, candidates,
                                     first_frame_index)

    def encode_batch_to_distortion(self, rgb, total_distortion, candidates, first_frame_index=0):
        """Synchronous: the fewest steps of encode_best_in_batch_budget's order after which the batch's distortions sum to at
        most total_distortion.  over_distortion: even every frame at its least distortion does not reach it (all are there; the
        output is valid).  Returns (bytes, sizes, chosen, over_distortion, distortion)."""
        return self._encode_rd_batch("encode_batch_to_distortion", _ffi.RD_SMALLEST_AT_DISTORTION, rgb, total_distortion,
                                     candidates, first_frame_index)

    @staticmethod
    def _bitrate_args(name, bytes_per_frame, buffer_bytes, level):
        import torch
        assert level.is_cuda and level.dtype == torch.int64 and level.numel() == 1, "level: CUDA int64 tensor of one element"
        rate, cap = int(bytes_per_frame), int(buffer_bytes)
        if not 1 <= rate <= cap < 2 ** 62:
            raise EncoderError(_ffi.E_ARG, f"{name}: need 1 <= bytes_per_frame <= buffer_bytes < 2^62")
        return rate, cap

    @staticmethod
    def _over_level(sizes_l, start, rate, cap):
        """The frames whose record exceeds the level before them, replayed from the sizes (STATUS_OVER_BUDGET is set iff there
        are any)."""
        over, L = [], min(start, cap)
        for f, s in enumerate(sizes_l):
            if s > L:
                over.append(f)
            L = min(cap, L - s + rate)
        return over

    def _encode_bitrate(self, name, fn, rgb, bytes_per_frame, buffer_bytes, candidates, level, first_frame_index, with_dist):
        """The two bitrate encodes: (bytes, sizes, chosen, over_budget_frames, distortion per frame or None)."""
        import torch
        rate, cap = self._bitrate_args(name, bytes_per_frame, buffer_bytes, level)
        level_in = level.contiguous()
        start = int(level_in.item())
        level_out = torch.empty(1, dtype=torch.int64, device=level.device)   # a retry starts from the same level
        data, sizes_l, chosen_l, dist_l, _ = self._encode_candidates(
            name, fn, rgb, candidates, first_frame_index, (rate, cap, _ptr(level_in), _ptr(level_out)), with_dist)
        level.copy_(level_out.view_as(level))
        return data, sizes_l, chosen_l, self._over_level(sizes_l, start, rate, cap), dist_l

    def encode_at_bitrate(self, rgb, bytes_per_frame, buffer_bytes, candidates, level, first_frame_index=0):
        """Synchronous constant bitrate (a leaky bucket, include/mpeg1_hip.h m1v_encode_cbr_device): bytes_per_frame per frame
        into a buffer of buffer_bytes.  level: CUDA int64 tensor [1], the bytes available to the next frame; each frame goes at
        the largest of `candidates` whose record fits it, else at the smallest.  The level is advanced over the batch in place,
        only when the call succeeds, so that consecutive calls form one stream.  Returns (bytes, sizes, chosen,
        over_budget_frames)."""
        return self._encode_bitrate("encode_at_bitrate", "m1v_encode_cbr_device", rgb, bytes_per_frame, buffer_bytes, candidates,
                                    level, first_frame_index, False)[:4]

    def encode_best_at_bitrate(self, rgb, bytes_per_frame, buffer_bytes, candidates, level, first_frame_index=0):
        """Synchronous constant bitrate that picks by distortion (include/mpeg1_hip.h, m1v_encode_rd_cbr_device): the leaky bucket
        of encode_at_bitrate, each frame at the candidate of LEAST DISTORTION whose record fits the level (ties: the smaller
        record, then the smaller quality), else at its smallest record.  The level is advanced over the batch in place, only
        when the call succeeds.  Returns (bytes, sizes, chosen, over_budget_frames, distortion)."""
        return self._encode_bitrate("encode_best_at_bitrate", "m1v_encode_rd_cbr_device", rgb, bytes_per_frame, buffer_bytes,
                                    candidates, level, first_frame_index, True)

    @staticmethod
    def _rd_tables(sizes, dist, status):
        import torch
        assert sizes.is_cuda and sizes.dtype == torch.int64 and sizes.dim() == 2, "sizes: CUDA int64 [K, n]"
        assert dist.is_cuda and dist.dtype == torch.int64 and dist.shape == sizes.shape, "dist: CUDA int64 [K, n]"
        K, n = sizes.shape
        if status is not None:
            assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= K, "status: CUDA int32, one per candidate"
        return sizes.contiguous(), dist.contiguous(), K, n

    def rd_batch_pick(self, sizes, dist, rule, limit, status=None):
        """The batch pick alone on an rd table the caller holds (frame_rd_table's two CUDA int64 tensors [K, n]; status: its
        CUDA int32 status words, or None): re-pick at another limit without another table pass.  Synchronous.  Returns
        (picks, over): the candidate INDEX of every frame and whether the rule's limit was missed."""
        import torch
        sizes, dist, K, n = self._rd_tables(sizes, dist, status)
        limit = self._uint64(limit, "rd_batch_pick: the limit")
        picks = torch.zeros(max(n, 1), dtype=torch.uint8, device=sizes.device)
        word = torch.zeros(1, dtype=torch.int32, device=sizes.device)
        _call("m1v_rd_batch_pick_device", self._h, _ptr(sizes), _ptr(dist), _ptr(status), n, K, int(rule), limit, _ptr(picks),
              None, _ptr(word), _stream())
        bits = int(word.item())
        return [int(k) for k in picks[:n].cpu()], bool(bits & (_ffi.STATUS_OVER_BUDGET | _ffi.STATUS_OVER_DISTORTION))

    def rd_bitrate_pick(self, sizes, dist, bytes_per_frame, buffer_bytes, level, status=None):
        """The bitrate pick alone on an rd table the caller holds (as rd_batch_pick).  level: CUDA int64 tensor [1], advanced in
        place.  Synchronous.  Returns (picks, over_frames): the candidate index of every frame and the frames that fitted
        nothing."""
        import torch
        sizes, dist, K, n = self._rd_tables(sizes, dist, status)
        rate, cap = self._bitrate_args("rd_bitrate_pick", bytes_per_frame, buffer_bytes, level)
        level_in = level.contiguous()
        start = int(level_in.item())
        level_out = torch.empty(1, dtype=torch.int64, device=level.device)
        picks = torch.zeros(max(n, 1), dtype=torch.uint8, device=sizes.device)
        word = torch.zeros(1, dtype=torch.int32, device=sizes.device)
        _call("m1v_rd_cbr_pick_device", self._h, _ptr(sizes), _ptr(dist), _ptr(status), n, K, rate, cap, _ptr(level_in),
              _ptr(level_out), _ptr(picks), None, _ptr(word), _stream())
        picks_l = [int(k) for k in picks[:n].cpu()]
        level.copy_(level_out.view_as(level))
        rows = sizes.cpu()
        return picks_l, self._over_level([int(rows[k, f]) for f, k in enumerate(picks_l)], start, rate, cap)

    # ---- batches of many streams (include/mpeg1_hip.h, "Streams") ----------------------------------------------------------
    @staticmethod
    def _spans(spans, n, device):
        """`spans` as a StreamSpans on the device: what stream_spans() made, or the pairs it takes.  They must add up to n."""
        if not isinstance(spans, StreamSpans):
            spans = stream_spans(spans, device)
        assert spans.n_frames == n, f"the spans hold {spans.n_frames} frames, the batch {n}"
        return spans

    def encode_streams_device(self, rgb, spans, out=None, sizes=None, meta=None, stream_bytes=None, quality=None):
        """encode() for a batch that is the concatenation of `spans` (what stream_spans() returns: the spans are not checked on
        the host, the device reports STATUS_STREAMS in meta[1]).  Asynchronous on torch's current stream.  Returns
        (out, sizes, meta, stream_bytes): encode()'s three and int64[n_streams], the bytes of each stream's records, which lie in
        `out` back to back in batch order."""
        import torch
        n = rgb.shape[0]
        self._check_input(rgb)
        if out is None:
            out = torch.empty(self.default_out_capacity(n), dtype=torch.uint8, device=rgb.device)
        if sizes is None:
            sizes = torch.empty(max(n, 1), dtype=torch.int64, device=rgb.device)
        if meta is None:
            meta = torch.zeros(2, dtype=torch.int64, device=rgb.device)
        if stream_bytes is None:
            stream_bytes = torch.empty(len(spans), dtype=torch.int64, device=rgb.device)
        q = self._quality_tensor(quality, n, rgb.device) if quality is not None else None
        _call("m1v_encode_streams_device", self._h, _ptr(rgb), n, _ptr(spans), len(spans), _ptr(q), _ptr(out), out.numel(),
              _ptr(sizes), _ptr(stream_bytes), *_meta_ptrs(meta), _stream())
        return out, sizes, meta, stream_bytes

    def encode_streams(self, rgb, spans, quality=None):
        """Synchronous: one batch of many streams.  spans: stream_spans([(n_frames, first_frame_index), ...]) or those pairs, one
        per stream in batch order; frame j of a span is frame first_frame_index + j of its stream, and its record is what
        encode(..., first_frame_index=...) gives for it.  quality: as in encode().  Returns (bytes, sizes, stream_bytes): the
        records in batch order, each record's size, and the bytes of each stream's contiguous range."""
        import torch
        n = rgb.shape[0]
        spans = self._spans(spans, n, rgb.device)
        if quality is not None:
            quality = self._quality_tensor(quality, n, rgb.device)
        stream_bytes = torch.zeros(len(spans), dtype=torch.int64, device=rgb.device)
        data, sizes_l, _ = self._encode_retrying(
            rgb, "encode_streams",
            lambda out, sizes, meta: self.encode_streams_device(rgb, spans, out, sizes, meta, stream_bytes, quality))
        return data, sizes_l, [int(b) for b in stream_bytes.cpu()]

    @staticmethod
    def _stream_rates(name, bytes_per_frame, buffer_bytes, n_streams, device):
        """One rate for every stream (scalars, checked here) or one per stream (sequences, or bytes_per_frame a CUDA int64 tensor
        [n_streams, 2] of (bytes_per_frame, buffer_bytes); checked on the device): (rate, cap, tensor or None)."""
        import torch
        if isinstance(bytes_per_frame, torch.Tensor):
            assert bytes_per_frame.is_cuda and bytes_per_frame.dtype == torch.int64 and tuple(bytes_per_frame.shape) == (n_streams, 2), \
                "rates: CUDA int64 [n_streams, 2]"
            return 0, 0, bytes_per_frame.contiguous()
        if isinstance(bytes_per_frame, numbers.Integral) and isinstance(buffer_bytes, numbers.Integral):
            rate, cap = int(bytes_per_frame), int(buffer_bytes)
            if not 1 <= rate <= cap < 2 ** 62:
                raise EncoderError(_ffi.E_ARG, f"{name}: need 1 <= bytes_per_frame <= buffer_bytes < 2^62")
            return rate, cap, None
        per_stream = [[x] * n_streams if isinstance(x, numbers.Integral) else list(x) for x in (bytes_per_frame, buffer_bytes)]
        assert all(len(x) == n_streams for x in per_stream), "rates: one per stream"
        rates = [[int(r), int(c)] for r, c in zip(*per_stream)]
        if any(not 0 <= x < 2 ** 63 for row in rates for x in row):
            raise EncoderError(_ffi.E_ARG, f"{name}: rates must fit int64")
        return 0, 0, torch.tensor(rates, dtype=torch.int64).to(device)

    @staticmethod
    def _levels(levels, n_streams):
        import torch
        assert isinstance(levels, torch.Tensor) and levels.is_cuda and levels.dtype == torch.int64 and levels.numel() == n_streams, \
            "levels: CUDA int64 tensor, one element per stream"

    def encode_streams_at_bitrate(self, rgb, spans, candidates, bytes_per_frame, buffer_bytes, levels, by="size"):
        """Synchronous constant bitrate with one leaky bucket per stream (include/mpeg1_hip.h, m1v_encode_streams_cbr_device): one
        table pass, one pick and one encode for the whole batch.  spans: as in encode_streams.  bytes_per_frame, buffer_bytes: one
        rate for every stream, or one per stream (sequences).  levels: CUDA int64 tensor [n_streams], the bytes available to each
        stream's next frame, advanced in place, only when the call succeeds.  by: "size" (each frame at the largest candidate
        whose record fits its stream's level, encode_at_bitrate's pick) or "distortion" (the least distortion that fits,
        encode_best_at_bitrate's).  Returns (bytes, sizes, chosen, stream_bytes, over_budget, distortion or None)."""
        import torch
        n = rgb.shape[0]
        name = "encode_streams_at_bitrate"
        self._check_input(rgb)
        spans = self._spans(spans, n, rgb.device)
        rule = _ffi.STREAMS_RULES[by]
        rate, cap, d_rates = self._stream_rates(name, bytes_per_frame, buffer_bytes, len(spans), rgb.device)
        self._levels(levels, len(spans))
        level_in = levels.contiguous()
        level_out = torch.empty_like(level_in)                               # a retry starts from the same levels
        cand_buf = self._candidates(candidates, name)
        chosen = torch.zeros(max(n, 1), dtype=torch.uint8, device=rgb.device)
        with_dist = rule == _ffi.STREAMS_LEAST_DISTORTION
        dist = torch.zeros(max(n, 1), dtype=torch.int64, device=rgb.device) if with_dist else None
        stream_bytes = torch.zeros(len(spans), dtype=torch.int64, device=rgb.device)
        data, sizes_l, status = self._encode_retrying(
            rgb, name,
            lambda out, sizes, meta: _call(
                "m1v_encode_streams_cbr_device", self._h, _ptr(rgb), n, _ptr(spans), len(spans), cand_buf, len(cand_buf), rule,
                rate, cap, _ptr(d_rates), _ptr(level_in), _ptr(level_out), _ptr(chosen), _ptr(out), out.numel(), _ptr(sizes),
                _ptr(dist), _ptr(stream_bytes), *_meta_ptrs(meta), _stream()))
        levels.copy_(level_out.view_as(levels))
        return (data, sizes_l, [int(c) for c in chosen[:n].cpu()], [int(b) for b in stream_bytes.cpu()],
                bool(status & _ffi.STATUS_OVER_BUDGET), [int(d) for d in dist[:n].cpu()] if with_dist else None)

    def streams_bitrate_pick(self, sizes, dist, spans, bytes_per_frame, buffer_bytes, levels, by="size", status=None, levels_out=None):
        """The pick of encode_streams_at_bitrate alone, on a table the caller holds (frame_size_table's or frame_rd_table's CUDA
        int64 tensors [K, n]; dist may be None when by="size"; status: the table's CUDA int32 status words, or None).  The
        spans and per-stream rates are checked on the device.  levels: CUDA int64 [n_streams], advanced in place, or, with
        levels_out (CUDA int64 [n_streams], which may be `levels` itself), left alone while levels_out receives the new
        levels.  Synchronous.  Returns (picks, distortion, status bits): the candidate INDEX of every frame, the picks'
        distortion (None without dist) and the pick's status word (STATUS_OVER_BUDGET, STATUS_STREAMS, ...)."""
        import torch
        assert sizes.is_cuda and sizes.dtype == torch.int64 and sizes.dim() == 2, "sizes: CUDA int64 [K, n]"
        K, n = sizes.shape
        sizes = sizes.contiguous()
        if dist is not None:
            assert dist.is_cuda and dist.dtype == torch.int64 and dist.shape == sizes.shape, "dist: CUDA int64 [K, n]"
            dist = dist.contiguous()
        if status is not None:
            assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= K, "status: CUDA int32, one per candidate"
        if not isinstance(spans, StreamSpans):
            spans = stream_spans(spans, sizes.device)
        rate, cap, d_rates = self._stream_rates("streams_bitrate_pick", bytes_per_frame, buffer_bytes, len(spans), sizes.device)
        self._levels(levels, len(spans))
        level_in = levels.contiguous()
        if levels_out is not None:
            self._levels(levels_out, len(spans))
            assert levels_out.is_contiguous()
        level_out = levels_out if levels_out is not None else torch.empty_like(level_in)
        picks = torch.zeros(max(n, 1), dtype=torch.uint8, device=sizes.device)
        pick_dist = torch.zeros(max(n, 1), dtype=torch.int64, device=sizes.device) if dist is not None else None
        word = torch.zeros(1, dtype=torch.int32, device=sizes.device)
        _call("m1v_streams_cbr_pick_device", self._h, _ptr(sizes), _ptr(dist), _ptr(status), n, K, _ptr(spans), len(spans),
              _ffi.STREAMS_RULES[by], rate, cap, _ptr(d_rates), _ptr(level_in), _ptr(level_out), _ptr(picks), _ptr(pick_dist),
              _ptr(word), _stream())
        bits = int(word.item()) & 0xFFFFFFFF
        if levels_out is None:
            levels.copy_(level_out.view_as(levels))
        return ([int(k) for k in picks[:n].cpu()], [int(d) for d in pick_dist[:n].cpu()] if pick_dist is not None else None, bits)

    # ---- a budget per stream (include/mpeg1_hip.h, "Streams: a budget per stream") ------------------------------------------
    @staticmethod
    def _stream_limits(name, limits, n_streams, device):
        """One limit for every stream (a scalar, checked here) or one per stream (a sequence of uint64 values, or a CUDA int64
        tensor [n_streams] that holds their bit patterns): (limit, tensor or None)."""
        import torch
        if isinstance(limits, torch.Tensor):
            assert limits.is_cuda and limits.dtype == torch.int64 and limits.numel() == n_streams, "limits: CUDA int64 [n_streams]"
            return 0, limits.contiguous()
        if isinstance(limits, numbers.Integral):
            return Mpeg1Encoder._uint64(limits, f"{name}: the limit"), None
        per_stream = [Mpeg1Encoder._uint64(x, f"{name}: a limit") for x in limits]
        assert len(per_stream) == n_streams, "limits: one per stream"
        return 0, torch.tensor([x - 2 ** 64 if x >= 2 ** 63 else x for x in per_stream], dtype=torch.int64).to(device)

    def _encode_streams_budget(self, name, rule, rgb, spans, candidates, limits):
        """The encodes with a budget per stream: (bytes, sizes, chosen, stream_bytes, over, distortion per frame or None, the
        status word of every stream)."""
        import torch
        n = rgb.shape[0]
        self._check_input(rgb)
        spans = self._spans(spans, n, rgb.device)
        limit, d_limits = self._stream_limits(name, limits, len(spans), rgb.device)
        cand_buf = self._candidates(candidates, name)
        chosen = torch.zeros(max(n, 1), dtype=torch.uint8, device=rgb.device)
        with_dist = rule != _ffi.SPANS_LARGEST_THAT_FITS
        dist = torch.zeros(max(n, 1), dtype=torch.int64, device=rgb.device) if with_dist else None
        stream_bytes = torch.zeros(len(spans), dtype=torch.int64, device=rgb.device)
        stream_status = torch.zeros(len(spans), dtype=torch.int32, device=rgb.device)
        data, sizes_l, status = self._encode_retrying(
            rgb, name,
            lambda out, sizes, meta: _call(
                "m1v_encode_streams_budget_device", self._h, _ptr(rgb), n, _ptr(spans), len(spans), cand_buf, len(cand_buf), rule,
                limit, _ptr(d_limits), _ptr(chosen), _ptr(out), out.numel(), _ptr(sizes), _ptr(dist), _ptr(stream_bytes),
                _ptr(stream_status), *_meta_ptrs(meta), _stream()))
        return (data, sizes_l, [int(c) for c in chosen[:n].cpu()], [int(b) for b in stream_bytes.cpu()],
                bool(status & _ffi.SPANS_OVER_BITS[rule]), [int(d) for d in dist[:n].cpu()] if with_dist else None,
                [int(w) & 0xFFFFFFFF for w in stream_status.cpu()])

    def encode_streams_to_budget(self, rgb, spans, candidates, limits, by="size"):
        """Synchronous: every stream of the batch within its own byte budget (include/mpeg1_hip.h,
        m1v_encode_streams_budget_device): one table pass, one pick and one encode for the whole batch.  spans: as in
        encode_streams.  limits: bytes for the sum of a stream's records; one for every stream, or one per stream (a sequence or a
        CUDA int64 tensor [n_streams]).  by: "size" (encode_to_batch_budget's pick on each stream's frames alone) or "distortion"
        (encode_best_in_batch_budget's).  Returns (bytes, sizes, chosen, stream_bytes, over_budget, distortion or None,
        stream_status): over_budget says that some stream does not fit even at its smallest records, stream_status which
        (STATUS_OVER_BUDGET per stream, or 0)."""
        assert by in ("size", "distortion"), 'by: "size" or "distortion"'
        return self._encode_streams_budget("encode_streams_to_budget", _ffi.SPANS_RULES[by], rgb, spans, candidates, limits)

    def encode_streams_to_distortion(self, rgb, spans, candidates, ceilings):
        """Synchronous: every stream of the batch at the fewest bytes whose distortions sum to at most the stream's ceiling
        (encode_batch_to_distortion's pick on each stream's frames alone).  ceilings: one for every stream, or one per stream.
        Returns (bytes, sizes, chosen, stream_bytes, over_distortion, distortion, stream_status): STATUS_OVER_DISTORTION per
        stream whose ceiling even its least distortion misses (the output is valid)."""
        return self._encode_streams_budget("encode_streams_to_distortion", _ffi.SPANS_SMALLEST_AT_DISTORTION, rgb, spans,
                                           candidates, ceilings)

    def streams_budget_pick(self, sizes, dist, spans, rule, limits, status=None):
        """The pick of the two encodes above alone, on a table the caller holds (frame_size_table's or frame_rd_table's CUDA int64
        tensors [K, n]; dist may be None under SPANS_LARGEST_THAT_FITS; status: the table's CUDA int32 status words, or None).
        rule: a SPANS_* value.  limits: as in encode_streams_to_budget.  The spans are checked on the device.  Synchronous.
        Returns (picks, distortion, status bits, stream_status): the candidate INDEX of every frame, the picks' distortion (None
        without dist), the pick's status word and the status word of every stream."""
        import torch
        assert sizes.is_cuda and sizes.dtype == torch.int64 and sizes.dim() == 2, "sizes: CUDA int64 [K, n]"
        K, n = sizes.shape
        sizes = sizes.contiguous()
        if dist is not None:
            assert dist.is_cuda and dist.dtype == torch.int64 and dist.shape == sizes.shape, "dist: CUDA int64 [K, n]"
            dist = dist.contiguous()
        if status is not None:
            assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= K, "status: CUDA int32, one per candidate"
        if not isinstance(spans, StreamSpans):
            spans = stream_spans(spans, sizes.device)
        limit, d_limits = self._stream_limits("streams_budget_pick", limits, len(spans), sizes.device)
        picks = torch.zeros(max(n, 1), dtype=torch.uint8, device=sizes.device)
        pick_dist = torch.zeros(max(n, 1), dtype=torch.int64, device=sizes.device) if dist is not None else None
        stream_status = torch.zeros(len(spans), dtype=torch.int32, device=sizes.device)
        word = torch.zeros(1, dtype=torch.int32, device=sizes.device)
        _call("m1v_streams_budget_pick_device", self._h, _ptr(sizes), _ptr(dist), _ptr(status), n, K, _ptr(spans), len(spans),
              int(rule), limit, _ptr(d_limits), _ptr(picks), _ptr(pick_dist), _ptr(stream_status), _ptr(word), _stream())
        bits = int(word.item()) & 0xFFFFFFFF
        return ([int(k) for k in picks[:n].cpu()], [int(d) for d in pick_dist[:n].cpu()] if pick_dist is not None else None, bits,
                [int(w) & 0xFFFFFFFF for w in stream_status.cpu()])

    def set_pipelined(self, enable=True):
        """Overlap each batch's layout + gather (internal stream) with the next batch's encode kernel.
        Outputs of a batch are complete only behind flush(); callers double-buffer `out`."""
        _call("m1v_set_pipelined", self._h, 1 if enable else 0)

    def flush(self, stream=None):
        """Make `stream` (torch stream, default: the current one) wait for all pending gathers."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream()
        _call("m1v_flush", self._h, C.c_void_p(st.cuda_stream))

    def default_out_capacity(self, n):
        # typical output is far below the worst-case bound; callers that need the guarantee pass
        # `out` of frame_bound * n bytes.  NOSPACE is reported through the status word.
        return int(min(self.frame_bound, self.frame_bytes_in // 2 + 4096) * max(n, 1))

    def encode_to_bytes(self, rgb, first_frame_index=0, quality=None):
        """Synchronous convenience: returns (bytes, [sizes]).  quality: as in encode()."""
        if quality is not None:     # one upload, reused by a retry
            quality = self._quality_tensor(quality, rgb.shape[0], rgb.device)
        data, sizes_l, _ = self._encode_retrying(
            rgb, "encode", lambda out, sizes, meta: self.encode(rgb, first_frame_index, out, sizes, meta, quality))
        return data, sizes_l

    def encode_host(self, rgb_np, first_frame_index=0, with_planes=False):
        """numpy uint8 [n,H,W,C] through the host-buffer entry point (PCIe inclusive).  with_planes: also return the
        uint8 [n,3,H*W] Y/Cb/Cr planes from the same upload (m1v_encode_planes_host: the image_<k>.bit content)."""
        import numpy as np
        rgb_np = np.ascontiguousarray(rgb_np, dtype=np.uint8)
        n = rgb_np.shape[0]
        cap = self.frame_bound * max(n, 1)
        out = np.empty(cap, np.uint8)
        sizes = np.zeros(max(n, 1), np.uint64)
        planes = np.empty((n, 3, self.height * self.width), np.uint8) if with_planes else None
        rc = _ffi.lib().m1v_encode_planes_host(self._h, rgb_np.ctypes.data, n, int(first_frame_index), out.ctypes.data,
                                               cap, sizes.ctypes.data, planes.ctypes.data if with_planes and n else None)
        if rc < 0:
            raise EncoderError(rc, "m1v_encode_planes_host")
        res = out[:rc].tobytes(), [int(s) for s in sizes[:n]]
        return res + (planes,) if with_planes else res

    # ---- partial pipelines --------------------------------------------------------------------
    def coefficients(self, rgb):
        """int16 [n, strips*mb_rows*6, 64] zigzag-ordered quantised levels (BASELINE config 2)."""
        import torch
        n = rgb.shape[0]
        out = torch.empty((n, self.blocks_per_frame, 64), dtype=torch.int16, device=rgb.device)
        _call("m1v_coefficients_device", self._h, _ptr(rgb), n, _ptr(out), _stream())
        return out

    def convert(self, rgb):
        """uint8 [n, 3, H*W]: Y, full-resolution Cb, full-resolution Cr."""
        import torch
        n = rgb.shape[0]
        out = torch.empty((n, 3, self.height * self.width), dtype=torch.uint8, device=rgb.device)
        _call("m1v_convert_device", self._h, _ptr(rgb), n, _ptr(out), _stream())
        return out

    def subsample(self, cb, cr):
        import torch
        n = (self.width // 2) * (self.height // 2)
        a = torch.empty(n, dtype=torch.uint8, device=cb.device)
        b = torch.empty(n, dtype=torch.uint8, device=cb.device)
        _call("m1v_subsample_device", self._h, _ptr(cb), _ptr(cr), _ptr(a), _ptr(b), _stream())
        return a, b

    def synth(self, n_frames, seed=504, first_frame_index=0, device=None, out=None):
        """Device-generated synthetic frames (identical to oracle orc_synth_frame by definition).  out: reuse this tensor."""
        import torch
        dev = device or torch.device("cuda", self.device)
        rgb = out if out is not None else torch.empty((n_frames, self.height, self.width, self.channels), dtype=torch.uint8, device=dev)
        assert rgb.numel() == n_frames * self.frame_bytes_in and rgb.is_contiguous()
        _call("m1v_synth_device", _ptr(rgb), self.frame_bytes_in, n_frames, seed, first_frame_index, _stream())
        return rgb

    # ---- measurement ----------------------------------------------------------------------------
    def profile(self, enable=True):
        _ffi.lib().m1v_profile_enable(self._h, 1 if enable else 0)

    def profile_read(self):
        n, ms = C.c_int(0), C.c_double(0.0)
        _call("m1v_profile_read", self._h, C.byref(n), C.byref(ms))
        return n.value, ms.value

    def profile_read_times(self, cap=4096):
        """Durations (ms) of the dominant kernel's launches since profile(True), in launch order."""
        buf, n = (C.c_float * cap)(), C.c_int(0)
        _call("m1v_profile_read_times", self._h, buf, cap, C.byref(n))
        return [float(buf[i]) for i in range(min(n.value, cap))]

    def reserve_scratch(self, worst_case=True):
        """Size the overflow arena for every run (True) or return to the default 1/256 (False); see mpeg1_hip.h."""
        _call("m1v_reserve_scratch", self._h, 1 if worst_case else 0)

    def scratch_bytes(self):
        return int(_ffi.lib().m1v_scratch_bytes(self._h))

    def debug_set_input_mode(self, mode):
        """Test hook: -1 automatic, 0 byte loads, 2 funnel-shifted 28-byte loads (see mpeg1_hip.h)."""
        _call("m1v_debug_set_input_mode", self._h, int(mode))

    def debug_set_path(self, path):
        """Test hook: which encode kernel serves the batches: -1 by geometry, 0 runs, 1 tiles (see mpeg1_hip.h)."""
        _call("m1v_debug_set_path", self._h, {"auto": -1, "runs": 0, "tiles": 1}.get(path, path))

    @property
    def path(self):
        return "tiles" if _ffi.lib().m1v_path_in_use(self._h) == 1 else "runs"

    @property
    def size_table_fused(self):
        """1: a size table (and the table of a budget, batch-budget or bitrate call) is one fused pass; 0: one probe per
        quality (an encoder forced by a debug hook)."""
        return _ffi.lib().m1v_size_table_fused(self._h)

    def debug_set_lds_words(self, words):
        _call("m1v_debug_set_lds_words", self._h, int(words))

    def debug_set_dense_threads(self, threads):
        _call("m1v_debug_set_dense_threads", self._h, int(threads))

    def debug_assemble_shape(self):
        """Test hook: the assembly kernel's shape under the plan in force, as (group, lanes_log2, segs, producer) with the
        producer "tiles", "dense" or "strips" (see mpeg1_hip.h)."""
        out = (C.c_int * 4)()
        _call("m1v_debug_assemble_shape", self._h, out)
        return out[0], out[1], out[2], ("tiles", "dense", "strips")[out[3]]

    def debug_set_assemble_shape(self, group=0, lanes_log2=0):
        """Test hook: force the assembly kernel's strips per workgroup and lanes per segment; 0 = the plan's own (see mpeg1_hip.h)."""
        _call("m1v_debug_set_assemble_shape", self._h, int(group), int(lanes_log2))


def file_prolog():
    buf = (C.c_uint8 * 27)()
    _ffi.lib().m1v_file_prolog(buf)
    return bytes(buf)


# ---- the coarse entry point, as the reference spells it --------------------------------------------
_LOAD_FN = C.CFUNCTYPE(C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int)
_FREE_FN = C.CFUNCTYPE(None, C.c_void_p)
_keepalive = {}


def set_image_loader(load):
    """Register a Python image loader with the library (include/encoder.h: encoder_set_image_loader).
    `load(path: str) -> numpy uint8 array [H, W, C]` or None.  C callers normally get stb_image registered by
    including encoder.h; Python callers can plug in any decoder (pixels then are that decoder's, not stb's)."""
    import numpy as np
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]

    def _load(path, pw, ph, pc, desired):
        arr = load(path.decode())
        if arr is None:
            return None
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        h, w, c = arr.shape
        buf = libc.malloc(arr.nbytes)
        C.memmove(buf, arr.ctypes.data, arr.nbytes)
        pw[0], ph[0], pc[0] = w, h, c
        return buf

    def _free(p):
        libc.free(p)

    cb = (_LOAD_FN(_load), _FREE_FN(_free))
    _keepalive["loader"] = cb
    _ffi.lib().encoder_set_image_loader(C.cast(cb[0], C.c_void_p), C.cast(cb[1], C.c_void_p))


def mpeg_encode_procedure(images_folder, bitstream_folder, video_path, quality_factor, region=None):
    """int mpeg_encode_procedure(images_folder, bitstream_folder, video_path, quality_factor) — the reference's
    one public operator (include/encoder.h:20), same arguments, same return codes (0 ok, 1 cannot open video,
    -1 folder/images/dimension problems).  region: None = library default (the reference's 96x144 corner unless
    EC504_ENCODE_REGION=full), "strict" or "full"."""
    L = _ffi.lib()
    args = [str(images_folder).encode(), str(bitstream_folder).encode(), str(video_path).encode(), int(quality_factor)]
    if region is None:
        return L.mpeg_encode_procedure(*args)
    return L.mpeg_encode_procedure_region(*args, 1 if region == "full" else 0)
