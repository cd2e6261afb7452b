"""ctypes binding of the in-tree libencoder.so (include/mpeg1_hip.h + include/encoder.h).

The library is the product: hand-written HIP kernels for gfx950 behind a C-ABI.  There is no CPU
fallback — if the shared object is missing or cannot be loaded this module raises.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# EC504_LIBENCODER: a library variant (tools/mkvariant.sh) instead of the in-tree build, for the tuning tools
LIB_PATH = os.environ.get("EC504_LIBENCODER") or os.path.join(PKG_DIR, "libencoder.so")

MODE_STRICT, MODE_FULL = 0, 1
OK, E_ARG, E_UNENCODABLE, E_NOSPACE, E_HIP, E_NODEVICE, E_SCRATCH = 0, -1, -2, -3, -4, -5, -6
STATUS_UNENCODABLE, STATUS_NOSPACE, STATUS_SCRATCH, STATUS_QUALITY, STATUS_OVER_BUDGET = 1, 2, 4, 8, 16
STATUS_OVER_DISTORTION = 32
RD_BEST_IN_BUDGET, RD_SMALLEST_AT_DISTORTION = 0, 1
MAX_CANDIDATES = 8
ORDER_RGB, ORDER_BGR = 0, 1
PLANES_REFERENCE, PLANES_I420, PLANES_YV12, PLANES_NV12, PLANES_NV21 = 0, 1, 2, 3, 4
PLANE_PRESETS = {"reference": PLANES_REFERENCE, "i420": PLANES_I420, "yv12": PLANES_YV12, "nv12": PLANES_NV12, "nv21": PLANES_NV21}


class _Layout(C.Structure):
    """What the layout structs of include/mpeg1_hip.h share: every field is a count of bytes."""

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class PlaneLayout(_Layout):
    """m1v_plane_layout (include/mpeg1_hip.h): where the Y, Cb and Cr samples of a frame lie, in bytes."""
    _fields_ = [(name, C.c_size_t) for name in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")]

SAMPLES_YUY2, SAMPLES_UYVY, SAMPLES_YVYU, SAMPLES_P010 = 0, 1, 2, 3
SAMPLE_PRESETS = {"yuy2": SAMPLES_YUY2, "uyvy": SAMPLES_UYVY, "yvyu": SAMPLES_YVYU, "p010": SAMPLES_P010}


class SampleLayout(_Layout):
    """m1v_sample_layout (include/mpeg1_hip.h): the plane layout with the distance between neighbouring luma samples."""
    _fields_ = [(name, C.c_size_t) for name in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "y_step", "c_step", "frame_stride")]

RGB_PLANES_RGB, RGB_PLANES_BGR, RGB_PLANES_GBR = 0, 1, 2
RGB_PLANE_ORDERS = {"rgb": RGB_PLANES_RGB, "bgr": RGB_PLANES_BGR, "gbr": RGB_PLANES_GBR}


class RgbPlaneLayout(_Layout):
    """m1v_rgb_plane_layout (include/mpeg1_hip.h): where the R, G and B bytes of a frame lie, in bytes."""
    _fields_ = [(name, C.c_uint64) for name in ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")]

SAMPLE_F16, SAMPLE_BF16, SAMPLE_F32 = 0, 1, 2
FLOAT_SAMPLES = {"float16": SAMPLE_F16, "bfloat16": SAMPLE_BF16, "float32": SAMPLE_F32}
FLOAT_SAMPLE_BYTES = {SAMPLE_F16: 2, SAMPLE_BF16: 2, SAMPLE_F32: 4}
FLOAT_SAMPLE_DTYPES = {code: name for name, code in FLOAT_SAMPLES.items()}   # the torch dtype's name: getattr(torch, ...)
RANGE_UNIT, RANGE_BYTE = 0, 1
FLOAT_RANGES = {"unit": RANGE_UNIT, "byte": RANGE_BYTE}


class FloatPlaneLayout(_Layout):
    """m1v_float_plane_layout (include/mpeg1_hip.h): where the float R, G and B samples of a frame lie, in bytes, their type
    (SAMPLE_*) and their value range (RANGE_*)."""
    _fields_ = [(name, C.c_uint64) for name in ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")] + \
               [("sample", C.c_int32), ("range", C.c_int32)]


class FloatPixelLayout(_Layout):
    """m1v_float_pixel_layout (include/mpeg1_hip.h): where the float samples of a frame's interleaved pixels lie, in bytes, which
    of a pixel's samples are R, G and B (ORDER_*), their type (SAMPLE_*) and their value range (RANGE_*)."""
    _fields_ = [(name, C.c_uint64) for name in ("row_pitch", "frame_stride", "pixel_step")] + \
               [("order", C.c_int32), ("sample", C.c_int32), ("range", C.c_int32)]

PIXEL_ORDERS = {"rgb": ORDER_RGB, "bgr": ORDER_BGR}


class DownscaleLayout(_Layout):
    """m1v_downscale_layout (include/mpeg1_hip.h): where the bytes of a frame's SOURCE pixels lie (a surface of twice the encoder's
    width and height), in bytes, which of a pixel's bytes are R, G and B (ORDER_*), and the factor (2)."""
    _fields_ = [(name, C.c_uint64) for name in ("row_pitch", "frame_stride", "pixel_step")] + \
               [("order", C.c_int32), ("factor", C.c_int32)]


class DownscalePlaneLayout(_Layout):
    """m1v_downscale_plane_layout (include/mpeg1_hip.h): where the Y, Cb and Cr samples of a frame's SOURCE lie (4:2:0 planes of
    twice the encoder's width and height), in bytes, the factor (2) and a reserved 0."""
    _fields_ = [(name, C.c_uint64) for name in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")] + \
               [("factor", C.c_int32), ("reserved", C.c_int32)]


class DownscaleWordLayout(_Layout):
    """m1v_downscale_word_layout (include/mpeg1_hip.h): where the Y, Cb and Cr words of a frame's SOURCE lie (4:2:0 planes of 16-bit
    little-endian words, twice the encoder's width and height), in bytes, the factor (2) and the shift from average to sample."""
    _fields_ = [(name, C.c_uint64) for name in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")] + \
               [("factor", C.c_int32), ("shift", C.c_int32)]


# m1v_downscale_word_layout_preset: the tightly packed sources
WORDS_P010, WORDS_I010, WORDS_I012, WORDS_I016 = 0, 1, 2, 3
WORD_PRESETS = {"p010": WORDS_P010, "p012": WORDS_P010, "p016": WORDS_P010, "i010": WORDS_I010, "i012": WORDS_I012, "i016": WORDS_I016}

STATUS_STREAMS = 64
MAX_STREAMS = 4096
STREAMS_LARGEST_THAT_FITS, STREAMS_LEAST_DISTORTION = 0, 1
STREAMS_RULES = {"size": STREAMS_LARGEST_THAT_FITS, "distortion": STREAMS_LEAST_DISTORTION}
SPANS_LARGEST_THAT_FITS, SPANS_LEAST_DISTORTION, SPANS_SMALLEST_AT_DISTORTION = 0, 1, 2
# the rule of a budget per stream: what the limit bounds and what the pick goes by -> the rule, and the bit a stream over it sets
SPANS_RULES = {"size": SPANS_LARGEST_THAT_FITS, "distortion": SPANS_LEAST_DISTORTION, "ceiling": SPANS_SMALLEST_AT_DISTORTION}
SPANS_OVER_BITS = {SPANS_LARGEST_THAT_FITS: STATUS_OVER_BUDGET, SPANS_LEAST_DISTORTION: STATUS_OVER_BUDGET,
                   SPANS_SMALLEST_AT_DISTORTION: STATUS_OVER_DISTORTION}


class StreamSpan(C.Structure):
    """m1v_stream_span (include/mpeg1_hip.h): the frames of one stream in a batch.  The array the calls take lives on the device."""
    _fields_ = [("first_frame", C.c_uint32), ("n_frames", C.c_uint32), ("first_frame_index", C.c_int32), ("reserved", C.c_uint32)]


class StreamRate(C.Structure):
    """m1v_stream_rate (include/mpeg1_hip.h): the refill per frame and the buffer of one stream's leaky bucket, in bytes."""
    _fields_ = [("bytes_per_frame", C.c_uint64), ("buffer_bytes", C.c_uint64)]

_u8p = C.POINTER(C.c_uint8)

# every symbol include/mpeg1_hip.h declares (tests check that the library exports all of them)
MPEG1_HIP_SYMBOLS = [
    "m1v_device_count", "m1v_warm_up", "m1v_last_error", "m1v_create", "m1v_batch_limit", "m1v_destroy", "m1v_strips",
    "m1v_mb_rows", "m1v_frame_bound", "m1v_frame_bound_for", "m1v_frame_bytes_in", "m1v_file_prolog", "m1v_encode_device", "m1v_encode_host",
    "m1v_encode_planes_host", "m1v_encode_quality_device", "m1v_frame_sizes_device", "m1v_encode_budget_device",
    "m1v_frame_size_table_device", "m1v_encode_batch_budget_device", "m1v_encode_cbr_device",
    "m1v_frame_rd_table_device", "m1v_encode_rd_device",
    "m1v_encode_rd_batch_device", "m1v_encode_rd_cbr_device", "m1v_rd_batch_pick_device", "m1v_rd_cbr_pick_device",
    "m1v_encode_streams_device", "m1v_encode_streams_cbr_device", "m1v_streams_cbr_pick_device",
    "m1v_encode_streams_budget_device", "m1v_streams_budget_pick_device",
    "m1v_set_pipelined", "m1v_flush", "m1v_alloc_host", "m1v_free_host", "m1v_alloc_device", "m1v_free_device",
    "m1v_coefficients_device", "m1v_convert_device", "m1v_convert_host", "m1v_subsample_device", "m1v_synth_device",
    "m1v_profile_enable", "m1v_profile_read", "m1v_profile_read_times", "m1v_debug_set_lds_words", "m1v_debug_set_dense_threads",
    "m1v_debug_set_input_mode", "m1v_reserve_scratch", "m1v_scratch_bytes", "m1v_debug_set_path", "m1v_path_in_use", "m1v_debug_fail_alloc",
    "m1v_debug_fail_encode", "m1v_debug_assemble_shape", "m1v_debug_set_assemble_shape", "m1v_size_table_fused", "m1v_set_input_layout", "m1v_input_layout",
    "m1v_plane_layout_preset", "m1v_set_plane_layout", "m1v_plane_layout_in_force",
    "m1v_sample_layout_preset", "m1v_set_sample_layout", "m1v_sample_layout_in_force",
    "m1v_rgb_plane_layout_preset", "m1v_set_rgb_plane_layout", "m1v_rgb_plane_layout_in_force",
    "m1v_float_plane_layout_preset", "m1v_set_float_plane_layout", "m1v_float_plane_layout_in_force", "m1v_float_planes_to_bytes_device",
    "m1v_float_pixel_layout_preset", "m1v_set_float_pixel_layout", "m1v_float_pixel_layout_in_force", "m1v_float_pixels_to_bytes_device",
    "m1v_downscale_layout_preset", "m1v_set_downscale_layout", "m1v_downscale_layout_in_force", "m1v_downscale_to_bytes_device",
    "m1v_downscale_plane_layout_preset", "m1v_set_downscale_plane_layout", "m1v_downscale_plane_layout_in_force",
    "m1v_downscale_planes_to_i420_device",
    "m1v_downscale_word_layout_preset", "m1v_set_downscale_word_layout", "m1v_downscale_word_layout_in_force",
    "m1v_downscale_words_to_i420_device",
    "m1v_set_frame_table", "m1v_frame_table", "m1v_set_plane_table", "m1v_plane_table",
    "m1v_delivery_create", "m1v_delivery_destroy", "m1v_delivery_step", "m1v_delivery_flush", "m1v_delivery_wait", "m1v_delivery_bytes",
]
DELIVERY_NONE = 2


ENCODER_H_SYMBOLS = ["mpeg_encode_procedure", "mpeg_encode_procedure_region", "encoder_set_image_loader",
                     "encoder_set_host_threads", "encoder_release_cache"]


class EncoderLibraryMissing(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EncoderLibraryMissing(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.m1v_device_count.restype = C.c_int
    L.m1v_last_error.restype = C.c_char_p
    L.m1v_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.m1v_create.restype = C.c_int
    L.m1v_destroy.argtypes = [vp]
    L.m1v_destroy.restype = None
    for name in ("m1v_strips", "m1v_mb_rows", "m1v_batch_limit"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = C.c_int
    for name in ("m1v_frame_bound", "m1v_frame_bytes_in"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = C.c_size_t
    L.m1v_file_prolog.argtypes = [_u8p]
    L.m1v_file_prolog.restype = C.c_size_t
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_encode_device.restype = C.c_int
    L.m1v_encode_quality_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_encode_quality_device.restype = C.c_int
    L.m1v_frame_sizes_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.m1v_frame_sizes_device.restype = C.c_int
    L.m1v_encode_budget_device.argtypes = [vp, vp, C.c_int, C.c_int, _u8p, C.c_int, C.c_uint64, vp, vp,
                                           vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_encode_budget_device.restype = C.c_int
    L.m1v_frame_size_table_device.argtypes = [vp, vp, C.c_int, _u8p, C.c_int, vp, vp, vp]
    L.m1v_frame_size_table_device.restype = C.c_int
    L.m1v_encode_batch_budget_device.argtypes = [vp, vp, C.c_int, C.c_int, _u8p, C.c_int, C.c_uint64, vp,
                                                 vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_encode_batch_budget_device.restype = C.c_int
    L.m1v_encode_cbr_device.argtypes = [vp, vp, C.c_int, C.c_int, _u8p, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp,
                                        vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_encode_cbr_device.restype = C.c_int
    L.m1v_frame_rd_table_device.argtypes = [vp, vp, C.c_int, _u8p, C.c_int, vp, vp, vp, vp]
    L.m1v_frame_rd_table_device.restype = C.c_int
    L.m1v_encode_rd_device.argtypes = [vp, vp, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_uint64, vp, vp,
                                       vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.m1v_encode_rd_device.restype = C.c_int
    L.m1v_encode_rd_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_uint64, vp,
                                             vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.m1v_encode_rd_batch_device.restype = C.c_int
    L.m1v_encode_rd_cbr_device.argtypes = [vp, vp, C.c_int, C.c_int, _u8p, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp,
                                           vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.m1v_encode_rd_cbr_device.restype = C.c_int
    L.m1v_rd_batch_pick_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, vp]
    L.m1v_rd_batch_pick_device.restype = C.c_int
    L.m1v_rd_cbr_pick_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp]
    L.m1v_rd_cbr_pick_device.restype = C.c_int
    L.m1v_encode_streams_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.m1v_encode_streams_device.restype = C.c_int
    L.m1v_encode_streams_cbr_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, _u8p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp,
                                                vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.m1v_encode_streams_cbr_device.restype = C.c_int
    L.m1v_streams_cbr_pick_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp,
                                              vp, vp, vp, vp, vp, vp]
    L.m1v_streams_cbr_pick_device.restype = C.c_int
    L.m1v_encode_streams_budget_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, _u8p, C.c_int, C.c_int, C.c_uint64, vp, vp,
                                                   vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.m1v_encode_streams_budget_device.restype = C.c_int
    L.m1v_streams_budget_pick_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp,
                                                 vp, vp, vp]
    L.m1v_streams_budget_pick_device.restype = C.c_int
    L.m1v_set_pipelined.argtypes = [vp, C.c_int]
    L.m1v_set_pipelined.restype = C.c_int
    L.m1v_flush.argtypes = [vp, vp]
    L.m1v_flush.restype = C.c_int
    L.m1v_alloc_host.argtypes = [C.c_size_t]
    L.m1v_alloc_host.restype = vp
    L.m1v_free_host.argtypes = [vp]
    L.m1v_free_host.restype = None
    L.m1v_warm_up.argtypes = [C.c_int]
    L.m1v_warm_up.restype = C.c_int
    L.m1v_encode_host.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
    L.m1v_encode_host.restype = C.c_long
    L.m1v_encode_planes_host.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    L.m1v_encode_planes_host.restype = C.c_long
    L.m1v_coefficients_device.argtypes = [vp, vp, C.c_int, vp, vp]
    L.m1v_coefficients_device.restype = C.c_int
    L.m1v_convert_device.argtypes = [vp, vp, C.c_int, vp, vp]
    L.m1v_convert_device.restype = C.c_int
    L.m1v_convert_host.argtypes = [vp, vp, C.c_int, vp]
    L.m1v_convert_host.restype = C.c_int
    L.m1v_subsample_device.argtypes = [vp, vp, vp, vp, vp, vp]
    L.m1v_subsample_device.restype = C.c_int
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_synth_device.restype = C.c_int
    L.m1v_profile_enable.argtypes = [vp, C.c_int]
    L.m1v_profile_enable.restype = C.c_int
    L.m1v_profile_read.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.m1v_profile_read.restype = C.c_int
    L.m1v_profile_read_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.m1v_profile_read_times.restype = C.c_int
    L.m1v_debug_set_input_mode.argtypes = [vp, C.c_int]
    L.m1v_debug_set_input_mode.restype = C.c_int
    L.m1v_reserve_scratch.argtypes = [vp, C.c_int]
    L.m1v_reserve_scratch.restype = C.c_int
    L.m1v_scratch_bytes.argtypes = [vp]
    L.m1v_scratch_bytes.restype = C.c_size_t
    L.m1v_debug_set_lds_words.argtypes = [vp, C.c_int]
    L.m1v_debug_set_lds_words.restype = C.c_int
    L.m1v_debug_set_dense_threads.argtypes = [vp, C.c_int]
    L.m1v_debug_set_dense_threads.restype = C.c_int
    L.m1v_debug_set_path.argtypes = [vp, C.c_int]
    L.m1v_debug_set_path.restype = C.c_int
    L.m1v_path_in_use.argtypes = [vp]
    L.m1v_path_in_use.restype = C.c_int
    L.m1v_debug_assemble_shape.argtypes = [vp, C.POINTER(C.c_int)]
    L.m1v_debug_assemble_shape.restype = C.c_int
    L.m1v_debug_set_assemble_shape.argtypes = [vp, C.c_int, C.c_int]
    L.m1v_debug_set_assemble_shape.restype = C.c_int
    L.m1v_size_table_fused.argtypes = [vp]
    L.m1v_size_table_fused.restype = C.c_int
    L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.m1v_set_input_layout.restype = C.c_int
    L.m1v_input_layout.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.m1v_input_layout.restype = C.c_int
    # per layout struct: its preset (the number of ints it takes in front of the struct), its setter and its getter
    for kind, struct, preset_ints in (("plane", PlaneLayout, 3), ("sample", SampleLayout, 3), ("rgb_plane", RgbPlaneLayout, 3),
                                      ("float_plane", FloatPlaneLayout, 5), ("float_pixel", FloatPixelLayout, 6),
                                      ("downscale", DownscaleLayout, 5), ("downscale_plane", DownscalePlaneLayout, 4),
                                      ("downscale_word", DownscaleWordLayout, 4)):
        getattr(L, f"m1v_{kind}_layout_preset").argtypes = [C.c_int] * preset_ints + [C.POINTER(struct)]
        getattr(L, f"m1v_set_{kind}_layout").argtypes = [vp, C.POINTER(struct)]
        getattr(L, f"m1v_{kind}_layout_in_force").argtypes = [vp, C.POINTER(struct)]
        for name in (f"m1v_{kind}_layout_preset", f"m1v_set_{kind}_layout", f"m1v_{kind}_layout_in_force"):
            getattr(L, name).restype = C.c_int
    for name in ("m1v_float_planes_to_bytes_device", "m1v_float_pixels_to_bytes_device", "m1v_downscale_to_bytes_device",
                 "m1v_downscale_planes_to_i420_device", "m1v_downscale_words_to_i420_device"):
        getattr(L, name).argtypes = [vp, vp, C.c_int, vp, vp]
        getattr(L, name).restype = C.c_int
    L.m1v_set_frame_table.argtypes = [vp, C.c_int]
    L.m1v_set_frame_table.restype = C.c_int
    L.m1v_frame_table.argtypes = [vp]
    L.m1v_frame_table.restype = C.c_int
    L.m1v_set_plane_table.argtypes = [vp, C.c_int]
    L.m1v_set_plane_table.restype = C.c_int
    L.m1v_plane_table.argtypes = [vp]
    L.m1v_plane_table.restype = C.c_int
    L.m1v_debug_fail_alloc.argtypes = [C.c_int]
    L.m1v_debug_fail_alloc.restype = None
    L.m1v_debug_fail_encode.argtypes = [C.c_int]
    L.m1v_debug_fail_encode.restype = None
    L.m1v_delivery_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.m1v_delivery_create.restype = C.c_int
    L.m1v_delivery_destroy.argtypes = [vp]
    L.m1v_delivery_destroy.restype = None
    L.m1v_delivery_step.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.m1v_delivery_step.restype = C.c_int
    L.m1v_delivery_flush.argtypes = [vp]
    L.m1v_delivery_flush.restype = C.c_int
    L.m1v_delivery_wait.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(vp)]
    L.m1v_delivery_wait.restype = C.c_int
    L.m1v_delivery_bytes.argtypes = [vp, C.c_int]
    L.m1v_delivery_bytes.restype = C.c_uint64
    L.mpeg_encode_procedure.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.mpeg_encode_procedure.restype = C.c_int
    L.mpeg_encode_procedure_region.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.mpeg_encode_procedure_region.restype = C.c_int
    L.encoder_set_image_loader.argtypes = [C.c_void_p, C.c_void_p]
    L.encoder_set_image_loader.restype = None
    _lib = L
    return L


def last_error():
    return lib().m1v_last_error().decode(errors="replace")
