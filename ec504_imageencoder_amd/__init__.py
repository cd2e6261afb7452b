"""MI355X-native MPEG-1 I-frame encode path (drop-in for ec504_ImageEncoder's hot path).

Product code lives in csrc/ (HIP kernels + C host driver, built into libencoder.so); this package
is the thin host-side mirror used by tests and bench.py.
"""
from . import _ffi  # noqa: F401
from .encoder import (EncoderError, FrameTable, Mpeg1Encoder, distortion_to_psnr, downscale_layout_preset, downscale_plane_layout_preset, downscale_strides, downscale_word_layout_preset, file_prolog, float_pixel_layout_preset, float_pixel_strides,  # noqa: F401
                      float_plane_layout_preset,
                      float_plane_strides, mpeg_encode_procedure,
                      plane_layout_preset, psnr_to_distortion, rgb_plane_layout_preset, rgb_plane_strides, sample_layout_preset,
                      set_image_loader, surface_strides, StreamSpans, stream_spans)
