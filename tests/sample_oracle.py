"""The checker for sample layouts (m1v_set_sample_layout): tests/plane_oracle.py's frame walk fed by samplers that step through
the luma row with y_step as well — TEST INFRASTRUCTURE ONLY.  The definition of include/mpeg1_hip.h, restated in numpy:
    luma block at (x, y), row i, sample j        frame[y_offset + (y + i) * y_pitch + (x + j) * y_step]
    chroma plane p of the macroblock at (x, y)   frame[p_offset + (y / 2 + i) * c_pitch + (x / 2 + j) * c_step]
tests/test_sample_layout_abi.py pins it to plane_oracle.layout_samplers for y_step = 1.
"""
import numpy as np

import plane_oracle
from plane_oracle import Unencodable  # noqa: F401


def layout_samplers(frame, layout):
    """(luma_block, chroma_block) that read one frame's bytes (a flat uint8 array starting at the frame's base) through a sample
    layout: a dict with y_offset, cb_offset, cr_offset, y_pitch, c_pitch, y_step, c_step, no zeros."""
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    rows = np.arange(8)[:, None]
    cols = np.arange(8)[None, :]
    y_off, y_pitch, y_step = layout["y_offset"], layout["y_pitch"], layout["y_step"]
    c_off, c_pitch, c_step = (layout["cb_offset"], layout["cr_offset"]), layout["c_pitch"], layout["c_step"]

    def luma_block(x, y):
        return frame[y_off + (y + rows) * y_pitch + (x + cols) * y_step]

    def chroma_block(p, x, y):
        return frame[c_off[p] + (y // 2 + rows) * c_pitch + (x // 2 + cols) * c_step]

    return luma_block, chroma_block


def encode_layout(frame, layout, W, H, frame_index, qf, mode):
    """plane_oracle.encode_frame over layout_samplers(frame, layout)."""
    luma_block, chroma_block = layout_samplers(frame, layout)
    return plane_oracle.encode_frame(luma_block, chroma_block, W, H, frame_index, qf, mode)


def addressed_mask(layout, xe, ye, length):
    """A boolean array of `length` bytes from a frame's base: True where the definition addresses a sample of the xe x ye region."""
    mask = np.zeros(length, bool)
    r, c = np.arange(ye)[:, None], np.arange(xe)[None, :]
    mask[(layout["y_offset"] + r * layout["y_pitch"] + c * layout["y_step"]).reshape(-1)] = True
    r, c = np.arange(ye // 2)[:, None], np.arange(xe // 2)[None, :]
    for off in (layout["cb_offset"], layout["cr_offset"]):
        mask[(off + r * layout["c_pitch"] + c * layout["c_step"]).reshape(-1)] = True
    return mask
