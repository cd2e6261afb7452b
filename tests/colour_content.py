"""Content for the colour conversion inside the encode kernels: frames of flat cells, one colour per cell, and the colours that
fp64 rounding decides (the ties).  The parity, surface and rgb plane tests send the same colours through their kernels."""
import functools

import numpy as np


# The encode kernels convert pixels themselves (fp32 fast path + fp64 re-evaluation of ties), with code of their own per
# input mode.  Pictures of FLAT 8x8 cells at quality 50 pin every converted value: the DC divisor is 8, a flat block of
# value v has DC 8v + 2, so its level is exactly v and a conversion that is off by one changes the stream.  Cell (r, c)
# repeats with period W/2 across and H/4 down, which makes the chroma blocks flat too: the chroma block of macroblock
# (strip s, row mb) is cut from picture rows 4mb..4mb+3, columns [8s, 8s+8) and [W/2+8s, W/2+8s+8) (encoder.h:347-348),
# and every colour of a picture lies in its top quarter as well, so each one is coded as Y, as Cb and as Cr.
_CW, _CH = 2048, 1024
_COLOURS_PER_FRAME = (_CW // 16) * (_CH // 32)


def _flat_cell_frames(colours, channels=3, alpha_seed=1):
    """colours: uint8 [n, 3] -> frames uint8 [ceil(n / 4096), H, W, channels] (the last frame padded with colour 0)."""
    per = _COLOURS_PER_FRAME
    nf = (len(colours) + per - 1) // per
    pad = np.zeros((nf * per, 3), np.uint8)
    pad[:len(colours)] = colours
    cells = pad.reshape(nf, _CH // 32, _CW // 16, 3)
    cells = np.tile(cells, (1, 4, 2, 1))                                   # period H/4 down, W/2 across
    frames = np.repeat(np.repeat(cells, 8, 1), 8, 2)
    if channels == 4:
        alpha = np.random.default_rng(alpha_seed).integers(0, 256, frames.shape[:3] + (1,), dtype=np.uint8)
        frames = np.concatenate([frames, alpha], -1)
    return np.ascontiguousarray(frames)


@functools.lru_cache(maxsize=1)
def _tie_colours():
    """Every (r, g, b) for which at least one of the three formulas is an exact integer or closer than 5e-4 above one:
    the inputs whose bytes fp64 rounding decides in the reference, and all that take the kernels' fp64 branch."""
    v = np.arange(1 << 24, dtype=np.int64)
    r, g, b = v >> 16, (v >> 8) & 255, v & 255
    y = (299000 * r + 587000 * g + 114000 * b) % 1000000
    cb = (128000000 - 168736 * r - 331264 * g + 500000 * b) % 1000000
    cr = (128000000 + 500000 * r - 418688 * g - 81312 * b) % 1000000
    sel = (y < 500) | (cb < 500) | (cr < 500)
    return np.stack([r[sel], g[sel], b[sel]], -1).astype(np.uint8)
