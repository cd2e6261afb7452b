"""The downscale layout's model and inputs for its tests (no tests here): down2, the numpy statement of the definition in
include/mpeg1_hip.h ("Downscale layout"); sources of noise and sources that repeat each pixel of a picture 2 x 2, so that down2
returns the picture exactly (how content defined in rendition pixels reaches the back half of the kernels); and place(), which
puts a source into a device buffer of noise with row padding, a gap between frames and a surrounding surface, and returns the
strided view and its layout."""
import numpy as np

ORDERS = ("rgb", "bgr")
WIDTHS = (3, 4)     # bytes per source pixel
GUARD = 64          # bytes of the allocation in front of and behind every batch


def down2(src, order="rgb"):
    """The picture the encoder codes for the source src, uint8 [n, 2H, 2W, C >= 3] with a pixel's bytes in memory order:
    uint8 [n, H, W, 3] in R, G, B order.  Widen, add the four strided views, + 2, >> 2; the order applied, a 4th byte dropped."""
    s = np.asarray(src)
    assert s.dtype == np.uint8 and s.ndim == 4 and s.shape[1] % 2 == 0 and s.shape[2] % 2 == 0 and s.shape[3] >= 3
    s = s.astype(np.uint16)
    out = ((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2)[..., :3]
    if order == "bgr":
        out = out[..., ::-1]
    else:
        assert order == "rgb"
    return np.ascontiguousarray(out.astype(np.uint8))


def noise_source(seed, n, H, W, C=3):
    """n source frames of uniform noise for a W x H rendition: uint8 [n, 2H, 2W, C]."""
    return np.random.default_rng(seed).integers(0, 256, (n, 2 * H, 2 * W, C), dtype=np.uint8)


def replicated_source(px, order="rgb"):
    """The source [n, 2H, 2W, 3] (bytes in memory order) whose every 2 x 2 cell repeats the pixel of the picture px [n, H, W, 3]
    (R, G, B): down2 of it is px."""
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim == 4 and px.shape[3] == 3
    mem = px[..., ::-1] if order == "bgr" else px
    return np.ascontiguousarray(np.repeat(np.repeat(mem, 2, axis=1), 2, axis=2))


def cell_source(values, n, H, W, C=3):
    """A source whose every cell holds the four `values` (upper left, upper right, lower left, lower right) in every colour."""
    cell = np.asarray(values, dtype=np.uint8).reshape(2, 2)
    return np.ascontiguousarray(np.broadcast_to(np.tile(cell, (H, W))[None, :, :, None], (n, 2 * H, 2 * W, C)))


def geometry(n, H2, W2, P, pad=0, gap=0, window=(0, 0), margin=(0, 0)):
    """(row_pitch, frame_stride, offset of source pixel (0, 0) of frame 0, bytes of the allocation) of a batch of n H2 x W2 sources
    of P-byte pixels that start at pixel `window` = (x0, y0) of surfaces with `margin` = (pixels to the right, rows below), rows
    padded by `pad` bytes and frames `gap` bytes apart."""
    (x0, y0), (right, below) = window, margin
    pitch = (x0 + W2 + right) * P + pad
    frame = (y0 + H2 + below) * pitch + gap
    return pitch, frame, GUARD + y0 * pitch + x0 * P, GUARD + n * frame + GUARD


def host_buffer(src, P, fill_seed=0, **where):
    """The allocation as a numpy array of noise (seed fill_seed) with the colour bytes src[..., :3] written where the layout
    addresses them; row padding, gaps, the surface around the window, 4th bytes and the guards keep the noise."""
    n, H2, W2, _ = src.shape
    pitch, frame, at, total = geometry(n, H2, W2, P, **where)
    host = np.random.default_rng(1000 + fill_seed).integers(0, 256, total, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(host[at:], (n, H2, W2, 3), (frame, pitch, P, 1))
    view[...] = src[..., :3]
    return host, (pitch, frame, at)


def place(torch, src, P, order="rgb", fill_seed=0, **where):
    """src on the device: (the strided uint8 view [n, 2H, 2W, P] the encoder takes, its layout as set_downscale_layout takes it,
    the whole buffer)."""
    from ec504_imageencoder_amd import downscale_strides
    n, H2, W2, _ = src.shape
    host, (pitch, frame, at) = host_buffer(src, P, fill_seed, **where)
    buf = torch.from_numpy(host).cuda()
    x = torch.as_strided(buf, (n, H2, W2, P), (frame, pitch, P, 1), at)
    lay = downscale_strides(tuple(x.shape), tuple(x.stride()), "nhwc", order)
    if n == 1:
        lay["frame_stride"] = max(lay["frame_stride"], frame)
    return x, lay, buf
