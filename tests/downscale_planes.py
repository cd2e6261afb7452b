"""The downscale plane layout's model and inputs for its tests (no tests here): down2_planes, the numpy statement of the
definition in include/mpeg1_hip.h ("Downscale plane layout"); sources of noise, sources that repeat each sample of a picture's
planes 2 x 2, so that the model returns the planes exactly (how content defined in rendition samples reaches the back half of the
kernels), and sources whose every cell holds four given values; and place(), which puts a source into a device buffer of noise
with row padding, gaps between planes and frames, a surrounding surface and an odd base offset, and returns the [n, L] view and
its layout.  A source is the triple (Y [n, 2H, 2W], Cb [n, H, W], Cr [n, H, W]) of a W x H rendition, whatever form it is stored in."""
import numpy as np

PRESETS = ("i420", "yv12", "nv12", "nv21")
CSTEP = {"i420": 1, "yv12": 1, "nv12": 2, "nv21": 2}
GUARD = 64          # bytes of the allocation in front of and behind every batch
# where a source lies: tight; a pitched window with padded rows whose pitches are no multiple of 4, gaps between planes and
# frames, a surrounding surface, and a base at an odd byte of the allocation
TIGHT = dict()
PITCHED = dict(pad=13, cpad=7, plane_gap=3, gap=5, window=(6, 2), margin=(2, 4), shift=1)


def box(s):
    """The 2 x 2 box average of uint8 planes [..., 2h, 2w], rounding half up: widen, add the four strided views, + 2, >> 2."""
    s = np.asarray(s)
    assert s.dtype == np.uint8 and s.shape[-2] % 2 == 0 and s.shape[-1] % 2 == 0
    s = s.astype(np.uint16)
    return ((s[..., 0::2, 0::2] + s[..., 0::2, 1::2] + s[..., 1::2, 0::2] + s[..., 1::2, 1::2] + 2) >> 2).astype(np.uint8)


def down2_planes(frame_bytes, layout, W, H):
    """The definition on one frame: frame_bytes is a flat uint8 array from the frame's base, layout a dict with the source's
    y_offset, cb_offset, cr_offset, y_pitch, c_pitch, c_step (no zeros).  Returns (Y [H, W], Cb [H/2, W/2], Cr [H/2, W/2], their
    tightly packed I420 frame [W * H * 3 / 2])."""
    frame = np.asarray(frame_bytes, dtype=np.uint8).reshape(-1)
    Y = box(frame[layout["y_offset"] + np.arange(2 * H)[:, None] * layout["y_pitch"] + np.arange(2 * W)[None, :]])
    at = np.arange(H)[:, None] * layout["c_pitch"] + np.arange(W)[None, :] * layout["c_step"]
    Cb, Cr = box(frame[layout["cb_offset"] + at]), box(frame[layout["cr_offset"] + at])
    return Y, Cb, Cr, np.concatenate([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)])


def model_frames(source):
    """The tightly packed I420 frames [n, W * H * 3 / 2] of the rendition of a source triple."""
    Y, Cb, Cr = (box(p) for p in source)
    n = Y.shape[0]
    return np.ascontiguousarray(np.concatenate([Y.reshape(n, -1), Cb.reshape(n, -1), Cr.reshape(n, -1)], 1))


def noise_source(seed, n, H, W):
    """A source of uniform noise for a W x H rendition, the same samples whatever preset stores them."""
    rng = np.random.default_rng(seed)
    out = tuple(rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((n, 2 * H, 2 * W), (n, H, W), (n, H, W)))
    for p in out:
        p.setflags(write=False)
    return out


def pack(source, preset):
    """The tightly packed frames [n, 6 W H] of a source triple in the form `preset`."""
    Y, Cb, Cr = source
    n = Y.shape[0]
    first, second = (Cr, Cb) if preset in ("yv12", "nv21") else (Cb, Cr)
    if CSTEP[preset] == 1:
        chroma = [first.reshape(n, -1), second.reshape(n, -1)]
    else:
        chroma = [np.stack([first, second], -1).reshape(n, -1)]
    return np.ascontiguousarray(np.concatenate([Y.reshape(n, -1)] + chroma, 1))


def replicated_planes(y, cb, cr):
    """The source triple whose every 2 x 2 cell repeats the sample of the planes y [n, H, W], cb, cr [n, H/2, W/2]: the model of it
    is the planes."""
    rep = lambda p: np.ascontiguousarray(np.repeat(np.repeat(np.asarray(p, dtype=np.uint8), 2, axis=-2), 2, axis=-1))
    return rep(y), rep(cb), rep(cr)


def replicated_source(y, cb, cr, preset):
    """replicated_planes as tightly packed frames of the form `preset`."""
    return pack(replicated_planes(y, cb, cr), preset)


def cell_source(y_cell, cb_cell, cr_cell, n, H, W):
    """A source triple whose every cell of a plane holds that plane's four values (upper left, upper right, lower left, lower right)."""
    tile = lambda cell, h, w: np.ascontiguousarray(np.broadcast_to(np.tile(np.asarray(cell, dtype=np.uint8).reshape(2, 2), (h, w)), (n, 2 * h, 2 * w)))
    return tile(y_cell, H, W), tile(cb_cell, H // 2, W // 2), tile(cr_cell, H // 2, W // 2)


def geometry(W, H, preset, pad=0, cpad=0, plane_gap=0, gap=0, window=(0, 0), margin=(0, 0), shift=0, spread=False):
    """(layout of the source as set_downscale_plane_layout takes it with no zeros, bytes a frame's surface spans, offset of frame
    0's base in the allocation) of 2W x 2H sources that start at luma sample `window` = (x0, y0) of surfaces with `margin` =
    (samples to the right, rows below), all four even; luma rows padded by `pad` and chroma rows by `cpad` bytes, `plane_gap`
    bytes between planes, frames `gap` bytes apart, the base `shift` bytes behind the guard.  spread: the planar presets with
    c_step 2 — each component in a plane of its own whose every other byte belongs to nobody."""
    (x0, y0), (right, below) = window, margin
    assert not (x0 | y0 | right | below) & 1
    SW, SH = x0 + 2 * W + right, y0 + 2 * H + below
    planar = CSTEP[preset] == 1
    c_step = 2 if spread or not planar else 1
    y_pitch, c_pitch = SW + pad, (SW // 2) * c_step + cpad
    first = SH * y_pitch + plane_gap
    if planar:
        second = first + (SH // 2) * c_pitch + plane_gap
        total = second + (SH // 2) * c_pitch
    else:
        second, total = first + 1, first + (SH // 2) * c_pitch
    cb, cr = (second, first) if preset in ("yv12", "nv21") else (first, second)
    inside = (y0 // 2) * c_pitch + (x0 // 2) * c_step
    lay = dict(y_offset=y0 * y_pitch + x0, cb_offset=cb + inside, cr_offset=cr + inside, y_pitch=y_pitch, c_pitch=c_pitch, c_step=c_step,
               frame_stride=total + gap, factor=2, reserved=0)
    return lay, total, GUARD + shift


def addressed(lay, n, W, H, at, total):
    """bool [total]: the bytes of an allocation that the definition addresses for n frames whose first base lies at `at`."""
    mask = np.zeros(total, bool)
    for f in range(n):
        F = at + f * lay["frame_stride"]
        mask[F + lay["y_offset"] + np.arange(2 * H)[:, None] * lay["y_pitch"] + np.arange(2 * W)[None, :]] = True
        c = np.arange(H)[:, None] * lay["c_pitch"] + np.arange(W)[None, :] * lay["c_step"]
        mask[F + lay["cb_offset"] + c] = True
        mask[F + lay["cr_offset"] + c] = True
    return mask


def host_buffer(source, preset, fill_seed=0, **where):
    """The allocation as a numpy array of noise (seed fill_seed) with the source's samples written where the layout addresses
    them; row padding, gaps, the surface around the window, the other bytes of a spread plane and the guards keep the noise.
    Returns (host, layout, offset of frame 0's base, bytes of a frame's row of the [n, L] view)."""
    Y, Cb, Cr = source
    n, H, W = Cb.shape
    lay, span, at = geometry(W, H, preset, **where)
    stride = lay["frame_stride"]
    host = np.random.default_rng(1000 + fill_seed).integers(0, 256, at + n * stride + GUARD, dtype=np.uint8)
    as_strided = np.lib.stride_tricks.as_strided
    as_strided(host[at + lay["y_offset"]:], (n, 2 * H, 2 * W), (stride, lay["y_pitch"], 1))[...] = Y
    as_strided(host[at + lay["cb_offset"]:], (n, H, W), (stride, lay["c_pitch"], lay["c_step"]))[...] = Cb
    as_strided(host[at + lay["cr_offset"]:], (n, H, W), (stride, lay["c_pitch"], lay["c_step"]))[...] = Cr
    return host, lay, at, span


def place(torch, source, preset, fill_seed=0, **where):
    """source on the device: (the uint8 view [n, L] the encoder takes, rows frame_stride apart, its layout as
    set_downscale_plane_layout takes it, the whole buffer).  Every batch lies GUARD bytes inside its allocation."""
    host, lay, at, span = host_buffer(source, preset, fill_seed, **where)
    n = source[0].shape[0]
    buf = torch.from_numpy(host).cuda()
    return torch.as_strided(buf, (n, span), (lay["frame_stride"], 1), at), lay, buf
