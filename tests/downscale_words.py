"""The downscale word layout's model and inputs for its tests (no tests here): down2_words, the numpy statement of the definition
in include/mpeg1_hip.h ("Downscale word layout"); sources of noise per preset, sources that repeat each sample of a picture's
planes 2 x 2 as the word `byte << shift` with noise in the bits below the shift, so that the model returns the planes exactly (how
content defined in rendition samples reaches the back half of the kernels), and sources whose every cell holds four given words;
and place(), which puts a source into a device buffer of noise with row padding, gaps between planes and frames, a surrounding
surface and an odd base offset, and returns the [n, L] view and its layout.  A source is the triple (Y [n, 2H, 2W], Cb [n, H, W],
Cr [n, H, W]) of uint16 words of a W x H rendition, whatever form it is stored in."""
import numpy as np

PRESETS = ("p010", "p012", "p016", "i010", "i012", "i016")      # the names Mpeg1Encoder.set_downscale_word_layout takes
SHIFT = {"p010": 8, "p012": 8, "p016": 8, "i010": 2, "i012": 4, "i016": 8}
CSTEP = {"p010": 4, "p012": 4, "p016": 4, "i010": 2, "i012": 2, "i016": 2}
# the words a decoder writes: (bits of the value, bits below it that are zero)
DEPTH = {"p010": (10, 6), "p012": (12, 4), "p016": (16, 0), "i010": (10, 0), "i012": (12, 0), "i016": (16, 0)}
GUARD = 64          # bytes of the allocation in front of and behind every batch
# where a source lies: tight; a pitched window with padded rows whose pitches are no multiple of 4, gaps between planes and
# frames, a surrounding surface, and a base at an odd byte of the allocation
TIGHT = dict()
PITCHED = dict(pad=13, cpad=7, plane_gap=3, gap=5, window=(6, 2), margin=(2, 4), base=1)


def box(s, shift):
    """min(((the 2 x 2 sum of uint16 planes [..., 2h, 2w]) + 2 >> 2) >> shift, 255) as uint8: the average rounds half up at the
    word's precision, the shift truncates."""
    s = np.asarray(s)
    assert s.dtype == np.uint16 and s.shape[-2] % 2 == 0 and s.shape[-1] % 2 == 0 and 0 <= shift <= 8
    s = s.astype(np.uint32)
    a = (s[..., 0::2, 0::2] + s[..., 0::2, 1::2] + s[..., 1::2, 0::2] + s[..., 1::2, 1::2] + 2) >> 2
    return np.minimum(a >> shift, 255).astype(np.uint8)


def down2_words(planes, shift):
    """The definition on a source triple of uint16 planes: the tightly packed I420 frames [n, W * H * 3 / 2] of the rendition."""
    Y, Cb, Cr = (box(p, shift) for p in planes)
    n = Y.shape[0]
    return np.ascontiguousarray(np.concatenate([Y.reshape(n, -1), Cb.reshape(n, -1), Cr.reshape(n, -1)], 1))


def words_at(frame_bytes, at):
    """The little-endian words at byte offsets `at` of a flat uint8 array."""
    frame = np.asarray(frame_bytes, dtype=np.uint8).reshape(-1)
    return (frame[at].astype(np.uint16) | frame[at + 1].astype(np.uint16) << 8).astype(np.uint16)


def down2_frame(frame_bytes, layout, W, H):
    """The definition on one frame: frame_bytes is a flat uint8 array from the frame's base, layout a dict with the source's
    y_offset, cb_offset, cr_offset, y_pitch, c_pitch, c_step (no zeros) and shift.  Returns the tightly packed I420 frame."""
    Y = words_at(frame_bytes, layout["y_offset"] + np.arange(2 * H)[:, None] * layout["y_pitch"] + 2 * np.arange(2 * W)[None, :])
    at = np.arange(H)[:, None] * layout["c_pitch"] + np.arange(W)[None, :] * layout["c_step"]
    Cb, Cr = words_at(frame_bytes, layout["cb_offset"] + at), words_at(frame_bytes, layout["cr_offset"] + at)
    return down2_words((Y[None], Cb[None], Cr[None]), layout["shift"])[0]


def noise_source(seed, n, H, W, preset, over=False):
    """A source of uniform noise for a W x H rendition in the words a decoder writes for `preset`: the value's bits are noise, the
    bits below a high-aligned value are zero.  over: every bit of every word is noise (a high-aligned word's low bits, a
    low-aligned word's bits above the stated depth, which the definition clamps)."""
    rng = np.random.default_rng(seed)
    bits, low = DEPTH[preset]
    draw = (lambda shape: rng.integers(0, 1 << 16, shape, dtype=np.uint16)) if over else \
        (lambda shape: (rng.integers(0, 1 << bits, shape, dtype=np.uint16) << low).astype(np.uint16))
    out = tuple(draw(shape) for shape in ((n, 2 * H, 2 * W), (n, H, W), (n, H, W)))
    for p in out:
        p.setflags(write=False)
    return out


def at_the_boundary(planes, shift, seed):
    """planes with every other cell (a noise choice, about half of them) rewritten so that its four-sum is 4 * (s << shift) - 1 or
    - 2 for a noise sample s of 1 .. 255: rounded half up the average is s << shift and the sample s, truncated the average is
    (s << shift) - 1 and the sample s - 1.  On plain noise a missing `+ 2` moves a sample once in 2 << shift cells, at shift 8 not
    once in a macroblock; here it moves about every other one.  The four words of such a cell are noise around s << shift."""
    rng = np.random.default_rng(9000 + seed)
    out = []
    for p in planes:
        n, h, w = p.shape[0], p.shape[1] // 2, p.shape[2] // 2
        b = rng.integers(1, 256, (n, h, w)).astype(np.int64) << shift
        m = np.minimum(np.maximum(np.minimum(b - 2, 65535 - b) // 3, 0), 3 << shift)
        d = [np.rint((rng.random((n, h, w)) * 2 - 1) * m).astype(np.int64) for _ in range(3)]
        last = b - rng.integers(1, 3, (n, h, w)) - (d[0] + d[1] + d[2])
        words = [b + d[0], b + d[1], b + d[2], last]
        assert all(((0 <= v) & (v <= 65535)).all() for v in words)
        take = rng.random((n, h, w)) < 0.5
        q = np.array(p, dtype=np.uint16)
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            # (which corner gets which word varies with the cell)
            pick = np.choose((np.arange(h * w).reshape(h, w) + k) % 4, words)
            q[:, dy::2, dx::2] = np.where(take, pick, q[:, dy::2, dx::2]).astype(np.uint16)
        q.setflags(write=False)
        out.append(q)
    return tuple(out)


def noise_for(W, H, preset, n=9):
    """The noise source of a size and preset that the GPU arithmetic test and the CPU census share: a decoder's words for the
    low-aligned presets, noise in every bit (the low bits included) for the presets whose shift is 8, and about every other cell
    at a sample's boundary (at_the_boundary).  The frames depend on n: the census takes frame 0 of the default nine."""
    seed = W * 100 + H + 7 * PRESETS.index(preset)
    return at_the_boundary(noise_source(seed, n, H, W, preset, over=SHIFT[preset] == 8), SHIFT[preset], seed)


def above_depth_source(preset, n, H, W, seed=11):
    """Words of a low-aligned preset around the top of its depth: noise of the top two sample values of the depth and of the
    first values above it, so that averages fall on both sides of the clamp."""
    top, span = 1 << DEPTH[preset][0], 2 << SHIFT[preset]
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(top - span, top + span, shape).astype(np.uint16) for shape in ((n, 2 * H, 2 * W), (n, H, W), (n, H, W)))


def pack(source, preset):
    """The tightly packed frames [n, 6 W H] of uint16 words of a source triple in the form `preset`."""
    Y, Cb, Cr = source
    n = Y.shape[0]
    if CSTEP[preset] == 2:
        chroma = [Cb.reshape(n, -1), Cr.reshape(n, -1)]
    else:
        chroma = [np.stack([Cb, Cr], -1).reshape(n, -1)]
    return np.ascontiguousarray(np.concatenate([Y.reshape(n, -1)] + chroma, 1))


def replicated_planes(y, cb, cr, shift, seed=0):
    """The source triple whose every 2 x 2 cell repeats the word `sample << shift | noise below the shift` of the planes y
    [n, H, W], cb, cr [n, H/2, W/2] of uint8: the average of four equal words is the word and the shift drops the noise, so the
    model of it is the planes."""
    rng = np.random.default_rng(7000 + seed)

    def rep(p):
        p = np.asarray(p, dtype=np.uint8)
        word = (p.astype(np.uint16) << shift | rng.integers(0, 1 << shift, p.shape, dtype=np.uint16)).astype(np.uint16)
        return np.ascontiguousarray(np.repeat(np.repeat(word, 2, axis=-2), 2, axis=-1))

    return rep(y), rep(cb), rep(cr)


def replicated_source(y, cb, cr, preset, seed=0):
    """replicated_planes as tightly packed frames of words of the form `preset`."""
    return pack(replicated_planes(y, cb, cr, SHIFT[preset], seed), preset)


def cell_source(y_cell, cb_cell, cr_cell, n, H, W):
    """A source triple whose every cell of a plane holds that plane's four words (upper left, upper right, lower left, lower right)."""
    tile = lambda cell, h, w: np.ascontiguousarray(np.broadcast_to(np.tile(np.asarray(cell, dtype=np.uint16).reshape(2, 2), (h, w)), (n, 2 * h, 2 * w)))
    return tile(y_cell, H, W), tile(cb_cell, H // 2, W // 2), tile(cr_cell, H // 2, W // 2)


def geometry(W, H, preset, pad=0, cpad=0, plane_gap=0, gap=0, window=(0, 0), margin=(0, 0), base=0, shared=False, cr_first=False):
    """(layout of the source as set_downscale_word_layout takes it with no zeros but the shift, bytes a frame's surface spans,
    offset of frame 0's base in the allocation) of 2W x 2H sources that start at luma word `window` = (x0, y0) of surfaces with
    `margin` = (words to the right, rows below), all four even; luma rows padded by `pad` and chroma rows by `cpad` bytes,
    `plane_gap` bytes between planes, frames `gap` bytes apart, the base `base` bytes behind the guard.  cr_first: Cr in front of
    Cb.  shared: one chroma plane with c_step 4 whose every other word belongs to nobody, named by both offsets — the one way in
    which c_step = 4 planes are not interleaved with each other while their offsets lie within one 4-byte group (a source of it
    has Cb == Cr)."""
    (x0, y0), (right, below) = window, margin
    assert not (x0 | y0 | right | below) & 1
    SW, SH = x0 + 2 * W + right, y0 + 2 * H + below
    planar = CSTEP[preset] == 2 and not shared
    c_step = 2 if planar else 4
    y_pitch, c_pitch = 2 * SW + pad, (SW // 2) * c_step + cpad
    first = SH * y_pitch + plane_gap
    if planar:
        second = first + (SH // 2) * c_pitch + plane_gap
        total = second + (SH // 2) * c_pitch
    else:
        second, total = first + (0 if shared else 2), first + (SH // 2) * c_pitch
    cb, cr = (second, first) if cr_first else (first, second)
    inside = (y0 // 2) * c_pitch + (x0 // 2) * c_step
    lay = dict(y_offset=y0 * y_pitch + 2 * x0, cb_offset=cb + inside, cr_offset=cr + inside, y_pitch=y_pitch, c_pitch=c_pitch, c_step=c_step,
               frame_stride=total + gap, factor=2, shift=SHIFT[preset])
    return lay, total, GUARD + base


def addressed(lay, n, W, H, at, total):
    """bool [total]: the bytes of an allocation that the definition addresses for n frames whose first base lies at `at`."""
    mask = np.zeros(total, bool)
    for f in range(n):
        F = at + f * lay["frame_stride"]
        y = F + lay["y_offset"] + np.arange(2 * H)[:, None] * lay["y_pitch"] + 2 * np.arange(2 * W)[None, :]
        c = np.arange(H)[:, None] * lay["c_pitch"] + np.arange(W)[None, :] * lay["c_step"]
        for first in (y, F + lay["cb_offset"] + c, F + lay["cr_offset"] + c):
            mask[first] = True
            mask[first + 1] = True
    return mask


def host_buffer(source, preset, fill_seed=0, **where):
    """The allocation as a numpy array of noise bytes (seed fill_seed) with the source's words written where the layout addresses
    them; row padding, gaps, the surface around the window, the other words of a shared plane and the guards keep the noise.
    Returns (host, layout, offset of frame 0's base, bytes of a frame's row of the [n, L] view)."""
    Y, Cb, Cr = source
    n, H, W = Cb.shape
    lay, span, at = geometry(W, H, preset, **where)
    assert lay["cb_offset"] != lay["cr_offset"] or np.array_equal(Cb, Cr)
    stride = lay["frame_stride"]
    host = np.random.default_rng(1000 + fill_seed).integers(0, 256, at + n * stride + GUARD, dtype=np.uint8)
    as_strided = np.lib.stride_tricks.as_strided
    for plane, off, shape, pitch, step in ((Y, lay["y_offset"], (n, 2 * H, 2 * W), lay["y_pitch"], 2),
                                           (Cb, lay["cb_offset"], (n, H, W), lay["c_pitch"], lay["c_step"]),
                                           (Cr, lay["cr_offset"], (n, H, W), lay["c_pitch"], lay["c_step"])):
        as_strided(host[at + off:], shape, (stride, pitch, step))[...] = plane & 0xff
        as_strided(host[at + off + 1:], shape, (stride, pitch, step))[...] = plane >> 8
    return host, lay, at, span


def place(torch, source, preset, fill_seed=0, **where):
    """source on the device: (the uint8 view [n, L] the encoder takes, rows frame_stride apart, its layout as
    set_downscale_word_layout takes it, the whole buffer).  Every batch lies GUARD bytes inside its allocation."""
    host, lay, at, span = host_buffer(source, preset, fill_seed, **where)
    n = source[0].shape[0]
    buf = torch.from_numpy(host).cuda()
    return torch.as_strided(buf, (n, span), (lay["frame_stride"], 1), at), lay, buf
