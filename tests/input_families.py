"""One builder of encoder inputs for the three sweeps (tests/test_gpu_geometry.py, tests/test_gpu_code_space.py,
tests/test_gpu_hard_content.py) — TEST INFRASTRUCTURE ONLY (no tests in this module; tests/test_input_families_cpu.py pins its
host side and that the families reach every tile-shaped kernel of the registry).

build(torch, family, W, H, mode, quality, max_frames, ...) takes content in one of two forms, packed pixels [n, H, W, 3 | 4] or
independent planes Y [n, ye, xe], Cb, Cr [n, ye / 2, xe / 2] of the coded region, and returns an Input: the encoder with the
layout (and the table mode) in force, the device object its calls take, `kind` ("rgb", "rgba", "planes": which oracle record
applies) and `kernels`, the source names of the registry entries the family launches.  Everything that is not an addressed
sample is noise of fill_seed: row padding, gaps between frames, a fourth plane, the low bytes of P010, the chroma of odd picture
rows in packed 4:2:2, picture columns and rows beyond the coded region of plane-form content, the guards around allocations.

  family                     content         layout                                                          kernels
  rgb, rgb-fallback          pixels 3        packed (rgb-fallback: 8-word LDS image, worst-case arena)        k_*_tiles
  rgb-runs                   pixels 3        packed, forced to the run kernels                                k_encode_dense, _strips
  rgba                       pixels 4        packed                                                           k_encode_dense, _strips, k_*_table_rgba
  surface-<c>-<order>-<l>    pixels c        tests/test_gpu_surface.py's surface l                            k_*_surface
  planes-<l>                 either          tests/test_gpu_planes.py's layout l (pixels: their converted     k_*_planes
                                             planes, the oracle's RGB records)
  rgbplanes-pitched, -bgr    pixels 3        uint8 NCHW: row pitch W + 13; tight in plane order B, G, R       k_*_rgb_planes
  float16-, bfloat16-,       pixels 3        the window of tests/test_gpu_float_planes.py (odd x0, odd        k_*_float_planes
  float32-window                             pitch, a fourth plane) of patterns whose byte under the rule
                                             of include/mpeg1_hip.h is the pixel (float_bits)
  yuy2, uyvy, p010           planes          the tight sample presets                                         k_*_step2
  kt-<family>                the family's    the family's frames scattered in a pool, named by a frame table  kt_* of the family's
  kp-planes-<preset>,        the family's    every plane at an address of its own behind a plane table; a     kp_*_planes,
  kp-rgbplanes-pitched                       plane's block is exactly its read-contract range                 kp_*_rgb_planes
"""
import numpy as np

import float_planes as fp
import geometry_space as gs
from layout_inputs import (RESIDUES, SEPARATE, _addressed, _addresses, _blocks, _buffer, _device_table, _layout, _planar,
                           _plane_encoder, _Rgb, _RgbPlanes, _sample_view, _Samples, _surface, _Surface, _surface_encoder,
                           _surface_geometry, _view, _write_planes, _Ycc)
from layout_inputs import _float_planes_tensor as _tensor
from layout_inputs import _noise as _sample_noise
from layout_inputs import _scatter as _sample_scatter

GUARD = 64
SAMPLE_PRESETS = ("yuy2", "uyvy", "p010")
FLOAT_KINDS = {"float16-window": "float16", "bfloat16-window": "bfloat16", "float32-window": "float32"}
FLOAT_RANGES = ("unit", "byte")
TABLE_KINDS = ("encode", "size_table", "rd_table")
KT_FAMILIES = ["kt-" + f for f in ("surface-4-bgr-gap", "surface-3-rgb-packed", "planes-nv12", "planes-i420", "yuy2", "rgbplanes-pitched")]
KP_FAMILIES = ["kp-planes-i420", "kp-planes-nv12", "kp-planes-reference", "kp-rgbplanes-pitched"]
NEW_FAMILIES = ["rgbplanes-pitched", "rgbplanes-bgr", *FLOAT_KINDS, *SAMPLE_PRESETS, *KT_FAMILIES, *KP_FAMILIES]
# how a plane-table family groups its planes into allocations (tests/test_gpu_plane_table.py): NV12's chroma entries share one
_KP_GROUPS = {"i420": SEPARATE, "nv12": (((0, 0),), ((1, 0), (2, 0))), "reference": SEPARATE}


def base_family(family):
    """(table mode "", "kt" or "kp", the family behind the prefix)."""
    return (family[:2], family[3:]) if family.startswith(("kt-", "kp-")) else ("", family)


def kernels(family):
    """The source names of the registry entries (kKernels, csrc/m1v_kernels.hip) that the family's encode, size-table and
    rd-table calls launch."""
    table, base = base_family(family)
    if base in ("rgb", "rgb-fallback"):
        stem = "tiles"
    elif base == "rgb-runs":                    # (its size table is one probe per quality on the run kernels)
        return ("k_encode_dense", "k_encode_strips")
    elif base == "rgba":                        # the encode by the height: strips of fewer than 64 blocks, or dense
        return ("k_encode_dense", "k_encode_strips", "k_size_table_rgba", "k_rd_table_rgba")
    elif base.startswith("surface-"):
        stem = "surface"
    elif base.startswith("planes-"):
        stem = "planes"
    elif base.startswith("rgbplanes-"):
        stem = "rgb_planes"
    elif base in FLOAT_KINDS:
        stem = "float_planes"
    else:
        assert base in SAMPLE_PRESETS, family
        stem = "step2"
    return tuple(f"k{table[1:]}_{row}_{stem}" for row in TABLE_KINDS)


def content_form(family):
    """What a family takes when a sweep has both forms of one content: "pixels" or "planes"."""
    base = base_family(family)[1]
    return "planes" if base.startswith("planes-") or base in SAMPLE_PRESETS else "pixels"


# ---- the host side: pure numpy, pinned by tests/test_input_families_cpu.py --------------------------------------------------
def _round_to(x32, kind):
    """fp32 values rounded to `kind` (nearest even), as bit patterns — the rounding of float_planes.jitter_noise."""
    if kind == "float16":
        return x32.astype(np.float16).view(np.uint16)
    if kind == "bfloat16":
        u = x32.view(np.uint32)
        return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return x32.view(np.uint32).copy()


def float_bits(px, kind, rng, seed=0):
    """Packed pixels [n, H, W, 3] -> bit patterns [n, 3, H, W] of `kind` whose byte under the rule (float_planes.rule_bytes) is
    that pixel: (byte + jitter) / 255 (range unit) or byte + jitter (range byte) with jitter uniform in +-0.49, as
    float_planes.jitter_noise draws it, rounded to the type; where the type does not resolve the jitter (bfloat16 has 8
    significant bits) the sample is the type's nearest value to the byte itself.  Verified against the rule here."""
    byte = np.ascontiguousarray(px[..., :3].transpose(0, 3, 1, 2)).astype(np.float64)
    scale = 255.0 if rng == "unit" else 1.0
    jitter = np.random.default_rng(7000 + seed).uniform(-0.49, 0.49, byte.shape)
    bits = _round_to(((byte + jitter) / scale).astype(np.float32), kind)
    want = byte.astype(np.uint8)
    plain = _round_to((byte / scale).astype(np.float32), kind)
    bits = np.where(fp.rule_bytes(bits, kind, rng) == want, bits, plain)
    assert np.array_equal(fp.rule_bytes(bits, kind, rng), want), (kind, rng)
    return bits


def sample_frames(preset, W, H, Y, Cb, Cr, fill_seed=0):
    """Plane-form content in the tight sample preset -> (host image of the buffer, layout, byte offset of frame 0): noise of
    fill_seed as a whole, the addressed bytes are the planes (tests/layout_inputs.py's _noise and _scatter)."""
    from ec504_imageencoder_amd import sample_layout_preset
    lay = sample_layout_preset(W, H, preset)
    host = _sample_noise(Y.shape[0], lay, GUARD, seed=5000 + fill_seed)
    _sample_scatter(host, lay, GUARD, Y, Cb, Cr)
    return host, lay, GUARD


def region(W, H, mode):
    sh = gs.shape(W, H, mode)
    return 16 * sh["n_strips"], 16 * sh["n_mbrows"]


def plane_table_family(family):
    """The tests/test_gpu_plane_table.py family object of a kp- family."""
    base = base_family(family)[1]
    if base == "rgbplanes-pitched":
        return _Rgb("rgb")
    preset = base.split("-")[1]
    return _Ycc(preset, _KP_GROUPS[preset])


def plane_ranges(family, W, H, mode):
    """Per plane of a kp- family (v, lo, E, A) as _Ycc.planes / _Rgb.planes give them, for the coded region of the mode."""
    return plane_table_family(family).planes(W, H, region(W, H, mode))


class _YccFrames(_Samples):
    """tests/layout_inputs.py's _Samples for any layout of tests/test_gpu_planes.py: a frame is the bytes of its extent."""

    def __init__(self, preset, mode):
        self.preset, self.mode = preset, mode

    def layout(self, W, H):
        from ec504_imageencoder_amd import sample_layout_preset
        if self.preset in SAMPLE_PRESETS:
            return sample_layout_preset(W, H, self.preset)
        return dict(_layout(self.preset, W, H)[0], y_step=1)

    def span(self, W, H):
        from ec504_imageencoder_amd.encoder import plane_layout_extent
        xe, ye = region(W, H, self.mode)
        return plane_layout_extent(self.layout(W, H), xe // 16, ye // 16)

    def frames(self, W, H, Y, Cb, Cr, fill_seed):
        """One host image per frame: noise of fill_seed, the addressed bytes the planes."""
        lay, L = self.layout(W, H), self.span(W, H)
        rng = np.random.default_rng(6000 + fill_seed)
        out = []
        for f in range(Y.shape[0]):
            host = rng.integers(0, 256, L, dtype=np.uint8)
            _sample_scatter(host, lay, 0, Y[f:f + 1], Cb[f:f + 1], Cr[f:f + 1])
            out.append(host)
        return out


def _frame_table_family(base, mode):
    """The tests/test_gpu_frame_table.py family object behind a kt- family."""
    if base.startswith("surface-"):
        _, channels, order, layout = base.split("-")
        assert layout in ("packed", "odd", "gap")
        return _Surface(int(channels), _surface_geometry(layout, 0, 1, int(channels))[0], order)     # (the pitch less W * C)
    if base == "rgbplanes-pitched":
        return _RgbPlanes()
    return _YccFrames(base.split("-")[1] if base.startswith("planes-") else base, mode)


# ---- placement of scattered frames and planes (every frame its own picture) -------------------------------------------------
def _pool(torch, size, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    pool = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda", generator=gen)
    assert pool.data_ptr() % 16 == 0
    return pool


def _memory_order(n):
    """tests/test_gpu_frame_table.py's: descending with the first two swapped — a permutation of the batch's, not ascending."""
    order = list(range(n))[::-1]
    if n >= 3:
        order[0], order[1] = order[1], order[0]
    return order


def scatter_frames(torch, fam, pics, W, H, fill_seed=0):
    """tests/test_gpu_frame_table.py's _scatter with every frame a picture of its own: a pool of noise of fill_seed, each frame
    GUARD bytes and more from its neighbours, bases of the residues mod 16 of RESIDUES, unequal gaps.  Returns (pool, bases)."""
    L = fam.span(W, H)
    where, cursor = {}, GUARD
    for k, p in enumerate(_memory_order(len(pics))):
        where[p] = (cursor + 15) // 16 * 16 + RESIDUES[k % len(RESIDUES)]
        cursor = where[p] + L + GUARD + 16 * ((5 * k) % 7)
    pool = _pool(torch, cursor + GUARD, 3000 + fill_seed)
    for p, pic in enumerate(pics):
        fam.write(torch, pool, where[p], pic, W, H)
    return pool, [where[p] for p in range(len(pics))]


def place_planes(torch, fam, virtuals, W, H, reg, fill_seed=0):
    """tests/test_gpu_plane_table.py's _place with every frame a picture of its own: each block (a group of planes that share an
    allocation; its bytes are exactly the planes' read-contract ranges) in a pool per group, GUARD bytes and more around it,
    bases of several residues mod 16; of a block only the addressed samples are written.  Returns (pools, int64 [n, 3])."""
    blocks = _blocks(fam, W, H, reg)
    G, n = len(blocks), len(virtuals)
    where, cursors = {}, [GUARD] * G
    for k, pic in enumerate(_memory_order(n)):
        for g in range(G):
            at = (cursors[g] + 15) // 16 * 16 + RESIDUES[(k + 3 * g) % len(RESIDUES)]
            where[(pic, g)] = at
            cursors[g] = at + blocks[g][1] + GUARD + 16 * ((5 * k + g) % 7)
    pools = [_pool(torch, max(cursors) + GUARD, 4000 + fill_seed + 100 * g) for g in range(G)]
    by_address = sorted(range(G), key=lambda i: pools[i].data_ptr())
    pool_of = {g: by_address[(g - 1) % G] for g in range(G)}      # luma goes to the highest: never Y, Cb, Cr memory order
    host = [p.cpu().numpy() for p in pools]
    table = np.zeros((n, 3), np.int64)
    for (pic, g), at in where.items():
        v0, length, pointers, A = blocks[g]
        assert at >= GUARD and at + length + GUARD <= len(host[pool_of[g]])
        host[pool_of[g]][at + (A - v0)] = virtuals[pic][A]
        for p, d in pointers:                   # (d < 0 for an RGB plane: its range starts c_offset behind its pointer)
            table[pic, p] = pools[pool_of[g]].data_ptr() + at + d
    for p, h in zip(pools, host):
        p.copy_(torch.from_numpy(h))
    return pools, table


# ---- the builder ------------------------------------------------------------------------------------------------------------
class Input:
    """What build() returns.  enc, dev, kind, kernels; keep holds the allocations alive; buf, lay, base are those of a plane
    layout in stride mode (tests/gpu_calls.py's _oracle_on_buffer reads them)."""
    buf = lay = base = None

    def __init__(self, family, enc, dev, kind, keep=()):
        self.family, self.enc, self.dev, self.kind, self.keep, self.kernels = family, enc, dev, kind, keep, kernels(family)


def _new_encoder(W, H, Q, mode, cap, channels=3):
    from ec504_imageencoder_amd import Mpeg1Encoder
    return Mpeg1Encoder(W, H, Q, mode, channels=channels, max_frames=cap)


def _tiles(enc):
    assert enc.path == "tiles" and enc.size_table_fused == 1
    return enc


def build(torch, family, W, H, mode, quality, max_frames, pixels=None, planes=None, orc=None, fill_seed=None, offset=None,
          forced_runs=False, float_range="unit"):
    """pixels: packed [n, H, W, 3 | 4]; planes: (Y [n, ye, xe], Cb, Cr [n, ye / 2, xe / 2]) — exactly one of them.  A YCbCr
    family given pixels takes the planes the oracle converts them to (orc) and keeps the RGB records.  offset: the packed
    families' bytes between a 256-byte boundary and the buffer's first byte (None: a tensor of its own)."""
    assert (pixels is None) != (planes is None)
    table, base = base_family(family)
    fill = len(family) if fill_seed is None else fill_seed
    Q, cap = quality, max_frames
    kind = "planes" if pixels is None else ("rgba" if pixels.shape[-1] == 4 else "rgb")
    ycc = base.startswith("planes-") or base in SAMPLE_PRESETS
    assert ycc or pixels is not None, family
    if ycc and pixels is not None:
        assert base.startswith("planes-"), family
        planes = _addressed(orc, pixels, mode)
    xe, ye = region(W, H, mode)

    if table == "kt":
        fam = _frame_table_family(base, mode)
        enc = _new_encoder(W, H, Q, mode, cap, getattr(fam, "channels", 3))
        if ycc:
            pics = fam.frames(W, H, *planes, fill_seed=fill)
            enc.set_sample_layout(dict(fam.layout(W, H), frame_stride=fam.span(W, H)))
        elif isinstance(fam, _Surface):
            pics = list(pixels)
            enc.set_input_layout(fam.pitch(W), 0, fam.order)
        else:
            pics, P = list(pixels), fam.pitch(W)
            enc.set_rgb_plane_layout(dict(r_offset=0, g_offset=H * P, b_offset=2 * H * P, row_pitch=P, frame_stride=3 * H * P))
        _tiles(enc).set_frame_table()
        assert enc.frame_table and enc.path == "tiles"
        pool, bases = scatter_frames(torch, fam, pics, W, H, fill_seed=fill)
        return Input(family, enc, _addresses(torch, pool, bases), kind, keep=(pool,))

    if table == "kp":
        fam = plane_table_family(family)
        enc = _new_encoder(W, H, Q, mode, cap)
        if fam.rgb:
            virtuals = [fam.virtual(pic, W, H) for pic in pixels]
            enc.set_rgb_plane_layout(fam.encoder_layout(W, H))
        else:
            lay = fam.oracle_layout(W, H)
            virtuals = []
            for f in range(planes[0].shape[0]):
                v = np.zeros(lay["frame_stride"], np.uint8)
                _sample_scatter(v, lay, 0, *(p[f:f + 1] for p in planes))
                virtuals.append(v)
            enc.set_plane_layout(fam.encoder_layout(W, H))
        _tiles(enc).set_plane_table()
        assert enc.plane_table and not enc.frame_table and enc.path == "tiles"
        pools, addresses = place_planes(torch, fam, virtuals, W, H, (xe, ye), fill_seed=fill)
        return Input(family, enc, _device_table(torch, addresses), kind, keep=tuple(pools))

    if base.startswith("planes-"):
        lay, at = _layout(base.split("-")[1], W, H)
        n = planes[0].shape[0]
        buf = _buffer(torch, n, lay, at, fill_seed=fill)
        _write_planes(torch, buf, lay, at, *planes)
        enc = _plane_encoder(W, H, Q, mode, cap, lay)
        out = Input(family, enc, _view(torch, buf, n, lay, at, enc), kind, keep=(buf,))
        out.buf, out.lay, out.base = buf, lay, at
        return out

    if base in SAMPLE_PRESETS:
        host, lay, at = sample_frames(base, W, H, *planes, fill_seed=fill)
        enc = _new_encoder(W, H, Q, mode, cap)
        enc.set_sample_layout(lay)
        assert _tiles(enc).sample_layout == lay
        buf = torch.from_numpy(host).cuda()
        return Input(family, enc, _sample_view(torch, buf, planes[0].shape[0], lay, at, enc), kind, keep=(buf,))

    if base.startswith("surface-"):
        _, channels, order, layout = base.split("-")
        assert pixels.shape[-1] == int(channels)
        dev, pitch, stride = _surface(torch, pixels, layout, order, fill_seed=fill)
        return Input(family, _surface_encoder(W, H, Q, mode, int(channels), cap, pitch, stride, order), dev, kind)

    if base.startswith("rgbplanes-"):
        dev, lay = _planar(torch, pixels, base.split("-")[1], fill_seed=fill)
        enc = _new_encoder(W, H, Q, mode, cap)
        enc.set_rgb_plane_layout(lay)
        assert _tiles(enc).rgb_plane_layout == lay
        return Input(family, enc, dev, kind)

    if base in FLOAT_KINDS:
        bits = float_bits(pixels, FLOAT_KINDS[base], float_range, seed=fill)
        dev, lay = _tensor(torch, bits, FLOAT_KINDS[base], "window", float_range, seed=fill)
        enc = _new_encoder(W, H, Q, mode, cap)
        enc.set_float_plane_layout(lay)
        assert _tiles(enc).float_plane_layout == lay
        return Input(family, enc, dev, kind)

    assert base in ("rgb", "rgb-fallback", "rgb-runs", "rgba") and kind == ("rgba" if base == "rgba" else "rgb"), family
    px = pixels
    keep = ()
    if offset is None:
        dev = torch.from_numpy(px.copy()).cuda()
    else:
        buf = torch.zeros(px.size + 8, dtype=torch.uint8, device="cuda")
        dev = buf[offset:offset + px.size].view(px.shape)
        dev.copy_(torch.from_numpy(px.copy()).cuda())
        assert dev.data_ptr() % 256 == offset
        keep = (buf,)
    enc = _new_encoder(W, H, Q, mode, cap, px.shape[-1])
    if base == "rgb-runs" or forced_runs:         # the K-probe fallback: one run-kernel probe per quality
        enc.debug_set_path("runs")
        assert enc.path == "runs" and enc.size_table_fused == 0
    else:                                         # README: 3 channels on the tile path and 4 channels always take the fused pass
        assert enc.path == ("tiles" if kind == "rgb" else "runs") and enc.size_table_fused == 1
    if base == "rgb-fallback":
        enc.debug_set_lds_words(8)
        enc.reserve_scratch(True)
    return Input(family, enc, dev, kind, keep)
