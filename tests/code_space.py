"""Content that walks the whole code space of the entropy stage, and a census of it — TEST INFRASTRUCTURE ONLY (no tests in this
module; tests/test_code_space_cpu.py pins the census, tests/test_gpu_code_space.py feeds the kernels).

tests/hard_content.py loads the entropy stage; this module enumerates it.  Two things are enumerated, and the oracle decides
about every block of either:

  AC pairs    For r = run - 1 in 0..61, |L| in 1..255 and both signs one block of samples: 128 plus the inverse DCT of ONE
              coefficient at zigzag position r + 2, of amplitude (|L| + 1/2) x the divisor of quality q there, rounded and clipped
              to 0..255.  The block is accepted when the oracle (orc.fdct, orc.quant_zigzag) gives a non-zero DC level, nothing at
              positions 1..r + 1 and exactly L at r + 2, and codes the whole block: (r, L) is then the FIRST pair the reference
              codes of it, whatever clipping and rounding add behind.  Qualities are tried from the top of the allowed range
              downwards and the first that accepts is taken.  "narrow" allows qualities up to 76 (every level stages in one byte),
              "wide" up to 92.  A pair that no quality accepts is not in the set: what no block of samples reaches is outside the
              reference's behaviour.
  DC levels   For k in 2..2042 the block of sample sum S = 8 k - 16 (flat S // 64, the first S % 64 samples one higher): the
              oracle's FDCT gives the DC coefficient (S + 16) >> 3 = k, which is the DC level where the DC divisor is 1
              (qualities 92..100).  Levels 0 and 1 come from flat blocks of 0 and 1 at quality 50 (DC divisor 8).

The accepted blocks are laid out as 352x288 frames, ONE QUALITY PER FRAME (frames of a set are encoded with per-frame quality),
sorted by quality (descending), r, |L| and sign, so that a frame holds a contiguous range of pairs; what is left of a frame is
flat 128.  Three forms:

  luma planes    the blocks themselves (form "planes": Y of a plane layout)
  chroma planes  (form "planes": Cb, Cr) blocks of the same quality group again, behind the chroma DC size table: the 110 table
                 entries and each row's first escape level first, then the others from the longest run downwards
  grey pictures  R = G = B = the block (form "grey", for the RGB, RGBA and surface families); acceptance is checked again on the
                 luma orc.convert makes of the grey block, and a block that fails it is searched for again on that luma

census() reads a set of frames back through the oracle alone."""
import ctypes as C

import numpy as np

import hard_content as hc

W, H = 352, 288
BW, BH = W // 8, H // 8                   # 44 x 36 luma blocks, 22 x 18 chroma blocks per plane
LUMA_SLOTS, CHROMA_SLOTS = BW * BH, 2 * (BW // 2) * (BH // 2)
TOP = {"narrow": 76, "wide": 92}
DC_Q, DC_LOW_Q = 92, 50
RUNS = range(62)
_cache = {}


# ---- the oracle, called without per-call conversions ------------------------------------------------------------------------
class _Block:
    """orc.fdct + orc.quant_zigzag on preallocated buffers."""

    def __init__(self, orc):
        self.orc, self.L = orc, orc.lib()
        self.px, self.dct, self.zz = np.empty(64, np.uint8), np.empty(64, np.int32), np.empty(64, np.int32)
        self.pp, self.dp, self.zp = self.px.ctypes.data_as(orc._u8p), self.dct.ctypes.data_as(orc._i32p), self.zz.ctypes.data_as(orc._i32p)
        self.div = {q: orc.scale_qmatrix(q) for q in range(1, 101)}
        self.divp = {q: d.ctypes.data_as(orc._i32p) for q, d in self.div.items()}
        self.bits = orc.OrcBits()

    def levels(self, px, q):
        """The 64 zigzag levels of 64 samples at quality q (a view of a buffer: copy to keep)."""
        self.px[:] = px
        self.L.orc_fdct(self.pp, self.dp)
        self.L.orc_quant_zigzag(self.dp, self.divp[q], self.zp)
        return self.zz

    def codable(self):
        """Whether the oracle codes the levels of the last call."""
        self.L.orc_bits_init(C.byref(self.bits))
        rc = self.L.orc_encode_block(1, self.zp, C.byref(self.bits))
        self.L.orc_bits_free(C.byref(self.bits))
        return rc == 0


def _bases():
    """[64, 64]: the samples of a unit coefficient at each zigzag position (orthonormal inverse DCT, the scale of orc.fdct)."""
    from scipy.fft import idctn
    inv = np.argsort(hc._ZIGZAG)
    out = np.zeros((64, 64))
    for pos in range(64):
        c = np.zeros(64)
        c[inv[pos]] = 1.0
        out[pos] = idctn(c.reshape(8, 8), norm="ortho").reshape(64)
    return out, inv


def row_lengths(orc):
    """The 32 row lengths of the run/level table, from the oracle: row r holds codes for |level| 1..row_lengths[r]; the next
    level is the row's first escape (hard_content._ac_bits: a table code has at most 17 bits)."""
    if "rows" not in _cache:
        rows = []
        for r in range(32):
            n = 0
            while hc._ac_bits(orc, r, n + 1) <= 17:
                n += 1
            rows.append(n)
        assert all(hc._ac_bits(orc, r, 1) == 20 for r in range(32, 62))
        _cache["rows"] = tuple(rows)
    return _cache["rows"]


def table_entries(orc):
    """The (r, |L|) of the 110 table entries."""
    return [(r, lv) for r, n in enumerate(row_lengths(orc)) for lv in range(1, n + 1)]


def first_escapes(orc):
    """The (r, |L|) of each row's first escape level."""
    return [(r, n + 1) for r, n in enumerate(row_lengths(orc))]


# ---- AC pairs ---------------------------------------------------------------------------------------------------------------
def _grey_of_luma(orc):
    """(grey [256], luma [256]): for each wanted luma the grey value R = G = B whose converted luma is nearest (the oracle maps
    the 256 greys onto 204 lumas, each within 1 of the grey), and the oracle's luma of every grey."""
    g = np.arange(256, dtype=np.uint8)
    luma = orc.convert(np.repeat(g[:, None], 3, 1))[0]
    want = np.arange(256)
    grey = np.abs(luma.astype(int)[None, :] - want[:, None]).argmin(1).astype(np.uint8)
    return grey, luma


def _search(blk, bases, inv, r, level, top, grey=None):
    """(q, samples [64] uint8) of the first quality from `top` downwards that accepts (r, level), or None.
    At each quality the plain block comes first: amplitude (|L| + 1/2) x divisor.  Where clipping to 0..255 leaves it short of
    the level, the amplitude is raised by bisection between the plain one and the sign pattern of the basis function (which
    gives the largest coefficient samples in 0..255 can give): the coefficient grows with the amplitude.  Where even the sign
    pattern falls short the search ends, as divisors only grow when the quality falls.
    grey: (grey of luma, luma of grey) — the samples are grey values and acceptance is on their converted luma."""
    pos = r + 2
    n = inv[pos]
    sign = 1 if level > 0 else -1
    want = abs(level)

    def attempt(amplitude, q):
        px = np.clip(np.rint(128 + sign * amplitude * bases[pos]), 0, 255).astype(np.uint8)
        if grey is not None:
            px = grey[0][px]
        zz = blk.levels(px if grey is None else grey[1][px], q)
        ok = zz[pos] == level and zz[0] != 0 and not zz[1:pos].any() and blk.codable()
        return px, abs(int(zz[pos])) if zz[pos] * sign >= 0 else -1, ok

    for q in range(top, 0, -1):
        d = int(blk.div[q][n])
        lo = (want + 0.5) * d
        px, got, ok = attempt(lo, q)
        if ok:
            return q, px
        if got >= want:
            continue                                  # the level is there, something else is in the way: next quality
        hi = 1e5
        if attempt(hi, q)[1] < want:
            return None
        for _ in range(24):
            mid = (lo + hi) / 2
            px, got, ok = attempt(mid, q)
            if ok:
                return q, px
            if got == want:
                break
            lo, hi = (mid, hi) if got < want else (lo, mid)
    return None


def ac_blocks(orc, kind, form):
    """[(q, r, L, samples [64] uint8)] of the set `kind` ("narrow" | "wide") in form "planes" | "grey", sorted by quality
    (descending), r, |L| and sign.  In form "grey" the samples are the grey value of the pixels, and acceptance holds for the
    luma the oracle converts them to."""
    key = ("ac", kind, form)
    if key not in _cache:
        blk = _Block(orc)
        bases, inv = _bases()
        grey = _grey_of_luma(orc) if form == "grey" else None
        out = []
        for r in RUNS:
            for lv in range(1, 256):
                for level in (lv, -lv):
                    hit = _search(blk, bases, inv, r, level, TOP[kind], grey)
                    if hit:
                        out.append((hit[0], r, level, hit[1]))
        out.sort(key=lambda e: (-e[0], e[1], abs(e[2]), e[2] < 0))
        _cache[key] = out
    return _cache[key]


def _fill(planes, slots_per_frame, blocks_wide, blocks):
    """Writes 8x8 blocks into the planes [n, h, w] in raster order of each plane's blocks, plane after plane."""
    for i, px in enumerate(blocks):
        f, k = divmod(i, slots_per_frame)
        by, bx = divmod(k, blocks_wide)
        planes[f, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = np.asarray(px).reshape(8, 8)


def ac_frames(orc, kind, form):
    """The frames of a set: dict(form, qualities [n], Y [n, H, W] and, for form "planes", Cb, Cr [n, H / 2, W / 2]; for form
    "grey", rgb [n, H, W, 3]).  Read-only, built once."""
    key = ("frames", kind, form)
    if key not in _cache:
        blocks = ac_blocks(orc, kind, form)
        priority = set(table_entries(orc)) | set(first_escapes(orc))
        quals, Ys, Cbs, Crs = [], [], [], []
        for q in sorted({e[0] for e in blocks}, reverse=True):
            group = [e for e in blocks if e[0] == q]
            n = -(-len(group) // LUMA_SLOTS)
            Y = np.full((n, H, W), 128, np.uint8)
            _fill(Y, LUMA_SLOTS, BW, [e[3] for e in group])
            quals += [q] * n
            Ys.append(Y)
            if form == "planes":
                first = [e for e in group if (e[1], abs(e[2])) in priority]
                rest = [e for e in group if (e[1], abs(e[2])) not in priority]
                assert len(first) <= n * CHROMA_SLOTS, (q, len(first))
                chroma = np.full((2 * n, H // 2, W // 2), 128, np.uint8)       # Cb, Cr of frame 0, Cb, Cr of frame 1, ...
                _fill(chroma, CHROMA_SLOTS // 2, BW // 2, [e[3] for e in (first + rest[::-1])[:n * CHROMA_SLOTS]])
                Cbs.append(chroma[0::2])
                Crs.append(chroma[1::2])
        out = dict(form=form, qualities=quals, Y=np.concatenate(Ys))
        if form == "planes":
            out.update(Cb=np.concatenate(Cbs), Cr=np.concatenate(Crs))
        else:
            out["rgb"] = np.ascontiguousarray(np.repeat(out["Y"][..., None], 3, 3))
        _cache[key] = _frozen(out)
    return _cache[key]


def _frozen(frames):
    for v in frames.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return frames


# ---- DC levels --------------------------------------------------------------------------------------------------------------
def dc_block(k):
    """Samples [64] whose DC coefficient is k (2..2042): sum 8 k - 16."""
    assert 2 <= k <= 2042
    v, extra = divmod(8 * k - 16, 64)
    px = np.full(64, v, np.uint8)
    px[:extra] += 1
    return px


DC_LEVELS = range(2, 2043)
DC_FRAMES = 3                             # 3 x 792 chroma slots hold the 2041 levels once; the luma slots hold them twice


def dc_frames(orc, form):
    """DC_FRAMES frames at quality DC_Q whose luma blocks walk the DC levels 2..2042 (block i of the set: level 2 + i % 2041) and,
    in form "planes", whose chroma blocks do (block j: 2 + (j + 1000) % 2041), then one frame at quality DC_LOW_Q of flat blocks
    of 0, 1 and 2 (DC levels 0, 1 and 2 there).  The same dict as ac_frames."""
    key = ("dc", form)
    if key not in _cache:
        n = DC_FRAMES + 1
        m = len(DC_LEVELS)
        Y = np.zeros((n, H, W), np.uint8)
        _fill(Y, LUMA_SLOTS, BW, [dc_block(2 + i % m) for i in range(DC_FRAMES * LUMA_SLOTS)])
        _fill(Y[DC_FRAMES:], LUMA_SLOTS, BW, [np.full(64, i % 3, np.uint8) for i in range(LUMA_SLOTS)])
        out = dict(form=form, qualities=[DC_Q] * DC_FRAMES + [DC_LOW_Q], Y=Y)
        if form == "planes":
            chroma = np.zeros((2 * n, H // 2, W // 2), np.uint8)
            _fill(chroma, CHROMA_SLOTS // 2, BW // 2, [dc_block(2 + (j + 1000) % m) for j in range(DC_FRAMES * CHROMA_SLOTS)])
            _fill(chroma[2 * DC_FRAMES:], CHROMA_SLOTS // 2, BW // 2, [np.full(64, j % 3, np.uint8) for j in range(CHROMA_SLOTS)])
            out.update(Cb=chroma[0::2], Cr=chroma[1::2])
        else:
            out["rgb"] = np.ascontiguousarray(np.repeat(Y[..., None], 3, 3))
        _cache[key] = _frozen(out)
    return _cache[key]


# ---- reading a set back through the oracle ----------------------------------------------------------------------------------
def plane_levels(orc, plane, q):
    """Zigzag levels [blocks, 64] of every 8x8 block of one plane at quality q, in raster order of the plane's blocks
    (hard_content.plane_coefficients, on preallocated buffers)."""
    blk = _cache.setdefault("block", _Block(orc))
    h, w = plane.shape
    return np.stack([blk.levels(plane[by:by + 8, bx:bx + 8].reshape(64), q).copy() for by in range(0, h - 7, 8) for bx in range(0, w - 7, 8)])


def frame_levels(orc, frames, f, q=None):
    """Zigzag levels [blocks, 64] of frame f at quality q (default: the frame's own) in coding order: strips of 16 columns
    from the left, macroblocks downwards, four luma blocks, Cb, Cr."""
    q = frames["qualities"][f] if q is None else q
    if frames["form"] == "grey":
        return orc.frame_coefficients(frames["rgb"][f], W, H, q, orc.MODE_FULL)
    y = plane_levels(orc, frames["Y"][f], q).reshape(BH, BW, 64)
    cb = plane_levels(orc, frames["Cb"][f], q).reshape(BH // 2, BW // 2, 64)
    cr = plane_levels(orc, frames["Cr"][f], q).reshape(BH // 2, BW // 2, 64)
    out = []
    for sx in range(BW // 2):
        for my in range(BH // 2):
            out += [y[2 * my + b // 2, 2 * sx + b % 2] for b in range(4)] + [cb[my, sx], cr[my, sx]]
    return np.stack(out)


def frame_encodable(orc, frames, f, q=None):
    """Whether the oracle codes every block of frame f at quality q (default: the frame's own)."""
    q = frames["qualities"][f] if q is None else q
    if frames["form"] == "grey":
        return hc.frame_encodable(orc, frames["rgb"][f], q)
    blk = _cache.setdefault("block", _Block(orc))
    for p in ("Y", "Cb", "Cr"):
        plane = frames[p][f]
        for by in range(0, plane.shape[0], 8):
            for bx in range(0, plane.shape[1], 8):
                blk.levels(plane[by:by + 8, bx:bx + 8].reshape(64), q)
                if not blk.codable():
                    return False
    return True


def block_names(orc, frames, f, q=None):
    """Per block of frame f in coding order: (is_luma, DC level, first coded pair (r, L) or None)."""
    out = []
    for i, z in enumerate(frame_levels(orc, frames, f, q)):
        pairs = hc.coded_pairs(z)
        out.append((i % 6 < 4, int(z[0]), pairs[0] if pairs else None))
    return out


def census(orc, frames):
    """What a set of frames makes the reference code, each frame at its own quality, from the oracle's coefficients alone:
      first_luma, first_chroma   the set of signed (r, L) that is the FIRST coded pair of a block (hard_content.coded_pairs)
      dc_luma, dc_chroma         the set of DC levels
      blocks                     the number of blocks"""
    key = ("census", id(frames))
    if key not in _cache:
        out = dict(first_luma=set(), first_chroma=set(), dc_luma=set(), dc_chroma=set(), blocks=0)
        for f in range(len(frames["qualities"])):
            for luma, dc, first in block_names(orc, frames, f):
                out["dc_luma" if luma else "dc_chroma"].add(dc)
                if first:
                    out["first_luma" if luma else "first_chroma"].add(first)
                out["blocks"] += 1
        _cache[key] = (frames, out)              # (keeps `frames` alive: its id is the key)
    return _cache[key][1]


def both_signs(pairs):
    """The set of (r, |L|) that a set of signed pairs holds in both signs."""
    return {(r, lv) for r, lv in pairs if lv > 0 and (r, -lv) in pairs}


def _code_at(orc, luma, z, offset):
    """Which code of a block holds bit `offset` of the block's bits: text."""
    dc = hc._dc_bits(orc, luma, z[0])
    if offset < dc:
        return f"in the DC code of level {int(z[0])} ({'luma' if luma else 'chroma'} size table; the level's low byte is {abs(int(z[0])) & 0xff})"
    at = dc
    for k, (r, level) in enumerate(hc.coded_pairs(z)):
        n = hc._ac_bits(orc, r, level)
        if offset < at + n:
            return f"in the code of pair {k} of the block, (r = {r}, L = {level}), {'a table entry' if n <= 17 else f'a {n}-bit escape'}"
        at += n
    return "in the end-of-block code"


def describe_difference(orc, frames, f, got, want, q=None, index=0):
    """Text for a failed comparison of the record of frame f: the first code whose bits differ, by name.  got, want: the
    frame's record (44 header bytes, then per strip 38 header bits, per macroblock 2 bits and six blocks, zero bits to the next
    byte; 4 trailer bytes).  The payload is compared first: a record of another length differs in its header's length field,
    which names nothing.  The codes' lengths are the oracle's (orc.encode_block_bits, hard_content._ac_bits)."""
    q = frames["qualities"][f] if q is None else q
    head = f"frame {index + f} (quality {q})"
    if got == want:
        return f"{head}: records are equal"
    n = min(len(got), len(want))
    at = next((i for i in range(44, n) if got[i] != want[i]), n)
    if at == n:
        first = next((i for i in range(min(n, 44)) if got[i] != want[i]), n)
        return f"{head}: first difference at byte {first}, outside the blocks; sizes {len(got)} / {len(want)}"
    bit = 8 * (at - 44) + 8 - (got[at] ^ want[at]).bit_length()      # the first differing bit of the payload
    levels = frame_levels(orc, frames, f, q)
    pos, i = 0, 0
    for sx in range(BW // 2):
        pos += 38
        for my in range(BH // 2):
            pos += 2
            for b in range(6):
                rc, s = orc.encode_block_bits(b < 4, levels[i])
                assert rc == 0
                if pos + len(s) > bit:
                    z = levels[i]
                    pairs = hc.coded_pairs(z)
                    pair = "no AC code" if not pairs else f"first pair (r = {pairs[0][0]}, L = {pairs[0][1]})"
                    where = _code_at(orc, b < 4, z, bit - pos) if bit >= pos else "in the header bits before the block"
                    return (f"{head}, strip {sx}, macroblock {my}, block {b} ({'luma' if b < 4 else 'chroma'}): DC level {int(z[0])}, "
                            f"{pair}; the first differing bit is {where} (bit {bit} of the payload, byte {at} of the record; "
                            f"the block's {len(s)} bits start at {pos}); sizes {len(got)} / {len(want)}")
                pos += len(s)
                i += 1
        pos = (pos + 7) & ~7
    return f"{head}: first difference at byte {at}, behind the last block; sizes {len(got)} / {len(want)}"


def describe_frame(orc, frames, f, q=None):
    """Text for a failed comparison of a number (a size, a distortion) of frame f: what the frame carries."""
    names = block_names(orc, frames, f, q)
    firsts = [x[2] for x in names if x[2]]
    dcs = sorted({x[1] for x in names})
    span = f"first pairs (r, L) from {firsts[0]} to {firsts[-1]} ({len(set(firsts))} distinct)" if firsts else "no AC codes"
    return f"frame {f} (own quality {frames['qualities'][f]}): {span}, DC levels {dcs[0]}..{dcs[-1]} ({len(dcs)} distinct)"


# ---- the same space as zigzag blocks, for the pins of the oracle itself -------------------------------------------------------
def exhaustive_groups():
    """{group name: [(is_luma, zigzag block [64] int32)]}: every code word the block coder can be asked for, whether a block of
    samples reaches it or not.
      ac_dc1_rNN   z[0] = 1, z[r + 2] = L for L = 1, -1, 2, -2, ... 255, -255, as luma and then as chroma (r = 0..61)
      ac_dc0_rNN   z[0] = 0, z[r + 1] = L likewise (r = 0..62: the first pair's run starts at position 0)
      dc_luma, dc_chroma   z[0] = -2042..2042 alone"""
    levels = [s * lv for lv in range(1, 256) for s in (1, -1)]
    out = {}
    for kind, dc, runs in (("dc1", 1, range(62)), ("dc0", 0, range(63))):
        for r in runs:
            blocks = []
            for luma in (1, 0):
                for lv in levels:
                    z = np.zeros(64, np.int32)
                    z[0] = dc
                    z[r + 1 + dc] = lv
                    blocks.append((luma, z))
            out[f"ac_{kind}_r{r:02d}"] = blocks
    for luma, name in ((1, "dc_luma"), (0, "dc_chroma")):
        blocks = []
        for k in range(-2042, 2043):
            z = np.zeros(64, np.int32)
            z[0] = k
            blocks.append((luma, z))
        out[name] = blocks
    return out


def group_digest(block_bits, blocks):
    """SHA-256 over the bit strings block_bits(is_luma, z) of a group, one per line."""
    import hashlib
    return hashlib.sha256("\n".join(block_bits(luma, z) for luma, z in blocks).encode()).hexdigest()
