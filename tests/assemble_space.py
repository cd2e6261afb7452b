"""The placement space of k_assemble (ec504_imageencoder_amd/csrc/m1v_assemble.h): the cases that walk it, a CPU model of the
kernel's placement, and a census — TEST INFRASTRUCTURE ONLY (no tests in this module; tests/test_assemble_space_cpu.py pins the
census and the model, tests/test_gpu_assemble_space.py feeds the kernel).

k_assemble sees nothing of a picture but its segment table: per (frame, strip) up to `segs` segments of (bits, source word), and
the strips' bit totals.  One workgroup places the segments of `group` consecutive strips into an LDS image of 14,336 bytes that is
laid out against the 16-byte grid of the output address, 2^lanes_log2 lanes of four words per segment, and stores the image.  Its
control flow depends on
    ns, nseg         strips and segments of the workgroup (the last group of a frame may hold fewer strips)
    chunks           ceil(nseg / 256): the placement table holds 256 segments
    lead, img_end    the group's bytes are image bytes [lead, img_end): lead = (output address of its first byte) mod 16
    passes           ceil(img_end / 14336)
    unchecked        img_end + 4 (4 L + 4) <= 14336: the first trip places without range checks
    per segment      nw = ceil(bits / 32) source words, the phase sh = destination bit mod 32, the long loop (nw >= 4 L) and its trips
    the two ends     the first and the last 16-byte unit of the group, whole or byte by byte
all of which this module derives from the oracle alone (frame_coefficients, encode_block_bits' C entry point, the 38-bit slice
header on a strip's first segment): a tile segment is one strip x one tile row (2 bits + 6 blocks per macroblock row, over 4 rows or
the remainder), the run kernel's segments are the pieces of geometry_space.run_plan's runs inside a strip (padded with empty
segments to `segs` per strip), the strip kernel's segment is the strip.  plan_shape restates plan_for's choice of group and
lanes_log2 (m1v_kernels.hip); the GPU tests hold it against m1v_debug_assemble_shape on every case.

place_batch is the byte-level restatement: clear the image, OR each segment at its destination bit, walk the passes and the
chunks, store the units.  It takes `slips`, each one a way the kernel could be subtly wrong; the CPU tests show that every slip
changes the bytes of the case that is there for it (the dropped range check cannot: what it lets through is zero; it shows as
image words touched outside the image, which place_batch reports).

Content is noise in the style of geometry_space.noise (a per-frame amplitude; amplitude 0 = a flat frame), or, where a group must
carry more than a few bits per block, heavy() below, with a per-frame quality as the coarse knob and its density as the fine one
(noise codes 13 to 30 bits per block at ANY quality: the reference's walk stops at the first pair of adjacent non-zero
coefficients).  The parameters below were found on the CPU by searching seeds, densities and qualities with this module's own
census (census() is the search's measure)."""
import collections
import ctypes as C

import numpy as np

import geometry_space as gs

IMAGE_BYTES = 14336          # kAsmImageBytes
CHUNK = 256                  # kAsmChunk
MAX_GROUP = 16               # kAsmMaxGroup
GROUPS = (1, 2, 4, 8, 16)
LANES_LOG2 = (1, 2, 3, 4)
GUARD = 256                  # guard bytes on either side of the output in the pool (a multiple of 16)
POISON = 0xA5
FIRST = 23                   # frame index of frame 0 of the first batch

# A scene: one geometry with its content; `shapes` the (group, lanes_log2) pairs it runs under, 0 = the plan's own.
# amp, quality: one value per frame (quality None = the encoder's).  path "runs" forces a 3-channel encoder to the run kernels.
Scene = collections.namedtuple("Scene", "name W H channels qf path n seed amp quality shapes why mode", defaults=("full",))
ALL_SHAPES = tuple((g, k) for g in GROUPS for k in LANES_LOG2)
# The macroblock of fewest bits an RGB picture can make: flat (0, 88, 0) at quality 1, every DC level 1: 2 + 6 x 5 = 32 bits (a luma
# block costs 5 bits at level 0 or 1, a chroma block 5 at level 1 and 4 at level 0, but Cb and Cr at level 0 need a green so
# bright that the luma level is 2 or more; a search of the colour cube finds nothing below 32)
LEAST = ("flat", (0, 88, 0))
LEAST_QUALITY, LEAST_MACROBLOCK_BITS = 1, 32

H = "heavy"
SCENES = (
    # a, b, c, f: every shape on the tile producer; 17 strips = groups of 16 + 1, 8 + 8 + 1, ...; five tile rows (4, 4, 4, 4, 1
    # macroblock rows); a noise frame (15 words per segment) and heavy frames of about 40, 67 and 134 words per segment
    Scene("tiles-sweep", 272, 272, 3, 90, None, 4, 1, (256, (H, 256), (H, 256), (H, 256)), (12, 50, 75, 90), ((0, 0),) + ALL_SHAPES,
          "every shape; groups of fewer strips; passes at every group size; long segments for every L"),
    # a: the run kernel's table (258 blocks per strip, runs of 256: three segments per strip, of which some are empty)
    Scene("runs-sweep", 256, 688, 3, 90, "runs", 3, 2, (256, (H, 200), (H, 256)), (12, 60, 90), ((0, 0),) + ALL_SHAPES,
          "every shape on the run kernel's segments; zero-bit segments"),
    # a: the strip kernel's table (54 blocks per strip, one segment per strip)
    # (its last frame: the shortest strip there is, 38 + 9 x 32 bits)
    Scene("strips-sweep", 272, 144, 4, 90, None, 4, 3, (256, (H, 128), (H, 256), LEAST), (12, 75, 90, LEAST_QUALITY), ((0, 0),) + ALL_SHAPES,
          "every shape on the strip kernel's segments; the shortest strip"),
    # d: 16 strips x 17 tile rows = 272 segments under group 16; one pass at quality 4, two at quality 12
    Scene("chunks-2", 256, 1088, 3, 12, None, 2, 4, (256, 256), (4, 12), ((16, 0), (16, 1)),
          "two chunks with one pass and with two"),
    # d: 16 strips x 33 tile rows = 528 segments under group 16; a gentle frame (one pass) and a noise frame
    Scene("chunks-3", 256, 2064, 3, 12, None, 2, 5, (6, 256), (2, 12), ((16, 0),),
          "three chunks with one pass and with several"),
    # e: what the plan reaches with no hook: one strip of 257 tile rows
    Scene("plan-alone", 16, 16400, 3, 12, None, 2, 6, (256, 256), (4, 12), ((0, 0),),
          "two chunks, and two passes, by the plan alone"),
    # g: groups of 4 strips x 29 macroblock rows whose bytes end in and just below the window of the range checks; a strip's last
    # segment is one macroblock row, shorter than 4 L words for L = 16, so that its idle lanes reach behind the group's end
    Scene("window", 256, 464, 3, 90, None, 4, 7, ((H, 206), (H, 212), (H, 216), (H, 218)), (90, 90, 90, 90), ((4, 4), (4, 3), (4, 2), (4, 1)),
          "single-pass workgroups with and without range checks"),
    # b, h, i: one macroblock per frame; flat frames of one macroblock row: groups inside one 16-byte unit
    Scene("one-macroblock", 16, 16, 3, 12, None, 7, 8, (256,) * 7, None, ((0, 0),), "a one-macroblock picture"),
    Scene("flat-row", 256, 16, 3, 12, None, 3, 9, (0, 0, 256), None, ((1, 0), (2, 0), (0, 0)),
          "groups that begin and end inside one 16-byte unit"),
    # i: five macroblock rows = tile rows of 4 and 1: the last segment of a strip of the flat frame is one macroblock, 32 bits
    Scene("flat-short", 256, 80, 3, 12, None, 2, 10, (LEAST, 256), (LEAST_QUALITY, 12), ((0, 0), (1, 0)),
          "the shortest tile segment: one macroblock of 32 bits, exactly one word"),
    # b: 19 strips: last groups of 3 strips behind groups of 4, 8 and 16
    Scene("short-group", 304, 64, 3, 12, None, 2, 11, (256, 256), None, ((0, 0), (4, 0), (8, 0), (16, 0)),
          "a last workgroup of 1 < ns < group strips, ns no power of two"),
)
ALIGN_SCENE = "tiles-sweep"     # out at each of the 16 byte alignments (tests/test_gpu_assemble_space.py)
HARDEST = ("chunks-2", (16, 1))  # >= 2 passes x 2 chunks x long segments (L = 2: every segment of 8 words or more is long)
WINDOW = ("window", (4, 4))


def scene(name):
    return next(s for s in SCENES if s.name == name)


# ---- the plan, restated -----------------------------------------------------------------------------------------------------
def geometry(sc):
    sh = gs.shape(sc.W, sc.H, sc.mode)
    bps = 6 * sh["n_mbrows"]
    if sc.channels == 3 and sc.path != "runs":
        producer, T, segs = "tiles", 0, sh["tile_rows"]
    else:
        rp = gs.run_plan(sh["n_strips"], sh["n_mbrows"])
        producer, T = rp["producer"], rp["T"]
        segs = -(-bps // T) + 1 if producer == "dense" else 1
    return dict(n_strips=sh["n_strips"], n_mbrows=sh["n_mbrows"], bps=bps, producer=producer, T=T, segs=segs)


def plan_shape(sc, forced=(0, 0)):
    """plan_for's (asm_group, asm_lanes_log2, segs, producer) for a scene, with the forced values applied after its own."""
    g = geometry(sc)
    qscale = 1 if sc.qf <= 25 else (2 if sc.qf <= 50 else (4 if sc.qf <= 76 else 8))
    bpb = 22 * qscale
    strip_est = (38 + g["n_mbrows"] * (2 + 6 * bpb)) // 8 + 1
    group = 1
    while group < MAX_GROUP and 2 * group * strip_est * 5 // 4 <= IMAGE_BYTES and 2 * group <= g["n_strips"]:
        group *= 2
    seg_blocks = 24 if g["producer"] == "tiles" else (g["T"] if g["producer"] == "dense" else g["bps"])
    seg_words = seg_blocks * bpb // 32
    lg = 1
    while lg < 4 and (4 << lg) * 5 < seg_words * 8:
        lg += 1
    return (forced[0] or group, forced[1] or lg, g["segs"], g["producer"])


def hook_accepts(sc, group, lg):
    """What m1v_debug_set_assemble_shape takes."""
    return (group == 0 or (group in GROUPS and group <= geometry(sc)["n_strips"])) and 0 <= lg <= 4


# ---- content and segments ---------------------------------------------------------------------------------------------------
_cache = {}


_ZIGZAG = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24,
                    31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56,
                    59, 61, 35, 36, 48, 49, 57, 58, 62, 63])        # zigzag index of raster position r
HEAVY_QUALITY, HEAVY_LEVELS = 90, 8


def heavy(orc, seed, H, W, density):
    """A grey picture [H, W] that loads the block coder.  Noise codes almost nothing (the reference's walk stops at the first pair
    of adjacent non-zero coefficients: tests/hard_content.py), so every 8x8 block here is the inverse DCT of ISOLATED
    coefficients: each even zigzag position 2..62 is lit with probability density / 256, at a level of 1..8 (either sign) times
    the divisor of quality 90 there, over a DC of 128.  All positions lit code about 265 bits per luma block at quality 90, 130 at
    75, 76 at 50 and 21 at 25 (the levels quantise away): the per-frame quality is the coarse knob, the density the fine one.
    The choices come from geometry_space's counter generator."""
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    b = gs._bytes(seed, nby * nbx * 64).reshape(nby, nbx, 2, 32).astype(np.int32)
    div = orc.scale_qmatrix(HEAVY_QUALITY).astype(np.float64)       # raster order
    lit = b[:, :, 0, :31] < density
    level = 1 + (b[:, :, 1, :31] >> 1) % HEAVY_LEVELS
    sign = np.where(b[:, :, 1, :31] & 1, -1, 1)
    pos = np.argsort(_ZIGZAG)[np.arange(2, 64, 2)]                  # raster positions of the even zigzag indices
    c = np.zeros((nby, nbx, 64))
    c[:, :, pos] = np.where(lit, sign * (level + 0.5) * div[pos], 0)
    c[:, :, 0] = 1024
    k = np.arange(8)
    D = np.sqrt(2 / 8) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    D[0] /= np.sqrt(2)
    px = np.einsum("ui,abuv,vj->abij", D, c.reshape(nby, nbx, 8, 8), D)
    return np.clip(np.rint(px), 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8)[:H, :W]


def pixels(orc, sc, batch=0):
    """Packed frames [n, H, W, channels] of a scene's batch (read-only).  Per frame, by the scene's `amp`: noise of that amplitude;
    0 = flat grey of a level that depends on the frame; ("flat", (r, g, b)) = that colour (alpha 255); ("heavy", density) = heavy()
    in R, G and B (alpha, where there is one, is noise)."""
    key = ("px", sc.name, batch)
    if key not in _cache:
        out = np.empty((sc.n, sc.H, sc.W, sc.channels), np.uint8)
        for f in range(sc.n):
            seed = (sc.seed * 64 + batch) * 64 + f
            if isinstance(sc.amp[f], tuple) and sc.amp[f][0] == "flat":
                out[f] = 255
                out[f, :, :, :3] = sc.amp[f][1]
            elif isinstance(sc.amp[f], tuple):
                out[f] = gs.noise(seed + 32, (sc.H, sc.W, sc.channels))
                out[f, :, :, :3] = heavy(orc, seed, sc.H, sc.W, sc.amp[f][1])[:, :, None]
            elif sc.amp[f]:
                out[f] = gs.noise(seed, (sc.H, sc.W, sc.channels), sc.amp[f])
            else:
                out[f] = 40 + 50 * f + 7 * batch
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _omode(orc, sc):
    return orc.MODE_FULL if sc.mode == "full" else orc.MODE_STRICT


def qualities(sc):
    return [sc.qf] * sc.n if sc.quality is None else list(sc.quality)


def record(orc, sc, f, batch=0):
    """The oracle's record of frame f of a batch, as frame FIRST + 100 * batch + f."""
    key = ("rec", sc.name, batch, f)
    if key not in _cache:
        _cache[key] = orc.encode_frame(pixels(orc, sc, batch)[f], sc.W, sc.H, FIRST + 100 * batch + f, qualities(sc)[f], _omode(orc, sc),
                                       channels=sc.channels)
    return _cache[key]


def block_ranges(g, s):
    """The blocks [lo, hi) of strip s that each of its `segs` segments holds (empty ranges pad the run kernel's)."""
    bps = g["bps"]
    if g["producer"] == "tiles":
        return [(24 * t, min(24 * t + 24, bps)) for t in range(g["segs"])]
    if g["producer"] == "strips":
        return [(0, bps)]
    T = g["T"]
    w_lo, w_hi = s * bps // T, ((s + 1) * bps - 1) // T
    out = []
    for q in range(g["segs"]):
        w = w_lo + q
        out.append((max(w * T, s * bps) - s * bps, min((w + 1) * T, (s + 1) * bps) - s * bps) if w <= w_hi else (0, 0))
    return out


def segments(orc, sc, f, batch=0, px=None):
    """[strip][segment] = (bits, value): the segment's bits as an integer of `bits` bits, from the oracle's coefficients and its
    block coder.  The slice header rides on a strip's first block, the two macroblock bits on a macroblock's first block.
    px: frames of the caller's own in place of the scene's content (not cached)."""
    key = ("seg", sc.name, batch, f)
    if px is None and key in _cache:
        return _cache[key]
    g = geometry(sc)
    L = orc.lib()
    zz = orc.frame_coefficients((pixels(orc, sc, batch) if px is None else px)[f], sc.W, sc.H, qualities(sc)[f], _omode(orc, sc),
                                channels=sc.channels)
    zz = np.ascontiguousarray(zz, np.int32)
    base = zz.ctypes.data
    i32p = C.POINTER(C.c_int32)
    out = []
    for s in range(g["n_strips"]):
        strip = []
        for lo, hi in block_ranges(g, s):
            b = orc.OrcBits()
            L.orc_bits_init(C.byref(b))
            for k in range(lo, hi):
                if k == 0:                       # the 38 bits of the slice header (mpeg1_slice)
                    L.orc_bits_put(C.byref(b), 0x000001, 24)
                    L.orc_bits_put(C.byref(b), (s + 1) & 0xff, 8)
                    L.orc_bits_put(C.byref(b), 1, 5)
                    L.orc_bits_put(C.byref(b), 0, 1)
                if k % 6 == 0:
                    L.orc_bits_put(C.byref(b), 0x3, 2)
                rc = L.orc_encode_block(int(k % 6 < 4), C.cast(base + 256 * (s * g["bps"] + k), i32p), C.byref(b))
                assert rc == 0, (sc.name, f, s, k, rc)
            nb = int(b.nbits)
            raw = C.string_at(b.buf, (nb + 7) // 8) if nb else b""
            L.orc_bits_free(C.byref(b))
            strip.append((nb, int.from_bytes(raw, "big") >> ((-nb) % 8) if nb else 0))
        out.append(strip)
    if px is None:
        _cache[key] = out
    return out


def source_words(bits, value):
    """A segment as the encode kernels leave it in the scratch: big-endian words from a word boundary, zero bits behind."""
    nw = (bits + 31) // 32
    v = value << (32 * nw - bits)
    return [(v >> (32 * (nw - 1 - i))) & 0xffffffff for i in range(nw)]


# ---- the workgroups of a batch ----------------------------------------------------------------------------------------------
class Workgroup:
    """What k_assemble's workgroup (frame f, group index x) derives, with the kernel's conditions restated literally."""

    def __init__(self, f, x, segs_f, group, lg, T, A0):
        n_strips = len(segs_f)
        self.f, self.x, self.group, self.lg, self.L, self.T = f, x, group, lg, 1 << lg, T
        self.s0 = x * group
        self.ns = min(group, n_strips - self.s0)
        self.nseg = self.ns * T
        self.chunks = -(-self.nseg // CHUNK)
        self.seg = [segs_f[self.s0 + j][t] for j in range(self.ns) for t in range(T)]      # q = j * T + t
        strip_bits = [sum(b for b, _ in segs_f[self.s0 + j]) for j in range(self.ns)]
        self.pad = [((-strip_bits[q // T]) & 7) if q % T == T - 1 else 0 for q in range(self.nseg)]
        self.group_bytes = sum((b + 7) >> 3 for b in strip_bits)
        self.A0 = A0                                              # output address of the group's first byte
        self.lead = A0 & 15
        self.img_end = self.lead + self.group_bytes
        self.passes = -(-self.img_end // IMAGE_BYTES)
        self.unchecked = self.img_end + 4 * (4 * self.L + 4) <= IMAGE_BYTES
        self.dest, at = [], 0                                     # destination bit from the group's first byte
        for q in range(self.nseg):
            self.dest.append(at)
            at += self.seg[q][0] + self.pad[q]
        assert at == 8 * self.group_bytes
        self.nw = [(b + 31) >> 5 for b, _ in self.seg]
        self.sh = [(d + 8 * self.lead) & 31 for d in self.dest]
        self.long = [nw >= 4 * self.L for nw in self.nw]
        self.trips = [(nw - 4 * self.L) // (4 * self.L) + 1 if nw >= 4 * self.L else 0 for nw in self.nw]

    def in_window(self):
        """A single pass whose first trip is range-checked: img_end in the 16 (L + 1) bytes below the image's end."""
        return self.passes == 1 and not self.unchecked

    def below_window(self):
        """Unchecked, with img_end in the 16 (L + 1) bytes directly below the window."""
        return self.unchecked and self.img_end + 2 * 16 * (self.L + 1) > IMAGE_BYTES

    def boundary_in_segment(self):
        """Segments that hold a pass boundary strictly inside their bits."""
        out = []
        for p in range(1, self.passes):
            P = 8 * (p * IMAGE_BYTES - self.lead)
            out += [q for q in range(self.nseg) if self.dest[q] < P < self.dest[q] + self.seg[q][0]]
        return out

    def boundary_beside_shared_word(self):
        """Pairs (q, q + 1) of non-empty segments whose shared word (the junction is not on a word boundary of the image) is the last
        word of a pass or the first of the next.  (Passes begin on word boundaries of the image, so a pass boundary cannot fall
        INSIDE a word: this is the nearest thing, the shared word that one pass stores and the next must not touch.)"""
        out = []
        for p in range(1, self.passes):
            w = p * IMAGE_BYTES // 4
            for q in range(self.nseg - 1):
                J = self.dest[q] + self.seg[q][0] + 8 * self.lead     # image bit where q ends
                if self.seg[q][0] and self.seg[q + 1][0] and not self.pad[q] and J & 31 and J >> 5 in (w - 1, w):
                    out.append(q)
        return out

    def classes(self):
        return (f"ns={self.ns} nseg={self.nseg} chunks={self.chunks} lead={self.lead} img_end={self.img_end} passes={self.passes} "
                f"unchecked={int(self.unchecked)} L={self.L} long={sum(self.long)} max_nw={max(self.nw)}")


def workgroups(orc, sc, shape, align=0, batch=0, px=None):
    """Every workgroup of a batch under a shape (group, lanes_log2, both resolved), the output `align` bytes off a 16-byte
    boundary; and the batch's bytes.  px: frames of the caller's own in place of the scene's content."""
    group, lg = shape
    g = geometry(sc)
    out, fo = [], 0
    for f in range(sc.n):
        segs_f = segments(orc, sc, f, batch, px)
        B0 = 0
        for x in range(-(-g["n_strips"] // group)):
            wg = Workgroup(f, x, segs_f, group, lg, g["segs"], align + fo + 44 + B0)
            out.append(wg)
            B0 += wg.group_bytes
        fo += 48 + B0
    return out, fo


# ---- the byte-level restatement ---------------------------------------------------------------------------------------------
SLIPS = ("store-not-or", "no-padding", "carry-kept-over-pass", "carry-lost-at-chunk", "long-loop-stops-early", "no-range-check",
         "lead-ignored", "first-unit-whole", "last-unit-whole")


def _alignbit(p, c, sh):
    return (((p << 32) | c) >> sh) & 0xffffffff


def place_workgroup(wg, pool, slips=()):
    """k_assemble's steps 2 and 3 for one workgroup, into `pool` (a bytearray whose byte 0 lies on a 16-byte boundary; wg.A0 counts
    from it).  Returns the image words outside [0, capacity) that a scatter touched (none, unless a slip is in force)."""
    L, T, cap_words = wg.L, wg.T, IMAGE_BYTES // 4
    lead_placed = 0 if "lead-ignored" in slips else wg.lead
    a_lo = wg.A0 & ~15
    outside = set()
    words = [source_words(*s) for s in wg.seg]
    pad = [0] * wg.nseg if "no-padding" in slips else wg.pad
    carry = 0
    # the slip drops the check where the kernel needs it in a single pass: in the window below the image's end
    check = not wg.unchecked and not ("no-range-check" in slips and wg.passes == 1)
    for pass0 in range(0, wg.img_end, IMAGE_BYTES):
        pass_bytes = min(IMAGE_BYTES, wg.img_end - pass0)
        word0, capw = pass0 >> 2, (pass_bytes + 3) >> 2
        img = [0] * cap_words
        if pass0 != 0 and "carry-kept-over-pass" not in slips:
            carry = 0

        def put(k, o, check):
            if check:
                if o == 0 or not 0 <= k < capw:
                    return
            elif not 0 <= k < cap_words:
                outside.add(k)
                return
            img[k] = o if "store-not-or" in slips else img[k] | o

        for c0 in range(0, wg.nseg, CHUNK):
            if c0 != 0 and "carry-lost-at-chunk" in slips:
                carry = 0
            cnt = min(CHUNK, wg.nseg - c0)
            place = []                                     # scan_chunk: destination bit of every segment of the chunk
            for q in range(c0, c0 + cnt):
                place.append(carry)
                carry += wg.seg[q][0] + pad[q]
            for e in range(cnt):
                q = c0 + e
                src, nw = words[q], wg.nw[q]
                d = place[e] + 8 * lead_placed
                sh, k00 = d & 31, (d >> 5) - word0
                if check and (k00 + max(nw + 1, 4 * L) <= 0 or k00 >= capw):
                    continue                               # (a shortcut of the model: the checked scatter drops all of it)
                word = lambda i: src[i] if 0 <= i < nw else 0
                for i in range(4 * L):                     # the first trip: lane `sub` holds words 4 sub .. 4 sub + 3
                    put(k00 + i, _alignbit(word(i - 1), word(i), sh), check)
                for w0 in range(0, 4 * L, 4):              # the long loop of the lane that holds words w0 ..
                    w = w0 + 4 * L
                    while (w < nw) if "long-loop-stops-early" in slips else (w <= nw):
                        for i in range(w, w + 4):
                            put(k00 + i, _alignbit(word(i - 1), word(i), sh), True)
                        w += 4 * L
        # ---- 3. the image leaves ----
        raw = b"".join(x.to_bytes(4, "big") for x in img)
        for k in range((pass_bytes + 15) >> 4):
            ib = pass0 + 16 * k
            at = a_lo + ib
            whole = ib >= wg.lead and ib + 16 <= wg.img_end
            if ("first-unit-whole" in slips and ib <= wg.lead < ib + 16) or ("last-unit-whole" in slips and ib < wg.img_end < ib + 16):
                whole = True
            if whole:
                pool[at:at + 16] = raw[16 * k:16 * k + 16]
            else:
                for b in range(16):
                    if wg.lead <= ib + b < wg.img_end:
                        pool[at + b] = raw[16 * k + b]
    return outside


def place_batch(orc, sc, shape, align=0, batch=0, slips=(), only=None):
    """The pool after a batch: GUARD poison bytes (and `align` more), the records, poison.  The headers and trailers are the
    oracle's and are written first (the kernel writes them beside the groups; a slip that spills over them loses).  `only`: a set
    of (f, x) the slips apply to (default: every workgroup).  Returns (pool, total, touched outside the image)."""
    wgs, total = workgroups(orc, sc, shape, align, batch)
    pool = bytearray([POISON]) * (GUARD + 16 + total + GUARD + 16)
    at = GUARD + align
    for f in range(sc.n):
        rec = record(orc, sc, f, batch)
        pool[at:at + 44] = rec[:44]
        pool[at + len(rec) - 4:at + len(rec)] = rec[-4:]
        at += len(rec)
    assert at == GUARD + align + total, (at, total)
    outside = set()
    for wg in wgs:
        wg_pool = Workgroup.__new__(Workgroup)
        wg_pool.__dict__.update(wg.__dict__)
        wg_pool.A0 = wg.A0 + GUARD                        # (GUARD is a multiple of 16: the same lead)
        use = slips if only is None or (wg.f, wg.x) in only else ()
        outside |= {(wg.f, wg.x, k) for k in place_workgroup(wg_pool, pool, use)}
    return pool, total, outside


def expected_pool(orc, sc, align=0, batch=0):
    recs = b"".join(record(orc, sc, f, batch) for f in range(sc.n))
    pool = bytearray([POISON]) * (GUARD + 16 + len(recs) + GUARD + 16)
    pool[GUARD + align:GUARD + align + len(recs)] = recs
    return pool, len(recs)


# ---- naming a difference ----------------------------------------------------------------------------------------------------
def describe_difference(orc, sc, shape, got, align=0, batch=0):
    """Text for a failed comparison: got = the output bytes [0, total) as the device left them.  Names the frame, the workgroup,
    its classes, and the strip and segment of the first differing byte."""
    wgs, total = workgroups(orc, sc, shape, align, batch)
    want = b"".join(record(orc, sc, f, batch) for f in range(sc.n))
    at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
    head = f"{sc.name} {sc.W}x{sc.H} shape {shape} align {align} batch {batch}"
    if at is None:
        return f"{head}: equal over {min(len(got), len(want))} bytes; lengths {len(got)} / {len(want)}"
    for wg in wgs:
        lo = wg.A0 - align
        if lo <= at < lo + wg.group_bytes:
            bit = 8 * (at - lo)
            q = max(k for k in range(wg.nseg) if wg.dest[k] <= bit)
            return (f"{head}: first difference at byte {at} (got {got[at]:#04x}, want {want[at]:#04x}): frame {wg.f}, workgroup "
                    f"{wg.x} ({wg.classes()}), strip {wg.s0 + q // wg.T}, segment {q % wg.T} (q = {q}, chunk {q // CHUNK}, "
                    f"nw = {wg.nw[q]}, sh = {wg.sh[q]}, bit {bit - wg.dest[q]} of its {wg.seg[q][0]}), pass {(at - lo + wg.lead) // IMAGE_BYTES}")
    f = next(k for k in range(sc.n) if sum(len(record(orc, sc, j, batch)) for j in range(k + 1)) > at)
    return f"{head}: first difference at byte {at}, in the header or trailer of frame {f}"


# ---- census -----------------------------------------------------------------------------------------------------------------
def cases():
    """Every (scene, forced shape) the sweep runs."""
    return [(sc, forced) for sc in SCENES for forced in sc.shapes]


def case_id(sc, forced):
    return f"{sc.name}-g{forced[0]}-l{forced[1]}"


def _cls(n):
    return "1" if n == 1 else ("2" if n == 2 else ">=3")


def census(orc):
    """{item: {class: sorted list}} over every case, output 16-byte aligned, first batch."""
    c = collections.defaultdict(lambda: collections.defaultdict(set))
    rows = []
    for sc, forced in cases():
        group, lg, segs, producer = plan_shape(sc, forced)
        assert hook_accepts(sc, *forced), (sc.name, forced)
        wgs, total = workgroups(orc, sc, (group, lg))
        cid = case_id(sc, forced)
        L = 1 << lg
        c["a. shapes (group, lanes_log2) by producer"][producer].add((group, lg))
        if forced == (0, 0):
            c["a. shapes (group, lanes_log2) by producer"][producer + ", the plan's own"].add((group, lg))
        rows.append((cid, producer, group, lg, segs, len(wgs), total, sorted({w.passes for w in wgs}), sorted({w.chunks for w in wgs}),
                     sum(w.in_window() for w in wgs), sum(sum(w.long) for w in wgs)))
        for w in wgs:
            if w.ns < w.group:
                c["b. group sizes"]["ns < group: (ns, group)"].add((w.ns, w.group))
            if sc.W == 16 and sc.H == 16:
                c["b. group sizes"]["one-macroblock picture: (ns, nseg)"].add((w.ns, w.nseg))
            c["c. passes"]["passes"].add(_cls(w.passes))
            if w.group >= 4 and w.boundary_in_segment():
                c["c. passes"]["group >= 4, a pass boundary inside a segment: groups"].add(w.group)
            if w.group >= 4 and w.boundary_beside_shared_word():
                c["c. passes"]["group >= 4, a pass boundary beside a word two segments share: cases"].add(cid)
            c["d. (chunks, passes)"]["pairs"].add((_cls(w.chunks), "1" if w.passes == 1 else ">=2"))
            if forced == (0, 0) and w.chunks >= 2:
                c["e. by the plan alone"]["several chunks: scenes"].add(sc.name)
            if forced == (0, 0) and w.passes >= 2:
                c["e. by the plan alone"]["several passes: scenes"].add(sc.name)
            for q in range(w.nseg):
                bits, nw, sh = w.seg[q][0], w.nw[q], w.sh[q]
                if nw in (4 * L - 1, 4 * L, 4 * L + 1):
                    c["f. long segments"][f"L={L}: nw among 4L-1, 4L, 4L+1"].add(nw)
                if nw >= 8 * L:
                    c["f. long segments"][f"L={L}: two trips or more (nw >= 8L): trips"].add(w.trips[q])
                if nw:
                    c["f. long segments"][f"L={L}: phases of the first trip"].add(sh)
                if w.long[q]:
                    c["f. long segments"][f"L={L}: phases in the long loop"].add(sh)
                if bits and bits % 32 == 0:
                    c["f. long segments"]["bits a multiple of 32: (bits, long)"].add((bits, w.long[q]))
                c["i. short segments"][f"{producer}: fewest bits"].add(bits)
                if bits == 0:
                    c["i. short segments"][f"{producer}: zero-bit segments"].add(True)
            if w.in_window():
                c["g. range checks"][f"L={L}: single pass, checked (img_end)"].add(w.img_end)
            if w.below_window():
                c["g. range checks"][f"L={L}: unchecked directly below the window (img_end)"].add(w.img_end)
            c["h. edges"]["lead"].add(w.lead)
            c["h. edges"]["img_end mod 16"].add(w.img_end % 16)
            if w.lead and w.img_end < 16:
                c["h. edges"]["begins and ends inside one unit: (lead, img_end)"].add((w.lead, w.img_end))
            if w.img_end % 16 == 0:
                c["h. edges"]["ends exactly on a unit: cases"].add(cid)
    out = {k: {kk: sorted(vv) for kk, vv in v.items()} for k, v in c.items()}
    for producer in ("tiles", "dense", "strips"):
        fewest = out["i. short segments"][f"{producer}: fewest bits"]
        out["i. short segments"][f"{producer}: fewest bits"] = fewest[:1]
        out["i. short segments"].setdefault(f"{producer}: zero-bit segments", [False])
    return out, rows


def census_text(orc):
    out, rows = census(orc)
    lines = ["# Census of the placement space of k_assemble: census_text() of tests/assemble_space.py, written by the command in",
             "# profiles/README.md and read, never written, by tests/test_assemble_space_cpu.py.",
             "# A case is a scene under a forced shape (g0 / l0 = the plan's own).  Classes are those of the workgroups (frame, group)",
             "# with the output on a 16-byte boundary, first batch.  L = 2^lanes_log2 lanes of four words per segment; the LDS image",
             f"# holds {IMAGE_BYTES} bytes, the placement table {CHUNK} segments.",
             "== cases: id, producer, group, lanes_log2, segs, workgroups, bytes, passes, chunks, workgroups in the window, long segments =="]
    lines += [f"  {' '.join(str(x).replace(' ', '') for x in r)}" for r in rows]
    for item in sorted(out):
        lines.append(f"== {item} ==")
        for k in sorted(out[item]):
            v = out[item][k]
            shown = v if len(v) <= 40 else v[:20] + ["..."] + v[-5:]
            lines.append(f"  {k}: {len(v)} -> {' '.join(str(x).replace(' ', '') for x in shown)}")
    return "\n".join(lines) + "\n"
