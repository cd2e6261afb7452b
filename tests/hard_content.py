"""Pictures and planes that load the entropy stage, and a census of what they make it code — TEST INFRASTRUCTURE ONLY (no
tests in this module; tests/test_hard_content_cpu.py pins the census, tests/test_gpu_hard_content.py feeds the kernels).

Noise codes almost nothing: VLC_encode stops at the first pair of adjacent non-zero coefficients (image_processing.c:421), so
a block of noise is its DC size and one or two AC codes.  The generators here build every 8x8 block as the inverse DCT of a few
ISOLATED coefficients (a zero before each), so that the walk goes on: every run length, levels on both sides of every table
row's end (the `in_table` boundary of ac_code), 20-bit escapes, 28-bit escapes (|level| >= 128), blocks of more than 64 and of
more than 128 bits.

  _heavy_picture, _emitted_levels, _ZIGZAG   the generator of tests/test_gpu_parity.py (moved here unchanged)
  extreme_pattern_picture                    the sign patterns of test_extreme_levels_at_the_narrow_staging_boundary
  sweep_picture, plane_sweep                 one isolated coefficient per block, position and level cycling (below)
  coded_pairs, census                        the reference's walk of one zigzag block; of a set of blocks, counted

A DC level of 0 changes the first run (`prev = -1` in block_bits_pass1), so sweep pictures also carry blocks of a few lit
pixels on black.  Such a block never codes an AC level, though: a block of pixel sum S has DC coefficient (S + 16) >> 3, which
quantises to 0 only for S <= 8 * q[0] - 17; no AC basis function exceeds 0.2405 per pixel, so every AC coefficient is below
0.2405 * S < 1.93 * q[0] - 4, and every AC divisor is at least 2 * q[0] - 1 (the matrix has 8 at DC and at least 16 elsewhere).
tests/test_hard_content_cpu.py::test_dc_level_zero_never_codes_an_ac_level searches for a counter-example with the oracle's
own DCT at every quality and finds none; the census condition "blocks with DC level 0 that code an AC level" is therefore
pinned at 0."""
import numpy as np

_ZIGZAG = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24,
                    31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56,
                    59, 61, 35, 36, 48, 49, 57, 58, 62, 63])


def _heavy_picture(rng, W, H, npos, amp, big_fraction=0.0):
    """Grey picture whose every 8x8 block is an inverse DCT of `npos` ISOLATED coefficients (odd zigzag
    positions, so each has run >= 1 and VLC_encode never stops early) of magnitude up to `amp`:
    long code sequences, table codes and 20-bit escapes.  A `big_fraction` of the blocks instead carries
    ONE coefficient of magnitude 400..500 at zigzag position 1 or 3 (level >= 128 at qf 92: 28-bit escape)."""
    from scipy.fft import idctn
    inv = np.argsort(_ZIGZAG)
    pic = np.zeros((H, W, 3), np.uint8)
    for by in range(0, H, 8):
        for bx in range(0, W, 8):
            c = np.zeros(64)
            c[0] = 8 * 128
            if rng.random() < big_fraction:
                c[inv[rng.choice([1, 3])]] = rng.choice([-1, 1]) * rng.uniform(400, 500)
            else:
                pos = rng.choice(np.arange(1, 64, 2), size=npos, replace=False)
                c[inv[pos]] = rng.choice([-1, 1], npos) * rng.uniform(amp * 0.5, amp, npos)
            g = np.clip(np.round(idctn(c.reshape(8, 8), norm="ortho")), 0, 255).astype(np.uint8)
            pic[by:by + 8, bx:bx + 8, :] = g[..., None]
    return pic


def _emitted_levels(z):
    """AC levels VLC_encode actually codes: up to the first non-zero whose predecessor is non-zero."""
    out = []
    for p in range(1, 64):
        if z[p] != 0:
            if z[p - 1] != 0:
                break
            out.append(int(z[p]))
    return out


def _extreme_patterns():
    i, j = np.divmod(np.arange(64), 8)
    pats = []
    for (u, v) in ((0, 4), (4, 0), (4, 4), (0, 1), (1, 0), (7, 7)):
        b = np.cos((2 * i + 1) * u * np.pi / 16) * np.cos((2 * j + 1) * v * np.pi / 16)
        pats += [((b > 0) * 255).astype(np.uint8).reshape(8, 8), ((b < 0) * 255).astype(np.uint8).reshape(8, 8)]
    return pats


def extreme_pattern_picture(rng, W, H):
    """Grey picture whose blocks are, at random, the sign patterns (255 / 0) of the basis functions with the largest
    coefficients and the smallest divisors: the largest levels there are (924 / divisor at zigzag positions 1 and 2)."""
    pats = _extreme_patterns()
    pic = np.zeros((H, W, 3), np.uint8)
    for by in range(0, H, 8):
        for bx in range(0, W, 8):
            pic[by:by + 8, bx:bx + 8, :] = pats[rng.integers(len(pats))][..., None]
    return pic


# ---- the sweep ----------------------------------------------------------------------------------------------------------------
LEVELS = (1, 2, 3, 5, 8, 13, 18, 25, 33, 40, 41, 60, 100, 127, 128, 129, 200, 255)
_DCS = (40, 128, 215)


def _block_unencodable(orc, px, is_luma, divisors):
    """The oracle's verdict on one block of samples at the given divisors (|level| >= 256 in a coded position)."""
    import ctypes as C
    zz = orc.quant_zigzag(orc.fdct(px), divisors)
    bits = orc.OrcBits()
    L = orc.lib()
    L.orc_bits_init(C.byref(bits))
    rc = L.orc_encode_block(int(is_luma), zz.ctypes.data_as(orc._i32p), C.byref(bits))
    L.orc_bits_free(C.byref(bits))
    return rc != 0


def _sweep_plane(orc, rng, w, h, q, is_luma, seen=None, coded_up_to=None):
    """One plane of h x w samples (multiples of 8) by the sweep rule.  Block k (raster order of the plane):
      - one isolated coefficient at zigzag position 2 + k % 62 (run - 1 = 0..61 behind a non-zero DC), whose target level
        walks LEVELS (advancing once more every 62 blocks, so that every position meets every level) with a random sign;
      - every third block a second coefficient of level 1, 2, 3 or 5 at least two positions away;
      - every fifth block ("heavy") up to five more of levels 2 and 3, eleven positions apart and at least two from every
        other: at runs of about ten these are escapes, and the block has more than 64 or 128 bits;
      - over a DC of 40, 128 or 215 in turn where the amplitude fits under it, else over 128;
      - every 29th block instead black with one to three lit pixels (DC level 0 at low qualities, see the module's docstring).
    Amplitudes are (|level| + 1/2) x the divisor of quality q at that position, so that the truncating quantiser lands on
    the target.  A block whose samples would leave 0..255 is scaled down as a whole (its levels shrink, the positions stay);
    a heavy block is clipped instead, as _heavy_picture does (most of its codes survive, with other levels).
    seen(px) is what the oracle sees of the 8x8 samples (the converted luma of a grey RGB block; default: px itself); a
    block it cannot encode at quality `coded_up_to` (default q) is replaced by a flat one."""
    from scipy.fft import idctn
    assert w % 8 == 0 and h % 8 == 0
    inv = np.argsort(_ZIGZAG)
    div = orc.scale_qmatrix(q)
    top = orc.scale_qmatrix(q if coded_up_to is None else coded_up_to)
    plane = np.zeros((h, w), np.uint8)
    k = -1
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            k += 1
            if k % 29 == 28:
                px = np.zeros(64, np.uint8)
                lit = rng.choice(64, size=int(rng.integers(1, 4)), replace=False)
                px[lit] = rng.integers(1, 256, len(lit))
                plane[by:by + 8, bx:bx + 8] = px.reshape(8, 8)
                continue
            p = 2 + k % 62
            level = LEVELS[(k // 62 + k) % len(LEVELS)]
            coded = {p: (level + 0.5) * (-1 if rng.random() < 0.5 else 1)}
            if k % 3 == 2:
                p2 = 2 + (p - 2 + 2 + (k // 3) % 59) % 62
                coded[p2] = ((1, 2, 3, 5)[(k // 3) % 4] + 0.5) * (-1 if rng.random() < 0.5 else 1)
            heavy = k % 5 == 3
            if heavy:
                for j in range(1, 6):
                    pj = 2 + (p - 2 + 11 * j) % 62
                    if all(abs(pj - o) >= 2 for o in coded):
                        coded[pj] = (2 + j % 2 + 0.5) * (-1 if rng.random() < 0.5 else 1)
            c = np.zeros(64)
            for pos, lv in coded.items():
                c[inv[pos]] = lv * div[inv[pos]]
            ac = idctn(c.reshape(8, 8), norm="ortho")
            peak = np.abs(ac).max()
            dc = _DCS[(k // 7) % 3]
            if peak > min(dc, 255 - dc) - 0.5:
                dc = 128
            if peak > 127 and not heavy:
                ac *= 127 / peak
            px = np.clip(np.round(dc + ac), 0, 255).astype(np.uint8)
            if _block_unencodable(orc, px.reshape(64) if seen is None else seen(px), is_luma, top):
                px = np.full((8, 8), dc, np.uint8)
            plane[by:by + 8, bx:bx + 8] = px
    return plane


def sweep_picture(rng, W, H, q, orc=None, coded_up_to=None):
    """Grey R = G = B picture [H, W, 3] whose luma follows the sweep rule (_sweep_plane) with levels aimed at quality q and
    every block encodable at quality `coded_up_to` (default q; divisors shrink as the quality grows, so at every lower one
    too).  The oracle converts a grey pixel to a luma within 1 of it and to chroma 127 or 128: what it sees decides."""
    if orc is None:
        import oracle_ffi as orc

    def seen(px):
        return orc.convert(np.repeat(px.reshape(64, 1), 3, 1))[0]

    luma = _sweep_plane(orc, rng, W, H, q, 1, seen, coded_up_to)
    return np.ascontiguousarray(np.repeat(luma[..., None], 3, 2))


def plane_sweep(rng, W, H, q, orc=None, coded_up_to=None):
    """(Y [H, W], Cb [H / 2, W / 2], Cr [H / 2, W / 2]): three planes built independently by the sweep rule — chroma carries
    hard blocks that no RGB picture maps to."""
    if orc is None:
        import oracle_ffi as orc
    Y = _sweep_plane(orc, rng, W, H, q, 1, None, coded_up_to)
    Cb = _sweep_plane(orc, rng, W // 2, H // 2, q, 0, None, coded_up_to)
    Cr = _sweep_plane(orc, rng, W // 2, H // 2, q, 0, None, coded_up_to)
    return Y, Cb, Cr


def plane_coefficients(orc, plane, q):
    """Zigzag levels [blocks, 64] of every 8x8 block of one plane at quality q (raster order of the plane's blocks)."""
    h, w = plane.shape
    div = orc.scale_qmatrix(q)
    return np.stack([orc.quant_zigzag(orc.fdct(plane[by:by + 8, bx:bx + 8]), div)
                     for by in range(0, h - 7, 8) for bx in range(0, w - 7, 8)])


def plane_encodable(orc, plane, q, is_luma):
    """Whether the oracle codes every 8x8 block of the plane at quality q."""
    div = orc.scale_qmatrix(q)
    h, w = plane.shape
    return not any(_block_unencodable(orc, plane[by:by + 8, bx:bx + 8], is_luma, div)
                   for by in range(0, h - 7, 8) for bx in range(0, w - 7, 8))


def frame_encodable(orc, pic, q):
    H, W = pic.shape[:2]
    try:
        orc.encode_frame(pic, W, H, 0, q, orc.MODE_FULL)
        return True
    except ValueError:
        return False


# ---- what tests/test_gpu_hard_content.py encodes --------------------------------------------------------------------------------
ENCODER_Q = 92
TABLE_NARROW = (20, 50, 76)                       # qualities[-1] <= narrow_q: the narrow (byte-staged) size-table kernel
TABLE_WIDE = (1, 20, 50, 76, 77, 85, 90, 92)      # K = 8 on the wide (int16-staged) kernel
EXTREME_Q = 77                                    # the extreme-pattern frame is coded at 76 and 77 only (924 / 3 = 308 at 92)
_cache = {}


def _first(make, ok, tries=12):
    for _ in range(tries):
        x = make()
        if ok(x):
            return x
    raise AssertionError("no encodable picture in %d draws" % tries)


def hard_frames(orc, W, H):
    """uint8 [4, H, W, 3], built once per size: a sweep picture aimed at quality 92, _heavy_picture(10, 130, 0.4) (the
    quality-92 content of test_long_blocks_and_global_fallback), _heavy_picture(16, 120) (its quality-90 content) — all
    three encodable at ENCODER_Q — and the extreme-pattern picture, encodable up to EXTREME_Q."""
    key = ("rgb", W, H)
    if key not in _cache:
        rng = np.random.default_rng(9200 + W)
        frames = [sweep_picture(rng, W, H, ENCODER_Q, orc),
                  _first(lambda: _heavy_picture(rng, W, H, 10, 130, 0.4), lambda p: frame_encodable(orc, p, ENCODER_Q)),
                  _first(lambda: _heavy_picture(rng, W, H, 16, 120), lambda p: frame_encodable(orc, p, ENCODER_Q)),
                  _first(lambda: extreme_pattern_picture(rng, W, H), lambda p: frame_encodable(orc, p, EXTREME_Q))]
        _cache[key] = np.stack(frames)
        _cache[key].setflags(write=False)
    return _cache[key]


def hard_planes(orc, W, H):
    """(Y [4, H, W], Cb, Cr [4, H / 2, W / 2]), built once per size: plane_sweep aimed at 92; plane_sweep aimed at 76 and kept
    encodable at 92; three independent _heavy_picture(10, 130, 0.4) planes (encodable at ENCODER_Q); three independent
    extreme-pattern planes (encodable up to EXTREME_Q)."""
    key = ("planes", W, H)
    if key not in _cache:
        rng = np.random.default_rng(9300 + W)

        def heavy(w, h, luma):
            return _first(lambda: _heavy_picture(rng, w, h, 10, 130, 0.4)[..., 0], lambda p: plane_encodable(orc, p, ENCODER_Q, luma))

        def extreme(w, h, luma):
            return _first(lambda: extreme_pattern_picture(rng, w, h)[..., 0], lambda p: plane_encodable(orc, p, EXTREME_Q, luma))

        frames = [plane_sweep(rng, W, H, ENCODER_Q, orc), plane_sweep(rng, W, H, 76, orc, coded_up_to=ENCODER_Q),
                  (heavy(W, H, 1), heavy(W // 2, H // 2, 0), heavy(W // 2, H // 2, 0)),
                  (extreme(W, H, 1), extreme(W // 2, H // 2, 0), extreme(W // 2, H // 2, 0))]
        _cache[key] = tuple(np.stack([f[i] for f in frames]) for i in range(3))
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


# ---- the census ---------------------------------------------------------------------------------------------------------------
_code_len = {}
_dc_len = {}


def _dc_bits(orc, is_luma, dc):
    """Bits of the DC part of a block (everything but the AC codes and the end-of-block code)."""
    key = (int(is_luma), int(dc))
    if key not in _dc_len:
        z = np.zeros(64, np.int32)
        z[0] = dc
        rc, s = orc.encode_block_bits(is_luma, z)
        assert rc == 0
        _dc_len[key] = len(s) - 2
    return _dc_len[key]


def _ac_bits(orc, r, level):
    """Bits of the code of (run - 1 = r, level), taken from the oracle: one block that codes exactly that pair."""
    key = (int(r), int(level))
    if key not in _code_len:
        z = np.zeros(64, np.int32)
        if r + 2 <= 63:
            z[0], z[r + 2] = 1, level
        else:
            z[r + 1] = level                   # run 63 exists only behind a DC level of 0
        rc, s = orc.encode_block_bits(1, z)
        assert rc == 0, key
        n = len(s) - 2 - _dc_bits(orc, 1, z[0])
        escape = n in (20, 28)                 # a table code has at most 17 bits
        assert n <= 17 or escape, (key, n)
        assert not escape or s[len(s) - 2 - n:].startswith("000001"), key
        _code_len[key] = n
    return _code_len[key]


def coded_pairs(z):
    """The reference's walk of one zigzag block: [(run - 1, level)] behind the DC, or from position 0 when the DC level is 0,
    up to the first non-zero level without a zero before it."""
    zeros = 0 if z[0] != 0 else 1
    mine = []
    for p in range(1, 64):
        if z[p] == 0:
            zeros += 1
            continue
        if zeros == 0:
            break
        mine.append((zeros - 1, int(z[p])))
        zeros = 0
    return mine


def census(orc, coefficients, is_luma=None):
    """What the reference codes of zigzag blocks [n, 64].  is_luma: one flag for all blocks, or None for the macroblock order
    of orc.frame_coefficients (four luma blocks, then Cb and Cr).  The walk is the reference's: (level, zeros before it)
    pairs behind the DC, or from position 0 when the DC level is 0, up to the first pair without a zero before it.  Every
    block must be encodable.  Returns a dict:
      pairs       [(run - 1, level)] in coding order, over all blocks
      bits        bits per block (orc.encode_block_bits); the walk's own count is asserted equal to it
      esc20       20-bit escapes (out of table, |level| < 128);  esc28: 28-bit escapes (|level| >= 128)
      runs        the set of run - 1 values;  distinct: the set of (run - 1, |level|)
      over64, over128   blocks of more than 64 / 128 bits
      dc0_ac      blocks with DC level 0 that code at least one AC level
      positive, negative   codes of either sign;  max_level: the largest |level| coded"""
    co = np.asarray(coefficients, dtype=np.int32).reshape(-1, 64)
    out = dict(pairs=[], bits=[], esc20=0, esc28=0, runs=set(), distinct=set(), over64=0, over128=0, dc0_ac=0,
               positive=0, negative=0, max_level=0, blocks=len(co))
    for i, z in enumerate(co):
        luma = (i % 6) < 4 if is_luma is None else bool(is_luma)
        rc, s = orc.encode_block_bits(luma, z)
        assert rc == 0, f"census: block {i} is unencodable"
        mine = coded_pairs(z)
        total = _dc_bits(orc, luma, z[0]) + 2
        for r, level in mine:
            n = _ac_bits(orc, r, level)
            total += n
            out["esc20"] += n == 20
            out["esc28"] += n == 28
        assert total == len(s), (i, total, len(s))
        out["pairs"] += mine
        out["bits"].append(len(s))
        out["over64"] += len(s) > 64
        out["over128"] += len(s) > 128
        out["dc0_ac"] += bool(z[0] == 0 and mine)
    for r, level in out["pairs"]:
        out["runs"].add(r)
        out["distinct"].add((r, abs(level)))
        out["positive"] += level > 0
        out["negative"] += level < 0
        out["max_level"] = max(out["max_level"], abs(level))
    return out
