"""The picture shapes that walk the address arithmetic of the tile-shaped kernels and of the run kernels, and a census of them —
TEST INFRASTRUCTURE ONLY (no tests in this module; tests/test_geometry_space_cpu.py pins the census and the content,
tests/test_gpu_geometry.py feeds the kernels).

tests/code_space.py enumerates what a block can code; this module enumerates where a block can lie.  Five sets of sizes:

  tile     64 sizes.  For grid (a, b) in ((0, 0), (1, 1)), s in 1..8, m in 1..4, k the running index 0..63:
               W = 16 (8 a + s) + (7 k mod 16),   H = 16 (4 b + m) + (5 k mod 16)
           A tile is 8 strips x 4 macroblock rows: grid (0, 0) is one partial tile, grid (1, 1) a 2 x 2 grid of tiles whose last
           column holds s strips and whose last row holds m macroblock rows.  Every (strips_here, mrows_here) pair in both grids,
           every residue of W and of H mod 16 four times each; no size beyond 271 x 143.  The 32 members with even k have an even
           height: those are compared with the real reference (odd heights are outside its behaviour: DESIGN.md).
  batch    the tile-set member of grid (1, 1), s = 3, m = 1 (184 x 88) in batches of 7, 8, 9, 16 and 17 frames on an encoder of
           max_frames = 17: the workgroup-to-(frame, tile) map takes frames in groups of 8 and the n % 8 others on another branch.
  run      n_mbrows in (9, 10, 11, 13, 21, 42, 43, 48) x n_strips in (1, 2, 5) for the run kernels (4-channel encodes, and
           3 channels forced to them): a strip of fewer than 64 blocks takes k_encode_strips (9, 10), 11 is the first dense one
           (66 blocks per strip, runs of 64), 42 and 43 straddle the 256 blocks from which a run has 256.  The W residues
           (0, 5, 8, 11 in turn) and a buffer offset of 0 or 1 byte select each input mode of the run kernels.
  strict   three sizes from 96 x 144 up, W residues 0, 11 (odd) and 6: the region stays 6 strips x 9 rows, the pitch varies.
  oddw     W in (33, 35, 47) x H in (32, 34).  In the tile set the parities of W and H are the same bit (7 k and 5 k both carry
           the parity of k), so it has no odd width (chroma stride W / 2 rounded down) at an even height, and every odd-width
           member of it is at a height the reference cannot confirm.  These six are odd widths at even heights: the CPU tests
           compare the oracle with the reference there, the GPU tests the device with the oracle.

Families that restrict the size take the nearest size below: surfaces, RGB planes and float planes W & ~1, the 4:2:0 plane
presets and the packed 4:2:2 / P010 sample presets W & ~1 and H & ~1 (the number of strips and macroblock rows stays); a family
behind a frame table (kt-) or a plane table (kp-) inherits the rule of the family behind the prefix.

The content is noise from a counter-based generator written out here (splitmix64 of seed and index: no PIL, no numpy Generator,
nothing of the reference), full range for quality 12 and of amplitude 20 around mid-grey for quality 90.  The census mirrors the
host's plan (plan_for and run_kernel of ec504_imageencoder_amd/csrc/m1v_kernels.hip: fast_ok = 3 channels and W % 8 == 0; input
mode 1 = fast_ok and a 4-byte aligned buffer, 2 = 3 channels aligned otherwise, 3 = 4 channels aligned, 0 = byte loads; the strip
kernel has modes 0 and 1 only)."""
import collections
import hashlib

import numpy as np

TILE_STRIPS, TILE_MBROWS = 8, 4
GRIDS = ((0, 0), (1, 1))
FIRST = 17                                # the frame index of frame 0 of every set
CONTENTS = {"q12": (12, 256), "q90": (90, 20)}      # name: (encoder quality, amplitude of the noise)
TABLE_QUALITIES = {"q12": (1, 12), "q90": (20, 76, 77, 90)}
BATCH_SIZES = (7, 8, 9, 16, 17)
BATCH_MAX = 17
RUN_MBROWS = (9, 10, 11, 13, 21, 42, 43, 48)
RUN_STRIPS = (1, 2, 5)
RUN_RESIDUES = (0, 5, 8, 11)
FRAMES = {"tile": 3, "batch": BATCH_MAX, "run": 2, "strict": 3, "oddw": 3}
ODD_WIDTHS = tuple((W, H) for W in (33, 35, 47) for H in (32, 34))

Member = collections.namedtuple("Member", "set k W H mode grid s m")


# ---- the sets ---------------------------------------------------------------------------------------------------------------
def tile_set():
    out, k = [], 0
    for g, (a, b) in enumerate(GRIDS):
        for s in range(1, TILE_STRIPS + 1):
            for m in range(1, TILE_MBROWS + 1):
                out.append(Member("tile", k, 16 * (TILE_STRIPS * a + s) + 7 * k % 16, 16 * (TILE_MBROWS * b + m) + 5 * k % 16, "full", g, s, m))
                k += 1
    return out


def batch_member():
    return next(t._replace(set="batch") for t in tile_set() if (t.grid, t.s, t.m) == (1, 3, 1))


def run_set():
    out = []
    for rows in RUN_MBROWS:
        for strips in RUN_STRIPS:
            k = len(out)
            W, H = 16 * strips + RUN_RESIDUES[k % 4], 16 * rows + 5 * k % 16
            out.append(Member("run", k, W, H, "full", None, shape(W, H)["strips_here"], shape(W, H)["mrows_here"]))
    return out


def strict_set():
    return [Member("strict", k, W, H, "strict", 0, 6, 1) for k, (W, H) in enumerate(((96, 144), (107, 149), (118, 160)))]


def odd_width_set():
    return [Member("oddw", k, W, H, "full", 0, W // 16, H // 16) for k, (W, H) in enumerate(ODD_WIDTHS)]


def all_members():
    return tile_set() + [batch_member()] + run_set() + strict_set() + odd_width_set()


def name(t):
    return f"{t.set}:{t.W}x{t.H}"


def restricted(t, family):
    """The member at the nearest size below that the family takes; a family behind a frame table (kt-) or a plane table (kp-)
    takes what the family behind the prefix takes."""
    if family.startswith(("kt-", "kp-")):
        family = family[3:]
    if family.startswith(("surface-", "rgbplanes-", "float16-", "bfloat16-", "float32-")):
        return t._replace(W=t.W & ~1)
    if family in ("planes-i420", "planes-nv12", "planes-yv12", "planes-nv21", "yuy2", "uyvy", "p010"):
        return t._replace(W=t.W & ~1, H=t.H & ~1)
    return t


def shape(W, H, mode="full"):
    """What the kernels make of a size: strips and macroblock rows of the coded region, the tile grid and its remainders."""
    strips, rows = (W // 16, H // 16) if mode == "full" else (6, 9)
    cols, trows = -(-strips // TILE_STRIPS), -(-rows // TILE_MBROWS)
    return dict(n_strips=strips, n_mbrows=rows, tile_cols=cols, tile_rows=trows,
                strips_here=strips - TILE_STRIPS * (cols - 1), mrows_here=rows - TILE_MBROWS * (trows - 1))


def run_plan(n_strips, n_mbrows):
    """The run kernels' plan for a geometry: producer, run length T, units per frame, blocks of the last (short) run."""
    bps = 6 * n_mbrows
    if bps < 64:
        return dict(producer="strips", bps=bps, T=64, units=n_strips, rem=0)
    T = 256 if bps >= 256 else bps // 64 * 64
    return dict(producer="dense", bps=bps, T=T, units=-(-n_strips * bps // T), rem=n_strips * bps % T)


def input_mode(channels, W, offset, producer):
    """The input mode run_kernel picks for a packed buffer `offset` bytes off a 4-byte boundary."""
    aligned = offset % 4 == 0
    fast = channels == 3 and W % 8 == 0 and aligned
    if producer == "strips":
        return 1 if fast else 0
    return 1 if fast else (2 if aligned and channels == 3 else (3 if aligned else 0))


# ---- content ----------------------------------------------------------------------------------------------------------------
def _bytes(seed, count):
    """count bytes: the top byte of splitmix64(seed * 2^32 + i)."""
    x = np.arange(count, dtype=np.uint64) + np.uint64((seed << 32) & 0xFFFFFFFFFFFFFFFF)
    x = x * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((x ^ (x >> np.uint64(31))) >> np.uint64(56)).astype(np.uint8)


def noise(seed, shape_, amp=256):
    """Noise of a shape: every byte value (amp 256) or 128 - amp / 2 .. 128 + amp / 2 - 1."""
    b = _bytes(seed, int(np.prod(shape_))).reshape(shape_)
    if amp >= 256:
        return b
    return (128 - amp // 2 + ((b.astype(np.uint16) * amp) >> 8)).astype(np.uint8)


def _seed(t, content, part):
    return ((t.W * 4096 + t.H) * 2 + list(CONTENTS).index(content)) * 8 + part


_cache = {}


def pixels(t, content, channels=3, n=None):
    """Packed frames [n, H, W, channels] of a member (read-only): R, G, B noise of the content's amplitude; alpha is full-range
    noise of its own."""
    n_all = FRAMES[t.set]                 # (frame f is the same bytes whatever the number of frames: the generator counts)
    key = ("px", t.W, t.H, content, channels, n_all)
    if key not in _cache:
        px = noise(_seed(t, content, 0), (n_all, t.H, t.W, 3), CONTENTS[content][1])
        if channels == 4:
            px = np.concatenate([px, noise(_seed(t, content, 1), (n_all, t.H, t.W, 1))], -1)
        px = np.ascontiguousarray(px)
        px.setflags(write=False)
        _cache[key] = px
    return _cache[key][:n_all if n is None else n]


def planes(t, content):
    """Independent noise planes of a member's coded region (read-only): Y [n, ye, xe], Cb and Cr [n, ye / 2, xe / 2]."""
    n = FRAMES[t.set]                     # (frame f is the same bytes whatever the number of frames: the generator counts)
    key = ("planes", t.W, t.H, t.mode, content, n)
    if key not in _cache:
        sh, amp = shape(t.W, t.H, t.mode), CONTENTS[content][1]
        xe, ye = 16 * sh["n_strips"], 16 * sh["n_mbrows"]
        out = (noise(_seed(t, content, 2), (n, ye, xe), amp), noise(_seed(t, content, 3), (n, ye // 2, xe // 2), amp),
               noise(_seed(t, content, 4), (n, ye // 2, xe // 2), amp))
        for p in out:
            p.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def tight_layout(t):
    """The layout under which planes(t, ...) of one frame lie behind one another, for tests/plane_oracle.py."""
    sh = shape(t.W, t.H, t.mode)
    xe, ye = 16 * sh["n_strips"], 16 * sh["n_mbrows"]
    return dict(y_offset=0, cb_offset=xe * ye, cr_offset=xe * ye + xe * ye // 4, y_pitch=xe, c_pitch=xe // 2, c_step=1,
                frame_stride=xe * ye * 3 // 2)


def omode(orc, t):
    return orc.MODE_FULL if t.mode == "full" else orc.MODE_STRICT


def record(orc, t, content, f, q=None, channels=3):
    """The oracle's record of packed frame f of a member at quality q (default: the content's) as frame FIRST + f."""
    q = CONTENTS[content][0] if q is None else q
    key = ("rec", t.W, t.H, t.mode, content, channels, f, q)
    if key not in _cache:
        _cache[key] = orc.encode_frame(pixels(t, content, channels, f + 1)[f], t.W, t.H, FIRST + f, q, omode(orc, t), channels=channels)
    return _cache[key]


def plane_record(orc, t, content, f, q=None):
    """plane_oracle's record of frame f of planes(t, content)."""
    import plane_oracle
    q = CONTENTS[content][0] if q is None else q
    key = ("prec", t.W, t.H, t.mode, content, f, q)
    if key not in _cache:
        frame = np.concatenate([p[f].reshape(-1) for p in planes(t, content)])
        # (the region of the tight planes is the member's: a frame of xe x ye has the same strips and rows in either mode)
        _cache[key] = plane_oracle.encode_layout(frame, tight_layout(t), t.W, t.H, FIRST + f, q, omode(orc, t))
    return _cache[key]


def digest(orc, t):
    """{content: SHA-256 over the oracle's records of the member's packed R, G, B frames at the content's quality}."""
    return {c: hashlib.sha256(b"".join(record(orc, t, c, f) for f in range(FRAMES[t.set]))).hexdigest() for c in CONTENTS}


# ---- census -----------------------------------------------------------------------------------------------------------------
RESTRICTIONS = (("any size (rgb, rgb-fallback, rgba, planes-reference, planes-odd)", "rgb"),
                ("W even (surface-*)", "surface-"),
                ("W and H even (planes-i420, planes-nv12)", "planes-i420"))


def census():
    """Per set, the classes that are hit: {set: {class: sorted list}}.  The tile set once per size restriction."""
    out = {}
    for label, family in RESTRICTIONS:
        c = collections.defaultdict(set)
        for t0 in tile_set():
            t = restricted(t0, family)
            sh = shape(t.W, t.H)
            assert (sh["strips_here"], sh["mrows_here"], sh["tile_cols"]) == (t.s, t.m, t.grid + 1)
            c["(strips_here, mrows_here, grid)"].add((sh["strips_here"], sh["mrows_here"], t.grid))
            c["W mod 16"].add(t.W % 16)
            c["H mod 16"].add(t.H % 16)
            c["W parity"].add(t.W % 2)
            c["H parity"].add(t.H % 2)
            c["3 W mod 16"].add(3 * t.W % 16)
            if t.s % 2:
                c["odd strips_here, by grid"].add((t.s, t.grid))
            c["sizes"].add((t.W, t.H))
        c["(W parity, H parity)"] = {(restricted(t, family).W % 2, restricted(t, family).H % 2) for t in tile_set()}
        if family == "rgb":
            c["number of members with even H (those are compared with the real reference)"] = {sum(t.H % 2 == 0 for t in tile_set())}
        out[f"tile, {label}"] = {k: sorted(v) for k, v in c.items()}
    b = batch_member()
    sh = shape(b.W, b.H)
    out["batch"] = {"size": [(b.W, b.H)], "(strips_here, mrows_here, tiles per frame)": [(sh["strips_here"], sh["mrows_here"], sh["tile_cols"] * sh["tile_rows"])],
                    "(n, n mod 8, n // 8)": [(n, n % 8, n // 8) for n in BATCH_SIZES], "max_frames": [BATCH_MAX]}
    c = collections.defaultdict(set)
    rows = []
    for t in run_set():
        sh = shape(t.W, t.H)
        p = run_plan(sh["n_strips"], sh["n_mbrows"])
        modes = {(ch, off): input_mode(ch, t.W, off, p["producer"]) for ch in (3, 4) for off in (0, 1)}
        rows.append((t.W, t.H, sh["n_strips"], sh["n_mbrows"], p["producer"], p["bps"], p["T"], p["units"], p["rem"],
                     tuple(modes[k] for k in sorted(modes))))
        c["producer"].add(p["producer"])
        c["T"].add(p["T"])
        for (ch, off), mode in modes.items():
            c["(producer, input mode)"].add((p["producer"], mode))
            if p["producer"] == "dense":
                c["dense input mode"].add(mode)
        c["last run short"].add(p["rem"] != 0)
        c["W mod 16"].add(t.W % 16)
    out["run"] = {k: sorted(v) for k, v in c.items()}
    out["run"]["(W, H, n_strips, n_mbrows, producer, blocks per strip, T, units, (n_strips * bps) mod T, "
               "input modes for (3 ch, +0), (3 ch, +1), (4 ch, +0), (4 ch, +1))"] = rows
    out["strict"] = {"sizes": [(t.W, t.H) for t in strict_set()], "W mod 16": sorted({t.W % 16 for t in strict_set()}),
                     "W parity": sorted({t.W % 2 for t in strict_set()}), "3 W mod 16": sorted({3 * t.W % 16 for t in strict_set()}),
                     "region (strips, macroblock rows)": [(6, 9)]}
    out["oddw"] = {"sizes": [(t.W, t.H) for t in odd_width_set()],
                   "(W parity, H parity)": sorted({(t.W % 2, t.H % 2) for t in odd_width_set()}),
                   "(n_strips, n_mbrows)": sorted({(t.s, t.m) for t in odd_width_set()})}
    return out


def census_text():
    lines = ["# Census of the geometry space (tests/geometry_space.py), written by tests/test_geometry_space_cpu.py.",
             "# A tile is 8 strips x 4 macroblock rows; strips_here / mrows_here are those of the last tile column / row.",
             "# grid 0 = one partial tile, grid 1 = 2 x 2 tiles.  Input modes of the run kernels: 0 byte loads, 1 aligned rows,",
             "# 2 any row offset in an aligned buffer (3 channels), 3 aligned 4-channel pixels; the strip kernel has 0 and 1.",
             "# In the tile set W and H have the same parity (7 k and 5 k carry the parity of k): its odd widths all lie at odd",
             "# heights, where the reference cannot run.  The set oddw holds odd widths at even heights.",
             "# tests/golden/geometry_space.json records a hash for every member at its own size (tile, batch, run, strict, oddw);",
             "# the sizes restricted for surfaces (W & ~1) and for the 4:2:0 presets (W & ~1, H & ~1) have no recorded hash and are",
             "# not run through the reference: the device is compared with the oracle there."]
    for set_name, classes in census().items():
        lines.append(f"== {set_name} ==")
        for k, v in classes.items():
            if k.startswith("(W, H, n_strips"):
                lines.append(f"  {k}:")
                lines += [f"    {row}" for row in v]
            else:
                lines.append(f"  {k}: {len(v)} -> {' '.join(str(x).replace(' ', '') for x in v)}")
    return "\n".join(lines) + "\n"


# ---- naming a difference ----------------------------------------------------------------------------------------------------
def slice_starts(rec, n_strips):
    """Byte offsets of the slices of one record, found by walking the slice start codes 00 00 01 (strip + 1) & 0xff from the
    end of the 44 header bytes (a strip ends on a byte boundary); fewer than n_strips where the walk loses them."""
    out, at = [], 44
    for s in range(n_strips):
        at = rec.find(bytes((0, 0, 1, (s + 1) & 0xff)), at)
        if at < 0:
            break
        out.append(at)
        at += 4
    return out


def slice_starts_backwards(rec, n_strips):
    """The same walk from the record's end (the last occurrence of each code before the next strip's).  Nothing keeps a
    payload from holding 00 00 01 xx; where it holds the code the walk looks for, the two walks differ."""
    out, end = [], len(rec)
    for s in range(n_strips - 1, -1, -1):
        at = rec.rfind(bytes((0, 0, 1, (s + 1) & 0xff)), 44, end)
        if at < 0:
            break
        out.append(at)
        end = at
    return out[::-1]


def describe_difference(got, want, W, H, mode, n):
    """Text for a failed comparison of n frame records: got, want are sequences of n records (bytes).  Names the first
    differing frame, the slice in it (by the start codes of the oracle's record), the strip's tile column and that column's
    strips_here, and whether the difference starts in the 38 bits of the slice header or at a bit offset behind them."""
    assert len(want) == n
    sh = shape(W, H, mode)
    head = (f"{W}x{H} {mode} ({sh['n_strips']} strips x {sh['n_mbrows']} macroblock rows, {sh['tile_cols']} x {sh['tile_rows']} tiles, "
            f"last column {sh['strips_here']} strips, last row {sh['mrows_here']} macroblock rows), {n} frames")
    if len(got) != n:
        return f"{head}: {len(got)} records"
    for f in range(n):
        g, w = got[f], want[f]
        if g == w:
            continue
        m = min(len(g), len(w))
        at = next((i for i in range(44, m) if g[i] != w[i]), None)
        if at is None:
            first = next((i for i in range(m) if g[i] != w[i]), m)
            return f"{head}: frame {f}: first difference at byte {first}, outside the slices; sizes {len(g)} / {len(w)}"
        starts, back = slice_starts(w, sh["n_strips"]), slice_starts_backwards(w, sh["n_strips"])
        i = max((k for k, s in enumerate(starts) if s <= at), default=None)
        if i is None or len(starts) != sh["n_strips"]:
            return f"{head}: frame {f}: first difference at byte {at}; the slice walk found {len(starts)} slices; sizes {len(g)} / {len(w)}"
        if starts != back:                        # a payload holds a start code: say so and do not name a slice
            j = max((k for k, s in enumerate(back) if s <= at), default=0)
            return (f"{head}: frame {f}: first difference at byte {at}; the payload holds a slice start code, so the slice is "
                    f"{min(i, j)}..{max(i, j)} (walks from the front {starts} and from the end {back}); sizes {len(g)} / {len(w)}")
        bit = 8 * (at - starts[i]) + 8 - (g[at] ^ w[at]).bit_length()
        col = i // TILE_STRIPS
        here = min(TILE_STRIPS, sh["n_strips"] - TILE_STRIPS * col)
        where = "in the slice header" if bit < 38 else f"at bit {bit - 38} behind the slice header"
        same = [k for k in range(n) if k != f and g == want[k]]
        swapped = f"; the record is the oracle's for frame {same[0]}" if same else ""
        return (f"{head}: frame {f}, slice {i} (strip {i}, strip {i % TILE_STRIPS} of tile column {col}, which holds {here} strips; "
                f"slice bytes {starts[i]}..{(starts + [len(w) - 4])[i + 1]}): the first difference is {where} (byte {at} of the record); "
                f"sizes {len(g)} / {len(w)}{swapped}")
    return f"{head}: records are equal"


def split(data, sizes):
    """The records of a concatenation, by the sizes the encoder reported."""
    out, at = [], 0
    for s in sizes:
        out.append(data[at:at + s])
        at += s
    return out
