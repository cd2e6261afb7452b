"""Every input layout at the top of its 32-bit in-frame offsets and with frames past 4 GiB — TEST INFRASTRUCTURE ONLY (no tests in
this module; tests/test_address_space_cpu.py pins the cases on the host, tests/test_gpu_address_space.py feeds the kernels).

The setters promise two things about addresses (include/mpeg1_hip.h): byte offsets inside a frame are 32-bit (an extent E below
2^32 is accepted, 2^32 is refused) and the frame stride is 64-bit.  The kernels lean on both: a row's address is a uniform 64-bit
frame base plus a 32-bit offset.  This module places frames so that those offsets and bases take the values nothing else reaches.

The pool.  One allocation of POOL_BYTES (about 10 GiB).  Frame 0 of every case starts at F = pool + FRAME0 = pool + 2^31 + 64 KiB;
the pool ends MARGIN behind F + S_MAX + 2^32, S_MAX the largest frame stride a case uses.  So every plausible 32-bit slip of a
kernel lands inside it and gives wrong bytes, never a fault: an in-frame offset sign-extended from 32 bits reaches down to
F - 2^31; one taken mod 2^31, and a frame base f * stride taken mod 2^32, stay in [F, F + 2^32 + S_MAX).  Every byte the read
contract does not address is fill: byte (a mod 251) of one of two 251-byte patterns that differ in every byte, a being the
byte's distance from the pool's first byte (a prime period, so that addresses 2^31 or 2^32 apart hold different fill).

The cases.  kind x edge x geometry x table mode; n = 2 frames of different content, first_frame_index FIRST.
  kinds       surface-<3|4>-<rgb|bgr>; planes-<preset> (all five); samples-<yuy2|uyvy|p010>; rgbplanes-<rgb|gbr>;
              fplanes-<float16|bfloat16|float32>; fpixels-<dtype>-<3|4>
  geometries  a = 48 x 32 (two macroblock rows, one partial tile); b = 184 x 88 (tests/geometry_space.py's batch member: two tile
              rows, the last of one macroblock row; width and height beyond the coded region), for pitch_top only
  edges       each computed from the setter's own rule (accepts(), the arithmetic of csrc/m1v_runtime.h restated) with the kind's
              alignment (sample size; P010: even pitches, odd offsets):
    pitch_top      offsets ordinary, the row pitch the largest the setter accepts.  YCbCr kinds: the luma pitch; the chroma pitch is
                   the largest that keeps the last chroma row in front of the last luma row (at their own maxima both
                   planes would end in the same bytes), so chroma rows reach up to 2^32 less a luma row
    offset_top     ordinary pitches, the last plane (both chroma components; the plane highest in memory) at the largest accepted
                   offset: the whole plane lies in [2^31, 2^32) and E rounded up to 4 is 2^32 or 2^32 - 4
    cross_31       a pitch such that the addressed bytes of one picture row straddle in-frame offset 2^31 with 8 bytes and more on
                   either side.  Planar YCbCr cannot have a luma row and a chroma row straddle the same offset without sharing
                   bytes, so those kinds have cross_31 (a luma row, by the pitch) and cross_31c (a row of the last chroma plane, by
                   its offset); packed 4:2:2 has both in the one row
    stride_4g_d, stride_4g_0   ordinary in-frame layout, frame stride 2^32 + D and 2^32: frame 1 lies past 4 GiB
    both           pitch_top with the stride 2^32 + D
  table modes "" (the stride kernels), kt (m1v_set_frame_table) and kp (m1v_set_plane_table) where the kind takes one, for the
  in-frame edges; the entries are F + f * stride, so all planes of a frame share one pointer.

The model.  Sparse: the bytes a case writes, as sorted pool offsets and values over fill — no large array.  gather(rule) reads a
case's samples back through an address rule: "exact", or one of the slips above ("sext": the in-frame offset sign-extended from 32
bits, "mod31": taken mod 2^31, "base32": the frame base f * stride taken mod 2^32).  A fifth slip, a limit `lim` = (E rounded up to
4) - 16 computed from E mod 2^32, is not modelled: - 16 in 32 bits gives the same word as in 64, and the fetch side and the read
side of the plane kernels compare with the same limit, so a wrong limit moves which unaddressed bytes a unit over-reads and no
addressed byte (profiles/r30_address_space_mutation.txt)."""
import collections
import math

import numpy as np

import float_planes as fp
import plane_oracle

T31, T32 = 2 ** 31, 2 ** 32
MARGIN = 65536
FRAME0 = T31 + MARGIN                      # F - pool: a multiple of 256
D_BYTES, D_SAMPLES = 13, 20                # the small stride excess: any alignment for byte kinds, whole samples for float kinds
S_MAX = T32 + D_SAMPLES
POOL_BYTES = (FRAME0 + S_MAX + T32 + MARGIN + 4095) // 4096 * 4096
PERIOD = 251
FILLS = ("a", "b")
N, FIRST = 2, 17
GEOMETRIES = {"a": (48, 32), "b": (184, 88)}
Q_BYTE, Q_HALF = 60, 90                    # an encoder quality that stages levels in bytes (<= 76) and one in halfwords
TABLE_NARROW, TABLE_WIDE = (20, 76), (20, 76, 77, 90)
AMPLITUDE = 20                             # noise around mid-grey: codable at every quality used (tests/geometry_space.py's q90)
RULES = ("sext", "mod31", "base32")
PLANE_PRESETS = ("reference", "i420", "yv12", "nv12", "nv21")
SAMPLE_PRESETS = ("yuy2", "uyvy", "p010")
FLOAT_RANGE = {"float16": "unit", "bfloat16": "byte", "float32": "unit"}
SAMPLE_CODE = {"float16": 0, "bfloat16": 1, "float32": 2}
RANGE_CODE = {"unit": 0, "byte": 1}

Kind = collections.namedtuple("Kind", "name family a b")
Case = collections.namedtuple("Case", "kind edge geometry table")
Comp = collections.namedtuple("Comp", "label off pitch step rows cols S")


def kinds():
    out = [Kind(f"surface-{c}-{o}", "surface", c, o) for c in (3, 4) for o in ("rgb", "bgr")]
    out += [Kind(f"planes-{p}", "planes", p, None) for p in PLANE_PRESETS]
    out += [Kind(f"samples-{p}", "samples", p, None) for p in SAMPLE_PRESETS]
    out += [Kind(f"rgbplanes-{o}", "rgb_planes", o, None) for o in ("rgb", "gbr")]
    out += [Kind(f"fplanes-{d}", "float_planes", d, None) for d in fp.KINDS]
    out += [Kind(f"fpixels-{d}-{s}", "float_pixels", d, s) for d in fp.KINDS for s in (3, 4)]
    return out


KIND = {k.name: k for k in kinds()}
YCC = ("planes", "samples")
THREE = ("rgb_planes", "float_planes")
ROWS = ("surface", "float_pixels")


def sample_bytes(kind):
    return fp.BYTES[kind.a] if kind.family in ("float_planes", "float_pixels") else 1


def unit(kind):
    """The alignment the kind's offsets, pitches and stride keep: the sample size; 2 for P010's 16-bit words."""
    return 2 if kind.name == "samples-p010" else sample_bytes(kind)


def content_form(kind):
    return "planes" if kind.family in YCC else "pixels"


def tables(kind):
    """The table modes the kind takes beside the stride kernels."""
    if kind.family in ("float_planes", "float_pixels"):
        return ()
    return ("kt", "kp") if kind.family in ("planes", "rgb_planes") else ("kt",)


def edges(kind):
    out = ["pitch_top"] + (["offset_top"] if kind.family not in ROWS else []) + ["cross_31"]
    if kind.family == "planes" or kind.name == "samples-p010":
        out.append("cross_31c")
    return out + ["stride_4g_d", "stride_4g_0", "both"]


IN_FRAME = ("pitch_top", "offset_top", "cross_31", "cross_31c")


def cases():
    out = []
    for k in kinds():
        out += [Case(k.name, e, "a", "") for e in edges(k)] + [Case(k.name, "pitch_top", "b", "")]
        out += [Case(k.name, e, "a", t) for t in tables(k) for e in edges(k) if e in IN_FRAME]
    return out


def case_id(c):
    return "-".join(x for x in (c.table, c.kind, c.edge, c.geometry) if x)


def region(W, H):
    return W // 16 * 16, H // 16 * 16


# ---- the setters' arithmetic (csrc/m1v_runtime.h: rows_fit, m1v_set_sample_layout, three_planes_fit), restated ----------------
def _preset(kind, W, H):
    """The ordinary layout of a kind: the tight preset, as the C presets give it (no zeros), without the frame stride."""
    S = sample_bytes(kind)
    if kind.family == "surface":
        return dict(row_pitch=W * kind.a + 16, order=kind.b)
    if kind.family == "float_pixels":
        step = kind.b * S
        return dict(row_pitch=W * step + 4 * S, pixel_step=step, order=0 if kind.b == 3 else 1, sample=SAMPLE_CODE[kind.a],
                    range=RANGE_CODE[FLOAT_RANGE[kind.a]])
    if kind.family in THREE:
        at = {"rgb": (0, 1, 2), "bgr": (2, 1, 0), "gbr": (2, 0, 1)}[kind.a if kind.family == "rgb_planes" else "rgb"]
        lay = dict(r_offset=at[0] * W * H * S, g_offset=at[1] * W * H * S, b_offset=at[2] * W * H * S, row_pitch=W * S)
        if kind.family == "float_planes":
            lay.update(sample=SAMPLE_CODE[kind.a], range=RANGE_CODE[FLOAT_RANGE[kind.a]])
        return lay
    if kind.family == "planes":
        luma, p = W * H, kind.a
        if p == "reference":
            return dict(y_offset=0, cb_offset=luma, cr_offset=2 * luma, y_pitch=W, c_pitch=W // 2, y_step=1, c_step=1)
        planar, cr_first = p in ("i420", "yv12"), p in ("yv12", "nv21")
        second = (W // 2) * (H // 2) if planar else 1
        return dict(y_offset=0, cb_offset=luma + (second if cr_first else 0), cr_offset=luma + (0 if cr_first else second), y_pitch=W,
                    c_pitch=W // 2 if planar else W, y_step=1, c_step=1 if planar else 2)
    if kind.a == "p010":
        return dict(y_offset=1, cb_offset=2 * W * H + 1, cr_offset=2 * W * H + 3, y_pitch=2 * W, c_pitch=2 * W, y_step=2, c_step=4)
    y, cb, cr = {"yuy2": (0, 1, 3), "uyvy": (1, 0, 2)}[kind.a]
    return dict(y_offset=y, cb_offset=cb, cr_offset=cr, y_pitch=2 * W, c_pitch=4 * W, y_step=2, c_step=4)


def _row_bytes(kind, W):
    if kind.family == "surface":
        return W * kind.a
    if kind.family == "float_pixels":
        return W * kind.b * sample_bytes(kind)
    return W * sample_bytes(kind)


def _ycc_rows(lay, W, H):
    """(bytes up to the last addressed luma byte from y_offset, the same of a chroma plane from its offset)"""
    xe, ye = region(W, H)
    return ((ye - 1) * lay["y_pitch"] + (xe - 1) * lay["y_step"] + 1, (ye // 2 - 1) * lay["c_pitch"] + (xe // 2 - 1) * lay["c_step"] + 1)


def _three_offsets(lay):
    return [lay["r_offset"], lay["g_offset"], lay["b_offset"]]


def extent(kind, lay, W, H):
    """E: one past the last byte of a frame the read contract addresses, from the frame's base."""
    if kind.family in ROWS:
        return (H - 1) * lay["row_pitch"] + _row_bytes(kind, W)
    if kind.family in THREE:
        return max(_three_offsets(lay)) + (H - 1) * lay["row_pitch"] + _row_bytes(kind, W)
    y_rows, c_rows = _ycc_rows(lay, W, H)
    return max(lay["y_offset"] + y_rows, max(lay["cb_offset"], lay["cr_offset"]) + c_rows)


def accepts(kind, lay, W, H):
    """Whether the kind's C setter accepts `lay` (its fields with no zeros, frame_stride included) on a W x H 3-channel encoder
    (a surface kind: its own channel count): the checks of csrc/m1v_runtime.h in their order, argument errors of other kinds
    (unknown codes, null pointers) left out."""
    S, row, stride = sample_bytes(kind), _row_bytes(kind, W), lay["frame_stride"]
    if kind.family != "samples" and kind.family != "planes" and W % 2:
        return False
    if kind.family in ROWS:
        pitch = lay["row_pitch"]
        if kind.family == "float_pixels" and (lay["pixel_step"] not in (3 * S, 4 * S) or (pitch | stride) % S):
            return False
        E = (H - 1) * pitch + row
        return pitch >= row and pitch < T32 and E < T32 and stride >= E
    if kind.family in THREE:
        off, pitch = _three_offsets(lay), lay["row_pitch"]
        if any(v % S for v in off + [pitch, stride]) or pitch < row:
            return False
        lo, hi = min(off), max(off)
        if pitch >= T32 or hi >= T32 or hi + (H - 1) * pitch + row >= T32:
            return False
        for a in range(3):
            for b in range(a + 1, 3):
                d = abs(off[a] - off[b])
                q, r = d // pitch, d % pitch
                if (r < row and q <= H - 1) or (pitch - r < row and q + 1 <= H - 1):
                    return False
        return stride >= hi + (H - 1) * pitch + row - lo
    steps = (lay["y_step"], lay["c_step"])
    if steps not in ((1, 1), (1, 2), (2, 4)) or (kind.family == "planes" and lay["c_step"] > 2):
        return False
    if lay["c_step"] == 4 and abs(lay["cb_offset"] - lay["cr_offset"]) > 3:
        return False
    if stride == 0 or lay["y_pitch"] < W * lay["y_step"] or lay["c_pitch"] < W // 2 * lay["c_step"]:
        return False
    if any(lay[k] >= T32 for k in ("y_pitch", "c_pitch", "y_offset", "cb_offset", "cr_offset")):
        return False
    E = extent(kind, lay, W, H)
    return E < T32 and stride >= E


# ---- the edges -----------------------------------------------------------------------------------------------------------------
def _floor_to(x, u):
    return x // u * u


def _straddling_pitch(at, y0, span, u):
    """The pitch p (a multiple of u) with at + y0 * p = 2^31 - d for the d nearest span / 2 that allows one, 8 <= d <= span - 8."""
    for k in range(span):
        for d in (span // 2 + k, span // 2 - k):
            if 8 <= d <= span - 8 and (T31 - d - at) % (y0 * u) == 0:
                return (T31 - d - at) // y0
    raise AssertionError("no straddling pitch")


def layout(case):
    """(lay, bumps): the layout of a case as its setter takes it (every field, no zeros) and, for an edge at a setter's maximum,
    the (field, ...) groups whose members raised by unit(kind) together the setter must refuse."""
    kind, (W, H) = KIND[case.kind], GEOMETRIES[case.geometry]
    u, row, edge = unit(kind), _row_bytes(kind, W), case.edge
    xe, ye = region(W, H)
    lay, bumps = _preset(kind, W, H), []
    top = T32 - 1
    if edge in ("pitch_top", "both"):
        if kind.family in ROWS:
            lay["row_pitch"] = _floor_to((top - row) // (H - 1), u)
            bumps = [("row_pitch",)]
        elif kind.family in THREE:
            lay["row_pitch"] = _floor_to((top - max(_three_offsets(lay)) - row) // (H - 1), u)
            bumps = [("row_pitch",)]
        else:
            # the luma pitch at its maximum; the chroma pitch the largest that keeps the last chroma row in front of the last luma
            # row, which ends with the frame (at their own maxima both planes would end in the same bytes)
            y_row = (xe - 1) * lay["y_step"] + 1
            lay["y_pitch"] = _floor_to((top - lay["y_offset"] - y_row) // (ye - 1), u)
            c_row = (xe // 2 - 1) * lay["c_step"] + 1
            room = lay["y_offset"] + (ye - 1) * lay["y_pitch"] - 16
            lay["c_pitch"] = _floor_to((room - max(lay["cb_offset"], lay["cr_offset"]) - c_row) // (ye // 2 - 1), u)
            bumps = [("y_pitch",)]
    elif edge == "offset_top":
        if kind.family in THREE:
            last = max(("r_offset", "g_offset", "b_offset"), key=lambda k: lay[k])
            lay[last] = _floor_to(top - ((H - 1) * lay["row_pitch"] + row), u)
            bumps = [(last,)]
        else:
            delta = _floor_to(top - _ycc_rows(lay, W, H)[1] - max(lay["cb_offset"], lay["cr_offset"]), u)
            lay["cb_offset"] += delta
            lay["cr_offset"] += delta
            bumps = [("cb_offset", "cr_offset")]
    elif edge == "cross_31":
        if kind.family in YCC:      # a luma row; packed 4:2:2: an even row, whose bytes hold the chroma row y0 / 2 too
            y0 = (ye // 2 + 2) & ~1
            span = (xe - 1) * lay["y_step"] + 1
            lay["y_pitch"] = _straddling_pitch(lay["y_offset"], y0, span, u)
            if kind.name in ("samples-yuy2", "samples-uyvy"):
                lay["c_pitch"] = 2 * lay["y_pitch"]
        else:
            at = min(_three_offsets(lay)) if kind.family in THREE else 0
            lay["row_pitch"] = _straddling_pitch(at, H // 2 + 1, row, u)
    elif edge == "cross_31c":       # row r0 of the chroma plane highest in memory, by both chroma offsets
        r0, c_row = ye // 4 + 1, (xe // 2 - 1) * lay["c_step"] + 1
        d = c_row // 2
        d += (T31 - d - r0 * lay["c_pitch"] - max(lay["cb_offset"], lay["cr_offset"])) % u
        delta = T31 - d - r0 * lay["c_pitch"] - max(lay["cb_offset"], lay["cr_offset"])
        assert delta % u == 0 and 8 <= d <= c_row - 8
        lay["cb_offset"] += delta
        lay["cr_offset"] += delta
    lay["frame_stride"] = T32 + (0 if edge not in ("stride_4g_d", "both") else (D_BYTES if u == 1 else D_SAMPLES))
    return lay, bumps


# ---- addressed samples ---------------------------------------------------------------------------------------------------------
def components(case):
    """The components of a frame: per component the offset of sample (0, 0), the bytes between rows and between samples, its
    rows and samples per row, and the bytes of a sample.  Pixel kinds: R, G, B of the W x H picture; YCbCr kinds: Y, Cb, Cr of
    the coded region."""
    kind, (W, H) = KIND[case.kind], GEOMETRIES[case.geometry]
    lay, S = layout(case)[0], sample_bytes(kind)
    if kind.family in YCC:
        xe, ye = region(W, H)
        return [Comp("Y", lay["y_offset"], lay["y_pitch"], lay["y_step"], ye, xe, 1),
                Comp("Cb", lay["cb_offset"], lay["c_pitch"], lay["c_step"], ye // 2, xe // 2, 1),
                Comp("Cr", lay["cr_offset"], lay["c_pitch"], lay["c_step"], ye // 2, xe // 2, 1)]
    if kind.family in THREE:
        return [Comp(c, lay[f"{c.lower()}_offset"], lay["row_pitch"], S, H, W, S) for c in "RGB"]
    if kind.family == "surface":
        at = (0, 1, 2) if kind.b == "rgb" else (2, 1, 0)
        return [Comp(c, at[i], lay["row_pitch"], kind.a, H, W, 1) for i, c in enumerate("RGB")]
    at = (0, 1, 2) if lay["order"] == 0 else (2, 1, 0)
    return [Comp(c, at[i] * S, lay["row_pitch"], lay["pixel_step"], H, W, S) for i, c in enumerate("RGB")]


def offsets(comp):
    """int64 [rows, cols, S]: the in-frame offset of every byte of a component."""
    r, c, b = np.ogrid[0:comp.rows, 0:comp.cols, 0:comp.S]
    return comp.off + r.astype(np.int64) * comp.pitch + c.astype(np.int64) * comp.step + b


def slipped(case, o, f, rule):
    """The pool offset a kernel with address rule `rule` reads for in-frame offset(s) o of frame f."""
    stride = layout(case)[0]["frame_stride"]
    base = f * stride
    if rule == "sext":
        o = np.where(o >= T31, o - T32, o)
    elif rule == "mod31":
        o = o & (T31 - 1)
    elif rule == "base32":
        base %= T32
    else:
        assert rule == "exact", rule
    return FRAME0 + base + o


def applies(case, rule):
    """Whether a slip can change what a case reads: an offset of 2^31 or more for the two offset rules; a frame base of 2^32 or
    more that the kernels compute themselves (with a table the host does) for base32."""
    if rule == "base32":
        return not case.table
    return any(int(offsets(c).max()) >= T31 for c in components(case))


# ---- content -------------------------------------------------------------------------------------------------------------------
def content(case):
    """The frames of a case, a pure function of it: pixels uint8 [N, H, W, 3], or planes (Y [N, ye, xe], Cb, Cr [N, ye / 2, xe / 2]);
    noise of AMPLITUDE around mid-grey, every frame its own."""
    W, H = GEOMETRIES[case.geometry]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(case)))
    g = np.random.default_rng(seed)
    lo, hi = 128 - AMPLITUDE, 128 + AMPLITUDE
    if content_form(KIND[case.kind]) == "pixels":
        return g.integers(lo, hi, (N, H, W, 3), dtype=np.uint8)
    xe, ye = region(W, H)
    return tuple(g.integers(lo, hi, shape, dtype=np.uint8) for shape in ((N, ye, xe), (N, ye // 2, xe // 2), (N, ye // 2, xe // 2)))


def _round_to(x32, dtype):
    if dtype == "float16":
        return x32.astype(np.float16).view(np.uint16)
    if dtype == "bfloat16":
        w = x32.view(np.uint32)
        return ((w + np.uint32(0x7fff) + ((w >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return x32.view(np.uint32).copy()


def float_bits(byte, dtype, seed):
    """Bit patterns of `dtype` whose byte under the rule of include/mpeg1_hip.h (float_planes.rule_bytes) is `byte`: the byte plus
    a jitter within +-0.49, scaled to the kind's range, where the type resolves it; the type's nearest value to the byte elsewhere."""
    rng = FLOAT_RANGE[dtype]
    scale = fp.SCALE[rng]
    jitter = np.random.default_rng(9000 + seed).uniform(-0.49, 0.49, byte.shape)
    bits = _round_to(((byte.astype(np.float64) + jitter) / scale).astype(np.float32), dtype)
    plain = _round_to((byte.astype(np.float64) / scale).astype(np.float32), dtype)
    bits = np.where(fp.rule_bytes(bits, dtype, rng) == byte, bits, plain)
    assert np.array_equal(fp.rule_bytes(bits, dtype, rng), byte)
    return bits


def component_samples(case, frames):
    """Per component the samples [N, rows, cols] as the memory holds them: bytes, or the bit patterns of float samples."""
    kind = KIND[case.kind]
    if content_form(kind) == "planes":
        return list(frames)
    planes = [np.ascontiguousarray(frames[..., i]) for i in range(3)]
    if sample_bytes(kind) == 1:
        return planes
    return [float_bits(p, kind.a, i) for i, p in enumerate(planes)]


def _bytes_of(samples, S):
    """[..., S] little-endian bytes of samples"""
    if S == 1:
        return samples[..., None].astype(np.uint8)
    return np.ascontiguousarray(samples.astype("<u2" if S == 2 else "<u4")).view(np.uint8).reshape(samples.shape + (S,))


def writes(case):
    """(pool offsets int64 [k], bytes uint8 [k]) of everything the case's frames hold, sorted by offset; no byte twice."""
    comps, samples = components(case), component_samples(case, content(case))
    at, val = [], []
    for comp, s in zip(comps, samples):
        for f in range(N):
            at.append(slipped(case, offsets(comp), f, "exact").reshape(-1))
            val.append(_bytes_of(s[f], comp.S).reshape(-1))
    at, val = np.concatenate(at), np.concatenate(val)
    order = np.argsort(at, kind="stable")
    at, val = at[order], val[order]
    assert np.all(np.diff(at) > 0), f"{case_id(case)}: two samples share a byte"
    assert at[0] >= FRAME0 and at[-1] < POOL_BYTES - MARGIN
    return at, val


def fill_pattern(fill):
    a = np.random.default_rng(251).integers(0, 256, PERIOD, dtype=np.uint8)
    return a if fill == "a" else a ^ np.uint8(0xff)


class Sparse:
    """The pool as a case leaves it: its writes over fill."""

    def __init__(self, case, fill):
        self.at, self.val = writes(case)
        self.pattern = fill_pattern(fill)

    def read(self, at):
        at = np.asarray(at, np.int64)
        assert at.min() >= 0 and at.max() < POOL_BYTES, "a slip leaves the pool"
        k = np.minimum(np.searchsorted(self.at, at), len(self.at) - 1)
        return np.where(self.at[k] == at, self.val[k], self.pattern[at % PERIOD])


def gather(case, model, rule="exact"):
    """What a kernel that addresses by `rule` codes: the case's content form, read from the model."""
    kind = KIND[case.kind]
    out = []
    for comp in components(case):
        raw = np.stack([model.read(slipped(case, offsets(comp), f, rule)) for f in range(N)]).astype(np.uint8)
        if comp.S == 1:
            out.append(raw[..., 0])
        else:
            bits = np.ascontiguousarray(raw).view("<u2" if comp.S == 2 else "<u4")[..., 0]
            out.append(fp.rule_bytes(bits, kind.a, FLOAT_RANGE[kind.a]))
    return tuple(out) if content_form(kind) == "planes" else np.stack(out, -1)


# ---- the oracle's records ------------------------------------------------------------------------------------------------------
def record(orc, case, frames, f, quality, index):
    """The record of frame f at `quality` and frame index `index`; None where the oracle cannot code it."""
    W, H = GEOMETRIES[case.geometry]
    try:
        if content_form(KIND[case.kind]) == "pixels":
            return orc.encode_frame(frames[f], W, H, index, quality, orc.MODE_FULL)
        Y, Cb, Cr = (p[f] for p in frames)
        return plane_oracle.encode_frame(lambda x, y: Y[y:y + 8, x:x + 8], lambda p, x, y: (Cb, Cr)[p][y // 2:y // 2 + 8, x // 2:x // 2 + 8],
                                         W, H, index, quality, orc.MODE_FULL)
    except ValueError:
        return None


def records(orc, case, frames, qualities, first=FIRST):
    """One record per frame: frame f at qualities[f] (or the one quality) and index first + f."""
    qs = [qualities] * N if isinstance(qualities, int) else list(qualities)
    return [record(orc, case, frames, f, qs[f], first + f) for f in range(N)]


def distortion(orc, case, frames, f, quality):
    import hard_content
    import rd_oracle
    W, H = GEOMETRIES[case.geometry]
    if content_form(KIND[case.kind]) == "pixels":
        return rd_oracle.frame_distortion(orc, frames[f], W, H, quality, orc.MODE_FULL)
    d = rd_oracle.divisors_zigzag(orc, quality)
    return int(sum(rd_oracle.block_distortion(hard_content.plane_coefficients(orc, p[f], 100), hard_content.plane_coefficients(orc, p[f], quality), d).sum()
                   for p in frames))


# ---- the census ----------------------------------------------------------------------------------------------------------------
def units(case):
    """Every addressed run of 16 bytes of one row (for a row of samples that do not lie next to one another: 16 bytes from an
    addressed one on), as (component label, first offset from F) with the frame term in: int64 arrays per component."""
    stride = layout(case)[0]["frame_stride"]
    out = {}
    for comp in components(case):
        o = offsets(comp)[:, :, 0]
        span = (comp.cols - 1) * comp.step + comp.S
        starts = o[:, :1] + np.arange(0, max(span - 15, 1))[None, :]
        out[comp.label] = np.concatenate([(f * stride + starts).reshape(-1) for f in range(N)])
    return out


def census(case):
    """What tests/test_address_space_cpu.py holds every case to."""
    lay, _ = layout(case)
    kind, (W, H) = KIND[case.kind], GEOMETRIES[case.geometry]
    us = units(case)
    every = np.concatenate(list(us.values()))
    straddles = {label: bool(np.any((u < T31) & (u + 16 > T31))) for label, u in us.items()}
    in_frame = np.concatenate([offsets(c).reshape(-1) for c in components(case)])
    lo = min(int(slipped(case, in_frame, f, rule).min()) for f in range(N) for rule in ("exact",) + RULES)
    hi = max(int(slipped(case, in_frame, f, rule).max()) for f in range(N) for rule in ("exact",) + RULES)
    return dict(below=bool(np.any(every + 16 <= T31)), above=bool(np.any(every >= T31)), straddles=straddles,
                last_byte=int(in_frame.max()), extent=extent(kind, lay, W, H), frame1=lay["frame_stride"] + int(in_frame.min()),
                slips_inside=MARGIN <= lo and hi + MARGIN <= POOL_BYTES, lowest=lo, highest=hi)


def gcd_plane(offs, S):
    """The plane stride in elements of the [n, C, H, W] view whose channels hold three planes at byte offsets offs, and C."""
    g = 0
    for o in offs:
        g = math.gcd(g, o // S)
    g = g or 1
    return g, max(offs) // S // g + 1
