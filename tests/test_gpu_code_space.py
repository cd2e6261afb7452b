"""GPU tests of the entropy stage over the whole code space (-m gpu): every entry of the run/level table, every (run, level)
pair a block of samples reaches as its first coded pair, both signs, 20- and 28-bit escapes, and every DC level 0..2042 — the
content of tests/code_space.py, whose census tests/test_code_space_cpu.py pins — through each kernel family: encodes on the tile
path, the run kernels, RGBA, a pitched BGRA surface and NV12 / I420 planes, the global-memory fallback of the tile kernels, and
the size table, the rd table and the frame_sizes probe of the table kernels.  The families are those of tests/input_families.py:

  rgb, rgb-runs, rgba, surface-4-bgr-gap, planes-nv12, planes-i420   k_*_tiles, the run kernels, k_*_rgba, k_*_surface, k_*_planes
  rgbplanes-pitched                  k_*_rgb_planes     (encodes, tables)
  float16-, float32-window           k_*_float_planes   (encodes; float32 the fallback; bfloat16-window the tables): patterns
                                     whose byte under the rule is the grey picture's, so the census is the pinned one
  yuy2                               k_*_step2          (encodes, fallback, tables)
  kt-planes-nv12, kt-surface-4-bgr-gap   kt_*_planes (encodes), kt_*_surface (tables): frames behind a frame table
  kp-planes-i420, kp-planes-nv12     kp_*_planes        (encodes and fallback; tables): planes behind a plane table

Every comparison is for equality with the CPU oracle (tests/plane_oracle.py for planes, tests/rd_oracle.py for the distortion)
and every status word is 0.  A set's frames carry one quality each and are encoded with per-frame quality, ten frames to a call;
the narrow set (qualities <= 76) goes on an encoder of quality 76, so that the byte-staged kernels run, the wide set and the DC
frames on one of quality 92.  A failure names the first differing frame and, from the census, the block whose bits differ first
by its DC level and first (r, L): a wrong table entry reads as an entry.  All frames are 352x288; the oracle's records are cached
per module."""
import numpy as np
import pytest

import code_space as cs
import input_families as fam
import plane_oracle
import rd_oracle as rd
from test_gpu_rd_table import _rd
from test_gpu_size_table import _table
from test_gpu_surface import _encode

pytestmark = pytest.mark.gpu

W, H = cs.W, cs.H
FIRST = 17
BATCH = 10
SETS = ("narrow", "wide", "dc")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- content and the oracle's answers, once per module ----------------------------------------------------------------------
_cache = {}


def _frames(orc, name, kind):
    """The frames of a set for an input kind: "rgb" and "rgba" take the grey pictures, "planes" the planes."""
    form = "planes" if kind == "planes" else "grey"
    return cs.dc_frames(orc, form) if name == "dc" else cs.ac_frames(orc, name, form)


def _pixels(orc, name, kind):
    """Packed pixels [n, H, W, channels] of a set; alpha is noise."""
    key = ("px", name, kind)
    if key not in _cache:
        px = _frames(orc, name, kind)["rgb"]
        if kind == "rgba":
            rng = np.random.default_rng(len(name))
            px = np.ascontiguousarray(np.concatenate([px, rng.integers(0, 256, px.shape[:3] + (1,), dtype=np.uint8)], -1))
        _cache[key] = px
    return _cache[key]


_PLANE_LAYOUT = dict(y_offset=0, cb_offset=W * H, cr_offset=W * H + W * H // 4, y_pitch=W, c_pitch=W // 2, c_step=1,
                     frame_stride=W * H * 3 // 2)


def _record(orc, name, kind, f, q):
    """The oracle's record of frame f of a set at quality q as frame FIRST + f."""
    key = ("rec", name, kind, f, q)
    if key not in _cache:
        if kind == "planes":
            fr = _frames(orc, name, kind)
            frame = np.concatenate([fr[p][f].reshape(-1) for p in ("Y", "Cb", "Cr")])
            _cache[key] = plane_oracle.encode_layout(frame, _PLANE_LAYOUT, W, H, FIRST + f, q, orc.MODE_FULL)
        else:
            px = _pixels(orc, name, kind)
            _cache[key] = orc.encode_frame(px[f], W, H, FIRST + f, q, orc.MODE_FULL, channels=px.shape[-1])
    return _cache[key]


def _distortion(orc, name, kind, f, q):
    key = ("dist", name, kind, f, q)
    if key not in _cache:
        if kind == "planes":
            fr = _frames(orc, name, kind)
            d = rd.divisors_zigzag(orc, q)
            _cache[key] = int(sum(rd.block_distortion(_raw(orc, name, p, f), cs.plane_levels(orc, fr[p][f], q), d).sum()
                                  for p in ("Y", "Cb", "Cr")))
        else:
            px = _pixels(orc, name, kind)
            _cache[key] = rd.frame_distortion(orc, px[f], W, H, q, orc.MODE_FULL, px.shape[-1])
    return _cache[key]


def _raw(orc, name, plane, f):
    """The raw coefficients of one plane of a frame: its levels at quality 100, where every divisor is 1."""
    key = ("raw", name, plane, f)
    if key not in _cache:
        _cache[key] = cs.plane_levels(orc, _frames(orc, name, "planes")[plane][f], 100)
    return _cache[key]


class _Case:
    """One encoder (at most BATCH frames a call) on one input family with all frames of one set on the device.
    family: a family of tests/input_families.py, which builds the encoder and its input; the planes- families, the sample
    presets and their table twins take the planes of a set, every other family its grey pictures."""

    def __init__(self, torch, orc, family, name):
        self.torch, self.orc, self.family, self.name = torch, orc, family, name
        self.Q = cs.TOP["narrow"] if name == "narrow" else cs.TOP["wide"]
        base = fam.base_family(family)[1]
        if fam.content_form(family) == "planes":
            fr = _frames(orc, name, "planes")
            content = dict(planes=(fr["Y"].copy(), fr["Cb"].copy(), fr["Cr"].copy()))           # (the sets are read-only)
        else:
            content = dict(pixels=_pixels(orc, name, "rgba" if base == "rgba" or base.startswith("surface-4-") else "rgb"))
        self.input = fam.build(torch, family, W, H, "full", self.Q, BATCH, float_range=fam.FLOAT_RANGES[SETS.index(name) % 2], **content)
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        self.frames = _frames(orc, name, self.kind)
        self.qualities = self.frames["qualities"]
        self.n = len(self.qualities)
        assert max(self.qualities) <= self.Q

    def batches(self):
        return [(a, min(a + BATCH, self.n)) for a in range(0, self.n, BATCH)]

    def groups(self):
        """(first frame, end) of each run of frames of one quality, at most BATCH frames each."""
        out, a = [], 0
        for f in range(1, self.n + 1):
            if f == self.n or self.qualities[f] != self.qualities[a] or f - a == BATCH:
                out.append((a, f))
                a = f
        return out

    def record(self, f, q=None):
        return _record(self.orc, self.name, self.kind, f, self.qualities[f] if q is None else q)

    def check_encode(self, a, b, what):
        """Frames a..b - 1 at their own qualities in one call: bytes and sizes are the oracle's."""
        want = [self.record(f) for f in range(a, b)]
        got, sizes = _encode(self.torch, self.enc, self.dev[a:b], FIRST + a, quality=self.qualities[a:b])
        if got == b"".join(want) and sizes == [len(r) for r in want]:
            return
        at = 0
        for i, f in enumerate(range(a, b)):
            mine = got[at:at + sizes[i]]
            at += sizes[i]
            if mine != want[i]:
                pytest.fail(f"{self.family}, {self.name} set, {what}: "
                            + cs.describe_difference(self.orc, self.frames, f, mine, want[i]))
        pytest.fail(f"{self.family}, {self.name} set, {what}: {len(got)} bytes for sizes {sizes}")

    def fail_number(self, what, f, q, got, want):
        pytest.fail(f"{self.family}, {self.name} set, {what} at quality {q}: {got} != {want} (oracle) for "
                    + cs.describe_frame(self.orc, self.frames, f, q))

    def close(self):
        self.enc.close()


# ---- 1. encodes -------------------------------------------------------------------------------------------------------------
ENCODE_FAMILIES = ["rgb", "rgb-runs", "rgba", "surface-4-bgr-gap", "planes-nv12", "planes-i420",
                   "rgbplanes-pitched", "float16-window", "float32-window", "yuy2", "kt-planes-nv12", "kp-planes-i420"]
FALLBACK_FAMILIES = ["rgb", "surface-4-bgr-gap", "planes-nv12", "planes-i420", "float32-window", "yuy2", "kp-planes-i420"]


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", ENCODE_FAMILIES)
def test_encode_matches_the_oracle(torch_cuda, orc, family, name):
    """Per-frame quality batches of a set: packed RGB on the tile path and forced to the run kernels, RGBA, a pitched BGRA
    surface with a gap between the frames, NV12 and I420 planes."""
    case = _Case(torch_cuda, orc, family, name)
    for a, b in case.batches():
        case.check_encode(a, b, "encode")
    case.close()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", FALLBACK_FAMILIES)
def test_global_memory_fallback_matches_the_oracle(torch_cuda, orc, family, name):
    """The same batches with an 8-word LDS image and the worst-case arena reserved, which sends every unit through the
    global-memory fallback (as test_encode_per_frame_quality_and_probe does); then once more with the hooks off."""
    case = _Case(torch_cuda, orc, family, name)
    case.enc.debug_set_lds_words(8)
    case.enc.reserve_scratch(True)
    for a, b in case.batches():
        case.check_encode(a, b, "encode through the global-memory fallback")
    case.enc.debug_set_lds_words(0)
    case.enc.reserve_scratch(False)
    a, b = case.batches()[0]
    case.check_encode(a, b, "encode after the fallback")
    case.close()


# ---- 2. tables --------------------------------------------------------------------------------------------------------------
TABLE_FAMILIES = ["rgb", "rgba", "surface-4-bgr-gap", "planes-nv12",      # one per table kernel
                  "yuy2", "rgbplanes-pitched", "bfloat16-window", "kt-surface-4-bgr-gap", "kp-planes-nv12"]


def _probe(torch, enc, dev, qs):
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    sizes = enc.frame_sizes(dev, quality=qs, status=st)
    enc.flush()
    torch.cuda.synchronize()
    assert int(st.cpu()[0]) == 0
    return [int(s) for s in sizes.cpu()]


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", TABLE_FAMILIES)
def test_tables_match_the_oracle(torch_cuda, orc, family, name):
    """A frame is encodable at its own quality q and below: each run of frames of one quality is asked for (20, 50, q) —
    the narrow kernel for q <= 76, the wide one above.  frame_size_table, frame_rd_table (sizes and exact distortion) and
    frame_sizes give the oracle's numbers."""
    torch = torch_cuda
    case = _Case(torch, orc, family, name)
    for a, b in case.groups():
        quals = tuple(sorted({20, 50, case.qualities[a]}))
        dev = case.dev[a:b]
        want = [[len(case.record(f, q)) for f in range(a, b)] for q in quals]
        table, status = _table(torch, case.enc, dev, quals)
        assert status == [0] * len(quals), (family, name, quals, status)
        sizes, dist, status = _rd(torch, case.enc, dev, quals)
        assert status == [0] * len(quals), (family, name, quals, status)
        for k, q in enumerate(quals):
            probe = _probe(torch, case.enc, dev, [q] * (b - a))
            for i, f in enumerate(range(a, b)):
                for what, got in (("frame_size_table", table[k][i]), ("frame_rd_table size", sizes[k][i]), ("frame_sizes", probe[i])):
                    if got != want[k][i]:
                        case.fail_number(what, f, q, got, want[k][i])
                d = _distortion(orc, name, case.kind, f, q)
                if dist[k][i] != d:
                    case.fail_number("frame_rd_table distortion", f, q, dist[k][i], d)
    case.close()
