"""GPU tests of the entropy stage over the whole code space (-m gpu): every entry of the run/level table, every (run, level)
pair a block of samples reaches as its first coded pair, both signs, 20- and 28-bit escapes, and every DC level 0..2042 — the
content of tests/code_space.py, whose census tests/test_code_space_cpu.py pins — through each kernel family: encodes on the tile
path, the run kernels, RGBA, a pitched BGRA surface and NV12 / I420 planes, the global-memory fallback of the tile kernels, and
the size table, the rd table and the frame_sizes probe of the four table kernels.

Every comparison is for equality with the CPU oracle (tests/plane_oracle.py for planes, tests/rd_oracle.py for the distortion)
and every status word is 0.  A set's frames carry one quality each and are encoded with per-frame quality, ten frames to a call;
the narrow set (qualities <= 76) goes on an encoder of quality 76, so that the byte-staged kernels run, the wide set and the DC
frames on one of quality 92.  A failure names the first differing frame and, from the census, the block whose bits differ first
by its DC level and first (r, L): a wrong table entry reads as an entry.  All frames are 352x288; the oracle's records are cached
per module."""
import numpy as np
import pytest

import code_space as cs
import plane_oracle
import rd_oracle as rd
from test_gpu_planes import _buffer, _layout, _plane_encoder, _view, _write_planes
from test_gpu_rd_table import _rd
from test_gpu_size_table import _table
from test_gpu_surface import _encode, _surface, _surface_encoder

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
    family: "rgb" | "rgb-runs" | "rgba" (packed) | "surface-<channels>-<order>-<layout>" | "planes-<layout>"."""

    def __init__(self, torch, orc, family, name):
        from ec504_imageencoder_amd import Mpeg1Encoder
        self.torch, self.orc, self.family, self.name = torch, orc, family, name
        self.Q = cs.TOP["narrow"] if name == "narrow" else cs.TOP["wide"]
        if family.startswith("planes-"):
            self.kind = "planes"
            fr = _frames(orc, name, "planes")
            n = len(fr["qualities"])
            lay, base = _layout(family.split("-")[1], W, H)
            buf = _buffer(torch, n, lay, base, fill_seed=len(family))
            _write_planes(torch, buf, lay, base, fr["Y"].copy(), fr["Cb"].copy(), fr["Cr"].copy())     # (the sets are read-only)
            self.enc = _plane_encoder(W, H, self.Q, "full", BATCH, lay)
            self.dev = _view(torch, buf, n, lay, base, self.enc)
            self.keep = buf
        elif family.startswith("surface-"):
            _, channels, order, layout = family.split("-")
            self.kind = "rgb" if channels == "3" else "rgba"
            self.dev, pitch, stride = _surface(torch, _pixels(orc, name, self.kind), layout, order, fill_seed=len(family))
            self.enc = _surface_encoder(W, H, self.Q, "full", int(channels), BATCH, pitch, stride, order)
        else:
            self.kind = "rgba" if family == "rgba" else "rgb"
            px = _pixels(orc, name, self.kind)
            self.dev = torch.from_numpy(px.copy()).cuda()
            self.enc = Mpeg1Encoder(W, H, self.Q, "full", channels=px.shape[-1], max_frames=BATCH)
            if family == "rgb-runs":
                self.enc.debug_set_path("runs")
                assert self.enc.path == "runs" and self.enc.size_table_fused == 0
            else:                                 # README: 3 channels on the tile path and 4 channels always take the fused pass
                assert self.enc.path == ("tiles" if family == "rgb" else "runs") and self.enc.size_table_fused == 1
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
ENCODE_FAMILIES = ["rgb", "rgb-runs", "rgba", "surface-4-bgr-gap", "planes-nv12", "planes-i420"]
FALLBACK_FAMILIES = ["rgb", "surface-4-bgr-gap", "planes-nv12", "planes-i420"]


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
TABLE_FAMILIES = ["rgb", "rgba", "surface-4-bgr-gap", "planes-nv12"]     # one per table kernel


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
