"""The case class, the sets and the cached content and oracle records of the code-space sweep (tests/test_gpu_code_space.py),
which tests/test_gpu_float_pixels_sweeps.py runs with another input.  (That module reads _table through this one, beside the
names defined here.)"""
import numpy as np
import pytest

import code_space as cs
import input_families as fam
import plane_oracle
import rd_oracle as rd
from gpu_calls import _encode, _table

W, H = cs.W, cs.H
FIRST = 17
BATCH = 10
SETS = ("narrow", "wide", "dc")


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
        assert max(self.qualities) <= self.Q, (max(self.qualities), self.Q)

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


def _probe(torch, enc, dev, qs):
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    sizes = enc.frame_sizes(dev, quality=qs, status=st)
    enc.flush()
    torch.cuda.synchronize()
    assert int(st.cpu()[0]) == 0, int(st.cpu()[0])
    return [int(s) for s in sizes.cpu()]
