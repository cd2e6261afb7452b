"""The case class, the sizes, frame sets and qualities and the cached content and oracle records of the hard-content sweep
(tests/test_gpu_hard_content.py), which the rd table, rd encode and float pixel tests run through their own calls."""
import numpy as np

import hard_content as hc
import input_families as fam
import plane_oracle
import rd_oracle as rd
from gpu_calls import _frames, _table

Q = hc.ENCODER_Q
FIRST = 17
HARD3 = (0, 1, 2)             # sweep, heavy 10/130/0.4, heavy 16/120: encodable at every quality up to Q
HARD4 = (0, 1, 2, 3)          # ... and the extreme-pattern frame, coded at 76 and 77 only


SIZES = [(352, 288), (176, 208)]


_content_cache = {}
_record_cache = {}


def _content(orc, kind, W, H):
    """Seven frames: hard_frames / hard_planes 0..3, then three gentle ones (noise of amplitude 4, 40, 20 around mid-grey).
    kind "rgb": [7, H, W, 3]; "rgba": the same pixels with noise in alpha; "planes": (Y, Cb, Cr)."""
    key = (kind, W, H)
    if key not in _content_cache:
        rng = np.random.default_rng(W + H)
        if kind == "planes":
            Y, Cb, Cr = hc.hard_planes(orc, W, H)
            gentle = [np.concatenate([_frames(rng, 1, w, h, 1, amp)[..., 0] for amp in (4, 40, 20)])
                      for (w, h) in ((W, H), (W // 2, H // 2), (W // 2, H // 2))]
            _content_cache[key] = tuple(np.concatenate([a, g]) for a, g in zip((Y, Cb, Cr), gentle))
        else:
            px = np.concatenate([hc.hard_frames(orc, W, H)] + [_frames(rng, 1, W, H, 3, amp) for amp in (4, 40, 20)])
            if kind == "rgba":
                px = np.concatenate([px, rng.integers(0, 256, px.shape[:3] + (1,), dtype=np.uint8)], -1)
            _content_cache[key] = np.ascontiguousarray(px)
    return _content_cache[key]


def _record(orc, kind, W, H, c, q, index):
    """The oracle's record of content frame c at quality q as frame `index` (raises where the frame is unencodable)."""
    key = (kind, W, H, c, q, index)
    if key not in _record_cache:
        if kind == "planes":
            Y, Cb, Cr = _content(orc, kind, W, H)
            frame = np.concatenate([Y[c].reshape(-1), Cb[c].reshape(-1), Cr[c].reshape(-1)])
            lay = dict(y_offset=0, cb_offset=W * H, cr_offset=W * H + W * H // 4, y_pitch=W, c_pitch=W // 2, c_step=1,
                       frame_stride=frame.size)
            _record_cache[key] = plane_oracle.encode_layout(frame, lay, W, H, index, q, orc.MODE_FULL)
        else:
            px = _content(orc, kind, W, H)
            _record_cache[key] = orc.encode_frame(px[c], W, H, index, q, orc.MODE_FULL, channels=px.shape[-1])
    return _record_cache[key]


class _Case:
    """One encoder of quality Q on one input family with a batch of content frames on the device.
    family: a family of tests/input_families.py, which builds the encoder and its input; the planes- families, the sample
    presets and their table twins take hard_planes, every other family hard_frames."""

    def __init__(self, torch, orc, family, W, H, ids, forced_runs=False):
        self.torch, self.orc, self.W, self.H, self.ids, self.n = torch, orc, W, H, tuple(ids), len(ids)
        sel = list(ids)
        base = fam.base_family(family)[1]
        if fam.content_form(family) == "planes":
            content = dict(planes=tuple(p[sel] for p in _content(orc, "planes", W, H)))
        else:
            content = dict(pixels=_content(orc, "rgba" if base == "rgba" or base.startswith("surface-4-") else "rgb", W, H)[sel])
        self.input = fam.build(torch, family, W, H, "full", Q, self.n, forced_runs=forced_runs, float_range=fam.FLOAT_RANGES[W // 176 % 2],
                               **content)
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        self.buf, self.lay, self.base = self.input.buf, self.input.lay, self.input.base

    def record(self, f, q):
        return _record(self.orc, self.kind, self.W, self.H, self.ids[f], q, FIRST + f)

    def sizes(self, q):
        return [len(self.record(f, q)) for f in range(self.n)]

    def records(self, qs):
        recs = [self.record(f, q) for f, q in enumerate(qs)]
        return b"".join(recs), [len(r) for r in recs]

    def table(self, quals):
        got, status = _table(self.torch, self.enc, self.dev, quals)
        assert status == [0] * len(quals), (quals, status)
        return got

    def probe(self, qs):
        st = self.torch.full((1,), 0x40, dtype=self.torch.int32, device="cuda")
        sizes = self.enc.frame_sizes(self.dev, quality=qs, status=st)
        self.enc.flush()
        self.torch.cuda.synchronize()
        assert int(st.cpu()[0]) == 0, int(st.cpu()[0])
        return [int(s) for s in sizes.cpu()]

    def close(self):
        self.enc.close()


QS_A = (92, 50, 76, 77)
QS_B = (77, 92, 50, 76)


_dist_cache = {}


def _case_dist(orc, case, f, q):
    """D of frame f of a _Case at quality q, from the oracle (cached per content frame)."""
    key = (case.kind, case.W, case.H, case.ids[f], q)
    if key not in _dist_cache:
        W, H = case.W, case.H
        if case.kind == "planes":
            d = rd.divisors_zigzag(orc, q)
            planes = [p[case.ids[f]] for p in _content(orc, "planes", W, H)]
            _dist_cache[key] = int(sum(rd.block_distortion(hc.plane_coefficients(orc, p, 100), hc.plane_coefficients(orc, p, q), d).sum()
                                       for p in planes))
        else:
            px = _content(orc, case.kind, W, H)[case.ids[f]]
            _dist_cache[key] = rd.frame_distortion(orc, px, W, H, q, orc.MODE_FULL, px.shape[-1])
    return _dist_cache[key]
