"""The case class, the tile-set members and the family lists of the geometry sweep (tests/test_gpu_geometry.py), which
tests/test_gpu_float_pixels_sweeps.py runs with another input and tests/test_input_families_cpu.py holds against the code object."""
import numpy as np
import pytest

import geometry_space as gs
import hard_content as hc
import input_families as fam
import rd_oracle as rd
from gpu_calls import _encode, _rd, _table

FIRST = gs.FIRST
TILE_FAMILIES = ["rgb", "rgb-fallback", "rgba", "surface-3-rgb-odd", "surface-4-bgr-gap", "surface-3-bgr-packed",
                 "planes-i420", "planes-nv12", "planes-reference", "planes-odd"] + fam.NEW_FAMILIES
PADDED_FAMILIES = [f for f in TILE_FAMILIES if f.startswith(("surface-", "planes-"))] + fam.NEW_FAMILIES


RUN_FAMILIES = ["rgba", "rgb-runs"]


_dist_cache = {}


def _plane_levels(orc, t, content, f, q):
    key = ("levels", t.W, t.H, t.mode, content, f, q)
    if key not in _dist_cache:
        _dist_cache[key] = [hc.plane_coefficients(orc, p[f], q) for p in gs.planes(t, content)]
    return _dist_cache[key]


def _distortion(orc, t, content, kind, f, q):
    """D(frame f, q) from the oracle: packed frames through rd_oracle.frame_distortion (planes that are the image of the RGB
    frame have its coefficients), independent planes block by block."""
    key = (kind, t.W, t.H, t.mode, content, f, q)
    if key not in _dist_cache:
        if kind == "planes":
            d = rd.divisors_zigzag(orc, q)
            _dist_cache[key] = int(sum(rd.block_distortion(c, lv, d).sum()
                                       for c, lv in zip(_plane_levels(orc, t, content, f, 100), _plane_levels(orc, t, content, f, q))))
        else:
            ch = 4 if kind == "rgba" else 3
            _dist_cache[key] = rd.frame_distortion(orc, gs.pixels(t, content, ch, f + 1)[f], t.W, t.H, q, gs.omode(orc, t), ch)
    return _dist_cache[key]


class _Case:
    """One encoder on one input family with the first n frames of a member's content on the device.
    family: a family of tests/input_families.py, which builds the encoder and its input.
    offset: bytes between a 256-byte boundary and a packed buffer's first byte."""

    def __init__(self, torch, orc, family, t, content, n=None, max_frames=None, fill_seed=None, offset=0):
        self.torch, self.orc, self.family, self.content = torch, orc, family, content
        self.t = t = gs.restricted(t, family)
        self.n = n = gs.FRAMES[t.set] if n is None else n
        self.Q = Q = gs.CONTENTS[content][0]
        cap = n if max_frames is None else max_frames
        W, H = t.W, t.H
        base = fam.base_family(family)[1]
        if fam.content_form(family) == "planes" and base not in ("planes-i420", "planes-nv12"):
            content_ = dict(planes=tuple(p[:n].copy() for p in gs.planes(t, content)))         # (the content is read-only)
        else:                                     # the 4:2:0 presets take the planes of the RGB noise: the oracle's RGB records
            channels = 4 if base == "rgba" else (int(base.split("-")[1]) if base.startswith("surface-") else 3)
            content_ = dict(pixels=gs.pixels(t, content, channels, n).copy())
        self.input = fam.build(torch, family, W, H, t.mode, Q, cap, orc=orc, fill_seed=fill_seed, offset=offset,
                               float_range=fam.FLOAT_RANGES[t.k % 2], **content_)
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        sh = gs.shape(W, H, t.mode)
        assert (self.enc.strips, self.enc.mb_rows) == (sh["n_strips"], sh["n_mbrows"]), (
            (self.enc.strips, self.enc.mb_rows), (sh["n_strips"], sh["n_mbrows"]))

    def where(self, what):
        return f"{self.family}, {gs.name(self.t)}, {self.content} content, {what}"

    def record(self, f, q=None):
        if self.kind == "planes":
            return gs.plane_record(self.orc, self.t, self.content, f, q)
        return gs.record(self.orc, self.t, self.content, f, q, 4 if self.kind == "rgba" else 3)

    def check_records(self, what, got, sizes, want, n=None):
        n = self.n if n is None else n
        if got == b"".join(want) and sizes == [len(r) for r in want]:
            return
        t = self.t
        pytest.fail(self.where(what) + f": sizes {sizes}: " + gs.describe_difference(gs.split(got, sizes), want, t.W, t.H, t.mode, n))

    def check_encode(self, what="encode", quality=None, n=None):
        """Frames 0..n - 1 in one call, at the encoder's quality or one quality per frame: bytes and sizes are the oracle's."""
        n = self.n if n is None else n
        want = [self.record(f, None if quality is None else quality[f]) for f in range(n)]
        got, sizes = _encode(self.torch, self.enc, self.dev[:n], FIRST, quality=quality)
        self.check_records(what, got, sizes, want, n)

    def check_numbers(self, what, got, want):
        if got != want:
            bad = next((k, f) for k in range(len(want)) for f in range(len(want[k])) if got[k][f] != want[k][f])
            sh = gs.shape(self.t.W, self.t.H, self.t.mode)
            pytest.fail(self.where(what) + f": row {bad[0]}, frame {bad[1]}: {got[bad[0]][bad[1]]} != {want[bad[0]][bad[1]]} (oracle); "
                        f"last tile column {sh['strips_here']} strips, last tile row {sh['mrows_here']} macroblock rows of "
                        f"{sh['tile_cols']} x {sh['tile_rows']} tiles; all rows {got} / {want}")

    def check_probe(self, qs, n=None):
        n = self.n if n is None else n
        st = self.torch.full((1,), 0x40, dtype=self.torch.int32, device="cuda")
        sizes = self.enc.frame_sizes(self.dev[:n], quality=qs, status=st)
        self.enc.flush()
        self.torch.cuda.synchronize()
        assert int(st.cpu()[0]) == 0, self.where("frame_sizes status")
        self.check_numbers("frame_sizes", [[int(s) for s in sizes.cpu()]], [[len(self.record(f, q)) for f, q in enumerate(qs)]])

    def check_tables(self, quals, n=None, with_rd=True):
        """frame_size_table and frame_rd_table (sizes and exact distortion) at `quals` on frames 0..n - 1."""
        n = self.n if n is None else n
        dev = self.dev[:n]
        want = [[len(self.record(f, q)) for f in range(n)] for q in quals]
        table, status = _table(self.torch, self.enc, dev, quals)
        assert status == [0] * len(quals), self.where(f"frame_size_table status {status}")
        self.check_numbers(f"frame_size_table{quals}", table, want)
        if with_rd:
            sizes, dist, status = _rd(self.torch, self.enc, dev, quals)
            assert status == [0] * len(quals), self.where(f"frame_rd_table status {status}")
            self.check_numbers(f"frame_rd_table{quals} sizes", sizes, want)
            self.check_numbers(f"frame_rd_table{quals} distortion", dist,
                               [[_distortion(self.orc, self.t, self.content, self.kind, f, q) for f in range(n)] for q in quals])

    def check_coefficients(self):
        got = self.enc.coefficients(self.dev).cpu().numpy().astype(np.int32)
        t = self.t
        for f in range(self.n):
            want = self.orc.frame_coefficients(gs.pixels(t, self.content, 3, f + 1)[f], t.W, t.H, self.Q, gs.omode(self.orc, t))
            if got[f].shape != want.shape or not np.array_equal(got[f], want):
                b = int(np.flatnonzero((got[f] != want).any(1))[0]) if got[f].shape == want.shape else -1
                rows = self.enc.mb_rows
                pytest.fail(self.where("coefficients") + f": frame {f}, first differing block {b} = strip {b // (6 * rows)}, macroblock row "
                            f"{b // 6 % rows}, block {b % 6} of {self.enc.strips} strips x {rows} macroblock rows")

    def check_everything(self):
        """What the family's row of the module's table lists."""
        quals = gs.TABLE_QUALITIES[self.content]
        self.check_encode()
        if self.family == "rgb-fallback":
            return
        if self.family == "rgb":
            qs = [quals[(f + 1) % len(quals)] for f in range(self.n)]
            self.check_encode("encode with per-frame quality", quality=qs)
            self.check_probe(qs)
            self.check_coefficients()
        self.check_tables(quals)

    def close(self):
        self.enc.close()


def _members(grid, m):
    return [t for t in gs.tile_set() if (t.grid, t.m) == (grid, m)]
