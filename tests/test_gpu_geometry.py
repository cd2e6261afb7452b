"""GPU tests of the shape-dependent address arithmetic over the whole geometry space (-m gpu): every (strips_here, mrows_here)
pair of a partial tile and of a 2 x 2 tile grid, every residue of W and of H mod 16, batches that take both branches of the
workgroup-to-(frame, tile) map, the run kernels' run lengths, producers and input modes, the strict region under three pitches,
and odd widths at even heights — the sizes of tests/geometry_space.py, whose census, content and oracle records
tests/test_geometry_space_cpu.py pins — through each kernel family:

  rgb                 encode, encode with per-frame quality, frame_sizes, frame_size_table, frame_rd_table, coefficients
  rgb-fallback        encode with an 8-word LDS image and the worst-case arena: every tile goes through the arena
  rgb-runs            (run set) packed RGB forced to the run kernels: encode, frame_sizes, the size table as probes
  rgba                encode on the run kernels (strips or dense by height), the fused size and rd tables
  surface-*           encode, size table, rd table (even W): a pitch one byte over, a gap behind BGRA rows, packed BGR
  planes-i420, -nv12  the tight presets (even W and H), planes that are the image of the RGB noise: the oracle's RGB records
  planes-reference, -odd   independent noise planes against tests/plane_oracle.py
  rgbplanes-pitched, -bgr  k_*_rgb_planes (even W): uint8 NCHW at row pitch W + 13, and tight in plane order B, G, R
  float16-, bfloat16-, float32-window   k_*_float_planes (even W): a window at an odd x0 and an odd pitch of a 4-plane tensor of
                      jitter patterns whose byte under the rule is the RGB noise; range unit / byte by the size index
  yuy2, uyvy, p010    k_*_step2 (even W and H): the tight sample presets, independent noise planes in the addressed bytes
  kt-<family>         kt_*_surface, _planes, _step2, _rgb_planes: surface-4-bgr-gap, surface-3-rgb-packed, planes-nv12,
                      planes-i420, yuy2 and rgbplanes-pitched as frames scattered in a pool behind a frame table (planes-odd
                      too, at the odd widths)
  kp-planes-i420, -nv12, -reference, kp-rgbplanes-pitched   kp_*_planes, kp_*_rgb_planes: every plane at an address of its own
                      behind a plane table, its allocation-visible range exactly the read contract's
Each of the families from rgbplanes- on: encode, size table, rd table.  tests/input_families.py builds every family's input and
names the kernels it reaches; tests/test_input_families_cpu.py holds those names against the code object.

Every comparison is for equality with the CPU oracle (tests/rd_oracle.py for the distortion) and every status word is 0.  The
content is noise, so every block differs from its neighbours (tests/test_geometry_space_cpu.py::test_content_is_position_sensitive):
a re-read strip or macroblock row that reaches a block changes the record.  Each size runs at quality 12 on full-range noise
with tables at (1, 12) and at quality 90 on noise of amplitude 20 with tables at (20, 76, 77, 90): both staging widths.  A
failing comparison of records names the frame, the slice, its tile column and that column's strips (geometry_space.
describe_difference).  The tests do not check where the kernels read; test_padding_does_not_reach_a_block checks that what lies
outside the addressed samples never changes the output."""
import numpy as np
import pytest

import geometry_space as gs
import hard_content as hc
import input_families as fam
import rd_oracle as rd
from test_gpu_rd_table import _rd
from test_gpu_size_table import _table
from test_gpu_surface import _encode

pytestmark = pytest.mark.gpu

FIRST = gs.FIRST
TILE_FAMILIES = ["rgb", "rgb-fallback", "rgba", "surface-3-rgb-odd", "surface-4-bgr-gap", "surface-3-bgr-packed",
                 "planes-i420", "planes-nv12", "planes-reference", "planes-odd"] + fam.NEW_FAMILIES
PADDED_FAMILIES = [f for f in TILE_FAMILIES if f.startswith(("surface-", "planes-"))] + fam.NEW_FAMILIES
BATCH_FAMILIES = ["rgb", "rgba", "surface-4-bgr-gap", "planes-nv12", "float32-window", "yuy2", "kt-planes-nv12", "kp-rgbplanes-pitched"]
RUN_FAMILIES = ["rgba", "rgb-runs"]
STRICT_FAMILIES = ["rgb", "surface-3-rgb-odd", "planes-reference", "rgbplanes-pitched", "float16-window", "kt-surface-4-bgr-gap"]

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- the oracle's numbers, once per module ----------------------------------------------------------------------------------
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
        assert (self.enc.strips, self.enc.mb_rows) == (sh["n_strips"], sh["n_mbrows"])

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


# ---- 1. the tile set --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("family", TILE_FAMILIES)
def test_tile_set(torch_cuda, orc, family, grid, m):
    """The eight sizes (s = 1..8 strips in the last tile column) of one grid and one m (macroblock rows in the last tile row),
    three frames each, at both contents."""
    members = _members(grid, m)
    assert [t.s for t in members] == list(range(1, 9))
    for t in members:
        for content in gs.CONTENTS:
            case = _Case(torch_cuda, orc, family, t, content)
            case.check_everything()
            case.close()


# ---- 2. padding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("family", PADDED_FAMILIES)
def test_padding_does_not_reach_a_block(torch_cuda, orc, family, m):
    """The 2 x 2 sizes under two different fills of everything but the addressed samples (row padding, gaps, the bytes behind
    a chroma row that a re-read or moved-back unit fetches): identical records, sizes and tables."""
    torch = torch_cuda
    for t in _members(1, m):
        for content, quals in gs.TABLE_QUALITIES.items():
            results = []
            for fill in (1, 2):
                case = _Case(torch, orc, family, t, content, fill_seed=fill)
                results.append((_encode(torch, case.enc, case.dev, FIRST), _table(torch, case.enc, case.dev, quals)))
                case.close()
            (a, a_sizes), (b, b_sizes) = results[0][0], results[1][0]
            if (a, a_sizes) != (b, b_sizes):      # the second fill's records as `got`, the first fill's as `want`: where the fill leaks in
                r = case.t
                pytest.fail(case.where("encode under two fills") + f": the output depends on the fill; sizes {b_sizes} / {a_sizes}: "
                            + gs.describe_difference(gs.split(b, b_sizes), gs.split(a, a_sizes), r.W, r.H, r.mode, len(a_sizes)))
            case.check_numbers(f"frame_size_table{quals} under two fills", results[1][1][0], results[0][1][0])
            assert results[0][1][1] == results[1][1][1] == [0] * len(quals), case.where("frame_size_table status")


# ---- 3. batches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", BATCH_FAMILIES)
def test_batch_set(torch_cuda, orc, family):
    """184 x 88 (4 tiles a frame) in batches of 7, 8, 9, 16 and 17 frames on an encoder of max_frames = 17: frames in groups of
    8 and a tail of n % 8.  Every frame's record is the oracle's record of that frame at its index, which a wrong frame / tile
    map breaks as swapped or duplicated frames; the size table and the rd table at K = 2."""
    case = _Case(torch_cuda, orc, family, gs.batch_member(), "q12", n=gs.BATCH_MAX, max_frames=gs.BATCH_MAX)
    for n in gs.BATCH_SIZES:
        case.check_encode(f"encode of {n} frames", n=n)
        case.check_tables(gs.TABLE_QUALITIES["q12"], n=n)
    case.close()


def test_batch_set_pipelined_sequence(torch_cuda, orc):
    """Batches of 17, 8 and 9 frames in pipelined mode behind one flush."""
    torch = torch_cuda
    case = _Case(torch, orc, "rgb", gs.batch_member(), "q12", n=gs.BATCH_MAX, max_frames=gs.BATCH_MAX)
    case.enc.set_pipelined(True)
    calls = []
    for n in (17, 8, 9):
        out = torch.empty(case.enc.frame_bound * n, dtype=torch.uint8, device="cuda")
        calls.append((n,) + tuple(case.enc.encode(case.dev[:n], FIRST, out=out)))
    case.enc.flush()
    torch.cuda.synchronize()
    for n, out, sizes, meta in calls:
        total, status = (int(x) for x in meta.cpu())
        assert status & 0xFFFFFFFF == 0, (n, status)
        case.check_records(f"pipelined encode of {n} frames", out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()],
                           [case.record(f) for f in range(n)], n)
    case.close()


# ---- 4. the run kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", gs.RUN_MBROWS)
@pytest.mark.parametrize("family", RUN_FAMILIES)
def test_run_set(torch_cuda, orc, family, rows):
    """Strips of `rows` macroblock rows, 1, 2 and 5 of them, two frames, both contents, the buffer on a 4-byte boundary and one
    byte behind it (the input mode: geometry_space.input_mode).  RGBA on its default producer; packed RGB forced to the run
    kernels, where the size table is one probe per quality."""
    members = [t for t in gs.run_set() if gs.shape(t.W, t.H)["n_mbrows"] == rows]
    assert [gs.shape(t.W, t.H)["n_strips"] for t in members] == list(gs.RUN_STRIPS)
    for t in members:
        for content, quals in gs.TABLE_QUALITIES.items():
            for offset in (0, 1):
                case = _Case(torch_cuda, orc, family, t, content, offset=offset)
                case.check_encode(f"encode, buffer offset {offset}")
                if family == "rgb-runs":
                    qs = [quals[(f + 1) % len(quals)] for f in range(case.n)]
                    case.check_probe(qs)
                    case.check_tables(quals, with_rd=False)
                case.close()


# ---- 5. odd widths at even heights ------------------------------------------------------------------------------------------
# the families that take an odd width (a frame table serves any plane layout, planes-odd's too)
ODD_WIDTH_FAMILIES = ["rgb", "rgb-fallback", "rgba", "planes-reference", "planes-odd", "kp-planes-reference", "kt-planes-odd"]


@pytest.mark.parametrize("family", ODD_WIDTH_FAMILIES)
def test_odd_widths_at_even_heights(torch_cuda, orc, family):
    """33, 35 and 47 wide at 32 and 34 high: the chroma stride W / 2 rounds down at heights where the reference runs, so the
    oracle's records here are records the reference confirms at these sizes (tests/test_geometry_space_cpu.py); the tile set has
    odd widths at odd heights only."""
    for t in gs.odd_width_set():
        for content in gs.CONTENTS:
            case = _Case(torch_cuda, orc, family, t, content)
            case.check_everything()
            case.close()


# ---- 6. the strict region ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", STRICT_FAMILIES)
def test_strict_set(torch_cuda, orc, family):
    """6 strips x 9 macroblock rows of pictures of three widths: the region stays, the pitch varies."""
    for t in gs.strict_set():
        for content in gs.CONTENTS:
            case = _Case(torch_cuda, orc, family, t, content)
            case.check_everything()
            case.close()
