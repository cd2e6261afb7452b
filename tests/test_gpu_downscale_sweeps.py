"""The three sweeps of the downscale kernels (-m gpu): geometry (tests/test_gpu_geometry.py), code space
(tests/test_gpu_code_space.py) and hard content (tests/test_gpu_hard_content.py) through k_downscale_encode,
k_downscale_size_table and k_downscale_rd_table of both source pixel widths.  The cases are those modules' own case classes with
another input: the content's packed pixels become a source that repeats each pixel 2 x 2 (downscale.replicated_source), whose
box average is the content exactly, written into the window at source pixel (3, 1) of a larger surface of noise with padded rows
and a gap between frames (downscale.place); a 4th byte is noise.  So the records, censuses and failure messages are the existing
sweeps': a failure names the member, the frame, the slice and the tile column, or the block by its DC level and first (run,
level).  These sweeps hold the back half and the addressing; the arithmetic of the average is held on noise sources by
tests/test_gpu_downscale.py.

REACHED (tests/downscale_sweeps.py) lists the (kernel row, source pixel width) this module sends content through;
tests/test_downscale_abi.py holds it against the code object, so a downscale kernel added without a sweep fails there.

  geometry      all 64 members of geometry_space.tile_set() and the batch member at even widths, narrow staging (quality 12):
                encode, size table, rd table; the four members of tests/test_input_families_cpu.py at wide staging (quality 90)
  code space    the narrow, wide and DC sets: encodes with per-frame quality; size table, rd table and the frame_sizes probe
  hard content  size tables (narrow and wide), the rd table's sizes and distortion, encodes with per-frame quality and the probe
  fallback      one member through the global-memory fallback (m1v_debug_set_lds_words)
"""
import pytest

import code_space as cs
import code_space_cases as code
import downscale as ds
import geometry_cases as geo
import geometry_space as gs
import hard_content as hc
import hard_content_cases as hard
import rd_oracle as rd
from downscale_sweeps import VARIANTS
from gpu_calls import _encode, _rd

pytestmark = pytest.mark.gpu

IDS = [f"x{Cs}" for Cs in VARIANTS]
# the members of tests/test_input_families_cpu.py
MEMBERS = [next(t for t in gs.tile_set() if (t.grid, t.s, t.m) == key) for key in ((0, 1, 1), (0, 8, 4), (1, 3, 1), (1, 7, 3))]
WHERE = dict(pad=13, gap=5, window=(3, 1), margin=(2, 3))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def family(Cs):
    """The family name a case reports; it starts with "surface-", so geometry_space.restricted gives the even widths."""
    return f"surface-downscale-x{Cs}"


class _Input:
    kind, buf, lay, base = "rgb", None, None, None


def build(torch, Cs, W, H, mode, Q, cap, pixels, fill, order):
    """input_families.build for a downscale variant: the encoder with the layout in force and the window view of the source."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    out = _Input()
    out.dev, lay, _ = ds.place(torch, ds.replicated_source(pixels, order), Cs, order, fill_seed=fill, **WHERE)
    out.enc = Mpeg1Encoder(W, H, Q, mode, max_frames=cap)
    out.enc.set_downscale_layout(lay)
    assert out.enc.path == "tiles" and out.enc.size_table_fused == 1 and out.enc.downscale_layout == lay
    return out


# ---- geometry -----------------------------------------------------------------------------------------------------------------
class _Geometry(geo._Case):
    def __init__(self, torch, orc, Cs, t, content, n=None, max_frames=None):
        self.torch, self.orc, self.family, self.content = torch, orc, family(Cs), content
        self.t = t = gs.restricted(t, self.family)
        assert t.W % 2 == 0
        self.n = n = gs.FRAMES[t.set] if n is None else n
        self.Q = gs.CONTENTS[content][0]
        self.input = build(torch, Cs, t.W, t.H, t.mode, self.Q, n if max_frames is None else max_frames,
                           gs.pixels(t, content, 3, n).copy(), Cs + t.k, ("rgb", "bgr")[t.k % 2])
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        sh = gs.shape(t.W, t.H, t.mode)
        assert (self.enc.strips, self.enc.mb_rows) == (sh["n_strips"], sh["n_mbrows"])


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_tile_set(torch_cuda, orc, Cs, grid, m):
    """The eight sizes (s = 1..8 strips in the last tile column) of one grid and one m, three frames each, at narrow staging."""
    members = geo._members(grid, m)
    assert [t.s for t in members] == list(range(1, 9))
    for t in members:
        case = _Geometry(torch_cuda, orc, Cs, t, "q12")
        case.check_everything()
        case.close()


@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_tile_set_wide_staging(torch_cuda, orc, Cs):
    """One strip x one row; a whole tile; 2 x 2 grids with 3 x 1 and 7 x 3 in the last column / row, at quality 90."""
    for t in MEMBERS:
        case = _Geometry(torch_cuda, orc, Cs, t, "q90")
        case.check_everything()
        case.close()


@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_batch_set(torch_cuda, orc, Cs):
    """184 x 88 in batches of 7, 8, 9, 16 and 17 frames on an encoder of max_frames = 17."""
    case = _Geometry(torch_cuda, orc, Cs, gs.batch_member(), "q12", n=gs.BATCH_MAX, max_frames=gs.BATCH_MAX)
    for n in gs.BATCH_SIZES:
        case.check_encode(f"encode of {n} frames", n=n)
        case.check_tables(gs.TABLE_QUALITIES["q12"], n=n)
    case.close()


@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_fallback(torch_cuda, orc, Cs):
    """The 2 x 2 grid with 7 x 3 in the last column / row with an LDS image of 8 words and the worst-case arena reserved: every
    unit goes through the global-memory fallback."""
    case = _Geometry(torch_cuda, orc, Cs, MEMBERS[3], "q12")
    case.enc.debug_set_lds_words(8)
    case.enc.reserve_scratch(True)
    case.check_everything()
    case.close()


# ---- code space ---------------------------------------------------------------------------------------------------------------
class _CodeSpace(code._Case):
    def __init__(self, torch, orc, Cs, name):
        self.torch, self.orc, self.family, self.name = torch, orc, family(Cs), name
        self.Q = cs.TOP["narrow"] if name == "narrow" else cs.TOP["wide"]
        self.input = build(torch, Cs, code.W, code.H, "full", self.Q, code.BATCH, code._pixels(orc, name, "rgb"),
                           Cs, ("bgr", "rgb")[code.SETS.index(name) % 2])
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        self.frames = code._frames(orc, name, self.kind)
        self.qualities = self.frames["qualities"]
        self.n = len(self.qualities)
        assert max(self.qualities) <= self.Q


@pytest.mark.parametrize("name", code.SETS)
@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_code_space_encodes(torch_cuda, orc, Cs, name):
    case = _CodeSpace(torch_cuda, orc, Cs, name)
    for a, b in case.batches():
        case.check_encode(a, b, "encode")
    case.close()


@pytest.mark.parametrize("name", code.SETS)
@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_code_space_tables(torch_cuda, orc, Cs, name):
    """Each run of frames of one quality q is asked for (20, 50, q): frame_size_table, frame_rd_table (sizes and exact
    distortion) and frame_sizes give the oracle's numbers."""
    torch = torch_cuda
    case = _CodeSpace(torch, orc, Cs, name)
    for a, b in case.groups():
        quals = tuple(sorted({20, 50, case.qualities[a]}))
        dev = case.dev[a:b]
        want = [[len(case.record(f, q)) for f in range(a, b)] for q in quals]
        table, status = code._table(torch, case.enc, dev, quals)
        assert status == [0] * len(quals), (case.family, name, quals, status)
        sizes, dist, status = _rd(torch, case.enc, dev, quals)
        assert status == [0] * len(quals), (case.family, name, quals, status)
        for k, q in enumerate(quals):
            probe = code._probe(torch, case.enc, dev, [q] * (b - a))
            for i, f in enumerate(range(a, b)):
                for what, got in (("frame_size_table", table[k][i]), ("frame_rd_table size", sizes[k][i]), ("frame_sizes", probe[i])):
                    if got != want[k][i]:
                        case.fail_number(what, f, q, got, want[k][i])
                d = code._distortion(orc, name, case.kind, f, q)
                if dist[k][i] != d:
                    case.fail_number("frame_rd_table distortion", f, q, dist[k][i], d)
    case.close()


# ---- hard content -------------------------------------------------------------------------------------------------------------
class _Hard(hard._Case):
    def __init__(self, torch, orc, Cs, W, H, ids):
        self.torch, self.orc, self.W, self.H, self.ids, self.n = torch, orc, W, H, tuple(ids), len(ids)
        self.family = family(Cs)
        self.input = build(torch, Cs, W, H, "full", hard.Q, self.n, hard._content(orc, "rgb", W, H)[list(ids)],
                           Cs, ("rgb", "bgr")[W // 176 % 2])
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        self.buf, self.lay, self.base = None, None, None


_dist_cache = {}


def _distortion(orc, W, H, c, q):
    key = (W, H, c, q)
    if key not in _dist_cache:
        _dist_cache[key] = rd.frame_distortion(orc, hard._content(orc, "rgb", W, H)[c], W, H, q, orc.MODE_FULL, 3)
    return _dist_cache[key]


@pytest.mark.parametrize("W,H", hard.SIZES)
@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_hard_content_tables(torch_cuda, orc, Cs, W, H):
    """(20, 50, 76) takes the narrow kernels and carries the extreme-pattern frame; K = 8 up to 92 the wide ones.  The rd table
    gives the same sizes and the oracle's distortion."""
    case = _Hard(torch_cuda, orc, Cs, W, H, hard.HARD4)
    want = [case.sizes(q) for q in hc.TABLE_NARROW]
    assert case.table(hc.TABLE_NARROW) == want
    sizes, dist, status = _rd(torch_cuda, case.enc, case.dev, hc.TABLE_NARROW)
    assert (sizes, status) == (want, [0] * len(hc.TABLE_NARROW))
    assert dist == [[_distortion(orc, W, H, c, q) for c in hard.HARD4] for q in hc.TABLE_NARROW]
    case.close()
    case = _Hard(torch_cuda, orc, Cs, W, H, hard.HARD3)
    want = [case.sizes(q) for q in hc.TABLE_WIDE]
    assert case.table(hc.TABLE_WIDE) == want
    sizes, dist, status = _rd(torch_cuda, case.enc, case.dev, hc.TABLE_WIDE)
    assert (sizes, status) == (want, [0] * len(hc.TABLE_WIDE))
    assert dist == [[_distortion(orc, W, H, c, q) for c in hard.HARD3] for q in hc.TABLE_WIDE]
    case.close()


@pytest.mark.parametrize("W,H", hard.SIZES)
@pytest.mark.parametrize("Cs", VARIANTS, ids=IDS)
def test_hard_content_encodes(torch_cuda, orc, Cs, W, H):
    """Three hard frames at the encoder's quality 92, and four (with the extreme-pattern frame at 76 / 77) at qualities that
    mix 50, 76, 77 and 92 in one batch, with the frame_sizes probe."""
    torch = torch_cuda
    case3, case4 = _Hard(torch, orc, Cs, W, H, hard.HARD3), _Hard(torch, orc, Cs, W, H, hard.HARD4)
    assert _encode(torch, case3.enc, case3.dev, hard.FIRST) == case3.records([hard.Q] * case3.n)
    for qs in (hard.QS_A, hard.QS_B):
        assert _encode(torch, case4.enc, case4.dev, hard.FIRST, quality=list(qs)) == case4.records(qs), qs
        assert case4.probe(list(qs)) == case4.records(qs)[1], qs
    case3.close()
    case4.close()
