"""The three sweeps of the downscaled word kernels (-m gpu): geometry (tests/test_gpu_geometry.py), code space
(tests/test_gpu_code_space.py) and hard content (tests/test_gpu_hard_content.py) through k_half_words_encode,
k_half_words_size_table and k_half_words_rd_table of both chroma steps: one interleaved high-aligned preset (P010, shift 8) and one
planar low-aligned preset (I010, shift 2).  The cases are those modules' own case classes with another input: the content's planes
(the form the planes- families take) become a source of words that repeats each sample 2 x 2 as `sample << shift` with noise in
the bits below the shift (downscale_words.replicated_planes), whose average, shifted down, is the content exactly, written as a
pitched window of a larger surface of noise with padded rows, gaps between planes and frames and an odd base
(downscale_words.place); Cb and Cr alternate in which comes first.  So the records, censuses and failure messages are the existing
sweeps': a failure names the member, the frame, the slice and the tile column, or the block by its DC level and first (run,
level).  These sweeps hold the back half and the addressing; the arithmetic of the average is held on noise sources by
tests/test_gpu_downscale_words.py.

REACHED (tests/downscale_word_sweeps.py) lists the (kernel row, chroma step) this module sends content through;
tests/test_downscale_words_abi.py holds it against the code object, so a kernel added without a sweep fails there.

  geometry      all 64 members of geometry_space.tile_set() and the batch member at even sizes, narrow staging (quality 12):
                encode, size table, rd table; the four members of tests/test_input_families_cpu.py at wide staging (quality 90)
  code space    the narrow, wide and DC sets: encodes with per-frame quality; size table, rd table and the frame_sizes probe
  hard content  size tables (narrow and wide), the rd table's sizes and distortion, encodes with per-frame quality and the probe
  fallback      one member through the global-memory fallback (m1v_debug_set_lds_words)
"""
import numpy as np
import pytest

import code_space as cs
import code_space_cases as code
import downscale_words as dw
import geometry_cases as geo
import geometry_space as gs
import hard_content as hc
import hard_content_cases as hard
from downscale_word_sweeps import FORMS, VARIANTS
from gpu_calls import _encode, _rd

pytestmark = pytest.mark.gpu

IDS = [f"cstep{c}" for c in VARIANTS]
# the members of tests/test_input_families_cpu.py
MEMBERS = [next(t for t in gs.tile_set() if (t.grid, t.s, t.m) == key) for key in ((0, 1, 1), (0, 8, 4), (1, 3, 1), (1, 7, 3))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def family(cstep):
    """The family name a case reports."""
    return f"planes-downscale-words-cstep{cstep}"


class _Input:
    kind, buf, lay, base = "planes", None, None, None


def _whole(plane, h, w, seed):
    """A content plane of the coded region as a plane of the whole picture: noise outside the region, which is not coded."""
    n, ph, pw = plane.shape
    if (ph, pw) == (h, w):
        return plane
    out = np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)
    out[:, :ph, :pw] = plane
    return out


def build(torch, cstep, W, H, mode, Q, cap, planes, fill, k):
    """input_families.build for a variant: the encoder with the layout in force and the [n, L] view of the source."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    out = _Input()
    y, cb, cr = planes
    preset = FORMS[cstep]
    src = dw.replicated_planes(_whole(y, H, W, fill), _whole(cb, H // 2, W // 2, fill + 1), _whole(cr, H // 2, W // 2, fill + 2),
                               dw.SHIFT[preset], seed=fill)
    out.dev, lay, _ = dw.place(torch, src, preset, fill_seed=fill, cr_first=bool(k % 2), **dw.PITCHED)
    out.enc = Mpeg1Encoder(W, H, Q, mode, max_frames=cap)
    out.enc.set_downscale_word_layout(lay)
    assert out.enc.path == "tiles" and out.enc.size_table_fused == 1 and out.enc.downscale_word_layout == lay and lay["c_step"] == cstep
    return out


# ---- geometry -----------------------------------------------------------------------------------------------------------------
class _Geometry(geo._Case):
    def __init__(self, torch, orc, cstep, t, content, n=None, max_frames=None):
        self.torch, self.orc, self.family, self.content = torch, orc, family(cstep), content
        self.t = t = gs.restricted(t, "planes-i420")
        assert t.W % 2 == 0 and t.H % 2 == 0
        self.n = n = gs.FRAMES[t.set] if n is None else n
        self.Q = gs.CONTENTS[content][0]
        self.input = build(torch, cstep, t.W, t.H, t.mode, self.Q, n if max_frames is None else max_frames,
                           tuple(p[:n] for p in gs.planes(t, content)), cstep + t.k, t.k)
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        sh = gs.shape(t.W, t.H, t.mode)
        assert (self.enc.strips, self.enc.mb_rows) == (sh["n_strips"], sh["n_mbrows"])


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_tile_set(torch_cuda, orc, cstep, grid, m):
    """The eight sizes (s = 1..8 strips in the last tile column) of one grid and one m, three frames each, at narrow staging."""
    members = geo._members(grid, m)
    assert [t.s for t in members] == list(range(1, 9))
    for t in members:
        case = _Geometry(torch_cuda, orc, cstep, t, "q12")
        case.check_everything()
        case.close()


@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_tile_set_wide_staging(torch_cuda, orc, cstep):
    """One strip x one row; a whole tile; 2 x 2 grids with 3 x 1 and 7 x 3 in the last column / row, at quality 90."""
    for t in MEMBERS:
        case = _Geometry(torch_cuda, orc, cstep, t, "q90")
        case.check_everything()
        case.close()


@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_batch_set(torch_cuda, orc, cstep):
    """184 x 88 in batches of 7, 8, 9, 16 and 17 frames on an encoder of max_frames = 17."""
    case = _Geometry(torch_cuda, orc, cstep, gs.batch_member(), "q12", n=gs.BATCH_MAX, max_frames=gs.BATCH_MAX)
    for n in gs.BATCH_SIZES:
        case.check_encode(f"encode of {n} frames", n=n)
        case.check_tables(gs.TABLE_QUALITIES["q12"], n=n)
    case.close()


@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_fallback(torch_cuda, orc, cstep):
    """The 2 x 2 grid with 7 x 3 in the last column / row with an LDS image of 8 words and the worst-case arena reserved: every
    unit goes through the global-memory fallback."""
    case = _Geometry(torch_cuda, orc, cstep, MEMBERS[3], "q12")
    case.enc.debug_set_lds_words(8)
    case.enc.reserve_scratch(True)
    case.check_everything()
    case.close()


# ---- code space ---------------------------------------------------------------------------------------------------------------
class _CodeSpace(code._Case):
    def __init__(self, torch, orc, cstep, name):
        self.torch, self.orc, self.family, self.name = torch, orc, family(cstep), name
        self.Q = cs.TOP["narrow"] if name == "narrow" else cs.TOP["wide"]
        fr = code._frames(orc, name, "planes")
        self.input = build(torch, cstep, code.W, code.H, "full", self.Q, code.BATCH, (fr["Y"], fr["Cb"], fr["Cr"]), cstep,
                           code.SETS.index(name))
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        self.frames = code._frames(orc, name, self.kind)
        self.qualities = self.frames["qualities"]
        self.n = len(self.qualities)
        assert max(self.qualities) <= self.Q


@pytest.mark.parametrize("name", code.SETS)
@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_code_space_encodes(torch_cuda, orc, cstep, name):
    case = _CodeSpace(torch_cuda, orc, cstep, name)
    for a, b in case.batches():
        case.check_encode(a, b, "encode")
    case.close()


@pytest.mark.parametrize("name", code.SETS)
@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_code_space_tables(torch_cuda, orc, cstep, name):
    """Each run of frames of one quality q is asked for (20, 50, q): frame_size_table, frame_rd_table (sizes and exact
    distortion) and frame_sizes give the oracle's numbers."""
    torch = torch_cuda
    case = _CodeSpace(torch, orc, cstep, name)
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
    def __init__(self, torch, orc, cstep, W, H, ids):
        self.torch, self.orc, self.W, self.H, self.ids, self.n = torch, orc, W, H, tuple(ids), len(ids)
        self.family = family(cstep)
        self.input = build(torch, cstep, W, H, "full", hard.Q, self.n, tuple(p[list(ids)] for p in hard._content(orc, "planes", W, H)),
                           cstep, W // 176)
        self.enc, self.dev, self.kind = self.input.enc, self.input.dev, self.input.kind
        self.buf, self.lay, self.base = None, None, None


@pytest.mark.parametrize("W,H", hard.SIZES)
@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_hard_content_tables(torch_cuda, orc, cstep, W, H):
    """(20, 50, 76) takes the narrow kernels and carries the extreme-pattern frame; K = 8 up to 92 the wide ones.  The rd table
    gives the same sizes and the oracle's distortion."""
    for ids, quals in ((hard.HARD4, hc.TABLE_NARROW), (hard.HARD3, hc.TABLE_WIDE)):
        case = _Hard(torch_cuda, orc, cstep, W, H, ids)
        want = [case.sizes(q) for q in quals]
        assert case.table(quals) == want
        sizes, dist, status = _rd(torch_cuda, case.enc, case.dev, quals)
        assert (sizes, status) == (want, [0] * len(quals))
        assert dist == [[hard._case_dist(orc, case, f, q) for f in range(case.n)] for q in quals]
        case.close()


@pytest.mark.parametrize("W,H", hard.SIZES)
@pytest.mark.parametrize("cstep", VARIANTS, ids=IDS)
def test_hard_content_encodes(torch_cuda, orc, cstep, W, H):
    """Three hard frames at the encoder's quality 92, and four (with the extreme-pattern frame at 76 / 77) at qualities that
    mix 50, 76, 77 and 92 in one batch, with the frame_sizes probe."""
    torch = torch_cuda
    case3, case4 = _Hard(torch, orc, cstep, W, H, hard.HARD3), _Hard(torch, orc, cstep, W, H, hard.HARD4)
    assert _encode(torch, case3.enc, case3.dev, hard.FIRST) == case3.records([hard.Q] * case3.n)
    for qs in (hard.QS_A, hard.QS_B):
        assert _encode(torch, case4.enc, case4.dev, hard.FIRST, quality=list(qs)) == case4.records(qs), qs
        assert case4.probe(list(qs)) == case4.records(qs)[1], qs
    case3.close()
    case4.close()
