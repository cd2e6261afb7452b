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
import pytest

import geometry_space as gs
from geometry_cases import FIRST, PADDED_FAMILIES, RUN_FAMILIES, TILE_FAMILIES, _Case, _members
from gpu_calls import _encode, _table

pytestmark = pytest.mark.gpu

BATCH_FAMILIES = ["rgb", "rgba", "surface-4-bgr-gap", "planes-nv12", "float32-window", "yuy2", "kt-planes-nv12", "kp-rgbplanes-pitched"]
STRICT_FAMILIES = ["rgb", "surface-3-rgb-odd", "planes-reference", "rgbplanes-pitched", "float16-window", "kt-surface-4-bgr-gap"]

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


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
