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
import pytest

from code_space_cases import SETS, _Case, _distortion, _probe
from gpu_calls import _rd, _table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


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
