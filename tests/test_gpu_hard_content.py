"""GPU tests of the entropy stage on hard content through every kernel family (-m gpu): the fused size tables (narrow and wide
staging), per-frame quality, the frame_sizes probe, the rate calls, and the encode kernels of every layout, on the content of
tests/hard_content.py — every run length, levels on both sides of every table row's end, 20- and 28-bit escapes, blocks of more
than 64 and 128 bits (tests/test_hard_content_cpu.py pins that census).  The content of the other GPU test modules is noise,
which codes little more than DC sizes.  The families are those of tests/input_families.py:

  size tables, row independence, table against probes   rgb (k_size_table_tiles), rgba (_rgba), surface-4-bgr-gap, surface-3-rgb-odd
                      (_surface), planes-nv12, planes-odd (_planes), yuy2 (_step2), rgbplanes-pitched (_rgb_planes), bfloat16-window
                      (_float_planes), kt-surface-4-bgr-gap (kt_size_table_surface), kp-planes-nv12 (kp_size_table_planes)
  encodes, per-frame quality, probe, the fallback        rgb, rgba, eight surfaces, planes-i420, -nv12, -pitched, -odd, rgbplanes-bgr
                      (k_encode_rgb_planes), float16-window (k_encode_float_planes), uyvy, p010 (k_encode_step2), kt-yuy2
                      (kt_encode_step2), kp-rgbplanes-pitched (kp_encode_rgb_planes)
  the rate calls      rgb, surface-4-bgr-gap, planes-nv12, float32-window, kp-planes-nv12

Every comparison is for equality with the CPU oracle (tests/plane_oracle.py for planes); every status word is 0.  Sizes are
352x288 and, for a partial last tile column, 176x208.  The oracle's records are cached per module."""
import pytest

import hard_content as hc
from gpu_calls import _encode, _frame_rule, _oracle_on_buffer
from hard_content_cases import FIRST, HARD3, HARD4, QS_A, QS_B, SIZES, Q, _Case
from rate_rules import batch_rule, cbr_rule

pytestmark = pytest.mark.gpu

RATE6 = (0, 4, 1, 5, 2, 6)    # hard and flat frames in turn


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- content and the oracle's records, once per module ----------------------------------------------------------------------


NEW_TABLE_FAMILIES = ["yuy2", "rgbplanes-pitched", "bfloat16-window", "kt-surface-4-bgr-gap", "kp-planes-nv12"]
TABLE_FAMILIES = ["rgb", "rgba", "surface-4-bgr-gap", "surface-3-rgb-odd", "planes-nv12", "planes-odd"] + NEW_TABLE_FAMILIES
KERNEL_FAMILIES = ["rgb", "rgba", "surface-4-bgr-gap", "planes-nv12"] + NEW_TABLE_FAMILIES     # one per size-table kernel


# ---- 1. size tables against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("family", TABLE_FAMILIES)
def test_size_tables_match_the_oracle(torch_cuda, orc, family, W, H):
    """(20, 50, 76) takes the narrow kernel (qualities[-1] <= narrow_q = 76 for this matrix), K = 8 up to 92 the wide one; the
    narrow call also carries the extreme-pattern frame (levels up to 115 in one byte)."""
    case = _Case(torch_cuda, orc, family, W, H, HARD4)
    assert case.table(hc.TABLE_NARROW) == [case.sizes(q) for q in hc.TABLE_NARROW]
    if case.kind == "planes" and "odd" in family:       # the samples lie in the device buffer where the layout says
        want = _oracle_on_buffer(orc, case.buf, case.n, case.lay, case.base, W, H, FIRST, [76] * case.n, orc.MODE_FULL)
        assert want == [case.record(f, 76) for f in range(case.n)]
    case.close()
    case = _Case(torch_cuda, orc, family, W, H, HARD3)
    assert case.table(hc.TABLE_WIDE) == [case.sizes(q) for q in hc.TABLE_WIDE]
    case.close()


# ---- 2. a row does not depend on its neighbours -----------------------------------------------------------------------------
@pytest.mark.parametrize("family", KERNEL_FAMILIES)
def test_a_row_does_not_depend_on_its_neighbours(torch_cuda, orc, family):
    """The rows of 50 and 76 from the narrow kernel equal the same rows of a call that also asks for 77 (the wide kernel:
    the extreme-pattern frame has levels of 128 and more there); both are the oracle's."""
    W, H = 352, 288
    case = _Case(torch_cuda, orc, family, W, H, HARD4)
    narrow = case.table((20, 50, 76))
    wide = case.table((20, 50, 76, 77))
    assert narrow == wide[:3]
    assert wide == [case.sizes(q) for q in (20, 50, 76, 77)]
    assert case.table((50,)) == [wide[1]] and case.table((76, 77)) == wide[2:]
    case.close()


# ---- 3. the fused table equals the probes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", KERNEL_FAMILIES)
def test_fused_table_equals_the_probes(torch_cuda, orc, family):
    """frame_size_table row k == frame_sizes(quality=[q_k] * n) on the same encoder, and — where the hook exists: packed 3 and
    4 channels — the table of an encoder forced to the run kernels (size_table_fused == 0: one probe per quality)."""
    W, H = 352, 288
    case = _Case(torch_cuda, orc, family, W, H, HARD3)
    table = case.table(hc.TABLE_WIDE)
    for k, q in enumerate(hc.TABLE_WIDE):
        assert case.probe([q] * case.n) == table[k], q
    assert table == [case.sizes(q) for q in hc.TABLE_WIDE]
    case.close()
    if family in ("rgb", "rgba"):
        forced = _Case(torch_cuda, orc, family, W, H, HARD3, forced_runs=True)
        assert forced.table(hc.TABLE_WIDE) == table
        forced.close()


# ---- 4. encode, encode with per-frame quality, frame_sizes ------------------------------------------------------------------
ENCODE_FAMILIES = (["rgb", "rgba"] + [f"surface-{c}-{o}-{l}" for c in (3, 4) for o in ("rgb", "bgr") for l in ("odd", "window")]
                   + [f"planes-{l}" for l in ("i420", "nv12", "pitched", "odd")]
                   + ["rgbplanes-bgr", "float16-window", "uyvy", "p010", "kt-yuy2", "kp-rgbplanes-pitched"])


def _encodes(torch, case3, case4):
    assert _encode(torch, case3.enc, case3.dev, FIRST) == case3.records([Q] * case3.n)
    for qs in (QS_A, QS_B):
        assert _encode(torch, case4.enc, case4.dev, FIRST, quality=list(qs)) == case4.records(qs), qs
        assert case4.probe(list(qs)) == case4.records(qs)[1], qs


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("family", ENCODE_FAMILIES)
def test_encode_per_frame_quality_and_probe(torch_cuda, orc, family, W, H):
    """Three hard frames at the encoder's quality 92, and four (with the extreme-pattern frame at 76 / 77) at qualities that
    mix 50, 76, 77 and 92 in one batch; then the same with an 8-word LDS image and the worst-case arena reserved, which sends
    every unit — blocks over 64 bits included — through the global-memory fallback."""
    torch = torch_cuda
    case3, case4 = _Case(torch, orc, family, W, H, HARD3), _Case(torch, orc, family, W, H, HARD4)
    _encodes(torch, case3, case4)
    for case in (case3, case4):
        case.enc.debug_set_lds_words(8)
        case.enc.reserve_scratch(True)
    _encodes(torch, case3, case4)
    for case in (case3, case4):
        case.enc.debug_set_lds_words(0)
        case.enc.reserve_scratch(False)
    _encodes(torch, case3, case4)
    case3.close()
    case4.close()


# ---- 5. the rate calls ------------------------------------------------------------------------------------------------------
CANDS = (20, 50, 76, 85, 92)


@pytest.mark.parametrize("family", ["rgb", "surface-4-bgr-gap", "planes-nv12", "float32-window", "kp-planes-nv12"])
def test_rate_calls(torch_cuda, orc, family):
    """encode_to_budget, encode_to_batch_budget and a three-call chain of encode_at_bitrate on six frames, hard and flat in
    turn: picks, sizes and bytes are the rules of tests/test_rate_abi.py on the oracle's sizes, with budgets taken from those
    sizes so that the choice differs between frames."""
    torch = torch_cuda
    W, H = 352, 288
    case = _Case(torch, orc, family, W, H, RATE6)
    enc, dev, n = case.enc, case.dev, case.n
    s = [case.sizes(c) for c in CANDS]

    def want(pick):
        return case.records([CANDS[k] for k in pick])

    cap = sorted(s[2])[n // 2]                                     # the median size at candidate 76
    pick, over = _frame_rule(s, cap)
    assert len(set(pick)) > 1, pick
    got, sizes, ch, ov = enc.encode_to_budget(dev, cap, CANDS, first_frame_index=FIRST)
    assert (ch, ov, (got, sizes)) == ([CANDS[k] for k in pick], over, want(pick))

    B = (sum(s[2]) + sum(s[3])) // 2
    pick, over = batch_rule(s, B)
    assert len(set(pick)) > 1 and not over, pick
    got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, CANDS, first_frame_index=FIRST)
    assert (ch, ov, (got, sizes)) == ([CANDS[k] for k in pick], over, want(pick))

    r = sorted(s[2])[n // 2]
    start = 2 * r
    pick, over, lvl = cbr_rule(s, r, 2 * r, start)
    assert len(set(pick)) > 1, pick
    level = torch.full((1,), start, dtype=torch.int64, device="cuda")
    parts = [enc.encode_at_bitrate(dev[a:a + 2], r, 2 * r, CANDS, level, first_frame_index=FIRST + a) for a in (0, 2, 4)]
    assert int(level.cpu()[0]) == lvl
    assert [c for p in parts for c in p[2]] == [CANDS[k] for k in pick]
    assert [f + 2 * i for i, p in enumerate(parts) for f in p[3]] == over
    assert (b"".join(p[0] for p in parts), [x for p in parts for x in p[1]]) == want(pick)
    case.close()
