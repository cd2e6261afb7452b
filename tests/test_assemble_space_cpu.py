"""CPU pins of tests/assemble_space.py: the census of the cases that tests/test_gpu_assemble_space.py feeds k_assemble, the
byte-level model of its placement against the oracle, and the slips the cases are there to catch.

  census     the committed profiles/r32_assemble_census.txt (read, never written here) is what census_text() gives, and every
             item a-i of the placement space is reached: a case that drifts out of its branch fails here, without a GPU.
  model      place_batch rebuilds the oracle's records for every case, touches no word outside the image and no guard byte.
  slips      each way the kernel could be subtly wrong changes the bytes of the case that is there for it (or, for the dropped
             range check, touches words behind the image: see test_dropped_range_check_reaches_behind_the_image).
  hooks      the two entry points refuse null arguments before they touch a device."""
import ctypes as C
import os

import pytest

import assemble_space as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = os.path.join(ROOT, "profiles", "r32_assemble_census.txt")


@pytest.fixture(scope="module")
def census(orc):
    return A.census(orc)[0]


# ---- census -----------------------------------------------------------------------------------------------------------------
def test_census_is_the_committed_one(orc):
    """The committed text is read, never written: a change of the scenes, of the model or of plan_shape that alters a line fails
    here until the file is rewritten from census_text(), and the rewrite shows as a diff."""
    text = A.census_text(orc)
    print(text)
    committed = open(CENSUS).read()
    if committed != text:
        a, b = committed.splitlines(), text.splitlines()
        k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        pytest.fail(f"profiles/r32_assemble_census.txt differs from census_text() at line {k + 1}:\n  committed: {(a + [''])[k][:300]}\n"
                    f"  generated: {(b + [''])[k][:300]}")


def test_a_every_shape(census):
    shapes = census["a. shapes (group, lanes_log2) by producer"]
    assert set(A.ALL_SHAPES) <= {tuple(x) for x in shapes["tiles"]}
    for name in ("runs-sweep", "strips-sweep"):          # 16 and 17 strips: the hook accepts every pair, and every pair is run
        sc = A.scene(name)
        accepted = {(g, k) for g, k in A.ALL_SHAPES if A.hook_accepts(sc, g, k)}
        assert accepted == set(A.ALL_SHAPES) <= set(sc.shapes), name
        assert accepted <= {tuple(x) for x in shapes[A.geometry(sc)["producer"]]}, name
    for sc, forced in A.cases():
        assert A.hook_accepts(sc, *forced), (sc.name, forced)
    sweeps = {A.geometry(sc)["producer"] for sc in A.SCENES if sc.name.endswith("-sweep")}
    assert sweeps == {"tiles", "dense", "strips"}


def test_b_group_sizes(census):
    b = census["b. group sizes"]
    short = {tuple(x) for x in b["ns < group: (ns, group)"]}
    assert {(1, g) for g in (2, 4, 8, 16)} <= short
    assert {(3, g) for g in (4, 8, 16)} <= short           # 1 < ns < group, and no power of two
    assert b["one-macroblock picture: (ns, nseg)"] == [(1, 1)]


def test_c_passes(census):
    c = census["c. passes"]
    assert c["passes"] == ["1", "2", ">=3"]
    assert c["group >= 4, a pass boundary inside a segment: groups"]
    assert c["group >= 4, a pass boundary beside a word two segments share: cases"]


def test_d_chunks_by_passes(census):
    assert {tuple(x) for x in census["d. (chunks, passes)"]["pairs"]} == {(c, p) for c in ("1", "2", ">=3") for p in ("1", ">=2")}


def test_e_reached_by_the_plan_alone(census):
    e = census["e. by the plan alone"]
    assert e["several chunks: scenes"] and e["several passes: scenes"]


def test_f_long_segments(census):
    f = census["f. long segments"]
    for L in (2, 4, 8, 16):
        assert f[f"L={L}: nw among 4L-1, 4L, 4L+1"] == [4 * L - 1, 4 * L, 4 * L + 1], L
        assert min(f[f"L={L}: two trips or more (nw >= 8L): trips"]) >= 2, L
        assert f[f"L={L}: phases of the first trip"] == list(range(32)), L
        assert f[f"L={L}: phases in the long loop"] == list(range(32)), L
    assert any(is_long for _, is_long in f["bits a multiple of 32: (bits, long)"])
    assert any(not is_long for _, is_long in f["bits a multiple of 32: (bits, long)"])


def test_g_range_checks(census):
    g = census["g. range checks"]
    for L in (16, 2):
        window = g[f"L={L}: single pass, checked (img_end)"]
        assert window and all(A.IMAGE_BYTES - 16 * (L + 1) < e <= A.IMAGE_BYTES for e in window), (L, window)
        below = g[f"L={L}: unchecked directly below the window (img_end)"]
        assert below and all(A.IMAGE_BYTES - 32 * (L + 1) < e <= A.IMAGE_BYTES - 16 * (L + 1) for e in below), (L, below)


def test_h_edges(census):
    h = census["h. edges"]
    assert h["lead"] == list(range(16)) and h["img_end mod 16"] == list(range(16))
    assert h["begins and ends inside one unit: (lead, img_end)"]
    assert h["ends exactly on a unit: cases"]


def test_i_short_segments(census):
    i = census["i. short segments"]
    # tiles: one macroblock row without the slice header, of the macroblock of fewest bits (assemble_space.LEAST): one word
    assert i["tiles: fewest bits"] == [A.LEAST_MACROBLOCK_BITS] == [32]
    # strips: the header and nine such macroblocks
    assert i["strips: fewest bits"] == [38 + 9 * A.LEAST_MACROBLOCK_BITS]
    assert i["dense: zero-bit segments"] == [True] and i["dense: fewest bits"] == [0]      # the run kernel pads with empty segments
    assert i["tiles: zero-bit segments"] == [False] and i["strips: zero-bit segments"] == [False]


def test_i_no_macroblock_is_shorter(orc):
    """LEAST is the least: no flat colour of a grid over the cube codes a macroblock in fewer bits at quality 1, 2 or 12 (DC levels
    only shrink with the quality, and a flat block has no AC level)."""
    import numpy as np
    seen = {}
    for q in (1, 2, 12):
        for r in range(0, 256, 15):
            for g in list(range(0, 256, 15)) + [88]:
                for b in range(0, 256, 15):
                    px = np.empty((16, 16, 3), np.uint8)
                    px[:] = (r, g, b)
                    dc = tuple(int(x) for x in orc.frame_coefficients(px, 16, 16, q, orc.MODE_FULL)[:, 0])
                    seen.setdefault(dc, (r, g, b, q))
    bits = {dc: 2 + sum(len(orc.encode_block_bits(k < 4, [lv] + [0] * 63)[1]) for k, lv in enumerate(dc)) for dc in seen}
    assert min(bits.values()) == A.LEAST_MACROBLOCK_BITS
    assert bits[(1,) * 6] == A.LEAST_MACROBLOCK_BITS and seen[(1,) * 6][3] == A.LEAST_QUALITY


def test_plan_mirror_on_the_committed_parity_cases():
    """What the mirror says of the two cases of test_assemble_kernel_passes_chunks_and_long_segments that were labelled "552
    segments in one group": the plan groups 2 strips at quality 12 and 1 at quality 75, so 138 and 69 segments, one chunk."""
    for qf, group in ((12, 2), (75, 1)):
        sc = A.Scene("x", 128, 4368, 3, qf, None, 1, 0, (256,), None, ((0, 0),), "")
        g, lg, segs, producer = A.plan_shape(sc)
        assert (g, segs, producer) == (group, 69, "tiles") and g * segs <= A.CHUNK


# ---- the model against the oracle -------------------------------------------------------------------------------------------
def _guards_intact(pool, align, total):
    lo = A.GUARD + align
    return all(b == A.POISON for b in pool[:lo]) and all(b == A.POISON for b in pool[lo + total:])


@pytest.mark.parametrize("sc", A.SCENES, ids=lambda sc: sc.name)
def test_model_rebuilds_the_oracles_records(orc, sc):
    for forced in sc.shapes:
        shape = A.plan_shape(sc, forced)[:2]
        for align in ((0, 5) if forced == sc.shapes[0] else (0,)):
            pool, total, outside = A.place_batch(orc, sc, shape, align)
            want, wtotal = A.expected_pool(orc, sc, align)
            assert total == wtotal and not outside, (forced, align, sorted(outside)[:4])
            lo = A.GUARD + align
            assert pool == want, A.describe_difference(orc, sc, shape, bytes(pool[lo:lo + total]), align)
            assert _guards_intact(pool, align, total)


def test_model_at_every_alignment(orc):
    sc = A.scene(A.ALIGN_SCENE)
    shape = A.plan_shape(sc)[:2]
    for align in range(16):
        pool, total, outside = A.place_batch(orc, sc, shape, align)
        assert pool == A.expected_pool(orc, sc, align)[0] and not outside, align


# ---- slips ------------------------------------------------------------------------------------------------------------------
SLIP_CASES = {
    "store-not-or": ("tiles-sweep", (4, 4)),             # neighbouring segments share their boundary word
    "no-padding": ("tiles-sweep", (4, 4)),               # a strip's zero bits ride on its last segment
    "carry-kept-over-pass": ("chunks-2", (16, 1)),       # two passes: the scan starts again
    "carry-lost-at-chunk": ("chunks-2", (16, 1)),        # two chunks: the scan goes on
    "long-loop-stops-early": ("tiles-sweep", (4, 1)),    # segments of a multiple of four words leave a tail word
    "lead-ignored": ("tiles-sweep", (4, 4)),
    "first-unit-whole": ("tiles-sweep", (4, 4)),
    "last-unit-whole": ("tiles-sweep", (4, 4)),
}


@pytest.mark.parametrize("slip", sorted(SLIP_CASES))
def test_slip_changes_the_record(orc, slip):
    name, shape = SLIP_CASES[slip]
    sc = A.scene(name)
    want, total = A.expected_pool(orc, sc)
    pool, _, _ = A.place_batch(orc, sc, shape, slips=(slip,))
    assert pool[A.GUARD:A.GUARD + total] != want[A.GUARD:A.GUARD + total], slip
    assert slip in A.SLIPS


def test_last_unit_written_whole_changes_a_guard_byte(orc):
    """The batch's last group ends img_end mod 16 bytes into a unit; written whole, the unit covers the four trailer bytes and
    then 12 - img_end mod 16 bytes of the guard.  At some alignment of the output that is at least one."""
    sc = A.scene("tiles-sweep")
    shape = (4, 4)
    hit = []
    for align in range(16):
        wgs, total = A.workgroups(orc, sc, shape, align)
        last = wgs[-1]
        pool, _, _ = A.place_batch(orc, sc, shape, align, slips=("last-unit-whole",), only={(last.f, last.x)})
        spills = 0 < last.img_end % 16 < 12
        assert _guards_intact(pool, align, total) == (not spills), (align, last.img_end % 16)
        hit.append(spills)
    assert any(hit) and not all(hit)


def test_first_unit_written_whole_on_an_output_that_starts_in_the_guard(orc):
    """The first group of a frame lies 44 bytes behind the record's start, so its first unit never reaches the guard in front:
    the slip costs header bytes (or the group in front its last bytes).  Nothing the kernel writes starts closer to the pool's
    edge than the header itself."""
    sc = A.scene("tiles-sweep")
    for align in (1, 9):
        wgs, total = A.workgroups(orc, sc, (4, 4), align)
        pool, _, _ = A.place_batch(orc, sc, (4, 4), align, slips=("first-unit-whole",), only={(0, 0)})
        want, _ = A.expected_pool(orc, sc, align)
        lo = A.GUARD + align
        assert wgs[0].lead == (align + 44) % 16
        assert pool[lo:lo + 44] != want[lo:lo + 44] and _guards_intact(pool, align, total)


def test_dropped_range_check_reaches_behind_the_image(orc):
    """In the window (one pass, img_end within 16 (L + 1) bytes of the image's end) the first trip's lanes behind a segment's end
    still address up to 4 L + 3 words behind its start.  Without the range check those words lie behind the image, in the
    placement table.  What the lanes OR there is zero (nothing of the group lies behind img_end), so the record does NOT change:
    this slip shows as words touched outside the image, which the model reports and the correct placement never does."""
    name, shape = A.WINDOW
    sc = A.scene(name)
    wgs, _ = A.workgroups(orc, sc, shape)
    window = {(w.f, w.x) for w in wgs if w.in_window()}
    assert window
    _, _, outside = A.place_batch(orc, sc, shape, slips=("no-range-check",), only=window)
    assert outside and {(f, x) for f, x, _ in outside} <= window
    assert all(k >= A.IMAGE_BYTES // 4 for _, _, k in outside)
    assert not A.place_batch(orc, sc, shape)[2]


# ---- the hooks, without a device --------------------------------------------------------------------------------------------
def test_hooks_refuse_null_arguments():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    out = (C.c_int * 4)()
    assert L.m1v_debug_assemble_shape(None, out) == _ffi.E_ARG
    assert L.m1v_debug_set_assemble_shape(None, 0, 0) == _ffi.E_ARG
    assert L.m1v_debug_assemble_shape.restype is C.c_int and L.m1v_debug_set_assemble_shape.restype is C.c_int
