"""CPU pins of tests/geometry_space.py: the census of the shapes that tests/test_gpu_geometry.py feeds the kernels, conditions
on its content, and the oracle at those shapes against the real reference and against recorded hashes.

  census        the committed profiles/r17_geometry_census.txt (read, never written here) is what census_text() gives, and
                nothing is missing from it: every
                (strips_here, mrows_here) pair 1..8 x 1..4 in both grids, all 16 residues of W and of H, both parities, every
                batch class, every input mode and both producers of the run kernels.
  content       is position-sensitive, which is what lets a GPU test see a wrong clamp: for every tile-set size the picture
                whose last coded strip repeats the strip before it, the one whose last macroblock row repeats the row before it
                and the one whose chroma source columns of the last strip (read with stride W / 2: they lie anywhere in the
                picture, cropped columns included) repeat those of the strip before it each give another record.
  reference     the 32 tile-set members of even height and the six odd widths at even heights (the set oddw: in the tile set
                W and H have the same parity) through the reference's folder driver, as
                tests/test_oracle_vs_reference.py::test_driver_end_to_end does (full mode, quality 12; skipped where
                oracle/_ref is not available).  No test runs the reference at an odd height: it corrupts its heap there
                (DESIGN.md), whether glibc notices is chance, and a test that waits for an abort is no test.
  hashes        tests/golden/geometry_space.json (written by tests/golden/make_goldens.py) holds the SHA-256 of the oracle's
                records of every member of every set, odd heights included, on the generated content; the oracle here must give
                them.  This runs everywhere: for the even-height members it ties the oracle of any machine to the one that was
                compared with the reference."""
import json
import os

import numpy as np
import pytest

import geometry_space as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = os.path.join(ROOT, "profiles", "r17_geometry_census.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden", "geometry_space.json")


# ---- census -----------------------------------------------------------------------------------------------------------------
def test_census_is_the_committed_one():
    """The committed text is read, never written: a change of the sets, of shape(), run_plan() or input_mode() that alters a
    line — the per-size rows of the run set included — fails here until `python tests/golden/make_goldens.py geometry_space`
    rewrites the file, and the rewrite shows as a diff."""
    committed, text = open(CENSUS).read(), gs.census_text()
    if committed != text:
        a, b = committed.splitlines(), text.splitlines()
        k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        pytest.fail(f"profiles/r17_geometry_census.txt differs from census_text() at line {k + 1}:\n  committed: {(a + [''])[k][:300]}\n"
                    f"  generated: {(b + [''])[k][:300]}")


def test_census_is_complete():
    c = gs.census()
    pairs = [(s, m, g) for g in (0, 1) for s in range(1, 9) for m in range(1, 5)]
    for label, _ in gs.RESTRICTIONS:
        tile = c[f"tile, {label}"]
        assert tile["(strips_here, mrows_here, grid)"] == sorted(pairs), label
        assert tile["odd strips_here, by grid"] == sorted((s, g) for g in (0, 1) for s in (1, 3, 5, 7)), label
    any_size = c["tile, " + gs.RESTRICTIONS[0][0]]
    assert any_size["W mod 16"] == any_size["H mod 16"] == any_size["3 W mod 16"] == list(range(16))
    assert any_size["W parity"] == any_size["H parity"] == [0, 1] and len(any_size["sizes"]) == 64
    even_w = c["tile, " + gs.RESTRICTIONS[1][0]]
    assert even_w["W mod 16"] == list(range(0, 16, 2)) and even_w["H mod 16"] == list(range(16))
    even = c["tile, " + gs.RESTRICTIONS[2][0]]
    assert even["W mod 16"] == even["H mod 16"] == list(range(0, 16, 2))
    assert c["batch"]["(n, n mod 8, n // 8)"] == [(7, 7, 0), (8, 0, 1), (9, 1, 1), (16, 0, 2), (17, 1, 2)]
    assert c["batch"]["(strips_here, mrows_here, tiles per frame)"] == [(3, 1, 4)] and c["batch"]["size"] == [(184, 88)]
    run = c["run"]
    assert run["producer"] == ["dense", "strips"] and run["dense input mode"] == [0, 1, 2, 3]
    assert run["(producer, input mode)"] == [("dense", 0), ("dense", 1), ("dense", 2), ("dense", 3), ("strips", 0), ("strips", 1)]
    assert run["T"] == [64, 192, 256] and run["last run short"] == [False, True]
    assert c["strict"]["W parity"] == [0, 1] and len(c["strict"]["W mod 16"]) == 3
    assert any_size["(W parity, H parity)"] == [(0, 0), (1, 1)]      # the formula's: odd widths at even heights are the set oddw
    assert c["oddw"]["(W parity, H parity)"] == [(1, 0)] and len(c["oddw"]["sizes"]) == 6


def test_tile_set_is_the_formula():
    tiles = gs.tile_set()
    assert len(tiles) == 64 and [t.k for t in tiles] == list(range(64))
    assert max(t.W for t in tiles) <= 271 and max(t.H for t in tiles) <= 143
    for r in range(16):
        assert sum(t.W % 16 == r for t in tiles) == 4 and sum(t.H % 16 == r for t in tiles) == 4
    assert sum(t.H % 2 == 0 for t in tiles) == 32
    for t in tiles:
        sh = gs.shape(t.W, t.H)
        assert (sh["strips_here"], sh["mrows_here"], sh["tile_cols"], sh["tile_rows"]) == (t.s, t.m, t.grid + 1, t.grid + 1)
        for family in ("surface-3-rgb-odd", "planes-nv12"):          # the nearest size below keeps the shape
            r = gs.restricted(t, family)
            assert gs.shape(r.W, r.H) == sh and r.W % 2 == 0 and (family.startswith("surface") or r.H % 2 == 0)


def test_run_set_is_what_the_issue_names():
    plans = {(gs.shape(t.W, t.H)["n_mbrows"], gs.shape(t.W, t.H)["n_strips"]): gs.run_plan(gs.shape(t.W, t.H)["n_strips"], gs.shape(t.W, t.H)["n_mbrows"])
             for t in gs.run_set()}
    assert sorted(plans) == [(r, s) for r in gs.RUN_MBROWS for s in gs.RUN_STRIPS]
    assert all(plans[r, s]["producer"] == ("strips" if r < 11 else "dense") for r, s in plans)
    assert (plans[11, 1]["T"], plans[11, 1]["bps"]) == (64, 66)
    assert plans[42, 1]["T"] == 192 and plans[43, 1]["T"] == 256 and plans[43, 1]["bps"] == 258
    assert plans[11, 5]["units"] == 6 and plans[11, 5]["rem"] == 330 % 64


# ---- content ----------------------------------------------------------------------------------------------------------------
def test_generator_is_pinned():
    """The generator is written out in geometry_space.py; these bytes pin it wherever the suite runs."""
    assert gs._bytes(0, 4).tolist() == [226, 110, 6, 248]
    assert gs._bytes(5, 3).tolist() == gs._bytes(5, 8)[:3].tolist()
    b = gs.noise(3, (1 << 16,))
    assert 200 < np.bincount(b, minlength=256).min() and np.bincount(b, minlength=256).max() < 320
    g = gs.noise(3, (1 << 12,), 20)
    assert g.min() == 118 and g.max() == 137


@pytest.mark.parametrize("content", list(gs.CONTENTS))
def test_content_is_position_sensitive(orc, content):
    q = gs.CONTENTS[content][0]
    checked = {"strip": 0, "row": 0, "chroma": 0}
    for t in gs.tile_set():
        sh = gs.shape(t.W, t.H)
        xe, ye, hw = 16 * sh["n_strips"], 16 * sh["n_mbrows"], t.W // 2
        px = gs.pixels(t, content)[0]
        want = orc.encode_frame(px, t.W, t.H, 0, q, orc.MODE_FULL)
        blocks = orc.frame_coefficients(px, t.W, t.H, q, orc.MODE_FULL).reshape(sh["n_strips"], sh["n_mbrows"], 6, 64)
        if sh["n_strips"] > 1:
            alt = px.copy()
            alt[:, xe - 16:xe] = px[:, xe - 32:xe - 16]
            assert orc.encode_frame(alt, t.W, t.H, 0, q, orc.MODE_FULL) != want, (gs.name(t), "last strip")
            checked["strip"] += 1
        if sh["n_mbrows"] > 1:
            alt = px.copy()
            alt[ye - 16:ye] = px[ye - 32:ye - 16]
            assert orc.encode_frame(alt, t.W, t.H, 0, q, orc.MODE_FULL) != want, (gs.name(t), "last macroblock row")
            checked["row"] += 1
        if sh["n_strips"] > 1:
            # the chroma samples of the last strip: flat indices r * (W / 2) + x / 2 + j of the full-resolution planes
            idx = (np.arange(ye // 2)[:, None] * hw + (xe - 16) // 2 + np.arange(8)[None, :]).reshape(-1)
            alt = px.reshape(-1, 3).copy()
            alt[idx] = px.reshape(-1, 3)[idx - 8]
            alt = alt.reshape(px.shape)
            assert orc.encode_frame(alt, t.W, t.H, 0, q, orc.MODE_FULL) != want, (gs.name(t), "chroma source columns")
            got = orc.frame_coefficients(alt, t.W, t.H, q, orc.MODE_FULL).reshape(blocks.shape)
            assert not np.array_equal(got[-1, :, 4:], blocks[-1, :, 4:]), (gs.name(t), "chroma blocks of the last strip")
            checked["chroma"] += 1
    assert checked == {"strip": 60, "row": 56, "chroma": 60}      # all but the sizes of one strip / one macroblock row


def test_every_member_is_encodable_at_every_quality_the_gpu_tests_use(orc):
    import plane_oracle
    for t in gs.all_members():
        for content, quals in gs.TABLE_QUALITIES.items():
            for q in quals:
                for ch in (3, 4):
                    assert len(gs.record(orc, t, content, 0, q, ch)) > 48, (gs.name(t), content, q, ch)
    for t in gs.tile_set()[::9] + gs.strict_set():                # (the plane oracle walks blocks in Python)
        for content, quals in gs.TABLE_QUALITIES.items():
            try:
                gs.plane_record(orc, t, content, 0, quals[-1])
            except plane_oracle.Unencodable:
                pytest.fail(f"{gs.name(t)} {content}: planes unencodable")


# ---- a difference is named by its shape -------------------------------------------------------------------------------------
def test_a_difference_is_named_by_its_slice(orc):
    t = next(x for x in gs.tile_set() if (x.grid, x.s, x.m) == (1, 5, 2))
    n = 3
    want = [gs.record(orc, t, "q12", f) for f in range(n)]
    assert "records are equal" in gs.describe_difference(want, want, t.W, t.H, "full", n)
    starts = gs.slice_starts(want[1], 13)
    assert len(starts) == 13 and starts[0] == 44 and all(want[1][s:s + 4] == bytes((0, 0, 1, i + 1)) for i, s in enumerate(starts))
    got = list(want)
    rec = bytearray(want[1])
    rec[starts[10] + 9] ^= 0x10                                   # bit 75 of slice 10: bit 37 behind its header
    got[1] = bytes(rec)
    text = gs.describe_difference(got, want, t.W, t.H, "full", n)
    assert "frame 1, slice 10 (strip 10, strip 2 of tile column 1, which holds 5 strips" in text, text
    assert "at bit 37 behind the slice header" in text and "last column 5 strips, last row 2 macroblock rows" in text, text
    rec = bytearray(want[1])
    rec[starts[3] + 3] ^= 0x01                                    # the strip number
    got[1] = bytes(rec)
    text = gs.describe_difference(got, want, t.W, t.H, "full", n)
    assert "slice 3 (strip 3, strip 3 of tile column 0, which holds 8 strips" in text and "in the slice header" in text, text
    # a payload that holds the start code of the next strip: the walks from both ends differ, and the text says so
    rec = bytearray(want[1])
    rec[starts[4] + 20:starts[4] + 24] = bytes((0, 0, 1, 6))
    fake = bytes(rec)
    assert gs.slice_starts(fake, 13)[5] == starts[4] + 20 and gs.slice_starts_backwards(fake, 13) == starts
    rec[starts[8] + 9] ^= 0x10
    text = gs.describe_difference([want[0], bytes(rec), want[2]], [want[0], fake, want[2]], t.W, t.H, "full", n)
    assert "the payload holds a slice start code" in text and "frame 1" in text, text
    got = [want[0], want[2], want[1]]
    text = gs.describe_difference(got, want, t.W, t.H, "full", n)
    assert "frame 1" in text and "the record is the oracle's for frame 2" in text, text


# ---- the oracle against the real reference, even heights --------------------------------------------------------------------
@pytest.mark.reference
def test_oracle_matches_the_reference_on_the_even_height_members(ref, orc, tmp_path):
    """Two frames of the member's quality-12 content as JPEGs through the reference's driver; JPEG decoding happens on both
    sides, so what both encode is the decoded RGB (ref.dump_rgb)."""
    from ref_ffi import _check_folder, _make_folder
    members = [t for t in gs.tile_set() if t.H % 2 == 0]
    assert len(members) == 32 and {(t.s, t.grid) for t in members} == {(s, g) for s in range(1, 9) for g in (0, 1)}
    # the formula gives even widths where it gives even heights (k even): odd widths at even heights come from these six
    members += gs.odd_width_set()
    assert all(t.W % 2 == 1 and t.H % 2 == 0 for t in gs.odd_width_set()) and len(gs.odd_width_set()) == 6
    for t in members:
        d = _make_folder(tmp_path, f"{t.set}{t.k}", list(gs.pixels(t, "q12", 3, 2)))
        _, frames = _check_folder(ref, orc, d, 12, modes=("full",))
        assert frames[0].shape == (t.H, t.W, 3), gs.name(t)


# ---- recorded hashes --------------------------------------------------------------------------------------------------------
def test_oracle_gives_the_recorded_hashes(orc):
    gold = json.load(open(GOLDEN))["sha256"]
    members = gs.all_members()
    assert sorted(gold) == sorted(gs.name(t) for t in members) and len(gold) == 64 + 1 + 24 + 3 + 6
    assert sum(t.H % 2 for t in members if t.set == "tile") == 32                 # odd heights: the oracle alone
    for t in members:
        assert gs.digest(orc, t) == gold[gs.name(t)], gs.name(t)
