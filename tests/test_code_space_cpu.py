"""CPU pins of tests/code_space.py: the census of the content that tests/test_gpu_code_space.py feeds the kernels.  As in
tests/test_hard_content_cpu.py these are conditions on the CONTENT — on what the oracle codes of it — not on the code under test:
a later edit of the generator cannot quietly take a table entry out of the GPU tests.  The census is also written to
profiles/r14_code_space_census.txt.

A pair (r, |L|) counts when it is the first coded pair of some block in BOTH signs.  Pinned, for the luma of the plane form and
for the luma of the grey pictures alike (the floors are those of the plain one-cosine construction: 2,752 and 6,822 pairs, 366
of level 128 and up; raising the amplitude where clipping falls short, as code_space._search does, gives more):
  narrow (qualities <= 76)  all 110 table entries; each of the 32 rows' first escape level; level 1 at every r in 32..61;
                            at least 2,700 pairs; no level beyond 127
  wide (qualities <= 92)    the same table and edge conditions; at least 6,500 pairs; at least 300 of level 128 and up, with
                            128, 129 and 255 among the levels
  chroma planes             all 110 table entries and the 32 first escape levels, in either set
  DC, planes                luma and chroma each hold every level 0..2042
  DC, grey pictures         luma holds every multiple of 256 up to 1792 and at least 1,600 distinct levels
  every frame               encodable at its own quality and at the lower ones the GPU tests ask tables for
The row lengths come from the oracle (code_space.row_lengths: a table code has at most 17 bits), not from the kernels' table."""
import os

import numpy as np
import pytest

import code_space as cs
import hard_content as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = {"narrow": 2700, "wide": 6500}
_records = {}


def _edge_conditions(orc, both, what):
    table, escapes = cs.table_entries(orc), cs.first_escapes(orc)
    assert len(table) == 110 and len(escapes) == 32
    assert not [e for e in table if e not in both], (what, [e for e in table if e not in both])
    assert not [e for e in escapes if e not in both], (what, [e for e in escapes if e not in both])


def _note(name, frames, c, both=None):
    line = f"{name}: {len(frames['qualities'])} frames at qualities {sorted(set(frames['qualities']), reverse=True)}, {c['blocks']} blocks\n"
    if both is not None:
        for plane, b in both.items():
            big = sorted({lv for _, lv in b if lv >= 128})
            line += (f"    {plane}: {len(b)} first pairs (r, |L|) in both signs, runs {len({r for r, _ in b})} of 62, largest level "
                     f"{max(lv for _, lv in b)}, {sum(lv >= 128 for _, lv in b)} pairs of level 128 and up"
                     + (f" (levels {big[0]}..{big[-1]})" if big else "") + "\n")
    line += f"    DC levels: luma {len(c['dc_luma'])} distinct ({min(c['dc_luma'])}..{max(c['dc_luma'])}), chroma {len(c['dc_chroma'])} distinct\n"
    _records[name] = line


def test_row_lengths_come_from_the_oracle(orc):
    """32 rows, 110 entries; every run from 32 up is an escape at level 1; row 0 ends at 39 (level 40 is its first escape)."""
    rows = cs.row_lengths(orc)
    assert len(rows) == 32 and sum(rows) == 110 and rows[0] == 39 and rows[1] == 18 and min(rows) == 1
    assert list(rows) == sorted(rows, reverse=True)


@pytest.mark.parametrize("form", ["planes", "grey"])
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_ac_set_census(orc, kind, form):
    frames = cs.ac_frames(orc, kind, form)
    n = len(frames["qualities"])
    assert frames["Y"].shape == (n, cs.H, cs.W) and max(frames["qualities"]) == cs.TOP[kind]
    assert frames["qualities"] == sorted(frames["qualities"], reverse=True)
    c = cs.census(orc, frames)
    both = cs.both_signs(c["first_luma"])
    _edge_conditions(orc, both, (kind, form, "luma"))
    assert not [r for r in range(32, 62) if (r, 1) not in both]
    assert len(both) >= FLOOR[kind], len(both)
    levels = {lv for _, lv in both}
    if kind == "narrow":
        assert max(abs(lv) for _, lv in c["first_luma"] | c["first_chroma"]) <= 127
    else:
        assert sum(lv >= 128 for _, lv in both) >= 300 and {128, 129, 255} <= levels
    noted = {"luma": both}
    if form == "planes":
        chroma = cs.both_signs(c["first_chroma"])
        _edge_conditions(orc, chroma, (kind, form, "chroma"))
        noted["chroma"] = chroma
    else:
        assert np.array_equal(frames["rgb"][..., 0], frames["rgb"][..., 2]) and np.array_equal(frames["rgb"][..., 0], frames["rgb"][..., 1])
    _note(f"{kind} set, {form}", frames, c, noted)
    # the blocks the census found are the blocks the generator placed: every accepted (r, L) is the first pair of a luma block
    assert {(r, lv) for _, r, lv, _ in cs.ac_blocks(orc, kind, form)} <= c["first_luma"]


@pytest.mark.parametrize("form", ["planes", "grey"])
def test_dc_census(orc, form):
    frames = cs.dc_frames(orc, form)
    assert frames["qualities"] == [cs.DC_Q] * cs.DC_FRAMES + [cs.DC_LOW_Q]
    assert orc.scale_qmatrix(cs.DC_Q)[0] == 1 and orc.scale_qmatrix(cs.DC_LOW_Q)[0] == 8
    c = cs.census(orc, frames)
    if form == "planes":
        assert c["dc_luma"] >= set(range(2043)), sorted(set(range(2043)) - c["dc_luma"])[:10]
        assert c["dc_chroma"] >= set(range(2043)), sorted(set(range(2043)) - c["dc_chroma"])[:10]
    else:
        assert c["dc_luma"] >= set(range(0, 1793, 256)) and len(c["dc_luma"]) >= 1600, len(c["dc_luma"])
    _note(f"DC levels, {form}", frames, c)


def test_dc_block_has_the_dc_coefficient_it_is_built_for(orc):
    for k in cs.DC_LEVELS:
        assert orc.fdct(cs.dc_block(k))[0] == k, k


@pytest.mark.parametrize("form", ["planes", "grey"])
def test_every_frame_is_encodable_where_it_is_coded(orc, form):
    """At its own quality (per-frame encodes), and at 20 and 50 below it (the tables of tests/test_gpu_code_space.py)."""
    for frames in (cs.ac_frames(orc, "narrow", form), cs.ac_frames(orc, "wide", form), cs.dc_frames(orc, form)):
        for f, q in enumerate(frames["qualities"]):
            for lower in sorted({20, 50, q}):
                if lower <= q:
                    assert cs.frame_encodable(orc, frames, f, lower), (form, f, q, lower)


def test_a_difference_is_named_by_its_block(orc):
    """describe_difference on a record with one bit flipped inside a known block: the text names that block's pair."""
    import plane_oracle
    frames = cs.ac_frames(orc, "narrow", "planes")
    f = 0
    frame = np.concatenate([frames[p][f].reshape(-1) for p in ("Y", "Cb", "Cr")])
    lay = dict(y_offset=0, cb_offset=cs.W * cs.H, cr_offset=cs.W * cs.H * 5 // 4, y_pitch=cs.W, c_pitch=cs.W // 2, c_step=1, frame_stride=frame.size)
    want = plane_oracle.encode_layout(frame, lay, cs.W, cs.H, 0, frames["qualities"][f], orc.MODE_FULL)
    names = cs.block_names(orc, frames, f)
    levels = cs.frame_levels(orc, frames, f)
    # strip 0, macroblock 3, block 1: its bits start behind the strip's 38, three macroblocks, this one's 2 and block 0
    at = 38 + sum(2 * (i % 6 == 0) + len(orc.encode_block_bits(i % 6 < 4, levels[i])[1]) for i in range(19))
    got = bytearray(want)
    bit = at + 1
    got[44 + bit // 8] ^= 0x80 >> (bit % 8)
    text = cs.describe_difference(orc, frames, f, bytes(got), want)
    luma, dc, first = names[19]
    assert f"macroblock 3, block 1 (luma): DC level {dc}, first pair (r = {first[0]}, L = {first[1]})" in text, text
    assert f"in the DC code of level {dc}" in text, text
    # a bit of the block's first AC code, in a record that is also one byte longer (the header's length field differs too)
    got = bytearray(want) + b"\0"
    got[4:6] = ((int.from_bytes(want[4:6], "big") + 1) & 0xffff).to_bytes(2, "big")
    bit = at + hc._dc_bits(orc, 1, dc)
    got[44 + bit // 8] ^= 0x80 >> (bit % 8)
    text = cs.describe_difference(orc, frames, f, bytes(got), want)
    assert f"in the code of pair 0 of the block, (r = {first[0]}, L = {first[1]})" in text, text
    assert "records are equal" in cs.describe_difference(orc, frames, f, want, want)


def test_zz_census_record_is_written(orc):
    """Runs last in this module (pytest keeps file order): the censuses noted above, to profiles/r14_code_space_census.txt."""
    if len(_records) < 6:                                 # selected alone: take the censuses now
        for form in ("planes", "grey"):
            for kind in ("narrow", "wide"):
                test_ac_set_census(orc, kind, form)
            test_dc_census(orc, form)
    text = ("# Census of the code-space content (tests/code_space.py), written by tests/test_code_space_cpu.py from the CPU oracle.\n"
            "# A pair (r, |L|), r = zeros before the level minus 1, counts when it is the FIRST coded pair of some block in both signs.\n"
            f"# Table: 110 entries in rows of {list(cs.row_lengths(orc))}.\n"
            + "".join(_records[k] for k in sorted(_records)))
    path = os.path.join(ROOT, "profiles", "r14_code_space_census.txt")
    try:
        with open(path, "w") as fh:
            fh.write(text)
    except OSError:                                       # a read-only checkout keeps the committed record
        pass
    assert "first pairs (r, |L|) in both signs" in open(path).read()
