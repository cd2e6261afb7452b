"""CPU pins of tests/hard_content.py: the census of the content that tests/test_gpu_hard_content.py feeds the kernels.  The
conditions are conditions on the CONTENT (does it still make the reference code escapes, long runs, long blocks?), not
measurements of the code under test: a later edit of the generator cannot quietly turn the GPU tests back into DC-only tests.
Each content's census is also written to profiles/r11_hard_content_census.txt.

Per 352x288 sweep frame, aimed at quality q and counted at q (for plane sweeps separately over luma and over chroma blocks):
  q = 12, 50, 76, 92   every run value 0..61 coded, codes of both signs, encodable
  q = 50, 76, 92       at least 100 blocks over 64 bits, at least one over 128
  q = 76               at least 100 20-bit escapes, no level beyond +-127, at least 300 distinct (run, |level|) pairs
  q = 92               at least 50 28-bit escapes, at least 100 20-bit escapes
Two conditions one would want are NOT pinned, for reasons in the content, not in the code under test:
  - blocks over 64 / 128 bits are not required at quality 12.  Its AC divisors start at 67, and the samples of a block span
    0..255, which bounds the sum of its coefficient magnitudes by a few hundred: a block carries five or six levels of 1 or 2
    there, and codes of that size behind runs below 32 are table codes of 3 to 17 bits.  Measured: 120 luma blocks over 64 bits,
    none over 128 (the longest has 86 bits); 62 of the 792 chroma blocks over 64.
  - "some blocks with DC level 0 code an AC level" is replaced by its opposite: the reference's arithmetic cannot
    produce one (tests/hard_content.py's docstring has the inequality; test_dc_level_zero_never_codes_an_ac_level searches for
    a counter-example with the oracle's DCT at every quality).  The census pins the count at 0, and that the sweep does carry
    blocks with DC level 0 (which take the `prev = -1` start without a code behind it)."""
import os

import numpy as np
import pytest

import hard_content as hc
import plane_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 352, 288
QUALITIES = (12, 50, 76, 92)
_records = {}


def _note(name, c):
    bits = np.asarray(c["bits"])
    _records[name] = (f"{name}: {c['blocks']} blocks, {len(c['pairs'])} AC codes ({len(c['pairs']) / c['blocks']:.2f} per block), "
                      f"runs {len(c['runs'])} of 62 (max {max(c['runs'], default=-1)}), {len(c['distinct'])} distinct (run, |level|), "
                      f"largest level {c['max_level']}, +{c['positive']} / -{c['negative']}\n"
                      f"    20-bit escapes {c['esc20']}, 28-bit escapes {c['esc28']}, blocks over 64 bits {c['over64']}, over 128 bits "
                      f"{c['over128']}, longest {bits.max()} bits, DC level 0 with an AC code {c['dc0_ac']}\n")
    return c


def _pinned(c, q, dc0_blocks):
    assert c["runs"] >= set(range(62)), sorted(set(range(62)) - c["runs"])
    assert c["positive"] > 0 and c["negative"] > 0
    assert c["dc0_ac"] == 0
    if q < 50:
        assert dc0_blocks > 0                    # blocks of a few lit pixels on black: DC level 0 (no AC code can follow)
    if q >= 50:
        assert c["over64"] >= 100 and c["over128"] >= 1, (c["over64"], c["over128"])
    if q == 76:
        assert c["esc20"] >= 100 and c["max_level"] <= 127 and len(c["distinct"]) >= 300, (c["esc20"], c["max_level"], len(c["distinct"]))
        assert c["esc28"] == 0
    if q == 92:
        assert c["esc28"] >= 50 and c["esc20"] >= 100, (c["esc28"], c["esc20"])
        assert c["max_level"] >= 128


@pytest.mark.parametrize("q", QUALITIES)
def test_sweep_picture_census(orc, q):
    pic = hc.sweep_picture(np.random.default_rng(q), W, H, q, orc)
    assert pic.shape == (H, W, 3) and pic.dtype == np.uint8 and np.array_equal(pic[..., 0], pic[..., 1])
    assert hc.frame_encodable(orc, pic, q)
    co = orc.frame_coefficients(pic, W, H, q, orc.MODE_FULL)
    c = _note(f"sweep_picture 352x288 aimed at {q}, counted at {q}", hc.census(orc, co))
    _pinned(c, q, int((co[:, 0] == 0).sum()))
    assert all(len(orc.encode_frame(pic, W, H, 0, lower, orc.MODE_FULL)) > 48 for lower in (1, 20) if lower < q)


@pytest.mark.parametrize("q", QUALITIES)
def test_plane_sweep_census(orc, q):
    """Luma and chroma blocks separately: the chroma planes are built by the same rule, at a quarter of the blocks each."""
    Y, Cb, Cr = hc.plane_sweep(np.random.default_rng(q + 1), W, H, q, orc)
    assert Y.shape == (H, W) and Cb.shape == Cr.shape == (H // 2, W // 2)
    luma = hc.plane_coefficients(orc, Y, q)
    chroma = np.concatenate([hc.plane_coefficients(orc, Cb, q), hc.plane_coefficients(orc, Cr, q)])
    _pinned(_note(f"plane_sweep 352x288 luma aimed at {q}, counted at {q}", hc.census(orc, luma, 1)), q, int((luma[:, 0] == 0).sum()))
    _pinned(_note(f"plane_sweep 352x288 chroma aimed at {q}, counted at {q}", hc.census(orc, chroma, 0)), q, int((chroma[:, 0] == 0).sum()))


@pytest.mark.parametrize("size", [(352, 288), (176, 208)])
def test_gpu_content_is_encodable_and_hard_at_every_quality_it_is_coded_at(orc, size):
    """hard_frames / hard_planes: frames 0..2 at every quality of both tables and at the encoder's, the extreme-pattern frame up
    to EXTREME_Q; and at the top quality each frame still codes escapes and long blocks (the extreme one: levels of 128 up)."""
    w, h = size
    frames = hc.hard_frames(orc, w, h)
    Y, Cb, Cr = hc.hard_planes(orc, w, h)
    assert frames.shape == (4, h, w, 3) and Y.shape == (4, h, w) and Cb.shape == Cr.shape == (4, h // 2, w // 2)
    names = ("sweep 92", "heavy 10/130/0.4", "heavy 16/120", "extreme patterns")
    plane_names = ("plane_sweep 92", "plane_sweep 76 kept encodable at 92", "heavy 10/130/0.4 planes", "extreme-pattern planes")
    for f in range(4):
        top = hc.ENCODER_Q if f < 3 else hc.EXTREME_Q
        for q in sorted(set(hc.TABLE_NARROW + hc.TABLE_WIDE + (hc.ENCODER_Q,))):
            if q <= top:
                assert hc.frame_encodable(orc, frames[f], q), (f, q)
                assert all(hc.plane_encodable(orc, p[f], q, luma) for p, luma in ((Y, 1), (Cb, 0), (Cr, 0))), (f, q)
        assert not (f == 3 and hc.frame_encodable(orc, frames[f], hc.ENCODER_Q))
        for q in ((76, top) if f < 3 else (76, 77)):
            c = _note(f"hard_frames {w}x{h} [{f}] {names[f]}, counted at {q}",
                      hc.census(orc, orc.frame_coefficients(frames[f], w, h, q, orc.MODE_FULL)))
            chroma = np.concatenate([hc.plane_coefficients(orc, Cb[f], q), hc.plane_coefficients(orc, Cr[f], q)])
            pl = _note(f"hard_planes {w}x{h} [{f}] {plane_names[f]} luma, counted at {q}", hc.census(orc, hc.plane_coefficients(orc, Y[f], q), 1))
            pc = _note(f"hard_planes {w}x{h} [{f}] {plane_names[f]} chroma, counted at {q}", hc.census(orc, chroma, 0))
            for x in (c, pl, pc):
                if f < 3 and q == top:
                    assert x["esc20"] >= 50 and x["over64"] >= 20, (f, q, x["esc20"], x["over64"])
                if q == 77 or (q == 92 and f < 2):
                    assert x["esc28"] >= 10, (f, q, x["esc28"])
                if q == 76:
                    assert x["esc28"] == 0 and x["max_level"] <= 127


def test_dc_level_zero_never_codes_an_ac_level(orc):
    """For every quality and every AC position, both signs: the block of samples in 0..255 that maximises that coefficient
    under the largest pixel sum whose DC level is still 0 (greedy: brightest where the basis function is largest) quantises
    to level 0 there.  So `prev = -1` in block_bits_pass1 never meets a code, in any content."""
    i, j = np.divmod(np.arange(64), 8)
    seen_divisors = set()
    for q in range(1, 101):
        div = orc.scale_qmatrix(q)
        if tuple(div) in seen_divisors:
            continue
        seen_divisors.add(tuple(div))
        budget = 8 * int(div[0]) - 17                     # (S + 16) >> 3 < q[0]  <=>  S <= 8 q[0] - 17
        if budget < 1:
            continue
        for k in range(1, 64):
            u, v = divmod(k, 8)
            basis = np.cos((2 * i + 1) * u * np.pi / 16) * np.cos((2 * j + 1) * v * np.pi / 16)
            for sign in (1, -1):
                px = np.zeros(64, np.int64)
                left = budget
                for at in np.argsort(-sign * basis):
                    if left <= 0 or sign * basis[at] <= 0:
                        break
                    px[at] = min(255, left)
                    left -= px[at]
                d = orc.fdct(px.astype(np.uint8))
                assert d[0] // div[0] == 0, (q, k)
                assert int(d[k] / div[k]) == 0, (q, k, sign, int(d[k]), int(div[k]))


@pytest.mark.parametrize("q", [50, 76, 92])
def test_plane_oracle_equals_the_oracle_on_hard_grey_pictures(orc, q):
    """The second checker on hard content, as tests/test_planes_abi.py pins it on its own: the luma plane of a plane sweep as a
    grey RGB picture, converted by the oracle — plane_oracle on those planes gives the oracle's record of the picture."""
    Y = hc.plane_sweep(np.random.default_rng(q + 1), W, H, q, orc)[0]
    rgb = np.ascontiguousarray(np.repeat(Y[..., None], 3, 2))
    if not hc.frame_encodable(orc, rgb, q):               # (the converted luma is within 1 of Y: a level at the very edge)
        rgb = hc.sweep_picture(np.random.default_rng(q + 1), W, H, q, orc)
    want = orc.encode_frame(rgb, W, H, 300, q, orc.MODE_FULL)
    frame = np.concatenate(orc.convert(rgb))
    assert plane_oracle.encode_layout(frame, plane_oracle.reference_layout(W, H), W, H, 300, q, orc.MODE_FULL) == want


def test_plane_oracle_record_length_equals_the_census_bits_on_hard_chroma(orc):
    """Planes that no RGB picture maps to (hard chroma): the length of plane_oracle's record is the census's bit count — 38
    header bits per strip and 2 per macroblock plus the blocks' bits, padded to a byte per strip, 44 header and 4 trailer
    bytes.  Two independent walks of the same blocks agree."""
    w, h, q = 176, 208, 92
    Y, Cb, Cr = (p[0] for p in hc.hard_planes(orc, w, h))
    frame = np.concatenate([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)])
    lay = dict(y_offset=0, cb_offset=w * h, cr_offset=w * h + w * h // 4, y_pitch=w, c_pitch=w // 2, c_step=1, frame_stride=frame.size)
    rec = plane_oracle.encode_layout(frame, lay, w, h, 0, q, orc.MODE_FULL)
    bits = {"y": np.asarray(hc.census(orc, hc.plane_coefficients(orc, Y, q), 1)["bits"]).reshape(h // 8, w // 8),
            "cb": np.asarray(hc.census(orc, hc.plane_coefficients(orc, Cb, q), 0)["bits"]).reshape(h // 16, w // 16),
            "cr": np.asarray(hc.census(orc, hc.plane_coefficients(orc, Cr, q), 0)["bits"]).reshape(h // 16, w // 16)}
    total = 44 + 4
    for s in range(w // 16):
        n = 38 + (h // 16) * 2 + bits["y"][:, 2 * s:2 * s + 2].sum() + bits["cb"][:, s].sum() + bits["cr"][:, s].sum()
        total += (int(n) + 7) // 8
    assert len(rec) == total


def test_zz_census_record_is_written(orc):
    """Runs last in this module (pytest keeps file order): the censuses noted above, to profiles/r11_hard_content_census.txt."""
    if len(_records) < 44:                                # selected alone: take the censuses now
        for q in QUALITIES:
            test_sweep_picture_census(orc, q)
            test_plane_sweep_census(orc, q)
        for size in ((352, 288), (176, 208)):
            test_gpu_content_is_encodable_and_hard_at_every_quality_it_is_coded_at(orc, size)
    text = ("# Census of the hard entropy content (tests/hard_content.py), written by tests/test_hard_content_cpu.py from the CPU oracle.\n"
            "# run = zeros before a coded level, minus 1; escapes are the 20- and 28-bit codes of levels outside the table.\n"
            + "".join(_records[k] for k in sorted(_records)))
    path = os.path.join(ROOT, "profiles", "r11_hard_content_census.txt")
    try:
        with open(path, "w") as fh:
            fh.write(text)
    except OSError:                                       # a read-only checkout keeps the committed record
        pass
    assert "28-bit escapes" in open(path).read()
