"""CPU pins of tests/input_families.py, the builder behind the three sweeps (tests/test_gpu_geometry.py,
tests/test_gpu_code_space.py, tests/test_gpu_hard_content.py):

  completeness  every tile-shaped kernel of the code object (source names k_, kt_, kp_ + encode / size_table / rd_table) is
                declared by a family of the geometry sweep's tile set; a kernel family added without a sweep family fails here.
  host side     at four tile-set members (one strip x one row; a whole tile; 2 x 2 grids with 3 x 1 and 7 x 3 in the last
                column / row) and both contents: the float patterns of every type and range give the pixels back under the
                rule; the yuy2 / uyvy / p010 frame bytes read through tests/sample_oracle.py give geometry_space.plane_record;
                the plane ranges of the kp- families are the first and last byte tests/sample_oracle.py's addressed_mask marks.
  restricted    every new family keeps the strips and macroblock rows of all 64 members."""
import re

import numpy as np
import pytest

import float_planes as fp
import geometry_space as gs
import input_families as fam
import sample_oracle

MEMBERS = [next(t for t in gs.tile_set() if (t.grid, t.s, t.m) == key) for key in ((0, 1, 1), (0, 8, 4), (1, 3, 1), (1, 7, 3))]
# kernels whose names match the pattern and that no family declares, each with its reason
EXCLUDED = {"k_size_table_sizes": "writes the size table out behind every k_size_table_* kernel: one workgroup per (frame, quality), no tile shape",
            "k_rd_table_sizes": "writes the rd table out behind every k_rd_table_* kernel: one workgroup per (frame, quality), no tile shape"}


# ---- completeness -----------------------------------------------------------------------------------------------------------
def _source_names():
    """The source names of the code object's kernels that match k[tp]?_(encode|size_table|rd_table)_\\w+, from the metadata
    notes: a mangled name carries each identifier behind its length."""
    from code_object import _code_object
    out = set()
    for name, _, _ in _code_object()[1]:
        m = re.search(r"\d(k[tp]?_(?:encode|size_table|rd_table)_[a-z0-9_]+)", name)    # (up to the I or E behind the identifier)
        if m:
            assert name[:m.start(1)].endswith(str(len(m.group(1)))), name
            out.add(m.group(1))
    return out


def test_the_tile_set_reaches_every_tile_shaped_kernel():
    import geometry_cases as geo
    found = _source_names()
    assert len(found) > 40, sorted(found)
    assert set(EXCLUDED) <= found
    declared = {k for f in geo.TILE_FAMILIES + geo.RUN_FAMILIES for k in fam.kernels(f)}
    # (both stagings of every name are reached because both contents run: quality 12 narrow, quality 90 wide)
    assert found - set(EXCLUDED) == declared, (sorted(found - set(EXCLUDED) - declared), sorted(declared - found))
    missing = [f for f in fam.NEW_FAMILIES if f not in geo.TILE_FAMILIES or f not in geo.PADDED_FAMILIES]
    assert not missing, missing


def test_kernel_names_by_family():
    assert fam.kernels("yuy2") == ("k_encode_step2", "k_size_table_step2", "k_rd_table_step2")
    assert fam.kernels("kt-planes-nv12") == ("kt_encode_planes", "kt_size_table_planes", "kt_rd_table_planes")
    assert fam.kernels("kp-rgbplanes-pitched") == ("kp_encode_rgb_planes", "kp_size_table_rgb_planes", "kp_rd_table_rgb_planes")
    assert fam.kernels("bfloat16-window")[0] == "k_encode_float_planes" and fam.kernels("rgb-fallback")[0] == "k_encode_tiles"


# ---- restricted -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", fam.NEW_FAMILIES)
def test_restricted_keeps_the_shape(family):
    base = fam.base_family(family)[1]
    for t in gs.tile_set() + gs.strict_set() + [gs.batch_member()]:
        r = gs.restricted(t, family)
        assert gs.shape(r.W, r.H, r.mode) == gs.shape(t.W, t.H, t.mode) and (t.W - r.W, t.H - r.H) in ((0, 0), (1, 0), (0, 1), (1, 1))
        if base != "planes-reference":
            assert r.W % 2 == 0, (family, gs.name(t))
        if base in ("planes-i420", "planes-nv12") + fam.SAMPLE_PRESETS:
            assert r.H % 2 == 0, (family, gs.name(t))
        assert r == gs.restricted(t, base)
    assert any(gs.restricted(t, "kp-planes-reference").W % 2 for t in gs.tile_set())


# ---- the host side ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", list(gs.CONTENTS))
@pytest.mark.parametrize("kind", fp.KINDS)
def test_float_patterns_give_the_pixels_back(kind, content):
    for i, t0 in enumerate(MEMBERS):
        t = gs.restricted(t0, kind + "-window")
        px = gs.pixels(t, content)
        for rng in fam.FLOAT_RANGES:
            bits = fam.float_bits(px, kind, rng, seed=i)
            assert bits.shape == (px.shape[0], 3, t.H, t.W) and bits.dtype == (np.uint32 if kind == "float32" else np.uint16)
            assert np.array_equal(fp.rule_bytes(bits, kind, rng).transpose(0, 2, 3, 1), px), (kind, rng, gs.name(t))
            # jitter noise, not exact images: most samples are not the type's nearest value to the byte itself
            plain = fam._round_to((px.transpose(0, 3, 1, 2).astype(np.float64) / fp.SCALE[rng]).astype(np.float32), kind)
            if kind != "bfloat16":
                assert (bits != plain).mean() > 0.5, (kind, rng, (bits != plain).mean())


@pytest.mark.parametrize("content", list(gs.CONTENTS))
@pytest.mark.parametrize("preset", fam.SAMPLE_PRESETS)
def test_sample_frames_give_the_plane_record(orc, preset, content):
    for t0 in MEMBERS:
        t = gs.restricted(t0, preset)
        xe, ye = fam.region(t.W, t.H, t.mode)
        Y, Cb, Cr = (p[:1] for p in gs.planes(t, content))
        host, lay, base = fam.sample_frames(preset, t.W, t.H, Y, Cb, Cr, fill_seed=1)
        got = sample_oracle.encode_layout(host[base:], lay, t.W, t.H, gs.FIRST, gs.CONTENTS[content][0], gs.omode(orc, t))
        assert got == gs.plane_record(orc, t, content, 0), (preset, gs.name(t))
        # another fill changes every kind of padding and no addressed byte
        other = fam.sample_frames(preset, t.W, t.H, Y, Cb, Cr, fill_seed=2)[0]
        mask = sample_oracle.addressed_mask(lay, xe, ye, lay["frame_stride"])
        a, b = host[base:base + lay["frame_stride"]], other[base:base + lay["frame_stride"]]
        assert np.array_equal(a[mask], b[mask]) and (a[~mask] != b[~mask]).mean() > 0.9
        assert (host[:base] != other[:base]).any() and (host[base + lay["frame_stride"]:] != other[base + lay["frame_stride"]:]).any()
        if preset == "p010":
            assert not mask[0::2].any()                           # the low byte of every word
        else:
            rows = mask.reshape(t.H, 2 * t.W)
            assert not rows[1::2, (1 if preset == "yuy2" else 0)::2].any()     # the chroma of odd picture rows


def _one_plane(offset, pitch, step):
    """A layout under which addressed_mask marks one plane alone: the plane as luma, and chroma inside it."""
    return dict(y_offset=offset, y_pitch=pitch, y_step=step, cb_offset=offset, cr_offset=offset, c_pitch=pitch, c_step=step)


@pytest.mark.parametrize("family", fam.KP_FAMILIES)
def test_plane_ranges_are_the_addressed_bytes(family):
    for t0 in MEMBERS + gs.strict_set()[1:2]:
        t = gs.restricted(t0, family)
        xe, ye = fam.region(t.W, t.H, t.mode)
        f = fam.plane_table_family(family)
        ranges = fam.plane_ranges(family, t.W, t.H, t.mode)
        e = f.encoder_layout(t.W, t.H)
        if f.rgb:
            one = [(_one_plane(e[k], e["row_pitch"], 1), (t.W, t.H), e[k]) for k in ("r_offset", "g_offset", "b_offset")]
            length = e["frame_stride"]
        else:
            o = f.oracle_layout(t.W, t.H)
            one = [(_one_plane(o["y_offset"], o["y_pitch"], 1), (xe, ye), e["y_offset"])]
            one += [(_one_plane(o[k], o["c_pitch"], o["c_step"]), (xe // 2, ye // 2), e[k]) for k in ("cb_offset", "cr_offset")]
            length = o["frame_stride"]
            whole = np.flatnonzero(sample_oracle.addressed_mask(o, xe, ye, length))
            assert np.array_equal(whole, np.unique(np.concatenate([r[3] for r in ranges])))
        for (lay, (w, h), offset), (v, lo, E, A) in zip(one, ranges):
            at = np.flatnonzero(sample_oracle.addressed_mask(lay, w, h, length))
            assert np.array_equal(at, np.sort(A)), (family, gs.name(t))
            assert at[0] == v + offset and at[-1] + 1 == v + E, (family, gs.name(t), at[0], at[-1], v, lo, E)
            assert lo == (offset if f.rgb else 0)                 # the header: an RGB plane's range starts at its offset
        # a block is exactly the union of its planes' ranges
        for (v0, length_, pointers, A), group in zip(fam._blocks(f, t.W, t.H, (xe, ye)), f.groups):
            assert v0 == min(ranges[p][0] + ranges[p][1] for p, _ in group)
            assert v0 + length_ == max(ranges[p][0] + ranges[p][2] for p, _ in group) == A.max() + 1
