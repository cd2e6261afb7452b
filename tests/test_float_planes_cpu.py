"""CPU checks of the float plane rule (include/mpeg1_hip.h, "Float plane layout"; tests/float_planes.py): the numpy rule against
exact rational arithmetic; the census of inputs that separate the rule from each wrong neighbour (the product rounded in fp16,
the product in double, floor(x * 255 + 0.5), ties half-up, truncation); the tie picture, whose oracle records tell the three tie
roundings apart; and the pure Python mirrors of the preset and of the stride helper."""
import numpy as np
import pytest

import float_planes as fp


# ---- the rule against exact arithmetic --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["unit", "byte"])
@pytest.mark.parametrize("kind", ["float16", "bfloat16"])
def test_rule_equals_exact_arithmetic_on_every_16_bit_pattern(kind, rng):
    p = fp.all_patterns(kind)
    got = fp.rule_bytes(p, kind, rng)
    wrong = [hex(int(v)) for v in p if fp.exact_byte(int(v), kind, rng) != got[int(v)]]
    assert not wrong, wrong[:10]


def test_rule_equals_exact_arithmetic_on_fp32_boundaries_ties_specials_and_a_sample():
    b = fp.boundary_values()
    got = fp.rule_bytes(b, "float32", "unit")
    assert [fp.exact_byte(int(v), "float32", "unit") for v in b] == got.tolist()
    t = fp.ties_byte_range("float32")
    assert [fp.exact_byte(int(v), "float32", "byte") for v in t] == fp.rule_bytes(t, "float32", "byte").tolist()
    s = fp.special_f32()
    for rng in ("unit", "byte"):
        assert [fp.exact_byte(int(v), "float32", rng) for v in s] == fp.rule_bytes(s, "float32", rng).tolist()
    g = np.random.default_rng(7)
    # 10,000 random fp32 values: half of them random patterns (every exponent), half in the range where the byte is not 0 or 255
    r = np.concatenate([g.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32),
                        g.uniform(-0.1, 1.1, 5000).astype(np.float32).view(np.uint32)])
    got = fp.rule_bytes(r, "float32", "unit")
    assert [fp.exact_byte(int(v), "float32", "unit") for v in r] == got.tolist()
    assert len(np.unique(got)) == 256


def test_edge_cases_the_definition_names():
    s = fp.special_f32()
    for rng in ("unit", "byte"):
        got = dict(zip((int(v) for v in s), fp.rule_bytes(s, "float32", rng).tolist()))
        assert got[0x7f800000] == 255 and got[0x7f7fffff] == 255                    # +inf, FLT_MAX
        for v in (0x00000000, 0x80000000, 0xff800000, 0xff7fffff, 0x007fffff, 0x807fffff, 0x00000001, 0x80000001,
                  0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fa5a5a5, 0xffffffff, 0x7fffffff, 0x7fc12345):
            assert got[v] == 0, hex(v)
    for kind in ("float16", "bfloat16"):
        p = fp.all_patterns(kind)
        f = fp.to_f32(p, kind)
        for rng in ("unit", "byte"):
            b = fp.rule_bytes(p, kind, rng)
            assert not b[np.isnan(f)].any() and not b[np.signbit(f)].any()
            assert (b[np.isposinf(f)] == 255).all()
            tiny = np.abs(f) < np.float32(2.0 ** -14 if kind == "float16" else 2.0 ** -126)     # zeros and denormals
            assert tiny.sum() > 2 and not b[tiny].any()


# ---- the census: inputs that separate the rule from its neighbours -----------------------------------------------------------
def test_product_rounded_in_fp16_differs_on_124_patterns():
    p = fp.all_patterns("float16")
    with np.errstate(all="ignore"):
        h = p.view(np.float16) * np.float16(255)
        assert h.dtype == np.float16
        alt = np.clip(np.where(np.isnan(h), 0, np.rint(h.astype(np.float32))), 0, 255).astype(np.uint8)
    assert int((alt != fp.rule_bytes(p, "float16", "unit")).sum()) == 124


def test_product_in_double_and_floor_of_half_added_differ_on_the_boundary_values():
    b = fp.boundary_values()
    x = b.view(np.float32)
    rule = fp.rule_bytes(b, "float32", "unit")
    in_double = np.clip(np.rint(x.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    assert int((in_double != rule).sum()) == 128
    half_added = np.clip(np.floor(x * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.uint8)
    assert int((half_added != rule).sum()) == 130


@pytest.mark.parametrize("kind", fp.KINDS)
def test_ties_of_range_byte(kind):
    t = fp.ties_byte_range(kind)
    k = np.arange(len(t))
    assert len(t) == (128 if kind == "bfloat16" else 255)
    assert np.array_equal(fp.to_f32(t, kind), k.astype(np.float32) + np.float32(0.5))        # exact in the type
    got = fp.rule_bytes(t, kind, "byte").astype(np.int64)
    assert np.array_equal(got, k + (k & 1))                                                  # the even neighbour
    assert (got != k + 1).sum() == (len(k) + 1) // 2 and (got != k).sum() == len(k) // 2     # not half-up, not truncation


@pytest.mark.parametrize("kind,pattern", [("float16", 0x3800), ("bfloat16", 0x3f00)])
def test_one_tie_of_range_unit_per_16_bit_type(kind, pattern):
    """Exactly one pattern whose fp32 product with 255 is a tie between two bytes: 0.5 -> 127.5 -> 128."""
    p = fp.all_patterns(kind)
    with np.errstate(all="ignore"):
        t = fp.to_f32(p, kind) * np.float32(255)
        tie = np.isfinite(t) & (t > 0) & (t < 255) & (t - np.floor(t) == np.float32(0.5))
    assert [int(v) for v in p[tie]] == [pattern]
    assert fp.rule_bytes(p[tie], kind, "unit").tolist() == [128]


# ---- the tie picture --------------------------------------------------------------------------------------------------------
def test_tie_picture_separates_the_three_roundings_in_the_record(orc):
    k, even = fp.tie_picture("even")
    assert k.shape == (256, 256) and sorted(set(k.ravel().tolist())) == list(range(255))
    pictures = {r: fp.tie_picture(r)[1] for r in ("even", "up", "down")}
    for kind in fp.KINDS:       # the samples of every type give the "even" picture by the rule
        samples, want = fp.tie_picture_samples(kind)
        assert np.array_equal(fp.rule_bytes(samples, kind, "byte").transpose(1, 2, 0), want)
    assert np.array_equal(fp.tie_picture_samples("float32")[1], even)
    for Q in (12, 100):
        rec = {r: orc.encode_frame(np.ascontiguousarray(px), 256, 256, 0, Q, orc.MODE_FULL) for r, px in pictures.items()}
        assert rec["even"] != rec["up"] and rec["even"] != rec["down"] and rec["up"] != rec["down"], Q
    # bf16's picture (k % 128) separates them too
    k7 = k % 128
    for Q in (12, 100):
        rec = [orc.encode_frame(np.ascontiguousarray(np.repeat(b.astype(np.uint8)[:, :, None], 3, axis=2)), 256, 256, 0, Q, orc.MODE_FULL)
               for b in (k7 + (k7 & 1), k7 + 1, k7)]
        assert len(set(rec)) == 3, Q


def test_boundary_picture_separates_double_and_floor_in_the_record(orc):
    samples, want = fp.boundary_picture()
    x = samples[0].view(np.float32)
    in_double = np.clip(np.rint(x.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    half_added = np.clip(np.floor(x * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.uint8)
    rec = [orc.encode_frame(np.ascontiguousarray(np.repeat(b[:, :, None], 3, axis=2)), 256, 256, 0, 100, orc.MODE_FULL)
           for b in (want[:, :, 0], in_double, half_added)]
    assert rec[0] != rec[1] and rec[0] != rec[2]


# ---- the pure mirrors ---------------------------------------------------------------------------------------------------------
def test_preset_and_strides_are_the_byte_layout_times_the_sample_size():
    from ec504_imageencoder_amd import float_plane_layout_preset, float_plane_strides, rgb_plane_layout_preset, rgb_plane_strides
    from ec504_imageencoder_amd.encoder import FLOAT_PLANE_LAYOUT_FIELDS
    assert FLOAT_PLANE_LAYOUT_FIELDS == ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride", "sample", "range")
    assert float_plane_layout_preset(48, 16, "rgb", "float16") == dict(
        r_offset=0, g_offset=1536, b_offset=3072, row_pitch=96, frame_stride=4608, sample=0, range=0)
    assert float_plane_layout_preset(48, 16, "bgr", "bfloat16", "byte") == dict(
        r_offset=3072, g_offset=1536, b_offset=0, row_pitch=96, frame_stride=4608, sample=1, range=1)
    assert float_plane_layout_preset(48, 16, "gbr", "float32") == dict(
        r_offset=6144, g_offset=0, b_offset=3072, row_pitch=192, frame_stride=9216, sample=2, range=0)
    for code, (dtype, S) in enumerate((("float16", 2), ("bfloat16", 2), ("float32", 4))):
        for order in ("rgb", "bgr", "gbr"):
            want = {k: v * S for k, v in rgb_plane_layout_preset(144, 80, order).items()}
            assert float_plane_layout_preset(144, 80, order, dtype, "byte") == dict(want, sample=code, range=1)
        # the window x[:, :, 5:5+32, 9:9+48] of a contiguous [2, 4, 70, 101] tensor, strides in elements
        shape, strides = (2, 4, 32, 48), (28280, 7070, 101, 1)
        want = {k: v * S for k, v in rgb_plane_strides(shape, strides, (2, 1, 0)).items()}
        assert float_plane_strides(shape, strides, dtype, (2, 1, 0)) == dict(want, sample=code, range=0)
        assert want["row_pitch"] == 101 * S and want["r_offset"] == 2 * 7070 * S
    for bad in (dict(dtype="float64"), dict(dtype="uint8"), dict(dtype="float16", range="full"), dict(dtype="float16", order="rbg")):
        args = dict(dict(order="rgb", dtype="float16", range="unit"), **bad)
        with pytest.raises(ValueError):
            float_plane_layout_preset(48, 16, args["order"], args["dtype"], args["range"])
    with pytest.raises(ValueError):
        float_plane_strides((2, 3, 32, 48), (4608, 1536, 48, 2), "float32")     # every other sample
    with pytest.raises(ValueError):
        float_plane_strides((2, 3, 32, 48), (4608, 1536, 47, 1), "float32")     # a pitch below W


def test_the_torch_dtype_names_the_sample_type():
    torch = pytest.importorskip("torch")
    from ec504_imageencoder_amd import float_plane_layout_preset
    for dtype, code in ((torch.float16, 0), (torch.bfloat16, 1), (torch.float32, 2)):
        assert float_plane_layout_preset(16, 16, "rgb", dtype)["sample"] == code
    with pytest.raises(ValueError):
        float_plane_layout_preset(16, 16, "rgb", torch.float64)
