"""CPU-side checks of the downscale word layout's C ABI (m1v_downscale_word_layout_preset / m1v_set_downscale_word_layout /
m1v_downscale_word_layout_in_force / m1v_downscale_words_to_i420_device, include/mpeg1_hip.h): declared, exported and bound; the
struct's size and offsets; the preset against the Python mirror and against the header's table; the header's and the kernel
header's text; and the gfx950 code object holds the kernels of csrc/m1v_downscale_words.h — 12 tile kernels and 1 bytes kernel,
without scratch, without a MODE switch and without fp64, at four waves per SIMD or more, with names that no other code-object test
counts — each of them reached by the sweeps of tests/test_gpu_downscale_word_sweeps.py."""
import ctypes as C
import os
import re

from code_object import EXISTING, RGB_PLANES_COUNTED, SAMPLE_LAYOUT_COUNTED, _code_object, _ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride", "factor", "shift")
SYMBOLS = ("m1v_downscale_word_layout_preset", "m1v_set_downscale_word_layout", "m1v_downscale_word_layout_in_force",
           "m1v_downscale_words_to_i420_device")
ROWS = ("encode", "size_table", "rd_table")
SIZES = ((16, 16), (48, 32), (354, 144), (1920, 1080), (3840, 2160))
# what the code-object tests of the other layouts count kernels by: no new mangled name may contain one
TAKEN = EXISTING + RGB_PLANES_COUNTED + SAMPLE_LAYOUT_COUNTED + ("k_downscale_", "k_half_planes_", "k_float_", "_rgb_planes", "_step2",
                                                                 "k_encode_planes")
# the completeness pattern of tests/test_input_families_cpu.py
TILE_SHAPED = r"\d(k[tp]?_(?:encode|size_table|rd_table)_[a-z0-9_]+)"


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, downscale_word_layout_preset
    from ec504_imageencoder_amd.encoder import DOWNSCALE_WORD_LAYOUT_FIELDS
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_downscale_word_layout\s*\{(.*?)\}\s*m1v_downscale_word_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip()
               for n in re.sub(r"^\s*(uint64_t|int32_t)", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS == DOWNSCALE_WORD_LAYOUT_FIELDS, members
    # the new section stands behind the downscale plane layout's struct and prototypes, whose own section is unchanged up to there
    assert text.index("} m1v_downscale_plane_layout;") < text.index("int m1v_downscale_planes_to_i420_device(") < \
        text.index("/* Downscale word layout") < text.index("} m1v_downscale_word_layout;")
    assert re.search(r"enum\s*\{\s*M1V_WORDS_P010\s*=\s*0,\s*M1V_WORDS_I010\s*=\s*1,\s*M1V_WORDS_I012\s*=\s*2,\s*M1V_WORDS_I016\s*=\s*3\s*\}", code)
    assert (_ffi.WORDS_P010, _ffi.WORDS_I010, _ffi.WORDS_I012, _ffi.WORDS_I016) == (0, 1, 2, 3)
    declared = re.findall(r"\b(m1v_\w+)\s*\(", code)
    assert sorted(set(declared)) == sorted(_ffi.MPEG1_HIP_SYMBOLS)
    L = _ffi.lib()
    for name in SYMBOLS:
        assert name in declared and name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    S = _ffi.DownscaleWordLayout
    assert tuple(n for n, _ in S._fields_) == FIELDS
    assert C.sizeof(S) == 64
    assert [getattr(S, n).offset for n in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert [getattr(S, n).size for n in FIELDS] == [8] * 7 + [4, 4]
    assert list(L.m1v_downscale_word_layout_preset.argtypes) == [C.c_int] * 4 + [C.POINTER(S)]
    assert list(L.m1v_set_downscale_word_layout.argtypes) == [C.c_void_p, C.POINTER(S)]
    assert list(L.m1v_downscale_word_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(S)]
    assert list(L.m1v_downscale_words_to_i420_device.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert callable(Mpeg1Encoder.set_downscale_word_layout) and callable(Mpeg1Encoder.downscale_words_to_i420)
    assert isinstance(Mpeg1Encoder.downscale_word_layout, property)
    assert callable(downscale_word_layout_preset)


def test_header_carries_the_definition_the_read_contract_and_what_is_not_covered():
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    section = text[text.index("/* Downscale word layout"):text.index("} m1v_downscale_word_layout;")]
    for phrase in ("F + y_offset + Y * y_pitch + 2 * X", "F + p_offset + V * c_pitch + U * c_step",
                   "a = (w(2x, 2y) + w(2x+1, 2y) + w(2x, 2y+1) + w(2x+1, 2y+1) + 2) >> 2", "sample = min(a >> shift, 255)",
                   "rounds half up", "the >> shift truncates", "16-bit little-endian word", "u < width / 2",
                   "box filter per plane", "no chroma-siting correction", "M1V_PLANES_I420 frame of those rendition samples", "channels = 3",
                   "[F, F + E) rounded up to the next 4-byte boundary", "never influence the output",
                   "the other component's words of a c_step = 4 plane",
                   "rows = 2 * ye for luma and ye for chroma", "4 * xe for luma and (xe - 1) * c_step + 2 for chroma",
                   "shift outside 0 .. 8", "c_step other than 2 or 4", "more than 3 bytes apart", "frame_stride == 0",
                   "0 < y_pitch < 4 * width", "0 < c_pitch < width * c_step", "frame_stride < E",
                   "ask m1v_downscale_word_layout_in_force", "reads the whole source",
                   "factor 4 and other filters", "sources of odd extent", "big-endian", "4:2:2 and 4:4:4 word sources (P210, Y210, yuv422p10le)",
                   "rounding instead of truncation at the shift", "a\n * frame table or a plane table", "the host-buffer", "the folder CLI",
                   "several renditions in one pass"):
        assert phrase in section, phrase
    # the older sections still say what they do not cover
    older = text[text.index("/* Downscale plane layout"):text.index("} m1v_downscale_plane_layout;")]
    assert "4:2:2 and P010 sources" in older
    proof = open(os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_downscale_words.h")).read()
    for phrase in ("Read contract", "luma wave", "chroma wave", "4 (x + 8) <= 4 xe <= 4 W", "4 * 8 * n_strips = 2 xe",
                   "`lim` = E - 64", "o + 62 <= E", "o - 2 >= lim - 1 >= 0", "E >= 2048", "4 * 65535 + 2 < 2^18"):
        assert phrase in proof, phrase


def test_null_encoder_and_null_out_are_argument_errors():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    values = (0, 12288, 12290, 192, 192, 4, 18432, 2, 8)
    lay = _ffi.DownscaleWordLayout(*values)
    assert L.m1v_set_downscale_word_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_downscale_word_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_downscale_word_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_downscale_words_to_i420_device(None, None, 0, None, None) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, values))
    assert L.m1v_downscale_word_layout_preset(48, 32, _ffi.WORDS_P010, 2, None) == _ffi.E_ARG
    assert L.m1v_last_error()


def _table_row(W, H, preset):
    """The row of the header's preset table."""
    shift, c_step, c_pitch, cr = {"p010": (8, 4, 4 * W, 8 * W * H + 2), "i010": (2, 2, 2 * W, 10 * W * H), "i012": (4, 2, 2 * W, 10 * W * H),
                                  "i016": (8, 2, 2 * W, 10 * W * H)}[preset]
    return dict(y_offset=0, cb_offset=8 * W * H, cr_offset=cr, y_pitch=4 * W, c_pitch=c_pitch, c_step=c_step, frame_stride=12 * W * H,
                factor=2, shift=shift)


def test_preset_against_the_python_mirror_the_table_and_its_errors():
    import pytest
    from ec504_imageencoder_amd import _ffi, downscale_word_layout_preset
    L = _ffi.lib()
    assert sorted(_ffi.WORD_PRESETS) == ["i010", "i012", "i016", "p010", "p012", "p016"]
    assert _ffi.WORD_PRESETS["p010"] == _ffi.WORD_PRESETS["p012"] == _ffi.WORD_PRESETS["p016"] == _ffi.WORDS_P010
    for W, H in SIZES:
        for preset in ("p010", "i010", "i012", "i016"):
            lay = _ffi.DownscaleWordLayout()
            assert L.m1v_downscale_word_layout_preset(W, H, _ffi.WORD_PRESETS[preset], 2, C.byref(lay)) == _ffi.OK
            got = lay.as_dict()
            assert got == downscale_word_layout_preset(W, H, preset), (W, H, preset)
            assert got == _table_row(W, H, preset), (W, H, preset)
    keep = dict(zip(FIELDS, (9,) * 9))
    for args in ((48, 16, 4, 2), (48, 16, -1, 2), (47, 16, 1, 2), (48, 15, 3, 2), (0, 16, 1, 2),
                 (48, 0, 1, 2), (-2, 16, 1, 2), (48, 16, 1, 1), (48, 16, 3, 4), (48, 16, 2, 0)):
        lay = _ffi.DownscaleWordLayout(**keep)
        assert L.m1v_downscale_word_layout_preset(*args, C.byref(lay)) == _ffi.E_ARG, args
        assert L.m1v_last_error()
        assert lay.as_dict() == keep
    for args in ((48, 16, "nv12"), (47, 16, "i010"), (48, 15, "p010"), (0, 16, "i010"), (48, 16, "i010", 4)):
        with pytest.raises(ValueError):
            downscale_word_layout_preset(*args)


# ---- the code object --------------------------------------------------------------------------------------------------------
def _mine():
    bodies, recs = _code_object()
    return {n: b for n, b in bodies.items() if "k_half_words_" in n}, [r for r in recs if "k_half_words_" in r[0]]


def _variant(name):
    """(row, stage8, chroma step) of a tile kernel's mangled name, None for another kernel."""
    m = re.search(r"\d+k_half_words_(encode|size_table|rd_table)ILb([01])ELi\d+ELi([24])EEE", name)
    return (m.group(1), int(m.group(2)), int(m.group(3))) if m else None


def test_twelve_tile_kernels_and_one_bytes_kernel():
    bodies, recs = _mine()
    assert len(bodies) == 13 and len(recs) == 13, sorted(bodies)
    assert sorted(bodies) == sorted(r[0] for r in recs)
    tiles = [_variant(n) for n in bodies if _variant(n)]
    assert len(tiles) == 12 and set(tiles) == {(row, stage8, cstep) for row in ROWS for stage8 in (0, 1) for cstep in (2, 4)}
    assert sum(1 for n in bodies if re.search(r"\d+k_half_words_to_i420E", n)) == 1
    # every name of the prefix is a tile kernel or the bytes kernel: nothing else hides behind it
    assert all(_variant(n) or re.search(r"\d+k_half_words_to_i420E", n) for n in bodies)


def test_no_scratch_four_waves_no_mode_switch_and_no_fp64():
    bodies, recs = _mine()
    assert len(recs) == 13
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) <= 128, (name, vgprs)      # four waves per SIMD at the least
    for name, body in bodies.items():
        ops = [o[0] for o in _ops(body)]
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name
        assert not any(o.startswith("v_") and "f64" in o for o in ops), name


def test_rows_are_loaded_sixteen_bytes_at_a_time():
    """A lane's source row is two 16-byte loads (four for interleaved chroma: the two of the narrow unit and two more under the
    wave-uniform choice) whatever its alignment, 16 rows of a block (8 rendition rows x 2) each, and no byte or halfword loads from
    global memory in the tile kernels.  The loads are counted over what the shared body itself holds: the plane kernel of the same
    row and staging (k_encode_planes, ...), whose front half brings its pixels in by LDS-DMA."""
    bodies, _ = _mine()
    every, _ = _code_object()
    assert sum(1 for n in bodies if _variant(n)) == 12
    for name, body in bodies.items():
        v = _variant(name)
        if not v:
            continue
        sibling = [b for n, b in every.items() if re.search(r"\d+k_%s_planesILb%dELi\d+ELi%dEEE" % (v[0], v[1], v[2] // 2), n)]
        assert len(sibling) == 1, (name, len(sibling))
        ops, shared = [o[0] for o in _ops(body)], [o[0] for o in _ops(sibling[0])]
        assert ops.count("global_load_dwordx4") - shared.count("global_load_dwordx4") == 16 * v[2], (name, ops.count("global_load_dwordx4"))
        assert not any(o in ("global_load_ubyte", "global_load_ushort", "global_load_sbyte", "global_load_sshort") for o in ops), name


def test_no_name_that_another_test_counts():
    mine, recs = _mine()
    for name in list(mine) + [r[0] for r in recs]:
        assert not any(c in name for c in TAKEN), name
        assert not re.search(TILE_SHAPED, name), name
    bodies, _ = _code_object()
    assert not [n for n in bodies if re.search(r"k[tp]_\w*half_words", n)]       # no table twins


def test_the_sweeps_reach_every_tile_kernel():
    """The completeness pin of the new name pattern: every (row, chroma step) of the code object is declared by
    tests/downscale_word_sweeps.py, which tests/test_gpu_downscale_word_sweeps.py runs, and that module declares nothing the
    code object lacks.  (Both stagings of each are reached: every sweep runs narrow and wide qualities.)"""
    import downscale_word_sweeps as sweeps
    bodies, _ = _mine()
    found = {(v[0], v[2]) for v in map(_variant, bodies) if v}
    assert len(found) == 6
    assert found == set(sweeps.REACHED) and len(sweeps.REACHED) == len(set(sweeps.REACHED))
