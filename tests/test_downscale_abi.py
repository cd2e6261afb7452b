"""CPU-side checks of the downscale layout's C ABI (m1v_downscale_layout_preset / m1v_set_downscale_layout /
m1v_downscale_layout_in_force / m1v_downscale_to_bytes_device, include/mpeg1_hip.h): declared, exported and bound; the struct's
size and offsets; the preset against the Python mirror; and the gfx950 code object holds the kernels of csrc/m1v_downscale.h — 12
tile kernels and 1 bytes kernel, without scratch and without a MODE switch, at four waves per SIMD or more, with names that no
other code-object test counts — each of them reached by the sweeps of tests/test_gpu_downscale_sweeps.py."""
import ctypes as C
import os
import re

from code_object import EXISTING, RGB_PLANES_COUNTED, SAMPLE_LAYOUT_COUNTED, _code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("row_pitch", "frame_stride", "pixel_step", "order", "factor")
SYMBOLS = ("m1v_downscale_layout_preset", "m1v_set_downscale_layout", "m1v_downscale_layout_in_force",
           "m1v_downscale_to_bytes_device")
ROWS = ("encode", "size_table", "rd_table")
# what the code-object tests of the other layouts count kernels by: no new mangled name may contain one
TAKEN = EXISTING + RGB_PLANES_COUNTED + SAMPLE_LAYOUT_COUNTED
# the completeness pattern of tests/test_input_families_cpu.py
TILE_SHAPED = r"\d(k[tp]?_(?:encode|size_table|rd_table)_[a-z0-9_]+)"


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, downscale_layout_preset, downscale_strides
    from ec504_imageencoder_amd.encoder import DOWNSCALE_LAYOUT_FIELDS
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_downscale_layout\s*\{(.*?)\}\s*m1v_downscale_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip()
               for n in re.sub(r"^\s*(uint64_t|int32_t)", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS == DOWNSCALE_LAYOUT_FIELDS, members
    declared = re.findall(r"\b(m1v_\w+)\s*\(", code)
    assert sorted(set(declared)) == sorted(_ffi.MPEG1_HIP_SYMBOLS)
    L = _ffi.lib()
    for name in SYMBOLS:
        assert name in declared and name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert tuple(n for n, _ in _ffi.DownscaleLayout._fields_) == FIELDS
    assert C.sizeof(_ffi.DownscaleLayout) == 32
    assert [getattr(_ffi.DownscaleLayout, n).offset for n in FIELDS] == [0, 8, 16, 24, 28]
    assert [getattr(_ffi.DownscaleLayout, n).size for n in FIELDS] == [8, 8, 8, 4, 4]
    assert list(L.m1v_downscale_layout_preset.argtypes) == [C.c_int] * 5 + [C.POINTER(_ffi.DownscaleLayout)]
    assert list(L.m1v_set_downscale_layout.argtypes) == [C.c_void_p, C.POINTER(_ffi.DownscaleLayout)]
    assert list(L.m1v_downscale_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(_ffi.DownscaleLayout)]
    assert list(L.m1v_downscale_to_bytes_device.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert callable(Mpeg1Encoder.set_downscale_layout) and callable(Mpeg1Encoder.downscale_to_bytes)
    assert isinstance(Mpeg1Encoder.downscale_layout, property)
    assert callable(downscale_layout_preset) and callable(downscale_strides)


def test_header_carries_the_definition_the_read_contract_and_what_is_not_covered():
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    section = text[text.index("/* Downscale layout"):text.index("} m1v_downscale_layout;")]
    for phrase in ("F + Y * row_pitch + X * pixel_step + i", "(s(2x, 2y) + s(2x+1, 2y) + s(2x, 2y+1) + s(2x+1, 2y+1) + 2) >> 2",
                   "rounds half up", "[F + Y * row_pitch, F + Y * row_pitch + 2 * width * pixel_step)", "2 * height - 1",
                   "A 4th byte inside a pixel may be read and never influences the output", "channels = 3",
                   "factor 4 and other factors", "filters other than the box", "sources of odd", "downscaled YCbCr planes, RGB planes and float layouts",
                   "a frame table or a plane table", "the host-buffer", "the folder CLI", "several renditions in one pass"):
        assert phrase in section, phrase
    proof = open(os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_downscale.h")).read()
    for phrase in ("Read contract", "luma wave", "chroma wave", "x + 8 <= W / 2 + 8 n_strips <= W", "2 (x + 8) * P <= 2 W * P"):
        assert phrase in proof, phrase


def test_null_encoder_and_null_out_are_argument_errors():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    lay = _ffi.DownscaleLayout(288, 18432, 3, 0, 2)
    assert L.m1v_set_downscale_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_downscale_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_downscale_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_downscale_to_bytes_device(None, None, 0, None, None) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, (288, 18432, 3, 0, 2)))
    assert L.m1v_downscale_layout_preset(48, 32, 3, 0, 2, None) == _ffi.E_ARG


def test_preset_against_the_python_mirror_and_its_errors():
    import pytest
    from ec504_imageencoder_amd import _ffi, downscale_layout_preset
    L = _ffi.lib()
    for W, H in ((16, 16), (48, 32), (354, 144), (1920, 1080), (3840, 2160)):
        for step in (3, 4):
            for order, ocode in _ffi.PIXEL_ORDERS.items():
                lay = _ffi.DownscaleLayout()
                assert L.m1v_downscale_layout_preset(W, H, step, ocode, 2, C.byref(lay)) == _ffi.OK
                got = lay.as_dict()
                assert got == downscale_layout_preset(W, H, step, order), (W, H, step, order)
                assert got == dict(row_pitch=2 * W * step, frame_stride=2 * H * 2 * W * step, pixel_step=step, order=ocode, factor=2)
    keep = dict(zip(FIELDS, (9,) * 5))
    for args in ((48, 16, 2, 0, 2), (48, 16, 5, 0, 2), (48, 16, 1, 0, 2), (48, 16, 3, 2, 2), (48, 16, 3, -1, 2), (48, 16, 3, 0, 1),
                 (48, 16, 3, 0, 4), (48, 16, 4, 0, 0), (0, 16, 3, 0, 2), (48, 0, 4, 0, 2), (-2, 16, 3, 0, 2)):
        lay = _ffi.DownscaleLayout(**keep)
        assert L.m1v_downscale_layout_preset(*args, C.byref(lay)) == _ffi.E_ARG, args
        assert L.m1v_last_error()
        assert lay.as_dict() == keep
    for args in ((48, 16, 2), (0, 16, 3), (48, 16, 3, "gbr"), (48, 16, 3, "rgb", 4)):
        with pytest.raises(ValueError):
            downscale_layout_preset(*args)


# ---- the code object --------------------------------------------------------------------------------------------------------
def _mine():
    bodies, recs = _code_object()
    return {n: b for n, b in bodies.items() if "k_downscale_" in n}, [r for r in recs if "k_downscale_" in r[0]]


def _variant(name):
    """(row, stage8, bytes per source pixel) of a tile kernel's mangled name, None for another kernel."""
    m = re.search(r"\d+k_downscale_(encode|size_table|rd_table)ILb([01])ELi\d+ELi([34])EEE", name)
    return (m.group(1), int(m.group(2)), int(m.group(3))) if m else None


def test_twelve_tile_kernels_and_one_bytes_kernel():
    bodies, recs = _mine()
    assert len(bodies) == 13 and len(recs) == 13, sorted(bodies)
    assert sorted(bodies) == sorted(r[0] for r in recs)
    tiles = [_variant(n) for n in bodies if _variant(n)]
    assert len(tiles) == 12 and set(tiles) == {(row, stage8, Cs) for row in ROWS for stage8 in (0, 1) for Cs in (3, 4)}
    assert sum(1 for n in bodies if re.search(r"\d+k_downscale_to_bytesE", n)) == 1
    # every name of the prefix is a tile kernel or the bytes kernel: nothing else hides behind it
    assert all(_variant(n) or re.search(r"\d+k_downscale_to_bytesE", n) for n in bodies)


def test_no_scratch_four_waves_and_no_mode_switch():
    bodies, recs = _mine()
    assert len(recs) == 13
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) <= 128, (name, vgprs)      # four waves per SIMD at the least
    for name, body in bodies.items():
        ops = [l.split("//")[0].split()[0] for l in body.splitlines() if l.split("//")[0].strip() and not l.strip().startswith(("/", ";"))]
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name


def test_rows_are_loaded_sixteen_bytes_at_a_time():
    """A lane's source row is 3 or 4 16-byte loads whatever its alignment: 16 rows of a block (8 rendition rows x 2) per kernel,
    and no byte or word loads from global memory in the tile kernels."""
    bodies, _ = _mine()
    for name, body in bodies.items():
        v = _variant(name)
        if not v:
            continue
        ops = [l.split("//")[0].split()[0] for l in body.splitlines() if l.split("//")[0].strip() and not l.strip().startswith(("/", ";"))]
        assert ops.count("global_load_dwordx4") == 16 * v[2], (name, ops.count("global_load_dwordx4"))
        assert not any(o in ("global_load_ubyte", "global_load_ushort", "global_load_sbyte") for o in ops), name


def test_no_name_that_another_test_counts():
    mine, recs = _mine()
    for name in list(mine) + [r[0] for r in recs]:
        assert not any(c in name for c in TAKEN), name
        assert not re.search(TILE_SHAPED, name), name
    bodies, _ = _code_object()
    assert not [n for n in bodies if re.search(r"k[tp]_\w*downscale", n)]       # no table twins


def test_the_sweeps_reach_every_tile_kernel():
    """The completeness pin of the new name pattern: every (row, bytes per source pixel) of the code object is declared by
    tests/downscale_sweeps.py, which tests/test_gpu_downscale_sweeps.py runs, and that module declares nothing the code object
    lacks.  (Both stagings of each are reached: every sweep runs narrow and wide qualities.)"""
    import downscale_sweeps as sweeps
    bodies, _ = _mine()
    found = {(v[0], v[2]) for v in map(_variant, bodies) if v}
    assert len(found) == 6
    assert found == set(sweeps.REACHED) and len(sweeps.REACHED) == len(set(sweeps.REACHED))
