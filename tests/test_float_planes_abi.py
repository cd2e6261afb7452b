"""CPU-side checks of the float plane layout's C ABI (m1v_float_plane_layout_preset / m1v_set_float_plane_layout /
m1v_float_plane_layout_in_force / m1v_float_planes_to_bytes_device, include/mpeg1_hip.h): declared, exported and bound; the
header carries the definition; the preset against the Python mirror; and the gfx950 code object holds the kernels of
csrc/m1v_float_planes.h — 18 tile kernels and 3 bytes kernels, without scratch and without a MODE switch, with no table twins and
with names that the other code-object tests do not count."""
import ctypes as C
import os
import re

import pytest

from code_object import EXISTING, _code_object
from code_object import RGB_PLANES_COUNTED as COUNTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride", "sample", "range")
SYMBOLS = ("m1v_float_plane_layout_preset", "m1v_set_float_plane_layout", "m1v_float_plane_layout_in_force",
           "m1v_float_planes_to_bytes_device")
FAMILIES = ("k_encode_float_planes", "k_size_table_float_planes", "k_rd_table_float_planes")


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, float_plane_layout_preset, float_plane_strides
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_float_plane_layout\s*\{(.*?)\}\s*m1v_float_plane_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip()
               for n in re.sub(r"^\s*(uint64_t|int32_t)", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS, members
    assert re.search(r"M1V_SAMPLE_F16\s*=\s*0\s*,\s*M1V_SAMPLE_BF16\s*=\s*1\s*,\s*M1V_SAMPLE_F32\s*=\s*2", code)
    assert re.search(r"M1V_RANGE_UNIT\s*=\s*0\s*,\s*M1V_RANGE_BYTE\s*=\s*1", code)
    # every symbol the header declares is in the list, and the list holds nothing else
    declared = re.findall(r"\b(m1v_\w+)\s*\(", code)
    assert sorted(set(declared)) == sorted(_ffi.MPEG1_HIP_SYMBOLS)
    L = _ffi.lib()
    for name in SYMBOLS:
        assert name in declared and name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert tuple(n for n, _ in _ffi.FloatPlaneLayout._fields_) == FIELDS
    assert C.sizeof(_ffi.FloatPlaneLayout) == 48
    assert list(L.m1v_set_float_plane_layout.argtypes) == [C.c_void_p, C.POINTER(_ffi.FloatPlaneLayout)]
    assert list(L.m1v_float_plane_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(_ffi.FloatPlaneLayout)]
    assert list(L.m1v_float_planes_to_bytes_device.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert _ffi.FLOAT_SAMPLES == {"float16": 0, "bfloat16": 1, "float32": 2} and _ffi.FLOAT_RANGES == {"unit": 0, "byte": 1}
    assert callable(Mpeg1Encoder.set_float_plane_layout) and callable(Mpeg1Encoder.float_planes_to_bytes)
    assert isinstance(Mpeg1Encoder.float_plane_layout, property)
    assert callable(float_plane_layout_preset) and callable(float_plane_strides)


def test_header_carries_the_definition():
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    for phrase in ("ties to even", "one fp32 multiplication", "NaN", "F + c_offset + y * row_pitch + x * S",
                   "[F + c_offset, F + c_offset + (height - 1) * row_pitch + width * S)", "only addressed samples",
                   "np.clip(np.where(np.isnan(t), 0, np.rint(t)), 0, 255)", "float frames behind a frame table"):
        assert phrase in text, phrase


def test_null_encoder_and_null_out_are_argument_errors():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    lay = _ffi.FloatPlaneLayout(0, 1536, 3072, 96, 4608, 0, 0)
    assert L.m1v_set_float_plane_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_float_plane_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_float_plane_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_float_planes_to_bytes_device(None, None, 0, None, None) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, (0, 1536, 3072, 96, 4608, 0, 0)))
    assert L.m1v_float_plane_layout_preset(48, 16, 0, 0, 0, None) == _ffi.E_ARG


def test_preset_against_the_python_mirror_and_its_errors():
    from ec504_imageencoder_amd import _ffi, float_plane_layout_preset
    L = _ffi.lib()
    for W, H in ((16, 16), (48, 32), (354, 144), (3840, 2160)):
        for order, ocode in _ffi.RGB_PLANE_ORDERS.items():
            for dtype, scode in _ffi.FLOAT_SAMPLES.items():
                for rng, rcode in _ffi.FLOAT_RANGES.items():
                    lay = _ffi.FloatPlaneLayout()
                    assert L.m1v_float_plane_layout_preset(W, H, ocode, scode, rcode, C.byref(lay)) == _ffi.OK
                    assert lay.as_dict() == float_plane_layout_preset(W, H, order, dtype, rng), (W, H, order, dtype, rng)
    keep = dict(zip(FIELDS, (9,) * 7))
    for args in ((48, 16, 3, 0, 0), (48, 16, -1, 0, 0), (48, 16, 0, 3, 0), (48, 16, 0, -1, 0), (48, 16, 0, 0, 2), (48, 16, 0, 0, -1),
                 (0, 16, 0, 0, 0), (48, 0, 0, 0, 0)):
        lay = _ffi.FloatPlaneLayout(**keep)
        assert L.m1v_float_plane_layout_preset(*args, C.byref(lay)) == _ffi.E_ARG, args
        assert lay.as_dict() == keep


# ---- the code object --------------------------------------------------------------------------------------------------------
def _mine():
    bodies, recs = _code_object()
    return {n: b for n, b in bodies.items() if "float_planes" in n}, [r for r in recs if "float_planes" in r[0]]


def test_eighteen_tile_kernels_and_three_bytes_kernels():
    bodies, recs = _mine()
    assert len(bodies) == 21 and len(recs) == 21, sorted(bodies)
    for family in FAMILIES:
        for sample in ("9F16Sample", "10Bf16Sample", "9F32Sample"):
            for stage8 in (0, 1):
                pat = r"\d+%sILb%dELi\d+ENS_%sE" % (family, stage8, sample)
                assert sum(1 for n in bodies if re.search(pat, n)) == 1, pat
    for sample in ("9F16Sample", "10Bf16Sample", "9F32Sample"):
        assert sum(1 for n in bodies if re.search(r"\d+k_float_planes_to_bytesINS_%sE" % sample, n)) == 1, sample
    assert sorted(bodies) == sorted(r[0] for r in recs)


def test_no_scratch_and_no_mode_switch():
    bodies, recs = _mine()
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) <= 128, (name, vgprs)      # four waves per SIMD at the least
    for name, body in bodies.items():
        ops = [l.split("//")[0].split()[0] for l in body.splitlines() if l.split("//")[0].strip() and not l.strip().startswith(("/", ";"))]
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name


def test_no_table_twins_and_no_existing_family_name():
    bodies, _ = _code_object()
    assert not [n for n in bodies if re.search(r"k[tp]_\w*float_planes", n)]
    mine, recs = _mine()
    for name in list(mine) + [r[0] for r in recs]:
        assert not any(c in name for c in EXISTING + COUNTED), name
