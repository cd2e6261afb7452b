"""CPU-side checks of the float pixel layout's C ABI (m1v_float_pixel_layout_preset / m1v_set_float_pixel_layout /
m1v_float_pixel_layout_in_force / m1v_float_pixels_to_bytes_device, include/mpeg1_hip.h): declared, exported and bound; the
struct's size and offsets; the preset against the Python mirror; and the gfx950 code object holds the kernels of
csrc/m1v_float_pixels.h — 36 tile kernels and 3 bytes kernels, without scratch and without a MODE switch, at four waves per SIMD
or more, with names that no other code-object test counts — each of them reached by the sweeps of
tests/test_gpu_float_pixels_sweeps.py."""
import ctypes as C
import os
import re

import float_planes as fp
from code_object import EXISTING, RGB_PLANES_COUNTED, SAMPLE_LAYOUT_COUNTED, _code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("row_pitch", "frame_stride", "pixel_step", "order", "sample", "range")
SYMBOLS = ("m1v_float_pixel_layout_preset", "m1v_set_float_pixel_layout", "m1v_float_pixel_layout_in_force",
           "m1v_float_pixels_to_bytes_device")
ROWS = ("encode", "size_table", "rd_table")
SAMPLES = {"float16": "9F16Sample", "bfloat16": "10Bf16Sample", "float32": "9F32Sample"}
# what the code-object tests of the other layouts count kernels by: no new mangled name may contain one
TAKEN = ("float_planes",) + EXISTING + RGB_PLANES_COUNTED + SAMPLE_LAYOUT_COUNTED
# the completeness pattern of tests/test_input_families_cpu.py
TILE_SHAPED = r"\d(k[tp]?_(?:encode|size_table|rd_table)_[a-z0-9_]+)"


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, float_pixel_layout_preset, float_pixel_strides
    from ec504_imageencoder_amd.encoder import FLOAT_PIXEL_LAYOUT_FIELDS
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_float_pixel_layout\s*\{(.*?)\}\s*m1v_float_pixel_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip()
               for n in re.sub(r"^\s*(uint64_t|int32_t)", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS == FLOAT_PIXEL_LAYOUT_FIELDS, members
    declared = re.findall(r"\b(m1v_\w+)\s*\(", code)
    assert sorted(set(declared)) == sorted(_ffi.MPEG1_HIP_SYMBOLS)
    L = _ffi.lib()
    for name in SYMBOLS:
        assert name in declared and name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert tuple(n for n, _ in _ffi.FloatPixelLayout._fields_) == FIELDS
    assert C.sizeof(_ffi.FloatPixelLayout) == 40
    assert [getattr(_ffi.FloatPixelLayout, n).offset for n in FIELDS] == [0, 8, 16, 24, 28, 32]
    assert [getattr(_ffi.FloatPixelLayout, n).size for n in FIELDS] == [8, 8, 8, 4, 4, 4]
    assert list(L.m1v_float_pixel_layout_preset.argtypes) == [C.c_int] * 6 + [C.POINTER(_ffi.FloatPixelLayout)]
    assert list(L.m1v_set_float_pixel_layout.argtypes) == [C.c_void_p, C.POINTER(_ffi.FloatPixelLayout)]
    assert list(L.m1v_float_pixel_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(_ffi.FloatPixelLayout)]
    assert list(L.m1v_float_pixels_to_bytes_device.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert _ffi.PIXEL_ORDERS == {"rgb": 0, "bgr": 1}
    assert callable(Mpeg1Encoder.set_float_pixel_layout) and callable(Mpeg1Encoder.float_pixels_to_bytes)
    assert isinstance(Mpeg1Encoder.float_pixel_layout, property)
    assert callable(float_pixel_layout_preset) and callable(float_pixel_strides)


def test_header_carries_the_definition_and_points_to_the_rule():
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    section = text[text.index("/* Float pixel layout"):text.index("} m1v_float_pixel_layout;")]
    for phrase in ("F + y * row_pitch + x * pixel_step + i * S", "[F + y * row_pitch, F + y * row_pitch + width * pixel_step)",
                   "A 4th sample inside a pixel may be read and never influences the output", "\"Float plane layout\"",
                   "ARGB", "float YCbCr", "the host-buffer entry points", "a frame table or a plane table", "channels = 3"):
        assert phrase in section, phrase
    assert "np.rint" not in section and "ties to even" not in section       # the rule is stated once, by the float plane layout
    proof = open(os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_float_pixels.h")).read()
    for phrase in ("Read contract", "luma wave", "chroma wave", "x + 8 <= W / 2 + 8 n_strips <= W"):
        assert phrase in proof, phrase


def test_null_encoder_and_null_out_are_argument_errors():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    lay = _ffi.FloatPixelLayout(288, 4608, 6, 0, 0, 0)
    assert L.m1v_set_float_pixel_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_float_pixel_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_float_pixel_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_float_pixels_to_bytes_device(None, None, 0, None, None) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, (288, 4608, 6, 0, 0, 0)))
    assert L.m1v_float_pixel_layout_preset(48, 16, 3, 0, 0, 0, None) == _ffi.E_ARG


def test_preset_against_the_python_mirror_and_its_errors():
    from ec504_imageencoder_amd import _ffi, float_pixel_layout_preset
    L = _ffi.lib()
    for W, H in ((16, 16), (48, 32), (354, 144), (3840, 2160)):
        for samples in (3, 4):
            for order, ocode in _ffi.PIXEL_ORDERS.items():
                for dtype, scode in _ffi.FLOAT_SAMPLES.items():
                    for rng, rcode in _ffi.FLOAT_RANGES.items():
                        lay = _ffi.FloatPixelLayout()
                        assert L.m1v_float_pixel_layout_preset(W, H, samples, ocode, scode, rcode, C.byref(lay)) == _ffi.OK
                        got = lay.as_dict()
                        assert got == float_pixel_layout_preset(W, H, samples, dtype, order, rng), (W, H, samples, order, dtype, rng)
                        S = fp.BYTES[dtype]
                        assert got == dict(row_pitch=W * samples * S, frame_stride=H * W * samples * S, pixel_step=samples * S,
                                           order=ocode, sample=scode, range=rcode)
    keep = dict(zip(FIELDS, (9,) * 6))
    for args in ((48, 16, 2, 0, 0, 0), (48, 16, 5, 0, 0, 0), (48, 16, 1, 0, 0, 0), (48, 16, 3, 2, 0, 0), (48, 16, 3, -1, 0, 0),
                 (48, 16, 3, 0, 3, 0), (48, 16, 3, 0, -1, 0), (48, 16, 3, 0, 0, 2), (48, 16, 3, 0, 0, -1), (0, 16, 3, 0, 0, 0),
                 (48, 0, 4, 0, 0, 0)):
        lay = _ffi.FloatPixelLayout(**keep)
        assert L.m1v_float_pixel_layout_preset(*args, C.byref(lay)) == _ffi.E_ARG, args
        assert lay.as_dict() == keep


# ---- the code object --------------------------------------------------------------------------------------------------------
def _mine():
    bodies, recs = _code_object()
    return {n: b for n, b in bodies.items() if "k_float_pixels_" in n}, [r for r in recs if "k_float_pixels_" in r[0]]


def _variant(name):
    """(row, stage8, type, samples per pixel) of a tile kernel's mangled name, None for another kernel."""
    m = re.search(r"\d+k_float_pixels_(encode|size_table|rd_table)ILb([01])ELi\d+ENS_(\w+?Sample)ELi([34])EEE", name)
    if not m:
        return None
    kind = {v: k for k, v in SAMPLES.items()}[m.group(3)]
    return m.group(1), int(m.group(2)), kind, int(m.group(4))


def test_thirty_six_tile_kernels_and_three_bytes_kernels():
    bodies, recs = _mine()
    assert len(bodies) == 39 and len(recs) == 39, sorted(bodies)
    assert sorted(bodies) == sorted(r[0] for r in recs)
    tiles = [_variant(n) for n in bodies if _variant(n)]
    want = {(row, stage8, kind, Cs) for row in ROWS for stage8 in (0, 1) for kind in SAMPLES for Cs in (3, 4)}
    assert len(tiles) == 36 and set(tiles) == want
    for sample in SAMPLES.values():
        assert sum(1 for n in bodies if re.search(r"\d+k_float_pixels_to_bytesINS_%sE" % sample, n)) == 1, sample


def test_no_scratch_four_waves_and_no_mode_switch():
    bodies, recs = _mine()
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) <= 128, (name, vgprs)      # four waves per SIMD at the least
    for name, body in bodies.items():
        ops = [l.split("//")[0].split()[0] for l in body.splitlines() if l.split("//")[0].strip() and not l.strip().startswith(("/", ";"))]
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name


def test_no_name_that_another_test_counts():
    mine, recs = _mine()
    for name in list(mine) + [r[0] for r in recs]:
        assert not any(c in name for c in TAKEN), name
        assert not re.search(TILE_SHAPED, name), name
    bodies, _ = _code_object()
    assert not [n for n in bodies if re.search(r"k[tp]_\w*float_pixels", n)]       # no table twins


def test_the_sweeps_reach_every_tile_kernel():
    """The completeness pin of the new name pattern: every (row, type, samples per pixel) of the code object is declared by
    tests/test_gpu_float_pixels_sweeps.py, and that module declares nothing the code object lacks.  (Both stagings of each are
    reached: every sweep runs narrow and wide qualities.)"""
    import float_pixel_sweeps as sweeps
    bodies, _ = _mine()
    found = {v[:1] + v[2:] for v in map(_variant, bodies) if v}
    assert len(found) == 18
    assert found == set(sweeps.REACHED) and len(sweeps.REACHED) == len(set(sweeps.REACHED))
    # every name of the pattern is a tile kernel or a bytes kernel: nothing else hides behind the prefix
    assert all(_variant(n) or "k_float_pixels_to_bytes" in n for n in bodies)
