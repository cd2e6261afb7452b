"""CPU-side checks of the RGB plane input layout (m1v_rgb_plane_layout_preset / m1v_set_rgb_plane_layout /
m1v_rgb_plane_layout_in_force, include/mpeg1_hip.h): the calls and the struct are declared, exported and bound; the presets
against hand-computed values and against the Python mirror; the torch-free stride helper on hand-written shapes and strides;
and the gfx950 code object holds the three kernel families of csrc/m1v_rgb_planes.h (k_encode_rgb_planes,
k_size_table_rgb_planes, k_rd_table_rgb_planes) in both stagings with the shape the design needs."""
import ctypes as C
import os
import re

import pytest

from code_object import _gfx950_disassembly
from code_object import RGB_PLANES_COUNTED as COUNTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_encode_rgb_planes", "k_size_table_rgb_planes", "k_rd_table_rgb_planes")
FIELDS = ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")
ORDERS = ("rgb", "bgr", "gbr")


# ---- the three calls and the struct -----------------------------------------------------------------------------------------
def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, rgb_plane_layout_preset, rgb_plane_strides
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_rgb_plane_layout\s*\{(.*?)\}\s*m1v_rgb_plane_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip() for n in re.sub(r"^\s*uint64_t", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS, members
    assert re.search(r"M1V_RGB_PLANES_RGB\s*=\s*0\s*,\s*M1V_RGB_PLANES_BGR\s*=\s*1\s*,\s*M1V_RGB_PLANES_GBR\s*=\s*2", code)
    assert re.search(r"\bint\s+m1v_rgb_plane_layout_preset\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*m1v_rgb_plane_layout\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_set_rgb_plane_layout\s*\(\s*m1v_encoder\s*\*\s*\w+\s*,\s*const\s+m1v_rgb_plane_layout\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_rgb_plane_layout_in_force\s*\(\s*const\s+m1v_encoder\s*\*\s*\w+\s*,\s*m1v_rgb_plane_layout\s*\*\s*\w+\s*\)", code)
    # the definition, the limits and the read contract are stated beside the declarations
    for phrase in ("c_offset + y * row_pitch + x", "an odd width", "row interleave", "Read contract", "are never read"):
        assert phrase in text, phrase
    L = _ffi.lib()
    for name in ("m1v_rgb_plane_layout_preset", "m1v_set_rgb_plane_layout", "m1v_rgb_plane_layout_in_force"):
        assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert tuple(n for n, _ in _ffi.RgbPlaneLayout._fields_) == FIELDS
    assert all(t is C.c_uint64 for _, t in _ffi.RgbPlaneLayout._fields_)
    assert C.sizeof(_ffi.RgbPlaneLayout) == 40
    assert list(L.m1v_rgb_plane_layout_preset.argtypes) == [C.c_int, C.c_int, C.c_int, C.POINTER(_ffi.RgbPlaneLayout)]
    assert list(L.m1v_set_rgb_plane_layout.argtypes) == [C.c_void_p, C.POINTER(_ffi.RgbPlaneLayout)]
    assert list(L.m1v_rgb_plane_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(_ffi.RgbPlaneLayout)]
    assert _ffi.RGB_PLANE_ORDERS == {"rgb": 0, "bgr": 1, "gbr": 2}
    assert callable(Mpeg1Encoder.set_rgb_plane_layout) and isinstance(Mpeg1Encoder.rgb_plane_layout, property)
    assert callable(rgb_plane_layout_preset) and callable(rgb_plane_strides)


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    lay = _ffi.RgbPlaneLayout(0, 768, 1536, 48, 2304)
    assert L.m1v_set_rgb_plane_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_rgb_plane_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_rgb_plane_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, (0, 768, 1536, 48, 2304)))
    assert L.m1v_rgb_plane_layout_preset(352, 288, 0, None) == _ffi.E_ARG


# hand-computed: (r_offset, g_offset, b_offset, row_pitch, frame_stride); the name is the planes' order in memory
PRESETS = {
    (352, 288): {"rgb": (0, 101376, 202752, 352, 304128), "bgr": (202752, 101376, 0, 352, 304128), "gbr": (202752, 0, 101376, 352, 304128)},
    (48, 16): {"rgb": (0, 768, 1536, 48, 2304), "bgr": (1536, 768, 0, 48, 2304), "gbr": (1536, 0, 768, 48, 2304)},
}


@pytest.mark.parametrize("size", sorted(PRESETS))
@pytest.mark.parametrize("name", ORDERS)
def test_presets_against_hand_computed_values(size, name):
    from ec504_imageencoder_amd import _ffi, rgb_plane_layout_preset, rgb_plane_strides
    W, H = size
    lay = _ffi.RgbPlaneLayout()
    assert _ffi.lib().m1v_rgb_plane_layout_preset(W, H, _ffi.RGB_PLANE_ORDERS[name], C.byref(lay)) == _ffi.OK
    want = dict(zip(FIELDS, PRESETS[size][name]))
    assert lay.as_dict() == want
    assert rgb_plane_layout_preset(W, H, name) == want
    # the preset is the layout of a contiguous [n, 3, H, W] tensor whose channels are in that order
    assert rgb_plane_strides((5, 3, H, W), (3 * H * W, H * W, W, 1), name) == want


def test_preset_errors_and_the_python_mirror():
    from ec504_imageencoder_amd import _ffi, rgb_plane_layout_preset
    L = _ffi.lib()
    keep = dict(zip(FIELDS, (9,) * 5))
    for order in (-1, 3, 4, 99):
        lay = _ffi.RgbPlaneLayout(**keep)
        assert L.m1v_rgb_plane_layout_preset(352, 288, order, C.byref(lay)) == _ffi.E_ARG
        assert lay.as_dict() == keep
    for W, H in ((0, 288), (352, 0), (-16, 16)):
        assert L.m1v_rgb_plane_layout_preset(W, H, 0, C.byref(_ffi.RgbPlaneLayout())) == _ffi.E_ARG
        with pytest.raises(ValueError):
            rgb_plane_layout_preset(W, H, "rgb")
    with pytest.raises(ValueError):
        rgb_plane_layout_preset(352, 288, "rbg")
    for W in (16, 96, 176, 354, 3840):
        for H in (16, 144, 2160):
            for name, code in _ffi.RGB_PLANE_ORDERS.items():
                lay = _ffi.RgbPlaneLayout()
                assert L.m1v_rgb_plane_layout_preset(W, H, code, C.byref(lay)) == _ffi.OK
                assert lay.as_dict() == rgb_plane_layout_preset(W, H, name), (W, H, name)


# ---- the stride helper ------------------------------------------------------------------------------------------------------
def test_strides_of_packed_windowed_and_four_plane_tensors():
    from ec504_imageencoder_amd import rgb_plane_strides
    H, W = 32, 48
    # a contiguous [7, 3, 32, 48] tensor
    assert rgb_plane_strides((7, 3, H, W), (4608, 1536, 48, 1)) == dict(r_offset=0, g_offset=1536, b_offset=3072, row_pitch=48, frame_stride=4608)
    assert rgb_plane_strides((7, 3, H, W), (4608, 1536, 48, 1), "bgr") == dict(r_offset=3072, g_offset=1536, b_offset=0, row_pitch=48, frame_stride=4608)
    assert rgb_plane_strides((7, 3, H, W), (4608, 1536, 48, 1), "gbr") == dict(r_offset=3072, g_offset=0, b_offset=1536, row_pitch=48, frame_stride=4608)
    # the window x[:, :, 5:5+32, 9:9+48] of a contiguous [2, 3, 70, 101] tensor: the strides of the large tensor
    assert rgb_plane_strides((2, 3, H, W), (21210, 7070, 101, 1)) == dict(r_offset=0, g_offset=7070, b_offset=14140, row_pitch=101, frame_stride=21210)
    # the first three planes of a contiguous [4, 4, 32, 48] RGBA tensor, and B, G, R of its last three (A, B, G, R order)
    assert rgb_plane_strides((4, 4, H, W), (6144, 1536, 48, 1)) == dict(r_offset=0, g_offset=1536, b_offset=3072, row_pitch=48, frame_stride=6144)
    assert rgb_plane_strides((4, 4, H, W), (6144, 1536, 48, 1), (3, 2, 1)) == dict(r_offset=4608, g_offset=3072, b_offset=1536, row_pitch=48, frame_stride=6144)
    # planes interleaved by rows: x.permute(0, 2, 1, 3) of a contiguous [n, H, 3, W] tensor
    assert rgb_plane_strides((2, 3, H, W), (4608, 48, 144, 1)) == dict(r_offset=0, g_offset=48, b_offset=96, row_pitch=144, frame_stride=4608)
    # a single frame's stride says nothing: the bytes its planes span
    assert rgb_plane_strides((1, 3, H, W), (0, 1536, 48, 1))["frame_stride"] == 3072 + 31 * 48 + 48
    assert rgb_plane_strides((0, 3, H, W), (4608, 1536, 48, 1))["row_pitch"] == 48
    for shape, strides, order in (
            ((2, 3, H, W), (4608, 1, 144, 3), "rgb"),        # x.permute(0, 3, 1, 2) of an NHWC tensor: a row's bytes are not adjacent
            ((2, 3, H, W), (4608, 1536, 48, 2), "rgb"),      # every other byte
            ((2, 3, H, W), (4608, 1536, 47, 1), "rgb"),      # a pitch below W
            ((2, 2, H, W), (3072, 1536, 48, 1), "rgb"),      # two channels
            ((2, 3, H, W), (4608, 1536, 48, 1), (0, 1, 3)),  # a channel the tensor does not have
            ((2, 3, H, W), (4608, 1536, 48, 1), "rbg"),      # an unknown order
            ((3, H, W), (1536, 48, 1), "rgb")):              # not four dimensions
        with pytest.raises(ValueError):
            rgb_plane_strides(shape, strides, order)


# ---- the code object --------------------------------------------------------------------------------------------------------
def _kernels(family):
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if family in n}
    recs = re.findall(r"\.name:\s*(\S*%s\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)" % family, notes, re.S)
    return bodies, recs


@pytest.mark.parametrize("family", FAMILIES)
def test_every_instantiation_exists_without_scratch(family):
    """[STAGE8][R]: byte / halfword staging, one ring; 0 bytes of private segment (a spill would join the vmcnt queue the row loop
    counts on) and at most 96 VGPRs, the budget of the packed and surface kernels."""
    bodies, recs = _kernels(family)
    assert len(bodies) == 2 and len(recs) == 2, (sorted(bodies), recs)
    for stage8 in (0, 1):
        pat = r"%sILb%dELi\d+EE" % (family, stage8)
        assert sum(1 for n in bodies if re.search(pat, n)) == 1, (pat, sorted(bodies))
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0 and int(vgprs) <= 96, (name, scratch, vgprs)


@pytest.mark.parametrize("family", FAMILIES)
def test_rgb_plane_kernel_shape(family):
    """Each instantiation brings its pixels in by LDS-DMA only, in the fetch shape of k_encode_tiles (two 1-KiB instructions per
    row-step: sixteen; plus the three of the wave's VLC table; the row loop waits vmcnt 2 seven times, then 0), takes the integer
    row pass in the default rounding mode (sixteen v_mul_hi_i32, no MODE switch: no s_setreg), keeps the fp64 tie path of the colour
    stage, and has no scratch instruction."""
    bodies, recs = _kernels(family)
    assert bodies and recs
    for name, body in bodies.items():
        lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))]
        ops = [l.split()[0] for l in lines]
        assert sum(o == "global_load_lds_dwordx4" for o in ops) == 16, name
        assert sum(o == "global_load_lds_dword" for o in ops) == 3, name
        assert sum(o.startswith("v_mul_hi_i32") for o in ops) == 16, name
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name
        assert any(re.match(r"v_fma_f64|v_mul_f64|v_add_f64", o) for o in ops), name
        if family == "k_encode_rgb_planes":
            assert not any(o.startswith(("global_load_dword", "global_load_ubyte", "global_load_ushort", "global_load_sbyte",
                                         "global_load_short", "flat_load", "buffer_load")) for o in ops), name
        first_read = next(i for i, l in enumerate(lines) if l.startswith("ds_read_b64"))
        waits = [int(x) for l in lines[:first_read + 4000] for x in re.findall(r"s_waitcnt vmcnt\((\d+)\)", l)]
        assert waits[:8] == [2, 2, 2, 2, 2, 2, 2, 0], (name, waits[:12])


def test_rgb_plane_kernels_keep_out_of_the_counted_names():
    """The existing code-object tests count kernels by these substrings."""
    for family in FAMILIES:
        bodies, recs = _kernels(family)
        assert bodies and recs
        for name in list(bodies) + [r[0] for r in recs]:
            assert not any(c in name for c in COUNTED), name
