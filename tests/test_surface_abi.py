"""CPU-side checks of the surface input layout (m1v_set_input_layout / m1v_input_layout, include/mpeg1_hip.h): both calls are
declared, exported and bound, a null encoder is an argument error, the pure stride helper of the Python mirror derives a layout
from a tensor's shape and strides, and the gfx950 code object holds both surface kernel families (k_encode_surface,
k_size_table_surface; csrc/m1v_tiles.h) in every [staging][bytes per pixel][byte order] instantiation with the shape the design
needs."""
import ctypes as C
import os
import re

import pytest

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_encode_surface", "k_size_table_surface")
COUNTED = ("k_encode_tiles", "k_encode_dense", "k_encode_strips", "k_size_table_tiles", "k_size_table_rgba", "k_assemble")


# ---- the two calls ----------------------------------------------------------------------------------------------------------
def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+m1v_set_input_layout\s*\(\s*m1v_encoder\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*size_t\s+\w+\s*,\s*int\s+\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_input_layout\s*\(\s*const\s+m1v_encoder\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)", code)
    assert re.search(r"M1V_ORDER_RGB\s*=\s*0\s*,\s*M1V_ORDER_BGR\s*=\s*1", code)
    L = _ffi.lib()
    for name in ("m1v_set_input_layout", "m1v_input_layout"):
        assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
    assert L.m1v_set_input_layout.restype is C.c_int
    assert list(L.m1v_set_input_layout.argtypes) == [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    assert L.m1v_input_layout.restype is C.c_int
    assert list(L.m1v_input_layout.argtypes) == [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    assert (_ffi.ORDER_RGB, _ffi.ORDER_BGR) == (0, 1)
    assert callable(Mpeg1Encoder.set_input_layout) and isinstance(Mpeg1Encoder.input_layout, property)


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    assert L.m1v_set_input_layout(None, 0, 0, 0) == _ffi.E_ARG
    assert L.m1v_set_input_layout(None, 4096, 0, 1) == _ffi.E_ARG
    pitch, stride, order = C.c_size_t(7), C.c_size_t(7), C.c_int(7)
    assert L.m1v_input_layout(None, C.byref(pitch), C.byref(stride), C.byref(order)) == _ffi.E_ARG
    assert (pitch.value, stride.value, order.value) == (7, 7, 7)


# ---- the stride helper (pure: shapes and strides only) ----------------------------------------------------------------------
def test_strides_of_a_packed_tensor():
    from ec504_imageencoder_amd import surface_strides
    assert surface_strides((5, 288, 352, 3), (288 * 352 * 3, 352 * 3, 3, 1)) == (352 * 3, 288 * 352 * 3)
    assert surface_strides((2, 1080, 1920, 4), (1080 * 1920 * 4, 1920 * 4, 4, 1)) == (1920 * 4, 1080 * 1920 * 4)


def test_strides_of_a_padded_pitch():
    from ec504_imageencoder_amd import surface_strides
    pitch = 352 * 4 + 256
    assert surface_strides((3, 288, 352, 4), (288 * pitch, pitch, 4, 1)) == (pitch, 288 * pitch)
    assert surface_strides((3, 288, 352, 3), (288 * (352 * 3 + 1), 352 * 3 + 1, 3, 1)) == (352 * 3 + 1, 288 * (352 * 3 + 1))


def test_strides_of_a_window_of_a_larger_surface():
    """surface[:, y0:y0+H, x0:x0+W, :] of a [n, 600, 800, 4] surface keeps the surface's strides."""
    from ec504_imageencoder_amd import surface_strides
    assert surface_strides((4, 288, 352, 4), (600 * 800 * 4, 800 * 4, 4, 1)) == (800 * 4, 600 * 800 * 4)


def test_strides_of_a_frame_gap_and_of_a_single_frame():
    from ec504_imageencoder_amd import surface_strides
    pitch = 352 * 3
    assert surface_strides((4, 288, 352, 3), (288 * pitch + 4099, pitch, 3, 1)) == (pitch, 288 * pitch + 4099)
    # the smallest stride that holds a frame's window: its last row ends where its pixels end
    assert surface_strides((2, 288, 352, 3), (287 * (pitch + 64) + pitch, pitch + 64, 3, 1)) == (pitch + 64, 287 * (pitch + 64) + pitch)
    # one frame: its stride says nothing (torch keeps any value there)
    assert surface_strides((1, 288, 352, 3), (1, pitch + 5, 3, 1)) == (pitch + 5, 288 * (pitch + 5))


def test_strides_that_no_layout_describes():
    from ec504_imageencoder_amd import surface_strides
    W, H = 352, 288
    with pytest.raises(ValueError):
        surface_strides((2, H, W, 3), (H * W * 4, W * 4, 4, 1))            # [..., :3] of an RGBA tensor: pixels 4 apart
    with pytest.raises(ValueError):
        surface_strides((2, H, W, 3), (H * W * 3, W * 3, 3, 2))            # bytes of a pixel not adjacent
    with pytest.raises(ValueError):
        surface_strides((2, H, W, 3), (H * W * 3, W * 3 - 1, 3, 1))        # a pitch below W * C
    with pytest.raises(ValueError):
        surface_strides((2, H, W // 2, 3), (H * W * 3, 0, 3, 1))           # expanded rows
    with pytest.raises(ValueError):
        surface_strides((2, H, W, 3), ((H - 1) * W * 3 + W * 3 - 1, W * 3, 3, 1))   # frames overlap
    with pytest.raises(ValueError):
        surface_strides((H, W, 3), (W * 3, 3, 1))


# ---- the code object --------------------------------------------------------------------------------------------------------
def _kernels(family):
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if family in n}
    recs = re.findall(r"\.name:\s*(\S*%s\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)" % family, notes, re.S)
    return bodies, recs


@pytest.mark.parametrize("family", FAMILIES)
def test_every_instantiation_exists(family):
    """[STAGE8][BPP][ORDER]: byte / halfword staging x 3- / 4-byte pixels x R,G,B / B,G,R."""
    bodies, recs = _kernels(family)
    assert len(bodies) == 8 and len(recs) == 8, (sorted(bodies), recs)
    for stage8 in (0, 1):
        for bpp in (3, 4):
            for order in (0, 1):
                pat = r"%sILb%dELi\d+ELi%dELi%dEE" % (family, stage8, bpp, order)
                assert sum(1 for n in bodies if re.search(pat, n)) == 1, (pat, sorted(bodies))


@pytest.mark.parametrize("family", FAMILIES)
def test_surface_kernel_shape(family):
    """Each instantiation brings its pixels in by LDS-DMA only (two instructions per row-step: sixteen), takes the integer row
    pass in the default rounding mode (sixteen v_mul_hi_i32, no MODE switch), evaluates the fp64 colour expression unfused,
    uses no scratch and at most 128 VGPRs; the ring is two row-steps deep and every row is read as soon as ITS two instructions
    have landed: the first eight vmcnt waits of the row loop are 2, 2, 2, 2, 2, 2, 2, 0."""
    bodies, recs = _kernels(family)
    assert bodies and recs
    for name, body in bodies.items():
        lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))]
        ops = [l.split()[0] for l in lines]
        assert sum(o == "global_load_lds_dwordx4" for o in ops) == 16, name
        assert sum(o.startswith("v_mul_hi_i32") for o in ops) == 16, name
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name
        assert not any(o.startswith(("v_fma_f64", "v_fmac_f64")) for o in ops), name
        if family == "k_encode_surface":
            assert not any(o.startswith(("global_load_dword", "flat_load")) for o in ops), name
        first_read = next(i for i, l in enumerate(lines) if l.startswith(("ds_read_b64", "ds_read_b128")))
        waits = [int(x) for l in lines[:first_read + 2500] for x in re.findall(r"s_waitcnt vmcnt\((\d+)\)", l)]
        assert waits[:8] == [2, 2, 2, 2, 2, 2, 2, 0], (name, waits[:12])
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0 and int(vgprs) <= 128, (name, scratch, vgprs)


def test_surface_kernels_keep_out_of_the_counted_names():
    """tests/test_abi.py, test_size_table_abi.py and test_rgba_table_abi.py count kernels by these substrings."""
    for family in FAMILIES:
        bodies, recs = _kernels(family)
        assert bodies and recs
        for name in list(bodies) + [r[0] for r in recs]:
            assert not any(c in name for c in COUNTED), name
