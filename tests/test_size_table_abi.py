"""CPU-side checks of the size table (m1v_frame_size_table_device, include/mpeg1_hip.h): the entry point is declared, exported
and bound, argument errors are reported without a device, and its tile kernel in the gfx950 code object has the shape the
design needs (no scratch, no MODE switch, the default-rounding row pass, at most 128 VGPRs)."""
import ctypes as C
import os
import re

import pytest

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "m1v_frame_size_table_device"


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import _ffi
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    L = _ffi.lib()
    assert NAME in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, NAME)
    fn = getattr(L, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 8


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    assert L.m1v_frame_size_table_device(None, None, 0, q, 2, None, None, None) == _ffi.E_ARG
    assert "null" in _ffi.last_error()


def _kernels():
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if "k_size_table_tiles" in n}
    recs = re.findall(r"\.name:\s*(\S*k_size_table_tiles\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)", notes, re.S)
    return bodies, recs


def test_size_table_kernel_shape():
    """Both stagings (byte and halfword levels) exist; neither touches scratch, switches MODE or multiplies by 181/128 (the
    round-down row pass is k_encode_tiles' alone: tests/test_abi.py::test_rounding_mode_of_the_pixel_stage); the row pass is the
    integer form (sixteen v_mul_hi_i32); the pixels arrive by LDS-DMA as in k_encode_tiles; <= 128 VGPRs."""
    bodies, recs = _kernels()
    assert len(bodies) == 2 and len(recs) == 2, (sorted(bodies), recs)
    for name, body in bodies.items():
        lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))]
        ops = [l.split()[0] for l in lines]
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any("0x3fb50000" in l for l in lines), name
        assert not any(o.startswith(("scratch_", "v_fma_f64", "v_fmac_f64")) for o in ops), name
        assert sum(o.startswith("v_mul_hi_i32") for o in ops) == 16, name
        assert sum(o == "global_load_lds_dwordx4" for o in ops) == 16, name
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0 and int(vgprs) <= 128, (name, scratch, vgprs)


@pytest.mark.parametrize("forbidden", ["k_encode_dense", "k_encode_strips", "k_encode_tiles", "k_assemble"])
def test_size_table_kernels_keep_out_of_the_counted_names(forbidden):
    """tests/test_abi.py counts the encode kernels by these substrings."""
    bodies, _ = _kernels()
    assert bodies and not any(forbidden in n for n in bodies)
