"""CPU-side checks of the fused size table for 4-channel input (k_size_table_rgba, csrc/m1v_tiles.h) and of the query that
tells a caller what a size table costs (m1v_size_table_fused, include/mpeg1_hip.h): the query is declared, exported and bound,
a null encoder gives -1, and the gfx950 code object holds the kernel in both stagings with the shape the design needs."""
import ctypes as C
import os
import re

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "m1v_size_table_fused"
KERNEL = "k_size_table_rgba"
COUNTED = ("k_size_table_tiles", "k_encode_dense", "k_encode_strips", "k_encode_tiles", "k_assemble")


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+m1v_encoder\s*\*" % NAME, text)
    L = _ffi.lib()
    assert NAME in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, NAME)
    fn = getattr(L, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 1
    assert isinstance(Mpeg1Encoder.size_table_fused, property)


def test_null_encoder_gives_minus_one():
    from ec504_imageencoder_amd import _ffi
    assert _ffi.lib().m1v_size_table_fused(None) == -1


def _kernels():
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if KERNEL in n}
    recs = re.findall(r"\.name:\s*(\S*%s\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)" % KERNEL, notes, re.S)
    return bodies, recs


def test_rgba_table_kernel_shape():
    """Both stagings (byte and halfword levels) exist.  Each brings its pixels in by LDS-DMA (two instructions per row-step:
    sixteen), takes the integer row pass in the default rounding mode (sixteen v_mul_hi_i32, no MODE switch), uses no scratch
    and at most 128 VGPRs."""
    bodies, recs = _kernels()
    assert len(bodies) == 2 and len(recs) == 2, (sorted(bodies), recs)
    assert any("ILb0E" in n for n in bodies) and any("ILb1E" in n for n in bodies), sorted(bodies)
    for name, body in bodies.items():
        lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))]
        ops = [l.split()[0] for l in lines]
        assert sum(o == "global_load_lds_dwordx4" for o in ops) == 16, name
        assert sum(o.startswith("v_mul_hi_i32") for o in ops) == 16, name
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name
        assert not any(o.startswith(("v_fma_f64", "v_fmac_f64")) for o in ops), name
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0 and int(vgprs) <= 128, (name, scratch, vgprs)


def test_rgba_table_kernel_keeps_out_of_the_counted_names():
    """tests/test_abi.py and tests/test_size_table_abi.py count kernels by these substrings."""
    bodies, recs = _kernels()
    assert bodies and recs
    for name in list(bodies) + [r[0] for r in recs]:
        assert not any(c in name for c in COUNTED), name
