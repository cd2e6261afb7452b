"""CPU-side checks of the per-frame quality / frame-size budget ABI (include/mpeg1_hip.h): the three entry points and the two
status bits are declared, exported and bound, and argument errors are reported without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m1v_encode_quality_device", "m1v_frame_sizes_device", "m1v_encode_budget_device")


def _header():
    return open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()


def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import _ffi
    text = _header()
    L = _ffi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes, name


def test_status_bits_match_the_header():
    from ec504_imageencoder_amd import _ffi
    text = _header()
    assert re.search(r"M1V_STATUS_QUALITY\s*=\s*8u", text) and re.search(r"M1V_STATUS_OVER_BUDGET\s*=\s*16u", text)
    assert (_ffi.STATUS_QUALITY, _ffi.STATUS_OVER_BUDGET) == (8, 16)
    bits = [_ffi.STATUS_UNENCODABLE, _ffi.STATUS_NOSPACE, _ffi.STATUS_SCRATCH, _ffi.STATUS_QUALITY, _ffi.STATUS_OVER_BUDGET]
    assert sum(bits) == 31 and all(b & (b - 1) == 0 for b in bits)


def test_null_encoder_is_an_argument_error():
    """No device needed: the entry points refuse a null encoder before touching the runtime."""
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    assert L.m1v_encode_quality_device(None, None, 0, 0, None, None, 0, None, None, None, None) == _ffi.E_ARG
    assert L.m1v_frame_sizes_device(None, None, 0, None, None, None, None) == _ffi.E_ARG
    assert L.m1v_encode_budget_device(None, None, 0, 0, q, 2, 1000, None, None, None, 0, None, None, None, None) == _ffi.E_ARG
    assert "null" in _ffi.last_error()
