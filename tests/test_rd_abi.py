"""CPU-side checks of the rd table and the rate-distortion encode (m1v_frame_rd_table_device, m1v_encode_rd_device,
include/mpeg1_hip.h): the entry points and constants are declared, exported and bound, argument errors are reported without a
device, the kernels of the rd-table row exist for every input layout and use no scratch, and the host helpers that turn a
distortion into dB and back are consistent."""
import ctypes as C
import math
import os
import re

import pytest

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"m1v_frame_rd_table_device": 9, "m1v_encode_rd_device": 17}


def _header():
    return open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()


@pytest.mark.parametrize("name", sorted(ARGS))
def test_declared_exported_and_bound(name):
    from ec504_imageencoder_amd import _ffi
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, _header())
    assert m, name
    assert len(m.group(1).split(",")) == ARGS[name]
    L = _ffi.lib()
    assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name)
    fn = getattr(L, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == ARGS[name]


def test_signatures_match_the_header():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    vp, u8p = C.c_void_p, C.POINTER(C.c_uint8)
    assert L.m1v_frame_rd_table_device.argtypes == [vp, vp, C.c_int, u8p, C.c_int, vp, vp, vp, vp]
    # enc, d_rgb, n_frames, first, candidates, n_candidates, rule, limit, d_limits, d_chosen, d_out, out_cap, sizes, dist, total, status, stream
    assert L.m1v_encode_rd_device.argtypes == [vp, vp, C.c_int, C.c_int, u8p, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, C.c_size_t,
                                               vp, vp, vp, vp, vp]
    decl = re.search(r"\bint\s+m1v_encode_rd_device\s*\(([^;]*)\);", _header()).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["enc", "d_rgb", "n_frames", "first_frame_index", "candidates", "n_candidates", "rule", "limit", "d_limits",
                     "d_chosen", "d_out", "out_cap", "d_frame_sizes", "d_frame_distortion", "d_total", "d_status", "stream"]


def test_constants():
    from ec504_imageencoder_amd import _ffi
    text = _header()
    assert re.search(r"M1V_RD_BEST_IN_BUDGET\s*=\s*0\s*,\s*M1V_RD_SMALLEST_AT_DISTORTION\s*=\s*1", text)
    assert re.search(r"M1V_STATUS_OVER_DISTORTION\s*=\s*32u", text)
    assert (_ffi.RD_BEST_IN_BUDGET, _ffi.RD_SMALLEST_AT_DISTORTION, _ffi.STATUS_OVER_DISTORTION) == (0, 1, 32)
    bits = [_ffi.STATUS_UNENCODABLE, _ffi.STATUS_NOSPACE, _ffi.STATUS_SCRATCH, _ffi.STATUS_QUALITY, _ffi.STATUS_OVER_BUDGET,
            _ffi.STATUS_OVER_DISTORTION]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32]


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    assert L.m1v_frame_rd_table_device(None, None, 0, q, 2, None, None, None, None) == _ffi.E_ARG
    assert "null" in _ffi.last_error()
    assert L.m1v_encode_rd_device(None, None, 0, 0, q, 2, 0, 0, None, None, None, 0, None, None, None, None, None) == _ffi.E_ARG
    assert "null" in _ffi.last_error()


def test_rd_table_kernels_exist_for_every_layout_and_use_no_scratch():
    """The instantiations of the size-table row: both staging widths of the packed 3- and 4-channel kernels, of the four surface
    orders and of chroma step 1 and 2; 0 bytes of private segment each; at most 128 VGPRs, as the size table."""
    _, notes = _gfx950_disassembly()
    recs = re.findall(r"\.name:\s*(\S*k_rd_table_(?:tiles|rgba|surface|planes)\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)",
                      notes, re.S)
    by_family = {}
    for name, scratch, vgprs in recs:
        assert int(scratch) == 0 and int(vgprs) <= 128, (name, scratch, vgprs)
        family = re.search(r"k_rd_table_([a-z]+)", name).group(1)
        by_family[family] = by_family.get(family, 0) + 1
    assert by_family == {"tiles": 2, "rgba": 2, "surface": 8, "planes": 4}, by_family


def test_psnr_helpers():
    from ec504_imageencoder_amd import distortion_to_psnr, psnr_to_distortion
    blocks = 22 * 18 * 6
    assert distortion_to_psnr(0, blocks) == math.inf
    assert distortion_to_psnr(255 * 255 * 64 * blocks, blocks) == pytest.approx(0.0, abs=1e-12)
    assert distortion_to_psnr(1232963, blocks) == pytest.approx(10 * math.log10(255.0 ** 2 * 64 * blocks / 1232963))
    for db in (20.0, 33.3, 45.0):
        d = psnr_to_distortion(db, blocks)
        assert distortion_to_psnr(d, blocks) >= db - 1e-9 and distortion_to_psnr(d + 2, blocks) < db
    with pytest.raises(ValueError):
        distortion_to_psnr(-1, blocks)
    with pytest.raises(ValueError):
        psnr_to_distortion(30, 0)
