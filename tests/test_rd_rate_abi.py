"""CPU-side checks of the batch and bitrate picks by distortion (m1v_encode_rd_batch_device, m1v_encode_rd_cbr_device,
m1v_rd_batch_pick_device, m1v_rd_cbr_pick_device, include/mpeg1_hip.h): the entry points are declared, exported and bound with
the header's arguments, a null encoder is an argument error without a device, the constants are those of the rd encode, and the
three pick kernels are in the gfx950 code object without scratch."""
import ctypes as C
import os
import re

import pytest

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "m1v_encode_rd_batch_device": ["enc", "d_rgb", "n_frames", "first_frame_index", "candidates", "n_candidates", "rule", "limit",
                                   "d_chosen", "d_out", "out_cap", "d_frame_sizes", "d_frame_distortion", "d_total", "d_status",
                                   "stream"],
    "m1v_encode_rd_cbr_device": ["enc", "d_rgb", "n_frames", "first_frame_index", "candidates", "n_candidates", "bytes_per_frame",
                                 "buffer_bytes", "d_level_in", "d_level_out", "d_chosen", "d_out", "out_cap", "d_frame_sizes",
                                 "d_frame_distortion", "d_total", "d_status", "stream"],
    "m1v_rd_batch_pick_device": ["enc", "d_sizes", "d_distortion", "d_table_status", "n_frames", "n_candidates", "rule", "limit",
                                 "d_picks", "d_pick_distortion", "d_status", "stream"],
    "m1v_rd_cbr_pick_device": ["enc", "d_sizes", "d_distortion", "d_table_status", "n_frames", "n_candidates", "bytes_per_frame",
                               "buffer_bytes", "d_level_in", "d_level_out", "d_picks", "d_pick_distortion", "d_status", "stream"],
}


def _header():
    return open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_exported_and_bound(name):
    from ec504_imageencoder_amd import _ffi
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, _header())
    assert m, name
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == NAMES[name]
    L = _ffi.lib()
    assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name)
    fn = getattr(L, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(NAMES[name])


def test_signatures_match_the_header():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    vp, u8p, i, u64, sz = C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_uint64, C.c_size_t
    assert L.m1v_encode_rd_batch_device.argtypes == [vp, vp, i, i, u8p, i, i, u64, vp, vp, sz, vp, vp, vp, vp, vp]
    assert L.m1v_encode_rd_cbr_device.argtypes == [vp, vp, i, i, u8p, i, u64, u64, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    assert L.m1v_rd_batch_pick_device.argtypes == [vp, vp, vp, vp, i, i, i, u64, vp, vp, vp, vp]
    assert L.m1v_rd_cbr_pick_device.argtypes == [vp, vp, vp, vp, i, i, u64, u64, vp, vp, vp, vp, vp, vp]


def test_constants_are_unchanged():
    from ec504_imageencoder_amd import _ffi
    text = _header()
    assert re.search(r"M1V_RD_BEST_IN_BUDGET\s*=\s*0\s*,\s*M1V_RD_SMALLEST_AT_DISTORTION\s*=\s*1", text)
    assert re.search(r"M1V_STATUS_OVER_DISTORTION\s*=\s*32u", text)
    assert (_ffi.RD_BEST_IN_BUDGET, _ffi.RD_SMALLEST_AT_DISTORTION) == (0, 1)
    assert (_ffi.STATUS_OVER_BUDGET, _ffi.STATUS_OVER_DISTORTION, _ffi.MAX_CANDIDATES) == (16, 32, 8)
    import rd_rate_model
    assert (rd_rate_model.BEST_IN_BUDGET, rd_rate_model.SMALLEST_AT_DISTORTION, rd_rate_model.UNENCODABLE) == (0, 1, 1)


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    calls = (
        lambda: L.m1v_encode_rd_batch_device(None, None, 0, 0, q, 2, 0, 0, None, None, 0, None, None, None, None, None),
        lambda: L.m1v_encode_rd_cbr_device(None, None, 0, 0, q, 2, 100, 1000, None, None, None, None, 0, None, None, None, None, None),
        lambda: L.m1v_rd_batch_pick_device(None, None, None, None, 0, 2, 0, 0, None, None, None, None),
        lambda: L.m1v_rd_cbr_pick_device(None, None, None, None, 0, 2, 100, 1000, None, None, None, None, None, None),
    )
    for call in calls:
        assert call() == _ffi.E_ARG
        assert "null" in _ffi.last_error()


def test_python_methods_exist():
    from ec504_imageencoder_amd import Mpeg1Encoder
    for name in ("encode_best_in_batch_budget", "encode_batch_to_distortion", "encode_best_at_bitrate", "rd_batch_pick",
                 "rd_bitrate_pick"):
        assert callable(getattr(Mpeg1Encoder, name)), name


def test_pick_kernels_exist_and_use_no_scratch():
    """k_rd_chains, k_rd_batch_pick and k_rd_cbr_pick: one instantiation each, 0 bytes of private segment, no spills."""
    _, notes = _gfx950_disassembly()
    recs = re.findall(r"\.name:\s*(\S*k_rd_(?:chains|batch_pick|cbr_pick)\S*).*?\.private_segment_fixed_size:\s*(\d+)"
                      r".*?\.vgpr_spill_count:\s*(\d+)", notes, re.S)
    kinds = sorted(re.search(r"k_rd_(chains|batch_pick|cbr_pick)", name).group(1) for name, _, _ in recs)
    assert kinds == ["batch_pick", "cbr_pick", "chains"], recs
    for name, scratch, spills in recs:
        assert int(scratch) == 0 and int(spills) == 0, (name, scratch, spills)
