"""CPU-side checks of the budget per stream (include/mpeg1_hip.h "Streams: a budget per stream":
m1v_encode_streams_budget_device, m1v_streams_budget_pick_device): the prototypes and the constants are in the header, exported and
bound; a null encoder, null spans and an unknown rule are argument errors without a device; the Python methods exist; and exactly
the k_span_* kernels of csrc/m1v_span_budget.h are in the gfx950 code object, without scratch and under names no other test counts."""
import ctypes as C
import os
import re

import pytest

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "m1v_encode_streams_budget_device": ["enc", "d_rgb", "n_frames", "d_spans", "n_streams", "candidates", "n_candidates", "rule", "limit",
                                         "d_stream_limits", "d_chosen", "d_out", "out_cap", "d_frame_sizes", "d_frame_distortion",
                                         "d_stream_bytes", "d_stream_status", "d_total", "d_status", "stream"],
    "m1v_streams_budget_pick_device": ["enc", "d_sizes", "d_distortion", "d_table_status", "n_frames", "n_candidates", "d_spans",
                                       "n_streams", "rule", "limit", "d_stream_limits", "d_picks", "d_pick_distortion",
                                       "d_stream_status", "d_status", "stream"],
}
# the substrings and the pattern by which other tests count kernels of the code object
COUNTED = ("k_streams_", "k_rd_chains", "k_rd_batch_pick", "k_rd_cbr_pick", "k_rate_pick", "k_assemble", "float_planes", "k_float_pixels_")
TILE_SHAPED = r"k[tp]?_(?:encode|size_table|rd_table)_"


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
    assert L.m1v_encode_streams_budget_device.argtypes == [vp, vp, i, vp, i, u8p, i, i, u64, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    assert L.m1v_streams_budget_pick_device.argtypes == [vp, vp, vp, vp, i, i, vp, i, i, u64, vp, vp, vp, vp, vp, vp]


def test_the_constants():
    from ec504_imageencoder_amd import _ffi
    import streams_budget_model as bm
    text = _header()
    assert "Streams: a budget per stream" in text
    assert re.search(r"M1V_SPANS_LARGEST_THAT_FITS\s*=\s*0\s*,\s*M1V_SPANS_LEAST_DISTORTION\s*=\s*1\s*,\s*M1V_SPANS_SMALLEST_AT_DISTORTION\s*=\s*2", text)
    assert (_ffi.SPANS_LARGEST_THAT_FITS, _ffi.SPANS_LEAST_DISTORTION, _ffi.SPANS_SMALLEST_AT_DISTORTION) == (0, 1, 2)
    assert _ffi.SPANS_RULES["size"] == 0 and _ffi.SPANS_RULES["distortion"] == 1 and set(_ffi.SPANS_RULES.values()) == {0, 1, 2}
    assert bm.RULES == (0, 1, 2)
    assert bm.OVER_BIT == _ffi.SPANS_OVER_BITS == {0: _ffi.STATUS_OVER_BUDGET, 1: _ffi.STATUS_OVER_BUDGET, 2: _ffi.STATUS_OVER_DISTORTION}


def test_argument_errors_need_no_device():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    spans = (_ffi.StreamSpan * 1)(_ffi.StreamSpan(0, 0, 0, 0))
    sp = C.cast(spans, C.c_void_p)
    enc = C.c_void_p(8)   # never dereferenced: the spans are checked behind the encoder and in front of everything else

    def encode(e, s, rule=0, n_streams=1):
        return L.m1v_encode_streams_budget_device(e, None, 0, s, n_streams, q, 2, rule, 100, None, None, None, 0, None, None, None, None,
                                                  None, None, None)

    def pick(e, s, rule=0, n_streams=1):
        return L.m1v_streams_budget_pick_device(e, None, None, None, 0, 2, s, n_streams, rule, 100, None, None, None, None, None, None)

    for call in (encode, pick):
        for e, s in ((None, sp), (enc, None)):
            assert call(e, s) == _ffi.E_ARG
            assert "null" in _ffi.last_error()
        for n_streams in (0, -1, _ffi.MAX_STREAMS + 1):
            assert call(enc, sp, n_streams=n_streams) == _ffi.E_ARG
            assert "n_streams" in _ffi.last_error()
        assert call(enc, C.c_void_p(sp.value + 2)) == _ffi.E_ARG
        assert "aligned" in _ffi.last_error()
    # an unknown rule: the pick-only call checks it behind the spans, in front of anything it reads of the encoder
    for rule in (-1, 3, 99):
        assert pick(enc, sp, rule=rule) == _ffi.E_ARG
        assert "rule" in _ffi.last_error()


def test_python_surface_exists():
    import ec504_imageencoder_amd as pkg
    for name in ("encode_streams_to_budget", "encode_streams_to_distortion", "streams_budget_pick"):
        assert callable(getattr(pkg.Mpeg1Encoder, name)), name


def test_exactly_the_span_kernels_exist_without_scratch():
    """k_span_plan and k_span_budget (one instantiation per rule): 0 bytes of private segment, no spills; and none of their names
    holds a substring by which another test counts kernels."""
    _, notes = _gfx950_disassembly()
    recs = re.findall(r"\.name:\s*(\S*k_span_\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)", notes, re.S)
    kinds = sorted(re.search(r"k_span_([a-z]+)", name).group(1) for name, _, _ in recs)
    assert kinds == ["budget", "budget", "budget", "plan"], recs
    assert len({name for name, _, _ in recs}) == 4
    for name, scratch, spills in recs:
        assert int(scratch) == 0 and int(spills) == 0, (name, scratch, spills)
        assert not any(c in name for c in COUNTED), name
        assert not re.search(TILE_SHAPED, name), name
