"""CPU-side checks of the plane table (m1v_set_plane_table / m1v_plane_table, include/mpeg1_hip.h): the two calls are declared,
exported and bound, refuse a null encoder, the header states the definition, and the Python mirror carries the setter, the property
and plane_frames(); the code object holds a kp_* twin of every plane and RGB plane kernel, of the same template arguments, without
scratch and at its twin's occupancy, which fetches the three entries with scalar loads, and none of any other kernel."""
import ctypes as C
import os
import re

import pytest

from code_object import _kernels, _ops, _vgprs, _waves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the layout families whose kernels have a plane-table twin (kp_*), and their instantiations per row: [STAGE8] x the chroma steps
PLANE_KERNELS = {"planes": 4, "rgb_planes": 2}
# ... and what the existing frame-table test pins per row, which the new prefix must leave alone
TABLE_KERNELS = {"surface": 8, "planes": 4, "step2": 2, "rgb_planes": 2}
ROWS = ("encode", "size_table", "rd_table")
NO_TWIN = ("encode_tiles", "size_table_tiles", "size_table_rgba", "rd_table_tiles", "rd_table_rgba") + \
    tuple(f"{row}_{family}" for row in ROWS for family in ("surface", "step2"))


def test_both_symbols_are_exported():
    from ec504_imageencoder_amd import _ffi
    raw = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
    L = _ffi.lib()
    for name in ("m1v_set_plane_table", "m1v_plane_table"):
        assert hasattr(raw, name), name
        assert name in _ffi.MPEG1_HIP_SYMBOLS and getattr(L, name).restype is C.c_int
    assert list(L.m1v_set_plane_table.argtypes) == [C.c_void_p, C.c_int]
    assert list(L.m1v_plane_table.argtypes) == [C.c_void_p]


def test_null_encoder():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    assert L.m1v_set_plane_table(None, 1) == _ffi.E_ARG
    assert "null encoder" in _ffi.last_error()
    assert L.m1v_set_plane_table(None, 0) == _ffi.E_ARG
    assert L.m1v_plane_table(None) == -1


def test_declared_and_documented():
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+m1v_set_plane_table\s*\(\s*m1v_encoder\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_plane_table\s*\(\s*const\s+m1v_encoder\s*\*\s*\w+\s*\)", code)
    # the definition, the alignment rule, when the table is read, the read contract per plane and what is left out
    for phrase in ("uint64_t[n_frames][3]", "8-byte aligned", "on the stream", "Read contract, per plane",
                   "E_p = p_offset + (rows_p - 1) * pitch_p + row_bytes_p", "Y, Cb, Cr", "R, G, B", "P010"):
        assert phrase in text, phrase
    # what tests/test_frame_table_abi.py looks for is still there
    for phrase in ("uint64_t[n_frames]", "8-byte aligned", "on the stream", "not validated", "per plane"):
        assert phrase in text, phrase
    comment = text[text.index("/* Frame table:"):text.index("int m1v_set_frame_table")]
    assert "uint64_t[n_frames] " in comment and "Not covered" in comment and "P010" in comment and "host-buffer" in comment


def test_python_mirror():
    from ec504_imageencoder_amd import FrameTable, Mpeg1Encoder
    assert callable(Mpeg1Encoder.set_plane_table) and callable(Mpeg1Encoder.plane_frames)
    assert isinstance(Mpeg1Encoder.plane_table, property)
    assert callable(Mpeg1Encoder.set_frame_table) and callable(Mpeg1Encoder.frames) and isinstance(Mpeg1Encoder.frame_table, property)

    class _Table:           # what FrameTable reads of the int64 [n, 3] tensor it wraps: the class and its constructor are as they were
        shape, device = (5, 3), "cuda:0"

        def data_ptr(self):
            return 4096

    ft = FrameTable(_Table(), [object()] * 15)
    assert ft.shape == (5,) and len(ft) == 5 and ft.data_ptr() == 4096 and len(ft.frames) == 15


def _template_arguments(name, source):
    """The template arguments of a mangled kernel name, between its source name and its parameter list."""
    return re.search(r"\d+%sI(.*?)Ev" % source, name).group(1)


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("family", sorted(PLANE_KERNELS))
def test_every_plane_table_instantiation_mirrors_its_stride_kernel(row, family):
    """kp_<row>_<family>: one instantiation beside every k_<row>_<family> (same template arguments), without scratch, at no lower
    occupancy by VGPRs than its twin; the three entries arrive by scalar loads."""
    stride, table = f"k_{row}_{family}", f"kp_{row}_{family}"
    want, got = _vgprs(stride), _vgprs(table)
    assert len(got) == len(want) == PLANE_KERNELS[family], (sorted(got), sorted(want))
    twins = {_template_arguments(n, stride): n for n in want}
    bodies = _kernels(table)[0]
    assert len(bodies) == PLANE_KERNELS[family] and len(twins) == len(want)
    for name, (scratch, vgprs) in got.items():
        twin = twins.get(_template_arguments(name, table))
        assert twin, (name, sorted(twins))
        assert scratch == 0 and want[twin][0] == 0, name
        assert _waves(vgprs) >= _waves(want[twin][1]), (name, vgprs, want[twin][1])
        loads = [o for o in _ops(bodies[name]) if o[0] == "s_load_dwordx2"]
        by_base = {}
        for o in loads:
            by_base.setdefault(o[2], set()).add(int(o[3], 0))
        assert len(loads) >= 3 and any({0, 8, 16} <= offs for offs in by_base.values()), (name, by_base)
        # the two-base fetch: the LDS-DMA that covers two planes takes one 64-bit address per lane
        assert any(o[0] == "global_load_lds_dwordx4" and o[-1] == "off" for o in _ops(bodies[name])), name


@pytest.mark.parametrize("kernel", NO_TWIN)
def test_other_kernels_have_no_plane_table_twin(kernel):
    assert _kernels("k_" + kernel)[0] and not _kernels("kp_" + kernel)[0]


@pytest.mark.parametrize("row", ROWS)
def test_the_frame_table_counts_still_hold(row):
    """The kt_* and k_* counts that tests/test_frame_table_abi.py pins: the prefix kp_ keeps its expressions from matching."""
    for family, count in TABLE_KERNELS.items():
        assert len(_kernels(f"k_{row}_{family}")[0]) == len(_kernels(f"kt_{row}_{family}")[0]) == count, (row, family)
