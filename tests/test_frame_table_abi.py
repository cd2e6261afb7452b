"""CPU-side checks of the frame table (m1v_set_frame_table / m1v_frame_table, include/mpeg1_hip.h): the two calls are declared,
exported and bound, refuse a null encoder, and the Python mirror carries the setter, the property, the frames() helper and the
FrameTable object; the code object holds a kt_* twin of every tile-shaped kernel of a non-packed layout, of the same shape, and none
of a packed kernel."""
import ctypes as C
import os
import re

import pytest

from code_object import _kernels, _ops, _vgprs, _waves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the layout families whose kernels have a frame-table twin (kt_*), and their instantiations per row: [STAGE8] x the variants
TABLE_KERNELS = {"surface": 8, "planes": 4, "step2": 2, "rgb_planes": 2}
PACKED_KERNELS = ("k_encode_tiles", "k_size_table_tiles", "k_size_table_rgba", "k_rd_table_tiles", "k_rd_table_rgba")


def test_both_symbols_are_exported():
    from ec504_imageencoder_amd import _ffi
    raw = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
    L = _ffi.lib()
    for name in ("m1v_set_frame_table", "m1v_frame_table"):
        assert hasattr(raw, name), name
        assert name in _ffi.MPEG1_HIP_SYMBOLS and getattr(L, name).restype is C.c_int
    assert list(L.m1v_set_frame_table.argtypes) == [C.c_void_p, C.c_int]
    assert list(L.m1v_frame_table.argtypes) == [C.c_void_p]


def test_null_encoder():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    assert L.m1v_set_frame_table(None, 1) == _ffi.E_ARG
    assert L.m1v_set_frame_table(None, 0) == _ffi.E_ARG
    assert L.m1v_frame_table(None) == -1


def test_declared_and_documented():
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+m1v_set_frame_table\s*\(\s*m1v_encoder\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_frame_table\s*\(\s*const\s+m1v_encoder\s*\*\s*\w+\s*\)", code)
    # the definition, the alignment rule, when the table is read and what is left out are stated beside the declarations
    for phrase in ("uint64_t[n_frames]", "8-byte aligned", "on the stream", "not validated", "per plane"):
        assert phrase in text, phrase


def test_python_mirror():
    from ec504_imageencoder_amd import FrameTable, Mpeg1Encoder
    assert callable(Mpeg1Encoder.set_frame_table) and callable(Mpeg1Encoder.frames)
    assert isinstance(Mpeg1Encoder.frame_table, property)

    class _Table:           # what FrameTable reads of the int64 tensor it wraps
        shape, device = (5,), "cuda:0"

        def data_ptr(self):
            return 4096

    keep = [object(), object()]
    ft = FrameTable(_Table(), keep)
    assert ft.shape == (5,) and len(ft) == 5 and ft.device == "cuda:0" and ft.data_ptr() == 4096 and ft.frames == tuple(keep)


@pytest.mark.parametrize("row", ("encode", "size_table", "rd_table"))
@pytest.mark.parametrize("family", sorted(TABLE_KERNELS))
def test_every_table_instantiation_mirrors_its_stride_kernel(row, family):
    """kt_<row>_<family>: one instantiation beside every k_<row>_<family> (same template arguments), without scratch, at no lower
    occupancy by VGPRs than its twin, and with the stride kernel's loads from global memory into registers: the entry arrives by a
    scalar load."""
    stride, table = f"k_{row}_{family}", f"kt_{row}_{family}"
    want, got = _vgprs(stride), _vgprs(table)
    assert len(got) == len(want) == TABLE_KERNELS[family], (sorted(got), sorted(want))
    bodies_s, bodies_t = _kernels(stride)[0], _kernels(table)[0]
    assert len(bodies_t) == len(bodies_s) == TABLE_KERNELS[family]
    for name, (scratch, vgprs) in got.items():
        twin = name.replace(f"{len(table)}{table}I", f"{len(stride)}{stride}I")     # (the mangled name carries the length of the source name)
        assert twin in want, (name, twin)
        assert scratch == 0 and want[twin][0] == 0, name
        assert _waves(vgprs) >= _waves(want[twin][1]), (name, vgprs, want[twin][1])

        def vector_loads(body):
            return sorted(o[0] for o in _ops(body) if o[0].startswith(("global_load", "flat_load", "buffer_load", "scratch_")))

        assert vector_loads(bodies_t[name]) == vector_loads(bodies_s[twin]), name
        assert sum(o[0] == "s_load_dwordx2" for o in _ops(bodies_t[name])) >= 1, name


@pytest.mark.parametrize("family", PACKED_KERNELS)
def test_packed_kernels_have_no_table_twin(family):
    assert _kernels(family)[0] and not _kernels("kt_" + family[2:])[0]
