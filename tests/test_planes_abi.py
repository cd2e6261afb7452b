"""CPU-side checks of the plane input layout (m1v_plane_layout_preset / m1v_set_plane_layout / m1v_plane_layout_in_force,
include/mpeg1_hip.h): the calls and the struct are declared, exported and bound; the presets against hand-computed values and
against the Python mirror; the second checker of the GPU suite (tests/plane_oracle.py) pinned to the oracle; and the gfx950 code
object holds both plane kernel families (k_encode_planes, k_size_table_planes; csrc/m1v_planes.h) in every [staging][c_step]
instantiation with the shape the design needs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from code_object import _gfx950_disassembly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_encode_planes", "k_size_table_planes")
COUNTED = ("k_encode_tiles", "k_encode_dense", "k_encode_strips", "k_encode_surface", "k_size_table_tiles", "k_size_table_rgba",
           "k_size_table_surface", "k_assemble", "k_rate_pick")
FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")


# ---- the three calls and the struct -----------------------------------------------------------------------------------------
def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, plane_layout_preset
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_plane_layout\s*\{(.*?)\}\s*m1v_plane_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip() for n in re.sub(r"^\s*size_t", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS, members
    assert re.search(r"M1V_PLANES_REFERENCE\s*=\s*0\s*,\s*M1V_PLANES_I420\s*=\s*1\s*,\s*M1V_PLANES_YV12\s*=\s*2\s*,\s*"
                     r"M1V_PLANES_NV12\s*=\s*3\s*,\s*M1V_PLANES_NV21\s*=\s*4", code)
    assert re.search(r"\bint\s+m1v_plane_layout_preset\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*m1v_plane_layout\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_set_plane_layout\s*\(\s*m1v_encoder\s*\*\s*\w+\s*,\s*const\s+m1v_plane_layout\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_plane_layout_in_force\s*\(\s*const\s+m1v_encoder\s*\*\s*\w+\s*,\s*m1v_plane_layout\s*\*\s*\w+\s*\)", code)
    L = _ffi.lib()
    for name in ("m1v_plane_layout_preset", "m1v_set_plane_layout", "m1v_plane_layout_in_force"):
        assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert tuple(n for n, _ in _ffi.PlaneLayout._fields_) == FIELDS
    assert all(t is C.c_size_t for _, t in _ffi.PlaneLayout._fields_)
    assert C.sizeof(_ffi.PlaneLayout) == 7 * C.sizeof(C.c_size_t)
    assert list(L.m1v_plane_layout_preset.argtypes) == [C.c_int, C.c_int, C.c_int, C.POINTER(_ffi.PlaneLayout)]
    assert list(L.m1v_set_plane_layout.argtypes) == [C.c_void_p, C.POINTER(_ffi.PlaneLayout)]
    assert list(L.m1v_plane_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(_ffi.PlaneLayout)]
    assert _ffi.PLANE_PRESETS == {"reference": 0, "i420": 1, "yv12": 2, "nv12": 3, "nv21": 4}
    assert callable(Mpeg1Encoder.set_plane_layout) and isinstance(Mpeg1Encoder.plane_layout, property)
    assert callable(plane_layout_preset)


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    lay = _ffi.PlaneLayout(0, 100, 200, 10, 5, 1, 300)
    assert L.m1v_set_plane_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_plane_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_plane_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, (0, 100, 200, 10, 5, 1, 300)))
    assert L.m1v_plane_layout_preset(352, 288, 0, None) == _ffi.E_ARG


# hand-computed: (y_offset, cb_offset, cr_offset, y_pitch, c_pitch, c_step, frame_stride)
PRESETS = {
    (352, 288): {
        "reference": (0, 101376, 202752, 352, 176, 1, 304128),
        "i420": (0, 101376, 126720, 352, 176, 1, 152064),
        "yv12": (0, 126720, 101376, 352, 176, 1, 152064),
        "nv12": (0, 101376, 101377, 352, 352, 2, 152064),
        "nv21": (0, 101377, 101376, 352, 352, 2, 152064),
    },
    (1920, 1080): {
        "reference": (0, 2073600, 4147200, 1920, 960, 1, 6220800),
        "i420": (0, 2073600, 2592000, 1920, 960, 1, 3110400),
        "yv12": (0, 2592000, 2073600, 1920, 960, 1, 3110400),
        "nv12": (0, 2073600, 2073601, 1920, 1920, 2, 3110400),
        "nv21": (0, 2073601, 2073600, 1920, 1920, 2, 3110400),
    },
}


@pytest.mark.parametrize("size", sorted(PRESETS))
@pytest.mark.parametrize("name", ("reference", "i420", "yv12", "nv12", "nv21"))
def test_presets_against_hand_computed_values(size, name):
    from ec504_imageencoder_amd import _ffi, plane_layout_preset
    W, H = size
    lay = _ffi.PlaneLayout()
    assert _ffi.lib().m1v_plane_layout_preset(W, H, _ffi.PLANE_PRESETS[name], C.byref(lay)) == _ffi.OK
    want = dict(zip(FIELDS, PRESETS[size][name]))
    assert lay.as_dict() == want
    assert plane_layout_preset(W, H, name) == want


def test_preset_errors_and_the_python_mirror():
    from ec504_imageencoder_amd import _ffi, plane_layout_preset
    L = _ffi.lib()
    keep = dict(zip(FIELDS, (9, 9, 9, 9, 9, 9, 9)))
    for W, H in ((353, 288), (352, 289), (105, 49)):
        for name in ("i420", "yv12", "nv12", "nv21"):
            lay = _ffi.PlaneLayout(**keep)
            assert L.m1v_plane_layout_preset(W, H, _ffi.PLANE_PRESETS[name], C.byref(lay)) == _ffi.E_ARG, (W, H, name)
            assert lay.as_dict() == keep
            with pytest.raises(ValueError):
                plane_layout_preset(W, H, name)
        lay = _ffi.PlaneLayout()
        assert L.m1v_plane_layout_preset(W, H, _ffi.PLANES_REFERENCE, C.byref(lay)) == _ffi.OK
        assert lay.as_dict() == plane_layout_preset(W, H, "reference")
        assert lay.as_dict() == dict(zip(FIELDS, (0, W * H, 2 * W * H, W, W // 2, 1, 3 * W * H)))
    for preset in (-1, 5, 99):
        lay = _ffi.PlaneLayout(**keep)
        assert L.m1v_plane_layout_preset(352, 288, preset, C.byref(lay)) == _ffi.E_ARG
        assert lay.as_dict() == keep
    for W, H in ((0, 288), (352, 0), (-16, 16)):
        assert L.m1v_plane_layout_preset(W, H, 0, C.byref(_ffi.PlaneLayout())) == _ffi.E_ARG
        with pytest.raises(ValueError):
            plane_layout_preset(W, H, "reference")
    with pytest.raises(ValueError):
        plane_layout_preset(352, 288, "nv16")
    # every even geometry of a small sweep: the mirror is the library's arithmetic
    for W in (16, 96, 176, 354, 1918):
        for H in (16, 144, 290):
            for name, code in _ffi.PLANE_PRESETS.items():
                lay = _ffi.PlaneLayout()
                assert L.m1v_plane_layout_preset(W, H, code, C.byref(lay)) == _ffi.OK
                assert lay.as_dict() == plane_layout_preset(W, H, name), (W, H, name)


# ---- the second checker is pinned to the first ------------------------------------------------------------------------------
def _picture(W, H, seed):
    """Gradient + noise: encodable at the qualities used here, every block different."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * 2 + yy * 5) % 256], axis=-1)
    return ((base + rng.integers(0, 48, (H, W, 3))) % 256).astype(np.uint8)


@pytest.mark.parametrize("W,H,mode,qf,index", [
    (96, 48, "full", 12, 0), (96, 48, "full", 50, 300), (176, 144, "full", 12, 300), (176, 144, "full", 50, 0),
    (105, 49, "full", 40, 0), (105, 49, "full", 12, 300), (352, 288, "strict", 12, 0), (352, 288, "strict", 50, 300),
])
def test_plane_oracle_equals_the_oracle_on_converted_planes(orc, W, H, mode, qf, index):
    import plane_oracle
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    rgb = _picture(W, H, seed=W * 1000 + H + qf)
    want = orc.encode_frame(rgb, W, H, index, qf, m)
    frame = np.concatenate(orc.convert(rgb))
    got = plane_oracle.encode_layout(frame, plane_oracle.reference_layout(W, H), W, H, index, qf, m)
    assert got == want


def test_plane_oracle_reports_unencodable(orc):
    """A luma plane of 255 / 0 in bands of four rows: the block fails at quality 92 and codes at 76."""
    import plane_oracle
    W, H = 96, 48
    Y = np.where((np.arange(H)[:, None] % 8) < 4, 255, 0).astype(np.uint8).repeat(W, axis=1)
    frame = np.concatenate([Y.reshape(-1), np.full(2 * W * H, 128, np.uint8)])
    lay = plane_oracle.reference_layout(W, H)
    assert len(plane_oracle.encode_layout(frame, lay, W, H, 0, 76, orc.MODE_FULL)) > 48
    with pytest.raises(plane_oracle.Unencodable):
        plane_oracle.encode_layout(frame, lay, W, H, 0, 92, orc.MODE_FULL)


# ---- the code object --------------------------------------------------------------------------------------------------------
def _kernels(family):
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if family in n}
    recs = re.findall(r"\.name:\s*(\S*%s\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)" % family, notes, re.S)
    return bodies, recs


@pytest.mark.parametrize("family", FAMILIES)
def test_every_instantiation_exists(family):
    """[STAGE8][R][CSTEP]: byte / halfword staging x one plane per chroma component / interleaved pairs."""
    bodies, recs = _kernels(family)
    assert len(bodies) == 4 and len(recs) == 4, (sorted(bodies), recs)
    for stage8 in (0, 1):
        for cstep in (1, 2):
            pat = r"%sILb%dELi\d+ELi%dEE" % (family, stage8, cstep)
            assert sum(1 for n in bodies if re.search(pat, n)) == 1, (pat, sorted(bodies))


@pytest.mark.parametrize("family", FAMILIES)
def test_plane_kernel_shape(family):
    """Each instantiation brings its pixels in by LDS-DMA only (one 1-KiB instruction per two row-steps with one plane per
    chroma component: four; per row-step with interleaved pairs: eight; plus the three of the wave's VLC table), takes the
    integer row pass in the default rounding mode (sixteen v_mul_hi_i32, no MODE switch), holds no fp64 arithmetic or conversion
    at all (the colour stage is gone, not skipped at run time), uses no scratch, and fits 96 VGPRs (encode, byte staging) or 128.
    The row loop waits for one instruction at a time with the others in flight — vmcnt 3, 2, 1, 0, or 3 (five times), 2, 1, 0 —
    so vmcnt(0) is its last wait only."""
    bodies, recs = _kernels(family)
    assert bodies and recs
    for name, body in bodies.items():
        cstep = int(re.search(r"ILb\dELi\d+ELi(\d)EE", name).group(1))
        lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))]
        ops = [l.split()[0] for l in lines]
        n_dma = 4 if cstep == 1 else 8
        assert sum(o == "global_load_lds_dwordx4" for o in ops) == n_dma, name
        assert sum(o == "global_load_lds_dword" for o in ops) == 3, name
        assert sum(o.startswith("v_mul_hi_i32") for o in ops) == 16, name
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name
        assert not any(re.match(r"v_\w*f64", o) for o in ops), (name, [o for o in ops if "f64" in o][:4])
        if family == "k_encode_planes":
            assert not any(o.startswith(("global_load_dword", "global_load_ubyte", "global_load_ushort", "global_load_sbyte",
                                         "global_load_short", "flat_load", "buffer_load")) for o in ops), name
        first_read = next(i for i, l in enumerate(lines) if l.startswith("ds_read_b64"))
        waits = [int(x) for l in lines[:first_read + 2500] for x in re.findall(r"s_waitcnt vmcnt\((\d+)\)", l)]
        want = [3, 2, 1, 0] if cstep == 1 else [3, 3, 3, 3, 3, 2, 1, 0]
        assert waits[:len(want)] == want, (name, waits[:12])
    for name, scratch, vgprs in recs:
        narrow_encode = family == "k_encode_planes" and "ILb1E" in name
        assert int(scratch) == 0 and int(vgprs) <= (96 if narrow_encode else 128), (name, scratch, vgprs)


def test_plane_kernels_keep_out_of_the_counted_names():
    """The existing code-object tests count kernels by these substrings."""
    for family in FAMILIES:
        bodies, recs = _kernels(family)
        assert bodies and recs
        for name in list(bodies) + [r[0] for r in recs]:
            assert not any(c in name for c in COUNTED), name
