"""CPU-side checks of the sample input layout (m1v_sample_layout_preset / m1v_set_sample_layout / m1v_sample_layout_in_force,
include/mpeg1_hip.h): the calls and the struct are declared, exported and bound; the presets against hand-computed values and
against the Python mirror; the checker of the GPU suite (tests/sample_oracle.py) pinned to tests/plane_oracle.py where the two
overlap; and the gfx950 code object holds the three step-2 kernel families (k_encode_step2, k_size_table_step2,
k_rd_table_step2; csrc/m1v_step2.h) in both stagings with the shape the design needs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from code_object import _gfx950_disassembly
from code_object import SAMPLE_LAYOUT_COUNTED as COUNTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("k_encode_step2", "k_size_table_step2", "k_rd_table_step2")
FIELDS = ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "y_step", "c_step", "frame_stride")
NAMES = ("yuy2", "uyvy", "yvyu", "p010")


# ---- the three calls and the struct -----------------------------------------------------------------------------------------
def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi, sample_layout_preset
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+m1v_sample_layout\s*\{(.*?)\}\s*m1v_sample_layout\s*;", code, re.S)
    assert m
    members = [n for decl in m.group(1).split(";") if decl.strip() for n in re.sub(r"^\s*size_t", "", decl).replace(" ", "").split(",")]
    assert tuple(members) == FIELDS, members
    assert re.search(r"M1V_SAMPLES_YUY2\s*=\s*0\s*,\s*M1V_SAMPLES_UYVY\s*=\s*1\s*,\s*M1V_SAMPLES_YVYU\s*=\s*2\s*,\s*M1V_SAMPLES_P010\s*=\s*3", code)
    assert re.search(r"\bint\s+m1v_sample_layout_preset\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*m1v_sample_layout\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_set_sample_layout\s*\(\s*m1v_encoder\s*\*\s*\w+\s*,\s*const\s+m1v_sample_layout\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+m1v_sample_layout_in_force\s*\(\s*const\s+m1v_encoder\s*\*\s*\w+\s*,\s*m1v_sample_layout\s*\*\s*\w+\s*\)", code)
    # the definition, the even-row rule and the truncation are stated beside the declarations
    for phrase in ("y_step", "EVEN picture rows", "truncation, not rounding", "P012 and P016"):
        assert phrase in text, phrase
    L = _ffi.lib()
    for name in ("m1v_sample_layout_preset", "m1v_set_sample_layout", "m1v_sample_layout_in_force"):
        assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert tuple(n for n, _ in _ffi.SampleLayout._fields_) == FIELDS
    assert all(t is C.c_size_t for _, t in _ffi.SampleLayout._fields_)
    assert C.sizeof(_ffi.SampleLayout) == 8 * C.sizeof(C.c_size_t)
    assert C.sizeof(_ffi.PlaneLayout) == 7 * C.sizeof(C.c_size_t)                   # the older struct keeps its size
    assert list(L.m1v_sample_layout_preset.argtypes) == [C.c_int, C.c_int, C.c_int, C.POINTER(_ffi.SampleLayout)]
    assert list(L.m1v_set_sample_layout.argtypes) == [C.c_void_p, C.POINTER(_ffi.SampleLayout)]
    assert list(L.m1v_sample_layout_in_force.argtypes) == [C.c_void_p, C.POINTER(_ffi.SampleLayout)]
    assert _ffi.SAMPLE_PRESETS == {"yuy2": 0, "uyvy": 1, "yvyu": 2, "p010": 3}
    assert callable(Mpeg1Encoder.set_sample_layout) and isinstance(Mpeg1Encoder.sample_layout, property)
    assert callable(Mpeg1Encoder.set_plane_layout) and isinstance(Mpeg1Encoder.plane_layout, property)
    assert callable(sample_layout_preset)


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    lay = _ffi.SampleLayout(0, 1, 3, 64, 128, 2, 4, 1024)
    assert L.m1v_set_sample_layout(None, None) == _ffi.E_ARG
    assert L.m1v_set_sample_layout(None, C.byref(lay)) == _ffi.E_ARG
    assert L.m1v_sample_layout_in_force(None, C.byref(lay)) == _ffi.E_ARG
    assert lay.as_dict() == dict(zip(FIELDS, (0, 1, 3, 64, 128, 2, 4, 1024)))
    assert L.m1v_sample_layout_preset(352, 288, 0, None) == _ffi.E_ARG


# hand-computed: (y_offset, cb_offset, cr_offset, y_pitch, c_pitch, y_step, c_step, frame_stride)
PRESETS = {
    (352, 288): {
        "yuy2": (0, 1, 3, 704, 1408, 2, 4, 202752),
        "uyvy": (1, 0, 2, 704, 1408, 2, 4, 202752),
        "yvyu": (0, 3, 1, 704, 1408, 2, 4, 202752),
        "p010": (1, 202753, 202755, 704, 704, 2, 4, 304128),
    },
    (16, 16): {
        "yuy2": (0, 1, 3, 32, 64, 2, 4, 512),
        "uyvy": (1, 0, 2, 32, 64, 2, 4, 512),
        "yvyu": (0, 3, 1, 32, 64, 2, 4, 512),
        "p010": (1, 513, 515, 32, 32, 2, 4, 768),
    },
}


@pytest.mark.parametrize("size", sorted(PRESETS))
@pytest.mark.parametrize("name", NAMES)
def test_presets_against_hand_computed_values(size, name):
    from ec504_imageencoder_amd import _ffi, sample_layout_preset
    from ec504_imageencoder_amd.encoder import plane_layout_extent
    W, H = size
    lay = _ffi.SampleLayout()
    assert _ffi.lib().m1v_sample_layout_preset(W, H, _ffi.SAMPLE_PRESETS[name], C.byref(lay)) == _ffi.OK
    want = dict(zip(FIELDS, PRESETS[size][name]))
    assert lay.as_dict() == want
    assert sample_layout_preset(W, H, name) == want
    # the extent of the tightly packed frame, one past its last addressed byte: the frame's last byte is a luma sample in UYVY
    # and the Cr word's high byte in P010; in YUY2 and YVYU it is a chroma byte of an odd row, which nobody addresses
    extent = plane_layout_extent(want, W // 16, H // 16)
    assert extent == want["frame_stride"] - (1 if name in ("yuy2", "yvyu") else 0)


def test_preset_errors_and_the_python_mirror():
    from ec504_imageencoder_amd import _ffi, plane_layout_preset, sample_layout_preset
    L = _ffi.lib()
    keep = dict(zip(FIELDS, (9,) * 8))
    for W, H in ((353, 288), (352, 289), (105, 49)):
        for name in NAMES:
            lay = _ffi.SampleLayout(**keep)
            assert L.m1v_sample_layout_preset(W, H, _ffi.SAMPLE_PRESETS[name], C.byref(lay)) == _ffi.E_ARG, (W, H, name)
            assert lay.as_dict() == keep
            with pytest.raises(ValueError):
                sample_layout_preset(W, H, name)
    for preset in (-1, 4, 5, 99):
        lay = _ffi.SampleLayout(**keep)
        assert L.m1v_sample_layout_preset(352, 288, preset, C.byref(lay)) == _ffi.E_ARG
        assert lay.as_dict() == keep
    for W, H in ((0, 288), (352, 0), (-16, 16)):
        assert L.m1v_sample_layout_preset(W, H, 0, C.byref(_ffi.SampleLayout())) == _ffi.E_ARG
        with pytest.raises(ValueError):
            sample_layout_preset(W, H, "yuy2")
    with pytest.raises(ValueError):
        sample_layout_preset(352, 288, "nv12")
    for W in (16, 96, 176, 354, 1918):
        for H in (16, 144, 290):
            for name, code in _ffi.SAMPLE_PRESETS.items():
                lay = _ffi.SampleLayout()
                assert L.m1v_sample_layout_preset(W, H, code, C.byref(lay)) == _ffi.OK
                assert lay.as_dict() == sample_layout_preset(W, H, name), (W, H, name)
    # the older preset call is what it was: code 5 is no plane preset, and its struct is untouched by the refusal
    old = _ffi.PlaneLayout(9, 9, 9, 9, 9, 9, 9)
    assert L.m1v_plane_layout_preset(352, 288, 5, C.byref(old)) == _ffi.E_ARG
    assert old.as_dict() == dict.fromkeys(("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride"), 9)
    with pytest.raises(ValueError):
        plane_layout_preset(352, 288, "yuy2")


def test_extent_with_steps():
    """plane_layout_extent with the steps put in: luma row bytes (xe - 1) * y_step + 1, chroma row bytes (xe / 2 - 1) * c_step + 1;
    a plane layout (no y_step) is what it was."""
    from ec504_imageencoder_amd import plane_layout_preset, sample_layout_preset
    from ec504_imageencoder_amd.encoder import plane_layout_extent
    W, H = 176, 80
    lay = sample_layout_preset(W, H, "yuy2")
    assert plane_layout_extent(lay, 11, 5) == max(79 * 352 + 175 * 2 + 1, 3 + 39 * 704 + 87 * 4 + 1) == 28159
    assert plane_layout_extent(dict(lay, y_offset=1, cb_offset=0, cr_offset=2), 11, 5) == 28160
    assert plane_layout_extent(sample_layout_preset(W, H, "p010"), 11, 5) == 2 * W * H + 3 + 39 * 352 + 87 * 4 + 1 == 3 * W * H
    nv12 = plane_layout_preset(W, H, "nv12")
    assert plane_layout_extent(nv12, 11, 5) == plane_layout_extent(dict(nv12, y_step=1), 11, 5) == W * H * 3 // 2


# ---- the helper is pinned to the plane oracle -------------------------------------------------------------------------------
def test_sample_oracle_equals_the_plane_oracle_with_luma_step_one(orc):
    import plane_oracle
    import sample_oracle
    from ec504_imageencoder_amd import plane_layout_preset
    W, H = 96, 48
    rng = np.random.default_rng(7)
    for name in ("nv12", "i420"):
        lay = plane_layout_preset(W, H, name)
        frame = rng.integers(0, 256, lay["frame_stride"], dtype=np.uint8)
        a, b = plane_oracle.layout_samplers(frame, lay), sample_oracle.layout_samplers(frame, dict(lay, y_step=1))
        for x, y in ((0, 0), (8, 8), (80, 32), (88, 40)):
            assert np.array_equal(a[0](x, y), b[0](x, y))
        for p in (0, 1):
            for x, y in ((0, 0), (80, 32)):
                assert np.array_equal(a[1](p, x, y), b[1](p, x, y))
        for qf, index in ((12, 0), (50, 300)):
            assert sample_oracle.encode_layout(frame, dict(lay, y_step=1), W, H, index, qf, orc.MODE_FULL) == \
                plane_oracle.encode_layout(frame, lay, W, H, index, qf, orc.MODE_FULL)


def test_sample_oracle_reads_yuy2_as_the_scattered_planes(orc):
    """A YUY2 frame through the helper equals its samples scattered into I420 planes (chroma of the even rows) through the plane
    oracle; the 255 / 0 luma bands of four rows (test_planes_abi.py) fail at quality 92 and code at 76."""
    import plane_oracle
    import sample_oracle
    from ec504_imageencoder_amd import plane_layout_preset, sample_layout_preset
    W, H = 96, 48
    lay = sample_layout_preset(W, H, "yuy2")
    frame = np.random.default_rng(8).integers(0, 256, lay["frame_stride"], dtype=np.uint8)
    rows = frame.reshape(H, 2 * W)
    i420 = np.concatenate([rows[:, 0::2].reshape(-1), rows[0::2, 1::4].reshape(-1), rows[0::2, 3::4].reshape(-1)])
    assert sample_oracle.encode_layout(frame, lay, W, H, 3, 12, orc.MODE_FULL) == \
        plane_oracle.encode_layout(i420, plane_layout_preset(W, H, "i420"), W, H, 3, 12, orc.MODE_FULL)
    bands = np.full((H, 2 * W), 128, np.uint8)
    bands[:, 0::2] = np.where((np.arange(H)[:, None] % 8) < 4, 255, 0)
    assert len(sample_oracle.encode_layout(bands.reshape(-1), lay, W, H, 0, 76, orc.MODE_FULL)) > 48
    with pytest.raises(sample_oracle.Unencodable):
        sample_oracle.encode_layout(bands.reshape(-1), lay, W, H, 0, 92, orc.MODE_FULL)


def test_addressed_mask_counts_three_bytes_per_two_pixels():
    import sample_oracle
    from ec504_imageencoder_amd import sample_layout_preset
    W, H = 48, 32
    for name in NAMES:
        lay = sample_layout_preset(W, H, name)
        mask = sample_oracle.addressed_mask(lay, W, H, lay["frame_stride"])
        assert int(mask.sum()) == W * H * 3 // 2, name


# ---- the code object --------------------------------------------------------------------------------------------------------
def _kernels(family):
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if family in n}
    recs = re.findall(r"\.name:\s*(\S*%s\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)" % family, notes, re.S)
    return bodies, recs


@pytest.mark.parametrize("family", FAMILIES)
def test_every_instantiation_exists(family):
    """[STAGE8][R]: byte / halfword staging, one ring."""
    bodies, recs = _kernels(family)
    assert len(bodies) == 2 and len(recs) == 2, (sorted(bodies), recs)
    for stage8 in (0, 1):
        pat = r"%sILb%dELi\d+EE" % (family, stage8)
        assert sum(1 for n in bodies if re.search(pat, n)) == 1, (pat, sorted(bodies))


@pytest.mark.parametrize("family", FAMILIES)
def test_step2_kernel_shape(family):
    """Each instantiation brings its pixels in by LDS-DMA only (one 1-KiB instruction per row-step: eight; plus the three of the
    wave's VLC table), takes the integer row pass in the default rounding mode (sixteen v_mul_hi_i32, no MODE switch), holds no
    fp64 arithmetic or conversion, uses no scratch, and fits 96 VGPRs (encode, byte staging) or 128.  The row loop waits for one
    instruction at a time with three in flight — vmcnt 3 (five times), 2, 1, 0 — so vmcnt(0) is its last wait only."""
    bodies, recs = _kernels(family)
    assert bodies and recs
    for name, body in bodies.items():
        lines = [l.split("//")[0].strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))]
        ops = [l.split()[0] for l in lines]
        assert sum(o == "global_load_lds_dwordx4" for o in ops) == 8, name
        assert sum(o == "global_load_lds_dword" for o in ops) == 3, name
        assert sum(o.startswith("v_mul_hi_i32") for o in ops) == 16, name
        assert not any(o.startswith("s_setreg") for o in ops), name
        assert not any(o.startswith("scratch_") for o in ops), name
        assert not any(re.match(r"v_\w*f64", o) for o in ops), (name, [o for o in ops if "f64" in o][:4])
        if family == "k_encode_step2":
            assert not any(o.startswith(("global_load_dword", "global_load_ubyte", "global_load_ushort", "global_load_sbyte",
                                         "global_load_short", "flat_load", "buffer_load")) for o in ops), name
        first_read = next(i for i, l in enumerate(lines) if l.startswith("ds_read_b64"))
        waits = [int(x) for l in lines[:first_read + 2500] for x in re.findall(r"s_waitcnt vmcnt\((\d+)\)", l)]
        assert waits[:8] == [3, 3, 3, 3, 3, 2, 1, 0], (name, waits[:12])
    for name, scratch, vgprs in recs:
        narrow_encode = family == "k_encode_step2" and "ILb1E" in name
        assert int(scratch) == 0 and int(vgprs) <= (96 if narrow_encode else 128), (name, scratch, vgprs)


def test_step2_kernels_keep_out_of_the_counted_names():
    """The existing code-object tests count kernels by these substrings."""
    for family in FAMILIES:
        bodies, recs = _kernels(family)
        assert bodies and recs
        for name in list(bodies) + [r[0] for r in recs]:
            assert not any(c in name for c in COUNTED), name
