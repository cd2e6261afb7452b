"""Host-side checks of the luma colour sums of the tile kernels (csrc/m1v_kernels.hip, luma_sums_denormal and convert_row_tile):
the exhaustive proof of their arithmetic, what the code object must keep for it to hold, and the claims of the GPU test's
content (tests/luma_denormal.py).

The row pass is not touched (the pixels return to unit scale in the and-or that cuts them from the sums), so
tools/fdct_f32_proof.cpp has no new instantiation and tests/test_host_tables.py keeps running it as it is."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import luma_denormal as ld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
TILE_KERNELS = ("k_encode_tilesILb0ELi", "k_encode_tilesILb1ELi", "k_coefficient_tilesILi")


def test_denormal_colour_sums_over_all_rgb_triples_and_phases(tmp_path):
    """tools/colour_fast_proof.c denormal [down]: for all 2^24 triples x the four dword phases of a pixel, Y coefficients, in
    round-to-nearest and rounded toward minus infinity (the tile kernels' mode): the sum of masked-in-place bytes and rescaled
    coefficients is the unit-scale sum * 2^-24 bit for bit, the same pixels are flagged by the integer test on its low 15 bits,
    and one and-or returns the raw pixel at unit scale.  (The two modes run side by side: 10 s each, denormal operands are slow
    on the host.)"""
    exe = str(tmp_path / "proof")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-frounding-math", os.path.join(ROOT, "tools", "colour_fast_proof.c"), "-o", exe, "-lm"],
                   check=True)
    runs = [subprocess.Popen([exe, "denormal"] + mode, stdout=subprocess.PIPE, text=True) for mode in ([], ["down"])]
    for p in runs:
        out = p.communicate()[0]
        assert p.returncode == 0, out
        assert "4 phases x 16777216 triples; flagged 16774 per phase" in out and all(
            f"{what}: 0" in out for what in ("t' != t * 2^-24", "flags differ", "pixels differ", "subnormal sums")), out


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    obj = os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_kernels.o")
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(obj)):
        pytest.skip("llvm tools or object file absent")
    td = str(tmp_path_factory.mktemp("co"))
    shutil.copy(obj, os.path.join(td, "k.o"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=td, capture_output=True, text=True)
    cos = glob.glob(os.path.join(td, "k.o.*gfx950*"))
    if not cos:
        pytest.skip("cannot extract the gfx950 code object")
    return cos[0]


def test_tile_kernels_keep_fp32_denormals_and_convert_chroma_only(code_object):
    """What the denormal sums need of the code object, per tile kernel that takes them (both stagings of k_encode_tiles and
    k_coefficient_tiles):
    * fp32 denormals enabled in the kernel descriptor (a flushed operand would read every colour byte as 0) and, as
      tests/test_abi.py checks, one switch of MODE that writes its two fp32 rounding bits only;
    * 192 byte-to-float conversions, the chroma wave's 8 rows x 24: the luma arm has none;
    * 64 and-ors (mask from a scalar, bias from a vector register), one per pixel of the 8 rows, and no scratch
      (tests/test_abi.py holds the register budget)."""
    objdump = os.path.join(LLVM, "llvm-objdump")
    desc = subprocess.run([objdump, "-D", "-j", ".rodata", code_object], capture_output=True, text=True).stdout
    text = subprocess.run([objdump, "-d", code_object], capture_output=True, text=True).stdout
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.S | re.M)}
    kds = {m.group(1): m.group(2) for m in re.finditer(r"^[0-9a-f]+ <(\S+)\.kd>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", desc, re.S | re.M)}
    for stem in TILE_KERNELS:
        names = [k for k in bodies if stem in k]
        assert len(names) == 1, (stem, names)
        body, kd = bodies[names[0]], kds[names[0]]
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", kd), (stem, kd)
        assert len(re.findall(r"\bs_setreg_imm32_b32 hwreg\(HW_REG_MODE, 0, 2\), 2", body)) == 1 and body.count("s_setreg") == 1, stem
        assert len(re.findall(r"\bv_cvt_f32_ubyte[0-3]", body)) == 192, stem
        assert len(re.findall(r"\bv_and_or_b32 v\d+, v\d+, s\d+, v\d+", body)) >= 64, stem
        assert "scratch_" not in body, stem


def test_tie_content_holds_every_tie_colour_at_every_phase():
    """tests/luma_denormal.py: the tie colours include every Y sum the kernel can flag (the proof flags 16774 per phase), and
    the frames of every size hold each of them at each of the four byte phases."""
    ties = ld.luma_tie_colours()
    assert 16774 <= len(ties) < 40000
    code = lambda px: (px[:, 0].astype(np.int64) << 16) | (px[:, 1].astype(np.int64) << 8) | px[:, 2]
    want = set((code(ties)[:, None] * 4 + np.arange(4)).reshape(-1).tolist())
    for W, H in ld.SIZES:
        px = ld.content("ties", W, H).reshape(-1, 3)
        phase = (3 * np.arange(len(px))) & 3
        assert want <= set((code(px) * 4 + phase).tolist()), (W, H)
        for name in ("extremes", "noise"):
            f = ld.content(name, W, H)
            assert f.shape == (2, H, W, 3) and (name == "noise" or set(np.unique(f).tolist()) == {0, 255})
