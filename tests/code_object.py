"""The gfx950 code object of csrc/m1v_kernels.o as the *_abi.py tests read it: unbundled and disassembled once per run, the parsed
forms that several of those tests share, and the lists of kernel names that one of them takes from another."""
import functools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=1)
def disassembly():
    """(llvm-objdump -d, llvm-readobj --notes) of the gfx950 code object in m1v_kernels.o: some 900,000 lines of text, so every
    test of a run reads this one copy.  (A skip raises, so it is not cached: each test that asks is skipped.)"""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    obj = os.path.join(ROOT, "ec504_imageencoder_amd", "csrc", "m1v_kernels.o")
    if not (os.path.exists(objdump) and os.path.exists(obj)):
        pytest.skip("llvm tools or object absent")
    import glob
    import shutil
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(obj, os.path.join(td, "k.o"))
        subprocess.run([objdump, "--offloading", "k.o"], cwd=td, capture_output=True, text=True)
        cos = glob.glob(os.path.join(td, "k.o.*gfx950*"))
        if not cos:
            pytest.skip("cannot extract the gfx950 code object")
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readobj", "--notes", cos[0]], capture_output=True, text=True).stdout
        return subprocess.run([objdump, "-d", cos[0]], capture_output=True, text=True).stdout, notes


_gfx950_disassembly = disassembly       # the name its call sites in the test modules have always used


# tests/test_rgb_planes_abi.py: what the code-object tests of the other input layouts count kernels by
RGB_PLANES_COUNTED = ("k_encode_tiles", "k_encode_dense", "k_encode_strips", "k_encode_surface", "k_encode_planes", "k_encode_step2",
                      "k_size_table_tiles", "k_size_table_rgba", "k_size_table_surface", "k_size_table_planes", "k_size_table_step2",
                      "k_rd_table_tiles", "k_rd_table_rgba", "k_rd_table_surface", "k_rd_table_planes", "k_rd_table_step2", "k_assemble",
                      "k_rate_pick")


# tests/test_sample_layout_abi.py: what the code-object tests of the other input layouts count kernels by (test_planes_abi.py,
# test_surface_abi.py, test_rgba_table_abi.py, test_rd_abi.py)
SAMPLE_LAYOUT_COUNTED = ("k_encode_tiles", "k_encode_dense", "k_encode_strips", "k_encode_surface", "k_encode_planes", "k_size_table_tiles",
                         "k_size_table_rgba", "k_size_table_surface", "k_size_table_planes", "k_rd_table_tiles", "k_rd_table_rgba",
                         "k_rd_table_surface", "k_rd_table_planes", "k_assemble", "k_rate_pick")


# tests/test_float_planes_abi.py: the families whose names the issue of the float plane layout lists; no new mangled name may
# contain one
EXISTING = ("k_encode_planes", "k_size_table_planes", "k_encode_rgb_planes", "k_size_table_rgb_planes", "k_rd_table_rgb_planes",
            "k_encode_step2", "k_encode_surface", "k_size_table_tiles")


@functools.lru_cache(maxsize=1)
def _code_object():
    """({kernel: body}, [(kernel, scratch bytes, VGPRs)]) of the whole code object, disassembled and parsed once per run."""
    asm, notes = _gfx950_disassembly()
    bodies = dict(re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S))
    recs = re.findall(r"\.name:\s*(_ZN\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)", notes, re.S)
    return bodies, recs


def _kernels(family):
    bodies, recs = _code_object()
    mine = re.compile(r"\d+%sI" % family)
    return {n: b for n, b in bodies.items() if mine.search(n)}, [r for r in recs if mine.search(r[0])]


def _ops(body):
    return [l.split("//")[0].split() for l in body.splitlines() if l.split("//")[0].strip() and not l.strip().startswith(("/", ";"))]


def _waves(vgprs):
    """Waves per SIMD that a VGPR count allows on gfx950: 512 registers per lane in blocks of 8, 8 waves at most."""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def _vgprs(family):
    """{mangled name: (scratch bytes, VGPRs)} of a kernel family."""
    return {n: (int(sc), int(v)) for n, sc, v in _kernels(family)[1]}
