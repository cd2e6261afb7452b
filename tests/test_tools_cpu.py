"""The two tools a host-only change leans on, on the CPU: tools/device_code_diff.py (are the kernels of two trees the same
code?) on hand-written assembly, no compiler; tools/pmc_record_r04.py --rehash (take the PMC record's hash again) on a copy."""
import importlib.util
import json
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernel(name, fn, body, vgprs=8):
    """One kernel as the compiler lays it out: the body between .type and .Lfunc_end, its descriptor inside."""
    return (f"\t.section\t.text.{name}\n\t.type\t{name},@function\n{name}:\n{body}"
            f"\t.section\t.rodata\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr {vgprs}\n\t.end_amdhsa_kernel\n"
            f"\t.section\t.text.{name}\n.Lfunc_end{fn}:\n\t.size\t{name}, .Lfunc_end{fn}-{name}\n")


def _file(kernels):
    meta = "".join(f"  - .agpr_count:     0\n    .args:\n      - .offset:         0\n    .name:           {k}\n    .vgpr_count:     8\n"
                   for k, _ in kernels)
    return "".join(text for _, text in kernels) + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + meta + "...\n\t.end_amdgpu_metadata\n"


def _loop(fn, tmp, addend="1"):
    return (f"\ts_mov_b32 s0, 0\n.LBB{fn}_1:{' ' * (12 - len(str(fn)))}; =>This Loop Header: Depth=1\n\ts_add_i32 s0, s0, {addend}\n"
            f".Ltmp{tmp}:\n\ts_cbranch_scc0 .LBB{fn}_1\n; %bb.2:                ;   in Loop: Header=BB{fn}_1 Depth=1\n\ts_endpgm\n")


def test_device_code_diff_ignores_emission_order_and_reports_real_differences():
    d = _tool("device_code_diff")
    left = d.split_kernels(_file([("k_a", _kernel("k_a", 0, _loop(0, 3))), ("k_b", _kernel("k_b", 1, _loop(1, 4, "2")))]))
    # the same two kernels emitted in the other order: other function numbers, other temporaries, a wider label column
    right = d.split_kernels(_file([("k_b", _kernel("k_b", 10, _loop(10, 0, "2"))), ("k_a", _kernel("k_a", 11, _loop(11, 7)))]))
    assert set(left) == {"k_a", "k_b"} and "s_add_i32 s0, s0, 2" in left["k_b"] and ".amdhsa_next_free_vgpr 8" in left["k_b"]
    assert ".name: k_b" in left["k_b"] and "k_a" not in left["k_b"]
    assert d.compare(left, right) == (2, [])
    # one operand
    changed = d.split_kernels(_file([("k_a", _kernel("k_a", 0, _loop(0, 3))), ("k_b", _kernel("k_b", 1, _loop(1, 4, "3")))]))
    assert d.compare(left, changed) == (2, ["k_b"])
    # a descriptor field
    assert d.compare(left, d.split_kernels(_file([("k_a", _kernel("k_a", 0, _loop(0, 3), vgprs=16)),
                                                   ("k_b", _kernel("k_b", 1, _loop(1, 4, "2")))]))) == (2, ["k_a"])
    # a kernel on one side only, either side
    alone = d.split_kernels(_file([("k_a", _kernel("k_a", 0, _loop(0, 3)))]))
    assert d.compare(left, alone) == (1, ["k_b"]) and d.compare(alone, left) == (1, ["k_b"])


def test_pmc_record_tool_hashes_the_sources_the_record_names():
    record = json.load(open(os.path.join(ROOT, "profiles", "r04_pmc.json")))
    assert _tool("pmc_record_r04").SOURCES == record["sources"]


def test_pmc_rehash_changes_the_hash_and_nothing_else(tmp_path):
    tool = _tool("pmc_record_r04")
    committed = os.path.join(ROOT, "profiles", "r04_pmc.json")
    before = json.load(open(committed))
    stale = dict(before, source_sha256="0" * 64)
    copy = str(tmp_path / "record.json")
    json.dump(stale, open(copy, "w"), indent=1)
    tool.rehash(copy)
    after = json.load(open(copy))
    assert after["source_sha256"] == tool.source_sha256(before["sources"]) != stale["source_sha256"]
    assert {k: v for k, v in after.items() if k != "source_sha256"} == {k: v for k, v in before.items() if k != "source_sha256"}
    # on a current record: not one byte moves
    shutil.copy(committed, copy)
    tool.rehash(copy)
    assert open(copy, "rb").read() == open(committed, "rb").read()
