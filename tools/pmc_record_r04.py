#!/usr/bin/env python3
"""Writes profiles/r04_pmc.json, the committed PMC record bench.py reads for `roofline.traffic` and `roofline.valu`, from the
summaries of tools/pmc_r04.sh (one directory per kernel and workload):

    python tools/pmc_record_r04.py gpurun_out/pmc4_base_runs_1920x1080 gpurun_out/pmc4_base_tiles_1920x1080 ...

The record carries the SHA-256 of the kernel sources it was measured on; bench.py reports whether that still matches the
tree (`pmc_fresh`) and tests/test_bench_record.py fails on a stale record, so a kernel change cannot leave old counters in
the bench line unnoticed.

A change that leaves every kernel's code as it was (tools/device_code_diff.py says so) keeps the counters and takes the hash again:

    python tools/pmc_record_r04.py --rehash [record.json]

recomputes `source_sha256` over the record's own `sources` and leaves everything else in the file as it is.

A change that leaves SOME kernels' code as it was (tools/device_code_diff.py names the ones that differ) measures the changed
ones again and keeps the counters of the others:

    python tools/pmc_record_r04.py --update OUT/pmc4_base_tiles_1920x1080 OUT/pmc4_base_tiles_3840x2160      (OUT: where tools/pmc_r04.sh wrote)

replaces the workloads of the given directories (same kernel, width and height) in the record and takes the hash again."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "r04_pmc.json")
SOURCES = ["ec504_imageencoder_amd/csrc/" + f for f in ("m1v_kernels.hip", "m1v_tiles.h", "m1v_planes.h", "m1v_encode_tile_body.h",
                                                        "m1v_size_table_body.h", "m1v_assemble.h", "fdct_f32.h", "m1v_downscale_planes.h")]


def source_sha256(sources=SOURCES):
    """bench.py's own hash (over the sources without comments and whitespace differences), so that both sides agree."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._pmc_sources_sha256(sources)


def rehash(path=RECORD):
    """Replaces the record's hash by the tree's over the record's own sources, in the text: nothing else in the file moves."""
    text = open(path).read()
    doc = json.loads(text)
    old, new = doc["source_sha256"], source_sha256(doc["sources"])
    open(path, "w").write(text.replace(f'"{old}"', f'"{new}"'))
    print(f"{path}: source_sha256 {old} -> {new}" if old != new else f"{path}: source_sha256 {old} is current")


def parse(path):
    out, cur = {}, None
    for line in open(path):
        if not line.startswith(" "):
            cur = line.strip()
            out[cur] = {}
        else:
            m = re.match(r"\s+(\S+)\s+n=\s*\d+ mean=(\S+)", line)
            if m and cur:
                out[cur][m.group(1)] = float(m.group(2))
    return out


def record_of(d):
    m = re.search(r"pmc4_(\w+?)_(runs|tiles)_(\d+)x(\d+)(?:_n(\d+))?", os.path.basename(d.rstrip("/")))
    if not m:
        raise SystemExit(f"{d}: not a tools/pmc_r04.sh directory")
    kernel = "k_encode_tiles" if m.group(2) == "tiles" else "k_encode_dense"
    c = parse(os.path.join(d, "summary.txt")).get(kernel)
    if not c:
        raise SystemExit(f"{d}: no counters of {kernel}")
    W, H = int(m.group(3)), int(m.group(4))
    rec = {"kernel": kernel, "width": W, "height": H, "frames": 300, "fetch_size_kib": c["FETCH_SIZE"], "write_size_kib": c["WRITE_SIZE"],
           "kernel_us_under_profiler": round(c["DURATION_NS"] / 1e3, 1), "l1_to_l2_read_requests": int(c["TCP_TCC_READ_REQ_sum"]),
           "pixel_lines_128B": W * H * 3 * 300 // 128, "source_dir": os.path.basename(d.rstrip("/")),
           "valu": {"insts_per_launch": int(c["SQ_INSTS_VALU"]), "simds": 1024,
                    "clock_ghz": round(c["GRBM_GUI_ACTIVE"] / 8 / (c["DURATION_NS"] * 1e-9) / 1e9, 3),
                    "source": "rocprofv3 --pmc SQ_INSTS_VALU (tools/pmc_r04.sh)"},
           "waves": int(c["SQ_WAVES"]), "wave_quad_cycles": c["SQ_WAVE_CYCLES"], "wait_any_quad_cycles": c["SQ_WAIT_ANY"],
           "ta_addr_stalled_by_tc_cycles": c["TA_ADDR_STALLED_BY_TC_CYCLES_sum"], "l2_hits": c["TCC_HIT_sum"], "l2_misses": c["TCC_MISS_sum"]}
    asm = parse(os.path.join(d, "summary.txt")).get("k_assemble")
    if asm:
        rec["assemble"] = {"kernel": "k_assemble", "kernel_us_under_profiler": round(asm["DURATION_NS"] / 1e3, 1),
                           "fetch_size_kib": asm.get("FETCH_SIZE"), "write_size_kib": asm.get("WRITE_SIZE"),
                           "insts_valu": int(asm["SQ_INSTS_VALU"]), "insts_salu": int(asm["SQ_INSTS_SALU"]), "waves": int(asm["SQ_WAVES"])}
    return rec


def main():
    if sys.argv[1:2] == ["--rehash"]:
        return rehash(*sys.argv[2:3])
    out = RECORD
    if sys.argv[1:2] == ["--update"]:
        doc = json.load(open(out))
        for rec in (record_of(d) for d in sys.argv[2:]):
            key = lambda r: (r["kernel"], r["width"], r["height"], r["frames"])
            at = [i for i, r in enumerate(doc["workloads"]) if key(r) == key(rec)]
            if not at:
                raise SystemExit(f"{rec['source_dir']}: the record has no such workload")
            doc["workloads"][at[0]] = rec
        doc["source_sha256"] = source_sha256(doc["sources"])
        json.dump(doc, open(out, "w"), indent=1)
        print(open(out).read())
        return
    recs = [record_of(d) for d in sys.argv[1:]]
    json.dump({"source_sha256": source_sha256(), "sources": SOURCES, "workloads": recs}, open(out, "w"), indent=1)
    print(open(out).read())


if __name__ == "__main__":
    main()
