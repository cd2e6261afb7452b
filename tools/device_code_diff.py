#!/usr/bin/env python3
"""Are the gfx950 kernels of two trees the same code?  The evidence a host-only change needs before it rehashes the PMC record.

    python tools/device_code_diff.py <checkout or .s> <checkout or .s>

A checkout's m1v_kernels.hip is compiled with the Makefile's own HIPCC and HIPFLAGS plus -save-temps=obj (what `make isa`
does) into a temporary directory.  The device assembly is split per kernel into body, .amdhsa_kernel descriptor and metadata
entry, and the numbers of the local labels (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>), which only say in which order the functions were
emitted, are replaced.  Prints the count of kernels compared and every kernel that differs or exists on one side only; exits
non-zero on any difference.  It compares text: what the instructions are is none of its business."""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("ec504_imageencoder_amd", "csrc")


def device_asm(tree, workdir):
    """The text of the gfx950 assembly of `tree` (a checkout, or an assembly file that is read as it is)."""
    if os.path.isfile(tree):
        return open(tree).read()
    csrc = os.path.join(tree, CSRC)
    flags = subprocess.run(["make", "-s", "-C", csrc, "--eval", "print-hipcc: ; @echo $(HIPCC) $(HIPFLAGS)", "print-hipcc"],
                           check=True, capture_output=True, text=True).stdout.split()
    subprocess.run(flags + ["-save-temps=obj", "-c", "m1v_kernels.hip", "-o", os.path.join(workdir, "m1v.o")],
                   check=True, cwd=csrc)
    (asm,) = [f for f in os.listdir(workdir) if f.endswith(".s") and "amdgcn" in f]
    return open(os.path.join(workdir, asm)).read()


def normalise(lines):
    """The lines with the emission-order numbers of local labels replaced: the function's own number dropped, temporaries
    numbered by first appearance; runs of blanks collapsed (the comment column moves with a label's width)."""
    tmp = {}
    text = re.sub(r"BB\d+_(?=\d)", "BB_", "\n".join(" ".join(l.split()) for l in lines))  # .LBB<n>_<block>, and BB<n>_<block> in the loop comments
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    return re.sub(r"\.Ltmp(\d+)", lambda m: ".Ltmp_%d" % tmp.setdefault(m.group(1), len(tmp)), text)


def split_kernels(asm):
    """{kernel: normalised text of body + descriptor + metadata entry} of an assembly file."""
    body, desc, meta = {}, {}, {}
    cur = in_desc = entry = None
    in_meta = False
    for line in asm.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif re.match(r"\s*\.amdhsa_kernel\s", line):
            in_desc = line.split()[1]
            desc[in_desc] = []
        elif re.match(r"\s*\.end_amdhsa_kernel", line):
            in_desc = None
        elif in_desc:
            desc[in_desc].append(line.strip())
        elif re.match(r"\.Lfunc_end\d+:", line):
            cur = None
        elif cur:
            body[cur].append(line)
        elif line.startswith("amdhsa.kernels:"):
            in_meta = True
        elif in_meta and line.startswith("  - "):
            entry = []
            entry.append(line[4:].strip())
        elif in_meta and line.startswith("    ") and entry is not None:
            entry.append(line.rstrip())
            if line.strip().startswith(".name:"):
                meta[line.split()[1]] = entry
        elif in_meta:
            in_meta, entry = False, None
    return {k: normalise(body.get(k, []) + ["-- descriptor --"] + desc[k] + ["-- metadata --"] + meta.get(k, [])) for k in desc}


def compare(a, b):
    """(kernels on both sides, sorted names that differ or exist on one side only) of two split_kernels results."""
    return len(a.keys() & b.keys()), sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k))


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    sides = []
    for tree in argv[1:]:
        with tempfile.TemporaryDirectory() as workdir:
            sides.append(split_kernels(device_asm(tree, workdir)))
    both, differing = compare(*sides)
    print(f"{argv[1]}: {len(sides[0])} kernels, {argv[2]}: {len(sides[1])} kernels, compared {both}, differing {len(differing)}")
    for k in differing:
        print(("differs: " if k in sides[0] and k in sides[1] else f"only in {argv[1] if k in sides[0] else argv[2]}: ") + k)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
