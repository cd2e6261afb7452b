#!/usr/bin/env python3
"""What pass 1 of the tile kernels' bits stage sees on the bench content (k_synth: uniform random bytes), counted with the CPU
oracle alone: one frame, FULL region, the oracle's levels (tests/oracle_ffi.py frame_coefficients), emit_set and the walk
restated from csrc/m1v_kernels.hip.  Blocks are grouped by 64 in the oracle's order as a stand-in for a wave: a wave's trip
count is the largest number of coded levels among its 64 blocks, and a trip is "touched" by a property when any lane that is
still active in it has the property.

    python tools/bits_trip_stats.py [--w 1920 --h 1080 --quality 12 --seed 504]

profiles/r29_bits_trip.txt holds the output for the bench shape."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import code_space as cs          # noqa: E402
import oracle_ffi as orc         # noqa: E402

M64 = (1 << 64) - 1


def emit_set(nz):
    stop = nz & (nz << 1) & M64
    below = ((stop & -stop) - 1) if stop else M64
    return nz & ~1 & below, stop == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--quality", type=int, default=12)
    ap.add_argument("--seed", type=int, default=504)
    a = ap.parse_args()
    rows = cs.row_lengths(orc)
    px = orc.synth_frames(1, a.w, a.h, seed=a.seed)[0]
    z = orc.frame_coefficients(px, a.w, a.h, a.quality, orc.MODE_FULL)
    weights = 1 << np.arange(64, dtype=object)
    blocks, no_pair = [], 0
    for lv in z:
        nz = int(((lv != 0).astype(object) * weights).sum())
        emit, free = emit_set(nz)
        no_pair += free
        codes, prev = [], 0 if lv[0] != 0 else -1
        while emit:
            p = (emit & -emit).bit_length() - 1
            emit &= emit - 1
            r, L = p - prev - 2, abs(int(lv[p]))
            codes.append((p, r, L, r < 32 and L <= rows[r]))
            prev = p
        blocks.append(codes)
    n = len(blocks)
    coded = [c for b in blocks for c in b]
    trips, other, high = [], 0, 0
    for g in range(0, n - n % 64, 64):
        wave = blocks[g:g + 64]
        t = max(len(b) for b in wave)
        trips.append(t)
        for k in range(t):
            lanes = [b[k] for b in wave if len(b) > k]
            other += any(not (c[2] == 1 and c[3]) for c in lanes)
            high += any(c[0] >= 32 for c in lanes)
    total = sum(trips)
    dist = {k: trips.count(k) / len(trips) for k in sorted(set(trips))}
    print(f"content: synthetic frame 0 of seed {a.seed}, {a.w}x{a.h}, FULL, quality {a.quality}; {n} blocks, {len(trips)} groups of 64")
    print(f"coded AC levels per block                        {len(coded) / n:.2f}")
    print(f"loop trips per group of 64: mean                 {total / len(trips):.2f}")
    print("                            distribution         " + "  ".join(f"{k}: {100 * v:.0f} %" for k, v in dist.items()))
    print(f"coded levels that are +-1                        {100 * sum(c[2] == 1 for c in coded) / len(coded):.1f} %")
    print(f"codes that take the escape                       {100 * sum(not c[3] for c in coded) / len(coded):.1f} %")
    print(f"   of them with run - 1 >= 32 (no table row)     {100 * sum(c[1] >= 32 for c in coded) / len(coded):.1f} %")
    print(f"trips with a lane outside 'level +-1, table'     {100 * other / total:.0f} %")
    print(f"trips that touch a zigzag position >= 32         {100 * high / total:.0f} %")
    print(f"blocks with no adjacent non-zero pair            {100 * no_pair / n:.0f} %")


if __name__ == "__main__":
    main()
