#!/usr/bin/env python3
"""What the distortion costs: the rd-table pass (m1v_frame_rd_table_device, the k_rd_table_* kernels) beside the fused size-table
pass (m1v_frame_size_table_device) of the SAME build, in one process, on the same frames and qualities.  The times are those of
the dominant kernel alone, from the library's own events (m1v_profile_read_times: one duration per pass).  Per leg `--settle`
unprofiled back-to-back calls, then `--launches` profiled ones; the legs alternate for `--rounds` rounds, the order reversed
every other round.  Prints, and writes to --out, the median kernel time of each leg over all its profiled launches, the
per-round medians (the spread) and the ratio rd table / size table.
    usage: rd_table_timing.py [--channels 3] [--w 1920 --h 1080 --n 300] [--q 12] [--out profiles/r12_rd_table_timing.txt]
Before anything is timed the sizes of the two calls are compared, and frame 0's distortion row is printed.
Measured cost (profiles/r12_rd_table_timing.txt): not measured yet."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE8 = (2, 3, 4, 6, 8, 9, 10, 12)      # the K = 8 table of tools/rgba_table_timing.py


def qualities(q):
    """Eight strictly increasing qualities up to q: TABLE8 scaled to the encoder's quality factor."""
    qs = sorted({max(1, x * q // 12) for x in TABLE8})
    return tuple(qs)


def summary(times):
    """(median over every launch, [median of each round]) of {round: [ms]}."""
    return statistics.median([t for r in times for t in r]), [statistics.median(r) for r in times]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--q", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    assert torch.cuda.is_available(), "rd_table_timing.py measures on the GPU: there is no fallback"

    enc = Mpeg1Encoder(a.w, a.h, a.q, "full", channels=a.channels, max_frames=a.n)
    assert enc.size_table_fused == 1
    rgb = enc.synth(a.n, seed=504)
    quals = qualities(a.q)
    K = len(quals)
    qbuf = (C.c_uint8 * K)(*quals)
    sizes = torch.zeros(K * a.n, dtype=torch.int64, device="cuda")
    sizes_rd = torch.zeros(K * a.n, dtype=torch.int64, device="cuda")
    dist = torch.zeros(K * a.n, dtype=torch.int64, device="cuda")
    status = torch.zeros(K, dtype=torch.int32, device="cuda")
    L = _ffi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    legs = {
        "size table": lambda: L.m1v_frame_size_table_device(enc._h, p(rgb), a.n, qbuf, K, p(sizes), p(status), None),
        "rd table": lambda: L.m1v_frame_rd_table_device(enc._h, p(rgb), a.n, qbuf, K, p(sizes_rd), p(dist), p(status), None),
    }
    for go in legs.values():
        assert go() == 0, _ffi.last_error()
    torch.cuda.synchronize()
    assert torch.equal(sizes, sizes_rd), "the rd table's sizes differ from the size table's"
    assert int(status.abs().sum().item()) == 0
    d0 = [int(x) for x in dist.view(K, a.n)[:, 0].cpu()]

    times = {leg: [] for leg in legs}
    names = list(legs)
    for r in range(a.rounds):
        for leg in (names if r % 2 == 0 else names[::-1]):
            go = legs[leg]
            for _ in range(a.settle):
                assert go() == 0, _ffi.last_error()
            torch.cuda.synchronize()
            enc.profile(True)
            for _ in range(a.launches):
                assert go() == 0, _ffi.last_error()
            torch.cuda.synchronize()
            ms = enc.profile_read_times(cap=a.launches)
            enc.profile(False)
            assert len(ms) == a.launches, (leg, len(ms))
            times[leg].append(ms)
    enc.close()

    lines = [f"{a.n} x {a.w}x{a.h}x{a.channels}, encoder quality {a.q}, K = {K} qualities {quals}: kernel time per pass in ms "
             f"(m1v_profile_read_times), {a.rounds} rounds of {a.settle} settle + {a.launches} profiled launches per leg, legs alternating",
             f"device: {torch.cuda.get_device_name(0)}; sizes of the two calls equal; distortion of frame 0 per quality: {d0}"]
    med = {}
    for leg in names:
        med[leg], rounds = summary(times[leg])
        lines.append(f"{leg:10s} median {med[leg]:8.4f} ms   per round: " + " ".join(f"{x:.4f}" for x in rounds))
    lines.append(f"ratio rd table / size table = {med['rd table'] / med['size table']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
