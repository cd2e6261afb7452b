#!/usr/bin/env python3
"""Size-table and budget calls of two builds of the library side by side in ONE process on one device: this tree's
libencoder.so and another build's (the parent commit's), the way tools/sustained.py compares plain steps.  Per library and
leg: `--settle` untimed back-to-back calls, then `--launches` timed ones with one synchronisation (wall time per call);
libraries and legs alternate for `--rounds` rounds and the median round is printed, with the ratio to the other library.
    legs: plain (m1v_encode_device), table K = 1 / 2 / 4 / 8 (m1v_frame_size_table_device), budget K = 8
    usage: rgba_table_timing.py --other <path to the other libencoder.so> [--channels 4] [--w 1920 --h 1080 --n 300]
The K = 8 tables of the two libraries are compared before anything is timed."""
import argparse
import ctypes as C
import os
import statistics
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True)
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--w", type=int, default=1920)
ap.add_argument("--h", type=int, default=1080)
ap.add_argument("--n", type=int, default=300)
ap.add_argument("--q", type=int, default=12)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--settle", type=int, default=60)
ap.add_argument("--launches", type=int, default=100)
a = ap.parse_args()
import torch

vp = C.c_void_p
TABLES = {1: (a.q,), 2: (6, 12), 4: (3, 6, 9, 12), 8: (2, 3, 4, 6, 8, 9, 10, 12)}


def load(path):
    L = C.CDLL(path)
    L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_frame_size_table_device.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint8), C.c_int, vp, vp, vp]
    L.m1v_encode_budget_device.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_uint64, vp, vp, vp,
                                           C.c_size_t, vp, vp, vp, vp]
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_destroy.argtypes = [vp]
    L.m1v_last_error.restype = C.c_char_p
    h = vp()
    assert L.m1v_create(C.byref(h), 0, a.w, a.h, a.channels, a.q, 1, a.n) == 0, L.m1v_last_error()
    return L, h


libs = {"this tree": load(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so")), "other": load(a.other)}
rgb = torch.empty((a.n, a.h, a.w, a.channels), dtype=torch.uint8, device="cuda")
libs["this tree"][0].m1v_synth_device(rgb.data_ptr(), a.w * a.h * a.channels, a.n, 504, 0, None)
out = torch.empty(a.n * (a.w * a.h // 2 + 4096), dtype=torch.uint8, device="cuda")
sizes = torch.empty(a.n, dtype=torch.int64, device="cuda")
meta = torch.zeros(2, dtype=torch.int64, device="cuda")
table = torch.zeros(8 * a.n, dtype=torch.int64, device="cuda")
status = torch.zeros(8, dtype=torch.int32, device="cuda")
budget = int(0.75 * a.w * a.h * 3 // 54)


def legs(L, h):
    yield "plain", lambda: L.m1v_encode_device(h, rgb.data_ptr(), a.n, 0, out.data_ptr(), out.numel(), sizes.data_ptr(),
                                               meta.data_ptr(), meta.data_ptr() + 8, None)
    for k, c in TABLES.items():
        qs = (C.c_uint8 * k)(*[min(x, a.q) for x in c])
        yield f"table K={k}", (lambda qs=qs, k=k: L.m1v_frame_size_table_device(h, rgb.data_ptr(), a.n, qs, k, table.data_ptr(),
                                                                                status.data_ptr(), None))
    qs8 = (C.c_uint8 * 8)(*[min(x, a.q) for x in TABLES[8]])
    yield "budget K=8", lambda: L.m1v_encode_budget_device(h, rgb.data_ptr(), a.n, 0, qs8, 8, budget, None, None, out.data_ptr(),
                                                           out.numel(), sizes.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8, None)


# the two libraries agree on the K = 8 table of these frames
seen = []
for nm, (L, h) in libs.items():
    go = dict(legs(L, h))["table K=8"]
    table.zero_()
    assert go() == 0, L.m1v_last_error()
    torch.cuda.synchronize()
    seen.append(table.clone())
    assert int(status.abs().sum().item()) == 0
assert torch.equal(seen[0], seen[1]), "the two libraries' tables differ"

res = {}
names = list(libs)
for r in range(a.rounds):
    for nm in (names if r % 2 == 0 else names[::-1]):
        L, h = libs[nm]
        for leg, go in legs(L, h):
            for _ in range(a.settle):
                assert go() == 0, L.m1v_last_error()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                assert go() == 0, L.m1v_last_error()
            torch.cuda.synchronize()
            res.setdefault((nm, leg), []).append((time.perf_counter() - t0) / a.launches)
print(f"{a.n} x {a.w}x{a.h}x{a.channels} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); tables equal")
for leg, _ in legs(*libs["this tree"]):
    t, o = (statistics.median(res[(nm, leg)]) * 1e6 for nm in names)
    print(f"{leg:11s} this tree {t:8.1f}  other {o:8.1f}  this/other {t / o:6.3f}   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[("this tree", leg)]) + " | " + " ".join(f"{x * 1e6:.1f}" for x in res[("other", leg)]))
for L, h in libs.values():
    L.m1v_destroy(h)
