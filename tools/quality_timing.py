#!/usr/bin/env python3
"""Step times of the per-frame quality entry points against the plain call, on one device (include/mpeg1_hip.h):

    plain       m1v_encode_device
    quality     m1v_encode_quality_device, every frame at the encoder's quality (one selection launch + one scalar load
                per workgroup more than plain)
    probe       m1v_frame_sizes_device (the encode kernel + k_frame_sizes instead of k_assemble)
    budget K    m1v_encode_budget_device with K candidates (tiles: one size-table pass + the pick + one encode; runs: K probes
                + the pick + one encode)
    batch K     m1v_encode_batch_budget_device with K candidates and a budget of n frames at that size (the size table of
                budget K + k_rate_pick, one workgroup + one encode)
    cbr K       m1v_encode_cbr_device with K candidates, that size per frame into a buffer of two frames (separate level
                pointers: every call starts from the same level)
    table K     m1v_frame_size_table_device with K qualities (one fused pass, k_size_table_tiles or, with --channels 4,
                k_size_table_rgba, + k_size_table_sizes; an encoder forced by --path runs: K probes)

Each leg: `--settle` untimed calls, then `--launches` timed back-to-back calls with one synchronisation (wall time per call),
legs alternating for `--rounds` rounds; the median round is printed.  `kernel` is the median duration of the encode kernel
(HIP events around it, a separate pass; a size-table pass counts as one launch), so a budget call can be set against (K + 1) x
the plain encode kernel, and a size table against K x.
    usage: quality_timing.py [--w 1920 --h 1080 --n 300] [--channels 3|4] [--path tiles|runs] [--only plain,table,budget]
A/B of the table and budget calls against another build of the library in one process: tools/rgba_table_timing.py."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=1920)
ap.add_argument("--h", type=int, default=1080)
ap.add_argument("--n", type=int, default=300)
ap.add_argument("--q", type=int, default=12)
ap.add_argument("--path", default="")
ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--only", default="", help="comma-separated leg name prefixes (plain is always timed)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--settle", type=int, default=100)
ap.add_argument("--launches", type=int, default=200)
a = ap.parse_args()
import torch
from ec504_imageencoder_amd import Mpeg1Encoder, _ffi

enc = Mpeg1Encoder(a.w, a.h, a.q, "full", channels=a.channels, max_frames=a.n)
if a.path:
    enc.debug_set_path(a.path)
L, h = _ffi.lib(), enc._h
rgb = enc.synth(a.n)
out = torch.empty(enc.default_out_capacity(a.n), dtype=torch.uint8, device="cuda")
sizes = torch.empty(a.n, dtype=torch.int64, device="cuda")
meta = torch.zeros(2, dtype=torch.int64, device="cuda")
qual = torch.full((a.n,), a.q, dtype=torch.uint8, device="cuda")
vp = C.c_void_p
R, O, S, T, ST, Q = (vp(x) for x in (rgb.data_ptr(), out.data_ptr(), sizes.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8,
                                     qual.data_ptr()))
CANDS = {2: (6, 12), 4: (3, 6, 9, 12), 8: (2, 3, 4, 6, 8, 9, 10, 12)}
table_sizes = torch.empty(8 * a.n, dtype=torch.int64, device="cuda")
table_status = torch.zeros(8, dtype=torch.int32, device="cuda")
TS, TST = vp(table_sizes.data_ptr()), vp(table_status.data_ptr())
TABLES = {1: (a.q,), 2: CANDS[2], 4: CANDS[4], 8: CANDS[8]}
budget = int(0.75 * a.w * a.h * 3 // 54)   # ~ the record of a noise frame at quality 8-9 (1080p: 114.5 KB at 12)
level_in = torch.full((1,), 2 * budget, dtype=torch.int64, device="cuda")
level_out = torch.zeros(1, dtype=torch.int64, device="cuda")
LI, LO = vp(level_in.data_ptr()), vp(level_out.data_ptr())


def legs():
    only = tuple(x for x in a.only.split(",") if x)
    for leg in all_legs():
        if not only or leg[0] == "plain" or leg[0].startswith(only):
            yield leg


def all_legs():
    yield "plain", lambda: L.m1v_encode_device(h, R, a.n, 0, O, out.numel(), S, T, ST, None), 1
    yield "quality", lambda: L.m1v_encode_quality_device(h, R, a.n, 0, Q, O, out.numel(), S, T, ST, None), 1
    yield "probe", lambda: L.m1v_frame_sizes_device(h, R, a.n, None, S, ST, None), 1
    for k, c in CANDS.items():
        cand = (C.c_uint8 * k)(*[min(x, a.q) for x in c])
        yield f"budget K={k}", (lambda cand=cand, k=k: L.m1v_encode_budget_device(h, R, a.n, 0, cand, k, budget, None, None, O,
                                                                                  out.numel(), S, T, ST, None)), k + 1
        yield f"batch K={k}", (lambda cand=cand, k=k: L.m1v_encode_batch_budget_device(h, R, a.n, 0, cand, k, budget * a.n, None, O,
                                                                                       out.numel(), S, T, ST, None)), k + 1
        yield f"cbr K={k}", (lambda cand=cand, k=k: L.m1v_encode_cbr_device(h, R, a.n, 0, cand, k, budget, 2 * budget, LI, LO, None,
                                                                            O, out.numel(), S, T, ST, None)), k + 1
    for k, c in TABLES.items():
        qs = (C.c_uint8 * k)(*[min(x, a.q) for x in c])
        yield f"table K={k}", (lambda qs=qs, k=k: L.m1v_frame_size_table_device(h, R, a.n, qs, k, TS, TST, None)), k


res = {}
for r in range(a.rounds):
    for name, go, _ in legs():
        for _ in range(a.settle):
            assert go() == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.launches):
            assert go() == 0
        torch.cuda.synchronize()
        res.setdefault(name, []).append((time.perf_counter() - t0) / a.launches)
        assert int(meta[1].item()) & ~_ffi.STATUS_OVER_BUDGET == 0, (name, int(meta[1].item()))
        assert int(table_status.abs().sum().item()) == 0, name
kern = {}
for name, go, per_call in legs():
    enc.profile(True)
    enc.profile_read_times()
    for _ in range(50):
        assert go() == 0
    torch.cuda.synchronize()
    t = enc.profile_read_times()
    enc.profile(False)
    kern[name] = statistics.median(t) * 1e3, len(t) // 50
plain_k = kern["plain"][0]
print(f"{a.n} x {a.w}x{a.h}x{a.channels} q{a.q} path={enc.path} size_table_fused={enc.size_table_fused}  budget={budget} B/frame")
for name, go, per_call in legs():
    step = statistics.median(res[name]) * 1e6
    k_us, launches = kern[name]
    print(f"{name:13s} step {step:8.1f} us  x{step / (statistics.median(res['plain']) * 1e6):5.2f} of plain  "
          f"encode kernel {k_us:7.1f} us x {launches} (x{k_us / plain_k:4.2f})  K(+1) x plain kernel = {per_call * plain_k:8.1f} us   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[name]))
enc.close()
