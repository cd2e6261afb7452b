#!/usr/bin/env python3
"""What a byte budget per stream costs and what it saves (include/mpeg1_hip.h "Streams: a budget per stream"), side by side in
ONE process on one device, by the protocol of tools/streams_timing.py.  Per leg and side: `--settle` untimed back-to-back calls,
then `--launches` timed ones with one synchronisation (wall time per call); the sides alternate over `--rounds` rounds and the
median round is printed with the ratio left / right and the range of that ratio over the rounds.
      A/A        m1v_encode_streams_budget_device | the same call again          (the spread one call against itself shows here)
      per rule (largest that fits, least distortion), `--streams` streams of n / streams frames each, K = `--k` candidates:
      (a) calls  one m1v_encode_streams_budget_device | one existing batch call per stream on its slice, one after the other
                 (m1v_encode_batch_budget_device, m1v_encode_rd_batch_device: what a caller does without this call)
      (b) limit  one m1v_encode_streams_budget_device | ONE existing batch call over all n frames with a single limit
                 (what it costs to have `--streams` limits instead of one)
    usage: streams_budget_timing.py [--w 1920 --h 1080 --n 300] [--streams 30] [--k 8]
The plain step against the parent commit is bench.py's to measure on the two checkouts.  Before anything is timed the records,
sizes and picks of the new call are compared with those of the per-stream calls."""
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
ap.add_argument("--streams", type=int, default=30)
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--settle", type=int, default=5)
ap.add_argument("--launches", type=int, default=10)
a = ap.parse_args()
import torch

from ec504_imageencoder_amd import _ffi

L = _ffi.lib()
vp = C.c_void_p
W, H, N, S, K = a.w, a.h, a.n, a.streams, a.k
assert N % S == 0 and 1 <= K <= min(8, a.q)
PER = N // S
h = vp()
assert L.m1v_create(C.byref(h), 0, W, H, 3, a.q, 1, N) == 0, _ffi.last_error()
assert L.m1v_size_table_fused(h) == 1

rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(rgb.data_ptr(), W * H * 3, N, 504, 0, None)
FRAME_IN, SLOT = W * H * 3, W * H // 2 + 4096          # bytes of a frame, and of d_out per frame
outs = [torch.empty(N * SLOT, dtype=torch.uint8, device="cuda") for _ in range(2)]
sizes = [torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(2)]
chosen = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(2)]
dist = [torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(2)]
meta = torch.zeros(2 * S + 2, dtype=torch.int64, device="cuda")      # (total, status) of every call of a side
stream_bytes = torch.zeros(S, dtype=torch.int64, device="cuda")
stream_status = torch.zeros(S, dtype=torch.int32, device="cuda")
spans = torch.tensor([[s * PER, PER, 1000 * s, 0] for s in range(S)], dtype=torch.int32, device="cuda")
cands = (C.c_uint8 * K)(*range(a.q - K + 1, a.q + 1))
OVER = _ffi.STATUS_OVER_BUDGET


def ran(go, what, allowed=0):
    """One call of `go`, waited for; its status words may hold the bits of `allowed` only (the timed steps are whole encodes)."""
    meta.zero_()
    assert go() == 0, (what, _ffi.last_error())
    torch.cuda.synchronize()
    assert all(int(x) & ~allowed == 0 for x in meta[1::2].cpu()), f"{what}: status {meta[1::2].cpu().tolist()}"


# the limits: four fifths of what each stream's frames take at the largest candidate, so that the picks are mixed
table = torch.zeros((K, N), dtype=torch.int64, device="cuda")
assert L.m1v_frame_size_table_device(h, rgb.data_ptr(), N, cands, K, table.data_ptr(), None, None) == 0, _ffi.last_error()
torch.cuda.synchronize()
top = table[K - 1].cpu().tolist()
limits_l = [sum(top[s * PER:(s + 1) * PER]) * 4 // 5 for s in range(S)]
limits = torch.tensor(limits_l, dtype=torch.int64, device="cuda")
ONE_LIMIT = sum(limits_l)


def streams_call(rule, side=0):
    return lambda: L.m1v_encode_streams_budget_device(
        h, rgb.data_ptr(), N, spans.data_ptr(), S, cands, K, rule, 0, limits.data_ptr(), chosen[side].data_ptr(), outs[side].data_ptr(),
        outs[side].numel(), sizes[side].data_ptr(), dist[side].data_ptr() if rule else None, stream_bytes.data_ptr(),
        stream_status.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8, None)


def single_call(rule, first, count, index, s, limit):
    """The existing batch call of the rule on frames [first, first + count), into its own part of the second side's buffers."""
    head = [h, rgb.data_ptr() + first * FRAME_IN, count, index, cands, K]
    out = [chosen[1].data_ptr() + first, outs[1].data_ptr() + first * SLOT, count * SLOT, sizes[1].data_ptr() + 8 * first]
    tail = [meta.data_ptr() + 16 * (s + 1), meta.data_ptr() + 16 * (s + 1) + 8, None]
    if rule:
        return L.m1v_encode_rd_batch_device(*head, _ffi.RD_BEST_IN_BUDGET, limit, *out, dist[1].data_ptr() + 8 * first, *tail)
    return L.m1v_encode_batch_budget_device(*head, limit, *out, *tail)


def per_stream_calls(rule):
    def go():
        for s in range(S):
            rc = single_call(rule, s * PER, PER, 1000 * s, s, limits_l[s])
            if rc:
                return rc
        return 0
    return go


def one_limit(rule):
    return lambda: single_call(rule, 0, N, 0, 0, ONE_LIMIT)


RULES = ((_ffi.SPANS_LARGEST_THAT_FITS, "largest that fits"), (_ffi.SPANS_LEAST_DISTORTION, "least distortion"))
legs = [("A/A (m1v_encode_streams_budget_device, least distortion | the same call)", streams_call(_ffi.SPANS_LEAST_DISTORTION, 0),
         streams_call(_ffi.SPANS_LEAST_DISTORTION, 1))]
for rule, name in RULES:
    ran(streams_call(rule), name + ", streams", OVER)
    ran(per_stream_calls(rule), name + ", per stream", OVER)
    at = 0
    for s in range(S):                                   # the new call's contiguous ranges against each call's own output
        nb = int(stream_bytes[s].item())
        assert nb == int(meta[2 * (s + 1)].item()), f"{name}: stream {s} bytes"
        assert torch.equal(outs[0][at:at + nb], outs[1][s * PER * SLOT:s * PER * SLOT + nb]), f"{name}: stream {s} records"
        at += nb
    assert torch.equal(sizes[0], sizes[1]) and torch.equal(chosen[0], chosen[1]), f"{name}: sizes or picks"
    print(f"{name}: frames per picked quality {sorted((q, chosen[0].cpu().tolist().count(q)) for q in set(chosen[0].cpu().tolist()))}", flush=True)
    legs += [(f"(a) calls, {name}: one new call, {S} x {PER} frames, K = {K} | {S} existing batch calls on the slices",
              streams_call(rule), per_stream_calls(rule)),
             (f"(b) limit, {name}: one new call with {S} limits | one existing batch call over {N} frames with one limit",
              streams_call(rule), one_limit(rule))]

res = {}
for r in range(a.rounds):
    for leg, go_left, go_right in legs:
        for side, go in ((0, go_left), (1, go_right)) if r % 2 == 0 else ((1, go_right), (0, go_left)):
            for _ in range(a.settle):
                assert go() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                assert go() == 0
            torch.cuda.synchronize()
            res.setdefault((leg, side), []).append((time.perf_counter() - t0) / a.launches)
print(f"{N} x {W}x{H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); limits: four fifths of "
      f"each stream's bytes at the largest candidate; records, sizes and picks of the new call equal to the per-stream calls'; device: "
      + torch.cuda.get_device_name(0), flush=True)
for leg, _, _ in legs:
    t, o = (statistics.median(res[(leg, side)]) * 1e6 for side in (0, 1))
    ratios = [p / q for p, q in zip(res[(leg, 0)], res[(leg, 1)])]
    print(f"{leg}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
          + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 0)]) + " | " + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 1)]), flush=True)
L.m1v_destroy(h)
