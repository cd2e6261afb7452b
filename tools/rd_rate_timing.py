#!/usr/bin/env python3
"""What the batch and bitrate picks by distortion cost: m1v_encode_rd_batch_device (both rules) and m1v_encode_rd_cbr_device
beside m1v_encode_rd_device of the SAME build, in one process, on the same frames and candidates.  The four calls share the rd
table and the encode and differ only in the pick between them.  Per leg: the whole call as the device sees it (`--calls` calls
queued back to back between two events, per call) and the two profiled kernels (m1v_profile_read_times: the table pass and the
encode).  The legs alternate for `--rounds` rounds, the order reversed every other round.  Then the two pick-only calls
(m1v_rd_batch_pick_device, m1v_rd_cbr_pick_device) on the table of the same frames, timed the same way: their own time per call,
beside k_rate_pick's 17.4 us (batch) and 28.1 us (bitrate) of profiles/r07_rate_timing.txt.  K = 8 and K = 2.
    usage: rd_rate_timing.py [--w 1920 --h 1080 --n 300] [--q 12] [--out profiles/r15_rd_rate_timing.txt]
Target: each new encode call <= 1.05 x m1v_encode_rd_device at K = 8.  The limits are taken from the table itself (the middle
candidate's totals), so that the picks are mixed."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE8 = (2, 3, 4, 6, 8, 9, 10, 12)      # the K = 8 table of tools/rgba_table_timing.py


def qualities(q, k):
    """k strictly increasing qualities up to q: TABLE8 scaled to the encoder's quality factor (k = 2: its ends' neighbours)."""
    qs = sorted({max(1, x * q // 12) for x in TABLE8})
    return tuple(qs) if k >= len(qs) else tuple(qs[i * (len(qs) - 1) // (k - 1)] for i in range(k)) if k > 1 else (qs[-1],)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--q", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pick-calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    assert torch.cuda.is_available(), "rd_rate_timing.py measures on the GPU: there is no fallback"

    n = a.n
    enc = Mpeg1Encoder(a.w, a.h, a.q, "full", max_frames=n)
    assert enc.size_table_fused == 1
    rgb = enc.synth(n, seed=504)
    L = _ffi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    chosen = torch.zeros(n, dtype=torch.uint8, device="cuda")
    fdist = torch.zeros(n, dtype=torch.int64, device="cuda")
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")
    total, status = p(meta), C.c_void_p(meta.data_ptr() + 8)
    lin = torch.zeros(1, dtype=torch.int64, device="cuda")
    lout = torch.zeros(1, dtype=torch.int64, device="cuda")
    picks = torch.zeros(n, dtype=torch.uint8, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    lines = [f"{n} x {a.w}x{a.h}x3, encoder quality {a.q}, device: {torch.cuda.get_device_name(0)}",
             f"per leg and round: {a.settle} settle calls, then {a.calls} calls between two events (call = device time per call, ms) "
             f"and {a.calls} profiled calls (table, encode = median kernel time, ms); {a.rounds} rounds, legs alternating"]

    def timed(go, calls):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            assert go() == 0, _ffi.last_error()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / calls

    for K in (8, 2):
        quals = qualities(a.q, K)
        K = len(quals)
        cand = (C.c_uint8 * K)(*quals)
        s_t, d_t = enc.frame_rd_table(rgb, quals)
        torch.cuda.synchronize()
        mid = K // 2
        budget, ceiling = int(s_t[mid].sum().item()), int(d_t[mid].sum().item())
        rate = max(1, budget // n)
        lin.fill_(2 * rate)
        per_frame = max(1, budget // n)
        legs = {
            "rd per frame": lambda: L.m1v_encode_rd_device(enc._h, p(rgb), n, 0, cand, K, 0, per_frame, None, p(chosen), p(out), out.numel(),
                                                           p(sizes), p(fdist), total, status, None),
            "rd batch bytes": lambda: L.m1v_encode_rd_batch_device(enc._h, p(rgb), n, 0, cand, K, 0, budget, p(chosen), p(out), out.numel(),
                                                                   p(sizes), p(fdist), total, status, None),
            "rd batch dist": lambda: L.m1v_encode_rd_batch_device(enc._h, p(rgb), n, 0, cand, K, 1, ceiling, p(chosen), p(out), out.numel(),
                                                                  p(sizes), p(fdist), total, status, None),
            "rd bitrate": lambda: L.m1v_encode_rd_cbr_device(enc._h, p(rgb), n, 0, cand, K, rate, 2 * rate, p(lin), p(lout), p(chosen), p(out),
                                                             out.numel(), p(sizes), p(fdist), total, status, None),
        }
        names = list(legs)
        call_ms = {leg: [] for leg in legs}
        kern_ms = {leg: ([], []) for leg in legs}
        mixed = {}
        for r in range(a.rounds):
            for leg in (names if r % 2 == 0 else names[::-1]):
                go = legs[leg]
                for _ in range(a.settle):
                    assert go() == 0, _ffi.last_error()
                call_ms[leg].append(timed(go, a.calls))
                assert int(meta[1].item()) & 0xFFFFFFCF == 0, (leg, int(meta[1].item()))   # (the over-limit bits may be set)
                mixed[leg] = len(set(chosen.cpu().tolist()))
                enc.profile(True)
                for _ in range(a.calls):
                    assert go() == 0, _ffi.last_error()
                torch.cuda.synchronize()
                ms = enc.profile_read_times(cap=2 * a.calls)
                enc.profile(False)
                assert len(ms) == 2 * a.calls, (leg, len(ms))
                kern_ms[leg][0].extend(ms[0::2])
                kern_ms[leg][1].extend(ms[1::2])
        lines.append(f"## K = {K}, candidates {quals}; batch budget {budget} bytes, ceiling {ceiling}, {rate} bytes per frame into {2 * rate}")
        base = statistics.median(call_ms["rd per frame"])
        for leg in names:
            med = statistics.median(call_ms[leg])
            lines.append(f"{leg:15s} call {med:8.4f} ms  ratio to rd per frame {med / base:.4f}   table {statistics.median(kern_ms[leg][0]):8.4f}"
                         f"  encode {statistics.median(kern_ms[leg][1]):8.4f}   qualities picked: {mixed[leg]}   per round: "
                         + " ".join(f"{x:.4f}" for x in call_ms[leg]))
        s_c, d_c = s_t.contiguous(), d_t.contiguous()
        pick_legs = {
            "batch pick bytes": lambda: L.m1v_rd_batch_pick_device(enc._h, p(s_c), p(d_c), None, n, K, 0, budget, p(picks), p(fdist), p(word), None),
            "batch pick dist": lambda: L.m1v_rd_batch_pick_device(enc._h, p(s_c), p(d_c), None, n, K, 1, ceiling, p(picks), p(fdist), p(word), None),
            "bitrate pick": lambda: L.m1v_rd_cbr_pick_device(enc._h, p(s_c), p(d_c), None, n, K, rate, 2 * rate, p(lin), p(lout), p(picks),
                                                             p(fdist), p(word), None),
        }
        for leg, go in pick_legs.items():
            timed(go, 20)
            us = [1000.0 * timed(go, a.pick_calls) for _ in range(a.rounds)]
            lines.append(f"{leg:17s} {statistics.median(us):8.2f} us per call ({a.pick_calls} calls back to back, launches included)   per round: "
                         + " ".join(f"{x:.2f}" for x in us))
    enc.close()
    lines.append("k_rate_pick (profiles/r07_rate_timing.txt, kernel alone, n = 300, K = 8): batch form 17.4 us, bitrate form 28.1 us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
