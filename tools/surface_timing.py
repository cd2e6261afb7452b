#!/usr/bin/env python3
"""Surface encodes (m1v_set_input_layout) of this tree against what a caller of another build of the library (the parent
commit's, which has no input layout) does for the same frames, side by side in ONE process on one device, the way
tools/rgba_table_timing.py compares size tables.  Per leg and side: `--settle` untimed back-to-back calls, then `--launches`
timed ones with one synchronisation (wall time per call); sides and legs alternate for `--rounds` rounds and the median round is
printed with the ratio this / other.
    legs  plain packed C=3 / C=4            this tree's default kernels | the other library's          (no regression)
          B,G,R(,A) surface, pitch W*C+256  one surface step            | torch gather-and-swizzle copy into a packed
                                                                          buffer + the other library's plain step
          packed through k_encode_surface   pitch W*C set explicitly    | the other library's plain step (tiles / runs)
          table K=8, budget K=8             on the padded surface       | this tree on the packed frames
    usage: surface_timing.py --other <path to the other libencoder.so> [--w 1920 --h 1080 --n 300]
Every surface output (records, sizes, K = 8 table) is compared with the other library's output on the packed copy before
anything is timed."""
import argparse
import ctypes as C
import os
import statistics
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True)
ap.add_argument("--w", type=int, default=1920)
ap.add_argument("--h", type=int, default=1080)
ap.add_argument("--n", type=int, default=300)
ap.add_argument("--q", type=int, default=12)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--settle", type=int, default=60)
ap.add_argument("--launches", type=int, default=100)
a = ap.parse_args()
import torch

vp = C.c_void_p
K8 = (2, 3, 4, 6, 8, 9, 10, 12)
PAD = 256


def load(path):
    L = C.CDLL(path)
    L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_frame_size_table_device.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint8), C.c_int, vp, vp, vp]
    L.m1v_encode_budget_device.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_uint64, vp, vp, vp,
                                           C.c_size_t, vp, vp, vp, vp]
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_destroy.argtypes = [vp]
    L.m1v_path_in_use.argtypes = [vp]
    L.m1v_last_error.restype = C.c_char_p
    if hasattr(L, "m1v_set_input_layout"):
        L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    return L


def create(L, channels, layout=None):
    h = vp()
    assert L.m1v_create(C.byref(h), 0, a.w, a.h, channels, a.q, 1, a.n) == 0, L.m1v_last_error()
    if layout:
        assert L.m1v_set_input_layout(h, *layout) == 0, L.m1v_last_error()
    return h


this, other = load(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so")), load(a.other)
out = torch.empty(a.n * (a.w * a.h // 2 + 4096), dtype=torch.uint8, device="cuda")
sizes = torch.empty(a.n, dtype=torch.int64, device="cuda")
meta = torch.zeros(2, dtype=torch.int64, device="cuda")
table = torch.zeros(8 * a.n, dtype=torch.int64, device="cuda")
status = torch.zeros(8, dtype=torch.int32, device="cuda")
budget = int(0.75 * a.w * a.h * 3 // 54)
qs8 = (C.c_uint8 * 8)(*[min(x, a.q) for x in K8])


def plain(L, h, ptr):
    return lambda: L.m1v_encode_device(h, ptr, a.n, 0, out.data_ptr(), out.numel(), sizes.data_ptr(), meta.data_ptr(),
                                       meta.data_ptr() + 8, None)


def table8(L, h, ptr):
    return lambda: L.m1v_frame_size_table_device(h, ptr, a.n, qs8, 8, table.data_ptr(), status.data_ptr(), None)


def budget8(L, h, ptr):
    return lambda: L.m1v_encode_budget_device(h, ptr, a.n, 0, qs8, 8, budget, None, None, out.data_ptr(), out.numel(),
                                              sizes.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8, None)


def result(go, what):
    """The outputs of one call: (records, sizes) of an encode, or the K = 8 table."""
    out.zero_(), sizes.zero_(), meta.zero_(), table.zero_()
    assert go() == 0, what
    torch.cuda.synchronize()
    assert int(meta[1].item()) == 0 and int(status.abs().sum().item()) == 0, what
    return out[:int(meta[0].item())].clone(), sizes.clone(), table.clone()


legs = []          # (name, this side, other side)
handles, alive = [], []
for ch in (3, 4):
    rgb = torch.empty((a.n, a.h, a.w, ch), dtype=torch.uint8, device="cuda")
    this.m1v_synth_device(rgb.data_ptr(), a.w * a.h * ch, a.n, 504, 0, None)
    perm = torch.tensor([2, 1, 0] + ([3] if ch == 4 else []), device="cuda")
    pitch = a.w * ch + PAD
    buf = torch.randint(0, 256, (a.n * a.h * pitch,), dtype=torch.uint8, device="cuda")
    surface = torch.as_strided(buf, (a.n, a.h, a.w, ch), (a.h * pitch, pitch, ch, 1))      # B,G,R(,A), padded rows
    surface.copy_(rgb[..., perm])
    e_this, e_other = create(this, ch), create(other, ch)
    e_surf = create(this, ch, (pitch, 0, 1))
    e_packed = create(this, ch, (a.w * ch, 0, 0))
    handles += [(this, e_this), (other, e_other), (this, e_surf), (this, e_packed)]
    alive += [rgb, buf]                                     # (the legs hold raw pointers)
    assert this.m1v_path_in_use(e_surf) == 1 and this.m1v_path_in_use(e_packed) == 1
    plain_other = plain(other, e_other, rgb.data_ptr())

    def copy_then_plain(surface=surface, perm=perm, enc=e_other):
        packed = surface[..., perm].contiguous()           # what a caller does today: gather and swizzle into a packed buffer
        return other.m1v_encode_device(enc, packed.data_ptr(), a.n, 0, out.data_ptr(), out.numel(), sizes.data_ptr(),
                                       meta.data_ptr(), meta.data_ptr() + 8, None)   # (stream order keeps `packed` alive: one stream)

    # outputs first: every way to the records of these frames gives the other library's bytes
    want = result(plain_other, "other plain")
    for nm, go in (("this plain", plain(this, e_this, rgb.data_ptr())), ("surface", plain(this, e_surf, surface.data_ptr())),
                   ("packed through the surface kernels", plain(this, e_packed, rgb.data_ptr())), ("copy + other", copy_then_plain)):
        got = result(go, nm)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"C={ch}: {nm}: records differ"
    want_t = result(table8(other, e_other, rgb.data_ptr()), "other table")[2]
    for nm, go in (("surface table", table8(this, e_surf, surface.data_ptr())), ("this table", table8(this, e_this, rgb.data_ptr()))):
        assert torch.equal(result(go, nm)[2], want_t), f"C={ch}: {nm}: tables differ"
    kind = "tiles" if other.m1v_path_in_use(e_other) == 1 else "runs"
    legs += [
        (f"C={ch} plain packed (this | other)", plain(this, e_this, rgb.data_ptr()), plain_other),
        (f"C={ch} BG{'RA' if ch == 4 else 'R'} surface pitch W*{ch}+{PAD} (surface step | copy + other plain)",
         plain(this, e_surf, surface.data_ptr()), copy_then_plain),
        (f"C={ch} packed through k_encode_surface (| other plain, {kind})", plain(this, e_packed, rgb.data_ptr()), plain_other),
        (f"C={ch} table K=8 (surface | this packed)", table8(this, e_surf, surface.data_ptr()), table8(this, e_this, rgb.data_ptr())),
        (f"C={ch} budget K=8 (surface | this packed)", budget8(this, e_surf, surface.data_ptr()), budget8(this, e_this, rgb.data_ptr())),
    ]

res = {}
for r in range(a.rounds):
    for name, go_this, go_other in legs:
        for side, go in ((0, go_this), (1, go_other)) if r % 2 == 0 else ((1, go_other), (0, go_this)):
            for _ in range(a.settle):
                assert go() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                assert go() == 0
            torch.cuda.synchronize()
            res.setdefault((name, side), []).append((time.perf_counter() - t0) / a.launches)
print(f"{a.n} x {a.w}x{a.h} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); "
      "records, sizes and K = 8 tables equal on every path")
for name, _, _ in legs:
    t, o = (statistics.median(res[(name, side)]) * 1e6 for side in (0, 1))
    print(f"{name}\n    left {t:8.1f}  right {o:8.1f}  left/right {t / o:6.3f}   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 0)]) + " | " + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 1)]))
for L, h in handles:
    L.m1v_destroy(h)
