#!/usr/bin/env python3
"""What encoding float planes in place (m1v_set_float_plane_layout) costs and what it saves, side by side in ONE process on one
device, in the mould of tools/plane_table_timing.py.  Per leg and side: `--settle` untimed back-to-back calls, then `--launches`
timed ones with one synchronisation (wall time per call); the sides alternate over `--rounds` rounds and the median round is
printed with the ratio left / right and the range of that ratio over the rounds.
    per sample type (float16, bfloat16, float32), left = the encode step on the float tensor [n, 3, H, W]:
      A/A       | the same call again                                           (the spread one call against itself shows here)
      (a) bytes | the uint8 RGB plane step on bytes converted beforehand        (the parent's kernels: what the wider samples cost)
      (b) eager | x.mul(255).round().clamp(0, 255).to(torch.uint8), then (a)    (what callers do today)
      (c) two   | m1v_float_planes_to_bytes_device, then (a)                    (the best two-pass form)
    usage: float_planes_timing.py [--w 1920 --h 1080 --n 300] [--only <text>[,<text>]]
The records and sizes of (a) and (c) are compared with the float step's before anything is timed; for (b) the count of bytes in
which torch's expression (evaluated in the tensor's own type) differs from the rule is printed."""
import argparse
import ctypes as C
import os
import statistics
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=1920)
ap.add_argument("--h", type=int, default=1080)
ap.add_argument("--n", type=int, default=300)
ap.add_argument("--q", type=int, default=12)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--settle", type=int, default=10)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--only", default="")
a = ap.parse_args()
import torch

vp = C.c_void_p
W, H, N = a.w, a.h, a.n
assert W % 2 == 0
LUMA = W * H


class RgbPlaneLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")]


class FloatPlaneLayout(C.Structure):
    _fields_ = RgbPlaneLayout._fields_ + [("sample", C.c_int32), ("range", C.c_int32)]


L = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
L.m1v_set_rgb_plane_layout.argtypes = [vp, C.POINTER(RgbPlaneLayout)]
L.m1v_set_float_plane_layout.argtypes = [vp, C.POINTER(FloatPlaneLayout)]
L.m1v_float_planes_to_bytes_device.argtypes = [vp, vp, C.c_int, vp, vp]
L.m1v_destroy.argtypes = [vp]
L.m1v_last_error.restype = C.c_char_p
handles = []


def create(layout):
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, 3, a.q, 1, N) == 0, L.m1v_last_error()
    setter = L.m1v_set_float_plane_layout if isinstance(layout, FloatPlaneLayout) else L.m1v_set_rgb_plane_layout
    assert setter(h, C.byref(layout)) == 0, L.m1v_last_error()
    handles.append(h)
    return h


out = torch.empty(N * (W * H // 2 + 4096), dtype=torch.uint8, device="cuda")
sizes = torch.empty(N, dtype=torch.int64, device="cuda")
meta = torch.zeros(2, dtype=torch.int64, device="cuda")


def step(h, ptr):
    return lambda: L.m1v_encode_device(h, ptr, N, 0, out.data_ptr(), out.numel(), sizes.data_ptr(), meta.data_ptr(),
                                       meta.data_ptr() + 8, None)


def result(go, what):
    out.zero_(), sizes.zero_(), meta.zero_()
    assert go() == 0, what
    torch.cuda.synchronize()
    assert int(meta[1].item()) == 0, f"{what}: status {int(meta[1].item())}"   # (the timed steps must be whole encodes)
    return out[:int(meta[0].item())].clone(), sizes.clone()


def same(got, want, what):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{what}: records differ"


# ---- the pictures: synthetic bytes as planes, and each type's samples byte / 255 rounded to the type ----
rgb = torch.empty((N, 3, H, W), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(rgb.data_ptr(), LUMA * 3, N, 504, 0, None)
torch.cuda.synchronize()
staged = torch.empty_like(rgb)         # where the two-pass forms put their bytes
e_bytes = create(RgbPlaneLayout(0, LUMA, 2 * LUMA, W, 3 * LUMA))
legs, keep, notes = [], [], []
for code, dtype in enumerate((torch.float16, torch.bfloat16, torch.float32)):
    name = str(dtype).rsplit(".", 1)[-1]
    if a.only and not any(text in name for text in a.only.split(",")):
        continue
    S = 2 if code < 2 else 4
    x = torch.empty((N, 3, H, W), dtype=dtype, device="cuda")
    for f in range(0, N, 10):            # in pieces: no float32 temporary of the batch's size
        x[f:f + 10] = (rgb[f:f + 10].float() / 255.0).to(dtype)
    e_float = create(FloatPlaneLayout(0, LUMA * S, 2 * LUMA * S, W * S, 3 * LUMA * S, code, 0))
    float_step = step(e_float, x.data_ptr())
    staged_step = step(e_bytes, staged.data_ptr())

    def eager_then_bytes(x=x):           # (the expression's result encoded where torch put it: no copy into `staged`)
        y = x.mul(255).round().clamp(0, 255).to(torch.uint8)
        return step(e_bytes, y.data_ptr())()

    def kernel_then_bytes(x=x, staged_step=staged_step, e_float=e_float):   # (bound now: the loop goes on to the next type's encoder)
        rc = L.m1v_float_planes_to_bytes_device(e_float, x.data_ptr(), N, staged.data_ptr(), None)
        return rc or staged_step()

    want = result(float_step, name)
    assert L.m1v_float_planes_to_bytes_device(e_float, x.data_ptr(), N, staged.data_ptr(), None) == 0
    torch.cuda.synchronize()
    converted = staged.clone()           # the bytes converted beforehand
    same(result(step(e_bytes, converted.data_ptr()), name + " bytes"), want, name + ": uint8 planes of the rule's bytes")
    same(result(kernel_then_bytes, name + " two-pass"), want, name + ": bytes kernel + uint8 step")
    differ = 0
    for f in range(0, N, 10):
        differ += int((x[f:f + 10].mul(255).round().clamp(0, 255).to(torch.uint8) != converted[f:f + 10]).sum().item())
    notes.append(f"{name}: torch's expression in {name} differs from the rule in {differ} of {converted.numel()} bytes")
    keep += [x, converted]
    legs += [(f"{name}: A/A (float step | float step)", float_step, float_step),
             (f"{name}: (a) float step | uint8 RGB plane step on bytes converted beforehand", float_step, step(e_bytes, converted.data_ptr())),
             (f"{name}: (b) float step | eager torch expression + uint8 step", float_step, eager_then_bytes),
             (f"{name}: (c) float step | m1v_float_planes_to_bytes_device + uint8 step", float_step, kernel_then_bytes)]
res = {}
for r in range(a.rounds):
    for name, go_left, go_right in legs:
        for side, go in ((0, go_left), (1, go_right)) if r % 2 == 0 else ((1, go_right), (0, go_left)):
            for _ in range(a.settle):
                assert go() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                assert go() == 0
            torch.cuda.synchronize()
            res.setdefault((name, side), []).append((time.perf_counter() - t0) / a.launches)
print(f"{N} x {W}x{H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); records and sizes of "
      "(a) and (c) equal to the float step's; device: " + torch.cuda.get_device_name(0), flush=True)
for note in notes:
    print(note)
for name, _, _ in legs:
    t, o = (statistics.median(res[(name, side)]) * 1e6 for side in (0, 1))
    ratios = [x / y for x, y in zip(res[(name, 0)], res[(name, 1)])]
    print(f"{name}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 0)]) + " | " + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 1)]))
for h in handles:
    L.m1v_destroy(h)
