#!/usr/bin/env python3
"""What encoding float pixels in place (m1v_set_float_pixel_layout) costs and what it saves, side by side in ONE process on one
device, by the protocol of tools/float_planes_timing.py.  Per leg and side: `--settle` untimed back-to-back calls, then
`--launches` timed ones with one synchronisation (wall time per call); the sides alternate over `--rounds` rounds and the median
round is printed with the ratio left / right and the range of that ratio over the rounds.
    per sample type (float16, bfloat16, float32) and pixel width (3, 4), left = the encode step on the float tensor [n, H, W, C]:
      A/A        | the same call again                                          (the spread one call against itself shows here)
      (a) bytes  | the uint8 step on bytes converted beforehand: the default packed step (C = 3), the surface step on
                   [n, H, W, 4] bytes (C = 4)                                   (what the wider samples cost)
      (b) eager  | x.mul(255).round().clamp(0, 255).to(torch.uint8), then (a)   (what callers do today)
      (c) planes | x.permute(0, 3, 1, 2)[:, :3].contiguous(), then the float plane step   (today's route through the library)
      (d) two    | m1v_float_pixels_to_bytes_device, then the default packed step on its [n, H, W, 3] bytes
    usage: float_pixels_timing.py [--w 1920 --h 1080 --n 300] [--only <text>[,<text>]]     (text: e.g. float16x3)
The records and sizes of (a), (c) and (d) are compared with the in-place step's before anything is timed; for (b) the count of
bytes in which torch's expression (evaluated in the tensor's own type) differs from the rule is printed."""
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


class FloatPlaneLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")] + \
               [("sample", C.c_int32), ("range", C.c_int32)]


class FloatPixelLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("row_pitch", "frame_stride", "pixel_step")] + \
               [("order", C.c_int32), ("sample", C.c_int32), ("range", C.c_int32)]


L = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
L.m1v_set_float_plane_layout.argtypes = [vp, C.POINTER(FloatPlaneLayout)]
L.m1v_set_float_pixel_layout.argtypes = [vp, C.POINTER(FloatPixelLayout)]
L.m1v_float_pixels_to_bytes_device.argtypes = [vp, vp, C.c_int, vp, vp]
L.m1v_destroy.argtypes = [vp]
L.m1v_last_error.restype = C.c_char_p
handles = []


def create(layout=None, channels=3):
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, channels, a.q, 1, N) == 0, L.m1v_last_error()
    if isinstance(layout, FloatPixelLayout):
        assert L.m1v_set_float_pixel_layout(h, C.byref(layout)) == 0, L.m1v_last_error()
    elif isinstance(layout, FloatPlaneLayout):
        assert L.m1v_set_float_plane_layout(h, C.byref(layout)) == 0, L.m1v_last_error()
    elif layout == "surface":
        assert L.m1v_set_input_layout(h, W * channels, 0, 0) == 0, L.m1v_last_error()
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


# ---- the pictures: synthetic packed bytes, and each type's samples byte / 255 rounded to the type ----
rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(rgb.data_ptr(), LUMA * 3, N, 504, 0, None)
torch.cuda.synchronize()
rgba = torch.zeros((N, H, W, 4), dtype=torch.uint8, device="cuda")      # the same bytes as four-byte pixels
rgba[..., :3] = rgb
staged = torch.empty_like(rgb)          # where the bytes kernel puts its bytes
e_packed = create()
e_surface4 = create("surface", channels=4)
packed_step = step(e_packed, rgb.data_ptr())
legs, notes, header = [], [], ""
for code, dtype in enumerate((torch.float16, torch.bfloat16, torch.float32)):
    name = str(dtype).rsplit(".", 1)[-1]
    S = 2 if code < 2 else 4
    e_planes = create(FloatPlaneLayout(0, LUMA * S, 2 * LUMA * S, W * S, 3 * LUMA * S, code, 0))
    for Cs in (3, 4):
        tag = f"{name}x{Cs}"
        if a.only and not any(text in tag for text in a.only.split(",")):
            continue
        x = torch.zeros((N, H, W, Cs), dtype=dtype, device="cuda")
        for f in range(0, N, 10):            # in pieces: no float32 temporary of the batch's size
            x[f:f + 10, ..., :3] = (rgb[f:f + 10].float() / 255.0).to(dtype)
        e_pixels = create(FloatPixelLayout(W * Cs * S, LUMA * Cs * S, Cs * S, 0, code, 0))
        in_place = step(e_pixels, x.data_ptr())
        bytes_step = packed_step if Cs == 3 else step(e_surface4, rgba.data_ptr())
        e_bytes = e_packed if Cs == 3 else e_surface4

        def eager_then_bytes(x=x, e_bytes=e_bytes):     # (the expression's result encoded where torch put it)
            y = x.mul(255).round().clamp(0, 255).to(torch.uint8)
            return step(e_bytes, y.data_ptr())()

        def planes_then_float(x=x, e_planes=e_planes):
            y = x.permute(0, 3, 1, 2)[:, :3].contiguous()
            return step(e_planes, y.data_ptr())()

        def kernel_then_bytes(x=x, e_pixels=e_pixels):
            rc = L.m1v_float_pixels_to_bytes_device(e_pixels, x.data_ptr(), N, staged.data_ptr(), None)
            return rc or step(e_packed, staged.data_ptr())()

        want = result(in_place, tag)
        same(result(bytes_step, tag + " bytes"), want, tag + ": uint8 step on the rule's bytes")
        same(result(planes_then_float, tag + " planes"), want, tag + ": permute + float plane step")
        same(result(kernel_then_bytes, tag + " two-pass"), want, tag + ": bytes kernel + packed step")
        assert torch.equal(staged, rgb), tag + ": the bytes kernel's bytes"
        differ = 0
        for f in range(0, N, 10):
            differ += int((x[f:f + 10, ..., :3].mul(255).round().clamp(0, 255).to(torch.uint8) != rgb[f:f + 10]).sum().item())
        notes.append(f"{tag}: torch's expression in {name} differs from the rule in {differ} of {rgb.numel()} bytes")
        uint8_step = "default packed step" if Cs == 3 else "surface step on [n, H, W, 4] bytes"
        legs += [(f"{tag}: A/A (in place | in place)", in_place, in_place),
                 (f"{tag}: (a) in place | {uint8_step} on bytes converted beforehand", in_place, bytes_step),
                 (f"{tag}: (b) in place | eager torch expression + (a)", in_place, eager_then_bytes),
                 (f"{tag}: (c) in place | permute(0, 3, 1, 2)[:, :3].contiguous() + float plane step", in_place, planes_then_float),
                 (f"{tag}: (d) in place | m1v_float_pixels_to_bytes_device + default packed step", in_place, kernel_then_bytes)]
        res = {}
        for r in range(a.rounds):           # a variant's legs are timed while its tensor is the only large one alive
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
        if not header:
            header = (f"{N} x {W}x{H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); records "
                      "and sizes of (a), (c) and (d) equal to the in-place step's; device: " + torch.cuda.get_device_name(0))
            print(header, flush=True)
        print(notes[-1])
        for leg, _, _ in legs:
            t, o = (statistics.median(res[(leg, side)]) * 1e6 for side in (0, 1))
            ratios = [p / q for p, q in zip(res[(leg, 0)], res[(leg, 1)])]
            print(f"{leg}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
                  + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 0)]) + " | " + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 1)]), flush=True)
        legs = []
        del x, in_place, eager_then_bytes, planes_then_float, kernel_then_bytes
        torch.cuda.empty_cache()
for h in handles:
    L.m1v_destroy(h)
