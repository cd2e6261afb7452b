#!/usr/bin/env python3
"""What encoding a 2:1 downscaled rendition of 16-bit YCbCr frames in place (m1v_set_downscale_word_layout) costs and what it
saves, side by side in ONE process on one device, by the protocol of tools/downscale_planes_timing.py.  Per leg and side:
`--settle` untimed back-to-back calls, then `--launches` timed ones with one synchronisation (wall time per call); the sides
alternate over `--rounds` rounds and the median round is printed with the ratio left / right and the range of that ratio over the
rounds.
    per source form (p010, i010), left = the encode step of the W x H rendition on the [n, 12 W H] bytes of the source frames:
      A/A        | the same call again                                          (the spread one call against itself shows here)
      (a) bytes  | the I420 plane step on the rendition's planes, averaged beforehand     (what the four-fold, double-width
                   fetch costs)
      (b) two    | m1v_downscale_words_to_i420_device, then the I420 plane step on its [n, W H 3 / 2] bytes
      (c) bytes2 | the 8-bit downscale plane step (m1v_set_downscale_plane_layout, k_half_planes_*) on NV12 / I420 sources of
                   the same picture size, [n, 6 W H] bytes: another picture, so only the times compare
    usage: downscale_words_timing.py [--w 1920 --h 1080 --n 300] [--only p010|i010]        (w, h: the rendition's)
The records and sizes of (a) and (b) are compared with the in-place step's before anything is timed."""
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
assert W % 2 == 0 and H % 2 == 0
PRESETS = {"p010": (0, 3), "i010": (1, 1)}      # (M1V_WORDS_*, the M1V_PLANES_* of the 8-bit source of the same form)


class PlaneLayout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")]


class DownscalePlaneLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")] + \
               [("factor", C.c_int32), ("reserved", C.c_int32)]


class DownscaleWordLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")] + \
               [("factor", C.c_int32), ("shift", C.c_int32)]


L = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
L.m1v_plane_layout_preset.argtypes = [C.c_int] * 3 + [C.POINTER(PlaneLayout)]
L.m1v_set_plane_layout.argtypes = [vp, C.POINTER(PlaneLayout)]
L.m1v_downscale_plane_layout_preset.argtypes = [C.c_int] * 4 + [C.POINTER(DownscalePlaneLayout)]
L.m1v_set_downscale_plane_layout.argtypes = [vp, C.POINTER(DownscalePlaneLayout)]
L.m1v_downscale_word_layout_preset.argtypes = [C.c_int] * 4 + [C.POINTER(DownscaleWordLayout)]
L.m1v_set_downscale_word_layout.argtypes = [vp, C.POINTER(DownscaleWordLayout)]
L.m1v_downscale_words_to_i420_device.argtypes = [vp, vp, C.c_int, vp, vp]
L.m1v_frame_bound.argtypes = [vp]
L.m1v_frame_bound.restype = C.c_size_t
L.m1v_destroy.argtypes = [vp]
L.m1v_last_error.restype = C.c_char_p
handles = []


def create():
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, 3, a.q, 1, N) == 0, L.m1v_last_error()
    handles.append(h)
    return h


e_planes = create()
out = torch.empty(N * L.m1v_frame_bound(e_planes), dtype=torch.uint8, device="cuda")
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


# ---- the sources: synthetic bytes at the source's size, read as the form's words (for i010 with the six bits above the depth
#      cleared, a software decoder's words); the 8-bit source of (c) is synthetic bytes of its own ----
src = torch.empty((N, 12 * W * H), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(src.data_ptr(), 12 * W * H, N, 504, 0, None)
low = src.clone()
low.view(N, 6 * W * H, 2)[:, :, 1] &= 3
bytes_src = torch.empty((N, 6 * W * H), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(bytes_src.data_ptr(), 6 * W * H, N, 505, 0, None)
torch.cuda.synchronize()
staged = torch.empty((N, W * H * 3 // 2), dtype=torch.uint8, device="cuda")      # where the to-i420 kernel puts its bytes
rendition = torch.empty_like(staged)                                           # ... and a copy taken beforehand
i420 = PlaneLayout()
assert L.m1v_plane_layout_preset(W, H, 1, C.byref(i420)) == 0
assert L.m1v_set_plane_layout(e_planes, C.byref(i420)) == 0, L.m1v_last_error()
plane_step = step(e_planes, rendition.data_ptr())
header = ""
for tag, (preset, byte_preset) in PRESETS.items():
    if a.only and tag not in a.only.split(","):
        continue
    words = src if tag == "p010" else low
    e_down = create()
    lay = DownscaleWordLayout()
    assert L.m1v_downscale_word_layout_preset(W, H, preset, 2, C.byref(lay)) == 0
    assert L.m1v_set_downscale_word_layout(e_down, C.byref(lay)) == 0, L.m1v_last_error()
    in_place = step(e_down, words.data_ptr())
    e_bytes = create()
    byte_lay = DownscalePlaneLayout()
    assert L.m1v_downscale_plane_layout_preset(W, H, byte_preset, 2, C.byref(byte_lay)) == 0
    assert L.m1v_set_downscale_plane_layout(e_bytes, C.byref(byte_lay)) == 0, L.m1v_last_error()
    byte_step = step(e_bytes, bytes_src.data_ptr())

    def kernel_then_planes(e_down=e_down, words=words):
        rc = L.m1v_downscale_words_to_i420_device(e_down, words.data_ptr(), N, staged.data_ptr(), None)
        return rc or step(e_planes, staged.data_ptr())()

    assert L.m1v_downscale_words_to_i420_device(e_down, words.data_ptr(), N, rendition.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want = result(in_place, tag)
    same(result(plane_step, tag + " bytes"), want, tag + ": I420 plane step on the rendition's bytes")
    same(result(kernel_then_planes, tag + " two-pass"), want, tag + ": to-i420 kernel + I420 plane step")
    result(byte_step, "8-bit")
    legs = [(f"{tag}: A/A (in place | in place)", in_place, in_place),
            (f"{tag}: (a) in place | I420 plane step on planes averaged beforehand", in_place, plane_step),
            (f"{tag}: (b) in place | m1v_downscale_words_to_i420_device + I420 plane step", in_place, kernel_then_planes),
            (f"{tag}: (c) in place | 8-bit downscale plane step on {'NV12' if byte_preset == 3 else 'I420'} sources of the same size", in_place, byte_step)]
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
    if not header:
        header = (f"{N} x {W}x{H} from {2 * W}x{2 * H} words q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + "
                  f"{a.launches} timed); records and sizes of (a) and (b) equal to the in-place step's; device: "
                  + torch.cuda.get_device_name(0))
        print(header, flush=True)
    for leg, _, _ in legs:
        t, o = (statistics.median(res[(leg, side)]) * 1e6 for side in (0, 1))
        ratios = [p / q for p, q in zip(res[(leg, 0)], res[(leg, 1)])]
        print(f"{leg}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
              + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 0)]) + " | " + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 1)]), flush=True)
    del in_place, kernel_then_planes, byte_step
for h in handles:
    L.m1v_destroy(h)
