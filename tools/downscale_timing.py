#!/usr/bin/env python3
"""What encoding a 2:1 downscaled rendition in place (m1v_set_downscale_layout) costs and what it saves, side by side in ONE
process on one device, by the protocol of tools/float_pixels_timing.py.  Per leg and side: `--settle` untimed back-to-back calls,
then `--launches` timed ones with one synchronisation (wall time per call); the sides alternate over `--rounds` rounds and the
median round is printed with the ratio left / right and the range of that ratio over the rounds.
    per source pixel width (3, 4), left = the encode step of the W x H rendition on the [n, 2H, 2W, C] uint8 source:
      A/A        | the same call again                                          (the spread one call against itself shows here)
      (a) bytes  | the default packed step on the rendition's bytes, averaged beforehand   (what the four-fold fetch costs)
      (b) two    | m1v_downscale_to_bytes_device, then the default packed step on its [n, H, W, 3] bytes
      (c) torch  | torch computing the same bytes (cells, widened, summed, + 2, >> 2, to uint8), then the default packed step
    usage: downscale_timing.py [--w 1920 --h 1080 --n 300] [--only x3|x4]        (w, h: the rendition's)
The records and sizes of (a), (b) and (c) are compared with the in-place step's before anything is timed."""
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


class DownscaleLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("row_pitch", "frame_stride", "pixel_step")] + [("order", C.c_int32), ("factor", C.c_int32)]


L = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
L.m1v_set_downscale_layout.argtypes = [vp, C.POINTER(DownscaleLayout)]
L.m1v_downscale_to_bytes_device.argtypes = [vp, vp, C.c_int, vp, vp]
L.m1v_destroy.argtypes = [vp]
L.m1v_last_error.restype = C.c_char_p
handles = []


def create(layout=None):
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, 3, a.q, 1, N) == 0, L.m1v_last_error()
    if layout is not None:
        assert L.m1v_set_downscale_layout(h, C.byref(layout)) == 0, L.m1v_last_error()
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


def torch_down2(x):
    """The definition in torch: reshape to cells, widen, sum, + 2, >> 2, to uint8; the 4th byte dropped."""
    cells = x.view(N, H, 2, W, 2, x.shape[-1])[..., :3]
    return cells.to(torch.int16).sum(dim=(2, 4), dtype=torch.int16).add_(2).bitwise_right_shift_(2).to(torch.uint8)


# ---- the pictures: synthetic packed bytes at the source's size; the rendition's bytes by the definition ----
src3 = torch.empty((N, 2 * H, 2 * W, 3), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(src3.data_ptr(), 4 * W * H * 3, N, 504, 0, None)
torch.cuda.synchronize()
rendition = torch_down2(src3).contiguous()
staged = torch.empty_like(rendition)    # where the bytes kernel puts its bytes
e_packed = create()
packed_step = step(e_packed, rendition.data_ptr())
header = ""
for Cs in (3, 4):
    tag = f"x{Cs}"
    if a.only and tag not in a.only.split(","):
        continue
    if Cs == 3:
        x = src3
    else:
        x = torch.zeros((N, 2 * H, 2 * W, 4), dtype=torch.uint8, device="cuda")
        x[..., :3] = src3
    e_down = create(DownscaleLayout(2 * W * Cs, 2 * H * 2 * W * Cs, Cs, 0, 2))
    in_place = step(e_down, x.data_ptr())

    def kernel_then_bytes(x=x, e_down=e_down):
        rc = L.m1v_downscale_to_bytes_device(e_down, x.data_ptr(), N, staged.data_ptr(), None)
        return rc or step(e_packed, staged.data_ptr())()

    def torch_then_bytes(x=x):      # (the expression's result encoded where torch put it)
        y = torch_down2(x)
        return step(e_packed, y.data_ptr())()

    want = result(in_place, tag)
    same(result(packed_step, tag + " bytes"), want, tag + ": packed step on the definition's bytes")
    same(result(kernel_then_bytes, tag + " two-pass"), want, tag + ": bytes kernel + packed step")
    assert torch.equal(staged, rendition), tag + ": the bytes kernel's bytes"
    same(result(torch_then_bytes, tag + " torch"), want, tag + ": torch + packed step")
    legs = [(f"{tag}: A/A (in place | in place)", in_place, in_place),
            (f"{tag}: (a) in place | default packed step on bytes averaged beforehand", in_place, packed_step),
            (f"{tag}: (b) in place | m1v_downscale_to_bytes_device + default packed step", in_place, kernel_then_bytes),
            (f"{tag}: (c) in place | torch cells.sum + 2 >> 2 + default packed step", in_place, torch_then_bytes)]
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
        header = (f"{N} x {W}x{H} from {2 * W}x{2 * H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + "
                  f"{a.launches} timed); records and sizes of (a), (b) and (c) equal to the in-place step's; device: "
                  + torch.cuda.get_device_name(0))
        print(header, flush=True)
    for leg, _, _ in legs:
        t, o = (statistics.median(res[(leg, side)]) * 1e6 for side in (0, 1))
        ratios = [p / q for p, q in zip(res[(leg, 0)], res[(leg, 1)])]
        print(f"{leg}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
              + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 0)]) + " | " + " ".join(f"{v * 1e6:.1f}" for v in res[(leg, 1)]), flush=True)
    if Cs == 4:
        del x
    del in_place, kernel_then_bytes, torch_then_bytes
    torch.cuda.empty_cache()
for h in handles:
    L.m1v_destroy(h)
