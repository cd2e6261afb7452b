#!/usr/bin/env python3
"""What a plane table (m1v_set_plane_table) costs and what it saves, side by side in ONE process on one device, in the mould of
tools/frame_table_timing.py.  Per leg and side: `--settle` untimed back-to-back calls, then `--launches` timed ones with one
synchronisation (wall time per call); the sides alternate over `--rounds` rounds and the median round is printed with the ratio
left / right and the range of that ratio over the rounds.
    per layout (I420 planes; NV12 planes; R/G/B planes):
      A/A        frame-table encode | the same call again                           (the spread one call against itself shows here)
      (1) planes plane-table encode, three pointers computed from each frame's base | frame-table encode, same contiguous buffer
                                                                                     (what the per-lane address and the clamp per plane cost)
      (2) apart  plane-table encode of planes that lie in three separate allocations | a device copy of those planes into contiguous
                 frames (one copy per plane) followed by the stride encode           (what the table saves)
    usage: plane_table_timing.py [--w 1920 --h 1080 --n 300] [--only <text>[,<text>]]
Every output (records and sizes) of every side is compared with the stride encode of the same pictures before anything is timed."""
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
ap.add_argument("--settle", type=int, default=40)
ap.add_argument("--launches", type=int, default=60)
ap.add_argument("--only", default="")
a = ap.parse_args()
import torch

vp = C.c_void_p
W, H, N = a.w, a.h, a.n
assert W % 2 == 0 and H % 2 == 0
LUMA, QUARTER = W * H, (W // 2) * (H // 2)


def layout_struct(ctype, *names):
    return type("Layout", (C.Structure,), {"_fields_": [(k, ctype) for k in names]})


PlaneLayout = layout_struct(C.c_size_t, "y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")
RgbPlaneLayout = layout_struct(C.c_uint64, "r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")

L = C.CDLL(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
L.m1v_set_plane_layout.argtypes = [vp, C.POINTER(PlaneLayout)]
L.m1v_set_rgb_plane_layout.argtypes = [vp, C.POINTER(RgbPlaneLayout)]
L.m1v_set_frame_table.argtypes = [vp, C.c_int]
L.m1v_set_plane_table.argtypes = [vp, C.c_int]
L.m1v_destroy.argtypes = [vp]
L.m1v_last_error.restype = C.c_char_p
handles = []


def create(layout, table=None):
    """An encoder with `layout` (a PlaneLayout or an RgbPlaneLayout) and the table mode `table` (None, "frames", "planes")."""
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, 3, a.q, 1, N) == 0, L.m1v_last_error()
    setter = L.m1v_set_plane_layout if isinstance(layout, PlaneLayout) else L.m1v_set_rgb_plane_layout
    assert setter(h, C.byref(layout)) == 0, L.m1v_last_error()
    if table:
        assert (L.m1v_set_frame_table if table == "frames" else L.m1v_set_plane_table)(h, 1) == 0, L.m1v_last_error()
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


def addresses(rows):
    return torch.tensor(rows, dtype=torch.int64).cuda()


# ---- the pictures: synthetic bytes that every layout reads as they lie (tools/layout_timing.py): the step is timed, not the pictures ----
ycc = torch.empty((N, LUMA * 3 // 2), dtype=torch.uint8, device="cuda")     # tightly packed 4:2:0 frames
rgb = torch.empty((N, 3, H, W), dtype=torch.uint8, device="cuda")
L.m1v_synth_device(ycc.data_ptr(), LUMA * 3 // 2, N, 504, 0, None)
L.m1v_synth_device(rgb.data_ptr(), LUMA * 3, N, 504, 0, None)
torch.cuda.synchronize()
legs, keep = [], []
for name in ("I420", "NV12", "R/G/B"):
    if name == "R/G/B":
        frames, stride = rgb, 3 * LUMA
        whole = RgbPlaneLayout(0, LUMA, 2 * LUMA, W, stride)
        apart_layout, offsets = whole, (0, LUMA, 2 * LUMA)      # (a plane's range starts at its offset: its pointer lies that far in front)
        planes = [rgb[:, c].reshape(N, LUMA).clone() for c in range(3)]     # three allocations: every frame's R, G and B
        spans = [(c * LUMA, LUMA) for c in range(3)]
        entry = [(planes[p], 0) for p in range(3)]
    else:
        frames, stride = ycc, LUMA * 3 // 2
        planar = name == "I420"
        whole = PlaneLayout(0, LUMA, LUMA + (QUARTER if planar else 1), W, W // 2 if planar else W, 1 if planar else 2, stride)
        apart_layout, offsets = PlaneLayout(0, 0, 0 if planar else 1, W, whole.c_pitch, whole.c_step, LUMA), (0, 0, 0)
        spans = [(0, LUMA), (LUMA, QUARTER), (LUMA + QUARTER, QUARTER)] if planar else [(0, LUMA), (LUMA, 2 * QUARTER)]
        planes = [ycc[:, at:at + length].clone() for at, length in spans]   # allocations of their own: every frame's Y, Cb, Cr (or Y, UV)
        entry = [(planes[0], 0), (planes[1], 0), (planes[2], 0) if planar else (planes[1], 0)]
    flat = frames.view(N, -1)
    staged = torch.empty_like(flat)                                         # where the caller without a table copies the planes to
    by_frame = addresses([flat.data_ptr() + f * stride for f in range(N)])
    by_plane = addresses([[flat.data_ptr() + f * stride] * 3 for f in range(N)])
    apart = addresses([[t.data_ptr() + f * t.stride(0) + d - o for (t, d), o in zip(entry, offsets)] for f in range(N)])
    keep += [planes, staged, by_frame, by_plane, apart]
    e_stride, e_frames, e_planes, e_apart = create(whole), create(whole, "frames"), create(whole, "planes"), create(apart_layout, "planes")
    frame_step, plane_step, apart_step = step(e_frames, by_frame.data_ptr()), step(e_planes, by_plane.data_ptr()), step(e_apart, apart.data_ptr())
    staged_step = step(e_stride, staged.data_ptr())

    def copy_then_stride(planes=planes, staged=staged, spans=spans, staged_step=staged_step):
        for t, (at, length) in zip(planes, spans):
            staged[:, at:at + length].copy_(t)
        return staged_step()

    want = result(step(e_stride, flat.data_ptr()), name)
    same(result(frame_step, name + " frame table"), want, name + ": frame table")
    same(result(plane_step, name + " plane table"), want, name + ": plane table, one buffer")
    same(result(apart_step, name + " planes apart"), want, name + ": plane table, separate allocations")
    same(result(copy_then_stride, name + " copy"), want, name + ": copy + stride")
    assert torch.equal(staged, flat)
    legs += [(f"{name} planes: A/A (frame table | frame table)", frame_step, frame_step),
             (f"{name} planes: (1) plane table of pointers from one base | frame table, same buffer", plane_step, frame_step),
             (f"{name} planes: (2) separately allocated planes, plane table | device copy into frames + stride", apart_step, copy_then_stride)]
if a.only:
    legs = [leg for leg in legs if any(text in leg[0] for text in a.only.split(","))]
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
      "every side equal to the stride encode's; device: " + torch.cuda.get_device_name(0), flush=True)
for name, _, _ in legs:
    t, o = (statistics.median(res[(name, side)]) * 1e6 for side in (0, 1))
    ratios = [x / y for x, y in zip(res[(name, 0)], res[(name, 1)])]
    print(f"{name}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 0)]) + " | " + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 1)]))
for h in handles:
    L.m1v_destroy(h)
