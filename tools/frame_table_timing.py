#!/usr/bin/env python3
"""What a frame table (m1v_set_frame_table) costs and what it saves, side by side in ONE process on one device, in the mould of
tools/rgb_planes_timing.py.  Per leg and side: `--settle` untimed back-to-back calls, then `--launches` timed ones with one
synchronisation (wall time per call); the sides alternate over `--rounds` rounds and the median round is printed with the ratio
left / right and the range of that ratio over the rounds.
    per layout (B,G,R,A surface with padded rows; NV12 planes; R/G/B planes):
      A/A        stride encode | the same call again                              (the spread one call against itself shows here)
      table      table encode of base + f * stride | stride encode, same buffer   (what the table lookup costs)
      scattered  table encode of the frames where they lie, in a shuffled order | a device gather of those frames into a contiguous
                 batch (one index_select over the frames' rows) followed by the stride encode   (what the table saves)
    --other <libencoder.so>: also   stride encode of this tree | of the other library (the parent commit's); tools/layout_timing.py
    is the fuller form of that leg, with its own A/A side
    usage: frame_table_timing.py [--w 1920 --h 1080 --n 300] [--other <path>] [--only <text>[,<text>]]
Every output (records and sizes) of every side is compared with the stride encode of the same pictures before anything is timed."""
import argparse
import ctypes as C
import os
import statistics
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--other", default="")
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


def layout_struct(ctype, *names):
    return type("Layout", (C.Structure,), {"_fields_": [(k, ctype) for k in names]})


PlaneLayout = layout_struct(C.c_size_t, "y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")
RgbPlaneLayout = layout_struct(C.c_uint64, "r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")


def load(path):
    L = C.CDLL(path)
    L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.m1v_destroy.argtypes = [vp]
    L.m1v_last_error.restype = C.c_char_p
    for kind, struct in (("plane", PlaneLayout), ("rgb_plane", RgbPlaneLayout)):
        getattr(L, f"m1v_{kind}_layout_preset").argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(struct)]
        getattr(L, f"m1v_set_{kind}_layout").argtypes = [vp, C.POINTER(struct)]
    if hasattr(L, "m1v_set_frame_table"):
        L.m1v_set_frame_table.argtypes = [vp, C.c_int]
    return L


this = load(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so"))
other = load(a.other) if a.other else None
handles = []


def create(L, channels, surface=None, preset=None, table=False):
    """An encoder of L; surface: the arguments of m1v_set_input_layout; preset: (kind, struct, preset number, frame stride)."""
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, channels, a.q, 1, N) == 0, L.m1v_last_error()
    if surface:
        assert L.m1v_set_input_layout(h, *surface) == 0, L.m1v_last_error()
    if preset:
        kind, struct, number, frame_stride = preset
        lay = struct()
        assert getattr(L, f"m1v_{kind}_layout_preset")(W, H, number, C.byref(lay)) == 0, L.m1v_last_error()
        lay.frame_stride = frame_stride
        assert getattr(L, f"m1v_set_{kind}_layout")(h, C.byref(lay)) == 0, L.m1v_last_error()
    if table:
        assert L.m1v_set_frame_table(h, 1) == 0, L.m1v_last_error()
    handles.append((L, h))
    return h


out = torch.empty(N * (W * H // 2 + 4096), dtype=torch.uint8, device="cuda")
sizes = torch.empty(N, dtype=torch.int64, device="cuda")
meta = torch.zeros(2, dtype=torch.int64, device="cuda")


def step(L, h, ptr):
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


# ---- the pictures: synthetic frames of 3 and 4 bytes per pixel, whose bytes every layout reads as they lie (tools/layout_timing.py):
#      the step is timed, not the pictures.  `pool` holds the same frames in a shuffled order: frame f lies at row place[f]. ----
rgb3 = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
rgb4 = torch.empty((N, H, W, 4), dtype=torch.uint8, device="cuda")
this.m1v_synth_device(rgb3.data_ptr(), W * H * 3, N, 504, 0, None)
this.m1v_synth_device(rgb4.data_ptr(), W * H * 4, N, 504, 0, None)
torch.cuda.synchronize()
gen = torch.Generator()
gen.manual_seed(504)
place = torch.randperm(N, generator=gen)
place_dev = place.cuda()
frame3, frame4 = W * H * 3, W * H * 4
layouts = [   # (name, channels, create()'s layout arguments, frames, bytes between frames)
    ("B,G,R,A surface, rows 4 * W bytes apart", 3, {"surface": (W * 4, frame4, 1)}, rgb4, frame4),
    ("NV12 planes", 3, {"preset": ("plane", PlaneLayout, 3, frame3)}, rgb3, frame3),
    ("R/G/B planes", 3, {"preset": ("rgb_plane", RgbPlaneLayout, 0, frame3)}, rgb3, frame3),
]
legs, keep = [], []
for name, channels, layout, frames, stride in layouts:
    rows = frames.view(N, -1)
    pool = torch.empty_like(rows)
    pool[place_dev] = rows                                      # frame f lies at pool[place[f]]
    staged = torch.empty_like(rows)                             # where the caller without a table gathers to
    in_order = torch.tensor([frames.data_ptr() + f * stride for f in range(N)], dtype=torch.int64).cuda()
    scattered = torch.tensor([pool.data_ptr() + int(place[f]) * stride for f in range(N)], dtype=torch.int64).cuda()
    keep += [pool, staged, in_order, scattered]
    e_stride, e_table = create(this, channels, **layout), create(this, channels, table=True, **layout)
    by_stride = step(this, e_stride, frames.data_ptr())
    by_table = step(this, e_table, in_order.data_ptr())
    by_scattered = step(this, e_table, scattered.data_ptr())
    staged_step = step(this, e_stride, staged.data_ptr())

    def gather_then_stride(pool=pool, staged=staged, staged_step=staged_step):
        torch.index_select(pool, 0, place_dev, out=staged)
        return staged_step()

    want = result(by_stride, name)
    same(result(by_table, name + " table"), want, name + ": table")
    same(result(by_scattered, name + " scattered"), want, name + ": scattered table")
    same(result(gather_then_stride, name + " gather"), want, name + ": gather + stride")
    assert torch.equal(staged, rows)
    legs += [(f"{name}: A/A (stride | stride)", by_stride, by_stride),
             (f"{name}: table of base + f * stride | stride, same buffer", by_table, by_stride),
             (f"{name}: scattered frames, table | device gather + stride", by_scattered, gather_then_stride)]
    if other:
        by_other = step(other, create(other, channels, **layout), frames.data_ptr())
        same(result(by_other, name + " other"), want, name + ": other library")
        legs.append((f"{name}: stride, this tree | the other library", by_stride, by_other))
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
      "every side equal to the stride encode's; device: " + torch.cuda.get_device_name(0))
for name, _, _ in legs:
    t, o = (statistics.median(res[(name, side)]) * 1e6 for side in (0, 1))
    ratios = [x / y for x, y in zip(res[(name, 0)], res[(name, 1)])]
    print(f"{name}\n    left {t:9.1f}  right {o:9.1f}  left/right {t / o:6.4f}  (rounds {min(ratios):6.4f} .. {max(ratios):6.4f})   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 0)]) + " | " + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 1)]))
for L, h in handles:
    L.m1v_destroy(h)
