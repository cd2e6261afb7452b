#!/usr/bin/env python3
"""The same encode step of every input layout on this tree's library and on another build of it (the parent commit's), side by
side in ONE process on one device, for a change that leaves the device code as it was (tools/device_code_diff.py) and can only
move host launch overhead.  Three sides per leg: this tree, the other library, and a copy of this tree's library loaded as a
third image (the A/A side).  Per leg and side: `--settle` untimed back-to-back calls, then `--launches` timed ones with one
synchronisation (wall time per call); the order of the sides rotates over `--rounds` rounds and the median round is printed with
this / other.  The A/A spread of a leg = the range of this / copy over the rounds: what one library against itself shows in this
run; `within` = the median this / other lies inside it.
    legs  packed C=3 (tiles), packed C=4 (runs), B,G,R surface with padded rows, NV12 planes, YUY2 samples, R/G/B planes
    usage: layout_timing.py --other <path to the other libencoder.so> [--w 1920 --h 1080 --n 300]
The records and sizes of the three sides are compared on every leg before anything is timed."""
import argparse
import ctypes as C
import os
import shutil
import statistics
import tempfile
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
W, H, N = a.w, a.h, a.n
assert W % 2 == 0 and H % 2 == 0


def layout_struct(ctype, *names):
    return type("Layout", (C.Structure,), {"_fields_": [(k, ctype) for k in names]})


PlaneLayout = layout_struct(C.c_size_t, "y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")
SampleLayout = layout_struct(C.c_size_t, "y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "y_step", "c_step", "frame_stride")
RgbPlaneLayout = layout_struct(C.c_uint64, "r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")


def load(path):
    L = C.CDLL(path)
    L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.m1v_destroy.argtypes = [vp]
    L.m1v_last_error.restype = C.c_char_p
    for kind, struct in (("plane", PlaneLayout), ("sample", SampleLayout), ("rgb_plane", RgbPlaneLayout)):
        getattr(L, f"m1v_{kind}_layout_preset").argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(struct)]
        getattr(L, f"m1v_set_{kind}_layout").argtypes = [vp, C.POINTER(struct)]
    return L


this_path = os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so")
tmp = tempfile.mkdtemp()
libs = {"this": load(this_path), "other": load(a.other), "copy": load(shutil.copy(this_path, os.path.join(tmp, "libencoder_copy.so")))}
handles = []


def create(L, channels, surface=None, preset=None):
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


# ---- the pictures: synthetic frames of 3 and 4 bytes per pixel.  Every layout reads the same bytes: a surface with padded rows lies
#      in the 4-byte frames' buffer, and the plane and sample layouts take the 3-byte frames' bytes as they lie, frames 3 * W * H
#      apart (NV12 spans 1.5, YUY2 2, R/G/B planes 3 W * H of them): the step is timed, not the pictures ----
rgb3 = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
rgb4 = torch.empty((N, H, W, 4), dtype=torch.uint8, device="cuda")
libs["this"].m1v_synth_device(rgb3.data_ptr(), W * H * 3, N, 504, 0, None)
libs["this"].m1v_synth_device(rgb4.data_ptr(), W * H * 4, N, 504, 0, None)
torch.cuda.synchronize()
frame = W * H * 3
legs = [   # (name, channels, create()'s layout arguments, input)
    ("packed C=3 (k_encode_tiles)", 3, {}, rgb3),
    ("packed C=4 (run kernels)", 4, {}, rgb4),
    ("B,G,R surface, rows 4 * W bytes apart (k_encode_surface)", 3, {"surface": (W * 4, W * H * 4, 1)}, rgb4),
    ("NV12 planes (k_encode_planes)", 3, {"preset": ("plane", PlaneLayout, 3, frame)}, rgb3),
    ("YUY2 samples (k_encode_step2)", 3, {"preset": ("sample", SampleLayout, 0, frame)}, rgb3),
    ("R/G/B planes (k_encode_rgb_planes)", 3, {"preset": ("rgb_plane", RgbPlaneLayout, 0, frame)}, rgb3),
]
sides = ("this", "other", "copy")
go = {}
for name, channels, layout, frames in legs:
    for side in sides:
        go[(name, side)] = step(libs[side], create(libs[side], channels, **layout), frames.data_ptr())
    want = result(go[(name, "other")], name)
    for side in ("this", "copy"):
        got = result(go[(name, side)], name)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{name}: the records of {side} and other differ"

res = {}
for r in range(a.rounds):
    for name, _, _, _ in legs:
        for side in sides[r % 3:] + sides[:r % 3]:
            f = go[(name, side)]
            for _ in range(a.settle):
                assert f() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                assert f() == 0
            torch.cuda.synchronize()
            res.setdefault((name, side), []).append((time.perf_counter() - t0) / a.launches)
print(f"{N} x {W}x{H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); records and sizes "
      "of the three sides equal on every leg; device: " + torch.cuda.get_device_name(0))
for name, _, _, _ in legs:
    t, o, c = (statistics.median(res[(name, side)]) * 1e6 for side in sides)
    aa = [x / y for x, y in zip(res[(name, "this")], res[(name, "copy")])]
    verdict = "within" if min(aa) <= t / o <= max(aa) else "OUTSIDE"
    print(f"{name}\n    this {t:8.1f}  other {o:8.1f}  copy {c:8.1f}   this/other {t / o:6.4f}  {verdict} the A/A spread {min(aa):6.4f} .. {max(aa):6.4f}\n"
          "    rounds: " + " | ".join(" ".join(f"{x * 1e6:.1f}" for x in res[(name, side)]) for side in sides))
for L, h in handles:
    L.m1v_destroy(h)
shutil.rmtree(tmp)
