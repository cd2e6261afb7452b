#!/usr/bin/env python3
"""Plane encodes (m1v_set_plane_layout) of this tree against another build of the library (the parent commit's, which has no
plane layout), side by side in ONE process on one device, in the mould of tools/surface_timing.py.  Per leg and side:
`--settle` untimed back-to-back calls, then `--launches` timed ones with one synchronisation (wall time per call); sides and
legs alternate for `--rounds` rounds and the median round is printed with the ratio left / right.
    legs  plain packed C=3 / C=4, BGRA surface   this tree | the other library       (the existing kernels: no regression)
          reference planes / NV12 / I420 step    this tree | the other library's packed RGB step on the RGB frames the planes
                                                             were converted from (same records out)
          the same                               this tree | what a caller of the other library must do: a torch YCbCr -> RGB
                                                             conversion into a packed buffer + its packed step (ITS BYTES
                                                             DIFFER: 8-bit YCbCr -> RGB -> YCbCr is not the identity; a cost
                                                             comparison only)
          table K=8, budget K=8 on NV12          this tree | the other library's on packed RGB
          YUY2 / P010 step                       this tree | the other library's packed RGB step, and its NV12 step where it
                                                             has plane layouts, on the same pictures (m1v_set_sample_layout:
                                                             samples two bytes apart; same records out)
    --only <text>: time only the legs whose name contains <text> (several: a comma-separated list); every output is still checked
    usage: planes_timing.py --other <path to the other libencoder.so> [--w 1920 --h 1080 --n 300]
Every plane output (records, sizes, K = 8 table) is compared with the other library's output on the RGB frames before anything
is timed.  Also printed: the time of the encode kernel alone under m1v_profile_* for each side."""
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
ap.add_argument("--only", default="")
a = ap.parse_args()
import torch

vp = C.c_void_p
K8 = (2, 3, 4, 6, 8, 9, 10, 12)
PAD = 256
W, H, N = a.w, a.h, a.n
assert W % 2 == 0 and H % 2 == 0


class PlaneLayout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "c_step", "frame_stride")]


class SampleLayout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("y_offset", "cb_offset", "cr_offset", "y_pitch", "c_pitch", "y_step", "c_step", "frame_stride")]


def load(path):
    L = C.CDLL(path)
    L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_frame_size_table_device.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint8), C.c_int, vp, vp, vp]
    L.m1v_encode_budget_device.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_uint64, vp, vp, vp,
                                           C.c_size_t, vp, vp, vp, vp]
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_convert_device.argtypes = [vp, vp, C.c_int, vp, vp]
    L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.m1v_profile_enable.argtypes = [vp, C.c_int]
    L.m1v_profile_read.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.m1v_destroy.argtypes = [vp]
    L.m1v_path_in_use.argtypes = [vp]
    L.m1v_last_error.restype = C.c_char_p
    if hasattr(L, "m1v_set_plane_layout"):
        L.m1v_plane_layout_preset.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(PlaneLayout)]
        L.m1v_set_plane_layout.argtypes = [vp, C.POINTER(PlaneLayout)]
    if hasattr(L, "m1v_set_sample_layout"):
        L.m1v_sample_layout_preset.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(SampleLayout)]
        L.m1v_set_sample_layout.argtypes = [vp, C.POINTER(SampleLayout)]
    return L


this, other = load(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so")), load(a.other)
handles, alive = [], []


def create(L, channels, surface=None, planes=None, samples=None):
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, channels, a.q, 1, N) == 0, L.m1v_last_error()
    if surface:
        assert L.m1v_set_input_layout(h, *surface) == 0, L.m1v_last_error()
    if planes is not None:
        lay = PlaneLayout()
        assert L.m1v_plane_layout_preset(W, H, planes, C.byref(lay)) == 0, L.m1v_last_error()
        assert L.m1v_set_plane_layout(h, C.byref(lay)) == 0, L.m1v_last_error()
    if samples is not None:
        lay = SampleLayout()
        assert L.m1v_sample_layout_preset(W, H, samples, C.byref(lay)) == 0, L.m1v_last_error()
        assert L.m1v_set_sample_layout(h, C.byref(lay)) == 0, L.m1v_last_error()
    handles.append((L, h))
    return h


out = torch.empty(N * (W * H // 2 + 4096), dtype=torch.uint8, device="cuda")
sizes = torch.empty(N, dtype=torch.int64, device="cuda")
meta = torch.zeros(2, dtype=torch.int64, device="cuda")
table = torch.zeros(8 * N, dtype=torch.int64, device="cuda")
status = torch.zeros(8, dtype=torch.int32, device="cuda")
budget = int(0.75 * W * H * 3 // 54)
qs8 = (C.c_uint8 * 8)(*[min(x, a.q) for x in K8])


def plain(L, h, ptr):
    return lambda: L.m1v_encode_device(h, ptr, N, 0, out.data_ptr(), out.numel(), sizes.data_ptr(), meta.data_ptr(),
                                       meta.data_ptr() + 8, None)


def table8(L, h, ptr):
    return lambda: L.m1v_frame_size_table_device(h, ptr, N, qs8, 8, table.data_ptr(), status.data_ptr(), None)


def budget8(L, h, ptr):
    return lambda: L.m1v_encode_budget_device(h, ptr, N, 0, qs8, 8, budget, None, None, out.data_ptr(), out.numel(),
                                              sizes.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8, None)


def result(go, what):
    """The outputs of one call: (records, sizes) of an encode, or the K = 8 table."""
    out.zero_(), sizes.zero_(), meta.zero_(), table.zero_()
    assert go() == 0, what
    torch.cuda.synchronize()
    assert int(meta[1].item()) == 0 and int(status.abs().sum().item()) == 0, what
    return out[:int(meta[0].item())].clone(), sizes.clone(), table.clone()


def same(got, want, what):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{what}: records differ"


legs = []          # (name, left, right)

# ---- the existing kernels: packed 3- and 4-channel steps, a BGRA surface step ----
rgb3 = None
for ch in (3, 4):
    rgb = torch.empty((N, H, W, ch), dtype=torch.uint8, device="cuda")
    this.m1v_synth_device(rgb.data_ptr(), W * H * ch, N, 504, 0, None)
    alive.append(rgb)
    e_this, e_other = create(this, ch), create(other, ch)
    want = result(plain(other, e_other, rgb.data_ptr()), "other plain")
    same(result(plain(this, e_this, rgb.data_ptr()), "this plain"), want, f"C={ch} plain")
    legs.append((f"C={ch} plain packed (this | other)", plain(this, e_this, rgb.data_ptr()), plain(other, e_other, rgb.data_ptr())))
    if ch == 3:
        rgb3, e_rgb_this, e_rgb_other, want_rgb = rgb, e_this, e_other, want
    else:
        pitch = W * 4 + PAD
        buf = torch.randint(0, 256, (N * H * pitch,), dtype=torch.uint8, device="cuda")
        surface = torch.as_strided(buf, (N, H, W, 4), (H * pitch, pitch, 4, 1))
        surface.copy_(rgb[..., torch.tensor([2, 1, 0, 3], device="cuda")])
        alive.append(buf)
        s_this, s_other = create(this, 4, surface=(pitch, 0, 1)), create(other, 4, surface=(pitch, 0, 1))
        same(result(plain(this, s_this, surface.data_ptr()), "this surface"), want, "BGRA surface")
        same(result(plain(other, s_other, surface.data_ptr()), "other surface"), want, "BGRA surface (other)")
        legs.append((f"C=4 BGRA surface pitch W*4+{PAD} (this | other)", plain(this, s_this, surface.data_ptr()),
                     plain(other, s_other, surface.data_ptr())))
        del rgb

# ---- planes converted from the 3-channel frames ----
ref = torch.empty((N, 3, H * W), dtype=torch.uint8, device="cuda")          # what m1v_convert_device writes
assert this.m1v_convert_device(e_rgb_this, rgb3.data_ptr(), N, ref.data_ptr(), None) == 0
quarter = (H // 2) * (W // 2)
# the samples the chroma addressing reaches: the first (H / 2) rows of W / 2 bytes of each full-resolution plane
i420 = torch.cat([ref[:, 0], ref[:, 1, :quarter], ref[:, 2, :quarter]], dim=1).contiguous()
nv12 = torch.cat([ref[:, 0], torch.stack([ref[:, 1, :quarter], ref[:, 2, :quarter]], dim=2).view(N, -1)], dim=1).contiguous()
torch.cuda.synchronize()
alive += [ref, i420, nv12]
want_table = result(table8(other, e_rgb_other, rgb3.data_ptr()), "other table")[2]
want_budget = result(budget8(other, e_rgb_other, rgb3.data_ptr()), "other budget")
packed = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
alive.append(packed)


def to_rgb(y, cb, cr):
    """8-bit full-range BT.601 YCbCr -> packed R,G,B bytes in `packed` (torch: what a caller without plane input does)."""
    yf, cbf, crf = y.float(), cb.float() - 128.0, cr.float() - 128.0
    packed[..., 0] = (yf + 1.402 * crf).round_().clamp_(0, 255)
    packed[..., 1] = (yf - 0.344136 * cbf - 0.714136 * crf).round_().clamp_(0, 255)
    packed[..., 2] = (yf + 1.772 * cbf).round_().clamp_(0, 255)


def up(c):                                                  # [N, H/2, W/2] -> [N, H, W], nearest
    return c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def convert_reference():
    to_rgb(ref[:, 0].view(N, H, W), ref[:, 1].view(N, H, W), ref[:, 2].view(N, H, W))


def convert_i420():
    to_rgb(i420[:, :H * W].view(N, H, W), up(i420[:, H * W:H * W + quarter].view(N, H // 2, W // 2)),
           up(i420[:, H * W + quarter:].view(N, H // 2, W // 2)))


def convert_nv12():
    c = nv12[:, H * W:].view(N, H // 2, W // 2, 2)
    to_rgb(nv12[:, :H * W].view(N, H, W), up(c[..., 0]), up(c[..., 1]))


plane_legs = []
for name, preset, frames, conv in (("reference planes", 0, ref, convert_reference), ("I420", 1, i420, convert_i420),
                                   ("NV12", 3, nv12, convert_nv12)):
    e = create(this, 3, planes=preset)
    assert this.m1v_path_in_use(e) == 1
    same(result(plain(this, e, frames.data_ptr()), name), want_rgb, name)
    assert torch.equal(result(table8(this, e, frames.data_ptr()), name + " table")[2], want_table), f"{name}: tables differ"
    same(result(budget8(this, e, frames.data_ptr()), name + " budget"), want_budget, name + " budget")

    def convert_then_plain(conv=conv):
        conv()
        return other.m1v_encode_device(e_rgb_other, packed.data_ptr(), N, 0, out.data_ptr(), out.numel(), sizes.data_ptr(),
                                       meta.data_ptr(), meta.data_ptr() + 8, None)

    assert convert_then_plain() == 0
    torch.cuda.synchronize()
    assert int(meta[1].item()) == 0
    legs.append((f"{name} step (this | other packed RGB step, same records)", plain(this, e, frames.data_ptr()),
                 plain(other, e_rgb_other, rgb3.data_ptr())))
    legs.append((f"{name} step (this | torch YCbCr->RGB + other packed step; other bytes differ: cost only)",
                 plain(this, e, frames.data_ptr()), convert_then_plain))
    plane_legs.append((name, e, frames))
    if name == "NV12":
        legs.append(("table K=8 (this NV12 | other packed RGB)", table8(this, e, frames.data_ptr()), table8(other, e_rgb_other, rgb3.data_ptr())))
        legs.append(("budget K=8 (this NV12 | other packed RGB)", budget8(this, e, frames.data_ptr()), budget8(other, e_rgb_other, rgb3.data_ptr())))

# ---- samples two bytes apart: the same pictures as packed 4:2:2 (chroma in the even rows; the odd rows' chroma bytes are
#      noise) and as P010 (the sample in each word's high byte; the low bytes are noise) ----
yuy2 = torch.randint(0, 256, (N, H, W // 2, 4), dtype=torch.uint8, device="cuda")
yuy2.view(N, H, W, 2)[..., 0] = i420[:, :H * W].view(N, H, W)
yuy2[:, 0::2, :, 1] = i420[:, H * W:H * W + quarter].view(N, H // 2, W // 2)
yuy2[:, 0::2, :, 3] = i420[:, H * W + quarter:].view(N, H // 2, W // 2)
p010 = torch.randint(0, 256, (N, H * 3 // 2 * W, 2), dtype=torch.uint8, device="cuda")
p010[..., 1] = nv12
torch.cuda.synchronize()
alive += [yuy2, p010]
e_nv12_other = create(other, 3, planes=3) if hasattr(other, "m1v_set_plane_layout") else None
for name, preset, frames in (("YUY2", 0, yuy2), ("P010", 3, p010)):
    e = create(this, 3, samples=preset)
    assert this.m1v_path_in_use(e) == 1
    same(result(plain(this, e, frames.data_ptr()), name), want_rgb, name)
    assert torch.equal(result(table8(this, e, frames.data_ptr()), name + " table")[2], want_table), f"{name}: tables differ"
    same(result(budget8(this, e, frames.data_ptr()), name + " budget"), want_budget, name + " budget")
    legs.append((f"{name} step (this | other packed RGB step, same records)", plain(this, e, frames.data_ptr()),
                 plain(other, e_rgb_other, rgb3.data_ptr())))
    if e_nv12_other is not None:
        legs.append((f"{name} step (this | other NV12 step, same records)", plain(this, e, frames.data_ptr()),
                     plain(other, e_nv12_other, nv12.data_ptr())))
    plane_legs.append((name, e, frames))

if a.only:
    legs = [leg for leg in legs if any(text in leg[0] for text in a.only.split(","))]
    plane_legs = [leg for leg in plane_legs if any(text in leg[0] for text in a.only.split(","))]
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
print(f"{N} x {W}x{H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); "
      "records, sizes, K = 8 tables and budget encodes equal on every plane path; device: " + torch.cuda.get_device_name(0))
for name, _, _ in legs:
    t, o = (statistics.median(res[(name, side)]) * 1e6 for side in (0, 1))
    print(f"{name}\n    left {t:8.1f}  right {o:8.1f}  left/right {t / o:6.3f}   rounds: "
          + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 0)]) + " | " + " ".join(f"{x * 1e6:.1f}" for x in res[(name, 1)]))


# ---- the encode kernel alone (m1v_profile_*): the producer's launches of back-to-back steps, after the settle ----
def kernel_us(L, h, ptr):
    go = plain(L, h, ptr)
    for _ in range(a.settle):
        assert go() == 0
    torch.cuda.synchronize()
    L.m1v_profile_enable(h, 1)
    for _ in range(a.launches):
        assert go() == 0
    torch.cuda.synchronize()
    n, ms = C.c_int(0), C.c_double(0.0)
    assert L.m1v_profile_read(h, C.byref(n), C.byref(ms)) == 0
    L.m1v_profile_enable(h, 0)
    return ms.value * 1e3 / max(n.value, 1)


print("encode kernel alone (m1v_profile_*), us per launch:")
print(f"    other k_encode_tiles on packed RGB  {kernel_us(other, e_rgb_other, rgb3.data_ptr()):8.1f}")
print(f"    this  k_encode_tiles on packed RGB  {kernel_us(this, e_rgb_this, rgb3.data_ptr()):8.1f}")
for name, e, frames in plane_legs:
    print(f"    this  plane / sample kernel on {name:<17s} {kernel_us(this, e, frames.data_ptr()):8.1f}")
for L, h in handles:
    L.m1v_destroy(h)
