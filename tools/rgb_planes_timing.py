#!/usr/bin/env python3
"""RGB plane encodes (m1v_set_rgb_plane_layout) of this tree against another build of the library (the parent commit's, which has
no such layout), side by side in ONE process on one device, in the mould of tools/planes_timing.py.  Per leg and side:
`--settle` untimed back-to-back calls, then `--launches` timed ones with one synchronisation (wall time per call); sides and
legs alternate for `--rounds` rounds and the median round is printed with the ratio left / right.
    legs  plain packed C=3                       this tree | the other library       (identical code: the A/A spread of the run)
          RGB surface step, pitch W * 3          this tree | the other library's packed RGB step       (the surface kernels, for
                                                             comparison with the next leg in the same run)
          RGB planes step                        this tree | the other library's packed RGB step on the interleaved copy of the
                                                             same pictures (same records out)
          the same                               this tree | what a caller of the other library must do: torch's
                                                             permute(0, 2, 3, 1) copy into a packed buffer + its packed step
          table K=8, budget K=8 on RGB planes    this tree | the other library's on packed RGB
    --only <text>: time only the legs whose name contains <text> (several: a comma-separated list); every output is still checked
    usage: rgb_planes_timing.py --other <path to the other libencoder.so> [--w 1920 --h 1080 --n 300]
Every planar output (records, sizes, K = 8 table, budget encode) is compared with the other library's output on the packed copy
before anything is timed.  Also printed: the time of the encode kernel alone under m1v_profile_* for each side."""
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
W, H, N = a.w, a.h, a.n
assert W % 2 == 0


class RgbPlaneLayout(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("r_offset", "g_offset", "b_offset", "row_pitch", "frame_stride")]


def load(path):
    L = C.CDLL(path)
    L.m1v_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 7
    L.m1v_encode_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.m1v_frame_size_table_device.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint8), C.c_int, vp, vp, vp]
    L.m1v_encode_budget_device.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_uint64, vp, vp, vp,
                                           C.c_size_t, vp, vp, vp, vp]
    L.m1v_synth_device.argtypes = [vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.m1v_set_input_layout.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int]
    L.m1v_profile_enable.argtypes = [vp, C.c_int]
    L.m1v_profile_read.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.m1v_destroy.argtypes = [vp]
    L.m1v_path_in_use.argtypes = [vp]
    L.m1v_last_error.restype = C.c_char_p
    if hasattr(L, "m1v_set_rgb_plane_layout"):
        L.m1v_rgb_plane_layout_preset.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(RgbPlaneLayout)]
        L.m1v_set_rgb_plane_layout.argtypes = [vp, C.POINTER(RgbPlaneLayout)]
    return L


this, other = load(os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so")), load(a.other)
handles = []


def create(L, surface=None, rgb_planes=None):
    h = vp()
    assert L.m1v_create(C.byref(h), 0, W, H, 3, a.q, 1, N) == 0, L.m1v_last_error()
    if surface:
        assert L.m1v_set_input_layout(h, *surface) == 0, L.m1v_last_error()
    if rgb_planes is not None:
        lay = RgbPlaneLayout()
        assert L.m1v_rgb_plane_layout_preset(W, H, rgb_planes, C.byref(lay)) == 0, L.m1v_last_error()
        assert L.m1v_set_rgb_plane_layout(h, C.byref(lay)) == 0, L.m1v_last_error()
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


# ---- the pictures: packed synthetic frames, and their planes (a contiguous [N, 3, H, W] tensor) ----
rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
this.m1v_synth_device(rgb.data_ptr(), W * H * 3, N, 504, 0, None)
nchw = rgb.permute(0, 3, 1, 2).contiguous()
packed = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")   # where the caller without planar input copies to
torch.cuda.synchronize()

e_this, e_other = create(this), create(other)
want = result(plain(other, e_other, rgb.data_ptr()), "other plain")
same(result(plain(this, e_this, rgb.data_ptr()), "this plain"), want, "C=3 plain")
want_table = result(table8(other, e_other, rgb.data_ptr()), "other table")[2]
want_budget = result(budget8(other, e_other, rgb.data_ptr()), "other budget")
e_surface = create(this, surface=(W * 3, 0, 0))
same(result(plain(this, e_surface, rgb.data_ptr()), "this surface"), want, "RGB surface")
e_planes = create(this, rgb_planes=0)
assert this.m1v_path_in_use(e_planes) == 1
same(result(plain(this, e_planes, nchw.data_ptr()), "RGB planes"), want, "RGB planes")
assert torch.equal(result(table8(this, e_planes, nchw.data_ptr()), "RGB planes table")[2], want_table), "RGB planes: tables differ"
same(result(budget8(this, e_planes, nchw.data_ptr()), "RGB planes budget"), want_budget, "RGB planes budget")


def permute_then_plain():
    packed.copy_(nchw.permute(0, 2, 3, 1))
    return other.m1v_encode_device(e_other, packed.data_ptr(), N, 0, out.data_ptr(), out.numel(), sizes.data_ptr(),
                                   meta.data_ptr(), meta.data_ptr() + 8, None)


same(result(permute_then_plain, "permute + other plain"), want, "permute + other plain")
assert torch.equal(packed, rgb)

legs = [   # (name, left, right)
    ("C=3 plain packed (this | other)", plain(this, e_this, rgb.data_ptr()), plain(other, e_other, rgb.data_ptr())),
    ("RGB surface step pitch W*3 (this | other packed RGB step, same records)", plain(this, e_surface, rgb.data_ptr()),
     plain(other, e_other, rgb.data_ptr())),
    ("RGB planes step (this | other packed RGB step, same records)", plain(this, e_planes, nchw.data_ptr()),
     plain(other, e_other, rgb.data_ptr())),
    ("RGB planes step (this | torch permute copy + other packed RGB step, same records)", plain(this, e_planes, nchw.data_ptr()),
     permute_then_plain),
    ("table K=8 (this RGB planes | other packed RGB)", table8(this, e_planes, nchw.data_ptr()), table8(other, e_other, rgb.data_ptr())),
    ("budget K=8 (this RGB planes | other packed RGB)", budget8(this, e_planes, nchw.data_ptr()), budget8(other, e_other, rgb.data_ptr())),
]
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
print(f"{N} x {W}x{H} q{a.q}: us per call, median of {a.rounds} rounds ({a.settle} settle + {a.launches} timed); "
      "records, sizes, K = 8 tables and budget encodes equal on the planar path; device: " + torch.cuda.get_device_name(0))
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
print(f"    other k_encode_tiles on packed RGB        {kernel_us(other, e_other, rgb.data_ptr()):8.1f}")
print(f"    this  k_encode_tiles on packed RGB        {kernel_us(this, e_this, rgb.data_ptr()):8.1f}")
print(f"    this  k_encode_surface on packed RGB      {kernel_us(this, e_surface, rgb.data_ptr()):8.1f}")
print(f"    this  k_encode_rgb_planes on the planes   {kernel_us(this, e_planes, nchw.data_ptr()):8.1f}")
for L, h in handles:
    L.m1v_destroy(h)
