"""The layout kind x call matrix (-m gpu): what every entry point that asks "which input layout is in force?" answers in every
state an encoder can be in, compared for equality with tests/golden/layout_matrix.json.

States: a 48x32 FULL-mode encoder (3 strips x 2 macroblock rows: a chroma row pair and a last strip) with packed input, a
surface layout, a plane layout, a sample layout with y_step 2, an RGB plane layout, a float plane layout and a float pixel
layout, and the 4-channel encoder with packed input and a surface layout.  In each: every getter, both table setters, the
packed-only calls, a d_rgb one byte off alignment, both to-bytes calls, every setter with each of its refusals, and from Python
_check_input with tensors of a wrong dtype, rank, row stride and frame stride, frames() and plane_frames().  Beside the states:
every setter with a good argument on the 3-channel, 4-channel, odd-width and hook-forced encoders, the presets, and a null
encoder.  Per case the golden holds the return code and the m1v_last_error() text, or the exception's type and message.

No case launches an encode kernel: each is refused in front of a launch, reads state, or is an empty batch.

The golden is a record of the commit named in its header, not of the tree under test: EC504_LAYOUT_MATRIX_RECORD=<commit> in
the environment makes this module write the file (on a checkout of that commit) and compare nothing."""
import ctypes as C
import json
import os

import pytest

import golden_io

pytestmark = pytest.mark.gpu

GOLDEN = "layout_matrix.json"
RECORD = os.environ.get("EC504_LAYOUT_MATRIX_RECORD")
W, H, N = 48, 32, 2
STATES = ("packed", "surface", "planes", "samples2", "rgb_planes", "float_planes", "float_pixels", "packed4", "surface4")
SECTIONS = STATES + ("good_rgb", "good_rgba", "good_odd", "good_hooked", "presets", "null_encoder")
SETTERS = ("m1v_set_input_layout", "m1v_set_plane_layout", "m1v_set_sample_layout", "m1v_set_rgb_plane_layout",
           "m1v_set_float_plane_layout", "m1v_set_float_pixel_layout")
BIG = 2 ** 32


def _structs():
    from ec504_imageencoder_amd import _ffi
    return {"plane": _ffi.PlaneLayout, "sample": _ffi.SampleLayout, "rgb_plane": _ffi.RgbPlaneLayout,
            "float_plane": _ffi.FloatPlaneLayout, "float_pixel": _ffi.FloatPixelLayout}


def _rc(L, rc):
    """[return code, the reason where the call failed]"""
    return [int(rc), L.m1v_last_error().decode() if rc < 0 else ""]


def _set(L, h, name, args):
    """The C setter `name`: args = the three arguments of m1v_set_input_layout, a dict of the layout struct's fields, or None."""
    if name == "m1v_set_input_layout":
        return _rc(L, L.m1v_set_input_layout(h, *args))
    struct = _structs()[name[len("m1v_set_"):-len("_layout")]]
    return _rc(L, getattr(L, name)(h, C.byref(struct(**args)) if args is not None else None))


def _snapshot(L, h):
    """Every getter, the table modes, the path and the size table's kind."""
    pitch, stride, order = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    rc = L.m1v_input_layout(h, C.byref(pitch), C.byref(stride), C.byref(order))
    out = {"m1v_input_layout": _rc(L, rc) + ([pitch.value, stride.value, order.value] if rc == 0 else [])}
    for kind, struct in _structs().items():
        name, c = f"m1v_{kind}_layout_in_force", struct()
        rc = getattr(L, name)(h, C.byref(c))
        out[name] = _rc(L, rc) + ([c.as_dict()] if rc == 1 else [])
    for name in ("m1v_frame_table", "m1v_plane_table", "m1v_path_in_use", "m1v_size_table_fused"):
        out[name] = int(getattr(L, name)(h))
    return out


def _good(w, h, channels):
    """One argument per setter that a 3-channel encoder of even width w accepts."""
    from ec504_imageencoder_amd import (float_pixel_layout_preset, float_plane_layout_preset, plane_layout_preset,
                                        rgb_plane_layout_preset, sample_layout_preset)
    return {"m1v_set_input_layout": (w * channels + 16, 0, 1),
            "m1v_set_plane_layout": plane_layout_preset(w, h, "nv12"),
            "m1v_set_sample_layout": sample_layout_preset(w, h, "yuy2"),
            "m1v_set_rgb_plane_layout": rgb_plane_layout_preset(w, h, "gbr"),
            "m1v_set_float_plane_layout": float_plane_layout_preset(w, h, "rgb", "float16", "unit"),
            "m1v_set_float_pixel_layout": float_pixel_layout_preset(w, h, 4, "float32", "bgr", "byte")}


def _refusals(enc):
    """(setter, label, argument): one argument per refusal of every setter, for a 3-channel encoder in the order of the checks."""
    from ec504_imageencoder_amd.encoder import (float_pixel_layout_preset, float_plane_layout_preset, plane_layout_extent,
                                                plane_layout_preset, rgb_plane_layout_preset, sample_layout_preset)
    Cn = enc.channels
    row, P = W * Cn, W * Cn + 16
    cases = [("m1v_set_input_layout", "order", (P, 0, 2)), ("m1v_set_input_layout", "order_negative", (P, 0, -1)),
             ("m1v_set_input_layout", "pitch_below_row", (row - 1, 0, 0)), ("m1v_set_input_layout", "pitch_4g", (BIG, 0, 0)),
             ("m1v_set_input_layout", "window_4g", (BIG // (H - 1), 0, 0)),
             ("m1v_set_input_layout", "stride_below_window", (P, (H - 1) * P + row - 1, 0))]
    pl = plane_layout_preset(W, H, "nv12")
    extent = plane_layout_extent(dict(pl, y_step=1), enc.strips, enc.mb_rows)
    cases += [("m1v_set_plane_layout", k, dict(pl, **v)) for k, v in (
        ("c_step_3", dict(c_step=3)), ("no_stride", dict(frame_stride=0)), ("luma_pitch_below", dict(y_pitch=W - 1)),
        ("chroma_pitch_below", dict(c_pitch=W - 1)), ("pitch_4g", dict(y_pitch=BIG)), ("offset_4g", dict(cr_offset=BIG)),
        ("extent_4g", dict(y_pitch=2 ** 31)), ("stride_below_planes", dict(frame_stride=extent - 1)))]
    sl = sample_layout_preset(W, H, "yuy2")
    extent = plane_layout_extent(sl, enc.strips, enc.mb_rows)
    cases += [("m1v_set_sample_layout", k, dict(sl, **v)) for k, v in (
        ("steps_2_2", dict(c_step=2)), ("steps_3_4", dict(y_step=3)), ("steps_1_4", dict(y_step=1)),
        ("chroma_apart", dict(cb_offset=0, cr_offset=4)), ("no_stride", dict(frame_stride=0)),
        ("luma_pitch_below", dict(y_pitch=2 * W - 1)), ("chroma_pitch_below", dict(c_pitch=2 * W - 1)),
        ("pitch_4g", dict(c_pitch=BIG)), ("offset_4g", dict(y_offset=BIG)), ("extent_4g", dict(y_pitch=2 ** 31)),
        ("stride_below_planes", dict(frame_stride=extent - 1)))]
    rp = rgb_plane_layout_preset(W, H, "gbr")
    cases += [("m1v_set_rgb_plane_layout", k, dict(rp, **v)) for k, v in (
        ("pitch_below_width", dict(row_pitch=W - 1)), ("pitch_4g", dict(row_pitch=BIG)), ("offset_4g", dict(b_offset=BIG)),
        ("extent_4g", dict(row_pitch=BIG // (H - 1))), ("planes_share", dict(g_offset=rp["r_offset"] + 1)),
        ("planes_share_rows", dict(g_offset=rp["r_offset"] + W - 1, row_pitch=2 * W)),
        ("stride_below_planes", dict(frame_stride=rp["frame_stride"] - 1)))]
    for dtype, S in (("float16", 2), ("float32", 4)):
        fl = float_plane_layout_preset(W, H, "rgb", dtype, "unit")
        cases += [("m1v_set_float_plane_layout", f"{dtype}_{k}", dict(fl, **v)) for k, v in (
            ("sample", dict(sample=3)), ("sample_negative", dict(sample=-1)), ("range", dict(range=2)),
            ("sample_and_range", dict(sample=7, range=7)), ("offset_unaligned", dict(g_offset=fl["g_offset"] + S // 2)),
            ("pitch_unaligned", dict(row_pitch=fl["row_pitch"] + 1)), ("stride_unaligned", dict(frame_stride=fl["frame_stride"] + 1)),
            ("pitch_below_row", dict(row_pitch=(W - 1) * S)), ("pitch_4g", dict(row_pitch=BIG)), ("offset_4g", dict(b_offset=BIG)),
            ("planes_share", dict(g_offset=fl["r_offset"] + S)), ("stride_below_planes", dict(frame_stride=fl["frame_stride"] - S)))]
        fx = float_pixel_layout_preset(W, H, 4, dtype, "bgr", "byte")
        step, pitch = fx["pixel_step"], fx["row_pitch"]
        cases += [("m1v_set_float_pixel_layout", f"{dtype}_{k}", dict(fx, **v)) for k, v in (
            ("order", dict(order=2)), ("sample", dict(sample=3)), ("range", dict(range=-1)), ("order_and_sample", dict(order=5, sample=5)),
            ("step_one_sample", dict(pixel_step=S)), ("step_5_samples", dict(pixel_step=5 * S)), ("step_0", dict(pixel_step=0)),
            ("pitch_unaligned", dict(row_pitch=pitch + 1)), ("stride_unaligned", dict(frame_stride=fx["frame_stride"] + S // 2)),
            ("pitch_below_row", dict(row_pitch=W * step - S)), ("pitch_4g", dict(row_pitch=BIG)),
            ("rows_4g", dict(row_pitch=BIG // (H - 1) // S * S)), ("stride_below_rows", dict(frame_stride=(H - 1) * pitch + W * step - S)))]
    return cases


def _establish(enc, state):
    from ec504_imageencoder_amd import float_pixel_layout_preset, float_plane_layout_preset
    if state in ("surface", "surface4"):
        enc.set_input_layout(W * enc.channels + 16, 0, "bgr" if state == "surface" else "rgb")
    elif state == "planes":
        enc.set_plane_layout("nv12")
    elif state == "samples2":
        enc.set_sample_layout("yuy2")
    elif state == "rgb_planes":
        enc.set_rgb_plane_layout("gbr")
    elif state == "float_planes":
        enc.set_float_plane_layout(float_plane_layout_preset(W, H, "rgb", "float16", "unit"))
    elif state == "float_pixels":
        enc.set_float_pixel_layout(float_pixel_layout_preset(W, H, 4, "float32", "bgr", "byte"))


def _right_tensor(torch, state):
    """(dtype, shape, strides in elements, index of the row stride) of a batch the state's layout takes."""
    Cn = 4 if state.endswith("4") else 3
    if state in ("packed", "packed4"):
        return torch.uint8, (N, H, W, Cn), (H * W * Cn, W * Cn, Cn, 1), 1
    if state in ("surface", "surface4"):
        P = W * Cn + 16
        return torch.uint8, (N, H, W, Cn), (H * P, P, Cn, 1), 1
    if state in ("planes", "samples2"):
        L = W * H * 3 // 2 if state == "planes" else 2 * W * H
        return torch.uint8, (N, L), (L, 1), 1
    if state in ("rgb_planes", "float_planes"):
        return (torch.uint8 if state == "rgb_planes" else torch.float16), (N, 3, H, W), (3 * H * W, H * W, W, 1), 2
    return torch.float32, (N, H, W, 4), (H * W * 4, W * 4, 4, 1), 1


def _view(torch, dtype, shape, strides):
    elements = sum((d - 1) * s for d, s in zip(shape, strides)) + 1
    return torch.empty(elements + 64, dtype=dtype, device="cuda").as_strided(shape, strides)


def _raised(fn):
    """"ok" and what fn returned, or the exception's type and message."""
    try:
        got = fn()
    except Exception as e:  # noqa: BLE001 (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return ["ok", list(got.shape) if hasattr(got, "shape") else None]


def _python_cases(torch, enc, state):
    dtype, shape, strides, row = _right_tensor(torch, state)
    bump = lambda i, by: tuple(s + by if k == i else s for k, s in enumerate(strides))  # noqa: E731
    tensors = {"right": _view(torch, dtype, shape, strides),
               "wrong_dtype": _view(torch, torch.float16 if dtype == torch.uint8 else torch.uint8, shape, strides),
               "other_float": _view(torch, torch.bfloat16, shape, strides),
               "wrong_rank": _view(torch, dtype, shape[1:], strides[1:]),
               "wrong_row_stride": _view(torch, dtype, shape, bump(row, 8)),
               "wrong_frame_stride": _view(torch, dtype, shape, bump(0, 64)),
               "on_the_host": torch.empty(shape, dtype=dtype)}
    out = {k: _raised(lambda t=t: enc._check_input(t)) for k, t in tensors.items()}
    right = tensors["right"]
    out["frames"] = _raised(lambda: enc.frames([right[0], right[1]]))
    flat = [tuple(torch.empty(4096, dtype=torch.uint8, device="cuda") for _ in range(3)) for _ in range(N)]
    out["plane_frames"] = _raised(lambda: enc.plane_frames(flat))
    out["float_planes_to_bytes"] = _raised(lambda: enc.float_planes_to_bytes(right[:0]))
    out["float_pixels_to_bytes"] = _raised(lambda: enc.float_pixels_to_bytes(right[:0]))
    return out


def _state_cases(torch, L, enc, state, buf):
    """Everything asked of `enc` in one state.  buf: 64 device bytes at a 256-byte boundary that no case reads or writes."""
    h = enc._h
    at, off = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 1)
    host = (C.c_uint8 * 64)()
    out = {"before": _snapshot(L, h)}

    def encode_off_alignment():
        return _rc(L, L.m1v_encode_device(h, off, 0, 0, at, 64, None, None, None, None))

    out["encode_off_alignment"] = encode_off_alignment()
    for table in ("m1v_set_frame_table", "m1v_set_plane_table"):
        on = _rc(L, getattr(L, table)(h, 1))
        out[table] = {"on": on, "tables": [int(L.m1v_frame_table(h)), int(L.m1v_plane_table(h))],
                      "encode_off_alignment": encode_off_alignment(),
                      "encode_aligned": _rc(L, L.m1v_encode_device(h, at, 0, 0, at, 64, None, None, None, None)),
                      "off": _rc(L, getattr(L, table)(h, 0)), "tables_off": [int(L.m1v_frame_table(h)), int(L.m1v_plane_table(h))]}
    out["m1v_debug_set_path"] = {"runs": _rc(L, L.m1v_debug_set_path(h, 0)), "path": int(L.m1v_path_in_use(h)),
                                 "auto": _rc(L, L.m1v_debug_set_path(h, -1))}
    out["m1v_debug_set_input_mode"] = {"bytes": _rc(L, L.m1v_debug_set_input_mode(h, 0)), "path": int(L.m1v_path_in_use(h)),
                                       "auto": _rc(L, L.m1v_debug_set_input_mode(h, -1))}
    out["m1v_convert_device"] = _rc(L, L.m1v_convert_device(h, at, 0, at, None))
    out["m1v_coefficients_device"] = _rc(L, L.m1v_coefficients_device(h, at, 0, at, None))
    out["m1v_convert_host"] = _rc(L, L.m1v_convert_host(h, host, 0, host))
    out["m1v_encode_host"] = _rc(L, L.m1v_encode_host(h, host, 0, 0, host, 64, None))
    for name in ("m1v_float_planes_to_bytes_device", "m1v_float_pixels_to_bytes_device"):
        fn = getattr(L, name)
        out[name] = {"empty": _rc(L, fn(h, at, 0, at, None)), "off_alignment": _rc(L, fn(h, off, 0, at, None)),
                     "two_bytes_off": _rc(L, fn(h, C.c_void_p(buf.data_ptr() + 2), 0, at, None)),
                     "negative": _rc(L, fn(h, at, -1, at, None)), "null_frames": _rc(L, fn(h, None, 1, at, None)),
                     "null_bytes": _rc(L, fn(h, at, 1, None, None))}
    out["setters"] = {f"{name}:{label}": _set(L, h, name, args) for name, label, args in _refusals(enc)}
    out["python"] = _python_cases(torch, enc, state)
    out["after"] = _snapshot(L, h)
    return out


def _good_cases(L, enc, w):
    """Every setter with an argument that a 3-channel encoder of even width w accepts, then with none; the state after each."""
    h, out = enc._h, {}
    for name, args in _good(w, H, enc.channels).items():
        out[name] = {"set": _set(L, h, name, args), "then": _snapshot(L, h),
                     "reset": _set(L, h, name, None if name != "m1v_set_input_layout" else (0, 0, 0)), "back": _snapshot(L, h)}
    return out


def _preset_cases(L):
    S = _structs()
    out = {}

    def run(name, struct, *args):
        c = S[struct]()
        rc = getattr(L, name)(*args, C.byref(c))
        out[f"{name}{args}"] = _rc(L, rc) + ([c.as_dict()] if rc == 0 else [])
        out[f"{name}{args} null"] = _rc(L, getattr(L, name)(*args, None))

    for args in ((W, H, 3), (W, H, 5), (W, H, -1), (0, H, 1), (W + 1, H, 1), (W + 1, H, 0)):
        run("m1v_plane_layout_preset", "plane", *args)
    for args in ((W, H, 3), (W, H, 4), (W, -1, 0), (W, H + 1, 0)):
        run("m1v_sample_layout_preset", "sample", *args)
    for args in ((W, H, 2), (W, H, 3), (0, 0, 0)):
        run("m1v_rgb_plane_layout_preset", "rgb_plane", *args)
    for args in ((W, H, 1, 0, 0), (W, H, 2, 1, 1), (W, H, 0, 2, 0), (W, H, 0, 3, 0), (W, H, 0, -1, 0), (W, H, 0, 0, 2), (W, H, 0, 3, 2),
                 (W, H, 3, 0, 0), (0, H, 0, 0, 0), (0, H, 3, 3, 3)):
        run("m1v_float_plane_layout_preset", "float_plane", *args)
    for args in ((W, H, 3, 0, 0, 0), (W, H, 4, 1, 1, 1), (W, H, 4, 0, 2, 0), (W, H, 5, 0, 0, 0), (W, H, 3, 2, 0, 0), (W, H, 3, 0, 3, 0),
                 (W, H, 3, 0, 0, 2), (W, H, 3, 0, 3, 2), (W, 0, 3, 0, 0, 0), (W, H, 2, 2, 3, 2)):
        run("m1v_float_pixel_layout_preset", "float_pixel", *args)
    return out


def _null_cases(L, buf):
    at = C.c_void_p(buf.data_ptr())
    S = _structs()
    out = {name: _set(L, None, name, args) for name, args in _good(W, H, 3).items()}
    out.update({f"{name} null layout": _set(L, None, name, None) for name in SETTERS[1:]})
    for kind, struct in S.items():
        out[f"m1v_{kind}_layout_in_force"] = _rc(L, getattr(L, f"m1v_{kind}_layout_in_force")(None, C.byref(struct())))
    out["m1v_input_layout"] = _rc(L, L.m1v_input_layout(None, None, None, None))
    for name in ("m1v_set_frame_table", "m1v_set_plane_table", "m1v_debug_set_path", "m1v_debug_set_input_mode"):
        out[name] = _rc(L, getattr(L, name)(None, 1))
    for name in ("m1v_float_planes_to_bytes_device", "m1v_float_pixels_to_bytes_device", "m1v_convert_device", "m1v_coefficients_device"):
        out[name] = _rc(L, getattr(L, name)(None, at, 0, at, None))
    out["m1v_encode_device"] = _rc(L, L.m1v_encode_device(None, at, 0, 0, at, 64, None, None, None, None))
    return out


@pytest.fixture(scope="module")
def matrix():
    """Every section of the matrix, asked once of this tree's library; what JSON makes of it (lists for tuples)."""
    import torch
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    assert torch.cuda.is_available()
    L = _ffi.lib()
    buf = torch.empty(64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    got = {}
    for state in STATES:
        enc = Mpeg1Encoder(W, H, 12, "full", channels=4 if state.endswith("4") else 3, max_frames=N)
        _establish(enc, state)
        got[state] = _state_cases(torch, L, enc, state, buf)
        enc.close()
    for section, width, channels, hooked in (("good_rgb", W, 3, False), ("good_rgba", W, 4, False), ("good_odd", W - 1, 3, False),
                                             ("good_hooked", W, 3, True)):
        enc = Mpeg1Encoder(width, H, 12, "full", channels=channels, max_frames=N)
        if hooked:
            enc.debug_set_path("runs")
        got[section] = _good_cases(L, enc, W)
        enc.close()
    got["presets"] = _preset_cases(L)
    got["null_encoder"] = _null_cases(L, buf)
    torch.cuda.synchronize()
    got = json.loads(json.dumps(got))
    if RECORD:
        header = {"recorded_on_commit": RECORD, "what": "tests/test_gpu_layout_matrix.py: the layout kind x call matrix of that commit",
                  "encoder": f"{W}x{H} FULL, max_frames {N}, quality 12"}
        with open(os.path.join(golden_io.GOLDEN, GOLDEN), "w") as f:
            json.dump({"header": header, "sections": got}, f, indent=1, sort_keys=True)
            f.write("\n")
    return got


@pytest.mark.parametrize("section", SECTIONS)
def test_layout_matrix(matrix, section):
    """Case by case: the return code and reason, or the exception, that the recorded commit gave."""
    if RECORD:
        return
    want, got = golden_io.load_json(GOLDEN)["sections"][section], matrix[section]

    def differing(a, b, path=""):
        if isinstance(a, dict) and isinstance(b, dict):
            return [d for k in sorted(set(a) | set(b)) for d in
                    (differing(a[k], b[k], f"{path}/{k}") if k in a and k in b else [f"{path}/{k}: only in {'the golden' if k in a else 'this tree'}"])]
        return [] if a == b else [f"{path}: the golden has {a!r}, this tree {b!r}"]

    assert differing(want, got) == []


def test_the_golden_names_the_commit_it_records(matrix):
    golden = golden_io.load_json(GOLDEN)
    assert len(golden["header"]["recorded_on_commit"]) >= 7 and sorted(golden["sections"]) == sorted(SECTIONS)
