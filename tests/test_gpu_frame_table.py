"""GPU tests of the frame table (m1v_set_frame_table; -m gpu): batches whose frames lie at separate device addresses, named by a
device array of one 64-bit address per frame, through every tile-shaped kernel family that takes a layout.

The checkers are the CPU oracles of the layouts' own tests: orc.encode_frame on the packed picture for the surface and RGB plane
layouts, tests/sample_oracle.py on a frame's bytes for the plane and sample layouts.  A scattered batch is a pool of noise into
which each distinct picture is written once, at a base of its own; the table names those bases.  Every comparison is for
equality and every status word is 0.  No test hands the library an address outside a live allocation."""
import ctypes as C

import numpy as np
import pytest

from gpu_calls import _encode, _table
from layout_inputs import FIRST, RESIDUES, _addresses, _check, _picture_of, _RgbPlanes, _Samples, _Surface

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = ((16, 16), (48, 32), (144, 80))     # one macroblock; one partial tile; a 2 x 2 tile grid
BATCHES = (1, 3, 9, 17)                     # up to 8 frames and more: both branches of the workgroup -> (frame, tile) map
QUALITIES = (12, 100)                       # byte staging, halfword staging (noise of amplitude 64: no level reaches 256)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- one layout of each kernel family ---------------------------------------------------------------------------------------


FAMILIES = {"bgra": _Surface(4, 12, "bgr"),     # pitched B,G,R,A surface (k_*_surface, 4-byte pixels)
            "rgb": _Surface(3, 0, "rgb"),        # R,G,B surface with pitch W * 3: how a packed buffer reaches the table
            "nv12": _Samples("nv12"),            # k_*_planes, interleaved chroma
            "i420": _Samples("i420"),            # k_*_planes, planar chroma
            "yuy2": _Samples("yuy2"),            # k_*_step2
            "rgb_planes": _RgbPlanes()}          # k_*_rgb_planes, pitched


# ---- scattered placement ----------------------------------------------------------------------------------------------------


def _scatter(torch, fam, pics, n, W, H, fill_seed=0):
    """The first n frames of a batch (frame f shows pics[_picture_of(f)]) in a pool of noise of fill_seed: every distinct picture
    once, GUARD bytes and more around it, bases of several residues mod 16, unequal gaps, and a memory order that is a permutation
    of the batch's and not ascending.  Returns (pool, [byte offset of frame f's base])."""
    ids = sorted({_picture_of(f) for f in range(n)})
    order = ids[::-1]
    if len(order) >= 3:
        order[0], order[1] = order[1], order[0]
    L = fam.span(W, H)
    where, cursor = {}, GUARD
    for k, p in enumerate(order):
        where[p] = (cursor + 15) // 16 * 16 + RESIDUES[k % len(RESIDUES)]
        cursor = where[p] + L + GUARD + 16 * ((5 * k) % 7)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3000 + fill_seed)
    pool = torch.randint(0, 256, (cursor + GUARD,), dtype=torch.uint8, device="cuda", generator=gen)
    assert pool.data_ptr() % 16 == 0
    for p in ids:
        fam.write(torch, pool, where[p], pics[p], W, H)
    bases = [where[_picture_of(f)] for f in range(n)]
    if n >= 3:
        assert bases[2] == bases[0] and bases != sorted(bases) and len({b % 16 for b in bases}) >= 2 and any(b % 2 for b in bases)
    return pool, bases


_cache = {}


def _expected(orc, name, size, Q, n):
    """17 pictures of that family and size (noise; amplitude 64 at quality 100) and the oracle's records of the batch's first n
    frames as frames 17.., computed once per frame and shared by the tests."""
    W, H = size
    fam = FAMILIES[name]
    if (name, size, Q) not in _cache:
        rng = np.random.default_rng(sum(map(ord, name)) * 1000 + W + H + Q)
        pics = fam.pictures(rng, max(BATCHES), W, H, 64 if Q == 100 else 256)
        for p in pics:
            p.setflags(write=False)
        _cache[(name, size, Q)] = (pics, [])
    pics, recs = _cache[(name, size, Q)]
    while len(recs) < n:
        recs.append(fam.want(orc, pics[_picture_of(len(recs))], W, H, FIRST + len(recs), Q))
    return pics, recs[:n]


def _table_encoder(fam, W, H, Q, n, stride=0):
    enc = fam.encoder(W, H, Q, n, stride)
    before = (enc.path, enc.size_table_fused, enc.scratch_bytes(), enc._input)
    enc.set_frame_table()
    assert enc.frame_table and (enc.path, enc.size_table_fused, enc.scratch_bytes(), enc._input) == before == ("tiles", 1) + before[2:]
    return enc


# ---- 1. the parity matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,name,size", [(i * len(SIZES) + j, name, s) for i, name in enumerate(FAMILIES) for j, s in enumerate(SIZES)])
def test_parity_matrix(torch_cuda, orc, k, name, size):
    """Records and sizes of encode, and the size-table and rd-table rows, of scattered frames at both stagings; the batch size
    rotates so that every family meets batches of 1, 3, 9 and 17."""
    torch = torch_cuda
    W, H = size
    fam = FAMILIES[name]
    for qi, Q in enumerate(QUALITIES):
        n = BATCHES[(k + qi) % 4]
        pics, recs = _expected(orc, name, size, Q, n)
        pool, bases = _scatter(torch, fam, pics, n, W, H, fill_seed=k)
        enc = _table_encoder(fam, W, H, Q, n)
        _check(torch, enc, _addresses(torch, pool, bases), recs)
        enc.close()


# ---- 2. table against stride on the device ----------------------------------------------------------------------------------
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
CANDS5 = (2, 4, 6, 8, 12)


@pytest.mark.parametrize("name", ["bgra", "nv12", "yuy2", "rgb_planes"])
def test_table_equals_stride_on_one_buffer(torch_cuda, name):
    """One contiguous buffer, frames an odd stride apart, and the table of base + f * stride: every call family gives the same
    outputs with the table off, on, and off again, on one encoder."""
    torch = torch_cuda
    W, H, n, first = 144, 80, 9, 40
    fam = FAMILIES[name]
    rng = np.random.default_rng(7 + len(name))
    amps = (256, 64, 16, 128, 32, 8)
    pics = [fam.pictures(rng, 1, W, H, amps[f % len(amps)])[0] for f in range(n)]
    stride = fam.span(W, H) + 37
    pool = torch.randint(0, 256, (2 * GUARD + n * stride,), dtype=torch.uint8, device="cuda")
    for f in range(n):
        fam.write(torch, pool, GUARD + 1 + f * stride, pics[f], W, H)
    batch = fam.view(torch, pool, GUARD + 1, W, H, n, stride)
    table = _addresses(torch, pool, [GUARD + 1 + f * stride for f in range(n)])
    enc = fam.encoder(W, H, 12, n, stride)
    qs = [int(q) for q in np.random.default_rng(3).integers(1, 13, n)]

    def every_call(x):
        st1 = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
        st8 = torch.full((8,), 0x40, dtype=torch.int32, device="cuda")
        probe = enc.frame_sizes(x, quality=qs, status=st1)
        rd = enc.frame_rd_table(x, K8, status=st8)
        enc.flush()
        torch.cuda.synchronize()
        out = {"plain": _encode(torch, enc, x, first), "quality": _encode(torch, enc, x, first, quality=qs),
               "frame_sizes": ([int(v) for v in probe.cpu()], int(st1.cpu()[0])), "size table": _table(torch, enc, x, K8),
               "rd table": ([t.cpu().numpy().tolist() for t in rd], [int(v) for v in st8.cpu()])}
        s = [out["size table"][0][K8.index(c)] for c in CANDS5]
        cap = sorted(v for row in s for v in row)[len(s) * n // 2]
        B = (sum(s[1]) + sum(s[2])) // 2
        r = sorted(s[2])[2]
        out["budget"] = enc.encode_to_budget(x, cap, CANDS5, first_frame_index=first)
        out["batch budget"] = enc.encode_to_batch_budget(x, B, CANDS5, first_frame_index=first)
        out["rd"] = enc.encode_best_in_budget(x, cap, CANDS5, first_frame_index=first)
        out["rd batch"] = enc.encode_best_in_batch_budget(x, B, CANDS5, first_frame_index=first)
        for key, call in (("bitrate", enc.encode_at_bitrate), ("rd bitrate", enc.encode_best_at_bitrate)):
            level = torch.full((1,), 10 ** 6, dtype=torch.int64, device="cuda")
            out[key] = (call(x, r, 2 * r, CANDS5, level, first_frame_index=first), int(level.cpu()[0]))
        return out

    by_stride = every_call(batch)
    assert by_stride["plain"][1] == by_stride["size table"][0][-1] and by_stride["size table"][1] == [0] * 8
    assert len(set(by_stride["budget"][2])) > 1, by_stride["budget"][2]
    layout = enc._input
    enc.set_frame_table()
    assert enc.frame_table and enc._input == layout         # (the frame stride is kept and reported, and unused)
    by_table = every_call(table)
    for key in by_stride:
        assert by_table[key] == by_stride[key], key
    with pytest.raises(AssertionError):
        enc.encode(batch)                                   # while the table is on the frames themselves are refused
    enc.set_frame_table(False)
    assert not enc.frame_table
    with pytest.raises(AssertionError):
        enc.encode(table)
    again = every_call(batch)                               # turning the table off restores stride addressing
    for key in by_stride:
        assert again[key] == by_stride[key], key
    enc.close()


# ---- 3. separate allocations through frames() -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_separately_allocated_tensors_through_frames(torch_cuda, orc, name):
    """A Python list of individually allocated tensors (one of them twice) goes through Mpeg1Encoder.frames and matches the
    oracle; what the layout in force would not take as a batch of one is refused."""
    from ec504_imageencoder_amd import FrameTable
    torch = torch_cuda
    (W, H), Q, n = (48, 32), 12, 9
    fam = FAMILIES[name]
    pics, recs = _expected(orc, name, (W, H), Q, n)
    own = {}
    for p in sorted({_picture_of(f) for f in range(n)}):
        buf = torch.randint(0, 256, ((fam.span(W, H) + 3) // 4 * 4,), dtype=torch.uint8, device="cuda")   # an allocation of its own
        fam.write(torch, buf, 0, pics[p], W, H)
        own[p] = fam.view(torch, buf, 0, W, H)
    tensors = [own[_picture_of(f)] for f in range(n)]
    assert len({t.data_ptr() for t in tensors}) == n - 1
    enc = fam.encoder(W, H, Q, n)
    with pytest.raises(AssertionError):
        enc.encode(enc.frames(tensors))                     # a table needs set_frame_table
    enc.set_frame_table()
    ft = enc.frames(tensors)
    assert isinstance(ft, FrameTable) and ft.shape == (n,) and ft.table.dtype == torch.int64 and ft.table.is_cuda
    assert ft.table.cpu().tolist() == [t.data_ptr() for t in tensors] and all(a is b for a, b in zip(ft.frames, tensors))
    del own, tensors                                        # the table keeps its frames alive
    _check(torch, enc, ft, recs)
    for bad in (torch.zeros(7, dtype=torch.uint8, device="cuda"), ft.frames[0].to(torch.int8), ft.frames[0].cpu()):
        with pytest.raises(AssertionError):
            enc.frames([ft.frames[0], bad])
    with pytest.raises(AssertionError):
        enc.frames([])
    enc.close()


def test_frames_needs_a_layout(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    enc = Mpeg1Encoder(48, 32, 12, "full", max_frames=2)
    with pytest.raises(AssertionError):
        enc.frames([torch.zeros((32, 48, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(EncoderError) as ei:
        enc.set_frame_table()
    assert ei.value.code == _ffi.E_ARG and not enc.frame_table
    enc.close()


# ---- 4. padding and surroundings are never used -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_surroundings_are_never_used(torch_cuda, orc, name):
    """The same pictures at the same places under two fills of everything else in the pool (the guards around each frame, the
    gaps, row padding, the alpha... of the pool's own noise): identical records and tables, the oracle's."""
    torch = torch_cuda
    fam = FAMILIES[name]
    Q, n = 12, 3
    for size in ((48, 32), (144, 80)):
        W, H = size
        pics, recs = _expected(orc, name, size, Q, n)
        results = []
        for fill in (1, 2):
            pool, bases = _scatter(torch, fam, pics, n, W, H, fill_seed=40 + fill)
            table = _addresses(torch, pool, bases)
            enc = _table_encoder(fam, W, H, Q, n)
            rd = enc.frame_rd_table(table, (5, Q))
            torch.cuda.synchronize()
            results.append((_encode(torch, enc, table, FIRST), _table(torch, enc, table, (5, Q)), [t.cpu().numpy().tolist() for t in rd]))
            enc.close()
        assert results[0] == results[1]
        assert results[0][0] == (b"".join(recs), [len(r) for r in recs])


# ---- 5. the table is read on the stream -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bgra", "i420", "rgb_planes"])
def test_the_table_is_read_on_the_stream(torch_cuda, orc, name):
    """The table holds frame 0's address in every entry until a device-to-device copy, queued on the current stream directly in
    front of each call with no synchronisation between them, writes the real addresses: the records are the oracle's."""
    torch = torch_cuda
    (W, H), Q, n = (144, 80), 12, 9
    fam = FAMILIES[name]
    pics, recs = _expected(orc, name, (W, H), Q, n)
    pool, bases = _scatter(torch, fam, pics, n, W, H, fill_seed=5)
    real = _addresses(torch, pool, bases)
    stale = _addresses(torch, pool, [bases[0]] * n)
    enc = _table_encoder(fam, W, H, Q, n)
    table = stale.clone()
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    table.copy_(real)
    out, sizes, meta = enc.encode(table, FIRST, out=out)
    table.copy_(stale)
    table.copy_(real)
    rows = enc.frame_size_table(table, (Q,), status=st)
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status & 0xFFFFFFFF == 0 and int(st.cpu()[0]) == 0
    assert [int(s) for s in sizes[:n].cpu()] == [len(r) for r in recs] == rows.cpu().numpy().tolist()[0]
    assert out[:total].cpu().numpy().tobytes() == b"".join(recs)
    enc.close()


# ---- 6. the flag's life cycle -----------------------------------------------------------------------------------------------
def _setters(W, H):
    """name -> (sets a layout of that kind, restores the default through that setter, a call of it that is an argument error)."""
    from ec504_imageencoder_amd import plane_layout_preset, rgb_plane_layout_preset, sample_layout_preset
    return {
        "input": (lambda e: e.set_input_layout(W * 3 + 4), lambda e: e.set_input_layout(), lambda e: e.set_input_layout(1)),
        "plane": (lambda e: e.set_plane_layout("nv12"), lambda e: e.set_plane_layout(None),
                  lambda e: e.set_plane_layout(dict(plane_layout_preset(W, H, "nv12"), y_pitch=1))),
        "sample": (lambda e: e.set_sample_layout("yuy2"), lambda e: e.set_sample_layout(None),
                   lambda e: e.set_sample_layout(dict(sample_layout_preset(W, H, "yuy2"), y_pitch=1))),
        "rgb_plane": (lambda e: e.set_rgb_plane_layout("bgr"), lambda e: e.set_rgb_plane_layout(None),
                      lambda e: e.set_rgb_plane_layout(dict(rgb_plane_layout_preset(W, H, "bgr"), row_pitch=1))),
    }


def test_every_layout_setter_clears_the_flag_and_a_failed_one_keeps_it(torch_cuda, orc):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n = 48, 32, 3
    setters = _setters(W, H)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    assert enc.frame_table is False and _ffi.lib().m1v_frame_table(enc._h) == 0
    with pytest.raises(EncoderError) as ei:                 # the default packed layout: refused, and the message names the way
        enc.set_frame_table()
    assert ei.value.code == _ffi.E_ARG and "m1v_set_input_layout" in str(ei.value) and not enc.frame_table
    enc.set_frame_table(False)                              # (turning it off is always accepted)
    for first, (set_first, _, _) in setters.items():
        for second, (set_second, restore, bad) in setters.items():
            set_first(enc)
            assert not enc.frame_table
            enc.set_frame_table()
            enc.set_frame_table()                           # (idempotent)
            assert enc.frame_table and _ffi.lib().m1v_frame_table(enc._h) == 1
            with pytest.raises(EncoderError) as ei:         # an argument error of any setter leaves the flag as it was
                bad(enc)
            assert ei.value.code == _ffi.E_ARG and enc.frame_table, (first, second)
            set_second(enc)                                 # a fresh record: the table is off
            assert not enc.frame_table, (first, second)
            enc.set_frame_table()
            restore(enc)                                    # ... and so does the setter that restores the default
            assert not enc.frame_table and enc.input_layout == (0, 0, "rgb"), (first, second)
    # after all that a table encode is exact
    fam = FAMILIES["rgb_planes"]
    pics, recs = _expected(orc, "rgb_planes", (W, H), 12, n)
    pool, bases = _scatter(torch, fam, pics, n, W, H)
    P = fam.pitch(W)
    enc.set_rgb_plane_layout(dict(r_offset=0, g_offset=H * P, b_offset=2 * H * P, row_pitch=P, frame_stride=3 * H * P))
    enc.set_frame_table()
    _check(torch, enc, _addresses(torch, pool, bases), recs)
    enc.close()


def test_an_injected_allocation_failure_keeps_the_flag(torch_cuda, orc):
    """m1v_debug_fail_alloc (EC504_DEBUG_HOOKS=1) inside a layout setter of a 4-channel encoder, whose default plan needs scratch
    of another size than the tile plan: M1V_E_HIP, the layout and the table stay in force and the next table encode is exact."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    torch = torch_cuda
    W, H, n = 352, 288, 3
    fam = FAMILIES["bgra"]
    rng = np.random.default_rng(58)
    pics = fam.pictures(rng, n, W, H)
    recs = [fam.want(orc, pics[_picture_of(f)], W, H, FIRST + f, 12) for f in range(n)]
    pool, bases = _scatter(torch, fam, pics, n, W, H, fill_seed=6)
    table = _addresses(torch, pool, bases)
    enc = _table_encoder(fam, W, H, 12, n)
    before = (enc.input_layout, enc.path, enc.scratch_bytes())
    _ffi.lib().m1v_debug_fail_alloc(1)
    try:
        with pytest.raises(EncoderError) as ei:
            enc.set_input_layout()
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_alloc(0)
    assert enc.frame_table and (enc.input_layout, enc.path, enc.scratch_bytes()) == before
    _check(torch, enc, table, recs)
    enc.set_input_layout()
    assert not enc.frame_table and enc.path == "runs"
    enc.close()


def test_a_misaligned_table_is_an_argument_error(torch_cuda, orc):
    """A table pointer that is not 8-byte aligned: M1V_E_ARG from the encode and the table calls before anything is launched (the
    outputs keep their fill), and the next call on the encoder is exact.  The pointer lies inside the table's own allocation."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    (W, H), Q, n = (48, 32), 12, 3
    fam = FAMILIES["nv12"]
    pics, recs = _expected(orc, "nv12", (W, H), Q, n)
    pool, bases = _scatter(torch, fam, pics, n, W, H, fill_seed=9)
    room = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    room[:n].copy_(_addresses(torch, pool, bases))
    enc = _table_encoder(fam, W, H, Q, n)
    L = _ffi.lib()
    out = torch.full((enc.frame_bound * n,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    meta = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qs = (C.c_uint8 * 2)(5, Q)
    for off in (1, 4, 7):
        p = C.c_void_p(room.data_ptr() + off)
        assert L.m1v_encode_device(enc._h, p, n, FIRST, C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(sizes.data_ptr()),
                                   C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8), stream) == _ffi.E_ARG
        assert "8-byte aligned" in _ffi.last_error()
        assert L.m1v_frame_size_table_device(enc._h, p, n, qs, 2, C.c_void_p(sizes.data_ptr()), None, stream) == _ffi.E_ARG
        assert L.m1v_frame_sizes_device(enc._h, p, n, None, C.c_void_p(sizes.data_ptr()), None, stream) == _ffi.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((sizes == -1).all()) and bool((meta == -1).all())
    _check(torch, enc, room[:n], recs)
    enc.close()


# ---- 7. pipelined mode and delivery -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bgra", "nv12"])
def test_pipelined_mode_and_host_delivery(torch_cuda, orc, name):
    """Two batches of tables in pipelined mode, complete behind one flush; then one HostDelivery step and its flush on a table
    that frames() made."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    (W, H), Q, n = (144, 80), 12, 9
    fam = FAMILIES[name]
    pics, recs = _expected(orc, name, (W, H), Q, n)
    pool, bases = _scatter(torch, fam, pics, n, W, H, fill_seed=11)
    enc = _table_encoder(fam, W, H, Q, n)
    enc.set_pipelined(True)
    assert enc.frame_table and enc.path == "tiles"
    whole, part = _addresses(torch, pool, bases), _addresses(torch, pool, bases[4:7])
    outs = [torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
    a = enc.encode(whole, FIRST, out=outs[0])
    b = enc.encode(part, FIRST + 4, out=outs[1])
    enc.flush()
    torch.cuda.synchronize()
    for (out, sizes, meta), want in ((a, recs), (b, recs[4:7])):
        total, status = (int(x) for x in meta.cpu())
        assert status & 0xFFFFFFFF == 0 and [int(s) for s in sizes[:len(want)].cpu()] == [len(r) for r in want]
        assert out[:total].cpu().numpy().tobytes() == b"".join(want)
    enc.set_pipelined(False)
    assert enc.frame_table
    ft = enc.frames([fam.view(torch, pool, base, W, H) for base in bases])
    hd = HostDelivery(enc, n)
    hd.step(ft, FIRST)
    assert hd.last is None
    del ft                                                  # (the delivery keeps the pending batch's input alive)
    hd.fence()
    assert bytes(hd.result().numpy()) == b"".join(recs) and [int(v) for v in hd.frame_sizes(n)] == [len(r) for r in recs]
    hd.close()
    enc.close()
