"""GPU tests of the plane table (m1v_set_plane_table; -m gpu): batches whose frames' planes lie at separate device addresses, named
by a device array of three 64-bit addresses per frame (Y, Cb, Cr or R, G, B), through the kp_* kernels.

The checkers are the CPU oracles of the layouts' own tests: tests/sample_oracle.py on the virtual contiguous frame made of the same
planes under the preset layout, orc.encode_frame on the interleaved picture for planes of R, G and B.  A plane is placed by
writing the samples the definition addresses, and nothing else, into a pool of noise: everything else inside the range the read
contract allows from the plane's pointer, and around it, is the pool's noise.  Every comparison is for equality and every status
word is 0.  No test hands the library an address whose range [P, P + E_p) leaves a live allocation."""
import ctypes as C

import numpy as np
import pytest

from gpu_calls import _encode, _table
from layout_inputs import SEPARATE, _blocks, _check, _device_table, _picture_of, _Rgb, _Ycc

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = ((16, 16), (48, 32), (144, 80))     # one macroblock (64-byte chroma planes); 3 strips: the odd-strip unit; a 2 x 2 tile grid
BATCHES = (1, 3, 9, 17)                     # up to 8 frames and more: both branches of the workgroup -> (frame, tile) map
QUALITIES = (12, 100)                       # byte staging, halfword staging (noise of amplitude 64: no level reaches 256)
RESIDUES = (1, 6, 11, 0, 7, 13, 4, 15)      # a block base's address mod 16, slot by slot
FIRST = 17


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- the families: the layout the encoder is given, the virtual frame the oracle reads, and how the planes are grouped ------------


FAMILIES = {"i420": _Ycc("i420", SEPARATE),
            "yv12": _Ycc("yv12", SEPARATE),                                      # the offsets are swapped, not the pointers
            "nv12": _Ycc("nv12", (((0, 0),), ((1, 0), (2, 0)))),                 # both chroma entries hold the UV pointer, offsets 0 and 1
            "nv12_plus1": _Ycc("nv12", (((0, 0),), ((1, 0), (2, 1))), (0, 0)),   # [f][2] = [f][1] + 1, both offsets 0
            "reference": _Ycc("reference", SEPARATE),                            # full-resolution chroma planes, c_pitch = W / 2
            "rgb_planes": _Rgb("rgb"),
            "gbr_planes": _Rgb("gbr")}


# ---- placement --------------------------------------------------------------------------------------------------------------


def _place(torch, fam, pics, n, W, H, fill_seed=0, tight=False):
    """The first n frames of a batch (frame f shows pics[_picture_of(f)]) in noise-filled pools of torch's generator: each block of
    each distinct picture written once, GUARD bytes and more around it, bases of several residues mod 16, unequal gaps, the blocks
    of one frame in different tensors and not in Y, Cb, Cr memory order.  tight: one pool in which the chroma blocks of picture 0
    lie directly in front of the luma block of picture 1 (and those of picture 1 in front of the luma of picture 0), no gap.
    Returns (pools, int64 numpy [n, 3] of plane addresses)."""
    ids = sorted({_picture_of(f) for f in range(n)})
    order = ids[::-1]
    if len(order) >= 3:
        order[0], order[1] = order[1], order[0]
    blocks = _blocks(fam, W, H)
    G = len(blocks)
    where = {}                                                  # (picture, group) -> (pool index, byte offset of the block)
    cursors = [GUARD] * (1 if tight else G)
    if tight:
        assert len(ids) >= 2
        seq = [(0, g) for g in range(1, G)] + [(1, 0)] + [(1, g) for g in range(1, G)] + [(0, 0)]
        for pic, g in seq:
            where[(pic, g)] = (0, cursors[0])
            cursors[0] += blocks[g][1]
        cursors[0] += GUARD
    for k, pic in enumerate(order):
        for g in range(G):
            if (pic, g) in where:
                continue
            t = 0 if tight else g
            at = (cursors[t] + 15) // 16 * 16 + RESIDUES[(k + 3 * g) % len(RESIDUES)]
            where[(pic, g)] = (t, at)
            cursors[t] = at + blocks[g][1] + GUARD + 16 * ((5 * k + g) % 7)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4000 + fill_seed)
    pools = [torch.randint(0, 256, (max(cursors) + GUARD,), dtype=torch.uint8, device="cuda", generator=gen) for _ in cursors]
    # the tensors in memory order; luma goes to the highest, so a frame's blocks are never in Y, Cb, Cr order
    by_address = sorted(range(len(pools)), key=lambda i: pools[i].data_ptr())
    pool_of = {t: by_address[(t - 1) % len(pools)] for t in range(len(pools))}
    host = [p.cpu().numpy() for p in pools]
    for (pic, g), (t, at) in where.items():
        v0, length, _, A = blocks[g]
        assert at >= GUARD and at + length + GUARD <= len(host[pool_of[t]])
        host[pool_of[t]][at + (A - v0)] = fam.virtual(pics[pic], W, H)[A]
    for p, h in zip(pools, host):
        p.copy_(torch.from_numpy(h))
    table = np.zeros((n, 3), np.int64)
    for f in range(n):
        for g in range(G):
            t, at = where[(_picture_of(f), g)]
            for p, d in blocks[g][2]:   # (d < 0 for an RGB plane: its range starts c_offset behind its pointer)
                table[f, p] = pools[pool_of[t]].data_ptr() + at + d
    if n >= 3 and not tight:
        assert (table[2] == table[0]).all() and len({int(a) % 16 for a in table.reshape(-1)}) >= 3 and any(int(a) % 2 for a in table.reshape(-1))
    if G == 3 and not tight:
        assert not (table[0, 0] < table[0, 1] < table[0, 2]) and len({pool_of[t] for t in range(3)}) == 3
    return pools, table


_cache = {}


def _expected(orc, name, size, Q, n):
    """17 pictures of that family and size (noise; amplitude 64 at quality 100) and the oracle's records of the batch's first n
    frames as frames 17.., computed once per frame and shared by the tests.  Families that read the same virtual frame share."""
    W, H = size
    fam = FAMILIES[name]
    key = (getattr(fam, "preset", name), size, Q)
    if key not in _cache:
        rng = np.random.default_rng(sum(map(ord, str(key[0]))) * 1000 + W + H + Q)
        pics = fam.pictures(rng, max(BATCHES), W, H, 64 if Q == 100 else 256)
        for p in pics:
            p.setflags(write=False)
        _cache[key] = (pics, [])
    pics, recs = _cache[key]
    while len(recs) < n:
        recs.append(fam.want(orc, pics[_picture_of(len(recs))], W, H, FIRST + len(recs), Q))
    return pics, recs[:n]


def _plane_encoder(fam, W, H, Q, n, stride=0):
    enc = fam.encoder(W, H, Q, n, stride)
    before = (enc.path, enc.size_table_fused, enc.scratch_bytes(), enc._input)
    enc.set_plane_table()
    assert enc.plane_table and not enc.frame_table
    assert (enc.path, enc.size_table_fused, enc.scratch_bytes(), enc._input) == before == ("tiles", 1) + before[2:]
    return enc


# ---- 1. the parity matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,name,size", [(i * len(SIZES) + j, name, s) for i, name in enumerate(FAMILIES) for j, s in enumerate(SIZES)])
def test_parity_matrix(torch_cuda, orc, k, name, size):
    """Records and sizes of encode, and the size-table and rd-table rows, of scattered planes at both stagings; the batch size
    rotates so that every family meets batches of 1, 3, 9 and 17."""
    torch = torch_cuda
    W, H = size
    fam = FAMILIES[name]
    for qi, Q in enumerate(QUALITIES):
        n = BATCHES[(k + qi) % 4]
        pics, recs = _expected(orc, name, size, Q, n)
        pools, table = _place(torch, fam, pics, n, W, H, fill_seed=k)
        enc = _plane_encoder(fam, W, H, Q, n)
        _check(torch, enc, _device_table(torch, table), recs)
        enc.close()


# ---- 2. plane table against frame table on the device -----------------------------------------------------------------------
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
CANDS5 = (2, 4, 6, 8, 12)


@pytest.mark.parametrize("name", ["i420", "nv12", "rgb_planes"])
def test_plane_table_equals_frame_table_on_one_buffer(torch_cuda, name):
    """One contiguous buffer, frames an odd stride apart: the plane table of pointers computed from each frame's base gives the
    frame table's outputs through every call family, on one encoder whose two table modes replace one another."""
    torch = torch_cuda
    W, H, n, first = 144, 80, 9, 40
    fam = FAMILIES[name]
    rng = np.random.default_rng(11 + len(name))
    amps = (256, 64, 16, 128, 32, 8)
    frames = [fam.virtual(fam.pictures(rng, 1, W, H, amps[f % len(amps)])[0], W, H) for f in range(n)]
    stride = len(frames[0]) + 37
    host = np.random.default_rng(5).integers(0, 256, 2 * GUARD + n * stride, dtype=np.uint8)
    for f in range(n):
        host[GUARD + 1 + f * stride:][:len(frames[f])] = frames[f]
    pool = torch.from_numpy(host).cuda()
    bases = [pool.data_ptr() + GUARD + 1 + f * stride for f in range(n)]
    by_frame = torch.tensor(bases, dtype=torch.int64).cuda()
    by_plane = torch.tensor([[b, b, b] for b in bases], dtype=torch.int64).cuda()
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

    layout = enc._input
    enc.set_frame_table()
    by_frames = every_call(by_frame)
    assert by_frames["plain"][1] == by_frames["size table"][0][-1] and by_frames["size table"][1] == [0] * 8
    assert len(set(by_frames["budget"][2])) > 1, by_frames["budget"][2]
    enc.set_plane_table()                                   # the plane mode replaces the frame mode
    assert enc.plane_table and not enc.frame_table and enc._input == layout
    by_planes = every_call(by_plane)
    for key in by_frames:
        assert by_planes[key] == by_frames[key], key
    with pytest.raises(AssertionError):
        enc.encode(by_frame)                                # while the plane table is on a frame table is refused
    enc.set_frame_table()                                   # ... and the frame mode replaces the plane mode
    assert enc.frame_table and not enc.plane_table
    with pytest.raises(AssertionError):
        enc.encode(by_plane)
    again = every_call(by_frame)
    for key in by_frames:
        assert again[key] == by_frames[key], key
    enc.close()


# ---- 3. nothing but the addressed samples is used ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_surroundings_are_never_used(torch_cuda, orc, name):
    """The same samples at the same places under two fills of everything else in the pools (the guards, the gaps, row padding, and
    every byte of a plane's range that belongs to no sample of it): identical records and tables, the oracle's."""
    torch = torch_cuda
    fam = FAMILIES[name]
    Q, n = 12, 3
    for size in ((48, 32), (144, 80)):
        W, H = size
        pics, recs = _expected(orc, name, size, Q, n)
        results = []
        for fill in (1, 2):
            pools, table = _place(torch, fam, pics, n, W, H, fill_seed=40 + fill)
            dev = _device_table(torch, table)
            enc = _plane_encoder(fam, W, H, Q, n)
            rd = enc.frame_rd_table(dev, (5, Q))
            torch.cuda.synchronize()
            results.append((_encode(torch, enc, dev, FIRST), _table(torch, enc, dev, (5, Q)), [t.cpu().numpy().tolist() for t in rd]))
            enc.close()
        assert results[0] == results[1]
        assert results[0][0] == (b"".join(recs), [len(r) for r in recs])


@pytest.mark.parametrize("name", ["i420", "nv12", "nv12_plus1", "gbr_planes"])
@pytest.mark.parametrize("size", SIZES)
def test_chroma_planes_directly_in_front_of_another_frames_luma(torch_cuda, orc, name, size):
    """One pool without gaps: a frame's chroma blocks end where another frame's luma block begins, so a load clamped against
    another plane's extent reads that frame's samples."""
    torch = torch_cuda
    fam = FAMILIES[name]
    W, H = size
    Q, n = 12, 3
    pics, recs = _expected(orc, name, size, Q, n)
    pools, table = _place(torch, fam, pics, n, W, H, fill_seed=77, tight=True)
    assert len(pools) == 1
    enc = _plane_encoder(fam, W, H, Q, n)
    _check(torch, enc, _device_table(torch, table), recs)
    enc.close()


# ---- 4. the table is read on the stream -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["i420", "nv12", "rgb_planes"])
def test_the_table_is_written_by_a_kernel_on_the_stream(torch_cuda, orc, name):
    """The table holds frame 0's planes in every entry until an elementwise kernel, queued on the current stream directly in front
    of each call with no synchronisation between them, writes the real addresses: the records are the oracle's."""
    torch = torch_cuda
    (W, H), Q, n = (144, 80), 12, 9
    fam = FAMILIES[name]
    pics, recs = _expected(orc, name, (W, H), Q, n)
    pools, table = _place(torch, fam, pics, n, W, H, fill_seed=5)
    stale = _device_table(torch, np.repeat(table[:1], n, axis=0))
    delta = _device_table(torch, table - np.repeat(table[:1], n, axis=0))
    enc = _plane_encoder(fam, W, H, Q, n)
    dev = stale.clone()
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.add(stale, delta, out=dev)
    out, sizes, meta = enc.encode(dev, FIRST, out=out)
    dev.copy_(stale)
    torch.add(stale, delta, out=dev)
    rows = enc.frame_size_table(dev, (Q,), status=st)
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status & 0xFFFFFFFF == 0 and int(st.cpu()[0]) == 0
    assert [int(s) for s in sizes[:n].cpu()] == [len(r) for r in recs] == rows.cpu().numpy().tolist()[0]
    assert out[:total].cpu().numpy().tobytes() == b"".join(recs)
    enc.close()


# ---- 5. separately allocated tensors through plane_frames() -----------------------------------------------------------------
def _own_tensors(torch, name, vf, W, H):
    """The three plane tensors of one virtual frame, each an allocation of its own, and the layout under which their first bytes
    are the planes' pointers."""
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731  (a copy: an allocation of its own on the device)
    if name == "rgb_planes":
        fam = FAMILIES[name]
        e = fam.encoder_layout(W, H)
        P = e["row_pitch"]
        rows = [vf[e[k]:e[k] + H * P - 13] for k in ("r_offset", "g_offset", "b_offset")]
        return tuple(torch.as_strided(t(r), (H, W), (P, 1)) for r in rows), e
    y = t(vf[:W * H].reshape(H, W))
    if name == "i420":
        q = (W // 2) * (H // 2)
        return (y, t(vf[W * H:W * H + q].reshape(H // 2, W // 2)), t(vf[W * H + q:W * H + 2 * q].reshape(H // 2, W // 2))), \
            dict(y_offset=0, cb_offset=0, cr_offset=0, y_pitch=W, c_pitch=W // 2, c_step=1, frame_stride=W * H)
    uv = t(vf[W * H:].reshape(H // 2, W))
    return (y, uv, uv), dict(y_offset=0, cb_offset=0, cr_offset=1, y_pitch=W, c_pitch=W, c_step=2, frame_stride=W * H)


@pytest.mark.parametrize("name", ["i420", "nv12", "rgb_planes"])
def test_separately_allocated_tensors_through_plane_frames(torch_cuda, orc, name):
    """Per frame three individually allocated tensors (the NV12 UV tensor twice; one frame's planes used by another frame) go through
    Mpeg1Encoder.plane_frames and match the oracle; what the layout in force would not take as a plane is refused."""
    from ec504_imageencoder_amd import FrameTable, Mpeg1Encoder
    torch = torch_cuda
    (W, H), Q, n = (48, 32), 12, 9
    fam = FAMILIES[name]
    pics, recs = _expected(orc, name, (W, H), Q, n)
    own, layout = {}, None
    for p in sorted({_picture_of(f) for f in range(n)}):
        own[p], layout = _own_tensors(torch, name, fam.virtual(pics[p], W, H), W, H)
    frames = [own[_picture_of(f)] for f in range(n)]
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    (enc.set_rgb_plane_layout if fam.rgb else enc.set_plane_layout)(layout)
    with pytest.raises(AssertionError):
        enc.encode(enc.plane_frames(frames))                # a plane table needs set_plane_table
    enc.set_plane_table()
    ft = enc.plane_frames(frames)
    assert isinstance(ft, FrameTable) and ft.shape == (n,) and tuple(ft.table.shape) == (n, 3)
    assert ft.table.dtype == torch.int64 and ft.table.is_cuda and len(ft.frames) == 3 * n
    offs = [layout[k] for k in ("r_offset", "g_offset", "b_offset")] if fam.rgb else [0, 0, 0]
    assert ft.table.cpu().tolist() == [[t.data_ptr() - o for t, o in zip(f, offs)] for f in frames]
    if name == "nv12":
        assert int(ft.table[0, 1]) == int(ft.table[0, 2])
    del own, frames                                         # the table keeps its planes alive
    _check(torch, enc, ft, recs)
    good = ft.frames[:3]
    for bad in (torch.zeros(7, dtype=torch.uint8, device="cuda"), good[0].to(torch.int8), good[0].cpu(), good[0][:, ::2]):
        with pytest.raises(AssertionError):
            enc.plane_frames([good, (bad, good[1], good[2])])
    with pytest.raises(AssertionError):
        enc.plane_frames([])
    with pytest.raises(AssertionError):
        enc.plane_frames([good[:2]])
    enc.close()


# ---- 6. the mode's life cycle -----------------------------------------------------------------------------------------------
def test_life_cycle(torch_cuda, orc):
    """On -> every layout setter turns it off; a failed setter leaves it as it was; the frame and plane modes replace one another;
    refused, with a message that says why, on the packed, surface and (2, 4) layouts."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi, plane_layout_preset, rgb_plane_layout_preset
    torch = torch_cuda
    W, H, n = 48, 32, 3
    L = _ffi.lib()
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    assert enc.plane_table is False and L.m1v_plane_table(enc._h) == 0
    refused = ((lambda e: None, "no planes"), (lambda e: e.set_input_layout(W * 3 + 4), "m1v_set_frame_table"),
               (lambda e: e.set_sample_layout("yuy2"), "P010"), (lambda e: e.set_sample_layout("p010"), "P010"))
    for prepare, word in refused:
        prepare(enc)
        with pytest.raises(EncoderError) as ei:
            enc.set_plane_table()
        assert ei.value.code == _ffi.E_ARG and word in str(ei.value) and not enc.plane_table, word
        enc.set_plane_table(False)                          # (turning it off is always accepted)
    served = {"plane": (lambda e: e.set_plane_layout("nv12"), lambda e: e.set_plane_layout(None),
                        lambda e: e.set_plane_layout(dict(plane_layout_preset(W, H, "nv12"), y_pitch=1))),
              "sample": (lambda e: e.set_sample_layout(dict(plane_layout_preset(W, H, "i420"), y_step=1)), lambda e: e.set_sample_layout(None),
                         lambda e: e.set_sample_layout(dict(plane_layout_preset(W, H, "i420"), y_step=1, y_pitch=1))),
              "rgb_plane": (lambda e: e.set_rgb_plane_layout("bgr"), lambda e: e.set_rgb_plane_layout(None),
                            lambda e: e.set_rgb_plane_layout(dict(rgb_plane_layout_preset(W, H, "bgr"), row_pitch=1)))}
    others = {"input": (lambda e: e.set_input_layout(W * 3 + 4), lambda e: e.set_input_layout(), lambda e: e.set_input_layout(1)),
              "yuy2": (lambda e: e.set_sample_layout("yuy2"), lambda e: e.set_sample_layout(None), lambda e: e.set_sample_layout({"bogus": 1}))}
    for first, (set_first, _, _) in served.items():
        for second, (set_second, restore, bad) in {**served, **others}.items():
            set_first(enc)
            assert not enc.plane_table and not enc.frame_table
            enc.set_plane_table()
            enc.set_plane_table()                           # (idempotent)
            assert enc.plane_table and L.m1v_plane_table(enc._h) == 1 and L.m1v_frame_table(enc._h) == 0
            enc.set_frame_table()                           # each setter selects its own mode
            assert enc.frame_table and not enc.plane_table and L.m1v_plane_table(enc._h) == 0
            enc.set_plane_table()
            assert enc.plane_table and not enc.frame_table
            with pytest.raises((EncoderError, ValueError)):  # an argument error of any setter leaves the mode as it was
                bad(enc)
            assert enc.plane_table and not enc.frame_table, (first, second)
            set_second(enc)                                 # a fresh record: tables are off
            assert not enc.plane_table and not enc.frame_table, (first, second)
            set_first(enc)
            enc.set_plane_table()
            restore(enc)                                    # ... and so does the setter that restores the default
            assert not enc.plane_table and enc.input_layout == (0, 0, "rgb"), (first, second)
            set_first(enc)
            enc.set_plane_table()
            enc.set_frame_table(False)                      # either setter with 0 turns tables off
            assert not enc.plane_table and not enc.frame_table
    # after all that a plane-table encode is exact
    fam = FAMILIES["i420"]
    pics, recs = _expected(orc, "i420", (W, H), 12, n)
    pools, table = _place(torch, fam, pics, n, W, H)
    enc.set_plane_layout(fam.encoder_layout(W, H))
    enc.set_plane_table()
    _check(torch, enc, _device_table(torch, table), recs)
    enc.close()


def test_a_misaligned_table_is_an_argument_error(torch_cuda, orc):
    """A table pointer misaligned by 4: M1V_E_ARG from the encode and the table calls before anything is launched (the outputs keep
    their fill), and the next call on the encoder is exact.  The pointer lies inside the table's own allocation."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    (W, H), Q, n = (48, 32), 12, 3
    fam = FAMILIES["nv12"]
    pics, recs = _expected(orc, "nv12", (W, H), Q, n)
    pools, table = _place(torch, fam, pics, n, W, H, fill_seed=9)
    room = torch.zeros((n + 1, 3), dtype=torch.int64, device="cuda")
    room[:n].copy_(_device_table(torch, table))
    enc = _plane_encoder(fam, W, H, Q, n)
    L = _ffi.lib()
    out = torch.full((enc.frame_bound * n,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    meta = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qs = (C.c_uint8 * 2)(5, Q)
    p = C.c_void_p(room.data_ptr() + 4)
    assert L.m1v_encode_device(enc._h, p, n, FIRST, C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(sizes.data_ptr()),
                               C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8), stream) == _ffi.E_ARG
    assert "8-byte aligned" in _ffi.last_error() and "m1v_set_plane_table" in _ffi.last_error()
    assert L.m1v_frame_size_table_device(enc._h, p, n, qs, 2, C.c_void_p(sizes.data_ptr()), None, stream) == _ffi.E_ARG
    assert L.m1v_frame_sizes_device(enc._h, p, n, None, C.c_void_p(sizes.data_ptr()), None, stream) == _ffi.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((sizes == -1).all()) and bool((meta == -1).all())
    _check(torch, enc, room[:n], recs)
    enc.close()


# ---- 7. per-frame quality, one budget call, one rd call ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["yv12", "nv12_plus1", "gbr_planes"])
def test_quality_budget_and_rd_calls(torch_cuda, orc, name):
    """Scattered planes through the per-frame quality encode against the oracle, and through one budget call and one rd call
    against the same calls on the contiguous frames with the table off."""
    torch = torch_cuda
    (W, H), n = (144, 80), 9
    fam = FAMILIES[name]
    pics, _ = _expected(orc, name, (W, H), 12, n)
    pools, table = _place(torch, fam, pics, n, W, H, fill_seed=21)
    dev = _device_table(torch, table)
    qs = [int(q) for q in np.random.default_rng(8).integers(1, 13, n)]
    want = [fam.want(orc, pics[_picture_of(f)], W, H, FIRST + f, qs[f]) for f in range(n)]
    enc = _plane_encoder(fam, W, H, 12, n)
    assert _encode(torch, enc, dev, FIRST, quality=qs) == (b"".join(want), [len(r) for r in want])
    cap = sorted(len(r) for r in want)[n // 2]
    by_table = (enc.encode_to_budget(dev, cap, CANDS5, first_frame_index=FIRST), enc.encode_best_in_budget(dev, cap, CANDS5, first_frame_index=FIRST))
    enc.close()
    # the same pictures as contiguous frames of the oracle's layout, no table
    ref = fam if fam.rgb else _Ycc(fam.preset, SEPARATE)
    enc = ref.encoder(W, H, 12, n)
    frames = np.stack([ref.virtual(pics[_picture_of(f)], W, H) for f in range(n)])
    batch = torch.from_numpy(frames).cuda()
    if fam.rgb:
        e = ref.encoder_layout(W, H)
        batch = torch.as_strided(batch, (n, 3, H, W), (e["frame_stride"], H * e["row_pitch"], e["row_pitch"], 1),
                                 min(e[k] for k in ("r_offset", "g_offset", "b_offset")))
    by_stride = (enc.encode_to_budget(batch, cap, CANDS5, first_frame_index=FIRST), enc.encode_best_in_budget(batch, cap, CANDS5, first_frame_index=FIRST))
    assert by_table == by_stride
    assert len(set(by_table[0][2])) > 1, by_table[0][2]
    enc.close()


# ---- 8. pipelined mode and delivery -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["i420", "rgb_planes"])
def test_pipelined_mode_and_host_delivery(torch_cuda, orc, name):
    """Two batches of plane tables in pipelined mode, complete behind one flush; then one HostDelivery step and its flush."""
    from ec504_imageencoder_amd import FrameTable
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    (W, H), Q, n = (144, 80), 12, 9
    fam = FAMILIES[name]
    pics, recs = _expected(orc, name, (W, H), Q, n)
    pools, table = _place(torch, fam, pics, n, W, H, fill_seed=11)
    enc = _plane_encoder(fam, W, H, Q, n)
    enc.set_pipelined(True)
    assert enc.plane_table and enc.path == "tiles"
    whole, part = _device_table(torch, table), _device_table(torch, table[4:7])
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
    assert enc.plane_table
    ft = FrameTable(_device_table(torch, table), pools)
    hd = HostDelivery(enc, n)
    hd.step(ft, FIRST)
    assert hd.last is None
    del ft, pools                                           # (the delivery keeps the pending batch's input alive)
    hd.fence()
    assert bytes(hd.result().numpy()) == b"".join(recs) and [int(v) for v in hd.frame_sizes(n)] == [len(r) for r in recs]
    hd.close()
    enc.close()
