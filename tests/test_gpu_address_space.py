"""Every input layout at the top of its 32-bit in-frame offsets and with frames past 4 GiB, through the kernels (-m gpu).

The cases, the pool and the fills are tests/address_space.py's; tests/test_address_space_cpu.py shows on the host that every case
lies where its name says, that no 32-bit slip of a kernel can leave the pool and that each modelled slip changes a record.  Here
every case is placed in the one pool of the module (about 10 GiB, filled once per fill; a case writes its samples, runs and
restores the fill) and goes, under both fills, through

  the plain encode on an encoder of quality 60 (levels staged in bytes) and of quality 90 (in halfwords),
  the encode with per-frame quality, m1v_frame_sizes_device,
  the size table and the rd table at a narrow (20, 76) and a wide (20, 76, 77, 90) candidate set,
  for the float kinds the to-bytes call of the layout, against the rule of tests/float_planes.py,
  and, for the stride_4g_d case of each kind, an encode in pipelined mode and encode_streams with two spans,

each compared for equality with the oracle's records, sizes and distortions of the content (status 0, sizes and totals equal).
The calls go through the Python wrapper with torch.as_strided views of the pool (frames() and plane_frames() for the table
modes), so that its _check_input arithmetic meets the same strides.  The C setter itself accepts each case and refuses the
next value up of an edge at its maximum.  If the pool cannot be allocated the tests fail; none skips."""
import numpy as np
import pytest

import address_space as A

pytestmark = pytest.mark.gpu

CASES = A.cases()
STREAM_SPANS = ((1, 5), (1, 40))        # encode_streams: frame 0 is frame 5 of one stream, frame 1 frame 40 of another
QUALITIES = sorted(set(A.TABLE_WIDE) | {A.Q_BYTE})
PER_FRAME = (A.Q_HALF, A.Q_BYTE)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def pool(torch_cuda):
    torch = torch_cuda
    try:
        held = [torch.empty(A.POOL_BYTES, dtype=torch.uint8, device="cuda")]
    except Exception as e:  # noqa: BLE001 (whatever the allocator raises: the tests fail, they do not skip)
        pytest.fail(f"the pool of {A.POOL_BYTES} bytes cannot be allocated: {e}")
    assert held[0].data_ptr() % 256 == 0
    yield held[0]
    del held[0]
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=A.FILLS)
def filled(torch_cuda, pool, request):
    """The pool under one fill: the only large operation of the module, once per fill."""
    torch = torch_cuda
    pattern = torch.from_numpy(A.fill_pattern(request.param)).cuda()
    whole = A.POOL_BYTES // A.PERIOD * A.PERIOD
    pool[:whole].view(-1, A.PERIOD).copy_(pattern)
    pool[whole:].copy_(pattern[:A.POOL_BYTES - whole])
    torch.cuda.synchronize()
    return pool, pattern


@pytest.fixture(scope="module")
def encoders():
    """One encoder per geometry, channel count and quality, shared by the cases: each case sets its own layout."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    made = {}

    def get(W, H, Q, channels):
        key = (W, H, Q, channels)
        if key not in made:
            made[key] = Mpeg1Encoder(W, H, Q, "full", channels=channels, max_frames=A.N)
            made[key].reserve_scratch(True)      # (no batch exhausts the worst case: status 4 cannot occur)
        return made[key]

    yield get
    for enc in made.values():
        enc.close()


_expected = {}


def _oracle(orc, case):
    """Once per case, for both fills: the records of both frames at every quality used and at the streams' indices, the
    distortions at the tables' qualities."""
    key = A.case_id(case)
    if key not in _expected:
        frames = A.content(case)
        rec = {q: A.records(orc, case, frames, q) for q in QUALITIES}
        assert all(None not in r for r in rec.values())
        dist = {q: [A.distortion(orc, case, frames, f, q) for f in range(A.N)] for q in A.TABLE_WIDE}
        streams = [A.record(orc, case, frames, f, A.Q_HALF, i) for f, (_, i) in enumerate(STREAM_SPANS)] if case.edge == "stride_4g_d" else None
        _expected[key] = (frames, rec, dist, streams)
    return _expected[key]


def _set_layout(enc, kind, lay):
    if kind.family == "surface":
        enc.set_input_layout(lay["row_pitch"], lay["frame_stride"], lay["order"])
    elif kind.family == "planes":
        enc.set_plane_layout({k: v for k, v in lay.items() if k != "y_step"})
    else:
        {"samples": enc.set_sample_layout, "rgb_planes": enc.set_rgb_plane_layout, "float_planes": enc.set_float_plane_layout,
         "float_pixels": enc.set_float_pixel_layout}[kind.family](lay)


def _view(torch, pool, case, lay):
    """The batch as the wrapper takes it under the case's layout: a torch.as_strided view of the pool from F on."""
    kind, (W, H) = A.KIND[case.kind], A.GEOMETRIES[case.geometry]
    S, stride = A.sample_bytes(kind), lay["frame_stride"]
    if kind.family == "surface":
        return pool.as_strided((A.N, H, W, kind.a), (stride, lay["row_pitch"], kind.a, 1), A.FRAME0)
    if kind.family in A.YCC:
        return pool.as_strided((A.N, A.extent(kind, lay, W, H)), (stride, 1), A.FRAME0)
    typed = pool if S == 1 else pool.view(getattr(torch, kind.a))
    if kind.family in A.THREE:      # the channels of an [n, C, H, W] tensor whose plane stride divides the three offsets
        plane, channels = A.gcd_plane([lay["r_offset"], lay["g_offset"], lay["b_offset"]], S)
        return typed.as_strided((A.N, channels, H, W), (stride // S, plane, lay["row_pitch"] // S, 1), A.FRAME0 // S)
    return typed.as_strided((A.N, H, W, kind.b), (stride // S, lay["row_pitch"] // S, kind.b, 1), A.FRAME0 // S)


def _device_argument(torch, pool, enc, case, lay):
    """What the calls take in the place of rgb: the view, or the table of its frames or planes (entries F + f * stride)."""
    kind, (W, H) = A.KIND[case.kind], A.GEOMETRIES[case.geometry]
    view = _view(torch, pool, case, lay)
    if not case.table:
        return view
    if case.table == "kt":
        enc.set_frame_table()
        assert enc.frame_table and not enc.plane_table
        return enc.frames([view[f] for f in range(A.N)])
    enc.set_plane_table()
    assert enc.plane_table and not enc.frame_table
    base = [A.FRAME0 + f * lay["frame_stride"] for f in range(A.N)]
    if kind.family == "planes":     # a plane's tensor starts at its pointer, the frame's base: the layout's offset lies inside it
        E = A.extent(kind, lay, W, H)
        return enc.plane_frames([(pool.as_strided((E,), (1,), b),) * 3 for b in base])
    return enc.plane_frames([tuple(pool.as_strided((H, W), (lay["row_pitch"], 1), b + lay[k]) for k in ("r_offset", "g_offset", "b_offset"))
                             for b in base])


def _encode(torch, enc, dev, first, quality=None):
    """One encode into a worst-case buffer -> (status, sizes, total, bytes)."""
    n = dev.shape[0]
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    out, sizes, meta = enc.encode(dev, first, out=out, quality=quality)
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    return status & 0xFFFFFFFF, [int(s) for s in sizes[:n].cpu()], total, out[:min(total, out.numel())].cpu().numpy().tobytes()


def _check(what, got, want):
    status, sizes, total, data = got
    print(f"{what}: status {status}, sizes {sizes} (oracle {[len(r) for r in want]}), total {total}")
    assert status == 0, what
    assert sizes == [len(r) for r in want] and total == sum(sizes), what
    bad = [f for f in range(len(want)) if data[sum(sizes[:f]):sum(sizes[:f + 1])] != want[f]]
    assert not bad, f"{what}: the records of frames {bad} are not the oracle's"


def _tables(torch, enc, dev, quals, rec, dist):
    st = torch.full((len(quals),), 0x40, dtype=torch.int32, device="cuda")
    table = enc.frame_size_table(dev, quals, status=st)
    st2 = torch.full((len(quals),), 0x40, dtype=torch.int32, device="cuda")
    sizes, d = enc.frame_rd_table(dev, quals, status=st2)
    enc.flush()
    torch.cuda.synchronize()
    want = [[len(r) for r in rec[q]] for q in quals]
    print(f"tables {quals}: sizes {table.tolist()} / {sizes.tolist()} (oracle {want}), distortion {d.tolist()}")
    assert st.tolist() == [0] * len(quals) and st2.tolist() == [0] * len(quals), quals
    assert table.tolist() == want, f"frame_size_table{quals}"
    assert sizes.tolist() == want, f"frame_rd_table{quals} sizes"
    assert d.tolist() == [dist[q] for q in quals], f"frame_rd_table{quals} distortion"


@pytest.mark.parametrize("case", CASES, ids=[A.case_id(c) for c in CASES])
def test_address_space(torch_cuda, orc, filled, encoders, case):
    from ec504_imageencoder_amd.encoder import EncoderError
    torch = torch_cuda
    pool, pattern = filled
    kind, (W, H) = A.KIND[case.kind], A.GEOMETRIES[case.geometry]
    lay, bumps = A.layout(case)
    frames, rec, dist, streams = _oracle(orc, case)
    channels = kind.a if kind.family == "surface" else 3
    enc, enc_byte = encoders(W, H, A.Q_HALF, channels), encoders(W, H, A.Q_BYTE, channels)

    for group in bumps:             # the C setter refuses the next value up, and leaves the encoder as it was
        with pytest.raises(EncoderError, match="4 GiB"):
            _set_layout(enc, kind, dict(lay, **{k: lay[k] + A.unit(kind) for k in group}))

    at, val = A.writes(case)
    where = torch.from_numpy(at).cuda()
    pool[where] = torch.from_numpy(val).cuda()
    try:
        _set_layout(enc, kind, lay)
        _set_layout(enc_byte, kind, lay)
        assert enc.path == "tiles" and enc.size_table_fused == 1
        dev, dev_byte = _device_argument(torch, pool, enc, case, lay), _device_argument(torch, pool, enc_byte, case, lay)

        _check(f"encode at {A.Q_HALF}", _encode(torch, enc, dev, A.FIRST), rec[A.Q_HALF])
        _check(f"encode at {A.Q_BYTE}", _encode(torch, enc_byte, dev_byte, A.FIRST), rec[A.Q_BYTE])
        per_frame = [rec[q][f] for f, q in enumerate(PER_FRAME)]
        _check(f"encode with per-frame quality {PER_FRAME}", _encode(torch, enc, dev, A.FIRST, quality=list(PER_FRAME)), per_frame)

        st = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
        sizes = enc.frame_sizes(dev, quality=list(PER_FRAME), status=st)
        enc.flush()
        torch.cuda.synchronize()
        print(f"frame_sizes: {sizes.tolist()}, status {st.tolist()}")
        assert st.tolist() == [0] and sizes.tolist() == [len(r) for r in per_frame], "frame_sizes"

        for quals in (A.TABLE_NARROW, A.TABLE_WIDE):
            _tables(torch, enc, dev, quals, rec, dist)

        if kind.family == "float_planes":
            got = enc.float_planes_to_bytes(dev).cpu().numpy()
            assert np.array_equal(got, frames.transpose(0, 3, 1, 2)), "float_planes_to_bytes"
        if kind.family == "float_pixels":
            got = enc.float_pixels_to_bytes(dev).cpu().numpy()
            assert np.array_equal(got, frames), "float_pixels_to_bytes"

        if streams is not None:     # the stride_4g_d case of the kind
            enc.set_pipelined(True)
            try:
                _check("pipelined encode", _encode(torch, enc, dev, A.FIRST), rec[A.Q_HALF])
            finally:
                enc.flush()
                torch.cuda.synchronize()
                enc.set_pipelined(False)
            data, sizes, stream_bytes = enc.encode_streams(dev, STREAM_SPANS)
            print(f"encode_streams: sizes {sizes}, stream bytes {stream_bytes}")
            assert [int(s) for s in sizes] == [len(r) for r in streams] == stream_bytes and bytes(data) == b"".join(streams), "encode_streams"
    finally:
        torch.cuda.synchronize()
        pool[where] = pattern[where % A.PERIOD]
        torch.cuda.synchronize()
