"""Batches and pictures past the extents of a grid (-m gpu): how many frames one call carries, the second trip of the grid-stride
kernels with capped grids, and the two batches between which the tile kernels' group divisor leaves the magic multiplication.

a. Long batches: 16 x 16 FULL at quality 12 with 65,535 and 65,537 frames through encode, frame_sizes and coefficients (the tile
   form, and the run-shaped k_coefficients of an encoder forced to the run kernels, whose grid's z is the batch).  The rule
   (include/mpeg1_hip.h beside max_frames): one call carries at most m1v_batch_limit = min(max_frames, the extents the device
   reports for a grid's y and z) frames; a longer batch is refused with M1V_E_ARG in front of every launch and the next call is an
   ordinary one.  So 65,535 frames equal the oracle byte for byte, and 65,537 do too where the device's limit admits them, else
   the call is refused with a reason that names the limit and the next call is exact.  The limit is read from the device.
b. Past the capped grids: convert over nine 4096 x 4096 frames of all 2^24 colours rolled by k pixels (k_convert4's second trip,
   every tie colour in every slot of a group), one 4099 x 4099 frame (the byte-wise k_convert: second trip, first exhaustive run),
   the 4096 x 4096 frame one byte off alignment; synth over nine frames of more than 64 MiB whose size is no multiple of 8; subsample
   from one macroblock up (m1v_create refuses smaller pictures, so the 2 x 2 plane cannot be reached through the library).  All
   compared with the oracle's planes or frames, the large ones on the device.
c. The divisor switch: 33 and 32 frames of 7680 x 4320 (4,080 tiles per frame: 32 * 8 * 4080^2 < 2^32 <= 33 * 8 * 4080^2), the
   cheaper of the two picture sizes in device and oracle time (1.1 G pixels against 4.3 G for 517 frames of 3840 x 2160), through
   encode, frame_size_table and frame_rd_table at K = 8, every frame against the oracle and rd_oracle on 16 threads (the records
   of all 33 frames, the sizes and distortions of the three distinct pictures at the eight qualities: once for both batches)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import launch_side as LS
import rd_oracle as rd

pytestmark = pytest.mark.gpu

Q = 12
K8 = (1, 2, 4, 6, 8, 10, 11, 12)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _enc(W, H, channels=3, max_frames=1, mode="full"):
    from ec504_imageencoder_amd import Mpeg1Encoder
    return Mpeg1Encoder(W, H, Q, mode, channels=channels, max_frames=max_frames)


# hipDeviceAttribute_t (hip_runtime_api.h): hipDeviceAttributeCudaCompatibleBegin = 0, then in declaration order.  The block's
# extents stand right in front of the grid's; they and the multiprocessor count are held against what torch reports of the device,
# so a runtime that numbered the attributes otherwise fails here and not in a comparison of limits
_HIP_ATTR = {"MaxBlockDimX": 26, "MaxGridDimX": 29, "MaxGridDimY": 30, "MaxGridDimZ": 31, "MaxThreadsPerBlock": 56, "MultiprocessorCount": 63}


def _loaded_hip():
    """The HIP runtime this process has loaded (torch's own copy), by the path it is mapped from: no second runtime is started."""
    import ctypes as C
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64" in line}
    assert len(paths) == 1, f"one HIP runtime is loaded: {sorted(paths)}"
    return C.CDLL(paths.pop())


def _device_limits(torch):
    """(x, y, z) extents of a grid as the device reports them, asked of the HIP runtime that torch has loaded."""
    import ctypes as C
    hip, dev = _loaded_hip(), torch.cuda.current_device()

    def attribute(name):
        v = C.c_int(0)
        assert hip.hipDeviceGetAttribute(C.byref(v), _HIP_ATTR[name], dev) == 0, name
        return v.value

    props = torch.cuda.get_device_properties(dev)
    assert attribute("MaxThreadsPerBlock") == props.max_threads_per_block == attribute("MaxBlockDimX")
    assert attribute("MultiprocessorCount") == props.multi_processor_count
    return attribute("MaxGridDimX"), attribute("MaxGridDimY"), attribute("MaxGridDimZ")


# ---- a. long batches ----------------------------------------------------------------------------------------------------------------
LONG_W = LONG_H = 16
LONG_N = 65537
LONG_POOL = 13
LONG_FIRST = 250        # the index passes 255 -> 256 at once, and 65,535 -> 65,536 inside the batch

_long = {}


def _long_batch(orc):
    """The batch [65537, 16, 16, 3] of 13 distinct pictures in a drawn order, the oracle's records of all of it (0.05 s) and the
    pool's coefficients.  Computed once; read, never written."""
    if not _long:
        rng = np.random.default_rng(65537)
        amps = (256, 200, 4, 250, 120, 256, 60, 230, 256, 16, 180, 240, 256)
        pool = np.stack([np.clip(rng.integers(0, 256, (1, 1, 3)) + rng.integers(-a, a + 1, (LONG_H, LONG_W, 3)), 0, 255).astype(np.uint8)
                         for a in amps])
        order = rng.integers(0, LONG_POOL, LONG_N)
        assert all(order[e - 1] != order[e] for e in (65535, 65536))
        batch = np.ascontiguousarray(pool[order])
        data, sizes = orc.encode_frames(batch, LONG_N, LONG_W, LONG_H, LONG_FIRST, Q, orc.MODE_FULL, threads=16)
        sizes = [int(s) for s in sizes]
        assert len(set(sizes)) > 3, "the pool's records differ in size"
        coef = np.stack([orc.frame_coefficients(p, LONG_W, LONG_H, Q, orc.MODE_FULL).reshape(6, 64) for p in pool])
        _long.update(batch=batch, order=order, data=data, sizes=sizes, coef=coef)
    return _long


@pytest.fixture(scope="module")
def long_rig(torch_cuda, orc):
    enc = _enc(LONG_W, LONG_H, max_frames=LONG_N)
    assert enc.path == "tiles"
    dev = torch_cuda.from_numpy(_long_batch(orc)["batch"]).cuda()
    yield enc, dev
    enc.close()


@pytest.fixture(scope="module")
def runs_enc():
    """An encoder forced to the run kernels: its coefficients() launches the run-shaped k_coefficients, whose grid's z is the
    batch's frames (the call is not bound by max_frames)."""
    enc = _enc(LONG_W, LONG_H, max_frames=1)
    enc.debug_set_path("runs")
    assert enc.path == "runs"
    yield enc
    enc.close()


def _run_coefficients(torch, enc, dev, n, L):
    """coefficients of the first n frames through the run-shaped kernel against the oracle."""
    coef = enc.coefficients(dev[:n])
    torch.cuda.synchronize()
    want = torch.from_numpy(L["coef"].astype(np.int16)).cuda()[torch.from_numpy(L["order"][:n]).cuda()]
    assert coef.shape == want.shape and torch.equal(coef, want), f"k_coefficients over {n} frames"


def _exact(torch, enc, dev, n, L):
    """encode, frame_sizes and coefficients of the first n frames against the oracle."""
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    out, sizes, meta = enc.encode(dev[:n], LONG_FIRST, out=out)
    word = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    probe = enc.frame_sizes(dev[:n], status=word)
    coef = enc.coefficients(dev[:n])
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    want_sizes = L["sizes"][:n]
    assert status & 0xFFFFFFFF == 0 and int(word.item()) == 0
    assert total == sum(want_sizes)
    assert torch.equal(sizes[:n].cpu(), torch.tensor(want_sizes, dtype=torch.int64)), "encode: sizes"
    assert torch.equal(probe.cpu(), torch.tensor(want_sizes, dtype=torch.int64)), "frame_sizes"
    assert torch.equal(out[:total].cpu(), torch.frombuffer(bytearray(L["data"][:total]), dtype=torch.uint8)), "encode: bytes"
    want_coef = torch.from_numpy(L["coef"].astype(np.int16)).cuda()[torch.from_numpy(L["order"][:n]).cuda()]
    assert torch.equal(coef, want_coef), "coefficients"


def test_device_grid_limits(torch_cuda, long_rig):
    enc, _ = long_rig
    x, y, z = _device_limits(torch_cuda)
    print(f"grid extents the device reports: x {x}, y {y}, z {z}; m1v_batch_limit of max_frames {LONG_N}: {enc.batch_limit}")
    assert enc.batch_limit == min(LONG_N, y, z)


def test_long_batch_65535(torch_cuda, orc, long_rig, runs_enc):
    enc, dev = long_rig
    assert enc.batch_limit >= 65535, "every HIP device takes 65,535 workgroups along y and z"
    _exact(torch_cuda, enc, dev, 65535, _long_batch(orc))
    _run_coefficients(torch_cuda, runs_enc, dev, 65535, _long_batch(orc))


def test_long_batch_65537(torch_cuda, orc, long_rig, runs_enc):
    """Exact where the device's limit admits 65,537 frames; else refused in front of the first launch, the limit named, and the
    next call exact (a poisoned counter set would make it clear and wait, and a counter left half used would make it wrong).
    The run-shaped k_coefficients (grid z) keeps the same rule; the tile form of coefficients, whose grid has one dimension,
    takes the 65,537 frames either way."""
    from ec504_imageencoder_amd import _ffi
    from ec504_imageencoder_amd.encoder import EncoderError
    torch = torch_cuda
    enc, dev = long_rig
    L = _long_batch(orc)
    _, y, z = _device_limits(torch)
    limit = min(y, z)
    print(f"65,537 frames against the device's limit of {limit}: {'exact' if LONG_N <= limit else 'refused'}")
    if LONG_N <= limit:
        _exact(torch, enc, dev, LONG_N, L)
        _run_coefficients(torch, runs_enc, dev, LONG_N, L)
        return
    out = torch.full((enc.frame_bound * 8,), LS.POISON, dtype=torch.uint8, device="cuda")
    word = torch.full((1,), 0x40, dtype=torch.int32, device="cuda")
    for call in (lambda: enc.encode(dev, LONG_FIRST, out=out), lambda: enc.frame_sizes(dev, status=word), lambda: runs_enc.coefficients(dev),
                 lambda: enc.frame_size_table(dev, K8), lambda: enc.frame_rd_table(dev, K8)):
        with pytest.raises(EncoderError, match=str(limit)) as err:
            call()
        assert err.value.code == _ffi.E_ARG
    torch.cuda.synchronize()
    assert bool((out == LS.POISON).all()) and int(word.item()) == 0x40, "a refused call queues nothing"
    _exact(torch, enc, dev, limit, L)        # the longest batch the rule admits, at once behind the refusals
    _run_coefficients(torch, runs_enc, dev, limit, L)
    _exact(torch, enc, dev, 9, L)
    tiles = enc.coefficients(dev)            # the tile form: a one-dimensional grid of 65,537 workgroups
    want = torch.from_numpy(L["coef"].astype(np.int16)).cuda()[torch.from_numpy(L["order"]).cuda()]
    assert torch.equal(tiles, want), "coefficients of 65,537 frames on the tile form"


# ---- b. past the capped grids -------------------------------------------------------------------------------------------------------
def _oracle_planes(orc, frame, channels):
    Y, Cb, Cr = orc.convert(frame, channels=channels)
    return np.stack([Y, Cb, Cr])


@pytest.mark.parametrize("channels", [3, 4])
def test_convert_second_trip_of_k_convert4(torch_cuda, orc, channels):
    """Nine frames of 2^24 pixels = 37.7 M groups of four against the 33.5 M one trip of 131,072 workgroups covers."""
    torch = torch_cuda
    n = 9
    enc = _enc(4096, 4096, channels)
    rgb = torch.empty((n, 4096, 4096, channels), dtype=torch.uint8, device="cuda")
    want = torch.empty((n, 3, 1 << 24), dtype=torch.uint8, device="cuda")
    for k in range(n):
        frame = LS.rolled_colours(k, channels)
        rgb[k].copy_(torch.from_numpy(frame))
        want[k].copy_(torch.from_numpy(_oracle_planes(orc, frame, channels)))
    assert rgb.data_ptr() % 4 == 0 and (n << 22) > 131072 * 256
    got = enc.convert(rgb)
    torch.cuda.synchronize()
    bad = [k for k in range(n) if not torch.equal(got[k], want[k])]
    assert not bad, f"frames {bad} differ from the oracle's planes"
    if channels == 3:       # the same frame from a buffer one byte off alignment: the byte-wise kernel on every colour
        flat = torch.empty(3 * (1 << 24) + 8, dtype=torch.uint8, device="cuda")
        off = flat[1:1 + 3 * (1 << 24)].view(1, 4096, 4096, 3)
        off.copy_(rgb[3:4])
        assert off.data_ptr() % 4 == 1
        assert torch.equal(enc.convert(off)[0], want[3]), "one byte off alignment"
    enc.close()


@pytest.mark.parametrize("channels", [3, 4])
def test_convert_second_trip_of_k_convert(torch_cuda, orc, channels):
    """4099 x 4099 = 16,801,801 pixels, odd: the byte-wise kernel, whose one trip of 65,536 workgroups covers 2^24."""
    torch = torch_cuda
    W = H = 4099
    assert (W * H) % 4 and W * H > 65536 * 256
    c = (np.arange(W * H, dtype=np.uint32) * np.uint32(2654435761 % (1 << 24) | 1)) & np.uint32(0xFFFFFF)   # every colour, in a stride
    assert len(np.unique(c[:1 << 24])) == 1 << 24
    frame = np.empty((W * H, channels), np.uint8)
    frame[:, 0], frame[:, 1], frame[:, 2] = c >> 16, (c >> 8) & 255, c & 255
    if channels == 4:
        frame[:, 3] = 255 - frame[:, 1]
    frame = frame.reshape(1, H, W, channels)
    enc = _enc(W, H, channels)
    got = enc.convert(torch.from_numpy(frame).cuda())
    want = torch.from_numpy(_oracle_planes(orc, frame[0], channels)).cuda()
    assert torch.equal(got[0], want)
    enc.close()


def test_synth_second_trip_and_unaligned_tails(torch_cuda, orc):
    """Nine frames of 4099 x 4099 x 4 = 67,207,204 bytes (above 64 MiB, 4 mod 8): 75.6 M words against the 67.1 M one trip of
    262,144 workgroups covers, and every odd frame starts 4 bytes off an 8-byte boundary."""
    torch = torch_cuda
    W = H = 4099
    n, nbytes = 9, W * H * 4
    assert nbytes > 64 << 20 and nbytes % 8 == 4 and n * ((nbytes + 7) // 8) > 262144 * 256
    enc = _enc(W, H, 4)
    out = torch.full((n, H, W, 4), LS.POISON, dtype=torch.uint8, device="cuda")
    enc.synth(n, seed=77, first_frame_index=250, out=out)
    want = orc.synth_frames(n, W, H, seed=77, first_index=250, channels=4)
    for f in range(n):
        assert torch.equal(out[f].view(-1), torch.from_numpy(want[f].reshape(-1)).cuda()), f"frame {f}"
    enc.close()


SUBSAMPLE_SIZES = [(16, 16), (18, 16), (18, 18), (34, 30), (34, 32), (66, 62), (130, 66), (1030, 18), (2050, 34)]


@pytest.mark.parametrize("W, H", SUBSAMPLE_SIZES)
def test_subsample_sizes(torch_cuda, orc, W, H):
    """From the smallest picture an encoder takes (one macroblock: m1v_create refuses anything below, so 2 x 2 cannot be reached)
    up to widths whose half is odd, and sizes whose quarter is no multiple of 256: part of one workgroup, 255 lanes, one lane
    more than a workgroup, many workgroups with a part one."""
    torch = torch_cuda
    assert ((W // 2) * (H // 2)) % 256 != 0 and ((W // 2) % 2 == 1 or (W, H) == (16, 16))
    rng = np.random.default_rng(W * 10000 + H)
    cb, cr = (rng.integers(0, 256, W * H, dtype=np.uint8) for _ in range(2))
    enc = _enc(W, H)
    a, b = enc.subsample(torch.from_numpy(cb).cuda(), torch.from_numpy(cr).cuda())
    wa, wb = orc.subsample(cb, cr, W, H)
    assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb)
    enc.close()


# ---- c. the divisor switch ----------------------------------------------------------------------------------------------------------
SW_W, SW_H = 7680, 4320
SW_FIRST = 250

_switch = {}


def _pictures():
    """Three distinct 7680 x 4320 pictures: noise, a gradient under light noise, noise of an amplitude that changes per macroblock row."""
    rng = np.random.default_rng(4080)
    shape = (SW_H, SW_W, 3)
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    ramp = (np.arange(SW_W, dtype=np.int16)[None, :, None] // 11 + np.arange(SW_H, dtype=np.int16)[:, None, None] // 7
            + np.array([0, 60, 130], np.int16)[None, None, :]) % 256
    gentle = np.clip(ramp + rng.integers(-6, 7, shape, dtype=np.int16), 0, 255).astype(np.uint8)
    amp = (np.arange(SW_H, dtype=np.int16)[:, None, None] // 16 * 37 % 100 + 8)
    mixed = np.clip(128 + rng.integers(-128, 129, shape, dtype=np.int16) * amp // 64, 0, 255).astype(np.uint8)
    return np.stack([noise, gentle, mixed])


def _switch_oracle(orc):
    """Once for both batches, on 16 threads: the three pictures, the oracle's records of all 33 frames, its sizes of each picture
    at K8, and rd_oracle's distortions (block_distortion over slices of the pictures' blocks, summed)."""
    if not _switch:
        last, nxt = LS.switch_batches(*LS.tile_grid(SW_W, SW_H))
        assert (last, nxt) == (32, 33)
        pics = _pictures()
        with ThreadPoolExecutor(16) as pool:
            recs = [pool.submit(orc.encode_frame, pics[f % 3], SW_W, SW_H, SW_FIRST + f, Q, orc.MODE_FULL) for f in range(nxt)]
            jobs = {(p, q): pool.submit(orc.encode_frame, pics[p], SW_W, SW_H, 0, q, orc.MODE_FULL) for p in range(3) for q in K8[:-1]}
            coef = {(p, q): pool.submit(orc.frame_coefficients, pics[p], SW_W, SW_H, q, orc.MODE_FULL) for p in range(3) for q in K8 + (100,)}
            parts = {}
            for p in range(3):      # (rd_oracle.frame_distortion in slices: the raw coefficients are the levels at quality 100)
                c = coef[(p, 100)].result().reshape(-1, 64)
                for q in K8:
                    lv, d = coef.pop((p, q)).result().reshape(-1, 64), rd.divisors_zigzag(orc, q)
                    parts[(p, q)] = [pool.submit(rd.block_distortion, c[a:a + 8192], lv[a:a + 8192], d) for a in range(0, len(c), 8192)]
            D = {k: int(sum(int(j.result().sum()) for j in v)) for k, v in parts.items()}
            recs = [bytes(j.result()) for j in recs]
            S = {k: len(j.result()) for k, j in jobs.items()}
        data, sizes = b"".join(recs), [len(r) for r in recs]
        assert len(set(sizes[:3])) == 3, "the three pictures' records differ in size"
        S.update({(p, Q): sizes[p] for p in range(3)})      # (a record's size does not depend on its frame index)
        _switch.update(pics=pics, data=data, sizes=sizes, S=S, D=D, n=(last, nxt))
    return _switch


@pytest.fixture(scope="module")
def switch_rig(torch_cuda, orc):
    torch = torch_cuda
    o = _switch_oracle(orc)
    enc = _enc(SW_W, SW_H, max_frames=o["n"][1])
    assert enc.path == "tiles" and enc.size_table_fused == 1
    pics = torch.from_numpy(o["pics"]).cuda()
    dev = pics[torch.arange(o["n"][1], device="cuda") % 3].contiguous()
    del pics
    yield enc, dev
    enc.close()


@pytest.mark.parametrize("which", [1, 0], ids=["33_plain_division", "32_magic"])
def test_divisor_switch(torch_cuda, orc, switch_rig, which):
    torch = torch_cuda
    enc, dev = switch_rig
    o = _switch_oracle(orc)
    n = o["n"][which]
    cols, rows = LS.tile_grid(SW_W, SW_H)
    group = LS.launch_divisors(cols, rows, n)[0]
    print(f"{SW_W} x {SW_H}: {cols} x {rows} tiles, {n} frames, group divisor {group[0]} with multiplier {group[1]} ({'magic' if group[1] else 'plain division'})")
    assert (group[1] == 0) == (which == 1)
    batch = dev[:n]
    want_sizes = o["sizes"][:n]
    out = torch.empty(sum(want_sizes) + 4096, dtype=torch.uint8, device="cuda")
    out, sizes, meta = enc.encode(batch, SW_FIRST, out=out)
    st = torch.full((len(K8),), 0x40, dtype=torch.int32, device="cuda")
    table = enc.frame_size_table(batch, K8, status=st)
    st2 = torch.full((len(K8),), 0x40, dtype=torch.int32, device="cuda")
    rd_sizes, rd_dist = enc.frame_rd_table(batch, K8, status=st2)
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status & 0xFFFFFFFF == 0 and total == sum(want_sizes)
    assert [int(s) for s in sizes[:n].cpu()] == want_sizes
    got = out[:total].cpu().numpy().tobytes()
    at = np.concatenate([[0], np.cumsum(want_sizes)])
    bad = [f for f in range(n) if got[at[f]:at[f + 1]] != o["data"][at[f]:at[f + 1]]]
    assert not bad, f"the records of frames {bad} are not the oracle's"
    assert st.tolist() == [0] * len(K8) and st2.tolist() == [0] * len(K8)
    want_table = [[o["S"][(f % 3, q)] for f in range(n)] for q in K8]
    assert table.tolist() == want_table, "frame_size_table"
    assert rd_sizes.tolist() == want_table, "frame_rd_table sizes"
    assert rd_dist.tolist() == [[o["D"][(f % 3, q)] for f in range(n)] for q in K8], "frame_rd_table distortion"
