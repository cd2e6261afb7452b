"""GPU tests of the rd table (m1v_frame_rd_table_device, Mpeg1Encoder.frame_rd_table; -m gpu).  distortion[k][f] must be exactly
the measure of include/mpeg1_hip.h computed from the CPU oracle alone (tests/rd_oracle.py), and sizes[k][f] exactly what
frame_size_table writes for the same input — on noise, where the quantisation term is all there is, and on the hard content of
tests/hard_content.py, where the dropped levels dominate — through every kernel family of the rd-table row."""
import ctypes as C

import numpy as np
import pytest

import rd_oracle as rd
from gpu_calls import _frames, _mixed_frames, _oracle_sizes, _rd
from hard_content_cases import _Case, _case_dist

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sizes(torch, enc, dev, quals):
    t = enc.frame_size_table(dev, quals)
    enc.flush()
    torch.cuda.synchronize()
    return t.cpu().numpy().tolist()


def _oracle_dist(orc, px, mode, quals, channels=3):
    n, H, W = px.shape[:3]
    return [[rd.frame_distortion(orc, px[f], W, H, q, mode, channels) for f in range(n)] for q in quals]


# ---- 1. the table against the oracle: packed 3-channel noise ----------------------------------------------------------------
CASES = {
    # name: (W, H, Q, mode, n, amps, qualities)
    "cif_full_k8": (352, 288, 12, "full", 4, (4, 40, 256, 120), (1, 2, 3, 5, 7, 9, 11, 12)),
    "cif_strict_k1": (352, 288, 12, "strict", 3, (4, 40, 256), (7,)),
    "q90_wide_staging": (352, 288, 90, "full", 3, (4, 40, 20), (1, 20, 60, 76, 77, 85, 90)),
    "q90_narrow_only": (352, 288, 90, "full", 2, (40, 256), (10, 50, 76)),
    "partial_tiles_366x216": (366, 216, 12, "full", 3, (4, 40, 256), (1, 6, 12)),
    "tiny_105x49": (105, 49, 12, "full", 4, (4, 40, 256, 120), (1, 12)),
    "hd_one_frame_partial_last_tile_row": (1920, 1080, 12, "full", 1, (120,), (1, 5, 12)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_matches_oracle(torch_cuda, orc, case):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, Q, mode, n, amps, quals = CASES[case]
    enc = Mpeg1Encoder(W, H, Q, mode, max_frames=n)
    assert enc.path == "tiles" and enc.size_table_fused == 1
    rng = np.random.default_rng(sum(map(ord, case)))
    px = _mixed_frames(rng, n, W, H, 3, amps)
    dev = torch_cuda.from_numpy(px).cuda()
    sizes, dist, status = _rd(torch_cuda, enc, dev, quals)
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    assert status == [0] * len(quals), status
    assert sizes == _sizes(torch_cuda, enc, dev, quals)
    assert sizes == [_oracle_sizes(orc, px, m, q, 3) for q in quals]
    assert dist == _oracle_dist(orc, px, m, quals), (quals, dist)
    enc.close()


def test_the_gradient_of_the_design_table(torch_cuda, orc):
    """The pinned table of tests/test_rd_oracle_cpu.py, from the device: distortion is not monotonic in the quality."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H = 352, 288
    enc = Mpeg1Encoder(W, H, 92, "full", max_frames=1)
    dev = torch_cuda.from_numpy(rd.gradient_frame(W, H)[None]).cuda()
    sizes, dist, status = _rd(torch_cuda, enc, dev, rd.GRADIENT_QUALITIES)
    assert status == [0] * 8
    assert [r[0] for r in sizes] == list(rd.GRADIENT_BYTES) and [r[0] for r in dist] == list(rd.GRADIENT_D)
    enc.close()


# ---- 2. hard content through each kernel family -----------------------------------------------------------------------------


FAMILIES = ["rgb", "rgba", "surface-3-bgr-window", "surface-4-bgr-window", "planes-i420", "planes-nv12"]
NARROW_IDS, NARROW_Q = (0, 1, 2, 3, 6), (20, 50, 76)    # three hard frames, the extreme-pattern frame, a gentle one
WIDE_IDS, WIDE_Q = (0, 1, 2, 4, 5), (50, 77, 92)


@pytest.mark.parametrize("W,H", [(352, 288), (176, 208)])
@pytest.mark.parametrize("family", FAMILIES)
def test_hard_content_through_each_family(torch_cuda, orc, family, W, H):
    """Both staging widths of every family's kernel (the plane families: chroma step 1 and 2); 176x208 has a partial last
    tile column and row."""
    for ids, quals in ((NARROW_IDS, NARROW_Q), (WIDE_IDS, WIDE_Q)):
        case = _Case(torch_cuda, orc, family, W, H, ids)
        sizes, dist, status = _rd(torch_cuda, case.enc, case.dev, quals)
        assert status == [0] * len(quals), (quals, status)
        assert sizes == case.table(quals) == [case.sizes(q) for q in quals]
        assert dist == [[_case_dist(orc, case, f, q) for f in range(case.n)] for q in quals], quals
        case.close()


@pytest.mark.parametrize("family", ["rgb", "planes-nv12"])
def test_unencodable_quality_leaves_the_other_rows_exact(torch_cuda, orc, family):
    """The extreme-pattern frame has levels of 308 at qualities 90 and 92 (924 / 3): status k carries the bit there and only
    there."""
    from ec504_imageencoder_amd import _ffi
    W, H, quals = 352, 288, (50, 76, 90, 92)
    case = _Case(torch_cuda, orc, family, W, H, (0, 3, 1))
    for q, codable in zip(quals, (True, True, False, False)):       # what the oracle says of the extreme-pattern frame
        try:
            case.record(1, q)
            assert codable, q
        except ValueError:
            assert not codable, q
    sizes, dist, status = _rd(torch_cuda, case.enc, case.dev, quals)
    assert status == [0, 0, _ffi.STATUS_UNENCODABLE, _ffi.STATUS_UNENCODABLE]
    for k in (0, 1):
        assert sizes[k] == case.sizes(quals[k])
        assert dist[k] == [_case_dist(orc, case, f, quals[k]) for f in range(case.n)]
    # the next call on the encoder starts from clear status words
    assert _rd(torch_cuda, case.enc, case.dev, (50, 76)) == (sizes[:2], dist[:2], [0, 0])
    case.close()


# ---- 3. what the call writes, and the encoder's state across calls ----------------------------------------------------------
def test_writes_nothing_else_and_counters_are_cleared(torch_cuda, orc):
    """Sentinels around the three outputs; the second call is as exact as the first; encodes, size tables and rd tables of
    5, 1 and 5 frames interleaved (what a longer batch left in the counters must not reach a shorter one, nor the next)."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n, quals = 352, 288, 5, (3, 8, 12)
    K = len(quals)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    rng = np.random.default_rng(77)
    px = _mixed_frames(rng, n, W, H, 3)
    dev = torch.from_numpy(px).cuda()
    want_s = [_oracle_sizes(orc, px, orc.MODE_FULL, q, 3) for q in quals]
    want_d = _oracle_dist(orc, px, orc.MODE_FULL, quals)
    out, sizes0, meta = enc.encode(dev, 9)
    enc.flush()
    torch.cuda.synchronize()
    before = (out.clone(), sizes0.clone(), meta.clone())
    L = _ffi.lib()
    q = (C.c_uint8 * K)(*quals)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for m in (n, 1, n):
        sizes = torch.full((3 + K * m + 5,), -77, dtype=torch.int64, device="cuda")
        dist = torch.full((3 + K * m + 5,), -78, dtype=torch.int64, device="cuda")
        status = torch.full((3 + K + 2,), 0x40, dtype=torch.int32, device="cuda")
        assert L.m1v_frame_rd_table_device(enc._h, C.c_void_p(dev.data_ptr()), m, q, K, C.c_void_p(sizes.data_ptr() + 24),
                                           C.c_void_p(dist.data_ptr() + 24), C.c_void_p(status.data_ptr() + 12), stream) == 0
        torch.cuda.synchronize()
        assert [int(s) for s in sizes.cpu()] == [-77] * 3 + [s for row in want_s for s in row[:m]] + [-77] * 5, m
        assert [int(s) for s in dist.cpu()] == [-78] * 3 + [s for row in want_d for s in row[:m]] + [-78] * 5, m
        assert [int(s) for s in status.cpu()] == [0x40] * 3 + [0] * K + [0x40] * 2
        assert _sizes(torch, enc, dev[:m], quals) == [row[:m] for row in want_s]
        got = enc.encode(dev[:m], 9)
        enc.flush()
        torch.cuda.synchronize()
        assert int(got[2].cpu()[1]) == 0 and [int(s) for s in got[1][:m].cpu()] == [int(s) for s in sizes0[:m].cpu()]
    for a, b in zip(before, (out, sizes0, meta)):
        assert torch.equal(a, b)
    # n_frames == 0: OK, nothing written
    sizes.fill_(-5)
    dist.fill_(-6)
    status.fill_(0x40)
    assert L.m1v_frame_rd_table_device(enc._h, C.c_void_p(dev.data_ptr()), 0, q, K, C.c_void_p(sizes.data_ptr()),
                                       C.c_void_p(dist.data_ptr()), C.c_void_p(status.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    assert set(int(s) for s in sizes.cpu()) == {-5} and set(int(s) for s in dist.cpu()) == {-6}
    assert set(int(s) for s in status.cpu()) == {0x40}
    enc.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_profiled_pass_is_one_launch_on_the_callers_stream(torch_cuda, orc, pipelined):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, n, quals = 352, 288, 3, (2, 7, 12)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    if pipelined:
        enc.set_pipelined(True)
    scratch = enc.scratch_bytes()
    px = _mixed_frames(np.random.default_rng(5), n, W, H, 3)
    dev = torch_cuda.from_numpy(px).cuda()
    enc.profile(True)
    s, d = enc.frame_rd_table(dev, quals)
    torch_cuda.cuda.current_stream().synchronize()          # complete in stream order, without flush()
    launches, _ = enc.profile_read()
    enc.profile(False)
    assert launches == 1 and enc.scratch_bytes() == scratch
    assert s.cpu().numpy().tolist() == [_oracle_sizes(orc, px, orc.MODE_FULL, q, 3) for q in quals]
    assert d.cpu().numpy().tolist() == _oracle_dist(orc, px, orc.MODE_FULL, quals)
    enc.close()


@pytest.mark.parametrize("stage", [1, 2, 3])
def test_failed_call_leaves_the_encoder_correct(torch_cuda, orc, stage):
    """m1v_debug_fail_encode armed during an rd-table call: 1 = before the table kernel, 2 = between it and the sizes kernel
    (the counters, the distortion sums among them, hold this call's sums), 3 = after the sizes kernel.  The call fails with
    M1V_E_HIP; the rd table and the size table after it are exact."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    W, H, n, quals = 352, 288, 4, (3, 6, 9, 12)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=5)
    rng = np.random.default_rng(300 + stage)
    px = _mixed_frames(rng, n, W, H, 3)
    dev = torch.from_numpy(px).cuda()
    other = torch.from_numpy(_frames(rng, 5, W, H, 3)).cuda()
    _ffi.lib().m1v_debug_fail_encode(stage)
    try:
        with pytest.raises(EncoderError) as ei:
            enc.frame_rd_table(other, quals)
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    enc.flush()
    torch.cuda.synchronize()
    want_s = [_oracle_sizes(orc, px, orc.MODE_FULL, q, 3) for q in quals]
    sizes, dist, status = _rd(torch, enc, dev, quals)
    assert (sizes, status) == (want_s, [0] * len(quals))
    assert dist == _oracle_dist(orc, px, orc.MODE_FULL, quals)
    assert _sizes(torch, enc, dev, quals) == want_s
    enc.close()


def test_argument_errors(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=2)
    dev = torch.zeros((2, 288, 352, 3), dtype=torch.uint8, device="cuda")
    for quals in ((), (4, 4), (8, 4), (0, 4), (4, 13), tuple(range(1, 10))):
        with pytest.raises(EncoderError) as ei:
            enc.frame_rd_table(dev, quals)
        assert ei.value.code == _ffi.E_ARG, quals
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    sizes = torch.zeros(32, dtype=torch.int64, device="cuda")
    dist = torch.zeros(32, dtype=torch.int64, device="cuda")
    ps, pd, pr = C.c_void_p(sizes.data_ptr()), C.c_void_p(dist.data_ptr()), C.c_void_p(dev.data_ptr())
    assert L.m1v_frame_rd_table_device(enc._h, pr, 3, q, 2, ps, pd, None, None) == _ffi.E_ARG
    assert L.m1v_frame_rd_table_device(enc._h, pr, -1, q, 2, ps, pd, None, None) == _ffi.E_ARG
    assert L.m1v_frame_rd_table_device(enc._h, pr, 2, q, 2, None, pd, None, None) == _ffi.E_ARG
    assert L.m1v_frame_rd_table_device(enc._h, pr, 2, q, 2, ps, None, None, None) == _ffi.E_ARG
    assert L.m1v_frame_rd_table_device(enc._h, None, 2, q, 2, ps, pd, None, None) == _ffi.E_ARG
    assert L.m1v_frame_rd_table_device(enc._h, pr, 2, None, 2, ps, pd, None, None) == _ffi.E_ARG
    # an encoder forced to the run kernels has no fused table: there is no probe fallback for the distortion
    enc.debug_set_path("runs")
    assert enc.size_table_fused == 0
    assert L.m1v_frame_rd_table_device(enc._h, pr, 2, q, 2, ps, pd, None, None) == _ffi.E_ARG
    assert "fused" in _ffi.last_error()
    torch.cuda.synchronize()
    assert set(int(s) for s in sizes.cpu()) == {0} and set(int(s) for s in dist.cpu()) == {0}
    enc.close()
