"""GPU tests of the fused size table for 4-channel input (k_size_table_rgba; -m gpu).  A 4-channel encoder keeps its encodes on
the run kernels (path == "runs") but takes its size tables — and those of budget, batch-budget and bitrate calls — from ONE
fused pass (size_table_fused == 1).  Every table is compared for equality with the oracle's record sizes; the K-probe table
of a hook-forced encoder (debug_set_path("runs"): size_table_fused == 0) is the device-side reference."""
import ctypes as C

import numpy as np
import pytest

from gpu_calls import _frames, _mixed_frames, _oracle, _oracle_sizes, _table
from rate_rules import batch_rule, cbr_rule
from table_cases import SEQUENCE, RateMixed
from table_cases import RGBA_CASES as CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _fused(W, H, Q, mode, n, pipelined=False):
    """A 4-channel encoder as a caller gets it: run kernels for the encode, the fused pass for the table."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, mode, channels=4, max_frames=n)
    assert enc.path == "runs" and enc.size_table_fused == 1
    if pipelined:
        enc.set_pipelined(True)
        assert enc.size_table_fused == 1
    return enc


def _probing(W, H, Q, mode, n):
    """The same encoder forced to runs by the hook: one probe per quality."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(W, H, Q, mode, channels=4, max_frames=n)
    enc.debug_set_path("runs")
    assert enc.path == "runs" and enc.size_table_fused == 0
    return enc


def _rgba(rng, n, W, H, amps=(4, 40, 256, 120)):
    """Mixed-amplitude frames; the alpha bytes are noise, so a kernel that reads alpha as a colour gets every size wrong."""
    px = _mixed_frames(rng, n, W, H, 4, amps)
    px[..., 3] = rng.integers(0, 256, px.shape[:3], dtype=np.uint8)
    return px


# ---- 1. the table against the oracle --------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_matches_oracle(torch_cuda, orc, case):
    W, H, Q, mode, n, amps, quals = CASES[case]
    enc = _fused(W, H, Q, mode, n)
    rng = np.random.default_rng(sum(map(ord, case)) + 4)
    px = _rgba(rng, n, W, H, amps)
    dev = torch_cuda.from_numpy(px).cuda()
    got, status = _table(torch_cuda, enc, dev, quals)
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    want = [_oracle_sizes(orc, px, m, q, 4) for q in quals]
    assert status == [0] * len(quals), status
    assert got == want, (quals, got, want)
    enc.close()


# ---- 2. any buffer alignment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_odd_input_address_through_the_c_entry_point(torch_cuda, orc, offset):
    from ec504_imageencoder_amd import _ffi
    W, H, n, quals = 352, 288, 3, (2, 8, 12)
    enc = _fused(W, H, 12, "full", n)
    px = _rgba(np.random.default_rng(21 + offset), n, W, H)
    buf = torch_cuda.zeros(px.size + 8, dtype=torch_cuda.uint8, device="cuda")
    buf[offset:offset + px.size] = torch_cuda.from_numpy(px.reshape(-1)).cuda()
    sizes = torch_cuda.full((len(quals) * n,), -1, dtype=torch_cuda.int64, device="cuda")
    q = (C.c_uint8 * len(quals))(*quals)
    rc = _ffi.lib().m1v_frame_size_table_device(enc._h, C.c_void_p(buf.data_ptr() + offset), n, q, len(quals),
                                                C.c_void_p(sizes.data_ptr()), None,
                                                C.c_void_p(torch_cuda.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch_cuda.cuda.synchronize()
    want = [s for qq in quals for s in _oracle_sizes(orc, px, orc.MODE_FULL, qq, 4)]
    assert [int(s) for s in sizes.cpu()] == want
    enc.close()


# ---- 3. the fused pass against K probes, device against device ------------------------------------------------------------
@pytest.mark.parametrize("case", ["cif_full_k8", "q90_wide_staging", "partial_tiles_366x216", "strip_kernel_352x144"])
def test_fused_equals_the_probes(torch_cuda, case):
    W, H, Q, mode, n, amps, quals = CASES[case]
    fused, probing = _fused(W, H, Q, mode, n), _probing(W, H, Q, mode, n)
    dev = torch_cuda.from_numpy(_rgba(np.random.default_rng(33), n, W, H, amps)).cuda()
    a, b = _table(torch_cuda, fused, dev, quals), _table(torch_cuda, probing, dev, quals)
    assert a == b and a[1] == [0] * len(quals)
    fused.close()
    probing.close()


def test_1080p_batch_equals_the_probes(torch_cuda):
    """300 x 1080p synthetic frames (every byte noise, alpha included), K = 8."""
    n, quals = 300, (1, 2, 4, 6, 8, 10, 11, 12)
    fused, probing = _fused(1920, 1080, 12, "full", n), _probing(1920, 1080, 12, "full", n)
    dev = fused.synth(n, seed=504)
    a, b = _table(torch_cuda, fused, dev, quals), _table(torch_cuda, probing, dev, quals)
    assert a[1] == [0] * len(quals) and b[1] == [0] * len(quals)
    for k, q in enumerate(quals):
        assert a[0][k] == b[0][k], q
    fused.close()
    probing.close()


# ---- 4. the same pixels without their alpha bytes, on the 3-channel tile table -----------------------------------------------
@pytest.mark.parametrize("case", ["cif_full_k8", "q90_wide_staging", "partial_tiles_366x216", "tiny_105x49"])
def test_equals_the_tile_table_of_the_stripped_pixels(torch_cuda, case):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, Q, mode, n, amps, quals = CASES[case]
    px = _rgba(np.random.default_rng(44), n, W, H, amps)
    fused = _fused(W, H, Q, mode, n)
    tiles = Mpeg1Encoder(W, H, Q, mode, max_frames=n)
    assert tiles.path == "tiles" and tiles.size_table_fused == 1
    got = _table(torch_cuda, fused, torch_cuda.from_numpy(px).cuda(), quals)
    want = _table(torch_cuda, tiles, torch_cuda.from_numpy(np.ascontiguousarray(px[..., :3])).cuda(), quals)
    assert got == want
    fused.close()
    tiles.close()


# ---- 5. launches and results of the rate calls ----------------------------------------------------------------------------
CANDS5 = (2, 4, 6, 8, 12)


def _frame_rule(s, cap):
    """m1v_encode_budget_device's rule on a table s[k][f]: the largest candidate that fits, else the smallest."""
    pick = []
    for f in range(len(s[0])):
        fits = [k for k in range(len(s)) if s[k][f] <= cap]
        pick.append(fits[-1] if fits else 0)
    return pick, [f for f in range(len(s[0])) if s[pick[f]][f] > cap]


@pytest.mark.parametrize("forced", [False, True], ids=["fused", "hook_forced"])
def test_rate_calls_launches_and_results(torch_cuda, orc, forced):
    """A K = 5 budget, batch-budget and bitrate call on a 4-channel encoder: one size-table pass + one encode = 2 profiled
    launches (K + 1 = 6 on the hook-forced encoder); bytes, sizes, picks and the over-budget flag are the rule applied to the
    oracle's table."""
    n, W, H = 5, 352, 288
    enc = _probing(W, H, 12, "full", n) if forced else _fused(W, H, 12, "full", n)
    expect = len(CANDS5) + 1 if forced else 2
    px = _rgba(np.random.default_rng(101), n, W, H)
    dev = torch_cuda.from_numpy(px).cuda()
    s = [_oracle_sizes(orc, px, orc.MODE_FULL, c, 4) for c in CANDS5]
    level = torch_cuda.full((1,), 10 ** 6, dtype=torch_cuda.int64, device="cuda")
    for call in ("budget", "batch", "cbr"):
        enc.profile(True)
        if call == "budget":
            cap = sorted(x for row in s for x in row)[len(s) * n // 2]
            got, sizes, ch, ov = enc.encode_to_budget(dev, cap, CANDS5)
            pick, over = _frame_rule(s, cap)
            assert len(set(pick)) > 1, pick
        elif call == "batch":
            B = (sum(s[1]) + sum(s[2])) // 2
            got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, CANDS5)
            pick, over = batch_rule(s, B)
        else:
            r = sorted(s[2])[2]
            got, sizes, ch, ov = enc.encode_at_bitrate(dev, r, 2 * r, CANDS5, level)
            pick, over, lvl = cbr_rule(s, r, 2 * r, 10 ** 6)
            assert int(level.cpu()[0]) == lvl
        launches, _ = enc.profile_read()
        enc.profile(False)
        assert launches == expect, (call, launches)
        chosen = [CANDS5[k] for k in pick]
        want, wsizes = _oracle(orc, px, 0, chosen, orc.MODE_FULL, 4)
        assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), call
    enc.close()


# ---- 6. what the call writes ----------------------------------------------------------------------------------------------
def test_writes_nothing_else(torch_cuda):
    """Sentinels past [K][n] and past the K status words, and the output of an earlier encode, stay untouched."""
    from ec504_imageencoder_amd import _ffi
    n, quals = 3, (4, 8, 12)
    enc = _fused(352, 288, 12, "full", 5)
    dev = torch_cuda.from_numpy(_rgba(np.random.default_rng(41), n, 352, 288)).cuda()
    out, sizes0, meta = enc.encode(dev, 9)
    enc.flush()
    torch_cuda.cuda.synchronize()
    before = (out.clone(), sizes0.clone(), meta.clone())
    K = len(quals)
    sizes = torch_cuda.full((K * n + 5,), -77, dtype=torch_cuda.int64, device="cuda")
    status = torch_cuda.full((K + 2,), 0x40, dtype=torch_cuda.int32, device="cuda")
    q = (C.c_uint8 * K)(*quals)
    stream = C.c_void_p(torch_cuda.cuda.current_stream().cuda_stream)
    L = _ffi.lib()
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), n, q, K, C.c_void_p(sizes.data_ptr()),
                                         C.c_void_p(status.data_ptr()), stream) == 0
    enc.flush()
    torch_cuda.cuda.synchronize()
    got = [int(s) for s in sizes.cpu()]
    assert all(s > 48 for s in got[:K * n]) and got[K * n:] == [-77] * 5
    assert [int(s) for s in status.cpu()] == [0] * K + [0x40] * 2
    for a, b in zip(before, (out, sizes0, meta)):
        assert torch_cuda.equal(a, b)
    sizes.fill_(-5)
    status.fill_(0x40)
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), 0, q, K, C.c_void_p(sizes.data_ptr()),
                                         C.c_void_p(status.data_ptr()), stream) == 0
    torch_cuda.cuda.synchronize()
    assert set(int(s) for s in sizes.cpu()) == {-5} and set(int(s) for s in status.cpu()) == {0x40}
    enc.close()


# ---- 7. encoder state across calls of every kind --------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_interleaved_calls_stay_exact(torch_cuda, orc, pipelined):
    """SEQUENCE of tests/test_gpu_rate.py (plain, per-frame, probe, table, budget, batch-budget and bitrate calls) twice."""
    enc = _fused(352, 288, 12, "full", 5, pipelined)
    calls = RateMixed(torch_cuda, orc, enc, seed=700 + pipelined)
    for _ in range(2):
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("sequence", "rgba", pipelined))
    enc.close()


@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("pipelined", [False, True])
def test_failed_table_call_leaves_the_encoder_correct(torch_cuda, orc, pipelined, stage):
    """m1v_debug_fail_encode makes the table call return M1V_E_HIP on the host (nothing faults on the device): 1 = before the
    fused kernel, 2 = between it and the sizes kernel (the counters hold this call's sums), 3 = after the sizes kernel.  Every
    call of every kind after it is exact."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    enc = _fused(352, 288, 12, "full", 5, pipelined)
    calls = RateMixed(torch_cuda, orc, enc, seed=800 + 10 * stage + pipelined)
    calls.call("table", 5)
    calls.call("plain", 4)
    calls.check("before")
    dev = torch_cuda.from_numpy(_frames(calls.rng, 5, 352, 288, 4)).cuda()
    _ffi.lib().m1v_debug_fail_encode(stage)
    try:
        with pytest.raises(EncoderError) as ei:
            enc.frame_size_table(dev, (3, 6, 9, 12))
        assert ei.value.code == _ffi.E_HIP
    finally:
        _ffi.lib().m1v_debug_fail_encode(0)
    enc.flush()
    torch_cuda.cuda.synchronize()
    for kind, n in SEQUENCE:
        calls.call(kind, n)
    calls.check("after the failure")
    enc.close()


# ---- 8. a level no code exists for ----------------------------------------------------------------------------------------
def test_unencodable_quality_is_flagged_like_the_probes(torch_cuda, orc):
    """The picture of tests/test_gpu_state.py::_unencodable (at quality 92 every block has |level| 308 after a zero) with an
    alpha byte: M1V_STATUS_UNENCODABLE in exactly the status words where the K-probe encoder sets it; every other row is the
    oracle's."""
    from gpu_calls import _unencodable
    from ec504_imageencoder_amd import _ffi
    W, H, n, quals = 352, 288, 2, (12, 50, 92)
    fused, probing = _fused(W, H, 92, "full", n), _probing(W, H, 92, "full", n)
    px = _unencodable(fused, n).copy()
    px[..., 3] = np.random.default_rng(8).integers(0, 256, px.shape[:3], dtype=np.uint8)
    dev = torch_cuda.from_numpy(px).cuda()
    got, status = _table(torch_cuda, fused, dev, quals)
    ref, ref_status = _table(torch_cuda, probing, dev, quals)
    bit = _ffi.STATUS_UNENCODABLE
    assert [x & bit for x in status] == [x & bit for x in ref_status], (status, ref_status)
    assert all(x in (0, bit) for x in status), status                 # the fused pass has no other bit to report
    assert status[-1] == bit and 0 in status, status
    for k, q in enumerate(quals):
        if status[k] == 0:
            assert got[k] == _oracle_sizes(orc, px, orc.MODE_FULL, q, 4) == ref[k], q
    fused.close()
    probing.close()
