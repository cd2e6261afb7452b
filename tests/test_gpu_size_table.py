"""GPU tests of the size table (m1v_frame_size_table_device, Mpeg1Encoder.frame_size_table) and of the budget encode built on it
(-m gpu).  d_sizes[k][f] must be the length of the oracle's record of frame f at quality qualities[k], on the tile path (one
fused k_size_table_tiles pass) and on the run / strip paths (one probe per quality); a budget call on tiles is one size-table
pass + one encode."""
import ctypes as C

import numpy as np
import pytest

from gpu_calls import _frames, _mixed_frames, _oracle, _oracle_sizes, _table
from table_cases import CANDS, Mixed, _rule
from table_cases import RGB_CASES as CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- 1. the table against the oracle --------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_matches_oracle(torch_cuda, orc, case):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, Q, mode, n, amps, quals = CASES[case]
    enc = Mpeg1Encoder(W, H, Q, mode, max_frames=n)
    assert enc.path == "tiles"
    rng = np.random.default_rng(sum(map(ord, case)))
    rgb = _mixed_frames(rng, n, W, H, 3, amps)
    dev = torch_cuda.from_numpy(rgb).cuda()
    got, status = _table(torch_cuda, enc, dev, quals)
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    want = [_oracle_sizes(orc, rgb, m, q, 3) for q in quals]
    assert status == [0] * len(quals), status
    assert got == want, (quals, got, want)
    enc.close()


def test_odd_input_address_through_the_c_entry_point(torch_cuda, orc):
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    W, H, n, quals = 352, 288, 3, (2, 8, 12)
    enc = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
    rng = np.random.default_rng(21)
    rgb = _mixed_frames(rng, n, W, H, 3)
    buf = torch_cuda.zeros(rgb.size + 4, dtype=torch_cuda.uint8, device="cuda")
    buf[1:1 + rgb.size] = torch_cuda.from_numpy(rgb.reshape(-1)).cuda()
    sizes = torch_cuda.full((len(quals) * n,), -1, dtype=torch_cuda.int64, device="cuda")
    q = (C.c_uint8 * len(quals))(*quals)
    rc = _ffi.lib().m1v_frame_size_table_device(enc._h, C.c_void_p(buf.data_ptr() + 1), n, q, len(quals),
                                                C.c_void_p(sizes.data_ptr()), None,
                                                C.c_void_p(torch_cuda.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch_cuda.cuda.synchronize()
    want = [s for qq in quals for s in _oracle_sizes(orc, rgb, orc.MODE_FULL, qq, 3)]
    assert [int(s) for s in sizes.cpu()] == want
    enc.close()


def test_1080p_batch_equals_the_probe_device_against_device(torch_cuda):
    """300 x 1080p synthetic frames: row k of the table = frame_sizes(quality=[q_k] * n)."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    n, quals = 300, (1, 2, 4, 6, 8, 10, 11, 12)
    enc = Mpeg1Encoder(1920, 1080, 12, "full", max_frames=n)
    dev = enc.synth(n, seed=504)
    got, status = _table(torch_cuda, enc, dev, quals)
    assert status == [0] * len(quals)
    for k, q in enumerate(quals):
        want = [int(s) for s in enc.frame_sizes(dev, quality=[q] * n).cpu()]
        assert got[k] == want, q
    enc.close()


# ---- 2. the fallback of the run and strip paths ---------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("producer", ["runs", "strips"])
def test_fallback_gives_the_same_table(torch_cuda, orc, producer, pipelined):
    from ec504_imageencoder_amd import Mpeg1Encoder
    W, H, C_ = (352, 144, 4) if producer == "strips" else (352, 288, 3)
    n, quals = 4, (1, 3, 8, 12)
    enc = Mpeg1Encoder(W, H, 12, "full", channels=C_, max_frames=n)
    if producer == "runs":
        enc.debug_set_path("runs")
    assert enc.path == "runs"
    if pipelined:
        enc.set_pipelined(True)
    rng = np.random.default_rng(31 + pipelined)
    rgb = _mixed_frames(rng, n, W, H, C_)
    dev = torch_cuda.from_numpy(rgb).cuda()
    got, status = _table(torch_cuda, enc, dev, quals)
    assert status == [0] * len(quals)
    assert got == [_oracle_sizes(orc, rgb, orc.MODE_FULL, q, C_) for q in quals]
    if producer == "runs":                       # the same table as the tile kernel's on the same frames
        tiles = Mpeg1Encoder(W, H, 12, "full", max_frames=n)
        assert _table(torch_cuda, tiles, dev, quals)[0] == got
        tiles.close()
    enc.close()


# ---- 3. what the call writes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_writes_nothing_else(torch_cuda, producer):
    """Sentinels past [K][n] and the output of an earlier encode stay untouched; the status words are zero."""
    from ec504_imageencoder_amd import Mpeg1Encoder, _ffi
    n, quals = 3, (4, 8, 12)
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=5)
    if producer == "runs":
        enc.debug_set_path("runs")
    rng = np.random.default_rng(41)
    dev = torch_cuda.from_numpy(_mixed_frames(rng, n, 352, 288, 3)).cuda()
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
    # n_frames == 0: OK, nothing written
    sizes.fill_(-5)
    status.fill_(0x40)
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), 0, q, K, C.c_void_p(sizes.data_ptr()),
                                         C.c_void_p(status.data_ptr()), stream) == 0
    torch_cuda.cuda.synchronize()
    assert set(int(s) for s in sizes.cpu()) == {-5} and set(int(s) for s in status.cpu()) == {0x40}
    enc.close()


def test_argument_errors(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=2)
    dev = torch_cuda.zeros((2, 288, 352, 3), dtype=torch_cuda.uint8, device="cuda")
    for quals in ((), (4, 4), (8, 4), (0, 4), (4, 13), tuple(range(1, 10))):
        with pytest.raises(EncoderError) as ei:
            enc.frame_size_table(dev, quals)
        assert ei.value.code == _ffi.E_ARG, quals
        q = (C.c_uint8 * max(len(quals), 1))(*quals)
        sizes = torch_cuda.zeros(32, dtype=torch_cuda.int64, device="cuda")
        assert _ffi.lib().m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), 2, q, len(quals),
                                                      C.c_void_p(sizes.data_ptr()), None, None) == _ffi.E_ARG, quals
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    sizes = torch_cuda.zeros(32, dtype=torch_cuda.int64, device="cuda")
    big = torch_cuda.zeros((3, 288, 352, 3), dtype=torch_cuda.uint8, device="cuda")
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(big.data_ptr()), 3, q, 2, C.c_void_p(sizes.data_ptr()), None, None) == _ffi.E_ARG
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), 2, q, 2, None, None, None) == _ffi.E_ARG
    assert L.m1v_frame_size_table_device(enc._h, None, 2, q, 2, C.c_void_p(sizes.data_ptr()), None, None) == _ffi.E_ARG
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), 2, None, 2, C.c_void_p(sizes.data_ptr()), None, None) == _ffi.E_ARG
    assert L.m1v_frame_size_table_device(enc._h, C.c_void_p(dev.data_ptr()), -1, q, 2, C.c_void_p(sizes.data_ptr()), None, None) == _ffi.E_ARG
    torch_cuda.cuda.synchronize()
    assert set(int(s) for s in sizes.cpu()) == {0}
    enc.close()


# ---- 4. encoder state across calls of every kind --------------------------------------------------------------------------


SEQUENCE = (("plain", 5), ("table", 3), ("probe", 3), ("table", 5), ("quality", 5), ("budget", 2), ("table", 1), ("plain", 5))


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_interleaved_calls_stay_exact(torch_cuda, orc, producer, pipelined):
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=5)
    if producer == "runs":
        enc.debug_set_path("runs")
    if pipelined:
        enc.set_pipelined(True)
    calls = Mixed(torch_cuda, orc, enc, seed=100 + pipelined + 2 * len(producer))
    for _ in range(2):
        for kind, n in SEQUENCE:
            calls.call(kind, n)
        calls.check(("sequence", producer, pipelined))
    enc.close()


@pytest.mark.parametrize("stage", [1, 2, 3])
@pytest.mark.parametrize("pipelined", [False, True])
def test_failed_size_table_call_leaves_the_encoder_correct(torch_cuda, orc, pipelined, stage):
    """m1v_debug_fail_encode armed during a size-table call on tiles: 1 = before the probe kernel, 2 = between the probe kernel
    and the sizes kernel (the counters hold this call's sums), 3 = after the sizes kernel.  The call fails with M1V_E_HIP; every
    call of every kind after it is exact."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=5)
    if pipelined:
        enc.set_pipelined(True)
    calls = Mixed(torch_cuda, orc, enc, seed=200 + 10 * stage + pipelined)
    calls.call("table", 5)
    calls.call("plain", 4)
    calls.check("before")
    dev = torch_cuda.from_numpy(_frames(calls.rng, 5, 352, 288, 3)).cuda()
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


# ---- 5. the budget encode on the size table -------------------------------------------------------------------------------
@pytest.mark.parametrize("producer", ["tiles", "runs"])
def test_budget_call_launches_and_result(torch_cuda, orc, producer):
    """On tiles a K-candidate budget call is one size-table pass + one encode: 2 profiled launches (K + 1 on the run path).  Its
    picks, sizes and bytes are the rule applied to the oracle's table."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    n = 6
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=n)
    if producer == "runs":
        enc.debug_set_path("runs")
    rng = np.random.default_rng(51)
    rgb = _mixed_frames(rng, n, 352, 288, 3)
    dev = torch_cuda.from_numpy(rgb).cuda()
    first = 17
    table = {c: _oracle(orc, rgb, first, [c] * n, orc.MODE_FULL, 3)[1] for c in CANDS}
    allsizes = sorted(s for c in CANDS for s in table[c])
    budget = allsizes[len(allsizes) // 2]
    chosen, over = _rule(table, [budget] * n)
    assert len(set(chosen)) > 1, chosen
    enc.profile(True)
    got, sizes, ch, ov = enc.encode_to_budget(dev, budget, CANDS, first_frame_index=first)
    launches, _ = enc.profile_read()
    enc.profile(False)
    assert launches == (2 if producer == "tiles" else len(CANDS) + 1), launches
    want, wsizes = _oracle(orc, rgb, first, chosen, orc.MODE_FULL, 3)
    assert (ch, ov, sizes) == (chosen, over, wsizes) and got == want
    enc.close()
