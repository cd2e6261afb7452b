"""GPU tests of the picks alone (m1v_rd_batch_pick_device, m1v_rd_cbr_pick_device, Mpeg1Encoder.rd_batch_pick / rd_bitrate_pick;
-m gpu) on crafted rd tables against the Python model (tests/rd_rate_model.py): picks, picked distortion, status word and level,
all by exact equality."""
import ctypes as C
import random

import pytest

import rd_rate_model as M

pytestmark = pytest.mark.gpu

MAX_FRAMES = 513
OVER_BIT = {M.BEST_IN_BUDGET: 16, M.SMALLEST_AT_DISTORTION: 32}
U64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def enc(torch_cuda):
    from ec504_imageencoder_amd import Mpeg1Encoder
    e = Mpeg1Encoder(176, 208, 12, "full", max_frames=MAX_FRAMES)
    yield e
    e.close()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tables(torch, S, D, status):
    s = torch.tensor(S, dtype=torch.int64).cuda()
    d = torch.tensor(D, dtype=torch.int64).cuda()
    st = torch.tensor(status, dtype=torch.int32).cuda() if status is not None else None
    return s, d, st


def _batch_many(torch, enc, S, D, rule, limits, status=None):
    """One m1v_rd_batch_pick_device per limit, back to back on the current stream, one wait:
    [(picks, picked D, status word)] per limit."""
    from ec504_imageencoder_amd import _ffi
    K, n, m = len(S), len(S[0]), len(limits)
    s, d, st = _tables(torch, S, D, status)
    picks = torch.full((m, n), 255, dtype=torch.uint8, device="cuda")
    pd = torch.full((m, n), -1, dtype=torch.int64, device="cuda")
    word = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _ffi.lib()
    for i, limit in enumerate(limits):
        rc = L.m1v_rd_batch_pick_device(enc._h, _p(s), _p(d), _p(st), n, K, rule, int(limit), C.c_void_p(picks.data_ptr() + i * n),
                                        C.c_void_p(pd.data_ptr() + 8 * i * n), C.c_void_p(word.data_ptr() + 4 * i), stream)
        assert rc == 0, _ffi.last_error()
    torch.cuda.synchronize()
    picks, pd, word = picks.cpu().tolist(), pd.cpu().tolist(), word.cpu().tolist()
    return [(picks[i], pd[i], word[i] & 0xFFFFFFFF) for i in range(m)]


def _expected_by_prefix(S, D, rule, status=None):
    """{limit: (picks, over)} at every prefix boundary of the order of all steps and one below it, plus 0 and 2^64 - 1, from the
    model's chains and order (the same thing as M.batch_pick at that limit: _check_batch checks a sample)."""
    ch = M.chains(S, D, status)
    order = M.steps(S, D, ch)
    byte = rule == M.BEST_IN_BUDGET
    picks = [c[0] for c in ch]
    total = sum((S if byte else D)[k][f] for f, k in enumerate(picks))
    after = [(total, list(picks))]                       # (the bounded sum, the picks) after each prefix of the order
    for f, j, ds, dd in order:
        total += ds if byte else -dd
        picks[f] = ch[f][j]
        after.append((total, list(picks)))
    limits = {0, U64} | {t - e for t, _ in after for e in (0, 1) if 0 <= t - e <= U64}
    want = {}
    for limit in limits:
        if byte:     # the longest prefix whose bytes fit; none, not even the start: over budget
            fits = [i for i, (t, _) in enumerate(after) if t <= limit]
            want[limit] = (after[fits[-1]][1], False) if fits else (after[0][1], True)
        else:        # the shortest prefix that reaches the ceiling; none: over, every step taken
            reach = [i for i, (t, _) in enumerate(after) if t <= limit]
            want[limit] = (after[reach[0]][1], False) if reach else (after[-1][1], True)
    return want


def _check_batch(torch, enc, S, D, status=None, sample=6, seed=0):
    rng = random.Random(seed)
    for rule in (M.BEST_IN_BUDGET, M.SMALLEST_AT_DISTORTION):
        want = _expected_by_prefix(S, D, rule, status)
        limits = sorted(want)
        for limit in rng.sample(limits, min(sample, len(limits))) + [0, U64]:      # the table above is the model's
            assert want[limit] == M.batch_pick(S, D, rule, limit, status), (rule, limit)
        got = _batch_many(torch, enc, S, D, rule, limits, status)
        for limit, (picks, pd, word) in zip(limits, got):
            w_picks, w_over = want[limit]
            assert picks == w_picks, (rule, limit)
            assert pd == [D[k][f] for f, k in enumerate(w_picks)], (rule, limit)
            assert word == (OVER_BIT[rule] if w_over else 0), (rule, limit)


def _random_table(rng, n, K, hi=6):
    return [[rng.randint(1, hi) for _ in range(n)] for _ in range(K)], [[rng.randint(1, hi) for _ in range(n)] for _ in range(K)]


# ---- 1. the batch forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 2, 9, 150, 300])
def test_batch_pick_on_random_tables_with_ties(torch_cuda, enc, n, K):
    """Values in 1..6: nearly every ratio and many (s, D) pairs tie; dominated, duplicate and collinear candidates and sizes that
    fall as k grows are everywhere.  Every prefix boundary and one below it, 0 and 2^64 - 1, both rules."""
    rng = random.Random(1000 * n + K)
    S, D = _random_table(rng, n, K)
    _check_batch(torch_cuda, enc, S, D, seed=n + K)
    if n == 9:                                  # a second table on the same encoder, and the first one again: the same results
        S2, D2 = _random_table(rng, n, K, hi=40)
        _check_batch(torch_cuda, enc, S2, D2, seed=1)
        _check_batch(torch_cuda, enc, S, D, seed=n + K)


def test_batch_pick_crafted_shapes(torch_cuda, enc):
    """Dominated (k = 2), duplicate (k = 3 = k = 1) and collinear (k = 0, 1, 4, 7 on one line: every step of slope 2) candidates,
    and a size that falls as k grows (k = 5 .. 7); frame 2 differs by one value, so that its first step comes before all others."""
    S = [[10] * 3, [20] * 3, [25] * 3, [20] * 3, [30] * 3, [40] * 3, [38] * 3, [36] * 3]
    D = [[100, 100, 101], [80] * 3, [90] * 3, [80] * 3, [60] * 3, [50] * 3, [49] * 3, [48] * 3]
    assert M.chains(S, D) == [[0, 1, 4, 7]] * 3
    assert [t[:2] for t in M.steps(S, D, M.chains(S, D))][:3] == [(2, 1), (0, 1), (0, 2)]
    for _ in range(2):
        _check_batch(torch_cuda, enc, S, D, sample=50)


@pytest.mark.parametrize("flip", [False, True])
def test_ratios_that_differ_only_in_the_full_cross_product(torch_cuda, enc, flip):
    """Frame a's step is (ds, dd) = (m, 1000 (m + 1)), frame b's (m - 1, 1000 m), m = 2^31: b's ratio is the greater by
    1000 / (m (m - 1)), far below fp64's resolution at 1000, and the cross products pass 2^64.  Limits that admit exactly one
    of the two steps, in both frame orders."""
    m = 2 ** 31
    a = ([10, 10 + m], [1000 * (m + 1) + 5, 5])
    b = ([10, 10 + m - 1], [1000 * m + 5, 5])
    cols = (b, a) if flip else (a, b)
    S = [[c[0][k] for c in cols] for k in range(2)]
    D = [[c[1][k] for c in cols] for k in range(2)]
    ib = 0 if flip else 1
    assert float(1000 * (m + 1)) / float(m) == float(1000 * m) / float(m - 1)          # fp64 calls them equal
    only_b = [1 if f == ib else 0 for f in range(2)]
    for limit in (20 + m - 1, 20 + m):
        assert M.batch_pick(S, D, M.BEST_IN_BUDGET, limit) == (only_b, False)
    start = sum(D[0])
    assert M.batch_pick(S, D, M.SMALLEST_AT_DISTORTION, start - 1000 * m) == (only_b, False)
    _check_batch(torch_cuda, enc, S, D, sample=50)
    got = _batch_many(torch_cuda, enc, S, D, M.BEST_IN_BUDGET, [20 + m - 1, 20 + m])
    assert [g[0] for g in got] == [only_b, only_b] and [g[2] for g in got] == [0, 0]
    got = _batch_many(torch_cuda, enc, S, D, M.SMALLEST_AT_DISTORTION, [start - 1000 * m])
    assert got[0][0] == only_b and got[0][2] == 0


def test_large_values_need_128_bit_sums_and_products(torch_cuda, enc):
    """D near 2^62 with s near 2^32 - 1 in 7 frames: the start's distortions sum to more than 2^64."""
    n = 7
    S = [[1 + f for f in range(n)], [2 ** 31 + f for f in range(n)], [2 ** 32 - 1 - f for f in range(n)]]
    D = [[2 ** 62 + 2 ** 61 - f for f in range(n)], [2 ** 61 + 7 * f for f in range(n)], [3 + f for f in range(n)]]
    assert sum(D[0]) > 2 ** 64
    _check_batch(torch_cuda, enc, S, D, sample=50)


def test_rows_out_of_the_running(torch_cuda, enc):
    rng = random.Random(77)
    S, D = _random_table(rng, 9, 8)
    for status in ([0, 1, 0, 0, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 0, 0, 1], [1] * 8, [0] * 8):
        assert M.running(8, status) == ([k for k in range(8) if not status[k]] or [0])
        _check_batch(torch_cuda, enc, S, D, status=status, sample=50)
    # status bits other than UNENCODABLE do not put a row out
    _check_batch(torch_cuda, enc, S, D, status=[2, 8, 16, 32, 0, 0, 0, 0], sample=50)


def test_python_rd_batch_pick(torch_cuda, enc):
    torch = torch_cuda
    rng = random.Random(5)
    S, D = _random_table(rng, 9, 4, hi=30)
    s, d, st = _tables(torch, S, D, [0, 1, 0, 0])
    for rule in (M.BEST_IN_BUDGET, M.SMALLEST_AT_DISTORTION):
        for limit in (0, 60, 120, 10 ** 6):
            assert enc.rd_batch_pick(s, d, rule, limit) == M.batch_pick(S, D, rule, limit)
            assert enc.rd_batch_pick(s, d, rule, limit, status=st) == M.batch_pick(S, D, rule, limit, [0, 1, 0, 0])


# ---- 2. the bitrate form ---------------------------------------------------------------------------------------------------
def _cbr(torch, enc, S, D, rate, cap, level, status=None, same_pointer=False):
    """One m1v_rd_cbr_pick_device -> (picks, picked D, status word, level out)."""
    from ec504_imageencoder_amd import _ffi
    K, n = len(S), len(S[0])
    s, d, st = _tables(torch, S, D, status)
    picks = torch.full((max(n, 1),), 255, dtype=torch.uint8, device="cuda")
    pd = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    lin = torch.tensor([level], dtype=torch.int64).cuda()
    lout = lin if same_pointer else torch.full((1,), -12345, dtype=torch.int64, device="cuda")
    rc = _ffi.lib().m1v_rd_cbr_pick_device(enc._h, _p(s), _p(d), _p(st), n, K, rate, cap, _p(lin), _p(lout), _p(picks), _p(pd),
                                           _p(word), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _ffi.last_error()
    torch.cuda.synchronize()
    if not same_pointer:
        assert int(lin.item()) == level
    return picks[:n].cpu().tolist(), pd[:n].cpu().tolist(), int(word.item()) & 0xFFFFFFFF, int(lout.item())


def _check_cbr(torch, enc, S, D, rate, cap, level, status=None, same_pointer=False):
    w_picks, w_over, w_level = M.bitrate_walk(S, D, rate, cap, level, status)
    picks, pd, word, out = _cbr(torch, enc, S, D, rate, cap, level, status, same_pointer)
    assert picks == w_picks
    assert pd == [D[k][f] for f, k in enumerate(w_picks)]
    assert word == (16 if w_over else 0)
    assert out == w_level
    return w_over


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 2, 9, 150, 300, 513])
def test_bitrate_pick_on_random_tables(torch_cuda, enc, n, K):
    """n = 513 crosses the 512 frames staged per step.  A level that starts negative, one above the capacity, one in between;
    rates at which some frames fit nothing and others everything."""
    rng = random.Random(2000 * n + K)
    S, D = _random_table(rng, n, K)
    seen = set()
    for rate, cap, level in ((2, 7, -5), (3, 4, 100), (1, 3, 2), (6, 6, 6), (4, 40, 0)):
        over = _check_cbr(torch_cuda, enc, S, D, rate, cap, level)
        seen.add(bool(over))
    if n >= 9:
        assert seen == {False, True}
    _check_cbr(torch_cuda, enc, S, D, 2, 7, -5, same_pointer=True)       # d_level_out == d_level_in
    _check_cbr(torch_cuda, enc, S, D, 2, 7, -5)                          # and the same result again


def test_bitrate_pick_largest_fitting_record_is_not_the_least_distortion(torch_cuda, enc):
    S = [[10, 10, 10], [20, 20, 20], [30, 30, 30]]
    D = [[50, 50, 50], [5, 60, 40], [40, 5, 45]]
    picks, over, level = M.bitrate_walk(S, D, 25, 30, 30)
    assert picks == [1, 2, 1] and over == []          # frame 0: 30 fits but 20 has less D; frame 2: level 25, 20 fits, D 40
    assert level == 30
    _check_cbr(torch_cuda, enc, S, D, 25, 30, 30)
    for status in ([0, 1, 0], [1, 1, 1], [1, 1, 0]):
        _check_cbr(torch_cuda, enc, S, D, 25, 30, 30, status=status)
        _check_cbr(torch_cuda, enc, S, D, 5, 30, -40, status=status)
    # large values: records near 2^32, D near 2^62, a capacity near 2^62
    S = [[2 ** 32 - 1, 2 ** 31, 7], [2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]]
    D = [[2 ** 62 + 1, 2 ** 62, 5], [2 ** 62, 2 ** 62 - 1, 4]]
    _check_cbr(torch_cuda, enc, S, D, 2 ** 31, 2 ** 62 - 1, 2 ** 33)
    _check_cbr(torch_cuda, enc, S, D, 1, 2 ** 32, -(2 ** 40))


def test_two_chained_bitrate_calls_equal_one(torch_cuda, enc):
    rng = random.Random(9)
    S, D = _random_table(rng, 300, 8)
    rate, cap, level = 3, 9, 1
    whole = _cbr(torch_cuda, enc, S, D, rate, cap, level)
    a = _cbr(torch_cuda, enc, [r[:131] for r in S], [r[:131] for r in D], rate, cap, level)
    b = _cbr(torch_cuda, enc, [r[131:] for r in S], [r[131:] for r in D], rate, cap, a[3])
    assert (a[0] + b[0], a[1] + b[1], a[2] | b[2], b[3]) == whole
    assert whole[:1] + whole[3:] == (M.bitrate_walk(S, D, rate, cap, level)[0], M.bitrate_walk(S, D, rate, cap, level)[2])


def test_python_rd_bitrate_pick(torch_cuda, enc):
    torch = torch_cuda
    rng = random.Random(6)
    S, D = _random_table(rng, 20, 4)
    s, d, _ = _tables(torch, S, D, None)
    level = torch.tensor([-3], dtype=torch.int64).cuda()
    picks, over, out = M.bitrate_walk(S, D, 3, 8, -3)
    assert enc.rd_bitrate_pick(s, d, 3, 8, level) == (picks, over)
    assert int(level.item()) == out
    picks2, over2, out2 = M.bitrate_walk(S, D, 3, 8, out)
    assert enc.rd_bitrate_pick(s, d, 3, 8, level) == (picks2, over2) and int(level.item()) == out2


# ---- 3. the empty batch, argument errors -----------------------------------------------------------------------------------
def test_empty_batch_and_argument_errors(torch_cuda, enc):
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    L = _ffi.lib()
    s, d, _ = _tables(torch, [[1, 2], [3, 4]], [[5, 6], [7, 8]], None)
    picks = torch.full((4,), 9, dtype=torch.uint8, device="cuda")
    pd = torch.full((4,), -9, dtype=torch.int64, device="cuda")
    word = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    lin = torch.tensor([50], dtype=torch.int64).cuda()
    lout = torch.tensor([-9], dtype=torch.int64).cuda()

    def batch(e=enc._h, n=2, K=2, rule=0, s=s, d=d, picks=picks, word=word):
        return L.m1v_rd_batch_pick_device(e, _p(s), _p(d), None, n, K, rule, 5, _p(picks), _p(pd), _p(word), None)

    def cbr(n=2, K=2, rate=2, cap=7, s=s, d=d, picks=picks, word=word, lin=lin, lout=lout):
        return L.m1v_rd_cbr_pick_device(enc._h, _p(s), _p(d), None, n, K, rate, cap, _p(lin), _p(lout), _p(picks), _p(pd), _p(word), None)

    for call in (batch, cbr):
        assert call(n=MAX_FRAMES + 1) == _ffi.E_ARG and call(n=-1) == _ffi.E_ARG
        assert call(K=0) == _ffi.E_ARG and call(K=9) == _ffi.E_ARG
        assert call(s=None) == _ffi.E_ARG and call(d=None) == _ffi.E_ARG and call(picks=None) == _ffi.E_ARG
        assert call(word=None) == _ffi.E_ARG
    assert batch(rule=2) == _ffi.E_ARG and batch(rule=-1) == _ffi.E_ARG
    assert cbr(rate=0) == _ffi.E_ARG and cbr(rate=8) == _ffi.E_ARG and cbr(cap=2 ** 62) == _ffi.E_ARG
    assert cbr(lin=None) == _ffi.E_ARG and cbr(lout=None) == _ffi.E_ARG
    torch.cuda.synchronize()
    untouched = lambda: (picks.cpu().tolist(), pd.cpu().tolist()) == ([9] * 4, [-9] * 4)
    assert untouched() and int(word.item()) == -9 and int(lout.item()) == -9
    # the empty batch: the status word is written as 0 (the bitrate form also moves the level), nothing else
    assert batch(n=0) == 0
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and untouched()
    word.fill_(-9)
    assert cbr(n=0) == 0
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and int(lout.item()) == 7 and int(lin.item()) == 50 and untouched()
