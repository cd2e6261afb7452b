"""Every call on a caller's stream that is not the null stream (-m gpu): include/mpeg1_hip.h promises that the *_device entry points
are asynchronous on `stream`, and a PyTorch caller's streams do not wait for the null stream.

Each case runs on one torch.cuda.Stream S (the two-encoder case on two).  The input buffer holds decoy frames (valid frames whose
oracle records differ from the real ones in every frame: tests/launch_side.py, tests/test_launch_side_cpu.py).  Queued on S without
a wait in between: the outputs are poisoned with 0xA5, the gate (device work of at least 20 ms and 20 times the ungated duration
of the same call, both measured with events and printed), a copy of the real frames over the decoys, the call, copies of every
output.  Then S is waited for once.  A launch, memset or event wait that went to another stream has run while the gate held S
back: it read decoys or left poison, a plain mismatch with the oracle's records and sizes and with the models' picks (rd_oracle,
rd_rate_model, streams_model, the byte rules of tests/test_rate_abi.py).  Where every argument was on the device before the gate,
S.query() must be false when the call returns: the call did not wait for its stream.

The ungated run that measures the call comes first, on the same encoder with the same frames: whatever a mis-ordered kernel could
read has then been written by a correct batch of the same shape.

The library's own streams apart, a test keeps S alive and one more stream at most; nothing here depends on two streams making
progress at the same time."""
import ctypes as C

import numpy as np
import pytest

import frame_axis as fa
import launch_side as LS
import rd_oracle as rd
import rd_rate_model as M
import streams_model as sm
from rate_rules import batch_rule

pytestmark = pytest.mark.gpu

Q = 12
K8 = (1, 2, 4, 6, 8, 10, 11, 12)
FIRST = 250
OVER_BUDGET, OVER_DISTORTION = 16, 32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def side(torch_cuda):
    """(S, the gate): one non-default stream for the module, and the calibrated gate."""
    torch = torch_cuda
    S = torch.cuda.Stream()
    assert S.cuda_stream != 0 and S.cuda_stream != torch.cuda.default_stream().cuda_stream
    gate = LS.Gate(torch)
    print(f"gate: {gate.calibrate(S):.3f} ms per unit of {gate.unit} ({'torch.cuda._sleep' if gate._sleep else 'fill'})")
    return S, gate


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _bytes(t):
    """A contiguous tensor as its bytes, to poison it whatever its type."""
    import torch
    assert t.is_contiguous()
    return t.view(-1).view(torch.uint8)


class Rig:
    """One encoder and its input: `buf` is what the calls take as rgb and holds the decoys; `load(frames)` queues the copy of a
    frame set over it on the current stream."""

    def __init__(self, torch, orc, name):
        from ec504_imageencoder_amd import Mpeg1Encoder
        self.name = name
        kind, W, H, n, mode, path = {
            "tiles": ("packed3", 144, 80, 9, "full", "tiles"),
            "runs": ("packed3", 48, 32, 3, "full", "runs"),
            "strips": ("packed4", 640, 480, 4, "strict", "runs"),
            "frame_table": ("surface3", 144, 80, 9, "full", "tiles"),
        }[name]
        self.W, self.H, self.n, self.mode = W, H, n, mode
        self.channels = 4 if kind == "packed4" else 3
        self.omode = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
        self.decoy, self.real = LS.frame_sets(kind, W, H, n)
        self.enc = Mpeg1Encoder(W, H, Q, mode, channels=self.channels, max_frames=n)
        if name == "runs":
            self.enc.debug_set_path("runs")
        assert self.enc.path == path, (name, self.enc.path)
        self.enc.reserve_scratch(True)      # (no batch exhausts the worst case: STATUS_SCRATCH cannot occur)
        self.dev = {"decoy": torch.from_numpy(self.decoy).cuda(), "real": torch.from_numpy(self.real).cuda()}
        if kind == "surface3":      # rows 16 bytes longer than the picture's, each frame an allocation of its own, named by a table
            pitch = W * 3 + 16
            self.enc.set_input_layout(pitch, H * pitch)
            self.enc.set_frame_table()
            self.surfaces = [torch.zeros((H, pitch), dtype=torch.uint8, device="cuda") for _ in range(n)]
            self.views = [s.as_strided((H, W, 3), (pitch, 3, 1)) for s in self.surfaces]
            self.buf = self.enc.frames(self.views)       # the table: device memory that only kernels read, uploaded here, in front of every gate
        else:
            self.buf = torch.empty_like(self.dev["decoy"])
        self.load("decoy")
        torch.cuda.synchronize()
        self._records = {}
        self.orc = orc

    def load(self, which):
        if hasattr(self, "views"):
            for v, src in zip(self.views, self.dev[which]):
                v.copy_(src)
        else:
            self.buf.copy_(self.dev[which])

    def records(self, qualities=None, first=FIRST, indices=None):
        """The oracle's records of the real frames, each at its own index and quality."""
        qualities = [Q] * self.n if qualities is None else [int(q) for q in qualities]
        indices = [first + f for f in range(self.n)] if indices is None else list(indices)
        key = (tuple(qualities), tuple(indices))
        if key not in self._records:
            self._records[key] = [self.orc.encode_frame(self.real[f], self.W, self.H, indices[f], qualities[f], self.omode, self.channels)
                                  for f in range(self.n)]
        return self._records[key]

    def table(self):
        """(S[k][f], D[k][f]) of the real frames at K8, from the oracle and rd_oracle."""
        if "table" not in self._records:
            s = [[len(self.orc.encode_frame(self.real[f], self.W, self.H, 0, q, self.omode, self.channels)) for f in range(self.n)] for q in K8]
            d = [[rd.frame_distortion(self.orc, self.real[f], self.W, self.H, q, self.omode, self.channels) for f in range(self.n)] for q in K8]
            self._records["table"] = (s, d)
        return self._records["table"]


@pytest.fixture(scope="module")
def rigs(torch_cuda, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(torch_cuda, orc, name)
        return made[name]

    yield get
    for rig in made.values():
        rig.enc.close()


def gated(torch, side, rig, outputs, call, expect_busy=False, stream=None, load=None):
    """The sequence of the module's docstring around call() on S.  outputs: the tensors the call writes (poisoned, snapshot);
    returns (what call() returned, the snapshots)."""
    S, gate = side
    S = stream or S
    load = load or rig.load
    with torch.cuda.stream(S):
        load("real")
    call_ms = gate.measure(S, call)             # ungated, and the correct batch in front of the gated one
    with torch.cuda.stream(S):
        load("decoy")
    S.synchronize()
    with torch.cuda.stream(S):
        for o in outputs:
            _bytes(o).fill_(LS.POISON)
        length = gate(S, LS.gate_ms(call_ms))
        load("real")
        result = call()
        busy = not S.query()
        snaps = [o.clone() for o in outputs]
    S.synchronize()
    print(f"{rig.name if rig else ''}: call {call_ms:.3f} ms ungated, gate {length:.1f} ms, stream busy at return: {busy}")
    assert length >= 20.0 and length >= 20.0 * call_ms
    if expect_busy:
        assert busy, "the call waited for its stream (or the gate had run out when it returned)"
    return result, snaps


def _outputs(torch, enc, n, extra=()):
    out = torch.empty(enc.frame_bound * n, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    meta = torch.empty(2, dtype=torch.int64, device="cuda")
    return [out, sizes, meta, *extra]


def _check_records(snaps, want, what=""):
    out, sizes, meta = snaps[:3]
    total, status = (int(x) for x in meta.cpu())
    want_sizes = [len(r) for r in want]
    assert status & 0xFFFFFFFF == 0, (what, status)
    assert [int(s) for s in sizes.cpu()] == want_sizes, what
    assert total == sum(want_sizes), what
    assert out[:total].cpu().numpy().tobytes() == b"".join(want), f"{what}: the bytes are not the oracle's records of the real frames"


# ---- encodes: the three producers and a layout that is not packed, behind its frame table -----------------------------------------------
@pytest.mark.parametrize("per_frame", [False, True], ids=["own_quality", "per_frame_quality"])
@pytest.mark.parametrize("name", ["tiles", "runs", "strips", "frame_table"])
def test_encode(torch_cuda, orc, side, rigs, name, per_frame):
    torch = torch_cuda
    rig = rigs(name)
    enc, n = rig.enc, rig.n
    qs = [(3 * f) % Q + 1 for f in range(n)] if per_frame else None
    d_q = torch.tensor(qs, dtype=torch.uint8).cuda() if per_frame else None
    outs = _outputs(torch, enc, n)
    torch.cuda.synchronize()

    def call():
        enc.encode(rig.buf, FIRST, out=outs[0], sizes=outs[1], meta=outs[2], quality=d_q)

    _, snaps = gated(torch, side, rig, outs, call, expect_busy=True)
    _check_records(snaps, rig.records(qs), name)


def test_shorter_batch_behind_a_longer_one(torch_cuda, orc, side, rigs):
    """9, 4 and 9 frames back to back behind one gate: the batch of 4 hands over a counter set that the 9 frames in front left
    dirty beyond its own length, which the host clears with memsets on the stream; the third batch adds to that set."""
    torch = torch_cuda
    rig = rigs("tiles")
    enc, n = rig.enc, rig.n
    three = [_outputs(torch, enc, m) for m in (n, 4, n)]
    firsts = (FIRST, FIRST + 1, FIRST + 2)
    torch.cuda.synchronize()

    def call():
        for outs, first, m in zip(three, firsts, (n, 4, n)):
            enc.encode(rig.buf[:m], first, out=outs[0], sizes=outs[1], meta=outs[2])

    _, snaps = gated(torch, side, rig, [o for outs in three for o in outs], call, expect_busy=True)
    for b, (first, m) in enumerate(zip(firsts, (n, 4, n))):
        _check_records(snaps[3 * b:3 * b + 3], rig.records(first=first)[:m], f"batch {b} of {m} frames")


# ---- sizes and tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles", "strips", "frame_table"])
def test_sizes_and_tables(torch_cuda, orc, side, rigs, name):
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    rig = rigs(name)
    enc, n = rig.enc, rig.n
    S_, D_ = rig.table()
    qs = [(5 * f) % Q + 1 for f in range(n)]
    d_q = torch.tensor(qs, dtype=torch.uint8).cuda()
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    word = torch.empty(1, dtype=torch.int32, device="cuda")
    table = torch.empty((len(K8), n), dtype=torch.int64, device="cuda")
    words = torch.empty(len(K8), dtype=torch.int32, device="cuda")
    rd_sizes, rd_dist = torch.empty_like(table), torch.empty_like(table)
    rd_words = torch.empty_like(words)
    qbuf = (C.c_uint8 * len(K8))(*K8)
    L, st = _ffi.lib(), lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def call():
        assert L.m1v_frame_sizes_device(enc._h, _p(rig.buf), n, _p(d_q), _p(sizes), _p(word), st()) == 0, _ffi.last_error()
        assert L.m1v_frame_size_table_device(enc._h, _p(rig.buf), n, qbuf, len(K8), _p(table), _p(words), st()) == 0, _ffi.last_error()
        if enc.size_table_fused:
            assert L.m1v_frame_rd_table_device(enc._h, _p(rig.buf), n, qbuf, len(K8), _p(rd_sizes), _p(rd_dist), _p(rd_words), st()) == 0, _ffi.last_error()

    assert enc.size_table_fused == 1
    _, snaps = gated(torch, side, rig, [sizes, word, table, words, rd_sizes, rd_dist, rd_words], call, expect_busy=True)
    assert snaps[0].tolist() == [len(r) for r in rig.records(qs)] and snaps[1].tolist() == [0], "frame_sizes"
    assert snaps[2].tolist() == S_ and snaps[3].tolist() == [0] * len(K8), "frame_size_table"
    assert snaps[4].tolist() == S_ and snaps[5].tolist() == D_ and snaps[6].tolist() == [0] * len(K8), "frame_rd_table"


# ---- the pick-and-encode calls ---------------------------------------------------------------------------------------------------------
def _limits(S_, D_, rule):
    bound = D_ if rule == rd.SMALLEST_AT_DISTORTION else S_
    return [bound[(3 * f + 1) % len(bound)][f] for f in range(len(S_[0]))]


def _batch_limit(S_, D_, rule, bound):
    """(limit, picks, over): the first limit between the smallest and the largest total of `bound` under which the batch rule's
    picks differ between frames and stay within it."""
    n = len(S_[0])
    lo, hi = (sum(pick(r[f] for r in bound) for f in range(n)) for pick in (min, max))
    for i in (8, 6, 10, 4, 12, 5, 11, 3, 13, 7, 9, 2, 14, 1, 15):
        limit = lo + (hi - lo) * i // 16
        picks, over = M.batch_pick(S_, D_, rule, limit)
        if len(set(picks)) > 1 and not over:
            return limit, picks, over
    raise AssertionError("no limit gives the batch rule picks that differ between frames")


CANDIDATE_CALLS = ("budget", "best_in_budget", "to_distortion", "batch_budget", "best_in_batch_budget", "batch_to_distortion")


@pytest.mark.parametrize("which", CANDIDATE_CALLS)
def test_pick_and_encode(torch_cuda, orc, side, rigs, which):
    """The table, the pick and the encode of one call, all behind the gate, through the C entry point with every argument on the
    device beforehand."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    rig = rigs("tiles")
    enc, n = rig.enc, rig.n
    S_, D_ = rig.table()
    with_dist = which not in ("budget", "batch_budget")
    keep = []
    if which in ("budget", "best_in_budget", "to_distortion"):
        rule = {"budget": fa.LARGEST, "best_in_budget": rd.BEST_IN_BUDGET, "to_distortion": rd.SMALLEST_AT_DISTORTION}[which]
        limits = _limits(S_, D_, rule)
        picks, over = fa.per_frame_model(S_, D_, rule, limits)
        d_limits = torch.tensor(limits, dtype=torch.int64).cuda()
        keep.append(d_limits)
        fn = "m1v_encode_budget_device" if which == "budget" else "m1v_encode_rd_device"
        middle = (0, _p(d_limits)) if which == "budget" else (rule, 0, _p(d_limits))
        bit = (OVER_DISTORTION if which == "to_distortion" else OVER_BUDGET) if over else 0
    elif which == "batch_budget":
        budget = (sum(S_[3]) + sum(S_[4])) // 2
        picks, over = batch_rule(S_, budget)
        fn, middle, bit = "m1v_encode_batch_budget_device", (budget,), OVER_BUDGET if over else 0
    else:
        rule = M.BEST_IN_BUDGET if which == "best_in_batch_budget" else M.SMALLEST_AT_DISTORTION
        bound = S_ if rule == M.BEST_IN_BUDGET else D_
        limit, picks, over = _batch_limit(S_, D_, rule, bound)
        fn, middle = "m1v_encode_rd_batch_device", (rule, limit)
        bit = (OVER_BUDGET if rule == M.BEST_IN_BUDGET else OVER_DISTORTION) if over else 0
    assert len(set(picks)) > 1, "the picks differ between frames"
    chosen = torch.empty(n, dtype=torch.uint8, device="cuda")
    dist = torch.empty(n, dtype=torch.int64, device="cuda") if with_dist else None
    outs = _outputs(torch, enc, n, [chosen] + ([dist] if with_dist else []))
    cbuf = (C.c_uint8 * len(K8))(*K8)
    torch.cuda.synchronize()

    def call():
        args = [enc._h, _p(rig.buf), n, FIRST, cbuf, len(K8), *middle, _p(chosen), _p(outs[0]), outs[0].numel(), _p(outs[1])]
        args += [_p(dist)] if with_dist else []
        rc = getattr(_ffi.lib(), fn)(*args, C.c_void_p(outs[2].data_ptr()), C.c_void_p(outs[2].data_ptr() + 8),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _ffi.last_error()

    _, snaps = gated(torch, side, rig, outs, call, expect_busy=True)
    total, status = (int(x) for x in snaps[2].cpu())
    assert status & 0xFFFFFFFF == bit
    assert snaps[3].tolist() == [K8[k] for k in picks], "the picks"
    if with_dist:
        assert snaps[4].tolist() == [D_[k][f] for f, k in enumerate(picks)], "the picks' distortion"
    want = rig.records([K8[k] for k in picks])
    assert [int(s) for s in snaps[1].cpu()] == [len(r) for r in want] == [S_[k][f] for f, k in enumerate(picks)]
    assert total == sum(len(r) for r in want) and snaps[0][:total].cpu().numpy().tobytes() == b"".join(want)


@pytest.mark.parametrize("by", [fa.BY_SIZE, fa.BY_DISTORTION])
def test_bitrate_level_carried_on_the_device(torch_cuda, orc, side, rigs, by):
    """Two bitrate calls back to back behind one gate, 5 and 4 frames: the second reads the level the first wrote, on the device."""
    from ec504_imageencoder_amd import _ffi
    torch = torch_cuda
    rig = rigs("tiles")
    enc, n, cut = rig.enc, rig.n, 5
    S_, D_ = rig.table()
    rate = sum(S_[4]) // n
    cap, L0 = 2 * rate, rate // 2
    picks, over, after = fa.bitrate_walk(S_, D_, by, rate, cap, L0)
    mid = fa.bitrate_walk(S_, D_, by, rate, cap, L0, 0, cut)[2]
    assert len(set(picks)) > 1 and mid not in (L0, cap)
    with_dist = by == fa.BY_DISTORTION
    fn = "m1v_encode_rd_cbr_device" if with_dist else "m1v_encode_cbr_device"
    level0 = torch.tensor([L0], dtype=torch.int64).cuda()
    levels = torch.empty(3, dtype=torch.int64, device="cuda")       # [0] the start, [1] between the calls, [2] behind them
    chosen = torch.empty(n, dtype=torch.uint8, device="cuda")
    dist = torch.empty(n, dtype=torch.int64, device="cuda") if with_dist else None
    a, b = _outputs(torch, enc, cut), _outputs(torch, enc, n - cut)
    cbuf = (C.c_uint8 * len(K8))(*K8)
    torch.cuda.synchronize()

    def one(lo, count, outs, level_in, level_out):
        args = [enc._h, C.c_void_p(rig.buf.data_ptr() + lo * enc.frame_bytes_in), count, FIRST + lo, cbuf, len(K8), rate, cap,
                C.c_void_p(levels.data_ptr() + 8 * level_in), C.c_void_p(levels.data_ptr() + 8 * level_out),
                C.c_void_p(chosen.data_ptr() + lo), _p(outs[0]), outs[0].numel(), _p(outs[1])]
        args += [C.c_void_p(dist.data_ptr() + 8 * lo)] if with_dist else []
        rc = getattr(_ffi.lib(), fn)(*args, C.c_void_p(outs[2].data_ptr()), C.c_void_p(outs[2].data_ptr() + 8),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _ffi.last_error()

    def call():
        one(0, cut, a, 0, 1)
        one(cut, n - cut, b, 1, 2)

    def load(which):        # the start level travels with the frames: the decoy level is the capacity
        rig.load(which)
        levels[0:1].copy_(level0 if which == "real" else level0 * 0 + cap)

    outs = a + b + [chosen, levels[1:]] + ([dist] if with_dist else [])
    _, snaps = gated(torch, side, rig, outs, call, expect_busy=True, load=load)
    assert snaps[6].tolist() == [K8[k] for k in picks] and snaps[7].tolist() == [mid, after]
    if with_dist:
        assert snaps[8].tolist() == [D_[k][f] for f, k in enumerate(picks)]
    want = rig.records([K8[k] for k in picks])
    for lo, hi, (out, sizes, meta) in ((0, cut, snaps[0:3]), (cut, n, snaps[3:6])):
        total, status = (int(x) for x in meta.cpu())
        assert status & 0xFFFFFFFF == (OVER_BUDGET if any(lo <= f < hi for f in over) else 0)
        assert [int(s) for s in sizes.cpu()] == [len(r) for r in want[lo:hi]]
        assert out[:total].cpu().numpy().tobytes() == b"".join(want[lo:hi])


# ---- the picks alone, on tables the caller holds ---------------------------------------------------------------------------------------
def test_picks_on_held_tables(torch_cuda, orc, side, rigs):
    """m1v_rd_batch_pick_device, m1v_rd_cbr_pick_device and m1v_streams_cbr_pick_device read tables that a copy behind the gate
    puts in the place of the decoy frames' tables."""
    from ec504_imageencoder_amd import _ffi, stream_spans
    torch = torch_cuda
    rig = rigs("tiles")
    enc, n = rig.enc, rig.n
    S_, D_ = rig.table()
    decoy_S = [[len(orc.encode_frame(rig.decoy[f], rig.W, rig.H, 0, q, rig.omode)) for f in range(n)] for q in K8]
    decoy_D = [[rd.frame_distortion(orc, rig.decoy[f], rig.W, rig.H, q, rig.omode) for f in range(n)] for q in K8]
    tables = {"real": (torch.tensor(S_).cuda(), torch.tensor(D_).cuda()), "decoy": (torch.tensor(decoy_S).cuda(), torch.tensor(decoy_D).cuda())}
    d_S, d_D = torch.empty_like(tables["real"][0]), torch.empty_like(tables["real"][1])
    K = len(K8)
    limit, want_batch, _ = _batch_limit(S_, D_, M.BEST_IN_BUDGET, S_)
    rate = sum(S_[4]) // n
    cap, L0 = 2 * rate, rate // 2
    want_walk, _, after = M.bitrate_walk(S_, D_, rate, cap, L0)
    pairs = [(4, 7), (0, 0), (5, 300)]
    spans = sm.spans_of(pairs)
    rates, levels = [(rate, cap), (rate, cap), (rate * 2, rate * 3)], [L0, 5, rate]
    want_streams, want_sdist, after_streams, bits = sm.streams_bitrate(S_, D_, spans, rates, levels, sm.LEAST_DISTORTION)
    assert want_batch != M.batch_pick(decoy_S, decoy_D, M.BEST_IN_BUDGET, limit)[0]
    d_spans = stream_spans(pairs)
    d_rates = torch.tensor(rates, dtype=torch.int64).cuda()
    level_in, levels_in = torch.tensor([L0], dtype=torch.int64).cuda(), torch.tensor(levels, dtype=torch.int64).cuda()
    level_out, levels_out = torch.empty_like(level_in), torch.empty_like(levels_in)
    picks = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    pick_dist = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3)]
    words = [torch.empty(1, dtype=torch.int32, device="cuda") for _ in range(3)]
    L, st = _ffi.lib(), lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def call():
        assert L.m1v_rd_batch_pick_device(enc._h, _p(d_S), _p(d_D), None, n, K, M.BEST_IN_BUDGET, limit, _p(picks[0]), _p(pick_dist[0]),
                                          _p(words[0]), st()) == 0, _ffi.last_error()
        assert L.m1v_rd_cbr_pick_device(enc._h, _p(d_S), _p(d_D), None, n, K, rate, cap, _p(level_in), _p(level_out), _p(picks[1]),
                                        _p(pick_dist[1]), _p(words[1]), st()) == 0, _ffi.last_error()
        assert L.m1v_streams_cbr_pick_device(enc._h, _p(d_S), _p(d_D), None, n, K, _p(d_spans), len(pairs), _ffi.STREAMS_RULES["distortion"],
                                             0, 0, _p(d_rates), _p(levels_in), _p(levels_out), _p(picks[2]), _p(pick_dist[2]), _p(words[2]),
                                             st()) == 0, _ffi.last_error()

    def load(which):
        d_S.copy_(tables[which][0])
        d_D.copy_(tables[which][1])

    load("decoy")
    outs = picks + pick_dist + words + [level_out, levels_out]
    _, snaps = gated(torch, side, rig, outs, call, expect_busy=True, load=load)
    for k, want in enumerate((want_batch, want_walk, want_streams)):
        assert snaps[k].tolist() == want, ("rd_batch_pick", "rd_bitrate_pick", "streams_bitrate_pick")[k]
        assert snaps[3 + k].tolist() == [D_[c][f] for f, c in enumerate(want)]
    assert want_sdist == [D_[c][f] for f, c in enumerate(want_streams)]
    assert snaps[9].tolist() == [after] and snaps[10].tolist() == after_streams
    assert int(snaps[8].item()) & 0xFFFFFFFF == bits


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def test_encode_streams(torch_cuda, orc, side, rigs):
    """m1v_encode_streams_device: k_streams_map in front of the producer and k_streams_finish behind k_assemble."""
    from ec504_imageencoder_amd import stream_spans
    torch = torch_cuda
    rig = rigs("tiles")
    enc, n = rig.enc, rig.n
    pairs = [(4, 7), (0, 0), (5, 300)]
    spans = sm.spans_of(pairs)
    d_spans = stream_spans(pairs)
    stream_bytes = torch.empty(len(pairs), dtype=torch.int64, device="cuda")
    outs = _outputs(torch, enc, n, [stream_bytes])
    torch.cuda.synchronize()

    def call():
        enc.encode_streams_device(rig.buf, d_spans, out=outs[0], sizes=outs[1], meta=outs[2], stream_bytes=stream_bytes)

    _, snaps = gated(torch, side, rig, outs, call, expect_busy=True)
    want = rig.records(indices=sm.frame_indices(spans, n))
    _check_records(snaps, want, "encode_streams_device")
    assert snaps[3].tolist() == sm.stream_bytes(spans, [len(r) for r in want])


@pytest.mark.parametrize("by", [fa.BY_SIZE, fa.BY_DISTORTION])
def test_encode_streams_at_bitrate(torch_cuda, orc, side, rigs, by):
    """The method of Mpeg1Encoder, which waits for S itself: the table, k_streams_bitrate, the encode and k_streams_finish."""
    torch = torch_cuda
    rig = rigs("tiles")
    enc, n = rig.enc, rig.n
    S_, D_ = rig.table()
    rate = sum(S_[4]) // n
    pairs, rates, levels = [(4, 7), (0, 0), (5, 300)], [(rate, 2 * rate), (rate, 2 * rate), (2 * rate, 3 * rate)], [rate // 2, 5, rate]
    spans = sm.spans_of(pairs)
    rule = sm.LARGEST_THAT_FITS if by == fa.BY_SIZE else sm.LEAST_DISTORTION
    picks, want_dist, after, bits = sm.streams_bitrate(S_, D_, spans, rates, levels, rule)
    d_levels = torch.empty(len(pairs), dtype=torch.int64, device="cuda")
    start = torch.tensor(levels, dtype=torch.int64).cuda()
    torch.cuda.synchronize()

    def call():
        d_levels.copy_(start)
        return enc.encode_streams_at_bitrate(rig.buf, pairs, K8, [r for r, _ in rates], [c for _, c in rates], d_levels, by=by)

    (data, sizes, chosen, stream_bytes, over, dist), snaps = gated(torch, side, rig, [], call)
    assert chosen == [K8[k] for k in picks] and d_levels.tolist() == after and over == bool(bits & sm.STATUS_OVER_BUDGET)
    assert dist == (want_dist if by == fa.BY_DISTORTION else None)
    want = rig.records(chosen, indices=sm.frame_indices(spans, n))
    assert data == b"".join(want) and sizes == [len(r) for r in want] and stream_bytes == sm.stream_bytes(spans, sizes)


# ---- the helpers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles", "runs", "strips"])
def test_coefficients_convert_subsample_synth(torch_cuda, orc, side, rigs, name):
    """The tile form of the coefficient kernel (tiles) and the run-shaped k_coefficients (an encoder forced to the run kernels; 4
    channels), k_convert4 with 3 and 4 channels, k_subsample and k_synth."""
    torch = torch_cuda
    rig = rigs(name)
    enc, n, W, H, ch = rig.enc, rig.n, rig.W, rig.H, rig.channels
    coef = torch.empty((n, enc.blocks_per_frame, 64), dtype=torch.int16, device="cuda")
    planes = torch.empty((n, 3, H * W), dtype=torch.uint8, device="cuda")
    sub = [torch.empty((W // 2) * (H // 2), dtype=torch.uint8, device="cuda") for _ in range(2)]
    synth = torch.empty((n, H, W, ch), dtype=torch.uint8, device="cuda")
    from ec504_imageencoder_amd import _ffi
    L, st = _ffi.lib(), lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def call():
        assert L.m1v_coefficients_device(enc._h, _p(rig.buf), n, _p(coef), st()) == 0
        assert L.m1v_convert_device(enc._h, _p(rig.buf), n, _p(planes), st()) == 0
        # the chroma planes of frame 2 that the convert in front wrote: the subsample reads them in stream order
        assert L.m1v_subsample_device(enc._h, C.c_void_p(planes[2, 1].data_ptr()), C.c_void_p(planes[2, 2].data_ptr()), _p(sub[0]), _p(sub[1]), st()) == 0
        assert L.m1v_synth_device(_p(synth), enc.frame_bytes_in, n, 504, FIRST, st()) == 0

    _, snaps = gated(torch, side, rig, [coef, planes, sub[0], sub[1], synth], call, expect_busy=True)
    got = snaps[0].cpu().numpy().astype(np.int32)
    for f in range(n):
        assert np.array_equal(got[f], orc.frame_coefficients(rig.real[f], W, H, Q, rig.omode, ch)), f"coefficients of frame {f}"
        Y, Cb, Cr = orc.convert(rig.real[f], channels=ch)
        assert np.array_equal(snaps[1][f].cpu().numpy(), np.stack([Y, Cb, Cr])), f"planes of frame {f}"
    Y, Cb, Cr = orc.convert(rig.real[2], channels=ch)
    wa, wb = orc.subsample(Cb, Cr, W, H)
    assert np.array_equal(snaps[2].cpu().numpy(), wa) and np.array_equal(snaps[3].cpu().numpy(), wb), "subsample"
    assert np.array_equal(snaps[4].cpu().numpy().reshape(n, -1), orc.synth_frames(n, W, H, seed=504, first_index=FIRST, channels=ch).reshape(n, -1)), "synth"


@pytest.mark.parametrize("layout", ["float_planes", "float_pixels"])
def test_to_bytes(torch_cuda, orc, side, layout):
    """m1v_float_planes_to_bytes_device and m1v_float_pixels_to_bytes_device against the rule of tests/float_planes.py."""
    import float_planes as fp
    from ec504_imageencoder_amd import Mpeg1Encoder
    from ec504_imageencoder_amd.encoder import float_pixel_layout_preset, float_plane_layout_preset
    torch = torch_cuda
    W, H, n = 48, 32, 3
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    sets = {}
    for which, seed in (("decoy", 81), ("real", 82)):
        bits, packed = fp.jitter_noise(seed, n, H, W, "float16")
        x = torch.from_numpy(bits.view(np.float16)).cuda()                     # [n, 3, H, W]
        if layout == "float_pixels":
            x = x.permute(0, 2, 3, 1).contiguous()                             # [n, H, W, 3]
        sets[which] = (x, packed)
    if layout == "float_planes":
        enc.set_float_plane_layout(float_plane_layout_preset(W, H, "rgb", "float16"))
        out = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        want = sets["real"][1].transpose(0, 3, 1, 2)
        to_bytes = enc.float_planes_to_bytes
    else:
        enc.set_float_pixel_layout(float_pixel_layout_preset(W, H, 3, "float16"))
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        want = sets["real"][1]
        to_bytes = enc.float_pixels_to_bytes
    buf = sets["decoy"][0].clone()
    torch.cuda.synchronize()
    rig = type("R", (), {"name": layout})()
    _, snaps = gated(torch, side, rig, [out], lambda: to_bytes(buf, out=out), expect_busy=True, load=lambda which: buf.copy_(sets[which][0]))
    assert np.array_equal(snaps[0].cpu().numpy(), want)
    assert not np.array_equal(sets["decoy"][1], sets["real"][1])
    enc.close()


# ---- pipelined mode --------------------------------------------------------------------------------------------------------------------
def test_pipelined_batches_complete_behind_flush(torch_cuda, orc, side, rigs):
    """Three batches back to back in pipelined mode (the assembly runs on the library's stream behind an event), the snapshots
    behind flush() on S; then the switch back to the plain mode, and one more exact call."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    proto = rigs("tiles")
    n, W, H = proto.n, proto.W, proto.H
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    rig = type("R", (), {"name": "pipelined"})()
    buf = proto.dev["decoy"].clone()
    three = [_outputs(torch, enc, n) for _ in range(3)]
    firsts = (FIRST, FIRST + n, 3)
    enc.set_pipelined(True)
    torch.cuda.synchronize()

    def call():
        for outs, first in zip(three, firsts):
            enc.encode(buf, first, out=outs[0], sizes=outs[1], meta=outs[2])
        enc.flush()

    try:
        _, snaps = gated(torch, side, rig, [o for outs in three for o in outs], call, expect_busy=True, load=lambda which: buf.copy_(proto.dev[which]))
        for b, first in enumerate(firsts):
            _check_records(snaps[3 * b:3 * b + 3], proto.records(first=first), f"pipelined batch {b}")
    finally:
        torch.cuda.synchronize()
        enc.set_pipelined(False)
    outs = _outputs(torch, enc, n)
    _, snaps = gated(torch, side, rig, outs, lambda: enc.encode(buf, FIRST, out=outs[0], sizes=outs[1], meta=outs[2]), expect_busy=True,
                     load=lambda which: buf.copy_(proto.dev[which]))
    _check_records(snaps, proto.records(), "back in the plain mode")
    enc.close()


# ---- a failed call, then an exact one ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_exact_call_behind_a_failed_one(torch_cuda, orc, side, rigs, stage):
    """m1v_debug_fail_encode(stage): the call returns M1V_E_HIP after it took a counter set; the next call clears both sets on S
    and is exact, all of it behind the gate."""
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder, _ffi
    torch = torch_cuda
    proto = rigs("tiles")
    n = proto.n
    enc = Mpeg1Encoder(proto.W, proto.H, Q, "full", max_frames=n)
    rig = type("R", (), {"name": f"fail stage {stage}"})()
    buf = proto.dev["decoy"].clone()
    lost, outs = _outputs(torch, enc, n), _outputs(torch, enc, n)
    torch.cuda.synchronize()

    def call():
        _ffi.lib().m1v_debug_fail_encode(stage)
        try:
            with pytest.raises(EncoderError) as err:
                enc.encode(buf, FIRST, out=lost[0], sizes=lost[1], meta=lost[2])
            assert err.value.code == _ffi.E_HIP
        finally:
            _ffi.lib().m1v_debug_fail_encode(0)
        enc.encode(buf, FIRST, out=outs[0], sizes=outs[1], meta=outs[2])

    _, snaps = gated(torch, side, rig, outs, call, expect_busy=True, load=lambda which: buf.copy_(proto.dev[which]))
    _check_records(snaps, proto.records(), f"behind a failure at stage {stage}")
    enc.close()


def _ungated_encode_ms(torch, gate, S, enc, dev, first=0):
    """The device time of one encode of dev on S with nothing in front of it, between two events."""
    n = dev.shape[0]
    outs = _outputs(torch, enc, n)
    return gate.measure(S, lambda: enc.encode(dev, first, out=outs[0], sizes=outs[1], meta=outs[2]))


def _retry_gate(torch, side, enc, dev, what):
    """The gate in front of a step loop whose first batch is encoded twice: sized by the ungated encode of the same batch on this
    encoder as the loop finds it (forced LDS image, default arena: the batch that runs out of scratch) and on a twin with the
    worst case reserved (what the retry runs, every unit in the arena), whichever is longer.  Queues it on S; returns its length."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    S, gate = side
    n = dev.shape[0]
    twin = Mpeg1Encoder(enc.width, enc.height, Q, "full", max_frames=n)
    twin.debug_set_lds_words(8)
    twin.reserve_scratch(True)
    first_ms, retry_ms = _ungated_encode_ms(torch, gate, S, enc, dev), _ungated_encode_ms(torch, gate, S, twin, dev)
    torch.cuda.synchronize()
    twin.close()
    call_ms = max(first_ms, retry_ms)
    length = gate(S, LS.gate_ms(call_ms))
    print(f"{what}: encode {first_ms:.3f} ms ungated (default arena), {retry_ms:.3f} ms (worst case reserved), gate {length:.1f} ms")
    assert length >= 20.0 and length >= 20.0 * call_ms
    return length


# ---- delivery to the host, and its retry -------------------------------------------------------------------------------------------------
def test_host_delivery_and_its_retry(torch_cuda, orc, side):
    """HostDelivery.step on S: three batches, the first of which runs out of overflow scratch behind the gate (a forced LDS image
    of 8 words and the default arena) and is encoded again, with the worst case reserved, behind the batch already queued."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    from ec504_imageencoder_amd.delivery import HostDelivery
    torch = torch_cuda
    S, gate = side
    W, H, n = 1280, 720, 24            # (the shape at which the suite forces the retry: tests/test_gpu_parity.py)
    enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
    enc.debug_set_lds_words(8)
    hd = HostDelivery(enc, n)
    before = enc.scratch_bytes()
    host = [orc.synth_frames(n, W, H, seed=90 + k).reshape(n, H, W, 3) for k in range(4)]
    real = [torch.from_numpy(h).cuda() for h in host[:3]]
    decoy = torch.from_numpy(host[3]).cuda()
    bufs = [decoy.clone() for _ in range(3)]
    wants = [orc.encode_frames(host[k], n, W, H, 10 * k, Q, orc.MODE_FULL, threads=16)[0] for k in range(3)]
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(S):
        _retry_gate(torch, side, enc, real[0], "host delivery")
        for k in range(3):
            bufs[k].copy_(real[k])
            hd.step(bufs[k], 10 * k)    # (waits on the host for the 16 bytes of the batch in front: the gate ends under the second step)
            if hd.last is not None and len(got) < k:
                hd.delivered[hd.last[0]].synchronize()
                got.append(bytes(hd.result().numpy()))
        hd.fence()
        got.append(bytes(hd.result().numpy()))
    S.synchronize()
    print(f"host delivery: scratch {before} bytes before, {enc.scratch_bytes()} afterwards")
    assert got == wants
    assert enc.scratch_bytes() > before, "the step reserved the worst case: a batch ran out of overflow scratch and was encoded again"
    hd.close()
    enc.close()


def test_step_pipeline_retry_on_a_side_stream(torch_cuda, orc, side):
    """The same forced retry through sharding.StepPipeline, world 1, with the step loop on S behind the gate: the exchange and
    the retry run on the pipeline's own side stream, ordered behind S by events."""
    import socket
    import torch.distributed as dist
    from ec504_imageencoder_amd import Mpeg1Encoder
    from ec504_imageencoder_amd.sharding import StepPipeline
    torch = torch_cuda
    S, gate = side
    W, H, n, steps = 1280, 720, 12, 3
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        enc = Mpeg1Encoder(W, H, Q, "full", max_frames=n)
        enc.debug_set_lds_words(8)
        cap = enc.default_out_capacity(n)
        outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
        metas = [torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2)]
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        h_outs = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        h_metas = [torch.zeros(2, dtype=torch.int64, pin_memory=True) for _ in range(2)]
        host_frames = [orc.synth_frames(n, W, H, seed=300 + k).reshape(n, H, W, 3) for k in range(steps + 1)]
        real = [torch.from_numpy(h).cuda() for h in host_frames[:steps]]
        bufs = [torch.from_numpy(host_frames[steps]).cuda().clone() for _ in range(steps)]      # decoys
        state = {"step": 0, "held": {}}
        torch.cuda.synchronize()

        def encode(b, k=None):
            k = state["step"] if k is None else k
            state["held"][b] = k
            bufs[k].copy_(real[k])
            enc.encode(bufs[k], 100 * k, out=outs[b], sizes=sizes, meta=metas[b])
            h_metas[b].copy_(metas[b], non_blocking=True)
            h_outs[b].copy_(outs[b], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            if k == state["step"]:
                state["step"] += 1

        def retry(b):
            enc.reserve_scratch(True)
            encode(b, state["held"][b])

        host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        got = []
        with torch.cuda.stream(S):
            pipe = StepPipeline(encode, h_outs, h_metas, 1, 0, transport="host", host_buffer=host, retry=retry)
            _retry_gate(torch, side, enc, real[0], "step pipeline")
            for k in range(steps):
                pipe.step()
                if pipe.last_counts is not None and len(got) < k:
                    got.append(bytes(host[:pipe.last_counts[0]].numpy()))
            pipe.fence()
            got.append(bytes(pipe.result().numpy()))
        print(f"step pipeline: retries {pipe.retries}")
        assert pipe.retries >= 1
        wants = [orc.encode_frames(host_frames[k], n, W, H, 100 * k, Q, orc.MODE_FULL, threads=16)[0] for k in range(steps)]
        assert got == wants
        enc.close()
    finally:
        dist.destroy_process_group()


# ---- two encoders on two streams ---------------------------------------------------------------------------------------------------------
def test_two_encoders_on_two_streams(torch_cuda, orc, side, rigs):
    """Interleaved calls of two encoders, each on its own stream behind its own gate, with no wait between them: independent
    encoders share no device state."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    torch = torch_cuda
    S, gate = side
    T = torch.cuda.Stream()
    proto = rigs("tiles")
    n, W, H = proto.n, proto.W, proto.H
    encs = [Mpeg1Encoder(W, H, Q, "full", max_frames=n) for _ in range(2)]
    bufs = [proto.dev["decoy"].clone() for _ in range(2)]
    rounds = 3
    outs = [[_outputs(torch, e, n) for _ in range(rounds)] for e in encs]
    flat = [o for per in outs for three in per for o in three]
    call_ms = []
    for e, st in enumerate((S, T)):     # each encoder's three calls ungated, on its stream, with the real frames
        with torch.cuda.stream(st):
            bufs[e].copy_(proto.dev["real"])
        call_ms.append(gate.measure(st, lambda: [encs[e].encode(bufs[e], FIRST + 7 * r + e, out=o[0], sizes=o[1], meta=o[2])
                                                 for r, o in enumerate(outs[e])]))
        with torch.cuda.stream(st):
            bufs[e].copy_(proto.dev["decoy"])
    torch.cuda.synchronize()
    for o in flat:
        _bytes(o).fill_(LS.POISON)
    torch.cuda.synchronize()
    snaps = [[], []]
    lengths = [gate(st, LS.gate_ms(ms)) for st, ms in zip((S, T), call_ms)]
    for e, st in enumerate((S, T)):
        with torch.cuda.stream(st):
            bufs[e].copy_(proto.dev["real"])
    for r in range(rounds):             # S, T, S, T, ...: every call of one encoder between two of the other
        for e, st in enumerate((S, T)):
            with torch.cuda.stream(st):
                o = outs[e][r]
                encs[e].encode(bufs[e], FIRST + 7 * r + e, out=o[0], sizes=o[1], meta=o[2])
                snaps[e].append([x.clone() for x in o])
    busy = [not st.query() for st in (S, T)]
    S.synchronize()
    T.synchronize()
    print(f"two encoders: three calls {call_ms[0]:.3f} and {call_ms[1]:.3f} ms ungated, gates {lengths[0]:.1f} and {lengths[1]:.1f} ms, "
          f"streams busy when the last call returned: {busy}")
    assert all(g >= 20.0 and g >= 20.0 * ms for g, ms in zip(lengths, call_ms))
    for e in range(2):
        for r in range(rounds):
            _check_records(snaps[e][r], proto.records(first=FIRST + 7 * r + e), f"encoder {e}, call {r}")
    for enc in encs:
        enc.close()
