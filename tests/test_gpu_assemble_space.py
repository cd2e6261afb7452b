"""GPU sweep of k_assemble over its placement space (-m gpu): every case of tests/assemble_space.py through Mpeg1Encoder.encode
with caller-owned outputs, against the oracle: the record bytes, the sizes, the total and the status.

Every run first holds the kernel's shape (m1v_debug_assemble_shape) against the plan mirror of the model, forced or not.  The
output lies in a pool of poison bytes with guards on both sides; no guard byte and no byte behind the total may change.  A
second batch with other content runs on the same encoder (the counters the first assembly cleared).  A failure names the frame,
the workgroup, its classes from the model, and the strip and segment of the first differing byte.

One process, one encoder per scene (kept for the module).  No case is built to fault: every shape the hook takes is one the
plan can produce, and the kernel's range checks hold for all of them (tests/test_assemble_space_cpu.py: the model touches no
word outside the image)."""
import numpy as np
import pytest

import assemble_space as A

pytestmark = pytest.mark.gpu

SLACK = 64      # bytes of capacity behind the total in the sweep: they must stay poison


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def rig(torch_cuda, orc):
    """Encoders and uploaded frames, one per scene, for the module."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    encoders, frames = {}, {}

    class Rig:
        torch = torch_cuda

        def encoder(self, sc, **kw):
            if sc.name not in encoders or kw:
                enc = Mpeg1Encoder(sc.W, sc.H, sc.qf, "full", channels=sc.channels, max_frames=kw.get("max_frames", sc.n))
                if sc.path == "runs":
                    enc.debug_set_path("runs")
                if kw:
                    return enc
                encoders[sc.name] = enc
            return encoders[sc.name]

        def frames(self, sc, batch):
            if (sc.name, batch) not in frames:
                frames[sc.name, batch] = torch_cuda.from_numpy(np.array(A.pixels(orc, sc, batch))).cuda()
            return frames[sc.name, batch]

    yield Rig()
    for enc in encoders.values():
        enc.close()


def _pool(torch, total, cap, align):
    pool = torch.full((A.GUARD + 16 + cap + A.GUARD,), A.POISON, dtype=torch.uint8, device="cuda")
    assert pool.data_ptr() % 16 == 0
    lo = A.GUARD + align
    return pool, pool[lo:lo + cap]


def _want_pool(orc, sc, batch, cap, align, frames=None):
    """The pool as it must be afterwards: the records of the first `frames` frames (default all), poison everywhere else."""
    recs = b"".join(A.record(orc, sc, f, batch) for f in range(sc.n if frames is None else frames))
    want = np.full(A.GUARD + 16 + cap + A.GUARD, A.POISON, np.uint8)
    lo = A.GUARD + align
    want[lo:lo + len(recs)] = np.frombuffer(recs, np.uint8)
    return want


def _set_shape(orc, enc, sc, forced):
    """Force the shape and hold what the library reports against the plan mirror; returns the resolved (group, lanes_log2)."""
    enc.debug_set_assemble_shape(*forced)
    got, want = enc.debug_assemble_shape(), A.plan_shape(sc, forced)
    assert got == want, f"{sc.name} forced {forced}: the library plans {got}, the mirror {want}"
    return got[:2]


def _launch(rig, orc, enc, sc, batch, align, cap):
    torch = rig.torch
    total = sum(len(A.record(orc, sc, f, batch)) for f in range(sc.n))
    cap = total + SLACK if cap is None else cap
    pool, out = _pool(torch, total, cap, align)
    sizes = torch.full((sc.n,), -1, dtype=torch.int64, device="cuda")
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")        # (total: 64 bits; the status word: the low 32 of meta[1])
    enc.encode(rig.frames(sc, batch), A.FIRST + 100 * batch, out=out, sizes=sizes, meta=meta, quality=sc.quality)
    return pool, sizes, meta, total, cap


def _check(rig, orc, sc, shape, batch, align, launched, status=0, frames=None):
    pool, sizes, meta, total, cap = launched
    got_total, got_status = (int(x) for x in meta.cpu())
    where = f"{sc.name} shape {shape} align {align} batch {batch}"
    assert got_status & 0xFFFFFFFF == status, (where, "status", got_status)
    assert got_total == total, (where, "total", got_total, total)
    assert [int(x) for x in sizes.cpu()] == [len(A.record(orc, sc, f, batch)) for f in range(sc.n)], (where, "sizes")
    got, want = pool.cpu().numpy(), _want_pool(orc, sc, batch, cap, align, frames)
    if not np.array_equal(got, want):
        lo = A.GUARD + align
        k = int(np.flatnonzero(got != want)[0])
        if k < lo or k >= lo + total:
            pytest.fail(f"{where}: pool byte {k - lo} relative to the output changed to {got[k]:#04x} "
                        f"({'guard in front' if k < lo else 'behind the total'}; total {total}, capacity {cap})")
        pytest.fail(A.describe_difference(orc, sc, shape, got[lo:lo + total].tobytes(), align, batch))


def _run(rig, orc, sc, forced, align=0, batches=(0, 1)):
    enc = rig.encoder(sc)
    shape = _set_shape(orc, enc, sc, forced)
    for batch in batches:
        launched = _launch(rig, orc, enc, sc, batch, align, None)
        enc.flush()
        rig.torch.cuda.synchronize()
        _check(rig, orc, sc, shape, batch, align, launched)
    return shape


# ---- the sweep --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc,forced", A.cases(), ids=[A.case_id(sc, forced) for sc, forced in A.cases()])
def test_case(rig, orc, sc, forced):
    _run(rig, orc, sc, forced)


def test_every_alignment_of_the_output(rig, orc):
    """17 strips in groups of 4 (the plan's own) and of 16: `out` at each of the 16 byte alignments, so every group meets every lead."""
    sc = A.scene(A.ALIGN_SCENE)
    for forced in ((0, 0), (16, 2)):
        for align in range(16):
            _run(rig, orc, sc, forced, align, batches=(0,))


def test_capacity_exactly_the_total_and_one_byte_less(rig, orc):
    """out_cap = total: everything fits.  out_cap = total - 1: STATUS_NOSPACE with the full total and every size reported; every
    record in front of the last is exact; the last frame's range and the guards stay poison."""
    from ec504_imageencoder_amd import _ffi
    sc = A.scene("tiles-sweep")
    enc = rig.encoder(sc)
    for forced in ((0, 0), (16, 1)):
        shape = _set_shape(orc, enc, sc, forced)
        total = sum(len(A.record(orc, sc, f, 0)) for f in range(sc.n))
        for cap, status, frames in ((total, 0, None), (total - 1, _ffi.STATUS_NOSPACE, sc.n - 1)):
            launched = _launch(rig, orc, enc, sc, 0, 3, cap)
            enc.flush()
            rig.torch.cuda.synchronize()
            _check(rig, orc, sc, shape, 0, 3, launched, status, frames)


def test_pipelined_mode_on_the_hardest_cell(rig, orc):
    """>= 2 passes x 2 chunks x long segments under set_pipelined(True): two batches in turn on the two internal buffer sets,
    each into its own pool, compared behind one flush; then each once more (the counter sets alternate)."""
    name, forced = A.HARDEST
    sc = A.scene(name)
    wgs, _ = A.workgroups(orc, sc, A.plan_shape(sc, forced)[:2])
    assert any(w.passes >= 2 and w.chunks >= 2 and any(w.long) for w in wgs)
    enc = rig.encoder(sc)
    shape = _set_shape(orc, enc, sc, forced)
    enc.set_pipelined(True)
    try:
        assert enc.debug_assemble_shape()[:2] == shape
        for _ in range(2):
            launched = [_launch(rig, orc, enc, sc, batch, 0, None) for batch in (0, 1)]
            enc.flush()
            rig.torch.cuda.synchronize()
            for batch in (0, 1):
                _check(rig, orc, sc, shape, batch, 0, launched[batch])
    finally:
        enc.set_pipelined(False)


@pytest.mark.parametrize("which", ["hardest", "window"])
def test_scratch_of_4_gib(rig, orc, which):
    """The same two cells through k_assemble<true> (64-bit source offsets): an encoder of so many frames that its scratch,
    reserved for the worst case, is 4 GiB or more (the rig of tests/test_gpu_state.py, section c, at these small pictures: the
    scratch is allocated, never filled).  The frames of a short batch lie at its start, so the offsets themselves stay small;
    offsets past 2^32 are that test's."""
    name, forced = A.HARDEST if which == "hardest" else A.WINDOW
    sc = A.scene(name)
    per_frame = 23088 * (-(-sc.W // 128)) * (-(-sc.H // 64))        # a compact slot and a worst-case slot per tile, at least
    enc = rig.encoder(sc, max_frames=2 ** 32 // per_frame + 200)
    try:
        enc.reserve_scratch(True)
        assert enc.scratch_bytes() >= 2 ** 32, enc.scratch_bytes()
        shape = _set_shape(orc, enc, sc, forced)
        assert enc.scratch_bytes() >= 2 ** 32
        for batch in (0, 1):
            launched = _launch(rig, orc, enc, sc, batch, 0, None)
            enc.flush()
            rig.torch.cuda.synchronize()
            _check(rig, orc, sc, shape, batch, 0, launched)
    finally:
        enc.close()


def test_refused_hook_arguments_change_nothing(rig, orc):
    """Values the plan cannot produce are M1V_E_ARG, and the next encode is exact with the shape that was in force."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    sc = A.scene("tiles-sweep")                                     # 17 strips
    enc = rig.encoder(sc)
    shape = _set_shape(orc, enc, sc, (8, 2))
    for group, lg in ((3, 0), (32, 0), (-1, 0), (6, 2), (0, 5), (0, -1), (16, 7), (17, 0)):
        with pytest.raises(EncoderError) as ei:
            enc.debug_set_assemble_shape(group, lg)
        assert ei.value.code == _ffi.E_ARG, (group, lg)
        assert enc.debug_assemble_shape()[:2] == (8, 2), (group, lg)
    launched = _launch(rig, orc, enc, sc, 0, 0, None)
    rig.torch.cuda.synchronize()
    _check(rig, orc, sc, shape, 0, 0, launched)
    one = A.scene("one-macroblock")                                 # one strip: no group but 1
    enc = rig.encoder(one)
    with pytest.raises(EncoderError) as ei:
        enc.debug_set_assemble_shape(2, 0)
    assert ei.value.code == _ffi.E_ARG
    _run(rig, orc, one, (1, 4), batches=(0,))
    _run(rig, orc, one, (0, 0), batches=(0,))
