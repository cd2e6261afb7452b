"""GPU parity tests proper (-m gpu): the HIP path, called through the C-ABI of include/mpeg1_hip.h,
against the oracle on the same seeded inputs and against the committed golden vectors.
Bar: bit-exact (integer / byte work; the fp64 colour conversion is truncated to u8)."""
import hashlib
import struct

import os

import numpy as np
import pytest

import golden_io as G
from colour_content import _CH, _COLOURS_PER_FRAME, _CW, _flat_cell_frames, _tie_colours
# the hard-content generators live in tests/hard_content.py
from hard_content import _ZIGZAG, _emitted_levels, _heavy_picture, extreme_pattern_picture  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _enc(W, H, qf=12, mode="full", channels=3, max_frames=8):
    from ec504_imageencoder_amd import Mpeg1Encoder
    return Mpeg1Encoder(W, H, qf, mode, channels=channels, max_frames=max_frames)


def _omode(orc, mode):
    return orc.MODE_FULL if mode == "full" else orc.MODE_STRICT


def test_library_is_the_hip_build(torch_cuda):
    from ec504_imageencoder_amd import _ffi
    assert _ffi.lib().m1v_device_count() >= 1
    maps = open("/proc/self/maps").read()
    assert "ec504_imageencoder_amd/libencoder.so" in maps


def test_synth_matches_oracle_definition(torch_cuda, orc):
    for W, H, C in ((16, 16, 3), (33, 7, 3), (352, 288, 3), (5, 3, 4)):
        enc_geom = _enc(max(W, 16), max(H, 16), channels=C)  # only used for its synth helper signature
        enc_geom.width, enc_geom.height, enc_geom.frame_bytes_in = W, H, W * H * C
        got = enc_geom.synth(3, seed=77, first_frame_index=9).cpu().numpy()
        assert np.array_equal(got, orc.synth_frames(3, W, H, seed=77, first_index=9, channels=C))
        enc_geom.close()


def test_colour_conversion_exhaustive_2_24(torch_cuda, orc):
    """Every RGB triple through k_convert vs the oracle AND vs the reference-generated SHA-256."""
    torch = torch_cuda
    want = G.load_json("colour_exhaustive.json")["sha256"]
    enc = _enc(4096, 4096)  # 2^24 pixels in one frame
    v = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
    rgb = torch.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).to(torch.uint8).reshape(1, 4096, 4096, 3).contiguous()
    planes = enc.convert(rgb).cpu().numpy()[0]
    got = [hashlib.sha256(planes[i].tobytes()).hexdigest() for i in range(3)]
    assert got == [want["Y"], want["Cb"], want["Cr"]]
    enc.close()


# ---- colour conversion INSIDE the encode kernels (image_processing.c:104-106) ------------------------------------


def _check_colours_through(torch, orc, colours, configure, channels=3, chunk=48):
    enc = _enc(_CW, _CH, 50, "full", channels=channels, max_frames=chunk)
    configure(enc)
    per = _COLOURS_PER_FRAME * chunk
    for lo in range(0, len(colours), per):
        frames = _flat_cell_frames(colours[lo:lo + per], channels)
        n = frames.shape[0]
        want, wsizes = orc.encode_frames(frames, n, _CW, _CH, 0, 50, orc.MODE_FULL, channels=channels, threads=16)
        got, sizes = enc.encode_to_bytes(torch.from_numpy(frames).cuda(), 0)
        assert sizes == [int(x) for x in wsizes] and got == want, f"colours {lo}..{lo + per}"
    enc.close()


_INPUT_MODES = {
    "tiles": (3, lambda e: e.debug_set_path("tiles")),                     # LDS-DMA tiles (the default path)
    "runs-aligned": (3, lambda e: e.debug_set_path("runs")),               # 24-byte row loads
    "runs-funnel": (3, lambda e: e.debug_set_input_mode(2)),               # 28-byte loads + v_alignbyte
    "runs-bytes": (3, lambda e: e.debug_set_input_mode(0)),                # byte loads, per-pixel branch
    "runs-rgba": (4, lambda e: None),                                      # 32-byte rows of 4-channel pixels
}


@pytest.mark.parametrize("mode", list(_INPUT_MODES))
def test_colour_inside_the_encode_kernels_ties_and_sample(torch_cuda, orc, mode):
    """All tie / near-tie colours (every input that takes the fp64 branch, ~1 % of 2^24) and 2^20 random colours (2^17
    for the byte-load mode) through each input mode of the encode kernels, as Y, Cb and Cr each."""
    channels, configure = _INPUT_MODES[mode]
    ties = _tie_colours()
    assert 50000 < len(ties) < 400000
    rng = np.random.default_rng(2024)
    sample = rng.integers(0, 256, ((1 << 17) if mode == "runs-bytes" else (1 << 20), 3), dtype=np.uint8)
    _check_colours_through(torch_cuda, orc, np.concatenate([ties, sample]), configure, channels)


@pytest.mark.parametrize("path", ["tiles", "runs"])
def test_colour_inside_the_encode_kernels_exhaustive_2_24(torch_cuda, orc, path):
    """Every one of the 2^24 RGB triples through each encode kernel, coded as Y, Cb and Cr (4096 flat-cell frames)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    colours = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8)
    _check_colours_through(torch_cuda, orc, colours, lambda e: e.debug_set_path(path))


# What each case of the test below reaches in k_assemble, as tests/assemble_space.py's model derives it from the oracle and as
# the test asserts it (the shape through m1v_debug_assemble_shape).  Noise codes 13 to 30 bits per block at any quality (the
# reference's walk stops at the first pair of adjacent non-zero coefficients), so no strip of noise outgrows the 14-KiB image:
# the cases once labelled "several passes" and "three chunks" took one of each under the shape the plan chooses, and the two
# 128 x 4368 cases now force the 8 strips per workgroup their labels assumed.  tests/test_gpu_assemble_space.py sweeps the space.
#   key (W, H, qf, path): forced group (plan: the shape the plan chose where one is forced: 138 and 69 segments, one chunk), then the
#   shape, passes, chunks and long-loop trips the model must find
_ASSEMBLE_CLAIMS = {
    (1920, 1080, 100, "tiles"): dict(force=0, shape=(1, 4, 17, "tiles"), passes={1}, chunks={1}, trips=0),
    (1920, 1080, 90, "runs"): dict(force=0, shape=(1, 4, 3, "dense"), passes={1}, chunks={1}, trips=1),
    (128, 4368, 12, "tiles"): dict(force=8, plan=(2, 3, 69, "tiles"), shape=(8, 3, 69, "tiles"), passes={3}, chunks={3}, trips=0),
    (128, 4368, 75, "tiles"): dict(force=8, plan=(1, 4, 69, "tiles"), shape=(8, 4, 69, "tiles"), passes={2}, chunks={3}, trips=0),
    (640, 480, 50, "auto"): dict(force=0, shape=(4, 4, 1, "strips"), passes={1}, chunks={1}, trips=0),
    (4112, 160, 30, "tiles"): dict(force=0, shape=(16, 4, 3, "tiles"), passes={1}, chunks={1}, trips=0),
    (16, 16, 12, "tiles"): dict(force=0, shape=(1, 3, 1, "tiles"), passes={1}, chunks={1}, trips=0),
}


@pytest.mark.parametrize("W,H,channels,mode,qf,n,path", [
    (1920, 1080, 3, "full", 100, 2, "tiles"),    # one strip per workgroup, 17 segments of ~12 words: one pass, no long segment
    (1920, 1080, 3, "full", 90, 2, "runs"),      # the run kernel's long segments (64 words and more per lane group: the extra loop)
    (128, 4368, 3, "full", 12, 3, "tiles"),      # 69 tile rows x 8 strips (forced) = 552 segments in one group: three CHUNKS, three passes
    (128, 4368, 3, "full", 75, 2, "tiles"),      # ... with 16 lanes per segment: three chunks, two passes
    (640, 480, 4, "strict", 50, 5, "auto"),      # 4 channels, 54 blocks per strip: the strip-per-workgroup kernel, one segment per strip
    (4112, 160, 3, "full", 30, 2, "tiles"),      # 257 strips: 17 groups, the last of one strip; start codes wrap at 256
    (16, 16, 3, "full", 12, 7, "tiles"),         # one macroblock per frame
])
def test_assemble_kernel_passes_chunks_and_long_segments(torch_cuda, orc, W, H, channels, mode, qf, n, path):
    """k_assemble (csrc/m1v_assemble.h) outside the shape the host sizes it for: groups whose bytes outgrow the LDS image
    (passes), groups of more than 256 segments (chunks), segments longer than their lanes' first trip, the three producers of
    segment tables (tiles, runs, strips), every frame's size and the total against the oracle, and a second batch on the same
    encoder (the counters the first batch's assembly cleared).  What each case reaches is asserted, not assumed
    (_ASSEMBLE_CLAIMS): the shape as the library reports it, the classes as the model derives them from the oracle."""
    import assemble_space as A
    torch = torch_cuda
    claim = _ASSEMBLE_CLAIMS[W, H, qf, path]
    enc = _enc(W, H, qf, mode, channels=channels, max_frames=n)
    if path != "auto":
        enc.debug_set_path(path)
    sc = A.Scene("parity", W, H, channels, qf, "runs" if path == "runs" else None, n, 0, (256,) * n, None, ((0, 0),), "", mode)
    planned = enc.debug_assemble_shape()                   # what the plan chooses, before anything is forced
    assert planned == A.plan_shape(sc) and (planned == claim["shape"] or planned == claim.get("plan"))
    enc.debug_set_assemble_shape(claim["force"], 0)
    assert enc.debug_assemble_shape() == A.plan_shape(sc, (claim["force"], 0)) == claim["shape"]
    rng = np.random.default_rng(W * 31 + H + qf)
    for first in (0, 250):
        rgb = rng.integers(0, 256, (n, H, W, channels), dtype=np.uint8)
        if first == 0:
            wgs, _ = A.workgroups(orc, sc, claim["shape"][:2], px=rgb)
            got = ({w.passes for w in wgs}, {w.chunks for w in wgs}, max(max(w.trips) for w in wgs))
            assert got == (claim["passes"], claim["chunks"], claim["trips"]), got
        want, wsizes = orc.encode_frames(rgb, n, W, H, first, qf, _omode(orc, mode), channels=channels)
        got, sizes = enc.encode_to_bytes(torch.from_numpy(rgb).cuda(), first)
        assert sizes == [int(x) for x in wsizes], (first, sizes[:3], list(wsizes[:3]))
        assert got == want, first
    enc.close()


@pytest.mark.parametrize("path", ["tiles", "runs"])
def test_failed_reconfiguration_leaves_the_encoder_usable(torch_cuda, orc, path):
    """m1v_reserve_scratch allocates the worst-case arena, m1v_set_pipelined a second set of buffers; when one of those
    allocations fails (injected) the call reports M1V_E_HIP and the encoder keeps its previous scratch, geometry and
    mode: the next batch encodes correctly, and a later reservation succeeds."""
    from ec504_imageencoder_amd import EncoderError, _ffi
    W, H, n = 352, 288, 3
    enc = _enc(W, H, max_frames=n)
    enc.debug_set_path(path)
    rgb = enc.synth(n, seed=31)
    want, _ = orc.encode_frames(rgb.cpu().numpy(), n, W, H, 7, 12, orc.MODE_FULL)
    assert enc.encode_to_bytes(rgb, 7)[0] == want
    before = enc.scratch_bytes()
    # (what fails: the only allocation of the arena reservation; the second of the three that pipelined mode needs)
    for nth, reconfigure in ((1, lambda: enc.reserve_scratch(True)), (2, lambda: enc.set_pipelined(True))):
        _ffi.lib().m1v_debug_fail_alloc(nth)
        with pytest.raises(EncoderError) as ei:
            reconfigure()
        assert ei.value.code == _ffi.E_HIP
        _ffi.lib().m1v_debug_fail_alloc(0)
        assert enc.scratch_bytes() == before and enc.path == path
        assert enc.encode_to_bytes(rgb, 7)[0] == want
    enc.reserve_scratch(True)
    assert enc.scratch_bytes() > before
    assert enc.encode_to_bytes(rgb, 7)[0] == want
    # a switch of the encode kernel allocates the other path's scratch, segment table, run metadata / tile order: whichever of
    # them fails, the encoder stays on the path it was on — and a forced LDS image that cannot be set up leaves the old one
    other = "runs" if path == "tiles" else "tiles"
    for nth in (1, 2, 3):
        before = enc.scratch_bytes()
        _ffi.lib().m1v_debug_fail_alloc(nth)
        try:
            enc.debug_set_path(other)
            failed = False
        except EncoderError as err:
            failed = True
            assert err.code == _ffi.E_HIP
        _ffi.lib().m1v_debug_fail_alloc(0)
        if failed:
            assert enc.path == path and enc.scratch_bytes() == before
            assert enc.encode_to_bytes(rgb, 7)[0] == want
        else:                       # fewer than nth allocations were needed: the switch went through
            assert enc.path == other and enc.encode_to_bytes(rgb, 7)[0] == want
            enc.debug_set_path(path)
    _ffi.lib().m1v_debug_fail_alloc(1)
    with pytest.raises(EncoderError):
        enc.debug_set_lds_words(8)
    _ffi.lib().m1v_debug_fail_alloc(0)
    assert enc.encode_to_bytes(rgb, 7)[0] == want
    enc.close()


def test_host_delivery_retries_a_batch_that_ran_out_of_scratch(torch_cuda, orc):
    """A forced tiny LDS image sends every unit to the overflow arena, which the default reservation cannot hold: the batch
    reports M1V_STATUS_SCRATCH.  HostDelivery (and StepPipeline, world 1, below) reserve the worst case and encode the same
    frames again behind the batch that is already queued; what is delivered is the oracle's stream."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    W, H, n = 1280, 720, 24
    enc = _enc(W, H, max_frames=n)
    enc.debug_set_lds_words(8)
    hd = HostDelivery(enc, n)
    batches = [enc.synth(n, seed=90 + k) for k in range(3)]
    wants = [orc.encode_frames(b.cpu().numpy(), n, W, H, 10 * k, 12, orc.MODE_FULL)[0] for k, b in enumerate(batches)]
    got = []
    for k, b in enumerate(batches):
        hd.step(b, 10 * k)
        if hd.last is not None and len(got) < k:
            hd.delivered[hd.last[0]].synchronize()
            got.append(bytes(hd.result().numpy()))
    hd.fence()
    got.append(bytes(hd.result().numpy()))
    assert got == wants
    hd.close()
    enc.close()


def test_step_pipeline_retry_with_the_real_encoder(torch_cuda, orc):
    """The N > 1 step loop (sharding.StepPipeline, as bench.py --backend gloo drives it: blobs staged through pinned host memory)
    with the REAL encoder as producer, world 1: a forced tiny LDS image makes the first batch run out of overflow scratch
    (M1V_STATUS_SCRATCH travels with the byte count), the rank reserves the worst case and encodes the same frames again, and
    what is gathered for every step is the oracle's stream."""
    import socket
    import torch.distributed as dist
    from ec504_imageencoder_amd.sharding import StepPipeline
    torch = torch_cuda
    W, H, n, steps = 1280, 720, 12, 4
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        enc = _enc(W, H, max_frames=n)
        enc.debug_set_lds_words(8)
        cap = enc.default_out_capacity(n)
        outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
        metas = [torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2)]
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        h_outs = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        h_metas = [torch.zeros(2, dtype=torch.int64, pin_memory=True) for _ in range(2)]
        batches = [enc.synth(n, seed=300 + k) for k in range(steps)]
        state = {"step": 0, "held": {}}

        def encode(b, k=None):
            k = state["step"] if k is None else k
            state["held"][b] = k
            enc.encode(batches[k], 100 * k, out=outs[b], sizes=sizes, meta=metas[b])
            h_metas[b].copy_(metas[b], non_blocking=True)
            h_outs[b].copy_(outs[b], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            if k == state["step"]:
                state["step"] += 1

        def retry(b):
            enc.reserve_scratch(True)
            encode(b, state["held"][b])

        host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        pipe = StepPipeline(encode, h_outs, h_metas, 1, 0, transport="host", host_buffer=host, retry=retry)
        got = []
        for k in range(steps):
            pipe.step()
            if pipe.last_counts is not None and len(got) < k:
                got.append(bytes(host[:pipe.last_counts[0]].numpy()))
        pipe.fence()
        got.append(bytes(pipe.result().numpy()))
        assert pipe.retries >= 1
        wants = [orc.encode_frames(b.cpu().numpy(), n, W, H, 100 * k, 12, orc.MODE_FULL)[0] for k, b in enumerate(batches)]
        assert got == wants
        enc.close()
    finally:
        dist.destroy_process_group()


def test_bench_starts_its_own_ranks(torch_cuda):
    """`python bench.py --gpus 2` as the driver runs it (no torchrun around it): bench.py starts torch.distributed.run as a child
    and prints ONE JSON line with n_gpus 2.  Rehearsal on this one-GPU box: gloo, both ranks on cuda:0."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1",
                        "--frames", "8", "--width", "352", "--height", "288", "--settle-ms", "0", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["global_frames"] == 16 and d["value"] > 0
    assert "step_frac" in d["roofline"]


def test_c_caller_of_the_delivery(torch_cuda, orc, tmp_path):
    """tests/delivery_main.c: a main.c-style caller in plain C (no HIP headers) drives m1v_delivery_* — five batches of
    different synthetic frames, every batch's records copied to pinned host memory under the next batch's encode and
    appended to a file.  The file is the oracle's stream of the same 5 x n frames."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "delivery_main")
    lib_dir = os.path.join(root, "ec504_imageencoder_amd")
    subprocess.run(["gcc", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "delivery_main.c"), "-o", exe,
                    "-L" + lib_dir, "-lencoder", "-Wl,-rpath," + lib_dir], check=True)
    W, H, n, batches = 352, 288, 4, 5
    out = str(tmp_path / "v.mpeg")
    p = subprocess.run([exe, str(W), str(H), str(n), str(batches), out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    frames = orc.synth_frames(n * batches, W, H, seed=504)
    want = orc.encode_sequence(frames, n * batches, W, H, 12, orc.MODE_FULL)
    assert open(out, "rb").read() == want


def test_host_delivery_overlapped_with_the_next_encode(torch_cuda, orc):
    """HostDelivery: batch k's records travel to pinned host memory on a side stream while batch k+1 encodes.  Five
    batches of DIFFERENT frames through two buffers: what arrives on the host is the oracle's stream, every time."""
    from ec504_imageencoder_amd.delivery import HostDelivery
    W, H, n = 352, 288, 3
    enc = _enc(W, H, max_frames=n)
    hd = HostDelivery(enc, n)
    batches = [enc.synth(n, seed=70 + k) for k in range(5)]
    wants = [orc.encode_frames(b.cpu().numpy(), n, W, H, 100 * k, 12, orc.MODE_FULL)[0] for k, b in enumerate(batches)]
    got = []
    for k, b in enumerate(batches):
        hd.step(b, 100 * k)
        if hd.last is not None and len(got) < k:      # batch k-1 was delivered behind the encode of batch k
            hd.delivered[hd.last[0]].synchronize()
            got.append(bytes(hd.result().numpy()))
    hd.fence()
    got.append(bytes(hd.result().numpy()))
    assert got == wants
    hd.close()
    enc.close()


def test_path_policy(torch_cuda, orc):
    """Every 3-channel picture takes the tile kernel, whatever its width and the alignment of its buffer; 4-channel input and
    the run kernel's tuning hooks (a forced run length or input mode) take the run kernel; m1v_debug_set_path overrides.
    Same bytes either way."""
    torch = torch_cuda
    for W in (352, 356, 350):
        enc = _enc(W, 288, max_frames=2)
        assert enc.path == "tiles", (W, enc.path)
        enc.close()
    enc4 = _enc(352, 288, channels=4, max_frames=2)
    assert enc4.path == "runs"
    enc4.close()
    W, H, n = 352, 288, 2
    rgb = np.random.default_rng(9).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    want, _ = orc.encode_frames(rgb, n, W, H, 0, 12, orc.MODE_FULL)
    flat = torch.empty(rgb.size + 16, dtype=torch.uint8, device="cuda")
    enc = _enc(W, H, max_frames=n)
    for shift, forced, path_after in ((0, None, "tiles"), (2, None, "tiles"), (0, "runs", "runs"), (2, "runs", "runs"), (0, "auto", "tiles")):
        if forced:
            enc.debug_set_path(forced)
        dev = flat[shift:shift + rgb.size].view(n, H, W, 3)
        dev.copy_(torch.from_numpy(rgb))
        got, _ = enc.encode_to_bytes(dev, 0)
        assert got == want and enc.path == path_after, (shift, forced, enc.path)
    enc.debug_set_input_mode(0)      # a forced input mode is a run-kernel hook
    assert enc.path == "runs"
    got, _ = enc.encode_to_bytes(flat[:rgb.size].view(n, H, W, 3), 0)
    assert got == want
    enc.close()


def test_subsample(torch_cuda, orc):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    W, H = 352, 288
    cb = rng.integers(0, 256, W * H, dtype=np.uint8)
    cr = rng.integers(0, 256, W * H, dtype=np.uint8)
    enc = _enc(W, H)
    a, b = enc.subsample(torch.from_numpy(cb).cuda(), torch.from_numpy(cr).cuda())
    wa, wb = orc.subsample(cb, cr, W, H)
    assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb)
    enc.close()


@pytest.mark.parametrize("W,H,mode", [(1920, 1080, "full"), (1920, 1080, "strict"), (352, 288, "full"),
                                      (360, 250, "full"), (100, 150, "strict"), (3840, 2160, "full")])
def test_config2_coefficients_bit_exact(torch_cuda, orc, W, H, mode):
    """BASELINE config 2: DCT+quant+zigzag only, every block coefficient vs the oracle; through the tile form of the
    kernel (3-channel default: LDS-DMA tiles, whole-line stores) and through the run-shaped one (forced; serves 4 channels),
    also from a buffer that starts at an odd address, and at a quality whose levels need all 16 bits of the output."""
    torch = torch_cuda
    for qf, shift, path in ((12, 0, "auto"), (12, 0, "runs"), (100, 1, "auto")):
        enc = _enc(W, H, qf, mode=mode, max_frames=2)
        if path != "auto":
            enc.debug_set_path(path)
        src = enc.synth(2, seed=2024)
        flat = torch.empty(src.numel() + 16, dtype=torch.uint8, device="cuda")
        rgb = flat[shift:shift + src.numel()].view(src.shape)
        rgb.copy_(src)
        got = enc.coefficients(rgb).cpu().numpy().astype(np.int32)
        host = src.cpu().numpy()
        for f in range(2):
            want = orc.frame_coefficients(host[f], W, H, qf, _omode(orc, mode))
            assert got[f].shape == want.shape and np.array_equal(got[f], want), (qf, shift, path, f)
        enc.close()


@pytest.mark.parametrize("fn", G.E2E_FILES)
def test_golden_files_through_hip(torch_cuda, orc, fn):
    """Committed reference outputs (tests/golden, produced by the real reference): the HIP path must
    reproduce the reference's .mpeg bytes from the stb-decoded pixels."""
    torch = torch_cuda
    z = G.load(fn)
    rgb = z["rgb"]
    n, H, W, C = rgb.shape
    d = torch.from_numpy(rgb).cuda()
    from ec504_imageencoder_amd import file_prolog
    for _, qf, mode, _, want in G.e2e_cases([fn]):
        enc = _enc(W, H, qf, mode, channels=C, max_frames=n)
        got, sizes = enc.encode_to_bytes(d, 0)
        assert file_prolog() + got == want, (fn, qf, mode)
        assert sum(sizes) == len(got)
        # host-buffer entry point gives the same bytes
        hgot, hsizes = enc.encode_host(rgb, 0)
        assert hgot == got and hsizes == sizes
        # .bit side file planes: from the device entry point and from the one-upload host entry point
        # (m1v_encode_planes_host, two half-batch uploads overlapped with the plane downloads)
        planes = enc.convert(d).cpu().numpy()
        pgot, psizes, hplanes = enc.encode_host(rgb, 0, with_planes=True)
        assert pgot == got and psizes == sizes and np.array_equal(hplanes, planes)
        for i in range(n):
            blob = struct.pack("<ii", W, H) + planes[i].tobytes()
            assert hashlib.sha256(blob).hexdigest() == str(z["bit_sha256"][i])
        enc.close()


def test_golden_300_frames_hour_wrap(torch_cuda, orc):
    torch = torch_cuda
    z = G.load("e2e_300_wrap.npz")
    rgb = z["rgb"][z["frame_index"]]
    n, H, W, C = rgb.shape
    from ec504_imageencoder_amd import file_prolog
    enc = _enc(W, H, 12, "strict", channels=C, max_frames=n)
    got, _ = enc.encode_to_bytes(torch.from_numpy(rgb).cuda(), 0)
    assert file_prolog() + got == z["mpeg_strict_q12"].tobytes()
    # two batches with the right global index give the same stream (sharding invariant)
    a, _ = enc.encode_to_bytes(torch.from_numpy(rgb[:130]).cuda(), 0)
    b, _ = enc.encode_to_bytes(torch.from_numpy(rgb[130:]).cuda(), 130)
    assert a + b == got
    enc.close()


@pytest.mark.parametrize("W,H,mode,qf,n", [(352, 288, "full", 12, 4), (352, 288, "strict", 50, 3), (96, 144, "strict", 12, 2),
                                           (1920, 1080, "full", 12, 3), (1920, 1080, "full", 30, 2), (400, 600, "full", 5, 2),
                                           (360, 250, "full", 12, 2), (366, 250, "full", 12, 2), (100, 150, "strict", 12, 2),
                                           (3840, 2160, "full", 12, 1), (32, 3008, "full", 12, 2), (16, 16, "full", 12, 9),
                                           (4128, 32, "full", 12, 2), (7680, 4320, "full", 12, 1),
                                           (105, 49, "full", 12, 5), (1366, 768, "full", 12, 2), (333, 301, "full", 40, 3)])
def test_random_frames_byte_exact(torch_cuda, orc, W, H, mode, qf, n):
    """Seeded synthetic frames: HIP stream == oracle stream, sizes too.  Covers the unaligned-width
    slow load path (366), tall strips that need the chunk loop (3008 rows = 1128 blocks per strip),
    4K (strip byte 0xF0, dimension wrap), the smallest picture, more than 255 strips (the uint8 slice byte wraps; the
    oracle is pinned on this by tests/test_oracle_vs_reference.py), 8K (480 strips, 194,400 blocks per frame) and the
    funnel-shifted 28-byte row loads (odd widths; 105x49x3 bytes per frame is odd, so frames are misaligned against each
    other and the last row of the last frame ends the buffer)."""
    enc = _enc(W, H, qf, mode, max_frames=n)
    rgb = enc.synth(n, seed=1234 + W)
    got, sizes = enc.encode_to_bytes(rgb, first_frame_index=250)  # crosses the hour wrap at 256
    want, wsizes = orc.encode_frames(rgb.cpu().numpy(), n, W, H, 250, qf, _omode(orc, mode), threads=8)
    assert got == want
    assert sizes == [int(s) for s in wsizes]
    enc.close()


def test_rgba_input(torch_cuda, orc):
    W, H, n = 352, 288, 2
    enc = _enc(W, H, 12, "full", channels=4, max_frames=n)
    rgb = enc.synth(n, seed=9)
    got, _ = enc.encode_to_bytes(rgb, 0)
    want, _ = orc.encode_frames(rgb.cpu().numpy(), n, W, H, 0, 12, orc.MODE_FULL, channels=4)
    assert got == want
    enc.close()


@pytest.mark.parametrize("qf,npos,amp,big", [(12, 6, 700, 0.0), (50, 8, 300, 0.0), (90, 16, 120, 0.0), (92, 10, 130, 0.4)])
def test_long_blocks_and_global_fallback(torch_cuda, orc, qf, npos, amp, big):
    """Blocks longer than 64 bits (register accumulator overflows -> second walk), 20- and 28-bit
    escapes, and strips larger than the LDS image (forced with a tiny LDS capacity -> global-memory
    atomics path) must still match the oracle bit for bit."""
    torch = torch_cuda
    rng = np.random.default_rng(qf * 100 + npos)
    W, H = 176, 144
    pics = []
    for _ in range(6):
        p = _heavy_picture(rng, W, H, npos, amp, big)
        try:  # drop pictures the reference itself cannot encode (|level| >= 256 -> segfault)
            orc.encode_frame(p, W, H, 0, qf, orc.MODE_FULL)
            pics.append(p)
        except ValueError:
            pass
    assert len(pics) >= 2
    pics = np.stack(pics)
    co = orc.frame_coefficients(pics[0], W, H, qf, orc.MODE_FULL)
    assert max(len(orc.encode_block_bits(1, z)[1]) for z in co[:240]) > 64
    if big:
        assert any(abs(v) >= 128 for z in co for v in _emitted_levels(z))  # 28-bit escapes are exercised
    if big:
        assert any(40 < abs(v) < 128 for z in co for v in _emitted_levels(z))  # and 20-bit ones
    want, wsizes = orc.encode_frames(pics, len(pics), W, H, 0, qf, orc.MODE_FULL)
    for lds_words in (0, 64, 8):
        enc = _enc(W, H, qf, "full", max_frames=len(pics))
        enc.debug_set_lds_words(lds_words)
        got, sizes = enc.encode_to_bytes(torch.from_numpy(pics).cuda(), 0)
        assert got == want, (qf, lds_words)
        assert sizes == [int(x) for x in wsizes]
        enc.close()


@pytest.mark.parametrize("qf", [76, 77])
def test_extreme_levels_at_the_narrow_staging_boundary(torch_cuda, orc, qf):
    """Quality 76 is the last one staged as one byte per level (smallest AC divisor 8: |level| <= 1022/8 = 127),
    77 the first staged as int16.  Blocks made of the sign patterns of the basis functions with the largest
    coefficients and the smallest divisors exercise the largest levels either side of the switch."""
    torch = torch_cuda
    W, H = 256, 144
    rng = np.random.default_rng(qf)
    pics = []
    for _ in range(3):
        pic = extreme_pattern_picture(rng, W, H)
        try:
            orc.encode_frame(pic, W, H, 0, qf, orc.MODE_FULL)
            pics.append(pic)
        except ValueError:
            pass
    assert pics, "every picture was unencodable"
    pics = np.stack(pics)
    co = orc.frame_coefficients(pics[0], W, H, qf, orc.MODE_FULL)
    # with the default matrix the binding position is (0,1)/(1,0): 924 / 8 = 115 at quality 76, 924 / 7 = 132 at 77
    assert np.abs(co[:, 1:]).max() >= (128 if qf == 77 else 110)
    want, wsizes = orc.encode_frames(pics, len(pics), W, H, 0, qf, orc.MODE_FULL)
    enc = _enc(W, H, qf, "full", max_frames=len(pics))
    got, sizes = enc.encode_to_bytes(torch.from_numpy(pics).cuda(), 0)
    assert got == want and sizes == [int(x) for x in wsizes]
    assert np.array_equal(enc.coefficients(torch.from_numpy(pics).cuda()).cpu().numpy()[0].astype(np.int32), co)
    enc.close()


@pytest.mark.parametrize("W,H,mode,qf,n,shift", [
    (1920, 1080, "full", 12, 2, 0),    # the benchmark geometry: 15 x 17 tiles, last tile row 3 macroblock rows
    (352, 288, "full", 12, 3, 0),      # 22 strips: last tile column 6 strips wide; 18 macroblock rows = 4.5 tile rows
    (352, 288, "strict", 50, 2, 0),    # the reference's 96 x 144 corner: one tile column of 6 strips, 2.25 tile rows
    (101, 49, "full", 12, 2, 0),       # odd width: rows start at every byte phase
    (366, 150, "full", 75, 2, 1),      # odd width AND the buffer itself starts off a 4-byte boundary
    (1366, 768, "full", 90, 1, 3),     # wide staging (int16 levels), unaligned buffer
    (16, 16, "full", 12, 3, 0),        # one macroblock
    (4112, 144, "full", 25, 1, 2),     # 257 strips: strip byte wraps (uint8), 33 tile columns
    (640, 2304, "full", 100, 1, 0),    # 144 macroblock rows = 36 tile rows, divisor 1 everywhere
])
def test_tile_and_run_paths_agree_with_the_oracle(torch_cuda, orc, W, H, mode, qf, n, shift):
    """The two encode kernels (tiles: LDS-DMA of 8-strip x 4-macroblock-row tiles; runs: a lane loads its own block rows)
    give the oracle's bytes on the same buffer, also when the buffer starts at an odd address (`shift` bytes into an
    allocation)."""
    torch = torch_cuda
    rng = np.random.default_rng(W * 31 + H + qf)
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    rgb[:, : H // 2] = (rgb[:, : H // 2] // 32) * 32          # upper half compressible: short and long blocks in one strip
    want, wsizes = orc.encode_frames(rgb, n, W, H, 250, qf, _omode(orc, mode), threads=8)
    flat = torch.empty(rgb.size + 16, dtype=torch.uint8, device="cuda")
    dev = flat[shift:shift + rgb.size].view(n, H, W, 3)
    dev.copy_(torch.from_numpy(rgb))
    for path in ("tiles", "runs"):
        enc = _enc(W, H, qf, mode, max_frames=n)
        enc.debug_set_path(path)
        assert enc.path == path
        got, sizes = enc.encode_to_bytes(dev, first_frame_index=250)
        assert sizes == [int(x) for x in wsizes], (path, sizes[:4], [int(x) for x in wsizes[:4]])
        assert got == want, path
        enc.close()


@pytest.mark.parametrize("threads", [64, 128, 192, 256, 320, 384])
def test_dense_run_lengths(torch_cuda, orc, threads):
    """Every supported run length of the dense kernel gives the same bytes (segment stitching at all phases)."""
    W, H, n = 1920, 1080, 2
    enc = _enc(W, H, 12, "full", max_frames=n)
    rgb = enc.synth(n, seed=99)
    want, wsizes = orc.encode_frames(rgb.cpu().numpy(), n, W, H, 3, 12, orc.MODE_FULL, threads=8)
    enc.debug_set_dense_threads(threads)
    got, sizes = enc.encode_to_bytes(rgb, first_frame_index=3)
    assert got == want and sizes == [int(x) for x in wsizes]
    enc.close()


def test_pipelined_mode_matches(torch_cuda, orc):
    """Pipelined mode: layout + gather of batch k on the internal stream while batch k+1 encodes.  Six batches of
    different frames back to back, outputs double-buffered by the caller, one flush at the end: every batch's
    bytes, sizes, totals and status equal the oracle's."""
    torch = torch_cuda
    W, H, n = 704, 576, 6
    enc = _enc(W, H, 12, "full", max_frames=n)
    enc.set_pipelined(True)
    batches = [enc.synth(n, seed=1000 + k) for k in range(6)]
    outs = [torch.empty(enc.default_out_capacity(n), dtype=torch.uint8, device="cuda") for _ in range(6)]
    res = []
    for k, rgb in enumerate(batches):
        res.append(enc.encode(rgb, first_frame_index=10 * k, out=outs[k]))
    enc.flush()
    torch.cuda.synchronize()
    for k, (out, sizes, meta) in enumerate(res):
        want, wsizes = orc.encode_frames(batches[k].cpu().numpy(), n, W, H, 10 * k, 12, orc.MODE_FULL, threads=8)
        total, status = (int(x) for x in meta.cpu())
        assert status & 0xFFFFFFFF == 0 and total == len(want), k
        assert out[:total].cpu().numpy().tobytes() == want, k
        assert [int(x) for x in sizes[:n].cpu()] == [int(x) for x in wsizes], k
    # switching back restores the plain stream-ordered behaviour
    enc.set_pipelined(False)
    got, _ = enc.encode_to_bytes(batches[0], 0)
    assert got == orc.encode_frames(batches[0].cpu().numpy(), n, W, H, 0, 12, orc.MODE_FULL, threads=8)[0]
    enc.close()


def test_unencodable_level_is_reported(torch_cuda, orc):
    """|level| >= 256 with run >= 1: the reference dereferences NULL (vlc.c:349 -> bit_vector.c:100).
    The HIP path reports M1V_E_UNENCODABLE instead of producing bytes; the oracle flags the same input."""
    torch = torch_cuda
    from ec504_imageencoder_amd import EncoderError, _ffi
    W, H, qf = 96, 144, 92
    yy, xx = np.mgrid[0:H, 0:W]
    a = ((yy % 8) < 4).astype(np.uint8) * 255     # vertical step: zigzag position 2 = 308 after a zero at 1
    pic = np.stack([a, a, a], -1)[None]
    with pytest.raises(ValueError):
        orc.encode_frame(pic[0], W, H, 0, qf, orc.MODE_FULL)
    enc = _enc(W, H, qf, "full", max_frames=1)
    with pytest.raises(EncoderError) as ei:
        enc.encode_to_bytes(torch.from_numpy(pic).cuda(), 0)
    assert ei.value.code == _ffi.E_UNENCODABLE
    with pytest.raises(EncoderError) as ei:
        enc.encode_host(pic, 0)
    assert ei.value.code == _ffi.E_UNENCODABLE
    enc.close()


def _per_frame_oracle(orc, host, W, H, first, qs):
    recs = [orc.encode_frame(host[f], W, H, first + f, q, orc.MODE_FULL) for f, q in enumerate(qs)]
    return b"".join(recs), [len(r) for r in recs]


def test_encode_to_bytes_grows_an_output_buffer_that_is_too_small(torch_cuda, orc):
    """A first output buffer of 100 bytes for two records of a few hundred: STATUS_NOSPACE, and encode_to_bytes encodes again
    into a worst-case buffer.  What it returns is the oracle's stream, at the encoder's quality and at one quality per frame."""
    W, H, n = 96, 48, 2
    enc = _enc(W, H, 12, "full", max_frames=n)
    enc.default_out_capacity = lambda n_frames: 100
    rgb = enc.synth(n, seed=61)
    host = rgb.cpu().numpy()
    want, wsizes = orc.encode_frames(host, n, W, H, 4, 12, orc.MODE_FULL)
    assert len(want) > 100
    assert enc.encode_to_bytes(rgb, 4) == (want, [int(x) for x in wsizes])
    assert enc.encode_to_bytes(rgb, 4, quality=[5, 12]) == _per_frame_oracle(orc, host, W, H, 4, [5, 12])
    enc.close()


def test_encode_to_bytes_recovers_from_scratch_and_output_together(torch_cuda, orc):
    """A forced 8-word LDS image sends all 45 tile units of the batch to an overflow arena of 32 slots (STATUS_SCRATCH) and the
    first output buffer holds 100 bytes (STATUS_NOSPACE): within its three attempts encode_to_bytes reserves the worst-case
    scratch, takes a worst-case output buffer and returns the oracle's stream; the next call on the encoder is exact too."""
    W, H, n = 352, 288, 3
    enc = _enc(W, H, 12, "full", max_frames=n)
    enc.debug_set_lds_words(8)
    enc.default_out_capacity = lambda n_frames: 100
    rgb = enc.synth(n, seed=62)
    want, wsizes = orc.encode_frames(rgb.cpu().numpy(), n, W, H, 9, 12, orc.MODE_FULL)
    before = enc.scratch_bytes()
    assert enc.encode_to_bytes(rgb, 9) == (want, [int(x) for x in wsizes])
    assert enc.scratch_bytes() > before
    assert enc.encode_to_bytes(rgb, 9) == (want, [int(x) for x in wsizes])
    enc.close()


def test_encode_to_bytes_refuses_an_unencodable_frame_and_goes_on(torch_cuda, orc):
    """Bands of four rows of 255 / 0 at quality 92 hold a level the VLC cannot code (the oracle refuses the frame; it codes
    an all-noise frame even at quality 100, so that is no refusal case): encode_to_bytes raises E_UNENCODABLE without a retry,
    and the encoder then encodes a plain frame exactly."""
    torch = torch_cuda
    from ec504_imageencoder_amd import EncoderError, _ffi
    W, H, qf = 96, 48, 92
    bands = np.where((np.arange(H)[:, None] % 8) < 4, 255, 0).astype(np.uint8).repeat(W, axis=1)
    pic = np.stack([bands, bands, bands], -1)[None]
    with pytest.raises(ValueError):
        orc.encode_frame(pic[0], W, H, 0, qf, orc.MODE_FULL)
    enc = _enc(W, H, qf, "full", max_frames=1)
    with pytest.raises(EncoderError) as ei:
        enc.encode_to_bytes(torch.from_numpy(pic).cuda(), 0)
    assert ei.value.code == _ffi.E_UNENCODABLE
    rgb = enc.synth(1, seed=63)
    want, wsizes = orc.encode_frames(rgb.cpu().numpy(), 1, W, H, 2, qf, orc.MODE_FULL)
    assert enc.encode_to_bytes(rgb, 2) == (want, [int(x) for x in wsizes])
    enc.close()


def test_argument_errors(torch_cuda):
    from ec504_imageencoder_amd import EncoderError, Mpeg1Encoder
    with pytest.raises(EncoderError):
        Mpeg1Encoder(64, 64, 12, "strict")      # 96x144 region does not fit (reference reads out of bounds)
    with pytest.raises(EncoderError):
        Mpeg1Encoder(8, 8, 12, "full")          # not even one macroblock
    with pytest.raises(EncoderError):
        Mpeg1Encoder(352, 288, 12, "full", channels=2)
    enc = Mpeg1Encoder(352, 288, 12, "full", max_frames=2)
    rgb = enc.synth(3)
    with pytest.raises(EncoderError):
        enc.encode(rgb)                          # 3 frames > max_frames
    enc.close()


def test_output_capacity_is_checked(torch_cuda, orc):
    torch = torch_cuda
    from ec504_imageencoder_amd import _ffi
    enc = _enc(352, 288, 12, "full", max_frames=2)
    rgb = enc.synth(2)
    small = torch.zeros(6000, dtype=torch.uint8, device="cuda")   # one frame fits, two do not
    out, sizes, meta = enc.encode(rgb, 0, out=small)
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status & _ffi.STATUS_NOSPACE
    want, wsizes = orc.encode_frames(rgb.cpu().numpy(), 2, 352, 288, 0, 12, orc.MODE_FULL)
    assert total == len(want)                                      # sizes are still exact
    assert small[:int(wsizes[0])].cpu().numpy().tobytes() == want[:int(wsizes[0])]
    enc.close()


def test_full_size_batch_properties(torch_cuda, orc):
    """BASELINE config 3 at full size (300 x 1080p): properties that do not need 300 oracle frames —
    (1) determinism, (2) every frame record parses (headers, back-patched length, trailer),
    (3) a frame encoded alone with its global index equals its record inside the batch (sharding
    invariant), (4) six frames spot-checked byte for byte against the oracle, (5) sum of sizes == total."""
    torch = torch_cuda
    W, H, n = 1920, 1080, 300
    enc = _enc(W, H, 12, "full", max_frames=n)
    rgb = enc.synth(n, seed=504)
    out, sizes, meta = enc.encode(rgb, 0)
    out2, sizes2, meta2 = enc.encode(rgb, 0, out=torch.empty_like(out))
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status == 0 and total == int(meta2.cpu()[0])
    assert torch.equal(out[:total], out2[:total]) and torch.equal(sizes, sizes2)
    blob = out[:total].cpu().numpy().tobytes()
    sz = [int(s) for s in sizes.cpu()]
    assert sum(sz) == total
    off = 0
    for f in range(n):
        rec = blob[off:off + sz[f]]
        assert rec[:4] == b"\x00\x00\x01\xe0" and rec[16:20] == b"\x00\x00\x01\xb3"
        assert rec[28:32] == b"\x00\x00\x01\xb8" and rec[36:44] == b"\x00\x00\x01\x00\x00\x0f\xff\xf8"
        assert rec[32] == ((f & 0xFF) & 0x1F) << 2
        assert struct.unpack(">H", rec[4:6])[0] == (sz[f] - 48 + 36) & 0xFFFF
        assert rec[44:49] == b"\x00\x00\x01\x01\x0b" or rec[44:48] == b"\x00\x00\x01\x01"
        assert rec[-4:] == b"\x00\x00\x00\x00"
        off += sz[f]
    offs = np.concatenate([[0], np.cumsum(sz)])
    for f in (0, 1, 149, 255, 256, 299):
        want = orc.encode_frame(rgb[f].cpu().numpy(), W, H, f, 12, orc.MODE_FULL)
        assert blob[offs[f]:offs[f + 1]] == want, f
        alone, _ = enc.encode_to_bytes(rgb[f:f + 1], first_frame_index=f)
        assert alone == want
    enc.close()


def test_profile_events_bracket_only_the_encode_kernel(torch_cuda):
    """m1v_profile_read_times (the source of bench.py's roofline.achieved) must time the dominant kernel alone: exactly
    one duration per launch, each positive, and each BELOW the duration of the whole call it belongs to as seen by events
    around that call on the same stream (the call also launches the layout and gather kernels; a lost closing event once
    made the profile report the whole step).  Structure, not speed: no ratio is asserted."""
    torch = torch_cuda
    n, W, H = 100, 1920, 1080
    enc = _enc(W, H, 12, "full", max_frames=n)
    rgb = enc.synth(n, seed=5)
    for _ in range(5):
        enc.encode(rgb)
    torch.cuda.synchronize()
    enc.profile(True)
    marks = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        enc.encode(rgb)
        b.record()
        marks.append((a, b))
    torch.cuda.synchronize()
    times = enc.profile_read_times()
    enc.profile(False)
    assert len(times) == 20 and all(t > 0 for t in times)
    for t, (a, b) in zip(times, marks):
        assert t < a.elapsed_time(b)
    assert enc.profile_read_times() == []          # reading resets the collection
    enc.close()


def test_full_size_4k_batch_properties(torch_cuda, orc):
    """BASELINE config 4 at full size (300 x 3840x2160, 7.5 GB of input resident in HBM): the properties of
    test_full_size_batch_properties — determinism, every record parses (slice byte up to 240, SEQ carries W & 0xFF = 0,
    H & 0xFF = 112), sum of sizes == total — and frames 0 / 255 / 256 / 299 byte for byte against the oracle, also when
    encoded alone with their global index (sharding invariant across the hour wrap)."""
    torch = torch_cuda
    W, H, n = 3840, 2160, 300
    enc = _enc(W, H, 12, "full", max_frames=n)
    assert enc.strips == 240 and enc.mb_rows == 135
    rgb = enc.synth(n, seed=504)
    out, sizes, meta = enc.encode(rgb, 0)
    out2, sizes2, meta2 = enc.encode(rgb, 0, out=torch.empty_like(out))
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status == 0 and total == int(meta2.cpu()[0])
    assert torch.equal(out[:total], out2[:total]) and torch.equal(sizes, sizes2)
    del out2
    sz = [int(s) for s in sizes.cpu()]
    assert sum(sz) == total
    offs = np.concatenate([[0], np.cumsum(sz)])
    head = torch.stack([out[int(o):int(o) + 48] for o in offs[:-1]]).cpu().numpy()
    tail = torch.stack([out[int(o) - 4:int(o)] for o in offs[1:]]).cpu().numpy()
    for f in range(n):
        rec = head[f].tobytes()
        assert rec[:4] == b"\x00\x00\x01\xe0" and rec[16:20] == b"\x00\x00\x01\xb3"
        assert rec[20:23] == bytes([0, 0, 112])               # (w >> 4), (w & 15) << 4 | (h >> 8), h & 0xFF with uint8 w, h
        assert rec[28:32] == b"\x00\x00\x01\xb8" and rec[36:44] == b"\x00\x00\x01\x00\x00\x0f\xff\xf8"
        assert rec[32] == ((f & 0xFF) & 0x1F) << 2
        assert struct.unpack(">H", rec[4:6])[0] == (sz[f] - 48 + 36) & 0xFFFF
        assert rec[44:48] == b"\x00\x00\x01\x01" and tail[f].tobytes() == b"\x00\x00\x00\x00"
    for f in (0, 255, 256, 299):
        want = orc.encode_frame(rgb[f].cpu().numpy(), W, H, f, 12, orc.MODE_FULL)
        assert out[int(offs[f]):int(offs[f + 1])].cpu().numpy().tobytes() == want, f
        alone, _ = enc.encode_to_bytes(rgb[f:f + 1], first_frame_index=f)
        assert alone == want
        assert want.count(b"\x00\x00\x01\xf0") >= 1             # strip 240's start code (0xF0) is emitted
    enc.close()


def test_input_modes_agree_on_one_buffer(torch_cuda, orc):
    """The dense kernel loads its pixels in one of four ways (aligned 24-byte rows, 28-byte rows + funnel shift, 32-byte
    rows of 4-channel pixels, byte loads), picked from width / channels / alignment.  m1v_debug_set_input_mode forces the
    byte-load and the funnel path onto a buffer that would take the aligned path: same bytes out, and equal to the oracle."""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    for (W, H, C) in ((1920, 288, 3), (360, 304, 3), (352, 288, 4)):
        n = 2
        rgb = rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)
        want, _ = orc.encode_frames(rgb, n, W, H, 3, 12, orc.MODE_FULL, channels=C)
        dev = torch.from_numpy(rgb).cuda()
        for mode in (-1, 0, 2):
            enc = _enc(W, H, 12, "full", channels=C, max_frames=n)
            enc.debug_set_input_mode(mode)
            got, _ = enc.encode_to_bytes(dev, 3)
            assert got == want, (W, H, C, mode)
            enc.close()


def test_fuzz_slice(torch_cuda, orc):
    """A seeded slice of tests/fuzz_parity.py (the hand-run soak) so that every test run carries randomised coverage:
    random width / height (odd ones too) / channels / region / quality factor / frame index / content class / dense run
    length / LDS image size / pipelined mode / forced input mode, HIP stream vs oracle stream byte for byte."""
    import fuzz_parity
    cases, skipped, fails = fuzz_parity.run(budget=60.0, seed=20261004, max_cases=160, max_pixels=1024 * 800, verbose=False)
    assert not fails, fails[:5]
    assert cases >= 40 and skipped < cases // 2


def test_sequence_fuzz_slice(torch_cuda, orc):
    """A seeded slice of the sequence mode of tests/fuzz_parity.py (hand-run soak: fuzz_parity.py SECONDS SEED seq): one
    encoder per case through 4..12 random steps (batch sizes 0..max_frames, pipelined on / off, forced path, LDS image,
    reservation, run length and input mode, injected encode failures), every encode against the oracle."""
    import fuzz_parity
    cases, encodes, skipped, fails = fuzz_parity.run_sequences(budget=60.0, seed=20261016, max_cases=80, verbose=False)
    assert not fails, fails[:5]
    assert cases >= 30 and encodes >= 200 and skipped < encodes // 4, (cases, encodes, skipped)


def test_scratch_is_compact_and_overflow_is_handled(torch_cuda, orc):
    """Round 1 reserved a worst-case slot (28 KiB) per run of 256 blocks: 1.6 GB for 34 MB of payload.  Now a run owns a
    compact slot and only runs that outgrow the LDS image take a worst-case slot from an overflow arena:
    (1) 300 x 1080p at quality 12 holds less than 4x its payload as scratch and the noise benchmark never overflows;
    (2) when every run overflows (forced here with a tiny LDS image; heavy pictures stay below the default compact slot at
        every quality factor tried) the default arena is exhausted -> M1V_STATUS_SCRATCH, and after reserve_scratch() (what
        encode_to_bytes does on its own) the stream equals the oracle's."""
    torch = torch_cuda
    from ec504_imageencoder_amd import _ffi
    W, H, n = 1920, 1080, 300
    enc = _enc(W, H, 12, "full", max_frames=n)
    rgb = enc.synth(n, seed=504)
    out, sizes, meta = enc.encode(rgb, 0)
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status == 0
    assert enc.scratch_bytes() < 4 * total, (enc.scratch_bytes(), total)
    enc.close()

    rng = np.random.default_rng(9)
    W, H, n = 96, 1088, 8           # 6 strips x 68 macroblock rows = 2448 blocks: 10 runs per frame, 80 in the batch
    pic = _heavy_picture(rng, W, H, 6, 700)                    # every block codes six isolated coefficients: > 64 bits
    heavy = np.ascontiguousarray(np.broadcast_to(pic, (n, H, W, 3)))
    want, wsizes = orc.encode_frames(heavy, n, W, H, 0, 12, orc.MODE_FULL)
    enc = _enc(W, H, 12, "full", max_frames=n)
    enc.debug_set_lds_words(64)     # 256-byte LDS image (a realistic picture does not outgrow the default 2 KiB): every run overflows
    dev = torch.from_numpy(heavy).cuda()
    out, sizes, meta = enc.encode(dev, 0)
    torch.cuda.synchronize()
    status = int(meta.cpu()[1]) & 0xFFFFFFFF
    assert status & _ffi.STATUS_SCRATCH, status         # 80 runs overflow, the default arena holds 32
    before = enc.scratch_bytes()
    got, gsizes = enc.encode_to_bytes(dev, 0)           # reserves the worst case and encodes again
    assert got == want and gsizes == [int(x) for x in wsizes]
    assert enc.scratch_bytes() > before
    got2, _ = enc.encode_to_bytes(dev, 0)               # and stays correct on the next batch (counter reset)
    assert got2 == want
    enc.close()


def test_plane_conversion_paths(torch_cuda, orc):
    """m1v_convert_device has two kernels: four pixels per lane with dword loads and packed stores (pixel count a multiple
    of 4, aligned pointers) and the byte-wise one.  Both, for 3 and 4 channels, against the oracle's planes — on noise and
    on a grey picture (r = g = b: every chroma sample is an exact tie that takes the fp64 path)."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    for (W, H, C) in ((64, 48, 3), (64, 48, 4), (37, 23, 3), (37, 23, 4)):
        noise = rng.integers(0, 256, (1, H, W, C), dtype=np.uint8)
        grey = np.repeat(rng.integers(0, 256, (1, H, W, 1), dtype=np.uint8), C, 3)
        for pic in (noise, grey):
            e = Mpeg1Encoder_for_planes(W, H, C)
            got = e.convert(torch.from_numpy(pic).cuda()).cpu().numpy()[0]
            Y, Cb, Cr = orc.convert(pic, channels=C)
            assert np.array_equal(got[0], Y) and np.array_equal(got[1], Cb) and np.array_equal(got[2], Cr), (W, H, C)
            e.close()


def Mpeg1Encoder_for_planes(W, H, C):
    from ec504_imageencoder_amd import Mpeg1Encoder
    return Mpeg1Encoder(W, H, 12, "full", channels=C, max_frames=1)
