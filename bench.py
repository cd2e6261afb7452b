#!/usr/bin/env python3
"""Headline benchmark: 1080p I-frames/s of the MPEG-1 I-frame hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W        (N > 1: starts torch.distributed.run itself, as a child process)
    python bench.py ... --dump-outputs DIR                (also writes the last timed step's output as DIR/<name>.npy)
    python bench.py ... --full                            (also the legs below that take runs of their own)

A step = one pass of the hot path over one batch of synthetic frames that are already resident in
HBM (BASELINE.json configs[2]: 300 x 1920x1080, FULL region, quality factor 12): RGB in, contiguous
frame records out (also in HBM).  For N > 1 every rank encodes its own 300 frames (global frame
indices rank*300 ...); the step loop is ec504_imageencoder_amd.sharding.StepPipeline: the encode of
step k on the main stream, the exchange of step k-1's bitstreams on a side stream (--gather xgmi:
grouped send/recv to rank 0 over RCCL; --gather host: every rank copies its bitstream into its slice
of one pinned host buffer), one host wait per step on eight pinned bytes per rank, nothing allocated
inside the loop.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps, writes the outputs (--dump-outputs) and prints the line; `ms_per_step`
is the wall time of one timed step.  `sustained`, `config4`, `host_delivery` and `cpu_baseline` are measured only with
--full (each can then still be switched off on its own: --sustained-s 0, --no-config4, --deliver none, --no-cpu-baseline).

The line's `roofline` prices the dominant kernel (k_encode_tiles for 3-channel input, k_encode_dense otherwise; --path
forces one) against HBM with its time from HIP events recorded on the launch stream inside the library (per launch:
min / median / max) — `frac` — and the WHOLE step by the same formula — `step_frac` = algorithmic bytes x frames/s / peak
(SURVEY 8d); it carries the HBM bytes of the committed PMC passes (`traffic`, `pmc_fresh`).  `sustained` is a second,
longer leg (about 2.5 s of back-to-back steps) during which a child process samples socket power and shader clock
(rocm-smi): what the chip holds when the run is long enough to sit at its power limit, and the vector-issue share of the
kernel at THAT clock (`valu`).  `config4` = BASELINE config 4 (300 x 3840x2160) measured in the same process.
`host_delivery`: the same steps with every batch's records delivered to pinned host memory under the next encode.
`cpu_baseline` is the oracle timed on this box's host cores (bounded samples).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec
SIMDS = 1024            # 256 CUs x 4 SIMDs; a wave's vector instruction issues over 2 cycles (same guide, "Wave scheduling")
VALU_CYCLES_PER_INST = 2.0


def launch_command(n_gpus, argv, port, script=None):
    """The command `bench.py --gpus N` (N > 1) starts when it was not itself started by torch.distributed.run: one rank per
    GPU of this node, rendezvous on 127.0.0.1 (the container's hostname may not resolve)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), script or os.path.abspath(__file__)] + list(argv)


def self_launch(n_gpus, argv):
    """N > 1 without WORLD_SIZE: run the ranks as a CHILD process group (never exec: the parent has not touched the GPU and does
    not; the child's stdout — rank 0's JSON line — is this process's stdout) and leave with its return code."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.run(launch_command(n_gpus, argv, port), env=env).returncode


class PowerSampler:
    """Socket power and shader clock of one GPU while a leg of the benchmark runs: a child shell polls rocm-smi every ~0.1 s into
    a temporary file (a child process: nothing in this process touches the SMU).  summary() = medians over the samples, or None
    when rocm-smi is absent or prints nothing this parser knows."""

    def __init__(self, device=0, seconds=6.0):
        import shutil
        import subprocess
        import tempfile
        self.proc = self.path = None
        self.device = device
        exe = shutil.which("rocm-smi") or ("/opt/rocm/bin/rocm-smi" if os.path.exists("/opt/rocm/bin/rocm-smi") else None)
        if not exe:
            return
        fd, self.path = tempfile.mkstemp(prefix="ec504_power_")
        os.close(fd)
        loop = (f"{exe} -d {device} --showmaxpower 2>/dev/null; for i in $(seq 1 {int(seconds / 0.1)}); do echo @ $(date +%s.%N); "
                f"{exe} -d {device} --showpower --showclocks 2>/dev/null; sleep 0.05; done")
        self.proc = subprocess.Popen(["bash", "-c", loop], stdout=open(self.path, "w"), stderr=subprocess.DEVNULL)

    def stop(self):
        if self.proc:
            self.proc.terminate()
            try:
                self.proc.wait(timeout=5)
            except Exception:
                self.proc.kill()
            self.proc = None

    def summary(self, t_begin, t_end):
        """Medians over the samples taken in [t_begin, t_end] (time.time())."""
        import re
        import statistics
        self.stop()
        if not self.path:
            return None
        try:
            text = open(self.path).read()
        finally:
            os.unlink(self.path)
            self.path = None
        cap = re.search(r"Max Graphics Package Power \(W\):\s*([0-9.]+)", text)
        watts, mhz = [], []
        for block in text.split("@ ")[1:]:
            head, _, body = block.partition("\n")
            try:
                t = float(head.strip())
            except ValueError:
                continue
            if not (t_begin <= t <= t_end):
                continue
            w = re.search(r"Package Power \(W\):\s*([0-9.]+)", body)
            c = re.search(r"sclk clock level:[^\n]*\((\d+)Mhz\)", body)
            if w:
                watts.append(float(w.group(1)))
            if c:
                mhz.append(float(c.group(1)))
        if not watts and not mhz:
            return None
        return {"power_w": round(statistics.median(watts), 1) if watts else None, "cap_w": float(cap.group(1)) if cap else None,
                "sclk_mhz": round(statistics.median(mhz), 1) if mhz else None, "samples": max(len(watts), len(mhz)),
                "source": "rocm-smi --showpower --showclocks polled by a child process during the leg (medians)"}


def _host_cpu():
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    return model, os.cpu_count() or 1, usable


def cpu_baseline(W, H, qf, seed, gpu_head=None, budget_s=10.0):
    """The oracle (CPU restatement of the reference's path, oracle/mpeg1_oracle.c) timed on bounded samples of the same
    workload, on this box's host cores.  This leg is the only place bench.py touches oracle/: besides the timing it
    checks, outside the timed GPU region, that the GPU's first frame records (gpu_head: bytes) equal the oracle's.
      value / cores = 1   one thread, FULL region: the reference's execution model (it is single-threaded)
      strict              one thread, the 96x144 region the UNMODIFIED reference encodes (colour-converts the whole
                          frame, codes 54 macroblocks)
      threads             frame-parallel oracle on all usable host cores: what the host could do, labelled as such"""
    import oracle_ffi as orc
    model, online, usable = _host_cpu()

    def timed(mode, threads, budget, chunk):
        n, dt, verified = 0, 0.0, None
        while dt < budget and n < 8192:     # bounded sample, generated chunk-wise to bound host memory
            frames = orc.synth_frames(chunk, W, H, seed=seed, first_index=n)
            t0 = time.perf_counter()
            body, sizes = orc.encode_frames(frames, chunk, W, H, n, qf, mode, threads=threads)
            dt += time.perf_counter() - t0
            if n == 0 and gpu_head is not None and mode == orc.MODE_FULL:
                k = int(sizes[0] + sizes[1])
                verified = bool(gpu_head[:k] == body[:k])
            n += chunk
        return n, dt, verified

    n1, t1, verified = timed(orc.MODE_FULL, 1, budget_s, 16)
    ns, ts, _ = timed(orc.MODE_STRICT, 1, budget_s / 4, 16)
    nt_threads = max(1, min(usable, 64))
    nt, tt, _ = timed(orc.MODE_FULL, nt_threads, budget_s / 2, 4 * nt_threads)
    out = {"value": round(n1 / t1, 3), "unit": "frames/s", "cores": 1, "kind": "port",
           "sample": f"{n1} x {W}x{H} synthetic frames, FULL region, qf {qf}, oracle/mpeg1_oracle.c single thread, {t1:.1f} s",
           "host": {"cpu": model, "cores_online": online, "cores_usable": usable},
           "build": "gcc -O2 -ffp-contract=off -fno-fast-math (oracle/Makefile); the reference's own Makefile uses -g without -O",
           "strict": {"value": round(ns / ts, 3), "unit": "frames/s", "cores": 1,
                      "sample": f"{ns} frames, the 96x144 region of the unmodified reference, {ts:.1f} s"},
           "threads": {"value": round(nt / tt, 3), "unit": "frames/s", "cores": nt_threads,
                       "sample": f"{nt} frames, FULL region, frame-parallel on {nt_threads} threads, {tt:.1f} s"}}
    if verified is not None:
        out["gpu_output_matches_oracle"] = verified
    return out


def _code_only(text):
    """The source text without comments and without whitespace differences: what the compiler sees.  The PMC record's hash is
    taken over this, so that a comment edit does not make the committed counters look stale."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == '"' or c == "'":                      # string / character literal: copied verbatim
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
        else:
            out.append(c)
            i += 1
    return "\n".join(" ".join(line.split()) for line in "".join(out).splitlines() if line.strip())


def _pmc_sources_sha256(sources):
    import hashlib
    h = hashlib.sha256()
    for f in sources:
        h.update(_code_only(open(os.path.join(ROOT, f), encoding="utf-8").read()).encode("utf-8"))
    return h.hexdigest()


def _committed_pmc(W, H, n, kernel="k_encode_dense"):
    """The committed rocprofv3 PMC record of this workload and kernel (profiles/r04_pmc.json, written by
    tools/pmc_record_r04.py from the summaries of tools/pmc_r04.sh), or None.  PMC cannot be collected from inside this
    process; the record names the kernel sources it was measured on, and `fresh` says whether they are still the tree's."""
    try:
        with open(os.path.join(ROOT, "profiles", "r04_pmc.json")) as f:
            doc = json.load(f)
        fresh = _pmc_sources_sha256(doc["sources"]) == doc["source_sha256"]
        for rec in doc["workloads"]:
            if [rec["width"], rec["height"], rec["frames"], rec["kernel"]] == [W, H, n, kernel]:
                return dict(rec, fresh=fresh)
    except (OSError, KeyError, ValueError):
        pass
    return None


def pmc_traffic(rec):
    """HBM bytes per launch of the dominant kernel: (2 x FETCH_SIZE + WRITE_SIZE) KiB — on gfx950 FETCH_SIZE counts half
    of the bytes of wide reads (MI355X_MICROARCH.md, HBM section)."""
    return int((2 * rec["fetch_size_kib"] + rec["write_size_kib"]) * 1024) if rec else None


def valu_roofline(rec, kernel_ms, sclk_mhz=None):
    """How much of the kernel's time vector-ALU issue alone accounts for: (vector instructions per launch, PMC) x 2 cycles (a
    wave's vector instruction occupies its SIMD's issue port for two cycles, MI355X_MICROARCH.md) / 1024 SIMDs / the shader
    clock — the clock rocm-smi showed during the sustained leg of this run, or, without one, the clock of the PMC pass — against
    the kernel time.  The rest of the time is memory latency the waves in flight do not hide, and workgroup turnover."""
    if not rec or "valu" not in rec or kernel_ms <= 0:
        return None
    v = rec["valu"]
    ghz = sclk_mhz / 1e3 if sclk_mhz else v.get("clock_ghz")
    if not ghz:
        return None
    issue_ms = v["insts_per_launch"] * VALU_CYCLES_PER_INST / SIMDS / (ghz * 1e9) * 1e3
    return {"bound": "valu-issue", "achieved": round(issue_ms, 4), "peak": round(kernel_ms, 4), "unit": "ms of issue per ms of kernel",
            "frac": round(issue_ms / kernel_ms, 4), "insts_per_launch": v["insts_per_launch"], "cycles_per_inst": VALU_CYCLES_PER_INST,
            "simds": SIMDS, "sclk_ghz": round(ghz, 3), "sclk_source": "rocm-smi during the sustained leg" if sclk_mhz else "GRBM_GUI_ACTIVE of the PMC pass",
            "source": "rocprofv3 --pmc SQ_INSTS_VALU (tools/pmc_r04.sh)"}


def cli_bench(args):
    """the folder-level entry point end to end — a folder of JPEG files through ./encoder
    (tools/encoder_cli.c -> mpeg_encode_procedure in libencoder.so: stb decode on the host pool, pinned staging,
    HIP encode, .mpeg + image_<k>.bit written) timed as a whole process, beside the REAL reference binary
    (oracle/_ref/ref_encoder_full, built from the reference's sources in the build container) on a bounded subset of
    the same folder, whose files must be byte-identical to ours.  Not the headline metric: one JSON line of its own."""
    import shutil
    import subprocess
    import tempfile
    import numpy as np
    from PIL import Image
    W, H, n, qf = args.width, args.height, args.frames, args.quality
    exe, ref = os.path.join(ROOT, "encoder"), os.path.join(ROOT, "oracle", "_ref", "ref_encoder_full")
    if not os.path.exists(exe):
        raise SystemExit("./encoder is not built (make encoder needs the reference's stb_image.h)")
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tempfile.mkdtemp(prefix="ec504_cli_", dir=base)
    try:
        rng = np.random.default_rng(504)
        os.makedirs(os.path.join(d, "images"))
        n_ref = min(n, args.cli_reference_frames)
        os.makedirs(os.path.join(d, "subset"))
        for i in range(n):          # smooth picture + noise: compressible like camera frames, every frame different
            coarse = rng.integers(0, 256, (H // 40 + 1, W // 40 + 1, 3), dtype=np.uint8).repeat(40, 0).repeat(40, 1)[:H, :W]
            img = np.clip(coarse.astype(np.int16) + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
            path = os.path.join(d, "images", f"frame_{i:04d}.jpg")
            Image.fromarray(img).save(path, quality=90)
            if i < n_ref:
                shutil.copy(path, os.path.join(d, "subset", f"frame_{i:04d}.jpg"))
        jpeg_bytes = sum(e.stat().st_size for e in os.scandir(os.path.join(d, "images")))

        def run(binary, images, tag, env=None, extra=()):
            out = os.path.join(d, tag)
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            e = dict(os.environ, EC504_ENCODE_REGION="full")
            e.update(env or {})
            t0 = time.perf_counter()
            rc = subprocess.run([binary, images + "/", out, os.path.join(out, "v.mpeg"), str(qf), *extra], cwd=d, env=e,
                                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
            dt = time.perf_counter() - t0
            assert rc == 0, (binary, rc)
            return dt, out

        run(exe, "subset", "warm", extra=("full",))                 # page in the library and the GPU runtime once
        res = {}
        for tag, env in (("default", {}), ("no_bit_files", {"EC504_WRITE_BIT": "0"}),
                         ("one_host_thread", {"EC504_HOST_THREADS": "1"})):
            best = min(run(exe, "images", "ours_" + tag, env, ("full",))[0] for _ in range(args.cli_repeats))
            res[tag] = {"seconds": round(best, 3), "frames_per_s": round(n / best, 1)}
        line = {"metric": f"{W}x{H} JPEG folder -> .mpeg + .bit, frames/s (whole CLI process, end to end)",
                "value": res["default"]["frames_per_s"], "unit": "frames/s", "n_gpus": 1, "higher_is_better": True,
                "data": "synthetic", "dtype": "f32 (colour fast path, FDCT) + f64 (colour ties) + int32 (VLC, packing)", "vs_baseline": None,
                "config": {"workload": f"{n} JPEG files {W}x{H} (quality 90, {jpeg_bytes / n / 1e3:.0f} KB each) in {os.path.dirname(d)}, "
                                       f"FULL region, quality_factor {qf}, ./encoder = tools/encoder_cli.c + libencoder.so",
                           "host_threads": os.cpu_count(), "runs": res}}
        if os.path.exists(ref) and not args.no_cpu_baseline:
            t_ref, ref_out = run(ref, "subset", "ref")
            _, our_out = run(exe, "subset", "ours_subset", extra=("full",))
            same = all(open(os.path.join(ref_out, f), "rb").read() == open(os.path.join(our_out, f), "rb").read()
                       for f in ["v.mpeg"] + [f"image_{k}.bit" for k in range(1, n_ref + 1)])
            line["cpu_baseline"] = {"value": round(n_ref / t_ref, 3), "unit": "frames/s", "cores": 1, "kind": "reference",
                                    "sample": f"the reference's own ./encoder (FULL bounds) on the first {n_ref} files of the same folder, {t_ref:.1f} s",
                                    "output_matches_reference": same}
            assert same, "CLI output differs from the reference binary's"
        print(json.dumps(line), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def config4_leg(torch, Mpeg1Encoder, gpu_index, qf, seed, frames=300, warm=12, steps=30):
    """BASELINE config 4 in the same process: 300 x 3840x2160 synthetic frames resident in HBM (7.5 GB), the same step loop, the
    encode kernel's time from the library's events; `traffic` from the committed PMC record of this workload."""
    W, H = 3840, 2160
    dev = torch.device("cuda", gpu_index)
    enc = Mpeg1Encoder(W, H, qf, "full", max_frames=frames, device=gpu_index)
    try:
        rgb = enc.synth(frames, seed=seed, first_frame_index=0, device=dev)
        outs = [torch.empty(enc.default_out_capacity(frames), dtype=torch.uint8, device=dev) for _ in range(2)]
        metas = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in outs]
        sizes = torch.empty(frames, dtype=torch.int64, device=dev)
        for k in range(warm):
            enc.encode(rgb, 0, out=outs[k % 2], sizes=sizes, meta=metas[k % 2])
        torch.cuda.synchronize(dev)
        enc.profile(True)
        t0 = time.perf_counter()
        for k in range(steps):
            enc.encode(rgb, 0, out=outs[k % 2], sizes=sizes, meta=metas[k % 2])
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        times = enc.profile_read_times(cap=steps + 8)
        enc.profile(False)
        total, status = (int(x) for x in metas[(steps - 1) % 2].cpu())
        assert (status & 0xFFFFFFFF) == 0, f"device status {status:#x}"
        alg = 3 * W * H * frames + total
        k_ms = sum(times) / max(len(times), 1)
        fps = frames * steps / dt
        pmc = _committed_pmc(W, H, frames, "k_encode_tiles" if enc.path == "tiles" else "k_encode_dense")
        traffic = pmc_traffic(pmc)
        return {"workload": f"{frames} x {W}x{H} synthetic RGB frames, FULL region, quality_factor {qf}, input and output resident in HBM",
                "value": round(fps, 1), "unit": "frames/s", "mpixels_per_s": round(fps * W * H / 1e6, 1), "steps": steps, "warmup": warm,
                "ms_per_step": round(dt / steps * 1e3, 4), "bytes_out_per_frame": round(total / frames, 1),
                "kernel": "k_encode_tiles" if enc.path == "tiles" else "k_encode_dense", "kernel_ms": round(k_ms, 4),
                "achieved": round(alg / (k_ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS, "unit_roofline": "GB/s",
                "frac": round(alg / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                "step_frac": round(alg / frames * fps / 1e9 / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_launch": int(alg),
                "traffic": traffic, "traffic_over_algorithmic": round(traffic / alg, 4) if traffic else None,
                "pmc_fresh": bool(pmc and pmc.get("fresh"))}
    finally:
        enc.close()


DUMP_HEAD_BYTES = 4 << 20      # the first 4 MiB of the stream, byte for byte
DUMP_SAMPLE_BYTES = 1 << 21    # plus 2 Mi bytes at fixed, seeded positions over the whole stream


def dump_outputs(dirname, stream, sizes, meta):
    """What the caller of the timed path receives from its last step, as float64 / float32 .npy files (about 40 MB at most):
      meta            [total bytes, status bits]
      frame_sizes     bytes of every frame record (this rank's frames)
      frame_sums      per frame record: sum of its bytes, and sum of byte x (1 + position in the record): every byte counts
      stream_head     the first DUMP_HEAD_BYTES bytes of the stream (values 0..255)
      stream_sample   the stream at DUMP_SAMPLE_BYTES positions drawn from [0, total) by a fixed seed, and those positions
    stream = the uint8 stream (frame records back to back), sizes = int64 record sizes, meta = (total, status)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    data = stream.cpu().numpy() if hasattr(stream, "cpu") else np.asarray(stream)
    data = np.ascontiguousarray(data, np.uint8)
    sizes = np.asarray(sizes.cpu().numpy() if hasattr(sizes, "cpu") else sizes, np.int64)
    total = int(data.size)
    np.save(os.path.join(dirname, "meta.npy"), np.asarray(meta, np.float64))
    np.save(os.path.join(dirname, "frame_sizes.npy"), sizes.astype(np.float64))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if sizes.size else np.zeros(0, np.int64)
    sums = np.zeros((sizes.size, 2), np.float64)
    for i, (s, k) in enumerate(zip(starts, sizes)):
        rec = data[s:s + k].astype(np.int64)
        sums[i] = (rec.sum(), (rec * np.arange(1, rec.size + 1, dtype=np.int64)).sum())
    np.save(os.path.join(dirname, "frame_sums.npy"), sums)
    np.save(os.path.join(dirname, "stream_head.npy"), data[:DUMP_HEAD_BYTES].astype(np.float32))
    pos = np.sort(np.random.default_rng(504).integers(0, max(total, 1), DUMP_SAMPLE_BYTES)) if total else np.zeros(0, np.int64)
    np.save(os.path.join(dirname, "stream_sample.npy"), data[pos].astype(np.float32))
    np.save(os.path.join(dirname, "stream_sample_positions.npy"), pos.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults long enough to sit past the GPU's clock ramp: after an idle start the first ~35 steps (35 ms) run up to
    # 30 % slower (tools/step_ramp.py: 1.11 ms -> 0.86 ms per step), so short runs under-report the steady state
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames", type=int, default=300, help="frames per GPU per step")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--quality", type=int, default=12)
    ap.add_argument("--settle-ms", type=float, default=80.0,
                    help="keep the GPU busy re-generating the synthetic input for this long before the warm-up steps, so "
                         "that short runs are not timed inside the clock ramp (0 = off); reported as clock_settle_ms")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the `cpu_baseline` leg")
    ap.add_argument("--host-path", action="store_true", help="also time the host-buffer (PCIe inclusive) entry point")
    ap.add_argument("--pipeline", action="store_true",
                    help="N=1: overlap each batch's layout + gather with the next batch's encode (m1v_set_pipelined); "
                         "measured equal to the stream-ordered default once the gather became cheap")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo = rehearsal of the N>1 code path on a box with ONE GPU: every rank encodes on cuda:0, "
                         "the bitstream gather goes through host memory (numbers are not meaningful)")
    ap.add_argument("--gather", default="xgmi", choices=["xgmi", "host"],
                    help="N>1: how the per-rank bitstreams reach one place.  xgmi = grouped send/recv to rank 0 (RCCL); "
                         "host = every rank copies its blob into its slice of one pinned host buffer shared by the ranks")
    ap.add_argument("--deliver", default="host", choices=["none", "host"],
                    help="N=1, --full: after the headline run, time the same steps with every batch's frame records delivered to pinned host "
                         "memory (device-to-host copy of batch k on a side stream under the encode of batch k+1); reported as the "
                         "`host_delivery` sub-record, never as `value`")
    ap.add_argument("--path", default="auto", choices=["auto", "tiles", "runs"],
                    help="which encode kernel serves the batches (include/mpeg1_hip.h, m1v_debug_set_path); auto = the library's choice")
    ap.add_argument("--cli", action="store_true",
                    help="instead of the headline run: time the folder-of-JPEGs CLI path end to end (SURVEY 8f.1/8f.2)")
    ap.add_argument("--sustained-s", type=float, default=2.5,
                    help="N=1, --full: length of the second, sustained leg (back-to-back steps with socket power and shader clock sampled by a "
                         "child rocm-smi poller); 0 = off.  Reported as `sustained`, never as `value`")
    ap.add_argument("--no-config4", action="store_true", help="N=1, --full: skip the 300 x 3840x2160 leg (BASELINE config 4, `config4`)")
    ap.add_argument("--cli-reference-frames", type=int, default=6)
    ap.add_argument("--cli-repeats", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="N=1: after the headline run, also the legs that take runs of their own: `sustained`, `config4`, "
                         "`host_delivery`, `cpu_baseline` (off in a plain run)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0) as DIR/<name>.npy (float32/float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cli:
        if args.frames == 300:
            args.frames = 128
        return cli_bench(args)
    if not args.full:      # a plain run: the headline steps and nothing else
        args.sustained_s, args.no_config4, args.no_cpu_baseline, args.deliver = 0.0, True, True, "none"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started the way the driver starts it (python bench.py --gpus N ...): the ranks run as a child process group, this
        # process never initialises the GPU
        sys.exit(self_launch(args.gpus, sys.argv[1:]))

    import numpy as np
    import torch
    import torch.distributed as dist
    from ec504_imageencoder_amd import Mpeg1Encoder
    from ec504_imageencoder_amd.sharding import StepPipeline, shared_host_buffer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start with python bench.py --gpus N (it launches its ranks itself)")
    if args.backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit(f"{world} ranks over RCCL need {world} GPUs, this node shows {torch.cuda.device_count()} "
                         "(--backend gloo rehearses the N > 1 code path on one GPU)")
    distributed = world > 1
    rehearsal = args.backend == "gloo"
    gpu_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(gpu_index)
    dev = torch.device("cuda", gpu_index)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    W, H, n, qf, seed = args.width, args.height, args.frames, args.quality, 504
    enc = Mpeg1Encoder(W, H, qf, "full", max_frames=n, device=gpu_index)
    if args.path != "auto":
        enc.debug_set_path(args.path)
    first = rank * n  # global frame index of this rank's first frame
    rgb = enc.synth(n, seed=seed, first_frame_index=first, device=dev)
    # two output buffers: for N > 1 the exchange of step k overlaps the encode of step k+1
    outs = [torch.empty(enc.default_out_capacity(n), dtype=torch.uint8, device=dev) for _ in range(2)]
    if not distributed and args.pipeline:
        # one GPU: the library overlaps each batch's layout + gather (internal stream) with the next batch's
        # encode kernel; outputs are double-buffered here and joined by enc.flush() inside the timed region
        enc.set_pipelined(True)
    metas = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in outs]
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    out, meta = outs[0], metas[0]
    step_no = 0

    pipe = None
    if distributed:
        # One encode to learn the size of a step's output, so that the gather buffers need not be worst-case sized
        # (every step of the benchmark encodes the same frames; a real caller sizes them from frame_bound).
        enc.encode(rgb, first, out=outs[0], sizes=sizes, meta=metas[0])
        torch.cuda.synchronize(dev)
        mine = torch.tensor([int(metas[0][0].item())], dtype=torch.int64, device="cpu" if rehearsal else dev)
        dist.all_reduce(mine, op=dist.ReduceOp.MAX)
        per_rank = (int(mine.item()) * 5 // 4 + 4095) & ~4095
        host_buf = shm_path = None
        if args.gather == "host":
            name = f"ec504_bench_{os.environ.get('MASTER_PORT', '0')}"
            if rank == 0:
                host_buf, shm_path = shared_host_buffer(world * per_rank, 0, name)
            dist.barrier()
            if rank != 0:
                host_buf, shm_path = shared_host_buffer(world * per_rank, rank, name)

        if rehearsal:   # gloo moves host tensors: the blobs are staged through pinned host memory on the side stream
            h_outs = [torch.empty(per_rank, dtype=torch.uint8, pin_memory=True) for _ in outs]
            h_metas = [torch.zeros(2, dtype=torch.int64, pin_memory=True) for _ in outs]

            def encode(b):
                enc.encode(rgb, first, out=outs[b], sizes=sizes, meta=metas[b])
                h_metas[b].copy_(metas[b], non_blocking=True)
                h_outs[b].copy_(outs[b][:per_rank], non_blocking=True)
                torch.cuda.current_stream().synchronize()
            pipe = StepPipeline(encode, h_outs, h_metas, world, rank, transport=args.gather, host_buffer=host_buf,
                                gather_capacity=world * per_rank, retry=lambda b: (enc.reserve_scratch(True), encode(b)))
        else:
            def encode(b):
                enc.encode(rgb, first, out=outs[b], sizes=sizes, meta=metas[b])
            def retry(b):      # a batch ran out of overflow scratch: reserve the worst case, encode the same frames again
                enc.reserve_scratch(True)
                encode(b)
                torch.cuda.current_stream().synchronize()
            pipe = StepPipeline(encode, outs, metas, world, rank, transport=args.gather, host_buffer=host_buf,
                                gather_capacity=world * per_rank, retry=retry)

    def step():
        nonlocal step_no
        if distributed:
            pipe.step()
            return
        b = step_no % len(outs)
        step_no += 1
        enc.encode(rgb, first, out=outs[b], sizes=sizes, meta=metas[b])

    def fence():
        if distributed:
            pipe.fence()
        else:
            enc.flush()
        torch.cuda.synchronize(dev)

    # not a step: the input is regenerated in place (identical bytes) until the clocks have ramped up
    t_settle = time.perf_counter()
    while (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
        enc.synth(n, seed=seed, first_frame_index=first, device=dev, out=rgb)
        torch.cuda.synchronize(dev)
    for _ in range(args.warmup):
        step()
    fence()
    if distributed:
        dist.barrier()
    enc.profile(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    kernel_times = enc.profile_read_times(cap=max(args.steps, 1) + 8)
    launches, kernel_ms = len(kernel_times), float(sum(kernel_times))
    enc.profile(False)
    if distributed:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearsal else dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        if rank == 0 and pipe.result() is not None:
            # the gathered stream of the last step begins with rank 0's own records (checked outside the timed region)
            own = int(pipe.last_counts[0])
            assert bytes(pipe.result()[:64].cpu().numpy()) == bytes(outs[(pipe.step_no - 1) % 2][:64].cpu().numpy()) and own > 0

    total_bytes, status = (int(x) for x in meta.cpu())
    assert (status & 0xFFFFFFFF) == 0, f"device status {status:#x}"

    if args.dump_outputs and rank == 0:
        # the last timed step's product: one GPU = its output buffer; N > 1 = the stream gathered on rank 0
        if distributed:
            last_total, last_status = sum(int(c) for c in pipe.last_counts), status
            stream = pipe.result()
        else:
            b_last = (step_no - 1) % len(outs)
            last_total, last_status = (int(x) for x in metas[b_last].cpu())
            stream = outs[b_last][:last_total]
        dump_outputs(args.dump_outputs, stream, sizes[:n], (last_total, last_status))

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        fps = world * n * args.steps / elapsed
        out_per_frame = total_bytes / n
        alg_bytes_frame = 3 * W * H + out_per_frame            # RGB read once + emitted bytes
        k_ms = kernel_ms / max(launches, 1)
        kernel_name = "k_encode_tiles" if enc.path == "tiles" else "k_encode_dense"
        pmc = _committed_pmc(W, H, n, kernel_name)
        alg_bytes = alg_bytes_frame * n
        achieved = alg_bytes / (k_ms * 1e-3) / 1e9 if launches else 0.0
        step_achieved = alg_bytes_frame * fps / world / 1e9       # per GPU: SURVEY 8(d), algorithmic bytes x frames/s
        line = {
            "metric": "1080p I-frames/s" if (W, H) == (1920, 1080) else f"{W}x{H} I-frames/s",
            "mpixels_per_s_definition": "frames/s x W x H / 1e6",
            "value": round(fps, 1), "unit": "frames/s", "mpixels_per_s": round(fps * W * H / 1e6, 1),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "clock_settle_ms": args.settle_ms,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (colour fast path, FDCT: exact integers in floats) + f64 (colour ties) + int32 (VLC, packing)",
            "data": "synthetic",
            "config": {"workload": f"{n} x {W}x{H} synthetic RGB frames per GPU, FULL region (all macroblocks), quality_factor {qf}, "
                                   "input and output resident in HBM" + ("" if distributed or not args.pipeline else "; batch k's assembly overlaps batch k+1's encode (two output buffers)"), "frames_per_gpu": n,
                       "global_frames": n * world, "bytes_out_per_frame": round(out_per_frame, 1),
                       "parallelism": f"frames sharded {n}/GPU" + (
                           (", grouped send/recv of the bitstreams to rank 0 (RCCL)" if args.gather == "xgmi" else
                            ", every rank copies its bitstream into its slice of one pinned host buffer") if distributed else "")},
            # "hbm" is the roofline BASELINE.json prices the path against: `frac` = the dominant kernel alone, `step_frac` = the whole
            # step (encode + assembly; per GPU).  What the kernel's time is made of is measured in the `sustained` leg below.
            "roofline": {"bound": "hbm", "kernel": kernel_name, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                         "step_achieved": round(step_achieved, 2), "step_frac": round(step_achieved / HBM_PEAK_GBS, 5),
                         "traffic": pmc_traffic(pmc), "pmc_fresh": bool(pmc and pmc.get("fresh")),
                         "l1_to_l2_read_requests_per_pixel_line": round(pmc["l1_to_l2_read_requests"] / pmc["pixel_lines_128B"], 3)
                         if pmc and pmc.get("l1_to_l2_read_requests") and pmc.get("pixel_lines_128B") else None,
                         "kernel_ms": round(k_ms, 4), "kernel_ms_min": round(min(kernel_times), 4) if kernel_times else None,
                         "kernel_ms_median": round(float(np.median(kernel_times)), 4) if kernel_times else None,
                         "kernel_ms_max": round(max(kernel_times), 4) if kernel_times else None, "launches_timed": launches,
                         "algorithmic_bytes_per_launch": int(alg_bytes)},
        }
        if world == 1 and args.sustained_s > 0:
            # A run long enough to sit at the package power limit: the same steps for ~args.sustained_s seconds, wall clock only
            # (no event records: two per launch would leave gaps in which the chip boosts), power and clock sampled by a child.
            k_sus = max(args.steps, int(args.sustained_s / (ms_per_step * 1e-3)))
            sampler = PowerSampler(gpu_index, seconds=args.sustained_s + 4.0)
            time.sleep(0.4)                              # (the poller's first rocm-smi call)
            w_b = time.time()
            t0 = time.perf_counter()
            for _ in range(k_sus):
                step()
            fence()
            dt = time.perf_counter() - t0
            w_e = time.time()
            power = sampler.summary(w_b + min(0.5, 0.25 * dt), w_e)
            sus_fps = n * k_sus / dt
            line["sustained"] = {"value": round(sus_fps, 1), "unit": "frames/s", "steps": k_sus, "ms_per_step": round(dt / k_sus * 1e3, 4),
                                 "step_frac": round(alg_bytes_frame * sus_fps / 1e9 / HBM_PEAK_GBS, 5), "power": power,
                                 "note": "the headline steps repeated back to back for this long; `value` above is the run the driver asked for"}
            line["roofline"]["valu"] = valu_roofline(pmc, k_ms, power["sclk_mhz"] if power and power.get("sclk_mhz") else None)
        else:
            line["roofline"]["valu"] = valu_roofline(pmc, k_ms)
        if world == 1 and not args.no_config4 and (W, H) == (1920, 1080) and args.path == "auto":
            line["config4"] = config4_leg(torch, Mpeg1Encoder, gpu_index, qf, seed)
        if world == 1 and not args.no_cpu_baseline:
            head = out[:min(out.numel(), 4 * (W * H // 2))].cpu().numpy().tobytes()   # first frame records of rank 0
            line["cpu_baseline"] = cpu_baseline(W, H, qf, seed, gpu_head=head)
            assert line["cpu_baseline"].get("gpu_output_matches_oracle", True), "GPU output differs from the oracle"
        if world == 1 and args.deliver == "host":
            # the path's product is a host bitstream (north_star; the reference fwrites it, encoder.h:445): input resident,
            # records of batch k copied to one of two pinned buffers while batch k+1 encodes
            from ec504_imageencoder_amd.delivery import HostDelivery
            hd = HostDelivery(enc, n, capacity=outs[0].numel())
            # its own step counts, whatever the headline's were: pinned buffers are first touched, and the copy engine's
            # queue fills, over the first ~16 steps (a 20-step run behind 4 warm-up steps measured 0.84 of the resident rate,
            # the same loop behind 50 steps 0.96)
            hd_warm, hd_steps, chunk = max(16, args.warmup), max(100, args.steps), 20
            for _ in range(hd_warm):
                hd.step(rgb, first)
            hd.fence()
            hd.bytes_delivered = 0
            chunk_ms = []
            t0 = time.perf_counter()
            for k in range(hd_steps):
                if k % chunk == 0:
                    tc = time.perf_counter()
                hd.step(rgb, first)
                if k % chunk == chunk - 1:
                    chunk_ms.append((time.perf_counter() - tc) / chunk * 1e3)
            hd.fence()
            dt = time.perf_counter() - t0
            same = bool(torch.equal(hd.result(), outs[(step_no - 1) % len(outs)][:total_bytes].cpu()))
            line["host_delivery"] = {"value": round(n * hd_steps / dt, 1), "unit": "frames/s", "ms_per_step": round(dt / hd_steps * 1e3, 4),
                                     "steps": hd_steps, "warmup": hd_warm,
                                     "ms_per_step_min_of_20": round(min(chunk_ms), 4) if chunk_ms else None,
                                     "ms_per_step_median_of_20": round(float(np.median(chunk_ms)), 4) if chunk_ms else None,
                                     "pcie_gb_per_s": round(hd.bytes_delivered / dt / 1e9, 2), "bytes_per_step": hd.bytes_delivered // hd_steps,
                                     "holds_device_resident_rate": round(n * hd_steps / dt / fps, 4),
                                     "holds_sustained_rate": round(n * hd_steps / dt / line["sustained"]["value"], 4) if "sustained" in line else None,
                                     "delivered_equals_device_output": same,
                                     "note": "input resident in HBM; frame records of batch k -> pinned host memory on a side stream while batch "
                                             "k+1 encodes (ec504_imageencoder_amd/delivery.py); one host wait per step on 16 pinned bytes"}
            assert same, "delivered bytes differ from the device-resident output"
            hd.close()
        if world == 1 and args.host_path:
            # PCIe-inclusive rate of the host-buffer entry point (never the headline value)
            m = min(n, 64)
            res = {}
            for kind, pin in (("pageable", False), ("pinned", True)):
                host_rgb = rgb[:m].cpu()
                if pin:
                    host_rgb = host_rgb.pin_memory()
                arr = host_rgb.numpy()
                enc.encode_host(arr, first)
                t0 = time.perf_counter()
                for _ in range(3):
                    enc.encode_host(arr, first)
                res[kind] = round(3 * m / (time.perf_counter() - t0), 1)
            line["host_buffer_path"] = {"value": res["pinned"], "pageable": res["pageable"], "unit": "frames/s", "frames": m,
                                        "note": "m1v_encode_host: synchronous H2D + encode + D2H; pinned vs pageable input"}
            # the side kernels of the path, device resident: the Y/Cb/Cr planes of the image_<k>.bit files (k_convert4:
            # 3 B in + 3 B out per pixel) and the coefficient-only kernel of BASELINE config 2 (3 B in, 128 B out per block)
            side = {}
            for name, fn, bytes_per_frame in (("planes", lambda: enc.convert(rgb[:m]), 6 * W * H),
                                              ("coefficients", lambda: enc.coefficients(rgb[:m]), 3 * W * H + enc.blocks_per_frame * 128)):
                for _ in range(3):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(5):
                    fn()
                b.record()
                torch.cuda.synchronize(dev)
                ms = a.elapsed_time(b) / 5
                side[name] = {"ms": round(ms, 4), "frames": m, "achieved_gbs": round(bytes_per_frame * m / (ms * 1e-3) / 1e9, 1),
                              "frac_of_hbm_peak": round(bytes_per_frame * m / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            line["side_kernels"] = side
        print(json.dumps(line), flush=True)
    if distributed:
        dist.barrier()
        if args.gather == "host" and rank == 0 and shm_path:
            os.unlink(shm_path)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
