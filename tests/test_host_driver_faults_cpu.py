"""What the folder-level host driver (csrc/encoder_host.c) does when the GPU side fails under it, and what it keeps
between two calls of one process.  The driver is linked with tests/host_driver_standin.c, whose m1v_* calls can be made
to fail by number (STANDIN_FAIL_CREATE / _ALLOC / _ENCODE, STANDIN_NOSPACE_ENCODE), and with
tests/host_driver_calls_main.c, which makes several calls from a script and prints each return value; both programs are
stand-alone, built with -fsanitize=address (leak check on) and -fsanitize=thread, and run as child processes.  Every case
runs under both, with EC504_HOST_THREADS=1 (the serial program) and 4.  Expected bytes are the oracle's over the folder in
directory order (tests/host_driver_cases.py); pictures are 176x144 or smaller, raw pixels, so nothing here needs the
reference tree except the last test, which compares the early exits with the reference binary where that survives them."""
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as orc
from host_driver_cases import JUNK, Folder, check_exact, check_prefix, check_prolog_only, frames_retired, raw_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["tests/host_driver_calls_main.c", "ec504_imageencoder_amd/csrc/encoder_host.c", "tests/host_driver_standin.c",
           "oracle/mpeg1_oracle.c"]
W, H, QF = 176, 144, 12
N_FRAMES, BATCH = 11, 2                                   # 6 chunks: 2 2 2 2 2 1
N_CHUNKS = (N_FRAMES + BATCH - 1) // BATCH

BOTH = pytest.mark.parametrize("san,threads", [("address", 1), ("address", 4), ("thread", 1), ("thread", 4)])


def _compile(out, san, sources):
    exe = str(out / f"calls_{san}")
    subprocess.run(["gcc", "-O1", "-g", "-w", f"-fsanitize={san}", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
                    *[os.path.join(ROOT, s) for s in sources], "-o", exe, "-lm", "-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("hostdrv_faults")
    return {san: _compile(out, san, SOURCES) for san in ("address", "thread")}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The input folders, written once and only read afterwards."""
    d = tmp_path_factory.mktemp("hostdrv_folders")
    w = {"a": Folder(d / "a", orc.synth_frames(N_FRAMES, W, H, seed=71)),
         "b": Folder(d / "b", orc.synth_frames(5, 128, H, seed=72)),                       # another geometry
         "rgba": Folder(d / "rgba", orc.synth_frames(5, W, H, seed=73, channels=4)),
         "grey": Folder(d / "grey", orc.synth_frames(3, W, H, seed=74, channels=3)[..., :1]),
         "mixed": Folder(d / "mixed", orc.synth_frames(7, W, H, seed=75)),
         "head": Folder(d / "head", orc.synth_frames(7, W, H, seed=76)),
         "hole": Folder(d / "hole", orc.synth_frames(7, W, H, seed=77)),
         "none": Folder(d / "none", orc.synth_frames(2, W, H, seed=78))}
    m = w["mixed"]
    rgba = np.concatenate([m.frames[m.order[4]], np.full((H, W, 1), 255, np.uint8)], axis=2)
    m.overwrite(4, raw_file(rgba))                       # a 4-channel file among 3-channel ones, met in the third chunk of 2
    for p in (0, 1):
        w["head"].overwrite(p, JUNK)                     # the first two files of the folder do not decode
        w["none"].overwrite(p, JUNK)                     # no file decodes
    for p in (2, 3):
        w["hole"].overwrite(p, JUNK)                     # with chunks of 2: the whole second chunk
    (d / "a_file").write_text("a regular file")
    w["file"] = str(d / "a_file")
    return w


class Run:
    """A script for tests/host_driver_calls_main.c, built line by line.  call() names a fresh output folder per call."""

    def __init__(self, exe, tmp_path, threads, **env):
        self.exe, self.tmp, self.lines, self.outs = exe, tmp_path, [], []
        self.env = {"EC504_HOST_THREADS": str(threads), **env}

    def add(self, *lines):
        self.lines += lines
        return self

    def call(self, images, qf=QF, region="full", bits=None, make_out=True):
        out = self.tmp / f"o{len(self.outs) + 1}"
        if make_out:
            out.mkdir()
        video = self.tmp / f"v{len(self.outs) + 1}.mpeg"
        self.outs.append((str(bits or out), str(video)))
        images = images.path if isinstance(images, Folder) else images
        self.lines.append(f"call {images} {bits or out} {video} {qf} {region}")
        return self

    def run(self):
        """-> [(return value, {create, alloc, encode}, the driver's messages)] per call.  The process itself must end with
        status 0: 66 is a ThreadSanitizer report, 67 an AddressSanitizer or leak report."""
        script = self.tmp / "script.txt"
        script.write_text("\n".join(self.lines) + "\n")
        env = {k: v for k, v in os.environ.items() if not k.startswith(("EC504_", "STANDIN_"))}
        env.update(TSAN_OPTIONS="exitcode=66 halt_on_error=1", ASAN_OPTIONS="exitcode=67 detect_leaks=1", **self.env)
        p = subprocess.run([self.exe, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-4000:])
        calls, text = [], []
        for line in p.stdout.decode(errors="replace").splitlines():
            if line.startswith("== call "):
                w = line.split()
                calls.append((int(w[4]), {k: int(v) for k, v in (x.split("=") for x in w[5:])}, "\n".join(text)))
                text = []
            else:
                text.append(line)
        assert len(calls) == len(self.outs), p.stdout.decode(errors="replace")[-4000:]
        return calls


THREE_LANES = {"EC504_DEVICES": "0,0,0", "EC504_BATCH": str(BATCH)}
# pinned buffers of one call with three lanes: an output buffer per lane, and N + 1 = 4 slots of pixels and of planes
ALLOCS_THREE_LANES = 3 + 4 * 2


@BOTH
def test_create_failure_on_the_first_lane(exes, world, tmp_path, san, threads):
    """m1v_create fails for lane 0 while the pool page-locks the buffers: -1, the error with the library's text, the video
    is its 27-byte prolog, no side file, nothing leaked; the next call of the process is exact."""
    a = world["a"]
    r = Run(exes[san], tmp_path, threads, **THREE_LANES)
    r.add("env STANDIN_FAIL_CREATE 1").call(a).add("env STANDIN_FAIL_CREATE").call(a)
    (rc1, n1, text1), (rc2, n2, text2) = r.run()
    assert rc1 == -1 and "Error: cannot set up the GPU encoder: injected failure (STANDIN_FAIL_CREATE 1)" in text1
    assert "Note:" not in text1 and n1["create"] == 1 and n1["encode"] == 0
    check_prolog_only(*r.outs[0])
    assert rc2 == 0 and "Note:" not in text2 and "Error" not in text2 and n2["create"] == 4
    check_exact(*r.outs[1], a.expect(QF, orc.MODE_FULL))


@BOTH
@pytest.mark.parametrize("k", [2, 3])
def test_create_failure_on_a_later_lane_falls_back_to_fewer_lanes(exes, world, tmp_path, san, threads, k):
    """m1v_create fails for lane k-1 of 3: a Note, the call goes on with k-1 lanes and its files are exact.  The kept
    context has k-1 lanes, so the next call, which wants 3, replaces it: all three creates (the counter says so), no Note,
    exact.  With the knob naming a create of the second call as well, that call falls back again and says so."""
    a = world["a"]
    want = a.expect(QF, orc.MODE_FULL)
    r = Run(exes[san], tmp_path, threads, **THREE_LANES)
    r.add(f"env STANDIN_FAIL_CREATE {k}").call(a).call(a)
    r.add("release", "reset", f"env STANDIN_FAIL_CREATE {k},{k + 2}").call(a).call(a)
    calls = r.run()
    note = f"Note: encoder {k} of 3 could not be created (injected failure (STANDIN_FAIL_CREATE {k})): continuing with {k - 1}"
    again = f"Note: encoder 2 of 3 could not be created (injected failure (STANDIN_FAIL_CREATE {k + 2})): continuing with 1"
    for (rc, n, text), out, notes, creates in zip(calls, r.outs, ([note], [], [note], [again]), (k, k + 3, k, k + 2)):
        assert rc == 0 and "Error" not in text, text
        assert [ln for ln in text.splitlines() if ln.startswith("Note:")] == notes
        assert n["create"] == creates
        check_exact(*out, want)


@BOTH
def test_every_pinned_allocation_failure(exes, world, tmp_path, san, threads):
    """A good call makes ALLOCS_THREE_LANES pinned allocations (counted); each of them in turn returns NULL in a call of
    its own: -1, the message, a prolog-only video, no side file, and the call after it is exact."""
    a = world["a"]
    want = a.expect(QF, orc.MODE_FULL)
    r = Run(exes[san], tmp_path, threads, **THREE_LANES)
    r.call(a)
    for k in range(1, ALLOCS_THREE_LANES + 1):
        r.add("release", "reset", f"env STANDIN_FAIL_ALLOC {k}").call(a).add("env STANDIN_FAIL_ALLOC").call(a)
    calls = r.run()
    assert calls[0][0] == 0 and calls[0][1]["alloc"] == ALLOCS_THREE_LANES, calls[0]
    check_exact(*r.outs[0], want)
    for k in range(1, ALLOCS_THREE_LANES + 1):
        (rc1, n1, text1), (rc2, n2, text2) = calls[2 * k - 1], calls[2 * k]
        assert rc1 == -1 and text1.count("Error: Memory allocation failed.") == 1, (k, text1)
        assert n1["alloc"] == ALLOCS_THREE_LANES and n1["encode"] == 0, (k, n1)
        check_prolog_only(*r.outs[2 * k - 1])
        assert rc2 == 0 and "Error" not in text2 and n2["alloc"] == 2 * ALLOCS_THREE_LANES, (k, text2, n2)
        check_exact(*r.outs[2 * k], want)


@BOTH
@pytest.mark.parametrize("devices,k", [("0", 1), ("0,0,0", 1), ("0,0,0", 3), ("0,0,0", N_CHUNKS)])
def test_encode_failure_leaves_a_prefix_of_whole_chunks(exes, world, tmp_path, san, threads, devices, k):
    """The k-th m1v_encode_planes_host of the process returns M1V_E_HIP: the first, a middle one with other lanes at work
    and .bit writers behind them, the last.  -1 and the error with the library's text.  Chunks are retired in order, so the
    video holds the prolog and the whole records of the chunks in front of the failed one and nothing of it or after it: a
    prefix of the good stream; image_<k>.bit exists, exact, for those frames and for no other.  The next call is exact.

    Which chunk the k-th encode is: on one thread (and with one lane) chunks reach the stand-in in order, so it is chunk
    k-1 (from 0).  With N lanes on pool threads chunk c starts once chunk c-N is retired, and chunk c+N not before c is, so
    between c-N+1 and c+N-1 encodes come in front of c's: c lies in k-N .. k+N-2."""
    a = world["a"]
    want = a.expect(QF, orc.MODE_FULL)
    lanes = len(devices.split(","))
    r = Run(exes[san], tmp_path, threads, EC504_DEVICES=devices, EC504_BATCH=str(BATCH))
    r.add(f"env STANDIN_FAIL_ENCODE {k}").call(a).add("env STANDIN_FAIL_ENCODE").call(a)
    (rc1, n1, text1), (rc2, n2, text2) = r.run()
    assert rc1 == -1 and text1.count(f"Error: GPU encode failed: injected failure (STANDIN_FAIL_ENCODE {k})") == 1, text1
    assert "Image processing finished." not in text1
    m = frames_retired(r.outs[0][1], want, BATCH)
    print(f"chunks retired in front of failed encode {k}: {m}")
    if threads == 1 or lanes == 1:
        assert m == k - 1
    else:
        assert max(0, k - lanes) <= m <= min(N_CHUNKS - 1, k + lanes - 2)
    check_prefix(*r.outs[0], want, min(m * BATCH, N_FRAMES))
    assert rc2 == 0 and "Error" not in text2 and n2["encode"] - n1["encode"] == N_CHUNKS
    check_exact(*r.outs[1], want)


@BOTH
@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_output_buffer_regrow_and_its_failures(exes, world, tmp_path, san, threads, devices):
    """M1V_E_NOSPACE from the 2nd encode, whatever the capacity: the lane's buffer is given back, the worst case allocated
    (one more pinned allocation) and the chunk done again: exact.  On one lane, where the redo is the next encode of the
    process: the regrow allocation fails, or the redo says NOSPACE again: -1 with the failure line, and the chunks in front
    (here chunk 0) stay, as after any failed encode.  The call after them is exact."""
    a = world["a"]
    want = a.expect(QF, orc.MODE_FULL)
    lanes = len(devices.split(","))
    allocs = lanes + min(lanes + 1, N_CHUNKS) * 2
    r = Run(exes[san], tmp_path, threads, EC504_DEVICES=devices, EC504_BATCH=str(BATCH))
    r.add("env STANDIN_NOSPACE_ENCODE 2").call(a)
    if lanes == 1:
        r.add("release", "reset", f"env STANDIN_FAIL_ALLOC {allocs + 1}").call(a)
        r.add("release", "reset", "env STANDIN_FAIL_ALLOC", "env STANDIN_NOSPACE_ENCODE 2,3").call(a)
        r.add("env STANDIN_NOSPACE_ENCODE").call(a)
    calls = r.run()
    rc, n, text = calls[0]
    assert rc == 0 and "Error" not in text and n == {"create": lanes, "alloc": allocs + 1, "encode": N_CHUNKS + 1}, (text, n)
    check_exact(*r.outs[0], want)
    if lanes == 1:
        for (rc, n, text), out, named in zip(calls[1:3], r.outs[1:3], (2, 3)):
            assert rc == -1 and n["alloc"] == allocs + 1, (text, n)
            assert text.count(f"Error: GPU encode failed: injected failure (STANDIN_NOSPACE_ENCODE {named})") == 1, text
            check_prefix(*out, want, BATCH)
        rc, n, text = calls[3]
        assert rc == 0 and "Error" not in text
        check_exact(*r.outs[3], want)


@BOTH
def test_the_kept_context_is_reused_or_replaced_as_the_next_call_needs(exes, world, tmp_path, san, threads):
    """One process, call after call with something else asked for each time; every call gives the bytes a fresh process
    gives (the oracle's), and the count of m1v_create calls shows whether the kept encoders were taken over (no create) or
    freed and replaced.  Ends with EC504_KEEP_ENCODER=0 and two releases in a row; ASan's leak check and a double free
    would end the process with status 67."""
    a, b = world["a"], world["b"]
    r = Run(exes[san], tmp_path, threads, **THREE_LANES)
    steps = []                                           # (folder, quality, mode, write_bit, creates expected in this call)
    full, strict = orc.MODE_FULL, orc.MODE_STRICT

    def step(folder, qf, region, mode, creates, *lines, write_bit=True):
        r.add(*lines).call(folder, qf, region)
        steps.append((folder, qf, mode, write_bit, creates))

    step(a, QF, "full", full, 3)
    step(a, QF, "full", full, 0)                               # the same again: taken over
    step(a, 30, "full", full, 3)                               # another quality
    step(b, 30, "full", full, 3)                               # another geometry (5 frames: 3 chunks)
    step(a, 30, "strict", strict, 3)                           # another region
    step(a, 30, "full", full, 3, "env EC504_BATCH 3")          # a larger batch does not fit the kept buffers
    step(a, 30, "full", full, 0, "env EC504_BATCH 1")          # a smaller one does (11 chunks, and the 4 slots kept are enough)
    step(a, 30, "full", full, 0, f"env EC504_BATCH {BATCH}")
    step(a, 30, "full", full, 0, "env EC504_WRITE_BIT 0", write_bit=False)   # no planes needed: the kept set (with planes) serves
    step(a, 30, "full", full, 3, "release", write_bit=False)                 # a set without planes ...
    step(a, 30, "full", full, 3, "env EC504_WRITE_BIT 1")                    # ... does not serve a call that writes them
    step(a, 30, "full", full, 1, "env EC504_DEVICES 0")                      # another lane count
    step(a, 30, "full", full, 2, "env EC504_DEVICES 0,0")
    step(a, 30, "env", full, 0, "env EC504_ENCODE_REGION full")              # mpeg_encode_procedure reads the region
    step(a, 30, "env", strict, 2, "env EC504_ENCODE_REGION strict")
    step(a, 30, "full", full, 2, "env EC504_KEEP_ENCODER 0")                 # the kept set does not match; the new one is not kept
    step(a, 30, "full", full, 2)
    r.add("release", "release", "env EC504_KEEP_ENCODER", "threads 2", "env EC504_HOST_THREADS")
    step(a, 30, "full", full, 2)                                             # encoder_set_host_threads sizes the pool
    r.add("release", "release")
    calls = r.run()
    creates = 0
    for i, ((rc, n, text), out, (folder, qf, mode, write_bit, made)) in enumerate(zip(calls, r.outs, steps)):
        assert rc == 0 and "Error" not in text and "Note" not in text, (i, text)
        assert n["create"] - creates == made, (i, n, made)
        creates = n["create"]
        check_exact(*out, folder.expect(qf, mode), write_bit)


@BOTH
def test_early_exits_and_odd_folders(exes, world, tmp_path, san, threads):
    """The exits in front of the frame loop and the folders that are not a plain run of equal pictures, one call each in
    one process (so each also starts from what the one before left).  See the assertions for what each must leave."""
    a = world["a"]
    r = Run(exes[san], tmp_path, threads, **THREE_LANES)
    r.add("noloader").call(a).add("loader")                                  # 0
    r.call(str(tmp_path / "absent"))                                         # 1
    r.call(world["file"])                                                    # 2
    r.call(world["none"])                                                    # 3
    r.call(world["grey"])                                                    # 4
    r.call(world["rgba"])                                                    # 5
    r.add("env EC504_BATCH 1").call(world["mixed"])                          # 6
    r.add("env EC504_BATCH 2").call(world["mixed"])                          # 7
    r.call(world["head"])                                                    # 8
    r.call(world["hole"])                                                    # 9
    r.call(a, bits=world["file"])                                            # 10
    r.call(a, make_out=False)                                                # 11
    calls = r.run()
    rcs = [c[0] for c in calls]
    text = [c[2] for c in calls]
    assert rcs == [-1, 0, -1, -1, -1, 0, -1, -1, 0, 0, 0, 0], rcs
    assert "Error: no image loader registered" in text[0]
    check_prolog_only(*r.outs[0])
    assert os.path.isdir(tmp_path / "absent") and f"Created directory for images: {tmp_path / 'absent'}" in text[1]
    check_prolog_only(*r.outs[1])
    assert "Error: Could not open images directory." in text[2]
    check_prolog_only(*r.outs[2])
    assert text[3].count("Error loading image") == 2 and "No images found in directory." in text[3]
    check_prolog_only(*r.outs[3])
    assert "Error: Image does not have correct color channels for RBG to YCbCr conversion." in text[4]
    check_prolog_only(*r.outs[4])
    assert calls[4][1]["create"] == 0                    # refused in front of the GPU side
    check_exact(*r.outs[5], world["rgba"].expect(QF, orc.MODE_FULL))
    for i in (6, 7):                                     # the end state of a dimension mismatch: what was written is taken back
        assert text[i].count("Error: Image channel counts do not match") == 1 and "dimensions" not in text[i]
        check_prolog_only(*r.outs[i])
    assert calls[6][1]["encode"] > calls[5][1]["encode"]     # (frames HAD been encoded when the odd file was met)
    assert text[8].count("Error loading image") == 2
    check_exact(*r.outs[8], world["head"].expect(QF, orc.MODE_FULL))
    assert text[9].count("Error loading image") == 2
    check_exact(*r.outs[9], world["hole"].expect(QF, orc.MODE_FULL))
    assert text[10].count("Error: Could not open bitstream file.") == N_FRAMES
    with open(r.outs[10][1], "rb") as fh:
        assert fh.read() == a.expect(QF, orc.MODE_FULL)[0]
    assert "Error" not in text[11] and f"Created directory for bitstreams: {r.outs[11][0]}" in text[11]
    check_exact(*r.outs[11], a.expect(QF, orc.MODE_FULL))


@pytest.mark.reference
def test_early_exits_agree_with_the_reference_binary(exes, world, tmp_path):
    """The same early exits through the reference's own driver (oracle/_ref/ref_encoder_strict), where it survives them:
    return value and the bytes of the video.  Not compared: a folder of pictures with fewer than 3 channels — the reference
    prints the same message and then crashes (it goes on into the conversion with the pointer it did not get) — and no
    loader, which the reference cannot be without."""
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_encoder_strict")
    if not os.path.exists(ref):
        if not os.path.exists("/root/reference/include/encoder.h"):
            pytest.skip("reference sources not present")
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref"], check=True)
    cases = [("absent", str(tmp_path / "absent_ours"), str(tmp_path / "absent_ref")), ("file", world["file"], world["file"]),
             ("none", world["none"].path, world["none"].path)]
    r = Run(exes["address"], tmp_path, 4)
    for _, ours, _ in cases:
        r.call(ours, region="strict")
    calls = r.run()
    for (name, _, theirs), (rc, _, text), (out, video) in zip(cases, calls, r.outs):
        (tmp_path / f"ref_{name}").mkdir()
        p = subprocess.run([ref, theirs, str(tmp_path / f"ref_{name}"), str(tmp_path / f"ref_{name}.mpeg"), str(QF)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == rc & 0xFF, (name, p.returncode, rc)
        with open(video, "rb") as f1, open(tmp_path / f"ref_{name}.mpeg", "rb") as f2:
            assert f1.read() == f2.read(), name
        assert os.listdir(tmp_path / f"ref_{name}") == [] and os.listdir(out) == []
        for line in ("Could not open images directory.", "No images found in directory.", "Created directory for images"):
            assert (line in text) == (line in p.stdout.decode(errors="replace")), (name, line)
    assert os.path.isdir(tmp_path / "absent_ours") and os.path.isdir(tmp_path / "absent_ref")
