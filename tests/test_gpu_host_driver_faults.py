"""The folder-level host driver (csrc/encoder_host.c) through the real library when the GPU side returns errors under it:
m1v_create failing for lane 0 and for a later lane (m1v_debug_fail_alloc), the first encode failing at each of its stages
(m1v_debug_fail_encode).  In process with a Python loader of raw-pixel files, as
tests/test_dropin.py::test_host_driver_with_a_custom_loader: 208x160, 8 frames, EC504_BATCH=3, expected bytes from the
oracle.  The hooks are injected error RETURNS in host code (EC504_DEBUG_HOOKS=1, set by conftest.py): nothing faults on
the device.  A failure in a LATER chunk is not tried here — the encode hook fails the next encode of the process, which
the lanes would race for; tests/test_host_driver_faults_cpu.py does that with the stand-in, by call number."""
import ctypes as C
import struct

import numpy as np
import pytest

from host_driver_cases import Folder, check_exact, check_prolog_only

pytestmark = pytest.mark.gpu

W, H, N, QF, BATCH = 208, 160, 8, 12, 3
E_HIP = -4


def _load(path):
    raw = open(path, "rb").read()
    if len(raw) < 12:
        return None
    w, h, c = struct.unpack_from("<iii", raw, 0)
    return np.frombuffer(raw, np.uint8, w * h * c, 12).reshape(h, w, c)


@pytest.fixture(scope="module")
def folder(tmp_path_factory, orc):
    return Folder(tmp_path_factory.mktemp("hostdrv_gpu") / "images", orc.synth_frames(N, W, H, seed=31))


@pytest.fixture
def driver(monkeypatch, tmp_path, capfd, folder, orc):
    """call() -> (return value, what the driver printed, bits folder, video path) of one mpeg_encode_procedure over the
    folder; the kept encoders of whatever ran before are released first, every hook is off afterwards."""
    from ec504_imageencoder_amd import _ffi, mpeg_encode_procedure, set_image_loader
    L = _ffi.lib()
    libc = C.CDLL(None)
    for name in ("EC504_DEVICE", "EC504_WRITE_BIT", "EC504_KEEP_ENCODER", "EC504_HOST_THREADS", "EC504_EXTRA_SLOTS", "EC504_ENCODE_REGION"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("EC504_BATCH", str(BATCH))
    set_image_loader(_load)
    L.encoder_release_cache()
    count = [0]

    def call():
        count[0] += 1
        bits, video = tmp_path / f"bits{count[0]}", tmp_path / f"v{count[0]}.mpeg"
        libc.fflush(None)                                # (what earlier calls of the process left in C's buffer is not this call's)
        capfd.readouterr()
        rc =mpeg_encode_procedure(str(folder.path), str(bits), str(video), QF, region="full")
        libc.fflush(None)
        return rc, capfd.readouterr().out, str(bits), str(video)

    try:
        yield call
    finally:
        L.m1v_debug_fail_alloc(0)
        L.m1v_debug_fail_encode(0)
        L.encoder_release_cache()


@pytest.fixture(scope="module")
def create_allocations():
    """A = the hooked allocations of one m1v_create at this geometry: m1v_debug_fail_alloc(nth) makes a plain create fail
    with M1V_E_HIP (and leave NULL behind) for nth = 1 .. A, and nth = A + 1 lets it through."""
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    enc = C.c_void_p()
    try:
        for nth in range(1, 65):
            L.m1v_debug_fail_alloc(nth)
            rc = L.m1v_create(C.byref(enc), 0, W, H, 3, QF, 1, BATCH)
            if rc == 0:
                assert enc.value
                return nth - 1
            assert rc == E_HIP and not enc.value, (nth, rc, L.m1v_last_error())
        raise AssertionError("m1v_create still fails at the 64th hooked allocation")
    finally:
        L.m1v_debug_fail_alloc(0)
        if enc.value:
            L.m1v_destroy(enc)


def test_create_failure_on_lane_0_and_on_lane_1(driver, create_allocations, folder, monkeypatch, orc):
    """EC504_DEVICES=0,0: two lanes, created one after the other on the calling thread while the pool page-locks the
    buffers.  Every hooked allocation of lane 0's create failing (nth = 1 .. A): -1, the error line, a 27-byte video, no
    side file.  nth = A + 1 is the first allocation of lane 1's create: a Note, return 0, and the files of one lane are the
    oracle's.  After each, the next call (both lanes again) is exact."""
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    A = create_allocations
    assert A >= 1
    want = folder.expect(QF, orc.MODE_FULL)
    monkeypatch.setenv("EC504_DEVICES", "0,0")
    for nth in range(1, A + 2):
        L.encoder_release_cache()
        L.m1v_debug_fail_alloc(nth)
        try:
            rc, text, bits, video = driver()
        finally:
            L.m1v_debug_fail_alloc(0)
        if nth <= A:
            assert rc == -1 and "Error: cannot set up the GPU encoder: allocation failed" in text and "Note:" not in text, (nth, text)
            check_prolog_only(bits, video)
        else:
            assert rc == 0 and "Error" not in text, (nth, text)
            assert "Note: encoder 2 of 2 could not be created (allocation failed" in text and "continuing with 1" in text, text
            check_exact(bits, video, want)
        rc, text, bits, video = driver()
        assert rc == 0 and "Error" not in text and "Note:" not in text, (nth, text)
        check_exact(bits, video, want)


@pytest.mark.parametrize("stage", [1, 2, 3])
def test_first_encode_failure_at_each_stage(driver, folder, monkeypatch, orc, stage):
    """EC504_DEVICES=0: one lane, so the hooked encode is chunk 0's.  It returns M1V_E_HIP at `stage`: -1, the error line
    with the library's text, a 27-byte video (nothing was retired), no side file; the next call of the process, on fresh
    encoders (a failed call keeps none), is exact."""
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    monkeypatch.setenv("EC504_DEVICES", "0")
    L.m1v_debug_fail_encode(stage)
    try:
        rc, text, bits, video = driver()
    finally:
        L.m1v_debug_fail_encode(0)
    assert rc == -1 and text.count("Error: GPU encode failed: injected failure (m1v_debug_fail_encode)") == 1, text
    check_prolog_only(bits, video)
    rc, text, bits, video = driver()
    assert rc == 0 and "Error" not in text, text
    check_exact(bits, video, folder.expect(QF, orc.MODE_FULL))
