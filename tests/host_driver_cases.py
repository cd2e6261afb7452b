"""Folders of raw-pixel "*.jpg" files for the folder-level host driver (csrc/encoder_host.c), what the oracle expects of
them, and checks of what a call left on disk.  Shared by tests/test_host_driver_faults_cpu.py (the driver linked with
tests/host_driver_standin.c, as child processes under sanitizers) and tests/test_gpu_host_driver_faults.py (the real
library, in process).  A file holds int32 W, H, C and then the pixels, the format of tests/raw_loader_main.c."""
import os
import struct

import numpy as np

import oracle_ffi as orc

PROLOG_BYTES = 27
JUNK = b"\xff\xd8 junk"                           # shorter than the 12-byte header: every raw loader refuses it


def raw_file(frame):
    h, w, c = frame.shape
    return struct.pack("<iii", w, h, c) + np.ascontiguousarray(frame, np.uint8).tobytes()


class Folder:
    """`frames` (uint8 [n, H, W, C]) written as f00.jpg, f01.jpg, ... into `path`; `order` = their indices in raw directory
    order, which is the order of the frame records.  overwrite() replaces the file at a POSITION of that order (the
    directory entry stays where it is, so the order holds)."""

    def __init__(self, path, frames):
        self.path, self.frames = str(path), frames
        os.makedirs(self.path)
        for i, f in enumerate(frames):
            with open(os.path.join(self.path, f"f{i:02d}.jpg"), "wb") as fh:
                fh.write(raw_file(f))
        with open(os.path.join(self.path, "notes.txt"), "w") as fh:
            fh.write("not an image")
        self.order = [int(e.name[1:3]) for e in os.scandir(self.path) if ".jpg" in e.name]
        self.gone = set()                          # positions whose file no longer decodes
        self._expect = {}

    def overwrite(self, position, content):
        with open(os.path.join(self.path, f"f{self.order[position]:02d}.jpg"), "wb") as fh:
            fh.write(content)
        self.gone.add(position)
        self._expect.clear()

    def loaded(self):
        """The frames the driver loads, in the order of their records."""
        return np.stack([self.frames[i] for p, i in enumerate(self.order) if p not in self.gone])

    def expect(self, qf, mode):
        """(video bytes, record size of each frame, image_<k>.bit bytes of each frame) from the oracle, computed once."""
        key = (qf, mode)
        if key not in self._expect:
            fr = self.loaded()
            n, h, w, c = fr.shape
            body, sizes = orc.encode_frames(fr, n, w, h, 0, qf, mode, channels=c)
            bits = [struct.pack("<ii", w, h) + b"".join(p.tobytes() for p in orc.convert(f, c)) for f in fr]
            self._expect[key] = (orc.file_prolog() + body, [int(s) for s in sizes], bits)
        return self._expect[key]


def bit_files(folder):
    return sorted(n for n in os.listdir(folder) if n.endswith(".bit"))


def check_prefix(out_dir, video_path, want, n_frames):
    """The call left exactly the first n_frames frame records behind the prolog, and image_1.bit .. image_<n_frames>.bit
    with the oracle's planes, and no other side file.  `want` = Folder.expect(...)."""
    video, sizes, bits = want
    with open(video_path, "rb") as fh:
        got = fh.read()
    assert len(got) == PROLOG_BYTES + sum(sizes[:n_frames]), (len(got), n_frames)
    assert got == video[:len(got)]
    assert bit_files(out_dir) == sorted(f"image_{k}.bit" for k in range(1, n_frames + 1))
    for k in range(1, n_frames + 1):
        with open(os.path.join(out_dir, f"image_{k}.bit"), "rb") as fh:
            assert fh.read() == bits[k - 1], k


def check_exact(out_dir, video_path, want, write_bit=True):
    """The whole good stream and every side file (or none of them, with EC504_WRITE_BIT=0)."""
    video, sizes, _ = want
    if write_bit:
        check_prefix(out_dir, video_path, want, len(sizes))
    else:
        with open(video_path, "rb") as fh:
            assert fh.read() == video
        assert bit_files(out_dir) == []


def check_prolog_only(out_dir, video_path):
    with open(video_path, "rb") as fh:
        assert fh.read() == orc.file_prolog()
    assert not os.path.isdir(out_dir) or bit_files(out_dir) == []


def frames_retired(video_path, want, chunk):
    """How many whole chunks of `chunk` frames the video holds behind its prolog; an assertion fails if it does not end
    on a chunk's edge."""
    sizes = want[1]
    size = os.path.getsize(video_path)
    edges = [PROLOG_BYTES + sum(sizes[:min(m * chunk, len(sizes))]) for m in range((len(sizes) + chunk - 1) // chunk + 1)]
    assert size in edges, (size, edges)
    return edges.index(size)
