"""Content of tests/test_gpu_luma_denormal.py, built on the host (tests/test_luma_denormal_cpu.py checks what it claims).

The luma waves of the tile kernels take a colour byte where it lies in its dword (csrc/m1v_kernels.hip, luma_sums_denormal), so
what a colour meets depends on the byte phase of its pixel: pixel x of a picture row starts at byte 3x of the row, and rows are
a multiple of four pixels wide here, so the phase is (3 * i) & 3 for the pixel's index i in the frame."""
import numpy as np

SIZES = [(128, 64), (144, 80), (176, 208)]  # one whole tile; a partial last tile column and row; tests/test_gpu_hard_content.py's
QUALITIES = [12, 92]                        # the byte-staged and the wide kernel
CONTENTS = ["ties", "extremes", "noise"]
_cache = {}


def luma_tie_colours():
    """uint8 [k, 3]: the colours whose Y lies within 2.6e-4 above or 2.5e-4 below an integer, in exact integer arithmetic (the
    coefficients are multiples of 1e-6).  The kernel flags a sum whose fraction is below 10 / 32768 after adding 1.5e-4, with an
    error below 1e-4 (component_t): a subset of these."""
    if "ties" not in _cache:
        r, g, b = (x.reshape(-1).astype(np.int64) for x in np.meshgrid(*[np.arange(256)] * 3, indexing="ij"))
        f = (299000 * r + 587000 * g + 114000 * b) % 1000000
        _cache["ties"] = np.stack([r, g, b], 1).astype(np.uint8)[(f < 260) | (f > 999750)]
    return _cache["ties"]


def tie_pixels():
    """uint8 [m, 3], m a multiple of 4: the tie colours four times; copy k starts k pixels behind a multiple of four, so colour
    i of it lies at phase (i + k) & 3 of any frame sequence the pixels are cut into."""
    ties, grey = luma_tie_colours(), np.full((1, 3), 128, np.uint8)
    parts = []
    for k in range(4):
        parts += [np.repeat(grey, k, 0), ties, np.repeat(grey, (-(k + len(ties))) % 4, 0)]
    return np.concatenate(parts)


def content(name, W, H):
    """uint8 [n, H, W, 3], read-only.  "ties": as many frames as hold tie_pixels() (the last one filled with its first pixels
    again); "extremes": two frames of bytes 0 and 255 only; "noise": two frames of uniform bytes."""
    key = (name, W, H)
    if key not in _cache:
        assert W % 4 == 0
        if name == "ties":
            px = tie_pixels()
            n = -(-len(px) // (W * H))
            frames = np.resize(px, (n * W * H, 3)).reshape(n, H, W, 3)
        else:
            rng = np.random.default_rng(2900 + W + {"extremes": 0, "noise": 1}[name])
            frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
            if name == "extremes":
                frames = ((frames >> 7) * 255).astype(np.uint8)
        frames = np.ascontiguousarray(frames)
        frames.setflags(write=False)
        _cache[key] = frames
    return _cache[key]
