"""The launch side of the library — TEST INFRASTRUCTURE ONLY (no tests in this module; tests/test_launch_side_cpu.py checks the
helpers with the oracle alone, tests/test_gpu_caller_stream.py and tests/test_gpu_grid_extents.py use them).

Three things, each a pure function of its arguments:

  the gate       device work of a chosen duration queued on one stream (torch.cuda._sleep where torch has it, else a repeated
                 large fill), calibrated with events on first use.  Work queued behind it on the same stream runs after it; work
                 that a mistaken launch put on any other stream runs at once, while the gate still holds the stream back.
  frame sets     per input kind a decoy and a real set of valid frames whose oracle records differ in every frame: the input
                 buffer holds the decoys until a copy queued behind the gate puts the real frames in their place.
  the divisor    div_magic and udiv of m1v_kernels.hip restated, the tile grid of a picture and the two batch lengths between which
                 the tile kernels' group divisor d = 8 * tiles_per_frame leaves the magic multiplication for the plain division
                 (n_max * d >= 2^32 with n_max = n_frames * tiles_per_frame)."""
import numpy as np

POISON = 0xA5
TILE_STRIPS, TILE_MB_ROWS = 8, 4        # kTileStrips, kTileMbRows (m1v_tiles.h): a tile is 128 x 64 pixels


# ---- the gate -------------------------------------------------------------------------------------------------------------------
class Gate:
    """gate(stream, ms) queues about `ms` milliseconds of device work on `stream`; measure(stream, fn) is the device time of what
    fn queues on `stream`, between two events.  One per process: the calibration is a measurement of this device."""

    def __init__(self, torch):
        self.torch = torch
        self._sleep = getattr(torch.cuda, "_sleep", None)
        self._fill = None if self._sleep else torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
        self.unit = 1 << 18 if self._sleep else 1       # cycles of one _sleep (calibrate() scales it), or one fill of 256 MiB
        self.ms_per_unit = None

    def _work(self, units):
        for _ in range(units):
            if self._sleep:
                self._sleep(self.unit)
            else:
                self._fill.fill_(1)

    def measure(self, stream, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def calibrate(self, stream):
        if self.ms_per_unit is None:
            self.measure(stream, lambda: self._work(1))
            if self._sleep:     # about 2 ms a launch, whatever the counter's frequency
                ms = max(self.measure(stream, lambda: self._work(1)), 1e-3)
                self.unit = max(1, min(int(self.unit * 2.0 / ms), (1 << 31) - 1))
            self.ms_per_unit = max(self.measure(stream, lambda: self._work(8)) / 8, 1e-3)
        return self.ms_per_unit

    def __call__(self, stream, ms):
        """Queue the gate; returns the milliseconds it was sized for (>= ms)."""
        per = self.calibrate(stream)
        units = int(ms / per) + 1
        with self.torch.cuda.stream(stream):
            self._work(units)
        return units * per


def gate_ms(call_ms):
    """The length a gate must have for a call that takes call_ms ungated: at least 20 ms and at least 20 times the call."""
    return max(20.0, 20.0 * call_ms)


# ---- decoy and real frame sets --------------------------------------------------------------------------------------------------
KINDS = ("packed3", "packed4", "surface3")      # surface3: pitched rows, the frames of a frame table


def _noise(seed, n, W, H, channels, amps):
    rng = np.random.default_rng(seed)
    out = np.empty((n, H, W, channels), np.uint8)
    for f in range(n):
        base = rng.integers(0, 256, (1, 1, channels))
        out[f] = np.clip(base + rng.integers(-amps[f % len(amps)], amps[f % len(amps)] + 1, (H, W, channels)), 0, 255).astype(np.uint8)
    return out


def frame_sets(kind, W, H, n):
    """(decoy, real): two arrays [n, H, W, C] of valid frames of `kind` with different pixels and different oracle records in
    every frame (records_differ asserts the latter).  Amplitudes near 256 keep AC codes in a record at quality 12."""
    assert kind in KINDS
    channels = 4 if kind == "packed4" else 3
    seed = 31000 + 10 * KINDS.index(kind)
    decoy = _noise(seed, n, W, H, channels, (250, 200, 256, 230))
    real = _noise(seed + 1, n, W, H, channels, (256, 240, 220, 252))
    return decoy, real


def records(orc, frames, first, qualities, mode):
    """The oracle's record of every frame at its own index and quality."""
    n, H, W, channels = frames.shape
    return [orc.encode_frame(frames[f], W, H, first + f, int(qualities[f]), mode, channels) for f in range(n)]


def records_differ(orc, decoy, real, first, quality, mode):
    """True when the oracle's records of the two sets differ in every frame (at the same index and quality)."""
    n = real.shape[0]
    a, b = records(orc, decoy, first, [quality] * n, mode), records(orc, real, first, [quality] * n, mode)
    return all(x != y for x, y in zip(a, b))


# ---- the divisor switch ---------------------------------------------------------------------------------------------------------
def div_magic(d, n_max):
    """(d, m) as div_magic of m1v_kernels.hip gives them: m = floor(2^32 / d) + 1 while n_max * d < 2^32 and d >= 2, else 0."""
    return d, ((1 << 32) // d + 1) & 0xFFFFFFFF if d >= 2 and n_max * d < (1 << 32) else 0


def udiv(n, dm):
    """udiv of m1v_kernels.hip: the high half of the 32 x 32-bit product n * m, or the plain division where m = 0."""
    d, m = dm
    return (n * m) >> 32 if m else n // d


def tile_grid(W, H):
    """(tile_cols, tile_rows) of a W x H picture in mode "full" (TileGrid of m1v_kernels.hip)."""
    strips, mb_rows = W // 16, H // 16
    return -(-strips // TILE_STRIPS), -(-mb_rows // TILE_MB_ROWS)


def switch_batches(tile_cols, tile_rows):
    """(last, next): the longest batch whose group divisor is still the magic one, n * 8 * tpf^2 < 2^32, and the one after it,
    the first on the plain division."""
    tpf = tile_cols * tile_rows
    last = ((1 << 32) - 1) // (8 * tpf * tpf)
    assert last * 8 * tpf * tpf < (1 << 32) <= (last + 1) * 8 * tpf * tpf
    return last, last + 1


def launch_divisors(tile_cols, tile_rows, n_frames):
    """The divisor pairs fill_tile_grid gives a launch over n_frames: (div_group, div_frame, div_cols) and the launch's units."""
    tpf = tile_cols * tile_rows
    units = n_frames * tpf
    return div_magic(8 * tpf, units), div_magic(tpf, units), div_magic(tile_cols, tpf), units


def frame_unit_of(b, n_frames, group, per_frame):
    """frame_unit_of of m1v_kernels.hip: (frame, unit) of workgroup b."""
    full = n_frames // 8
    if b < full * group[0]:
        gq = udiv(b, group)
        r = b - gq * group[0]
        return gq * 8 + (r & 7), r >> 3
    t = b - full * group[0]
    q = udiv(t, per_frame)
    return full * 8 + q, t - q * per_frame[0]


def rolled_colours(k, channels=3):
    """Frame k of the convert test: all 2^24 colours in index order, rolled by k pixels, as [4096, 4096, channels] (a 4th byte
    is the colour's low byte inverted)."""
    c = np.roll(np.arange(1 << 24, dtype=np.uint32), k)
    px = np.empty((1 << 24, channels), np.uint8)
    px[:, 0], px[:, 1], px[:, 2] = c >> 16, (c >> 8) & 255, c & 255
    if channels == 4:
        px[:, 3] = ~px[:, 2]
    return px.reshape(4096, 4096, channels)
